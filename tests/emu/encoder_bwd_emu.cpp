// The encoder's backward pass on the CPU fiber emulator (TEST INFRASTRUCTURE ONLY; see hip_emu.h): the real kernels of
// csrc/kernels/encoder_bwd_f32.h behind the real host code of csrc/aae_encoder_bwd_impl.h, so that the library built here exports the
// same entry points as libaae_hip.so (aae_conv_backward, aae_linear_backward, their workspace twins, the labels) on host pointers.
// Built by tests/test_emu_encoder_bwd.py with the compiler and flags of the Makefile here, together with hip_emu.cpp.
#include "hip_emu.h"

// the emulator runs the blocks of a launch one after the other, every thread of a block as a fiber of this process: a block's static
// LDS arrays are function-level statics
#define __shared__ static
// (the whole-chain call walks an aae_encoder handle, which lives in the library's main translation unit)
#define AAE_ENCODER_BWD_LAYERS_ONLY

#include <string>

#include "../../augmentedautoencoder_amd/csrc/aae_encoder_bwd_impl.h"

namespace {
thread_local std::string t_error;
}
namespace aae_host {
void set_last_error(const char* msg) { t_error = msg ? msg : ""; }
}
extern "C" const char* aae_last_error(void) { return t_error.c_str(); }
