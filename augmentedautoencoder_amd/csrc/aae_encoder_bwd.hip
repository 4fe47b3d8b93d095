// Eighth translation unit of libaae_hip.so: the encoder's backward pass (kernels/encoder_bwd_core.h, kernels/encoder_bwd_f32.h) and
// its C ABI (aae_conv_backward, aae_linear_backward, aae_encoder_backward), compiled beside the other seven and linked with them
// (__graft_entry__.build()).
#include <hip/hip_runtime.h>

#define AAE_LAUNCH(kernel, grid, block, smem, stream, ...) \
    hipLaunchKernelGGL(kernel, (grid), (block), (smem), (stream), __VA_ARGS__)

#include "device_intrinsics.h"
#include "aae_encoder_bwd_impl.h"
