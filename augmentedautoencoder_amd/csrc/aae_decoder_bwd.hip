// Seventh translation unit of libaae_hip.so: the decoder's backward pass (kernels/decoder_bwd_core.h, kernels/decoder_bwd_f32.h) and
// its C ABI (aae_upconv_backward, aae_dense_backward), compiled beside the other six and linked with them (__graft_entry__.build()).
#include <hip/hip_runtime.h>

#define AAE_LAUNCH(kernel, grid, block, smem, stream, ...) \
    hipLaunchKernelGGL(kernel, (grid), (block), (smem), (stream), __VA_ARGS__)

#include "device_intrinsics.h"
#include "aae_decoder_bwd_impl.h"
