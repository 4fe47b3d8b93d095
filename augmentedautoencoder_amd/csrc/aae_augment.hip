// Fifth translation unit of libaae_hip.so: the training-batch kernel (kernels/augment_core.h, kernels/augment_batch.h) and its C ABI
// (aae_augment_*), compiled beside the other four and linked with them (__graft_entry__.build()).
#include <hip/hip_runtime.h>

#define AAE_LAUNCH(kernel, grid, block, smem, stream, ...) \
    hipLaunchKernelGGL(kernel, (grid), (block), (smem), (stream), __VA_ARGS__)

#include "aae_augment_impl.h"
