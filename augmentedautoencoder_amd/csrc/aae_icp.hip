// Fourth translation unit of libaae_hip.so: the depth ICP refinement (kernels/icp_core.h, kernels/icp_kernels.h) and its C ABI
// (aae_icp_*), compiled beside aae_hip.hip, aae_wino.hip and aae_render.hip and linked with them (__graft_entry__.build()).
#include <hip/hip_runtime.h>

#define AAE_LAUNCH(kernel, grid, block, smem, stream, ...) \
    hipLaunchKernelGGL(kernel, (grid), (block), (smem), (stream), __VA_ARGS__)

#include "aae_icp_impl.h"
