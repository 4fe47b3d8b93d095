// Third translation unit of libaae_hip.so: the mesh rasteriser (kernels/render_core.h, kernels/render_raster.h) and its C ABI
// (aae_mesh_*, aae_render_*), compiled beside aae_hip.hip and aae_wino.hip and linked with them (__graft_entry__.build()).
#include <hip/hip_runtime.h>

#define AAE_LAUNCH(kernel, grid, block, smem, stream, ...) \
    hipLaunchKernelGGL(kernel, (grid), (block), (smem), (stream), __VA_ARGS__)

#include "aae_render_impl.h"
