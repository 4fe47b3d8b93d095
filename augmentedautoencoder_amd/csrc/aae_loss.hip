// Sixth translation unit of libaae_hip.so: the loss kernels (kernels/loss_core.h, kernels/recon_loss.h) and their C ABI
// (aae_recon_loss, aae_latent_reg_loss), compiled beside the other five and linked with them (__graft_entry__.build()).
#include <hip/hip_runtime.h>

#define AAE_LAUNCH(kernel, grid, block, smem, stream, ...) \
    hipLaunchKernelGGL(kernel, (grid), (block), (smem), (stream), __VA_ARGS__)

#include "aae_loss_impl.h"
