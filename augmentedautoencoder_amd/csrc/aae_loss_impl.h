// Host side of the loss kernels (kernels/recon_loss.h): the argument checks, the choice of the kernel form by image size and the
// launches behind aae_recon_loss and aae_latent_reg_loss (include/aae_hip.h).  Part of aae_loss.hip.
#pragma once

#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>

#include "../../include/aae_hip.h"
#include "kernels/recon_loss.h"

namespace aae_host {
void set_last_error(const char* msg);          // aae_host_types.h: the thread's aae_last_error() text lives in aae_hip.hip
}

namespace aae_loss {

static_assert(AAE_LOSS_L2 == LOSS_L2 && AAE_LOSS_L1 == LOSS_L1, "include/aae_hip.h and loss_core.h disagree");
static_assert(AAE_LOSS_MAX_N == LOSS_MAX_N && AAE_LOSS_MAX_BATCH == LOSS_MAX_BATCH, "include/aae_hip.h and recon_loss.h disagree");

constexpr size_t LOSS_WS_ALIGN = 16;

static int lfail(int code, const char* fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    aae_host::set_last_error(buf);
    return code;
}

static inline size_t workspace_bytes(int B) { return (((size_t)(B + 1) * sizeof(float)) + LOSS_WS_ALIGN - 1) / LOSS_WS_ALIGN * LOSS_WS_ALIGN; }

template <int KIND, int HIST>
static void launch_recon_kind(const LossArgs& a, int B, hipStream_t stream) {
    if (a.n <= 1 * LOSS_BLOCK) AAE_LAUNCH((recon_loss_kernel<1, KIND, HIST>), dim3(B), dim3(LOSS_BLOCK), 0, stream, a);
    else if (a.n <= 8 * LOSS_BLOCK) AAE_LAUNCH((recon_loss_kernel<8, KIND, HIST>), dim3(B), dim3(LOSS_BLOCK), 0, stream, a);
    else if (a.n <= LOSS_RESIDENT_ROWS * LOSS_BLOCK) AAE_LAUNCH((recon_loss_kernel<LOSS_RESIDENT_ROWS, KIND, HIST>), dim3(B), dim3(LOSS_BLOCK), 0, stream, a);
    else AAE_LAUNCH((recon_loss_kernel<0, KIND, HIST>), dim3(B), dim3(LOSS_BLOCK), 0, stream, a);
}

template <int HIST>
static void launch_recon(const LossArgs& a, int kind, int B, hipStream_t stream) {
    if (kind == LOSS_L1) launch_recon_kind<LOSS_L1, HIST>(a, B, stream);
    else launch_recon_kind<LOSS_L2, HIST>(a, B, stream);
}

}  // namespace aae_loss

extern "C" {

size_t aae_recon_loss_workspace_bytes(int B, int n) {
    if (B < 1 || n < 1 || B > AAE_LOSS_MAX_BATCH || n > AAE_LOSS_MAX_N) return 0;
    return aae_loss::workspace_bytes(B);
}

int aae_recon_loss(const aae_recon_loss_desc* d, const float* x, const float* target, float* loss, float* per_image, float* dx, void* workspace,
                   size_t ws_bytes, void* stream) {
    using namespace aae_loss;
    const char* who = "aae_recon_loss";
    if (!d || !x || !target || !loss || !workspace) return lfail(AAE_ERR_INVALID, "%s: null argument (desc, x, target, loss and workspace are required)", who);
    if (d->B < 1 || d->n < 1 || d->bootstrap_ratio < 1) return lfail(AAE_ERR_INVALID, "%s: B = %d, n = %d, bootstrap_ratio = %d", who, d->B, d->n, d->bootstrap_ratio);
    if (d->kind != AAE_LOSS_L2 && d->kind != AAE_LOSS_L1) return lfail(AAE_ERR_INVALID, "%s: kind %d is neither AAE_LOSS_L2 nor AAE_LOSS_L1", who, d->kind);
    const int k = d->n / d->bootstrap_ratio;
    if (k < 1) return lfail(AAE_ERR_INVALID, "%s: bootstrap_ratio %d selects n / ratio = 0 of %d elements", who, d->bootstrap_ratio, d->n);
    if (d->B > AAE_LOSS_MAX_BATCH || d->n > AAE_LOSS_MAX_N)
        return lfail(AAE_ERR_UNSUPPORTED, "%s: B = %d, n = %d over the limits of %d images and %d elements per image", who, d->B, d->n, AAE_LOSS_MAX_BATCH, AAE_LOSS_MAX_N);
    const size_t need = workspace_bytes(d->B);
    if (ws_bytes < need || ((uintptr_t)workspace & (LOSS_WS_ALIGN - 1)))
        return lfail(AAE_ERR_WORKSPACE, "%s: workspace %p of %zu bytes; %zu bytes, %zu-byte aligned, are needed", who, workspace, ws_bytes, need, LOSS_WS_ALIGN);

    LossArgs a;
    a.x = x; a.t = target; a.dx = dx; a.per_image = per_image; a.means = (float*)workspace; a.sink = a.means + d->B;
    a.n = d->n; a.k = k; a.select_all = k == d->n;
    a.scale = (float)(1.0 / ((double)d->B * (double)k));
    int hist = HIST_LANE;
#ifdef AAE_EXPERIMENTS
    if (const char* env = getenv("AAE_LOSS_HIST")) hist = atoi(env);          // 1: a histogram per wave, 2: one shared histogram (the measured losers)
    if (hist == HIST_WAVE) launch_recon<HIST_WAVE>(a, d->kind, d->B, (hipStream_t)stream);
    else if (hist == HIST_SHARED) launch_recon<HIST_SHARED>(a, d->kind, d->B, (hipStream_t)stream);
    else
#endif
        launch_recon<HIST_LANE>(a, d->kind, d->B, (hipStream_t)stream);
    (void)hist;
    AAE_LAUNCH(recon_loss_finish_kernel, dim3(1), dim3(LOSS_BLOCK), 0, (hipStream_t)stream, (const float*)a.means, d->B, loss);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return lfail(AAE_ERR_RUNTIME, "%s: launch failed: %s", who, hipGetErrorString(e));
    return AAE_OK;
}

int aae_latent_reg_loss(const float* z, int B, int J, float* loss, float* dz, void* stream) {
    using namespace aae_loss;
    const char* who = "aae_latent_reg_loss";
    if (!z || !loss) return lfail(AAE_ERR_INVALID, "%s: null argument (z and loss are required)", who);
    if (B < 1 || J < 1) return lfail(AAE_ERR_INVALID, "%s: B = %d, J = %d", who, B, J);
    if (B > AAE_LOSS_MAX_BATCH || J > AAE_LOSS_MAX_LATENT)
        return lfail(AAE_ERR_UNSUPPORTED, "%s: B = %d, J = %d over the limits of %d rows and %d columns", who, B, J, AAE_LOSS_MAX_BATCH, AAE_LOSS_MAX_LATENT);
    AAE_LAUNCH(latent_reg_kernel, dim3(1), dim3(LOSS_BLOCK), 0, (hipStream_t)stream, z, B, J, loss, dz);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return lfail(AAE_ERR_RUNTIME, "%s: launch failed: %s", who, hipGetErrorString(e));
    return AAE_OK;
}

}  // extern "C"
