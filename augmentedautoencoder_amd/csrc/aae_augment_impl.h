// Host side of the training-batch kernel (kernels/augment_batch.h): the shape checks and the one launch behind aae_augment_batch
// (include/aae_hip.h).  Part of aae_augment.hip.
#pragma once

#include <stdarg.h>
#include <stdio.h>

#include <atomic>

#include "../../include/aae_hip.h"
#include "kernels/augment_batch.h"

namespace aae_host {
void set_last_error(const char* msg);          // aae_host_types.h: the thread's aae_last_error() text lives in aae_hip.hip
}

namespace aae_augment {

static_assert(sizeof(aae_augment_op) == sizeof(AugOp) && sizeof(AugOp) == 32, "aae_augment_op is the kernel's AugOp");
static_assert(AAE_AUGMENT_MAX_OPS == AUG_MAX_OPS && AAE_AUGMENT_MAX_BLUR_K == AUG_MAX_BLUR_K, "include/aae_hip.h and augment_core.h disagree");
static_assert(AAE_AUGMENT_AFFINE == AUG_AFFINE && AAE_AUGMENT_DROPOUT == AUG_DROPOUT && AAE_AUGMENT_BLUR == AUG_BLUR && AAE_AUGMENT_ADD == AUG_ADD &&
              AAE_AUGMENT_INVERT == AUG_INVERT && AAE_AUGMENT_MULTIPLY == AUG_MULTIPLY && AAE_AUGMENT_CONTRAST == AUG_CONTRAST, "op codes");

// the workgroup's LDS on gfx950: two image buffers must fit
constexpr size_t AUG_LDS_BYTES = 160 * 1024;
constexpr size_t AUG_MAX_IMAGE_BYTES = AUG_LDS_BYTES / 2;
constexpr int AUG_MAX_DIM = 4095;             // aug_divmod's divisor range
constexpr int AUG_MAX_BATCH = 1 << 20;

static int afail(int code, const char* fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    aae_host::set_last_error(buf);
    return code;
}

static inline bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

// The kernel's dynamic-LDS ceiling, raised to the whole 160 KiB once per device and never lowered, so two host threads that launch
// different image sizes cannot take the ceiling away from each other between the attribute call and the launch.
static int raise_lds_ceiling(const char* who) {
    static std::atomic<uint64_t> done{0};
    int dev = 0;
    hipError_t e = hipGetDevice(&dev);
    if (e != hipSuccess) return afail(AAE_ERR_RUNTIME, "%s: hipGetDevice: %s", who, hipGetErrorString(e));
    const uint64_t bit = dev >= 0 && dev < 64 ? 1ull << dev : 0;
    if (bit && (done.load(std::memory_order_acquire) & bit)) return AAE_OK;
    e = hipFuncSetAttribute((const void*)augment_batch_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)AUG_LDS_BYTES);
    if (e != hipSuccess) return afail(AAE_ERR_RUNTIME, "%s: hipFuncSetAttribute(%zu bytes of LDS): %s", who, AUG_LDS_BYTES, hipGetErrorString(e));
    done.fetch_or(bit, std::memory_order_release);
    return AAE_OK;
}

}  // namespace aae_augment

extern "C" {

size_t aae_augment_max_image_bytes(void) { return aae_augment::AUG_MAX_IMAGE_BYTES; }

int aae_augment_batch(const aae_augment_shape* s, const void* train_x, const void* mask_x, const void* train_y, const void* bg,
                      const int32_t* train_idx, const int32_t* bg_idx, const int32_t* n_ops, const aae_augment_op* ops,
                      const uint32_t* aux, void* batch_x_u8, float* batch_x_f32, float* batch_y_f32, void* stream) {
    using namespace aae_augment;
    const char* who = "aae_augment_batch";
    if (!s || !train_x || !mask_x || !train_y || !bg || !train_idx || !bg_idx || !n_ops || !ops) return afail(AAE_ERR_INVALID, "%s: null argument", who);
    if (s->aux_words < 0 || (s->aux_words > 0 && !aux)) return afail(AAE_ERR_INVALID, "%s: %d aux words, aux = %p", who, s->aux_words, (const void*)aux);
    if (s->N < 1 || s->M < 1 || s->B < 1 || s->B > AUG_MAX_BATCH) return afail(AAE_ERR_INVALID, "%s: N = %d, M = %d, batch = %d", who, s->N, s->M, s->B);
    if (s->H < 1 || s->W < 1 || s->H > AUG_MAX_DIM || s->W > AUG_MAX_DIM || s->C < 1 || s->C > AUG_MAX_CHANNELS)
        return afail(AAE_ERR_UNSUPPORTED, "%s: image %dx%dx%d outside [1,%d] x [1,%d] x [1,%d]", who, s->H, s->W, s->C, AUG_MAX_DIM, AUG_MAX_DIM, AUG_MAX_CHANNELS);
    const size_t total = (size_t)s->H * s->W * s->C;
    if (total > AUG_MAX_IMAGE_BYTES)
        return afail(AAE_ERR_UNSUPPORTED, "%s: an image of %dx%dx%d = %zu bytes is over the limit of %zu bytes (two image buffers in %zu bytes of LDS)", who,
                     s->H, s->W, s->C, total, AUG_MAX_IMAGE_BYTES, AUG_LDS_BYTES);
    if (!batch_x_u8 && !batch_x_f32 && !batch_y_f32) return AAE_OK;

    AugDims a;
    a.N = s->N; a.M = s->M; a.H = s->H; a.W = s->W; a.C = s->C; a.aux_words = s->aux_words;
    a.rcp_C = 1.0f / (float)s->C; a.rcp_W = 1.0f / (float)s->W;
    a.vec4 = total % 4 == 0 && aligned16(train_x) && aligned16(train_y) && aligned16(bg) && aligned16(batch_x_u8) && aligned16(batch_x_f32) && aligned16(batch_y_f32);
    const size_t smem = 2 * ((total + 3) / 4) * sizeof(uint32_t);
    if (int rc = raise_lds_ceiling(who)) return rc;
    AAE_LAUNCH(augment_batch_kernel, dim3(s->B), dim3(AUG_BLOCK), smem, (hipStream_t)stream, (const uint8_t*)train_x, (const uint8_t*)mask_x,
               (const uint8_t*)train_y, (const uint8_t*)bg, train_idx, bg_idx, n_ops, reinterpret_cast<const AugOp*>(ops), aux, (uint8_t*)batch_x_u8,
               batch_x_f32, batch_y_f32, a);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return afail(AAE_ERR_RUNTIME, "%s: launch failed: %s", who, hipGetErrorString(e));
    return AAE_OK;
}

}  // extern "C"
