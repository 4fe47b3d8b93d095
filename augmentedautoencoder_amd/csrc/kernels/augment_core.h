// The per-pixel arithmetic of Dataset.batch (the reference's auto_pose/ae/dataset.py:456-495): the background composite, the
// seven augmenters of the cfg template's [Augmentation] CODE chain restated from imgaug 0.4.0's documentation (DESIGN section 4,
// table "imgaug 0.4.0 semantics assumed") and the /255 conversion.  Plain functions that compile for the device (augment_batch.h)
// and for the host (tests/native/augment_host.cpp drives them against the NumPy float64 restatement in tests/augment_reference.py).
//
// Images are uint8 between ops.  Every real result becomes uint8 by aug_round_u8: clip to [0,255], then round half to even.
// Image accessors are callables  src(y, x, c) -> uint8_t.
#pragma once

#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define AUG_HD __host__ __device__ __forceinline__
#define AUG_UNROLL _Pragma("unroll")
#else
#include <math.h>
#define AUG_HD static inline
#define AUG_UNROLL
#endif

namespace aae_augment {

enum AugCode : int32_t {
    AUG_AFFINE = 1,      // f[0] = 1 / scale
    AUG_DROPOUT = 2,     // i[0] mask bits, i[1] row table (cell row * w_s), i[2] column table: word offsets into the aux pool; i[3] = h_s * w_s when per channel, else 0
    AUG_BLUR = 3,        // i[0] = k (odd, 1 ... AUG_MAX_BLUR_K), i[1] = word offset of k fp32 weights in the aux pool
    AUG_ADD = 4,         // f[c] = the integer added to channel c
    AUG_INVERT = 5,      // i[c] != 0: channel c is inverted
    AUG_MULTIPLY = 6,    // f[c] = factor of channel c
    AUG_CONTRAST = 7,    // f[c] = alpha of channel c
};

constexpr int AUG_MAX_OPS = 16;
constexpr int AUG_MAX_BLUR_K = 15;
constexpr int AUG_MAX_CHANNELS = 3;

// one op of an image's program: 32 bytes, the same for every lane of the image's workgroup (augment_batch.h keeps it in SGPRs)
struct AugOp {
    int32_t code;
    int32_t i[4];
    float f[3];
};

AUG_HD uint8_t aug_round_u8(float r) {
    r = r >= 0.0f ? r : 0.0f;               // a NaN (a hostile factor) becomes 0 here, before the cast
    r = r > 255.0f ? 255.0f : r;
    return (uint8_t)(int)rintf(r);          // round half to even (the default rounding mode on the host, v_rndne_f32 on the device)
}

// np.float32(v / 255.): for these 256 values the correctly rounded fp32 quotient is the float64 quotient rounded to fp32
// (tests/test_augment_cpu.py checks all of them)
AUG_HD float aug_unit(uint8_t v) { return (float)v / 255.0f; }

// cv2.BORDER_REFLECT_101 (scipy's 'mirror'): ... 2 1 | 0 1 2 ... n-1 | n-2 n-3 ...; one reflection, so |i - [0,n)| < n
AUG_HD int aug_reflect101(int i, int n) {
    i = i < 0 ? -i : i;
    return i >= n ? 2 * (n - 1) - i : i;
}

// q = e / d, r = e % d for 0 <= e < 2^22, 1 <= d < 2^12, rcp = 1.0f / d: the fp32 quotient is off by at most one
AUG_HD void aug_divmod(int e, int d, float rcp, int* q, int* r) {
    int qq = (int)((float)e * rcp);
    int rr = e - qq * d;
    if (rr < 0) { qq -= 1; rr += d; }
    if (rr >= d) { qq += 1; rr -= d; }
    *q = qq;
    *r = rr;
}

// x = mask ? bg : train_x  (dataset.py:476)
AUG_HD uint8_t aug_composite(uint8_t obj, uint8_t bg, uint8_t mask) { return mask ? bg : obj; }

// Affine(scale=s), order 1, mode='constant', cval=0: src = centre + (dst - centre) / s about ((W-1)/2, (H-1)/2); the four
// neighbours are blended, a neighbour outside the image counts as 0
template <class Src>
AUG_HD uint8_t aug_affine_pixel(const Src& src, int y, int x, int c, int H, int W, float inv_s) {
    const float cx = 0.5f * (float)(W - 1), cy = 0.5f * (float)(H - 1);
    float sx = cx + ((float)x - cx) * inv_s, sy = cy + ((float)y - cy) * inv_s;
    // far outside: everything is 0 (and the casts below stay defined)
    if (!(sx > -1.0f && sx < (float)W && sy > -1.0f && sy < (float)H)) return 0;
    const float fx0 = floorf(sx), fy0 = floorf(sy);
    const int x0 = (int)fx0, y0 = (int)fy0;
    const float fx = sx - fx0, fy = sy - fy0;
    const bool xa = x0 >= 0, xb = x0 + 1 < W, ya = y0 >= 0, yb = y0 + 1 < H;
    const float p00 = (xa && ya) ? (float)src(y0, x0, c) : 0.0f;
    const float p01 = (xb && ya) ? (float)src(y0, x0 + 1, c) : 0.0f;
    const float p10 = (xa && yb) ? (float)src(y0 + 1, x0, c) : 0.0f;
    const float p11 = (xb && yb) ? (float)src(y0 + 1, x0 + 1, c) : 0.0f;
    const float top = (1.0f - fx) * p00 + fx * p01, bot = (1.0f - fx) * p10 + fx * p11;
    return aug_round_u8((1.0f - fy) * top + fy * bot);
}

// GaussianBlur: the K x K sum of w[dy] * w[dx] * src over the reflect-101 neighbourhood, rows first, in fp32, rounded once.  K is a
// template parameter so that both loops unroll and w[] is indexed by constants only (on the device: the weights stay in SGPRs and the
// tap loop holds no load but the LDS gathers); aug_blur_dispatch turns the op's k into K.
template <int K, class Src>
AUG_HD uint8_t aug_blur_pixel(const Src& src, const float (&w)[K], int y, int x, int c, int H, int W) {
    constexpr int r = K >> 1;
    float acc = 0.0f;
    AUG_UNROLL
    for (int dy = 0; dy < K; ++dy) {
        const int yy = aug_reflect101(y + dy - r, H);
        float row = 0.0f;
    AUG_UNROLL
        for (int dx = 0; dx < K; ++dx) row += w[dx] * (float)src(yy, aug_reflect101(x + dx - r, W), c);
        acc += w[dy] * row;
    }
    return aug_round_u8(acc);
}

template <int K>
struct AugK {
    static constexpr int value = K;
};

// fn(AugK<k>{}) for an odd k in [1, AUG_MAX_BLUR_K]; false for any other k
template <class Fn>
AUG_HD bool aug_blur_dispatch(int k, const Fn& fn) {
    switch (k) {
        case 1: fn(AugK<1>{}); return true;
        case 3: fn(AugK<3>{}); return true;
        case 5: fn(AugK<5>{}); return true;
        case 7: fn(AugK<7>{}); return true;
        case 9: fn(AugK<9>{}); return true;
        case 11: fn(AugK<11>{}); return true;
        case 13: fn(AugK<13>{}); return true;
        case 15: fn(AugK<15>{}); return true;
    }
    return false;
}

// CoarseDropout: bit (c * plane + row_cell + col_cell) of the mask set -> the pixel is dropped.  The index is formed in uint32 (table
// entries come from device memory and may hold anything); bit_set(b) answers for one bit and answers "kept" for a bit outside the pool
template <class Bits>
AUG_HD uint8_t aug_dropout_pixel(uint8_t v, const Bits& bit_set, uint32_t row_cell, uint32_t col_cell, int c, uint32_t plane) {
    return bit_set((uint32_t)c * plane + row_cell + col_cell) ? (uint8_t)0 : v;
}

// the four pointwise ops on one value of channel c (f = op.f[c], flag = op.i[c])
AUG_HD uint8_t aug_add(uint8_t v, float f) { return aug_round_u8((float)v + f); }
AUG_HD uint8_t aug_invert(uint8_t v, int flag) { return flag ? (uint8_t)(255 - v) : v; }
AUG_HD uint8_t aug_multiply(uint8_t v, float f) { return aug_round_u8((float)v * f); }
AUG_HD uint8_t aug_contrast(uint8_t v, float f) { return aug_round_u8(128.0f + f * ((float)v - 128.0f)); }

AUG_HD bool aug_is_pointwise(int32_t code) { return code >= AUG_ADD && code <= AUG_CONTRAST; }

AUG_HD uint8_t aug_pointwise(int32_t code, uint8_t v, float f, int flag) {
    switch (code) {
        case AUG_ADD: return aug_add(v, f);
        case AUG_INVERT: return aug_invert(v, flag);
        case AUG_MULTIPLY: return aug_multiply(v, f);
        case AUG_CONTRAST: return aug_contrast(v, f);
    }
    return v;
}

}  // namespace aae_augment
