// The per-element arithmetic of the training loss (the reference's auto_pose/ae/decoder.py:86-132 and encoder.py:97-100): the
// error of an element, its sortable key, the radix digits and the narrowing step of the threshold selection that stands in for
// tf.nn.top_k, the selection rule, the gradient of an element and the row functions of the latent-norm regulariser (DESIGN
// section 4i, table "TensorFlow semantics assumed").  Plain functions that compile for the device (recon_loss.h) and for the host
// (tests/native/loss_host.cpp drives them serially against the NumPy restatement in tests/loss_reference.py).
//
// Selection of the k largest errors of an image by threshold: T = the k-th largest key, found most significant digit first
// (LOSS_PASSES histograms of LOSS_BINS bins over the keys that still match the digits chosen so far); an element is selected when
// its key is above T, or equals T and fewer than `ties_wanted` equal keys precede it in index order.
#pragma once

#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define LOSS_HD __host__ __device__ __forceinline__
#else
#include <math.h>
#define LOSS_HD static inline
#endif

namespace aae_loss {

enum LossKind : int32_t { LOSS_L2 = 0, LOSS_L1 = 1 };

constexpr int LOSS_DIGIT_BITS = 8;
constexpr int LOSS_BINS = 1 << LOSS_DIGIT_BITS;
constexpr int LOSS_PASSES = 32 / LOSS_DIGIT_BITS;

LOSS_HD uint32_t loss_bits(float v) {
    uint32_t u;
    __builtin_memcpy(&u, &v, sizeof(u));
    return u;
}

// one rounding, never contracted with a neighbouring addition (the host driver is built with -ffp-contract=off)
LOSS_HD float loss_mul(float a, float b) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __fmul_rn(a, b);
#else
    return a * b;
#endif
}

// d = x - t in fp32; squared_difference / absolute_difference: the bits NumPy float32 gives
LOSS_HD float loss_error(int kind, float d) { return kind == LOSS_L1 ? fabsf(d) : loss_mul(d, d); }

// errors are non-negative, so the bit pattern with the sign cleared orders as the numbers do; a NaN ranks above +inf
LOSS_HD uint32_t loss_key(float e) { return loss_bits(e) & 0x7FFFFFFFu; }

LOSS_HD int loss_shift(int pass) { return 32 - LOSS_DIGIT_BITS * (pass + 1); }

// digit of `key` that pass 0 ... LOSS_PASSES - 1 looks at, most significant first: always inside [0, LOSS_BINS)
LOSS_HD uint32_t loss_digit(uint32_t key, int pass) { return (key >> loss_shift(pass)) & (uint32_t)(LOSS_BINS - 1); }

// does `key` still match the digits chosen by the passes before `pass`?
LOSS_HD bool loss_in_play(uint32_t key, uint32_t prefix, int pass) {
    if (pass == 0) return true;
    const int s = loss_shift(pass - 1);
    return (key >> s) == (prefix >> s);
}

LOSS_HD uint32_t loss_extend(uint32_t prefix, uint32_t digit, int pass) { return prefix | (digit << loss_shift(pass)); }

// Narrowing: with `above` keys in the bins over this one and h in it, the remaining-th largest key in play lies here
LOSS_HD bool loss_bin_holds(uint32_t above, uint32_t h, uint32_t remaining) { return above < remaining && remaining - above <= h; }

// The whole step over one histogram: the chosen digit, how many keys of that bin are still wanted, and the bin's count.
// sum(hist) >= remaining >= 1 on entry, so exactly one bin holds.
LOSS_HD void loss_narrow(const uint32_t* hist, uint32_t remaining, uint32_t* digit, uint32_t* left, uint32_t* held) {
    uint32_t above = 0;
    *digit = 0; *left = remaining; *held = 0;
    for (int b = LOSS_BINS - 1; b >= 0; --b) {
        if (loss_bin_holds(above, hist[b], remaining)) {
            *digit = (uint32_t)b;
            *left = remaining - above;
            *held = hist[b];
            return;
        }
        above += hist[b];
    }
}

// tie_rank = equal keys before this element in index order: the lowest indices win (tf.nn.top_k)
LOSS_HD bool loss_selected(uint32_t key, uint32_t T, uint32_t tie_rank, uint32_t ties_wanted) {
    return key > T || (key == T && tie_rank < ties_wanted);
}

// d loss / d x of one element; scale = float32(1 / (B k)).  L2: 2 d scale; L1: sign(d) scale, sign(0) = 0 (a NaN stays a NaN)
LOSS_HD float loss_grad(int kind, float d, bool selected, float scale) {
    if (kind == LOSS_L1) {
        const uint32_t u = loss_bits(d), mag = u & 0x7FFFFFFFu;
        const uint32_t signed_scale = (u & 0x80000000u) | loss_bits(scale);
        const uint32_t g = !selected || mag == 0u ? 0u : (mag > 0x7F800000u ? u : signed_scale);
        float r;
        __builtin_memcpy(&r, &g, sizeof(r));
        return r;
    }
    return selected ? loss_mul(2.0f * d, scale) : 0.0f;
}

// ---- Encoder.reg_loss: mean_b | ||z_b|| - 1 |.  The row's sum of squares is held in fp64 (J is a latent size). ----
LOSS_HD double reg_row_norm(double sum_sq) { return sqrt(sum_sq); }

LOSS_HD float reg_row_loss(double norm) { return (float)fabs(norm - 1.0); }

// sign(||z|| - 1) z / ||z|| / B; a zero row has no direction: 0 (TensorFlow would give NaN)
LOSS_HD float reg_row_grad(float z, double norm, double inv_B) {
    if (!(norm > 0.0)) return norm == 0.0 ? 0.0f : (float)norm;
    const double s = norm > 1.0 ? 1.0 : (norm < 1.0 ? -1.0 : (norm == 1.0 ? 0.0 : norm));
    return (float)(s * (double)z / norm * inv_B);
}

}  // namespace aae_loss
