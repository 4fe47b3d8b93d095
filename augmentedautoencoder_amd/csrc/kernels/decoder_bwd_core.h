// Index maps of the decoder's backward pass: the activation derivative, the phase decomposition of an exact
// 2x nearest-neighbour upsample followed by a KS x KS 'same' convolution, and the three gathers built on it (the source pixel a
// weight-gradient row reads, the delta pixel a phase contracts against, the delta pixel a data-gradient row reads).  Plain
// functions that compile for the device (decoder_bwd_f32.h) and for the host (tests/native/decoder_bwd_host.cpp runs them serially
// against the direct float64 formulas of tests/decoder_grad_reference.py).
//
// A stage in phase form.  scale = 2 (exact 2x) has P = 4 phases (py, px) = (phase >> 1, phase & 1) of U = (KS + 1) / 2 taps per
// axis; scale = 1 (no resize) is the one-phase case with U = KS.  Output pixel (scale h + py, scale w + px) reads source pixel
// (h + d0(py) + ty, w + d0(px) + tx) through folded tap (ty, tx); tap kh of the KS x KS kernel folds into ty = tap_of(py, kh).
// The upsampled range [0, scale H) maps exactly onto the source range [0, H), so "the tap is outside the upsampled image" and
// "the source pixel is outside the source" are the same condition: the border needs no folding.
#pragma once

#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define DBWD_HD __host__ __device__ __forceinline__
#else
#include <math.h>
#define DBWD_HD static inline
#endif

// tests/native/decoder_bwd_host.cpp seeds index mistakes (its --mutate flag) to show that its case table notices them; the library
// never defines this
#ifdef DECODER_BWD_SEEDED_MISTAKES
static int decoder_bwd_mistake = 0;
#define DBWD_MISTAKE(n) (decoder_bwd_mistake == (n))
#else
#define DBWD_MISTAKE(n) false
#endif

namespace aae_bwd {

enum BwdAct : int32_t { BWD_ACT_RELU = 0, BWD_ACT_SIGMOID = 1 };          // aae::ACT_RELU / ACT_SIGMOID of the forward
enum BwdMistake : int32_t { MISTAKE_PHASE_OFFSET = 1, MISTAKE_TAPS_NOT_FLIPPED = 2, MISTAKE_BORDER_FOLDED = 3, MISTAKE_PARITY_SWAPPED = 4 };

struct StageGeom {
    int32_t B, H, W, Cin, Cout, KS, pad;
    int32_t scale;      // 2: exact 2x upsampling (four phases), 1: no resize (one phase)
    int32_t P, U;       // phases, taps per axis of a phase
};

// d(k) = floor((p + k - pad) / 2): the source offset tap k of output parity p reads (aae_decoder_impl.h::phase_src_offset)
DBWD_HD int phase_src_offset(int p, int k, int pad) {
    const int v = p + k - pad;
    return v >= 0 ? v / 2 : -((-v + 1) / 2);
}

// offset of folded tap 0 of parity p
DBWD_HD int phase_d0(const StageGeom& g, int p) {
    if (g.scale == 1) return -g.pad;
    return phase_src_offset(p, 0, g.pad) + (DBWD_MISTAKE(MISTAKE_PHASE_OFFSET) ? 1 : 0);
}

// folded tap that tap k of the KS-tap kernel lands on, for output parity p
DBWD_HD int tap_of(const StageGeom& g, int p, int k) {
    if (g.scale == 1) return k;
    return phase_src_offset(p, k, g.pad) - phase_src_offset(p, 0, g.pad);
}

DBWD_HD StageGeom make_geom(int B, int H, int W, int Cin, int Cout, int KS, int scale) {
    StageGeom g;
    g.B = B; g.H = H; g.W = W; g.Cin = Cin; g.Cout = Cout; g.KS = KS; g.pad = (KS - 1) / 2; g.scale = scale;
    g.P = scale == 2 ? 4 : 1;
    g.U = scale == 2 ? (KS + 1) / 2 : KS;
    return g;
}

DBWD_HD int phase_py(int phase) { return phase >> 1; }
DBWD_HD int phase_px(int phase) { return phase & 1; }

DBWD_HD int clamp_or_reject(int v, int n) {
    if (DBWD_MISTAKE(MISTAKE_BORDER_FOLDED)) return v < 0 ? 0 : (v >= n ? n - 1 : v);        // (what a clamped resize index would do)
    return (v < 0 || v >= n) ? -1 : v;
}

// activation derivative: delta = dL/d(pre-activation) from g = dL/da and the activation value a
DBWD_HD float act_delta(int act, float g, float a) {
    if (act == BWD_ACT_SIGMOID) {
#if defined(__HIP_DEVICE_COMPILE__)
        return __fmul_rn(__fmul_rn(g, a), __fsub_rn(1.0f, a));
#else
        const float ga = g * a, om = 1.0f - a;
        return ga * om;
#endif
    }
    return a > 0.0f ? g : 0.0f;
}

// ---- weight gradient: dWphase[ty, tx, ci, co] = sum over source pixels (b, h, w) of a_in[src_pixel] * delta[delta_pixel] ----------
// pixel index (b H + h) W + w of the source pixel that row tap (ty, tx) reads at contraction pixel (b, h, w); -1 outside the source
DBWD_HD int wgrad_src_pixel(const StageGeom& g, int phase, int ty, int tx, int b, int h, int w) {
    const int sy = clamp_or_reject(h + phase_d0(g, phase_py(phase)) + ty, g.H);
    const int sx = clamp_or_reject(w + phase_d0(g, phase_px(phase)) + tx, g.W);
    if (sy < 0 || sx < 0) return -1;
    return (b * g.H + sy) * g.W + sx;
}

// pixel index in delta [B, scale H, scale W] of the output pixel of `phase` above source pixel (b, h, w)
DBWD_HD int phase_delta_pixel(const StageGeom& g, int phase, int b, int h, int w) {
    if (g.scale == 1) return (b * g.H + h) * g.W + w;
    const int py = DBWD_MISTAKE(MISTAKE_PARITY_SWAPPED) ? phase_px(phase) : phase_py(phase);
    const int px = DBWD_MISTAKE(MISTAKE_PARITY_SWAPPED) ? phase_py(phase) : phase_px(phase);
    return (b * 2 * g.H + 2 * h + py) * (2 * g.W) + 2 * w + px;
}

// ---- data gradient: g_in[b, h, w, ci] = sum over (phase, ty, tx, co) of delta[dgrad_delta_pixel] * Wphase[ty, tx, ci, co] -------------
// the output pixel of `phase` that read source pixel (b, h, w) through tap (ty, tx): the tap runs the other way; -1 if there is none
DBWD_HD int dgrad_delta_pixel(const StageGeom& g, int phase, int ty, int tx, int b, int h, int w) {
    const int sgn = DBWD_MISTAKE(MISTAKE_TAPS_NOT_FLIPPED) ? 1 : -1;
    const int oh = h + sgn * (phase_d0(g, phase_py(phase)) + ty), ow = w + sgn * (phase_d0(g, phase_px(phase)) + tx);
    if (oh < 0 || oh >= g.H || ow < 0 || ow >= g.W) return -1;
    return phase_delta_pixel(g, phase, b, oh, ow);
}

// ---- the unfold: dW[kh, kw] = sum over phases of dWphase[tap_of(py, kh), tap_of(px, kw)] ----------------------------------------------
DBWD_HD int unfold_tap(const StageGeom& g, int phase, int kh, int kw) {
    return tap_of(g, phase_py(phase), kh) * g.U + tap_of(g, phase_px(phase), kw);
}

}  // namespace aae_bwd
