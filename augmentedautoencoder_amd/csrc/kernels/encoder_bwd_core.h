// Index maps of the encoder's backward pass: the TF 'same' padding of a strided convolution, the source pixel a
// weight-gradient row reads at an output pixel, the taps an input parity sees, and the delta pixel an input pixel reads through a
// tap.  Plain functions that compile for the device (encoder_bwd_f32.h) and for the host (tests/native/encoder_bwd_host.cpp runs them
// serially against the direct float64 formulas of tests/encoder_grad_reference.py).
//
// A layer: a_out[b, oy, ox, co] = relu(sum a_in[b, S oy + kh - pt, S ox + kw - pl, ci] w[kh, kw, ci, co] + bias), Ho = ceil(H / S),
// total padding max((Ho - 1) S + KS - H, 0), before = total / 2, the odd pixel at the end.  Input pixel iy is read by output row oy
// through tap kh exactly when S oy + kh - pt = iy, so a pixel of parity r = iy mod S sees only the taps kh = (r + pt) mod S + S m:
// per parity class the data gradient is a small stride-1 convolution over the delta grid.  Taps are selected, never summed.
#pragma once

#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define EBWD_HD __host__ __device__ __forceinline__
#else
#define EBWD_HD static inline
#endif

// tests/native/encoder_bwd_host.cpp seeds index mistakes (its --mutate flag) to show that its case table notices them; the library
// never defines this
#ifdef ENCODER_BWD_SEEDED_MISTAKES
static int encoder_bwd_mistake = 0;
#define EBWD_MISTAKE(n) (encoder_bwd_mistake == (n))
#else
#define EBWD_MISTAKE(n) false
#endif

namespace aae_ebwd {

enum EbwdMistake : int32_t {
    MISTAKE_PADS_SWAPPED = 1,           // (before, after) exchanged
    MISTAKE_PARITY_RESIDUE = 2,         // the first tap of a parity off by one
    MISTAKE_TAPS_NOT_MATCHED = 3,       // the data gradient multiplies delta's tap with another tap of w (seeded in the host driver's own loop)
    MISTAKE_XY_PADS_EXCHANGED = 4,      // the y padding used in x and the x padding in y
    MISTAKE_ZERO_PARITY_UNWRITTEN = 5   // a parity class without a tap is skipped instead of zeroed (seeded in the host driver's own loop)
};

struct ConvGeom {
    int32_t B, H, W, Cin, Cout, KS, S;
    int32_t Ho, Wo;
    int32_t pt, pb, pl, pr;     // padding before / after in y, before / after in x
};

// oracle.reference_cpu.same_pad
EBWD_HD void same_pad(int n, int ks, int s, int* out, int* before, int* after) {
    const int o = (n + s - 1) / s;
    int total = (o - 1) * s + ks - n;
    if (total < 0) total = 0;
    *out = o;
    *before = total / 2;
    *after = total - total / 2;
    if (EBWD_MISTAKE(MISTAKE_PADS_SWAPPED)) { const int t = *before; *before = *after; *after = t; }
}

EBWD_HD ConvGeom make_geom(int B, int H, int W, int Cin, int Cout, int KS, int S) {
    ConvGeom g;
    g.B = B; g.H = H; g.W = W; g.Cin = Cin; g.Cout = Cout; g.KS = KS; g.S = S;
    int ho, wo, pt, pb, pl, pr;
    same_pad(H, KS, S, &ho, &pt, &pb);
    same_pad(W, KS, S, &wo, &pl, &pr);
    g.Ho = ho; g.Wo = wo;
    if (EBWD_MISTAKE(MISTAKE_XY_PADS_EXCHANGED)) { g.pt = pl; g.pb = pr; g.pl = pt; g.pr = pb; }
    else { g.pt = pt; g.pb = pb; g.pl = pl; g.pr = pr; }
    return g;
}

// float32(v / 255.) of a uint8 input pixel: the value the forward's 256-entry table holds (one correctly rounded division)
EBWD_HD float u8_to_unit(unsigned v) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __fdiv_rn((float)v, 255.0f);
#else
    return (float)v / 255.0f;
#endif
}

// ---- weight gradient: dW[kh, kw, ci, co] = sum over output pixels (b, oy, ox) of a_in[src_pixel] * delta[b, oy, ox, co] ---------------
// pixel index (b H + iy) W + ix of the input pixel tap (kh, kw) reads at output pixel (b, oy, ox); -1 in the padding
EBWD_HD int wgrad_src_pixel(const ConvGeom& g, int kh, int kw, int b, int oy, int ox) {
    const int iy = g.S * oy + kh - g.pt, ix = g.S * ox + kw - g.pl;
    if (iy < 0 || iy >= g.H || ix < 0 || ix >= g.W) return -1;
    return (b * g.H + iy) * g.W + ix;
}

// ---- data gradient by input parity ----------------------------------------------------------------------------------------------------
// pixels of parity r along an axis of n pixels: r, r + S, ...
EBWD_HD int parity_extent(int n, int r, int S) { return r < n ? (n - r + S - 1) / S : 0; }

// the taps a pixel of parity r sees along an axis padded by `pad` before: first, first + S, ... below KS
EBWD_HD int parity_first_tap(int r, int pad, int S) { return (r + pad + (EBWD_MISTAKE(MISTAKE_PARITY_RESIDUE) ? 1 : 0)) % S; }
EBWD_HD int parity_tap_count(int KS, int r, int pad, int S) {
    const int f = parity_first_tap(r, pad, S);
    return f < KS ? (KS - 1 - f) / S + 1 : 0;
}
EBWD_HD int parity_tap(int r, int pad, int S, int m) { return parity_first_tap(r, pad, S) + S * m; }

// pixel index (b Ho + oy) Wo + ox of the output pixel that read input pixel (b, iy, ix) through tap (kh, kw); -1 if there is none
EBWD_HD int dgrad_delta_pixel(const ConvGeom& g, int kh, int kw, int b, int iy, int ix) {
    const int ny = iy + g.pt - kh, nx = ix + g.pl - kw;
    if (ny < 0 || nx < 0 || ny % g.S != 0 || nx % g.S != 0) return -1;
    const int oy = ny / g.S, ox = nx / g.S;
    if (oy >= g.Ho || ox >= g.Wo) return -1;
    return (b * g.Ho + oy) * g.Wo + ox;
}

}  // namespace aae_ebwd
