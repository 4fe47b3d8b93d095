// Stand-alone host driver of csrc/kernels/encoder_bwd_core.h: a layer's backward pass in PARITY form, run serially through the same
// index maps the kernels call (the padding, the weight-gradient gather, the tap list of a parity, the delta pixel of an input pixel
// and a tap), with float64 sums, so that tests/test_encoder_bwd_cpu.py can hold the maps against the direct formulas of
// tests/encoder_grad_reference.py.
//
//   encoder_bwd_host [--mutate N] <in> <out>
//     in : int32 head[12] = {0, B, H, W, Cin, Cout, KS, S, u8, with_g_in, 0, 0}; a_in (float32, or uint8 padded to a multiple of 4 bytes),
//                                                                                float32 a_out, g_out, w
//          int32 head[12] = {1, B, J, U, with_g_a, 0 ...};                       float32 a, dz, w
//     out: float32 delta, db, dw, then g_in when asked for (a layer); db, dw, then g_a when asked for (the dense layer)
//   --mutate N seeds index mistake N (EbwdMistake of the core header: 1 pads (before, after) swapped, 2 the parity tap residue off by
//   one, 3 taps not matched to w's (kh, kw) in the data gradient, 4 x and y pads exchanged, 5 zero-parity pixels left unwritten): the
//   test records how many cases of the table notice each.  g_in starts as NaN: a pixel nobody writes stays NaN.
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#define ENCODER_BWD_SEEDED_MISTAKES
#include "../../augmentedautoencoder_amd/csrc/kernels/encoder_bwd_core.h"

using namespace aae_ebwd;

static bool read_all(FILE* f, void* p, size_t bytes) { return fread(p, 1, bytes, f) == bytes; }
static bool write_f32(FILE* f, const std::vector<double>& v) {
    std::vector<float> o(v.size());
    for (size_t i = 0; i < v.size(); ++i) o[i] = (float)v[i];
    return fwrite(o.data(), 4, o.size(), f) == o.size();
}

static int run_layer(const int32_t* head, FILE* in, FILE* out) {
    const int B = head[1], H = head[2], W = head[3], Cin = head[4], Cout = head[5], KS = head[6], S = head[7], u8 = head[8], with_g_in = head[9];
    if (B < 1 || H < 1 || W < 1 || Cin < 1 || Cout < 1 || KS < 1 || S < 1) return 3;
    // the output shape is the forward's, whatever the seeded mistake does to the padding
    const int Ho = (H + S - 1) / S, Wo = (W + S - 1) / S;
    const ConvGeom g = make_geom(B, H, W, Cin, Cout, KS, S);
    const size_t n_in = (size_t)B * H * W * Cin, n_out = (size_t)B * Ho * Wo * Cout, n_w = (size_t)KS * KS * Cin * Cout;
    std::vector<float> a_in(n_in), a_out(n_out), g_out(n_out), w(n_w);
    if (u8) {
        std::vector<unsigned char> raw((n_in + 3) / 4 * 4);
        if (!read_all(in, raw.data(), raw.size())) return 2;
        for (size_t i = 0; i < n_in; ++i) a_in[i] = u8_to_unit(raw[i]);
    } else if (!read_all(in, a_in.data(), n_in * 4)) {
        return 2;
    }
    if (!read_all(in, a_out.data(), n_out * 4) || !read_all(in, g_out.data(), n_out * 4) || !read_all(in, w.data(), n_w * 4)) return 2;

    std::vector<double> delta(n_out), db(Cout, 0.0);
    for (size_t i = 0; i < n_out; ++i) {
        delta[i] = a_out[i] > 0.0f ? (double)g_out[i] : 0.0;
        db[i % Cout] += delta[i];
    }
    std::vector<double> dw(n_w, 0.0);
    for (int b = 0; b < B; ++b)
        for (int oy = 0; oy < Ho; ++oy)
            for (int ox = 0; ox < Wo; ++ox) {
                const double* d = &delta[((size_t)(b * Ho + oy) * Wo + ox) * Cout];
                for (int kh = 0; kh < KS; ++kh)
                    for (int kw = 0; kw < KS; ++kw) {
                        const int sp = wgrad_src_pixel(g, kh, kw, b, oy, ox);
                        if (sp < 0) continue;
                        const float* a = &a_in[(size_t)sp * Cin];
                        double* acc = &dw[(size_t)(kh * KS + kw) * Cin * Cout];
                        for (int ci = 0; ci < Cin; ++ci)
                            for (int co = 0; co < Cout; ++co) acc[(size_t)ci * Cout + co] += (double)a[ci] * d[co];
                    }
            }
    if (!write_f32(out, delta) || !write_f32(out, db) || !write_f32(out, dw)) return 4;
    if (with_g_in) {
        std::vector<double> g_in(n_in, (double)NAN);
        for (int ry = 0; ry < S; ++ry)
            for (int rx = 0; rx < S; ++rx) {
                const int nty = parity_tap_count(KS, ry, g.pt, S), ntx = parity_tap_count(KS, rx, g.pl, S);
                if (nty * ntx == 0 && EBWD_MISTAKE(MISTAKE_ZERO_PARITY_UNWRITTEN)) continue;
                const int Hp = parity_extent(H, ry, S), Wp = parity_extent(W, rx, S);
                for (int b = 0; b < B; ++b)
                    for (int jy = 0; jy < Hp; ++jy)
                        for (int jx = 0; jx < Wp; ++jx) {
                            const int iy = ry + S * jy, ix = rx + S * jx;
                            double* o = &g_in[((size_t)(b * H + iy) * W + ix) * Cin];
                            for (int ci = 0; ci < Cin; ++ci) o[ci] = 0.0;
                            for (int ty = 0; ty < nty; ++ty)
                                for (int tx = 0; tx < ntx; ++tx) {
                                    const int kh = parity_tap(ry, g.pt, S, ty), kw = parity_tap(rx, g.pl, S, tx);
                                    const int dp = dgrad_delta_pixel(g, kh, kw, b, iy, ix);
                                    if (dp < 0) continue;
                                    const double* d = &delta[(size_t)dp * Cout];
                                    const int tap = EBWD_MISTAKE(MISTAKE_TAPS_NOT_MATCHED) ? (KS - 1 - kh) * KS + (KS - 1 - kw) : kh * KS + kw;
                                    const float* wt = &w[(size_t)tap * Cin * Cout];
                                    for (int ci = 0; ci < Cin; ++ci)
                                        for (int co = 0; co < Cout; ++co) o[ci] += d[co] * (double)wt[(size_t)ci * Cout + co];
                                }
                        }
            }
        if (!write_f32(out, g_in)) return 4;
    }
    return 0;
}

static int run_dense(const int32_t* head, FILE* in, FILE* out) {
    const int B = head[1], J = head[2], U = head[3], with_g_a = head[4];
    if (B < 1 || J < 1 || U < 1) return 3;
    std::vector<float> a((size_t)B * J), dz((size_t)B * U), w((size_t)J * U);
    if (!read_all(in, a.data(), a.size() * 4) || !read_all(in, dz.data(), dz.size() * 4) || !read_all(in, w.data(), w.size() * 4)) return 2;
    std::vector<double> db(U, 0.0), dw((size_t)J * U, 0.0), g_a((size_t)B * J, 0.0);
    for (int b = 0; b < B; ++b)
        for (int u = 0; u < U; ++u) {
            const double d = (double)dz[(size_t)b * U + u];
            db[u] += d;
            for (int j = 0; j < J; ++j) {
                dw[(size_t)j * U + u] += (double)a[(size_t)b * J + j] * d;
                g_a[(size_t)b * J + j] += d * (double)w[(size_t)j * U + u];
            }
        }
    if (!write_f32(out, db) || !write_f32(out, dw)) return 4;
    if (with_g_a && !write_f32(out, g_a)) return 4;
    return 0;
}

int main(int argc, char** argv) {
    int at = 1;
    if (argc > 2 && !strcmp(argv[1], "--mutate")) {
        encoder_bwd_mistake = atoi(argv[2]);
        at = 3;
    }
    if (argc != at + 2) {
        fprintf(stderr, "usage: encoder_bwd_host [--mutate N] <in> <out>\n");
        return 1;
    }
    FILE* in = fopen(argv[at], "rb");
    FILE* out = fopen(argv[at + 1], "wb");
    if (!in || !out) return 2;
    int32_t head[12];
    if (!read_all(in, head, sizeof(head))) return 2;
    const int rc = head[0] == 1 ? run_dense(head, in, out) : run_layer(head, in, out);
    fclose(in);
    if (fclose(out)) return 4;
    return rc;
}
