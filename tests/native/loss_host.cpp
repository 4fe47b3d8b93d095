// Stand-alone host driver of csrc/kernels/loss_core.h: the selection of an image run serially with the same key, digit and
// narrowing functions the kernels call, the gradient of every element, and the regulariser's row functions.
//
//   loss_host <in> <out>         in: int32 B, n, kind, bootstrap_ratio; float32 x[B*n]; float32 target[B*n]
//                                out: float32 loss, per_image[B], dx[B*n]
//   loss_host --reg <in> <out>   in: int32 B, J; float32 z[B*J]         out: float32 loss, dz[B*J]
//
// The sums here are float64 over the float32 errors (the order of the kernels' float32 sums is theirs, and tested on the device).
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "../../augmentedautoencoder_amd/csrc/kernels/loss_core.h"

using namespace aae_loss;

static bool read_all(FILE* f, void* p, size_t bytes) { return fread(p, 1, bytes, f) == bytes; }

static int run_recon(const char* in, const char* out) {
    FILE* f = fopen(in, "rb");
    if (!f) return 2;
    int32_t head[4];
    if (!read_all(f, head, sizeof(head))) return 2;
    const int B = head[0], n = head[1], kind = head[2], ratio = head[3];
    if (B < 1 || n < 1 || ratio < 1 || n / ratio < 1) return 3;
    const size_t total = (size_t)B * n;
    std::vector<float> x(total), t(total), dx(total), per_image(B);
    if (!read_all(f, x.data(), total * 4) || !read_all(f, t.data(), total * 4)) return 2;
    fclose(f);

    const uint32_t k = (uint32_t)(n / ratio);
    const float scale = (float)(1.0 / ((double)B * (double)k));
    std::vector<float> d(n);
    std::vector<uint32_t> key(n);
    double batch = 0.0;
    for (int b = 0; b < B; ++b) {
        const float* xb = &x[(size_t)b * n];
        const float* tb = &t[(size_t)b * n];
        for (int i = 0; i < n; ++i) {
            d[i] = xb[i] - tb[i];
            key[i] = loss_key(loss_error(kind, d[i]));
        }
        uint32_t T = 0, want = UINT32_MAX;                     // ratio 1: every key >= 0 is selected
        if (k < (uint32_t)n) {
            uint32_t prefix = 0, remaining = k;
            for (int pass = 0; pass < LOSS_PASSES; ++pass) {
                uint32_t hist[LOSS_BINS] = {0};
                for (int i = 0; i < n; ++i)
                    if (loss_in_play(key[i], prefix, pass)) hist[loss_digit(key[i], pass)] += 1;
                uint32_t digit, left, held;
                loss_narrow(hist, remaining, &digit, &left, &held);
                prefix = loss_extend(prefix, digit, pass);
                remaining = left;
            }
            T = prefix;
            want = remaining;
        }
        double sum = 0.0;
        uint32_t ties = 0;                                     // keys == T before element i
        for (int i = 0; i < n; ++i) {
            const bool sel = loss_selected(key[i], T, ties, want);
            if (key[i] == T) ties += 1;
            if (sel) sum += (double)loss_error(kind, d[i]);
            dx[(size_t)b * n + i] = loss_grad(kind, d[i], sel, scale);
        }
        per_image[b] = (float)(sum / (double)k);
        batch += sum / (double)k;
    }
    const float loss = (float)(batch / (double)B);
    FILE* g = fopen(out, "wb");
    if (!g) return 2;
    fwrite(&loss, 4, 1, g);
    fwrite(per_image.data(), 4, B, g);
    fwrite(dx.data(), 4, total, g);
    fclose(g);
    return 0;
}

static int run_reg(const char* in, const char* out) {
    FILE* f = fopen(in, "rb");
    if (!f) return 2;
    int32_t head[2];
    if (!read_all(f, head, sizeof(head))) return 2;
    const int B = head[0], J = head[1];
    if (B < 1 || J < 1) return 3;
    std::vector<float> z((size_t)B * J), dz((size_t)B * J);
    if (!read_all(f, z.data(), z.size() * 4)) return 2;
    fclose(f);
    double total = 0.0;
    for (int b = 0; b < B; ++b) {
        double s = 0.0;
        for (int c = 0; c < J; ++c) s += (double)z[(size_t)b * J + c] * (double)z[(size_t)b * J + c];
        const double norm = reg_row_norm(s);
        total += (double)reg_row_loss(norm);
        for (int c = 0; c < J; ++c) dz[(size_t)b * J + c] = reg_row_grad(z[(size_t)b * J + c], norm, 1.0 / (double)B);
    }
    const float loss = (float)(total / (double)B);
    FILE* g = fopen(out, "wb");
    if (!g) return 2;
    fwrite(&loss, 4, 1, g);
    fwrite(dz.data(), 4, dz.size(), g);
    fclose(g);
    return 0;
}

int main(int argc, char** argv) {
    if (argc == 4 && argv[1][0] == '-' && argv[1][1] == '-' && argv[1][2] == 'r') return run_reg(argv[2], argv[3]);
    if (argc == 3) return run_recon(argv[1], argv[2]);
    fprintf(stderr, "usage: loss_host <in> <out> | loss_host --reg <in> <out>\n");
    return 1;
}
