// Host driver of csrc/kernels/augment_core.h: the workgroup of augment_batch.h as serial loops over one image at a time (composite
// into a buffer, the ops in order between two buffers with the kernel's range checks, the three outputs), outputs that start full
// of 0xA5.  Built and run by tests/test_augment_cpu.py (also with -fsanitize=address,undefined).
//
// augment_host <in.bin> <out.bin>
//   in: int32 N, M, H, W, C, B, aux_words; uint8 train_x[N*H*W*C], mask_x[N*H*W], train_y[N*H*W*C], bg[M*H*W*C]; int32 train_idx[B],
//       bg_idx[B], n_ops[B]; AugOp ops[B*16]; uint32 aux[aux_words]   (tests/augment_cases.py: write_input)
//   out: uint8 batch_x[B*H*W*C]; float32 batch_x[B*H*W*C]; float32 batch_y[B*H*W*C]
// augment_host --unit <out.bin>
//   out: float32 aug_unit(v) for v = 0 ... 255
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../../augmentedautoencoder_amd/csrc/kernels/augment_core.h"

using namespace aae_augment;

template <typename T>
static void rd(FILE* f, std::vector<T>& v) {
    if (!v.empty() && fread(v.data(), sizeof(T), v.size(), f) != v.size()) {
        fprintf(stderr, "augment_host: short input file\n");
        exit(2);
    }
}

static float bits_float(uint32_t u) {
    float f;
    memcpy(&f, &u, 4);
    return f;
}

int main(int argc, char** argv) {
    if (argc == 3 && strcmp(argv[1], "--unit") == 0) {
        FILE* out = fopen(argv[2], "wb");
        if (!out) return 1;
        for (int v = 0; v < 256; ++v) {
            const float u = aug_unit((uint8_t)v);
            fwrite(&u, 4, 1, out);
        }
        fclose(out);
        return 0;
    }
    if (argc != 3) {
        fprintf(stderr, "usage: augment_host <in.bin> <out.bin> | augment_host --unit <out.bin>\n");
        return 1;
    }
    FILE* in = fopen(argv[1], "rb");
    FILE* out = fopen(argv[2], "wb");
    if (!in || !out) return 1;
    std::vector<int32_t> hd(7);
    rd(in, hd);
    const int N = hd[0], M = hd[1], H = hd[2], W = hd[3], C = hd[4], B = hd[5], aux_words = hd[6];
    if (N < 1 || M < 1 || H < 1 || W < 1 || C < 1 || C > AUG_MAX_CHANNELS || B < 1 || aux_words < 0 || H > 4095 || W > 4095) return 1;
    const size_t total = (size_t)H * W * C;
    std::vector<uint8_t> train_x(N * total), mask_x((size_t)N * H * W), train_y(N * total), bg(M * total);
    std::vector<int32_t> train_idx(B), bg_idx(B), n_ops(B);
    std::vector<AugOp> ops((size_t)B * AUG_MAX_OPS);
    std::vector<uint32_t> aux(aux_words);
    rd(in, train_x); rd(in, mask_x); rd(in, train_y); rd(in, bg); rd(in, train_idx); rd(in, bg_idx); rd(in, n_ops); rd(in, ops); rd(in, aux);
    fclose(in);

    std::vector<uint8_t> out_u8(B * total, 0xA5);
    std::vector<float> out_x(B * total, bits_float(0xA5A5A5A5u)), out_y(B * total, bits_float(0xA5A5A5A5u));
    const float rcp_C = 1.0f / (float)C, rcp_W = 1.0f / (float)W;
    std::vector<uint8_t> buf0(total), buf1(total);
    for (int b = 0; b < B; ++b) {
        const int ti = train_idx[b], bi = bg_idx[b];
        if (ti < 0 || ti >= N || bi < 0 || bi >= M) continue;
        uint8_t* cur = buf0.data();
        uint8_t* other = buf1.data();
        for (size_t e = 0; e < total; ++e) {
            // the kernel's index arithmetic: byte -> (pixel, channel) -> (row, column)
            int pix, c, y, x;
            aug_divmod((int)e, C, rcp_C, &pix, &c);
            aug_divmod(pix, W, rcp_W, &y, &x);
            if ((size_t)pix != e / C || (size_t)y != e / C / W) return 5;
            out_y[b * total + e] = aug_unit(train_y[ti * total + e]);
            cur[e] = aug_composite(train_x[ti * total + e], bg[bi * total + e], mask_x[(size_t)ti * H * W + pix]);
        }
        int n = n_ops[b];
        n = n < 0 ? 0 : (n > AUG_MAX_OPS ? AUG_MAX_OPS : n);
        for (int k = 0; k < n; ++k) {
            const AugOp op = ops[(size_t)b * AUG_MAX_OPS + k];
            const uint8_t* src = cur;
            auto at = [&](int y, int x, int c) -> uint8_t { return src[((size_t)y * W + x) * C + c]; };
            auto spatial = [&](auto fn) {
                for (int y = 0; y < H; ++y)
                    for (int x = 0; x < W; ++x)
                        for (int c = 0; c < C; ++c) other[((size_t)y * W + x) * C + c] = fn(y, x, c);
                uint8_t* t = cur; cur = other; other = t;
            };
            if (op.code == AUG_AFFINE) {
                const float inv_s = op.f[0];
                spatial([&](int y, int x, int c) { return aug_affine_pixel(at, y, x, c, H, W, inv_s); });
            } else if (op.code == AUG_BLUR) {
                const int kk = op.i[0], w0 = op.i[1];
                if (kk >= 1 && kk <= AUG_MAX_BLUR_K && (kk >> 1) < H && (kk >> 1) < W && w0 >= 0 && w0 <= aux_words - kk)
                    aug_blur_dispatch(kk, [&](auto K) {
                        float w[K.value];
                        for (int t = 0; t < K.value; ++t) w[t] = bits_float(aux[w0 + t]);
                        spatial([&](int y, int x, int c) { return aug_blur_pixel<K.value>(at, w, y, x, c, H, W); });
                    });
            } else if (op.code == AUG_DROPOUT) {
                const int m0 = op.i[0], r0 = op.i[1], c0 = op.i[2], plane = op.i[3];
                if (m0 >= 0 && r0 >= 0 && c0 >= 0 && plane >= 0 && r0 <= aux_words - H && c0 <= aux_words - W) {
                    const uint32_t words = aux_words > m0 ? (uint32_t)(aux_words - m0) : 0u;
                    auto bit_set = [&](uint32_t bit) -> bool { return (bit >> 5) < words && ((aux[m0 + (bit >> 5)] >> (bit & 31u)) & 1u); };
                    spatial([&](int y, int x, int c) { return aug_dropout_pixel(at(y, x, c), bit_set, aux[r0 + y], aux[c0 + x], c, (uint32_t)plane); });
                }
            } else if (aug_is_pointwise(op.code)) {
                for (size_t e = 0; e < total; ++e) {
                    const int c = (int)(e % C);
                    cur[e] = aug_pointwise(op.code, cur[e], op.f[c], op.i[c]);
                }
            }
        }
        for (size_t e = 0; e < total; ++e) {
            out_u8[b * total + e] = cur[e];
            out_x[b * total + e] = aug_unit(cur[e]);
        }
    }
    fwrite(out_u8.data(), 1, out_u8.size(), out);
    fwrite(out_x.data(), 4, out_x.size(), out);
    fwrite(out_y.data(), 4, out_y.size(), out);
    fclose(out);
    return 0;
}
