// Kernels of the encoder's backward pass, fp32 throughout, v_mfma_f32_32x32x2_f32 for the products:
//
//   delta_bias_kernel + column_sum_finish_kernel   (decoder_bwd_f32.h) delta = g_out where a_out > 0, per-channel sums through fixed trees
//   conv_wgrad_kernel<NT, AVEC> + splitk_sum_kernel   dW [KS KS Cin, Cout] = gather(a_in)^T delta, K = B Ho Wo split over the grid
//   conv_dgrad_kernel<NT>                          g_in of one input parity = gather(delta) . w^T over the taps that parity sees
//   column_partial_kernel + column_sum_finish_kernel, dense_dw_kernel, dense_dz_kernel<NT> + splitk_sum_kernel   the linear dense layer
//
// The block is the one of decoder_bwd_f32.h: four waves stacked in rows, wave v owns rows 32 v ... 32 v + 31 of a 128-row tile and
// all 32 NT columns.  The weight gradient contracts over output pixels, the slow index of both NHWC operands: k-major slabs
// ([32 k][128 rows], [32 k][32 NT columns]).  A loader thread owns ONE k of the slab -- it decodes that output pixel once per slab
// -- and four runs of four consecutive rows, whose taps and channels it decoded once before the K loop; with Cin a multiple of 4 a
// run is one 16-byte load, and a row of delta is read in 16-byte pieces when Cout is a multiple of 4.  The data gradient contracts
// over (tap, co), co the fast index of delta and of w: the row-major slabs of tile_f32.h (mfma_slab), both operands in 16-byte
// pieces straight from delta and from w [KS,KS,Cin,Cout] -- taps are selected, never summed, so there is no folded copy.  Both MFMA
// kernels fetch the next slab into registers before they multiply the current one.  Ragged tiles are zero-filled in LDS and masked
// at the store.  No atomics: every output element has one writer and every sum one order.
#pragma once

#include "decoder_bwd_f32.h"
#include "encoder_bwd_core.h"

namespace aae_ebwd {

using aae_bwd::BWD_BLOCK;
using aae_bwd::BWD_BM;
using aae_bwd::BWD_BK;

// -DAAE_EBWD_SERIAL_SLABS builds the load - barrier - multiply - barrier loop of section 4j instead, for the A/B of tools/bench_encoder_bwd.py
#ifdef AAE_EBWD_SERIAL_SLABS
constexpr bool kSlabInFlight = false;
#else
constexpr bool kSlabInFlight = true;
#endif

// ---- weight gradient ------------------------------------------------------------------------------------------------------------------
struct ConvWgradArgs {
    const void* a_in;       // [B][H][W][Cin] float32, or uint8 (in_u8)
    const float* delta;     // [B Ho Wo][Cout]
    float* partial;         // [splits][M][Cout]; dw itself when splits = 1
    ConvGeom g;
    int M;                  // KS * KS * Cin, row (kh KS + kw) Cin + ci
    int K;                  // B * Ho * Wo
    int row_tiles, col_tiles, splits, slabs_per_split;
    int in_u8;
};

// a loader row: (kh - pt + 16) << 26 | (kw - pl + 16) << 20 | ci, -1 past M  (|kh - pt|, |kw - pl| <= 7, ci < 2^20)
__device__ __forceinline__ int wgrad_row_code(const ConvGeom& g, int R, int M) {
    if (R >= M) return -1;
    const int tap = R / g.Cin, ci = R - tap * g.Cin;
    const int kh = tap / g.KS, kw = tap - kh * g.KS;
    return ((kh - g.pt + 16) << 26) | ((kw - g.pl + 16) << 20) | ci;
}

// grid: ((split * row_tiles) + row tile) * col_tiles + column tile
template <int NT, bool AVEC>
__global__ __launch_bounds__(BWD_BLOCK) void conv_wgrad_kernel(ConvWgradArgs a) {
    constexpr int BN = 32 * NT;
    constexpr int AE = AVEC ? 1 : 4;                    // decoded rows per run: the run's first, or each of the four
    __shared__ __attribute__((aligned(16))) float As[BWD_BK * BWD_BM];
    __shared__ __attribute__((aligned(16))) float Bs[BWD_BK * BN];
    const ConvGeom g = a.g;
    int bid = blockIdx.x;
    const int ct = bid % a.col_tiles; bid /= a.col_tiles;
    const int rt = bid % a.row_tiles;
    const int split = bid / a.row_tiles;
    const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
    const int ak = t >> 3, aq = t & 7;                  // A loader: k of the slab, runs aq + 8 j
    const bool bvec = (g.Cout & 3) == 0;
    const float* a_f = static_cast<const float*>(a.a_in);
    const unsigned char* a_b = static_cast<const unsigned char*>(a.a_in);

    int code[4][AE];
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int e = 0; e < AE; ++e) code[j][e] = wgrad_row_code(g, rt * BWD_BM + 4 * (aq + 8 * j) + e, a.M);

    const int k_begin = split * a.slabs_per_split * BWD_BK;
    const int k_end = min(a.K, k_begin + a.slabs_per_split * BWD_BK);

    f32x4 ra[4], rb[NT];
    auto fetch = [&](int k0) {
        const int kk = k0 + ak;
        const bool k_ok = kk < k_end;
        int ox = 0, oy = 0, b = 0;
        if (k_ok) {                                     // the output pixel of this thread's k, once per slab
            ox = kk % g.Wo;
            const int q = kk / g.Wo;
            oy = q % g.Ho;
            b = q / g.Ho;
        }
        const int iy0 = g.S * oy, ix0 = g.S * ox;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            f32x4 v = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
            for (int e = 0; e < AE; ++e) {
                const int c = code[j][e];
                if (!k_ok || c < 0) continue;
                const int iy = iy0 + ((c >> 26) & 63) - 16, ix = ix0 + ((c >> 20) & 63) - 16, ci = c & 0xFFFFF;
                if (iy < 0 || iy >= g.H || ix < 0 || ix >= g.W) continue;
                const size_t src = (size_t)((b * g.H + iy) * g.W + ix) * g.Cin + ci;
                if (AVEC) v = *reinterpret_cast<const f32x4*>(a_f + src);
                else v[e] = a.in_u8 ? u8_to_unit(a_b[src]) : a_f[src];
            }
            ra[j] = v;
        }
#pragma unroll
        for (int jj = 0; jj < NT; ++jj) {
            const int i = t + BWD_BLOCK * jj;
            const int kb = i / (BN / 4), cq = i - kb * (BN / 4);
            const int col = ct * BN + 4 * cq, kb_abs = k0 + kb;
            f32x4 v = {0.0f, 0.0f, 0.0f, 0.0f};
            if (kb_abs < k_end && col < g.Cout) {
                const float* src = a.delta + (size_t)kb_abs * g.Cout + col;
                if (bvec) v = *reinterpret_cast<const f32x4*>(src);
                else
                    for (int q = 0; q < 4; ++q) if (col + q < g.Cout) v[q] = src[q];
            }
            rb[jj] = v;
        }
    };

    f32x16 acc[1][NT];
#pragma unroll
    for (int ni = 0; ni < NT; ++ni)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[0][ni][r] = 0.0f;

    if (kSlabInFlight && k_begin < k_end) fetch(k_begin);
    for (int k0 = k_begin; k0 < k_end; k0 += BWD_BK) {
        if (!kSlabInFlight) fetch(k0);
#pragma unroll
        for (int j = 0; j < 4; ++j) aae::lds_write4(As + ak * BWD_BM + 4 * (aq + 8 * j), ra[j]);
#pragma unroll
        for (int jj = 0; jj < NT; ++jj) aae::lds_write4(Bs + 4 * (t + BWD_BLOCK * jj), rb[jj]);       // (kb BN + 4 cq = 4 i)
        __syncthreads();
        if (kSlabInFlight && k0 + BWD_BK < k_end) fetch(k0 + BWD_BK);    // the next slab travels under the MFMAs
        const int i = lane & 31, hh = lane >> 5;
#pragma unroll
        for (int s = 0; s < BWD_BK / 2; ++s) {
            const float av = As[(2 * s + hh) * BWD_BM + 32 * wv + i];
#pragma unroll
            for (int ni = 0; ni < NT; ++ni) acc[0][ni] = aae::mfma_32x32x2(av, Bs[(2 * s + hh) * BN + 32 * ni + i], acc[0][ni]);
        }
        __syncthreads();
    }
    aae_bwd::store_tile<NT>(acc, a.partial + (size_t)split * a.M * g.Cout, g.Cout, rt * BWD_BM + 32 * wv, a.M, ct * BN, g.Cout, lane);
}

// ---- data gradient by input parity ----------------------------------------------------------------------------------------------------
struct ConvDgradArgs {
    const float* delta;     // [B Ho Wo][Cout]
    const float* w;         // [KS][KS][Cin][Cout]
    float* g_in;            // [B][H][W][Cin]
    ConvGeom g;
    int C4;                 // ceil(Cout / 4): k slots of one tap
    int row_tiles;          // of the largest parity class
    int col_tiles;
};

// grid: ((parity * row_tiles) + row tile) * col_tiles + column tile; parity = ry S + rx.  Rows are the pixels (b, jy, jx) of the parity's
// grid, input pixel (ry + S jy, rx + S jx); k slot (ty ntx + tx) C4 + c4 is channels 4 c4 ... of tap (fy + S ty, fx + S tx).
template <int NT>
__global__ __launch_bounds__(BWD_BLOCK) void conv_dgrad_kernel(ConvDgradArgs a) {
    constexpr int BN = 32 * NT;
    __shared__ __attribute__((aligned(16))) float As[aae::kSlabFloatsA];
    __shared__ __attribute__((aligned(16))) float Bs[8 * BN * 4];
    __shared__ int row_pixel[BWD_BM];                   // input pixel index of a tile row, -1 past the parity's rows
    const ConvGeom g = a.g;
    int bid = blockIdx.x;
    const int ct = bid % a.col_tiles; bid /= a.col_tiles;
    const int rt = bid % a.row_tiles;
    const int parity = bid / a.row_tiles;
    const int ry = parity / g.S, rx = parity - ry * g.S;
    const int Hp = parity_extent(g.H, ry, g.S), Wp = parity_extent(g.W, rx, g.S);
    const int Mp = g.B * Hp * Wp;
    if (rt * BWD_BM >= Mp) return;                      // (the whole block: a smaller parity class has fewer row tiles)
    const int nty = parity_tap_count(g.KS, ry, g.pt, g.S), ntx = parity_tap_count(g.KS, rx, g.pl, g.S);
    const int kslots = nty * ntx * a.C4;
    const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
    const int aslot = t & 7;
    const int n0 = ct * BN;
    const bool vec = (g.Cout & 3) == 0;

    // the pixel of a tile row, decoded once: the A loader's four rows (t >> 3) + 32 j, and the table the store reads
    int pb[4], py[4], px[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int m = rt * BWD_BM + (t >> 3) + 32 * j;
        if (m < Mp) {
            const int jx = m % Wp, q = m / Wp;
            px[j] = rx + g.S * jx;
            py[j] = ry + g.S * (q % Hp);
            pb[j] = q / Hp;
        } else {
            pb[j] = -1; py[j] = 0; px[j] = 0;
        }
        if (aslot == 0) row_pixel[(t >> 3) + 32 * j] = pb[j] < 0 ? -1 : (pb[j] * g.H + py[j]) * g.W + px[j];
    }

    f32x4 ra[4], rb[NT];
    auto fetch = [&](int s0) {
        const int gs = s0 + aslot;
        const bool slot_ok = gs < kslots;
        const int tp = slot_ok ? gs / a.C4 : 0;
        const int c4 = slot_ok ? gs - tp * a.C4 : 0;
        const int ty = tp / ntx, tx = tp - ty * ntx;
        const int kh = parity_tap(ry, g.pt, g.S, ty), kw = parity_tap(rx, g.pl, g.S, tx);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            f32x4 v = {0.0f, 0.0f, 0.0f, 0.0f};
            if (slot_ok && pb[j] >= 0) {
                const int dp = dgrad_delta_pixel(g, kh, kw, pb[j], py[j], px[j]);
                if (dp >= 0) {
                    const float* src = a.delta + (size_t)dp * g.Cout + 4 * c4;
                    if (vec) v = *reinterpret_cast<const f32x4*>(src);
                    else
                        for (int q = 0; q < 4; ++q) if (4 * c4 + q < g.Cout) v[q] = src[q];
                }
            }
            ra[j] = v;
        }
#pragma unroll
        for (int jj = 0; jj < NT; ++jj) {
            const int i = t + BWD_BLOCK * jj;           // 8 BN = 256 NT slots of (k slot, column)
            const int slot = i / BN, c = i - slot * BN;
            const int gsb = s0 + slot;
            f32x4 v = {0.0f, 0.0f, 0.0f, 0.0f};
            if (gsb < kslots && n0 + c < g.Cin) {
                const int tpb = gsb / a.C4, c4b = gsb - tpb * a.C4;
                const int tyb = tpb / ntx, txb = tpb - tyb * ntx;
                const int wt = parity_tap(ry, g.pt, g.S, tyb) * g.KS + parity_tap(rx, g.pl, g.S, txb);      // the tap delta was read through
                const float* src = a.w + ((size_t)wt * g.Cin + n0 + c) * g.Cout + 4 * c4b;
                if (vec) v = *reinterpret_cast<const f32x4*>(src);
                else
                    for (int q = 0; q < 4; ++q) if (4 * c4b + q < g.Cout) v[q] = src[q];
            }
            rb[jj] = v;
        }
    };

    f32x16 acc[1][NT];
#pragma unroll
    for (int ni = 0; ni < NT; ++ni)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[0][ni][r] = 0.0f;

    if (kSlabInFlight && kslots > 0) fetch(0);
    for (int s0 = 0; s0 < kslots; s0 += 8) {
        if (!kSlabInFlight) fetch(s0);
#pragma unroll
        for (int j = 0; j < 4; ++j) aae::lds_write4(As + aae::a_slab_off((t >> 3) + 32 * j, aslot), ra[j]);
#pragma unroll
        for (int jj = 0; jj < NT; ++jj) aae::lds_write4(Bs + 4 * (t + BWD_BLOCK * jj), rb[jj]);       // ((slot BN + c) 4 = 4 i)
        __syncthreads();
        if (kSlabInFlight && s0 + 8 < kslots) fetch(s0 + 8);             // the next slab travels under the MFMAs
        aae::mfma_slab<1, NT>(As, Bs, BN, 32 * wv, 0, lane, acc);
        __syncthreads();
    }
    if (kslots == 0) __syncthreads();                   // (row_pixel)
#pragma unroll
    for (int ni = 0; ni < NT; ++ni) {
        const int c = n0 + 32 * ni + (lane & 31);
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int pix = row_pixel[32 * wv + aae::acc_row(r, lane)];
            if (pix >= 0 && c < g.Cin) a.g_in[(size_t)pix * g.Cin + c] = acc[0][ni][r];
        }
    }
}

// ---- the linear dense layer: db = column sums of dz ------------------------------------------------------------------------------------
// the partial sums of delta_bias_kernel without the activation mask: grid (ceil(C / cw), chunks), partial [chunks][C]
#if defined(__clang__)
#pragma clang diagnostic push
#pragma clang diagnostic ignored "-Wcuda-compat"      // (an `inline` kernel, as in decoder_bwd_f32.h)
#endif
inline __global__ __launch_bounds__(BWD_BLOCK) void column_partial_kernel(const float* x, float* partial, int rows, int C, int cw, int rows_per_chunk) {
    __shared__ float sums[BWD_BLOCK];
    const int t = threadIdx.x, cl = t & (cw - 1), rl = t / cw, nrl = BWD_BLOCK / cw;
    const int c = blockIdx.x * cw + cl;
    const int row0 = blockIdx.y * rows_per_chunk;
    const int row1 = min(rows, row0 + rows_per_chunk);
    float s = 0.0f;
    if (c < C)
        for (int r = row0 + rl; r < row1; r += nrl) s += x[(size_t)r * C + c];
    sums[t] = s;
    __syncthreads();
    if (rl == 0 && c < C) {
        float tot = sums[cl];
        for (int l = 1; l < nrl; ++l) tot += sums[l * cw + cl];
        partial[(size_t)blockIdx.y * C + c] = tot;
    }
}

#if defined(__clang__)
#pragma clang diagnostic pop
#endif

}  // namespace aae_ebwd
