// Kernels of the decoder's backward pass, fp32 throughout, v_mfma_f32_32x32x2_f32 for the three products:
//
//   delta_bias_kernel + column_sum_finish_kernel   delta = dL/d(pre-activation) written once, per-channel sums through fixed trees
//   wgrad_kernel<NT> + wgrad_reduce_kernel         dWphase = up(a_in)^T delta, per phase and K split -> partials -> dW [KS,KS,Cin,Cout]
//   fold_weights_kernel                            W [KS,KS,Cin,Cout] -> folded phase weights, packed [K/4][Cin][4] (fp64 sums, one rounding)
//   dgrad_kernel<NT>                               g_in = gather(delta) . Wfolded^T
//   dense_dw_kernel, dense_dz_kernel<NT> + splitk_sum_kernel
//
// Every MFMA kernel is a block of four waves stacked in rows: wave v owns rows 32 v ... 32 v + 31 of a 128-row tile and all
// 32 NT columns (NT = 1, 2, 4).  Ragged tiles are zero-filled in LDS and masked at the store.  The weight gradient contracts
// over pixels, the slow index of both NHWC operands: for one k, 32 consecutive rows (channels) are contiguous in memory, so its
// slabs are kept k-major in LDS ([32 k][128 rows], [32 k][32 NT columns]) -- a straight copy in, and a fragment read is 32
// consecutive words.  The data gradient and the dense dz contract over channels, the fast index: they use the row-major slabs of
// tile_f32.h (mfma_slab).  No atomics: every output element has one writer and every sum one order.
// The kernels that are no templates are `inline`: the encoder's backward pass (encoder_bwd_f32.h, another translation unit) launches
// delta_bias_kernel, column_sum_finish_kernel, dense_dw_kernel, dense_dz_kernel and splitk_sum_kernel too.
#pragma once

#include "decoder_bwd_core.h"
#include "tile_f32.h"

#if defined(__clang__)
#pragma clang diagnostic push
#pragma clang diagnostic ignored "-Wcuda-compat"      // (an `inline` kernel: one definition per library, which is what is meant)
#endif

namespace aae_bwd {

constexpr int BWD_BLOCK = 256;
constexpr int BWD_BM = 128;           // tile rows
constexpr int BWD_BK = 32;            // k per slab
constexpr int BWD_MAX_CHUNKS = 256;   // row chunks of the column sums

// (b, h, w) of a pixel index that advances by a fixed step
struct PixelWalk {
    int b, h, w;
    __device__ __forceinline__ void start(int pix, int H, int W) {
        w = pix % W;
        const int q = pix / W;
        h = q % H;
        b = q / H;
    }
    __device__ __forceinline__ void advance(int n, int H, int W) {
        w += n;
        while (w >= W) { w -= W; ++h; }
        while (h >= H) { h -= H; ++b; }
    }
};

// ---- delta and the column sums -------------------------------------------------------------------------------------------------------
struct DeltaBiasArgs {
    const float* g_out;     // [rows][C]
    const float* a_out;     // [rows][C]
    float* delta;           // [rows][C]
    float* partial;         // [chunks][C]
    int rows, C, act;
    int cw;                 // channels per block: a power of two, 4 ... 64
    int rows_per_chunk;
};

// grid (ceil(C / cw), chunks): the block's 256 / cw row lanes walk the chunk's rows, a lane's sum is one chain in row order, the
// lanes are added in lane order
inline __global__ __launch_bounds__(BWD_BLOCK) void delta_bias_kernel(DeltaBiasArgs a) {
    __shared__ float sums[BWD_BLOCK];
    const int t = threadIdx.x, cl = t & (a.cw - 1), rl = t / a.cw, nrl = BWD_BLOCK / a.cw;
    const int c = blockIdx.x * a.cw + cl;
    const int row0 = blockIdx.y * a.rows_per_chunk;
    const int row1 = min(a.rows, row0 + a.rows_per_chunk);
    float s = 0.0f;
    if (c < a.C)
        for (int r = row0 + rl; r < row1; r += nrl) {
            const size_t i = (size_t)r * a.C + c;
            const float d = act_delta(a.act, a.g_out[i], a.a_out[i]);
            a.delta[i] = d;
            s += d;
        }
    sums[t] = s;
    __syncthreads();
    if (rl == 0 && c < a.C) {
        float tot = sums[cl];
        for (int l = 1; l < nrl; ++l) tot += sums[l * a.cw + cl];
        a.partial[(size_t)blockIdx.y * a.C + c] = tot;
    }
}

// out[c] = partial[0][c] + partial[1][c] + ... in that order
inline __global__ __launch_bounds__(BWD_BLOCK) void column_sum_finish_kernel(const float* partial, int chunks, int C, float* out) {
    const int c = blockIdx.x * BWD_BLOCK + threadIdx.x;
    if (c >= C) return;
    float s = partial[c];
    for (int k = 1; k < chunks; ++k) s += partial[(size_t)k * C + c];
    out[c] = s;
}

// ---- tile store ---------------------------------------------------------------------------------------------------------------------
template <int NT>
__device__ __forceinline__ void store_tile(const f32x16 (&acc)[1][NT], float* out, int ld, int row0, int rows, int col0, int cols, int lane) {
#pragma unroll
    for (int ni = 0; ni < NT; ++ni) {
        const int c = col0 + 32 * ni + (lane & 31);
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int m = row0 + aae::acc_row(r, lane);
            if (m < rows && c < cols) out[(size_t)m * ld + c] = acc[0][ni][r];
        }
    }
}

// ---- weight gradient ------------------------------------------------------------------------------------------------------------------
struct WgradArgs {
    const float* a_in;      // [B][H][W][Cin]
    const float* delta;     // [B][scale H][scale W][Cout]
    float* partial;         // [splits][P][rows_per_phase][Cout]
    StageGeom g;
    int rows_per_phase;     // U * U * Cin, row (ty U + tx) Cin + ci
    int row_tiles, col_tiles;           // per phase
    int splits, slabs_per_split;
    int kpix;               // B * H * W, the contraction length of one phase
};

// grid: ((phase * splits + split) * row_tiles + row tile) * col_tiles + column tile
template <int NT>
__global__ __launch_bounds__(BWD_BLOCK) void wgrad_kernel(WgradArgs a) {
    constexpr int BN = 32 * NT;
    __shared__ float As[BWD_BK * BWD_BM];
    __shared__ float Bs[BWD_BK * BN];
    const StageGeom g = a.g;
    int bid = blockIdx.x;
    const int ct = bid % a.col_tiles; bid /= a.col_tiles;
    const int rt = bid % a.row_tiles; bid /= a.row_tiles;
    const int split = bid % a.splits;
    const int phase = bid / a.splits;
    const int t = threadIdx.x, lane = t & 63, wv = t >> 6;

    // A loader: a fixed row of the tile per thread, every second k of the slab
    const int ar = t & (BWD_BM - 1), ak = t >> 7;
    const int R = rt * BWD_BM + ar;
    const bool a_row_ok = R < a.rows_per_phase;
    const int tap = a_row_ok ? R / g.Cin : 0, ci = a_row_ok ? R - tap * g.Cin : 0;
    const int ty = tap / g.U, tx = tap - ty * g.U;
    // B loader: a fixed column per thread, every (256 / BN)-th k
    constexpr int BSTEP = BWD_BLOCK / BN;
    const int bc = t % BN, bk = t / BN;
    const int col = ct * BN + bc;
    const bool b_col_ok = col < g.Cout;

    const int k_begin = split * a.slabs_per_split * BWD_BK;
    const int k_end = min(a.kpix, k_begin + a.slabs_per_split * BWD_BK);
    PixelWalk pa, pb;
    pa.start(min(k_begin + ak, a.kpix - 1), g.H, g.W);
    pb.start(min(k_begin + bk, a.kpix - 1), g.H, g.W);

    f32x16 acc[1][NT];
#pragma unroll
    for (int ni = 0; ni < NT; ++ni)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[0][ni][r] = 0.0f;

    for (int k0 = k_begin; k0 < k_end; k0 += BWD_BK) {
#pragma unroll 4
        for (int k = ak; k < BWD_BK; k += 2) {
            float v = 0.0f;
            if (a_row_ok && k0 + k < k_end) {
                const int sp = wgrad_src_pixel(g, phase, ty, tx, pa.b, pa.h, pa.w);
                if (sp >= 0) v = a.a_in[(size_t)sp * g.Cin + ci];
            }
            As[k * BWD_BM + ar] = v;
            pa.advance(2, g.H, g.W);
        }
#pragma unroll 4
        for (int k = bk; k < BWD_BK; k += BSTEP) {
            float v = 0.0f;
            if (b_col_ok && k0 + k < k_end) v = a.delta[(size_t)phase_delta_pixel(g, phase, pb.b, pb.h, pb.w) * g.Cout + col];
            Bs[k * BN + bc] = v;
            pb.advance(BSTEP, g.H, g.W);
        }
        __syncthreads();
        const int i = lane & 31, hh = lane >> 5;
#pragma unroll
        for (int s = 0; s < BWD_BK / 2; ++s) {
            const float av = As[(2 * s + hh) * BWD_BM + 32 * wv + i];
#pragma unroll
            for (int ni = 0; ni < NT; ++ni) acc[0][ni] = aae::mfma_32x32x2(av, Bs[(2 * s + hh) * BN + 32 * ni + i], acc[0][ni]);
        }
        __syncthreads();
    }
    float* out = a.partial + ((size_t)split * g.P + phase) * a.rows_per_phase * g.Cout;
    store_tile<NT>(acc, out, g.Cout, rt * BWD_BM + 32 * wv, a.rows_per_phase, ct * BN, g.Cout, lane);
}

// dW[kh, kw, ci, co] = sum over phases (outer, ascending) and splits (inner, ascending) of the phase's folded tap: the K reduce
// and the unfold of the four phases in one pass
struct WgradReduceArgs {
    const float* partial;
    float* dw;
    StageGeom g;
    int rows_per_phase, splits;
    int total;              // KS * KS * Cin * Cout
};

inline __global__ __launch_bounds__(BWD_BLOCK) void wgrad_reduce_kernel(WgradReduceArgs a) {
    const StageGeom g = a.g;
    for (int e = blockIdx.x * BWD_BLOCK + threadIdx.x; e < a.total; e += gridDim.x * BWD_BLOCK) {
        const int co = e % g.Cout;
        int q = e / g.Cout;
        const int ci = q % g.Cin; q /= g.Cin;
        const int kw = q % g.KS, kh = q / g.KS;
        float s = 0.0f;
        for (int phase = 0; phase < g.P; ++phase) {
            const int row = unfold_tap(g, phase, kh, kw) * g.Cin + ci;
            for (int sp = 0; sp < a.splits; ++sp) s += a.partial[(((size_t)sp * g.P + phase) * a.rows_per_phase + row) * g.Cout + co];
        }
        a.dw[e] = s;
    }
}

// ---- folded weights of the data gradient ----------------------------------------------------------------------------------------------
// wf [(phase U U + tap) C4 + c4][Cin][4]: element q of the slot is Wphase[tap][ci][4 c4 + q] (0 past Cout), Wphase the float64 sum
// of the taps of W that fold into it, rounded once (aae_decoder_impl.h::fold_phase)
struct FoldArgs {
    const float* w;         // [KS][KS][Cin][Cout]
    float* wf;
    StageGeom g;
    int C4;                 // ceil(Cout / 4)
    int total;              // P * U * U * C4 * Cin * 4
};

inline __global__ __launch_bounds__(BWD_BLOCK) void fold_weights_kernel(FoldArgs a) {
    const StageGeom g = a.g;
    for (int e = blockIdx.x * BWD_BLOCK + threadIdx.x; e < a.total; e += gridDim.x * BWD_BLOCK) {
        const int q = e & 3;
        int r = e >> 2;
        const int ci = r % g.Cin; r /= g.Cin;
        const int c4 = r % a.C4; r /= a.C4;
        const int tap = r % (g.U * g.U), phase = r / (g.U * g.U);
        const int co = 4 * c4 + q;
        double s = 0.0;
        if (co < g.Cout)
            for (int kh = 0; kh < g.KS; ++kh)
                for (int kw = 0; kw < g.KS; ++kw)
                    if (unfold_tap(g, phase, kh, kw) == tap) s += (double)a.w[((size_t)(kh * g.KS + kw) * g.Cin + ci) * g.Cout + co];
        a.wf[e] = (float)s;
    }
}

// ---- data gradient --------------------------------------------------------------------------------------------------------------------
struct DgradArgs {
    const float* delta;     // [B][scale H][scale W][Cout]
    const float* wf;        // [kslots][Cin][4]
    float* g_in;            // [B][H][W][Cin]
    StageGeom g;
    int C4, kslots;         // P * U * U * C4 slots of 4 k
    int M;                  // B * H * W
    int row_tiles, col_tiles;
};

template <int NT>
__global__ __launch_bounds__(BWD_BLOCK) void dgrad_kernel(DgradArgs a) {
    constexpr int BN = 32 * NT;
    __shared__ __attribute__((aligned(16))) float As[aae::kSlabFloatsA];
    __shared__ __attribute__((aligned(16))) float Bs[8 * BN * 4];
    const StageGeom g = a.g;
    const int ct = blockIdx.x % a.col_tiles, rt = blockIdx.x / a.col_tiles;
    const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
    // A loader: slot t & 7 of rows (t >> 3) + 32 j
    const int aslot = t & 7;
    int pb[4], ph[4], pw[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int m = rt * BWD_BM + (t >> 3) + 32 * j;
        if (m < a.M) {
            pw[j] = m % g.W;
            const int q = m / g.W;
            ph[j] = q % g.H;
            pb[j] = q / g.H;
        } else {
            pb[j] = -1; ph[j] = 0; pw[j] = 0;
        }
    }
    const int n0 = ct * BN;
    const int UU = g.U * g.U;
    const bool vec = (g.Cout & 3) == 0;

    f32x16 acc[1][NT];
#pragma unroll
    for (int ni = 0; ni < NT; ++ni)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[0][ni][r] = 0.0f;

    for (int s0 = 0; s0 < a.kslots; s0 += 8) {
        const int gs = s0 + aslot;
        const bool slot_ok = gs < a.kslots;
        const int c4 = slot_ok ? gs % a.C4 : 0;
        const int tp = slot_ok ? gs / a.C4 : 0;
        const int tap = tp % UU, phase = tp / UU;
        const int ty = tap / g.U, tx = tap - ty * g.U;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            f32x4 v = {0.0f, 0.0f, 0.0f, 0.0f};
            if (slot_ok && pb[j] >= 0) {
                const int dp = dgrad_delta_pixel(g, phase, ty, tx, pb[j], ph[j], pw[j]);
                if (dp >= 0) {
                    const float* src = a.delta + (size_t)dp * g.Cout + 4 * c4;
                    if (vec) v = *reinterpret_cast<const f32x4*>(src);
                    else
                        for (int q = 0; q < 4; ++q) if (4 * c4 + q < g.Cout) v[q] = src[q];
                }
            }
            aae::lds_write4(As + aae::a_slab_off((t >> 3) + 32 * j, aslot), v);
        }
        for (int i = t; i < 8 * BN; i += BWD_BLOCK) {
            const int slot = i / BN, c = i - slot * BN;
            f32x4 v = {0.0f, 0.0f, 0.0f, 0.0f};
            if (s0 + slot < a.kslots && n0 + c < g.Cin) v = *reinterpret_cast<const f32x4*>(a.wf + ((size_t)(s0 + slot) * g.Cin + n0 + c) * 4);
            aae::lds_write4(Bs + (slot * BN + c) * 4, v);
        }
        __syncthreads();
        aae::mfma_slab<1, NT>(As, Bs, BN, 32 * wv, 0, lane, acc);
        __syncthreads();
    }
    store_tile<NT>(acc, a.g_in, g.Cin, rt * BWD_BM + 32 * wv, a.M, n0, g.Cin, lane);
}

// ---- dense layer ----------------------------------------------------------------------------------------------------------------------
// dW[j, u] = sum over b (ascending) of z[b, j] * delta[b, u]: K = B, memory-bound
inline __global__ __launch_bounds__(BWD_BLOCK) void dense_dw_kernel(const float* z, const float* delta, float* dw, int B, int J, int U) {
    const long long total = (long long)J * U;
    for (long long e = (long long)blockIdx.x * BWD_BLOCK + threadIdx.x; e < total; e += (long long)gridDim.x * BWD_BLOCK) {
        const int u = (int)(e % U), j = (int)(e / U);
        float s = 0.0f;
        for (int b = 0; b < B; ++b) s = fmaf(z[(size_t)b * J + j], delta[(size_t)b * U + u], s);
        dw[e] = s;
    }
}

struct DenseDzArgs {
    const float* delta;     // [B][U]
    const float* w;         // [J][U]
    float* partial;         // [splits][B][J]
    int B, J, U;
    int row_tiles, col_tiles, splits, slabs_per_split;
};

// dz = delta . W^T: M = B, N = J, K = U split over the grid; both operands are row-major in k
template <int NT>
__global__ __launch_bounds__(BWD_BLOCK) void dense_dz_kernel(DenseDzArgs a) {
    constexpr int BN = 32 * NT;
    __shared__ __attribute__((aligned(16))) float As[aae::kSlabFloatsA];
    __shared__ __attribute__((aligned(16))) float Bs[8 * BN * 4];
    int bid = blockIdx.x;
    const int ct = bid % a.col_tiles; bid /= a.col_tiles;
    const int rt = bid % a.row_tiles;
    const int split = bid / a.row_tiles;
    const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
    const int n0 = ct * BN;
    const int k_begin = split * a.slabs_per_split * BWD_BK;
    const int k_end = min(a.U, k_begin + a.slabs_per_split * BWD_BK);
    const bool vec = (a.U & 3) == 0;

    f32x16 acc[1][NT];
#pragma unroll
    for (int ni = 0; ni < NT; ++ni)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[0][ni][r] = 0.0f;

    for (int k0 = k_begin; k0 < k_end; k0 += BWD_BK) {
        for (int i = t; i < BWD_BM * 8; i += BWD_BLOCK) {
            const int slot = i & 7, row = i >> 3;
            const int m = rt * BWD_BM + row, k = k0 + 4 * slot;
            f32x4 v = {0.0f, 0.0f, 0.0f, 0.0f};
            if (m < a.B && k < k_end) {
                const float* src = a.delta + (size_t)m * a.U + k;
                if (vec) v = *reinterpret_cast<const f32x4*>(src);           // (k_end is a multiple of 4 here: U and the slab size are)
                else
                    for (int q = 0; q < 4; ++q) if (k + q < k_end) v[q] = src[q];
            }
            aae::lds_write4(As + aae::a_slab_off(row, slot), v);
        }
        for (int i = t; i < 8 * BN; i += BWD_BLOCK) {
            const int slot = i & 7, c = i >> 3;
            const int n = n0 + c, k = k0 + 4 * slot;
            f32x4 v = {0.0f, 0.0f, 0.0f, 0.0f};
            if (n < a.J && k < k_end) {
                const float* src = a.w + (size_t)n * a.U + k;
                if (vec) v = *reinterpret_cast<const f32x4*>(src);
                else
                    for (int q = 0; q < 4; ++q) if (k + q < k_end) v[q] = src[q];
            }
            aae::lds_write4(Bs + (slot * BN + c) * 4, v);
        }
        __syncthreads();
        aae::mfma_slab<1, NT>(As, Bs, BN, 32 * wv, 0, lane, acc);
        __syncthreads();
    }
    store_tile<NT>(acc, a.partial + (size_t)split * a.B * a.J, a.J, rt * BWD_BM + 32 * wv, a.B, n0, a.J, lane);
}

// out[e] = partial[0][e] + partial[1][e] + ... in that order
inline __global__ __launch_bounds__(BWD_BLOCK) void splitk_sum_kernel(const float* partial, int splits, int total, float* out) {
    for (int e = blockIdx.x * BWD_BLOCK + threadIdx.x; e < total; e += gridDim.x * BWD_BLOCK) {
        float s = partial[e];
        for (int k = 1; k < splits; ++k) s += partial[(size_t)k * total + e];
        out[e] = s;
    }
}

}  // namespace aae_bwd

#if defined(__clang__)
#pragma clang diagnostic pop
#endif
