// Decoder.reconstr_loss and Encoder.reg_loss with their gradients: one 1024-lane workgroup per image.
//
// recon_loss_kernel<PER, KIND, HIST>.  Element i of an image belongs to lane i % 1024, row j = i / 1024 (consecutive lanes read consecutive
// floats).  PER > 0: the image's differences d = x - t stay in PER VGPRs per lane from the one read to the gradient store (PER = 1,
// 8, 48: images of up to 1024, 8192 and 49152 elements; 128 x 128 x 3 is exactly the last).  PER = 0: a larger image is read
// again by every pass (it stays in L2).
//
//   1. bootstrap_ratio > 1: the k-th largest key T by LOSS_PASSES radix passes.  A pass counts the digit of every key still in
//      play into an LDS histogram, sums the histogram's copies per bin, and wave 0 narrows: a suffix sum over the 256 bins across
//      its lanes and loss_bin_holds on each.  The histogram (HIST_LANE) has 32 copies interleaved by lane, word = bin * 32 +
//      lane % 32: whatever the digits are, the 32 lanes of a half-wave add to 32 different banks, so the few exponents that
//      reconstruction errors share cost no more than spread digits do.  (HIST_WAVE, one 256-bin copy per wave, and HIST_SHARED,
//      one copy, serialise on a crowded bin; they are kept in the experiments build to be measured against.)
//   2. one sweep: select (key > T, or key == T and among the first `want` ties in index order), add the selected errors, store
//      the gradient of every element.  When the tie group is exactly `want` long (the common case) every key == T is selected
//      and no order is needed; otherwise the ties before an element are counted: a ballot per (row, wave), an exclusive
//      block-wide prefix over the 64 rows x 16 waves of a chunk in index order, a running base from chunk to chunk.
//   3. sums: a lane adds at most 64 rows, a wave reduces by a shuffle tree, the (chunk, wave) partials of the image by a tree over
//      1024 LDS words; the image's mean goes to the workspace with a plain store and recon_loss_finish_kernel reduces the B
//      means in a fixed order.  No floating-point atomic anywhere.
//
// The only data-derived index is a histogram bin, loss_digit() & 255.  Nothing device-resident moves a lane outside its buffers.
#pragma once

#include <hip/hip_runtime.h>

#include "loss_core.h"

namespace aae_loss {

constexpr int LOSS_BLOCK = 1024;
constexpr int LOSS_WAVES = LOSS_BLOCK / 64;
constexpr int LOSS_CHUNK_ROWS = 64;                                  // rows a lane adds before the tree steps; (row, wave) prefix entries = 1024
constexpr int LOSS_MAX_CHUNKS = LOSS_BLOCK / LOSS_WAVES;             // (chunk, wave) partial sums = 1024
constexpr int LOSS_RESIDENT_ROWS = 48;
constexpr int LOSS_MAX_N = LOSS_MAX_CHUNKS * LOSS_CHUNK_ROWS * LOSS_BLOCK;
constexpr int LOSS_MAX_BATCH = 64 * LOSS_BLOCK;                      // the finish kernel: a lane adds at most 64 means before the tree

enum LossHist : int { HIST_LANE = 0, HIST_WAVE = 1, HIST_SHARED = 2 };

template <int HIST> struct LossHistLayout;
template <> struct LossHistLayout<HIST_LANE> {
    static constexpr int COPIES = 32, BIN_STRIDE = 32, COPY_STRIDE = 1;
    static __device__ __forceinline__ int copy(int lane, int wave) { return lane & 31; }
};
template <> struct LossHistLayout<HIST_WAVE> {
    static constexpr int COPIES = LOSS_WAVES, BIN_STRIDE = 1, COPY_STRIDE = LOSS_BINS;
    static __device__ __forceinline__ int copy(int lane, int wave) { return wave; }
};
template <> struct LossHistLayout<HIST_SHARED> {
    static constexpr int COPIES = 1, BIN_STRIDE = 1, COPY_STRIDE = 0;
    static __device__ __forceinline__ int copy(int lane, int wave) { return 0; }
};

struct LossArgs {
    const float* x;
    const float* t;
    float* dx;               // [B, n] or null
    float* per_image;        // [B] or null
    float* means;            // [B] in the workspace
    float* sink;             // one word of the workspace that the lanes past the end of an image store into
    int n, k, select_all;
    float scale;             // float32(1 / (B k))
};

__device__ __forceinline__ uint32_t loss_uniform(uint32_t v) { return (uint32_t)__builtin_amdgcn_readfirstlane((int)v); }

// lane 0 receives the sum, added in a fixed tree
__device__ __forceinline__ float loss_wave_sum(float v) {
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o);
    return v;
}

// the sum of one value per lane of the workgroup, in lane 0 of wave 0; `slots` has LOSS_WAVES words
__device__ __forceinline__ float loss_block_sum(float v, float* slots, int lane, int wave) {
    v = loss_wave_sum(v);
    if (lane == 0) slots[wave] = v;
    __syncthreads();
    float r = 0.0f;
    if (wave == 0) {
        r = lane < LOSS_WAVES ? slots[lane] : 0.0f;
        for (int o = LOSS_WAVES / 2; o > 0; o >>= 1) r += __shfl_down(r, o);
    }
    return r;
}

// The rows of an image: each(chunk, f) calls f(row, index, d) for every row of a chunk (chunk < 0: of the image), the same trip
// count in every lane.  A lane of the last row that lies past the end of the image holds d = 0: key 0 at the highest indices, the
// very end of the stable descending order, so it is never among the first k <= n, it adds 0 to a sum, and a validity mask is
// needed at one place only, the gradient store.  (A mask per row in every sweep costs the 48-row form its SGPRs.)
template <int PER>
struct LossRows {
    float d[PER];
    int n, tid;
    __device__ __forceinline__ LossRows(const float* __restrict__ x, const float* __restrict__ t, int n_, int tid_) : n(n_), tid(tid_) {
#pragma unroll
        for (int j = 0; j < PER; ++j) {
            const int i = j * LOSS_BLOCK + tid;
            const int c = i < n ? i : n - 1;                         // past the end: the last element is read (no mask is kept across the loads) and dropped
            const float v = x[c] - t[c];
            d[j] = i < n ? v : 0.0f;
        }
    }
    __device__ __forceinline__ int chunks() const { return 1; }
    // The sweeps sit inside the pass loop and are unrolled: left alone, the compiler computes the PER keys of a lane once, ahead of
    // the loop, and spills them.  The empty asm makes each d opaque at every sweep, so a key lives from its multiply to its compare.
    template <class F>
    __device__ __forceinline__ void each(int chunk, F&& f) const {
#pragma unroll
        for (int j = 0; j < PER; ++j) {
            float v = d[j];
            asm volatile("" : "+v"(v));
            f(j, j * LOSS_BLOCK + tid, v);
            __builtin_amdgcn_sched_barrier(0);                       // one row's masks at a time: 48 rows of them do not fit the SGPRs
        }
    }
};

template <>
struct LossRows<0> {
    const float* __restrict__ x;
    const float* __restrict__ t;
    int n, tid, rows;
    __device__ __forceinline__ LossRows(const float* __restrict__ x_, const float* __restrict__ t_, int n_, int tid_)
        : x(x_), t(t_), n(n_), tid(tid_), rows((n_ + LOSS_BLOCK - 1) / LOSS_BLOCK) {}
    __device__ __forceinline__ int chunks() const { return (rows + LOSS_CHUNK_ROWS - 1) / LOSS_CHUNK_ROWS; }
    template <class F>
    __device__ __forceinline__ void each(int chunk, F&& f) const {
        const int j0 = chunk < 0 ? 0 : chunk * LOSS_CHUNK_ROWS;
        const int j1 = chunk < 0 ? rows : (j0 + LOSS_CHUNK_ROWS < rows ? j0 + LOSS_CHUNK_ROWS : rows);
        for (int j = j0; j < j1; ++j) {
            const int i = j * LOSS_BLOCK + tid;
            f(j, i, i < n ? x[i] - t[i] : 0.0f);
        }
    }
};

// the selecting sweep over one chunk: the sum of this lane's selected errors; IN_ORDER: ranks[] holds the ties before each (row, wave)
template <int KIND, bool IN_ORDER, bool WITH_DX, class Rows>
__device__ __forceinline__ float loss_sweep(const Rows& rows, int chunk, uint32_t T, uint32_t want, const uint32_t* ranks, float* dx, float* sink, float scale,
                                            int lane, int wave) {
    const int row0 = chunk * LOSS_CHUNK_ROWS;
    float sum = 0.0f;
    int n = rows.n;
    asm volatile("" : "+s"(n));                      // a compare of its own: sharing the masks of the load would keep 48 of them alive all through the kernel
    float* out = WITH_DX ? dx + (size_t)row0 * LOSS_BLOCK + rows.tid : nullptr;          // walks a row at a time: 48 precomputed addresses would not fit the VGPRs
    rows.each(chunk, [&](int j, int i, float d) {
        const float e = loss_error(KIND, d);
        const uint32_t key = loss_key(e);
        uint32_t rank = 0, wanted = 1;
        if (IN_ORDER) {
            const unsigned long long ties = __ballot(key == T);
            rank = ranks[(j - row0) * LOSS_WAVES + wave] + (uint32_t)__popcll(ties & ((1ull << lane) - 1ull));
            wanted = want;
        }
        const bool sel = loss_selected(key, T, rank, wanted);
        sum += sel ? e : 0.0f;
        if (WITH_DX) {
            const float g = loss_grad(KIND, d, sel, scale);
            asm volatile("" : "+v"(out));
            *(i < n ? out : sink) = g;                          // one select per store; a branch per row costs the 48-row form its SGPRs
            out += LOSS_BLOCK;
        }
    });
    return sum;
}

template <int PER, int KIND, int HIST>
__global__ __launch_bounds__(LOSS_BLOCK) void recon_loss_kernel(const LossArgs a) {
    using L = LossHistLayout<HIST>;
    constexpr int HIST_WORDS = LOSS_BINS * L::COPIES;
    __shared__ uint32_t hist[HIST_WORDS];
    __shared__ __attribute__((aligned(16))) uint32_t totals[LOSS_BINS];
    __shared__ uint32_t ranks[LOSS_BLOCK];          // ties per (row, wave) of a chunk, then the ties before each
    __shared__ float partial[LOSS_BLOCK];           // selected errors per (chunk, wave)
    __shared__ uint32_t wave_count[LOSS_WAVES];
    __shared__ float wave_sum[LOSS_WAVES];
    __shared__ uint32_t pick[3];                    // the narrowing step's digit, remaining count and bin count

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int n = a.n;
    const size_t at = (size_t)blockIdx.x * (size_t)n;
    const LossRows<PER> rows(a.x + at, a.t + at, n, tid);
    float* __restrict__ dx = a.dx ? a.dx + at : nullptr;

    uint32_t T = 0, want = 1;
    bool in_order = false;                           // the tie group is longer than `want`: index order decides
    if (!a.select_all) {
        uint32_t prefix = 0, remaining = (uint32_t)a.k, held = 0;
        for (int pass = 0; pass < LOSS_PASSES; ++pass) {
            for (int w = tid; w < HIST_WORDS; w += LOSS_BLOCK) hist[w] = 0;
            __syncthreads();
            rows.each(-1, [&](int, int, float d) {
                const uint32_t key = loss_key(loss_error(KIND, d));
                if (loss_in_play(key, prefix, pass))
                    atomicAdd(&hist[loss_digit(key, pass) * L::BIN_STRIDE + L::copy(lane, wave) * L::COPY_STRIDE], 1u);
            });
            __syncthreads();
            if (tid < LOSS_BINS) {
                uint32_t s = 0;
#pragma unroll
                for (int c = 0; c < L::COPIES; ++c) s += hist[tid * L::BIN_STRIDE + ((c + tid) % L::COPIES) * L::COPY_STRIDE];      // rotated: 32 lanes, 32 banks
                totals[tid] = s;
            }
            __syncthreads();
            if (wave == 0) {
                const uint4 h4 = reinterpret_cast<const uint4*>(totals)[lane];                  // bins 4 lane ... 4 lane + 3
                const uint32_t h[4] = {h4.x, h4.y, h4.z, h4.w};
                const uint32_t own = h[0] + h[1] + h[2] + h[3];
                uint32_t suffix = own;                                                          // keys in this lane's bins and every higher lane's
                for (int o = 1; o < 64; o <<= 1) {
                    const uint32_t v = __shfl_down(suffix, o);
                    if (lane + o < 64) suffix += v;
                }
                uint32_t above = suffix - own;
#pragma unroll
                for (int c = 3; c >= 0; --c) {
                    if (loss_bin_holds(above, h[c], remaining)) {
                        pick[0] = (uint32_t)(4 * lane + c);
                        pick[1] = remaining - above;
                        pick[2] = h[c];
                    }
                    above += h[c];
                }
            }
            __syncthreads();
            prefix = loss_extend(prefix, loss_uniform(pick[0]) & (uint32_t)(LOSS_BINS - 1), pass);
            remaining = loss_uniform(pick[1]);
            held = loss_uniform(pick[2]);
        }
        T = prefix;
        want = remaining;
        in_order = held != remaining;
    }

    partial[tid] = 0.0f;
    __syncthreads();
    uint32_t base = 0;                              // ties in the chunks before this one
    const int chunks = rows.chunks();
    for (int chunk = 0; chunk < chunks; ++chunk) {
        float sum;
        if (in_order) {
            const int row0 = chunk * LOSS_CHUNK_ROWS;
            ranks[tid] = 0;
            __syncthreads();
            rows.each(chunk, [&](int j, int, float d) {
                const unsigned long long ties = __ballot(loss_key(loss_error(KIND, d)) == T);
                if (lane == 0) ranks[(j - row0) * LOSS_WAVES + wave] = (uint32_t)__popcll(ties);
            });
            __syncthreads();
            // exclusive prefix over the 1024 (row, wave) counts in index order
            const uint32_t own = ranks[tid];
            uint32_t incl = own;
            for (int o = 1; o < 64; o <<= 1) {
                const uint32_t v = __shfl_up(incl, o);
                if (lane >= o) incl += v;
            }
            if (lane == 63) wave_count[wave] = incl;
            __syncthreads();
            uint32_t before = 0, total = 0;
#pragma unroll
            for (int w = 0; w < LOSS_WAVES; ++w) {
                const uint32_t c = wave_count[w];
                before += w < wave ? c : 0u;
                total += c;
            }
            ranks[tid] = base + before + incl - own;
            base += total;
            __syncthreads();
            sum = dx ? loss_sweep<KIND, true, true>(rows, chunk, T, want, ranks, dx, a.sink, a.scale, lane, wave)
                     : loss_sweep<KIND, true, false>(rows, chunk, T, want, ranks, dx, a.sink, a.scale, lane, wave);
            __syncthreads();                         // ranks[] is rewritten by the next chunk
        } else {
            sum = dx ? loss_sweep<KIND, false, true>(rows, chunk, T, want, ranks, dx, a.sink, a.scale, lane, wave)
                     : loss_sweep<KIND, false, false>(rows, chunk, T, want, ranks, dx, a.sink, a.scale, lane, wave);
        }
        sum = loss_wave_sum(sum);
        if (lane == 0) partial[chunk * LOSS_WAVES + wave] = sum;
    }
    __syncthreads();
    const float total = loss_block_sum(partial[tid], wave_sum, lane, wave);
    if (tid == 0) {
        const float mean = total / (float)a.k;
        a.means[blockIdx.x] = mean;
        if (a.per_image) a.per_image[blockIdx.x] = mean;
    }
}

// loss = mean of the B per-image means, added in a fixed order: a lane adds at most 64, then trees
__global__ __launch_bounds__(LOSS_BLOCK) void recon_loss_finish_kernel(const float* __restrict__ means, int B, float* __restrict__ loss) {
    __shared__ float wave_sum[LOSS_WAVES];
    const int tid = threadIdx.x;
    float v = 0.0f;
    for (int i = tid; i < B; i += LOSS_BLOCK) v += means[i];
    const float total = loss_block_sum(v, wave_sum, tid & 63, tid >> 6);
    if (tid == 0) loss[0] = total / (float)B;
}

// Encoder.reg_loss: one workgroup, one wave per row of z at a time (row r belongs to wave r % 16); the sum of squares of a row in
// fp64 by a butterfly, so every lane holds it.  The row's loss is added into the accumulator of lane (visit % 64) of the wave: a
// lane adds at most 64 rows for B <= 65536, then the same trees as above.
__global__ __launch_bounds__(LOSS_BLOCK) void latent_reg_kernel(const float* __restrict__ z, int B, int J, float* __restrict__ loss, float* __restrict__ dz) {
    __shared__ float wave_sum[LOSS_WAVES];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const double inv_B = 1.0 / (double)B;
    float acc = 0.0f;
    int visit = 0;
    for (int r = wave; r < B; r += LOSS_WAVES, ++visit) {
        const float* __restrict__ row = z + (size_t)r * (size_t)J;
        double s = 0.0;
        for (int c = lane; c < J; c += 64) {
            const double v = (double)row[c];
            s += v * v;
        }
        for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
        const double norm = reg_row_norm(s);
        if (lane == (visit & 63)) acc += reg_row_loss(norm);
        if (dz) {
            float* __restrict__ out = dz + (size_t)r * (size_t)J;
            for (int c = lane; c < J; c += 64) out[c] = reg_row_grad(row[c], norm, inv_B);
        }
    }
    const float total = loss_block_sum(acc, wave_sum, lane, wave);
    if (tid == 0) loss[0] = total / (float)B;
}

}  // namespace aae_loss
