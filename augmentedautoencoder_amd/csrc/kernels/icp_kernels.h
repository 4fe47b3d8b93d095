// The depth refinement's kernels: icp_points (ordered compaction of a depth image into float64 points),
// icp_stats (centroid and largest distance of a point list), icp_gather (the host-drawn subsample), icp_step (one ICP
// iteration of up to 16 problems) and icp_finish (best_fit_transform(A, src) per problem).  The arithmetic is icp_core.h's;
// here are only the splits over threads and blocks, chosen so that no result depends on them.
//
// Cross-block protocol: arrive-and-leave tickets only (block_ticket_arrive).  No block waits for another, every loop is
// bounded by an argument, partials cross blocks as 8-byte device-scope atomics on both sides.
#pragma once

#include <hip/hip_runtime.h>

#include "../device_intrinsics.h"
#include "icp_core.h"

namespace aae_icp {

constexpr int kIcpBlock = 256;                   // icp_points / icp_stats / icp_gather / icp_finish
constexpr int kIcpStepThreads = 512;             // icp_step: 8 waves scan disjoint eighths of the targets
constexpr int kIcpStepWaves = kIcpStepThreads / 64;

struct IcpProblems {                              // the problem table, in the kernel arguments
    int32_t n[ICP_MAX_PROBLEMS];
    int32_t mode[ICP_MAX_PROBLEMS];
};

// ---- icp_points ------------------------------------------------------------------------------------------------------
struct IcpPointsArgs {
    const float* depth;                           // image p at depth + p * img_stride, w[p] x h[p] dense
    long long img_stride;
    int32_t w[ICP_MAX_PROBLEMS], h[ICP_MAX_PROBLEMS];
    IcpCamera cam[ICP_MAX_PROBLEMS];
    double* pts;                                  // list p at pts + p * pts_stride (doubles), capacity w x h points
    long long pts_stride;
    int32_t* chunk_counts;                        // [P][chunk_stride]
    int chunk_stride;
    const double* stats;                          // nullptr: keep every point; else (centroid[3], radius, thresh) per problem
    int stats_stride;
    int32_t* counts;                              // counts[p * 2 + counts_off]
    int counts_off;
};

// chunk c = pixels [256 c, 256 c + 256) in row-major order.  WRITE = false: the chunk's number of points.  WRITE = true:
// the chunk adds up the counts in front of it and writes its points behind them (no look-back, no waiting).
template <bool WRITE>
__global__ __launch_bounds__(kIcpBlock) void icp_points(const IcpPointsArgs a) {
    __shared__ int s_wave[kIcpBlock / 64];
    __shared__ int s_base[kIcpBlock / 64];
    const int p = blockIdx.y, c = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int w = a.w[p], npix = w * a.h[p];
    if (c * kIcpBlock >= npix) return;
    const int i = c * kIcpBlock + tid;
    bool keep = false;
    double pt[3] = {0.0, 0.0, 0.0};
    if (i < npix) {
        const float d = a.depth[(long long)p * a.img_stride + i];
        if (icp_is_point(d)) {
            icp_backproject(a.cam[p], i % w, i / w, d, pt);
            keep = true;
            if (a.stats) {
                const double* st = a.stats + (long long)p * a.stats_stride;
                keep = icp_filter_keeps(pt, st, st[4]);
            }
        }
    }
    const unsigned long long mask = __builtin_amdgcn_ballot_w64(keep);
    if (lane == 0) s_wave[wave] = __builtin_popcountll(mask);
    if (WRITE) {
        int before = 0;
        for (int k = tid; k < c; k += kIcpBlock) before += a.chunk_counts[(long long)p * a.chunk_stride + k];
        for (int m = 32; m >= 1; m >>= 1) before += __shfl_xor(before, m, 64);
        if (lane == 0) s_base[wave] = before;
    }
    __syncthreads();
    int block_count = 0, wave_off = 0;
    for (int k = 0; k < kIcpBlock / 64; ++k) {
        if (k < wave) wave_off += s_wave[k];
        block_count += s_wave[k];
    }
    if (!WRITE) {
        if (tid == 0) a.chunk_counts[(long long)p * a.chunk_stride + c] = block_count;
        return;
    }
    int base = 0;
    for (int k = 0; k < kIcpBlock / 64; ++k) base += s_base[k];
    const int rank = base + wave_off + __builtin_popcountll(mask & ((1ull << lane) - 1ull));
    if (keep && rank >= 0 && rank < npix) {                                             // (w h is the list's capacity; counts of this image never exceed it)
        double* o = a.pts + (long long)p * a.pts_stride + (long long)rank * 3;
        o[0] = pt[0]; o[1] = pt[1]; o[2] = pt[2];
    }
    if (tid == 0 && (c + 1) * kIcpBlock >= npix) a.counts[p * 2 + a.counts_off] = base + block_count;
}

// ---- icp_stats -------------------------------------------------------------------------------------------------------
// one block per problem: centroid = mean, radius = largest distance from it (icp_utils.py:251-252), thresh = factor * radius
__global__ __launch_bounds__(kIcpBlock) void icp_stats(const double* pts, long long pts_stride, const int32_t* counts, int capacity, double factor,
                                                       double* stats, int stats_stride) {
    __shared__ double acc[3][ICP_LANES];
    __shared__ double cen[3];
    const int p = blockIdx.x, tid = threadIdx.x;
    int n = counts[p * 2];
    n = n < 0 ? 0 : (n > capacity ? capacity : n);
    const double* P = pts + (long long)p * pts_stride;
    double s0 = 0.0, s1 = 0.0, s2 = 0.0;
    for (int i = tid; i < n; i += ICP_LANES) { s0 += P[3 * i]; s1 += P[3 * i + 1]; s2 += P[3 * i + 2]; }
    acc[0][tid] = s0; acc[1][tid] = s1; acc[2][tid] = s2;
    __syncthreads();
    for (int s = ICP_LANES / 2; s > 0; s >>= 1) {
        if (tid < s) { acc[0][tid] += acc[0][tid + s]; acc[1][tid] += acc[1][tid + s]; acc[2][tid] += acc[2][tid + s]; }
        __syncthreads();
    }
    if (tid < 3) cen[tid] = acc[tid][0] / (double)n;
    __syncthreads();
    const double c0 = cen[0], c1 = cen[1], c2 = cen[2];
    double m = 0.0;
    for (int i = tid; i < n; i += ICP_LANES) {
        const double d2 = icp_dist2(P[3 * i], P[3 * i + 1], P[3 * i + 2], c0, c1, c2);
        m = d2 > m ? d2 : m;
    }
    __syncthreads();
    acc[0][tid] = m;
    __syncthreads();
    for (int s = ICP_LANES / 2; s > 0; s >>= 1) {
        if (tid < s) acc[0][tid] = acc[0][tid + s] > acc[0][tid] ? acc[0][tid + s] : acc[0][tid];
        __syncthreads();
    }
    if (tid == 0) {
        double* st = stats + (long long)p * stats_stride;
        const double radius = sqrt(acc[0][0]);
        st[0] = c0; st[1] = c1; st[2] = c2; st[3] = radius; st[4] = factor * radius;
    }
}

// ---- icp_gather ------------------------------------------------------------------------------------------------------
struct IcpGatherArgs {
    IcpProblems pr;
    const double* syn; long long syn_stride;
    const double* real; long long real_stride;
    const int32_t* counts;                        // [P][2]
    int syn_capacity, real_capacity;
    const int32_t* sub_syn; const int32_t* sub_real; int sub_stride;
    double* src; double* orig; double* dst; long long sub_pts_stride;
    int32_t* error;                               // [P], zeroed before the launch
};

__device__ __forceinline__ int icp_clamp_index(int idx, int count, int capacity, bool* bad) {
    int hi = count < capacity ? count : capacity;
    if (hi < 1) { *bad = true; hi = 1; }                                            // an empty list has no valid index; slot 0 exists whatever the count says
    if (idx < 0 || idx >= hi) { *bad = true; idx = idx < 0 ? 0 : hi - 1; }
    return idx;
}

__global__ __launch_bounds__(kIcpBlock) void icp_gather(const IcpGatherArgs a) {
    const int p = blockIdx.y, i = blockIdx.x * kIcpBlock + threadIdx.x;
    if (i >= a.pr.n[p]) return;
    bool bad = false;
    const int is = icp_clamp_index(a.sub_syn[(long long)p * a.sub_stride + i], a.counts[p * 2], a.syn_capacity, &bad);
    const int ir = icp_clamp_index(a.sub_real[(long long)p * a.sub_stride + i], a.counts[p * 2 + 1], a.real_capacity, &bad);
    const double* s = a.syn + (long long)p * a.syn_stride + (long long)is * 3;
    const double* r = a.real + (long long)p * a.real_stride + (long long)ir * 3;
    const long long o = (long long)p * a.sub_pts_stride + (long long)i * 3;
    for (int k = 0; k < 3; ++k) { a.src[o + k] = s[k]; a.orig[o + k] = s[k]; a.dst[o + k] = r[k]; }
    if (bad) atomicOr(&a.error[p], ICP_ERR_INDEX);
}

// ---- icp_step --------------------------------------------------------------------------------------------------------
struct IcpStepArgs {
    IcpProblems pr;
    double* src; const double* dst; long long sub_pts_stride;
    const double* stats; int stats_stride;        // the origin of the sums: the synthetic centroid
    double* partials;                             // [P][ICP_MAX_BLOCKS][ICP_NQ]
    IcpState* state;                              // [P]
    unsigned long long* tickets;                  // [P][kTicketSlotWords]
    unsigned nonce;
    int lds_points;                               // targets the dynamic LDS holds: >= every n
    int max_iterations;
    double tolerance;
    double* d2_out; int32_t* idx_out; int out_stride;          // optional: the last iteration's squared distances and matches
};

__host__ __device__ constexpr size_t icp_step_smem(int lds_points) {
    return (size_t)lds_points * 24 + (size_t)kIcpStepWaves * 64 * 12 + (size_t)ICP_BLOCK_POINTS * ICP_NQ * 8 + ICP_NQ * 8 + 16 * 8 + 16;
}

// Block (bx, p): source points [64 bx, 64 bx + 64) of problem p against all of its targets, staged once into LDS; wave w
// scans targets [w per, (w + 1) per) with broadcast reads, lane = source point; the waves' keys merge in wave order.  Then
// the block's 16 sums in point order, a ticket, and the last block of the problem adds the partials in block order, solves,
// moves the source points and advances the problem's state.  A finished problem's blocks return at once.
__global__ __launch_bounds__(kIcpStepThreads) void icp_step(const IcpStepArgs a) {
    const int p = blockIdx.y, bx = blockIdx.x, n = a.pr.n[p];
    if (bx * ICP_BLOCK_POINTS >= n) return;
    IcpState* st = a.state + p;
    if (st->done) return;
    AAE_DYN_SMEM(smem);
    double* tx = reinterpret_cast<double*>(smem);
    double* ty = tx + a.lds_points;
    double* tz = ty + a.lds_points;
    double* wbest = tz + a.lds_points;                                              // [waves][64]
    double* q = wbest + kIcpStepWaves * 64;                                        // [64][16]
    double* S = q + ICP_BLOCK_POINTS * ICP_NQ;                                     // [16]
    double* T = S + ICP_NQ;                                                        // [16]
    int* wbest_i = reinterpret_cast<int*>(T + 16);                                 // [waves][64]
    int* flag = wbest_i + kIcpStepWaves * 64;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int nblk = (n + ICP_BLOCK_POINTS - 1) / ICP_BLOCK_POINTS;
    double* src = a.src + (long long)p * a.sub_pts_stride;
    const double* dst = a.dst + (long long)p * a.sub_pts_stride;
    const double* org = a.stats + (long long)p * a.stats_stride;

    for (int j = tid; j < n; j += kIcpStepThreads) { tx[j] = dst[3 * j]; ty[j] = dst[3 * j + 1]; tz[j] = dst[3 * j + 2]; }
    const int i = bx * ICP_BLOCK_POINTS + lane;
    const bool valid = i < n;
    const double sx = valid ? src[3 * i] : 0.0, sy = valid ? src[3 * i + 1] : 0.0, sz = valid ? src[3 * i + 2] : 0.0;
    __syncthreads();

    const int per = (n + kIcpStepWaves - 1) / kIcpStepWaves;
    const int j0 = wave * per < n ? wave * per : n, j1 = j0 + per < n ? j0 + per : n;
    double best = __builtin_huge_val();
    int bi = j0 < n ? j0 : 0;                                                      // always a valid target, whatever the distances are
#pragma unroll 4
    for (int j = j0; j < j1; ++j) {
        const double d2 = icp_dist2(sx, sy, sz, tx[j], ty[j], tz[j]);
        if (d2 < best) { best = d2; bi = j; }                                      // ascending j: the lowest index of a tie
    }
    wbest[wave * 64 + lane] = best;
    wbest_i[wave * 64 + lane] = bi;
    __syncthreads();
    const int cnt = n - bx * ICP_BLOCK_POINTS < ICP_BLOCK_POINTS ? n - bx * ICP_BLOCK_POINTS : ICP_BLOCK_POINTS;
    if (tid < cnt) {
        double d2 = wbest[tid];
        int idx = wbest_i[tid];
        for (int w = 1; w < kIcpStepWaves; ++w)
            if (icp_key_less(wbest[w * 64 + tid], wbest_i[w * 64 + tid], d2, idx)) { d2 = wbest[w * 64 + tid]; idx = wbest_i[w * 64 + tid]; }
        const double dist = sqrt(d2);
        const double s3[3] = {sx, sy, sz}, d3[3] = {tx[idx], ty[idx], tz[idx]};
        icp_pair_terms(s3, d3, org, dist, q + tid * ICP_NQ);
        if (a.d2_out) a.d2_out[(long long)p * a.out_stride + i] = d2;
        if (a.idx_out) a.idx_out[(long long)p * a.out_stride + i] = idx;
    }
    __syncthreads();
    double* part = a.partials + ((long long)p * ICP_MAX_BLOCKS + bx) * ICP_NQ;
    if (tid < ICP_NQ) {
        double s = 0.0;
        for (int k = 0; k < cnt; ++k) s += q[k * ICP_NQ + tid];
        __hip_atomic_store(part + tid, s, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    if (!aae::block_ticket_arrive(a.tickets + (long long)p * aae::kTicketSlotWords, a.nonce, (unsigned)nblk, (unsigned)bx, flag)) return;

    if (tid < ICP_NQ) {
        const double* all = a.partials + (long long)p * ICP_MAX_BLOCKS * ICP_NQ;
        double s = 0.0;
        for (int b = 0; b < nblk; ++b) s += __hip_atomic_load(all + b * ICP_NQ + tid, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        S[tid] = s;
    }
    __syncthreads();
    if (tid == 0) {
        double Tl[16];
        const double mean = icp_solve(S, n, org, a.pr.mode[p], Tl);
        for (int k = 0; k < 16; ++k) T[k] = Tl[k];
        IcpState s = *st;
        icp_advance(&s, mean, a.tolerance, a.max_iterations);
        *st = s;
    }
    __syncthreads();
    for (int k = tid; k < n; k += kIcpStepThreads) icp_apply(T, src + 3 * k);       // every other block has read its points
}

// ---- icp_finish ------------------------------------------------------------------------------------------------------
struct IcpFinishArgs {
    IcpProblems pr;
    const double* orig; const double* src; long long sub_pts_stride;
    const double* stats; int stats_stride;
    const IcpState* state;
    double* T_out;                                // [P][16]
    int32_t* iterations_out;                      // [P]: the reference's i
    double* mean_error_out;                       // [P]
};

__global__ __launch_bounds__(kIcpBlock) void icp_finish(const IcpFinishArgs a) {
    __shared__ double acc[ICP_NQ][ICP_LANES];
    const int p = blockIdx.x, tid = threadIdx.x, n = a.pr.n[p];
    if (n == 0) {                                                                   // a problem left out of the call: the identity, i = -1
        if (tid < 16) a.T_out[p * 16 + tid] = (tid % 5 == 0) ? 1.0 : 0.0;
        if (tid == 0) { a.iterations_out[p] = -1; a.mean_error_out[p] = 0.0; }
        return;
    }
    const double* A = a.orig + (long long)p * a.sub_pts_stride;
    const double* B = a.src + (long long)p * a.sub_pts_stride;
    const double* org = a.stats + (long long)p * a.stats_stride;
    double s[ICP_NQ];
    for (int k = 0; k < ICP_NQ; ++k) s[k] = 0.0;
    for (int i = tid; i < n; i += ICP_LANES) {
        double q[ICP_NQ];
        icp_pair_terms(A + 3 * i, B + 3 * i, org, 0.0, q);
        for (int k = 0; k < ICP_NQ; ++k) s[k] += q[k];
    }
    for (int k = 0; k < ICP_NQ; ++k) acc[k][tid] = s[k];
    __syncthreads();
    for (int h = ICP_LANES / 2; h > 0; h >>= 1) {
        if (tid < h)
            for (int k = 0; k < ICP_NQ; ++k) acc[k][tid] += acc[k][tid + h];
        __syncthreads();
    }
    if (tid == 0) {
        double S[ICP_NQ], T[16];
        for (int k = 0; k < ICP_NQ; ++k) S[k] = acc[k][0];
        icp_solve(S, n, org, a.pr.mode[p], T);
        for (int k = 0; k < 16; ++k) a.T_out[p * 16 + k] = T[k];
        a.iterations_out[p] = a.state[p].iterations - 1;
        a.mean_error_out[p] = a.state[p].mean_error;
    }
}

}  // namespace aae_icp
