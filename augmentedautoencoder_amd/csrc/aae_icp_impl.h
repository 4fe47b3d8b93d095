// Host side of the depth refinement: the workspace layout and the launch sequences behind aae_icp_* (include/aae_hip.h).
// Part of aae_icp.hip.
#pragma once

#include <stdarg.h>
#include <stdio.h>
#include <string.h>

#include <atomic>

#include "../../include/aae_hip.h"
#include "kernels/icp_kernels.h"

namespace aae_host {
void set_last_error(const char* msg);          // aae_host_types.h: the thread's aae_last_error() text lives in aae_hip.hip
}

static_assert(AAE_ICP_MAX_PROBLEMS == ICP_MAX_PROBLEMS && AAE_ICP_MAX_POINTS == ICP_MAX_POINTS, "header and kernels disagree");
static_assert(AAE_ICP_DEPTH_ONLY == ICP_DEPTH_ONLY && AAE_ICP_NO_DEPTH == ICP_NO_DEPTH && AAE_ICP_NO_DEPTH_ZERO_T == ICP_NO_DEPTH_ZERO_T,
              "header and kernels disagree");

namespace aae_icp {

static int ifail(int code, const char* fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    aae_host::set_last_error(buf);
    return code;
}

#define AAE_ICP_TRY(expr)                                                                                             \
    do {                                                                                                              \
        hipError_t e__ = (expr);                                                                                      \
        if (e__ != hipSuccess)                                                                                        \
            return aae_icp::ifail(AAE_ERR_RUNTIME, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(e__), __FILE__, __LINE__); \
    } while (0)

#define AAE_ICP_MAX_DIM 4096
#define AAE_ICP_STATS 8                           /* doubles per problem: centroid[3], radius, thresh, spare                */

static inline size_t up256(size_t v) { return (v + 255) / 256 * 256; }

// block_ticket_arrive() nonces: unique per launch within the process, never 0
static unsigned next_nonce() {
    static std::atomic<unsigned> counter{1};
    unsigned n = counter.fetch_add(1, std::memory_order_relaxed);
    while (n == 0) n = counter.fetch_add(1, std::memory_order_relaxed);
    return n;
}

struct WsLayout {
    size_t syn, real, chunks_syn, chunks_real, stats, counts, src, orig, dst, partials, state, tickets, total;
    long long syn_stride, real_stride, sub_stride;          // doubles per problem
    int chunk_syn, chunk_real;                              // chunks per problem
};

static WsLayout ws_layout(const aae_icp_shape& s) {
    WsLayout l;
    const size_t P = (size_t)s.n_problems;
    l.syn_stride = (long long)s.W * s.H * 3;
    l.real_stride = (long long)s.crop_w * s.crop_h * 3;
    l.sub_stride = (long long)s.max_points * 3;
    l.chunk_syn = (s.W * s.H + kIcpBlock - 1) / kIcpBlock;
    l.chunk_real = (s.crop_w * s.crop_h + kIcpBlock - 1) / kIcpBlock;
    size_t o = 0;
    l.syn = o;         o += up256(P * l.syn_stride * sizeof(double));
    l.real = o;        o += up256(P * l.real_stride * sizeof(double));
    l.chunks_syn = o;  o += up256(P * l.chunk_syn * sizeof(int32_t));
    l.chunks_real = o; o += up256(P * l.chunk_real * sizeof(int32_t));
    l.stats = o;       o += up256(P * AAE_ICP_STATS * sizeof(double));
    l.counts = o;      o += up256(P * 2 * sizeof(int32_t));
    l.src = o;         o += up256(P * l.sub_stride * sizeof(double));
    l.orig = o;        o += up256(P * l.sub_stride * sizeof(double));
    l.dst = o;         o += up256(P * l.sub_stride * sizeof(double));
    l.partials = o;    o += up256(P * ICP_MAX_BLOCKS * ICP_NQ * sizeof(double));
    l.state = o;       o += up256(P * sizeof(IcpState));
    l.tickets = o;     o += up256(P * aae::kTicketSlotWords * sizeof(unsigned long long));
    l.total = o;
    return l;
}

static int check_shape(const aae_icp_shape* s, const void* ws, size_t ws_bytes, const char* who) {
    if (!s || !ws) return ifail(AAE_ERR_INVALID, "%s: null argument", who);
    if (s->n_problems < 1 || s->n_problems > AAE_ICP_MAX_PROBLEMS)
        return ifail(AAE_ERR_INVALID, "%s: %d problems outside [1,%d] per call", who, s->n_problems, AAE_ICP_MAX_PROBLEMS);
    if (s->max_points < 3 || s->max_points > AAE_ICP_MAX_POINTS)
        return ifail(AAE_ERR_INVALID, "%s: max_points %d outside [3,%d]", who, s->max_points, AAE_ICP_MAX_POINTS);
    if (s->W < 1 || s->H < 1 || s->W > AAE_ICP_MAX_DIM || s->H > AAE_ICP_MAX_DIM || s->crop_w < 1 || s->crop_h < 1 || s->crop_w > AAE_ICP_MAX_DIM ||
        s->crop_h > AAE_ICP_MAX_DIM)
        return ifail(AAE_ERR_UNSUPPORTED, "%s: frame %dx%d or crop %dx%d outside [1,%d]", who, s->W, s->H, s->crop_w, s->crop_h, AAE_ICP_MAX_DIM);
    const WsLayout l = ws_layout(*s);
    if (ws_bytes < l.total) return ifail(AAE_ERR_WORKSPACE, "%s: workspace of %zu bytes, %zu needed", who, ws_bytes, l.total);
    if (((uintptr_t)ws & 255) != 0) return ifail(AAE_ERR_WORKSPACE, "%s: workspace must be 256-byte aligned", who);
    return AAE_OK;
}

static int prepare_run(const aae_icp_shape* s, const float* syn_depth, const float* crop_depth, const int32_t* crop_dims, const double* K,
                       double factor, int32_t* counts_out, void* ws, size_t ws_bytes, void* stream_) {
    const char* who = "aae_icp_prepare";
    const int rc = check_shape(s, ws, ws_bytes, who);
    if (rc != AAE_OK) return rc;
    if (!syn_depth || !crop_depth || !crop_dims || !K || !counts_out) return ifail(AAE_ERR_INVALID, "%s: null argument", who);
    if (!(K[0] != 0.0) || !(K[4] != 0.0)) return ifail(AAE_ERR_INVALID, "%s: K[0,0] and K[1,1] must not be 0", who);
    const int P = s->n_problems;
    for (int p = 0; p < P; ++p) {
        const int h = crop_dims[2 * p], w = crop_dims[2 * p + 1];
        if (h < 1 || w < 1 || (long long)h * w > (long long)s->crop_w * s->crop_h)
            return ifail(AAE_ERR_INVALID, "%s: crop %d is %d x %d, the slots hold %d pixels", who, p, h, w, s->crop_w * s->crop_h);
    }
    const WsLayout l = ws_layout(*s);
    hipStream_t stream = (hipStream_t)stream_;
    char* base = (char*)ws;

    IcpPointsArgs a;
    memset(&a, 0, sizeof(a));
    a.depth = syn_depth;
    a.img_stride = (long long)s->W * s->H;
    for (int p = 0; p < P; ++p) {
        a.w[p] = s->W; a.h[p] = s->H;
        a.cam[p].K00 = K[0]; a.cam[p].K02 = K[2]; a.cam[p].K11 = K[4]; a.cam[p].K12 = K[5];
    }
    a.pts = (double*)(base + l.syn);
    a.pts_stride = l.syn_stride;
    a.chunk_counts = (int32_t*)(base + l.chunks_syn);
    a.chunk_stride = l.chunk_syn;
    a.stats = nullptr;
    a.stats_stride = AAE_ICP_STATS;
    a.counts = (int32_t*)(base + l.counts);
    a.counts_off = 0;
    const dim3 block(kIcpBlock);
    AAE_LAUNCH(icp_points<false>, dim3(l.chunk_syn, P), block, 0, stream, a);
    AAE_LAUNCH(icp_points<true>, dim3(l.chunk_syn, P), block, 0, stream, a);
    AAE_LAUNCH(icp_stats, dim3(P), block, 0, stream, (const double*)(base + l.syn), l.syn_stride, (const int32_t*)(base + l.counts), s->W * s->H,
               factor, (double*)(base + l.stats), AAE_ICP_STATS);

    IcpPointsArgs b = a;
    b.depth = crop_depth;
    b.img_stride = (long long)s->crop_w * s->crop_h;
    for (int p = 0; p < P; ++p) {
        b.h[p] = crop_dims[2 * p]; b.w[p] = crop_dims[2 * p + 1];
        b.cam[p].K02 = (double)(crop_dims[2 * p] / 2);                         // icp_utils.py:256-257: shape[0] / 2 for x, shape[1] / 2 for y, floored
        b.cam[p].K12 = (double)(crop_dims[2 * p + 1] / 2);
    }
    b.pts = (double*)(base + l.real);
    b.pts_stride = l.real_stride;
    b.chunk_counts = (int32_t*)(base + l.chunks_real);
    b.chunk_stride = l.chunk_real;
    b.stats = (const double*)(base + l.stats);
    b.counts_off = 1;
    AAE_LAUNCH(icp_points<false>, dim3(l.chunk_real, P), block, 0, stream, b);
    AAE_LAUNCH(icp_points<true>, dim3(l.chunk_real, P), block, 0, stream, b);
    AAE_ICP_TRY(hipGetLastError());
    AAE_ICP_TRY(hipMemcpyAsync(counts_out, base + l.counts, (size_t)P * 2 * sizeof(int32_t), hipMemcpyDeviceToHost, stream));
    return AAE_OK;
}

// kernel_ms: nullptr, or max_iterations + 2 floats (the timed variant: events around every launch, then a synchronise)
static int refine_run(const aae_icp_shape* s, const int32_t* n_points, const int32_t* sub_syn, const int32_t* sub_real, const int32_t* modes,
                      int max_iterations, double tolerance, double* T_out, int32_t* iterations_out, double* mean_error_out, int32_t* error_out,
                      double* d2_out, int32_t* idx_out, void* ws, size_t ws_bytes, void* stream_, float* kernel_ms, const char* who) {
    const int rc = check_shape(s, ws, ws_bytes, who);
    if (rc != AAE_OK) return rc;
    if (!n_points || !sub_syn || !sub_real || !modes || !T_out || !iterations_out || !mean_error_out || !error_out)
        return ifail(AAE_ERR_INVALID, "%s: null argument", who);
    if (max_iterations < 1 || max_iterations > 1000) return ifail(AAE_ERR_INVALID, "%s: max_iterations %d outside [1,1000]", who, max_iterations);
    const int P = s->n_problems;
    IcpProblems pr;
    memset(&pr, 0, sizeof(pr));
    int n_max = 0;
    for (int p = 0; p < P; ++p) {
        if (n_points[p] != 0 && (n_points[p] < 3 || n_points[p] > s->max_points))                // 0: the problem is left out
            return ifail(AAE_ERR_INVALID, "%s: problem %d has %d points, outside [3,%d]", who, p, n_points[p], s->max_points);
        if (modes[p] & ~(AAE_ICP_DEPTH_ONLY | AAE_ICP_NO_DEPTH | AAE_ICP_NO_DEPTH_ZERO_T)) return ifail(AAE_ERR_INVALID, "%s: unknown mode bits %d", who, modes[p]);
        pr.n[p] = n_points[p];
        pr.mode[p] = modes[p];
        n_max = n_points[p] > n_max ? n_points[p] : n_max;
    }
    if (n_max == 0) n_max = 1;                                                                   // grids of one block that returns at once
    const WsLayout l = ws_layout(*s);
    hipStream_t stream = (hipStream_t)stream_;
    char* base = (char*)ws;
    const size_t smem = icp_step_smem(n_max);
    // per device and cheap: set on every call, so a second GPU of the process is covered too
    AAE_ICP_TRY(hipFuncSetAttribute((const void*)icp_step, hipFuncAttributeMaxDynamicSharedMemorySize, (int)icp_step_smem(ICP_MAX_POINTS)));

    const int n_launch = max_iterations + 2;
    hipEvent_t* ev = nullptr;
    if (kernel_ms) {
        ev = new hipEvent_t[n_launch + 1]();
        for (int i = 0; i <= n_launch; ++i) {
            hipError_t e = hipEventCreate(&ev[i]);
            if (e != hipSuccess) {
                for (int k = 0; k < i; ++k) (void)hipEventDestroy(ev[k]);
                delete[] ev;
                return ifail(AAE_ERR_RUNTIME, "%s: hipEventCreate: %s", who, hipGetErrorString(e));
            }
        }
    }
    int stage = 0;
    hipError_t err = hipSuccess;
#define AAE_ICP_MARK() do { if (ev && err == hipSuccess) err = hipEventRecord(ev[stage++], stream); } while (0)
    err = hipMemsetAsync(error_out, 0, (size_t)P * sizeof(int32_t), stream);
    if (err == hipSuccess) err = hipMemsetAsync(base + l.state, 0, (size_t)P * sizeof(IcpState), stream);

    IcpGatherArgs g;
    memset(&g, 0, sizeof(g));
    g.pr = pr;
    g.syn = (const double*)(base + l.syn); g.syn_stride = l.syn_stride;
    g.real = (const double*)(base + l.real); g.real_stride = l.real_stride;
    g.counts = (const int32_t*)(base + l.counts);
    g.syn_capacity = s->W * s->H; g.real_capacity = s->crop_w * s->crop_h;
    g.sub_syn = sub_syn; g.sub_real = sub_real; g.sub_stride = s->max_points;
    g.src = (double*)(base + l.src); g.orig = (double*)(base + l.orig); g.dst = (double*)(base + l.dst);
    g.sub_pts_stride = l.sub_stride;
    g.error = error_out;
    AAE_ICP_MARK();
    if (err == hipSuccess) AAE_LAUNCH(icp_gather, dim3((n_max + kIcpBlock - 1) / kIcpBlock, P), dim3(kIcpBlock), 0, stream, g);

    IcpStepArgs a;
    memset(&a, 0, sizeof(a));
    a.pr = pr;
    a.src = g.src; a.dst = g.dst; a.sub_pts_stride = l.sub_stride;
    a.stats = (const double*)(base + l.stats); a.stats_stride = AAE_ICP_STATS;
    a.partials = (double*)(base + l.partials);
    a.state = (IcpState*)(base + l.state);
    a.tickets = (unsigned long long*)(base + l.tickets);
    a.lds_points = n_max;
    a.max_iterations = max_iterations;
    a.tolerance = tolerance;
    a.d2_out = d2_out; a.idx_out = idx_out; a.out_stride = s->max_points;
    const dim3 sgrid((n_max + ICP_BLOCK_POINTS - 1) / ICP_BLOCK_POINTS, P);
    for (int it = 0; it < max_iterations && err == hipSuccess; ++it) {
        a.nonce = next_nonce();
        AAE_ICP_MARK();
        AAE_LAUNCH(icp_step, sgrid, dim3(kIcpStepThreads), smem, stream, a);
    }

    IcpFinishArgs f;
    memset(&f, 0, sizeof(f));
    f.pr = pr;
    f.orig = g.orig; f.src = g.src; f.sub_pts_stride = l.sub_stride;
    f.stats = a.stats; f.stats_stride = AAE_ICP_STATS;
    f.state = a.state;
    f.T_out = T_out; f.iterations_out = iterations_out; f.mean_error_out = mean_error_out;
    AAE_ICP_MARK();
    if (err == hipSuccess) AAE_LAUNCH(icp_finish, dim3(P), dim3(kIcpBlock), 0, stream, f);
    AAE_ICP_MARK();
#undef AAE_ICP_MARK
    if (err == hipSuccess) err = hipGetLastError();
    if (ev) {
        if (err == hipSuccess) err = hipEventSynchronize(ev[n_launch]);
        for (int i = 0; i < n_launch && err == hipSuccess; ++i) err = hipEventElapsedTime(&kernel_ms[i], ev[i], ev[i + 1]);
        for (int i = 0; i <= n_launch; ++i) (void)hipEventDestroy(ev[i]);
        delete[] ev;
    }
    if (err != hipSuccess) return ifail(AAE_ERR_RUNTIME, "%s: %s", who, hipGetErrorString(err));
    return AAE_OK;
}

}  // namespace aae_icp

extern "C" {

size_t aae_icp_workspace_bytes(int n_problems, int max_points, int W, int H, int crop_w, int crop_h) {
    if (n_problems < 1 || n_problems > AAE_ICP_MAX_PROBLEMS || max_points < 3 || max_points > AAE_ICP_MAX_POINTS || W < 1 || H < 1 || crop_w < 1 ||
        crop_h < 1 || W > AAE_ICP_MAX_DIM || H > AAE_ICP_MAX_DIM || crop_w > AAE_ICP_MAX_DIM || crop_h > AAE_ICP_MAX_DIM)
        return 0;
    const aae_icp_shape s = {n_problems, max_points, W, H, crop_w, crop_h};
    return aae_icp::ws_layout(s).total;
}

int aae_icp_workspace_info(const aae_icp_shape* shape, int problem, int what, size_t* offset_bytes, size_t* capacity) {
    using namespace aae_icp;
    if (!shape || !offset_bytes || !capacity) return ifail(AAE_ERR_INVALID, "aae_icp_workspace_info: null argument");
    if (aae_icp_workspace_bytes(shape->n_problems, shape->max_points, shape->W, shape->H, shape->crop_w, shape->crop_h) == 0 || problem < 0 ||
        problem >= shape->n_problems)
        return ifail(AAE_ERR_INVALID, "aae_icp_workspace_info: bad shape or problem %d", problem);
    const WsLayout l = ws_layout(*shape);
    switch (what) {
    case 0: *offset_bytes = l.syn + (size_t)problem * l.syn_stride * sizeof(double); *capacity = (size_t)shape->W * shape->H; break;
    case 1: *offset_bytes = l.real + (size_t)problem * l.real_stride * sizeof(double); *capacity = (size_t)shape->crop_w * shape->crop_h; break;
    case 2: *offset_bytes = l.stats + (size_t)problem * AAE_ICP_STATS * sizeof(double); *capacity = 5; break;
    default: return ifail(AAE_ERR_INVALID, "aae_icp_workspace_info: unknown item %d", what);
    }
    return AAE_OK;
}

int aae_icp_prepare(const aae_icp_shape* shape, const float* syn_depth, const float* crop_depth, const int32_t* crop_dims, const double* K,
                    double max_mean_dist_factor, int32_t* counts_out, void* workspace, size_t ws_bytes, void* stream) {
    return aae_icp::prepare_run(shape, syn_depth, crop_depth, crop_dims, K, max_mean_dist_factor, counts_out, workspace, ws_bytes, stream);
}

int aae_icp_refine(const aae_icp_shape* shape, const int32_t* n_points, const int32_t* sub_syn, const int32_t* sub_real, const int32_t* modes,
                   int max_iterations, double tolerance, double* T_out, int32_t* iterations_out, double* mean_error_out, int32_t* error_out,
                   double* d2_out, int32_t* idx_out, void* workspace, size_t ws_bytes, void* stream) {
    return aae_icp::refine_run(shape, n_points, sub_syn, sub_real, modes, max_iterations, tolerance, T_out, iterations_out, mean_error_out, error_out,
                               d2_out, idx_out, workspace, ws_bytes, stream, nullptr, "aae_icp_refine");
}

int aae_icp_refine_timed(const aae_icp_shape* shape, const int32_t* n_points, const int32_t* sub_syn, const int32_t* sub_real, const int32_t* modes,
                         int max_iterations, double tolerance, double* T_out, int32_t* iterations_out, double* mean_error_out, int32_t* error_out,
                         double* d2_out, int32_t* idx_out, void* workspace, size_t ws_bytes, void* stream, float* kernel_ms) {
    if (!kernel_ms) return aae_icp::ifail(AAE_ERR_INVALID, "aae_icp_refine_timed: null argument");
    return aae_icp::refine_run(shape, n_points, sub_syn, sub_real, modes, max_iterations, tolerance, T_out, iterations_out, mean_error_out, error_out,
                               d2_out, idx_out, workspace, ws_bytes, stream, kernel_ms, "aae_icp_refine_timed");
}

}  // extern "C"
