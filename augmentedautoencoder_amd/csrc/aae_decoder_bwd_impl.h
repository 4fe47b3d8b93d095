// Host side of the decoder's backward pass (kernels/decoder_bwd_f32.h): the argument checks, the launch plan of a stage (tile widths,
// K splits, workspace layout), the launches behind aae_upconv_backward / aae_dense_backward / aae_decoder_backward (include/aae_hip.h)
// and the labels of what ran.  Part of aae_decoder_bwd.hip; the CPU emulator's driver (tests/emu/decoder_bwd_emu.cpp) includes it too.
#pragma once

#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>

#include <string>
#include <vector>

#include "../../include/aae_hip.h"
#include "kernels/decoder_bwd_f32.h"

namespace aae_host {
void set_last_error(const char* msg);          // aae_host_types.h: the thread's aae_last_error() text lives in aae_hip.hip
}

namespace aae_bwd {

constexpr size_t BWD_WS_ALIGN = 256;
constexpr int BWD_TARGET_BLOCKS = 512;         // a weight-gradient / dz grid below this splits K (two blocks per CU)
constexpr int BWD_MAX_SPLITS = 64;
constexpr long long BWD_MAX_ELEMS = 0x7FFFFFFFll;      // the kernels index pixels and small tensors with int

static thread_local std::vector<std::string> t_labels;            // what the last call of this thread launched
static thread_local std::vector<hipEvent_t>* t_events = nullptr;  // aae_decoder_backward_timed: an event after every launch

static int bfail(int code, const char* fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    aae_host::set_last_error(buf);
    return code;
}

static void launched(hipStream_t stream, const char* fmt, ...) {
    char buf[256];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    t_labels.push_back(buf);
    if (t_events) {
        hipEvent_t e;
        if (hipEventCreate(&e) == hipSuccess) {
            (void)hipEventRecord(e, stream);
            t_events->push_back(e);
        }
    }
}

static inline size_t ws_align(size_t bytes) { return (bytes + BWD_WS_ALIGN - 1) / BWD_WS_ALIGN * BWD_WS_ALIGN; }
static inline int ceil_div_i(long long a, long long b) { return (int)((a + b - 1) / b); }
static inline int tile_nt(int n) { return n <= 32 ? 1 : (n <= 64 ? 2 : 4); }

// K splits of a grid of `tiles` blocks over `slabs` slabs: enough blocks to fill the chip, no empty split
static void choose_bwd_splits(int tiles, int slabs, int* splits, int* per) {
    int s = ceil_div_i(BWD_TARGET_BLOCKS, tiles);
    if (s > BWD_MAX_SPLITS) s = BWD_MAX_SPLITS;
    if (s > slabs) s = slabs;
    if (s < 1) s = 1;
    *per = ceil_div_i(slabs, s);
    *splits = ceil_div_i(slabs, *per);
}

struct ColumnSumPlan {
    int cw = 4, chunks = 1, rows_per_chunk = 1;
};

static ColumnSumPlan plan_column_sums(long long rows, int C) {
    ColumnSumPlan p;
    while (p.cw < 64 && p.cw < C) p.cw *= 2;
    const int lanes = BWD_BLOCK / p.cw;
    long long chunks = (rows + 8ll * lanes - 1) / (8ll * lanes);
    if (chunks > BWD_MAX_CHUNKS) chunks = BWD_MAX_CHUNKS;
    if (chunks < 1) chunks = 1;
    p.rows_per_chunk = (int)((rows + chunks - 1) / chunks);
    p.chunks = (int)((rows + p.rows_per_chunk - 1) / p.rows_per_chunk);
    return p;
}

struct StagePlan {
    StageGeom g;
    long long out_elems = 0;        // B * UH * UW * Cout
    ColumnSumPlan sums;
    // weight gradient
    int rows_per_phase = 0, w_nt = 1, w_row_tiles = 0, w_col_tiles = 0, w_splits = 1, w_slabs_per_split = 1, kpix = 0;
    // data gradient
    int C4 = 0, kslots = 0, d_nt = 1, d_row_tiles = 0, d_col_tiles = 0;
    // workspace
    size_t off_delta = 0, off_sums = 0, off_wf = 0, off_partial = 0, total = 0;
};

static int plan_stage(const aae_upconv_backward_desc* d, bool with_g_in, StagePlan& p, const char* who) {
    if (d->B < 1 || d->H < 1 || d->W < 1 || d->Cin < 1 || d->UH < 1 || d->UW < 1 || d->Cout < 1 || d->KS < 1 || (d->KS & 1) == 0)
        return bfail(AAE_ERR_INVALID, "%s: non-positive shape or even kernel size (B %d, %dx%dx%d -> %dx%dx%d, KS %d)", who, d->B, d->H, d->W, d->Cin, d->UH, d->UW, d->Cout, d->KS);
    if (d->act != BWD_ACT_RELU && d->act != BWD_ACT_SIGMOID) return bfail(AAE_ERR_INVALID, "%s: activation %d is neither ReLU (0) nor sigmoid (1)", who, d->act);
    const bool x2 = d->UH == 2 * d->H && d->UW == 2 * d->W, x1 = d->UH == d->H && d->UW == d->W;
    if (!x2 && !x1)
        return bfail(AAE_ERR_UNSUPPORTED, "%s: the backward pass of a %dx%d -> %dx%d resize is not built: only exact 2x and 1x stages train", who, d->H, d->W, d->UH, d->UW);
    const long long in_elems = (long long)d->B * d->H * d->W * d->Cin, out_elems = (long long)d->B * d->UH * d->UW * d->Cout;
    const long long w_elems = (long long)d->KS * d->KS * d->Cin * d->Cout;
    p.g = make_geom(d->B, d->H, d->W, d->Cin, d->Cout, d->KS, x2 ? 2 : 1);
    p.C4 = (d->Cout + 3) / 4;
    const long long wf_elems = (long long)p.g.P * p.g.U * p.g.U * p.C4 * d->Cin * 4;
    if (in_elems > BWD_MAX_ELEMS || out_elems > BWD_MAX_ELEMS || w_elems > BWD_MAX_ELEMS || wf_elems > BWD_MAX_ELEMS)
        return bfail(AAE_ERR_UNSUPPORTED, "%s: a tensor of this stage has 2^31 elements or more (input %lld, output %lld, weights %lld); use a smaller batch", who, in_elems, out_elems, w_elems);
    p.out_elems = out_elems;
    p.sums = plan_column_sums((long long)d->B * d->UH * d->UW, d->Cout);
    p.kpix = d->B * d->H * d->W;
    p.rows_per_phase = p.g.U * p.g.U * d->Cin;
    p.w_nt = tile_nt(d->Cout);
    p.w_row_tiles = ceil_div_i(p.rows_per_phase, BWD_BM);
    p.w_col_tiles = ceil_div_i(d->Cout, 32 * p.w_nt);
    choose_bwd_splits(p.g.P * p.w_row_tiles * p.w_col_tiles, ceil_div_i(p.kpix, BWD_BK), &p.w_splits, &p.w_slabs_per_split);
    p.kslots = p.g.P * p.g.U * p.g.U * p.C4;
    p.d_nt = tile_nt(d->Cin);
    p.d_row_tiles = ceil_div_i(p.kpix, BWD_BM);
    p.d_col_tiles = ceil_div_i(d->Cin, 32 * p.d_nt);
    size_t off = 0;
    p.off_delta = off; off += ws_align((size_t)out_elems * sizeof(float));
    p.off_sums = off; off += ws_align((size_t)p.sums.chunks * d->Cout * sizeof(float));
    p.off_wf = off; if (with_g_in) off += ws_align((size_t)wf_elems * sizeof(float));
    p.off_partial = off; off += ws_align((size_t)p.w_splits * p.g.P * p.rows_per_phase * d->Cout * sizeof(float));
    p.total = off;
    return AAE_OK;
}

static bool misaligned(const void* p) { return ((uintptr_t)p & 15) != 0; }

static void launch_delta_sums(const float* g_out, const float* a_out, float* delta, float* partial, float* db, long long rows, int C, int act,
                              const ColumnSumPlan& sp, hipStream_t stream, const char* name) {
    DeltaBiasArgs a;
    a.g_out = g_out; a.a_out = a_out; a.delta = delta; a.partial = partial; a.rows = (int)rows; a.C = C; a.act = act; a.cw = sp.cw; a.rows_per_chunk = sp.rows_per_chunk;
    AAE_LAUNCH(delta_bias_kernel, dim3((unsigned)ceil_div_i(C, sp.cw), (unsigned)sp.chunks), dim3(BWD_BLOCK), 0, stream, a);
    launched(stream, "%s:delta_bias rows=%lld C=%d chunks=%d", name, rows, C, sp.chunks);
    AAE_LAUNCH(column_sum_finish_kernel, dim3((unsigned)ceil_div_i(C, BWD_BLOCK)), dim3(BWD_BLOCK), 0, stream, (const float*)partial, sp.chunks, C, db);
    launched(stream, "%s:column_sum_finish C=%d", name, C);
}

template <int NT>
static void launch_wgrad_nt(const WgradArgs& a, unsigned grid, hipStream_t stream) { AAE_LAUNCH((wgrad_kernel<NT>), dim3(grid), dim3(BWD_BLOCK), 0, stream, a); }
template <int NT>
static void launch_dgrad_nt(const DgradArgs& a, unsigned grid, hipStream_t stream) { AAE_LAUNCH((dgrad_kernel<NT>), dim3(grid), dim3(BWD_BLOCK), 0, stream, a); }
template <int NT>
static void launch_dz_nt(const DenseDzArgs& a, unsigned grid, hipStream_t stream) { AAE_LAUNCH((dense_dz_kernel<NT>), dim3(grid), dim3(BWD_BLOCK), 0, stream, a); }

static inline unsigned grid_for(long long total) {
    long long b = (total + BWD_BLOCK - 1) / BWD_BLOCK;
    return (unsigned)(b > 4096 ? 4096 : (b < 1 ? 1 : b));
}

static int upconv_backward_impl(const aae_upconv_backward_desc* d, const float* a_in, const float* a_out, const float* g_out, const float* w, float* dw, float* db,
                                float* g_in, void* workspace, size_t ws_bytes, hipStream_t stream, const char* name, const char* who) {
    if (!d || !a_in || !a_out || !g_out || !w || !dw || !db || !workspace)
        return bfail(AAE_ERR_INVALID, "%s: null argument (desc, a_in, a_out, g_out, w, dw, db and workspace are required)", who);
    StagePlan p;
    if (int rc = plan_stage(d, g_in != nullptr, p, who)) return rc;
    if (misaligned(a_in) || misaligned(a_out) || misaligned(g_out) || misaligned(w) || misaligned(dw) || misaligned(db) || misaligned(g_in))
        return bfail(AAE_ERR_INVALID, "%s: every tensor must be 16-byte aligned", who);
    if (ws_bytes < p.total || ((uintptr_t)workspace & (BWD_WS_ALIGN - 1)))
        return bfail(AAE_ERR_WORKSPACE, "%s: workspace %p of %zu bytes; %zu bytes, %zu-byte aligned, are needed", who, workspace, ws_bytes, p.total, BWD_WS_ALIGN);
    unsigned char* base = static_cast<unsigned char*>(workspace);
    float* delta = reinterpret_cast<float*>(base + p.off_delta);
    float* sums = reinterpret_cast<float*>(base + p.off_sums);
    float* wf = reinterpret_cast<float*>(base + p.off_wf);
    float* partial = reinterpret_cast<float*>(base + p.off_partial);
    const StageGeom& g = p.g;

    launch_delta_sums(g_out, a_out, delta, sums, db, (long long)d->B * d->UH * d->UW, d->Cout, d->act, p.sums, stream, name);

    WgradArgs wa;
    wa.a_in = a_in; wa.delta = delta; wa.partial = partial; wa.g = g; wa.rows_per_phase = p.rows_per_phase; wa.row_tiles = p.w_row_tiles; wa.col_tiles = p.w_col_tiles;
    wa.splits = p.w_splits; wa.slabs_per_split = p.w_slabs_per_split; wa.kpix = p.kpix;
    const unsigned wgrid = (unsigned)(g.P * p.w_splits * p.w_row_tiles * p.w_col_tiles);
    if (p.w_nt == 1) launch_wgrad_nt<1>(wa, wgrid, stream);
    else if (p.w_nt == 2) launch_wgrad_nt<2>(wa, wgrid, stream);
    else launch_wgrad_nt<4>(wa, wgrid, stream);
    launched(stream, "%s:wgrad_mfma_f32 %d phases x (M=%d N=%d K=%d) tiles=%dx%d nt=%d splits=%d", name, g.P, p.rows_per_phase, d->Cout, p.kpix, p.w_row_tiles, p.w_col_tiles,
             p.w_nt, p.w_splits);
    WgradReduceArgs ra;
    ra.partial = partial; ra.dw = dw; ra.g = g; ra.rows_per_phase = p.rows_per_phase; ra.splits = p.w_splits; ra.total = d->KS * d->KS * d->Cin * d->Cout;
    AAE_LAUNCH(wgrad_reduce_kernel, dim3(grid_for(ra.total)), dim3(BWD_BLOCK), 0, stream, ra);
    launched(stream, "%s:wgrad_reduce_unfold phases=%d splits=%d", name, g.P, p.w_splits);

    if (g_in) {
        FoldArgs fa;
        fa.w = w; fa.wf = wf; fa.g = g; fa.C4 = p.C4; fa.total = p.kslots * d->Cin * 4;
        AAE_LAUNCH(fold_weights_kernel, dim3(grid_for(fa.total)), dim3(BWD_BLOCK), 0, stream, fa);
        launched(stream, "%s:fold_weights phases=%d taps=%dx%d", name, g.P, g.U, g.U);
        DgradArgs da;
        da.delta = delta; da.wf = wf; da.g_in = g_in; da.g = g; da.C4 = p.C4; da.kslots = p.kslots; da.M = p.kpix; da.row_tiles = p.d_row_tiles; da.col_tiles = p.d_col_tiles;
        const unsigned dgrid = (unsigned)(p.d_row_tiles * p.d_col_tiles);
        if (p.d_nt == 1) launch_dgrad_nt<1>(da, dgrid, stream);
        else if (p.d_nt == 2) launch_dgrad_nt<2>(da, dgrid, stream);
        else launch_dgrad_nt<4>(da, dgrid, stream);
        launched(stream, "%s:dgrad_mfma_f32 M=%d N=%d K=%d tiles=%dx%d nt=%d splits=1", name, p.kpix, d->Cin, 4 * p.kslots, p.d_row_tiles, p.d_col_tiles, p.d_nt);
    }
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return bfail(AAE_ERR_RUNTIME, "%s: launch failed: %s", who, hipGetErrorString(e));
    return AAE_OK;
}

struct DensePlan {
    ColumnSumPlan sums;
    int nt = 1, row_tiles = 0, col_tiles = 0, splits = 1, slabs_per_split = 1;
    size_t off_delta = 0, off_sums = 0, off_partial = 0, total = 0;
};

static int plan_dense(const aae_dense_backward_desc* d, bool with_dz, DensePlan& p, const char* who) {
    if (d->B < 1 || d->J < 1 || d->U < 1) return bfail(AAE_ERR_INVALID, "%s: B = %d, J = %d, U = %d", who, d->B, d->J, d->U);
    if ((long long)d->B * d->U > BWD_MAX_ELEMS || (long long)d->J * d->U > BWD_MAX_ELEMS || (long long)d->B * d->J > BWD_MAX_ELEMS)
        return bfail(AAE_ERR_UNSUPPORTED, "%s: a tensor of this layer has 2^31 elements or more (B %d, J %d, U %d)", who, d->B, d->J, d->U);
    p.sums = plan_column_sums(d->B, d->U);
    p.nt = tile_nt(d->J);
    p.row_tiles = ceil_div_i(d->B, BWD_BM);
    p.col_tiles = ceil_div_i(d->J, 32 * p.nt);
    choose_bwd_splits(p.row_tiles * p.col_tiles, ceil_div_i(d->U, BWD_BK), &p.splits, &p.slabs_per_split);
    size_t off = 0;
    p.off_delta = off; off += ws_align((size_t)d->B * d->U * sizeof(float));
    p.off_sums = off; off += ws_align((size_t)p.sums.chunks * d->U * sizeof(float));
    p.off_partial = off; if (with_dz) off += ws_align((size_t)p.splits * d->B * d->J * sizeof(float));
    p.total = off;
    return AAE_OK;
}

static int dense_backward_impl(const aae_dense_backward_desc* d, const float* z, const float* a_out, const float* g_out, const float* w, float* dw, float* db, float* dz,
                               void* workspace, size_t ws_bytes, hipStream_t stream, const char* who) {
    if (!d || !z || !a_out || !g_out || !w || !dw || !db || !workspace)
        return bfail(AAE_ERR_INVALID, "%s: null argument (desc, z, a_out, g_out, w, dw, db and workspace are required)", who);
    DensePlan p;
    if (int rc = plan_dense(d, dz != nullptr, p, who)) return rc;
    if (misaligned(z) || misaligned(a_out) || misaligned(g_out) || misaligned(w) || misaligned(dw) || misaligned(db) || misaligned(dz))
        return bfail(AAE_ERR_INVALID, "%s: every tensor must be 16-byte aligned", who);
    if (ws_bytes < p.total || ((uintptr_t)workspace & (BWD_WS_ALIGN - 1)))
        return bfail(AAE_ERR_WORKSPACE, "%s: workspace %p of %zu bytes; %zu bytes, %zu-byte aligned, are needed", who, workspace, ws_bytes, p.total, BWD_WS_ALIGN);
    unsigned char* base = static_cast<unsigned char*>(workspace);
    float* delta = reinterpret_cast<float*>(base + p.off_delta);
    float* sums = reinterpret_cast<float*>(base + p.off_sums);
    float* partial = reinterpret_cast<float*>(base + p.off_partial);
    launch_delta_sums(g_out, a_out, delta, sums, db, d->B, d->U, BWD_ACT_RELU, p.sums, stream, "dense");
    AAE_LAUNCH(dense_dw_kernel, dim3(grid_for((long long)d->J * d->U)), dim3(BWD_BLOCK), 0, stream, z, (const float*)delta, dw, d->B, d->J, d->U);
    launched(stream, "dense:dw_plain M=%d N=%d K=%d", d->J, d->U, d->B);
    if (dz) {
        DenseDzArgs a;
        a.delta = delta; a.w = w; a.partial = partial; a.B = d->B; a.J = d->J; a.U = d->U; a.row_tiles = p.row_tiles; a.col_tiles = p.col_tiles; a.splits = p.splits;
        a.slabs_per_split = p.slabs_per_split;
        const unsigned grid = (unsigned)(p.splits * p.row_tiles * p.col_tiles);
        if (p.nt == 1) launch_dz_nt<1>(a, grid, stream);
        else if (p.nt == 2) launch_dz_nt<2>(a, grid, stream);
        else launch_dz_nt<4>(a, grid, stream);
        launched(stream, "dense:dz_mfma_f32 M=%d N=%d K=%d tiles=%dx%d nt=%d splits=%d", d->B, d->J, d->U, p.row_tiles, p.col_tiles, p.nt, p.splits);
        AAE_LAUNCH(splitk_sum_kernel, dim3(grid_for((long long)d->B * d->J)), dim3(BWD_BLOCK), 0, stream, (const float*)partial, p.splits, d->B * d->J, dz);
        launched(stream, "dense:dz_reduce splits=%d", p.splits);
    }
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return bfail(AAE_ERR_RUNTIME, "%s: launch failed: %s", who, hipGetErrorString(e));
    return AAE_OK;
}

}  // namespace aae_bwd

extern "C" {

size_t aae_upconv_backward_workspace_bytes(const aae_upconv_backward_desc* d, int with_g_in) {
    aae_bwd::StagePlan p;
    if (!d || aae_bwd::plan_stage(d, with_g_in != 0, p, "aae_upconv_backward_workspace_bytes")) return 0;
    return p.total;
}

int aae_upconv_backward(const aae_upconv_backward_desc* d, const float* a_in, const float* a_out, const float* g_out, const float* w_hwio, float* dw, float* db,
                        float* g_in, void* workspace, size_t ws_bytes, void* stream) {
    aae_bwd::t_labels.clear();
    return aae_bwd::upconv_backward_impl(d, a_in, a_out, g_out, w_hwio, dw, db, g_in, workspace, ws_bytes, (hipStream_t)stream, "up", "aae_upconv_backward");
}

size_t aae_dense_backward_workspace_bytes(const aae_dense_backward_desc* d, int with_dz) {
    aae_bwd::DensePlan p;
    if (!d || aae_bwd::plan_dense(d, with_dz != 0, p, "aae_dense_backward_workspace_bytes")) return 0;
    return p.total;
}

int aae_dense_backward(const aae_dense_backward_desc* d, const float* z, const float* a_out, const float* g_out, const float* w, float* dw, float* db, float* dz,
                       void* workspace, size_t ws_bytes, void* stream) {
    aae_bwd::t_labels.clear();
    return aae_bwd::dense_backward_impl(d, z, a_out, g_out, w, dw, db, dz, workspace, ws_bytes, (hipStream_t)stream, "aae_dense_backward");
}

int aae_decoder_bwd_label_count(void) { return (int)aae_bwd::t_labels.size(); }

const char* aae_decoder_bwd_label(int i) {
    if (i < 0 || i >= (int)aae_bwd::t_labels.size()) return "";
    return aae_bwd::t_labels[i].c_str();
}

}  // extern "C"

#ifndef AAE_DECODER_BWD_STAGES_ONLY        // (the emulator's driver has no aae_decoder handle to walk: it builds the stage calls alone)
namespace aae_bwd {

struct ChainPlan {
    int L = 0;                                          // stages after the dense layer
    aae_dense_backward_desc dense;
    std::vector<aae_upconv_backward_desc> stages;
    std::vector<size_t> act_off, act_count;             // the forward workspace: [0] dense output, [i] output of hidden stage i
    size_t g_bytes = 0, scratch = 0, total = 0;
};

static int plan_chain(const aae_decoder* dec, int B, bool with_dz, ChainPlan& c, const char* who) {
    aae_decoder_desc d;
    if (!dec || aae_decoder_get_desc(dec, &d) != AAE_OK) return bfail(AAE_ERR_INVALID, "%s: null decoder", who);
    if (B < 1) return bfail(AAE_ERR_INVALID, "%s: batch %d < 1", who, B);
    if (d.batch_norm)
        return bfail(AAE_ERR_UNSUPPORTED, "%s: batch_norm: the backward pass needs the training-mode batch statistics, which are not built", who);
    c.L = d.num_layers;
    std::vector<int> dh(c.L), dw(c.L);
    for (int i = 0; i < c.L; ++i) {
        long long prod = 1;
        for (int j = i; j < c.L; ++j) prod *= d.strides[j];
        dh[i] = (int)(d.out_h / prod);
        dw[i] = (int)(d.out_w / prod);
    }
    c.dense.B = B; c.dense.J = d.latent_size; c.dense.U = dh[0] * dw[0] * d.num_filters[0];
    DensePlan dp;
    if (int rc = plan_dense(&c.dense, with_dz, dp, who)) return rc;
    c.scratch = dp.total;
    int H = dh[0], W = dw[0], C = d.num_filters[0];
    for (int i = 1; i <= c.L; ++i) {
        const bool last = i == c.L;
        aae_upconv_backward_desc s;
        s.B = B; s.H = H; s.W = W; s.Cin = C; s.UH = last ? d.out_h : dh[i]; s.UW = last ? d.out_w : dw[i]; s.Cout = last ? d.out_c : d.num_filters[i];
        s.KS = d.kernel_size; s.act = last ? BWD_ACT_SIGMOID : BWD_ACT_RELU;
        StagePlan sp;
        if (int rc = plan_stage(&s, true, sp, who)) return rc;
        if (sp.total > c.scratch) c.scratch = sp.total;
        c.stages.push_back(s);
        H = s.UH; W = s.UW; C = s.Cout;
    }
    c.act_off.resize(c.L); c.act_count.resize(c.L);
    for (int i = 0; i < c.L; ++i) {
        if (aae_decoder_activation_info(dec, B, i, &c.act_off[i], &c.act_count[i]) != AAE_OK) return AAE_ERR_INVALID;
        if (c.act_count[i] * sizeof(float) > c.g_bytes) c.g_bytes = c.act_count[i] * sizeof(float);
    }
    c.g_bytes = ws_align(c.g_bytes);
    c.total = 2 * c.g_bytes + c.scratch;
    return AAE_OK;
}

static int decoder_backward_impl(const aae_decoder* dec, int B, const float* z, const float* x, const float* dx, const void* forward_workspace, const float* const* weights,
                                 float* const* grads, float* dz, void* workspace, size_t ws_bytes, hipStream_t stream) {
    const char* who = "aae_decoder_backward";
    if (!dec || !z || !x || !dx || !forward_workspace || !weights || !grads || !workspace)
        return bfail(AAE_ERR_INVALID, "%s: null argument (only dz may be null)", who);
    ChainPlan c;
    if (int rc = plan_chain(dec, B, dz != nullptr, c, who)) return rc;
    for (int i = 0; i < 2 * (c.L + 1); ++i)
        if (!weights[i] || !grads[i]) return bfail(AAE_ERR_INVALID, "%s: weights[%d] or grads[%d] is null", who, i, i);
    if (ws_bytes < c.total || ((uintptr_t)workspace & (BWD_WS_ALIGN - 1)))
        return bfail(AAE_ERR_WORKSPACE, "%s: workspace %p of %zu bytes; %zu bytes, %zu-byte aligned, are needed", who, workspace, ws_bytes, c.total, BWD_WS_ALIGN);
    unsigned char* base = static_cast<unsigned char*>(workspace);
    float* gbuf[2] = {reinterpret_cast<float*>(base), reinterpret_cast<float*>(base + c.g_bytes)};
    void* scratch = base + 2 * c.g_bytes;
    const unsigned char* fwd = static_cast<const unsigned char*>(forward_workspace);
    auto act = [&](int i) { return reinterpret_cast<const float*>(fwd + c.act_off[i]); };
    const float* g = dx;
    for (int i = c.L; i >= 1; --i) {                    // stage i reads activation i - 1 and wrote activation i (the last one: x)
        char name[16];
        snprintf(name, sizeof(name), "up%d", i);
        float* g_in = gbuf[i & 1];
        if (int rc = upconv_backward_impl(&c.stages[i - 1], act(i - 1), i == c.L ? x : act(i), g, weights[2 * i], grads[2 * i], grads[2 * i + 1], g_in, scratch, c.scratch,
                                          stream, name, who))
            return rc;
        g = g_in;
    }
    return dense_backward_impl(&c.dense, z, act(0), g, weights[0], grads[0], grads[1], dz, scratch, c.scratch, stream, who);
}

}  // namespace aae_bwd

extern "C" {

size_t aae_decoder_backward_workspace_bytes(const aae_decoder* dec, int B) {
    aae_bwd::ChainPlan c;
    if (aae_bwd::plan_chain(dec, B, true, c, "aae_decoder_backward_workspace_bytes")) return 0;
    return c.total;
}

int aae_decoder_backward(const aae_decoder* dec, int B, const float* z, const float* x, const float* dx, const void* forward_workspace, const float* const* weights,
                         float* const* grads, float* dz, void* workspace, size_t ws_bytes, void* stream) {
    aae_bwd::t_labels.clear();
    return aae_bwd::decoder_backward_impl(dec, B, z, x, dx, forward_workspace, weights, grads, dz, workspace, ws_bytes, (hipStream_t)stream);
}

int aae_decoder_backward_timed(const aae_decoder* dec, int B, const float* z, const float* x, const float* dx, const void* forward_workspace, const float* const* weights,
                               float* const* grads, float* dz, void* workspace, size_t ws_bytes, void* stream, float* kernel_ms, int max_kernels, int* n_kernels) {
    using namespace aae_bwd;
    if (!kernel_ms || !n_kernels) return bfail(AAE_ERR_INVALID, "aae_decoder_backward_timed: null output");
    t_labels.clear();
    std::vector<hipEvent_t> ev;
    hipEvent_t first;
    if (hipEventCreate(&first) != hipSuccess) return bfail(AAE_ERR_RUNTIME, "aae_decoder_backward_timed: hipEventCreate failed");
    (void)hipEventRecord(first, (hipStream_t)stream);
    ev.push_back(first);
    t_events = &ev;
    int rc = decoder_backward_impl(dec, B, z, x, dx, forward_workspace, weights, grads, dz, workspace, ws_bytes, (hipStream_t)stream);
    t_events = nullptr;
    if (rc == AAE_OK && hipEventSynchronize(ev.back()) != hipSuccess) rc = bfail(AAE_ERR_RUNTIME, "aae_decoder_backward_timed: hipEventSynchronize failed");
    if (rc == AAE_OK) {
        const int n = (int)ev.size() - 1;
        for (int i = 0; i < n && i < max_kernels; ++i) {
            float ms = 0.f;
            (void)hipEventElapsedTime(&ms, ev[i], ev[i + 1]);
            kernel_ms[i] = ms;
        }
        *n_kernels = n;
    }
    for (hipEvent_t e : ev) (void)hipEventDestroy(e);
    return rc;
}

}  // extern "C"
#endif  // AAE_DECODER_BWD_STAGES_ONLY
