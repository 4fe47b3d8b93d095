// Host side of the encoder's backward pass (kernels/encoder_bwd_f32.h): the argument checks, the launch plan of a layer (tile widths,
// K splits, workspace layout), the launches behind aae_conv_backward / aae_linear_backward / aae_encoder_backward (include/aae_hip.h)
// and the labels of what ran.  The chain's refusals ask the handle as it is WHEN BACKWARD IS CALLED (aae_encoder_split_precision_for_batch,
// aae_encoder_activation_info): an option changed between the forward and the backward changes the answer, so the caller sets options
// before the forward; any AAE_ERR_UNSUPPORTED of aae_encoder_activation_info is reported as compact_workspace, its only cause today.
// Part of aae_encoder_bwd.hip; the CPU emulator's driver (tests/emu/encoder_bwd_emu.cpp) includes it too.
#pragma once

#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>

#include <string>
#include <vector>

#include "../../include/aae_hip.h"
#include "kernels/encoder_bwd_f32.h"

namespace aae_host {
void set_last_error(const char* msg);          // aae_host_types.h: the thread's aae_last_error() text lives in aae_hip.hip
}

namespace aae_ebwd {

constexpr size_t EBWD_WS_ALIGN = 256;
constexpr int EBWD_TARGET_BLOCKS = 512;        // a weight-gradient / g_a grid below this splits K (two blocks per CU)
constexpr int EBWD_MAX_SPLITS = 256;              // (one block per CU for the single-tile weight gradient of the first layer)
constexpr long long EBWD_MAX_ELEMS = 0x7FFFFFFFll;     // the kernels index pixels and small tensors with int
constexpr int EBWD_MAX_KS = 7, EBWD_MAX_STRIDE = 2;
constexpr int EBWD_MAX_CHUNKS = aae_bwd::BWD_MAX_CHUNKS;

static thread_local std::vector<std::string> t_labels;            // what the last call of this thread launched
static thread_local std::vector<hipEvent_t>* t_events = nullptr;  // aae_encoder_backward_timed: an event after every launch

static int efail(int code, const char* fmt, ...) {
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

static inline size_t ws_align(size_t bytes) { return (bytes + EBWD_WS_ALIGN - 1) / EBWD_WS_ALIGN * EBWD_WS_ALIGN; }
static inline int ceil_div_i(long long a, long long b) { return (int)((a + b - 1) / b); }
static inline int tile_nt(int n) { return n <= 32 ? 1 : (n <= 64 ? 2 : 4); }
static inline bool misaligned(const void* p) { return ((uintptr_t)p & 15) != 0; }
static inline unsigned grid_for(long long total) {
    long long b = (total + BWD_BLOCK - 1) / BWD_BLOCK;
    return (unsigned)(b > 4096 ? 4096 : (b < 1 ? 1 : b));
}

// K splits of a grid of `tiles` blocks over `slabs` slabs: enough blocks to fill the chip, no empty split (section 4j's rule)
static void choose_splits(int tiles, int slabs, int* splits, int* per) {
    int s = ceil_div_i(EBWD_TARGET_BLOCKS, tiles);
    if (s > EBWD_MAX_SPLITS) s = EBWD_MAX_SPLITS;
    if (s > slabs) s = slabs;
    if (s < 1) s = 1;
    *per = ceil_div_i(slabs, s);
    *splits = ceil_div_i(slabs, *per);
}

// the chunk plan of delta_bias_kernel / column_partial_kernel (section 4j's rule)
struct ColumnSumPlan {
    int cw = 4, chunks = 1, rows_per_chunk = 1;
};

static ColumnSumPlan plan_column_sums(long long rows, int C) {
    ColumnSumPlan p;
    while (p.cw < 64 && p.cw < C) p.cw *= 2;
    const int lanes = BWD_BLOCK / p.cw;
    long long chunks = (rows + 8ll * lanes - 1) / (8ll * lanes);
    if (chunks > EBWD_MAX_CHUNKS) chunks = EBWD_MAX_CHUNKS;
    if (chunks < 1) chunks = 1;
    p.rows_per_chunk = (int)((rows + chunks - 1) / chunks);
    p.chunks = (int)((rows + p.rows_per_chunk - 1) / p.rows_per_chunk);
    return p;
}

struct ConvPlan {
    ConvGeom g;
    long long out_elems = 0;        // B * Ho * Wo * Cout
    ColumnSumPlan sums;
    // weight gradient
    int M = 0, K = 0, w_nt = 1, w_row_tiles = 0, w_col_tiles = 0, w_splits = 1, w_slabs_per_split = 1;
    bool avec = false;
    // data gradient
    int P = 1, C4 = 0, d_nt = 1, d_row_tiles = 0, d_col_tiles = 0;
    // workspace
    size_t off_delta = 0, off_sums = 0, off_partial = 0, total = 0;
};

static int plan_conv(const aae_conv_backward_desc* d, ConvPlan& p, const char* who) {
    if (d->B < 1 || d->H < 1 || d->W < 1 || d->Cin < 1 || d->Cout < 1 || d->KS < 1 || d->S < 1)
        return efail(AAE_ERR_INVALID, "%s: non-positive shape (B %d, %dx%dx%d -> %d channels, KS %d, stride %d)", who, d->B, d->H, d->W, d->Cin, d->Cout, d->KS, d->S);
    if (d->x_dtype != AAE_DTYPE_U8 && d->x_dtype != AAE_DTYPE_F32)
        return efail(AAE_ERR_INVALID, "%s: x_dtype %d is neither uint8 (0) nor float32 (1)", who, d->x_dtype);
    if (d->S > EBWD_MAX_STRIDE)
        return efail(AAE_ERR_UNSUPPORTED, "%s: stride %d: the backward pass is built for strides 1 and 2", who, d->S);
    if (d->KS > EBWD_MAX_KS)
        return efail(AAE_ERR_UNSUPPORTED, "%s: kernel size %d: the backward pass is built for KS 1 ... %d", who, d->KS, EBWD_MAX_KS);
    if (d->Cin >= (1 << 20))
        return efail(AAE_ERR_UNSUPPORTED, "%s: %d input channels: the weight gradient's row code holds a channel below 2^20", who, d->Cin);
    const long long in_elems = (long long)d->B * d->H * d->W * d->Cin;
    const long long w_elems = (long long)d->KS * d->KS * d->Cin * d->Cout;
    const int Ho = (d->H + d->S - 1) / d->S, Wo = (d->W + d->S - 1) / d->S;
    const long long out_elems = (long long)d->B * Ho * Wo * d->Cout;
    if (in_elems > EBWD_MAX_ELEMS || out_elems > EBWD_MAX_ELEMS || w_elems > EBWD_MAX_ELEMS)
        return efail(AAE_ERR_UNSUPPORTED, "%s: a tensor of this layer has 2^31 elements or more (input %lld, output %lld, weights %lld); use a smaller batch", who, in_elems, out_elems, w_elems);
    p.g = make_geom(d->B, d->H, d->W, d->Cin, d->Cout, d->KS, d->S);
    p.out_elems = out_elems;
    p.K = d->B * Ho * Wo;
    p.sums = plan_column_sums(p.K, d->Cout);
    p.M = d->KS * d->KS * d->Cin;
    p.avec = (d->Cin & 3) == 0 && d->x_dtype == AAE_DTYPE_F32;
    p.w_nt = tile_nt(d->Cout);
    p.w_row_tiles = ceil_div_i(p.M, BWD_BM);
    p.w_col_tiles = ceil_div_i(d->Cout, 32 * p.w_nt);
    choose_splits(p.w_row_tiles * p.w_col_tiles, ceil_div_i(p.K, BWD_BK), &p.w_splits, &p.w_slabs_per_split);
    if ((long long)p.w_splits * w_elems > EBWD_MAX_ELEMS)
        return efail(AAE_ERR_UNSUPPORTED, "%s: the weight gradient's K-split partials have 2^31 elements or more (weights %lld)", who, w_elems);
    p.P = d->S * d->S;
    p.C4 = (d->Cout + 3) / 4;
    p.d_nt = tile_nt(d->Cin);
    p.d_row_tiles = ceil_div_i((long long)d->B * parity_extent(d->H, 0, d->S) * parity_extent(d->W, 0, d->S), BWD_BM);      // parity 0 is the largest class
    p.d_col_tiles = ceil_div_i(d->Cin, 32 * p.d_nt);
    size_t off = 0;
    p.off_delta = off; off += ws_align((size_t)out_elems * sizeof(float));
    p.off_sums = off; off += ws_align((size_t)p.sums.chunks * d->Cout * sizeof(float));
    p.off_partial = off; if (p.w_splits > 1) off += ws_align((size_t)p.w_splits * w_elems * sizeof(float));
    p.total = off;
    return AAE_OK;
}

template <int NT>
static void launch_wgrad_nt(const ConvWgradArgs& a, bool avec, unsigned grid, hipStream_t stream) {
    if (avec) AAE_LAUNCH((conv_wgrad_kernel<NT, true>), dim3(grid), dim3(BWD_BLOCK), 0, stream, a);
    else AAE_LAUNCH((conv_wgrad_kernel<NT, false>), dim3(grid), dim3(BWD_BLOCK), 0, stream, a);
}
template <int NT>
static void launch_dgrad_nt(const ConvDgradArgs& a, unsigned grid, hipStream_t stream) { AAE_LAUNCH((conv_dgrad_kernel<NT>), dim3(grid), dim3(BWD_BLOCK), 0, stream, a); }
template <int NT>
static void launch_dz_nt(const aae_bwd::DenseDzArgs& a, unsigned grid, hipStream_t stream) { AAE_LAUNCH((aae_bwd::dense_dz_kernel<NT>), dim3(grid), dim3(BWD_BLOCK), 0, stream, a); }

static int conv_backward_impl(const aae_conv_backward_desc* d, const void* a_in, const float* a_out, const float* g_out, const float* w, float* dw, float* db, float* g_in,
                              void* workspace, size_t ws_bytes, hipStream_t stream, const char* name, const char* who) {
    if (!d || !a_in || !a_out || !g_out || !w || !dw || !db || !workspace)
        return efail(AAE_ERR_INVALID, "%s: null argument (desc, a_in, a_out, g_out, w, dw, db and workspace are required)", who);
    ConvPlan p;
    if (int rc = plan_conv(d, p, who)) return rc;
    if (misaligned(a_in) || misaligned(a_out) || misaligned(g_out) || misaligned(w) || misaligned(dw) || misaligned(db) || misaligned(g_in))
        return efail(AAE_ERR_INVALID, "%s: every tensor must be 16-byte aligned", who);
    if (ws_bytes < p.total || ((uintptr_t)workspace & (EBWD_WS_ALIGN - 1)))
        return efail(AAE_ERR_WORKSPACE, "%s: workspace %p of %zu bytes; %zu bytes, %zu-byte aligned, are needed", who, workspace, ws_bytes, p.total, EBWD_WS_ALIGN);
    unsigned char* base = static_cast<unsigned char*>(workspace);
    float* delta = reinterpret_cast<float*>(base + p.off_delta);
    float* sums = reinterpret_cast<float*>(base + p.off_sums);
    float* partial = p.w_splits > 1 ? reinterpret_cast<float*>(base + p.off_partial) : dw;
    const ConvGeom& g = p.g;

    aae_bwd::DeltaBiasArgs ba;
    ba.g_out = g_out; ba.a_out = a_out; ba.delta = delta; ba.partial = sums; ba.rows = p.K; ba.C = d->Cout; ba.act = aae_bwd::BWD_ACT_RELU; ba.cw = p.sums.cw;
    ba.rows_per_chunk = p.sums.rows_per_chunk;
    AAE_LAUNCH(aae_bwd::delta_bias_kernel, dim3((unsigned)ceil_div_i(d->Cout, p.sums.cw), (unsigned)p.sums.chunks), dim3(BWD_BLOCK), 0, stream, ba);
    launched(stream, "%s:delta_bias rows=%d C=%d chunks=%d", name, p.K, d->Cout, p.sums.chunks);
    AAE_LAUNCH(aae_bwd::column_sum_finish_kernel, dim3((unsigned)ceil_div_i(d->Cout, BWD_BLOCK)), dim3(BWD_BLOCK), 0, stream, (const float*)sums, p.sums.chunks, d->Cout, db);
    launched(stream, "%s:column_sum_finish C=%d", name, d->Cout);

    ConvWgradArgs wa;
    wa.a_in = a_in; wa.delta = delta; wa.partial = partial; wa.g = g; wa.M = p.M; wa.K = p.K; wa.row_tiles = p.w_row_tiles; wa.col_tiles = p.w_col_tiles;
    wa.splits = p.w_splits; wa.slabs_per_split = p.w_slabs_per_split; wa.in_u8 = d->x_dtype == AAE_DTYPE_U8;
    const unsigned wgrid = (unsigned)(p.w_splits * p.w_row_tiles * p.w_col_tiles);
    if (p.w_nt == 1) launch_wgrad_nt<1>(wa, p.avec, wgrid, stream);
    else if (p.w_nt == 2) launch_wgrad_nt<2>(wa, p.avec, wgrid, stream);
    else launch_wgrad_nt<4>(wa, p.avec, wgrid, stream);
    launched(stream, "%s:wgrad_mfma_f32 M=%d N=%d K=%d tiles=%dx%d nt=%d load=%s splits=%d", name, p.M, d->Cout, p.K, p.w_row_tiles, p.w_col_tiles, p.w_nt,
             p.avec ? "x4" : (wa.in_u8 ? "u8" : "x1"), p.w_splits);
    if (p.w_splits > 1) {
        AAE_LAUNCH(aae_bwd::splitk_sum_kernel, dim3(grid_for((long long)p.M * d->Cout)), dim3(BWD_BLOCK), 0, stream, (const float*)partial, p.w_splits, p.M * d->Cout, dw);
        launched(stream, "%s:wgrad_reduce splits=%d", name, p.w_splits);
    }
    if (g_in) {
        ConvDgradArgs da;
        da.delta = delta; da.w = w; da.g_in = g_in; da.g = g; da.C4 = p.C4; da.row_tiles = p.d_row_tiles; da.col_tiles = p.d_col_tiles;
        const unsigned dgrid = (unsigned)(p.P * p.d_row_tiles * p.d_col_tiles);
        if (p.d_nt == 1) launch_dgrad_nt<1>(da, dgrid, stream);
        else if (p.d_nt == 2) launch_dgrad_nt<2>(da, dgrid, stream);
        else launch_dgrad_nt<4>(da, dgrid, stream);
        launched(stream, "%s:dgrad_parity_mfma_f32 parities=%d M=%d N=%d K=%d tiles=%dx%d nt=%d splits=1", name, p.P, d->B * d->H * d->W, d->Cin, d->KS * d->KS * 4 * p.C4,
                 p.d_row_tiles, p.d_col_tiles, p.d_nt);
    }
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return efail(AAE_ERR_RUNTIME, "%s: launch failed: %s", who, hipGetErrorString(e));
    return AAE_OK;
}

// ---- the linear dense layer z = flat(a) w + b: a [B,J], w [J,U], dz [B,U] ---------------------------------------------------------------
struct LinearPlan {
    ColumnSumPlan sums;
    int nt = 1, row_tiles = 0, col_tiles = 0, splits = 1, slabs_per_split = 1;
    size_t off_sums = 0, off_partial = 0, total = 0;
};

static int plan_linear(const aae_dense_backward_desc* d, bool with_g_a, LinearPlan& p, const char* who) {
    if (d->B < 1 || d->J < 1 || d->U < 1) return efail(AAE_ERR_INVALID, "%s: B = %d, J = %d, U = %d", who, d->B, d->J, d->U);
    if ((long long)d->B * d->U > EBWD_MAX_ELEMS || (long long)d->J * d->U > EBWD_MAX_ELEMS || (long long)d->B * d->J > EBWD_MAX_ELEMS)
        return efail(AAE_ERR_UNSUPPORTED, "%s: a tensor of this layer has 2^31 elements or more (B %d, J %d, U %d)", who, d->B, d->J, d->U);
    p.sums = plan_column_sums(d->B, d->U);
    p.nt = tile_nt(d->J);
    p.row_tiles = ceil_div_i(d->B, BWD_BM);
    p.col_tiles = ceil_div_i(d->J, 32 * p.nt);
    choose_splits(p.row_tiles * p.col_tiles, ceil_div_i(d->U, BWD_BK), &p.splits, &p.slabs_per_split);
    if ((long long)p.splits * d->B * d->J > EBWD_MAX_ELEMS)
        return efail(AAE_ERR_UNSUPPORTED, "%s: the K-split partials of dL/da have 2^31 elements or more (B %d, J %d)", who, d->B, d->J);
    size_t off = 0;
    p.off_sums = off; off += ws_align((size_t)p.sums.chunks * d->U * sizeof(float));
    p.off_partial = off; if (with_g_a && p.splits > 1) off += ws_align((size_t)p.splits * d->B * d->J * sizeof(float));
    p.total = off;
    return AAE_OK;
}

static int linear_backward_impl(const aae_dense_backward_desc* d, const float* a, const float* dz, const float* w, float* dw, float* db, float* g_a, void* workspace,
                                size_t ws_bytes, hipStream_t stream, const char* who) {
    if (!d || !a || !dz || !w || !dw || !db || !workspace) return efail(AAE_ERR_INVALID, "%s: null argument (desc, a, dz, w, dw, db and workspace are required)", who);
    LinearPlan p;
    if (int rc = plan_linear(d, g_a != nullptr, p, who)) return rc;
    if (misaligned(a) || misaligned(dz) || misaligned(w) || misaligned(dw) || misaligned(db) || misaligned(g_a))
        return efail(AAE_ERR_INVALID, "%s: every tensor must be 16-byte aligned", who);
    if (ws_bytes < p.total || ((uintptr_t)workspace & (EBWD_WS_ALIGN - 1)))
        return efail(AAE_ERR_WORKSPACE, "%s: workspace %p of %zu bytes; %zu bytes, %zu-byte aligned, are needed", who, workspace, ws_bytes, p.total, EBWD_WS_ALIGN);
    unsigned char* base = static_cast<unsigned char*>(workspace);
    float* sums = reinterpret_cast<float*>(base + p.off_sums);
    float* partial = p.splits > 1 ? reinterpret_cast<float*>(base + p.off_partial) : g_a;
    AAE_LAUNCH(column_partial_kernel, dim3((unsigned)ceil_div_i(d->U, p.sums.cw), (unsigned)p.sums.chunks), dim3(BWD_BLOCK), 0, stream, dz, sums, d->B, d->U, p.sums.cw,
               p.sums.rows_per_chunk);
    launched(stream, "dense:column_partial rows=%d C=%d chunks=%d", d->B, d->U, p.sums.chunks);
    AAE_LAUNCH(aae_bwd::column_sum_finish_kernel, dim3((unsigned)ceil_div_i(d->U, BWD_BLOCK)), dim3(BWD_BLOCK), 0, stream, (const float*)sums, p.sums.chunks, d->U, db);
    launched(stream, "dense:column_sum_finish C=%d", d->U);
    AAE_LAUNCH(aae_bwd::dense_dw_kernel, dim3(grid_for((long long)d->J * d->U)), dim3(BWD_BLOCK), 0, stream, a, dz, dw, d->B, d->J, d->U);
    launched(stream, "dense:dw_plain M=%d N=%d K=%d", d->J, d->U, d->B);
    if (g_a) {
        aae_bwd::DenseDzArgs da;
        da.delta = dz; da.w = w; da.partial = partial; da.B = d->B; da.J = d->J; da.U = d->U; da.row_tiles = p.row_tiles; da.col_tiles = p.col_tiles; da.splits = p.splits;
        da.slabs_per_split = p.slabs_per_split;
        const unsigned grid = (unsigned)(p.splits * p.row_tiles * p.col_tiles);
        if (p.nt == 1) launch_dz_nt<1>(da, grid, stream);
        else if (p.nt == 2) launch_dz_nt<2>(da, grid, stream);
        else launch_dz_nt<4>(da, grid, stream);
        launched(stream, "dense:ga_mfma_f32 M=%d N=%d K=%d tiles=%dx%d nt=%d splits=%d", d->B, d->J, d->U, p.row_tiles, p.col_tiles, p.nt, p.splits);
        if (p.splits > 1) {
            AAE_LAUNCH(aae_bwd::splitk_sum_kernel, dim3(grid_for((long long)d->B * d->J)), dim3(BWD_BLOCK), 0, stream, (const float*)partial, p.splits, d->B * d->J, g_a);
            launched(stream, "dense:ga_reduce splits=%d", p.splits);
        }
    }
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return efail(AAE_ERR_RUNTIME, "%s: launch failed: %s", who, hipGetErrorString(e));
    return AAE_OK;
}

}  // namespace aae_ebwd

extern "C" {

size_t aae_conv_backward_workspace_bytes(const aae_conv_backward_desc* d) {
    aae_ebwd::ConvPlan p;
    if (!d || aae_ebwd::plan_conv(d, p, "aae_conv_backward_workspace_bytes")) return 0;
    return p.total;
}

int aae_conv_backward(const aae_conv_backward_desc* d, const void* a_in, const float* a_out, const float* g_out, const float* w_hwio, float* dw, float* db, float* g_in,
                      void* workspace, size_t ws_bytes, void* stream) {
    aae_ebwd::t_labels.clear();
    return aae_ebwd::conv_backward_impl(d, a_in, a_out, g_out, w_hwio, dw, db, g_in, workspace, ws_bytes, (hipStream_t)stream, "conv", "aae_conv_backward");
}

size_t aae_linear_backward_workspace_bytes(const aae_dense_backward_desc* d, int with_g_a) {
    aae_ebwd::LinearPlan p;
    if (!d || aae_ebwd::plan_linear(d, with_g_a != 0, p, "aae_linear_backward_workspace_bytes")) return 0;
    return p.total;
}

int aae_linear_backward(const aae_dense_backward_desc* d, const float* a, const float* dz, const float* w, float* dw, float* db, float* g_a, void* workspace, size_t ws_bytes,
                        void* stream) {
    aae_ebwd::t_labels.clear();
    return aae_ebwd::linear_backward_impl(d, a, dz, w, dw, db, g_a, workspace, ws_bytes, (hipStream_t)stream, "aae_linear_backward");
}

int aae_encoder_bwd_label_count(void) { return (int)aae_ebwd::t_labels.size(); }

const char* aae_encoder_bwd_label(int i) {
    if (i < 0 || i >= (int)aae_ebwd::t_labels.size()) return "";
    return aae_ebwd::t_labels[i].c_str();
}

}  // extern "C"

#ifndef AAE_ENCODER_BWD_LAYERS_ONLY        // (the emulator's driver has no aae_encoder handle to walk: it builds the layer calls alone)
namespace aae_ebwd {

struct ChainPlan {
    int L = 0;                                          // conv layers
    std::vector<aae_conv_backward_desc> layers;
    aae_dense_backward_desc dense;
    std::vector<size_t> act_off, act_count;             // the forward workspace: output of conv layer i
    size_t g_bytes = 0, scratch = 0, total = 0;
};

static int plan_chain(const aae_encoder* enc, int B, int x_dtype, ChainPlan& c, const char* who) {
    aae_encoder_desc d;
    if (!enc || aae_encoder_get_desc(enc, &d) != AAE_OK) return efail(AAE_ERR_INVALID, "%s: null encoder", who);
    if (B < 1) return efail(AAE_ERR_INVALID, "%s: batch %d < 1", who, B);
    if (x_dtype != AAE_DTYPE_U8 && x_dtype != AAE_DTYPE_F32) return efail(AAE_ERR_INVALID, "%s: x_dtype %d is neither uint8 (0) nor float32 (1)", who, x_dtype);
    if (d.batch_norm)
        return efail(AAE_ERR_UNSUPPORTED, "%s: batch_norm: the backward pass needs the training-mode batch statistics, which are not built", who);
    if (aae_encoder_split_precision_for_batch(enc, B))
        return efail(AAE_ERR_UNSUPPORTED, "%s: split precision: the forward of a batch of %d leaves fp16 (hi, lo) activations; the backward pass reads fp32 ones (set \"precision\" to 0)", who, B);
    c.L = d.num_layers;
    c.act_off.resize(c.L); c.act_count.resize(c.L);
    for (int i = 0; i < c.L; ++i) {
        const int rc = aae_encoder_activation_info(enc, B, i, &c.act_off[i], &c.act_count[i]);
        if (rc == AAE_ERR_UNSUPPORTED)
            return efail(AAE_ERR_UNSUPPORTED, "%s: compact_workspace: the forward has overwritten the output of layer %d, which the backward pass reads (set \"compact_workspace\" to 0)", who, i);
        if (rc != AAE_OK) return rc;
        if (c.act_count[i] * sizeof(float) > c.g_bytes) c.g_bytes = c.act_count[i] * sizeof(float);
    }
    int H = d.in_h, W = d.in_w, C = d.in_c;
    for (int i = 0; i < c.L; ++i) {
        aae_conv_backward_desc s;
        s.B = B; s.H = H; s.W = W; s.Cin = C; s.Cout = d.num_filters[i]; s.KS = d.kernel_size; s.S = d.strides[i]; s.x_dtype = i == 0 ? x_dtype : AAE_DTYPE_F32;
        ConvPlan cp;
        if (int rc = plan_conv(&s, cp, who)) return rc;
        if (cp.total > c.scratch) c.scratch = cp.total;
        c.layers.push_back(s);
        H = cp.g.Ho; W = cp.g.Wo; C = s.Cout;
    }
    c.dense.B = B; c.dense.J = H * W * C; c.dense.U = d.latent_size;
    LinearPlan lp;
    if (int rc = plan_linear(&c.dense, true, lp, who)) return rc;
    if (lp.total > c.scratch) c.scratch = lp.total;
    c.g_bytes = ws_align(c.g_bytes);
    c.total = 2 * c.g_bytes + c.scratch;
    return AAE_OK;
}

static int encoder_backward_impl(const aae_encoder* enc, int B, const void* x, int x_dtype, const float* dz, const void* forward_workspace, const float* const* weights,
                                 float* const* grads, float* dx, void* workspace, size_t ws_bytes, hipStream_t stream) {
    const char* who = "aae_encoder_backward";
    if (!enc || !x || !dz || !forward_workspace || !weights || !grads || !workspace) return efail(AAE_ERR_INVALID, "%s: null argument (only dx may be null)", who);
    ChainPlan c;
    if (int rc = plan_chain(enc, B, x_dtype, c, who)) return rc;
    for (int i = 0; i < 2 * (c.L + 1); ++i)
        if (!weights[i] || !grads[i]) return efail(AAE_ERR_INVALID, "%s: weights[%d] or grads[%d] is null", who, i, i);
    if (ws_bytes < c.total || ((uintptr_t)workspace & (EBWD_WS_ALIGN - 1)))
        return efail(AAE_ERR_WORKSPACE, "%s: workspace %p of %zu bytes; %zu bytes, %zu-byte aligned, are needed", who, workspace, ws_bytes, c.total, EBWD_WS_ALIGN);
    unsigned char* base = static_cast<unsigned char*>(workspace);
    float* gbuf[2] = {reinterpret_cast<float*>(base), reinterpret_cast<float*>(base + c.g_bytes)};
    void* scratch = base + 2 * c.g_bytes;
    const unsigned char* fwd = static_cast<const unsigned char*>(forward_workspace);
    auto act = [&](int i) { return reinterpret_cast<const float*>(fwd + c.act_off[i]); };
    float* g = gbuf[c.L & 1];
    if (int rc = linear_backward_impl(&c.dense, act(c.L - 1), dz, weights[2 * c.L], grads[2 * c.L], grads[2 * c.L + 1], g, scratch, c.scratch, stream, who)) return rc;
    for (int i = c.L - 1; i >= 0; --i) {                // layer i reads activation i - 1 (the first one: x) and wrote activation i
        char name[16];
        snprintf(name, sizeof(name), "conv%d", i + 1);
        float* g_in = i == 0 ? dx : gbuf[i & 1];
        if (int rc = conv_backward_impl(&c.layers[i], i == 0 ? x : (const void*)act(i - 1), act(i), g, weights[2 * i], grads[2 * i], grads[2 * i + 1], g_in, scratch, c.scratch,
                                        stream, name, who))
            return rc;
        g = g_in;
    }
    return AAE_OK;
}

}  // namespace aae_ebwd

extern "C" {

size_t aae_encoder_backward_workspace_bytes(const aae_encoder* enc, int B) {
    aae_ebwd::ChainPlan c;
    if (aae_ebwd::plan_chain(enc, B, AAE_DTYPE_F32, c, "aae_encoder_backward_workspace_bytes")) return 0;
    return c.total;
}

int aae_encoder_backward(const aae_encoder* enc, int B, const void* x, int x_dtype, const float* dz, const void* forward_workspace, const float* const* weights,
                         float* const* grads, float* dx, void* workspace, size_t ws_bytes, void* stream) {
    aae_ebwd::t_labels.clear();
    return aae_ebwd::encoder_backward_impl(enc, B, x, x_dtype, dz, forward_workspace, weights, grads, dx, workspace, ws_bytes, (hipStream_t)stream);
}

int aae_encoder_backward_timed(const aae_encoder* enc, int B, const void* x, int x_dtype, const float* dz, const void* forward_workspace, const float* const* weights,
                               float* const* grads, float* dx, void* workspace, size_t ws_bytes, void* stream, float* kernel_ms, int max_kernels, int* n_kernels) {
    using namespace aae_ebwd;
    if (!kernel_ms || !n_kernels) return efail(AAE_ERR_INVALID, "aae_encoder_backward_timed: null output");
    t_labels.clear();
    std::vector<hipEvent_t> ev;
    hipEvent_t first;
    if (hipEventCreate(&first) != hipSuccess) return efail(AAE_ERR_RUNTIME, "aae_encoder_backward_timed: hipEventCreate failed");
    (void)hipEventRecord(first, (hipStream_t)stream);
    ev.push_back(first);
    t_events = &ev;
    int rc = encoder_backward_impl(enc, B, x, x_dtype, dz, forward_workspace, weights, grads, dx, workspace, ws_bytes, (hipStream_t)stream);
    t_events = nullptr;
    if (rc == AAE_OK && hipEventSynchronize(ev.back()) != hipSuccess) rc = efail(AAE_ERR_RUNTIME, "aae_encoder_backward_timed: hipEventSynchronize failed");
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
#endif  // AAE_ENCODER_BWD_LAYERS_ONLY
