// Handles and shared host-side types of libaae_hip.so: error reporting, the Layer record of one convolution, the encoder and
// codebook handles (their launch-planning knobs and scan settings: aae_options.h).  Part of aae_hip_impl.h.
#pragma once

#include "aae_options.h"

namespace aae_host {

static thread_local std::string g_last_error;

static int fail(int code, const char* fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    g_last_error = buf;
    return code;
}

// for the library's other translation units (aae_render.hip): aae_last_error() reads the text of this one
void set_last_error(const char* msg) { g_last_error = msg; }

#define AAE_HIP_TRY(expr)                                                                      \
    do {                                                                                        \
        hipError_t e__ = (expr);                                                                \
        if (e__ != hipSuccess)                                                                  \
            return aae_host::fail(AAE_ERR_RUNTIME, "%s failed: %s (%s:%d)", #expr,              \
                                  hipGetErrorString(e__), __FILE__, __LINE__);                  \
    } while (0)

static inline size_t align_up(size_t v, size_t a) { return (v + a - 1) / a * a; }
static inline int ceil_div(int a, int b) { return (a + b - 1) / b; }

// [TF-semantics] 'SAME': out = ceil(in/s); total = max((out-1)*s + k - in, 0); before = total/2.
static inline void same_pad(int in, int k, int s, int* out, int* before) {
    const int o = ceil_div(in, s);
    int total = (o - 1) * s + k - in;
    if (total < 0) total = 0;
    *out = o;
    *before = total / 2;
}

enum LayerKind { KIND_FIRST_MFMA = 0, KIND_IGEMM = 1, KIND_GENERIC = 2 };

struct Layer {
    int H = 0, W = 0, Cin = 0, Ho = 0, Wo = 0, Cout = 0, CoutPad = 0;
    int KS = 0, S = 0, pt = 0, pl = 0;
    int relu = 1;
    int index = -1;             // position among the conv layers (0 = first); -1: the dense layer
    LayerKind kind = KIND_GENERIC;
    float* w_hwio = nullptr;    // device [KS*KS*Cin][Cout]
    float* wp = nullptr;        // device [K/4][CoutPad][4]      (igemm)
    unsigned* wp16 = nullptr;   // device [slabs][8][CoutPad][4 dwords]: (hi, lo) halves of w*2^w_shift (f32x3h)
    int w_shift = 0;
    float* wino[4] = {nullptr, nullptr, nullptr, nullptr};   // Winograd-domain weights of the four polyphase components (conv_winograd_f32.h), index 2 eh + ew;
    int wino_geom = -1;         // ... and the block geometry the layer runs with (-1: not eligible / not prepared)
    float* bias = nullptr;
    float* bn_scale = nullptr;  // folded inference BN: x*scale + shift
    float* bn_shift = nullptr;
    // first-layer staging geometry
    int rowlen = 0, first_smem = 0;       // conv1 (conv_first_f32.h): staged floats per input row, LDS bytes
    bool first_packable = true;
    int rowlen4 = 0, lead4 = 0;           // same for the dword-staged uint8 form (0 = not applicable)
    long long K() const { return (long long)KS * KS * Cin; }
};

struct KernelRecord {
    std::string label;
    double flops;
};

constexpr int kX3hRing = 256;          // range-flag slots of eager f32x3h forwards (reused round-robin)
constexpr int kX3hCaptured = 64;       // ... of forwards recorded into HIP graphs (one each, never reused)

}  // namespace aae_host

struct aae_encoder : aae_host::EncoderOptions {     // (every option: aae_options.h)
    aae_encoder_desc desc;
    std::vector<aae_host::Layer> layers;   // conv layers
    aae_host::Layer dense;                 // 1x1 "conv" over the flattened activation
    float* lut = nullptr;                  // device [256] float32(v/255.)
    // f32x3h range flags: "an activation left the range its fp16 (hi, lo) pair carries exactly".  One int per forward, taken
    // round-robin from a ring (eager forwards) or, for forwards recorded into a HIP graph, from a region that is never recycled
    // (a graph bakes the address).  Nobody has to wait for the stream after a forward: the flags of many forwards are polled
    // together when their results are consumed (aae_encoder_x3h_poll).
    int* x3h_sat = nullptr;                // device [kX3hRing + kX3hCaptured]
    std::atomic<unsigned long long> x3h_seq{0};
    int x3h_captured = 0;                  // slots of the captured region handed out so far (under x3h_mu) ...
    std::vector<int> x3h_free;             // ... and the ones given back (aae_encoder_x3h_release_slot)
    std::vector<hipEvent_t> x3h_release_ev; // per captured slot: recorded behind the flag clear of its release -- a slot is handed out again only once that clear has executed
    std::mutex x3h_mu;
    std::mutex wino_mu;                    // guards the one-time preparation of the Winograd-domain weights (ensure_winograd_weights)
    std::vector<void*> allocations;
    std::vector<aae_host::KernelRecord> records;   // of the most recent completed forward (swapped in under rec_mu)
    std::mutex rec_mu;
    long long* wavek_timeline = nullptr;   // device [3 layers][512 blocks][8] phase stamps when option wavek_timeline is on (profiling tools)
    int cu_count = 0;                      // compute units of the device the handle lives on
};

struct aae_codebook : aae_host::ScanSettings {     // (what the scan modes switch: aae_options.h)
    float* E = nullptr;    // device [N][J] (fp32 codebook), or the bf16 rows when dtype == AAE_DTYPE_BF16
    void* E_alloc = nullptr;   // the allocation E lies in (E is aligned up to kCodebookAlign inside it)
    int dtype = AAE_DTYPE_F32;
    int N = 0, J = 0;
    int cu_count = 256;    // compute units of the device the handle lives on: the query-resident scan puts one block on each
    // upright search (col_stride k > 1): a compacted copy of rows 0, k, 2k, ... prepared by
    // aae_codebook_prepare_upright; the scan then runs over N/k rows and the winning row id is scaled by k
    aae_codebook* upright = nullptr;   // the copy for the stride asked for last (one of upright_copies)
    int upright_stride = 0;
    // every compacted copy ever prepared, one per stride, kept until the handle is destroyed: a captured HIP graph may
    // hold the address of a copy made for another stride than the one in use now
    std::vector<std::pair<int, aae_codebook*>> upright_copies;
};
