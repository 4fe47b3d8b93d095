// Layer launches and the forward pass of the encoder (/root/reference/auto_pose/ae/encoder.py:37-68: conv -> ReLU -> [BN] per layer,
// flatten, dense): one function per kernel family that fills the kernel's argument record from a Layer and the plan, then
// forward_impl, which walks the layers.  Part of aae_hip_impl.h.
#pragma once

namespace aae_host {

// ------------------------------------------------------------ layer launches
struct Timer {
    bool on = false;
    hipStream_t stream = nullptr;
    std::vector<hipEvent_t> ev;
    int mark() {
        if (!on) return AAE_OK;
        hipEvent_t e;
        AAE_HIP_TRY(hipEventCreate(&e));
        ev.push_back(e);
        AAE_HIP_TRY(hipEventRecord(e, stream));
        return AAE_OK;
    }
};

// The end of every launch function: the kernel's record under its printf-style label, the launch's error, the timer's event.
__attribute__((format(printf, 3, 4))) static int launch_done(Timer& tm, double flops, const char* fmt, ...) {
    char label[128];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(label, sizeof(label), fmt, ap);
    va_end(ap);
    note_kernel({label, flops});
    AAE_HIP_TRY(hipGetLastError());
    return tm.mark();
}

// ------------------------------------------------------------ form lists
// Every instantiation of a kernel family is ONE row of the family's list, X(when, kernel, lds): `when` selects the row from the family's dispatch keys (a form has
// exactly the layer tags its rows name: a tag only makes the symbol unique per encoder layer -- separate rows in rocprofv3 --stats -- and a list never instantiates
// one the launch code does not ask for), `kernel` is the instantiation in parentheses, `lds` the most dynamic LDS it is launched with.  Two things are generated from
// a list, and from nothing else: the family's dispatch -- AAE_FORM_LAUNCH in a function whose parameters are the keys, false for "no such form in this build" -- and
// the family's line in set_launch_attributes, which raises the LDS ceiling of every row when a handle is created.  A new or retired form is one row.  The rows of
// the experiments build sit in the *_EXPERIMENTS part of their list.
#define AAE_FORM_LAUNCH(when, kernel, lds) if (when) { AAE_LAUNCH(kernel, grid, block, lds, stream, a); return true; }
// (a launch below the row's ceiling: `smem` of the enclosing function -- a size that depends on the layer or on the grid)
#define AAE_FORM_LAUNCH_SMEM(when, kernel, lds) if (when) { AAE_LAUNCH(kernel, grid, block, smem, stream, a); return true; }
#define AAE_FORM_CEILING(when, kernel, lds) (void)hipFuncSetAttribute((const void*)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, lds);

// conv_igemm_f32_kernel<SPLITK, DMA, SCATTER, TAG, BREG, NW>, encoder and decoder.  The register-staged operand path (!dma) and LDS-DMA without the weights in
// registers on a tagged layer are reachable in the experiments build only.
enum IgemmForm { IGEMM_PLAIN, IGEMM_BREG, IGEMM_BREG_N256, IGEMM_SPLITK, IGEMM_UPCONV_PHASES };
#ifdef AAE_EXPERIMENTS
#define AAE_IGEMM_FORMS_EXPERIMENTS(X) \
    X(form == IGEMM_PLAIN && dma && tag == 1, (aae::conv_igemm_f32_kernel<false, true, false, 1>), aae::kConvIgemmSmem) \
    X(form == IGEMM_PLAIN && dma && tag == 2, (aae::conv_igemm_f32_kernel<false, true, false, 2>), aae::kConvIgemmSmem) \
    X(form == IGEMM_PLAIN && dma && tag == 3, (aae::conv_igemm_f32_kernel<false, true, false, 3>), aae::kConvIgemmSmem)
#else
#define AAE_IGEMM_FORMS_EXPERIMENTS(X)
#endif
#define AAE_IGEMM_FORMS(X) \
    X(form == IGEMM_BREG_N256 && tag == 1, (aae::conv_igemm_f32_kernel<false, true, false, 1, true, 4>), 2 * aae::kSlabFloatsA * 4) \
    X(form == IGEMM_BREG_N256 && tag == 2, (aae::conv_igemm_f32_kernel<false, true, false, 2, true, 4>), 2 * aae::kSlabFloatsA * 4) \
    X(form == IGEMM_BREG && tag == 1, (aae::conv_igemm_f32_kernel<false, true, false, 1, true>), aae::kConvIgemmSmem) \
    X(form == IGEMM_BREG && tag == 2, (aae::conv_igemm_f32_kernel<false, true, false, 2, true>), aae::kConvIgemmSmem) \
    X(form == IGEMM_BREG && tag == 3, (aae::conv_igemm_f32_kernel<false, true, false, 3, true>), aae::kConvIgemmSmem) \
    AAE_IGEMM_FORMS_EXPERIMENTS(X) \
    X(form == IGEMM_PLAIN && dma, (aae::conv_igemm_f32_kernel<false, true>), aae::kConvIgemmSmem) \
    X(form == IGEMM_PLAIN && !dma, (aae::conv_igemm_f32_kernel<false>), aae::kConvIgemmSmem) \
    X(form == IGEMM_SPLITK && dma, (aae::conv_igemm_f32_kernel<true, true>), aae::kConvIgemmSmem) \
    X(form == IGEMM_SPLITK && !dma, (aae::conv_igemm_f32_kernel<true>), aae::kConvIgemmSmem) \
    X(form == IGEMM_UPCONV_PHASES, (aae::conv_igemm_f32_kernel<false, true, true>), aae::kConvIgemmSmem)

// conv_igemm_x3h_kernel<OUT> (register-staged), conv_igemm_x3h_dma_kernel<OUT, TAG, WM> and conv_igemm_x3h_wide_kernel<OUT, TAG>
enum X3hForm { X3H_PLANES, X3H_F32, X3H_PARTIAL, X3H_WIDE256, X3H_WIDE128 };
#ifdef AAE_EXPERIMENTS
#define AAE_X3H_FORMS_EXPERIMENTS(X) \
    X(form == X3H_WIDE128 && tag == 1, (aae::conv_igemm_x3h_dma_kernel<aae::X3H_OUT_PLANES, 1, 4>), (aae::x3h_dma_smem<4>())) \
    X(form == X3H_WIDE128 && tag == 2, (aae::conv_igemm_x3h_dma_kernel<aae::X3H_OUT_PLANES, 2, 4>), (aae::x3h_dma_smem<4>())) \
    X(form == X3H_WIDE128 && tag == 3, (aae::conv_igemm_x3h_dma_kernel<aae::X3H_OUT_PLANES, 3, 4>), (aae::x3h_dma_smem<4>())) \
    X(form == X3H_F32 && !dma, (aae::conv_igemm_x3h_kernel<aae::X3H_OUT_F32>), aae::kConvIgemmSmem) \
    X(form == X3H_PLANES && !dma, (aae::conv_igemm_x3h_kernel<aae::X3H_OUT_PLANES>), aae::kConvIgemmSmem) \
    X(form == X3H_PARTIAL && !dma, (aae::conv_igemm_x3h_kernel<aae::X3H_OUT_PARTIAL>), aae::kConvIgemmSmem)
#else
#define AAE_X3H_FORMS_EXPERIMENTS(X)
#endif
#define AAE_X3H_FORMS(X) \
    X(form == X3H_WIDE256 && tag == 1, (aae::conv_igemm_x3h_wide_kernel<aae::X3H_OUT_PLANES, 1>), aae::kX3hWideSmem) \
    X(form == X3H_WIDE256 && tag == 2, (aae::conv_igemm_x3h_wide_kernel<aae::X3H_OUT_PLANES, 2>), aae::kX3hWideSmem) \
    X(form == X3H_WIDE256 && tag == 3, (aae::conv_igemm_x3h_wide_kernel<aae::X3H_OUT_PLANES, 3>), aae::kX3hWideSmem) \
    AAE_X3H_FORMS_EXPERIMENTS(X) \
    X(form == X3H_F32 && dma, (aae::conv_igemm_x3h_dma_kernel<aae::X3H_OUT_F32>), aae::kConvIgemmSmem) \
    X(form == X3H_PLANES && dma && tag == 1, (aae::conv_igemm_x3h_dma_kernel<aae::X3H_OUT_PLANES, 1>), aae::kConvIgemmSmem) \
    X(form == X3H_PLANES && dma && tag == 2, (aae::conv_igemm_x3h_dma_kernel<aae::X3H_OUT_PLANES, 2>), aae::kConvIgemmSmem) \
    X(form == X3H_PLANES && dma && tag == 3, (aae::conv_igemm_x3h_dma_kernel<aae::X3H_OUT_PLANES, 3>), aae::kConvIgemmSmem) \
    X(form == X3H_PLANES && dma, (aae::conv_igemm_x3h_dma_kernel<aae::X3H_OUT_PLANES>), aae::kConvIgemmSmem) \
    X(form == X3H_PARTIAL && dma, (aae::conv_igemm_x3h_dma_kernel<aae::X3H_OUT_PARTIAL>), aae::kConvIgemmSmem)

// conv_wavek_f32_kernel / conv_wavek_multi_kernel<MT, NT, WAVES, DEPTH, TAG, SPREAD>: a shape (its key: launch_wavek) for the tags 1 ... 3 and 0 = any other layer.
// The product build carries the three forms the planner uses -- 4 waves, 2 slabs in flight, the spread schedules -- ; the forms that measured slower (8 waves, 3 slabs
// in flight, the burst schedules: CHANGELOG.md rounds 2-4) exist in the experiments build.
#define AAE_WAVEK_ROWS(X, K, key, MT, NT, WAVES, DEPTH, SPREAD) \
    X(form == key && tag == 1, (aae::K<MT, NT, WAVES, DEPTH, 1, SPREAD>), (aae::conv_wavek_smem<MT, NT, WAVES>())) \
    X(form == key && tag == 2, (aae::K<MT, NT, WAVES, DEPTH, 2, SPREAD>), (aae::conv_wavek_smem<MT, NT, WAVES>())) \
    X(form == key && tag == 3, (aae::K<MT, NT, WAVES, DEPTH, 3, SPREAD>), (aae::conv_wavek_smem<MT, NT, WAVES>())) \
    X(form == key && (tag < 1 || tag > 3), (aae::K<MT, NT, WAVES, DEPTH, 0, SPREAD>), (aae::conv_wavek_smem<MT, NT, WAVES>()))
constexpr int kWaveKOtherSchedule = 100000;      // added to a shape's key: the load schedule that is not the shape's default (burst for 64 x 64 and 32 x 32 tiles, spread for 64 x 32)
#ifdef AAE_EXPERIMENTS
#define AAE_WAVEK_FORMS_EXPERIMENTS(X) \
    AAE_WAVEK_ROWS(X, conv_wavek_f32_kernel, kWaveKOtherSchedule + 242, 2, 2, 4, 2, false) AAE_WAVEK_ROWS(X, conv_wavek_f32_kernel, kWaveKOtherSchedule + 1142, 1, 1, 4, 2, false) \
    AAE_WAVEK_ROWS(X, conv_wavek_f32_kernel, 243, 2, 2, 4, 3, false) AAE_WAVEK_ROWS(X, conv_wavek_f32_kernel, 282, 2, 2, 8, 2, false) \
    AAE_WAVEK_ROWS(X, conv_wavek_f32_kernel, 143, 2, 1, 4, 3, false) AAE_WAVEK_ROWS(X, conv_wavek_f32_kernel, 1143, 1, 1, 4, 3, false) \
    AAE_WAVEK_ROWS(X, conv_wavek_f32_kernel, 182, 2, 1, 8, 2, false) AAE_WAVEK_ROWS(X, conv_wavek_f32_kernel, 1182, 1, 1, 8, 2, false)
// (grouped: the spread schedule for 64 x 32 tiles and three slabs in flight for them -- aae_multi_impl.h, launch_wavek_multi)
#define AAE_WAVEK_MULTI_FORMS_EXPERIMENTS(X) \
    AAE_WAVEK_ROWS(X, conv_wavek_multi_kernel, kWaveKOtherSchedule + 142, 2, 1, 4, 2, true) AAE_WAVEK_ROWS(X, conv_wavek_multi_kernel, 143, 2, 1, 4, 3, false)
#else
#define AAE_WAVEK_FORMS_EXPERIMENTS(X)
#define AAE_WAVEK_MULTI_FORMS_EXPERIMENTS(X)
#endif
#define AAE_WAVEK_FORMS(X) \
    AAE_WAVEK_ROWS(X, conv_wavek_f32_kernel, 242, 2, 2, 4, 2, true) AAE_WAVEK_ROWS(X, conv_wavek_f32_kernel, 142, 2, 1, 4, 2, false) \
    AAE_WAVEK_ROWS(X, conv_wavek_f32_kernel, 1142, 1, 1, 4, 2, true) AAE_WAVEK_FORMS_EXPERIMENTS(X)
#define AAE_WAVEK_MULTI_FORMS(X) \
    AAE_WAVEK_ROWS(X, conv_wavek_multi_kernel, 242, 2, 2, 4, 2, true) AAE_WAVEK_ROWS(X, conv_wavek_multi_kernel, 142, 2, 1, 4, 2, false) \
    AAE_WAVEK_ROWS(X, conv_wavek_multi_kernel, 1142, 1, 1, 4, 2, true) AAE_WAVEK_MULTI_FORMS_EXPERIMENTS(X)

// conv_first_f32_kernel<KS, C, IN_U8, OUT_PLANES, VEC4, GROUP_SPLIT> at the layer's own LDS size (first_lds: Layer::first_smem) and the grouped query's
// conv_first_multi_kernel<KS, C, IN_U8, VEC4, GROUP_SPLIT> at the CU's 160 KB
#define AAE_FIRST_ROWS(X, C) \
    X(cin == C && group_split && vec4, (aae::conv_first_f32_kernel<5, C, true, false, true, true>), first_lds) \
    X(cin == C && group_split && u8, (aae::conv_first_f32_kernel<5, C, true, false, false, true>), first_lds) \
    X(cin == C && group_split, (aae::conv_first_f32_kernel<5, C, false, false, false, true>), first_lds) \
    X(cin == C && planes && vec4, (aae::conv_first_f32_kernel<5, C, true, true, true>), first_lds) \
    X(cin == C && planes && u8, (aae::conv_first_f32_kernel<5, C, true, true>), first_lds) \
    X(cin == C && planes, (aae::conv_first_f32_kernel<5, C, false, true>), first_lds) \
    X(cin == C && vec4, (aae::conv_first_f32_kernel<5, C, true, false, true>), first_lds) \
    X(cin == C && u8, (aae::conv_first_f32_kernel<5, C, true, false>), first_lds) \
    X(cin == C, (aae::conv_first_f32_kernel<5, C, false, false>), first_lds)
#define AAE_FIRST_FORMS(X) AAE_FIRST_ROWS(X, 3) AAE_FIRST_ROWS(X, 1)
#define AAE_FIRST_MULTI_ROWS(X, C, GROUP_SPLIT) \
    X(cin == C && group_split == GROUP_SPLIT && vec4, (aae::conv_first_multi_kernel<5, C, true, true, GROUP_SPLIT>), 160 * 1024) \
    X(cin == C && group_split == GROUP_SPLIT && u8, (aae::conv_first_multi_kernel<5, C, true, false, GROUP_SPLIT>), 160 * 1024) \
    X(cin == C && group_split == GROUP_SPLIT, (aae::conv_first_multi_kernel<5, C, false, false, GROUP_SPLIT>), 160 * 1024)
#define AAE_FIRST_MULTI_FORMS(X) AAE_FIRST_MULTI_ROWS(X, 3, true) AAE_FIRST_MULTI_ROWS(X, 3, false) AAE_FIRST_MULTI_ROWS(X, 1, true) AAE_FIRST_MULTI_ROWS(X, 1, false)

// dense_gemv_f32_kernel<MQ, TICKET> and dense_gemv_multi_kernel<MQ>: the activation chunk + half sums of MQ batch rows, or the finishing block's row-group sums
constexpr int gemv_smem(int mq, bool ticket) {
    return (ticket && 2 * mq * aae::kGemvChunk * (int)sizeof(float) + 16 < aae::kGemvTicketSmem) ? aae::kGemvTicketSmem : 2 * mq * aae::kGemvChunk * (int)sizeof(float) + 16;
}
#define AAE_GEMV_ROWS(X, TICKET) \
    X(ticket == TICKET && mq == 1, (aae::dense_gemv_f32_kernel<1, TICKET>), gemv_smem(1, TICKET)) X(ticket == TICKET && mq == 2, (aae::dense_gemv_f32_kernel<2, TICKET>), gemv_smem(2, TICKET)) \
    X(ticket == TICKET && mq == 3, (aae::dense_gemv_f32_kernel<3, TICKET>), gemv_smem(3, TICKET)) X(ticket == TICKET && mq == 4, (aae::dense_gemv_f32_kernel<4, TICKET>), gemv_smem(4, TICKET)) \
    X(ticket == TICKET && mq == 8, (aae::dense_gemv_f32_kernel<8, TICKET>), gemv_smem(8, TICKET))
#ifdef AAE_EXPERIMENTS
#define AAE_GEMV_FORMS(X) AAE_GEMV_ROWS(X, true) AAE_GEMV_ROWS(X, false)       // (without the in-launch finish: a reduce launch adds up the chunk rows)
#else
#define AAE_GEMV_FORMS(X) AAE_GEMV_ROWS(X, true)
#endif
#define AAE_GEMV_MULTI_FORMS(X) \
    X(mq == 1, (aae::dense_gemv_multi_kernel<1>), gemv_smem(1, true)) X(mq == 2, (aae::dense_gemv_multi_kernel<2>), gemv_smem(2, true)) \
    X(mq == 3, (aae::dense_gemv_multi_kernel<3>), gemv_smem(3, true)) X(mq == 4, (aae::dense_gemv_multi_kernel<4>), gemv_smem(4, true))

// the grouped query's scans, as far as aae_multi_impl.h launches them: scan_stream_multi_kernel<NQ> and scan_resident_multi_kernel<RH>
#define AAE_SCAN_STREAM_MULTI_ROWS(X, NQ) X(nq == NQ, (aae::scan_stream_multi_kernel<NQ>), NQ * 128 * (int)sizeof(float) + aae::kScanTicketSmem)
#define AAE_SCAN_STREAM_MULTI_FORMS(X) AAE_SCAN_STREAM_MULTI_ROWS(X, 1) AAE_SCAN_STREAM_MULTI_ROWS(X, 2) AAE_SCAN_STREAM_MULTI_ROWS(X, 3) AAE_SCAN_STREAM_MULTI_ROWS(X, 4)
#define AAE_SCAN_RESIDENT_MULTI_ROWS(X, RH) X(rh == RH, (aae::scan_resident_multi_kernel<RH>), (aae::scan_resident_smem<false, RH>()))
#define AAE_SCAN_RESIDENT_MULTI_FORMS(X) AAE_SCAN_RESIDENT_MULTI_ROWS(X, 1) AAE_SCAN_RESIDENT_MULTI_ROWS(X, 2) AAE_SCAN_RESIDENT_MULTI_ROWS(X, 4)

#ifdef AAE_EXPERIMENTS
// detect_chain_kernel<MQ, S0, S1, S2>: (batch class, wave-tile shape code of conv2 ... conv4) -- what plan_wavek gives the reference network at B = 1, 2, 3, 4
#define AAE_CHAIN_FORMS(X) \
    X(mq == 1 && shapes == 0, (aae::detect_chain_kernel<1, 0, 0, 0>), aae::kChainSmem) X(mq == 2 && shapes == 100, (aae::detect_chain_kernel<2, 1, 0, 0>), aae::kChainSmem) \
    X(mq == 4 && shapes == 10, (aae::detect_chain_kernel<4, 0, 1, 0>), aae::kChainSmem) X(mq == 4 && shapes == 210, (aae::detect_chain_kernel<4, 2, 1, 0>), aae::kChainSmem)
// conv_wino_phase_kernel<TH, TW, SWAP, GEOM>: the four polyphase components as launches of their own, per block geometry
#define AAE_WINO_PHASE_ROWS(X, GEOM) \
    X(geom == GEOM && eh && ew, (aae::conv_wino_phase_kernel<3, 3, false, GEOM>), (aae::wino_smem_bytes<GEOM>())) \
    X(geom == GEOM && eh && !ew, (aae::conv_wino_phase_kernel<3, 2, false, GEOM>), (aae::wino_smem_bytes<GEOM>())) \
    X(geom == GEOM && !eh && ew, (aae::conv_wino_phase_kernel<3, 2, true, GEOM>), (aae::wino_smem_bytes<GEOM>())) \
    X(geom == GEOM && !eh && !ew, (aae::conv_wino_phase_kernel<2, 2, false, GEOM>), (aae::wino_smem_bytes<GEOM>()))
#define AAE_WINO_PHASE_FORMS(X) AAE_WINO_PHASE_ROWS(X, 0) AAE_WINO_PHASE_ROWS(X, 2)
#endif

// The LDS ceiling of every form of every list, raised when a handle is created (on the device the handle lives on: the attribute belongs to the device's copy of
// the function) -- never in front of a launch.  A grouped query cannot run without an encoder handle, so the handle's creation covers its kernels too.
static void set_launch_attributes(const aae_encoder* enc) {
    wino_set_attributes();
    AAE_IGEMM_FORMS(AAE_FORM_CEILING)
    AAE_X3H_FORMS(AAE_FORM_CEILING)
    AAE_WAVEK_FORMS(AAE_FORM_CEILING)
    AAE_WAVEK_MULTI_FORMS(AAE_FORM_CEILING)
    AAE_GEMV_FORMS(AAE_FORM_CEILING)
    AAE_GEMV_MULTI_FORMS(AAE_FORM_CEILING)
    AAE_SCAN_STREAM_MULTI_FORMS(AAE_FORM_CEILING)
    AAE_SCAN_RESIDENT_MULTI_FORMS(AAE_FORM_CEILING)
    AAE_FIRST_MULTI_FORMS(AAE_FORM_CEILING)
#ifdef AAE_EXPERIMENTS
    AAE_CHAIN_FORMS(AAE_FORM_CEILING)
    AAE_WINO_PHASE_FORMS(AAE_FORM_CEILING)
#endif
    if (!enc->layers.empty() && enc->layers[0].kind == KIND_FIRST_MFMA) {          // (a decoder's context has no conv1)
        const int first_lds = enc->layers[0].first_smem;
        AAE_FIRST_FORMS(AAE_FORM_CEILING)
    }
}

// ------------------------------------------------------------ shared pieces of the conv launches
// What the four conv argument records (ConvIgemmArgs of the encoder and of the decoder, ConvWaveKArgs, ConvIgemmX3hArgs) take from the layer: bias / folded batch
// norm, the geometry of M output rows, the byte sizes of the two buffer views -- and the one check that the input fits a 32-bit view (fp32 and fp16-pair
// activations: 4 bytes per element either way).
template <class Args>
static int conv_layer_args(Args& a, const Layer& L, int M, const char* name) {
    a.bias = L.bias; a.bn_scale = L.bn_scale; a.bn_shift = L.bn_shift;
    a.H = L.H; a.W = L.W; a.Cin = L.Cin; a.Ho = L.Ho; a.Wo = L.Wo; a.Cout = L.Cout; a.CoutPad = L.CoutPad;
    a.KS = L.KS; a.S = L.S; a.pt = L.pt; a.pl = L.pl; a.M = M; a.relu = L.relu;
    const unsigned long long x_bytes = (unsigned long long)(M / (L.Ho * L.Wo)) * L.H * L.W * L.Cin * sizeof(float);
    a.x_bytes = (unsigned)x_bytes;
    a.slabs_total = (int)(L.K() / 32);
    a.wp_bytes = (unsigned)((unsigned long long)a.slabs_total * 8ull * L.CoutPad * 16ull);
    if (x_bytes >= 0xFFFFFFF0ull)
        return fail(AAE_ERR_UNSUPPORTED, "%s: input activation of %llu bytes exceeds the 4 GiB buffer view; use a smaller batch", name, x_bytes);
    return AAE_OK;
}

// the second launch of a split-K layer: partial sums [splits][M][Cout] -> bias / ReLU / batch norm -> the layer's output (planes: fp16 pairs of value * out_scale)
static int launch_reduce_tail(const aae_encoder* enc, const Layer& L, const float* partial, float* out, long long M, int splits, bool planes, float out_scale,
                              hipStream_t stream, Timer& tm, const char* name) {
    aae::SplitKReduceArgs r;
    r.partial = partial; r.bias = L.bias; r.bn_scale = L.bn_scale; r.bn_shift = L.bn_shift; r.out = out;
    r.MN = M * L.Cout; r.Cout = L.Cout; r.splits = splits; r.relu = L.relu;
    r.out_planes = planes ? 1 : 0; r.out_scale = out_scale; r.sat_flag = planes ? t_x3h_flag : nullptr;
    launch_splitk_reduce(r, stream, enc->reduce_small != 0);
    return launch_done(tm, 0.0, "%s:splitk_reduce", name);
}

static bool launch_igemm_form(int form, bool dma, int tag, dim3 grid, int smem, hipStream_t stream, const aae::ConvIgemmArgs& a) {
    const dim3 block(256);
    AAE_IGEMM_FORMS(AAE_FORM_LAUNCH_SMEM)
    return false;
}

static int launch_igemm(aae_encoder* enc, const Layer& L, const float* x, int M, float* out, float* partial,
                        hipStream_t stream, Timer& tm, const char* name, int tag = 0) {
    aae::ConvIgemmArgs a;
    a.x = x; a.wp = L.wp; a.stagger = enc->igemm_stagger;
    if (int rc = conv_layer_args(a, L, M, name)) return rc;
    a.num_mt = ceil_div(M, 128);
    a.num_nt = L.CoutPad / 128;
    choose_splits(enc, a.num_mt * a.num_nt, a.slabs_total, &a.splits, &a.slabs_per_split);
    const int nblk = a.num_mt * a.num_nt * a.splits;
    const double flops = 2.0 * (double)M * (double)L.K() * (double)L.Cout;
#ifdef AAE_EXPERIMENTS
    const bool dma = enc->igemm_dma != 0;
#else
    const bool dma = true;                     // (the register-staged operand path: experiments build)
#endif
    const char* kname = dma ? "conv_igemm_f32_dma" : "conv_igemm_f32";
    const char* missing = "%s: no igemm instantiation for form %d, tag %d in this build";
    if (a.splits == 1) {
        a.out = out;
#ifdef AAE_EXPERIMENTS
        const bool breg = dma && enc->igemm_breg && tag >= 1 && tag <= 3;
#else
        const bool breg = tag >= 1 && tag <= 3;   // (weights through LDS for the conv layers: experiments build)
#endif
        // 128 x 256 block tiles (each wave 64 x 128) where the layer is wide enough and the grid stays large
        if (breg && enc->igemm_breg_wide && (tag == 1 || tag == 2) && L.CoutPad % 256 == 0 &&
            a.num_mt * (L.CoutPad / 256) >= enc->igemm_breg_wide_min_blocks) {
            a.num_nt = L.CoutPad / 256;
            if (!launch_igemm_form(IGEMM_BREG_N256, dma, tag, dim3(a.num_mt * a.num_nt), 2 * aae::kSlabFloatsA * 4, stream, a))
                return fail(AAE_ERR_RUNTIME, missing, name, IGEMM_BREG_N256, tag);
            return launch_done(tm, flops, "%s:conv_igemm_f32_dma_breg_n256 M=%d N=%d K=%lld", name, M, L.Cout, L.K());
        }
        // weights in registers: A buffers only (32 KB: three blocks per CU); grids too small to give every CU three blocks keep the
        // 64 KB footprint so that the blocks spread two per CU instead of 3/2/1
        const int smem = breg && nblk >= enc->igemm_breg_min_blocks ? 2 * aae::kSlabFloatsA * 4 : aae::kConvIgemmSmem;
        if (!launch_igemm_form(breg ? IGEMM_BREG : IGEMM_PLAIN, dma, tag, dim3(nblk), smem, stream, a))
            return fail(AAE_ERR_RUNTIME, missing, name, breg ? IGEMM_BREG : IGEMM_PLAIN, tag);
        return launch_done(tm, flops, "%s:%s M=%d N=%d K=%lld", name, breg ? "conv_igemm_f32_dma_breg" : kname, M, L.Cout, L.K());
    }
    a.out = partial;
    if (!launch_igemm_form(IGEMM_SPLITK, dma, tag, dim3(nblk), aae::kConvIgemmSmem, stream, a)) return fail(AAE_ERR_RUNTIME, missing, name, IGEMM_SPLITK, tag);
    if (int rc = launch_done(tm, flops, "%s:%s_splitk%d M=%d N=%d K=%lld", name, kname, a.splits, M, L.Cout, L.K())) return rc;
    return launch_reduce_tail(enc, L, partial, out, M, a.splits, false, 1.f, stream, tm, name);
}

// wave-split-K igemm (conv_wavek_f32.h): small M -- the per-detection batches.  form: the plan's shape key (+ kWaveKOtherSchedule)
static bool launch_wavek_form(int form, int tag, int waves, dim3 grid, hipStream_t stream, const aae::ConvWaveKArgs& a) {
    const dim3 block(64 * waves);
    AAE_WAVEK_FORMS(AAE_FORM_LAUNCH)
    return false;
}

// (conv_layer_args' 4 GiB check is not expected to fire here -- plan_wavek refuses such a layer (plan_wavek_core), and the grouped query plans rows that plan_wavek
//  accepted for the same detections (multi_encoder_groupable) or at most three 16 x 16 images (plan_mid_ragged) -- ; its answer is ignored, so this function returns
//  what it returned before the check moved into the shared fill)
static aae::ConvWaveKArgs wavek_args(const aae_encoder* enc, const Layer& L, const WaveKPlan& w, const float* x, int M, float* out, float* partial,
                                     unsigned long long* tickets, unsigned nonce, int tag) {
    aae::ConvWaveKArgs a;
    a.x = x; a.wp = L.wp; a.out = out;
    a.partial = partial; a.partial_bytes = (unsigned)w.partial_bytes; a.tickets = tickets; a.nonce = nonce;
    (void)conv_layer_args(a, L, M, "wave-split-K layer");
    a.ablate = enc->wavek_ablate; a.pingpong = enc->wavek_pingpong; a.spread = enc->wavek_spread;
    a.timeline = (enc->wavek_timeline && tag >= 1 && tag <= 3 && w.blocks() <= 512)       // (the debug buffer holds 512 blocks per layer)
                     ? enc->wavek_timeline + (size_t)(tag - 1) * 512 * 8 : nullptr;
    a.num_mt = w.num_mt; a.num_nt = w.num_nt; a.gsplits = w.gsplits;
    a.tail_tiles = w.tail_tiles; a.tail_gsplits = w.tail_g;
    return a;
}

static int launch_wavek(aae_encoder* enc, const Layer& L, const WaveKPlan& w, const float* x, int M, float* out, float* partial,
                        unsigned long long* tickets, unsigned nonce, hipStream_t stream, Timer& tm, const char* name, int tag) {
    const aae::ConvWaveKArgs a = wavek_args(enc, L, w, x, M, out, partial, tickets, nonce, tag);
    const int key = wavek_shape_key(w);
    const bool burst = (key == 242 && !(a.spread & 1)) || (key == 1142 && !(a.spread & 2));
    if (!launch_wavek_form(key + (burst ? kWaveKOtherSchedule : 0), tag, w.waves, dim3(w.blocks()), stream, a))
        return fail(AAE_ERR_RUNTIME, "%s: no wave-split-K instantiation for MT=%d NT=%d waves=%d depth=%d spread=%d in this build", name, w.MT, w.NT, w.waves, w.depth, a.spread);
    char tail[24] = "";
    if (w.tail_tiles > 0) snprintf(tail, sizeof(tail), "t%dx%d", w.tail_tiles, w.tail_g);       // (e.g. g1t64x4: the last 64 tiles cut four ways)
    return launch_done(tm, 2.0 * (double)M * (double)L.K() * (double)L.Cout, "%s:conv_wavek_f32_%dx%d_w%d_d%d_g%d%s M=%d N=%d K=%lld", name, 32 * w.MT, 32 * w.NT,
                       w.waves, w.depth, w.gsplits, tail, M, L.Cout, L.K());
}

static bool launch_x3h_form(int form, bool dma, int tag, dim3 grid, hipStream_t stream, const aae::ConvIgemmX3hArgs& a) {
    const dim3 block(form == X3H_WIDE256 || form == X3H_WIDE128 ? 512 : 256);          // (the wide tiles: 8 waves)
    AAE_X3H_FORMS(AAE_FORM_LAUNCH)
    return false;
}

// f32x3h variant: x and (unless out_f32) out are fp16 (hi, lo) pairs of value * 2^x3h_act_shift (x3h_pair_index layout).
static int launch_igemm_x3h(aae_encoder* enc, const Layer& L, const void* x, int M, void* out, bool out_f32, float* partial,
                            hipStream_t stream, Timer& tm, const char* name, int tag = 0) {
    aae::ConvIgemmX3hArgs a;
    a.x = static_cast<const unsigned short*>(x); a.wp = L.wp16;
    if (int rc = conv_layer_args(a, L, M, name)) return rc;
    a.inv_scale = ldexpf(1.f, -(enc->x3h_act_shift + L.w_shift));
    a.out_scale = ldexpf(1.f, enc->x3h_act_shift);
    a.sat_flag = out_f32 ? nullptr : t_x3h_flag;
    a.num_mt = ceil_div(M, 128);
    a.num_nt = L.CoutPad / 128;
    choose_splits(enc, a.num_mt * a.num_nt, a.slabs_total, &a.splits, &a.slabs_per_split);
    const int nblk = a.num_mt * a.num_nt * a.splits;
    const double flops = 2.0 * (double)M * (double)L.K() * (double)L.Cout;
#ifdef AAE_EXPERIMENTS
    const bool dma = enc->x3h_dma != 0;
#else
    const bool dma = true;
#endif
    const char* kname = dma ? "conv_igemm_x3h_dma" : "conv_igemm_x3h";
    const char* missing = "%s: no f32x3h igemm instantiation for form %d, tag %d in this build";
    // 256 x 256 tiles, 8 waves of 64 x 128 (LDS traffic per MFMA -33 %): layers with Cout % 256 == 0 whose grid still fills the chip
    const bool wide256 = dma && !out_f32 && enc->x3h_wide256 && L.CoutPad % 256 == 0 && tag >= 1 && tag <= 3 &&
                         ceil_div(M, 256) * (L.CoutPad / 256) >= enc->x3h_wide256_min_blocks;
    bool wide128 = false;
#ifdef AAE_EXPERIMENTS
    // 256 x 128 tiles (8 waves, one block per CU) when they still give every CU a block
    wide128 = !wide256 && dma && !out_f32 && tag >= 1 && tag <= 3 && enc->x3h_wide_min_blocks > 0 && ceil_div(M, 256) * a.num_nt >= enc->x3h_wide_min_blocks;
#endif
    if (wide256 || wide128) {
        a.num_mt = ceil_div(M, 256);
        if (wide256) a.num_nt = L.CoutPad / 256;
        a.splits = 1;
        a.slabs_per_split = a.slabs_total;
        a.out = out;
        const int form = wide256 ? X3H_WIDE256 : X3H_WIDE128;
        if (!launch_x3h_form(form, dma, tag, dim3(a.num_mt * a.num_nt), stream, a)) return fail(AAE_ERR_RUNTIME, missing, name, form, tag);
        return launch_done(tm, flops, "%s:conv_igemm_x3h_%s M=%d N=%d K=%lld", name, wide256 ? "wide256" : "dma256", M, L.Cout, L.K());
    }
    if (a.splits == 1) {
        a.out = out;
        const int form = out_f32 ? X3H_F32 : X3H_PLANES;
        if (!launch_x3h_form(form, dma, tag, dim3(nblk), stream, a)) return fail(AAE_ERR_RUNTIME, missing, name, form, tag);
        return launch_done(tm, flops, "%s:%s M=%d N=%d K=%lld", name, kname, M, L.Cout, L.K());
    }
    a.out = partial;
    if (!launch_x3h_form(X3H_PARTIAL, dma, tag, dim3(nblk), stream, a)) return fail(AAE_ERR_RUNTIME, missing, name, X3H_PARTIAL, tag);
    if (int rc = launch_done(tm, flops, "%s:%s_splitk%d M=%d N=%d K=%lld", name, kname, a.splits, M, L.Cout, L.K())) return rc;
    return launch_reduce_tail(enc, L, partial, static_cast<float*>(out), M, a.splits, !out_f32, a.out_scale, stream, tm, name);
}

// group_split (never with planes): per-detection batches, one block per 32-pixel group -- the caller's grid has z = 4
static bool launch_first_form(int cin, bool u8, bool vec4, bool planes, bool group_split, dim3 grid, int smem, hipStream_t stream, const aae::ConvFirstArgs& a) {
    const dim3 block(256);
    AAE_FIRST_FORMS(AAE_FORM_LAUNCH_SMEM)
    return false;
}

// arguments of the first-layer kernel for a batch of B crops; returns the number of tile runs (blocks along grid.x)
static int first_core_args(const aae_encoder* enc, const Layer& L, const void* x, bool u8, int B, float* out, bool planes, aae::ConvFirstCore& a) {
    a.x = x; a.lut = enc->lut; a.w = L.w_hwio; a.bias = L.bias; a.bn_scale = L.bn_scale; a.bn_shift = L.bn_shift;
    a.out = out; a.H = L.H; a.W = L.W; a.Ho = L.Ho; a.Wo = L.Wo; a.Cout = L.Cout;
    a.S = L.S; a.pt = L.pt; a.pl = L.pl; a.relu = L.relu;
    a.vec4 = (u8 && L.rowlen4 > 0 && enc->first_vec4 && (reinterpret_cast<uintptr_t>(x) & 3) == 0) ? 1 : 0;   // dword loads want a 4-byte aligned batch
    a.rowlen = a.vec4 ? L.rowlen4 : L.rowlen;
    a.lead = a.vec4 ? L.lead4 : 0;
    a.out_scale = ldexpf(1.f, enc->x3h_act_shift);
    a.sat_flag = planes ? t_x3h_flag : nullptr;
    a.tiles_per_image = ceil_div(L.Ho * L.Wo, 128);
    a.total_tiles = B * a.tiles_per_image;
    int tpb = ceil_div(a.total_tiles, enc->first_target_blocks);
    if (tpb < 1) tpb = 1;
    if (tpb > enc->first_max_tiles_per_block) tpb = enc->first_max_tiles_per_block;
    a.tiles_per_block = tpb;
    return ceil_div(a.total_tiles, tpb);
}

static int launch_first(aae_encoder* enc, const Layer& L, const void* x, bool u8, int B, float* out, bool planes,
                        hipStream_t stream, Timer& tm, const aae::TicketPrep* prep = nullptr) {
    aae::ConvFirstArgs a;
    if (prep) a.prep = *prep;
    else a.prep.n = 0;
    const int runs = first_core_args(enc, L, x, u8, B, out, planes, a);
    // per-detection batches: the four 32-pixel groups of every tile go to four blocks (10.6 -> ? us at B = 1)
    const bool group_split = !planes && a.total_tiles <= enc->first_group_split_max_tiles;
    const dim3 grid(runs + (a.prep.n > 0 ? 1 : 0), ceil_div(L.Cout, 128), group_split ? 4 : 1);    // + the ticket-preparation block
    if (!launch_first_form(L.Cin, u8, u8 && a.vec4, planes, group_split, grid, L.first_smem, stream, a))
        return fail(AAE_ERR_RUNTIME, "conv1: no first-layer instantiation for %d input channels in this build", L.Cin);
    return launch_done(tm, 2.0 * (double)B * L.Ho * L.Wo * (double)L.K() * L.Cout, "conv1:conv_first_f32%s M=%d N=%d K=%lld", group_split ? "_g4" : "",
                       B * L.Ho * L.Wo, L.Cout, L.K());
}

static int launch_generic(aae_encoder* enc, const Layer& L, const void* x, bool u8, long long B, float* out,
                          hipStream_t stream, Timer& tm, const char* name) {
    aae::ConvDirectArgs a;
    a.x = x; a.lut = enc->lut; a.w = L.w_hwio; a.bias = L.bias; a.bn_scale = L.bn_scale; a.bn_shift = L.bn_shift;
    a.out = out; a.H = L.H; a.W = L.W; a.Cin = L.Cin; a.Ho = L.Ho; a.Wo = L.Wo; a.Cout = L.Cout;
    a.KS = L.KS; a.S = L.S; a.pt = L.pt; a.pl = L.pl; a.relu = L.relu;
    a.total = B * L.Ho * L.Wo * L.Cout;
    long long blocks = (a.total + 255) / 256;
    if (blocks > 8192) blocks = 8192;
    if (u8) AAE_LAUNCH((aae::conv_direct_generic_kernel<true>), dim3((unsigned)blocks), dim3(256), 0, stream, a);
    else AAE_LAUNCH((aae::conv_direct_generic_kernel<false>), dim3((unsigned)blocks), dim3(256), 0, stream, a);
    return launch_done(tm, 2.0 * (double)B * L.Ho * L.Wo * (double)L.K() * L.Cout, "%s:conv_direct_generic", name);
}

// dense layer at B <= 8: weight-streaming GEMV + the fixed-order chunk reduction
static int gemv_max_batch(const aae_encoder* enc) {
    return enc->dense_gemv_max_batch < 1 ? 1 : (enc->dense_gemv_max_batch > aae::kGemvMaxBatch ? aae::kGemvMaxBatch : enc->dense_gemv_max_batch);
}
static bool gemv_uses_ticket(const aae_encoder* enc, const Layer& D) {
    return enc->gemv_ticket && D.Cout % 4 == 0 && D.CoutPad / 128 <= kGemvTicketSlots;
}

static aae::DenseGemvArgs gemv_args(const Layer& D, const float* x, int B, float* partial) {
    aae::DenseGemvArgs a;
    a.x = x; a.wp = D.wp; a.partial = partial; a.B = B; a.K = (int)D.K(); a.Cout = D.Cout; a.CoutPad = D.CoutPad;
    a.wp_bytes = (unsigned)((unsigned long long)(D.K() / 4) * D.CoutPad * 16ull);
    a.partial_bytes = (unsigned)gemv_partial_bytes(D, B);
    a.bias = nullptr; a.bn_scale = nullptr; a.bn_shift = nullptr; a.out = nullptr; a.tickets = nullptr; a.nonce = 0; a.relu = 0;
    return a;
}

static bool launch_gemv_form(int mq, bool ticket, dim3 grid, hipStream_t stream, const aae::DenseGemvArgs& a) {
    const dim3 block(256);
    AAE_GEMV_FORMS(AAE_FORM_LAUNCH)
    return false;
}

static int launch_dense_gemv(aae_encoder* enc, const Layer& D, const float* x, int B, float* out, float* partial,
                             unsigned long long* tickets, unsigned nonce, hipStream_t stream, Timer& tm) {
    aae::DenseGemvArgs a = gemv_args(D, x, B, partial);
    const int chunks = ceil_div(a.K, aae::kGemvChunk);
    const dim3 grid(chunks, D.CoutPad / 128);
    const int MQ = B <= 4 ? B : 8;
    const bool ticket = tickets && gemv_uses_ticket(enc, D);
    if (ticket) {
        a.bias = D.bias; a.bn_scale = D.bn_scale; a.bn_shift = D.bn_shift; a.out = out;
        a.tickets = tickets;
        a.nonce = nonce; a.relu = D.relu;
    }
    // (without the in-launch finish: the experiments build -- forward_impl never plans it in the product build)
    if (!launch_gemv_form(MQ, ticket, grid, stream, a)) return fail(AAE_ERR_RUNTIME, "dense GEMV for %d rows%s: no instantiation in this build", MQ, ticket ? "" : " without its in-launch finish");
    if (int rc = launch_done(tm, 2.0 * B * (double)D.K() * D.Cout, "dense:dense_gemv_f32%s chunks=%d M=%d N=%d K=%d", ticket ? "_ticket" : "", chunks, B, D.Cout, a.K)) return rc;
    return ticket ? AAE_OK : launch_reduce_tail(enc, D, partial, out, B, chunks, false, 1.f, stream, tm, "dense");
}

// One extra ticket range the first kernel of the forward prepares for a launch that FOLLOWS the encoder on the same
// stream (the single-launch codebook scan of aae_encode_nn).
struct ExtraTicketPrep {
    unsigned long long* words = nullptr;
    int count = 0;
    unsigned nonce = 0;
    // aae_encode_nn, B <= 4, top-1 on the fp32 stream scan: the scan itself, ready to run as the last phase of the persistent
    // per-detection launch (tickets / nonce = the words above)
    bool scan_ready = false;
    aae::ScanArgs scan;
};

#ifdef AAE_EXPERIMENTS
// The persistent per-detection launch (detect_chain.h) serves a forward when every layer behind the first runs the
// wave-split-K kernel in one of its three 4-wave / depth-2 shapes, the dense layer is the ticketed GEMV, and each layer
// output has its own buffer.
static int chain_shape_code(const WaveKPlan& w) { return w.MT == 1 ? 0 : (w.NT == 1 ? 1 : 2); }

// the instantiated (batch class, shape sequence) kernels: what plan_wavek gives the reference network at B = 1, 2, 3, 4
struct ChainVariant { int mq, s0, s1, s2; };
static const ChainVariant kChainVariants[] = {{1, 0, 0, 0}, {2, 1, 0, 0}, {4, 0, 1, 0}, {4, 2, 1, 0}};

static bool chain_eligible(const aae_encoder* enc, int B, const std::vector<WaveKPlan>& plans, bool dense_gemv_ticket) {
    const size_t nl = enc->layers.size();
    if (!enc->detect_chain || B > 4 || nl != (size_t)aae::kChainConv + 1 || enc->compact_workspace || !dense_gemv_ticket) return false;
    if (enc->wavek_ablate || (enc->wavek_timeline && !enc->chain_timeline)) return false;   // (profiling aids of the stand-alone launches)
    if (enc->wavek_spread != 3) return false;                  // (the phases are compiled with the default schedules)
    for (size_t li = 1; li < nl; ++li) {
        const WaveKPlan& w = plans[li];
        if (!w.use || w.waves != 4 || w.depth != 2 || w.tail_tiles > 0 || enc->layers[li].Cout % 4 != 0) return false;
        if (!((w.MT == 1 && w.NT == 1) || (w.MT == 2 && w.NT == 1) || (w.MT == 2 && w.NT == 2))) return false;
    }
    if (enc->dense.Cout % 4 != 0) return false;
    const int mq = B <= 2 ? B : 4;
    for (const ChainVariant& v : kChainVariants)
        if (v.mq == mq && v.s0 == chain_shape_code(plans[1]) && v.s1 == chain_shape_code(plans[2]) && v.s2 == chain_shape_code(plans[3])) return true;
    return false;
}

// (every block resident at once: the kernel waits grid-wide)
#define AAE_FORM_LAUNCH_RESIDENT(when, kernel, lds) if (when) { AAE_LAUNCH_RESIDENT(kernel, grid, block, lds, stream, a); return true; }
static bool launch_chain_form(int mq, int shapes, dim3 grid, hipStream_t stream, const aae::DetectChainArgs& a) {
    const dim3 block(256);
    AAE_CHAIN_FORMS(AAE_FORM_LAUNCH_RESIDENT)
    return false;
}

static int launch_detect_chain(aae_encoder* enc, int B, const std::vector<WaveKPlan>& plans, const std::vector<unsigned>& nonces, unsigned gemv_nonce,
                               unsigned barrier_nonce, const float* act0, unsigned char* base, const Workspace& ws, unsigned long long* tickets, float* z_out,
                               const ExtraTicketPrep* extra, hipStream_t stream, Timer& tm) {
    const size_t nl = enc->layers.size();
    const Layer& D = enc->dense;
    aae::DetectChainArgs a;
    memset(&a, 0, sizeof(a));
    const float* cur = act0;
    double flops = 0.0;
    for (size_t li = 1; li < nl; ++li) {
        const Layer& L = enc->layers[li];
        const WaveKPlan& w = plans[li];
        float* out = reinterpret_cast<float*>(base + ws.act_off[li]);
        a.conv[li - 1] = wavek_args(enc, L, w, cur, B * L.Ho * L.Wo, out, reinterpret_cast<float*>(base + ws.chain_partial_off[li]),
                                    tickets + li * kLayerTicketWords, nonces[li], 0);          // (tag 0: no per-layer stamps ...)
        // ... unless option chain_timeline = 1 + layer asks for the phase stamps of ONE conv layer, kept behind the launch's own stamps
        if (enc->chain_timeline == 1 + (int)li && enc->wavek_timeline && w.num_mt * w.num_nt * w.gsplits <= 256)
            a.conv[li - 1].timeline = enc->wavek_timeline + 256 * aae::kChainStamps;
        flops += 2.0 * (double)B * L.Ho * L.Wo * (double)L.K() * L.Cout;
        cur = out;
    }
    a.dense = gemv_args(D, cur, B, reinterpret_cast<float*>(base + ws.chain_partial_off[nl]));
    a.dense.bias = D.bias; a.dense.bn_scale = D.bn_scale; a.dense.bn_shift = D.bn_shift; a.dense.out = z_out; a.dense.relu = D.relu;
    a.dense.tickets = tickets + kConvTicketBytes / 8; a.dense.nonce = gemv_nonce;
    a.dense_tiles = D.CoutPad / 128;
    a.dense_chunks = ceil_div((int)D.K(), aae::kGemvChunk);
    flops += 2.0 * B * (double)D.K() * D.Cout;
    a.has_scan = (extra && extra->scan_ready) ? 1 : 0;
    if (a.has_scan) {
        a.scan = extra->scan;
        flops += 2.0 * B * (double)a.scan.N * a.scan.J;
    }
    a.barrier.words = tickets + (kConvTicketBytes + kGemvTicketBytes) / 8;
    a.barrier.nonce = barrier_nonce;
    a.timeline = (enc->chain_timeline && enc->wavek_timeline) ? enc->wavek_timeline : nullptr;      // (3 * 512 * 8 stamps: up to 307 blocks x 40)
    if (a.timeline && (size_t)std::min(enc->detect_chain_blocks, enc->cu_count > 0 ? enc->cu_count : enc->detect_chain_blocks) * aae::kChainStamps > 3u * 512u * 8u) a.timeline = nullptr;
    int grid = enc->detect_chain_blocks;
    if (enc->cu_count > 0 && grid > enc->cu_count) grid = enc->cu_count;
    if (grid < 1) grid = 1;
    const int shapes = chain_shape_code(plans[1]) * 100 + chain_shape_code(plans[2]) * 10 + chain_shape_code(plans[3]);
    if (!launch_chain_form(B <= 2 ? B : 4, shapes, dim3(grid), stream, a))               // (kChainVariants)
        return fail(AAE_ERR_RUNTIME, "no persistent per-detection kernel for batch %d / wave-tile shapes %d", B, shapes);
    return launch_done(tm, flops, "chain:detect_chain_f32 B=%d blocks=%d shapes=%d%d%d phases=conv2..conv%zu+dense%s", B, grid, chain_shape_code(plans[1]),
                       chain_shape_code(plans[2]), chain_shape_code(plans[3]), nl, a.has_scan ? "+scan" : "");
}

#endif  // AAE_EXPERIMENTS

#ifdef AAE_EXPERIMENTS
// A conv layer as four polyphase Winograd launches (conv_winograd_f32.h): the phases add up in the output buffer, the last one applies
// bias / ReLU / BN.  The 3 x 3-tap phase goes first (it stores), the 2 x 2-tap one last.
static bool launch_wino_phase_form(int geom, int eh, int ew, dim3 grid, hipStream_t stream, const aae::ConvWinoArgs& a) {
    const dim3 block(512);
    AAE_WINO_PHASE_FORMS(AAE_FORM_LAUNCH)
    return false;
}
#endif

// 64-column blocks of a region per XCD (conv_winograd_f32.h: wino_block).  Option winograd_xcd_cols: -1 = the measured default per layer,
// 0 = plain block order, S > 0 = S where the layer's column-block count allows it.
static int wino_xcd_cols(const aae_encoder* enc, const Layer& L) {
    const int nbn = L.Cout / 64;
    int s = enc->winograd_xcd_cols;
    if (s < 0) s = nbn >= 8 ? 4 : nbn;
    while (s > 0 && !aae::wino_xcd_cols_valid(nbn, s)) s >>= 1;
    return s;
}

static int launch_winograd(aae_encoder* enc, const Layer& L, const float* x, int B, float* out, hipStream_t stream, Timer& tm, const char* name) {
    aae::ConvWinoArgs a;
    a.x = x; a.U = nullptr; a.bias = L.bias; a.bn_scale = L.bn_scale; a.bn_shift = L.bn_shift; a.out = out;
    a.B = B; a.H = L.H; a.W = L.W; a.Cin = L.Cin; a.Cout = L.Cout; a.Ho = L.Ho; a.Wo = L.Wo; a.relu = L.relu;
    a.eh = a.ew = 0; a.mode = 0;
    a.blocks_x = L.wino_geom == 0 ? L.Wo / 16 : 1;
    a.blocks_y = L.wino_geom == 0 ? L.Ho / 16 : 1;
    a.regions = L.wino_geom == 0 ? a.blocks_x * a.blocks_y * B : ceil_div(B, 4);
    a.xcd_cols = wino_xcd_cols(enc, L);
    const unsigned grid = aae::wino_grid_blocks(a.regions, L.Cout / 64, a.xcd_cols);
    const double tiles = (double)B * (L.Ho / 2) * (L.Wo / 2);
#ifdef AAE_EXPERIMENTS
    if (enc->winograd == 2) {
        // one launch per phase, the phases add up in the output buffer (A/B of the one-launch form: 2 % slower)
        static const int order[4][2] = {{1, 1}, {1, 0}, {0, 1}, {0, 0}};
        for (int i = 0; i < 4; ++i) {
            const int eh = order[i][0], ew = order[i][1];
            a.eh = eh; a.ew = ew; a.U = L.wino[2 * eh + ew];
            a.mode = i == 0 ? 0 : (i == 3 ? 2 : 1);
            if (!launch_wino_phase_form(L.wino_geom == 0 ? 0 : 2, eh, ew, dim3(grid), stream, a))      // (geometry 1 as four windows of their own: WinoGeom<2>)
                return fail(AAE_ERR_RUNTIME, "%s: no Winograd phase instantiation for geometry %d", name, L.wino_geom);
            const int taps = (eh ? 3 : 2) * (ew ? 3 : 2), points = ((eh ? 3 : 2) + 1) * ((ew ? 3 : 2) + 1);
            if (int rc = launch_done(tm, 2.0 * tiles * points * (double)L.Cin * (double)L.Cout, "%s:conv_wino_f32 phase %d%d (%d taps as %d products per 2x2 outputs) M=%d N=%d C=%d",
                                     name, eh, ew, taps, points, B * L.Ho * L.Wo, L.Cout, L.Cin)) return rc;
        }
        return AAE_OK;
    }
#endif
    // one launch for the layer: the four phases inside the block, output written once
    aae::ConvWinoLayerArgs p;
    p.c = a;
    for (int i = 0; i < 4; ++i) p.U4[i] = L.wino[i];
    wino_layer_launch(L.wino_geom, enc->winograd_wide, enc->winograd_stage32, grid, stream, p, enc->winograd_static_halo);
    // (the record carries the flops the kernel EXECUTES -- 49 products per 2 x 2 outputs and channel pair where the direct form
    //  multiplies 100 -- so that its TFLOP/s figure is a statement about the kernel)
    return launch_done(tm, 2.0 * tiles * 49.0 * (double)L.Cin * (double)L.Cout, "%s:conv_wino_f32 layer (25 taps as 49 products per 2x2 outputs) M=%d N=%d C=%d", name,
                       B * L.Ho * L.Wo, L.Cout, L.Cin);
}

// The round-fill rule on a block count: do `blocks` Winograd blocks fill winograd_min_fill_pct per cent of the rounds they occupy (winograd_rule has the
// measurements; winograd_min_blocks > 0 -- tests, A/B -- asks for a plain count instead)?  Each caller counts its OWN way, and the three counts stay different:
// winograd_rule and mid_group_layers (aae_multi_impl.h) count regions x Cout / 64 -- the latter only the complete regions where the ragged blocks leave the
// launch --, plan_multi's per-detection group pass counts the XCD-padded grid (wino_grid_blocks).
static bool wino_fills(const aae_encoder* enc, long long blocks) {
    if (enc->winograd_min_blocks > 0) return blocks >= enc->winograd_min_blocks;
    const long long cus = wavek_round_blocks(enc), rounds = (blocks + cus - 1) / cus;
    return 100 * blocks >= (long long)enc->winograd_min_fill_pct * rounds * cus;
}
static bool winograd_rule(const aae_encoder* enc, const Layer& L, int B);
static bool runs_winograd(const aae_encoder* enc, const Layer& L, int B) { return L.wino[0] && winograd_rule(enc, L, B); }
// would any conv layer of a batch of B take the Winograd form, were its weights there?
static bool wants_winograd_weights(const aae_encoder* enc, int B) {
    for (const Layer& L : enc->layers)
        if (L.kind == KIND_IGEMM && !L.wino[0] && winograd_rule(enc, L, B)) return true;
    return false;
}
// the Winograd-domain weights of every eligible layer: packed from the device copy of the HWIO kernel and uploaded, once (NOT from a hot call:
// it allocates and copies synchronously -- aae_encoder_workspace_bytes / aae_multi_workspace_bytes call it for batches that will use them)
static int ensure_winograd_weights(aae_encoder* enc) {
    std::lock_guard<std::mutex> lk(enc->wino_mu);
    for (Layer& L : enc->layers) {
        if (L.kind != KIND_IGEMM || L.wino_geom < 0 || L.wino[0] || !L.w_hwio) continue;
        std::vector<float> k((size_t)L.K() * L.Cout);
        AAE_HIP_TRY(hipMemcpy(k.data(), L.w_hwio, k.size() * sizeof(float), hipMemcpyDeviceToHost));
        float* dev[4] = {nullptr, nullptr, nullptr, nullptr};
        for (int eh = 0; eh < 2; ++eh)
            for (int ew = 0; ew < 2; ++ew) {
                const std::vector<float> U = pack_weights_winograd(k.data(), L.KS, L.Cin, L.Cout, eh, ew, !eh && ew);
                if (int rc = upload(enc, U.data(), U.size(), &dev[2 * eh + ew])) return rc;
            }
        for (int q = 3; q >= 0; --q) L.wino[q] = dev[q];          // (component 0 last: runs_winograd asks for it)
    }
    return AAE_OK;
}
static bool winograd_rule(const aae_encoder* enc, const Layer& L, int B) {
    if (!enc->winograd || L.wino_geom < 0 || B < enc->winograd_min_batch) return false;
    // (the kernel reads the input through a 32-bit buffer view whose upper half marks "outside the image": activations below 2 GiB)
    const unsigned long long x_bytes = (unsigned long long)B * L.H * L.W * L.Cin * sizeof(float);
    if (x_bytes >= 0x7FFFFF00ull) return false;
    // A launch costs WHOLE rounds of blocks (one block per compute unit at a time: 121-131 KB of LDS), and a block-slot of the Winograd form
    // costs 0.55-0.6 of what the direct kernels need for the same outputs (tools/wino_ab.py, profiles/r15/winograd_vs_direct_every_layer_forced.jsonl:
    // direct / Winograd = 1.65-1.85 at full rounds, 1.0 where the blocks fill half of the rounds they occupy): a layer gains when its blocks
    // fill at least winograd_min_fill_pct (56) per cent of their rounds -- default net: conv2 from B = 9, conv3 from 18, conv4 (four images
    // per block) from 69, and e.g. not conv3 at B = 33 ... 35 or conv4 at B = 129 ... 140 (a new round for a few blocks)
    return wino_fills(enc, (long long)(L.Cout / 64) * (L.wino_geom == 0 ? (long long)(L.Ho / 16) * (L.Wo / 16) * B : (long long)ceil_div(B, 4)));
}

// layer_begin / layer_end: run only the layers [layer_begin, layer_end) of the chain -- conv layers 0 ... nl - 1, the dense layer = nl; x is
// then the INPUT of layer layer_begin (fp32 activation when layer_begin > 0) and the workspace the one of a whole forward (the grouped
// mid-batch query runs conv1 and the dense layer per object around its one-launch-per-layer Winograd convolutions: aae_multi_impl.h).
static int forward_impl(aae_encoder* enc, const void* x, int x_dtype, int B, float* z_out, void* workspace,
                        size_t ws_bytes, void* stream_v, Timer& tm, const ExtraTicketPrep* extra = nullptr, bool* extra_prepared = nullptr,
                        bool* scan_done = nullptr, int layer_begin = 0, int layer_end = -1) {
    if (extra_prepared) *extra_prepared = false;
    if (scan_done) *scan_done = false;
    if (!enc || !x || !z_out) return fail(AAE_ERR_INVALID, "aae_encoder_forward: null argument");
    if (B < 1) return fail(AAE_ERR_INVALID, "aae_encoder_forward: batch %d < 1", B);
    if (x_dtype != AAE_DTYPE_U8 && x_dtype != AAE_DTYPE_F32)
        return fail(AAE_ERR_INVALID, "aae_encoder_forward: x_dtype %d (want AAE_DTYPE_U8 or AAE_DTYPE_F32)", x_dtype);
    const Workspace ws = plan_workspace(enc, B);
    if (ws_bytes < ws.total) return fail(AAE_ERR_WORKSPACE, "workspace %zu B < required %zu B for batch %d", ws_bytes, ws.total, B);
    if (!workspace || ((uintptr_t)workspace & 255)) return fail(AAE_ERR_WORKSPACE, "workspace must be non-null and 256-B aligned");
    hipStream_t stream = static_cast<hipStream_t>(stream_v);
    unsigned char* base = static_cast<unsigned char*>(workspace);
    float* partial = reinterpret_cast<float*>(base + ws.partial_off);
    unsigned long long* tickets = reinterpret_cast<unsigned long long*>(base + ws.ticket_off);
    unsigned long long* gemv_tickets = tickets + kConvTicketBytes / 8;
    auto layer_tickets = [&](size_t li) { return tickets + li * kLayerTicketWords; };     // li == layers.size(): the dense layer
    RecordScope rec(enc);
    tm.stream = stream;
    if (int rc = tm.mark()) return rc;

    const void* cur = x;
    bool cur_u8 = (x_dtype == AAE_DTYPE_U8);
    t_x3h_last_slot = -1;
    const bool ranged = layer_begin != 0 || layer_end >= 0;
    if (layer_end < 0) layer_end = (int)enc->layers.size() + 1;
    if (ranged && (layer_begin < 0 || layer_begin >= layer_end || layer_end > (int)enc->layers.size() + 1 || runs_split(enc, B) || (layer_begin > 0 && cur_u8)))
        return fail(AAE_ERR_INVALID, "aae_encoder_forward: layer range [%d, %d) of a %zu-layer encoder", layer_begin, layer_end, enc->layers.size() + 1);
    if (runs_split(enc, B)) {
        // this forward's range flag: a ring slot, or -- while the stream is being captured into a graph -- a slot of its own
        hipStreamCaptureStatus capture = hipStreamCaptureStatusNone;
        (void)hipStreamIsCapturing(stream, &capture);
        int slot;
        if (capture != hipStreamCaptureStatusNone) {
            std::lock_guard<std::mutex> lk(enc->x3h_mu);
            slot = -1;
            for (size_t f = 0; f < enc->x3h_free.size(); ++f) {          // a released slot whose flag clear has executed (aae_encoder_x3h_release_slot)
                const size_t k = (size_t)(enc->x3h_free[f] - kX3hRing);
                if (k < enc->x3h_release_ev.size() && enc->x3h_release_ev[k] && hipEventQuery(enc->x3h_release_ev[k]) != hipSuccess) continue;
                slot = enc->x3h_free[f];
                enc->x3h_free.erase(enc->x3h_free.begin() + (long)f);
                break;
            }
            if (slot < 0) {
                if (enc->x3h_captured >= kX3hCaptured)         // (nothing is consumed by the failing call)
                    return fail(AAE_ERR_UNSUPPORTED, "more than %d f32x3h forwards live in HIP graphs on one encoder handle (aae_encoder_x3h_release_slot returns a destroyed graph's slot)", kX3hCaptured);
                slot = kX3hRing + enc->x3h_captured++;
            }
        } else {
            slot = (int)(enc->x3h_seq.fetch_add(1, std::memory_order_relaxed) % kX3hRing);
        }
        t_x3h_flag = enc->x3h_sat + slot;
        t_x3h_last_slot = slot;
        // f32x3h: conv1 (fp32 MFMA, K = 75) emits fp16 hi/lo planes, every later layer runs the
        // split-precision igemm on planes; only the latent z comes back as fp32.
        for (size_t li = 0; li < enc->layers.size(); ++li) {
            const Layer& L = enc->layers[li];
            float* out = reinterpret_cast<float*>(base + ws.act_off[li]);
            char name[16];
            snprintf(name, sizeof(name), "conv%zu", li + 1);
            int rc;
            if (li == 0) rc = launch_first(enc, L, cur, cur_u8, B, out, true, stream, tm);
            else rc = launch_igemm_x3h(enc, L, cur, B * L.Ho * L.Wo, out, false, partial, stream, tm, name, (int)li);
            if (rc) return rc;
            cur = out;
        }
        return launch_igemm_x3h(enc, enc->dense, cur, B, z_out, true, partial, stream, tm, "dense");
    }

    // ---- plan every layer first: the ticketed launches get their nonces now, so that the first kernel can install them
    const size_t nl = enc->layers.size();
    const Layer& D = enc->dense;
    std::vector<WaveKPlan> plans(nl + 1);
    std::vector<unsigned> nonces(nl + 1, 0u);
    for (size_t li = 0; li < nl; ++li) {
        const Layer& L = enc->layers[li];
        const bool first_mfma = li == 0 && L.kind == KIND_FIRST_MFMA;
        if (!first_mfma && L.kind == KIND_IGEMM && !(li == 0 && cur_u8) && !runs_winograd(enc, L, B)) plans[li] = plan_wavek(enc, L, (long long)B * L.Ho * L.Wo, false);
    }
#ifdef AAE_EXPERIMENTS
    const bool dense_gemv = D.kind == KIND_IGEMM && B <= gemv_max_batch(enc) && enc->dense_gemv && D.K() % aae::kGemvChunk == 0;
#else
    // (the GEMV whose chunk rows a second launch adds up -- latent sizes that are no multiple of 4 or beyond 1024, option
    //  gemv_ticket = 0 -- lives in the experiments build; here such a dense layer takes the wave-split-K / split-K matrix path)
    const bool dense_gemv = D.kind == KIND_IGEMM && B <= gemv_max_batch(enc) && enc->dense_gemv && D.K() % aae::kGemvChunk == 0 && gemv_uses_ticket(enc, D);
#endif
    const bool gemv_ticket = dense_gemv && gemv_uses_ticket(enc, D);
    if (!dense_gemv && D.kind == KIND_IGEMM && enc->wavek_dense) plans[nl] = plan_wavek(enc, D, B, false);
    aae::TicketPrep prep;
    prep.n = 0;
    auto add_prep = [&](unsigned long long* words, int count, unsigned nonce) {
        if (prep.n >= aae::kMaxTicketPrep) return false;
        prep.words[prep.n] = words; prep.count[prep.n] = count; prep.nonce[prep.n] = nonce; ++prep.n;
        return true;
    };
    for (size_t li = 0; li <= nl; ++li)
        if (plans[li].use && (plans[li].gsplits > 1 || plans[li].tail_tiles > 0)) {
            nonces[li] = next_nonce();
            add_prep(layer_tickets(li), plans[li].tail_tiles > 0 ? plans[li].tail_tiles : plans[li].num_mt * plans[li].num_nt, nonces[li]);
        }
    unsigned gemv_nonce = 0;
    if (gemv_ticket) {
        gemv_nonce = next_nonce();
        add_prep(gemv_tickets, (D.CoutPad / 128) * aae::kTicketSlotWords, gemv_nonce);
    }
    const bool extra_listed = extra && extra->words && add_prep(extra->words, extra->count, extra->nonce);
    // the persistent per-detection launch: its grid-barrier words count monotonically inside a launch and must start from
    // (nonce, 0) -- also when a captured graph replays the launch with the SAME nonce.  The first kernel resets them with the
    // other ticket words; where it cannot, a memset in front of the launch does.
#ifdef AAE_EXPERIMENTS
    const bool chain = !ranged && chain_eligible(enc, B, plans, gemv_ticket);
    unsigned long long* barrier_words = tickets + (kConvTicketBytes + kGemvTicketBytes) / 8;
    const unsigned barrier_nonce = chain ? next_nonce() : 0u;
    const bool barrier_listed = chain && add_prep(barrier_words, aae::kGridBarrierWords, barrier_nonce);
#endif
    const bool can_prepare = enc->ticket_prep && enc->layers[0].kind == KIND_FIRST_MFMA && prep.n > 0;
    if (extra_prepared) *extra_prepared = can_prepare && extra_listed;

#ifdef AAE_EXPERIMENTS
    // ---- per-detection batches: the first layer as its own launch, everything behind it in ONE persistent launch
    if (chain) {
        const Layer& L0 = enc->layers[0];
        float* out0 = reinterpret_cast<float*>(base + ws.act_off[0]);
        int rc;
        if (L0.kind == KIND_FIRST_MFMA) rc = launch_first(enc, L0, cur, cur_u8, B, out0, false, stream, tm, can_prepare ? &prep : nullptr);
        else if (L0.kind == KIND_IGEMM && !cur_u8) {
            if (plans[0].use)
                rc = launch_wavek(enc, L0, plans[0], static_cast<const float*>(cur), B * L0.Ho * L0.Wo, out0, partial, layer_tickets(0), nonces[0],
                                  stream, tm, "conv1", 0);
            else rc = launch_igemm(enc, L0, static_cast<const float*>(cur), B * L0.Ho * L0.Wo, out0, partial, stream, tm, "conv1", 0);
        } else rc = launch_generic(enc, L0, cur, cur_u8, B, out0, stream, tm, "conv1");
        if (rc) return rc;
        if (!(can_prepare && barrier_listed)) AAE_HIP_TRY(hipMemsetAsync(barrier_words, 0, (size_t)aae::kGridBarrierWords * 8, stream));
        rc = launch_detect_chain(enc, B, plans, nonces, gemv_nonce, barrier_nonce, out0, base, ws, tickets, z_out, extra, stream, tm);
        if (rc == AAE_OK && scan_done) *scan_done = extra && extra->scan_ready;
        return rc;
    }
#endif

    for (size_t li = (size_t)layer_begin; li < nl && (int)li < layer_end; ++li) {
        const Layer& L = enc->layers[li];
        float* out = reinterpret_cast<float*>(base + ws.act_off[li]);
        char name[16];
        snprintf(name, sizeof(name), "conv%zu", li + 1);
        int rc;
        if (li == 0 && L.kind == KIND_FIRST_MFMA) rc = launch_first(enc, L, cur, cur_u8, B, out, false, stream, tm, can_prepare ? &prep : nullptr);
        else if (L.kind == KIND_IGEMM && !cur_u8) {
            if (runs_winograd(enc, L, B)) rc = launch_winograd(enc, L, static_cast<const float*>(cur), B, out, stream, tm, name);
            else if (plans[li].use)
                rc = launch_wavek(enc, L, plans[li], static_cast<const float*>(cur), B * L.Ho * L.Wo, out, partial, layer_tickets(li), nonces[li],
                                  stream, tm, name, (int)li);
            else rc = launch_igemm(enc, L, static_cast<const float*>(cur), B * L.Ho * L.Wo, out, partial, stream, tm, name, (int)li);
        } else rc = launch_generic(enc, L, cur, cur_u8, B, out, stream, tm, name);
        if (rc) return rc;
        cur = out;
        cur_u8 = false;
    }
    if (layer_end <= (int)nl) return AAE_OK;
    if (dense_gemv)
        return launch_dense_gemv(enc, D, static_cast<const float*>(cur), B, z_out, partial, gemv_ticket ? gemv_tickets : nullptr, gemv_nonce, stream, tm);
    if (plans[nl].use)
        return launch_wavek(enc, D, plans[nl], static_cast<const float*>(cur), B, z_out, partial, layer_tickets(nl), nonces[nl], stream, tm, "dense", 0);
    if (D.kind == KIND_IGEMM) return launch_igemm(enc, D, static_cast<const float*>(cur), B, z_out, partial, stream, tm, "dense");
    return launch_generic(enc, D, cur, false, B, z_out, stream, tm, "dense");
}


}  // namespace aae_host
