/* aae_hip.h -- C ABI of libaae_hip.so: the MI355X (gfx950) implementation of the
 * AugmentedAutoencoder orientation-inference hot path.
 *
 * The reference has no FFI for this path: its boundary is a Python class API
 * whose back end is tf.Session.run.  Each entry point below
 * names the reference interface it replaces (paths relative to /root/reference).
 * INTEGRATION.md shows the ctypes binding a maintainer would add.
 *
 * Conventions
 *   - plain C types only; device buffers are raw device pointers owned by the
 *     caller (e.g. torch tensors); `stream` is a hipStream_t passed as void*.
 *   - every call returns AAE_OK (0) or a negative error code; the message for
 *     the calling thread is available from aae_last_error().  Nothing exits
 *     the process (the reference print()+exit(-1)s on fatal errors).
 *   - handles own their device weights / codebook and are immutable after
 *     creation (aae_codebook_update excepted); concurrent calls on distinct
 *     streams with distinct workspaces are allowed.  No allocation happens
 *     inside forward / nn / similarity: scratch comes from the caller-provided
 *     workspace sized by the *_workspace_bytes queries.
 */
#ifndef AAE_HIP_H_
#define AAE_HIP_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define AAE_ABI_VERSION 3

#define AAE_OK 0
#define AAE_ERR_INVALID (-1)      /* bad argument                                  */
#define AAE_ERR_UNSUPPORTED (-2)  /* shape / dtype outside what the kernels cover  */
#define AAE_ERR_RUNTIME (-3)      /* HIP runtime error (message has the detail)    */
#define AAE_ERR_WORKSPACE (-4)    /* workspace too small / misaligned              */

#define AAE_DTYPE_U8 0            /* uint8 crops: converted as float32(v/255.)     */
#define AAE_DTYPE_F32 1
#define AAE_DTYPE_BF16 2          /* codebook storage only: bfloat16 rows (2 B/elem), J == 128 */

#define AAE_MAX_LAYERS 8

#define AAE_SCAN_AUTO 0           /* B <= 4, top-1 / top-2..8: streaming kernel that answers inside its launch; B > 4, top-1 /
                                    * top-2..8, stride 1: query-resident MFMA kernel; else the tile-resident MFMA kernels    */
#define AAE_SCAN_AUTO_PACKED 7    /* AUTO, but the top-1 query-resident scan (B > 4) reads queries normalised and packed by a
                                     launch in front instead of normalising the raw codes in its own prologue: A/B, same answers
                                     (the other A/B modes: include/aae_hip_tuning.h) */

typedef struct aae_encoder aae_encoder;
typedef struct aae_codebook aae_codebook;
typedef struct aae_decoder aae_decoder;

/* Shapes of Encoder(input, latent_space_size, num_filters, kernel_size, strides,
 * batch_norm)  -- auto_pose/ae/encoder.py:14, filled from the [Network]/[Dataset]
 * cfg keys exactly as ae_factory.build_encoder does (auto_pose/ae/ae_factory.py:33-48). */
typedef struct aae_encoder_desc {
    int32_t in_h, in_w, in_c;             /* [Dataset] H, W, C                      */
    int32_t num_layers;
    int32_t num_filters[AAE_MAX_LAYERS];  /* [Network] NUM_FILTER                   */
    int32_t strides[AAE_MAX_LAYERS];      /* [Network] STRIDES                      */
    int32_t kernel_size;                  /* [Network] KERNEL_SIZE_ENCODER          */
    int32_t latent_size;                  /* [Network] LATENT_SPACE_SIZE            */
    int32_t batch_norm;                   /* [Network] BATCH_NORMALIZATION (0/1)    */
    float bn_eps;                         /* tf.layers.batch_normalization eps 1e-3 */
} aae_encoder_desc;

int aae_abi_version(void);
/* 1 in the experiments build (-DAAE_EXPERIMENTS: every kernel variant that measured slower than the defaults, the profiling and
 * ablation aids -- tools/ and the A/B tests), 0 in the product library (include/aae_hip_tuning.h lists what lives where) */
int aae_has_experiments(void);
const char* aae_last_error(void);

/* ---- Encoder: auto_pose/ae/encoder.py:37-68 (encoder_out + z) -----------------
 * host_weights (float32, host memory), in TF variable order:
 *   per conv layer i : kernel HWIO [k,k,Cin,Cout], bias [Cout]
 *                      (+ gamma, beta, moving_mean, moving_variance [Cout] if batch_norm)
 *   then             : dense kernel [Ho*Wo*C_last, latent], dense bias [latent]
 * Replaces graph construction + factory.restore_checkpoint (ae_factory.py:149-172). */
int aae_encoder_create(const aae_encoder_desc* desc, const void* const* host_weights, int n_weights,
                       aae_encoder** out);
void aae_encoder_destroy(aae_encoder* enc);

/* Options (set before sizing the workspace).  The ones a caller may want:
 *   "precision" (0): 0 = exact fp32 matrix-core arithmetic (bitwise an fp32 fma chain);
 *                    1 = "f32x3h": fp32 in/out, every product of conv2..dense evaluated as three fp16 MFMAs on (hi, lo) operand
 *                        pairs with fp32 accumulation (>= 22-bit operands).  Explicit opt-in; same parity tolerances; activations
 *                        then live in the workspace as fp16 (hi, lo) pairs of x * 2^x3h_act_shift, interleaved per 32-channel chunk.
 *                    2 = f32x3h where it is faster: batches whose first implicit-GEMM layer has at least 256 64x64 output tiles
 *                        (B >= 4 of the default net) run as 1, smaller ones as 0 -- per-detection batches are faster AND exact on
 *                        the fp32 wave-split-K path.
 *   "x3h_act_shift" (4): power-of-two activation pre-scale of the f32x3h format (|x| < 4094 keeps full accuracy; larger values
 *                        saturate gracefully up to 2x and raise the range flag, aae_encoder_x3h_poll).
 *   "compact_workspace" (0): two alternating activation buffers instead of one per layer (805 instead of 973 MB at B = 256; layer
 *                        outputs are then not inspectable through aae_encoder_activation_info).
 *   "dense_gemv" (1): batches of <= 8 run the dense layer as a weight-streaming GEMV instead of a padded matrix-core tile
 *                        (same value up to fp32 summation order).
 *   "multi_group_plan" (1): aae_encode_nn_multi -- a group of objects runs ONE launch plan chosen for the group's total tile count
 *                        (answers differ from per-object aae_encode_nn calls by fp32 summation order only); 0 = every object its
 *                        own plan: bit-identical to aae_encode_nn.
 * Everything else the call accepts -- the planner's constants, kernel-variant switches for A/B measurements -- is listed in
 * include/aae_hip_tuning.h.  In this (product) build every accepted value gives results that are bit-identical to the defaults
 * or differ by fp32 rounding / summation order only; variants that measured slower and the profiling aids live in the experiments build
 * (aae_has_experiments()) and are refused here with AAE_ERR_UNSUPPORTED. */
int aae_encoder_set_option(aae_encoder* enc, const char* name, int value);

size_t aae_encoder_workspace_bytes(const aae_encoder* enc, int B);

/* z = Encoder.z for a batch of crops; replaces session.run(encoder.z, {encoder.x: x})
 * (auto_pose/ae/codebook.py:145,206) and the x/255. of codebook.py:58-59.
 * x: device [B,H,W,C] NHWC (BGR), uint8 or float32.  z_out: device [B, latent] float32. */
int aae_encoder_forward(aae_encoder* enc, const void* x, int x_dtype, int B, float* z_out,
                        void* workspace, size_t ws_bytes, void* stream);

/* Same, with HIP events around every kernel launch on `stream` (synchronises the
 * stream).  kernel_ms[i] receives the duration of launch i; returns the launch
 * count through n_kernels.  Labels / algorithmic FLOPs of launch i for this B
 * come from the two queries below (valid after any forward with the same B). */
int aae_encoder_forward_timed(aae_encoder* enc, const void* x, int x_dtype, int B, float* z_out,
                              void* workspace, size_t ws_bytes, void* stream,
                              float* kernel_ms, int max_kernels, int* n_kernels);
const char* aae_encoder_kernel_label(const aae_encoder* enc, int i);
double aae_encoder_kernel_flops(const aae_encoder* enc, int i);

/* Byte offset / element count of layer `layer`'s activation [B,Ho,Wo,Cout] inside the
 * workspace after a forward with batch B (parity tests of encoder.py:41-54 per layer). */
/* f32x3h range check ("precision" = 1 only).  Activations travel between layers as fp16 (hi, lo) pairs of
 * x * 2^x3h_act_shift; a pair carries |x * 2^shift| < 65504 (default shift 4: |x| < 4094) at full accuracy.  Every
 * kernel that writes pairs raises a sticky device flag when a value falls outside; this call waits for `stream`,
 * returns the flag and clears it.  1 = the latents of the forwards since the last call may be inaccurate: recompute them
 * with "precision" = 0 (the Python mirror does that automatically).  Exact fp32 mode never sets the flag. */
int aae_encoder_x3h_saturated(aae_encoder* enc, int* flag_out, void* stream);

/* The same check without a wait per forward.  Every f32x3h forward raises its OWN flag: one of 256 slots taken round-robin
 * (a forward recorded into a HIP graph gets one of 64 slots that are never reused -- the graph bakes the address).
 * aae_encoder_x3h_last_slot(): slot of the most recent forward / aae_encode_nn issued by the calling thread, -1 when that
 * forward ran in exact fp32.  aae_encoder_x3h_poll(): waits for `stream` ONCE, returns the flags of `n` slots (1 = that
 * forward met an out-of-range activation: recompute it with "precision" = 0) and clears the raised ones.  A caller can so
 * queue any number of forwards without a host round trip and check them when it consumes the results (the Python mirror:
 * EncoderEngine.settle()).  With more than 256 un-polled forwards a slot is shared: a raised flag may then belong to either
 * user -- a spurious fp32 recomputation at worst, never a missed one.  aae_encoder_x3h_saturated() reports and clears all
 * slots at once. */
int aae_encoder_x3h_last_slot(void);
int aae_encoder_x3h_poll(aae_encoder* enc, const int* slots, int n, int* flags_out, void* stream);
/* A forward recorded into a HIP graph owns its slot (one of 64) until the owner of the graph gives it back: call this when
 * the graph is destroyed (the Python mirror: CapturedNearestNeighbour.close()).  Slots of eager forwards need no release. */
int aae_encoder_x3h_release_slot(aae_encoder* enc, int slot, void* stream);   /* the flag is reset asynchronously on `stream` */

/* 1 when a forward of batch B on this handle runs in f32x3h (precision 1, or precision 2 and a large enough batch):
 * the layer outputs in the workspace are then fp16 (hi, lo) pairs instead of fp32 (aae_encoder_activation_info). */
int aae_encoder_split_precision_for_batch(const aae_encoder* enc, int B);

int aae_encoder_activation_info(const aae_encoder* enc, int B, int layer, size_t* offset_bytes,
                                size_t* count);

/* ---- Codebook: auto_pose/ae/codebook.py:18-51 ---------------------------------
 * E: [N, J] rows already normalised (embedding_normalized variable, codebook.py:28-36, as left
 * by update_embedding :214-216); float32 (AAE_DTYPE_F32, the reference's storage) or bfloat16
 * bit patterns (AAE_DTYPE_BF16, J == 128: half the HBM bytes per scan; queries keep fp32
 * accuracy as three bf16 terms).  Host or device source. */
int aae_codebook_create(const void* E, int N, int J, int dtype, int src_is_device, aae_codebook** out);
int aae_codebook_update(aae_codebook* cb, const void* E, int src_is_device, void* stream);  /* embedding_assign_op */
void aae_codebook_destroy(aae_codebook* cb);
int aae_codebook_set_scan_mode(aae_codebook* cb, int mode);     /* AAE_SCAN_AUTO (default) | AAE_SCAN_AUTO_PACKED | the A/B modes of aae_hip_tuning.h */
/* Upright search (codebook.py:65-66: arg-max over columns 0, k, 2k, ... of the similarity, k = num_cyclo): builds /
 * refreshes a compacted device copy of every col_stride-th row, so that aae_codebook_nn(col_stride = k) scans N/k
 * rows instead of masking a full scan (same scores, same tie rule).  Allocates; call it once outside timed /
 * graph-captured regions.  aae_codebook_update keeps the copy in step.  Without it nn falls back to the masked scan. */
int aae_codebook_prepare_upright(aae_codebook* cb, int col_stride, void* stream);

size_t aae_codebook_workspace_bytes(const aae_codebook* cb, int B, int topk);

/* Nearest rotation indices for un-normalised latents z [B,J] (device):
 * l2_normalize (codebook.py:27) -> matmul transpose_b (:50) -> argmax (:64-68) or
 * top-n (:69-71).  col_stride = 1, or num_cyclo for `upright` (:66; only with topk 1).
 * idx_out: device int64 [B, topk]; score_out: device float32 [B, topk] (cosine).
 * Ties resolve to the lowest index (np.argmax); top-k is score-descending,
 * index-ascending among equal scores.  topk 2..8 is computed inside the scan: B <= 4 (the
 * reference's one-crop-per-call top-n) in ONE launch -- every block of the streaming kernel
 * leaves a sorted list per query and the last block to arrive merges them; B > 4 on the
 * query-resident kernel (sorted per-lane lists) + a merge launch.  topk > 8 materialises the
 * [B,N] similarity in the workspace first -- aae_codebook_workspace_bytes(cb, B, topk)
 * accounts for either. */
int aae_codebook_nn(aae_codebook* cb, const float* z, int B, int topk, int col_stride,
                    int64_t* idx_out, float* score_out, void* workspace, size_t ws_bytes, void* stream);

/* Kernel launches the calling thread's last aae_codebook_nn call queued; after aae_encode_nn / aae_encode_nn_topk: the launches
 * of that call's codebook stage.  Thread-local, like aae_multi_last_launches. */
int aae_codebook_last_launches(void);

/* The same query `reps` times back to back, queued from C between two HIP events on `stream`: *period_ms = device time per
 * query = its kernel(s) + the dependent-launch gap, without the caller's per-call host cost (a Python loop spends longer per
 * call than the 12 us kernel of the B = 1 query takes).  bench.py's `scan.kernel_period_us`, measured in the run that
 * reports it.  (One call between two events on an idle stream measures the events' own latency more than the kernel.)
 * Waits for the second event. */
int aae_codebook_nn_timed(aae_codebook* cb, const float* z, int B, int topk, int col_stride,
                          int64_t* idx_out, float* score_out, void* workspace, size_t ws_bytes, void* stream, int reps, float* period_ms);

/* aae_encoder_forward followed by aae_codebook_nn(topk = 1) on `stream` in ONE call: what
 * Codebook.nearest_rotation(session, x) does per detection (auto_pose/ae/codebook.py:55-68,
 * m3_interface/ae_pose_estimator.py:143-170).  Same results as the two calls, bit for bit.  For B <= 4 the query is
 * six launches: the encoder's first kernel prepares the ticket words of the later launches (wave-split-K tiles, dense
 * GEMV chunks, scan block partials), each of which then finishes its own reduction ("last block to arrive").
 * z_out: device [B, latent] (also returned: Encoder.z).  Workspaces as for the two separate calls. */
int aae_encode_nn(aae_encoder* enc, aae_codebook* cb, const void* x, int x_dtype, int B, int col_stride, float* z_out,
                  int64_t* idx_out, float* score_out, void* enc_workspace, size_t enc_ws_bytes, void* cb_workspace,
                  size_t cb_ws_bytes, void* stream);

/* aae_encode_nn with a top-k scan (col_stride 1): aae_encoder_forward followed by aae_codebook_nn(topk) in ONE call -- what
 * Codebook.nearest_rotation(session, x, top_n) does for its single crop (auto_pose/ae/codebook.py:55-71, eval/ae_eval.py:173-201).
 * Same results as the two calls, bit for bit.  B <= 4, topk 2..8: still six launches, the scan's ticket words prepared by the
 * encoder's first kernel; otherwise the two calls back to back.  idx_out / score_out: device [B, topk].
 * cb_workspace: aae_codebook_workspace_bytes(cb, B, topk). */
int aae_encode_nn_topk(aae_encoder* enc, aae_codebook* cb, const void* x, int x_dtype, int B, int topk, float* z_out,
                       int64_t* idx_out, float* score_out, void* enc_workspace, size_t enc_ws_bytes, void* cb_workspace,
                       size_t cb_ws_bytes, void* stream);

/* Full cosine-similarity matrix cs_out [B,N] (device) = session.run(cos_similarity)
 * (codebook.py:63); parity / debugging path, the nn call never materialises it for topk 1. */
int aae_codebook_similarity(aae_codebook* cb, const float* z, int B, float* cs_out,
                            void* workspace, size_t ws_bytes, void* stream);

/* normalized_embedding_query (codebook.py:27) for test_embedding(normalized=True) (:135-145). */
int aae_l2_normalize(const float* z, int B, int J, float* q_out, void* stream);

/* Multi-GPU gather payload (object-sharded inference, one process per GPU): row pos[i] (pos == NULL: row i) of the
 * fixed-capacity buffer packed[capacity][2] receives (idx[i*stride], float bits of score[i*stride]).  One launch
 * instead of four framework element-wise ops in the step that ends in the RCCL all_gather; rows that belong to other
 * ranks keep the -1 sentinel.  Replaces the per-detection bookkeeping of m3_interface/ae_pose_estimator.py:143-170. */
int aae_pack_pairs(const int64_t* idx, const float* score, const int32_t* pos, int n, int stride, int64_t* packed,
                   void* stream);

/* The way back after the all_gather: gathered[world * rows_per_rank][2] holds every rank's packed buffer; answer i of the
 * batch (i < n <= rows_per_rank) is row i of block owner[i] (owner == NULL: block 0).  Writes idx_out[i] (int64) and
 * score_out[i] (float32) in one launch (replaces a fancy-index gather + two element-wise conversions per step). */
int aae_unpack_pairs(const int64_t* gathered, const int32_t* owner, int n, int rows_per_rank, int64_t* idx_out, float* score_out,
                     void* stream);

/* ---- Caller side ("next" row N1): detector crops for a whole image in one launch -------------
 * AePoseEstimator.extract_square_patch(black_borders=True) + cv2.resize(INTER_LINEAR)
 * (auto_pose/m3_interface/ae_pose_estimator.py:106-131,157-162).
 * img: device uint8 [H,W,C]; boxes: device int32 [D,5] = x, y, w, h, size with
 * size = int(max(h, w) * pad_factor); out: device uint8 [D,out_h,out_w,C]. */
int aae_crop_resize_u8(const void* img, int H, int W, int C, const int32_t* boxes, int D,
                       int out_h, int out_w, void* out, void* stream);

/* All detections of ONE object class of a frame in one call: aae_crop_resize_u8 into `crops` (device scratch
 * [n, in_h, in_w, in_c] uint8, the encoder's input shape) followed by aae_encode_nn on them -- what
 * AePoseEstimator.process does per detected box (m3_interface/ae_pose_estimator.py:143-170: extract_square_patch,
 * cv2.resize, one session.run, np.argmax), for n boxes, without a host round trip per launch.  img / boxes / idx_out /
 * score_out may be device memory or device-accessible pinned host memory (a result written straight into pinned memory
 * needs no copy back, an image read from it no upload).  Same results as the two calls. */
int aae_detect_nn(aae_encoder* enc, aae_codebook* cb, const void* img, int H, int W, int C, const int32_t* boxes, int n,
                  int col_stride, void* crops, float* z_out, int64_t* idx_out, float* score_out,
                  void* enc_workspace, size_t enc_ws_bytes, void* cb_workspace, size_t cb_ws_bytes, void* stream);

/* ---- A frame's detections of SEVERAL objects in one call: one launch per LAYER across the objects ---------------------------
 * The reference keeps one AAE (encoder weights + codebook) per object class in one process -- 30 for T-LESS
 * (auto_pose/cfg_m3vision/m3_config_tless.cfg:10-39, m3_interface/ae_pose_estimator.py:61-78) -- and runs one session.run per
 * detected box (:143-170), whatever class it belongs to.  An item = (that class's encoder, its codebook, the n boxes of the
 * class in this frame, col_stride as in aae_codebook_nn).  Inputs and outputs are concatenated in item order: x / crops
 * [rows,H,W,C], z_out [rows,latent], idx_out [rows] int64, score_out [rows], rows = sum of n (aae_multi_rows).
 * Items with n <= 4 whose per-object call would run the per-detection chain (fp32, default options, fp32 codebook, stride 1
 * or a prepared upright copy) are GROUPED: conv1, every later conv layer, the dense GEMV and the codebook scan each run as ONE
 * launch over all grouped items -- objects with different n included -- every block the per-object launch's block, tickets per
 * (object, tile): a frame with C classes costs 6 launches instead of 6 C; a conv layer whose blocks fill the chip over ALL
 * grouped objects (conv2 from ~9 boxes per frame) runs as one polyphase-Winograd launch instead ("multi_group_winograd").
 * Items with n >= 5 whose conv layers are all eligible for polyphase Winograd (default options) form MID-BATCH groups: one Winograd
 * launch per conv layer across the objects for every layer the group's blocks fill the chip on (eight buckets of ~32 crops fill it
 * like one batch of 256; four classes with six boxes each fill conv2 and conv3 -- the other layers run per object), conv1 and the
 * dense layer likewise, the codebook scans in one launch per row-part count + one reduce launch;
 * where the incomplete four-image blocks of an 8 x 8-output layer would open one more round of blocks, the last n mod 4 images
 * of every object are computed by one grouped launch of the direct kernel ("multi_mid_ragged").
 * A class with a few boxes beyond four (5 ... 8; up to 12 for a frame's only such class) is answered as items of <= 4 boxes inside the
 * per-detection group ("multi_split_items").  All other items are answered by aae_encode_nn inside the same call.
 * Results against one aae_encode_nn call per item: with the defaults a group runs ONE launch plan chosen for the group
 * ("multi_group_plan" = 1) resp. the Winograd form where the object alone would take the direct kernels, so latents differ by
 * fp32 summation order / the two forms' rounding (tests bound it at 5e-6 of the latent scale, measured <= 2.3e-6; indices equal
 * wherever the top-2 cosine gap exceeds that), as a batch of another size does; every answer is checked against the object's own fp64 oracle.  With encoder
 * options "multi_group_plan" = 0 and "multi_mid_group" = 0 the call is bit-identical to the per-object calls.
 * All encoders must share the crop shape and the latent size.  The workspace (aae_multi_workspace_bytes; scan_only = 1 for
 * aae_codebook_nn_multi) holds a slice per grouped item: nothing in it outlives the call. */
typedef struct aae_multi_item {
    aae_encoder* enc;        /* may be NULL for aae_codebook_nn_multi */
    aae_codebook* cb;
    int32_t n;               /* detections of this object (>= 1) */
    int32_t col_stride;      /* 1, or num_cyclo for the upright search */
} aae_multi_item;

size_t aae_multi_workspace_bytes(const aae_multi_item* items, int n_items, int scan_only);
int aae_multi_rows(const aae_multi_item* items, int n_items);
int aae_encode_nn_multi(const aae_multi_item* items, int n_items, const void* x, int x_dtype, float* z_out, int64_t* idx_out,
                        float* score_out, void* workspace, size_t ws_bytes, void* stream);
/* the codebook stage alone: z [rows,J] raw latent codes in item order; grouped items: ONE scan launch over their codebooks */
int aae_codebook_nn_multi(const aae_multi_item* items, int n_items, const float* z, int64_t* idx_out, float* score_out,
                          void* workspace, size_t ws_bytes, void* stream);
/* aae_crop_resize_u8 of all boxes (device or pinned int32 [rows,5], item order) into `crops` (device scratch [rows,H,W,C] uint8)
 * + aae_encode_nn_multi: all launches of a frame in ONE call (what AePoseEstimator.process does box by box). */
int aae_detect_nn_multi(const aae_multi_item* items, int n_items, const void* img, int H, int W, int C, const int32_t* boxes,
                        void* crops, float* z_out, int64_t* idx_out, float* score_out, void* workspace, size_t ws_bytes, void* stream);
/* kernel launches the grouped part of the calling thread's last multi call queued (diagnostics / bench) */
int aae_multi_last_launches(void);

/* ---- Decoder ("next" row N4): auto_pose/ae/decoder.py:36-84 (Decoder.x), inference only ---------
 * Decoder(reconstruction_target, latent_code, num_filters, kernel_size, strides, ...) as
 * ae_factory.build_decoder fills it (auto_pose/ae/ae_factory.py:50-70): num_filters / strides
 * are the REVERSED [Network] NUM_FILTER / STRIDES.
 *   dense(latent -> h0*w0*F0, relu)[+BN] -> reshape [h0,w0,F0]
 *   for F_i, size_i: resize_nearest_neighbor(size_i) -> conv2d(F_i, k, 'same', relu)[+BN]
 *   resize_nearest_neighbor([H,W]) -> conv2d(C, k, 'same', sigmoid)
 * with size_i = [H / prod(strides[i:]), W / prod(strides[i:])] (decoder.py:41).
 * host_weights (float32, host), TF variable order:
 *   dense kernel [latent, h0*w0*F0], bias (+ gamma, beta, moving_mean, moving_variance if BN)
 *   per hidden conv i = 1..L-1: kernel HWIO [k,k,F_{i-1},F_i], bias (+ 4 BN arrays)
 *   output conv: kernel [k,k,F_{L-1},C], bias.
 * The auxiliary mask head (decoder.py:66-73) does not feed Decoder.x and is not evaluated. */
typedef struct aae_decoder_desc {
    int32_t out_h, out_w, out_c;          /* reconstruction target shape = [Dataset] H, W, C */
    int32_t num_layers;                   /* len(NUM_FILTER)                                 */
    int32_t num_filters[AAE_MAX_LAYERS];  /* reversed [Network] NUM_FILTER                   */
    int32_t strides[AAE_MAX_LAYERS];      /* reversed [Network] STRIDES                      */
    int32_t kernel_size;                  /* [Network] KERNEL_SIZE_DECODER                   */
    int32_t latent_size;
    int32_t batch_norm;
    float bn_eps;
} aae_decoder_desc;

int aae_decoder_create(const aae_decoder_desc* desc, const void* const* host_weights, int n_weights,
                       aae_decoder** out);
void aae_decoder_destroy(aae_decoder* dec);
size_t aae_decoder_workspace_bytes(const aae_decoder* dec, int B);

/* x = Decoder.x for a batch of latent codes; replaces session.run(decoder.x, {encoder.x: ...})
 * after the encoder (auto_pose/eval/eval_plots.py:33,59) and
 * session.run(decoder.x, {decoder._latent_code: z}) (eval_plots.py:78).
 * z: device [B, latent] float32 (NOT normalised).  x_out: device [B,H,W,C] float32 in [0,1]. */
int aae_decoder_forward(aae_decoder* dec, const float* z, int B, float* x_out, void* workspace,
                        size_t ws_bytes, void* stream);
int aae_decoder_forward_timed(aae_decoder* dec, const float* z, int B, float* x_out, void* workspace,
                              size_t ws_bytes, void* stream, float* kernel_ms, int max_kernels, int* n_kernels);
const char* aae_decoder_kernel_label(const aae_decoder* dec, int i);
double aae_decoder_kernel_flops(const aae_decoder* dec, int i);
/* workspace region of hidden activation `stage` (0 = dense output, i = i-th hidden conv) */
int aae_decoder_activation_info(const aae_decoder* dec, int B, int stage, size_t* offset_bytes, size_t* count);

/* ---- Mesh rasteriser: the views a codebook is built from -----------------------------------------
 * Replaces Renderer.render (auto_pose/meshrenderer/meshrenderer_phong.py:101-168 for model = reconst,
 * meshrenderer.py:84-137 for model = cad: one OpenGL draw per view), calc_2d_bbox on the rendered depth
 * (pysixd/view_sampler.py:10-15) and extract_square_patch + cv2.resize(INTER_NEAREST) on the rendered colour
 * (auto_pose/ae/dataset.py:308-373) for a batch of views in a few launches.  Geometry is float64 / integer and
 * reproducible bit for bit (csrc/kernels/render_core.h states the rule); parity with an OpenGL driver is unpinned.
 * Deviations: a triangle with a vertex nearer than `near` is dropped whole instead of clipped; no multisampling. */
typedef struct aae_mesh aae_mesh;

#define AAE_MODEL_RECONST 0       /* indexed mesh, per-vertex normals and colours, Phong shader                */
#define AAE_MODEL_CAD 1           /* triangle soup with per-face normals, constant material (cad_shader.frag)  */

/* Host arrays, copied to the device: verts / normals [n_verts,3] float32, colors [n_verts,3] float32 rgb in [0,1] or NULL
 * (160/255, meshrenderer_phong.py:50), faces [n_faces,3] int32 (every index is checked).  Vertices are stored as
 * float32(vertex * vertex_scale), as the reference's vertex buffer holds them. */
int aae_mesh_create(const float* verts, const float* normals, const float* colors, int n_verts, const int32_t* faces, int n_faces,
                    int model, float vertex_scale, aae_mesh** out);
void aae_mesh_destroy(aae_mesh* mesh);

typedef struct aae_render_params {
    double K[9];                  /* row-major intrinsics; K[3], K[6], K[7] must be 0 (camera.py:177-185)      */
    double t[3];                  /* translation of every view when the call takes no per-view ts            */
    int32_t W, H;                 /* render dims                                                               */
    double clip_near, clip_far;
    double pad_factor;            /* [Dataset] PAD_FACTOR (embedding views only)                               */
    float light[3];               /* light position in eye coordinates; the reference's default (400,400,400) */
    float ambient, diffuse, specular;   /* 0.4, 0.8, 0.3                                                       */
} aae_render_params;

size_t aae_render_workspace_bytes(const aae_mesh* mesh, int n_views, int W, int H);

/* Dataset.render_embedding_image_batch without the host: Rs device float64 [n,9] (row-major rotations) ->
 * crops_out device uint8 [n,crop,crop,3] BGR, bbs_out device int32 [n,4] (x, y, w, h), visible_out device int32 [n]
 * (0: no pixel covered -- the reference raises ValueError from calc_2d_bbox; that view's crop and box are 0).
 * The workspace may hold anything on entry; no allocation, no synchronisation, capturable into a graph.  n <= 65535. */
int aae_render_embedding_views(const aae_mesh* mesh, const double* Rs, int n, const aae_render_params* params, int crop,
                               void* crops_out, int32_t* bbs_out, int32_t* visible_out, void* workspace, size_t ws_bytes, void* stream);
/* the same call with the time of each of its six launches (init, vertex, clear, raster, bbox, crop) from events on
 * `stream`; synchronises, so not for capture */
int aae_render_embedding_views_timed(const aae_mesh* mesh, const double* Rs, int n, const aae_render_params* params, int crop,
                                     void* crops_out, int32_t* bbs_out, int32_t* visible_out, void* workspace, size_t ws_bytes,
                                     void* stream, float* kernel_ms);
/* Full frames: ts device float64 [n,3] (one translation per view) or NULL (params->t) -> bgr_out device uint8 [n,H,W,3],
 * depth_out device float32 [n,H,W] (0 = background), tri_out device int32 [n,H,W] or NULL (index of the visible face, -1 =
 * background), bbs_out / visible_out as above. */
int aae_render_frames(const aae_mesh* mesh, const double* Rs, const double* ts, int n, const aae_render_params* params,
                      void* bgr_out, float* depth_out, int32_t* tri_out, int32_t* bbs_out, int32_t* visible_out, void* workspace,
                      size_t ws_bytes, void* stream);

/* Training pairs: the loop of Dataset.render_training_images (auto_pose/ae/dataset.py:219-306) for n rotations at params->t, the
 * geometry of a pair done once.  Rs device float64 [n,9]; lights device float32 [n,6] (position xyz in eye coordinates, ambient,
 * diffuse, specular: the light train_x is drawn with); offsets device float64 [n,2] (u_x, u_y: train_x is cut around
 * int32(obj_bb + [u_x w, u_y h, 0, 0]), dataset.py:282-285).  params: t, K, dims, near / far, pad_factor and the default light
 * train_y is drawn with.  train_x / train_y device uint8 [n,crop,crop,3] BGR, mask_x device uint8 [n,crop,crop] (1 where the
 * train_x sample is background), bbs_out device int32 [n,4] (the true box), visible_out device int32 [n] (0: no pixel covered;
 * that view's crops are 0 and its mask all 1).  train_y is byte for byte aae_render_embedding_views of the same call, train_x
 * what aae_render_frames with that view's light gives, cut around the shifted box.  The workspace
 * (aae_render_training_workspace_bytes) may hold anything on entry; no allocation, no synchronisation, no copy from host
 * memory: capturable into a graph.  n <= 65535. */
size_t aae_render_training_workspace_bytes(const aae_mesh* mesh, int n_views, int W, int H);
int aae_render_training_views(const aae_mesh* mesh, const double* Rs, const float* lights, const double* offsets, int n,
                              const aae_render_params* params, int crop, void* train_x, void* mask_x, void* train_y, int32_t* bbs_out,
                              int32_t* visible_out, void* workspace, size_t ws_bytes, void* stream);
/* the same call with the time of each of its six launches (init, vertex, clear, raster, bbox, crop) from events on `stream`;
 * synchronises, so not for capture */
int aae_render_training_views_timed(const aae_mesh* mesh, const double* Rs, const float* lights, const double* offsets, int n,
                                    const aae_render_params* params, int crop, void* train_x, void* mask_x, void* train_y, int32_t* bbs_out,
                                    int32_t* visible_out, void* workspace, size_t ws_bytes, void* stream, float* kernel_ms);

/* Several meshes into one frame: Renderer.render_many (meshrenderer.py:140-194, meshrenderer_phong.py:170-224), which
 * PoseVisualizer.render_poses (visualization/render_pose.py) and the multi-object demos end in.  A draw is (mesh of a set, R, t,
 * scene); the draws of one scene share one depth buffer.  Per draw the fragments are those of aae_render_frames for that mesh and
 * pose alone; across draws the nearest fp32 depth wins, at equal depth the earlier draw of the call's arrays, then the lower face
 * (GL_LESS, the first-drawn fragment kept).  The box of a draw is calc_2d_bbox of the draw rendered alone, as render_many
 * returns it, not the box of its visible part.  One light and one set of Phong constants per call. */
typedef struct aae_mesh_set aae_mesh_set;
/* borrows the meshes (they must outlive the set); all of one model kind, else AAE_ERR_UNSUPPORTED; allocation happens here */
int aae_mesh_set_create(const aae_mesh* const* meshes, int n_meshes, aae_mesh_set** out);
void aae_mesh_set_destroy(aae_mesh_set* set);

#define AAE_SCENE_MAX_DRAWS 256   /* the (mesh, scene) table of a call travels in the kernel arguments               */
size_t aae_render_scenes_workspace_bytes(const aae_mesh_set* set, int n_draws, int n_scenes, int W, int H);

/* obj_ids, scene_ids: HOST int32 [n_draws], validated here (0 <= obj < meshes of the set, 0 <= scene < n_scenes; any order;
 * a scene without draws is all background).  Rs device float64 [n_draws,9], ts device float64 [n_draws,3] (required; params->t
 * and pad_factor are not read).  bgr_out device uint8 [n_scenes,H,W,3], depth_out device float32 [n_scenes,H,W] (0 = background),
 * draw_out / tri_out device int32 [n_scenes,H,W] or NULL (-1 = background), bbs_out device int32 [n_draws,4], visible_out
 * device int32 [n_draws] (0: the draw covers no pixel, its box is 0).  n_draws <= AAE_SCENE_MAX_DRAWS, n_scenes <= 65535,
 * n_draws * (largest face count of the set) <= 2^32 - 1.  The workspace may hold anything on entry; no allocation, no
 * synchronisation, no copy from host memory: capturable into a graph. */
int aae_render_scenes(const aae_mesh_set* set, const int32_t* obj_ids, const int32_t* scene_ids, const double* Rs, const double* ts,
                      int n_draws, int n_scenes, const aae_render_params* params, void* bgr_out, float* depth_out,
                      int32_t* draw_out, int32_t* tri_out, int32_t* bbs_out, int32_t* visible_out,
                      void* workspace, size_t ws_bytes, void* stream);
/* the same call with the time of each of its six launches (init, vertex, clear, raster, bbox, frame) from events on `stream`;
 * synchronises, so not for capture */
int aae_render_scenes_timed(const aae_mesh_set* set, const int32_t* obj_ids, const int32_t* scene_ids, const double* Rs, const double* ts,
                            int n_draws, int n_scenes, const aae_render_params* params, void* bgr_out, float* depth_out,
                            int32_t* draw_out, int32_t* tri_out, int32_t* bbs_out, int32_t* visible_out,
                            void* workspace, size_t ws_bytes, void* stream, float* kernel_ms);

/* The blend of visualization/render_pose.py:44-46, device uint8 buffers of n_pixels*3 bytes:
 * out[e] = render[e] > 0 ? (uint8)((render[e] * (e % 3 == channel)) * 2./3. + image[e] * 1./3.) : image[e], in float64 as NumPy
 * computes it; out may alias image */
int aae_overlay_blend(const void* image, const void* render, size_t n_pixels, int channel, void* out, void* stream);

/* ---- Depth ICP refinement ---------------------------------------------------------------------------
 * Replaces icp_refinement's point clouds, filter and ICP loop (auto_pose/eval/icp_utils.py:96-175,248-274 and the
 * same code in auto_pose/icp/icp.py) for up to AAE_ICP_MAX_PROBLEMS detections per call, all in float64
 * (csrc/kernels/icp_core.h states the arithmetic and the exactness rule).  The caller renders the synthetic depth
 * (aae_render_frames), decides "too few points", draws the subsample and composes the pose: the random numbers and
 * the 4x4 products stay on the host.  Nearest neighbours are exact; among equidistant targets the lowest index wins
 * (the reference's KD-tree answers any of them).
 * The workspace may hold anything on entry; no allocation and no synchronisation inside a call. */
#define AAE_ICP_MAX_PROBLEMS 16
#define AAE_ICP_MAX_POINTS 4096   /* subsampled points of one problem (the reference draws at most 3000)          */
#define AAE_ICP_DEPTH_ONLY 1      /* best_fit_transform(depth_only=True): R = I, t = (0, 0, dz)                   */
#define AAE_ICP_NO_DEPTH 2        /* no_depth=True, eval/icp_utils.py:60-61: t = (t_x, t_y, 0)                    */
#define AAE_ICP_NO_DEPTH_ZERO_T 4 /* with AAE_ICP_NO_DEPTH, icp/icp.py:58-61: t = (0, 0, 0)                        */

typedef struct aae_icp_shape {
    int32_t n_problems;           /* 1 ... AAE_ICP_MAX_PROBLEMS                                                   */
    int32_t max_points;           /* 3 ... AAE_ICP_MAX_POINTS: the largest subsample of a problem                 */
    int32_t W, H;                 /* the synthetic depth frames                                                   */
    int32_t crop_w, crop_h;       /* the largest depth crop (a crop of h x w needs h * w <= crop_w * crop_h)      */
} aae_icp_shape;

size_t aae_icp_workspace_bytes(int n_problems, int max_points, int W, int H, int crop_w, int crop_h);

/* Steps 1-3.  syn_depth device float32 [P,H,W] (rendered at R_est, t = (0, 0, t_z)); crop_depth device float32
 * [P, crop_w * crop_h], crop p dense (crop_dims[2p] rows x crop_dims[2p+1] columns, host int32) at the front of its
 * slot; K host float64 [9] (K_test); max_mean_dist_factor 2.0 or 4.0.  Per problem the workspace then holds the
 * synthetic points (depth != 0, row-major order, misc.py:65-70), their centroid and largest distance, and the real
 * points of the crop (principal point (rows / 2, columns / 2) floored, as the reference sets it) nearer to the
 * centroid than factor * that distance, in order.  counts_out: host int32 [P,2] (synthetic, real), written by a copy
 * queued on `stream` (pinned memory keeps it asynchronous): valid once the stream has reached it. */
int aae_icp_prepare(const aae_icp_shape* shape, const float* syn_depth, const float* crop_depth, const int32_t* crop_dims,
                    const double* K, double max_mean_dist_factor, int32_t* counts_out, void* workspace, size_t ws_bytes, void* stream);

/* where a prepared workspace keeps problem `problem`'s data (for the tests and for callers that want the clouds):
 * what = 0 synthetic points (float64 [count,3]), 1 real points, 2 (centroid[3], largest distance, threshold) float64 [5] */
int aae_icp_workspace_info(const aae_icp_shape* shape, int problem, int what, size_t* offset_bytes, size_t* capacity);

/* Steps 5-6 on a prepared workspace: icp(A = syn[sub_syn], B = real[sub_real], tolerance) per problem.  n_points host
 * int32 [P] (3 ... max_points, or 0 for a problem to leave out: T = identity, i = -1; else AAE_ERR_INVALID); sub_syn / sub_real device int32 [P, max_points] (an index outside
 * [0, count) is clamped and sets bit 0 of error_out[p]); modes host int32 [P] (AAE_ICP_* flags).  Queues one gather,
 * max_iterations icp_step launches (a converged problem's blocks return at once) and one finish, with no host round trip:
 * intended to be capturable, not yet exercised under capture.
 * Outputs, device: T_out float64 [P,16] (row-major 4x4), iterations_out int32 [P] (the reference's i), mean_error_out
 * float64 [P], error_out int32 [P], and optionally (or NULL) the last iteration's distances float64 [P, max_points]
 * and matched target indices int32 [P, max_points]. */
int aae_icp_refine(const aae_icp_shape* shape, const int32_t* n_points, const int32_t* sub_syn, const int32_t* sub_real,
                   const int32_t* modes, int max_iterations, double tolerance, double* T_out, int32_t* iterations_out,
                   double* mean_error_out, int32_t* error_out, double* d2_out, int32_t* idx_out, void* workspace,
                   size_t ws_bytes, void* stream);
/* the same call with the time of each launch (gather, max_iterations steps, finish: max_iterations + 2 floats) from
 * events on `stream`; synchronises, so not for capture */
int aae_icp_refine_timed(const aae_icp_shape* shape, const int32_t* n_points, const int32_t* sub_syn, const int32_t* sub_real,
                         const int32_t* modes, int max_iterations, double tolerance, double* T_out, int32_t* iterations_out,
                         double* mean_error_out, int32_t* error_out, double* d2_out, int32_t* idx_out, void* workspace,
                         size_t ws_bytes, void* stream, float* kernel_ms);

/* ---- training batches: Dataset.batch (auto_pose/ae/dataset.py:456-495) in one launch --------------------------------
 * One workgroup per batch image: x = mask ? bg : train_x is composited into LDS, the image's op program runs there
 * (uint8 between ops; every real result is clipped to [0,255] and rounded half to even), and the result is written as
 * uint8 and / or as float32(v / 255.).  csrc/kernels/augment_core.h states the arithmetic of every op; DESIGN section 4
 * lists the imgaug 0.4.0 semantics it assumes.  Random numbers are drawn by the caller: a program holds only values. */
#define AAE_AUGMENT_MAX_OPS 16
#define AAE_AUGMENT_MAX_BLUR_K 15
#define AAE_AUGMENT_AFFINE 1    /* f[0] = 1 / scale                                                                      */
#define AAE_AUGMENT_DROPOUT 2   /* i[0] mask bits, i[1] row table, i[2] column table (word offsets into aux); i[3] =
                                   h_s * w_s when per channel, else 0.  row table: int32 [H] cell row * w_s; column table:
                                   int32 [W] cell column; bit (c * i[3] + row + column) set = dropped                     */
#define AAE_AUGMENT_BLUR 3      /* i[0] = k (odd, <= AAE_AUGMENT_MAX_BLUR_K, k / 2 < min(H, W)), i[1] = word offset of
                                   k normalised float32 weights in aux                                                   */
#define AAE_AUGMENT_ADD 4       /* f[c] = integer added to channel c                                                     */
#define AAE_AUGMENT_INVERT 5    /* i[c] != 0: 255 - x on channel c                                                       */
#define AAE_AUGMENT_MULTIPLY 6  /* f[c] = factor of channel c                                                            */
#define AAE_AUGMENT_CONTRAST 7  /* f[c] = alpha of channel c: 128 + alpha * (x - 128)                                    */

typedef struct aae_augment_op {
    int32_t code;
    int32_t i[4];
    float f[3];
} aae_augment_op;

typedef struct aae_augment_shape {
    int32_t N, M;                 /* training images, background images                                           */
    int32_t H, W, C;              /* C <= 3; H * W * C <= aae_augment_max_image_bytes()                           */
    int32_t B;                    /* batch size = workgroups                                                      */
    int32_t aux_words;            /* dwords in aux                                                                */
} aae_augment_shape;

/* the largest H * W * C: two image buffers must fit the workgroup's LDS (81920; 128 x 128 x 3 is 49152) */
size_t aae_augment_max_image_bytes(void);

/* All pointers device-resident.  train_x / train_y uint8 [N,H,W,C], mask_x one byte per pixel [N,H,W] (non-zero =
 * background), bg uint8 [M,H,W,C]; train_idx / bg_idx / n_ops int32 [B]; ops [B, AAE_AUGMENT_MAX_OPS]; aux uint32
 * [aux_words] (NULL when 0).  Outputs [B,H,W,C], each may be NULL: batch_x_u8, batch_x_f32 = float32(x / 255.),
 * batch_y_f32 = float32(train_y / 255.).  An image over the LDS limit is refused with AAE_ERR_UNSUPPORTED naming the
 * limit, and nothing is launched.  The kernel trusts no index: an image whose train_idx / bg_idx is out of range is
 * left unwritten, an op whose aux ranges do not lie inside aux is skipped.  One launch on `stream`, no allocation, no
 * synchronisation. */
int aae_augment_batch(const aae_augment_shape* shape, const void* train_x, const void* mask_x, const void* train_y, const void* bg,
                      const int32_t* train_idx, const int32_t* bg_idx, const int32_t* n_ops, const aae_augment_op* ops,
                      const uint32_t* aux, void* batch_x_u8, float* batch_x_f32, float* batch_y_f32, void* stream);

/* ---- The training loss: bootstrapped L2 / L1 reconstruction loss and the latent-norm regulariser (the reference's
 * auto_pose/ae/decoder.py:86-132, encoder.py:97-100), with their gradients with respect to the tensors they read. ------- */
#define AAE_LOSS_L2 0
#define AAE_LOSS_L1 1
#define AAE_LOSS_MAX_BATCH 65536      /* B of both calls                                                              */
#define AAE_LOSS_MAX_N 4194304        /* n = H * W * C of one image                                                   */
#define AAE_LOSS_MAX_LATENT 1048576   /* J                                                                            */

typedef struct aae_recon_loss_desc { int32_t B, n, kind /* 0 = L2, 1 = L1 */, bootstrap_ratio; } aae_recon_loss_desc;

/* bytes of workspace aae_recon_loss needs (16-byte aligned); 0 for a B or n outside the limits */
size_t aae_recon_loss_workspace_bytes(int B, int n);

/* x / target device float32 [B, n].  e = (x - t)^2 (L2) or |x - t| (L1) in fp32.  bootstrap_ratio > 1: per image the
 * k = n / bootstrap_ratio (integer division) largest errors are selected, among equal errors the lowest indices first
 * (tf.nn.top_k); bootstrap_ratio = 1: every element.  per_image[b] = mean of image b's selected errors, loss = mean of
 * per_image over B.  dx[b, i] = 2 (x - t) / (B k) (L2) or sign(x - t) / (B k) (L1) on a selected element, 0 elsewhere;
 * every element of dx is written.  per_image and dx may be NULL.  A NaN error ranks above every number: that image's
 * mean and the loss are NaN, the other images are unaffected, the call returns AAE_OK.  Refused with nothing launched:
 * a NULL desc / x / target / loss / workspace (AAE_ERR_INVALID), B < 1, n < 1, bootstrap_ratio < 1, a kind other than
 * the two, k = 0 (AAE_ERR_INVALID), B or n over the limits above (AAE_ERR_UNSUPPORTED), a short or misaligned workspace
 * (AAE_ERR_WORKSPACE).  Two launches on `stream`; no allocation, no synchronisation, no host copy, no floating-point
 * atomic (the same inputs give the same bits); capturable. */
int aae_recon_loss(const aae_recon_loss_desc* d, const float* x, const float* target,
                   float* loss /* [1] */, float* per_image /* [B] or null */, float* dx /* [B*n] or null */,
                   void* workspace, size_t ws_bytes, void* stream);

/* z device float32 [B, J].  loss = mean_b | ||z_b|| - 1 |;  dz[b] = sign(||z_b|| - 1) z_b / ||z_b|| / B, 0 for a zero
 * row (dz may be NULL).  One launch on `stream`, no workspace, no allocation, no synchronisation; capturable. */
int aae_latent_reg_loss(const float* z, int B, int J, float* loss /* [1] */, float* dz /* [B*J] or null */, void* stream);

/* ---- The decoder's backward pass: the gradient of every variable of a stage and dL/d(input), from dL/d(output) and the
 * activations the forward left behind.  A stage is: nearest resize of a_in [B,H,W,Cin] to UH x UW
 * (iy = min(y H / UH, H - 1)), KS x KS 'same' stride-1 convolution with w [KS,KS,Cin,Cout], bias, activation -> a_out.
 *   delta = g_out where a_out > 0 else 0 (ReLU, act 0);  (g_out a_out)(1 - a_out) in that order, fp32 (sigmoid, act 1)
 *   db[co] = sum delta;  dw[kh,kw,ci,co] = sum up(a_in)[b,y+kh-p,x+kw-p,ci] delta[b,y,x,co];  g_in = the transposed convolution
 * Exact 2x stages run phase-folded (four U x U problems on the source grid, U = (KS + 1) / 2), 1x stages as the one-phase case;
 * any other resize is refused with AAE_ERR_UNSUPPORTED and nothing launched (the forward's direct kernel runs it; training it is
 * not built).  No floating-point atomic: the same inputs give the same bits.  No allocation, synchronisation or host copy;
 * capturable.  Every tensor is a 16-byte aligned device float32 array; g_in / dz may be NULL (that product is not computed). */
typedef struct aae_upconv_backward_desc { int32_t B, H, W, Cin, UH, UW, Cout, KS, act /* 0 = ReLU, 1 = sigmoid */; } aae_upconv_backward_desc;
typedef struct aae_dense_backward_desc { int32_t B, J, U; } aae_dense_backward_desc;

/* bytes of workspace (256-byte aligned) the call needs; 0 for a shape the call refuses */
size_t aae_upconv_backward_workspace_bytes(const aae_upconv_backward_desc* d, int with_g_in);
int aae_upconv_backward(const aae_upconv_backward_desc* d, const float* a_in, const float* a_out, const float* g_out,
                        const float* w_hwio, float* dw /* [KS,KS,Cin,Cout] */, float* db /* [Cout] */,
                        float* g_in /* [B,H,W,Cin] or null */, void* workspace, size_t ws_bytes, void* stream);

/* the dense layer a_out = relu(z w + b), z [B,J], w [J,U]:  dw = z^T delta, db = sum_b delta, dz = delta w^T */
size_t aae_dense_backward_workspace_bytes(const aae_dense_backward_desc* d, int with_dz);
int aae_dense_backward(const aae_dense_backward_desc* d, const float* z, const float* a_out, const float* g_out,
                       const float* w, float* dw /* [J,U] */, float* db /* [U] */, float* dz /* [B,J] or null */,
                       void* workspace, size_t ws_bytes, void* stream);

/* The whole decoder, after aae_decoder_forward(dec, z, B, x, forward_workspace, ...) of the same batch: dx = dL/dx [B,H,W,C] in,
 * the gradient of every variable out.  weights[] / grads[]: device pointers in the order of aae_decoder_create (kernel, bias per
 * layer, dense first), in checkpoint shapes; the weights are the caller's current ones (the folded copies are made on the device per
 * call).  dz [B, latent] may be NULL.  forward_workspace is only read.  Refused with AAE_ERR_UNSUPPORTED and nothing launched: a
 * decoder with batch_norm (training-mode statistics are not built), a stage whose resize is neither exactly 2x nor 1x.
 * The timed twin synchronises the stream and returns the time between launches (labels: aae_decoder_bwd_label). */
int aae_decoder_get_desc(const aae_decoder* dec, aae_decoder_desc* out);
size_t aae_decoder_backward_workspace_bytes(const aae_decoder* dec, int B);
int aae_decoder_backward(const aae_decoder* dec, int B, const float* z, const float* x, const float* dx, const void* forward_workspace,
                         const float* const* weights, float* const* grads, float* dz, void* workspace, size_t ws_bytes, void* stream);
int aae_decoder_backward_timed(const aae_decoder* dec, int B, const float* z, const float* x, const float* dx, const void* forward_workspace,
                               const float* const* weights, float* const* grads, float* dz, void* workspace, size_t ws_bytes, void* stream,
                               float* kernel_ms, int max_kernels, int* n_kernels);

/* what the last backward call of the calling thread launched, in launch order: "<stage>:<form> M= N= K= ... splits=" */
int aae_decoder_bwd_label_count(void);
const char* aae_decoder_bwd_label(int i);

/* ---- The encoder's backward pass: the gradient of every variable of a layer and dL/d(input), from dL/d(output) and the
 * activations the forward left behind.  A layer is a KS x KS TF-'same' convolution of stride S with
 * w [KS,KS,Cin,Cout] (Ho = ceil(H / S); padding before = total / 2, the odd pixel at the end), bias, ReLU -> a_out [B,Ho,Wo,Cout].
 *   delta = g_out where a_out > 0 else 0;  db[co] = sum delta
 *   dw[kh,kw,ci,co] = sum a_in[b, S oy + kh - pt, S ox + kw - pl, ci] delta[b,oy,ox,co]   (taps in the padding contribute nothing)
 *   g_in[b,iy,ix,ci] = sum delta[b,oy,ox,co] w[kh,kw,ci,co] over S oy + kh - pt = iy, S ox + kw - pl = ix
 * The data gradient runs by input parity (iy mod S, ix mod S): each class is a stride-1 problem over the taps it sees; a class
 * without a tap (KS 1, S 2) is written with zeros.  a_in is float32, or uint8 read as float32(v / 255.) (x_dtype: AAE_DTYPE_*),
 * the two inputs the forward's first layer takes.  Strides 1 and 2, KS 1 ... 7; a stride of 3 or more is refused with
 * AAE_ERR_UNSUPPORTED and nothing launched.  No floating-point atomic: the same inputs give the same bits.  No allocation,
 * synchronisation or host copy; capturable.  Every tensor is 16-byte aligned; g_in / g_a / dx may be NULL (not computed). */
typedef struct aae_conv_backward_desc { int32_t B, H, W, Cin, Cout, KS, S, x_dtype /* of a_in: AAE_DTYPE_U8 | AAE_DTYPE_F32 */; } aae_conv_backward_desc;

/* bytes of workspace (256-byte aligned) the call needs; 0 for a shape the call refuses */
size_t aae_conv_backward_workspace_bytes(const aae_conv_backward_desc* d);
int aae_conv_backward(const aae_conv_backward_desc* d, const void* a_in, const float* a_out, const float* g_out,
                      const float* w_hwio, float* dw /* [KS,KS,Cin,Cout] */, float* db /* [Cout] */,
                      float* g_in /* [B,H,W,Cin] or null */, void* workspace, size_t ws_bytes, void* stream);

/* the linear dense layer z = a w + b, a [B,J], w [J,U], dz = dL/dz [B,U]:  dw = a^T dz, db = sum_b dz, g_a = dz w^T */
size_t aae_linear_backward_workspace_bytes(const aae_dense_backward_desc* d, int with_g_a);
int aae_linear_backward(const aae_dense_backward_desc* d, const float* a, const float* dz, const float* w,
                        float* dw /* [J,U] */, float* db /* [U] */, float* g_a /* [B,J] or null */,
                        void* workspace, size_t ws_bytes, void* stream);

/* The whole encoder, after aae_encoder_forward(enc, x, x_dtype, B, z, forward_workspace, ...) of the same batch: dz = dL/dz
 * [B, latent] in, the gradient of every variable out.  weights[] / grads[]: device pointers in the order of aae_encoder_create
 * (kernel, bias per conv layer, then the dense layer), in checkpoint shapes; the weights are the caller's current ones.
 * dx [B,H,W,C] float32 may be NULL.  forward_workspace is only read: the ReLU masks and the layer inputs are the fp32 activations
 * the forward left there.  Refused with AAE_ERR_UNSUPPORTED and nothing launched: an encoder with batch_norm (training-mode
 * statistics are not built), a batch whose forward ran in split precision (aae_encoder_split_precision_for_batch) or with
 * "compact_workspace" (the activations are then fp16 pairs, or overwritten), a stride of 3 or more.
 * The timed twin synchronises the stream and returns the time between launches (labels: aae_encoder_bwd_label). */
int aae_encoder_get_desc(const aae_encoder* enc, aae_encoder_desc* out);
size_t aae_encoder_backward_workspace_bytes(const aae_encoder* enc, int B);
int aae_encoder_backward(const aae_encoder* enc, int B, const void* x, int x_dtype, const float* dz, const void* forward_workspace,
                         const float* const* weights, float* const* grads, float* dx, void* workspace, size_t ws_bytes, void* stream);
int aae_encoder_backward_timed(const aae_encoder* enc, int B, const void* x, int x_dtype, const float* dz, const void* forward_workspace,
                               const float* const* weights, float* const* grads, float* dx, void* workspace, size_t ws_bytes, void* stream,
                               float* kernel_ms, int max_kernels, int* n_kernels);

/* what the last encoder-backward call of the calling thread launched, in launch order: "<layer>:<form> M= N= K= ... splits=" */
int aae_encoder_bwd_label_count(void);
const char* aae_encoder_bwd_label(int i);

#ifdef __cplusplus
}
#endif
#endif /* AAE_HIP_H_ */
