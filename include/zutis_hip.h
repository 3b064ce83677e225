/* libzutis_hip — C ABI of the MI355X (gfx950) kernels behind the ZUTIS dense-prediction hot path.
 *
 * The reference (NoelShin/zutis) has no FFI layer: its boundary is the Python nn.Module call surface
 * (SURVEY.md §8b).  This header is the boundary *underneath* this build's Python mirror of that surface
 * (zutis_amd/dropin/networks/zutis.py ...): every entry point replaces one stock-op sequence of the reference,
 * cited per function as file:line relative to the reference root.
 *
 * Conventions
 *   - extern "C"; every entry returns int: 0 = ok, <0 = error (ZH_ERR_*); zh_last_error() gives thread-local text.
 *   - All pointers are raw DEVICE pointers owned by the caller (PyTorch tensors); the library never allocates,
 *     frees or synchronises.  Scratch is passed in (void* workspace, size_t bytes) with a *_workspace_size query.
 *   - Last argument: the hipStream_t to launch on (pass torch.cuda.current_stream().cuda_stream).
 *   - Layout: contiguous row-major, tokens channels-last [B, T, D].  "f16" = IEEE half; fp32 accumulate everywhere.
 *   - Split pairs (the reference-equivalent "f16x3" precision): a tensor x stored as two fp16 planes, hi = f16(x) at the
 *     pointer and lo = f16(x - hi) `lo_plane` ELEMENTS further on (22 significand bits).  Producers take a `lo_plane`
 *     argument (0 = write the plain fp16 tensor only; the hi plane alone IS that tensor); zh_gemm_f16x3 and the split-pair
 *     form of zh_attention_f16 consume them.
 *   - Re-entrant.  Process-wide state: none on the product path; the developer entry zh_dev_set_gemm_overrides() (forced GEMM tile /
 *     super-tile height, used by tests and tools only) is process-wide by design, and zh_last_error() text is thread-local, as is the
 *     number of launches in flight that a plan replay loop sets while it runs (zh_dev_set_gemm_inflight).
 */
#ifndef ZUTIS_HIP_H
#define ZUTIS_HIP_H

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct ihipStream_t* zh_stream_t; /* == hipStream_t */

#define ZH_OK 0
#define ZH_ERR_ARG (-1)
#define ZH_ERR_HIP (-2)
#define ZH_ERR_WORKSPACE (-3)

/* GEMM epilogue activations */
#define ZH_ACT_NONE 0
#define ZH_ACT_QUICKGELU 1 /* x*sigmoid(1.702x)  networks/clip_arch.py:295-297 */
#define ZH_ACT_RELU 2      /* networks/zutis.py:546-549; networks/transformer.py:289 */
#define ZH_ACT_SIGMOID 3   /* networks/zutis.py:209 */
#define ZH_ACT_GELU_ERF 4  /* nn.GELU, networks/selfmask/vision_transformer.py:79 */

/* ABI version: bumped whenever an entry point's signature changes.  zh_version() returns the value the library was BUILT
 * with; a binding compiled / written against this header must refuse a library that reports another one (zutis_amd/_lib.py
 * does) — ctypes cannot see a changed argument list. */
#define ZH_ABI_VERSION 247 /* 247: zh_second_largest_component / zh_components_workspace_size (the mask post-processing of bilateral_solver_output on the device: fill holes, label, second largest, ZH_CCL_TILE_*); 246: zh_dev_set_gemm_inflight / zh_dev_gemm_plan_inflight; the replay loops zh_plan_run_multi / zh_plan_run2 tell the GEMM tile chooser how many launches meet on the chip (a behaviour change: other tiles in flight, the same bits); 245: zh_jpeg_encode / zh_jpeg_encode_host (the device JPEG encoder: overlays leave the GPU as the scan of a baseline JPEG, ZH_JPEG_ENC_*); 244: zh_jpeg_decode_split / zh_jpeg_decode_split_host (a scan without restart markers split among lanes, ZH_JPEG_CHUNK_*, ZH_JPEG_SPLIT_*, ZH_JPEG_STATUS_UNSYNCED); 243: zh_jpeg_decode / zh_jpeg_decode_host (the device JPEG decoder: baseline files reach the GPU as file bytes, ZH_JPEG_*); 242: the attention entries take head_dim 128 (a behaviour change: a stale build would refuse the ViT-L decoder); 241: zh_dev_attention_plan (what the attention launcher decides, asked without launching), ZH_ATTN_QUERY_BLOCK / ZH_ATTN_KEY_TILE_*; 240: zh_topk_rows orders every NaN first and -0.0 equal to +0.0 (a behaviour change: a stale build would select other columns); 239: zh_png_deflate (the device PNG encoder: pictures leave the GPU as the zlib stream of their PNG, ZH_PNG_SEGMENT_BYTES); 238: zh_dev_gemm_plan (what the GEMM dispatcher decides, asked without launching); 237: zh_runs_label_maps (semantic ground truth painted from the annotations' run lengths, ZH_OVERLAP_*, ZH_LABEL_TILE_*); 236: zh_polygon_runs (polygon annotations to run lengths on the device, ZH_POLYGON_LDS_CROSSINGS); 235: zh_instance_paint (instance predictions as pictures: id map and colour overlay of the kept masks); 234: COCO mask AP on the device (zh_rle_prefix, zh_rle_pair_iou, zh_coco_match, ZH_RLE_IOU_LDS_RUNS); 233: zh_upsample_argmax_bytes (predictions as file bytes: the label PNG's bytes and a colour overlay from the arg-max launch); 232: the criterion's assignment and mask packing on the device (zh_linear_assignment, zh_pack_masks_u8); 231: zh_upsample_argmax_score (evaluation: the confusion matrix fused into the arg-max launch, ZH_GT_*); 230: the training sample on the device (zh_synth_geometry_u8, zh_synth_photometric_u8, zh_synth_blur_u8, zh_synth_compose); 229: zh_resize_normalize_u8 (MaskDataset's resize + normalise of a ragged u8 batch, ZH_FILTER_*); 228: zh_resize_crop_normalize_u8 (CLIP pre-processing of a ragged u8 batch); 227: the fp16 residual stream (zh_gemm_f16_res16, zh_layernorm_f16, zh_assemble_tokens_ln_f16); 226: the training criterion (zh_mask_match_cost, zh_mask_match_grad, zh_upsample_ce_fwd / _bwd, zh_gemm_f32_strided), ZH_STATUS_LABEL; 225: zh_dev_set_gemm_persist; 224: zero_word of zh_mask_nms; 223: zh_mask_rle_fused_kept; 222: zh_mask_rle_kept; 221: packed_capacity of zh_mask_runs_kept (the kept masks' transitions as one list), packed form of zh_rle_from_transitions_host; 220: flags argument of zh_gemm_f16x3 (ZH_GEMM_FIXED_K_ORDER); 219: workspace of zh_mask_runs / zh_mask_runs_kept (two-launch run extraction); 218: status word of the LayerNorm family, f16_scale of the unit-norm producers; 217: zh_mask_runs_kept, range_flag / packed arguments of zh_instance_mask_stats / zh_mask_nms; 216: zh_sum_layernorm_f32, few-row kernel behind zh_gemm_f16x3; 215: zh_rle_from_transitions_host; 214: zh_gemm_f16x3 accepts planeW = 0 (fp16-valued weight: two products); 213: workspace argument of zh_masked_mean_tokens; 212: zh_attention_f16_splitk; 211: zh_dev_set_gemm_overrides; 210: pos_y / pos_x tables on zh_gemm_f16 / zh_gemm_f16x3 */
int zh_version(void);
const char* zh_arch(void);
const char* zh_last_error(void);

/* DEVELOPER entry (tests / tools, not part of the reference's surface): force the GEMM tile variant for the calls that follow.
 * group_m = super-tile height (0 = default 4); tile = tile code for zh_gemm_f16 (64|128|192|256|2064|2128|3064; 7032 / 7096 / 7128 = the
 * 64 x 64 / 128 x 96 / 128 x 128 tiles on 64-k slices) and zh_gemm_f16x3 (64|96|192|256|448|512|3064|1288; 3066 = 64 x 64 on 32-k slices,
 * 6464 / 6496 = 128 x 64 / 128 x 96 on 64-k slices in three / two whole slots, 7096 / 7128 = 128 x 96 / 128 x 128 on the circular piece ring;
 * 5122 / 5124 = the planeW = 0 form of 512 on two slots / as 2 x 4 waves of 128 x 64, 4484 = of 448 as 4 x 2 waves of 48 x 128), 0 = the cost model's choice; tile_small = the same, applied to M <= 4096 only.  Process-wide;
 * the initial values come from ZH_GEMM_GROUP_M / ZH_GEMM_TILE / ZH_GEMM_TILE_SMALL, read once. */
int zh_dev_set_gemm_overrides(int group_m, int tile, int tile_small);

/* DEVELOPER entry: what the GEMM dispatcher (csrc/gemm_dispatch.h) decides for a call, without launching; it is the function the three
 * GEMM entries below ask, under the overrides in force (zh_dev_set_gemm_overrides) and for the launches in flight that the calling
 * thread's next launch would see (1 unless forced, zh_dev_set_gemm_inflight).  Nothing is dereferenced: it runs without a GPU.
 * mode: 0 = zh_gemm_f16, 1 = zh_gemm_f16_res16, 2 = zh_gemm_f16x3, 3 = zh_gemm_f16x3 with planeW = 0; out_kind: 0 f32, 1 f16, 2 split pair
 * (modes 0 / 1: out_f16); C / bias / residual: the pointer VALUES of the call (alignment only, NULL = absent); has_pos: pos tables given.
 * plan (HOST int[6]) = {family (0 LDS ring, 1 few-row kernel), tile code as launched (0 = the base tile of the scalar / direct paths,
 * 32 = the few-row kernel), tile_m, tile_n, store path (ring: 0 scalar, 1 direct, 2 wide; few-row: 0 scalar, 1 vec), peel rows M'
 * (0 = one launch; else the call runs as rows [0, M') and [M', M), each with a plan of its own)}.  Returns what the entry's tile-related
 * argument checks return (grid too large; zh_gemm_f16: a forced code that is no tile code). */
int zh_dev_gemm_plan(int mode, int M, int N, int K, int batch, long lda, long ldw, long ldc, long strideC, long planeC,
                     long ldr, long strideR, int res_rows, int out_kind, int act, int flags,
                     const void* C, const void* bias, const void* residual, int has_pos, int* plan);

/* DEVELOPER entry: the big plain-fp16 GEMM tiles (256 x 256 / 256 x 192) are persistent — `workgroups` of them walk a launch's tiles and
 * request the next tile's first K slices under the current tile's epilogue (csrc/gemm_kernel.h PERS; bitwise the one-workgroup-per-
 * tile results).  Default (-1): the current device's CU count rounded down to a multiple of 8, resolved at the first launch (256 on an
 * MI355X in SPX mode; ZH_GEMM_PERSIST, validated the same way, read once); 0 = one workgroup per tile; any multiple of 8 forces that
 * many (tests use 8 to make small problems walk several tiles per workgroup).  Process-wide: the library's one mutable word that
 * steers product launches, written only here. */
int zh_dev_set_gemm_persist(int workgroups);

/* DEVELOPER entries: the number of copies of a GEMM launch that meet on the chip, which the tile chooser counts against the chip's
 * rounds (csrc/gemm_dispatch.h).  On the product path it is 1, and the stream count inside the replay loops zh_plan_run_multi (count)
 * and zh_plan_run2 (2): set for the duration of the loop on the calling thread, restored when it returns.  The bits of a result do not
 * depend on it.  zh_dev_set_gemm_inflight forces one value for every GEMM launch of the process (tests / tools: eager calls at a
 * forced value); 0 = not forced.  zh_dev_gemm_plan_inflight is zh_dev_gemm_plan for a given number (1 .. 64) instead of the one the
 * calling thread's next launch would see. */
int zh_dev_set_gemm_inflight(int inflight);
int zh_dev_gemm_plan_inflight(int mode, int M, int N, int K, int batch, long lda, long ldw, long ldc, long strideC, long planeC,
                              long ldr, long strideR, int res_rows, int out_kind, int act, int flags,
                              const void* C, const void* bias, const void* residual, int has_pos, int inflight, int* plan);

/* C[b][m][n] = act(sum_k A[b][m][k]*W[b][n][k] + bias[n] + pos[m][n]) + residual[b][m % res_rows][n]
 * A [M,K] f16 (lda), W [N,K] f16 (ldw) — torch Linear layout; C f32 or f16 (out_f16); bias/residual f32 or NULL.
 * K % 64 == 0; lda/ldw % 8 == 0.  residual may alias C (in-place x += ...).
 * pos (optional, pos_y and pos_x both NULL = none): output rows are pixels, m = image * pos_h*pos_w + y * pos_w + x, and
 * pos[m][n] = pos_y[y][n] + pos_x[x][n] with tables [pos_h, ld_pos] / [pos_w, ld_pos], fp32 or (pos_f16) fp16, ld_pos % 8 == 0,
 * N % 4 == 0.  This is the
 * `pos` term of the decoder's key projection of `memory + pos` (transformer.py:281-283): the sine PE is [py(y) | px(x)]
 * (positional_embedding.py:47-52), so pos @ Wk^T separates into two small input-independent tables and `memory + pos` is
 * never materialised; the accumulators start from the table values (read under the operand prefetch). */
int zh_gemm_f16(const void* A, long lda, long strideA, const void* W, long ldw, long strideW,
                void* C, long ldc, long strideC, int out_f16,
                const float* bias, const float* residual, long ldr, long strideR, int res_rows,
                const void* pos_y, const void* pos_x, long ld_pos, int pos_h, int pos_w, int pos_f16,
                int act, int M, int N, int K, int batch, zh_stream_t stream);

/* The residual update of a HALF-precision stream, x = x + linear(y) as the reference's own fp16 tower computes it (third-party
 * clip.load leaves the model in fp16 on a GPU, utils/extract_image_embeddings.py:43,72-78; ResidualAttentionBlock.forward,
 * clip_arch.py:318-321):  C[b][m][n] = f16( f16(sum_k A W + bias[n]) + residual[b][m % res_rows][n] ),  C and residual f16, the sum of
 * products and both additions in fp32, two roundings to fp16 (the Linear's output, then the sum).  Shapes, strides and alignment as
 * zh_gemm_f16 with out_f16 = 1; ldr % 4 == 0 and an 8-byte aligned residual (16-byte row stores also need ldr % 8 == 0 and 16-byte
 * alignment).  residual may alias C. */
int zh_gemm_f16_res16(const void* A, long lda, long strideA, const void* W, long ldw, long strideW,
                      void* C, long ldc, long strideC,
                      const float* bias, const void* residual, long ldr, long strideR, int res_rows,
                      int M, int N, int K, int batch, zh_stream_t stream);

/* The same contraction at the reference's precision (the reference computes every Linear / einsum in fp32:
 * clip_arch.py:286-292 keeps LayerNorm fp32, zutis.py:55 casts the CLIP weights to fp32).  A and W are split pairs
 * (planeA / planeW = element offset of the lo plane); the kernel accumulates Ah.Wh + Ah.Wl + Al.Wh in fp32 (dropped
 * term: 2^-22 relative) and multiplies the accumulator by out_scale (weights are packed as W * 2^s, out_scale = 2^-s,
 * so that lo planes stay normal fp16 numbers) before the bias.  out_kind: 0 = f32 (residual allowed), 1 = f16,
 * 2 = split pair (lo plane at C + planeC).
 * planeW = 0: W has NO lo plane — every value of W * 2^s is an fp16 number, as for the released CLIP towers, whose weights the
 * reference's own constructor rounds to fp16 (convert_weights, clip_arch.py:566-587,625) before zutis.py:55 / encode_image use
 * them: the kernel then issues Ah.Wh + Al.Wh only, bit-identical to the three-product form on a zero lo plane, at 2/3 of the
 * MFMA work ("f16x2").  A is always a split pair.
 * flags: ZH_GEMM_FIXED_K_ORDER (1) = the caller compares results of calls with different M / N bit for bit (sharded retrieval): only
 * the LDS-ring kernels, whose K order is the same for every tile shape, are used; 0 = few-row problems (M <= 128, a small grid) take the
 * few-row kernel (gemm_skinny.h: K split over the waves of a workgroup — a different, equally fp32-class summation order). */
#define ZH_GEMM_FIXED_K_ORDER 1
int zh_gemm_f16x3(const void* A, long lda, long strideA, long planeA, const void* W, long ldw, long strideW, long planeW,
                  void* C, long ldc, long strideC, long planeC, int out_kind, float out_scale,
                  const float* bias, const float* residual, long ldr, long strideR, int res_rows,
                  const void* pos_y, const void* pos_x, long ld_pos, int pos_h, int pos_w, int pos_f16,
                  int act, int M, int N, int K, int batch, int flags, zh_stream_t stream);

/* Flash attention: O = softmax(scale * Q K^T) V per (image, head); Q [Tq, heads*dh] rows with stride ldq, etc.
 * f16 in/out, fp32 softmax/accumulate; head_dim in {64, 96, 128} (128: the ViT-L towers' decoder, 8 heads over width 1024).
 * planeQ / planeK / planeV != 0 (all or none): Q, K, V are split pairs; scores are Kh.Qh + Kl.Qh + Kh.Ql and the
 * probabilities are split in registers, O += Vh.Ph + Vl.Ph + Vh.Pl (fp32-class).  planeO != 0: O is written as a split pair.
 * Replaces nn.MultiheadAttention core at clip_arch.py:314-316, transformer.py:272-286,
 * selfmask/vision_transformer.py:110-133 (which materialises [B,heads,T,T]). */
/* The same attention with the KEYS split over `ksplit` (2..64) workgroups per (image, head, 128-query block) and one merge launch:
 * for few queries against many keys (the decoder's cross-attention, transformer.py:281-286: 100 queries x 1764 keys).  Partials
 * (unnormalised fp32 O, running max, row sum) go through `workspace` (zh_attention_splitk_workspace_size bytes, 16-byte aligned). */
/* Tiling of the attention kernels (static_asserts hold the kernels to these): queries per workgroup, keys per tile of the fp16 and of the
 * split-pair kernels.  A key split's chunks are whole tiles. */
#define ZH_ATTN_QUERY_BLOCK 128
#define ZH_ATTN_KEY_TILE_F16 64
#define ZH_ATTN_KEY_TILE_X3 32
size_t zh_attention_splitk_workspace_size(int batch, int heads, int Tq, int head_dim, int ksplit);
int zh_attention_f16_splitk(const void* Q, long ldq, long strideQ, const void* K, long ldk, long strideK,
                            const void* V, long ldv, long strideV, void* O, long ldo, long strideO,
                            int batch, int heads, int Tq, int Tk, int head_dim, float scale,
                            long planeQ, long planeK, long planeV, long planeO, int ksplit, void* workspace, size_t workspace_bytes,
                            zh_stream_t stream);
int zh_attention_f16(const void* Q, long ldq, long strideQ, const void* K, long ldk, long strideK,
                     const void* V, long ldv, long strideV, void* O, long ldo, long strideO,
                     int batch, int heads, int Tq, int Tk, int head_dim, float scale,
                     long planeQ, long planeK, long planeV, long planeO, zh_stream_t stream);

/* The same under CLIP's causal mask (build_attention_mask, clip_arch.py:525-531: -inf above the diagonal), Tq = Tk = T:
 * the text tower's resblocks (clip_arch.py:534-541). */
int zh_attention_causal_f16(const void* Q, long ldq, long strideQ, const void* K, long ldk, long strideK,
                            const void* V, long ldv, long strideV, void* O, long ldo, long strideO,
                            int batch, int heads, int T, int head_dim, float scale,
                            long planeQ, long planeK, long planeV, long planeO, zh_stream_t stream);

/* DEVELOPER entry: what the attention launcher (csrc/attention_dispatch.h) decides for a call, without launching; it is the function the
 * three entries above ask.  The arguments are theirs without scale and stream: causal = 1 for zh_attention_causal_f16 (Tq = Tk = T),
 * ksplit <= 1 with workspace NULL / 0 for the unsplit entries.  Pointers are VALUES (null and alignment checks only): nothing is
 * dereferenced, it runs without a GPU.  Returns what the entry's argument checks return, zh_last_error() included.
 * plan (HOST int[10]) = {variant (0 fp16, 1 split pair, 2 split pair with the software-pipelined loop: head_dim 64 / 96 only), key tile, query blocks per
 * (image, head), workgroups with work (batch * heads * query blocks * ksplit), grid (those rounded up to 8), pipelined loop (0 / 1),
 * ksplit as launched (1 = none), keys per chunk (0 = no split), workspace bytes needed (0 = no split), grid of the merge launch (0 = none)}. */
int zh_dev_attention_plan(const void* Q, long ldq, long strideQ, const void* K, long ldk, long strideK,
                          const void* V, long ldv, long strideV, const void* O, long ldo, long strideO,
                          int batch, int heads, int Tq, int Tk, int head_dim, int causal,
                          long planeQ, long planeK, long planeV, long planeO, int ksplit, const void* workspace, size_t workspace_bytes,
                          int* plan);

/* Text tower glue.  x = token_embedding(text) + positional_embedding (clip_arch.py:535-537): tokens int64 [n,ctx],
 * table f32 [vocab,D], pos f32 [ctx,D] -> out f32 [n*ctx, D]. */
int zh_embed_tokens_f32(const long long* tokens, const float* table, const float* pos, float* out, long n, int ctx, int D,
                        int vocab, zh_stream_t stream);
/* x[arange(n), text.argmax(-1)] (clip_arch.py:545): x f32 [n*ctx, D] -> out f32 [n, D]; first maximum on ties. */
int zh_eot_rows_f32(const long long* tokens, const float* x, float* out, long n, int ctx, int D, zh_stream_t stream);
/* Prompt ensembling tail (utils/extract_text_embeddings.py:110-112): x f32 [groups,T,E] unit-norm rows ->
 * out[g] = mean_t x[g,t] / ||mean_t x[g,t]||. */
int zh_group_mean_l2norm(const float* x, float* out, int groups, int T, int E, zh_stream_t stream);

/* Row LayerNorm (biased variance, eps inside sqrt): clip_arch.py:286-292, transformer.py:249-251, 140-150.
 * in_row(r) = (r / in_group_rows)*in_group_stride + in_offset + r % in_group_rows   (drops the cls token for ln_post,
 * clip_arch.py:403-404); out_row(r) uses the same form (stacks decoder layers as [B,L,Q,D], transformer.py:140-150).
 * Outputs (any may be NULL): y f32, y f16, (y + add[r % add_rows]) f16 / f32
 * (query_pos add, transformer.py:268,277). gamma/beta both NULL => no affine. */
int zh_layernorm_f32(const float* x, long in_group_rows, long in_group_stride, long in_offset,
                     long out_group_rows, long out_group_stride, long out_offset,
                     const float* gamma, const float* beta, float eps,
                     float* out_f32, void* out_f16, void* out_f16_plus, float* out_f32_plus,
                     const float* add, int add_rows, int rows, int D, long lo_plane, int* status, zh_stream_t stream);
/* The same LayerNorm of an fp16 input x (the half-precision residual stream; CLIP's LayerNorm subclass widens an fp16 input to fp32
 * and back, clip_arch.py:286-292): statistics, affine and every output formed in fp32.  x 16-byte aligned, D % 8 == 0, lo_plane % 8 == 0. */
int zh_layernorm_f16(const void* x, long in_group_rows, long in_group_stride, long in_offset,
                     long out_group_rows, long out_group_stride, long out_offset,
                     const float* gamma, const float* beta, float eps,
                     float* out_f32, void* out_f16, void* out_f16_plus, float* out_f32_plus,
                     const float* add, int add_rows, int rows, int D, long lo_plane, int* status, zh_stream_t stream);
/* status (here, zh_layernorm_f16, zh_sum_layernorm_f32, zh_global_ln_l2; may be NULL): a device word into which ZH_STATUS_NONFINITE (2) is OR-ed when a row's
 * variance is inf / NaN.  The split-pair (f16x3) operands of this library hold |x| < 65504: beyond it hi = inf and every later product is
 * a NaN that reaches the next LayerNorm of the path — checking there costs one compare per row.  The host reads the word once per
 * forward (at its next synchronisation) and raises; bit 0 of the same word is zh_instance_mask_stats' range flag. */
#define ZH_STATUS_RANGE 1
#define ZH_STATUS_NONFINITE 2
#define ZH_STATUS_LABEL 4 /* zh_upsample_ce_fwd: a label that is neither < n_cat nor ignore_index (never used as an index) */

/* Split-K combine + bias + residual + LayerNorm (+ a second, chained LayerNorm) in one pass over each row (round 4):
 *   x = ((parts[0] + ... + parts[n_parts-1]) + bias) + residual      parts f32 [n_parts][rows, D] at part_stride, in plane order
 *   out_sum[r] = x                                                  (may alias residual: `x = x + attn(...)`, clip_arch.py:318-321)
 *   y = LN(x; gamma, beta, eps)   -> out_f32 / out_f16 at out_row(r) = (r / out_group_rows) * out_group_stride + out_offset + r % out_group_rows,
 *                                    not written for r % out_group_rows == 0 when skip_first_in_group (ln_post drops cls, clip_arch.py:403-404)
 *   z = LN(y; gamma2, beta2, eps2) -> out2_* at out2_row(r)         (norm3 -> decoder.norm, transformer.py:140-150,291)
 * Replaces the fp32 epilogue of the N = D GEMMs whose K was split over workgroups (zh_gemm_f16x3 with batch = S over K slabs) and the
 * LayerNorm launch that followed them.  gamma NULL: only out_sum.  Any output may be NULL. */
int zh_sum_layernorm_f32(const float* parts, int n_parts, long part_stride, const float* bias, const float* residual,
                         float* out_sum, const float* gamma, const float* beta, float eps,
                         float* out_f32, void* out_f16, long lo_plane,
                         long out_group_rows, long out_group_stride, long out_offset, int skip_first_in_group,
                         const float* gamma2, const float* beta2, float eps2, float* out2_f32, void* out2_f16, long lo_plane2,
                         long out2_group_rows, long out2_group_stride, long out2_offset,
                         int rows, int D, int* status, zh_stream_t stream);

/* cat(class_embedding, patch_emb) + pos_embed, then ln_pre: clip_arch.py:384-397.  out [B,T,D] f32.
 * gamma = beta = NULL: no LayerNorm (DINO ViT prepare_tokens, selfmask/vision_transformer.py:269-281). */
int zh_assemble_tokens_ln(const float* patch_emb, const float* class_embedding, const float* pos_embed,
                          const float* gamma, const float* beta, float eps, float* out,
                          int B, int T, int D, zh_stream_t stream);

/* The same with out f16 [B,T,D]: the half-precision residual stream after ln_pre (clip_arch.py:384-397 in the fp16 tower of
 * utils/extract_image_embeddings.py:43,72-73), rounded once from the fp32 LayerNorm result. */
int zh_assemble_tokens_ln_f16(const float* patch_emb, const float* class_embedding, const float* pos_embed,
                              const float* gamma, const float* beta, float eps, void* out,
                              int B, int T, int D, zh_stream_t stream);

/* x / (||x||_2 + eps) per row: queries (eps = 0) zutis.py:515; averaged tokens (eps = 1e-7) zutis.py:413. */
int zh_l2norm_rows(const float* x, float* out_f32, void* out_f16, float eps, int rows, int D, long lo_plane, float f16_scale, zh_stream_t stream);
/* f16_scale (zh_l2norm_rows, zh_global_ln_l2, zh_cast_f32_f16; a power of two, 1 = none): the fp16 / split-pair copy holds y * f16_scale; its
 * consumer multiplies its accumulator by 1 / f16_scale (zh_gemm_f16x3 out_scale).  Unit-norm rows (|y| ~ 0.04) are stored times 2^10 so that
 * the lo half of the pair is a normal fp16 number (22 significant bits instead of ~19); fp32 outputs are never scaled. */

/* F.layer_norm over the whole (h,w,c) volume per image (no affine) then x/(||x||_c + l2_eps): zutis.py:320-322. */
size_t zh_global_ln_l2_workspace_size(int B, int M, int C);
int zh_global_ln_l2(const float* x, float* out_f32, void* out_f16, float eps, float l2_eps,
                    int B, int M, int C, void* workspace, size_t workspace_bytes, long lo_plane, float f16_scale, int* status,
                    zh_stream_t stream);

/* im2col of the stride==kernel patch conv (pure re-index): clip_arch.py:340,378; selfmask/vision_transformer.py:182.
 * out f16 [B*gh*gw, Kpad], k = c*p*p + i*p + j, zero padded.  pad_to_patch = 0: gh = floor((H-p)/p)+1 (CLIP, trailing
 * pixels dropped); 1: gh = ceil(H/p) with zero pixels (make_input_divisible, selfmask/vision_transformer.py:260-267). */
int zh_im2col_f16(const float* x, void* out, int B, int Cin, int H, int W, int patch, int Kpad, int pad_to_patch,
                  long lo_plane, zh_stream_t stream);

/* Bicubic positional-embedding resample: clip_arch.py:356-374 (scale = float(1/((h+0.1)/g))) and
 * selfmask/vision_transformer.py:377-401 (scale = g/h).  pos [has_cls + g*g, D] -> out [has_cls + h*w, D]. */
int zh_posembed_bicubic(const float* pos, float* out, int grid, int h, int w, int D, float scale_h, float scale_w,
                        int has_cls, zh_stream_t stream);

/* F.interpolate(scale_factor=2, bilinear) on channels-last tokens: zutis.py:491-495.  relu != 0: max(., 0) after the
 * interpolation — the engine applies the (linear) first ffn1 layer and the text-space projection to the h*w tokens and
 * upsamples their outputs (a linear map commutes with the interpolation, whose weights sum to 1), zutis.py:491-503,319. */
int zh_upsample2x_bilinear_cl(const float* x, float* out_f32, void* out_f16, int B, int h, int w, int D, long lo_plane,
                              int relu, zh_stream_t stream);

/* PositionEmbeddingSine(normalize=True): positional_embedding.py:29-52 -> [h*w, D] channels-last. */
int zh_sine_pe(float* out, int h, int w, int D, float temperature, zh_stream_t stream);

/* memory + pos (transformer.py:281): out f16 = a f16 + add f32[r % add_rows].  a_lo_plane != 0: a is a split pair. */
int zh_add_rowperiodic_f16(const void* a, const float* add, void* out, long rows, int D, int add_rows, long a_lo_plane,
                           long lo_plane, zh_stream_t stream);

/* x[i] = value (tgt = zeros_like(queries), zutis.py:164) — a kernel so that it can be part of a launch plan. */
int zh_fill_f32(float* x, float value, long n, zh_stream_t stream);

/* f32 -> f16 (optionally + add[r % add_rows]). */
int zh_cast_f32_f16(const float* x, const float* add, int add_rows, void* out, long rows, int D, long lo_plane, float f16_scale,
                    zh_stream_t stream);

/* argmax_c(F.interpolate(logits, size=(H,W), bilinear)) fused, bit-identical to ATen incl. ties: zutis.py:366-372.
 * logits_lo f32 [B,n,h,w] -> labels int64 [B,H,W].  scale_* = float32(in)/float32(out) computed by the host. */
int zh_upsample_argmax(const float* logits_lo, long long* labels, int B, int n, int h, int w, int H, int W,
                       float scale_h, float scale_w, zh_stream_t stream);

/* zh_upsample_argmax with RunningScore._fast_hist as its epilogue: zutis.py:366-372 + utils/running_score.py:11-16 in one launch.
 * hist_accum int64 [n*n]: hist_accum[n*g + p] += 1 for every pixel whose ground truth g is below n (255 / 1000 are dropped, as
 * _fast_hist masks them), p being exactly the label zh_upsample_argmax gives the pixel.  gt u8: ZH_GT_U8 [B,H,W], g = the byte;
 * ZH_GT_RG16 [B,H,W,3] interleaved, g = R + 256 * G (datasets/imagenet_s.py:93).  labels: NULL, or int64 [B,H,W] that receives
 * the label map as well, bit for bit zh_upsample_argmax's.  n <= 46340 (as zh_confusion_hist).  Equal (g, p) pairs are merged
 * inside a wave: one 64-bit integer atomic per distinct pair per wave (after 8 distinct pairs the lanes left add their own 1):
 * exact, order-independent. */
#define ZH_GT_U8 0
#define ZH_GT_RG16 1
int zh_upsample_argmax_score(const float* logits_lo, const unsigned char* gt, int gt_format, long long* hist_accum,
                             long long* labels, int B, int n, int h, int w, int H, int W, float scale_h, float scale_w,
                             zh_stream_t stream);

/* zh_upsample_argmax with the label leaving as the bytes of the file it becomes: zutis.py:366-372 in the two formats
 * zh_upsample_argmax_score reads — datasets/imagenet_s.py:93 read backwards.  The label of a pixel is exactly zh_upsample_argmax's.
 * labels_out u8, or NULL: ZH_GT_U8 [B,H,W], the byte is the label (n <= 256); ZH_GT_RG16 [B,H,W,3] interleaved, R = label & 255,
 * G = label >> 8, B = 0 (n <= 65536).  overlay_out u8 [B,H,W,3], or NULL (not both): the colour picture over the decoded image,
 * out[p][c] = (img[p][c] * (256 - alpha) + palette[label][c] * alpha + 128) >> 8 in integers, alpha in 0..256 (256: the pure palette
 * colour, 0: the image).  palette u8 [n,3].  img is image b of a staging buffer as zh_resize_normalize_u8 takes it: HWC u8 at
 * packed + 16 * desc[8 b], of size W x H — desc int32 [B, 8] rows (offset / 16, w, h, ...).  packed and desc are NOT checked here
 * (every row's (w, h) must be (W, H) and lie inside packed: the caller's duty); they are read only with an overlay. */
int zh_upsample_argmax_bytes(const float* logits_lo, unsigned char* labels_out, int label_format, unsigned char* overlay_out,
                             const unsigned char* packed, const int* desc, const unsigned char* palette, int alpha,
                             int B, int n, int h, int w, int H, int W, float scale_h, float scale_w, zh_stream_t stream);

/* F.interpolate(x, size, bilinear) on `planes` NCHW planes (return_logits zutis.py:368-371; masks zutis.py:422-423);
 * optional mask_u8 = value > threshold. */
int zh_upsample_bilinear_nchw(const float* x, float* out, unsigned char* mask_u8, float threshold, long planes,
                              int h, int w, int H, int W, float scale_h, float scale_w, zh_stream_t stream);

/* SelfMask inference tail, selfmask.py:207-221: per image the query with the largest objectness logit (first maximum),
 * its mask plane [h,w] bilinearly resampled (scale_* as for zh_upsample_bilinear_nchw; H,W = cropped output) and
 * thresholded -> out_u8 [B,H,W], index int64 [B].  objectness f32 [B,Q] (logits), masks f32 [B,Q,h,w]. */
int zh_select_upsample_mask(const float* objectness, const float* masks, unsigned char* out_u8, long long* index, int B, int Q,
                            int h, int w, int H, int W, float scale_h, float scale_w, float threshold, zh_stream_t stream);

/* F.interpolate(mask[None,None], size=(H,W), mode="nearest") on a u8 mask: datasets/index_dataset.py:215
 * (restore the original resolution of a pseudo-mask).  scale_* = float32(in)/float32(out). */
int zh_resize_nearest_u8(const unsigned char* x, unsigned char* out, int h, int w, int H, int W, float scale_h, float scale_w,
                         zh_stream_t stream);

/* RunningScore._fast_hist: utils/running_score.py:11-16.  hist_accum int64 [n*n] += bincount(n*gt+pred), 0<=gt<n. */
int zh_confusion_hist(const long long* label_true, const long long* label_pred, long long* hist_accum, long total,
                      int n_class, zh_stream_t stream);

/* ---- instance prediction, zutis.py:374-420 ---- */
/* binary = p > threshold; size = sum(binary); confidence = sum(p*binary)/(size+1e-7)   (zutis.py:390-397).
 * mask_proposals f32: image b at + b*stride_image, [Q, M] contiguous inside (last decoder layer slice). */
int zh_instance_mask_stats(const float* mask_proposals, long stride_image, float threshold, int B, int Q, int M,
                           float* sizes, float* confidence, unsigned char* binary, int* range_flag, zh_stream_t stream);
/* range_flag (may be NULL; zero it first): bit 0 is OR-ed in when a proposal is outside [0, 1] or a NaN — the reference's range asserts
 * (zutis.py:385-386) without a reduction and a device -> host copy of their own. */
/* avg[b,q,:] = sum_m binary[b,q,m]*tokens[b,m,:] / (size+1e-7)  (zutis.py:404-406; the reference materialises
 * B x Q x hw x E).  Pixels are processed in chunks of 128 by separate workgroups; per-chunk partial sums go through `workspace`
 * (zh_masked_mean_workspace_size bytes) and are added in chunk order. */
size_t zh_masked_mean_workspace_size(int B, int Q, int M, int E);
int zh_masked_mean_tokens(const float* tokens, const unsigned char* binary, const float* sizes, float* avg,
                          int B, int Q, int M, int E, void* workspace, size_t workspace_bytes, zh_stream_t stream);
/* category = argmax_n sigmoid(T * text_n . avg/(||avg||+1e-7)); score = confidence * max  (zutis.py:409-420). */
int zh_instance_classify(const float* avg, const float* text, const float* confidence, float temperature,
                         int rows, int n_classes, int E, long long* category, float* score, zh_stream_t stream);
/* pairwise |a&b|, |a|b| of n {0,1} u8 masks (bit-packed popcount): utils/iou.py:6-37 inside the NMS loop
 * zutis.py:245-278. */
size_t zh_mask_iou_workspace_size(int n, long pixels);
int zh_mask_iou_counts(const unsigned char* masks, int n, long pixels, int* inter, int* uni,
                       void* workspace, size_t workspace_bytes, zh_stream_t stream);

/* ---- CLIP image pre-processing for embedding extraction ---- */
/* Resize(n_px, BICUBIC) + CenterCrop(n_px) + ToTensor + Normalize of SimpleDataset, utils/extract_image_embeddings.py:97-103, for
 * B decoded RGB images of DIFFERENT sizes in one launch, bit-identical to Pillow's 8-bit resampler (two separable integer passes
 * with 22-bit coefficients, u8 intermediate) followed by NumPy's fp32 (v / 255 - mean) / std.
 * packed u8: the images back to back, each [h, w, 3] at a 16-byte-aligned offset, packed_bytes in all (reads are checked against
 * it).  desc int32 [B, 8]: offset / 16, w, h, resized nw, nh, crop left, top, 0 — the host computes torchvision's roundings.
 * lut f32 [3, 256]: the normalised value of byte v in channel c, filled on the host.  out f32 [B, 3, n_px, n_px].
 * kmax: an upper bound of the taps per output pixel over the batch, ceil(2 * max(in / out, 1)) * 2 + 1 on either axis, at most
 * ZH_RCN_KMAX (it sizes the launch's LDS; 7 for a 500 x 375 photograph at 336).  An image whose descriptor does not fit (more taps than kmax,
 * bytes outside packed, crop outside the resized image) gets NaN in its whole output and is not read. */
#define ZH_RCN_KMAX 152
int zh_resize_crop_normalize_u8(const unsigned char* packed, long packed_bytes, const int* desc, int B, int n_px, int kmax,
                                const float* lut, float* out, zh_stream_t stream);
/* MaskDataset's transform, datasets/index_dataset.py:405-411 — TF.resize(image, image_size, BILINEAR) + to_tensor + normalize — for B
 * decoded RGB images of different sizes that all resize to ONE out_w x out_h, in one launch and with no crop: the same two-pass
 * 8-bit resampler with Pillow's filter `filter` (ZH_FILTER_BILINEAR: the triangle 1 - |x| of support 1, taps per output pixel
 * ceil(max(in / out, 1)) * 2 + 1; ZH_FILTER_BICUBIC: as above), bit-identical to Image.resize((out_w, out_h), filter) followed by
 * the fp32 (v / 255 - mean) / std.  packed, desc, lut, kmax as for zh_resize_crop_normalize_u8 (kmax >= 3 for bilinear); a pass whose
 * size does not change has identity coefficients (Pillow skips it).  out f32 [B, 3, out_h, out_w].  A descriptor whose
 * (nw, nh, left, top) is not (out_w, out_h, 0, 0), or that does not fit as above, gets NaN and is not read. */
#define ZH_FILTER_BILINEAR 2 /* PIL.Image.BILINEAR */
#define ZH_FILTER_BICUBIC 3  /* PIL.Image.BICUBIC */
int zh_resize_normalize_u8(const unsigned char* packed, long packed_bytes, const int* desc, int B, int out_h, int out_w, int filter,
                           int kmax, const float* lut, float* out, zh_stream_t stream);

/* ---- bilateral solver (SelfMask refinement), utils/bilateral_solver.py:40-195; float64 ---- */
/* convert_tensor_to_pil_image, utils/utils.py:261-273: fp32 x*std+mean, *255, clip, TRUNCATE.  x f32 [3,H,W] (device)
 * -> rgb u8 [H,W,3] (device).  mean3/std3 are HOST float[3]. */
int zh_denormalize_u8(const float* x, unsigned char* rgb, int H, int W, const float* mean3, const float* std3,
                      zh_stream_t stream);
/* per-pixel lattice coordinates (x/ss, y/ss, Y/sl, U/sc, V/sc), bilateral_solver.py:42-50 -> int32 [H*W,5] (parity probe). */
int zh_bgrid_coords(const unsigned char* rgb, int H, int W, double sigma_spatial, double sigma_luma, double sigma_chroma,
                    int* coords, zh_stream_t stream);
/* BilateralGrid + bistochastize + BilateralSolver.solve for one channel: bilateral_solver.py:58-149 with the
 * constants of bilateral_solver_output (:162-175: confidence 0.999, lam 256, A_diag_min 1e-5, cg_tol 1e-5, maxiter 25)
 * passed by the caller.  rgb u8 [H,W,3]; target u8 [H,W] or f64 [H,W] (exactly one non-NULL); out_soft f64 [H,W];
 * stats int32 [2] = {nvertices, cg iterations} (device, may be NULL); n_out/m_out f64 [H*W] debug copies of the
 * bistochastisation vectors (may be NULL).  The device lattice is dense; it matches the reference's, whose vertex hash is
 * sum c_d 255^d, only while every lattice coordinate stays below 255 (sigmas of about 1 or more, at most 254 spatial cells a side). */
size_t zh_bilateral_workspace_size(int H, int W, double sigma_spatial, double sigma_luma, double sigma_chroma);
int zh_bilateral_solve(const unsigned char* rgb, const unsigned char* target_u8, const double* target_f64, int H, int W,
                       double sigma_spatial, double sigma_luma, double sigma_chroma, double confidence, double lam,
                       double a_diag_min, double cg_tol, int cg_maxiter, double* out_soft, int* stats,
                       double* n_out, double* m_out, void* workspace, size_t workspace_bytes, zh_stream_t stream);

/* The same for B images of one size in ONE sequence of launches (blockIdx.y = image): rgb u8 [B,H,W,3], target [B,H,W],
 * out_soft f64 [B,H,W], stats int32 [B,2], n_out / m_out f64 [B,H*W]; workspace = B * zh_bilateral_workspace_size(...) bytes.
 * A solve is ~110 small launches (grid build, 11 bistochastisation steps, 3 per CG iteration): batching shares them —
 * the pseudo-label driver's batched mode (datasets/index_dataset.py:189-204 runs batch 1). */
int zh_bilateral_solve_batch(const unsigned char* rgb, const unsigned char* target_u8, const double* target_f64, int B, int H, int W,
                             double sigma_spatial, double sigma_luma, double sigma_chroma, double confidence, double lam,
                             double a_diag_min, double cg_tol, int cg_maxiter, double* out_soft, int* stats,
                             double* n_out, double* m_out, void* workspace, size_t workspace_bytes, zh_stream_t stream);

/* output_solver > 0.5 on the device (networks/selfmask/selfmask.py:231): x f64 [n] -> out u8 {0,1} [n]. */
int zh_threshold_f64_u8(const double* x, double threshold, unsigned char* out, long n, zh_stream_t stream);

/* The post-processing of bilateral_solver_output, utils/bilateral_solver.py:185-193, for B images of one size in ONE fixed sequence of
 * launches (blockIdx.y = image; nothing is read back, so the entry is stream-ordered and capturable): binary_fill_holes(soft > 0.5),
 * ndimage.label (4-connected), a count per label with the background as label 0, and the label that is SECOND largest under the key
 * (count, label) = np.argsort(counts, kind="stable")[-2]; all ones when there is no object.  The reference's plain np.argsort is not
 * stable: where the largest or the second-largest count is not unique its answer is implementation-defined, and this rule is the one
 * kept (zutis_amd/components.py).  Everywhere else the outputs are scipy's, bit for bit.
 * Exactly one of soft (f64 [B,H,W]; foreground = soft > threshold, a NaN is background) and binary (u8 [B,H,W]; foreground = non-zero)
 * is non-NULL.  mask_out u8 {0,1} [B,H,W]; filled_out u8 {0,1} [B,H,W] (the filled foreground) and labels_out int32 [B,H,W] (scipy's
 * numbering: 1 .. nr in raster order of each component's first pixel, 0 = background) may be NULL; stats int32 [B,4] = {nr_objects,
 * chosen label, chosen count, 1 if the all-ones fallback was taken (then label -1, count H*W)}.  workspace: B *
 * zh_components_workspace_size(H, W) bytes, 4-byte aligned (ZH_ERR_WORKSPACE when short; nothing is written then); up to (H*W + 1) / 2
 * components, H = 1 and W = 1 included, H*W <= 2^31 - 1.  Tiles of ZH_CCL_TILE_H x ZH_CCL_TILE_W pixels are labelled in LDS and merged
 * across their borders in global memory (csrc/components.hip). */
#define ZH_CCL_TILE_H 32
#define ZH_CCL_TILE_W 32
size_t zh_components_workspace_size(int H, int W); /* per image */
int zh_second_largest_component(const double* soft, const unsigned char* binary, double threshold, int B, int H, int W,
                                unsigned char* mask_out, unsigned char* filled_out, int* labels_out, int* stats, void* workspace,
                                size_t workspace_bytes, zh_stream_t stream);

/* Retrieval (datasets/index_dataset.py:163-167): per row of scores [rows, N] (row stride ld) the k largest entries, score
 * descending, ties by ascending index — replaces torch.argsort(descending=True)[:n_images] per category.  NaNs of either
 * sign and any payload come first (in index order) and -0.0 ties with +0.0, as torch.sort(descending=True, stable=True)
 * orders them; val_out returns the stored bits.
 * idx_out int64 [rows,k]; val_out f32 [rows,k] or NULL.  k <= 1024.  The index reported for column i is
 * idx_map[row*ld + i] when idx_map != NULL (merging candidate lists that carry global image indices), else i + idx_add
 * (chunk offset); ties are broken by ascending column.  Output rows have stride out_ld >= k. */
int zh_topk_rows(const float* scores, long ld, int rows, long N, int k, const long long* idx_map, long long idx_add,
                 long long* idx_out, float* val_out, long out_ld, zh_stream_t stream);

/* Greedy per-category mask NMS on the device: networks/zutis.py:211-299 (copy: coco20k_eval.py:54-136).  inter / uni int32
 * [B,Q,Q] from zh_mask_iou_counts (IoU = inter / (uni + 1e-7) in float64 = utils/iou.py:30-32), scores f32 [B,Q], category_ids
 * int64 [B,Q].  nms_type 0 hard | 1 linear | 2 gaussian; the reference's constants are nms_threshold 0.3, sigma 0.5,
 * score_threshold 0.001.  Output per image, in the reference's emission order (category ascending, 0 skipped, then selection
 * order; empty masks skipped): out_index int32 [B,Q], out_score f64 [B,Q], out_category int64 [B,Q], out_count int32 [B]. */
int zh_mask_nms(const int* inter, const int* uni, const float* scores, const long long* category_ids, int B, int Q,
                int nms_type, double nms_threshold, double sigma, double score_threshold,
                int* out_index, double* out_score, long long* out_category, int* out_count, double* packed, const int* range_flag,
                int* zero_word, zh_stream_t stream);
/* packed (may be NULL): f64 [B, 4Q + 2] = per image [out_index (-1 past the count) | out_score | out_category | category_ids | count,
 * *range_flag] — everything the host needs in one device -> host copy.  zero_word (may be NULL): one int32 the kernel sets to 0 — the
 * cursor of the zh_mask_rle_fused_kept launched behind it (saves the caller a fill launch). */

/* Device-side run extraction for COCO RLE + boxes + areas of selected masks (masks u8 [n,H,W] row-major; sel int32
 * [n_sel] mask indices): positions int32 [n_sel, max_runs] = column-major pixel indices where the value changes;
 * nruns int32 [n_sel,2] = {#transitions, value of pixel 0}; box_area int32 [n_sel,5] = {xmin,ymin,xmax,ymax,area}.
 * Replaces the mask D2H in front of pycocotools.mask.encode / masks_to_boxes, zutis.py:288-294,446-452. */
size_t zh_mask_runs_workspace_size(int n, int W);   /* n = n_sel (zh_mask_runs) or B * Q (zh_mask_runs_kept): per-panel counts / boxes */
int zh_mask_runs(const unsigned char* masks, const int* sel, int n_sel, int H, int W, int max_runs,
                 int* positions, int* nruns, int* box_area, void* workspace, size_t workspace_bytes, zh_stream_t stream);
/* The same for the queries zh_mask_nms kept, straight from its device outputs (masks u8 [B,Q,H,W]; kept_index int32 [B,Q], kept_count
 * int32 [B]): row b*Q + j of positions / nruns / box_area describes image b's j-th kept mask; rows j >= kept_count[b] are not written.
 * packed_capacity = 0: positions int32 [B*Q, max_runs] as above.  packed_capacity > 0: positions is ONE list of packed_capacity ints —
 * the kept masks' transitions back to back (image-major, kept order; a mask contributes min(#transitions, max_runs) entries, so the
 * host finds every list from nruns alone); entries that would fall past the capacity are not written (the host sees that from the
 * same counts and asks again).  A short head of such a list travels in the same device -> host copy as the small tables. */
int zh_mask_runs_kept(const unsigned char* masks, const int* kept_index, const int* kept_count, int B, int Q, int H, int W, int max_runs,
                      int* positions, long packed_capacity, int* nruns, int* box_area, void* workspace, size_t workspace_bytes,
                      zh_stream_t stream);

/* COCO RLE strings of the kept masks on the device (= pycocotools.mask.encode(...)["counts"], zutis.py:290,448) from zh_mask_runs_kept's
 * PACKED list and nruns table: mask b*Q + j (j < kept_count[b]) gets its string at out + 5 * off + 16 * rank, off = start of its list in
 * `positions` (sum of min(transitions, max_runs) over the kept masks in front of it), rank = number of kept masks in front of it;
 * out_len int32 [B*Q] = the string's length, -1 when the mask has more than max_runs transitions or its list / string does not fit the
 * capacities (the caller encodes that mask from its pixels).  HW = pixels per mask.  A mask's string is never written outside
 * [5 * off + 16 * rank, min(that + 5 * transitions + 16, out_capacity)): for HW < 2^24 a string of nc = transitions + 1 + (pixel 0 set)
 * values is at most 5 * nc characters and `out` is checked for those; for 2^24 <= HW < 2^31, where a value can take 6 or 7 characters,
 * the string is measured first and reported -1, with no character written, when it does not fit that window. */
int zh_mask_rle_kept(const int* positions, long packed_capacity, const int* nruns, const int* kept_count, int B, int Q, int max_runs, long HW,
                     unsigned char* out, long out_capacity, int* out_len, zh_stream_t stream);

/* Runs + box + area + RLE string of the kept masks in ONE launch (one workgroup per kept mask, the mask held as bits in LDS): what
 * zh_mask_runs_kept + zh_mask_rle_kept produce, for masks with W <= 1024 whose bits (H*W/8 bytes), count table and run list
 * (4 * max_runs bytes) fit 150 KB of LDS (zh_mask_rle_fused_supported).  bits (may be NULL: the bytes of `masks` are packed instead) =
 * the masks bit-packed as zh_mask_iou_counts leaves them in its workspace: u64 [B*Q][(H*W + 63) / 64], bit i of word w = pixel 64 w + i
 * (row-major) is non-zero.  info int32 [B*Q, 8] = {offset of the string in `out`, its length (-1: not encoded — more than max_runs
 * transitions, or `out` is full: the caller uses zh_mask_runs for that mask), xmin, ymin, xmax, ymax, area, transitions}; rows of slots
 * j >= kept_count[b] are not written.  cursor: ONE int32 the caller has zeroed; strings are placed in order of arrival. */
int zh_mask_rle_fused_supported(int H, int W, int max_runs);
int zh_mask_rle_fused_kept(const unsigned char* masks, const unsigned long long* bits, const int* kept_index, const int* kept_count, int B, int Q,
                           int H, int W, int max_runs, unsigned char* out, long out_capacity, int* cursor, int* info, zh_stream_t stream);

/* A picture of the instance predictions, painted behind zh_mask_nms where the masks, the kept list and the decoded image already lie:
 * what utils/visualiser.py:154-187 (trainer.py:368-372, coco20k_eval.py:271-276) asks detectron2 for, as an id map and / or a colour
 * overlay.  Masks: bits (u64 [B*Q][(H*W + 63) / 64] as zh_mask_iou_counts leaves them, see zh_mask_rle_fused_kept) when not NULL, else
 * masks u8 [B,Q,H,W] (non-zero = in the mask); both give the same output.  Slot table exactly as zh_mask_nms writes it, consumed from
 * that launch with no host visit: index int32 [B,Q] (slot j of image b shows mask index[b,j]), score f64 [B,Q], count int32 [B];
 * entries past count[b] are never read, a slot whose index is outside [0, Q) is not painted.  colours u8 [B,Q,3], one per SLOT.
 *   painted slots: j < count[b] with score[b,j] > min_score (float64, strict, as convert_to_instances compares, visualiser.py:139);
 *   paint rank:    the painted slots by score descending, ties to the lower slot (ordered on the device);
 *   top(p):        the painted slot of lowest rank whose mask is non-zero at pixel p = y W + x, or none.
 * ids_out (may be NULL): top(p) + 1, 0 for none — ZH_GT_U8 u8 [B,H,W] (Q <= 255, else ZH_ERR_ARG), ZH_GT_RG16 u8 [B,H,W,3] = (id & 255,
 * id >> 8, 0), the convention of the label files (zh_upsample_argmax_bytes).  overlay_out (may be NULL; not both) u8 [B,H,W,3]: the
 * image byte where there is no top; else with c = colours[b, top(p)]: c itself when outline != 0 and a 4-neighbour INSIDE the image has
 * another top (another slot, or none), otherwise (img * (256 - alpha) + c * alpha + 128) >> 8 per channel, alpha in 0..256 — the integers
 * of zh_upsample_argmax_bytes.  Pixels without a top are never outline pixels; the image border alone makes no outline.  img: packed +
 * desc under the contract of zh_upsample_argmax_bytes (NOT checked here; read only with an overlay).  Q <= ZH_PAINT_MAX_Q (the rank table
 * lives in LDS).  workspace >= zh_instance_paint_workspace_size bytes, 16-byte aligned: the rank table and a u16 id per pixel for the outline. */
#define ZH_PAINT_MAX_Q 1024
size_t zh_instance_paint_workspace_size(int B, int Q, int H, int W);
int zh_instance_paint(const unsigned char* masks, const unsigned long long* bits, const int* index, const double* score, const int* count,
                      const unsigned char* colours, int alpha, int outline, double min_score, const unsigned char* packed, const int* desc,
                      unsigned char* ids_out, int id_format, unsigned char* overlay_out, int B, int Q, int H, int W, void* workspace,
                      size_t workspace_bytes, zh_stream_t stream);

/* ---- Training criterion, criterion.py::Criterion (called by Trainer.fit, trainer.py:105-160).  All fp32; the full-resolution
 * proposals, tokens, logits and their gradients are never written: every full-res value is a bilinear sample (ATen size= form,
 * scale_* = float32(in)/float32(out)) of the low-res input, formed where it is reduced.  Sums are blocked and reduced in a fixed
 * order (no float atomics): costs, losses and gradients are bitwise reproducible run to run.
 *
 * Matching costs, criterion.py:97-135 (dice_loss :26-41, binary_cross_entropy_loss :43-61, cost_matrix :131), every (image, layer) in
 * one call.  proposals f32 [B, L, Q, h, w] in [0, 1]; gt_u8 [n_tot, H, W] (non-zero = in the mask): image b's instances are rows
 * inst_off[b] .. inst_off[b+1]-1 (inst_off int32 [B+1], device); n_max = max instances of an image.  Outputs: costs f32 — image b's
 * [L, n_b, Q] block at offset L * inst_off[b] * Q — = weight_dice * dice + weight_bce * bce with
 *   dice = 1 - (2 sum(g p) + 1) / (sum p + sum g + 1),  bce = -sum (g ? A : B) / (H W),  A = max(log p, -100), B = max(log(1-p), -100);
 * stat_p f32 [B, L, Q] (sum p), stat_pg (sum g p, the layout of costs), stat_g f32 [n_tot] (sum g) for zh_mask_match_grad;
 * skip int32 [B] = 1 where an image's GT masks sum to 0 (criterion.py:116-118); ZH_STATUS_RANGE OR-ed into *status when a proposal
 * is outside [0, 1] or NaN (the asserts of criterion.py:71-72).  workspace >= zh_mask_match_cost_workspace_size. */
size_t zh_mask_match_cost_workspace_size(int B, int L, int Q, int H, int n_max);
int zh_mask_match_cost(const float* proposals, const unsigned char* gt_u8, const int* inst_off, float* costs, float* stat_p,
                       float* stat_pg, float* stat_g, int* skip, int* status, int B, int L, int Q, int h, int w, int H, int W,
                       int n_max, float weight_dice, float weight_bce, float scale_h, float scale_w, void* workspace,
                       size_t workspace_bytes, zh_stream_t stream);
/* Backward of the matched costs, criterion.py:136-149 (the autograd of cost_matrix[i, q] through F.interpolate, :124-125).
 * pairs int32 [n_pairs, 4] = (b, l, q, i) with i local to image b, at most one pair per (b, l, q).  grad_proposals f32 [B, L, Q, h, w]
 * is zeroed and each matched plane gets the adjoint upsample of
 *   grad_out[0] * loss_scale * ( weight_dice * -(2 g D - N) / D^2 + weight_bce * (p - g) / max(p (1 - p), 1e-12) / (H W) ),
 * D = sum p + sum g + 1, N = 2 sum(g p) + 1 (stat_* of zh_mask_match_cost); loss_scale = weight_mask_loss / batch_size (:150,152). */
int zh_mask_match_grad(const float* proposals, const unsigned char* gt_u8, const int* inst_off, const int* pairs, int n_pairs,
                       const float* stat_p, const float* stat_pg, const float* stat_g, const float* grad_out, float* grad_proposals,
                       int B, int L, int Q, int h, int w, int H, int W, float weight_dice, float weight_bce, float loss_scale,
                       float scale_h, float scale_w, zh_stream_t stream);
/* Cross-entropy on upsampled logits, criterion.py:77-95: einsum(te, upsample(tok)) = upsample(einsum(te, tok)), so the caller
 * passes the low-res logits f32 [B, n_cat, h, w] (zh_gemm_f32_strided); labels int64 [B, H, W].  lse f32 [B, H, W] (log-sum-exp
 * per pixel, kept for the backward); out f32 [2] = (mean NLL over the pixels whose label != ignore_index — NaN when there is none,
 * as torch —, that count).  A label that is neither in [0, n_cat) nor ignore_index counts as ignored and OR-s ZH_STATUS_LABEL into
 * *status.  workspace >= zh_upsample_ce_workspace_size. */
size_t zh_upsample_ce_workspace_size(int B, int H, int W);
int zh_upsample_ce_fwd(const float* logits_lo, const long long* labels, float* lse, float* out, int* status, int B, int n_cat,
                       int h, int w, int H, int W, int ignore_index, float scale_h, float scale_w, void* workspace,
                       size_t workspace_bytes, zh_stream_t stream);
/* Its backward: grad_logits_lo f32 [B, n_cat, h, w] (fully written) = adjoint upsample of grad_out[0] / out[1] * (softmax - onehot),
 * 0 on ignored pixels (ce_out = the `out` of zh_upsample_ce_fwd). */
int zh_upsample_ce_bwd(const float* logits_lo, const long long* labels, const float* lse, const float* ce_out,
                       const float* grad_out, float* grad_logits_lo, int B, int n_cat, int h, int w, int H, int W,
                       int ignore_index, float scale_h, float scale_w, zh_stream_t stream);
/* C[t](m, n) = sum_k A[t](m, k) B[t](n, k), every operand by element strides (batch, row, k): the low-res text contraction
 * einsum("nc,bchw->bnhw") of criterion.py:88-90 and its transpose for the token gradient.  fp32, fixed k order. */
int zh_gemm_f32_strided(const float* A, long sAb, long sAm, long sAk, const float* Bm, long sBb, long sBn, long sBk, float* C,
                        long sCb, long sCm, long sCn, int batch, int M, int N, int K, zh_stream_t stream);

/* The criterion's assignment on the device: scipy.optimize.linear_sum_assignment(cost_matrix) of criterion.py:133 for every (image,
 * layer) of one call, and the matched costs summed into the mask loss of criterion.py:145,150.  costs / inst_off / skip: exactly what
 * zh_mask_match_cost wrote and read (image b's [L, n_b, Q] float32 block at L * inst_off[b] * Q); n_max = max instances of an image,
 * n_tot = inst_off[B].  One wavefront per problem runs scipy's rectangular shortest-augmenting-path solve (Crouse / Jonker-Volgenant)
 * in float64 with scipy's scan order and tie rule, transposed when n_b > Q: the matches are scipy's, ties included.
 * Outputs: pairs int32 [n_pairs, 4] = (b, l, q, i) in (b, l, i) order (the tensor zh_mask_match_grad reads; 16-byte aligned, room for
 * sum_b L * min(n_b, Q) rows), *n_pairs, *mask_loss = f32(float64 sum of the matched costs in that order / B).  An image with
 * skip[b] != 0 or no instance gives no pairs.  A problem with a non-finite cost gives no pairs and ORs ZH_STATUS_NONFINITE into
 * *status — unlike scipy, which accepts +inf entries, every cost must be finite (zh_mask_match_cost cannot produce a non-finite cost
 * without having set ZH_STATUS_RANGE).  Limit: max(n_max, Q) <= ZH_ASSIGN_MAX_DIM (32 bytes of LDS state per column, 16 per row:
 * 48 KB at the cap; zh_linear_assignment_max_dim() = the value the library was built with), ZH_ERR_ARG above it.
 * workspace >= zh_linear_assignment_workspace_size. */
#define ZH_ASSIGN_MAX_DIM 1024
int zh_linear_assignment_max_dim(void);
size_t zh_linear_assignment_workspace_size(int B, int L, int n_tot);
int zh_linear_assignment(const float* costs, const int* inst_off, const int* skip, int B, int L, int Q, int n_max, int n_tot,
                         int* pairs, int* n_pairs, float* mask_loss, int* status, void* workspace, size_t workspace_bytes,
                         zh_stream_t stream);
/* The ragged ground truth of a criterion call (criterion.py:97-118: one [n_b, H, W] tensor per image) -> gt_u8 [n_tot, H, W]
 * (non-zero -> 1) and inst_off int32 [B + 1] on the device, in one launch per 32 images.  src / counts: HOST arrays [B] of the
 * images' DEVICE source pointers and instance counts — they travel as kernel arguments, so nothing is copied to the device and the
 * entry cannot be part of a launch plan; elem_size 1 (bool, uint8) or 8 (int64); HW = H * W.  An image whose source pointer IS its
 * place in gt_u8 is left as it is (masks that already lie packed in one allocation: only inst_off is written); any other overlap of a
 * source with gt_u8 is undefined.  gt_u8 may be NULL when every count is 0. */
int zh_pack_masks_u8(const void* const* src, const int* counts, int B, int elem_size, long HW, unsigned char* gt_u8, int* inst_off,
                     zh_stream_t stream);

/* ---- COCO mask AP, trainer.py:255-292 / coco20k_eval.py:280-308: what pycocotools' COCOeval.evaluate computes for iouType "segm"
 * (zutis_amd/coco_eval.py; accumulate / summarize stay NumPy float64 on the host: they touch flags and scores only).  A call serves
 * n_masks masks — detections and ground truths alike — as uncompressed run counts (column-major, the run of zeros first, as the RLE
 * strings of zutis.py:290,448 decode): counts int32, mask m's runs at run_off[m] .. run_off[m + 1] - 1 (run_off int32 [n_masks + 1]).
 *
 * zh_rle_prefix (the area and the running sums behind maskApi's rleArea / rleIou): one wave per mask scans its counts into
 * run_end int32 (position where run k ends) and run_fg int32 (foreground pixels in front of run k), both laid out as counts, and
 * area int32 [n_masks].  hw int32 [n_masks] = h * w of each mask: a mask with a negative count, or whose counts do not sum to its
 * h * w, gets bit (m & 31) of status[m >> 5] (int32 [(n_masks + 31) / 32], zeroed by the caller) and area 0, and no later entry
 * reads its runs. */
int zh_rle_prefix(const int* counts, const int* run_off, const int* hw, int n_masks, int* run_end, int* run_fg, int* area, int* status,
                  zh_stream_t stream);
/* IoU of every (detection, ground truth) pair of every group in one launch (COCOeval.computeIoU -> maskUtils.iou -> rleIou), one wave
 * per pair.  groups int32 [n_groups, 8] = {det_off, D, gt_off, G, pair_off, 0, 0, 0}: the group's D detections are the masks
 * det_mask[det_off ..] (score-descending, cut to the largest max-det by the host), its G ground truths gt_mask[gt_off ..] with
 * gt_crowd[gt_off ..] (iscrowd), and its D x G results lie row-major at pair_off (= the sum of D * G over the groups in front: ascending;
 * n_pairs = the total, at most 2^31 - 1).  inter int32 [n_pairs] = pixels in both; iou f64 [n_pairs] = inter / (area_d + area_g - inter),
 * or inter / area_d against a crowd, 0 when inter is 0 (as rleIou): ONE float64 division of integers, bit for bit NumPy's.  A pair with
 * a mask that zh_rle_prefix flagged gets inter -1 and iou -1.  A ground truth of up to ZH_RLE_IOU_LDS_RUNS runs is searched in LDS, a
 * longer one in global memory (zh_rle_iou_lds_runs() = the value the library was built with).  n_pairs = 0 launches nothing. */
#define ZH_RLE_IOU_LDS_RUNS 1024
int zh_rle_iou_lds_runs(void);
int zh_rle_pair_iou(const int* run_end, const int* run_fg, const int* run_off, const int* area, const int* status, const int* groups,
                    int n_groups, const int* det_mask, const int* gt_mask, const int* gt_crowd, long n_pairs, int* inter, double* iou,
                    zh_stream_t stream);
/* COCOeval.evaluateImg for every (group, area range, IoU threshold), one lane each, the T * A <= 64 problems of a group in one wave.
 * iou / groups / det_mask / area / gt_crowd as above (area is read for the detections only: an unmatched detection whose area lies
 * outside the range is ignored); n_gt = length of the ground-truth lists; gt_order / gt_ignore int32 [A, n_gt]: per area range the
 * group's ground truths ignored-last (stable) as indices local to the group, and their ignore flags in that order; thresholds f64 [T];
 * area_ranges f64 [A, 2].  Outputs, with n_det = length of det_mask: match int32 [n_det, A, T] = the matched ground truth's index in
 * its group or -1; ignore u8 [n_det, A, T].  workspace >= zh_coco_match_workspace_size bytes (the lanes' matched flags). */
size_t zh_coco_match_workspace_size(long n_gt, int T, int A);
int zh_coco_match(const double* iou, const int* groups, int n_groups, const int* det_mask, const int* area, const int* gt_order,
                  const int* gt_ignore, const int* gt_crowd, long n_gt, const double* thresholds, int T, const double* area_ranges, int A,
                  int* match, unsigned char* ignore, void* workspace, size_t workspace_bytes, zh_stream_t stream);
/* Polygon annotations to run counts (zutis_amd/polygons.py): pycocotools' annToRLE for polygon segmentations — rleFrPoly per polygon
 * and the union of an annotation's polygons — as zutis_amd/rle.py restates them (_polygon_boundary, _polygon_counts, from_polygons: the
 * definition, count for count), for n_annotations annotations in one launch, one workgroup each.  xs / ys int32: the vertices of all
 * polygons scaled as rleFrPoly scales them, int(5 * v + .5); polygon p's are vert_off[p] .. vert_off[p + 1] - 1 (vert_off int32
 * [n_polygons + 1]) and annotation a's polygons poly_off[a] .. poly_off[a + 1] - 1 (poly_off int32 [n_annotations + 1]); step_pref
 * int32: per polygon the exclusive prefix of its edges' step counts max(|dx|, |dy|) + 1 (the edge from vertex e to the polygon's next
 * one, the last closing it), k + 1 entries at vert_off[p] + p; hw int32 [n_annotations, 2] = (h, w); flags int32 [n_annotations]: non-zero
 * = leave it to the host.  counts int32: annotation a's runs (column-major, the run of zeros first, as zh_rle_prefix reads them) start
 * at out_off[a] (out_off int32 [n_annotations + 1], the slice at least its kept crossings + 1 long); n_runs int32 [n_annotations] = how
 * many, or -1 for an annotation left to the host: flagged, or outside what the workgroup holds in LDS — more than
 * ZH_POLYGON_LDS_CROSSINGS crossings in all its polygons, a polygon of more than half as many vertices or of more than 2^22 walk
 * points (zh_polygon_lds_crossings() = the value the library was built with). */
#define ZH_POLYGON_LDS_CROSSINGS 4096
int zh_polygon_lds_crossings(void);
int zh_polygon_runs(const int* xs, const int* ys, const int* step_pref, const int* vert_off, const int* poly_off, const int* hw,
                    const int* flags, const int* out_off, int n_annotations, int* counts, int* n_runs, zh_stream_t stream);
/* Semantic ground truth from annotations (zutis_amd/annotation_labels.py): the label maps the COCO datasets open at
 * {dir_dataset}/annotations/semantic_segmentation_masks/{stem}.png (datasets/coco2017.py:134, datasets/coco20k.py:178; the labels
 * are the ranks of datasets/coco2017.py:152-244) for B images in one launch.  run_end / run_off / status: n_masks masks exactly as
 * zh_rle_prefix leaves them (n_runs = run_off[n_masks]: the length of run_end).  Image b's paint list is list_mask / list_label
 * [list_off[b] .. list_off[b + 1]) (list_off int32 [B + 1], the lists n_list entries long in all): the index of a mask and the label
 * byte it paints, in paint order; hw int32 [B, 2] = (h, w); image b's map is u8 row-major [h, w] at out + out_off[b] (out_off int64
 * [B + 1]; a same-size batch laid back to back is a [B, H, W] tensor), out_bytes the length of out.  A gather, one lane per pixel of
 * a ZH_LABEL_TILE_W x ZH_LABEL_TILE_H tile: the pixel's column-major position x * h + y is searched in each entry's run ends, the last
 * entry first, and is covered when the index of the first run end greater than it is odd.  ZH_OVERLAP_LAST: the label of the last
 * entry that covers the pixel; ZH_OVERLAP_IGNORE: that label when exactly one entry covers it, ignore_value when two or more do; 0
 * when none does.  No atomics: the bytes are the same every time.  No cap on a list's length or on a mask's runs.  A mask
 * zh_rle_prefix flagged, an index outside 0 .. n_masks - 1 and a mask of fewer than two runs paint nothing; an image that does not
 * lie inside out is not written.  max_tiles: at least ceil(w / ZH_LABEL_TILE_W) * ceil(h / ZH_LABEL_TILE_H) of every image (the
 * grid's width: an image's pixels past it are not written); B <= 65535; B = 0 or max_tiles = 0 launches nothing. */
#define ZH_OVERLAP_LAST 0
#define ZH_OVERLAP_IGNORE 1
#define ZH_LABEL_TILE_W 32
#define ZH_LABEL_TILE_H 8
int zh_runs_label_maps(const int* run_end, const int* run_off, const int* status, int n_masks, long n_runs, const int* list_off,
                       const int* list_mask, const unsigned char* list_label, int n_list, const int* hw, const long long* out_off,
                       int B, int max_tiles, int overlap, int ignore_value, unsigned char* out, long out_bytes, zh_stream_t stream);

/* ---- device PNG encoder (zutis_amd/png_device.py is the definition; csrc/png.hip) ---- */
/* The zlib stream of the PNG of B u8 images, byte for byte png_device.deflate_np: every row filtered with type 2 (Up), the filtered
 * bytes cut into segments of ZH_PNG_SEGMENT_BYTES, each one fixed-Huffman deflate block of literals and distance-1 matches over its runs
 * of equal bytes followed by an empty stored block, 78 01 in front, 03 00 and the Adler-32 behind.  What is left for the host is the
 * chunk framing (png_device.frame: signature, IHDR, PLTE, the IDAT's CRC-32, IEND).
 * images u8 [image_bytes]: image b is [h, w, c] row-major at img_off[b] (int64 [B]), (h, w) = hw[2 b], hw[2 b + 1] (int32 [B, 2]); c = 1 or
 * 3 for the whole call.  out u8 [out_bytes]: image b's stream starts at out_off[b] (int64 [B]) and is lengths[b] (int32 [B]) bytes long,
 * at most png_device.stream_bound(h, w, c) = 2 + full * 18438 + (rest ? (9 rest + 20) / 8 + 4 : 0) + 6 with full, rest = divmod(h * (w c + 1),
 * ZH_PNG_SEGMENT_BYTES) — the stride the caller lays the streams out at; bytes past the length are not written.  max_segments: at least
 * ceil(h (w c + 1) / ZH_PNG_SEGMENT_BYTES) of every image (the grid's width).  An image that does not fit — h or w below 1, more than
 * 0x6fffffff filtered bytes, bytes outside images, more segments than max_segments, a bound that does not fit behind out_off[b] — is
 * not read and not written: lengths[b] = -1.  Two launches; workspace >= zh_png_deflate_workspace_size bytes, 16-byte aligned: a
 * fixed-stride slot and (bytes, Adler pair) per segment.  B <= 65535; B = 0 launches nothing.  The bytes are the same every time. */
#define ZH_PNG_SEGMENT_BYTES 16384
size_t zh_png_deflate_workspace_size(int B, int max_segments);
int zh_png_deflate(const unsigned char* images, long image_bytes, const long long* img_off, const int* hw, int c, int B, int max_segments,
                   const long long* out_off, unsigned char* out, long out_bytes, int* lengths, void* workspace, size_t workspace_bytes,
                   zh_stream_t stream);

/* ---- device JPEG decoder (zutis_amd/jpeg_device.py is the definition; csrc/jpeg.hip and csrc/jpeg_host.hip over csrc/jpeg_codec.h) ---- */
/* B baseline JPEG files, given as their entropy-coded bytes and parsed headers (jpeg_device.parse / pack), decoded to interleaved RGB
 * u8 [h, w, 3], byte for byte jpeg_device.decode_np = what Pillow (libjpeg-turbo) gives for Image.open(p).convert("RGB"): Huffman
 * decoding, islow inverse DCT, fancy chroma upsampling of the cropped planes, 16-bit fixed-point YCbCr -> RGB.
 * scan u8 [scan_bytes]: the entropy segments of all files (the bytes between the RSTn markers, stuffed bytes still in).
 * segments int32 [n_segments, ZH_JPEG_SEGMENT_WORDS] = {image, first byte, end byte, first MCU}: one lane decodes one segment, so
 *   the caller sorts them by length (longest first); a segment holds min(restart interval, MCUs - first MCU) MCUs, all of them
 *   when the interval is 0.
 * images int32 [B, ZH_JPEG_IMAGE_WORDS] = {w, h, components (1 | 3), luma sampling h, v ((1,1) | (2,1) | (2,2); chroma is (1,1)),
 *   MCUs per row, MCU rows, table set, first 8 x 8 block in the workspace, output offset / 16, restart interval in MCUs, 0}.
 * tables u8 [n_sets, ZH_JPEG_TABLE_SET_BYTES]: four canonical Huffman tables (luma DC, luma AC, chroma DC, chroma AC) of
 *   ZH_JPEG_HUFF_TABLE_BYTES each — look u16 [256] = (length << 8 | value) of the code that is a prefix of 8 bits (0: longer), maxcode
 *   int32 [18] by length (-1: none), valoff int32 [18], vals u8 [256] — then quant u16 [2, 64] (luma, chroma) in natural order;
 *   n_sets <= ZH_JPEG_MAX_TABLE_SETS (they live in LDS), n_segments <= ZH_JPEG_MAX_SEGMENTS.
 * out u8 [out_bytes]: image b's pixels at 16 * its offset word, the offsets ops.resize_crop_normalize / resize_normalize read.
 * status int32 [B]: 0, or the OR of ZH_JPEG_STATUS_* — the image's pixels are then not to be used (the caller decodes it on the host).
 * By construction, whatever the bytes say: every loop is bounded by the geometry (a block takes at most 64 symbols, a segment at most
 * 64 x its blocks); no byte outside a segment's range is read (a read past the end yields zero bits and, once such bits are used,
 * sets TRUNCATED) and no coefficient outside the image's block range is written; a descriptor that does not fit (sizes, offsets,
 * table set, block range, output range) is not read through and nothing of its image is written.
 * max_image_blocks / max_image_pixels: at least the blocks (MCUs x blocks per MCU) and the pixels of every image — the widths of the
 * grids of launches B and C; an image beyond them gets DESCRIPTOR.  B <= 65535.
 * n_blocks: 8 x 8 blocks of the whole batch (below 2^24); workspace >= zh_jpeg_decode_workspace_size bytes, 16-byte aligned: MCU counters int32 [B],
 * coefficients int16 [n_blocks, 64] in natural order (zeroed here), samples u8 [n_blocks, 64].  Three launches (entropy: one lane per
 * segment; dequantise + inverse DCT: one lane per block; upsample + colour: one lane per pixel) behind two fills.  B = 0 launches
 * nothing. */
#define ZH_JPEG_IMAGE_WORDS 12
#define ZH_JPEG_SEGMENT_WORDS 4
#define ZH_JPEG_HUFF_TABLE_BYTES 912
#define ZH_JPEG_TABLE_SET_BYTES 3904
#define ZH_JPEG_MAX_TABLE_SETS 16
#define ZH_JPEG_MAX_SEGMENTS 1048576
#define ZH_JPEG_STATUS_TRUNCATED 1   /* bits past the end of the segment were used */
#define ZH_JPEG_STATUS_CODE 2        /* an undefined Huffman code */
#define ZH_JPEG_STATUS_INDEX 4       /* a coefficient index past 63 */
#define ZH_JPEG_STATUS_MARKER 8      /* a marker (FF not followed by 00) inside a segment */
#define ZH_JPEG_STATUS_BITS 16       /* a DC extra-bit count above 11 or an AC count above 10 */
#define ZH_JPEG_STATUS_SEGMENT 32    /* a segment row outside the scan bytes or the image's MCUs */
#define ZH_JPEG_STATUS_DESCRIPTOR 64 /* an image row the launch cannot serve */
#define ZH_JPEG_STATUS_INCOMPLETE 128 /* the segments that decoded do not cover the image's MCUs */
size_t zh_jpeg_decode_workspace_size(int B, long n_blocks);
int zh_jpeg_decode(const unsigned char* scan, long scan_bytes, const int* segments, int n_segments, const int* images, int B,
                   const unsigned char* tables, int n_sets, long n_blocks, long max_image_blocks, long max_image_pixels,
                   unsigned char* out, long out_bytes, int* status, void* workspace, size_t workspace_bytes, zh_stream_t stream);

/* zh_jpeg_decode with the entropy stage of every segment split among lanes (self-synchronising Huffman decoding, made exact by a
 * verifying pass): a file without restart markers is ONE segment, which zh_jpeg_decode gives to one lane.  Arguments and results as
 * zh_jpeg_decode, and:
 * chunks int32 [n_chunks, ZH_JPEG_CHUNK_WORDS] = {segment row, first byte, unstuffed bits of the segment in front of it, 1 for the
 *   first chunk of its segment}: every segment [lo, hi) cut every chunk_bytes bytes (a cut that falls on the 00 of an FF 00 pair moves
 *   behind it), the chunks of a segment in order and next to each other, the segments in the order of their rows; a segment without
 *   bytes has one chunk (jpeg_device.chunk_rows).  chunk_bytes: a multiple of 16 in ZH_JPEG_CHUNK_BYTES_MIN .. 4096
 *   (ZH_JPEG_CHUNK_BYTES is what the loaders stage); n_chunks <= ZH_JPEG_MAX_CHUNKS.
 * Launches: `passes` (1 .. 64; ZH_JPEG_SPLIT_PASSES by default) of the lenient synchronising kernel — one workgroup per sequence of
 *   ZH_JPEG_SPLIT_LANES chunk rows; lane i decodes the symbols that start in its chunk from the state (bit, block in MCU, coefficient
 *   index) lane i - 1 hands it, until no state changes; a sequence's first lane takes the last state of the sequence before it from
 *   the launch before; a decoder that cannot fail: an undefined code skips a bit, an index past 63 ends the block, a category is
 *   clamped —, a segmented scan of the blocks every chunk completes (two launches), the strict pass (one lane per chunk, the rules of
 *   zh_jpeg_decode, DC values as differences) and the DC sums per segment and component; then the pixel stage of zh_jpeg_decode.
 * The strict pass compares the state it ends in with the state the next chunk started from and the blocks it completed with the
 *   count the scan used: a difference sets ZH_JPEG_STATUS_UNSYNCED.  The first chunk of a segment starts from the true state, so an
 *   image without that bit (and without an error bit) was decoded from true states throughout: its pixels are zh_jpeg_decode's.
 *   passes >= the sequences of the longest segment always suffices.  A chunk row that does not fit — outside its segment, not behind
 *   its predecessor, longer than chunk_bytes + 1, an unstuffed count that is not the count of its predecessor's bytes — gives its
 *   image DESCRIPTOR; a row whose segment or image cannot be told is ignored (the image then stays INCOMPLETE).
 * Every loop is bounded by the bits of a chunk or by ZH_JPEG_SPLIT_LANES; nothing outside out, status and the workspace is written.
 * workspace >= zh_jpeg_decode_split_workspace_size bytes, 16-byte aligned: that of zh_jpeg_decode, then per chunk the state it
 *   starts from and ends in, its block count and first block, per sequence two hand-over states, its open block sum and carry. */
#define ZH_JPEG_CHUNK_WORDS 4
#define ZH_JPEG_CHUNK_BYTES 128
#define ZH_JPEG_CHUNK_BYTES_MIN 16
#define ZH_JPEG_SPLIT_LANES 256
#define ZH_JPEG_SPLIT_PASSES 2
#define ZH_JPEG_MAX_CHUNKS 4194304
#define ZH_JPEG_STATUS_UNSYNCED 256  /* split decoding: a chunk did not start from the state its predecessor ended in */
size_t zh_jpeg_decode_split_workspace_size(int B, long n_blocks, long n_chunks);
int zh_jpeg_decode_split(const unsigned char* scan, long scan_bytes, const int* segments, int n_segments, const int* chunks, long n_chunks,
                         int chunk_bytes, int passes, const int* images, int B, const unsigned char* tables, int n_sets, long n_blocks,
                         long max_image_blocks, long max_image_pixels, unsigned char* out, long out_bytes, int* status, void* workspace,
                         size_t workspace_bytes, zh_stream_t stream);

/* ---- device JPEG encoder (zutis_amd/jpeg_device.py encode_np / scan_np is the definition; csrc/jpeg_enc.hip and csrc/jpeg_host.hip over
 * csrc/jpeg_codec.h) ---- */
/* The entropy-coded scan of the baseline JPEG of B u8 RGB images, byte for byte jpeg_device.scan_np = what Pillow (libjpeg-turbo) writes
 * between the SOS header and EOI for save(f, "JPEG", quality, subsampling, restart_marker_blocks=ZH_JPEG_ENC_INTERVAL_MCUS): 16-bit
 * fixed-point RGB -> YCbCr, edge replication to the MCU grid, h2v2 chroma downsampling (subsampling 2) or none (0), the islow forward DCT,
 * quantisation by the two tables given, libjpeg's dummy-block rule, the Annex K Huffman tables, a restart marker every
 * ZH_JPEG_ENC_INTERVAL_MCUS MCUs.  What is left for the host is the header in front (jpeg_device.header_bytes) and FF D9 behind.
 * images u8 [image_bytes]: image b is [h, w, 3] row-major at img_off[b] (int64 [B]), (h, w) = hw[2 b], hw[2 b + 1] (int32 [B, 2]).
 * subsampling: 0 (4:4:4) or 2 (4:2:0) for the whole call; quant u16 [2, 64]: the luma and chroma tables in natural order, 1 .. 255.
 * out u8 [out_bytes]: image b's scan starts at out_off[b] (int64 [B]), RSTn markers included; at most slot_bytes of it are written,
 * the slots [out_off[b], out_off[b] + slot_bytes) being the caller's layout (jpeg_device.scan_slot); bytes past the length inside the
 * slot are not written.  lengths[b] (int32 [B]) is the TRUE length of the scan also when it exceeds slot_bytes: the caller sees the
 * overflow there and encodes that image another way.  max_mcus: at least the MCUs of every image (the grids' width).  An image that
 * does not fit — h or w outside 1 .. 65535, bytes outside images, more MCUs than max_mcus, a slot outside out — is not read and not
 * written: lengths[b] = -1.
 * Three launches (coefficients: one lane per 8 x 8 block; entropy: one workgroup per restart interval; gather: the intervals into the
 * slot with the markers between); workspace >= zh_jpeg_encode_workspace_size bytes, 16-byte aligned: per image the zig-zag int16
 * coefficients of max_mcus MCUs, a worst-case slot (ZH_JPEG_ENC_BLOCK_BYTES per block, doubled by stuffing) and a length word per
 * interval.  Every loop is bounded by the geometry and these constants; nothing outside out, lengths and the workspace is written.
 * B <= 65535; B = 0 launches nothing.  The bytes are the same every time. */
#define ZH_JPEG_ENC_INTERVAL_MCUS 16
#define ZH_JPEG_ENC_BLOCK_BYTES 208 /* a block's bits at the most: 11 + 11 of DC, 63 x (16 + 10) of AC = 1660 */
#define ZH_JPEG_ENC_SLOT_EXTRA 1024 /* jpeg_device.scan_slot(h, w) = 3 h w + this */
size_t zh_jpeg_encode_workspace_size(int B, long max_mcus, int subsampling);
int zh_jpeg_encode(const unsigned char* images, long image_bytes, const long long* img_off, const int* hw, int B, int subsampling,
                   long max_mcus, const unsigned short* quant, const long long* out_off, unsigned char* out, long out_bytes,
                   long slot_bytes, int* lengths, void* workspace, size_t workspace_bytes, zh_stream_t stream);
/* HOST twin of zh_jpeg_encode: HOST pointers, the same codec functions in three loops, scratch allocated inside at the workspace's sizes. */
int zh_jpeg_encode_host(const unsigned char* images, long image_bytes, const long long* img_off, const int* hw, int B, int subsampling,
                        long max_mcus, const unsigned short* quant, const long long* out_off, unsigned char* out, long out_bytes,
                        long slot_bytes, int* lengths);

/* Native launch plans (zutis_amd/plan.py): replay n recorded calls of the entry points above (op id + 32 argument words
 * each; dispatcher generated from this header) in one C loop; zh_plan_run2 alternates two plans on two streams. */
int zh_plan_run(const void* cmds, int n, zh_stream_t stream);
int zh_plan_run2(const void* cmds_a, int na, zh_stream_t stream_a, const void* cmds_b, int nb, zh_stream_t stream_b);
/* `count` plans round-robin on `count` streams (launch i of every plan before launch i+1 of any). */
int zh_plan_run_multi(const void* const* cmds, const int* n, const zh_stream_t* streams, int count);
/* Name of the entry point the library dispatches plan op `op` to (NULL if out of range): the host checks it against its
 * own table so that a stale library cannot mis-dispatch. */
const char* zh_plan_op_name(int op);

/* HOST helper: RLE string from run lengths (pycocotools rleToString). */
long zh_rle_counts_to_string_host(const long long* counts, long n, char* out, long cap);
/* HOST.  The RLE strings of n masks from zh_mask_runs' output in one call: positions int32 [n, stride] (packed = 0) or the packed
 * list of zh_mask_runs_kept (packed = 1, stride = its max_runs: row i follows row i - 1, min(transitions, stride) entries each), nruns
 * int32 [n, 2] (transitions, value of pixel 0), HW pixels per mask; strings back to back in `out` (cap bytes), offsets int64 [n + 1]; a
 * mask with more transitions than `stride` gets an empty string (the caller re-encodes it from the mask).  Returns the total length,
 * -1 when cap is too small.  Replaces pycocotools.mask.encode per kept mask (networks/zutis.py:290,448). */
long zh_rle_from_transitions_host(const int* positions, long stride, int packed, const int* nruns, long n, long HW, char* out, long cap,
                                  long long* offsets);

/* One training sample of IndexDataset.__getitem__ on the device — datasets/index_dataset.py:301-385: random_scale / random_crop /
 * random_hflip (datasets/augmentations/geometric_transforms.py), ColorJitter + RandomGrayscale + GaussianBlur
 * (datasets/base_dataset.py:62-78), to_tensor + normalize, copy_paste (datasets/augmentations/copy_paste.py) — for a batch of B
 * samples made of N sub-images, every random draw taken from a recipe (zutis_amd/synth.py).  Bit-identical to Pillow / torch on the
 * host except the blur.  Between the stages a sub-image is u8 [C, C, 4] = (R, G, B, mask byte in {0, 1, ignore_index}).
 * packed / packed_bytes: as for zh_resize_crop_normalize_u8, the u8 [h, w] masks packed next to the images.
 * desc int32 [N, 32] per sub-image: image offset / 16, w, h, scaled nw, nh, mask offset / 16, pad left, pad top, crop left, crop top,
 *   flip, label id, flags (1 jitter, 2 grey, 4 blur, 8 padded), op order (four 2-bit codes, first op lowest: 0 brightness, 1 contrast,
 *   2 saturation, 3 hue), hue shift (the u8 added to H), brightness / contrast / saturation factors (fp32 bits), the ATen nearest
 *   scales float(h) / float(nh), float(w) / float(nw) (fp32 bits), the paste draws u_top, u_left (float64 bits, two slots each), 0.
 * work int32 [N, 12], 8-byte aligned, initialised by the caller to (0 x 8, C, -1, C, -1): four u64 sums (the scaled image's R, G, B:
 *   its mean is the pad fill; the grey sum behind the contrast mean) and the object's box ymin, ymax, xmin, xmax.
 * zh_synth_geometry_u8: Pillow BILINEAR at (nw, nh) (the resampler of zh_resize_normalize_u8, kmax as there, >= 3), ATen nearest
 *   for the mask, pad (image: the integer channel mean of the scaled image; mask: ignore_index), crop C x C, flip -> out_rgbm, box -> work.
 *   fill_w x fill_h: the largest scaled extent among the PADDED sub-images (0: none is padded, the sums are not computed).  A descriptor
 *   the launch cannot serve (bytes outside packed, more taps than kmax) gives an all-ignore crop and is not read through. */
int zh_synth_geometry_u8(const unsigned char* packed, long packed_bytes, const int* desc, int N, int C, int ignore_index, int kmax,
                         int fill_w, int fill_h, int* work, unsigned char* out_rgbm, zh_stream_t stream);
/* ColorJitter's ops in desc's order (ImageEnhance blends; the hue shift through Pillow's RGB <-> HSV) and RandomGrayscale, in place;
 * the contrast mean is reduced over the image as it stands when contrast is reached (work). */
int zh_synth_photometric_u8(unsigned char* rgbm, const int* desc, int N, int C, int* work, zh_stream_t stream);
/* Separable Gaussian, BORDER_REFLECT_101, of the sub-images whose flags say blur: rgbm -> out_rgbm (the others are not written).
 * weights f32 [N, ksize], normalised; ksize odd, radius at most 48.  fp32 sums rounded to nearest: within one level of the exact value. */
int zh_synth_blur_u8(const unsigned char* rgbm, const int* desc, const float* weights, int N, int C, int ksize, unsigned char* out_rgbm,
                     zh_stream_t stream);
/* copy_paste per output pixel + normalisation.  samples int32 [B, 4]: first sub-image, n (at most 64), first one-hot row, 0.  A sub-image
 * is read from rgbm_blurred when its flags say blur, else from rgbm.  lut f32 [3, 256] as for zh_resize_crop_normalize_u8.
 * -> image f32 [B, 3, C, C], semantic int64 [B, C, C], onehot u8 (bool) [sum n, C, C]. */
int zh_synth_compose(const unsigned char* rgbm, const unsigned char* rgbm_blurred, const int* desc, const int* samples, const int* work,
                     const float* lut, int N, int B, int C, int ignore_index, float* image, long long* semantic, unsigned char* onehot,
                     zh_stream_t stream);

/* HOST helper (no GPU): COCO RLE string of one u8 [H,W] mask = pycocotools.mask.encode(np.asfortranarray(m))["counts"]
 * (zutis.py:290,448; datasets/index_dataset.py:219).  Returns the length, -1 if cap is too small. */
long zh_rle_encode_host(const unsigned char* mask, int H, int W, char* out, long cap);

/* HOST twin of zh_jpeg_decode (no GPU, HOST pointers, its own scratch): the same codec (csrc/jpeg_codec.h) and the same pixel
 * arithmetic on the CPU, for the CPU tests and the host sanitizer program (tools/host/jpeg_host_check.cpp).  Arguments as there. */
int zh_jpeg_decode_host(const unsigned char* scan, long scan_bytes, const int* segments, int n_segments, const int* images, int B,
                        const unsigned char* tables, int n_sets, long n_blocks, unsigned char* out, long out_bytes, int* status);
/* HOST twin of zh_jpeg_decode_split: the same passes over the same rows with the same functions of csrc/jpeg_codec.h, lanes as loops. */
int zh_jpeg_decode_split_host(const unsigned char* scan, long scan_bytes, const int* segments, int n_segments, const int* chunks, long n_chunks,
                              int chunk_bytes, int passes, const int* images, int B, const unsigned char* tables, int n_sets, long n_blocks,
                              unsigned char* out, long out_bytes, int* status);

#ifdef __cplusplus
}
#endif
#endif /* ZUTIS_HIP_H */
