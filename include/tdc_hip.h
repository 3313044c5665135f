/* tdc_hip.h — C ABI of libtdc_hip.so: the MI355X (gfx950) implementation of TDC-Video's video-encoding hot path.
 *
 * The reference (Hoar012/TDC-Video) is 100 % Python and has no FFI layer; its boundary for this path is the Python
 * mixin `CambrianMetaForCausalLM.{encode_images, prepare_inputs_labels_for_multimodal}` (tdc/cambrian_arch.py:698,
 * :864).  Each entry point below replaces the eager-op sequence of one stage of that function; the citation next to
 * it names the reference lines it replaces.  `tdc-video_amd/` (Python) marshals torch tensors' data_ptr() into these
 * calls; INTEGRATION.md shows the ctypes binding a maintainer of the reference would add.
 *
 * Conventions
 *  - every pointer is a DEVICE pointer unless the name ends in `_host`; nothing is allocated inside a call
 *    (composite calls take a caller-provided workspace; query its size with the matching *_workspace_bytes);
 *  - `stream` is a hipStream_t passed as void*; calls only enqueue work (no synchronisation);
 *  - return value: 0 on success, otherwise a hipError_t / negative TDC_E* code (message on stderr);
 *  - 16-bit tensors are fp16 (TDC_F16) or bf16 (TDC_BF16), accumulation / LayerNorm / softmax / GELU are fp32;
 *  - activation matrices are row-major [rows, ld] with ld = round_up(cols, 64) and ZERO pad columns; weights are
 *    nn.Linear layout [out, in] padded the same way (prepared once by tdc-video_amd/weights.py).
 *
 * Memory contract (pinned by tests/test_hip_memory_contract.py: outputs inside sentinel-filled arenas, inputs surrounded by
 * 0x00 / 0xFF bytes, results bit-identical under both)
 *  - a call READS only the rows / elements its description names: rows 0 .. rows-1 (through the row map where there is one -
 *    never the gaps of a map), columns 0 .. cols-1 plus, where a kernel loads whole 16-byte pieces, the ZERO pad columns up to
 *    ld that the convention above promises.  Memory behind the last row, in front of the base pointer, rows a map or an index
 *    array never names, and scratch / workspace contents on entry never reach a result;
 *  - a call WRITES only what the "writes:" line of its description says.  Pure outputs are fully overwritten there (no
 *    accumulation into their previous contents).  Where the line says "pad columns: caller", the kernel leaves the columns
 *    cols .. ld untouched and a consumer that relies on zero pad columns needs them zeroed once by the buffer's owner.
 */
#ifndef TDC_HIP_H
#define TDC_HIP_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define TDC_F16 0
#define TDC_BF16 1

#define TDC_ACT_NONE 0
#define TDC_ACT_GELU_ERF 1   /* nn.GELU() default, ACT2FN["gelu"]          */
#define TDC_ACT_GELU_TANH 2  /* "gelu_pytorch_tanh" (SigLIP MLP)            */
#define TDC_ACT_SWIGLU 3     /* silu(x1)*x2 on interleaved (x1,x2) columns  */

#define TDC_E_BADARG (-2)
#define TDC_E_WORKSPACE (-3)

/* row(m) = (m / seg) * stride + off + (m % seg) * inner ; identity when seg == 0 */
typedef struct { int seg, stride, off, inner; } tdc_rowmap;

/* C[c_map(m), n] = act(sum_k A[a_map(m), k] * W[n, k] + bias[n]) + res[r_map(m), n]        (nn.Linear + epilogue)
 * K % 64 == 0, N % 4 == 0 (N % 8 == 0 for SWIGLU, output col = n/2).  Replaces every nn.Linear on the path.
 * An activation excludes a residual and an fp32 output (TDC_E_BADARG): the activation epilogues store 16-bit values. */
typedef struct {
    const void* A; int lda;
    const void* W; int ldw;
    void* C; int ldc;
    const float* bias;
    const void* res; int ldres;
    int M, N, K;
    int dtype, out_f32, res_f32, act;
    tdc_rowmap a_map, c_map, r_map;
    /* LayerNorm fused into the GEMMs around it (ViT towers; all NULL = plain GEMM).
     * Producer (the fp32 residual-stream GEMMs: out_f32, fp32 res, identity c_map / r_map, N % 64 == 0): with x16 != NULL
     * the updated row is also written as 16-bit to x16 [rows, ldx16] and, per row m and 64-column slot s, (mean, M2) of
     * the slot's 64 values to ln_part[(s * M + m) * 2 ..] (slot-major); tdc_ln_finalize turns them into (mean, rstd) per row.
     * Producer over a 16-bit residual stream (16-bit C and res of one type - in place when C == res -, identity c_map / r_map,
     * N % 64 == 0, 16-byte aligned rows): ln_part != NULL with x16 == NULL - only the partials are emitted, of the fp32 sums
     * acc + bias + float(res) that are rounded into C; the consumer then reads the stream itself as its A operand.
     * Consumer (16-bit output, no residual, identity a_map): with ln_stats != NULL, A holds the RAW rows x (x16 of the
     * producer) and W the gamma-folded weight W diag(gamma); the epilogue computes
     *   act(rstd[m] * (acc[m, n] - mean[m] * ln_c1[n]) + bias[n])   == act(LayerNorm(x) W^T + b)
     * with ln_stats [M, 2] = (mean, rstd), ln_c1[n] = sum_k W'[n, k] (of the 16-bit W'), bias = beta W^T + b. */
    void* x16; int ldx16; float* ln_part;
    const float* ln_stats; const float* ln_c1;
    /* in_fp8 != 0: A and W hold OCP e4m3 bytes (K % 128 == 0, lda / ldw % 16 == 0, both counted in values), accumulated by
     * v_mfma_f32_16x16x128_f8f6f4 (unit block scales); `dtype` stays the 16-bit type of C / res.  The dequantisation scales ride on the
     * LayerNorm-fold operand ln_stats[m] = (*, s_a[m] * s_w): C = act(s_a[m] s_w acc + bias).  ln_c1 is not read (may be NULL)
     * and ln_stats[m].x is used by out_fp8 only. */
    int in_fp8;
    /* out_fp8 != 0 (with in_fp8 + ln_stats, no residual, N % 64 == 0): C receives OCP e4m3 bytes [M, ldc] (ldc in bytes,
     * % 16 == 0) scaled per row by s_h[m] = B[m]^p / 448, where B[m] = ln_stats[m].y * ln_stats[m].x * out_w2max + out_bmax
     * bounds |A W^T + b| on that row (Cauchy-Schwarz: ln_stats.x = the 2-norm of the quantised A row as tdc_layernorm's
     * y8 path writes it, out_w2max = the largest 2-norm of a quantised W row, out_bmax = max|bias|) and p = 2 for SWIGLU
     * (|silu(a) b| <= |a| |b|), 1 otherwise (|gelu(a)| <= |a|).  e4m3 is a floating-point format: a scale that is safe but
     * an order of magnitude loose costs no relative precision.  out_stats[m] = (0, s_h[m] * out_wscale) are the ln_stats
     * of the fp8-operand GEMM that consumes C (out_wscale = its per-tensor weight scale). */
    int out_fp8; float* out_stats; float out_w2max, out_bmax, out_wscale;
    /* c_pad8 != 0 (16-bit C, no residual, no bias, N % 4 == 0, ldc >= round_up(N, 8)): the rows of C are writable up to
     * round_up(N, 8) columns - the 16-byte row stores of the staged epilogue may then run 4 columns past an N with
     * N % 8 == 4 (unspecified values there) instead of falling back to 8-byte stores.  Used by the transposed value
     * projection of the Q-Former (N = frames x tokens). */
    int c_pad8;
    /* c16_dtype_p1 != 0: the 16-bit type of C and of a 16-bit res is (c16_dtype_p1 - 1) instead of `dtype` (0 = `dtype`, so a
     * zero-initialised descriptor keeps the operand type).  For the residual-stream GEMMs of a tower whose operands are bf16
     * and whose residual stream is kept in fp16 (tdc_vit_model.res_dtype_p1): C = fp16(acc + bias + float(res)), one rounding.
     * Needs 16-bit C (out_f32 == 0), act == NONE, no LayerNorm-fusion / fp8 operand. */
    int c16_dtype_p1;
    /* writes: C[c_map(m), 0 .. n_out) for m < M, n_out = N (N / 2 for SWIGLU) - and, with c_pad8, possibly the columns
     * N .. round_up(N, 8) of those rows; never the columns n_out (round_up(N, 8)) .. ldc (pad columns: caller), never a row no
     * m < M maps to.  In place (C == res) the same set.  x16[m, 0 .. N), ln_part[s][m][0 .. 2) for s < N / 64, out_stats[m][0 .. 2)
     * for m < M.  reads: A[a_map(m), 0 .. K), W[n, 0 .. K) for n < N, bias[0 .. N), res[r_map(m), 0 .. N), ln_stats[m], ln_c1[0 .. N). */
} tdc_gemm_desc;
int tdc_gemm(const tdc_gemm_desc* d, void* stream);
/* Diagnostics only (tools/, never the product path): 1 = skip the C-tile epilogue (nothing is written), 2 = un-staged
 * epilogue; 0 (the default) = normal operation.  Prints a warning on stderr when switched on; returns the previous mode.
 * The library reads no environment variable for this. */
int tdc_gemm_set_debug(int mode);
/* Workgroups of the persistent GEMM kernel: 0 (default) = one per CU the device reports; a multiple of 8 (>= 8, at most the
 * device's) for a process confined to part of the chip by a CU mask, which the device properties do not show.  Results never
 * depend on it.  Prints a note on stderr when set; returns the previous value, -1 when refused.  The library reads no
 * environment variable for this. */
int tdc_gemm_set_persistent_grid(int workgroups);
/* per-row e4m3 quantisation of a 16-bit matrix x [rows, ldx] (cols % 8 == 0, cols <= 4608): y8 [rows, ldy8] = x / s_a[r]
 * with s_a[r] = max|x[r]| / 448 (zero bytes up to the next multiple of 128 columns when ldy8 allows), stats[r] =
 * (0, s_a[r] * wscale) - the operands of an fp8-operand tdc_gemm whose input does not come out of a LayerNorm (the
 * attention output, the MLP hidden).
 * writes: y8[r, 0 .. round_up(cols, 128)) when ldy8 >= that, else y8[r, 0 .. cols); stats[r][0 .. 2); r < rows. */
int tdc_quantize_rows_fp8(const void* x, int ldx, int rows, int cols, int dtype, void* y8, int ldy8, float* stats,
                          float wscale, void* stream);
/* (mean, M2) partials [slots, rows, 2] of `slots` 64-column slots per row -> stats [rows, 2] = (mean, 1 / sqrt(var + eps)), biased
 * variance over slots * 64 columns (nn.LayerNorm); Chan's parallel combination in a fixed order.  writes: stats[r][0 .. 2), r < rows. */
int tdc_ln_finalize(const float* ln_part, int slots, int rows, float eps, float* stats, void* stream);

/* LayerNorm over `cols` real columns of x [rows, ldx] (fp32 or 16-bit), optional additive table before the norm:
 * x'[r] = x[r] + add[(r % add_period) mapped by add_mode]; y = LN(x') * gamma + beta.  Writes y16 (16-bit, pad
 * columns zeroed, may be NULL) and/or y32 (fp32, may alias x, may be NULL).
 * add_mode 0: table row = r % add_period; 1: SVA 2x2 window position ((y&1)*2 + (x&1)) of token r % add_period on a
 * sqrt(add_period)-wide grid (tdc/vision_sampler.py:375-384).
 * writes: columns 0 .. round_up(cols, 64) of the rows y_map(r), r < rows, of every output given (y16 / y32 / y8: zeros beyond
 * cols) when EVERY given output has ld >= round_up(cols, 64), otherwise columns 0 .. cols only (pad columns: caller); columns
 * beyond round_up(cols, 64) never; y8_stats[y_map(r)][0 .. 2).  reads: x[x_map(r), 0 .. cols), gamma / beta / add rows [0 .. cols). */
typedef struct {
    const void* x; int ldx; int x_f32;
    void* y16; int ldy16;
    float* y32; int ldy32;
    const float* gamma; const float* beta; float eps;
    const float* add; int ldadd; int add_period; int add_mode;
    int rows, cols, dtype;
    tdc_rowmap x_map, y_map; /* row r reads x[x_map(r)] and writes y*[y_map(r)] (identity when seg == 0) */
    /* fp8 output (may be NULL; when set it is the only output: y16 and y32 must be NULL): y8 [rows, ldy8] OCP e4m3 bytes = y / s_a[r] with the
     * per-row scale s_a[r] = max|y[r]| / 448, pad columns zero; y8_stats[r] = (1.07 ||y[r] / s_a[r]||_2, s_a[r] * y8_wscale) is
     * the ln_stats operand of the fp8-operand tdc_gemm that consumes y8 (y8_wscale = that GEMM's per-tensor weight scale;
     * the first entry - an upper bound of the 2-norm of the QUANTISED row - only matters to tdc_gemm_desc.out_fp8). */
    void* y8; int ldy8; float* y8_stats; float y8_wscale;
    /* x_dtype_p1 != 0 (with x_f32 == 0): the 16-bit type of x is (x_dtype_p1 - 1) instead of `dtype` (0 = `dtype`): an fp16
     * residual stream normalised into bf16 GEMM operands.  Needs y32 == NULL, y8 == NULL, add == NULL, cols % 8 == 0. */
    int x_dtype_p1;
} tdc_ln_desc;
int tdc_layernorm(const tdc_ln_desc* d, void* stream);

/* softmax(Q K^T * scale) V (no mask but the optional key padding mask of the biased form).  Q element (b, s, h, c) at q + b*q_bs + s*q_rs + h*head_dim + c (same for
 * k, v, o).  head_dim <= 80 (TDC_E_BADARG above).  Replaces HF SigLIP/DINOv2 attention (HF:models/siglip/modeling_siglip.py:273-308),
 * BertSelfAttention self and cross (tdc/Qformer.py:169-275). */
typedef struct {
    const void *q, *k, *v; void* o;
    long long q_bs, k_bs, v_bs, o_bs;
    int q_rs, k_rs, v_rs, o_rs;
    int batch, heads, head_dim, sq, sk;
    float scale; int dtype;       /* scale: finite and >= 0 (TDC_E_BADARG otherwise, nothing is written): the kernels take the
                                     exponent offset of a row as max(q.k) * scale, which is its largest score only then.
                                     scale == 0 is valid: every key weighs the same and o is the mean of V (-0.0 counts as 0) */
    /* optional additive score bias, fp32 (NULL = none): score(b,h,q,k) = scale*q.k + gate[(b*sq+q)*gate_rs + h] *
     * bias[h*bias_hs + q*bias_rs + k].  BEATs gated relative position bias
     * (tdc/audio_models/beats/backbone.py:650-661); needs sk % 4 == 0, head_dim <= 64. */
    const float* bias; long long bias_hs; int bias_rs;
    const float* gate; int gate_rs;
    /* optional key padding mask of the biased form (NULL = none; needs `bias`): key k of batch item b is excluded from the
     * softmax (score -inf BEFORE the bias is added, backbone.py:633-643) when key_mask[b*key_mask_bs + k] != 0.
     * key_mask_bs % 4 == 0, 4-byte aligned.  BEATs padded batches (BEATs.py:142-153: padding_mask of extract_features). */
    const unsigned char* key_mask; long long key_mask_bs;
    /* kernel form: TDC_ATTN_FORM_AUTO (0) picks by shape (the 32x32x16 kernel for long sequences at head dim 64 / 72, the
     * 16x16x32 kernels otherwise); TDC_ATTN_FORM_16X16 keeps the 16x16x32 kernels for every shape (tests compare the forms) */
    int form;
    /* optional per-item key count (device int32 [batch], NULL = sk for every item): item b attends to the keys [0, k_len[b]),
     * 1 <= k_len[b] <= sk.  The item runs the code a uniform launch of the same kernel form with sk = k_len[b] runs - the same
     * key tiles from key 0, the same masked last tile -, so its output rows are bit for bit that launch's.  Keys at and beyond
     * k_len[b] are never loaded (row indices are clamped to k_len[b] - 1): any bit pattern there, NaN included, leaves the result
     * unchanged.  Under TDC_ATTN_FORM_AUTO the form is picked from sq and sk as passed: a caller who wants AUTO's pick for every
     * item keeps k_len[b] >= 64 where sq >= 256 (below that every shape runs the 16x16x32 kernels anyway). */
    const int* k_len;
    /* optional per-item K / V source (device int32 [batch], NULL = b): item b reads its keys / values at k + kv_index[b]*k_bs and
     * v + kv_index[b]*v_bs; q and o stay at b.  Several items may name one slot (P prompts over one frame's K / V).
     * Both fields exclude `bias` (TDC_E_BADARG); their entries are NOT checked on the device: the caller range-checks them. */
    const int* kv_index;
    /* writes: o element (b, s, h, c) for b < batch, s < sq, h < heads, c < head_dim - nothing else: not the columns beyond
     * heads * head_dim of a row (pad columns: caller), not row sq of the last query tile.  reads: q rows s < sq, k / v rows
     * s < sk of every batch item - with k_len the rows s < k_len[b] only, with kv_index the rows of the slots it names only
     * (a slot no item names is not read) -, k_len[0 .. batch), kv_index[0 .. batch), bias[h][q][0 .. sk),
     * gate[(b*sq+q)][0 .. heads), key_mask[b][0 .. sk). */
} tdc_attn_desc;
#define TDC_ATTN_FORM_AUTO 0
#define TDC_ATTN_FORM_16X16 1
/* (round 4's TDC_ATTN_FORM_PW = 2, a slower one-wave-per-SIMD prototype, left the library in round 5: any other value = AUTO;
 *  the prototype lives in tools/attention_pw/) */
int tdc_attention(const tdc_attn_desc* d, void* stream);

/* ---- small data-movement / reduction kernels ------------------------------------------------------------- */
/* pixels [B,3,H,W] (px_f32: 0 = the 16-bit type `dtype`, 1 = fp32, 2 = the OTHER 16-bit type - fp16 frames into bf16
 * towers) -> patches [B*gh*gw, ldp] 16-bit `dtype` in conv-weight order (c,ky,kx), zero pad.
 * Patch-embed conv as a GEMM (HF:models/siglip/modeling_siglip.py:124-130, dinov2/modeling_dinov2.py:140-151).
 * writes: WHOLE rows patches[row, 0 .. ldp) (zeros from 3*patch*patch on), B*gh*gw rows. */
int tdc_im2col(const void* px, int px_f32, void* patches, int ldp, int B, int H, int W, int patch, int dtype,
               void* stream);
/* x32 [B, S, ld] rows `row` of every batch := vec[ld] (cls token + pos[0]).  writes: those B rows, all ld columns (vec has ld entries) */
int tdc_set_rows(float* x32, int ld, int B, int S, int row, const float* vec, void* stream);
/* the same into a 16-bit matrix x16 [B*S, ld] of type `dtype` (vec stays fp32): the cls row of a 16-bit residual stream */
/* writes: as tdc_set_rows */
int tdc_set_rows16(void* x16, int ld, int B, int S, int row, const float* vec, int dtype, void* stream);
/* separable 2-tap resample of a token grid: x (fp32 or 16-bit `dtype`) [B, tok_off + n_in*n_in, ldx] -> y 16-bit
 * (`out_dtype`: may differ from `dtype` - bf16 towers feeding an fp16 connector) [B, n_out*n_out, ldy]; idx0/idx1/frac are
 * device arrays [n_out] (bilinear, align_corners=False; built by host).
 * siglip_encoder.py:43-69, dino_encoder.py:81-107 (and the cls drop of feature_select :66-79).
 * writes: WHOLE rows y[row, 0 .. ldy) (zeros from `cols` on), B*n_out*n_out rows.  reads: x columns 0 .. cols of the token rows. */
int tdc_resample_tokens(const void* x, int x_f32, int ldx, int tok_off, int n_in, void* y, int ldy, int n_out,
                        const int* idx0, const int* idx1, const float* frac, int B, int cols, int dtype, int out_dtype,
                        void* stream);
/* adjacent-frame cosine similarity on flattened features f [T, n] 16-bit: sims[t] = cos(f[t], f[t+1]), t < T-1
 * (tdc/cambrian_arch.py:832-842); n % 8 == 0.  scratch: tdc_frame_cossim_scratch_floats(T) floats.  The reduction
 * order is fixed (fp32), so the similarity ranking is reproducible run to run.
 * writes: sims[0 .. T-1) and the scratch (every word of it before it is read: its contents on entry do not matter). */
int tdc_frame_cossim(const void* f, long long n, int T, float* sims, float* scratch, int dtype, void* stream);
size_t tdc_frame_cossim_scratch_floats(int T);
/* cosine similarity of arbitrary slot pairs of a slab of per-frame features (the frame cache's DINOv2 rows): frame s starts
 * at slab + s * slot_stride elements (16-bit, slot_stride % 8 == 0, slab 16-byte aligned), n elements each (n % 8 == 0);
 * pairs: device int32 [n_pairs, 2] (slot_a, slot_b), n_pairs <= 65535.  sims[p] is bit for bit what tdc_frame_cossim gives
 * for the same two frames adjacent in a contiguous buffer (shared chunking and reduction order).
 * scratch: tdc_pair_cossim_scratch_floats(n_pairs) floats.  writes: sims[0 .. n_pairs) and the scratch (as tdc_frame_cossim);
 * reads: the n elements of the slots the pairs name - not the gap n .. slot_stride behind a slot, not the other slots. */
int tdc_pair_cossim(const void* slab, long long slot_stride, long long n, const int* pairs, int n_pairs, float* sims,
                    float* scratch, int dtype, void* stream);
size_t tdc_pair_cossim_scratch_floats(int n_pairs);
/* 128-bit content fingerprint of rows of any type: row r = the row_bytes bytes at base + rows[r] * row_stride (rows: device
 * int32 [n_rows], n_rows <= 65535; any alignment, any length) -> out[2r], out[2r + 1] (device u64).  Words w_i = the row as
 * little-endian u64 (tail zero-padded), x_i = w_i ^ (i * 0x9E3779B97F4A7C15), h_k = mix(sum_i mix(x_i ^ S_k) ^ row_bytes)
 * with the splitmix64 finaliser mix and S_1 = 0x243F6A8885A308D3, S_2 = 0x13198A2E03707344 (sums mod 2^64: the bits do not
 * depend on the reduction order).  Not cryptographic.  scratch: tdc_fingerprint_rows_scratch_bytes(n_rows) bytes.
 * writes: out[0 .. 2 n_rows) and the scratch (contents on entry do not matter).  reads: exactly the row_bytes bytes of each row:
 * the bytes in front of an unaligned row start and behind its end never reach the fingerprint. */
int tdc_fingerprint_rows(const void* base, long long row_stride, const int* rows, int n_rows, long long row_bytes,
                         unsigned long long* out, void* scratch, void* stream);
size_t tdc_fingerprint_rows_scratch_bytes(int n_rows);
/* mean over the token axis: x [B, P, ld] 16-bit -> y [B, ld] 16-bit (global context, cambrian_arch.py:1009).
 * reads and writes WHOLE rows of ld elements: y's pad columns are the mean of x's (zero) pad columns */
int tdc_token_mean(const void* x, int P, int ld, void* y, int B, int dtype, void* stream);
/* adaptive_avg_pool1d over the token axis: y[b, k] = mean of x rows [floor(kN/K), ceil((k+1)N/K)) of frame
 * src_row[b] (b when NULL); frame f starts at row f*frame_rows (frame_rows >= N: extra rows, e.g. audio tokens, are
 * not pooled - the key frame is pooled BEFORE the audio concat, cambrian_arch.py:1609,1633-1637).
 * reads rows 0 .. N of the named frames and writes y [B*K, ld], WHOLE rows of ld elements (pad columns as tdc_token_mean) */
int tdc_adaptive_pool_tokens(const void* x, int N, int frame_rows, int ld, void* y, int K, int B,
                             const int* src_row, int dtype, void* stream);
/* out[i, :cols] = table_k[row] where (k,row) = src[2i], src[2i+1]; tables: up to 4 16-bit matrices with their ld.
 * Used for unpad+newline (cambrian_arch.py:1195-1293) and token emission (:1668-1709).
 * writes: out[i, 0 .. cols) for i < n (pad columns: caller).  reads: the `cols` columns of the table rows `src` names, src[0 .. 2n).
 * scale[k] != NULL (all four NULL, as a zero-initialised struct has them: the form above, unchanged): table k holds OCP e4m3
 * bytes [rows, ld[k]] (ld[k] in BYTES) and scale[k] one fp32 scale per table row (the compact feature store, features.py):
 *   out[i, c] = T16(float(e4m3 table_k[row, c]) * scale_k[row]),  c < cols
 * - one fp32 multiply, one round-to-nearest-even conversion to the call's 16-bit `dtype`; the e4m3 NaN codes give NaN.  One
 * call may mix 16-bit and e4m3 tables.  The e4m3 form
 * writes: out[i, 0 .. cols) only (pad columns: caller), as the 16-bit form.
 * reads: the `cols` BYTES of the table rows `src` names and the scale_k[row] of those rows, src[0 .. 2n) - nothing else: not the
 * bytes cols .. ld[k] behind a row, not the rows or scales `src` does not name.
 * 16-byte stores with 16- or 8-byte loads when cols, ldo, ld[k] and the bases allow it (cols % 8 == 0, ldo % 8 == 0, out 16-byte
 * aligned; ld[k] and base[k] multiples of 16 with cols % 16 == 0, or of 8), element-wise otherwise. */
typedef struct { const void* base[4]; int ld[4]; const float* scale[4]; } tdc_gather_tables;
int tdc_gather_rows(const tdc_gather_tables* t, const int* src, void* out, int ldo, int n, int cols, int dtype,
                    void* stream);
/* every row of out [rows, ld] (16-bit, ld % 8 == 0) := row[0 .. ld) (the SVA queries start as `vision_query` on every
 * window of every frame, cambrian_arch.py:1018-1023).  writes: WHOLE rows, rows * ld elements */
int tdc_fill_rows(const void* row, void* out, int ld, int rows, void* stream);
/* rows of x [rows, ld] 16-bit scaled to unit L2 norm over `cols` (F.normalize, eps 1e-12; cambrian_arch.py:1664).
 * reads and writes x[r, 0 .. cols) in place; the pad columns are neither read nor written */
int tdc_l2_normalize(void* x, int ld, int rows, int cols, int dtype, void* stream);
/* SVA core (tdc/vision_sampler.py:215-291): per query (frame t, window (i,j)) attend over the 2x2 windows of
 * n_towers towers: q [T*side*side, ldq]; kv[tower] [T*(side*r)^2, ldkv] with K at col 0 and V at col `dim`;
 * mask [T*side*side, n_towers*r*r] uint8; out [T*side*side, ldo].  heads x head_dim = dim.
 * writes: out[qi, 0 .. dim) for the T*side*side queries (pad columns: caller - tdc-video_amd/ops.py zeroes them at allocation).
 * Head dims of 8 x a power of two (the path's own: 64) run a fixed-order reduction and are bit-reproducible; any other head dim
 * runs the element-wise kernel, which sums its scores with LDS atomics: NOT bit-reproducible run to run (last-bit differences). */
typedef struct {
    const void* q; int ldq;
    const void* kv[2]; int ldkv;
    const unsigned char* mask;
    void* out; int ldo;
    int T, side, r, n_towers, dim, heads, dtype;
} tdc_sva_attn_desc;
int tdc_sva_attention(const tdc_sva_attn_desc* d, void* stream);
/* Q-Former embeddings (tdc/Qformer.py:78-108): h[f, s] = LN(s < K ? query[qsrc[f], s] : word[ids[s-K]] + pos[s-K])
 * -> h32 [F*(K+Lt), ld] fp32 and h16.  writes: WHOLE rows of both, ld elements (zeros from `cols` on).  reads: the query rows
 * qsrc names, the `word` rows ids names, pos rows 0 .. Lt.
 * Prompt table (frame_prompt != NULL): ids is a [P, ids_ld] table (ids_ld >= Lt), frame f embeds prompt p = frame_prompt[f]:
 * row s >= K is LN(word[ids[p*ids_ld + s-K]] + pos[s-K]) when s-K < prompt_len[p] - bit for bit the single-prompt row - and a
 * WHOLE ZERO row of h32 and h16 otherwise (every frame still occupies K + Lt rows).  writes: the same rows.  reads: frame_prompt
 * [0 .. F), prompt_len[p] and ids[p][0 .. prompt_len[p]) of the prompts frame_prompt names - never the ids behind prompt_len[p],
 * never a prompt no frame names.  The entries are NOT checked on the device: the caller range-checks them. */
typedef struct {
    const void* query; int ldq; const int* qsrc;
    const float* word; const float* pos; int ldw; const int* ids; int Lt;
    const float* gamma; const float* beta; float eps;
    float* h32; void* h16; int ld;
    int F, K, cols, dtype;
    const int* frame_prompt; const int* prompt_len; int ids_ld;   /* prompt table (all NULL / 0: one prompt for every frame) */
} tdc_qembed_desc;
int tdc_qformer_embed(const tdc_qembed_desc* d, void* stream);

/* ---- composite: one ViT tower forward (a2-a4) --------------------------------------------------------------------
 * Replaces SiglipVisionTower._forward / DinoVisionTower._forward (tdc/multimodal_encoder/siglip_encoder.py:71-78,
 * dino_encoder.py:109-120) incl. the HF SiglipVisionModel / Dinov2Model they wrap: patch-embed GEMM (+pos, +cls),
 * n_layers x {LN, qkv GEMM, attention, out GEMM (+residual), LN, fc1 GEMM (+GELU-tanh / SwiGLU), fc2 GEMM (+residual)},
 * optional final LN - with `fused` the two LayerNorms of a block are not kernels: the residual-stream GEMM before them
 * emits the 16-bit row copy + per-slot statistics and the GEMM after them folds (mean, rstd) into its epilogue -, bilinear resample of the token grid (cls dropped).  Weights are the prepared (padded, fused,
 * LayerScale-folded) tensors of tdc-video_amd/weights.py; all pointers are device pointers except `layers`
 * (host array).  The residual stream is fp32 or 16-bit (res_dtype_p1).  Nothing is allocated: the caller passes a workspace of at least
 * tdc_vit_workspace_bytes() bytes (256-byte aligned).  The three composites (tdc_vit_fwd, tdc_qformer_fwd, tdc_connector_fwd)
 * write `out` (WHOLE rows, ldo elements - pad columns zero) and their workspace, never a byte beyond workspace_bytes as queried;
 * the workspace needs NO initialisation: whatever it holds on entry (a previous call's state, NaN patterns) never reaches `out` -
 * buffers inside it that a kernel expects zeroed are zeroed by the composite itself. */
typedef struct { const void* w; const float* b; int n, k; } tdc_lin;      /* w [n, k] 16-bit (padded), b [n] or NULL */
typedef struct {
    const float *ln1_g, *ln1_b, *ln2_g, *ln2_b;
    tdc_lin qkv, out, fc1, fc2;
    /* LayerNorm fusion (tdc_vit_model.fused): row sums of the gamma-folded qkv / fc1 weight (tdc_gemm_desc.ln_c1); the
     * lin's weight is then W diag(gamma) and its bias beta W^T + b.  qkv_c1 == NULL: this layer's LN1 runs as a kernel
     * (layer 0, whose input comes from the patch embedding). */
    const float *qkv_c1, *fc1_c1;
    /* fp8 towers (tdc_vit_model.fp8): qkv.w / fc1.w hold e4m3 bytes [n, round_up(k, 128)] with these per-tensor scales;
     * zeros [>= max n] fp32 zeros (the ln_c1 operand of an fp8-operand tdc_gemm) */
    float qkv_wscale, fc1_wscale; const float* zeros;
    float out_wscale, fc2_wscale;    /* fp8 level 2: out.w / fc2.w are e4m3 too */
    float fc1_w2max, fc1_bmax;       /* fp8 level 3: max row 2-norm of fc1's e4m3 weight (in units of fc1_wscale), max |fc1.b|
                                        (tdc_gemm_desc.out_w2max / out_bmax) */
} tdc_vit_layer;
typedef struct {
    int dtype, dim, heads, head_dim, n_layers, patch, has_cls;
    int act;                         /* TDC_ACT_GELU_TANH (SigLIP), TDC_ACT_SWIGLU / TDC_ACT_GELU_ERF (DINOv2) */
    float eps;
    tdc_lin patch_lin;               /* [pad64(dim), pad64(3*patch*patch)] */
    const float* pos; int ldpos;     /* [P (+1), pad64(dim)] fp32 position rows for this patch grid (row 0 = cls) */
    const float* cls_row;            /* cls + pos[0], [pad64(dim)] (NULL when !has_cls) */
    const float *lnf_g, *lnf_b;      /* final LayerNorm (NULL: take the raw residual stream, SigLIP hidden_states[-1]) */
    const tdc_vit_layer* layers_host;
    int fused;                       /* pre-LayerNorms folded into the qkv / fc1 GEMMs (dim % 64 == 0) */
    int fp8;                         /* 1: the LayerNorms emit e4m3 rows + per-row scales and the qkv / fc1 GEMMs run on fp8
                                        operands (dim % 128 == 0; excludes `fused`); 2: out-proj / fc2 as well, their inputs
                                        (attention output, MLP hidden) quantised per row by tdc_quantize_rows_fp8; 3: as 2, but
                                        fc1 writes the MLP hidden as e4m3 itself (tdc_gemm_desc.out_fp8; needs fc1's output
                                        width == fc2.k) */
    int out_dtype_p1;                /* 16-bit type of tdc_vit_fwd's `out` rows, PLUS ONE: 0 = the same as `dtype` (so a
                                        zero-initialised struct behaves as before the field existed), TDC_F16 + 1 / TDC_BF16 + 1
                                        = that type (the towers - 98 % of the FLOPs - in bf16, the connector and the Q-Former
                                        behind them in fp16: compressed tokens within 1e-3 of the fp32 oracle) */
    int res_dtype_p1;                /* type of the residual stream in HBM: 0 = fp32 (read-modify-write in the out-projection /
                                        fc2 epilogues, 8 B per element), TDC_F16 + 1 / TDC_BF16 + 1 = that 16-bit type (4 B per
                                        element and half the LayerNorm input bytes; fp16 is the reference's own arithmetic: its
                                        HF towers run under torch_dtype=float16, tdc/builder.py:69, residual adds included).
                                        Sums are formed in fp32 and rounded once: x <- T16(acc + bias + float(x)).  With
                                        `fused` (round 6; needs the stream's type == `dtype`): the folded consumers read the
                                        stream itself, the read-modify-write epilogues emit only the per-slot partials and no
                                        LayerNorm kernel runs inside the layer loop.  Excludes `fp8`. */
} tdc_vit_model;
size_t tdc_vit_workspace_bytes(const tdc_vit_model* m, int B, int H, int W);
/* px [B,3,H,W] (px_f32 as in tdc_im2col: 0 = `dtype`, 1 = fp32, 2 = the other 16-bit type) -> out [B*out_grid*out_grid, ldo] 16-bit (`out_dtype_p1`); idx0/idx1/frac: bilinear tables
 * [out_grid] for the (H/patch)-wide grid (device).  H == W required (the reference pads frames to squares). */
int tdc_vit_fwd(const tdc_vit_model* m, const void* px, int px_f32, int B, int H, int W, int out_grid,
                const int* idx0, const int* idx1, const float* frac, void* out, int ldo, void* workspace,
                size_t workspace_bytes, void* stream);

/* ---- composite: the batched Q-Former TDC compressor (a13-a18) -------------------------------------------------------
 * Replaces `Qformer.bert(input_ids, query_embeds, encoder_hidden_states)` + `vision_proj` + `F.normalize`
 * (tdc/cambrian_arch.py:1653-1667, tdc/Qformer.py:804-965) for ALL compressed frames of a video at once:
 * enc [F*Nenc, ldenc] 16-bit (the frames' LLM-space tokens), query [nC*K, ldq] (query_proj of the pooled key frames),
 * qsrc[f] = chunk of frame f, ids[Lt] = BERT prompt ids (Lt may be 0) -> out [F*K, ldo] 16-bit unit-norm context rows.
 * Per layer: fused q|k|v GEMM, self-attention over S = K+Lt rows, dense+residual, LN; even layers: cross-attention of
 * the K query rows against the frame's Nenc tokens (all layers' K/V projections come from ONE stacked GEMM,
 * SURVEY D7); dual FFN (query rows / text rows).  Hidden stream fp32 + 16-bit copy. */
typedef struct {
    tdc_lin qkv, attn_out; const float *attn_ln_g, *attn_ln_b;
    int has_cross, cross_idx;
    tdc_lin cross_q, cross_out; const float *cross_ln_g, *cross_ln_b;
    tdc_lin fq1, fq2; const float *fq_ln_g, *fq_ln_b;      /* intermediate_query / output_query */
    tdc_lin ft1, ft2; const float *ft_ln_g, *ft_ln_b;      /* intermediate / output (text rows) */
    const void *cross_q_tiled, *cross_out_tiled;           /* fragment-major copies of cross_q.w / cross_out.w for the fused block
                                                              (tdc_qformer_xattn_tile_weight), NULL: the per-kernel sequence */
} tdc_qformer_layer;
/* The multi-prompt form of the composite below (tdc_qformer_model.prompts != NULL): P prompts over ONE video in one launch
 * sequence.  The call's F then counts VIRTUAL frames - the compressed frames of prompt 0, then those of prompt 1, ... -, its
 * `enc` holds the enc_frames DISTINCT frames [enc_frames*Nenc, ldenc] that the stacked K/V projection runs over ONCE, its `ids`
 * is the [n_prompts, Lt] table (Lt = the longest prompt) and `out` is [F*K, ldo] in virtual-frame order.  Virtual frame f reads
 * the K/V of distinct frame kv_src[f], embeds prompt frame_prompt[f] of prompt_len[..] ids and self-attends over
 * self_len[f] = K + prompt_len[frame_prompt[f]] of its K + Lt rows; the rows behind are zero-embedded padding that the
 * row-mapped GEMMs / LayerNorms compute and nothing valid reads.  Row block f of `out` is bit for bit what the single-prompt
 * call over that prompt's frames returns for the frame.  All four arrays are device int32, range-checked by the caller
 * (kv_src in [0, enc_frames), frame_prompt in [0, n_prompts), prompt_len in [0, Lt]).  The workspace query reads enc_frames
 * from the model: the K/V buffers are sized by enc_frames, everything else by F.  Runs the default form and xattn_mode 0 / 1;
 * a model and shape that resolve to xattn_mode 2 return TDC_E_BADARG (the whole-block kernel has no per-frame K/V source).
 * reads beyond the single form: kv_src / frame_prompt / self_len [0 .. F), prompt_len[0 .. n_prompts); writes: as the single form. */
typedef struct {
    int n_prompts, enc_frames;
    const int *kv_src, *frame_prompt, *prompt_len, *self_len;
} tdc_qformer_prompts;
typedef struct {
    int dtype, dim, heads, n_layers, H;
    float eps;
    const float *word, *pos; int ldw;
    const float *emb_ln_g, *emb_ln_b;
    tdc_lin cross_kv;                                       /* [n_cross*2*dim, pad64(H)]: (K_j | V_j) per cross layer */
    tdc_lin vision_proj;                                    /* [pad64(H), pad64(dim)] */
    const tdc_qformer_layer* layers_host;
    /* the fused cross-attention block (tdc_qformer_xattn; used when tdc_qformer_xattn_supported() and cross_k.w != NULL):
     * the same projections stacked per kind - cross_k [n_cross*dim, pad64(H)] with its bias, cross_v [n_cross*dim, pad64(H)]
     * WITHOUT bias (it is the A operand of the transposed GEMM V^T = Wv enc^T) and cross_bv [n_cross*dim] fp32 = the value
     * biases, added after the PV product */
    tdc_lin cross_k, cross_v; const float* cross_bv;
    /* how tdc_qformer_fwd runs the cross-attention block when the shape is one tdc_qformer_xattn supports (else 0):
     * 0 = per-kernel sequence; 1 = q GEMM + tdc_attention, then output projection + residual + LayerNorm in one kernel
     * (needs cross_out_tiled); 2 = the whole block in one kernel per layer (needs cross_k / cross_v / both tiled weights) */
    int xattn_mode;
    const tdc_qformer_prompts* prompts;                     /* NULL: one prompt (the form described above) */
    /* kept cross-attention K/V.  kv_keep == NULL (and kv_state 0): the stacked K/V projection writes
     * the workspace's K/V region, as described above.  kv_keep != NULL: a caller-owned, 256-byte aligned buffer
     * [U*Nenc, cross_kv.n] of 16-bit values, row stride cross_kv.n (U = prompts->enc_frames in the multi-prompt form, else F),
     * takes that region's place: the stacked GEMM's C and every cross layer's K / V operands point into it.  The workspace
     * layout and tdc_qformer_workspace_bytes do not change.  kv_state 0 (fill): the composite runs the stacked GEMM into
     * kv_keep - the same launch on the same operands with another C pointer, so the rows are the workspace form's bit for bit.
     * kv_state 1 (ready): kv_keep holds the rows of an earlier fill over the same enc rows and weights; the GEMM is skipped
     * and `enc` may be NULL.  Any other kv_state, a misaligned kv_keep, or kv_state != 0 without kv_keep: TDC_E_BADARG.
     * A model and shape that resolve to xattn_mode 2 return TDC_E_BADARG with kv_keep (the whole-block kernel keeps K and
     * transposed V in two buffers of other shapes); xattn_mode 0 / 1 are served.
     * writes (fill): kv_keep[r, 0 .. cross_kv.n) for r < U*Nenc, nothing else of it.  ready: no byte of kv_keep is written,
     * those rows are read, and no byte of enc is read. */
    void* kv_keep; int kv_state;
} tdc_qformer_model;
size_t tdc_qformer_workspace_bytes(const tdc_qformer_model* m, int F, int K, int Lt, int Nenc);

/* ---- the Q-Former cross-attention block of one layer as ONE kernel (the north_star's kernel) ----------
 * Replaces, for the K query rows of every compressed frame, BertSelfAttention (cross form) + BertSelfOutput
 * (tdc/Qformer.py:128-130,185-188,205-264,285-289, called from BertLayer.forward :432-447):
 *     q = h[:, :K] Wq^T + bq;  ctx = softmax(q_h k_h^T * scale) v_h per head;  h[:, :K] = LayerNorm(ctx Wo^T + bo + h[:, :K])
 * h16 / h32: the 16-bit copy and the fp32 master of the hidden stream [F*S, ldh] (query rows of frame f = rows f*S + [0, K));
 * both are updated in place.  k [F*Nenc, ldk]: this layer's key rows (enc Wk^T + bk; pass the column-offset pointer);
 * vt [dim, ldvt]: this layer's values TRANSPOSED, vt[c][f*Nenc + key] = (enc Wv^T)[f*Nenc + key][c] WITHOUT the bias -
 * i.e. tdc_gemm with A = Wv, W = enc -, ldvt >= round_up(F*Nenc, 8) (with Nenc % 8 == 4 the last, half-valid key group of a
 * frame is read as one 16-byte piece: the last frame's read runs 4 columns past F*Nenc, values unused); bv [dim] fp32 or NULL.  wq / wo: the two [dim, dim] weights in the kernel's
 * FRAGMENT-MAJOR layout, dim*dim 16-bit values each, made once per weight by tdc_qformer_xattn_tile_weight from the
 * nn.Linear layout [dim, ldw] (a wave's MFMA operand is then 1 KiB of consecutive bytes instead of 16 rows x 64 B).
 * Supported: dim == 768, head dim 64, K % 16 == 0, Nenc % 4 == 0, 8 <= Nenc <= 224 (tdc_qformer_xattn_supported); the
 * composite tdc_qformer_fwd falls back to the per-kernel sequence (q GEMM, tdc_attention, dense GEMM, tdc_layernorm) otherwise. */
typedef struct {
    void* h16; float* h32; int ldh;
    int F, K, S;
    const void* wq; const float* bq; const void* wo; const float* bo;
    const void* k; int ldk;
    const void* vt; long long ldvt; const float* bv;
    int Nenc;
    const float *ln_g, *ln_b; float eps;
    int dim, heads; float scale; int dtype;     /* scale: finite and >= 0, as in tdc_attn_desc; the ctx form does not read it */
    /* ctx != NULL: the OUTPUT-PROJECTION-ONLY form - ctx [F*K, ldctx] 16-bit is the attention output of the flat query rows
     * (row f*K + k), produced by separate launches (q GEMM, tdc_attention); the kernel then computes
     * h[:, :K] = LayerNorm(ctx Wo^T + bo + h[:, :K]) alone: wq / bq / k / vt / bv / Nenc / scale are not read. */
    const void* ctx; int ldctx;
    /* res16 != 0 (ctx form only): the residual is the 16-bit hidden state - h16 is read as the residual and only h16 is written;
     * h32 is neither read nor written and may be NULL.  (The arithmetic of the reference's half-precision inference,
     * tdc/Qformer.py:285-289 on 16-bit tensors; half the bytes of the launch.  tdc_qformer_fwd uses it in its default form
     * and carries the query rows in 16 bits from here to the LayerNorm behind the layer's query FFN, which writes both copies again.) */
    int res16;
    /* writes: h16 / h32 [f*S + k, 0 .. dim) for f < F, k < K (h16 only with res16) - the text rows f*S + K .. (f+1)*S, the
     * columns dim .. ldh and the rows behind F*S keep their bytes.  reads: those query rows, k rows 0 .. F*Nenc (columns
     * 0 .. dim), vt[c][0 .. round_up(F*Nenc, 8)) - the documented 4 columns past F*Nenc with Nenc % 8 == 4 are loaded and
     * masked: any bit pattern there, NaN included, leaves the result unchanged -, ctx rows 0 .. F*K. */
} tdc_xattn_desc;
int tdc_qformer_xattn_supported(int dim, int heads, int K, int Nenc);
int tdc_qformer_xattn(const tdc_xattn_desc* d, void* stream);
/* writes: out[0 .. dim*dim).  reads: w[r, 0 .. dim) for r < dim (dim = 768). */
int tdc_qformer_xattn_tile_weight(const void* w, int ldw, void* out, int dtype, void* stream);
int tdc_qformer_fwd(const tdc_qformer_model* m, const void* enc, int ldenc, int F, int Nenc, const void* query, int ldq,
                    const int* qsrc, const int* ids, int Lt, int K, void* out, int ldo, void* workspace,
                    size_t workspace_bytes, void* stream);

/* ---- composite: the connector (a6-a9) -------------------------------------------------------------------------------
 * Replaces mm_projector_aux_{0,1} + global context (tdc/cambrian_arch.py:80-90,1002-1013), the window gather + masks and
 * the 3-layer `vision_sampler_0` (cambrian_arch.py:601-695,1018-1053; tdc/vision_sampler.py:170-401,519-566) and
 * `mm_projector` (cambrian_arch.py:65-69,1149-1150) for T frames: the two towers' tokens sig [T*P, ld_s] / dino
 * [T*P, ld_d] (16-bit, P = (side*r)^2 tokens per frame) -> out [T*side*side, ldo] 16-bit in the LLM width H.
 * mask [T*side*side, 2*r*r] uint8 is the reference's window-validity mask (host geometry: tdc-video_amd/segment.py).
 * Per SVA layer: proj_context once per frame, proj_in split into its query / context column blocks (the context half is a
 * per-frame bias), k|v LayerNorm affines folded into ONE [P-token, 2C] GEMM per tower with the position embedding added
 * inside the LayerNorm launch, tdc_sva_attention, o_proj + residual, LayerNorm, proj_out MLP + residual. */
typedef struct { tdc_lin fc1, fc2; const float *ln_g, *ln_b; } tdc_aux_proj;
typedef struct {
    tdc_lin proj_context, proj_in_c, proj_in_q;
    const float* pos[2]; int ldpos;                  /* pos_embed_{0,1} [r*r, pad64(C)] fp32 */
    tdc_lin kv[2];                                   /* (K | V) projection of tower i, LayerNorm affines folded */
    const float *q_ln_g, *q_ln_b; tdc_lin q_proj, o_proj;
    const float *norm_g, *norm_b; tdc_lin out1, out2;
} tdc_sva_layer;
typedef struct {
    int dtype, C, side, r, heads, n_layers;
    tdc_aux_proj aux[2];
    const void* vision_query;                        /* [pad64(C)] 16-bit, pad columns zero */
    const float *ones_C, *zeros_C;                   /* [pad64(C)] (the un-affine LayerNorm of the k/v inputs) */
    const tdc_sva_layer* layers_host;
    tdc_lin mm1, mm2;                                /* mm_projector: Linear(C, H) + GELU, Linear(H, H) */
    /* kept aux rows.  All three NULL: the aux LayerNorm rows of tower i and the per-frame mean of tower
     * 0's rows live in the workspace, as described above.  All three set: caller-owned, 256-byte aligned buffers of 16-bit
     * values take those regions' place - aux_keep[i] [T*P, pad64(C)] and ctx_keep [T, pad64(C)], row stride pad64(C).  The aux
     * LayerNorm writes aux_keep[i], tdc_token_mean reads aux_keep[0] and writes ctx_keep, and every later reader (each layer's
     * un-affine LayerNorm, each layer's proj_context GEMM) reads them there: the same launches on the same operands with
     * other pointers, so the rows are the workspace form's bit for bit and `out` is too.  The workspace layout and
     * tdc_connector_workspace_bytes do not change.  Some but not all of the three set, or a misaligned one: TDC_E_BADARG before
     * the first launch.
     * writes: exactly the elements the workspace regions received - aux_keep[i][row, 0 .. pad64(C)) for row < T*P (pad columns
     * zero, as tdc_layernorm leaves them) and ctx_keep[t, 0 .. pad64(C)) for t < T -, nothing else of them. */
    void* aux_keep[2]; void* ctx_keep;
} tdc_connector_model;
size_t tdc_connector_workspace_bytes(const tdc_connector_model* m, int T);
int tdc_connector_fwd(const tdc_connector_model* m, const void* sig, int ld_s, const void* dino, int ld_d, int T,
                      const unsigned char* mask, void* out, int ldo, void* workspace, size_t workspace_bytes,
                      void* stream);

/* ---- frame pre-processing on the device -----------------------------------------------------------
 * `process_images` for ONE tower (tdc/mm_datautils.py:270-314): frames uint8 [T, H, W, 3] (RGB, as decord / numpy give
 * them) -> expand2square with the pad colour -> Pillow `Image.resize((R, R))` (bicubic with antialiasing, 8 bpc:
 * byte-exact, same 22-bit fixed-point coefficients / pass order / uint8 intermediate as Resample.c) -> per-channel
 * table lut[c*256 + v] = ((v / 255) - mean[c]) / std[c] (fp32, built by the host exactly as the HF image processor
 * computes it) -> out [T, 3, R, R] 16-bit (or fp32).  bounds [R, 2] / coeffs [R, ksize] int32 are Resample.c's
 * precompute_coeffs + normalize_coeffs_8bpc for max(H,W) -> R (tdc-video_amd/preprocess.py).  scratch:
 * tdc_preprocess_scratch_bytes() bytes.  writes: out [T, 3, R, R] and the scratch (contents on entry do not matter);
 * reads: the T frames, bounds / coeffs rows 0 .. R, lut[0 .. 768). */
size_t tdc_preprocess_scratch_bytes(int T, int H, int W, int R);
int tdc_preprocess_frames(const unsigned char* frames, int T, int H, int W, int R, const int* bounds, const int* coeffs,
                          int ksize, int pad_r, int pad_g, int pad_b, const float* lut, void* out, int out_f32,
                          int dtype, unsigned char* scratch, void* stream);

/* ---- YUV 4:2:0 -> RGB ------------------------------------------------------------------------
 * T frames of 8-bit 4:2:0 (NV12 / NV21 as a hardware decoder writes them, planar I420 as a software decoder does) ->
 * rgb uint8 [T, H, W, 3] contiguous, what tdc_preprocess_frames takes.  Pixel (y, x) takes luma Y[y, x] and the chroma
 * sample (U, V)[y >> 1, x >> 1] (replication); the chroma planes have Hc = (H + 1) / 2 rows of Wc = (W + 1) / 2 samples.
 * With Y' = Y - y_off, Cb = U - 128, Cr = V - 128, in int32 (>> arithmetic, clip8 to [0, 255]):
 *     R = clip8((cy*Y' + crv*Cr          + 32768) >> 16)
 *     G = clip8((cy*Y' - cgu*Cb - cgv*Cr + 32768) >> 16)
 *     B = clip8((cy*Y' + cbu*Cb          + 32768) >> 16)
 * The coefficients are the host's: floor(real * 65536 + 0.5) of the matrix and range it chose (preprocess.yuv_coefficients).
 * This entry is tdc_yuv_to_rgb (below) at bits = 8, 4:2:0: the same refusals, the same choice of form and the same grid,
 * in front of a kernel written out for bytes.
 * One kernel serves every layout through the two chroma pointers and c_step; the host picks its 8-pixel vector form when W,
 * the pointers, the pitches and the frame strides are multiples of the access widths (8 bytes luma and rgb; chroma 4 bytes
 * each planar, or 8 bytes at the lower pointer when u and v are neighbours), its 2 x 2 byte form otherwise: same bytes.
 * TDC_E_BADARG before any launch: a null pointer; T, H or W outside [1, 65535]; c_step not 1 or 2; y_pitch < W; c_pitch <
 * c_step * Wc; for T > 1 a frame stride that does not clear the plane's last row; y_off not 0 or 16; a coefficient outside
 * [0, 2^18] (the accumulators then stay below 2^28 for every input byte).
 * writes: rgb [T, H, W, 3] and nothing else.  reads: W bytes of each of the H luma rows and, of each of the Hc chroma rows,
 * c_step * (Wc - 1) + 1 bytes from u and from v.  never read: pitch padding, the rows between a plane's end and the next
 * frame. */
typedef struct {
    const unsigned char *y, *u, *v;   /* first byte of frame 0's planes; NV12: u = uv, v = uv + 1 (NV21: the other way) */
    long long y_frame, c_frame;       /* bytes from one frame's plane to the next frame's (u and v share c_frame) */
    int y_pitch, c_pitch;             /* bytes per plane row */
    int c_step;                       /* bytes between chroma samples of a row: 1 planar (I420), 2 interleaved (NV12) */
} tdc_yuv420_planes;
typedef struct { int y_off, cy, crv, cgu, cgv, cbu; } tdc_yuv_coef;      /* host struct, passed by value into the kernel */
int tdc_yuv420_to_rgb(const tdc_yuv420_planes* p, const tdc_yuv_coef* c, int T, int H, int W,
                      unsigned char* rgb /* [T, H, W, 3] contiguous */, void* stream);

/* ---- YUV -> RGB at 8, 10 and 12 bits, 4:2:0 / 4:2:2 / 4:4:4 -----------------------------------
 * The surfaces the entry above does not take: P010 / P012 / P016 (16-bit words, the sample in the high bits), planar or
 * interleaved yuv4xxp10le / 12le (the sample in the low bits), 8-bit 4:2:2 and 4:4:4.  Same output, same replication, and at
 * bits = 8, 4:2:0 the same bytes as the entry above.  With s = bits - 8:
 *   sample   a byte at bits = 8, else a little-endian 16-bit word w taken as (w >> shift) & (2^bits - 1), shift = 16 - bits
 *            when msb_aligned and 0 otherwise: the bits outside the sample are ignored, whatever they hold
 *   chroma   pixel (y, x) takes (U, V)[y >> sub_y, x >> sub_x]; the chroma planes have Hc = (H + sub_y) >> sub_y rows of
 *            Wc = (W + sub_x) >> sub_x samples; (sub_x, sub_y) is (1, 1) 4:2:0, (1, 0) 4:2:2 or (0, 0) 4:4:4
 *   Y' = Y - y_off, Cb = U - 2^(bits-1), Cr = V - 2^(bits-1), in int32 (>> arithmetic, clip8 to [0, 255]):
 *     R = clip8((cy*Y' + crv*Cr          + 2^(15+s)) >> (16+s))
 *     G = clip8((cy*Y' - cgu*Cb - cgv*Cr + 2^(15+s)) >> (16+s))
 *     B = clip8((cy*Y' + cbu*Cb          + 2^(15+s)) >> (16+s))
 * The coefficients are the host's (preprocess.yuv_coefficients with its bits argument); y_off is 0 or 16 << s.  The transfer
 * function is not touched: PQ or HLG samples come out as PQ or HLG bytes (tdc_yuv_hdr_to_rgb below tone-maps them).
 * A thread owns (1 + sub_y) rows, so a chroma sample is loaded once.  The host picks the 8-pixel vector form when W % 8 == 0
 * and the pointers, the pitches and (T > 1) the frame strides are multiples of the access widths - luma 8 bytes (bits = 8) or
 * 16 (words), rgb 8, chroma the 8 >> sub_x samples of one plane in one load, or that many pairs at the lower pointer when u
 * and v are neighbours (32 bytes: aligned to 16) - and the form of one sample per load otherwise: same bytes.
 * TDC_E_BADARG before any launch: what the entry above refuses (with the pitches and frame strides measured in bytes); bits
 * not 8, 10 or 12; another (sub_x, sub_y); msb_aligned not 0 or 1, or 1 at bits = 8; c_step not one or two sample sizes;
 * y_off not 0 or 16 << s; at 16-bit samples an odd pointer, pitch, frame stride or c_step; y_pitch below W samples, c_pitch
 * below c_step * Wc; for T > 1 a frame stride that does not clear the plane's last row; a coefficient outside [0, 2^18], or
 * cy * 2^bits + max(crv, cgu + cgv, cbu) * 2^(bits-1) + 2^(15+s) >= 2^31 (an accumulator could leave int32; coefficients
 * inside [0, 2^18] stay below 2^30 + 2^29 + 2^19 at 12 bits, so the first check already implies this one).
 * writes: rgb [T, H, W, 3] and nothing else.  reads: the W samples of each of the H luma rows and, of each of the Hc chroma
 * rows, c_step * (Wc - 1) + sample size bytes from u and from v.  never read: pitch padding, the rows between a plane's end
 * and the next frame. */
typedef struct {
    const unsigned char *y, *u, *v;   /* first byte of frame 0's planes; interleaved: u and v one sample apart, either order */
    long long y_frame, c_frame;       /* bytes from one frame's plane to the next frame's (u and v share c_frame) */
    int y_pitch, c_pitch;             /* bytes per plane row */
    int c_step;                       /* bytes between chroma samples of a row: one sample size planar, two interleaved */
    int bits;                         /* significant bits of a sample: 8 (bytes), 10 or 12 (16-bit words) */
    int msb_aligned;                  /* 16-bit words: 1 = the sample is the word's high bits (P010), 0 = its low bits */
    int sub_x, sub_y;                 /* chroma sub-sampling shifts */
} tdc_yuv_planes;
int tdc_yuv_to_rgb(const tdc_yuv_planes* p, const tdc_yuv_coef* c, int T, int H, int W,
                   unsigned char* rgb /* [T, H, W, 3] contiguous */, void* stream);

/* ---- HDR YUV -> SDR RGB: PQ / HLG surfaces of 10 or 12 bits tone-mapped to sRGB bytes ------------
 * The surfaces, the sample extraction, the sub-sampling, the replicated chroma, the thread ownership and the two kernel forms
 * are those of the entry above; bits is 10 or 12.  The project's own stated formula, not claimed equal to any library's tone
 * mapper.  s = bits - 8, N = 2^bits - 1.
 * Stage A, int32, exact - YCbCr to non-linear R'G'B' codes at full depth, Y', Cb, Cr as above (clipN to [0, N], the clamp
 * taken on the accumulator before the shift):
 *     E_R = clipN((cy*Y' + crv*Cr          + 32768) >> 16)
 *     E_G = clipN((cy*Y' - cgu*Cb - cgv*Cr + 32768) >> 16)
 *     E_B = clipN((cy*Y' + cbu*Cb          + 32768) >> 16)
 *   with the coefficients of preprocess.yuv_code_coefficients: floor(real * 65536 + 0.5) of the matrix factors times the luma
 *   scale N / (219 << s) and the chroma scale N / (224 << s) (limited range; both 1 at full range).
 * Stage B, float32 (defined in fp64 over the same float32 table):
 *   1. l_c = lut[E_c].  PQ: lut[i] = 10000 * PQ_EOTF(i / N) / white (ST 2084; linear light in units of SDR white).
 *      HLG: lut[i] = the BT.2100 inverse OETF of i / N (scene light in [0, 1]).
 *   2. HLG only (ootf_exp != 0): Ys = luma . l;  g = ootf_scale * Ys^ootf_exp for Ys > 0 and g = 0 for Ys = 0;  l_c <- g * l_c
 *      (the BT.2100 OOTF: ootf_scale = peak / white, ootf_exp = gamma - 1, gamma = 1.2 + 0.42 * log10(peak / 1000)).
 *   3. m = max(l_R, l_G, l_B);  f = (1 + m * inv_p2) / (1 + m);  l_c <- f * l_c   (extended Reinhard on the largest channel,
 *      inv_p2 = (white / peak)^2: slope 1 at black, monotone, m = peak / white goes to 1; the hue is kept).
 *   4. x = gamut * l   (row-major 3 x 3: BT.2020 -> BT.709 primaries, or the identity).
 *   5. x clipped to [0, 1];  v = 12.92 x for x <= 0.0031308, else 1.055 x^(1/2.4) - 0.055 (the sRGB OETF);  the byte is
 *      floor(255 v + 0.5).
 * Stage A is bit for bit the integer formula; every byte is within 1 of the definition (a float32 evaluation within 0.5 of
 * the fp64 one on the 0 .. 255 scale moves the rounded byte by at most 1).  The powers are exp2(k * log2(x)) on the hardware
 * instructions; both kernel forms run one device function per pixel and give the same bytes.
 * TDC_E_BADARG before any launch: everything the entry above refuses; bits = 8; a null descriptor; lut null or not 4-byte
 * aligned; a non-finite float in the descriptor; inv_p2 outside (0, 1]; ootf_exp outside [0, 1); ootf_scale <= 0 when
 * ootf_exp != 0.
 * writes: rgb [T, H, W, 3] and nothing else.  reads: what the entry above reads, plus exactly 2^bits floats at lut. */
typedef struct {
    const float* lut;       /* device: 2^bits entries, code -> light */
    float ootf_scale;       /* HLG: peak / white */
    float ootf_exp;         /* HLG: gamma - 1; 0: no OOTF (PQ) */
    float luma[3];          /* the luminance weights of the OOTF */
    float inv_p2;           /* (white / peak)^2 */
    float gamut[9];         /* row-major 3 x 3, applied to linear light */
} tdc_hdr_desc;             /* host struct, passed by value into the kernel */
int tdc_yuv_hdr_to_rgb(const tdc_yuv_planes* p, const tdc_yuv_coef* c, const tdc_hdr_desc* h, int T, int H, int W,
                       unsigned char* rgb /* [T, H, W, 3] contiguous */, void* stream);

/* ---- packed YUV -> RGB: YUY2, UYVY, Y210, AYUV, Y410, Y416, v210 -------------------------------
 * Surfaces in which luma and chroma share one row, little-endian.  A row is a run of groups; a group of P pixels is
 *   TDC_YUVP_YUYV / YVYU / UYVY / VYUY   4 bytes, P = 2, in the order the name spells (YUYV = Y0 U Y1 V: YUY2)       bits 8
 *   TDC_YUVP_Y210                        4 16-bit words Y0 U Y1 V, P = 2 (Y210, Y212, a Y216 container)               bits 10, 12
 *   TDC_YUVP_VUYA / AYUV                 4 bytes, P = 1: V U Y A (Microsoft AYUV, VUYX) or A Y U V; A is ignored       bits 8
 *   TDC_YUVP_Y410                        one 32-bit word, P = 1: U = bits 0-9, Y = 10-19, V = 20-29, 30-31 ignored     bits 10
 *   TDC_YUVP_Y416                        4 16-bit words U Y V A, P = 1 (Y412, a Y416 container); A is ignored          bits 10, 12
 *   TDC_YUVP_V210                        four 32-bit words, P = 6: w0 = Cb0 | Y0<<10 | Cr0<<20, w1 = Y1 | Cb1<<10 | Y2<<20,
 *                                        w2 = Cr1 | Y3<<10 | Cb2<<20, w3 = Y4 | Cr2<<10 | Y5<<20; bits 30-31 ignored     bits 10
 * A 16-bit word holds its sample as in tdc_yuv_planes: (w >> shift) & (2^bits - 1), shift = 16 - bits when msb_aligned, else 0.
 * A row's read set is its ceil(W / P) whole groups.  Pixel (y, x) takes the luma of its position and the chroma pair of its
 * group (4:2:2 and v210: pair x >> 1), replicated as in the entries above.
 * h == NULL: the bytes are exactly those tdc_yuv_to_rgb writes for the same samples held in planes of `bits`, 4:2:2 or
 * 4:4:4.  h != NULL (bits 10 or 12): exactly those of tdc_yuv_hdr_to_rgb.  The kernels run the same per-pixel device code.
 * The host picks the form from alignment facts alone, same bytes: the group form (a thread owns one group of one row:
 * byte, 16-bit or 32-bit loads, byte stores; any W, pitch, view and frame offset), or the vector form when W % 8 == 0 (v210:
 * also W >= 24), base, pitch and (T > 1) frame stride are multiples of 16 and rgb of 8: eight pixels per thread (v210: 24) in
 * 16-byte loads and 8-byte stores; what is left of a v210 row after its W / 24 such units (8 or 16 pixels) goes group by
 * group, one 16-byte load each.
 * TDC_E_BADARG before any launch: a null pointer (p, c, rgb, p->base); T, H or W outside [1, 65535]; an unknown format;
 * bits the format does not take (above); msb_aligned not 0 or 1, or 1 for anything but Y210 / Y416; a base, pitch or frame
 * stride that is not a multiple of the word size (2 for Y210 / Y416, 4 for Y410 / V210); pitch below the row's read set;
 * for T > 1 a frame stride that does not clear the last row; the coefficient and y_off checks of tdc_yuv_to_rgb; with h:
 * bits = 8 and everything tdc_yuv_hdr_to_rgb refuses about the descriptor.
 * writes: rgb [T, H, W, 3] and nothing else.  reads: the ceil(W / P) groups of each of the H rows, plus - with h - exactly
 * 2^bits floats at h->lut.  never read: pitch padding, the bytes between a frame's last row and the next frame.  read, but
 * changing nothing: alpha, bits 30-31, the bits of a word outside the sample, the unused tail of a row's last group. */
enum { TDC_YUVP_YUYV = 0, TDC_YUVP_YVYU = 1, TDC_YUVP_UYVY = 2, TDC_YUVP_VYUY = 3, TDC_YUVP_Y210 = 4, TDC_YUVP_VUYA = 5,
       TDC_YUVP_AYUV = 6, TDC_YUVP_Y410 = 7, TDC_YUVP_Y416 = 8, TDC_YUVP_V210 = 9 };
typedef struct {
    const unsigned char* base;        /* first byte of frame 0 */
    long long frame;                  /* bytes from frame to frame */
    int pitch;                        /* bytes per row */
    int format;                       /* TDC_YUVP_* */
    int bits;                         /* significant bits of a sample */
    int msb_aligned;                  /* 16-bit words: 1 = the sample is the word's high bits, 0 = its low bits */
} tdc_yuv_packed;           /* host struct, passed by value into the kernel */
int tdc_yuv_packed_to_rgb(const tdc_yuv_packed* p, const tdc_yuv_coef* c, const tdc_hdr_desc* h /* NULL: SDR */,
                          int T, int H, int W, unsigned char* rgb /* [T, H, W, 3] contiguous */, void* stream);

/* ---- YUV 4:2:0 / 4:2:2 -> RGB with interpolated chroma, sited ---------------------------------------
 * The entries above rebuild full-resolution chroma by replication.  These two interpolate it linearly per axis, on the chroma
 * SAMPLES, at the samples' depth and before anything else; the per-pixel formula of tdc_yuv_to_rgb (h == NULL) or stage A and
 * B of tdc_yuv_hdr_to_rgb (h != NULL, bits 10 or 12) then runs unchanged on the result.  The project's own stated formula,
 * not claimed equal to any library's scaler.
 * Per axis that is sub-sampled by 2, position p has k = p >> 1 and n chroma samples on that axis (Wc = (W + 1) >> 1 across,
 * Hc = (H + 1) >> 1 down); it takes two taps with weights in quarters, the indices clamped to [0, n - 1]:
 *     siting of the axis                                              even p                    odd p
 *     0 co-sited: sample k sits on luma 2k                            4 C[k]                    2 C[k] + 2 C[min(k+1, n-1)]
 *     1 centred:  sample k sits midway between luma 2k and 2k + 1     3 C[k] + C[max(k-1, 0)]   3 C[k] + C[min(k+1, n-1)]
 * An axis that is not sub-sampled (the rows of 4:2:2) has weight 4 on its own sample and its siting is ignored.  The 2-D
 * weight is the product of the two axes' weights - four taps, in sixteenths, summing to 16 - and the sum is rounded once:
 *     C'(y, x) = (sum w_ij * C_ij + 8) >> 4        in int32, for U and V alike
 * C' takes the place of the replicated sample: the bytes are exactly those the replicate entries write for 4:4:4 planes
 * holding C'.  (sit_x, sit_y) of ffmpeg's / H.273's chroma_sample_loc_type: left (0, 1) - MPEG-2, H.264, HEVC 4:2:0; center
 * (1, 1) - JPEG, MPEG-1; topleft (0, 0) - BT.2020 UHD; top (1, 0).  4:2:2 from SDI is sit_x = 0.
 * tdc_yuv_linear_to_rgb takes every tdc_yuv_planes the planar entries take at 4:2:0 or 4:2:2, 8-bit 4:2:0 included;
 * tdc_yuv_packed_linear_to_rgb takes the 4:2:2 formats YUYV, YVYU, UYVY, VYUY, Y210 and V210.  Thread ownership, the forms and
 * the alignment facts that choose between them are those of the replicate entry of the same surface; all forms give the same
 * bytes.  A thread loads its own run of chroma samples in every chroma row it needs as the replicate kernel does, and the
 * one sample left (centred) and right of the run as single-sample loads.
 * TDC_E_BADARG before any launch: a null s; sit_x or sit_y not 0 or 1; a 4:4:4 surface (sub_x = 0; VUYA, AYUV, Y410, Y416);
 * everything the replicate entry of the same surface refuses - tdc_yuv_to_rgb, tdc_yuv_packed_to_rgb - and, with h,
 * bits = 8 and everything tdc_yuv_hdr_to_rgb refuses about the descriptor.
 * writes: rgb [T, H, W, 3] and nothing else.  reads: EXACTLY the read set of the replicate entry of the same surface (plus,
 * with h, the 2^bits floats at h->lut): every neighbour is clamped by index on the picture's own Wc and Hc.  never read: pitch
 * padding, the bytes between a plane's or frame's end and the next frame, a neighbour from frame t - 1 or t + 1.  read, but
 * changing nothing: the bits of a word outside the sample, the unused tail of a packed row's last group. */
typedef struct { int sit_x, sit_y; } tdc_chroma_site;    /* 0 co-sited, 1 centred; host struct, passed by value into the kernel */
int tdc_yuv_linear_to_rgb(const tdc_yuv_planes* p, const tdc_yuv_coef* c, const tdc_hdr_desc* h /* NULL: SDR */,
                          const tdc_chroma_site* s, int T, int H, int W, unsigned char* rgb /* [T, H, W, 3] contiguous */,
                          void* stream);
int tdc_yuv_packed_linear_to_rgb(const tdc_yuv_packed* p, const tdc_yuv_coef* c, const tdc_hdr_desc* h /* NULL: SDR */,
                                 const tdc_chroma_site* s, int T, int H, int W, unsigned char* rgb /* [T, H, W, 3] contiguous */,
                                 void* stream);

/* ---- display orientation of decoded RGB frames -------------------------------------------------
 * A decoder writes the coded picture; the orientation travels beside it (the display matrix or `rotate` tag of MP4 / MOV,
 * the EXIF orientation of a still).  src uint8 [T, H, W, 3] contiguous, the stored frames S -> dst uint8 [T, H', W', 3]
 * contiguous, the upright frames O, what tdc_preprocess_frames takes.  quarters = the clockwise quarter turns that make
 * the stored frame upright (rotate / 90), then hflip mirrors left-right:
 *     quarters 0: O[y, x] = S[y, x]               (H', W') = (H, W)
 *     quarters 1: O[y, x] = S[H-1-x, y]           (H', W') = (W, H)
 *     quarters 2: O[y, x] = S[H-1-y, W-1-x]       (H', W') = (H, W)
 *     quarters 3: O[y, x] = S[x, W-1-y]           (H', W') = (W, H)
 *     hflip:      O'[y, x] = O[y, W'-1-x]
 * the eight elements of the dihedral group; a vertical flip is (2, 1); (0, 0) is a plain copy.  A permutation of bytes:
 * exact, the three bytes of a pixel stay in order.  quarters 1 and 3 move tiles of 64 x 64 pixels through LDS, read along
 * source rows and written along destination rows; quarters 0 and 2 move rows, the pixel order reversed where needed.  The
 * host picks 4-byte accesses where the pointer and the row length in bytes are multiples of 4 (the transposing cases:
 * src and 3 W for the loads, dst and 3 H for the stores, each on its own; the others: src, dst and 3 W together), byte
 * accesses otherwise: same bytes.  Every byte offset is 64-bit.
 * TDC_E_BADARG before any launch: a null pointer; T, H or W outside [1, 65535]; quarters outside 0 .. 3; hflip outside
 * {0, 1}; src [0, 3 T H W) and dst [0, 3 T H W) overlapping.
 * writes: dst [0, 3 T H W) and nothing else.  reads: src [0, 3 T H W) and nothing else. */
int tdc_orient_frames(const unsigned char* src /* [T, H, W, 3] contiguous */, int T, int H, int W,
                      int quarters /* 0..3 clockwise */, int hflip /* 0 / 1 */,
                      unsigned char* dst /* [T, H', W', 3] contiguous */, void* stream);

/* ---- channel-first, BGR, RGBA and gray frames to packed RGB ------------------------------------
 * Decoded pictures in the layouts decoders, capture and image readers write, described by a base pointer, three byte
 * strides (frame, row, pixel) and the byte offsets chan[0..2] of the R, G and B sample inside a pixel, all non-negative:
 *     O[t, y, x, c] = src[t*frame_stride + y*row_stride + x*pixel_stride + chan[c]]     c = 0, 1, 2 (R, G, B)
 * O uint8 [T, H, W, 3] contiguous, what tdc_preprocess_frames takes.  Channel-first [T, C, H, W]: pixel_stride 1, chan =
 * the plane stride times the plane's number; BGRA: 4, (2, 1, 0); ARGB: 4, (1, 2, 3); BGR: 3, (2, 1, 0); gray: 1, (0, 0, 0);
 * gray + alpha interleaved: 2, (0, 0, 0).  A row pitch, an aligned surface height and a crop are strides and a base.  An
 * ignored channel (alpha, X) is no part of the result; alpha is dropped, not composited; gray is replicated.  Exact: every
 * output byte is a copy of one input byte.  Forms, chosen on the host from the descriptor alone and moving the same bytes:
 * four pixels per thread with 4-byte loads (pixel_stride 1: one per distinct channel offset; 3 and 4 with every chan <
 * pixel_stride: the four pixels' 12 or 16 bytes, 16 as one load where aligned) and three 4-byte stores when W, dst, the
 * source pointer (pixel_stride 1: plus each chan), row_stride and frame_stride are multiples of 4; one pixel per thread
 * with byte accesses otherwise.  Every byte offset is 64-bit.
 * TDC_E_BADARG before any launch: a null s, s->src or dst; T, H or W outside [1, 65535]; a stride or an offset that is
 * negative or above 2^40; dst [0, 3 T H W) overlapping the source extent, which runs from src + min(chan) to the last
 * byte of the last pixel's sample (of its group of pixel_stride bytes where pixel_stride is 3 or 4 and every chan <
 * pixel_stride).
 * writes: dst [0, 3 T H W) and nothing else.  reads: the three sample bytes of each pixel (t, y, x) of [0, T) x [0, H) x
 * [0, W); where pixel_stride is 3 or 4 and every chan < pixel_stride, the pixel_stride bytes of that pixel's group (an
 * ignored byte may be read; its value changes nothing); nothing else - no pitch padding, no other row or frame, no byte
 * before a row's first group or after its last. */
typedef struct {
    const unsigned char* src;
    long long frame_stride, row_stride, pixel_stride;     /* bytes */
    long long chan[3];                                    /* byte offsets of R, G, B */
} tdc_rgb_source;
int tdc_pack_rgb(const tdc_rgb_source* s, int T, int H, int W, unsigned char* dst /* [T, H, W, 3] contiguous */, void* stream);

/* ---- one field of interlaced video rebuilt to a full-height frame ------------------------------
 * An interlaced picture holds two fields taken at two moments; one of them, kept alone, is a half-height picture without
 * the double image.  src: the kept field's RGB picture F, Hf rows of W pixels per frame, sample c of field pixel (t, k, x)
 * at src + t * frame_stride + k * row_stride + 3 x + c (byte strides: 3 W for a dense field picture, 6 W for the field of
 * an interleaved RGB frame read where it lies) -> dst uint8 [T, 2 Hf, W, 3] contiguous, the rebuilt frames O, what
 * tdc_preprocess_frames takes.  parity = 0: the field is the even rows of the frame (the top field), 1: the odd rows.
 * With cl(i) = min(max(i, 0), Hf - 1), per byte:
 *     O[2k + parity]      = F[k]                                                        the kept rows: exact copies
 *     O[2k + 1 - parity], with m = k - parity:
 *         fill 0 (linear):  (F[cl(m)] + F[cl(m+1)] + 1) >> 1
 *         fill 1 (cubic):   clip_0_255((9 * (F[cl(m)] + F[cl(m+1)]) - F[cl(m-1)] - F[cl(m+2)] + 8) >> 4)
 * the two-tap mean and the (-1, 9, 9, -1) / 16 half-sample filter, both in integers; a constant column stays constant.
 * The cubic sum lies in [-502, 4598]: every negative sum clips to 0 whichever way a shift of a negative number rounds, so
 * that rounding is no part of the definition.  A stated formula, no library's deinterlacer.
 * A thread owns a column of 16, 4 or 1 bytes of the row and walks a run of 16 field rows, the filter's window held in
 * registers and slid down; the host picks the column width from the alignment of src, both strides, dst and 3 W alone
 * (all multiples of 16: 16 bytes; of 4: 4 bytes; otherwise bytes; frame_stride at T = 1 and row_stride at Hf = 1 are never
 * applied and are left out) and the forms produce the same bytes.  Every byte
 * offset is 64-bit.
 * TDC_E_BADARG before any launch: a null pointer; T or W outside [1, 65535]; Hf outside [1, 32767]; parity or fill
 * outside {0, 1}; a stride that is negative or above 2^40; row_stride < 3 W; frame_stride < (Hf - 1) * row_stride + 3 W;
 * dst [0, 6 T Hf W) overlapping the source extent [src, src + (T - 1) * frame_stride + (Hf - 1) * row_stride + 3 W).
 * writes: dst [0, 6 T Hf W) and nothing else.  reads: the 3 W bytes of each of the Hf rows of each of the T frames and
 * nothing else - never the gap between two rows, where the other field lies, nor the pitch padding, nor another frame. */
int tdc_field_to_frame(const unsigned char* src, long long frame_stride, long long row_stride /* bytes */,
                       int T, int Hf, int W, int parity /* 0: field on even rows, 1: odd */, int fill /* 0 linear, 1 cubic */,
                       unsigned char* dst /* [T, 2 Hf, W, 3] contiguous */, void* stream);

/* ---- BEATs audio front end --------------------------------------------------------------------------
 * kaldi fbank as BEATs.preprocess calls it (tdc/audio_models/beats/BEATs.py:115-129: torchaudio.compliance.kaldi.fbank,
 * 128 mel bins, 16 kHz, 25 ms / 10 ms, povey window, pre-emphasis 0.97, DC removal, dither 0, snip_edges) on B
 * equal-length waveforms wav [B, n_samples] (fp16 or fp32, amplitude +-1; item stride wav_bs), followed by
 * (x - mean) * inv_scale.  Host-built fp32 tables: window [400], twiddle [256][2] (cos, sin of 2 pi k / 512), banks
 * [128][257], range [128][2] (non-zero span of each mel row).  Outputs (either may be NULL): plain fp32
 * [B, frames, 128]; patches 16-bit [B * (frames/16) * 8, ldp] = the im2col of the 16x16 / stride-16 patch conv
 * (BEATs.py:145-148), row (frame/16)*8 + mel/16, column (frame%16)*16 + mel%16.  tdc_fbank_frames(n) = frame count.
 * writes: plain [B, frames, 128]; patches rows 0 .. B*(frames/16)*8, columns 0 .. 256.  reads: n_samples samples per item. */
int tdc_fbank_frames(long long n_samples);
int tdc_fbank(const void* wav, int wav_f32, long long n_samples, long long wav_bs, int B, const float* window,
              const float* twiddle, const float* banks, const int* range, float* plain, void* patches, int ldp,
              int dtype, float mean, float inv_scale, void* stream);
/* gate of the gated relative position bias (backbone.py:652-657): q [rows, ldq] 16-bit (heads x head_dim columns, the
 * un-scaled q_proj output); w2 [2, head_dim], b2 [2] = grep_linear rows / biases summed in groups of 4; grep_a
 * [heads]; gate [rows, ldg] fp32 = ga * (gb * grep_a[h] - 1) + 2.  Consumed by tdc_attention's `gate`.
 * writes: gate[r, 0 .. heads) for r < rows (columns heads .. ldg: caller). */
int tdc_relpos_gate(const void* q, int ldq, int rows, int heads, int head_dim, const float* w2, const float* b2,
                    const float* grep_a, float* gate, int ldg, int dtype, void* stream);

/* ---- decoded PCM -> the mono 16 kHz waveform tdc_fbank takes -----------------------------------
 * What a decoder hands over (interleaved s16, planar float32, any channel count, 8 .. 192 kHz) resampled to 16 kHz by the
 * project's own stated formula, not claimed equal to librosa's, soxr's or any library's.  For an input rate sr (integer Hz):
 * g = gcd(sr, 16000), L = 16000 / g, M = sr / g.  With rolloff = 0.9, Z = 32 zero crossings, Kaiser beta = 8.0:
 *     c = rolloff * min(1, 16000 / sr)            cutoff, as a fraction of the input Nyquist
 *     W = Z / c                                   half-width in input samples;  K = ceil(W)
 *     h(tau) = c * sinc(c * tau) * I0(beta * sqrt(1 - (tau / W)^2)) / I0(beta)   for |tau| < W, else 0;  sinc(x) = sin(pi x) / (pi x)
 *     table[p][j] = h(p / L - j),  j = -K+1 .. K (column j + K - 1),  p = 0 .. L-1
 *     y[n] = sum_j table[(n M) mod L][j] * x[floor(n M / L) + j]
 * Each row table[p] is divided by its own sum (DC gain exactly 1); the table is built in float64 and rounded once to float32
 * (audio.resample_tables).  x is 0 outside [0, n_in); n M is computed in 64 bits.  Input sample: x = s / 32768 for int16
 * (exact in fp32), a float32 as it is.  Channel: one index, or -1 = the fp32 mean of all channels (summed in ascending
 * order, one division), taken before filtering.  L == M == 1 (sr = 16000) is a plain convert / select: no table is read.
 * pcm: sample i of channel c is element i * sample_stride + c * channel_stride.  table: device, [L][2K] floats.  The call
 * writes output samples out_lo .. out_lo + n_out - 1 of the track to out[0 .. n_out), fp32 or (out_f32 = 0) fp16 = round to
 * nearest of the fp32 sum; outputs past ceil(n_in L / M) are those of the zero-padded track.  A lane runs the 2K taps of its
 * row in ascending j as one fp32 FMA chain from 0, so every fp32 output is within (2K + 8) * 2^-24 * S * max|x| of the
 * float64 definition, S = max_p sum_j |table[p][j]| (about 2.2), and the bits of output n depend only on n and the input -
 * never on out_lo, n_out or the tile it lands in.  The host picks 16-byte loads for a dense channel (sample_stride = 1)
 * whose 16-byte groups are aligned in every addressed channel, loads of one sample otherwise: same bits.
 * TDC_E_BADARG before any launch: a null pointer; pcm not aligned to its sample, out to its element, table to 8 bytes; fmt
 * outside {0, 1}; n_in < 1; channels outside [1, 65535]; channel < -1 or >= channels; sample_stride < 1; channel_stride < 0;
 * K < 1; L outside [1, 640]; M outside [1, 2^20]; a negative out_lo / n_out, or out_lo + n_out (or n_in) above 2^40; a
 * tile's span (255 M / L + 2K samples, plus the 2K taps at L == 1) beyond 64 KiB of LDS.
 * writes: out[0 .. n_out) and nothing else.  reads: only samples [0, n_in) of the addressed channels (the one, or all for the
 * mean), and L * 2K floats of the table (none at L == M == 1).  never read: the other channels, the padding between the
 * samples of a strided view. */
int tdc_pcm_resample(const void* pcm, int fmt /* 0 s16, 1 f32 */, long long n_in, int channels,
                     long long sample_stride, long long channel_stride /* in elements */,
                     int channel /* >= 0, or -1 = mean */, int L, int M,
                     const float* table /* [L][2K] */, int K,
                     long long out_lo, long long n_out, void* out, int out_f32, void* stream);

/* ---- launch profiler -------------------------------------------------------------------------------------------------
 * Between tdc_profile_start and tdc_profile_stop every tdc_gemm / tdc_attention / tdc_layernorm / tdc_qformer_xattn launch -
 * called directly or from inside a composite (tdc_vit_fwd, tdc_connector_fwd, tdc_qformer_fwd) - is bracketed by two
 * hipEvents on its launch stream and leaves one record.  tdc_profile_stop waits for the recorded events, fills `recs` (at
 * most `cap`) and returns the number of launches seen (negative TDC_E* on error).  tdc_profile_tag sets the tag copied into
 * the records that follow (returns the previous one); tdc_qformer_fwd tags the launches of the cross-attention block
 *  with TDC_PROF_TAG_XATTN_BLOCK by itself.  One profile at a time per process; off by default (one global word
 * is tested per launch).  Measurement infrastructure of bench.py: the profiled step runs the same host path as the timed one. */
#define TDC_PROF_GEMM 1
#define TDC_PROF_ATTN 2
#define TDC_PROF_LN 3
#define TDC_PROF_XATTN 4
#define TDC_PROF_TAG_XATTN_BLOCK 1
typedef struct {
    int kind, tag;
    float ms;                       /* elapsed between the two events */
    int M, N, K, act, res, out_f32; /* GEMM: the launch's shape / epilogue (N, K as passed: padded); ATTN: M = batch * heads,
                                       N = sq, K = sk, act = head_dim; LN: M = rows, N = cols; XATTN: M = F * K rows, N = Nenc,
                                       act = 1 for the output-projection form */
    const void* W;                  /* GEMM: the weight pointer (callers map it to the un-padded dims) */
    double flops;                   /* algorithmic FLOPs of the launch from the dims as passed (GEMM 2 M N K, attention
                                       4 b h sq sk d, XATTN its GEMM + attention products); 0 for LN */
} tdc_prof_rec;
int tdc_profile_start(int max_records);
int tdc_profile_stop(tdc_prof_rec* recs, int cap);
int tdc_profile_tag(int tag);

/* library / device info */
const char* tdc_version(void);
int tdc_device_info(int* cu_count, size_t* hbm_bytes);

#ifdef __cplusplus
}
#endif
#endif
