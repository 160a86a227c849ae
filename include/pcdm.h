/* pcdm.h -- C-ABI of libpcdm.so: the MI355X (gfx950) kernels behind the PCDMs stage-2 denoise loop.
 *
 * The reference (tencent-ailab/PCDMs) has NO native/FFI boundary for this path: its boundary is
 * two Python objects, pipe.unet and pipe.scheduler (stage2_batchtest_inpaint_model.py:125-132),
 * and every device op is an ATen/cuDNN/cuBLAS/xformers call made from inside diffusers 0.24.0.
 * Each entry point below therefore cites the reference / diffusers op it replaces (SURVEY.md §2.1
 * K-numbers); the Python mirror of the reference interface lives in pcdms_amd/ and calls these
 * through ctypes.
 *
 * Conventions: plain pointers to DEVICE memory, sizes as ints, a hipStream_t (passed as void*),
 * every call asynchronous on that stream, no allocation inside, no global state.  Activations
 * are NHWC / token-major bf16 ("u16" storage); statistics, biases and time embeddings fp32.
 * Return 0 on success, a negative code otherwise: -1 bad arguments (incl. a tile configuration that is not valid for the
 * problem), -2 an operand beyond the 2 GiB range of the 32-bit buffer offsets, <= -1000 a HIP launch failure (-1000 - hipError_t).
 */
#ifndef PCDM_H
#define PCDM_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

typedef void* pcdm_stream_t; /* hipStream_t */

#define PCDM_ABI_VERSION 6   /* what pcdm_version() returns for the library this header belongs to */
int pcdm_version(void);
/* 1 only for the test-only CPU lane emulator build (tests/emu); the product .so returns 0. */
int pcdm_is_emulator(void);

/* ---- K4 GroupNorm(+SiLU)  [torch.nn.GroupNorm inside ResnetBlock2D.norm1/2, Transformer2DModel.norm,
 *      conv_norm_out: stage2_inpaint_unet_2d_condition.py:435-441,817-819].
 * x = virtual channel-concat of x1 [B,HW,C1] and x2 [B,HW,C2] (x2 may be NULL, C2 = 0): the up-block
 * skip concat (ref :792-793, K6) is never materialised.  y [B,HW,C1+C2] bf16.
 * ws: fp32 workspace of pcdm_groupnorm_ws_floats(B, C1+C2) floats, ZERO-FILLED once when allocated and written by nothing but
 * pcdm_groupnorm afterwards (its head holds arrival counters that every launch leaves at zero); one workspace may serve calls of
 * any shape with B' <= B on one stream.
 * Shapes whose slab is split over several workgroups that exchange statistics inside the launch (UNet levels 0 / 1) rely on those
 * workgroups being co-resident: the library checks the device (occupancy x CUs, no CU mask) and each workgroup's wait is BOUNDED --
 * if its partners do not arrive (~50 ms: CUs held by another stream / process) it computes the slab's statistics alone: slower, same
 * result up to summation order, never a hang.  pcdm_groupnorm_cluster_timeouts reads how often that happened (synchronous). */
int64_t pcdm_groupnorm_ws_floats(int B, int C);
int pcdm_groupnorm_cluster_timeouts(const float* ws, unsigned* count_out, pcdm_stream_t s);
int pcdm_groupnorm(const void* x1, int C1, const void* x2, int C2, int B, int HW, int groups, float eps,
                   const float* gamma, const float* beta, int fuse_silu, void* y, float* ws, pcdm_stream_t s);

/* GroupNorm whose FIRST source is the not-yet-reduced output of a split-K pcdm_gemm (defer_reduce = 1):
 *   x1[m, n] = bf16( sum_s part[s][m][n] + bias[n] + rowvec[m / HW][n] + residual[m][n] ),  m < M = B * HW, n < N  (= C1)
 * -- the arithmetic (and summation order) of the reduce kernel pcdm_gemm would have launched: results are bit-identical to
 * pcdm_gemm(defer_reduce = 0) + pcdm_groupnorm.  x2 / C2: the second (plain bf16) source of the virtual concat, as pcdm_groupnorm.
 * pre_out [M, N] bf16 must always be provided; it is WRITTEN (the reduced pre-norm tensor, for the residual / skip connections
 * that read it later) iff store_pre != 0 -- except on the two-launch path of very large slabs, which writes it regardless. */
typedef struct pcdm_gn_splitk_src {
    uint32_t struct_size;  /* = sizeof(pcdm_gn_splitk_src) of the header the HOST was compiled against (ABI 6), as pcdm_gemm_params.struct_size: zero-initialise
                              the struct, set this; pcdm_groupnorm_splitk returns -1 for any other size before it reads another field -- a host built against
                              an older header would otherwise hand the kernel a garbage step_error store target */
    const float* part;     /* pcdm_gemm_params.ws of the producing call */
    int32_t split_k, M, N, Npad;
    const float* bias;     /* [Npad] or NULL */
    const float* rowvec;   /* fp32 [B, ldrv] or NULL (rows_per_batch of the producing call must be HW) */
    int64_t ldrv;
    const int32_t* rowvec_step;   /* as pcdm_gemm_params.rowvec_step / rowvec_step_stride */
    int64_t rowvec_step_stride;
    const void* residual;  /* bf16 [M, ldr] or NULL (res_mod = M) */
    int64_t ldr;
    void* pre_out;
    int32_t store_pre;
    int32_t rowvec_step_count;    /* as pcdm_gemm_params.rowvec_step_count / step_error (ABI 6) */
    int32_t* step_error;
} pcdm_gn_splitk_src;
int pcdm_groupnorm_splitk(const pcdm_gn_splitk_src* src, const void* x2, int C2, int B, int HW, int groups, float eps,
                          const float* gamma, const float* beta, int fuse_silu, void* y, float* ws, pcdm_stream_t s);

/* ---- K8 LayerNorm  [BasicTransformerBlock.norm1/2/3, diffusers attention.py]  x,y [rows,C] bf16 */
int pcdm_layernorm(const void* x, void* y, int rows, int C, float eps, const float* gamma, const float* beta,
                   pcdm_stream_t s);

/* ---- K1/K2/K3/K5/K6/K7/K11 GEMM / implicit-GEMM conv3x3 on MFMA with fused epilogues.
 *  out[m, n] = epilogue( sum_k A[m, k] * W[n, k] )
 *  A (bf16), one of
 *    linear : A[m, k] = (k < c1 ? a[m*lda + k] : a2[m*lda2 + k - c1])      (Linear, 1x1 conv, skip concat)
 *    conv3x3: m = (b, oy, ox) over [B, Ho, Wo]; k = (ky*3+kx)*cin + c; pad 1 (or no_pad_lo); stride 1|2;
 *             upsample=1 reads a[b, iy*Hi/Ho, ix*Wi/Wo, c] (nearest interpolation to Ho x Wo folded in -- iy>>1, ix>>1 for the
 *             usual x2: Upsample2D, K5; other sizes: diffusers' upsample_size path for latents not divisible by 8)
 *  W: packed bf16 [Npad, K] (K contiguous; rows >= N zero).  K % 64 == 0, Npad % 64 == 0.
 *  epilogue: + bias[n] + rowvec[m / rows_per_batch, n] + residual[(m % res_mod), n]  then
 *    PCDM_EPI_STORE   : out[m*ldo + n]                                bf16
 *    PCDM_EPI_GEGLU   : W rows interleaved per 64 as [32 h | 32 gate]; out[m*ldo + n/2..] = h*gelu(gate)
 *    PCDM_EPI_SPLIT_VT: n <  vt_col0 -> out[m*ldo + n];  n >= vt_col0 -> out2[b, n - vt_col0, t]
 *                       with m = b*rows_per_batch + t, out2 pitch ldo2 (V^T for pcdm_flash_attn)
 *    PCDM_EPI_NCHW_F32: out as fp32 [B, N, rows_per_batch] (conv_out -> eps in NCHW) */
enum { PCDM_EPI_STORE = 0, PCDM_EPI_GEGLU = 1, PCDM_EPI_SPLIT_VT = 2, PCDM_EPI_NCHW_F32 = 3 };
enum { PCDM_ACT_NONE = 0, PCDM_ACT_SILU = 1, PCDM_ACT_GELU = 2 };
typedef struct pcdm_gemm_params {
    uint32_t struct_size;  /* = sizeof(pcdm_gemm_params) of the header the HOST was compiled against (ABI 4): a struct of another size -- an older or
                              newer header -- is refused with -1 before any field behind it is read */
    const void* a;
    const void* a2;
    int64_t lda, lda2;
    int32_t c1;
    int32_t conv;      /* 0 linear, 1 conv3x3 */
    int32_t B, Hi, Wi, Ho, Wo, stride, upsample, cin;
    const void* w;
    int32_t M, N, K, Npad;
    const float* bias;
    const float* rowvec;   /* fp32 [M / rows_per_batch, ldrv] */
    int64_t ldrv;          /* 0 -> N */
    int32_t rows_per_batch;
    const void* residual;
    int64_t ldr;
    int32_t res_mod;
    int32_t epilogue;
    int32_t vt_col0;
    void* out;
    int64_t ldo;
    void* out2;
    int64_t ldo2;
    int32_t split_k;   /* > 1: split K over split_k workgroups per tile (PCDM_EPI_STORE only); partial sums in ws */
    float* ws;         /* fp32 workspace, >= split_k * M * Npad floats */
    int64_t ws_floats;
    int64_t ldw;       /* row stride of W in elements (0 -> K); lets an activation slice act as the [N,K] operand.  As for a packed W, ALL Npad
                          rows are read (rows >= N only enter output columns that are never stored, so they may hold anything): the slice
                          must have (Npad - 1) * ldw + K readable elements behind w -- a caller whose tensor ends earlier allocates the
                          difference (tests/test_operand_containment.py runs the call at exactly this extent) */
    int32_t no_pad_lo; /* conv: 1 = zero padding at the bottom/right only (taps start AT the output pixel): the VAE
                          encoder's Downsample2D(padding=0) + F.pad(0,1,0,1); 0 = symmetric padding 1 */
    int32_t tile;      /* 0 = heuristic; 1..26 = explicit tile configuration (gemm.hip dispatch_tile; 22 / 23 = the 176-row tiles), 31..36 = the A-in-registers thin-K
                          kernel (rowgemm.hip; K = 320, linear); -1 if invalid for the problem */
    int32_t act;       /* PCDM_ACT_*: out = act(acc + bias + rowvec) + residual.  With PCDM_EPI_GEGLU: gate activation, 0 = GELU(erf) (GEGLU),
                          PCDM_ACT_SILU = SwiGLU (DINOv2 SwiGLUFFN).  SiLU: the convs of
                          ControlNetConditioningEmbedding (stage2_batchtest_inpaint_model.py:101); GELU(erf): ImageProjModel_p (:54-56) */
    int32_t zero_rows; /* linear only: the caller guarantees A rows [0, zero_rows) are all-zero; they are not read and tiles entirely
                          inside them run the epilogue only.  The CFG unconditional half of attn2.to_out: context == 0 => attention
                          output == 0 => out = bias + residual (stage2_inpaint_pipeline.py:457-458) */
    const float* ln_wsum;  /* non-NULL (tiles 31..36: the A-in-registers kernel, K = 320; tiles 2 / 4 / 7 / 8 / 17 / 18 / 23 / 26: the folded instances of the tiled
                              kernel, any K, see ln_row_stats): W and bias carry a FOLDED LayerNorm -- W' = W diag(gamma),
                              bias' = bias + W beta (BasicTransformerBlock.norm1/2/3 in front of to_q|k|v, to_q and the GEGLU projection: K8 fused into
                              K7 / K11) -- and ln_wsum[n] = sum_k W'[n, k] (fp32 [Npad], of the bf16 values).  The kernel takes each A row's mean / rstd
                              (eps ln_eps) and returns rstd (acc - mean ln_wsum[n]) + bias'[n] = LayerNorm(A) W^T + bias.  Other tiles return -1 when set */
    float ln_eps;
    int32_t defer_reduce;  /* split_k > 1 only: leave the split_k fp32 partial slabs in ws ([split_k][M][Npad]) and do NOT launch the reduce
                              kernel: out is not written; bias / rowvec / residual are not applied.  The consumer applies them:
                              pcdm_groupnorm_splitk (the GroupNorm that follows every split-K convolution of the UNet: conv1 -> norm2, conv2 ->
                              the next block's norm) reads the slabs, so the reduce launch, its bf16 write and the norm's read of it disappear.
                              ws must stay untouched until that consumer has run (same stream). */
    const int32_t* rowvec_step;  /* optional DEVICE counter: the row vector block in use is rowvec + (*rowvec_step) * rowvec_step_stride floats -- the
                                    time-embedding projections of EVERY denoise step are computed once per sampling call (they depend on the
                                    timestep table and the class labels only) and a captured step picks its block by the device step index */
    int64_t rowvec_step_stride;
    int32_t dup_rows;      /* conv3x3 + PCDM_EPI_STORE only, > 0: the M rows computed are ALSO written as rows m + dup_rows of out (which then has
                              M + dup_rows rows), with the row-vector row (m + dup_rows) / rows_per_batch and the residual row m + dup_rows of
                              their own: one contraction, two epilogues.  For a batch whose second half has the same conv INPUT as the first
                              but its own time embedding -- the two classifier-free-guidance halves at conv_in and at the first ResnetBlock2D's
                              conv1 (stage2_inpaint_pipeline.py:499-501 doubles the latents; mask, masked latents and pose are shared).  Needs
                              N % 8 == 0, ldo % 8 == 0, rows_per_batch >= 32 and dup_rows % rows_per_batch == 0 with a rowvec; else -1 */
    const float* ln_row_stats;  /* with ln_wsum on a tiled instance (tiles 2 / 4 / 7 / 8 / 17 / 18 / 26; 23 with partials only): [M][K / 32][2] fp32 -- per A row and 32-column run
                                   {sum, sum of squares about the run's own mean}, as left by the launch that produced A with row_stats_out -- the
                                   kernel merges them into the row's LayerNorm statistics (Chan) instead of taking them in its K loop (NULL: in the
                                   loop, every N tile again: pays for N <~ 1280 only).  K % 64 == 0, K <= 1280, 16-byte aligned */
    float* row_stats_out;       /* linear PCDM_EPI_STORE launches on tiles 2 / 4 / 5 / 6 / 7 / 8 / 10 / 18 (else -1): also write those partials of the
                                   rows stored, [M][N / 32][2] fp32, from the bf16-rounded output values (bias / rowvec / residual included).  The
                                   producer of the rows a LayerNorm reads next (Transformer2DModel.proj_in, attn1 / attn2 .to_out + residual).
                                   N % 32 == 0 */
    int32_t rowvec_step_count;  /* > 0 with rowvec_step: the number of blocks behind rowvec.  A counter value outside [0, count) is CLAMPED into the table on
                                   the device (the launch stays inside the caller's memory) and, if step_error is non-NULL, *step_error is set to 1 -- the
                                   host reads it when it next synchronises (pcdm_unet_step_overflow for the UNet context).  0: unchecked (ABI <= 3 behaviour) */
    int32_t* step_error;        /* DEVICE int32, written only on an out-of-range step (never cleared by the library) */
    const void* a3;             /* conv3x3 with EXTRA K (ABI 5): K = 9 cin + cx, cx > 0 -- behind the nine taps the contraction runs on over a 1x1 convolution of
                                   up to two more NHWC bf16 tensors of the OUTPUT geometry: a2 [M, lda2] supplies the first c1 channels, a3 [M, lda3] the
                                   other cx - c1 (NULL when c1 == cx); W rows are [9 cin taps | c1 | cx - c1].  ResnetBlock2D.conv_shortcut over the block's
                                   (concatenated) input composed into conv2 (resnet.py as composed at stage2_inpaint_unet_2d_condition.py:321-344,407-430):
                                   no shortcut launch, no residual round trip.  stride 1, no upsample, Hi == Ho, Wi == Wo, symmetric padding, no dup_rows;
                                   c1, cx multiples of 64; lda2 >= c1, lda3 >= cx - c1, both multiples of 8; else -1 */
    int64_t lda3;
    uint64_t tap_lut;           /* conv3x3 over a SUBSET of the nine taps per output-channel group (ABI 5): with tap_group_n > 0 the K axis holds ntaps = K / cin
                                   (1..4) taps; output channels [g tap_group_n, (g + 1) tap_group_n) (g < 4) use the taps whose ids (ky * 3 + kx, 0..8) are the
                                   nibbles of bits [16 g, 16 g + 4 ntaps) of tap_lut, in K order; W rows are [ntaps taps x cin].  The phase decomposition of
                                   Upsample2D: conv3x3(nearest-upsample x2 (x)) at output pixel (2y + a, 2x + b) is a 2x2 convolution of x with summed taps, i.e.
                                   one 3x3 launch on the LOW-RES input with N = 4 Cout (group = phase 2a + b, taps {3(a+i) + b + j}), 4/9 of the FLOPs, followed by
                                   pcdm_pixel_shuffle2 (diffusers Upsample2D as composed at stage2_inpaint_unet_2d_condition.py:407-430).  stride 1, no upsample,
                                   no extra K (a2 / a3), tap_group_n a multiple of the N tile in use (else -1: pick a tile that divides it).  Only the
                                   4 ntaps low bits of each group's 16 are read (higher bits are ignored); every tap id must be <= 8; a group whose ntaps
                                   taps are all tap 0 is taken for ntaps <= 3 and refused (-1) at ntaps = 4 */
    int32_t tap_group_n;
} pcdm_gemm_params;
/* Since pcdm_version() == 5 the struct above STARTS with struct_size and ends with a3, lda3, tap_lut, tap_group_n (6 left it unchanged; 4: ended with rowvec_step_count, step_error; 3: no struct_size, ended with
 * ln_row_stats, row_stats_out, gn_stats_out, gn_stats_gs -- the last two are gone with the GroupNorm-statistics producer; 2: ended with
 * dup_rows; 1: with ln_eps).  Zero-initialise it (memset), set struct_size = sizeof(pcdm_gemm_params): the library compares it with its own and
 * returns -1 on a mismatch, so a host built against another header fails at its first call instead of having trailing fields misread.
 * (Comparing pcdm_version() with PCDM_ABI_VERSION at start-up remains good practice: the other entry points have no such guard.)
 * bias, rowvec, ldrv and rowvec_step_stride must keep 16-byte alignment (4 floats): the epilogues load them as float4; a violation returns -1.
 * *rowvec_step is device memory the library cannot validate at launch: pass rowvec_step_count to have it bounded on the device. */
int pcdm_gemm(const pcdm_gemm_params* p, pcdm_stream_t s);

/* ---- K9/K10 fused attention (replaces xformers.ops.memory_efficient_attention enabled at
 *      stage2_batchtest_inpaint_model.py:133).  head_dim = 64.  softmax(q k^T * scale) v, fp32 softmax.
 *  q  [B*Lq, ldq]  bf16, head h at columns [64h, 64h+64)
 *  k  [B*Lk, ldk]  bf16, same head layout
 *  vt [B, H*64, ldvt] bf16 = V transposed (key index contiguous), as written by PCDM_EPI_SPLIT_VT
 *  o  [B*Lq, ldo]  bf16, columns [0, H*64) of rows [0, B*Lq) written, nothing else
 *  Any B, H, Lq, Lk >= 1: keys of a partial 64-key tile are masked out of the softmax, tail queries of a partial 128-query block are not
 *  stored.  The scores may lie anywhere in the fp32 range the softmax can represent: a query whose first key tile scores far below
 *  the later ones (or whose scores are all far below zero) is computed like any other.  Reruns are bit-identical.
 *  V^T padding: the columns [Lk, ldvt) of vt that share a 64-key tile with a valid key are READ and multiplied by an exact zero (P of a
 *  masked key), so they may hold any FINITE value -- the result is bit-identical to zero padding -- but must not hold NaN or Inf
 *  (0 * NaN = NaN would reach o).  PCDM_EPI_SPLIT_VT does not write them: its consumers allocate the V^T buffer zeroed.
 *  Returns -1 without launching (o untouched) for: a NULL pointer; B, H, Lq or Lk < 1; ldq, ldk, ldvt or ldo not a multiple of 8
 *  elements; ldvt < Lk; q, k, vt or o not 16-byte aligned (rows are moved in 16-byte pieces); pcdm_flash_attn_thr: thr_log2 outside
 *  [0, 16] or NaN.  Returns -2 without launching when Lk * ldk or 64 * ldvt reaches 2^30 elements (the K / V^T tiles are addressed
 *  with 32-bit byte offsets from the head's first row). */
int pcdm_flash_attn(const void* q, int64_t ldq, const void* k, int64_t ldk, const void* vt, int64_t ldvt,
                    void* o, int64_t ldo, int B, int H, int Lq, int Lk, float scale, pcdm_stream_t s);
/* The same with the lazy-rescale threshold made explicit: the running softmax reference of a query moves only when a key tile's
 * maximum exceeds it by more than thr_log2 (log2 units, 0 <= thr <= 16; P <= 2^thr); 0 = eager online softmax.  pcdm_flash_attn
 * uses PCDM_ATTN_DEFAULT_THR.  Mathematically identical for every thr (P, the row sum and O carry the same reference). */
#define PCDM_ATTN_DEFAULT_THR 8.0f
int pcdm_flash_attn_thr(const void* q, int64_t ldq, const void* k, int64_t ldk, const void* vt, int64_t ldvt,
                        void* o, int64_t ldo, int B, int H, int Lq, int Lk, float scale, float thr_log2, pcdm_stream_t s);

/* ---- N4 (BASELINE.json configs[4]): the same attention with OCP e4m3 operands on the MX-scaled fp8 MFMA (unit block
 *      scales; twice the bf16 matrix rate).  No reference counterpart (attention enters at stage2_batchtest_inpaint_model.py:133).
 * pcdm_quantize_fp8: y[r, c] = e4m3(sat(x[r, c] * scale)) for bf16 x [rows, ldx] -> bytes y [rows, ldy]; columns [cols, cols_pad) are
 *   written as zero (cols_pad % 8 == 0).  Used for K [B*Lk, C] and V^T [B*C, Lk -> padded to a multiple of 16].
 *   sat clamps to +-448 (+-inf included) and keeps NaN: a NaN in x gives an e4m3 NaN byte (0x7f or 0xff), never a finite number.
 *   x needs only its natural 2-byte alignment and any ldx >= cols: rows are read 16 bytes at a time where x is 16-byte aligned and
 *   ldx % 8 == 0, element by element otherwise (the same bytes come out).  y is stored in 8-byte pieces: y 8-byte aligned, ldy % 8 == 0.
 *   Returns -1 without launching (y untouched) for: a NULL pointer; rows or cols < 1; cols_pad < cols or not a multiple of 8; ldy < cols_pad
 *   or not a multiple of 8; ldx < cols; y not 8-byte aligned.
 * pcdm_flash_attn_fp8: q bf16 as in pcdm_flash_attn; k8 [B*Lk, ldk] / vt8 [B, H*64, ldvt] e4m3 bytes (ldk, ldvt multiples of 16,
 *   ldvt >= Lk, padding zero); k_descale / v_descale undo the quantisation scales; thr_log2 <= 8.  fp32 softmax, P rounded to e4m3.
 *   V^T padding: as for pcdm_flash_attn the columns [Lk, ldvt) inside the last key tile are multiplied by an exact zero; pcdm_quantize_fp8
 *   writes them as zero, and any e4m3 byte other than the NaN patterns 0x7f / 0xff gives the same bits.
 *   Returns -1 without launching (o untouched) for: a NULL pointer; B, H, Lq or Lk < 1; ldq not a multiple of 8 elements, ldk or ldvt
 *   not a multiple of 16 bytes, ldo not a multiple of 4 elements (o is stored in 8-byte pieces, so 4 is enough where the bf16 kernel
 *   needs 8); ldvt < Lk; q, k8 or vt8 not 16-byte aligned, o not 8-byte aligned; thr_log2 outside [0, 8] or NaN (P <= 2^thr must stay
 *   below e4m3's 448); k_descale or v_descale not > 0 (NaN included).  Returns -2 without launching when Lk * ldk or 64 * ldvt reaches
 *   2^31 - 1 bytes (32-bit byte offsets). */
int pcdm_quantize_fp8(const void* x, void* y, int64_t rows, int cols, int cols_pad, int64_t ldx, int64_t ldy, float scale, pcdm_stream_t s);
int pcdm_flash_attn_fp8(const void* q, int64_t ldq, const void* k8, int64_t ldk, const void* vt8, int64_t ldvt, void* o, int64_t ldo,
                        int B, int H, int Lq, int Lk, float scale, float k_descale, float v_descale, float thr_log2, pcdm_stream_t s);

/* ---- Single-head attention for wide heads: the VAE mid-block attention (diffusers Attention, one head of width d = C).
 *      o = softmax(q k^T * scale) v, fp32 scores, online fp32 softmax, fp32 accumulation, P and o rounded to bf16.
 *  d  head width: a multiple of 64, 64 <= d <= 512
 *  q  [B*Lq, ldq]  bf16, columns [0, d)  (e.g. a column view of the PCDM_EPI_SPLIT_VT output, row stride 2d)
 *  k  [B*Lk, ldk]  bf16, columns [0, d)
 *  vt [B, d, ldvt] bf16 = V transposed (key index contiguous), as written by PCDM_EPI_SPLIT_VT; columns [Lk, ldvt) are never used
 *  o  [B*Lq, ldo]  bf16, columns [0, d) written, nothing else
 *  Any Lq >= 1, Lk >= 1 (keys of a partial tile are masked out of the softmax), the whole batch in one launch, no workspace;
 *  reruns are bit-identical.  Returns -1 without launching for: a NULL pointer, B, Lq or Lk < 1, d not a multiple of 64 or above 512,
 *  a row stride that is not a multiple of 8 elements or smaller than d, ldvt < Lk, a pointer not 16-byte aligned, a non-finite scale. */
int pcdm_attn_wide(const void* q, int64_t ldq, const void* k, int64_t ldk, const void* vt, int64_t ldvt, void* o, int64_t ldo,
                   int B, int Lq, int Lk, int d, float scale, pcdm_stream_t s);

/* ---- K12 time / class embedding helpers.
 * pcdm_timestep_embedding: diffusers Timesteps(dim, flip_sin_to_cos, shift) (ref :184,677): out fp32 [B,dim];
 *   t read from a DEVICE table of `rows` timesteps: t_dev[row] (int64), broadcast over B.  row = step_dev ? *step_dev : 0, bounded on the
 *   device (ABI 6): a counter outside [0, rows) uses the nearest valid row and sets *step_error (may be NULL) to 1.  Returns -1 without
 *   launching for a NULL t_dev / out, B or dim < 1, an odd dim, rows < 1 or a step_error that is not 4-byte aligned.
 * pcdm_small_linear: y[b,n] = act_out( sum_k act_in(x[b,k]) * W[n,k] + bias[n] ), x,y fp32, W bf16 [N,K],
 *   B <= 32; act_in: 1 = SiLU; act_out: 1 = SiLU before `add`, 2 = SiLU after `add`.  (TimestepEmbedding MLPs ref :191-197,247; every ResnetBlock2D.time_emb_proj) */
int pcdm_timestep_embedding(const int64_t* t_dev, int rows, const int32_t* step_dev, int32_t* step_error, float* out, int B, int dim,
                            int flip_sin_to_cos, float shift, pcdm_stream_t s);
int pcdm_small_linear(const float* x, const void* w, const float* bias, const float* add, float* y, int B, int K,
                      int N, int act_in, int act_out, pcdm_stream_t s);
/* The same embeddings for a whole timestep TABLE (once per sampling call instead of five launches per denoise step):
 * pcdm_timestep_embedding_rows: out[i, :] = Timesteps(t_dev[i]), i < n (fp32 [n, dim]);
 * pcdm_time_class_combine: out[i * B + b, :] = bf16( silu( emb_t[i, :] + (cls ? cls[b, :] : 0) ) ) -- emb = time_embedding(t_i) + class_embedding(b)
 *   as every ResnetBlock2D consumes it (silu(emb)), for all steps and batch entries: the A operand of ONE time_emb_proj GEMM with
 *   M = n * B rows.  Same per-row arithmetic as the per-step launches (bit-identical results). */
int pcdm_timestep_embedding_rows(const int64_t* t_dev, int n, float* out, int dim, int flip_sin_to_cos, float shift, pcdm_stream_t s);
int pcdm_time_class_combine(const float* emb_t, const float* cls, void* out_bf16, int n, int B, int D, pcdm_stream_t s);
/* float32-timestep forms (the fractional timesteps of the sigma-space samplers with timestep_spacing="linspace", e.g. 749.25): the SAME kernels
 * instantiated for a float table; the timestep is used as the fp32 value it is, so an integer-valued float gives the bits of the int64 form.
 * rows / step_dev / step_error of pcdm_timestep_embedding_f32: exactly as pcdm_timestep_embedding (bounded on the device, ABI 6). */
int pcdm_timestep_embedding_f32(const float* t_dev, int rows, const int32_t* step_dev, int32_t* step_error, float* out, int B, int dim,
                                int flip_sin_to_cos, float shift, pcdm_stream_t s);
int pcdm_timestep_embedding_rows_f32(const float* t_dev, int n, float* out, int dim, int flip_sin_to_cos, float shift, pcdm_stream_t s);

/* ---- P-2 input assembly: cat([cat([latents]*2), mask, masked_latents], 1) (stage2_inpaint_pipeline.py:499-501)
 * -> NHWC bf16 [Bout, h, w, cpad] with channels >= 9 zero.  latents fp32 NCHW [N,4,h,w]; Bout = rep*N rows
 * (rep = 2 with CFG); mask fp32 [1|Bout,1,h,w]; masked fp32 [1|Bout,4,h,w] (batch-broadcast when *_b == 1).
 * mask == NULL: the 8-channel stage-3 input cat([latents, gen_t_img_latents], 1) (stage3_refined_pipeline.py:538). */
int pcdm_assemble_input(const float* latents, int N, int rep, const float* mask, int mask_b, const float* masked,
                        int masked_b, void* out, int h, int w, int cpad, pcdm_stream_t s);
/* The same with scheduler.scale_model_input folded in (stage2_inpaint_pipeline.py:500): scale_tab != NULL multiplies the four LATENT channels
 * by the fp32 scalar scale_tab[row * scale_stride + scale_col] of a DEVICE table of scale_rows rows -- one fp32 multiply, then the one rounding
 * to bf16; mask, masked-latent and padding channels are untouched.  row = step_dev ? *step_dev : 0, bounded on the device: a counter outside
 * [0, scale_rows) reads the nearest valid row and sets *step_error (may be NULL) to 1.  scale_tab == NULL: pcdm_assemble_input, bit for bit.
 * For the pcdm_multistep_step table: scale_stride = PCDM_MS_ROW, scale_col = PCDM_MS_IN_SCALE.  Returns -1 without launching for what
 * pcdm_assemble_input refuses, h or w < 1, and with a table: scale_rows < 1, scale_col outside [0, scale_stride), a step_error not 4-byte aligned. */
int pcdm_assemble_input_ex(const float* latents, int N, int rep, const float* mask, int mask_b, const float* masked,
                           int masked_b, void* out, int h, int w, int cpad, const float* scale_tab, int scale_stride, int scale_col,
                           int scale_rows, const int32_t* step_dev, int32_t* step_error, pcdm_stream_t s);
/* NCHW fp32 -> NHWC bf16 (pose feature st_pose_f, ref :430-431) and back.  y 16-byte aligned for the first (8-channel stores).  Both return -1
 * without launching for a NULL pointer or B, C or HW < 1; the first also for Cpad < C or Cpad % 8 != 0. */
int pcdm_nchw_f32_to_nhwc_bf16(const float* x, void* y, int B, int C, int Cpad, int HW, pcdm_stream_t s); /* y [B,HW,Cpad], c >= C zero */
int pcdm_nhwc_bf16_to_nchw_f32(const void* x, float* y, int B, int C, int HW, pcdm_stream_t s);
int pcdm_f32_to_bf16(const float* x, void* y, int64_t n, pcdm_stream_t s);

/* ---- K13 CFG combine + scheduler step (stage2_inpaint_pipeline.py:510-519).
 * eps [2N or N, C*HW] fp32 (uncond rows first).  g = guidance scale (cfg=0: eps used as is).
 * x_prev = cx*x + ce*eps_guided (+ cn*noise); coefficients read from row `row` of the DEVICE table coef[rows][4] =
 * {cx, ce, cn, unused} so that one captured hipGraph serves every step.  row = step_dev ? *step_dev : 0, bounded on the device (ABI 6): a
 * counter outside [0, rows) uses the nearest valid row and sets *step_error (may be NULL) to 1.
 * Optionally writes the guided eps (eps_out) and x0 = c0x*x + c0e*eps is left to the host scheduler.
 * coef == NULL (with x_prev == NULL: the CFG combine alone) reads no table: rows and step_error are then ignored and not checked.
 * Returns -1 without launching for a NULL eps, n < 1, x_prev without x or coef, and with a table: rows < 1 or a step_error that is not
 * 4-byte aligned. */
int pcdm_cfg_step(const float* eps, int cfg, float g, const float* x, const float* noise, float* x_prev,
                  float* eps_out, const float* coef, int rows, const int32_t* step_dev, int32_t* step_error, int64_t n, pcdm_stream_t s);
/* CFG combine + diffusers UniPCMultistepScheduler.step (the shipped driver's scheduler: stage2_batchtest_inpaint_model.py:132;
 * SURVEY.md Appendix A-10; solver order <= 2) as one kernel on static state, replayable from a hipGraph.  Row `row` of the DEVICE
 * table coef[rows][12] = {a_x, a_e, use_corrector, c_last, c_m1, c_m2, c_mt, p_x, p_mt, p_m1, 0, 0}:
 *   m_t = a_x x + a_e eps_guided;  x_c = use_corrector ? c_last last + c_m1 m1 + c_m2 m2 + c_mt m_t : x;  x' = p_x x_c + p_mt m_t + p_m1 m1
 * then, in place: x <- x', m2 <- m1, m1 <- m_t, last <- x_c (all fp32 [n]; zero m1 / m2 / last before step 0).
 * row = step_dev ? *step_dev : 0, bounded on the device (ABI 6): a counter outside [0, rows) uses the nearest valid row and sets *step_error
 * (may be NULL) to 1.  Returns -1 without launching for a NULL eps / state / coef pointer, n < 1, rows < 1 or a step_error that is not
 * 4-byte aligned. */
int pcdm_unipc_step(const float* eps, int cfg, float g, float* x, float* m1, float* m2, float* last, const float* coef,
                    int rows, const int32_t* step_dev, int32_t* step_error, int64_t n, pcdm_stream_t s);
/* CFG combine + DPMSolverMultistepScheduler.step ("DPM++ 2M" and its SDE form; dpmsolver++ / sde-dpmsolver++, solver order <= 2,
 * midpoint / heun) as one kernel on static state, replayable from a hipGraph.  Row `row` of the DEVICE table
 * coef[rows][8] = {a_x, a_e, p_x, p_m0, p_m1, p_z, 0, 0}:
 *   m0 = a_x x + a_e eps_guided;  x' = p_x x + p_m0 m0 + p_m1 m1 + p_z noise_all[row][i]
 * then, in place: x <- x', m1 <- m0 (all fp32 [n]; zero m1 before step 0).  noise_all [rows, n] (as many rows as coef) may be NULL when
 * no row has p_z != 0 (the term is then skipped).  row = step_dev ? *step_dev : 0, bounded on the device (ABI 6) before either table is
 * addressed: a counter outside [0, rows) uses the nearest valid row and sets *step_error (may be NULL) to 1.  Returns -1 without launching
 * for a NULL eps / state / coef pointer, n < 1, rows < 1 or a step_error that is not 4-byte aligned. */
int pcdm_dpmpp_step(const float* eps, int cfg, float g, float* x, float* m1, const float* noise_all, const float* coef,
                    int rows, const int32_t* step_dev, int32_t* step_error, int64_t n, pcdm_stream_t s);
/* CFG combine + one step of EulerDiscreteScheduler / EulerAncestralDiscreteScheduler / LMSDiscreteScheduler / PNDMScheduler (PLMS) as one
 * kernel on static state, replayable from a hipGraph: the four are linear maps on (x, a saved sample, eps and up to three older eps, noise)
 * with host-known scalars.  State, all fp32 [n], distinct buffers, zeroed before step 0: x, xs (saved sample), h1 / h2 / h3 (eps history,
 * h1 newest).  Row `row` of the DEVICE table coef[rows][PCDM_MS_ROW]:
 *   {c_x, c_s, c_0, c_1, c_2, c_3, c_z, in_scale, save, push, 0, 0}
 *   e  = eps_guided (cfg: fma(g, eps_cond - eps_uncond, eps_uncond))
 *   x' = c_x x + c_s xs + c_0 e + c_1 h1 + c_2 h2 + c_3 h3 + c_z noise_all[row][i]
 *   save != 0: xs <- x (the OLD x);  push != 0: h3 <- h2, h2 <- h1, h1 <- e;  x <- x'
 * Arithmetic: the product c_x x, then FUSED multiply-adds (one rounding each) in exactly the order written, on the GPU and in the lane emulator
 * alike.  The noise term is skipped when noise_all (fp32 [rows, n]) is NULL or the row's c_z is 0.  in_scale is not read here: it is the
 * per-step input scale of pcdm_assemble_input_ex, kept in the same row.  row = step_dev ? *step_dev : 0, bounded on the device: a counter
 * outside [0, rows) uses the nearest valid row and sets *step_error (may be NULL) to 1.  One element per lane, no atomics; 16-byte accesses
 * where the addresses allow plus a scalar tail.  Returns -1 without launching for a NULL eps / state / coef pointer, rows < 1, n < 1 or a
 * step_error that is not 4-byte aligned. */
#define PCDM_MS_ROW 12
#define PCDM_MS_CX 0
#define PCDM_MS_CS 1
#define PCDM_MS_C0 2
#define PCDM_MS_C1 3
#define PCDM_MS_C2 4
#define PCDM_MS_C3 5
#define PCDM_MS_CZ 6
#define PCDM_MS_IN_SCALE 7
#define PCDM_MS_SAVE 8
#define PCDM_MS_PUSH 9
int pcdm_multistep_step(const float* eps, int cfg, float g, float* x, float* xs, float* h1, float* h2, float* h3, const float* noise_all,
                        const float* coef, int rows, const int32_t* step_dev, int32_t* step_error, int64_t n, pcdm_stream_t s);
/* Stage-1 prior: CFG combine (src/pipelines/stage1_prior_pipeline.py:467-471) + diffusers
 * UnCLIPScheduler.step (:478-483) + optional affine read-out (post_process_latents, stage1_prior_transformer.py:299-301).
 * pred [2N or N, n/N] fp32 (uncond rows first); HOST coefficients c8 = {p_x, p_e, clip, c_x0, c_x, c_noise, out_scale,
 * out_shift}:  x0 = clamp(p_x*x + p_e*pred_guided, +-clip) (clip <= 0: none);
 * x_prev = (c_x0*x0 + c_x*x + c_noise*noise) * out_scale + out_shift.  x_prev may alias x. */
int pcdm_unclip_step(const float* pred, int cfg, float g, const float* x, const float* noise, float* x_prev,
                     const float* c8, int64_t n, pcdm_stream_t s);
/* The same step with its eight coefficients read from row `row` of a DEVICE table coef[rows][8] and its noise from slab `row`
 * of noise_all [rows, n] (NULL: none), updating x in place: one captured hipGraph serves every step of the stage-1 loop.
 * row = step_dev ? *step_dev : 0, bounded on the device (ABI 6) before either table is addressed: a counter outside [0, rows) uses the
 * nearest valid row and sets *step_error (may be NULL) to 1.  Returns -1 without launching for a NULL pred / x / coef, n < 1, rows < 1 or a
 * step_error that is not 4-byte aligned. */
int pcdm_unclip_step_dev(const float* pred, int cfg, float g, float* x, const float* noise_all, const float* coef,
                         int rows, const int32_t* step_dev, int32_t* step_error, int64_t n, pcdm_stream_t s);
/* rescale_noise_cfg (stage2_inpaint_pipeline.py:52-63): out = gr * cfg * std(text)/std(cfg) + (1-gr) * cfg, per sample
 * over n = C*H*W elements (unbiased std); cfg_eps / text_eps / out fp32 [N, n]; out may alias cfg_eps. */
int pcdm_rescale_noise_cfg(const float* cfg_eps, const float* text_eps, float* out, int N, int64_t n,
                           float guidance_rescale, pcdm_stream_t s);
/* p[r, c] = softmax_c(scale * s[r, c]) : fp32 [rows, ld_s] -> bf16 [rows, ld_p], cols <= 8192.  The VAE's single-head
 * d = 512 attention (AutoencoderKL mid block) = pcdm_gemm (K Q^T, fp32) + this + pcdm_gemm (P V).
 * Columns [cols, ld_p) of p are not written.  Domain: every score finite or -inf (which gives exactly 0), |scale * s * log2(e)| < 1e30
 * for the finite ones, and at least one finite score per row; a row of only -inf gives NaN, as torch.softmax does.  Outside that
 * domain (a row below -1e30 throughout, a product that overflows fp32) the row may come out NaN where the exact softmax exists.
 * Returns -1 without launching (p untouched) for: a NULL pointer; rows or cols < 1; cols > 8192; ld_s < cols; ld_p < cols. */
int pcdm_softmax_rows(const float* s_in, void* p_out, int rows, int cols, int64_t ld_s, int64_t ld_p, float scale,
                      pcdm_stream_t s);
/* AutoencoderKL helpers (stage2_inpaint_pipeline.py:443-444, :528-532):
 * gaussian_sample: out[B,zc,HW] = (mean + exp(0.5*clamp(logvar,-30,20)) * noise) * scale from moments fp32 [B,2*zc,HW];
 * image_to_uint8: VaeImageProcessor.postprocess -- x fp32 [B,cstride,HW] (first 3 channels) -> uint8 [B,HW,3]. */
int pcdm_gaussian_sample(const float* moments, const float* noise, float* out, int B, int zc, int HW, float scale,
                         pcdm_stream_t s);
int pcdm_image_to_uint8(const float* x, void* out, int B, int cstride, int HW, pcdm_stream_t s);
/* y = sum_i c[i] * x_i  (i < nin <= 6), fp32; UniPC predictor/corrector linear combinations. */
int pcdm_lincomb(float* y, int nin, const float* const* xs, const float* c, int64_t n, pcdm_stream_t s);
/* *step_dev += 1.  Reads no table: every reader of a table bounds the counter itself (ABI 6). */
int pcdm_advance_step(int32_t* step_dev, pcdm_stream_t s);
/* out NHWC bf16 [B, 2H, 2W, C] <- in [B * H * W, 4 * C] bf16 (columns = phase 2a + b major, then channel): out[b, 2y + a, 2x + bb, c] =
 * in[(b, y, x), (2a + bb) C + c].  The second half of the phase-decomposed Upsample2D convolution (pcdm_gemm_params.tap_lut).  C % 8 == 0. */
int pcdm_pixel_shuffle2(const void* in, void* out, int B, int H, int W, int C, pcdm_stream_t s);
/* FreeU (arXiv 2309.11497; diffusers 0.24.0 apply_freeu / fourier_filter, threshold 1) in front of one decoder resnet's [hidden | skip] concat.
 * hidden bf16 [B * H * W, C1], skip bf16 [B * H * W, C2] (NHWC rows):
 *   hidden_out[:, c] = bf16(float(hidden[:, c]) * b) for c < C1 / 2, = hidden[:, c] above (hidden_out == hidden: in place, the upper half is not touched);
 *   skip_out = ifftn(ifftshift(fftshift(fftn(skip)) * mask)).real over (H, W) with mask = 1 except s on [H/2 - 1 : H/2 + 1, W/2 - 1 : W/2 + 1],
 *   evaluated as skip + (s - 1) * (the projection onto the frequencies ky in {0, -1}, kx in {0, -1}, one frequency along an axis of length 1):
 *   plane sums (fixed order) and correction in fp64 -- fp32 sums miss one ulp where the correction cancels an element --, rounded to bf16 once:
 *   every element within one bf16 ulp of the fp64 FFT form; s = 1 returns skip bit for bit.  skip is not written (skip_out == skip is
 *   refused).  Reruns are bit-identical, a plane's result does not depend on B, nothing is allocated: graph-capturable.
 * One launch while H * W <= 355 (the (image, 64-channel) slab stays in LDS); larger planes take two launches through `workspace`
 * (pcdm_freeu_ws_bytes bytes, 16-byte aligned, no initialisation; 0 bytes -- workspace may be NULL -- for the one-launch sizes).
 * Any H, W >= 1.  C1 and C2 must be multiples of 8: anything else, a NULL or not 16-byte aligned tensor, B, H or W < 1, B > 65535 or
 * H * W > 2^24 returns -1 without launching (pcdm_freeu_ws_bytes: -1). */
int64_t pcdm_freeu_ws_bytes(int B, int H, int W, int C1, int C2);
int pcdm_freeu(const void* hidden, void* hidden_out, const void* skip, void* skip_out, int B, int H, int W, int C1, int C2, float b, float s,
               void* workspace, pcdm_stream_t st);

/* ---- Image metrics of the evaluation drivers (stage2_batchtest_inpaint_model.py:203-219, stage3_batchtest_refined_model.py): score the N decoded
 * samples of a pair against the target on the device and keep the best one, without a host round trip.
 * Images are NHWC with 3 channels, uint8 (is_f32 = 0) or fp32 (is_f32 = 1; both tensors the same type): cand [N, Hc, Wc, 3], ref [ref_n, Hr, Wr, 3] with
 * ref_n = 1 (one target for every candidate) or N.  Each comes with a window {x0, y0, W, H} (int32[4], HOST memory) into its own image -- the right
 * half of a [source | target] canvas is scored against a stand-alone target with no crop copy; the two windows have the same W, H.
 * Every call returns -1 and writes nothing for: channels != 3, ref_n not 1 or N, a window that leaves its image or differs in size from the other,
 * N > 65535, a workspace smaller than pcdm_metrics_ws_bytes or not 8-byte aligned, and (pcdm_ssim) sigma whose radius r = int(3.5 sigma + 0.5) is 0 or
 * above 8, or W < 2r + 1 or H < 2r + 1.
 * pcdm_metrics_ws_bytes: size of the caller-provided workspace for pcdm_ssim at this sigma (and for pcdm_psnr; sigma <= 0: for pcdm_psnr alone).  The
 *   workspace holds per-workgroup partial sums only, needs no initialisation, and is added up in a fixed order: reruns are bit-identical.
 * pcdm_ssim: scores[n] (fp32, device) = skimage.metrics.structural_similarity(ref, cand[n], gaussian_weights=True, sigma=sigma,
 *   use_sample_covariance=False, channel_axis=2, data_range=R) with R = data_range, or, for data_range < 0, max - min of the candidate's window over
 *   all channels: separable Gaussian of radius r, weights exp(-(i / sigma)^2 / 2) normalised to 1, five filtered moments per channel, population
 *   covariances, the map averaged over the interior [r, H - r) x [r, W - r) and the channels (no tap of an averaged pixel leaves the window, so
 *   pixels outside it never enter).  fp64 accumulation on values centred per image: |score - fp64 skimage| <= 1e-5, and a constant candidate against
 *   a constant reference (R = 0) is NaN for any constant.  argmax (int32, device; may be NULL) = np.argmax(scores): the first maximum, a NaN ranks
 *   as the maximum.  Three launches (min / max, tiles, final sum), no host synchronisation.
 * pcdm_psnr: mse[n] = mean squared difference over the windows (uint8: integer accumulation, exact), psnr[n] = 10 log10(data_range^2 / mse[n]), +inf for
 *   identical windows; data_range > 0 (255 for uint8 images); either output may be NULL.
 * pcdm_select_image: out <- the window of cand_u8[*index_dev] (the index read on the device, clamped into [0, N)): normalized = 0: uint8 [H, W, 3];
 *   normalized = 1: fp32 NCHW [1, 3, H, W] = (x / 255 - 0.5) / 0.5 in fp32 -- transforms.ToTensor() + Normalize([0.5], [0.5]), bit for bit. */
int64_t pcdm_metrics_ws_bytes(int N, int ref_n, int W, int H, float sigma);
int pcdm_ssim(const void* cand, int N, int Hc, int Wc, const int32_t* cand_win, const void* ref, int ref_n, int Hr, int Wr, const int32_t* ref_win,
              int channels, int is_f32, float sigma, float data_range, float* scores, int32_t* argmax, void* ws, int64_t ws_bytes, pcdm_stream_t s);
int pcdm_psnr(const void* cand, int N, int Hc, int Wc, const int32_t* cand_win, const void* ref, int ref_n, int Hr, int Wr, const int32_t* ref_win,
              int channels, int is_f32, float data_range, float* mse, float* psnr, void* ws, int64_t ws_bytes, pcdm_stream_t s);
int pcdm_select_image(const void* cand_u8, int N, int Hc, int Wc, const int32_t* win, int channels, const int32_t* index_dev, void* out, int normalized,
                      pcdm_stream_t s);

/* ---- LPIPS v0.1, net = 'alex', eval mode (the second per-pair metric of the paper's protocol; the reference's metrics.py calls the lpips package)
 * on the device in exact fp32: every convolution is an implicit GEMM on the fp32-input MFMA (v_mfma_f32_16x16x4_f32: a k-ordered fmaf chain per
 * output, no bf16 operand anywhere), activations NHWC fp32.  The network is restated from its published definition: scaling layer
 * (x - shift) / scale with shift = (-.030, -.088, -.188), scale = (.458, .448, .450); AlexNet features conv1 3->64 11x11 s4 p2, MaxPool 3x3 s2, conv2
 * 64->192 5x5 p2, MaxPool 3x3 s2, conv3 192->384, conv4 384->256, conv5 256->256 (3x3 p1), each with bias + ReLU; per ReLU output l:
 * n = f / (sqrt(sum_c f^2) + 1e-10), d_l = mean_{h,w} sum_c lin_l[c] (n0 - n1)^2; result sum_l d_l.
 * pcdm_pack_lpips_conv: HOST loops, fp32 [Cout, Cin, kh, kw] -> fp32 [Kpad / 4][Npad][4] with k = (ky kw + kx) Cp + c, Cp = Cin rounded up to 4
 *   (conv1: 3 -> 4), Kpad = kh kw Cp rounded up to 16, Npad = Cout rounded up to 16, zeros elsewhere; bias -> fp32 [Npad].  Returns Npad (< 0: bad
 *   arguments); *K_out = Kpad, *cin_out = Cp; output pointers may be NULL to query sizes.  Upload both.
 * pcdm_conv2d_f32: out NHWC fp32 [B, Ho, Wo, Cout] = conv(x NHWC fp32 [B, Hi, Wi, Cin], w) + bias, ReLU when relu != 0; Ho = (Hi + 2 pad - kh) / stride
 *   + 1.  Cin is the PADDED channel count (% 4 == 0), w_packed / bias as pcdm_pack_lpips_conv left them; any kernel size, stride and padding;
 *   taps outside the image contribute zeros.  Per output the products are accumulated in one fixed k order: reruns are bit-identical and a row's
 *   result does not depend on where in the batch it lies.  x and w_packed 16-byte aligned.
 * pcdm_maxpool3s2_f32: MaxPool2d(3, stride 2) without padding (floor) on NHWC fp32, C % 4 == 0, Hi, Wi >= 3.
 * pcdm_lpips: out[n] (fp32 [N], device) = LPIPS of image n of img0 against image n (ref_n = N) or image 0 (ref_n = 1) of img1; layers (may be
 *   NULL): fp32 [5, N], the five d_l, whose fp32 sum in tap order is out[n]; argmin (int32, device, may be NULL) = np.argmin(out): the first
 *   minimum, a NaN ranks as the minimum -- feed it to pcdm_select_image for the best-LPIPS candidate.
 *   is_f32 = 0: images uint8 NHWC [n, Hi, Wi, 3], x = p / 255; is_f32 = 1: fp32 NCHW [n, 3, Hi, Wi].  normalize != 0: x <- 2 x - 1 (inputs in
 *   [0, 1]); normalize = 0 feeds x as it is -- on uint8 that is what the reference's LPIPS.calculate_from_disk computes (metrics.py:484-498 hands
 *   [0, 1] images to a network that expects [-1, 1]; kept, not corrected).  Windows {x0, y0, W, H} (HOST memory) as for pcdm_ssim; W, H >= 31
 *   (below that the second pool has no window), (N + ref_n) W H < 2^28.  Both images of every pair run as ONE batch of N + ref_n.
 *   ws: pcdm_lpips_ws_bytes(N, ref_n, H, W) bytes, 16-byte aligned, no initialisation: the activations and 5 N 32 fp64 partial sums.  No atomics,
 *   no allocation, no host synchronisation; 14 launches on s.  Returns -1 and writes nothing for any argument outside the above. */
typedef struct pcdm_lpips_weights {
    const float* conv_w[5];   /* device, pcdm_pack_lpips_conv layout */
    const float* conv_b[5];   /* device, fp32 [Npad] */
    const float* lin[5];      /* device, fp32 [64 | 192 | 384 | 256 | 256] */
} pcdm_lpips_weights;
int pcdm_pack_lpips_conv(const float* w, const float* bias, int Cout, int Cin, int kh, int kw, float* out_w, float* out_bias, int* K_out, int* cin_out);
int pcdm_conv2d_f32(const float* x, int B, int Hi, int Wi, int Cin, const float* w_packed, const float* bias, int Cout, int kh, int kw, int stride, int pad,
                    int relu, float* out, pcdm_stream_t s);
int pcdm_maxpool3s2_f32(const float* x, int B, int Hi, int Wi, int C, float* out, pcdm_stream_t s);
int64_t pcdm_lpips_ws_bytes(int N, int ref_n, int H, int W);
int pcdm_lpips(const void* img0, int N, int H0, int W0, const int32_t* win0, const void* img1, int ref_n, int H1, int W1, const int32_t* win1, int is_f32,
               int normalize, const pcdm_lpips_weights* wts, float* out, float* layers, int32_t* argmin, void* ws, int64_t ws_bytes, pcdm_stream_t s);

/* ---- FID (the third metric of the paper's protocol; the reference's metrics.py:23-257 and inception.py) on the device: torchvision's InceptionV3
 * trunk in exact fp32 on the same fp32-input MFMA convolution as LPIPS, fp64 statistics, mean and covariance.  The Frechet distance itself is host
 * fp64 (pcdms_amd/metrics.py: frechet_distance).  Restated from the published definition; torchvision is not a dependency.
 * pcdm_conv2d_f32_ex: pcdm_conv2d_f32 with a padding per axis (Ho = (Hi + 2 pad_h - kh) / stride + 1, Wo likewise with pad_w: the 1 x 7 / 7 x 1 /
 *   1 x 3 / 3 x 1 kernels) and an output slice: out is an NHWC tensor with out_pitch channels per pixel and the Cout results of a pixel go to its
 *   channels [out_offset, out_offset + Cout); no other byte of out is written, so the branches of an Inception block write the concatenated tensor
 *   directly.  0 <= out_offset <= out_pitch - Cout, B Ho Wo out_pitch < 2^31.  Same packed weights (pcdm_pack_lpips_conv), same k order: with pad_h
 *   = pad_w, out_pitch = Cout, out_offset = 0 the result equals pcdm_conv2d_f32's bit for bit.
 * pcdm_maxpool3s2_f32_ex: pcdm_maxpool3s2_f32 into the channels [out_offset, out_offset + C) of an out_pitch-channel tensor (both % 4 == 0).
 * pcdm_avgpool3_f32: F.avg_pool2d(x, 3, 1, 1) (count_include_pad) on NHWC fp32, C % 4 == 0: the nine taps added in (dy, dx) order in fp32, zeros
 *   outside the image, the sum divided by 9.
 * pcdm_global_avgpool_f32: out[b, c] (fp32 [B, C]) = mean over the P pixels of NHWC fp32 [B, P, C]: pixel order, fp64 sum, rounded once.
 * pcdm_inception_input: out fp32 NHWC [N, Ho, Wo, 4] (channel 3 = 0) <- the window {x0, y0, W, H} (HOST memory) of uint8 NHWC [N, Hi, Wi, 3]
 *   (is_f32 = 0, x = p / 255) or fp32 NCHW [N, 3, Hi, Wi] (is_f32 = 1).  resize != 0: Ho = Wo = 299, F.upsample(x, (299, 299), mode='bilinear') =
 *   align_corners False, no antialias, for enlarging and reducing alike; resize = 0: Ho = H, Wo = W.  normalize != 0: x[c] s_c / 0.5 + (m_c - 0.5) /
 *   0.5 with s = (0.229, 0.224, 0.225), m = (0.485, 0.456, 0.406) -- the reference applies this remap, which torchvision means for [-1, 1] inputs, to
 *   [0, 1] images; kept, not corrected.  Coordinates are exact rationals and the arithmetic is fp64, rounded to fp32 once.
 * pcdm_inception_features: out (fp32 [N, dims], device) = the global spatial mean of the block output with dims channels, dims in {64, 192, 768,
 *   2048} = the reference's BLOCK_INDEX_BY_DIM (64: first max-pool, 192: second max-pool, 768: Mixed_6e, 2048: Mixed_7c = pool3).  Image arguments
 *   as pcdm_inception_input.  Every convolution is Conv2d(bias = False) + BatchNorm2d(eps = 1e-3, running statistics) + ReLU; the caller folds the
 *   BatchNorm into weight and bias (fp64, rounded to fp32 once) and packs with pcdm_pack_lpips_conv.  The 94 convolutions, in the order of
 *   pcdm_inception_weights (= torchvision's module order):
 *     0-4   Conv2d_1a_3x3, Conv2d_2a_3x3, Conv2d_2b_3x3, Conv2d_3b_1x1, Conv2d_4a_3x3 (a 3 x 3 / stride-2 max-pool after 2b and after 4a)
 *     5-25  Mixed_5b, Mixed_5c, Mixed_5d (InceptionA), 7 each: branch1x1, branch5x5_1, branch5x5_2, branch3x3dbl_1, _2, _3, branch_pool
 *     26-29 Mixed_6a (InceptionB): branch3x3, branch3x3dbl_1, _2, _3
 *     30-69 Mixed_6b .. Mixed_6e (InceptionC), 10 each: branch1x1, branch7x7_1, _2, _3, branch7x7dbl_1, _2, _3, _4, _5, branch_pool
 *     70-75 Mixed_7a (InceptionD): branch3x3_1, _2, branch7x7x3_1, _2, _3, _4
 *     76-93 Mixed_7b, Mixed_7c (InceptionE), 9 each: branch1x1, branch3x3_1, _2a, _2b, branch3x3dbl_1, _2, _3a, _3b, branch_pool
 *   dims = 64 / 192 / 768 / 2048 uses the first 3 / 5 / 70 / 94 of them; the others may be NULL.  The network input (299 x 299, or the window when
 *   resize = 0) must leave every layer at least one output: 75 x 75 is the smallest for dims = 2048.  N <= 65535, N H W < 2^27.
 *   ws: pcdm_inception_ws_bytes(N, H, W, dims) bytes for an H x W NETWORK input (299, 299 when resizing), 16-byte aligned, no initialisation.
 *   No atomics, no allocation, no host synchronisation; reruns are bit-identical and a row's features do not depend on its place in the batch.
 *   Returns -1 and writes nothing for any argument outside the above.
 * pcdm_fid_accumulate: sum[j] += sum_b feat[b, j], gram[i, j] += sum_b feat[b, i] feat[b, j] for feat fp32 [B, D], sum fp64 [D], gram fp64 [D, D]
 *   (zeroed by the caller before the first batch): one thread per output, the samples in order, products and sums in fp64 -- the state after n
 *   samples is bit-identical however they were split into batches.  D <= 8192.
 * pcdm_fid_finalize: mu = sum / n, sigma[i, j] = (gram[i, j] - sum[i] sum[j] / n) / (n - 1) = np.cov(rowvar = False), symmetric bit for bit; n >= 2. */
typedef struct pcdm_inception_weights {
    const float* w[94];      /* device, pcdm_pack_lpips_conv layout, BatchNorm folded in */
    const float* bias[94];   /* device, fp32 [Npad] */
} pcdm_inception_weights;
int pcdm_conv2d_f32_ex(const float* x, int B, int Hi, int Wi, int Cin, const float* w_packed, const float* bias, int Cout, int kh, int kw, int stride,
                       int pad_h, int pad_w, int relu, float* out, int out_pitch, int out_offset, pcdm_stream_t s);
int pcdm_maxpool3s2_f32_ex(const float* x, int B, int Hi, int Wi, int C, float* out, int out_pitch, int out_offset, pcdm_stream_t s);
int pcdm_avgpool3_f32(const float* x, int B, int H, int W, int C, float* out, pcdm_stream_t s);
int pcdm_global_avgpool_f32(const float* x, int B, int P, int C, float* out, pcdm_stream_t s);
int pcdm_inception_input(const void* img, int N, int Hi, int Wi, const int32_t* win, int is_f32, int resize, int normalize, float* out, pcdm_stream_t s);
int64_t pcdm_inception_ws_bytes(int B, int H, int W, int dims);
int pcdm_inception_features(const void* img, int N, int Hi, int Wi, const int32_t* win, int is_f32, int resize, int normalize, int dims,
                            const pcdm_inception_weights* wts, float* out, void* ws, int64_t ws_bytes, pcdm_stream_t s);
int pcdm_fid_accumulate(const float* feat, int B, int D, double* sum, double* gram, pcdm_stream_t s);
int pcdm_fid_finalize(const double* sum, const double* gram, int64_t n, int D, double* mu, double* sigma, pcdm_stream_t s);

/* ---- Input preparation of the evaluation drivers (stage2_batchtest_inpaint_model.py:135-149: Image.resize((W, H), Image.BICUBIC), the
 * [source | black] and [source pose | target pose] canvases, ToTensor + Normalize, CLIPImageProcessor) on the device, from the decoded uint8 pixels.
 * pcdm_resample_u8: Pillow's 8-bit separable resampler.  src uint8 HWC [Hs, Ws, channels] (channels 3 or 1, contiguous) -> the Hd x Wd window at
 *   pixel (x0, y0) of a uint8 HWC canvas dst with dst_pitch BYTES between rows (dst_pitch >= (x0 + Wd) channels; the caller guarantees that
 *   y0 + Hd rows exist); bytes outside the window are not touched, so pasting needs no extra launch.  The filter lives in the tables, one per
 *   axis, int32 in DEVICE memory: xtab = [lo (Wd) | count (Wd) | coeff (Wd * kx)], ytab likewise with Hd, ky.  Output o of an axis is
 *   clip8((2^21 + sum_{j < count[o]} coeff[o * k + j] * in[lo[o] + j]) >> 22) in 32-bit integers (weights of about 2^22 in sum, pixels <= 255: no
 *   overflow), the horizontal pass first and rounded to uint8, then the vertical pass over those bytes.  For Pillow's result build a table as
 *   ImagingResample does: scale = in / out, filterscale = max(scale, 1), support = filter_support * filterscale, center = (o + 0.5) scale,
 *   lo = max(int(center - support + 0.5), 0), hi = min(int(center + support + 0.5), in), count = hi - lo, w_j = filter((j + lo - center + 0.5) /
 *   filterscale) normalised to sum 1 in fp64, coeff = int(w 2^22 + 0.5) (w < 0: int(w 2^22 - 0.5)), k = 2 int(ceil(support)) + 1
 *   (pcdms_amd/preprocess.py).  An axis whose size does not change takes a NULL table and is copied, as Pillow skips it; a NULL table with
 *   different sizes, or a table with equal sizes, returns -1.  Table entries are clamped into the image on the device, so a wrong table cannot
 *   cause an access outside src, dst's window or the workspace.
 *   One launch: a workgroup owns a 32 x 16 output tile, resamples the input rows it needs horizontally into LDS (rows * 32 * channels bytes) and
 *   runs the vertical pass out of LDS.  When the rows of a tile exceed 24 KiB of LDS (vertical downscales beyond about 15 : 1) the call takes two
 *   launches through ws (uint8, pcdm_resample_ws_bytes; 0 and NULL otherwise): same bytes.  No atomics, no host synchronisation.
 * pcdm_u8_to_nchw: out fp32 NCHW [1, channels, H, W] <- (x - mean[c]) / std[c] over the window win = {x0, y0, W, H} (HOST memory) of src,
 *   mean / std HOST float[channels], every operation in fp32 in this order.  mode 0: x = float(p) / float(scale) -- scale 255, mean = std = 0.5 is
 *   transforms.ToTensor() + Normalize([0.5], [0.5]) bit for bit; mode 1: x = float(double(p) * scale) -- scale 1 / 255 with the OpenAI mean / std is
 *   rescale + normalize of transformers' CLIPImageProcessor (numpy backend) bit for bit; the window is its centre crop. */
int64_t pcdm_resample_ws_bytes(int Hs, int Ws, int Hd, int Wd, int channels, int ky);
int pcdm_resample_u8(const void* src, int Hs, int Ws, int channels, const int32_t* xtab, int kx, const int32_t* ytab, int ky, void* dst, int Hd, int Wd,
                     int64_t dst_pitch, int x0, int y0, void* ws, int64_t ws_bytes, pcdm_stream_t s);
int pcdm_u8_to_nchw(const void* src_u8, int Hs, int Ws, int channels, const int32_t* win, int mode, double scale, const float* mean, const float* std_,
                    float* out, pcdm_stream_t s);

/* ---- The reference's metric scripts (caculate_metrics_256.py / _512.py -> metrics.py: calculate_from_disk) on the device: the OpenCV resize in
 * front of every metric, L1 / MAE, and the uniform-window SSIM of the `ssim` array.  OpenCV and scikit-image are not dependencies: the algorithms
 * are restated from their published definitions and checked against fp64 restatements (tests/test_eval_metrics.py); parity with the packages
 * themselves is NOT pinned by a test here -- the same standing as LPIPS and FID.
 * pcdm_resize_cubic_f32: cv2.resize(img.astype(np.float32), (Wd, Hd), interpolation=cv2.INTER_CUBIC) [/ divisor] -- resizeGeneric_ with
 *   HResizeCubic / VResizeCubic and the float work type.  src HWC [Hs, Ws, 3], uint8 (src_is_f32 = 0; converted as astype does) or fp32; the result
 *   is image `index` of the fp32 batch dst, NHWC [N, Hd, Wd, 3] (nchw = 0) or NCHW [N, 3, Hd, Wd] (nchw = 1); no other image of dst is written.
 *   Per axis scale = 1.0 / ((double)n_out / (double)n_in); for output d: f = (float)((d + 0.5) * scale - 0.5) (fp64, rounded once), s = floor(f),
 *   t = f - s in fp32; taps are the source indices s - 1 .. s + 2, each clamped into [0, n_in - 1]; coefficients in fp32 with A = -0.75f:
 *   c0 = ((A (t + 1) - 5 A)(t + 1) + 8 A)(t + 1) - 4 A, c1 = ((A + 2) t - (A + 3)) t t + 1, c2 = c1 at 1 - t, c3 = 1 - c0 - c1 - c2.  The
 *   horizontal pass first, S[-1] c0 + S[0] c1 + S[1] c2 + S[2] c3 in fp32 from left to right into an fp32 row, then the vertical pass over those
 *   rows in the same way.  No antialiasing when reducing, no rounding, no clipping: the result overshoots below 0 and above 255.  Equal sizes
 *   copy the image bit for bit (t = 0: coefficients 0, 1, 0, 0).  divisor > 0: every output is x / divisor as a true fp32 division (the
 *   reference's / 255.0).  Contraction is OFF in this kernel: every multiply and add above is its own IEEE operation, no fused multiply-add
 *   (the rest of the library is built with -ffp-contract=fast), as a plain C++ build of OpenCV's generic path computes; reruns are bit-identical.
 *   One launch: a workgroup owns a 32 x 16 output tile and stages the horizontally filtered source rows it needs in LDS (24 KB).  No atomics, no
 *   workspace, no host synchronisation; every index is clamped on the device.  Returns -1 and writes nothing for channels != 3, non-positive
 *   sizes, index outside [0, N), dst (or an fp32 src) not 4-byte aligned, or an image of 2^31 elements or more.
 * pcdm_absdiff: l1[n] = mean |a - b| (compare_l1), mae[n] = sum |a - b| / sum (a + b) (compare_mae) over the windows; images, windows, ref_n and
 *   refusals as for pcdm_psnr; ws: pcdm_metrics_ws_bytes(N, ref_n, W, H, 0) bytes.  a - b and a + b are formed in fp32 per element (as numpy does
 *   on float32 arrays) and summed in fp64 -- uint8 inputs in integers, exact -- in a fixed order; the quotient is taken in fp64 and rounded to
 *   fp32 once.  A zero denominator gives what IEEE division gives (NaN or inf).  Either output may be NULL.  Two launches.
 * pcdm_ssim_box: scores[n] = skimage.metrics.structural_similarity(ref, cand[n], win_size=w, data_range=R, channel_axis=2) with skimage's
 *   defaults: five moments under a w x w mean filter, NP = w^2, covariances multiplied by NP / (NP - 1) (the sample covariance), C1 = (0.01 R)^2,
 *   C2 = (0.03 R)^2, the map averaged over the interior [p, H - p) x [p, W - p), p = (w - 1) / 2, and the channels (no tap of an averaged pixel
 *   leaves the window, so the filter's boundary mode never enters).  w odd, 3 <= w <= 51 (the reference: 51); R = data_range, or, for data_range
 *   < 0, max - min of the candidate's window.  fp64 accumulation on values centred per image, as pcdm_ssim: |score - fp64| <= 1e-5.  Other
 *   arguments and refusals as for pcdm_ssim, plus W < w or H < w; ws: pcdm_ssim_box_ws_bytes.  Three launches, no atomics. */
int pcdm_resize_cubic_f32(const void* src, int src_is_f32, int Hs, int Ws, int channels, float* dst, int N, int Hd, int Wd, int index, int nchw,
                          float divisor, pcdm_stream_t s);
int pcdm_absdiff(const void* cand, int N, int Hc, int Wc, const int32_t* cand_win, const void* ref, int ref_n, int Hr, int Wr, const int32_t* ref_win,
                 int channels, int is_f32, float* l1, float* mae, void* ws, int64_t ws_bytes, pcdm_stream_t s);
int64_t pcdm_ssim_box_ws_bytes(int N, int ref_n, int W, int H, int win_size);
int pcdm_ssim_box(const void* cand, int N, int Hc, int Wc, const int32_t* cand_win, const void* ref, int ref_n, int Hr, int Wr, const int32_t* ref_win,
                  int channels, int is_f32, int win_size, float data_range, float* scores, void* ws, int64_t ws_bytes, pcdm_stream_t s);

/* ---- DWPose pose maps from keypoints: what controlnet_aux's DWposeDetector.__call__ does after its networks (dwpose/__init__.py:55-87 -> draw_pose
 * -> util.draw_bodypose / draw_handpose / draw_facepose, then cv2.resize(..., INTER_LINEAR)), on the device.  OpenCV is not a dependency: the
 * arithmetic from keypoints to integers repeats the reference's, but the RASTER RULES below are this library's own statement of OpenCV's
 * ellipse2Poly + fillConvexPoly, circle and line; parity with the cv2 package is NOT pinned by a test here (tests/test_pose.py pins the rules
 * against Pillow's rasteriser) -- the same standing as pcdm_resize_cubic_f32.
 * pcdm_pose_draw: keypoints fp32 [M, P, 134, 2] (x, y in pixels of the Wd x Hd detection frame), scores fp32 [M, P, 134], OpenPose order (what
 *   Wholebody.__call__ returns: 18 body joints, 6 feet, 68 face, 21 left hand, 21 right hand); a map with fewer persons is padded with score 0.
 *   out uint8 [M, Hd, Wd, 3], every byte written.  tables: int32[740] in DEVICE memory, filled on the host by pcdm_pose_tables and uploaded by the
 *   caller; ws: pcdm_pose_ws_bytes(M, P) bytes, 4-byte aligned (NULL when P = 0).  Two launches, no atomics, no host synchronisation; the result
 *   does not depend on launch order.  Returns -1 and writes nothing for P > 32, a side above 4096, M > 65535 or a missing pointer.
 *   Pass 1 fills a table of 185 slots per person in DRAW ORDER, empty where the reference draws nothing: limbs (for i < 17: for person),
 *   joints (for i < 18: for person), all left hands then all right hands (20 edges then 21 points each; hands = 0: none), face points
 *   (faces = 0: none; the reference has that call commented out).  Arithmetic, every operation its own IEEE operation (no contraction, true
 *   division, correctly rounded sqrt): c = k / float(W or H) in fp32; a body joint is visible iff score > 0.3f; a hand or face point with
 *   score < 0.3f becomes c = -1.  Joint: disc of radius 4 at (int(c_x * W), int(c_y * H)) (fp32 product, truncated), colour table[i], no
 *   coordinate test.  Limb i (both joints visible): Y = c_x * float(W), X = c_y * float(H) in fp32, centre (int((Y0 + Y1) / 2), int((X0 + X1) / 2)),
 *   a = int(sqrt((X0 - X1)^2 + (Y0 - Y1)^2) / 2) in fp32, theta = int(atan2(X0 - X1, Y0 - Y1) * (180.0 / pi)) in double, colour table[i].  Hand
 *   edge e: a line between its two points (int(c_x * W), int(c_y * H)) if all four integers are >= 1, colour rint(hsv_to_rgb(e / 20, 1, 1) * 255);
 *   hand point: disc of radius 1, (0, 0, 255), if both integers are >= 1; face point: radius 3, white, same test.  Integers are clamped to
 *   +-2^20 (NaN: the lower bound), so any float is a valid keypoint.
 *   Pass 2: a workgroup owns a 32 x 8 pixel tile of one map, keeps the slots that can touch it (in order, in LDS) and every pixel takes the LAST
 *   slot that covers it: a limb as colour * 3 / 5 per channel (the canvas * 0.6 the reference applies after the limb layer), anything else as
 *   is; uncovered pixels are 0.  Coverage of pixel (x, y), integers only, dx = x - cx, dy = y - cy:
 *     limb:  C = lround(cos(theta deg) * 16384), S = lround(sin(theta deg) * 16384) (pcdm_pose_tables, double), u = 2 (dx C + dy S),
 *            v = 2 (dy C - dx S), A = 2 a + 1, B = 9: |u| <= A * 16384 and |v| <= B * 16384 and B^2 u^2 + A^2 v^2 <= A^2 B^2 2^28 -- the ellipse of
 *            half-axes (a, 4) inflated by half a pixel (fillConvexPoly paints the outline too); a = 0 needs no special case.  The last test is
 *            evaluated in 128 bits, so no a overflows it.
 *     disc of radius r:  dx^2 + dy^2 <= r^2 + r / 2 (integer division).
 *     line (x0, y0) - (x1, y1), one pixel wide: the major axis is x when |x1 - x0| >= |y1 - y0|; with n = the major |delta| and k = 0 .. n the
 *            major coordinate is start + sgn * k and the minor one start + sgn * floor((2 k |minor delta| + n) / (2 n)); evaluated per pixel.
 * pcdm_pose_tables: fills HOST int32[count = 740]: {C, S} of 0 .. 359 degrees, then the 20 hand-edge colours as r | g << 8 | b << 16
 *   (matplotlib's hsv_to_rgb in double, rounded half to even).
 * pcdm_resize_linear_u8: cv2.resize(uint8 image, (Wd, Hd), interpolation=cv2.INTER_LINEAR) in OpenCV's 8-bit fixed-point form, src
 *   [M, Hs, Ws, 3] -> dst [M, Hd, Wd, 3].  Per axis scale = 1.0 / ((double)n_out / (double)n_in), f = (float)((d + 0.5) * scale - 0.5), s = floor(f),
 *   t = f - s in fp32; weights w0 = rint((1 - t) * 2048), w1 = rint(t * 2048).  Horizontally an index outside [0, n_in - 2] is clamped and its
 *   t set to 0; vertically the two rows s, s + 1 are clamped into the image and t is kept.  S = src[s] w0 + src[s + 1] w1 in int per row,
 *   out = (((b0 * (S0 >> 4)) >> 16) + ((b1 * (S1 >> 4)) >> 16) + 2) >> 2.  Equal sizes copy.  One launch; -1 for non-positive sizes or 2^31 bytes.
 * pcdm_resize_cv_u8: cv2.resize(uint8 image, (Wd, Hd), interpolation=cv2.INTER_LANCZOS4 | cv2.INTER_AREA), the resampling of controlnet_aux's
 *   resize_image (util.py:87-97: Lanczos4 when the picture is enlarged, area otherwise), src [M, Hs, Ws, 3] -> dst [M, Hd, Wd, 3].  The rules are
 *   restated from OpenCV's published generic (non-SIMD) path; coefficient details have differed between OpenCV releases, and parity with the cv2
 *   package is NOT pinned by a test here (tests/test_resize_cv.py pins them against an independent restatement and against their fp64
 *   definitions).  `rule` names the arithmetic, the caller picks it as cv2 does (pcdms_amd/preprocess.py: resize_cv); xtab / ytab are the tables of
 *   the two axes, int32 in DEVICE memory, built on the host.  Per axis scale = 1.0 / ((double)n_out / (double)n_in).
 *   rule 0, INTER_LANCZOS4 (any size change; no antialiasing when reducing).  Table [s (n_out) | coeff (n_out * 8)].  For output d:
 *     f = (float)((d + 0.5) * scale - 0.5), s = floor(f), t = f - s in fp32; the eight taps are the sources s - 3 .. s + 4, each clamped into
 *     [0, n_in - 1].  Real coefficients for t >= FLT_EPSILON, in double: y0 = -(t + 3) pi / 4, s0 = sin(y0), c0 = cos(y0),
 *     c_i = (float)((a_i s0 + b_i c0) / (y_i y_i)) with y_i = -(t + 3 - i) pi / 4 and (a_i, b_i) = (1, 0), (-r, -r), (0, 1), (r, -r), (-1, 0), (r, r),
 *     (0, -1), (-r, r), r = 0.70710678118654752440; they are summed in fp32 in index order and each multiplied by 1.f / sum; for t < FLT_EPSILON
 *     they are (0, 0, 0, 1, 0, 0, 0, 0).  coeff = rint(c_i * 2048) (ties to even) saturated to int16; the eight need not sum to 2048.
 *     S = sum src alpha in int32 per source row, out = clip8((sum_k S_k beta_k + 2^21) >> 22), the vertical sum in 64-bit integers (so no image
 *     overflows it; an int32 accumulator differs only where |sum| >= 2^31, which pictures do not reach).  Sines and cosines are taken on the host
 *     only: the device reads integers.
 *   rule 1, INTER_AREA on integer ratios (scale_x, scale_y integers >= 1 within DBL_EPSILON; no tables, NULL is fine): the sx x sy box of every
 *     output; 2 x 2: (a + b + c + d + 2) >> 2; any other box: the int32 sum times (float)(1.f / (sx sy)) as ONE fp32 multiply, rounded to nearest
 *     even and saturated.  -1 when a ratio is no such integer or sx sy > 2^23.
 *   rule 2, INTER_AREA proper (scale_x >= 1 and scale_y >= 1, else -1).  Table [count (n_out) | source (n_out * k) | weight as fp32 bits
 *     (n_out * k)], k = (int)scale + 2; output d lists, with f1 = d scale, f2 = f1 + scale, cell = min(scale, n_in - f1), s1 = ceil(f1),
 *     s2 = min(floor(f2), n_in - 1), s1 = min(s1, s2): (s1 - 1, (float)((s1 - f1) / cell)) if s1 - f1 > 1e-3; (j, (float)(1.0 / cell)) for
 *     j = s1 .. s2 - 1; (s2, (float)(min(min(f2 - s2, 1.0), cell) / cell)) if f2 - s2 > 1e-3.  fp32, every multiply and add its own IEEE operation
 *     (no contraction, as pcdm_resize_cubic_f32): per source row of an output row, in table order, buf = 0 then buf = buf + (float)src alpha entry
 *     by entry; sum = beta buf for the first row, sum = sum + beta buf for every later one; out = rint(sum) (ties to even), saturated.
 *   rule 3, INTER_AREA when either axis enlarges (cv2 then takes its 8-bit bilinear path with other indices).  Table [s (n_out) | w0, w1
 *     (n_out * 2)]: s = floor(d scale), t = (float)((d + 1) - (s + 1) (1 / scale)), t = 0 if t <= 0 else t - floor(t), on BOTH axes;
 *     w0 = rint((1 - t) * 2048), w1 = rint(t * 2048); horizontally s >= n_in - 1 is clamped to n_in - 1 with t = 0.  The rows s, s + 1 and the
 *     columns s, s + 1 are clamped into the image on the device and the arithmetic is pcdm_resize_linear_u8's: S = src[s] w0 + src[s + 1] w1,
 *     out = (((b0 * (S0 >> 4)) >> 16) + ((b1 * (S1 >> 4)) >> 16) + 2) >> 2.  Weights are clamped into [0, 2048].
 *   Equal sizes copy under every rule (cv2's dsize == ssize return) and read no table.  Every table entry is clamped on the device -- indices
 *   into the image, counts into [0, k], coefficients into their range -- so a wrong table gives wrong pixels, never an access outside src or
 *   dst.  One launch, a lane per output pixel; no workspace, no atomics, no host synchronisation; reruns are bit-identical and an image's result
 *   does not depend on its place in the batch.  Returns -1 and writes nothing for a NULL src or dst, non-positive sizes, M < 0, an unknown rule,
 *   a NULL table the rule needs, or 2^31 bytes or more on either side; M = 0 returns 0. */
int pcdm_pose_tables(int32_t* tables, int count);
int64_t pcdm_pose_ws_bytes(int M, int P);
int pcdm_pose_draw(const float* keypoints, const float* scores, int M, int P, int Hd, int Wd, int hands, int faces, const int32_t* tables, void* out,
                   void* ws, int64_t ws_bytes, pcdm_stream_t s);
int pcdm_resize_linear_u8(const void* src, int M, int Hs, int Ws, void* dst, int Hd, int Wd, pcdm_stream_t s);
int pcdm_resize_cv_u8(const void* src, int M, int Hs, int Ws, void* dst, int Hd, int Wd, int rule, const int32_t* xtab, const int32_t* ytab,
                      pcdm_stream_t s);

/* ---- The whole-body pose estimator: image + person boxes -> 133 keypoints and scores per box (what Wholebody.__call__ gets from its second
 * network, the top-down DWPose-l of mmpose: CSPNeXt-l backbone, RTMCC head, SimCC decoding).  The boxes come from the person detector below
 * (pcdm_detect_forward) or from the caller.  mmpose and mmdet are not dependencies; the network is restated from its published definition below, and parity with mmpose on
 * the published checkpoint is NOT pinned by a test that runs by default (tests/test_dwpose.py holds a dormant pin) -- the same standing as LPIPS, FID
 * and the OpenCV rules.  Everything is fp32; activations are NHWC with channels padded to multiples of 4 (padding channels exactly 0).  The schedule
 * is one C call, pcdm_dwpose_forward, or the same launches driven from the host (pcdms_amd/pose.py: DWPoseEstimator); these are its kernels.  No atomics, no allocation, no host synchronisation, fixed
 * summation orders: reruns are bit-identical and a crop's result does not depend on its place in the batch.  Arguments outside the stated ranges
 * return -1 and write nothing.
 *
 * Box -> crop (GetBBoxCenterScale, TopdownAffine without UDP), fp32, every operation its own: c = ((x1 + x2) 0.5, (y1 + y2) 0.5),
 *   (w, h) = (x2 - x1, y2 - y1) 1.25; ar = Win / Hin: if w > h ar then h = w / ar else w = h ar.  The warp is one scale s = Win / w about the centre
 *   (no rotation; mmpose derives it from the widths), destination centre (0.5 Win, 0.5 Hin).
 * pcdm_pose_crop: images uint8 [N, H, W, 3] (RGB), boxes fp32 [R, 4] = (x1, y1, x2, y2) in DEVICE memory, image_index int32 [R] on the device (NULL:
 *   image 0; an index outside [0, N) gives a black crop) -> out fp32 NHWC [R or 2 R, Hin, Win, 4].  Sampling is this library's statement of OpenCV's
 *   8-bit warpAffine(INTER_LINEAR, BORDER_CONSTANT 0): in double, inv = w / Win, bx = cx - 0.5 Win inv, by = cy - 0.5 Hin inv (the inverse map
 *   xs = (xd - 0.5 Win) / s + cx split into its two terms); X = (rint(bx 1024) + 16 + rint(inv xd 1024)) >> 5, Y likewise from by and yd (rint: half
 *   to even, saturated to int32, NaN the lower bound; 64-bit sums): a 1/32 sub-pixel grid, sx = X >> 5, fx = X & 31.  The four weights of the
 *   32 x 32 table at scale 2^15 are exact products, (32 - fx)(32 - fy) 32, fx (32 - fy) 32, (32 - fx) fy 32, fx fy 32 (sum 2^15; the table is not
 *   stored); pixels outside the image are 0; value = (sum + 2^14) >> 15 per channel.  Then (value - mean_c) / std_c in fp32 with mean (123.675,
 *   116.28, 103.53), std (58.395, 57.12, 57.375); channel 3 = 0.  flip: crops R .. 2 R - 1 are crops 0 .. R - 1 mirrored in x (destination column
 *   Win - 1 - x of the SAME crop, not a warp of the mirrored image).  One launch.  Hin, Win <= 4096.
 * pcdm_conv2d_f32_act: pcdm_conv2d_f32_ex (same packed weights, same k order) plus: the input is the channel slice [in_offset, in_offset + Cin) of
 *   an NHWC tensor with in_pitch channels per pixel (both multiples of 4); act 0 none, 1 ReLU, 2 SiLU = v / (1 + exp(-v)); residual (or NULL): the
 *   slice [res_offset, res_offset + Cout) of an NHWC tensor [B, Ho, Wo, res_pitch], added AFTER the activation (it may be the output slice itself);
 *   a_scale (or NULL): fp32 [B, Cin], 16-byte aligned: the A operand of image b, channel c is x a_scale[b, c] (one fp32 product) -- the channel
 *   attention folded into the convolution that consumes it.  The output slice must not overlap the INPUT slice (-1 when both are slices of one
 *   tensor of one pitch; other aliasing is the caller's to avoid); this holds for pcdm_dwconv5_silu_f32 and pcdm_maxpool5_f32 too.  With in_pitch = Cin, in_offset = 0, act <= 1, no residual and no a_scale the result
 *   is bit for bit pcdm_conv2d_f32_ex's.  A linear layer is the 1 x 1 case with B = 1, Hi = 1, Wi = rows.
 * pcdm_dwconv5_silu_f32: depthwise 5 x 5, pad 2, stride 1, + bias, SiLU on the slice [in_offset, +C) of [B, H, W, in_pitch] into the slice
 *   [out_offset, +C) of [B, H, W, out_pitch]; w fp32 [25, C] (tap ky 5 + kx, then channel), bias [C]; C, pitches, offsets multiples of 4.  One
 *   fmaf chain per output over the taps in (ky, kx) order, taps outside the image skipped.
 * pcdm_maxpool5_f32: MaxPool2d(5, stride 1, pad 2) between channel slices as above (the two may be disjoint slices of one tensor): the padding never
 *   wins, a NaN does.  SPP's 5 / 9 / 13 pools are this one cascaded, which is exact for a maximum.
 * pcdm_fc_hsigmoid_f32: out[b, n] = clamp(sum_c w[n, c] x[b, c] + bias[n] + 3, 0, 6) / 6 for x fp32 [B, C], w [C, C]: ChannelAttention's vector
 *   from pcdm_global_avgpool_f32's means.
 * pcdm_scalenorm_f32: out[b rows + k, i] = x / max(|x|_2 dim^-0.5, eps) g[0] over i < dim, element i of row (b, k) at x[b batch_stride + k row_stride
 *   + i elem_stride]; columns dim .. out_pitch - 1 are written 0.  side_out (with side_scale fp32 [dim], or both NULL): side_out[row, i] =
 *   x side_scale[i].  g in device memory.
 * pcdm_gau_core_f32: uv fp32 [B T, 2 e + 128] = (u | v | base) per token, gamma / beta fp32 [2, 128]: q = base gamma[0] + beta[0], k = base gamma[1] +
 *   beta[1], A = relu(q k^T / sqrt(128))^2 over the T tokens of a crop, out fp32 [B T, e] = u (A v).  T <= 256, e a multiple of 4.
 * pcdm_simcc_decode: simcc_x fp32 [R2 K, x_pitch] (x_bins logits), simcc_y [R2 K, y_pitch] (y_bins), R2 = 2 R with flip: crop R + r is crop r
 *   mirrored, its output for keypoint k is row flip_idx[k] (int32 [K] on the device) with the x bins reversed; merged = 0.5 (plain + flipped).  Per
 *   axis loc = argmax (np.argmax: the first maximum, a NaN ranks highest); score = max_x > max_y ? max_y : max_x (raw logits); both loc = -1 where
 *   score <= 0; keypoints [R, K, 2] = (loc / 2) / (Win, Hin) (w, h) + c - 0.5 (w, h) in fp32, each operation its own; scores [R, K].
 *
 * The network (Conv = convolution without bias + BatchNorm(eps 1e-5: the config's bare SyncBN) + SiLU, the BatchNorm folded on the host in fp64):
 *   stem: Conv 3x3 s2 3 -> 32, Conv 3x3 32 -> 32, Conv 3x3 32 -> 64.  Four stages (in, out, blocks, identity, spp) = (64, 128, 3, yes, no),
 *   (128, 256, 6, yes, no), (256, 512, 6, yes, no), (512, 1024, 3, no, yes): Conv 3x3 s2 in -> out; with spp: Conv 1x1 out -> out/2, max-pools 5 / 9
 *   / 13 (stride 1, same size), cat [x, p5, p9, p13], Conv 1x1 2 out -> out; then the CSP layer, mid = out / 2: main = Conv 1x1 -> mid, short = Conv
 *   1x1 -> mid, the blocks on main (Conv 3x3 mid -> mid; depthwise 5x5 + BN + SiLU; Conv 1x1 mid -> mid; + input when identity), cat (main, short),
 *   x hardsigmoid(fc(global mean(x))) with fc a 1x1 convolution with bias, Conv 1x1 -> out.  Head on the stride-32 map [h, w] of 1024 channels:
 *   Conv2d 7x7 pad 3 with bias -> K maps, flattened to [K, h w]; ScaleNorm(h w); Linear(h w -> 256); GAU: hn = ScaleNorm(256)(x), (u, v, base) =
 *   split(SiLU(Linear(256 -> 1152)(hn)), 512, 512, 128), the core above, x res_scale + Linear(512 -> 256)(core); Linear(256 -> 2 Win) and
 *   Linear(256 -> 2 Hin) give the SimCC logits.  No linear has a bias. */
/* pcdm_dwpose_forward: the whole estimator as ONE C call (as pcdm_inception_features): crop, backbone, head and decode, 60-odd launches on the
 *   caller's stream, on one caller-owned workspace of pcdm_dwpose_ws_bytes(cfg, R, flip) bytes (16-byte aligned), keypoints fp32 [R, K, 2] and scores
 *   fp32 [R, K] out.  Bit for bit the per-kernel calls above in the same order (pcdms_amd/pose.py runs either).  cfg: the crop size, K <= 256, the
 *   stem's and the four stages' output channels (multiples of 8), blocks per stage, identity / spp flags.  wts: HOST arrays of DEVICE pointers --
 *   conv_w / conv_b [n_conv]: the packed convolutions (pcdm_pack_lpips_conv, BatchNorm folded) in schedule order: stem 0, 1, 2; per stage: the
 *   strided convolution, (spp: conv1, conv2,) main_conv, short_conv, per block conv1 and pointwise_conv, final_conv; then final_layer, mlp.1,
 *   gau.uv, gau.o, and cls_x and cls_y as ONE linear (x rows first); dw_w / dw_b [n_dw]: the depthwise layers in block order ([25, C] and [C]);
 *   fc_w / fc_b: the four attention layers; mlp_g, ln_g ([1]), gamma, beta ([2, 128]), res_scale ([256]); flip_idx (int32 [K]; may be NULL
 *   without flip).  -1 and nothing written for a NULL pointer, counts that do not match cfg, or sizes outside the ranges above. */
typedef struct pcdm_dwpose_config {
    int32_t Hin, Win, K;
    int32_t stem;
    int32_t n_stages;               /* 4 */
    int32_t out[4], blocks[4], identity[4], spp[4];
} pcdm_dwpose_config;
typedef struct pcdm_dwpose_weights {
    const float* const* conv_w;
    const float* const* conv_b;
    const float* const* dw_w;
    const float* const* dw_b;
    int32_t n_conv, n_dw;
    const float* fc_w[4];
    const float* fc_b[4];
    const float* mlp_g;
    const float* ln_g;
    const float* gamma;
    const float* beta;
    const float* res_scale;
    const int32_t* flip_idx;
} pcdm_dwpose_weights;
int64_t pcdm_dwpose_ws_bytes(const pcdm_dwpose_config* cfg, int R, int flip);
int pcdm_dwpose_forward(const void* images, int N, int H, int W, const float* boxes, const int32_t* image_index, int R, int flip,
                        const pcdm_dwpose_config* cfg, const pcdm_dwpose_weights* wts, float* keypoints, float* scores, void* ws, int64_t ws_bytes,
                        pcdm_stream_t s);
int pcdm_pose_crop(const void* images, int N, int H, int W, const float* boxes, const int32_t* image_index, int R, int flip, int Hin, int Win, float* out,
                   pcdm_stream_t s);
int pcdm_conv2d_f32_act(const float* x, int B, int Hi, int Wi, int Cin, int in_pitch, int in_offset, const float* w_packed, const float* bias, int Cout,
                        int kh, int kw, int stride, int pad_h, int pad_w, int act, const float* residual, int res_pitch, int res_offset,
                        const float* a_scale, float* out, int out_pitch, int out_offset, pcdm_stream_t s);
int pcdm_dwconv5_silu_f32(const float* x, int B, int H, int W, int C, int in_pitch, int in_offset, const float* w, const float* bias, float* out,
                          int out_pitch, int out_offset, pcdm_stream_t s);
int pcdm_maxpool5_f32(const float* x, int B, int H, int W, int C, int in_pitch, int in_offset, float* out, int out_pitch, int out_offset, pcdm_stream_t s);
int pcdm_fc_hsigmoid_f32(const float* x, int B, int C, const float* w, const float* bias, float* out, pcdm_stream_t s);
int pcdm_scalenorm_f32(const float* x, int B, int rows, int dim, int64_t batch_stride, int64_t row_stride, int64_t elem_stride, float eps, const float* g,
                       float* out, int out_pitch, const float* side_scale, float* side_out, int side_pitch, pcdm_stream_t s);
int pcdm_gau_core_f32(const float* uv, int B, int T, int e, const float* gamma, const float* beta, float* out, pcdm_stream_t s);
int pcdm_simcc_decode(const float* simcc_x, int x_pitch, int x_bins, const float* simcc_y, int y_pitch, int y_bins, int R, int K, int flip,
                      const int32_t* flip_idx, const float* boxes, int Hin, int Win, float* keypoints, float* scores, pcdm_stream_t s);

/* ---- The person detector: image -> person boxes (what Wholebody.__call__ gets from its first network, mmdet's YOLOX-l of
 * yolox_l_8xb8-300e_coco.py, after it keeps label 0 with score > 0.5 and applies mmpose's nms(0.7)).  mmdet, mmpose and mmcv are not dependencies;
 * the network is restated from its published definition below, and parity with mmdet on the published checkpoint is NOT pinned by a test that
 * runs by default (tests/test_person_detector.py holds a dormant pin) -- the same standing as DWPose, LPIPS and FID.  Everything is fp32;
 * activations are NHWC with channels padded to multiples of 4 (padding channels exactly 0).  No atomics, no allocation, no host synchronisation,
 * fixed orders: reruns are bit-identical and an image's result does not depend on its place in the batch.  Arguments outside the stated ranges
 * return -1 and write nothing.
 *
 * Input (mmdet's test pipeline: Resize(keep_ratio), Pad(pad_to_square, 114)): with S the detector's square size (a multiple of 32, 32 .. 4096),
 *   f = S / max(H, W) in double, (Wr, Hr) = (int(W f + 0.5), int(H f + 0.5)) (pcdm_detect_resized; -1 if a side would vanish); the image is resized
 *   to Wr x Hr by pcdm_resize_linear_u8's rule and placed top-left in an S x S canvas that is 114 elsewhere; the scale factor is (Wr / W, Hr / H),
 *   each rounded to fp32.  The network sees B, G, R (the reference hands mmdet a BGR array; YOLOX's preprocessor neither swaps nor normalises),
 *   values 0 .. 255.
 * pcdm_detect_prep: images uint8 RGB [N, H, W, 3] -> the Focus tensor fp32 [N, S/2, S/2, 12]: channel (patch p) 3 + c with the patches in the order
 *   top-left, bottom-left, top-right, bottom-right ((dy, dx) = (0, 0), (1, 0), (0, 1), (1, 1)) and c over B, G, R.  One launch.
 * pcdm_upsample2_nearest_f32: out[b, y, x, out_offset + c] = x[b, y / 2, x / 2, in_offset + c] for x [B, H, W, in_pitch], out [B, 2 H, 2 W,
 *   out_pitch]; C, pitches, offsets multiples of 4.  As for pcdm_conv2d_f32_act, -1 when both are overlapping slices of one tensor given by one base
 *   pointer and one pitch; any other aliasing (another base pointer into the same allocation, another pitch) is the caller's to avoid.
 *
 * The network (Conv = convolution without bias + BatchNorm(eps 1e-3) + SiLU, the BatchNorm folded on the host in fp64):
 *   backbone (CSPDarknet P5): stem Conv 3x3 12 -> 64 on the Focus tensor.  Four stages (in, out, blocks, identity, spp) = (64, 128, 3, yes, no),
 *   (128, 256, 9, yes, no), (256, 512, 9, yes, no), (512, 1024, 3, no, yes): Conv 3x3 s2 in -> out; with spp: Conv 1x1 out -> out/2, max-pools 5 / 9 /
 *   13 (stride 1, same size), cat [x, p5, p9, p13], Conv 1x1 2 out -> out; then the CSP layer, mid = out / 2: main = Conv 1x1 -> mid, short = Conv 1x1
 *   -> mid, the blocks on main (Conv 1x1 mid -> mid, Conv 3x3 mid -> mid, + block input when identity), cat (main, short), Conv 1x1 2 mid -> out.
 *   Outputs c3, c4, c5 = stages 2, 3, 4 (256 @ S/8, 512 @ S/16, 1024 @ S/32).
 *   neck (YOLOXPAFPN; every CSP layer has 3 blocks without identity; up2 = nearest x 2): r5 = reduce_layers.0 Conv 1x1 1024 -> 512 (c5);
 *   t4 = top_down_blocks.0 CSP(1024 -> 512)(cat [up2(r5), c4]); r4 = reduce_layers.1 Conv 1x1 512 -> 256 (t4); p3 = top_down_blocks.1 CSP(512 ->
 *   256)(cat [up2(r4), c3]); p4 = bottom_up_blocks.0 CSP(512 -> 512)(cat [downsamples.0 Conv 3x3 s2 256 -> 256 (p3), r4]); p5 = bottom_up_blocks.1
 *   CSP(1024 -> 1024)(cat [downsamples.1 Conv 3x3 s2 512 -> 512 (p4), r5]); out_convs.i Conv 1x1 -> 256 on p3, p4, p5.
 *   head, per level i: multi_level_cls_convs.i and multi_level_reg_convs.i, two Conv 3x3 256 -> 256 each; multi_level_conv_cls.i Conv2d 1x1 with bias
 *   -> C classes on the cls branch; multi_level_conv_reg.i (-> 4) and multi_level_conv_obj.i (-> 1), Conv2d 1x1 with bias, both on the reg branch.
 *   Two load-time merges, bit-identical per output: main_conv and short_conv run as one convolution, conv_reg and conv_obj as one.  A level's
 *   head tensor is fp32 [N, S/stride, S/stride, 8 + C4]: reg 0 .. 3, obj 4, 5 .. 7 zero, the class logits from 8 (C4 = C rounded up to 4, padding 0).
 *
 * Decode and selection (YOLOXHead.predict_by_feat for one class of interest; then mmpose's nms):
 * pcdm_detect_decode: priors in level order (stride 8, 16, 32), row-major, at (x, y) = (col, row) stride; P = 21 (S / 32)^2 an image.  Per prior,
 *   in fp32, every operation its own: centre = pred_xy stride + (x, y); wh = exp(pred_wh) stride; box = centre -+ wh / 2; label = the first argmax
 *   of the C class logits after sigmoid; score = sigmoid(max cls) sigmoid(obj); the box is divided by the scale factor (x by Wr / W, y by Hr / H),
 *   BEFORE the NMS, as in mmdet.  candidates[n, i] = label == class_id and score >= 0.01 and score > score_thr.  Out: boxes fp32 [N, P, 4], scores
 *   [N, P], labels and candidates int32 [N, P].  The reference applies its 0.5 filter after mmdet's NMS; a greedy NMS in descending score order
 *   never lets a lower score suppress a higher one, so filtering first gives the same set.
 * pcdm_nms_f32: one greedy pass per image over the boxes whose flags[n, i] != 0 (a NaN score is never one), in the order (score descending, index
 *   ascending), made by counting, without atomics.  If more than max_candidates (<= 1024) are flagged, the best max_candidates are used.  In that
 *   order a box that is still kept suppresses every later one with IoU > thr, IoU = inter / (area a + area b - inter) with `offset` added to every
 *   width and height (mmcv's nms: offset 0; mmpose's: 1); equality keeps; a suppressed box suppresses nothing.  keep (or NULL): int32 [N, P] flags of
 *   the first max_det kept (it must not be `flags`); out_boxes fp32 [N, max_det, 4] / out_scores [N, max_det] (both or neither; one of keep and
 *   out_boxes must be given): the first max_det kept in order, the rows behind them 0; count int32 [N] (or NULL) = the rows written; overflow int32
 *   [N] (or NULL) = more than max_candidates flagged, or more than max_det kept, or overflow_in[n] (int32 [N] or NULL) != 0.  1 <= max_det <=
 *   max_candidates.  One launch, one workgroup an image; N P < 2^24.  Untuned: every flagged box reads all P scores for its rank, so the cost grows
 *   with P times the number of flagged boxes (measured only as part of pcdm_detect_forward: profiles/yolox_bench.json).
 * pcdm_detect_forward: prep, network, decode and the two passes -- pcdm_nms_f32(candidates, nms_thr 0.65, offset 0) then pcdm_nms_f32(its keep,
 *   pose_nms_thr 0.7, offset 1) -- as ONE C call on one caller-owned workspace of pcdm_detect_ws_bytes(cfg, N) bytes (16-byte aligned).  Bit for bit
 *   the per-kernel calls in the same order (pcdms_amd/pose.py: PersonDetector runs either).  Out: boxes fp32 [N, max_det, 4] (x1, y1, x2, y2 in
 *   pixels of the image, score order, rows beyond count 0), scores [N, max_det], count and overflow int32 [N].  cfg: S; num_classes (<= 1024) and
 *   class_id; the stem's, the four stages' and the head's channels (multiples of 8); blocks per stage and per neck CSP layer (<= 64);
 *   max_candidates (1 .. 1024) and max_det (1 .. max_candidates); the three thresholds.  wts: HOST arrays of DEVICE pointers, conv_w / conv_b
 *   [n_conv]: the packed convolutions (pcdm_pack_lpips_conv, BatchNorm folded) in schedule order: stem; per stage: the strided convolution, (spp:
 *   conv1, conv2,) main_conv | short_conv as one, per block conv1 and conv2, final_conv; reduce_layers.0, top_down_blocks.0, reduce_layers.1,
 *   top_down_blocks.1, downsamples.0, bottom_up_blocks.0, downsamples.1, bottom_up_blocks.1 (CSP layers as above), out_convs 0 .. 2; per level:
 *   cls_convs 0, 1, conv_cls (C4 outputs, the padding rows 0), reg_convs 0, 1, conv_reg | conv_obj as one (8 outputs, rows 5 .. 7 zero).  -1 and
 *   nothing written for a NULL pointer, a count that does not match cfg, or sizes outside the ranges above. */
typedef struct pcdm_detect_config {
    int32_t S;
    int32_t num_classes, class_id;
    int32_t stem, head;
    int32_t out[4], blocks[4];
    int32_t neck_blocks;
    int32_t max_candidates, max_det;
    float score_thr, nms_thr, pose_nms_thr;
} pcdm_detect_config;
typedef struct pcdm_detect_weights {
    const float* const* conv_w;
    const float* const* conv_b;
    int32_t n_conv;
} pcdm_detect_weights;
int pcdm_detect_resized(int H, int W, int S, int* Hr, int* Wr);
int pcdm_detect_prep(const void* images, int N, int H, int W, int S, float* out, pcdm_stream_t s);
int pcdm_upsample2_nearest_f32(const float* x, int B, int H, int W, int C, int in_pitch, int in_offset, float* out, int out_pitch, int out_offset,
                               pcdm_stream_t s);
int pcdm_detect_decode(const float* head8, const float* head16, const float* head32, int N, int S, int num_classes, int class_id, float score_thr, int H,
                       int W, float* boxes, float* scores, int32_t* labels, int32_t* candidates, pcdm_stream_t s);
int pcdm_nms_f32(const float* boxes, const float* scores, const int32_t* flags, int N, int P, int max_candidates, int max_det, float thr, float offset,
                 const int32_t* overflow_in, int32_t* keep, float* out_boxes, float* out_scores, int32_t* count, int32_t* overflow, pcdm_stream_t s);
int64_t pcdm_detect_ws_bytes(const pcdm_detect_config* cfg, int N);
int pcdm_detect_forward(const void* images, int N, int H, int W, const pcdm_detect_config* cfg, const pcdm_detect_weights* wts, float* boxes,
                        float* scores, int32_t* count, int32_t* overflow, void* ws, int64_t ws_bytes, pcdm_stream_t s);

/* ---- The UNet forward as ONE entry ("a fused unet_forward(ctx, ...)" over an opaque context).
 * Replaces Stage2_InapintUNet2DConditionModel.forward (/root/reference/src/models/stage2_inpaint_unet_2d_condition.py:579-825) for a host
 * that is not Python: pcdm_unet_create from the topology, pcdm_unet_set_weight / _set_vector with the packed tensors under their
 * diffusers module paths, ONE caller-owned workspace (pcdm_unet_workspace_bytes, zeroed once by pcdm_unet_workspace_init), then per
 * sampling call pcdm_unet_prepare_conditioning (class embedding, pose feature, cross-attention K / V^T: step-invariant) and per denoise
 * step pcdm_unet_forward.  No allocation inside, every launch on the caller's stream, fixed scratch addresses (hipGraph-capturable).
 * Weight names (N = diffusers module path, e.g. "down_blocks.0.resnets.1." / "...attentions.0."):
 *   optional "up_blocks.i.upsamplers.0.conv4" (the upsampler's convolution as four 2x2 phase kernels: pcdm_gemm_params.tap_lut; used when the target is 2H x 2W),
 *   conv_in, conv_out, N"conv1", N"conv2", N"conv_shortcut", optional N"conv2s" (conv2's packed rows with conv_shortcut's [N, Cx] appended along K,
 *   bias = the sum: when registered, conv2 + conv_shortcut of that resnet run as ONE launch through pcdm_gemm_params.a2 / a3), "down_blocks.i.downsamplers.0.conv", "up_blocks.i.upsamplers.0.conv"  (pcdm_pack conv3x3 / linear)
 *   N"proj_in", N"proj_out", N"qkv" (to_q|to_k|to_v rows), N"o1", N"q2", N"kv2" (to_k|to_v of attn2), N"o2", N"ff1" (GEGLU packing), N"ff2",
 *   optional N"qkv_ln" / N"q2_ln" / N"ff1_ln" (LayerNorm folded, with wsum), optional N"ffo" = [Wp W2 | Wp] with bias Wp b2 + bp (W2, b2 = ff.net.2;
 *   Wp, bp = proj_out; N = C, K = 5 C: when registered, ff.net.2 (+ residual) -> proj_out (+ residual) of that block run as ONE two-source GEMM),
 *   "time_emb_proj" (all resnets' rows concatenated in resnet order),
 *   "time_embedding.linear_1/2", "class_embedding.linear_1/2" (bf16 [N, K] unpadded + fp32 bias, for pcdm_small_linear)
 * Vectors (fp32): N"norm1.weight" / ".bias", N"norm2.*" (resnets), N"norm.*" and N"transformer_blocks.0.norm{1,2,3}.*" (transformers),
 *   "conv_norm_out.weight" / ".bias".
 * Tile choices: a new context starts with the committed tuning table (pcdms_amd/tuning/gfx950.json, measured on MI355X; compiled in through
 * csrc/tuning_table.inc) -- the (tile, split_k) pcdm_gemm should use for a problem key (ln, M, Npad, K, conv, stride, upsample, epilogue,
 * two_source, residual, flag: 1 = zero_rows, 2 = dup_rows); pcdm_unet_set_tile overrides / adds entries, pcdm_unet_get_tile reads one (-1: none:
 * the library heuristic decides).
 * Return codes as everywhere; pcdm_unet_last_error names the missing weight / failing call. */
typedef struct pcdm_unet pcdm_unet;
typedef struct pcdm_unet_config {
    int32_t out_channels;
    int32_t n_levels;               /* <= 8 */
    int32_t block_out_channels[8];  /* multiples of 64; heads[i] * 64 == block_out_channels[i] */
    int32_t heads[8];
    int32_t cross_attn[8];          /* down block i is CrossAttnDownBlock2D (up block n-1-i mirrors it) */
    int32_t layers_per_block;
    int32_t cross_attention_dim;
    int32_t norm_groups;
    float norm_eps;
    int32_t class_embed;            /* 1: "projection" class embedding (stage 2), 0: none (stage 3) */
    int32_t flip_sin_to_cos;
    float freq_shift;
} pcdm_unet_config;
pcdm_unet* pcdm_unet_create(const pcdm_unet_config* cfg);
void pcdm_unet_destroy(pcdm_unet* u);
const char* pcdm_unet_last_error(const pcdm_unet* u);
int pcdm_unet_set_weight(pcdm_unet* u, const char* name, const void* w_bf16, const float* bias, const float* wsum, int N, int K, int Npad, int cin);
int pcdm_unet_set_vector(pcdm_unet* u, const char* name, const float* v, int n);
int pcdm_unet_set_tile(pcdm_unet* u, int ln, int M, int Npad, int K, int conv, int stride, int upsample, int epilogue, int two_source, int residual,
                       int zero_rows, int tile, int split_k);
/* 1: every attention of the UNet with OCP e4m3 K / V^T / Q / P operands (pcdm_quantize_fp8 + pcdm_flash_attn_fp8; BASELINE.json configs[4]), 0
 * (default): bf16.  Switch before pcdm_unet_prepare_conditioning (it quantises the context K / V^T) and before capturing a graph. */
int pcdm_unet_set_attention_fp8(pcdm_unet* u, int on);
/* FreeU in the two lowest-resolution up blocks (pcdm_freeu in front of every resnet of up block 0 with (b1, s1) and of up block 1 with (b2, s2);
 * diffusers 0.24.0 enable_freeu(s1, s2, b1, b2)); on = 0 (default): off, the four floats are ignored.  Only while it is on does the plan hold
 * the FreeU buffers ("fu_s", "fu_ws"): with it off pcdm_unet_workspace_bytes / _layout answer as without this call.  Switching re-plans (buffers
 * move: run pcdm_unet_workspace_init and pcdm_unet_prepare_conditioning again, and capture again); changing only the floats does not. */
int pcdm_unet_set_freeu(pcdm_unet* u, int on, float s1, float s2, float b1, float b2);
int pcdm_unet_get_tile(const pcdm_unet* u, int ln, int M, int Npad, int K, int conv, int stride, int upsample, int epilogue, int two_source, int residual,
                       int flag, int* tile, int* split_k);
int64_t pcdm_unet_workspace_bytes(pcdm_unet* u, int B, int h, int w, int L);
int pcdm_unet_workspace_init(pcdm_unet* u, int B, int h, int w, int L, void* workspace, pcdm_stream_t s);
/* ehs fp32 [B, L, cross_attention_dim]; class_labels fp32 [B, K of class_embedding.linear_1] or NULL; pose fp32 NCHW [pose_b = 1 | B, C0, h, w] or
 * NULL; zero_ctx_batches: leading batch entries of ehs that are all-zero (the CFG unconditional half: their cross-attention is skipped) */
int pcdm_unet_prepare_conditioning(pcdm_unet* u, int B, int h, int w, int L, const float* ehs, const float* class_labels, const float* pose, int pose_b,
                                   int zero_ctx_batches, void* workspace, pcdm_stream_t s);
/* Optional, after pcdm_unet_prepare_conditioning on the same workspace: the caller guarantees that batch entries b and b + B/2 always carry the
 * same x_in rows and pose feature (the two classifier-free-guidance halves: stage2_inpaint_pipeline.py:499-501 doubles the latents and shares
 * mask / masked latents / pose): conv_in, the first norm1 and the first conv1's contraction then run once for both halves. */
int pcdm_unet_set_shared_cfg_input(pcdm_unet* u, void* workspace, int shared);
/* Optional, after pcdm_unet_prepare_conditioning on the same workspace: the time / class embedding MLPs (ref :661-708) and every
 * ResnetBlock2D.time_emb_proj for ALL n timesteps of t_dev, once per sampling call (2 + 2 ceil(n / 32) + 2 launches) instead of five launches
 * per denoise step.  table: caller-owned device memory of pcdm_unet_time_table_bytes(u, n, B) bytes, alive while forwards use it.
 * pcdm_unet_forward calls on this workspace that pass the same t_dev and a device step counter pick their block by that counter; any other
 * call computes the embeddings per step as before.  Bit-identical to the per-step launches.  The table is keyed on the POINTER t_dev: a host
 * that rewrites the timestep buffer in place (another schedule or step count) must call pcdm_unet_prepare_timesteps again before the
 * next forward (not checkable at launch: it lives in device memory).  The device step counter must stay below n: ABI 6 bounds it on the
 * device (clamped into the table, error flag: pcdm_unet_step_overflow). */
int64_t pcdm_unet_time_table_bytes(const pcdm_unet* u, int n, int B);
int pcdm_unet_prepare_timesteps(pcdm_unet* u, const int64_t* t_dev, int n, void* table, void* workspace, pcdm_stream_t s);
/* The float32-timestep forms of pcdm_unet_prepare_timesteps / pcdm_unet_forward (t_dev is a float table: fractional timesteps); everything
 * else as the int64 forms, and the same bits for integer-valued floats. */
int pcdm_unet_prepare_timesteps_f32(pcdm_unet* u, const float* t_dev, int n, void* table, void* workspace, pcdm_stream_t s);
/* x_in NHWC bf16 [B, h, w, conv_in.cin] (pcdm_assemble_input / pcdm_nchw_f32_to_nhwc_bf16); timestep = t_dev[step_dev ? *step_dev : 0] (device);
 * pose_b as passed to prepare_conditioning (0: no pose); eps_out fp32 NCHW [B, out_channels, h, w].
 * KNOWN REMAINDER of the ABI 6 bound: these two calls take no length for t_dev.  With step_dev NULL they read t_dev[0] (length 1); with the
 * t_dev of pcdm_unet_prepare_timesteps the counter is bounded into that table's n rows (pcdm_unet_step_overflow).  With a device counter but
 * WITHOUT a table prepared for this t_dev the length is unknown to the library: *step_dev < length of t_dev stays the caller's contract (a
 * negative counter reads row 0, no flag). */
int pcdm_unet_forward(pcdm_unet* u, const void* x_in, const int64_t* t_dev, const int32_t* step_dev, int B, int h, int w, int L, int pose_b,
                      void* workspace, float* eps_out, pcdm_stream_t s);
int pcdm_unet_forward_f32(pcdm_unet* u, const void* x_in, const float* t_dev, const int32_t* step_dev, int B, int h, int w, int L, int pose_b,
                          void* workspace, float* eps_out, pcdm_stream_t s);
/* Did a pcdm_unet_forward on this workspace ever find *step_dev outside the time table of pcdm_unet_prepare_timesteps (>= n or negative)?  Such a
 * forward does NOT read out of bounds -- every consumer of the table clamps the step on the device -- but its time embedding is that of the
 * last table row: *flag_out = 1 then (and stays 1 until pcdm_unet_workspace_init / pcdm_unet_prepare_timesteps clear it).  Synchronises s. */
int pcdm_unet_step_overflow(pcdm_unet* u, void* workspace, int* flag_out, pcdm_stream_t s);
/* Host-side weight packing (plain loops on HOST memory; upload the result): the layouts pcdm_gemm / pcdm_unet_set_weight expect, from the
 * fp32 tensors of a diffusers state dict.  Each returns Npad (< 0: bad arguments); output pointers may be NULL to query sizes.
 *   pcdm_pack_linear : [N, K] -> bf16 [Npad, K], bias -> fp32 [Npad]                       (Npad = N rounded up to pad_to, normally 64)
 *   pcdm_pack_conv3x3: [N, Cin, 3, 3] -> bf16 [Npad, 9 Cp], k = (ky 3 + kx) Cp + c          (Cp = Cin rounded up to 64; *K_out = 9 Cp, *cin_out = Cp)
 *   pcdm_pack_geglu  : [2 D, K] rows [h | gate] -> bf16 [2 Dp, K], rows per 64 = [32 h | 32 gate], bias likewise (GEMM N = D, Npad = 2 Dp) */
int pcdm_pack_linear(const float* w, const float* bias, int N, int K, int pad_to, uint16_t* out_w, float* out_bias);
int pcdm_pack_conv3x3(const float* w, const float* bias, int N, int Cin, int pad_to, uint16_t* out_w, float* out_bias, int* K_out, int* cin_out);
int pcdm_pack_geglu(const float* w, const float* bias, int D, int K, uint16_t* out_w, float* out_bias);

/* ---- Test / debug hooks for workspace containment (tests/test_workspace_containment.py).  Not for product code; both the product library and
 * the lane-emulator build export them.
 *
 * Red zone: a process-wide byte count (default 0; a non-negative multiple of 256, anything else is refused with -1) that EVERY workspace layout
 * computed afterwards leaves unused behind each buffer it carves out of a caller-owned workspace -- the five sub-allocators: the plan of
 * pcdm_unet_*, and the layouts of pcdm_dwpose_forward, pcdm_detect_forward, pcdm_lpips and pcdm_inception_features.  The matching
 * pcdm_unet_workspace_bytes / *_ws_bytes count those bytes; the cached UNet plan is keyed on the value, so changing it re-plans (and moves every
 * buffer: conditionings prepared under another value are void).  With 0 every offset and every total is what it was without the hook.
 * Set it BEFORE a layout is computed (before the *_ws_bytes query whose workspace a call will run on), keep it unchanged across all calls on that
 * workspace, and RESTORE it (0) afterwards: it is not thread-safe and nothing resets it.  A test fills the zones with a byte pattern, runs the
 * calls, and requires the pattern to be intact: a kernel that overruns its buffer by a padded row or a full-line store then shows, instead of
 * landing silently in the next buffer of the same workspace.
 *
 * Layout enumerators: one per sub-allocator, with the arguments of its *_ws_bytes plus an index.  Each returns the NUMBER of entries (>= 1) and,
 * for 0 <= index < that number, writes the buffer's name (a string owned by the library; for the UNet valid until the context re-plans or is
 * destroyed), its byte offset in the workspace and its byte count WITHOUT the red zone (the red zone, if any, follows at offset + bytes).
 * index = -1 only counts (the three output pointers may then be NULL; NULL outputs are skipped for any index).  Returns -1 for arguments the
 * matching *_ws_bytes refuses and for any other index.  Entries come in offset order; pcdm_unet_workspace_layout reports the live regions of
 * the context's plan for that shape (and, like pcdm_unet_workspace_bytes, makes it the current plan). */
int pcdm_set_workspace_redzone(int64_t bytes);
int64_t pcdm_get_workspace_redzone(void);
int pcdm_unet_workspace_layout(pcdm_unet* u, int B, int h, int w, int L, int index, const char** name, int64_t* offset, int64_t* bytes);
int pcdm_dwpose_ws_layout(const pcdm_dwpose_config* cfg, int R, int flip, int index, const char** name, int64_t* offset, int64_t* bytes);
int pcdm_detect_ws_layout(const pcdm_detect_config* cfg, int N, int index, const char** name, int64_t* offset, int64_t* bytes);
int pcdm_lpips_ws_layout(int N, int ref_n, int H, int W, int index, const char** name, int64_t* offset, int64_t* bytes);
int pcdm_inception_ws_layout(int B, int H, int W, int dims, int index, const char** name, int64_t* offset, int64_t* bytes);

#ifdef __cplusplus
}
#endif
#endif
