/*
 * mxa.h -- C ABI of the MI355X-native MX top-k attention library (libmxa.so).
 *
 * Plain pointers, sizes and a hipStream_t; no torch types.  Every device
 * pointer is a gfx950 device allocation; every call is asynchronous on
 * `stream` and returns an MXA_* status (0 = OK, < 0 = error, nothing launched).
 * No global state: calls are reentrant; one call per stream at a time.
 *
 * Each entry point names the reference interface it replaces.  Reference
 * paths are relative to d9bjo0522/mx_quantization (snapshot 2025-12-12).
 * The reference's own native boundary is the pybind module
 * microxscaling/mx/cpp/funcs.cpp:234-242 (7 functions), JIT-built by
 * microxscaling/mx/custom_extensions.py:11-19; its Python fallbacks in
 * mx_ops.py / elemwise_ops.py are what the workloads actually run.
 */
#ifndef MXA_H_
#define MXA_H_

#include <stdint.h>
#include <hip/hip_runtime_api.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MXA_ABI_VERSION 6  /* 6: mxa_matmul_bt */

/* status codes */
#define MXA_OK 0
#define MXA_ERR_ARG (-1)          /* bad shape / pointer / option */
#define MXA_ERR_UNSUPPORTED (-2)  /* valid for the reference, not implemented here */
#define MXA_ERR_LAUNCH (-3)       /* HIP launch error */
#define MXA_ERR_WORKSPACE (-4)    /* workspace too small */

/* storage dtypes of tensor arguments.  The reference's ops follow their input's dtype
 * (microxscaling/mx/mx_ops.py:85, :283; elemwise_ops.py:146): on float16 / bfloat16
 * tensors the shared exponent is floor(log2) computed in that dtype, a float16 all-zero
 * block quantizes to NaN (2^-126 underflows: log2(0) = -inf, scale 2^-127 = 0, 0/0; with
 * scale_bits <= 5 the clamped scale 2^-15 is a float16 and the block stays 0), so does a
 * float16 block whose maximum is one of the top five codes 0x7bfb .. 0x7bff (floor(log2)
 * computed in float16 is 16 there and the scale 2^16 is inf), x / 2^e that falls below the
 * dtype's normals is rounded to the dtype (a negative x that underflows gives +0.0), and
 * every op's result is a tensor of that dtype. */
#define MXA_DT_F32 0
#define MXA_DT_F16 1
#define MXA_DT_BF16 2

/* rounding modes: microxscaling/mx/formats.py:12-16 (RoundingMode) */
#define MXA_ROUND_NEAREST 0
#define MXA_ROUND_FLOOR 1
#define MXA_ROUND_EVEN 2

/* approximator kinds, per operand side.
 * funcs/exponent_based_prediction.py:44-318 and
 * microxscaling/examples/deit/exponent_based_prediction.py:135-178 */
#define MXA_OP_SIGN 0     /* exp-sign:  (mx<0 ? -1 : +1) * 2^e_block        (ex_pred, partial_*) */
#define MXA_OP_MXINT8 1   /* MXINT8 values                                    (partial_* MX side) */
#define MXA_OP_MXINT4 2   /* MXINT4 values (Sanger)                           (MXINT4)            */
#define MXA_OP_EXION 3    /* two_step_leading_ones incl. its e*(...) quirk    (EXION)             */
#define MXA_OP_TRUE_EX 4  /* exponent_based_sign_leading_ones (values only)   (true_ex)           */

/* prediction modes of the fused op (the caller's `pred_mode`) */
#define MXA_PRED_EX_PRED 0
#define MXA_PRED_PARTIAL_Q 1
#define MXA_PRED_PARTIAL_K 2
#define MXA_PRED_MXINT4 3
#define MXA_PRED_EXION 4
#define MXA_PRED_TRUE_EX 5  /* exponent_based_sign_leading_ones (PixArt MX_transformer_block.py:663-664)   */
#define MXA_PRED_ELSA 6     /* elsa_approximation.approximation_scores (funcs/elsa_approximation.py:115-143);
                               self-attention only (N == T): the reference scales row n by the norm of
                               key row n (:126, :142-143), which broadcasts only when N == T         */

int mxa_abi_version(void);
const char* mxa_status_string(int status);

/*
 * MX block quantization of a contiguous tensor viewed as (outer, axis_len, inner),
 * blocks of `block_size` along the middle axis (0 = whole axis), integer element
 * formats with elem_mbits in {8, 4, 2} (int8 / int4 / int2).
 * Replaces quantize_mx_op -> _quantize_mx (microxscaling/mx/mx_ops.py:180-341)
 * and the reference's native quantize_mx_func_cpp / quantize_mx_by_tile_func_cuda
 * (microxscaling/mx/cpp/funcs.cpp:23-98, :177-231; mx.cu:116-287).
 *   y      : dequantized values, same layout as x (required)
 *   codes  : element codes, same layout as x (nullable)
 *   exps   : block scale exponents (outer, nblocks, inner), INT16_MIN = NaN (nullable)
 *   bfloat : elementwise pre-rounding of x (0/32 = none, 16 = bfloat16; quantize_elemwise_op)
 *   dtype  : MXA_DT_* of x and y
 */
int mxa_quantize_mx(const void* x, void* y, int8_t* codes, int16_t* exps,
                    int64_t outer, int64_t axis_len, int64_t inner, int32_t block_size,
                    int32_t elem_mbits, int32_t scale_bits, int32_t round_mode,
                    int32_t flush_subnormals, int32_t bfloat, int32_t dtype, hipStream_t stream);

/*
 * Shared exponents of the blocks of a (outer, axis_len, inner) tensor.
 * Replaces _shared_exponents (microxscaling/mx/mx_ops.py:49-99).
 *   method 0 = "max" -> out (outer, nblocks, inner); 1 = "none" -> out like x.
 *   ebits > 0 applies the [-emax, emax] / NaN clamp of :90-97.  x and out: dtype (MXA_DT_*).
 */
int mxa_shared_exponents(const void* x, void* out, int64_t outer, int64_t axis_len, int64_t inner,
                         int32_t block_size, int32_t method, int32_t ebits, int32_t dtype, hipStream_t stream);

/*
 * Elementwise bfloatX quantization.  Replaces quantize_elemwise_op / _quantize_bfloat
 * (microxscaling/mx/elemwise_ops.py:201-277) and quantize_elemwise_func_cuda
 * (microxscaling/mx/cpp/elemwise.cu:12-95).  bfloat 10..31 (0 / 32: identity), any
 * MXA_ROUND_*, allow_denorm 0 / 1.  As in the reference's Python path the result is NaN where
 * floor(log2|x|), computed in the tensor's dtype, is above the dtype's largest exponent --
 * the top codes of the top binade, both signs: float32 0x7f7fffd4 .. 0x7f7fffff (FLT_MAX
 * among them), bfloat16 0x7f58 .. 0x7f7f, float16 0x7bfb .. 0x7bff (2^pe is inf, x / inf = 0,
 * 0 * inf = NaN).  The same holds wherever a `bfloat` argument rounds operands or results.
 */
int mxa_quantize_bfloat(const void* x, void* y, int64_t n, int32_t bfloat, int32_t round_mode,
                        int32_t allow_denorm, int32_t dtype, hipStream_t stream);

/*
 * Approximator operand values along the last axis (rows x d, leading dims ld_x / ld_out),
 * MX block size 32.  Replaces the tensors returned by exponent_approximation's methods
 * (funcs/exponent_based_prediction.py:44-318): op_kind MXA_OP_*.  x and out: dtype.
 */
int mxa_approx_values(const void* x, void* out, int64_t rows, int32_t d, int64_t ld_x,
                      int64_t ld_out, int32_t op_kind, int32_t flush_subnormals, int32_t bfloat,
                      int32_t dtype, hipStream_t stream);
/*
 * The same with the element width of the MX codes the operands are derived from: elem_bits 8 is
 * mxa_approx_values; 4: every op_kind from MXINT4 codes (exponent_approximation at a_elem_format
 * "int4": MXA_OP_SIGN, MXA_OP_EXION and MXA_OP_TRUE_EX of the MXINT4 tensor, MXA_OP_MXINT8 and
 * MXA_OP_MXINT4 both that tensor); any other width: MXA_ERR_ARG.
 */
int mxa_approx_values_bits(const void* x, void* out, int64_t rows, int32_t d, int64_t ld_x,
                           int64_t ld_out, int32_t op_kind, int32_t flush_subnormals, int32_t bfloat,
                           int32_t dtype, int32_t elem_bits, hipStream_t stream);

/*
 * torch.topk(vals, k, dim=-1, largest=True, sorted=True) with torch's CPU index
 * order (aten TopKImpl.h:45-86 -> libstdc++ nth_element + sort / partial_sort),
 * as called at workloads/deit/scripts/main.py:123, workloads/DiT/models.py:194,
 * workloads/PixArt/models/MX_transformer_block.py:678, :825.
 * rows x n with leading dim ld; n <= 1024 (PixArt 512x512 self-attention rows:
 * MX_transformer_block.py:648-717, 1,024 tokens).  out_vals nullable.
 * out_mask (nullable): the prune mask zeros.scatter_(-1, idx, 1) of the callers
 * (deit main.py:147-148; examples/deit/top_k.py:16-42) as rows x ceil(n/32)
 * words, bit j%32 of word j/32 set iff j is kept.  vals / out_vals: dtype (MXA_DT_*).
 */
int mxa_topk(const void* vals, int64_t rows, int32_t n, int64_t ld, int32_t k,
             int64_t* out_idx, void* out_vals, uint32_t* out_mask, int32_t dtype, hipStream_t stream);

/*
 * mxa_topk with a device workspace (the same results): rows of <= 256 values go through
 * the packed 32-bit selection pass and the one-lane tail (the fused op's selection
 * engine), which stage per-row state in the workspace.  mxa_topk_workspace_bytes:
 * the bytes it needs (0: no workspace path for this shape -- mxa_topk_ws then runs
 * mxa_topk; -1: invalid arguments).  workspace: 16-B aligned device memory.
 */
int64_t mxa_topk_workspace_bytes(int64_t rows, int32_t n, int32_t k);
int mxa_topk_ws(const void* vals, int64_t rows, int32_t n, int64_t ld, int32_t k,
                int64_t* out_idx, void* out_vals, uint32_t* out_mask, int32_t dtype,
                void* workspace, int64_t workspace_bytes, hipStream_t stream);

/*
 * The fused hot path: MXINT8 true scores, approximate scores, top-k prune,
 * softmax over the kept scores, MXINT8 P.V -- the mx_quant branch of
 *   QuantizedAttention.forward  workloads/deit/scripts/main.py:100-152
 *   Attention.forward           workloads/DiT/models.py:168-225
 *   MXSelfAttention.forward     workloads/PixArt/models/MX_transformer_block.py:648-717
 *   MXCrossAttention.forward    workloads/PixArt/models/MX_transformer_block.py:792-859
 * from q (B,H,N,D), k/v (B,H,T,D) to the pre-projection output (B,H,N,D).
 * Strides are in elements for the (b,h,row) dims; the D dim must be contiguous.
 */
typedef struct mxa_attn_params {
  const void* q;           /* dtype `dtype`                                                 */
  const void* k;
  const void* v;
  int64_t q_strides[3];
  int64_t k_strides[3];
  int64_t v_strides[3];
  int32_t B, H, N, T, D;
  int32_t k_top;           /* kept keys per query row (top_k != 0)                         */
  float scale;             /* float32(head_dim ** -0.5) as the caller computes it          */
  int32_t pred_mode;       /* MXA_PRED_*                                                   */
  int32_t top_k;           /* 0: dense softmax (blocks excluded from top-k)                */
  int32_t approx;          /* 0: top-k on the true scores (approx_flag / ex_pred False)    */
  int32_t flush_subnormals;/* mx_specs["mx_flush_fp32_subnorms"]                           */
  int32_t bfloat;          /* mx_specs["bfloat"]: 0/32 none, 16 bfloat16                   */
  const void* bias;        /* additive score bias (PixArt mask), dtype `dtype`, nullable   */
  int64_t bias_strides[4]; /* (b,h,n,t) strides in elements of `dtype`, 0 = broadcast: any
                              non-negative values (the t stride too: a transposed or
                              every-second-element view is read in place); no alignment
                              beyond the element's is required                             */
  void* out;               /* (B,H,N,D) output, dtype: score_dtype ? score_dtype : dtype   */
  int64_t out_strides[3];  /* (b,h,n) strides in elements of out's dtype, the D axis
                              contiguous: any non-negative values that keep the B*H*N rows
                              apart ((B,N,H*D): {N*H*D, D, H*D}); no alignment beyond the
                              element's.  The kernels store exactly the D elements of each
                              row and nothing else; that out holds them is the caller's to
                              check (M.mx_topk_attention checks shape, dtype and device)   */
  int64_t* idx_out;        /* (B,H,N,k_top) contiguous int64, nullable                     */
  float* true_out;         /* optional (B,H,N,T) contiguous true scores (tests)            */
  float* pred_out;         /* optional (B,H,N,T) contiguous approximate scores            */
  uint32_t* mask_out;      /* optional prune mask (B,H,N,ceil(T/32)) words: bit t%32 of word
                              t/32 set iff key t is kept (zeros.scatter_(-1, idx, 1))      */
  const float* elsa_proj;  /* MXA_PRED_ELSA: (D,D) row-major orthogonal matrix P of the
                              caller; hash bit j = (MX(x) . P[j] >= 0)  (:105-112)           */
  const float* elsa_cos;   /* MXA_PRED_ELSA: (D+1) floats cos(clamp(pi/D*h - 0.127, 0)), the
                              caller's torch.cos values (:138-143); nullable: computed on the
                              device, correctly rounded                                    */
  void* workspace;         /* device scratch of mxa_attention_workspace_bytes() bytes     */
  int64_t workspace_bytes;
  int32_t dtype;           /* MXA_DT_* of q, k, v, bias: their MX quantization follows it   */
  int32_t score_dtype;     /* 0: the GEMM outputs (true / approximate scores, P, out) are in
                              `dtype` (the ops on tensors of that dtype); MXA_DT_F16 / BF16:
                              torch.autocast -- the fp32 q, k, v operands' matmuls return that
                              dtype, P = zeros_like(true scores) is of it and is quantized by its
                              rules (deit main.py:101, :118, :147; engine.py:97).  true_out /
                              pred_out hold those dtype values as float32.
                              With a bias (float32, as q is): `true_scores += bias` is in
                              place, true = score_dtype(true + bias); `pred = pred + bias` is
                              out of place and torch promotes it, pred = fl32(score_dtype(aQ
                              aK^T) + bias) with no second rounding: the ranking, and
                              pred_out, are of float32 values (MX_transformer_block.py:
                              821-822).  With 16-bit q, k, v and bias both sums stay in
                              `dtype`.                                                      */
} mxa_attn_params;

int64_t mxa_attention_workspace_bytes(const mxa_attn_params* p);
int mxa_attention(const mxa_attn_params* p, hipStream_t stream);

/*
 * The approximate scores alone: pred = aQ @ aK^T (+ bias) for p->pred_mode into
 * p->pred_out (required, (B,H,N,T) contiguous) -- what the callers compute from
 * exponent_approximation's operands (deit main.py:101-118, DiT models.py:176-190,
 * PixArt MX_transformer_block.py:658-677, :805-822) or ELSA's approximation_scores,
 * without the top-k, softmax or P.V.  v and out are ignored (may be null).
 */
int mxa_approx_scores(const mxa_attn_params* p, hipStream_t stream);

/*
 * mxa_attention / mxa_approx_scores / mxa_attention_workspace_bytes for rows of up to 1,024
 * keys: PixArt 512x512 self-attention, N = T = 1,024 tokens (MXSelfAttention.forward,
 * workloads/PixArt/models/MX_transformer_block.py:624-717).  The same parameter struct,
 * strides, outputs (out, idx_out, mask_out, true_out, pred_out) and workspace rules.  With
 * T <= 512 they run exactly what their short siblings run.  With 513 <= T <= 1,024: the top-k
 * path with 1 <= k_top <= 64, every pred_mode (ELSA with N == T), approx = 0, bias,
 * flush_subnormals and bfloat, on float32 tensors -- the selection runs one wave per query row
 * (the engine of mxa_topk's long rows) and the finishing kernel reads the kept keys from the
 * workspace.  MXA_ERR_UNSUPPORTED, before any HIP call, with T > 512 for: top_k == 0 (the dense
 * branch), k_top > 64, float16 / bfloat16 tensors or a nonzero autocast score_dtype, and
 * T > 1,024.  mxa_attention and the fused projections (mxa_qkv_attention, mxa_attention_proj,
 * mxa_cross_attention) keep their T <= 512 rule.
 */
int64_t mxa_attention_long_workspace_bytes(const mxa_attn_params* p);
int mxa_attention_long(const mxa_attn_params* p, hipStream_t stream);
int mxa_approx_scores_long(const mxa_attn_params* p, hipStream_t stream);

/*
 * The same three with the element width of the attention core as an argument (W4A4: the
 * reference's PixArt inference, workloads/PixArt/scripts/mx_inference.py:106-122, runs
 * MXSelfAttention / MXCrossAttention.forward, MX_transformer_block.py:648-717, :792-859, at
 * w_elem_format = a_elem_format = "int4").  The same parameter struct and workspace rules.
 *   elem_bits 8: exactly mxa_attention_long / mxa_approx_scores_long /
 *                mxa_attention_long_workspace_bytes -- the same kernels, bytes, statuses, size.
 *   elem_bits 4: Q and K (along D), P (along the keys) and V (along the tokens) are MXINT4 --
 *                codes in [-7, 7], one per byte, code unit 2^(es - 2) -- and every approximator
 *                is built from the MXINT4 MX_Q / MX_K, as exponent_approximation does at
 *                a_elem_format "int4" (funcs/exponent_based_prediction.py:18-31): a value that
 *                rounds to the int4 code 0 has the exp-sign "+", partial_*'s MX side is the
 *                MXINT4 tensor, EXION's integer is MX / 2^e * 64 of the int4 value.
 *                Float32 tensors; bfloat, flush_subnormals, bias, approx = 0, pred_mode ex_pred,
 *                partial_Q, partial_K, MXINT4, EXION and true_ex, every optional output, D <= 128;
 *                the top-k path with k_top <= 64 at T <= 1,024 (finish16_kernel, above 512 keys
 *                behind select_long_kernel), and k_top > 64 or the dense branch at T <= 256
 *                (finish_qk_kernel): PixArt's self-attention at 256 / 1,024 tokens, its 120-token
 *                cross-attention and the dense steps of exclude_timesteps.
 *                MXA_ERR_UNSUPPORTED, before any HIP call: MXA_PRED_ELSA (with approx), float16 /
 *                bfloat16 tensors or a nonzero score_dtype, k_top > 64 or the dense branch with
 *                T > 256 (finish_kernel, dense_rows_kernel), T > 1,024.
 *   any other width: -1 / MXA_ERR_ARG before any HIP call.
 * The fused projections at 4 bits (a W4A4 block in one call) are mxa_qkv_attention_bits,
 * mxa_attention_proj_bits and mxa_cross_attention_bits below; their siblings without _bits return
 * MXA_ERR_ARG for a 4-bit weight.
 */
int64_t mxa_attention_bits_workspace_bytes(const mxa_attn_params* p, int32_t elem_bits);
int mxa_attention_bits(const mxa_attn_params* p, int32_t elem_bits, hipStream_t stream);
int mxa_approx_scores_bits(const mxa_attn_params* p, int32_t elem_bits, hipStream_t stream);

/*
 * mxa_attention_bits with the whole of the 513 .. 1,024-key rows: the dense branch and every k_top.
 * The reference's MXSelfAttention.forward takes attn = softmax(true scores)
 * (workloads/PixArt/models/MX_transformer_block.py:704-705) when the model runs with
 * self_top_k=False, in the exclude_timesteps and in the exclude_blocks -- at 512 x 512 a dense
 * row of 1,024 keys -- and its self_k is a free parameter (the top-k branch, :700-702: gather,
 * softmax, scatter).  The same parameter struct, strides, outputs and workspace rules.
 *   - every call mxa_attention_bits(p, elem_bits) accepts runs exactly what that runs: the same
 *     kernels, bytes, statuses and workspace size;
 *   - with 513 <= T <= 1,024 also top_k == 0 and 65 <= k_top <= T, at elem_bits 8 and 4, on
 *     finish_qk_long_kernel: every key's score and P.V on v_mfma_i32_16x16x32_i8, three passes
 *     over the key blocks (maximum, sum, codes and P.V) with the arithmetic of finish_qk_kernel;
 *     the top-k case behind select_long_kernel, whose prune-mask words it reads (a workspace
 *     region when the caller takes no mask_out: the size does not depend on mask_out).
 * MXA_ERR_UNSUPPORTED, before any HIP call: T > 1,024; with T > 512 float16 / bfloat16 tensors
 * or a nonzero score_dtype; at elem_bits 4 what mxa_attention_bits refuses at T <= 512, and
 * MXA_PRED_ELSA (with approx).  Any other width: -1 / MXA_ERR_ARG.  The fused projections keep
 * their T <= 512 rule.  mxa_attention_full_finish_kernel: the MXA_FIN_* kind of the call
 * (no launch; the workspace may be null), as mxa_attention_finish_kernel for mxa_attention.
 */
int64_t mxa_attention_full_workspace_bytes(const mxa_attn_params* p, int32_t elem_bits);
int mxa_attention_full(const mxa_attn_params* p, int32_t elem_bits, hipStream_t stream);
int mxa_attention_full_finish_kernel(const mxa_attn_params* p, int32_t elem_bits);

/*
 * Which kernels mxa_attention(p) runs (no launch; the workspace may be null):
 *   MXA_PATH_ROWS_SPLIT  selection kernel (scores + top-k) then finishing kernel
 *                        (gather, softmax, MX(P), P.V on int8 MFMA) -- top_k != 0
 *   MXA_PATH_ROWS_FUSED  one row kernel for all of it -- the dense branch (top_k == 0)
 * or a negative MXA_ERR_* for invalid parameters.
 */
#define MXA_PATH_ROWS_FUSED 2
#define MXA_PATH_ROWS_SPLIT 3
int mxa_attention_path(const mxa_attn_params* p);

/*
 * Which finishing kernel mxa_attention(p) runs, and so on which engines its two dense
 * contractions (QK^T, P.V: microxscaling/mx/matmul.py:68-76, :85-88 as the callers use them,
 * workloads/deit/scripts/main.py:124-152, workloads/DiT/models.py:194-225) run (no launch):
 *   MXA_FIN_GATHER16    finish16_kernel: kept-key QK^T on v_dot4, P.V on v_mfma_i32_16x16x32_i8
 *   MXA_FIN_GATHER32    finish_kernel: kept-key QK^T on v_dot4, P.V on v_mfma_i32_32x32x32_i8
 *   MXA_FIN_MFMA        finish_qk_kernel: every key's QK^T and P.V on v_mfma_i32_16x16x32_i8
 *                       (the prune mask applied in the softmax)
 *   MXA_FIN_DENSE_MFMA  the dense branch (top_k == 0) on finish_qk_kernel, every key kept
 *   MXA_FIN_DENSE_ROWS  the dense branch on dense_rows_kernel (T > 256): v_dot4 for both
 * and, reported by mxa_attention_full_finish_kernel for mxa_attention_full alone:
 *   MXA_FIN_MFMA_LONG        finish_qk_long_kernel: top-k with k >= 65 on rows over 512 keys
 *   MXA_FIN_DENSE_MFMA_LONG  finish_qk_long_kernel: top_k == 0 on rows over 512 keys
 * or a negative MXA_ERR_* for invalid parameters.
 */
#define MXA_FIN_GATHER16 1
#define MXA_FIN_GATHER32 2
#define MXA_FIN_MFMA 3
#define MXA_FIN_DENSE_MFMA 4
#define MXA_FIN_DENSE_ROWS 5
#define MXA_FIN_MFMA_LONG 6
#define MXA_FIN_DENSE_MFMA_LONG 7
int mxa_attention_finish_kernel(const mxa_attn_params* p);

/*
 * Measurement entry point (bench.py): runs mxa_attention `iters` times on `stream`
 * recording HIP events between the kernels, synchronizes the stream, and writes
 * the mean milliseconds of each stage to stage_ms[MXA_ATTN_STAGES]:
 *   0 the operand builders (for mxa_qkv_attention_timed the x quantization + projection).  A
 *   call that forks (below): slot 0 then covers the critical builder only -- Q's and K's rows --
 *   and V's columns are built on the library's stream during slot 3
 *   1, 2 empty  3 scores+top-k, to the join (on MXA_PATH_ROWS_FUSED: 0)
 *   4 gather+softmax+P+P.V (on MXA_PATH_ROWS_FUSED: the dense row kernel)
 * Host-synchronizing: not for use inside graph capture.
 *
 * Streams.  Every entry point enqueues on `stream` and the caller sees one ordered stream: what
 * was enqueued on it before the call happens before the call's first read or write, and what is
 * enqueued after the call sees all of its results.  Inside, a top-k call of mxa_attention and its
 * _long / _bits / _full siblings on q, k, v whose selection runs the one-lane tail (T <= 256, no
 * bias, an approximator whose scores pack, k_top + 2 <= 48) builds V's table, which only its
 * finishing kernel reads, on one stream of the library's own per device, created on the first
 * such call and kept: forked behind the selection kernel, beside the tail, and joined before the
 * finishing kernel, both with events.  It therefore reads v and writes the workspace from that
 * stream too, between those two points.  While `stream` is capturing a graph
 * (hipStreamIsCapturing) the call keeps everything on `stream`.
 */
#define MXA_ATTN_STAGES 5
#define MXA_ATTN_STAGES_PLUS1 6
int mxa_attention_timed(const mxa_attn_params* p, hipStream_t stream, int32_t iters, float* stage_ms);

/*
 * The fused MX Linear qkv projection in front of the attention core: the patched
 * modules' `qkv = self.qkv(x).reshape(B, N, 3, H, D)` (workloads/deit/scripts/main.py:87-88,
 * workloads/DiT/models.py:156-157) with self.qkv an mx.Linear (microxscaling/mx/linear.py:
 * 20-103: out = bf(fl32(MX(bf(x)) @ MX(bf(W))^T)); out = bf(out + bf(bias))), feeding the
 * attention's MX operands directly -- the fp32 q / k / v never reach HBM.
 *
 * mxa_linear_weight_prep: W (out_features, in_features) fp32 row-major -> MXINT8 codes +
 * block exponents along in_features into `wq` (mxa_linear_weight_bytes bytes, 16-B
 * aligned; once per weight), laid out MFMA-ready in column groups of group_width
 * (the qkv projection: out_features = 3 * H * D, group_width = D -- one head's q, k or v).
 * The buffer starts with a header recording out_features, in_features, group_width,
 * flush_subnormals and bfloat; mxa_qkv_attention returns MXA_ERR_ARG for a buffer whose
 * header does not match (3*H*D, C, D, p->flush_subnormals, p->bfloat).  A buffer prepared
 * in another process (or copied) has its header read once, synchronously -- so not
 * inside a stream capture: call once before capturing.
 *
 * mxa_qkv_attention: mxa_attention with q, k, v produced from x (p->q, p->k, p->v are
 * ignored; self-attention, p->N == p->T; p->bias is the additive score bias, float32, as in
 * mxa_attention -- M.mx_qkv_attention's attn_bias).  The projection is exact-then-rounded (the
 * reference's fp32 GEMM order is unpinned: equal within fp32 rounding).
 */
typedef struct mxa_qkv_params {
  const float* x;        /* (B*N, C) tokens, row stride x_row_stride (elements)            */
  int64_t x_row_stride;
  int32_t C;             /* in_features                                                     */
  const void* wq;        /* mxa_linear_weight_prep output for W (3*H*D, C), group_width D    */
  const float* bias;     /* (3*H*D) or null                                                 */
  float* qkv_out;        /* optional (B*N, 3*H*D) fp32 projection (tests)                   */
  int32_t autocast_dtype;/* 0, or MXA_DT_F16 / BF16: torch.autocast's F.linear -- the product
                            rounded to that dtype, then + bias in fp32 (linear.py:88-101 under
                            autocast: the fp16 output + fp32 bias promotes to fp32)         */
} mxa_qkv_params;

int64_t mxa_linear_weight_bytes(int32_t out_features, int32_t in_features, int32_t group_width);
int mxa_linear_weight_prep(const float* w, int32_t out_features, int32_t in_features, int32_t group_width,
                           int32_t flush_subnormals, int32_t bfloat, void* wq, hipStream_t stream);
/*
 * The same with the element width as an argument: elem_bits 8 is mxa_linear_weight_bytes /
 * mxa_linear_weight_prep exactly (the same bytes, the same size); elem_bits 4 prepares MXINT4
 * (the reference's w_elem_format "int4": codes in [-7, 7], one exponent-folded digit plane --
 * a smaller buffer, its header marked 4 bits); any other width: -1 / MXA_ERR_ARG before any
 * HIP call.  mxa_linear and mxa_mlp take the width from the weight's header and quantize their
 * activations at the same width (W4A4); the attention entry points (mxa_qkv_attention,
 * mxa_attention_proj, mxa_cross_attention) return MXA_ERR_ARG for a 4-bit weight: a W4A4 block
 * goes through their *_bits forms (below, after mxa_cross_attention).
 */
int64_t mxa_linear_weight_bytes_bits(int32_t out_features, int32_t in_features, int32_t group_width,
                                     int32_t elem_bits);
int mxa_linear_weight_prep_bits(const float* w, int32_t out_features, int32_t in_features, int32_t group_width,
                                int32_t flush_subnormals, int32_t bfloat, int32_t elem_bits, void* wq,
                                hipStream_t stream);
int64_t mxa_qkv_attention_workspace_bytes(const mxa_attn_params* p, const mxa_qkv_params* x);
int mxa_qkv_attention(const mxa_attn_params* p, const mxa_qkv_params* x, hipStream_t stream);
/* mxa_attention_timed for the fused projection path (stage 0 = x quantize + projection) */
int mxa_qkv_attention_timed(const mxa_attn_params* p, const mxa_qkv_params* x, hipStream_t stream, int32_t iters,
                            float* stage_ms);

/*
 * mx.Linear forward (microxscaling/mx/linear.py:20-103) on a prepared weight:
 *   out = bf(fl32(MX(bf(x), along in_features) @ MX(bf(W), along in_features)^T));
 *   out = bf(out + bf(bias))          (bf = quantize_elemwise_op: bfloat rounding or none)
 * x (rows, in_features) fp32 at x_row_stride; wq from mxa_linear_weight_prep(W, out_features,
 * in_features, any group_width, flush_subnormals, bfloat) -- MXA_ERR_ARG if its header
 * differs -- or from mxa_linear_weight_prep_bits: MX is MXINT8, or MXINT4 for both operands
 * with a 4-bit weight (its header's width); out (rows, out_features) fp32 at out_row_stride.  Every product is the exact sum
 * rounded once (the reference's MKL sgemm order is unpinned: equal within fp32 rounding).
 * autocast_dtype: 0, or MXA_DT_F16 / BF16 (torch.autocast: the product rounded to that
 * dtype before the fp32 bias add).  The patched modules' proj Linear (deit main.py:154, DiT
 * models.py:227) and every Linear of the mx.Linear drop-in.
 */
int64_t mxa_linear_workspace_bytes(int64_t rows, int32_t in_features, int32_t out_features);
int mxa_linear(const float* x, int64_t rows, int32_t in_features, int64_t x_row_stride, const void* wq,
               int32_t out_features, const float* bias, float* out, int64_t out_row_stride,
               int32_t flush_subnormals, int32_t bfloat, int32_t autocast_dtype, void* workspace,
               int64_t workspace_bytes, hipStream_t stream);

/*
 * The MLP half of a block in one call: fc1 -> GELU -> fc2 with fc1 and fc2 mx.Linear
 * (microxscaling/mx/linear.py:20-103) and nn.GELU between them -- workloads/DiT/models.py:
 * 257-271 with act_layer = nn.GELU(approximate="tanh") at :286-287, timm's Mlp with nn.GELU
 * (workloads/deit/models_v2.py:55), PixArt's GELU(approximate="tanh") feed-forward
 * (MX_transformer_block.py:70-106); drop1, norm and drop2 are identities at inference:
 *   pre = mx.Linear(x; W1, b1)      exactly what mxa_linear computes
 *   act = gelu(pre)                 float32; MXA_ACT_GELU 0.5 h (1 + erf(h / sqrt 2)),
 *                                   MXA_ACT_GELU_TANH torch's tanh form
 *   y   = mx.Linear(act; W2, b2)    its input rule included: bf(act), MXINT8 blocks of 32
 *                                   (MXINT4 throughout when w1 and w2 are 4-bit weights;
 *                                   weights of different widths: MXA_ERR_ARG)
 * Float32, no autocast.  fc1's epilogue applies the GELU and writes fc2's MX input codes
 * itself, so the fp32 hidden matrix never reaches HBM; an fc1 that does not run on that
 * kernel (w1 prepared in groups that are neither hidden_features nor a multiple of 32
 * columns, or in_features beyond 72 blocks of 32 -- 144 for 4-bit weights) goes through an fp32 workspace and the row
 * quantizer with the same GELU: the same bits.  A NaN in x gives NaN rows in pre, act and
 * y.  pre = +-inf is not pinned (torch's own CPU kernel returns NaN for gelu(+inf) in the erf
 * form).  w1 / w2: mxa_linear_weight_prep of W1 (hidden_features, in_features) / W2
 * (out_features, hidden_features), any group_width, with these flush_subnormals / bfloat --
 * MXA_ERR_ARG if a header differs.  pre_out / act_out: optional (rows, hidden_features)
 * contiguous fp32 copies of pre and act (tests).  mxa_mlp_workspace_bytes sizes for the path
 * the call takes, from w1's header when this process has seen it (prepared or verified
 * here; else, and for w1 == NULL, the larger fallback size, which serves both paths).
 */
#define MXA_ACT_GELU 0
#define MXA_ACT_GELU_TANH 1
int64_t mxa_mlp_workspace_bytes(int64_t rows, int32_t in_features, const void* w1, int32_t hidden_features,
                                int32_t out_features);
int mxa_mlp(const float* x, int64_t rows, int32_t in_features, int64_t x_row_stride, const void* w1,
            int32_t hidden_features, const float* b1, int32_t act, const void* w2, int32_t out_features,
            const float* b2, float* y, int64_t y_row_stride, float* pre_out, float* act_out,
            int32_t flush_subnormals, int32_t bfloat, void* workspace, int64_t workspace_bytes,
            hipStream_t stream);

/*
 * The attention core with the proj Linear fused behind it: the patched modules'
 *   x = attn_out.transpose(1, 2).reshape(B, N, C);  x = self.proj(x)
 * (workloads/deit/scripts/main.py:152-154, workloads/DiT/models.py:225-227; proj an
 * mx.Linear, microxscaling/mx/linear.py:20-103) after mxa_attention (xq == NULL) or
 * mxa_qkv_attention (xq != NULL).  With D % 32 == 0 (float32, no autocast) the finishing
 * kernel MX-quantizes each 32-column P.V tile straight into the proj's input codes -- the
 * fp32 attention output never reaches HBM; otherwise (a 32-element block of C spans two
 * heads) the output goes through a workspace copy and the row quantizer.  p->out is not
 * written (may be NULL); y (B*N, out_features) fp32 at y_row_stride.  Top-k path only.
 */
typedef struct mxa_proj_params {
  const void* wq;        /* mxa_linear_weight_prep output for W_proj (out_features, H*D)      */
  int32_t out_features;
  const float* bias;     /* (out_features) or null                                           */
  float* y;              /* (B*N, out_features) rows at y_row_stride                         */
  int64_t y_row_stride;
} mxa_proj_params;

int64_t mxa_attention_proj_workspace_bytes(const mxa_attn_params* p, const mxa_qkv_params* xq,
                                           const mxa_proj_params* pj);
int mxa_attention_proj(const mxa_attn_params* p, const mxa_qkv_params* xq, const mxa_proj_params* pj,
                       hipStream_t stream);
/* mxa_attention_timed for it: stage_ms[MXA_PROJ_STAGES] -- slots 0..4 as mxa_attention_timed
 * (slot 0 the x quantize + qkv projection when xq != NULL), slot 5 the proj Linear (with
 * the row quantizer when the output went through the workspace) */
#define MXA_PROJ_STAGES 6
int mxa_attention_proj_timed(const mxa_attn_params* p, const mxa_qkv_params* xq, const mxa_proj_params* pj,
                             hipStream_t stream, int32_t iters, float* stage_ms);

/*
 * Cross-attention with its q and kv Linears fused in front: PixArt's MXCrossAttention.forward
 * (workloads/PixArt/models/MX_transformer_block.py:765-860),
 *   q = to_q(x);  k = to_k(cond);  v = to_v(cond)          all mx.Linear (linear.py:20-103)
 * from two token sources -- x (B*N, C) image tokens, cond (B*T, C_kv) text tokens -- feeding
 * the attention's MX operands directly: the fp32 q, k, v never reach HBM.  p->q, p->k, p->v
 * are ignored; p->N and p->T are independent; p->bias is the additive mask (PixArt's
 * (B,1,1,T) attention_mask bias through zero strides), as in mxa_attention.  Float32, no
 * autocast: a nonzero p->score_dtype returns MXA_ERR_UNSUPPORTED.  wq_q / wq_kv are checked
 * against their headers, (H*D, C, D) and (2*H*D, C_kv, D) with p->flush_subnormals and
 * p->bfloat: MXA_ERR_ARG on a mismatch.  Every other mxa_attention rule applies (T <= 512,
 * D <= 128, ELSA needs N == T).
 * pj == NULL: p->out is written; top_k == 0 (the dense branch) is allowed.  pj != NULL: the
 * to_out[0] mx.Linear runs behind the attention exactly as in mxa_attention_proj (top-k only;
 * p->out is not written).  The workspace is the attention's plus the MX codes of x and cond,
 * plus mxa_attention_proj's regions with pj.
 */
typedef struct mxa_cross_params {
  const float* x;          /* (B*N, C) query tokens, row stride x_row_stride (elements)        */
  int64_t x_row_stride;
  int32_t C;
  const float* cond;       /* (B*T, C_kv) key / value tokens, row stride cond_row_stride       */
  int64_t cond_row_stride;
  int32_t C_kv;
  const void* wq_q;        /* mxa_linear_weight_prep of W_q (H*D, C), group_width D             */
  const void* wq_kv;       /* ... of cat(W_k, W_v) along out_features (2*H*D, C_kv), group_width D */
  const float* bias_q;     /* (H*D) or null                                                    */
  const float* bias_kv;    /* (2*H*D) or null                                                  */
  float* q_out;            /* optional (B*N, H*D) fp32 projection (tests)                      */
  float* kv_out;           /* optional (B*T, 2*H*D) fp32 projection (tests)                    */
} mxa_cross_params;

int64_t mxa_cross_attention_workspace_bytes(const mxa_attn_params* p, const mxa_cross_params* xc,
                                            const mxa_proj_params* pj);
int mxa_cross_attention(const mxa_attn_params* p, const mxa_cross_params* xc, const mxa_proj_params* pj,
                        hipStream_t stream);

/*
 * The three fused blocks with the element width as an argument: the W4A4 block in one call (the
 * reference's PixArt inference runs every Linear and both attentions at w_elem_format =
 * a_elem_format = "int4", workloads/PixArt/scripts/mx_inference.py:106-122).  The same parameter
 * structs, outputs and workspace rules as mxa_qkv_attention, mxa_attention_proj and
 * mxa_cross_attention.
 *   elem_bits 8: exactly the sibling without _bits -- the same kernels, bytes, statuses and
 *                workspace size, MXA_ERR_ARG for a 4-bit weight included.
 *   elem_bits 4: every weight of the call (qkv, or q and kv, and proj) is an
 *                mxa_linear_weight_prep_bits(.., 4) buffer with the header the sibling expects at
 *                elem_bits 4; an 8-bit weight, or widths mixed within one call: MXA_ERR_ARG.  x
 *                and cond are quantized at MXINT4 and every projection is mxa_linear's on the same
 *                4-bit weight bit for bit (the exact product rounded once, then the Linear output
 *                rule); the fp32 q, k, v never reach HBM: the projection kernel writes the
 *                operands mxa_attention_bits(p, 4) would build from them, and the attention is
 *                that call's on rows of at most 512 keys.  With pj the attention's fp32 output
 *                goes through a workspace copy and the MXINT4 row quantizer for every D (at 8 bits
 *                only for D % 32 != 0), then mxa_linear's kernel for the 4-bit proj weight.
 *                Float32, no autocast.  MXA_ERR_UNSUPPORTED, before any HIP call: a nonzero
 *                score_dtype or autocast_dtype, float16 / bfloat16 tensors, MXA_PRED_ELSA (with
 *                approx), T > 512, k_top > 64, the dense branch with 256 < T <= 512.
 *                The workspace: the 8-bit size without pj; with pj the 8-bit size plus, for
 *                D % 32 == 0, the 256-byte-aligned fp32 copy (B*N*H*D floats).
 *   any other width: -1 / MXA_ERR_ARG before any HIP call.
 * There are no timed variants at 4 bits.
 */
int64_t mxa_qkv_attention_bits_workspace_bytes(const mxa_attn_params* p, const mxa_qkv_params* x, int32_t elem_bits);
int mxa_qkv_attention_bits(const mxa_attn_params* p, const mxa_qkv_params* x, int32_t elem_bits, hipStream_t stream);
int64_t mxa_attention_proj_bits_workspace_bytes(const mxa_attn_params* p, const mxa_qkv_params* xq,
                                                const mxa_proj_params* pj, int32_t elem_bits);
int mxa_attention_proj_bits(const mxa_attn_params* p, const mxa_qkv_params* xq, const mxa_proj_params* pj,
                            int32_t elem_bits, hipStream_t stream);
int64_t mxa_cross_attention_bits_workspace_bytes(const mxa_attn_params* p, const mxa_cross_params* xc,
                                                 const mxa_proj_params* pj, int32_t elem_bits);
int mxa_cross_attention_bits(const mxa_attn_params* p, const mxa_cross_params* xc, const mxa_proj_params* pj,
                             int32_t elem_bits, hipStream_t stream);

/*
 * The self-attention block at 512 x 512: the fused qkv projection and the proj Linear on rows of
 * 513 .. 1,024 keys (PixArt's MXSelfAttention.forward, workloads/PixArt/models/MX_transformer_block.py:624-717,
 * at N = T = 1,024; DiT at 512 x 512; DeiT at 384 x 384, 577 tokens).  The parameter structs, outputs
 * and workspace rules of mxa_qkv_attention_bits and mxa_attention_proj_bits (xq may be NULL in the proj
 * form: q, k, v given).
 *   T <= 512: exactly the _bits sibling at the same elem_bits -- the same kernels, bytes, statuses
 *             and workspace size (at 4 bits the 32-row and dense-row kernel shapes stay refused).
 *   513 <= T <= 1,024, float32: the projection kernel of the sibling writes the operands
 *             mxa_attention_full(p, elem_bits) would build from q, k, v, and the attention is that
 *             call's: every k_top <= T, every pred_mode (MXA_PRED_ELSA at 8 bits only), approx == 0,
 *             bias, bfloat, flush_subnormals, the optional outputs, and (qkv form only) the dense
 *             branch.  The proj's input: at 8 bits with D % 32 == 0 and k_top <= 32 the 16-row
 *             finishing kernel writes the MX codes itself; every other call (D % 32 != 0,
 *             k_top > 32, 4 bits) goes through the fp32 workspace copy and the row quantizer -- the
 *             same y bit for bit.  The workspace holds that 256-byte-aligned copy (B*N*H*D floats)
 *             exactly when the codes are not written directly.
 *   Unchanged answers: pj with top_k == 0 and xq with N != T are MXA_ERR_ARG.  MXA_ERR_UNSUPPORTED,
 *             before any HIP call: T > 1,024, D > 128, float16 / bfloat16 tensors, a nonzero
 *             score_dtype or autocast_dtype on rows over 512 keys, MXA_PRED_ELSA (with approx) at
 *             4 bits.
 * mxa_qkv_attention, mxa_attention_proj, mxa_cross_attention and their _bits forms keep T <= 512;
 * cross-attention is not extended (its T is the condition length).
 */
int64_t mxa_qkv_attention_full_workspace_bytes(const mxa_attn_params* p, const mxa_qkv_params* x, int32_t elem_bits);
int mxa_qkv_attention_full(const mxa_attn_params* p, const mxa_qkv_params* x, int32_t elem_bits, hipStream_t stream);
int64_t mxa_attention_proj_full_workspace_bytes(const mxa_attn_params* p, const mxa_qkv_params* xq,
                                                const mxa_proj_params* pj, int32_t elem_bits);
int mxa_attention_proj_full(const mxa_attn_params* p, const mxa_qkv_params* xq, const mxa_proj_params* pj,
                            int32_t elem_bits, hipStream_t stream);

/*
 * mx.matmul forward (microxscaling/mx/matmul.py:31-100, :211-222): in1 (batch, M, K)
 * quantized along K, in2 (batch, K, Nc) quantized along K, fp32 result (batch, M, Nc)
 * contiguous.  Integer formats, block size 32.  a_dtype / b_dtype (MXA_DT_*): each operand's
 * MX quantization follows its dtype; c is the exact product rounded once to c_dtype (the
 * operands' dtype, or torch.autocast's: P (float16) @ V (float32) under autocast, deit
 * main.py:152 with engine.py:97).
 */
int mxa_matmul(const void* a, const void* b, void* c, int64_t batch, int32_t M, int32_t K,
               int32_t Nc, int64_t a_batch_stride, int64_t b_batch_stride, int32_t elem_mbits_a,
               int32_t elem_mbits_b, int32_t flush_subnormals, int32_t bfloat, int32_t a_dtype,
               int32_t b_dtype, int32_t c_dtype, void* workspace, int64_t workspace_bytes, hipStream_t stream);
int64_t mxa_matmul_workspace_bytes(int64_t batch, int32_t M, int32_t K, int32_t Nc);
/* mxa_matmul with in2 given transposed: bt (batch, Nc, K) row-major, i.e. in2 = bt^T (the
 * k.transpose(-2, -1) view of deit main.py:101, DiT models.py:169), quantized along K as in
 * mxa_matmul -- no copy of the transposed operand.  Same workspace (mxa_matmul_workspace_bytes). */
int mxa_matmul_bt(const void* a, const void* bt, void* c, int64_t batch, int32_t M, int32_t K,
                  int32_t Nc, int64_t a_batch_stride, int64_t bt_batch_stride, int32_t elem_mbits_a,
                  int32_t elem_mbits_b, int32_t flush_subnormals, int32_t bfloat, int32_t a_dtype,
                  int32_t b_dtype, int32_t c_dtype, void* workspace, int64_t workspace_bytes, hipStream_t stream);

/* Self-tests of the int8 MFMA operand/accumulator lane maps the kernels rely on:
 * C = A * B computed by one MFMA, row-major int8 operands, int32 result; the host
 * compares.  mxa_selftest_mfma: v_mfma_i32_16x16x32_i8 (A 16x32, B 32x16; mx.matmul);
 * mxa_selftest_mfma32: v_mfma_i32_32x32x32_i8 (A 32x32, B 32x32; the finishing
 * kernel's P.V). */
int mxa_selftest_mfma(const int8_t* a, const int8_t* b, int32_t* c, hipStream_t stream);
int mxa_selftest_mfma32(const int8_t* a, const int8_t* b, int32_t* c, hipStream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* MXA_H_ */
