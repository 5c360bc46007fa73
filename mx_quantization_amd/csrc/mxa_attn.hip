// The MX top-k attention hot path on gfx950, and the mx.matmul drop-in.
//
//   rows_prep(Q), rows_prep(K)  MXINT8 codes + block exponents + approximator operands
//                               (mxa_quant.hip)
//   cols_prep(V)                MXINT8 codes of V along tokens, stored [d][t]
//   select_kernel               approximate scores + torch-CPU-order top-k, four query
//                               rows per wave (mxa_select.hpp, mxa_topk_grp.hpp), the
//                               one-lane tail (mxa_tail.hpp)
//   select_long_kernel          rows of 513 .. 1,024 keys (mxa_attention_long): one wave per query
//                               row, the scores into the wave top-k's mirror (mxa_select_long.hpp);
//                               finish16_kernel then reads the kept keys from the workspace
//   finish16_kernel / finish_kernel / finish_qk_kernel
//                               the kept keys' true scores, softmax, MX(P), P.V on int8
//                               MFMA (mxa_finish16.hpp, mxa_finish.hpp, mxa_finish_qk.hpp)
//   dense (top_k=False)         finish_qk_kernel with every key kept (T <= 256), else
//                               dense_rows_kernel (mxa_rows2.hpp)
//   finish_qk_long_kernel       mxa_attention_full on rows of 513 .. 1,024 keys: the dense branch and
//                               k > 64, three passes over the key blocks (mxa_finish_qk_long.hpp)
//   mxa_qkv_attention_full / mxa_attention_proj_full
//                               those rows with the fused qkv projection in front and the proj Linear
//                               behind: qkv_proj_kernel as it is; the proj's codes from finish16_kernel's
//                               LONG + XO instantiations (MXINT8, D % 32 == 0, k <= 32), else the fp32 copy
// Which of these finishes a call is finish_choice's answer (mxa_launch.hpp) to the call's facts
// (attn_fin_facts): attn_validate takes its refusal, attn_layout whether to hold mask words,
// launch_rows (mxa_fin.hip) the kernel, the *_finish_kernel entry points the kind they report.
//
// This is the mx_quant branch of the patched attention forward:
//   workloads/deit/scripts/main.py:100-152, workloads/DiT/models.py:168-225,
//   workloads/PixArt/models/MX_transformer_block.py:648-717, :792-859.
#include "mxa_launch.hpp"

#include <algorithm>
#include <cstdlib>
#include <mutex>
#include <vector>

namespace mxa {

typedef int v16i __attribute__((ext_vector_type(16)));
typedef int v4i_ __attribute__((ext_vector_type(4)));

// Self-test of the v_mfma_i32_32x32x32_i8 lane maps of the finishing kernel's P.V: A (32x32 row-major
// M x K), B (32x32 row-major K x N) -> C (32x32 row-major) through the same maps.
__global__ void selftest_mfma32_kernel(const int8_t* A, const int8_t* B, int32_t* C) {
  const int lane = threadIdx.x, ln = lane & 31, kh = 16 * (lane >> 5), m0 = 4 * (lane >> 5);
  v4i_ a4, b4;
  for (int w = 0; w < 4; ++w) {
    uint32_t x = 0, y = 0;
    for (int j = 0; j < 4; ++j) {
      x |= (uint32_t)(uint8_t)A[ln * 32 + kh + 4 * w + j] << (8 * j);
      y |= (uint32_t)(uint8_t)B[(kh + 4 * w + j) * 32 + ln] << (8 * j);
    }
    a4[w] = (int)x;
    b4[w] = (int)y;
  }
  const v16i zero = {};
  const v16i c = __builtin_amdgcn_mfma_i32_32x32x32_i8(a4, b4, zero, 0, 0, 0);
  for (int i = 0; i < 16; ++i) C[(8 * (i >> 2) + m0 + (i & 3)) * 32 + ln] = c[i];
}

__global__ void selftest_mfma_kernel(const int8_t* A, const int8_t* B, int32_t* C) {
  // A row-major 16x32, B row-major 32x16 (k-major), C row-major 16x16
  const int lane = threadIdx.x;
  const int r = lane & 15, kg = lane >> 4;
  long av = 0, bv = 0;
  for (int j = 0; j < 8; ++j) {
    av |= (long)(uint8_t)A[r * 32 + kg * 8 + j] << (8 * j);
    bv |= (long)(uint8_t)B[(kg * 8 + j) * 16 + r] << (8 * j);
  }
  const v4i zero = {0, 0, 0, 0};
  const v4i c = __builtin_amdgcn_mfma_i32_16x16x32_i8(av, bv, zero, 0, 0, 0);
  for (int i = 0; i < 4; ++i) C[(4 * kg + i) * 16 + r] = c[i];
}

}  // namespace mxa

using namespace mxa;

namespace {

// the selection kernel's score mode of a call (ranked: the selection kernel runs)
int score_mode(const mxa_attn_params* p, bool ranked) {
  if (!(p->approx && ranked)) return kModeTrue;
  switch (p->pred_mode) {
    case MXA_PRED_EX_PRED: return kModeExSign;
    case MXA_PRED_EXION: return kModeOpMul;
    case MXA_PRED_TRUE_EX: return kModeTrueEx;
    case MXA_PRED_ELSA: return kModeElsa;
    default: return kModeOpExp;
  }
}

// the operands a score mode reads next to the MX codes and exponents of Q and K: approximator
// codes, zero indicators (true_ex), approximator scales, sign / hash words, key norms (ELSA);
// prep_signs: rows_prep writes the sign words (ELSA's hash words are elsa_prep's)
struct ModeNeeds { bool op, z, sa, sg, knorm, prep_signs; };
ModeNeeds mode_needs(int mode) {
  ModeNeeds n{};
  n.op = mode == kModeOpExp || mode == kModeOpMul || mode == kModeTrueEx;
  n.z = mode == kModeTrueEx;
  n.sa = mode != kModeTrue && mode != kModeElsa;
  n.sg = mode == kModeExSign || mode == kModeElsa;
  n.knorm = mode == kModeElsa;
  n.prep_signs = mode == kModeExSign;
  return n;
}

// How far an entry point reaches, in order: each value takes every call the one before it takes, on the
// same kernels.  kReachShort: rows of at most 512 keys; kReachLong (the *_long and *_bits entry points):
// rows of at most kLongRowsT keys on the kernels that existed before finish_qk_long_kernel; kReachFull
// (mxa_attention_full): those rows' dense branch and k_top > 64 too; kReachBlock (mxa_qkv_attention_full,
// mxa_attention_proj_full): on those rows the fused qkv projection and the proj Linear as well
enum Reach { kReachShort, kReachLong, kReachFull, kReachBlock };

// the proj Linear's input comes MX-quantized out of the finishing kernel (MXINT8 only: at 4 bits the
// fp32 rows go through the workspace and the row quantizer for every D; rows over 512 keys: from the LONG
// 16-row kernel alone, k <= 32 -- there is no 32-row kernel behind it, and finish_qk_long_kernel writes fp32)
bool proj_codes_direct(const mxa_attn_params* p, int elem_bits, Reach reach) {
  if (reach == kReachBlock && long_rows(p->T) && !(p->top_k && p->k_top <= 32)) return false;
  return elem_bits == 8 && p->D % 32 == 0 && p->dtype == MXA_DT_F32 && p->score_dtype <= MXA_DT_F32;
}
// a width as a prepared weight's header and flat_rows_prep state it: 0 MXINT8, 4 MXINT4
int header_bits(int elem_bits) { return elem_bits == 4 ? 4 : 0; }

// One attention call
struct AttnCall {
  const mxa_attn_params* p;
  hipStream_t stream;
  const mxa_qkv_params* xq;    // the fused qkv projection (q, k, v produced from x and the prepared weight)
  const mxa_cross_params* xc;  // cross-attention's projections (q from x, k and v from cond; N and T independent)
  const mxa_proj_params* pj;   // the proj Linear behind it (y = mx.Linear(out.transpose(1,2).reshape(B,N,C)))
  bool scores_only;  // the approximate (or true) scores into p->pred_out / true_out, no top-k
  Reach reach;       // the entry point's (kReachShort unless named)
  hipEvent_t* ev;    // the timed entry points' stage events
  int *plan, *fin;   // plan: only report the kernel path (MXA_PATH_*), launch nothing; fin (with plan): the
                     // finishing kernel (MXA_FIN_*, 0 for the scores alone)
  int elem_bits = 8;  // 8 MXINT8; 4 (the *_bits / *_full entry points) MXINT4 for Q, K, P and V and for the
                      // codes every approximator is derived from (include/mxa.h mxa_attention_bits); with
                      // xq / xc / pj (W4A4): for x, cond and the proj's input too, on 4-bit weights
};

// what finish_choice (mxa_launch.hpp) decides a call's finishing kernel from; p: the call's parameters
// as the kernels see them (attention_impl's copy)
FinFacts attn_fin_facts(const AttnCall& c, const mxa_attn_params* p) {
  return {p->top_k != 0, p->top_k ? p->k_top : 0, p->T, (p->D + 31) / 32, c.pj && proj_codes_direct(p, c.elem_bits, c.reach),
          p->dtype != MXA_DT_F32 || p->score_dtype > MXA_DT_F32, c.elem_bits, c.reach >= kReachFull, c.reach == kReachBlock};
}

// one side's (Q's or K's) row operands; null: the score mode does not read it
struct AttnOperands { int8_t *codes, *op, *z; int16_t *sT, *sA; uint32_t* sg; };
AttnOperands carve_operands(Carver& ws, int64_t rows, int nbd, const ModeNeeds& n) {
  const int64_t dpad = 32 * (int64_t)nbd;
  AttnOperands o{};
  o.codes = ws.take<int8_t>(rows * dpad);
  o.op = ws.take<int8_t>(n.op ? rows * dpad : 0);
  o.z = ws.take<int8_t>(n.z ? rows * dpad : 0);
  o.sT = ws.take<int16_t>(rows * nbd);
  o.sA = ws.take<int16_t>(n.sa ? rows * nbd : 0);
  o.sg = ws.take<uint32_t>(n.sg ? rows * nbd : 0);
  return o;
}

// workspace regions in their order, 256-B aligned
struct AttnLayout {
  int nbd, dpad, ntb, tpad;
  ModeNeeds needs;
  AttnOperands q, k;
  float* knorm;
  int8_t* vt; int16_t* vs;
  uint16_t* idx16; uint32_t *tail, *fbf, *mask;
  MxRows x, c;  // fused qkv projection: x's codes / exponents; cross-attention: the query (x), key / value (c) tokens'
  MxRows y;     // fused proj Linear: its input (MFMA-ready) ...
  float* yf;    // ... and the attention's fp32 output it is quantized from (D % 32 != 0 only)
  int64_t total;
};

// p: as attn_fin_facts; workspace: the call's, or null to size it
AttnLayout attn_layout(const AttnCall& c, const mxa_attn_params* p, int mode, void* workspace) {
  const mxa_qkv_params* xq = c.xq;
  const mxa_cross_params* xc = c.xc;
  const mxa_proj_params* pj = c.pj;
  AttnLayout L{};
  Carver ws(workspace);
  const int64_t BH = (int64_t)p->B * p->H;
  L.nbd = (p->D + 31) / 32; L.dpad = L.nbd * 32;
  L.ntb = (p->T + 31) / 32; L.tpad = L.ntb * 32;
  L.needs = mode_needs(mode);
  const int64_t qrows = BH * p->N, krows = BH * p->T;
  L.q = carve_operands(ws, qrows, L.nbd, L.needs);
  L.k = carve_operands(ws, krows, L.nbd, L.needs);
  L.knorm = ws.take<float>(L.needs.knorm ? krows : 0);
  L.vt = ws.take<int8_t>(BH * p->D * (int64_t)L.tpad);
  L.vs = ws.take<int16_t>(BH * L.ntb * (int64_t)p->D);
  L.idx16 = ws.take<uint16_t>(p->top_k ? qrows * (int64_t)p->k_top : 0);  // used when the caller takes no idx
  {  // the one-lane top-k tail's staging records (mxa_tail.hpp); the packed selection
     // pass's per-workgroup flags (at most one workgroup per 16 query rows of a head)
    const bool pk = p->top_k && sel_packs(mode, p->T, p->bias != nullptr);
    const int tw = p->top_k ? sel_tail_width(mode, p->T, p->k_top, p->bias != nullptr) : 0;
    L.tail = ws.take<uint32_t>(tw ? qrows * (int64_t)tail_rec_words(tw) : 0);
    L.fbf = ws.take<uint32_t>(pk ? BH * (int64_t)((p->N + 15) / 16) : 0);
  }
  // the prune-mask words for a finishing kernel that reads them, when the caller takes none
  // (reserved whatever mask_out is: the size must not depend on it; nor does it on P's width, which no
  // kernel kind depends on)
  L.mask = ws.take<uint32_t>(finish_choice(attn_fin_facts(c, p)).reads_mask ? qrows * (int64_t)L.ntb : 0);
  const int64_t qtok = (int64_t)p->B * p->N;
  if (xq) L.x = carve_mx_rows(ws, qtok, xq->C, false);
  if (xc) {
    L.x = carve_mx_rows(ws, qtok, xc->C, false);
    L.c = carve_mx_rows(ws, (int64_t)p->B * p->T, xc->C_kv, false);
  }
  if (pj) {
    L.y = carve_mx_rows(ws, qtok, p->H * p->D, true);
    L.yf = ws.take<float>(proj_codes_direct(p, c.elem_bits, c.reach) ? 0 : qtok * p->H * p->D);
  }
  L.total = ws.off;
  return L;
}

bool attn_shape_ok(const mxa_attn_params* p) { return p && p->B > 0 && p->H > 0 && p->N > 0 && p->T > 0 && p->D > 0; }

// the workspace of a call; sized for the approximator whenever it may run (the proj Linear
// and top-k run the selection kernel, pred_out the scores alone)
int64_t attn_workspace_total(const AttnCall& c) {
  return attn_layout(c, c.p, score_mode(c.p, c.pj || c.p->top_k || c.p->pred_out), nullptr).total;
}

// the refusals of a call, in their order; every one before the prepared weights' header
// checks returns without a HIP call
int attn_validate(const AttnCall& c) {
  const auto [p, stream, xq, xc, pj, scores_only, reach, ev, plan, fin, elem_bits] = c;
  if (!p || !mx_width_ok(elem_bits)) return MXA_ERR_ARG;
  if (pj) {
    if (scores_only || !p->top_k || !pj->wq || !pj->y || pj->out_features <= 0 || pj->y_row_stride < pj->out_features)
      return MXA_ERR_ARG;
    if ((int64_t)p->B * p->N > INT32_MAX) return MXA_ERR_UNSUPPORTED;
  }
  if (xq) {
    if (!xq->x || !xq->wq || xq->C <= 0 || xq->x_row_stride < xq->C || p->N != p->T || scores_only) return MXA_ERR_ARG;
  } else if (xc) {
    if (!xc->x || !xc->cond || !xc->wq_q || !xc->wq_kv || xc->C <= 0 || xc->C_kv <= 0 || xc->x_row_stride < xc->C ||
        xc->cond_row_stride < xc->C_kv || scores_only)
      return MXA_ERR_ARG;
  } else if (!p->q || !p->k) {
    return MXA_ERR_ARG;
  }
  if (!scores_only && ((!p->v && !xq && !xc) || (!p->out && !pj))) return MXA_ERR_ARG;
  if (scores_only && !(p->approx ? p->pred_out : p->true_out)) return MXA_ERR_ARG;
  if (!attn_shape_ok(p)) return MXA_ERR_ARG;
  if (!scores_only && p->top_k && (p->k_top <= 0 || p->k_top > p->T)) return MXA_ERR_ARG;
  if (p->pred_mode < MXA_PRED_EX_PRED || p->pred_mode > MXA_PRED_ELSA) return MXA_ERR_ARG;
  if (p->dtype < MXA_DT_F32 || p->dtype > MXA_DT_BF16 || p->score_dtype < 0 || p->score_dtype > MXA_DT_BF16)
    return MXA_ERR_ARG;
  // W4A4 (a fused projection or proj Linear at 4 bits): float32 tensors and scores, no autocast
  if (elem_bits == 4 && (xq || xc || pj) &&
      (p->dtype != MXA_DT_F32 || p->score_dtype != 0 || (xq && xq->autocast_dtype != 0)))
    return MXA_ERR_UNSUPPORTED;
  // the fused qkv projection on rows over 512 keys: unsupported, not a bad argument, for float16 / bfloat16
  // tensors and under autocast (the rule below would answer MXA_ERR_ARG first; the score dtype and the
  // form without xq are the long rows' refusal further down)
  if (reach == kReachBlock && long_rows(p->T) && xq && (p->dtype != MXA_DT_F32 || xq->autocast_dtype != 0))
    return MXA_ERR_UNSUPPORTED;
  if (xq && (p->dtype != MXA_DT_F32 || (xq->autocast_dtype != 0 && xq->autocast_dtype != p->score_dtype)))
    return MXA_ERR_ARG;  // the fused projection reads fp32 x; under autocast its scores follow autocast
  if (xc && p->dtype != MXA_DT_F32) return MXA_ERR_ARG;
  if (xc && p->score_dtype != 0) return MXA_ERR_UNSUPPORTED;  // the cross projections: float32, no autocast
  // approximators whose operands are not exact in float16 / bfloat16 (EXION's e*(2^l1+2^l2),
  // true_ex's per-element exponents, ELSA's fp32 projections): float32 only
  if ((p->dtype != MXA_DT_F32 || p->score_dtype > MXA_DT_F32) && p->approx &&
      (p->pred_mode == MXA_PRED_EXION || p->pred_mode == MXA_PRED_TRUE_EX || p->pred_mode == MXA_PRED_ELSA))
    return MXA_ERR_UNSUPPORTED;
  if (!valid_bfloat(p->bfloat)) return MXA_ERR_ARG;
  if (p->T > (reach == kReachShort ? kShortRowsT : kLongRowsT) || p->D > 32 * kMaxNB) return MXA_ERR_UNSUPPORTED;
  // rows over 512 keys: float32, no fused projection but kReachBlock's qkv and proj Linears; MXINT4:
  // float32, and the approximators of exponent_approximation (ELSA's hashes would need the width too)
  const bool xdt = p->dtype != MXA_DT_F32 || p->score_dtype > MXA_DT_F32;
  if ((long_rows(p->T) && (xc || ((xq || pj) && reach != kReachBlock) || xdt)) || (elem_bits == 4 && xdt)) return MXA_ERR_UNSUPPORTED;
  if (elem_bits == 4 && p->approx && p->pred_mode == MXA_PRED_ELSA) return MXA_ERR_UNSUPPORTED;
  // ... and a finishing kernel with an instantiation for them (finish_choice: the 16-row and the MFMA
  // kernels), or the scores alone
  if (!scores_only && finish_choice(attn_fin_facts(c, p)).status) return MXA_ERR_UNSUPPORTED;
  // the prepared weights must have been prepared for this geometry and these settings
  // (every weight of the call at the call's width: an 8-bit call refuses a 4-bit weight and a 4-bit
  // call an 8-bit one)
  const int HD = p->H * p->D, fl = p->flush_subnormals, bf = p->bfloat, hb = header_bits(elem_bits);
  if (xq && !linear_weight_verify(xq->wq, linear_weight_header(3 * HD, xq->C, p->D, fl, bf, hb), stream)) return MXA_ERR_ARG;
  if (xc && !(linear_weight_verify(xc->wq_q, linear_weight_header(HD, xc->C, p->D, fl, bf, hb), stream) &&
              linear_weight_verify(xc->wq_kv, linear_weight_header(2 * HD, xc->C_kv, p->D, fl, bf, hb), stream)))
    return MXA_ERR_ARG;
  if (pj) {
    int wb = 0;
    if (!linear_weight_verify_any_group(pj->wq, pj->out_features, HD, fl, bf, stream, hb ? &wb : nullptr) || wb != hb)
      return MXA_ERR_ARG;
  }
  return MXA_OK;
}

// the operand builder's arguments for one side: x at strides s (B, H, row), R rows per head
RowsPrepArgs attn_rows_prep(const mxa_attn_params& pp, const AttnLayout& L, const AttnOperands& o, const void* x,
                            const int64_t* s, int R, int op_kind, int elem_bits) {
  RowsPrepArgs r{};
  r.x = x; r.s0 = s[0]; r.s1 = s[1]; r.s2 = s[2];
  r.H = pp.H; r.R = R; r.rows = (int64_t)pp.B * pp.H * R; r.D = pp.D; r.nb = L.nbd; r.dpad = L.dpad;
  r.vec4 = may_load_16B(x, pp.dtype, s[0], s[1], s[2]);
  r.op_kind = op_kind; r.flush = pp.flush_subnormals; r.bfloat = pp.bfloat;
  r.dt = pp.dtype;  // (the fused projections, which write these operands themselves, take float32 only)
  r.codes = o.codes; r.sT = o.sT; r.op = o.op; r.zind = o.z; r.sA = o.sA;
  r.signs = L.needs.prep_signs ? o.sg : nullptr;
  r.mbits = elem_bits;
  return r;
}

// the token matrix of one projection pass: ntok tokens per image of C features, its prepared
// weight (parts * H * D rows) and bias, the optional fp32 output, its MX rows in the workspace
struct ProjTokens {
  const float* x; int64_t row_stride; int C, ntok;
  const void* wq; const float* bias;
  float* out; int autocast;
  MxRows rows;
};

// One projection pass (part: ProjPart): x -> MX codes along C (rows_prep) into the workspace,
// then the projection kernel on the prepared weight, writing the part's q / k operands (rq,
// rk) and V's transposed codes (cv)
// (elem_bits 4: the tokens quantized at MXINT4, the weight a 4-bit one -- one digit plane)
int launch_proj_pass(const mxa_attn_params& pp, int part, const ProjTokens& t, const RowsPrepArgs& rq,
                     const RowsPrepArgs& rk, const ColsPrepArgs& cv, hipStream_t stream, int elem_bits) {
  const int parts = part == kPartQKV ? 3 : part == kPartKV ? 2 : 1;
  const int nbk = (t.C + 31) / 32, Cpad = 32 * nbk;
  const int64_t tokens = (int64_t)pp.B * t.ntok;
  const RowsPrepArgs rx = flat_rows_prep(t.x, tokens, t.C, t.row_stride, pp.flush_subnormals, pp.bfloat, t.rows.codes, t.rows.exps, 0,
                                         header_bits(elem_bits));
  int rc = launch_rows_prep(rx, stream);
  if (rc) return rc;
  const LinearLayout W = linear_layout(parts * pp.H * pp.D, t.C, pp.D, header_bits(elem_bits));
  const unsigned char* wb = static_cast<const unsigned char*>(t.wq);
  ProjArgs pa{};
  pa.xc = t.rows.codes; pa.xs = t.rows.exps;  // (rx's codes / sT, or at 4 bits its op / sA)
  pa.pk = reinterpret_cast<const int8_t*>(wb + W.pk);
  pa.pe = reinterpret_cast<const int16_t*>(wb + W.pe);
  pa.ps = reinterpret_cast<const int16_t*>(wb + W.ps);
  pa.gs = reinterpret_cast<const int16_t*>(wb + W.gs);
  pa.pn = reinterpret_cast<const int16_t*>(wb + W.pn);
  pa.pd = reinterpret_cast<const int8_t*>(wb + W.pd);
  if (W.ps - W.pk >= ((int64_t)1 << 31) || W.total - W.pd >= ((int64_t)1 << 31))
    return MXA_ERR_UNSUPPORTED;  // 32-bit buffer offsets
  pa.pk_bytes = (int)(W.pe - W.pk);
  pa.pe_bytes = (int)(W.ps - W.pe);
  pa.pd_bytes = (int)(W.total - W.pd);
  pa.ntb = (t.ntok + 31) / 32;
  pa.bias = t.bias; pa.qkv_out = t.out; pa.autocast = t.autocast;
  pa.B = pp.B; pa.N = t.ntok; pa.H = pp.H; pa.D = pp.D; pa.nbk = nbk; pa.Cpad = Cpad; pa.bfloat = pp.bfloat;
  pa.smax = gemm_smax(nbk);
  pa.rq = rq; pa.rk = rk; pa.cv = cv;
  return elem_bits == 4 ? launch_proj4(pa, stream, part) : launch_proj(pa, stream, part);
}

// ---- the fork: finish-only operands beside the tail ("The side lane") ----
// A call on q, k, v whose packed selection hands its rows to the one-lane tail is five dependent
// kernels, and the tail (LDS-bound at three waves per SIMD) leaves registers, wave slots and the whole
// memory system idle.  What only the finishing kernel reads is therefore built on a stream of the
// library's own, behind the packed selection pass and beside the tail, and joined before the finishing
// kernel; the caller still sees one ordered stream.  Beside select_kernel itself the same launch only
// takes its issue slots (measured), so a call without a tail does not fork.
// What moves: V's columns.  Measured and left where they were (§8): the codes and sT of Q and K (a
// second pass over Q and K, longer than the tail) and the 64-bit selection pass (launch_select_packed).
constexpr int kSideDevices = 64;

// One device's lane: created on the first forked call there and kept for the process
struct SideState {
  int state;  // 0 untried, 1 usable, -1 the runtime gave none (calls keep the single-stream order)
  hipStream_t stream;
  hipEvent_t packed, join;
};

// One call's use of the lane.  The lane and its events are one per device, so forked calls hold a
// process-wide lock from their fork to their join's enqueue (host time only); the streams order the rest.
//   lane():    what launch_select forks with: it records `packed` behind the packed pass on the caller's
//              stream and makes the lane wait for it -- so the lane is also behind the call's critical
//              builder and behind the previous call's finishing kernel, which still reads the tables
//              the side launches overwrite
//   forked():  launch_select did; the lane now holds work to join
//   join():    the caller's stream waits for the lane (the destructor does, on an error path too)
class SideFork {
 public:
  SideFork(hipStream_t caller, bool wanted) : caller_(caller) {
    if (!wanted) return;
    hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing(caller, &cap) != hipSuccess || cap != hipStreamCaptureStatusNone) {
      (void)hipGetLastError();
      return;  // under capture: today's single-stream order
    }
    static std::mutex mu;
    lock_ = std::unique_lock<std::mutex>(mu);
    s_ = lane(caller);
    if (!s_) lock_.unlock();
  }
  ~SideFork() { (void)join(); }
  SideFork(const SideFork&) = delete;
  SideFork& operator=(const SideFork&) = delete;
  bool on() const { return s_ != nullptr; }
  hipStream_t stream() const { return s_->stream; }
  SideLane lane() const { return {s_->stream, s_->packed}; }
  void forked() { forked_ = true; }
  int join() {
    if (!forked_) return MXA_OK;
    forked_ = false;
    const bool ok = hipEventRecord(s_->join, s_->stream) == hipSuccess && hipStreamWaitEvent(caller_, s_->join, 0) == hipSuccess;
    return ok ? MXA_OK : MXA_ERR_LAUNCH;
  }

 private:
  // the lane of the caller's device, which must be the current one (the lane is created on it)
  static SideState* lane(hipStream_t caller) {
    static SideState lanes[kSideDevices] = {};
    int dev = -1;
    hipDevice_t sdev = -1;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= kSideDevices ||
        (caller && (hipStreamGetDevice(caller, &sdev) != hipSuccess || (int)sdev != dev))) {
      (void)hipGetLastError();
      return nullptr;
    }
    SideState& s = lanes[dev];
    if (s.state == 0) {
      const bool ok = hipStreamCreateWithFlags(&s.stream, hipStreamNonBlocking) == hipSuccess &&
                      hipEventCreateWithFlags(&s.packed, hipEventDisableTiming) == hipSuccess &&
                      hipEventCreateWithFlags(&s.join, hipEventDisableTiming) == hipSuccess;
      s.state = ok ? 1 : -1;
      if (!ok) (void)hipGetLastError();
    }
    return s.state == 1 ? &s : nullptr;
  }
  hipStream_t caller_;
  SideState* s_ = nullptr;
  bool forked_ = false;
  std::unique_lock<std::mutex> lock_;
};

// Q's and K's operands and V's transposed codes: from q, k, v in one launch (scores alone: Q
// and K), or out of the fused projections -- qkv in one pass; cross-attention's query tokens
// -> the q operands, then its key / value tokens -> the k operands and V (two launches of
// the projection kernel by parts).  side (a forked call on q, k, v): Q's and K's rows are launched
// here and V's builder is left in *side for the lane (launch_cols_prep)
int attn_build_operands(const AttnCall& c, const mxa_attn_params& pp, const AttnLayout& L, int opq, int opk, ColsPrepArgs* side) {
  const int bits = c.elem_bits;
  const RowsPrepArgs rq = attn_rows_prep(pp, L, L.q, pp.q, pp.q_strides, pp.N, opq, bits);
  const RowsPrepArgs rk = attn_rows_prep(pp, L, L.k, pp.k, pp.k_strides, pp.T, opk, bits);
  ColsPrepArgs cv{};
  cv.x = pp.v; cv.s0 = pp.v_strides[0]; cv.s1 = pp.v_strides[1]; cv.s2 = pp.v_strides[2];
  cv.H = pp.H; cv.mats = (int64_t)pp.B * pp.H; cv.R = pp.T; cv.C = pp.D; cv.nb = L.ntb; cv.rpad = L.tpad;
  cv.mbits = bits; cv.flush = pp.flush_subnormals; cv.bfloat = pp.bfloat; cv.dt = pp.dtype;
  cv.codes_t = L.vt; cv.tb_major = 1; cv.scale = L.vs;
  if (c.xq) {
    const mxa_qkv_params& xq = *c.xq;
    return launch_proj_pass(pp, kPartQKV, {xq.x, xq.x_row_stride, xq.C, pp.N, xq.wq, xq.bias, xq.qkv_out, xq.autocast_dtype, L.x},
                            rq, rk, cv, c.stream, bits);
  }
  if (c.xc) {
    const mxa_cross_params& xc = *c.xc;
    const int rc = launch_proj_pass(pp, kPartQ, {xc.x, xc.x_row_stride, xc.C, pp.N, xc.wq_q, xc.bias_q, xc.q_out, 0, L.x}, rq,
                                    rk, cv, c.stream, bits);
    if (rc) return rc;
    return launch_proj_pass(pp, kPartKV, {xc.cond, xc.cond_row_stride, xc.C_kv, pp.T, xc.wq_kv, xc.bias_kv, xc.kv_out, 0, L.c},
                            rq, rk, cv, c.stream, bits);
  }
  if (c.scores_only) {
    const int rc = launch_rows_prep(rq, c.stream);
    return rc ? rc : launch_rows_prep(rk, c.stream);
  }
  if (!side) return launch_attn_prep(rq, rk, cv, c.stream);  // Q, K and V in one launch
  *side = cv;
  ColsPrepArgs none = cv;
  none.mats = 0;
  return launch_attn_prep(rq, rk, none, c.stream);
}

// ELSA: hashes of MX(Q), MX(K); norms of MX(K) rows
int attn_elsa_prep(const mxa_attn_params& pp, const AttnLayout& L, hipStream_t stream) {
  const int64_t BH = (int64_t)pp.B * pp.H;
  ElsaPrepArgs eq{};
  eq.codes = L.q.codes; eq.sT = L.q.sT; eq.proj = pp.elsa_proj; eq.rows = BH * pp.N;
  eq.D = pp.D; eq.nb = L.nbd; eq.dpad = L.dpad; eq.hash = L.q.sg;
  const int rc = launch_elsa_prep(eq, stream);
  if (rc) return rc;
  ElsaPrepArgs ek = eq;
  ek.codes = L.k.codes; ek.sT = L.k.sT; ek.rows = BH * pp.T; ek.hash = L.k.sg; ek.norm = L.knorm;
  return launch_elsa_prep(ek, stream);
}

// the selection and finishing kernels' arguments: the call's geometry ...
Rows2Args rows2_shape(const mxa_attn_params& pp, const AttnLayout& L) {
  Rows2Args r2{};
  r2.B = pp.B; r2.H = pp.H; r2.N = pp.N; r2.T = pp.T; r2.D = pp.D;
  r2.nbd = L.nbd; r2.dpad = L.dpad; r2.ntb = L.ntb; r2.tpad = L.tpad; r2.k_top = pp.top_k ? pp.k_top : 0;
  r2.kst = L.dpad + 16; r2.vst = L.tpad + 16;  // conflict-free b128 reads of the LDS code tables
  return r2;
}
// ... and, once the workspace is known to hold the layout, its operands and outputs (direct:
// the finishing kernel writes the proj Linear's input codes)
int rows2_bind(Rows2Args& r2, const mxa_attn_params& pp, const AttnLayout& L, const mxa_proj_params* pj, bool direct) {
  r2.qc = L.q.codes; r2.qop = L.q.op; r2.qz = L.q.z; r2.qsT = L.q.sT; r2.qsA = L.q.sA; r2.qsg = L.q.sg;
  r2.kc = L.k.codes; r2.kop = L.k.op; r2.kz = L.k.z; r2.ksT = L.k.sT; r2.ksA = L.k.sA; r2.ksg = L.k.sg;
  r2.knorm = L.knorm; r2.elsa_cos = pp.elsa_cos; r2.vt = L.vt; r2.vs = L.vs;
  r2.bfloat = pp.bfloat; r2.flush_p = pp.flush_subnormals; r2.scale = pp.scale;
  r2.in_dt = pp.dtype; r2.s_dt = pp.score_dtype > MXA_DT_F32 ? pp.score_dtype : pp.dtype;
  r2.bias = pp.bias;
  r2.bs0 = pp.bias_strides[0]; r2.bs1 = pp.bias_strides[1]; r2.bs2 = pp.bias_strides[2]; r2.bs3 = pp.bias_strides[3];
  r2.out = pp.out; r2.os0 = pp.out_strides[0]; r2.os1 = pp.out_strides[1]; r2.os2 = pp.out_strides[2];
  r2.idx_out = pp.idx_out; r2.true_out = pp.true_out; r2.pred_out = pp.pred_out; r2.mask_out = pp.mask_out;
  r2.idx16 = L.idx16; r2.tail_rec = L.tail; r2.fb_flags = L.fbf;
  if (!r2.mask_out) r2.mask_out = L.mask;  // (the layout holds one exactly when the MFMA finishing kernel runs)
  if (direct) {
    r2.xo_codes = L.y.codes; r2.xo_exps = L.y.exps;
  } else if (pj) {  // fp32 (B, N, H*D) into the workspace, then the row quantizer
    r2.out = L.yf;
    r2.os0 = (int64_t)pp.N * pp.H * pp.D; r2.os1 = pp.D; r2.os2 = (int64_t)pp.H * pp.D;
    r2.s_dt = MXA_DT_F32;
    if (pp.dtype != MXA_DT_F32 || pp.score_dtype > MXA_DT_F32) return MXA_ERR_UNSUPPORTED;
  }
  return MXA_OK;
}

// the proj Linear on the attention's output rows (quantized first unless the finishing
// kernel wrote the codes)
int attn_proj_linear(const mxa_attn_params& pp, const AttnLayout& L, const mxa_proj_params& pj, bool direct,
                     hipStream_t stream, int elem_bits) {
  const int C = pp.H * pp.D;
  const int64_t tokens = (int64_t)pp.B * pp.N;
  if (!direct) {
    const int rc =
        launch_rows_prep(flat_rows_prep(L.yf, tokens, C, C, pp.flush_subnormals, pp.bfloat, L.y.codes, L.y.exps, 1,
                                        header_bits(elem_bits)),
                         stream);
    if (rc) return rc;
  }
  return launch_linear_codes(L.y.codes, L.y.exps, tokens, C, pj.wq, pj.out_features, pj.bias, pj.y, pj.y_row_stride,
                             pp.bfloat, 0, stream, true);
}

int attention_impl(const AttnCall& c) {
  int rc = attn_validate(c);
  if (rc) return rc;
  mxa_attn_params pp = *c.p;
  if (c.scores_only) {  // the selection kernel alone, with no kept keys
    pp.top_k = pp.k_top = 0;
    pp.idx_out = nullptr; pp.mask_out = nullptr;
  }
  const bool topk = pp.top_k != 0;
  const bool ranked = topk || c.scores_only;  // the selection kernel runs
  const int mode = score_mode(&pp, ranked);
  if (mode == kModeElsa && (!pp.elsa_proj || pp.N != pp.T)) return MXA_ERR_ARG;  // elsa_approximation.py:126, :142
  const AttnLayout L = attn_layout(c, &pp, mode, pp.workspace);
  const int BH = (int)((int64_t)pp.B * pp.H);
  const FinFacts ff = attn_fin_facts(c, &pp);
  const bool direct = ff.xo;

  int opq = MXA_OP_SIGN, opk = MXA_OP_SIGN;
  switch (pp.pred_mode) {
    case MXA_PRED_PARTIAL_Q: opq = MXA_OP_MXINT8; break;  // Q = MXINT8, K = exp-sign
    case MXA_PRED_PARTIAL_K: opk = MXA_OP_MXINT8; break;  // Q = exp-sign, K = MXINT8
    case MXA_PRED_MXINT4: opq = opk = MXA_OP_MXINT4; break;
    case MXA_PRED_EXION: opq = opk = MXA_OP_EXION; break;
    case MXA_PRED_TRUE_EX: opq = opk = MXA_OP_TRUE_EX; break;
    default: break;
  }
  const int S0 = (pp.T + 63) / 64;
  const int S = S0 <= 1 ? 1 : (S0 <= 2 ? 2 : (S0 <= 4 ? 4 : 8));
  Rows2Args r2 = rows2_shape(pp, L);
  // feasibility of the path's kernels (LDS budgets), before any pointer is bound
  // (rows over 512 keys: the one-wave-per-row selection kernel, mxa_select_long.hpp)
  auto select = [&](bool plan, const SideLane* side = nullptr) {
    return long_rows(pp.T) ? launch_select_long(r2, mode, BH, c.stream, plan) : launch_select(r2, mode, BH, c.stream, plan, side);
  };
  rc = c.scores_only ? MXA_OK : launch_rows(r2, ff, mode == kModeTrue, S, BH, c.stream, true);
  if (!rc && ranked) rc = select(true);
  if (rc) return rc;
  if (c.plan) {
    *c.plan = topk ? MXA_PATH_ROWS_SPLIT : MXA_PATH_ROWS_FUSED;
    if (c.fin) *c.fin = c.scores_only ? 0 : finish_choice(ff).kind;
    return MXA_OK;
  }
  if (!pp.workspace || pp.workspace_bytes < L.total) return MXA_ERR_WORKSPACE;
  if (!aligned16(pp.workspace)) return MXA_ERR_ARG;

  auto mark = [&c](int slot) { if (c.ev) (void)hipEventRecord(c.ev[slot], c.stream); };  // a stage's start
  mark(0);
  // forked: q, k, v given and the packed selection with its tail to run beside (launch_select_packed's
  // tail branch, which forks the lane it is given)
  SideFork fork(c.stream, topk && !c.xq && !c.xc && !long_rows(pp.T) && L.fbf &&
                              sel_tail_width(mode, pp.T, pp.k_top, pp.bias != nullptr) == kTailPref);
  ColsPrepArgs side{};
  rc = attn_build_operands(c, pp, L, opq, opk, fork.on() ? &side : nullptr);
  if (!rc && mode == kModeElsa) rc = attn_elsa_prep(pp, L, c.stream);
  if (rc) return rc;
  mark(1), mark(2), mark(3);  // stages 1 and 2 are empty: the operand builders run as stage 0
  rc = rows2_bind(r2, pp, L, c.pj, direct);
  if (!rc && ranked) {
    const SideLane lane = fork.on() ? fork.lane() : SideLane{};
    rc = select(false, fork.on() ? &lane : nullptr);
  }
  if (fork.on()) {
    fork.forked();  // (joined after an error too)
    if (!rc) rc = launch_cols_prep(side, fork.stream());
    const int rj = fork.join();  // the finishing kernel reads what the lane built
    if (!rc) rc = rj;
  }
  if (rc) return rc;
  mark(4);
  if (!c.scores_only) {
    rc = launch_rows(r2, ff, mode == kModeTrue, S, BH, c.stream, false);
    if (rc) return rc;
  }
  mark(5);
  if (c.pj) {
    rc = attn_proj_linear(pp, L, *c.pj, direct, c.stream, c.elem_bits);
    if (rc) return rc;
    mark(6);
  }
  return MXA_OK;
}

int timed_impl(const mxa_attn_params* p, const mxa_qkv_params* xq, const mxa_proj_params* pj, hipStream_t stream,
               int32_t iters, float* stage_ms) {
  if (iters <= 0 || !stage_ms) return MXA_ERR_ARG;
  const int ns = pj ? MXA_PROJ_STAGES : MXA_ATTN_STAGES, ne = ns + 1;
  std::vector<hipEvent_t> ev((size_t)iters * ne);
  for (auto& e : ev)
    if (hipEventCreate(&e) != hipSuccess) return MXA_ERR_LAUNCH;
  int rc = MXA_OK;
  for (int i = 0; i < iters && rc == MXA_OK; ++i)
    rc = attention_impl({.p = p, .stream = stream, .xq = xq, .pj = pj, .ev = &ev[(size_t)i * ne]});
  if (rc == MXA_OK && hipStreamSynchronize(stream) != hipSuccess) rc = MXA_ERR_LAUNCH;
  if (rc == MXA_OK) {
    for (int s = 0; s < ns; ++s) {
      double acc = 0.0;
      for (int i = 0; i < iters; ++i) {
        float ms = 0.0f;
        (void)hipEventElapsedTime(&ms, ev[(size_t)i * ne + s], ev[(size_t)i * ne + s + 1]);
        acc += ms;
      }
      stage_ms[s] = (float)(acc / iters);
    }
  }
  for (auto& e : ev) (void)hipEventDestroy(e);
  return rc;
}

}  // namespace

extern "C" int mxa_abi_version(void) { return MXA_ABI_VERSION; }

extern "C" const char* mxa_status_string(int status) {
  switch (status) {
    case MXA_OK: return "ok";
    case MXA_ERR_ARG: return "invalid argument";
    case MXA_ERR_UNSUPPORTED: return "unsupported configuration";
    case MXA_ERR_LAUNCH: return "HIP kernel launch failed";
    case MXA_ERR_WORKSPACE: return "workspace too small";
    default: return "unknown status";
  }
}

extern "C" int64_t mxa_attention_workspace_bytes(const mxa_attn_params* p) {
  return attn_shape_ok(p) ? attn_workspace_total({.p = p}) : -1;
}

extern "C" int64_t mxa_qkv_attention_workspace_bytes(const mxa_attn_params* p, const mxa_qkv_params* xq) {
  if (!attn_shape_ok(p) || !xq || xq->C <= 0) return -1;
  return attn_workspace_total({.p = p, .xq = xq});
}

extern "C" int64_t mxa_attention_proj_workspace_bytes(const mxa_attn_params* p, const mxa_qkv_params* xq,
                                                      const mxa_proj_params* pj) {
  if (!attn_shape_ok(p) || !pj || pj->out_features <= 0 || (xq && xq->C <= 0)) return -1;
  return attn_workspace_total({.p = p, .xq = xq, .pj = pj});
}

extern "C" int64_t mxa_cross_attention_workspace_bytes(const mxa_attn_params* p, const mxa_cross_params* xc,
                                                       const mxa_proj_params* pj) {
  if (!attn_shape_ok(p) || !xc || xc->C <= 0 || xc->C_kv <= 0 || (pj && pj->out_features <= 0)) return -1;
  return attn_workspace_total({.p = p, .xc = xc, .pj = pj});
}

extern "C" int mxa_attention(const mxa_attn_params* p, hipStream_t stream) {
  return attention_impl({.p = p, .stream = stream});
}

extern "C" int mxa_approx_scores(const mxa_attn_params* p, hipStream_t stream) {
  return attention_impl({.p = p, .stream = stream, .scores_only = true});
}

extern "C" int64_t mxa_attention_long_workspace_bytes(const mxa_attn_params* p) {
  return mxa_attention_workspace_bytes(p);  // one layout (attn_layout): no region has a 512-key limit
}

extern "C" int mxa_attention_long(const mxa_attn_params* p, hipStream_t stream) {
  return attention_impl({.p = p, .stream = stream, .reach = kReachLong});
}

extern "C" int mxa_approx_scores_long(const mxa_attn_params* p, hipStream_t stream) {
  return attention_impl({.p = p, .stream = stream, .scores_only = true, .reach = kReachLong});
}

extern "C" int64_t mxa_attention_bits_workspace_bytes(const mxa_attn_params* p, int32_t elem_bits) {
  // codes stay one byte each: the same regions at either width
  return mx_width_ok(elem_bits) ? mxa_attention_long_workspace_bytes(p) : -1;
}

extern "C" int mxa_attention_bits(const mxa_attn_params* p, int32_t elem_bits, hipStream_t stream) {
  return attention_impl({.p = p, .stream = stream, .reach = kReachLong, .elem_bits = elem_bits});
}

// mxa_attention_bits plus, on rows over 512 keys, the dense branch and k_top > 64
// (MX_transformer_block.py:704-705, :700-702) on finish_qk_long_kernel
extern "C" int64_t mxa_attention_full_workspace_bytes(const mxa_attn_params* p, int32_t elem_bits) {
  return mx_width_ok(elem_bits) && attn_shape_ok(p) ? attn_workspace_total({.p = p, .reach = kReachFull}) : -1;
}

extern "C" int mxa_attention_full(const mxa_attn_params* p, int32_t elem_bits, hipStream_t stream) {
  return attention_impl({.p = p, .stream = stream, .reach = kReachFull, .elem_bits = elem_bits});
}

extern "C" int mxa_attention_full_finish_kernel(const mxa_attn_params* p, int32_t elem_bits) {
  int plan = -1, fin = -1;
  const int rc = attention_impl({.p = p, .reach = kReachFull, .plan = &plan, .fin = &fin, .elem_bits = elem_bits});
  return rc ? rc : fin;
}

extern "C" int mxa_approx_scores_bits(const mxa_attn_params* p, int32_t elem_bits, hipStream_t stream) {
  return attention_impl({.p = p, .stream = stream, .scores_only = true, .reach = kReachLong, .elem_bits = elem_bits});
}

extern "C" int mxa_qkv_attention(const mxa_attn_params* p, const mxa_qkv_params* xq, hipStream_t stream) {
  if (!xq) return MXA_ERR_ARG;
  return attention_impl({.p = p, .stream = stream, .xq = xq});
}

extern "C" int mxa_attention_proj(const mxa_attn_params* p, const mxa_qkv_params* xq, const mxa_proj_params* pj,
                                  hipStream_t stream) {
  if (!pj) return MXA_ERR_ARG;
  return attention_impl({.p = p, .stream = stream, .xq = xq, .pj = pj});
}

extern "C" int mxa_cross_attention(const mxa_attn_params* p, const mxa_cross_params* xc, const mxa_proj_params* pj,
                                   hipStream_t stream) {
  if (!xc) return MXA_ERR_ARG;
  return attention_impl({.p = p, .stream = stream, .xc = xc, .pj = pj});
}

// The fused blocks at a stated width.  8: the siblings above, call for call.  4 (W4A4): every weight a
// 4-bit one, x / cond and the proj's input quantized at MXINT4, the attention mxa_attention_bits(p, 4)'s
// on rows of at most 512 keys
extern "C" int64_t mxa_qkv_attention_bits_workspace_bytes(const mxa_attn_params* p, const mxa_qkv_params* xq,
                                                          int32_t elem_bits) {
  if (!mx_width_ok(elem_bits) || !attn_shape_ok(p) || !xq || xq->C <= 0) return -1;
  return attn_workspace_total({.p = p, .xq = xq, .elem_bits = elem_bits});
}

extern "C" int mxa_qkv_attention_bits(const mxa_attn_params* p, const mxa_qkv_params* xq, int32_t elem_bits,
                                      hipStream_t stream) {
  if (!xq) return MXA_ERR_ARG;
  return attention_impl({.p = p, .stream = stream, .xq = xq, .elem_bits = elem_bits});
}

extern "C" int64_t mxa_attention_proj_bits_workspace_bytes(const mxa_attn_params* p, const mxa_qkv_params* xq,
                                                           const mxa_proj_params* pj, int32_t elem_bits) {
  if (!mx_width_ok(elem_bits) || !attn_shape_ok(p) || !pj || pj->out_features <= 0 || (xq && xq->C <= 0)) return -1;
  return attn_workspace_total({.p = p, .xq = xq, .pj = pj, .elem_bits = elem_bits});
}

extern "C" int mxa_attention_proj_bits(const mxa_attn_params* p, const mxa_qkv_params* xq, const mxa_proj_params* pj,
                                       int32_t elem_bits, hipStream_t stream) {
  if (!pj) return MXA_ERR_ARG;
  return attention_impl({.p = p, .stream = stream, .xq = xq, .pj = pj, .elem_bits = elem_bits});
}

extern "C" int64_t mxa_cross_attention_bits_workspace_bytes(const mxa_attn_params* p, const mxa_cross_params* xc,
                                                            const mxa_proj_params* pj, int32_t elem_bits) {
  if (!mx_width_ok(elem_bits) || !attn_shape_ok(p) || !xc || xc->C <= 0 || xc->C_kv <= 0 || (pj && pj->out_features <= 0))
    return -1;
  return attn_workspace_total({.p = p, .xc = xc, .pj = pj, .elem_bits = elem_bits});
}

extern "C" int mxa_cross_attention_bits(const mxa_attn_params* p, const mxa_cross_params* xc, const mxa_proj_params* pj,
                                        int32_t elem_bits, hipStream_t stream) {
  if (!xc) return MXA_ERR_ARG;
  return attention_impl({.p = p, .stream = stream, .xc = xc, .pj = pj, .elem_bits = elem_bits});
}

// The self-attention blocks at their full reach: the *_bits siblings call for call on rows of at most 512
// keys; on rows of 513 .. 1,024 keys the fused qkv projection in front of, and the proj Linear behind,
// what mxa_attention_full runs there (MX_transformer_block.py:624-717 at 512 x 512)
extern "C" int64_t mxa_qkv_attention_full_workspace_bytes(const mxa_attn_params* p, const mxa_qkv_params* xq,
                                                          int32_t elem_bits) {
  if (!mx_width_ok(elem_bits) || !attn_shape_ok(p) || !xq || xq->C <= 0) return -1;
  return attn_workspace_total({.p = p, .xq = xq, .reach = kReachBlock, .elem_bits = elem_bits});
}

extern "C" int mxa_qkv_attention_full(const mxa_attn_params* p, const mxa_qkv_params* xq, int32_t elem_bits,
                                      hipStream_t stream) {
  if (!xq) return MXA_ERR_ARG;
  return attention_impl({.p = p, .stream = stream, .xq = xq, .reach = kReachBlock, .elem_bits = elem_bits});
}

extern "C" int64_t mxa_attention_proj_full_workspace_bytes(const mxa_attn_params* p, const mxa_qkv_params* xq,
                                                           const mxa_proj_params* pj, int32_t elem_bits) {
  if (!mx_width_ok(elem_bits) || !attn_shape_ok(p) || !pj || pj->out_features <= 0 || (xq && xq->C <= 0)) return -1;
  return attn_workspace_total({.p = p, .xq = xq, .pj = pj, .reach = kReachBlock, .elem_bits = elem_bits});
}

extern "C" int mxa_attention_proj_full(const mxa_attn_params* p, const mxa_qkv_params* xq, const mxa_proj_params* pj,
                                       int32_t elem_bits, hipStream_t stream) {
  if (!pj) return MXA_ERR_ARG;
  return attention_impl({.p = p, .stream = stream, .xq = xq, .pj = pj, .reach = kReachBlock, .elem_bits = elem_bits});
}

extern "C" int mxa_attention_path(const mxa_attn_params* p) {
  int plan = -1;
  const int rc = attention_impl({.p = p, .plan = &plan});
  return rc ? rc : plan;
}

extern "C" int mxa_attention_finish_kernel(const mxa_attn_params* p) {
  int plan = -1, fin = -1;
  const int rc = attention_impl({.p = p, .plan = &plan, .fin = &fin});
  return rc ? rc : fin;
}

extern "C" int mxa_attention_timed(const mxa_attn_params* p, hipStream_t stream, int32_t iters, float* stage_ms) {
  return timed_impl(p, nullptr, nullptr, stream, iters, stage_ms);
}

extern "C" int mxa_qkv_attention_timed(const mxa_attn_params* p, const mxa_qkv_params* xq, hipStream_t stream,
                                       int32_t iters, float* stage_ms) {
  if (!xq) return MXA_ERR_ARG;
  return timed_impl(p, xq, nullptr, stream, iters, stage_ms);
}

extern "C" int mxa_attention_proj_timed(const mxa_attn_params* p, const mxa_qkv_params* xq, const mxa_proj_params* pj,
                                        hipStream_t stream, int32_t iters, float* stage_ms) {
  if (!pj) return MXA_ERR_ARG;
  return timed_impl(p, xq, pj, stream, iters, stage_ms);
}

// mx.matmul's workspace: the MX rows along K of a, then of b's transpose (Nc rows per matrix)
struct MatmulLayout { MxRows a, bt; };
static MatmulLayout matmul_layout(Carver& ws, int64_t batch, int M, int K, int Nc) {
  MatmulLayout L{};
  L.a = carve_mx_rows(ws, batch * M, K, false);
  L.bt = carve_mx_rows(ws, batch * Nc, K, false);
  return L;
}

extern "C" int64_t mxa_matmul_workspace_bytes(int64_t batch, int32_t M, int32_t K, int32_t Nc) {
  if (batch <= 0 || M <= 0 || K <= 0 || Nc <= 0) return -1;
  Carver ws;
  matmul_layout(ws, batch, M, K, Nc);
  return ws.off;
}

// in2 given as b (batch, K, Nc) row-major (cols_prep: codes transposed to [Nc][kpad],
// exponents [nbk][Nc]) or, bt_rows, as its transpose bt (batch, Nc, K) row-major (rows_prep:
// the same codes and blocks along K, exponents [Nc][nbk]) -- the k.transpose(-2, -1) view of
// the callers needs no copy
static int matmul_impl(const void* a, const void* b, bool bt_rows, void* c, int64_t batch, int32_t M, int32_t K,
                       int32_t Nc, int64_t a_batch_stride, int64_t b_batch_stride, int32_t elem_mbits_a,
                       int32_t elem_mbits_b, int32_t flush_subnormals, int32_t bfloat, int32_t a_dtype, int32_t b_dtype,
                       int32_t c_dtype, void* workspace, int64_t workspace_bytes, hipStream_t stream) {
  if (!a || !b || !c || batch <= 0 || M <= 0 || K <= 0 || Nc <= 0) return MXA_ERR_ARG;
  for (int dt : {a_dtype, b_dtype, c_dtype})
    if (dt < MXA_DT_F32 || dt > MXA_DT_BF16) return MXA_ERR_ARG;
  if (!mx_width_ok(elem_mbits_a) || !mx_width_ok(elem_mbits_b)) return MXA_ERR_UNSUPPORTED;
  if (!valid_bfloat(bfloat)) return MXA_ERR_ARG;
  Carver ws(workspace);
  const MatmulLayout L = matmul_layout(ws, batch, M, K, Nc);
  if (!workspace || workspace_bytes < ws.off) return MXA_ERR_WORKSPACE;
  const int nbk = (K + 31) / 32, kpad = nbk * 32;
  int8_t *ac = L.a.codes, *bt = L.bt.codes;
  int16_t *as = L.a.exps, *bsc = L.bt.exps;
  // MX rows along K (rows_prep): a, and b's transpose when given so
  auto rows_mx = [&](const void* x, int64_t bstride, int R, int mbits, int dt, int8_t* codes, int16_t* exps) {
    RowsPrepArgs ra{};
    ra.x = x; ra.s0 = bstride; ra.s1 = 0; ra.s2 = K; ra.H = 1; ra.R = R; ra.rows = batch * R;
    ra.D = K; ra.nb = nbk; ra.dpad = kpad;
    ra.vec4 = may_load_16B(x, dt, bstride, 0, K);
    ra.op_kind = mbits == 8 ? MXA_OP_MXINT8 : MXA_OP_MXINT4;
    ra.flush = flush_subnormals; ra.bfloat = bfloat; ra.dt = dt;
    ra.codes = nullptr; ra.sT = nullptr; ra.op = codes; ra.sA = exps;
    return launch_rows_prep(ra, stream);
  };
  int rc = rows_mx(a, a_batch_stride, M, elem_mbits_a, a_dtype, ac, as);
  if (rc) return rc;
  if (bt_rows) {
    rc = rows_mx(b, b_batch_stride, Nc, elem_mbits_b, b_dtype, bt, bsc);
  } else {
    ColsPrepArgs cb{};
    cb.x = b; cb.s0 = b_batch_stride; cb.s1 = 0; cb.s2 = Nc; cb.H = 1; cb.mats = batch; cb.R = K; cb.C = Nc;
    cb.nb = nbk; cb.rpad = kpad; cb.mbits = elem_mbits_b; cb.flush = flush_subnormals; cb.bfloat = bfloat; cb.dt = b_dtype;
    cb.codes_t = bt; cb.scale = bsc;
    rc = launch_cols_prep(cb, stream);
  }
  if (rc) return rc;
  // C[b] = MX(A[b]) @ MX(B[b]) on the block-scaled GEMM (mxa_gemm.hpp): A's MX codes
  // row-major along K, B's transposed codes [Nc][kpad], exponents [nbk][Nc] or [Nc][nbk]
  GemmArgs g{};
  g.a = ac; g.ae = as; g.a_bat = (int64_t)M * kpad; g.ae_bat = (int64_t)M * nbk; g.lda = kpad;
  g.b = bt; g.b_bat = (int64_t)Nc * kpad; g.ldb = kpad;
  g.be = bsc; g.be_bat = (int64_t)nbk * Nc;
  g.be_n = bt_rows ? nbk : 1; g.be_k = bt_rows ? 1 : Nc;
  g.M = M; g.Nc = Nc; g.nbk = nbk;
  g.linear = 0; g.dt = c_dtype; g.bfloat = bfloat;
  g.c = c; g.c_bat = (int64_t)M * Nc; g.ldc = Nc;
  return launch_gemm(g, batch, stream);
}

extern "C" int mxa_matmul(const void* a, const void* b, void* c, int64_t batch, int32_t M, int32_t K, int32_t Nc,
                          int64_t a_batch_stride, int64_t b_batch_stride, int32_t elem_mbits_a, int32_t elem_mbits_b,
                          int32_t flush_subnormals, int32_t bfloat, int32_t a_dtype, int32_t b_dtype,
                          int32_t c_dtype, void* workspace, int64_t workspace_bytes, hipStream_t stream) {
  return matmul_impl(a, b, false, c, batch, M, K, Nc, a_batch_stride, b_batch_stride, elem_mbits_a, elem_mbits_b,
                     flush_subnormals, bfloat, a_dtype, b_dtype, c_dtype, workspace, workspace_bytes, stream);
}

extern "C" int mxa_matmul_bt(const void* a, const void* bt, void* c, int64_t batch, int32_t M, int32_t K, int32_t Nc,
                             int64_t a_batch_stride, int64_t bt_batch_stride, int32_t elem_mbits_a, int32_t elem_mbits_b,
                             int32_t flush_subnormals, int32_t bfloat, int32_t a_dtype, int32_t b_dtype,
                             int32_t c_dtype, void* workspace, int64_t workspace_bytes, hipStream_t stream) {
  return matmul_impl(a, bt, true, c, batch, M, K, Nc, a_batch_stride, bt_batch_stride, elem_mbits_a, elem_mbits_b,
                     flush_subnormals, bfloat, a_dtype, b_dtype, c_dtype, workspace, workspace_bytes, stream);
}

extern "C" int mxa_selftest_mfma32(const int8_t* a, const int8_t* b, int32_t* c, hipStream_t stream) {
  if (!a || !b || !c) return MXA_ERR_ARG;
  hipLaunchKernelGGL(selftest_mfma32_kernel, dim3(1), dim3(64), 0, stream, a, b, c);
  return launch_status();
}

extern "C" int mxa_selftest_mfma(const int8_t* a, const int8_t* b, int32_t* c, hipStream_t stream) {
  if (!a || !b || !c) return MXA_ERR_ARG;
  hipLaunchKernelGGL(selftest_mfma_kernel, dim3(1), dim3(64), 0, stream, a, b, c);
  return launch_status();
}
