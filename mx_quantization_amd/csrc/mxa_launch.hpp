// Host-side launchers shared across the library's translation units (one TU per
// kernel family, so that hipcc compiles them in parallel).
#pragma once
#include <algorithm>
#include <atomic>
#include <type_traits>

#include "mxa_proj_args.hpp"
#include "mxa_rows2.hpp"

namespace mxa {

// what a launcher returns after its launches: did the runtime take them?
inline int launch_status() { return hipGetLastError() == hipSuccess ? MXA_OK : MXA_ERR_LAUNCH; }
inline bool aligned16(const void* ptr) { return (reinterpret_cast<uintptr_t>(ptr) & 15u) == 0; }
// the element widths of include/mxa.h: MXINT8 or MXINT4
inline bool mx_width_ok(int elem_bits) { return elem_bits == 8 || elem_bits == 4; }
// the bfloat settings of include/mxa.h: 0 / 32 (no rounding) or bfloat10 .. bfloat31
inline bool valid_bfloat(int bfloat) { return bfloat == 0 || bfloat == 32 || (bfloat >= 10 && bfloat <= 31); }
// may rows at ptr + i0 * s0 + i1 * s1 + i2 * s2 (elements of dtype) be read in 16-B loads?
inline bool may_load_16B(const void* ptr, int dtype, int64_t s0, int64_t s1, int64_t s2) {
  const int64_t vpe = dtype == MXA_DT_F32 ? 4 : 8;  // elements per 16 B
  return aligned16(ptr) && s0 % vpe == 0 && s1 % vpe == 0 && s2 % vpe == 0;
}

// A cursor over a caller's workspace.  take<T>(count): the typed pointer at the running
// offset, which advances by the bytes rounded up to 256; count 0 takes nothing and gives
// nullptr (a region the call does not need).  A null base only sizes.  A workspace layout is
// one function of a cursor and the shapes: its *_workspace_bytes function runs it on a null
// base (the size is the final offset), the entry point on the caller's pointer.
struct Carver {
  uintptr_t base;
  int64_t off = 0;
  explicit Carver(void* workspace = nullptr) : base(reinterpret_cast<uintptr_t>(workspace)) {}
  template <class T>
  T* take(int64_t count) {
    if (count <= 0) return nullptr;
    T* ptr = base ? reinterpret_cast<T*>(base + (uintptr_t)off) : nullptr;
    off += (count * (int64_t)sizeof(T) + 255) / 256 * 256;
    return ptr;
  }
};
// MXINT8 rows of a (rows x cols) matrix along cols: codes [rows][32 nb], block exponents
// [rows][nb].  mfma_rows: the codes in the MX GEMM's MFMA-ready blocks of 32 whole rows
// (RowsPrepArgs::mfma_rows)
struct MxRows { int8_t* codes; int16_t* exps; };
inline MxRows carve_mx_rows(Carver& ws, int64_t rows, int cols, bool mfma_rows) {
  const int64_t nb = (cols + 31) / 32;
  MxRows r{};
  r.codes = ws.take<int8_t>((mfma_rows ? (rows + 31) / 32 * 32 : rows) * nb * 32);
  r.exps = ws.take<int16_t>(rows * nb);
  return r;
}

// RowsPrepArgs of a float32 row-major matrix (rows x cols, row_stride elements from row to
// row) -> MXINT8 rows along its last axis: codes [rows][32 nb] (mfma_rows: in the MX GEMM's
// MFMA-ready row blocks) and block exponents [rows][nb].  elem_bits 4 (a prepared weight's header width; 0 / 8: MXINT8):
// MXINT4 codes in [-7, 7] and the code unit's exponents es - 2 into the same two arrays (the
// block body's op / sA outputs)
inline RowsPrepArgs flat_rows_prep(const void* x, int64_t rows, int cols, int64_t row_stride, int flush, int bfloat,
                                   int8_t* codes, int16_t* exps, int mfma_rows, int elem_bits = 0) {
  RowsPrepArgs r{};
  r.x = x; r.s0 = 0; r.s1 = 0; r.s2 = row_stride;
  r.H = 1; r.R = rows; r.rows = rows; r.D = cols; r.nb = (cols + 31) / 32; r.dpad = 32 * r.nb;
  r.vec4 = may_load_16B(x, MXA_DT_F32, 0, 0, row_stride);
  r.op_kind = MXA_OP_MXINT8; r.flush = flush; r.bfloat = bfloat; r.dt = MXA_DT_F32;
  r.codes = codes; r.sT = exps; r.mfma_rows = mfma_rows;
  if (elem_bits == 4) {
    r.op_kind = MXA_OP_MXINT4;
    r.codes = nullptr; r.sT = nullptr; r.op = codes; r.sA = exps;
  }
  return r;
}

// rows of 513 .. 1,024 keys (the *_long entry points of include/mxa.h): the selection runs one
// wave per query row (mxa_select_long.hpp) and the 16-row finishing kernel reads the kept keys
// from the workspace instead of staging the head's K table (mxa_finish16.hpp)
constexpr int kShortRowsT = 512, kLongRowsT = 1024;
inline bool long_rows(int T) { return T > kShortRowsT; }
// The side lane of a forked attention call (mxa_attn.hip, SideFork): the library's own stream beside the
// caller's, joined before the finishing kernel.  `packed`: the event launch_select records behind the
// packed pass
struct SideLane { hipStream_t stream; hipEvent_t packed; };
// selection kernel (mxa_sel.hip); plan: only check the LDS budget, launch nothing
// side (nullable; given only where the packed pass runs with its tail, sel_tail_width == kTailPref): the
// lane is forked behind the packed pass -- it waits for `packed` -- so that the caller's launches on
// it run beside the tail
int launch_select(const Rows2Args& ra, int mode, int BH, hipStream_t stream, bool plan, const SideLane* side = nullptr);
// ... for long rows (mxa_sel_long.hip)
int launch_select_long(const Rows2Args& ra, int mode, int BH, hipStream_t stream, bool plan);
// the one-lane tail's prefix (measured, DeiT-base: 48 positions 0.575-0.583 ms against 0.585-0.599
// for 64 -- 12 KB of LDS per wave, 3 waves per SIMD instead of 2, outweighs the selection kernel's
// extra step -- and 0.573-0.584 for 56; a 32-position prefix is slower: the selection kernel then
// runs one more lockstep step per row).  Measured again with the tail's block stores
// (profiles/ab_tail_blocks.txt, libraries ld0 / p56l0 / p64l0, select stage of four alternating
// runs): 48 positions 0.502-0.506 ms, 56 0.510-0.512, 64 0.519-0.520 -- the tail still pays for
// record size (its LDS per wave sets the waves per SIMD), so 48 stays.  MXA_TAIL_PREF: a
// tools-only build of another width for same-box A/Bs (build_native defines)
#ifndef MXA_TAIL_PREF
#define MXA_TAIL_PREF 48
#endif
constexpr int kTailPref = MXA_TAIL_PREF;
// the selection's packed pass: rows of <= 256 keys, the approximators whose scores pack
// (sums of a few small integers times powers of two), no bias (a bias of -10000 next to
// small scores needs the key's low byte: PixArt's masked cross-attention would fall back
// for every row)
inline bool sel_packs(int mode, int T, bool bias) {
  return !bias && T <= 256 && (mode == kModeExSign || mode == kModeOpExp || mode == kModeOpMul || mode == kModeTrueEx);
}
// the prefix the one-lane tail takes over (mxa_tail.hpp), 0 = none: k + 2 <= TW (the
// introselect's last range and the sort of [0, k-1) lie in it), not partial_sort (k*64 <= T)
// (k - 1 <= 32: the final stable rank of [0, k-1) in at most 32 registers per lane; k + ntw
// <= TW: the prune-mask words are set in the prefix's free positions)
inline int tail_width_for(int n, int k) {
  if (k <= 0 || k > 33 || (int64_t)k * 64 <= n) return 0;
  return k + 2 <= kTailPref && k + (n + 31) / 32 <= kTailPref ? kTailPref : 0;
}
inline int sel_tail_width(int mode, int T, int k, bool bias) { return sel_packs(mode, T, bias) ? tail_width_for(T, k) : 0; }

// one score mode per translation unit of mxa_sel.hip (MXA_SEL_PART 1..6)
int launch_select_p1(const Rows2Args& ra, int BH, hipStream_t stream, bool plan, const SideLane* side);  // ex_pred
int launch_select_p2(const Rows2Args& ra, int BH, hipStream_t stream, bool plan, const SideLane* side);  // EXION
int launch_select_p3(const Rows2Args& ra, int BH, hipStream_t stream, bool plan, const SideLane* side);  // MXINT4 / partial
int launch_select_p4(const Rows2Args& ra, int BH, hipStream_t stream, bool plan, const SideLane* side);  // true_ex
int launch_select_p5(const Rows2Args& ra, int BH, hipStream_t stream, bool plan, const SideLane* side);  // ELSA
int launch_select_p6(const Rows2Args& ra, int BH, hipStream_t stream, bool plan, const SideLane* side);  // the true scores
inline int launch_select_mode(const Rows2Args& ra, int mode, int BH, hipStream_t stream, bool plan, const SideLane* side) {
  switch (mode) {
    case kModeExSign: return launch_select_p1(ra, BH, stream, plan, side);
    case kModeOpMul: return launch_select_p2(ra, BH, stream, plan, side);
    case kModeOpExp: return launch_select_p3(ra, BH, stream, plan, side);
    case kModeTrueEx: return launch_select_p4(ra, BH, stream, plan, side);
    case kModeElsa: return launch_select_p5(ra, BH, stream, plan, side);
    default: return launch_select_p6(ra, BH, stream, plan, side);
  }
}
// ---- the finishing kernel of a call: the one decision -------------------------------------
// attn_validate, attn_layout, launch_rows and the *_finish_kernel entry points all read
// finish_choice of the same facts; nothing else asks which kernel runs.
// (MXA_FQ_KMIN: a tools-only build of the MFMA kernel's threshold for same-box A/Bs, build_native defines)
#ifndef MXA_FQ_KMIN
#define MXA_FQ_KMIN 65
#endif
// topk, k (0 on the dense branch), xo: the finishing kernel writes the proj Linear's MX input codes
// (the call's `direct`, known before any pointer is bound); xdt: float16 / bfloat16 inputs or scores;
// bits: 8 or 4, P's element width; full: the entry point reaches finish_qk_long_kernel (mxa_attention_full);
// block: it reaches the fused projections on rows over 512 keys too (the *_full fused blocks), where xo is
// the LONG 16-row kernel's: MXINT8, k <= 32
struct FinFacts { bool topk; int k, T, nbd; bool xo, xdt; int bits; bool full; bool block = false; };
// kind: MXA_FIN_* (include/mxa.h); reads_mask: the kernel reads the selection's prune-mask words (the
// caller's mask_out, else a workspace copy), not the kept indices; status: MXA_ERR_UNSUPPORTED where the
// kind has no instantiation for the facts
struct FinChoice { int kind; bool reads_mask; int status; };
inline FinChoice finish_choice(const FinFacts& f) {
  const bool lng = long_rows(f.T), w4 = f.bits == 4, regs = f.T <= 256 && f.nbd <= 4;  // regs: a row's scores in registers
  FinChoice c{};
  if (f.full && lng && (!f.topk || f.k > 64))  // the tiled MFMA kernel (mxa_finish_qk_long.hpp)
    c.kind = f.topk ? MXA_FIN_MFMA_LONG : MXA_FIN_DENSE_MFMA_LONG;
  else if (!f.topk)  // the dense branch: finish_qk_kernel with every key kept, else the v_dot4 row kernel
    c.kind = regs ? MXA_FIN_DENSE_MFMA : MXA_FIN_DENSE_ROWS;
  else if (f.k >= MXA_FQ_KMIN && regs && !f.xo)  // k a large share of T (mxa_finish_qk.hpp)
    c.kind = MXA_FIN_MFMA;
  else  // k <= 64 (DeiT's 20 / 30, PixArt's 20; with the proj's codes: k <= 32): 16-row tiles, else 32-row
    c.kind = f.k <= (f.xo ? 32 : 64) ? MXA_FIN_GATHER16 : MXA_FIN_GATHER32;
  c.reads_mask = c.kind == MXA_FIN_MFMA || c.kind == MXA_FIN_MFMA_LONG;
  // long rows and MXINT4 P: float32 without the proj's codes (but the fused blocks' on the LONG 16-row
  // kernel at MXINT8), and not on the 32-row or the dense row kernel (a K table of <= 512 keys, MXINT8 P only)
  const bool lxo = f.block && lng && !w4 && c.kind == MXA_FIN_GATHER16;
  if ((lng || w4) && (f.xdt || (f.xo && !lxo) || c.kind == MXA_FIN_GATHER32 || c.kind == MXA_FIN_DENSE_ROWS))
    c.status = MXA_ERR_UNSUPPORTED;
  return c;
}

// ---- what the three finishing kernels' launches share (mxa_fin.hip, mxa_fin16.hip,
// mxa_fin_qk.hip): tiles of tile_rows query rows, one tile per wave at a time --------------
// Waves per workgroup and query rows per workgroup.  lds(w): the LDS bytes of a workgroup
// of w waves; wave_cap: the waves per CU the kernel's registers allow.  A head's tiles
// round-robin over the waves of one workgroup (the K / V tables staged once per head); few
// heads (PixArt cross-attention): the tiles split over grid.y so that the grid still has ~2
// workgroups per CU.  Waves per workgroup: the fewest sequential tile rounds per CU --
// workgroups per CU over the concurrency the LDS and the registers allow, times each
// workgroup's rounds over its tiles; ties to the smaller workgroup (measured on the 32-row
// kernel, wave_cap 12: DeiT-base 4 waves, 2 workgroups per CU, 0.29 ms vs 0.36 ms with 5;
// DiT 8 waves, 0.36 ms vs 0.61 ms with 4).  MXA_ERR_UNSUPPORTED: one wave does not fit
// the 160 KB.
template <class LdsFn>
inline int finish_tile_plan(int tile_rows, int N, int BH, LdsFn lds, int wave_cap, int* waves, int* rows_per_wg) {
  const int tiles = (N + tile_rows - 1) / tile_rows;
  if (lds(1) > 160 * 1024) return MXA_ERR_UNSUPPORTED;
  int chunks = 1;
  while ((int64_t)BH * chunks < 512 && chunks < tiles) ++chunks;
  const int tpc = (tiles + chunks - 1) / chunks;
  const int64_t wgs_per_cu = ((int64_t)BH * chunks + 255) / 256;
  int w = 1;
  int64_t best = -1;
  for (int c = 1; c <= std::min(8, tpc); ++c) {
    const size_t t = lds(c);
    if (t > 160 * 1024) break;
    const int64_t conc = std::max<int64_t>(1, std::min<int64_t>(160 * 1024 / t, wave_cap / c));
    const int64_t score = (wgs_per_cu + conc - 1) / conc * ((tpc + c - 1) / c);
    if (best < 0 || score < best) best = score, w = c;
  }
  *waves = w;
  *rows_per_wg = tile_rows * tpc;
  return MXA_OK;
}
// the wave cap of a kernel whose registers allow wps waves per SIMD (plan = true, before any
// code object is looked at: 2)
inline int finish_wave_cap(int wps) { return 4 * std::max(1, std::min(8, wps)); }
// waves per SIMD the kernel's registers allow: a property of the code object (gfx950
// only), cached per kernel function; concurrent first launches compute the same value
template <auto Kernel>
inline int kernel_waves_per_simd() {
  static std::atomic<int> cached{0};
  int wps = cached.load(std::memory_order_relaxed);
  if (!wps) {
    hipFuncAttributes fa{};
    wps = hipFuncGetAttributes(&fa, reinterpret_cast<const void*>(Kernel)) == hipSuccess && fa.numRegs > 0
              ? 512 / ((fa.numRegs + 7) / 8 * 8) : 2;
    cached.store(wps, std::memory_order_relaxed);
  }
  return wps;
}
// the launch of a planned finishing kernel (ra.waves, ra.rows_per_wg) with lds bytes of LDS
template <auto Kernel>
inline int launch_finish_tiles(const Rows2Args& ra, int BH, size_t lds, hipStream_t stream) {
  if (hipFuncSetAttribute(reinterpret_cast<const void*>(Kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) !=
      hipSuccess)
    return MXA_ERR_LAUNCH;
  const unsigned gy = (unsigned)((ra.N + ra.rows_per_wg - 1) / ra.rows_per_wg);
  hipLaunchKernelGGL(Kernel, dim3((unsigned)BH, gy), dim3(64 * ra.waves), lds, stream, ra);
  return launch_status();
}

// ---- what the two MFMA finishing kernels' launches share (mxa_fin_qk.hip, mxa_fin_qkl.hip) ----
// their plan: tiles of tile_rows query rows, lds bytes of LDS per workgroup and none per wave
inline int finish_mfma_plan(const Rows2Args& ra, int tile_rows, size_t lds, int BH, int regs_waves_per_simd, int* waves,
                            int* rows_per_wg) {
  return finish_tile_plan(tile_rows, ra.N, BH, [lds](int) { return lds; }, finish_wave_cap(regs_waves_per_simd), waves,
                          rows_per_wg);
}
// their EXTRA instantiations: a bias, the debug true scores or bfloatX rounding
inline bool finish_mfma_extra(const Rows2Args& ra) { return ra.bias || ra.true_out || (ra.bfloat != 0 && ra.bfloat != 32); }
// one instantiation planned by its own registers, then launched
template <auto Kernel>
inline int launch_finish_mfma(Rows2Args ra, int tile_rows, size_t lds, int BH, hipStream_t stream) {
  const int rc = finish_mfma_plan(ra, tile_rows, lds, BH, kernel_waves_per_simd<Kernel>(), &ra.waves, &ra.rows_per_wg);
  return rc ? rc : launch_finish_tiles<Kernel>(ra, BH, lds, stream);
}
// fn(std::integral_constant<int, NB>) for the NB = nbd blocks per head dim (1..4)
template <class Fn>
inline int dispatch_nbd(int nbd, Fn fn) {
  switch (nbd) {
    case 1: return fn(std::integral_constant<int, 1>{});
    case 2: return fn(std::integral_constant<int, 2>{});
    case 3: return fn(std::integral_constant<int, 3>{});
    default: return fn(std::integral_constant<int, 4>{});
  }
}

// the MFMA finishing kernel's launches (mxa_fin_qk.hip): float32 inputs and scores (x0), float16 / bfloat16 (x1)
int launch_finish_qk_x0(const Rows2Args& ra, int BH, hipStream_t stream, bool plan);
int launch_finish_qk_x1(const Rows2Args& ra, int BH, hipStream_t stream, bool plan);
int launch_finish_qk_x0w4(const Rows2Args& ra, int BH, hipStream_t stream, bool plan);  // float32, MXINT4 P
// its tiled sibling for rows of 513 .. 1,024 keys (mxa_fin_qkl.hip): float32, MXINT8 / MXINT4 P
int launch_finish_qk_long_w8(const Rows2Args& ra, int BH, hipStream_t stream, bool plan);
int launch_finish_qk_long_w4(const Rows2Args& ra, int BH, hipStream_t stream, bool plan);
// the 16-row finishing kernel (mxa_fin16.hip): float32 (x0), float16 / bfloat16 (x1)
int launch_finish16_x0(const Rows2Args& ra, int BH, hipStream_t stream, bool plan);
int launch_finish16_x1(const Rows2Args& ra, int BH, hipStream_t stream, bool plan);
int launch_finish16_l0(const Rows2Args& ra, int BH, hipStream_t stream, bool plan);  // long rows, float32
int launch_finish16_x0w4(const Rows2Args& ra, int BH, hipStream_t stream, bool plan);  // float32, MXINT4 P
int launch_finish16_l0w4(const Rows2Args& ra, int BH, hipStream_t stream, bool plan);  // ... on long rows
int launch_finish16_l0xo(const Rows2Args& ra, int BH, hipStream_t stream, bool plan);  // long rows, the proj's codes
// the 32-row finishing kernel for NB blocks per head dim (mxa_fin.hip parts 1..4)
int launch_finish32_p1(const Rows2Args& ra, int BH, hipStream_t stream, bool plan);
int launch_finish32_p2(const Rows2Args& ra, int BH, hipStream_t stream, bool plan);
int launch_finish32_p3(const Rows2Args& ra, int BH, hipStream_t stream, bool plan);
int launch_finish32_p4(const Rows2Args& ra, int BH, hipStream_t stream, bool plan);
// the row kernel finish_choice(f) names (mxa_fin.hip); true_mode: the selection kernel ranked, and
// wrote, the true scores; plan: f.xo stands for the proj's code pointers, which are not bound yet
int launch_rows(const Rows2Args& ra, const FinFacts& f, bool true_mode, int S, int BH, hipStream_t stream, bool plan);
// fused projection kernel (mxa_proj.hip): part 0 the self-attention q, k, v of one token
// matrix, 1 / 2 cross-attention's q and k, v passes (mxa_proj.hpp ProjPart)
int launch_proj(const ProjArgs& pa, hipStream_t stream, int part = 0);
// ... at MXINT4 (mxa_proj4.hip): pa.xc / pa.xs MXINT4 rows, the weight a 4-bit one (pd one plane)
int launch_proj4(const ProjArgs& pa, hipStream_t stream, int part);
// does the prepared weight at wq carry this header?  Buffers prepared in this process
// are looked up host-side; others have their header read once (not under stream capture)
// (elem_bits: the header's field -- 0 an MXINT8 weight, 4 an MXINT4 one; the attention entry
// points ask for 0, so they refuse a 4-bit weight)
LinearWeightHeader linear_weight_header(int out_f, int in_f, int gw, int flush, int bfloat, int elem_bits = 0);
bool linear_weight_verify(const void* wq, const LinearWeightHeader& want, hipStream_t stream);

// does the prepared weight carry (out_f, in_f, flush, bfloat), whatever its group width?
// elem_bits null: an MXINT8 weight only; else the weight's own width (0 or 4) is accepted and
// returned
bool linear_weight_verify_any_group(const void* wq, int out_f, int in_f, int flush, int bfloat, hipStream_t stream,
                                    int* elem_bits = nullptr);
// the header of a prepared weight this process has seen (verified or prepared)
bool linear_weight_known_header(const void* wq, LinearWeightHeader* h);
// the largest row + column exponent spread whose shifted int32 block sums stay exact over
// nbk K-blocks: nbk * 32 * 127^2 * 2^smax < 2^31 (mxa_gemm.hip)
int gemm_smax(int nbk);
// block-scaled MX GEMM (mxa_gemm.hip); mx.Linear on MX rows with a prepared weight
// (slow: gemm_slow_bytes of device scratch for the list of waves the fp64 kernel takes)
// bits4: the operands are MXINT4 and ga.bpd, where set, is a 4-bit weight's one digit plane
// (mx_gemm_dig4_kernel; the tile kernel takes the codes as they are)
int launch_gemm(const GemmArgs& ga, int64_t batch, hipStream_t stream, bool bits4 = false);
// the GemmArgs launch_linear_codes launches (bpd set: the weight's digits cover the output
// columns); *bits4: the weight's header says MXINT4 (the rows must be MXINT4 too)
GemmArgs linear_gemm_args(const int8_t* xc, const int16_t* xs, int64_t rows, int in_f, const void* wq, int out_f,
                          const float* bias, float* out, int64_t out_row_stride, int bfloat, int autocast, bool x_mfma,
                          bool* bits4 = nullptr);
int launch_linear_codes(const int8_t* xc, const int16_t* xs, int64_t rows, int in_f, const void* wq, int out_f,
                        const float* bias, float* out, int64_t out_row_stride, int bfloat, int autocast,
                        hipStream_t stream, bool x_mfma);

}  // namespace mxa
