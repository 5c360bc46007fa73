"""What the test files share on the device's side of a comparison: moving arrays to and from
the GPU, the two equalities, the tolerance checks, the golden directory, the package fixture,
and the attention op's harness: attn_run (the op to host arrays), check_attn (its scores,
indices and mask against a reference), attn_entry (one C entry point called directly),
check_siblings (every entry point that accepts a call against mxa_attention_full and the op), rnd,
host_params and the RCase tables' r_scale / r_kw.  Imported like the *_cases.py modules (`from gpu_support import M  # noqa: F401`
brings the fixture into a test file); it imports without a GPU -- torch.cuda is touched only
inside dev / from_bits -- so the CPU tests use same, same_bits and load from here too.

same is value equality (-0.0 equals +0.0), same_bits compares bit patterns (it does not): a
call site keeps the one it has."""
import os

import numpy as np
import pytest
import torch

from oracle import mx_oracle as O

G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
OUT_TOL = 1e-3  # the attention output, normwise relative error
TDT = {"f16": torch.float16, "bf16": torch.bfloat16}
ELEM = {8: "int8", 4: "int4"}  # the ops' elem_bits -> the oracle's elem


@pytest.fixture(scope="module")
def M():
    import mx_quantization_amd as m
    return m


def load(name):
    return np.load(os.path.join(G, name))


def rnd(shape, seed, mult=1.0):
    return (np.random.default_rng(seed).standard_normal(shape, dtype=np.float32) * np.float32(mult)).astype(np.float32)


def host_params(nat, B, H, Nq, T, D, k, mode="ex_pred", top_k=1):
    """AttnParams for the entry points' host logic: non-null placeholders, nothing is launched"""
    p = nat.AttnParams()
    p.q = p.k = p.v = p.out = 16
    p.elsa_proj = 16
    p.B, p.H, p.N, p.T, p.D, p.k_top = B, H, Nq, T, D, k
    p.pred_mode, p.top_k, p.approx, p.scale = nat.PRED_MODES[mode], top_k, 1, 0.125
    return p


# ---- the RCase tables (attn4_cases.py, long_dense_cases.py): k = 0 dense, mode None approx=False ----
def r_scale(c):
    return float(np.float32(c.D ** -0.5))


def r_kw(c):
    kw = dict(k_top=c.k) if c.k else dict(top_k=False)
    if c.k and c.mode is None:
        kw["approx"] = False
    elif c.k:
        kw["pred_mode"] = c.mode
    return kw


def dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def dev_opt(x):
    """dev for an optional tensor (a bias)"""
    return None if x is None else dev(x)


def host(t, f32=False):
    """f32: converted to float32 on the device first (a 16-bit tensor has no numpy dtype)"""
    t = t.detach()
    return (t.float() if f32 else t).cpu().numpy()


def from_bits(u16, dt):
    """uint16 bit patterns of the dtype ("f16" / "bf16") -> a device tensor of it"""
    return torch.from_numpy(np.ascontiguousarray(u16).view(np.int16)).view(TDT[dt]).cuda()


def to_f32(u16, dt):
    """uint16 bit patterns of the dtype -> float32 values (exact)"""
    return torch.from_numpy(np.ascontiguousarray(u16).view(np.int16)).view(TDT[dt]).float().numpy()


def to_bits(t):
    """device tensor -> float32 array, or the uint16 patterns of a 16-bit tensor"""
    if t.dtype == torch.float32:
        return host(t)
    return host(t.contiguous().view(torch.int16)).view(np.uint16)


def same(a, b, what="", signed=False):
    """Equal values, NaN against NaN allowed; signed: the zeros' signs too."""
    a, b = np.asarray(a), np.asarray(b)
    assert a.shape == b.shape, (what, a.shape, b.shape)
    ok = (a == b) | (np.isnan(a) & np.isnan(b)) if a.dtype.kind == "f" else a == b
    if signed:
        ok &= (np.signbit(a) == np.signbit(b)) | np.isnan(a)
    if not ok.all():
        bad = np.argwhere(~ok)
        raise AssertionError(f"{what}: {bad.shape[0]}/{ok.size} mismatches, first {bad[:4].tolist()}: "
                             f"{a[tuple(bad[0])]} vs {b[tuple(bad[0])]}")


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def same_bits(got, ref, what="", dt=None, x=None, patterns=False):
    """Equal bit patterns (-0.0 is not +0.0); a NaN on both sides counts as equal, nothing else
    is left out.  Both sides are taken as float32 values.  patterns: uint32 arrays, and uint16
    ones of the 16-bit dtype dt, are bit patterns already and a float32 array is viewed as
    such; the two dtypes must agree.  x: the inputs' patterns, quoted beside a mismatch."""
    if patterns:
        g, r = _bits(got), _bits(ref)
        assert g.dtype == r.dtype, (what, g.dtype, r.dtype)
    else:
        g, r = _bits(np.asarray(got, dtype=np.float32)), _bits(np.asarray(ref, dtype=np.float32))
    assert g.shape == r.shape, (what, g.shape, r.shape)
    if g.dtype == np.uint32:
        inf, mag = 0x7F800000, 0x7FFFFFFF
    else:
        inf, mag = {"f16": 0x7C00, "bf16": 0x7F80}[dt], 0x7FFF
    ok = (g == r) | (((g & mag) > inf) & ((r & mag) > inf))
    if not ok.all():
        bad = np.argwhere(~ok)
        first = []
        for i in map(tuple, bad[:4]):
            src = "" if x is None or np.shape(x) != g.shape else f" x={int(_bits(x)[i]):#x}"
            first.append(f"{list(i)}:{src} got {int(g[i]):#x} want {int(r[i]):#x}")
        raise AssertionError(f"{what}: {bad.shape[0]}/{ok.size} mismatches; " + "; ".join(first))


def out_close(got, ref, tol, what):
    """the NaN pattern bit-exact, the finite elements within tol normwise"""
    same(np.isnan(got), np.isnan(ref), what + " NaN pattern")
    fin = ~np.isnan(ref)
    g, r = got[fin].astype(np.float64), ref[fin].astype(np.float64)
    err = np.linalg.norm(g - r) / max(np.linalg.norm(r), 1e-30)  # (0 when nothing is finite)
    assert err <= tol, f"{what}: normwise error {err:.3e} > {tol}"


# ---- the row-wise bound on the attention output ("The attention output") ----
ELIGIBLE_ELEMS, ELIGIBLE_ROWS = 0.005, 0.15  # the largest eligible shares a test may have
EXACT_GAP = 150.0  # a kept score this far below the row's maximum has p = 0 on both sides
TAU_C0 = 5.5  # ulps: exp on the device 1, numpy's exp 3, the quotients 1 (device) and 1/2 (numpy)


def ref_chain(n):
    """the longest chain of float32 additions in numpy's sum of n contiguous terms: in order
    below 8; else 8 accumulators over blocks of at most 128 (16 each), 3 to combine them, one
    per level of the pairwise recursion above 128"""
    return n - 1 if n < 8 else -(-min(n, 128) // 8) + 3 + max(0, int(np.ceil(np.log2(n / 128))))


def finish_kernel_of(T, D, k):
    """mxa_launch.hpp finish_choice for a float32 call without proj codes; k = 0: dense"""
    mfma = T <= 256 and (D + 31) // 32 <= 4
    if not k:
        return "dense_qk" if mfma else "dense_rows"
    return "qk" if k >= 65 and mfma else ("fin16" if k <= 64 else "fin32")


def n_add_and_chain(kernel, T, k):
    """(fp32 additions per output element, longest chain of fp32 additions in the row sum) of a
    finishing kernel, read from its code.  The three MFMA kernels add one fmaf of an exact int32
    block sum per key block; dense_rows_kernel accumulates in fp64 and converts once.  Row sums:
    finish16_kernel its KS slots per lane (mxa_fin16.hip: 5 / 8 / 12 / 16 for ceil(k / 4)) and two
    quad steps; finish_kernel KS slots (mxa_fin.hip: 8 / 16 / 32 for ceil(k / 16)) and the four
    steps of a 16-lane reduction; finish_qk_kernel 8 keys of every block per lane and two
    steps; dense_rows_kernel ceil(T / 64) per lane and the six steps of a wave reduction."""
    ntb = (T + 31) // 32
    if kernel == "fin16":
        return ntb, min(s for s in (5, 8, 12, 16) if 4 * s >= k) + 2
    if kernel == "fin32":
        return ntb, min(s for s in (8, 16, 32) if 16 * s >= k) + 4
    return {"qk": (ntb, 8 * ntb + 2), "dense_qk": (ntb, 8 * ntb + 2), "dense_rows": (1, (T + 63) // 64 + 6)}[kernel]


def out_row_bound(r, v, kernel=None, bits=8):
    """From the oracle's result r (true, attn, out; idx on the top-k path) and v alone: the
    elementwise bound A + F on |got - r["out"]| of the kernel that runs the call, the finite
    rows, the eligible shares (elements, rows), the kernel's name and the eligible set.
    A = (n_add + 1) 2^-24 |Pq| @ |Vq| is the accumulation; F = sum over the eligible kept
    elements of one code step 2^(eP - 6) |Vq| (MXINT4 P and V, bits = 4: 2^(eP - 2)): the elements whose p lies within a relative tau
    of a rounding tie of its block's code grid, and every non-zero element of a block whose
    maximum lies within 2 tau of a binade boundary.  tau_j = (TAU_C0 + (chain + ref_chain) / 2 +
    2 |x_j - max|) 2^-23 (an addition rounds by half an ulp).  A row whose kept scores all
    equal the maximum or lie EXACT_GAP below it has no eligible element: its p are 1/m,
    correctly rounded, on both sides.  At 4 bits a rounding tie at y >= 7 (between the codes 7
    and 8) is no tie: both sides clip to 7."""
    elem, (unit, top) = ELEM[bits], (2, 4) if bits == 4 else (6, 64)  # the code unit's exponent, the top binade's first code
    attn, true = np.asarray(r["attn"], np.float64), np.asarray(r["true"], np.float64)
    T, D = attn.shape[-1], v.shape[-1]
    k = r["idx"].shape[-1] if "idx" in r else 0
    kernel = kernel or finish_kernel_of(T, D, k)
    assert bits == 8 or kernel in ("fin16", "qk", "dense_qk"), kernel  # the kernels with an MXINT4-P form
    n_add, chain = n_add_and_chain(kernel, T, k)
    kept = O.prune_mask(r["idx"], T) if k else np.ones(attn.shape, bool)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        pq, _, pe = O.quantize_mx(r["attn"], elem, 32, -1)
        vq = np.abs(O.quantize_mx(np.asarray(v, np.float32), elem, 32, -2)[0].astype(np.float64))
        S = np.matmul(np.abs(pq.astype(np.float64)), vq)
        fin = np.isfinite(attn).all(-1) & np.isfinite(r["out"]).all(-1) & np.isfinite(S).all(-1)
        gap = np.where(kept, np.abs(true - np.max(np.where(kept, true, -np.inf), -1, keepdims=True)), np.inf)
        gap = np.where(fin[..., None], gap, np.inf)
        loose = ((gap > 0) & (gap < EXACT_GAP)).any(-1, keepdims=True)  # (else the row is exact)
        tau = (TAU_C0 + (chain + ref_chain(k or T)) / 2 + 2.0 * gap) * 2.0 ** -23
        pb, _ = O.to_blocks(r["attn"], -1, 32)
        pb = pb.astype(np.float64)
        tb = O.to_blocks(np.where(np.isfinite(tau), tau, 0).astype(np.float32), -1, 32)[0].astype(np.float64)
        live = O.to_blocks((kept & loose & fin[..., None] & (attn > 0)).astype(np.float32), -1, 32)[0] > 0
        step = np.exp2(pe.astype(np.float64) - unit)  # (..., nb, 1): one code step of the block
        y = pb / step
        tie = np.abs(y - np.floor(y) - 0.5) <= tb * y
        if bits == 4:
            tie &= np.floor(y) < 7
        pmax = pb.max(-1, keepdims=True)
        tmax = np.take_along_axis(tb, pb.argmax(-1)[..., None], -1)
        mant = pmax / (top * step)  # in [1, 2)
        edge = (mant * (1 - 2 * tmax) < 1) | (mant * (1 + 2 * tmax) >= 2)
        elig = live & (tie | edge)
        F = np.matmul(O.from_blocks(np.where(elig, step, 0.0), T, -1), np.where(np.isfinite(vq), vq, 0.0))
    shares = (elig.sum() / max(1, (kept & fin[..., None]).sum()), elig.any((-1, -2))[fin].mean() if fin.any() else 0.0)
    return (n_add + 1) * 2.0 ** -24 * S + F, fin, shares, kernel, O.from_blocks(elig, T, -1)


def out_rows_close(got, r, v, what, kernel=None, bits=8):
    """The attention output of a float32 call with bfloat 0 / 32 against the oracle's at that width
    (O.attention(elem=ELEM[bits])), row by row: |got - ref| <= A + F elementwise on the finite rows (out_row_bound), the NaN pattern
    equal everywhere.  The eligible shares are asserted first, from the oracle alone.  Prints
    the kernel, the shares and the worst ratio; on failure its row and column."""
    bound, fin, (se, sr), kernel, _ = out_row_bound(r, v, kernel, bits)
    assert se <= ELIGIBLE_ELEMS and sr <= ELIGIBLE_ROWS, f"{what}: eligible elements {se:.4%}, rows {sr:.2%}"
    ref = np.asarray(r["out"])
    same(np.isnan(got), np.isnan(ref), what + " NaN pattern")
    err = np.abs(got[fin].astype(np.float64) - ref[fin].astype(np.float64))
    b = bound[fin]
    ratio = np.where(err == 0, 0.0, err / np.where(b > 0, b, 1e-300))
    worst = float(ratio.max()) if ratio.size else 0.0
    print(f"out_rows_close {what}: {kernel} w{bits}, eligible elements {se:.4%} rows {sr:.2%}, worst |got - ref| / (A + F) {worst:.3f}")
    if worst > 1:
        i = np.unravel_index(np.argmax(ratio), ratio.shape)
        row = np.argwhere(fin)[i[0]].tolist()
        raise AssertionError(f"{what}: |got - ref| / (A + F) = {worst:.3f} at row {row} column {i[1]}: "
                             f"got {got[fin][i]!r} want {ref[fin][i]!r} bound {b[i]:.3e}")


# ---- the attention op: run it, compare it, call one entry point directly -------------------------
def attn_run(M, q, k, v, scale, bits=8, scores=True, **kw):
    """M.mx_topk_attention at width bits on host arrays or device tensors (the keywords' arrays
    too) -> dict of host arrays: out; idx and mask (as bools) on the top-k path; true and pred
    with scores"""
    topk = kw.get("top_k", True)
    q, k, v = (dev(x) if isinstance(x, np.ndarray) else x for x in (q, k, v))
    kw = {a: (dev(x) if isinstance(x, np.ndarray) else x) for a, x in kw.items()}
    res = M.mx_topk_attention(q, k, v, scale, return_scores=scores, return_mask=topk, elem_bits=bits, **kw)
    torch.cuda.synchronize()
    got = dict(out=host(res[0]))
    if topk:
        got.update(idx=host(res[1]), mask=host(M.unpack_mask(res[-1], k.shape[-2])))
    else:
        assert res[1] is None
    if scores:
        got.update(true=host(res[2]), pred=host(res[3]))
    return got


def check_attn(got, ref, what, cmp=same):
    """attn_run's result against the oracle's (or the reference's) true, pred (absent with approx
    off or on the dense branch) and idx: the scores by cmp (same / same_bits), where the call took
    them; the kept indices and the prune mask equal; no idx on the dense branch"""
    if "true" in got:
        cmp(got["true"], ref["true"], what + " true")
        if "pred" in ref:
            cmp(got["pred"], ref["pred"], what + " pred")
    if "idx" in ref:
        idx = np.asarray(ref["idx"]).astype(np.int64)
        same(got["idx"], idx, what + " idx")
        same(got["mask"], O.prune_mask(idx, ref["true"].shape[-1]), what + " mask")
    else:
        assert "idx" not in got


def check_exact_out(M, c, inputs, r, scale, bits, what):
    """An exact-result case (exact_out_cases.Case) at width bits: idx, mask and true equal, out bit
    for bit; without and with the scores (the plain and the EXTRA instantiations; a bias or
    bfloat: EXTRA both times)"""
    q, kk, v, bias = inputs
    kw = dict(c.kw)
    kw.update(dict(k_top=c.k) if c.k else dict(top_k=False))
    for scores in (False, True):
        got = attn_run(M, q, kk, v, scale, bits, scores, bias=dev_opt(bias), **kw)
        w = f"{what} w{bits} scores={scores}"
        if c.k:
            same(got["idx"], r["idx"], w + " idx")
            same(got["mask"], O.prune_mask(r["idx"], c.T), w + " mask")
        if scores:
            same(got["true"], r["true"], w + " true")
        same_bits(got["out"], r["out"], w + " out")


ENTRY_SIZES = {"mxa_attention": "mxa_attention_workspace_bytes", "mxa_attention_long": "mxa_attention_long_workspace_bytes",
               "mxa_attention_bits": "mxa_attention_bits_workspace_bytes", "mxa_attention_full": "mxa_attention_full_workspace_bytes",
               "mxa_approx_scores": "mxa_attention_workspace_bytes", "mxa_approx_scores_long": "mxa_attention_long_workspace_bytes",
               "mxa_approx_scores_bits": "mxa_attention_bits_workspace_bytes"}


def attn_entry(M, name, q, k, v, scale, bits=None, take=("idx", "mask", "scores"), idx=None, **kw):
    """The C entry point `name` (a key of ENTRY_SIZES) called directly on device tensors, on the
    workspace its own size function asks for; bits: the width argument of the *_bits / *_full
    entry points.  kw: k_top (20), top_k, pred_mode, approx, bias.  take: the outputs bound beside
    out -- "idx" (idx: a caller's int64 buffer in its place), "mask" (the words), "scores" (true
    and pred); an output not taken stays null, and idx and mask exist on the top-k path only.  An
    mxa_approx_scores* entry point gets mx_approx_scores' parameters (v and scale unused) and binds
    pred alone.  Returns the device tensors by name, NaN-filled before the call."""
    ops, lib = M.ops, M._native.lib()
    kt, topk, mode = kw.pop("k_top", 20), kw.pop("top_k", True), kw.pop("pred_mode", "ex_pred")
    approx, bias = kw.pop("approx", True), kw.pop("bias", None)
    assert not kw, kw
    nan = lambda *shape: torch.full(shape, float("nan"), dtype=torch.float32, device=q.device)
    res = {}
    if "approx_scores" in name:
        p, dv, (B, H, Nq, T, D), keep = ops._attn_params(q, k, None, 1.0, 0, mode, False, True, bias, False, 0, None)
        res["pred"] = nan(B, H, Nq, T)
    else:
        p, dv, (B, H, Nq, T, D), keep = ops._attn_params(q, k, v, scale, kt, mode, topk, approx and topk, bias, False, 0, None)
        res["out"] = ops._bind_out(p, nan(B, H, Nq, D))
        if topk and idx is not None:
            res["idx"], p.idx_out = idx, idx.data_ptr()
        elif topk and "idx" in take:
            res["idx"] = ops._new_idx(p, B, H, Nq, kt, True, dv)
        if topk and "mask" in take:
            res["mask"] = torch.empty((B, H, Nq, (T + 31) // 32), dtype=torch.int32, device=dv)
            p.mask_out = res["mask"].data_ptr()
        if "scores" in take:
            res["true"], res["pred"] = nan(B, H, Nq, T), nan(B, H, Nq, T)
            p.true_out = res["true"].data_ptr()
    p.pred_out = res["pred"].data_ptr() if "pred" in res else None
    ops._call_with_workspace(getattr(lib, ENTRY_SIZES[name]), getattr(lib, name), name, p, *(() if bits is None else (bits,)),
                             dev=dv)
    torch.cuda.synchronize()
    return res


def _equal_bits(got, want, what):
    """the same tensors by name (or absent on both sides), torch.equal on the bit patterns"""
    assert set(got) == set(want), (what, sorted(got), sorted(want))
    for name, a in got.items():
        b = want[name]
        assert torch.equal(a.view(torch.int32) if a.dtype == torch.float32 else a,
                           b.view(torch.int32) if b.dtype == torch.float32 else b), (what, name)


def check_siblings(M, q, k, v, scale, widths, **kw):
    """A float32 ex_pred call (device tensors; kw: k_top / top_k) that the sibling entry points take too,
    at each width: every attention entry point whose documented rules (include/mxa.h) accept it --
    mxa_attention_full, mxa_attention_bits; at width 8 mxa_attention_long and, with T <= 512, mxa_attention
    -- called directly, writes the bytes mxa_attention_full writes (out, idx, true, pred, the mask words),
    and so does M.mx_topk_attention; the same for the scores alone (mxa_approx_scores, _long, _bits and
    M.mx_approx_scores)"""
    T, topk = k.shape[-2], kw.get("top_k", True)
    for bits in widths:
        names = [("mxa_attention_full", bits), ("mxa_attention_bits", bits)]
        if bits == 8:
            names += [("mxa_attention_long", None)] + ([("mxa_attention", None)] if T <= 512 else [])
        res = M.mx_topk_attention(q, k, v, scale, return_scores=True, return_mask=topk, elem_bits=bits, **kw)
        op = dict(zip(("out", "idx", "true", "pred", "mask"), res))
        if not topk:
            assert op.pop("idx") is None
        full = None
        for name, width in names:
            got = attn_entry(M, name, q, k, v, scale, width, **kw)
            _equal_bits(got, op, f"{name} w{bits} vs the op")
            full = full or got
            _equal_bits(got, full, f"{name} w{bits} vs mxa_attention_full")
        pred = dict(pred=M.mx_approx_scores(q, k, "ex_pred", elem_bits=bits))
        for name, width in names[1:]:
            name = name.replace("attention", "approx_scores")
            _equal_bits(attn_entry(M, name, q, k, None, 1.0, width), pred, f"{name} w{bits}")


def quantize_bfloat_in_dtype(A, bfloat):
    """_quantize_bfloat (elemwise_ops.py:201-216 -> _quantize_elemwise_core :144-160) on a
    float16 / bfloat16 tensor, every step in the tensor's own dtype as torch computes it:
    on bfloat16 the `abs + 0.5` of _round_mantissa (:64-65) itself rounds (243.5 -> 244), so
    the result is not the float32 rounding of the same values."""
    if bfloat in (0, 32):
        return A
    bits = bfloat - 7
    pe = torch.floor(torch.log2(torch.abs(A) + (A == 0).type(A.dtype))).clip(min=-126)
    out = A / (2 ** pe) * (2 ** (bits - 2))
    out = torch.sign(out) * torch.floor(torch.abs(out) + 0.5)
    return out / (2 ** (bits - 2)) * (2 ** pe)


def check_mlp_chain(M, x, W1, b1, W2, b2, act, *, elem_bits=8, cmp, bfloat=0, w1=None, what="", flush=False):
    """The equalities of the MLP chain on the device, each by cmp (same / same_bits): pre is
    mx_linear's and the oracle's fc1; y is mx_linear's and the oracle's fc2 of the activation
    the device produced; y without the hidden copies.  w1: fc1's weight as prepared by the
    caller.  Returns y, pre, act on the host."""
    kw = dict(flush_subnormals=flush, bfloat=bfloat, elem_bits=elem_bits)
    ok = dict(elem=ELEM[elem_bits], flush=flush, bfloat=bfloat or 32)
    y, pre, a = M.mx_mlp(dev(x), dev(W1) if w1 is None else w1, dev_opt(b1), dev(W2), dev_opt(b2), act=act,
                         return_hidden=True, **kw)
    torch.cuda.synchronize()
    cmp(host(pre), host(M.mx_linear(dev(x), dev(W1), dev_opt(b1), **kw)), f"{what} pre vs mx_linear")
    cmp(host(pre), O.mx_linear(x, W1, b1, **ok), f"{what} pre vs oracle")
    cmp(host(y), host(M.mx_linear(a, dev(W2), dev_opt(b2), **kw)), f"{what} y vs mx_linear(act)")
    cmp(host(y), O.mx_linear(host(a), W2, b2, **ok), f"{what} y vs the oracle's Linear of act")
    y2 = M.mx_mlp(dev(x), dev(W1) if w1 is None else w1, dev_opt(b1), dev(W2), dev_opt(b2), act=act, **kw)
    cmp(host(y2), host(y), f"{what} y without the hidden copies")
    return host(y), host(pre), host(a)
