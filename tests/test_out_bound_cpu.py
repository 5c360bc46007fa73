"""gpu_support.out_rows_close on the CPU: a float32 model of the kernels' softmax (exp2 of the
scaled difference, one-ulp errors at random, another summation order) stays inside the bound
and flips P codes only inside the eligible set; the five defects the normwise bar lets through
("The attention output") do not."""
import functools

import numpy as np
import pytest

from gpu_support import ELIGIBLE_ELEMS, ELIGIBLE_ROWS, OUT_TOL, out_close, out_row_bound, out_rows_close
from oracle import mx_oracle as O

F32 = np.float32
SHAPES = {"fin16": (4, 6, 197, 197, 64, 20), "qk": (1, 2, 64, 256, 72, 154), "fin32": (1, 2, 40, 300, 128, 257),
          "long": (1, 2, 20, 1000, 72, 64), "dense_qk": (2, 3, 77, 120, 72, 0), "dense_rows": (1, 2, 40, 300, 32, 0)}


@functools.lru_cache(maxsize=None)
def case(name):
    B, H, N, T, D, k = SHAPES[name]
    rng = np.random.default_rng(len(name) * 100 + T)
    q, kk, v = (rng.standard_normal((B, H, n, D), dtype=F32) for n in (N, T, T))
    r = O.attention(q, kk, v, float(D) ** -0.5, **(dict(k_top=k) if k else dict(top_k=False)))
    return v, r, O.quantize_mx(r["attn"], "int8", 32, -1)[0], O.quantize_mx(v, "int8", 32, -2)[0]


def device_model(r, v, rng):
    """P as a kernel computes it: exp2((x - mx) * log2 e) in float32, a sequential sum, the
    correctly rounded quotient, each with a random error of -1 / 0 / +1 ulp; then MX(P) and the
    product summed per 32-key block in float32."""
    true = r["true"]
    T = true.shape[-1]
    kept = O.prune_mask(r["idx"], T) if "idx" in r else np.ones(true.shape, bool)
    x = np.where(kept, true, -np.inf).astype(F32)
    jit = lambda a: (a.view(np.int32) + rng.integers(-1, 2, a.shape) * (a > 0)).astype(np.int32).view(F32)  # noqa: E731
    e = jit(np.exp2(((x - x.max(-1, keepdims=True)) * F32(1.4426950408889634)).astype(F32)).astype(F32))
    s = np.zeros(e.shape[:-1], F32)
    for j in range(T):
        s = (s + e[..., j]).astype(F32)
    p = jit((e / s[..., None]).astype(F32))
    pq, codes, _ = O.quantize_mx(p, "int8", 32, -1)
    vq = O.quantize_mx(v, "int8", 32, -2)[0]
    out = np.zeros(true.shape[:-1] + (v.shape[-1],), F32)
    for b in range(0, T, 32):
        out = (out + np.matmul(pq[..., b:b + 32].astype(np.float64), vq[..., b:b + 32, :].astype(np.float64))).astype(F32)
    return out, codes


@pytest.mark.parametrize("name", list(SHAPES))
def test_float32_softmax_model_stays_inside(name):
    v, r, _, _ = case(name)
    out_rows_close(r["out"].copy(), r, v, name + " reference")
    _, fin, (se, sr), _, elig = out_row_bound(r, v)
    assert fin.all() and se <= ELIGIBLE_ELEMS and sr <= ELIGIBLE_ROWS
    ref_codes = O.quantize_mx(r["attn"], "int8", 32, -1)[1]
    for seed in range(3):
        out, codes = device_model(r, v, np.random.default_rng(seed))
        flipped = O.from_blocks(codes != ref_codes, r["attn"].shape[-1], -1)
        print(f"{name} model {seed}: {flipped.sum()} codes moved, {elig.sum()} eligible")
        assert not (flipped & ~elig).any(), f"{name}: a code moved outside the eligible set"
        assert np.abs(codes - ref_codes).max() <= 1
        out_rows_close(out, r, v, f"{name} model {seed}")


def _mutants(name):
    """the reference's own quantized operands with one defect each, as float32 outputs"""
    v, r, pq, vq = case(name)
    a = r["attn"]
    T, D = a.shape[-1], v.shape[-1]
    row = (0, 0, 3)
    out = {}
    p1 = pq.copy()  # a kept key with a small weight dropped
    j = np.where(a[row] > 0, a[row], np.inf).argmin()
    p1[row + (j,)] = 0
    out["dropped key"] = O.exact_matmul_f32(p1, vq)
    v2 = vq.copy()  # a V block scale one exponent up in one token block of one column
    v2[0, 0, 32:64, 5] *= 2
    out["V block scale"] = O.exact_matmul_f32(pq, v2)
    p3 = pq.copy()  # a P code three steps off
    j = a[row].argmax()
    step = np.exp2(np.floor(np.log2(a[row][32 * (j // 32):32 * (j // 32) + 32].max())) - 6)
    p3[row + (j,)] += 3 * step
    out["P code off"] = O.exact_matmul_f32(p3, vq)
    p4 = pq.copy()  # a wrong element in the last, ragged key block
    last = [t for t in range(32 * ((T - 1) // 32), T) if pq[row + (t,)] > 0]
    if last:
        p4[row + (last[0],)] = pq[row + (last[-1],)] * 2
        out["ragged block"] = O.exact_matmul_f32(p4, vq)
    o5 = r["out"].copy()  # one bad output column of the D = 72 clamp
    if D == 72:
        o5[..., 3, 71] = o5[..., 3, 70]
        out["column clamp"] = o5
    return out


@pytest.mark.parametrize("name", list(SHAPES))
def test_defects_the_normwise_bar_passes_are_caught(name):
    v, r, _, _ = case(name)
    muts = _mutants(name)
    assert len(muts) >= 3
    for what, got in muts.items():
        err = O.normwise_rel_err(got, r["out"])
        print(f"{name} {what}: normwise {err:.2e}")
        if name == "fin16" and what != "V block scale":  # one bad row in 4,728 (a block scale is
            out_close(got, r["out"], OUT_TOL, what)      # every row of a head): the old bar passes ...
        with pytest.raises(AssertionError, match="A \\+ F"):  # ... the row-wise bound does not
            out_rows_close(got, r, v, f"{name} {what}")
