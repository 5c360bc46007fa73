"""The conditions tests/test_gpu_bias_out.py and the bias cases of tests/test_gpu_dtype.py rely on, from the
oracle, the library's host logic and the fixtures alone (no GPU): every case of tests/bias_cases.py runs on
the finishing kernel it names; the eligible shares of the row-wise bound stay within the caps for every value
set; a bias read with a wrong batch or head stride, or not read at all, changes the kept indices (the true
scores on the dense branch); and the reference's autocast fixture tells the float32 `pred + bias` from one
rounded to the autocast dtype again.

The shares measured here (elements, rows; the largest over the five value sets of a case) are recorded in
DESIGN.md, "Bias layouts and the caller's out"."""
import ctypes

import numpy as np
import pytest
import torch

import bias_cases as BC
from gpu_support import ELIGIBLE_ELEMS, ELIGIBLE_ROWS, TDT, host_params, load, out_row_bound, same
from oracle import mx_oracle as O

ids = dict(ids=BC.case_id)


@pytest.fixture(scope="module")
def nat():
    from mx_quantization_amd import _native
    return _native


@pytest.mark.parametrize("c", BC.CASES, **ids)
def test_case_runs_on_its_finishing_kernel(nat, c):
    p = host_params(nat, c.B, c.H, c.N, c.T, c.D, c.k, top_k=int(c.k > 0))
    p.bias, p.approx = 16, int(c.mode is not None)
    assert nat.lib().mxa_attention_full_finish_kernel(ctypes.byref(p), c.bits) == c.kind


@pytest.mark.parametrize("c", BC.CASES, **ids)
def test_eligible_shares_within_caps(c):
    worst = [0.0, 0.0]
    for vs in BC.VALUE_SETS:
        se, sr = BC.shares(c, vs)
        worst = [max(worst[0], se), max(worst[1], sr)]
        assert se <= ELIGIBLE_ELEMS and sr <= ELIGIBLE_ROWS, f"{vs}: eligible elements {se:.4%}, rows {sr:.2%}"
    print(f"{BC.case_id(c)}: eligible elements {worst[0]:.4%} rows {worst[1]:.2%}")


@pytest.mark.parametrize("c", BC.CASES, **ids)
def test_bias_discriminates_heads_batches_and_presence(c):
    """idx (dense: true) of every row of a head >= 1 changes when head 0's bias is read for every head, of every
    row of an image >= 1 when image 0's is read for every image; without the bias most rows change"""
    key = "idx" if c.k else "true"
    full = BC.reference(c)[key]
    rows = lambda vs: (BC.reference(c, vs)[key] != full).any(-1)  # noqa: E731  (B, H, N)
    h, b, none = rows("head0"), rows("hnt"), rows("none")
    assert h[:, 1:].all() and not h[:, 0].any(), h.mean()
    assert b[1:].all() and not b[0].any(), b.mean()
    assert none.mean() > 0.5, none.mean()
    print(f"{BC.case_id(c)}: rows that change without the bias {none.mean():.1%}")


@pytest.mark.parametrize("c", BC.CASES, **ids)
def test_mask_value_set_keeps_a_nan_row(c):
    out = BC.reference(c, "mask")["out"]
    nan = np.isnan(out).all(-1)
    assert nan[c.B - 1, :, 2].all() and nan.sum() == c.H and not np.isnan(out[~nan]).any()


@pytest.mark.parametrize("bits", [8, 4])
@pytest.mark.parametrize("vs", ["full", "hnt"])
def test_fused_block_references(bits, vs):
    """the fused blocks' references: shares within the caps, and the bias moves the kept indices"""
    ch, bias, r = BC.cross_reference(bits, vs)
    qkv, heads, sbias, rs = BC.self_reference(bits, vs)
    for what, ref, v, plain in (("cross", r, ch["vh"], ch["r"]), ("self", rs, heads[2], None)):
        se, sr = out_row_bound(ref, v, bits=bits)[2]
        print(f"{what} d48 w{bits} {vs}: eligible elements {se:.4%} rows {sr:.2%}")
        assert se <= ELIGIBLE_ELEMS and sr <= ELIGIBLE_ROWS
        if plain is not None:
            assert (plain["idx"] != ref["idx"]).any(-1).mean() > 0.5


# ---- the reference's fixtures (tests/golden/gen_dtype_bias_golden.py) --------------------------------------
def _round(x, dt):
    return torch.from_numpy(np.ascontiguousarray(x)).to(TDT[dt]).float().numpy()


@pytest.mark.parametrize("dt", ["f16", "bf16"])
@pytest.mark.parametrize("btag", ["real", "mask"])
def test_autocast_fixture_discriminates(dt, btag):
    """Under autocast the reference's `pred = pred + bias` is float32 (torch's promotion of the 16-bit pred and the
    float32 bias): the stored pred is float32, holds values the autocast dtype cannot represent, ranks to the
    stored idx as it is -- and to other indices once rounded to the dtype again.
    Rows (of 240) whose kept indices change: f16 real 14, f16 mask 31, bf16 real 82, bf16 mask 75 (the mask
    leaves the unmasked values as they were: there the order of torch's tied values moves, which depends on the
    whole row)."""
    F = load("attn_dtype_bias_ac.npz")
    pred, idx = F[f"{dt}/{btag}/pred"], F[f"{dt}/{btag}/idx"].astype(np.int64)
    assert pred.dtype == np.float32 and F[f"{dt}/{btag}/true"].dtype == np.uint16
    same(O.topk(pred, idx.shape[-1])[1], idx, "the stored pred ranks to the stored idx")
    again = _round(pred, dt)
    assert (again != pred).any()
    changed = (O.topk(again, idx.shape[-1])[1] != idx).any(-1)
    print(f"{dt} {btag}: {(again != pred).mean():.1%} of pred not representable, {changed.sum()} of {changed.size} rows re-rank")
    assert changed.sum() >= 1


def test_dtype_fixture_stores_the_reference_dtypes():
    F, G32 = load("attn_dtype_bias.npz"), load("attn_dtype_bias_g32.npz")
    for name in F.files + G32.files:
        a = (F if name in F.files else G32)[name]
        assert a.dtype == (np.int16 if name.endswith("/idx") else np.uint16), (name, a.dtype)
