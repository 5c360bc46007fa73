"""The attention output bit for bit: the inputs of tests/exact_out_cases.py, whose out is the
only float32 result a correct softmax, MX(P), MX(V) and P.V can produce (test_exact_out_cpu.py
proves that per case with the oracle alone), on every finishing kernel -- finish16_kernel and
its LONG variant, finish_kernel, finish_qk_kernel top-k and dense, dense_rows_kernel.  idx, the
prune mask and the true scores against the oracle as everywhere else; the dispatch pinned with
mxa_attention_finish_kernel where rows of at most 512 keys leave a choice.

Each case runs the op twice: with no score output (the plain instantiations; a bias, the
score outputs and bfloat rounding select the EXTRA ones) and with it."""
import ctypes

import pytest
import torch

import exact_out_cases as EC
from gpu_support import M, dev, dev_opt, host, same, same_bits  # noqa: F401
from oracle import mx_oracle as O

pytestmark = pytest.mark.gpu


def _op_kw(c):
    kw = dict(c.kw)
    kw.update(dict(k_top=c.k) if c.k else dict(top_k=False))
    return kw


@pytest.mark.parametrize("c", EC.CASES, ids=EC.case_id)
def test_exact_out(M, c):
    q, kk, v, bias = EC.inputs(c)
    r = EC.reference(c)
    tq, tk, tv, tb = dev(q), dev(kk), dev(v), dev_opt(bias)
    kw = _op_kw(c)
    what = EC.case_id(c)
    if c.T <= 512:
        p, _, _, _ = M.ops._attn_params(tq, tk, tv, EC.SCALE, c.k, kw.get("pred_mode", "ex_pred"), c.k > 0,
                                        c.k > 0 and kw.get("approx", True), tb, False, kw.get("bfloat", 0), None)
        p.out = 16  # the query launches nothing
        assert M._native.lib().mxa_attention_finish_kernel(ctypes.byref(p)) == c.kind
    for scores in (False, True):
        res = M.mx_topk_attention(tq, tk, tv, EC.SCALE, bias=tb, return_scores=scores, return_mask=c.k > 0, **kw)
        torch.cuda.synchronize()
        w = f"{what} scores={scores}"
        if c.k:
            same(host(res[1]), r["idx"], w + " idx")
            same(host(M.unpack_mask(res[-1], c.T)), O.prune_mask(r["idx"], c.T), w + " mask")
        else:
            assert res[1] is None
        if scores:
            same(host(res[2]), r["true"], w + " true")
        same_bits(host(res[0]), r["out"], w + " out")


def test_exact_out_long_rows_32_row_chunks(M):
    """The long rows' selection kernel in chunks of 32 rows (mxa_sel_long.hip: BH * ceil(N / 32)
    >= 2048, which no other test reaches): 1,024 heads of 33 rows share one K / V, expanded
    and made contiguous on the device; the oracle runs once on a single head of all 33,792
    query rows.  idx, mask and out of every row bit for bit."""
    c = EC.CHUNK32
    q, kk, v, _ = EC.inputs(c, (1, 1))
    r = EC.reference(c, (1, 1))
    tq = dev(q.reshape(c.B, c.H, c.N, c.D))
    tk, tv = (dev(x).expand(c.B, c.H, c.T, c.D).contiguous() for x in (kk, v))
    out, idx, mask = M.mx_topk_attention(tq, tk, tv, EC.SCALE, k_top=c.k, return_mask=True)
    torch.cuda.synchronize()
    del tk, tv
    want = r["idx"].reshape(c.B, c.H, c.N, c.k)
    same(host(idx), want, "idx")
    same(host(M.unpack_mask(mask, c.T)), O.prune_mask(want, c.T), "mask")
    same_bits(host(out), r["out"].reshape(c.B, c.H, c.N, c.D), "out")
