"""The partition step's exchange on the device (mxa_topk_grp.hpp grp_partition: one slot
index space, one combined mask per lane) on the rows built for it (exchange_cases.py): the
standalone top-k, packed and 64-bit elements, and two fused calls, bit-exact against
libstdc++'s order."""
import numpy as np
import pytest

import exchange_cases as XC
from gpu_support import M, dev  # noqa: F401
from oracle import mx_oracle as O

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def batches():
    """{n: (rows, rows on the device)}, built once"""
    out = {}
    for n in sorted({n for n, _ in XC.NK}):
        rows = XC.batch(n)
        out[n] = (rows, dev(rows))
    return out


@pytest.mark.parametrize("n,k", XC.NK)
def test_topk_exchange_rows(M, batches, n, k):
    rows, rows_t = batches[n]
    _, want = O.topk(rows, k)
    names = [name for name, _ in XC.named_rows(n)]
    for packed in (True, False):
        _, idx = M.topk(rows_t, k, packed=packed)
        got = idx.cpu().numpy()
        bad = sorted({names[r] for r in np.argwhere(got != want)[:, 0]})
        assert not bad, f"n{n} k{k} packed={packed}: rows {bad[:6]} differ"


@pytest.mark.parametrize("B,H,N,T,D,k", XC.FUSED)
def test_fused_exchange(M, B, H, N, T, D, k):
    rng = np.random.default_rng(N + k)
    q, kk, v = (rng.standard_normal((B, H, n, D), dtype=np.float32) for n in (N, T, T))
    r = O.attention(q, kk, v, D ** -0.5, k_top=k, pred_mode="ex_pred")
    _, idx = M.mx_topk_attention(dev(q), dev(kk), dev(v), D ** -0.5, k_top=k, pred_mode="ex_pred")[:2]
    assert np.array_equal(idx.cpu().numpy().reshape(r["idx"].shape), r["idx"])
