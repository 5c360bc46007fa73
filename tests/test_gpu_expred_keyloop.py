"""The ex_pred key loop for one and two blocks (key records, product-form values, the loop with
and without the pred store) and the peeled first partition step behind it, on small shapes:
pred, idx and true bit-exact against the oracle.  Every case runs with return_scores=True and
False: the two copies of the loop."""
import math

import numpy as np
import pytest

from gpu_support import M, dev, host, same  # noqa: F401
from oracle import mx_oracle as O

pytestmark = pytest.mark.gpu

B, H = 1, 2
DS = (32, 64, 48)  # one block, two blocks, a second block of 16 elements
TS = (1, 15, 16, 17, 31, 32, 33, 48, 49, 50, 64, 65, 127, 128, 129, 197, 224, 225, 256)


def inputs(case, T, D):
    """a: standard-normal, 5 query rows (a row group and a ragged one); b: a two-value alphabet
    (every partition step full of ties); c: all-equal scores on 37 rows (a workgroup boundary at
    32): the depth-limit and heap hand-overs behind the first step."""
    rng = np.random.default_rng(1000 * T + D)
    N = 37 if case == "c" else 5
    if case == "a":
        q, k = rng.standard_normal((B, H, N, D)), rng.standard_normal((B, H, T, D))
    elif case == "b":
        q, k = rng.choice([-1.0, 1.0], (B, H, N, D)), rng.choice([-1.0, 1.0], (B, H, T, D))
    else:
        q, k = np.ones((B, H, N, D)), np.ones((B, H, T, D))
    v = rng.standard_normal((B, H, T, D))
    return q.astype(np.float32), k.astype(np.float32), v.astype(np.float32)


def check(M, q, k, v, ks, what, pred=None):
    """Both copies of the loop at every k of ks against the oracle (scores once, top-k per k).
    pred: the oracle's scores where the caller had to sum its operands' products itself."""
    D, T = q.shape[-1], k.shape[-2]
    scale = float(D) ** -0.5
    with np.errstate(all="ignore"):
        ref = O.attention(q, k, v, scale, k_top=ks[0])
    if pred is not None:
        ref["pred"], ref["idx"] = pred, O.topk(pred, ks[0])[1]
    qd, kd, vd = dev(q), dev(k), dev(v)
    for kt in ks:
        want = ref["idx"] if kt == ks[0] else O.topk(ref["pred"], kt)[1]
        _, idx, true_s, pred_s = M.mx_topk_attention(qd, kd, vd, scale, k_top=kt, return_scores=True)
        _, idx_n = M.mx_topk_attention(qd, kd, vd, scale, k_top=kt)[:2]
        same(host(pred_s), ref["pred"], f"{what} k{kt} pred", signed=True)
        same(host(true_s), ref["true"], f"{what} k{kt} true")
        same(host(idx), want, f"{what} k{kt} idx (scores returned)")
        same(host(idx_n), want, f"{what} k{kt} idx (no scores)")


@pytest.mark.parametrize("D", DS)
@pytest.mark.parametrize("case", ["a", "b", "c"])
def test_keyloop_shapes(M, case, D):
    for T in TS:
        q, k, v = inputs(case, T, D)
        check(M, q, k, v, sorted({min(20, T), min(33, T)}), f"{case} T{T} D{D}")


@pytest.mark.parametrize("kt", [1, 34])
def test_keyloop_k_edges(M, kt):
    """k = 1; k = 34: one past the tail's limit, the packed pass finishes its rows itself."""
    q, k, v = inputs("a", 197, 64)
    check(M, q, k, v, [kt], f"a T197 D64")
    q, k, v = inputs("b", 197, 64)
    check(M, q, k, v, [kt], f"b T197 D64")


@pytest.mark.parametrize("D", DS)
def test_approx_scores_alone(M, D):
    q, k, _ = inputs("a", 197, D)
    aq, ak = O.approx_operands(q, k, "ex_pred")
    same(host(M.mx_approx_scores(dev(q), dev(k), "ex_pred")), O.exact_matmul_f32(aq, np.swapaxes(ak, -1, -2)), f"D{D}",
         signed=True)


def test_fast_range_edges(M):
    """Block exponents across [kExpFastLo, kExpFastHi]: keys at 2^59 .. 2^63, query rows at
    2^-49 .. 2^-53, a key with a NaN block, a zero key row and a key whose blocks are 60 binades
    apart -- the records' redo path, with N % 4 != 0.
    The oracle's exact_matmul_f32 sums in float64, which is exact only while a row's products
    span <= 53 bits; the 60-binade key's do not (where its large block cancels, m0 = 0, the
    float64 sum drops the small block: 0.0 for -1.32e-23).  So that key's column is the oracle's
    operands summed exactly (math.fsum); every other column must equal the oracle's own."""
    T, D, N = 197, 64, 5
    rng = np.random.default_rng(7)
    k = rng.standard_normal((B, H, T, D)) * np.ldexp(1.0, 59 + np.arange(T) % 5)[:, None]
    q = rng.standard_normal((B, H, N, D)) * np.ldexp(1.0, -49 - np.arange(N))[:, None]
    k[:, :, 7, 40] = np.nan
    k[:, :, 11] = 0.0
    k[:, :, 13, :32] = rng.standard_normal(32) * 2.0 ** 30
    k[:, :, 13, 32:] = rng.standard_normal(32) * 2.0 ** -30
    v = rng.standard_normal((B, H, T, D))
    q, k, v = q.astype(np.float32), k.astype(np.float32), v.astype(np.float32)
    with np.errstate(all="ignore"):
        aq, ak = O.approx_operands(q, k, "ex_pred")
        pred = O.exact_matmul_f32(aq, np.swapaxes(ak, -1, -2))
    for h in range(H):
        for r in range(N):
            pred[0, h, r, 13] = np.float32(math.fsum((aq[0, h, r].astype(np.float64) * ak[0, h, 13].astype(np.float64)).tolist()))
    check(M, q, k, v, [20, 33], "edges", pred=pred)
