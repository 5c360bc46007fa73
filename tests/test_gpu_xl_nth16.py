"""float16 / bfloat16 top-k with k_top > 64 on rows of 1,025 .. 4,096 keys through the fused op (mxa_attention_nth_dt:
select_xl_nth_kernel, then finish_gather_xl_kernel for k_top <= 256 or the masked 16-bit finish_qk_xl_kernel above).

O.attention computes in float32 only and these shapes have no golden file, so the checks are test_gpu_xl_nth.py's
test_nth_16_bit's: the recorded true / pred rows bit-equal to those of the k_top = 16 call on the same tensors (a
call served before these kernels existed), idx equal to torch.topk on the CPU of the recorded pred rows, the mask words
O.prune_mask's, the output dtype, and out against a float64 softmax(true[idx]) . v[idx]:
  bfloat16  normwise within 2^-6 + 2^-8 (MXINT8 P and V: 2^-7 each; the output's rounding: 2^-8), and per query row
            ||got - ref|| / ||ref|| within ROW_TOL = twice the worst such figure of the bfloat16 call with T = 4,096,
            k_top = 64, D = 72 on the same draws, which finish16_xl_kernel serves: measured once, 0.01526 (the
            doubling is the margin for the longer sum; nothing is fitted to the kernels under test);
  float16   the two shapes keep fewer keys than the row has 32-key blocks (65 < 66, 100 < 128), so every row has an
            all-zero P block, which float16 quantizes to NaN, and 0 * NaN reaches every element: out is all NaN.
B = 1, H = 2, N = 33: two tiles and a one-row remainder, two heads."""
import numpy as np
import pytest
import torch

from gpu_support import M, host, rnd, same, same_bits  # noqa: F401
from oracle import mx_oracle as O

pytestmark = pytest.mark.gpu

N = 33
BASE_ROW_ERR = 0.01526  # bfloat16, T = 4,096, k_top = 64, D = 72: the worst row of row_errors (see above)
ROW_TOL = 2 * BASE_ROW_ERR
BF16, F16 = torch.bfloat16, torch.float16
GATHER = [(1025, 65, 32, BF16), (1025, 256, 72, BF16), (2085, 154, 72, BF16), (4096, 154, 72, BF16), (4096, 256, 128, BF16),
          (2085, 65, 72, F16), (4096, 100, 72, F16)]
MASKED = [(1025, 257, 72, BF16), (2085, 300, 72, BF16)]


def row_errors(out, true_s, idx, v):
    """per query row ||out - ref|| / ||ref|| against the float64 softmax(true[idx]) . v[idx], and the normwise error"""
    s = np.take_along_axis(host(true_s).astype(np.float64), idx, -1)
    p = np.exp(s - s.max(-1, keepdims=True))
    p /= p.sum(-1, keepdims=True)
    vk = host(v, f32=True).astype(np.float64)[0][np.arange(idx.shape[1])[:, None, None], idx[0]]  # (H, N, k, D)
    ref = np.einsum("hnk,hnkd->hnd", p[0], vk)[None]
    got = host(out, f32=True).astype(np.float64)
    return np.linalg.norm(got - ref, axis=-1) / np.linalg.norm(ref, axis=-1), O.normwise_rel_err(got, ref)


def check(M, T, k, D, dt, autocast=None, biased=False):
    tdt = torch.float32 if autocast else dt
    q, kk, v = (torch.from_numpy(rnd(s, 40 + i)).to(tdt).cuda() for i, s in enumerate(((1, 2, N, D), (1, 2, T, D), (1, 2, T, D))))
    kw = dict(autocast=autocast, bias=torch.from_numpy(rnd((2, N, T), 43)).to(tdt).cuda() if biased else None)
    out, idx, true_s, pred_s, mask = M.mx_topk_attention(q, kk, v, D ** -0.5, k_top=k, return_scores=True, return_mask=True, **kw)
    _, _, true16, pred16 = M.mx_topk_attention(q, kk, v, D ** -0.5, k_top=16, return_scores=True, **kw)
    torch.cuda.synchronize()
    assert out.dtype == dt
    same_bits(host(true_s), host(true16), "true rows of the k = 16 call")
    same_bits(host(pred_s), host(pred16), "pred rows of the k = 16 call")
    want = torch.topk(pred_s.cpu(), k, dim=-1).indices.numpy()
    same(host(idx), want, "idx")
    same(host(M.unpack_mask(mask, T)), O.prune_mask(want, T), "mask")
    got = host(out, f32=True)
    if dt == F16:
        assert np.isnan(got).all()
        return
    assert np.isfinite(got).all()
    rows, err = row_errors(out, true_s, want, v)
    print(f"T{T} k{k} D{D}: normwise {err:.5f}, worst row {rows.max():.5f} (bound {ROW_TOL:.5f})")
    assert err <= 2.0 ** -6 + 2.0 ** -8, err
    assert rows.max() <= ROW_TOL, rows.max()


@pytest.mark.parametrize("T,k,D,dt", GATHER + MASKED, ids=str)
def test_nth16(M, T, k, D, dt):
    check(M, T, k, D, dt)


@pytest.mark.parametrize("kw", [dict(autocast=BF16), dict(biased=True)], ids=str)
def test_nth16_autocast_and_bias(M, kw):
    check(M, 2085, 154, 72, BF16, **kw)
