"""Top-k outside torch's partial_sort regime on rows of 1,025 .. 4,096 keys: M.topk (mxa_topk_xl_nth) and the fused
op (mxa_attention_nth: select_xl_nth_kernel, then finish16_xl_kernel for k <= 64 or the masked finish_qk_xl_kernel
for k > 64).

topk: torch.topk on the CPU tensor is the specification -- indices and mask equal, values bit for bit -- on
test_gpu_xl_rows.topk_rows' rows plus the negated Musser median-of-three adversary, which O.introselect_probe shows
reaching introselect's depth limit (the __heap_select fall-back) at the pairs of DEPTH; at the other pairs (k at or
next to n, and the two shortest rows) it does not, and the assertion says so too.
The fused op: idx, mask words and recorded scores bit for bit against the oracle, out by out_close at OUT_TOL and
out_rows_close -- test_gpu_xl_rows.check_case.  B = 1, H = 2, N = 33.  For k > 64 the row bound is asserted through
gpu_support.out_row_bound itself (check_masked): out_rows_close first asserts, from the oracle alone, that at most
15 % of the rows hold an element within tau of a rounding tie, and tau grows with the kernel's sum chain -- 8 ntb + 2
= 530 additions at 2,085 keys against the 16-row kernel's 18 -- so at (2085, 65) 31.8 % of the rows do, whatever the
device computes.  The elementwise bound A + F and the NaN pattern are asserted as out_rows_close asserts them.
float16 / bfloat16 at (1279, 20): O.attention computes in float32 only and there is no golden file for this shape,
so the check is of the selection: idx and mask against torch.topk on the CPU of the score rows the call itself
recorded, those rows bit-equal to the rows of the k = 16 call mxa_attention_dt already serves; out only within
the formats' own error of a float64 softmax(true[idx]) . v[idx] (MXINT8 P and V: 2^-7 each; the output's rounding:
2^-8 at bfloat16), 2^-6 + 2^-8 normwise at bfloat16 (float16 turns the rows' all-zero P blocks into NaN, which 0 * NaN carries into every element)."""
import numpy as np
import pytest
import torch

from gpu_support import ENTRY_SIZES, OUT_TOL, M, attn_entry, attn_run, check_attn, dev, host, out_close  # noqa: F401
from gpu_support import out_row_bound, rnd, same, same_bits, to_bits
from oracle import mx_oracle as O
from test_gpu_xl_rows import N, case, check_case, mode_kw, topk_rows

pytestmark = pytest.mark.gpu

NK = [(1025, 17), (1025, 1024), (1025, 1025), (1279, 20), (2085, 33), (2085, 1000), (4096, 65), (4096, 2048), (4096, 4096),
      (4095, 64)]
DEPTH = {(2085, 33), (2085, 1000), (4096, 65), (4095, 64), (2085, 154)}  # the adversary row reaches the depth limit


def adversary(n):
    """Musser's median-of-three killer, negated (the comparator is `greater`)"""
    h = n // 2
    a = np.where(np.arange(h) % 2 == 0, np.arange(h) + 1, h + np.arange(h))
    return -np.concatenate([a, 2 * np.arange(1, h + 1), [2 * h + 1] * (n % 2)]).astype(np.float32)


@pytest.mark.parametrize("n,k,dt", [nk + (torch.float32,) for nk in NK] + [(2085, 154, torch.float16), (2085, 154, torch.bfloat16)],
                         ids=str)
def test_topk_xl_nth(M, n, k, dt):
    x = torch.cat([topk_rows(n), torch.from_numpy(adversary(n))[None]]).to(dt)
    assert O.introselect_probe(x[-1].float().numpy(), k)["depth_limit"] == ((n, k) in DEPTH)
    wv, wi = torch.topk(x, k, dim=-1)
    gv, gi, gm = M.topk(x.cuda(), k, return_mask=True)
    torch.cuda.synchronize()
    same(host(gi), wi.numpy(), f"n{n} k{k} idx")
    dts = {torch.float16: "f16", torch.bfloat16: "bf16"}.get(dt)
    same_bits(to_bits(gv), to_bits(wv), f"n{n} k{k} values", dt=dts, patterns=True)
    same(host(M.unpack_mask(gm, n)), O.prune_mask(wi.numpy(), n), f"n{n} k{k} mask")


def test_topk_xl_nth_k0(M):
    x = topk_rows(2085).cuda()
    gv, gi, gm = M.topk(x, 0, return_mask=True)
    torch.cuda.synchronize()
    assert gi.shape == (x.shape[0], 0) and not host(gm).any()


@pytest.mark.parametrize("mode", ["ex_pred", "MXINT4", "true"])
@pytest.mark.parametrize("D", [32, 72])
@pytest.mark.parametrize("T,k", [(1025, 17), (1279, 20), (2085, 33), (2085, 64)])
def test_nth_gather16(M, T, k, D, mode):
    check_case(M, T, k, D, mode)


def check_masked(M, T, k, mode, bits=8, biased=False):
    """check_case for k > 64: the row bound is the three-pass MFMA kernels' ("qk": one fmaf per key block, a sum
    chain of 8 ntb + 2), which gpu_support.finish_kernel_of names for rows of at most 256 keys only"""
    q, kk, v, bias, scale, ref = case(T, k, 72, mode, bits, biased)
    what = f"T{T} k{k} {mode} w{bits}" + (" bias" if biased else "")
    kw = dict(k_top=k, **mode_kw(mode), **(dict(bias=bias) if biased else {}))
    got = attn_run(M, q, kk, v, scale, bits, **kw)  # with the scores: the EXTRA form
    check_attn(got, ref, what, same_bits)
    out_close(got["out"], ref["out"], OUT_TOL, what + " out")
    bound, fin, shares, _, _ = out_row_bound(ref, v, "qk", bits)
    same(np.isnan(got["out"]), np.isnan(ref["out"]), what + " NaN pattern")
    err = np.abs(got["out"][fin].astype(np.float64) - ref["out"][fin].astype(np.float64))
    print(f"{what}: eligible elements {shares[0]:.4%} rows {shares[1]:.2%}, worst |got - ref| / (A + F) "
          f"{float(np.max(err / np.maximum(bound[fin], 1e-300), initial=0.0)):.3f}")
    assert (err <= bound[fin]).all(), what + " out: |got - ref| > A + F"
    plain = attn_run(M, q, kk, v, scale, bits, scores=False, **kw)  # ... and the plain form
    same(plain["idx"], got["idx"], what + " idx without the scores")
    same_bits(plain["out"], got["out"], what + " out without the scores")
    kwd = {a: dev(x) if isinstance(x, np.ndarray) else x for a, x in kw.items()}  # ... and on the workspace's mask words
    bare = M.mx_topk_attention(dev(q), dev(kk), dev(v), scale, elem_bits=bits, **kwd)[0]
    same_bits(host(bare), got["out"], what + " out without mask_out")


@pytest.mark.parametrize("mode", ["ex_pred", "true"])
@pytest.mark.parametrize("T,k", [(2085, 65), (2085, 154), (4096, 65), (4096, 614)])
def test_nth_masked_mfma(M, T, k, mode):
    check_masked(M, T, k, mode)


def test_nth_mask_bias(M):
    check_masked(M, 2085, 154, "ex_pred", biased=True)


@pytest.mark.parametrize("T,k", [(1279, 20), (2085, 154)])
def test_nth_mxint4_elements(M, T, k):
    check_case(M, T, k, 72, "ex_pred", bits=4) if k <= 64 else check_masked(M, T, k, "ex_pred", bits=4)


@pytest.mark.parametrize("dt", [torch.float16, torch.bfloat16], ids=str)
def test_nth_16_bit(M, dt):
    T, k, D = 1279, 20, 72
    q, kk, v = (torch.from_numpy(rnd(s, 40 + i)).to(dt).cuda() for i, s in enumerate(((1, 2, N, D), (1, 2, T, D), (1, 2, T, D))))
    out, idx, true_s, pred_s, mask = M.mx_topk_attention(q, kk, v, D ** -0.5, k_top=k, return_scores=True, return_mask=True)
    _, _, true16, pred16 = M.mx_topk_attention(q, kk, v, D ** -0.5, k_top=16, return_scores=True)
    torch.cuda.synchronize()
    assert out.dtype == dt
    same_bits(host(true_s), host(true16), "true rows of the k = 16 call")
    same_bits(host(pred_s), host(pred16), "pred rows of the k = 16 call")
    want = torch.topk(pred_s.cpu(), k, dim=-1).indices.numpy()
    same(host(idx), want, "idx")
    same(host(M.unpack_mask(mask, T)), O.prune_mask(want, T), "mask")
    s = np.take_along_axis(host(true_s).astype(np.float64), want, -1)
    p = np.exp(s - s.max(-1, keepdims=True))
    p /= p.sum(-1, keepdims=True)
    vk = host(v, f32=True).astype(np.float64)[0][np.arange(2)[:, None, None], want[0]]  # (H, N, k, D)
    ref = np.einsum("hnk,hnkd->hnd", p[0], vk)[None]
    got = host(out, f32=True)
    fin = np.isfinite(got)
    if dt == torch.float16:  # float16 quantizes an all-zero P block to NaN, and 0 * NaN reaches every row (test_gpu_long_dtype.py)
        assert not fin.any()
        return
    assert fin.all()
    err = O.normwise_rel_err(got, ref)
    assert err <= 2.0 ** -6 + 2.0 ** -8, err


# ---- siblings: mxa_attention_nth (the op) writes mxa_attention_dt's bytes where both accept --------------
ENTRY_SIZES.setdefault("mxa_attention_dt", "mxa_attention_dt_workspace_bytes")  # (attn_entry's table of size functions)


@pytest.mark.parametrize("T,kw", [(1280, dict(k_top=20)), (1000, dict(k_top=129)), (2085, dict(top_k=False))], ids=str)
def test_nth_writes_the_dt_entry_points_bytes(M, T, kw):
    q, kk, v = dev(rnd((1, 2, N, 72), T)), dev(rnd((1, 2, T, 72), T + 1)), dev(rnd((1, 2, T, 72), T + 2))
    topk = kw.get("top_k", True)
    res = M.mx_topk_attention(q, kk, v, 0.125, return_scores=True, return_mask=topk, **kw)
    old = attn_entry(M, "mxa_attention_dt", q, kk, v, 0.125, 8, **kw)
    op = dict(zip(("out", "idx", "true", "pred", "mask"), res))
    assert set(old) == {n for n, t in op.items() if t is not None}
    for name, t in old.items():
        assert torch.equal(t.view(torch.int32) if t.dtype == torch.float32 else t,
                           op[name].view(torch.int32) if t.dtype == torch.float32 else op[name]), name
