"""The forked attention call (mxa_attn.hip SideFork): the operand tables that only the finishing
kernel reads are built on the library's own stream, behind the packed selection pass and beside its
one-lane tail.

What the caller must not notice: two calls back to back on one shared workspace (call n + 1's builders
against call n's finishing kernel), the same on a non-default stream behind a long kernel, a call
whose rows split between the tail and the 64-bit pass, and the tables themselves -- byte for byte
what the one-pass builder writes.

Shapes: B 2, H 2, N = T = 70 and 197, D 64, k 20, ex_pred: the packed pass, the one-lane tail and
finish16_kernel all run (mxa_launch.hpp tail_width_for, finish_choice)."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from gpu_support import M, OUT_TOL, check_attn, dev, host, out_close, rnd  # noqa: F401
from oracle import mx_oracle as O

B, H, D, K = 2, 2, 64, 20
SIZES = (70, 197)
SCALE = float(np.float32(D ** -0.5))


def inputs(n, seed):
    return tuple(rnd((B, H, n, D), 10 * seed + i) for i in range(3))


# ---- rows that pack and rows that do not, in one call ------------------------------------------
def mixed_rows(n):
    """every fifth query row (shifted per head): its second 32-block scaled by 2^-20"""
    r = np.arange(n)
    return [[r[(r + 2 * h + b) % 5 == 0] for h in range(H)] for b in range(B)]


@functools.lru_cache(maxsize=None)
def mixed_case(n):
    """q, k, v with mixed_rows scaled, the oracle's result and its approximate scores"""
    q, kk, v = inputs(n, 3)
    q = q.copy()
    for b in range(B):
        for h in range(H):
            q[b, h, mixed_rows(n)[b][h], 32:] *= np.float32(2.0 ** -20)
    r = O.attention(q, kk, v, SCALE, k_top=K, pred_mode="ex_pred")
    aq, ak = O.approx_operands(q, kk, "ex_pred")
    return q, kk, v, r, O.exact_matmul_f32(aq, np.swapaxes(ak, -1, -2))


def row_packs(pred):
    """mxa_order.hpp q_bad_bits over a row: no score needs its low mantissa byte (NaN packs)"""
    u = np.ascontiguousarray(pred, np.float32).view(np.uint32)
    nan = (u & 0x7FFFFFFF) > 0x7F800000
    return ~(((u & 0xFF) != 0) & ~nan).any(-1)


@pytest.mark.parametrize("n", SIZES)
def test_mixed_case_has_both_kinds_of_row(n):
    """CPU: the scaled rows' sums of +-2^e span more than the 16 bits a packed element keeps, so the
    packed pass leaves them for the 64-bit pass; every other row packs.  Both kinds in every head."""
    _, _, _, r, pred = mixed_case(n)
    packs = row_packs(pred)
    for b in range(B):
        for h in range(H):
            want = np.ones(n, bool)
            want[mixed_rows(n)[b][h]] = False
            assert np.array_equal(packs[b, h], want), (b, h)
            assert 0 < want.sum() < n
    assert np.array_equal(r["pred"], pred)


# ---- the entry point on a workspace and a stream of the test's own -------------------------------
def bind(M, q, k, v):
    """AttnParams of the ex_pred top-k call on device tensors with fresh out, idx and mask bound"""
    p, dv, (_, _, n, t, _), keep = M.ops._attn_params(q, k, v, SCALE, K, "ex_pred", True, True, None, False, 0, None)
    res = dict(out=M.ops._bind_out(p, torch.full((B, H, n, D), float("nan"), device=dv)),
               idx=M.ops._new_idx(p, B, H, n, K, True, dv),
               mask=torch.zeros((B, H, n, (t + 31) // 32), dtype=torch.int32, device=dv))
    p.mask_out = res["mask"].data_ptr()
    return p, res, keep


def workspace(M, p):
    nbytes = M._native.lib().mxa_attention_full_workspace_bytes(ctypes.byref(p), 8)
    assert nbytes > 0
    return torch.zeros(nbytes, dtype=torch.uint8, device="cuda")


def launch(M, p, ws, stream):
    p.workspace, p.workspace_bytes = ws.data_ptr(), ws.numel()
    M._native.check(M._native.lib().mxa_attention_full(ctypes.byref(p), 8, stream), "mxa_attention_full")


def alone(M, qkv):
    """the call by itself on a workspace of its own, host arrays"""
    t = [dev(x) for x in qkv]
    p, res, _ = bind(M, *t)
    launch(M, p, workspace(M, p), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return {a: host(x) for a, x in res.items()}


@functools.lru_cache(maxsize=None)
def pair(n):
    """two calls' inputs; their results are computed once per test session on first use"""
    return inputs(n, 1), inputs(n, 2)


_ALONE = {}


def pair_alone(M, n):
    if n not in _ALONE:
        _ALONE[n] = tuple(alone(M, x) for x in pair(n))
    return _ALONE[n]


def same_bytes(got, want, what):
    for name in want:
        g, w = got[name], want[name]
        assert g.dtype == w.dtype and np.array_equal(g.view(np.uint8), w.view(np.uint8)), (what, name)


def back_to_back(M, n, stream, ahead=None):
    """both calls of pair(n) on one workspace with nothing between them, on `stream` (a torch stream, or
    None: the current one) behind ahead() queued there"""
    ta, tb = ([dev(x) for x in qkv] for qkv in pair(n))
    pa, ra, _ = bind(M, *ta)
    pb, rb, _ = bind(M, *tb)
    ws = workspace(M, pa)
    torch.cuda.synchronize()  # the inputs, outputs and workspace exist before another stream uses them
    if stream is None:
        sp = torch.cuda.current_stream().cuda_stream
        launch(M, pa, ws, sp)
        launch(M, pb, ws, sp)
    else:
        with torch.cuda.stream(stream):
            held = ahead()
            launch(M, pa, ws, stream.cuda_stream)
            launch(M, pb, ws, stream.cuda_stream)
        del held
    torch.cuda.synchronize()
    return ({a: host(x) for a, x in ra.items()}, {a: host(x) for a, x in rb.items()})


@pytest.mark.gpu
@pytest.mark.parametrize("n", SIZES)
def test_back_to_back_calls_share_a_workspace(M, n):
    """call n + 1's builders, on either stream, wait for call n's finishing kernel: each call's out,
    idx and mask words are the bytes it writes alone on a workspace of its own"""
    want = pair_alone(M, n)
    got = back_to_back(M, n, None)
    for i in range(2):
        same_bytes(got[i], want[i], f"N{n} call {i}")
    assert not np.array_equal(want[0]["idx"], want[1]["idx"])


@pytest.mark.gpu
@pytest.mark.parametrize("n", SIZES)
def test_back_to_back_calls_on_a_busy_side_stream(M, n):
    """the same on a non-default torch stream with milliseconds of matmuls queued ahead of the calls:
    the fork waits for the caller's stream, not for the host"""
    want = pair_alone(M, n)
    a = torch.randn(2048, 2048, device="cuda")

    def ahead():
        x = a
        for _ in range(8):
            x = (x @ a) * 1e-3
        return x

    got = back_to_back(M, n, torch.cuda.Stream(), ahead)
    for i in range(2):
        same_bytes(got[i], want[i], f"N{n} call {i}")


@pytest.mark.gpu
@pytest.mark.parametrize("n", SIZES)
def test_tail_rows_and_left_rows_in_a_forked_call(M, n):
    """rows the packed pass hands to the tail and rows it leaves for the 64-bit pass in every head
    (test_mixed_case_has_both_kinds_of_row), so that the packed pass, the tail, the 64-bit pass and the
    lane's builders all have work in one forked call; pred, idx and mask equal the oracle's, out within
    the output's bound"""
    q, kk, v, r, _ = mixed_case(n)
    res = M.mx_topk_attention(dev(q), dev(kk), dev(v), SCALE, k_top=K, pred_mode="ex_pred", return_scores=True,
                              return_mask=True)
    torch.cuda.synchronize()
    got = dict(out=host(res[0]), idx=host(res[1]), true=host(res[2]), pred=host(res[3]), mask=host(M.unpack_mask(res[4], n)))
    check_attn(got, r, f"N{n}")
    out_close(got["out"], r["out"], OUT_TOL, f"N{n} out")


# ---- the tables of a forked call (the rows launch without V's blocks in its grid) ---------------
def qk_tables(ws, n):
    """codes, sT, sA and the sign words of Q, then of K, out of an ex_pred call's workspace
    (attn_layout / carve_operands: 256-byte aligned regions in this order)"""
    rows, nbd = B * H * n, (D + 31) // 32
    sizes = dict(codes=rows * 32 * nbd, sT=rows * nbd * 2, sA=rows * nbd * 2, sg=rows * nbd * 4)
    off, out = 0, {}
    for side in "qk":
        for name, nbytes in sizes.items():
            out[side + "." + name] = host(ws[off:off + nbytes])
            off += (nbytes + 255) // 256 * 256
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("n", SIZES)
def test_forked_builders_write_the_one_pass_tables(M, n):
    """after one attention call, Q's and K's codes, sT, sA and sign words in the workspace are the
    bytes the one-pass row builder writes (mxa_approx_scores: rows_prep_kernel on the same layout).
    The inputs include a zero block, a NaN block, a block below the half step of its neighbour's
    scale and the tiny-scale branch (es < -121)."""
    q, kk, v = (x.copy() for x in inputs(n, 4))
    q[0, 0, 1, :32] = 0.0
    q[0, 1, 2, 40] = np.nan
    q[1, 0, 3, 33:] *= np.float32(2.0 ** -9)  # elements that round to the code 0, negative ones among them
    kk[0, 0, 4, 32:] *= np.float32(2.0 ** -125)
    kk[1, 1, 5, :32] = np.float32(-0.0)
    t = [dev(x) for x in (q, kk, v)]
    p, res, _ = bind(M, *t)  # (res holds the outputs the call writes)
    ws = workspace(M, p)
    launch(M, p, ws, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    got = qk_tables(ws, n)
    assert not np.isnan(host(res["out"])[0, 0, 0]).any()

    ps, _, _, _ = M.ops._attn_params(t[0], t[1], None, 1.0, 0, "ex_pred", False, True, None, False, 0, None)
    pred = torch.empty((B, H, n, n), device="cuda")
    ps.pred_out = pred.data_ptr()
    ws1 = torch.zeros_like(ws)
    ps.workspace, ps.workspace_bytes = ws1.data_ptr(), ws1.numel()
    M._native.check(M._native.lib().mxa_approx_scores(ctypes.byref(ps), torch.cuda.current_stream().cuda_stream),
                    "mxa_approx_scores")
    torch.cuda.synchronize()
    want = qk_tables(ws1, n)
    for name in want:
        assert np.array_equal(got[name], want[name]), (n, name, int((got[name] != want[name]).sum()))
    assert want["q.codes"].any() and want["k.sg"].any()
