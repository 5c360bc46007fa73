"""The fused op and topk on rows of 4,097 .. 16,384 keys (mxa_attention_xxl: select_xxl_kernel and
finish16_xxl_kernel; mxa_topk_xxl), k <= 64 and k * 64 <= T -- torch's partial_sort regime.  The checks are
test_gpu_xl_rows.py's (check_case): kept indices, prune-mask words and scores bit for bit against the oracle,
the output within OUT_TOL and row by row (out_rows_close), the call without the scores bit-equal.
B = 1, H = 2, N = 33: two 16-row tiles and a ragged row.  (T, k) and the edge each hits:
  4097 / 16   the smallest accepted row: five chunks, one key in the last (selection strip and finishing tile)
  4097 / 64   k * 64 <= T with a full heap
  5000 / 20   a ragged last 32-block and a ragged 64-key scan step
  9249 / 20   ten chunks, 33 keys in the last: an even count beside 4097's and 5000's five, so that the
              finishing kernel's two scale buffers end on either parity
  16384 / 20, / 64   the full length, and with the full heap
  16383 / 1   a heap of one
out_rows_close asserts its precondition (eligible rows <= 15 %) itself; computed on the CPU from the oracle alone
for every case below, the largest share is 6.06 % (16384 / 64), so no case needs the bound asserted directly.
On the parent every one of these calls is refused: attn_validate answers MXA_ERR_UNSUPPORTED (NativeError -2) for
T > kXlRowsT = 4,096 at every reach, and mxa_topk_xl_nth for n > 4,096 -- read from the code, not run."""
import numpy as np
import pytest
import torch

from gpu_support import ELEM, OUT_TOL, M, attn_run, host, out_close, out_rows_close, rnd, same, same_bits, to_bits  # noqa: F401
from oracle import mx_oracle as O
from test_gpu_xl_rows import case, check_case, topk_rows

pytestmark = pytest.mark.gpu

TK = [(4097, 16), (4097, 64), (5000, 20), (9249, 20), (16384, 20), (16384, 64), (16383, 1)]


@pytest.mark.parametrize("mode", ["ex_pred", "MXINT4", "true"])
@pytest.mark.parametrize("D", [32, 72])
@pytest.mark.parametrize("T,k", TK)
def test_xxl_rows(M, T, k, D, mode):
    check_case(M, T, k, D, mode)


@pytest.mark.parametrize("T,k", [(5000, 20), (16384, 64)])
def test_xxl_rows_mxint4_elements(M, T, k):
    check_case(M, T, k, 72, "ex_pred", bits=4)


def test_xxl_rows_mask_bias(M):
    check_case(M, 9249, 20, 72, "ex_pred", biased=True)


def test_rounds_and_waves_without_a_tile(M):
    """16 heads of 257 tiles: the launch plan (finish_tile_plan) gives workgroups of three waves and nine tiles
    -- three rounds, the scale buffers carried from one round's last chunk to the next round's first -- and the
    last workgroup of a head five tiles: in its second round the third wave has none and only stages V's scales
    and meets the chunk barriers.  The oracle on each head's first and last workgroup (144 and 65 rows)."""
    T, k, D, n = 4097, 16, 32, 4097
    q, kk, v = rnd((1, 16, n, D), 70), rnd((1, 16, T, D), 71), rnd((1, 16, T, D), 72)
    got = attn_run(M, q, kk, v, 0.125, k_top=k, scores=False)
    rows = list(range(144)) + list(range(n - 65, n))
    ref = O.attention(q[:, :, rows], kk, v, 0.125, k_top=k)
    same(got["idx"][:, :, rows], np.asarray(ref["idx"]).astype(np.int64), "idx")
    out_rows_close(got["out"][:, :, rows], ref, v, "out (the first 144 and the last 65 rows)")


def test_v_nan_in_a_block_no_row_keeps(M):
    """test_gpu_xl_rows.py's check at 16,384 keys, the NaN in a chunk beyond the fourth: the block's scale is
    staged with its chunk and reaches every row's output column though no row keeps a key of the block"""
    T, k, D, c = 16384, 20, 72, 37
    q, kk, v, _, scale, ref = case(T, k, D, "ex_pred", H=1, n=4)
    free = np.setdiff1d(np.arange(T // 32), np.unique(ref["idx"] // 32))
    free = free[free >= 4 * 32]  # (32 key blocks per chunk)
    assert free.size, "a key block beyond the fourth chunk that no row keeps"
    vn = v.copy()
    vn[0, 0, 32 * free[free.size // 2] + 5, c] = np.nan
    got = attn_run(M, q, kk, v, scale, k_top=k, scores=False)["out"]
    gotn = attn_run(M, q, kk, vn, scale, k_top=k, scores=False)["out"]
    same(np.isnan(gotn), np.isnan(O.attention(q, kk, vn, scale, k_top=k)["out"]), "NaN pattern")
    assert np.isnan(gotn[..., c]).all() and not np.isnan(got).any()
    others = np.arange(D) != c
    same_bits(gotn[..., others], got[..., others], "the other columns")


# ---- topk: torch.topk on the CPU tensor is the specification (test_gpu_xl_rows.py's row families) ----------
NK = [(4097, 64), (4097, 1), (5000, 64), (5000, 1), (16384, 64), (16384, 1)]  # k: the largest allowed, and 1


@pytest.mark.parametrize("n,k,dt", [nk + (torch.float32,) for nk in NK] + [(5000, 64, torch.float16), (5000, 64, torch.bfloat16)],
                         ids=str)
def test_topk_xxl(M, n, k, dt):
    x = topk_rows(n).to(dt)
    wv, wi = torch.topk(x, k, dim=-1)
    gv, gi, gm = M.topk(x.cuda(), k, return_mask=True)
    torch.cuda.synchronize()
    same(host(gi), wi.numpy(), f"n{n} k{k} idx")
    dts = {torch.float16: "f16", torch.bfloat16: "bf16"}.get(dt)
    same_bits(to_bits(gv), to_bits(wv), f"n{n} k{k} values", dt=dts, patterns=True)
    same(host(M.unpack_mask(gm, n)), O.prune_mask(wi.numpy(), n), f"n{n} k{k} mask")
