"""float16 / bfloat16 tensors and torch.autocast score dtypes on rows of 513 .. 4,096 keys on the device
(mx_topk_attention -> mxa_attention_dt -> the XDT forms of finish16_kernel LONG, finish_qk_long_kernel,
finish16_xl_kernel and finish_qk_xl_kernel), against the reference's own run
(tests/golden/gen_long_dtype_golden.py -> attn_long_dtype.npz; the cases: long_dtype_cases.py).

Bit-exact: the kept indices, the recorded true / approximate score rows, the NaN pattern of the output (every float16
top-k case carries all-zero P blocks, which float16 quantizes to NaN).  Tolerance: the output's finite elements,
normwise, test_gpu_dtype.py's TOL (the reference's P.V order is unpinned).  q, k, v are drawn as the generator drew
them; q's recorded bit patterns are compared first."""
import numpy as np
import pytest
import torch

import long_dtype_cases as LD
from gpu_support import M, from_bits, host, load, out_close, rnd, same, to_bits, to_f32  # noqa: F401
from test_gpu_dtype import TOL

pytestmark = pytest.mark.gpu
TDT = {"f32": torch.float32, "f16": torch.float16, "bf16": torch.bfloat16}


@pytest.fixture(scope="module")
def F():
    return load("attn_long_dtype.npz")


@pytest.mark.parametrize("c", LD.CASES, ids=LD.case_id)
def test_long_rows_dtype(M, F, c):
    pre, odt = LD.case_id(c), c.ac or c.dt
    shapes = ((LD.B, LD.H, LD.N, c.D), (LD.B, LD.H, c.T, c.D), (LD.B, LD.H, c.T, c.D))
    q, k, v = (torch.from_numpy(rnd(shp, c.seed + i)).to(TDT[c.dt]).cuda() for i, shp in enumerate(shapes))
    same(to_bits(q), F[pre + "/q"], pre + " the draw of q")
    kw = dict(k_top=c.k, pred_mode=c.mode) if c.k else dict(top_k=False)
    if c.bias:
        kw["bias"] = torch.from_numpy(rnd((LD.H, LD.N, c.T), c.seed + 3, 2.0)).to(TDT[c.dt]).cuda()
    if c.ac:
        kw["autocast"] = TDT[c.ac]
    out, idx, true_s, pred_s = M.mx_topk_attention(q, k, v, c.D ** -0.5, return_scores=True, **kw)
    assert out.dtype == TDT[odt]
    same(host(true_s)[:, :, :4], to_f32(F[pre + "/true"], odt), pre + " true")
    if c.k:
        same(host(idx), F[pre + "/idx"].astype(np.int64), pre + " idx")
        same(host(pred_s)[:, :, :4], to_f32(F[pre + "/pred"], odt), pre + " pred")
    else:
        assert idx is None
    ref = to_f32(F[pre + "/out"], odt)
    if c.k and odt == "f16":  # the NaN pattern compared below is not an empty one
        assert np.isnan(ref).any(), pre
    out_close(host(out, f32=True), ref, TOL[odt], pre + " out")
