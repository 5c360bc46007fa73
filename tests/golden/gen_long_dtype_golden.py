"""attn_long_dtype.npz: the reference's attention glue on float16 / bfloat16 tensors and under torch.autocast on rows
of 513 .. 4,096 keys (the fixture of tests/test_gpu_long_dtype.py; the cases are tests/long_dtype_cases.py's).

Run where gen_golden.py runs (the reference checkout at MXA_REFERENCE), on the CPU:
    python tests/golden/gen_long_dtype_golden.py
It imports attention_glue_t, specs, rnd and _bits from gen_golden.py, which stays as it is, and for the case with a
score bias the glue of gen_dtype_bias_golden.py.  k and v are not stored (the file stays under 1 MiB): generator and
test both draw q, k, v (and the bias, times 2) with rnd(shape, seed + i) followed by .to(dtype).  Per case the file
holds q's bit patterns, which guard the draw, idx as int16, out as the dtype's bit patterns, and true / pred for the
first four query rows of each head.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [HERE, os.path.dirname(HERE)]
from gen_dtype_bias_golden import glue  # noqa: E402
from gen_golden import OUT, _bits, attention_glue_t, rnd, specs  # noqa: E402
import long_dtype_cases as LD  # noqa: E402

TDT = {"f32": torch.float32, "f16": torch.float16, "bf16": torch.bfloat16}


def draw(c):
    shapes = ((LD.B, LD.H, LD.N, c.D), (LD.B, LD.H, c.T, c.D), (LD.B, LD.H, c.T, c.D))
    q, k, v = (torch.from_numpy(rnd(shp, c.seed + i)).to(TDT[c.dt]) for i, shp in enumerate(shapes))
    bias = torch.from_numpy(rnd((LD.H, LD.N, c.T), c.seed + 3, 2.0)).to(TDT[c.dt]) if c.bias else None
    return q, k, v, bias


def main():
    s, out = specs(), {}
    for c in LD.CASES:
        q, k, v, bias = draw(c)
        sc, top_k = c.D ** -0.5, c.k != 0
        with torch.autocast("cpu", dtype=TDT[c.ac or "f16"], enabled=c.ac is not None):
            r = glue(q, k, v, s, sc, c.k, c.mode, bias, top_k=top_k) if c.bias else attention_glue_t(q, k, v, s, sc, c.k, c.mode, top_k=top_k)
        pre = LD.case_id(c)
        assert r["out"].dtype == np.uint16 and r["true"].dtype == np.uint16, pre
        out[pre + "/q"] = q.numpy() if c.dt == "f32" else _bits(q)
        out[pre + "/out"], out[pre + "/true"] = r["out"], r["true"][:, :, :4]
        if top_k:
            assert r["pred"].dtype == np.uint16, pre
            out[pre + "/idx"], out[pre + "/pred"] = r["idx"], r["pred"][:, :, :4]
        print(pre, "NaN share of out", float(np.isnan(torch.from_numpy(r["out"].view(np.int16)).view(TDT[c.ac or c.dt]).float().numpy()).mean()))
    path = os.path.join(OUT, "attn_long_dtype.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")
    assert os.path.getsize(path) < (1 << 20)


if __name__ == "__main__":
    main()
