"""attn_long.npz: the reference's glue on rows of 1,000 keys (the long-row fused op's fixture).

Run where gen_golden.py runs (the reference checkout at MXA_REFERENCE):
    python tests/golden/gen_long_rows_golden.py
It imports attention_glue, specs and rnd from gen_golden.py, which stays as it is: the
mx_quant branch of PixArt's MXSelfAttention.forward (MX_transformer_block.py:648-717) on
q (1, 1, 32, 72), k and v (1, 1, 1000, 72), k_top 20, scale 1 / sqrt(72), for ex_pred and
MXINT4.  Stored: the inputs, `true` once, then per mode `pred`, `idx` (int16) and `out`.
N = 32 keeps the file under 1 MiB (two float32 (32, 1000) score matrices per mode do not
compress); the rows' length, which the fixture is about, is not cut.
"""
import math
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from gen_golden import OUT, attention_glue, rnd, specs  # noqa: E402

N, T, D, K = 32, 1000, 72, 20


def main():
    q = torch.from_numpy(rnd((1, 1, N, D), 0))
    k = torch.from_numpy(rnd((1, 1, T, D), 1))
    v = torch.from_numpy(rnd((1, 1, T, D), 2))
    sc = 1 / math.sqrt(D)
    store = dict(q=q.numpy(), k=k.numpy(), v=v.numpy(), scale=np.float32(sc), k_top=np.int32(K))
    for mode in ("ex_pred", "MXINT4"):
        r = attention_glue(q, k, v, specs(), sc, K, mode)
        if "true" in store:
            assert np.array_equal(store["true"], r["true"])
        store["true"] = r["true"]
        store[f"{mode}/pred"] = r["pred"]
        store[f"{mode}/idx"] = r["idx"].astype(np.int16)
        store[f"{mode}/out"] = r["out"]
    path = os.path.join(OUT, "attn_long.npz")
    np.savez_compressed(path, **store)
    print("wrote", path, os.path.getsize(path), "bytes")
    assert os.path.getsize(path) < (1 << 20)


if __name__ == "__main__":
    main()
