"""Generate tests/golden/attn_int4.npz FROM THE REFERENCE ITSELF: the attention glue of
gen_golden.py (attention_glue, unchanged) under the PixArt inference spec
w_elem_format = a_elem_format = 'int4' (workloads/PixArt/scripts/mx_inference.py:106-122).

Run only where the reference tree exists (see gen_golden.py):

    python tests/golden/gen_attn4_golden.py

Fixture data only: inputs and the reference's outputs (idx stored as int16).  Keys:
  self/{q,k,v,scale,true}             q, k, v (1, 2, 70, 72), scale 72^-0.5
  self/<mode>_k20/{pred,aq,ak,idx,out}  the six approximators, k = 20; aq / ak: the first 32 rows
                                      of every head (the six operand pairs of the drop-in check)
  self/trueK_k30/{idx,out}            approx=False, k = 30
  self/dense/out                      top_k=False
  cross/{q,k,v,scale,bias,true}       q (1, 2, 64, 72), k / v (1, 2, 120, 72), the PixArt mask bias
                                      (60 valid text tokens), flush, bfloat = 16
  cross/<mode>_k20/{pred,aq,ak,idx,out}  ex_pred and MXINT4
  cross/dense/out
"""
import math
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gen_golden as GG  # noqa: E402  (imports the reference)

MODES = ("ex_pred", "partial_Q", "partial_K", "MXINT4", "two_step_leading_ones", "true_ex")
INT4 = dict(a_elem_format="int4", w_elem_format="int4")


def pack(store, tag, r, keep=("pred", "aq", "ak", "idx", "out")):
    for kk in keep:
        if kk in r:
            store[f"{tag}/{kk}"] = r[kk][..., :32, :] if kk in ("aq", "ak") else r[kk]


def main():
    store = {}
    q, k, v = (torch.from_numpy(GG.rnd((1, 2, 70, 72), 40 + s)) for s in (0, 1, 2))
    sc = 72 ** -0.5
    s4 = GG.specs(**INT4)
    store.update({"self/q": q.numpy(), "self/k": k.numpy(), "self/v": v.numpy(), "self/scale": np.float32(sc)})
    for mode in MODES:
        r = GG.attention_glue(q, k, v, s4, sc, 20, mode)
        store["self/true"] = r["true"]
        pack(store, f"self/{mode}_k20", r)
    pack(store, "self/trueK_k30", GG.attention_glue(q, k, v, s4, sc, 30, "ex_pred", approx=False), ("idx", "out"))
    pack(store, "self/dense", GG.attention_glue(q, k, v, s4, sc, 20, "ex_pred", top_k=False), ("out",))

    # the PixArt cross-attention slice of gen_golden.gen_attention, 64 query rows, at int4 with bfloat = 16
    q = torch.from_numpy(GG.rnd((1, 2, 64, 72), 50))
    k = torch.from_numpy(GG.rnd((1, 2, 120, 72), 51))
    v = torch.from_numpy(GG.rnd((1, 2, 120, 72), 52))
    mask = torch.zeros(1, 120)
    mask[:, :60] = 1
    bias = ((1 - mask) * -10000.0).unsqueeze(1)  # (B,1,T)
    attn_bias = torch.zeros([64, 120]) + bias.unsqueeze(1).repeat(1, 2, 1, 1)  # (B,H,N,T)
    sc = 1 / math.sqrt(72)
    sx = GG.specs(mx_flush_fp32_subnorms=True, bfloat=16, **INT4)
    store.update({"cross/q": q.numpy(), "cross/k": k.numpy(), "cross/v": v.numpy(), "cross/scale": np.float32(sc),
                  "cross/bias": bias.numpy()})
    for mode in ("ex_pred", "MXINT4"):
        r = GG.attention_glue(q, k, v, sx, sc, 20, mode, bias=attn_bias)
        store["cross/true"] = r["true"]
        pack(store, f"cross/{mode}_k20", r)
    pack(store, "cross/dense", GG.attention_glue(q, k, v, sx, sc, 20, "ex_pred", top_k=False, bias=attn_bias), ("out",))
    store = {kk: (vv.astype(np.int16) if kk.endswith("/idx") else vv) for kk, vv in store.items()}
    path = os.path.join(GG.OUT, "attn_int4.npz")
    np.savez_compressed(path, **store)
    print("wrote attn_int4", os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
