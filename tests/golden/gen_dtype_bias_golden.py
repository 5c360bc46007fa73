"""attn_dtype_bias.npz (+ attn_dtype_bias_g32.npz, attn_dtype_bias_ac.npz): the reference's glue with a score bias on float16 /
bfloat16 tensors and under torch.autocast (the fixture of tests/test_gpu_dtype.py's bias cases).

Run where gen_golden.py runs (the reference checkout at MXA_REFERENCE):
    python tests/golden/gen_dtype_bias_golden.py
It imports mx, approx_ops, specs and rnd through gen_golden.py, which stays as it is, and restates
attention_glue_t with attention_glue's two bias lines exactly as the modules have them
(MX_transformer_block.py:821-822): `true_scores += bias` in place -- the sum stays in the scores'
dtype -- and `pred = pred + bias` out of place, which torch promotes to float32 when pred is a
16-bit autocast result and the bias float32.  Every result is stored in the dtype the reference
returns: 16-bit tensors as uint16 patterns, float32 as float32, idx as int16.

Inputs are stored once, as float16 patterns: the bfloat16 tensors are their .to(bfloat16)
(round to nearest even, the same on every device), the autocast case's float32 q, k, v their
.float().  The shapes are tests/bias_cases.py's, one per finishing kernel with a 16-bit
instantiation; DENSE_MFMA runs on the first two heads of GATHER16's tensors, DENSE_ROWS on
GATHER32's.  Three files, each under 1 MiB (one would hold 1.5 MiB): the dtype cases, those of the
300-key shape (GATHER32, DENSE_ROWS), and the autocast ones, which read attn_dtype_bias.npz's inputs.
"""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from gen_golden import OUT, _bits, approx_ops, mx, rnd, specs  # noqa: E402

SHAPES = {"g16": (2, 3, 40, 77, 48, 20), "mfma": (2, 2, 40, 130, 64, 65), "g32": (2, 2, 40, 300, 72, 129)}
DT = {"f16": torch.float16, "bf16": torch.bfloat16}


def glue(q, k, v, s, scale, k_top, mode, bias, top_k=True):
    res = {}
    true_scores = mx.matmul(q, k.transpose(-2, -1), mx_specs=s, mode_config='aa')
    true_scores = true_scores * scale
    if bias is not None:
        true_scores += bias
    res["true"] = true_scores
    if top_k:
        aq, ak = approx_ops(q, k, s, mode)
        pred = aq @ ak.transpose(-2, -1)
        if bias is not None:
            pred = pred + bias
        res["pred"] = pred
        _, idx = torch.topk(pred, k_top, dim=-1, largest=True, sorted=True)
        vals = true_scores.gather(dim=-1, index=idx)
        res["idx"] = idx
        attn = torch.zeros_like(true_scores)
        attn.scatter_(-1, idx, torch.softmax(vals, dim=-1).to(attn.dtype))
    else:
        attn = torch.softmax(true_scores, dim=-1)
    res["out"] = mx.matmul(attn, v, mx_specs=s, mode_config='aa')
    return {kk: (vv.numpy().astype(np.int16) if vv.dtype == torch.int64 else
                 (vv.numpy() if vv.dtype == torch.float32 else _bits(vv))) for kk, vv in res.items()}


def main():
    s = specs()
    out, ac = {}, {}
    x16 = {}
    for j, (tag, (B, H, N, T, D, _)) in enumerate(SHAPES.items()):
        x16[tag] = [torch.from_numpy(rnd(shp, 70 + 10 * j + i)).to(torch.float16)
                    for i, shp in enumerate(((B, H, N, D), (B, H, T, D), (B, H, T, D)))]
        x16[tag].append(torch.from_numpy(rnd((H, N, T), 75 + 10 * j, 2.0)).to(torch.float16))  # a real-valued (H, N, T) bias
        for n, t in zip(("q", "k", "v", "bias"), x16[tag]):
            out[f"{tag}/{n}"] = _bits(t)
    for name, dt in DT.items():
        x = {tag: [t.to(dt) for t in ts] for tag, ts in x16.items()}
        for tag, (B, H, N, T, D, k_top) in SHAPES.items():
            if (tag, name) == ("g32", "bf16"):
                continue
            q, k, v, bias = x[tag]
            for mode in (("ex_pred", "MXINT4") if tag == "g16" else ("ex_pred",)):
                r = glue(q, k, v, s, D ** -0.5, k_top, mode, bias)
                assert r["out"].dtype == np.uint16 and r["pred"].dtype == np.uint16
                if tag == "g16":
                    if f"{name}/g16/true" in out:
                        assert np.array_equal(out[f"{name}/g16/true"], r["true"])
                    out[f"{name}/g16/true"] = r["true"]  # (the same for both modes)
                    out[f"{name}/g16/{mode}/pred"] = r["pred"]
                out[f"{name}/{tag}/{mode}/idx"], out[f"{name}/{tag}/{mode}/out"] = r["idx"], r["out"]
        # the dense branch: DENSE_MFMA (the first two heads of g16), DENSE_ROWS (the g32 shape)
        q, k, v, bias = x["g16"]
        out[f"{name}/dense_mfma/out"] = glue(q[:, :2], k[:, :2], v[:, :2], s, 48 ** -0.5, 0, "ex_pred", bias[:2], top_k=False)["out"]
        q, k, v, bias = x["g32"]
        out[f"{name}/dense_rows/out"] = glue(q, k, v, s, 72 ** -0.5, 0, "ex_pred", bias, top_k=False)["out"]
    # float32 q, k, v under torch.autocast with a float32 bias: a real-valued (B, H, N, T) one and the (B, 1, 1, T) mask
    B, H, N, T, D, k_top = SHAPES["g16"]
    q, k, v = (t.float() for t in x16["g16"][:3])
    real = torch.from_numpy(rnd((B, H, N, T), 99, 2.0))
    mask = torch.zeros((B, 1, 1, T))
    mask[0, ..., 50:], mask[1, ..., 33:] = -10000.0, -10000.0
    ac["real/bias"], ac["mask/bias"] = real.numpy(), mask.numpy()
    for name, dt in DT.items():
        for btag, bias in (("real", real), ("mask", mask)):
            with torch.autocast("cpu", dtype=dt):
                r = glue(q, k, v, s, D ** -0.5, k_top, "ex_pred", bias)
                rd = glue(q, k, v, s, D ** -0.5, k_top, "ex_pred", bias, top_k=False)
            assert r["true"].dtype == np.uint16 and r["out"].dtype == np.uint16
            for key in ("true", "pred", "idx", "out"):
                ac[f"{name}/{btag}/{key}"] = r[key]
            ac[f"{name}/{btag}/dense/out"] = rd["out"]
            print(name, btag, "pred dtype", r["pred"].dtype)
    big = {n: out.pop(n) for n in list(out) if "g32/" in n or "dense_rows/" in n}
    for fname, d in (("attn_dtype_bias.npz", out), ("attn_dtype_bias_g32.npz", big), ("attn_dtype_bias_ac.npz", ac)):
        path = os.path.join(OUT, fname)
        np.savez_compressed(path, **d)
        print("wrote", path, os.path.getsize(path), "bytes")
        assert os.path.getsize(path) < (1 << 20)


if __name__ == "__main__":
    main()
