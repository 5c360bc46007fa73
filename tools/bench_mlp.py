"""M.mx_mlp against the unfused chain M.mx_linear -> torch.nn.functional.gelu -> M.mx_linear at the
MLP shapes of DeiT-base (50,432 x 768 -> 3,072 -> 768) and DiT-XL/2 (16,384 x 1,152 -> 4,608 ->
1,152), both GELU forms, weights prepared once.

    python tools/bench_mlp.py [--steps 20] [--warmup 3] [--reps 3]

Every shape and chain is warmed up first; then per shape `reps` repetitions alternate the
two chains, each timed with device events around `steps` calls.  Prints per shape the median
and the spread (max - min over the repetitions) of both chains in ms per call, the normwise
relative difference of the two y, and the algorithmic HBM bytes of both chains computed from
the shapes (not measured).  One JSON line per shape."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import mx_quantization_amd as M  # noqa: E402
from ab_routes import timed  # noqa: E402

SHAPES = (("deit_base", 50432, 768, 3072, 768), ("dit_xl2", 16384, 1152, 4608, 1152))


def algorithmic_bytes(rows, inf, hid, outf):
    """Bytes each chain must move through HBM, from the shapes: operands read once and results
    written once per kernel (weights: fc1's digits 2 B per element, fc2's codes 1 B; block
    exponents 2 B per 32 elements)."""
    codes = lambda r, c: r * c + r * ((c + 31) // 32) * 2  # noqa: E731  MXINT8 rows + exponents
    x_prep = rows * inf * 4 + codes(rows, inf)              # rows_prep(x): read fp32, write codes
    w = 2 * hid * inf + hid * 4 + outf * hid + outf * (hid // 32) * 2 + outf * 4
    fc2 = codes(rows, hid) + rows * outf * 4                # read the hidden codes, write y
    fused = x_prep + codes(rows, inf) + codes(rows, hid) + fc2 + w
    hidden = rows * hid * 4
    unfused = (x_prep + codes(rows, inf) + hidden  # fc1 writes the fp32 hidden matrix
               + 2 * hidden                        # torch's GELU reads and rewrites it
               + hidden + codes(rows, hid)         # rows_prep reads it, writes the codes
               + fc2 + w)
    return fused, unfused



def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=3)
    args = ap.parse_args()
    if args.steps < 20:
        ap.error("--steps must be at least 20")
    dev = torch.device("cuda", 0)
    g = torch.Generator(device="cpu").manual_seed(0)
    cases = []
    for name, rows, inf, hid, outf in SHAPES:
        x = torch.randn(rows, inf, generator=g).to(dev)
        W1, b1 = (torch.randn(hid, inf, generator=g) * inf ** -0.5).to(dev), (torch.randn(hid, generator=g) * 0.1).to(dev)
        W2, b2 = (torch.randn(outf, hid, generator=g) * hid ** -0.5).to(dev), (torch.randn(outf, generator=g) * 0.1).to(dev)
        w1, w2 = M.LinearWeightMX(W1, hid), M.LinearWeightMX(W2, outf)
        for act in ("gelu", "gelu_tanh"):
            approx = "tanh" if act == "gelu_tanh" else "none"
            fused = lambda x=x, w1=w1, b1=b1, w2=w2, b2=b2, act=act: M.mx_mlp(x, w1, b1, w2, b2, act=act)  # noqa: E731
            unfused = lambda x=x, w1=w1, b1=b1, w2=w2, b2=b2, approx=approx: M.mx_linear(  # noqa: E731
                torch.nn.functional.gelu(M.mx_linear(x, w1, b1), approximate=approx), w2, b2)
            cases.append((name, act, (rows, inf, hid, outf), fused, unfused))
    for _, _, _, fused, unfused in cases:  # warm-up of every shape before any timing
        for _ in range(args.warmup):
            fused()
            unfused()
    torch.cuda.synchronize()
    for name, act, shape, fused, unfused in cases:
        tf, tu = [], []
        for _ in range(args.reps):  # alternating
            tf.append(timed(fused, args.steps))
            tu.append(timed(unfused, args.steps))
        yf, yu = fused(), unfused()
        diff = (torch.linalg.norm((yf - yu).double()) / torch.linalg.norm(yu.double())).item()
        bf, bu = algorithmic_bytes(*shape)
        print(json.dumps({
            "shape": name, "act": act, "rows_in_hidden_out": shape, "steps": args.steps, "reps": args.reps,
            "fused_ms_median": round(statistics.median(tf), 4), "fused_ms_spread": round(max(tf) - min(tf), 4),
            "unfused_ms_median": round(statistics.median(tu), 4), "unfused_ms_spread": round(max(tu) - min(tu), 4),
            "fused_ms": [round(t, 4) for t in tf], "unfused_ms": [round(t, 4) for t in tu],
            "y_normwise_rel_diff": diff, "fused_algorithmic_MB": round(bf / 1e6, 1),
            "unfused_algorithmic_MB": round(bu / 1e6, 1)}), flush=True)


if __name__ == "__main__":
    main()
