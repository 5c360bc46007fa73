"""The MXINT4 MLP and Linear (M.mx_mlp / M.mx_linear with elem_bits=4, weights prepared once)
under the reference's PixArt specs (int4 / int4, bfloat 16) against what those specs ran before
-- the drop-in mx.Linear -> F.gelu -> mx.Linear on the mx_matmul route, which re-quantizes the
weight on every call and writes the fp32 hidden matrix -- and against the MXINT8 mx_mlp /
mx_linear.  Shapes: the MLPs of DiT-XL/2 / PixArt (16,384 x 1,152 -> 4,608 -> 1,152) and
DeiT-base (50,432 x 768 -> 3,072 -> 768); the Linears 1,152 -> 3,456 and 1,152 -> 1,152 at
16,384 rows.

    python tools/bench_int4.py [--steps 20] [--warmup 3] [--reps 3] [--bfloat 16]

tools/bench_mlp.py's protocol: every chain of every shape is warmed up first; then per shape
`reps` repetitions alternate the chains, each timed with device events around `steps` calls.
One JSON line per shape: median and spread (max - min over the repetitions) per chain in ms per
call, whether y of the int4 chain equals the old route's bit for bit, the algorithmic HBM bytes
from the shapes (not measured), and the share of 32-row blocks the one-digit K loop takes (the
gate of mxa_gemm.hpp restated on the device tensors: row-block spread <= 4, weight column
spreads <= 4, no subnormal results)."""
import argparse
import importlib
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import mx_quantization_amd as M  # noqa: E402
from ab_routes import timed  # noqa: E402
from mx_quantization_amd import ops  # noqa: E402
from mx_quantization_amd.mx.elemwise_ops import quantize_elemwise_op  # noqa: E402
from mx_quantization_amd.mx.specs import apply_mx_specs  # noqa: E402

L = importlib.import_module("mx_quantization_amd.mx.linear")

MLPS = (("dit_xl2", 16384, 1152, 4608, 1152), ("deit_base", 50432, 768, 3072, 768))
LINEARS = (("qkv_1152_3456", 16384, 1152, 3456), ("proj_1152_1152", 16384, 1152, 1152))
SPECS = {  # the reference's workloads/PixArt/scripts/mx_inference.py:106-122
    'w_elem_format': 'int4', 'a_elem_format': 'int4', 'scale_bits': 8, 'shared_exp_method': 'max', 'block_size': 32,
    'bfloat': 16, 'fp': 0, 'bfloat_subnorms': True, 'round': 'nearest', 'round_mx_output': 'nearest',
    'round_output': 'nearest', 'round_weight': 'nearest', 'mx_flush_fp32_subnorms': False, 'custom_cuda': False,
    'quantize_backprop': False,
}


def old_linear(x, W, b, s):
    """mx/linear.py's mx_matmul route (the lines behind the prepared-weight test), called directly"""
    bf_in = quantize_elemwise_op(x, mx_specs=s, round=s["round_output"])
    bf_w = quantize_elemwise_op(W, mx_specs=s, round=s["round_weight"])
    out = ops.mx_matmul(bf_in.reshape(1, -1, bf_in.shape[-1]), bf_w.t().unsqueeze(0), 4, 4,
                        flush=s["mx_flush_fp32_subnorms"]).reshape(x.shape[:-1] + (W.shape[0],))
    out = quantize_elemwise_op(out, mx_specs=s, round=s["round_output"])
    bb = quantize_elemwise_op(b, mx_specs=s, round=s["round_weight"])
    return quantize_elemwise_op(out + bb, mx_specs=s, round=s["round_output"])


def unit_exps(A, s):
    """(rows, nb) float: floor(log2(block max)) of the bfloat-rounded A, -inf for an all-zero block"""
    A = quantize_elemwise_op(A, mx_specs=s, round="nearest")
    pad = (-A.shape[1]) % 32
    if pad:
        A = torch.nn.functional.pad(A, (0, pad))
    m = A.abs().reshape(A.shape[0], -1, 32).amax(-1)
    return torch.where(m > 0, torch.floor(torch.log2(m)), torch.full_like(m, float("-inf")))


def digit_share(x, W, s):
    """share of x's 32-row blocks on the one-digit K loop with the weight W"""
    ex, ew = unit_exps(x, s), unit_exps(W, s).clamp(min=-126.0)
    hi = ex.amax(-1)
    lo = torch.where(torch.isinf(ex), torch.full_like(ex, float("inf")), ex).amin(-1)
    sp = torch.where(torch.isinf(hi), torch.zeros_like(hi), hi - lo)
    pad = (-sp.shape[0]) % 32
    spb = torch.nn.functional.pad(sp, (0, pad)).reshape(-1, 32).amax(-1)
    lob = torch.nn.functional.pad(lo, (0, pad), value=float("inf")).reshape(-1, 32).amin(-1)
    wsp = (ew.amax(-1) - ew.amin(-1)).max().item()
    ok = (spb <= 4) & (wsp <= 4) & (lob - 2 + ew.min().item() - 2 >= -126)
    return round(ok.float().mean().item(), 4), int(spb.max().item()), int(wsp)


def mlp_bytes(rows, inf, hid, outf):
    """algorithmic HBM bytes of the three chains, from the shapes (codes 1 B per element, block
    exponents 2 B per 32; weight digits: one plane at 4 bits, two at 8; fc2 beyond the digit
    kernel's K reads the weight's codes, 1 B)"""
    codes = lambda r, c: r * c + r * ((c + 31) // 32) * 2  # noqa: E731
    x_prep = rows * inf * 4 + codes(rows, inf)
    fc2 = codes(rows, hid) + rows * outf * 4
    w4 = hid * inf + outf * hid
    w8 = 2 * hid * inf + (2 if hid <= 32 * 72 else 1) * outf * hid
    fused4 = x_prep + codes(rows, inf) + codes(rows, hid) + fc2 + w4
    fused8 = x_prep + codes(rows, inf) + codes(rows, hid) + fc2 + w8
    hidden = rows * hid * 4
    # the old route: bf(x), bf(W) elementwise passes (read + write fp32), both operands quantized per
    # call, fp32 product, bf(out), bias pass -- twice -- and torch's GELU over the fp32 hidden matrix
    def lin(r, i, o):
        return (2 * r * i * 4 + 2 * o * i * 4 + r * i * 4 + codes(r, i) + o * i * 4 + codes(o, i) + codes(r, i) + codes(o, i)
                + r * o * 4 + 2 * r * o * 4 + 2 * r * o * 4)
    old = lin(rows, inf, hid) + 2 * hidden + lin(rows, hid, outf)
    return fused4, old, fused8



def stats(ts):
    return {"ms_median": round(statistics.median(ts), 4), "ms_spread": round(max(ts) - min(ts), 4), "ms": [round(t, 4) for t in ts]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--bfloat", type=int, default=16)
    ap.add_argument("--only", default="", help="comma-separated shape names")
    args = ap.parse_args()
    if args.steps < 20:
        ap.error("--steps must be at least 20")
    dev = torch.device("cuda", 0)
    g = torch.Generator(device="cpu").manual_seed(0)
    bf = args.bfloat
    s = apply_mx_specs(dict(SPECS, bfloat=bf))
    assert L.fused_elem_bits(s) == 4
    only = set(filter(None, args.only.split(",")))
    cases = []
    for name, rows, inf, hid, outf in MLPS:
        if only and name not in only:
            continue
        x = torch.randn(rows, inf, generator=g).to(dev)
        W1, b1 = (torch.randn(hid, inf, generator=g) * inf ** -0.5).to(dev), (torch.randn(hid, generator=g) * 0.1).to(dev)
        W2, b2 = (torch.randn(outf, hid, generator=g) * hid ** -0.5).to(dev), (torch.randn(outf, generator=g) * 0.1).to(dev)
        q1, q2 = M.LinearWeightMX(W1, hid, False, bf, elem_bits=4), M.LinearWeightMX(W2, outf, False, bf, elem_bits=4)
        e1, e2 = M.LinearWeightMX(W1, hid, False, bf), M.LinearWeightMX(W2, outf, False, bf)
        a = lambda x=x, q1=q1, b1=b1, q2=q2, b2=b2: M.mx_mlp(x, q1, b1, q2, b2, act="gelu_tanh", bfloat=bf)  # noqa: E731
        b = lambda x=x, W1=W1, b1=b1, W2=W2, b2=b2: old_linear(  # noqa: E731
            torch.nn.functional.gelu(old_linear(x, W1, b1, s), approximate="tanh"), W2, b2, s)
        c = lambda x=x, e1=e1, b1=b1, e2=e2, b2=b2: M.mx_mlp(x, e1, b1, e2, b2, act="gelu_tanh", bfloat=bf)  # noqa: E731
        _, _, act = M.mx_mlp(x, q1, b1, q2, b2, act="gelu_tanh", bfloat=bf, return_hidden=True)
        share = {"fc1": digit_share(x, W1, s), "fc2": digit_share(act, W2, s)}
        del act
        cases.append((name, "mlp", (rows, inf, hid, outf), a, b, c, share))
    for name, rows, inf, outf in LINEARS:
        if only and name not in only:
            continue
        x = torch.randn(rows, inf, generator=g).to(dev)
        W, bb = (torch.randn(outf, inf, generator=g) * inf ** -0.5).to(dev), (torch.randn(outf, generator=g) * 0.1).to(dev)
        q, e = M.LinearWeightMX(W, outf, False, bf, elem_bits=4), M.LinearWeightMX(W, outf, False, bf)
        a = lambda x=x, q=q, bb=bb: M.mx_linear(x, q, bb, bfloat=bf)  # noqa: E731
        b = lambda x=x, W=W, bb=bb: old_linear(x, W, bb, s)  # noqa: E731
        c = lambda x=x, e=e, bb=bb: M.mx_linear(x, e, bb, bfloat=bf)  # noqa: E731
        cases.append((name, "linear", (rows, inf, outf), a, b, c, {"linear": digit_share(x, W, s)}))
    for case in cases:  # warm-up of every chain of every shape before any timing
        for _ in range(args.warmup):
            for fn in case[3:6]:
                fn()
    torch.cuda.synchronize()
    for name, kind, shape, a, b, c, share in cases:
        ta, tb, tc = [], [], []
        for _ in range(args.reps):  # alternating
            ta.append(timed(a, args.steps))
            tb.append(timed(b, args.steps))
            tc.append(timed(c, args.steps))
        ya, yb = a(), b()
        same = (ya.view(torch.int32) == yb.view(torch.int32)) | (ya.isnan() & yb.isnan())
        out = {"shape": name, "kind": kind, "dims": shape, "bfloat": bf, "steps": args.steps, "reps": args.reps,
               "int4_prepared": stats(ta), "int4_mx_matmul_route": stats(tb), "int8_prepared": stats(tc),
               "y_int4_vs_old_route_mismatches": int((~same).sum().item()), "y_elements": ya.numel(),
               "int4_beats_old_route_by_more_than_its_spread": statistics.median(tb) - statistics.median(ta) > max(tb) - min(tb),
               "digit_share_maxrowspread_maxcolspread": share}
        if kind == "mlp":
            b4, bo, b8 = mlp_bytes(*shape)
            out["algorithmic_MB"] = {"int4_prepared": round(b4 / 1e6, 1), "int4_mx_matmul_route": round(bo / 1e6, 1),
                                     "int8_prepared": round(b8 / 1e6, 1)}
        print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
