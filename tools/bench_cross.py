"""A fused PixArt-alpha attention block against the unfused chain of public ops, weights prepared once.

  --block cross (default): M.mx_cross_attention (with the proj Linear behind it) against M.mx_linear
      (q), M.mx_linear (kv), M.mx_topk_attention, M.mx_linear (to_out[0]) at B = 8, N = 256 image
      tokens, T = 120 text tokens, C = C_kv = 1152, H = 16 (D = 72), k = 20, the mask bias;
  --block self: M.mx_qkv_attention (with the proj Linear) against M.mx_linear (qkv),
      M.mx_topk_attention, M.mx_linear (proj) at the 256 x 256 image: B = 8, N = 256, C = 1152, H = 16,
      k = 20, no bias.  --tokens / --batch / --channels / --heads give another self-attention shape: over
      512 tokens the fused call is the *_full entry point (rows of 513 .. 1,024 keys) -- the 512 x 512
      image is --tokens 1024 --batch 2; DeiT-base at 384 x 384 (D = 64: the proj's codes straight from the
      finishing kernel) --tokens 577 --batch 8 --channels 768 --heads 12.
MXINT4 and ex_pred approximators, flush_subnormals.  --elem-bits 4: every Linear and the attention at
MXINT4 (W4A4, the reference's PixArt script; the fused call is the *_bits entry point).  --bfloat: the
bfloat setting of every op (the script runs 16).  The defaults reproduce the MXINT8 cross run.

    python tools/bench_cross.py [--block cross|self] [--elem-bits 8|4] [--bfloat 0] [--steps 20] [--warmup 3] [--reps 3]
                                [--tokens N] [--batch B] [--channels C] [--heads H]      (--block self only)

Both chains and both modes are warmed up first; then per mode `reps` repetitions alternate the
two chains, each timed with device events around `steps` calls.  Prints per mode the median
and the spread (max - min over the repetitions) of both chains in ms per call, whether idx and y
agree bit for bit and the normwise relative difference of the two y.  One JSON line per mode."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import mx_quantization_amd as M  # noqa: E402
from ab_routes import timed  # noqa: E402

B_IMG, N_IMG, T_TXT, C_IMG, H_IMG, K_TOP = 8, 256, 120, 1152, 16, 20  # the PixArt-alpha block at 256 x 256
MODES = ("MXINT4", "ex_pred")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--block", choices=("cross", "self"), default="cross")
    ap.add_argument("--elem-bits", type=int, choices=(8, 4), default=8)
    ap.add_argument("--bfloat", type=int, default=0)
    ap.add_argument("--tokens", type=int, default=None)
    ap.add_argument("--batch", type=int, default=None)
    ap.add_argument("--channels", type=int, default=None)
    ap.add_argument("--heads", type=int, default=None)
    args = ap.parse_args()
    if args.steps < 20:
        ap.error("--steps must be at least 20")
    shape_args = (args.tokens, args.batch, args.channels, args.heads)
    if args.block != "self" and any(a is not None for a in shape_args):
        ap.error("--tokens / --batch / --channels / --heads go with --block self")
    # the run's shape: the PixArt block's unless --block self names another
    N, B, C, H = (d if a is None else a for a, d in zip(shape_args, (N_IMG, B_IMG, C_IMG, H_IMG)))
    T, CKV = T_TXT, C_IMG
    if C % H:
        ap.error("--channels must be a multiple of --heads")
    pixart = (B, N, C, H) == (B_IMG, N_IMG, C_IMG, H_IMG)
    label = f"pixart_{args.block}" if pixart else f"self_B{B}_N{N}_C{C}_H{H}"
    dev = torch.device("cuda", 0)
    g = torch.Generator(device="cpu").manual_seed(0)
    D = C // H
    scale = D ** -0.5
    x, cond = torch.randn(B, N, C, generator=g).to(dev), torch.randn(B, T, CKV, generator=g).to(dev)
    lin = lambda o, i: ((torch.randn(o, i, generator=g) * i ** -0.5).to(dev), (torch.randn(o, generator=g) * 0.1).to(dev))  # noqa: E731
    (Wq, bq), (Wkv, bkv), (Wo, bo) = lin(C, C), lin(2 * C, CKV), lin(C, C)
    bias = torch.where(torch.arange(T) < T // 2, 0.0, -10000.0).reshape(1, 1, 1, T).repeat(B, 1, 1, 1).to(dev)
    kw = dict(flush_subnormals=True, bfloat=args.bfloat)
    bits = dict(elem_bits=args.elem_bits)
    prep = lambda W, gw: M.LinearWeightMX(W, gw, **kw, **bits)  # noqa: E731
    # the fused call takes the weights in head groups; mx_linear takes any grouping: one group each
    wo = prep(Wo, C)
    if args.block == "cross":
        wq_f, wkv_f = prep(Wq, D), prep(Wkv, D)
        wq_u, wkv_u = prep(Wq, C), prep(Wkv, 2 * C)

        def fused(mode):
            return M.mx_cross_attention(x, cond, wq_f, bq, wkv_f, bkv, H, scale, k_top=K_TOP, pred_mode=mode, bias=bias,
                                        proj_weight=wo, proj_bias=bo, **kw, **bits)

        def unfused(mode):
            q = M.mx_linear(x, wq_u, bq, **kw).view(B, N, H, D).transpose(1, 2)
            kv = M.mx_linear(cond, wkv_u, bkv, **kw).view(B, T, 2, H, D)
            k, v = kv[:, :, 0].transpose(1, 2), kv[:, :, 1].transpose(1, 2)
            out, idx = M.mx_topk_attention(q, k, v, scale, k_top=K_TOP, pred_mode=mode, bias=bias, **kw, **bits)
            return M.mx_linear(out.transpose(1, 2).reshape(B, N, C), wo, bo, **kw), idx
    else:
        (Wqkv, bqkv) = lin(3 * C, C)
        wqkv_f, wqkv_u = prep(Wqkv, D), prep(Wqkv, 3 * C)

        def fused(mode):
            return M.mx_qkv_attention(x, wqkv_f, bqkv, H, scale, k_top=K_TOP, pred_mode=mode, proj_weight=wo, proj_bias=bo,
                                      **kw, **bits)

        def unfused(mode):
            qkv = M.mx_linear(x, wqkv_u, bqkv, **kw).view(B, N, 3, H, D)
            q, k, v = (qkv[:, :, j].transpose(1, 2) for j in range(3))
            out, idx = M.mx_topk_attention(q, k, v, scale, k_top=K_TOP, pred_mode=mode, **kw, **bits)
            return M.mx_linear(out.transpose(1, 2).reshape(B, N, C), wo, bo, **kw), idx

    for mode in MODES:  # warm-up of both chains before any timing
        for _ in range(args.warmup):
            fused(mode)
            unfused(mode)
    torch.cuda.synchronize()
    for mode in MODES:
        tf, tu = [], []
        for _ in range(args.reps):  # alternating
            tf.append(timed(lambda: fused(mode), args.steps))
            tu.append(timed(lambda: unfused(mode), args.steps))
        (yf, idf), (yu, idu) = fused(mode), unfused(mode)
        diff = (torch.linalg.norm((yf - yu).double()) / torch.linalg.norm(yu.double())).item()
        shape = (B, N, T, C, H, K_TOP) if args.block == "cross" else (B, N, N, C, H, K_TOP)
        print(json.dumps({
            "shape": label, "B_N_T_C_H_k": shape, "pred_mode": mode, "elem_bits": args.elem_bits,
            "bfloat": args.bfloat, "steps": args.steps, "reps": args.reps,
            "fused_ms_median": round(statistics.median(tf), 4), "fused_ms_spread": round(max(tf) - min(tf), 4),
            "unfused_ms_median": round(statistics.median(tu), 4), "unfused_ms_spread": round(max(tu) - min(tu), 4),
            "fused_ms": [round(t, 4) for t in tf], "unfused_ms": [round(t, 4) for t in tu],
            "idx_equal": bool(torch.equal(idf, idu)), "y_equal": bool(torch.equal(yf, yu)),
            "y_normwise_rel_diff": diff}), flush=True)


if __name__ == "__main__":
    main()
