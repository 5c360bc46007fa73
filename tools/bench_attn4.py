"""The MXINT4 attention core, M.mx_topk_attention(.., elem_bits=4), against
the 8-bit fused call at the same shape and against what a W4A4 caller ran before it: the unchanged
glue of the patched attention forward on the drop-in modules under the int4 spec -- mx.matmul
(true QK^T), funcs.exponent_approximation and a torch matmul (pred), M.topk on the N x T matrix,
torch gather / softmax / scatter, mx.matmul (P.V) -- as tools/bench_long_rows.py lays it out.
PixArt-alpha shapes (workloads/PixArt/models/MX_transformer_block.py:624-717, :765-860; the spec
of workloads/PixArt/scripts/mx_inference.py:106-122), ex_pred, k = 20, D = 72:
  self_256    B 8, H 16, N = T = 256
  self_512    B 2, H 16, N = T = 1,024
  cross       B 8, H 16, N = 256, T = 120, the mask bias (60 valid text tokens)

    python tools/bench_attn4.py [--steps 20] [--warmup 3] [--reps 3] [--only fused4|fused8] [--shapes a,b]

The three routes are warmed up first; then per shape `reps` repetitions alternate them, each timed
with device events around `steps` calls.  Prints per shape the median and the spread (max - min
over the repetitions) of each route in ms per call, whether idx agrees between the 4-bit call and
the chain and the normwise relative difference of their outputs.  One JSON line per shape.
--only: one fused call alone (for a kernel trace of it)."""
import argparse
import json

import torch

from ab_routes import M, agreement, alternate, chain, ms_fields

H, D, K_TOP, MODE = 16, 72, 20, "ex_pred"
SHAPES = {"self_256": (8, 256, 256, False), "self_512": (2, 1024, 1024, False), "cross": (8, 256, 120, True)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--only", choices=("fused4", "fused8"))
    ap.add_argument("--shapes", default=",".join(SHAPES))
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    scale = D ** -0.5
    for name in args.shapes.split(","):
        B, N, T, masked = SHAPES[name]
        g = torch.Generator(device="cpu").manual_seed(0)
        q = torch.randn(B, H, N, D, generator=g).to(dev)
        k, v = (torch.randn(B, H, T, D, generator=g).to(dev) for _ in range(2))
        bias = None
        if masked:
            bias = torch.zeros(B, 1, 1, T, device=dev)
            bias[..., T // 2:] = -10000.0

        def fused(bits):
            return M.mx_topk_attention(q, k, v, scale, k_top=K_TOP, pred_mode=MODE, bias=bias, elem_bits=bits)

        routes = {"fused4": lambda: fused(4), "fused8": lambda: fused(8),
                  "chain4": lambda: chain(q, k, v, scale, K_TOP, MODE, 4, bias)}
        if args.only:
            routes = {args.only: routes[args.only]}
        times, = alternate([routes], args.steps, args.warmup, args.reps)
        line = {"shape": name, "B_H_N_T_D_k": (B, H, N, T, D, K_TOP), "pred_mode": MODE, "steps": args.steps,
                "reps": args.reps, **ms_fields(times)}
        if not args.only:
            line.update(agreement(routes["fused4"](), routes["chain4"]()))
        print(json.dumps(line), flush=True)
        del q, k, v


if __name__ == "__main__":
    main()
