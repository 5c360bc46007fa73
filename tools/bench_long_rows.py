"""M.mx_topk_attention on rows of 1,024 keys (select_long_kernel, finish16_kernel) against the chain such a caller
had to run before it: the unchanged glue of the patched attention forward on the drop-in modules
-- mx.matmul (true QK^T), funcs.exponent_approximation and a torch matmul (pred), M.topk on the
N x T matrix (torch's CPU order), torch gather / softmax / scatter, mx.matmul (P.V) -- laid out
as tests/glue_deit.py lays out DeiT's.  The PixArt-alpha 512x512 self-attention block
(workloads/PixArt/models/MX_transformer_block.py:624-717): B = 2, H = 16, N = T = 1,024, D = 72,
k = 20, ex_pred and MXINT4.

    python tools/bench_long_rows.py [--steps 20] [--warmup 3] [--reps 3] [--fused-only]

Both routes and both modes are warmed up first; then per mode `reps` repetitions alternate the
two routes, each timed with device events around `steps` calls.  Prints per mode the median and
the spread (max - min over the repetitions) of both routes in ms per call, whether idx agrees
and the normwise relative difference of the two outputs.  One JSON line per mode.
--fused-only: the fused call alone (for a kernel trace of it)."""
import argparse
import json

import torch

from ab_routes import M, agreement, alternate, chain, ms_fields

B, H, N, D, K_TOP = 2, 16, 1024, 72, 20
MODES = ("ex_pred", "MXINT4")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--fused-only", action="store_true")
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    g = torch.Generator(device="cpu").manual_seed(0)
    q, k, v = (torch.randn(B, H, N, D, generator=g).to(dev) for _ in range(3))
    scale = D ** -0.5

    def fused(mode):
        return M.mx_topk_attention(q, k, v, scale, k_top=K_TOP, pred_mode=mode)

    def routes(mode):
        r = {"fused": lambda: fused(mode)}
        if not args.fused_only:
            r["chain"] = lambda: chain(q, k, v, scale, K_TOP, mode)
        return r

    for mode, times in zip(MODES, alternate(map(routes, MODES), args.steps, args.warmup, args.reps)):
        line = {"shape": "pixart_self_512", "B_H_N_T_D_k": (B, H, N, N, D, K_TOP), "pred_mode": mode,
                "steps": args.steps, "reps": args.reps, **ms_fields(times)}
        if not args.fused_only:
            line.update(agreement(*(fn() for fn in routes(mode).values())))
        print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
