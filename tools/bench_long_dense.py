"""The dense branch and a large k on rows of 1,024 keys, M.mx_topk_attention -> mxa_attention_full
(finish_qk_long_kernel), against the chain such a caller runs without it: the unchanged glue of
the patched attention forward on the drop-in modules -- mx.matmul (true QK^T), then torch softmax
(dense) or funcs.exponent_approximation, a torch matmul (pred), M.topk on the N x T matrix, torch
gather / softmax / scatter (top-k), then mx.matmul (P.V) -- as tools/bench_long_rows.py lays it
out.  The PixArt-alpha 512x512 self-attention block (workloads/PixArt/models/
MX_transformer_block.py:648-717): B = 2, H = 16, N = T = 1,024, D = 72, ex_pred; the cases dense
(self_top_k=False, exclude_timesteps, exclude_blocks) and k = 154, at widths 8 and 4.

    python tools/bench_long_dense.py [--steps 20] [--warmup 3] [--reps 3] [--cases dense,k154] [--widths 8,4] [--fused-only]

Both routes of every case are warmed up first; then per case `reps` repetitions alternate the two
routes, each timed with device events around `steps` calls.  Prints per case the median and the
spread (max - min over the repetitions) of both routes in ms per call, whether idx agrees and the
normwise relative difference of the two outputs.  One JSON line per case.
--fused-only: the fused call alone (for a kernel trace of it)."""
import argparse
import json

import torch

from ab_routes import M, agreement, alternate, chain, ms_fields

B, H, N, D, MODE = 2, 16, 1024, 72, "ex_pred"
CASES = {"dense": 0, "k154": 154}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--cases", default=",".join(CASES))
    ap.add_argument("--widths", default="8,4")
    ap.add_argument("--fused-only", action="store_true")
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    g = torch.Generator(device="cpu").manual_seed(0)
    q, k, v = (torch.randn(B, H, N, D, generator=g).to(dev) for _ in range(3))
    scale = D ** -0.5

    def fused(kt, bits):
        res = M.mx_topk_attention(q, k, v, scale, k_top=kt or 20, top_k=kt > 0, pred_mode=MODE, elem_bits=bits)
        return res[0], res[1]

    def routes(run):
        _, kt, bits = run
        r = {"fused": lambda: fused(kt, bits)}
        if not args.fused_only:
            r["chain"] = lambda: chain(q, k, v, scale, kt, MODE, bits)
        return r

    runs = [(name, CASES[name], int(w)) for name in args.cases.split(",") for w in args.widths.split(",")]
    for run, times in zip(runs, alternate(map(routes, runs), args.steps, args.warmup, args.reps)):
        name, kt, bits = run
        line = {"shape": "pixart_self_512", "case": name, "elem_bits": bits, "B_H_N_T_D_k": (B, H, N, N, D, kt), "pred_mode": MODE,
                "steps": args.steps, "reps": args.reps, **ms_fields(times)}
        if not args.fused_only:
            line.update(agreement(*(fn() for fn in routes(run).values())))
        print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
