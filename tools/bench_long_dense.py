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
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import mx_quantization_amd as M  # noqa: E402

B, H, N, D, MODE = 2, 16, 1024, 72, "ex_pred"
CASES = {"dense": 0, "k154": 154}


def timed(fn, steps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(steps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / steps


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
    M.install_dropin()
    from funcs import exponent_approximation
    from mx import matmul
    from mx.specs import apply_mx_specs
    specs = {bits: apply_mx_specs({"a_elem_format": f"int{bits}", "w_elem_format": f"int{bits}", "block_size": 32,
                                   "scale_bits": 8, "bfloat": 32, "shared_exp_method": "max", "round": "nearest"})
             for bits in (8, 4)}

    def fused(kt, bits):
        res = M.mx_topk_attention(q, k, v, scale, k_top=kt or 20, top_k=kt > 0, pred_mode=MODE, elem_bits=bits)
        return res[0], res[1]

    def chain(kt, bits):
        s = specs[bits]
        true_scores = matmul(q, k.transpose(-2, -1), mx_specs=s, mode_config="aa") * scale
        if not kt:
            return matmul(torch.softmax(true_scores, dim=-1), v, mx_specs=s, mode_config="aa"), None
        aq, ak = exponent_approximation(Q=q, K=k, mx_specs=s).exponent_based_sign()
        pred_scores = aq @ ak.transpose(-2, -1)
        _, idx = M.topk(pred_scores, kt)
        vals = true_scores.gather(dim=-1, index=idx)
        attn = torch.zeros_like(true_scores)
        attn.scatter_(-1, idx, torch.softmax(vals, dim=-1).to(attn.dtype))
        return matmul(attn, v, mx_specs=s, mode_config="aa"), idx

    runs = [(name, CASES[name], int(w)) for name in args.cases.split(",") for w in args.widths.split(",")]
    for _, kt, bits in runs:  # warm-up of both routes of every case before any timing
        for _ in range(args.warmup):
            fused(kt, bits)
            if not args.fused_only:
                chain(kt, bits)
    torch.cuda.synchronize()
    for name, kt, bits in runs:
        tf, tc = [], []
        for _ in range(args.reps):  # alternating
            tf.append(timed(lambda: fused(kt, bits), args.steps))
            if not args.fused_only:
                tc.append(timed(lambda: chain(kt, bits), args.steps))
        line = {"shape": "pixart_self_512", "case": name, "elem_bits": bits, "B_H_N_T_D_k": (B, H, N, N, D, kt), "pred_mode": MODE,
                "steps": args.steps, "reps": args.reps,
                "fused_ms_median": round(statistics.median(tf), 4), "fused_ms_spread": round(max(tf) - min(tf), 4),
                "fused_ms": [round(t, 4) for t in tf]}
        if not args.fused_only:
            (of, idf), (oc, idc) = fused(kt, bits), chain(kt, bits)
            line.update({
                "chain_ms_median": round(statistics.median(tc), 4), "chain_ms_spread": round(max(tc) - min(tc), 4),
                "chain_ms": [round(t, 4) for t in tc], "idx_equal": None if idc is None else bool(torch.equal(idf, idc)),
                "out_normwise_rel_diff": (torch.linalg.norm((of - oc).double()) / torch.linalg.norm(oc.double())).item()})
        print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
