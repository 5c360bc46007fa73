"""M.mx_topk_attention on rows of 1,024 keys (mxa_attention_long) against the chain such a caller
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
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import mx_quantization_amd as M  # noqa: E402

B, H, N, D, K_TOP = 2, 16, 1024, 72, 20
MODES = ("ex_pred", "MXINT4")


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
    specs = apply_mx_specs({"a_elem_format": "int8", "w_elem_format": "int8", "block_size": 32, "scale_bits": 8,
                            "bfloat": 32, "shared_exp_method": "max", "round": "nearest"})

    def fused(mode):
        return M.mx_topk_attention(q, k, v, scale, k_top=K_TOP, pred_mode=mode)

    def chain(mode):
        true_scores = matmul(q, k.transpose(-2, -1), mx_specs=specs, mode_config="aa") * scale
        ea = exponent_approximation(Q=q, K=k, mx_specs=specs)
        aq, ak = {"ex_pred": ea.exponent_based_sign, "MXINT4": ea.MXINT4}[mode]()
        pred_scores = aq @ ak.transpose(-2, -1)
        _, idx = M.topk(pred_scores, K_TOP)
        vals = true_scores.gather(dim=-1, index=idx)
        attn = torch.zeros_like(true_scores)
        attn.scatter_(-1, idx, torch.softmax(vals, dim=-1).to(attn.dtype))
        return matmul(attn, v, mx_specs=specs, mode_config="aa"), idx

    for mode in MODES:  # warm-up of both routes before any timing
        for _ in range(args.warmup):
            fused(mode)
            if not args.fused_only:
                chain(mode)
    torch.cuda.synchronize()
    for mode in MODES:
        tf, tc = [], []
        for _ in range(args.reps):  # alternating
            tf.append(timed(lambda: fused(mode), args.steps))
            if not args.fused_only:
                tc.append(timed(lambda: chain(mode), args.steps))
        line = {"shape": "pixart_self_512", "B_H_N_T_D_k": (B, H, N, N, D, K_TOP), "pred_mode": mode,
                "steps": args.steps, "reps": args.reps,
                "fused_ms_median": round(statistics.median(tf), 4), "fused_ms_spread": round(max(tf) - min(tf), 4),
                "fused_ms": [round(t, 4) for t in tf]}
        if not args.fused_only:
            (of, idf), (oc, idc) = fused(mode), chain(mode)
            line.update({
                "chain_ms_median": round(statistics.median(tc), 4), "chain_ms_spread": round(max(tc) - min(tc), 4),
                "chain_ms": [round(t, 4) for t in tc], "idx_equal": bool(torch.equal(idf, idc)),
                "out_normwise_rel_diff": (torch.linalg.norm((of - oc).double()) / torch.linalg.norm(oc.double())).item()})
        print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
