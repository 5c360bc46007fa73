"""Timings of top-k attention on rows of 4,097 .. 16,384 keys (mxa_attention_xxl) beside the standing call at
4,096 keys (mxa_attention_xl's kernels), and of mxa_topk_xxl.

    python tools/bench_xxl.py [--reps 5] [--iters 3] [--once NAME]

B = 1, 16 heads, D = 72, k = 20, ex_pred (PixArt-Sigma: N = T = 4,096 at 1024 x 1024, 16,384 on the 2K
checkpoint).  Every repetition runs the cases one after another (alternating), `iters` calls each between two
events; the line per case is the median and the range of the repetitions, and the cost per query row and key
(ns) that the per-length comparison uses.  T = 4,097 runs the new kernels at the old length: the selection's
cost per key there against T = 4,096 separates the design (per-chunk strip, tables through L2) from the length.
--once NAME: one call of one case and nothing else, for a kernel trace."""
import argparse
import statistics
import sys

import torch

sys.path.insert(0, ".")
import mx_quantization_amd as M  # noqa: E402


def cases():
    g = torch.Generator(device="cuda").manual_seed(0)
    r = lambda *s: torch.randn(*s, device="cuda", generator=g)  # noqa: E731
    cs = {}
    for T, bits in ((4096, 8), (4097, 8), (16384, 8), (16384, 4)):
        q, k, v = r(1, 16, T, 72), r(1, 16, T, 72), r(1, 16, T, 72)
        cs[f"T{T} k20 ex_pred w{bits}"] = (lambda q=q, k=k, v=v, bits=bits: M.mx_topk_attention(q, k, v, 72 ** -0.5, k_top=20, elem_bits=bits),
                                           16 * T * T)
    rows = r(16384, 16384)
    cs["topk 16384 x 16384 k20"] = (lambda: M.topk(rows, 20), 16384 * 16384)
    return cs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--once", default=None)
    a = ap.parse_args()
    cs = cases()
    if a.once:
        cs[a.once][0]()
        torch.cuda.synchronize()
        return
    for fn, _ in cs.values():  # warm-up: code objects loaded, workspaces cached
        fn()
    torch.cuda.synchronize()
    ms = {n: [] for n in cs}
    for _ in range(a.reps):
        for n, (fn, _) in cs.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.iters):
                fn()
            e1.record()
            e1.synchronize()
            ms[n].append(e0.elapsed_time(e1) / a.iters)
    for n, t in ms.items():
        med = statistics.median(t)
        print(f"{n:28s} median {med:9.3f} ms  min {min(t):9.3f}  max {max(t):9.3f}  ({a.reps} x {a.iters})  "
              f"{med * 1e6 / cs[n][1]:.4f} ns per row and key")


if __name__ == "__main__":
    main()
