"""Timings of the top-k branch outside partial_sort's regime on rows of 1,025 .. 4,096 keys (mxa_attention_nth,
mxa_topk_xl_nth) beside the nearest calls the library served before: k = 20 and the dense branch at 4,096 keys.

    python tools/bench_xl_nth.py [--reps 5] [--iters 3] [--once NAME] [--dtype f32]

B = 1, 16 heads, D = 72 (PixArt-Sigma at 1024 x 1024).  Every repetition runs the cases one after another
(alternating), `iters` calls each between two events; the line per case is the median and the range of the
repetitions.  --once NAME: one call of one case and nothing else, for a kernel trace.
--dtype f16 / bf16: the 16-bit cases instead (mxa_attention_nth_dt) -- T = 4,096, k = 154 on tensors of that dtype
(finish_gather_xl_kernel; in a library built with a lower MXA_GXL_MAXK and loaded through MXA_LIB, the masked 16-bit
finish_qk_xl_kernel), the float32 call of the same shape, and the 16-bit glue chain on the drop-in modules
(tools/ab_routes.py chain)."""
import argparse
import statistics
import sys

import torch

sys.path.insert(0, ".")
import mx_quantization_amd as M  # noqa: E402


DTYPES = {"f32": torch.float32, "f16": torch.float16, "bf16": torch.bfloat16}


def cases(dtype="f32"):
    g = torch.Generator(device="cuda").manual_seed(0)
    r = lambda *s: torch.randn(*s, device="cuda", generator=g)  # noqa: E731
    q, k, v = r(1, 16, 4096, 72), r(1, 16, 4096, 72), r(1, 16, 4096, 72)
    if dtype != "f32":
        from ab_routes import chain
        q16, k16, v16 = (t.to(DTYPES[dtype]) for t in (q, k, v))
        return {f"T4096 k154 ex_pred {dtype}": lambda: M.mx_topk_attention(q16, k16, v16, 72 ** -0.5, k_top=154),
                "T4096 k154 ex_pred f32 (served before)": lambda: M.mx_topk_attention(q, k, v, 72 ** -0.5, k_top=154),
                f"T4096 k154 ex_pred {dtype} glue chain": lambda: chain(q16, k16, v16, 72 ** -0.5, 154)}
    qs, ks, vs = r(1, 16, 1279, 72), r(1, 16, 1279, 72), r(1, 16, 1279, 72)
    rows = r(65536, 4096)
    att = lambda q, k, v, **kw: (lambda: M.mx_topk_attention(q, k, v, 72 ** -0.5, **kw))  # noqa: E731
    return {"T4096 k154 ex_pred": att(q, k, v, k_top=154), "T4096 k154 MXINT4": att(q, k, v, k_top=154, pred_mode="MXINT4"),
            "T4096 k20 ex_pred (served before)": att(q, k, v, k_top=20), "T4096 dense (served before)": att(q, k, v, top_k=False),
            "T1279 k20 ex_pred": att(qs, ks, vs, k_top=20), "T1279 k16 ex_pred (served before)": att(qs, ks, vs, k_top=16),
            "topk 65536 x 4096 k128": lambda: M.topk(rows, 128), "topk 65536 x 4096 k64 (served before)": lambda: M.topk(rows, 64)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--once", default=None)
    ap.add_argument("--dtype", default="f32", choices=tuple(DTYPES))
    a = ap.parse_args()
    cs = cases(a.dtype)
    if a.once:
        cs[a.once]()
        torch.cuda.synchronize()
        return
    for fn in cs.values():  # warm-up: code objects loaded, workspaces cached
        fn()
    torch.cuda.synchronize()
    ms = {n: [] for n in cs}
    for _ in range(a.reps):
        for n, fn in cs.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.iters):
                fn()
            e1.record()
            e1.synchronize()
            ms[n].append(e0.elapsed_time(e1) / a.iters)
    for n, t in ms.items():
        print(f"{n:40s} median {statistics.median(t):9.3f} ms  min {min(t):9.3f}  max {max(t):9.3f}  ({a.reps} x {a.iters})")


if __name__ == "__main__":
    main()
