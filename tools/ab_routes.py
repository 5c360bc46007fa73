"""What the A/B tools of the fused attention share (bench_long_rows.py, bench_attn4.py,
bench_long_dense.py; timed also bench_cross.py, bench_int4.py, bench_mlp.py): the device-event
timer, the chain a caller runs without the fused op -- the unchanged glue of the patched attention
forward on the drop-in modules, laid out as tests/glue_deit.py lays out DeiT's -- the
warm-up-all-then-alternate protocol and the JSON line's timing and agreement fields."""
import functools
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import mx_quantization_amd as M  # noqa: E402


def timed(fn, steps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(steps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / steps


@functools.lru_cache(maxsize=None)
def specs(bits):
    """the drop-in's mx_specs at a_elem_format = w_elem_format = int8 / int4 (installs the drop-in)"""
    M.install_dropin()
    from mx.specs import apply_mx_specs
    return apply_mx_specs({"a_elem_format": f"int{bits}", "w_elem_format": f"int{bits}", "block_size": 32, "scale_bits": 8,
                           "bfloat": 32, "shared_exp_method": "max", "round": "nearest"})


def chain(q, k, v, scale, k_top, mode="ex_pred", bits=8, bias=None):
    """mx.matmul (true QK^T) [+ bias]; k_top = 0, the dense branch: torch softmax; else
    funcs.exponent_approximation (ex_pred / MXINT4 operands) and a torch matmul (pred) [+ bias],
    M.topk on the N x T matrix (torch's CPU order), torch gather / softmax / scatter; then mx.matmul
    (P.V).  Returns (out, idx or None)."""
    s = specs(bits)
    from funcs import exponent_approximation
    from mx import matmul
    true_scores = matmul(q, k.transpose(-2, -1), mx_specs=s, mode_config="aa") * scale
    if bias is not None:
        true_scores = true_scores + bias
    if not k_top:
        return matmul(torch.softmax(true_scores, dim=-1), v, mx_specs=s, mode_config="aa"), None
    ea = exponent_approximation(Q=q, K=k, mx_specs=s)
    aq, ak = {"ex_pred": ea.exponent_based_sign, "MXINT4": ea.MXINT4}[mode]()
    pred_scores = aq @ ak.transpose(-2, -1)
    if bias is not None:
        pred_scores = pred_scores + bias
    _, idx = M.topk(pred_scores, k_top)
    vals = true_scores.gather(dim=-1, index=idx)
    attn = torch.zeros_like(true_scores)
    attn.scatter_(-1, idx, torch.softmax(vals, dim=-1).to(attn.dtype))
    return matmul(attn, v, mx_specs=s, mode_config="aa"), idx


def alternate(groups, steps, warmup, reps):
    """groups: dicts route name -> call.  Every route of every group is warmed up before any
    timing; then, group by group, `reps` repetitions alternate the group's routes, each timed with
    device events around `steps` calls.  Yields each group's {route: [ms per call]} once it is
    timed."""
    groups = list(groups)
    for routes in groups:
        for _ in range(warmup):
            for fn in routes.values():
                fn()
    torch.cuda.synchronize()
    for routes in groups:
        times = {r: [] for r in routes}
        for _ in range(reps):
            for r, fn in routes.items():
                times[r].append(timed(fn, steps))
        yield times


def ms_fields(times):
    """the line's fields of every route: median, spread (max - min over the repetitions), the list"""
    line = {}
    for r, ts in times.items():
        line.update({f"{r}_ms_median": round(statistics.median(ts), 4), f"{r}_ms_spread": round(max(ts) - min(ts), 4),
                     f"{r}_ms": [round(t, 4) for t in ts]})
    return line


def agreement(fused, chained):
    """(out, idx) of the fused call and of the chain: whether idx agrees (None on the dense branch)
    and the normwise relative difference of the outputs"""
    (of, idf), (oc, idc) = fused[:2], chained
    return {"idx_equal": None if idc is None else bool(torch.equal(idf, idc)),
            "out_normwise_rel_diff": (torch.linalg.norm((of - oc).double()) / torch.linalg.norm(oc.double())).item()}
