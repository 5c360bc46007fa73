"""Which kernels of an attention step ran beside which: the last whole steps of a rocprofv3
--kernel-trace csv, one line per kernel with its queue and its start and end in microseconds
from the step's first kernel.

    rocprofv3 --kernel-trace -d DIR -o run --output-format csv -- python bench.py ...
    python tools/trace_overlap.py DIR/.../run_kernel_trace.csv [steps=2]

A step ends with its finishing kernel (a name with "finish" in it).  A kernel that starts before the
previous line's kernel ended is marked with the names it overlapped and for how long."""
import csv
import re
import sys


def short(name):
    m = re.search(r"(\w+_kernel)", name)
    return m.group(1) if m else name[:40]


def main(path, steps=2):
    with open(path, newline="") as fh:
        rows = list(csv.DictReader(fh))
    ks = sorted(({"name": short(r["Kernel_Name"]), "q": r.get("Queue_Id", "?"), "s": int(r["Start_Timestamp"]),
                  "e": int(r["End_Timestamp"])} for r in rows), key=lambda k: k["s"])
    ends = [i for i, k in enumerate(ks) if "finish" in k["name"]]
    if len(ends) < steps + 1:
        raise SystemExit(f"{path}: {len(ends)} finishing kernels, need {steps + 1}")
    for n in range(steps, 0, -1):
        lo, hi = ends[-n - 1] + 1, ends[-n]
        step = ks[lo:hi + 1]
        t0 = step[0]["s"]
        print(f"step -{n}: {(step[-1]['e'] - t0) / 1e3:.1f} us, {len(step)} kernels")
        for i, k in enumerate(step):
            beside = []
            for j, o in enumerate(step):
                ov = min(k["e"], o["e"]) - max(k["s"], o["s"])
                if j != i and ov > 0:
                    beside.append(f"{o['name']} {ov / 1e3:.1f}")
            print(f"  q{k['q']:>3} {k['name']:28s} {(k['s'] - t0) / 1e3:9.1f} .. {(k['e'] - t0) / 1e3:9.1f} us"
                  + ("   beside: " + ", ".join(beside) if beside else ""))


if __name__ == "__main__":
    main(sys.argv[1], int(sys.argv[2]) if len(sys.argv) > 2 else 2)
