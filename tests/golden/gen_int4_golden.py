"""Generate tests/golden/linear_int4.npz FROM THE REFERENCE ITSELF: its mx.Linear under the
specs its PixArt inference script ships (workloads/PixArt/scripts/mx_inference.py:106-122:
w_elem_format = a_elem_format = "int4"), on the CPU, at bfloat 16 (the script's) and 32.  Not
run by any test.

    MXA_REFERENCE=<checkout of the reference> python tests/golden/gen_int4_golden.py

Outputs and seeds only -- the tests regenerate the inputs (tests/int4_cases.py golden_inputs:
x = standard_normal, W = 0.15 standard_normal, b = 0.5 standard_normal from seed, seed + 1,
seed + 2; the MLP's W2 = 0.1 and b2 = 0.1 standard_normal from seed + 3, seed + 4):
  lin<i>/seed, lin<i>/shape (rows, in, out), lin<i>/y_bf16, lin<i>/y_bf32     three Linears
  mlp/seed, mlp/shape (rows, in, hidden, out), mlp/{pre,act,y}_bf{16,32}      fc1 -> GELU(tanh) -> fc2
"""
import os
import sys

import numpy as np
import torch

REF = os.environ.get("MXA_REFERENCE")
if not REF:
    sys.exit("set MXA_REFERENCE to a checkout of the reference (d9bjo0522/mx_quantization)")
sys.path.insert(0, os.path.join(REF, "microxscaling"))
sys.path.insert(0, REF)

from mx import Linear  # noqa: E402  (reference)
from mx.specs import apply_mx_specs  # noqa: E402

OUT = os.path.dirname(os.path.abspath(__file__))
torch.set_num_threads(8)

SPECS = {  # workloads/PixArt/scripts/mx_inference.py:106-122
    'w_elem_format': 'int4', 'a_elem_format': 'int4', 'scale_bits': 8,
    'shared_exp_method': 'max', 'block_size': 32, 'bfloat': 16, 'fp': 0,
    'bfloat_subnorms': True, 'round': 'nearest', 'round_mx_output': 'nearest',
    'round_output': 'nearest', 'round_weight': 'nearest',
    'mx_flush_fp32_subnorms': False, 'custom_cuda': False, 'quantize_backprop': False,
}
LINEARS = ((70, 96, 160, 4100), (33, 100, 136, 4110), (45, 4608, 40, 4120))
MLP = (70, 96, 160, 40, 4200)


def rnd(shape, seed, mult=1.0):
    return (np.random.default_rng(seed).standard_normal(shape, dtype=np.float32) * np.float32(mult)).astype(np.float32)


def layer(inf, outf, W, b, bfloat):
    lin = Linear(inf, outf, bias=True, mx_specs=apply_mx_specs(dict(SPECS, bfloat=bfloat)))
    lin.weight.data, lin.bias.data = torch.from_numpy(W).clone(), torch.from_numpy(b).clone()
    return lin


def main():
    store = {}
    for i, (rows, inf, outf, seed) in enumerate(LINEARS):
        x, W, b = rnd((rows, inf), seed), rnd((outf, inf), seed + 1, 0.15), rnd((outf,), seed + 2, 0.5)
        store[f"lin{i}/seed"] = np.int64(seed)
        store[f"lin{i}/shape"] = np.array([rows, inf, outf], np.int64)
        for bf in (16, 32):
            with torch.no_grad():
                store[f"lin{i}/y_bf{bf}"] = layer(inf, outf, W, b, bf)(torch.from_numpy(x)).numpy()
    rows, inf, hid, outf, seed = MLP
    x, W1, b1 = rnd((rows, inf), seed), rnd((hid, inf), seed + 1, 0.15), rnd((hid,), seed + 2, 0.5)
    W2, b2 = rnd((outf, hid), seed + 3, 0.1), rnd((outf,), seed + 4, 0.1)
    store["mlp/seed"] = np.int64(seed)
    store["mlp/shape"] = np.array([rows, inf, hid, outf], np.int64)
    for bf in (16, 32):
        with torch.no_grad():
            pre = layer(inf, hid, W1, b1, bf)(torch.from_numpy(x))
            a = torch.nn.GELU(approximate="tanh")(pre)
            y = layer(hid, outf, W2, b2, bf)(a)
        for name, t in (("pre", pre), ("act", a), ("y", y)):
            store[f"mlp/{name}_bf{bf}"] = t.numpy()
    np.savez_compressed(os.path.join(OUT, "linear_int4.npz"), **store)
    print("wrote linear_int4.npz")


if __name__ == "__main__":
    main()
