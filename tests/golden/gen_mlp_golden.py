"""Generate tests/golden/mlp.npz FROM THE REFERENCE ITSELF: the MLP of a block as the patched
models run it -- fc1 = mx.Linear, act = nn.GELU, fc2 = mx.Linear (workloads/DiT/models.py:
257-271 and :286-287, timm's Mlp in workloads/deit/models_v2.py:55) -- on the CPU, with the
workloads' mx specs (gen_golden.py BASE_SPECS).  Not run by any test.

    MXA_REFERENCE=<checkout of the reference> python tests/golden/gen_mlp_golden.py

Per case <tag>/: seeded x, W1, b1, W2, b2 and the reference's pre = fc1(x), act = gelu(pre),
y = fc2(act).
  tanh/  (70, 96 -> 160 -> 40)   nn.GELU(approximate="tanh")
  erf/   (33, 100 -> 136 -> 96)  nn.GELU()
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

BASE_SPECS = {  # workloads/DiT/scripts/sample_ddp.py:51-67 (== deit main.py:716-736)
    'w_elem_format': 'int8', 'a_elem_format': 'int8', 'scale_bits': 8,
    'shared_exp_method': 'max', 'block_size': 32, 'bfloat': 32, 'fp': 0,
    'bfloat_subnorms': True, 'round': 'nearest', 'round_mx_output': 'nearest',
    'round_output': 'nearest', 'round_weight': 'nearest',
    'mx_flush_fp32_subnorms': False, 'custom_cuda': False, 'quantize_backprop': False,
}
CASES = (("tanh", 70, 96, 160, 40, "tanh", 700), ("erf", 33, 100, 136, 96, "none", 710))


def rnd(shape, seed, mult=1.0):
    return (np.random.default_rng(seed).standard_normal(shape, dtype=np.float32) * np.float32(mult)).astype(np.float32)


def main():
    store = {}
    for tag, rows, inf, hid, outf, approx, seed in CASES:
        x = torch.from_numpy(rnd((rows, inf), seed))
        W1 = torch.from_numpy(rnd((hid, inf), seed + 1, 0.15))
        b1 = torch.from_numpy(rnd((hid,), seed + 2, 0.5))
        W2 = torch.from_numpy(rnd((outf, hid), seed + 3, 0.1))
        b2 = torch.from_numpy(rnd((outf,), seed + 4, 0.1))
        fc1 = Linear(inf, hid, bias=True, mx_specs=apply_mx_specs(dict(BASE_SPECS)))
        fc2 = Linear(hid, outf, bias=True, mx_specs=apply_mx_specs(dict(BASE_SPECS)))
        fc1.weight.data, fc1.bias.data = W1.clone(), b1.clone()
        fc2.weight.data, fc2.bias.data = W2.clone(), b2.clone()
        act = torch.nn.GELU(approximate=approx)
        with torch.no_grad():
            pre = fc1(x)
            a = act(pre)
            y = fc2(a)
        for name, t in (("x", x), ("W1", W1), ("b1", b1), ("W2", W2), ("b2", b2), ("pre", pre), ("act", a), ("y", y)):
            store[f"{tag}/{name}"] = t.numpy()
    np.savez_compressed(os.path.join(OUT, "mlp.npz"), **store)
    print("wrote mlp.npz")


if __name__ == "__main__":
    main()
