"""What tests/test_quant_args_cpu.py and tests/test_gpu_quant_args.py share: the fixtures of
tests/golden/gen_quant_args_golden.py (the reference's _quantize_bfloat, _quantize_mx and
_shared_exponents over all their arguments), the bit comparison, and the codes that the
three top-binade / zero-sign classes of DESIGN.md §2 are witnessed at."""
import functools
import os

import numpy as np

import gpu_support
from gpu_support import G

# every comparison here is one of bit patterns: the fixtures hold uint32 / uint16 arrays
same_bits = functools.partial(gpu_support.same_bits, patterns=True)
ROUNDS = ("nearest", "floor", "even")
F32_BFLOATS = (10, 13, 16, 19, 24, 31)
# (bfloat, round, allow_denorm) stored for every 16-bit pattern
BF16_CASES = ([(b, "nearest", 1) for b in (10, 11, 16, 24)] +
              [(b, r, 1) for b in (10, 16) for r in ("floor", "even")] + [(b, "nearest", 0) for b in (10, 16)])
# key suffix -> M.quantize_mx arguments, for the (rows, 32) 16-bit matrices
MX16_CASES = {f"{e}_{r}": dict(elem_mbits=int(e[3:]), round=r) for e in ("int8", "int4", "int2") for r in ROUNDS}
MX16_CASES["int8_nearest_flush"] = dict(elem_mbits=8, flush=True)
MX16_CASES["int8_nearest_sb5"] = dict(elem_mbits=8, scale_bits=5)
MX16_CASES["int8_nearest_sb2"] = dict(elem_mbits=8, scale_bits=2)
MX16_CASES["int8_nearest_bf10"] = dict(elem_mbits=8, bfloat=10)
Z_CASES = [(bs, ax) for bs in (9, 32, 0) for ax in (-1, -2, 0)]

# class A: floor(log2|x|) computed in the dtype is one above the dtype's largest exponent
# from this code of the top binade on (both signs): _quantize_bfloat returns NaN
TOP_NAN_FIRST = {"f32": 0x7F7FFFD4, "bf16": 0x7F58, "f16": 0x7BFB}
TOP_FINITE_LAST = {"f32": 0x7F7FFFFF, "bf16": 0x7F7F, "f16": 0x7BFF}

_CACHE = {}


def load(name):
    """One fixture file (read once per process, never modified)."""
    if name not in _CACHE:
        _CACHE[name] = dict(np.load(os.path.join(G, name + ".npz")))
    return _CACHE[name]


def nan16(u, dt):
    inf = 0x7C00 if dt == "f16" else 0x7F80
    return (u & 0x7FFF) > inf
