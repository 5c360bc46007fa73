"""Generate tests/golden/quant_args*.npz FROM THE REFERENCE ITSELF: the quantizer entry
points (_quantize_bfloat, _quantize_mx, _shared_exponents) over all their arguments.

Run only where the reference checkout exists (MXA_REFERENCE, as for gen_golden.py):

    python tests/golden/gen_quant_args_golden.py

It imports the reference's `mx` package, runs on the CPU and stores only inputs and
outputs.  No test imports it.  The vectors are split over four files so that each stays
below 1 MiB (tests/quant_args_cases.py names the cases in them):

    quant_args.npz        _quantize_bfloat and _shared_exponents on every 16-bit pattern;
                          the (3, 70, 45) shape cases
    quant_args_f32.npz    _quantize_bfloat on the structured float32 set; the set through
                          _quantize_mx behind _quantize_bfloat and through _shared_exponents
    quant_args_f16.npz    _quantize_mx on every finite float16 value (sorted / shuffled / hand blocks)
    quant_args_bf16.npz   the same for bfloat16

16-bit arrays are stored as uint16 bit patterns of the dtype, float32 arrays as float32.
"""
import os
import sys

sys.dont_write_bytecode = True  # never write __pycache__ into the reference tree

import numpy as np
import torch

REF = os.environ.get("MXA_REFERENCE", "/root/reference")
sys.path.insert(0, os.path.join(REF, "microxscaling"))

from mx.elemwise_ops import _quantize_bfloat  # noqa: E402  (reference)
from mx.mx_ops import _quantize_mx, _shared_exponents  # noqa: E402  (reference)

OUT = os.path.dirname(os.path.abspath(__file__))
torch.set_num_threads(8)

DTYPES = (("f16", torch.float16, 0x7C00), ("bf16", torch.bfloat16, 0x7F80))
ROUNDS = ("nearest", "floor", "even")
F32_EXP_FIELDS = (0, 1, 2, 63, 100, 126, 127, 128, 190, 253, 254)
F32_BFLOATS = (10, 13, 16, 19, 24, 31)


def _bits(t):
    """float16 / bfloat16 tensor -> its uint16 bit patterns (numpy holds no bfloat16)."""
    return t.contiguous().view(torch.int16).numpy().view(np.uint16)


def _from_bits(u16, dt):
    return torch.from_numpy(np.ascontiguousarray(u16, dtype=np.uint16).view(np.int16)).view(dt)


def f32_structured():
    """The float32 inputs as uint32 bit patterns, padded with zeros to whole 32-wide rows.

    Per exponent field and sign, for each dropped width w = 1..23 (bfloat 31..9 keeps
    23 - w mantissa bits): the low w bits at the tie, tie -+ 1 ulp, all ones and zero,
    under kept bits 0, 1 (even / odd), six middle pairs and the top pair; then the top 48
    codes of the binade (where float32 log2 reaches the next integer); then the specials."""
    pats = []
    for E in F32_EXP_FIELDS:
        for w in range(1, 24):
            tie = 1 << (w - 1)
            lows = sorted({tie, (tie - 1) & ((1 << w) - 1), (tie + 1) & ((1 << w) - 1), (1 << w) - 1, 0})
            kb = 23 - w
            top = (1 << kb) - 1
            mids = [m >> w for m in (0x2AAAAA, 0x555555, 0x333333, 0x6DB6DB, 0x1C71C7, 0x400000)]
            kept = sorted({0, 1 & top, top, top & ~1} | {m & top for m in mids} | {(m ^ 1) & top for m in mids})
            for k in kept:
                for lo in lows:
                    pats.append((E << 23) | (k << w) | lo)
        pats.extend((E << 23) | m for m in range((1 << 23) - 48, 1 << 23))
    pats = np.array(pats, dtype=np.uint32)
    both = np.concatenate([pats, pats | np.uint32(0x80000000)])
    special = np.array([0x00000000, 0x80000000, 0x7F800000, 0xFF800000, 0x7FC00000, 0x7F7FFFFF, 0xFF7FFFFF,
                        0x00000001, 0x80000001], dtype=np.uint32)
    u = np.concatenate([special, both])
    u = u[np.sort(np.unique(u, return_index=True)[1])]  # each pattern once, in the order built
    pad = (-u.size) % 32
    return np.concatenate([u, np.zeros(pad, np.uint32)])


def gen_main():
    out = {}
    # ---- _quantize_bfloat, float32 structured set ------------------------------------
    u = f32_structured()
    out["f32/x"] = u
    x = torch.from_numpy(u.view(np.float32).copy())
    for b in F32_BFLOATS:
        for rnd in ROUNDS:
            for den in (True, False):
                out[f"f32/bf{b}_{rnd}_{int(den)}"] = _quantize_bfloat(x.clone(), b, round=rnd, allow_denorm=den).numpy()
    # the set behind _quantize_bfloat through _quantize_mx (32-wide rows), and its exponents
    rows = x.reshape(-1, 32)
    for b in (16, 10):
        xb = _quantize_bfloat(rows.clone(), b, round="nearest")
        out[f"f32/mx_int8_bf{b}"] = _quantize_mx(xb, 8, elem_format="int8", block_size=32, axes=[-1],
                                                 round="nearest").numpy()
    for eb in (0, 8, 5, 3):
        out[f"f32/sexp_none_e{eb}"] = _shared_exponents(x.clone(), method="none", ebits=eb).numpy()
    for eb in (0, 5):
        out[f"f32/sexp_max_e{eb}"] = _shared_exponents(rows.clone(), method="max", axes=[-1], ebits=eb).numpy()
    np.savez_compressed(os.path.join(OUT, "quant_args_f32.npz"), **out)
    print("wrote quant_args_f32", u.size)
    # ---- 16-bit dtypes ---------------------------------------------------------------
    out = {}
    allbits = np.arange(65536, dtype=np.uint32).astype(np.uint16)
    for name, dt, _ in DTYPES:
        xa = _from_bits(allbits, dt)
        for b in (10, 11, 16, 24):
            out[f"{name}/bf{b}_nearest_1"] = _bits(_quantize_bfloat(xa.clone(), b, round="nearest", allow_denorm=True))
        for b in (10, 16):
            for rnd in ("floor", "even"):
                out[f"{name}/bf{b}_{rnd}_1"] = _bits(_quantize_bfloat(xa.clone(), b, round=rnd, allow_denorm=True))
            out[f"{name}/bf{b}_nearest_0"] = _bits(_quantize_bfloat(xa.clone(), b, round="nearest", allow_denorm=False))
        for eb in (0, 8, 5, 3):
            out[f"{name}/sexp_none_e{eb}"] = _bits(_shared_exponents(xa.clone(), method="none", ebits=eb))
        # ragged last blocks with inner > 1, and the whole-axis block
        rng = np.random.default_rng(9)
        z = torch.from_numpy(rng.standard_normal((3, 70, 45), dtype=np.float32) *
                             np.exp2(rng.integers(-6, 7, (3, 70, 45))).astype(np.float32)).to(dt)
        out[f"{name}/z"] = _bits(z)
        for bs in (9, 32, 0):
            for ax in (-1, -2, 0):
                out[f"{name}/z_bs{bs}_ax{ax}"] = _bits(_quantize_mx(z.clone(), 8, elem_format="int8", block_size=bs,
                                                                    axes=[ax], round="nearest"))
    np.savez_compressed(os.path.join(OUT, "quant_args.npz"), **out)
    print("wrote quant_args")


def mx_rows(name, lim):
    """(rows, 32) uint16 inputs: every finite value sorted by magnitude, the same values in
    a seeded shuffle, then the hand-built blocks; and the three row counts."""
    mag = np.repeat(np.arange(lim, dtype=np.uint32), 2)
    mag[1::2] |= 0x8000  # +v, -v, next magnitude ...
    srt = mag.astype(np.uint16).reshape(-1, 32)
    shf = np.random.default_rng(11).permutation(mag.astype(np.uint16)).reshape(-1, 32)
    rng = np.random.default_rng(12)
    if name == "f16":
        # 0x7bfa: floor(log2) = 15 (finite); 0x7bfb, 0x7bff: 16, and 2^16 is inf in float16
        tops = (0x7BFA, 0x7BFB, 0x7BFF, 0xFBFB)
        fill = np.array([0x7BF0, 0x3C00, 0xBC00, 0x0001, 0x8001, 0x03FF, 0x83FF, 0x0400, 0x8400, 0x5640, 0xD640,
                         0x6FFF, 0xEFFF, 0x7000, 0xF000, 0x0000, 0x8000], dtype=np.uint16)
        inf, nan, one = 0x7C00, 0x7E00, 0x3C00
    else:
        # 0x7f57: floor(log2) = 127; 0x7f58: 128 (above the scale's 127)
        tops = (0x7F57, 0x7F58, 0x7F7F, 0xFF58)
        fill = np.array([0x7F00, 0x3F80, 0xBF80, 0x0001, 0x8001, 0x007F, 0x807F, 0x0080, 0x8080, 0x7B40, 0xFB40,
                         0x7BFF, 0xFBFF, 0x7C00, 0xFC00, 0x0000, 0x8000], dtype=np.uint16)
        inf, nan, one = 0x7F80, 0x7FC0, 0x3F80
    hand = []
    for t in tops:
        blk = np.concatenate([fill, rng.integers(0, lim // 2, 15).astype(np.uint16) | (rng.integers(0, 2, 15) << 15).astype(np.uint16)])
        blk[rng.integers(17, 32)] = t
        hand.append(blk)
    hand.append(np.zeros(32, np.uint16))
    hand.append(np.full(32, 0x8000, np.uint16))
    for s in (inf, inf | 0x8000, nan):
        blk = np.full(32, one, np.uint16)
        blk[1::2] |= 0x8000
        blk[3] = s
        hand.append(blk)
    hand = np.stack(hand).astype(np.uint16)
    return np.concatenate([srt, shf, hand]), np.array([srt.shape[0], shf.shape[0], hand.shape[0]], np.int64)


def gen_mx16():
    for name, dt, lim in DTYPES:
        out = {}
        xb, counts = mx_rows(name, lim)
        out["mx_x"], out["mx_rows"] = xb, counts
        x = _from_bits(xb, dt)

        def q(elem, rnd="nearest", sb=8, flush=False):
            return _bits(_quantize_mx(x.clone(), sb, elem_format=elem, block_size=32, axes=[-1], round=rnd,
                                      flush_fp32_subnorms=flush))
        for elem in ("int8", "int4", "int2"):
            for rnd in ROUNDS:
                out[f"mx_{elem}_{rnd}"] = q(elem, rnd)
        out["mx_int8_nearest_flush"] = q("int8", flush=True)
        for sb in (5, 2):
            out[f"mx_int8_nearest_sb{sb}"] = q("int8", sb=sb)
        # bfloat 10 (3 mantissa bits) in front, as quantize_mx's bfloat argument has it
        xq = _quantize_bfloat(x.clone(), 10, round="nearest")
        out["mx_int8_nearest_bf10"] = _bits(_quantize_mx(xq, 8, elem_format="int8", block_size=32, axes=[-1],
                                                         round="nearest"))
        srt = x[: int(counts[0])]
        for eb in (0, 5):
            out[f"sexp_max_e{eb}"] = _bits(_shared_exponents(srt.clone(), method="max", axes=[-1], ebits=eb))
        np.savez_compressed(os.path.join(OUT, f"quant_args_{name}.npz"), **out)
        print("wrote quant_args_" + name, xb.shape)


if __name__ == "__main__":
    for w in sys.argv[1:] or ["main", "mx16"]:
        globals()["gen_" + w]()
