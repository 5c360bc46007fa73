"""The quantizer-argument fixtures (tests/golden/gen_quant_args_golden.py) against the
oracle, on the CPU: every float32 array of the fixture equals the oracle's bit for bit, so
the two vouch for each other, and the fixture holds the witnesses of the three classes of
DESIGN.md §2 that tests/test_gpu_quant_args.py decides on the device:

  A  _quantize_bfloat is NaN where floor(log2|x|), computed in the tensor's dtype, is
     above the dtype's largest exponent (the top codes of the top binade);
  B  a float16 block whose maximum is such a value quantizes to NaN as a whole;
  C  x / 2^e that underflows in a 16-bit dtype gives +0.0 whatever the sign of x.
"""
import numpy as np
import pytest

import quant_args_cases as QC
from oracle import mx_oracle as O
from quant_args_cases import same_bits


@pytest.fixture(scope="module")
def F():
    return QC.load("quant_args_f32")


@pytest.fixture(scope="module")
def X(F):
    return F["f32/x"].view(np.float32)


def test_f32_set_is_what_it_says(F):
    u = F["f32/x"]
    assert u.dtype == np.uint32 and u.size % 32 == 0 and 10000 < u.size < 25000
    have = set(u.tolist())
    for s in (0x0, 0x80000000, 0x7F800000, 0xFF800000, 0x7FC00000, 0x7F7FFFFF, 0xFF7FFFFF, 0x1, 0x80000001):
        assert s in have
    for E in (0, 1, 2, 63, 100, 126, 127, 128, 190, 253, 254):
        for sign in (0, 0x80000000):
            assert all((sign | (E << 23) | m) in have for m in range((1 << 23) - 48, 1 << 23)), E
            for w in range(1, 24):  # the tie of every dropped width, under an even and an odd kept bit
                assert (sign | (E << 23) | (1 << (w - 1))) in have
                if w < 23:
                    assert (sign | (E << 23) | (1 << w) | (1 << (w - 1))) in have


@pytest.mark.parametrize("b", QC.F32_BFLOATS)
def test_oracle_quantize_bfloat(F, X, b):
    for rnd in QC.ROUNDS:
        for den in (1, 0):
            key = f"f32/bf{b}_{rnd}_{den}"
            same_bits(O.quantize_bfloat(X, b, rnd, bool(den)), F[key], key, x=F["f32/x"])


def test_oracle_quantize_mx_behind_bfloat(F, X):
    rows = X.reshape(-1, 32)
    for b in (16, 10):
        got = O.quantize_mx(O.quantize_bfloat(rows, b), "int8", 32, -1)[0]
        same_bits(got, F[f"f32/mx_int8_bf{b}"], f"mx(bfloat {b})")


def test_oracle_shared_exponents(F, X):
    for eb in (0, 8, 5, 3):
        same_bits(O.shared_exponents(X, "none", eb), F[f"f32/sexp_none_e{eb}"], f"none ebits {eb}")
    for eb in (0, 5):
        same_bits(O.shared_exponents(X.reshape(-1, 32), "max", eb), F[f"f32/sexp_max_e{eb}"], f"max ebits {eb}")


def test_class_a_witnesses_f32(F):
    """NaN from 0x7f7fffd4 up to FLT_MAX (both signs), finite one code below, at every
    stored configuration."""
    u = F["f32/x"]
    mag = u & 0x7FFFFFFF
    top = (mag >= QC.TOP_NAN_FIRST["f32"]) & (mag <= QC.TOP_FINITE_LAST["f32"])
    below = mag == QC.TOP_NAN_FIRST["f32"] - 1
    assert top.sum() == 2 * 44 and below.sum() == 2
    for b in QC.F32_BFLOATS:
        for rnd in QC.ROUNDS:
            for den in (1, 0):
                y = F[f"f32/bf{b}_{rnd}_{den}"]
                assert np.isnan(y[top]).all() and not np.isnan(y[below]).any(), (b, rnd, den)
                assert np.isnan(y).sum() == top.sum() + 1  # and the NaN input, nothing else


@pytest.mark.parametrize("dt", ["f16", "bf16"])
def test_class_a_witnesses_16bit(dt):
    D = QC.load("quant_args")
    inf = 0x7C00 if dt == "f16" else 0x7F80
    code = np.arange(65536, dtype=np.uint32)
    mag = code & 0x7FFF
    top = (mag >= QC.TOP_NAN_FIRST[dt]) & (mag < inf)
    for b, rnd, den in QC.BF16_CASES:
        y = D[f"{dt}/bf{b}_{rnd}_{den}"]
        assert y.dtype == np.uint16 and y.shape == (65536,)
        nan = QC.nan16(y, dt)
        assert nan[top].all() and not nan[mag == QC.TOP_NAN_FIRST[dt] - 1].any(), (b, rnd, den)
        assert (nan == (top | (mag > inf))).all()


def test_class_b_witnesses():
    """float16 blocks whose maximum is 0x7bfb .. 0x7bff are NaN throughout; 0x7bfa is not."""
    D = QC.load("quant_args_f16")
    x = D["mx_x"]
    mx = (x & 0x7FFF).max(axis=1)
    topb = (mx >= 0x7BFB) & (mx < 0x7C00)
    n_srt, n_shf, n_hand = D["mx_rows"]
    assert topb[:n_srt].any() and topb[n_srt:n_srt + n_shf].any() and topb[-n_hand:].sum() == 3
    assert (mx[-n_hand:] == 0x7BFA).sum() == 1
    for key in QC.MX16_CASES:
        if "sb" in key or "bf" in key:
            continue  # a 5- or 2-bit scale has its own NaN blocks below 2^16; bfloat 10 rounds 0x7bfa up
        nan = QC.nan16(D["mx_" + key], "f16")
        assert nan[topb].all(), key
        assert not nan[mx == 0x7BFA].any(), key
    # bfloat16: either side of 0x7f58 (128 is above the 8-bit scale's largest exponent)
    B = QC.load("quant_args_bf16")
    mxb = (B["mx_x"] & 0x7FFF).max(axis=1)
    nan = QC.nan16(B["mx_int8_nearest"], "bf16")
    assert (mxb == 0x7F57).any() and (mxb == 0x7F58).any()
    assert not nan[mxb == 0x7F57].any() and nan[mxb == 0x7F58].all()


@pytest.mark.parametrize("dt", ["f16", "bf16"])
def test_class_c_witnesses(dt):
    """In the shuffled blocks some negative input quantizes to +0.0 (its scaled value
    underflowed in the dtype), next to negative inputs that keep -0.0."""
    D = QC.load("quant_args_" + dt)
    n_srt, n_shf, _ = D["mx_rows"]
    x = D["mx_x"][n_srt:n_srt + n_shf]
    for key in ("int8_nearest", "int8_floor", "int8_even", "int4_nearest", "int2_nearest"):
        y = D["mx_" + key][n_srt:n_srt + n_shf]
        neg = (x & 0x8000) != 0
        assert (neg & (y == 0x0000)).any(), key
        assert (neg & (y == 0x8000)).any(), key


def test_fixture_files_stay_small():
    import os
    total = 0
    for name in ("quant_args", "quant_args_f32", "quant_args_f16", "quant_args_bf16"):
        n = os.path.getsize(os.path.join(QC.G, name + ".npz"))
        assert n < (1 << 20), (name, n)
        total += n
    assert total < 3_000_000
