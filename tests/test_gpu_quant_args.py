"""The quantizer entry points over all their arguments, on the device, against vectors the
reference itself produced (tests/golden/gen_quant_args_golden.py) and the oracle that
tests/test_quant_args_cpu.py pins to them.

Everything is compared as bit patterns (uint32 / uint16): a NaN on both sides counts as
equal, nothing else is left out -- no element masked, no tolerance, -0.0 is not +0.0.  The
three classes of DESIGN.md §2 (A: NaN at the top codes of the top binade, B: the float16
NaN block at shared exponent 16, C: +0.0 where x / 2^e underflows in a 16-bit dtype) sit in
these vectors; the CPU test names their witnesses.

The two fused witnesses at the end show the shared helpers reaching their other callers:
their NaN pattern is bit-exact, the finite part compared as the existing tests do (the
Linear bit-exact, the attention output within 1e-3 normwise, its indices bit-exact)."""
import numpy as np
import pytest
import torch

import quant_args_cases as QC
from gpu_support import TDT, M, dev, from_bits, host, out_close, to_bits  # noqa: F401
from oracle import mx_oracle as O
from quant_args_cases import same_bits

pytestmark = pytest.mark.gpu
FLT_MAX = np.float32(3.4028234663852886e38)


def same_ints(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    if not np.array_equal(got, want):
        bad = np.argwhere(got != want)
        raise AssertionError(f"{what}: {bad.shape[0]}/{got.size} mismatches, first {bad[:4].tolist()}: "
                             f"{got[tuple(bad[0])]} vs {want[tuple(bad[0])]}")


@pytest.fixture(scope="module")
def F32():
    d = QC.load("quant_args_f32")
    return d, dev(d["f32/x"].view(np.float32))


# ------------------------------------------------------------------ mxa_quantize_bfloat
@pytest.mark.parametrize("b", QC.F32_BFLOATS)
def test_quantize_bfloat_f32(M, F32, b):
    d, x = F32
    for rnd in QC.ROUNDS:
        for den in (1, 0):
            key = f"f32/bf{b}_{rnd}_{den}"
            same_bits(to_bits(M.quantize_bfloat(x, b, rnd, bool(den))), d[key], key, x=d["f32/x"])


@pytest.mark.parametrize("dt", ["f16", "bf16"])
def test_quantize_bfloat_every_16bit_pattern(M, dt):
    d = QC.load("quant_args")
    code = np.arange(65536, dtype=np.uint32).astype(np.uint16)
    x = from_bits(code, dt)
    for b, rnd, den in QC.BF16_CASES:
        key = f"{dt}/bf{b}_{rnd}_{den}"
        y = M.quantize_bfloat(x, b, rnd, bool(den))
        assert y.dtype == TDT[dt]
        same_bits(to_bits(y), d[key], key, dt, x=code)


# ------------------------------------------------------------------ mxa_quantize_mx
@pytest.mark.parametrize("dt", ["f16", "bf16"])
@pytest.mark.parametrize("case", list(QC.MX16_CASES))
def test_quantize_mx_every_16bit_value(M, dt, case):
    """(rows, 32) blocks of every finite value: sorted, shuffled, hand-built."""
    d = QC.load("quant_args_" + dt)
    y = M.quantize_mx(from_bits(d["mx_x"], dt), block_size=32, axis=-1, **QC.MX16_CASES[case])
    assert y.dtype == TDT[dt]
    same_bits(to_bits(y), d["mx_" + case], f"{dt} {case}", dt, x=d["mx_x"])


@pytest.mark.parametrize("dt", ["f16", "bf16"])
def test_quantize_mx_16bit_shapes(M, dt):
    """(3, 70, 45): ragged last blocks with inner > 1, 32-blocks off the last axis, block_size 0."""
    d = QC.load("quant_args")
    z = from_bits(d[f"{dt}/z"], dt)
    for bs, ax in QC.Z_CASES:
        key = f"{dt}/z_bs{bs}_ax{ax}"
        same_bits(to_bits(M.quantize_mx(z, 8, bs, ax)), d[key], key, dt, x=d[f"{dt}/z"])


@pytest.mark.parametrize("b", [16, 10])
def test_quantize_mx_bfloat_argument(M, F32, b):
    d, x = F32
    rows = d["f32/x"].view(np.float32).reshape(-1, 32)
    want = O.quantize_mx(O.quantize_bfloat(rows, b), "int8", 32, -1)[0]
    same_bits(want, d[f"f32/mx_int8_bf{b}"], "oracle vs fixture")
    got = M.quantize_mx(x.reshape(-1, 32), 8, 32, -1, bfloat=b)
    same_bits(to_bits(got), want, f"quantize_mx(bfloat={b})", x=d["f32/x"].reshape(-1, 32))
    got = M.quantize_mx(x.reshape(-1, 32, 1).expand(-1, 32, 3).contiguous(), 8, 32, 1, bfloat=b)  # inner = 3
    for j in range(3):
        same_bits(np.ascontiguousarray(to_bits(got)[..., j]), want, f"quantize_mx(bfloat={b}), axis 1 of 3, inner {j}")


def test_quantize_mx_nan_block_exponent_word(M, F32):
    """want_codes: the exponent word of a NaN block is INT16_MIN, its codes 0."""
    d16 = QC.load("quant_args_f16")
    xb = d16["mx_x"]
    y, codes, exps = M.quantize_mx(from_bits(xb, "f16"), 8, 32, -1, want_codes=True)
    nanblk = QC.nan16(d16["mx_int8_nearest"], "f16").all(axis=1)
    mx = (xb & 0x7FFF).max(axis=1)
    assert nanblk[(mx >= 0x7BFB) & (mx < 0x7C00)].all() and nanblk[mx == 0].all()
    e = host(exps).reshape(-1)
    same_ints(e == np.iinfo(np.int16).min, nanblk, "f16 NaN exponent words")
    assert not host(codes)[nanblk].any()
    d, x = F32
    y, codes, exps = M.quantize_mx(x.reshape(-1, 32), 8, 32, -1, bfloat=16, want_codes=True)
    nanblk = np.isnan(d["f32/mx_int8_bf16"]).all(axis=1)
    assert nanblk.any() and not nanblk.all()
    e = host(exps).reshape(-1)
    same_ints(e == np.iinfo(np.int16).min, nanblk, "f32 NaN exponent words")
    assert not host(codes)[nanblk].any()


# ------------------------------------------------------------------ mxa_shared_exponents
def test_shared_exponents_f32_ebits(M, F32):
    d, x = F32
    for eb in (0, 8, 5, 3):
        same_bits(to_bits(M.shared_exponents(x, "none", ebits=eb)), d[f"f32/sexp_none_e{eb}"], f"none ebits {eb}",
                  x=d["f32/x"])
    for eb in (0, 5):
        got = M.shared_exponents(x.reshape(-1, 32), "max", -1, 32, ebits=eb)
        same_bits(to_bits(got), d[f"f32/sexp_max_e{eb}"], f"max ebits {eb}")


@pytest.mark.parametrize("dt", ["f16", "bf16"])
def test_shared_exponents_16bit_ebits(M, dt):
    d, dm = QC.load("quant_args"), QC.load("quant_args_" + dt)
    code = np.arange(65536, dtype=np.uint32).astype(np.uint16)
    x = from_bits(code, dt)
    for eb in (0, 8, 5, 3):
        got = M.shared_exponents(x, "none", ebits=eb)
        assert got.dtype == TDT[dt]
        same_bits(to_bits(got), d[f"{dt}/sexp_none_e{eb}"], f"{dt} none ebits {eb}", dt, x=code)
    srt = from_bits(dm["mx_x"][: int(dm["mx_rows"][0])], dt)
    for eb in (0, 5):
        got = M.shared_exponents(srt, "max", -1, 32, ebits=eb)
        same_bits(to_bits(got), dm[f"sexp_max_e{eb}"], f"{dt} max ebits {eb}", dt)


# ------------------------------------------------------------------ mxa_approx_values
@pytest.mark.parametrize("dt", ["f16", "bf16"])
@pytest.mark.parametrize("kind,key", [("mxint8", "int8_nearest"), ("mxint4", "int4_nearest")])
def test_approx_values_16bit(M, dt, kind, key):
    d = QC.load("quant_args_" + dt)
    x = from_bits(d["mx_x"], dt)
    same_bits(to_bits(M.approx_values(x, kind)), d["mx_" + key], f"{dt} approx_values {kind}", dt, x=d["mx_x"])
    if kind == "mxint8":
        same_bits(to_bits(M.approx_values(x, kind, bfloat=10)), d["mx_int8_nearest_bf10"],
                  f"{dt} approx_values {kind} bfloat=10", dt, x=d["mx_x"])


@pytest.mark.parametrize("kind", ["sign", "mxint8"])
def test_approx_values_f32_bfloat16(M, F32, kind):
    d, x = F32
    rows = d["f32/x"].view(np.float32).reshape(-1, 32)
    ea = O.ExponentApproximation(rows, rows[:1], bfloat=16)
    want = ea.partial_K()[0] if kind == "sign" else ea.MX_Q
    got = M.approx_values(x.reshape(-1, 32), kind, bfloat=16)  # whole aligned blocks: the float4 kernel
    same_bits(to_bits(got), want, f"approx_values({kind}, bfloat=16)", x=d["f32/x"].reshape(-1, 32))
    pad = np.zeros((rows.shape[0], 40), np.float32)  # d = 40: a ragged block, the one-lane-per-element kernel
    pad[:, :32] = rows
    got = M.approx_values(dev(pad), kind, bfloat=16)
    same_bits(np.ascontiguousarray(to_bits(got)[:, :32]), want, f"approx_values({kind}, bfloat=16), d = 40")


def special_values(x):
    """The special blocks of test_gpu_parity's test_approximator_operands_special_blocks_vs_oracle
    into the six (i, j) slices of a standard normal x of shape (2, 3, rows, D): a NaN, a +Inf and a
    -Inf element, every fifth column of a slice zero, an all-zero row, slices scaled by 2^-120 and
    2^90, and one by 2^-130: subnormal blocks, where the flush decides something."""
    x[0, 0, 3, 5], x[0, 1, 4, 40], x[1, 2, 6, x.shape[-1] - 2] = np.nan, np.inf, -np.inf
    x[1, 0, :, ::5] = 0.0
    x[0, 2, 9, :] = 0.0
    x[1, 1] *= np.float32(2.0 ** -120)
    x[1, 2] *= np.float32(2.0 ** 90)
    x[0, 2] *= np.float32(2.0 ** -130)
    return x


APPROX_MODES = {"sign": "ex_pred", "exion": "two_step_leading_ones", "true_ex": "true_ex"}


@pytest.mark.parametrize("D", [64, 72])
def test_approx_values_kinds_on_both_kernels(M, D):
    """Every operand kind, with and without the subnormal flush, on NaN / Inf / zero / tiny / huge /
    subnormal blocks: the float4 kernel (D = 64, aligned) and the one-lane-per-element kernel
    (D = 72; D = 64 at a data pointer 4 bytes off 16-byte alignment) against the oracle, and
    against each other, bit for bit."""
    x = special_values(np.random.default_rng(17).standard_normal((2, 3, 40, D), dtype=np.float32))
    xd = dev(x)
    assert xd.data_ptr() % 16 == 0
    rows = x.size // D
    buf = torch.empty(rows * D + 1, dtype=torch.float32, device="cuda")
    off = buf[1:].view(rows, D)  # contiguous, 4 bytes off: the general kernel whatever D
    off.copy_(xd.view(rows, D))
    assert off.is_contiguous() and off.data_ptr() % 16 == 4
    for kind in M.ops.OP_KINDS:
        for flush in (False, True):
            what = f"approx_values({kind}, flush={flush}), D = {D}"
            if kind in APPROX_MODES:
                want = O.approx_operands(x, x, APPROX_MODES[kind], flush=flush)[0]
            else:
                want = O.quantize_mx(x, "int8" if kind == "mxint8" else "int4", 32, -1, flush=flush)[0]
            got = to_bits(M.approx_values(xd, kind, flush=flush))
            same_bits(got, want, what, x=x)
            if D == 64:
                gen = to_bits(M.approx_values(off, kind, flush=flush)).reshape(x.shape)
                same_bits(gen, want, what + ", general kernel", x=x)
                same_bits(gen, got, what + ", general against float4 kernel", x=x)


@pytest.mark.parametrize("rnd", QC.ROUNDS)
@pytest.mark.parametrize("mbits", [8, 4, 2])
def test_quantize_mx_row32_matches_generic(M, mbits, rnd):
    """quantize_mx along a contiguous last axis in 32-blocks (one lane per element) and the same
    blocks along axis 0 of the transpose (inner = 96: one thread per block): values, codes and
    block exponents transposes of each other, bit for bit; MXINT8 nearest also against the oracle."""
    x = special_values(np.random.default_rng(17).standard_normal((2, 3, 16, 64), dtype=np.float32)).reshape(96, 64)
    xd = dev(x)
    xt = xd.T.contiguous()
    for flush in (False, True):
        for sb in (8, 5):
            what = f"quantize_mx(int{mbits}, {rnd}, flush={flush}, scale_bits={sb})"
            y, c, e = M.quantize_mx(xd, mbits, 32, -1, sb, rnd, flush, want_codes=True)
            yt, ct, et = M.quantize_mx(xt, mbits, 32, 0, sb, rnd, flush, want_codes=True)
            assert e.shape == (96, 2, 1) and et.shape == (1, 2, 96)
            same_bits(host(yt).T, host(y), what + " values", x=x)
            same_ints(host(ct).T, host(c), what + " codes")
            same_ints(host(et)[0].T, host(e)[:, :, 0], what + " exponents")
            if mbits == 8 and rnd == "nearest":
                want = O.quantize_mx(x, "int8", 32, -1, sb, flush=flush)[0]
                same_bits(host(y), want, what + " against the oracle", x=x)


# ------------------------------------------------------------------ the shared callers
def test_mx_linear_bfloat16_top_code(M):
    """mx_linear(bfloat=16) with one FLT_MAX in x: bf16(FLT_MAX) is NaN (class A), so its
    block, and with it the output row, are NaN; the other rows bit-exact."""
    rng = np.random.default_rng(41)
    x = rng.standard_normal((5, 64), dtype=np.float32)
    W = rng.standard_normal((40, 64), dtype=np.float32) * np.float32(0.125)
    x[2, 7] = FLT_MAX
    want = O.mx_linear(x, W, bfloat=16)
    assert np.isnan(want[2]).all() and np.isfinite(np.delete(want, 2, 0)).all()
    same_bits(host(M.mx_linear(dev(x), dev(W), bfloat=16)), want, "mx_linear(bfloat=16)")


def test_mx_topk_attention_bfloat16_top_code(M):
    rng = np.random.default_rng(42)
    q, k, v = (rng.standard_normal((1, 1, 40, 32), dtype=np.float32) for _ in range(3))
    q[0, 0, 11, 5] = FLT_MAX
    sc = 32 ** -0.5
    r = O.attention(q, k, v, sc, k_top=5, bfloat=16)
    assert np.isnan(r["out"][0, 0, 11]).all() and np.isfinite(np.delete(r["out"], 11, 2)).all()
    out, idx, true_s, pred_s = M.mx_topk_attention(dev(q), dev(k), dev(v), sc, k_top=5, bfloat=16, return_scores=True)
    same_bits(host(true_s), r["true"], "true scores")
    same_bits(host(pred_s), r["pred"], "approximate scores")
    same_ints(host(idx), r["idx"], "idx")
    out_close(host(out), r["out"], 1e-3, "attention out")
