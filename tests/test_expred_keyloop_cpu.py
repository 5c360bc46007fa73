"""The ex_pred key loop's arithmetic for one and two blocks (mxa_select.hpp sel_scores), restated
in numpy and checked against the oracle's score, fl32(exact sum_b m_b 2^(eq_b + ek_b)).

The kernel forms, over the fast range (every block exponent of the row and of the key in
[kExpFastLo, kExpFastHi] = [-50, 61], so e_b = eq_b + ek_b in [-100, 122]) and for even block
lengths n_b (so every m_b = n_b - 2 popc is even):
    h_b = popc(~sq_b ^ sk_b) + n_b / 2 - 32 = m_b / 2
    t_b = K_b * Q2_b,  K_b = bits (ek_b + 127) << 23 (the key's record), Q2_b = bits (eq_b + 128) << 23
    x0 = (float)h0 * t0,   v = fmaf((float)h1, t1, x0)
An odd D (odd m in the last block) takes expred_score's shifted-int32 form, modelled here too.
The fma's single rounding is done in integers (round to nearest even on the exact sum; a
term more than 40 binades below the other acts as a sticky bit), not with numpy's float casts.
"""
from fractions import Fraction

import numpy as np
import pytest

import exchange_cases  # noqa: F401  (puts tools/ on the path)
from oracle import mx_oracle as O
from topk_model import keys_from_f32

F32, U32, I64 = np.float32, np.uint32, np.int64
LO, HI = -50, 61  # kExpFastLo, kExpFastHi


def split_exp(e):
    """e in [-100, 122] as eq + ek, both in the fast range."""
    eq = np.clip(e // 2, LO, HI)
    ek = e - eq
    assert ((ek >= LO) & (ek <= HI)).all()
    return eq, ek


def round_int_f32_bits(S, lo):
    """Bits of fl32(S * 2^lo) for int64 S (|S| < 2^53), round to nearest even, +0 for S = 0,
    inf on overflow; the results here are never subnormal (asserted)."""
    S = S.astype(I64)
    sign = (S < 0).astype(np.uint64)
    M = np.abs(S)
    mant, ex = np.frexp(M.astype(np.float64))  # exact: M < 2^53
    nb = ex.astype(I64)  # bit length
    sh = nb - 24
    up_sh = np.maximum(sh, 0)
    q = np.where(sh > 0, M >> up_sh, M << np.maximum(-sh, 0))
    rem = np.where(sh > 0, M & ((I64(1) << up_sh) - 1), 0)
    half = np.where(sh > 0, I64(1) << np.maximum(up_sh - 1, 0), 1)
    q = q + ((rem > half) | ((rem == half) & ((q & 1) == 1) & (sh > 0)))
    carry = q == (1 << 24)
    q = np.where(carry, q >> 1, q)
    field = sh + carry + lo + 23 + 127
    assert (field[M != 0] >= 1).all()
    bits = (sign << np.uint64(31)) | (np.clip(field, 0, 255).astype(np.uint64) << np.uint64(23)) | (q - (1 << 23)).astype(np.uint64) & np.uint64(0x7FFFFF)
    bits = np.where(field >= 255, (sign << np.uint64(31)) | np.uint64(0x7F800000), bits)
    return np.where(M == 0, 0, bits).astype(U32)


def exact_sum_bits(a0, e0, a1, e1):
    """Bits of fl32(a0 2^e0 + a1 2^e1), small integers a_b, one rounding of the exact sum."""
    gap = e1 - e0
    lo = np.minimum(e0, e1)
    big0 = gap < 0  # term 0 has the larger exponent
    ab, asm = np.where(big0, a0, a1).astype(I64), np.where(big0, a1, a0).astype(I64)
    g = np.abs(gap)
    far = (g > 40) & (ab != 0)
    # a nonzero term below every bit the rounding looks at: its sign as a sticky unit
    asm = np.where(far, np.sign(asm), asm)
    lo = np.where(far, np.maximum(e0, e1) - 40, lo)
    g = np.where(far, 40, g)
    # (a zero larger term: the sum is the smaller term, at its own exponent)
    g = np.where(ab == 0, 0, g)
    return round_int_f32_bits((ab << g) + asm, lo)


def f32_bits_pow2(field):
    return (field.astype(U32) << U32(23)).view(F32)


def kernel_value_bits(m0, e0, m1, e1):
    """The key loop's value for block counts (m0, m1) and exponent sums (e0, e1)."""
    out = np.zeros(m0.shape, U32)
    even = (m0 % 2 == 0) & (m1 % 2 == 0)
    # the product form
    eq0, ek0 = split_exp(e0)
    eq1, ek1 = split_exp(e1)
    t0 = f32_bits_pow2(ek0 + 127) * f32_bits_pow2(eq0 + 128)
    t1 = f32_bits_pow2(ek1 + 127) * f32_bits_pow2(eq1 + 128)
    assert np.array_equal(t0.astype(np.float64), np.ldexp(1.0, e0 + 1)) and np.array_equal(t1.astype(np.float64), np.ldexp(1.0, e1 + 1))
    h0, h1 = (m0 // 2).astype(F32), (m1 // 2).astype(F32)
    with np.errstate(over="ignore"):
        x0 = h0 * t0
    fin = np.isfinite(x0)
    assert np.array_equal(x0.astype(np.float64)[fin], (h0.astype(np.float64) * t0.astype(np.float64))[fin])  # exact
    prod = exact_sum_bits(m0 // 2, e0 + 1, m1 // 2, e1 + 1)  # fmaf(h1, t1, x0): one rounding
    # an infinite x0 (|h0 t0| = 2^128) stays infinite through the fma unless it meets the
    # opposite infinity, which |h1 t1| <= 2^127 is not
    prod = np.where(fin, prod, x0.view(U32))
    out[even] = prod[even]
    # expred_score (odd D): spans <= 23 bits from >= -100 as one int32 conversion, else fp64
    emin = np.minimum(e0, e1)
    near = np.abs(e1 - e0) <= 23
    s = (m0.astype(I64) << np.where(near, e0 - emin, 0)) + (m1.astype(I64) << np.where(near, e1 - emin, 0))
    near_bits = round_int_f32_bits(s, emin)
    with np.errstate(over="ignore"):
        far_bits = (m0 * np.ldexp(1.0, e0) + m1 * np.ldexp(1.0, e1)).astype(F32).view(U32)
    odd = ~even
    out[odd] = np.where(near, near_bits, far_bits)[odd]
    return out


def oracle_bits(m0, e0, m1, e1):
    """The oracle's ex_pred score of a row and a key whose blocks give (m_b, e_b): its exact
    matmul on operands m_b (as a two-element row) and 2^e_b (as a column)."""
    A = np.stack([m0, m1], -1).astype(F32)[:, None, :]
    B = np.stack([np.ldexp(1.0, e0), np.ldexp(1.0, e1)], -1).astype(F32)[:, :, None]
    with np.errstate(over="ignore"):
        return O.exact_matmul_f32(A, B).reshape(-1).view(U32)


def cases(anchor):
    """Every (m0, m1) in [-32, 32]^2 at every gap in [-222, 222], the smaller exponent at -100
    (anchor 'lo') or the larger at 122 ('hi'): both corners on either block are among them."""
    m = np.arange(-32, 33)
    gap = np.arange(-222, 223)
    M0, M1, G = np.meshgrid(m, m, gap, indexing="ij")
    M0, M1, G = M0.ravel(), M1.ravel(), G.ravel()
    if anchor == "lo":
        e0 = -100 + np.maximum(0, -G)
    else:
        e0 = 122 - np.maximum(0, G)
    e1 = e0 + G
    assert e0.min() >= -100 and e1.min() >= -100 and e0.max() <= 122 and e1.max() <= 122
    return M0, e0, M1, e1


def order_key_fast(u):
    """mxa_order.hpp order_key_fast on the value's bits."""
    u = u.astype(U32)
    return u ^ ((u.view(np.int32) >> 31).view(U32) | U32(0x80000000))


@pytest.fixture(scope="module", params=["lo", "hi"])
def swept(request):
    m0, e0, m1, e1 = cases(request.param)
    return m0, e0, m1, e1, kernel_value_bits(m0, e0, m1, e1), oracle_bits(m0, e0, m1, e1)


def test_value_equals_oracle_bit_for_bit(swept):
    m0, e0, m1, e1, got, want = swept
    bad = np.nonzero(got != want)[0]
    assert bad.size == 0, [(int(m0[i]), int(e0[i]), int(m1[i]), int(e1[i]), hex(got[i]), hex(want[i])) for i in bad[:5]]
    zero = m0 * np.ldexp(1.0, e0) + m1 * np.ldexp(1.0, e1) == 0
    assert zero.any() and (got[zero] == 0).all()  # a zero sum is +0
    assert (got != 0x80000000).all() and ((got & 0x7FFFFFFF) <= 0x7F800000).all()  # never -0, never NaN


def test_integer_rounding_against_fractions():
    """round_int_f32_bits / exact_sum_bits (the sticky unit included) on a sample, against
    Python's rationals rounded by float32's own definition."""
    rng = np.random.default_rng(5)
    a0, a1 = rng.integers(-16, 17, 4000), rng.integers(-16, 17, 4000)
    e0, e1 = rng.integers(-99, 124, 4000), rng.integers(-99, 124, 4000)
    got = exact_sum_bits(a0, e0, a1, e1)
    for i in range(4000):
        x = Fraction(int(a0[i])) * Fraction(2) ** int(e0[i]) + Fraction(int(a1[i])) * Fraction(2) ** int(e1[i])
        if x == 0:
            assert got[i] == 0
            continue
        ax = abs(x)
        e = ax.numerator.bit_length() - ax.denominator.bit_length()
        e -= Fraction(2) ** e > ax  # 2^e <= ax < 2^(e+1)
        scaled = ax / Fraction(2) ** (e - 23)
        q, r = divmod(scaled.numerator, scaled.denominator)
        q += (2 * r > scaled.denominator) or (2 * r == scaled.denominator and q & 1)
        if q == 1 << 24:
            q, e = q >> 1, e + 1
        want = ((x < 0) << 31) | (0x7F800000 if e > 127 else ((e + 127) << 23) | (q - (1 << 23)))
        assert int(got[i]) == want, (a0[i], e0[i], a1[i], e1[i])


def test_packed_element_and_pack_test(swept):
    """The key of a fast value is the general order key; the packed element built from it is
    qelem(order_key_fast(v), j) of the oracle's value, and the low-byte pack test (badf) is
    q_bad_bits of it."""
    _, _, _, _, got, want = swept
    key = order_key_fast(got)
    assert np.array_equal(key.astype(np.uint64), keys_from_f32(want.view(F32)))
    for j in (0, 1, 15, 16, 196, 255):
        el = (key & U32(0xFFFFFF00)) | U32(j)
        ref = (order_key_fast(want) & U32(0xFFFFFF00)) | U32(j)
        assert np.array_equal(el, ref)
        assert np.array_equal(el & U32(0xFF), np.full(el.shape, j, U32))
    nan = (want & 0x7FFFFFFF) > 0x7F800000
    assert np.array_equal(got & U32(0xFF), np.where(nan, 0, want & U32(0xFF)).astype(U32))
    assert ((got & 0xFF) != 0).any() and ((got & 0xFF) == 0).any()


@pytest.mark.parametrize("n", [32, 16, 8, 2, 30])
def test_half_count_from_complemented_signs(n):
    """h = popc(~sq ^ sk) + n / 2 - 32 = (n - 2 popc(sq ^ sk)) / 2 when the words' bits from n up
    are equal (prep leaves them 0)."""
    rng = np.random.default_rng(n)
    mask = (1 << n) - 1
    sq = rng.integers(0, 1 << 32, 5000, dtype=np.uint64) & mask
    sk = rng.integers(0, 1 << 32, 5000, dtype=np.uint64) & mask
    popc = lambda x: np.array([bin(int(v)).count("1") for v in x])
    h = popc((~sq & 0xFFFFFFFF) ^ sk) + n // 2 - 32
    assert np.array_equal(2 * h, n - 2 * popc(sq ^ sk))


def test_record_word_carries_out_of_range_exponents():
    """expred_rec_word / expred_rec_exp (mxa_select.hpp) restated: inside the fast range the bits
    of 2^ek; outside a NaN (or +inf) at or above 0x7F800000 with a zero low byte that gives the
    raw int16 exponent back -- INT16_MIN (a NaN block) included."""
    INT16_MIN = -32768
    ek = np.concatenate([np.arange(-16383, 16384), [INT16_MIN]]).astype(np.int64)
    inside = (ek >= LO) & (ek <= HI)
    s15 = np.where(ek == INT16_MIN, -16384, ek)
    w = np.where(inside, (ek + 127) << 23, 0x7F800000 | ((s15 & 0x7FFF) << 8)).astype(np.int64)
    assert (w[inside] < 0x7F800000).all() and (w[~inside] >= 0x7F800000).all() and (w < 1 << 31).all()
    assert ((w & 0xFF) == 0).all()
    s = ((w >> 8) & 0x7FFF)
    s = np.where(s >= 1 << 14, s - (1 << 15), s)  # bits 8..22, sign-extended
    back = np.where(w < 0x7F800000, (w >> 23) - 127, np.where(s == -16384, INT16_MIN, s))
    assert np.array_equal(back, ek)
    # times any power of two, as the key loop does: still not a finite value, low byte still 0
    f = w[~inside].astype(U32).view(F32)
    for q2 in (F32(2.0) ** -49, F32(1.0), F32(2.0) ** 62, F32(0.0)):
        with np.errstate(invalid="ignore"):
            t = (f * q2).astype(F32)
        assert not np.isfinite(t).any() and ((t.view(U32) & 0xFF) == 0).all()


def test_record_bits_are_powers_of_two():
    e = np.arange(LO, HI + 1)
    assert np.array_equal(f32_bits_pow2(e + 127).astype(np.float64), np.ldexp(1.0, e))
    assert np.array_equal(f32_bits_pow2(e + 128).astype(np.float64), np.ldexp(1.0, e + 1))
