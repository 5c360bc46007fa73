"""Inputs whose attention output is the only float32 result a correct implementation can
produce (tests/test_exact_out_cpu.py proves it per case with the oracle alone,
tests/test_gpu_exact_out.py compares the device's out bit for bit).

Scores that make the softmax exact.  Keys come from classes: class c < nbd has one constant on
the columns of D block c and zeros elsewhere, the last class is the all-zero key.  A query row
carries 8.0 on one D block with a sign of its own.  The key constant is 256 / (the block's
width), 8.0 on a full block and 32.0 on the 8 columns of D = 72's third one, so with SCALE =
1/8 a row's true scores are {+-256, 0} (with the bias also -1000 and -1000 +- 256): every gap
is 0 or at least 256, exp of everything below the maximum is exactly 0 in float32 (e^-103.3 is
the smallest subnormal's half), the m kept keys tied at the maximum get p = 1/m and every other
kept key exactly 0.  A "+" row's maximum is its own class (m = the class size, 2 .. 6: below
every k but 1), a "-" row's maximum is everything else (m = k on the top-k path).

A V that makes P.V independent of the order of operations: integers |n| <= 15 times 2^e per
(32-token block, column), e in 0 .. 3.  V then is its own MXINT8 along the tokens, every
product Pq * Vq is an integer times the row's P granule and the sum of their magnitudes stays
below 2^24 granules, so every summation order gives the same float32."""
import collections
import functools

import numpy as np

from gpu_support import same, same_bits
from oracle import mx_oracle as O

SCALE = 0.125
QC = 8.0  # the query constant; a key class on a block of w columns carries 256 / w
SIZES = (3, 5, 2, 6)  # hot class sizes, rotated per head: T - size >= k at (T, k) = (70, 64)
GATHER16, GATHER32, MFMA, DENSE_MFMA, DENSE_ROWS = 1, 2, 3, 4, 5  # include/mxa.h MXA_FIN_*

# kind: the finishing kernel (MXA_FIN_*); long: the 16-row kernel's LONG variant (T > 512);
# k = 0: the dense branch; bias: 0 / -1000 on the key halves and one fully -inf row; kw: the
# op's further arguments (approx, pred_mode, bfloat)
Case = collections.namedtuple("Case", "kind B H N T D k bias kw")


def _c(kind, B, H, N, T, D, k, bias=False, **kw):
    return Case(kind, B, H, N, T, D, k, bias, tuple(sorted(kw.items())))


def case_id(c):
    name = {GATHER16: "fin16", GATHER32: "fin32", MFMA: "qk", DENSE_MFMA: "dense_qk", DENSE_ROWS: "dense_rows"}[c.kind]
    s = f"{name}{'_long' if c.T > 512 else ''}-B{c.B}N{c.N}T{c.T}D{c.D}" + (f"k{c.k}" if c.k else "")
    return s + ("-bias" if c.bias else "") + "".join(f"-{a}={b}" for a, b in c.kw)


def _cases(bf16):
    out = []
    # finish16_kernel: slot counts 5 / 8 / 12 / 16 (k = 20 / 30 / 48 / 64), k = 1 one V row
    out += [_c(GATHER16, 1, 2, 20, T, D, k) for T in (70, 197) for D in (32, 64, 72, 128) for k in (1, 7, 20, 30, 48, 64)]
    # its LONG variant
    out += [_c(GATHER16, 1, 2, 20, T, D, k) for T in (513, 1000) for D in (32, 72, 128) for k in (20, 30, 48, 64)]
    # finish_kernel
    out += [_c(GATHER32, 2, 2, 40, 300, D, k) for D, k in ((32, 65), (72, 129), (128, 257))]
    # finish_qk_kernel, top-k and dense
    out += [_c(MFMA, 1, 2, N, T, D, k) for N, T, k in ((70, 130, 65), (77, 120, 77), (33, 256, 154)) for D in (64, 72)]
    out += [_c(DENSE_MFMA, 1, 2, N, T, D, 0) for N, T in ((5, 20), (77, 120), (256, 256)) for D in (64, 72)]
    # dense_rows_kernel
    out += [_c(DENSE_ROWS, 2, 2, 40, 300, D, 0) for D in (32, 72)]
    # a bias per kernel (the EXTRA instantiations); k below half the keys: the tie at the maximum
    # of a "-" row spans the unmasked half
    out += [_c(GATHER16, 2, 2, 20, 197, 72, 20, True), _c(GATHER16, 2, 2, 20, 1000, 72, 20, True),
            _c(GATHER32, 2, 2, 40, 300, 72, 129, True), _c(MFMA, 2, 2, 33, 256, 72, 65, True),
            _c(DENSE_MFMA, 2, 2, 77, 120, 72, 0, True), _c(DENSE_ROWS, 2, 2, 40, 300, 72, 0, True)]
    # top-k of the true scores; the MXINT4 approximator
    out += [_c(GATHER16, 1, 2, 20, 197, 64, 20, approx=False), _c(GATHER16, 1, 2, 20, 197, 64, 20, pred_mode="MXINT4")]
    if bf16:  # the oracle's bfloat=16: only while test_exact_out_cpu's conditions hold with it
        out += [_c(GATHER16, 1, 2, 20, 197, 64, 20, bfloat=16), _c(MFMA, 1, 2, 77, 120, 72, 77, bfloat=16)]
    return out


CASES = _cases(bf16=True)
# the long rows' 32-row selection chunks (mxa_sel_long.hip: BH * ceil(N / 32) >= 2048): BH = 1,024
# heads of 33 rows sharing one K / V; the oracle runs once on one head of all 33,792 query rows
CHUNK32 = _c(GATHER16, 64, 16, 33, 513, 32, 20)


def _key_classes(rng, T, nbd, rot):
    """class of every key: hot class c (< nbd) has SIZES[(c + rot) % 4] keys, the rest are the
    zero class (nbd).  Hot keys lie on both sides of `split` (key 512 of a long row, the middle
    otherwise: the bias halves), key 0 and the last key -- in the ragged 32-block -- among them."""
    split = 512 if T > 512 else T // 2
    lo = [0] + [int(x) for x in rng.permutation(np.arange(1, split))]
    hi = [T - 1] + [int(x) for x in rng.permutation(np.arange(split, T - 1))]
    cls = np.full(T, nbd, dtype=np.int64)
    for c in range(nbd):
        for i in range(SIZES[(c + rot) % len(SIZES)]):
            pool = hi if (i % 2 == 0 and hi) or not lo else lo
            cls[pool.pop(0)] = c
    return cls


@functools.lru_cache(maxsize=None)
def inputs(c, heads=None):
    """q, k, v, bias (None without), of a case; heads: (B, H) other than the case's (CHUNK32's
    single oracle head).  Computed once; no test writes to them."""
    B, H = heads or (c.B, c.H)
    N, T, D = (c.N, c.T, c.D) if heads is None else (c.B * c.H * c.N, c.T, c.D)
    rng = np.random.default_rng([c.kind, N, T, D, c.k, int(c.bias)])
    nbd = (D + 31) // 32
    width = [min(32, D - 32 * b) for b in range(nbd)]
    q = np.zeros((B, H, N, D), np.float32)
    k = np.zeros((B, H, T, D), np.float32)
    for b in range(B):
        for h in range(H):
            cls = _key_classes(rng, T, nbd, b * H + h)
            for j in range(nbd):
                k[b, h, cls == j, 32 * j:32 * j + 32] = np.float32(256.0 / width[j])
            blk = (np.arange(N) + rng.integers(0, nbd)) % nbd
            sign = rng.choice(np.array([-1.0, 1.0], np.float32), N)
            for r in range(N):
                q[b, h, r, 32 * blk[r]:32 * blk[r] + 32] = np.float32(QC) * sign[r]
    n = rng.integers(-15, 16, (B, H, T, D)).astype(np.float32)
    e = rng.integers(0, 4, (B, H, (T + 31) // 32, D)).astype(np.float32)
    v = (n * np.exp2(np.repeat(e, 32, axis=2)[:, :, :T])).astype(np.float32)
    bias = None
    if c.bias:
        bias = np.zeros((B, 1, N, T), np.float32)
        bias[:, :, :, T // 2:] = -1000.0
        bias[B - 1, 0, 2, :] = -np.inf  # every key masked: the row's softmax, and its output, are NaN
    return q, k, v, bias


def oracle_kw(c):
    kw = dict(c.kw)
    if c.k:
        kw["k_top"] = c.k
    else:
        kw["top_k"] = False
    return kw


@functools.lru_cache(maxsize=None)
def reference(c, heads=None):
    """the oracle's result on inputs(c, heads), computed once and left unchanged"""
    q, k, v, bias = inputs(c, heads)
    return O.attention(q, k, v, SCALE, bias=bias, **oracle_kw(c))


def tied(c, r):
    """(m, kept): per query row the number of keys that share the softmax's maximum weight, and
    the number of keys the softmax runs over (k, or T on the dense branch); m = 0 for a NaN row"""
    a = r["attn"]
    with np.errstate(invalid="ignore"):
        m = (a == a.max(-1, keepdims=True)).sum(-1)
    return np.where(np.isnan(a).any(-1), 0, m), (c.k or c.T)


# ---- the five conditions under which out is the only float32 result ----------
# Each takes the case, its inputs (q, k, v, bias), the oracle's reference at the width and the width as
# the oracle's elem; test_exact_out_cpu.py, test_attn4_cpu.py and test_long_dense_cpu.py call them.
WIDTH = {"int8": (6, 15 * 8), "int4": (2, 7 * 8)}  # es - (a code unit's exponent); the bound on |v|


def _bf(c):
    return dict(c.kw).get("bfloat", 32)


def _finite_rows(r):
    return ~np.isnan(r["attn"]).any(-1)


def _mx(a, c, elem, axis):
    return O.quantize_mx(O.quantize_bfloat(a, _bf(c)), elem, 32, axis)


def score_gaps_are_zero_or_wide(c, inputs, r, elem):
    """1. within every query row two true scores are equal or at least 150 apart: exp of the
    lower one is exactly 0 in float32, by np.exp and by exp2((v - mx) log2 e), subnormals flushed
    or not (e^-150 < 2^-216)"""
    t = np.sort(r["true"].astype(np.float64), axis=-1)
    fin = np.isfinite(t).all(-1)
    assert fin.sum() >= fin.size - (c.H if c.bias else 0) and fin.any()
    gap = np.diff(t[fin], axis=-1)
    assert ((gap == 0) | (gap >= 150)).all(), gap[(gap != 0) & (gap < 150)][:4]
    assert (gap >= 150).any(-1).all()  # (no row whose scores all tie)
    x = np.float32(-150.0)
    assert np.exp(x) == 0 and np.exp2(np.float32(x * np.float32(1.4426950408889634))) == 0


def operands_are_their_own_mx(c, inputs, r, elem):
    """2. q and k are their own MX along D, v along the tokens, and v holds integers"""
    q, k, v, _ = inputs
    same_bits(_mx(q, c, elem, -1)[0], q, "MX(q)")
    same_bits(_mx(k, c, elem, -1)[0], k, "MX(k)")
    same_bits(_mx(v, c, elem, -2)[0], v, "MX(v)")
    assert (v == np.round(v)).all() and np.abs(v).max() <= WIDTH[elem][1]


def out_is_the_exact_product(c, inputs, r, elem):
    """3. out equals the float64 product of the quantized operands, that product is a float32,
    and the per-element sum of |Pq| |Vq| is below 2^24 granules (a row's granule: the code step
    2^(e - 6), at int4 2^(e - 2), of its lowest non-zero P block, V being integers): every partial
    sum in every order is an integer below 2^24 times the granule, so exact in float32"""
    fin = _finite_rows(r)
    pq, _, pe = _mx(r["attn"], c, elem, -1)
    vq = _mx(inputs[2], c, elem, -2)[0]
    with np.errstate(invalid="ignore"):
        prod = np.matmul(pq.astype(np.float64), vq.astype(np.float64))
        S = np.matmul(np.abs(pq).astype(np.float64), np.abs(vq).astype(np.float64))
    assert (prod[fin] == prod[fin].astype(np.float32)).all()
    same_bits(r["out"][fin], O.quantize_bfloat(prod[fin].astype(np.float32), _bf(c)), "out vs the exact product")
    assert np.isnan(r["out"][~fin]).all()
    blk, _ = O.to_blocks(pq, -1, 32)
    e = np.where((blk != 0).any(-1), pe[..., 0], np.inf)  # the exponents of the non-zero blocks
    gran = np.exp2(e.min(-1) - WIDTH[elem][0])[fin]
    assert np.isfinite(gran).all()
    assert (pq[fin] / gran[:, None] == np.round(pq[fin] / gran[:, None])).all()
    worst = (S[fin] / gran[:, None]).max()
    print(f"{case_id(c)} {elem}: sum |Pq||Vq| reaches 2^{np.log2(max(worst, 1)):.1f} granules")
    assert worst < 2 ** 24


def p_codes_survive_four_ulp(c, inputs, r, elem):
    """4. every non-zero p moved by 4 ulp either way keeps the MX codes of P (at int4: p = 1/m lies
    4 ulp inside a cell of the 4-bit grid, floor(p 2^(2 - e) + 1/2) with the clip at 7 -- m = 65,
    129: y = 7.9 clips from either side).  Rows whose m is a power of two are exempt: p = 1/m is
    exact there in any implementation, and below it lies the next binade."""
    m, _ = tied(c, r)
    rows = (m > 0) & ((m & (m - 1)) != 0)
    assert rows.any() or c.k == 1
    a = r["attn"][rows]
    codes = _mx(a, c, elem, -1)[1]
    for d in (-4, 4):
        b = a.copy().view(np.int32)
        b[a != 0] += d
        same(_mx(b.view(np.float32), c, elem, -1)[1], codes, f"P codes at {d} ulp")


def tie_counts_vary(c, inputs, r, elem):
    """5. rows with m < k (kept slots of zero weight, P blocks whose codes are all zero) and
    rows with m >= k; on the dense branch m takes several values; k = 1 has m = 1"""
    m_all, kept = tied(c, r)
    m = m_all[m_all > 0]
    if c.k == 1:
        assert (m == 1).all()
    elif c.k:
        assert (m < kept).any() and (m >= kept).any(), np.unique(m)
        fin = _finite_rows(r)
        assert (np.take_along_axis(r["attn"], r["idx"], -1)[fin] == 0).any()  # a kept slot of zero weight
        if c.T >= 197:  # (a row of three key blocks can have a hot key in each)
            pq = O.quantize_mx(r["attn"], elem, 32, -1)[0]
            idx_blocks = np.take_along_axis(O.to_blocks(pq, -1, 32)[0].any(-1), r["idx"] >> 5, -1)
            assert (~idx_blocks)[fin].any()  # a kept key in a P block whose codes are all zero
    else:
        assert len(np.unique(m)) >= 3, np.unique(m)
    if c.T > 512 and not c.bias:  # the rows won by a hot class: weights on both sides of key 512
        hot = (r["attn"] > 0) & ((m_all > 0) & (m_all < kept))[..., None]
        assert hot[..., :512].any() and hot[..., 512:].any()


CONDITIONS = (score_gaps_are_zero_or_wide, operands_are_their_own_mx, out_is_the_exact_product, p_codes_survive_four_ulp,
              tie_counts_vary)
