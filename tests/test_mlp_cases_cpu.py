"""CPU proof, with the oracle alone, that every input of tests/mlp_cases.py sits in the regime
its GPU test (tests/test_gpu_mlp.py) is about: the digit kernel's gate and spreads at fc1 and
at fc2, the GELU's all-zero hidden block, the quantizer's es < -121 block, the hidden block
whose pre is normal and whose act is subnormal, the flush-sensitivity of y, the dictated pre
of the GELU cases and torch's CPU kernel on the regions where the formula pins the result.
The GPU tests repeat these assertions before their first device call."""
import numpy as np
import pytest

import gate_cases as GC
import mlp_cases as MC
from oracle import mx_oracle as O


def _same(a, b):
    return bool(((a == b) | (np.isnan(a) & np.isnan(b))).all())


@pytest.mark.parametrize("inf", MC.K_EDGE_INF)
def test_k_edge_regime(inf):
    x, W1, b1, W2, b2 = MC.k_edge(inf)
    fig = MC.assert_k_edge(inf, x, W1)
    print(inf, fig)
    pre = O.mx_linear(x, W1, b1)
    # the GELU is exercised, not saturated: pre of order 1
    assert 0.3 < pre.std() < 3 and np.isfinite(pre).all()
    al = lambda n: (n + 255) // 256 * 256  # noqa: E731
    r, h = MC.K_EDGE_ROWS, MC.K_EDGE_HID
    assert MC.workspace_bytes(r, inf, h, False) - MC.workspace_bytes(r, inf, h, True) == al(r * h * 4)


def test_workload_width_blocks():
    """what the two workload-width chains run: fc1's K-blocks within the fused kernel's 72,
    fc2's beyond the digit kernel's 72 (so on the tile kernel), a full and a one-row row block"""
    for inf, hid in ((768, 3072), (1152, 4608)):
        assert inf // 32 in (24, 36) and inf // 32 <= MC.MLP_NBK_MAX
        assert hid // 32 in (96, 144) and hid // 32 > MC.MLP_NBK_MAX and (hid // 32) // 4 in (24, 36)


@pytest.mark.parametrize("flush", [False, True])
@pytest.mark.parametrize("act", MC.ACTS)
@pytest.mark.parametrize("name", MC.EXTREMES)
def test_extremes_regime(name, act, flush):
    c = MC.extremes(name)
    fig, pre, a = MC.assert_extremes(name, *c, act, flush)
    print(name, act, flush, fig)
    # the oracle's float64 sums against the exact integer sums, on this activation: which of
    # the two a device result has to match where they differ
    _, _, _, W2, b2 = c
    yo, ye = O.mx_linear(a, W2, b2, flush=flush), MC.exact_mx_linear(a, W2, b2, flush=flush)
    ties = int((yo != ye).sum())
    print("oracle != exact fc2 elements:", ties)
    assert ties == 0 and _same(yo, ye)
    x, W1, b1 = c[:3]
    assert _same(pre, MC.exact_mx_linear(x, W1, b1, flush=flush))


def test_exact_linear_is_the_oracle_on_ordinary_data():
    x, W1, b1, W2, b2 = MC.case(37, 100, 72, 9, 3)
    assert _same(MC.exact_mx_linear(x, W1, b1), O.mx_linear(x, W1, b1))
    assert _same(MC.exact_mx_linear(x * np.float32(2.0 ** -120), W1 * np.float32(2.0 ** -20)),
                 O.mx_linear(x * np.float32(2.0 ** -120), W1 * np.float32(2.0 ** -20)))  # subnormal results


@pytest.mark.parametrize("kind", ["fast", "slow"])
def test_gelu_pinned_pre(kind):
    x, W1, b1, t = MC.gelu_pinned(kind)
    fig = MC.assert_gelu_pinned(kind, x, W1, b1, t)
    print(kind, fig, t.size)
    at = np.abs(t.astype(np.float64))
    if kind == "fast":
        assert at.max() == 2.0 ** 100 and at[at >= 10].min() < 13 and at.min() == 64 * 2.0 ** -120
        assert (t >= 10).any() and (t <= -10).any() and (at <= 2.0 ** -30).any() and t.size % 32 == 0 and t.size % 16 == 0
    else:
        sub = (at < 2.0 ** -126) & (at > 0)
        assert sub.sum() >= 20 and at[sub].min() == 2.0 ** -149 and (at == 2.0 ** -126).any()
        z = t[t == 0]
        assert np.signbit(z).any() and (~np.signbit(z)).any()  # both zeros are reached as pre
        assert t.size % 16 == 0


@pytest.mark.parametrize("act", MC.ACTS)
def test_torch_gelu_closed_form(act):
    """torch's CPU kernel equals the closed form bit for bit on the pinned regions: the
    dictated targets, a sweep of 10 .. 1000 in both signs, powers of two up to 2^100."""
    pre = [MC.gelu_pinned(k)[3] for k in ("fast", "slow")]
    sweep = np.linspace(10.0, 1000.0, 19801).astype(np.float32)
    p2 = np.exp2(np.arange(4, 101)).astype(np.float32)
    tiny = np.exp2(np.arange(-149, -29)).astype(np.float32)
    pre = np.concatenate(pre + [sweep, -sweep, p2, -p2, tiny, -tiny, np.float32(3) * tiny[:100]])
    want = MC.gelu_closed_form(pre)
    assert not np.isnan(want).any()
    MC.same_bits(MC.gelu_cpu(pre, act), want, act)


def test_same_bits_tells_the_zeros_apart():
    z = np.zeros(3, np.float32)
    MC.same_bits(z, z)
    MC.same_bits(np.array([np.nan], np.float32), np.array([-np.nan], np.float32))
    with pytest.raises(AssertionError):
        MC.same_bits(z, -z)
    assert (z == -z).all()


# ---- what a wrong epilogue quantizer would do to y, modelled on the oracle ----------------------
def _fc2_of_values(qa, W2, b2, flush):
    """fc2 of already quantized hidden values (the oracle's mx_linear behind its input rule)"""
    qw = O.quantize_mx(W2, "int8", 32, -1, flush=flush)[0]
    return (O.exact_matmul_f32(qa, qw.T) + b2).astype(np.float32)


@pytest.mark.parametrize("act", MC.ACTS)
def test_modelled_quantizer_faults_change_y(act):
    """Three faults of the epilogue quantizer restated on the oracle's hidden values of the
    "tiny" case; each moves y away from what test_mlp_hidden_extremes compares the device with,
    so that test can fail on them:
      * flush_subnormals not passed on (the epilogue quantizes as if it were 0);
      * a block of es < -121 through q8_code without its factor 64 (codes of x 2^-es, not 64 x 2^-es);
      * the -0.0 the GELU gives for pre <= -10 coming out as +0.0 (same_bits, not ==)."""
    x, W1, b1, W2, b2 = MC.extremes("tiny")
    a = MC.gelu_cpu(O.mx_linear(x, W1, b1, flush=True), act)
    want = O.mx_linear(a, W2, b2, flush=True)
    assert _same(want, _fc2_of_values(O.quantize_mx(a, "int8", 32, -1, flush=True)[0], W2, b2, True))  # the model
    got = _fc2_of_values(O.quantize_mx(a, "int8", 32, -1, flush=False)[0], W2, b2, True)
    assert (got != want).mean() > 0.9

    a = MC.gelu_cpu(O.mx_linear(x, W1, b1), act)
    want = O.mx_linear(a, W2, b2)
    qa, _, es = O.quantize_mx(a, "int8", 32, -1)
    assert (es[:, 5, 0] < -121).all()
    blk = a[:, 160:192].astype(np.float64) * np.exp2(-es[:, 5].astype(np.float64))  # x 2^-es, without the 64
    codes = np.copysign(np.minimum(np.floor(np.abs(blk) + 0.5), 127.0), blk)
    qa[:, 160:192] = (codes * np.exp2(es[:, 5].astype(np.float64) - 6)).astype(np.float32)
    assert (_fc2_of_values(qa, W2, b2, False) != want).mean() > 0.9

    xs, W1s, b1s, _, _ = MC.extremes("zero_block")
    z = MC.gelu_cpu(O.mx_linear(xs, W1s, b1s), act)[:, 32:64]
    assert (z == 0).all() and np.signbit(z).all()
    with pytest.raises(AssertionError):
        MC.same_bits(np.abs(z), z)
