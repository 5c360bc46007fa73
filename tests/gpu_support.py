"""What the test files share on the device's side of a comparison: moving arrays to and from
the GPU, the two equalities, the tolerance check, the golden directory and the package
fixture.  Imported like the *_cases.py modules (`from gpu_support import M  # noqa: F401`
brings the fixture into a test file); it imports without a GPU -- torch.cuda is touched only
inside dev / from_bits -- so the CPU tests use same, same_bits and load from here too.

same is value equality (-0.0 equals +0.0), same_bits compares bit patterns (it does not): a
call site keeps the one it has."""
import os

import numpy as np
import pytest
import torch

from oracle import mx_oracle as O

G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
OUT_TOL = 1e-3  # the attention output, normwise relative error
TDT = {"f16": torch.float16, "bf16": torch.bfloat16}


@pytest.fixture(scope="module")
def M():
    import mx_quantization_amd as m
    return m


def load(name):
    return np.load(os.path.join(G, name))


def dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def dev_opt(x):
    """dev for an optional tensor (a bias)"""
    return None if x is None else dev(x)


def host(t, f32=False):
    """f32: converted to float32 on the device first (a 16-bit tensor has no numpy dtype)"""
    t = t.detach()
    return (t.float() if f32 else t).cpu().numpy()


def from_bits(u16, dt):
    """uint16 bit patterns of the dtype ("f16" / "bf16") -> a device tensor of it"""
    return torch.from_numpy(np.ascontiguousarray(u16).view(np.int16)).view(TDT[dt]).cuda()


def to_f32(u16, dt):
    """uint16 bit patterns of the dtype -> float32 values (exact)"""
    return torch.from_numpy(np.ascontiguousarray(u16).view(np.int16)).view(TDT[dt]).float().numpy()


def to_bits(t):
    """device tensor -> float32 array, or the uint16 patterns of a 16-bit tensor"""
    if t.dtype == torch.float32:
        return host(t)
    return host(t.contiguous().view(torch.int16)).view(np.uint16)


def same(a, b, what="", signed=False):
    """Equal values, NaN against NaN allowed; signed: the zeros' signs too."""
    a, b = np.asarray(a), np.asarray(b)
    assert a.shape == b.shape, (what, a.shape, b.shape)
    ok = (a == b) | (np.isnan(a) & np.isnan(b)) if a.dtype.kind == "f" else a == b
    if signed:
        ok &= (np.signbit(a) == np.signbit(b)) | np.isnan(a)
    if not ok.all():
        bad = np.argwhere(~ok)
        raise AssertionError(f"{what}: {bad.shape[0]}/{ok.size} mismatches, first {bad[:4].tolist()}: "
                             f"{a[tuple(bad[0])]} vs {b[tuple(bad[0])]}")


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def same_bits(got, ref, what="", dt=None, x=None, patterns=False):
    """Equal bit patterns (-0.0 is not +0.0); a NaN on both sides counts as equal, nothing else
    is left out.  Both sides are taken as float32 values.  patterns: uint32 arrays, and uint16
    ones of the 16-bit dtype dt, are bit patterns already and a float32 array is viewed as
    such; the two dtypes must agree.  x: the inputs' patterns, quoted beside a mismatch."""
    if patterns:
        g, r = _bits(got), _bits(ref)
        assert g.dtype == r.dtype, (what, g.dtype, r.dtype)
    else:
        g, r = _bits(np.asarray(got, dtype=np.float32)), _bits(np.asarray(ref, dtype=np.float32))
    assert g.shape == r.shape, (what, g.shape, r.shape)
    if g.dtype == np.uint32:
        inf, mag = 0x7F800000, 0x7FFFFFFF
    else:
        inf, mag = {"f16": 0x7C00, "bf16": 0x7F80}[dt], 0x7FFF
    ok = (g == r) | (((g & mag) > inf) & ((r & mag) > inf))
    if not ok.all():
        bad = np.argwhere(~ok)
        first = []
        for i in map(tuple, bad[:4]):
            src = "" if x is None or np.shape(x) != g.shape else f" x={int(_bits(x)[i]):#x}"
            first.append(f"{list(i)}:{src} got {int(g[i]):#x} want {int(r[i]):#x}")
        raise AssertionError(f"{what}: {bad.shape[0]}/{ok.size} mismatches; " + "; ".join(first))


def out_close(got, ref, tol, what):
    """the NaN pattern bit-exact, the finite elements within tol normwise"""
    same(np.isnan(got), np.isnan(ref), what + " NaN pattern")
    fin = ~np.isnan(ref)
    g, r = got[fin].astype(np.float64), ref[fin].astype(np.float64)
    err = np.linalg.norm(g - r) / max(np.linalg.norm(r), 1e-30)  # (0 when nothing is finite)
    assert err <= tol, f"{what}: normwise error {err:.3e} > {tol}"


def quantize_bfloat_in_dtype(A, bfloat):
    """_quantize_bfloat (elemwise_ops.py:201-216 -> _quantize_elemwise_core :144-160) on a
    float16 / bfloat16 tensor, every step in the tensor's own dtype as torch computes it:
    on bfloat16 the `abs + 0.5` of _round_mantissa (:64-65) itself rounds (243.5 -> 244), so
    the result is not the float32 rounding of the same values."""
    if bfloat in (0, 32):
        return A
    bits = bfloat - 7
    pe = torch.floor(torch.log2(torch.abs(A) + (A == 0).type(A.dtype))).clip(min=-126)
    out = A / (2 ** pe) * (2 ** (bits - 2))
    out = torch.sign(out) * torch.floor(torch.abs(out) + 0.5)
    return out / (2 ** (bits - 2)) * (2 ** pe)


def check_mlp_chain(M, x, W1, b1, W2, b2, act, *, elem_bits=8, cmp, bfloat=0, w1=None, what="", flush=False):
    """The equalities of the MLP chain on the device, each by cmp (same / same_bits): pre is
    mx_linear's and the oracle's fc1; y is mx_linear's and the oracle's fc2 of the activation
    the device produced; y without the hidden copies.  w1: fc1's weight as prepared by the
    caller.  Returns y, pre, act on the host."""
    kw = dict(flush_subnormals=flush, bfloat=bfloat, elem_bits=elem_bits)
    ok = dict(elem=f"int{elem_bits}", flush=flush, bfloat=bfloat or 32)
    y, pre, a = M.mx_mlp(dev(x), dev(W1) if w1 is None else w1, dev_opt(b1), dev(W2), dev_opt(b2), act=act,
                         return_hidden=True, **kw)
    torch.cuda.synchronize()
    cmp(host(pre), host(M.mx_linear(dev(x), dev(W1), dev_opt(b1), **kw)), f"{what} pre vs mx_linear")
    cmp(host(pre), O.mx_linear(x, W1, b1, **ok), f"{what} pre vs oracle")
    cmp(host(y), host(M.mx_linear(a, dev(W2), dev_opt(b2), **kw)), f"{what} y vs mx_linear(act)")
    cmp(host(y), O.mx_linear(host(a), W2, b2, **ok), f"{what} y vs the oracle's Linear of act")
    y2 = M.mx_mlp(dev(x), dev(W1) if w1 is None else w1, dev_opt(b1), dev(W2), dev_opt(b2), act=act, **kw)
    cmp(host(y2), host(y), f"{what} y without the hidden copies")
    return host(y), host(pre), host(a)
