"""Inputs and the oracle chain of the self-attention block on rows of 513 .. 1,024 keys
(tests/test_long_block_cpu.py, tests/test_gpu_long_block.py; include/mxa.h mxa_qkv_attention_full,
mxa_attention_proj_full): cross_cases.self_case / self_chain's construction on a shape tuple -- the qkv
mx.Linear, O.qkv_split, the attention core at the width, each computed once and left unchanged.
Nothing here touches the device.

The CPU file proves with the oracle alone that every case's eligible shares of the row-wise bound
(gpu_support.out_row_bound) are within the caps and that the heads of a case keep different keys; the
GPU file only compares."""
import collections
import functools

import numpy as np

import cross_cases as CC
from gpu_support import ELEM, out_row_bound
from oracle import mx_oracle as O

# shape (B, N, C, H); k = 0: dense (the qkv front only); wsc: the qkv weight's scale -- 0.2 peaks the
# softmax of the two cases whose rows keep more than 64 keys (at 0.05 the flat rows exceed the row cap)
Case = collections.namedtuple("Case", "shape k wsc")
CASES = {
    # LONG + XO, KS = 5; 17 key blocks, the last of one key; the last 16-row tile of one row; two images
    "d32k20": Case((2, 513, 64, 2), 20, 0.05),
    "d32k32": Case((1, 513, 64, 2), 32, 0.05),     # KS = 8, the last k with direct codes
    "d32k33": Case((1, 513, 64, 2), 33, 0.05),     # the first k on the copy route at D % 32 == 0
    "d72k20": Case((1, 520, 144, 2), 20, 0.05),    # PixArt's head width: a ragged D block, the copy route
    "d64k30": Case((1, 600, 128, 2), 30, 0.05),    # NB = 2 in the XO epilogue
    "d128k20": Case((1, 513, 256, 2), 20, 0.05),   # NB = 4
    "d32t1024": Case((1, 1024, 64, 2), 20, 0.05),  # the longest row
    "d64k129": Case((1, 513, 128, 2), 129, 0.2),   # finish_qk_long_kernel behind the projection; proj by copy
    "d72dense": Case((1, 513, 144, 2), 0, 0.2),    # the qkv front only
}
TOPK = tuple(n for n, c in CASES.items() if c.k)


def kernel_of(k):
    """gpu_support.n_add_and_chain's entry of the kernel that finishes a case (mxa_launch.hpp
    finish_choice on rows over 512 keys: the tiled MFMA kernel keeps finish_qk_kernel's counts)"""
    return "dense_qk" if not k else ("qk" if k > 64 else "fin16")


def codes_direct(D, k, bits):
    """the 16-row finishing kernel writes the proj Linear's MX input codes itself (else the fp32
    workspace copy and the row quantizer): width 8, D % 32 == 0, k <= 32"""
    return bits == 8 and D % 32 == 0 and 0 < k <= 32


@functools.lru_cache(maxsize=None)
def case(name):
    """x, Wqkv, bqkv, Wo, bo, drawn in this order"""
    (B, N, C, H), _, wsc = CASES[name]
    f = CC._normal(np.random.default_rng(9000 + B * 100 + N * 7 + C))
    return f(B, N, C), f(3 * C, C, sc=wsc), f(3 * C, sc=0.1), f(C, C, sc=0.05), f(C, sc=0.1)


def mask_bias(B, N):
    """a (B, 1, N, N) mask bias of 0 / -10000: each query row's own parity class of keys stays"""
    i = np.arange(N)
    m = np.where((i[:, None] + i[None, :]) % 2 == 0, 0.0, -10000.0).astype(np.float32)
    return np.ascontiguousarray(np.broadcast_to(m[None, None], (B, 1, N, N)))


@functools.lru_cache(maxsize=None)
def chain(name, mode="ex_pred", flush=False, bfloat=0, elem="int8", approx=True, masked=False):
    """{qkv, qh, kh, vh, bias, r} of a case: the qkv Linear, O.qkv_split, the attention core"""
    (B, N, C, H), k, _ = CASES[name]
    x, W, b, _, _ = case(name)
    kw = dict(elem=elem, flush=flush, bfloat=bfloat or 32)
    qkv = O.mx_linear(x, W, b, **kw)
    qh, kh, vh = (np.ascontiguousarray(t) for t in O.qkv_split(qkv, H))
    bias = mask_bias(B, N) if masked else None
    akw = dict(top_k=False) if not k else dict(k_top=k, **(dict(pred_mode=mode) if approx else dict(approx=False)))
    r = O.attention(qh, kh, vh, (C // H) ** -0.5, bias=bias, **akw, **kw)
    return dict(qkv=qkv, qh=qh, kh=kh, vh=vh, bias=bias, r=r)


def shares(name, bits, **kw):
    """the eligible shares (elements, rows) of a case's row-wise bound, from the oracle alone"""
    c = chain(name, elem=ELEM[bits], **kw)
    return out_row_bound(c["r"], c["vh"], kernel_of(CASES[name].k), bits)[2]
