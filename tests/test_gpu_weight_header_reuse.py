"""A prepared weight at an address the host has noted another header for: torch's caching
allocator hands a freed weight's block to the next buffer of its size, and the library's note
of the freed weight's header (pointer -> header) is then stale.  The device's copy decides."""
import numpy as np
import pytest
import torch

from gpu_support import M, dev, host, same  # noqa: F401

pytestmark = pytest.mark.gpu


def test_copied_weight_at_a_freed_weights_address(M):
    rng = np.random.default_rng(11)
    x = dev(rng.standard_normal((1, 64, 128), dtype=np.float32))
    W = dev(rng.standard_normal((3 * 128, 128), dtype=np.float32) * np.float32(0.05))
    wq = M.LinearWeightMX(W, 64)
    o1, i1 = M.mx_qkv_attention(x, wq, None, 2, 0.125, k_top=10)
    other = M.LinearWeightMX(W, 64, flush_subnormals=True)  # the same size, another header
    M.mx_qkv_attention(x, other, None, 2, 0.125, k_top=10, flush_subnormals=True)
    freed = other.buf.data_ptr()
    del other
    cp = M.LinearWeightMX.__new__(M.LinearWeightMX)
    cp.__dict__.update(wq.__dict__)
    cp.buf = wq.buf.clone()  # usually the block just freed; the call must succeed wherever it lies
    print("the copy took the freed weight's address:", cp.buf.data_ptr() == freed)
    o2, i2 = M.mx_qkv_attention(x, cp, None, 2, 0.125, k_top=10)
    same(host(i2), host(i1), "idx")
    assert torch.equal(o2, o1)
    # a header that really differs is still refused (the device's copy says flush = 0)
    cp.flush = True
    with pytest.raises(M.NativeError):
        M.mx_qkv_attention(x, cp, None, 2, 0.125, k_top=10, flush_subnormals=True)
