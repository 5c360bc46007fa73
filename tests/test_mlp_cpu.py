"""CPU checks of the MLP entry point (include/mxa.h mxa_mlp): its argument validation runs
before any launch, and mxa_mlp_workspace_bytes follows the formula restated here."""
from mx_quantization_amd import _native as N


def _al(n):
    return (n + 255) // 256 * 256


def _mx_rows(rows, cols):
    """MX rows of a (rows, cols) matrix: MFMA-ready codes of whole 32-row blocks (32 B per
    block of 32 columns), then an int16 exponent per row and block; each region to 256 B."""
    nb = (cols + 31) // 32
    return _al((rows + 31) // 32 * 32 * nb * 32) + _al(rows * nb * 2)


def mlp_workspace(rows, inf, hidden, fused):
    """x's MX rows + the hidden matrix's MX rows (fc2's input codes); the fallback -- an fc1
    that does not run on the quantizing digit kernel -- adds the fp32 hidden matrix.  (The
    fused size needs a prepared w1 on the device: tests/test_gpu_mlp.py checks it there.)"""
    return _mx_rows(rows, inf) + _mx_rows(rows, hidden) + (0 if fused else _al(rows * hidden * 4))


def test_mlp_arg_errors():
    lib = N.lib()
    args = dict(x=1, rows=4, inf=32, xs=32, w1=1, hid=32, b1=None, act=0, w2=1, outf=32, b2=None, y=1, ys=32)

    def call(**kw):
        a = dict(args, **kw)
        return lib.mxa_mlp(a["x"], a["rows"], a["inf"], a["xs"], a["w1"], a["hid"], a["b1"], a["act"], a["w2"], a["outf"],
                           a["b2"], a["y"], a["ys"], None, None, 0, 0, None, 0, None)

    for null in ("x", "w1", "w2", "y"):
        assert call(**{null: None}) == -1, null  # MXA_ERR_ARG
    assert call(act=2) == -1 and call(act=-1) == -1
    assert call(xs=31) == -1 and call(ys=31) == -1
    assert call(rows=0) == -1 and call(hid=0) == -1
    assert lib.mxa_mlp(1, 4, 32, 32, 1, 32, None, 0, 1, 32, None, 1, 32, None, None, 0, 9, None, 0, None) == -1  # bfloat


def test_mlp_workspace_formula():
    lib = N.lib()
    # a weight this process has not seen (and none at all): the fallback's size, which serves both paths
    for rows, inf, hid, outf in ((70, 96, 160, 40), (50432, 768, 3072, 768), (33, 100, 136, 96)):
        want = mlp_workspace(rows, inf, hid, fused=False)
        assert lib.mxa_mlp_workspace_bytes(rows, inf, None, hid, outf) == want
        assert lib.mxa_mlp_workspace_bytes(rows, inf, 4096, hid, outf) == want
        assert want - mlp_workspace(rows, inf, hid, fused=True) == _al(rows * hid * 4)
    # DeiT-base: the fp32 hidden matrix is 620 MB of the fallback's workspace, the codes 165 MB
    assert mlp_workspace(50432, 768, 3072, True) == _al(50432 * 768) + _al(50432 * 24 * 2) + _al(50432 * 3072) + _al(50432 * 96 * 2)
    assert lib.mxa_mlp_workspace_bytes(0, 96, None, 160, 40) == -1
    assert lib.mxa_mlp_workspace_bytes(70, 96, None, 0, 40) == -1


def test_abi_version_unchanged():
    assert N.lib().mxa_abi_version() == N.ABI_VERSION == 6
