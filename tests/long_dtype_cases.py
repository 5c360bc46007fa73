"""The float16 / bfloat16 cases on rows of 513 .. 4,096 keys (mxa_attention_dt) that tests/golden/gen_long_dtype_golden.py
records from the reference and test_gpu_long_dtype.py / test_long_dtype_cpu.py run: one table, no code.  B = 1, H = 2,
N = 33 (two full 16-row tiles and one ragged row).  q, k, v (and a bias) are not stored: both sides draw them with
rnd(shape, seed + i) followed by .to(dtype)."""
import collections

B, H, N = 1, 2, 33
GATHER16, MFMA_LONG, DENSE_MFMA_LONG, GATHER16_XL, DENSE_MFMA_XL = 1, 6, 7, 8, 9  # include/mxa.h MXA_FIN_*
# fin: the finishing kernel; k = 0: the dense branch; dt: the tensors' dtype ("f32" under autocast); ac: the autocast dtype
Case = collections.namedtuple("Case", "fin T D k dt ac mode bias seed")


def _c(fin, T, D, k, dt, ac=None, mode="ex_pred", bias=False, seed=300):
    return Case(fin, T, D, k, dt, ac, mode, bias, seed)


CASES = [
    _c(GATHER16, 577, 72, 20, "f16"), _c(GATHER16, 577, 72, 20, "bf16"),  # 18 key blocks + 1 key
    _c(GATHER16, 577, 64, 20, "f32", ac="f16"), _c(GATHER16, 577, 64, 20, "f32", ac="f16", mode="MXINT4"),  # DeiT-384's call
    _c(MFMA_LONG, 600, 72, 129, "f16"),
    _c(DENSE_MFMA_LONG, 577, 72, 0, "f16"), _c(DENSE_MFMA_LONG, 577, 72, 0, "bf16"),
    _c(GATHER16_XL, 1025, 72, 16, "f16"),  # one key in the second chunk
    _c(GATHER16_XL, 2085, 72, 20, "f16"), _c(GATHER16_XL, 2085, 72, 20, "bf16"),  # three chunks, the last ragged
    _c(DENSE_MFMA_XL, 1025, 72, 0, "f16"), _c(DENSE_MFMA_XL, 2085, 72, 0, "f16"), _c(DENSE_MFMA_XL, 2085, 72, 0, "bf16"),
    _c(GATHER16_XL, 2085, 72, 20, "f16", bias=True),  # EXTRA && XDT: an (H, N, T) bias of the tensors' dtype
]


def case_id(c):
    return (f"T{c.T}D{c.D}" + (f"k{c.k}" if c.k else "dense") + f"-{c.dt}" + (f"-ac_{c.ac}" if c.ac else "") +
            (f"-{c.mode}" if c.mode != "ex_pred" else "") + ("-bias" if c.bias else ""))
