"""Record what the host side of libmxa.so decides without a GPU: workspace sizes, kernel paths
and first refusals over a grid of arguments (tests/golden/host_table.json, checked by
tests/test_host_table_cpu.py).  ctypes through _native only, so the same script runs on any
commit with the same C ABI:

    python tools/record_host_table.py [out.json]

No row reaches a launch: the attention calls carry a null workspace (the workspace error, or an
earlier refusal, is what is recorded), and the entry points that read a prepared weight's
header past validation are only sized, never called.

The file holds each of the three big tables as its distinct rows plus, per shape, the run-length
coded row numbers (many argument sets get the same answers), and sizes in units of 256 bytes
(every region is 256-B aligned): pack() / unpack().
"""
import ctypes
import itertools
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from mx_quantization_amd import _native as N  # noqa: E402

PH = 16  # a non-null placeholder pointer: nothing reads it

# (B, H, N, T, D, k): the three bench configs, then shapes around the layout's decisions
SHAPES = [(256, 12, 197, 197, 64, 20), (64, 16, 256, 256, 72, 154), (8, 16, 256, 120, 72, 20),
          (2, 2, 40, 40, 64, 7), (2, 2, 40, 40, 64, 33), (2, 2, 40, 40, 64, 34), (2, 2, 96, 96, 64, 70),
          (2, 2, 45, 70, 48, 7), (1, 1, 1, 1, 32, 1), (1, 2, 300, 257, 72, 100), (1, 2, 64, 512, 128, 65),
          (1, 1, 8, 513, 64, 4), (1, 1, 8, 64, 129, 4)]
# both sides of every threshold the finishing-kernel decision reads (T 256 / 257, 512 / 513, 1024 / 1025;
# k 32 / 33, 64 / 65, k = T; D 128 / 129), on the short and the long rows
SHAPES += [(1, 2, 40, 256, 64, 64), (1, 2, 40, 256, 64, 65), (1, 2, 40, 256, 72, 100), (1, 2, 40, 257, 64, 65),
           (1, 2, 40, 200, 64, 200), (1, 2, 40, 513, 64, 64), (1, 2, 40, 513, 64, 65), (1, 2, 33, 513, 32, 32),
           (1, 2, 33, 513, 32, 33), (1, 2, 40, 1024, 72, 154), (1, 2, 40, 1025, 72, 154), (1, 2, 40, 1000, 128, 1000),
           (1, 2, 40, 600, 129, 65)]
FUSED_SHAPES = SHAPES[:15]  # the fused entry points take no long rows: the shapes up to the k = 64 / 65 pair
MODES = sorted(N.PRED_MODES.values())
DTYPES = [(N.DT_F32, 0), (N.DT_F16, 0), (N.DT_BF16, 0), (N.DT_F32, N.DT_F16)]
# the plain attention's axes, in row order: pred_mode, approx, top_k, pred_out, bias, (dtype, score_dtype)
ATTN_AXES = [MODES, [0, 1], [0, 1], [0, 1], [0, 1], DTYPES]
# the fused entry points' (sizes only): pred_mode, approx, top_k, pred_out, bias, (dtype, score_dtype);
# approx = 0 ignores the mode, so it is recorded for the first mode alone
FUSED_AXES = [MODES, [0, 1], [0, 1], [0, 1], [0, 1], [DTYPES[0], DTYPES[3]]]
CS, CKVS, OUTFS = (96, 1152), (160, 1152), (96, 1152)
WIDTHS = (8, 4, 3)  # the *_bits / *_full entry points' elem_bits: MXINT8, MXINT4, an invalid width
# an attention row's columns: size, path, finishing kernel, mxa_attention, mxa_approx_scores ("attn"), then
# ("attn_ext", a table of its own so that the rows repeat) the *_long pair; per width (size, mxa_attention_bits,
# mxa_approx_scores_bits); per width (size, mxa_attention_full, mxa_attention_full_finish_kernel);
# mxa_attention_proj with a null weight pointer.  The *_bits and *_full sizes are recorded as their excess
# over the row's first column (0: the same layout; mxa_attention_full on long rows: its prune-mask words),
# the refusal -1 as it is
ATTN_COLS, ATTN_EXT_COLS = 5, 2 + 3 * len(WIDTHS) + 3 * len(WIDTHS) + 1
# (batch, M, K, Nc) for mxa_matmul; (rows, in, out) for mxa_linear; (rows, in, hidden, out) for mxa_mlp
MATMUL_SHAPES = [(1, 1, 1, 1), (3, 45, 70, 33), (1, 32, 32, 32), (2, 31, 33, 65), (1, 197, 64, 197), (3072, 197, 64, 197),
                 (1024, 256, 72, 256), (128, 256, 72, 120), (1, 8, 256, 8), (1, 8, 257, 8), (4, 7, 31, 4), (2, 64, 96, 1),
                 (1, 1, 4096, 1), (5, 100, 100, 100), (1, 255, 255, 255), (16, 33, 129, 31), (1, 50432, 768, 2304),
                 (2, 128, 128, 128), (1, 1000, 72, 3), (7, 3, 5, 2), (0, 4, 4, 4), (1, 4, 0, 4)]
LINEAR_SHAPES = [(1, 1, 1), (37, 100, 70), (65, 128, 96), (32, 32, 32), (31, 33, 65), (50432, 768, 2304), (50432, 768, 768),
                 (16384, 1152, 3456), (16384, 1152, 1152), (394, 768, 3072), (394, 3072, 768), (45, 96, 96), (90, 96, 288),
                 (140, 160, 192), (1, 4096, 1), (33, 31, 7), (64, 64, 64), (63, 65, 1), (1000, 72, 72), (255, 255, 255),
                 (0, 64, 32), (8, 0, 32)]
MLP_SHAPES = [(1, 1, 1, 1), (65, 128, 96, 64), (37, 100, 70, 50), (32, 32, 32, 32), (31, 33, 65, 17), (50432, 768, 3072, 768),
              (16384, 1152, 4608, 1152), (394, 768, 3072, 768), (45, 96, 384, 96), (33, 31, 7, 5), (64, 64, 256, 64),
              (63, 65, 1, 3), (1000, 72, 288, 72), (255, 255, 255, 255), (1, 4096, 1, 1), (140, 160, 192, 96),
              (96, 96, 100, 96), (129, 192, 768, 192), (2, 2048, 8192, 2048), (7, 3, 5, 2), (0, 64, 32, 16), (8, 64, 0, 16)]


def attn_params(shape, mode, approx, top_k, pred_out, bias, dt):
    B, H, Nq, T, D, k = shape
    p = N.AttnParams()
    p.q = p.k = p.v = p.out = PH
    p.B, p.H, p.N, p.T, p.D, p.k_top = B, H, Nq, T, D, k
    p.pred_mode, p.approx, p.top_k, p.scale = mode, approx, top_k, 0.125
    p.dtype, p.score_dtype = dt
    p.elsa_proj = p.elsa_cos = PH
    if pred_out:
        p.pred_out = p.true_out = PH
    if bias:
        p.bias = PH
    return p


def attn_rows(shape):
    lib = N.lib()
    rows = []
    pj = N.ProjParams()  # a proj Linear without its weight: refused before anything reads one
    pj.out_features, pj.y, pj.y_row_stride = 96, PH, 96
    for combo in itertools.product(*ATTN_AXES):
        p = ctypes.byref(attn_params(shape, *combo))
        excess = lambda v: v if v < 0 else v - row[0]
        row = [lib.mxa_attention_workspace_bytes(p), lib.mxa_attention_path(p), lib.mxa_attention_finish_kernel(p),
               lib.mxa_attention(p, None), lib.mxa_approx_scores(p, None),
               lib.mxa_attention_long(p, None), lib.mxa_approx_scores_long(p, None)]
        for w in WIDTHS:
            row += [excess(lib.mxa_attention_bits_workspace_bytes(p, w)), lib.mxa_attention_bits(p, w, None),
                    lib.mxa_approx_scores_bits(p, w, None)]
        for w in WIDTHS:
            row += [excess(lib.mxa_attention_full_workspace_bytes(p, w)), lib.mxa_attention_full(p, w, None),
                    lib.mxa_attention_full_finish_kernel(p, w)]
        row.append(lib.mxa_attention_proj(p, None, ctypes.byref(pj), None))
        rows.append(row)
    return rows


def fused_rows(shape):
    """per row: qkv[C], proj[out_f], proj with xq[C][out_f], cross[C][C_kv], cross with pj[C][C_kv][out_f]"""
    lib = N.lib()
    rows = []
    for combo in itertools.product(*FUSED_AXES):
        if not combo[1] and combo[0] != MODES[0]:
            continue
        p = ctypes.byref(attn_params(shape, *combo))
        row = []
        xqs, pjs = [N.QkvParams() for _ in CS], [N.ProjParams() for _ in OUTFS]
        for xq, C in zip(xqs, CS):
            xq.C = C
        for pj, of in zip(pjs, OUTFS):
            pj.out_features = of
        row += [lib.mxa_qkv_attention_workspace_bytes(p, ctypes.byref(xq)) for xq in xqs]
        row += [lib.mxa_attention_proj_workspace_bytes(p, None, ctypes.byref(pj)) for pj in pjs]
        row += [lib.mxa_attention_proj_workspace_bytes(p, ctypes.byref(xq), ctypes.byref(pj)) for xq in xqs for pj in pjs]
        for C, Ckv in itertools.product(CS, CKVS):
            xc = N.CrossParams()
            xc.C, xc.C_kv = C, Ckv
            row.append(lib.mxa_cross_attention_workspace_bytes(p, ctypes.byref(xc), None))
            row += [lib.mxa_cross_attention_workspace_bytes(p, ctypes.byref(xc), ctypes.byref(pj)) for pj in pjs]
        rows.append(row)
    return rows


def compute():
    lib = N.lib()
    attn = [attn_rows(s) for s in SHAPES]
    return {
        "shapes": [list(s) for s in SHAPES],
        "attn": [[r[:ATTN_COLS] for r in rows] for rows in attn],
        "attn_ext": [[r[ATTN_COLS:] for r in rows] for rows in attn],
        "fused": [fused_rows(s) for s in FUSED_SHAPES],
        "matmul": [lib.mxa_matmul_workspace_bytes(*s) for s in MATMUL_SHAPES],
        "linear": [lib.mxa_linear_workspace_bytes(*s) for s in LINEAR_SHAPES],
        "mlp": [lib.mxa_mlp_workspace_bytes(r, i, None, h, o) for r, i, h, o in MLP_SHAPES],
    }


def _units(v):
    return v // 256 if v > 0 and v % 256 == 0 else v


def pack(table):
    """compute()'s table as it is stored.  A size that is no multiple of 256 is stored as -v - 2
    (sizes are > 0 or -1), so that unpack() is exact for whatever the library answers."""
    size = lambda v: _units(v) if v <= 0 or v % 256 == 0 else -v - 2
    out = dict(table)
    for key, size_cols in (("attn", (0,)), ("attn_ext", ()), ("fused", range(20))):
        rows, index = {}, []
        for per_shape in table[key]:
            runs = []
            for r in per_shape:
                r = tuple(size(v) if c in size_cols else v for c, v in enumerate(r))
                i = rows.setdefault(r, len(rows))
                if runs and runs[-1][0] == i:
                    runs[-1][1] += 1
                else:
                    runs.append([i, 1])
            index.append(runs)
        out[key] = {"rows": [list(r) for r in rows], "index": index}
    for key in ("matmul", "linear", "mlp"):
        out[key] = [size(v) for v in table[key]]
    return out


def unpack(stored):
    size = lambda v: v * 256 if v > 0 else (v if v >= -1 else -v - 2)
    out = dict(stored)
    for key, size_cols in (("attn", (0,)), ("attn_ext", ()), ("fused", range(20))):
        if key not in stored:  # a file recorded before the table had this part
            continue
        rows = [[size(v) if c in size_cols else v for c, v in enumerate(r)] for r in stored[key]["rows"]]
        out[key] = [[rows[i] for i, n in runs for _ in range(n)] for runs in stored[key]["index"]]
    for key in ("matmul", "linear", "mlp"):
        out[key] = [size(v) for v in stored[key]]
    return out


if __name__ == "__main__":
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "tests", "golden", "host_table.json")
    with open(out, "w") as f:
        json.dump(pack(compute()), f, separators=(",", ":"))
        f.write("\n")
    print(out, os.path.getsize(out), "bytes")
