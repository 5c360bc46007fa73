"""The library's host-side decisions against a recorded table (tests/golden/host_table.json,
written by tools/record_host_table.py): every workspace size, the kernel path and finishing
kernel, and the first refusal of mxa_attention / mxa_approx_scores and their *_long, *_bits and
*_full siblings (at widths 8, 4 and an invalid one) with a null workspace, over shapes x score
modes x flags x dtypes.  Nothing launches, so it runs without a GPU.  The
table is a record of what the library answered when it was written: a change of the host code
that is meant to leave sizes and refusals alone must reproduce it, one that is meant to change
them re-records it."""
import importlib.util
import json
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def tables():
    spec = importlib.util.spec_from_file_location("record_host_table", os.path.join(ROOT, "tools", "record_host_table.py"))
    rec = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(rec)
    with open(os.path.join(ROOT, "tests", "golden", "host_table.json")) as f:
        want = rec.unpack(json.load(f))
    return rec, rec.compute(), want


def test_table_covers_the_recorder(tables):
    rec, got, want = tables
    assert want["shapes"] == [list(s) for s in rec.SHAPES]
    assert set(got) == set(want)
    assert len(want["attn"]) == len(rec.SHAPES) >= 26
    n_attn = 1
    for ax in rec.ATTN_AXES:
        n_attn *= len(ax)
    assert all(len(rows) == n_attn and all(len(r) == rec.ATTN_COLS == 5 for r in rows) for rows in want["attn"])
    assert len(want["attn_ext"]) == len(rec.SHAPES)
    assert all(len(rows) == n_attn and all(len(r) == rec.ATTN_EXT_COLS == 21 for r in rows) for rows in want["attn_ext"])
    assert len(want["fused"]) == len(rec.FUSED_SHAPES) >= 15
    assert all(rows and all(len(r) == 20 for r in rows) for rows in want["fused"])
    assert len(want["matmul"]) == len(rec.MATMUL_SHAPES) >= 20
    assert len(want["linear"]) == len(rec.LINEAR_SHAPES) >= 20
    assert len(want["mlp"]) == len(rec.MLP_SHAPES) >= 20


@pytest.mark.parametrize("key", ["attn", "attn_ext", "fused"])
def test_attention_rows(tables, key):
    rec, got, want = tables
    assert len(got[key]) == len(want[key])
    for shape, g, w in zip(rec.SHAPES, got[key], want[key]):
        assert len(g) == len(w), shape
        bad = [(i, a, b) for i, (a, b) in enumerate(zip(g, w)) if a != b]
        assert not bad, f"{key} {shape}: {len(bad)} rows differ, first (row, got, recorded): {bad[0]}"


@pytest.mark.parametrize("key", ["matmul", "linear", "mlp"])
def test_linear_family_sizes(tables, key):
    rec, got, want = tables
    assert got[key] == want[key]
