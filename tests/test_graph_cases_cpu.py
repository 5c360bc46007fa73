"""tests/graph_cases.py from the oracle alone: a replay on B that silently reused A's data cannot pass
as B, the cases that are to fork when eager meet the forking condition, and each case reaches the
path its name states."""
import numpy as np
import pytest

import gate_cases as GC
import graph_cases as GR
import topk_cases as TC
from gpu_support import ELEM, finish_kernel_of
from oracle import mx_oracle as O

WITH_IDX = [n for n, c in GR.CASES.items() if "idx" in c.outs and c.facts.get("k", 1)]
PACKS = ("ex_pred", "two_step_leading_ones", "MXINT4", "partial_Q", "partial_K", "true_ex")  # mxa_launch.hpp sel_packs' modes


def forks(f):
    """mxa_attn.hip attention_impl's condition on a call on q, k, v: top-k, rows of at most 256 keys whose scores
    pack (no bias), and the one-lane tail behind the packed pass (mxa_launch.hpp sel_tail_width == kTailPref)"""
    return bool(f["k"]) and not f["bias"] and f["T"] <= 256 and f["mode"] in PACKS and TC.tail_width_for(f["T"], f["k"]) == TC.TAIL_PREF


def test_every_entry_point_has_a_case():
    fam = {c.family for c in GR.CASES.values()}
    assert fam == {"attn", "scores", "block", "linear", "mlp", "matmul", "quant", "topk", "glue"}
    assert {f: sum(c.check for c in GR.CASES.values() if c.family == f) for f in fam} == dict.fromkeys(fam, 1)


@pytest.mark.parametrize("name", list(GR.CASES))
def test_inputs_of_a_and_b_differ_and_agree_in_layout(name):
    a, b = GR.CASES[name].inputs("A"), GR.CASES[name].inputs("B")
    assert list(a) == list(b)
    for n in a:
        assert a[n].shape == b[n].shape and a[n].dtype == b[n].dtype, n
        assert not np.array_equal(a[n], b[n]), n


@pytest.mark.parametrize("name", WITH_IDX)
def test_kept_indices_of_a_and_b_differ(name):
    """in every (batch, head) slice -- and in every row of the standalone top-k's small case"""
    c = GR.CASES[name]
    ia, ib = c.oracle("A")["idx"], c.oracle("B")["idx"]
    assert ia.shape == ib.shape and ia.shape[-1] == (c.facts.get("k") or ia.shape[-1])
    diff = (ia != ib).any(-1)
    assert diff.reshape(-1, diff.shape[-1]).any(-1).all(), name
    assert diff.mean() > 0.9, (name, diff.mean())


def test_forked_cases_fork_and_the_others_do_not():
    for c in GR.CASES.values():
        if c.family == "attn":
            assert forks(c.facts) == c.forked, c.name
    n, k = GR.FORKED_EAGER
    assert forks(dict(k=k, bias=False, T=n, mode="ex_pred")) and GR.CASES["forked_n197"].facts["T"] == n
    assert sorted(c.facts["T"] for c in GR.CASES.values() if c.name.startswith("forked_")) == [70, 197]
    assert GR.CASES["width4"].forked and GR.CASES["f16"].forked  # (the 4-bit and the float16 call fork as well)


def test_attention_cases_reach_their_paths():
    f = {n: c.facts for n, c in GR.CASES.items() if c.family == "attn"}
    kern = {n: finish_kernel_of(x["T"], x["D"], x["k"]) for n, x in f.items() if x["T"] <= 512}
    # the packed pass (the scores pack, k > 0) with no tail behind it
    assert TC.tail_width_for(197, 100) == 0 and not f["packed_no_tail"]["bias"] and f["packed_no_tail"]["mode"] in PACKS
    assert kern["packed_no_tail"] == "qk" and kern["gather32"] == "fin32" and kern["dense"] == "dense_qk"
    assert kern["forked_n70"] == kern["forked_n197"] == "fin16"
    for n in ("long_k20", "long_k154", "long_dense"):  # rows of 513 .. 1,024 keys: select_long; k > 64 and dense: finish_qk_long
        assert 512 < f[n]["T"] <= 1024
    assert f["long_k20"]["k"] <= 64 < f["long_k154"]["k"] and f["long_dense"]["k"] == 0
    assert f["bias_flush"]["bias"] and GR.CASES["bias_flush"].inputs("A")["bias"].shape == (GR.B, 1, 1, 77)
    assert f["width4"]["bits"] == 4 and f["elsa"]["mode"] == "ELSA" and f["elsa"]["D"] == 64
    assert GR.CASES["f16"].inputs("A")["q"].dtype == np.float16
    assert GR.CASES["qkv_proj_long"].facts["T"] > 512 >= GR.CASES["qkv_w8"].facts["T"]


@pytest.mark.parametrize("bits", [8, 4])
def test_linear_cases_sit_on_the_digit_operands(bits):
    """the one-group weight's rows and columns are within the width's digit spread for A and B (gate_cases): the
    digit kernel sums them as digits; the weight in groups of 24 columns has no digits (the tile kernel)"""
    x, W, _ = GR.LINEAR
    for which in "AB":
        GC.assert_side(GR.CASES[f"linear_digit_w{bits}"].inputs(which)["x"], W, "digits", what=which, elem=ELEM[bits])
    assert GR.LINEAR_GROUPS["digit"] == W.shape[0] and GR.LINEAR_GROUPS["tile"] % 32 and W.shape[0] % GR.LINEAR_GROUPS["tile"] == 0


def test_topk_rows_pack_and_do_not():
    """rows 10 .. 19 need the low mantissa byte (the 64-bit pass), the others pack; row 5 holds zeros of both signs; the
    tail runs behind the packed pass at (197, 20), the wave kernel takes n = 600"""
    for which in "AB":
        v = GR.topk_rows(which)
        packs = ~((v.view(np.uint32) & 0xFF) != 0).any(-1)
        want = np.ones(70, bool)
        want[10:20] = False
        assert np.array_equal(packs, want), which
        assert np.signbit(v[5][v[5] == 0]).any() and not np.signbit(v[5][v[5] == 0]).all()
    assert TC.tail_width_for(197, 20) == TC.TAIL_PREF
    assert GR.CASES["topk_n600"].inputs("A")["vals"].shape[-1] > 512
    assert O.topk(GR.topk_rows("A"), 20)[1].shape == (70, 20)
