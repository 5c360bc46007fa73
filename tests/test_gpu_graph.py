"""Every entry point captured into a graph (torch.cuda.graph) and replayed on other inputs
(include/mxa.h "Streams": while `stream` is capturing, a call keeps everything on `stream`; a weight
whose header the host does not know is refused, because reading it would synchronise).

One protocol for every case of tests/graph_cases.py (replayed): static inputs holding A, the eager
results for A and for B kept as host bytes; a warm-up call on a side stream; one call captured with
the inputs holding A; then every output poisoned (NaN, -1), B copied in, one replay -- the bytes of
the eager call on B -- and the same with A and two replays in a row.  What a capture could bake in
shows as A's bytes in B's replay: a host decision taken from the data, a table built only on the
forked path, a constant copied from host memory that is gone at replay.  One case per family is also
compared with the oracle, and after every graph an eager forked call on the default stream writes the
bytes it wrote before any capture (the lane's stream and events survive a capture that skipped them).

Then: mxa_attention_full captured directly on a workspace and a stream of the test's own, two calls in
one graph; and the refusal of an unknown weight header under capture.  (The captured graph's shape is not
asserted: CUDAGraph.debug_dump writes no DOT file with the ROCm build of torch the suite runs on.)"""
import numpy as np
import pytest
import torch

import graph_cases as GR
from gpu_support import M, OUT_TOL, bind, check_attn, dev, host, launch, out_close, rnd, same, same_bytes, workspace  # noqa: F401
from oracle import mx_oracle as O

pytestmark = pytest.mark.gpu


def hosts(names, outs):
    """the op's outputs by name as host arrays (an output the call does not have, None, left out)"""
    return {n: host(t) for n, t in zip(names, outs) if t is not None}


def poison(outs):
    for t in outs:
        if t is not None:
            t.fill_(float("nan") if t.is_floating_point() else -1)


def warm_up(fn):
    """torch's capture recipe: the call once on a side stream, joined both ways"""
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        fn()
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()


def capture(fn, **kw):
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, **kw):
        outs = fn()
    return g, outs


@pytest.fixture(scope="module")
def forked_eager(M):
    """check(what): the eager forked call of graph_cases.FORKED_EAGER on the default stream, a workspace of its own,
    writes the bytes it wrote when this fixture was made -- before any capture of this module"""
    n, k = GR.FORKED_EAGER
    t = [dev(x) for x in GR.qkv(n, n, 64, 3).values()]

    def call():
        p, res, _ = bind(M, *t, GR._scale(64), k)
        launch(M, p, workspace(M, p), torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        return {a: host(x) for a, x in res.items()}

    want = call()
    return lambda what: same_bytes(call(), want, what + ": the eager forked call after the graph")


def replayed(M, c, forked_eager):
    """The protocol of the module's docstring on one case.  Returns the graph, the static inputs and outputs (device
    tensors by name) and the outputs of the last replay, on A, as host arrays."""
    A, B = c.inputs("A"), c.inputs("B")
    consts = c.consts(M)
    t = {n: dev(a) for n, a in A.items()}

    def load(X):
        for n in t:
            t[n].copy_(torch.from_numpy(np.ascontiguousarray(X[n])))

    def call():
        return tuple(c.call(M, t, consts))

    want_a = hosts(c.outs, call())
    load(B)
    want_b = hosts(c.outs, call())
    torch.cuda.synchronize()
    assert list(want_a) == list(want_b) and want_a
    for n in want_a:  # (an output that cannot tell A from B would prove nothing; topk_k0's empty outputs and zero mask aside)
        assert c.name == "topk_k0" or not np.array_equal(want_a[n], want_b[n]), (c.name, n)
    load(A)
    warm_up(call)
    g, outs = capture(call)
    poison(outs)
    load(B)
    g.replay()
    torch.cuda.synchronize()
    same_bytes(hosts(c.outs, outs), want_b, f"{c.name}: replay on B")
    poison(outs)
    load(A)
    g.replay()
    g.replay()
    torch.cuda.synchronize()
    got = hosts(c.outs, outs)
    same_bytes(got, want_a, f"{c.name}: two replays on A")
    forked_eager(c.name)
    return g, t, dict(zip(c.outs, outs)), got


def check_oracle(M, c, outs, got):
    """the replayed result on A against the oracle, by the family's existing comparison"""
    r, A = c.oracle("A"), c.inputs("A")
    if c.family == "attn":
        got = dict(got, mask=host(M.unpack_mask(outs["mask"], c.facts["T"])))
        check_attn(got, r, c.name)
        out_close(got["out"], r["out"], OUT_TOL, c.name + " out")
    elif c.family in ("block", "glue"):
        same(got["idx"], r["idx"], c.name + " idx")
        out_close(got["out"], r["out"], OUT_TOL, c.name + " out")
    elif c.family == "mlp":
        _, _, _, W2, b2 = GR.MLP
        same(got["pre"], r["pre"], c.name + " pre")
        same(got["y"], O.mx_linear(got["act"], W2, b2), c.name + " y vs the oracle's Linear of act")
    elif c.family == "topk":
        same(got["vals"], r["vals"], c.name + " vals")
        same(got["idx"], r["idx"], c.name + " idx")
        same(host(M.unpack_mask(outs["mask"], A["vals"].shape[-1])), O.prune_mask(r["idx"], A["vals"].shape[-1]), c.name + " mask")
    else:  # scores, linear, matmul, quant: the one output, equal values
        (name,) = [n for n in c.outs if n in r]
        same(got[name], r[name], f"{c.name} {name}")


@pytest.mark.parametrize("name", list(GR.CASES))
def test_captured_call_replays_on_new_inputs(M, forked_eager, name):
    c = GR.CASES[name]
    _, _, outs, got = replayed(M, c, forked_eager)
    if name == "topk_k0":
        assert not got["mask"].any()  # nothing kept: the poisoned words are cleared at every replay
    if c.check:
        check_oracle(M, c, outs, got)


# ---- the C entry point captured directly --------------------------------------------------------
def test_two_calls_in_one_graph_on_a_shared_workspace(M, forked_eager):
    """mxa_attention_full twice -- N = 197 and N = 70, both forked when eager -- captured into one graph on a stream
    and a workspace of the test's own: the second call's builders overwrite the tables the first call's finishing
    kernel reads, in stream order alone.  Each replayed call's out, idx and mask words are the bytes the call writes
    alone (eager, a workspace of its own); replayed three times."""
    sc = GR._scale(64)
    sets = [GR.qkv(197, 197, 64, 1), GR.qkv(70, 70, 64, 2)]
    want = []
    for x in sets:
        t = [dev(a) for a in x.values()]
        p, res, _ = bind(M, *t, sc, 20)
        launch(M, p, workspace(M, p), torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        want.append({a: host(r) for a, r in res.items()})
    keep = [[dev(a) for a in x.values()] for x in sets]
    calls = [bind(M, *t, sc, 20) for t in keep]
    ws = workspace(M, calls[0][0])
    assert ws.numel() >= workspace(M, calls[1][0]).numel()
    own = torch.cuda.Stream()
    torch.cuda.synchronize()

    def both():
        for p, _, _ in calls:
            launch(M, p, ws, torch.cuda.current_stream().cuda_stream)

    g, _ = capture(both, stream=own)
    for rep in range(3):
        for _, res, _ in calls:
            poison(res.values())
        g.replay()
        torch.cuda.synchronize()
        for i, (_, res, _) in enumerate(calls):
            same_bytes({a: host(r) for a, r in res.items()}, want[i], f"replay {rep} call {i}")
    forked_eager("two calls in one graph")


# ---- a weight whose header the host does not know -----------------------------------------------
ARG = "(status -1)"  # MXA_ERR_ARG in NativeError's text


def test_unknown_weight_header_is_refused_under_capture(M, forked_eager):
    """A prepared weight copied to a fresh allocation (test_gpu_weight_header_reuse.py): the host has no note of its
    header, and reading it from the device would synchronise -- under capture mx_linear and mx_qkv_attention refuse it
    (MXA_ERR_ARG); the call on the known weight behind the refusals, in the same capture, replays correctly; after the
    capture the eager call on the copy reads the header once and succeeds, and so does a second capture.
    (A shape and settings no other test prepares a weight with: a stale note of a freed weight cannot vouch for the copy.)"""
    Bn, N, C, Hn, k = 2, 40, 96, 3, 7
    D = C // Hn
    x = dev(rnd((Bn, N, C), 71))
    b = dev(rnd((3 * C,), 73, 0.1))
    known = M.LinearWeightMX(dev(rnd((3 * C, C), 72, 0.05)), D, flush_subnormals=True)

    def lin(w):
        return (M.mx_linear(x, w, b, flush_subnormals=True),)

    def attn(w):
        return M.mx_qkv_attention(x, w, b, Hn, GR._scale(D), k_top=k, flush_subnormals=True)

    def both(w):
        return lin(w) + tuple(attn(w))

    names = ("y", "out", "idx")
    want = hosts(names, both(known))
    warm_up(lambda: both(known))
    cp = M.LinearWeightMX.__new__(M.LinearWeightMX)
    cp.__dict__.update(known.__dict__)
    cp.buf = known.buf.clone()
    torch.cuda.synchronize()

    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for fn in (lin, attn):
            with pytest.raises(M.NativeError) as e:
                fn(cp)
            assert ARG in str(e.value), str(e.value)
        outs = both(known)
    poison(outs)
    g.replay()
    torch.cuda.synchronize()
    same_bytes(hosts(names, outs), want, "the known weight behind the refusals")

    same_bytes(hosts(names, both(cp)), want, "the copy, eager: its header is read once")
    g2, outs2 = capture(lambda: both(cp))
    for rep in range(2):
        poison(outs2)
        g2.replay()
        torch.cuda.synchronize()
        same_bytes(hosts(names, outs2), want, f"the copy, captured, replay {rep}")
    forked_eager("weight header")
