"""The calls tests/test_gpu_graph.py captures into a graph, one Case per call: two input sets, A and
B (a replay on B that silently reused A's data must not pass), the constants the call keeps between
replays (prepared weights, ELSA's matrix), the call itself and the oracle's result for either set.
Shapes are the smallest that reach the path a case names; inputs come from the existing case tables
where one of theirs fits.  Nothing here touches the device at import; consts and call run on it.

tests/test_graph_cases_cpu.py proves with the oracle alone that A's and B's kept indices differ for
every case that returns indices, that the forked cases meet the forking condition and that each
attention-core case reaches the path it names.

The float16 case's oracle is the float32 oracle on the float16 values (exact in float32): the CPU test
takes from it only that A and B keep different keys; the GPU test compares that case with the eager
call alone."""
import collections
import functools
import os

import numpy as np

import cross_cases as CC
import int4_cases as IC
import long_block_cases as LB
import mlp_cases as MC
import topk_cases as TC
from gpu_support import ELEM, G, dev, rnd
from oracle import mx_oracle as O

F32 = np.float32
B, H = 2, 2  # the attention core's cases
# inputs, oracle: which ("A" / "B") -> dict of arrays (oracle: None where the case is compared with the
# eager call alone); consts: M -> dict of what stays on the device between replays; call: (M, t, c) ->
# the op's outputs as a tuple named by outs (an entry may be None: idx on the dense branch); check: this
# case's replayed result is also compared with the oracle (one per family); forked: the call forks when eager
Case = collections.namedtuple("Case", "name family inputs consts call outs oracle check forked facts")
CASES = collections.OrderedDict()


def _add(name, family, inputs, call, outs, oracle=None, consts=None, check=False, forked=False, facts=None):
    assert name not in CASES
    CASES[name] = Case(name, family, functools.lru_cache(maxsize=None)(inputs), consts or (lambda M: {}), call, outs,
                       functools.lru_cache(maxsize=None)(oracle) if oracle else None, check, forked, facts or {})


def _scale(D):
    return float(F32(D ** -0.5))


# ---- the attention core -------------------------------------------------------------------------
def qkv(N, T, D, seed, dtype=F32):
    """test_gpu_side_lane.inputs' draws at N = T: rnd((B, H, rows, D), 10 seed + i)"""
    return dict(zip("qkv", (rnd((B, H, r, D), 10 * seed + i).astype(dtype) for i, r in enumerate((N, T, T)))))


def mask_bias(T, which):
    """(B, 1, 1, T): cross_cases.mask_bias for A (the second half of the keys masked); B masks the first third"""
    if which == "A":
        return CC.mask_bias(B, T)
    return np.where(np.arange(T) >= T // 3, 0.0, -10000.0).astype(F32)[None, None, None, :].repeat(B, 0)


@functools.lru_cache(maxsize=None)
def elsa_matrix(D):
    """an orthogonal (D, D) matrix (the Q of a random matrix's QR)"""
    return np.ascontiguousarray(np.linalg.qr(rnd((D, D), 77).astype(np.float64))[0].astype(F32))


def _attn(name, N, T, D, k, bias=False, dtype=F32, check=False, forked=False, **kw):
    """mx_topk_attention on (B, H, N, D) queries and T keys; k = 0: dense; kw: the op's further keywords"""
    elsa = kw.get("pred_mode") == "ELSA"
    okw = dict(k_top=k) if k else dict(top_k=False)

    def inputs(which):
        t = qkv(N, T, D, 1 if which == "A" else 2, dtype)
        if bias:
            t["bias"] = mask_bias(T, which).astype(dtype)
        return t

    def consts(M):
        return dict(elsa_proj=dev(elsa_matrix(D))) if elsa else {}

    def call(M, t, c):
        r = M.mx_topk_attention(t["q"], t["k"], t["v"], _scale(D), bias=t.get("bias"), return_mask=bool(k),
                                elsa_proj=c.get("elsa_proj"), **okw, **kw)
        return r if k else r[:2]

    def oracle(which):
        t = {a: x.astype(F32) for a, x in inputs(which).items()}
        return O.attention(t["q"], t["k"], t["v"], _scale(D), bias=t.get("bias"), elem=ELEM[kw.get("elem_bits", 8)],
                           flush=kw.get("flush_subnormals", False), elsa_proj=elsa_matrix(D) if elsa else None,
                           **okw, **({"pred_mode": kw["pred_mode"]} if "pred_mode" in kw else {}))

    _add(name, "attn", inputs, call, ("out", "idx", "mask") if k else ("out", "idx"), oracle, consts, check, forked,
         dict(N=N, T=T, D=D, k=k, bias=bias, mode=kw.get("pred_mode", "ex_pred"), bits=kw.get("elem_bits", 8)))


_attn("forked_n70", 70, 70, 64, 20, forked=True)
_attn("forked_n197", 197, 197, 64, 20, forked=True, check=True)
_attn("packed_no_tail", 197, 197, 64, 100)
_attn("gather32", 40, 300, 72, 65)
_attn("long_k20", 600, 600, 72, 20)
_attn("long_k154", 600, 600, 72, 154)
_attn("long_dense", 600, 600, 72, 0)
_attn("dense", 197, 197, 64, 0)
_attn("bias_flush", 40, 77, 48, 20, bias=True, flush_subnormals=True)
_attn("width4", 70, 70, 64, 20, forked=True, elem_bits=4, pred_mode="MXINT4")
_attn("elsa", 70, 70, 64, 20, pred_mode="ELSA")
_attn("f16", 70, 70, 64, 20, forked=True, dtype=np.float16)
FORKED_EAGER = (197, 20)  # the eager forked call made after every replayed graph: qkv(197, 197, 64, 3), k


def _scores():
    def call(M, t, c):
        return (M.mx_approx_scores(t["q"], t["k"], "ex_pred"),)

    def oracle(which):
        t = qkv(70, 70, 64, 1 if which == "A" else 2)
        aq, ak = O.approx_operands(t["q"], t["k"], "ex_pred")
        return dict(pred=O.exact_matmul_f32(aq, np.swapaxes(ak, -1, -2)))

    _add("approx_scores", "scores", lambda which: {a: x for a, x in qkv(70, 70, 64, 1 if which == "A" else 2).items() if a != "v"},
         call, ("pred",), oracle, check=True)


_scores()


# ---- the fused blocks ---------------------------------------------------------------------------
def _weight(M, W, group, bits):
    return M.LinearWeightMX(dev(W), group, elem_bits=bits)


def self_oracle(x, W, b, Hn, k, elem):
    """cross_cases.self_chain on given tokens: the qkv Linear, O.qkv_split, the attention core"""
    qkv_ = O.mx_linear(x, W, b, elem=elem)
    qh, kh, vh = (np.ascontiguousarray(t) for t in O.qkv_split(qkv_, Hn))
    r = dict(O.attention(qh, kh, vh, (x.shape[-1] // Hn) ** -0.5, k_top=k, pred_mode="ex_pred", elem=elem))
    r.update(qh=qh, kh=kh, vh=vh)
    return r


def _self_block(name, shape_k, tensors, bits, proj, check=False):
    """mx_qkv_attention on a self-attention case's weights (x is the input that changes), with the proj Linear or without"""
    (Bn, N, C, Hn), k = shape_k
    x, W, b, Wo, bo = tensors()
    D = C // Hn

    def inputs(which):
        return dict(x=x if which == "A" else rnd((Bn, N, C), 4242 + N))

    def consts(M):
        c = dict(w=_weight(M, W, D, bits), b=dev(b))
        if proj:
            c.update(wo=_weight(M, Wo, C, bits), bo=dev(bo))
        return c

    def call(M, t, c):
        return M.mx_qkv_attention(t["x"], c["w"], c["b"], Hn, _scale(D), k_top=k, elem_bits=bits, proj_weight=c.get("wo"),
                                  proj_bias=c.get("bo"))

    _add(name, "block", inputs, call, ("y" if proj else "out", "idx"),
         lambda which: self_oracle(inputs(which)["x"], W, b, Hn, k, ELEM[bits]), consts, check, facts=dict(T=N))


for _bits in (8, 4):
    for _proj in (False, True):
        _self_block(f"qkv{'_proj' if _proj else ''}_w{_bits}", CC.SELF_SHAPES["d32"], lambda: CC.self_case("d32"), _bits, _proj,
                    check=(_bits == 8 and not _proj))
_self_block("qkv_proj_long", (LB.CASES["d32k32"].shape, LB.CASES["d32k32"].k), lambda: LB.case("d32k32"), 8, True)


def _attn_proj():
    """mx_topk_attention_proj on the heads of the "d32" self-attention chain"""
    (Bn, N, C, Hn), k = CC.SELF_SHAPES["d32"]
    x, W, b, Wo, bo = CC.self_case("d32")

    def chain(which):
        return self_oracle(CASES["qkv_w8"].inputs(which)["x"], W, b, Hn, k, "int8")

    def call(M, t, c):
        return M.mx_topk_attention_proj(t["q"], t["k"], t["v"], _scale(C // Hn), c["wo"], c["bo"], k_top=k)

    _add("attn_proj", "block", lambda which: dict(zip("qkv", (chain(which)[a] for a in ("qh", "kh", "vh")))), call, ("y", "idx"),
         chain, lambda M: dict(wo=_weight(M, Wo, C, 8), bo=dev(bo)))


_attn_proj()


def _cross():
    """mx_cross_attention on cross_cases "d32" (finite tokens), a (B, 1, 1, T) mask bias"""
    (Bn, N, T, C, Ckv, Hn), k = CC.SHAPES["d32"]
    x, cond, Wq, bq, Wkv, bkv, _, _ = CC.case("d32", nan_x=False)
    D = C // Hn

    def inputs(which):
        if which == "A":
            return dict(x=x, cond=cond, bias=CC.mask_bias(Bn, T))
        return dict(x=rnd((Bn, N, C), 501), cond=rnd((Bn, T, Ckv), 502),
                    bias=np.where(np.arange(T) >= T // 3, 0.0, -10000.0).astype(F32)[None, None, None, :].repeat(Bn, 0))

    def oracle(which):
        t = inputs(which)
        kh, vh = CC.heads_kv(O.mx_linear(t["cond"], Wkv, bkv), Hn)
        return O.attention(CC.heads_q(O.mx_linear(t["x"], Wq, bq), Hn), kh, vh, D ** -0.5, k_top=k, pred_mode="ex_pred",
                           bias=t["bias"])

    def call(M, t, c):
        return M.mx_cross_attention(t["x"], t["cond"], c["wq"], c["bq"], c["wkv"], c["bkv"], Hn, _scale(D), k_top=k,
                                    pred_mode="ex_pred", bias=t["bias"])

    _add("cross_bias", "block", inputs, call, ("out", "idx"), oracle,
         lambda M: dict(wq=_weight(M, Wq, D, 8), bq=dev(bq), wkv=_weight(M, Wkv, D, 8), bkv=dev(bkv)))


_cross()


# ---- mx_linear, mx_mlp, mx_matmul, quantize_mx ----------------------------------------------------
LINEAR = IC.linear_case(70, 256, 48, 24)  # x, W, b: test_gpu_int4's grouped-weight case
LINEAR_GROUPS = {"digit": 48, "tile": 24}  # one group of out_features: digits; groups of 24 columns: the tile kernel


def _linear(path, bits):
    x, W, b = LINEAR

    def inputs(which):
        return dict(x=x if which == "A" else rnd(x.shape, 991))

    _add(f"linear_{path}_w{bits}", "linear", inputs, lambda M, t, c: (M.mx_linear(t["x"], c["w"], c["b"], elem_bits=bits),), ("y",),
         lambda which: dict(y=O.mx_linear(inputs(which)["x"], W, b, elem=ELEM[bits])),
         lambda M: dict(w=_weight(M, W, LINEAR_GROUPS[path], bits), b=dev(b)), check=(path == "digit" and bits == 8),
         facts=dict(path=path, bits=bits))


for _path in LINEAR_GROUPS:
    for _bits in (8, 4):
        _linear(_path, _bits)
MLP = MC.case(70, 96, 160, 40, 7)  # x, W1, b1, W2, b2


def _mlp(act, prepared):
    """prepared: both weights as LinearWeightMX; else tensors, prepared inside the captured call"""
    x, W1, b1, W2, b2 = MLP

    def inputs(which):
        return dict(x=x if which == "A" else rnd(x.shape, 992))

    def consts(M):
        w = (lambda W: _weight(M, W, W.shape[0], 8)) if prepared else dev
        return dict(w1=w(W1), b1=dev(b1), w2=w(W2), b2=dev(b2))

    _add(f"mlp_{act}", "mlp", inputs, lambda M, t, c: M.mx_mlp(t["x"], c["w1"], c["b1"], c["w2"], c["b2"], act=act, return_hidden=True),
         ("y", "pre", "act"), lambda which: dict(pre=O.mx_linear(inputs(which)["x"], W1, b1)), consts, check=prepared)


_mlp("gelu", True)
_mlp("gelu_tanh", False)


def _matmul(name, transposed, check=False):
    def inputs(which):
        s = 0 if which == "A" else 50
        return dict(a=rnd((3, 70, 96), 1 + s), b=rnd((3, 150, 96) if transposed else (96, 150), 2 + s))

    def oracle(which):
        t = inputs(which)
        return dict(c=O.mx_matmul(t["a"], np.swapaxes(t["b"], -1, -2) if transposed else t["b"]))

    _add(name, "matmul", inputs, lambda M, t, c: (M.mx_matmul(t["a"], t["b"].transpose(-2, -1) if transposed else t["b"]),), ("c",),
         oracle, check=check)


_matmul("matmul", False, check=True)
_matmul("matmul_bt", True)
_add("quantize_mx", "quant", lambda which: dict(A=rnd((70, 100), 3 if which == "A" else 53)),
     lambda M, t, c: M.quantize_mx(t["A"], want_codes=True), ("y", "codes", "exps"),
     lambda which: dict(y=O.quantize_mx(CASES["quantize_mx"].inputs(which)["A"], "int8", 32, -1)[0]), check=True)


# ---- the standalone top-k -------------------------------------------------------------------------
def topk_rows(which):
    """70 rows of 197: topk_cases.standalone_batch (rows that pack: the packed pass and, at k = 20, the tail), rows
    10 .. 19 random floats (their low mantissa bytes are set: the 64-bit pass), row 5 with zeros of both signs;
    B: the columns reversed and other random rows"""
    rows = TC.standalone_batch(197, 20)
    rows[5, ::3] = F32(-0.0)
    rows[5, 1::3] = F32(0.0)
    if which == "B":
        rows = np.ascontiguousarray(rows[:, ::-1])
    rows[10:20] = rnd((10, 197), 7 if which == "A" else 57)
    return rows


def _topk(name, vals, k, check=False):
    _add(name, "topk", lambda which: dict(vals=vals(which)), lambda M, t, c: M.topk(t["vals"], k, return_mask=True),
         ("vals", "idx", "mask"), lambda which: dict(zip(("vals", "idx"), O.topk(vals(which), k))), check=check, facts=dict(k=k))


_topk("topk_n197", topk_rows, 20, check=True)
_topk("topk_n600", lambda which: rnd((8, 600), 8 if which == "A" else 58), 20)
_topk("topk_k0", lambda which: rnd((70, 197), 9 if which == "A" else 59), 0)  # the mask alone, cleared


# ---- the unchanged DeiT glue on the drop-in modules -----------------------------------------------
GLUE_SPECS = {"a_elem_format": "int8", "w_elem_format": "int8", "block_size": 32, "scale_bits": 8, "bfloat": 32,
              "shared_exp_method": "max", "round": "nearest"}


def _glue():
    def inputs(which):
        d = np.load(os.path.join(G, "attn_deit_tiny.npz"))
        if which == "A":
            return {a: d[a] for a in "qkv"}
        return {a: rnd(d[a].shape, 60 + i) for i, a in enumerate("qkv")}

    def oracle(which):
        d = np.load(os.path.join(G, "attn_deit_tiny.npz"))
        if which == "A":  # the reference's own result
            return dict(idx=d["ex_pred_k20/idx"], out=d["ex_pred_k20/out"])
        t = inputs(which)
        return O.attention(t["q"], t["k"], t["v"], float(d["scale"]), k_top=20, pred_mode="ex_pred")

    def consts(M):
        M.install_dropin()
        from mx.specs import apply_mx_specs
        return dict(specs=apply_mx_specs(dict(GLUE_SPECS)), scale=float(np.load(os.path.join(G, "attn_deit_tiny.npz"))["scale"]))

    def call(M, t, c):
        import glue_deit
        assert M.bind_exact_topk(glue_deit) == 1
        try:
            return glue_deit.attention_core(t["q"], t["k"], t["v"], c["scale"], 20, c["specs"], pred_mode="ex_pred")
        finally:
            M.unbind_exact_topk(glue_deit)

    _add("glue_deit", "glue", inputs, call, ("out", "idx"), oracle, consts, check=True)


_glue()
