"""The training backward's decision record (diffusion_model_amd/autograd.py: _switches, decide_keep, plan_backward,
BackwardPlan) as a table: inputs against the path the backward took before the record existed.  No GPU, no library: the
library's answer (egcl_backward_fused_supported) and the free HBM come in as values."""
import dataclasses
import inspect

import pytest

from diffusion_model_amd import _lib, autograd as ag

BF16, F32 = _lib.PREC_BF16, _lib.PREC_F32
SIZES = (33, 64, 1, 17, 50)                                   # the ragged fully connected batch of tests/test_training.py
REF, NARROW, W256 = (1024, 1024, 256, 1024), (22, 30, 10, 18), (256, 256, 256, 256)       # (Wx, Wm, M, Wh)
GiB = 1 << 30


def _gep(sizes):
    out = [0]
    for n in sizes:
        out.append(out[-1] + n * (n - 1))
    return out


def _library_supports(Wx, Wm, M):
    """backward_recompute_supported (csrc/egnn_forward.hip) for these widths"""
    return Wx in (256, 512, 1024) and M == 256 and Wm % 64 == 0 and Wm >= 192


def _run(prec, env=None, H=36, widths=REF, chunk=4300, sizes=SIZES, spent=False, free=64 * GiB, L=2, max_nodes=None):
    """decide_keep + plan_backward composed as _EGNNFunction.forward / backward compose them"""
    Wx, Wm, M, Wh = widths
    sw, gep, p = ag._switches(env or {}), _gep(sizes), _lib.PRECISIONS[prec]
    E = gep[-1]
    keep = ag.decide_keep(p, E, L, Wx, Wm, M, sw, _library_supports(Wx, Wm, M), free)
    kept = keep and not spent
    supported = ag.fused_asked(p, E, kept, sw) and _library_supports(Wx, Wm, M)     # (asked only when the switches want it)
    bp = ag.plan_backward(p, H, Wx, Wm, M, Wh, E, chunk, gep, max(sizes) if max_nodes is None else max_nodes, kept, supported, sw)
    return keep, bp


PLAIN = ((0, 4352), (4352, 3458))                              # EDGE_CHUNK 4300 -> 4352 rows; E = 7810
WHOLE = ((0, 1056), (1056, 4304), (5360, 2450))                # cut at graph boundaries: 33 | 64, 1, 17 | 50 atoms
#                 prec split  fused  hip    kept   first     chunks K1P  node
BF16_DEFAULT = (BF16, False, True, True, True, "graph", WHOLE, 128, "hip")
FP32_CHAIN = (F32, False, False, False, False, None, PLAIN, 80, "torch")
CASES = {
    # the seven configurations of test_no_backward_reads_uninitialised_memory
    "bf16-graph": (("bf16", {}), {}, BF16_DEFAULT),
    "bf16-chain": (("bf16", {"EGNN_BWD_GRAPH": "0"}), {}, (BF16, False, True, True, True, None, PLAIN, 128, "hip")),
    "bf16-recompute": (("bf16", {"EGNN_BWD_SAVE": "0"}), {}, (BF16, False, True, True, False, "graph", WHOLE, 128, "hip")),
    "bf16-reduce": (("bf16", {"EGNN_BWD_FIRST": "1"}), {}, (BF16, False, True, True, True, "reduce", PLAIN, 128, "hip")),
    "fp16": (("fp16", {}), {}, (BF16, False, True, True, False, "graph", WHOLE, 128, "hip")),     # bf16 backward, nothing kept
    "fp32": (("fp32", {}), {}, FP32_CHAIN),
    "bf16x3": (("bf16x3", {}), {}, (F32, True, False, False, False, None, PLAIN, 80, "split")),
    # precedence
    "FIRST=1 wins over GRAPH=1": (("bf16", {"EGNN_BWD_FIRST": "1", "EGNN_BWD_GRAPH": "1"}), {},
                                  (BF16, False, True, True, True, "reduce", PLAIN, 128, "hip")),
    "FIRST=1, GRAPH=0": (("bf16", {"EGNN_BWD_FIRST": "1", "EGNN_BWD_GRAPH": "0"}), {},
                         (BF16, False, True, True, True, "reduce", PLAIN, 128, "hip")),
    "graph form needs <= 64-node graphs": (("bf16", {}), dict(max_nodes=65), (BF16, False, True, True, True, None, PLAIN, 128, "hip")),
    "reduce form needs <= 64-node graphs": (("bf16", {"EGNN_BWD_FIRST": "1"}), dict(max_nodes=65),
                                            (BF16, False, True, True, True, None, PLAIN, 128, "hip")),
    "first forms need the own GEMMs (H = 64)": (("bf16", {"EGNN_BWD_FIRST": "1"}), dict(H=64, widths=W256),
                                                (BF16, False, True, False, True, None, PLAIN, 136, "torch")),
    # the 64-atom graph has 4032 edges: a 3000-edge chunk (3008 rows) cannot hold it -> the chain, cut anywhere
    "a graph larger than the chunk": (("bf16", {}), dict(chunk=3000),
                                      (BF16, False, True, True, True, None, ((0, 3008), (3008, 3008), (6016, 1794)), 128, "hip")),
    "a chunk of exactly one graph": (("bf16", {}), dict(chunk=4032),
                                     (BF16, False, True, True, True, "graph", ((0, 1056), (1056, 4032), (5088, 2722)), 128, "hip")),
    "EDGE < 4: nothing kept, fused recompute": (("bf16", {"EGNN_EDGE": "3"}), {}, (BF16, False, True, True, False, "graph", WHOLE, 128, "hip")),
    "spent kept buffers: recompute": (("bf16", {}), dict(spent=True), (BF16, False, True, True, False, "graph", WHOLE, 128, "hip")),
    "too little HBM: recompute": (("bf16", {}), dict(free=1 << 20), (BF16, False, True, True, False, "graph", WHOLE, 128, "hip")),
    "FUSED=0": (("bf16", {"EGNN_BWD_FUSED": "0"}), {}, (BF16, False, False, False, False, None, PLAIN, 80, "torch")),
    "FUSED=0, fp16": (("fp16", {"EGNN_BWD_FUSED": "0"}), {}, (BF16, False, False, False, False, None, PLAIN, 80, "torch")),
    "fp32, OWN=1": (("fp32", {"EGNN_BWD_OWN": "1"}), {}, (F32, True, False, False, False, None, PLAIN, 80, "split")),
    "BLAS=1 beats OWN=1": (("fp32", {"EGNN_BWD_OWN": "1", "EGNN_BWD_BLAS": "1"}), {}, FP32_CHAIN),
    "BLAS=1 beats the tolerance-grade default": (("bf16x3", {"EGNN_BWD_BLAS": "1"}), {}, FP32_CHAIN),
    "f16c8": (("f16c8", {}), {}, (F32, True, False, False, False, None, PLAIN, 80, "split")),
    "f16c8, BLAS=1": (("f16c8", {"EGNN_BWD_BLAS": "1"}), {}, FP32_CHAIN),
    "node form hip needs Wh % 256 == 0": (("bf16", {}), dict(widths=(1024, 1024, 256, 1000)),
                                          (BF16, False, True, True, True, "graph", WHOLE, 128, "torch")),
    # the saved h is always fp32, so the own fp32 products take the node MLP of a bf16 backward too when it is not on the own
    # bf16 GEMMs (the edge chain's bf16 buffers stay on the BLAS library: _mm / _wgrad look at the operand type)
    "bf16, OWN=1, Wh % 256 != 0": (("bf16", {"EGNN_BWD_OWN": "1"}), dict(widths=(1024, 1024, 256, 1000)),
                                   (BF16, True, True, True, True, "graph", WHOLE, 128, "split")),
    # widths
    "narrow fp32": (("fp32", {}), dict(widths=NARROW), FP32_CHAIN),
    "narrow bf16": (("bf16", {}), dict(widths=NARROW), (BF16, False, False, False, False, None, PLAIN, 80, "torch")),
    "narrow bf16, OWN=1": (("bf16", {"EGNN_BWD_OWN": "1"}), dict(widths=NARROW), (BF16, True, False, False, False, None, PLAIN, 80, "split")),
    "H = 63 at fused-supported widths": (("bf16", {}), dict(H=63, widths=W256), (BF16, False, True, True, True, "graph", WHOLE, 128, "hip")),
    "H = 64 at fused-supported widths": (("bf16", {}), dict(H=64, widths=W256), (BF16, False, True, False, True, None, PLAIN, 136, "torch")),
    "H = 64, SAVE=0": (("bf16", {"EGNN_BWD_SAVE": "0"}), dict(H=64, widths=W256), (BF16, False, True, False, False, None, PLAIN, 136, "torch")),
    "H = 60: 128 columns without the own GEMMs": (("fp32", {}), dict(H=60), (F32, False, False, False, False, None, PLAIN, 128, "torch")),
    "no edges": (("bf16", {}), dict(sizes=(1, 1)), (BF16, False, False, False, False, None, (), 80, "torch")),
}


@pytest.mark.parametrize("name", list(CASES))
def test_plan_table(name):
    (prec, env), kw, want = CASES[name]
    keep, bp = _run(prec, env, **kw)
    got = (bp.prec, bp.split_products, bp.fused, bp.hip_gemms, bp.kept, bp.first, bp.chunks, bp.K1P, bp.node)
    assert got == want, name
    assert keep == (bp.kept or kw.get("spent", False))
    assert bp.rows == (0 if not bp.chunks else -(-min(kw.get("chunk", 4300), _gep(kw.get("sizes", SIZES))[-1]) // 64) * 64)
    assert sum(n for _, n in bp.chunks) == _gep(kw.get("sizes", SIZES))[-1] and all(n <= bp.rows for _, n in bp.chunks)
    assert str(bp.dtype) == {BF16: "torch.bfloat16", F32: "torch.float32"}[bp.prec]


def test_decide_keep_rule():
    sw = ag._switches({})
    E, L, Wx, Wm, M = 7810, 2, 1024, 1024, 256
    need = L * 7872 * (2 * Wx + Wm + M) * 2                                            # 7872 = E padded to 64 rows
    keep = lambda prec="bf16", env=None, E=E, supported=True, free=64 * GiB, Wx=Wx: ag.decide_keep(
        _lib.PRECISIONS[prec], E, L, Wx, Wm, M, sw if env is None else ag._switches(env), supported, free)
    assert keep() is True
    assert keep(free=2 * need + 2) is True and keep(free=2 * need) is False            # need < 0.5 * free, strictly
    assert keep(E=(1 << 21) - 1, free=1 << 60) is True and keep(E=1 << 21, free=1 << 60) is False   # E x Wx x 2 B < 4 GiB
    assert keep(E=1 << 22, Wx=512, free=1 << 60) is False and keep(E=(1 << 22) - 1, Wx=512, free=1 << 60) is True
    assert keep(supported=False) is False and keep(E=0) is False
    for prec in ("fp16", "fp32", "bf16x3", "f16c8"):
        assert keep(prec) is False
    for env in ({"EGNN_BWD_SAVE": "0"}, {"EGNN_BWD_FUSED": "0"}, {"EGNN_EDGE": "3"}, {"EGNN_EDGE": "0"}):
        assert keep(env=env) is False, env
    assert keep(env={"EGNN_EDGE": "5", "EGNN_BWD_SAVE": "1", "EGNN_BWD_GRAPH": "0", "EGNN_BWD_FIRST": "1"}) is True


def test_fused_is_asked_of_the_library_only_when_the_switches_want_it():
    on, off = ag._switches({}), ag._switches({"EGNN_BWD_FUSED": "0"})
    P = _lib.PRECISIONS
    assert ag.fused_asked(P["bf16"], 10, False, on) and ag.fused_asked(P["fp16"], 10, False, on)
    assert not ag.fused_asked(P["bf16"], 10, False, off) and not ag.fused_asked(P["bf16"], 0, False, on)
    for prec in ("fp32", "bf16x3", "f16c8"):
        assert not ag.fused_asked(P[prec], 10, False, on)
    assert ag.fused_asked(P["bf16"], 10, True, on)
    # asked, and the library says no: the generic chain
    bp = ag.plan_backward(P["bf16"], 36, 1024, 1024, 256, 1024, 7810, 4300, _gep(SIZES), 64, False, False, on)
    assert (bp.fused, bp.hip_gemms, bp.first, bp.node, bp.K1P) == (False, False, None, "torch", 80)


def test_switches_are_read_in_one_place(monkeypatch):
    assert ag._switches({}) == {"SAVE": True, "FUSED": True, "EDGE": 4, "FIRST": False, "GRAPH": True, "BLAS": False, "OWN": False,
                                "CHUNK": 1 << 20, "POISON_KEPT": False}
    for k, v in {"EGNN_BWD_SAVE": "0", "EGNN_BWD_FUSED": "0", "EGNN_EDGE": "2", "EGNN_BWD_FIRST": "1", "EGNN_BWD_GRAPH": "0",
                 "EGNN_BWD_BLAS": "1", "EGNN_BWD_OWN": "1", "EGNN_BWD_CHUNK": "4096", "EGNN_DEBUG_POISON_KEPT": "1"}.items():
        monkeypatch.setenv(k, v)
    assert ag._switches() == {"SAVE": False, "FUSED": False, "EDGE": 2, "FIRST": True, "GRAPH": False, "BLAS": True, "OWN": True,
                              "CHUNK": 4096, "POISON_KEPT": True}
    # only "1" switches an opt-in on, only "0" switches a default off (as before the record)
    assert ag._switches({"EGNN_BWD_FIRST": "true", "EGNN_BWD_GRAPH": "no", "EGNN_BWD_SAVE": ""}) == ag._switches({})
    src = inspect.getsource(ag)
    assert src.count("os.environ") == 1 and "getenv" not in src
    assert "os.environ" in inspect.getsource(ag._switches)


GOOD = dict(prec=BF16, split_products=False, fused=True, hip_gemms=True, kept=True, first="graph", rows=64,
            chunks=((0, 40), (40, 60)), K1P=128, node="hip", graph_edge_ptr=[0, 40, 40, 100])


@pytest.mark.parametrize("change,why", [
    (dict(first="reduce", hip_gemms=False, node="torch"), "first without hip_gemms"),
    (dict(first="graph", hip_gemms=False, node="torch"), "first without hip_gemms"),
    (dict(fused=False, kept=False), "hip_gemms without fused"),
    (dict(fused=False, hip_gemms=False, first=None, node="torch"), "kept without fused"),
    (dict(chunks=((0, 50), (50, 50))), "not cut at graph boundaries"),
    (dict(graph_edge_ptr=None), "not cut at graph boundaries"),
    (dict(prec=F32), "bf16 kernels"),
    (dict(hip_gemms=False, first=None), "node form 'hip' without hip_gemms"),
    (dict(node="split"), "node form 'split' without split_products"),
])
def test_invalid_combinations_are_rejected(change, why):
    ag.BackwardPlan(**GOOD)
    with pytest.raises(ValueError, match=why):
        ag.BackwardPlan(**{**GOOD, **change})


def test_plan_is_a_frozen_record():
    bp = ag.BackwardPlan(**GOOD)
    with pytest.raises(dataclasses.FrozenInstanceError):
        bp.first = None
    assert [f.name for f in dataclasses.fields(bp)] == ["prec", "split_products", "fused", "hip_gemms", "kept", "first", "rows",
                                                        "chunks", "K1P", "node"]
    # fused kernels without the library's own GEMMs (H >= 64) and the "reduce" form with arbitrary cuts are valid records
    ag.BackwardPlan(**{**GOOD, "hip_gemms": False, "first": None, "node": "torch", "K1P": 136, "chunks": ((0, 64), (64, 36))})
    ag.BackwardPlan(**{**GOOD, "first": "reduce", "chunks": ((0, 64), (64, 36))})
