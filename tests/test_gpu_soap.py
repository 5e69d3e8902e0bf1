"""GPU tests of the SOAP entries (csrc/eval/soap.hip) and of diffusion_model_amd.soap on top of them.

Bars (the truth is tests/golden/soap_golden.npz, mpmath at 60 digits; E = max |p - p_truth| / max |p_truth|):
  * E_host, the host statement's error, is measured per configuration (tests/_soap_util.py: e_host) and capped at 1e-7 by tests/test_soap_host.py;
  * the device against the same truth: 8 E_host -- host and device run one operation order (soap_math.h) without contraction and
    differ only in exp (a few ulp against 1) under the same amplification by beta; the device against the host statement where
    there is no truth (the default configuration beyond the three smallest graphs): the same 8 E_host;
  * cosines: |delta cos| <= 2 (eps_a + eps_b), so 4 x the descriptor bar of the same side; the cosine KERNELS against the host
    statement on the same rows: one order and IEEE operations on both sides, so 4 eps;
  * spectrum MSE bitwise, indices exactly; two identical calls bitwise.
Every input first passes the gap checks of tests/_soap_util.py.
"""
import functools
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from diffusion_model_amd import _lib, soap
from diffusion_model_amd.soap import SoapBasis
from tests import _soap_util as SU

G, _host, _tables, e_host = SU.golden(), SU.host_on_golden, SU.tables, SU.e_host

pytestmark = pytest.mark.gpu
DEV = "cuda"
EPS = float(np.finfo(float).eps)


def _onehot(types, A):
    return torch.eye(A, dtype=torch.int64)[torch.from_numpy(np.asarray(types)).long()]


def _device(name, pos, types, sizes, A, centres, coeff=False, cut=None):
    out = soap.soap_descriptors(torch.from_numpy(pos).to(DEV), _onehot(types, A).to(DEV), sizes, centres, SoapBasis(**SU.CONFIGS[name]),
                                neighbour_cut=cut, return_coefficients=coeff)
    return (out[0].cpu().numpy(), out[1].cpu().numpy()) if coeff else out.cpu().numpy()


@functools.lru_cache(maxsize=None)
def _host_all(name, A):
    """the host statement on EVERY atom of the whole fixture (computed once, never changed)"""
    pos, types, sizes = SU.fixture(A)
    assert SU.gap_ok(pos, sizes, SU.neighbour_cut(SU.CONFIGS[name]))
    rc, desc, coeff = SU.host_descriptors(_lib.lib(), pos, types, sizes, A, np.arange(len(types)), SU.CONFIGS[name], _tables(name)[1])
    assert rc == 0
    return desc, coeff


@pytest.mark.parametrize("A", SU.TYPES)
@pytest.mark.parametrize("name", list(SU.CONFIGS))
def test_descriptors_against_the_truth_and_the_host_statement(name, A):
    bar = 8 * e_host(name)
    pos, types, sizes = SU.fixture(A)
    truth, want = G[f"{name}_A{A}_desc"], _host_all(name, A)[0]
    first = _device(name, pos, types, sizes, A, "first")
    every = _device(name, pos, types, sizes, A, "all")
    cs = np.array([len(types) - 1, 7, 7, 0, 150, 7, 3, 283, 90])
    listed = _device(name, pos, types, sizes, A, torch.from_numpy(cs))
    assert first.shape == (len(sizes), SU.features(A, SU.CONFIGS[name]["n_max"], SU.CONFIGS[name]["l_max"]))
    if name == "default":                                                      # the truth: atom 0 of the three smallest graphs
        err = SU.descriptor_error(first[:3], truth)
    else:                                                                      # the truth: every atom
        err = SU.descriptor_error(every, truth)
    print(f"E_device[{name}, A={A}] = {err:.3e} against the truth, {SU.descriptor_error(every, want):.3e} against the host statement; "
          f"bar {bar:.3e}")
    assert err <= bar
    assert SU.descriptor_error(every, want) <= bar
    assert np.array_equal(first, every[SU.first_centres(sizes)]) and np.array_equal(listed, every[cs])
    # a species without an atom in the graph leaves its blocks exactly zero, a lone atom has l = 0 only
    assert np.count_nonzero(every[0]) == SU.CONFIGS[name]["n_max"] * (SU.CONFIGS[name]["n_max"] + 1) // 2
    # the cosine of every row with the next one, against the truth where it covers the rows
    if name == "small":
        got = soap.cosine(torch.from_numpy(every).to(DEV), torch.from_numpy(np.roll(every, -1, 0)).to(DEV)).cpu().numpy()
        assert float(np.abs(got - G[f"{name}_A{A}_cos"]).max()) <= 4 * max(bar, EPS)


@pytest.mark.parametrize("name", list(SU.CONFIGS))
def test_coefficients_against_the_truth_and_without_them(name):
    bar = 8 * e_host(name)
    pos, types, sizes = SU.fixture(2)
    cs = G[f"{name}_A2_centres"]
    desc, coeff = _device(name, pos, types, sizes, 2, torch.from_numpy(cs.astype(np.int64)), coeff=True)
    truth = G[f"{name}_A2_coeff"]
    assert coeff.shape == truth.shape and SU.descriptor_error(coeff, truth) <= bar
    assert SU.descriptor_error(coeff, _host_all(name, 2)[1][cs]) <= bar
    bare = _device(name, pos, types, sizes, 2, torch.from_numpy(cs.astype(np.int64)))     # NULL coefficient output
    again = _device(name, pos, types, sizes, 2, torch.from_numpy(cs.astype(np.int64)), coeff=True)
    assert np.array_equal(bare, desc) and np.array_equal(again[0], desc) and np.array_equal(again[1], coeff)   # bitwise


def test_a_large_graph_among_small_ones_and_a_callers_cut():
    rng = np.random.default_rng(21)
    sizes = [3, 600, 2]
    pos = np.concatenate([rng.uniform(0, 2.2 * np.cbrt(n), (n, 3)) for n in sizes]).astype(np.float32)
    types = rng.integers(0, 2, sum(sizes)).astype(np.int32)
    for cut in (None, 3.0):
        assert SU.gap_ok(pos, sizes, SU.neighbour_cut(SU.CONFIGS["small"]) if cut is None else cut)
        rc, want, _ = SU.host_descriptors(_lib.lib(), pos, types, sizes, 2, np.arange(len(types)), SU.CONFIGS["small"], _tables("small")[1], cut=cut)
        assert rc == 0
        got = _device("small", pos, types, sizes, 2, "all", cut=cut)
        assert SU.descriptor_error(got, want) <= 8 * e_host("small")
    assert not np.array_equal(got, _device("small", pos, types, sizes, 2, "all"))


def _rows():
    return _host("small", 3)[0]


def test_cosine_and_cosine_matrix_against_the_host_statement():
    L = _lib.lib()
    desc = _rows()
    a, b = desc[:70], desc[100:133]
    da, db = torch.from_numpy(a).to(DEV), torch.from_numpy(b).to(DEV)
    pairs = [[0, 0], [69, 32], [5, 7], [5, 7]]
    rc, want, gram = SU.host_cosines(L, a, b, pairs=pairs, gram=True)
    assert rc == 0
    got = soap.cosine(da, db, torch.tensor(pairs)).cpu().numpy()
    M = soap.cosine_matrix(da, db)
    assert M.shape == (70, 33) and float(np.abs(got - want).max()) <= 4 * EPS and float(np.abs(M.cpu().numpy() - gram).max()) <= 4 * EPS
    assert np.array_equal(got, M.cpu().numpy()[[0, 69, 5, 5], [0, 32, 7, 7]])               # one order in both kernels: bitwise
    assert np.array_equal(soap.cosine_matrix(da, db).cpu().numpy(), M.cpu().numpy())
    diag = soap.cosine(da[:33], db).cpu().numpy()                                            # no pair list: row p with row p
    assert np.array_equal(diag, np.diag(M.cpu().numpy()[:33]))
    one = soap.cosine_matrix(da[:1], da[:1]).cpu().numpy()
    assert one.shape == (1, 1) and abs(one[0, 0] - 1.0) <= 4 * EPS
    wide = soap.cosine_matrix(db, da).cpu().numpy()                                          # 33 x 70: the other tile edges
    assert float(np.abs(wide - gram.T).max()) <= 4 * EPS
    full = _host("default", 2)[0]                                                            # F = 5,115: many steps of 64, and a tail
    rc, want, _ = SU.host_cosines(L, full, full[::-1].copy(), n_pairs=3)
    got = soap.cosine(torch.from_numpy(full).to(DEV), torch.from_numpy(full[::-1].copy()).to(DEV)).cpu().numpy()
    assert rc == 0 and float(np.abs(got - want).max()) <= 4 * EPS


@pytest.mark.parametrize("S", [200, 7])
def test_nearest_spectra_against_the_host_statement(S):
    L = _lib.lib()
    t, r = SU.spectra(40 + S, 5, 70, S)
    dt, dr = torch.from_numpy(t).to(DEV), torch.from_numpy(r).to(DEV)
    tid, rid = ["a", "b", None, ("c", 1), 70], [("a", "b", ("c", 1))[q % 3] for q in range(70)]
    tg, rg = np.array([0, 1, 2, 3, 4], np.int32), np.array([(0, 1, 3)[q % 3] for q in range(70)], np.int32)
    for ids, groups in (((None, None), (None, None)), ((tid, rid), (tg, rg))):
        for k in (1, 3, 8):
            idx, mse, m = SU.nearest(t, r, k, *groups)
            assert SU.mse_gap_ok(m)
            rc, hi, hm = SU.host_nearest(L, t, r, k, *groups)
            gi, gm = soap.nearest_spectra(dt, dr, k, *ids)
            assert rc == 0 and gi.dtype == torch.int64 and gm.dtype == torch.float64
            assert np.array_equal(gi.cpu().numpy(), hi) and np.array_equal(gi.cpu().numpy(), idx)           # exactly
            assert np.array_equal(gm.cpu().numpy(), hm) and np.array_equal(gm.cpu().numpy(), mse)           # bitwise
    gi, gm = soap.nearest_spectra(dt[:1], dr[:3], 8)
    assert sorted(gi[0, :3].tolist()) == [0, 1, 2] and gi[0, 3:].tolist() == [-1] * 5 and torch.isinf(gm[0, 3:]).all()
    gi, gm = soap.nearest_spectra(dt, dr, 3, ["x"] * 5, ["x"] * 70)
    assert (gi == -1).all() and torch.isinf(gm).all()


def _records(A, n_graphs, seed, S=200, jitter=0.0, ids=None):
    """the fixture graphs as records (pos, x, id, spectrum [1, S]) on the host, as a data set holds them"""
    pos, types, sizes = SU.fixture(A, n_graphs)
    rng = np.random.default_rng(seed)
    pos = (pos + jitter * rng.standard_normal(pos.shape)).astype(np.float32)
    spec = SU.spectra(seed, len(sizes), 1, S)[0]
    recs, lo = [], 0
    for g, n in enumerate(sizes):
        recs.append(SimpleNamespace(pos=torch.from_numpy(pos[lo:lo + n]), x=_onehot(types[lo:lo + n], A), id=ids[g] if ids else f"s{seed}-{g}",
                                    spectrum=torch.from_numpy(spec[g:g + 1])))
        lo += n
    return recs


def _restate_first(name, recs, A):
    pos = np.concatenate([r.pos.numpy() for r in recs])
    types = np.concatenate([r.x.argmax(1).numpy() for r in recs])
    sizes = [len(r.pos) for r in recs]
    assert SU.gap_ok(pos, sizes, SU.neighbour_cut(SU.CONFIGS[name]))
    return SU.descriptors(pos, types, sizes, A, SU.first_centres(sizes), _tables(name)[0], SU.neighbour_cut(SU.CONFIGS[name]))[0]


@pytest.mark.parametrize("name", list(SU.CONFIGS))
def test_template_matching_end_to_end(name):
    n_graphs = 5 if name == "default" else 7
    targets = _records(2, n_graphs, 1, jitter=0.05)
    references = _records(2, n_graphs, 2, ids=["r0", "s1-3", "r2", "r3", "s1-2", "r5", "r6"])   # two share a target's id
    result, idx, mse, sim = soap.template_matching(targets, references, k=3, basis=SoapBasis(**SU.CONFIGS[name]), device=DEV)
    tk, rk = targets[1:], references[1:]                                       # the one-atom records are dropped
    spec = lambda recs: np.stack([r.spectrum[0].numpy() for r in recs])
    table: dict = {}
    code = lambda recs: np.array([table.setdefault(r.id, len(table)) for r in recs])
    tg, rg = code(tk), code(rk)
    widx, wmse, m = SU.nearest(spec(tk), spec(rk), 3, tg, rg)
    assert SU.mse_gap_ok(m)
    assert np.array_equal(idx.numpy(), widx) and np.array_equal(mse.numpy(), wmse)
    dt, dr = _restate_first(name, tk, 2), _restate_first(name, rk, 2)
    want = SU.cosine(np.repeat(dt, 3, 0), dr[widx.reshape(-1)]).reshape(-1, 3)
    bar = 4 * (8 * e_host(name) + 8 * e_host(name))                            # device and restatement, each within 8 E_host of the truth
    assert float(np.abs(sim.numpy() - want).max()) <= max(bar, 4 * EPS)
    assert list(result) == [r.id for r in tk]
    for t, rec in enumerate(tk):
        entry = result[rec.id]
        assert [list(e)[0] for e in entry] == [rk[j].id for j in widx[t]] and rec.id not in [list(e)[0] for e in entry]
        assert [list(e.values())[0] for e in entry] == [[float(mse[t, q]), float(sim[t, q])] for q in range(3)]


def test_soap_similarity_end_to_end():
    originals = _records(2, 5, 1)
    samples = _records(2, 5, 1, jitter=0.03)
    generated = [[None, SimpleNamespace(pos=s.pos.to(DEV), x=s.x.to(DEV))] for s in samples]
    basis = SoapBasis(**SU.CONFIGS["small"])
    sims, skipped = soap.soap_similarity(originals, generated, basis=basis)
    assert skipped == [0] and len(sims) == 4
    want = SU.cosine(_restate_first("small", originals[1:], 2), _restate_first("small", samples[1:], 2))
    assert float(np.abs(np.array(sims) - want).max()) <= max(64 * e_host("small"), 4 * EPS)
    assert all(0.0 < s < 1.0 for s in sims)
    same, _ = soap.soap_similarity(originals, [[SimpleNamespace(pos=o.pos.to(DEV), x=o.x.to(DEV))] for o in originals], basis=basis)
    assert float(np.abs(np.array(same) - 1.0).max()) <= 4 * EPS
    assert soap.soap_similarity([], []) == ([], [])


def test_python_layer_errors():
    pos, types, sizes = SU.fixture(2, 4)
    p, x = torch.from_numpy(pos), _onehot(types, 2)
    basis = SoapBasis(**SU.CONFIGS["small"])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        soap.soap_descriptors(p, x, sizes, basis=basis)
    for call in (lambda: soap.cosine(torch.ones(2, 3), torch.ones(2, 3)), lambda: soap.cosine_matrix(torch.ones(2, 3), torch.ones(2, 3)),
                 lambda: soap.nearest_spectra(torch.ones(2, 3), torch.ones(2, 3)), lambda: soap.template_matching(_records(2, 3, 1), _records(2, 3, 2), device="cpu")):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            call()
    p, x = p.to(DEV), x.to(DEV)
    for call in (lambda: soap.soap_descriptors(p, x, sizes, centres=torch.tensor([25]), basis=basis), lambda: soap.soap_descriptors(p, x, sizes, centres=torch.tensor([-1]), basis=basis),
                 lambda: soap.soap_descriptors(p, x, sizes, centres="last", basis=basis), lambda: soap.soap_descriptors(p, x, [1, 2, 5], basis=basis),
                 lambda: soap.soap_descriptors(p, x * 2, sizes, basis=basis), lambda: soap.soap_descriptors(p, torch.eye(5, dtype=torch.int64, device=DEV)[torch.zeros(25, dtype=torch.long, device=DEV)], sizes, basis=basis),
                 lambda: soap.soap_descriptors(p, x, sizes, basis=basis, neighbour_cut=0.0), lambda: soap.soap_descriptors(p, x, sizes, basis=basis, neighbour_cut=float("inf")),
                 lambda: soap.cosine(torch.ones(2, 3, device=DEV), torch.ones(3, 3, device=DEV)), lambda: soap.cosine(torch.ones(2, 3, device=DEV), torch.ones(2, 3, device=DEV), [[0, 2]]),
                 lambda: soap.cosine_matrix(torch.ones(2, 3, device=DEV), torch.ones(2, 4, device=DEV)), lambda: soap.nearest_spectra(torch.ones(2, 3, device=DEV), torch.ones(2, 3, device=DEV), k=9),
                 lambda: soap.nearest_spectra(torch.ones(2, 3, device=DEV), torch.ones(2, 3, device=DEV), k=0), lambda: soap.nearest_spectra(torch.ones(2, 3, device=DEV), torch.ones(2, 4, device=DEV)),
                 lambda: soap.nearest_spectra(torch.ones(2, 3, device=DEV), torch.ones(2, 3, device=DEV), 1, ["a", "b"], None), lambda: SoapBasis(8.0, 17, 10, 0.1),
                 lambda: SoapBasis(8.0, 15, 11, 0.1), lambda: SoapBasis(8.0, 15, 10, 0.0)):
        with pytest.raises(ValueError):
            call()
