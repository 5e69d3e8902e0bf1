"""GPU tests of the SOAP entries (csrc/eval/soap.hip) and of diffusion_model_amd.soap on top of them.

Bars (the truth is tests/golden/soap_golden.npz, mpmath at 60 digits; E = max |p - p_truth| / max |p_truth|):
  * E_host, the host statement's error, is measured per configuration (tests/_soap_util.py: e_host) and capped at 1e-7 by tests/test_soap_host.py;
  * the device against the same truth: 8 E_host -- host and device run one operation order (soap_math.h) without contraction and
    differ only in exp (a few ulp against 1) under the same amplification by beta; the device against the host statement where
    there is no truth (the default configuration beyond the three smallest graphs): the same 8 E_host;
  * cosines: |delta cos| <= 2 (eps_a + eps_b), so 4 x the descriptor bar of the same side; the cosine KERNELS against the host
    statement on the same rows: one order and IEEE operations on both sides, so 4 eps;
  * spectrum MSE bitwise, indices exactly; two identical calls bitwise;
  * the basis limits and the degenerate bases (tests/golden/soap_limits_golden.npz): 8 max(E_host, 2^-52); the rows of a cloud
    bitwise the same wherever the chunks of 32 staged atoms fall; exact ties of the nearest spectra to the lower index.
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


# ---- the basis limits, the degenerate bases, the chunk phases and the exact ties ------------------------------------------------------
# Bars: 8 max(E_host, 2^-52) of the configuration (E_host measured against tests/golden/soap_limits_golden.npz; the floor because
# E_host of a one-function basis can be exactly 0 while a device exp may still differ by an ulp); cosine kernels 4 eps; everything
# called bitwise below is compared through the int64 view.
def _same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.int64 if a.dtype.itemsize == 8 else np.int32),
                                                                     b.view(np.int64 if b.dtype.itemsize == 8 else np.int32))


def _any_config(name):
    """-> (n_max, l_max, the neighbour cut, the golden's flat tables, E_host) of an entry of CONFIGS or LIMIT_CONFIGS"""
    if name in SU.CONFIGS:
        cfg, flat, E = SU.CONFIGS[name], _tables(name)[1], e_host(name)
    else:
        cfg, flat, E = SU.LIMIT_CONFIGS[name], SU.limit_tables(name)[1], SU.e_host_limit(name)
    return cfg, flat, max(E, 2.0 ** -52)


def _lds_bytes(A, n_max, l_max, chunk=32):
    """the dynamic-LDS request of the descriptor launch, restated from the layout in soap.hip: doubles for the coefficients
    [A][n_max][LM], the harmonics [chunk][LM], the radial values [chunk][n_max (l_max+1)] and dx, dy, dz, d2 [chunk][4], then the
    species of the chunk's atoms as int [chunk]"""
    LM = (l_max + 1) ** 2
    return 8 * (A * n_max * LM + chunk * (LM + n_max * (l_max + 1) + 4)) + 4 * chunk


def _direct(name, pos, types, gp, centres, A, coeff=False):
    """egnn_soap_descriptor itself on device tensors (the Python layer refuses types outside [0, A) and empty graphs; the kernel
    promises rows for them) -> (desc, coeff | None)"""
    cfg, flat, _ = _any_config(name)
    n_max, l_max = cfg["n_max"], cfg["l_max"]
    cs, gp = np.ascontiguousarray(centres, dtype=np.int32), np.ascontiguousarray(gp, dtype=np.int32)
    N, F = len(types), SU.features(A, n_max, l_max)
    assert gp[0] == 0 and gp[-1] == N and np.all(np.diff(gp) >= 0) and cs.min() >= 0 and cs.max() < N and len(pos) == N
    up = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a, dtype=dt)).to(DEV)
    d_pos, d_type, d_gp, d_tab, d_cs = up(pos, np.float32), up(types, np.int32), up(gp, np.int32), up(flat, np.float64), up(cs, np.int32)
    desc = torch.full((len(cs), F), -7.0, dtype=torch.float64, device=DEV)
    co = torch.full((len(cs), A, n_max, (l_max + 1) ** 2), -7.0, dtype=torch.float64, device=DEV) if coeff else None
    rc = _lib.lib().egnn_soap_descriptor(_lib.stream_ptr(), len(gp) - 1, N, A, _lib.ptr(d_pos), _lib.ptr(d_type), _lib.ptr(d_gp), n_max, l_max,
                                         float(SU.neighbour_cut(cfg)), _lib.ptr(d_tab), len(cs), _lib.host_ptr(cs), _lib.ptr(d_cs), _lib.ptr(desc),
                                         _lib.ptr(co))
    assert rc == 0, _lib.lib().egnn_last_error()
    torch.cuda.synchronize()
    return desc.cpu().numpy(), None if co is None else co.cpu().numpy()


def _host_rows(name, pos, types, sizes, A, centres=None):
    cfg, flat, _ = _any_config(name)
    assert SU.gap_ok(pos, sizes, SU.neighbour_cut(cfg)), "ambiguous input: a distance on the neighbour cut"
    rc, desc, coeff = SU.host_descriptors(_lib.lib(), pos, types, sizes, A, np.arange(len(types)) if centres is None else centres, cfg, flat)
    assert rc == 0, _lib.lib().egnn_last_error()
    return desc, coeff


@pytest.mark.parametrize("name", list(SU.LIMIT_CONFIGS))
def test_descriptors_at_the_basis_limits_and_the_degenerate_bases(name):
    cfg, flat, E = _any_config(name)
    bar, A, n_max, l_max = 8 * E, cfg["A"], cfg["n_max"], cfg["l_max"]
    LG = SU.limits_golden()
    pos, types, sizes = SU.limit_fixture(name)                                  # asserts the gap condition
    want, want_coeff = SU.host_on_limit(name)
    truth, cs = LG[f"{name}_desc"], LG[f"{name}_centres"]
    basis = SoapBasis(**SU.basis_of(cfg))
    run = lambda centres, coeff=False: soap.soap_descriptors(torch.from_numpy(pos).to(DEV), _onehot(types, A).to(DEV), sizes, centres, basis,
                                                             return_coefficients=coeff)
    every, coeff = (x.cpu().numpy() for x in run("all", True))
    first = run("first").cpu().numpy()
    shuffled = np.random.default_rng(5).permutation(np.concatenate([np.arange(len(types)), [0, len(types) - 1, 3 % len(types)]]))
    listed = run(torch.from_numpy(shuffled)).cpu().numpy()
    err, err_host = SU.descriptor_error(every[cs], truth), SU.descriptor_error(every, want)
    print(f"E_device[{name}, A={A}] = {err:.3e} against the truth, {err_host:.3e} against the host statement; bar {bar:.3e}; "
          f"LDS {_lds_bytes(A, n_max, l_max)} B")
    assert every.shape == (len(types), SU.features(A, n_max, l_max))
    assert err <= bar and err_host <= bar
    assert SU.descriptor_error(coeff, want_coeff) <= bar
    assert _same(first, every[cs]) and _same(listed, every[shuffled])
    assert np.count_nonzero(every[0]) == n_max * (n_max + 1) // 2
    assert set(types[cs[3]:cs[3] + 17].tolist()) == set(range(A)), "the 17-atom graph holds every species"
    if name == "limit":
        # the largest launch the entry can make, from the layout in soap.hip; nothing else reaches it
        assert _lds_bytes(4, 16, 10) == 8 * (4 * 16 * 121 + 32 * (121 + 176 + 4)) + 4 * 32 == 139136 <= 160 * 1024
        assert all(_lds_bytes(c.get("A", 3), c["n_max"], c["l_max"]) < 139136 for k, c in {**SU.CONFIGS, **SU.LIMIT_CONFIGS}.items() if k != "limit")
        assert SU.descriptor_error(coeff[cs], LG["limit_coeff"]) <= bar
        # every cross-species block of the feature order at A = 4 is alive in the 17-atom graph's row
        z1, z2, _, _, _ = SU.feature_index(A, n_max, l_max)
        assert all(np.any(every[cs[3]][(z1 == a) & (z2 == b)] != 0.0) for a in range(4) for b in range(a, 4))
        bare = run("all").cpu().numpy()                                         # NULL coefficient pointer
        again = [x.cpu().numpy() for x in run("all", True)]
        assert _same(bare, every) and _same(again[0], every) and _same(again[1], coeff)


def _cloud(seed, n, A):
    """n atoms inside a cube of edge 2.4 (diagonal 4.16: every pair inside the cut of every configuration), every species present"""
    rng = np.random.default_rng(seed)
    types = np.concatenate([np.arange(A), rng.integers(0, A, n - A)]).astype(np.int32)
    return rng.uniform(0.0, 2.4, (n, 3)).astype(np.float32), rng.permutation(types)


def _far(k, A):
    """k atoms on a line beyond the cut of every atom of a _cloud and 10 apart from each other"""
    pos = np.zeros((k, 3), np.float32)
    pos[:, 0] = 20.0 + 10.0 * np.arange(k)
    return pos, (np.arange(k) % A).astype(np.int32)


def _chunk_phase(name, A, n_cloud, ks, sandwich):
    """graphs far_k + G for every k, G alone, the lone atoms, and (sandwich) live chunks around a chunk with no neighbour"""
    cfg, _, _ = _any_config(name)
    cut = SU.neighbour_cut(cfg)
    (gp_, gt), (hp, ht) = _cloud(31, n_cloud, A), _cloud(32, n_cloud, A)
    lone_p, lone_t = np.zeros((A, 3), np.float32), np.arange(A, dtype=np.int32)
    graphs = [(gp_, gt)] + [(np.concatenate([_far(k, A)[0], gp_]), np.concatenate([_far(k, A)[1], gt])) for k in ks]
    graphs += [(lone_p[z:z + 1], lone_t[z:z + 1]) for z in range(A)]
    if sandwich:
        fp, ft = _far(32, A)
        graphs += [(np.concatenate([gp_, hp]), np.concatenate([gt, ht])),                       # G + G'
                   (np.concatenate([gp_, fp, hp]), np.concatenate([gt, ft, ht])),               # G + far_32 + G'
                   (np.concatenate([gp_[:32], hp]), np.concatenate([gt[:32], ht])),             # G[:32] + G'
                   (np.concatenate([gp_[:32], fp, hp]), np.concatenate([gt[:32], ft, ht]))]     # G[:32] | far_32: a whole dead chunk | G'
    sizes = [len(t) for _, t in graphs]
    pos, types = np.concatenate([p for p, _ in graphs]), np.concatenate([t for _, t in graphs])
    assert SU.gap_ok(pos, sizes, cut)
    for p, _ in graphs[1:1 + len(ks)]:                                          # far atoms see nobody, the cloud sees all of itself
        k = len(p) - n_cloud
        d = np.linalg.norm(p[:, None, :].astype(np.float64) - p[None, :, :], axis=2)
        assert np.all(d[k:, k:] < cut) and np.all(d[:k, :][~np.eye(len(p), dtype=bool)[:k, :]] > cut)
    desc, coeff = (x.cpu().numpy() for x in soap.soap_descriptors(torch.from_numpy(pos).to(DEV), _onehot(types, A).to(DEV), sizes, "all",
                                                                  SoapBasis(**SU.basis_of(cfg)), return_coefficients=True))
    lo = SU.graph_ptr(sizes)
    rows = lambda g, a, b: (desc[lo[g] + a:lo[g] + b], coeff[lo[g] + a:lo[g] + b])
    both = lambda x, y: _same(x[0], y[0]) and _same(x[1], y[1])
    alone, lone0 = rows(0, 0, n_cloud), 1 + len(ks)
    want, _ = _host_rows(name, gp_, gt, [n_cloud], A)
    assert SU.descriptor_error(alone[0], want) <= 8 * _any_config(name)[2]
    for q, k in enumerate(ks):
        assert both(rows(1 + q, k, k + n_cloud), alone), f"the cloud behind {k} far atoms"
        for j in range(k):
            assert both(rows(1 + q, j, j + 1), rows(lone0 + j % A, 0, 1)), f"far atom {j} of {k}"
    if sandwich:
        s = lone0 + A
        n = n_cloud
        assert both(rows(s + 1, 0, n), rows(s, 0, n)) and both(rows(s + 1, n + 32, 2 * n + 32), rows(s, n, 2 * n))
        assert both(rows(s + 3, 0, 32), rows(s + 2, 0, 32)) and both(rows(s + 3, 64, 64 + n), rows(s + 2, 32, 32 + n))
        for g, at in ((s + 1, n), (s + 3, 32)):
            for j in range(32):
                assert both(rows(g, at + j, at + j + 1), rows(lone0 + j % A, 0, 1))
    return desc


def test_chunk_phase_changes_no_bit():
    """Every output is one thread's ascending sum over the in-cut atoms, so where a graph's chunks of 32 fall cannot change a bit;
    a stale staging row or a missing barrier would.  k = 32, 33, 64 put whole chunks without a neighbour in front of the cloud."""
    _chunk_phase("small", 3, 40, (0, 1, 31, 32, 33, 64), True)


def test_chunk_phase_changes_no_bit_at_the_limit():
    _chunk_phase("limit", 4, 17, (0, 31, 32), False)


@pytest.mark.parametrize("name,A", [("small", 3), ("n7l5", 4)])
def test_graph_sizes_around_the_chunk_in_one_batch(name, A):
    sizes = [31, 32, 33, 63, 96, 97]
    rng = np.random.default_rng(41)
    pos = np.concatenate([rng.uniform(0, 2.2 * np.cbrt(n), (n, 3)) for n in sizes]).astype(np.float32)
    types = rng.integers(0, A, sum(sizes)).astype(np.int32)
    cfg, _, E = _any_config(name)
    want, want_coeff = _host_rows(name, pos, types, sizes, A)
    got, coeff = (x.cpu().numpy() for x in soap.soap_descriptors(torch.from_numpy(pos).to(DEV), _onehot(types, A).to(DEV), sizes, "all",
                                                                 SoapBasis(**SU.basis_of(cfg)), return_coefficients=True))
    err = SU.descriptor_error(got, want)
    print(f"E_device[{name}, sizes {sizes}] = {err:.3e} against the host statement; bar {8 * E:.3e}")
    assert err <= 8 * E and SU.descriptor_error(coeff, want_coeff) <= 8 * E


def test_types_outside_the_range_and_empty_graphs_through_the_entry_itself():
    """soap_math.h: "a type outside [0, A) contributes nothing".  The Python layer refuses such input, the kernel promises this."""
    name, A = "small", 3
    _, _, E = _any_config(name)
    sizes = [45, 17]
    rng = np.random.default_rng(43)
    pos = np.concatenate([rng.uniform(0, 2.2 * np.cbrt(n), (n, 3)) for n in sizes]).astype(np.float32)
    types = rng.integers(0, A, sum(sizes)).astype(np.int32)
    off = np.array([0, 5, 33, 44, 50])                                          # a first atom, both chunks of graph 0, graph 1
    disabled = types.copy()
    disabled[off] = [-1, A, -1, A, -1]
    keep = np.setdiff1d(np.arange(len(types)), off)
    reduced_sizes = [45 - 4, 17 - 1]
    assert SU.gap_ok(pos, sizes, SU.neighbour_cut(SU.CONFIGS[name]))
    got, got_c = _direct(name, pos, disabled, SU.graph_ptr(sizes), np.arange(len(types)), A, coeff=True)
    ref, ref_c = _direct(name, pos[keep], types[keep], SU.graph_ptr(reduced_sizes), np.arange(len(keep)), A, coeff=True)
    assert _same(got[keep], ref) and _same(got_c[keep], ref_c)                  # the disabled atoms are not there
    want, _ = _host_rows(name, pos[keep], types[keep], reduced_sizes, A)
    assert SU.descriptor_error(ref, want) <= 8 * E
    # A disabled CENTRE has no self-term: its row is the sum over the enabled atoms of its graph alone.  The host statement says so
    # when the centre carries a species of its own, A (so A + 1 types), that nobody else has: the blocks (z1, z2 < A) of that row do
    # not see the centre, and they are the whole row at A types.
    z1, z2, _, _, _ = SU.feature_index(A + 1, 3, 2)
    sub = (z1 < A) & (z2 < A)
    for i in off:
        others = np.setdiff1d(off, [i])
        kept = np.setdiff1d(np.arange(len(types)), others)
        t4 = types.copy()
        t4[i] = A
        sz = [sizes[0] - int(np.sum(others < 45)), sizes[1] - int(np.sum(others >= 45))]
        at = int(np.searchsorted(kept, i))
        row, _ = _host_rows(name, pos[kept], t4[kept], sz, A + 1, centres=[at])
        assert SU.descriptor_error(got[i:i + 1], row[:, sub]) <= 8 * E, i
        assert np.count_nonzero(got[i]) > 0
    # empty graphs first, in the middle and last: the binary search of graph_ptr
    pos, types, sizes = SU.fixture(A, 4)
    holes = [0, 1, 2, 0, 0, 5, 17, 0]
    cs = np.concatenate([np.arange(len(types)), [24, 0, 3]])
    plain, plain_c = _direct(name, pos, types, SU.graph_ptr(sizes), cs, A, coeff=True)
    holed, holed_c = _direct(name, pos, types, SU.graph_ptr(holes), cs, A, coeff=True)
    assert _same(plain, holed) and _same(plain_c, holed_c)
    want, _ = _host_rows(name, pos, types, holes, A, centres=cs)
    assert SU.descriptor_error(holed, want) <= 8 * E
    assert _same(plain, soap.soap_descriptors(torch.from_numpy(pos).to(DEV), _onehot(types, A).to(DEV), sizes, torch.from_numpy(cs),
                                              SoapBasis(**SU.CONFIGS[name])).cpu().numpy())


@pytest.mark.parametrize("F", SU.COSINE_F)
def test_cosine_kernels_at_the_row_pair_and_column_edges(F):
    for rows_a, rows_b in SU.COSINE_SHAPES:
        a, b = SU.cosine_rows(F, rows_a, F), SU.cosine_rows(F + 1000, rows_b, F)
        da, db = torch.from_numpy(a).to(DEV), torch.from_numpy(b).to(DEV)
        want = SU.cosine_matrix(a, b)
        rc, _, host = SU.host_cosines(_lib.lib(), a, b, gram=True)
        M = soap.cosine_matrix(da, db).cpu().numpy()
        assert rc == 0 and M.shape == want.shape and float(np.abs(M - want).max()) <= 4 * EPS and float(np.abs(M - host).max()) <= 4 * EPS
        assert _same(soap.cosine_matrix(da, db).cpu().numpy(), M)
        ij = np.stack(np.meshgrid(np.arange(rows_a), np.arange(rows_b), indexing="ij"), -1).reshape(-1, 2)
        assert _same(soap.cosine(da, db, torch.from_numpy(ij)).cpu().numpy().reshape(rows_a, rows_b), M)   # entry (i, j), bitwise
        for P in (1, 3, 4, 5):
            pairs = SU.cosine_pairs(P, rows_a, rows_b)
            got = soap.cosine(da, db, torch.from_numpy(pairs)).cpu().numpy()
            assert got.shape == (P,) and _same(got, M[pairs[:, 0], pairs[:, 1]])
            assert _same(soap.cosine(da, db, torch.from_numpy(pairs)).cpu().numpy(), got)
        if rows_a >= 3:
            a[1] = 0.0                                                          # a zero row: NaN in its row and in its column only
            da = torch.from_numpy(a).to(DEV)
            rc, _, host = SU.host_cosines(_lib.lib(), a, b, gram=True)
            M, Mt = soap.cosine_matrix(da, db).cpu().numpy(), soap.cosine_matrix(db, da).cpu().numpy()
            assert rc == 0 and np.array_equal(np.isnan(M), np.isnan(host)) and np.isnan(M[1]).all() and np.isnan(M).sum() == rows_b
            assert np.isnan(Mt[:, 1]).all() and np.isnan(Mt).sum() == rows_b
            assert float(np.nanmax(np.abs(M - host))) <= 4 * EPS


def _nearest_three_ways(t, r, k, groups=(None, None), ids=(None, None)):
    """device = host statement = restatement: indices exactly, mse bitwise -> (idx, mse, candidate matrix)"""
    with np.errstate(invalid="ignore"):
        idx, mse, m = SU.nearest(t, r, k, *groups)
    rc, hi, hm = SU.host_nearest(_lib.lib(), t, r, k, *groups)
    gi, gm = soap.nearest_spectra(torch.from_numpy(t).to(DEV), torch.from_numpy(r).to(DEV), k, *ids)
    gi, gm = gi.cpu().numpy(), gm.cpu().numpy()
    assert rc == 0 and np.array_equal(gi, idx) and np.array_equal(gi, hi)
    assert _same(gm, mse) and _same(gm, hm)
    return idx, mse, m


def test_nearest_spectra_with_exact_ties_go_to_the_lower_index():
    t, r = SU.tie_spectra()
    tid, rid = ["a", "b", None, ("c", 1), 70], [("a", "b", ("c", 1))[q % 3] for q in range(70)]
    tg, rg = np.array([0, 1, 2, 3, 4], np.int32), np.array([(0, 1, 3)[q % 3] for q in range(70)], np.int32)
    straddles = []
    for ids, groups in (((None, None), (None, None)), ((tid, rid), (tg, rg))):
        for k in range(1, 9):
            idx, mse, m = _nearest_three_ways(t, r, k, groups, ids)
            assert SU.mse_gap_ok_with_ties(m) and not SU.mse_gap_ok(m)
            order = np.argsort(m, axis=1, kind="stable")
            straddles += [(k, q) for q in range(5) if np.isfinite(m[q, order[q, k]]) and m[q, order[q, k - 1]] == m[q, order[q, k]]]
    m = SU.mse_matrix(t, r)
    assert m[0, 17].tobytes() == m[0, 18].tobytes() == m[0, 3].tobytes() == m[0, 40].tobytes() and m[1, 5].tobytes() == m[1, 6].tobytes()
    assert straddles, "no tie straddles a k-th place"
    idx = _nearest_three_ways(t, r, 8)[0]
    assert idx[0, :4].tolist() == [3, 17, 18, 40] and idx[1, :2].tolist() == [5, 6]
    assert _nearest_three_ways(t, r, 8, (tg, rg), (tid, rid))[0][0, :2].tolist() == [17, 40]   # 3 and 18 carry target 0's id


def test_nearest_spectra_at_the_wavefront_and_workgroup_edges():
    for S in (1, 63, 64, 65):
        for T in (1, 3, 4, 5):
            for R in (1, 2, 9):
                t, r = SU.spectra(1000 * S + 10 * T + R, T, R, S)
                idx, mse, m = _nearest_three_ways(t, r, 8)                      # fewer candidates than k
                assert SU.mse_gap_ok(m)
                assert (idx[:, min(R, 8):] == -1).all() and (idx[:, :min(R, 8)] >= 0).all() and np.isposinf(mse[:, min(R, 8):]).all()


def test_nearest_spectra_with_non_finite_rows():
    t, r = SU.nonfinite_spectra()
    for k in (1, 8):
        idx, mse, m = _nearest_three_ways(t, r, k)
        assert SU.mse_gap_ok(m)
        assert not np.isin(idx, (2, 7)).any(), "a reference holding NaN or +inf is never selected"
        assert (idx[1] == -1).all() and np.isposinf(mse[1]).all(), "a target holding NaN finds nothing"
        assert (idx[[0, 2, 3]] >= 0).all() and np.isfinite(mse[[0, 2, 3]]).all()
