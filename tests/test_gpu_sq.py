"""GPU tests of the reciprocal-space statistics (csrc/eval/sq.hip through diffusion_model_amd.stats and .cells) at the smallest
shapes at which the kernels can go wrong: against the host statement egnn_sq_host, against the numpy restatement of
tests/_sq_util.py, and against the truth at 50 digits (tests/golden/sq_golden.npz).

Bars.  On the golden inputs the device must stay within 8 x the host statement's measured error against the truth, and never above
the caps of tests/_sq_util.py (1e-10 sqrt(N_a N_b) for D, 1e-9 sqrt(N_a) for rho, 1e-9 (sqrt(N_a) + sqrt(N_b)) for the shells).
Where there is no truth (the edge shapes) the device is compared with the host statement and with the restatement under the caps
themselves: the three sum in different orders, and the rounding of a sum of n terms grows with n, so the error measured on 65
atoms is no bound for 1025.  Integer outputs (hkl, bin, counts, vec_ptr) and |k| are bitwise the host statement's.  Every input
first passes the gap checks (asserted, never skipped).

The Debye kernel's blocks are 64 atoms i x 256 atoms j per tile and 256 / 512 q values per thread slot / pass; the rho kernel's
are 256 vectors per workgroup and 1024 staged atoms; the shell kernel looks at 1024 vectors per step.
"""
import functools
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from diffusion_model_amd import _lib, cells, stats
from tests import _cells_util as CU
from tests import _sq_util as SU

pytestmark = pytest.mark.gpu
DEV = "cuda"
G = SU.golden()
RAGGED = [0, 1, 2, 63, 64, 65, 130, 255, 256, 257]      # the row block of 64, the chunk of 256, and partial last blocks
ODD_Q = np.array([7.3, 0.0, 1.5, 25.0, 1.5, 0.05, 0.0])  # unsorted, with 0 and repeats


def _onehot(types, A):
    return torch.eye(A, dtype=torch.int64)[torch.from_numpy(np.asarray(types)).long()]


def _device_debye(pos, types, sizes, A, q, r_max=None, window=None):
    D = stats.debye_sums(torch.from_numpy(pos).to(DEV), _onehot(types, A).to(DEV), sizes, q, r_max=r_max, window=window)
    assert D.dtype == torch.float64 and tuple(D.shape) == (len(sizes), A, A, len(q))
    return D.cpu().numpy()


def _batch(sizes, A, seed, absent=None):
    parts = [SU.cloud(n, seed + 17 * i, A=A) for i, n in enumerate(sizes)]
    pos, types = np.concatenate([p for p, _ in parts]), np.concatenate([t for _, t in parts])
    if absent is not None:
        types[types == absent] = 0
    return pos, types


def _q_list(Q, uniform):
    if uniform:
        return 0.05 * np.arange(Q)                       # a uniform grid from 0
    q = np.random.default_rng(Q).uniform(0.0, 25.0, Q)   # any order
    q[: min(Q, len(ODD_Q))] = ODD_Q[:Q]
    return q


@functools.lru_cache(maxsize=None)
def _e_host():
    """the host statement's measured errors on the golden inputs: (Debye, rho, shells)"""
    lib = _lib.lib()
    e_d = e_r = e_s = 0.0
    for name in ("ragged", "coincident", "lorch"):
        c = SU.golden_cluster(G, name)
        D = SU.host_debye(lib, c["pos"], c["types"], c["sizes"], 2, G["q"], c["r_max"], c["window"])
        e_d = max(e_d, SU.debye_error(D, c["truth"], SU.n_types(c["types"], c["sizes"], 2)))
    for name in ("triclinic", "pair"):
        c = SU.golden_cell(G, name)
        h = SU.host_cells(lib, [c], c["q_max"], c["dq"])
        nt = np.bincount(c["types"], minlength=2)
        e_r, e_s = max(e_r, SU.rho_error(h["rho"], c["rho"], nt)), max(e_s, SU.shell_error(h["s"][0], c["s"], nt))
    return e_d, e_r, e_s


# ---- Debye sums ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["ragged", "coincident", "lorch"])
def test_debye_sums_equal_the_truth(name):
    c = SU.golden_cluster(G, name)
    bar = min(SU.CAP_DEBYE, 8 * _e_host()[0])
    D = _device_debye(c["pos"], c["types"], c["sizes"], 2, G["q"], c["r_max"], c["window"])
    err = SU.debye_error(D, c["truth"], SU.n_types(c["types"], c["sizes"], 2))
    print(f"{name}: device {err:.2e}, host statement {_e_host()[0]:.2e}, bar {bar:.2e}")
    assert err <= bar


@functools.lru_cache(maxsize=None)
def _ragged(A):
    return _batch(RAGGED, A, 300 + A, absent=A - 1 if A > 1 else None)


@pytest.mark.parametrize("Q", [1, 63, 64, 65, 255, 256, 257, 511, 512, 513])
@pytest.mark.parametrize("uniform", [False, True])
def test_debye_sums_at_the_q_block_edges(Q, uniform):
    pos, types = _ragged(2)
    sizes = RAGGED[:7]                                   # up to 130 atoms: every q block against every row block edge
    n = sum(sizes)
    q = _q_list(Q, uniform)
    D = _device_debye(pos[:n], types[:n], sizes, 2, q)
    H = SU.host_debye(_lib.lib(), pos[:n], types[:n], sizes, 2, q)
    nt = SU.n_types(types[:n], sizes, 2)
    assert SU.debye_error(D, H, nt) <= SU.CAP_DEBYE
    assert np.array_equal(D, D.transpose(0, 2, 1, 3))
    zero = q == 0
    if zero.any():
        want = (nt[:, :, None] * nt[:, None, :] - np.stack([np.diag(v) for v in nt])).astype(np.float64)
        assert np.array_equal(D[..., zero], np.repeat(want[..., None], zero.sum(), -1))


@pytest.mark.parametrize("A", [1, 2, 4])
@pytest.mark.parametrize("cut", [None, "cut", "lorch"])
def test_debye_sums_at_the_tile_edges(A, cut):
    """the whole ragged batch (chunk edges at 255, 256, 257 atoms), an absent type, with and without the cut and the window"""
    pos, types = _ragged(A)
    r_max = None if cut is None else 5.9
    assert SU.debye_gap_ok(pos, RAGGED, r_max)
    kw = dict(r_max=r_max, window="lorch" if cut == "lorch" else None)
    D = _device_debye(pos, types, RAGGED, A, ODD_Q, **kw)
    nt = SU.n_types(types, RAGGED, A)
    assert A == 1 or np.all(nt[:, A - 1] == 0)
    assert SU.debye_error(D, SU.host_debye(_lib.lib(), pos, types, RAGGED, A, ODD_Q, **kw), nt) <= SU.CAP_DEBYE
    assert SU.debye_error(D, SU.debye_restated(pos, types, RAGGED, A, ODD_Q, **kw), nt) <= SU.CAP_DEBYE
    assert np.array_equal(D[..., 2], D[..., 4]) and np.array_equal(D[..., 1], D[..., 6])      # the repeated q values


@pytest.mark.parametrize("cut", [None, "lorch"])
def test_debye_sums_of_a_graph_of_many_tiles(cut):
    """1025 atoms: 17 row blocks x 5 chunks, the last of each one atom wide"""
    pos, types = _batch([1025], 2, 77)
    r_max = None if cut is None else 6.0
    assert SU.debye_gap_ok(pos, [1025], r_max)
    kw = dict(r_max=r_max, window=cut)
    D = _device_debye(pos, types, [1025], 2, ODD_Q, **kw)
    nt = SU.n_types(types, [1025], 2)
    e_h = SU.debye_error(D, SU.host_debye(_lib.lib(), pos, types, [1025], 2, ODD_Q, **kw), nt)
    e_r = SU.debye_error(D, SU.debye_restated(pos, types, [1025], 2, ODD_Q, **kw), nt)
    print(f"1025 atoms ({cut}): device - host statement {e_h:.2e}, device - restatement {e_r:.2e}")
    assert e_h <= SU.CAP_DEBYE and e_r <= SU.CAP_DEBYE


def test_coincident_and_nearly_coincident_atoms():
    pos, types = SU.cloud(40, 9)
    pos[7] = pos[3]                                                  # coincident
    pos[11] = pos[5] + np.array([1e-6, 0, 0], dtype=np.float32)       # 1e-6 A apart (a few float32 steps)
    assert 0 < SU.distances(pos)[5, 11] < 2e-6
    for uniform in (False, True):
        q = _q_list(65, uniform)
        D = _device_debye(pos, types, [40], 2, q)
        nt = SU.n_types(types, [40], 2)
        assert np.all(np.isfinite(D))
        assert SU.debye_error(D, SU.host_debye(_lib.lib(), pos, types, [40], 2, q), nt) <= SU.CAP_DEBYE
        assert SU.debye_error(D, SU.debye_restated(pos, types, [40], 2, q), nt) <= SU.CAP_DEBYE


def test_debye_sums_are_reproducible_and_independent_of_the_batch():
    pos, types = _ragged(2)
    q = _q_list(65, False)
    a, b = _device_debye(pos, types, RAGGED, 2, q, r_max=5.9, window="lorch"), _device_debye(pos, types, RAGGED, 2, q, r_max=5.9, window="lorch")
    assert np.array_equal(a.view(np.int64), b.view(np.int64))
    lo = 0
    for g, n in enumerate(RAGGED):
        if n in (1, 65, 257):
            alone = _device_debye(pos[lo:lo + n], types[lo:lo + n], [n], 2, q, r_max=5.9, window="lorch")
            assert np.array_equal(alone[0].view(np.int64), a[g].view(np.int64)), n
        lo += n


# ---- cells ---------------------------------------------------------------------------------------------------------------------------
def _as_cell(c):
    return cells.PeriodicCell(c["lattice"], c["frac"], types=c["types"], num_types=c["A"], id=c["name"])


@functools.lru_cache(maxsize=None)
def _cell_batch():
    """cells of 1, 2, 24 (triclinic), 63, 64, 65 and 257 atoms with different lattices, and one too small for any vector"""
    out = [SU.cell_dict(5.0 * np.eye(3), [[0.3, 0.6, 0.9]], [0], "one"), SU.golden_cell(G, "pair"), SU.golden_cell(G, "triclinic")]
    for n in (63, 64, 65, 257):
        c = CU.random_cell(n, 500 + n, spread=1.0 if n == 65 else 0.0, check=False)
        out.append(SU.cell_dict(c["lattice"], c["frac"], c["types"], c["name"]))
    out.append(SU.cell_dict(0.9 * np.eye(3), [[0.2, 0.4, 0.6], [0.7, 0.1, 0.5]], [0, 1], "no-vector"))
    return out


def _compare_with_host(cs, q_max, dq, golden_bar=False):
    for c in cs:
        assert SU.cell_gap_ok(c["lattice"], q_max, dq), c["name"]
    h = SU.host_cells(_lib.lib(), cs, q_max, dq)
    d = cells.structure_factor([_as_cell(c) for c in cs], q_max=q_max, dq=dq, vectors=True, device=DEV)
    assert d.count.dtype == torch.int64 and d.hkl.dtype == torch.int32 and d.rho.dtype == torch.complex128
    assert np.array_equal(d.vec_ptr.numpy(), h["vec_ptr"])
    assert np.array_equal(d.hkl.cpu().numpy(), h["hkl"]) and np.array_equal(d.bin.cpu().numpy(), h["bin"])
    assert np.array_equal(d.k.cpu().numpy().view(np.int64), h["k"].view(np.int64))
    assert np.array_equal(d.count.cpu().numpy(), h["count"])
    rho, s, mean_k = d.rho.cpu().numpy(), d.s.cpu().numpy(), d.mean_k.cpu().numpy()
    assert np.array_equal(np.isnan(mean_k), h["count"] == 0)
    assert np.allclose(mean_k, h["mean_k"], rtol=1e-14, atol=0, equal_nan=True)
    worst_r = worst_s = 0.0
    for i, c in enumerate(cs):
        lo, hi = h["vec_ptr"][i], h["vec_ptr"][i + 1]
        nt = np.bincount(c["types"], minlength=2)
        worst_r = max(worst_r, SU.rho_error(rho[lo:hi], h["rho"][lo:hi], nt),
                      SU.rho_error(rho[lo:hi], SU.rho_restated(c["frac"], c["types"], 2, h["hkl"][lo:hi]), nt))
        worst_s = max(worst_s, SU.shell_error(s[i], h["s"][i], nt))
    assert worst_r <= SU.CAP_RHO and worst_s <= SU.CAP_SHELL
    return d, h


def test_cells_of_many_sizes_in_one_batch():
    cs = _cell_batch()
    d, h = _compare_with_host(cs, 6.0, 0.25)
    assert h["vec_ptr"][-1] == h["vec_ptr"][-2] and np.all(h["count"][-1] == 0) and torch.isnan(d.s[-1]).all()
    counts = np.diff(h["vec_ptr"])
    assert counts.max() > 1024 and sorted(d.sizes) == [1, 2, 2, 24, 63, 64, 65, 257]     # more than one step of the shell kernel
    again = cells.structure_factor([_as_cell(c) for c in cs], q_max=6.0, dq=0.25, vectors=True, device=DEV)
    for key in ("rho", "s", "mean_k", "k"):
        a, b = getattr(d, key), getattr(again, key)
        assert torch.equal(torch.view_as_real(a) if a.is_complex() else a.view(torch.int64),
                           torch.view_as_real(b) if b.is_complex() else b.view(torch.int64)), key
    tri = 2                                                # a cell alone gives the bits it gives inside the batch
    alone = cells.structure_factor(_as_cell(cs[tri]), q_max=6.0, dq=0.25, vectors=True, device=DEV)
    lo, hi = h["vec_ptr"][tri], h["vec_ptr"][tri + 1]
    assert torch.equal(torch.view_as_real(alone.rho), torch.view_as_real(d.rho[lo:hi]))
    assert torch.equal(alone.s[0].view(torch.int64), d.s[tri].view(torch.int64))


@pytest.mark.parametrize("name", ["triclinic", "pair"])
def test_cell_sums_equal_the_truth(name):
    c = SU.golden_cell(G, name)
    d, _ = _compare_with_host([c], c["q_max"], c["dq"])
    nt = np.bincount(c["types"], minlength=2)
    _, e_r, e_s = _e_host()
    bar_r, bar_s = min(SU.CAP_RHO, 8 * e_r), min(SU.CAP_SHELL, 8 * e_s)
    got_r, got_s = SU.rho_error(d.rho.cpu().numpy(), c["rho"], nt), SU.shell_error(d.s[0].cpu().numpy(), c["s"], nt)
    print(f"{name}: device rho {got_r:.2e} (bar {bar_r:.2e}), shells {got_s:.2e} (bar {bar_s:.2e})")
    assert np.array_equal(d.hkl.cpu().numpy(), c["hkl"]) and got_r <= bar_r and got_s <= bar_s


@pytest.mark.parametrize("count", [255, 256, 257, 1023, 1024, 1025])
def test_a_vector_count_about_the_vector_block(count):
    """q_max between the count-th and the next |k| of the triclinic cell: one below, at and one above the 256 vectors of a
    workgroup of the rho kernel and the 1024 vectors of a step of the shell kernel"""
    c = SU.golden_cell(G, "triclinic")
    box, k2 = SU.box_candidates(c["lattice"], 8.0)
    ka = np.sort(np.sqrt(k2[SU.half_space(box)]))
    q_max = 0.5 * (ka[count - 1] + ka[count])
    _, h = _compare_with_host([c], float(q_max), 0.25)
    assert h["vec_ptr"][-1] == count


# ---- the public layer ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["faber-ziman", "ashcroft-langreth"])
def test_structure_factor_forms_and_weights(form):
    sizes = [1, 3, 65, 130]
    pos, types = _batch(sizes, 2, 900)
    types[1:4] = 0                                          # the 3-atom graph lacks type 1
    q = 0.5 + 0.05 * np.arange(65)
    D = SU.debye_restated(pos, types, sizes, 2, q)
    nt = SU.n_types(types, sizes, 2)
    p, oh = torch.from_numpy(pos).to(DEV), _onehot(types, 2).to(DEV)
    ff = np.stack([5.0 + np.exp(-q / 9.0), 4.0 + 0.01 * q])    # [A, Q]
    for weights, b in ((None, np.array(stats.NEUTRON_LENGTHS)), ((1.0, 2.5), np.array([1.0, 2.5])), (torch.from_numpy(ff), ff)):
        sf = stats.structure_factor(p, oh, sizes, q, weights=weights, form=form)
        want_p, want_t = SU.finish_restated(D, nt, b, form)
        assert torch.equal(sf.n_type.cpu(), torch.from_numpy(nt)) and sf.sizes == sizes
        assert np.allclose(sf.partial.cpu().numpy(), want_p, rtol=0, atol=1e-9) and np.allclose(sf.total.cpu().numpy(), want_t, rtol=0, atol=1e-9)
        assert np.all(sf.partial[1, 1].cpu().numpy() == 0) and np.all(sf.partial[1, 0, 1].cpu().numpy() == 0)
    cs = _cell_batch()[:3]
    h = SU.host_cells(_lib.lib(), cs, 6.0, 0.25)
    d = cells.structure_factor([_as_cell(c) for c in cs], q_max=6.0, dq=0.25, form=form, weights=(1.0, 2.5), device=DEV)
    nt = np.stack([np.bincount(c["types"], minlength=2) for c in cs])
    Dc = h["s"] - np.stack([np.diag(v) for v in nt.astype(np.float64)])[..., None]
    want_p, want_t = SU.finish_restated(np.nan_to_num(Dc), nt, np.array([1.0, 2.5]), form)
    live = h["count"] > 0
    assert np.allclose(d.partial.cpu().numpy()[:, 1, 0][live], want_p[:, 1, 0][live], rtol=0, atol=1e-9)
    assert np.allclose(d.partial.cpu().numpy()[2, 0, 0][live[2]], want_p[2, 0, 0][live[2]], rtol=0, atol=1e-9)
    assert np.allclose(d.total.cpu().numpy()[live], want_t[live], rtol=0, atol=1e-9)
    assert torch.isnan(d.total[~torch.from_numpy(live)]).all() and np.allclose(d.q.cpu().numpy(), (np.arange(24) + 0.5) * 0.25)


def test_compare_structure_factors():
    a, b, c = SU.cloud(64, 1), SU.cloud(64, 2), SU.cloud(20, 3)
    graph = lambda pt, on, k=0: SimpleNamespace(pos=torch.from_numpy(pt[0]).to(on), x=_onehot(pt[1], 2).to(on), id=f"mp-{k}")  # noqa: E731
    originals = [graph(a, "cpu", 0), graph(c, "cpu", 1), graph(b, "cpu", 2)]
    same = stats.compare_structure_factors(originals, [[graph(a, DEV)], [graph(c, DEV)], [graph(b, DEV)]])
    assert same["sizes"] == [64, 20, 64] and tuple(same["q"].shape) == (491,) and abs(float(same["q"][-1]) - 25.0) < 1e-12
    assert tuple(same["partial"]["cos"].shape) == (3, 2, 2) and tuple(same["total_curve"]["l2"].shape) == (3,)
    for m in (same["partial"], same["total_curve"], same["total"]["partial"], same["total"]["total_curve"]):
        assert float((m["cos"] - 1).abs().max()) <= 1e-12 and float(m["l2"].abs().max()) == 0.0 and float(m["wasserstein"].abs().max()) == 0.0
    other = stats.compare_structure_factors(originals, [[graph(b, DEV)], [graph(c, DEV)], [graph(a, DEV)]], q=np.linspace(0.5, 12.0, 47))
    assert float(other["partial"]["l2"][1].abs().max()) == 0.0 and float(other["partial"]["l2"][0].min()) > 0.0
    assert float(other["total_curve"]["cos"][0]) < 1.0 and stats.compare_structure_factors([], []) == {}


def test_limits_raise_clear_errors():
    pos, types = SU.cloud(5, 4)
    p, oh = torch.from_numpy(pos).to(DEV), _onehot(types, 2).to(DEV)
    for bad, msg in (([0.5, -1.0], "finite and not negative"), ([0.5, float("nan")], "finite and not negative"), (np.zeros(4097), "at most 4096"),
                     ([], "at least one")):
        with pytest.raises(ValueError, match=msg):
            stats.debye_sums(p, oh, [5], bad)
    with pytest.raises(ValueError, match="Lorch"):
        stats.debye_sums(p, oh, [5], [0.5], window="lorch")
    with pytest.raises(ValueError, match="window"):
        stats.debye_sums(p, oh, [5], [0.5], window="hann", r_max=3.0)
    with pytest.raises(ValueError, match="5 atom types"):
        stats.debye_sums(p, _onehot(types, 5).to(DEV), [5], [0.5])
    with pytest.raises(ValueError, match="weights is required"):
        stats.structure_factor(p, _onehot(types, 3).to(DEV), [5], [0.5])
    with pytest.raises(ValueError, match="weights must be"):
        stats.structure_factor(p, oh, [5], [0.5, 1.0], weights=[1.0, 2.0, 3.0])
    with pytest.raises(ValueError, match="form"):
        stats.structure_factor(p, oh, [5], [0.5], form="bhatia-thornton")
    big = torch.zeros(32769 + 2, 3, device=DEV)
    with pytest.raises(ValueError, match="graph 1 has 32769 atoms"):
        stats.debye_sums(big, torch.ones(32771, 1, device=DEV), [2, 32769], [0.5])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        stats.debye_sums(p.cpu(), oh.cpu(), [5], [0.5])
    good = cells.PeriodicCell(5.0 * torch.eye(3), [[0.1, 0.2, 0.3]], types=[0])
    flat = cells.PeriodicCell([[5.0, 0, 0], [0, 5, 0], [5, 5, 0]], [[0.1, 0.2, 0.3]], types=[0])
    with pytest.raises(ValueError, match="cell 1: singular"):
        cells.structure_factor([good, flat], device=DEV)
    with pytest.raises(ValueError, match="cell 0: q_max = 1287.0 needs a Miller index of 1024"):
        cells.structure_factor(good, q_max=1287.0, dq=1.0, device=DEV)
    with pytest.raises(ValueError, match="shell bins"):
        cells.structure_factor(good, q_max=6.0, dq=0.001, device=DEV)
    with pytest.raises(ValueError, match="cell 0: 5 atom types"):
        cells.structure_factor(cells.PeriodicCell(5.0 * torch.eye(3), [[0.1, 0.2, 0.3]], types=[4]), device=DEV)
    with pytest.raises(ValueError, match="reciprocal vectors below q_max"):
        cells.structure_factor(cells.PeriodicCell(60.0 * torch.eye(3), [[0.1, 0.2, 0.3]], types=[0]), q_max=25.0, dq=0.05, weights=[1.0], device=DEV)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        cells.structure_factor(good, device="cpu")
