"""CPU tests of the reciprocal-space statistics: the host statement egnn_sq_host (csrc/eval/sq_host.cpp, the text the kernels
compile through sq_math.h) against

  * the truth at 50 digits (tests/golden/sq_golden.npz, written by tests/golden/make_sq_golden.py with mpmath) under the caps
    max |D - D_truth| / sqrt(N_a N_b) <= 1e-10, max |rho_a - rho_truth| / sqrt(N_a) <= 1e-9 and, per shell,
    |S_ab - S_truth| <= 1e-9 (sqrt(N_a) + sqrt(N_b)) with S_ab = <Re rho_a rho_b*> / sqrt(N_a N_b).  The caps are conditions (a
    few-ulp error per term times the term count at <= 4096 atoms), not fitted to this code; the measured errors are printed;
  * the numpy float64 restatement (tests/_sq_util.py): every integer output bitwise;
  * exact and hand cases; every bad argument, from the host statement and, before any launch, from the device entries;
  * a stand-alone program under the address and undefined-behaviour sanitizers.

Every input first passes the gap checks of tests/_sq_util.py (asserted, never skipped).
"""
import ctypes as C

import numpy as np
import pytest

from diffusion_model_amd import _lib
from tests import _cells_util as CU
from tests import _sq_util as SU
from tests._host_program import build_and_run

EINVAL = -22
G = SU.golden()
Q = G["q"]
CLUSTERS = ("ragged", "coincident", "lorch")
CELLS = ("triclinic", "pair")


def _lib_():
    return _lib.lib()


def _host_cluster(name):
    c = SU.golden_cluster(G, name)
    return c, SU.host_debye(_lib_(), c["pos"], c["types"], c["sizes"], 2, Q, c["r_max"], c["window"])


def e_host_debye():
    """the host statement's measured error on the golden clusters"""
    worst = 0.0
    for name in CLUSTERS:
        c, D = _host_cluster(name)
        worst = max(worst, SU.debye_error(D, c["truth"], SU.n_types(c["types"], c["sizes"], 2)))
    return worst


# ---- the truth -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", CLUSTERS)
def test_debye_sums_equal_the_truth_within_the_cap(name):
    c, D = _host_cluster(name)
    nt = SU.n_types(c["types"], c["sizes"], 2)
    err = SU.debye_error(D, c["truth"], nt)
    rest = SU.debye_error(SU.debye_restated(c["pos"], c["types"], c["sizes"], 2, Q, c["r_max"], c["window"]), c["truth"], nt)
    print(f"{name}: host statement {err:.2e}, restatement {rest:.2e} (cap {SU.CAP_DEBYE:.0e})")
    assert err <= SU.CAP_DEBYE and rest <= SU.CAP_DEBYE


@pytest.mark.parametrize("name", CELLS)
def test_cell_sums_equal_the_truth_within_the_caps(name):
    c = SU.golden_cell(G, name)
    h = SU.host_cells(_lib_(), [c], c["q_max"], c["dq"])
    nt = np.bincount(c["types"], minlength=2)
    assert np.array_equal(h["hkl"], c["hkl"])
    assert np.max(np.abs(h["k"] - c["k"])) <= 4e-16 * c["q_max"]
    e_rho, e_s = SU.rho_error(h["rho"], c["rho"], nt), SU.shell_error(h["s"][0], c["s"], nt)
    print(f"{name}: {len(c['hkl'])} vectors, rho {e_rho:.2e} (cap {SU.CAP_RHO:.0e}), shells {e_s:.2e} (cap {SU.CAP_SHELL:.0e})")
    assert e_rho <= SU.CAP_RHO and e_s <= SU.CAP_SHELL


# ---- the restatement: integer outputs bitwise ----------------------------------------------------------------------------------------
def _cells():
    tri = SU.golden_cell(G, "triclinic")
    cr = CU.cristobalite_cell()
    return [tri, SU.golden_cell(G, "pair"), SU.cell_dict(cr["lattice"], cr["frac"], cr["types"], "cristobalite"),
            SU.cell_dict(0.9 * np.eye(3), [[0.2, 0.4, 0.6]], [0], "no-vector")]


def test_vectors_bins_and_shell_counts_equal_the_restatement_exactly():
    cells, q_max, dq = _cells(), 6.0, 0.25
    for c in cells:
        assert SU.cell_gap_ok(c["lattice"], q_max, dq), c["name"]
    h = SU.host_cells(_lib_(), cells, q_max, dq)
    for i, c in enumerate(cells):
        hkl, ka, bins = SU.vectors_restated(c["lattice"], q_max, dq)
        lo, hi = h["vec_ptr"][i], h["vec_ptr"][i + 1]
        assert hi - lo == len(hkl), c["name"]
        assert np.array_equal(h["hkl"][lo:hi], hkl) and np.array_equal(h["bin"][lo:hi], bins)
        assert np.array_equal(h["k"][lo:hi].view(np.int64), ka.view(np.int64))
        # brute force: every integer triple of a box two wider, both half spaces
        box, k2 = SU.box_candidates(c["lattice"], q_max, extra=2)
        inside = (k2 < q_max * q_max) & np.any(box != 0, axis=1)
        full = np.concatenate([box[inside & (box[:, 0] > 0)]] * 2 + [box[inside & (box[:, 0] == 0)]])
        k_full = np.sqrt(np.concatenate([k2[inside & (box[:, 0] > 0)]] * 2 + [k2[inside & (box[:, 0] == 0)]]))
        assert len(full) == 2 * len(hkl)
        count = np.bincount(np.floor(k_full / dq).astype(np.int64), minlength=h["nbins"])
        assert np.array_equal(h["count"][i], count), c["name"]
        cnt, mean_k, s = SU.shells_restated(ka, bins, SU.rho_restated(c["frac"], c["types"], 2, hkl), h["nbins"])
        assert np.array_equal(cnt, h["count"][i])
        assert np.array_equal(np.isnan(mean_k), h["count"][i] == 0) and np.array_equal(np.isnan(h["mean_k"][i]), h["count"][i] == 0)
        assert np.allclose(h["mean_k"][i], mean_k, rtol=1e-14, atol=0, equal_nan=True)
        assert SU.shell_error(h["s"][i], s, np.bincount(c["types"], minlength=2)) <= SU.CAP_SHELL
    assert h["vec_ptr"][4] == h["vec_ptr"][3] and np.all(h["count"][3] == 0) and np.all(np.isnan(h["s"][3]))


# ---- exact and hand cases ------------------------------------------------------------------------------------------------------------
def test_zero_q_counts_the_pairs_exactly_and_d_is_symmetric():
    sizes = [0, 1, 2, 63, 130]
    parts = [SU.cloud(n, 40 + n, A=3) for n in sizes]
    pos, types = np.concatenate([p for p, _ in parts]), np.concatenate([t for _, t in parts])
    q = np.array([0.0, 1.3, 0.0, 9.0])
    D = SU.host_debye(_lib_(), pos, types, sizes, 3, q)
    nt = SU.n_types(types, sizes, 3).astype(np.float64)
    want = nt[:, :, None] * nt[:, None, :] - np.stack([np.diag(v) for v in nt])
    assert np.array_equal(D[..., 0], want) and np.array_equal(D[..., 2], want)
    assert np.array_equal(D, D.transpose(0, 2, 1, 3))


def test_a_dimer_gives_two_sinc():
    pos = np.array([[0.0, 0.0, 0.0], [1.0, 2.0, 2.0]], dtype=np.float32)     # r = 3 exactly
    q = np.array([0.0, 0.5, 1.5, 7.3, 25.0])
    D = SU.host_debye(_lib_(), pos, np.array([0, 0], np.int32), [2], 1, q)
    assert np.max(np.abs(D[0, 0, 0] - 2.0 * SU.sinc(3.0 * q))) <= 4e-16
    D = SU.host_debye(_lib_(), pos, np.array([0, 1], np.int32), [2], 2, q)
    assert np.all(D[0, 0, 0] == 0) and np.all(D[0, 1, 1] == 0) and np.max(np.abs(D[0, 0, 1] - SU.sinc(3.0 * q))) <= 4e-16
    D = SU.host_debye(_lib_(), pos, np.array([0, 0], np.int32), [2], 1, q, r_max=4.0, window="lorch")
    assert np.max(np.abs(D[0, 0, 0] - 2.0 * SU.sinc(np.pi * 3.0 / 4.0) * SU.sinc(3.0 * q))) <= 4e-16
    assert np.all(SU.host_debye(_lib_(), pos, np.array([0, 0], np.int32), [2], 1, q, r_max=3.0) == 0)   # r < r_max is strict


def test_permuting_atoms_and_relabelling_types_permutes_the_outputs():
    bar = 8 * e_host_debye()
    print(f"host statement's measured error {bar / 8:.2e}; bar {bar:.2e}")
    assert bar <= SU.CAP_DEBYE
    c = SU.golden_cluster(G, "ragged")
    lo = sum(c["sizes"][:3])
    pos, types = c["pos"][lo:], c["types"][lo:]
    D = SU.host_debye(_lib_(), pos, types, [65], 2, Q)
    perm = np.random.default_rng(5).permutation(65)
    Dp = SU.host_debye(_lib_(), pos[perm], (1 - types)[perm], [65], 2, Q)
    nt = SU.n_types(types, [65], 2)
    assert SU.debye_error(Dp[:, ::-1, ::-1], D, nt) <= bar


def test_a_simple_cubic_supercell_has_its_bragg_peaks_only():
    c, q_max, dq = SU.simple_cubic_supercell(), 6.0, 0.25
    assert SU.cell_gap_ok(c["lattice"], q_max, dq)
    h = SU.host_cells(_lib_(), [c], q_max, dq, A=1)
    bragg = np.all(h["hkl"] % 4 == 0, axis=1)
    assert bragg.sum() >= 10 and (~bragg).sum() >= 1000
    mod = np.abs(h["rho"][:, 0])
    assert np.max(np.abs(mod[bragg] - 64.0)) / 8.0 <= SU.CAP_RHO and np.max(mod[~bragg]) / 8.0 <= SU.CAP_RHO


def test_cristobalite_has_no_intensity_at_its_forbidden_reflections():
    cr = CU.cristobalite_cell()
    c = SU.cell_dict(cr["lattice"], cr["frac"], cr["types"], "cristobalite")
    assert SU.cell_gap_ok(c["lattice"], 6.0, 0.25)
    h = SU.host_cells(_lib_(), [c], 6.0, 0.25)
    par = h["hkl"] % 2
    mixed = ~(np.all(par == 0, axis=1) | np.all(par == 1, axis=1))          # the face-centred lattice of both species
    glide = np.all(par == 0, axis=1) & (h["hkl"].sum(1) % 4 == 2)            # the diamond sites of Si (type 1)
    assert mixed.sum() > 100 and glide.sum() >= 5
    assert np.max(np.abs(h["rho"][mixed, 0])) / 4.0 <= SU.CAP_RHO and np.max(np.abs(h["rho"][mixed, 1])) / np.sqrt(8.0) <= SU.CAP_RHO
    assert np.max(np.abs(h["rho"][glide, 1])) / np.sqrt(8.0) <= SU.CAP_RHO
    allowed = np.all(h["hkl"] == [1, 1, 1], axis=1)
    assert np.abs(h["rho"][allowed, 1])[0] > 1.0


# ---- bad arguments -------------------------------------------------------------------------------------------------------------------
def _bad_debye(**kw):
    pos, types = SU.cloud(5, 1)
    a = dict(pos=pos, types=types, sizes=[5], A=2, q=np.array([0.5, 1.0]), r_max=None, window=None)
    a.update(kw)
    return SU.host_debye(_lib_(), a["pos"], a["types"], a["sizes"], a["A"], a["q"], a["r_max"], a["window"], raw=True)[0]


def test_the_host_statement_rejects_bad_arguments():
    lib = _lib_()
    assert _bad_debye() == 0
    assert _bad_debye(A=5) == EINVAL and b"atom types" in lib.egnn_last_error()
    assert _bad_debye(q=np.linspace(0, 1, 4097)) == EINVAL and b"4096" in lib.egnn_last_error()
    assert _bad_debye(q=np.linspace(0, 1, 4096)) == 0
    for bad in (-0.5, np.nan, np.inf):
        assert _bad_debye(q=np.array([0.5, bad])) == EINVAL and b"q[1]" in lib.egnn_last_error()
    assert _bad_debye(window="lorch") == EINVAL and b"Lorch" in lib.egnn_last_error()
    assert _bad_debye(window="lorch", r_max=4.0) == 0
    assert _bad_debye(r_max=0.0) == EINVAL
    assert _bad_debye(types=np.array([0, 1, 2, 0, 1], np.int32)) == EINVAL and b"type" in lib.egnn_last_error()
    assert _bad_debye(sizes=[4]) == EINVAL and b"graph_ptr" in lib.egnn_last_error()      # runs from 0 to 4, N = 5
    assert _bad_debye(sizes=[7, -2]) == EINVAL
    good = SU.cell_dict(5.0 * np.eye(3), [[0.1, 0.2, 0.3]], [0], "one")
    assert SU.host_cells(lib, [good], 6.0, 0.25, raw=True) == 0
    assert SU.host_cells(lib, [good], 6.0, 0.25, A=5, raw=True) == EINVAL
    assert SU.host_cells(lib, [good], 6.0, 0.001, raw=True) == EINVAL and b"shell bins" in lib.egnn_last_error()     # 6000 bins
    flat = SU.cell_dict([[5, 0, 0], [0, 5, 0], [5, 5, 0]], [[0.1, 0.2, 0.3]], [0], "flat")
    assert SU.host_cells(lib, [good, flat], 6.0, 0.25, raw=True) == EINVAL and b"cell 1 has a singular lattice" in lib.egnn_last_error()
    assert SU.host_cells(lib, [good], 1287.0, 1.0, raw=True) == EINVAL and b"Miller index" in lib.egnn_last_error()   # 1024.2 > 1023
    assert SU.host_cells(lib, [SU.cell_dict(5.0 * np.eye(3), [[0.1, 0.2, 0.3]], [2], "type")], 6.0, 0.25, raw=True) == EINVAL
    assert SU.host_cells(lib, [SU.cell_dict(5.0 * np.eye(3), [[0.1, np.nan, 0.3]], [0], "nan")], 6.0, 0.25, raw=True) == EINVAL


def test_the_device_entries_reject_bad_arguments_before_any_launch():
    """every call below fails in the host-side checks: no stream, no device memory, no GPU is touched"""
    lib = _lib_()
    dummy = np.zeros(64, dtype=np.float64)
    d = dummy.ctypes.data_as(C.c_void_p)
    q_ok = np.array([0.5, 1.0])

    def debye(A=2, q=q_ok, r_max=np.inf, window=0, max_atoms=5):
        q = np.ascontiguousarray(q, dtype=np.float64)
        return lib.egnn_sq_debye(None, 1, A, d, d, d, max_atoms, q.size, q.ctypes.data_as(C.c_void_p), d, r_max, window, d, -1, d, d, d)

    assert debye() == EINVAL and b"n_tiles" in lib.egnn_last_error()       # the good arguments get as far as the tile check
    assert debye(A=5) == EINVAL and b"atom types" in lib.egnn_last_error()
    assert debye(q=np.linspace(0, 1, 4097)) == EINVAL and b"4096" in lib.egnn_last_error()
    for bad in (-1.0, np.nan, np.inf):
        assert debye(q=[0.5, bad]) == EINVAL and b"q[1]" in lib.egnn_last_error()
    assert debye(window=1) == EINVAL and b"Lorch" in lib.egnn_last_error()
    assert debye(max_atoms=32769) == EINVAL and b"32768" in lib.egnn_last_error()

    good, flat = np.ascontiguousarray(5.0 * np.eye(3).reshape(1, 9)), np.array([[5.0, 0, 0, 0, 5, 0, 5, 5, 0]])
    plan, n_rows = np.zeros((1, 4), dtype=np.int32), np.zeros(1, dtype=np.int32)
    p = lambda a: a.ctypes.data_as(C.c_void_p)   # noqa: E731
    assert lib.egnn_sq_cell_plan(1, p(flat), 6.0, p(plan), p(n_rows)) == EINVAL and b"singular" in lib.egnn_last_error()
    assert lib.egnn_sq_cell_plan(1, p(good), 1287.0, p(plan), p(n_rows)) == EINVAL and b"Miller index" in lib.egnn_last_error()
    assert lib.egnn_sq_cell_plan(1, p(good), 6.0, p(plan), p(n_rows)) == 0
    H = int(np.floor(6.0 * 5.0 / (2 * np.pi))) + 1
    assert plan.tolist() == [[H, H, H, 0]] and int(n_rows[0]) == (H + 1) * (2 * H + 1)
    assert lib.egnn_sq_cell_count(None, 1, p(flat), p(plan), d, d, 6.0, int(n_rows[0]), d) == EINVAL
    assert lib.egnn_sq_cell_count(None, 1, p(good), p(plan), d, d, 1287.0, int(n_rows[0]), d) == EINVAL
    assert lib.egnn_sq_cell_count(None, 1, p(good), p(plan), d, d, 6.0, int(n_rows[0]) + 1, d) == EINVAL and b"n_rows" in lib.egnn_last_error()
    cell_ptr, vec_ptr = np.array([0, 1], dtype=np.int32), np.array([0, 3], dtype=np.int32)

    def rho(A=2, lattice=good, q_max=6.0, dq=0.25, nbins=24, vp=vec_ptr, K=3, N=1):
        return lib.egnn_sq_cell_rho(None, 1, N, A, p(cell_ptr), p(lattice), p(plan), p(vp), d, d, d, d, d, d, q_max, dq, nbins, int(n_rows[0]), d,
                                    K, d, -1, d, d, d, d)

    assert rho() == EINVAL and b"n_tiles" in lib.egnn_last_error()         # the good arguments get as far as the tile check
    assert rho(A=5) == EINVAL and rho(lattice=flat) == EINVAL and rho(N=2) == EINVAL
    assert rho(dq=0.001, nbins=6000) == EINVAL and b"shell bins" in lib.egnn_last_error()
    assert rho(nbins=25) == EINVAL and b"nbins" in lib.egnn_last_error()
    big = np.array([0, (1 << 24) + 1], dtype=np.int32)
    assert rho(vp=big, K=(1 << 24) + 1) == EINVAL and b"vectors below q_max" in lib.egnn_last_error()
    assert lib.egnn_sq_cell_shells(None, 1, 2, 4097, p(vec_ptr), d, 3, d, d, d, d, d, d) == EINVAL
    assert lib.egnn_sq_cell_shells(None, 1, 5, 24, p(vec_ptr), d, 3, d, d, d, d, d, d) == EINVAL
    assert lib.egnn_sq_cell_shells(None, 1, 2, 24, p(big), d, (1 << 24) + 1, d, d, d, d, d, d) == EINVAL


# ---- the public layer has no CPU path ------------------------------------------------------------------------------------------------
def test_cpu_tensors_raise():
    import torch
    from diffusion_model_amd import cells, stats
    pos, oh = torch.zeros(3, 3), torch.eye(2)[[0, 1, 0]]
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        stats.debye_sums(pos, oh, [3], [0.5])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        stats.structure_factor(pos, oh, [3], [0.5])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        cells.structure_factor(cells.PeriodicCell(5.0 * torch.eye(3), [[0.1, 0.2, 0.3]], types=[0]), device="cpu")


def test_the_tile_list_visits_every_pair_block_once():
    from diffusion_model_amd.stats import _sq_tiles
    sizes = [0, 1, 2, 63, 64, 65, 130, 1025]
    tiles, tile_ptr = _sq_tiles(sizes)
    assert tile_ptr[0] == 0 and tile_ptr[-1] == len(tiles) and np.all(np.diff(tile_ptr) >= 0)
    for g, n in enumerate(sizes):
        mine = tiles[tile_ptr[g]:tile_ptr[g + 1]]
        assert np.all(mine[:, 0] == g)
        seen = np.zeros((n, n), dtype=np.int64)
        for _, c0, j0 in mine:
            i, j = np.arange(c0, min(c0 + 64, n)), np.arange(j0, min(j0 + 256, n))
            seen[np.ix_(i, j)] += i[:, None] < j[None, :]
        assert np.array_equal(seen, np.triu(np.ones((n, n), dtype=np.int64), 1))
    assert [len(_sq_tiles(s)[0]) for s in ([64] * 256, [512] * 32, [4096])] == [256, 384, 544]


# ---- sanitizers ----------------------------------------------------------------------------------------------------------------------
def test_sq_host_under_sanitizers(tmp_path):
    """the executable links its own sanitizer runtime (statically), so nothing is preloaded"""
    r = build_and_run(tmp_path, "sq_main", ["eval/sq_host.cpp", "host_logic.cpp"])
    assert r.returncode == 0 and "SQ-OK" in r.stdout, f"rc={r.returncode}\nstdout:\n{r.stdout}\nstderr:\n{r.stderr[-4000:]}"
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]
