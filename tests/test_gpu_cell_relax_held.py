"""The held-row evaluation of cells.relax (cell_relax_real_kernel, csrc/cells/cell_relax.hip) where it differs from the lattice-energy
kernel: at coordinates that have MOVED since the rows were searched, read unwrapped, every entry tested again against r_cut.

  1. egnn_cell_relax_real alone, on rows built by the numpy box walk at r_cut + skin on the reference coordinates w0 and evaluated at
     u = w0 + delta L^-1, |delta_i| <= skin / 2 (tests/_cell_relax_util.held: the constructions are checked without a device in
     tests/test_cell_relax_host.py), against the same truncated sums in mpmath at the wrapped u (no reciprocal vector: the truth's force
     is the real-space force).  The bar is the project's, 8 x max(E_host, 1e-16), E_host of egnn_cell_ewald_host on the same case under
     the same metric restricted to (e_real, e_short, F).  alpha * r_cut <= 3 and an unshifted pair table: one site too many or too few
     at the cutoff is ten orders above the bar.  Kept rows of 1, 63, 64, 65 and 129 sites, a held row of three wavefront passes that
     keeps less than one, a row that keeps nothing, the limit of the completeness argument (a site that stood r_cut + skin - 1e-3 away),
     a centre beyond a face and its own images, a coincidence that exists only after the move, and 8 + 2 + 1 centres in one launch.
  2. cells.relax(max_steps=k) for k = 0 .. 24 on the compressed rocksalt cell with the cap active: every evaluation of a real
     trajectory against a fresh cells.lattice_energy at the same coordinates, per atom and per component, and three of them (lists one
     full skin / 2 old, before the first two rebuilds, and the last) against the truth; once more on 192 atoms of displaced
     cristobalite with the rows refreshed on the device (method="grid")."""
import functools

import numpy as np
import pytest
import torch

from diffusion_model_amd import _lib, cells
from tests import _cell_ewald_util as EU
from tests import _cell_relax_util as RU
from tests import _cell_stats_util as STU

pytestmark = pytest.mark.gpu
FLOOR = 1e-16         # an E_host of exactly 0 (a case of no term) still allows the rounding of one operation


def _cell(c, A=None):
    return cells.PeriodicCell(c["lattice"], c["frac"], types=c["types"], num_types=c["A"] if A is None else A)


def _up(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def held_real(hs, row_args=None):
    """egnn_cell_relax_real on a batch of held cases with the model of the first: the coordinates are every case's u, the rows those of
    the box walk on the reference coordinates (or ``row_args``: the eight row arguments as cells._row_args gives them)
    -> (real [N, 5], coincident [C]); every output starts at -7 / 0"""
    L, c0 = _lib.lib(), hs[0]["case"]
    a = STU.batch_arrays([h["case"]["cell"] for h in hs])
    C, N = len(hs), int(a["cell_ptr"][-1])
    d = {k: _up(v) for k, v in a.items()}
    if row_args is None:
        rows = [_up(r) for r in RU.held_rows(hs)]
        who = _up(np.arange(N, dtype=np.int32))
        row_args = (N, _lib.ptr(rows[0]), int(rows[1].shape[0]), _lib.ptr(rows[1]), _lib.ptr(rows[2]), N, _lib.ptr(who), _lib.ptr(who))
    real = torch.full((N, 5), -7.0, dtype=torch.float64, device="cuda")
    flag = torch.zeros(C, dtype=torch.int32, device="cuda")
    q = np.ascontiguousarray(c0["charges"], dtype=np.float64)
    _lib.check(L.egnn_cell_relax_real(_lib.stream_ptr(), C, N, c0["cell"]["A"], RU.vp(a["cell_ptr"]), RU.vp(a["lattice"]), _lib.ptr(d["cell_ptr"]),
                                      _lib.ptr(d["lattice"]), _lib.ptr(d["frac"]), _lib.ptr(d["type"]), RU.vp(q), RU.vp(c0["pot"]), c0["n"],
                                      int(c0["shift"]), c0["kappa"], c0["alpha"], c0["r_cut"], c0["short_cut"], c0["k_max"], hs[0]["skin"], *row_args,
                                      _lib.ptr(real), _lib.ptr(flag)))
    return real.cpu().numpy(), flag.cpu().numpy()


@functools.lru_cache(maxsize=None)
def alone(name):
    """a held case in a launch of its own: computed once, never changed"""
    return held_real([RU.held(name)])


def check_against_truth(name):
    ex, e_host = RU.held_truth(name)
    assert e_host <= EU.CAP and float(ex["gap"]) > EU.GAP
    real, flag = alone(name)
    E, bar = RU.held_error(real, ex), 8 * max(e_host, FLOOR)
    print(f"held {name}: E(device, truth) = {E:.3e}  E_host = {e_host:.3e}  bar = {bar:.3e}  kept {np.diff(ex['row_ptr']).tolist()}")
    assert E <= bar
    assert flag.tolist() == [0]
    return real, ex


# ---- 1. the kernel alone ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("length", RU.HELD_ROWS)
def test_kept_row_lengths(length):
    real, ex = check_against_truth(f"row{length}")
    assert length in np.diff(ex["row_ptr"]).tolist()


def test_the_moved_thin_cell_and_the_rows_of_the_device_search():
    """r_cut = 3.2 A, skin 0.5 A: in every row entries have entered and left r_cut since the build.  The rows of cells._SiteSearch on
    the reference coordinates are those of the box walk, and give the same bits."""
    real, ex = check_against_truth("thin")
    h = RU.held("thin")
    cb = cells._CellBatch([_cell(h["ref"])], None)
    search = cells._SiteSearch(cb, h["case"]["r_cut"] + h["skin"], "direct")
    args, keep = cells._row_args(search, *cells._centres(cb, None))
    for mine, theirs in zip(RU.held_rows([h]), keep[:3]):
        assert np.array_equal(mine, theirs.cpu().numpy())
    again, flag = held_real([h], args)
    assert np.array_equal(again, real) and flag.tolist() == [0]


def test_three_passes_over_a_held_row_that_keeps_less_than_one():
    real, ex = check_against_truth("three")
    held = np.diff(RU.held_rows([RU.held("three")])[0])
    assert held.min() > 128 and held.max() <= 192 and np.diff(ex["row_ptr"]).max() < 64


def test_a_row_whose_every_entry_lies_outside_now():
    real, ex = check_against_truth("outside")
    assert np.diff(RU.held_rows([RU.held("outside")])[0]).tolist() == [6] and ex["row_ptr"].tolist() == [0, 0]
    assert not real.any()


def test_the_limit_of_the_completeness_argument():
    """atoms 0 and 1 stood r_cut + skin - 1e-3 apart and have come skin - 2e-4 closer: each is the other's only site.  Atoms 2 and 3 have
    left each other's sphere: zeros."""
    real, ex = check_against_truth("limit")
    assert np.diff(ex["row_ptr"]).tolist() == [1, 1, 0, 0]
    assert real[:2, 0].all() and real[:2, 1].all() and real[:2, 2].all() and not real[2:].any()


def test_a_centre_beyond_a_face_and_its_own_images():
    real, ex = check_against_truth("face")
    u = RU.held("face")["case"]["cell"]["frac"]
    assert u[0, 0] > 1.0
    lo, hi = ex["row_ptr"][:2]
    assert 0 in ex["atom"][lo:hi].tolist() and 1 in ex["atom"][lo:hi].tolist()


def test_a_coincidence_that_appears_only_after_the_move():
    hs = [RU.held("pair"), RU.held("coincide"), RU.held("pair")]
    real, flag = held_real(hs)
    assert flag.tolist() == [0, 1, 0]
    assert np.array_equal(real[0:2], alone("pair")[0]) and np.array_equal(real[4:6], alone("pair")[0])
    assert np.isfinite(real).all()                                  # the site on its centre adds nothing
    built, flag0 = held_real([dict(hs[1], case=dict(hs[1]["case"], cell=hs[1]["ref"]))])
    assert flag0.tolist() == [0] and np.isfinite(built).all()       # at the coordinates of the build there is none


def test_one_launch_over_three_cells_of_eleven_centres():
    """8 + 2 + 1 centres: three workgroups of four wavefronts, the last with one idle; every cell has the bits it has alone"""
    names = ["thin", "pair", "single"]
    hs = [RU.held(n) for n in names]
    real, flag = held_real(hs)
    assert real.shape == (11, 5) and flag.tolist() == [0, 0, 0]
    lo = 0
    for n in names:
        one = alone(n)[0]
        assert np.array_equal(real[lo:lo + len(one)], one), n
        lo += len(one)
    again, _ = held_real(hs)
    assert np.array_equal(again, real)
    check_against_truth("pair")
    check_against_truth("single")


# ---- 2. every evaluation of a real trajectory -----------------------------------------------------------------------------------------------
K_LAST = 24
TRAJECTORY = dict(skin=0.4, f_max=1e-4)       # max_step = 0.2 = skin / 2: the cap is active, a list is one full skin / 2 old before a rebuild


def relax(case, **kw):
    pot = cells.PairTable(*case["pot"], n=case["n"])
    return cells.relax([_cell(case["cell"])], case["charges"], pot, r_cut=case["r_cut"], short_cut=case["short_cut"], shift=case["shift"],
                       alpha=case["alpha"], k_max=case["k_max"], coulomb_constant=case["kappa"], **kw)


def fresh(case, res, **kw):
    pot = cells.PairTable(*case["pot"], n=case["n"])
    return cells.lattice_energy(res.cells, case["charges"], pot, r_cut=case["r_cut"], short_cut=case["short_cut"], shift=case["shift"],
                                alpha=case["alpha"], k_max=case["k_max"], coulomb_constant=case["kappa"], **kw)


def outputs(res):
    """the outputs of a one-cell Relaxation or CellEnergy as tests/_cell_ewald_util.error reads them"""
    return dict(e_atom=res.energy_per_atom.cpu().numpy(), comp_atom=res.components_per_atom.cpu().numpy(), force=res.forces.cpu().numpy(),
                energy=res.energy[0].cpu().numpy(), components=res.components[0].cpu().numpy())


@functools.lru_cache(maxsize=None)
def trajectory():
    """cells.relax(max_steps=k), k = 0 .. K_LAST, on the compressed rocksalt cell: computed once, never changed"""
    case = RU.compressed_rocksalt(3.8, 3)
    return case, [relax(case, max_steps=k, **TRAJECTORY) for k in range(K_LAST + 1)]


@functools.lru_cache(maxsize=None)
def truths():
    """-> {k: (EU.exact at res.frac of run k, E_host there)} for the two k just before the first two rebuilds and for K_LAST"""
    case, runs = trajectory()
    n = [int(r.n_rebuilds[0]) for r in runs]
    grows = [k for k in range(K_LAST) if n[k + 1] > n[k]]
    assert len(grows) >= 2, n
    out = {}
    for k in (grows[0], grows[1], K_LAST):
        at = dict(case, cell=dict(case["cell"], frac=runs[k].frac.cpu().numpy()))
        rc, h = EU.host(_lib.lib(), [at])
        assert rc == 0, _lib.lib().egnn_last_error()
        ex = EU.exact(at)
        assert float(ex["gap"]) > EU.GAP, (k, float(ex["gap"]))
        e_host = EU.error(h, ex)
        assert e_host <= EU.CAP
        out[k] = (ex, e_host)
    return out


def test_the_stop_at_max_steps_is_a_prefix_of_the_trajectory():
    case, runs = trajectory()
    n = [int(r.n_rebuilds[0]) for r in runs]
    print(f"n_rebuilds at k = 0 .. {K_LAST}: {n}")
    assert [int(r.steps[0]) for r in runs] == list(range(K_LAST + 1)) and not any(bool(r.converged[0]) for r in runs)
    assert all(b >= a for a, b in zip(n, n[1:])) and len(set(n)) >= 3          # non-decreasing, and it grows at least twice
    for k, r in enumerate(runs):
        one = relax(case, max_steps=k, check_every=1, **TRAJECTORY)
        assert torch.equal(one.frac, r.frac) and torch.equal(one.forces, r.forces) and torch.equal(one.energy, r.energy), k
        assert int(one.n_rebuilds[0]) == n[k]


def test_evaluations_before_a_rebuild_against_the_truth():
    case, runs = trajectory()
    for k, (ex, e_host) in truths().items():
        E, bar = EU.error(outputs(runs[k]), ex), 8 * max(e_host, FLOOR)
        print(f"k = {k}: n_rebuilds = {int(runs[k].n_rebuilds[0])}  E(held row, truth) = {E:.3e}  E_host = {e_host:.3e}  bar = {bar:.3e}")
        assert E <= bar, k


def test_every_evaluation_equals_a_fresh_one():
    """the held-row evaluation at u_k against cells.lattice_energy at the same coordinates, under the metric of the truth with the scales
    of the nearest k that has one"""
    case, runs = trajectory()
    T = truths()
    worst = 0.0
    for k, r in enumerate(runs):
        near = min(T, key=lambda t: (abs(t - k), t))
        ex, e_host = T[near]
        new = outputs(fresh(case, r))
        E, bar = EU.error(outputs(r), dict(ex, **{name: new[name] for name in ("e_atom", "comp_atom", "force", "energy", "components")})), \
            8 * max(e_host, FLOOR)
        worst = max(worst, E / bar)
        print(f"k = {k}: E(held row, fresh) = {E:.3e}  bar = {bar:.3e} (scales of k = {near})")
        assert E <= bar, k
    print(f"largest E / bar = {worst:.3f}")


def test_rows_refreshed_on_the_device_against_a_fresh_evaluation():
    """192 atoms of displaced cristobalite, 40 moves with the rows of the linked-cell search refreshed on the device at every rebuild: the
    last held-row evaluation against cells.lattice_energy (the direct search) at the same coordinates.  The cell is too large for 50
    digits: the scales are those of the truth in fp64 (tests/_cell_relax_util.scales, checked against the fixtures' on the host), and
    the bar is that of the BKS cristobalite fixture, 8 x E_host of the same model on the same structure."""
    case = RU.cristobalite192()
    res = relax(case, method="grid", f_max=1e-2, max_steps=40, skin=0.2, fire=cells.FireParameters(max_step=0.1))
    assert res.steps.tolist() == [40] and int(res.n_rebuilds[0]) >= 1
    new = outputs(fresh(case, res))
    se, sf = RU.scales(dict(case, cell=dict(case["cell"], frac=res.frac.cpu().numpy())))
    E, bar = EU.error(outputs(res), dict(new, scale_e=se, scale_f=sf)), 8 * max(EU.e_host("crist"), FLOOR)
    print(f"cristobalite 192, k = 40: n_rebuilds = {int(res.n_rebuilds[0])}  E(held row, fresh) = {E:.3e}  bar = {bar:.3e}")
    assert E <= bar
