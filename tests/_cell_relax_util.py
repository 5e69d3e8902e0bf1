"""The relaxation of periodic cells (csrc/cells/cell_relax_math.h) for the CPU and GPU tests (test infrastructure): the rocksalt
fixture, a numpy restatement of the step in the order of the header (256 strided partial sums, then the tree 128 .. 1), a scripted
sequence of forces that reaches every branch of the step, and the ctypes wrappers of the two host statements.

  * state of a batch: a dict of the arrays the step entries take (frac, velocity, since, moved, scalars [C, 5], counters [C, 4],
    done, rebuild, energy_trace, force_trace) -- ``new_state``;
  * ``step_restated`` changes such a dict as egnn_cell_relax_step_host does and returns the branch every cell took;
  * ``rebuild_restated`` is the caller's part of a rebuild: u <- wrap(u), since <- 0, the flag cleared;
  * held cases (``held``, ``HELD_CASES``): cells whose rows were walked at r_cut + skin on reference coordinates and whose atoms have
    moved by up to skin / 2 since, with the re-test in numpy, the truth's rows in the names of the held rows and the error metric of
    the lattice energy restricted to what egnn_cell_relax_real writes; ``scales``: the error scales of the truth in fp64.
"""
import functools
import math

import numpy as np

from tests import _cell_ewald_util as EU
from tests import _cells_util as CU
from tests import _cell_stats_util as STU

vp = EU.vp
THREADS = 256
RUNNING, CONVERGED, STEP_LIMIT, COINCIDENT, NOT_FINITE, STUCK = range(6)
FIRE = dict(dt=0.1, dt_max=1.0, n_min=5, f_inc=1.1, f_dec=0.5, a_start=0.1, f_a=0.99, max_step=0.2)
IDEAL_CAP = 1e-5        # the final rocksalt sites lie this close to the ideal ones (A): a cap, not a measurement
ROCKSALT = dict(f_max=1e-6, max_steps=480)   # 480: four times the 120 moves the restatement needed; a cap, not a measurement


def fire_args(fire):
    return (fire["dt_max"], fire["n_min"], fire["f_inc"], fire["f_dec"], fire["a_start"], fire["f_a"], fire["max_step"])


# ---- the rocksalt fixture -----------------------------------------------------------------------------------------------------------
def rocksalt_tables():
    pot = np.zeros((4, 2, 2))
    pot[0] = [[0.0, 1200.0], [1200.0, 0.0]]
    pot[1] = [[1.0, 3.125], [3.125, 1.0]]
    return pot


def rocksalt(translate=0.0):
    """-> (case with the displaced atoms, the ideal cell): charges (1, -1), A = 1200 eV and b = 3.125 / A on the unlike pair,
    r_cut = short_cut = 6, accuracy 1e-8, the atoms displaced by default_rng(5).uniform(-0.15, 0.15) A and then translated by
    ``translate`` in fractional coordinates"""
    ideal = EU.nacl_cell(5.64)
    disp = np.random.default_rng(5).uniform(-0.15, 0.15, (8, 3))
    cell = dict(ideal, frac=ideal["frac"] + disp / 5.64 + translate)
    return EU.make_case(cell, (1.0, -1.0), rocksalt_tables(), r_cut=6.0, short_cut=6.0, accuracy=1e-8, kappa=EU.KAPPA), ideal


def deviation(start_frac, moved, ideal, lattice):
    """the largest distance (A) of a final site from its ideal one after removing the mean translation; the final sites are the
    start plus the net unwrapped move"""
    d = (np.asarray(start_frac) - ideal["frac"]) @ np.asarray(lattice, np.float64) + moved
    d = d - d.mean(0)
    return float(np.sqrt((d * d).sum(1)).max())


# ---- the step restated --------------------------------------------------------------------------------------------------------------
def _dot(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def _reduce(x, is_max):
    """the order of cell_relax_math.h: partial t adds (or maximises) the terms t, t + 256, .. ascending from 0, then the tree"""
    part = np.zeros(THREADS)
    for k in range(0, len(x), THREADS):
        chunk = x[k:k + THREADS]
        part[:len(chunk)] = np.maximum(part[:len(chunk)], chunk) if is_max else part[:len(chunk)] + chunk
    off = THREADS // 2
    while off:
        part[:off] = np.maximum(part[:off], part[off:2 * off]) if is_max else part[:off] + part[off:2 * off]
        off //= 2
    return float(part[0])


def inverse(L):
    a, b, c = np.asarray(L, np.float64).reshape(3, 3)
    cross = lambda p, q: np.array([p[1] * q[2] - p[2] * q[1], p[2] * q[0] - p[0] * q[2], p[0] * q[1] - p[1] * q[0]])
    bc, ca, ab = cross(b, c), cross(c, a), cross(a, b)
    det = (a[0] * bc[0] + a[1] * bc[1]) + a[2] * bc[2]
    return np.stack([bc / det, ca / det, ab / det])


def new_state(cell_ptr, frac, fire, max_steps, trace=True):
    C, N = len(cell_ptr) - 1, int(cell_ptr[-1])
    sc = np.zeros((C, 5))
    sc[:, 0], sc[:, 1] = fire["dt"], fire["a_start"]
    return dict(frac=np.array(frac, dtype=np.float64).reshape(N, 3), velocity=np.zeros((N, 3)), since=np.zeros((N, 3)), moved=np.zeros((N, 3)),
                scalars=sc, counters=np.zeros((C, 4), np.int32), done=np.zeros(C, np.int32), rebuild=np.zeros(C, np.int32),
                energy_trace=np.full((max_steps + 1, C), np.nan) if trace else None, force_trace=np.full((max_steps + 1, C), np.nan) if trace else None)


def copy_state(s):
    return {k: (None if v is None else v.copy()) for k, v in s.items()}


def same_state(a, b):
    """the names of the arrays of two states that differ in a bit (NaN equals NaN)"""
    return [k for k in a if a[k] is not None and not np.array_equal(a[k], b[k], equal_nan=a[k].dtype.kind == "f")]


def step_restated(s, cell_ptr, lattice, force, energy, coincident, fire, f_max, max_steps, skin):
    """one step of every cell on the state ``s`` in place -> the branch of each cell: "idle", "coincident", "not finite", "converged",
    "limit", "frozen", or "move" with the flags "+" (P > 0), "g" (dt grown), "-" (P <= 0), "c" (capped)"""
    out = []
    for c in range(len(cell_ptr) - 1):
        lo, hi = int(cell_ptr[c]), int(cell_ptr[c + 1])
        if s["done"][c] or s["rebuild"][c]:
            out.append("idle")
            continue
        sc, ct = s["scalars"][c], s["counters"][c]
        if coincident[c]:
            ct[2], s["done"][c] = COINCIDENT, 1
            out.append("coincident")
            continue
        F, v, since = force[lo:hi], s["velocity"][lo:hi], s["since"][lo:hi]
        ff = _dot(F, F)
        P, FF, vv, fm2 = _reduce(_dot(F, v), False), _reduce(ff, False), _reduce(_dot(v, v), False), _reduce(ff, True)
        if not FF < 1e300:
            ct[2], s["done"][c] = NOT_FINITE, 1
            out.append("not finite")
            continue
        steps, dt, a, n_pos = int(ct[1]), float(sc[0]), float(sc[1]), int(ct[0])
        sc[2], sc[4] = energy[c], np.sqrt(fm2)
        if steps == 0:
            sc[3] = energy[c]
        if s["energy_trace"] is not None:
            s["energy_trace"][steps, c], s["force_trace"][steps, c] = energy[c], np.sqrt(fm2)
        if fm2 < f_max * f_max:
            ct[2], s["done"][c] = CONVERGED, 1
            out.append("converged")
            continue
        if steps >= max_steps:
            ct[2], s["done"][c] = STEP_LIMIT, 1
            out.append("limit")
            continue
        tag = "move"
        if P > 0.0:
            tag += "+"
            coef = (a * np.sqrt(vv)) / np.sqrt(FF)
            vn = (1.0 - a) * v + coef * F
            if n_pos > fire["n_min"]:
                tag += "g"
                dt, a = min(dt * fire["f_inc"], fire["dt_max"]), a * fire["f_a"]
            n_pos += 1
            vn = vn + dt * F
        else:
            tag += "-"
            a, dt, n_pos = fire["a_start"], dt * fire["f_dec"], 0
            vn = dt * F
        dr = dt * vn
        m = np.sqrt(_reduce(_dot(dr, dr), True))
        scale = fire["max_step"] / m if m > fire["max_step"] else 1.0
        if scale != 1.0:
            tag += "c"
        dr = scale * dr
        reach = since + dr
        if _reduce(_dot(since, since), True) > 0.0 and np.sqrt(_reduce(_dot(reach, reach), True)) > 0.5 * skin:
            if ct[3] == steps + 1:                      # froze at this step count before: not moved in between
                ct[2], s["done"][c] = STUCK, 1
                out.append("stuck")
                continue
            ct[3] = steps + 1
            s["rebuild"][c] = 1
            out.append("frozen")
            continue
        K = inverse(lattice[c])
        du = np.stack([_dot(dr, K[k][None, :]) for k in range(3)], 1)
        s["velocity"][lo:hi] = vn
        s["frac"][lo:hi] = s["frac"][lo:hi] + du
        s["since"][lo:hi] = reach
        s["moved"][lo:hi] = s["moved"][lo:hi] + dr
        sc[0], sc[1], ct[0], ct[1] = dt, a, n_pos, steps + 1
        out.append(tag)
    return out


def rebuild_restated(s, cell_ptr):
    for c in np.nonzero(s["rebuild"])[0]:
        lo, hi = int(cell_ptr[c]), int(cell_ptr[c + 1])
        s["frac"][lo:hi] = CU.wrap(s["frac"][lo:hi])
        s["since"][lo:hi] = 0.0
        s["rebuild"][c] = 0


# ---- the scripted sequence ------------------------------------------------------------------------------------------------------------
SCRIPT_SIZES = (1, 63, 64, 65, 257, 1025)
SCRIPT = dict(f_max=1e-3, max_steps=14, skin=0.6)
SCRIPT_LATTICE = np.array([[7.1, 0.0, 0.0], [0.9, 6.3, 0.0], [-0.4, 1.1, 8.2]])


def script():
    """-> (cell_ptr, lattice [C, 9], frac, calls): ``calls`` is a list of (force [N, 3], energy [C], coincident [C]).  The cells of
    SCRIPT_SIZES atoms all see the same kind of force at a call: a fixed direction field g scaled by the call's factor -- 0 velocity
    first (P <= 0), the same sign for eight calls (P > 0, then dt grows), a reversal (P <= 0), a large factor (the cap, then the
    freeze at skin 0.6 after capped moves of 0.2 A), small forces on the even cells (convergence) and large ones on the odd cells
    until max_steps; the last cell meets a coincident site at the end."""
    rng = np.random.default_rng(11)
    cell_ptr = np.concatenate([[0], np.cumsum(SCRIPT_SIZES)]).astype(np.int32)
    C, N = len(SCRIPT_SIZES), int(cell_ptr[-1])
    lattice = np.ascontiguousarray(np.tile(SCRIPT_LATTICE.reshape(1, 9), (C, 1)))
    frac = rng.uniform(-0.3, 1.3, (N, 3))
    g = rng.normal(size=(N, 3))
    cell_of = np.repeat(np.arange(C), SCRIPT_SIZES)
    factors = [1.0] * 9 + [-1.0, -1.0, 300.0, 300.0, 300.0]
    calls = []
    for k, f in enumerate(factors):
        calls.append((np.ascontiguousarray(f * g + 0.01 * rng.normal(size=(N, 3))), rng.normal(size=C), np.zeros(C, np.int32)))
    for k in range(8):
        per_cell = np.where(np.arange(C) % 2 == 0, 1e-5, 50.0)
        coincident = np.zeros(C, np.int32)
        coincident[C - 1] = int(k == 5)
        calls.append((np.ascontiguousarray(per_cell[cell_of, None] * g), rng.normal(size=C), coincident))
    return cell_ptr, lattice, frac, calls


# ---- the host statements ---------------------------------------------------------------------------------------------------------------
def step_host(L, s, cell_ptr, lattice, force, energy, coincident, fire, f_max, max_steps, skin):
    C, N = len(cell_ptr) - 1, int(cell_ptr[-1])
    return L.egnn_cell_relax_step_host(C, N, vp(cell_ptr), vp(lattice), vp(force), vp(energy), vp(coincident), *fire_args(fire), f_max, max_steps,
                                       skin, vp(s["frac"]), vp(s["velocity"]), vp(s["since"]), vp(s["moved"]), vp(s["scalars"]), vp(s["counters"]),
                                       vp(s["done"]), vp(s["rebuild"]), vp(s["energy_trace"]), vp(s["force_trace"]))


def relax_host(L, cases, f_max=1e-3, max_steps=1000, skin=1.0, fire=None, trace=True, **override):
    """egnn_cell_relax_host on the cells of ``cases`` with the parameters of the first -> (rc, dict)"""
    fire = dict(FIRE, **(fire or {}))
    c0 = dict(cases[0], **override)
    a = STU.batch_arrays([c["cell"] for c in cases])
    C, N, A = len(a["cell_ptr"]) - 1, int(a["cell_ptr"][-1]), max(c["cell"]["A"] for c in cases)
    rows = max(int(max_steps), 0) + 1
    out = dict(frac=np.full((N, 3), -7.0), energy=np.full(C, -7.0), initial_energy=np.full(C, -7.0), force=np.full((N, 3), -7.0),
               max_force=np.full(C, -7.0), steps=np.full(C, -7, np.int32), status=np.full(C, -7, np.int32), moved=np.full((N, 3), -7.0),
               n_rebuilds=np.full(C, -7, np.int32), energy_trace=np.full((rows, C), -7.0) if trace else None,
               force_trace=np.full((rows, C), -7.0) if trace else None, frac_trace=np.full((rows, N, 3), -7.0) if trace else None,
               start=a["frac"].copy())
    q = np.ascontiguousarray(c0["charges"], dtype=np.float64)
    rc = L.egnn_cell_relax_host(C, A, vp(a["cell_ptr"]), vp(a["lattice"]), vp(a["frac"]), vp(a["type"]), vp(q), vp(c0["pot"]), c0["n"],
                                int(c0["shift"]), c0["kappa"], c0["alpha"], c0["r_cut"], c0["short_cut"], c0["k_max"], fire["dt"], *fire_args(fire),
                                float(f_max), int(max_steps), float(skin), vp(out["frac"]), vp(out["energy"]), vp(out["initial_energy"]),
                                vp(out["force"]), vp(out["max_force"]), vp(out["steps"]), vp(out["status"]), vp(out["moved"]),
                                vp(out["n_rebuilds"]), vp(out["energy_trace"]), vp(out["force_trace"]), vp(out["frac_trace"]))
    return rc, out


@functools.lru_cache(maxsize=None)
def rocksalt_host(translate=0.0, skin=2.0):
    """the host loop on the rocksalt fixture (computed once, never changed) -> (result dict, deviation from the ideal sites in A)"""
    from diffusion_model_amd import _lib
    case, ideal = rocksalt(translate)
    rc, out = relax_host(_lib.lib(), [case], skin=skin, **ROCKSALT)
    assert rc == 0, _lib.lib().egnn_last_error()
    return out, deviation(out["start"], out["moved"], ideal, ideal["lattice"])


def d_host():
    """D_host: the deviation of the host loop (skin 2.0, no rebuild) from the ideal rocksalt sites, in A"""
    return rocksalt_host()[1]


def restated_loop(L, case, f_max, max_steps, skin, fire=None):
    """FIRE restated in numpy, its forces from egnn_cell_ewald_host at every step, for ONE cell that never asks for a rebuild
    -> dict(frac_trace, energy_trace, steps, frac, energy, status)"""
    fire = dict(FIRE, **(fire or {}))
    cell = case["cell"]
    cell_ptr = np.array([0, len(cell["types"])], np.int32)
    lattice = np.asarray(cell["lattice"], np.float64).reshape(1, 9)
    s = new_state(cell_ptr, CU.wrap(cell["frac"]), fire, max_steps)
    frac_trace = np.full((max_steps + 1, len(cell["types"]), 3), np.nan)
    while not s["done"][0]:
        rc, e = EU.host(L, [dict(case, cell=dict(cell, frac=s["frac"].copy()))])
        assert rc == 0, L.egnn_last_error()
        frac_trace[s["counters"][0, 1]] = s["frac"]
        branch = step_restated(s, cell_ptr, lattice, e["force"], e["energy"], e["coincident"], fire, f_max, max_steps, skin)
        assert branch != ["frozen"], "the restated loop holds no list: choose a skin that never rebuilds"
    return dict(frac_trace=frac_trace, energy_trace=s["energy_trace"][:, 0], steps=int(s["counters"][0, 1]), frac=s["frac"], energy=s["scalars"][0, 2],
                status=int(s["counters"][0, 2]))


def compressed_rocksalt(a, seed):
    """the rocksalt model in a cell compressed to edge ``a`` (5.64 A at rest), the atoms displaced by default_rng(seed).uniform(-0.3,
    0.3) A: forces of hundreds of eV / A, so that the cap on the move is active for many steps"""
    ideal = EU.nacl_cell(a)
    cell = dict(ideal, frac=ideal["frac"] + np.random.default_rng(seed).uniform(-0.3, 0.3, (8, 3)) / a)
    return EU.make_case(cell, (1.0, -1.0), rocksalt_tables(), r_cut=6.0, short_cut=6.0, accuracy=1e-8, kappa=EU.KAPPA)


# ---- held rows at moved coordinates (tests/test_gpu_cell_relax_held.py, checked without a GPU in tests/test_cell_relax_host.py) ------------
# A held case: a cell with wrapped reference coordinates w0, the rows of the box walk at r_cut + skin on w0 (tests/_cell_soap_util.sites:
# no device search), and the coordinates an evaluation reads, u = w0 + delta L^-1, every |delta_i| <= skin / 2: the bound of the freeze
# rule and no more.  The truth is EU.exact on frac = u (it wraps) with k_max below the shortest reciprocal vector: no vector, so its
# force is the real-space force and its components 0 and 4 are what egnn_cell_relax_real writes.  alpha * r_cut <= 3 and shift=False:
# a site too many or too few at the cutoff moves an atom's energy by erfc(3) / r_cut of a term, ten orders above the bar.
HELD_ALPHA = 0.7            # 0.7 x 4.11 A, the largest r_cut of a case, is 2.88
HELD_CHARGES = (-1.1, 2.3)
HELD_ROWS = (1, 63, 64, 65, 129)


def held_tables():
    """the tables of the thin lattice-energy fixture without the D / r^n term and with C / 1000 (tests/test_gpu_cell_ewald.soft_tables):
    the atoms of the small cells come as close as 0.2 A"""
    pot = EU.generic_tables(2, 1)
    pot[2], pot[3] = pot[2] / 1000.0, 0.0
    return pot


def thin8():
    """8 atoms in the thin triclinic lattice (widths 1.14 / 4.74 / 3.1 A), wrapped: small_cell() of tests/test_gpu_cell_ewald.py"""
    from tests import _cell_soap_util as CSU
    rng = np.random.default_rng(21)
    frac, types = rng.uniform(-0.5, 1.5, (8, 3)), rng.integers(0, 2, 8).astype(np.int32)
    return dict(lattice=CSU.thin_cell()["lattice"], frac=CU.wrap(frac), types=types, A=2, name="thin8")


def k_below_vectors(L):
    """half the length of the shortest reciprocal vector: a k_max with no vector below it"""
    from tests import _sq_util as SQU
    hkl, k2 = SQU.box_candidates(L, float(np.sqrt((SQU.reciprocal(L) ** 2).sum(1)).max()))
    return 0.5 * float(np.sqrt(k2[SQU.half_space(hkl)].min()))


def held_moves(n, skin, seed=3, still=(0,), part=(1,)):
    """Cartesian moves [n, 3] in random directions: 0.999 * skin / 2 long, but 0 for the atoms ``still`` and 0.3 * skin / 2 for ``part``"""
    g = np.random.default_rng(seed).normal(size=(n, 3))
    length = np.full(n, 0.999 * (skin / 2))
    length[[k for k in still if k < n]] = 0.0
    length[[k for k in part if k < n]] = 0.3 * (skin / 2)
    return g / np.sqrt((g * g).sum(1))[:, None] * length[:, None]


def held_case(ref, delta, r_cut, skin, u=None, charges=HELD_CHARGES, alpha=HELD_ALPHA):
    """``ref``: a cell dict with wrapped coordinates -> dict(case: the model on the cell at u = w0 + delta L^-1 (or ``u`` as given), ref,
    skin, delta)"""
    L = np.asarray(ref["lattice"], np.float64)
    assert np.array_equal(CU.wrap(ref["frac"]), ref["frac"]) and float(np.sqrt((delta * delta).sum(1)).max()) <= skin / 2
    if u is None:
        u = ref["frac"] + delta @ np.linalg.inv(L)
    case = EU.make_case(dict(ref, frac=np.ascontiguousarray(u)), charges, held_tables(), r_cut=r_cut, short_cut=r_cut, shift=False, alpha=alpha,
                        k_max=k_below_vectors(L))
    assert case["alpha"] * case["r_cut"] <= 3.0
    return dict(case=case, ref=ref, skin=float(skin), delta=delta)


def cut_for_kept_row(ref, u, length, most=4.5):
    """the midpoint rule of tests/test_gpu_cell_ewald.cut_for_row on the site distances AT u: a radius at which the first centre whose
    two distances differ has exactly ``length`` sites now"""
    from tests import _cell_soap_util as CSU
    cell = dict(ref, frac=u)
    for centre in range(len(ref["types"])):
        d = np.sort(np.sqrt(EU._norm2(CSU.sites(cell, most, centre)[2])))
        if d[length] - d[length - 1] > 1e-6:
            return float(0.5 * (d[length - 1] + d[length]))
    raise AssertionError(f"no centre with a row of {length} sites")


def _thin_case(length=None, r_cut=None, skin=0.5):
    ref = thin8()
    delta = held_moves(8, skin)
    if r_cut is None:
        r_cut = cut_for_kept_row(ref, ref["frac"] + delta @ np.linalg.inv(ref["lattice"]), length)
    return held_case(ref, delta, r_cut, skin)


def _outside_case():
    """the one-atom cube of edge 3 A at r_cut = 2.99 A: the six images of the held row lie at 3 A whatever the atom does"""
    ref = dict(EU.cube_cell(), A=2)
    return held_case(ref, held_moves(1, 0.5, still=(), part=()), 2.99, 0.5)


def _limit_case(r_cut=3.0, skin=1.0):
    """the limit of the completeness argument in a cube of 10 A: atoms 0 and 1 stand r_cut + skin - 1e-3 apart along x and move
    skin / 2 - 1e-4 each towards the other (the outermost entry of the held row counts now); atoms 2 and 3 stand r_cut - skin + 1e-3
    apart along y and move apart by the same (the entry no longer counts)"""
    x = np.array([[1.0, 2.0, 2.0], [1.0 + (r_cut + skin - 1e-3), 2.0, 2.0], [7.0, 5.0, 7.0], [7.0, 5.0 + (r_cut - skin + 1e-3), 7.0]])
    ref = dict(lattice=10.0 * np.eye(3), frac=x / 10.0, types=np.array([0, 1, 0, 1], np.int32), A=2, name="limit")
    m = skin / 2 - 1e-4
    delta = np.array([[m, 0.0, 0.0], [-m, 0.0, 0.0], [0.0, -m, 0.0], [0.0, m, 0.0]])
    return held_case(ref, delta, r_cut, skin)


def _face_case():
    """a cube of 4 A at r_cut = 4.5 A (every atom sees its own images at 4 A): atom 0 at x = 0.97 moves 0.999 * skin / 2 along +x to
    u_x = 1.03 > 1; atom 1, its neighbour across that face, does not move; atom 2 moves at random"""
    ref = dict(lattice=4.0 * np.eye(3), frac=np.array([[0.97, 0.5, 0.5], [0.3, 0.4, 0.6], [0.6, 0.9, 0.1]]), types=np.array([0, 1, 1], np.int32),
               A=2, name="face")
    delta = held_moves(3, 0.5, still=(1,), part=())
    delta[0] = [0.999 * 0.25, 0.0, 0.0]
    return held_case(ref, delta, 4.5, 0.5, alpha=0.6)


def _pair_cell(frac):
    return dict(lattice=4.0 * np.eye(3), frac=np.asarray(frac, np.float64), types=np.array([0, 1], np.int32), A=2, name="pair")


def _pair_case(skin=0.5, r_cut=3.2):
    """two atoms in a cube of 4 A, both moved"""
    return held_case(_pair_cell([[0.1, 0.2, 0.3], [0.45, 0.5, 0.6]]), held_moves(2, skin, seed=4, still=(), part=(1,)), r_cut, skin)


def _coincide_case(skin=0.5, r_cut=3.2):
    """a cube of 4 A (a power of two: the coordinates below are exact): the atoms stand 0.25 A apart along x at the build and move
    0.125 A each, to u_0 == u_1 exactly"""
    ref = _pair_cell([[0.25, 0.5, 0.75], [0.3125, 0.5, 0.75]])
    delta = np.array([[0.125, 0.0, 0.0], [-0.125, 0.0, 0.0]])
    return held_case(ref, delta, r_cut, skin, u=np.array([[0.28125, 0.5, 0.75], [0.28125, 0.5, 0.75]]))


def _single_case(skin=0.5, r_cut=3.2):
    """the one-atom cube of edge 3 A under the model of the thin case: the second cell of no pair in the batch"""
    return held_case(dict(EU.cube_cell(), A=2), held_moves(1, skin, seed=6, still=(), part=()), r_cut, skin)


# 129 kept sites need r_cut = 4.1 A: a skin of 0.4 A keeps r_cut + skin within 4.55 A, four widths of the thin lattice
HELD_CASES = {f"row{n}": functools.partial(_thin_case, n, skin=0.4 if n == 129 else 0.5) for n in HELD_ROWS}
HELD_CASES.update(thin=functools.partial(_thin_case, r_cut=3.2), three=functools.partial(_thin_case, r_cut=3.0, skin=1.5), outside=_outside_case,
                  limit=_limit_case, face=_face_case, pair=_pair_case, single=_single_case)
# the cases in every row of which an entry has entered r_cut since the build and another has left it
HELD_MOVED = ("row63", "row64", "row65", "row129", "thin", "three")


@functools.lru_cache(maxsize=None)
def held(name):
    """the held case of a name: built once, never changed"""
    return _coincide_case() if name == "coincide" else HELD_CASES[name]()


def held_rows(hs):
    """the rows of a batch of held cases at r_cut + skin on the reference coordinates, by the box walk -> (row_ptr, atom, code) int32"""
    from tests import _cell_soap_util as CSU
    N = sum(len(h["ref"]["types"]) for h in hs)
    return CSU.site_lists([h["ref"] for h in hs], hs[0]["case"]["r_cut"] + hs[0]["skin"], np.arange(N))[:3]


def held_retest(h):
    """the re-test in numpy, per centre: (atom [P], shift [P, 3], inside r_cut now [P], inside r_cut at the build [P], vector now [P, 3])
    over the P entries of its held row"""
    from tests import _cell_soap_util as CSU
    case, ref = h["case"], h["ref"]
    L, u, cut2 = np.asarray(ref["lattice"], np.float64), case["cell"]["frac"], case["r_cut"] * case["r_cut"]
    out = []
    for i in range(len(ref["types"])):
        j, code, r0 = CSU.sites(ref, case["r_cut"] + h["skin"], i)
        s = CU.shift_decode(code)
        d = CU.site_vectors(u[j], u[i], s, L)
        out.append((j, s, EU._norm2(d) < cut2, EU._norm2(r0) < cut2, d))
    return out


def truth_rows_as_held(h, ex):
    """the rows of the truth (named by the wrapped u) in the names of the held rows: site (j, s') of centre i about the wrapped
    coordinates is (j, s' - floor(u_j) + floor(u_i)) about u -> per centre a set of (atom, s_x, s_y, s_z)"""
    u = h["case"]["cell"]["frac"]
    n = np.rint(u - CU.wrap(u)).astype(np.int64)
    out = []
    for i in range(len(u)):
        lo, hi = int(ex["row_ptr"][i]), int(ex["row_ptr"][i + 1])
        j = ex["atom"][lo:hi].astype(np.int64)
        s = CU.shift_decode(ex["code"][lo:hi]) - n[j] + n[i]
        out.append({(int(a), *map(int, b)) for a, b in zip(j, s)})
    return out


def held_error(got, want):
    """tests/_cell_ewald_util.error restricted to what egnn_cell_relax_real writes: ``got`` [N, 5] = (e_real, e_short, F) per atom against
    components 0 and 4 and the force of ``want`` (from EU.exact without a vector), over the same scales"""
    se, sf = want["scale_e"], want["scale_f"]
    diff = np.abs(got[:, 2:] - want["force"])
    parts = [np.abs(got[:, 0] - want["comp_atom"][:, 0]) / se, np.abs(got[:, 1] - want["comp_atom"][:, 4]) / se,
             np.where(sf > 0.0, diff / np.where(sf > 0.0, sf, 1.0), np.where(diff == 0.0, 0.0, np.inf)).reshape(-1)]
    return max(float(p.max(initial=0.0)) for p in parts)


def as_real(e):
    """(e_real, e_short, F) [N, 5] of the outputs of a lattice-energy evaluation"""
    return np.concatenate([e["comp_atom"][:, [0, 4]], e["force"]], 1)


@functools.lru_cache(maxsize=None)
def held_truth(name):
    """-> (EU.exact on the wrapped u, E_host: egnn_cell_ewald_host on the same case under ``held_error``); computed once"""
    from diffusion_model_amd import _lib
    case = held(name)["case"]
    ex = EU.exact(case)
    rc, e = EU.host(_lib.lib(), [case])
    assert rc == 0, _lib.lib().egnn_last_error()
    assert not len(ex["hkl"]) and e["n_vectors"].tolist() == [0]
    return ex, held_error(as_real(e), ex)


def scales(case):
    """-> (scale_e [N], scale_f [N, 3]): the error scales of EU.exact, the sums of the absolute values of the elementary terms of an
    atom's energy and of each force component, in fp64 (a yardstick: fp64 is enough for it) for a cell too large for 50 digits"""
    from tests import _cell_soap_util as CSU
    cell, A = case["cell"], case["cell"]["A"]
    t, w = np.asarray(cell["types"]), CU.wrap(cell["frac"])
    q, kap, al, pot = case["charges"][t], case["kappa"], case["alpha"], case["pot"]
    N, V, uc = len(t), EU.volume(cell["lattice"]), EU.u_cut(case)
    se, sf = np.zeros(N), np.zeros((N, 3))
    for i in range(N):
        j, _, d = CSU.sites(cell, case["r_cut"], i)
        r = np.sqrt(EU._norm2(d))
        ec = np.vectorize(math.erfc)(al * r) / r
        a = np.abs(kap * q[i] * q[j] * ec / 2)
        fr = np.abs(kap * q[i] * q[j] * (ec + EU.TWO_OVER_SQRT_PI * al * np.exp(-(al * r) ** 2)) / (r * r))
        b, fs = np.zeros(len(r)), np.zeros(len(r))
        if pot is not None:
            ab = int(t[i]) * A + t[j]
            pa, pb, pc, pd = (pot[k].reshape(-1)[ab] for k in range(4))
            n, short = case["n"], r < case["short_cut"]
            u = pa * np.exp(-pb * r) - pc / r ** 6 + pd / r ** n
            du = -pa * pb * np.exp(-pb * r) + 6 * pc / r ** 7 - n * pd / r ** (n + 1)
            b, fs = np.where(short, np.abs(u - uc[ab]) / 2, 0.0), np.where(short, np.abs(du / r), 0.0)
        se[i] = (a + b).sum()
        sf[i] = ((fr + fs)[:, None] * np.abs(d)).sum(0)
    hkl, kv, k2 = EU.vectors(case)
    if len(hkl):
        g = np.exp(-k2 / (4 * al * al)) / k2
        ph = 2 * np.pi * (w @ hkl.T.astype(np.float64))
        c, s, aq, pre = np.abs(np.cos(ph)), np.abs(np.sin(ph)), np.abs(q), 4 * np.pi * kap / V * np.abs(q)
        Cs, Ss = aq @ c, aq @ s
        se += pre * ((c * g) @ Cs + (s * g) @ Ss)
        sf += 2 * pre[:, None] * ((g * (s * Cs + c * Ss)) @ np.abs(kv))
    Q = float(q.sum())
    se += np.abs(kap * al * q * q / math.sqrt(math.pi)) + np.abs(kap * math.pi * q * Q / (2 * al * al * V))
    return se, sf


def cristobalite192():
    """192 atoms of displaced beta-cristobalite 2 x 2 x 2 under BKS at r_cut = 4 A: the case of test_the_grid_search_holds_the_same_lists"""
    from tests import _cell_grid_util as GU
    cell = GU.displaced_cristobalite(2)
    cell = dict(cell, frac=cell["frac"] + np.random.default_rng(9).uniform(-0.08, 0.08, cell["frac"].shape) / 14.32)
    return EU.make_case(cell, EU.BKS_CHARGES, EU.bks_tables(), r_cut=4.0, short_cut=4.0, accuracy=1e-3)
