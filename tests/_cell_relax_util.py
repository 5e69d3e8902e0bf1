"""The relaxation of periodic cells (csrc/cells/cell_relax_math.h) for the CPU and GPU tests (test infrastructure): the rocksalt
fixture, a numpy restatement of the step in the order of the header (256 strided partial sums, then the tree 128 .. 1), a scripted
sequence of forces that reaches every branch of the step, and the ctypes wrappers of the two host statements.

  * state of a batch: a dict of the arrays the step entries take (frac, velocity, since, moved, scalars [C, 5], counters [C, 4],
    done, rebuild, energy_trace, force_trace) -- ``new_state``;
  * ``step_restated`` changes such a dict as egnn_cell_relax_step_host does and returns the branch every cell took;
  * ``rebuild_restated`` is the caller's part of a rebuild: u <- wrap(u), since <- 0, the flag cleared.
"""
import functools

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
