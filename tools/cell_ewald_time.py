"""Time the lattice energy of periodic cells (csrc/cells/cell_ewald.hip through cells.lattice_energy) on displaced beta-cristobalite
with BKS at r_cut = 10 A, short_cut = 5.5 A, accuracy = 1e-8, forces included:

  many-small   256 cells of 24 atoms (image box 2): 6,144 atoms;
  x5           one 3,000-atom cell;
  x10          one 24,000-atom cell, the site search through the grid rows.

Whole calls on PeriodicCell objects built before the clock starts, host clock, synchronised, best of 5 alternated rounds with the
spread (max - min) reported.  Baselines:
  (a) egnn_cell_ewald_host on one thread, whole, on many-small and x5; at 24,000 atoms it is SCALED from x5 by (24,000 / 3,000)^2 =
      64 (the site walk and the reciprocal sum are both quadratic in the atoms at one density), said so in the record;
  (b) float64 torch ops on the same device tensors for the reciprocal part alone: phases by matmul, exp(i phi), the amplitudes by a
      complex matmul and the per-atom energies and forces by a second one, in chunks of vectors where [vectors, atoms] would not fit.
By device events, on prepared arrays: the four launches alone (real, amplitudes, reciprocal, finish); by the host clock the site
search.  For the three kernels that are bound by transcendental functions the record gives terms per second x fp64 VALU
instructions per term against 39.3e12 lane-instructions per second (256 CUs x 4 SIMDs x 16 fp64 lanes x 2.4 GHz).  The
instructions per term were read from the disassembly of the kernels' loops (hipcc --save-temps, every instruction with an f64
suffix in the loop's basic blocks, all branches counted): FP64_PER_TERM below; they are an upper count of what a lane executes.
No time is gated: there is no earlier code to compare with.  A run without a GPU fails.

  python tools/cell_ewald_time.py                        # -> profiles/cell_ewald_time.json
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ROUNDS = 5
R_CUT, SHORT_CUT, ACCURACY = 10.0, 5.5, 1e-8
PEAK_FP64_LANE_INSTRUCTIONS = 39.3e12
# read from the gfx950 disassembly of the loops: real = site loop with erfc, exp and the pair potential; amplitude = one atom of the
# LDS loop (unrolled by two); recip = one vector with the force sums
FP64_PER_TERM = dict(real=253, amplitude=38, recip=50)


def _best(times):
    return dict(ms=round(min(times) * 1e3, 3), spread_ms=round((max(times) - min(times)) * 1e3, 3))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cell_ewald_time.json"))
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("tools/cell_ewald_time.py measures on the GPU: no device visible")
    import diffusion_model_amd as dma
    from diffusion_model_amd import _lib, cells as DC
    from tests import _cell_ewald_util as EU
    from tests import _cell_grid_util as GU

    periodic = lambda c: dma.PeriodicCell(c["lattice"], c["frac"], types=c["types"], num_types=2, id=c["name"])
    kw = dict(r_cut=R_CUT, short_cut=SHORT_CUT, accuracy=ACCURACY, device="cuda")
    BKS = DC.BKS

    def wall(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        return time.perf_counter() - t0, out

    def events(fn, reps=5):
        best = float("inf")
        for _ in range(reps):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            torch.cuda.synchronize()
            best = min(best, a.elapsed_time(b))
        return round(best, 3)

    def torch_reciprocal(cb, case, hkl_h, kv_h, k2_h):
        """the reciprocal energies and forces of a batch of cells of ONE lattice by float64 torch ops -> (e [C, n], F [C, n, 3])"""
        C, n = cb.C, cb.sizes[0]
        w = (cb.frac - torch.floor(cb.frac)).reshape(C, n, 3)
        q = torch.tensor(case["charges"], device="cuda")[cb.types.long()].reshape(C, n)
        V = abs(float(np.linalg.det(np.asarray(case["cell"]["lattice"]))))
        e, F = torch.zeros(C, n, dtype=torch.float64, device="cuda"), torch.zeros(C, n, 3, dtype=torch.float64, device="cuda")
        chunk = max(1, (1 << 26) // max(C * n, 1))
        for v0 in range(0, len(hkl_h), chunk):
            m = torch.from_numpy(hkl_h[v0:v0 + chunk].astype(np.float64)).cuda()
            kv = torch.from_numpy(kv_h[v0:v0 + chunk]).cuda()
            g = torch.from_numpy(np.exp(-k2_h[v0:v0 + chunk] / (4 * case["alpha"] ** 2)) / k2_h[v0:v0 + chunk]).cuda()
            E = torch.exp(2j * np.pi * (w @ m.T))                               # [C, n, v]
            S = torch.einsum("cnv,cn->cv", E, q.to(torch.complex128))          # the amplitudes: a complex matmul
            T = (E.conj() * (g * S)[:, None, :])                                # [C, n, v]
            e += T.real.sum(-1)
            F += -(T.imag @ kv)
        pre = 4 * np.pi * case["kappa"] / V
        return pre * q * e, 2 * pre * q[..., None] * F

    rng = np.random.default_rng(0)
    shapes = [("many-small", [GU.displaced_cristobalite(1, seed=int(s)) for s in rng.integers(0, 1 << 30, 256)], "auto", "whole"),
              ("x5", [GU.displaced_cristobalite(5)], "auto", "whole"),
              ("x10", [GU.displaced_cristobalite(10)], "grid", "scaled")]
    DC.lattice_energy(periodic(GU.displaced_cristobalite(1)), BKS.charges, BKS.potential, **kw)      # code objects loaded
    record = dict(r_cut=R_CUT, short_cut=SHORT_CUT, accuracy=ACCURACY, rounds=ROUNDS, fp64_per_term=FP64_PER_TERM,
                  peak_fp64_lane_instructions_per_s=PEAK_FP64_LANE_INSTRUCTIONS, shapes={})
    lib, host_x5_ms = _lib.lib(), None
    for name, cell_dicts, method, host_mode in shapes:
        pcs = [periodic(c) for c in cell_dicts]
        case = EU.make_case(cell_dicts[0], BKS.charges, EU.bks_tables(), r_cut=R_CUT, short_cut=SHORT_CUT, accuracy=ACCURACY)
        out = dict(cells=len(pcs), atoms=sum(len(c["frac"]) for c in cell_dicts), method=method)
        times = []
        for _ in range(ROUNDS):
            t, res = wall(lambda: DC.lattice_energy(pcs, BKS.charges, BKS.potential, method=method, **kw))
            times.append(t)
        out["call"] = _best(times)
        out["energy_per_atom_eV"] = float(res.energy.sum() / out["atoms"])
        out["max_force_eV_per_A"] = float(res.forces.abs().max())
        out["vectors"] = int(res.n_vectors.sum())
        # the parts alone, on prepared arrays
        cb = DC._CellBatch(pcs, "cuda")
        search = DC._SiteSearch(cb, R_CUT, method)
        idx_h, cell_h = DC._centres(cb, None)
        ts = []
        for _ in range(ROUNDS):
            t, (row_ptr, atom, code) = wall(lambda: search.rows(idx_h, cell_h))
            ts.append(t)
        out["site_search"] = _best(ts)
        out["sites"] = T = int(atom.shape[0])
        who = torch.cat([idx_h.to(torch.int32), torch.arange(cb.N, dtype=torch.int32)]).cuda()
        rows = (cb.N, _lib.ptr(row_ptr), T, _lib.ptr(atom), _lib.ptr(code), cb.N, _lib.ptr(who[:cb.N]), _lib.ptr(who[cb.N:]))
        q_h, pot_h = np.ascontiguousarray(case["charges"]), case["pot"]
        q_ptr, pot_ptr = _lib.host_ptr(q_h), _lib.host_ptr(pot_h)
        ew = (case["kappa"], case["alpha"], R_CUT, case["k_max"])
        real = torch.empty(cb.N, 5, dtype=torch.float64, device="cuda")
        flag = torch.zeros(cb.C, dtype=torch.int32, device="cuda")
        out["real_ms"] = events(lambda: _lib.check(lib.egnn_cell_ewald_real(*cb.args(A=True, types=True), q_ptr, pot_ptr, 24, 1, case["kappa"],
                                                                            case["alpha"], R_CUT, SHORT_CUT, case["k_max"], 1, *rows, _lib.ptr(real),
                                                                            _lib.ptr(flag))))
        vecs = DC._SqVectors(cb, case["k_max"], "k_max")
        hkl = torch.empty(max(vecs.K, 1), 3, dtype=torch.int32, device="cuda")
        table = torch.empty(max(vecs.K, 1), 5, dtype=torch.float64, device="cuda")
        rec = torch.empty(cb.N, 4, dtype=torch.float64, device="cuda")
        amp_head = cb.args(A=True, types=True, host=(_lib.ptr(vecs.plan_h), _lib.ptr(vecs.vec_ptr_h)), dev=(_lib.ptr(vecs.plan), _lib.ptr(vecs.vec_ptr)))
        out["amplitudes_ms"] = events(lambda: _lib.check(lib.egnn_cell_ewald_amplitudes(*amp_head, q_ptr, *ew, vecs.n_rows, _lib.ptr(vecs.row_ptr), vecs.K,
                                                                                        _lib.ptr(vecs.tiles), vecs.n_tiles, _lib.ptr(hkl), _lib.ptr(table))))
        rec_head = cb.args(A=True, types=True, host=(_lib.ptr(vecs.vec_ptr_h),), dev=(_lib.ptr(vecs.vec_ptr),))
        out["reciprocal_ms"] = events(lambda: _lib.check(lib.egnn_cell_ewald_recip(*rec_head, q_ptr, *ew, 1, vecs.K, _lib.ptr(hkl), _lib.ptr(table),
                                                                                   _lib.ptr(rec))))
        n_type = torch.empty(cb.C, 2, dtype=torch.int32, device="cuda")
        comp_atom, e_atom = torch.empty(cb.N, 5, dtype=torch.float64, device="cuda"), torch.empty(cb.N, dtype=torch.float64, device="cuda")
        force, comp = torch.empty(cb.N, 3, dtype=torch.float64, device="cuda"), torch.empty(cb.C, 5, dtype=torch.float64, device="cuda")
        energy = torch.empty(cb.C, dtype=torch.float64, device="cuda")
        out["finish_ms"] = events(lambda: _lib.check(lib.egnn_cell_ewald_finish(*cb.args(A=True, frac=False, types=True), q_ptr, *ew, _lib.ptr(real),
                                                                                _lib.ptr(rec), _lib.ptr(n_type), _lib.ptr(comp_atom), _lib.ptr(e_atom),
                                                                                _lib.ptr(force), _lib.ptr(comp), _lib.ptr(energy))))
        assert np.array_equal(energy.cpu().numpy(), res.energy.cpu().numpy()) and np.array_equal(force.cpu().numpy(), res.forces.cpu().numpy())
        pairs = sum(int(v) * n for v, n in zip(res.n_vectors.tolist(), cb.sizes))
        terms = dict(real=T, amplitude=pairs, recip=pairs)
        for key, ms in (("real", out["real_ms"]), ("amplitude", out["amplitudes_ms"]), ("recip", out["reciprocal_ms"])):
            rate = terms[key] / (ms * 1e-3)
            out[f"{key}_terms"] = terms[key]
            out[f"{key}_share_of_fp64_valu_peak"] = round(rate * FP64_PER_TERM[key] / PEAK_FP64_LANE_INSTRUCTIONS, 4)
        kernels = out["real_ms"] + out["amplitudes_ms"] + out["reciprocal_ms"] + out["finish_ms"]
        out["kernels_ms"] = round(kernels, 3)
        out["bound_by"] = ("the site search and the host side of the call" if out["call"]["ms"] - kernels > kernels else "the kernels")
        # (b) torch ops for the reciprocal part
        hkl_h, kv_h, k2_h = EU.vectors(case)
        ts = []
        for _ in range(ROUNDS):
            t, (te, tF) = wall(lambda: torch_reciprocal(cb, case, hkl_h, kv_h, k2_h))
            ts.append(t)
        out["torch_reciprocal"] = _best(ts)
        out["torch_reciprocal_max_energy_difference_eV"] = float((te.reshape(-1) - res.components_per_atom[:, 1]).abs().max())
        assert out["torch_reciprocal_max_energy_difference_eV"] < 1e-9
        # (a) the host statement
        if host_mode == "whole":
            t0 = time.perf_counter()
            rc, host = EU.host(lib, [dict(case, cell=c) for c in cell_dicts])
            out["host_statement_ms"] = round((time.perf_counter() - t0) * 1e3, 1)
            assert rc == 0
            out["max_energy_difference_to_host_eV"] = float(np.abs(host["e_atom"] - res.energy_per_atom.cpu().numpy()).max())
            assert out["max_energy_difference_to_host_eV"] < 1e-9 and host["n_vectors"].tolist() == res.n_vectors.tolist()
            if name == "x5":
                host_x5_ms = out["host_statement_ms"]
        else:
            out["host_statement_ms_scaled"] = round(host_x5_ms * (out["atoms"] / 3000.0) ** 2, 1)
            out["host_statement_scaled_from"] = "x5 by (atoms / 3,000)^2: the site walk and the reciprocal sum are quadratic in the atoms at one density"
        record["shapes"][name] = out
        print(name, json.dumps(out), flush=True)
    record["not_measured"] = ["hardware counters", "the host statement at 24,000 atoms (scaled from 3,000)", "cells above 24,000 atoms",
                              "other cutoffs and accuracies", "a particle-mesh reciprocal sum (none is implemented)",
                              "instructions executed per term (FP64_PER_TERM counts the loop's instructions in the disassembly, all branches)"]
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(record, f, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
