"""Writes tests/golden/cell_ewald_golden.npz: the truth of the lattice-energy fixtures (tests/_cell_ewald_util.fixtures), the same
truncated Ewald and pair sums evaluated by mpmath at 50 digits (tests/_cell_ewald_util.exact) and rounded once to float64.

Per fixture: the cell, charges, tables and parameters; the site rows and the vectors, their membership decided at 50 digits; the
per-atom components, energies and forces, the cell sums; per atom the sum of the absolute values of the elementary terms of its
energy and of each force component (the error scale).  The script asserts that no site lies within 1e-9 (relative) of r_cut or
short_cut and no vector within 1e-9 of k_max, and that the analytic force equals mpmath's numerical derivative of the energy.

Run from the repository root:  python tests/golden/make_cell_ewald_golden.py
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))

from tests import _cell_ewald_util as EU   # noqa: E402


def main():
    out = {}
    for name, case in EU.fixtures().items():
        ex = EU.exact(case, derivative=True)
        assert ex["gap"] > EU.GAP, (name, "a site or a vector lies within the gap of a cutoff", float(ex["gap"]))
        assert ex["deriv_error"] < 1e-25, (name, "the analytic force is not the derivative of the energy", float(ex["deriv_error"]))
        cell = case["cell"]
        out[f"{name}_lattice"], out[f"{name}_frac"], out[f"{name}_types"] = cell["lattice"], cell["frac"], cell["types"]
        out[f"{name}_charges"] = case["charges"]
        if case["pot"] is not None:
            out[f"{name}_pot"] = case["pot"]
        out[f"{name}_params"] = np.array([case["kappa"], case["alpha"], case["r_cut"], case["short_cut"], case["k_max"], case["n"], case["shift"]],
                                         np.float64)
        for k, v in ex.items():
            out[f"{name}_{k}"] = v
        rows = np.diff(ex["row_ptr"])
        print(f"{name}: atoms {len(cell['types'])}  sites/atom {rows.min()}..{rows.max()}  vectors {len(ex['hkl'])}  gap {float(ex['gap']):.2e}  "
              f"derivative {float(ex['deriv_error']):.1e}  E = {float(ex['energy']):.12g}")
    np.savez_compressed(EU.GOLDEN, **out)
    print("wrote", EU.GOLDEN, os.path.getsize(EU.GOLDEN), "bytes")


if __name__ == "__main__":
    main()
