"""Writes tests/golden/cell_stress_golden.npz: the truth of the strain derivative of the lattice energy on the five lattice-energy
fixtures (tests/_cell_ewald_util.fixtures), the truncated Ewald and pair virial sums evaluated by mpmath at 50 digits
(tests/_cell_stress_util.exact_stress) over the membership recorded in tests/golden/cell_ewald_golden.npz, rounded once to float64.

Per fixture: the cell, charges, tables and parameters (asserted equal to those of cell_ewald_golden.npz, so that its recorded
condition -- no site within 1e-9 of r_cut or short_cut, no vector within 1e-9 of k_max -- carries over); per atom and component the
six numbers D_xy in Voigt order, per atom and Voigt index the error scale, the cell sums with the summed scales, stress, pressure,
volume, and deriv_error: the analytic D against mpmath's numerical derivative of the truth's own cell energy under a symmetric
strain with the membership held, asserted below tests/_cell_stress_util.DERIV_BOUND.

Run from the repository root:  python tests/golden/make_cell_stress_golden.py
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))

from tests import _cell_ewald_util as EU    # noqa: E402
from tests import _cell_stress_util as XU   # noqa: E402


def main():
    out = {}
    for name, case in EU.fixtures().items():
        member = EU.truth(name)                       # asserts that the fixture is the one of the energy golden
        assert member["gap"] > EU.GAP, (name, float(member["gap"]))
        ex = XU.exact_stress(case, ex=member, derivative=True)
        assert ex["deriv_error"] <= XU.DERIV_BOUND, (name, "the analytic D is not the strain derivative of the energy", float(ex["deriv_error"]))
        for k in ("lattice", "frac", "types", "charges", "params"):
            out[f"{name}_{k}"] = EU.golden()[f"{name}_{k}"]
        if case["pot"] is not None:
            out[f"{name}_pot"] = case["pot"]
        for k, v in ex.items():
            out[f"{name}_{k}"] = v
        print(f"{name}: atoms {len(case['cell']['types'])}  derivative {float(ex['deriv_error']):.1e}  pressure = {float(ex['pressure']):.12g} eV/A^3  "
              f"D = {np.array2string(ex['strain'], precision=9)}")
    np.savez_compressed(XU.GOLDEN, **out)
    print("wrote", XU.GOLDEN, os.path.getsize(XU.GOLDEN), "bytes")


if __name__ == "__main__":
    main()
