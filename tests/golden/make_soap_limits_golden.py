#!/usr/bin/env python3
"""Generate tests/golden/soap_limits_golden.npz: the SOAP power spectrum at the basis limits and at the degenerate bases
(tests/_soap_util.py: LIMIT_CONFIGS), in pure mpmath at 60 digits, by the Basis, truth, check_quadrature and check_harmonics of
make_soap_golden.py (imported, not copied).  Nothing of the package is imported.  soap_golden.npz is not touched.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_soap_limits_golden.py

Per configuration, at ITS number of types A: the tables; positions, types and centres; the truth descriptor at atom 0 of the
fixture graphs the configuration lists (1, 2, 5 and 17 atoms; 64 too at the three small bases, all seven graphs at n_max = 1,
l_max = 0); the truth coefficients at the limit configuration only.  The same three identities as make_soap_golden.py are
asserted before anything is written (beta S beta^T = 1 inside Basis; a quadrature case applies where the basis has its n and l).
Only arrays are written, through a zip writer with fixed member times, so that a second run reproduces the file byte for byte.
"""
import io
import os
import sys
import zipfile

import mpmath as mp
import numpy as np

OUT = os.path.dirname(os.path.abspath(__file__))
sys.dont_write_bytecode = True
sys.path.insert(0, os.path.dirname(os.path.dirname(OUT)))
from tests import _soap_util as SU  # noqa: E402  (fixtures only)
from tests.golden.make_soap_golden import Basis, check_harmonics, check_quadrature, truth  # noqa: E402

mp.mp.dps = 60


def save(path, arrays):
    """np.savez_compressed with every member dated 1980-01-01: np.load reads it, and equal arrays give equal bytes"""
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as z:
        for key, value in arrays.items():
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.ascontiguousarray(value), allow_pickle=False)
            info = zipfile.ZipInfo(key + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type, info.external_attr = zipfile.ZIP_DEFLATED, 0o644 << 16
            z.writestr(info, buf.getvalue())


def main():
    out = {}
    for name, cfg in SU.LIMIT_CONFIGS.items():
        basis = Basis(**SU.basis_of(cfg))
        check_quadrature(basis)
        check_harmonics(basis)
        for k, v in basis.arrays().items():
            out[f"{name}_{k}"] = v
        A = cfg["A"]
        pos, types, sizes = SU.fixture(A, cfg["graphs"])
        assert SU.gap_ok(pos, sizes, SU.neighbour_cut(cfg)), "a pair distance on the neighbour cut"
        centres = SU.first_centres(sizes)
        desc, coeff, _ = truth(basis, pos, types, sizes, A, centres, mp.mpf(float(SU.neighbour_cut(cfg))), {})
        assert desc.shape == (len(sizes), SU.features(A, cfg["n_max"], cfg["l_max"]))
        out[f"{name}_pos"], out[f"{name}_types"], out[f"{name}_centres"], out[f"{name}_desc"] = pos, types, centres.astype(np.int32), desc
        if name == "limit":
            out[f"{name}_coeff"] = coeff
        print(name, "A", A, desc.shape, coeff.shape, float(np.abs(desc).max()), "species of the largest graph:",
              sorted(set(types[centres[-1]:].tolist())))
    path = os.path.join(OUT, "soap_limits_golden.npz")
    save(path, out)
    print(path, os.path.getsize(path), "bytes")
    assert os.path.getsize(path) < 1024 * 1024


if __name__ == "__main__":
    main()
