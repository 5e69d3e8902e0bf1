"""Local environments of periodic cells on the host (egnn_cell_env_host: csrc/cells/cell_host.cpp over the definitions the kernels
compile, csrc/cells/cell_math.h), without a GPU:

  * lattice_from_parameters recovers its six parameters to 1e-12 and places c on z, a in the xz-plane;
  * the infinite-lattice definition (restatement (i) of tests/_cells_util.py) gives the site sets of the reference's supercell rule
    (restatement (ii), make_dataset.py:79-111) for EVERY centre and 1-4 shells of beta-cristobalite and its triclinic distortion,
    and for every centre of a random 160-atom cell whose reference search used no bond that wraps round the supercell (at most
    10 % may); on the two-atom chain cell it gives 3 / 5 / 7 / 9 sites where the reference gives 6 at 3 and 4 shells -- the
    documented deviation ("Periodic cells");
  * positions agree with the reference's spelling float32(X_site) - float32(X_centre) within 2^-22 max|X|: two input roundings of
    2^-24 |X|, the subtraction's rounding and our own (each at most 2^-24 of a value below max|X|);
  * egnn_cell_env_host equals restatement (i) EXACTLY in every integer output and within 1 float32 ulp per position component, on
    every input and on mixed batches, fractional coordinates outside [0, 1) included;
  * bad arguments return EGNN_EINVAL with a message naming the cause, from the host statement and -- before anything is launched
    -- from the device entries;
  * the host statement runs clean under AddressSanitizer + UBSan as a stand-alone program (tests/host/cell_env_main.cpp).

No fixture executed from the reference is possible: the cell library it builds on is absent ("parity unpinned
by execution")."""
import ctypes as C
import functools

import numpy as np
import pytest

from diffusion_model_amd import _lib
from diffusion_model_amd.cells import lattice_from_parameters
from tests import _cells_util as CU
from tests._host_program import build_and_run

EINVAL = -22


@functools.lru_cache(maxsize=None)
def _cells():
    return dict(chain=CU.chain_cell(), cristobalite=CU.cristobalite_cell(), triclinic=CU.triclinic_cell(),
                r65=CU.random_cell(65, 11, spread=2.0), r160=CU.random_cell(160, 12), one=CU.one_atom_cell())


@functools.lru_cache(maxsize=None)
def _big():
    return CU.random_cell(1100, 13)


def _site_set(atom, code):
    return set((int(a),) + tuple(int(v) for v in CU.shift_decode(c)) for a, c in zip(atom, code))


# ---- lattice --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("params", [(7.3, 7.0, 7.5, 84.0, 97.0, 92.0), (7.16, 7.16, 7.16, 90.0, 90.0, 90.0), (11.0, 12.0, 10.5, 86.0, 95.0, 91.0),
                                    (5.0, 6.0, 7.0, 60.0, 70.0, 110.0)])
def test_lattice_from_parameters(params):
    L = lattice_from_parameters(*params).numpy()
    assert L.dtype == np.float64 and L.shape == (3, 3)
    a, b, c = L
    ang = lambda u, v: np.degrees(np.arccos(np.dot(u, v) / (np.linalg.norm(u) * np.linalg.norm(v))))
    got = (np.linalg.norm(a), np.linalg.norm(b), np.linalg.norm(c), ang(b, c), ang(a, c), ang(a, b))
    assert np.abs(np.array(got) - np.array(params)).max() <= 1e-12, got          # absolute: angstrom and degrees alike
    assert c[0] == 0.0 and c[1] == 0.0 and c[2] > 0.0          # c on z
    assert a[1] == 0.0 and a[0] > 0.0                           # a in the xz-plane
    assert np.dot(a, np.cross(b, c)) > 0.0                      # right-handed
    assert np.abs(L - CU.lattice_from_parameters(*params)).max() <= 1e-14


# ---- the definition against the reference rule -------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["cristobalite", "triclinic"])
def test_definition_gives_the_reference_site_sets(name):
    c = _cells()[name]
    sizes = {}
    for shells in (1, 2, 3, 4):
        for i in range(24):
            atom, code, pos = CU.environment(c["lattice"], c["frac"], c["bonds"], i, shells)
            want, wrapped, ref_pos, xmax = CU.reference_environment(c["lattice"], c["frac"], i, shells)
            assert not wrapped and _site_set(atom, code) == want, (name, shells, i)      # no centre is excluded
            sizes.setdefault(shells, set()).add(len(atom))
            for a, cd, p in zip(atom, code, pos):                                           # positions against the reference's spelling
                key = (int(a),) + tuple(int(v) for v in CU.shift_decode(cd))
                assert np.abs(p.astype(np.float64) - ref_pos[key].astype(np.float64)).max() <= 2.0 ** -22 * xmax
    assert sizes[2] == {9} and min(sizes[3]) == 15 and max(sizes[3]) == 21 and sizes[4] == {33}, sizes


def test_definition_against_the_reference_rule_on_a_random_cell():
    c = _cells()["r160"]
    excluded = compared = 0
    rows = {}
    for i in range(160):
        for shells in (1, 2, 3, 4):
            atom, code, pos = CU.environment(c["lattice"], c["frac"], c["bonds"], i, shells)
            want, wrapped, ref_pos, xmax = CU.reference_environment(c["lattice"], c["frac"], i, shells, rows=rows)
            if wrapped:
                excluded += 1
                continue
            compared += 1
            assert _site_set(atom, code) == want, (i, shells)
            for a, cd, p in zip(atom, code, pos):
                key = (int(a),) + tuple(int(v) for v in CU.shift_decode(cd))
                assert np.abs(p.astype(np.float64) - ref_pos[key].astype(np.float64)).max() <= 2.0 ** -22 * xmax
    assert excluded + compared == 4 * 160 and excluded <= 0.1 * (excluded + compared), (excluded, compared)


def test_chain_cell_is_the_documented_deviation():
    c = _cells()["chain"]
    for shells, n_sites in ((1, 3), (2, 5), (3, 7), (4, 9)):
        atom, code, _ = CU.environment(c["lattice"], c["frac"], c["bonds"], 1, shells)
        assert len(atom) == n_sites
        assert np.abs(CU.shift_decode(code)).max() == (shells + 1) // 2
        want, wrapped, _, _ = CU.reference_environment(c["lattice"], c["frac"], 1, shells)
        if shells <= 2:
            assert not wrapped and _site_set(atom, code) == want
        else:
            assert wrapped and len(want) == 6


# ---- the host statement against the restatement ----------------------------------------------------------------------------------
def _assert_host_equals_restatement(cells, centres=None, shells=2):
    rc, got = CU.host_environments(_lib.lib(), cells, centres=centres, shells=shells)
    assert rc == 0, _lib.lib().egnn_last_error()
    want = CU.restated_environments(cells, centres=centres, shells=shells)
    for k in ("bond_ptr", "bond_atom", "bond_shift", "size", "atom", "shift", "type"):
        assert got[k].dtype == np.int32 and np.array_equal(got[k], want[k]), k
    assert np.all(np.isfinite(got["pos"])) and CU.ulp_distance(got["pos"], want["pos"]).max(initial=0) <= 1
    return got


@pytest.mark.parametrize("name", ["chain", "cristobalite", "triclinic", "r65", "r160", "one"])
@pytest.mark.parametrize("shells", [1, 2, 3, 4])
def test_host_statement_equals_the_restatement(name, shells):
    got = _assert_host_equals_restatement([_cells()[name]], shells=shells)
    assert got["size"].min() >= 1 and np.all(got["shift"][np.cumsum(got["size"]) - got["size"]] == CU.CENTRE_CODE)


@pytest.mark.parametrize("shells", [1, 2, 3, 4])
def test_host_statement_equals_the_restatement_across_the_chunk(shells):
    """every centre of the ~1,100-atom cell, atoms 1023 and 1024 on either side of the 1024-atom chunk among them"""
    c = _big()
    assert len(c["frac"]) > 1024
    got = _assert_host_equals_restatement([c], shells=shells)
    assert len(got["size"]) == 1100


def test_host_statement_equals_the_restatement_on_mixed_batches():
    cs = _cells()
    assert cs["r65"]["frac"].min() < 0.0 and cs["r65"]["frac"].max() > 1.0 and cs["triclinic"]["frac"].min() < 0.0
    batch = [cs[k] for k in ("chain", "cristobalite", "triclinic", "r65", "r160", "one")]
    for shells in (1, 4):
        got = _assert_host_equals_restatement(batch, shells=shells)
        assert got["size"][-1] == 1                                       # the one-atom cell: no bond, a one-atom environment
    rng = np.random.default_rng(5)
    N = sum(len(c["frac"]) for c in batch)
    _assert_host_equals_restatement(batch, centres=rng.integers(0, N, 40), shells=3)      # any order, duplicates
    _assert_host_equals_restatement(batch[::-1], shells=2)


def test_host_statement_overflow_sentinel():
    c = _cells()["cristobalite"]
    rc, got = CU.host_environments(_lib.lib(), [c], shells=2, max_atoms=8)
    assert rc == 0 and np.all(got["size"] == 9) and len(got["atom"]) == 0          # sizes are 9: every centre exceeds 8
    rc, got = CU.host_environments(_lib.lib(), [c], shells=2, max_atoms=9)
    assert rc == 0 and np.all(got["size"] == 9) and len(got["atom"]) == 9 * 24


# ---- argument errors --------------------------------------------------------------------------------------------------------------
def test_argument_errors_return_einval():
    L = _lib.lib()
    cs = _cells()
    ok = [cs["chain"], cs["cristobalite"]]
    assert CU.host_environments(L, ok)[0] == 0

    def refused(word, cells=ok, **kw):
        assert CU.host_environments(L, cells, **kw)[0] == EINVAL, (word, kw)
        assert word in L.egnn_last_error(), (word, L.egnn_last_error())

    narrow = dict(cs["chain"], lattice=np.diag([3.2, 1.9, 3.2]))
    refused(b"cell 1 has a perpendicular width", cells=[cs["chain"], narrow])
    flat = dict(cs["chain"], lattice=np.array([[3.2, 0, 0], [0, 3.2, 0], [3.2, 3.2, 0.0]]))
    refused(b"cell 1 has a singular lattice", cells=[cs["chain"], flat])
    refused(b"shells 0", shells=0)
    refused(b"shells 5", shells=5)
    refused(b"max_atoms 0", max_atoms=0)
    refused(b"max_atoms 1025", max_atoms=1025)
    refused(b"5 atom types", A=5)
    refused(b"type 2 outside", raw=dict(type=np.full(26, 2, np.int32)))
    refused(b"outside its cell", centres=[26], centre_cell=[1])
    refused(b"outside its cell", centres=[-1], centre_cell=[0])
    refused(b"outside its cell", centres=[1], centre_cell=[1])
    refused(b"names cell", centres=[1], centre_cell=[2])
    refused(b"cutoff", cutoff=0.0)
    refused(b"cutoff", cutoff=-1.0)
    # null pointers
    cp = np.array([0, 2], np.int32)
    lat, fr, ty = np.ascontiguousarray(cs["chain"]["lattice"].reshape(1, 9)), np.ascontiguousarray(cs["chain"]["frac"]), np.zeros(2, np.int32)
    bp = np.zeros(3, np.int32)
    vp = lambda a: C.c_void_p(a.ctypes.data)
    full = [1, 2, vp(cp), vp(lat), vp(fr), vp(ty), 2.0, 0, None, None, 2, 256, vp(bp), 0, None, None, None, 0, None, None, None, None]
    assert L.egnn_cell_env_host(*full) == 0, L.egnn_last_error()
    for k in (2, 3, 4, 5, 12):
        args = list(full)
        args[k] = None
        assert L.egnn_cell_env_host(*args) == EINVAL and b"bad egnn_cell_env_host arguments" in L.egnn_last_error(), k
    args = list(full)
    args[7] = 1                                                          # a centre without its arrays
    assert L.egnn_cell_env_host(*args) == EINVAL

    # the device entries refuse the same arguments before they launch anything (no GPU is touched here)
    p = C.c_void_p(64)
    cp2 = np.array([0, 2, 4], np.int32)
    lat2 = np.ascontiguousarray(np.stack([cs["chain"]["lattice"].reshape(9), narrow["lattice"].reshape(9)]))
    lat_flat = np.ascontiguousarray(np.stack([cs["chain"]["lattice"].reshape(9), flat["lattice"].reshape(9)]))
    for lat_bad, word in ((lat2, b"cell 1 has a perpendicular width"), (lat_flat, b"cell 1 has a singular lattice")):
        assert L.egnn_cell_bonds_count(None, 2, 4, vp(cp2), vp(lat_bad), p, p, p, 2.0, p, 1, p) == EINVAL and word in L.egnn_last_error()
        assert L.egnn_cell_bonds_fill(None, 2, 4, vp(cp2), vp(lat_bad), p, p, p, 2.0, p, 1, p, 4, p, p) == EINVAL and word in L.egnn_last_error()
    assert L.egnn_cell_env_fill(None, 2, 4, 2, vp(cp2), vp(lat_flat), p, p, p, p, p, 4, p, p, 1, p, p, 2, 256, p, 4, p, p, p, p) == EINVAL
    assert b"singular" in L.egnn_last_error()
    good = np.ascontiguousarray(np.stack([cs["chain"]["lattice"].reshape(9)] * 2))
    assert L.egnn_cell_bonds_count(None, 2, 4, vp(cp2), vp(good), p, p, p, 0.0, p, 1, p) == EINVAL and b"cutoff" in L.egnn_last_error()
    assert L.egnn_cell_bonds_count(None, 2, 4, vp(cp2), vp(good), p, p, p, -2.0, p, 1, p) == EINVAL
    assert L.egnn_cell_bonds_count(None, 2, 4, None, vp(good), p, p, p, 2.0, p, 1, p) == EINVAL
    assert L.egnn_cell_bonds_count(None, 2, 4, vp(cp2), None, p, p, p, 2.0, p, 1, p) == EINVAL
    assert L.egnn_cell_bonds_count(None, 2, 4, vp(cp2), vp(good), p, p, None, 2.0, p, 1, p) == EINVAL
    assert L.egnn_cell_bonds_count(None, 2, 4, vp(cp2), vp(good), p, p, p, 2.0, None, 1, p) == EINVAL
    assert L.egnn_cell_bonds_count(None, 2, 5, vp(cp2), vp(good), p, p, p, 2.0, p, 1, p) == EINVAL and b"cell_ptr" in L.egnn_last_error()
    assert L.egnn_cell_bonds_fill(None, 2, 4, vp(cp2), vp(good), p, p, p, 2.0, p, 1, None, 4, p, p) == EINVAL
    assert L.egnn_cell_bonds_fill(None, 2, 4, vp(cp2), vp(good), p, p, p, 2.0, p, 1, p, 4, None, p) == EINVAL
    for shells, max_atoms, word in ((0, 256, b"shells 0"), (5, 256, b"shells 5"), (2, 0, b"max_atoms 0"), (2, 1025, b"max_atoms 1025")):
        assert L.egnn_cell_env_count(None, 2, 4, vp(cp2), p, p, 4, p, p, 1, p, p, shells, max_atoms, p) == EINVAL and word in L.egnn_last_error()
        assert L.egnn_cell_env_fill(None, 2, 4, 2, vp(cp2), vp(good), p, p, p, p, p, 4, p, p, 1, p, p, shells, max_atoms, p, 4, p, p, p, p) == EINVAL
        assert word in L.egnn_last_error()
    assert L.egnn_cell_env_count(None, 2, 4, vp(cp2), p, p, 4, p, p, 1, None, p, 2, 256, p) == EINVAL
    assert L.egnn_cell_env_count(None, 2, 4, vp(cp2), p, None, 4, p, p, 1, p, p, 2, 256, p) == EINVAL
    assert L.egnn_cell_env_count(None, 2, 4, vp(cp2), p, p, 4, p, p, 1, p, p, 2, 256, None) == EINVAL
    assert L.egnn_cell_env_fill(None, 2, 4, 5, vp(cp2), vp(good), p, p, p, p, p, 4, p, p, 1, p, p, 2, 256, p, 4, p, p, p, p) == EINVAL
    assert b"5 atom types" in L.egnn_last_error()
    assert L.egnn_cell_env_fill(None, 2, 4, 2, vp(cp2), vp(good), p, p, p, None, p, 4, p, p, 1, p, p, 2, 256, p, 4, p, p, p, p) == EINVAL
    assert L.egnn_cell_env_fill(None, 2, 4, 2, vp(cp2), vp(good), p, p, p, p, p, 4, p, p, 1, p, p, 2, 256, p, 4, p, p, p, None) == EINVAL


# ---- sanitizers ---------------------------------------------------------------------------------------------------------------------
def test_cell_env_host_under_sanitizers(tmp_path):
    """the executable links its own sanitizer runtime (statically), so nothing is preloaded"""
    r = build_and_run(tmp_path, "cell_env_main", ["cells/cell_host.cpp", "host_logic.cpp"])
    assert r.returncode == 0 and "CELL-ENV-OK" in r.stdout, f"rc={r.returncode}\nstdout:\n{r.stdout}\nstderr:\n{r.stderr[-4000:]}"
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]
