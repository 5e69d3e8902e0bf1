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
    every input and on mixed batches, fractional coordinates outside [0, 1) included; so it does in the dense regime the device
    tests rest on (dense_cells of tests/_cells_util.py: 700-1,000-site environments, frontiers of several hundred sites, 32 bonds
    per atom, shifts of +-4, the sentinel at a size of 729 / 993 / 1,233 sites), whose reach is asserted from the restatement;
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
def _assert_host_equals_restatement(cells, centres=None, shells=2, cutoff=CU.CUTOFF, max_atoms=256, want=None):
    """a centre whose restated environment exceeds ``max_atoms`` must show the sentinel max_atoms + 1 and no row; ``want``: the
    restatement of these centres where the caller has it already"""
    rc, got = CU.host_environments(_lib.lib(), cells, centres=centres, shells=shells, cutoff=cutoff, max_atoms=max_atoms)
    assert rc == 0, _lib.lib().egnn_last_error()
    want = dict(CU.restated_environments(cells, centres=centres, shells=shells) if want is None else want)
    assert all(c["cutoff"] == cutoff for c in cells)                       # the restated bond lists are those of this cutoff
    fits = np.repeat(want["size"] <= max_atoms, want["size"])
    want["size"] = np.where(want["size"] <= max_atoms, want["size"], max_atoms + 1).astype(np.int32)
    for k in ("atom", "shift", "type", "pos"):
        want[k] = want[k][fits]
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


# ---- the dense regime: environments, frontiers and bond rows beyond one wavefront ---------------------------------------------------
def test_dense_cells_reach_the_regime():
    """what the device tests of this regime rest on, from restatement (i) alone: an input that stops reaching it fails here"""
    cs = CU.dense_cells()
    deg = {k: np.diff(c["bonds"][0]) for k, c in cs.items()}
    assert len(cs["g80"]["frac"]) == 80 and deg["g80"].min() >= 24 and deg["g80"].max() <= 32      # past the 64-centre tile and the 64-lane block
    assert len(cs["g22"]["frac"]) == 22 and deg["g22"].min() >= 24 and deg["g22"].max() <= 32
    assert len(cs["g27"]["frac"]) == 27 and np.all(deg["g27"] == 32)                               # the ring search's degree limit, not beyond
    assert np.all(deg["ladder"] == 8) and np.all(deg["zincblende"] == 4)
    assert np.all(np.abs(CU.widths(cs["zincblende"]["lattice"]) - 2.6 * np.sqrt(2.0 / 3.0)) < 1e-12) and cs["zincblende"]["frac"].min() < 0.0
    # bond rows: the 80-atom cell's rows hold atoms of both 64-lane blocks; in the 27-atom cell one atom bonds through several images
    rp, at, _, _ = cs["g80"]["bonds"]
    both = [i for i in range(80) if np.sum(at[rp[i]:rp[i + 1]] < 64) >= 8 and np.sum(at[rp[i]:rp[i + 1]] >= 64) >= 8]
    assert len(both) >= 32 and min(both) < 64 <= max(both)                  # rows carried across the lane blocks, in both centre tiles
    rp, at, _, _ = cs["g27"]["bonds"]
    assert max(np.bincount(at[rp[i]:rp[i + 1]]).max() for i in range(27)) >= 2
    rp, at, _, _ = cs["cscl"]["bonds"]
    assert at.tolist() == [1] * 8 + [0] * 8 and rp.tolist() == [0, 8, 16]                    # eight images of ONE atom: eight bits in one lane
    reach = {k: CU.dense_reach(k, 4) for k in cs}
    assert reach["g80"]["sizes"].min() > 512 and reach["g80"]["sizes"].max() <= 1024 and reach["g80"]["frontier"].min() > 64
    assert reach["g22"]["sizes"].min() > 960 and reach["g22"]["sizes"].max() <= 1024 and reach["g22"]["frontier"].min() > 256
    assert np.all(reach["g27"]["sizes"] == reach["g27"]["sizes"][0]) and reach["g27"]["sizes"][0] > 1024
    assert reach["g80"]["max_shift"] == 2 and reach["g22"]["max_shift"] == 3 and reach["g27"]["max_shift"] == 3
    assert reach["ladder"]["sizes"].tolist() == [33] * 5 and reach["ladder"]["max_shift"] == 4 and reach["zincblende"]["sizes"].tolist() == [83] * 2
    env = reach["ladder"]["env"]
    sx = CU.shift_decode(env["shift"])[:, 0].reshape(5, 33)
    assert sx[0].min() == -4 and sx[0].max() == 3 and sx[4].min() == -3 and sx[4].max() == 4          # the two ends of the code range
    three = {k: CU.dense_reach(k, 3)["sizes"] for k in ("g80", "g27")}
    assert 256 < three["g80"].min() and three["g80"].max() <= 448 and np.all(three["g27"] == three["g27"][0]) and 512 < three["g27"][0] <= 960


@pytest.mark.parametrize("name", ["g80", "g22", "g27", "ladder", "zincblende", "cscl"])
@pytest.mark.parametrize("shells", [1, 2, 3, 4])
def test_host_statement_equals_the_restatement_on_dense_cells(name, shells):
    """max_atoms = 1024; the 27-atom cell at 4 shells holds more: there the sentinel and no row"""
    c = CU.dense_cells()[name]
    reach = CU.dense_reach(name, shells)
    got = _assert_host_equals_restatement([c], centres=CU.dense_centres(name), shells=shells, cutoff=c["cutoff"], max_atoms=1024, want=reach["env"])
    assert (got["size"].max() == 1025) == (name == "g27" and shells == 4)


def _dense_mixed():
    cs = CU.dense_cells()
    batch = [cs["ladder"], cs["g80"], cs["zincblende"], CU.one_atom_cell()]
    centres = np.concatenate([np.arange(5), 5 + np.arange(1, 80, 3), [85, 86, 87]])              # centres in every cell
    return batch, centres


def test_host_statement_equals_the_restatement_on_the_dense_mixed_batch():
    batch, centres = _dense_mixed()
    got = _assert_host_equals_restatement(batch, centres=centres, shells=3, max_atoms=1024)
    assert got["size"][:5].tolist() == [25] * 5 and got["size"][5:-3].min() > 256 and got["size"][-3:].tolist() == [41, 41, 1]
    _assert_host_equals_restatement(batch, centres=centres[::-1], shells=3, max_atoms=1024)


@pytest.mark.parametrize("name", ["g80", "g22"])
def test_host_statement_sentinel_at_the_largest_dense_environment(name):
    """max_atoms = the largest size fits; one less gives exactly the largest centres the sentinel and no row.  keys and seen of the
    host statement (max_atoms + 2 entries) are then at their fullest"""
    c = CU.dense_cells()[name]
    rc, full = CU.host_environments(_lib.lib(), [c], shells=4, cutoff=c["cutoff"], max_atoms=1024)
    assert rc == 0
    big = int(full["size"].max())
    largest = np.nonzero(full["size"] == big)[0]
    centres = np.concatenate([largest[:3], np.nonzero(full["size"] < big)[0][:2]])
    assert big > 704 and len(centres) >= 4
    want = CU.restated_environments([c], centres=centres, shells=4)
    assert want["size"].max() == big == want["size"][0]                                       # the restatement agrees on the size
    fit = _assert_host_equals_restatement([c], centres=centres, shells=4, cutoff=c["cutoff"], max_atoms=big, want=want)
    assert fit["size"].max() == big
    short = _assert_host_equals_restatement([c], centres=centres, shells=4, cutoff=c["cutoff"], max_atoms=big - 1, want=want)
    assert len(short["atom"]) == int(want["size"][want["size"] < big].sum()) > 0
    for g in (int(largest[0]), int(np.argmin(full["size"]))):                                 # one centre at its own size and one below
        one = CU.restated_environments([c], centres=[g], shells=4)
        s = int(one["size"][0])
        assert s == full["size"][g] > 704
        fit = _assert_host_equals_restatement([c], centres=[g], shells=4, cutoff=c["cutoff"], max_atoms=s, want=one)
        assert fit["size"].tolist() == [s] and len(fit["atom"]) == s
        short = _assert_host_equals_restatement([c], centres=[g], shells=4, cutoff=c["cutoff"], max_atoms=s - 1, want=one)
        assert short["size"].tolist() == [s] and len(short["atom"]) == 0                      # max_atoms + 1 = s: the sentinel


def test_host_statement_sentinel_beyond_1024_sites():
    c = CU.dense_cells()["g27"]
    assert np.all(CU.dense_reach("g27", 4)["sizes"] > 1024)
    rc, got = CU.host_environments(_lib.lib(), [c], shells=4, cutoff=1.6, max_atoms=1024)
    assert rc == 0 and np.all(got["size"] == 1025) and len(got["atom"]) == 0 and len(got["bond_atom"]) == 27 * 32


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
