"""Local environments of periodic cells on the device (csrc/cells/cell_env.hip through diffusion_model_amd.cells) against the host
statement egnn_cell_env_host, which tests/test_cells_host.py pins to the numpy restatement without a GPU:

  * bond lists and environments of ALL centres, 1-4 shells, of one batch of chain + cristobalite + triclinic + 65- + 160-atom +
    one-atom cells, and of a ~1,100-atom cell that crosses the 1024-atom chunk, equal the host statement bitwise -- row pointers,
    neighbours, shifts, sizes, atoms, types and the float32 positions -- and a second call equals the first bitwise.  These
    inputs stay inside one wavefront: no environment above 33 sites, no bond row above 7, max_atoms at most 256;
  * the dense regime (tests/_cells_util.py: dense_cells), every input's reach asserted from the restatement first: environments
    of 336-343 / 717-729 sites (80 atoms, 24-26 bonds each) and 972-993 sites, frontiers of 96-308 sites, i.e. several trips of the
    frontier loop and of the rank sort, max_atoms = 1024 with the dynamic-LDS limit of both kernel instantiations raised (81 KiB);
    the table sizes 2^10 / 2^11 / 2^12 and max_atoms = 960 / 961 on either side of 64 KiB; the largest environment at max_atoms =
    its size and one below (sentinel for exactly those centres), 1,233 sites against 1024 and a stop inside a frontier at
    max_atoms = 200, where a fill call leaves marked outputs untouched; a permuted centre list with duplicates; shifts of -4 and
    +4 (the ladder); eight image bits in one lane of the bond kernel (the CsCl cell); a mixed batch; 340-site graphs through the
    model, bitwise equal to the collated records;
  * centres given as a type, as a permuted index tensor with duplicates and as a subset follow the given order and equal the
    all-centres result of the same atom;
  * max_atoms = 8 on cristobalite at 2 shells (sizes are 9) raises ValueError naming cell and atom, the raw count entry returns
    the sentinel max_atoms + 1, and max_atoms = 9 succeeds;
  * .batch() of the cristobalite environments passes through a small EquivariantGNN.forward with finite output, bitwise equal to the
    forward on collate(.to_data_list(), device), and stats.structure_profile accepts the same batch.
"""
import functools

import numpy as np
import pytest
import torch

import diffusion_model_amd as dma
from diffusion_model_amd import _lib, cells as DC
from tests import _cells_util as CU
from tests._util import dims_for

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _periodic(c, id=None):
    return dma.PeriodicCell(c["lattice"], c["frac"], types=c["types"], num_types=c["A"], id=id or c["name"])


@functools.lru_cache(maxsize=None)
def _inputs(kind):
    if kind == "mixed":
        return (CU.chain_cell(), CU.cristobalite_cell(), CU.triclinic_cell(), CU.random_cell(65, 11, spread=2.0), CU.random_cell(160, 12),
                CU.one_atom_cell())
    return (CU.random_cell(1100, 13),)


@functools.lru_cache(maxsize=None)
def _host(kind, shells):
    rc, got = CU.host_environments(_lib.lib(), list(_inputs(kind)), shells=shells)
    assert rc == 0, _lib.lib().egnn_last_error()
    return got


def _device_arrays(env, cell_ptr):
    """an EnvironmentBatch in the layout of CU.host_environments (atoms counted over the whole batch)"""
    lo = torch.as_tensor(cell_ptr[:-1].astype(np.int64))[env.centre_cell]
    rows = torch.repeat_interleave(lo, torch.tensor(env.sizes, dtype=torch.int64))
    return dict(bond_ptr=env.bonds.row_ptr.cpu().numpy(), bond_atom=env.bonds.atom.cpu().numpy(), bond_shift=env.bonds.shift_code.cpu().numpy(),
                size=np.array(env.sizes, dtype=np.int32), atom=(env.atom.cpu() + rows).to(torch.int32).numpy(),
                shift=env.shift_code.cpu().numpy(), type=env.x.argmax(1).to(torch.int32).cpu().numpy(), pos=env.pos.cpu().numpy())


def _assert_bitwise(got, want):
    for k in ("bond_ptr", "bond_atom", "bond_shift", "size", "atom", "shift", "type"):
        assert got[k].dtype == np.int32 and np.array_equal(got[k], want[k]), k
    assert got["pos"].dtype == np.float32 and np.array_equal(got["pos"].view(np.int32), want["pos"].view(np.int32))


@pytest.mark.parametrize("shells", [1, 2, 3, 4])
@pytest.mark.parametrize("kind", ["mixed", "big"])
def test_device_equals_the_host_statement(kind, shells):
    cells = [_periodic(c) for c in _inputs(kind)]
    want = _host(kind, shells)
    env = dma.local_environments(cells, shells=shells, device=DEV)
    got = _device_arrays(env, want["cell_ptr"])
    _assert_bitwise(got, want)
    assert env.pos.dtype == torch.float32 and env.x.dtype == torch.int64 and env.x.shape[1] == 2 and env.exO.shape == (len(got["atom"]), 1)
    assert torch.equal(torch.nonzero(env.exO[:, 0]).reshape(-1).cpu(), env.ptr[:-1])                 # exO marks row 0 of every environment
    assert np.array_equal(env.shift.cpu().numpy(), CU.shift_decode(got["shift"]).astype(np.int32))
    again = _device_arrays(dma.local_environments(cells, shells=shells, device=DEV), want["cell_ptr"])
    _assert_bitwise(again, got)
    bonds = dma.bond_list(cells, device=DEV)
    assert torch.equal(bonds.row_ptr, env.bonds.row_ptr) and torch.equal(bonds.atom, env.bonds.atom) and torch.equal(bonds.shift_code, env.bonds.shift_code)
    if kind == "mixed":
        assert env.sizes[-1] == 1 and env.sizes[0] == (3, 5, 7, 9)[shells - 1]                      # one-atom cell; the chain


def test_centre_selection():
    cells = [_periodic(c) for c in _inputs("mixed")]
    shells = 3
    full = dma.local_environments(cells, shells=shells, device=DEV)
    N = len(full.sizes)
    types = torch.cat([c.types for c in cells])

    def rows(env, m):
        lo, hi = int(env.ptr[m]), int(env.ptr[m + 1])
        return env.pos[lo:hi], env.x[lo:hi], env.atom[lo:hi], env.shift[lo:hi], env.exO[lo:hi]

    def check(env, idx):
        assert len(env.sizes) == len(idx)
        for m, g in enumerate(idx):
            assert int(env.centre_cell[m]) == int(full.centre_cell[g]) and int(env.centre_atom[m]) == int(full.centre_atom[g])
            for a, b in zip(rows(env, m), rows(full, g)):
                assert torch.equal(a, b), (m, g)

    for t in (0, 1):
        check(dma.local_environments(cells, centres=t, shells=shells, device=DEV), torch.nonzero(types == t).reshape(-1).tolist())
    g = torch.Generator().manual_seed(3)
    perm = torch.cat([torch.randperm(N, generator=g)[:70], torch.tensor([5, 5, 0, N - 1, 5])])       # permuted, with duplicates
    check(dma.local_environments(cells, centres=perm, shells=shells, device=DEV), perm.tolist())
    subset = torch.arange(3, N, 17)
    check(dma.local_environments(cells, centres=subset.to(DEV), shells=shells, device=DEV), subset.tolist())
    with pytest.raises(ValueError, match="outside"):
        dma.local_environments(cells, centres=torch.tensor([N]), device=DEV)


def test_overflow_raises_and_the_count_entry_returns_the_sentinel():
    chain, crist = _periodic(CU.chain_cell()), _periodic(CU.cristobalite_cell())
    with pytest.raises(ValueError, match=r"cell 1, atom 0\b.*max_atoms = 8"):
        dma.local_environments([chain, crist], shells=2, max_atoms=8, device=DEV)
    env = dma.local_environments([chain, crist], shells=2, max_atoms=9, device=DEV)
    assert env.sizes == [5, 5] + [9] * 24
    cb = DC._CellBatch([chain, crist], DEV)
    bonds = DC._bond_list(cb, 2.0)
    cc = torch.tensor([[0, 0] + [1] * 24, list(range(26))], dtype=torch.int32, device=DEV)
    size = DC._env_count(cb, bonds, cc, 2, 8)                                                        # the raw count entry
    assert size.tolist() == [5, 5] + [9] * 24                                                        # max_atoms + 1 = 9: the sentinel
    size = DC._env_count(cb, bonds, cc, 4, 8)
    assert size.tolist() == [9, 9] + [9] * 24                                                        # the chain holds 9 > 8 sites at 4 shells too
    cc[0, 1] = 1                                                                                     # atom 1 is not in cell 1: the kernel's own check
    size = DC._env_count(cb, bonds, cc, 2, 256)
    assert size.tolist() == [5, 0] + [9] * 24
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        dma.local_environments([crist], device="cpu")
    with pytest.raises(_lib.EgnnError, match="cell 0 has a perpendicular width"):
        dma.bond_list(dma.PeriodicCell(np.diag([3.2, 1.9, 3.2]), [[0, 0, 0]], types=[0]), device=DEV)


def test_cells_without_atoms():
    """a batch of empty cells has an empty bond list and no environment; beside a real cell an empty one changes nothing"""
    empty = dma.PeriodicCell(5.0 * np.eye(3), np.zeros((0, 3)), types=[], num_types=2, id="empty")
    bonds = dma.bond_list([empty, empty], device=DEV)
    assert bonds.row_ptr.tolist() == [0] and bonds.num_bonds == 0
    env = dma.local_environments([empty, empty], shells=2, device=DEV)
    assert env.sizes == [] and env.pos.shape == (0, 3) and env.x.shape == (0, 2) and env.ptr.tolist() == [0]
    chain = _periodic(CU.chain_cell())
    both, alone = dma.local_environments([empty, chain, empty], shells=4, device=DEV), dma.local_environments(chain, shells=4, device=DEV)
    assert both.sizes == alone.sizes == [9, 9] and both.centre_cell.tolist() == [1, 1]
    assert torch.equal(both.pos, alone.pos) and torch.equal(both.atom, alone.atom) and torch.equal(both.shift, alone.shift)


# ---- the dense regime: frontiers, rank sorts and bond rows beyond one wavefront; the raised LDS limit -----------------------------
# Every input's reach is asserted from the restatement (CU.dense_reach; tests/test_cells_host.py holds the host statement to it on
# the same cells), so a cell that stops reaching the regime fails its precondition, not the comparison.
def _log_table(max_atoms):
    """csrc/cells/cell_env.hip, cell_log_table: the smallest power of two >= 2 (max_atoms + 64), at least 2^7"""
    lg = 7
    while (1 << lg) < 2 * (max_atoms + 64):
        lg += 1
    return lg


def _lds_bytes(max_atoms):
    """dynamic LDS of cell_env_kernel: four wavefronts x (site list + table) x 4 B"""
    return 4 * 4 * (max_atoms + 64 + (1 << _log_table(max_atoms)))


@functools.lru_cache(maxsize=None)
def _dense_host(name, shells, max_atoms=1024):
    c = CU.dense_cells()[name]
    rc, got = CU.host_environments(_lib.lib(), [c], shells=shells, cutoff=c["cutoff"], max_atoms=max_atoms)
    assert rc == 0, _lib.lib().egnn_last_error()
    return got


def _dense_device(name, shells, max_atoms=1024, centres=None):
    c = CU.dense_cells()[name]
    return dma.local_environments(_periodic(c), centres=centres, shells=shells, cutoff=c["cutoff"], max_atoms=max_atoms, device=DEV)


def _raw(name, shells, max_atoms, centres=None):
    """the arguments of the raw entries DC._env_count / egnn_cell_env_fill for one dense cell"""
    c = CU.dense_cells()[name]
    cb = DC._CellBatch([_periodic(c)], DEV)
    bonds = DC._bond_list(cb, c["cutoff"])
    ctr = torch.arange(cb.N) if centres is None else torch.as_tensor(centres)
    cc = torch.stack((torch.zeros_like(ctr), ctr)).to(torch.int32).to(DEV)
    return cb, bonds, cc


def _fill_into_marked_rows(cb, bonds, cc, shells, max_atoms, rows_each):
    """egnn_cell_env_fill into outputs of ``rows_each`` rows per centre, all marked -7 -> the four outputs"""
    M = int(cc.shape[1])
    T = M * rows_each
    env_ptr = (torch.arange(M + 1, dtype=torch.int32) * rows_each).to(DEV)
    outs = [torch.full((T,), -7, dtype=torch.int32, device=DEV) for _ in range(3)] + [torch.full((T, 3), -7.0, dtype=torch.float32, device=DEV)]
    _lib.check(_lib.lib().egnn_cell_env_fill(_lib.stream_ptr(), cb.C, cb.N, cb.A, _lib.ptr(cb.cell_ptr_h), _lib.ptr(cb.lattice_h),
                                             _lib.ptr(cb.cell_ptr), _lib.ptr(cb.lattice), _lib.ptr(cb.frac), _lib.ptr(cb.types),
                                             *DC._env_args(cb, bonds, cc, shells, max_atoms), _lib.ptr(env_ptr), T, *(_lib.ptr(t) for t in outs)))
    torch.cuda.synchronize()
    return outs


DENSE_CASES = [(n, s) for n in ("g80", "g22", "g27", "ladder", "zincblende", "cscl") for s in (1, 2, 3, 4) if (n, s) != ("g27", 4)]


@pytest.mark.parametrize("name,shells", DENSE_CASES)
def test_dense_environments_equal_the_host_statement(name, shells):
    """max_atoms = 1024: 81 KiB of dynamic LDS, so the count kernel and then the fill kernel run with their limit raised.  The
    27-atom cell at 4 shells exceeds 1024 sites: test_dense_limit_and_overflow"""
    assert _lds_bytes(1024) > 64 * 1024 and _log_table(1024) == 12
    reach = CU.dense_reach(name, shells)
    if name in ("g80", "g22", "g27") and shells >= 3:
        assert reach["frontier"].max() > 64 and reach["sizes"].max() > 64 and reach["sizes"].min() > 256      # loops of several trips
    if name in ("g80", "g22") and shells == 4:
        assert reach["frontier"].min() > 192 and reach["sizes"].min() > 704
    if name == "cscl":
        assert CU.dense_cells()[name]["bonds"][1].tolist() == [1] * 8 + [0] * 8        # one lane of the bond kernel sets eight image bits
    want = _dense_host(name, shells)
    assert np.array_equal(want["size"][CU.dense_centres(name)], reach["sizes"])                               # the restatement's sizes
    env = _dense_device(name, shells)
    got = _device_arrays(env, want["cell_ptr"])
    _assert_bitwise(got, want)
    assert np.array_equal(env.shift.cpu().numpy(), CU.shift_decode(got["shift"]).astype(np.int32))
    _assert_bitwise(_device_arrays(_dense_device(name, shells), want["cell_ptr"]), got)                       # a second call, bitwise


@pytest.mark.parametrize("max_atoms,shells,log_table,raised", [(729, 4, 11, False), (448, 3, 10, False), (512, 3, 11, False),
                                                               (960, 4, 11, False), (961, 4, 12, True)])
def test_dense_table_geometry(max_atoms, shells, log_table, raised):
    """the 80-atom cell at the table sizes on either side of a doubling and of the 64 KiB boundary of the dynamic LDS"""
    assert _log_table(max_atoms) == log_table and (_lds_bytes(max_atoms) > 64 * 1024) == raised
    reach = CU.dense_reach("g80", shells)
    assert reach["frontier"].max() > 64 and 256 < reach["sizes"].min() and reach["sizes"].max() <= max_atoms
    want = _dense_host("g80", shells, max_atoms)
    assert want["size"].max() <= max_atoms
    _assert_bitwise(_device_arrays(_dense_device("g80", shells, max_atoms), want["cell_ptr"]), want)


def test_dense_limit_and_overflow():
    # the 22-atom cell: its largest environments fit exactly; one site less and exactly those centres overflow
    full = _dense_host("g22", 4)
    big = int(full["size"].max())
    largest = np.nonzero(full["size"] == big)[0]
    assert 960 < big <= 1024 and 0 < len(largest) < 22 and CU.dense_reach("g22", 4)["sizes"].min() > 960
    _assert_bitwise(_device_arrays(_dense_device("g22", 4, big), full["cell_ptr"]), _dense_host("g22", 4, big))
    cb, bonds, cc = _raw("g22", 4, big - 1)
    size = DC._env_count(cb, bonds, cc, 4, big - 1).cpu().numpy()
    assert np.array_equal(size, _dense_host("g22", 4, big - 1)["size"]) and np.array_equal(np.nonzero(size == big)[0], largest)
    assert np.array_equal(size[size < big], full["size"][full["size"] < big])
    with pytest.raises(ValueError, match=rf"cell 0, atom {int(largest[0])}\b.*max_atoms = {big - 1} sites \({len(largest)} such"):
        _dense_device("g22", 4, big - 1)
    # the 27-atom cell holds more than 1024 sites about every centre: the sentinel, and a fill call that writes nothing
    assert np.all(CU.dense_reach("g27", 4)["sizes"] > 1024)
    cb, bonds, cc = _raw("g27", 4, 1024)
    assert DC._env_count(cb, bonds, cc, 4, 1024).tolist() == [1025] * 27 == _dense_host("g27", 4)["size"].tolist()
    for out in _fill_into_marked_rows(cb, bonds, cc, 4, 1024, rows_each=8):
        assert bool((out == -7).all())
    with pytest.raises(ValueError, match=r"cell 0, atom 0\b.*max_atoms = 1024 sites \(27 such"):
        _dense_device("g27", 4)
    # max_atoms = 200 on the 80-atom cell: 2 shells fit, the third stops inside a frontier of more than 64 sites
    assert CU.dense_reach("g80", 2)["sizes"].max() <= 200 < CU.dense_reach("g80", 3)["sizes"].min() and CU.dense_reach("g80", 3)["frontier"].min() > 64
    cb, bonds, cc = _raw("g80", 4, 200)
    assert DC._env_count(cb, bonds, cc, 4, 200).tolist() == [201] * 80 == _dense_host("g80", 4, 200)["size"].tolist()
    for out in _fill_into_marked_rows(cb, bonds, cc, 4, 200, rows_each=4):
        assert bool((out == -7).all())


def test_dense_centre_order():
    """a permuted centre list with duplicates: the four wavefronts of a workgroup run 700-site searches side by side in their
    slices of the LDS, in another grouping than the all-centres call"""
    assert CU.dense_reach("g80", 4)["sizes"].min() > 704
    g = torch.Generator().manual_seed(4)
    perm = torch.cat([torch.randperm(80, generator=g)[:37], torch.tensor([79, 79, 0, 79, 3, 0])])
    c = CU.dense_cells()["g80"]
    rc, want = CU.host_environments(_lib.lib(), [c], centres=perm.numpy(), shells=4, max_atoms=1024)
    assert rc == 0
    env = _dense_device("g80", 4, centres=perm)
    _assert_bitwise(_device_arrays(env, want["cell_ptr"]), want)
    full = _dense_device("g80", 4)
    for m, a in enumerate(perm.tolist()):
        lo, hi, flo, fhi = int(env.ptr[m]), int(env.ptr[m + 1]), int(full.ptr[a]), int(full.ptr[a + 1])
        assert int(env.centre_atom[m]) == a and hi - lo == fhi - flo
        for x, y in ((env.pos, full.pos), (env.atom, full.atom), (env.shift_code, full.shift_code), (env.x, full.x)):
            assert torch.equal(x[lo:hi], y[flo:fhi]), (m, a)


def test_dense_shift_codes_reach_both_ends():
    assert CU.dense_reach("ladder", 4)["max_shift"] == 4
    env = _dense_device("ladder", 4)
    sx = env.shift[:, 0].cpu().reshape(5, 33)
    assert sx[0].min() == -4 and sx[4].max() == 4 and int(env.shift[:, 1:].abs().max()) == 0
    assert int(env.shift_code.min()) == 40 and int(env.shift_code.max()) == 688                    # codes of (-4, 0, 0) and (4, 0, 0)
    _assert_bitwise(_device_arrays(env, _dense_host("ladder", 4)["cell_ptr"]), _dense_host("ladder", 4))


def test_dense_mixed_batch():
    cs = CU.dense_cells()
    batch = [cs["ladder"], cs["g80"], cs["zincblende"], CU.one_atom_cell()]
    centres = np.concatenate([np.arange(5), 5 + np.arange(1, 80, 3), [85, 86, 87]])
    assert CU.dense_reach("g80", 3)["sizes"].min() > 256 and CU.dense_reach("g80", 3)["frontier"].max() > 64
    cells = [_periodic(c) for c in batch]
    for ctr in (centres, centres[::-1].copy(), None):
        rc, want = CU.host_environments(_lib.lib(), batch, centres=ctr, shells=3, max_atoms=1024)
        assert rc == 0
        env = dma.local_environments(cells, centres=None if ctr is None else torch.from_numpy(ctr), shells=3, max_atoms=1024, device=DEV)
        _assert_bitwise(_device_arrays(env, want["cell_ptr"]), want)
    assert env.sizes[:5] == [25] * 5 and env.sizes[-3:] == [41, 41, 1] and min(env.sizes[5:85]) > 256


def test_dense_environments_compose_with_the_model():
    """340-site graphs (3 shells of the 80-atom cell) through the small EquivariantGNN: finite, and bitwise what the collated
    records give"""
    centres = torch.tensor([0, 13, 26, 39, 52, 65, 78, 41])
    env = _dense_device("g80", 3, 512, centres=centres)
    assert min(env.sizes) > 256 and CU.dense_reach("g80", 3)["sizes"].min() > 256
    batch = env.batch()
    assert batch.num_graphs == 8 and batch.sizes == env.sizes and batch.fully_connected
    H = 36
    torch.manual_seed(0)
    net = dma.EquivariantGNN(2, **dims_for(H, 128, 256, 256, 256)).to(DEV).eval()
    g = torch.Generator().manual_seed(1)
    h = torch.randn(batch.pos.shape[0], H, generator=g).to(DEV)
    with torch.no_grad():
        h1, x1 = net(batch.plan(), h, batch.pos, batch=batch.batch)
        ref = dma.collate(env.to_data_list(), device=DEV)
        assert torch.equal(ref.pos, batch.pos) and torch.equal(ref.x, batch.x) and torch.equal(ref.exO, batch.exO)
        assert torch.equal(ref.edge_index, batch.edge_index) and torch.equal(ref.batch, batch.batch)
        h2, x2 = net(ref.plan(), h, ref.pos, batch=ref.batch)
    assert bool(torch.isfinite(h1).all()) and bool(torch.isfinite(x1).all())
    assert torch.equal(h1, h2) and torch.equal(x1, x2)


def test_environments_compose_with_the_model_and_the_statistics():
    crist = _periodic(CU.cristobalite_cell())
    env = dma.local_environments(crist, shells=2, device=DEV)
    batch = env.batch()
    assert batch.num_graphs == 24 and batch.sizes == [9] * 24 and batch.fully_connected and batch.pos.is_cuda
    H = 36
    torch.manual_seed(0)
    net = dma.EquivariantGNN(2, **dims_for(H, 128, 256, 256, 256)).to(DEV).eval()
    g = torch.Generator().manual_seed(1)
    h = torch.randn(batch.pos.shape[0], H, generator=g).to(DEV)
    with torch.no_grad():
        h1, x1 = net(batch.plan(), h, batch.pos, batch=batch.batch)
        ref = dma.collate(env.to_data_list(), device=DEV)
        assert torch.equal(ref.pos, batch.pos) and torch.equal(ref.x, batch.x) and torch.equal(ref.exO, batch.exO)
        assert torch.equal(ref.edge_index, batch.edge_index) and torch.equal(ref.batch, batch.batch)
        h2, x2 = net(ref.plan(), h, ref.pos, batch=ref.batch)
    assert bool(torch.isfinite(h1).all()) and bool(torch.isfinite(x1).all())
    assert torch.equal(h1, h2) and torch.equal(x1, x2)
    prof = dma.stats.structure_profile(batch.pos, batch.x, batch.sizes)
    assert prof.n_type.shape == (24, 2) and int(prof.n_type.sum()) == 24 * 9
    assert int(prof.cn.sum()) == 24 * 9 * 2                      # every atom once per (own type, neighbour type) row
    recs = env.to_data_list()
    assert recs[0].id == ("cristobalite", 0) and recs[0].edge_index.shape == (2, 72) and float(recs[0].exO.sum()) == 1.0
