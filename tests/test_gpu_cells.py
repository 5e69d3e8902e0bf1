"""Local environments of periodic cells on the device (csrc/cells/cell_env.hip through diffusion_model_amd.cells) against the host
statement egnn_cell_env_host, which tests/test_cells_host.py pins to the numpy restatement without a GPU:

  * bond lists and environments of ALL centres, 1-4 shells, of one batch of chain + cristobalite + triclinic + 65- + 160-atom +
    one-atom cells, and of a ~1,100-atom cell that crosses the 1024-atom chunk, equal the host statement bitwise -- row pointers,
    neighbours, shifts, sizes, atoms, types and the float32 positions -- and a second call equals the first bitwise;
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
