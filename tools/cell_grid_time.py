"""Time the linked-cell kernels of periodic cells (csrc/cells/cell_grid.hip) against the direct ones (cell_env.hip, cell_stats.hip) on
displaced beta-cristobalite 5 x 5 x 5, 10 x 10 x 10 and 20 x 20 x 20: 3,000, 24,000 and 192,000 atoms in one cell.

  bond list    cells._bond_list(cutoff 2.0), method "grid" against "direct": the whole call on an uploaded batch (grid: the grid rule,
               binning, prefix sum, sort, count, prefix sum, fill), host clock, synchronised; and the entries alone, device events
               around back-to-back launches on prepared arrays: binning (egnn_cell_grid_count / _fill with the prefix sum between)
               and the walk (egnn_cell_bonds_grid_count / _fill) against egnn_cell_bonds_count / _fill.  The grid at several
               min_width values.
  pair counts  cells._pair_counts(R = 10, dR = 0.01), "grid" at reach 1, 2 and 3 against "direct": whole calls, and the entries
               egnn_cell_pair_counts_grid / egnn_cell_pair_counts alone.

Equal outputs are asserted wherever the direct side is run.  Best of 5 alternated rounds.  The direct side at 192,000 atoms is run
ONCE, in a child process under its own time limit (--direct-limit seconds), after everything else; where it does not finish, the
record says so.  From the whole calls the record derives the threshold of method="auto" (the smallest measured size at which the
grid beats the direct call by more than the spread of the rounds, rounded up to a power of two, at least 2,048) and the knobs
(reach of the pair grid, min_width of the bond grid: the fastest whole call at 24,000 atoms).  Nothing here is an estimate: a run
without a GPU fails.

  python tools/cell_grid_time.py                        # -> profiles/cell_grid_time.json
"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

R, DR, CUTOFF = 10.0, 0.01, 2.0
REPLICAS = (5, 10, 20)
REACHES = (1, 2, 3)
MIN_WIDTHS = (0.0, 3.0, 4.0)
DIRECT_ROUNDS_UP_TO = 24000        # above this the direct side is run once, in the child


def _setup():
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("tools/cell_grid_time.py measures on the GPU: no device visible")
    import diffusion_model_amd as dma
    from diffusion_model_amd import cells as DC
    from tests import _cell_grid_util as GU
    from tests import _cell_stats_util as SU

    def batch(m):
        c = GU.displaced_cristobalite(m)
        return DC._CellBatch([dma.PeriodicCell(c["lattice"], c["frac"], types=c["types"], num_types=2, id=c["name"])], "cuda")

    return torch, DC, SU, batch


def _bonds_equal(torch, a, b):
    return torch.equal(a.row_ptr, b.row_ptr) and torch.equal(a.atom, b.atom) and torch.equal(a.shift_code, b.shift_code)


def direct_once(m):
    """the child: the direct kernels on one shape, each run once after a small warm-up, compared with the grid's outputs"""
    torch, DC, SU, batch = _setup()
    nbins = SU.nbins_of(R, DR)
    small = batch(2)
    DC._bond_list(small, CUTOFF, "direct"), DC._pair_counts(small, DR, nbins, method="direct")      # code objects loaded
    cb = batch(m)
    out = {"atoms": cb.N}
    for name, direct, grid in (("bond_list", lambda: DC._bond_list(cb, CUTOFF, "direct"), lambda: DC._bond_list(cb, CUTOFF, "grid")),
                               ("pair_counts", lambda: DC._pair_counts(cb, DR, nbins, method="direct"),
                                lambda: DC._pair_counts(cb, DR, nbins, method="grid"))):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        want = direct()
        torch.cuda.synchronize()
        out[name + "_direct_ms_once"] = round((time.perf_counter() - t0) * 1e3, 2)
        got = grid()
        out[name + "_equal"] = bool(_bonds_equal(torch, got, want) if name == "bond_list" else torch.equal(got, want))
        print("DIRECT-ONCE", json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--direct-limit", type=float, default=240.0)
    ap.add_argument("--direct-once", type=int, default=0, help="(internal) run the direct kernels once on this many replicas and print the times")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cell_grid_time.json"))
    args = ap.parse_args()
    if args.direct_once:
        return direct_once(args.direct_once)

    torch, DC, SU, batch = _setup()
    from diffusion_model_amd import _lib
    lib = _lib.lib()
    nbins = SU.nbins_of(R, DR)
    record = {"rounds": args.rounds, "warmup_calls": args.warmup, "settings": dict(R=R, dR=DR, nbins=nbins, cutoff=CUTOFF),
              "gcn_arch": torch.cuda.get_device_properties(0).gcnArchName, "shapes": {}}

    def wall(fn, calls):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(calls):
            fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3 / calls

    def events(fn, calls):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(calls):
            fn()
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b) / calls

    def bond_entries(cb, grid):
        """the walk alone on a prepared grid: count, prefix sum, fill"""
        deg = torch.zeros(cb.N, dtype=torch.int32, device=cb.dev)
        _lib.check(lib.egnn_cell_bonds_grid_count(*DC._grid_bond_args(cb, grid, CUTOFF), _lib.ptr(deg)))
        row_ptr, E = DC._row_ptr(cb, deg)
        atom, code = (torch.empty(max(E, 1), dtype=torch.int32, device=cb.dev) for _ in range(2))
        _lib.check(lib.egnn_cell_bonds_grid_fill(*DC._grid_bond_args(cb, grid, CUTOFF), _lib.ptr(row_ptr), E, _lib.ptr(atom), _lib.ptr(code)))

    def pair_entry(cb, grid, counts):
        _lib.check(lib.egnn_cell_pair_counts_grid(*grid.args(cb, A=True), _lib.ptr(grid.sorted_frac),
                                                  _lib.ptr(grid.sorted_type), DR, nbins, grid.reach, _lib.ptr(grid.tiles), grid.n_tiles,
                                                  _lib.ptr(counts)))

    for m in REPLICAS:
        cb = batch(m)
        with_direct = cb.N <= DIRECT_ROUNDS_UP_TO
        flows, checks = {}, []
        # ---- bond list ----
        for mw in MIN_WIDTHS:
            flows[f"bond_grid_w{mw:g}"] = lambda mw=mw: DC._bond_list(cb, CUTOFF, "grid", min_width=mw)
        grid_b = DC._CellGrid(cb, DC._grid_cells(cb, "grid", CUTOFF, 1, 0.0), CUTOFF, 1)
        flows["bond_binning_entries"] = lambda: DC._CellGrid(cb, grid_b.nb_h.numpy(), CUTOFF, 1)
        flows["bond_walk_entries"] = lambda: bond_entries(cb, grid_b)
        # ---- pair counts ----
        grids_p, counts = {}, torch.zeros(cb.C, cb.A, cb.A, nbins, dtype=torch.int64, device=cb.dev)
        for reach in REACHES:
            flows[f"pair_grid_m{reach}"] = lambda reach=reach: DC._pair_counts(cb, DR, nbins, method="grid", reach=reach)
            grids_p[reach] = DC._CellGrid(cb, DC._grid_cells(cb, "grid", nbins * DR, reach, 0.0), nbins * DR, reach)
            flows[f"pair_walk_entry_m{reach}"] = lambda reach=reach: pair_entry(cb, grids_p[reach], counts)
        if with_direct:
            tiles = torch.from_numpy(DC._pair_tiles(cb.sizes, DC._image_boxes(cb, DR, nbins))).to(cb.dev)
            flows["bond_direct"] = lambda: DC._bond_list(cb, CUTOFF, "direct")
            flows["pair_direct"] = lambda: DC._pair_counts(cb, DR, nbins, method="direct")
            flows["pair_direct_entry"] = lambda: DC._pair_counts(cb, DR, nbins, tiles=tiles)
            want_b, want_p = flows["bond_direct"](), flows["pair_direct"]()
            for mw in MIN_WIDTHS:
                assert _bonds_equal(torch, flows[f"bond_grid_w{mw:g}"](), want_b), (m, mw)
            for reach in REACHES:
                assert torch.equal(flows[f"pair_grid_m{reach}"](), want_p), (m, reach)
            checks.append("bond list and pair counts of every grid flow equal the direct ones")
        else:
            first_b, first_p = flows["bond_grid_w0"](), flows["pair_grid_m1"]()
            for mw in MIN_WIDTHS[1:]:
                assert _bonds_equal(torch, flows[f"bond_grid_w{mw:g}"](), first_b), (m, mw)
            for reach in REACHES[1:]:
                assert torch.equal(flows[f"pair_grid_m{reach}"](), first_p), (m, reach)
            checks.append("every grid flow equals the others; the direct side: see direct_once")
        entry = {k for k in flows if "entr" in k}
        calls = 3 if cb.N <= DIRECT_ROUNDS_UP_TO else 1
        for k, fn in flows.items():
            (events if k in entry else wall)(fn, args.warmup)
        ms = {k: [] for k in flows}
        for _ in range(args.rounds):                            # alternating
            for k, fn in flows.items():
                ms[k].append(events(fn, 2 * calls) if k in entry else wall(fn, calls))
        rec = {"atoms": cb.N, "bond_nb": {f"{mw:g}": DC._grid_cells(cb, "grid", CUTOFF, 1, mw)[0].tolist() for mw in MIN_WIDTHS},
               "pair_nb": {str(r): grids_p[r].nb_h[0].tolist() for r in REACHES}, "bonds": int(DC._bond_list(cb, CUTOFF, "grid").num_bonds),
               "pairs_counted": int(flows["pair_grid_m2"]().sum()), "checked": checks,
               "ms_rounds": {k: [round(v, 4) for v in vs] for k, vs in ms.items()}, "ms_best": {k: round(min(vs), 4) for k, vs in ms.items()},
               "ms_spread": {k: round(max(vs) - min(vs), 4) for k, vs in ms.items()}}
        record["shapes"][str(cb.N)] = rec
        print(cb.N, json.dumps(rec["ms_best"]), flush=True)
        del cb, flows, grids_p, grid_b, counts
        torch.cuda.empty_cache()

    # ---- what the measurements choose ----
    at = record["shapes"]["24000"]["ms_best"]
    record["chosen"] = {"pair_reach": min(REACHES, key=lambda r: at[f"pair_grid_m{r}"]), "bond_min_width": min(MIN_WIDTHS, key=lambda w: at[f"bond_grid_w{w:g}"])}
    wins = {}
    for stat, grid_key in (("bond_list", f"bond_grid_w{record['chosen']['bond_min_width']:g}"), ("pair_counts", f"pair_grid_m{record['chosen']['pair_reach']}")):
        direct_key = "bond_direct" if stat == "bond_list" else "pair_direct"
        wins[stat] = [int(n) for n, rec in record["shapes"].items() if direct_key in rec["ms_best"] and
                      rec["ms_best"][direct_key] - rec["ms_best"][grid_key] > max(rec["ms_spread"][direct_key], rec["ms_spread"][grid_key])]
    record["grid_wins_at"] = wins
    both = sorted(set(wins["bond_list"]) & set(wins["pair_counts"]))
    threshold = None
    if both and 24000 in both:
        threshold = 2048
        while threshold < both[0]:
            threshold *= 2
    record["chosen"]["grid_min_atoms"] = threshold
    record["note"] = ("whole calls (bond_grid_*, bond_direct, pair_grid_*, pair_direct): host clock around cells._bond_list / cells._pair_counts on an "
                      "uploaded batch, synchronised; *_entries / *_entry: device events around back-to-back calls on prepared arrays.  Best of the "
                      "alternated rounds; ms_spread = max - min over the rounds.  grid_min_atoms: the smallest measured size at which BOTH "
                      "statistics win by more than the spread, rounded up to a power of two, at least 2,048; null: the grid did not win at 24,000 "
                      "atoms and method='auto' stays direct.")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    json.dump(record, open(args.out, "w"), indent=1)
    print("wrote", args.out, json.dumps(record["chosen"]), json.dumps(wins), flush=True)

    # ---- the direct side at 192,000 atoms: once, in a fresh process, under its own limit, after everything else ----
    del torch
    once = {"limit_s": args.direct_limit}
    try:
        child = subprocess.run([sys.executable, os.path.abspath(__file__), "--direct-once", str(REPLICAS[-1])], capture_output=True, text=True,
                               timeout=args.direct_limit)
        lines = [ln for ln in child.stdout.splitlines() if ln.startswith("DIRECT-ONCE ")]
        once.update(json.loads(lines[-1][len("DIRECT-ONCE "):]) if lines else {})
        once["finished"] = child.returncode == 0
        if child.returncode != 0:
            once["stderr_tail"] = child.stderr[-400:]
    except subprocess.TimeoutExpired as e:
        lines = [ln for ln in (e.stdout or b"").decode(errors="replace").splitlines() if ln.startswith("DIRECT-ONCE ")]
        once.update(json.loads(lines[-1][len("DIRECT-ONCE "):]) if lines else {})
        once["finished"] = False
        once["note"] = f"did not finish within {args.direct_limit:g} s"
    record["direct_once_192000"] = once
    json.dump(record, open(args.out, "w"), indent=1)
    print("direct once", json.dumps(once), flush=True)


if __name__ == "__main__":
    main()
