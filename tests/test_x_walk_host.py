"""x_walk (csrc/x_walk.h): which (tile, column share) unit a persistent coordinate workgroup runs at which step, enumerated for every
workgroup by the stand-alone program tests/host/x_walk_main.cpp under AddressSanitizer + UBSan (no GPU; the executable links its own
sanitizer runtime statically, so nothing is preloaded).  T in {1, 2, 255, 256, 257, 511, 512, 513, 8064, 8065} tiles x G in
{1, 8, 104, 255, 256, 304} workgroups, two shares: the program's header lists the checks."""
from tests._host_program import build_and_run


def test_x_walk_covers_pairs_keeps_xcds_and_balances(tmp_path):
    """Every unit once; a kept share 1 directly behind its share 0 on the same workgroup; every unit on a workgroup with the XCD index
    xcd_tile assigns to its position; no workgroup above ceil(2T/G) units, for every G of the list (the bound the program proves
    for all G, not only 8 | G); 63 units for every workgroup at T = 8,064, G = 256."""
    r = build_and_run(tmp_path, "x_walk_main", [])
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]
    assert r.returncode == 0 and "X-WALK-OK" in r.stdout, f"rc={r.returncode}\nstdout:\n{r.stdout[-6000:]}\nstderr:\n{r.stderr[-4000:]}"
