"""carve_layer_pack (csrc/host_logic.cpp), the one statement of a layer's packed streams, as a stand-alone program under
AddressSanitizer + UBSan (no GPU): tests/host/layer_pack_main.cpp carries the checks and its own main; the executable links its
own sanitizer runtime (statically), so nothing is preloaded and whatever the environment preloads does not matter."""
from tests._host_program import build_and_run


def test_layer_pack_layout_under_sanitizers(tmp_path):
    r = build_and_run(tmp_path, "layer_pack_main", ["host_logic.cpp"])
    assert r.returncode == 0 and "LAYER-PACK-OK" in r.stdout, f"rc={r.returncode}\nstdout:\n{r.stdout}\nstderr:\n{r.stderr[-4000:]}"
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]
