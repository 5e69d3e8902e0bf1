"""plan_forward (csrc/host_logic.cpp), the one place that decides how a layer's forward runs, against a hand-written table of
expected plans, as a stand-alone program under AddressSanitizer + UBSan (no GPU): tests/host/forward_plan_main.cpp carries the
table and its own main; the executable links its own sanitizer runtime (statically), so nothing is preloaded and whatever the
environment preloads does not matter."""
from tests._host_program import build_and_run


def test_forward_plan_table_under_sanitizers(tmp_path):
    r = build_and_run(tmp_path, "forward_plan_main", ["host_logic.cpp"])
    assert r.returncode == 0 and "FORWARD-PLAN-OK" in r.stdout, f"rc={r.returncode}\nstdout:\n{r.stdout[-6000:]}\nstderr:\n{r.stderr[-4000:]}"
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]
