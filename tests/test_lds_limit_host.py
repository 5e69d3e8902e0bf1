"""The per-device record behind the one dynamic-LDS-limit policy of the evaluation kernels (csrc/eval/lds_limit.h), as a
stand-alone program under AddressSanitizer + UBSan (no GPU): tests/host/lds_limit_main.cpp carries the checks and its own main."""
from tests._host_program import build_and_run


def test_lds_limit_record_under_sanitizers(tmp_path):
    r = build_and_run(tmp_path, "lds_limit_main", [], flags=["-pthread"])
    assert r.returncode == 0 and "LDS-LIMIT-OK" in r.stdout, f"rc={r.returncode}\nstdout:\n{r.stdout}\nstderr:\n{r.stderr[-4000:]}"
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]
