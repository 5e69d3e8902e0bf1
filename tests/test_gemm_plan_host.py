"""The host side of the training GEMMs (csrc/host_logic.cpp: plan_gemm_tn, gemm_tn_args_check, gemm_rows_args_check,
gemm_rows_out_check) as a stand-alone program under AddressSanitizer + UBSan (no GPU): tests/host/gemm_plan_main.cpp has its own
main and links its own sanitizer runtime statically, so nothing is preloaded.  The program reads the cases of
tests/_gemm_cases.py, checks that the argument checks accept each of them and refuse the bad variants (a bf16 output stride
that is no multiple of 8, a base pointer inside a 16-byte piece, a short workspace ...), sweeps E = 1 .. 40000 over the (M, N)
of the cases for the invariants of the split-K plan, and prints each case's plan, which is compared with the Python
restatement here and in tests/test_gemm_cases_cpu.py."""
import atexit
import functools
import os
import shutil
import tempfile

from tests import _gemm_cases as GC
from tests._host_program import build_and_run


@functools.lru_cache(maxsize=None)
def host_program_run():
    """build and run the program once per session -> (return code, stdout, stderr)"""
    tmp = tempfile.mkdtemp(prefix="gemm_plan_")
    atexit.register(shutil.rmtree, tmp, ignore_errors=True)
    cases = os.path.join(tmp, "cases.txt")
    with open(cases, "w") as f:
        f.write(GC.host_case_lines())
    r = build_and_run(tmp, "gemm_plan_main", ["host_logic.cpp"], args=[cases])
    return r.returncode, r.stdout, r.stderr


def host_plans():
    """{(E, M, N): (BN, tiles_n, S, steps_per_slice)} as the host code planned the cases"""
    _, out, _ = host_program_run()
    plans = {}
    for line in out.splitlines():
        w = line.split()
        if w and w[0] == "PLAN":
            v = [int(x) for x in w[1:]]
            plans[tuple(v[:3])] = tuple(v[3:])
    return plans


def test_gemm_plan_and_checks_under_sanitizers():
    rc, out, err = host_program_run()
    assert rc == 0 and "GEMM-PLAN-OK" in out, f"rc={rc}\nstdout:\n{out[-6000:]}\nstderr:\n{err[-4000:]}"
    assert "ERROR: AddressSanitizer" not in err and "runtime error" not in err, err[-4000:]
    assert f"cases: {len(GC.TN_CASES)} tn, {len(GC.ROWS_CASES)} rows" in out
    swept = {tuple(int(x) for x in line.split()[1:]) for line in out.splitlines() if line.startswith("SWEEP")}
    assert swept == {(c.M, c.N) for c in GC.TN_CASES}


def test_host_plan_equals_the_restatement():
    plans = host_plans()
    assert len(plans) == len({(c.E, c.M, c.N) for c in GC.TN_CASES})
    for c in GC.TN_CASES:
        p = GC.plan_gemm_tn(c.E, c.M, c.N)
        assert plans[(c.E, c.M, c.N)] == (p.BN, p.tiles_n, p.S, p.steps_per_slice), c
