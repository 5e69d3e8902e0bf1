"""plan_forward (csrc/host_logic.cpp), the one place that decides how a layer's forward runs, against a hand-written table of
expected plans, as a stand-alone program under AddressSanitizer + UBSan (no GPU): tests/host/forward_plan_main.cpp carries the
table and its own main; the executable links its own sanitizer runtime (statically), so nothing is preloaded and whatever the
environment preloads does not matter."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_forward_plan_table_under_sanitizers(tmp_path):
    exe = str(tmp_path / "forward_plan_main")
    cmd = ["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           "-fno-omit-frame-pointer", "-static-libasan", "-static-libubsan", os.path.join(ROOT, "tests", "host", "forward_plan_main.cpp"),
           os.path.join(ROOT, "diffusion_model_amd", "csrc", "host_logic.cpp"), "-o", exe]
    b = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert b.returncode == 0, b.stderr[-4000:]
    env = dict(os.environ, ASAN_OPTIONS="halt_on_error=1:abort_on_error=0", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    r = subprocess.run([exe], env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "FORWARD-PLAN-OK" in r.stdout, f"rc={r.returncode}\nstdout:\n{r.stdout[-6000:]}\nstderr:\n{r.stderr[-4000:]}"
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]
