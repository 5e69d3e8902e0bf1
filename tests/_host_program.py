"""Build and run one stand-alone program of tests/host/ under AddressSanitizer + UBSan (no GPU).  The program has its own main and
links its own sanitizer runtime statically, so nothing is preloaded and whatever the environment preloads does not matter."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "diffusion_model_amd", "csrc")


def build_and_run(directory, main, sources, args=(), flags=()):
    """tests/host/<main>.cpp with the files ``sources`` of csrc/, built into ``directory`` and run with ``args``
    -> the CompletedProcess of the run (text mode).  A failed build fails the calling test with the compiler's words."""
    exe = os.path.join(str(directory), main)
    cmd = ["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           "-fno-omit-frame-pointer", "-static-libasan", "-static-libubsan", *flags, os.path.join(ROOT, "tests", "host", main + ".cpp"),
           *(os.path.join(CSRC, s) for s in sources), "-o", exe]
    b = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert b.returncode == 0, b.stderr[-4000:]
    env = dict(os.environ, ASAN_OPTIONS="halt_on_error=1:abort_on_error=0", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    return subprocess.run([exe, *args], env=env, capture_output=True, text=True, timeout=120)
