"""The host helpers every unit of the C ABI shares (ramses_amd/csrc/host_util.hpp: fail / hipfail / HCHK, DevBuf and PinBuf,
grid_for) compiled by the plain host compiler with -fsanitize=address,undefined into a program of its own (tests/native/
host_util_check.cpp) and run as a child process.  The program brings counting stand-ins for hipMalloc / hipFree / hipHostMalloc /
hipHostFree / hipGetErrorString / ramses_amd_set_error, so nothing of the HIP runtime is linked and no GPU is opened; it checks
the buffers' allocation discipline (a first ensure(0) allocates, growth frees once and allocates once, a smaller request keeps
the pointer, a failed allocation leaves the buffer empty, release is idempotent, nothing stays allocated), the error path (text
and code as handed over, a message longer than the 512-byte buffer truncated) and the three regimes of grid_for.  That the
header compiles here at all is the check that it pulls in no kernel header."""
import os
import shutil
import subprocess

from helpers import hip_include

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "native", "host_util_check.cpp")


def test_host_util_under_the_sanitizers(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "host_util_check")
    # (the sanitizers' runtimes linked statically: the program then runs whatever else the environment preloads)
    r = subprocess.run([cxx, "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-D__HIP_PLATFORM_AMD__", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=undefined", "-static-libasan", "-static-libubsan", "-isystem", hip_include(),
                        "-I", os.path.join(ROOT, "ramses_amd"), SRC, "-o", exe],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    print(r.stdout)
    assert r.returncode == 0, "host_util.hpp does not compile with the host compiler alone"
    # (the program counts its own live blocks; the leak checker of the sanitizer needs ptrace, which not every sandbox grants)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, env=env)
    print(r.stdout)
    assert r.returncode == 0 and r.stdout.strip().splitlines()[-1:] == ["ok"], r.stdout
