"""The halo protocol the AMR, multigrid and CG units share (ramses_amd/csrc/peer_exchange.hpp: PeerExchange with plan / stage_out /
stage_in / rccl, and the communicator-list helpers peer_prefix / peer_lists) compiled by the plain host compiler with
-fsanitize=address,undefined into a program of its own (tests/native/peer_exchange_check.cpp) and run as a child process.  The
program brings stand-ins for the allocators, hipMemcpy / hipMemcpyAsync (a memcpy), hipStreamSynchronize and
ramses_amd_rccl_exchange (copies message i of the send buffer to message i of the receive buffer and records its arguments), so
nothing of the HIP runtime is linked and no GPU is opened.  It checks, for one and for three ranks, with a peer that has nothing
either way, a peer that only sends and both sides empty, at 8, 8*5 and 8*4 doubles per oct: the exported offset tables are the
prefix sums times the doubles per oct; stage_out leaves sendbuf in h_send and stage_in h_recv in recvbuf; a stage_in with another
tag or another ncpu is refused with the caller's text and leaves the exchange open, the matching one closes it, a second one is
refused; the RCCL call names exactly the peers with a message, in icpu order, on the null stream; a plan between stage_out and
stage_in closes the exchange and tables of another size never pass (new with the shared protocol); the pinned twins are not
reallocated for a smaller request or for one up to 1.5 times the first; nothing stays allocated after release."""
import os
import shutil
import subprocess

from helpers import hip_include

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "native", "peer_exchange_check.cpp")


def test_peer_exchange_under_the_sanitizers(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "peer_exchange_check")
    # (the sanitizers' runtimes linked statically: the program then runs whatever else the environment preloads)
    r = subprocess.run([cxx, "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-D__HIP_PLATFORM_AMD__", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=undefined", "-static-libasan", "-static-libubsan", "-isystem", hip_include(),
                        "-I", os.path.join(ROOT, "ramses_amd"), SRC, "-o", exe],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    print(r.stdout)
    assert r.returncode == 0, "peer_exchange.hpp does not compile with the host compiler alone"
    # (the program counts its own live blocks; the leak checker of the sanitizer needs ptrace, which not every sandbox grants)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, env=env)
    print(r.stdout)
    assert r.returncode == 0 and r.stdout.strip().splitlines()[-1:] == ["ok"], r.stdout
