"""The dense sweep of a uniform periodic level with any solver / slope pair (bench.py times LLF + minmod only):
scripts/sweep_probe.py N RIEMANN SLOPE_TYPE [STEPS] [NVAR] -> ms per sweep of the fast and the strict build (A/B of build
variants with RAMSES_AMD_LIB=...); NVAR > 5 adds passive scalars (each a fixed fraction of the density), the roofline share
counts 16 * NVAR bytes per cell
scripts/sweep_probe.py --balance [N] [STEPS]: with a library whose fast minmod unit was built with -DSWEEP_CYCLE_PROBE=1
(scripts/build_unit_variant.sh TAG hydro_sweep_fast_st1.o "-DSWEEP_CYCLE_PROBE=1", RAMSES_AMD_LIB=...), the shader clocks per
plane that every tile row of the fast LLF + minmod sweep spends before the barrier, inside it and after it, and the SIMD each
row's wave ran on (csrc/hydro_sweep.hip SWEEP_CYCLE_PROBE)"""
import ctypes as C
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

import ramses_amd  # noqa: E402
from ramses_amd import ic  # noqa: E402
from ramses_amd.hydro import HydroLevel  # noqa: E402


def balance():
    import numpy as np
    n = int(sys.argv[2]) if len(sys.argv) > 2 else 512
    steps = int(sys.argv[3]) if len(sys.argv) > 3 else 5
    L = ramses_amd.lib()
    try:
        read = L.ramses_amd_sweep_cycle_probe
    except AttributeError:
        sys.exit("this library was not built with -DSWEEP_CYCLE_PROBE=1")
    read.restype, read.argtypes = C.c_int, [C.c_void_p, C.c_long]
    p = ramses_amd.make_params(courant_factor=0.8, fast_math=True, riemann="llf", slope_type=1)
    lev = HydroLevel(n, n, n, 0.5 / n, params=p, ng=0)
    corner, back, dx = ic.sedov3d_corner_and_background(n)
    for v in range(5):
        lev.uold[v].fill_(float(back[v]))
        lev.uold[v, 0, 0, 0] = float(corner[v])
    dt = lev.courant_fine()[0]
    for _ in range(steps):
        lev.step(dt)
    torch.cuda.synchronize()
    nb, nr, nw = 8192, 12, 6
    buf = np.zeros((nb, nr, nw), dtype=np.uint64)
    assert read(buf.ctypes.data, buf.size) == 0
    buf = buf[buf[:, 2, 3] > 0]          # the blocks of the last launch that left sums
    planes = buf[:, :, 3].astype(np.float64)
    simd = (buf[:, :, 5] >> np.uint64(4)) & np.uint64(3)
    print("sweep balance %d^3 llf minmod fast: %d workgroups, %.0f planes each; shader clocks per plane, mean over workgroups" % (
        n, len(buf), planes.mean()))
    print("row   to-barrier  in-barrier  after-barrier   total   SIMD of the row's wave (share of workgroups on SIMD 0..3)")
    for r in range(nr):
        a, w, b = (buf[:, r, k].astype(np.float64) / planes[:, r] for k in range(3))
        share = [float((simd[:, r] == k).mean()) for k in range(4)]
        print("%3d   %10.0f  %10.0f  %13.0f  %6.0f   %s" % (r, a.mean(), w.mean(), b.mean(), (a + w + b).mean(),
                                                          " ".join("%.2f" % x for x in share)))
    sd = simd.astype(np.int64)
    same = np.all([(sd[:, r] == sd[:, r % 4]) for r in range(nr)], axis=0)
    four = np.array([len(set(row[:4])) == 4 for row in sd])
    print("workgroups whose waves w, w+4, w+8 share a SIMD: %.3f; whose waves 0..3 sit on four different SIMDs: %.3f" % (
        float(same.mean()), float(four.mean())))
    orders, counts = np.unique(sd[:, :4], axis=0, return_counts=True)
    print("SIMDs of waves 0..3, most frequent orders: %s" % ", ".join(
        "%s x%d" % ("".join(map(str, o)), c) for c, o in sorted(zip(counts.tolist(), orders.tolist()), reverse=True)[:6]))
    for k in range(4):
        rows = [r for r in range(nr) if r % 4 == k]
        busy = sum((buf[:, r, 0] + buf[:, r, 2]).astype(np.float64) / planes[:, r] for r in rows)
        print("waves %s: busy clocks per plane summed %.0f" % (rows, busy.mean()))


def main():
    if sys.argv[1:2] == ["--balance"]:
        return balance()
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 256
    riemann = sys.argv[2] if len(sys.argv) > 2 else "hllc"
    st = int(sys.argv[3]) if len(sys.argv) > 3 else 2
    steps = int(sys.argv[4]) if len(sys.argv) > 4 else 20
    nvar = int(sys.argv[5]) if len(sys.argv) > 5 else 5
    out = []
    for fast in (True, False):
        p = ramses_amd.make_params(courant_factor=0.8, fast_math=fast, riemann=riemann, slope_type=st, nvar=nvar)
        lev = HydroLevel(n, n, n, 0.5 / n, params=p, ng=0)
        corner, back, dx = ic.sedov3d_corner_and_background(n)
        for v in range(5):
            lev.uold[v].fill_(float(back[v]))
            lev.uold[v, 0, 0, 0] = float(corner[v])
        for v in range(5, nvar):
            lev.uold[v].copy_(lev.uold[0] * (0.1 * (v - 4)))
        dt = lev.courant_fine()[0]
        for _ in range(30):
            lev.step(dt)
        torch.cuda.synchronize()
        a, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(steps):
            lev.step(dt)
        e.record()
        torch.cuda.synchronize()
        ms = a.elapsed_time(e) / steps
        out.append("%s %.3f ms (%.1f%%)" % ("fast" if fast else "strict", ms, 100 * n ** 3 * 16 * nvar / (ms * 1e-3) / 8e12))
        del lev
    print("sweep_probe %d^3 %s slope %d%s: %s" % (n, riemann, st, " NVAR=%d" % nvar if nvar != 5 else "", "  ".join(out)))


if __name__ == "__main__":
    main()
