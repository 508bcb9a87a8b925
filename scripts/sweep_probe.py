"""The dense sweep of a uniform periodic level with any solver / slope pair (bench.py times LLF + minmod only):
scripts/sweep_probe.py N RIEMANN SLOPE_TYPE [STEPS] [NVAR] -> ms per sweep of the fast and the strict build (A/B of build
variants with RAMSES_AMD_LIB=...); NVAR > 5 adds passive scalars (each a fixed fraction of the density), the roofline share
counts 16 * NVAR bytes per cell"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

import ramses_amd  # noqa: E402
from ramses_amd import ic  # noqa: E402
from ramses_amd.hydro import HydroLevel  # noqa: E402


def main():
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
