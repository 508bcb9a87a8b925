"""ramses_amd_amrres_godunov of a level in tiles, for rocprofv3 --kernel-trace --stats:  python scripts/amr_tile_probe.py [level] [kind] [steps]
--pfix (anywhere on the line): the same level with pressure_fix, through a loop of its own over the public calls (bench.py knows
nothing of pressure_fix); kinds "covered" and "shell" (= bench.py's "partial"); RAMSES_AMD_TILE_SWEEP=0 selects the tree-walking
sweep for the comparison, RAMSES_AMD_PROBE_PFIX=0 times the same loop without pressure_fix.
--difmag X: the same loop with difmag = X and no pressure_fix (X = 0: the loop without either, the level's plain sweep in tiles);
--nvar N (5 .. 7) with --pfix / --difmag: N - 5 passive scalars.
--coarse-grid NX,NY,NZ [--lib PATH]: a level between walls (coarse_grid_probe below); kinds "full" and "shell"."""
import ctypes as C
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench  # noqa: E402


def pfix_probe(level, kind, steps, riemann="llf", difmag=None, nvar=5):
    """level `level` complete with level + 1 in a spherical shell ("covered"), or level `level` in a spherical shell over a
    complete level - 1 ("shell"): trees as bench.amr_resident_bench builds them; HIP events around ramses_amd_amrres_godunov"""
    import numpy as np
    import torch
    import ramses_amd
    from ramses_amd import ic
    from ramses_amd._capi import check, lib
    Lfull = level - 1 if kind == "shell" else level
    n = 2 ** Lfull
    z, y, x = np.meshgrid(np.arange(n), np.arange(n), np.arange(n), indexing="ij")
    r = np.sqrt((x - n / 2 + 0.5) ** 2 + (y - n / 2 + 0.5) ** 2 + (z - n / 2 + 0.5) ** 2)
    mask = (r >= 0.23 * n) & (r <= 0.36 * n)
    del x, y, z, r
    T = ic.uniform_tree(Lfull, order="morton", refine_mask=mask, slack=int(1.6 * mask.sum()) + 4096)
    igrid = np.ascontiguousarray(T["igrid_fine"] if kind == "shell" else T["igrid"])
    lists = [np.ascontiguousarray(T["igrid"]), np.ascontiguousarray(T["igrid_fine"])]
    ncells = 8 * len(igrid)
    dx = 0.5 / 2 ** level
    u = np.zeros((nvar, T["ncell"]))       # (passive scalars beyond 5: zero)
    u[0] = 1.0
    u[4] = 1e-5 / 0.4
    u[4, T["ncoarse"] + int(igrid[0]) - 1] = (1e-5 + 0.4 * 0.125 / dx ** 3) / 0.4
    vp = lambda a: a.ctypes.data_as(C.c_void_p)      # noqa: E731
    L = lib()
    pfix = os.environ.get("RAMSES_AMD_PROBE_PFIX", "1") != "0" and difmag is None
    os.environ.setdefault("RAMSES_AMD_TILE_MIN_OCTS", "0")
    os.environ.setdefault("RAMSES_AMD_DIFMAG_TILES", "1")       # (opt-in in production; RAMSES_AMD_TILE_SWEEP=0 still selects the tree walker)
    p = ramses_amd.make_params(courant_factor=0.8, riemann=riemann, difmag=difmag or 0.0, nvar=nvar)
    check(L.ramses_amd_amrres_invalidate())
    check(L.ramses_amd_amrres_load(nvar, T["ngridmax"], T["ncoarse"], vp(u), vp(T["son"]), vp(T["nbor"]), vp(T["father"])))
    if pfix:
        check(L.ramses_amd_amrres_enable_pfix())
    t0, w0 = L.ramses_amd_amrres_tile_sweeps(), L.ramses_amd_amrres_tree_sweeps()

    def set_unew():
        for ig in lists:
            if pfix:
                check(L.ramses_amd_amrres_set_unew_pfix(C.byref(p), len(ig), vp(ig)))
            else:
                check(L.ramses_amd_amrres_set_unew(len(ig), vp(ig)))

    def sweep():
        check(L.ramses_amd_amrres_godunov(C.byref(p), level, len(igrid), vp(igrid), dx, 1e-6, 32, 0, 1))
    for _ in range(2):
        set_unew()
        sweep()
    torch.cuda.synchronize()
    times = []
    for _ in range(steps):
        set_unew()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        sweep()
        b.record()
        torch.cuda.synchronize()
        times.append(a.elapsed_time(b))
    out = {"pressure_fix": pfix, "difmag": difmag or 0.0, "nvar": nvar, "level": level, "kind": kind, "riemann": riemann, "cells": ncells,
           "ms_per_sweep": sorted(times)[len(times) // 2], "ms_all": [round(t, 4) for t in times],
           "tile_sweeps": int(L.ramses_amd_amrres_tile_sweeps() - t0), "tree_sweeps": int(L.ramses_amd_amrres_tree_sweeps() - w0),
           "levels_in_tiles": int(L.ramses_amd_amrres_tiled_levels())}
    check(L.ramses_amd_amrres_invalidate())
    return out


def coarse_grid_probe(level, kind, steps, grid, riemann="llf", libpath=None):
    """--coarse-grid NX,NY,NZ: one godunov_fine of level `level` of a box whose coarse grid has NX x NY x NZ cells, the middle one
    active and the others boundary octs (walls): "full" = the level complete and listed (the active cell's octs), "shell" = the
    level in a spherical shell that reaches the walls over a complete level - 1.  Fast and strict arithmetic, the level in tiles
    against RAMSES_AMD_TILES=0 (Z-order, the tree walker) in the same library.  --lib PATH: the
    library of another commit instead (one without ramses_amd_amrres_coarse_grid keeps the host's numbering: its tree walker)."""
    import numpy as np
    import torch
    import ramses_amd
    from ramses_amd import ic
    from ramses_amd import _capi
    nx, ny, nz = grid
    act = (nx // 2, ny // 2, nz // 2)
    Lfull = level - 1 if kind == "shell" else level
    n = 2 ** Lfull
    mask = None
    if kind == "shell":
        z, y, x = np.meshgrid(np.arange(nz * n), np.arange(ny * n), np.arange(nx * n), indexing="ij", sparse=True)
        r = np.sqrt((x - (act[0] + 0.5) * n + 0.5) ** 2 + (y - (act[1] + 0.5) * n + 0.5) ** 2 + (z - (act[2] + 0.5) * n + 0.5) ** 2)
        inside = (x // n == act[0]) & (y // n == act[1]) & (z // n == act[2])
        mask = (r >= 0.30 * n) & (r <= 0.50 * n) & inside
        del r, inside
    T = ic.coarse_grid_tree(grid, Lfull, order="morton", refine_mask=mask, slack=(int(1.6 * mask.sum()) if mask is not None else 0) + 4096)
    no = 2 ** (Lfull - 1)
    ids = T["oct_ids"][Lfull][act[2] * no:(act[2] + 1) * no, act[1] * no:(act[1] + 1) * no, act[0] * no:(act[0] + 1) * no]
    active = [np.ascontiguousarray(np.sort(ids.reshape(-1)))]
    if kind == "shell":
        active.append(np.ascontiguousarray(np.sort(T["igrid_fine"])))
    igrid = active[-1]
    dx = 0.5 / 2 ** level
    u = np.zeros((5, T["ncell"]))
    u[0] = 1.0
    u[4] = 1e-5 / 0.4
    u[4, T["ncoarse"] + int(igrid[len(igrid) // 2]) - 1] = (1e-5 + 0.4 * 0.125 / dx ** 3) / 0.4
    vp = lambda a: a.ctypes.data_as(C.c_void_p)      # noqa: E731
    if libpath:
        L = C.CDLL(libpath)
        for name, res, args in _capi.SYMBOLS:
            if hasattr(L, name):
                f = getattr(L, name)
                f.restype, f.argtypes = res, args
    else:
        L = _capi.lib()

    def check(rc):
        if rc != 0:
            raise RuntimeError(L.ramses_amd_last_error().decode())
    os.environ.setdefault("RAMSES_AMD_TILE_MIN_OCTS", "0")
    out = {"coarse_grid": list(grid), "level": level, "kind": kind, "riemann": riemann, "cells": 8 * len(igrid), "library": libpath or "this commit's"}
    for tiles in ("1", "0"):
        os.environ["RAMSES_AMD_TILES"] = tiles
        check(L.ramses_amd_amrres_invalidate())
        if hasattr(L, "ramses_amd_amrres_coarse_grid"):
            check(L.ramses_amd_amrres_coarse_grid(nx, ny, nz))
        check(L.ramses_amd_amrres_load(5, T["ngridmax"], T["ncoarse"], vp(u), vp(T["son"]), vp(T["nbor"]), vp(T["father"])))
        for fast in (True, False):
            p = ramses_amd.make_params(courant_factor=0.8, riemann=riemann, fast_math=fast)
            t0, w0 = L.ramses_amd_amrres_tile_sweeps(), L.ramses_amd_amrres_tree_sweeps()

            def once():
                for ig in active:
                    check(L.ramses_amd_amrres_set_unew(len(ig), vp(ig)))
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                torch.cuda.synchronize()
                a.record()
                check(L.ramses_amd_amrres_godunov(C.byref(p), level, len(igrid), vp(igrid), dx, 1e-6, 32, 0, 1))
                b.record()
                torch.cuda.synchronize()
                return a.elapsed_time(b)
            for _ in range(2):
                once()
            times = [once() for _ in range(steps)]
            out["%s_%s" % ("tiles" if tiles == "1" else "no_tiles", "fast" if fast else "strict")] = {
                "ms_per_sweep": sorted(times)[len(times) // 2], "ms_all": [round(t, 4) for t in times],
                "tile_sweeps": int(L.ramses_amd_amrres_tile_sweeps() - t0), "tree_sweeps": int(L.ramses_amd_amrres_tree_sweeps() - w0),
                "levels_in_tiles": int(L.ramses_amd_amrres_tiled_levels())}
        check(L.ramses_amd_amrres_invalidate())
    return out


if __name__ == "__main__":
    args = [a for a in sys.argv[1:] if a != "--pfix"]
    grid = libpath = None
    if "--coarse-grid" in args:
        k = args.index("--coarse-grid")
        grid = tuple(int(v) for v in args[k + 1].split(","))
        del args[k:k + 2]
    if "--lib" in args:
        k = args.index("--lib")
        libpath = args[k + 1]
        del args[k:k + 2]
    if grid is not None:
        import torch
        torch.cuda.init()
        print(json.dumps(coarse_grid_probe(int(args[0]) if args else 8, {"partial": "shell", "covered": "full"}.get(args[1], args[1]) if len(args) > 1 else "full",
                                           int(args[2]) if len(args) > 2 else 5, grid, os.environ.get("RAMSES_AMD_BENCH_AMR_RIEMANN", "llf"), libpath)))
        sys.exit(0)
    difmag = None
    if "--difmag" in args:
        k = args.index("--difmag")
        difmag = float(args[k + 1])
        del args[k:k + 2]
    nvar = 5
    if "--nvar" in args:
        k = args.index("--nvar")
        nvar = int(args[k + 1])
        del args[k:k + 2]
    level = int(args[0]) if len(args) > 0 else 8
    kind = args[1] if len(args) > 1 else "covered"
    steps = int(args[2]) if len(args) > 2 else 5
    import torch
    torch.cuda.init()
    if "--pfix" in sys.argv[1:] or difmag is not None:
        print(json.dumps(pfix_probe(level, {"partial": "shell"}.get(kind, kind), steps, os.environ.get("RAMSES_AMD_BENCH_AMR_RIEMANN", "llf"), difmag, nvar)))
    else:
        out = bench.amr_resident_bench(level, steps=steps, kind=kind)
        print(json.dumps({k: out[k] for k in ("ms_per_sweep", "tree_walking_ms_per_sweep", "cells", "workload")}))
        print("frac", out["roofline"]["frac"])
