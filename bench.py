#!/usr/bin/env python
"""bench.py -- cell-updates/s of the Godunov sweep on a uniform Sedov3D level.

    python bench.py --gpus N --steps K --warmup W [--n 512] [--fast 0|1]

One "step" = one godunov_fine pass over this rank's level brick (+ the halo
exchange of uold for N>1): the fused set_unew+godunov_fine+set_uold kernel of
libramses_amd.so, with the state already resident in HBM.  Weak scaling: every
rank owns an n^3 brick of a (n*px, n*py, n*pz) periodic Sedov3D box.

Prints ONE JSON line on rank 0 (see README/DESIGN.md "Measurement").
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

HBM_PEAK_GBS = 8000.0        # MI355X HBM3E spec peak (MI355X_MICROARCH.md)
BYTES_PER_CELL_UPDATE = 80   # read uold + write unew, nvar=5, FP64


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--n", "--cells", dest="n", type=int, default=512, help="cells per direction of each rank's brick")
    ap.add_argument("--fast", type=int, default=1, help="1: FMA-contracted build (<=1e-12 of strict), 0: strict")
    ap.add_argument("--zchunk", type=int, default=0)
    ap.add_argument("--tile-rows", type=int, default=0)
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--stress-steps", type=int, default=60,
                    help="N=1: also time the sweep on the state after this many steps in all (0 = skip)")
    ap.add_argument("--no-overlap", action="store_true", help="N>1: exchange after the sweep instead of behind it")
    ap.add_argument("--overlap", choices=["auto", "on", "off"], default="auto",
                    help="N>1: hide the halo exchange behind the interior sweep (auto: measure both, keep the faster)")
    ap.add_argument("--vcycle-level", type=int, default=9,
                    help="multigrid V-cycle measurement: 2^level cells per direction per GPU (0 = skip)")
    ap.add_argument("--spinup-ms", type=int, default=150,
                    help="keep the sweep kernel busy on a scratch level of the same size this long before the warm-up steps (ramp; 0 = none)")
    ap.add_argument("--amr-level", type=int, default=8,
                    help="tree-walking (AMR) sweep measurement on a fully refined synthetic 2^level^3 tree (0 = skip)")
    ap.add_argument("--mhd-level", type=int, default=7,
                    help="MHD sweep measurement (SOLVER=mhd) on a uniform 2^level^3 level (0 = skip)")
    ap.add_argument("--mg-tune", type=int, default=-1,
                    help="fused smoother: 1 = library default (2+2 colour passes on 32-row tiles), 4 = one 4-pass launch, "
                         "12/16/24/32 = 2+2 passes on that many tile rows, 0 = one kernel per colour pass (-1: leave the default)")
    ap.add_argument("--vcycle-deadline", type=int, default=180, help="N>1: seconds before the V-cycle leg is abandoned")
    ap.add_argument("--deadline", type=int, default=900,
                    help="N>1: seconds before the whole run is abandoned (a hung collective must not hang the node)")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps, write the state the last timed step left as DIR/<name>.npy (float64, at most 64 MB in all)")
    return ap.parse_args()


def rank_grid(nranks):
    """Octant-style decomposition (the Hilbert split of a uniform grid gives
    axis-aligned bricks for 2^k ranks)."""
    p = [1, 1, 1]
    d = 0
    r = nranks
    while r > 1:
        assert r % 2 == 0, "rank count must be a power of two"
        p[d] *= 2
        r //= 2
        d = (d + 1) % 3
    return tuple(p)


def _cpu_baseline_port(n_ref=48, steps=1):
    """Scalar C port (oracle/hydro_oracle.c) on 1 core: fallback when the
    reference binaries are not present."""
    from oracle import pyoracle
    from ramses_amd import ic
    u, dx = ic.sedov3d(n_ref)
    p = pyoracle.make_params()
    dt = pyoracle.courant_uniform(p, u, dx, 0.8)
    pyoracle.godunov_uniform(p, u[:, :8, :8, :8].copy(), dx, dt)  # warm the library
    t0 = time.perf_counter()
    for _ in range(steps):
        u = pyoracle.godunov_uniform(p, u, dx, dt)
    t = time.perf_counter() - t0
    return {"value": n_ref ** 3 * steps / t, "unit": "cell-updates/s", "cores": 1, "kind": "port",
            "sample": "%d sweep(s) of a %d^3 Sedov3D level, oracle/hydro_oracle.c (godfine1+unsplit restatement), %.1f s"
                      % (steps, n_ref, t)}


def cpu_baseline():
    """The reference itself (oracle/_ref/ramses3d[_mpi], the unmodified F90
    program built by oracle/build_ref.sh) on the host cores of this box, on a
    bounded sample of the same workload: sedov3d.nml at 256^3 (config C2, MPI on up
    to 64 cores; 128^3 below 16 cores) or 64^3 (serial); the rate comes from its own
    'hydro - godunov' timer row."""
    import re
    import shutil
    ref = os.path.join(ROOT, "oracle", "_ref")
    mpi_bin, ser_bin = os.path.join(ref, "ramses3d_mpi"), os.path.join(ref, "ramses3d")
    mpiexec = "/opt/conda/bin/mpiexec"
    try:
        from oracle import ramses_snapshot as rs
        ncores = os.cpu_count() or 1
        try:
            import psutil
            ncores = psutil.cpu_count(logical=False) or ncores
        except Exception:
            pass
        if os.path.exists(mpi_bin) and os.path.exists(mpiexec) and ncores >= 2:
            P = 1
            while P * 2 <= min(ncores, 64):
                P *= 2
            level, nstep, binary = (8 if P >= 16 else 7), 10, mpi_bin
        elif os.path.exists(ser_bin):
            P, level, nstep, binary = 1, 6, 8, ser_bin
        else:
            return _cpu_baseline_port()
        nml = rs.sedov3d_namelist(level=level, nstepmax=nstep, foutput=1000, mem_factor=3.0 if P > 1 else 1.3)
        t0 = time.perf_counter()
        work, out = rs.run_reference(nml, nproc=P, binary=binary, timeout=600)
        wall = time.perf_counter() - t0
        shutil.rmtree(work, ignore_errors=True)
        nsweeps = len(re.findall(r"Fine step=", out))
        row = [l for l in out.splitlines() if "hydro - godunov" in l][-1].split()
        tg = float(row[2]) if P > 1 else float(row[0])     # MPI table: min avg MAX ...; serial: seconds
        n = 2 ** level
        return {"value": n ** 3 * nsweeps / tg, "unit": "cell-updates/s", "cores": P, "kind": "reference",
                "sample": "unmodified reference F90 (amdflang -O2, NVECTOR=32%s), sedov3d.nml at %d^3, %d godunov_fine sweeps, "
                          "'hydro - godunov' timer %s %.2f s (run wall %.1f s)"
                          % (", MPICH %d ranks" % P if P > 1 else ", serial", n, nsweeps, "max over ranks" if P > 1 else "=", tg, wall)}
    except Exception as exc:  # the baseline is a report, never a reason to lose the GPU number
        out = _cpu_baseline_port()
        out["sample"] += " (reference binary unavailable: %s)" % str(exc)[:200]
        return out


def vcycle_cpu_baseline():
    """The reference's own multigrid beside the V-cycle leg: the unmodified MPI program on config C4's stand-in --
    hydro + self-gravity of a dense block on a uniform level, 256^3 from 16 cores on (128^3 below) -- and its `poisson` timer row
    (amr/update_time.f90:59-178: save_phi_old + multigrid_fine + force_fine, maximum over the ranks) against the V-cycles its
    `==> Level= Step=` lines count (poisson/multigrid_fine_commons.f90:284): DOF/s = N^3 x V-cycles / t(poisson).  A lower bound
    of the reference's V-cycle rate (the row also holds force_fine and the first guess), which is the direction a baseline may err."""
    import importlib.util
    import re
    import shutil
    ref = os.path.join(ROOT, "oracle", "_ref")
    mpi_bin, mpiexec = os.path.join(ref, "ramses3d_mpi"), "/opt/conda/bin/mpiexec"
    try:
        from oracle import ramses_snapshot as rs
        spec = importlib.util.spec_from_file_location("mkb", os.path.join(ROOT, "tests", "golden", "make_golden_baseline.py"))
        mkb = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mkb)
        ncores = os.cpu_count() or 1
        try:
            import psutil
            ncores = psutil.cpu_count(logical=False) or ncores
        except Exception:
            pass
        if not (os.path.exists(mpi_bin) and os.path.exists(mpiexec)) or ncores < 2:
            return {"value": None, "note": "no MPI reference binary on this box"}
        P = 1
        while P * 2 <= min(ncores, 64):
            P *= 2
        level, nstep = (8 if P >= 16 else 7), 3
        nml = mkb.c4_namelist(level, nstep).replace("ngridtot=", "ngridtot=%d !" % int(3.0 * sum(8 ** l for l in range(level)) + 1000))
        t0 = time.perf_counter()
        work, out = rs.run_reference(nml, nproc=P, binary=mpi_bin, timeout=900)
        wall = time.perf_counter() - t0
        shutil.rmtree(work, ignore_errors=True)
        cycles = [int(m.group(1)) for m in re.finditer(r"==> Level=\s*%d Step=\s*(\d+)" % level, out)]
        row = [l for l in out.splitlines() if l.strip().endswith("poisson") or " poisson " in l + " "][-1].split()
        tp = float(row[2])                                   # MPI table: min avg MAX ...
        n = 2 ** level
        return {"value": float(n) ** 3 * sum(cycles) / tp, "unit": "DOF/s", "cores": P, "kind": "reference",
                "sample": "unmodified reference F90 (amdflang -O2, NVECTOR=32, MPICH %d ranks), hydro + self-gravity of a dense block at %d^3 "
                          "(config C4's stand-in), %d solves with %s V-cycles, 'poisson' timer (multigrid_fine + force_fine + first guess) "
                          "max over ranks %.2f s (run wall %.1f s)" % (P, n, len(cycles), cycles, tp, wall)}
    except Exception as exc:      # noqa: BLE001  (a report, never a reason to lose the GPU number)
        return {"value": None, "error": str(exc)[:300]}


def pmc_traffic(n, world, args):
    """HBM bytes per sweep launch from the rocprofv3 PMC passes (FETCH_SIZE with the
    gfx950 calibration + WRITE_SIZE), measured by scripts/profile_gpu.sh on this
    same command with the current kernel and committed under profiles/ (the newest
    r*_sweep_traffic.json); null when no matching profile."""
    import glob
    try:
        path = sorted(glob.glob(os.path.join(ROOT, "profiles", "r*_sweep_traffic.json")))[-1]
        t = json.load(open(path))
        if t["n"] == n and world == 1 and args.fast == 1 and not args.tile_rows and not args.zchunk:
            return t["traffic_bytes_per_launch"], ("%s: rocprofv3 PMC passes of this command (scripts/profile_gpu.sh), "
                                                   "NOT measured in this run" % os.path.relpath(path, ROOT))
    except Exception:
        pass
    return None, "no matching PMC profile under profiles/"


def rank_census(rank, world, local_dev, transport_note, group=None):
    """Who ran: every rank's device (ramses_amd_device_uid = hash of host name + PCI bus id, the number the Fortran shim
    compares before it brings RCCL up), so that an N-GPU line proves N ranks on N distinct devices."""
    import torch
    import torch.distributed as dist
    from ramses_amd._capi import lib, check
    uid = C.c_int64(0)
    check(lib().ramses_amd_device_uid(C.byref(uid)))
    try:
        bus = torch.cuda.get_device_properties(local_dev).pci_bus_id
    except Exception:     # noqa: BLE001
        bus = None
    mine = {"rank": rank, "device": local_dev, "uid": "%016x" % uid.value, "pci_bus_id": bus,
            "rccl_comm_of_the_library": bool(lib().ramses_amd_rccl_ready())}
    if world > 1:
        allr = [None] * world
        dist.all_gather_object(allr, mine, group=group)     # the transport's group: after a failed RCCL self-test the default group is unusable
    else:
        allr = [mine]
    return {"world_size": world, "distinct_devices": len({r["uid"] for r in allr}), "per_rank": allr,
            "library_rccl_ranks": sum(1 for r in allr if r["rccl_comm_of_the_library"]),
            "transport": "none (single rank)" if world == 1 else (transport_note or "RCCL send/recv (torch.distributed)")}


DUMP_CELLS = 1 << 20         # --dump-outputs: cells written per job (5 variables + the cell number, FP64: 48 MB)
DUMP_SEED = 20240917


def dump_outputs(lev, out_dir, world, rank):
    """--dump-outputs: what the timed steps hand their caller, the conserved state uold of the rank's brick after the last
    timed step (FP64).  Whole as state[nvar,nz,ny,nx] up to DUMP_CELLS cells (shared out over the ranks); above that the
    same seeded sample of cells in every run of the same size: state_sample[nvar,S] at the flat (z,y,x) cell numbers
    state_sample_cells[S].  state_sum[nvar]: every variable summed over all cells of the brick.  N>1: one set per rank,
    the file names end in _rank<r>.  Returns the names written."""
    import numpy as np
    import torch
    os.makedirs(out_dir, exist_ok=True)
    u = lev.interior(lev.uold)
    nvar, nz, ny, nx = u.shape
    ncell = nz * ny * nx
    budget = DUMP_CELLS // world
    arrays = {}
    if ncell <= budget:
        arrays["state"] = u.cpu().numpy()
    else:
        cells = np.sort(np.random.default_rng(DUMP_SEED).choice(ncell, size=budget, replace=False))
        c = torch.from_numpy(cells).to(u.device)
        arrays["state_sample"] = u[:, c // (ny * nx), (c // nx) % ny, c % nx].cpu().numpy()
        arrays["state_sample_cells"] = cells.astype(np.float64)
    arrays["state_sum"] = u.sum(dim=(1, 2, 3)).cpu().numpy()
    suffix = "_rank%d" % rank if world > 1 else ""
    names = []
    for name, a in arrays.items():
        names.append(name + suffix + ".npy")
        np.save(os.path.join(out_dir, names[-1]), np.ascontiguousarray(a, dtype=np.float64))
    return names


BYTES_PER_DOF_VCYCLE = 227   # 202 B fine level + 178/7 B coarse hierarchy


def vcycle_bench(level):
    """Second half of the metric: V-cycle DOF/s of multigrid_fine on a uniform
    periodic level (blob stand-in for cosmo.nml), one GPU."""
    import torch
    from ramses_amd.poisson import PoissonLevel
    n = 2 ** level
    lev = PoissonLevel(level, boxlen=1.0, epsilon=1e-30)   # never converges: exactly MAXITER=10 V-cycles
    lev.rho.fill_(1.0)
    a, b = int(0.375 * n), int(0.625 * n)
    lev.rho[a:b, a:b, a:b] = 10.0
    rho_tot = float(lev.rho.mean().item())
    lev.multigrid_fine(rho_tot)                              # warm-up
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    iters, err = lev.multigrid_fine(rho_tot)
    torch.cuda.synchronize()
    t = time.perf_counter() - t0
    dof = n ** 3 * iters / t
    gbs = dof * BYTES_PER_DOF_VCYCLE / 1e9
    return {"metric": "V-cycle DOF/s (multigrid_fine)", "value": dof, "unit": "DOF/s", "level": level,
            "vcycles": iters, "ms_per_vcycle": t / iters * 1e3, "final_error": err,
            "roofline": {"bound": "hbm", "achieved": gbs, "peak": HBM_PEAK_GBS, "unit": "GB/s",
                         "frac": gbs / HBM_PEAK_GBS, "bytes_per_dof": BYTES_PER_DOF_VCYCLE}}


def mg_rank_grid(nranks):
    """The rank grid of the distributed multigrid: the cubic box is cut along z first, then y, then x (2 ranks: two half
    boxes, 4: four quarter columns, 8: the octants -- the brick shapes the reference's Hilbert decomposition gives 2^k ranks
    on a uniform level); z first keeps the rows of a brick, which the smoother's tiles and the halo slabs stream, long."""
    p = [1, 1, 1]
    d = 2
    r = nranks
    while r > 1:
        assert r % 2 == 0, "rank count must be a power of two"
        p[d] *= 2
        r //= 2
        d = (d - 1) % 3
    return tuple(p)


def vcycle_bench_dist(level_local, rank, world, transport=None):
    """The same measurement on N = 2^k GPUs: the reference's box is a cube (nx = ny = nz = 1 is not a namelist item), so the
    level is the smallest cubic level that gives every GPU at least 2^level_local cells per direction's worth of work
    (N = 2, 4, 8 with level_local = 9: the 1024^3 level in bricks of 1024 x 1024 x 512, 1024 x 512 x 512, 512^3);
    distributed V-cycles with the 5-cell communication-avoiding halo and replicated coarse levels
    (ramses_amd/poisson_parallel.py).  Collective: every rank calls it."""
    import math
    import torch
    from ramses_amd.poisson_parallel import PoissonDecomposition
    pgrid = mg_rank_grid(world)
    level = level_local + int(math.ceil(math.log2(world) / 3.0))
    pd = PoissonDecomposition(pgrid, rank, level=level, boxlen=1.0, epsilon=1e-30, transport=transport)   # exactly MAXITER=10 V-cycles
    N = 1 << level
    a, b = int(0.375 * N), int(0.625 * N)
    nx, ny, nz = pd.dims
    pd.rho.fill_(1.0)
    sl = []
    for d, nd in ((2, nz), (1, ny), (0, nx)):                       # tensor axes are z, y, x
        lo, hi = max(a - pd.coords[d] * nd, 0), min(b - pd.coords[d] * nd, nd)
        sl.append(slice(lo, max(hi, lo)))
    pd.rho[sl[0], sl[1], sl[2]] = 10.0
    rho_tot = 1.0 + 9.0 * ((b - a) / N) ** 3
    pd.multigrid_fine(rho_tot)                # warm-up
    pd.exchanges = 0
    pd.tr.barrier()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    iters, err = pd.multigrid_fine(rho_tot)
    torch.cuda.synchronize()
    pd.tr.barrier()
    t = time.perf_counter() - t0
    t = pd.tr.allreduce(t, "cuda", op="max")
    dof = float(N) ** 3 * iters / t
    gbs = dof * BYTES_PER_DOF_VCYCLE / 1e9
    return {"metric": "V-cycle DOF/s (multigrid_fine)", "value": dof, "unit": "DOF/s", "n_gpus": world,
            "level": level, "rank_grid": "%dx%dx%d" % pgrid, "cells_per_gpu": "%dx%dx%d" % (nx, ny, nz),
            "vcycles": iters, "ms_per_vcycle": t / iters * 1e3, "final_error": err,
            "halo_exchanges_per_vcycle": pd.exchanges / iters,
            "replicated_levels_from": pd.lrep,
            "roofline": {"bound": "hbm", "achieved": gbs / world, "peak": HBM_PEAK_GBS, "unit": "GB/s per GPU",
                         "frac": gbs / world / HBM_PEAK_GBS, "bytes_per_dof": BYTES_PER_DOF_VCYCLE}}


BYTES_PER_CELL_UPDATE_AMR = 84   # 80 B + 4 B of `son` per cell on AMR levels


def amr_sweep_bench(level=8, steps=5, partial=False):
    """The other sweep kernel of the path, for the record: godunov_fine of an AMR level through the tree-walking sweep
    (csrc/amr_sweep.hip: the level's octs in the reference's own cell vectors and tree arrays son/nbor/father); strict
    arithmetic.  One call = group build + (father-cell walk | oct records of primitive variables) + sweep + coarse
    corrections.  Two trees, octs numbered along a Z-order curve (what refine_fine produces):
      partial=False  a fully refined 2^level^3 level (the best case of the father-oct grouping);
      partial=True   level-1 fully refined and `level` present only in a spherical shell (where a blast wave refines):
                     a third of the father octs have fewer than 8 sons, the shell's two surfaces interpolate their ghost
                     octs from level-1, every oct on a surface owes fluxes to coarse cells."""
    import numpy as np
    import torch
    import ramses_amd
    from ramses_amd import ic
    from ramses_amd._capi import check, lib
    n = 2 ** level
    if partial:
        nc = n // 2
        z, y, x = np.meshgrid(np.arange(nc), np.arange(nc), np.arange(nc), indexing="ij")
        r = np.sqrt((x - nc / 2 + 0.5) ** 2 + (y - nc / 2 + 0.5) ** 2 + (z - nc / 2 + 0.5) ** 2)
        mask = (r >= 0.23 * nc) & (r <= 0.36 * nc)
        T = ic.uniform_tree(level - 1, order="morton", refine_mask=mask)
        igrid = T["igrid_fine"]
        # father octs (level-1 octs) by their number of sons
        fz, fy, fx = np.nonzero(mask)
        key = ((fz >> 1) * (nc // 2) + (fy >> 1)) * (nc // 2) + (fx >> 1)
        sons = np.bincount(key)
        sons = sons[sons > 0]
        census = {"father_octs": int(sons.size), "with_fewer_than_8_sons": int((sons < 8).sum())}
    else:
        T = ic.uniform_tree(level, order="morton")
        igrid = T["igrid"]
        census = None
    ncells = 8 * len(igrid)
    dx = 0.5 / n
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()  # noqa: E731
    # sedov3d.nml's state built on the device in the tree's cell vectors: rho = 1, P = 1e-5, the blast energy in one cell
    d_uold = torch.zeros((5, T["ncell"]), dtype=torch.float64, device="cuda")
    d_uold[0].fill_(1.0)
    d_uold[4].fill_(1e-5 / 0.4)
    d_uold[4, T["ncoarse"] + int(igrid[0]) - 1] = (1e-5 + 0.4 * 0.125 / dx ** 3) / 0.4
    d_unew = d_uold.clone()
    d_son, d_nbor, d_father, d_igrid = dev(T["son"]), dev(T["nbor"]), dev(T["father"]), dev(igrid)
    nw = lib().ramses_amd_godunov_fine_amr_workspace(len(igrid), T["ngridmax"])
    d_work = torch.zeros(int(nw), dtype=torch.uint8, device="cuda")
    d_err = torch.zeros(1, dtype=torch.int32, device="cuda")
    p = ramses_amd.make_params(courant_factor=0.8)
    ptr = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731

    def run():
        check(lib().ramses_amd_godunov_fine_amr_device(C.byref(p), level, len(igrid), ptr(d_igrid), ptr(d_son), ptr(d_nbor),
                                                       ptr(d_father), T["ngridmax"], T["ncoarse"], ptr(d_uold), ptr(d_unew),
                                                       None, None, None, dx, 1e-6, 32, 0, 1, ptr(d_work), ptr(d_err),
                                                       C.c_void_p(torch.cuda.current_stream().cuda_stream)))
    for _ in range(2):
        run()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(steps):
        run()
    b.record()
    torch.cuda.synchronize()
    ms = a.elapsed_time(b) / steps
    gbs = ncells * BYTES_PER_CELL_UPDATE_AMR / (ms * 1e-3) / 1e9
    out = {"metric": "cell-updates/s (godunov_fine of an AMR level, tree-walking sweep)", "value": ncells / (ms * 1e-3),
           "unit": "cell-updates/s", "ms_per_sweep": ms, "cells": ncells, "arithmetic": "strict (bit-identical to the reference)",
           "workload": ("level %d in a spherical shell over a fully refined level %d" % (level, level - 1)) if partial else
                       ("fully refined synthetic %d^3 tree" % n),
           "layout": "the reference's cell vectors and tree arrays, Z-order oct numbering",
           "tree_errors": int(d_err.item()),
           "roofline": {"bound": "hbm", "achieved": gbs, "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": gbs / HBM_PEAK_GBS,
                        "bytes_per_cell": BYTES_PER_CELL_UPDATE_AMR}}
    if census:
        out["census"] = census
    return out


def amr_resident_bench(level=8, steps=5, kind="covered"):
    """godunov_fine of a level of a RESIDENT AMR run (ramses_amd_amrres_godunov: the path the patched program takes).  The device
    numbers the octs itself -- levels in tiles of 32 x 4 x 4 octs (csrc/amr_layout.hpp) -- and sweeps such a level with the dense
    z-marching kernel in place (ghost octs interpolated into free tile slots, fluxes owed to the coarser level filed and
    computed by a surface pass and replayed); the same call with RAMSES_AMD_TILE_DENSE=0 / RAMSES_AMD_COVERED_DENSE=0 walks the tree on the same layout.
      kind="full"     level `level` complete, nothing finer                (the tree-walking sweep's best case)
      kind="covered"  level `level` complete, level+1 in a spherical shell (levelmin of an AMR run: refined cells inside)
      kind="partial"  level `level` in a spherical shell over a complete level-1 (ghost octs and coarse-fine fluxes on both surfaces)
    Strict arithmetic is the headline of each leg, the fast build (the drop-in's default) rides beside it.  Timed with events around the call (list upload, ghost pre-pass, sweep, replay)."""
    import numpy as np
    import torch
    import ramses_amd
    from ramses_amd import ic
    from ramses_amd._capi import check, lib
    Lfull = level - 1 if kind == "partial" else level
    n = 2 ** Lfull
    mask = None
    if kind != "full":
        z, y, x = np.meshgrid(np.arange(n), np.arange(n), np.arange(n), indexing="ij")
        r = np.sqrt((x - n / 2 + 0.5) ** 2 + (y - n / 2 + 0.5) ** 2 + (z - n / 2 + 0.5) ** 2)
        mask = (r >= 0.23 * n) & (r <= 0.36 * n)
        del x, y, z, r
    # room in ngridmax for the tiles of the partial level (a production namelist's ngridmax has that slack anyway)
    T = ic.uniform_tree(Lfull, order="morton", refine_mask=mask, slack=7 if mask is None else int(1.6 * mask.sum()) + 4096)
    igrid = np.ascontiguousarray(T["igrid_fine"] if kind == "partial" else T["igrid"])
    lists = [np.ascontiguousarray(T["igrid"])] + ([np.ascontiguousarray(T["igrid_fine"])] if mask is not None else [])
    ncells = 8 * len(igrid)
    dx = 0.5 / 2 ** level
    u = np.zeros((5, T["ncell"]))
    u[0] = 1.0
    u[4] = 1e-5 / 0.4
    u[4, T["ncoarse"] + int(igrid[0]) - 1] = (1e-5 + 0.4 * 0.125 / dx ** 3) / 0.4
    vp = lambda a: a.ctypes.data_as(C.c_void_p)      # noqa: E731
    L = lib()
    out = {}
    for tag, env, fast in (("dense", "1", False), ("dense_fast", "1", True), ("tree", "0", False)):
        p = ramses_amd.make_params(courant_factor=0.8, fast_math=fast, riemann=os.environ.get("RAMSES_AMD_BENCH_AMR_RIEMANN", "llf"))   # (probe: another solver on the tiles)
        os.environ["RAMSES_AMD_COVERED_DENSE"] = env
        os.environ["RAMSES_AMD_TILE_DENSE"] = env
        check(L.ramses_amd_amrres_invalidate())
        check(L.ramses_amd_amrres_load(5, T["ngridmax"], T["ncoarse"], vp(u), vp(T["son"]), vp(T["nbor"]), vp(T["father"])))
        before = L.ramses_amd_amrres_tile_sweeps()

        def one():
            for ig in lists:
                check(L.ramses_amd_amrres_set_unew(len(ig), vp(ig)))
        for _ in range(2):
            one()
            check(L.ramses_amd_amrres_godunov(C.byref(p), level, len(igrid), vp(igrid), dx, 1e-6, 32, 0, 1))
        torch.cuda.synchronize()
        t = 0.0
        for _ in range(steps):
            one()
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            a.record()
            check(L.ramses_amd_amrres_godunov(C.byref(p), level, len(igrid), vp(igrid), dx, 1e-6, 32, 0, 1))
            b.record()
            torch.cuda.synchronize()
            t += a.elapsed_time(b)
        out[tag] = (t / steps, L.ramses_amd_amrres_tile_sweeps() - before, L.ramses_amd_amrres_tiled_levels())
    os.environ.pop("RAMSES_AMD_COVERED_DENSE", None)
    os.environ.pop("RAMSES_AMD_TILE_DENSE", None)
    check(L.ramses_amd_amrres_invalidate())
    ms, took, tiled = out["dense"]
    ms_fast = out["dense_fast"][0]
    gbs = ncells * BYTES_PER_CELL_UPDATE_AMR / (ms * 1e-3) / 1e9
    work = {"full": "level %d complete (%d^3), nothing finer" % (level, 2 ** level),
            "covered": "level %d complete (%d^3), level %d in a spherical shell: %d of its cells refined" % (level, n, level + 1, 0 if mask is None else int(mask.sum())),
            "partial": "level %d in a spherical shell (%d cells) over a complete level %d" % (level, ncells, level - 1)}[kind]
    return {"metric": "cell-updates/s (godunov_fine of a level of a resident AMR run, dense sweep on the device's tiles)",
            "value": ncells / (ms * 1e-3), "unit": "cell-updates/s", "ms_per_sweep": ms, "cells": ncells,
            "dense_sweeps_taken": int(took), "levels_in_tiles": int(tiled), "tree_walking_ms_per_sweep": out["tree"][0],
            "tree_walking_frac": ncells * BYTES_PER_CELL_UPDATE_AMR / (out["tree"][0] * 1e-3) / 1e9 / HBM_PEAK_GBS,
            "arithmetic": "strict (bit-identical to the reference)", "workload": work,
            "fast_arithmetic": {"ms_per_sweep": ms_fast, "value": ncells / (ms_fast * 1e-3),
                                "frac": ncells * BYTES_PER_CELL_UPDATE_AMR / (ms_fast * 1e-3) / 1e9 / HBM_PEAK_GBS,
                                "note": "the patched program's default on tiled levels (<= 1e-12 of the reference: tests/test_fast_certificate_gpu.py)"},
            "layout": "device numbering: tiles of 32x4x4 octs (csrc/amr_layout.hpp); host tree numbered along a Z-order curve",
            "includes": "oct list upload, ghost-oct interpolation pre-pass, the surface pass (fluxes owed to the coarser level), the dense sweep in place on the cell vectors, the replay of the "
                        "fluxes owed to the coarser level; HIP events around ramses_amd_amrres_godunov",
            "roofline": {"bound": "hbm", "achieved": gbs, "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": gbs / HBM_PEAK_GBS,
                         "bytes_per_cell": BYTES_PER_CELL_UPDATE_AMR}}


def amr_c5_shape_bench(steps=5):
    """BASELINE config C5 in its REAL shape (sedov3d.nml, levelmin=7, levelmax=10, 8 ranks), one rank's share of one coarse step:
    the rank's octant of levelmin (32768 of the 262144 octs of level 7: a list that is part of the level, the rest are its
    neighbours' octs) and three small levels around the blast -- ~1000 octs each at levels 8, 9, 10 -- with the reference's
    sub-cycling (nsubcycle=2: 1 + 2 + 4 + 8 = 15 godunov_fine calls, each between its set_unew and set_uold, in amr_step's order).
    The small levels take the tree-walking sweep (below RAMSES_AMD_TILE_MIN_OCTS = 32768 octs a level is a few launches of
    latency, not of work); reported: ms per coarse step of the hydro calls, and the same with every level forced onto tiles."""
    import numpy as np
    import torch
    import ramses_amd
    from ramses_amd import ic
    from ramses_amd._capi import check, lib
    L, n = 7, 128

    def sph(m, c, r):
        z, y, x = np.meshgrid(np.arange(m), np.arange(m), np.arange(m), indexing="ij")
        return ((x - c + 0.5) ** 2 + (y - c + 0.5) ** 2 + (z - c + 0.5) ** 2) < r * r
    T = ic.uniform_tree(L, order="morton", refine_mask=sph(n, 32, 6.2), refine_mask2=sph(2 * n, 64, 6.2), refine_mask3=sph(4 * n, 128, 6.2), slack=300000)
    # the rank's share of levelmin: the octs of the octant that holds the blast (level-7 octs sit at level-6 cell positions)
    ig7 = np.sort(T["igrid"])
    no = 2 ** (L - 1)
    # Z-order numbering: the first eighth of the level's octs is the low octant
    own7 = np.ascontiguousarray(ig7[: len(ig7) // 8])
    lists = {7: own7, 8: np.ascontiguousarray(np.sort(T["igrid_fine"])), 9: np.ascontiguousarray(np.sort(T["igrid_fine2"])),
             10: np.ascontiguousarray(np.sort(T["igrid_fine3"]))}
    alls = dict(lists)
    alls[7] = np.ascontiguousarray(ig7)
    u = np.zeros((5, T["ncell"]))
    u[0] = 1.0
    u[4] = 1e-5 / 0.4
    u[4, T["ncoarse"] + int(lists[10][0]) - 1] = (1e-5 + 0.4 * 0.125 / (0.5 / 2 ** 10) ** 3) / 0.4
    vp = lambda a: a.ctypes.data_as(C.c_void_p)      # noqa: E731
    Lb = lib()
    p = ramses_amd.make_params(courant_factor=0.8, fast_math=True)
    out = {}
    ncalls = [0]

    def amr_step(lev, dt):
        check(Lb.ramses_amd_amrres_set_unew(len(alls[lev]), vp(alls[lev])))
        if lev < 10:
            amr_step(lev + 1, dt / 2)
            amr_step(lev + 1, dt / 2)
        check(Lb.ramses_amd_amrres_godunov(C.byref(p), lev, len(lists[lev]), vp(lists[lev]), 0.5 / 2 ** lev, dt, 32, 0, 1))
        ncalls[0] += 1
        check(Lb.ramses_amd_amrres_set_uold(C.byref(p), len(alls[lev]), vp(alls[lev])))
    for tag, min_octs in (("production", None), ("all_levels_on_tiles", "0")):
        if min_octs is None:
            os.environ.pop("RAMSES_AMD_TILE_MIN_OCTS", None)
        else:
            os.environ["RAMSES_AMD_TILE_MIN_OCTS"] = min_octs
        check(Lb.ramses_amd_amrres_invalidate())
        check(Lb.ramses_amd_amrres_load(5, T["ngridmax"], T["ncoarse"], vp(u), vp(T["son"]), vp(T["nbor"]), vp(T["father"])))
        t0, d0 = Lb.ramses_amd_amrres_tree_sweeps(), Lb.ramses_amd_amrres_tile_sweeps()
        amr_step(7, 1e-7)
        amr_step(7, 1e-7)
        torch.cuda.synchronize()
        ncalls[0] = 0
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        w0 = time.perf_counter()
        a.record()
        for _ in range(steps):
            amr_step(7, 1e-7)
        b.record()
        torch.cuda.synchronize()
        out[tag] = {"ms_per_coarse_step": a.elapsed_time(b) / steps, "host_ms_per_coarse_step": (time.perf_counter() - w0) / steps * 1e3,
                    "godunov_calls_per_coarse_step": ncalls[0] // steps,
                    "tree_walking_sweeps": int(Lb.ramses_amd_amrres_tree_sweeps() - t0), "dense_sweeps": int(Lb.ramses_amd_amrres_tile_sweeps() - d0)}
    os.environ.pop("RAMSES_AMD_TILE_MIN_OCTS", None)
    check(Lb.ramses_amd_amrres_invalidate())
    cells = 8 * sum(len(lists[l]) * 2 ** (l - 7) for l in lists)        # cell updates of one coarse step (sub-cycling)
    ms = out["production"]["ms_per_coarse_step"]
    return {"metric": "ms per coarse step of one rank's share of BASELINE config C5 (set_unew + godunov_fine + set_uold, levels 7-10, sub-cycled)",
            "value": ms, "unit": "ms", "octs_per_level": {str(l): int(len(lists[l])) for l in lists}, "cell_updates_per_coarse_step": int(cells),
            "cell_updates_per_s": cells / (ms * 1e-3), "arithmetic": "fast on tiled levels (the drop-in's default), strict in the tree-walking sweep",
            "production": out["production"], "all_levels_on_tiles": out["all_levels_on_tiles"],
            "note": "levels 8-10 hold ~1000 octs each: their 14 sweeps per coarse step are launch latency, not work; levelmin's octant (32768 octs) "
                    "takes the dense sweep on tiles"}


BYTES_PER_CELL_UPDATE_MHD = 176   # 11 fields (5 Euler + 3 left-face + 3 right-face fields) read and written, FP64


def solver_sweep_bench(n, riemann="hllc", slope_type=1, steps=10):
    """The dense sweep of the same uniform level with another solver of the fast (default) build -- HLLC is what most production
    namelists choose; the headline line is sedov3d.nml's own LLF + minmod.  Timed with HIP events on torch's stream after 20
    untimed sweeps; sedov3d.nml's initial state (csrc/hydro_core.hpp hllc_flux_fast; profiles/r06_hllc_fast.txt)."""
    import torch
    import ramses_amd
    from ramses_amd import ic
    from ramses_amd.hydro import HydroLevel
    p = ramses_amd.make_params(courant_factor=0.8, fast_math=True, riemann=riemann, slope_type=slope_type)
    lev = HydroLevel(n, n, n, 0.5 / n, params=p, ng=0)
    corner, back, dx = ic.sedov3d_corner_and_background(n)
    for v in range(5):
        lev.uold[v].fill_(float(back[v]))
        lev.uold[v, 0, 0, 0] = float(corner[v])
    dt = lev.courant_fine()[0]
    for _ in range(20):
        lev.step(dt)
    torch.cuda.synchronize()
    a, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(steps):
        lev.step(dt)
    e.record()
    torch.cuda.synchronize()
    ms = a.elapsed_time(e) / steps
    assert bool(torch.isfinite(lev.uold).all().item())
    gbs = n ** 3 * BYTES_PER_CELL_UPDATE / (ms * 1e-3) / 1e9
    return {"metric": "cell-updates/s (Godunov sweep)", "value": n ** 3 / (ms * 1e-3), "unit": "cell-updates/s", "ms_per_sweep": ms,
            "solver": "%s, slope_type %d" % (riemann, slope_type), "arithmetic": "fast (the patched program's default)",
            "workload": "sedov3d.nml uniform %d^3, 20 sweeps in" % n,
            "roofline": {"bound": "hbm", "achieved": gbs, "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": gbs / HBM_PEAK_GBS}}


def mhd_sweep_bench(level=7, steps=5):
    """SOLVER=mhd: the constrained-transport MHD sweep of a uniform periodic 2^level^3 level through
    ramses_amd_mhd_godunov_brick (csrc/mhd_sweep.hip: the first correct path, one kernel per stage of mag_unsplit with the
    intermediates in HBM); hlld + hlld, moncen, a magnetised blast; strict arithmetic (bit-identical to the reference)."""
    import numpy as np
    import torch
    from ramses_amd.mhd import MhdLevel, make_mhd_params
    n = 2 ** level
    lev = MhdLevel(n, n, n, 1.0 / n, params=make_mhd_params(gamma=5.0 / 3.0, slope_type=2, riemann="hlld", riemann2d="hlld"))
    x = (torch.arange(n, dtype=torch.float64, device="cuda") + 0.5) / n
    Z, Y, X = torch.meshgrid(x, x, x, indexing="ij")
    r2 = (X - 0.5) ** 2 + (Y - 0.5) ** 2 + (Z - 0.5) ** 2
    b = (1.0, 0.5, -0.3)
    lev.uold[0].fill_(1.0)
    for c in range(3):
        lev.uold[5 + c].fill_(b[c])
        lev.uold[8 + c].fill_(b[c])
    lev.uold[4] = (0.1 + 10.0 * torch.exp(-r2 / (2 * 0.05 ** 2))) / (5.0 / 3.0 - 1.0) + 0.5 * sum(v * v for v in b)
    dt = 0.2 / n / 5.0
    for _ in range(2):
        lev.step(dt)
    torch.cuda.synchronize()
    a, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(steps):
        lev.step(dt)
    e.record()
    torch.cuda.synchronize()
    ms = a.elapsed_time(e) / steps
    assert bool(torch.isfinite(lev.uold).all().item())
    cells = n ** 3
    gbs = cells * BYTES_PER_CELL_UPDATE_MHD / (ms * 1e-3) / 1e9
    # the same sweep in the fast arithmetic (ramses_amd_mhd_godunov_brick_fast; RAMSES_AMD_MHD_FAST=1 routes the entry point)
    fast = None
    saved = os.environ.get("RAMSES_AMD_MHD_FAST")
    os.environ["RAMSES_AMD_MHD_FAST"] = "1"
    try:
        for _ in range(2):
            lev.step(dt)
        torch.cuda.synchronize()
        a.record()
        for _ in range(steps):
            lev.step(dt)
        e.record()
        torch.cuda.synchronize()
        msf = a.elapsed_time(e) / steps
        assert bool(torch.isfinite(lev.uold).all().item())
        fast = {"ms_per_sweep": msf, "value": cells / (msf * 1e-3), "frac": cells * BYTES_PER_CELL_UPDATE_MHD / (msf * 1e-3) / 1e9 / HBM_PEAK_GBS,
                "arithmetic": "fast (v_rcp_f64 + Newton divisions, contracted multiply-adds; <= 1e-12 of the reference program: "
                              "tests/test_mhd_fast_certificate_gpu.py)"}
    finally:
        if saved is None:
            os.environ.pop("RAMSES_AMD_MHD_FAST", None)
        else:
            os.environ["RAMSES_AMD_MHD_FAST"] = saved
    return {"metric": "cell-updates/s (MHD godunov_fine, SOLVER=mhd, constrained transport)", "value": cells / (ms * 1e-3),
            "fast_arithmetic": fast,
            "unit": "cell-updates/s", "ms_per_sweep": ms, "cells": cells, "solver": "hlld + hlld (2-D), moncen",
            "arithmetic": "strict (bit-identical to the reference)", "workload": "uniform periodic %d^3, magnetised blast" % n,
            "kernels": "mhd_prim_trace (ctoprim + edge fields + trace fused over LDS tiles, round 6) / flux / emf / update; the 47 predicted numbers, "
                       "the fluxes and the EMFs still cross HBM",
            "roofline": {"bound": "hbm", "achieved": gbs, "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": gbs / HBM_PEAK_GBS,
                         "bytes_per_cell": BYTES_PER_CELL_UPDATE_MHD}}


def pick_transport(rank, world, timeout):
    """RCCL is the transport.  Before anything is measured every rank exercises it once (an
    all-reduce and a ring send/recv of device tensors); the verdicts are combined over a gloo
    group.  If RCCL does not work on this node the exchange falls back to host-staged gloo --
    slower, still a valid whole-job number, and the JSON line says so."""
    import torch
    import torch.distributed as dist
    from ramses_amd.transport import DistTransport
    try:
        gloo = dist.new_group(backend="gloo", timeout=timeout)
    except Exception as exc:     # noqa: BLE001  (no usable interface for gloo: nothing to fall back to)
        sys.stderr.write("bench.py rank %d: no gloo group (%s); RCCL without self-test\n" % (rank, str(exc)[:120]))
        return DistTransport(), None
    ok, why = 1, ""
    try:
        tr = DistTransport()
        t = torch.ones(4, dtype=torch.float64, device="cuda")
        dist.all_reduce(t)
        recv = torch.zeros(1024, dtype=torch.float64, device="cuda")
        send = torch.full((1024,), float(rank), dtype=torch.float64, device="cuda")
        tr.sendrecv([(send, (rank + 1) % world)], [(recv, (rank - 1) % world)])
        torch.cuda.synchronize()
        if float(t[0].item()) != world or float(recv[0].item()) != (rank - 1) % world:
            ok, why = 0, "wrong data"
    except Exception as exc:     # noqa: BLE001
        ok, why = 0, str(exc)[:160]
    flag = torch.tensor([ok], dtype=torch.int32)
    dist.all_reduce(flag, op=dist.ReduceOp.MIN, group=gloo)
    if int(flag.item()) == 1:
        # RCCL works on this node: move the neighbour exchange behind the C ABI (the library's own RCCL
        # communicator, the entry the Fortran drop-in uses), with the same self-test; torch's RCCL
        # send/recv remains the fallback
        ok2, why2, tr2 = 1, "", None
        if os.environ.get("RAMSES_AMD_BENCH_TRANSPORT", "capi") == "capi":
            try:
                from ramses_amd.transport import RcclTransport
                tr2 = RcclTransport()
                recv = torch.zeros(1024, dtype=torch.float64, device="cuda")
                send = torch.full((1024,), float(rank), dtype=torch.float64, device="cuda")
                tr2.sendrecv([(send, (rank + 1) % world)], [(recv, (rank - 1) % world)])
                torch.cuda.synchronize()
                if float(recv[0].item()) != (rank - 1) % world:
                    ok2, why2 = 0, "wrong data"
            except Exception as exc:     # noqa: BLE001
                ok2, why2 = 0, str(exc)[:160]
        else:
            ok2, why2 = 0, "disabled by RAMSES_AMD_BENCH_TRANSPORT"
        flag2 = torch.tensor([ok2], dtype=torch.int32)
        dist.all_reduce(flag2, op=dist.ReduceOp.MIN, group=gloo)
        if int(flag2.item()) == 1:
            return tr2, "RCCL send/recv behind the C ABI (ramses_amd_rccl_sendrecv, the library's own communicator)"
        if why2:
            sys.stderr.write("bench.py rank %d: C-ABI RCCL transport not used: %s\n" % (rank, why2))
        return DistTransport(), None
    if why:
        sys.stderr.write("bench.py rank %d: RCCL self-test failed: %s\n" % (rank, why))
    return DistTransport(group=gloo, staged=True), "gloo send/recv staged through the host (the RCCL self-test failed on this node)"


def main():
    args = parse()
    import torch
    import torch.distributed as dist
    import ramses_amd
    from ramses_amd import ic
    from ramses_amd.hydro import HydroLevel
    from ramses_amd._capi import lib, check

    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    assert world == args.gpus, "launch with torch.distributed.run --nproc-per-node %d" % args.gpus
    # RAMSES_AMD_DIST_BACKEND=gloo: smoke-test the multi-rank path with all ranks on
    # one GPU (tensors staged through the host); never a measurement
    backend = os.environ.get("RAMSES_AMD_DIST_BACKEND", "nccl")
    # "nccl-shared": RCCL with several ranks on one GPU -- it must refuse, which exercises the fallback
    local_dev = local_rank % torch.cuda.device_count() if backend != "nccl" else local_rank
    torch.cuda.set_device(local_dev)
    transport, transport_note = None, None
    if world > 1:
        import datetime
        import threading

        def abandon():
            # a collective that never returns (RCCL bootstrap, a lost peer): say so and leave
            sys.stderr.write("bench.py rank %d: no result after %d s, giving up\n" % (rank, args.deadline))
            if rank == 0:
                print(json.dumps({"metric": "cell-updates/s (Godunov sweep), uniform Sedov3D", "value": None,
                                  "unit": "cell-updates/s", "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
                                  "error": "run abandoned after %d s (hung collective?)" % args.deadline}), flush=True)
            os._exit(3)

        watchdog = threading.Timer(args.deadline, abandon)
        watchdog.daemon = True
        watchdog.start()
        if backend == "nccl":
            dist.init_process_group("nccl", device_id=torch.device("cuda", local_dev))
            transport, transport_note = pick_transport(rank, world, datetime.timedelta(seconds=120))
        elif backend == "nccl-shared":
            dist.init_process_group("nccl")
            transport, transport_note = pick_transport(rank, world, datetime.timedelta(seconds=120))
        else:
            dist.init_process_group(backend)
            transport_note = "%s send/recv staged through the host (smoke-test mode, not a measurement)" % backend

    n = args.n
    pgrid = rank_grid(world)
    if args.zchunk or args.tile_rows:
        check(lib().ramses_amd_godunov_tune(args.tile_rows, args.zchunk))
    if args.mg_tune >= 0:
        check(lib().ramses_amd_mg_tune(args.mg_tune))
    params = ramses_amd.make_params(courant_factor=0.8, fast_math=bool(args.fast))
    if world == 1:
        lev = HydroLevel(n, n, n, 0.5 / n, params=params, ng=0)
        u, dx = ic.sedov3d(n) if n <= 256 else (None, 0.5 / n)
        if u is None:
            # sedov3d.nml built on the device (no 5 GB host array): the reference's IC is a uniform background plus ONE cell --
            # the 'point' region sits at the box corner and its non-periodic CIC cloud keeps cell (0,0,0) only
            # (ic.sedov3d_corner_and_background, hydro/init_flow_fine.f90:555-594; tests/test_ic_sedov.py)
            corner, back, dx = ic.sedov3d_corner_and_background(n)
            for v in range(5):
                lev.uold[v].fill_(float(back[v]))
                lev.uold[v, 0, 0, 0] = float(corner[v])
        else:
            lev.upload(u)
        exchange = None
    else:
        from ramses_amd.parallel import BrickDecomposition
        dec = BrickDecomposition(pgrid, rank, n, boxlen=0.5 * pgrid[0], transport=transport)
        lev = dec.make_level(params)
        dec.init_sedov(lev)
        exchange = dec
        dx = lev.dx
        exchange.make_virtual_fine_dp(lev)

    # one CFL step size for the whole run (min over ranks): dt only shrinks the
    # update, never changes the work per cell
    dt = lev.courant_fine()[0]
    if world > 1:
        dt = exchange.transport.allreduce(dt, "cuda", op="min")

    def step(ovl):
        if ovl:
            exchange.step_overlapped(lev, dt)     # halo exchange hidden behind the interior sweep
        else:
            lev.godunov_fine(dt)
            lev.set_uold()
            if exchange is not None:
                exchange.make_virtual_fine_dp(lev)

    # N>1: the split sweep (shell + interior) costs ~0.7 ms at 512^3; hiding the exchange
    # behind the interior pays only if the exchange is slower than that on this node.
    # Measure both schedules (untimed, max over ranks) and keep the faster one.
    overlap = False
    tune = None
    if exchange is not None and args.no_overlap:
        pass
    elif exchange is not None and args.overlap in ("on", "off"):
        overlap = args.overlap == "on"
    elif exchange is not None:
        tune = {}
        for mode in (False, True):
            for _ in range(2):
                step(mode)
            exchange.transport.barrier()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(4):
                step(mode)
            torch.cuda.synchronize()
            tune[mode] = exchange.transport.allreduce((time.perf_counter() - t0) / 4, "cuda", op="max")
        overlap = tune[True] < tune[False]

    # Ramp: the first ~8 sweeps of THIS kernel at THIS size run up to 10 % slower (per-step kernel times of a run that goes
    # straight into its timed steps: 3.54, 3.44, 3.35, 3.29, 3.24, 3.22 ... ms, RAMSES_AMD_BENCH_STEPS=1), and keeping another
    # kernel busy beforehand does not change that (the strict build on a 256^3 scratch level, round 2's spin-up, for 150, 600
    # or 1500 ms: the same five slow steps, profiles/r03_spinup_ab.txt) -- the power management follows the load of the kernel
    # that runs.  A run of the reference lasts hours, so the steady state is the honest number: the SAME sweep (same build,
    # same brick size) is kept busy on scratch buffers for --spinup-ms first.  Not a step of the workload (its state and
    # buffers are untouched); W and K below are exactly the requested ones; reported in `config`.
    spin_sweeps = 0
    if args.spinup_ms > 0:
        spin = HydroLevel(n, n, n, lev.dx, params=ramses_amd.make_params(courant_factor=0.8, fast_math=bool(args.fast)), ng=lev.ng)
        spin.uold[0].fill_(1.0)
        spin.uold[4].fill_(2.5)
        t_spin = time.perf_counter()
        while (time.perf_counter() - t_spin) * 1e3 < args.spinup_ms:
            for _ in range(8):
                spin.godunov_fine(1e-6 * lev.dx)
                spin.set_uold()
            spin_sweeps += 8
            torch.cuda.synchronize()
        del spin
        torch.cuda.empty_cache()

    for _ in range(args.warmup):
        step(overlap)

    # ---- timed region --------------------------------------------------------
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(args.steps)]
    if world > 1:
        exchange.transport.barrier()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i in range(args.steps):
        ev[i][0].record()           # same (current) stream the kernels launch on
        if overlap:
            exchange.step_overlapped(lev, dt)
            ev[i][1].record()       # sweep launches + wait for the hidden exchange
        else:
            lev.godunov_fine(dt)
            ev[i][1].record()
            lev.set_uold()
            if exchange is not None:
                exchange.make_virtual_fine_dp(lev)
    torch.cuda.synchronize()
    if world > 1:
        exchange.transport.barrier()
    t1 = time.perf_counter()
    elapsed = t1 - t0
    if world > 1:
        elapsed = exchange.transport.allreduce(elapsed, "cuda", op="max")
    kern_ms = sum(a.elapsed_time(b) for a, b in ev) / args.steps
    if os.environ.get("RAMSES_AMD_BENCH_STEPS"):      # debugging aid: the kernel time of every timed step
        sys.stderr.write("bench.py rank %d: ms per step %s\n" % (rank, " ".join("%.3f" % a.elapsed_time(b) for a, b in ev)))
    # the state of the last timed step, before anything below sweeps the level again
    dumped = dump_outputs(lev, args.dump_outputs, world, rank) if args.dump_outputs else None

    # N>1: where a step's time goes (untimed extra steps of the serial schedule, an event after every stage; max over ranks)
    breakdown = None
    if exchange is not None:
        acc = {"sweep": 0.0, "pack": 0.0, "sendrecv": 0.0, "unpack": 0.0}
        nprof, nbytes = 5, 0
        for _ in range(nprof):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            lev.godunov_fine(dt)
            b.record()
            lev.set_uold()
            pk, sr, up, nbytes = exchange.exchange_direct_profiled(lev, lev.uold, lev.nvar)
            torch.cuda.synchronize()
            acc["sweep"] += a.elapsed_time(b); acc["pack"] += pk; acc["sendrecv"] += sr; acc["unpack"] += up
        breakdown = {k + "_ms": exchange.transport.allreduce(v / nprof, "cuda", op="max") for k, v in acc.items()}
        breakdown["bytes_sent_per_rank"] = nbytes
        breakdown["bytes_to_peer_of_rank0"] = {str(k): v for k, v in sorted(getattr(exchange, "last_bytes_per_peer", {}).items())}
        if tune is not None:
            breakdown["schedule"] = {"serial_ms_per_step": tune[False] * 1e3, "overlapped_ms_per_step": tune[True] * 1e3,
                                     "chosen": "overlapped" if overlap else "serial"}
        breakdown["sendrecv_GBps_per_rank"] = nbytes / max(breakdown["sendrecv_ms"], 1e-9) / 1e6
        breakdown["note"] = ("%d extra steps of the serial schedule after the timed region: full-brick sweep, pack of the 26 regions, one "
                             "grouped send/recv (one message per peer), unpack; each stage between events on the launch stream, max over ranks"
                             % nprof)

    # sanity: the state must still be physical
    chk = lev.courant_fine()
    assert chk[0] > 0 and chk[1] > 0

    census = rank_census(rank, world, local_dev, transport_note, getattr(transport, "group", None))     # collective
    # Every rank on a device of its own and the exchange NOT behind the C ABI on every rank: the line measures a transport the
    # Fortran drop-in does not use (torch's RCCL, or gloo through the host).  Said loudly -- on stderr and in the line's
    # `config.transport_warning` -- next to the number; RAMSES_AMD_BENCH_STRICT_TRANSPORT=1 makes it a failed run instead
    # (value null, exit code 5).
    fallback_error = None
    if world > 1 and backend == "nccl" and census["distinct_devices"] == world and census["library_rccl_ranks"] != world:
        fallback_error = ("%d ranks on %d distinct devices, but the library's own RCCL communicator is up on %d of them: the exchange ran "
                          "through %s, not through ramses_amd_rccl_sendrecv" % (world, census["distinct_devices"], census["library_rccl_ranks"],
                                                                                census["transport"]))
        sys.stderr.write("bench.py rank %d: WARNING: %s\n" % (rank, fallback_error))
        if os.environ.get("RAMSES_AMD_BENCH_STRICT_TRANSPORT", "0") == "1":
            if rank == 0:
                print(json.dumps({"metric": "cell-updates/s (Godunov sweep), uniform Sedov3D", "value": None, "unit": "cell-updates/s",
                                  "n_gpus": world, "steps": args.steps, "warmup": args.warmup, "error": fallback_error,
                                  "config": {"ranks": census, "step_breakdown": breakdown}}), flush=True)
            if world > 1:
                dist.destroy_process_group()
            sys.exit(5)
    if rank == 0:
        cells = n ** 3
        value = cells * world * args.steps / elapsed
        traffic, traffic_src = pmc_traffic(n, world, args)
        achieved = cells * BYTES_PER_CELL_UPDATE / (kern_ms * 1e-3) / 1e9
        out = {
            "metric": "cell-updates/s (Godunov sweep), uniform Sedov3D",
            "value": value, "unit": "cell-updates/s", "n_gpus": world, "steps": args.steps,
            "warmup": args.warmup, "ms_per_step": elapsed / args.steps * 1e3,
            "higher_is_better": True, "scaling": "weak", "vs_baseline": None,
            "dtype": "f64", "data": "synthetic",
            "config": {"workload": "sedov3d.nml uniform %d^3 per GPU (%dx%dx%d ranks, global %dx%dx%d), "
                                   "hydro-only Godunov sweep, LLF + minmod, muscl"
                                   % (n, pgrid[0], pgrid[1], pgrid[2], n * pgrid[0], n * pgrid[1], n * pgrid[2]),
                       "arithmetic": "fast = the patched program's default (explicit FMAs, rcp/rsq + Newton; rel-Linf of the REFERENCE PROGRAM "
                                     "<= 4e-15 at 256^3 over 100 steps and at 128^3 over 120 steps, bound 1e-12: tests/test_fast_certificate_gpu.py; "
                                     "RAMSES_AMD_STRICT=1 selects the bit-identical build)" if args.fast else "strict (bit-identical to the reference)",
                       "spinup": "%d untimed sweeps of the same kernel on a scratch level of the same size before the warm-up steps (%d ms; the first ~8 "
                                 "sweeps of a kernel run up to 10 %% slower whatever ran before: profiles/r03_spinup_ab.txt)" % (spin_sweeps, args.spinup_ms),
                       "ranks": census,
                       "transport_warning": fallback_error,
                       "step_breakdown": breakdown,
                       "halo": "none (single rank, in-kernel periodic wrap)" if world == 1 else
                               ("RCCL send/recv (torch.distributed)" if transport_note is None else transport_note) +
                               " of 2-cell face slabs, all nvar fused, " +
                               "one grouped exchange of all 26 neighbour regions (one message per peer), " +
                               ("overlapped with the interior sweep on a second stream" if overlap else "after the sweep") +
                               ("" if tune is None else " (auto-selected: serial %.3f ms/step, overlapped %.3f ms/step)"
                                % (tune[False] * 1e3, tune[True] * 1e3))},
            "roofline": {"bound": "hbm", "achieved": achieved, "peak": HBM_PEAK_GBS, "unit": "GB/s",
                         "frac": achieved / HBM_PEAK_GBS, "traffic": traffic, "traffic_source": traffic_src,
                         "kernel": "godunov_sweep_kernel", "kernel_ms": kern_ms,
                         "algorithmic_bytes_per_launch": cells * BYTES_PER_CELL_UPDATE},
        }
        if dumped is not None:
            out["dumped_outputs"] = {"dir": args.dump_outputs, "files": dumped}
        if world == 1 and args.fast:
            # the other build of the same kernel, for the record: strict arithmetic
            # (bit-identical to the reference), a few launches after the timed region
            lev.params.fast_math = 0
            for _ in range(2):
                lev.godunov_fine(dt)
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(5):
                lev.godunov_fine(dt)
            b.record()
            torch.cuda.synchronize()
            ms = a.elapsed_time(b) / 5
            gbs = cells * BYTES_PER_CELL_UPDATE / (ms * 1e-3) / 1e9
            out["strict_build"] = {"kernel_ms": ms, "cell_updates_per_s": cells / (ms * 1e-3), "achieved": gbs,
                                   "unit": "GB/s", "frac": gbs / HBM_PEAK_GBS,
                                   "note": "same kernel, -ffp-contract=off and the reference's operation order: bit-identical results"}
            lev.params.fast_math = 1
        if world == 1 and args.stress_steps > 0:
            # the same kernel on a DEVELOPED state (SURVEY.md 8d's stress variant, "step >= 50"): the run goes on with the
            # Courant step of every step until it has taken stress_steps steps in all, then K sweeps are timed
            done = args.warmup + args.steps
            dts = dt
            while done < args.stress_steps:
                dts = lev.courant_fine()[0]
                lev.step(dts)
                done += 1
            dts = lev.courant_fine()[0]
            torch.cuda.synchronize()
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(10):
                lev.godunov_fine(dts)
            b.record()
            torch.cuda.synchronize()
            ms = a.elapsed_time(b) / 10
            gbs = cells * BYTES_PER_CELL_UPDATE / (ms * 1e-3) / 1e9
            out["stress"] = {"after_steps": done, "kernel_ms": ms, "cell_updates_per_s": cells / (ms * 1e-3), "achieved": gbs, "unit": "GB/s",
                             "frac": gbs / HBM_PEAK_GBS, "arithmetic": "fast" if args.fast else "strict",
                             "note": "10 sweeps of the state the run reaches after that many Courant-limited steps (blast wave developed: "
                                     "limiter and floor branches warm where it is)"}
            lev.params.fast_math = 1
        if world == 1 and args.vcycle_level > 0:
            del lev
            torch.cuda.empty_cache()
            out["vcycle"] = vcycle_bench(args.vcycle_level)
        if world == 1 and args.amr_level > 0:
            try:
                torch.cuda.empty_cache()
                # the resident path (what the patched program runs): device numbering in tiles + the dense sweep in place;
                # the tree-walking kernel on the host's own numbering beside it
                out["amr_sweep"] = amr_resident_bench(args.amr_level, kind="full")
                out["amr_sweep_partial"] = amr_resident_bench(args.amr_level + 1, kind="partial")
                out["amr_sweep_covered"] = amr_resident_bench(args.amr_level, kind="covered")
                try:
                    out["amr_c5_shape"] = amr_c5_shape_bench()
                except Exception as exc:     # noqa: BLE001
                    out["amr_c5_shape"] = {"value": None, "error": str(exc)[:300]}
                torch.cuda.empty_cache()
                out["amr_sweep_tree_walking"] = amr_sweep_bench(args.amr_level)
                out["amr_sweep_partial_tree_walking"] = amr_sweep_bench(args.amr_level + 1, partial=True)
            except Exception as exc:     # noqa: BLE001  (an extra line, never a reason to lose the headline)
                out.setdefault("amr_sweep", {"value": None})["error"] = str(exc)[:300]
        if world == 1 and args.stress_steps > 0:      # (with the other extra legs of a default run)
            try:
                torch.cuda.empty_cache()
                out["hllc_sweep"] = solver_sweep_bench(n, "hllc", 1)
            except Exception as exc:     # noqa: BLE001  (an extra line, never a reason to lose the headline)
                out["hllc_sweep"] = {"value": None, "error": str(exc)[:300]}
        if world == 1 and args.mhd_level > 0:
            try:
                torch.cuda.empty_cache()
                out["mhd_sweep"] = mhd_sweep_bench(args.mhd_level)
            except Exception as exc:     # noqa: BLE001  (an extra line, never a reason to lose the headline)
                out["mhd_sweep"] = {"value": None, "error": str(exc)[:300]}
        if world == 1 and not args.no_cpu_baseline:
            out["cpu_baseline"] = cpu_baseline()     # rank 0 at N=1 only
            if isinstance(out.get("vcycle"), dict) and out["vcycle"].get("value"):
                out["vcycle"]["cpu_baseline"] = vcycle_cpu_baseline()
    else:
        out = None

    if world > 1 and args.vcycle_level > 0:
        # second metric on several GPUs; collective, and guarded: whatever happens in
        # it, the headline line is printed (a watchdog ends every rank after the deadline)
        import threading
        note = {"metric": "V-cycle DOF/s (multigrid_fine)", "value": None}

        def bail():
            if rank == 0:
                note["error"] = "distributed V-cycle leg exceeded %d s" % args.vcycle_deadline
                out["vcycle"] = note
                print(json.dumps(out), flush=True)
            os._exit(0)

        wd = threading.Timer(args.vcycle_deadline, bail)
        wd.daemon = True
        wd.start()
        try:
            del lev, exchange, dec
            torch.cuda.empty_cache()
            vc = vcycle_bench_dist(args.vcycle_level, rank, world, transport)
        except Exception as exc:
            vc = dict(note, error=str(exc)[:300])
        wd.cancel()
        if rank == 0:
            out["vcycle"] = vc
    if rank == 0:
        print(json.dumps(out), flush=True)
    if world > 1:
        try:
            dist.destroy_process_group()
        except Exception:
            pass


if __name__ == "__main__":
    main()
