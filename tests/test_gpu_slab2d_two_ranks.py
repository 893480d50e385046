"""2-D grids cut along y over TWO RANKS through the C++ host loop (pion_host::sim_control_gpu: split stages, two
streams, request_min / allreduce_min), as two processes -- the 2-D counterpart of tests/test_gpu_host_two_ranks.py.

  * one GPU (always runs): transport pion_host::slab_comm_shm, both ranks on device 0; 3 steps, bit for bit against the
    single-domain GPU run, simtime ==;
  * two or more GPUs (skipped on a one-GPU box): the same cases over pion_host::slab_comm_rccl, one rank per device.

Every grid whose positions enter the solve (the (z,R) grids, the DMACH face) has dyadic dx and xmin, so that a slab's cell positions xmin_slab + (2 j + 1) dx / 2 are exactly the single
grid's (DESIGN s5 "2-D grids"): bit-for-bit is the right gate.

The single-domain run of every case is pinned by the existing suite, so nothing here is only a self-comparison:
  glm_periodic  tests/test_gpu_xtile.py::test_2d_rows_kernel_strict_bitexact_vs_oracle (mhd_blast_generic, GLM HLLD) and
                ::test_2d_rows_kernel_fast_vs_oracle
  dmr           tests/test_gpu_parity.py::test_dmr_strict (oracle, bit for bit)
  cyl_hd, cyl_glm  tests/test_gpu_xtile.py::test_cyl_rows_kernel_strict_bitexact_vs_oracle (blast_axi2d, hd_roe / glm_hlld_tr)
  wind2d        tests/test_gpu_wind_sources.py::test_run_wind2d_axisymmetric_matches_oracle (wind2d_axi with its source)
"""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NSTEPS = 3


def _case(case, strict):
    """(cfg, P, wind sources)"""
    from pion_amd import abi, problems
    if case == "glm_periodic":
        cfg, P = problems.mhd_blast_generic([70, 48], abi.EQGLM, abi.FLUX_RS_HLLD, strict_fp=strict)
        return cfg, P, []            # (Cartesian: no position enters the solve, dx = 1/70 is as good as a dyadic one)
    if case == "dmr":
        cfg, P = problems.double_mach_reflection(104, strict_fp=strict)     # 104 x 32, dx = 1/32
        return cfg, P, []
    if case == "cyl_hd":
        cfg, P = problems.blast_axi2d(64, abi.EQEUL, abi.FLUX_RSroe, strict_fp=strict)              # 64 x 32, dx = 1/64
        return cfg, P, []
    if case == "cyl_glm":
        cfg, P = problems.blast_axi2d(64, abi.EQGLM, abi.FLUX_RS_HLLD, ntracer=1, strict_fp=strict)
        return cfg, P, []
    if case == "wind2d":
        # 64 x 10, dx = 5e18 / 64 (5e18 = 5^19 2^18: every position (2 j + 1) dx / 2 of the grid is exact); the source
        # region (6 cells) reaches the first on-grid row of rank 1; slabs of 5 rows: an interior of one row
        return problems.wind2d_axi(64, ny=10, strict_fp=strict)
    raise KeyError(case)


def _tables(sim, cfg):
    if cfg.cooling:
        from pion_amd import cooling
        sim.set_cooling_tables(*cooling.build_tables(cfg.min_temp, cfg.max_temp))


def _worker(rank, world, transport, token, case, strict, q):
    try:
        sys.path.insert(0, ROOT)
        sys.path.insert(0, os.path.join(ROOT, "tests"))
        import ctypes as C
        from pion_amd import host_rccl, lib, slab
        cfg_g, P, srcs = _case(case, strict)
        cfg = slab.slab_config(cfg_g, rank, world)
        kw, device = (dict(shm_name=token), 0) if transport == "shm" else (dict(unique_id=token), rank)
        with host_rccl.HostSim(cfg, device, rank=rank, world=world, periodic_z=slab.slab_periodic(cfg_g), **kw) as s:
            g = lib.GpuSim(cfg, device, borrowed_handle=s.gpu_handle())
            _tables(g, cfg)
            keep = []
            for src in srcs:
                st, k = src.to_c()
                keep.append((st, k))
                sid = C.c_int(-1)
                s.lib.pion_host_sim_add_wind_source.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(C.c_int)]
                rc = s.lib.pion_host_sim_add_wind_source(s.s, C.byref(st), C.byref(sid))
                assert rc == 0, "add_wind_source rc=%d: %s" % (rc, s.last_error())
            s.init(slab.slab_slice(P, cfg_g, rank, world))
            n, t, ldt = s.time_int(NSTEPS)
            q.put((rank, t, s.download(0)))
    except Exception as e:   # noqa: BLE001
        q.put((rank, None, repr(e)))


def _run(case, transport, token, strict=1):
    import multiprocessing as mp
    from pion_amd import driver, lib
    cfg, P, srcs = _case(case, strict)
    with lib.GpuSim(cfg, 0) as g:
        _tables(g, cfg)
        sc = driver.SimControl(g, cfg)
        for src in srcs:
            sc.add_wind_source(src)
        sc.init(P)
        sc.time_int(NSTEPS)
        ref, tref = g.download(0), sc.simtime
    assert np.isfinite(ref).all()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_worker, args=(r, 2, transport, token, case, strict, q)) for r in range(2)]
    for p in procs:
        p.start()
    got = {}
    try:
        for _ in range(2):
            r, t, A = q.get(timeout=300)
            assert t is not None, A
            got[r] = (t, A)
    finally:
        for p in procs:
            p.join(timeout=120)
            if p.is_alive():
                p.kill()
    assert all(p.exitcode == 0 for p in procs)
    nb, nyl = cfg.nbc, cfg.ng[1] // 2
    for r in range(2):
        t, A = got[r]
        assert t == tref, (case, r, t, tref)
        want = ref[:, :, nb + r * nyl: nb + (r + 1) * nyl, nb:-nb]
        got_r = A[:, :, nb:nb + nyl, nb:-nb]
        print("%s rank %d: %d of %d on-grid values differ" % (case, r, (got_r != want).sum(), want.size))
        assert np.array_equal(got_r, want), (case, r, (got_r != want).sum())


def _token(case):
    import time
    return "/pion_s2d%d_%d_%s" % (os.getpid(), time.time_ns() % 1000000007, case)


CASES = ["glm_periodic", "dmr", "cyl_hd", "cyl_glm", "wind2d"]


@pytest.mark.parametrize("case", CASES)
def test_cpp_loop_two_ranks_2d_one_gpu_shared_memory_transport(case):
    """glm_periodic: both neighbours of a rank are the other rank; dmr: rank 0 owns the reflecting face and the internal
    DMR2 cells, rank 1 the time-dependent DMACH face; cyl_*: rank 0 owns the axis, rank 1 has BC_SLAB at YN; wind2d:
    cooling and a device-built wind source whose cells lie on both ranks"""
    _run(case, "shm", _token(case))


def test_cpp_loop_two_ranks_2d_fast_build():
    """the fast build is held to the same bits: both sides of a y interface are solved by one copy of the code"""
    _run("cyl_glm", "shm", _token("fast"), strict=0)


def _ngpu():
    try:
        import torch
        return torch.cuda.device_count()
    except Exception:   # noqa: BLE001
        return 0


@pytest.mark.skipif(_ngpu() < 2, reason="needs two GPUs: the RCCL transport between two devices")
@pytest.mark.parametrize("case", CASES)
def test_cpp_loop_two_ranks_2d_two_gpus_rccl(case):
    from pion_amd import host_rccl
    _run(case, "rccl", host_rccl.new_unique_id())
