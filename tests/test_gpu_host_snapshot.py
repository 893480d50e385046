"""Snapshot / restart of the C++ host loop on the GPU: k_pack_ongrid (pion_gpu_pack_ongrid / _unpack_ongrid), the
chunked streaming of pion_backend_gpu.cpp, and restarts across the oracle-bound loop and the device
(tests/test_host_snapshot.py holds the cases, the CPU loop and the helpers).  Everything is compared with ==.

Shapes: 13 x 7 x 6 (x below one wavefront and odd), 70 x 5 x 5 (x over one wavefront), 2-D 37 x 5 and 1-D 128 (the
three shapes of a "plane"); 1100 x 4 x 4 (x over one 1024-cell stretch of a wavefront); no case above 40 x 24 x 20."""
import os
import sys

import numpy as np
import pytest

from pion_amd import abi, cooling, driver, host_rccl, lib, problems, slab
from test_host_snapshot import (case, orc_loop, ongrid, restart_roundtrip, run_steps, run_ranks)  # noqa: F401

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class _GpuFactory:
    """make_loop for restart_roundtrip: the product's loop on device 0"""

    def __init__(self):
        self._lim = None

    def __call__(self, cfg, setup, sources=(), **kw):
        s = host_rccl.HostSim(cfg, 0, **kw)
        self._lim = setup(lib.GpuSim(cfg, 0, borrowed_handle=s.gpu_handle()), cfg)
        for src in sources:
            s.add_wind_source(src)
        return s

    def last_dt_limit(self):
        return self._lim


gpu_loop = _GpuFactory()


def _dev_buffer(n):
    import torch
    return torch.zeros(int(n), dtype=torch.float64, device="cuda:0")


def _grid(shape, eq=abi.EQGLM):
    shape = list(shape)
    if eq == abi.EQGLM and len(shape) > 1:
        return problems.mhd_blast_generic(shape, strict_fp=1)
    if len(shape) == 1:
        return problems.blast_sph1d(shape[0], strict_fp=1)
    return problems.hd_blast_box(shape, strict_fp=1)


def _slice(A, cfg, lo, hi):
    """numpy's view of pack_ongrid: on-grid cells of planes [lo, hi) of a downloaded array, [nvar][planes][ny][nx]"""
    nb = cfg.nbc
    if cfg.ndim == 3:
        return A[:, nb + lo:nb + hi, nb:-nb, nb:-nb]
    if cfg.ndim == 2:
        return A[:, 0, nb + lo:nb + hi, nb:-nb][:, :, None, :]
    return A[:, 0, 0, nb:-nb][:, None, None, :]


def _ranges(n, every):
    if every:
        return [(a, b) for a in range(n) for b in range(a + 1, n + 1)]
    return [(0, 1), (n - 1, n), (0, n)] + ([(1, n - 1)] if n > 2 else [])


@pytest.fixture(scope="module")
def stepped():
    """per shape: a handle half a step into a run (Ph differs from P), its two downloads"""
    made = {}

    def get(shape):
        if shape not in made:
            cfg, P = _grid(shape)
            g = lib.GpuSim(cfg, 0)
            sc = driver.SimControl(g, cfg)
            sc.init(P)
            dt = sc.calculate_timestep()
            g.stage(0.5 * dt, 1, 0)
            g.update_bcs(0.0, 1, 2)
            made[shape] = (cfg, g, g.download(0), g.download(1))
            assert not np.array_equal(made[shape][2], made[shape][3])
        return made[shape]
    yield get
    for _, g, _, _ in made.values():
        g.close()


@pytest.mark.parametrize("shape,every", [((13, 7, 6), True), ((70, 5, 5), False), ((1100, 4, 4), False),
                                         ((37, 5), True), ((128,), False)])
def test_pack_ongrid_equals_the_slice_of_download(stepped, shape, every):
    cfg, g, A0, A1 = stepped(shape)
    nplanes = 1 if cfg.ndim == 1 else cfg.ng[cfg.ndim - 1]
    for which, A in ((0, A0), (1, A1)):
        for lo, hi in _ranges(nplanes, every):
            n = g.ongrid_count(hi - lo)
            want = _slice(A, cfg, lo, hi)
            assert n == want.size
            buf = _dev_buffer(n + 8)
            buf[:] = -7.0
            g.pack_ongrid(which, lo, hi, buf.data_ptr())
            g.synchronize()
            got = buf.cpu().numpy()
            assert np.array_equal(got[:n].reshape(want.shape), want), (which, lo, hi)
            assert (got[n:] == -7.0).all(), "wrote past the buffer"


@pytest.mark.parametrize("shape", [(13, 7, 6), (70, 5, 5), (37, 5), (128,)])
def test_unpack_ongrid_changes_exactly_those_cells(shape):
    import torch
    cfg, P = _grid(shape)
    nplanes = 1 if cfg.ndim == 1 else cfg.ng[cfg.ndim - 1]
    rng = np.random.default_rng(5)
    with lib.GpuSim(cfg, 0) as g:
        sc = driver.SimControl(g, cfg)
        sc.init(P)
        before = g.download(0)
        for lo, hi in _ranges(nplanes, False):
            want = before.copy()
            new = rng.uniform(0.5, 1.5, size=_slice(want, cfg, lo, hi).shape)
            _slice(want, cfg, lo, hi)[...] = new
            buf = torch.from_numpy(new.reshape(-1)).to("cuda:0")
            g.unpack_ongrid(lo, hi, buf.data_ptr())
            assert np.array_equal(g.download(0), want) and np.array_equal(g.download(1), want), (lo, hi)
            before = want
    for bad in ((-1, 1), (0, nplanes + 1), (1, 1)):
        with lib.GpuSim(cfg, 0) as g:
            with pytest.raises(lib.PionGpuError):
                g.unpack_ongrid(bad[0], bad[1], _dev_buffer(16).data_ptr())


def test_step_after_unpack_equals_step_after_upload():
    """unpack writes P and Ph and drops the cached time step: the next dt and the next step are upload's"""
    import torch
    cfg, P = _grid((13, 7, 6))
    with lib.GpuSim(cfg, 0) as g:
        sc = driver.SimControl(g, cfg)
        sc.init(P)
        sc.time_int(2)
        state = g.download(0)
        sc.time_int(1)          # the handle now holds another state, its minima cached by the last stage
        data = np.ascontiguousarray(_slice(state, cfg, 0, cfg.ng[2])).reshape(-1)
        g.unpack_ongrid(0, cfg.ng[2], torch.from_numpy(data).to("cuda:0").data_ptr())
        g.update_bcs(0.0, 2, 2, assign=1)
        dt_unpack = g.calc_dt()
        g.set_glm_speeds(dt_unpack[0], cfg.dx, 0.25 / cfg.dx)
        g.advance_time(min(dt_unpack), 0.0)
        after_unpack = (g.download(0), g.download(1))
        g.upload(state)
        g.update_bcs(0.0, 2, 2, assign=1)
        dt_upload = g.calc_dt()
        g.set_glm_speeds(dt_upload[0], cfg.dx, 0.25 / cfg.dx)
        g.advance_time(min(dt_upload), 0.0)
        assert dt_unpack == dt_upload
        assert np.array_equal(g.download(0), after_unpack[0]) and np.array_equal(g.download(1), after_unpack[1])


def _data_region(path):
    _, info = host_rccl.read_snapshot_header(path)
    return open(path, "rb").read()[info["data_offset"]:]


def test_streamed_file_equals_the_whole_array_file(tmp_path, monkeypatch):
    """chunks of 1 and 4 planes (6 planes: an uneven last chunk) and the default against the oracle-bound loop's
    file of the same state (strict build, two steps in); read back in chunks it gives the same device state"""
    cfg, P = _grid((13, 7, 6))
    nosetup = lambda sim, c: None
    with orc_loop(cfg, nosetup) as s:
        s.init(P)
        run_steps(s, 2)
        s.write_snapshot(str(tmp_path / "orc.pionraw"))
        want = s.download(0)
    whole = _data_region(str(tmp_path / "orc.pionraw"))
    assert len(whole) == 8 * cfg.nvar * 13 * 7 * 6
    with gpu_loop(cfg, nosetup) as s:
        s.init(P)
        run_steps(s, 2)
        for chunk in ("1", "4", None):
            if chunk is None:
                monkeypatch.delenv("PION_SNAPSHOT_CHUNK_PLANES", raising=False)
            else:
                monkeypatch.setenv("PION_SNAPSHOT_CHUNK_PLANES", chunk)
            f = str(tmp_path / ("gpu_%s.pionraw" % chunk))
            s.write_snapshot(f)
            assert _data_region(f) == whole, chunk
    for chunk in ("1", "4"):
        monkeypatch.setenv("PION_SNAPSHOT_CHUNK_PLANES", chunk)
        with gpu_loop(cfg, nosetup) as s:
            s.restart(str(tmp_path / "gpu_4.pionraw"))
            assert np.array_equal(ongrid(s.download(0), cfg), ongrid(want, cfg)), chunk
            assert np.array_equal(ongrid(s.download(1), cfg), ongrid(want, cfg)), chunk


@pytest.mark.parametrize("name", ["glm3d", "euler_axi2d", "wind3d"])
def test_cross_restart_between_the_oracle_loop_and_the_device(name, tmp_path):
    """the oracle-bound loop writes at step 2, the strict device build reads and runs 3 steps (and the other way
    round): P and every dt are the oracle's uninterrupted 5 steps"""
    cfg, P, setup = case(name)
    with orc_loop(cfg, setup) as s:
        s.init(P, first_step_dt_limit=orc_loop.last_dt_limit())
        first = run_steps(s, 2)
        s.write_snapshot(str(tmp_path / "from_orc.pionraw"))
        steps = first + run_steps(s, 3)
        ref = ongrid(s.download(0), cfg)
    cut = lambda A: ongrid(A, cfg)
    with gpu_loop(cfg, setup) as s:
        s.restart(str(tmp_path / "from_orc.pionraw"))
        assert first + run_steps(s, 3) == steps
        assert np.array_equal(cut(s.download(0)), ref)
    with gpu_loop(cfg, setup) as s:
        s.init(P, first_step_dt_limit=gpu_loop.last_dt_limit())
        assert run_steps(s, 2) == first
        s.write_snapshot(str(tmp_path / "from_gpu.pionraw"))
    with orc_loop(cfg, setup) as s:
        s.restart(str(tmp_path / "from_gpu.pionraw"))
        assert first + run_steps(s, 3) == steps
        assert np.array_equal(cut(s.download(0)), ref)


@pytest.mark.parametrize("name", ["glm3d", "dmr2d"])
def test_fast_build_restart_equals_its_own_run(name, tmp_path):
    ref, got = restart_roundtrip(gpu_loop, name, tmp_path, strict_fp=0)
    assert got[2] == ref[2]
    assert np.array_equal(got[0], ref[0]) and np.array_equal(got[1], ref[1])


def test_device_built_wind_source_is_added_again_before_the_restart(tmp_path):
    """problems.wind2d_axi 32 x 16 with its constant source added again before the restart.

    The XP face of this problem is an inflow face, and its captured state is not in the file: a restart captures it
    again from the on-grid neighbour, as the reference's restart does.  The ghost cells keep the uncooled initial
    pressure while the gas next to them cools, so that neighbour leaves its initial state during the first step
    (measured at step 2: density 7.000000000014044e-24 against 7e-24 captured at the start; 156 ghost values differ at
    the restart, no on-grid cell; three steps later 244 on-grid values next to the face differ in the last digits).
    The only snapshot of this problem whose inflow face still borders initial-state cells is therefore the one at
    step 0: that restart must continue bit for bit -- with the first-step limit of the source, which only a source
    added through the loop brings back.  At step 2 the test pins what was just described: the restart reproduces
    every on-grid cell and every ghost cell except the inflow face's, and those hold the state of the on-grid cell the
    face captures from."""
    cfg, P, srcs = problems.wind2d_axi(32, ny=16, strict_fp=1)
    nb = cfg.nbc

    def setup(sim, c):
        sim.set_cooling_tables(*cooling.build_tables(c.min_temp, c.max_temp))
    p0, p2 = str(tmp_path / "wind0.pionraw"), str(tmp_path / "wind2.pionraw")
    with gpu_loop(cfg, setup, sources=srcs) as s:
        s.init(P)
        s.write_snapshot(p0)
        steps = run_steps(s, 2)
        s.write_snapshot(p2)
        mid = s.download(0)
        steps += run_steps(s, 3)
        ref = (s.download(0), s.download(1))
    from pion_amd import snapshot
    assert snapshot.read(p2)[2]["WIND_Nsources"] == "1" and host_rccl.read_snapshot_header(p2)[1]["t_step"] == 2
    with gpu_loop(cfg, setup, sources=srcs) as s:
        s.restart(p0)
        assert run_steps(s, 5) == steps
        assert np.array_equal(s.download(0), ref[0]) and np.array_equal(s.download(1), ref[1])
    with gpu_loop(cfg, setup, sources=srcs) as s:
        s.restart(p2)
        got = s.download(0)
        assert np.array_equal(got[..., :-nb], mid[..., :-nb])
        inflow = got[:, :, nb:-nb, -nb:]
        # (inflow_boundaries.cpp: one state, the on-grid neighbour of the last cell of the face's list)
        assert np.array_equal(inflow, np.broadcast_to(got[:, :, -nb - 1:-nb, -nb - 1:-nb], inflow.shape))
        assert s.get_time()["simtime"] == steps[1][1]


def test_windowed_handle_writes_and_restarts(tmp_path, monkeypatch):
    """a handle whose stages run in plane windows of <= 3 planes (tests/test_gpu_rows_windows.py's knob)"""
    cfg, P, setup = case("glm3d")
    stride = (cfg.ng[0] + 2 * cfg.nbc) * (cfg.ng[1] + 2 * cfg.nbc)
    monkeypatch.setenv("PION_ROWS_WINDOW_CELLS", str((3 + 2 * cfg.nbc) * stride + 1))
    with gpu_loop(cfg, setup) as s:
        assert lib.GpuSim(cfg, 0, borrowed_handle=s.gpu_handle()).rows_windows()["windows_whole_stage"] == 3
    ref, got = restart_roundtrip(gpu_loop, "glm3d", tmp_path)
    assert got[2] == ref[2]
    assert np.array_equal(got[0], ref[0]) and np.array_equal(got[1], ref[1])


def _gpu_rank(rank, world, name, paths, nsteps, q):
    try:
        for p in (ROOT, os.path.join(ROOT, "tests")):
            if p not in sys.path:
                sys.path.insert(0, p)
        cfg_g, P, setup = case("glm3d_z12")
        cfg = slab.slab_config(cfg_g, rank, world)
        with host_rccl.HostSim(cfg, 0, rank=rank, world=world, periodic_z=True, shm_name=name) as s:
            s.set_slab_extent(cfg_g.ng[2], rank * cfg.ng[2], cfg_g.bc_type[4], cfg_g.bc_type[5])
            s.init(slab.slab_slice(P, cfg_g, rank, world))
            s.time_int(nsteps)
            s.write_snapshot(paths[rank])
            q.put((rank, s.get_time(), None))
    except Exception as e:   # noqa: BLE001
        q.put((rank, None, repr(e)))


def test_two_ranks_on_one_gpu_write_one_rank_restarts(tmp_path):
    import multiprocessing as mp
    import time
    cfg, P, setup = case("glm3d_z12")
    with gpu_loop(cfg, setup) as s:
        s.init(P)
        steps = run_steps(s, 5)
        ref = ongrid(s.download(0), cfg)
    paths = [str(tmp_path / ("r%d.pionraw" % r)) for r in range(2)]
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    name = "/pion_gs%d_%d" % (os.getpid(), time.time_ns() % 1000000007)
    procs = [ctx.Process(target=_gpu_rank, args=(r, 2, name, paths, 2, q)) for r in range(2)]
    for p in procs:
        p.start()
    try:
        for _ in range(2):
            r, t, msg = q.get(timeout=300)
            assert t is not None, msg
            assert t["simtime"] == steps[1][1]
    finally:
        for p in procs:
            p.join(timeout=120)
            if p.is_alive():
                p.kill()
    assert all(p.exitcode == 0 for p in procs)
    with gpu_loop(cfg, setup) as s:
        s.restart(paths)
        assert run_steps(s, 3) == steps[2:]
        assert np.array_equal(ongrid(s.download(0), cfg), ref)
