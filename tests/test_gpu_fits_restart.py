"""Restart from FITS files on the GPU: k_unpack_fits (pion_gpu_unpack_fits) against the numpy restatement of
tests/fits_read_restate.py and the fast build against the strict one, the counter of rejected elements, the streamed
read against the fallback read, restarts across the oracle-bound loop and the device, across two ranks, and on a
handle that runs in plane windows.  Every comparison is == on the 8 bytes.

The kernel test takes the six shapes of tests/test_gpu_fits.py (the smallest at which the mapping can go wrong).  The
handle is bound to two tensors of the test's own, each with guard words before and behind the state and a sentinel of
its own in every cell, so that P and Ph are read back separately and every cell the kernel must not write -- ghost
cells, other planes, the guards -- is seen to keep its bits."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

import fits_read_restate as rr
import fits_restate as fr
from pion_amd import abi, host_rccl, lib, problems, slab
from test_gpu_fits import SHAPES, kernel_case
from test_host_snapshot import assemble, case, ongrid, orc_loop, run_steps

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
nosetup = lambda sim, c: None
GUARD = 64


def same(a, b):
    return fr.same_bits(a, b)


def _on_device(a):
    """the bytes of a numpy array as a device tensor of doubles (bit patterns kept)"""
    import torch
    return torch.from_numpy(np.frombuffer(np.ascontiguousarray(a).tobytes(), dtype="=f8").copy()).to("cuda:0")


def _file_elements(cfg, rng, lo, hi):
    """file elements of planes [lo, hi) as '>f8' [nvar][planes][rows][nx], values of both signs"""
    rows = cfg.ng[1] if cfg.ndim == 3 else 1
    return (rng.uniform(0.5, 1.5, size=(cfg.nvar, hi - lo, rows, cfg.ng[0])) - 1.0).astype(">f8")


def _put(A, cfg, lo, hi, vals):
    """vals [nvar][planes][rows][nx] into the on-grid cells of planes [lo, hi) of the all-cell array A"""
    nb = cfg.nbc
    if cfg.ndim == 3:
        A[:, nb + lo:nb + hi, nb:-nb, nb:-nb] = vals
    elif cfg.ndim == 2:
        A[:, 0, nb + lo:nb + hi, nb:-nb] = vals[:, :, 0, :]
    else:
        A[:, 0, 0, nb:-nb] = vals[:, 0, 0, :]


@pytest.mark.parametrize("name", SHAPES)
def test_unpack_fits_equals_the_restatement_in_both_builds(name):
    import torch
    cfg0 = kernel_case(name, 1)
    shape = problems.alloc(cfg0).shape
    n = int(np.prod(shape))
    nplanes = 1 if cfg0.ndim == 1 else cfg0.ng[cfg0.ndim - 1]
    ranges = [(0, nplanes)] + ([(1, 2)] if nplanes > 1 else [])
    rng = np.random.default_rng(17)
    sentinel = [rng.uniform(-9.0, -8.0, size=n + 2 * GUARD) for _ in range(2)]   # P and Ph: different in every cell
    got = {}
    for strict in (1, 0):
        cfg = kernel_case(name, strict)
        with lib.GpuSim(cfg, 0) as g:
            for lo, hi in ranges:
                t = [torch.from_numpy(s).to("cuda:0") for s in sentinel]
                g.bind_device_state(t[0].data_ptr() + 8 * GUARD, t[1].data_ptr() + 8 * GUARD)
                F = _file_elements(cfg, np.random.default_rng(23), lo, hi)
                rows = cfg.ng[1] if cfg.ndim == 3 else 1
                assert g.fits_prim_count(hi - lo) == F.size == cfg.nvar * (hi - lo) * rows * cfg.ng[0]
                buf = _on_device(F)
                torch.cuda.synchronize()
                g.unpack_fits(lo, hi, buf.data_ptr())
                assert g.unpack_fits_status() == 0
                vals, nbad = rr.from_big_endian(cfg, F)
                assert nbad == 0
                for which in (0, 1):
                    want = sentinel[which].copy()
                    _put(want[GUARD:-GUARD].reshape(shape), cfg, lo, hi, vals)
                    assert same(t[which].cpu().numpy(), want), (name, strict, lo, hi, which)
                got[(strict, lo, hi)] = t[0].cpu().numpy()
                mhd = cfg.eqntype in (abi.EQMHD, abi.EQGLM)
                assert mhd == (not same(vals, F.astype("=f8")))   # B, and only B, is rescaled
            for bad in ((-1, 1), (0, nplanes + 1), (1, 1)):
                with pytest.raises(lib.PionGpuError):
                    g.unpack_fits(bad[0], bad[1], 8)
            with pytest.raises(lib.PionGpuError):
                g.unpack_fits(0, 1, 0)
    for lo, hi in ranges:   # fast against strict
        assert same(got[(0, lo, hi)], got[(1, lo, hi)]), (lo, hi)


def test_rejected_elements_are_counted_and_the_count_is_cleared():
    """a NaN in the first element and -1e99 in the last one of a 70 x 3 x 2 buffer: values in a buffer the kernel
    reads, stored like any other"""
    import torch
    cfg = kernel_case("euler_tr_cool_70x3x2", 0)
    with lib.GpuSim(cfg, 0) as g:
        assert g.unpack_fits_status() == 0   # nothing unpacked yet
        F = _file_elements(cfg, np.random.default_rng(29), 0, 2)
        clean = _on_device(F)
        F.reshape(-1)[0] = np.nan
        F.reshape(-1)[-1] = -1.0e99
        assert rr.from_big_endian(cfg, F)[1] == 2
        planted = _on_device(F)
        torch.cuda.synchronize()
        g.unpack_fits(0, 2, planted.data_ptr())
        assert g.unpack_fits_status() == 2
        assert g.unpack_fits_status() == 0
        A = g.download(0)
        nb = cfg.nbc
        assert np.isnan(A[0, nb, nb, nb]) and A[-1, -nb - 1, -nb - 1, -nb - 1] == -1.0e99
        g.unpack_fits(0, 2, clean.data_ptr())
        assert g.unpack_fits_status() == 0
        # close to the null value counts (equalD), far from it does not
        F = _file_elements(cfg, np.random.default_rng(31), 0, 2)
        F.reshape(-1)[5] = -1.0e99 * (1.0 + 1.0e-13)
        F.reshape(-1)[6] = -1.0e99 * (1.0 + 1.0e-11)
        F.reshape(-1)[7] = np.inf
        assert rr.from_big_endian(cfg, F)[1] == 2
        near = _on_device(F)
        torch.cuda.synchronize()
        g.unpack_fits(0, 2, near.data_ptr())
        assert g.unpack_fits_status() == 2


class _Table(C.Structure):
    """pion_backend (pion_amd/host/pion_backend.h): the name and 24 function pointers"""
    _fields_ = [("f%d" % i, C.c_void_p) for i in range(25)]


def _table_without_fits_read_entries():
    """the product's backend table with fits_from_host and fits_read_status cleared"""
    h = host_rccl.load_host_library()
    h.pion_backend_gpu.restype = C.c_void_p
    t = _Table.from_buffer_copy(C.string_at(h.pion_backend_gpu(), C.sizeof(_Table)))
    assert t.f22 and t.f23 and t.f24
    t.f23 = t.f24 = None
    return t


def test_streamed_read_equals_the_fallback_read(tmp_path, monkeypatch):
    """chunks of 1 and 4 planes (6 planes: an uneven last chunk) and the default, fast build, two steps in"""
    cfg, P = problems.mhd_blast_generic([13, 7, 6], strict_fp=0)
    path = str(tmp_path / "two_steps.fits")
    with host_rccl.HostSim(cfg, 0) as s:
        s.init(P)
        run_steps(s, 2)
        s.write_fits(path)
    table = _table_without_fits_read_entries()
    with host_rccl.HostSim(cfg, 0, backend=C.addressof(table)) as s:
        assert s.restart(path) == ""
        want = (ongrid(s.download(0), cfg), ongrid(s.download(1), cfg), s.get_time(), run_steps(s, 1))
    og, nbad, missing, _ = rr.restate_files(cfg, [path])
    assert nbad == 0 and not missing and same(want[0], og) and same(want[1], og)
    with host_rccl.HostSim(cfg, 0) as s:
        for chunk in ("1", "4", None):
            if chunk is None:
                monkeypatch.delenv("PION_SNAPSHOT_CHUNK_PLANES", raising=False)
            else:
                monkeypatch.setenv("PION_SNAPSHOT_CHUNK_PLANES", chunk)
            s.init(P)   # another state, so that every chunk has something to change
            assert s.restart(path) == ""
            assert same(ongrid(s.download(0), cfg), want[0]) and same(ongrid(s.download(1), cfg), want[1]), chunk
            assert s.get_time() == want[2]
            assert run_steps(s, 1) == want[3]
        # the writers share the slots: files written after a streamed read are the files written before it
        s.restart(path)
        s.write_fits(str(tmp_path / "again.fits"))
    with host_rccl.HostSim(cfg, 0, backend=C.addressof(table)) as s:
        s.restart(path)
        s.write_fits(str(tmp_path / "fallback_again.fits"))
    assert open(str(tmp_path / "again.fits"), "rb").read() == open(str(tmp_path / "fallback_again.fits"), "rb").read()


def test_streamed_read_reports_rejected_elements_and_recovers(tmp_path):
    cfg, P = problems.mhd_blast_generic([13, 7, 6], strict_fp=0)
    path, bad = str(tmp_path / "good.fits"), str(tmp_path / "bad.fits")
    with host_rccl.HostSim(cfg, 0) as s:
        s.init(P)
        s.write_fits(path)
        hdus = rr.split_hdus(open(path, "rb").read())
        i = [rr.extname(h) for h, _ in hdus].index("psi")
        hdus[i] = (hdus[i][0], rr.plant(rr.plant(hdus[i][1], 3, float("nan")), 13 * 7 * 6 - 1, -1.0e99))
        open(bad, "wb").write(rr.join_hdus(hdus))
        with pytest.raises(RuntimeError, match="2 element"):
            s.restart(bad)
        assert s.restart(path) == ""
        assert same(ongrid(s.download(0), cfg), rr.restate_files(cfg, [path])[0])


def test_cross_restart_between_the_oracle_loop_and_the_device(tmp_path):
    """the oracle-bound loop writes after 2 steps, the strict device build reads and continues 3 steps, and the other
    way round: the state and every dt are those of the oracle-bound loop restarted from the same file"""
    cfg, P, setup = case("glm3d")
    by_orc, by_gpu = str(tmp_path / "from_orc.fits"), str(tmp_path / "from_gpu.fits")
    with orc_loop(cfg, setup) as s:
        s.init(P)
        first = run_steps(s, 2)
        s.write_fits(by_orc)
    with host_rccl.HostSim(cfg, 0) as s:
        s.init(P)
        assert run_steps(s, 2) == first
        s.write_fits(by_gpu)
    a, b = fr.images_of(by_orc), fr.images_of(by_gpu)
    assert list(a) == list(b) and all(same(a[n], b[n]) for n in a)
    with orc_loop(cfg, setup) as s:
        s.restart(by_orc)
        want = (run_steps(s, 3), s.download(0), s.download(1))
    for f in (by_orc, by_gpu):
        with host_rccl.HostSim(cfg, 0) as s:
            s.restart(f)
            assert s.get_time()["timestep"] == 2 and s.get_time()["simtime"] == first[-1][1]
            assert run_steps(s, 3) == want[0]
            assert same(ongrid(s.download(0), cfg), ongrid(want[1], cfg))
            assert same(ongrid(s.download(1), cfg), ongrid(want[2], cfg))
    with orc_loop(cfg, setup) as s:
        s.restart(by_gpu)
        assert run_steps(s, 3) == want[0] and same(ongrid(s.download(0), cfg), ongrid(want[1], cfg))


def _restart_rank(rank, world, shm, case_name, paths, nsteps, q):
    """a rank of a slab run on device 0 that restarts from FITS files and steps"""
    try:
        for p in (ROOT, os.path.join(ROOT, "tests")):
            if p not in sys.path:
                sys.path.insert(0, p)
        cfg_g, _ = fr.two_rank_case(case_name)
        cfg = slab.slab_config(cfg_g, rank, world)
        ax = slab.slab_axis(cfg_g)
        with host_rccl.HostSim(cfg, 0, rank=rank, world=world, periodic_z=slab.slab_periodic(cfg_g), shm_name=shm) as s:
            s.set_slab_extent(cfg_g.ng[ax], rank * cfg.ng[ax], cfg_g.bc_type[2 * ax], cfg_g.bc_type[2 * ax + 1])
            s.restart(paths)
            s.time_int(nsteps)
            q.put((rank, s.get_time(), s.download(0)))
    except Exception as e:   # noqa: BLE001
        q.put((rank, None, repr(e)))


@pytest.mark.parametrize("name", ["glm3d_z12", "glm2d_y12"])
def test_two_ranks_on_one_gpu_write_two_ranks_and_one_restart(name, tmp_path):
    """3-D cut along z, 2-D cut along y: two processes on device 0 write after two steps; one domain and two ranks
    restart from the two files and take two more steps"""
    import multiprocessing as mp
    import time
    cfg, P = fr.two_rank_case(name)
    paths = [str(tmp_path / ("r%d.fits" % r)) for r in range(2)]
    times = fr.run_two_ranks(name, "gpu", 2, paths)
    og, nbad, missing, par = rr.restate_files(cfg, paths)
    assert nbad == 0 and not missing and par["t_sim"] == times[0]["simtime"]
    with host_rccl.HostSim(cfg, 0) as s:
        s.init(rr.embed(cfg, og), simtime=par["t_sim"], timestep=par["t_step"], last_dt=par["last_dt"])
        want = (run_steps(s, 2), ongrid(s.download(0), cfg))
    with host_rccl.HostSim(cfg, 0) as s:
        s.restart(paths[::-1])
        assert same(ongrid(s.download(0), cfg), og)
        assert run_steps(s, 2) == want[0] and same(ongrid(s.download(0), cfg), want[1])
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    shm = "/pion_fr%d_%d" % (os.getpid(), time.time_ns() % 1000000007)
    procs = [ctx.Process(target=_restart_rank, args=(r, 2, shm, name, paths, 2, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = {}
    try:
        for _ in range(2):
            r, t, A = q.get(timeout=300)
            assert t is not None, A
            res[r] = (t, A)
    finally:
        for p in procs:
            p.join(timeout=120)
            if p.is_alive():
                p.kill()
    assert all(p.exitcode == 0 for p in procs)
    for r in range(2):
        assert res[r][0]["simtime"] == want[0][-1][1] and res[r][0]["timestep"] == 4
    assert same(assemble(res, cfg, 2), want[1])


def test_windowed_handle_restarts_from_fits(tmp_path, monkeypatch):
    """a handle whose stages run in plane windows of <= 3 planes (tests/test_gpu_rows_windows.py's knob)"""
    cfg, P, setup = case("glm3d")
    path = str(tmp_path / "w.fits")
    with host_rccl.HostSim(cfg, 0) as s:
        s.init(P)
        run_steps(s, 2)
        s.write_fits(path)
    og, _, _, par = rr.restate_files(cfg, [path])
    stride = (cfg.ng[0] + 2 * cfg.nbc) * (cfg.ng[1] + 2 * cfg.nbc)
    monkeypatch.setenv("PION_ROWS_WINDOW_CELLS", str((3 + 2 * cfg.nbc) * stride + 1))
    with host_rccl.HostSim(cfg, 0) as s:
        assert lib.GpuSim(cfg, 0, borrowed_handle=s.gpu_handle()).rows_windows()["windows_whole_stage"] == 3
        s.init(rr.embed(cfg, og), simtime=par["t_sim"], timestep=par["t_step"], last_dt=par["last_dt"])
        want = (run_steps(s, 3), ongrid(s.download(0), cfg), ongrid(s.download(1), cfg))
    with host_rccl.HostSim(cfg, 0) as s:
        s.restart(path)
        assert same(ongrid(s.download(0), cfg), og)
        assert run_steps(s, 3) == want[0]
        assert same(ongrid(s.download(0), cfg), want[1]) and same(ongrid(s.download(1), cfg), want[2])
