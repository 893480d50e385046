"""Projected images of a slab-decomposed run on the device: pion_gpu_project_part, the part instances of the kernels of
pion_amd/csrc/pion_project.hip, and the collective pion_host_sim_write_projection above them.  Every comparison is ==
on the 8 bytes or byte for byte on the file: the chain of parts and the single grid take the same additions in the
same order (pion_amd/csrc/dev_project.h, "parts").

The single-grid side -- pion_gpu_project on one handle of the whole domain -- is pinned to the numpy restatement by
tests/test_gpu_projection.py (and tests/test_host_projection.py on the host route); it is not checked again here.

Inputs as in tests/test_host_projection_ranks.py (tests/projection_parts_restate.py): rough states, NaN in every ghost
cell the rule may not read, the neighbour's first row in the one ghost row the Abel slope reads, images finite, and
per case the numpy proof that adding per-rank partial sums would NOT give the single sum's bits.

1. one process, one handle per slab on device 0, the test relays the device buffer: the narrowest test of the entry
   point.  Both builds.
2. one process per rank on device 0 over slab_comm_shm through HostSim.write_projection, device route and host route.
3. the same over slab_comm_rccl with a rank per device: skipped where the box has fewer than two GPUs."""
import ctypes as C
import multiprocessing as mp
import os
import sys
import time

import numpy as np
import pytest

import fits_restate as fr
import projection_parts_restate as pp
import projection_restate as pr
from pion_amd import abi, cooling, lib

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TESTS = os.path.join(ROOT, "tests")
SEED = 5
WORLD = {"euler_tr_70x9x10": 2, "glm_tr_66x5x15": 3, "cyl_70x10": 2, "cyl_70x40": 2, "cyl_70x40_off_axis": 2,
         "cyl_cool_70x40": 2}
CASES = [("euler_tr_70x9x10", 0), ("euler_tr_70x9x10", 1), ("euler_tr_70x9x10", 2),
         ("glm_tr_66x5x15", 0), ("glm_tr_66x5x15", 1), ("glm_tr_66x5x15", 2),
         ("cyl_70x10", None), ("cyl_70x40", None), ("cyl_70x40_off_axis", None), ("cyl_cool_70x40", None)]


def _tables(g, cfg):
    if cfg.cooling:
        g.set_cooling_tables(*cooling.build_tables(cfg.min_temp, cfg.max_temp))


def _whole(cfg_g, P, axis, fields):
    with lib.GpuSim(cfg_g, 0) as g:
        _tables(g, cfg_g)
        g.upload(pp.nan_ghosts(cfg_g, P))
        return g.project(axis, fields)


def _chain(name, strict, P, axis, fields, world):
    """the image after the parts of `world` handles, relayed in one device buffer with guard words behind it"""
    import torch
    cfg_g = pp.case(name, strict)
    buf = None
    for rank in range(world):
        cfg, A = pp.slab_state(P, cfg_g, rank, world)
        part = pp.part_of(cfg_g, rank, world)
        with lib.GpuSim(cfg, 0) as g:
            _tables(g, cfg)
            g.upload(A)   # no boundary update: the ghosts stay as the test made them
            n = g.project_part_count(axis, len(fields), part)
            if buf is None:
                buf = torch.zeros((n + 8,), dtype=torch.float64, device="cuda:0")
                buf[n:] = -7.0
            assert buf.numel() == n + 8                      # every rank: the image of the whole domain
            g.project_part(axis, fields, part, dimg_ptr=buf.data_ptr())
            g.synchronize()
    raw = buf.cpu().numpy()
    assert (raw[n:] == -7.0).all(), "wrote past the buffer"
    return raw[:n]


@pytest.mark.parametrize("name,axis", CASES)
def test_the_chain_of_parts_equals_the_whole_grid_in_both_builds(name, axis):
    world = WORLD[name]
    cfg_g = pp.case(name)
    axis = pp.axis_of(cfg_g, axis)
    P, fields = pr.rough_state(cfg_g, SEED), pp.fields_of(name, cfg_g)
    if axis in (2, abi.PROJ_AXIS_PERP):
        assert pp.naive_differs(cfg_g, P, fields, axis, world), "the state is too tame: another seed"
    for strict in (1, 0):
        whole = _whole(pp.case(name, strict), P, axis, fields)
        assert np.isfinite(whole).all() and np.abs(whole).max() > 0.0
        got = _chain(name, strict, P, axis, fields, world).reshape(whole.shape)
        assert fr.same_bits(got, whole), (name, axis, "strict" if strict else "fast")


@pytest.mark.parametrize("name,axis", [("euler_tr_70x9x10", 0), ("euler_tr_70x9x10", 2), ("cyl_70x40_off_axis", None)])
def test_one_part_that_is_the_whole_grid_equals_project(name, axis, monkeypatch):
    """plane_lo = 0, global_planes = the handle's own planes, last = 1, on +0.0; also on a handle whose stages run in
    plane windows (tests/test_gpu_rows_windows.py's knob): the image reads the state array itself"""
    cfg = pp.case(name)
    axis = pp.axis_of(cfg, axis)
    P, fields = pp.nan_ghosts(cfg, pr.rough_state(cfg, SEED)), pp.fields_of(name, cfg)
    part = pp.part_of(cfg, 0, 1)
    monkeypatch.delenv("PION_ROWS_WINDOW_CELLS", raising=False)
    with lib.GpuSim(cfg, 0) as g:
        g.upload(P)
        whole = g.project(axis, fields)
        assert fr.same_bits(g.project_part(axis, fields, part), whole)
    if cfg.ndim == 3:
        stride = (cfg.ng[0] + 2 * cfg.nbc) * (cfg.ng[1] + 2 * cfg.nbc)
        monkeypatch.setenv("PION_ROWS_WINDOW_CELLS", str((2 + 2 * cfg.nbc) * stride + 1))
        with lib.GpuSim(cfg, 0) as g:
            g.upload(P)
            assert g.rows_windows()["windows_whole_stage"] > 1
            assert fr.same_bits(g.project_part(axis, fields, part), whole)


def test_refusals_of_the_part_entry_points():
    import torch
    cfg = pp.case("cyl_70x10")
    fields = pr.fields_of(cfg)[:1]
    arr = abi.proj_fields(fields)
    buf = torch.zeros((70 * 40,), dtype=torch.float64, device="cuda:0")
    ptr = C.c_void_p(buf.data_ptr())
    bad = [((-1, 20, 0, 0.0), "plane_lo is not negative"), ((11, 20, 1, 0.0), "end above global_planes"),
           ((0, 9, 1, 0.0), "end above global_planes"), ((0, 20, 0, float("nan")), "global_xmin is finite"),
           ((0, 20, 0, float("inf")), "global_xmin is finite")]
    with lib.GpuSim(cfg, 0) as g:
        g.upload(pr.rough_state(cfg, SEED))
        for part, text in bad:
            p = abi.proj_part(part)
            assert g.lib.pion_gpu_project_part_count(g.h, abi.PROJ_AXIS_PERP, 1, C.byref(p)) == abi.E_INVAL
            assert text in g._err()
            assert g.lib.pion_gpu_project_part(g.h, 0, abi.PROJ_AXIS_PERP, 1, arr, C.byref(p), ptr) == abi.E_INVAL
            assert text in g._err()
        ok = abi.proj_part((0, 20, 0, 0.0))
        assert g.lib.pion_gpu_project_part_count(g.h, abi.PROJ_AXIS_PERP, 1, C.byref(ok)) == 70 * 20
        assert g.lib.pion_gpu_project_part(g.h, 0, abi.PROJ_AXIS_PERP, 1, arr, None, ptr) == abi.E_INVAL
        assert "no part" in g._err()
        assert g.lib.pion_gpu_project_part(g.h, 0, abi.PROJ_AXIS_PERP, 1, arr, C.byref(ok), None) == abi.E_INVAL
        assert "no buffer" in g._err()
        # everything pion_gpu_project refuses
        assert g.lib.pion_gpu_project_part(g.h, 0, 0, 1, arr, C.byref(ok), ptr) == abi.E_INVAL
        assert "along the symmetry axis" in g._err()
        assert g.lib.pion_gpu_project_part(g.h, 0, abi.PROJ_AXIS_PERP, 1, abi.proj_fields([("x", 3)]), C.byref(ok), ptr) == abi.E_INVAL
        assert "power of rho" in g._err()
        g.synchronize()
        assert (buf.cpu().numpy() == 0.0).all()   # nothing was launched
        g.download(0)                             # the handle lives on


# ---- one process per rank, through the C++ loop --------------------------------------------------------------------
class _Table(C.Structure):
    """pion_backend (pion_amd/host/pion_backend.h): the name and 28 function pointers"""
    _fields_ = [("f%d" % i, C.c_void_p) for i in range(29)]


def _host_route_table():
    from pion_amd import host_rccl
    h = host_rccl.load_host_library()
    h.pion_backend_gpu.restype = C.c_void_p
    t = _Table.from_buffer_copy(C.string_at(h.pion_backend_gpu(), C.sizeof(_Table)))
    assert t.f25 and t.f26 and t.f27 and t.f28
    t.f25 = t.f26 = t.f27 = t.f28 = None    # no projection entries: dev_project.h's functions in a host loop
    return t


def _sim(cfg, backend=None, **kw):
    from pion_amd import host_rccl
    s = host_rccl.HostSim(cfg, kw.pop("device", 0), backend=backend, **kw)
    _tables(lib.GpuSim(cfg, 0, borrowed_handle=s.gpu_handle()), cfg)
    return s


def _rank_worker(rank, world, shm, name, axis, outdir, transport, q):
    try:
        sys.path[:0] = [ROOT, TESTS]
        from pion_amd import slab
        cfg_g = pp.case(name, 0)   # the fast build
        P, fields = pr.rough_state(cfg_g, SEED), pp.fields_of(name, cfg_g)
        cfg, A = pp.slab_state(P, cfg_g, rank, world)
        ax = slab.slab_axis(cfg_g)
        lo, n, last, xmin = pp.part_of(cfg_g, rank, world)
        table = _host_route_table()
        out = []
        for tag, backend in (("dev", None), ("host", C.addressof(table))):
            kw = dict(rank=rank, world=world, periodic_z=(cfg_g.bc_type[2 * ax] == abi.BC_PERIODIC))
            if transport == "shm":
                kw.update(shm_name=shm + tag)
            else:
                kw.update(unique_id=shm[tag], device=rank)
            with _sim(cfg, backend, **kw) as s:
                s.init(slab.slab_slice(P, cfg_g, rank, world))
                s.finish_halo()
                g = lib.GpuSim(cfg, 0, borrowed_handle=s.gpu_handle())
                g.upload(A)   # the ghosts as the test makes them; the halo exchange is tests/test_gpu_host_two_ranks.py's
                s.set_slab_extent(n, lo, cfg_g.bc_type[2 * ax], cfg_g.bc_type[2 * ax + 1])
                s.write_projection(os.path.join(outdir, tag + ".fits"), pp.axis_of(cfg_g, axis), fields)
                out.append(bool(np.isnan(s.download(0)).any()))
        q.put((rank, 0, out))
    except Exception as e:   # noqa: BLE001
        q.put((rank, None, repr(e)))


def _run_ranks(world, shm, args, target=None):
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=target or _rank_worker, args=(r, world, shm) + tuple(args) + (q,)) for r in range(world)]
    res = {}
    try:
        for p in procs:
            p.start()
        for _ in range(world):
            out = q.get(timeout=120)
            res[out[0]] = out
        for p in procs:
            p.join(timeout=30)
            assert p.exitcode == 0
    finally:
        for p in procs:
            if p.is_alive():
                p.kill()
    return res


def _single_rank_file(name, axis, path, table=None):
    """the file of a single-rank sim of the global problem: device route, or (table) host route"""
    cfg_g = pp.case(name, 0)
    P, fields = pr.rough_state(cfg_g, SEED), pp.fields_of(name, cfg_g)
    with _sim(cfg_g, C.addressof(table) if table is not None else None) as s:
        s.init(P)
        lib.GpuSim(cfg_g, 0, borrowed_handle=s.gpu_handle()).upload(pp.nan_ghosts(cfg_g, P))
        s.write_projection(path, pp.axis_of(cfg_g, axis), fields)
    return open(path, "rb").read()


RANK_CASES = [("euler_tr_70x9x10", 2), ("euler_tr_70x9x10", 0), ("cyl_70x40", None)]


def _check_files(name, axis, tmp_path, transport, token):
    single = _single_rank_file(name, axis, str(tmp_path / "single.fits"))
    single_host = _single_rank_file(name, axis, str(tmp_path / "single_host.fits"), _host_route_table())
    res = _run_ranks(2, token, (name, axis, str(tmp_path), transport))
    for r in range(2):
        assert res[r][1] == 0 and all(res[r][2]), res[r]
    assert sorted(os.listdir(tmp_path)) == ["dev.fits", "host.fits", "single.fits", "single_host.fits"]
    dev, host = open(str(tmp_path / "dev.fits"), "rb").read(), open(str(tmp_path / "host.fits"), "rb").read()
    assert dev == single and host == single_host
    if pp.case(name).coord_sys != 2:
        assert host == dev   # column sums: the same bits on either route.  (The Abel weights hold a log, the device's
        #                      or the host's: tests/test_gpu_projection.py gates that difference on the single grid)


@pytest.mark.parametrize("name,axis", RANK_CASES)
def test_two_processes_over_shared_memory_write_the_single_rank_file(name, axis, tmp_path):
    _check_files(name, axis, tmp_path, "shm", "/pion_gpr%d_%d" % (os.getpid(), time.time_ns() % 1000000007))


def _ngpus():
    try:
        import torch
        return torch.cuda.device_count()
    except Exception:   # noqa: BLE001
        return 0


@pytest.mark.skipif(_ngpus() < 2, reason="needs two GPUs: ncclSend / ncclRecv of the image between two devices")
@pytest.mark.parametrize("name,axis", RANK_CASES)
def test_two_devices_over_rccl_write_the_single_rank_file(name, axis, tmp_path):
    from pion_amd import host_rccl
    _check_files(name, axis, tmp_path, "rccl", {tag: host_rccl.new_unique_id() for tag in ("dev", "host")})


# ---- a stepping cylindrical slab run: the ghost row the Abel slope reads is the halo exchange's, not the test's -------
def _axi_run(s, cfg_g, outdir):
    """regular outputs every 2 steps with two images beside each, 4 steps; the header names the base "r" """
    from test_host_snapshot import run_steps
    os.chdir(outdir)
    s.set_output("r", op_criterion=0, opfreq=2, checkpoint_freq=100)
    s.set_projection_output(abi.PROJ_AXIS_PERP, pr.fields_of(cfg_g)[:2])
    return run_steps(s, 4)


def _axi_worker(rank, world, shm, outdir, q):
    try:
        sys.path[:0] = [ROOT, TESTS]
        from pion_amd import host_rccl, problems, slab
        cfg_g, P = problems.blast_axi2d(64, abi.EQEUL, abi.FLUX_RSroe, strict_fp=1)   # 64 x 32, dx = 1/64: dyadic
        cfg = slab.slab_config(cfg_g, rank, world)
        with host_rccl.HostSim(cfg, 0, rank=rank, world=world, periodic_z=slab.slab_periodic(cfg_g), shm_name=shm) as s:
            s.init(slab.slab_slice(P, cfg_g, rank, world))
            n = cfg_g.ng[1] // world
            s.set_slab_extent(cfg_g.ng[1], rank * n, cfg_g.bc_type[2], cfg_g.bc_type[3])
            q.put((rank, 0, _axi_run(s, cfg_g, outdir)))
    except Exception as e:   # noqa: BLE001
        q.put((rank, None, repr(e)))


def test_a_stepping_cylindrical_run_of_two_ranks_writes_the_single_rank_images(tmp_path, monkeypatch):
    """blast_axi2d 64 x 32 over two ranks of 16 rows, strict build, a projection at steps 0, 2 and 4: at every output
    the row above rank 0's last own row is what finish_halo() left there.  Every image file byte for byte the file of
    the single-rank run (whose states the two-rank run reproduces: tests/test_gpu_slab2d_two_ranks.py)"""
    from pion_amd import host_rccl, problems
    a, b = tmp_path / "one", tmp_path / "two"
    a.mkdir(), b.mkdir()
    cfg_g, P = problems.blast_axi2d(64, abi.EQEUL, abi.FLUX_RSroe, strict_fp=1)
    monkeypatch.chdir(a)
    with host_rccl.HostSim(cfg_g, 0) as s:
        s.init(P)
        steps = _axi_run(s, cfg_g, str(a))
    shm = "/pion_gax%d_%d" % (os.getpid(), time.time_ns() % 1000000007)
    res = _run_ranks(2, shm, (str(b),), target=_axi_worker)
    images = ["r_proj_0000.%08d.fits" % k for k in (0, 2, 4)]
    for r in range(2):
        assert res[r][1] == 0 and res[r][2] == steps, res[r]      # every dt and time, ==
    assert sorted(f for f in os.listdir(b) if "proj" in f) == images
    from pion_amd import fits
    for f in images:
        assert open(str(a / f), "rb").read() == open(str(b / f), "rb").read(), f
        for n, img in fits.read(str(b / f))[1].items():
            assert img.shape == (32, 64) and np.isfinite(img).all() and np.abs(img).max() > 0.0, (f, n)
