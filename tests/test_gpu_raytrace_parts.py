"""The ray tracer in slab runs on the GPU, one process: a handle per slab on device 0, the planes of col carried from
handle to handle in device buffers (pion_gpu_raytrace_part), in the order pion_gpu_rt_chain gives.  The concatenation of
the slabs' arrays is compared with == against ONE handle of the whole domain (which test_gpu_raytrace.py pins to the
host loop and test_raytrace_rule.py to the restatement) and against the chained host loop
(pion_gpu_raytrace_host_part, test_raytrace_parts.py).  Both builds x both kernels (PION_RT_KERNEL).

The cases are raytrace_parts_cases.py's: internal faces inside a tile (the received plane sits in the tile, not in its
halo), faces on a tile boundary (received plane in the halo), a vertex on a face, sources off the grid, beyond the
domain along the slab axis, at infinity along and across it, the three opacity rules with negative columns.  Every
face buffer has guard words behind it."""
import numpy as np
import pytest

import raytrace_parts_cases as pc
from pion_amd import abi, driver, lib, problems, slab
from test_raytrace_rule import XMIN

pytestmark = pytest.mark.gpu

GUARD = 8


def face_buffer(n):
    import torch
    return torch.full((n + GUARD,), -7.0, dtype=torch.float64, device="cuda:0")


def guards_intact(buf, n):
    return bool((buf[n:] == -7.0).all().item())


def batches():
    """the cases grouped by what a set of handles shares (grid, ranks, geometry, state), at most MAX_RT_SOURCES each"""
    groups = {}
    for name in sorted(pc.CASES):
        ng, world, coord_sys, spec, yscale = pc.CASES[name]
        groups.setdefault((ng, world, coord_sys, yscale), []).append(name)
    out = []
    for key, names in sorted(groups.items()):
        for i in range(0, len(names), abi.MAX_RT_SOURCES):
            out.append((key, tuple(names[i:i + abi.MAX_RT_SOURCES])))
    return out


def device_chain(cfg, world, P, srcs, which=0):
    """[(col, dcol)] of the whole domain per source, from one handle per slab"""
    ax = slab.slab_axis(cfg)
    cfgs = [slab.slab_config(cfg, r, world) for r in range(world)]
    parts = [pc.part_of(cfg, r, world) for r in range(world)]
    sims = [lib.GpuSim(c, 0) for c in cfgs]
    try:
        for r, g in enumerate(sims):
            g.upload(pc.slab_state(P, cfg, r, world))
            for i, s in enumerate(srcs):
                sid, used = g.add_rt_source(s, part=parts[r])
                assert sid == i
                if not s.get("at_infinity", 0):   # the whole domain's vertex on every rank
                    want, _ = pc.rs.source_vertex(s["pos"], XMIN, pc.DX, cfg.ndim)
                    assert list(used[:cfg.ndim]) == want
        n = sims[0].rt_count(1)
        out = []
        for i, s in enumerate(srcs):
            roles = [lib.rt_chain(cfgs[r], s, parts[r]) for r in range(world)]
            lo = [face_buffer(n) for _ in range(world)]
            hi = [face_buffer(n) for _ in range(world)]
            done = set()
            while len(done) < world:
                before = len(done)
                for r in range(world):
                    recv, send_lo, send_hi = roles[r]
                    if r in done:
                        continue
                    src_rank = r - 1 if recv == abi.RT_RECV_BELOW else r + 1
                    if recv != abi.RT_RECV_NONE and src_rank not in done:
                        continue
                    fin = None
                    if recv == abi.RT_RECV_BELOW:
                        fin = hi[r - 1].data_ptr()
                    elif recv == abi.RT_RECV_ABOVE:
                        fin = lo[r + 1].data_ptr()
                    sims[r].raytrace_part(i, which, fin, lo[r].data_ptr() if send_lo else None,
                                          hi[r].data_ptr() if send_hi else None)
                    sims[r].synchronize()
                    done.add(r)
                assert len(done) > before
            assert all(guards_intact(b, n) for b in lo + hi)
            cat = 0 if ax == 2 else 1
            out.append(tuple(np.concatenate([g.rt_columns(i, what) for g in sims], cat) for what in (0, 1)))
        return out
    finally:
        for g in sims:
            g.close()


def whole_handle(cfg, P, srcs):
    with lib.GpuSim(cfg, 0) as g:
        g.upload(P)
        for s in srcs:
            g.add_rt_source(s)
        g.raytrace(0)
        return [(g.rt_columns(i, 0), g.rt_columns(i, 1)) for i in range(len(srcs))]


@pytest.mark.parametrize("kernel", ["tiles", "levels"])
@pytest.mark.parametrize("strict", [1, 0])
@pytest.mark.parametrize("key,names", batches(), ids=lambda v: "+".join(v) if isinstance(v, tuple) and isinstance(v[0], str) else None)
def test_chain_of_handles(key, names, strict, kernel, monkeypatch):
    monkeypatch.setenv("PION_RT_KERNEL", kernel)
    ng, world, coord_sys, yscale = key
    cfg = pc.global_cfg(ng, coord_sys, strict)
    P, _, _ = pc.state_of(cfg, yscale)
    srcs = [pc.source_of(cfg, pc.CASES[n][3]) for n in names]
    got = device_chain(cfg, world, P, srcs)
    want = whole_handle(cfg, P, srcs)
    for name, s, (col, dcol), (wcol, wdcol) in zip(names, srcs, got, want):
        hcol, hdcol, _ = pc.run_chain(cfg, s, world, pc.host_trace(cfg, s, world, P))
        assert np.array_equal(dcol, wdcol) and np.array_equal(dcol, hdcol), name
        bad = np.argwhere(col != wcol)
        assert bad.size == 0, (name, len(bad), bad[:5].tolist())
        assert np.array_equal(col, hcol), name


def test_whole_domain_part_equals_add_rt_source():
    ng = (27, 22, 25)
    cfg = pc.global_cfg(ng)
    P, _, _ = pc.state_of(cfg)
    srcs = [pc.source_of(cfg, sp) for sp in ({"cells": (5.0, 4.0, 3.0)}, {"cells": (30.0, -3.0, 28.0), "opacity": pc.MINUS},
                                             {"at_infinity": 1, "dir": 5})]
    want = whole_handle(cfg, P, srcs)
    with lib.GpuSim(cfg, 0) as g:
        g.upload(P)
        with lib.GpuSim(cfg, 0) as plain:
            for s in srcs:
                assert g.add_rt_source(s, part=(0, ng[2], XMIN[2])) == plain.add_rt_source(s)
        n = g.rt_count(1)
        lo, hi = face_buffer(n), face_buffer(n)
        for i in range(len(srcs)):
            g.raytrace_part(i, 0, None, lo.data_ptr(), hi.data_ptr())
            g.synchronize()
            col = g.rt_columns(i, 0)
            assert np.array_equal(col, want[i][0]) and np.array_equal(g.rt_columns(i, 1), want[i][1])
            assert np.array_equal(lo[:n].cpu().numpy().reshape(col[0].shape), col[0])
            assert np.array_equal(hi[:n].cpu().numpy().reshape(col[0].shape), col[-1])
            assert guards_intact(lo, n) and guards_intact(hi, n)
        g.raytrace(0)   # no slab face: every source at once is still allowed
        assert np.array_equal(g.rt_columns(0, 0), want[0][0])


def test_refusals_on_a_slab_handle():
    cfg = pc.global_cfg((20, 9, 12))
    c, part = slab.slab_config(cfg, 1, 3), pc.part_of(cfg, 1, 3)
    src = pc.source_of(cfg, {"cells": (7.0, 4.0, 1.0)})
    with lib.GpuSim(c, 0) as g:
        with pytest.raises(lib.PionGpuError, match="a slab of a decomposed run is not traced"):
            g.add_rt_source(src)
        for bad, text in [((-1, 12, XMIN[2]), "planes lie outside the whole domain"), ((9, 12, XMIN[2]), "planes lie outside"),
                          ((4, 12, float("nan")), "global_xmin is not finite")]:
            with pytest.raises(lib.PionGpuError, match=text):
                g.add_rt_source(src, part=bad)
        with pytest.raises(lib.PionGpuError, match="microphysics"):
            g.add_rt_source({"opacity": 7}, part=part)
        with pytest.raises(lib.PionGpuError, match="no such source"):
            g.raytrace_part(0, 0)
        assert g.add_rt_source(src, part=part)[0] == 0
        with pytest.raises(lib.PionGpuError, match="traced source by source"):
            g.raytrace(0)
        with pytest.raises(lib.PionGpuError, match="hands this part a plane"):
            g.raytrace_part(0, 0, None)
        with pytest.raises(lib.PionGpuError, match="which is 0"):
            g.raytrace_part(0, 2, 1)


def blast_slab(strict, rank=1, world=3, n=24):
    cfg, P = problems.mhd_blastwave(n, 3, abi.EQGLM, abi.FLUX_RS_HLLD, strict_fp=strict)
    return cfg, slab.slab_config(cfg, rank, world), slab.slab_slice(P, cfg, rank, world), (rank * (n // world), n, cfg.xmin[2])


def test_which_selects_p_or_ph_on_a_slab():
    """after a half step Ph differs from P; the middle slab traces either with a plane it is handed"""
    cfg, c, P, part = blast_slab(1)
    src = {"pos": (cfg.xmin[0] + 7 * cfg.dx, cfg.xmin[1] + 11 * cfg.dx, cfg.xmin[2] + 2 * cfg.dx)}
    assert lib.rt_chain(c, src, part) == (abi.RT_RECV_BELOW, 0, 1)
    face = np.random.default_rng(3).uniform(0.0, 2.0, (c.ng[1], c.ng[0]))
    with lib.GpuSim(c, 0) as g:
        sg = driver.SimControl(g, c)
        sg.init(P)
        sg.calculate_timestep()
        g.stage(0.5 * sg.dt, abi.OA1, 0)
        g.update_bcs(0.0, 1, 2, 0)
        g.add_rt_source(src, part=part)
        A = [g.download(0), g.download(1)]
        assert not np.array_equal(A[0][0], A[1][0])
        n = g.rt_count(1)
        fin, hi = face_buffer(n), face_buffer(n)
        import torch
        fin[:n] = torch.from_numpy(face.reshape(-1)).to("cuda:0")
        for which in (0, 1):
            g.raytrace_part(0, which, fin.data_ptr(), None, hi.data_ptr())
            g.synchronize()
            hcol, hdcol = lib.raytrace_host_part(c, src, part, A[which], face)
            assert np.array_equal(g.rt_columns(0, 0), hcol) and np.array_equal(g.rt_columns(0, 1), hdcol)
            assert np.array_equal(hi[:n].cpu().numpy().reshape(face.shape), hcol[-1]) and guards_intact(hi, n)


@pytest.mark.parametrize("strict", [1, 0])
def test_tracing_a_slab_is_read_only(strict):
    """a traced slab handle stepped twice: P and every dt == the same run without sources"""
    cfg, c, P, part = blast_slab(strict)
    out = []
    for traced in (False, True):
        with lib.GpuSim(c, 0) as g:
            sg = driver.SimControl(g, c)
            sg.init(P)
            n = g.rt_count(1)
            fin, lo, hi = face_buffer(n), face_buffer(n), face_buffer(n)
            fin[:n] = 0.5
            if traced:
                g.add_rt_source({"pos": (cfg.xmin[0] + 7 * cfg.dx, cfg.xmin[1], cfg.xmin[2] + 3 * cfg.dx)}, part=part)
                g.add_rt_source({"at_infinity": 1, "dir": 5}, part=part)

            def trace(which):
                if traced:
                    g.raytrace_part(0, which, fin.data_ptr(), None, hi.data_ptr())
                    g.raytrace_part(1, which, fin.data_ptr(), lo.data_ptr(), None)
            dts = []
            for _ in range(2):
                trace(0)
                sg.calculate_timestep()
                dts.append(sg.dt)
                trace(1)
                sg.advance_time()
            trace(0)
            if traced:
                assert np.all(np.isfinite(g.rt_columns(0, 0))) and g.rt_columns(1, 0).min() >= 0.5
            out.append((dts, g.download(0)))
    assert out[0][0] == out[1][0]
    assert np.array_equal(out[0][1], out[1][1], equal_nan=True)


# ---- one process per rank, through the C++ loop: every rank writes its own columns file ------------------------------
import multiprocessing as mp   # noqa: E402
import os                      # noqa: E402
import sys                     # noqa: E402
import time                    # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TESTS = os.path.join(ROOT, "tests")
OUTPUTS = (0, 2, 4)


def loop_case(which):
    """(cfg, P, sources, world): the 3-D box of test_host_columns_ranks.py over 3 ranks, or a cylindrical (z,R) blast of
    64 x 32 cells (dx = 1/64: dyadic) over 2 ranks with a source on the axis, one in rank 1 and one at infinity"""
    if which == "box3d":
        import test_host_columns_ranks as hc
        return hc.case() + (3,)
    cfg, P = problems.blast_axi2d(64, abi.EQEUL, abi.FLUX_RSroe, ntracer=1, strict_fp=1)
    P[5] = 0.5
    d = cfg.dx
    sources = [{"pos": (cfg.xmin[0] + 5.0 * d, 0.0), "opacity": abi.RT_OPACITY_TRACER},
               {"pos": (cfg.xmin[0] + 40.0 * d, 20.0 * d), "opacity": abi.RT_OPACITY_MINUS},
               {"at_infinity": 1, "dir": 3}]
    return cfg, P, sources, 2


def _loop_run(s, sources, outdir):
    from pion_amd import host_rccl
    from test_host_snapshot import run_steps
    used = [s.add_rt_source(src) for src in sources]
    os.chdir(outdir)   # the header names the base: the same one, "r", in every run
    s.set_output("r", op_criterion=0, opfreq=2, checkpoint_freq=100)
    s.set_output_filetype(host_rccl.FILE_FITS)
    s.set_column_output(True)
    return run_steps(s, 4), used


def _loop_worker(rank, world, token, which, outdir, transport, q):
    try:
        sys.path[:0] = [ROOT, TESTS]
        from pion_amd import host_rccl
        cfg_g, P, sources, _ = loop_case(which)
        ax = slab.slab_axis(cfg_g)
        cfg = slab.slab_config(cfg_g, rank, world)
        kw = dict(rank=rank, world=world, periodic_z=slab.slab_periodic(cfg_g))
        if transport == "shm":
            kw.update(shm_name=token)
        else:
            kw.update(unique_id=token)
        with host_rccl.HostSim(cfg, rank if transport == "rccl" else 0, **kw) as s:
            s.init(slab.slab_slice(P, cfg_g, rank, world))
            n = cfg_g.ng[ax] // world
            s.set_slab_extent(cfg_g.ng[ax], rank * n, cfg_g.bc_type[2 * ax], cfg_g.bc_type[2 * ax + 1])
            q.put((rank, 0) + _loop_run(s, sources, outdir))
    except Exception as e:   # noqa: BLE001
        q.put((rank, None, repr(e), None))


def _run_ranks(world, args):
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_loop_worker, args=(r, world) + tuple(args) + (q,)) for r in range(world)]
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


def _check_loop(which, transport, token, tmp_path, monkeypatch):
    from pion_amd import fits, host_rccl
    cfg_g, P, sources, world = loop_case(which)
    one, many = tmp_path / "one", tmp_path / "many"
    one.mkdir(), many.mkdir()
    res = _run_ranks(world, (token, which, str(many), transport))
    monkeypatch.chdir(one)
    with host_rccl.HostSim(cfg_g, 0) as s:
        s.init(P)
        steps, used = _loop_run(s, sources, str(one))
    for r in range(world):
        assert res[r][1] == 0, res[r]
        assert res[r][2] == steps and res[r][3] == used       # every dt and time; the whole domain's positions
    cols = ["r_cols_%04d.%08d.fits" % (r, k) for r in range(world) for k in OUTPUTS]
    assert sorted(f for f in os.listdir(many) if "cols" in f) == sorted(cols)
    for k in OUTPUTS:
        sparams, simages = fits.read(str(one / ("r_cols_0000.%08d.fits" % k)))
        rt = {key: v for key, v in sparams.items() if key.startswith("RT_")}
        parts = []
        for r in range(world):
            params, images = fits.read(str(many / ("r_cols_%04d.%08d.fits" % (r, k))))
            assert {key: v for key, v in params.items() if key.startswith("RT_")} == rt
            rparams, _ = fits.read(str(many / ("r_%04d.%08d.fits" % (r, k))))
            assert {key: v for key, v in params.items() if not key.startswith("RT_")} == rparams
            parts.append(images)
        assert len(simages) == 2 * len(sources)
        for name in simages:
            got = np.concatenate([p[name] for p in parts], 0)
            assert got.shape == simages[name].shape
            assert np.array_equal(got.view(np.uint64), simages[name].view(np.uint64)), (k, name)
            assert np.isfinite(got).all() and got.max() > 0.0
    return many, cols


@pytest.mark.parametrize("which", ["box3d", "axi2d"])
def test_ranks_over_shared_memory_write_the_planes_of_the_single_rank_file(which, tmp_path, monkeypatch):
    many, cols = _check_loop(which, "shm", "/pion_grt%d_%d" % (os.getpid(), time.time_ns() % 1000000007), tmp_path, monkeypatch)
    if which == "box3d":
        # the device's files are byte for byte the ones the CPU loop (the oracle's table, the host route) writes
        import test_host_columns_ranks as hc
        cpu = tmp_path / "cpu"
        cpu.mkdir()
        res = hc._run_ranks(hc._run_worker, hc.WORLD, (str(cpu), True))
        assert all(res[r][1] is not None for r in range(hc.WORLD)), res
        for f in cols:
            assert open(str(many / f), "rb").read() == open(str(cpu / f), "rb").read(), f


def _ngpus():
    try:
        import torch
        return torch.cuda.device_count()
    except Exception:   # noqa: BLE001
        return 0


@pytest.mark.skipif(_ngpus() < 3, reason="needs a GPU per rank: ncclSend / ncclRecv of the planes between three devices")
def test_three_devices_over_rccl_write_the_planes_of_the_single_rank_file(tmp_path, monkeypatch):
    from pion_amd import host_rccl
    _check_loop("box3d", "rccl", host_rccl.new_unique_id(), tmp_path, monkeypatch)


@pytest.mark.skipif(_ngpus() < 2, reason="needs a GPU per rank: ncclSend / ncclRecv of the planes between two devices")
def test_two_devices_over_rccl_write_the_planes_of_the_single_rank_file(tmp_path, monkeypatch):
    from pion_amd import host_rccl
    _check_loop("axi2d", "rccl", host_rccl.new_unique_id(), tmp_path, monkeypatch)
