"""Ray-traced column densities on the GPU: the kernels of pion_raytrace.hip (pion_gpu_raytrace) against the host loop
over the same rules (pion_gpu_raytrace_host, which test_raytrace_rule.py pins against the restatement of the
reference), col and dcol with ==: square root and division are IEEE operations on both sides and the file is built
without contraction or approximate functions, so nothing is left that may differ.

Both builds x both kernels (tiles, and levels through PION_RT_KERNEL=levels).  Shapes: 27 x 22 x 25 (2 x 3 x 3 tiles of
16 x 8 x 8 per octant, all partial, every distance threshold crossed), 9 x 7 x 5 (smaller than one tile), 2-D 41 x 23
(smaller than one 32 x 64 tile) and 70 x 150 (3 x 3 tiles), Cartesian and cylindrical; sources inside, on the edge, off
the grid, and where a tile ends with the grid's last cell.  Sources at infinity on 70 x 9 x 8 and 70 x 67: 72 and 67
rows are more than one wavefront's 64, 70 cells more than two staging blocks of 32.  The states hold NaN in every
ghost cell and get no boundary update: only on-grid cells are read."""
import ctypes as C

import numpy as np
import pytest

import raytrace_restate as rs
from pion_amd import abi, driver, lib, problems
from test_raytrace_rule import DX, XMIN, make_cfg, make_state, pos_of

pytestmark = pytest.mark.gpu


def cfg_of(ng, strict, coord_sys=1):
    bcs = None
    if coord_sys == 2:
        bcs = ["outflow", "outflow", "axisymmetric", "outflow"]
    cfg = make_cfg(ng, coord_sys=coord_sys, bcs=bcs)
    cfg.strict_fp = strict
    return cfg


def device_columns(cfg, P, srcs, which=0):
    """[(col, dcol)] per source from one handle"""
    with lib.GpuSim(cfg, 0) as g:
        g.upload(P)
        ids = [g.add_rt_source(s)[0] for s in srcs]
        assert ids == list(range(len(srcs)))
        g.raytrace(which)
        return [(g.rt_columns(i, 0), g.rt_columns(i, 1)) for i in ids]


def compare(cfg, srcs):
    P, _, _ = make_state(cfg)
    got = device_columns(cfg, P, srcs)
    for s, (col, dcol) in zip(srcs, got):
        hcol, hdcol = lib.raytrace_host(cfg, s, P)
        assert np.array_equal(dcol, hdcol), s
        bad = np.argwhere(col != hcol)
        assert bad.size == 0, (s, len(bad), bad[:5].tolist())


POINT_CASES = {
    "3d-interior": ((27, 22, 25), 1, [(5.0, 4.0, 3.0)]),
    "3d-off-grid": ((27, 22, 25), 1, [(-3.0, 25.0, 3.0), (30.0, -3.0, 28.0)]),
    "3d-tile-ends-with-grid": ((27, 22, 25), 1, [(16.0, 8.0, 8.0), (26.0, 21.0, 24.0), (11.0, 14.0, 17.0)]),
    "3d-corners": ((27, 22, 25), 1, [(0.0, 0.0, 0.0), (27.0, 22.0, 25.0)]),
    "3d-small": ((9, 7, 5), 1, [(4.0, 3.0, 2.0), (0.0, 0.0, 2.0), (-3.0, 10.0, 2.0)]),
    "2d-small": ((41, 23), 1, [(7.0, 5.0), (0.0, 6.0), (44.0, -3.0)]),
    "2d-tiles": ((70, 150), 1, [(32.0, 64.0), (69.0, 149.0), (3.0, 75.0), (-3.0, 153.0)]),
    "2d-cylindrical": ((70, 150), 2, [(35.0, 0.0), (20.0, 70.0)]),
}


@pytest.mark.parametrize("kernel", ["tiles", "levels"])
@pytest.mark.parametrize("strict", [1, 0])
@pytest.mark.parametrize("case", sorted(POINT_CASES))
def test_point_sources(case, strict, kernel, monkeypatch):
    ng, coord_sys, where = POINT_CASES[case]
    monkeypatch.setenv("PION_RT_KERNEL", kernel)
    cfg = cfg_of(ng, strict, coord_sys)
    srcs = [{"pos": pos_of(cfg, w)} for w in where]
    for i in range(0, len(srcs), abi.MAX_RT_SOURCES):
        compare(cfg, srcs[i:i + abi.MAX_RT_SOURCES])


@pytest.mark.parametrize("strict", [1, 0])
@pytest.mark.parametrize("ng", [(70, 9, 8), (70, 67)])
def test_sources_at_infinity(ng, strict):
    cfg = cfg_of(ng, strict)
    dirs = list(range(2 * len(ng)))
    for i in range(0, len(dirs), abi.MAX_RT_SOURCES):
        compare(cfg, [{"at_infinity": 1, "dir": d, "opacity": abi.RT_OPACITY_TOTAL + d % 3} for d in dirs[i:i + 4]])


@pytest.mark.parametrize("kernel", ["tiles", "levels"])
def test_opacity_rules_and_two_sources_on_one_handle(kernel, monkeypatch):
    monkeypatch.setenv("PION_RT_KERNEL", kernel)
    cfg = cfg_of((27, 22, 25), 1)
    compare(cfg, [{"pos": pos_of(cfg, (5.0, 4.0, 3.0)), "opacity": abi.RT_OPACITY_MINUS},
                  {"pos": pos_of(cfg, (20.0, 11.0, 30.0)), "opacity": abi.RT_OPACITY_TRACER},
                  {"at_infinity": 1, "dir": 3, "opacity": abi.RT_OPACITY_MINUS}])


def test_position_used_is_the_reference_vertex():
    cfg = cfg_of((9, 7, 5), 1)
    with lib.GpuSim(cfg, 0) as g:
        for cells in [(4.5, 3.3, 2.7), (4.0, 3.0, 2.0), (-2.5, 8.5, 0.49), (0.5, 0.5, 0.5)]:
            want, _ = rs.source_vertex(pos_of(cfg, cells), XMIN, DX, 3)
            _, used = g.add_rt_source({"pos": pos_of(cfg, cells)})
            assert list(used) == want


def test_refusals_on_a_handle():
    cfg = cfg_of((9, 7), 1)
    with lib.GpuSim(cfg, 0) as g:
        g.raytrace(0)   # no sources: nothing to do
        with pytest.raises(lib.PionGpuError, match="no such source"):
            g.rt_columns(0, 0)
        with pytest.raises(lib.PionGpuError, match="microphysics"):
            g.add_rt_source({"opacity": 5})
        with pytest.raises(lib.PionGpuError, match="a face of the grid"):
            g.add_rt_source({"at_infinity": 1, "dir": 4})
        for i in range(abi.MAX_RT_SOURCES):
            assert g.add_rt_source({"pos": pos_of(cfg, (i, 1.0))})[0] == i
        with pytest.raises(lib.PionGpuError, match="more than PION_MAX_RT_SOURCES"):
            g.add_rt_source({"pos": pos_of(cfg, (1.0, 1.0))})
        with pytest.raises(lib.PionGpuError, match="no such source"):
            g.rt_columns(0, 2)
    slab = make_cfg((9, 7, 5), bcs=["outflow"] * 4 + ["slab", "outflow"])
    with lib.GpuSim(slab, 0) as g:
        with pytest.raises(lib.PionGpuError, match="a slab of a decomposed run is not traced"):
            g.add_rt_source({})


def blast(strict, n=24):
    return problems.mhd_blastwave(n, 3, abi.EQGLM, abi.FLUX_RS_HLLD, strict_fp=strict)


def test_which_selects_p_or_ph():
    """after a half step Ph differs from P: which = 1 traces Ph, which = 0 still P"""
    cfg, P = blast(1)
    src = {"pos": (cfg.xmin[0] + 7 * cfg.dx, cfg.xmin[1] + 11 * cfg.dx, cfg.xmin[2] + 30 * cfg.dx)}
    with lib.GpuSim(cfg, 0) as g:
        sg = driver.SimControl(g, cfg)
        sg.init(P)
        sg.calculate_timestep()
        g.stage(0.5 * sg.dt, abi.OA1, 0)
        g.update_bcs(0.0, 1, 2, 0)
        g.add_rt_source(src)
        A = [g.download(0), g.download(1)]
        assert not np.array_equal(A[0][0], A[1][0])
        for which in (0, 1):
            g.raytrace(which)
            hcol, hdcol = lib.raytrace_host(cfg, src, A[which])
            assert np.array_equal(g.rt_columns(0, 0), hcol)
            assert np.array_equal(g.rt_columns(0, 1), hdcol)


@pytest.mark.parametrize("strict", [1, 0])
def test_tracing_is_read_only(strict):
    """a traced handle stepped twice: P and every dt == the same run without sources"""
    cfg, P = blast(strict)
    out = []
    for traced in (False, True):
        with lib.GpuSim(cfg, 0) as g:
            sg = driver.SimControl(g, cfg)
            sg.init(P)
            if traced:
                g.add_rt_source({"pos": (cfg.xmin[0] + 7 * cfg.dx, cfg.xmin[1], cfg.xmin[2] + 3 * cfg.dx)})
                g.add_rt_source({"at_infinity": 1, "dir": 0})
            dts = []
            for _ in range(2):
                if traced:
                    g.raytrace(0)
                sg.calculate_timestep()
                dts.append(sg.dt)
                if traced:
                    g.raytrace(1)
                sg.advance_time()
            if traced:
                g.raytrace(0)
                assert np.all(np.isfinite(g.rt_columns(0, 0))) and g.rt_columns(1, 0).max() > 0.0
            out.append((dts, g.download(0)))
    assert out[0][0] == out[1][0]
    assert np.array_equal(out[0][1], out[1][1])


@pytest.mark.parametrize("ng", [(27, 22, 25), (41, 23)])
def test_pack_columns_is_the_byte_swapped_array(ng):
    import torch
    cfg = cfg_of(ng, 1)
    P, _, _ = make_state(cfg)
    with lib.GpuSim(cfg, 0) as g:
        g.upload(P)
        g.add_rt_source({"pos": pos_of(cfg, (5.0, 4.0, 3.0)[:len(ng)])})
        g.raytrace(0)
        planes = ng[-1]
        per = g.rt_count(1)
        assert per == int(np.prod(ng[:-1])) and g.rt_count(planes) == int(np.prod(ng))
        for what in (0, 1):
            a = g.rt_columns(0, what).reshape(planes, -1)
            lo = 0
            for chunk in (1, 7, planes):   # chunk by chunk; the last one takes what is left
                hi = min(planes, lo + chunk)
                if lo >= hi:
                    break
                n = g.rt_count(hi - lo)
                buf = torch.full((n + 8,), -7.0, dtype=torch.float64, device="cuda:0")
                g.pack_columns(0, what, lo, hi, buf.data_ptr())
                g.synchronize()
                raw = buf.cpu().numpy()
                assert np.all(raw[n:] == -7.0)
                assert np.array_equal(raw[:n].view(">f8").astype("<f8").reshape(hi - lo, -1), a[lo:hi])
                lo = hi
        for lo, hi in [(-1, 2), (0, planes + 1), (3, 3)]:
            with pytest.raises(lib.PionGpuError, match="plane range"):
                g.pack_columns(0, 0, lo, hi, 1)
