"""Plane windows of the rows kernel (rows_tiling.h "plane windows", stage_launch in pion_step.hip): a handle whose
stages run as several launches of k_stage_rows2, each rebased to its window of planes (3-D) or rows (2-D), must give
bit for bit what the one-launch handle gives -- P, Ph, every dt, the HLLD -> HLL switch array and the error word, in
the strict AND the fast build: the same kernel code solves every interface wherever a launch starts (the property
tests/test_gpu_slab2d_parts.py relies on for interior + strips).

Each case builds two handles on the same input: one with PION_ROWS_WINDOW_CELLS unset, one with it set (around create
only) to L = (w + 2 nbc) s + 1, the smallest limit under which w planes of s cells fit one window.  Both run two full
second-order steps -- boundary update, half stage, boundary update, full stage, calc_dt -- and are compared after
every stage.  The one-launch run of a case is computed once and shared by the limits it is compared with.

Shapes: the smallest that reach every seam.  3-D GLM-MHD HLLD 70 x 9 x 11, periodic: one full 62-cell x tile plus a
remainder tile, ny odd against 2 and 4 rows per wavefront, x ghost images written by the kernel; windows of <= 3
planes (3, 3, 3, 2), of one plane (11 launches), and a limit that fits the grid (one window: the launches of the
unset handle).  Euler Roe-CV 64 x 8 x 9 reflecting / outflow: the plain instance at three wavefronts per SIMD.  Euler +
tracer FVS with cooling and a device-built wind source 20 x 10 x 9: cell flags are read, k_cooling_dE runs before
and k_dt_mp behind the windows.  Ideal MHD Roe with the H-correction 20 x 8 x 9: the eta arrays are rebased.  The GLM
case through PION_STAGE_INTERIOR + PION_STAGE_SLABBOUNDARY with the z faces looped back: the strips become launches
of their own.  2-D: Euler with the double-Mach-reflection faces 70 x 37 (<= 5 rows), GLM periodic 130 x 20 (<= 3 rows),
cylindrical Euler and GLM 64 x 24 with dyadic dx and xmin (<= 5 rows; the launch's copy of xmin[1] moves with the
window, exact for dyadic values)."""
import copy
import math

import numpy as np
import pytest

from pion_amd import abi, cooling, driver, lib, problems, wind

pytestmark = pytest.mark.gpu


def _stride(cfg):
    s = cfg.ng[0] + 2 * cfg.nbc
    return s * (cfg.ng[1] + 2 * cfg.nbc) if cfg.ndim == 3 else s


def _limit(cfg, w):
    """the smallest limit under which w planes fit one window: floor((L - 1) / s) - 2 nbc = w"""
    return (w + 2 * cfg.nbc) * _stride(cfg) + 1


def _handle(cfg, limit, monkeypatch):
    """a handle created with the knob set to `limit` (None: unset); the knob is read at create only"""
    if limit is None:
        monkeypatch.delenv("PION_ROWS_WINDOW_CELLS", raising=False)
    else:
        monkeypatch.setenv("PION_ROWS_WINDOW_CELLS", str(limit))
    g = lib.GpuSim(cfg, 0)
    monkeypatch.delenv("PION_ROWS_WINDOW_CELLS", raising=False)
    return g


# ---- cases: (cfg, P, wind sources, needs cooling tables)

def _glm3d(strict):
    cfg, _ = problems.mhd_blastwave(4, 3, abi.EQGLM, abi.FLUX_RS_HLLD, strict_fp=strict)
    cfg.ng[0], cfg.ng[1], cfg.ng[2] = 70, 9, 11
    cfg.dx = 1.0 / 70
    cfg.xmin[1], cfg.xmin[2] = -4.5 / 70, -5.5 / 70      # the hot sphere (radius 7 cells) centred along y and z
    P = problems.fill_mhd_blastwave(cfg)
    x, y, z = problems.cell_centres(cfg)
    # flow across every window seam from the first step
    P[abi.VZ] = 0.3 * np.cos(2 * np.pi * x)[None, None, :] + 0.1
    P[abi.VX] = 0.2 * np.sin(2 * np.pi * z * 70 / 11)[:, None, None]
    P[abi.BZ] = 0.3
    return cfg, P, [], False


def _roe3d(strict):
    cfg, P = problems.hd_blast_box([64, 8, 9], solver=abi.FLUX_RSroe, strict_fp=strict)
    return cfg, P, [], False


def _wind3d(strict):
    L = 3.160064e18
    cfg = abi.make_config(3, [20, 10, 9], abi.EQEUL, abi.FLUX_FVS, ntracer=1, artvisc=abi.AV_FKJ98_1D, etav=0.15,
                          gamma=1.6666666666666667, cfl=0.3, dx=L / 20, xmin=(0.0, 0.0, 0.0),
                          bcs=["reflecting", "one-way-outflow"] * 3,
                          refvec=[1.0e-24, 1.0e-13, 1.0e6, 1.0e6, 1.0e6, 1.0], min_temp=5.0e3, max_temp=1.0e8,
                          cooling=abi.COOL_WSS09_CIE_LINE_HEAT_COOL, mp_timestep_limit=1, strict_fp=strict)
    P = problems.alloc(cfg)
    X, Y, Z = problems.mesh(cfg)
    hot = (X - 0.5 * L) ** 2 + Y * Y + (Z - 0.2 * L) ** 2 < (0.25 * L) ** 2
    mu_over_kb = 0.609 * 1.672621898e-24 / 1.38064852e-16
    P[abi.RO] = np.where(hot, 20.0, 1.0) * 2.124229813e-24
    P[abi.PG] = P[abi.RO] * np.where(hot, 2.0e6, 7.5e3) / mu_over_kb
    P[abi.VZ] = 2.0e6 * (1.0 + 0.5 * np.sin(2 * np.pi * X / L))
    P[5] = np.where(hot, 1.0, 0.0)
    # the source sits on the reflecting corner: its cells span the planes 0 .. 3, i.e. two windows
    src = wind.WindSource(pos=(0.0, 0.0, 0.0), radius=3.3 * cfg.dx, mdot=1.0e-7, vinf=1500.0, vrot=0.0, Tw=3.0e4,
                          Rstar=6.96e11, Bstar=0.0, tracers=[1.0])
    return cfg, P, [src], True


def _hcorr3d(strict):
    cfg, P = problems.mhd_blast_generic([20, 8, 9], abi.EQMHD, abi.FLUX_RSroe, strict_fp=strict)
    cfg.artvisc = abi.AV_HCORR_FKJ98
    return cfg, P, [], False


def _dmr2d(strict):
    nx, ny = 70, 37
    cfg = abi.make_config(2, [nx, ny], abi.EQEUL, abi.FLUX_RSroe, artvisc=abi.AV_FKJ98_1D, etav=0.1, gamma=1.4, cfl=0.4,
                          dx=3.25 / nx, xmin=(0.0, 0.0, 0.0), bcs=["inflow", "outflow", "reflecting", "DMR"],
                          bc_dmach2=1, refvec=[1.0] * 5, strict_fp=strict)
    P = problems.alloc(cfg)
    X, Y, _ = problems.mesh(cfg)
    post = X <= 1.0 / 6.0 + Y / math.tan(math.pi / 3.0)
    P[abi.RO] = np.where(post, 8.0, 1.4)
    P[abi.PG] = np.where(post, 116.5, 1.0)
    P[abi.VX] = np.where(post, 7.14470958, 0.0)
    P[abi.VY] = np.where(post, -4.125, 0.0)
    return cfg, P, [], False


def _glm2d(strict):
    cfg, P = problems.mhd_blast_generic([130, 20], abi.EQGLM, abi.FLUX_RS_HLLD, strict_fp=strict)
    return cfg, P, [], False


def _cyl2d(eqntype, solver, strict):
    """problems.blast_axi2d's field on 64 x 24 cells: dx = 1/64 and xmin = (-1/2, 0) are dyadic"""
    cfg, _ = problems.blast_axi2d(64, eqntype, solver, strict_fp=strict)
    cfg.ng[1] = 24
    P = problems.alloc(cfg)
    X, Y, _ = problems.mesh(cfg)
    r2 = X * X + Y * Y
    P[abi.RO] = 1.0 + 0.3 * np.exp(-r2 / 0.05)
    P[abi.PG] = np.where(r2 < 0.15 * 0.15, 10.0, 0.1)
    P[abi.VX] = 0.2 * np.sin(2 * np.pi * X)
    P[abi.VY] = 0.1 * Y
    P[abi.VZ] = 0.3 * Y
    if eqntype != abi.EQEUL:
        P[abi.BX] = 0.5
        P[abi.BY] = 0.05 * Y
        P[abi.BZ] = 0.2 * Y
    if eqntype == abi.EQGLM:
        P[abi.SI] = 0.01 * np.sin(2 * np.pi * X) * Y
    return cfg, P, [], False


CASES = {
    "glm3d": _glm3d, "roe3d": _roe3d, "wind3d": _wind3d, "hcorr3d": _hcorr3d, "dmr2d": _dmr2d, "glm2d": _glm2d,
    "cyl2d_euler": lambda s: _cyl2d(abi.EQEUL, abi.FLUX_RSroe, s),
    "cyl2d_glm": lambda s: _cyl2d(abi.EQGLM, abi.FLUX_RS_HLLD, s),
}

_TABLES = {}


def _tables(cfg):
    key = (cfg.min_temp, cfg.max_temp)
    if key not in _TABLES:
        _TABLES[key] = cooling.build_tables(*key)
    return _TABLES[key]


class SelfComm:
    """SlabComm's call shape for a periodic slab whose z neighbour is itself (as tests/test_gpu_split_stage.py)"""

    def __init__(self, sim, two_streams):
        import torch
        n = sim.halo_count()
        self.top = torch.empty(n, dtype=torch.float64, device="cuda:0")
        self.bottom = torch.empty(n, dtype=torch.float64, device="cuda:0")
        self.pending = None
        self.streams = None
        if two_streams:
            sim.synchronize()
            self.streams = (torch.cuda.Stream(), torch.cuda.Stream(priority=-1))
            sim.set_stream(self.streams[0].cuda_stream)
            sim.set_comm_stream(self.streams[1].cuda_stream)

    def start(self, sim, which):
        assert self.pending is None
        sim.pack_halo(which, 5, self.top.data_ptr())
        sim.pack_halo(which, 4, self.bottom.data_ptr())
        self.pending = which

    def finish(self, sim):
        if self.pending is None:
            return
        which, self.pending = self.pending, None
        sim.unpack_halo(which, 4, self.top.data_ptr())
        sim.unpack_halo(which, 5, self.bottom.data_ptr())

    def allreduce_min(self, a, b):
        return a, b


def _run(g, cfg, P, srcs, tables, comm_mode=None, nsteps=2):
    """two second-order steps; returns the list of everything observed, in order, and the stage-kernel launches of the
    last part of each stage.  A device error word raises from calc_dt / download (lib.PionGpuError): recorded, too."""
    seen, launches = [], []
    hlld = (cfg.solver == abi.FLUX_RS_HLLD and cfg.eqntype != abi.EQEUL)
    if tables:
        g.set_cooling_tables(*_tables(cfg))
    comm = None if comm_mode is None else SelfComm(g, comm_mode == "streams")
    sc = driver.SimControl(g, cfg, comm=comm)
    for s in srcs:
        sc.add_wind_source(s)
    try:
        sc.init(P)
        for n in range(nsteps):
            dt = sc.calculate_timestep()
            seen.append(("dt %d" % n, np.array([dt])))
            sc._stage(0.5 * dt, abi.OA1, 0)
            launches.append(g.rows_windows()["launches_last_part"])
            sc.update_bcs(abi.OA1, abi.OA2)
            if comm is None:   # (a read-back between the parts of a split stage would join its streams)
                seen.append(("Ph %d" % n, g.download(1)))
                if hlld:
                    seen.append(("switch of the half stage %d" % n, g.get_hll_switch()))
            sc._stage(dt, abi.OA2, 1)
            launches.append(g.rows_windows()["launches_last_part"])
            sc.update_bcs(abi.OA2, abi.OA2)
            sc.simtime += dt
            sc.last_dt = dt
            sc.timestep += 1
            if comm is None:
                seen.append(("P %d" % n, g.download(0)))
                if hlld:
                    seen.append(("switch of the full stage %d" % n, g.get_hll_switch()))
        sc.finish_halo()
        seen.append(("P end", g.download(0)))
        if hlld:
            seen.append(("switch end", g.get_hll_switch()))
        seen.append(("dt end", np.array(g.calc_dt())))
    except lib.PionGpuError as e:
        seen.append(("error", np.array([e.rc])))
        seen.append((str(e), np.array([e.rc])))
    return seen, launches


_BASE = {}


def _baseline(case, strict, monkeypatch):
    """the one-launch run of a case (knob unset), computed once"""
    key = (case, strict)
    if key not in _BASE:
        cfg, P, srcs, tables = CASES[case](strict)
        with _handle(cfg, None, monkeypatch) as g:
            info = g.rows_windows()
            assert info["windows_whole_stage"] == 1 and info["limit_cells"] == 1 << 29
            seen, launches = _run(g, cfg, P, srcs, tables)
        assert launches == [1] * len(launches)
        assert seen[-1][0] == "dt end", seen[-1][0]                  # (no device error in the reference run)
        assert np.isfinite(seen[-2][1] if seen[-2][0] == "P end" else seen[-3][1]).all()
        _BASE[key] = (seen, launches)
    return _BASE[key]


def _same(want, got, cut=None):
    assert [k for k, _ in want] == [k for k, _ in got]
    for (k, a), (_, b) in zip(want, got):
        if cut is not None and a.size > 2:
            a, b = cut(a), cut(b)
        print("%-28s differs in %d of %d values" % (k, (a != b).sum(), a.size))
        assert np.array_equal(a, b), "%s: %d values differ" % (k, (a != b).sum())


# (case, planes or rows per window, the windows expected of a whole stage)
WINDOWED = [
    ("glm3d", 3, [3, 3, 3, 2]),
    ("glm3d", 1, [1] * 11),
    ("glm3d", 11, [11]),
    ("roe3d", 4, [3, 3, 3]),
    ("wind3d", 4, [3, 3, 3]),
    ("hcorr3d", 4, [3, 3, 3]),
    ("dmr2d", 5, [5, 5, 5, 5, 5, 4, 4, 4]),
    ("glm2d", 3, [3, 3, 3, 3, 3, 3, 2]),
    ("cyl2d_euler", 5, [5, 5, 5, 5, 4]),
    ("cyl2d_glm", 5, [5, 5, 5, 5, 4]),
]


@pytest.mark.parametrize("strict", [1, 0], ids=["strict", "fast"])
@pytest.mark.parametrize("case,w,sizes", WINDOWED, ids=["%s-w%d" % (c, w) for c, w, _ in WINDOWED])
def test_windowed_stages_equal_one_launch(case, w, sizes, strict, monkeypatch):
    want, _ = _baseline(case, strict, monkeypatch)
    cfg, P, srcs, tables = CASES[case](strict)
    L = _limit(cfg, w)
    plan = lib.rows_windows(cfg, limit=L)
    assert [b - a for a, b in plan] == sizes
    with _handle(cfg, L, monkeypatch) as g:
        info = g.rows_windows()
        assert info["limit_cells"] == L and info["windows_whole_stage"] == len(sizes)
        got, launches = _run(g, cfg, P, srcs, tables)
    assert launches == [len(sizes)] * 4, launches
    if len(sizes) > 1:
        assert info["windows_whole_stage"] > 1
    _same(want, got)


@pytest.mark.parametrize("strict", [1, 0], ids=["strict", "fast"])
@pytest.mark.parametrize("mode", ["one_stream", "streams"])
def test_windowed_split_stage_equals_whole_stage(mode, strict, monkeypatch):
    """interior + strips of a handle with windows of <= 3 planes against the whole stages of the one-launch handle; the
    interior [2, 9) runs as 3 launches, the two strips of 2 planes as one launch each"""
    want, _ = _baseline("glm3d", strict, monkeypatch)
    cfg, P, srcs, tables = CASES["glm3d"](strict)
    nb, nz = cfg.nbc, cfg.ng[2]
    cfg_s = copy.deepcopy(cfg)
    cfg_s.bc_type[4] = cfg_s.bc_type[5] = abi.BC_SLAB
    L = _limit(cfg_s, 3)
    assert lib.rows_windows(cfg_s, nb, nz - nb, limit=L) == [(2, 5), (5, 7), (7, 9)]
    assert lib.rows_windows(cfg_s, 0, nb, limit=L) == [(0, 2)]
    with _handle(cfg_s, L, monkeypatch) as g:
        assert g.rows_windows()["windows_whole_stage"] == 4
        got, launches = _run(g, cfg_s, P, srcs, tables, comm_mode=mode)
    assert launches == [2] * 4, launches      # the last part of every stage: the strips, one launch each
    keep = {"dt 0", "dt 1", "P end", "switch end", "dt end"}
    # on-grid planes and one plane beyond each z face (the parts do not write the outermost ghost planes' flags;
    # the z ghost planes of P arrive by the halo, which a periodic run fills with the same values)
    nga = abi.ng_all(cfg)

    def cut(a):
        a = a.reshape(-1, nga[2], nga[1], nga[0])
        return a[:, nb - 1:nb + nz + 1]

    _same([kv for kv in want if kv[0] in keep], got, cut)


def test_interior_windows_are_separate_launches(monkeypatch):
    """PION_STAGE_INTERIOR of the windowed handle alone: 3 launches for [2, 9) under windows of <= 3 planes, 7 under
    windows of one plane"""
    cfg, P, _, _ = CASES["glm3d"](1)
    cfg.bc_type[4] = cfg.bc_type[5] = abi.BC_SLAB
    for w, n in ((3, 3), (1, 7)):
        with _handle(cfg, _limit(cfg, w), monkeypatch) as g:
            sc = driver.SimControl(g, cfg)
            sc.init(P)
            dt = sc.calculate_timestep()
            g.stage_part(0.5 * dt, abi.OA1, 0, abi.STAGE_INTERIOR)
            assert g.rows_windows()["launches_last_part"] == n
            g.stage_part(0.5 * dt, abi.OA1, 0, abi.STAGE_SLABBOUNDARY)
            assert g.rows_windows()["launches_last_part"] == 2 * min(2, -(-2 // w))


def test_knobs(monkeypatch):
    cfg, _, _, _ = CASES["glm3d"](1)
    L = _limit(cfg, 3)
    # PION_ROWS_WINDOWS=0: the old selection, whatever the limit says
    monkeypatch.setenv("PION_ROWS_WINDOWS", "0")
    with _handle(cfg, L, monkeypatch) as g:
        assert g.rows_windows()["windows_whole_stage"] == 1
    monkeypatch.delenv("PION_ROWS_WINDOWS")
    # one plane with its ghost planes over the limit: the cell-per-thread kernel
    Lsmall = _limit(cfg, 1) - 1
    assert lib.rows_windows(cfg, limit=Lsmall) == []
    with _handle(cfg, Lsmall, monkeypatch) as g:
        assert g.rows_windows()["windows_whole_stage"] == 0
    # PION_STAGE_KERNEL=cell likewise reports no window
    monkeypatch.setenv("PION_STAGE_KERNEL", "cell")
    with _handle(cfg, L, monkeypatch) as g:
        assert g.rows_windows()["windows_whole_stage"] == 0
    monkeypatch.delenv("PION_STAGE_KERNEL")
    # 1-D: no rows kernel
    c1 = abi.make_config(1, [32], abi.EQEUL, abi.FLUX_RSroe, xmin=(0.0, 0, 0), xmax=(1.0, 0, 0), bcs=["outflow"] * 2,
                         refvec=[1.0] * 5)
    with _handle(c1, None, monkeypatch) as g:
        assert g.rows_windows()["windows_whole_stage"] == 0
