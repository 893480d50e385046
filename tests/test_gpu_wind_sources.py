"""GPU tests of the device-built stellar-wind sources (pion_gpu_add_wind_source / pion_gpu_get_wind_cells): membership
and states against the numpy restatement (tests/wind_restate.py), whole runs bit-exact against the oracle fed with
the device's own wind list, the error paths."""
import os

import numpy as np
import pytest

import wind_restate as wr
from cpu_backends import CpuSim, have_oracle
from pion_amd import abi, cooling, driver, lib, problems, slab, wind

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WND = os.path.join(ROOT, "tests", "golden", "eta_car.wnd.txt")
YEAR = 3.1558150e7


def _cfg(geom, eqntype=abi.EQEUL, n=16, cooling_=0, strict=1):
    """small grids of every geometry: 'sph' 1-D spherical, 'cyl' 2-D (z,R), 'cart2' 2-D Cartesian, 'cart3' 3-D"""
    kw = dict(ntracer=1, gamma=5.0 / 3.0, cfl=0.3, min_temp=5.0e3, max_temp=1.0e8, strict_fp=strict,
              cooling=cooling_, refvec=[1.0] * 16)
    if geom == "sph":
        return abi.make_config(1, [n], eqntype, abi.FLUX_RSroe, xmin=(0.0, 0.0, 0.0), xmax=(1.0e17, 0, 0),
                               bcs=["reflecting", "outflow"], coord_sys=3, **kw)
    if geom == "cyl":
        return abi.make_config(2, [n, n // 2], eqntype, abi.FLUX_RS_HLL, xmin=(-1.0e17, 0.0, 0.0),
                               xmax=(1.0e17, 1.0e17, 0), bcs=["outflow", "outflow", "axisymmetric", "outflow"],
                               coord_sys=2, **kw)
    if geom == "cart2":
        return abi.make_config(2, [n, n], eqntype, abi.FLUX_RS_HLL, xmin=(-1.0e17, -1.0e17, 0.0),
                               xmax=(1.0e17, 1.0e17, 0), bcs=["outflow"] * 4, **kw)
    return abi.make_config(3, [n, n, n], eqntype, abi.FLUX_RS_HLL, xmin=(-1.0e17, -1.0e17, -1.0e17),
                           xmax=(1.0e17, 1.0e17, 1.0e17), bcs=["outflow"] * 6, **kw)


def _src(cfg, pos=(0.0, 0.0, 0.0), radius=None, vrot=0.0, Bstar=0.0, **kw):
    return wind.WindSource(pos=pos, radius=radius if radius is not None else 3.3 * cfg.dx, mdot=1.0e-6, vinf=1000.0,
                           vrot=vrot, Tw=2.5e4, Rstar=7.0e11, Bstar=Bstar, tracers=[0.75], **kw)


def _on_grid(cfg, idx):
    nga = abi.ng_all(cfg)
    i = [idx % nga[0], (idx // nga[0]) % nga[1], idx // (nga[0] * nga[1])]
    on = np.ones(idx.size, dtype=bool)
    for a in range(cfg.ndim):
        on &= (i[a] >= cfg.nbc) & (i[a] < cfg.nbc + cfg.ng[a])
    return on


def _ulp_check(cfg, dev, ref):
    """device states within 4 ulp of the restatement (device exp/log); velocity and field components are measured
    against the magnitude of their vector (the rotation / toroidal terms are sums)"""
    assert dev.shape == ref.shape
    tol = np.zeros_like(ref)
    sc = np.abs(ref)
    vmag = np.sqrt((ref[:, 2:5] ** 2).sum(axis=1))
    sc[:, 2:5] = np.maximum(sc[:, 2:5], vmag[:, None])
    if cfg.eqntype != abi.EQEUL:
        bmag = np.sqrt((ref[:, 5:8] ** 2).sum(axis=1))
        sc[:, 5:8] = np.maximum(sc[:, 5:8], bmag[:, None])
    tol = 4.0 * np.spacing(sc)
    bad = ~(np.abs(dev - ref) <= tol)
    assert not bad.any(), (np.argwhere(bad)[:5], dev[bad][:5], ref[bad][:5])


@pytest.mark.parametrize("geom", ["sph", "cyl", "cart2", "cart3"])
def test_membership_matches_restatement(geom):
    cfg = _cfg(geom)
    dx = cfg.dx
    cases = [((0.0, 0.0, 0.0), 3.3 * dx),                    # centred (on a cell vertex)
             ((0.0, 0.0, 0.0), 1.5 * dx)]                    # radius = an exact cell-centre distance (1-D: 1.5 dx)
    if geom != "sph":
        cases.append(((0.0, 0.0, 0.0), np.sqrt(0.5 ** 2 + 1.5 ** 2) * dx))
        cases.append(((0.5 * dx, 0.0, 0.0), 2.5 * dx))       # on a cell face (x), off-centre
    if geom in ("cart2", "cart3"):
        cases.append(((-3.3 * dx, 2.2 * dx, 0.7 * dx), 2.9 * dx))   # off-centre
        cases.append(((cfg.xmin[0], 0.25 * dx, 0.0), 2.0 * dx))     # at the grid edge: ghosts included
    if geom == "cyl":
        cases.append(((-3.3 * dx, 0.0, 0.0), 2.9 * dx))
    with lib.GpuSim(cfg, 0) as g:
        for k, (pos, r) in enumerate(cases):
            sid = g.add_wind_source(_src(cfg, pos=pos, radius=r))
            assert sid == k
            idx, _ = g.get_wind_cells(sid)
            ridx = wr.members(cfg, pos, r)[0]
            assert idx.size > 0 and np.array_equal(idx, ridx), (pos, r, idx, ridx)


# spherical grids are Euler only (MHD in 1-D is EINVAL, tested below)
@pytest.mark.parametrize("geom,eqntype", [(g_, e_) for g_ in ("sph", "cyl", "cart2", "cart3")
                                          for e_ in (abi.EQEUL, abi.EQMHD, abi.EQGLM)
                                          if g_ != "sph" or e_ == abi.EQEUL])
@pytest.mark.parametrize("cool", [0, abi.COOL_WSS09_CIE_LINE_HEAT_COOL])
def test_states_match_restatement(geom, eqntype, cool):
    for vrot in (0.0, 200.0):
        for Bstar in (0.0, 0.1):
            out = {}
            for strict in (1, 0):
                cfg = _cfg(geom, eqntype, cooling_=cool, strict=strict)
                src = _src(cfg, vrot=vrot, Bstar=Bstar, pos=(0.0, 0.0, 0.0) if geom in ("sph", "cyl")
                           else (0.3 * cfg.dx, -0.2 * cfg.dx, 0.1 * cfg.dx))
                P = problems.alloc(cfg)
                P[abi.RO], P[abi.PG] = 1.0e-23, 1.0e-10
                with lib.GpuSim(cfg, 0) as g:
                    g.upload(P)
                    g.add_wind_source(src)
                    g.update_bcs(0.0, 2, 2, assign=1)
                    idx, st = g.get_wind_cells(0)
                    A = g.download(0).reshape(cfg.nvar, -1)
                    B = g.download(1).reshape(cfg.nvar, -1)
                # on-grid wind cells hold the states in P and Ph (ghost cells are refilled by the external
                # boundaries, which run after the internal ones)
                on = _on_grid(cfg, idx)
                assert on.any()
                assert np.array_equal(A[:, idx[on]].T, st[on]) and np.array_equal(B[:, idx[on]].T, st[on])
                out[strict] = st
            rs = wr.Source(src, cfg.ntracer)
            ridx, ref = rs.states(cfg)
            assert np.array_equal(idx, ridx)
            fin = np.isfinite(ref).all(axis=1)          # a cell exactly at a 2-D Cartesian source has dist = 0
            assert np.array_equal(np.isfinite(out[1]).all(axis=1), fin)
            _ulp_check(cfg, out[1][fin], ref[fin])
            # the fast build: within 1e-14 of the strict build (the wind code is compiled without contraction)
            a, b = out[0][fin], out[1][fin]
            assert np.all(np.abs(a - b) <= 1e-14 * np.abs(b))


def _lockstep(cfg, P, srcs, nsteps, t0=0.0, check=None):
    """device (SimControl on GpuSim) and oracle in lock step; before every oracle boundary update the oracle gets
    the device's own wind cells and states (orc_set_wind_cells) -- every update of one step runs at the step's start
    time, so the device's latest states are the ones that update writes; every dt compared with ==; P compared
    bit for bit.  Returns the simulation times of the steps."""
    with lib.GpuSim(cfg, 0) as g, CpuSim(cfg, "orc") as o:
        if cfg.cooling:
            T, tabs, sl = cooling.build_tables(cfg.min_temp, cfg.max_temp)
            g.set_cooling_tables(T, tabs, sl)
            o.set_cooling_tables(T, tabs, sl)
        for s in srcs:
            g.add_wind_source(s)
        rs = [wr.Source(s, cfg.ntracer) for s in srcs]

        class Fed:
            def __getattr__(self, k):
                return getattr(o, k)

            def update_bcs(self, simtime, cstep, maxstep, assign=0):
                idx, st = [], []
                for k, r in enumerate(rs):
                    if r.update(simtime):
                        i, s_ = g.get_wind_cells(k)
                        idx.append(i)
                        st.append(s_)
                        if check is not None:
                            check(simtime, k, r, i, s_)
                if idx:
                    o.set_wind_cells(np.concatenate(idx), np.concatenate(st))
                o.update_bcs(simtime, cstep, maxstep, assign)

        sg = driver.SimControl(g, cfg)
        so = driver.SimControl(Fed(), cfg)
        lim = wind.first_step_dt_limit(cfg, srcs)
        sg.first_step_dt_limit = so.first_step_dt_limit = lim
        sg.init(P, t0)
        so.init(P, t0)
        times = []
        for _ in range(nsteps):
            dg = sg.calculate_timestep()
            do = so.calculate_timestep()
            assert dg == do, (dg, do)
            sg.advance_time()
            so.advance_time()
            assert sg.simtime == so.simtime
            times.append(sg.simtime)
        a, b = g.download(0), o.download(0)
        assert np.array_equal(a, b), np.max(np.abs(a - b) / (np.abs(b) + 1e-300))
        return times


@pytest.mark.skipif(not have_oracle(), reason="liboracle.so not built")
def test_run_3d_constant_wind_matches_oracle():
    cfg, P, srcs = problems.wind3d_rot(32, strict_fp=1, eqntype=abi.EQEUL, vrot=0.0, Bstar=0.0)
    _lockstep(cfg, P, srcs, 6)


@pytest.mark.skipif(not have_oracle(), reason="liboracle.so not built")
def test_run_wind2d_axisymmetric_matches_oracle():
    cfg, P, srcs = problems.wind2d_axi(64, ny=32, strict_fp=1)
    _lockstep(cfg, P, srcs, 6)


@pytest.mark.skipif(not have_oracle(), reason="liboracle.so not built")
def test_run_evolving_etacar_matches_oracle_and_restatement():
    ev = wind.read_wind_evolution(WND)
    t0 = 5.0e10
    # before the 1837 -> 1838 onset the table is constant: a first run learns the step times, then the table is
    # shifted so that the onset starts at step 10 of the 40 compared steps
    cfg, P, srcs = problems.etacar2d_evolving(64, WND, t_now=t0, strict_fp=1)
    with lib.GpuSim(cfg, 0) as g:
        g.add_wind_source(srcs[0])
        sg = driver.SimControl(g, cfg)
        sg.first_step_dt_limit = wind.first_step_dt_limit(cfg, srcs)
        sg.init(P, t0)
        sg.time_int(10)
        t10 = sg.simtime
    off = t10 - ev.time[1]
    cfg, P, srcs = problems.etacar2d_evolving(64, WND, time_offset=off, t_now=t0, strict_fp=1)
    mdot = []

    def check(t, k, r, idx, st):
        ridx, ref = r.states(cfg)
        assert np.array_equal(idx, ridx)
        _ulp_check(cfg, st, ref)
        mdot.append(r.W["Mdot"])

    times = _lockstep(cfg, P, srcs, 40, t0=t0, check=check)
    et = srcs[0].evolution.time
    assert times[8] < et[1] and times[-1] > et[2], (times, et)   # the onset lies inside the run
    assert mdot[0] == ev.Mdot[1] and max(mdot) == ev.Mdot[2]


def test_evolving_inactive_then_clamped_after_tfinish():
    ev = wind.read_wind_evolution(WND)
    cfg = _cfg("cyl")
    t_end = ev.time[-1]
    src = wind.WindSource(pos=(0.0, 0.0), radius=3.3 * cfg.dx, tracers=[1.0], type=wind.EVOLVING, evolution=ev,
                          elements=[None], t_now=-5.0, update_freq=1.0)
    P = problems.alloc(cfg)
    P[abi.RO], P[abi.PG] = 2.0e-22, 1.0e-11
    rs = wr.Source(src, cfg.ntracer)
    with lib.GpuSim(cfg, 0) as g:
        g.upload(P)
        g.add_wind_source(src)
        idx, st = g.get_wind_cells(0)
        assert idx.size > 0
        # inactive (t < tstart = 0): flagged, not written
        g.update_bcs(-3.0, 2, 2, assign=1)
        assert not rs.update(-3.0)
        A = g.download(0).reshape(cfg.nvar, -1)
        assert np.array_equal(A[:, idx], P.reshape(cfg.nvar, -1)[:, idx])
        assert np.array_equal(g.get_wind_cells(0)[1], np.zeros_like(st))
        # active, inside the table, and clamped after tfinish
        for t in (1.0e10, ev.time[2] + 1.0e6, t_end + 1.0e9, t_end + 5.0e10):
            g.update_bcs(t, 2, 2)
            assert rs.update(t)
            _, st = g.get_wind_cells(0)
            _, ref = rs.states(cfg)
            _ulp_check(cfg, st, ref)
        assert rs.W["Vinf"] == ev.vinf[-1] and rs.W["Mdot"] == ev.Mdot[-1]


def test_error_paths_return_einval():
    cases = []
    cyl = _cfg("cyl")
    cases.append((cyl, _src(cyl, pos=(0.0, 0.5 * cyl.dx, 0.0))))          # off the axis
    sph = _cfg("sph")
    cases.append((sph, _src(sph, pos=(0.5 * sph.dx, 0.0, 0.0))))          # off r = 0
    c3 = _cfg("cart3")
    cases.append((c3, _src(c3, type=2)))
    cases.append((c3, _src(c3, type=3)))
    cases.append((c3, _src(c3, radius=0.0)))
    cases.append((c3, _src(c3, radius=-1.0)))
    ev = wind.WindEvolution({k: np.array([1.0]) for k in wind.COLUMNS})
    cases.append((c3, _src(c3, type=wind.EVOLVING, evolution=ev)))        # npt < 2
    for cfg, s in cases:
        with lib.GpuSim(cfg, 0) as g:
            with pytest.raises(lib.PionGpuError) as e:
                g.add_wind_source(s)
            assert e.value.rc == -1
    # MHD in 1-D: a 1-D Cartesian MHD grid (spherical grids are Euler only already at create)
    c1 = abi.make_config(1, [16], abi.EQMHD, abi.FLUX_RS_HLL, xmin=(0.0, 0, 0), xmax=(1.0, 0, 0),
                         bcs=["outflow"] * 2, refvec=[1.0] * 16)
    with lib.GpuSim(c1, 0) as g:
        with pytest.raises(lib.PionGpuError) as e:
            g.add_wind_source(_src(c1, pos=(0.5, 0, 0), radius=0.2))
        assert e.value.rc == -1


def test_cpp_loop_with_wind_source_equals_python_driver():
    """pion_host_sim_add_wind_source + pion_host_sim_time_int against the Python driver with the same source and
    the same first-step limit (calc_timestep.cpp:318-322)"""
    import ctypes as C
    abi.share_torch_hip_runtime()
    host = C.CDLL(os.path.join(ROOT, "pion_amd", "host", "libpion_host.so"))
    dp = C.POINTER(C.c_double)
    host.pion_host_sim_create.argtypes = [C.POINTER(abi.PionGpuConfig), C.c_int, C.POINTER(C.c_void_p)]
    host.pion_host_sim_add_wind_source.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(C.c_int)]
    host.pion_host_sim_init.argtypes = [C.c_void_p, dp, C.c_double, C.c_double, C.c_double]
    host.pion_host_sim_time_int.argtypes = [C.c_void_p, C.c_int, dp, dp]
    host.pion_host_sim_download.argtypes = [C.c_void_p, C.c_int, dp]
    host.pion_host_sim_destroy.argtypes = [C.c_void_p]
    host.pion_host_sim_destroy.restype = None
    cfg, P, srcs = problems.wind3d_rot(24, strict_fp=1)
    T, tabs, sl = cooling.build_tables(cfg.min_temp, cfg.max_temp)
    s = C.c_void_p()
    assert host.pion_host_sim_create(C.byref(cfg), 0, C.byref(s)) == 0
    try:
        host.pion_host_sim_handle.argtypes = [C.c_void_p]
        host.pion_host_sim_handle.restype = C.c_void_p
        hs = lib.GpuSim(cfg, 0, borrowed_handle=host.pion_host_sim_handle(s))
        hs.set_cooling_tables(T, tabs, sl)
        st, keep = srcs[0].to_c()
        sid = C.c_int(-1)
        assert host.pion_host_sim_add_wind_source(s, C.byref(st), C.byref(sid)) == 0 and sid.value == 0
        Pc = np.ascontiguousarray(P).reshape(-1)
        assert host.pion_host_sim_init(s, Pc.ctypes.data_as(dp), 0.0, 1e300, -1.0) == 0
        t, ldt = C.c_double(), C.c_double()
        assert host.pion_host_sim_time_int(s, 5, C.byref(t), C.byref(ldt)) == 5
        out = np.empty_like(Pc)
        assert host.pion_host_sim_download(s, 0, out.ctypes.data_as(dp)) == 0
        hidx, hst = hs.get_wind_cells(0)
    finally:
        host.pion_host_sim_destroy(s)
    with lib.GpuSim(cfg, 0) as g:
        g.set_cooling_tables(T, tabs, sl)
        g.add_wind_source(srcs[0])
        sc = driver.SimControl(g, cfg)
        sc.first_step_dt_limit = wind.first_step_dt_limit(cfg, srcs)
        sc.init(P)
        sc.time_int(5)
        assert sc.simtime == t.value and sc.last_dt == ldt.value
        assert np.array_equal(g.download(0).reshape(-1), out)
        gidx, gst = g.get_wind_cells(0)
        assert np.array_equal(gidx, hidx) and np.array_equal(gst, hst)


def test_two_z_slabs_hold_the_single_grids_wind_cells():
    """two z-slab handles of a 3-D grid: their on-grid wind cells and states are those of the single grid"""
    cfg, P, srcs = problems.wind3d_rot(16, strict_fp=1)
    src = srcs[0]
    src.pos = (0.3 * cfg.dx, -0.2 * cfg.dx, 0.6 * cfg.dx)

    def on_grid_cells(c, idx, st):
        n = abi.ng_all(c)
        i = [idx % n[0] - c.nbc, (idx // n[0]) % n[1] - c.nbc, idx // (n[0] * n[1]) - c.nbc]
        on = _on_grid(c, idx)
        z = c.xmin[2] + (2 * i[2][on] + 1) * (0.5 * c.dx)
        return {(int(i[0][k]), int(i[1][k]), float(zz)): tuple(st[on][j]) for j, (k, zz) in
                enumerate(zip(np.flatnonzero(on), z))}

    with lib.GpuSim(cfg, 0) as g:
        g.upload(P)
        g.add_wind_source(src)
        g.update_bcs(0.0, 2, 2, assign=1)
        whole = on_grid_cells(cfg, *g.get_wind_cells(0))
    parts = {}
    for r in range(2):
        c = slab.slab_config(cfg, r, 2)      # the slab's xmin: global xmin + rank * nz_local * dx
        Ps = problems.alloc(c)
        Ps[abi.RO], Ps[abi.PG] = 2.124229813e-20, 2.209037632e-08
        with lib.GpuSim(c, 0) as g:
            g.upload(Ps)
            g.add_wind_source(src)
            g.update_bcs(0.0, 2, 2, assign=1)
            parts.update(on_grid_cells(c, *g.get_wind_cells(0)))
    assert len(whole) > 0 and parts == whole
