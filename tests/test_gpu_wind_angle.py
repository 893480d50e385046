"""GPU tests of the rotating-star (LGM99) wind sources (pion_gpu_add_rotating_wind_source): membership and states
against the restatement (tests/wind_angle_restate.py), the evolution and activity rules, the error paths, whole runs
bit-exact against the oracle fed with the device's own wind list, the fast build, the C++ loop and z-slabs."""
import ctypes as C
import os

import numpy as np
import pytest

import wind_angle_restate as ar
import wind_restate as wr
from cpu_backends import CpuSim, have_oracle
from pion_amd import abi, cooling, driver, lib, problems, slab, wind

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WND = os.path.join(ROOT, "tests", "golden", "eta_car.wnd.txt")
MSUN_YR = 1.9891e33 / 3.1558150e7
# States against the restatement: the device's atan, sin, exp and log are the only difference.  Each component is
# measured in ulp of the largest of |value|, |v| (velocities), |B| (fields); the bound holds with margin.
ULP = 64


def _cfg(geom, eqntype=abi.EQEUL, n=16, cooling_=0, strict=1):
    """'cyl' 2-D (z,R), 'cart2' 2-D Cartesian, 'cart3' 3-D, 'sph' 1-D spherical"""
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


def _table(t=(-1.0e12, 1.0e12), Teff=(2.5e4, 3.0e4), mdot=(1.0e-6, 1.2e-6), vrot=(1.5e7, 1.8e7), vcrit=(3.0e7, 3.0e7),
           vinf=(1.0e8, 0.9e8), R=(7.0e11, 7.0e11)):
    cols = {c: np.zeros(len(t)) for c in wind.COLUMNS}
    cols.update(time=np.array(t, float), Teff=np.array(Teff, float), Mdot=np.array(mdot, float) * MSUN_YR,
                vrot=np.array(vrot, float), vcrit=np.array(vcrit, float), vinf=np.array(vinf, float),
                R=np.array(R, float), X_H=np.full(len(t), 0.7))
    return wind.WindEvolution(cols)


def _pos(cfg):
    """on the axis (cylindrical), else off every plane of cell centres"""
    if cfg.coord_sys == 2:
        return (0.0, 0.0, 0.0)
    return (0.3 * cfg.dx, -0.2 * cfg.dx, 0.1 * cfg.dx)


def _rsrc(cfg, pos=None, radius=None, ev=None, xi=-0.43, Bstar=0.0, t_now=0.0, elements=("X_H",), **kw):
    return wind.WindSource(pos=_pos(cfg) if pos is None else pos, radius=3.3 * cfg.dx if radius is None else radius,
                           vinf=1000.0, Bstar=Bstar, tracers=[0.5], type=wind.ANGLE,
                           evolution=_table() if ev is None else ev, elements=list(elements), t_now=t_now,
                           update_freq=1.0, xi=xi, **kw)


def _ulp_check(cfg, dev, ref, bound=ULP):
    assert dev.shape == ref.shape and dev.shape[0] > 0
    sc = np.abs(ref)
    vmag = np.sqrt((ref[:, 2:5] ** 2).sum(axis=1))
    sc[:, 2:5] = np.maximum(sc[:, 2:5], vmag[:, None])
    if cfg.eqntype != abi.EQEUL:
        bmag = np.sqrt((ref[:, 5:8] ** 2).sum(axis=1))
        sc[:, 5:8] = np.maximum(sc[:, 5:8], bmag[:, None])
    ulps = np.abs(dev - ref) / np.spacing(np.where(sc > 0, sc, 1e-300))
    assert np.isfinite(dev).all()
    assert ulps.max() <= bound, (ulps.max(), np.unravel_index(np.argmax(ulps), ulps.shape))
    return ulps.max()


def _on_grid(cfg, idx):
    nga = abi.ng_all(cfg)
    i = [idx % nga[0], (idx // nga[0]) % nga[1], idx // (nga[0] * nga[1])]
    on = np.ones(idx.size, dtype=bool)
    for a in range(cfg.ndim):
        on &= (i[a] >= cfg.nbc) & (i[a] < cfg.nbc + cfg.ng[a])
    return on


@pytest.mark.parametrize("geom", ["cyl", "cart2", "cart3"])
def test_membership_and_flags_equal_a_constant_source(geom):
    cfg = _cfg(geom)
    r = _rsrc(cfg)
    c = wind.WindSource(pos=r.pos, radius=r.radius, mdot=1e-6, vinf=1000.0, Tw=2.5e4, Rstar=7e11, tracers=[0.5])
    with lib.GpuSim(cfg, 0) as g0, lib.GpuSim(cfg, 0) as g2:
        assert g0.add_wind_source(c) == 0
        assert g2.add_rotating_wind_source(r) == 0
        i0, _ = g0.get_wind_cells(0)
        i2, s2 = g2.get_wind_cells(0)
        assert i2.size > 0 and np.array_equal(i0, i2)
        assert np.array_equal(i2, ar.Source(r, cfg.ntracer).cells(cfg)[0])
        assert np.array_equal(g0.get_flags(), g2.get_flags())
        assert not s2.any()                                  # nothing written before the first update
        # a constant source beside the rotating one keeps its own state path
        assert g2.add_wind_source(c) == 1


@pytest.mark.parametrize("geom,eqntype", [(g_, e_) for g_ in ("cyl", "cart2", "cart3")
                                          for e_ in (abi.EQEUL, abi.EQMHD, abi.EQGLM)])
@pytest.mark.parametrize("cool", [0, abi.COOL_WSS09_CIE_LINE_HEAT_COOL])
def test_states_match_restatement(geom, eqntype, cool):
    out = {}
    for strict in (1, 0):
        cfg = _cfg(geom, eqntype, cooling_=cool, strict=strict)
        src = _rsrc(cfg, Bstar=0.1 if eqntype != abi.EQEUL else 0.0)
        P = problems.alloc(cfg)
        P[abi.RO], P[abi.PG] = 1.0e-23, 1.0e-10
        with lib.GpuSim(cfg, 0) as g:
            g.upload(P)
            g.add_rotating_wind_source(src)
            g.update_bcs(3.0e11, 2, 2, assign=1)
            idx, st = g.get_wind_cells(0)
            A = g.download(0).reshape(cfg.nvar, -1)
            B = g.download(1).reshape(cfg.nvar, -1)
        on = _on_grid(cfg, idx)
        assert on.any()
        assert np.array_equal(A[:, idx[on]].T, st[on]) and np.array_equal(B[:, idx[on]].T, st[on])
        out[strict] = st
    rs = ar.Source(src, cfg.ntracer)
    assert rs.update(3.0e11)
    ridx, ref = rs.states(cfg)
    assert np.array_equal(idx, ridx)
    inner = wr.members(cfg, src.pos, src.radius)[1] < 0.75 * src.radius
    assert inner.any() and (~inner).any()           # both the 1e-31 core and the LGM99 density
    _ulp_check(cfg, out[1], ref)
    # both builds compile the wind code without contraction: the same bits
    assert np.array_equal(out[0], out[1])
    # the latitude dependence is there: the density at equal distance differs between pole and equator
    assert rs.W["v_rot"] / rs.W["vcrit"] > 0.4


def test_evolution_inactive_onset_and_clamps():
    ev = wind.read_wind_evolution(WND, time_offset=1.0e9)      # tstart = 1e9 s
    cfg = _cfg("cyl")
    src = _rsrc(cfg, ev=ev, elements=[None], t_now=0.0)
    P = problems.alloc(cfg)
    P[abi.RO], P[abi.PG] = 2.0e-22, 1.0e-11
    rs = ar.Source(src, cfg.ntracer)
    assert not rs.active
    with lib.GpuSim(cfg, 0) as g:
        g.upload(P)
        g.add_rotating_wind_source(src)
        idx, st = g.get_wind_cells(0)
        # inactive before tstart: flagged, not written
        g.update_bcs(5.0e8, 2, 2, assign=1)
        assert not rs.update(5.0e8)
        A = g.download(0).reshape(cfg.nvar, -1)
        assert np.array_equal(A[:, idx], P.reshape(cfg.nvar, -1)[:, idx])
        assert not g.get_wind_cells(0)[1].any()
        # active before, across and after the 1837 -> 1838 onset, then clamped after tfinish
        t = ev.time
        seen = []
        for tt in (2.0e9, t[1], 0.5 * (t[1] + t[2]), t[2] + 1.0e6, t[-1] + 1.0e9, t[-1] + 5.0e10):
            g.update_bcs(tt, 2, 2)
            assert rs.update(tt)
            _, st = g.get_wind_cells(0)
            _, ref = rs.states(cfg)
            _ulp_check(cfg, st, ref)
            seen.append(rs.W["Mdot"])
        assert seen[0] == ev.Mdot[0] and ev.Mdot[1] < seen[2] < ev.Mdot[2]
        assert rs.W["Vinf"] == ev.vinf[-1] and rs.W["Mdot"] == ev.Mdot[-1]
    # Tw is clamped at Teff_vec.back() = 150 000 K
    cfg = _cfg("cart3")
    src = _rsrc(cfg, ev=_table(Teff=(2.0e5, 2.0e5)))
    rs = ar.Source(src, cfg.ntracer)
    assert rs.W["Tw"] == 150000.0 and rs.update(1.0e11) and rs.W["Tw"] == 150000.0
    with lib.GpuSim(cfg, 0) as g:
        g.upload(problems.alloc(cfg) + 1.0e-20)
        g.add_rotating_wind_source(src)
        g.update_bcs(1.0e11, 2, 2, assign=1)
        _, ref = rs.states(cfg)
        _ulp_check(cfg, g.get_wind_cells(0)[1], ref)


def _einval(g, src, rotating=True):
    with pytest.raises(lib.PionGpuError) as e:
        g.add_rotating_wind_source(src) if rotating else g.add_wind_source(src)
    assert e.value.rc == -1


def test_error_paths_return_einval():
    c3, cyl, c2 = _cfg("cart3"), _cfg("cyl"), _cfg("cart2")
    for cfg in (_cfg("sph"), abi.make_config(1, [16], abi.EQEUL, abi.FLUX_RS_HLL, xmin=(0.0, 0, 0),
                                             xmax=(1.0, 0, 0), bcs=["outflow"] * 2, refvec=[1.0] * 16)):
        with lib.GpuSim(cfg, 0) as g:
            _einval(g, _rsrc(cfg, pos=(0.0, 0, 0), radius=3.3 * cfg.dx))       # 1-D: theta = 0
    with lib.GpuSim(cyl, 0) as g:
        _einval(g, _rsrc(cyl, pos=(0.0, 0.5 * cyl.dx, 0.0)))                    # off the axis
    with lib.GpuSim(c3, 0) as g:
        _einval(g, _rsrc(c3, orbit=(1.2, 1.0e15, 1.0e14, 1.0)))                  # orbit
        _einval(g, _rsrc(c3, radius=0.0))
        _einval(g, _rsrc(c3, radius=-1.0))
        _einval(g, _rsrc(c3, ev=_table(t=(0.0,), Teff=(2.5e4,), mdot=(1e-6,), vrot=(1e7,), vcrit=(3e7,),
                                       vinf=(1e8,), R=(7e11,))))                  # npt < 2
        s = _rsrc(c3)
        s.type = wind.EVOLVING
        _einval(g, s)                                                            # type != 2
        s = _rsrc(c3)
        s.type = wind.ANGLE
        _einval(g, s, rotating=False)                                            # add_wind_source(type 2)
        st, keep = s.to_c()
        i = C.c_int(-1)
        assert g.lib.pion_gpu_add_rotating_wind_source(g.h, C.byref(st), None, -0.43, C.byref(i)) == -1  # no vcrit
        # a cell-centre plane through the source: theta = 90 deg
        _einval(g, _rsrc(c3, pos=(0.3 * c3.dx, -0.2 * c3.dx, 0.5 * c3.dx)))
        assert g.add_rotating_wind_source(_rsrc(c3)) == 0                        # nothing of the failures stayed
        _einval(g, _rsrc(c3, xi=0.0))                                            # another xi
        ev1 = wind.WindSource(pos=(0, 0, 0), radius=3.3 * c3.dx, tracers=[1.0], type=wind.EVOLVING,
                              evolution=_table(), elements=[None], update_freq=1.0)
        _einval(g, ev1, rotating=False)                                          # type 1 after type 2
        assert g.add_rotating_wind_source(_rsrc(c3, pos=(-3.3 * c3.dx, 2.2 * c3.dx, 0.7 * c3.dx))) == 1
    with lib.GpuSim(c2, 0) as g:
        _einval(g, _rsrc(c2, pos=(0.5 * c2.dx, 0.3 * c2.dx, 0.0)))               # x = a cell centre: 90 deg
        _einval(g, _rsrc(c2, pos=(0.3 * c2.dx, 0.5 * c2.dx, 0.0)))               # y = a cell centre: 0 deg
        g.add_wind_source(wind.WindSource(pos=(0, 0), radius=3.3 * c2.dx, tracers=[1.0], type=wind.EVOLVING,
                                          evolution=_table(), elements=[None], update_freq=1.0))
        _einval(g, _rsrc(c2))                                                    # type 2 after type 1


@pytest.mark.parametrize("bad", ["omega", "Tw"])
def test_update_error_writes_nothing(bad):
    cfg = _cfg("cart3")
    kw = dict(vrot=(0.0, 0.0)) if bad == "omega" else dict(Teff=(900.0, 900.0))
    src = _rsrc(cfg, ev=_table(**kw))
    P = problems.alloc(cfg)
    P[abi.RO], P[abi.PG] = 1.0e-23, 1.0e-10
    with lib.GpuSim(cfg, 0) as g:
        g.upload(P)
        assert g.add_rotating_wind_source(src) == 0
        with pytest.raises(lib.PionGpuError) as e:
            g.update_bcs(1.0e11, 2, 2, assign=1)
        assert e.value.rc == -1
        assert np.array_equal(g.download(0).reshape(-1), P.reshape(-1))
        assert np.array_equal(g.download(1).reshape(-1), P.reshape(-1))
        assert not g.get_wind_cells(0)[1].any()
    # the Python driver surfaces it
    with lib.GpuSim(cfg, 0) as g:
        sc = driver.SimControl(g, cfg)
        sc.add_wind_source(src)
        with pytest.raises(lib.PionGpuError):
            sc.init(P)


def _lockstep(cfg, P, srcs, nsteps, t0=0.0, check=None, strict=True):
    """device (SimControl on GpuSim) and oracle in lock step, the oracle fed the device's wind cells and states
    before every boundary update; strict: every dt ==, P bit for bit; fast: the step of the device, P within 1e-10
    of each variable's largest value.  Returns the simulation times of the steps."""
    with lib.GpuSim(cfg, 0) as g, CpuSim(cfg, "orc") as o:
        if cfg.cooling:
            T, tabs, sl = cooling.build_tables(cfg.min_temp, cfg.max_temp)
            g.set_cooling_tables(T, tabs, sl)
            o.set_cooling_tables(T, tabs, sl)
        sg = driver.SimControl(g, cfg)
        for s in srcs:
            sg.add_wind_source(s)
        rs = [ar.Source(s, cfg.ntracer) for s in srcs]

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

        so = driver.SimControl(Fed(), cfg)
        so.first_step_dt_limit = sg.first_step_dt_limit
        sg.init(P, t0)
        so.init(P, t0)
        times = []
        for _ in range(nsteps):
            dg = sg.calculate_timestep()
            do = so.calculate_timestep()
            if strict:
                assert dg == do, (dg, do)
            else:
                assert abs(dg - do) <= 1e-11 * do
                so.dt = sg.dt
            sg.advance_time()
            so.advance_time()
            times.append(sg.simtime)
        a, b = g.download(0), o.download(0)
        if strict:
            assert np.array_equal(a, b), np.max(np.abs(a - b) / (np.abs(b) + 1e-300))
        else:
            scale = np.abs(b).reshape(cfg.nvar, -1).max(axis=1).reshape(-1, 1, 1, 1) + 1e-300
            assert np.max(np.abs(a - b) / scale) <= 1e-10, np.max(np.abs(a - b) / scale)
        return times


def _etacar_offset(t0):
    """time_offset that puts the 1837 -> 1838 onset at step 10 of etacar2d_lgm99(64)"""
    ev = wind.read_wind_evolution(WND)
    cfg, P, srcs = problems.etacar2d_lgm99(64, WND, t_now=t0, strict_fp=1)
    with lib.GpuSim(cfg, 0) as g:
        sg = driver.SimControl(g, cfg)
        sg.add_wind_source(srcs[0])
        sg.init(P, t0)
        sg.time_int(10)
        return sg.simtime - ev.time[1]


@pytest.mark.skipif(not have_oracle(), reason="liboracle.so not built")
def test_run_etacar_lgm99_matches_oracle_and_fast_build():
    t0 = 5.0e10
    off = _etacar_offset(t0)
    ev = wind.read_wind_evolution(WND)
    mdot = []

    def check(t, k, r, idx, st):
        ridx, ref = r.states(cfg)
        assert np.array_equal(idx, ridx)
        _ulp_check(cfg, st, ref)
        mdot.append(r.W["Mdot"])

    cfg, P, srcs = problems.etacar2d_lgm99(64, WND, time_offset=off, t_now=t0, strict_fp=1)
    times = _lockstep(cfg, P, srcs, 40, t0=t0, check=check)
    et = srcs[0].evolution.time
    assert times[8] < et[1] and times[-1] > et[2], (times, et)
    assert mdot[0] == ev.Mdot[1] and max(mdot) == ev.Mdot[2]
    cfg, P, srcs = problems.etacar2d_lgm99(64, WND, time_offset=off, t_now=t0, strict_fp=0)
    _lockstep(cfg, P, srcs, 40, t0=t0, strict=False)


@pytest.mark.skipif(not have_oracle(), reason="liboracle.so not built")
def test_run_rotstar3d_lgm99_glm_matches_oracle_and_fast_build():
    cfg, P, srcs = problems.rotstar3d_lgm99(32, strict_fp=1)
    _lockstep(cfg, P, srcs, 6)
    cfg, P, srcs = problems.rotstar3d_lgm99(32, strict_fp=0)
    _lockstep(cfg, P, srcs, 6, strict=False)


def test_cpp_loop_equals_python_driver():
    abi.share_torch_hip_runtime()
    host = C.CDLL(os.path.join(ROOT, "pion_amd", "host", "libpion_host.so"))
    dp = C.POINTER(C.c_double)
    host.pion_host_sim_create.argtypes = [C.POINTER(abi.PionGpuConfig), C.c_int, C.POINTER(C.c_void_p)]
    host.pion_host_sim_add_rotating_wind_source.argtypes = [C.c_void_p, C.c_void_p, dp, C.c_double,
                                                            C.POINTER(C.c_int)]
    host.pion_host_sim_init.argtypes = [C.c_void_p, dp, C.c_double, C.c_double, C.c_double]
    host.pion_host_sim_time_int.argtypes = [C.c_void_p, C.c_int, dp, dp]
    host.pion_host_sim_download.argtypes = [C.c_void_p, C.c_int, dp]
    host.pion_host_sim_destroy.argtypes = [C.c_void_p]
    host.pion_host_sim_destroy.restype = None
    host.pion_host_sim_handle.argtypes = [C.c_void_p]
    host.pion_host_sim_handle.restype = C.c_void_p
    t0 = 5.0e10
    cfg, P, srcs = problems.etacar2d_lgm99(64, WND, t_now=t0, strict_fp=1)
    s = C.c_void_p()
    assert host.pion_host_sim_create(C.byref(cfg), 0, C.byref(s)) == 0
    try:
        hs = lib.GpuSim(cfg, 0, borrowed_handle=host.pion_host_sim_handle(s))
        st, keep = srcs[0].to_c()
        sid = C.c_int(-1)
        assert host.pion_host_sim_add_rotating_wind_source(s, C.byref(st), keep[-1].ctypes.data_as(dp),
                                                           srcs[0].xi, C.byref(sid)) == 0 and sid.value == 0
        Pc = np.ascontiguousarray(P).reshape(-1)
        assert host.pion_host_sim_init(s, Pc.ctypes.data_as(dp), t0, 1e300, -1.0) == 0
        t, ldt = C.c_double(), C.c_double()
        assert host.pion_host_sim_time_int(s, 5, C.byref(t), C.byref(ldt)) == 5
        out = np.empty_like(Pc)
        assert host.pion_host_sim_download(s, 0, out.ctypes.data_as(dp)) == 0
        hidx, hst = hs.get_wind_cells(0)
    finally:
        host.pion_host_sim_destroy(s)
    with lib.GpuSim(cfg, 0) as g:
        sc = driver.SimControl(g, cfg)
        sc.add_wind_source(srcs[0])
        sc.init(P, t0)
        sc.time_int(5)
        assert sc.simtime == t.value and sc.last_dt == ldt.value
        assert np.array_equal(g.download(0).reshape(-1), out)
        gidx, gst = g.get_wind_cells(0)
        assert np.array_equal(gidx, hidx) and np.array_equal(gst, hst) and gst.any()


def test_two_z_slabs_hold_the_single_grids_rotating_wind_cells():
    cfg, P, srcs = problems.rotstar3d_lgm99(16, strict_fp=1)
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
        g.add_rotating_wind_source(src)
        g.update_bcs(0.0, 2, 2, assign=1)
        whole = on_grid_cells(cfg, *g.get_wind_cells(0))
    parts = {}
    for r in range(2):
        c = slab.slab_config(cfg, r, 2)
        Ps = problems.alloc(c)
        Ps[abi.RO], Ps[abi.PG] = 2.124229813e-20, 2.209037632e-08
        with lib.GpuSim(c, 0) as g:
            g.upload(Ps)
            g.add_rotating_wind_source(src)
            g.update_bcs(0.0, 2, 2, assign=1)
            parts.update(on_grid_cells(c, *g.get_wind_cells(0)))
    assert len(whole) > 0 and parts == whole
