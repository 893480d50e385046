"""GPU tests of wind sources on an orbit (pion_gpu_wind_source.orbit_*): after every boundary update the member
lists, the whole flag array and the states equal the restatement (tests/orbit_restate.py); whole strict runs of the
colliding-wind binaries are bit-exact against the oracle; z-slabs, the C++ loop, the NaN orbit, the error paths."""
import ctypes as C
import os

import numpy as np
import pytest

import orbit_restate as orr
import wind_restate as wr
from cpu_backends import CpuSim, have_oracle
from pion_amd import abi, driver, lib, problems, slab, wind
from test_gpu_wind_sources import _cfg, _on_grid, _src, _ulp_check

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
YEAR = orr.YEAR


def _orbit_cases(cfg):
    """(name, [WindSource]) on the grids of _cfg: the orbits sweep about two cells per update in the tests below"""
    dx = cfg.dx
    P = 1.0 / YEAR          # period 1 s: the tests step simtime through the orbit directly
    cases = [
        # two moving sources whose spheres overlap
        ("overlap2", [_src(cfg, pos=(-1.3 * dx, 0.4 * dx, 0.2 * dx), radius=3.1 * dx, orbit=(1.1, 2.0 * dx, 1.5 * dx, P)),
                      _src(cfg, pos=(1.2 * dx, -0.3 * dx, -0.1 * dx), radius=2.7 * dx,
                           orbit=(1.4, -1.0 * dx, 2.5 * dx, P))]),
        # a static source first, a moving one over it, a static one after
        ("static", [_src(cfg, pos=(0.3 * dx, 0.2 * dx, 0.0), radius=2.5 * dx),
                    _src(cfg, pos=(-2.0 * dx, 0.1 * dx, 0.3 * dx), radius=2.9 * dx, orbit=(1.2, 2.2 * dx, -0.7 * dx, P)),
                    _src(cfg, pos=(-3.5 * dx, -3.4 * dx, 0.5 * dx), radius=1.9 * dx)]),
        # an orbit that runs through the ghost layers of the grid's corner
        ("ghosts", [_src(cfg, pos=(cfg.xmin[0] + 2.0 * dx, cfg.xmin[1] + 1.6 * dx, 0.4 * dx), radius=2.6 * dx,
                         orbit=(1.3, 1.9 * dx, 1.2 * dx, P))]),
    ]
    return cases


def _check_update(g, cfg, rs, orb, t):
    """device against the restatement after the update at t"""
    assert np.array_equal(g.get_flags(), orb.flags)
    for k, s in enumerate(orb.srcs):
        pos = g.get_wind_source_pos(k)
        assert pos == tuple(orb.pos[k]) or (np.isnan(pos[0]) and np.isnan(orb.pos[k][0])), (k, pos, orb.pos[k])
        idx, st = g.get_wind_cells(k)
        ridx = orb.idx[k]
        assert np.array_equal(idx, ridx), (t, k, idx.size, ridx.size)
        assert rs[k].update(t)
        _, ref = orb.states(k, rs[k].W, rs[k].tr)
        fin = np.isfinite(ref).all(axis=1)
        _ulp_check(cfg, st[fin], ref[fin])


@pytest.mark.parametrize("geom", ["cart2", "cart3"])
@pytest.mark.parametrize("strict", [1, 0])
def test_moves_match_restatement(geom, strict):
    cfg = _cfg(geom, strict=strict)
    for name, srcs in _orbit_cases(cfg):
        P = problems.alloc(cfg)
        P[abi.RO], P[abi.PG] = 1.0e-23, 1.0e-10
        orb = orr.Orbits(cfg, srcs)
        rs = [wr.Source(s, cfg.ntracer) for s in srcs]
        changes = 0
        with lib.GpuSim(cfg, 0) as g:
            g.upload(P)
            for k, s in enumerate(srcs):
                assert g.add_wind_source(s) == k
            # set-up: the cells at the set-up position, as for a fixed source
            assert np.array_equal(g.get_flags(), orb.flags), name
            for k in range(len(srcs)):
                assert np.array_equal(g.get_wind_cells(k)[0], orb.idx[k])
            last = [i.copy() for i in orb.idx]
            for step, t in enumerate(np.linspace(0.0, 0.37, 12)):
                # every update of a step runs at its start time: two updates at each t
                for rep in range(2):
                    g.update_bcs(float(t), 2, 2, assign=1 if step == 0 and rep == 0 else 0)
                    orb.update(float(t))
                    _check_update(g, cfg, rs, orb, float(t))
                changes += sum(not np.array_equal(a, b) for a, b in zip(last, orb.idx))
                last = [i.copy() for i in orb.idx]
            # on-grid cells of the sources hold their states in P and Ph (the later source's where they overlap)
            A = g.download(0).reshape(cfg.nvar, -1)
            for k in range(len(srcs)):
                idx, st = g.get_wind_cells(k)
                later = np.zeros(idx.size, dtype=bool)
                for j in range(k + 1, len(srcs)):
                    later |= np.isin(idx, orb.idx[j])
                on = _on_grid(cfg, idx) & ~later
                assert np.array_equal(A[:, idx[on]].T, st[on]), (name, k)
        assert changes >= 8, (name, changes)
        if name == "static":
            # the moving source's first move left static cells unflagged (the reference's overlap quirk)
            lost = np.flatnonzero((orb.flags[orb.idx[0]] & orr.ISBD) == 0)
            assert lost.size > 0


def test_nan_orbit_loses_its_cells():
    cfg = _cfg("cart3")
    dx = cfg.dx
    srcs = [_src(cfg, pos=(0.6 * dx, 0.1 * dx, -0.2 * dx), radius=2.4 * dx, orbit=(1.5, 0.0, 2.0 * dx, 1.0)),
            _src(cfg, pos=(-2.0 * dx, 1.0 * dx, 0.0), radius=2.0 * dx, orbit=(1.5, 2.0 * dx, 0.0, 1.0))]
    P = problems.alloc(cfg)
    P[abi.RO], P[abi.PG] = 1.0e-23, 1.0e-10
    orb = orr.Orbits(cfg, srcs)
    with lib.GpuSim(cfg, 0) as g:
        g.upload(P)
        for s in srcs:
            g.add_wind_source(s)
        before = [g.get_wind_cells(k)[0] for k in range(2)]
        assert all(b.size > 0 for b in before)
        for t in (0.0, 1.0e5, 2.0e5):
            g.update_bcs(t, 2, 2, assign=int(t == 0.0))
            orb.update(t)
            for k in range(2):
                assert np.isnan(g.get_wind_source_pos(k)[0])
                assert g.get_wind_cells(k)[0].size == 0
            fl = g.get_flags()
            assert np.array_equal(fl, orb.flags)
            for b in before:
                assert not (fl[b] & orr.ISBD).any() and (fl[b] & orr.ISDOMAIN).all()
        # nothing written: the cells keep the uploaded state
        A = g.download(0).reshape(cfg.nvar, -1)
        on = np.concatenate([b[_on_grid(cfg, b)] for b in before])
        assert np.array_equal(A[:, on], P.reshape(cfg.nvar, -1)[:, on])


def test_orbit_error_paths_return_einval():
    orbit = (1.2, 1.0e15, 1.0e15, 1.0)
    for geom in ("sph", "cyl"):
        cfg = _cfg(geom)
        with lib.GpuSim(cfg, 0) as g:
            with pytest.raises(lib.PionGpuError) as e:
                g.add_wind_source(_src(cfg, orbit=orbit))
            assert e.value.rc == -1
            g.add_wind_source(_src(cfg))          # the same source without the orbit is fine
    c1 = abi.make_config(1, [16], abi.EQEUL, abi.FLUX_RS_HLL, xmin=(0.0, 0, 0), xmax=(1.0, 0, 0),
                         bcs=["outflow"] * 2, refvec=[1.0] * 16)
    with lib.GpuSim(c1, 0) as g:
        with pytest.raises(lib.PionGpuError) as e:
            g.add_wind_source(_src(c1, pos=(0.5, 0, 0), radius=0.2, orbit=orbit))
        assert e.value.rc == -1
        with pytest.raises(lib.PionGpuError):
            g.get_wind_source_pos(0)


def _orc_flags(o):
    out = np.zeros(o.ncell, dtype=np.uint8)
    f = o.lib.orc_get_flags
    f.restype = C.c_int
    assert f(o.h, out.ctypes.data_as(C.c_void_p)) == 0
    return out


def _lockstep_orbit(cfg, P, srcs, nsteps):
    """device and oracle in lock step, every dt compared with ==, P bit for bit at the end.  The oracle can only add
    wind flags, so at every update whose member lists differ from the last ones a fresh oracle handle takes over:
    P and Ph uploaded, the last GLM speeds replayed, the device's lists and states through orc_set_wind_cells, its
    flags then compared with the device's.  Returns the number of such changes."""
    assert not cfg.cooling
    with lib.GpuSim(cfg, 0) as g:
        for s in srcs:
            g.add_wind_source(s)
        orb = orr.Orbits(cfg, srcs)

        class Fed:
            def __init__(self):
                self.o = CpuSim(cfg, "orc")
                self.glm = None
                self.last = None
                self.changes = 0

            def __getattr__(self, k):
                return getattr(self.o, k)

            def set_glm_speeds(self, *a):
                self.glm = a
                return self.o.set_glm_speeds(*a)

            def update_bcs(self, simtime, cstep, maxstep, assign=0):
                cells = [g.get_wind_cells(k) for k in range(len(srcs))]
                idx = np.concatenate([c[0] for c in cells])
                st = np.concatenate([c[1] for c in cells])
                if self.last is not None and not np.array_equal(idx, self.last):
                    n = CpuSim(cfg, "orc")
                    n.upload(self.o.download(0))
                    n.upload_which(1, self.o.download(1))
                    if self.glm is not None:
                        n.set_glm_speeds(*self.glm)
                    self.o.close()
                    self.o = n
                    self.changes += 1
                self.last = idx
                self.o.set_wind_cells(idx, st)
                self.o.update_bcs(simtime, cstep, maxstep, assign)
                assert np.array_equal(_orc_flags(self.o), g.get_flags())

            def close(self):
                self.o.close()

        fed = Fed()
        try:
            sg = driver.SimControl(g, cfg)
            so = driver.SimControl(fed, cfg)
            sg.first_step_dt_limit = so.first_step_dt_limit = wind.first_step_dt_limit(cfg, srcs)
            sg.init(P)
            orb.update(sg.simtime)
            so.init(P)
            for _ in range(nsteps):
                dg = sg.calculate_timestep()
                do = so.calculate_timestep()
                assert dg == do, (dg, do)
                sg.advance_time()
                orb.update(so.simtime)   # the device's lists now belong to the step's start time
                so.advance_time()
                assert sg.simtime == so.simtime
                for k in range(len(srcs)):
                    assert np.array_equal(g.get_wind_cells(k)[0], orb.idx[k])
            assert np.array_equal(g.get_flags(), orb.flags)
            a, b = g.download(0), fed.o.download(0)
            assert np.array_equal(a, b), np.max(np.abs(a - b) / (np.abs(b) + 1e-300))
            return fed.changes
        finally:
            fed.close()


def _off_ghosts(cfg, srcs, nsteps_time):
    """the spheres stay at least one cell inside the grid over [0, nsteps_time]"""
    for s in srcs:
        for t in np.linspace(0.0, nsteps_time, 64):
            p = orr.orbit_position(s, cfg.ndim, t)
            for a in range(cfg.ndim):
                assert cfg.xmin[a] + s.radius + cfg.dx < p[a] < cfg.xmin[a] + cfg.ng[a] * cfg.dx - s.radius - cfg.dx


@pytest.mark.skipif(not have_oracle(), reason="liboracle.so not built")
def test_run_cwb2d_orbit_matches_oracle():
    cfg, P, srcs = problems.cwb2d_orbit(64, strict_fp=1)
    _off_ghosts(cfg, srcs, 3.0e8)
    changes = _lockstep_orbit(cfg, P, srcs, 60)
    assert changes >= 20, changes


@pytest.mark.skipif(not have_oracle(), reason="liboracle.so not built")
@pytest.mark.parametrize("eqntype", [abi.EQEUL, abi.EQGLM])
def test_run_cwb3d_orbit_matches_oracle(eqntype):
    cfg, P, srcs = problems.cwb3d_orbit(48, strict_fp=1, eqntype=eqntype)
    _off_ghosts(cfg, srcs, 1.0e8)
    changes = _lockstep_orbit(cfg, P, srcs, 40)
    assert changes >= 20, changes


def test_two_z_slabs_hold_the_single_grids_moving_cells():
    cfg, P, srcs = problems.cwb3d_orbit(16, strict_fp=1)
    src = srcs[0]
    src.pos = (0.3 * cfg.dx, -0.2 * cfg.dx, 0.6 * cfg.dx)
    src.orbit = (1.3, 2.0 * cfg.dx, 1.0 * cfg.dx, 1.0 / YEAR)
    times = [0.0, 0.05, 0.1, 0.2, 0.3]

    def on_grid_cells(c, idx, st):
        n = abi.ng_all(c)
        i = [idx % n[0] - c.nbc, (idx // n[0]) % n[1] - c.nbc, idx // (n[0] * n[1]) - c.nbc]
        on = _on_grid(c, idx)
        z = c.xmin[2] + (2 * i[2][on] + 1) * (0.5 * c.dx)
        return {(int(i[0][k]), int(i[1][k]), float(zz)): tuple(st[on][j]) for j, (k, zz) in
                enumerate(zip(np.flatnonzero(on), z))}

    whole = []
    with lib.GpuSim(cfg, 0) as g:
        g.upload(P)
        g.add_wind_source(src)
        for k, t in enumerate(times):
            g.update_bcs(t, 2, 2, assign=int(k == 0))
            whole.append(on_grid_cells(cfg, *g.get_wind_cells(0)))
    parts = [{} for _ in times]
    for r in range(2):
        c = slab.slab_config(cfg, r, 2)
        Ps = problems.alloc(c)
        Ps[abi.RO], Ps[abi.PG] = 2.124229813e-20, 2.209037632e-08
        with lib.GpuSim(c, 0) as g:
            g.upload(Ps)
            g.add_wind_source(src)
            for k, t in enumerate(times):
                g.update_bcs(t, 2, 2, assign=int(k == 0))
                parts[k].update(on_grid_cells(c, *g.get_wind_cells(0)))
    assert all(len(w) > 0 for w in whole)
    assert len(set(tuple(sorted(w)) for w in whole)) > 2      # the members changed
    for w, p in zip(whole, parts):
        assert p == w


def test_cpp_loop_with_moving_source_equals_python_driver():
    """pion_host_sim_add_wind_source passes the orbit through: the C++ loop and the Python driver agree"""
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
    host.pion_host_sim_handle.argtypes = [C.c_void_p]
    host.pion_host_sim_handle.restype = C.c_void_p
    cfg, P, srcs = problems.cwb3d_orbit(48, strict_fp=1)
    s = C.c_void_p()
    assert host.pion_host_sim_create(C.byref(cfg), 0, C.byref(s)) == 0
    try:
        hs = lib.GpuSim(cfg, 0, borrowed_handle=host.pion_host_sim_handle(s))
        keep = []
        for k, src in enumerate(srcs):
            st, kp = src.to_c()
            keep.append((st, kp))
            sid = C.c_int(-1)
            assert host.pion_host_sim_add_wind_source(s, C.byref(st), C.byref(sid)) == 0 and sid.value == k
        Pc = np.ascontiguousarray(P).reshape(-1)
        assert host.pion_host_sim_init(s, Pc.ctypes.data_as(dp), 0.0, 1e300, -1.0) == 0
        t, ldt = C.c_double(), C.c_double()
        assert host.pion_host_sim_time_int(s, 8, C.byref(t), C.byref(ldt)) == 8
        out = np.empty_like(Pc)
        assert host.pion_host_sim_download(s, 0, out.ctypes.data_as(dp)) == 0
        hcells = [hs.get_wind_cells(k) for k in range(2)]
        hpos = [hs.get_wind_source_pos(k) for k in range(2)]
        hflags = hs.get_flags()
    finally:
        host.pion_host_sim_destroy(s)
    with lib.GpuSim(cfg, 0) as g:
        for src in srcs:
            g.add_wind_source(src)
        sc = driver.SimControl(g, cfg)
        sc.first_step_dt_limit = wind.first_step_dt_limit(cfg, srcs)
        sc.init(P)
        sc.time_int(8)
        assert sc.simtime == t.value and sc.last_dt == ldt.value
        assert np.array_equal(g.download(0).reshape(-1), out)
        for k in range(2):
            gi, gs = g.get_wind_cells(k)
            assert np.array_equal(gi, hcells[k][0]) and np.array_equal(gs, hcells[k][1])
            assert g.get_wind_source_pos(k) == hpos[k] != tuple(srcs[k].pos)
        assert np.array_equal(g.get_flags(), hflags)
