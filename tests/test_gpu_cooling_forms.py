"""The cooling functions of mp_only_cooling other than the tabulated one on the device: EP.cooling = 2 (KI02) and 4..7
(a total-CIE curve the caller supplies), both floating-point builds.

References: pion_host_cooling_curve_rate for the curve; the numpy restatement of Edot (cooling_forms_cases.edot, pinned
to the reference's compiled code within 4 ulp through timescales, tests/test_cooling_forms.py); and
tests/golden/cooling_forms.npz, the reference's own mp_only_cooling object on the same curve (cooling-only vectors, KI02
through flag 7's form, whole steps, a 40-step run).  The device evaluates log10, exp and log itself, so the strict
build is not bit-identical to the fixtures; the gates are DESIGN.md s2's."""
import os
import sys

import numpy as np
import pytest

import cooling_forms_cases as cf
import golden_cases as gc
from pion_amd import abi, cooling, driver, lib

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
BUILDS = pytest.mark.parametrize("strict", [1, 0], ids=["strict", "fast"])


@pytest.fixture(scope="module")
def gold():
    z = np.load(os.path.join(HERE, "golden", "cooling_forms.npz"))
    return {k: z[k] for k in z.files}


def _gpu(cfg, cname=None):
    g = lib.GpuSim(cfg, 0)
    if cname is not None:
        g.set_cooling_curve(*cf.set_curve(cname))
    return g


# ------------------------------------------------------------------------------------------- flags and the missing curve
@pytest.mark.parametrize("flag", [2, 4, 5, 6, 7])
def test_create_accepts_the_cooling_flag(flag):
    with lib.GpuSim(cf.cool_cfg(flag), 0) as g:
        assert g.h


@pytest.mark.parametrize("flag", [1, 3, 9, -1])
def test_create_refuses_other_flags(flag):
    with pytest.raises(lib.PionGpuError) as e:
        lib.GpuSim(cf.cool_cfg(flag), 0)
    assert e.value.rc == -1   # PION_GPU_EINVAL


@BUILDS
def test_missing_curve_is_einval_and_nothing_is_launched(strict):
    cfg = cf.cool_cfg(6, strict_fp=strict)
    P = cf.uniform_state(cfg, 1.0e-24, 1.0e-12)
    with lib.GpuSim(cfg, 0) as g:
        g.upload(P)
        before = g.download(0)
        for call in (lambda: g.stage(1.0e8, 1, 1), lambda: g.calc_dt(), lambda: g.cooling_edot([1e-24], [1e5]),
                     lambda: g.cooling_timescale(np.ones((1, 5))), lambda: g.cooling_update(np.ones((1, 5)), 1.0),
                     lambda: g.cooling_curve_eval([1e5])):
            with pytest.raises(lib.PionGpuError, match="cooling curve not set"):
                call()
        assert np.array_equal(g.download(0), before)
        # the process goes on: with the curve the same handle runs
        g.set_cooling_curve(*cf.set_curve("knots9"))
        g.update_bcs(0.0, 1, 1, 1)
        t_dyn, t_mp = g.calc_dt()
        assert 0.0 < t_mp < 1.0e99
        g.stage(1.0e-3 * t_mp, 1, 1)
        assert (g.download(0)[abi.PG] != before[abi.PG]).any()
    # KI02 needs no curve, and no table
    with lib.GpuSim(cf.cool_cfg(2, strict_fp=strict), 0) as g:
        assert np.isfinite(g.cooling_edot([1e-24], [1e3])).all()


def test_set_cooling_curve_refuses_bad_curves():
    x, y, c, smin, smax = cf.set_curve("knots9")
    with lib.GpuSim(cf.cool_cfg(7), 0) as g:
        for args in ((x[:1], y[:1], c[:1], smin, smax), (x[::-1].copy(), y, c, smin, smax), (x, y, c, np.nan, smax),
                     (x, np.r_[y[:-1], np.inf], c, smin, smax), (x, y, np.r_[c[:-1], np.nan], smin, smax),
                     (np.arange(257.0), np.zeros(257), np.zeros(257), smin, smax)):
            with pytest.raises(lib.PionGpuError):
                g.set_cooling_curve(*args)
            with pytest.raises(lib.PionGpuError, match="cooling curve not set"):
                g.cooling_edot([1e-24], [1e5])
        g.set_cooling_curve(np.arange(256.0) / 32, np.full(256, -22.0), np.zeros(256), smin, smax)   # the most knots
        assert np.allclose(g.cooling_curve_eval([1e3, 1e5]), 1e-22, rtol=1e-12)


# ------------------------------------------------------------------------------------------- the curve
def _curve_temperatures(x):
    """2000 temperatures: every knot, its two neighbours in floating point, both extrapolated sides, the inside"""
    rng = np.random.default_rng(5)
    T = 10.0 ** rng.uniform(x[0] - 3.0, x[-1] + 2.5, 2000)
    k = 10.0 ** x
    T[:x.size] = k
    T[x.size:2 * x.size] = np.nextafter(k, 0.0)
    T[2 * x.size:3 * x.size] = np.nextafter(k, np.inf)
    # and the temperatures whose log10 is the knot itself or next to it, as far as 10**x gets there
    T[3 * x.size:4 * x.size] = 10.0 ** np.nextafter(x, -np.inf)
    T[4 * x.size:5 * x.size] = 10.0 ** np.nextafter(x, np.inf)
    T[-4:] = [0.0, 1e-300, 1e300, 5e-324]
    return T


@BUILDS
@pytest.mark.parametrize("bisect", [0, 1], ids=["guess", "bisect"])
@pytest.mark.parametrize("cname", cf.CURVES)
def test_device_curve_equals_host_curve(cname, bisect, strict, monkeypatch):
    """pion_gpu_cooling_curve_eval (the kernels' own function, curve in LDS) against pion_host_cooling_curve_rate to
    1e-12 relative; uniform knots with the spacing guess and with PION_COOL_BISECT=1, non-uniform knots bisect anyway"""
    if bisect:
        monkeypatch.setenv("PION_COOL_BISECT", "1")
    x, _ = cf.curve_knots(cname)
    T = _curve_temperatures(x)
    with _gpu(cf.cool_cfg(6, strict_fp=strict), cname) as g:
        got = g.cooling_curve_eval(T)
        bad = g.cooling_curve_eval([-1.0, np.nan, np.inf, -np.inf])
    want = cooling.curve_rate(T)
    assert np.isfinite(want[:-4]).all() and (want[:-4] > 0).all()
    over = np.isinf(want)   # (1e300 K on a rising upper extrapolation: both overflow)
    assert np.array_equal(np.isinf(got), over)
    err = np.where(over, 0.0, np.abs(got - np.where(over, 0.0, want)) / np.where((want > 0) & ~over, want, 1.0))
    print("curve %s bisect %d strict %d: max rel %.3e" % (cname, bisect, strict, err.max()))
    assert err.max() <= 1e-12
    assert np.isinf(bad).all() and (bad > 0).all()


# ------------------------------------------------------------------------------------------- Edot
@BUILDS
@pytest.mark.parametrize("cname", cf.CURVES)
@pytest.mark.parametrize("flag", cf.FLAGS)
def test_device_edot_equals_restatement(flag, cname, strict):
    """1000 (rho, T) pairs per flag and curve: within 1e-9 of the larger of the heating and cooling terms"""
    rng = np.random.default_rng(100 + flag)
    rho = 10.0 ** rng.uniform(-26, -19, 1000)
    x, _ = cf.curve_knots(cname)
    T = 10.0 ** rng.uniform(0.5, 10.0, 1000)
    T[:x.size] = 10.0 ** x
    with _gpu(cf.cool_cfg(flag, strict_fp=strict), cname) as g:
        got = g.cooling_edot(rho, T)
        bad = g.cooling_edot([1e-24] * 3, [-1.0, np.nan, np.inf])
    lam = cooling.curve_rate(T)
    want, scale = cf.edot(flag, rho, T, lam), cf.edot_terms(flag, rho, T, lam)
    err = np.abs(got - want) / scale
    print("edot flag %d %s strict %d: max %.3e of the larger term" % (flag, cname, strict, err.max()))
    assert err.max() <= 1e-9
    assert not np.isfinite(bad).any()   # reaches the integrator unchanged: its !isfinite branch halves the step


@BUILDS
def test_device_edot_ki02(strict):
    rng = np.random.default_rng(102)
    rho = cf.MU * 10.0 ** rng.uniform(-3, 6, 1000)
    T = 10.0 ** rng.uniform(0.0, 8.0, 1000)
    T[:8] = [5.0, np.nextafter(5.0, 0.0), np.nextafter(5.0, 10.0), 0.0, -1.0, -np.inf, np.inf, np.nan]
    with _gpu(cf.cool_cfg(2, strict_fp=strict)) as g:
        got = g.cooling_edot(rho, T)
    want, scale = cf.edot(2, rho, T), cf.edot_terms(2, rho, T)
    n = rho / cf.MU
    assert np.array_equal(got[3:8], np.zeros(5))              # T <= 0 or not finite: CoolingRate returns 0
    assert got[0] == 2.0e-26 * n[0] and got[1] == 2.0e-26 * n[1]   # T <= 5 K: heating only
    assert got[2] < 2.0e-26 * n[2]                            # just above: the cooling term is there
    ok = np.isfinite(T) & (T > 0)
    err = np.abs(got[ok] - want[ok]) / scale[ok]
    print("edot KI02 strict %d: max %.3e of the larger term" % (strict, err.max()))
    assert err.max() <= 1e-9


# ------------------------------------------------------------------------------------------- TimeUpdateMP, timescales
def _check_vectors(g, rho, pg, dt, want_p, want_t):
    P = np.zeros((rho.size, 5))
    P[:, abi.RO], P[:, abi.PG] = rho, pg
    t = g.cooling_timescale(P)
    terr = np.max(np.abs(t / want_t - 1.0))
    # one launch per dt: the seam takes one dt for all its states
    p = np.array([g.cooling_update(P[i:i + 1], float(dt[i]))[0] for i in range(rho.size)])
    assert np.array_equal(p[:, [0, 2, 3, 4]], P[:, [0, 2, 3, 4]])
    perr = np.abs(p[:, abi.PG] / want_p - 1.0)
    return perr, terr


@BUILDS
@pytest.mark.parametrize("cname", cf.CURVES)
@pytest.mark.parametrize("flag", cf.FLAGS)
def test_device_update_and_timescale_equal_the_reference(gold, flag, cname, strict):
    """every one of the 200 states: pressure within 1e-10 relative, time scale within 1e-9"""
    key = "f%d_%s_" % (flag, cname)
    with _gpu(cf.cool_cfg(flag, strict_fp=strict), cname) as g:
        perr, terr = _check_vectors(g, *(gold[key + k] for k in ("rho", "pg", "dt", "p", "t_mp")))
    print("update flag %d %s strict %d: max rel p %.3e (state %d), t %.3e" % (flag, cname, strict, perr.max(),
                                                                               perr.argmax(), terr))
    assert perr.size == cf.NSTATES and perr.max() <= 1e-10
    assert terr <= 1e-9


@BUILDS
def test_device_ki02_follows_flag7_with_ki02_curve(gold, strict):
    with _gpu(cf.ki02_cfg(2, strict_fp=strict)) as g:
        perr, terr = _check_vectors(g, *(gold["ki02_" + k] for k in ("rho", "pg", "dt", "p", "t_mp")))
    print("update KI02 strict %d: max rel p %.3e (state %d), t %.3e" % (strict, perr.max(), perr.argmax(), terr))
    assert perr.size == cf.NSTATES and perr.max() <= 1e-10
    assert terr <= 1e-9


# ------------------------------------------------------------------------------------------- whole steps
def _steps(cfg, P, cname, nsteps):
    with _gpu(cfg, cname) as g:
        sc = driver.SimControl(g, cfg)
        sc.init(P)
        dts = []
        for _ in range(nsteps):
            dts.append(sc.calculate_timestep())
            sc.advance_time()
        sc.finish_halo()
        return np.array(dts), g.download(0)


def _scaled_err(cfg, A, B):
    """the largest deviation of A from B over the on-grid cells, each variable in units of its own largest magnitude in
    B (the form of tests/test_gpu_parity.py); a variable that is zero everywhere in B must be zero in A"""
    a, b = gc.on_grid(cfg, A).reshape(cfg.nvar, -1), gc.on_grid(cfg, B).reshape(cfg.nvar, -1)
    scale = np.abs(b).max(axis=1, keepdims=True)
    zero = scale[:, 0] == 0.0
    assert (a[zero] == 0.0).all()
    return (np.abs(a - b)[~zero] / scale[~zero]).max()


@BUILDS
@pytest.mark.parametrize("kernel", ["rows", "cell"])
@pytest.mark.parametrize("name", sorted(cf.STEP_CASES))
def test_whole_steps_equal_the_reference(gold, name, kernel, strict, monkeypatch):
    """two second-order steps on the rows kernel (where the grid admits it) and on the cell-per-thread kernel: every dt
    within 1e-10 relative, every variable within 3e-11 of its own scale after both steps"""
    if kernel == "cell":
        monkeypatch.setenv("PION_STAGE_KERNEL", "cell")
    flag, cname = cf.STEP_CASES[name]
    cfg, P = cf.step_case(name, strict_fp=strict)
    dts, A = _steps(cfg, P, cname, cf.NSTEPS)
    derr = np.max(np.abs(dts / gold[name + "_dt"] - 1.0))
    err = _scaled_err(cfg, A, gold[name + "_P"])
    print("steps %s %s strict %d: dt %.3e state %.3e" % (name, kernel, strict, derr, err))
    assert derr <= 1e-10
    assert err <= 3e-11
    # the blob's cooling acted: the hottest cell has lost energy
    assert gc.on_grid(cfg, A)[abi.PG].max() < gc.on_grid(cfg, P)[abi.PG].max()


def _slab_worker(rank, world, port, strict, q):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, HERE)
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    import torch
    import torch.distributed as dist
    from pion_amd import slab
    torch.cuda.set_device(0)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    name = "hd_roe_tr_3d"
    cfg_g, P = cf.step_case(name, strict_fp=strict)
    cfg = slab.slab_config(cfg_g, rank, world)
    with lib.GpuSim(cfg, 0) as g:
        g.set_cooling_curve(*cf.set_curve(cf.STEP_CASES[name][1]))
        comm = slab.SlabComm(rank, world, True, g.halo_count(), torch.device("cuda", 0))
        comm.use_streams(g)
        sc = driver.SimControl(g, cfg, comm=comm)
        sc.init(slab.slab_slice(P, cfg_g, rank, world))
        dts = []
        for _ in range(cf.NSTEPS):
            dts.append(sc.calculate_timestep())
            sc.advance_time()
        sc.finish_halo()
        q.put((rank, np.array(dts), g.download(0)))
    dist.barrier()
    dist.destroy_process_group()


@BUILDS
def test_two_slabs_equal_the_reference(gold, strict):
    """the 3-D Euler case split into two z slabs (two ranks on one device, host-staged transport), both builds"""
    import torch.multiprocessing as mp
    name = "hd_roe_tr_3d"
    cfg, _ = cf.step_case(name)
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = 27500 + (os.getpid() % 2000) + 2000 * strict
    procs = [ctx.Process(target=_slab_worker, args=(r, 2, port, strict, q)) for r in range(2)]
    for p in procs:
        p.start()
    got = {}
    try:
        for _ in range(2):
            r, dts, A = q.get(timeout=240)
            got[r] = (dts, A)
    except Exception:
        for p in procs:
            p.kill()
        pytest.fail("the slab workers produced nothing within 240 s")
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    nb, nzl = cfg.nbc, cfg.ng[2] // 2
    want = gold[name + "_P"]
    for r in range(2):
        dts, A = got[r]
        assert np.max(np.abs(dts / gold[name + "_dt"] - 1.0)) <= 1e-10
        whole = want.copy()
        whole[:, nb + r * nzl: nb + (r + 1) * nzl] = A[:, nb:nb + nzl]
        # (the other slab's planes are the reference's own: only this rank's planes can differ)
        err = _scaled_err(cfg, whole, want)
        print("two slabs strict %d rank %d: state %.3e" % (strict, r, err))
        assert err <= 3e-11


@BUILDS
def test_cpp_loop_runs_a_curve_flag(gold, strict):
    """the C++ time loop (host_rccl.HostSim, one rank) with the curve handed over through its pass-through: the same two
    steps of the 3-D Euler case, flag 5, at the same gates"""
    from pion_amd import host_rccl
    name = "hd_roe_tr_3d"
    cfg, P = cf.step_case(name, strict_fp=strict)
    hs = host_rccl.HostSim(cfg, 0)
    try:
        hs.set_cooling_curve(*cf.set_curve(cf.STEP_CASES[name][1]))
        hs.init(P)
        dts = np.array([hs.step() for _ in range(cf.NSTEPS)])
        hs.finish_halo()
        A = np.asarray(hs.download(0)).reshape(P.shape)
    finally:
        hs.close()
    derr = np.max(np.abs(dts / gold[name + "_dt"] - 1.0))
    err = _scaled_err(cfg, A, gold[name + "_P"])
    print("C++ loop %s strict %d: dt %.3e state %.3e" % (name, strict, derr, err))
    assert derr <= 1e-10 and err <= 3e-11


# ------------------------------------------------------------------------------------------- end state
@BUILDS
def test_end_state_equals_the_reference(gold, strict):
    """40 steps of a 16^3 radiative blast, flag 6: L1 and L2 within 1e-10 refvec, conserved mass and momentum within 1e-10"""
    name, flag, cname, nsteps = cf.END_CASE
    cfg, P, nsteps = cf.end_case(strict_fp=strict)
    dts, A = _steps(cfg, P, cname, nsteps)
    want = gold[name + "_P"]
    derr = np.max(np.abs(dts / gold[name + "_dt"] - 1.0))
    l1, l2, mx = gc.diff_norms(cfg, A, want)
    tot, mag = gc.conserved_totals(cfg, A)
    tot_w, _ = gc.conserved_totals(cfg, want)
    cerr = (np.abs(tot - tot_w) / (mag + 1e-300))[:4].max()
    print("end state strict %d: dt %.3e L1 %.3e L2 %.3e max %.3e mass/momentum %.3e" % (strict, derr, l1.max(), l2.max(),
                                                                                         mx.max(), cerr))
    assert derr <= 1e-9
    assert l1.max() <= 1e-10 and l2.max() <= 1e-10
    assert cerr <= 1e-10
    tot0, _ = gc.conserved_totals(cfg, P)
    assert tot_w[-1] < 0.9 * tot0[-1]   # the blast has radiated


# ------------------------------------------------------------------------------------------- KI02 physics
@BUILDS
@pytest.mark.parametrize("n_H", [1.0, 100.0])
def test_ki02_gas_settles_at_its_equilibrium_temperature(n_H, strict):
    """a uniform 4-cell gas run to 50 cooling times ends within 1e-6 of the temperature where the restated rate vanishes"""
    from scipy.optimize import brentq
    rho = n_H * cf.MU
    Teq = brentq(lambda T: float(cf.edot(2, rho, T)), 10.0, 2.0e4, xtol=1e-12, rtol=1e-14)
    cfg = cf.ki02_cfg(2, strict_fp=strict)
    T0 = 3.0 * Teq
    pg = rho * T0 / cf.MU_TOT_OVER_KB
    # the cooling time of the equilibrium state: its thermal energy over its cooling term, which there equals the
    # heating 2e-26 n.  (The cooling time of the start state, three times hotter, is two orders shorter than the
    # relaxation it is meant to time: after 50 of those the gas has physically not arrived.)
    tc = rho * Teq / cf.MU_TOT_OVER_KB / (cf.GAMMA - 1.0) / (n_H * 2.0e-26)
    with _gpu(cfg) as g:
        g.upload(cf.uniform_state(cfg, rho, pg))
        g.update_bcs(0.0, 1, 1, 1)
        t, nstep = 0.0, 0
        while t < 50.0 * tc and nstep < 2000:
            t_dyn, t_mp = g.calc_dt()
            dt = min(t_mp, 50.0 * tc - t)
            g.stage(dt, 1, 1)
            g.update_bcs(t, 1, 1, 0)
            t += dt
            nstep += 1
        A = gc.on_grid(cfg, g.download(0))
    T = A[abi.PG] * cf.MU_TOT_OVER_KB / A[abi.RO]
    print("KI02 n_H %g strict %d: T_eq %.9g, reached %.9g in %d steps" % (n_H, strict, Teq, T.max(), nstep))
    assert t >= 50.0 * tc * (1 - 1e-12)
    assert (A[abi.VX:abi.VZ + 1] == 0.0).all()
    assert np.max(np.abs(T / Teq - 1.0)) <= 1e-6
