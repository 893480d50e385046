"""Cases shared by tests/golden/make_golden_cooling_forms.py (the fixture generator) and the tests of the cooling
functions of mp_only_cooling other than the tabulated one: EP.cooling = 2 (KI02) and 4..7 (a total-CIE curve the caller
supplies).  The two curves are SYNTHETIC: no published table is restated here."""
import math

import numpy as np

from pion_amd import abi, cooling, problems

FLAGS = [4, 5, 6, 7]
CURVES = ["knots9", "uniform64"]
GAMMA = 5.0 / 3.0
MIN_TEMP, MAX_TEMP = 1.0e2, 1.0e9       # EP.MinTemperature / MaxTemperature of the cooling-only vectors
NSTATES = 200
NSTEPS = 2

# constants.h:53,64; mp_only_cooling.cpp:81-85
M_P, K_B = 1.672621898e-24, 1.38064852e-16
MU, MU_TOT, MU_ELEC, MU_ION = 1.40 * M_P, 0.609 * M_P, 1.167 * M_P, 1.273 * M_P
MU_TOT_OVER_KB = MU_TOT / K_B


def curve_knots(name):
    """(log10 T, log10 Lambda) of a synthetic curve over 1e4..1e8 K, so that states fall below, inside and above"""
    if name == "knots9":
        x = np.array([4.0, 4.2, 4.5, 5.0, 5.4, 6.1, 6.9, 7.4, 8.0])
        y = np.array([-23.5, -21.9, -21.4, -21.2, -21.6, -22.3, -22.6, -22.7, -22.5])
        return x, y
    if name == "uniform64":
        x = np.linspace(4.0, 8.0, 64)
        y = -22.0 + 0.6 * np.sin(1.7 * (x - 4.0)) - 0.15 * (x - 6.0) ** 2 + 0.2 * np.cos(5.3 * x)
        return x, y
    raise KeyError(name)


def set_curve(name):
    """makes `name` the host library's process-global curve; returns what GpuSim.set_cooling_curve takes"""
    return cooling.set_curve(*curve_knots(name))


def _libm(fn):
    """the C library's function element-wise (numpy's own vector exp / log may differ from it in the last bit, and the
    restatement is compared with the reference's compiled code to a few ulp)"""
    def f(x):
        x = np.asarray(x, dtype=np.float64)
        out = np.empty(x.shape)
        for i, v in np.ndenumerate(x):
            try:
                out[i] = fn(float(v))
            except (ValueError, OverflowError):
                out[i] = np.nan
        return out
    return f


_exp, _log = _libm(math.exp), _libm(math.log)


def _heat(T):
    """2.733e-21*exp(-0.782991*log(T)) (mp_only_cooling.cpp:446, 481)"""
    return 2.733e-21 * _exp(-0.782991 * _log(T))


# ---- restatement of the rate formulas (numpy; each line cites the reference's) ----------------------------------
def ki02_lambda(T):
    """the cooling term of CoolingFn::CoolingRate, WhichFunction 2, per n^2 (cooling.cpp:390-391; MinTemp = 5 K, :110)"""
    T = np.asarray(T, dtype=np.float64)
    with np.errstate(all="ignore"):
        lam = 2.0e-19 * np.exp(-1.184e5 / (T + 1.0e3)) + 2.8e-28 * np.sqrt(T) * np.exp(-92.0 / T)
    return np.where(T > 5.0, lam, 0.0)


def ki02_lambda_scalar(T):
    """KI02's Lambda as the CIE curve of a flag 7 run (one double in, one out): inf for T < 0 or non-finite T, as
    cooling_rate_SD93CIE gives (cooling_SD93_cie.cpp:674-675), so that the integrator halves its step there"""
    if T < 0.0 or not np.isfinite(T):
        return np.inf
    return float(ki02_lambda(T))


def edot(flag, rho, T, lam=None):
    """mp_only_cooling::Edot (mp_only_cooling.cpp:377-415); lam = Lambda(T) of the CIE curve for flags 4..7"""
    rho = np.asarray(rho, dtype=np.float64)
    T = np.asarray(T, dtype=np.float64)
    with np.errstate(all="ignore"):
        if flag == 2:
            # :387  rate = -CoolingRate(T, 0, rho/Mu, 0, 0); cooling.cpp:333-336 (0 for T <= 0 or non-finite T),
            # :390-391 cooling for T > MinTemp, :395 heating 2e-26 n
            n = rho / MU
            rate = n * n * ki02_lambda(T) - n * 2.0e-26
            return np.where((T <= 0.0) | ~np.isfinite(T), -0.0, -rate)
        heat = _heat(T)
        if flag == 4:    # :429
            return -(rho * rho / MU_ELEC / MU_ION) * lam
        if flag == 5:    # :446-447
            return (rho * rho) * (heat / MU_ELEC / MU - lam / MU_ELEC / MU_ION)
        if flag == 7:    # :463
            return 2e-26 * rho / MU - (rho * rho / MU / MU) * lam
        if flag == 6:    # :481
            return (rho * rho) * (heat / MU_ELEC / MU - lam / MU / MU)
    raise KeyError(flag)


def edot_terms(flag, rho, T, lam=None):
    """the larger of |heating| and |cooling| of Edot: the scale of the project's Edot gate"""
    rho = np.asarray(rho, dtype=np.float64)
    T = np.asarray(T, dtype=np.float64)
    with np.errstate(all="ignore"):
        if flag == 2:
            n = rho / MU
            return np.maximum(n * n * ki02_lambda(T), n * 2.0e-26)
        heat = _heat(T)
        if flag == 4:
            return (rho * rho / MU_ELEC / MU_ION) * lam
        if flag == 5:
            return np.maximum(rho * rho * heat / MU_ELEC / MU, rho * rho * lam / MU_ELEC / MU_ION)
        if flag == 7:
            return np.maximum(2e-26 * rho / MU, (rho * rho / MU / MU) * lam)
        return np.maximum(rho * rho * heat / MU_ELEC / MU, rho * rho * lam / MU / MU)


def limits():
    """MinT_allowed, MaxT_allowed as the constructor leaves them (mp_only_cooling.cpp:140-146)"""
    return MIN_TEMP, MAX_TEMP


def timescale(flag, rho, pg, rate_fn, min_temp=MIN_TEMP):
    """mp_only_cooling::timescales, cooling time only (mp_only_cooling.cpp:333-368); rate_fn(T) = Lambda(T)"""
    rho = np.asarray(rho, dtype=np.float64)
    pg = np.asarray(pg, dtype=np.float64)
    Eint = pg / (GAMMA - 1.0)                      # :346
    T = pg * MU_TOT_OVER_KB / rho                  # :347
    T2 = np.maximum(min_temp, 0.5 * T)             # :360
    lam = (lambda t: None) if flag == 2 else rate_fn
    with np.errstate(all="ignore"):
        rate = np.maximum(np.abs(edot(flag, rho, T, lam(T))), np.abs(edot(flag, rho, T2, lam(T2))))   # :359-360
        t = np.minimum(1.0e99, Eint / rate)        # :361
    return np.where(T >= 1.1 * min_temp, t, 1.0e99)   # :354


# ---- cooling-only vectors ---------------------------------------------------------------------------------------
def cool_cfg(flag, strict_fp=1):
    """a 1-D periodic grid of 4 cells, first order: with identical cells at rest the dynamics vanish exactly, a full
    step is TimeUpdateMP(P, dt) and the microphysics time step is timescales(P)"""
    return abi.make_config(1, [4], abi.EQEUL, abi.FLUX_RSroe, artvisc=abi.AV_NONE, gamma=GAMMA, cfl=0.3, dx=1.0e16,
                           bcs=["periodic", "periodic"], refvec=[1.0e-24, 1.0e-13, 1.0e6, 1.0e6, 1.0e6], ooa=1, nbc=2,
                           min_temp=MIN_TEMP, max_temp=MAX_TEMP, cooling=flag, mp_timestep_limit=1, strict_fp=strict_fp)


def cool_states(seed, rate_fn, flag, tlo=1.5, thi=9.5, n=NSTATES, redrawn=None):
    """n (rho, p) states and a dt each: rho and T log-uniform, T from below MinTemperature to above MaxTemperature
    (10^tlo .. 10^thi K), dt from 1e-3 to 1e2 cooling times E / |Edot| (restated); 10 of them far shorter"""
    rng = np.random.default_rng(seed)
    rho = 10.0 ** rng.uniform(-26.0, -20.0, n)
    T = 10.0 ** rng.uniform(tlo, thi, n)
    pg = rho * T / MU_TOT_OVER_KB
    lam = None if flag == 2 else rate_fn(T)
    with np.errstate(all="ignore"):
        tc = pg / (GAMMA - 1.0) / np.abs(edot(flag, rho, T, lam))
    tc = np.where(np.isfinite(tc) & (tc > 0.0), tc, 1.0e12)
    dt = tc * 10.0 ** rng.uniform(-3.0, 2.0, n)
    # the first-order shortcut of Step_RK5CK needs |Edot| dt / E < 1e-6 (integrator.cpp:325-339): with dt >= 1e-3
    # cooling times a purely cooling function never gets there, so the first 10 states take 1e-9 .. 1e-7 of one
    dt[:10] = tc[:10] * 10.0 ** rng.uniform(-9.0, -7.0, 10)
    if flag != 2:
        # A state whose result the reference's own algorithm moves by more than a fifth of the 1e-10 pressure gate when
        # the curve changes by 1e-15 (one ulp) cannot be held to that gate by any build whose exp / log10 differ from
        # the host's in the last bit: it is drawn again (judged on the scalar restatement of TimeUpdateMP, host only)
        for i in range(n):
            for _ in range(50):
                p = [time_update(flag, rho[i], pg[i], dt[i], (lambda t, e=e: rate_fn(t) * (1.0 + e)), MIN_TEMP, MAX_TEMP, {})
                     for e in (0.0, 1.0e-15, -1.0e-15)]
                if max(abs(p[1] / p[0] - 1.0), abs(p[2] / p[0] - 1.0)) <= 2.0e-11:
                    break
                if redrawn is not None:
                    redrawn.append(i)   # (one entry per draw that was discarded)
                rho[i] = 10.0 ** rng.uniform(-26.0, -20.0)
                Ti = 10.0 ** rng.uniform(tlo, thi)
                pg[i] = rho[i] * Ti / MU_TOT_OVER_KB
                with np.errstate(all="ignore"):
                    tci = pg[i] / (GAMMA - 1.0) / abs(float(edot(flag, rho[i], Ti, rate_fn(Ti))))
                tci = tci if (np.isfinite(tci) and tci > 0.0) else 1.0e12
                dt[i] = tci * 10.0 ** (rng.uniform(-9.0, -7.0) if i < 10 else rng.uniform(-3.0, 2.0))
    return rho, pg, dt


def cool_seed(flag, ci):
    return 1000 * flag + ci


KI02_SEED = 2002
KI02_MIN_TEMP = 1.0   # EP.MinTemperature of the KI02 vectors: states on both sides of the 5 K threshold are updated


def ki02_cfg(flag, strict_fp=1):
    cfg = cool_cfg(flag, strict_fp)
    cfg.min_temp = KI02_MIN_TEMP
    cfg.max_temp = 1.0e8
    return cfg


def ki02_states(n=NSTATES):
    """KI02 through flag 7's form: T from 1.5 K to 1e6 K (both sides of the 5 K threshold), n_H from 0.01 to 1e4"""
    rng = np.random.default_rng(KI02_SEED)
    rho = MU * 10.0 ** rng.uniform(-2.0, 4.0, n)
    T = 10.0 ** rng.uniform(np.log10(1.5), 6.0, n)
    T[:20] = rng.uniform(4.0, 6.0, 20)
    pg = rho * T / MU_TOT_OVER_KB
    with np.errstate(all="ignore"):
        tc = pg / (GAMMA - 1.0) / np.abs(edot(2, rho, T))
    tc = np.where(np.isfinite(tc) & (tc > 0.0), tc, 1.0e12)
    dt = tc * 10.0 ** rng.uniform(-3.0, 2.0, n)
    dt[20:30] = tc[20:30] * 10.0 ** rng.uniform(-9.0, -7.0, 10)   # (the first-order shortcut, as in cool_states)
    return rho, pg, dt


def uniform_state(cfg, rho, pg):
    P = problems.alloc(cfg)
    P[abi.RO] = rho
    P[abi.PG] = pg
    return P


# ---- whole steps and the end state ------------------------------------------------------------------------------
STEP_CASES = {"hd_roe_tr_3d": (5, "uniform64"), "cyl_hd_2d": (6, "knots9"), "glm_hlld_3d": (7, "uniform64"),
              "hd_1d": (4, "knots9")}
END_CASE = ("blast16", 6, "uniform64", 40)
_L = 3.0e18
_RV = [1.0e-24, 1.0e-13, 1.0e6, 1.0e6, 1.0e6]


def _blob(cfg, X, Y, Z, centre, ntr=0, B=None):
    """a smooth state (10 % waves in density, 3e4 K, 10 km/s shear) with a hot (3e8 K), dense (x 30) blob: the gas lies
    inside the curve's knots, the blob beyond its upper end, and the expanding blob's rim cools below the lower one"""
    P = problems.alloc(cfg)
    L = _L
    r2 = (X - centre[0]) ** 2 + (Y - centre[1]) ** 2 + (Z - centre[2]) ** 2
    w = np.exp(-r2 / (0.15 * L) ** 2)
    ro = 2.0e-24 * (1.0 + 0.1 * np.sin(2 * np.pi * X / L) * np.cos(2 * np.pi * (Y + 0.3 * Z) / L)) * (1.0 + 29.0 * w)
    T = 3.0e3 * (1.0 + 9.0 * (0.5 + 0.5 * np.cos(2 * np.pi * (X + Y) / L))) * (1.0 - w) + 3.0e8 * w
    P[abi.RO] = ro
    P[abi.PG] = ro * T / MU_TOT_OVER_KB
    P[abi.VX] = 1.0e6 * np.sin(2 * np.pi * Y / L)
    P[abi.VY] = -0.5e6 * np.sin(2 * np.pi * X / L)
    if cfg.ndim == 3:
        P[abi.VZ] = 0.3e6 * np.cos(2 * np.pi * X / L)
    if B is not None:
        P[abi.BX], P[abi.BY], P[abi.BZ] = B
    for t in range(ntr):
        P[cfg.nvar - ntr + t] = w
    return P


def step_case(name, strict_fp=1):
    """(cfg, P): two second-order steps of each are recorded"""
    flag, _ = STEP_CASES[name]
    L = _L
    kw = dict(gamma=GAMMA, cfl=0.3, min_temp=1.0e2, max_temp=1.0e9, cooling=flag, mp_timestep_limit=1,
              strict_fp=strict_fp, artvisc=abi.AV_FKJ98_1D, etav=0.15)
    if name == "hd_roe_tr_3d":
        cfg = abi.make_config(3, [12, 10, 8], abi.EQEUL, abi.FLUX_RSroe, ntracer=1, dx=L / 12, refvec=_RV + [1.0],
                              bcs=["periodic"] * 6, **kw)
        X, Y, Z = problems.mesh(cfg)
        return cfg, _blob(cfg, X, Y, Z, (0.4 * L, 0.45 * L, 0.3 * L), ntr=1)
    if name == "cyl_hd_2d":
        cfg = abi.make_config(2, [24, 16], abi.EQEUL, abi.FLUX_RSroe, dx=L / 24, refvec=_RV, coord_sys=2,
                              bcs=["one-way-outflow", "one-way-outflow", "axisymmetric", "one-way-outflow"], **kw)
        X, Y, Z = problems.mesh(cfg)
        P = _blob(cfg, X, Y, 0.0 * Z, (0.5 * L, 0.0, 0.0))
        P[abi.VY] *= np.abs(Y) / L   # no flow through the axis
        return cfg, P
    if name == "glm_hlld_3d":
        cfg = abi.make_config(3, [12, 10, 8], abi.EQGLM, abi.FLUX_RS_HLLD, dx=L / 12,
                              refvec=_RV + [1.0e-6, 1.0e-6, 1.0e-6, 1.0e-6], bcs=["periodic"] * 6, **kw)
        X, Y, Z = problems.mesh(cfg)
        return cfg, _blob(cfg, X, Y, Z, (0.55 * L, 0.4 * L, 0.35 * L), B=(1.0e-6, 0.5e-6, 0.2e-6))
    if name == "hd_1d":
        cfg = abi.make_config(1, [64], abi.EQEUL, abi.FLUX_RSroe, dx=L / 64, refvec=_RV, bcs=["periodic"] * 2, **kw)
        X, Y, Z = problems.mesh(cfg)
        P = _blob(cfg, X, 0.0 * Y, 0.0 * Z, (0.5 * L, 0.0, 0.0))
        P[abi.VY] = 0.0
        return cfg, P
    raise KeyError(name)


def end_case(strict_fp=1):
    """a 16^3 radiative blast, flag 6: (cfg, P, steps)"""
    _, flag, _, nsteps = END_CASE
    L = _L
    cfg = abi.make_config(3, [16, 16, 16], abi.EQEUL, abi.FLUX_RSroe, ntracer=1, dx=L / 16, refvec=_RV + [1.0],
                          bcs=["reflecting", "one-way-outflow"] * 3, gamma=GAMMA, cfl=0.3, min_temp=1.0e2,
                          max_temp=1.0e9, cooling=flag, mp_timestep_limit=1, strict_fp=strict_fp,
                          artvisc=abi.AV_FKJ98_1D, etav=0.15)
    X, Y, Z = problems.mesh(cfg)
    return cfg, _blob(cfg, X, Y, Z, (0.0, 0.0, 0.0), ntr=1), nsteps


# ---- the reference side (oracle/_ref, where it is built) ---------------------------------------------------------
class RefCieCurve:
    """While open, the reference's cooling_rate_SD93CIE (the test double of oracle/ref_cooling.cpp) is `fn`: the address
    of a double(double) C function, or a Python callable (wrapped in a ctypes callback).  On exit the curves of
    EP.cooling = 8 are back, so that other tests' reference objects see what they expect."""

    def __init__(self, fn):
        import ctypes as C
        import cpu_backends
        cpu_backends.install_ref_rate_curves()   # (the three curves of EP.cooling = 8; ours replaces the CIE one)
        self.C = C
        self.ref = C.CDLL(cpu_backends.REF_SO)
        self.ref.ref_cooling_set_rate_curves.restype = None
        self.host = cooling._load()
        if callable(fn) and not isinstance(fn, C._CFuncPtr):
            self.keep = C.CFUNCTYPE(C.c_double, C.c_double)(fn)
            fn = self.keep
        self.fn = C.cast(fn, C.c_void_p)

    def _others(self):
        return [self.C.cast(getattr(self.host, f), self.C.c_void_p) for f in ("pion_host_hii_rrr", "pion_host_hii_total_cooling")]

    def __enter__(self):
        self.ref.ref_cooling_set_rate_curves(self.fn, *self._others())
        return self

    def __exit__(self, *a):
        self.ref.ref_cooling_set_rate_curves(self.C.cast(self.host.pion_host_cooling_rate_wss09, self.C.c_void_p), *self._others())


def host_curve_fn():
    """pion_host_cooling_curve_rate as the reference's CIE curve"""
    return cooling._load().pion_host_cooling_curve_rate


def ref_cool_only(cfg, rho, pg, dt):
    """the reference on the 4-cell grid, state by state: (p after a full first-order step of dt[i], t_mp, T_final)"""
    from cpu_backends import CpuSim
    from pion_amd import driver
    p_out, t_mp = np.zeros(rho.size), np.zeros(rho.size)
    nb = cfg.nbc
    with CpuSim(cfg, "ref") as r:
        sc = driver.SimControl(r, cfg)
        for i in range(rho.size):
            sc.simtime = 0.0
            sc.init(uniform_state(cfg, rho[i], pg[i]))
            t_mp[i] = r.calc_dt()[1]
            r.stage(float(dt[i]), 1, 1)
            A = r.download(0)[:, 0, 0, nb:-nb]
            assert (A == A[:, :1]).all() and (A[abi.VX:abi.VZ + 1] == 0.0).all() and (A[abi.RO] == rho[i]).all()
            p_out[i] = A[abi.PG, 0]
    return p_out, t_mp


def ref_steps(cfg, P, nsteps):
    """nsteps steps of the reference: (every dt, the end state)"""
    from cpu_backends import CpuSim
    from pion_amd import driver
    with CpuSim(cfg, "ref") as r:
        sc = driver.SimControl(r, cfg)
        sc.init(P)
        dts = []
        for _ in range(nsteps):
            dts.append(sc.calculate_timestep())
            sc.advance_time()
        sc.finish_halo()
        return np.array(dts), r.download(0)


# ---- scalar restatement of TimeUpdateMP, counting the branches it takes ------------------------------------------
def edot_scalar(flag, rho, T, rate_fn):
    """Edot for one state (the formulas of edot() above, with the C library's functions)"""
    if flag == 2:
        if T <= 0.0 or not math.isfinite(T):
            return -0.0
        n = rho / MU
        rate = 0.0
        if T > 5.0:
            rate += n * n * (2.0e-19 * math.exp(-1.184e5 / (T + 1.0e3)) + 2.8e-28 * math.sqrt(T) * math.exp(-92.0 / T))
        return -(rate - n * 2.0e-26)
    lam = rate_fn(T)
    if flag == 4:
        return -(rho * rho / MU_ELEC / MU_ION) * lam
    if flag == 7:
        return 2e-26 * rho / MU - (rho * rho / MU / MU) * lam
    heat = 2.733e-21 * math.exp(-0.782991 * math.log(T)) if T > 0.0 else math.nan
    if flag == 5:
        return (rho * rho) * (heat / MU_ELEC / MU - lam / MU_ELEC / MU_ION)
    return (rho * rho) * (heat / MU_ELEC / MU - lam / MU / MU)


def time_update(flag, rho, pg, dt, rate_fn, min_t, max_t, count):
    """mp_only_cooling::TimeUpdateMP (mp_only_cooling.cpp:167-218) with Int_Adaptive_RKCK, Stepper_RKCK and Step_RK5CK
    (integrator.cpp:285-602) for one state; count: dict of branch counters"""
    g = GAMMA

    def f(E):
        return edot_scalar(flag, rho, E * (g - 1.0) * MU_TOT_OVER_KB / rho, rate_fn)

    def step(p0, h):
        k1 = f(p0)
        if abs(k1) * h / (p0 + 1.0e-100) < 1.e-6:
            count["shortcut"] = count.get("shortcut", 0) + 1
            return p0 + k1 * h, k1 * h
        count["cashkarp"] = count.get("cashkarp", 0) + 1
        k1 *= h
        k2 = f(p0 + 0.2 * k1) * h
        k3 = f(p0 + 3. / 40. * k1 + 9. / 40. * k2) * h
        k4 = f(p0 + 0.3 * k1 + -0.9 * k2 + 1.2 * k3) * h
        k5 = f(p0 + -11. / 54. * k1 + 2.5 * k2 + -70. / 27. * k3 + 35. / 27. * k4) * h
        k6 = f(p0 + 1631. / 55296. * k1 + 175. / 512. * k2 + 575. / 13824. * k3 + 44275. / 110592. * k4 + 253. / 4096. * k5) * h
        c1, c3, c4, c6 = 37. / 378., 250. / 621., 125. / 594., 512. / 1771.
        pf = p0 + c1 * k1 + c3 * k3 + c4 * k4 + c6 * k6
        dp = ((c1 - 2825. / 27648.) * k1 + (c3 - 18575. / 48384.) * k3 + (c4 - 13525. / 55296.) * k4
              + -277. / 14336. * k5 + (c6 - 0.25) * k6)
        return pf, dp

    t, p1, h, ct, err = 0.0, pg / (g - 1.0), dt, 0, 0
    while True:
        hh, n = h, 0
        while True:
            with np.errstate(all="ignore"):
                ptemp, e = step(p1, hh)
            if not math.isfinite(e) or not math.isfinite(ptemp) or ptemp < 0.0:
                maxerr = 1000.0
            else:
                maxerr = abs(e / (abs(ptemp) + 1.e-100) / 1.0e-2)
            if maxerr > 1.0:
                hh /= 2.0
                count["halved"] = count.get("halved", 0) + 1
            n += 1
            if not (maxerr > 1.0 and n < 50):
                break
        if maxerr > 1.0:
            err += 1
        t += hh
        h = min(hh * 2.0, dt - t)
        ct += 1
        p1 = ptemp
        if not (t < dt and err == 0 and ct < 25):
            break
    p = p1 * (g - 1.0)
    T = p * MU_TOT_OVER_KB / rho
    if T > max_t:
        p *= max_t / T
        count["clamp_hi"] = count.get("clamp_hi", 0) + 1
    elif T < min_t:
        p *= min_t / T
        count["clamp_lo"] = count.get("clamp_lo", 0) + 1
    return p
