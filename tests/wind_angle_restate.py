"""Python `math` restatement of the reference's rotating-star wind (grid/stellar_wind_angle.cpp, WINDTYPE_ANGLE, after
Langer, Garcia-Segura & Mac Low 1999), for the rotating-source tests.

Every expression keeps the reference's operation order and cites its line (source/ of the PION tree).  Python floats
are IEEE doubles and `math` calls the C library, so the tables come out with the bits the host code of
libpion_gpu.so computes (it is built without contraction).  The states restate set_wind_cell_reference_state
(:464-691) per cell."""
import math

import numpy as np

from pion_amd import abi
import wind_restate as wr

PI, SQRT2 = 3.14159265358979324, 1.4142135623730950     # constants.h:45,48
ONE_MINUS_EPS = 1.0 - 1.0e-12                          # constants.h:151,157
C_GAMMA = 0.35                                         # stellar_wind_angle.cpp:60
NTHETA, NOMEGA, NTEFF = 25, 25, 22                     # :66-68


def pow_fast(a, b):
    """constants::pow_fast (constants.cpp:78-84)"""
    return math.exp(b * math.log(a))


def cmin(a, b):
    """std::min(a, b) = (b < a) ? b : a"""
    return b if b < a else a


def cmax(a, b):
    """std::max(a, b) = (a < b) ? b : a"""
    return b if a < b else a


def beta(Teff):
    """stellar_wind::beta (stellar_wind_BC.cpp:820-867)"""
    rsg = 0.125
    if Teff <= 3600.0:
        return rsg
    if Teff >= 22000.0:
        return 2.6
    if Teff < 6000.0:
        T0, b0, T1, b1 = 3600.0, rsg, 6000.0, 0.5
    elif Teff < 8000.0:
        T0, b0, T1, b1 = 6000.0, 0.5, 8000.0, 0.7
    elif Teff < 10000.0:
        T0, b0, T1, b1 = 8000.0, 0.7, 10000.0, 1.3
    elif Teff < 20000.0:
        T0, b0, T1, b1 = 10000.0, 1.3, 20000.0, 1.3
    else:
        T0, b0, T1, b1 = 20000.0, 1.3, 22000.0, 2.6
    return b0 + (Teff - T0) * (b1 - b0) / (T1 - T0)


def fn_phi(omega, theta, Teff):
    """:286-294"""
    ans = (omega / (22.0 * SQRT2 * beta(Teff))) * math.sin(theta) * pow_fast(1.0 - omega * math.sin(theta), -C_GAMMA)
    return cmin(ans, 0.5 * PI * ONE_MINUS_EPS)


def fn_alpha(omega, theta, Teff):
    """:304-315"""
    return pow_fast(math.cos(fn_phi(omega, theta, Teff))
                    + pow_fast(math.tan(theta), -2.0)
                    * (1.0 + C_GAMMA * (omega * math.sin(theta) / (1.0 - omega * math.sin(theta))))
                    * fn_phi(omega, theta, Teff)
                    * math.sin(fn_phi(omega, theta, Teff)), -1.0)


def integrand(theta, omega, Teff, xi):
    """:222-229"""
    return fn_alpha(omega, theta, Teff) * pow_fast(1.0 - omega * math.sin(theta), xi) * math.sin(theta)


def integrate_simpson(lo, hi, npt, omega, Teff, xi):
    """:239-276"""
    hh = (hi - lo) / npt
    ans = 0.0
    ans += integrand(lo, omega, Teff, xi)
    ans += integrand(hi, omega, Teff, xi)
    wt = 4
    for i in range(1, npt):
        x = lo + i * hh
        ans += wt * integrand(x, omega, Teff, xi)
        wt = 6 - wt
    ans *= hh / 3.0
    return ans


def fn_delta(omega, Teff, xi):
    """:325-333"""
    return 2.0 * pow_fast(integrate_simpson(0.001, PI / 2.0, 230, omega, Teff, xi), -1.0)


def fn_v_inf(omega, v_inf, theta):
    """:343-353"""
    omega = cmin(omega, 0.999)
    return cmax(0.5e5, v_inf * pow_fast(1.0 - omega * math.sin(theta), C_GAMMA))


class Tables:
    """setup_tables (:92-212) for one xi"""

    def __init__(self, xi):
        self.xi = xi
        th_min, th_mid, th_max = 0.1, 60.0, 89.9
        self.theta = [(th_min + k * ((th_mid - th_min) / 4.0)) * (PI / 180.0) if k <= 4 else
                      (th_mid + (k - 4) * ((th_max - th_mid) / (NTHETA - 5))) * (PI / 180.0) for k in range(NTHETA)]
        log_mu = [0.0] * NOMEGA
        for i in range(NOMEGA):
            log_mu[NOMEGA - i - 1] = -4.0 + i * (4.0 / (NOMEGA - 1))
        self.omega = [1 - pow_fast(10.0, log_mu[j]) for j in range(NOMEGA)]
        T0, T1, T2, T3, T4, T5, T6, T7 = 1000.0, 3600.0, 6000.0, 8000.0, 10000.0, 20000.0, 22000.0, 150000.0
        Te = [0.0] * NTEFF
        for i in range(NTEFF):
            if i == 0:
                Te[i] = T0
            if i == 1:
                Te[i] = T1
            if 2 <= i <= 6:
                Te[i] = T1 + i * ((T2 - T1) / 6)
            if i == 7:
                Te[i] = T2
            if 8 <= i <= 10:
                Te[i] = T2 + (i - 6) * ((T3 - T2) / 4)
            if i == 11:
                Te[i] = T3
            if 12 <= i <= 14:
                Te[i] = T3 + (i - 10) * ((T4 - T3) / 4)
            if i == 15:
                Te[i] = T4
            if i == 16:
                Te[i] = T5
            if 17 <= i <= 19:
                Te[i] = T5 + (i - 15) * ((T6 - T5) / 4)
            if i == 20:
                Te[i] = T6
            if i == 21:
                Te[i] = T7
        self.Teff = Te
        self.delta = [[fn_delta(self.omega[i], Te[j], xi) for j in range(NTEFF)] for i in range(NOMEGA)]
        self.alpha = [[[fn_alpha(self.omega[i], self.theta[j], Te[k]) for k in range(NTEFF)] for j in range(NTHETA)]
                      for i in range(NOMEGA)]

    def bilinear_delta(self, xr, yr):
        """interpolate_arrays::root_find_bilinear_vec (tools/interpolate.cpp:300-380) on delta(omega, Teff)"""
        x, y, f = self.omega, self.Teff, self.delta
        ihi, jhi, ilo, jlo = len(x) - 1, len(y) - 1, 0, 0
        while True:
            imid = ilo + int(math.floor((ihi - ilo) / 2.0))
            if x[imid] < xr:
                ilo = imid
            else:
                ihi = imid
            if not ihi - ilo > 1:
                break
        while True:
            jmid = jlo + int(math.floor((jhi - jlo) / 2.0))
            if y[jmid] < yr:
                jlo = jmid
            else:
                jhi = jmid
            if not jhi - jlo > 1:
                break
        xval = x[ihi] if xr > x[ihi] else (x[ilo] if xr < x[ilo] else xr)
        yval = y[jhi] if yr > y[jhi] else (y[jlo] if yr < y[jlo] else yr)
        result = (f[ilo][jlo] * (x[ihi] - xval) * (y[jhi] - yval)
                  + f[ihi][jlo] * (xval - x[ilo]) * (y[jhi] - yval)
                  + f[ilo][jhi] * (x[ihi] - xval) * (yval - y[jlo])
                  + f[ihi][jhi] * (xval - x[ilo]) * (yval - y[jlo]))
        result /= ((x[ihi] - x[ilo]) * (y[jhi] - y[jlo]))
        return result

    def trilinear_alpha(self, x, y, z):
        """interpolate_arrays::root_find_trilinear_vec (tools/interpolate.cpp:385-470) on alpha(omega, theta, Teff);
        ValueError where the reference calls rep.error (an index at 0) or reads past a vector"""
        xv, yv, zv, f = self.omega, self.theta, self.Teff, self.alpha

        def index(v, vec):
            i = 0
            while v > vec[i]:
                i += 1
                if i == len(vec):
                    raise ValueError("past the end")
            if i == 0:
                raise ValueError("out of range")
            return i
        xi, yi, zi = index(x, xv), index(y, yv), index(z, zv)
        x0, x1, y0, y1, z0, z1 = xv[xi - 1], xv[xi], yv[yi - 1], yv[yi], zv[zi - 1], zv[zi]
        dx = (x - x0) / (x1 - x0)
        dy = (y - y0) / (y1 - y0)
        dz = (z - z0) / (z1 - z0)
        f000 = f[xi - 1][yi - 1][zi - 1]
        f001 = f[xi - 1][yi - 1][zi]
        f010 = f[xi - 1][yi][zi - 1]
        f100 = f[xi][yi - 1][zi - 1]
        f110 = f[xi][yi][zi - 1]
        f011 = f[xi - 1][yi][zi]
        f101 = f[xi][yi - 1][zi]
        f111 = f[xi][yi][zi]
        c0 = f000
        c1 = f100 - f000
        c2 = f010 - f000
        c3 = f001 - f000
        c4 = f110 - f010 - f100 + f000
        c5 = f011 - f001 - f010 + f000
        c6 = f101 - f001 - f100 + f000
        c7 = f111 - f011 - f101 - f110 + f100 + f001 + f010 - f000
        return c0 + c1 * dx + c2 * dy + c3 * dz + c4 * dx * dy + c5 * dy * dz + c6 * dz * dx + c7 * dx * dy * dz

    def density_interp(self, omega, v_inf, mdot, radius, theta, Teff):
        """fn_density_interp (:386-455)"""
        omega = cmin(omega, 0.999)
        d = self.bilinear_delta(omega, Teff)
        a = self.trilinear_alpha(omega, theta, Teff)
        result = (mdot * a * d * pow_fast(1.0 - omega * math.sin(theta), self.xi))
        result /= (8.0 * PI * pow_fast(radius, 2.0) * fn_v_inf(omega, v_inf, theta))
        return result


_TABLES = {}


def tables(xi):
    if xi not in _TABLES:
        _TABLES[xi] = Tables(xi)
    return _TABLES[xi]


def theta_of(cfg, x, y, z):
    """stellar_wind::add_cell (stellar_wind_BC.cpp:286-318): 2-D atan(|R / z|), 3-D atan(|sqrt(x^2 + y^2) / z|)"""
    with np.errstate(all="ignore"):
        if cfg.ndim == 2:
            r = np.abs(y / x)
        else:
            r = np.abs(np.sqrt(x * x + y * y) / z)
    return np.array([math.atan(v) for v in r.tolist()])


def state(cfg, T, W, tracers, dist, theta, x, y, z):
    """set_wind_cell_reference_state (:464-691) for one cell, gamma = 5/3; W = dict(Mdot, Vinf, v_rot, vcrit, Tw,
    Rstar, Bstar, radius), cgs"""
    gamma = 5. / 3.
    p = [0.0] * cfg.nvar
    set_rho = True
    if dist < 0.75 * W["radius"] and cfg.ndim > 1:                     # :477-481
        p[0] = p[1] = 1.0e-31
        set_rho = False
    om = cmin(0.9999, W["v_rot"] / W["vcrit"])
    if set_rho:                                                         # :491-510
        p[0] = T.density_interp(om, W["Vinf"], W["Mdot"], dist, theta, W["Tw"])
        p[1] = W["Tw"] * wr.KB / wr.M_P
        p[1] *= pow_fast(T.density_interp(om, W["Vinf"], W["Mdot"], W["Rstar"], theta, W["Tw"]), 1.0 - gamma)
        p[1] *= pow_fast(p[0], gamma)
    Vinf = fn_v_inf(om, W["Vinf"], theta)                              # :513-514
    if cfg.ndim == 2:                                                   # :553-557
        p[2] = Vinf * x / dist
        p[3] = Vinf * y / dist
        p[4] = 0.0
    else:                                                               # :559-572
        p[2] = Vinf * x / dist
        p[3] = Vinf * y / dist
        p[4] = Vinf * z / dist
        xf = -W["v_rot"] * W["Rstar"] * y / pow_fast(dist, 2)
        yf = W["v_rot"] * W["Rstar"] * x / pow_fast(dist, 2)
        p[2] += xf
        p[3] += yf
    if cfg.eqntype in (abi.EQMHD, abi.EQGLM):                          # :584-638
        B_s = W["Bstar"] / math.sqrt(4.0 * math.pi)
        D_s = W["Rstar"] / dist
        D_2 = D_s * D_s
        bbs = (W["v_rot"] / Vinf) * B_s * D_s
        if cfg.ndim == 2:
            p[5] = B_s * D_2 * abs(x) / dist
            p[6] = B_s * D_2 / dist
            p[6] = y * p[6] if x > 0.0 else -y * p[6]
            bbs = bbs * y / dist
            p[7] = -bbs if x > 0.0 else bbs
        else:
            p[5] = B_s * D_2 / dist
            p[5] = x * p[5] if z > 0.0 else -x * p[5]
            p[6] = B_s * D_2 / dist
            p[6] = y * p[6] if z > 0.0 else -y * p[6]
            p[7] = B_s * D_2 * abs(z) / dist
            bbs *= math.sqrt(x * x + y * y) / dist
            bbs = -bbs if z > 0.0 else bbs
            p[5] += - bbs * y / dist
            p[6] += bbs * x / dist
        if cfg.eqntype == abi.EQGLM:                                    # :639-641
            p[8] = 0.0
    ftr = cfg.nvar - cfg.ntracer
    for v in range(cfg.ntracer):                                        # :657-658
        p[ftr + v] = tracers[v]
    Tmin = cfg.min_temp                                                 # :661-675
    if cfg.cooling:
        if p[1] * wr.MU_TOT_OVER_KB / p[0] < Tmin:
            p[1] = p[0] * Tmin / wr.MU_TOT_OVER_KB
    else:
        p[1] = cmax(p[1], Tmin * p[0] * wr.KB * 0.78625 / wr.M_P)
    return p


class Source:
    """One rotating source: add_evolving_source (:700-827), add_rotating_source (:836-932), update_source
    (:941-1019) and stellar_wind_evolution::set_cell_values (stellar_wind_BC.cpp:1334-1372).  `src` is a
    pion_amd.wind.WindSource of type ANGLE."""

    def __init__(self, src, ntracer):
        self.src = src
        self.T = tables(src.xi)
        ev = src.evolution
        t = list(ev.time)
        self.tstart, self.tfinish = t[0], t[-1]
        self.t_next = max(self.tstart, src.t_now)
        self.tr = list(src.tracers) + [0.0] * (ntracer - len(src.tracers))
        x = {}
        tn = src.t_now
        if ((tn + src.update_freq) > self.tstart or wr.equalD(self.tstart, tn)) and tn < self.tfinish:
            self.active = True
            Tw, mdot, vinf, vrot, vcrt, rstar = (wr.root_find_linear_vec(t, getattr(ev, k), tn)
                                                 for k in ("Teff", "Mdot", "vinf", "vrot", "vcrit", "R"))
            x = {e: wr.root_find_linear_vec(t, ev.cols[e], tn) for e in ev.cols if e.startswith("X_")}
        else:
            self.active = False
            mdot, vinf, vrot, Tw, vcrt, rstar = -100.0, -100.0, -100.0, -100.0, 0.0, 0.0
        for v, e in enumerate(src.elements):
            if e is not None:
                self.tr[v] = x.get(e, 0.0)
        self.W = dict(Mdot=mdot, Vinf=vinf, v_rot=vrot, vcrit=vcrt, Tw=cmin(Tw, self.T.Teff[-1]), Rstar=rstar,
                      Bstar=src.Bstar, radius=src.radius)

    def update(self, t_now):
        """set_cell_values at t_now: True if the source writes its cells"""
        if t_now >= self.t_next:
            ev = self.src.evolution
            t = list(ev.time)
            self.active = True
            self.t_next = min(t_now, self.tfinish)
            f = {k: wr.root_find_linear_vec(t, getattr(ev, k), t_now)
                 for k in ("Teff", "Mdot", "vinf", "vrot", "vcrit", "R")}
            self.W.update(Mdot=f["Mdot"], Vinf=f["vinf"], v_rot=f["vrot"], vcrit=f["vcrit"],
                          Tw=cmin(f["Teff"], self.T.Teff[-1]), Rstar=f["R"])
            for v, e in enumerate(self.src.elements):
                if e is not None:
                    self.tr[v] = wr.root_find_linear_vec(t, ev.cols[e], t_now)
        return self.active

    def cells(self, cfg):
        """(idx, dist, theta, x, y, z) of the member cells, in cell-id order"""
        idx, d, x, y, z = wr.members(cfg, self.src.pos, self.src.radius)
        return idx, d, theta_of(cfg, x, y, z), x, y, z

    def states(self, cfg):
        idx, d, th, x, y, z = self.cells(cfg)
        st = np.array([state(cfg, self.T, self.W, self.tr, float(d[k]), float(th[k]), float(x[k]), float(y[k]),
                             float(z[k])) for k in range(idx.size)]).reshape(idx.size, cfg.nvar)
        return idx, st
