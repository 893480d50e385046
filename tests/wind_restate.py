"""numpy restatement of the reference's stellar-wind source code, for the wind-source tests.

The reference's wind code cannot be built here (grid/stellar_wind_BC.cpp includes GSL through tools/interpolate.h),
so parity of the device's wind sources rests on this restatement -- the standard problems.wind_cells has had.  Every
expression keeps the reference's operation order and cites its line (source/ of the PION tree)."""
import math

import numpy as np

from pion_amd import abi
from pion_amd.problems import cell_centres

KB, M_P, PI = 1.38064852e-16, 1.672621898e-24, 3.14159265358979324   # constants.h:45,53,64
MSUN, YEAR = 1.9891e33, 3.1558150e7                                  # constants.h:107,113
MU_TOT_OVER_KB = 0.609 * M_P / KB                                    # mp_only_cooling.cpp:81-95


def equalD(a, b):
    """constants::equalD (constants.cpp:48-68)"""
    if a == b:
        return True
    if abs(a) + abs(b) < 1.0e-100:
        return True
    return abs(a - b) / (abs(a) + abs(b) + 1.0e-100) < 1.0e-12


def root_find_linear_vec(xarr, yarr, xreq):
    """interpolate_arrays::root_find_linear_vec (tools/interpolate.cpp:121-161), as written"""
    ihi, ilo = len(xarr) - 1, 0
    while True:
        imid = ilo + int(math.floor((ihi - ilo) / 2.0))
        if xarr[imid] < xreq:
            ilo = imid
        else:
            ihi = imid
        if not ihi - ilo > 1:
            break
    if xreq > xarr[ihi]:
        xval = xarr[ihi]
    elif xreq < xarr[ilo]:
        xval = xarr[ilo]
    else:
        xval = xreq
    with np.errstate(all="ignore"):   # IEEE arithmetic: 0/0 is NaN, as in C++
        y0, y1 = np.float64(yarr[ilo]), np.float64(yarr[ihi])
        return float(y0 + (y1 - y0) * (np.float64(xval) - xarr[ilo]) / (np.float64(xarr[ihi]) - xarr[ilo]))


def geometry(cfg, pos):
    """distance_vertex2cell and difference_vertex2cell of every cell (ghosts included), flattened in cell-id order:
    (dist, x, y, z).  UniformGrid (uniform_grid.cpp:1432-1461), uniform_grid_cyl (:1764-1820), uniform_grid_sph
    (:2085-2120)."""
    xc, yc, zc = cell_centres(cfg)
    Z, Y, X = np.meshgrid(zc, yc, xc, indexing="ij")
    X, Y, Z = X.reshape(-1), Y.reshape(-1), Z.reshape(-1)
    zero = np.zeros_like(X)
    if cfg.coord_sys == 2:
        Rc = Y + cfg.dx * cfg.dx / 12. / Y                       # VectorOps_Cyl::R_com (VectorOps.h:414-418)
        d = 0.0 + (pos[0] - X) * (pos[0] - X)
        d = d + (pos[1] - Rc) * (pos[1] - Rc)
        return np.sqrt(d), X - pos[0], Rc - pos[1], zero
    if cfg.coord_sys == 3:
        delta2 = cfg.dx / X                                      # VectorOps_Sph::R_com (VectorOps_spherical.h:188-196)
        delta2 = delta2 * delta2
        Rc = X * (1.0 + 0.25 * delta2) / (1.0 + delta2 / 12.0)
        return np.abs(pos[0] - Rc), Rc - pos[0], zero, zero
    t = pos[0] - X
    temp = 0.0 + t * t                                           # pow(v - x, 2.0)
    x, y, z = X - pos[0], zero, zero
    if cfg.ndim > 1:
        t = pos[1] - Y
        temp = temp + t * t
        y = Y - pos[1]
    if cfg.ndim > 2:
        t = pos[2] - Z
        temp = temp + t * t
        z = Z - pos[2]
    return np.sqrt(temp), x, y, z


def members(cfg, pos, radius):
    """BC_assign_STWIND_add_cells2src (stellar_wind_boundaries.cpp:200-240): (idx, dist, x, y, z) of the cells with
    dist <= radius, in cell-id order"""
    d, x, y, z = geometry(cfg, pos)
    idx = np.flatnonzero(d <= radius)
    return idx, d[idx], x[idx], y[idx], z[idx]


def states(cfg, dist, x, y, z, W, tracers):
    """stellar_wind::set_wind_cell_reference_state (stellar_wind_BC.cpp:375-600) with gamma = 5/3 (:331) for
    cells (dist, x, y, z); W = dict(Mdot, Vinf, v_rot, Tw, Rstar, Bstar, radius) in cgs.  Returns [n, nvar]."""
    with np.errstate(all="ignore"):
        return _states(cfg, dist, x, y, z, W, tracers)


def _states(cfg, dist, x, y, z, W, tracers):
    gamma = 5. / 3.
    n = dist.size
    p = np.zeros((cfg.nvar, n))
    ndim = cfg.ndim
    Mdot, Vinf, v_rot, Tw, Rstar, Bstar = (W[k] for k in ("Mdot", "Vinf", "v_rot", "Tw", "Rstar", "Bstar"))
    inner = (dist < 0.75 * W["radius"]) & (ndim > 1)                          # :388-393
    if ndim == 2 and cfg.coord_sys == 1:                                      # :402-423 slab symmetry
        p[0] = Mdot / (Vinf * 2.0 * PI * dist)
        p[1] = KB * Tw / M_P
        p[1] = p[1] * math.exp((gamma - 1.0) * math.log(2.0 * PI * Rstar * Vinf / Mdot))
        p[1] = p[1] * np.exp((gamma) * np.log(p[0]))
    else:                                                                     # :425-442
        ro = 1.0 / (dist)
        ro = ro * ro
        ro = ro * (Mdot / (Vinf * 4.0 * PI))
        pg = KB * Tw / M_P
        pg = pg * math.exp((gamma - 1.0) * math.log(4.0 * PI * Rstar * Rstar * Vinf / Mdot))
        pg = pg * np.exp((gamma) * np.log(ro))
        p[0] = np.where(inner, 1.0e-31, ro)
        p[1] = np.where(inner, 1.0e-31, pg)
    pf = np.exp(2.0 * np.log(dist))                                           # pconst.pow_fast(dist, 2)
    if ndim == 1:                                                             # :473-477
        p[2] = Vinf * x / dist
    elif ndim == 2:                                                           # :479-484
        p[2] = Vinf * x / dist
        p[3] = Vinf * y / dist
        p[4] = v_rot * Rstar * y / pf
    else:                                                                     # :486-494
        p[2] = Vinf * x / dist
        p[3] = Vinf * y / dist
        p[4] = Vinf * z / dist
        p[2] = p[2] + -v_rot * Rstar * y / pf
        p[3] = p[3] + v_rot * Rstar * x / pf
    if cfg.eqntype in (abi.EQMHD, abi.EQGLM):                                 # :502-564
        B_s = Bstar / math.sqrt(4.0 * PI)
        D_s = Rstar / dist
        D_2 = D_s * D_s
        beta = (v_rot / Vinf) * B_s * D_s
        if ndim == 2:
            p[5] = B_s * D_2 * np.abs(x) / dist
            by = B_s * D_2 / dist
            p[6] = np.where(x > 0.0, y * by, -y * by)
            beta = beta * y / dist
            p[7] = np.where(x > 0.0, -beta, beta)
        else:
            bx = B_s * D_2 / dist
            bx = np.where(z > 0.0, x * bx, -x * bx)
            by = B_s * D_2 / dist
            by = np.where(z > 0.0, y * by, -y * by)
            p[7] = B_s * D_2 * np.abs(z) / dist
            beta = beta * (np.sqrt(x * x + y * y) / dist)
            beta = np.where(z > 0.0, -beta, beta)
            p[5] = bx + -beta * y / dist
            p[6] = by + beta * x / dist
        if cfg.eqntype == abi.EQGLM:
            p[8] = 0.0
    ftr = cfg.nvar - cfg.ntracer
    for v in range(cfg.ntracer):
        p[ftr + v] = tracers[v]
    Tmin = cfg.min_temp                                                       # :578-590
    if cfg.cooling:
        T = p[1] * MU_TOT_OVER_KB / p[0]                                      # mp_only_cooling.cpp:274-280
        p[1] = np.where(T < Tmin, p[0] * Tmin / MU_TOT_OVER_KB, p[1])         # Set_Temp, :244-266
    else:
        fl = Tmin * p[0] * KB * 0.78625 / M_P
        p[1] = np.where(p[1] < fl, fl, p[1])
    return p.T.copy()


class Source:
    """One source's parameters and activity as stellar_wind(_evolution) keeps them: add_source (:120-217),
    add_evolving_source (:1109-1245), update_source (:1250-1330), set_cell_values (:1334-1372)."""

    def __init__(self, src, ntracer):
        self.src = src
        self.tr = list(src.tracers) + [0.0] * (ntracer - len(src.tracers))
        mdot, vinf, vrot, Tw, Rstar = src.mdot, src.vinf, src.vrot, src.Tw, src.Rstar
        self.active, self.t_next = True, 1.0e99
        if src.type == 1:
            ev = src.evolution
            t = list(ev.time)
            self.tstart, self.tfinish = t[0], t[-1]
            self.t_next = max(self.tstart, src.t_now)
            x = {}
            if ((src.t_now + src.update_freq) > self.tstart or equalD(self.tstart, src.t_now)) \
                    and src.t_now < self.tfinish:
                Tw, mdot, vinf, vrot, Rstar = (root_find_linear_vec(t, getattr(ev, k), src.t_now)
                                               for k in ("Teff", "Mdot", "vinf", "vrot", "R"))
                x = {e: root_find_linear_vec(t, ev.cols[e], src.t_now) for e in ev.cols if e.startswith("X_")}
            else:
                self.active = False
                mdot, vinf, Tw, vrot, Rstar = -100.0, -100.0, -100.0, 0.0, 0.0
            for v, e in enumerate(src.elements):
                if e is not None:
                    self.tr[v] = x.get(e, 0.0)
        self.W = dict(Mdot=mdot * MSUN / YEAR, Vinf=vinf * 1.0e5, v_rot=vrot * 1.0e5, Tw=Tw, Rstar=Rstar,
                      Bstar=src.Bstar, radius=src.radius)

    def update(self, t_now):
        """set_cell_values at t_now: True if the source writes its cells"""
        src = self.src
        if src.type == 1 and t_now >= self.t_next:
            ev = src.evolution
            t = list(ev.time)
            self.active = True
            self.t_next = min(t_now, self.tfinish)
            self.W.update(Tw=root_find_linear_vec(t, ev.Teff, t_now), Mdot=root_find_linear_vec(t, ev.Mdot, t_now),
                          v_rot=root_find_linear_vec(t, ev.vrot, t_now), Vinf=root_find_linear_vec(t, ev.vinf, t_now),
                          Rstar=root_find_linear_vec(t, ev.R, t_now))
            for v, e in enumerate(src.elements):
                if e is not None:
                    self.tr[v] = root_find_linear_vec(t, ev.cols[e], t_now)
        return self.active

    def states(self, cfg):
        idx, d, x, y, z = members(cfg, self.src.pos, self.src.radius)
        return idx, states(cfg, d, x, y, z, self.W, self.tr)
