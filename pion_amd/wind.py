"""Stellar-wind sources the device builds and updates itself (include/pion_gpu.h: pion_gpu_add_wind_source).

    src = wind.WindSource(pos=(0, 0, 0), radius=1.5e17, mdot=1e-7, vinf=1500.0, Tw=3e4, Rstar=6.96e11,
                          tracers=[1.0])
    sim.add_wind_source(src)               # pion_amd.lib.GpuSim; before the first update_bcs
    idx, states = sim.get_wind_cells(0)

Constant winds take Msun/yr and km/s (stellar_wind::add_source, grid/stellar_wind_BC.cpp:166-172); an evolving wind
(type EVOLVING) takes a table read by read_wind_evolution, in cgs, with its times already offset and scaled.  A
rotating star (type ANGLE, the LGM99 wind of grid/stellar_wind_angle.cpp) takes such a table too, its vcrit column
and `xi`, and is added with GpuSim.add_rotating_wind_source.
"""
import ctypes as C
import os

import numpy as np

from . import abi

CONSTANT, EVOLVING, ANGLE = 0, 1, 2   # WINDTYPE_CONSTANT, _EVOLVING, _ANGLE (grid/stellar_wind_BC.h:41-43)
ELEMENTS = ("X_H", "X_He", "X_C", "X_N", "X_O", "X_Z", "X_D")   # set_element_indices (:992-1024)
MAX_SOURCES = 8

_dp = C.POINTER(C.c_double)
NCOL = 16   # PION_WND_NCOL of include/pion_host.h
COLUMNS = ("time", "M", "L", "Teff", "Mdot", "vrot", "vcrit", "vinf") + ELEMENTS + ("R",)


class PionGpuWindSource(C.Structure):
    """ctypes mirror of pion_gpu_wind_source (include/pion_gpu.h)"""
    _fields_ = [
        ("pos", C.c_double * 3), ("radius", C.c_double), ("type", C.c_int),
        ("mdot", C.c_double), ("vinf", C.c_double), ("vrot", C.c_double),
        ("Tw", C.c_double), ("Rstar", C.c_double), ("Bstar", C.c_double),
        ("tracers", C.c_double * abi.PION_MAX_NVAR),
        ("npt", C.c_int),
        ("evo_time", _dp), ("evo_Teff", _dp), ("evo_Mdot", _dp), ("evo_vrot", _dp), ("evo_vinf", _dp),
        ("evo_R", _dp), ("evo_X", _dp * 7),
        ("evo_tracer_elem", C.c_int * abi.PION_MAX_NVAR),
        ("t_now", C.c_double), ("update_freq", C.c_double),
        ("orbit_ecc_fac", C.c_double), ("orbit_periastron", C.c_double * 2), ("orbit_period", C.c_double),
    ]


class WindEvolution:
    """A .wnd.txt table (stellar_wind_evolution::read_evolution_file): one numpy array per column, cgs,
    time = (t + time_offset) / t_scalefac, R = sqrt(L / (4 pi sigma Teff^4))."""

    def __init__(self, cols):
        self.cols = cols
        for k, v in cols.items():
            setattr(self, k, v)
        self.npt = cols["time"].size


def _host_lib():
    from . import lib
    lib.load_library()
    path = os.path.join(os.path.dirname(abi.library_path()), "..", "host", "libpion_host.so")
    C.CDLL(abi.library_path(), mode=C.RTLD_GLOBAL)
    h = C.CDLL(os.path.normpath(path))
    h.pion_host_read_wind_evolution.argtypes = [C.c_char_p, C.c_double, C.c_double, C.c_long, _dp]
    h.pion_host_read_wind_evolution.restype = C.c_long
    return h


def read_wind_evolution(path, time_offset=0.0, t_scalefac=1.0):
    """pion_host_read_wind_evolution (libpion_host.so) on `path`; returns a WindEvolution."""
    h = _host_lib()
    p = os.fsencode(path)
    n = h.pion_host_read_wind_evolution(p, time_offset, t_scalefac, 0, None)
    if n < 0:
        raise OSError("cannot read wind evolution file %s (rc %d)" % (path, n))
    tab = np.zeros((NCOL, max(n, 1)))
    rc = h.pion_host_read_wind_evolution(p, time_offset, t_scalefac, tab.shape[1], tab.ctypes.data_as(_dp))
    if rc != n:
        raise OSError("reading %s: rc %d" % (path, rc))
    return WindEvolution({c: tab[i, :n].copy() for i, c in enumerate(COLUMNS)})


class WindSource:
    """One SWP wind source.  Constant: mdot [Msun/yr], vinf, vrot [km/s], Tw [K], Rstar [cm], Bstar [G].
    Evolving: `evolution` (a WindEvolution), `elements` = per tracer an element name of ELEMENTS or None (the
    constant tracer value), `t_now` = simulation time at set-up, `update_freq` (already scaled).  `vinf` of an
    evolving source is only the parameter-file value the first-step limit uses (0: none).
    `orbit` = (ecentricity_fac, periastron_x [cm], periastron_y [cm], period [yr]) moves the source on the
    reference's ellipse around `pos` at every boundary update (2-D and 3-D Cartesian grids); None or a zero period:
    the source stays at `pos`.
    Rotating (type ANGLE): as evolving, the table's vcrit column included, and `xi` (WIND_i_xi), the exponent of the
    equatorial density enhancement."""

    def __init__(self, pos, radius, mdot=0.0, vinf=0.0, vrot=0.0, Tw=0.0, Rstar=0.0, Bstar=0.0, tracers=(),
                 type=CONSTANT, evolution=None, elements=None, t_now=0.0, update_freq=0.0, orbit=None, xi=0.0):
        self.pos = tuple(pos) + (0.0,) * (3 - len(pos))
        self.radius = radius
        self.mdot, self.vinf, self.vrot = mdot, vinf, vrot
        self.Tw, self.Rstar, self.Bstar = Tw, Rstar, Bstar
        self.tracers = list(tracers)
        self.type = type
        self.evolution = evolution
        self.elements = list(elements) if elements is not None else [None] * len(self.tracers)
        self.t_now, self.update_freq = t_now, update_freq
        self.xi = float(xi)
        self.orbit = tuple(float(v) for v in orbit) if orbit is not None else (0.0, 0.0, 0.0, 0.0)
        if len(self.orbit) != 4:
            raise ValueError("orbit = (ecentricity_fac, periastron_x, periastron_y, period_years)")

    def to_c(self):
        """(PionGpuWindSource, arrays to keep alive while the struct is used)"""
        s = PionGpuWindSource()
        for a in range(3):
            s.pos[a] = self.pos[a]
        s.radius, s.type = self.radius, self.type
        s.mdot, s.vinf, s.vrot = self.mdot, self.vinf, self.vrot
        s.Tw, s.Rstar, s.Bstar = self.Tw, self.Rstar, self.Bstar
        for v, t in enumerate(self.tracers):
            s.tracers[v] = t
        for v in range(abi.PION_MAX_NVAR):
            s.evo_tracer_elem[v] = -1
        keep = []
        if self.evolution is not None:
            ev = self.evolution
            s.npt = ev.npt

            def arr(x):
                a = np.ascontiguousarray(x, dtype=np.float64)
                keep.append(a)
                return a.ctypes.data_as(_dp)
            s.evo_time, s.evo_Teff, s.evo_Mdot = arr(ev.time), arr(ev.Teff), arr(ev.Mdot)
            s.evo_vrot, s.evo_vinf, s.evo_R = arr(ev.vrot), arr(ev.vinf), arr(ev.R)
            for e, name in enumerate(ELEMENTS):
                s.evo_X[e] = arr(ev.cols[name])
            for v, name in enumerate(self.elements):
                s.evo_tracer_elem[v] = -1 if name is None else ELEMENTS.index(name)
            keep.append(np.ascontiguousarray(ev.vcrit, dtype=np.float64))   # keep[-1]: pion_gpu_add_rotating_...
        s.t_now, s.update_freq = self.t_now, self.update_freq
        s.orbit_ecc_fac, s.orbit_periastron[0], s.orbit_periastron[1], s.orbit_period = self.orbit
        return s, keep


def first_step_dt_limit(cfg, sources, limit=None):
    """calc_dynamics_dt's first-step limit for wind sources, 0.1 CFL dx / (Vinf 1e5) per source
    (calc_timestep.cpp:318-322), combined by min with `limit` (None: none); None when nothing limits."""
    for s in sources:
        lim = 0.1 * cfg.cfl * cfg.dx / (s.vinf * 1.0e5) if s.vinf != 0.0 else float("inf")
        limit = lim if limit is None else min(limit, lim)
    return limit


def orbit_position(src, ndim, simtime):
    """pion_gpu_wind_orbit_position (host code of libpion_gpu.so, no device needed): the position of WindSource
    `src` on its orbit at `simtime` on a grid of `ndim` (2 or 3) dimensions, as a tuple of 3 floats."""
    from . import lib
    L = lib.load_library()
    st, keep = src.to_c()
    out = (C.c_double * 3)()   # PION_MAX_DIM
    rc = L.pion_gpu_wind_orbit_position(C.byref(st), int(ndim), float(simtime), out)
    del keep
    if rc != 0:
        raise ValueError("pion_gpu_wind_orbit_position: rc %d" % rc)
    return tuple(out[:3])


def angle_tables(xi):
    """pion_gpu_wind_angle_tables (host code of libpion_gpu.so, no device needed): stellar_wind_angle::setup_tables
    for `xi`.  Returns dict(theta[25], omega[25], Teff[22], delta[25, 22], alpha[25, 25, 22]) of numpy arrays."""
    from . import lib
    L = lib.load_library()
    out = dict(theta=np.zeros(25), omega=np.zeros(25), Teff=np.zeros(22), delta=np.zeros((25, 22)),
               alpha=np.zeros((25, 25, 22)))
    rc = L.pion_gpu_wind_angle_tables(float(xi), *(out[k].ctypes.data_as(_dp)
                                                   for k in ("theta", "omega", "Teff", "delta", "alpha")))
    if rc != 0:
        raise ValueError("pion_gpu_wind_angle_tables: rc %d" % rc)
    return out
