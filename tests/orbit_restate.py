"""Restatement of the reference's orbital motion of stellar-wind sources (BC_update_STWIND,
boundaries/stellar_wind_boundaries.cpp:253-352; stellar_wind::remove_cells and add_cell, grid/stellar_wind_BC.cpp:349-367
and :255-283), for the orbit tests.  The position keeps the reference's expressions in their order, in Python floats
(IEEE double, libm's sin/cos/atan/acos/sqrt); 0/0 and the square root of a negative number give NaN, as in C++."""
import math

import numpy as np

import wind_restate as wr
from pion_amd import abi

PI, YEAR = 3.14159265358979324, 3.1558150e7   # constants.h:45,107
ISGD, ISBD, ISDOMAIN, TIMESTEP, ISLEAF = 1, 2, 4, 8, 16


def _div(a, b):
    with np.errstate(all="ignore"):
        return float(np.float64(a) / np.float64(b))


def _sqrt(x):
    return math.sqrt(x) if x >= 0.0 else (x if x != x else float("nan"))


def orbit_position(src, ndim, simtime):
    """stellar_wind_boundaries.cpp:294-314 for WindSource `src` (src.orbit = (f, px, py, P_years)); 3 floats"""
    f, px, py, P = src.orbit
    pos = [src.pos[a] if a < ndim else 0.0 for a in range(3)]
    if P == 0:
        return tuple(pos)
    cos_a = _div(-1 * px, abs(px)) * math.cos(math.atan(_div(py, px)))
    sin_a = math.sin(_div(-1 * py, abs(py)) * math.acos(cos_a))
    a = _sqrt(px * px + py * py) * f
    e = _div(a * (f - 1), f)
    b = _sqrt(a * a - e * e)
    sin_t = math.sin(_div(2 * PI * simtime, P * YEAR))
    cos_t = math.cos(_div(2 * PI * simtime, P * YEAR))
    pos[0] = src.pos[0] - a * cos_a + cos_a * a * cos_t - sin_a * b * sin_t
    pos[1] = src.pos[1] - a * sin_a + sin_a * a * cos_t + cos_a * b * sin_t
    return tuple(pos)


def initial_flags(cfg):
    """the device's flags at create (pion_gpu_create; uniform_grid.cpp:343-356): on-grid cells are grid data and
    domain, ghost cells boundary data; all leaf cells that enter the time step"""
    nga = abi.ng_all(cfg)
    c = np.arange(int(np.prod(nga)))
    i = [c % nga[0] - cfg.nbc, (c // nga[0]) % nga[1] - cfg.nbc, c // (nga[0] * nga[1]) - cfg.nbc]
    on = np.ones(c.size, dtype=bool)
    for a in range(cfg.ndim):
        on &= (i[a] >= 0) & (i[a] < cfg.ng[a])
    return np.where(on, ISLEAF | TIMESTEP | ISGD | ISDOMAIN, ISLEAF | TIMESTEP | ISBD).astype(np.uint8)


def add_cells(flags, idx):
    """add_cell (stellar_wind_BC.cpp:277-278): isbd = true, isdomain = false"""
    flags[idx] = (flags[idx] | ISBD) & ~np.uint8(ISDOMAIN)


def remove_cells(flags, idx):
    """remove_cells (stellar_wind_BC.cpp:360-362): isbd = false, isdomain = true, timestep = true"""
    flags[idx] = (flags[idx] & ~np.uint8(ISBD)) | ISDOMAIN | TIMESTEP


class Orbits:
    """The sources of one grid as BC_update_STWIND moves them: positions, member lists and the whole flag array"""

    def __init__(self, cfg, srcs):
        self.cfg, self.srcs = cfg, srcs
        self.flags = initial_flags(cfg)
        self.pos = [tuple(s.pos[a] if a < cfg.ndim else 0.0 for a in range(3)) for s in srcs]
        self.idx = []
        for s, p in zip(srcs, self.pos):
            i = self.members(p, s.radius)
            add_cells(self.flags, i)
            self.idx.append(i)

    def members(self, pos, radius):
        with np.errstate(all="ignore"):
            return wr.members(self.cfg, pos, radius)[0]

    def moving(self, k):
        return self.srcs[k].orbit[3] != 0

    def update(self, simtime):
        """the moves of one boundary update, in id order"""
        for k, s in enumerate(self.srcs):
            if not self.moving(k):
                continue
            remove_cells(self.flags, self.members(self.pos[k], s.radius))
            self.pos[k] = orbit_position(s, self.cfg.ndim, simtime)
            self.idx[k] = self.members(self.pos[k], s.radius)
            add_cells(self.flags, self.idx[k])

    def states(self, k, W, tracers):
        """reference states of source k's cells at its current position (wind_restate.states)"""
        with np.errstate(all="ignore"):
            idx, d, x, y, z = wr.members(self.cfg, self.pos[k], self.srcs[k].radius)
        return idx, wr.states(self.cfg, d, x, y, z, W, tracers)
