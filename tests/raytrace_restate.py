"""A scalar restatement of the reference's short-characteristics tracer (source/raytracing/raytracer_SC.cpp; the line
numbers below are that file's), for the tests of the ray-traced column densities.  It visits the cells in the
reference's order -- octant by octant, then z, y, x outwards from the source (trace_octant / trace_plane /
trace_column, 2005-2094) -- on integer positions (cell size 2, cell centres odd, vertices even), and shares no code
with pion_amd/csrc/dev_raytrace.h.  Plain Python floats: IEEE doubles, every operation rounded once, nothing fused."""
import math

import numpy as np

OPACITY_TOTAL, OPACITY_MINUS, OPACITY_TRACER = 1, 2, 3


def equalD(a, b):
    """constants::equalD (constants.cpp:48-69)"""
    if a == b:
        return True
    if abs(a) + abs(b) < 1.0e-100:
        return True
    return abs(a - b) / (abs(a) + abs(b) + 1.0e-100) < 1.0e-12


def centre_source_on_cell(pos, xmin, dx):
    """centre_source_on_cell (1934-1996) for one axis"""
    dist = pos - xmin
    x = int(dist / dx)   # static_cast<int>: towards zero
    dist -= x * dx
    dist /= dx
    if not equalD(dist, 0.0):
        assert abs(dist) <= 1.0
        if equalD(dist, 0.5):
            if dist > 0:
                pos -= dist * dx
            else:
                pos -= (1.0 + dist) * dx
        elif dist > 0.0 and dist > 0.5:
            pos += (1.0 - dist) * dx
        elif dist > 0.0 and dist <= 0.5:
            pos -= dist * dx
        elif dist < 0.0 and dist <= -0.5:
            pos -= (1.0 + dist) * dx
        elif dist < 0.0 and dist > -0.5:
            pos -= dist * dx
    return pos


def source_vertex(pos, xmin, dx, ndim):
    """find_source_cell's centring (1902-1907) and get_ipos_vec (cell_interface.cpp:553-571): the moved position and
    its integer position, per axis"""
    moved, ipos = [], []
    for a in range(ndim):
        p = centre_source_on_cell(pos[a], xmin[a], dx)
        moved.append(p)
        ipos.append(int((1.0 + 1.0e-12) * ((p - xmin[a]) / (0.5 * dx))))
    return moved, ipos


def interpolate_2D(taumin, delta0, tau1, tau2):
    w1 = (1. - delta0) / max(taumin, tau1)
    w2 = delta0 / max(taumin, tau2)
    s = w1 + w2
    w1 /= s
    w2 /= s
    return w1 * tau1 + w2 * tau2


def interpolate_3D(taumin, delta0, delta1, tau1, tau2, tau3, tau4):
    w1 = (1. - delta0) * (1. - delta1) / max(taumin, tau1)
    w2 = delta0 * (1. - delta1) / max(taumin, tau2)
    w3 = (1. - delta0) * delta1 / max(taumin, tau3)
    w4 = delta0 * delta1 / max(taumin, tau4)
    s = w1 + w2 + w3 + w4
    w1 /= s
    w2 /= s
    w3 /= s
    w4 /= s
    return w1 * tau1 + w2 * tau2 + w3 * tau3 + w4 * tau4


class _Grid:
    """the on-grid cells, indexed (ix, iy, iz); NextPt gives None off the grid -- a boundary cell of the reference holds
    column 0 (ProcessCell 887-898), which is what the null-pointer branches give as well"""

    def __init__(self, ng, ndim):
        self.ng, self.ndim = list(ng) + [1] * (3 - len(ng)), ndim
        self.col = np.zeros((self.ng[2], self.ng[1], self.ng[0]))
        self.dcol = np.zeros_like(self.col)

    def on(self, c):
        return all(0 <= c[a] < self.ng[a] for a in range(3))

    def next(self, c, axis, step):
        if c is None:
            return None
        n = list(c)
        n[axis] += step
        return tuple(n) if self.on(n) else None

    def get_col(self, c):
        return float(self.col[c[2], c[1], c[0]])


def _col2cell_2d(G, taumin, c, entry, perp, delta):
    """col2cell_2d (2495-2533); entry, perp: (axis, step)"""
    c1 = G.next(c, *entry)
    if c1 is None:
        col1 = col2 = 0.0
    else:
        c2 = G.next(c1, *perp)
        col1 = G.get_col(c1)
        col2 = 0.0 if c2 is None else G.get_col(c2)
    return interpolate_2D(taumin, delta, col1, col2)


def _cell_cols_2d(G, ipos, taumin, dx, c):
    """cell_cols_2d (2132-2278): (column to the cell, ds)"""
    diffx = abs(2 * c[0] + 1 - ipos[0])
    diffy = abs(2 * c[1] + 1 - ipos[1])
    srcdir = [(a, -1 if 2 * c[a] + 1 > ipos[a] else 1) for a in range(2)]
    if diffx >= diffy:
        entry, perp = srcdir[0], srcdir[1]
        delta = float(diffy) / float(diffx)
        mindiff, maxdiff = diffy, diffx
    else:
        entry, perp = srcdir[1], srcdir[0]
        delta = float(diffx) / float(diffy)
        mindiff, maxdiff = diffx, diffy
    ds = dx * math.sqrt(1.0 + delta * delta)
    idx = 2.0
    idxo2 = 0.5 * idx
    if mindiff < idx and maxdiff < idx:
        return 0.0, ds
    if mindiff < idx:
        ngb = G.next(c, *entry)
        Nc = G.get_col(ngb) if ngb is not None else 0.0
        Nc = max(Nc, 0.0)
        if maxdiff < 10 * idx:
            maxd = float(maxdiff)
            maxmin2 = maxd - idx
            Nc *= math.sqrt((maxd * maxd + idxo2 * idxo2) / (maxmin2 * maxmin2 + idxo2 * idxo2)) * maxmin2 / maxd
        return Nc, ds
    return _col2cell_2d(G, taumin, c, entry, perp, delta), ds


def _cell_cols_3d(G, ipos, taumin, dx, c):
    """cell_cols_3d (2287-2486): (column to the cell, ds)"""
    d = [abs(2 * c[a] + 1 - ipos[a]) for a in range(3)]
    srcdir = [(a, -1 if 2 * c[a] + 1 > ipos[a] else 1) for a in range(3)]
    o = [0, 1, 2]
    if d[o[2]] > d[o[1]]:
        o[2], o[1] = o[1], o[2]
    if d[o[0]] <= d[o[1]]:
        o[0], o[1] = o[1], o[0]
    if d[o[1]] <= d[o[2]]:
        o[1], o[2] = o[2], o[1]
    entry = srcdir[o[0]]
    perp = [srcdir[o[1]], srcdir[o[2]]]
    deltas = [float(d[o[1]]) / float(d[o[0]]), float(d[o[2]]) / float(d[o[0]])]
    ds = dx * math.sqrt(1. + deltas[0] * deltas[0] + deltas[1] * deltas[1])
    idx = 2.0
    idxo2 = 0.5 * idx
    if d[o[0]] < idx:
        return 0.0, ds
    if d[o[1]] < idx:
        ngb = G.next(c, *entry)
        Nc = G.get_col(ngb) if ngb is not None else 0.0
        Nc = max(Nc, 0.0)
        if d[o[0]] < 15.0 * idxo2:
            mx = float(d[o[0]])
            mx2 = mx - idx
            Nc *= math.sqrt((mx * mx + idxo2 * idxo2) / (mx2 * mx2 + idxo2 * idxo2)) * mx2 / mx
        return Nc, ds
    if d[o[2]] < idx:
        Nc = _col2cell_2d(G, taumin, c, entry, perp[0], deltas[0])
        if d[o[0]] < 5 * idx:
            if d[o[0]] == 3 * idxo2:
                Nc *= 0.8388704928
            else:
                one_over_r2 = 1.0 / (d[o[0]] * d[o[0]] + d[o[1]] * d[o[1]])
                one_over_a2r2 = float(d[o[0]] * d[o[0]]) / ((d[o[0]] - idx) * (d[o[0]] - idx)) * one_over_r2
                Nc *= (1.0 + one_over_r2) * (1.0 - one_over_a2r2)
        return Nc, ds
    # col2cell_3d (2541-2615)
    c1 = G.next(c, *entry)
    if c1 is None:
        col1 = col2 = col3 = col4 = 0.0
    else:
        col1 = G.get_col(c1)
        c2 = G.next(c1, *perp[0])
        col2 = 0.0 if c2 is None else G.get_col(c2)
        c3 = G.next(c1, *perp[1])
        col3 = 0.0 if c3 is None else G.get_col(c3)
        if c2 is not None and c3 is not None:
            c4 = G.next(c2, *perp[1])
            assert c4 is not None, "lost on grid -- corner cell doesn't exist"
            col4 = G.get_col(c4)
        else:
            col4 = 0.0
    return interpolate_3D(taumin, deltas[0], deltas[1], col1, col2, col3, col4), ds


def _process_cell(G, c, col2cell, ds, opacity, rho, y):
    """ProcessCell (855-1057) for the opacity rules without microphysics"""
    r = float(rho[c[2], c[1], c[0]])
    if opacity == OPACITY_MINUS:
        cell_col = ds * r * (1.0 - float(y[c[2], c[1], c[0]]))
    elif opacity == OPACITY_TOTAL:
        cell_col = ds * r
    elif opacity == OPACITY_TRACER:
        cell_col = ds * r * float(y[c[2], c[1], c[0]])
    else:
        raise ValueError("RT-ProcessCell opacity?")
    G.dcol[c[2], c[1], c[0]] = cell_col
    col2cell += cell_col
    G.col[c[2], c[1], c[0]] = col2cell


def trace_point(ng, ndim, ipos, dx, opacity, rho, y=None):
    """RayTrace_SingleSource (1436-1566) for a finite source with integer position ipos (a vertex): (col, dcol), each
    [nz][ny][nx].  rho, y: on-grid arrays [nz][ny][nx]."""
    G = _Grid(ng, ndim)
    taumin = 0.7
    if ndim == 3:
        taumin *= 6.0 / 7.0
    ipos = list(ipos) + [0] * (3 - len(ipos))
    v = [ipos[a] // 2 for a in range(3)]
    assert all(2 * v[a] == ipos[a] for a in range(3))

    def outwards(a, side):
        """the on-grid indices of axis a on one side of the source, nearest first"""
        if a >= ndim:
            return [0] if side == 1 else []
        if side == 1:
            return list(range(max(v[a], 0), G.ng[a]))
        return list(range(min(v[a] - 1, G.ng[a] - 1), -1, -1))

    for oct_ in range(8):
        sides = [(oct_ >> a) & 1 for a in range(3)]
        for iz in outwards(2, sides[2]):
            for iy in outwards(1, sides[1]):
                for ix in outwards(0, sides[0]):
                    c = (ix, iy, iz)
                    if ndim == 3:
                        Nc, ds = _cell_cols_3d(G, ipos, taumin, dx, c)
                    else:
                        Nc, ds = _cell_cols_2d(G, ipos, taumin, dx, c)
                    _process_cell(G, c, Nc, ds, opacity, rho, y)
    return G.col, G.dcol


def trace_parallel(ng, ndim, direction, dx, opacity, rho, y=None):
    """trace_parallel_rays / trace_column_parallel (695-792): `direction` 0..5 = XN XP YN YP ZN ZP is the face the
    source lies beyond"""
    G = _Grid(ng, ndim)
    axis, towards_source = direction // 2, (-1 if direction % 2 == 0 else 1)
    n = G.ng[axis]
    others = [a for a in range(3) if a != axis]
    for j in range(G.ng[others[1]]):
        for i in range(G.ng[others[0]]):
            order = range(n) if towards_source < 0 else range(n - 1, -1, -1)
            for k in order:
                c = [0, 0, 0]
                c[axis], c[others[0]], c[others[1]] = k, i, j
                c = tuple(c)
                ngb = G.next(c, axis, towards_source)   # cell_cols_1d (801-846)
                Nc = G.get_col(ngb) if ngb is not None else 0.0
                _process_cell(G, c, Nc, dx, opacity, rho, y)
    return G.col, G.dcol


def trace(cfg_ng, ndim, xmin, dx, src, rho, y=None):
    """a source given as a dict (pos, at_infinity, dir, opacity): (col, dcol, moved position or None)"""
    if src.get("at_infinity", 0):
        col, dcol = trace_parallel(cfg_ng, ndim, src["dir"], dx, src.get("opacity", OPACITY_TOTAL), rho, y)
        return col, dcol, None
    moved, ipos = source_vertex(src["pos"], xmin, dx, ndim)
    col, dcol = trace_point(cfg_ng, ndim, ipos, dx, src.get("opacity", OPACITY_TOTAL), rho, y)
    return col, dcol, moved
