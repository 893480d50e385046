"""What the tests of a slab run's projected images (tests/test_host_projection_ranks.py,
tests/test_gpu_projection_ranks.py) share: the cases, the slabs of a global state with NaN in every ghost cell the rule
may not read, and the numpy sums that show that the states are rough enough for == to mean something -- the NAIVE
assembly (every rank sums its own planes from 0.0, the partial images are added afterwards) differs from the single
sum in at least one pixel, so only carrying the running sums from rank to rank gives the single grid's bits.

Extends tests/projection_restate.py (its field, its Abel geometry), shares nothing with pion_amd/csrc/dev_project.h.
The single-rank images themselves are pinned to that restatement by tests/test_host_projection.py and
tests/test_gpu_projection.py; here they are only the other side of an == comparison."""
import numpy as np

import projection_restate as pr
from pion_amd import abi, slab

COOL = pr.COOL


def case(name, strict=1):
    """global configurations: the slab axis divides by the rank count, positions are dyadic (dx = 1/8)"""
    kw = dict(strict_fp=strict, dx=0.125)
    cyl = lambda ng, **k: abi.make_config(2, ng, abi.EQEUL, abi.FLUX_RSroe, ntracer=1, coord_sys=2,
                                          **dict(dict(kw, bcs=pr.CYL_BCS), **k))
    if name == "euler_tr_70x9x10":       # nx > 64: the x tree has a second round; 5 planes per rank of 2
        return abi.make_config(3, [70, 9, 10], abi.EQEUL, abi.FLUX_RSroe, ntracer=1, **kw)
    if name == "glm_tr_66x5x15":         # 3 ranks
        return abi.make_config(3, [66, 5, 15], abi.EQGLM, abi.FLUX_RS_HLLD, ntracer=1, **kw)
    if name == "cyl_70x10":              # a 16-row Abel tile spans both ranks
        return cyl([70, 10])
    if name == "cyl_70x40":              # tile edges inside each rank
        return cyl([70, 40])
    if name == "cyl_70x40_off_axis":     # 3 dx off the axis
        return cyl([70, 40], xmin=(0.0, 3 * 0.125), bcs=["outflow"] * 4)
    if name == "cyl_cool_70x40":         # a temperature: T^-0.9
        return cyl([70, 40], **COOL)
    raise KeyError(name)


def fields_of(name, cfg):
    f = pr.fields_of(cfg)
    return f + [pr.HALPHA] if "cool" in name else f


def axis_of(cfg, axis=None):
    return abi.PROJ_AXIS_PERP if cfg.coord_sys == 2 else axis


def nan_ghosts(cfg, A, upper_row=False):
    """A with NaN in every ghost cell; upper_row: the first upper ghost row of the slab axis keeps its on-grid x cells
    (the one row the slope of a cylindrical part's last own row reads)"""
    out = np.full(A.shape, np.nan)
    nb = cfg.nbc
    sl = [slice(None)] + [slice(nb, nb + cfg.ng[a]) if a < cfg.ndim else slice(None) for a in (2, 1, 0)]
    out[tuple(sl)] = A[tuple(sl)]
    if upper_row:
        ax = 3 - slab.slab_axis(cfg)          # array axis of the slab axis
        sl[ax] = slice(nb + cfg.ng[slab.slab_axis(cfg)], nb + cfg.ng[slab.slab_axis(cfg)] + 1)
        out[tuple(sl)] = A[tuple(sl)]
    return out


def slab_state(P_global, cfg_g, rank, world):
    """(cfg, A) of rank `rank`: slab.slab_slice of the global state -- the neighbours' rows in the slab ghosts --, then
    NaN in the x ghosts, the lower slab ghosts and the outer upper ghost rows; a cylindrical rank below the last keeps
    the neighbour's first row"""
    cfg = slab.slab_config(cfg_g, rank, world)
    A = slab.slab_slice(P_global, cfg_g, rank, world)
    return cfg, nan_ghosts(cfg, A, upper_row=(cfg_g.coord_sys == 2 and rank < world - 1))


def part_of(cfg_g, rank, world):
    """(plane_lo, global_planes, last, global_xmin) of rank `rank`"""
    ax = slab.slab_axis(cfg_g)
    n = cfg_g.ng[ax] // world
    return rank * n, cfg_g.ng[ax], int(rank == world - 1), cfg_g.xmin[ax]


def naive_differs(cfg, A, fields, axis, world):
    """True if for at least one field and pixel the naive assembly over `world` ranks differs from the single sum.
    3-D along z: (sum_r (sum of rank r's planes from 0.0)) * dx against (one sum) * dx.  Cylindrical: 2 * (sum_r of rank
    r's segments from 0.0) against 2 * (one sum).  One numpy operation per addition, as in projection_restate."""
    differs = False
    for f in fields:
        v, _ = pr.field_value(cfg, A, f)
        if cfg.coord_sys != 2:
            assert axis == 2, "a pixel along x or y lies wholly in one rank: nothing to assemble"
            n = v.shape[0] // world
            single, naive = np.zeros(v[0].shape), np.zeros(v[0].shape)
            for k in range(v.shape[0]):
                single = single + v[k]
            for r in range(world):
                s = np.zeros(v[0].shape)
                for k in range(r * n, (r + 1) * n):
                    s = s + v[k]
                naive = naive + s
            differs |= bool(((single * cfg.dx) != (naive * cfg.dx)).any())
            continue
        v = v[0]
        Nr, dx = cfg.ng[1], cfg.dx
        n = Nr // world
        r = [cfg.xmin[1] + (2 * i + 1) * (0.5 * dx) for i in range(Nr)]
        s = np.zeros(v.shape)
        for i in range(Nr - 1):
            s[i] = (v[i + 1] - v[i]) / (r[i + 1] - r[i])
        s[Nr - 1] = s[Nr - 2]
        for j in range(Nr):
            single, naive, part, owner = np.zeros(v.shape[1]), np.zeros(v.shape[1]), np.zeros(v.shape[1]), None
            for ir, Rmin, xdx, x2dx in pr.abel_segments(r, Nr, r[j], dx):
                seg = s[ir] * x2dx + (v[ir] - s[ir] * Rmin) * xdx
                single = single + seg
                if owner is not None and ir // n != owner:
                    naive = naive + part
                    part = np.zeros(v.shape[1])
                owner = ir // n
                part = part + seg
            naive = naive + part
            differs |= bool(((single * 2.0) != (naive * 2.0)).any())
    return differs
