"""The rules of the ray-traced column densities (pion_amd/csrc/dev_raytrace.h) in their host loop,
pion_gpu_raytrace_host, against the scalar restatement of the reference's tracer in raytrace_restate.py: col and dcol
with ==.  No device: the library is only loaded."""
import itertools
import os

import numpy as np
import pytest

import raytrace_restate as rs
from pion_amd import abi, lib

need_lib = pytest.mark.skipif(not os.path.exists(abi.library_path()), reason="libpion_gpu.so not built")
pytestmark = need_lib

DX = 0.5
XMIN = (1.0, -2.0, 0.25)


def make_cfg(ng, coord_sys=1, ntracer=1, bcs=None, ndim=None):
    ndim = len(ng) if ndim is None else ndim
    return abi.make_config(ndim, ng, abi.EQEUL, abi.FLUX_RSroe, ntracer=ntracer, dx=DX, xmin=XMIN,
                           bcs=bcs if bcs is not None else ["outflow"] * (2 * ndim), coord_sys=coord_sys)


def make_state(cfg, seed=5, uniform=None):
    """a log-normal rho with rho dx from 5e-3 to 300 (both sides of every max(TauMin, tau)), a tracer in [0, 1]; the
    ghost cells hold NaN: only on-grid cells may be read"""
    rng = np.random.default_rng(seed)
    nga = abi.ng_all(cfg)
    P = np.full((cfg.nvar, nga[2], nga[1], nga[0]), np.nan)
    ng = [cfg.ng[0], cfg.ng[1], cfg.ng[2]]
    nb = [cfg.nbc if a < cfg.ndim else 0 for a in range(3)]
    sl = tuple(slice(nb[a], nb[a] + ng[a]) for a in (2, 1, 0))
    shape = (ng[2], ng[1], ng[0])
    tau = np.clip(np.exp(rng.normal(np.log(1.2), 2.4, shape)), 5.0e-3, 300.0)
    rho = tau / DX if uniform is None else np.full(shape, float(uniform))
    y = rng.uniform(0.0, 1.0, shape)
    for v in range(cfg.nvar):
        P[(v,) + sl] = 1.0
    P[(0,) + sl] = rho
    P[(cfg.nvar - 1,) + sl] = y
    return P, rho, y


def pos_of(cfg, cells):
    """physical position of a point `cells` cell widths from the low corner of the grid"""
    return tuple(XMIN[a] + cells[a] * DX for a in range(len(cells)))


def sources_3d(ng):
    nx, ny, nz = ng
    return {
        "interior": (5.0, 4.0, 3.0), "interior-moved": (5.5, 4.3, 2.7), "face": (0.0, 4.0, 3.0), "edge": (0.0, 0.0, 3.0),
        "corner": (0.0, 0.0, 0.0), "off-1": (-3.0, 4.0, 3.0), "off-2": (-3.0, ny + 3.0, 3.0),
        "off-3": (nx + 3.0, -3.0, nz + 3.0), "far-corner": (float(nx), float(ny), float(nz)),
    }


def sources_2d(ng):
    nx, ny = ng
    return {
        "interior": (7.0, 5.0), "interior-moved": (7.5, 5.49), "face": (0.0, 6.0), "corner": (0.0, 0.0),
        "off-1": (-3.0, 6.0), "off-2": (nx + 3.0, -3.0), "far-corner": (float(nx), float(ny)),
    }


def restate(cfg, src, rho, y):
    ng = [cfg.ng[a] for a in range(cfg.ndim)]
    return rs.trace(ng, cfg.ndim, XMIN, DX, src, rho, y)


def check(cfg, src, seed=5):
    P, rho, y = make_state(cfg, seed)
    col, dcol = lib.raytrace_host(cfg, src, P)
    rcol, rdcol, _ = restate(cfg, src, rho, y)
    assert np.all(np.isfinite(col)) and np.all(np.isfinite(dcol))
    assert np.array_equal(dcol, rdcol)
    assert np.array_equal(col, rcol)
    return col


def test_field_takes_both_sides_of_taumin():
    cfg = make_cfg((13, 11, 12))
    _, rho, _ = make_state(cfg)
    tau = rho * DX
    assert tau.min() < 0.1 and tau.max() > 100.0
    col = check(cfg, {"pos": pos_of(cfg, (5.0, 4.0, 3.0))})
    frac = np.mean(col < 0.6)
    assert 0.005 < frac < 0.5, frac


@pytest.mark.parametrize("ng", [(27, 22, 25), (9, 7, 5)])
@pytest.mark.parametrize("where", sorted(sources_3d((1, 1, 1))))
def test_point_source_3d(ng, where):
    cfg = make_cfg(ng)
    check(cfg, {"pos": pos_of(cfg, sources_3d(ng)[where])})


@pytest.mark.parametrize("coord_sys", [1, 2])
@pytest.mark.parametrize("where", sorted(sources_2d((1, 1))))
def test_point_source_2d(coord_sys, where):
    ng = (41, 23)
    bcs = ["outflow", "outflow", "axisymmetric" if coord_sys == 2 else "outflow", "outflow"]
    cfg = make_cfg(ng, coord_sys=coord_sys, bcs=bcs)
    check(cfg, {"pos": pos_of(cfg, sources_2d(ng)[where])})


@pytest.mark.parametrize("opacity", [abi.RT_OPACITY_TOTAL, abi.RT_OPACITY_MINUS, abi.RT_OPACITY_TRACER])
@pytest.mark.parametrize("ng", [(9, 7, 5), (12, 9)])
def test_opacity_rules(ng, opacity):
    cfg = make_cfg(ng)
    check(cfg, {"pos": pos_of(cfg, (3.0, 2.0, 1.0)[:len(ng)]), "opacity": opacity})
    check(cfg, {"at_infinity": 1, "dir": 1, "opacity": opacity})


@pytest.mark.parametrize("ng", [(9, 7, 5), (41, 23)])
def test_sources_at_infinity(ng):
    cfg = make_cfg(ng)
    P, rho, y = make_state(cfg)
    for d in range(2 * len(ng)):
        col = check(cfg, {"at_infinity": 1, "dir": d})
        # a sequential cumsum along the axis from the face the source lies beyond
        ax = 2 - d // 2
        r = rho * DX
        if d % 2:
            r = np.flip(r, ax)
        want = np.zeros_like(r)
        acc = np.zeros(np.delete(r.shape, ax))
        for k in range(r.shape[ax]):
            acc = acc + np.take(r, k, ax)
            idx = [slice(None)] * 3
            idx[ax] = k
            want[tuple(idx)] = acc
        if d % 2:
            want = np.flip(want, ax)
        assert np.array_equal(col, want)


def test_symmetry_of_a_uniform_field():
    n = 14
    cfg = make_cfg((n, n, n))
    P, _, _ = make_state(cfg, uniform=3.0)
    col, dcol = lib.raytrace_host(cfg, {"pos": pos_of(cfg, (n / 2, n / 2, n / 2))}, P)
    for a in (col, dcol):
        for perm in itertools.permutations(range(3)):
            assert np.array_equal(a, a.transpose(perm)), perm
        for ax in range(3):
            assert np.array_equal(a, np.flip(a, ax)), ax


def _plan_enumeration(cfg, cells):
    """levels, tile-levels and the dependency of every on-grid cell by enumeration, from the restatement's vertex"""
    ndim = cfg.ndim
    ng = [cfg.ng[a] for a in range(3)]
    tile, launches, levels = lib.rt_plan(cfg, {"pos": pos_of(cfg, cells)})
    _, ipos = rs.source_vertex(pos_of(cfg, cells), XMIN, DX, ndim)
    ipos = ipos + [0] * (3 - ndim)
    seen_L, seen_T = set(), set()
    for iz in range(ng[2]):
        for iy in range(ng[1]):
            for ix in range(ng[0]):
                i = (ix, iy, iz)
                d = [abs(2 * i[a] + 1 - ipos[a]) for a in range(3)]
                k = [(d[a] - 1) // 2 for a in range(3)]
                t = tuple(k[a] // tile[a] for a in range(3))
                L, T = sum(k), sum(t)
                seen_L.add(L)
                seen_T.add(T)
                # what the cell reads: one step nearer along the axis of the largest distance, 0 or 1 along the others
                o0 = max(range(ndim), key=lambda a: d[a])
                if d[o0] < 2:
                    continue
                for steps in itertools.product((0, 1), repeat=ndim - 1):
                    kk = list(k)
                    kk[o0] -= 1
                    others = [a for a in range(ndim) if a != o0]
                    ok = True
                    for a, s in zip(others, steps):
                        if s and d[a] < 2:
                            ok = False   # never read across a source plane
                        kk[a] -= s
                    if not ok:
                        continue
                    assert min(kk) >= 0
                    assert sum(kk) < L
                    tt = tuple(kk[a] // tile[a] for a in range(3))
                    assert sum(tt) < T or tt == t
    return tile, launches, levels, seen_L, seen_T


@pytest.mark.parametrize("ng,cells", [((9, 7, 5), (4.0, 3.0, 2.0)), ((9, 7, 5), (0.0, 0.0, 2.0)), ((9, 7, 5), (-3.0, 10.0, 2.0)),
                                      ((27, 22, 25), (5.0, 4.0, 3.0)), ((27, 22, 25), (30.0, -3.0, 28.0)),
                                      ((41, 23), (7.0, 5.0)), ((41, 23), (44.0, -3.0)), ((70, 150), (0.0, 75.0))])
def test_plan(ng, cells):
    cfg = make_cfg(ng)
    tile, launches, levels, seen_L, seen_T = _plan_enumeration(cfg, cells)
    assert tile == ((16, 8, 8) if len(ng) == 3 else (32, 64, 1))
    assert levels == max(seen_L) - min(seen_L) + 1 == len(seen_L)
    assert launches == max(seen_T) - min(seen_T) + 1 == len(seen_T)


def test_plan_of_a_source_at_infinity():
    assert lib.rt_plan(make_cfg((9, 7, 5)), {"at_infinity": 1, "dir": 4}) == ((0, 0, 0), 1, 1)


REFUSALS = [
    (dict(ng=(16,), ndim=1), {}, "1-D and spherical grids are not traced"),
    (dict(ng=(16,), ndim=1, coord_sys=3), {}, "1-D and spherical grids are not traced"),
    (dict(ng=(9, 7, 5), bcs=["outflow"] * 4 + ["slab", "outflow"]), {}, "a slab of a decomposed run is not traced"),
    (dict(ng=(9, 7)), {"opacity": 4}, "the opacity rule needs a microphysics object"),
    (dict(ng=(9, 7)), {"opacity": 0}, "the opacity rule needs a microphysics object"),
    (dict(ng=(9, 7)), {"opacity": 9}, "the opacity rule needs a microphysics object"),
    (dict(ng=(9, 7)), {"opacity": abi.RT_OPACITY_MINUS, "opacity_var": 1}, "opacity_var is not a tracer of the state"),
    (dict(ng=(9, 7)), {"opacity": abi.RT_OPACITY_TRACER, "opacity_var": -1}, "opacity_var is not a tracer of the state"),
    (dict(ng=(9, 7), ntracer=0), {"opacity": abi.RT_OPACITY_TRACER}, "opacity_var is not a tracer of the state"),
    (dict(ng=(9, 7)), {"at_infinity": 1, "dir": 4}, "the direction of a source at infinity is a face of the grid"),
    (dict(ng=(9, 7, 5)), {"at_infinity": 1, "dir": 6}, "the direction of a source at infinity is a face of the grid"),
    (dict(ng=(9, 7, 5)), {"at_infinity": 1, "dir": -1}, "the direction of a source at infinity is a face of the grid"),
    (dict(ng=(9, 7)), {"pos": (float("nan"), 0.0)}, "the position of a finite source is finite"),
]


@pytest.mark.parametrize("grid,src,text", REFUSALS)
def test_refusals(grid, src, text):
    cfg = make_cfg(**grid)
    assert text in lib.rt_refused(cfg, src)
    P = np.ones((cfg.nvar,) + tuple(reversed(abi.ng_all(cfg))))
    with pytest.raises(lib.PionGpuError, match="rc=-1.*" + text.split("(")[0]):
        lib.raytrace_host(cfg, src, P)
    with pytest.raises(lib.PionGpuError, match="rc=-1"):
        lib.rt_plan(cfg, src)


def test_accepted_sources_are_not_refused():
    assert lib.rt_refused(make_cfg((9, 7)), {"opacity": abi.RT_OPACITY_TRACER, "opacity_var": 0}) is None
    assert lib.rt_refused(make_cfg((9, 7), ntracer=0), {}) is None   # TOTAL reads no tracer
    assert lib.rt_refused(make_cfg((9, 7, 5)), {"at_infinity": 1, "dir": 5}) is None


# The analytic check: for a uniform density the column of a cell at distance r from a source on the grid is
# rho (r + ds / 2) up to the interpolation's error.  The bounds are 1.25 x the largest relative deviation of the
# restatement (raytrace_restate.py) on these grids: 2-D 48^2: 0.976632 %.  3-D 24^3: 8.387421 %, nearly all of it in
# the source-plane approximations of cell_cols_3d (2451-2470).  
ANALYTIC = {2: (48, 48), 3: (24, 24, 24)}
ANALYTIC_SEEN = {2: 0.009766321764053376, 3: 0.08387420812114224}


def analytic_deviation(col, ng, rho):
    ndim = len(ng)
    ctr = [n / 2 for n in ng] + [0.5] * (3 - ndim)
    z, y, x = np.meshgrid(*[np.arange(s) + 0.5 for s in col.shape], indexing="ij")
    off = [np.abs(x - ctr[0]), np.abs(y - ctr[1]), np.abs(z - ctr[2])]
    r = DX * np.sqrt(sum(o * o for o in off))
    big = np.maximum(np.maximum(off[0], off[1]), off[2])
    ds = DX * np.sqrt(sum((o / big) ** 2 for o in off))
    want = rho * (r + 0.5 * ds)
    return float(np.max(np.abs(col - want) / want))


@pytest.mark.parametrize("ndim", [2, 3])
def test_uniform_density_against_the_analytic_column(ndim):
    ng = ANALYTIC[ndim]
    cfg = make_cfg(ng)
    P, _, _ = make_state(cfg, uniform=2.0)
    col, _ = lib.raytrace_host(cfg, {"pos": pos_of(cfg, [n / 2 for n in ng])}, P)
    dev = analytic_deviation(col, ng, 2.0)
    print("analytic deviation %d-D: %.6f (bound %.6f)" % (ndim, dev, 1.25 * ANALYTIC_SEEN[ndim]))
    assert dev <= 1.25 * ANALYTIC_SEEN[ndim]
