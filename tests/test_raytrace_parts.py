"""The ray tracer in slab runs, host loop: pion_gpu_raytrace_host_part chained in-process over the ranks of a slab
decomposition, the planes of col handed from rank to rank in the order pion_gpu_rt_chain gives.  The concatenation of
the ranks' arrays is compared with == against the restatement's trace of the whole domain (raytrace_restate.py), col
and dcol.  No tolerance: a decomposed run gives the bits of the single grid, which is also why received columns are
not clamped at 0 as the reference clamps them (RT_MPI_boundaries.cpp:352,364).

No case is tame: for every case whose chain carries a plane the same chain run with zeros in place of the received
planes does not give the whole grid's bits.  The cases and why each is there: raytrace_parts_cases.py.
No device: the library is only loaded."""
import itertools
import os

import numpy as np
import pytest

import raytrace_parts_cases as pc
import raytrace_restate as rs
from pion_amd import abi, lib, slab
from test_raytrace_rule import DX, XMIN, make_cfg, make_state, pos_of

need_lib = pytest.mark.skipif(not os.path.exists(abi.library_path()), reason="libpion_gpu.so not built")
pytestmark = need_lib


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(np.ascontiguousarray(a).view(np.uint64), np.ascontiguousarray(b).view(np.uint64))


@pytest.mark.parametrize("case", sorted(pc.CASES))
def test_chain_gives_the_bits_of_the_whole_domain(case):
    ng, world, coord_sys, spec, yscale = pc.CASES[case]
    cfg = pc.global_cfg(ng, coord_sys)
    src = pc.source_of(cfg, spec)
    P, rho, y = pc.state_of(cfg, yscale)
    tcol, tdcol = pc.truth(cfg, src, rho, y)
    assert np.all(np.isfinite(tcol)) and np.all(np.isfinite(tdcol))
    roles = [lib.rt_chain(slab.slab_config(cfg, r, world), src, pc.part_of(cfg, r, world)) for r in range(world)]
    assert roles == pc.expected_roles(cfg, src, world)
    want_messages = sum(r[0] != abi.RT_RECV_NONE for r in roles)
    assert want_messages == sum(r[1] + r[2] for r in roles)   # every plane sent is received
    if want_messages:
        zcol, _, n = pc.run_chain(cfg, src, world, pc.host_trace(cfg, src, world, P), zeros=True)
        assert n == want_messages
        assert not same_bits(zcol, tcol), "a tame case: the received planes do not matter"
    else:
        assert case.endswith("across")
    col, dcol, n = pc.run_chain(cfg, src, world, pc.host_trace(cfg, src, world, P))
    assert n == want_messages
    assert same_bits(dcol, tdcol)
    bad = np.argwhere(col != tcol)
    assert bad.size == 0 and same_bits(col, tcol), (len(bad), bad[:5].tolist())


def test_no_clamp_negative_columns_cross_the_face():
    """MINUS with the tracer above 1 in some cells: negative columns in the planes handed over; the reference would
    clamp them at 0 on receipt, the single grid does not, and neither does the chain"""
    ng, world, coord_sys, spec, yscale = pc.CASES["3d-minus-tracer-above-1"]
    cfg = pc.global_cfg(ng, coord_sys)
    src = pc.source_of(cfg, spec)
    P, rho, y = pc.state_of(cfg, yscale)
    tcol, _ = pc.truth(cfg, src, rho, y)
    n = ng[2] // world
    handed = [tcol[n * r - 1] for r in range(1, world)]   # the source lies in rank 0: planes travel upwards
    assert all((h < 0.0).any() for h in handed)

    # clamping what is received changes the result: the decision is visible in this case
    def clamped(r, face):
        return pc.host_trace(cfg, src, world, P)(r, None if face is None else np.maximum(face, 0.0))
    ccol, _, _ = pc.run_chain(cfg, src, world, clamped)
    assert not same_bits(ccol, tcol)


@pytest.mark.parametrize("ng,world", [((20, 9, 12), 3), ((41, 24), 2)])
def test_vertex_is_the_whole_domains_on_every_rank(ng, world):
    """positions where centre_source_on_cell rounds (x.5: down; just below: up) and a slab whose own xmin would round
    the other way cannot arise: the vertex comes from global_xmin.  pos_used is checked on the device tests; here the
    roles and the trace agree with the restatement's vertex for positions on every face and half-way."""
    cfg = pc.global_cfg(ng)
    ax = len(ng) - 1
    P, rho, y = pc.state_of(cfg)
    n = ng[ax] // world
    for z in (n - 0.5, n + 0.49, n + 0.5, 2 * n - 0.51 if world > 2 else n + 1.5):
        cells = (7.0, 4.0, z) if ax == 2 else (7.0, z)
        src = {"pos": pos_of(cfg, cells)}
        tcol, tdcol = pc.truth(cfg, src, rho, y)
        col, dcol, _ = pc.run_chain(cfg, src, world, pc.host_trace(cfg, src, world, P))
        assert same_bits(col, tcol) and same_bits(dcol, tdcol), cells


def test_whole_domain_part_equals_the_plain_call():
    for ng in [(20, 9, 12), (41, 24)]:
        cfg = pc.global_cfg(ng)
        P, _, _ = pc.state_of(cfg)
        part = (0, ng[-1], XMIN[len(ng) - 1])
        for spec in ({"cells": (7.0, 4.0, 6.0)[:len(ng)]}, {"cells": (-3.0, 12.0, 15.0)[:len(ng)], "opacity": pc.MINUS},
                     {"at_infinity": 1, "dir": 2 * len(ng) - 1}, {"at_infinity": 1, "dir": 0}):
            src = pc.source_of(cfg, spec)
            assert lib.rt_chain(cfg, src, part) == (abi.RT_RECV_NONE, 0, 0)
            a, b = lib.raytrace_host_part(cfg, src, part, P), lib.raytrace_host(cfg, src, P)
            assert same_bits(a[0], b[0]) and same_bits(a[1], b[1])


def test_null_faces_are_accepted_where_nothing_is_received():
    ng, world, coord_sys, spec, _ = pc.CASES["3d-infinity-across"]
    cfg = pc.global_cfg(ng, coord_sys)
    src = pc.source_of(cfg, spec)
    P, rho, y = pc.state_of(cfg)
    for r in range(world):
        c = slab.slab_config(cfg, r, world)
        assert lib.rt_chain(c, src, pc.part_of(cfg, r, world)) == (abi.RT_RECV_NONE, 0, 0)
        lib.raytrace_host_part(c, src, pc.part_of(cfg, r, world), pc.slab_state(P, cfg, r, world), None)
    # a face where nothing is received is not read
    c = slab.slab_config(cfg, 1, world)
    a = lib.raytrace_host_part(c, src, pc.part_of(cfg, 1, world), pc.slab_state(P, cfg, 1, world), None)
    b = lib.raytrace_host_part(c, src, pc.part_of(cfg, 1, world), pc.slab_state(P, cfg, 1, world), np.full((9, 20), np.nan))
    assert same_bits(a[0], b[0])


def slab_cfg(ng=(9, 7, 4), rank=1, world=3, **kw):
    g = make_cfg(tuple(ng[:-1]) + (ng[-1] * world,), **kw)
    return slab.slab_config(g, rank, world), (rank * ng[-1], ng[-1] * world, XMIN[len(ng) - 1])


def test_part_refusals():
    cfg, part = slab_cfg()
    ok = {"pos": pos_of(cfg, (3.0, 2.0, 1.0))}
    assert lib.rt_part_refused(cfg, ok, part) is None
    assert "a slab of a decomposed run is not traced" in lib.rt_refused(cfg, ok)   # the plain call keeps refusing
    cases = [
        (cfg, ok, None, "raytrace: no part"),
        (cfg, ok, (-1, 12, XMIN[2]), "the part's planes lie outside the whole domain"),
        (cfg, ok, (9, 12, XMIN[2]), "the part's planes lie outside the whole domain"),
        (cfg, ok, (4, 7, XMIN[2]), "the part's planes lie outside the whole domain"),
        (cfg, ok, (4, 12, float("nan")), "the part's global_xmin is not finite"),
        (cfg, ok, (4, 12, float("inf")), "the part's global_xmin is not finite"),
        (cfg, {"opacity": 4}, part, "the opacity rule needs a microphysics object"),
        (cfg, {"opacity": pc.TRACER, "opacity_var": 1}, part, "opacity_var is not a tracer of the state"),
        (cfg, {"at_infinity": 1, "dir": 6}, part, "the direction of a source at infinity is a face of the grid"),
        (cfg, {"pos": (0.0, float("nan"), 0.0)}, part, "the position of a finite source is finite"),
    ]
    # a slab face on another axis than the slab axis is no part of a slab run
    odd = make_cfg((9, 7, 4), bcs=["slab", "outflow"] + ["outflow"] * 4)
    cases.append((odd, ok, (0, 4, XMIN[2]), "a slab of a decomposed run is not traced"))
    sph = make_cfg((16,), ndim=1, coord_sys=3)
    cases.append((sph, {}, (0, 16, XMIN[0]), "1-D and spherical grids are not traced"))
    for c, src, p, text in cases:
        assert text in lib.rt_part_refused(c, src, p), text
        Pz = np.ones((c.nvar,) + tuple(reversed(abi.ng_all(c))))
        with pytest.raises(lib.PionGpuError, match="rc=-1.*" + text.split("(")[0]):
            lib.raytrace_host_part(c, src, p, Pz)
        with pytest.raises(lib.PionGpuError, match="rc=-1.*" + text.split("(")[0]):
            lib.rt_chain(c, src, p)
        with pytest.raises(lib.PionGpuError, match="rc=-1"):
            lib.rt_plan_part(c, src, p)
    # a plane is received and there is none
    Pz = np.ones((cfg.nvar,) + tuple(reversed(abi.ng_all(cfg))))
    assert lib.rt_chain(cfg, ok, part)[0] == abi.RT_RECV_BELOW
    with pytest.raises(lib.PionGpuError, match="rc=-1.*no face"):
        lib.raytrace_host_part(cfg, ok, part, Pz, None)


def _enumerate_tiles(cfg, src, part, tile):
    """tile-levels that hold tiles and the (side, tile) pairs of y and z that hold cells, from the restatement's vertex"""
    ndim = cfg.ndim
    _, ipos = rs.source_vertex(src["pos"], XMIN, DX, ndim)
    ipos = list(ipos) + [0] * (3 - ndim)
    ipos[ndim - 1] -= 2 * part[0]
    seen_T, per_axis = set(), [set(), set(), set()]
    for i in itertools.product(*[range(cfg.ng[a]) for a in range(3)]):
        d = [abs(2 * i[a] + 1 - ipos[a]) for a in range(3)]
        t = [((d[a] - 1) // 2) // tile[a] for a in range(3)]
        seen_T.add(sum(t))
        for a in range(3):
            per_axis[a].add((2 * i[a] + 1 > ipos[a], t[a]))
    return seen_T, per_axis


@pytest.mark.parametrize("ng,world,cells", [((20, 9, 48), 3, (7.0, 4.0, 3.0)), ((20, 9, 48), 3, (-40.0, 30.0, 60.0)),
                                            ((20, 9, 12), 3, (23.0, 12.0, 15.0)), ((70, 264), 2, (35.0, 2.0)),
                                            ((70, 264), 2, (100.0, 300.0))])
def test_plan_of_a_part_counts_only_tiles_that_hold_cells(ng, world, cells):
    """a rank far from the source launches the tile-levels that hold tiles, and per launch the workgroups of the tiles
    between its nearest and its farthest cell -- not of every tile from the vertex outwards"""
    cfg = pc.global_cfg(ng)
    src = {"pos": pos_of(cfg, cells)}
    tile = (16, 8, 8) if len(ng) == 3 else (32, 64, 1)
    trimmed_somewhere = False
    for r in range(world):
        c, part = slab.slab_config(cfg, r, world), pc.part_of(cfg, r, world)
        launches, wg, wg0 = lib.rt_plan_part(c, src, part)
        seen_T, per_axis = _enumerate_tiles(c, src, part, tile)
        assert launches == len(seen_T) == max(seen_T) - min(seen_T) + 1
        assert wg == 2 * len(per_axis[1]) * len(per_axis[2])
        from_vertex = 2
        for a in (1, 2):
            from_vertex *= sum(max(t for s, t in per_axis[a] if s == side) + 1 for side in {s for s, _ in per_axis[a]})
        assert wg0 == from_vertex and wg <= wg0
        trimmed_somewhere |= wg < wg0
    assert trimmed_somewhere
    # the whole-domain plan of pion_gpu_rt_plan is the part plan of the whole domain
    whole = (0, ng[-1], XMIN[len(ng) - 1])
    assert lib.rt_plan_part(cfg, src, whole)[0] == lib.rt_plan(cfg, src)[1]
