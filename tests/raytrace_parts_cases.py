"""Cases and the in-process chain of the ray tracer in slab runs (pion_gpu_raytrace_host_part / pion_gpu_raytrace_part),
shared by test_raytrace_parts.py (host loop) and test_gpu_raytrace_parts.py (device).  Truth is the trace of the whole
domain; every comparison is == on the bits.

The states are test_raytrace_rule.make_state's (log-normal rho, rho dx from 5e-3 to 300, NaN in every ghost cell); a
rank's state is its planes of the whole state, NaN in the ghost planes of the slab axis too.

Positions are given in cell widths from the low corner of the WHOLE domain.  Why each case is there:
  3-D 20 x 9 x 12 over 3 ranks, 4 planes each: every internal face lies inside an 8-plane tile whatever the vertex.
  3-D 20 x 9 x 24 over 3 ranks, 8 planes each: z-vertex 8 lies on a face and puts the next face (16) on a tile boundary
      (received plane in the tile's halo); z-vertex 3 puts faces 8 and 16 mid-tile (k = 5, 13: received plane k = 4, 12
      inside tiles 0 and 1).
  2-D 41 x 24 over 2 ranks: smaller than one 32 x 64 tile, Cartesian and cylindrical.
  2-D 70 x 132 over 2 ranks, 66 rows each: with the row vertex at 0 rank 1 starts at k = 66 (received row k = 65, slot
      1 of the tile of rows 64..127); with the vertex at 2 it starts at k = 64, a tile boundary (received row in the
      halo)."""
import numpy as np

import raytrace_restate as rs
from pion_amd import abi, lib, slab
from test_raytrace_rule import DX, XMIN, make_cfg, make_state, pos_of

TOTAL, MINUS, TRACER = abi.RT_OPACITY_TOTAL, abi.RT_OPACITY_MINUS, abi.RT_OPACITY_TRACER

# name: (ng, world, coord_sys, source as a dict with `cells` (a finite source) or at_infinity / dir, tracer scale)
CASES = {
    "3d-inside-rank-1": ((20, 9, 12), 3, 1, {"cells": (7.0, 4.0, 6.0)}, 1.0),
    "3d-corner": ((20, 9, 12), 3, 1, {"cells": (0.0, 0.0, 0.0)}, 1.0),
    "3d-far-corner": ((20, 9, 12), 3, 1, {"cells": (20.0, 9.0, 12.0)}, 1.0),
    "3d-off-grid-below": ((20, 9, 12), 3, 1, {"cells": (-3.0, -3.0, -3.0)}, 1.0),
    "3d-off-grid-above": ((20, 9, 12), 3, 1, {"cells": (23.0, 12.0, 15.0)}, 1.0),
    "3d-vertex-on-face-4": ((20, 9, 12), 3, 1, {"cells": (7.0, 4.0, 4.0)}, 1.0),
    "3d-beyond-top-along-z": ((20, 9, 12), 3, 1, {"cells": (7.0, 4.0, 15.0)}, 1.0),
    "3d-moved-vertex": ((20, 9, 12), 3, 1, {"cells": (7.5, 4.3, 8.49)}, 1.0),
    "3d-24-vertex-8": ((20, 9, 24), 3, 1, {"cells": (7.0, 4.0, 8.0)}, 1.0),
    "3d-24-vertex-3": ((20, 9, 24), 3, 1, {"cells": (12.0, 4.0, 3.0)}, 1.0),
    "3d-minus": ((20, 9, 12), 3, 1, {"cells": (7.0, 4.0, 6.0), "opacity": MINUS}, 1.0),
    "3d-minus-tracer-above-1": ((20, 9, 12), 3, 1, {"cells": (7.0, 4.0, 1.0), "opacity": MINUS}, 1.6),
    "3d-tracer": ((20, 9, 12), 3, 1, {"cells": (7.0, 4.0, 6.0), "opacity": TRACER}, 1.0),
    "3d-infinity-zn": ((20, 9, 12), 3, 1, {"at_infinity": 1, "dir": 4}, 1.0),
    "3d-infinity-zp": ((20, 9, 12), 3, 1, {"at_infinity": 1, "dir": 5, "opacity": TRACER}, 1.0),
    "3d-infinity-across": ((20, 9, 12), 3, 1, {"at_infinity": 1, "dir": 0, "opacity": MINUS}, 1.0),
    "2d-inside-rank-0": ((41, 24), 2, 1, {"cells": (7.0, 5.0)}, 1.0),
    "2d-off-grid": ((41, 24), 2, 1, {"cells": (44.0, -3.0)}, 1.0),
    "2d-beyond-top": ((41, 24), 2, 1, {"cells": (20.0, 27.0), "opacity": MINUS}, 1.0),
    "2d-cylindrical-on-axis": ((41, 24), 2, 2, {"cells": (20.0, 0.0)}, 1.0),
    "2d-cylindrical-rank-1": ((41, 24), 2, 2, {"cells": (30.0, 17.0), "opacity": TRACER}, 1.0),
    "2d-infinity-yn": ((41, 24), 2, 1, {"at_infinity": 1, "dir": 2}, 1.0),
    "2d-infinity-yp": ((41, 24), 2, 2, {"at_infinity": 1, "dir": 3}, 1.0),
    "2d-tiles-vertex-0": ((70, 132), 2, 1, {"cells": (35.0, 0.0)}, 1.0),
    "2d-tiles-vertex-2": ((70, 132), 2, 1, {"cells": (33.0, 2.0)}, 1.0),
}


def global_cfg(ng, coord_sys=1, strict=1):
    bcs = ["outflow", "outflow", "axisymmetric", "outflow"] if coord_sys == 2 else None
    cfg = make_cfg(ng, coord_sys=coord_sys, bcs=bcs)
    cfg.strict_fp = strict
    return cfg


def source_of(cfg, spec):
    """the source of the whole domain as abi.rt_source takes it"""
    s = {k: v for k, v in spec.items() if k != "cells"}
    if "cells" in spec:
        s["pos"] = pos_of(cfg, spec["cells"])
    return s


def part_of(cfg, rank, world):
    ax = slab.slab_axis(cfg)
    n = cfg.ng[ax] // world
    return (rank * n, cfg.ng[ax], cfg.xmin[ax])


def state_of(cfg, yscale=1.0, seed=5):
    """(P, rho, y) of the whole domain; yscale > 1 puts the tracer above 1 in some cells"""
    P, rho, y = make_state(cfg, seed)
    if yscale != 1.0:
        y = y * yscale
        nb = [cfg.nbc if a < cfg.ndim else 0 for a in range(3)]
        sl = tuple(slice(nb[a], nb[a] + cfg.ng[a]) for a in (2, 1, 0))
        P[(cfg.nvar - 1,) + sl] = y
    return P, rho, y


def slab_state(P, cfg, rank, world):
    """the rank's planes of P, NaN in the ghost planes of the slab axis"""
    S = slab.slab_slice(P, cfg, rank, world)
    nb = cfg.nbc
    if cfg.ndim == 3:
        S[:, :nb] = np.nan
        S[:, -nb:] = np.nan
    else:
        S[:, :, :nb] = np.nan
        S[:, :, -nb:] = np.nan
    return S


def truth(cfg, src, rho, y):
    """the restatement's trace of the whole domain: (col, dcol)"""
    ng = [cfg.ng[a] for a in range(cfg.ndim)]
    col, dcol, _ = rs.trace(ng, cfg.ndim, XMIN, DX, src, rho, y)
    return col, dcol


def faces_of(col, ndim):
    """the lowest and highest own plane of a rank's col [nz][ny][nx]"""
    if ndim == 3:
        return col[0].copy(), col[-1].copy()
    return col[0, 0].copy(), col[0, -1].copy()


def expected_roles(cfg, src, world):
    """(recv_side, send_lo, send_hi) per rank by enumeration from the restatement's vertex: the rank that holds the
    vertex plane (clipped to the domain) starts the chain, the planes travel outwards from it"""
    ax = slab.slab_axis(cfg)
    n = cfg.ng[ax] // world
    if src.get("at_infinity", 0):
        if src["dir"] // 2 != ax:
            return [(abi.RT_RECV_NONE, 0, 0)] * world
        owner = world - 1 if src["dir"] % 2 else 0
    else:
        _, ipos = rs.source_vertex(src["pos"], XMIN, DX, cfg.ndim)
        assert ipos[ax] % 2 == 0
        owner = min(max((ipos[ax] // 2) // n, 0), world - 1)
    roles = []
    for r in range(world):
        recv = abi.RT_RECV_NONE if r == owner else (abi.RT_RECV_BELOW if r > owner else abi.RT_RECV_ABOVE)
        roles.append((recv, int(r <= owner and r > 0), int(r >= owner and r < world - 1)))
    return roles


def run_chain(cfg, src, world, trace, zeros=False):
    """Chains trace(rank, face_in or None) -> (col, dcol) over the ranks in the order the roles of pion_gpu_rt_chain
    give: a rank runs once the plane it receives exists.  zeros: every received plane is replaced by zeros (what a
    tracer that ignored it would see).  Returns (col, dcol) of the whole domain and the number of planes handed over."""
    ax = slab.slab_axis(cfg)
    cfgs = [slab.slab_config(cfg, r, world) for r in range(world)]
    roles = [lib.rt_chain(cfgs[r], src, part_of(cfg, r, world)) for r in range(world)]
    sent, done, messages = {}, {}, 0
    while len(done) < world:
        progressed = False
        for r in range(world):
            if r in done:
                continue
            recv, send_lo, send_hi = roles[r]
            face = None
            if recv != abi.RT_RECV_NONE:
                key = (r - 1, "hi") if recv == abi.RT_RECV_BELOW else (r + 1, "lo")
                if key not in sent:
                    continue
                face = np.zeros_like(sent[key]) if zeros else sent[key]
                messages += 1
            col, dcol = trace(r, face)
            lo, hi = faces_of(col, cfg.ndim)
            if send_lo:
                sent[(r, "lo")] = lo
            if send_hi:
                sent[(r, "hi")] = hi
            done[r] = (col, dcol)
            progressed = True
        assert progressed, "the roles leave a rank waiting for a plane nobody sends: %r" % (roles,)
    cat_axis = 0 if ax == 2 else 1
    return (np.concatenate([done[r][0] for r in range(world)], cat_axis),
            np.concatenate([done[r][1] for r in range(world)], cat_axis), messages)


def host_trace(cfg, src, world, P):
    """trace(rank, face) of run_chain through pion_gpu_raytrace_host_part"""
    def trace(r, face):
        return lib.raytrace_host_part(slab.slab_config(cfg, r, world), src, part_of(cfg, r, world),
                                      slab_state(P, cfg, r, world), face)
    return trace
