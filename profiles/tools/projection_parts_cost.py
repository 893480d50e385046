#!/usr/bin/env python3
"""Kernel time of one rank's part of a slab run's projected image (pion_gpu_project_part; DESIGN.md s6e, "Slab runs";
profiles/projection_parts.json), beside the whole-grid calls of profiles/tools/projection_cost.py measured again in the
same session:
    profiles/tools/projection_parts_cost.py [--abel 4096x2048] [--world 8] [--box 512x512x64] [--reps 20]
Abel: one rank's share (NR / world rows) of a cylindrical (z,R) Euler + 1 tracer grid of NZ x NR cells, three fields
(rho, rho^2, rho TR0), the lowest rank and the highest: the lowest rank's rows are met by few rays, the highest rank's
by every impact row below its upper edge.  Beside it the whole grid in one pion_gpu_project call.
Column sums: a GLM-MHD slab of NX x NY x NZ_local cells (fast build) along z, one field (rho), as a middle part and as
the last one; beside it pion_gpu_project on the same handle.
Chain: the end-to-end time of a two-rank chain on one GPU -- two handles, each its half of the Abel grid, part after
part in one device buffer, from the first call to a synchronised device.
Each call is timed --reps times after a warm-up, host clock from the call to a synchronised device.  The states are
uniform random numbers made on the device and bound to the handle (a part's upper ghost row is part of that array).
Prints one JSON line."""
import argparse
import json
import os
import sys

HERE = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from projection_cost import bound_state, timed  # noqa: E402

CYL_BCS = ["outflow", "outflow", "axisymmetric", "outflow"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--abel", default="4096x2048")
    ap.add_argument("--world", type=int, default=8)
    ap.add_argument("--box", default="512x512x64")
    ap.add_argument("--reps", type=int, default=20)
    a = ap.parse_args()
    import torch
    from pion_amd import abi, lib
    res = {"gpu_lib": os.environ.get("PION_GPU_LIB", "in-tree"), "reps": a.reps}
    perp = abi.PROJ_AXIS_PERP
    fields = [("coldens", 1, -1, 1.0, 0.0), ("emmeasure", 2, -1, 1.0, 0.0), ("windcol", 1, 5, 1.0, 0.0)]
    nz, nr = (int(x) for x in a.abel.split("x"))
    dx = 1.0 / nr

    def cyl(rows, lo):
        return abi.make_config(2, [nz, rows], abi.EQEUL, abi.FLUX_RSroe, ntracer=1, coord_sys=2, dx=dx, strict_fp=0,
                               bcs=CYL_BCS, xmin=(0.0, lo * dx))

    with lib.GpuSim(cyl(nr, 0), 0) as g:
        st = bound_state(g, g.cfg, torch)
        out = torch.empty(g.project_count(perp, 3), dtype=torch.float64, device="cuda:0")
        res["abel_whole"] = dict(timed(lambda: g.project(perp, fields, dbuf_ptr=out.data_ptr()), g.synchronize, a.reps),
                                 nz=nz, nr=nr, nfields=3)
        del st
    rows = nr // a.world
    img = torch.zeros(3 * nr * nz, dtype=torch.float64, device="cuda:0")
    for tag, rank in (("abel_part_lowest_rank", 0), ("abel_part_highest_rank", a.world - 1)):
        part = (rank * rows, nr, int(rank == a.world - 1), 0.0)
        with lib.GpuSim(cyl(rows, rank * rows), 0) as g:
            st = bound_state(g, g.cfg, torch)
            k = timed(lambda: g.project_part(perp, fields, part, dimg_ptr=img.data_ptr()), g.synchronize, a.reps)
            res[tag] = dict(k, nz=nz, rows=rows, world=a.world, rank=rank, nfields=3)
            del st
    # the chain over two ranks on one GPU
    half = nr // 2
    with lib.GpuSim(cyl(half, 0), 0) as g0, lib.GpuSim(cyl(half, half), 0) as g1:
        s0, s1 = bound_state(g0, g0.cfg, torch), bound_state(g1, g1.cfg, torch)

        def chain():
            img.zero_()
            g0.project_part(perp, fields, (0, nr, 0, 0.0), dimg_ptr=img.data_ptr())
            g0.synchronize()
            g1.project_part(perp, fields, (half, nr, 1, 0.0), dimg_ptr=img.data_ptr())

        res["abel_chain_two_ranks_one_gpu"] = dict(timed(chain, g1.synchronize, a.reps), nz=nz, nr=nr, nfields=3)
        assert bool(torch.isfinite(img).all())
        del s0, s1

    nx, ny, nzl = (int(x) for x in a.box.split("x"))
    cfg = abi.make_config(3, [nx, ny, nzl], abi.EQGLM, abi.FLUX_RS_HLLD, dx=1.0 / nx, strict_fp=0)
    one = [("coldens", 1, -1, 1.0, 0.0)]
    with lib.GpuSim(cfg, 0) as g:
        st = bound_state(g, cfg, torch)
        out = torch.zeros(g.project_count(2, 1), dtype=torch.float64, device="cuda:0")
        res["box"] = {"nx": nx, "ny": ny, "nz_local": nzl}
        res["box"]["whole_axis2_rho"] = timed(lambda: g.project(2, one, dbuf_ptr=out.data_ptr()), g.synchronize, a.reps)
        for tag, last in (("part_middle_axis2_rho", 0), ("part_last_axis2_rho", 1)):
            part = (nzl, 8 * nzl, last, 0.0)
            res["box"][tag] = timed(lambda: g.project_part(2, one, part, dimg_ptr=out.data_ptr()), g.synchronize, a.reps)
        del st
    print(json.dumps(res))


if __name__ == "__main__":
    main()
