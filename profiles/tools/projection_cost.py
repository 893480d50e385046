#!/usr/bin/env python3
"""Kernel time of the projected images against the least the kernels have to do (DESIGN.md s6e;
profiles/projection.json):
    profiles/tools/projection_cost.py [--abel 4096x2048] [--box 512] [--reps 20]
Abel: a cylindrical (z,R) Euler + 1 tracer grid of NZ x NR cells, three fields (rho, rho^2, rho TR0), one call.  Its
floor is the largest of: the fp64 issue time of the segment terms (6 unfused operations each: the rule forbids
contraction; 39.3e12 fp64 instruction-lanes per second, half the 78.6 TFLOP/s vector peak, which counts an FMA as
two), one read of the variables used at the 6.29 TB/s copy ceiling (DESIGN s4.1), and the weight evaluations (one
per (j, ir) pair, workgroup and field: no rate is claimed for those, they are counted).
Column sums: a GLM-MHD box of n^3 cells (fast build), one axis per call, with one field (rho) and with three (rho,
rho^2, p: two variables).  Floor: one read of the variables used at 6.29 TB/s.
Each call is timed --reps times after a warm-up, host clock from the call to a synchronised device (a call is one
launch; the launch itself is a few microseconds of the milliseconds measured).  The states are uniform random numbers
made on the device and bound to the handle.  Prints one JSON line."""
import argparse
import json
import os
import statistics
import sys
import time

HERE = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, HERE)

COPY_CEILING = 6.29e12      # bytes per second, DESIGN s4.1
FP64_LANES = 39.3e12        # fp64 instruction-lanes per second (78.6 TFLOP/s counts an FMA as two)


def timed(fn, sync, reps):
    fn()
    sync()
    out = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        sync()
        out.append(time.perf_counter() - t0)
    return {"median_ms": 1e3 * statistics.median(out), "min_ms": 1e3 * min(out), "max_ms": 1e3 * max(out)}


def bound_state(g, cfg, torch):
    """uniform random numbers in [0.5, 1.5) made on the device, bound as P and Ph"""
    n = cfg.nvar * g.ncell
    st = torch.rand(n, dtype=torch.float64, device="cuda:0") + 0.5
    g.bind_device_state(st.data_ptr(), st.data_ptr())
    return st


def cells_crossed(nz, nr, dx, zmin, deg, n_extra):
    """cells every ray of the inclined image crosses, counted from the geometry (numpy, no walk): the columns the ray
    spans inside the grid plus the rows it climbs on its incoming and on its outgoing branch -- every column or row
    boundary crossed is one more cell.  (Equal to the count of the walk of tests/angle_projection_restate.py on 70 x 37
    and 40 x 20 at 41 degrees and on 24 x 16 at 20 degrees: 269006, 45040 and 32684 cells.)"""
    import numpy as np
    tn = np.tan(np.deg2rad(deg))
    zmax, rmax = zmin + nz * dx, nr * dx
    pz = (zmin - n_extra * dx) + (np.arange(nz + 2 * n_extra) + 0.5) * dx
    total = 0
    for j in range(nr):
        b = (j + 0.5) * dx
        S = np.sqrt(rmax * rmax - b * b) / tn
        lo, hi = np.maximum(zmin, pz - S), np.minimum(zmax, pz + S)
        ok = hi > lo
        R = lambda z: np.sqrt(b * b + (z - pz) ** 2 * tn * tn)
        cols = np.ceil((hi - zmin) / dx) - np.floor((lo - zmin) / dx)
        row = lambda z: np.minimum(np.floor(R(z) / dx), nr - 1)
        rows_in = np.where(hi > pz, row(hi) - row(np.maximum(pz, lo)), 0)
        rows_out = np.where(lo < pz, row(lo) - row(np.minimum(pz, hi)), 0)
        total += int(np.where(ok, cols + rows_in + rows_out, 0).sum())
    return total


# issue cycles of one wavefront instruction (profiles/r02_valu_rates.txt): v_sqrt_f64 / v_rsq_f64 / v_rcp_f64 11.7; 1024
# SIMDs at the 1.7 GHz the chip sustains under fp64 load
TRANS_CYCLES, SIMD_CYCLES_PER_S = 11.7, 1024 * 1.7e9


def angle_cost(a, torch, abi, lib):
    """pion_gpu_project_angle on a cylindrical Euler + 1 tracer grid, three fields, per angle: median of --reps calls
    after a warm-up.  Floor: 8 fp64 square roots and 3 divisions per cell crossed, each counted as ONE transcendental
    instruction (the rsq / rcp seed; the Newton steps that make them IEEE are not counted), 64 cells per instruction"""
    nz, nr = (int(x) for x in a.abel.split("x"))
    cfg = abi.make_config(2, [nz, nr], abi.EQEUL, abi.FLUX_RSroe, ntracer=1, coord_sys=2, dx=1.0 / nr, strict_fp=0,
                          bcs=["outflow", "outflow", "axisymmetric", "outflow"])
    fields = [("coldens", 1, -1, 1.0, 0.0), ("emmeasure", 2, -1, 1.0, 0.0), ("windcol", 1, 5, 1.0, 0.0)]
    out = {}
    with lib.GpuSim(cfg, 0) as g:
        st = bound_state(g, cfg, torch)
        for deg in (float(x) for x in a.angle.split(",")):
            n, n_extra = g.project_angle_count(deg, 3)
            buf = torch.empty(n, dtype=torch.float64, device="cuda:0")
            k = timed(lambda: g.project_angle(deg, fields, dbuf_ptr=buf.data_ptr()), g.synchronize, a.reps)
            assert g.project_angle_status() == 0 and bool(torch.isfinite(buf).all())
            cells = cells_crossed(nz, nr, cfg.dx, 0.0, deg, n_extra)
            k.update(nz=nz, nr=nr, nfields=3, n_extra=n_extra, pixels=n // 3, cells_crossed=cells,
                     cells_per_pixel=cells / (n // 3), cells_per_s=cells / (1e-3 * k["median_ms"]),
                     floor_issue_ms=1e3 * (8 + 3) * TRANS_CYCLES * cells / 64 / SIMD_CYCLES_PER_S)
            k["ratio_to_issue_floor"] = k["median_ms"] / k["floor_issue_ms"]
            out["%g" % deg] = k
            del buf
        del st
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--abel", default="4096x2048")
    ap.add_argument("--box", type=int, default=512)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--angle", default="", help="degrees, comma separated: time the inclined projection of the --abel grid "
                    "at these angles (profiles/projection_angle.json) instead of the perpendicular images")
    a = ap.parse_args()
    import torch
    from pion_amd import abi, lib
    res = {"gpu_lib": os.environ.get("PION_GPU_LIB", "in-tree"), "reps": a.reps}
    if a.angle:
        res["angle"] = angle_cost(a, torch, abi, lib)
        print(json.dumps(res))
        return

    nz, nr = (int(x) for x in a.abel.split("x"))
    cfg = abi.make_config(2, [nz, nr], abi.EQEUL, abi.FLUX_RSroe, ntracer=1, coord_sys=2, dx=1.0 / nr, strict_fp=0,
                          bcs=["outflow", "outflow", "axisymmetric", "outflow"])
    fields = [("coldens", 1, -1, 1.0, 0.0), ("emmeasure", 2, -1, 1.0, 0.0), ("windcol", 1, 5, 1.0, 0.0)]
    with lib.GpuSim(cfg, 0) as g:
        st = bound_state(g, cfg, torch)
        out = torch.empty(g.project_count(abi.PROJ_AXIS_PERP, 3), dtype=torch.float64, device="cuda:0")
        k = timed(lambda: g.project(abi.PROJ_AXIS_PERP, fields, dbuf_ptr=out.data_ptr()), g.synchronize, a.reps)
        assert bool(torch.isfinite(out).all())
        # a ray of row j >= 1 starts at segment j - 1 (dx is a power of two here): nr - j + 1 segments; row 0: nr
        terms = 3 * nz * (nr + sum(nr - j + 1 for j in range(1, nr)))
        tiles_z = -(-nz // 256)   # a workgroup: 16 impact rows x 256 z cells
        k.update(nz=nz, nr=nr, nfields=3, segment_terms=terms,
                 floor_issue_ms=1e3 * 6 * terms / FP64_LANES,
                 floor_read_ms=1e3 * 2 * 8 * nz * nr / COPY_CEILING,          # rho and the tracer, once
                 weight_evaluations=3 * tiles_z * (terms // (3 * nz)),
                 # a lane walks the rows from its tile's first segment to the last, once per field
                 field_evaluations=sum(3 * nz * (nr - max(j0 - 1, 0)) for j0 in range(0, nr, 16)))
        k["ratio_to_issue_floor"] = k["median_ms"] / k["floor_issue_ms"]
        res["abel"] = k
        del st, out

    n = a.box
    cfg = abi.make_config(3, [n, n, n], abi.EQGLM, abi.FLUX_RS_HLLD, dx=1.0 / n, strict_fp=0)
    one = [("coldens", 1, -1, 1.0, 0.0)]
    three = one + [("emmeasure", 2, -1, 1.0, 0.0), ("pressure", 0, abi.PG, 1.0, 0.0)]
    with lib.GpuSim(cfg, 0) as g:
        st = bound_state(g, cfg, torch)
        out = torch.empty(g.project_count(0, 3), dtype=torch.float64, device="cuda:0")
        res["box"] = {"n": n, "nvar": cfg.nvar}
        for axis in (0, 1, 2):
            for tag, fl, nvars in (("rho", one, 1), ("rho_rho2_p", three, 2)):
                k = timed(lambda: g.project(axis, fl, dbuf_ptr=out.data_ptr()), g.synchronize, a.reps)
                k["floor_read_ms"] = 1e3 * nvars * 8 * n ** 3 / COPY_CEILING
                k["ratio_to_read_floor"] = k["median_ms"] / k["floor_read_ms"]
                k["GB_per_s_of_needed_bytes"] = nvars * 8 * n ** 3 / (1e-3 * k["median_ms"]) / 1e9
                res["box"]["axis%d_%s" % (axis, tag)] = k
        assert bool(torch.isfinite(out).all())
    print(json.dumps(res))


if __name__ == "__main__":
    main()
