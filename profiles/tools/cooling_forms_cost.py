#!/usr/bin/env python3
"""What the cooling functions of mp_only_cooling cost on the device, per launch (needs a GPU):

    python profiles/tools/cooling_forms_cost.py [--n 256] [--steps 3] [--out profiles/cooling_forms.json]

256^3 Euler + tracer (Wind3D's configuration, FVS, fast build, the rows kernel), two temperature distributions --
M3's initial state without its wind source, and a hot blast (tests/cooling_forms_cases._blob: 3e3 - 3e4 K gas with a
3e8 K blob, so that both extrapolated ends of a curve are evaluated) -- and on each, from the same state in the same
process:
    flag 8 (tables: the baseline), flag 6 on the 64-knot uniform curve (interval from the knot spacing), flag 7 on the
    9-knot curve (bisection), flag 2 (KI02: two exponentials and a root, no table).
HIP events of the library's own timing slots around the cooling launch of each stage (k_cooling_dE<EQ,NTR,FORM>, FORM =
table, curve or KI02 by the flag; k_cooling_dE / k_cooling_dE_form in a library from before the kernels were unified,
which PION_GPU_LIB may name for an A/B run; Euler has no prepass, which shares the slot) and around the cooling-time
launch behind each full step (k_dt_mp<FORM>, formerly k_dt_mp / k_dt_mp_form; timing is switched on after the first time
step, so k_dt is not in it).  One warm-up step is not timed."""
import argparse
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from pion_amd import abi, cooling, driver, lib, problems  # noqa: E402
import cooling_forms_cases as cf  # noqa: E402

RUNS = [("flag8_tables", 8, None), ("flag6_uniform64", 6, "uniform64"), ("flag7_knots9_bisect", 7, "knots9"),
        ("flag2_ki02", 2, None)]


def states(n):
    cfg, P, _, _ = problems.wind3d(n, strict_fp=0)
    X, Y, Z = problems.mesh(cfg)
    L = cfg.dx * n
    s = cf._L / L
    hot = cf._blob(cfg, (X - cfg.xmin[0]) * s, (Y - cfg.xmin[1]) * s, (Z - cfg.xmin[2]) * s,
                   (0.5 * cf._L, 0.5 * cf._L, 0.5 * cf._L), ntr=cfg.ntracer)
    return cfg, {"m3_initial": P, "hot_blast": hot}


def measure(cfg, P, flag, cname, steps):
    cfg.cooling = flag
    with lib.GpuSim(cfg, 0) as g:
        if flag == 8:
            g.set_cooling_tables(*cooling.build_tables(cfg.min_temp, cfg.max_temp))
        elif cname is not None:
            g.set_cooling_curve(*cooling.build_curve(*cf.curve_knots(cname)))
        sc = driver.SimControl(g, cfg)
        sc.init(P)
        sc.calculate_timestep()
        sc.advance_time()
        g.synchronize()
        g.enable_timing(True)
        for _ in range(steps):
            sc.calculate_timestep()
            sc.advance_time()
        t = g.get_timing()
        g.enable_timing(False)
    return {"cooling_source_ms_per_launch": t["prepass_ms"], "cooling_source_launches": t["prepass_n"],
            "cooling_time_ms_per_launch": t["dt_ms"], "cooling_time_launches": t["dt_n"],
            "stage_ms_per_launch": t["stage_ms"]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=256)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cooling_forms.json"))
    a = ap.parse_args()
    cfg, sts = states(a.n)
    res = {"grid": [a.n] * 3, "workload": "Euler + 1 tracer, FVS, FKJ98, fast build, rows kernel; cooling-time limit on",
           "steps_timed": a.steps, "status": "measured", "runs": {}}
    for sname, P in sts.items():
        for rname, flag, cname in RUNS:
            res["runs"]["%s/%s" % (sname, rname)] = measure(cfg, P, flag, cname, a.steps)
            print(sname, rname, res["runs"]["%s/%s" % (sname, rname)], flush=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
