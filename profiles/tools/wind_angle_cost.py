"""Cost of a rotating-star (LGM99) wind source on a 512^3 Euler grid (run under rocprofv3 --kernel-trace --stats):
the per-update state launch of a rotating source (k_wind_state_angle) beside that of a constant source
(k_wind_state), both of radius 20 cells (~33.5 k cells) at the origin, a cell corner, so that no member cell lies
on the equator."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from pion_amd import abi, lib, problems, wind


def main(n=512, updates=20):
    L = 1.0e17
    cfg = abi.make_config(3, [n, n, n], abi.EQEUL, abi.FLUX_FVS, ntracer=1, gamma=5.0 / 3.0, cfl=0.3,
                          xmin=(-L, -L, -L), xmax=(L, L, L), bcs=["outflow"] * 6, refvec=[1.0] * 6, min_temp=5.0e3)
    r = 20.0 * cfg.dx
    const = wind.WindSource(pos=(0.0, 0.0, 0.0), radius=r, mdot=1.0e-6, vinf=1000.0, Tw=2.5e4, Rstar=7.0e11,
                            tracers=[1.0])
    cols = {c: np.zeros(2) for c in wind.COLUMNS}
    cols.update(time=np.array([-1.0e12, 1.0e12]), Teff=np.array([2.5e4, 3.0e4]),
                Mdot=np.array([6.3e19, 7.5e19]), vrot=np.array([1.5e7, 1.8e7]), vcrit=np.array([3.0e7, 3.0e7]),
                vinf=np.array([1.0e8, 0.9e8]), R=np.array([7.0e11, 7.0e11]))
    rot = wind.WindSource(pos=(0.0, 0.0, 0.0), radius=r, tracers=[1.0], type=wind.ANGLE,
                          evolution=wind.WindEvolution(cols), elements=[None], update_freq=1.0, xi=-0.43)
    P = problems.alloc(cfg)
    P[abi.RO], P[abi.PG] = 1.0e-23, 1.0e-10
    with lib.GpuSim(cfg, 0) as g:
        g.upload(P)
        g.add_wind_source(const)
        g.add_rotating_wind_source(rot)
        n0 = g.get_wind_cells(0)[0].size
        n1 = g.get_wind_cells(1)[0].size
        for k in range(updates):
            g.update_bcs(1.0e9 * k, 2, 2)
        g.synchronize()
    print("wind cells: constant %d, rotating %d" % (n0, n1))


def stats_to_json(csv_path, what):
    """the kernel_stats.csv of a rocprofv3 --stats run as the JSON record kept under profiles/"""
    import csv
    import json
    rows = []
    with open(csv_path) as f:
        for r in csv.DictReader(f):
            rows.append(dict(kernel=r["Name"], calls=int(r["Calls"]), total_ms=float(r["TotalDurationNs"]) * 1e-6,
                             mean_us=float(r["AverageNs"]) * 1e-3, min_us=float(r["MinNs"]) * 1e-3,
                             max_us=float(r["MaxNs"]) * 1e-3))
    return json.dumps(dict(what=what, kernels=rows), indent=1)


if __name__ == "__main__":
    main(*(int(a) for a in sys.argv[1:]))
