"""Cost of moving wind sources on a 512^3 Euler grid (run under rocprofv3 --kernel-trace --hip-trace --stats): two
sources of radius 20 cells on orbits ("orbit"), or the same two sources held still ("static"), and `updates` boundary
updates at advancing times.  A moving source adds per update k_wind_unflag over its old box, the hipcub select over
its new box and k_wind_cells_dn; its k_wind_state reads the count from the device.  The script waits for the device
only after the last update."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from pion_amd import abi, lib, problems, wind

YEAR = 3.1558150e7


def main(mode="orbit", n=512, updates=30):
    n, updates = int(n), int(updates)
    L = 1.0
    cfg = abi.make_config(3, [n, n, n], abi.EQEUL, abi.FLUX_FVS, ntracer=1, gamma=5.0 / 3.0, cfl=0.3,
                          xmin=(-L, -L, -L), xmax=(L, L, L), bcs=["outflow"] * 6, refvec=[1.0] * 6, min_temp=5.0e3)
    dx = cfg.dx
    srcs = []
    for x in (0.25, -0.25):
        # binary about the origin (problems.binary_orbit); period 1 s: one update per 1e-3 s moves ~0.8 cells
        orbit = problems.binary_orbit(x, 1.0 / YEAR) if mode == "orbit" else None
        srcs.append(wind.WindSource(pos=(x, 0.0, 0.3 * dx), radius=20.0 * dx, mdot=1.0e-7, vinf=1500.0, Tw=3.0e4,
                                    Rstar=1.0e-3, tracers=[1.0], orbit=orbit))
    P = problems.alloc(cfg)
    P[abi.RO], P[abi.PG] = 1.0, 1.0
    with lib.GpuSim(cfg, 0) as g:
        g.upload(P)
        for s in srcs:
            g.add_wind_source(s)
        g.update_bcs(0.0, 2, 2, assign=1)
        g.synchronize()
        for k in range(updates):
            g.update_bcs(1.0e-3 * (k + 1), 2, 2)
        g.synchronize()
        cells = [g.get_wind_cells(k)[0].size for k in range(len(srcs))]
        pos = [g.get_wind_source_pos(k) for k in range(len(srcs))]
    print("mode %s: wind cells %s, positions / dx %s" % (mode, cells, [[p / dx for p in q[:2]] for q in pos]))


if __name__ == "__main__":
    main(*sys.argv[1:])
