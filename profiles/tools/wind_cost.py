"""Cost of the device-built wind sources on a 512^3 Euler grid (run under rocprofv3 --kernel-trace --stats):
membership of one source (k_wind_count + the hipcub select + k_wind_cells) and the per-update state launch
(k_wind_state) for a source of radius 20 cells (~33.5 k cells)."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from pion_amd import abi, lib, problems, wind


def main(n=512, updates=20):
    L = 1.0
    cfg = abi.make_config(3, [n, n, n], abi.EQEUL, abi.FLUX_FVS, ntracer=1, gamma=5.0 / 3.0, cfl=0.3,
                          xmin=(-L, -L, -L), xmax=(L, L, L), bcs=["outflow"] * 6, refvec=[1.0] * 6, min_temp=5.0e3)
    src = wind.WindSource(pos=(0.0, 0.0, 0.0), radius=20.0 * cfg.dx, mdot=1.0e-7, vinf=1500.0, Tw=3.0e4,
                          Rstar=1.0e-3, tracers=[1.0])
    P = problems.alloc(cfg)
    P[abi.RO], P[abi.PG] = 1.0, 1.0
    with lib.GpuSim(cfg, 0) as g:
        g.upload(P)
        g.add_wind_source(src)
        idx, _ = g.get_wind_cells(0)
        for _ in range(updates):
            g.update_bcs(0.0, 2, 2)
        g.synchronize()
    print("wind cells: %d" % idx.size)


if __name__ == "__main__":
    main(*(int(a) for a in sys.argv[1:]))
