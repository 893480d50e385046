#!/usr/bin/env python3
"""Generates cooling_forms.npz: the cooling functions of mp_only_cooling other than the tabulated one (EP.cooling =
4..7, and KI02 through flag 7's form) from oracle/_ref, i.e. from the REFERENCE's own mp_only_cooling object compiled
as it lies, with the product's pion_host_cooling_curve_rate (or, for KI02, a callback computing KI02's Lambda) as its
CIE curve.  Run in the build container only (the reference does not travel):

    make -C oracle ref && python tests/golden/make_golden_cooling_forms.py

Cases and seeds: tests/cooling_forms_cases.py.  See README_cooling_forms.md for what the arrays hold."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from pion_amd import cooling  # noqa: E402
import cooling_forms_cases as cf  # noqa: E402


def main():
    out = {}
    # cooling-only vectors, flags 4..7 on both curves
    for ci, cname in enumerate(cf.CURVES):
        cf.set_curve(cname)
        with cf.RefCieCurve(cf.host_curve_fn()):
            for flag in cf.FLAGS:
                key = "f%d_%s_" % (flag, cname)
                rho, pg, dt = cf.cool_states(cf.cool_seed(flag, ci), cooling.curve_rate, flag)
                p, tmp = cf.ref_cool_only(cf.cool_cfg(flag), rho, pg, dt)
                out[key + "rho"], out[key + "pg"], out[key + "dt"] = rho, pg, dt
                out[key + "p"], out[key + "t_mp"] = p, tmp
                print(key, "done")
    # KI02 through flag 7's form
    with cf.RefCieCurve(cf.ki02_lambda_scalar):
        rho, pg, dt = cf.ki02_states()
        p, tmp = cf.ref_cool_only(cf.ki02_cfg(7), rho, pg, dt)
        out["ki02_rho"], out["ki02_pg"], out["ki02_dt"], out["ki02_p"], out["ki02_t_mp"] = rho, pg, dt, p, tmp
    # whole steps and the end state
    for name, (flag, cname) in cf.STEP_CASES.items():
        cf.set_curve(cname)
        with cf.RefCieCurve(cf.host_curve_fn()):
            cfg, P = cf.step_case(name)
            out[name + "_dt"], out[name + "_P"] = cf.ref_steps(cfg, P, cf.NSTEPS)
            print(name, out[name + "_dt"])
    name, flag, cname, nsteps = cf.END_CASE
    cf.set_curve(cname)
    with cf.RefCieCurve(cf.host_curve_fn()):
        cfg, P, nsteps = cf.end_case()
        out[name + "_dt"], out[name + "_P"] = cf.ref_steps(cfg, P, nsteps)
        print(name, out[name + "_dt"][[0, -1]])
    np.savez_compressed(os.path.join(HERE, "cooling_forms.npz"), **out)


if __name__ == "__main__":
    main()
