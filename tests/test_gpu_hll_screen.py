"""The screened HLLD -> HLL switch prepass against the dense one (PION_HLL_SCREEN=0), in two fresh child processes.

After every stage the switch array the prepass left (pion_gpu_get_hll_switch, ghost cells included) must be the same
bytes on both paths, and so must the final state -- in the strict and in the fast build: the flux arithmetic is the
same code on both paths.  The screen must really have been taken where it is admitted (0 < active blocks < blocks after
the first stage) and must not have been where it is not (wind cells, an inflow face)."""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

pytestmark = pytest.mark.gpu

NSTEPS = 3
# name: (builder, screened)
CASES = ["m1_96_fast", "m1_96_strict", "odd_fast", "odd_strict", "walls_fast", "walls_strict", "wind_fast", "inflow_fast"]
SCREENED = {c: not c.startswith(("wind", "inflow")) for c in CASES}


def build_case(name):
    from pion_amd import abi, problems
    kind, strict = name.rsplit("_", 1)
    strict = 1 if strict == "strict" else 0
    setup = None
    if kind == "m1_96":
        cfg, P = problems.mhd_blastwave(96, 3, strict_fp=strict)   # the benchmark's problem, two x tiles (62 + 34)
    else:
        # 80 x 72 x 64: a full x tile and a remainder tile of 18 cells
        cfg, P = problems.mhd_blast_generic((80, 72, 64), strict_fp=strict)
        if kind == "walls":
            for d in range(6):
                cfg.bc_type[d] = abi.BC_REFLECTING if d % 2 == 0 else abi.BC_OUTFLOW
        elif kind == "inflow":
            cfg.bc_type[0] = abi.BC_INFLOW
            cfg.bc_type[1] = abi.BC_OUTFLOW
        elif kind == "wind":
            nga = abi.ng_all(cfg)
            i0 = (nga[0] // 4) + nga[0] * ((nga[1] // 4) + nga[1] * (nga[2] // 4))
            idx = np.array([i0, i0 + 1, i0 + nga[0], i0 + nga[0] + 1], dtype=np.int64)
            st = np.tile(np.array([2.0, 5.0, 0.1, 0.0, 0.0, 0.7, 0.7, 0.3, 0.0]), (idx.size, 1))

            def setup(g):
                g.set_wind_cells(idx, st)
    return cfg, P, setup


def run_cases(out):
    """child process: every case for NSTEPS steps; the switch array after each stage, the screen's counts, the end state"""
    from pion_amd import abi, driver, lib
    res = {}
    for name in CASES:
        cfg, P, setup = build_case(name)
        with lib.GpuSim(cfg, 0) as g:
            if setup:
                setup(g)
            sc = driver.SimControl(g, cfg)
            sc.init(P)
            counts = []
            for step in range(NSTEPS):
                sc.calculate_timestep()
                dt = sc.dt
                for i, (sdt, ooa, full) in enumerate(((0.5 * dt, abi.OA1, 0), (dt, abi.OA2, 1))):
                    sc._stage(sdt, ooa, full)
                    res["%s/hll/%d/%d" % (name, step, i)] = g.get_hll_switch()
                    counts.append(g.get_hll_screen_counts())
                    sc.update_bcs(ooa, abi.OA2)
                sc.simtime += dt
                sc.last_dt = dt
                sc.timestep += 1
            res["%s/counts" % name] = np.array(counts, dtype=np.int64)
            res["%s/state" % name] = g.download(0)
    np.savez(out, **res)


def _child(tmp_path, tag):
    out = str(tmp_path / ("%s.npz" % tag))
    r = subprocess.run([sys.executable, os.path.abspath(__file__), out], env=dict(os.environ), cwd=ROOT,
                       capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    return np.load(out)


def test_screened_prepass_equals_dense_prepass(tmp_path, monkeypatch):
    monkeypatch.setenv("PION_HLL_SCREEN", "0")
    dense = _child(tmp_path, "dense")
    monkeypatch.delenv("PION_HLL_SCREEN")
    scr = _child(tmp_path, "screened")
    assert sorted(dense.files) == sorted(scr.files)
    for name in CASES:
        cd, cs = dense[name + "/counts"], scr[name + "/counts"]
        print(name, "active/blocks per stage:", [tuple(c) for c in cs])
        # the dense child never screens
        assert (cd[:, 0] == -1).all(), (name, cd)
        if SCREENED[name]:
            # the first stage after init has no summary; every later one is screened, and only part of the grid is active
            assert tuple(cs[0]) == (-1, 0), (name, cs)
            assert (cs[1:, 0] > 0).all() and (cs[1:, 0] < cs[1:, 1]).all(), (name, cs)
        else:
            assert (cs[:, 0] == -1).all(), (name, cs)
        nflag = 0
        for step in range(NSTEPS):
            for i in range(2):
                k = "%s/hll/%d/%d" % (name, step, i)
                a, b = dense[k], scr[k]
                nflag += int(a.sum())
                assert a.tobytes() == b.tobytes(), (k, int((a != b).sum()))
        assert nflag > 0, name   # the comparison is not one of empty arrays
        a, b = dense[name + "/state"], scr[name + "/state"]
        assert a.tobytes() == b.tobytes(), (name, float(np.nanmax(np.abs(a - b))))


if __name__ == "__main__":
    run_cases(sys.argv[1])
