"""Every 2-D instance of both stage kernels, of both builds, against the ORACLE (table: instances_2d_cases.py).

test_every_hd_instantiation_3d / test_every_mhd_instantiation_3d (test_gpu_parity.py) run every instance of the 3-D
path, because this compiler has miscompiled single instances (csrc/Makefile).  This file does the same for what a 2-D
grid runs: the 3-D instance down its run-time `noz` path (Cartesian), the CYL instances of k_stage_rows2 (cylindrical
(z,R): 78 per build), and the instances of the cell-per-thread kernel k_stage in both geometries.  Each case is three
steps at the smallest shape that runs a full x tile and the remainder wavefront in one launch.

Per case, for the rows kernel (default environment) and for the cell-per-thread kernel (PION_STAGE_KERNEL=cell,
PION_ROWS_2D=0):
  strict build  bit for bit against the oracle, every time step equal; the Euler solvers that call exp / log / pow
                (linear, exact, hybrid) within 1e-9 of each variable's scale instead (the gate of test_hd_exact_hybrid),
                and for them rows kernel == cell kernel bit for bit: both call the same device library;
  fast build    within 3e-11 of each variable's scale (the gate of test_cyl_rows_kernel_fast_vs_oracle and
                test_2d_rows_kernel_fast_vs_oracle; 1e-9 for those three solvers), on inputs whose 1-ulp amplification
                in the oracle is <= 5e-12 (test_instances_2d_cases.py); then rows against cell: finite and within 1e-12
                (the gate of _fast_rows_vs_cell);
  both          after the last step, the time steps the full stage left behind equal what k_dt computes from the state
                (as test_fused_dt_equals_dt_kernel)."""
import numpy as np
import pytest

import instances_2d_cases as ic
from test_gpu_parity import run_pair

pytestmark = pytest.mark.gpu

CASES = list(ic.all_cases())
KERNEL_ENV = {"rows": {}, "cell": {"PION_STAGE_KERNEL": "cell", "PION_ROWS_2D": "0"}}


def _run(c, strict, kernel, monkeypatch):
    """three steps of one kernel against the oracle; returns the device's final state"""
    for k in ("PION_STAGE_KERNEL", "PION_ROWS_2D", "PION_ROWS"):
        monkeypatch.delenv(k, raising=False)
    for k, v in KERNEL_ENV[kernel].items():
        monkeypatch.setenv(k, v)
    cfg, P = ic.case(*c, strict)
    out = {}

    def after(g):
        fused = g.calc_dt()
        g.device_ptr(0)          # invalidates the cached minima -> the next call runs k_dt
        kern = g.calc_dt()
        assert fused == kern, (kernel, fused, kern)
        out["state"] = g.download(0)

    eq, solver = c[1], c[2]
    if strict and not ic.uses_libm(eq, solver):
        run_pair(cfg, P, ic.NSTEPS, after=after)
    else:
        tol = ic.GATE_LIBM if strict else ic.fast_gate(*c)
        run_pair(cfg, P, ic.NSTEPS, strict=False, tol=tol, after=after)
    return cfg, out["state"]


@pytest.mark.parametrize("strict", [1, 0], ids=["strict", "fast"])
@pytest.mark.parametrize("c", CASES, ids=[ic.case_id(*c) for c in CASES])
def test_2d_instance(c, strict, monkeypatch):
    cfg, rows = _run(c, strict, "rows", monkeypatch)
    _, cell = _run(c, strict, "cell", monkeypatch)
    assert np.isfinite(rows).all() and np.isfinite(cell).all()
    if strict:
        # (bit for bit through the oracle already where no libm call is involved)
        assert np.array_equal(rows, cell), "rows and cell kernel: %d values differ, max abs %g" % (
            (rows != cell).sum(), np.abs(rows - cell).max())
    else:
        scale = np.abs(cell).reshape(cfg.nvar, -1).max(axis=1).reshape(-1, 1, 1, 1) + 1e-300
        err = np.max(np.abs(rows - cell) / scale)
        assert err <= ic.GATE_ROWS_VS_CELL, err
