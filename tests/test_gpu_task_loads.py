"""The tasks of k_stage_rows2 request their data as one batch ahead of the solve (stage_rows2.h): the y task asks for
the rows C and, in its lower mode, M together with F; the x task of the plain second-order instances asks for the
start-of-step state in every launch, whether it is used or not.  Only the order of loads changed, so every result is
what it was: the grids here are the smallest on which a moved load can go wrong.

20 x 5 x 4: a remainder tile only, several row groups per wavefront, a last group of one row at two rows per wavefront.
66 x 6 x 5: one full x tile and a remainder of 4.  With PION_ROWS = 1, 2, 3 the lower mode -- where M and the early C
are read -- runs on every row, every second and every third.  With outflow faces the rows M and C of the first and
last group are ghost rows.  With wind cells (plain_cells == 0) the start-of-step loads are issued and dropped.

Strict build: == the oracle.  Fast build: the same bits whatever the rows per wavefront, and inside the gate of
tests/test_gpu_xtile.py against the oracle (its test is called on these grids: no number is defined here)."""
import functools

import numpy as np
import pytest

import test_gpu_xtile as xtile
from pion_amd import abi, cooling, driver, problems
from test_gpu_parity import run_pair, _gpu

pytestmark = pytest.mark.gpu

GRIDS_3D = [[20, 5, 4], [66, 6, 5]]
IDS_3D = ["20x5x4", "66x6x5"]


def _states(cfg, P, rows_list, monkeypatch, setup=None, first_dt_limit=None):
    """the state after three steps, for each of the rows per wavefront"""
    out = []
    for rows in rows_list:
        monkeypatch.setenv("PION_ROWS", rows)
        with _gpu(cfg) as g:
            if setup:
                setup(g)
            sc = driver.SimControl(g, cfg)
            sc.first_step_dt_limit = first_dt_limit
            sc.init(P)
            sc.time_int(3)
            out.append((g.download(0), sc.simtime))
    monkeypatch.delenv("PION_ROWS", raising=False)
    return out


def _same(out, rows_list):
    for (A, t), rows in zip(out[1:], rows_list[1:]):
        assert t == out[0][1], rows
        assert np.array_equal(A, out[0][0]), rows


def _xtile_gate(monkeypatch, cfg, P, **kw):
    """test_gpu_xtile's fast-build gate against the oracle, on this configuration"""
    monkeypatch.setattr(xtile, "_case", lambda name, ng, strict: (cfg, P))
    if kw:
        monkeypatch.setattr(xtile, "run_pair", functools.partial(run_pair, **kw))
    xtile.test_full_xtile_fast_vs_oracle("this", list(cfg.ng)[:cfg.ndim])


# ---- 3-D GLM-MHD, HLLD, periodic, second order -------------------------------------------------------------------
@pytest.mark.parametrize("ng", GRIDS_3D, ids=IDS_3D)
def test_glm_3d_strict_equals_the_oracle(ng):
    cfg, P = problems.mhd_blast_generic(ng, abi.EQGLM, abi.FLUX_RS_HLLD, strict_fp=1)
    run_pair(cfg, P, 3)


@pytest.mark.parametrize("ng", GRIDS_3D, ids=IDS_3D)
def test_glm_3d_fast_same_bits_for_1_2_3_rows(ng, monkeypatch):
    cfg, P = problems.mhd_blast_generic(ng, abi.EQGLM, abi.FLUX_RS_HLLD, strict_fp=0)
    rows = ["1", "2", "3"]
    _same(_states(cfg, P, rows, monkeypatch), rows)


@pytest.mark.parametrize("ng", GRIDS_3D, ids=IDS_3D)
def test_glm_3d_fast_inside_the_xtile_gate(ng, monkeypatch):
    cfg, P = problems.mhd_blast_generic(ng, abi.EQGLM, abi.FLUX_RS_HLLD, strict_fp=0)
    _xtile_gate(monkeypatch, cfg, P)


# ---- the other equation sets on 20 x 5 x 4 -----------------------------------------------------------------------
def test_ideal_mhd_3d_strict_equals_the_oracle():
    cfg, P = problems.mhd_blast_generic(GRIDS_3D[0], abi.EQMHD, abi.FLUX_RS_HLLD, strict_fp=1)
    run_pair(cfg, P, 3)


def test_euler_roe_3d_reflecting_outflow_strict_equals_the_oracle():
    """reflecting / outflow faces: the rows M and C of the first and the last row group are ghost rows"""
    cfg, P = problems.hd_blast_box(GRIDS_3D[0], solver=abi.FLUX_RSroe, strict_fp=1)
    assert [cfg.bc_type[f] for f in range(6)] == [abi.BC_REFLECTING, abi.BC_OUTFLOW] * 3
    run_pair(cfg, P, 3)


def test_first_order_3d_strict_equals_the_oracle():
    """OA1 / OA1: stencil and start-of-step array are one array"""
    cfg, P = problems.mhd_blast_generic(GRIDS_3D[0], abi.EQGLM, abi.FLUX_RS_HLLD, strict_fp=1)
    cfg.sp_ooa = cfg.tm_ooa = 1
    run_pair(cfg, P, 3)


# ---- a grid with internal-boundary cells: plain_cells == 0 -------------------------------------------------------
def _wind(strict, cool):
    cfg, P, (idx, st), dtl = problems.wind3d(8, strict_fp=strict)
    T, tabs, sl = cooling.build_tables(cfg.min_temp, cfg.max_temp)
    if not cool:
        cfg.cooling = 0
        cfg.mp_timestep_limit = 0

    def setup(s):
        if cool:
            s.set_cooling_tables(T, tabs, sl)
        s.set_wind_cells(idx, st)
    return cfg, P, setup, dtl


def test_wind3d_with_its_wind_cells_strict_equals_the_oracle():
    cfg, P, setup, dtl = _wind(1, True)
    run_pair(cfg, P, 3, first_dt_limit=dtl, setup=setup)


def test_wind_cells_without_cooling_fast_drops_the_start_of_step_loads(monkeypatch):
    """Wind3D's grid and wind cells without its cooling is the PLAIN second-order instance with plain_cells == 0: in
    the fast build the x task requests the start-of-step state, drops it and zeroes dU behind the solve"""
    cfg, P, setup, dtl = _wind(0, False)
    rows = ["1", "2", "3"]
    _same(_states(cfg, P, rows, monkeypatch, setup=setup, first_dt_limit=dtl), rows)
    _xtile_gate(monkeypatch, cfg, P, setup=setup, first_dt_limit=dtl)


# ---- 2-D: Cartesian and cylindrical ------------------------------------------------------------------------------
def _case_2d(kind, strict):
    if kind == "glm_70x7":
        return problems.mhd_blast_generic([70, 7], abi.EQGLM, abi.FLUX_RS_HLLD, strict_fp=strict)
    return problems.blast_axi2d(16, abi.EQGLM, abi.FLUX_RS_HLLD, strict_fp=strict)


KINDS_2D = ["glm_70x7", "glm_axi_16x8"]


@pytest.mark.parametrize("kind", KINDS_2D)
def test_2d_strict_equals_the_oracle(kind):
    cfg, P = _case_2d(kind, 1)
    run_pair(cfg, P, 3)


@pytest.mark.parametrize("kind", KINDS_2D)
def test_2d_fast_same_bits_for_1_2_16_rows(kind, monkeypatch):
    cfg, P = _case_2d(kind, 0)
    rows = ["1", "2", "16"]
    _same(_states(cfg, P, rows, monkeypatch), rows)
