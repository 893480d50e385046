"""The stage prepass on the device against the oracle, cell by cell, on the rough fields of prepass_cases.py.

Both run the OA1 half stage, the boundary update and the OA2 full stage with the same dt; test_prepass_cases.py shows
(without a GPU) that these fields put flagged and steep-but-unflagged cells into every class of cells in which the
kernels change their code shape, and no cell near a threshold.

  * SWITCH: pion_gpu_get_hll_switch after each stage == (div v < 0) & (gradp > 5) of the oracle's arrays at every cell of
    the array, ghosts included, in the strict and in the fast build; pion_gpu_get_hll_screen_counts shows the path: the
    3-D cases run twice, with the screen (second stage screened, as many active blocks as hll_screen.h's rule restated
    in numpy gives from the oracle's half-stage pressures) and with PION_HLL_SCREEN=0 (march / dense kernel in both
    stages).  march_3d is periodic with at most 3 blocks per axis: every block is a neighbour of every block, so all 12
    are active; screen_join (no periodic axis, blocks 3 x 2 x 3) keeps quiet blocks: 0 < active < total.  Ideal MHD
    (march_fit_*) leaves no pressure summary, its second stage is the march kernel's too.  Split stages: the planes /
    rows each part is the first to evaluate, against the oracle's whole stage, read between the parts and after both.
  * ETA: pion_gpu_get_hcorr_eta(axis) == the oracle's hcorr[axis] at every cell after each stage (OA1: edges are cell
    values, OA2: limited slopes): strict build bit for bit, the zeros in the last cell of every column included; fast
    build |eta_gpu - eta_orc| <= ETA_TOL s, s the larger |v_n| + c_fast (Euler: + c_s) of the interface's two cells.
    Measured on an MI355X over all eta cases, both stages and every axis: largest ratio 3.4e-16 (cyl_hcorr 3.363e-16,
    dense_hcorr 3.331e-16, roe_hcorr_tr 2.753e-16, roe_hcorr 2.562e-16, sph_hcorr 1.284e-16; far below 1e-12:
    contraction and the seeded roots and reciprocals only), ETA_TOL = 8 x 3.4e-16 = 2.72e-15.
  * CONSUMPTION: strict build, the states after each stage equal the oracle's bit for bit (either cell's flag makes the
    interface HLL; select_Hcorr_eta's neighbour look-ups); fast build, the rows kernel and PION_STAGE_KERNEL=cell agree
    to 1e-12 of each variable's scale (the gate of test_gpu_parity._fast_rows_vs_cell, on these two stages)."""
import contextlib
import copy
import os

import numpy as np
import pytest

import prepass_cases as pc
from pion_amd import abi

pytestmark = pytest.mark.gpu

ETA_TOL = 8 * 3.4e-16
BUILDS = pytest.mark.parametrize("strict", [1, 0], ids=["strict", "fast"])
WHOLE_SWITCH_CASES = [n for n in pc.SWITCH_CASES if not n.startswith("split")]
CONSUME_CASES = pc.FAST_STATE_CASES


@contextlib.contextmanager
def _env(**kw):
    """environment switches pion_gpu_create reads (None: unset), put back afterwards"""
    old = {k: os.environ.get(k) for k in kw}
    try:
        for k, v in kw.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


_GPU = {}


def gpu_run(name, strict, screen=True, kernel=None):
    """the device's two stages of case `name` with the oracle's dt, once per (case, build, switches): per stage the
    switch array, the screen's counts, eta per axis and the state the stage wrote; final: P after the last update"""
    key = (name, strict, screen, kernel)
    if key in _GPU:
        return _GPU[key]
    from pion_amd import lib
    orc = pc.oracle_run(name)
    cfg, P, info = pc.make(name, strict_fp=strict)
    nga = abi.ng_all(cfg)
    shp = (nga[2], nga[1], nga[0])
    out = {"stages": []}

    def record(g, i, S):
        if i == 2:
            out["final"] = g.download(0)
            return
        st = {"state": g.download(1 - i)}
        if cfg.solver == abi.FLUX_RS_HLLD:
            st["hll"] = g.get_hll_switch().reshape(shp)
            st["counts"] = g.get_hll_screen_counts()
        if cfg.artvisc == abi.AV_HCORR_FKJ98:
            st["eta"] = [g.get_hcorr_eta(a).reshape(shp) for a in range(cfg.ndim)]
        out["stages"].append(st)

    with _env(PION_HLL_SCREEN=None if screen else "0", PION_STAGE_KERNEL=kernel):
        with lib.GpuSim(cfg, 0) as g:
            out["own_dt"] = pc.two_stages(g, cfg, P, info["f"], t_dyn=orc["t_dyn"], record=record)
    _GPU[key] = out
    return out


def _assert_switch(name, i, got, want, where=None):
    bad = got != want
    if where is not None:
        bad &= where
    if bad.any():
        z, y, x = np.argwhere(bad)[0]
        raise AssertionError("%s stage %d: %d flags differ, first at (x, y, z) = (%d, %d, %d): device %d, oracle %d"
                             % (name, i, bad.sum(), x, y, z, got[z, y, x], want[z, y, x]))


# (PION_HLL_SCREEN=0 changes nothing for a case the screen is not admitted for)
SWITCH_RUNS = [(n, True) for n in WHOLE_SWITCH_CASES] + [(n, False) for n in WHOLE_SWITCH_CASES if n in pc.SCREENED_CASES]


@BUILDS
@pytest.mark.parametrize("name,screen", SWITCH_RUNS, ids=["%s-%s" % (n, "screen" if s else "noscreen") for n, s in SWITCH_RUNS])
def test_switch_equals_oracle_at_every_cell(name, screen, strict):
    orc = pc.oracle_run(name)
    run = gpu_run(name, strict, screen=screen)
    if strict:
        assert run["own_dt"] == orc["t_dyn"]
    counts = [st["counts"] for st in run["stages"]]
    print(name, "strict" if strict else "fast", "screen counts per stage:", counts,
          "flags set:", [int(st["hll"].sum()) for st in run["stages"]])
    for i, (g, o) in enumerate(zip(run["stages"], orc["stages"])):
        assert g["hll"].max() <= 1
        _assert_switch(name, i, g["hll"], pc.expected_switch(o))
    assert counts[0] == (-1, 0), counts
    if screen and name in pc.SCREENED_CASES:
        active, _ = pc.screen_blocks(orc["cfg"], orc["stages"][0]["state"])
        assert counts[1] == (int(active.sum()), active.size), (counts, int(active.sum()), active.size)
        assert 0 < counts[1][0] <= counts[1][1]
        if name == "screen_join":
            assert counts[1][0] < counts[1][1]
    else:
        assert counts[1] == (-1, 0), counts


def _ratio(cfg, S, axis, eg, eo):
    s = pc.cfast_plus_vn(cfg, S, axis)
    ax = 2 - axis
    nxt = np.concatenate([np.take(s, range(1, s.shape[ax]), axis=ax), np.take(s, [-1], axis=ax)], axis=ax)
    return np.abs(eg - eo) / np.maximum(s, nxt)


@BUILDS
@pytest.mark.parametrize("name", pc.ETA_CASES)
def test_eta_equals_oracle_at_every_cell(name, strict):
    orc = pc.oracle_run(name)
    cfg = orc["cfg"]
    run = gpu_run(name, strict)
    worst = 0.0
    for i, (g, o) in enumerate(zip(run["stages"], orc["stages"])):
        for a in range(cfg.ndim):
            eg, eo = g["eta"][a], o["eta"][a]
            assert (eo > 0).sum() > eo.size // 2 and (np.take(eo, -1, axis=2 - a) == 0).all()   # not a comparison of zeros
            if strict:
                bad = eg != eo
                assert not bad.any(), "%s stage %d axis %d: %d values differ, first at (z, y, x) = %s, max abs %g" % (
                    name, i, a, bad.sum(), np.argwhere(bad)[0].tolist(), np.abs(eg - eo).max())
            else:
                assert np.isfinite(eg).all()
                assert (np.take(eg, -1, axis=2 - a) == 0).all()
                r = _ratio(cfg, o["S"], a, eg, eo)
                worst = max(worst, float(r.max()))
                print("%s stage %d axis %d: max |eta_gpu - eta_orc| / s = %.3e" % (name, i, a, r.max()))
    if not strict:
        print("%s: largest ratio %.3e (ETA_TOL %.3e)" % (name, worst, ETA_TOL))
        assert worst <= ETA_TOL, (name, worst)


def _on_grid(cfg, A):
    sl = tuple(slice(cfg.nbc, -cfg.nbc) if a < cfg.ndim else slice(None) for a in (2, 1, 0))
    return A[(slice(None),) + sl]


@pytest.mark.parametrize("name", CONSUME_CASES)
def test_states_equal_oracle_strict(name):
    orc = pc.oracle_run(name)
    cfg = orc["cfg"]
    run = gpu_run(name, 1)
    for i, (g, o) in enumerate(zip(run["stages"], orc["stages"])):
        a, b = _on_grid(cfg, g["state"]), _on_grid(cfg, o["state"])
        bad = a != b
        assert not bad.any(), "%s stage %d: %d values differ, first at (var, z, y, x) = %s, max abs %g" % (
            name, i, bad.sum(), np.argwhere(bad)[0].tolist(), np.abs(a - b).max())
    assert np.array_equal(run["final"], orc["final"]), "%s: %d values differ after the last boundary update" % (
        name, (run["final"] != orc["final"]).sum())


@pytest.mark.parametrize("name", CONSUME_CASES)
def test_states_rows_kernel_vs_cell_kernel_fast(name):
    cfg = pc.oracle_run(name)["cfg"]
    rows, cell = gpu_run(name, 0), gpu_run(name, 0, kernel="cell")
    for i in range(2):
        a, b = rows["stages"][i]["state"], cell["stages"][i]["state"]
        a, b = _on_grid(cfg, a), _on_grid(cfg, b)
        scale = np.abs(b).reshape(cfg.nvar, -1).max(axis=1).reshape(-1, 1, 1, 1) + 1e-300
        assert np.isfinite(a).all()
        err = np.max(np.abs(a - b) / scale)
        print(name, "stage", i, "rows vs cell kernel: %.3e" % err)
        assert err <= 1e-12, (name, i, err)
        if "hll" in rows["stages"][i]:
            assert np.array_equal(rows["stages"][i]["hll"], cell["stages"][i]["hll"])


# --- split stages: the flags each part is the first to evaluate
class _Tap:
    """a halo exchange that reads the switch array between the interior part and the strips of every stage"""

    def __init__(self, comm):
        self.comm = comm
        self.seen = []

    def start(self, sim, which):
        self.comm.start(sim, which)

    def finish(self, sim):
        if self.comm.pending is not None:
            self.seen.append(sim.get_hll_switch())
        self.comm.finish(sim)

    def allreduce_min(self, a, b):
        return a, b


def _split_run(name, strict):
    from pion_amd import lib
    orc = pc.oracle_run(name)
    cfg, P, info = pc.make(name, strict_fp=strict)
    sa = cfg.ndim - 1
    cfg_s = copy.deepcopy(cfg)
    cfg_s.bc_type[2 * sa] = cfg_s.bc_type[2 * sa + 1] = abi.BC_SLAB
    if cfg.ndim == 3:
        from test_gpu_split_stage import SelfComm as Comm
    else:
        from test_gpu_slab2d_parts import SelfComm2D as Comm
    nga = abi.ng_all(cfg)
    shp = (nga[2], nga[1], nga[0])
    hll = []

    def record(g, i, S):
        if i < 2:
            hll.append(g.get_hll_switch().reshape(shp))
            assert g.get_hll_screen_counts() == (-1, 0)

    with lib.GpuSim(cfg_s, 0) as g:
        tap = _Tap(Comm(g, True))
        pc.two_stages(g, cfg_s, P, info["f"], t_dyn=orc["t_dyn"], record=record, comm=tap)
    assert len(tap.seen) == 3      # (one exchange per boundary update: init and the two stages; the last one feeds no stage)
    return orc, cfg, hll, [a.reshape(shp) for a in tap.seen[:2]]


@BUILDS
@pytest.mark.parametrize("name", ["split_3d", "split_2d"])
def test_switch_of_split_stages_equals_oracle(name, strict):
    """interior part: one range, the planes / rows [nb-1, n-nb+1); both strips: ONE launch of two ranges (3-D:
    k_prepass_hlld with a second cell range, 2-D: k_prepass_hlld_rows).  Together they evaluate the on-grid planes /
    rows -1 .. n of the slab axis, x (and y) ghosts included; the outermost ghost planes are nobody's.  Between the two
    parts the strips' planes still hold what the stage before left (zeros before the first)."""
    orc, cfg, hll, between = _split_run(name, strict)
    sa, nb = cfg.ndim - 1, cfg.nbc
    n = cfg.ng[sa]
    ix = pc.cell_indices(cfg)[sa]
    regions = {"lower strip": (-1, nb - 1), "interior": (nb - 1, n - nb + 1), "upper strip": (n - nb + 1, n + 1)}
    before = np.zeros_like(hll[0])
    for i, (got, o) in enumerate(zip(hll, orc["stages"])):
        want = pc.expected_switch(o)
        for k, (lo, hi) in regions.items():
            where = (ix >= nb + lo) & (ix < nb + hi)
            steep_not = (o["gradp"] > 5.0) & (o["divv"] >= 0.0)
            print(name, "stage", i, k, "flagged %d, steep but not flagged %d" % ((want[where] != 0).sum(), steep_not[where].sum()))
            assert (want[where] != 0).any() and steep_not[where].any()
            _assert_switch(name + " " + k, i, got, want, where)
            # after the interior part alone: its planes are done, the strips' are untouched
            _assert_switch(name + " " + k + " (between the parts)", i, between[i], want if k == "interior" else before, where)
        assert (before != want)[(ix >= nb - 1) & (ix < nb + nb - 1)].any()   # (untouched and done differ: the check sees a split)
        before = got
