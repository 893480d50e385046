"""The rough fields of prepass_cases.py, on the oracle alone (no GPU): what test_gpu_prepass.py compares the device with.

For every case the oracle runs the OA1 half stage, the boundary update and the OA2 full stage.  Then
  * its state is finite with rho, p > 0 after each stage (dt = f * calculate_timestep(), f from the case table);
  * no cell is near a threshold of the switch: |gradp - 5| <= 5e-12, or 0 < |div v| <= 1e-12 sum(|v+| + |v-|) / dx -- the
    fast build's reciprocal division and contraction move these sums by a few ulp, far below that margin, which in turn
    is far below the spacing of random data; a seed that produces such a cell is changed, no cell is excluded;
  * every class of cells in which the kernels change their code shape holds both a flagged cell and a steep cell that is
    NOT flagged (gradp > 5, div v >= 0), counted from the oracle's arrays, in both stages."""
import numpy as np
import pytest

import prepass_cases as pc
from cpu_backends import have_oracle
from pion_amd import abi

pytestmark = pytest.mark.skipif(not have_oracle(), reason="oracle/liboracle.so not built (run __graft_entry__.build())")


@pytest.mark.parametrize("name", list(pc.CASES))
def test_oracle_state_stays_finite_and_positive(name):
    run = pc.oracle_run(name)
    assert run["info"]["f"] <= 0.1
    for i, st in enumerate(run["stages"]):
        A = st["state"]
        assert np.isfinite(A).all(), (name, i)
        assert (A[abi.RO] > 0).all() and (A[abi.PG] > 0).all(), (name, i, A[abi.RO].min(), A[abi.PG].min())


@pytest.mark.parametrize("name", pc.SWITCH_CASES)
def test_no_cell_near_a_threshold(name):
    run = pc.oracle_run(name)
    for i, st in enumerate(run["stages"]):
        near = pc.near_threshold(run["cfg"], st)
        assert not near.any(), (name, i, np.argwhere(near)[:5].tolist())


@pytest.mark.parametrize("name", pc.SWITCH_CASES)
def test_every_class_has_flagged_and_steep_unflagged_cells(name):
    run = pc.oracle_run(name)
    cfg = run["cfg"]
    masks = pc.class_masks(cfg)
    for i, st in enumerate(run["stages"]):
        flagged = pc.expected_switch(st) != 0
        steep_not = (st["gradp"] > 5.0) & (st["divv"] >= 0.0)
        counts = {k: (int((flagged & m).sum()), int((steep_not & m).sum())) for k, m in masks.items()}
        print(name, "stage", i, "(flagged, steep but not flagged):", counts)
        for k, (nf, ns) in counts.items():
            assert nf > 0 and ns > 0, (name, i, k, nf, ns)
        if i == 0:
            # the region at rest: div v == 0 exactly, steep cells, none flagged
            rest = run["info"]["region"] == pc.REST
            inner = rest & (st["divv"] == 0.0)
            assert (st["gradp"][inner] > 5.0).any() and not flagged[inner].any(), name


@pytest.mark.parametrize("name", pc.SWITCH_CASES)
def test_spikes_are_planted_where_the_kernels_change_shape(name):
    run = pc.oracle_run(name)
    cfg, spikes = run["cfg"], run["info"]["spikes"]
    nb = cfg.nbc
    print(name, "%d spikes at all-cell (x, y, z):" % len(spikes), spikes)
    for a in range(cfg.ndim):
        assert any(c[a] == nb for c in spikes) and any(c[a] == nb + cfg.ng[a] - 1 for c in spikes), (name, a)
    for x in (61, 62, 123, 124):
        if nb <= x < nb + cfg.ng[0]:
            # (1-D: spikes keep two cells between them, one of a seam's two columns has it and makes the other steep)
            assert any(c[0] == x or (cfg.ndim == 1 and abs(c[0] - x) == 1) for c in spikes), (name, x)
    if cfg.ndim == 3:
        for z in (15, 16):
            if z < nb + cfg.ng[2]:
                assert any(c[2] == z for c in spikes), (name, z)
    if name == "march_3d":
        # a corner of the screen's blocks: on-grid x 61 | 62, y 3 | 4, z 7 | 8.  (screen_join: its calm region begins at
        # that corner, and a spike's velocity patch stays inside the rough region)
        assert any(c[0] - nb in (61, 62) and c[1] - nb in (3, 4) and c[2] - nb in (7, 8) for c in spikes), name
    # every spike is a x 50 jump against each of its on-grid neighbours' scale
    p = run["P"][abi.PG]
    for x, y, z in spikes:
        assert p[z, y, x] > 50.0 * np.exp(-pc.A_ROUGH) * 0.999


def _one_ulp(P, seed=1):
    rng = np.random.default_rng(seed)
    up = rng.integers(0, 2, P.shape) > 0
    # (exact zeros stay: v = 0 in the region at rest is what keeps div v == 0 there, away from the switch's threshold)
    return np.where(P == 0.0, P, np.where(up, np.nextafter(P, np.inf), np.nextafter(P, -np.inf)))


@pytest.mark.parametrize("name", sorted(set(pc.FAST_STATE_CASES + pc.ETA_CASES)))
def test_oracle_is_well_conditioned_where_the_fast_build_is_held_to_it(name):
    """1 ulp on every non-zero input value moves the oracle's states after both stages by rounding only: the cases on which
    test_gpu_prepass.py compares fast-build states (and the second stage's eta, which is computed from one) have a
    build-independent answer.  (Ideal-MHD HLLD next to a reflecting wall has none: tests/test_reference_conditioning.py.)"""
    from cpu_backends import CpuSim
    run = pc.oracle_run(name)
    cfg = run["cfg"]
    got = []
    with CpuSim(cfg, "orc") as o:
        pc.two_stages(o, cfg, _one_ulp(run["P"]), run["info"]["f"], t_dyn=run["t_dyn"],
                      record=lambda s, i, S: got.append(s.download(1 - i).copy()) if i < 2 else None)
    for i in range(2):
        a, b = got[i], run["stages"][i]["state"]
        scale = np.abs(b).reshape(cfg.nvar, -1).max(axis=1).reshape(-1, 1, 1, 1) + 1e-300
        s = float((np.abs(a - b) / scale).max())
        print(name, "stage", i, "1 ulp in -> %.2e out" % s)
        assert s < 1e-13, (name, i, s)


@pytest.mark.parametrize("name", pc.SCREENED_CASES)
def test_screen_blocks_of_the_second_stage(name):
    """the blocks the screened prepass of the second stage evaluates (hll_screen.h, restated in prepass_cases.py): flagged
    and steep-unflagged cells in active blocks, none flagged in a quiet one; screen_join must keep a quiet block"""
    run = pc.oracle_run(name)
    cfg = run["cfg"]
    st = run["stages"][1]
    active, (ez, ey, ex) = pc.screen_blocks(cfg, run["stages"][0]["state"])
    cell_active = active[ez, ey, ex]
    flagged = pc.expected_switch(st) != 0
    steep_not = (st["gradp"] > 5.0) & (st["divv"] >= 0.0)
    print(name, "active blocks %d of %d" % (active.sum(), active.size), "flagged / steep-unflagged in active blocks:",
          int((flagged & cell_active).sum()), int((steep_not & cell_active).sum()))
    assert (flagged & cell_active).any() and (steep_not & cell_active).any()
    assert not (flagged & ~cell_active).any()
    if name == "screen_join":
        assert 0 < active.sum() < active.size
        # the remainder of 1 < nbc rows joined the last y block: 2 blocks along y, not 3
        assert active.shape == (3, 2, 3)
