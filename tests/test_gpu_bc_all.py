"""k_bc_all -- every external face of any mix of boundary types in one launch, each ghost cell resolving its chain of
source cells down the axes -- against the per-face launch sequence X -> Y -> Z (k_bc_face, PION_FUSE_BC=0), which is
the reference's order (assign_update_bcs.cpp:185-252) and is itself pinned to the reference's boundary updaters by the
whole-step fixtures (tests/test_gpu_golden.py).  Random states everywhere (ghosts included), random mixes of face
types in 1-D, 2-D and 3-D for all three equation sets: the ghost cells must come out bit for bit the same -- corner
and edge ghosts (chains of two and three faces), the psi mirror rule of outflow / one-way faces through corners, the
one-way clamp behind a reflecting flip, inflow / fixed constants under other faces' operations, slab faces left alone.
Fixed cases add the faces the mixes never draw (DMR with DMR2, axisymmetric), and all-periodic grids take
k_bc_periodic_all against the same face sequence.  (The face sequence's rules against the CPU oracle, without a GPU:
tests/test_bc_rule.py.)"""
import numpy as np
import pytest

from pion_amd import abi

pytestmark = pytest.mark.gpu

TYPES = ["periodic", "outflow", "one-way-outflow", "reflecting", "inflow", "fixed", "jetreflect"]


def _run(cfg, P, fuse, monkeypatch, simtime=0.0):
    from pion_amd import lib
    if fuse:
        monkeypatch.delenv("PION_FUSE_BC", raising=False)
    else:
        monkeypatch.setenv("PION_FUSE_BC", "0")
    with lib.GpuSim(cfg, 0) as g:
        g.upload(P)
        g.update_bcs(simtime, 2, 2, assign=1)      # assignment: per-face sequence in both modes (captures inflow / fixed states)
        A0 = g.download(0)
        # scramble the ghosts again (keep the on-grid cells), then update WITHOUT assignment: this is the launch under test
        Q = P.copy()
        nb = cfg.nbc
        sl = tuple([slice(None)] + [slice(nb, -nb) if a < cfg.ndim else slice(None) for a in (2, 1, 0)])
        Q[sl] = A0[sl]
        g.upload(Q)
        g.update_bcs(simtime, 2, 2, assign=0)
        return g.download(0)


def _state(cfg, rng):
    nga = abi.ng_all(cfg)
    P = rng.normal(0.0, 1.0, (cfg.nvar, nga[2], nga[1], nga[0]))
    P[0] = np.abs(P[0]) + 0.1
    P[1] = np.abs(P[1]) + 0.1
    return P


def _both_equal(cfg, seed, monkeypatch, simtime=0.0):
    P = _state(cfg, np.random.default_rng(seed))
    a = _run(cfg, P, True, monkeypatch, simtime)
    b = _run(cfg, P, False, monkeypatch, simtime)
    assert np.array_equal(a, b), int((a != b).sum())
    return P, a


def test_double_mach_reflection(monkeypatch):
    """the DMR face with its shock line and the internal DMR2 boundary inside the one launch"""
    cfg = abi.make_config(2, [12, 5], abi.EQEUL, abi.FLUX_RSroe, ntracer=1, xmax=(1.0, 1.0),
                          bcs=["inflow", "outflow", "reflecting", "DMR"], bc_dmach2=1)
    _both_equal(cfg, 3, monkeypatch, simtime=0.013)


def test_cylindrical_glm(monkeypatch):
    cfg = abi.make_config(2, [6, 5], abi.EQGLM, abi.FLUX_RS_HLLD, xmax=(1.0, 1.0), coord_sys=2,
                          bcs=["jetreflect", "outflow", "axisymmetric", "fixed"])
    _both_equal(cfg, 5, monkeypatch)


@pytest.mark.parametrize("ng, slab", [([9, 7], False), ([5, 11, 7], False), ([7, 5, 6], True)])
def test_periodic_all_equals_face_sequence(ng, slab, monkeypatch):
    """k_bc_periodic_all on random ghosts; slab: the z faces are the neighbour ranks', their ghosts stay as uploaded"""
    ndim = len(ng)
    bcs = ["periodic"] * (2 * ndim - 2) + (["slab", "slab"] if slab else ["periodic", "periodic"])
    cfg = abi.make_config(ndim, ng, abi.EQGLM, abi.FLUX_RS_HLLD, xmax=(1.0, 1.0, 1.0), bcs=bcs)
    P, a = _both_equal(cfg, 7, monkeypatch)
    if slab:
        nb = cfg.nbc
        assert np.array_equal(a[:, :nb], P[:, :nb]) and np.array_equal(a[:, -nb:], P[:, -nb:])


@pytest.mark.parametrize("seed", range(12))
@pytest.mark.parametrize("eq", [abi.EQEUL, abi.EQMHD, abi.EQGLM])
def test_one_launch_equals_face_sequence(eq, seed, monkeypatch):
    rng = np.random.default_rng(1000 * eq + seed)
    ndim = [3, 3, 2, 3, 2, 1][seed % 6]
    ng = [int(rng.integers(5, 12)) for _ in range(ndim)]
    bcs = []
    for a in range(ndim):
        if rng.uniform() < 0.25:
            bcs += ["periodic", "periodic"]     # (periodic faces come in pairs)
        else:
            bcs += [TYPES[int(rng.integers(1, len(TYPES)))], TYPES[int(rng.integers(1, len(TYPES)))]]
    if all(b == "periodic" for b in bcs):
        bcs[0] = bcs[1] = "outflow"             # (all-periodic grids take k_bc_periodic_all)
    solver = abi.FLUX_RSroe if eq == abi.EQEUL else abi.FLUX_RS_HLLD
    ntr = int(rng.integers(0, 2))
    cfg = abi.make_config(ndim, ng, eq, solver, ntracer=ntr, xmax=(1.0, 1.0, 1.0), bcs=bcs, strict_fp=1)
    shape = (cfg.nvar,) + tuple((ng[a] + 2 * cfg.nbc) if a < ndim else 1 for a in (2, 1, 0))
    P = rng.normal(0.0, 1.0, shape)
    P[0] = np.abs(P[0]) + 0.1
    P[1] = np.abs(P[1]) + 0.1
    a = _run(cfg, P, True, monkeypatch)
    b = _run(cfg, P, False, monkeypatch)
    assert np.array_equal(a, b), (bcs, ng, int((a != b).sum()))
