"""The rules of the boundary update (pion_amd/csrc/dev_bc.h: ghost-slab enumeration, face lists, source-cell chains,
face operations, DMR states, capture cells), run on the host by tests/native/libbc_probe.so in the modes
pion_gpu_update_bcs has, against the CPU oracle's restatement of the reference's boundary updaters (orc_update_bcs).
Random states everywhere, ghosts included; every mode the configuration admits must give the oracle's whole array,
ghosts included, bit for bit.

The oracle's assigning update captures ALL inflow / fixed states before it fills any face; the product captures face
by face, after the lower faces were filled.  On random ghosts the two agree once the oracle's assigning update has run
ndim times (each pass settles the captures of one more axis), so the oracle is driven ndim times and the probe once."""
import math

import numpy as np
import pytest

import bc_probe as bp
from cpu_backends import CpuSim
from pion_amd import abi

TYPES = ["periodic", "outflow", "one-way-outflow", "reflecting", "inflow", "fixed", "jetreflect"]


def _state(cfg, rng):
    nga = abi.ng_all(cfg)
    P = rng.normal(0.0, 1.0, (cfg.nvar, nga[2], nga[1], nga[0]))
    P[0] = np.abs(P[0]) + 0.1
    P[1] = np.abs(P[1]) + 0.1
    return P


def _ongrid(cfg):
    nb = cfg.nbc
    return tuple([slice(None)] + [slice(nb, -nb) if a < cfg.ndim else slice(None) for a in (2, 1, 0)])


def _check(cfg, seed, simtime=0.0):
    """assignment, then an update without assignment on freshly scrambled ghosts: probe == oracle in every mode"""
    rng = np.random.default_rng(seed)
    P, Q = _state(cfg, rng), _state(cfg, rng)
    Q[_ongrid(cfg)] = P[_ongrid(cfg)]
    with CpuSim(cfg, "orc") as o:
        o.upload(P)
        for _ in range(cfg.ndim):
            o.update_bcs(simtime, 2, 2, assign=1)
        A_orc = o.download(0)
        o.upload(Q)
        o.update_bcs(simtime, 2, 2, assign=0)
        B_orc = o.download(0)
    assert np.array_equal(A_orc[_ongrid(cfg)], P[_ongrid(cfg)])
    # the assignment: the mode the product takes, and the face sequence (PION_FUSE_BC=0)
    refval = None
    for m in sorted({bp.mode(cfg, assign=True), bp.FACE_SEQUENCE}):
        rv = bp.new_refval()
        A = bp.update(cfg, m, P, rv, simtime, assign=True)
        assert np.array_equal(A, A_orc), ("assign", m, int((A != A_orc).sum()))
        refval = rv if m == bp.FACE_SEQUENCE else refval
    # the update proper
    modes = sorted({bp.mode(cfg, assign=False), bp.FACE_SEQUENCE})
    for m in modes:
        B = bp.update(cfg, m, Q, refval.copy(), simtime, assign=False)
        assert np.array_equal(B, B_orc), ("update", m, int((B != B_orc).sum()))
    return modes, Q, B_orc


@pytest.mark.parametrize("seed", range(12))
@pytest.mark.parametrize("eq", [abi.EQEUL, abi.EQMHD, abi.EQGLM])
def test_random_mixes(eq, seed):
    """the mixes of tests/test_gpu_bc_all.py: chains of two and three faces through corners, the psi mirror rule, the
    one-way clamp behind a flip, constants under other faces' operations"""
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
        bcs[0] = bcs[1] = "outflow"
    solver = abi.FLUX_RSroe if eq == abi.EQEUL else abi.FLUX_RS_HLLD
    cfg = abi.make_config(ndim, ng, eq, solver, ntracer=int(rng.integers(0, 2)), xmax=(1.0, 1.0, 1.0), bcs=bcs)
    modes, _, _ = _check(cfg, seed)
    assert modes == [bp.ONE_LAUNCH, bp.FACE_SEQUENCE], bcs


@pytest.mark.parametrize("ng", [[7], [6, 5], [5, 6, 7]])
def test_all_periodic(ng):
    cfg = abi.make_config(len(ng), ng, abi.EQGLM, abi.FLUX_RS_HLLD, xmax=(1.0, 1.0, 1.0))
    modes, _, _ = _check(cfg, 7)
    assert modes == [bp.PERIODIC_ALL, bp.FACE_SEQUENCE]


@pytest.mark.parametrize("ng, mode", [([5, 6, 7], bp.PERIODIC_ALL), ([6, 5], bp.ONE_LAUNCH)])
def test_slab_axis_left_alone(ng, mode):
    """periodic but for the slab axis (the neighbour ranks' faces): its ghosts come back untouched"""
    ndim = len(ng)
    cfg = abi.make_config(ndim, ng, abi.EQMHD, abi.FLUX_RS_HLLD, xmax=(1.0, 1.0, 1.0),
                          bcs=["periodic"] * (2 * ndim - 2) + ["slab", "slab"])
    modes, Q, B = _check(cfg, 11)
    assert modes == [mode, bp.FACE_SEQUENCE]
    nb = cfg.nbc
    ax = 1 if ndim == 3 else 2      # array axis of the slab axis (arrays are [v][z][y][x])
    for ghosts in (slice(0, nb), slice(-nb, None)):
        sl = tuple(ghosts if a == ax else slice(None) for a in range(4))
        assert np.array_equal(B[sl], Q[sl])


def test_double_mach_reflection():
    """the DMR face with its moving shock line and the internal DMR2 boundary"""
    simtime = 0.013
    cfg = abi.make_config(2, [12, 5], abi.EQEUL, abi.FLUX_RSroe, ntracer=1, xmax=(1.0, 1.0),
                          bcs=["inflow", "outflow", "reflecting", "DMR"], bc_dmach2=1)
    assert bp.dmr2_cols(cfg) == 2
    # no ghost cell centre of the YP list on the shock line: a build that contracts the position into an FMA and one
    # that does not then agree on which side every cell lies
    nga = abi.ng_all(cfg)
    sides = set()
    for iy in range(cfg.nbc + cfg.ng[1], nga[1]):
        y = bp.cell_centre(cfg, 1, iy)
        bpos = 10.0 * simtime / math.sin(math.pi / 3.0) + 1.0 / 6.0 + y / math.tan(math.pi / 3.0)
        for ix in range(nga[0]):
            assert abs(bp.cell_centre(cfg, 0, ix) - bpos) > 1e-9
            sides.add(bp.cell_centre(cfg, 0, ix) <= bpos)
    assert sides == {True, False}
    modes, _, _ = _check(cfg, 3, simtime)
    assert modes == [bp.ONE_LAUNCH, bp.FACE_SEQUENCE]


def test_cylindrical_glm():
    cfg = abi.make_config(2, [6, 5], abi.EQGLM, abi.FLUX_RS_HLLD, xmax=(1.0, 1.0), coord_sys=2,
                          bcs=["jetreflect", "outflow", "axisymmetric", "fixed"])
    _check(cfg, 5)


def test_1d_mhd_fixed_inflow():
    cfg = abi.make_config(1, [7], abi.EQMHD, abi.FLUX_RS_HLLD, xmax=(1.0,), bcs=["fixed", "inflow"])
    _check(cfg, 9)


# all-cell coordinates (x, y, z) with nbc = 2: along the face's axis the first on-grid cell; fixed: first cell of the
# list (lower axes at their first ghost, higher axes at their first on-grid cell), inflow: last cell of the list
CAPTURE = {
    (7,): {0: ((2, 0, 0), (2, 0, 0)), 1: ((8, 0, 0), (8, 0, 0))},
    (6, 5): {0: ((2, 2, 0), (2, 6, 0)), 1: ((7, 2, 0), (7, 6, 0)),
             2: ((0, 2, 0), (9, 2, 0)), 3: ((0, 6, 0), (9, 6, 0))},
    (5, 6, 7): {0: ((2, 2, 2), (2, 7, 8)), 1: ((6, 2, 2), (6, 7, 8)), 2: ((0, 2, 2), (8, 2, 8)),
                3: ((0, 7, 2), (8, 7, 8)), 4: ((0, 0, 2), (8, 9, 2)), 5: ((0, 0, 8), (8, 9, 8))},
}


@pytest.mark.parametrize("ng", sorted(CAPTURE))
def test_capture_cell(ng):
    cfg = abi.make_config(len(ng), list(ng), abi.EQEUL, abi.FLUX_RSroe, xmax=(1.0, 1.0, 1.0))
    assert cfg.nbc == 2
    for d, (fixed, inflow) in CAPTURE[ng].items():
        assert bp.capture_cell(cfg, d, inflow=False) == fixed, d
        assert bp.capture_cell(cfg, d, inflow=True) == inflow, d
