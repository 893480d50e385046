"""The cell update's data-dependent repairs on the device, against the CPU oracle.

CellAdvanceTime repairs a cell in four ways -- p <= 0 becomes 0.01 rho (no microphysics) or the MinTemperature floor
(microphysics), T < MinTemperature is floored, T > MaxTemperature is capped, tracers above 1 are renormalised (sCMA,
before and after the update) -- and a density <= 0 is fatal: the device raises ERR_NEG_DENSITY in its error word,
which the next read-back turns into PION_GPU_EPHYSICS.  The blasts of the other GPU tests never reach any of these.

Section 1 drives the device functions cell by cell through pion_gpu_cell_advance; section 2 runs the production
kernels on grids whose velocity field is hypersonic, so that hundreds of cells are repaired per step.  Every test
first asserts, from the oracle's result alone, that its input does reach the repairs it is about.

strict_fp = 1 is compared bit for bit.  strict_fp = 0 (FMA contraction, seeded reciprocals, regrouped sums) must give
every cell the same repair status and every variable within 1e-10 of the variable's largest magnitude.
"""
import math

import numpy as np
import pytest

import golden_cases as gc
from cpu_backends import CpuSim
from pion_amd import abi, cooling, driver, problems

pytestmark = pytest.mark.gpu

MU_KB = gc.ODE_MU_TOT_OVER_KB   # Mu_tot / k_B of mp_only_cooling: T = p Mu_tot / (k_B rho)
FAST_TOL = 1e-10                # of each variable's largest magnitude: the bound the fast build is held to
STATUS_RTOL = 1e-13             # fast build: a pressure this close to a repair value is a repaired one
P_REPAIRED, T_FLOOR, T_CEILING = 1, 2, 4
EQS = [abi.EQEUL, abi.EQMHD, abi.EQGLM]
EQNAME = {abi.EQEUL: "euler", abi.EQMHD: "mhd", abi.EQGLM: "glm"}
SVNAME = {abi.FLUX_RSroe: "roe", abi.FLUX_RS_HLL: "hll", abi.FLUX_RS_HLLD: "hlld"}


def _gpu(cfg):
    from pion_amd import lib
    return lib.GpuSim(cfg, 0)


def _base(cfg):
    return cfg.nvar - cfg.ntracer


def repair_status(cfg, ro, pg, rtol=0.0):
    """Per cell: P_REPAIRED where p == 0.01 rho (handles without microphysics), T_FLOOR / T_CEILING where p is the
    pressure of MinTemperature / MaxTemperature (handles with).  rtol = 0: exactly the value check_pressure and the
    ceiling assign."""
    def at(x):
        return np.abs(pg - x) <= rtol * np.abs(x)
    if cfg.cooling == 0:
        return np.where(at(0.01 * ro), P_REPAIRED, 0)
    return np.where(at(ro * cfg.min_temp / MU_KB), T_FLOOR, 0) | np.where(at(ro * cfg.max_temp / MU_KB), T_CEILING, 0)


def count(status, bit):
    return int(((status & bit) != 0).sum())


def assert_fast_close(cfg, got, want, what, max_left_out):
    """got, want: [nvar, ncells].  The repair status of every cell must agree -- but for max_left_out cells, which
    are then left out of the value comparison --, every other value within FAST_TOL of its variable's scale.
    Returns (largest error / scale, cells left out)."""
    assert np.isfinite(want).all() and np.isfinite(got).all(), what
    sw = repair_status(cfg, want[abi.RO], want[abi.PG])
    sg = repair_status(cfg, got[abi.RO], got[abi.PG], STATUS_RTOL)
    out = sw != sg
    assert out.sum() <= max_left_out, "%s: repair status differs in %d cells (%d allowed)" % (what, out.sum(), max_left_out)
    scale = np.abs(want).max(axis=1).reshape(-1, 1) + 1e-300
    err = (np.abs(got - want) / scale)[:, ~out]
    print("%s: max err/scale %.3e (variable %d), %d cells left out" % (what, err.max(), err.max(axis=1).argmax(),
                                                                      out.sum()))
    assert err.max() <= FAST_TOL, (what, err.max(axis=1))
    return err.max(), int(out.sum())


# ---------------------------------------------------------------------------------------------------------------------
# 1. the cell-level seam
# ---------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def cell_kat():
    import os
    return np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "cell_kat.npz"))


@pytest.mark.parametrize("case", gc.cell_cases(), ids=lambda c: gc.cell_key(*c))
def test_seam_reference_vectors_strict(cell_kat, case):
    """the reference's own CellAdvanceTime / CellTimeStep outputs (a third of the cells with p <= 0), set up as
    test_oracle_golden.py::test_cell_kat; MaxTemperature 1e9 there is out of every cell's reach"""
    key = gc.cell_key(*case)
    cfg = gc.cell_cfg(*case)
    P, dU = cell_kat[key + "_P"], cell_kat[key + "_dU"]
    with _gpu(cfg) as g:
        g.set_glm_speeds(gc.GLM_DT, cfg.dx, 0.25 / cfg.dx)
        assert np.array_equal(g.cell_advance(P, dU, fv_dt=gc.GLM_DT), cell_kat[key + "_Pf"], equal_nan=True)
        assert np.array_equal(g.cell_timestep(P), cell_kat[key + "_dt"], equal_nan=True)


SEAM_N = 2000
SEAM_MIN_TEMP, SEAM_MAX_TEMP = 2.0e3, 5.0e4   # inside the 50 K ... 1e6 K that cell_inputs' states span
SEAM_CASES = [(eq, ntr, cool) for eq in EQS for ntr in (0, 1, 2) for cool in (0, abi.COOL_WSS09_CIE_LINE_HEAT_COOL)]
_seam_refs = {}


def seam_cfg(eq, ntr, cool, strict_fp):
    solver = abi.FLUX_RSroe if eq == abi.EQEUL else abi.FLUX_RS_HLLD
    return abi.make_config(3, [4, 4, 4], eq, solver, ntracer=ntr, xmax=(1, 1, 1), cooling=cool,
                           min_temp=SEAM_MIN_TEMP, max_temp=SEAM_MAX_TEMP, strict_fp=strict_fp)


def oracle_cells(cfg, P, dU):
    """What the stage kernels' cell_update and cell_dt compute, from the oracle: its CellAdvanceTime seam, then
    the two lines of grid_update_state_vector's ceiling (Oracle::grid_update_state_vector, Temperature / Set_Temp of
    orc_eqns.h: the same operations in the same order, so bit for bit), and its CellTimeStep seam."""
    with CpuSim(cfg, "orc") as o:
        o.set_glm_speeds(gc.GLM_DT, cfg.dx, 0.25 / cfg.dx)
        Pf = o.cell_advance(P, dU, fv_dt=gc.GLM_DT)
        dt = o.cell_timestep(P)
    if cfg.cooling:
        hot = Pf[:, abi.PG] * MU_KB / Pf[:, abi.RO] > cfg.max_temp
        Pf[hot, abi.PG] = Pf[hot, abi.RO] * cfg.max_temp / MU_KB
    return Pf, dt


def seam_reference(case):
    """inputs and oracle outputs of one case, computed once; asserts that the inputs reach every repair"""
    if case not in _seam_refs:
        eq, ntr, cool = case
        cfg = seam_cfg(eq, ntr, cool, 1)
        rng = np.random.default_rng(20261 + SEAM_CASES.index(case))
        P, dU = gc.cell_inputs(rng, cfg, n=SEAM_N)
        if cool:
            # cell_inputs gives rho ~ 1e-24 and p ~ 1e-12 but leaves v, B and their dU of order one: every cell then
            # ends at the floor.  The remaining variables in the same units (cm/s, Gauss / sqrt(4 pi)): kinetic and
            # magnetic energy comparable with the thermal one, T before repairs between 1e2 K and 1e6 K
            P[:, abi.VX:abi.VZ + 1] *= 1.0e6
            dU[:, abi.MMX:abi.MMZ + 1] *= 1.0e-18
            if eq != abi.EQEUL:
                P[:, abi.BX:_base(cfg)] *= 1.0e-6
                dU[:, abi.BBX:_base(cfg)] *= 1.0e-6
        Pf, dt = oracle_cells(cfg, P, dU)
        assert np.isfinite(Pf).all() and np.isfinite(dt).all() and (Pf[:, abi.RO] > 0).all()
        st = repair_status(cfg, Pf[:, abi.RO], Pf[:, abi.PG])
        if cool == 0:
            assert count(st, P_REPAIRED) >= 100, count(st, P_REPAIRED)
        else:
            assert count(st, T_FLOOR) >= 100 and count(st, T_CEILING) >= 100, (count(st, T_FLOOR), count(st, T_CEILING))
        if ntr:
            assert (P[:, _base(cfg):] > 1.0).any(axis=1).sum() >= 100
            if cool:   # sCMA after the update too: x * (1 / x)
                assert 1.0 - 1e-15 < Pf[:, _base(cfg):].max() <= 1.0
        for a in (P, dU, Pf, dt):
            a.setflags(write=False)
        _seam_refs[case] = (P, dU, Pf, dt)
    return _seam_refs[case]


def _seam_id(c):
    return "%s_t%d_c%d" % (EQNAME[c[0]], c[1], c[2])


@pytest.mark.parametrize("case", SEAM_CASES, ids=_seam_id)
def test_seam_repairs_strict(case):
    P, dU, Pf, dt = seam_reference(case)
    cfg = seam_cfg(*case, 1)
    with _gpu(cfg) as g:
        g.set_glm_speeds(gc.GLM_DT, cfg.dx, 0.25 / cfg.dx)
        got = g.cell_advance(P, dU, fv_dt=gc.GLM_DT)
        assert np.array_equal(got, Pf), ((got != Pf).sum(), np.abs(got - Pf).max())
        assert np.array_equal(g.cell_timestep(P), dt)


@pytest.mark.parametrize("case", SEAM_CASES, ids=_seam_id)
def test_seam_repairs_fast(case):
    """Fast build: the same repair status in every cell, every variable (and the time step) within 1e-10 of its scale.
    Measured on an MI355X: at most 3.6e-15 over the 18 cases (always the pressure), no cell of another status."""
    P, dU, Pf, dt = seam_reference(case)
    cfg = seam_cfg(*case, 0)
    with _gpu(cfg) as g:
        g.set_glm_speeds(gc.GLM_DT, cfg.dx, 0.25 / cfg.dx)
        got = g.cell_advance(P, dU, fv_dt=gc.GLM_DT)
        gdt = g.cell_timestep(P)
    assert_fast_close(cfg, got.T, Pf.T, "seam " + _seam_id(case), 0)
    assert np.abs(gdt - dt).max() <= FAST_TOL * dt.max()


def _error_of(exc):
    from pion_amd import lib
    assert isinstance(exc.value, lib.PionGpuError)
    return exc.value.rc, str(exc.value)


@pytest.mark.parametrize("eq", [abi.EQEUL, abi.EQGLM], ids=lambda e: EQNAME[e])
def test_seam_negative_density_raises_and_clears(eq):
    """a density <= 0 after the update: EPHYSICS naming it (the oracle raises too); the word is cleared by the report"""
    from pion_amd import lib
    cfg = seam_cfg(eq, 1, 0, 1)
    rng = np.random.default_rng(99)
    P, dU = gc.cell_inputs(rng, cfg, n=500)
    bad = dU.copy()
    for i in (7, 250, 499):
        bad[i, abi.RHO] = -2.0 * P[i, abi.RO]
    want, _ = oracle_cells(cfg, P, dU)
    with CpuSim(cfg, "orc") as o, pytest.raises(RuntimeError, match="(?i)negative density"):
        o.cell_advance(P, bad, fv_dt=gc.GLM_DT)
    with _gpu(cfg) as g:
        g.set_glm_speeds(gc.GLM_DT, cfg.dx, 0.25 / cfg.dx)
        with pytest.raises(lib.PionGpuError) as exc:
            g.cell_advance(P, bad, fv_dt=gc.GLM_DT)
        rc, msg = _error_of(exc)
        assert rc == abi.E_PHYSICS and "negative density" in msg, (rc, msg)
        assert np.array_equal(g.cell_advance(P, dU, fv_dt=gc.GLM_DT), want)


def test_cooling_update_non_finite_raises():
    """mp_only_cooling::TimeUpdateMP on a state with a NaN pressure: EPHYSICS naming the cooling integration (every
    loop of the integrator is bounded: at most 25 steps of at most 50 halvings)"""
    from pion_amd import lib
    cfg = gc.cool_cfg(0)
    P, _ = gc.cool_states(np.random.default_rng(5), cfg.min_temp, cfg.max_temp, n=64)
    tables = cooling.build_tables(cfg.min_temp, cfg.max_temp)
    bad = P.copy()
    bad[17, abi.PG] = np.nan
    with _gpu(cfg) as g, CpuSim(cfg, "orc") as o:
        g.set_cooling_tables(*tables)
        o.set_cooling_tables(*tables)
        with pytest.raises(lib.PionGpuError) as exc:
            g.cooling_update(bad, 1.0e9)
        rc, msg = _error_of(exc)
        assert rc == abi.E_PHYSICS and "cooling" in msg, (rc, msg)
        assert np.array_equal(g.cooling_update(P, 1.0e9), o.cooling_update(P, 1.0e9))


# ---------------------------------------------------------------------------------------------------------------------
# 2. the production kernels on grids where cells need repairs
# ---------------------------------------------------------------------------------------------------------------------

def hypersonic(label, eq, solver, ntracer=0, artvisc=abi.AV_FKJ98_1D, strict_fp=1):
    """An existing problem with a hypersonic velocity field added: (cfg, P, setup).  Labels:
    A  the generic MHD blast on 14^3, velocities x 20/0.3 (Mach ~ 50 in the ambient gas)
    B  the Euler blast box on 14^3, velocities x 600
    C  the same two on 40 x 24
    D  the axisymmetric (z,R) blast on 32 x 16 with VX = 20 sin(2 pi X), VY = 15 sin(2 pi Y), VZ = 10 Y
    E  the cooling blast's configuration on 14^3: a 6e7 K bubble, |v| up to 3e8 cm/s, tracers up to 1.4"""
    tables = None

    def setup(sim):
        if tables:
            sim.set_cooling_tables(*tables)
    if label in "ABC":
        ng = [14, 14, 14] if label != "C" else [40, 24]
        if eq == abi.EQEUL:
            cfg, P = problems.hd_blast_box(ng, solver, ntracer=ntracer, artvisc=artvisc, strict_fp=strict_fp)
            # (with the H-correction x 600 repairs 91 cells in step 1, short of half of Roe's 248: x 900 repairs 173
            # and 188)
            P[abi.VX:abi.VZ + 1] *= 900.0 if artvisc == abi.AV_HCORR_FKJ98 else 600.0
        else:
            cfg, P = problems.mhd_blast_generic(ng, eq, solver, strict_fp=strict_fp, ntracer=ntracer)
            cfg.artvisc = artvisc
            P[abi.VX:abi.VZ + 1] *= 20.0 / 0.3
    elif label == "D":
        cfg, P = problems.blast_axi2d(32, eq, solver, ntracer=ntracer, artvisc=artvisc, strict_fp=strict_fp)
        X, Y, _ = problems.mesh(cfg)
        P[abi.VX] = 20.0 * np.sin(2 * np.pi * X)
        P[abi.VY] = 15.0 * np.sin(2 * np.pi * Y)
        P[abi.VZ] = 10.0 * Y
    else:
        c0, _ = problems.cooling_blast3d(14, strict_fp=strict_fp, solver=solver)
        L = c0.dx * 14
        nvb = {abi.EQEUL: 5, abi.EQMHD: 8, abi.EQGLM: 9}[eq]
        cfg = abi.make_config(3, [14, 14, 14], eq, solver, ntracer=1, artvisc=artvisc, etav=c0.etav, gamma=c0.gamma,
                              cfl=c0.cfl, xmin=(0.0, 0.0, 0.0), xmax=(L, L, L),
                              bcs=["reflecting", "one-way-outflow"] * 3,
                              refvec=[1.0e-24, 1.0e-13, 1.0e6, 1.0e6, 1.0e6] + [1.0e-6] * (nvb - 5) + [1.0],
                              min_temp=c0.min_temp, max_temp=c0.max_temp, cooling=c0.cooling,
                              mp_timestep_limit=c0.mp_timestep_limit, strict_fp=strict_fp)
        P = problems.alloc(cfg)
        X, Y, Z = problems.mesh(cfg)
        inside = X * X + Y * Y + Z * Z < (0.3 * L) ** 2
        k, V = 2.0 * math.pi / L, 3.0e8
        P[abi.RO] = np.where(inside, 20.0, 1.0) * 2.124229813e-24
        P[abi.PG] = P[abi.RO] * np.where(inside, 6.0e7, 7.5e3) / MU_KB
        P[abi.VX] = V * np.sin(2 * k * X + 0.3)
        P[abi.VY] = 0.7 * V * np.cos(3 * k * Y)
        P[abi.VZ] = -0.5 * V * np.sin(2 * k * Z + 0.1)
        if nvb >= 8:
            P[abi.BX], P[abi.BY], P[abi.BZ] = 1.0e-6, 2.0e-6, 0.5e-6
        P[nvb] = np.where(inside, 1.0, 0.0) + 0.4 * np.sin(4 * k * X) ** 2
        tables = cooling.build_tables(cfg.min_temp, cfg.max_temp)
    return cfg, P, setup


def ongrid(cfg, A):
    """[nvar, on-grid cells] of a state array"""
    nb = cfg.nbc
    sl = tuple(slice(nb, -nb) if a < cfg.ndim else slice(None) for a in (2, 1, 0))
    return A[(slice(None),) + sl].reshape(cfg.nvar, -1)


def grid_status(cfg, A, rtol=0.0):
    a = ongrid(cfg, A)
    return repair_status(cfg, a[abi.RO], a[abi.PG], rtol)


# Repaired on-grid cells (p == 0.01 rho) of the oracle after step 1 and step 2, measured on the oracle in the strict
# configuration; the tests demand half of them.  E: (floor, ceiling) per step.
REPAIRED = {
    ("A", abi.EQGLM, abi.FLUX_RS_HLLD): (509, 552), ("A", abi.EQGLM, abi.FLUX_RS_HLL): (509, 552),
    ("A", abi.EQMHD, abi.FLUX_RS_HLLD): (509, 552), ("A", abi.EQMHD, abi.FLUX_RS_HLL): (509, 552),
    ("A", abi.EQGLM, abi.FLUX_RSroe): (495, 541),
    ("B", abi.EQEUL, abi.FLUX_RSroe): (248, 350), ("B", abi.EQEUL, abi.FLUX_RS_HLL): (75, 109),
    ("C", abi.EQGLM, abi.FLUX_RS_HLLD): (37, 106), ("C", abi.EQMHD, abi.FLUX_RS_HLL): (37, 106),
    ("C", abi.EQEUL, abi.FLUX_RSroe): (0, 33),
    ("D", abi.EQEUL, abi.FLUX_RSroe): (0, 20), ("D", abi.EQGLM, abi.FLUX_RS_HLLD): (0, 30),
    ("D", abi.EQMHD, abi.FLUX_RS_HLL): (0, 30),
}
E_FLOOR, E_CEILING, E_TRACERS = 289, (5, 19), 34

_grid_refs = {}


def grid_reference(label, eq, solver, ntracer, artvisc):
    """The oracle's two steps of one case, computed once: dict bc (state after init), P (after each step), dt.
    Asserts that the case bites: half the repaired cells listed for it (where 0 is listed for step 1, at step 2 only)."""
    key = (label, eq, solver, ntracer, artvisc)
    if key in _grid_refs:
        return _grid_refs[key]
    cfg, P, setup = hypersonic(label, eq, solver, ntracer, artvisc, 1)
    ref = {"P": [], "dt": []}
    with CpuSim(cfg, "orc") as o:
        setup(o)
        so = driver.SimControl(o, cfg)
        so.init(P)
        ref["bc"] = o.download(0)
        for it in range(2):
            ref["dt"].append(so.calculate_timestep())
            so.advance_time()
            ref["P"].append(o.download(0))
    for it in range(2):
        a = ongrid(cfg, ref["P"][it])
        assert np.isfinite(a).all() and (a[abi.RO] > 0).all()
        st = grid_status(cfg, ref["P"][it])
        if label == "E":
            assert count(st, T_FLOOR) >= (E_FLOOR + 1) // 2, (it, count(st, T_FLOOR))
            assert count(st, T_CEILING) >= (E_CEILING[it] + 1) // 2, (it, count(st, T_CEILING))
            assert a[_base(cfg)].max() == 1.0
        else:
            want = REPAIRED[(label, eq, solver)][it]
            assert count(st, P_REPAIRED) >= (want + 1) // 2, (key, it, count(st, P_REPAIRED), want)
    if label == "E":
        assert (ongrid(cfg, ref["bc"])[_base(cfg)] > 1.0).sum() >= (E_TRACERS + 1) // 2
    for a in [ref["bc"]] + ref["P"]:
        a.setflags(write=False)
    _grid_refs[key] = ref
    return ref


def _case_id(c):
    label, eq, solver = c[:3]
    s = "%s_%s_%s" % (label, EQNAME[eq], SVNAME[solver])
    if len(c) > 3:
        s += "_t%d" % c[3]
    if len(c) > 4 and c[4] == abi.AV_HCORR_FKJ98:
        s += "_hcorr"
    return s


MHD_PAIRS = [(abi.EQGLM, abi.FLUX_RS_HLLD), (abi.EQGLM, abi.FLUX_RS_HLL), (abi.EQMHD, abi.FLUX_RS_HLLD),
             (abi.EQMHD, abi.FLUX_RS_HLL), (abi.EQGLM, abi.FLUX_RSroe)]
AV1, HC = abi.AV_FKJ98_1D, abi.AV_HCORR_FKJ98
# (label, eq, solver, ntracer, artvisc)
GRID_CASES = (
    [("A", eq, sv, 1, AV1) for eq, sv in MHD_PAIRS]
    + [("B", abi.EQEUL, abi.FLUX_RSroe, 1, AV1), ("B", abi.EQEUL, abi.FLUX_RS_HLL, 1, AV1)]
    # the H-correction selects the instances of the rows kernel that are not PLAIN
    + [("A", abi.EQGLM, abi.FLUX_RS_HLLD, t, HC) for t in (0, 2)]
    + [("A", abi.EQMHD, abi.FLUX_RS_HLL, t, HC) for t in (0, 2)]
    + [("B", abi.EQEUL, abi.FLUX_RSroe, t, HC) for t in (0, 2)]
    + [("C", abi.EQGLM, abi.FLUX_RS_HLLD, 1, AV1), ("C", abi.EQMHD, abi.FLUX_RS_HLL, 1, AV1),
       ("C", abi.EQEUL, abi.FLUX_RSroe, 1, AV1)]
    + [("D", abi.EQEUL, abi.FLUX_RSroe, 1, AV1), ("D", abi.EQGLM, abi.FLUX_RS_HLLD, 1, AV1),
       ("D", abi.EQMHD, abi.FLUX_RS_HLL, 1, AV1)]
    + [("E", abi.EQEUL, abi.FLUX_RSroe, 1, AV1), ("E", abi.EQEUL, abi.FLUX_RS_HLL, 1, AV1),
       ("E", abi.EQGLM, abi.FLUX_RS_HLL, 1, AV1), ("E", abi.EQGLM, abi.FLUX_RS_HLLD, 1, AV1)]
)


def run_strict(case):
    """two steps on the device, dt and every cell (ghost cells included) bit for bit the oracle's"""
    ref = grid_reference(*case)
    cfg, P, setup = hypersonic(*case, 1)
    with _gpu(cfg) as g:
        setup(g)
        sg = driver.SimControl(g, cfg)
        sg.init(P)
        assert np.array_equal(g.download(0), ref["bc"]), "boundary assignment differs"
        for it in range(2):
            dt = sg.calculate_timestep()
            assert dt == ref["dt"][it], (it, dt, ref["dt"][it])
            sg.advance_time()
            a, b = g.download(0), ref["P"][it]
            assert np.array_equal(a, b), "step %d: %d values differ, max abs %g" % (it, (a != b).sum(),
                                                                                      np.abs(a - b).max())


@pytest.mark.parametrize("case", GRID_CASES, ids=_case_id)
def test_grid_repairs_strict(case):
    run_strict(case)


@pytest.mark.parametrize("case", [("A", abi.EQGLM, abi.FLUX_RS_HLLD, 1, AV1), ("B", abi.EQEUL, abi.FLUX_RSroe, 1, AV1)],
                         ids=_case_id)
def test_grid_repairs_strict_cell_kernel(case, monkeypatch):
    """the cell-per-thread kernel k_stage (what 1-D grids run) on the same grids"""
    monkeypatch.setenv("PION_STAGE_KERNEL", "cell")
    run_strict(case)


FAST_CASES = [c for c in GRID_CASES if c[4] == AV1] + [("A", abi.EQGLM, abi.FLUX_RS_HLLD, 2, HC),
                                                       ("B", abi.EQEUL, abi.FLUX_RSroe, 0, HC)]


@pytest.mark.parametrize("start", [0, 1], ids=["from_ic", "from_step1"])
@pytest.mark.parametrize("case", FAST_CASES, ids=_case_id)
def test_grid_repairs_fast(case, start):
    """Fast build, ONE second-order step (the only route into the rows kernel's inlined u0 tail) from the state the
    oracle itself started that step from -- the initial condition, or its own state after one step --, with the oracle's
    dt: a cell that lands on the other side of p = 0 then differs in that cell alone.  Cells whose repair status is
    not the oracle's are left out, at most 0.5 % of the on-grid cells; every other value within 1e-10 of its
    variable's scale.  (Under a random 1e-14 relative perturbation of its input the oracle itself changes no
    cell's status in any of these comparisons and moves by up to 6.8e-12 of the scale -- GLM, 2-D --, 1.4e-13 for
    Euler and ideal MHD.)
    Measured on an MI355X, largest error / scale over both starts, no cell left out in any of the 46 comparisons:
    A (3-D MHD / GLM) 9.9e-14 (GLM Roe, psi), B (3-D Euler) 1.3e-15, C (2-D) 2.2e-13 (GLM HLLD, psi), 2.8e-14 (MHD HLL),
    8.8e-16 (Euler), D (axisymmetric) 2.7e-14, E (cooling) 1.9e-15, A with the H-correction 6.6e-14, B with it 9.7e-16."""
    ref = grid_reference(*case)
    cfg, P, setup = hypersonic(*case, 0)
    with _gpu(cfg) as g:
        setup(g)
        sg = driver.SimControl(g, cfg)
        if start == 0:
            sg.init(P)
        else:
            sg.init(ref["P"][0], simtime=ref["dt"][0])
            sg.timestep, sg.last_dt = 1, ref["dt"][0]
        dt = sg.calculate_timestep()
        assert abs(dt - ref["dt"][start]) <= FAST_TOL * ref["dt"][start], (dt, ref["dt"][start])
        sg.dt = ref["dt"][start]
        sg.advance_time()
        got = g.download(0)
    n = ongrid(cfg, got).shape[1]
    assert_fast_close(cfg, ongrid(cfg, got), ongrid(cfg, ref["P"][start]), "%s start %d" % (_case_id(case), start),
                      n // 200)


@pytest.mark.parametrize("route", ["calc_dt", "download"])
@pytest.mark.parametrize("case", [("B", abi.EQEUL, abi.FLUX_RS_HLL, 1, AV1), ("A", abi.EQGLM, abi.FLUX_RS_HLL, 1, AV1)],
                         ids=_case_id)
def test_negative_density_through_a_stage(case, route):
    """A step of 8 x the CFL step empties cells: the oracle raises "Negative density", the device must report
    EPHYSICS naming it no later than the first calc_dt() or download() after advance_time.  At 2 x neither does and
    the results agree bit for bit; after the error an upload of the clean state steps as if nothing had happened."""
    from pion_amd import lib
    cfg, P, setup = hypersonic(*case, 1)
    want = {}
    with CpuSim(cfg, "orc") as o:
        so = driver.SimControl(o, cfg)
        so.init(P)
        dt0 = so.calculate_timestep()
        so.dt = 8.0 * dt0
        with pytest.raises(RuntimeError, match="(?i)negative density"):
            so.advance_time()
    for f in (2.0, 1.0):
        with CpuSim(cfg, "orc") as o:
            so = driver.SimControl(o, cfg)
            so.init(P)
            so.calculate_timestep()
            so.dt = f * dt0
            so.advance_time()
            want[f] = o.download(0)
        assert np.isfinite(want[f]).all() and count(grid_status(cfg, want[f]), P_REPAIRED) >= 30
    with _gpu(cfg) as g:
        def step(f):
            sg = driver.SimControl(g, cfg)
            sg.init(P)
            assert sg.calculate_timestep() == dt0
            sg.dt = f * dt0
            sg.advance_time()
        step(2.0)
        assert np.array_equal(g.download(0), want[2.0])
        with pytest.raises(lib.PionGpuError) as exc:
            step(8.0)
            getattr(g, route)()
        rc, msg = _error_of(exc)
        assert rc == abi.E_PHYSICS and "negative density" in msg, (rc, msg)
        step(1.0)
        g.calc_dt()
        assert np.array_equal(g.download(0), want[1.0])
