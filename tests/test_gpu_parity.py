"""GPU parity tests (call through the C-ABI, compare with the CPU oracle).

strict_fp=1 kernels are built without FMA contraction: every comparison below is
BIT-EXACT for them.  strict_fp=0 (production) kernels are held to a relative
tolerance of 1e-11 per step on smooth data (fp64, a handful of ulps from FMA)."""
import numpy as np
import pytest

from pion_amd import abi, driver, problems

pytestmark = pytest.mark.gpu


def _gpu(cfg):
    from pion_amd import lib
    return lib.GpuSim(cfg, 0)


def _cpu(cfg):
    from cpu_backends import CpuSim
    return CpuSim(cfg, "orc")


def run_pair(cfg, P, nsteps, strict=True, tol=0.0, first_dt_limit=None, setup=None, after=None):
    """after(g): called with the device handle once the last step has been compared, before the handles close"""
    with _gpu(cfg) as g, _cpu(cfg) as o:
        if setup:
            setup(g)
            setup(o)
        sg, so = driver.SimControl(g, cfg), driver.SimControl(o, cfg)
        sg.first_step_dt_limit = so.first_step_dt_limit = first_dt_limit
        sg.init(P)
        so.init(P)
        a, b = g.download(0), o.download(0)
        assert np.array_equal(a, b), "boundary assignment differs"
        for it in range(nsteps):
            dg, do = sg.calculate_timestep(), so.calculate_timestep()
            if strict:
                assert dg == do, (it, dg, do)
            else:
                assert abs(dg - do) <= 1e-11 * do
            so.dt = sg.dt
            sg.advance_time()
            so.advance_time()
            a, b = g.download(0), o.download(0)
            if strict:
                assert np.array_equal(a, b), "step %d: %d values differ, max abs %g" % (
                    it, (a != b).sum(), np.abs(a - b).max())
            else:
                scale = np.abs(b).reshape(cfg.nvar, -1).max(axis=1).reshape(-1, 1, 1, 1) + 1e-300
                assert np.max(np.abs(a - b) / scale) <= tol, np.max(np.abs(a - b) / scale)
        if after:
            after(g)


HD_SOLVERS = [abi.FLUX_RSroe, abi.FLUX_RSroe_pv, abi.FLUX_FVS, abi.FLUX_RS_HLL]


@pytest.mark.parametrize("solver", HD_SOLVERS)
@pytest.mark.parametrize("ndim", [1, 2, 3])
def test_hd_blast_strict(solver, ndim):
    n = {1: 96, 2: 40, 3: 20}[ndim]
    cfg, P = problems.hd_blast_octant(n, ndim, solver=solver, ntracer=1, strict_fp=1, nzones=3.0)
    run_pair(cfg, P, 3)


@pytest.mark.parametrize("av", [abi.AV_NONE, abi.AV_HCORRECTION, abi.AV_HCORR_FKJ98])
@pytest.mark.parametrize("ndim", [1, 2, 3])
def test_hd_roe_viscosities_strict(av, ndim):
    n = {1: 96, 2: 40, 3: 20}[ndim]
    cfg, P = problems.hd_blast_octant(n, ndim, solver=abi.FLUX_RSroe, artvisc=av, strict_fp=1, nzones=3.0)
    run_pair(cfg, P, 3)


@pytest.mark.parametrize("solver", [abi.FLUX_RSlinear, abi.FLUX_RSexact, abi.FLUX_RShybrid])
def test_hd_exact_hybrid(solver):
    # exp/log/pow of the device maths library differ from glibc in the last bits
    cfg, P = problems.hd_blast_octant(32, 2, solver=solver, strict_fp=1, nzones=3.0)
    run_pair(cfg, P, 3, strict=False, tol=1e-9)


@pytest.mark.parametrize("eq", [abi.EQMHD, abi.EQGLM])
@pytest.mark.parametrize("solver", [abi.FLUX_RS_HLLD, abi.FLUX_RS_HLL])
@pytest.mark.parametrize("ndim", [2, 3])
def test_mhd_blast_strict(eq, solver, ndim):
    n = {2: 48, 3: 20}[ndim]
    cfg, P = problems.mhd_blastwave(n, ndim, eq, solver, strict_fp=1)
    run_pair(cfg, P, 3)


@pytest.mark.parametrize("ndim", [2, 3])
def test_glm_mixed_bcs_strict(ndim):
    bcs = ["outflow", "one-way-outflow", "reflecting", "outflow", "one-way-outflow", "reflecting"][:2 * ndim]
    cfg, P = problems.mhd_smooth({2: 40, 3: 18}[ndim], ndim, abi.EQGLM, abi.FLUX_RS_HLLD, bcs=bcs)
    run_pair(cfg, P, 3)


def test_dmr_strict():
    cfg, P = problems.double_mach_reflection(104, strict_fp=1)
    run_pair(cfg, P, 5)


def test_first_order_lf_strict():
    cfg, P = problems.hd_blast_octant(24, 3, solver=abi.FLUX_LF, strict_fp=1, nzones=3.0)
    cfg.sp_ooa = cfg.tm_ooa = 1
    run_pair(cfg, P, 3)


def test_fast_mode_tolerance():
    """Production kernels (FMA contraction): 1e-11 of each variable's scale per step on smooth data."""
    cfg, P = problems.mhd_smooth(32, 3, abi.EQGLM, abi.FLUX_RS_HLLD, strict_fp=0)
    run_pair(cfg, P, 3, strict=False, tol=1e-11)


@pytest.mark.parametrize("solver", [abi.FLUX_RSroe, abi.FLUX_FVS, abi.FLUX_RS_HLL])
def test_fast_mode_tolerance_hd(solver):
    """Production (fast) Euler kernels against the oracle on a 3-D blast with a tracer: FMA contraction,
    rsq-seeded roots and the division-free equalD move results by rounding only (1e-10 of each
    variable's scale after three steps across a shock)."""
    cfg, P = problems.hd_blast_octant(20, 3, solver=solver, ntracer=1, strict_fp=0, nzones=3.0)
    run_pair(cfg, P, 3, strict=False, tol=1e-10)


@pytest.mark.parametrize("eq,solvers", [(abi.EQEUL, [0, 1, 2, 3, 4, 5, 6, 8]), (abi.EQMHD, [0, 7, 8]), (abi.EQGLM, [0, 7, 8])])
def test_interface_flux_strict(eq, solvers):
    rng = np.random.default_rng(7)
    for sv in solvers:
        for ntr in (0, 2):
            for av in ((0, 1, 4) if sv == 4 else (1,)):
                cfg = abi.make_config(3, [4, 4, 4], eq, sv, ntracer=ntr, artvisc=av, xmax=(1, 1, 1), strict_fp=1)
                L, R = problems.random_states(rng, 2000, eq, ntr)
                aux = np.zeros((2000, 4))
                if av == 4:
                    aux[:, 0] = rng.uniform(0, 2, 2000)
                if sv == 7:
                    aux[:, 1] = rng.uniform(0, 1, 2000) < 0.3
                with _gpu(cfg) as g, _cpu(cfg) as o:
                    g.set_glm_speeds(0.01, cfg.dx, 0.25 / cfg.dx)
                    o.set_glm_speeds(0.01, cfg.dx, 0.25 / cfg.dx)
                    for ax in range(3):
                        Fg, _ = g.interface_flux(ax, L, R, aux, dt=0.01)
                        Fo, _ = o.interface_flux(ax, L, R, aux, dt=0.01)
                        if eq == abi.EQEUL and sv in (1, 2, 3):
                            # rarefaction/cavitation branches use exp/log/pow (riemann.cpp:829-963):
                            # device libm vs glibc differ in the last bits
                            ok = np.isfinite(Fo)
                            assert np.array_equal(np.isfinite(Fg), ok)
                            sc = np.abs(Fo[ok]).max()
                            assert np.max(np.abs(Fg[ok] - Fo[ok])) <= 1e-12 * sc
                        else:
                            assert np.array_equal(Fg, Fo, equal_nan=True), (eq, sv, ntr, av, ax,
                                                                             np.nanmax(np.abs(Fg - Fo)))


@pytest.mark.parametrize("eq,solvers", [(abi.EQEUL, [4, 6, 8]), (abi.EQMHD, [7, 8]), (abi.EQGLM, [7, 8])])
def test_interface_flux_fast_vs_oracle(eq, solvers):
    """The production (fast) build's interface fluxes on random left/right states against the oracle: the
    one-sided HLLD, the rsq/rcp-seeded roots and reciprocals, the fused source terms and FMA contraction
    change the result by rounding only: 99.9 % of 4000 random state pairs per axis within 1e-12 of the
    largest flux component (measured 1.5e-14), every pair within 1e-10 (measured 1.2e-11, GLM HLLD at a
    pair close to the fast = Alfven degeneracy, where 1/(rho (S_K-v_K)(S_K-S_M) - B_n^2) amplifies
    rounding in either build).  The random pairs include jumps of B_n that make the star density of the
    unselected side negative in ideal MHD: the flux must stay finite there (it once came out as 0 x NaN)."""
    rng = np.random.default_rng(11)
    for sv in solvers:
        cfg = abi.make_config(3, [4, 4, 4], eq, sv, ntracer=0, artvisc=1, xmax=(1, 1, 1), strict_fp=0)
        cfo = abi.make_config(3, [4, 4, 4], eq, sv, ntracer=0, artvisc=1, xmax=(1, 1, 1), strict_fp=1)
        L, R = problems.random_states(rng, 4000, eq, 0)
        aux = np.zeros((4000, 4))
        with _gpu(cfg) as g, _cpu(cfo) as o:
            g.set_glm_speeds(0.01, cfg.dx, 0.25 / cfg.dx)
            o.set_glm_speeds(0.01, cfo.dx, 0.25 / cfo.dx)
            for ax in range(3):
                Fg, _ = g.interface_flux(ax, L, R, aux, dt=0.01)
                Fo, _ = o.interface_flux(ax, L, R, aux, dt=0.01)
                assert np.isfinite(Fg).all() and np.isfinite(Fo).all()
                sc = np.abs(Fo).max(axis=1, keepdims=True) + 1e-300
                err = (np.abs(Fg - Fo) / sc).max(axis=1)
                assert err.max() <= 1e-10, (eq, sv, ax, err.max())
                assert np.quantile(err, 0.999) <= 1e-12, (eq, sv, ax, np.quantile(err, 0.999))


def _with_tracers(cfg0, P0, ntr):
    """same problem with ntr extra passive tracers (blast region = 1)"""
    base = cfg0.nvar - cfg0.ntracer
    bcs = [cfg0.bc_type[d] for d in range(2 * cfg0.ndim)]
    cfg = abi.make_config(cfg0.ndim, [cfg0.ng[a] for a in range(cfg0.ndim)], cfg0.eqntype, cfg0.solver, ntracer=ntr,
                          artvisc=cfg0.artvisc, etav=cfg0.etav, gamma=cfg0.gamma, cfl=cfg0.cfl, dx=cfg0.dx,
                          xmin=tuple(cfg0.xmin), bcs=bcs, refvec=[cfg0.refvec[v] for v in range(base)] + [1.0] * ntr,
                          strict_fp=cfg0.strict_fp)
    P = np.zeros((cfg.nvar,) + P0.shape[1:])
    P[:base] = P0[:base]
    hot = P0[abi.PG] > 2.0 * P0[abi.PG].min()
    for t in range(ntr):
        P[base + t] = np.where(hot, 1.0 - 0.25 * t, 0.1 * t)
    return cfg, P


def _fast_rows_vs_cell(cfg, P, nsteps, monkeypatch):
    """SECONDARY check (the primary one is the oracle comparison next to each call): fast-mode (FMA) instance of
    k_stage_rows2 against the fast cell-per-thread kernel k_stage -- the same arithmetic in a different code
    shape, so they agree to rounding, also on the degenerate symmetric blast where no build-independent answer
    exists (tests/test_reference_conditioning.py)"""
    out = {}
    for kern in ("rows", "cell"):
        monkeypatch.setenv("PION_STAGE_KERNEL", kern)
        with _gpu(cfg) as g:
            sg = driver.SimControl(g, cfg)
            sg.init(P)
            for _ in range(nsteps):
                sg.calculate_timestep()
                sg.advance_time()
            out[kern] = g.download(0)
    a, b = out["rows"], out["cell"]
    scale = np.abs(b).reshape(cfg.nvar, -1).max(axis=1).reshape(-1, 1, 1, 1) + 1e-300
    assert np.isfinite(a).all()
    assert np.max(np.abs(a - b) / scale) <= 1e-12, np.max(np.abs(a - b) / scale)


@pytest.mark.parametrize("strict", [1, 0])
@pytest.mark.parametrize("ntr", [0, 1, 2])
@pytest.mark.parametrize("solver", [0, 1, 2, 3, 4, 5, 6, 8])
def test_every_hd_instantiation_3d(solver, ntr, strict, monkeypatch):
    """every (solver, ntracer, fp mode) template instance of the 3-D stage kernel: this hipcc has
    miscompiled single instances (registers mixed up under -O3, under SLP, and at -O2 before the
    wavefront index was made uniform with readfirstlane, see csrc/Makefile), so each one is run"""
    cfg0, P0 = problems.hd_blast_octant(14, 3, solver=solver, strict_fp=strict, nzones=3.0)
    cfg, P = _with_tracers(cfg0, P0, ntr)
    if not strict:
        # primary: the fast instance against the ORACLE, cell by cell; secondary: against the fast
        # cell-per-thread kernel (same arithmetic, other code shape)
        run_pair(cfg, P, 2, strict=False, tol=1e-9 if solver in (1, 2, 3) else 1e-10)
        _fast_rows_vs_cell(cfg, P, 2, monkeypatch)
    elif solver in (1, 2, 3):
        run_pair(cfg, P, 2, strict=False, tol=1e-9)
    else:
        run_pair(cfg, P, 2)


@pytest.mark.parametrize("strict", [1, 0])
@pytest.mark.parametrize("ntr", [0, 1, 2])
@pytest.mark.parametrize("solver", [0, 1, 4, 7, 8])
@pytest.mark.parametrize("eq", [abi.EQMHD, abi.EQGLM])
def test_every_mhd_instantiation_3d(eq, solver, ntr, strict, monkeypatch):
    cfg0, P0 = problems.mhd_blastwave(14, 3, eq, solver, strict_fp=strict)
    cfg, P = _with_tracers(cfg0, P0, ntr)
    if strict:
        run_pair(cfg, P, 2)
    else:
        # primary: the fast instance against the ORACLE, cell by cell, on the blast without the degeneracies on
        # which the reference itself is discontinuous (tests/test_reference_conditioning.py); secondary: against
        # the fast cell-per-thread kernel on the symmetric blast (same arithmetic, other code shape)
        cfg_g, P_g = problems.mhd_blast_generic([14, 14, 14], eq, solver, strict_fp=0, ntracer=ntr)
        run_pair(cfg_g, P_g, 2, strict=False, tol=1e-10)
        _fast_rows_vs_cell(cfg, P, 2, monkeypatch)


@pytest.mark.parametrize("strict", [1, 0])
@pytest.mark.parametrize("case", ["hd", "mhd", "glm", "wind"])
def test_fused_dt_equals_dt_kernel(case, strict):
    """the full stage of k_stage_rows2 leaves (t_dyn, t_mp) of the new state behind; it must be what
    k_dt computes from that state (calc_timestep.cpp:271-507)"""
    from pion_amd import cooling
    setup = None
    dtl = None
    if case == "hd":
        cfg, P = problems.hd_blast_octant(14, 3, solver=abi.FLUX_RSroe, strict_fp=strict, nzones=3.0)
    elif case == "wind":
        cfg, P, (idx, st), dtl = problems.wind3d(16, strict_fp=strict)
        T, tabs, sl = cooling.build_tables(cfg.min_temp, cfg.max_temp)

        def setup(s):
            s.set_cooling_tables(T, tabs, sl)
            s.set_wind_cells(idx, st)
    else:
        cfg, P = problems.mhd_blastwave(14, 3, abi.EQGLM if case == "glm" else abi.EQMHD, abi.FLUX_RS_HLLD,
                                        strict_fp=strict)
    with _gpu(cfg) as g:
        if setup:
            setup(g)
        sg = driver.SimControl(g, cfg)
        sg.first_step_dt_limit = dtl
        sg.init(P)
        for _ in range(3):
            sg.calculate_timestep()
            sg.advance_time()
            fused = g.calc_dt()
            g.device_ptr(0)          # invalidates the cached minima -> next call runs k_dt
            kern = g.calc_dt()
            # both builds: k_dt and the fused reduction call the same function (cell_dt, dev_sweep.h), whose
            # fast-build form spells its multiply-adds out -- a restart goes through k_dt and must continue bit for bit
            assert fused == kern, (fused, kern)


@pytest.mark.parametrize("strict", [1, 0])
@pytest.mark.parametrize("ntr", [0, 1, 2])
@pytest.mark.parametrize("eq", [abi.EQMHD, abi.EQGLM])
def test_hlld_with_hcorrection_instances_3d(eq, ntr, strict, monkeypatch):
    """the HLLD instances of k_stage_rows2 exist twice (with and without the H-correction / microphysics
    code, see stage_rows2_go_z); the blast tests above run the plain ones, this one the others"""
    cfg0, P0 = problems.mhd_blastwave(14, 3, eq, abi.FLUX_RS_HLLD, strict_fp=strict)
    cfg0.artvisc = abi.AV_HCORR_FKJ98
    cfg, P = _with_tracers(cfg0, P0, ntr)
    if strict:
        run_pair(cfg, P, 2)
    else:
        cfg_g, P_g = problems.mhd_blast_generic([14, 14, 14], eq, abi.FLUX_RS_HLLD, strict_fp=0, ntracer=ntr)
        cfg_g.artvisc = abi.AV_HCORR_FKJ98
        run_pair(cfg_g, P_g, 2, strict=False, tol=1e-10)      # primary: against the oracle
        _fast_rows_vs_cell(cfg, P, 2, monkeypatch)             # secondary: against the cell-per-thread kernel


@pytest.mark.parametrize("strict", [1, 0])
@pytest.mark.parametrize("ntr", [0, 1, 2])
def test_hd_roe_with_hcorrection_instances_3d(ntr, strict, monkeypatch):
    """Euler Roe-CV is specialised like MHD HLLD (stage_rows2_go_z): the non-plain instances"""
    cfg0, P0 = problems.hd_blast_octant(14, 3, solver=abi.FLUX_RSroe, artvisc=abi.AV_HCORR_FKJ98, strict_fp=strict,
                                        nzones=3.0)
    cfg, P = _with_tracers(cfg0, P0, ntr)
    if strict:
        run_pair(cfg, P, 2)
    else:
        run_pair(cfg, P, 2, strict=False, tol=1e-10)          # primary: against the oracle
        _fast_rows_vs_cell(cfg, P, 2, monkeypatch)             # secondary: against the cell-per-thread kernel


def test_conserved_totals_fast_build_vs_cpu():
    """BASELINE gate: sums of the conserved quantities of the production (fast) build within 1e-10
    (relative to the sum of magnitudes) of the CPU reference path after several steps"""
    cfg, P = problems.mhd_blastwave(48, 3, abi.EQGLM, abi.FLUX_RS_HLLD, strict_fp=0)
    g_ = cfg.gamma

    def totals(A):
        q = A[:, 2:-2, 2:-2, 2:-2]
        ro, pg, v, B = q[0], q[1], q[2:5], q[5:8]
        E = pg / (g_ - 1.0) + 0.5 * ro * (v ** 2).sum(axis=0) + 0.5 * (B ** 2).sum(axis=0)
        vals = [ro, ro * v[0], ro * v[1], ro * v[2], E, B[0], B[1], B[2]]
        return np.array([x.sum() for x in vals]), np.array([np.abs(x).sum() for x in vals])

    with _gpu(cfg) as g, _cpu(cfg) as o:
        sg, so = driver.SimControl(g, cfg), driver.SimControl(o, cfg)
        sg.init(P)
        so.init(P)
        for _ in range(8):
            sg.calculate_timestep()
            so.calculate_timestep()
            so.dt = sg.dt
            sg.advance_time()
            so.advance_time()
        tg, ag = totals(g.download(0))
        to, _ = totals(o.download(0))
    rel = np.abs(tg - to) / (ag + 1e-300)
    assert rel.max() <= 1e-10, rel


def test_fast_ideal_mhd_blast_stays_finite_and_conserves_mass():
    """Production (fast) ideal-MHD HLLD on the blast wave, whose symmetric states sit on HLLD's degenerate
    branches (B_t = 0, fast = Alfven speed): eight steps stay finite and, the box being periodic, the
    total mass is the initial one to rounding (the flux form conserves it whatever the solver returns,
    so this catches NaNs and indexing slips, not solver accuracy)."""
    cfg, P = problems.mhd_blastwave(32, 3, abi.EQMHD, abi.FLUX_RS_HLLD, strict_fp=0)
    with _gpu(cfg) as g:
        sg = driver.SimControl(g, cfg)
        sg.init(P)
        m0 = g.download(0)[0, 2:-2, 2:-2, 2:-2].sum()
        for _ in range(8):
            sg.calculate_timestep()
            sg.advance_time()
        A = g.download(0)
    assert np.isfinite(A).all()
    m1 = A[0, 2:-2, 2:-2, 2:-2].sum()
    assert abs(m1 - m0) <= 1e-12 * m0, (m0, m1)
