"""The launch geometry of the stage kernel k_stage_rows2 against the ORACLE, at the tiling edges.

Each case first asks the host-side probe (tests/tiling_probe.py, pion_amd/csrc/rows_tiling.h) for the plan its
shape runs with on this device and asserts the shape sits on the edge it was chosen for, so that a retune of the rows
per wavefront or of the chunk model cannot move it off that edge unnoticed.  The data are neither separable nor
symmetric (sums of sines with incommensurate wave numbers, an off-centre blast; strict build: a per-cell
perturbation of ~1e-3 on top), so a cell updated from the wrong row or not at all cannot reproduce the right value.
P and Ph are torch tensors bound to the handle, and Ph is filled with NaN before every step: a cell or x-ghost image
the half stage fails to write becomes a NaN in P, which the bit-exact comparison rejects."""
import math
import os

import numpy as np
import pytest

from pion_amd import abi, driver, problems
import tiling_probe as tp

pytestmark = pytest.mark.gpu

# environment switches read by pion_gpu_create, each run by test_launch_switch_is_result_neutral below (and
# PION_STAGE_KERNEL, PION_ROWS, PION_ROWS1 in the shape matrix); tests/test_rows_tiling.py checks that every
# getenv("PION_...") of the library is listed here or set by another test
KNOBS = [
    ("PION_ZSLOPE_LDS", "0"),
    ("PION_UNEVEN_CHUNKS", "0"),
    ("PION_ZCHUNK", "1"),
    ("PION_ZCHUNK", "3"),
    ("PION_ZCHUNK", "7"),
    ("PION_FUSE_DT", "0"),
    ("PION_SPLIT_DT_MP", "0"),
    ("PION_CONCURRENT_STRIPS", "0"),
    ("PION_ROWS1", "1"),
    ("PION_ROWS1", "3"),
    ("PION_ROWS", "1"),
    ("PION_STAGE_KERNEL", "cell"),
    ("PION_FUSE_BC", "0"),
    ("PION_ROWS_2D", "0"),
]  # end of KNOBS


def _ncu():
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count


# ---- data that cannot hide a misplaced cell ----

def rich_case(kind, ng, strict, bcs=None, ntracer=None, spike=None, cooling=False):
    """kind: 'euler' (+ tracer), 'mhd', 'glm'.  ng: 2 or 3 extents.  spike: (x, y, z) on-grid cell whose pressure is
    raised 16x (sound speed 4x); the data are then smooth, without the blast."""
    ndim = len(ng)
    if kind == "euler":
        if cooling:
            cfg, _ = problems.cooling_blast3d(4, strict_fp=strict)
            cfg.ng[0], cfg.ng[1], cfg.ng[2] = ng
            cfg.dx = 3.160064e18 / ng[0]
        else:
            ntr = 1 if ntracer is None else ntracer
            b = bcs or ["reflecting", "outflow"] * ndim
            cfg = abi.make_config(ndim, ng, abi.EQEUL, abi.FLUX_RSroe, ntracer=ntr, artvisc=abi.AV_FKJ98_1D, etav=0.1,
                                  gamma=5.0 / 3.0, cfl=0.3, dx=1.0 / ng[0], bcs=b, strict_fp=strict,
                                  refvec=[1.0, 0.1, 1.0, 1.0, 1.0] + [1.0] * ntr)
    else:
        eq = abi.EQGLM if kind == "glm" else abi.EQMHD
        b = bcs or ["periodic"] * (2 * ndim)
        cfg = abi.make_config(ndim, ng, eq, abi.FLUX_RS_HLLD, artvisc=abi.AV_FKJ98_1D, etav=0.1, gamma=5.0 / 3.0,
                              cfl=0.24, dx=1.0 / ng[0], bcs=b, strict_fp=strict,
                              refvec=[1.0, 0.1, 1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 1.0][:cfg_nv(eq)])
    P = problems.alloc(cfg)
    X, Y, Z = problems.mesh(cfg)
    L = [cfg.ng[a] * cfg.dx for a in range(3)]
    u = (X - cfg.xmin[0]) / L[0]
    v = (Y - cfg.xmin[1]) / L[1]
    w = (Z - cfg.xmin[2]) / L[2] if ndim > 2 else 0.0 * X
    tau = 2.0 * math.pi
    f1 = np.sin(tau * (1.37 * u + 0.61 * v + 0.29 * w) + 0.4)
    f2 = np.sin(tau * (0.83 * u - 1.71 * v + 0.53 * w) + 1.1)
    f3 = np.cos(tau * (2.11 * u + 0.47 * v - 1.23 * w) + 0.7)
    blast = ((u - 0.31) ** 2 + (v - 0.58) ** 2 + ((w - 0.44) ** 2 if ndim > 2 else 0.0)) < 0.16 ** 2
    if spike is not None:
        blast[...] = False   # (the spike alone sets the time step)
    rho0, p0 = 1.0, 0.1
    if cooling:
        rho0, p0 = 2.124229813e-24, 2.124229813e-24 * 7.5e3 / (0.609 * 1.672621898e-24 / 1.38064852e-16)
    cs = math.sqrt(5.0 / 3.0 * p0 / rho0)
    P[abi.RO] = rho0 * (1.0 + 0.2 * f1 + 0.1 * f2)
    P[abi.PG] = p0 * (1.0 + 0.15 * f2 + 0.1 * f3) * np.where(blast, 10.0, 1.0)
    P[abi.VX] = cs * (0.3 * f3 + 0.05)
    P[abi.VY] = cs * (0.25 * f1 - 0.07)
    P[abi.VZ] = cs * (0.2 * f2 + 0.02)
    if kind != "euler":
        P[abi.BX] = 0.7 + 0.05 * f2
        P[abi.BY] = 0.7 - 0.05 * f3
        P[abi.BZ] = 0.3 + 0.05 * f1
    for t in range(cfg.nvar - (5 if kind == "euler" else cfg_nv(cfg.eqntype))):
        P[cfg.nvar - 1 - t] = 0.5 + 0.3 * f1 * f2
    if strict and spike is None:
        rng = np.random.default_rng(1234)
        for var in (abi.RO, abi.PG, abi.VX):
            P[var] *= 1.0 + 1e-3 * rng.uniform(-1.0, 1.0, P[var].shape)
    if spike is not None:
        nb = cfg.nbc
        x, y, z = spike
        idx = (z + nb, y + nb, x + nb) if ndim == 3 else (y + nb, x + nb)
        P[abi.PG][idx] *= 16.0
    return cfg, P


def cfg_nv(eq):
    return {abi.EQMHD: 8, abi.EQGLM: 9}[eq]


# ---- running against the oracle with a poisoned Ph ----

class _Env:
    def __init__(self, env):
        self.env = env or {}

    def __enter__(self):
        self.old = {k: os.environ.get(k) for k in self.env}
        os.environ.update(self.env)

    def __exit__(self, *a):
        for k, v in self.old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def _cooling_setup(cfg, sim):
    if cfg.cooling:
        from pion_amd import cooling
        sim.set_cooling_tables(*cooling.build_tables(cfg.min_temp, cfg.max_temp))


def run_gpu(cfg, P, nsteps, env=None, comm=None):
    """run nsteps on the GPU with P / Ph in torch tensors and Ph poisoned before every step; returns the dts, the
    state after every step and (t_dyn, t_mp) the handle computes after the last step"""
    import torch
    from pion_amd import lib
    from test_gpu_split_stage import SelfComm
    with _Env(env):
        g = lib.GpuSim(cfg, 0)
    with g:
        n = cfg.nvar * g.ncell
        tP = torch.zeros(n, dtype=torch.float64, device="cuda:0")
        tPh = torch.zeros(n, dtype=torch.float64, device="cuda:0")
        g.bind_device_state(tP.data_ptr(), tPh.data_ptr())
        _cooling_setup(cfg, g)
        cm = None if comm is None else SelfComm(g, comm == "streams")
        sg = driver.SimControl(g, cfg, comm=cm)
        sg.init(P)
        dts, states = [], []
        for it in range(nsteps):
            dts.append(sg.calculate_timestep())
            g.synchronize()
            tPh.fill_(float("nan"))
            torch.cuda.synchronize()
            g.synchronize()
            sg.advance_time()
            if comm is not None:
                sg.finish_halo()
            g.synchronize()
            states.append(tP.cpu().numpy().reshape(g.shape).copy())
        last_dt = g.calc_dt()
        del tP, tPh
    return dts, states, last_dt


def run_oracle(cfg, P, nsteps, dts):
    from cpu_backends import CpuSim
    with CpuSim(cfg, "orc") as o:
        _cooling_setup(cfg, o)
        so = driver.SimControl(o, cfg)
        so.init(P)
        odts, states = [], []
        for it in range(nsteps):
            odts.append(so.calculate_timestep())
            so.dt = dts[it]
            so.advance_time()
            states.append(o.download(0))
        return odts, states, o.calc_dt()


def compare(cfg, P, nsteps=2, strict=True, tol=0.0, env=None, comm=None):
    dts, gs, glast = run_gpu(cfg, P, nsteps, env=env, comm=comm)
    odts, os_, olast = run_oracle(cfg, P, nsteps, dts)
    for it in range(nsteps):
        a, b = gs[it], os_[it]
        if strict:
            assert dts[it] == odts[it], (it, dts[it], odts[it])
            bad = np.argwhere(a != b)
            assert len(bad) == 0, "step %d: %d values differ, first (var, z, y, x) %s: %r vs %r" % (
                it, len(bad), tuple(bad[0]), a[tuple(bad[0])], b[tuple(bad[0])])
        else:
            assert abs(dts[it] - odts[it]) <= 1e-11 * odts[it]
            assert np.isfinite(a).all(), "step %d: %d non-finite values" % (it, (~np.isfinite(a)).sum())
            scale = np.abs(b).reshape(cfg.nvar, -1).max(axis=1).reshape((-1,) + (1,) * (a.ndim - 1)) + 1e-300
            assert np.max(np.abs(a - b) / scale) <= tol, np.max(np.abs(a - b) / scale)
    if strict:
        assert glast == olast, (glast, olast)
    return dts, gs


# ---- the shape matrix ----

def _plan_for(cfg, second_order=True, env=None):
    env = env or {}
    ndim = cfg.ndim
    nx, ny = cfg.ng[0], cfg.ng[1]
    npl = cfg.ng[2] if ndim == 3 else 1
    euler = cfg.eqntype == abi.EQEUL
    # (pion_gpu_create: PION_ROWS sets both stages' rows, PION_ROWS1 then the first-order stage's)
    wr = int(env.get("PION_ROWS", 0))
    wr = wr if 1 <= wr <= 64 else 0
    wr1 = int(env.get("PION_ROWS1", wr))
    wr1 = wr1 if 1 <= wr1 <= 8 else 0
    p = tp.plan(ndim, nx, ny, npl, cfg.nvar, euler, second_order, ncu=_ncu(), want_rows=wr, want_rows1=wr1,
                want_zchunk=int(env.get("PION_ZCHUNK", 0)), uneven=env.get("PION_UNEVEN_CHUNKS", "1") != "0",
                zslope_lds=env.get("PION_ZSLOPE_LDS", "1") != "0")
    R = tp.launch_rows(p, ndim, nx, ny, cfg.nvar, second_order, zslope_lds=env.get("PION_ZSLOPE_LDS", "1") != "0",
                       ncu=_ncu(), wg_per_cu=2 if not euler else 3)
    return p, R, tp.tiling(nx, ny, R)


def _last_group_m(t):
    return t["nyg"] - 4 * ((t["nyg"] - 1) // 4)


# (id, kind, ng, env, edge check on (plan, R, tiling) of the second-order stage)
SHAPES = [
    ("rem0_62", "glm", [62, 10, 6], {"PION_ROWS": "2"}, lambda p, R, t: t["rem"] == 0 and t["ntx_full"] == 1),
    ("rem0_124", "euler", [124, 7, 5], {}, lambda p, R, t: t["rem"] == 0 and t["ntx_full"] == 2),
    ("rem1_63", "glm", [63, 9, 5], {}, lambda p, R, t: t["rem"] == 1 and t["spw"] == 21),
    ("rem30_92", "euler", [92, 11, 5], {"PION_ROWS": "1"}, lambda p, R, t: t["rem"] == 30 and t["spw"] == 2),
    ("rem31_93", "glm", [93, 7, 5], {}, lambda p, R, t: t["rem"] == 31 and t["spw"] == 1),
    ("rem61_123", "euler", [123, 6, 4], {}, lambda p, R, t: t["rem"] == 61 and t["spw"] == 1),
    ("rem61_61", "mhd", [61, 6, 5], {}, lambda p, R, t: t["rem"] == 61 and t["ntx_full"] == 0),
    # a partial last row group in a full tile (ny % R != 0)
    ("partial_full_tile", "euler", [62, 10, 4], {"PION_ROWS": "3"},
     lambda p, R, t: R == 3 and 10 % R and t["rem"] == 0),
    # the partial last group in segment 1 of a remainder wavefront: rem 20 -> 2 segments, 4 groups
    ("partial_segment1", "euler", [20, 11, 4], {"PION_ROWS": "3"},
     lambda p, R, t: R == 3 and t["spw"] == 2 and t["nyg"] % 2 == 0 and 11 % R),
    # the last 4-group of a full tile holds m = 1, 2, 3 row groups
    ("last4_m1", "glm", [62, 10, 4], {"PION_ROWS": "2"}, lambda p, R, t: R == 2 and _last_group_m(t) == 1),
    ("last4_m2", "euler", [62, 12, 4], {"PION_ROWS": "2"}, lambda p, R, t: R == 2 and _last_group_m(t) == 2),
    ("last4_m3", "euler", [62, 14, 4], {"PION_ROWS": "2"}, lambda p, R, t: R == 2 and _last_group_m(t) == 3),
    # a remainder wavefront whose trailing segments are idle: rem 8 -> 6 segments, 4 groups
    ("idle_segments", "glm", [8, 4, 5], {"PION_ROWS": "1"}, lambda p, R, t: t["spw"] == 6 and t["nyg"] % 6 == 4),
    # z: nz = 2 nbc (no split), around the uneven-chunk threshold, PION_ZCHUNK with uneven chunks on and off
    ("nz4", "glm", [20, 6, 4], {}, lambda p, R, t: p["nzb"] == 0),
    ("nz15", "euler", [20, 6, 15], {"PION_ZCHUNK": "4"}, lambda p, R, t: p["nzb"] == 0),
    ("nz16", "euler", [20, 6, 16], {"PION_ZCHUNK": "4"}, lambda p, R, t: p["nzb"] > 1),
    ("nz17", "glm", [20, 6, 17], {"PION_ZCHUNK": "4"}, lambda p, R, t: p["nzb"] > 1),
    ("zchunk1_uneven", "euler", [14, 5, 18], {"PION_ZCHUNK": "1"}, lambda p, R, t: p["nzb"] == 17),   # 16 x 1, 2
    ("zchunk3_even", "glm", [14, 5, 17], {"PION_ZCHUNK": "3", "PION_UNEVEN_CHUNKS": "0"},
     lambda p, R, t: p["nzb"] == 0 and p["zchunk"] == 3),
    # x boundaries: periodic (the xwrap ghost images), reflecting / outflow
    ("periodic_x_rem1", "euler_periodic", [63, 7, 5], {}, lambda p, R, t: t["rem"] == 1),
    ("reflect_outflow_rem31", "euler", [93, 5, 4], {}, lambda p, R, t: t["rem"] == 31),
    # HLLD flag prepass, dense kernel (9 all-cell planes): its x tiles (gx) at nga0 = nx + 4 = 62 and 63 and its y tiles
    # (gy) at nga1 not a multiple of 4
    ("prepass_nga0_62", "glm", [58, 9, 5], {}, lambda p, R, t: (58 + 4) % 62 == 0 and (9 + 4) % 4),
    ("prepass_nga0_63", "mhd", [59, 9, 5], {}, lambda p, R, t: (59 + 4) % 62 == 1 and (9 + 4) % 4),
    # ... and the marching kernel, which launch_prepass takes from PION_PREPASS_ZC = 16 all-cell planes up, at its
    # 62-cells-per-wavefront x edges; without the screen every stage takes the dense path
    # (their edge is checked on the configuration itself, in the test)
    ("prepass_march_nga0_62", "glm", [58, 9, 12], {"PION_HLL_SCREEN": "0"}, lambda p, R, t: True),
    ("prepass_march_nga0_63", "mhd", [59, 9, 12], {"PION_HLL_SCREEN": "0"}, lambda p, R, t: True),
    # the cell kernel at nx % 64 == 1 and ny % 4 == 1
    ("cell_kernel", "glm", [65, 5, 4], {"PION_STAGE_KERNEL": "cell"}, lambda p, R, t: True),
    ("cell_kernel_euler", "euler", [65, 9, 4], {"PION_STAGE_KERNEL": "cell"}, lambda p, R, t: True),
    # 2-D with the same x edges, R forced 1, 7, 64 and automatic
    ("2d_rem0_R1", "glm", [62, 9], {"PION_ROWS": "1"}, lambda p, R, t: R == 1 and t["rem"] == 0),
    ("2d_rem1_R7", "euler", [63, 20], {"PION_ROWS": "7"}, lambda p, R, t: R == 7 and t["rem"] == 1),
    ("2d_rem31_R64", "glm", [93, 70], {"PION_ROWS": "64"}, lambda p, R, t: R == 64 and 70 % 64),
    ("2d_rem61_auto", "euler", [123, 40], {}, lambda p, R, t: t["rem"] == 61),
    ("2d_periodic_rem30", "euler_periodic", [92, 13], {"PION_ROWS": "7"}, lambda p, R, t: t["rem"] == 30),
]


def _shape_case(kind, ng, strict):
    if kind == "euler_periodic":
        return rich_case("euler", ng, strict, bcs=["periodic"] * (2 * len(ng)))
    return rich_case(kind, ng, strict)


@pytest.mark.parametrize("name,kind,ng,env,edge", SHAPES, ids=[s[0] for s in SHAPES])
def test_shape_strict_bitexact_vs_oracle(name, kind, ng, env, edge):
    cfg, P = _shape_case(kind, ng, 1)
    if name.startswith("prepass_march"):
        # PION_PREPASS_ZC = 16 all-cell planes (kernels_prepass.hip), and all-cell rows of 62 k or 62 k + 1 cells
        assert cfg.ng[2] + 2 * cfg.nbc >= 16 and (cfg.ng[0] + 4) % 62 in (0, 1), ("the case is off its edge", name)
    if env.get("PION_STAGE_KERNEL") != "cell":
        p, R, t = _plan_for(cfg, True, env)
        assert edge(p, R, t), ("the case is off its edge", name, p, R, t)
        # and the probe's coverage of that exact launch
        nz = cfg.ng[2] if cfg.ndim == 3 else 1
        tp.check_launches(cfg.ndim, cfg.ng[0], cfg.ng[1], nz, cfg.nbc,
                          [dict(rows=R, kz0=0, kz1=nz, zchunk=p["zchunk"], nzb=p["nzb"], zcmax=p["zcmax"])])
    compare(cfg, P, 2, env=env)


FAST_SHAPES = ["rem0_62", "rem1_63", "rem31_93", "rem61_123", "partial_segment1", "nz17", "periodic_x_rem1"]


@pytest.mark.parametrize("name", FAST_SHAPES)
def test_shape_fast_vs_oracle(name):
    _, kind, ng, env, _ = [s for s in SHAPES if s[0] == name][0]
    if kind == "euler_periodic":
        cfg, P = rich_case("euler", ng, 0, bcs=["periodic"] * (2 * len(ng)))
    else:
        cfg, P = rich_case(kind, ng, 0)
    compare(cfg, P, 2, strict=False, tol=3e-11, env=env)


# ---- the fused time-step reduction at the seams ----

def _np_cell_dt(cfg, P):
    """a numpy restatement of the hydro cell time step (the minimum's location is what matters)"""
    nb = cfg.nbc
    s = (slice(None),) + (slice(nb, -nb),) * cfg.ndim
    Q = P[s]
    cs = np.sqrt(cfg.gamma * Q[abi.PG] / Q[abi.RO])
    vmax = np.maximum(np.maximum(np.abs(Q[abi.VX]), np.abs(Q[abi.VY])), np.abs(Q[abi.VZ]))
    return cfg.cfl * cfg.dx / (vmax + cs)


# (id, ng, env, spike cell (x, y, z))
SEAMS = [
    ("first_writer_full_tile", [70, 9, 6], {"PION_ROWS": "2"}, (0, 4, 3)),
    ("last_writer_full_tile", [70, 9, 6], {"PION_ROWS": "2"}, (61, 5, 2)),
    ("last_cell_remainder_segment", [70, 9, 6], {"PION_ROWS": "2"}, (69, 8, 3)),
    ("last_row_partial_group", [40, 11, 6], {"PION_ROWS": "3"}, (17, 10, 4)),
    ("first_plane_uneven_chunk", [20, 6, 24], {"PION_ZCHUNK": "8"}, (9, 3, 16)),
    ("last_plane_uneven_chunk", [20, 6, 24], {"PION_ZCHUNK": "8"}, (11, 2, 23)),
]


@pytest.mark.parametrize("name,ng,env,spike", SEAMS, ids=[s[0] for s in SEAMS])
def test_fused_dt_sees_the_seam_cell(name, ng, env, spike):
    cfg, P = rich_case("euler", ng, 1, spike=spike)
    if name.endswith("uneven_chunk"):
        p, R, t = _plan_for(cfg, True, env)
        n, ch = tp.zchunks(ng[2], p["zcmax"])
        assert p["nzb"] == n > 1 and any(spike[2] in (k0, k1 - 1) and k1 - k0 < 8 for k0, k1 in ch[:n]), (p, ch)
    dts, gs = compare(cfg, P, 1, env=env)
    # the spike is where the next dt comes from
    dtc = _np_cell_dt(cfg, gs[0])
    loc = np.unravel_index(np.argmin(dtc), dtc.shape)[::-1]
    assert max(abs(int(a) - b) for a, b in zip(loc, spike)) <= 1, (loc, spike)
    _, gs1, fused = run_gpu(cfg, P, 1, env=env)
    _, gs2, kern = run_gpu(cfg, P, 1, env=dict(env, PION_FUSE_DT="0"))
    assert np.array_equal(gs1[0], gs2[0])
    assert fused == kern, (fused, kern)


def test_fused_dt_sees_the_upper_strip_of_a_split_stage():
    cfg, P = rich_case("euler", [20, 6, 12], 1, bcs=["periodic"] * 6, spike=(7, 3, 11))
    dts, gs, fused = run_gpu(cfg, P, 1, comm="streams")
    _, os_, olast = run_oracle(cfg, P, 1, dts)
    assert np.array_equal(gs[0], os_[0])
    assert fused == olast, (fused, olast)
    dtc = _np_cell_dt(cfg, gs[0])
    loc = np.unravel_index(np.argmin(dtc), dtc.shape)[::-1]
    assert max(abs(int(a) - b) for a, b in zip(loc, (7, 3, 11))) <= 1, loc


# ---- every launch switch is result-neutral ----

@pytest.mark.parametrize("knob,value", KNOBS, ids=["%s=%s" % k for k in KNOBS])
def test_launch_switch_is_result_neutral(knob, value):
    env = {knob: value}
    if knob == "PION_SPLIT_DT_MP":
        cfg, P = rich_case("euler", [20, 6, 20], 1, cooling=True)
    elif knob == "PION_ROWS_2D":
        cfg, P = rich_case("glm", [70, 30], 1)   # (2-D: the rows kernel against the cell kernel)
    else:
        cfg, P = rich_case("glm", [40, 9, 44], 1)
        p, R, t = _plan_for(cfg, True, {})
        n, ch = tp.zchunks(44, p["zcmax"])
        assert p["nzb"] > 1 and len({k1 - k0 for k0, k1 in ch[:n]}) > 1, (p, ch)   # uneven chunks of several lengths
    dts0, gs0, last0 = run_gpu(cfg, P, 2)
    dts1, gs1, last1 = run_gpu(cfg, P, 2, env=env)
    assert dts0 == dts1 and last0 == last1, (dts0, dts1, last0, last1)
    for a, b in zip(gs0, gs1):
        assert np.array_equal(a, b)
    _, os_, olast = run_oracle(cfg, P, 2, dts0)
    assert np.array_equal(gs0[-1], os_[-1]) and last0 == olast


@pytest.mark.parametrize("knob,value", [("PION_CONCURRENT_STRIPS", "0"), ("PION_ZCHUNK", "3"),
                                        ("PION_UNEVEN_CHUNKS", "0"), ("PION_FUSE_DT", "0"), ("PION_ROWS1", "3")])
def test_launch_switch_is_result_neutral_split_stage(knob, value):
    cfg, P = rich_case("glm", [30, 7, 40], 1)
    dts0, gs0, last0 = run_gpu(cfg, P, 2, comm="streams")
    dts1, gs1, last1 = run_gpu(cfg, P, 2, env={knob: value}, comm="streams")
    assert dts0 == dts1 and last0 == last1, (dts0, dts1)
    for a, b in zip(gs0, gs1):
        assert np.array_equal(a, b)
    _, os_, olast = run_oracle(cfg, P, 2, dts0)
    assert np.array_equal(gs0[-1], os_[-1]) and last0 == olast
