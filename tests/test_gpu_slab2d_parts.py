"""2-D slabs, one process: a handle with PION_BC_SLAB on both y faces whose neighbour is the handle itself.

The slab axis of a 2-D grid is y.  The handle runs every stage as PION_STAGE_INTERIOR (rows [nbc, ny - nbc)) followed
by PION_STAGE_SLABBOUNDARY (the nbc rows next to each y face, one launch), and between the two its nbc halo rows are
copied device to device through pion_gpu_halo_spans on the communication stream -- what slab_comm_rccl does between two
ranks.  Beside it a single-domain handle, periodic in y, runs whole stages.  After each of 3 steps the on-grid part of P
and of Ph and every dt must be bit-identical, in the strict AND the fast build: a y interface is solved by one copy of
the code whichever wavefront owns it, so the result does not depend on where the row groups start.

The single-domain run is not only compared with itself: whole 2-D stages of the rows kernel are pinned to the oracle by
tests/test_gpu_xtile.py::test_2d_rows_kernel_strict_bitexact_vs_oracle (GLM HLLD, Euler Roe-CV, Euler FVS + tracer at
70 x 19) and ::test_2d_rows_kernel_fast_vs_oracle, the first-order and the non-specialised instances by
tests/test_gpu_parity.py::test_first_order_lf_strict / ::test_hd_blast_strict, the cooling source by
tests/test_gpu_cooling.py::test_wind3d_steps and tests/test_gpu_wind_sources.py::test_run_wind2d_axisymmetric_matches_oracle.

The first-order case (glm_hlld_oa1) is first order in space AND time, one of the no-split configurations: it checks that
everything then happens in the boundary call, and issues no row-range launch of its own.  The first-order range launch
(the half step of every second-order case: interior and strips of the OAMODE 1 instances) is covered by the other cases,
whose Ph is compared after every step.  test_interior_part_updates_the_interior_rows_only observes that the split is
real: a silent fall-back to "everything in the boundary call" would pass the comparisons, not that test.

Shapes: nx = 70 (one full 62-cell tile + a remainder wavefront); ny = 4 (= 2 nbc: no split, everything in the boundary
call), 5 (an interior of one row), 37 (an interior of 33 rows: no multiple of the rows per wavefront); each with the
automatic rows per wavefront and with PION_ROWS=4."""
import copy
import ctypes as C

import numpy as np
import pytest

from pion_amd import abi, cooling, driver, lib, problems
from split_checks import check_hll_switch

pytestmark = pytest.mark.gpu

NX = 70


def _hip():
    """the HIP runtime this process already uses (the one libpion_gpu.so is bound to)"""
    with open("/proc/self/maps") as f:
        paths = sorted({ln.split()[-1] for ln in f if "libamdhip64" in ln})
    assert paths, "no HIP runtime loaded"
    h = C.CDLL(paths[0])
    h.hipMemcpyAsync.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]
    h.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    return h


def _raw(g, which, put=None):
    """the device array itself (0 = P, 1 = Ph) through pion_gpu_device_ptr: GpuSim.download(1) hands out P while Ph is
    not the valid stencil array (after a full step), this reads -- or, with `put`, overwrites -- what is stored.  The
    address is asked for once per handle (asking discards the cached time step of the fused reduction)"""
    if not hasattr(g, "_raw_ptr"):
        g.lib.pion_gpu_device_ptr.argtypes = [C.c_void_p, C.c_int]
        g.lib.pion_gpu_device_ptr.restype = C.c_void_p
        g._raw_ptr = [g.lib.pion_gpu_device_ptr(g.h, w) for w in (0, 1)]
    g.synchronize()
    d = g._raw_ptr[which]
    nga = abi.ng_all(g.cfg)
    A = np.empty((g.cfg.nvar, nga[2], nga[1], nga[0])) if put is None else np.ascontiguousarray(put)
    kind = 2 if put is None else 1          # hipMemcpyDeviceToHost / HostToDevice
    assert _hip().hipMemcpy(*((A.ctypes.data, d) if put is None else (d, A.ctypes.data)), A.nbytes, kind) == 0
    return A


class SelfComm2D:
    """SlabComm's call shape for a slab that is its own neighbour, through the spans: no pack / unpack kernels"""

    def __init__(self, sim, two_streams):
        import torch
        self.hip = _hip()
        self.pending = None
        self.streams = None
        if two_streams:
            sim.synchronize()
            self.streams = (torch.cuda.Stream(), torch.cuda.Stream(priority=-1))
            sim.set_stream(self.streams[0].cuda_stream)
            sim.set_comm_stream(self.streams[1].cuda_stream)
        sim.lib.pion_gpu_get_stream.argtypes = [C.c_void_p, C.c_int]
        sim.lib.pion_gpu_get_stream.restype = C.c_void_p
        self.cs = sim.lib.pion_gpu_get_stream(sim.h, 1) or sim.lib.pion_gpu_get_stream(sim.h, 0)

    def start(self, sim, which):
        assert self.pending is None
        sim.halo_begin()          # the rows to send are complete on the communication stream from here
        self.pending = which

    def finish(self, sim):
        if self.pending is None:
            return
        which, self.pending = self.pending, None
        sp = sim.halo_spans(which)
        nb = sp["count_per_var"] * 8
        for v in range(sp["nvar"]):
            o = v * sp["var_stride"] * 8
            # my top rows -> my YN ghosts, my bottom rows -> my YP ghosts (3 = hipMemcpyDeviceToDevice)
            assert self.hip.hipMemcpyAsync(sp["recv_lo"] + o, sp["send_hi"] + o, nb, 3, self.cs) == 0
            assert self.hip.hipMemcpyAsync(sp["recv_hi"] + o, sp["send_lo"] + o, nb, 3, self.cs) == 0
        sim.halo_end()

    def allreduce_min(self, a, b):
        return a, b


_TABLES = {}


def _tables(cfg):
    key = (cfg.min_temp, cfg.max_temp)
    if key not in _TABLES:
        _TABLES[key] = cooling.build_tables(*key)
    return _TABLES[key]


def _periodic_y(cfg):
    cfg.bc_type[2] = cfg.bc_type[3] = abi.BC_PERIODIC
    return cfg


def _case(case, ny, strict):
    """(cfg, P, needs cooling tables): 70 x ny, periodic in y"""
    if case in ("glm_hlld", "glm_hlld_oa1"):
        cfg, _ = problems.mhd_blastwave(4, 2, abi.EQGLM, abi.FLUX_RS_HLLD, strict_fp=strict)
        cfg.ng[0], cfg.ng[1] = NX, ny
        cfg.dx = 1.0 / NX
        # keep the hot disc (radius 7 cells) on the grid: centred where the grid is thinner than the disc; ny = 37: its
        # lower edge on the YN face, so that its rim crosses the flag rows of both strips (of the upper one through the
        # periodic wrap) and of the interior part (check_hll_switch)
        cfg.xmin[1] = -min(0.5 * ny, 6.5) / NX
        if case == "glm_hlld_oa1":
            cfg.sp_ooa = cfg.tm_ooa = 1                # first order in space (and time), nbc stays 2
        P = problems.fill_mhd_blastwave(cfg)
        # a velocity across the y faces, so that the halo rows matter from the first step
        x, y, _ = problems.cell_centres(cfg)
        P[abi.VY] = 0.3 * np.cos(2 * np.pi * x)[None, None, :] + 0.1
        P[abi.VX] = 0.2 * np.sin(2 * np.pi * y * NX / ny)[None, :, None]
        return cfg, P, False
    if case in ("hd_roe", "hd_hll"):
        solver = abi.FLUX_RSroe if case == "hd_roe" else abi.FLUX_RS_HLL
        cfg, P = problems.hd_blast_box([NX, ny], solver=solver, strict_fp=strict)
        return _periodic_y(cfg), P, False
    if case == "hd_fvs_cool_tr":
        L = 3.160064e18
        cfg = abi.make_config(2, [NX, ny], abi.EQEUL, abi.FLUX_FVS, ntracer=1, artvisc=abi.AV_FKJ98_1D, etav=0.15,
                              gamma=1.6666666666666667, cfl=0.3, dx=L / NX, xmin=(0.0, 0.0, 0.0),
                              bcs=["reflecting", "one-way-outflow", "periodic", "periodic"],
                              refvec=[1.0e-24, 1.0e-13, 1.0e6, 1.0e6, 1.0e6, 1.0], min_temp=5.0e3, max_temp=1.0e8,
                              cooling=abi.COOL_WSS09_CIE_LINE_HEAT_COOL, mp_timestep_limit=1, strict_fp=strict)
        P = problems.alloc(cfg)
        X, Y, _ = problems.mesh(cfg)
        inside = X * X + Y * Y < (0.3 * L) ** 2
        mu_over_kb = 0.609 * 1.672621898e-24 / 1.38064852e-16
        P[abi.RO] = np.where(inside, 20.0, 1.0) * 2.124229813e-24
        P[abi.PG] = P[abi.RO] * np.where(inside, 2.0e6, 7.5e3) / mu_over_kb
        P[abi.VY] = 2.0e6 * (1.0 + 0.5 * np.sin(2 * np.pi * X / L))
        P[5] = np.where(inside, 1.0, 0.0)
        return cfg, P, True
    raise KeyError(case)


def _run(cfg, P, tables, comm_mode, nsteps=3):
    nb = cfg.nbc
    with lib.GpuSim(cfg, 0) as g:
        if tables:
            g.set_cooling_tables(*_tables(cfg))
        comm = None if comm_mode is None else SelfComm2D(g, comm_mode == "streams")
        _raw(g, 1)                               # (the address of Ph, before the first step)
        sc = driver.SimControl(g, cfg, comm=comm)
        sc.init(P)
        out = []
        for _ in range(nsteps):
            dt = sc.calculate_timestep()
            sc.advance_time()
            g.synchronize()
            # (Ph as stored: after a full step it still holds what the half step left)
            out.append((dt, g.download(0)[:, :, nb:-nb, nb:-nb].copy(), _raw(g, 1)[:, :, nb:-nb, nb:-nb].copy()))
        sc.finish_halo()
        g.synchronize()
        # the HLLD -> HLL switch the last stage's prepass left, [rows][nx_all] (HLLD cases)
        hll = g.get_hll_switch().reshape(abi.ng_all(cfg)[1], -1) if cfg.solver == abi.FLUX_RS_HLLD else None
        return out, hll


def _compare(case, ny, strict, mode):
    cfg, P, tables = _case(case, ny, strict)
    whole, hll_w = _run(cfg, P, tables, None)
    cfg_s = copy.deepcopy(cfg)
    cfg_s.bc_type[2] = cfg_s.bc_type[3] = abi.BC_SLAB
    split, hll_s = _run(cfg_s, P, tables, mode)
    for n, ((dtw, Pw, Phw), (dts, Ps, Phs)) in enumerate(zip(whole, split)):
        print("step %d dt %r %r  P differs in %d  Ph differs in %d values" % (n, dtw, dts, (Pw != Ps).sum(), (Phw != Phs).sum()))
        assert dtw == dts, (n, dtw, dts)
        assert np.array_equal(Pw, Ps), "step %d: %d values of P differ" % (n, (Pw != Ps).sum())
        assert np.array_equal(Phw, Phs), "step %d: %d values of Ph differ" % (n, (Phw != Phs).sum())
    assert np.isfinite(whole[-1][1]).all()
    if hll_w is not None:
        check_hll_switch(hll_w, hll_s, cfg.nbc)


CASES = ["glm_hlld", "hd_roe", "hd_fvs_cool_tr", "hd_hll", "glm_hlld_oa1"]


@pytest.mark.parametrize("strict", [1, 0], ids=["strict", "fast"])
@pytest.mark.parametrize("rows", [None, "4"], ids=["rows_auto", "rows4"])
@pytest.mark.parametrize("ny", [4, 5, 37])
@pytest.mark.parametrize("case", CASES)
def test_interior_plus_strips_equal_whole_stage_2d(case, ny, rows, strict, monkeypatch):
    if rows is None:
        monkeypatch.delenv("PION_ROWS", raising=False)
    else:
        monkeypatch.setenv("PION_ROWS", rows)
    _compare(case, ny, strict, "streams")


@pytest.mark.parametrize("case", ["glm_hlld", "hd_fvs_cool_tr"])
def test_interior_plus_strips_on_one_stream_2d(case, monkeypatch):
    """without a communication stream the halo copies and the strips follow the interior on the compute stream"""
    monkeypatch.delenv("PION_ROWS", raising=False)
    _compare(case, 37, 1, "one_stream")


@pytest.mark.parametrize("case", ["hd_roe", "glm_hlld"])
@pytest.mark.parametrize("ny", [4, 5, 37])
def test_interior_part_updates_the_interior_rows_only(case, ny, monkeypatch):
    """PION_STAGE_INTERIOR alone writes the rows [nbc, ny - nbc) of the destination array and no others (none at all for
    ny = 4 = 2 nbc, where no split is possible); PION_STAGE_SLABBOUNDARY then writes exactly the remaining rows"""
    monkeypatch.delenv("PION_ROWS", raising=False)
    cfg, P, _ = _case(case, ny, 1)
    cfg.bc_type[2] = cfg.bc_type[3] = abi.BC_SLAB
    nb = cfg.nbc
    with lib.GpuSim(cfg, 0) as g:
        sc = driver.SimControl(g, cfg)
        sc.init(P)
        dt = sc.calculate_timestep()
        _raw(g, 1, put=np.full_like(P, -7.0))   # Ph := a value no update produces (densities, pressures are positive)

        def written():
            A = _raw(g, 1)[:, 0, nb:-nb, nb:-nb]
            return sorted(set(np.nonzero((A != -7.0).any(axis=(0, 2)))[0].tolist()))

        g.stage_part(0.5 * dt, 1, 0, abi.STAGE_INTERIOR)
        interior = list(range(nb, ny - nb)) if ny > 2 * nb else []
        assert written() == interior
        g.stage_part(0.5 * dt, 1, 0, abi.STAGE_SLABBOUNDARY)
        assert written() == list(range(ny))


def test_halo_spans_of_a_2d_grid():
    """pion_gpu_halo_spans describes the nbc rows next to each y face: nbc * nx_all doubles per variable, x ghosts
    included, contiguous in the [nvar][ny_all][nx_all] array"""
    cfg, P, _ = _case("glm_hlld", 5, 1)
    cfg.bc_type[2] = cfg.bc_type[3] = abi.BC_SLAB
    nb, nxa, nya = cfg.nbc, NX + 2 * cfg.nbc, 5 + 2 * cfg.nbc
    with lib.GpuSim(cfg, 0) as g:
        assert g.halo_count() == cfg.nvar * nb * nxa
        for which in (0, 1):
            sp = g.halo_spans(which)
            assert sp["count_per_var"] == nb * nxa
            assert sp["var_stride"] == nxa * nya and sp["nvar"] == cfg.nvar
            base = sp["recv_lo"]
            assert sp["send_lo"] - base == 8 * nb * nxa
            assert sp["send_hi"] - base == 8 * 5 * nxa
            assert sp["recv_hi"] - base == 8 * (5 + nb) * nxa
        # pack / unpack take the y faces of a 2-D grid, and no others
        import torch
        buf = torch.zeros(g.halo_count(), dtype=torch.float64, device="cuda:0")
        g.upload(P)
        g.pack_halo(0, 3, buf.data_ptr())
        g.synchronize()
        want = P[:, 0, 5:5 + nb, :]          # the last nbc on-grid rows: all-cell rows ny .. ny + nbc - 1
        assert np.array_equal(buf.cpu().numpy().reshape(cfg.nvar, nb, nxa), want)
        with pytest.raises(lib.PionGpuError):
            g.pack_halo(0, 4, buf.data_ptr())
        with pytest.raises(lib.PionGpuError):
            g.pack_halo(0, 1, buf.data_ptr())


def test_slab_faces_elsewhere_are_rejected():
    """PION_BC_SLAB is legal on the two faces of the slab axis only: an x face of a 2-D grid, a y face of a 3-D grid and
    any face of a 1-D grid are EINVAL at create"""
    cfg, _, _ = _case("glm_hlld", 5, 1)
    for face in (0, 1):
        c = copy.deepcopy(cfg)
        c.bc_type[face] = abi.BC_SLAB
        with pytest.raises(lib.PionGpuError) as e:
            lib.GpuSim(c, 0)
        assert e.value.rc == abi.E_INVAL
    c3, _ = problems.mhd_blastwave(8, 3, abi.EQGLM, abi.FLUX_RS_HLLD, strict_fp=1)
    c3.bc_type[2] = abi.BC_SLAB
    with pytest.raises(lib.PionGpuError):
        lib.GpuSim(c3, 0)
    c1 = abi.make_config(1, [16], abi.EQEUL, abi.FLUX_RSroe, xmin=(0.0, 0, 0), xmax=(1.0, 0, 0), bcs=["outflow", "slab"],
                         refvec=[1.0] * 5)
    with pytest.raises(lib.PionGpuError):
        lib.GpuSim(c1, 0)
    # a cylindrical slab away from the axis: SLAB at YN, no axis
    cc, _ = problems.blast_axi2d(12, abi.EQEUL, abi.FLUX_RSroe, strict_fp=1)
    cc.bc_type[2] = abi.BC_SLAB
    cc.xmin[1] = 6 * cc.dx
    with lib.GpuSim(cc, 0) as g:
        assert g.halo_count() == cc.nvar * cc.nbc * (12 + 2 * cc.nbc)
