"""Projected images on the GPU: the kernels of pion_project.hip (pion_gpu_project) against the numpy restatement of
tests/projection_restate.py, the fast build against the strict one, the device route of the C++ loop against its host
route (dev_project.h's functions in a host loop, the same library), a handle whose stages run in plane windows, and one
run of the loop with projections at every output.

Column sums (3-D, b == 0) are compared with == on the 8 bytes.  Shapes: Euler + 1 tracer 70 x 9 x 6 and GLM 66 x 5 x 4:
an x extent of 64 + a remainder is the smallest at which the lane partition of the x sum and the 64-pixel stretches of
the y / z sums can go wrong.  The states are seeded rough positive numbers uploaded with NaN in every ghost cell and no
boundary update: only on-grid cells are read.

Abel images (cylindrical, NZ x NR = 70 x 37 and 5 x 2; NR = 37 is no multiple of the kernel's 16 impact rows or its
blocks of 16 segment rows; a grid that starts at the axis and one that starts 3 dx off it; one dx that is no power of
two).  sqrt is correctly rounded and nothing is contracted, so the only operation that may differ from numpy is log:
<= 1 ulp from the device's library, < 1 ulp from the host's, <= 2 ulp between them, on the non-negative log term of
x2dx.  Gate per pixel: |device - restatement| <= 4 eps * 2 sum_ir (|s| x2dx + |offset| |xdx|), the sum from the
restatement -- the 2-ulp bound with a factor 2 of margin.  Device against the host route gets the same gate.

T^b fields (b = -0.9, a handle with cooling): exp and log are each within 1 ulp on the device; the error of b log T is
amplified by |b log T|.  projection_restate.field_value derives the bound per cell (rel = eps (3 |b log T| + 3)) and
column_sum / abel_image carry it to the pixel; nothing here is a constant that was picked.

Every test prints the largest deviation / gate it saw."""
import ctypes as C
import os

import numpy as np
import pytest

import fits_restate as fr
import projection_restate as pr
from pion_amd import abi, cooling, fits, host_rccl, lib, problems
from test_host_snapshot import run_steps

pytestmark = pytest.mark.gpu


def nan_ghosts(cfg, P):
    """P with NaN in every ghost cell"""
    A = np.full(P.shape, np.nan)
    nb = cfg.nbc
    sl = (slice(None),) + tuple(slice(nb, nb + cfg.ng[a]) if a < cfg.ndim else slice(None) for a in (2, 1, 0))
    A[sl] = P[sl]
    return A


def device_images(name, axis, fields, P):
    """{strict: [nfields][NJ][NI]} from a handle of each build; guard words behind the buffer stay untouched"""
    import torch
    got = {}
    for strict in (1, 0):
        cfg = pr.case(name, strict)
        with lib.GpuSim(cfg, 0) as g:
            g.upload(P)   # NaN ghost cells, no boundary update
            n = g.project_count(axis, len(fields))
            nj, ni = g.project_shape(axis)
            assert n == len(fields) * nj * ni
            buf = torch.full((n + 8,), -7.0, dtype=torch.float64, device="cuda:0")
            g.project(axis, fields, dbuf_ptr=buf.data_ptr())
            g.synchronize()
            raw = buf.cpu().numpy()
            assert (raw[n:] == -7.0).all(), "wrote past the buffer"
            got[strict] = raw[:n].reshape(len(fields), nj, ni).copy()
    return got


@pytest.mark.parametrize("name", ["euler_tr_70x9x6", "glm_tr_66x5x4"])
@pytest.mark.parametrize("axis", [0, 1, 2])
def test_column_sums_equal_the_restatement_in_both_builds(name, axis):
    cfg = pr.case(name)
    fields = pr.fields_of(cfg)
    P = nan_ghosts(cfg, pr.rough_state(cfg))
    got = device_images(name, axis, fields, P)
    for i, (n, img, allowed) in enumerate(pr.project(cfg, P, fields, axis)):
        assert np.isfinite(img).all() and not allowed.any()
        assert fr.same_bits(got[1][i], img), (name, axis, n, "strict build")
        assert fr.same_bits(got[0][i], img), (name, axis, n, "fast build")


class _Table(C.Structure):
    """pion_backend (pion_amd/host/pion_backend.h): the name and 26 function pointers"""
    _fields_ = [("f%d" % i, C.c_void_p) for i in range(27)]


def _table_without_projection_entries():
    h = host_rccl.load_host_library()
    h.pion_backend_gpu.restype = C.c_void_p
    t = _Table.from_buffer_copy(C.string_at(h.pion_backend_gpu(), C.sizeof(_Table)))
    assert t.f24 and t.f25 and t.f26
    t.f25 = t.f26 = None
    return t


def _both_routes(cfg, P, axis, fields, tmp_path, setup=None):
    """({name: image} device route, the same of the host route, download(0)) of the C++ loop on the GPU"""
    out = []
    table = _table_without_projection_entries()
    for tag, backend in (("dev", None), ("host", C.addressof(table))):
        with host_rccl.HostSim(cfg, 0, backend=backend) as s:
            if setup:
                setup(lib.GpuSim(cfg, 0, borrowed_handle=s.gpu_handle()), cfg)
            s.init(P)
            path = str(tmp_path / (tag + ".fits"))
            s.write_projection(path, axis, fields)
            out.append(fits.read(path)[1])
            A = s.download(0)
    return out[0], out[1], A


@pytest.mark.parametrize("name,axis", [("euler_tr_70x9x6", 0), ("euler_tr_70x9x6", 1), ("glm_tr_66x5x4", 2)])
def test_device_route_equals_host_route_3d(name, axis, tmp_path):
    cfg = pr.case(name, 0)   # the fast build
    fields = pr.fields_of(cfg)
    dev, host, A = _both_routes(cfg, pr.rough_state(cfg), axis, fields, tmp_path)
    assert open(str(tmp_path / "dev.fits"), "rb").read() == open(str(tmp_path / "host.fits"), "rb").read()
    for n, img, _ in pr.project(cfg, A, fields, axis):
        assert fr.same_bits(dev[n], img) and fr.same_bits(host[n], img), n


def test_x_projection_of_a_windowed_handle(monkeypatch):
    """a handle whose stages run in plane windows (tests/test_gpu_rows_windows.py's knob): the image reads the state
    array itself, whatever the windows"""
    name, axis = "euler_tr_70x9x6", 0
    cfg = pr.case(name)
    fields = pr.fields_of(cfg)
    P = nan_ghosts(cfg, pr.rough_state(cfg))
    monkeypatch.delenv("PION_ROWS_WINDOW_CELLS", raising=False)
    with lib.GpuSim(cfg, 0) as g:
        g.upload(P)
        assert g.rows_windows()["windows_whole_stage"] == 1
        whole = g.project(axis, fields)
    stride = (cfg.ng[0] + 2 * cfg.nbc) * (cfg.ng[1] + 2 * cfg.nbc)
    monkeypatch.setenv("PION_ROWS_WINDOW_CELLS", str((2 + 2 * cfg.nbc) * stride + 1))
    with lib.GpuSim(cfg, 0) as g:
        g.upload(P)
        assert g.rows_windows()["windows_whole_stage"] == 3
        windowed = g.project(axis, fields)
    assert fr.same_bits(windowed, whole)
    for i, (n, img, _) in enumerate(pr.project(cfg, P, fields, axis)):
        assert fr.same_bits(windowed[i], img), n


CYL = ["cyl_70x37", "cyl_70x37_off_axis", "cyl_5x2", "cyl_70x37_dx0p1"]


@pytest.mark.parametrize("name", CYL)
def test_abel_images_within_the_gate_in_both_builds(name):
    cfg = pr.case(name)
    fields = pr.fields_of(cfg)
    P = nan_ghosts(cfg, pr.rough_state(cfg))
    got = device_images(name, abi.PROJ_AXIS_PERP, fields, P)
    assert fr.same_bits(got[0], got[1])   # the builds give the same bits
    worst = 0.0
    for i, (n, img, gate) in enumerate(pr.project(cfg, P, fields, abi.PROJ_AXIS_PERP)):
        assert np.isfinite(got[1][i]).all() and (gate > 0).all()
        ratio = (np.abs(got[1][i] - img) / gate).max()
        worst = max(worst, ratio)
        print(name, n, "largest |device - restatement| / gate = %.3g" % ratio)
        assert ratio <= 1.0, (name, n, ratio)
    print(name, "worst = %.3g" % worst)


@pytest.mark.parametrize("name", ["cyl_70x37", "cyl_70x37_dx0p1"])
def test_abel_device_route_against_host_route(name, tmp_path):
    cfg = pr.case(name, 0)
    fields = pr.fields_of(cfg)
    dev, host, A = _both_routes(cfg, pr.rough_state(cfg), abi.PROJ_AXIS_PERP, fields, tmp_path)
    for n, img, gate in pr.project(cfg, A, fields, abi.PROJ_AXIS_PERP):
        ratio = (np.abs(dev[n] - host[n]) / gate).max()
        print(name, n, "largest |device - host route| / gate = %.3g" % ratio)
        assert ratio <= 1.0, (name, n, ratio)
        assert (np.abs(host[n] - img) <= gate).all(), n


def _tables(sim, cfg):
    sim.set_cooling_tables(*cooling.build_tables(cfg.min_temp, cfg.max_temp))


@pytest.mark.parametrize("name,axes", [("euler_tr_cool_70x9x6", (0, 2)), ("cyl_cool_70x37", (abi.PROJ_AXIS_PERP,))])
def test_power_law_emissivity_within_the_derived_bound(name, axes, tmp_path):
    """rho^2 T^-0.9, and rho beside it (b == 0: its 3-D image keeps the same bits)"""
    cfg = pr.case(name)
    fields = [pr.HALPHA, pr.fields_of(cfg)[0]]
    P = nan_ghosts(cfg, pr.rough_state(cfg))
    for axis in axes:
        got = device_images(name, axis, fields, P)
        want = pr.project(cfg, P, fields, axis)
        for strict in (1, 0):
            assert np.isfinite(got[strict]).all()
            ratio = (np.abs(got[strict][0] - want[0][1]) / want[0][2]).max()
            print(name, axis, "strict" if strict else "fast", "halpha: largest deviation / bound = %.3g" % ratio)
            assert (want[0][2] > 0).all() and ratio <= 1.0, (name, axis, strict, ratio)
            if cfg.coord_sys != 2:
                assert fr.same_bits(got[strict][1], want[1][1])
        assert fr.same_bits(got[0], got[1])
    # ... and the host route of the same library
    dev, host, A = _both_routes(cfg, pr.rough_state(cfg), axes[-1], fields, tmp_path, setup=_tables)
    bound = pr.project(cfg, A, fields, axes[-1])[0][2]
    ratio = (np.abs(dev["halpha"] - host["halpha"]) / bound).max()
    print(name, "halpha: largest |device - host route| / bound = %.3g" % ratio)
    assert ratio <= 1.0


def test_refusals_on_the_device_handle():
    cfg = pr.case("euler_tr_70x9x6")
    with lib.GpuSim(cfg, 0) as g:
        g.upload(pr.rough_state(cfg))
        for axis, fields, text in ((3, [("x", 1)], "axis 0, 1 or 2"), (0, [("x", 3)], "power of rho"),
                                   (0, [("x", 2, -1, 1.0, -0.9)], "cooling == 0"), (0, [], "between 1 and 8")):
            with pytest.raises(lib.PionGpuError, match=text):
                g.project(axis, fields)
        with pytest.raises(lib.PionGpuError, match="no buffer"):
            g.project(0, [("x", 1)], dbuf_ptr=0)
        assert g.project(0, [("x", 1)]).shape == (1, 6, 9)   # the handle lives on
    cyl = pr.case("cyl_5x2")
    with lib.GpuSim(cyl, 0) as g:
        with pytest.raises(lib.PionGpuError, match="along the symmetry axis"):
            g.project_count(0, 1)


def _wind_run(tmp_path, tag, project):
    cfg, P, srcs = problems.wind2d_axi(32, ny=16, strict_fp=1)
    base = str(tmp_path / tag)
    with host_rccl.HostSim(cfg, 0) as s:
        _tables(lib.GpuSim(cfg, 0, borrowed_handle=s.gpu_handle()), cfg)
        for src in srcs:
            s.add_wind_source(src)
        s.init(P)
        s.set_output(base, op_criterion=0, opfreq=1, checkpoint_freq=100)
        if project:
            s.set_projection_output(abi.PROJ_AXIS_PERP, project)
        steps = run_steps(s, 4)
        return cfg, steps, s.download(0), s.download(1)


def test_wind2d_run_with_projections_at_every_output(tmp_path):
    """problems.wind2d_axi at 32 x 16, 4 steps: a file per output, and P, Ph and every dt == the run without"""
    tr0 = 5
    fields = [("coldens", 1, -1, 1.0, 0.0), ("windcol", 1, tr0, 1.0, 0.0), pr.HALPHA]
    cfg, steps, P, Ph = _wind_run(tmp_path, "w", fields)
    _, steps0, P0, Ph0 = _wind_run(tmp_path, "plain", None)
    assert steps == steps0 and np.array_equal(P, P0) and np.array_equal(Ph, Ph0)
    names = sorted(os.listdir(tmp_path))
    assert [n for n in names if n.startswith("w_proj")] == ["w_proj_0000.%08d.fits" % k for k in range(5)]
    assert not [n for n in names if n.startswith("plain_proj")]
    for k in range(5):
        params, images = fits.read(str(tmp_path / ("w_proj_0000.%08d.fits" % k)))
        assert params["t_step"] == k and list(images) == [f[0] for f in fields]
        assert all(im.shape == (16, 32) and np.isfinite(im).all() for im in images.values())
        assert (images["coldens"] > 0).all() and (images["halpha"] > 0).all() and (images["windcol"] >= 0).all()
    for n, img, gate in pr.project(cfg, P, fields, abi.PROJ_AXIS_PERP):   # the last file: the last state
        assert (np.abs(images[n] - img) <= gate).all(), n
