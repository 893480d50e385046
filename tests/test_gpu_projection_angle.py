"""The inclined projection of a cylindrical (z,R) grid on the GPU: k_angle_values and k_project_angle of
pion_project.hip (pion_gpu_project_angle) against the host route -- the same rule, pion_amd/csrc/dev_project_angle.h, in
the host loop of libpion_host.so, which tests/test_host_projection_angle.py pins bit for bit to a scalar restatement.

Nothing of the walk is evaluated differently on the device: sqrt and the divisions are IEEE, nothing is contracted, tan
and 1 / sin come from the host.  So both builds are compared with the host route with == on the 8 bytes wherever the
fields have no T^b.  Shapes: 70 x 37 at 41 degrees has NI = 154, three wavefronts per impact row with the last one
partial, and NR = 37 rows over 4-wavefront workgroups; a grid that starts 3 dx off the axis; 5 x 2, the smallest grid
the rule admits; 66 x 5 GLM (nvar 9) at atan(1/2), where rays graze cell corners.  The states have NaN in every ghost
cell and see no boundary update: only on-grid cells are read.

A T^b field differs through the device's log and exp: the per-cell bound of projection_restate.field_value carried
through the sum by the restatement (tests/angle_projection_restate.py)."""
import ctypes as C
import os

import numpy as np
import pytest

import fits_restate as fr
import projection_restate as pr
from pion_amd import abi, cooling, fits, host_rccl, lib, problems
from test_host_projection_angle import GRIDS, config, fields_of, restated, state
from test_host_snapshot import run_steps

pytestmark = pytest.mark.gpu

CASES = [("70x37", 41.0, "euler"), ("17x9_off_axis", 35.0, "euler"), ("5x2", 40.0, "euler"), ("66x5", 26.565051177, "glm")]


def device_images(cfg_of, deg, fields, P):
    """{strict: [nfields][NR][NI]} from a handle of each build; guard words behind the buffer stay untouched, and the
    status call reports no capped pixel"""
    import torch
    got = {}
    for strict in (1, 0):
        cfg = cfg_of(strict)
        with lib.GpuSim(cfg, 0) as g:
            g.upload(P)   # NaN ghost cells, no boundary update
            n, n_extra = g.project_angle_count(deg, len(fields))
            ni = cfg.ng[0] + 2 * n_extra
            assert n == len(fields) * cfg.ng[1] * ni
            buf = torch.full((n + 8,), -7.0, dtype=torch.float64, device="cuda:0")
            g.project_angle(deg, fields, dbuf_ptr=buf.data_ptr())
            assert g.project_angle_status() == 0
            raw = buf.cpu().numpy()
            assert (raw[n:] == -7.0).all(), "wrote past the buffer"
            got[strict] = raw[:n].reshape(len(fields), cfg.ng[1], ni).copy()
            # a second call on the same handle (the scratch of the first is reused), through the other wrapper
            assert fr.same_bits(g.project_angle(deg, fields[:1])[0], got[strict][0])
    return got


def _strictness(cfg, strict):
    c = type(cfg).from_buffer_copy(cfg)
    c.strict_fp = strict
    return c


@pytest.mark.parametrize("grid,deg,eqn", CASES)
def test_both_builds_equal_the_host_route(grid, deg, eqn):
    cfg = config(grid, eqn)
    fields, P = fields_of(cfg), state(cfg)
    info = {}
    want = lib.project_angle_on_host(cfg, deg, fields, P, info=info)
    assert info["ncapped"] == 0 and np.isfinite(want).all() and want.max() > 0.0
    got = device_images(lambda strict: _strictness(cfg, strict), deg, fields, P)
    for k, f in enumerate(fields):
        assert fr.same_bits(got[1][k], want[k]), (grid, deg, f[0], "strict build", np.abs(got[1][k] - want[k]).max())
        assert fr.same_bits(got[0][k], want[k]), (grid, deg, f[0], "fast build", np.abs(got[0][k] - want[k]).max())


def _tables(sim, cfg):
    sim.set_cooling_tables(*cooling.build_tables(cfg.min_temp, cfg.max_temp))


def test_a_power_of_T_stays_within_the_bound_of_the_field():
    """rho^2 T^-0.9, and rho beside it (b == 0: the same bits)"""
    grid, deg = "17x9_off_axis", 35.0
    cfg = config(grid, cool=True)
    fields, P = [pr.HALPHA, ("coldens", 1, -1, 1.0, 0.0)], state(cfg)
    want = restated(cfg, grid, deg, fields, P)
    w, allowed = np.array(want["img"][0]), np.array(want["allowed"][0])
    host = lib.project_angle_on_host(cfg, deg, fields, P)
    import torch
    for strict in (1, 0):
        c = _strictness(cfg, strict)
        with lib.GpuSim(c, 0) as g:
            _tables(g, c)
            g.upload(P)
            got = g.project_angle(deg, fields)
        some = allowed > 0
        for tag, ref in (("restatement", w), ("host route", host[0])):
            dev = np.abs(got[0] - ref)
            print("strict" if strict else "fast", "halpha: largest |device - %s| / bound = %.3g" % (tag, (dev[some] / allowed[some]).max()))
            assert (dev <= allowed).all(), (strict, tag)
        assert fr.same_bits(got[1], host[1])


class _Table(C.Structure):
    """pion_backend (pion_amd/host/pion_backend.h): the name and 36 function pointers, the last two project_angle_*"""
    _fields_ = [("f%d" % i, C.c_void_p) for i in range(37)]


def _table_without_angle_entries():
    h = host_rccl.load_host_library()
    h.pion_backend_gpu.restype = C.c_void_p
    t = _Table.from_buffer_copy(C.string_at(h.pion_backend_gpu(), C.sizeof(_Table)))
    assert all(getattr(t, "f%d" % i) for i in range(37))
    t.f35 = t.f36 = None
    return t


def test_the_file_of_the_device_route_is_the_host_routes(tmp_path):
    grid, deg = "70x37", 41.0
    cfg = config(grid)
    fields, P = fields_of(cfg), pr.rough_state(cfg)
    table = _table_without_angle_entries()
    for tag, backend in (("dev", None), ("host", C.addressof(table))):
        with host_rccl.HostSim(cfg, 0, backend=backend) as s:
            s.init(P)
            s.write_projection_angle(str(tmp_path / (tag + ".fits")), deg, fields)
            A = s.download(0)
    assert open(tmp_path / "dev.fits", "rb").read() == open(tmp_path / "host.fits", "rb").read()
    params, images = fits.read(str(tmp_path / "dev.fits"))
    want = lib.project_angle_on_host(cfg, deg, fields, A)
    assert params["pion_proj_n_extra"] == 42 and params["pion_proj_angle"] == 41.0
    for k, f in enumerate(fields):
        assert images[f[0]].shape == (37, 154) and fr.same_bits(images[f[0]], want[k])


def _wind_run(tmp_path, angle, perp):
    cfg, P, srcs = problems.wind2d_axi(32, ny=16, strict_fp=1)
    d = tmp_path / "run"      # every run under the same name: the headers carry it
    d.mkdir()
    fields = [("coldens", 1, -1, 1.0, 0.0), ("windcol", 1, 5, 1.0, 0.0), pr.HALPHA]
    with host_rccl.HostSim(cfg, 0) as s:
        _tables(lib.GpuSim(cfg, 0, borrowed_handle=s.gpu_handle()), cfg)
        for src in srcs:
            s.add_wind_source(src)
        s.init(P)
        s.set_output(str(d / "w"), op_criterion=0, opfreq=1, checkpoint_freq=100)
        if angle:
            s.set_projection_angle_output(41.0, fields)
        if perp:
            s.set_projection_output(abi.PROJ_AXIS_PERP, fields)
        steps = run_steps(s, 3)
        out = cfg, steps, s.download(0), s.download(1)
    files = {n: open(d / n, "rb").read() for n in sorted(os.listdir(d))}
    os.rename(d, tmp_path / ("kept_%d%d" % (angle, perp)))
    return out, files


def test_wind2d_run_with_inclined_images_at_every_output(tmp_path):
    """problems.wind2d_axi at 32 x 16, 3 steps: a file per output; P, Ph and every dt == the run without; the
    perpendicular file is byte for byte what it is without the inclined output"""
    (cfg, steps0, P0, Ph0), plain = _wind_run(tmp_path, False, True)
    (_, steps, P, Ph), both = _wind_run(tmp_path, True, True)
    assert steps == steps0 and np.array_equal(P, P0) and np.array_equal(Ph, Ph0)
    at = range(4)
    assert [n for n in both if "_proja_" in n] == ["w_proja_0000.%08d.fits" % k for k in at]
    assert not [n for n in plain if "_proja_" in n]
    for k in at:
        assert both["w_proj_0000.%08d.fits" % k] == plain["w_proj_0000.%08d.fits" % k]
        params, images = fits.read(str(tmp_path / "kept_11" / ("w_proja_0000.%08d.fits" % k)))
        assert params["t_step"] == k and list(images) == ["coldens", "windcol", "halpha"]
        ni = 32 + 2 * params["pion_proj_n_extra"]
        assert all(im.shape == (16, ni) and np.isfinite(im).all() for im in images.values())
        assert (images["coldens"] >= 0).all() and images["coldens"].max() > 0
    # the last file: the last state (b == 0: the bits of the host route)
    want = lib.project_angle_on_host(cfg, 41.0, [("coldens", 1, -1, 1.0, 0.0), ("windcol", 1, 5, 1.0, 0.0)], P)
    assert fr.same_bits(images["coldens"], want[0]) and fr.same_bits(images["windcol"], want[1])


def test_refusals_on_the_device_handle():
    cyl = config("5x2")
    one = [("x", 1)]
    with lib.GpuSim(cyl, 0) as g:
        g.upload(pr.rough_state(cyl))
        for deg, fields, text in ((float("nan"), one, "finite, above 0 and below 90"), (0.0, one, "finite, above 0 and below 90"),
                                  (-3.0, one, "finite, above 0 and below 90"), (135.0, one, "finite, above 0 and below 90"),
                                  (90.0, one, "PION_PROJ_AXIS_PERP"), (1.0e-7, one, "exceeds 2\\^31 - 1"),
                                  (40.0, [("x", 3)], "power of rho"), (40.0, [("x", 1, 6)], "not a variable"),
                                  (40.0, [("x", 2, -1, 1.0, -0.9)], "cooling == 0"), (40.0, [], "between 1 and 8")):
            with pytest.raises(lib.PionGpuError, match=text):
                g.project_angle(deg, fields)
        with pytest.raises(lib.PionGpuError, match="no buffer"):
            g.project_angle(40.0, one, dbuf_ptr=0)
        with pytest.raises(lib.PionGpuError, match="which is 0"):
            g.project_angle(40.0, one, which=2)
        with pytest.raises(lib.PionGpuError, match="PION_PROJ_AXIS_PERP"):
            g.project_angle_count(90.0, 1)
        assert g.project_angle_status() == 0
        assert g.project_angle(40.0, one).shape == (1, 2, 9)   # the handle lives on
    for make, text in ((lambda: pr.case("euler_tr_70x9x6"), "only a 2-D cylindrical"),
                       (lambda: abi.make_config(2, [12, 10], abi.EQEUL, abi.FLUX_RSroe, dx=0.125), "only a 2-D cylindrical"),
                       (lambda: abi.make_config(2, [5, 1], abi.EQEUL, abi.FLUX_RSroe, ntracer=1, coord_sys=2, bcs=pr.CYL_BCS,
                                                dx=0.125), "NR == 1"),
                       (lambda: abi.make_config(2, [5, 4], abi.EQEUL, abi.FLUX_RSroe, ntracer=1, coord_sys=2, dx=0.125,
                                                bcs=["outflow", "outflow", "axisymmetric", "slab"]), "PION_BC_SLAB")):
        with lib.GpuSim(make(), 0) as g:
            with pytest.raises(lib.PionGpuError, match=text):
                g.project_angle_count(40.0, 1)
            with pytest.raises(lib.PionGpuError, match=text):
                g.project_angle(40.0, one)
