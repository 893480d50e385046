"""Projected images of the C++ host loop (pion_host_sim_write_projection, pion_host_sim_set_projection_output) on the
CPU: the loop runs over the oracle's backend table, which has no project_* entries, so the images are made by the
fallback route -- array 0 downloaded whole, every pixel by dev_project.h's functions in a host loop.
(tests/test_gpu_projection.py: the same functions in the kernels of pion_project.hip.)

Expected values come from the numpy restatement in tests/projection_restate.py.  The column sums of a 3-D grid are
compared with == on the 8 bytes.  The Abel images differ from numpy only through log (glibc here, numpy's own there,
each within an ulp): per pixel |host - restatement| <= 4 eps * 2 sum_ir (|s| x2dx + |offset| |xdx|), the sum taken from
the restatement."""
import os

import numpy as np
import pytest

import fits_restate as fr
import projection_restate as pr
from pion_amd import abi, fits, problems
from test_host_snapshot import orc_loop, run_steps

nosetup = lambda sim, c: None


def _images(s, path, axis, fields):
    s.write_projection(path, axis, fields)
    return fits.read(path)


@pytest.mark.parametrize("name", ["euler_tr_70x9x6", "glm_tr_66x5x4"])
@pytest.mark.parametrize("axis", [0, 1, 2])
def test_column_sums_equal_the_restatement(name, axis, tmp_path):
    cfg = pr.case(name)
    fields = pr.fields_of(cfg)
    with orc_loop(cfg, nosetup) as s:
        s.init(pr.rough_state(cfg))
        A = s.download(0)
        params, images = _images(s, str(tmp_path / "p.fits"), axis, fields)
    want = pr.project(cfg, A, fields, axis)
    assert list(images) == [f[0] for f in fields]
    ng = cfg.ng
    shape = {0: (ng[2], ng[1]), 1: (ng[2], ng[0]), 2: (ng[1], ng[0])}[axis]
    for n, img, allowed in want:
        assert images[n].shape == shape and not allowed.any()
        assert fr.same_bits(images[n], img), (name, axis, n)
    # the simplest column, against a sum written out here: [j][i] has i on the lower-numbered axis
    nb = cfg.nbc
    og = A[0, nb:-nb, nb:-nb, nb:-nb]
    if axis == 2:
        col = 0.0
        for k in range(ng[2]):
            col = col + og[k, 3, 5]
        assert images["coldens"][3, 5] == col * cfg.dx
    assert params["pion_proj_axis"] == axis


@pytest.mark.parametrize("name", ["cyl_70x37", "cyl_70x37_off_axis", "cyl_5x2", "cyl_70x37_dx0p1"])
def test_abel_images_within_the_gate(name, tmp_path):
    cfg = pr.case(name)
    fields = pr.fields_of(cfg)
    with orc_loop(cfg, nosetup) as s:
        s.init(pr.rough_state(cfg))
        A = s.download(0)
        _, images = _images(s, str(tmp_path / "p.fits"), abi.PROJ_AXIS_PERP, fields)
    worst = 0.0
    for n, img, gate in pr.project(cfg, A, fields, abi.PROJ_AXIS_PERP):
        assert images[n].shape == (cfg.ng[1], cfg.ng[0]) and np.isfinite(images[n]).all() and (gate > 0).all()
        dev = np.abs(images[n] - img)
        worst = max(worst, (dev / gate).max())
        print(name, n, "largest deviation / gate = %.3g" % (dev / gate).max())
        assert (dev <= gate).all(), (name, n, (dev / gate).max())
        assert np.abs(img).max() > 0.0
    assert worst <= 1.0


def test_abel_of_a_uniform_field_is_the_chord_through_the_grid(tmp_path):
    """not a restatement: v = 1 everywhere has slope 0, and the integral from the first segment's Rmin = b to
    grid_max is 2 sqrt(grid_max^2 - b^2)"""
    cfg = pr.case("cyl_70x37")
    P = problems.alloc(cfg)
    P[:] = 1.0
    with orc_loop(cfg, nosetup) as s:
        s.init(P)
        _, images = _images(s, str(tmp_path / "u.fits"), abi.PROJ_AXIS_PERP, [("one", 0, -1, 1.0, 0.0)])
    r = cfg.xmin[1] + (np.arange(cfg.ng[1]) + 0.5) * cfg.dx
    chord = 2.0 * np.sqrt((r[-1] + 0.5 * cfg.dx) ** 2 - r ** 2)
    assert np.allclose(images["one"], chord[:, None] * np.ones(cfg.ng[0]), rtol=1e-13, atol=0)


def test_file_layout_and_header(tmp_path):
    cfg = pr.case("cyl_5x2")
    fields = pr.fields_of(cfg)[:2] + [("p_scaled", 0, abi.PG, 0.1, 0.0)]
    path, snap = str(tmp_path / "p.fits"), str(tmp_path / "s.fits")
    with orc_loop(cfg, nosetup) as s:
        s.init(pr.rough_state(cfg))
        s.write_projection(path, abi.PROJ_AXIS_PERP, fields)
        s.write_fits(snap)
    assert sorted(os.listdir(tmp_path)) == ["p.fits", "s.fits"]     # (the .part name is gone)
    hdus = fr.parse(path)   # block structure, printable cards, END, zero padding
    assert len(hdus) == 1 + 3 and hdus[0][1].size == 0
    fixed = lambda key, val: ("%-8s= %20s" % (key, val)).ljust(80)
    for (cards, data), f in zip(hdus[1:], fields):
        assert cards == ["XTENSION= 'IMAGE   '".ljust(80), fixed("BITPIX", -64), fixed("NAXIS", 2), fixed("NAXIS1", 5),
                         fixed("NAXIS2", 2), fixed("PCOUNT", 0), fixed("GCOUNT", 1),
                         ("EXTNAME = '%-8s'" % f[0]).ljust(80), "END".ljust(80)]
        assert data.size == 10
    params, images = fits.read(path)
    sparams, _ = fits.read(snap)
    extra = {"pion_proj_axis": abi.PROJ_AXIS_PERP}
    for i, (n, a, var, coef, b) in enumerate(fields):
        extra.update({"pion_proj_%d_a" % i: a, "pion_proj_%d_var" % i: var, "pion_proj_%d_coef" % i: coef,
                      "pion_proj_%d_b" % i: b})
    assert {k: params[k] for k in extra} == extra and isinstance(params["pion_proj_2_coef"], float)
    assert {k: v for k, v in params.items() if k not in extra} == sparams   # the snapshot's primary header, unchanged
    assert list(params)[:len(sparams)] == list(sparams)
    # big-endian on disk
    raw = open(path, "rb").read()
    first = images["coldens"].reshape(-1)[0]
    assert raw.count(np.array([first], dtype=">f8").tobytes()) >= 1


def _run(cfg, P, base, project, nsteps=6):
    with orc_loop(cfg, nosetup) as s:
        s.init(P)
        s.set_output(base, op_criterion=0, opfreq=2, checkpoint_freq=100)
        if project:
            s.set_projection_output(abi.PROJ_AXIS_PERP, pr.fields_of(cfg)[:2])
        steps = run_steps(s, nsteps)
        return steps, s.download(0), s.download(1)


def test_cadence_and_untouched_time_steps(tmp_path):
    cfg, P = problems.blast_axi2d(16, strict_fp=1)
    a, b = tmp_path / "a", tmp_path / "b"
    a.mkdir(), b.mkdir()
    plain = _run(cfg, P, str(a / "r"), False)
    with_proj = _run(cfg, P, str(b / "r"), True)
    assert with_proj[0] == plain[0]                                  # every dt and time, ==
    assert np.array_equal(with_proj[1], plain[1]) and np.array_equal(with_proj[2], plain[2])
    assert sorted(os.listdir(a)) == ["r_0000.%08d.pionraw" % k for k in (0, 2, 4, 6)]
    assert sorted(os.listdir(b)) == ["r_0000.%08d.pionraw" % k for k in (0, 2, 4, 6)] + \
        ["r_proj_0000.%08d.fits" % k for k in (0, 2, 4, 6)]
    for k in (0, 2, 4, 6):
        params, images = fits.read(str(b / ("r_proj_0000.%08d.fits" % k)))
        assert params["t_step"] == k and list(images) == ["coldens", "emmeasure"]
        assert images["coldens"].shape == (cfg.ng[1], cfg.ng[0])
    # the last file holds the projection of the last state
    want = pr.project(cfg, with_proj[1], pr.fields_of(cfg)[:2], abi.PROJ_AXIS_PERP)
    for n, img, gate in want:
        assert (np.abs(images[n] - img) <= gate).all(), n


REFUSED = [
    # (configuration, axis, fields, text)
    (lambda: abi.make_config(1, [24], abi.EQEUL, abi.FLUX_RSroe, dx=0.125), 0, None, "1-D grids"),
    (lambda: abi.make_config(1, [24], abi.EQEUL, abi.FLUX_RSroe, dx=0.125, coord_sys=3, bcs=["reflecting", "outflow"]),
     0, None, "spherical"),
    (lambda: abi.make_config(2, [12, 10], abi.EQEUL, abi.FLUX_RSroe, dx=0.125), 1, None, "2-D Cartesian"),
    (lambda: pr.case("cyl_5x2"), 0, None, "along the symmetry axis"),
    (lambda: pr.case("cyl_5x2"), 1, None, "PION_PROJ_AXIS_PERP only"),
    (lambda: pr.case("euler_tr_70x9x6"), abi.PROJ_AXIS_PERP, None, "axis 0, 1 or 2"),
    (lambda: pr.case("euler_tr_70x9x6"), -1, None, "axis 0, 1 or 2"),
    (lambda: pr.case("euler_tr_70x9x6"), 0, [], "between 1 and 8 fields"),
    (lambda: pr.case("euler_tr_70x9x6"), 0, [("f%d" % i, 1) for i in range(9)], "between 1 and 8 fields"),
    (lambda: pr.case("euler_tr_70x9x6"), 0, [("x", 3)], "power of rho"),
    (lambda: pr.case("euler_tr_70x9x6"), 0, [("x", -1)], "power of rho"),
    (lambda: pr.case("euler_tr_70x9x6"), 0, [("x", 1, 6)], "not a variable of the state"),
    (lambda: pr.case("euler_tr_70x9x6"), 0, [("", 1)], "1 to 15 characters"),
    (lambda: pr.case("euler_tr_70x9x6"), 0, [("a_name_16_bytes_", 1)], "1 to 15 characters"),
    (lambda: pr.case("euler_tr_70x9x6"), 0, [("it's", 1)], "printable ASCII without quotes"),
    (lambda: pr.case("euler_tr_70x9x6"), 0, [("x", 1, -1, float("nan"), 0.0)], "finite"),
    (lambda: pr.case("euler_tr_70x9x6"), 0, [("x", 2, -1, 1.0, -0.9)], "cooling == 0"),
]


@pytest.mark.parametrize("k", range(len(REFUSED)))
def test_refusals_have_a_code_and_a_text(k, tmp_path):
    make, axis, fields, text = REFUSED[k]
    cfg = make()
    fields = pr.fields_of(cfg)[:1] if fields is None else fields
    path = str(tmp_path / "x.fits")
    with orc_loop(cfg, nosetup) as s:
        s.init(pr.rough_state(cfg))
        arr = abi.proj_fields(fields)
        assert s.lib.pion_host_sim_write_projection(s.s, os.fsencode(path), axis, len(fields), arr) == abi.E_INVAL
        assert text in s.last_error()
        assert s.lib.pion_host_sim_set_projection_output(s.s, axis, len(fields), arr) == (0 if fields == [] else abi.E_INVAL)
        with pytest.raises(RuntimeError, match=text):
            s.write_projection(path, axis, fields)
        s.download(0)   # the sim lives on
    assert os.listdir(tmp_path) == []


def test_one_row_in_R_is_refused():
    one = abi.make_config(2, [5, 1], abi.EQEUL, abi.FLUX_RSroe, ntracer=1, coord_sys=2, bcs=pr.CYL_BCS, dx=0.125)
    with orc_loop(one, nosetup) as s:
        s.init(pr.rough_state(one))
        arr = abi.proj_fields(pr.fields_of(one)[:1])
        assert s.lib.pion_host_sim_write_projection(s.s, b"/dev/null/x", abi.PROJ_AXIS_PERP, 1, arr) == abi.E_INVAL
        assert "NR == 1" in s.last_error()


def test_slab_extent_and_bad_paths_are_refused(tmp_path):
    cfg = pr.case("cyl_5x2")
    fields = pr.fields_of(cfg)[:1]
    with orc_loop(cfg, nosetup) as s:
        s.init(pr.rough_state(cfg))
        arr = abi.proj_fields(fields)
        bad = os.fsencode(str(tmp_path / "no_such_dir" / "x.fits"))
        assert s.lib.pion_host_sim_write_projection(s.s, bad, abi.PROJ_AXIS_PERP, 1, arr) == abi.E_INVAL
        assert "cannot create" in s.last_error()
        assert s.lib.pion_host_sim_write_projection(s.s, None, abi.PROJ_AXIS_PERP, 1, arr) == abi.E_INVAL
        s.set_slab_extent(4, 0, cfg.bc_type[2], cfg.bc_type[3])
        assert s.lib.pion_host_sim_write_projection(s.s, bad, abi.PROJ_AXIS_PERP, 1, arr) == abi.E_INVAL
        assert "one rank of a slab run" in s.last_error()
        with pytest.raises(ValueError, match="one rank of a slab run"):
            s.set_projection_output(abi.PROJ_AXIS_PERP, fields)
        s.write_fits(str(tmp_path / "ok.fits"))   # the sim lives on
    assert sorted(os.listdir(tmp_path)) == ["ok.fits"]
