"""Ray-traced column densities of the C++ host loop (pion_host_sim_add_rt_source, pion_host_sim_set_column_output,
pion_host_sim_write_columns) on the CPU: the loop runs over the oracle's backend table, which has no ray-tracing entries,
so the sim keeps the sources itself and the writer downloads array 0 and runs pion_gpu_raytrace_host on it.
(tests/test_gpu_host_columns.py: the same files traced on the device and streamed.)

Expected images come from the scalar restatement of the reference's tracer in tests/raytrace_restate.py, applied to the
state the regular output of the same step holds; everything is compared with ==."""
import os

import numpy as np
import pytest

import raytrace_restate as rs
from pion_amd import abi, fits, host_rccl, problems
from test_host_snapshot import orc_loop, run_steps

nosetup = lambda sim, c: None


def column_cases(strict_fp=1):
    """name -> (cfg, P, sources): a 3-D Euler box with a tracer and a cylindrical (z,R) blast with one"""
    cfg3, P3 = problems.hd_blast_box([12, 10, 8], ntracer=1, strict_fp=strict_fp)
    nb = cfg3.nbc
    P3[5] = 0.25
    P3[5, nb + 2:nb + 6, nb + 3:nb + 7, nb + 1:nb + 9] = 0.75
    dx = cfg3.dx
    src3 = [{"pos": (4.0 * dx, 3.3 * dx, 2.0 * dx), "opacity": abi.RT_OPACITY_TOTAL},
            {"pos": (-2.0 * dx, 5.0 * dx, 9.5 * dx), "opacity": abi.RT_OPACITY_MINUS},
            {"at_infinity": 1, "dir": 1, "opacity": abi.RT_OPACITY_TRACER}]
    cfg2, P2 = problems.blast_axi2d(16, ntracer=1, strict_fp=strict_fp)
    P2[5] = 0.5
    d2 = cfg2.dx
    src2 = [{"pos": (cfg2.xmin[0] + 5.0 * d2, 0.0), "opacity": abi.RT_OPACITY_TRACER},
            {"at_infinity": 1, "dir": 3}]
    return {"box3d": (cfg3, P3, src3), "axi2d": (cfg2, P2, src2)}


def restated(cfg, state, src):
    """(col, dcol) of the restatement for the on-grid state {name: image} of a regular FITS output"""
    ng = [cfg.ng[a] for a in range(cfg.ndim)]
    shape = (cfg.ng[2], cfg.ng[1], cfg.ng[0])
    rho = state["GasDens"].reshape(shape)
    y = state["TR0"].reshape(shape)
    xmin = [cfg.xmin[a] for a in range(3)]
    col, dcol, moved = rs.trace(ng, cfg.ndim, xmin, cfg.dx, src, rho, y)
    return col, dcol, moved


def run(loop, cfg, P, base, sources, nsteps=6, **kw):
    """a run of nsteps with FITS outputs every 2 steps; sources: the columns file beside each"""
    with loop(cfg, nosetup, **kw) as s:
        used = [s.add_rt_source(src) for src in sources]
        s.init(P)
        s.set_output(base, op_criterion=0, opfreq=2, checkpoint_freq=100)
        s.set_output_filetype(host_rccl.FILE_FITS)
        if sources:
            s.set_column_output(True)
        steps = run_steps(s, nsteps)
        return steps, s.download(0), used


def check_run(loop, name, tmp_path, **kw):
    cfg, P, sources = column_cases()[name]
    base = str(tmp_path / "r")
    plain = run(loop, cfg, P, base, [], **kw)
    regular = ["r_0000.%08d.fits" % k for k in (0, 2, 4, 6)]
    assert sorted(os.listdir(tmp_path)) == regular                          # no sources: no new file
    before = {f: open(str(tmp_path / f), "rb").read() for f in regular}
    for f in regular:
        os.unlink(str(tmp_path / f))
    traced = run(loop, cfg, P, base, sources, **kw)
    cols = ["r_cols_0000.%08d.fits" % k for k in (0, 2, 4, 6)]
    assert sorted(os.listdir(tmp_path)) == sorted(regular + cols)           # one columns file per regular output
    assert traced[0] == plain[0] and np.array_equal(traced[1], plain[1])    # every dt and the state: read-only
    for f in regular:
        assert open(str(tmp_path / f), "rb").read() == before[f], f         # the regular outputs, byte for byte
    assert [u[0] for u in traced[2]] == list(range(len(sources)))
    shape = tuple(cfg.ng[a] for a in range(cfg.ndim))[::-1]
    for k, f, c in zip((0, 2, 4, 6), regular, cols):
        sparams, state = fits.read(str(tmp_path / f))
        params, images = fits.read(str(tmp_path / c))
        names = []
        for n in range(len(sources)):
            names += ["Col_Src_%d_T0" % n, "DCol_Src_%d_T0" % n]
        assert list(images) == names and params["t_step"] == k
        # the snapshot's primary header unchanged, then the sources under the reference's names
        extra = {key: v for key, v in params.items() if key not in sparams}
        assert {key: v for key, v in params.items() if key in sparams} == sparams
        want = {"RT_Nsources": len(sources)}
        for n, src in enumerate(sources):
            col, dcol, moved = restated(cfg, state, src)
            assert images["Col_Src_%d_T0" % n].shape == shape
            assert np.array_equal(images["Col_Src_%d_T0" % n], col.reshape(shape)), (k, n)
            assert np.array_equal(images["DCol_Src_%d_T0" % n], dcol.reshape(shape)), (k, n)
            assert col.max() > 0.0
            if src.get("at_infinity", 0):
                pos = [0.0, 0.0, 0.0]
                pos[src["dir"] // 2] = 1.0e200 if src["dir"] % 2 else -1.0e200
            else:
                pos = list(moved) + [0.0] * (3 - len(moved))
                assert list(traced[2][n][1]) == pos                         # the position reported back
            for d in range(3):
                want["RT_position_%d_%d" % (n, d)] = pos[d]
            want["RT_at_infty_%d" % n] = src.get("at_infinity", 0)
            want["RT_Opacity__%d" % n] = src.get("opacity", abi.RT_OPACITY_TOTAL)
            want["RT_Tau_var__%d" % n] = src.get("opacity_var", 0)
        assert extra == want
    return {c: open(str(tmp_path / c), "rb").read() for c in cols}


@pytest.mark.parametrize("name", ["box3d", "axi2d"])
def test_columns_beside_every_regular_output(name, tmp_path):
    check_run(orc_loop, name, tmp_path)


def test_write_columns_on_request_and_refusals(tmp_path):
    cfg, P, sources = column_cases()["box3d"]
    path = str(tmp_path / "c.fits")
    with orc_loop(cfg, nosetup) as s:
        s.init(P)
        with pytest.raises(RuntimeError, match="no radiation source"):
            s.write_columns(path)
        with pytest.raises(ValueError, match="no radiation source"):
            s.set_column_output(True)
        s.set_column_output(False)
        with pytest.raises(ValueError, match="microphysics"):
            s.add_rt_source({"opacity": 6})
        with pytest.raises(ValueError, match="opacity_var is not a tracer"):
            s.add_rt_source({"opacity": abi.RT_OPACITY_MINUS, "opacity_var": 3})
        for i in range(abi.MAX_RT_SOURCES):
            assert s.add_rt_source(sources[0])[0] == i
        with pytest.raises(ValueError, match="more than PION_MAX_RT_SOURCES"):
            s.add_rt_source(sources[0])
        with pytest.raises(RuntimeError, match="cannot create"):
            s.write_columns(str(tmp_path / "no_such_dir" / "c.fits"))
        s.write_columns(path)
        _, images = fits.read(path)
        assert len(images) == 2 * abi.MAX_RT_SOURCES
        assert np.array_equal(images["Col_Src_0_T0"], images["Col_Src_3_T0"])
    assert sorted(os.listdir(tmp_path)) == ["c.fits"]


def test_one_rank_of_several_is_refused(tmp_path):
    cfg, P, sources = column_cases()["box3d"]
    with orc_loop(cfg, nosetup) as s:
        s.init(P)
        s.add_rt_source(sources[0])
        s.set_slab_extent(16, 0, cfg.bc_type[4], cfg.bc_type[5])
        with pytest.raises(ValueError, match="one rank of a slab run"):
            s.add_rt_source(sources[1])
        with pytest.raises(ValueError, match="one rank of a slab run"):
            s.set_column_output(True)
        with pytest.raises(RuntimeError, match="one rank of a slab run"):
            s.write_columns(str(tmp_path / "c.fits"))
    assert os.listdir(tmp_path) == []
