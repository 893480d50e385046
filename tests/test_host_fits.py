"""FITS snapshots of the C++ host loop (pion_host_sim_write_fits, pion_amd/host/fits_io.h) on the CPU: the loop runs
over the oracle's backend table, which has no fits_* entries, so the files are written by the fallback route -- array
0 downloaded whole, the images evaluated by dev_output.h's functions in a host loop.  (tests/test_gpu_fits.py: the
same functions in the kernels of pion_output.hip, and the streamed files.)

Expected values come from the numpy restatement in tests/fits_restate.py, each expression with its reference line;
every comparison of values is == on the 8 bytes.  Files are parsed by fits_restate.parse, a few lines of numpy that
share nothing with pion_amd/fits.py; that reader is checked against it."""
import glob
import os
import struct

import numpy as np
import pytest

import fits_restate as fr
from pion_amd import abi, cooling, fits, host_rccl, problems, slab, snapshot
from test_host_snapshot import orc_loop, run_steps

nosetup = lambda sim, c: None


def tables(sim, c):
    if c.cooling:
        sim.set_cooling_tables(*cooling.build_tables(c.min_temp, c.max_temp))


def value_case(name):
    if name == "glm3d":
        return problems.mhd_blast_generic([10, 6, 5], strict_fp=1)
    if name == "cyl_glm_axis":
        return problems.blast_axi2d(16, abi.EQGLM, abi.FLUX_RS_HLLD, ntracer=1, strict_fp=1)
    if name == "mhd2d":
        return problems.mhd_blast_generic([12, 10], eqntype=abi.EQMHD, strict_fp=1)
    if name == "euler1d":
        return problems.hd_blast_box([24], strict_fp=1)
    if name == "sph1d":
        return problems.blast_sph1d(32, strict_fp=1)
    raise KeyError(name)


def list_case(name):
    """a configuration and a positive state (nothing is stepped)"""
    kw = dict(strict_fp=1, dx=0.125)
    cool = dict(cooling=8, min_temp=5.0e3, max_temp=1.0e8)
    ng = [6, 4, 3]
    if name == "euler":
        cfg = abi.make_config(3, ng, abi.EQEUL, abi.FLUX_RSroe, **kw)
    elif name == "euler_tr":
        cfg = abi.make_config(3, ng, abi.EQEUL, abi.FLUX_RSroe, ntracer=1, **kw)
    elif name == "euler_cool":
        cfg = abi.make_config(3, ng, abi.EQEUL, abi.FLUX_RSroe, **cool, **kw)
    elif name == "mhd":
        cfg = abi.make_config(3, ng, abi.EQMHD, abi.FLUX_RS_HLLD, **kw)
    elif name == "glm":
        cfg = abi.make_config(3, ng, abi.EQGLM, abi.FLUX_RS_HLLD, **kw)
    elif name == "glm_tr_cool":
        cfg = abi.make_config(3, ng, abi.EQGLM, abi.FLUX_RS_HLLD, ntracer=1, **cool, **kw)
    elif name == "six_tracers":
        cfg = abi.make_config(3, ng, abi.EQEUL, abi.FLUX_RSroe, ntracer=6, **kw)
    else:
        raise KeyError(name)
    P = np.random.default_rng(11).uniform(0.5, 1.5, size=problems.alloc(cfg).shape)
    return cfg, P


LISTS = {
    "euler": ["GasDens", "GasPres", "GasVX", "GasVY", "GasVZ", "Eint"],
    "euler_tr": ["GasDens", "GasPres", "GasVX", "GasVY", "GasVZ", "TR0", "Eint"],
    "euler_cool": ["GasDens", "GasPres", "GasVX", "GasVY", "GasVZ", "Temp"],
    "mhd": ["GasDens", "GasPres", "GasVX", "GasVY", "GasVZ", "Bx", "By", "Bz", "Eint", "divB", "Ptot"],
    "glm": ["GasDens", "GasPres", "GasVX", "GasVY", "GasVZ", "Bx", "By", "Bz", "psi", "Eint", "divB", "Ptot"],
    "glm_tr_cool": ["GasDens", "GasPres", "GasVX", "GasVY", "GasVZ", "Bx", "By", "Bz", "psi", "TR0", "Temp", "divB",
                    "Ptot"],
}


@pytest.fixture(scope="module")
def written(tmp_path_factory):
    """per value case: (cfg, path of the FITS file, path of the PIONRAW2 file, download(0)) two steps in"""
    made = {}
    d = tmp_path_factory.mktemp("fits")

    def get(name):
        if name not in made:
            cfg, P = value_case(name)
            f, r = str(d / (name + ".fits")), str(d / (name + ".pionraw"))
            with orc_loop(cfg, nosetup) as s:
                s.init(P)
                s.set_output(str(d / ("o'" + name + "_a_base_name_long_enough_to_need_a_second_card" * 2)), op_criterion=1, opfreq_time=0.37, checkpoint_freq=7)
                run_steps(s, 2)
                s.write_fits(f)
                s.write_snapshot(r)
                made[name] = (cfg, f, r, s.download(0))
        return made[name]
    return get


def test_structure_of_the_file(written):
    cfg, path, _, _ = written("glm3d")
    hdus = fr.parse(path)   # length, printable cards, END, blank and zero padding
    assert len(hdus) == 1 + 12
    fixed = lambda key, val: "%-8s= %20s" % (key, val) + " " * 50
    primary = hdus[0][0]
    assert primary[:4] == [fixed("SIMPLE", "T"), fixed("BITPIX", -64), fixed("NAXIS", 0), fixed("EXTEND", "T")]
    assert all(c.startswith("HIERARCH ") or c.startswith("CONTINUE  '") for c in primary[4:-1])
    assert hdus[0][1].size == 0
    for (cards, data), name in zip(hdus[1:], fr.image_names(cfg)):
        want = ["XTENSION= 'IMAGE   '" + " " * 60, fixed("BITPIX", -64), fixed("NAXIS", 3), fixed("NAXIS1", 10),
                fixed("NAXIS2", 6), fixed("NAXIS3", 5), fixed("PCOUNT", 0), fixed("GCOUNT", 1),
                ("EXTNAME = '%-8s'" % name).ljust(80), "END".ljust(80)]
        assert cards == want, name
        assert data.size == 10 * 6 * 5
    assert os.path.getsize(path) == len(primary_blocks(primary)) + 12 * (2880 + 2880)   # 2400 bytes of data + 480 of zeros


def primary_blocks(cards):
    n = len(cards) * 80
    return b" " * ((n + 2879) // 2880 * 2880)


@pytest.mark.parametrize("name", sorted(LISTS))
def test_image_list(name, tmp_path):
    cfg, P = list_case(name)
    path = str(tmp_path / "l.fits")
    with orc_loop(cfg, tables) as s:
        s.init(P)
        s.write_fits(path)
        A = s.download(0)
    got = fr.images_of(path)
    assert list(got) == LISTS[name] == fr.image_names(cfg)
    for (n, img) in fr.restate(cfg, A):
        assert fr.same_bits(got[n], fr.squeeze(img, cfg)), n


def test_six_tracers_are_refused_with_a_text(tmp_path):
    cfg, P = list_case("six_tracers")
    with orc_loop(cfg, nosetup) as s:
        s.init(P)
        assert s.lib.pion_host_sim_write_fits(s.s, os.fsencode(str(tmp_path / "x.fits"))) == abi.E_INVAL
        assert "5 tracers" in s.last_error()
        with pytest.raises(RuntimeError, match="5 tracers"):
            s.write_fits(str(tmp_path / "x.fits"))
    assert os.listdir(tmp_path) == []


@pytest.mark.parametrize("name", ["glm3d", "cyl_glm_axis", "mhd2d", "euler1d", "sph1d"])
def test_values_after_two_steps(name, written):
    cfg, path, _, A = written(name)
    got = fr.images_of(path)
    want = fr.restate(cfg, A)
    assert list(got) == [n for n, _ in want]
    nb = cfg.nbc
    og = {3: A[:, nb:-nb, nb:-nb, nb:-nb], 2: A[:, 0, nb:-nb, nb:-nb], 1: A[:, 0, 0, nb:-nb]}[cfg.ndim]
    for v, (n, img) in enumerate(want):
        assert fr.same_bits(got[n], fr.squeeze(img, cfg)), n
        if v < cfg.nvar:   # the primitive images against the slice of download(0) itself
            scale = np.sqrt(4 * np.pi) if n in ("Bx", "By", "Bz") else 1.0
            assert fr.same_bits(got[n], og[v] * scale) if scale != 1.0 else fr.same_bits(got[n], og[v]), n
    if "divB" in got:
        assert np.abs(got["divB"]).max() > 0.0
    # pion_amd.fits reads the same file to the same arrays
    params, images = fits.read(path)
    assert list(images) == list(got)
    for n in got:
        assert fr.same_bits(images[n], got[n]), n


REAL_KEYS = {"Gamma", "CFL", "eta_visc", "EP_Min_Temperature", "EP_Max_Temperature", "t_start", "t_finish", "t_sim",
             "min_timestep", "last_dt", "opfreq_time", "pion_dx", "pion_next_optime"}


def _bits(x):
    return struct.pack("<d", float(x))


@pytest.mark.parametrize("name", ["cyl_glm_axis", "glm3d"])
def test_header_round_trip(name, written):
    """every parameter parses to the bits the PIONRAW2 header of the same moment gives"""
    cfg, fpath, rpath, _ = written(name)
    _, _, hd = snapshot.read(rpath)
    ccfg, info = host_rccl.read_snapshot_header(rpath)
    params, _ = fits.read(fpath)
    # the cards themselves, without pion_amd.fits: name and raw value text
    raw = {}
    for c in fr.parse(fpath)[0][0][4:-1]:
        if c.startswith("HIERARCH "):
            k, _, v = c[9:].partition("=")
            raw[k.strip()] = v.strip()
    arrays = {"NGrid": 3, "Xmin": 3, "Xmax": 3, "Ref_Vector": cfg.nvar}
    strings = ("outfile", "BC_XN", "BC_XP", "BC_YN", "BC_YP", "BC_ZN", "BC_ZP")
    keys = [k for k in hd if k != "pion_data_offset"]
    assert "pion_data_offset" not in params and "pion_data_offset" not in raw
    assert sorted(params) == sorted(keys)
    for k in keys:
        if k in arrays:
            want = hd[k].split()
            assert len(want) == arrays[k] == len(params[k])
            for i, w in enumerate(want):
                assert _bits(float(raw["%s%d" % (k, i)])) == _bits(float(w)) == _bits(params[k][i]), (k, i)
        elif k in strings:
            assert params[k] == hd[k], k
        else:
            assert _bits(float(raw[k])) == _bits(float(hd[k])) == _bits(params[k]), k
            assert isinstance(params[k], float) == (k in REAL_KEYS), k   # (a real keeps its decimal point: "0.")
    # ... and to what pion_host_snapshot_read_header returns
    for k, f in (("t_sim", "t_sim"), ("last_dt", "last_dt"), ("t_start", "t_start"), ("t_finish", "t_finish"),
                 ("pion_next_optime", "next_optime"), ("opfreq_time", "opfreq_time"), ("min_timestep", "min_timestep")):
        assert _bits(params[k]) == _bits(info[f]), k
    assert (params["t_step"], params["pion_slab_lo"], params["pion_slab_n"]) == (2, 0, info["slab_n"])
    assert _bits(params["Gamma"]) == _bits(ccfg.gamma) and _bits(params["pion_dx"]) == _bits(ccfg.dx)
    assert params["outfile"] == info["outfile"] and "'" in params["outfile"]   # (a quote and a CONTINUE'd string)
    assert len(params["outfile"]) > 100 and sum(c.startswith("CONTINUE") for c in fr.parse(fpath)[0][0]) >= 1


def _run_with_outputs(cfg, P, base, filetype, nsteps):
    with orc_loop(cfg, nosetup) as s:
        s.init(P)
        s.set_output(base, op_criterion=0, opfreq=3, checkpoint_freq=2)
        if filetype is not None:
            s.set_output_filetype(filetype)
        out = []
        for _ in range(nsteps):
            k, t, ldt = s.time_int(1)
            out.append((s.get_time()["timestep"], t, ldt))
        state = s.download(0)
    return out, state


def test_cadence_fits_outputs_pionraw_checkpoints(tmp_path):
    cfg, P = value_case("euler1d")
    a, b = tmp_path / "a", tmp_path / "b"
    a.mkdir(), b.mkdir()
    raw_steps, raw_state = _run_with_outputs(cfg, P, str(a / "r"), None, 7)
    fits_steps, fits_state = _run_with_outputs(cfg, P, str(b / "r"), host_rccl.FILE_FITS, 7)
    assert fits_steps == raw_steps and np.array_equal(fits_state, raw_state)
    assert sorted(os.listdir(a)) == ["r_0000.%08d.pionraw" % k for k in (0, 3, 6)] + \
        ["r_0000.99999998.pionraw", "r_0000.99999999.pionraw"]
    assert sorted(os.listdir(b)) == ["r_0000.%08d.fits" % k for k in (0, 3, 6)] + \
        ["r_0000.99999998.pionraw", "r_0000.99999999.pionraw"]
    for k in (0, 3, 6):
        p, _ = fits.read(str(b / ("r_0000.%08d.fits" % k)))
        _, info = host_rccl.read_snapshot_header(str(a / ("r_0000.%08d.pionraw" % k)))
        assert p["t_step"] == k == info["t_step"] and _bits(p["t_sim"]) == _bits(info["t_sim"])
    # back to the default
    _, _ = _run_with_outputs(cfg, P, str(tmp_path / "c"), host_rccl.FILE_PIONRAW, 1)
    assert glob.glob(str(tmp_path / "c_0000.*.fits")) == []


def _join(paths, axis):
    parts = [fr.images_of(p) for p in paths]
    return {n: np.concatenate([q[n] for q in parts], axis=0) for n in parts[0]}


def test_two_ranks_3d_joined_images_equal_the_single_domain(tmp_path):
    """two ranks cut along z over the shared-memory transport, two steps: the seam's divB reads exchanged ghost planes"""
    name = "glm3d_z12"
    cfg, P = fr.two_rank_case(name)
    single = str(tmp_path / "single.fits")
    with orc_loop(cfg, nosetup) as s:
        s.init(P)
        steps = run_steps(s, 2)
        s.write_fits(single)
    paths = [str(tmp_path / ("r%d.fits" % r)) for r in range(2)]
    times = fr.run_two_ranks(name, "orc", 2, paths)
    assert times[0]["simtime"] == times[1]["simtime"] == steps[-1][1]
    want, got = fr.images_of(single), _join(paths, 0)
    assert list(got) == list(want)
    for n in want:
        assert fr.same_bits(got[n], want[n]), n
    for r, p in enumerate(paths):
        params, _ = fits.read(p)
        assert params["NGrid"] == [20, 12, 12] and (params["pion_slab_lo"], params["pion_slab_n"]) == (6 * r, 6)
        assert (params["pion_rank"], params["pion_world"]) == (r, 2)


def test_two_slabs_2d_joined_images_equal_the_single_domain(tmp_path):
    """2-D Cartesian GLM-MHD cut along y.  The oracle's table has no 2-D halo, so the slabs do not step here
    (tests/test_gpu_fits.py runs the two ranks): each slab is a sim of its own initialised with its rows of the
    single domain's step-2 state, ghost rows from the neighbouring slab included, as an exchange leaves them.  The
    seam's divB is the single domain's only if the stencil reads those rows."""
    cfg, P = fr.two_rank_case("glm2d_y12")
    single = str(tmp_path / "single.fits")
    with orc_loop(cfg, nosetup) as s:
        s.init(P)
        steps = run_steps(s, 2)
        s.write_fits(single)
        mid = s.download(0)
    paths = []
    for r in range(2):
        c = slab.slab_config(cfg, r, 2)
        with orc_loop(c, nosetup) as s:
            s.set_slab_extent(cfg.ng[1], r * c.ng[1], cfg.bc_type[2], cfg.bc_type[3])
            s.init(slab.slab_slice(mid, cfg, r, 2), simtime=steps[1][1], timestep=2, last_dt=steps[1][0])
            paths.append(str(tmp_path / ("y%d.fits" % r)))
            s.write_fits(paths[-1])
    want, got = fr.images_of(single), _join(paths, 0)
    for n in want:
        assert fr.same_bits(got[n], want[n]), n
    assert np.abs(want["divB"]).max() > 0.0


def test_bad_arguments_return_a_code_and_a_text(tmp_path):
    cfg, P = value_case("euler1d")
    with orc_loop(cfg, nosetup) as s:
        s.init(P)
        bad = os.fsencode(str(tmp_path / "no_such_dir" / "x.fits"))
        assert s.lib.pion_host_sim_write_fits(s.s, bad) == abi.E_INVAL
        assert "cannot create" in s.last_error()
        assert s.lib.pion_host_sim_write_fits(s.s, None) == abi.E_INVAL
        for t in (2, -1, 99):
            assert s.lib.pion_host_sim_set_output_filetype(s.s, t) == abi.E_INVAL
            assert "unknown file type" in s.last_error()
            with pytest.raises(ValueError, match="unknown file type"):
                s.set_output_filetype(t)
        # the sim lives on
        s.write_fits(str(tmp_path / "ok.fits"))
    assert sorted(os.listdir(tmp_path)) == ["ok.fits"]
