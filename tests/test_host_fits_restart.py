"""Restart of the C++ host loop from FITS files (pion_host_sim_read_fits, pion_amd/host/fits_io.h) on the CPU: the loop
runs over the oracle's backend table, which has no fits_from_host entry, so the images are read whole, converted by
dev_output.h's read rules in a host loop and uploaded.  (tests/test_gpu_fits_restart.py: the same rules in
k_unpack_fits, and the streamed read.)

Expected states come from tests/fits_read_restate.py -- the numpy restatement of the reference's reader applied to
the same file -- handed to a fresh sim through init + set_time.  Every comparison is == on the 8 bytes.  B is written
times sqrt(4 pi) and read times 1/sqrt(4 pi), so a restart from FITS need not continue the run that wrote the file bit
for bit where there is a magnetic field; for the Euler cases it must."""
import os
import shutil

import pytest

import fits_read_restate as rr
import fits_restate as fr
from pion_amd import abi, host_rccl, slab
from test_host_snapshot import assemble, case, ongrid, orc_loop, run_ranks, run_steps

# 1-D spherical, 2-D Cartesian, 2-D cylindrical (GLM, a tracer), 3-D Euler with tracer and cooling, 3-D GLM
GEOMETRIES = ["sph1d", "cart2d", "axi2d", "wind3d", "glm3d"]
EULER = ("sph1d", "cart2d", "wind3d")
K, M = 2, 3


def same(a, b):
    return fr.same_bits(a, b)


def from_restatement(cfg, setup, paths, nmore):
    """a fresh sim initialised from the restatement of the files and stepped: (P, Ph, [(dt, simtime)])"""
    og, nbad, missing, par = rr.restate_files(cfg, paths)
    assert nbad == 0 and not missing
    with orc_loop(cfg, setup) as s:
        s.init(rr.embed(cfg, og), simtime=par["t_sim"], timestep=par["t_step"], last_dt=par["last_dt"])
        steps = run_steps(s, nmore)
        return s.download(0), s.download(1), steps


@pytest.fixture(scope="module")
def glm_files(tmp_path_factory):
    """glm3d_z12 one step in: the FITS file, its PIONRAW2 twin, the state, and a later file"""
    d = tmp_path_factory.mktemp("fitsrestart")
    cfg, P, setup = case("glm3d_z12")
    with orc_loop(cfg, setup) as s:
        s.init(P)
        s.set_output(str(d / ("o'" + "a_base_name_long_enough_to_need_a_second_card" * 2)), op_criterion=1,
                     opfreq_time=0.37, checkpoint_freq=7)
        run_steps(s, 1)
        s.write_fits(str(d / "good.fits"))
        s.write_snapshot(str(d / "good.pionraw"))
        run_steps(s, 1)
        s.write_fits(str(d / "later.fits"))
    with orc_loop(cfg, setup) as s:
        s.restart(str(d / "good.fits"))
        state = s.download(0)
    return dict(dir=d, cfg=cfg, P=P, setup=setup, fits=str(d / "good.fits"), raw=str(d / "good.pionraw"),
                later=str(d / "later.fits"), state=state)


def test_header_equals_the_pionraw_header_of_the_same_moment(glm_files):
    fcfg, finfo = host_rccl.read_fits_header(glm_files["fits"])
    rcfg, rinfo = host_rccl.read_snapshot_header(glm_files["raw"])
    for f, _ in abi.PionGpuConfig._fields_:
        a, b = getattr(fcfg, f), getattr(rcfg, f)
        assert (list(a) == list(b)) if hasattr(a, "__len__") else (a == b), f
    assert finfo.pop("data_offset") == 0 and rinfo.pop("data_offset") > 0
    assert finfo == rinfo
    assert finfo["outfile"].startswith(str(glm_files["dir"] / "o'a_base")) and finfo["opfreq_time"] == 0.37
    with pytest.raises(ValueError, match="not a FITS file"):
        host_rccl.read_fits_header(glm_files["raw"])


@pytest.mark.parametrize("name", GEOMETRIES)
def test_restart_equals_a_sim_initialised_from_the_restatement(name, tmp_path):
    cfg, P, setup = case(name)
    path = str(tmp_path / (name + ".fits"))
    with orc_loop(cfg, setup) as s:
        s.init(P, first_step_dt_limit=orc_loop.last_dt_limit())
        first = run_steps(s, K)
        s.write_fits(path)
        written = s.download(0)
        rest = run_steps(s, M)
        uninterrupted = (s.download(0), s.download(1), rest)
    with orc_loop(cfg, setup) as s:
        assert s.restart(path) == ""
        t = s.get_time()
        assert t["timestep"] == K and t["simtime"] == first[-1][1] and t["last_dt"] == first[-1][0]
        read = s.download(0)
        steps = run_steps(s, M)
        got = (s.download(0), s.download(1), steps)
    want = from_restatement(cfg, setup, [path], M)
    assert got[2] == want[2], "dt / simtime sequence"
    assert same(got[0], want[0]) and same(got[1], want[1])
    mhd = cfg.eqntype in (abi.EQMHD, abi.EQGLM)
    for v in range(cfg.nvar):   # what was read: every variable but B has the bits that were written
        if not rr.is_b(cfg, v):
            assert same(ongrid(read, cfg)[v], ongrid(written, cfg)[v]), v
    if name in EULER:
        assert not mhd
        assert got[2] == uninterrupted[2]
        assert same(got[0], uninterrupted[0]) and same(got[1], uninterrupted[1])


def test_two_ranks_write_one_and_three_ranks_restart(tmp_path):
    name = "glm3d_z12"
    cfg, P, setup = case(name)
    paths = [str(tmp_path / ("w2_%d.fits" % r)) for r in range(2)]
    fr.run_two_ranks(name, "orc", 2, paths)
    infos = [host_rccl.read_fits_header(p)[1] for p in paths]
    assert [(i["rank"], i["world"], i["slab_lo"], i["slab_n"]) for i in infos] == [(0, 2, 0, 6), (1, 2, 6, 6)]
    want = from_restatement(cfg, setup, paths, 3)
    with orc_loop(cfg, setup) as s:
        s.restart(paths[::-1])
        assert run_steps(s, 3) == want[2]
        assert same(s.download(0), want[0]) and same(s.download(1), want[1])
    res3 = run_ranks(3, name, "restart", paths, 3)
    for r in range(3):
        assert res3[r][0]["simtime"] == want[2][-1][1] and res3[r][0]["timestep"] == 5
    assert same(assemble(res3, cfg, 3), ongrid(want[0], cfg))


def test_two_y_slabs_written_one_domain_restarts_2d(tmp_path):
    """2-D Cartesian Euler cut along y: each slab a sim of its own holding its rows of the step-2 state (the oracle's
    table has no 2-D halo); the single domain restarts from both files and continues the uninterrupted run"""
    cfg, P, setup = case("cart2d")
    with orc_loop(cfg, setup) as s:
        s.init(P)
        steps = run_steps(s, 2)
        mid = s.download(0)
        steps += run_steps(s, 3)
        ref = s.download(0)
    paths = []
    for r in range(2):
        c = slab.slab_config(cfg, r, 2)
        with orc_loop(c, setup) as s:
            s.set_slab_extent(cfg.ng[1], r * c.ng[1], cfg.bc_type[2], cfg.bc_type[3])
            s.init(slab.slab_slice(mid, cfg, r, 2), simtime=steps[1][1], timestep=2, last_dt=steps[1][0])
            paths.append(str(tmp_path / ("y%d.fits" % r)))
            s.write_fits(paths[-1])
    with orc_loop(cfg, setup) as s:
        s.restart(paths)
        assert run_steps(s, 3) == steps[2:]
        assert same(s.download(0), ref)


def test_images_are_found_by_name_not_by_position(glm_files, tmp_path):
    """image HDUs in reverse order, a foreign HDU (a binary table with a heap) between them, cards the reader does not
    know in the primary header"""
    hdus = rr.split_hdus(open(glm_files["fits"], "rb").read())
    primary = hdus[0][0].replace(b"END".ljust(80), b"COMMENT a card of somebody else's".ljust(80) +
                                 b"HIERARCH somebody_elses = 42".ljust(80) + b"END".ljust(80), 1)
    primary = primary.rstrip(b" ").ljust((len(primary.rstrip(b" ")) + 2879) // 2880 * 2880)
    images = hdus[1:][::-1]
    shuffled = str(tmp_path / "shuffled.fits")
    open(shuffled, "wb").write(rr.join_hdus([(primary, b"")] + images[:4] + [rr.foreign_hdu()] + images[4:]))
    assert [rr.extname(h) for h, _ in rr.split_hdus(open(shuffled, "rb").read())[1:4]] == ["Ptot", "divB", "Eint"]
    with orc_loop(glm_files["cfg"], glm_files["setup"]) as s:
        assert s.restart(shuffled) == ""
        assert same(s.download(0), glm_files["state"])


def test_missing_image_is_zeros_and_a_message(tmp_path):
    cfg, P, setup = case("axi2d")
    path, cut = str(tmp_path / "whole.fits"), str(tmp_path / "no_tr0.fits")
    with orc_loop(cfg, setup) as s:
        s.init(P)
        run_steps(s, 1)
        s.write_fits(path)
    hdus = rr.split_hdus(open(path, "rb").read())
    assert "TR0" in [rr.extname(h) for h, _ in hdus]
    open(cut, "wb").write(rr.join_hdus([x for x in hdus if rr.extname(x[0]) != "TR0"]))
    with orc_loop(cfg, setup) as s:
        s.restart(path)
        whole = ongrid(s.download(0), cfg)
    with orc_loop(cfg, setup) as s:
        note = s.restart(cut)
        assert "TR0" in note and "zero" in note
        got = ongrid(s.download(0), cfg)
    tr0 = cfg.nvar - 1
    assert whole[tr0].any() and not got[tr0].any()
    assert same(got[:tr0], whole[:tr0])
    og, nbad, missing, _ = rr.restate_files(cfg, [cut])
    assert missing == ["TR0"] and nbad == 0 and same(got, og)


def test_bad_files_return_an_error_and_a_text(glm_files, tmp_path):
    cfg, P, setup, good = glm_files["cfg"], glm_files["P"], glm_files["setup"], glm_files["fits"]
    raw = open(good, "rb").read()
    hdus = rr.split_hdus(raw)
    names = [rr.extname(h) for h, _ in hdus]
    n_el = cfg.ng[0] * cfg.ng[1] * cfg.ng[2]

    def variant(tag, i, header=None, data=None):
        out = list(hdus)
        out[i] = (header if header is not None else hdus[i][0], data if data is not None else hdus[i][1])
        f = str(tmp_path / (tag + ".fits"))
        open(f, "wb").write(rr.join_hdus(out))
        return f

    bad = {}
    bad["truncated"] = str(tmp_path / "short.fits")
    open(bad["truncated"], "wb").write(raw[:-2880])
    ip, id_ = names.index("GasPres"), names.index("GasDens")
    bad["BITPIX"] = variant("bitpix", ip, rr.replace_card(hdus[ip][0], "BITPIX  =", rr.fixed_card("BITPIX", -32)))
    bad["extents"] = variant("naxis1", id_, rr.replace_card(hdus[id_][0], "NAXIS1  =", rr.fixed_card("NAXIS1", cfg.ng[0] - 1)))
    bad["Gamma"] = variant("gamma", 0, rr.replace_card(hdus[0][0], "HIERARCH Gamma =", "HIERARCH Gamma = 1.5"))
    iz = names.index("Bz")
    null = variant("null", iz, data=rr.plant(hdus[iz][1], n_el - 1, -1.0e99))
    nan = variant("nan", id_, data=rr.plant(hdus[id_][1], 0, float("nan")))
    # planes 0 .. 5 only
    half = str(tmp_path / "half.fits")
    c0 = slab.slab_config(cfg, 0, 2)
    with orc_loop(c0, setup) as s:
        s.set_slab_extent(cfg.ng[2], 0, cfg.bc_type[4], cfg.bc_type[5])
        info = host_rccl.read_fits_header(good)[1]
        s.init(slab.slab_slice(P, cfg, 0, 2), simtime=info["t_sim"], timestep=info["t_step"], last_dt=info["last_dt"])
        s.write_fits(half)
    with orc_loop(cfg, setup) as s:
        s.init(P)
        for text, f in bad.items():
            with pytest.raises(RuntimeError, match=text):
                s.restart(f)
        with pytest.raises(RuntimeError, match="1 element"):
            s.restart(null)
        with pytest.raises(RuntimeError, match="1 element"):
            s.restart(nan)
        with pytest.raises(RuntimeError, match="different moments"):
            s.restart([good, glm_files["later"]])
        with pytest.raises(RuntimeError, match="plane 6 .* none of the files"):
            s.restart(half)
        with pytest.raises(RuntimeError, match="cannot open"):
            s.restart([good, str(tmp_path / "absent.fits")])
        # the process lives and the sim still restarts from the good file
        assert s.restart(good) == ""
        assert same(s.download(0), glm_files["state"])
    cfg2, P2, setup2 = case("glm3d")
    with orc_loop(cfg2, setup2) as s:
        s.init(P2)
        with pytest.raises(RuntimeError, match="NGrid"):
            s.restart(good)


def test_restart_picks_the_reader_by_content_not_by_name(glm_files, tmp_path):
    as_raw, as_fits = str(tmp_path / "fits_inside.pionraw"), str(tmp_path / "pionraw_inside.fits")
    shutil.copy(glm_files["fits"], as_raw)
    shutil.copy(glm_files["raw"], as_fits)
    with orc_loop(glm_files["cfg"], glm_files["setup"]) as s:
        s.restart(as_raw)
        assert same(s.download(0), glm_files["state"])
        s.restart(as_fits)   # the PIONRAW2 reader: B has the bits that were written
        with orc_loop(glm_files["cfg"], glm_files["setup"]) as t:
            t.restart(glm_files["raw"])
            assert same(s.download(0), t.download(0))
        assert not same(s.download(0), glm_files["state"])
        for mixed in ([as_raw, as_fits], [glm_files["raw"], glm_files["fits"]]):
            with pytest.raises(RuntimeError, match="two types"):
                s.restart(mixed)
        os.rename(as_raw, str(tmp_path / "back.fits"))
        s.restart(str(tmp_path / "back.fits"))
        assert same(s.download(0), glm_files["state"])
