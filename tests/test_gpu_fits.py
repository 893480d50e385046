"""FITS output on the GPU: the kernels of pion_output.hip (pion_gpu_pack_fits) against the numpy restatement of
tests/fits_restate.py, the fast build against the strict one, the streamed file against the file the fallback route
writes, and the C++ loop's files against the oracle-bound loop's and across two ranks.  Every comparison is == on the
8 bytes.

Shapes of the kernel test, the smallest at which the mapping can go wrong: 3-D GLM 5 x 4 x 3; 3-D Euler + tracer +
cooling 70 x 3 x 2 (a row longer than a wavefront, no multiple of 64); 2-D MHD 1030 x 3 (a row that crosses the
1024-cell stretch); 2-D cylindrical GLM 6 x 5; 1-D Euler 7; 1-D spherical 9.  The states are seeded random numbers
uploaded with random ghost cells and no boundary update in between: the stencil demonstrably reads ghosts."""
import ctypes as C
import os

import numpy as np
import pytest

import fits_restate as fr
from pion_amd import abi, host_rccl, lib, problems
from test_host_snapshot import orc_loop, run_steps

pytestmark = pytest.mark.gpu
nosetup = lambda sim, c: None

SHAPES = ["glm_5x4x3", "euler_tr_cool_70x3x2", "mhd_1030x3", "cyl_glm_6x5", "euler_7", "sph_9"]


def kernel_case(name, strict):
    kw = dict(strict_fp=strict, dx=0.125)
    if name == "glm_5x4x3":
        return abi.make_config(3, [5, 4, 3], abi.EQGLM, abi.FLUX_RS_HLLD, **kw)
    if name == "euler_tr_cool_70x3x2":
        return abi.make_config(3, [70, 3, 2], abi.EQEUL, abi.FLUX_RSroe, ntracer=1, cooling=8, min_temp=5.0e3,
                               max_temp=1.0e8, **kw)
    if name == "mhd_1030x3":
        return abi.make_config(2, [1030, 3], abi.EQMHD, abi.FLUX_RS_HLLD, **kw)
    if name == "cyl_glm_6x5":
        return abi.make_config(2, [6, 5], abi.EQGLM, abi.FLUX_RS_HLLD, coord_sys=2,
                               bcs=["outflow", "outflow", "axisymmetric", "outflow"], **kw)
    if name == "euler_7":
        return abi.make_config(1, [7], abi.EQEUL, abi.FLUX_RSroe, **kw)
    if name == "sph_9":
        return abi.make_config(1, [9], abi.EQEUL, abi.FLUX_RSroe, coord_sys=3, bcs=["reflecting", "outflow"], **kw)
    raise KeyError(name)


def _pack(g, lo, hi):
    """the buffer of planes [lo, hi) as native doubles [nimage][planes * rows * nx], and the guard words behind it"""
    import torch
    n = g.fits_count(hi - lo)
    buf = torch.full((n + 8,), -7.0, dtype=torch.float64, device="cuda:0")
    g.pack_fits(lo, hi, buf.data_ptr())
    g.synchronize()
    raw = buf.cpu().numpy()
    assert (raw[n:] == -7.0).all(), "wrote past the buffer"
    return raw[:n].view(">f8").astype("=f8")


def _planes(img, cfg, lo, hi):
    """planes [lo, hi) of a restated image [nz][ny][nx]"""
    if cfg.ndim == 3:
        return img[lo:hi]
    if cfg.ndim == 2:
        return img[:, lo:hi]
    return img


@pytest.mark.parametrize("name", SHAPES)
def test_pack_fits_equals_the_restatement_in_both_builds(name):
    cfg0 = kernel_case(name, 1)
    P = np.random.default_rng(7).uniform(0.5, 1.5, size=problems.alloc(cfg0).shape)
    P[2:] -= 1.0   # velocities, B, psi, tracers of both signs
    nplanes = 1 if cfg0.ndim == 1 else cfg0.ng[cfg0.ndim - 1]
    ranges = [(0, nplanes)] + ([(1, 2)] if nplanes > 1 else [])
    got = {}
    for strict in (1, 0):
        cfg = kernel_case(name, strict)
        with lib.GpuSim(cfg, 0) as g:
            g.upload(P)   # random ghost cells, no boundary update
            assert g.fits_images() == fr.image_names(cfg)
            want = fr.restate(cfg, P)
            for lo, hi in ranges:
                assert g.fits_count(hi - lo) == len(want) * (hi - lo) * (cfg.ng[1] if cfg.ndim == 3 else 1) * cfg.ng[0]
                buf = _pack(g, lo, hi).reshape(len(want), -1)
                for i, (n, img) in enumerate(want):
                    assert fr.same_bits(buf[i], np.ascontiguousarray(_planes(img, cfg, lo, hi)).reshape(-1)), \
                        (name, strict, lo, hi, n)
                got[(strict, lo, hi)] = buf
            for bad in ((-1, 1), (0, nplanes + 1), (1, 1)):
                with pytest.raises(lib.PionGpuError):
                    g.pack_fits(bad[0], bad[1], 8)
            with pytest.raises(lib.PionGpuError):
                g.pack_fits(0, 1, 0)
    for lo, hi in ranges:   # fast against strict
        assert fr.same_bits(got[(0, lo, hi)], got[(1, lo, hi)]), (lo, hi)


class _Table(C.Structure):
    """pion_backend (pion_amd/host/pion_backend.h): the name and 22 function pointers"""
    _fields_ = [("f%d" % i, C.c_void_p) for i in range(23)]


def _table_without_fits_entries():
    """a copy of the product's backend table as it was before the fits_* entries existed"""
    h = host_rccl.load_host_library()
    h.pion_backend_gpu.restype = C.c_void_p
    t = _Table.from_buffer_copy(C.string_at(h.pion_backend_gpu(), C.sizeof(_Table)))
    assert t.f21 and t.f22 and t.f20
    t.f21 = t.f22 = None
    return t


def test_streamed_file_equals_the_fallback_file(tmp_path, monkeypatch):
    """chunks of 1 and 4 planes (6 planes: an uneven last chunk) and the default, fast build, two steps in"""
    cfg, P = problems.mhd_blast_generic([13, 7, 6], strict_fp=0)
    table = _table_without_fits_entries()
    with host_rccl.HostSim(cfg, 0, backend=C.addressof(table)) as s:
        s.init(P)
        run_steps(s, 2)
        s.write_fits(str(tmp_path / "fallback.fits"))
        state = s.download(0)
    whole = open(str(tmp_path / "fallback.fits"), "rb").read()
    for n, img in fr.restate(cfg, state):
        assert fr.same_bits(fr.images_of(str(tmp_path / "fallback.fits"))[n], img), n
    with host_rccl.HostSim(cfg, 0) as s:
        s.init(P)
        run_steps(s, 2)
        assert np.array_equal(s.download(0), state)
        for chunk in ("1", "4", None):
            if chunk is None:
                monkeypatch.delenv("PION_SNAPSHOT_CHUNK_PLANES", raising=False)
            else:
                monkeypatch.setenv("PION_SNAPSHOT_CHUNK_PLANES", chunk)
            f = str(tmp_path / ("streamed_%s.fits" % chunk))
            s.write_fits(f)
            assert open(f, "rb").read() == whole, chunk
        # the PIONRAW2 writer shares the slots and the loop: it still writes the same file after a FITS write
        s.write_snapshot(str(tmp_path / "a.pionraw"))
        s.write_fits(str(tmp_path / "again.fits"))
        s.write_snapshot(str(tmp_path / "b.pionraw"))
        assert open(str(tmp_path / "a.pionraw"), "rb").read() == open(str(tmp_path / "b.pionraw"), "rb").read()


def test_c_loop_images_equal_the_oracle_bound_loops(tmp_path):
    """strict build, five steps of a GLM case through the C++ loop, regular outputs as FITS"""
    cfg, P = problems.mhd_blast_generic([20, 12, 9], strict_fp=1)
    files = {}
    for who, make in (("orc", lambda: orc_loop(cfg, nosetup)), ("gpu", lambda: host_rccl.HostSim(cfg, 0))):
        base = str(tmp_path / who)
        with make() as s:
            s.init(P)
            s.set_output(base, op_criterion=0, opfreq=5, checkpoint_freq=4)
            s.set_output_filetype(host_rccl.FILE_FITS)
            s.time_int(5)
        assert sorted(os.listdir(tmp_path)).count(who + "_0000.00000005.fits") == 1
        assert os.path.exists(base + "_0000.99999999.pionraw")   # the checkpoint of step 4
        files[who] = fr.images_of(base + "_0000.00000005.fits")
    assert list(files["gpu"]) == list(files["orc"]) and len(files["gpu"]) == 12
    for n in files["orc"]:
        assert fr.same_bits(files["gpu"][n], files["orc"][n]), n


@pytest.mark.parametrize("name", ["glm3d_z12", "glm2d_y12"])
def test_two_ranks_on_one_gpu_joined_images_equal_the_single_domain(name, tmp_path):
    """3-D cut along z, 2-D cut along y: two processes on device 0 over the shared-memory transport, two steps"""
    cfg, P = fr.two_rank_case(name)
    single = str(tmp_path / "single.fits")
    with host_rccl.HostSim(cfg, 0) as s:
        s.init(P)
        steps = run_steps(s, 2)
        s.write_fits(single)
    paths = [str(tmp_path / ("r%d.fits" % r)) for r in range(2)]
    times = fr.run_two_ranks(name, "gpu", 2, paths)
    assert times[0]["simtime"] == times[1]["simtime"] == steps[-1][1]
    want = fr.images_of(single)
    parts = [fr.images_of(p) for p in paths]
    for n in want:
        assert fr.same_bits(np.concatenate([q[n] for q in parts], axis=0), want[n]), n
    assert np.abs(want["divB"]).max() > 0.0
