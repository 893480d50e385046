"""Projected images of a slab-decomposed run on the CPU: pion_host_sim_write_projection as a collective call of 2 and 3
ranks (processes), the C++ loop over the oracle's backend table (no projection entries: the host route, dev_project.h's
part functions in a host loop) and pion_host::slab_comm_shm, whose send_to_above / recv_from_below carry the image
of the whole domain -- the running sums -- from rank to rank.  The last rank's file must be BYTE FOR BYTE the file a
single-rank sim of the global problem writes: no tolerance, both sides take the same route and the same additions.

The single-rank side of every comparison is pinned to the numpy restatement by tests/test_host_projection.py (and
tests/test_gpu_projection.py on the device); it is not checked again here.

Inputs (tests/projection_parts_restate.py): rough states; every rank's slab is slab.slab_slice of the global state with
NaN in the x ghosts, the lower slab ghosts and the outer upper ghost rows -- a rule that read one of them would give a
NaN image --, and the neighbour's first row in the one ghost row the Abel slope reads.  Each case asserts with numpy
that the naive assembly (per-rank sums from 0.0, added afterwards) differs from the single sum in some pixel, so a
chain that merely added partial images would fail.  Along x and y of a 3-D grid a pixel lies wholly in one rank and
there is nothing to assemble: the naive check is made for the slab axis and the cylindrical cases.

The oracle's table exchanges halos of 3-D grids only (its halo_count is 0 otherwise).  The cylindrical cases hand the
loop a copy of that table whose three halo entries do nothing: the test itself has put the neighbour's row into the
ghost row, and the image relay needs no attach()."""
import ctypes as C
import multiprocessing as mp
import os
import sys
import time

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TESTS = os.path.join(ROOT, "tests")

NENTRIES = 29   # pion_backend: the name and 28 function pointers
WORLD = {"euler_tr_70x9x10": 2, "glm_tr_66x5x15": 3, "cyl_70x10": 2, "cyl_70x40": 2, "cyl_70x40_off_axis": 2,
         "cyl_cool_70x40": 2}


def _backend(cfg):
    """(address of a pion_backend table bound to the oracle, objects to keep alive, the oracle-handle getter)"""
    from test_host_snapshot import orc_backend
    be = orc_backend()
    if cfg.ndim == 3:
        return be.pion_backend_oracle(), be, be
    Table = C.c_void_p * NENTRIES
    t = Table.from_buffer_copy(C.string_at(be.pion_backend_oracle(), C.sizeof(Table)))
    assert t[16] and not t[17], "the oracle's table: 17 entries, the rest NULL"
    count = cfg.nvar * cfg.nbc * (cfg.ng[0] + 2 * cfg.nbc)
    f_count = C.CFUNCTYPE(C.c_long, C.c_void_p)(lambda h: count)
    f_begin = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p)(lambda h, w, lo, hi: 0)
    t[13] = C.cast(f_count, C.c_void_p).value
    t[14] = C.cast(f_begin, C.c_void_p).value
    t[16] = C.cast(f_begin, C.c_void_p).value
    return C.addressof(t), (t, f_count, f_begin, be), be


def _prepare(name, seed):
    import projection_parts_restate as pp
    import projection_restate as pr
    cfg_g = pp.case(name)
    return cfg_g, pr.rough_state(cfg_g, seed), pp.fields_of(name, cfg_g)


def _open(cfg, be_addr, be, **kw):
    """(HostSim, the oracle handle's CpuSim) with the cooling tables a temperature needs"""
    from cpu_backends import CpuSim
    from pion_amd import cooling, host_rccl
    s = host_rccl.HostSim(cfg, 0, backend=be_addr, **kw)
    o = CpuSim(cfg, "orc", borrowed_handle=be.pion_backend_oracle_handle(s.gpu_handle()))
    if cfg.cooling:
        o.set_cooling_tables(*cooling.build_tables(cfg.min_temp, cfg.max_temp))
    return s, o


def _single_rank_file(name, seed, axis, path):
    import projection_parts_restate as pp
    cfg_g, P, fields = _prepare(name, seed)
    addr, keep, be = _backend(cfg_g)
    s, o = _open(cfg_g, addr, be)
    with s:
        s.init(P)
        o.upload_which(0, pp.nan_ghosts(cfg_g, P))
        s.write_projection(path, pp.axis_of(cfg_g, axis), fields)
    return open(path, "rb").read()


def _worker(rank, world, shm, name, seed, axis, path, mode, q):
    """mode: "write" (the collective call), "no_extent" (no set_slab_extent: refused, the sim lives on), "fail<r>" (rank
    r calls with a field the projection refuses)"""
    try:
        sys.path[:0] = [ROOT, TESTS]
        os.environ["PION_NO_TORCH"] = "1"
        import projection_parts_restate as pp
        from pion_amd import abi, slab
        cfg_g, P, fields = _prepare(name, seed)
        cfg, A = pp.slab_state(P, cfg_g, rank, world)
        ax = slab.slab_axis(cfg_g)
        addr, keep, be = _backend(cfg)
        periodic = cfg_g.bc_type[2 * ax] == abi.BC_PERIODIC
        s, o = _open(cfg, addr, be, rank=rank, world=world, periodic_z=periodic, shm_name=shm)
        with s:
            s.init(slab.slab_slice(P, cfg_g, rank, world))
            s.finish_halo()
            o.upload_which(0, A)
            lo, n, last, xmin = pp.part_of(cfg_g, rank, world)
            if mode != "no_extent":
                s.set_slab_extent(n, lo, cfg_g.bc_type[2 * ax], cfg_g.bc_type[2 * ax + 1])
            if mode == "fail%d" % rank:
                fields = [("x", 3)]
            arr = abi.proj_fields(fields)
            rc = s.lib.pion_host_sim_write_projection(s.s, os.fsencode(path), pp.axis_of(cfg_g, axis), len(fields), arr)
            text = s.last_error() if rc else ""
            alive = bool(np.isnan(s.download(0)).any())   # the sim lives on (and still holds the NaN ghosts)
            q.put((rank, rc, text, alive))
    except Exception as e:   # noqa: BLE001
        q.put((rank, None, repr(e), False))


def _run_ranks(target, world, args):
    """spawn `world` processes of target(rank, world, shm name, *args, queue); {rank: result tuple}.  Joined with a
    timeout and killed in finally: a chain that blocks fails the test, it does not hang it"""
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    shm = "/pion_pr%d_%d" % (os.getpid(), time.time_ns() % 1000000007)
    procs = [ctx.Process(target=target, args=(r, world, shm) + tuple(args) + (q,)) for r in range(world)]
    res = {}
    try:
        for p in procs:
            p.start()
        for _ in range(world):
            out = q.get(timeout=90)
            res[out[0]] = out
        for p in procs:
            p.join(timeout=30)
            assert p.exitcode == 0
    finally:
        for p in procs:
            if p.is_alive():
                p.kill()
        for n in (shm, shm + "_img"):
            try:
                os.unlink("/dev/shm" + n)
            except OSError:
                pass
    return res


CASES = [("euler_tr_70x9x10", 0), ("euler_tr_70x9x10", 1), ("euler_tr_70x9x10", 2),
         ("glm_tr_66x5x15", 0), ("glm_tr_66x5x15", 1), ("glm_tr_66x5x15", 2),
         ("cyl_70x10", None), ("cyl_70x40", None), ("cyl_70x40_off_axis", None), ("cyl_cool_70x40", None)]
SEED = 5


@pytest.mark.parametrize("name,axis", CASES)
def test_the_last_ranks_file_is_the_single_rank_file(name, axis, tmp_path):
    import projection_parts_restate as pp
    from pion_amd import fits
    world = WORLD[name]
    cfg_g, P, fields = _prepare(name, SEED)
    if axis in (None, 2):
        assert pp.naive_differs(cfg_g, P, fields, pp.axis_of(cfg_g, axis), world), "the state is too tame: another seed"
    single = _single_rank_file(name, SEED, axis, str(tmp_path / "single.fits"))
    path = str(tmp_path / "ranks.fits")
    res = _run_ranks(_worker, world, (name, SEED, axis, path, "write"))
    for r in range(world):
        assert res[r][1] == 0 and res[r][3], res[r]
    assert sorted(os.listdir(tmp_path)) == ["ranks.fits", "single.fits"]   # one file, no .part, nothing of other ranks
    assert open(path, "rb").read() == single
    params, images = fits.read(path)
    assert params["pion_world"] == 1 and params["pion_rank"] == 0 and params["pion_slab_lo"] == 0
    for n in images:
        assert np.isfinite(images[n]).all() and np.abs(images[n]).max() > 0.0, n


def test_more_than_one_rank_without_an_extent_is_refused(tmp_path):
    path = str(tmp_path / "x.fits")
    res = _run_ranks(_worker, 2, ("euler_tr_70x9x10", SEED, 2, path, "no_extent"))
    from pion_amd import abi
    for r in range(2):
        assert res[r][1] == abi.E_INVAL and res[r][3], res[r]
        assert "one rank of a slab run" in res[r][2] and "without a slab extent" in res[r][2]
    assert os.listdir(tmp_path) == []


@pytest.mark.parametrize("failing", [0, 1])
def test_a_failing_rank_passes_the_failure_on(failing, tmp_path):
    """rank `failing` of 3 is refused (a power of rho of 3): it still takes the message of the rank below, every rank
    above it returns an error, the last rank writes no file, nobody blocks; ranks below it have done their part"""
    from pion_amd import abi
    path = str(tmp_path / "x.fits")
    res = _run_ranks(_worker, 3, ("glm_tr_66x5x15", SEED, 2, path, "fail%d" % failing))
    for r in range(3):
        assert res[r][3], res[r]
        if r < failing:
            assert res[r][1] == 0
        elif r == failing:
            assert res[r][1] == abi.E_INVAL and "power of rho" in res[r][2]
        else:
            assert res[r][1] == abi.E_INVAL and "a rank below failed" in res[r][2]
    assert os.listdir(tmp_path) == []


def _run_worker(rank, world, shm, outdir, project, q):
    """the hd octant run of tests/test_host_two_ranks.py with regular outputs, with or without projections"""
    try:
        sys.path[:0] = [ROOT, TESTS]
        os.environ["PION_NO_TORCH"] = "1"
        from test_host_snapshot import run_steps
        from pion_amd import abi, problems, slab
        import projection_restate as pr
        cfg_g, P = problems.hd_blast_octant(12, 3, solver=abi.FLUX_RSroe, strict_fp=1, nzones=3.0)
        cfg = slab.slab_config(cfg_g, rank, world)
        addr, keep, be = _backend(cfg)
        s, o = _open(cfg, addr, be, rank=rank, world=world, periodic_z=False, shm_name=shm)
        with s:
            s.init(slab.slab_slice(P, cfg_g, rank, world))
            n = cfg_g.ng[2] // world
            s.set_slab_extent(cfg_g.ng[2], rank * n, cfg_g.bc_type[4], cfg_g.bc_type[5])
            os.chdir(outdir)   # the header names the base: the same one, "r", in every run
            s.set_output("r", op_criterion=0, opfreq=2, checkpoint_freq=100)
            if project:
                s.set_projection_output(2, pr.fields_of(cfg_g)[:2])
            steps = run_steps(s, 4)
            q.put((rank, steps, s.download(0), s.download(1)))
    except Exception as e:   # noqa: BLE001
        q.put((rank, None, repr(e), None))


def test_a_run_of_two_ranks_with_projections_at_every_output(tmp_path, monkeypatch):
    from test_host_snapshot import run_steps
    from pion_amd import abi, problems
    import projection_restate as pr
    a, b, c = tmp_path / "a", tmp_path / "b", tmp_path / "c"
    a.mkdir(), b.mkdir(), c.mkdir()
    plain = _run_ranks(_run_worker, 2, (str(a), False))
    proj = _run_ranks(_run_worker, 2, (str(b), True))
    for r in range(2):
        assert plain[r][1] is not None and proj[r][1] is not None, (plain[r], proj[r])
        assert proj[r][1] == plain[r][1]                                            # every dt and time, ==
        assert np.array_equal(proj[r][2], plain[r][2]) and np.array_equal(proj[r][3], plain[r][3])
    snaps = ["r_%04d.%08d.pionraw" % (r, k) for r in (0, 1) for k in (0, 2, 4)]
    images = ["r_proj_0000.%08d.fits" % k for k in (0, 2, 4)]      # one file per output, under rank 0000
    assert sorted(os.listdir(a)) == sorted(snaps)
    assert sorted(os.listdir(b)) == sorted(snaps + images)
    # the single-rank run of the global problem writes the same files
    cfg_g, P = problems.hd_blast_octant(12, 3, solver=abi.FLUX_RSroe, strict_fp=1, nzones=3.0)
    addr, keep, be = _backend(cfg_g)
    s, o = _open(cfg_g, addr, be)
    with s:
        s.init(P)
        monkeypatch.chdir(c)
        s.set_output("r", op_criterion=0, opfreq=2, checkpoint_freq=100)
        s.set_projection_output(2, pr.fields_of(cfg_g)[:2])
        assert run_steps(s, 4) == proj[0][1]
    for f in images:
        assert open(str(c / f), "rb").read() == open(str(b / f), "rb").read(), f


# ---- the part functions themselves, through the C view of the host library (no sim, no processes) -------------------
def _host_lib():
    from pion_amd import host_rccl
    return host_rccl.load_host_library()


def _dp(a):
    return a.ctypes.data_as(C.POINTER(C.c_double))


def _part_on_host(cfg, axis, fields, part, A, img):
    from pion_amd import abi
    A = np.ascontiguousarray(A, dtype=np.float64)
    rc = _host_lib().pion_host_project_part_on_host(C.byref(cfg), axis, len(fields), abi.proj_fields(fields),
                                                    C.byref(abi.proj_part(part)), _dp(A), _dp(img))
    assert rc == 0
    return img


PART_CASES = [("euler_tr_70x9x10", 0), ("euler_tr_70x9x10", 1), ("euler_tr_70x9x10", 2), ("glm_tr_66x5x15", 2),
              ("cyl_70x10", None), ("cyl_70x40_off_axis", None), ("cyl_cool_70x40", None)]


@pytest.mark.parametrize("name,axis", PART_CASES)
def test_a_part_that_is_the_whole_grid_equals_the_column_functions(name, axis):
    """proj_column_part / abel_column_part with plane_lo = 0, global_planes = the grid's own planes, last = 1 on +0.0 ==
    proj_column / abel_column, every pixel; and the same functions as a chain of parts, called one after another
    here, == again.  Every ghost cell of the whole grid is NaN."""
    import fits_restate as fr
    import projection_parts_restate as pp
    from pion_amd import abi
    cfg, P, fields = _prepare(name, SEED)
    axis = pp.axis_of(cfg, axis)
    A = np.ascontiguousarray(pp.nan_ghosts(cfg, P))
    lo, n, last, xmin = pp.part_of(cfg, 0, 1)
    nimg = _part_count(cfg, axis, len(fields))
    column = np.full(nimg, -7.0)
    assert _host_lib().pion_host_project_on_host(C.byref(cfg), axis, len(fields), abi.proj_fields(fields), _dp(A),
                                                 _dp(column)) == 0
    assert np.isfinite(column).all() and np.abs(column).max() > 0.0
    whole = _part_on_host(cfg, axis, fields, (0, n, 1, xmin), A, np.zeros(nimg))
    assert fr.same_bits(whole, column)
    world = WORLD[name]
    img = np.zeros(nimg)
    for rank in range(world):
        cfg_r, A_r = pp.slab_state(P, cfg, rank, world)
        _part_on_host(cfg_r, axis, fields, pp.part_of(cfg, rank, world), A_r, img)
    assert fr.same_bits(img, column)


def _part_count(cfg, axis, nfields):
    ng = list(cfg.ng)
    if cfg.coord_sys == 2:
        return nfields * ng[1] * ng[0]
    return nfields * {0: ng[2] * ng[1], 1: ng[2] * ng[0], 2: ng[1] * ng[0]}[axis]


def test_refusals_of_the_part_functions_on_the_host():
    """what pion_gpu_project_part refuses (tests/test_gpu_projection_ranks.py: the same texts from the device entry
    points), from the same function, proj_refused_part, on the CPU"""
    import projection_parts_restate as pp
    import projection_restate as pr
    from pion_amd import abi
    h = _host_lib()
    cfg = pp.case("cyl_70x10")
    perp = abi.PROJ_AXIS_PERP
    arr = abi.proj_fields(pr.fields_of(cfg)[:1])
    A = np.ascontiguousarray(pr.rough_state(cfg, SEED))
    img = np.zeros(70 * 20)
    refused = lambda axis, f, part, buf: h.pion_host_project_part_refused(
        C.byref(cfg), axis, 1, f, C.byref(abi.proj_part(part)) if part is not None else None, buf)
    bad = [((-1, 20, 0, 0.0), "plane_lo is not negative"), ((11, 20, 1, 0.0), "end above global_planes"),
           ((0, 9, 1, 0.0), "end above global_planes"), ((0, 20, 0, float("nan")), "global_xmin is finite"),
           ((0, 20, 0, float("inf")), "global_xmin is finite"), (None, "no part")]
    for part, text in bad:
        assert text in refused(perp, arr, part, _dp(img)).decode(), part
        p = C.byref(abi.proj_part(part)) if part is not None else None
        assert h.pion_host_project_part_on_host(C.byref(cfg), perp, 1, arr, p, _dp(A), _dp(img)) == abi.E_INVAL
    ok = (0, 20, 0, 0.0)
    assert "no buffer" in refused(perp, arr, ok, None).decode()
    assert h.pion_host_project_part_on_host(C.byref(cfg), perp, 1, arr, C.byref(abi.proj_part(ok)), _dp(A), None) == abi.E_INVAL
    # everything the whole-grid call refuses
    assert "along the symmetry axis" in refused(0, arr, ok, _dp(img)).decode()
    assert "power of rho" in refused(perp, abi.proj_fields([("x", 3)]), ok, _dp(img)).decode()
    assert (img == 0.0).all()
    assert refused(perp, arr, ok, _dp(img)) is None
    assert h.pion_host_project_part_on_host(C.byref(cfg), perp, 1, arr, C.byref(abi.proj_part(ok)), _dp(A), _dp(img)) == 0
    assert np.isfinite(img).all() and np.abs(img[:70 * 10]).max() > 0.0 and (img[70 * 10:] == 0.0).all()


def test_a_communicator_without_the_pair_is_refused(tmp_path):
    """a communicator of two ranks that leaves send_to_above / recv_from_below at the interface's default
    (tests/native/norelay_comm.cpp, compiled here): "not supported", from the calls and from the writer"""
    import subprocess
    import projection_parts_restate as pp
    from pion_amd import abi, slab
    so = str(tmp_path / "libnorelay_comm.so")
    subprocess.check_call([os.environ.get("CXX", "g++"), "-O1", "-fPIC", "-shared", "-std=c++14", "-o", so,
                           os.path.join(TESTS, "native", "norelay_comm.cpp")])
    nr = C.CDLL(so)
    nr.norelay_comm_create.restype = C.c_void_p
    nr.norelay_comm_recv.argtypes = [C.c_void_p, C.c_void_p, C.c_ulong, C.POINTER(C.c_int)]
    nr.norelay_comm_send.argtypes = [C.c_void_p, C.c_void_p, C.c_ulong, C.c_int]
    cfg_g, P, fields = _prepare("euler_tr_70x9x10", SEED)
    cfg = slab.slab_config(cfg_g, 0, 2)
    addr, keep, be = _backend(cfg)
    s, o = _open(cfg, addr, be)
    out = tmp_path / "out"
    out.mkdir()
    with s:
        s.comm = C.c_void_p(nr.norelay_comm_create(0, 2))     # (HostSim.close destroys it before the sim)
        buf, status = np.zeros(4), C.c_int(7)
        assert nr.norelay_comm_recv(s.comm, buf.ctypes.data, 32, C.byref(status)) == abi.E_INVAL
        assert nr.norelay_comm_send(s.comm, buf.ctypes.data, 32, 0) == abi.E_INVAL
        assert s.lib.pion_host_sim_set_comm(s.s, s.comm) == 0
        s.init(slab.slab_slice(P, cfg_g, 0, 2))
        s.set_slab_extent(cfg_g.ng[2], 0, cfg_g.bc_type[4], cfg_g.bc_type[5])
        arr = abi.proj_fields(fields)
        path = os.fsencode(str(out / "x.fits"))
        assert s.lib.pion_host_sim_write_projection(s.s, path, 2, len(fields), arr) == abi.E_INVAL
        assert "one rank of a slab run" in s.last_error() and "not supported" in s.last_error()
        with pytest.raises(ValueError, match="not supported"):
            s.set_projection_output(2, fields)
        s.download(0)   # the sim lives on
    assert os.listdir(out) == []
