"""Ray-traced column densities of a slab-decomposed run on the CPU: pion_host_sim_add_rt_source / write_columns /
set_column_output as collective calls of 3 ranks (processes), the C++ loop over the oracle's backend table (no
ray-tracing entries: the host route, pion_gpu_raytrace_host_part on a downloaded array) and pion_host::slab_comm_shm,
whose two relay directions carry one plane of col per internal face and source away from the source.  3-D only: the
oracle's table exchanges 3-D halos.

Every rank writes its own <base>_cols_<rank>.<step>.fits with its own planes.  Per output the ranks' images,
concatenated along z, must be == the images of the file a single-rank run of the global problem writes, the RT_* header
values equal (positions are the whole domain's), and the regular outputs byte for byte those of the run without sources.
The sources: inside rank 0 (planes travel upwards through both faces), beyond the top (downwards), at infinity along z
and across it (no message).  That the planes matter is shown first: chained with zeros in place of the received planes
the host loop does not give the whole grid's bits for any source whose chain carries a message.

A rank that fails (an uncreatable path) makes every rank return an error, and nobody blocks."""
import multiprocessing as mp
import os
import sys
import time

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TESTS = os.path.join(ROOT, "tests")
WORLD = 3
OUTPUTS = (0, 2, 4)


def case():
    """the 3-D Euler box of test_host_columns.py with 9 planes (3 per rank), a tracer, four sources"""
    from pion_amd import abi, problems
    cfg, P = problems.hd_blast_box([12, 10, 9], ntracer=1, strict_fp=1)
    nb = cfg.nbc
    P[5] = 0.25
    P[5, nb + 2:nb + 6, nb + 3:nb + 7, nb + 1:nb + 9] = 0.75
    dx = cfg.dx
    sources = [{"pos": (4.0 * dx, 3.3 * dx, 2.0 * dx), "opacity": abi.RT_OPACITY_TOTAL},
               {"pos": (-2.0 * dx, 5.0 * dx, 10.5 * dx), "opacity": abi.RT_OPACITY_MINUS},
               {"at_infinity": 1, "dir": 5, "opacity": abi.RT_OPACITY_TRACER},
               {"at_infinity": 1, "dir": 1, "opacity": abi.RT_OPACITY_TRACER}]
    return cfg, P, sources


def _open(cfg, **kw):
    from test_host_snapshot import orc_backend
    from pion_amd import host_rccl
    be = orc_backend()
    return host_rccl.HostSim(cfg, 0, backend=be.pion_backend_oracle(), **kw), be


def _rank_sim(rank, world, shm):
    from pion_amd import slab
    cfg_g, P, sources = case()
    cfg = slab.slab_config(cfg_g, rank, world)
    s, be = _open(cfg, rank=rank, world=world, periodic_z=False, shm_name=shm)
    return cfg_g, cfg, P, sources, s, be


def _run_worker(rank, world, shm, outdir, traced, q):
    """4 steps with FITS outputs every 2, with or without the sources and the columns beside every output"""
    try:
        sys.path[:0] = [ROOT, TESTS]
        os.environ["PION_NO_TORCH"] = "1"
        from test_host_snapshot import run_steps
        from pion_amd import host_rccl, slab
        cfg_g, cfg, P, sources, s, be = _rank_sim(rank, world, shm)
        with s:
            s.init(slab.slab_slice(P, cfg_g, rank, world))
            n = cfg_g.ng[2] // world
            s.set_slab_extent(cfg_g.ng[2], rank * n, cfg_g.bc_type[4], cfg_g.bc_type[5])
            used = [s.add_rt_source(src) for src in sources] if traced else []
            os.chdir(outdir)   # the header names the base: the same one, "r", in every run
            s.set_output("r", op_criterion=0, opfreq=2, checkpoint_freq=100)
            s.set_output_filetype(host_rccl.FILE_FITS)
            if traced:
                s.set_column_output(True)
            steps = run_steps(s, 4)
            q.put((rank, steps, s.download(0), used))
    except Exception as e:   # noqa: BLE001
        q.put((rank, None, repr(e), None))


def _fail_worker(rank, world, shm, outdir, failing, q):
    """write_columns on request; rank `failing` names a path that cannot be created"""
    try:
        sys.path[:0] = [ROOT, TESTS]
        os.environ["PION_NO_TORCH"] = "1"
        from pion_amd import slab
        cfg_g, cfg, P, sources, s, be = _rank_sim(rank, world, shm)
        with s:
            s.init(slab.slab_slice(P, cfg_g, rank, world))
            n = cfg_g.ng[2] // world
            s.set_slab_extent(cfg_g.ng[2], rank * n, cfg_g.bc_type[4], cfg_g.bc_type[5])
            for src in sources:
                s.add_rt_source(src)
            path = os.path.join(outdir, "no_such_dir" if rank == failing else "", "c_%d.fits" % rank)
            rc = s.lib.pion_host_sim_write_columns(s.s, os.fsencode(path))
            text = s.last_error() if rc else ""
            # the sim and the chain live on: the same call with good paths everywhere succeeds afterwards
            rc2 = s.lib.pion_host_sim_write_columns(s.s, os.fsencode(os.path.join(outdir, "again_%d.fits" % rank)))
            q.put((rank, rc, text, rc2))
    except Exception as e:   # noqa: BLE001
        q.put((rank, None, repr(e), None))


def _run_ranks(target, world, args):
    """spawn `world` processes of target(rank, world, shm name, *args, queue); {rank: result tuple}.  Joined with a
    timeout and killed in finally: a chain that blocks fails the test, it does not hang it"""
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    shm = "/pion_rc%d_%d" % (os.getpid(), time.time_ns() % 1000000007)
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
        for n in [shm] + [shm + k + str(r) for k in ("_img", "_dwn") for r in range(world)]:
            try:
                os.unlink("/dev/shm" + n)
            except OSError:
                pass
    return res


def test_the_planes_matter_for_every_source_with_a_chain():
    """not tame: with zeros in place of the received planes the chained host loop differs from the whole grid"""
    import raytrace_parts_cases as pc
    from pion_amd import abi, lib, slab
    cfg_g, P, sources = case()
    carried = 0
    for src in sources:
        roles = [lib.rt_chain(slab.slab_config(cfg_g, r, WORLD), src, pc.part_of(cfg_g, r, WORLD)) for r in range(WORLD)]
        whole = lib.raytrace_host(cfg_g, src, P)
        col, dcol, n = pc.run_chain(cfg_g, src, WORLD, pc.host_trace(cfg_g, src, WORLD, P))
        assert np.array_equal(col, whole[0]) and np.array_equal(dcol, whole[1])
        if any(r[0] != abi.RT_RECV_NONE for r in roles):
            zcol, _, _ = pc.run_chain(cfg_g, src, WORLD, pc.host_trace(cfg_g, src, WORLD, P), zeros=True)
            assert not np.array_equal(zcol, whole[0])
            carried += 1
    assert carried == 3


def test_a_run_of_three_ranks_with_columns_at_every_output(tmp_path, monkeypatch):
    from test_host_snapshot import run_steps
    from pion_amd import fits, host_rccl
    a, b, c = tmp_path / "a", tmp_path / "b", tmp_path / "c"
    a.mkdir(), b.mkdir(), c.mkdir()
    plain = _run_ranks(_run_worker, WORLD, (str(a), False))
    traced = _run_ranks(_run_worker, WORLD, (str(b), True))
    for r in range(WORLD):
        assert plain[r][1] is not None and traced[r][1] is not None, (plain[r], traced[r])
        assert traced[r][1] == plain[r][1] and np.array_equal(traced[r][2], plain[r][2])   # every dt, the state: read-only
    regular = ["r_%04d.%08d.fits" % (r, k) for r in range(WORLD) for k in OUTPUTS]
    cols = ["r_cols_%04d.%08d.fits" % (r, k) for r in range(WORLD) for k in OUTPUTS]
    assert sorted(os.listdir(a)) == sorted(regular)
    assert sorted(os.listdir(b)) == sorted(regular + cols)
    for f in regular:
        assert open(str(a / f), "rb").read() == open(str(b / f), "rb").read(), f          # byte for byte
    # the single-rank run of the global problem
    cfg_g, P, sources = case()
    s, be = _open(cfg_g)
    with s:
        used = [s.add_rt_source(src) for src in sources]
        s.init(P)
        monkeypatch.chdir(c)
        s.set_output("r", op_criterion=0, opfreq=2, checkpoint_freq=100)
        s.set_output_filetype(host_rccl.FILE_FITS)
        s.set_column_output(True)
        assert run_steps(s, 4) == traced[0][1]
    for r in range(WORLD):
        assert traced[r][3] == used                       # ids, and the whole domain's position on every rank
    for k in OUTPUTS:
        sparams, simages = fits.read(str(c / ("r_cols_0000.%08d.fits" % k)))
        rt = {key: v for key, v in sparams.items() if key.startswith("RT_")}
        assert rt["RT_Nsources"] == len(sources) and len(simages) == 2 * len(sources)
        parts = []
        for r in range(WORLD):
            params, images = fits.read(str(b / ("r_cols_%04d.%08d.fits" % (r, k))))
            assert {key: v for key, v in params.items() if key.startswith("RT_")} == rt
            # the header its FITS snapshot has, plus the RT_* keys
            rparams, _ = fits.read(str(b / ("r_%04d.%08d.fits" % (r, k))))
            assert {key: v for key, v in params.items() if not key.startswith("RT_")} == rparams
            assert list(images) == list(simages)
            parts.append(images)
        for name in simages:
            got = np.concatenate([p[name] for p in parts], 0)
            assert got.shape == simages[name].shape
            assert np.array_equal(got.view(np.uint64), simages[name].view(np.uint64)), (k, name)
            assert np.isfinite(got).all() and got.max() > 0.0


@pytest.mark.parametrize("failing", [0, 2])
def test_a_failing_rank_makes_every_rank_fail_and_nobody_blocks(failing, tmp_path):
    from pion_amd import abi
    res = _run_ranks(_fail_worker, WORLD, (str(tmp_path), failing))
    for r in range(WORLD):
        assert res[r][1] == abi.E_INVAL, res[r]
        if r == failing:
            assert "cannot create" in res[r][2]
        else:
            assert "failed, no file is written" in res[r][2]
        assert res[r][3] == 0, res[r]
    assert sorted(os.listdir(tmp_path)) == ["again_%d.fits" % r for r in range(WORLD)]
