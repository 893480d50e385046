"""Output times, checkpoints and snapshot / restart of the C++ host loop (pion_host::sim_control_gpu + snapshot_io),
on the CPU: the loop runs over the oracle's backend table (tests/native/orc_backend.cpp), whose snapshot entries are
NULL, so the files are written and read through whole-array download / upload with the ghosts stripped / embedded on
the host.  (tests/test_gpu_host_snapshot.py: the same files streamed from the device.)

Restated here, not imported: the limiter with its output-time clip (calc_timestep.cpp:219-262), equalD
(constants.cpp:48-70) and the output cadence of sim_init::output_data (sim_init.cpp:671-760)."""
import ctypes as C
import glob
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NATIVE = os.path.join(ROOT, "tests", "native")

from cpu_backends import CpuSim  # noqa: E402
from pion_amd import abi, driver, host_rccl, problems, slab, snapshot  # noqa: E402

HEADER_KEYS = ["gridndim", "NGrid", "Ncell", "Xmin", "Xmax", "eqn_type", "eqn_nvar", "num_tracer", "solver",
               "coord_sys", "Space_OOA", "Time_OOA", "Gamma", "CFL", "art_visc", "eta_visc", "Ref_Vector",
               "EP_cooling", "EP_MP_timestep_limit", "EP_Min_Temperature", "EP_Max_Temperature", "t_start", "t_finish",
               "t_step", "t_sim", "min_timestep", "last_dt", "op_freq", "opfreq_time", "op_criterion", "outfile",
               "BC_XN", "BC_XP", "BC_YN", "BC_YP", "BC_ZN", "BC_ZP", "BC_Ninternal", "JetSim", "WIND_Nsources",
               "pion_nbc", "pion_strict_fp", "pion_bc_dmach2", "pion_next_optime", "pion_rank", "pion_world",
               "pion_slab_lo", "pion_slab_n", "pion_data_offset"]


def orc_backend():
    subprocess.check_call(["make", "-s", "-C", NATIVE])
    lib = C.CDLL(os.path.join(NATIVE, "liborc_backend.so"))
    lib.pion_backend_oracle.restype = C.c_void_p
    lib.pion_backend_oracle_handle.restype = C.c_void_p
    lib.pion_backend_oracle_handle.argtypes = [C.c_void_p]
    return lib


def equalD(a, b):
    """constants::equalD"""
    if a == b:
        return True
    if abs(a) + abs(b) < 1.0e-100:
        return True
    return abs(a - b) / (abs(a) + abs(b) + 1.0e-100) < 1.0e-12


def case(name, strict_fp=1):
    """(cfg, P, setup): setup(handle-level sim, cfg) makes tables / wind cells and returns the first-step dt limit"""
    nosetup = lambda sim, cfg: None
    if name == "glm3d":
        return problems.mhd_blast_generic([20, 12, 9], strict_fp=strict_fp) + (nosetup,)
    if name == "glm3d_z12":
        return problems.mhd_blast_generic([20, 12, 12], strict_fp=strict_fp) + (nosetup,)
    if name == "glm20":
        return problems.mhd_blastwave(20, 3, abi.EQGLM, abi.FLUX_RS_HLLD, strict_fp=strict_fp) + (nosetup,)
    if name == "hd3d":
        return problems.hd_blast_box([12, 10, 8], strict_fp=strict_fp) + (nosetup,)
    if name == "axi2d":
        return problems.blast_axi2d(24, abi.EQGLM, abi.FLUX_RS_HLLD, ntracer=1, strict_fp=strict_fp) + (nosetup,)
    if name == "euler_axi2d":
        return problems.blast_axi2d(24, strict_fp=strict_fp) + (nosetup,)
    if name == "cart2d":
        return problems.hd_blast_box([16, 12], strict_fp=strict_fp) + (nosetup,)
    if name == "dmr2d":
        return problems.double_mach_reflection(32, strict_fp=strict_fp) + (nosetup,)
    if name == "sph1d":
        return problems.blast_sph1d(128, strict_fp=strict_fp) + (nosetup,)
    if name == "wind3d":
        cfg, P, _, _ = problems.wind3d(16, strict_fp=strict_fp)

        def setup(sim, c):
            from pion_amd import cooling
            sim.set_cooling_tables(*cooling.build_tables(c.min_temp, c.max_temp))
            _, (idx, st), dt_lim = problems.fill_wind3d(c, 16)
            if idx.size:
                sim.set_wind_cells(idx, st)
            return dt_lim
        return cfg, P, setup
    raise KeyError(name)


class OrcLoop:
    """host_rccl.HostSim over the oracle's backend table, with the set-up calls of its handle"""

    def __init__(self, cfg, setup, **kw):
        self.be = orc_backend()
        self.s = host_rccl.HostSim(cfg, 0, backend=self.be.pion_backend_oracle(), **kw)
        o = CpuSim(cfg, "orc", borrowed_handle=self.be.pion_backend_oracle_handle(self.s.gpu_handle()))
        self.dt_limit = setup(o, cfg)

    def __enter__(self):
        return self.s

    def __exit__(self, *a):
        self.s.close()


def run_steps(s, n):
    """n single steps of the C++ loop: [(dt, simtime), ...]"""
    out = []
    for _ in range(n):
        k, t, ldt = s.time_int(1)
        assert k == 1
        out.append((ldt, t))
    return out


RESTART_CASES = ["glm3d", "hd3d", "axi2d", "sph1d", "wind3d"]


def restart_roundtrip(make_loop, name, tmp_path, strict_fp=1, write_loop=None, nwrite=2, nmore=3):
    """uninterrupted nwrite + nmore steps against write at nwrite (by write_loop), restart in a fresh make_loop sim,
    nmore more steps: returns ((P, Ph, steps) uninterrupted, (P, Ph, steps) restarted)"""
    cfg, P, setup = case(name, strict_fp)
    path = str(tmp_path / (name + ".pionraw"))
    with make_loop(cfg, setup) as s:
        s.init(P, first_step_dt_limit=make_loop.last_dt_limit())
        steps = run_steps(s, nwrite + nmore)
        ref = (s.download(0), s.download(1), steps)
    with (write_loop or make_loop)(cfg, setup) as s:
        s.init(P, first_step_dt_limit=(write_loop or make_loop).last_dt_limit())
        first = run_steps(s, nwrite)
        s.write_snapshot(path)
    with make_loop(cfg, setup) as s:
        s.restart(path)
        t = s.get_time()
        assert t["timestep"] == nwrite and t["simtime"] == first[-1][1] and t["last_dt"] == first[-1][0]
        steps = first + run_steps(s, nmore)
        got = (s.download(0), s.download(1), steps)
    return ref, got


class _OrcFactory:
    """make_loop for restart_roundtrip: the oracle-bound loop"""

    def __init__(self):
        self._lim = None

    def __call__(self, cfg, setup, **kw):
        loop = OrcLoop(cfg, setup, **kw)
        self._lim = loop.dt_limit
        return loop

    def last_dt_limit(self):
        return self._lim


orc_loop = _OrcFactory()


@pytest.mark.parametrize("name", RESTART_CASES)
def test_restart_is_bit_identical(name, tmp_path):
    ref, got = restart_roundtrip(orc_loop, name, tmp_path)
    assert got[2] == ref[2], "dt / simtime sequence"
    assert np.array_equal(got[0], ref[0]) and np.array_equal(got[1], ref[1])


def test_unset_output_takes_the_parent_loops_steps():
    cfg, P, setup = case("glm20")
    with CpuSim(cfg, "orc") as o:
        sc = driver.SimControl(o, cfg)
        sc.init(P)
        want = []
        for _ in range(6):
            sc.calculate_timestep()
            sc.advance_time()
            want.append((sc.last_dt, sc.simtime))
    with orc_loop(cfg, setup) as s:
        s.init(P)
        assert run_steps(s, 6) == want


def test_output_time_clip_and_files(tmp_path):
    """op_criterion 1 with opfreq_time = 2.5 first steps: the limiter restated here, with ==; a file per output time"""
    cfg, P, setup = case("glm20")
    nsteps = 9
    with CpuSim(cfg, "orc") as o:
        sc = driver.SimControl(o, cfg)
        sc.init(P)
        dt0 = sc.calculate_timestep()
    T = 2.5 * dt0
    # the restated loop: SimControl's stages, the limiter of timestep_checking_and_limiting with the clip
    want, out_steps = [], [0]
    with CpuSim(cfg, "orc") as o:
        sc = driver.SimControl(o, cfg)
        sc.init(P)
        next_optime = 0.0 + T
        for _ in range(nsteps):
            t_dyn, t_mp = o.calc_dt()
            dt = min(t_dyn, t_mp)
            o.set_glm_speeds(t_dyn, cfg.dx, 0.25 / cfg.dx)
            dt = min(dt, 1.3 * sc.last_dt)
            dt = min(dt, next_optime - sc.simtime)
            assert dt > 0.0
            dt = min(dt, sc.finishtime - sc.simtime)
            sc.dt = dt
            sc.advance_time()
            want.append((dt, sc.simtime))
            if equalD(sc.simtime, next_optime):
                next_optime += T
                out_steps.append(sc.timestep)
    assert len(out_steps) >= 3 and any(b - a > 1 for a, b in zip(out_steps, out_steps[1:])), "clip not exercised"
    base = str(tmp_path / "clip")
    with orc_loop(cfg, setup) as s:
        s.init(P)
        s.set_output(base, op_criterion=1, opfreq_time=T, checkpoint_freq=1000)
        got = run_steps(s, nsteps)
        assert s.get_time()["next_optime"] == next_optime
    assert got == want
    files = sorted(glob.glob(base + "_0000.*.pionraw"))
    assert files == [base + "_0000.%08d.pionraw" % k for k in out_steps]
    for i, f in enumerate(files):
        _, info = host_rccl.read_snapshot_header(f)
        assert equalD(info["t_sim"], i * T) and info["t_step"] == out_steps[i]
        assert info["next_optime"] == (i + 1) * T or equalD(info["next_optime"], (i + 1) * T)


def test_cadence_and_checkpoints(tmp_path):
    cfg, P, setup = case("hd3d")
    base = str(tmp_path / "cad")
    ck = {0: base + "_0000.99999998.pionraw", 1: base + "_0000.99999999.pionraw"}
    with orc_loop(cfg, setup) as s:
        s.init(P)
        s.set_output(base, op_criterion=0, opfreq=3, checkpoint_freq=2)
        for step in range(1, 10):
            s.time_int(1)
            regular = sorted(f for f in glob.glob(base + "_0000.*.pionraw") if ".9999999" not in f)
            assert regular == [base + "_0000.%08d.pionraw" % k for k in range(0, step + 1, 3)], step
            if step % 2 == 0:
                # ids alternate with the parity of step / checkpoint_freq; the later one overwrites its predecessor
                f = ck[0] if step % 4 == 0 else ck[1]
                assert host_rccl.read_snapshot_header(f)[1]["t_step"] == step
            assert os.path.exists(ck[1]) == (step >= 2) and os.path.exists(ck[0]) == (step >= 4)
    assert not glob.glob(str(tmp_path / "*.part"))


def test_opfreq_zero_writes_first_and_final_state_only(tmp_path):
    cfg, P, setup = case("hd3d")
    with orc_loop(cfg, setup) as s:
        s.init(P)
        t = run_steps(s, 4)
    finish = 0.5 * (t[2][1] + t[3][1])   # inside the fourth step
    base = str(tmp_path / "fin")
    with orc_loop(cfg, setup) as s:
        s.init(P, finishtime=finish)
        s.set_output(base, op_criterion=0, opfreq=0, checkpoint_freq=1000)
        n, tend, _ = s.time_int(-1)
        assert n == 4 and tend == finish
    assert sorted(os.listdir(tmp_path)) == ["fin_0000.00000000.pionraw", "fin_0000.00000004.pionraw"]
    assert host_rccl.read_snapshot_header(base + "_0000.00000004.pionraw")[1]["t_sim"] == finish


def test_restart_mid_interval_keeps_the_output_times(tmp_path):
    cfg, P, setup = case("glm3d")
    with orc_loop(cfg, setup) as s:
        s.init(P)
        dt0 = run_steps(s, 1)[0][0]
    T = 2.5 * dt0
    a, b = tmp_path / "a", tmp_path / "b"
    a.mkdir(), b.mkdir()
    with orc_loop(cfg, setup) as s:
        s.init(P)
        s.set_output(str(a / "r"), op_criterion=1, opfreq_time=T, checkpoint_freq=1000)
        want = run_steps(s, 7)
        want_next = s.get_time()["next_optime"]
    with orc_loop(cfg, setup) as s:
        s.init(P)
        s.set_output(str(b / "r"), op_criterion=1, opfreq_time=T, checkpoint_freq=1000)
        first = run_steps(s, 2)
        assert not equalD(first[-1][1], T), "step 2 must lie inside an output interval"
        s.write_snapshot(str(tmp_path / "mid.pionraw"))
    with orc_loop(cfg, setup) as s:
        s.set_output(str(b / "r"), op_criterion=1, opfreq_time=T, checkpoint_freq=1000)
        s.restart(str(tmp_path / "mid.pionraw"))
        assert s.get_time()["next_optime"] == T
        got = first + run_steps(s, 5)
        assert s.get_time()["next_optime"] == want_next
    assert got == want
    assert sorted(os.listdir(a)) == sorted(os.listdir(b)) and len(os.listdir(a)) >= 3


def test_header_names_and_values(tmp_path):
    cfg, P, setup = case("axi2d")
    path = str(tmp_path / "h.pionraw")
    with orc_loop(cfg, setup) as s:
        s.init(P)
        s.set_output(str(tmp_path / "o"), op_criterion=1, opfreq_time=0.37, checkpoint_freq=7)
        steps = run_steps(s, 2)
        s.write_snapshot(path)
        state = s.download(0)
    gcfg, Pz, hd = snapshot.read(path)
    for k in HEADER_KEYS:
        assert k in hd, k
    ccfg, info = host_rccl.read_snapshot_header(path)
    for c in (gcfg, ccfg):
        for f, _ in abi.PionGpuConfig._fields_:
            a, b = getattr(c, f), getattr(cfg, f)
            assert (list(a) == list(b)) if hasattr(a, "__len__") else (a == b), f
    f8 = lambda k: [float(x) for x in hd[k].split()]
    assert f8("Gamma") == [cfg.gamma] and f8("CFL") == [cfg.cfl] and f8("eta_visc") == [cfg.etav]
    assert f8("Ref_Vector") == list(cfg.refvec)[:cfg.nvar]
    assert f8("Xmin")[:2] == list(cfg.xmin)[:2] and f8("Xmax")[0] == cfg.xmin[0] + cfg.ng[0] * cfg.dx
    assert [int(x) for x in hd["NGrid"].split()] == list(cfg.ng) and int(hd["Ncell"]) == cfg.ng[0] * cfg.ng[1]
    assert [hd[k] for k in ("BC_XN", "BC_XP", "BC_YN", "BC_YP", "BC_ZN", "BC_ZP")] == \
        ["outflow", "outflow", "axisymmetric", "outflow", "NONE", "NONE"]
    assert f8("t_sim") == [steps[-1][1]] == [info["t_sim"]] and f8("last_dt") == [steps[-1][0]] == [info["last_dt"]]
    assert int(hd["t_step"]) == 2 == info["t_step"] and f8("opfreq_time") == [0.37] == [info["opfreq_time"]]
    assert f8("pion_next_optime") == [info["next_optime"]] == [0.37]
    assert int(hd["op_criterion"]) == 1 == info["op_criterion"] and hd["outfile"] == info["outfile"] == str(tmp_path / "o")
    assert (info["rank"], info["world"], info["slab_lo"], info["slab_n"]) == (0, 1, 0, cfg.ng[1])
    assert int(hd["pion_data_offset"]) == info["data_offset"]
    nb = cfg.nbc
    assert np.array_equal(Pz[:, :, nb:-nb, nb:-nb], state[:, :, nb:-nb, nb:-nb])
    ghosts = Pz.copy()
    ghosts[:, :, nb:-nb, nb:-nb] = 0.0
    assert not ghosts.any()


def _edit_header(src, dst, old, new):
    """the file with one header line replaced by another of the same length"""
    raw = open(src, "rb").read()
    old, new = old.encode(), new.encode()
    assert len(old) == len(new) and raw.count(old) == 1
    open(dst, "wb").write(raw.replace(old, new))


def test_bad_files_return_an_error_and_a_text(tmp_path):
    cfg, P, setup = case("glm3d_z12")
    good = str(tmp_path / "good.pionraw")
    with orc_loop(cfg, setup) as s:
        s.init(P)
        run_steps(s, 1)
        s.write_snapshot(good)
        want = s.download(0)
    raw = open(good, "rb").read()
    bad = {}
    bad["magic"] = str(tmp_path / "magic.pionraw")
    open(bad["magic"], "wb").write(b"PIONRAW9" + raw[8:])
    gamma_line = [l for l in raw[8:4096].split(b"\n") if l.startswith(b"Gamma ")][0].decode() + "\n"
    bad["key"] = str(tmp_path / "key.pionraw")
    _edit_header(good, bad["key"], gamma_line, "\n" * len(gamma_line))
    bad["short"] = str(tmp_path / "short.pionraw")
    open(bad["short"], "wb").write(raw[:-8])
    lo, hi = str(tmp_path / "lo.pionraw"), str(tmp_path / "hi.pionraw")
    _edit_header(good, lo, "pion_slab_n 12\n", "pion_slab_n 05\n")
    _edit_header(good, hi, "pion_slab_lo 0\npion_slab_n 12\n", "pion_slab_lo 7\npion_slab_n 05\n")
    texts = {"magic": "magic", "key": "Gamma", "short": "truncated"}
    with orc_loop(cfg, setup) as s:
        s.init(P)
        for k, f in bad.items():
            with pytest.raises(RuntimeError, match=texts[k]):
                s.restart(f)
        with pytest.raises(RuntimeError, match="plane [56] .* none of the files"):
            s.restart([lo, hi])   # planes 5 and 6 are in neither
        with pytest.raises(RuntimeError, match="cannot open"):
            s.restart(str(tmp_path / "absent.pionraw"))
        with pytest.raises(ValueError, match="magic"):
            host_rccl.read_snapshot_header(bad["magic"])
        # the process lives and the sim still restarts from the good file
        s.restart(good)
        assert np.array_equal(s.download(0), want)
    cfg2, P2, setup2 = case("glm3d")
    with orc_loop(cfg2, setup2) as s:
        s.init(P2)
        with pytest.raises(RuntimeError, match="NGrid"):
            s.restart(good)


def test_set_output_and_slab_extent_refuse_bad_arguments(tmp_path):
    cfg, P, setup = case("hd3d")
    with orc_loop(cfg, setup) as s:
        s.init(P)
        for kw in (dict(op_criterion=2), dict(op_criterion=-1), dict(op_criterion=1, opfreq_time=0.0),
                   dict(op_criterion=1, opfreq_time=-1.0)):
            with pytest.raises(ValueError):
                s.set_output(str(tmp_path / "x"), **kw)
        assert s.lib.pion_host_sim_set_output(s.s, None, 0, 1, 0.0, 0) == abi.E_INVAL
        with pytest.raises(ValueError):
            s.set_slab_extent(cfg.ng[2] - 1, 0, abi.BC_REFLECTING, abi.BC_OUTFLOW)   # the slab does not fit
        with pytest.raises(ValueError):
            s.set_slab_extent(cfg.ng[2], 0, abi.BC_SLAB, abi.BC_OUTFLOW)


# ---- M ranks write, N ranks restart -----------------------------------------------------------------------------

def _rank_worker(rank, world, name, case_name, mode, paths, nsteps, q):
    """mode "write": init, nsteps, write paths[rank]; mode "restart": restart from paths, nsteps; puts P on the queue"""
    try:
        os.environ["PION_NO_TORCH"] = "1"
        for p in (ROOT, os.path.join(ROOT, "tests")):
            if p not in sys.path:
                sys.path.insert(0, p)
        cfg_g, P, setup = case(case_name)
        cfg = slab.slab_config(cfg_g, rank, world)
        ax = slab.slab_axis(cfg_g)
        with OrcLoop(cfg, setup, rank=rank, world=world, periodic_z=slab.slab_periodic(cfg_g), shm_name=name) as s:
            s.set_slab_extent(cfg_g.ng[ax], rank * cfg.ng[ax], cfg_g.bc_type[2 * ax], cfg_g.bc_type[2 * ax + 1])
            if mode == "write":
                s.init(slab.slab_slice(P, cfg_g, rank, world))
                s.time_int(nsteps)
                s.write_snapshot(paths[rank])
            else:
                s.restart(paths)
                s.time_int(nsteps)
            q.put((rank, s.get_time(), s.download(0)))
    except Exception as e:   # noqa: BLE001
        q.put((rank, None, repr(e)))


def run_ranks(world, case_name, mode, paths, nsteps):
    import multiprocessing as mp
    import time
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    name = "/pion_s%d_%d" % (os.getpid(), time.time_ns() % 1000000007)
    procs = [ctx.Process(target=_rank_worker, args=(r, world, name, case_name, mode, paths, nsteps, q))
             for r in range(world)]
    for p in procs:
        p.start()
    res = {}
    for _ in range(world):
        r, t, A = q.get(timeout=300)
        assert t is not None, A
        res[r] = (t, A)
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    return res


def assemble(res, cfg_g, world):
    """the ranks' on-grid cells as one global on-grid array"""
    nb, ax = cfg_g.nbc, slab.slab_axis(cfg_g)
    parts = []
    for r in range(world):
        A = res[r][1]
        parts.append(A[:, nb:-nb, nb:-nb, nb:-nb] if ax == 2 else A[:, :, nb:-nb, nb:-nb])
    return np.concatenate(parts, axis=1 if ax == 2 else 2)


def ongrid(A, cfg):
    nb = cfg.nbc
    return A[:, nb:-nb, nb:-nb, nb:-nb] if cfg.ndim == 3 else A[:, :, nb:-nb, nb:-nb]


def test_two_ranks_write_one_and_three_ranks_restart(tmp_path):
    name = "glm3d_z12"
    cfg, P, setup = case(name)
    with orc_loop(cfg, setup) as s:
        s.init(P)
        steps = run_steps(s, 5)
        ref = ongrid(s.download(0), cfg)
    paths = [str(tmp_path / ("w2_%d.pionraw" % r)) for r in range(2)]
    res = run_ranks(2, name, "write", paths, 2)
    assert res[0][0]["simtime"] == steps[1][1]
    infos = [host_rccl.read_snapshot_header(p)[1] for p in paths]
    assert [(i["rank"], i["world"], i["slab_lo"], i["slab_n"]) for i in infos] == [(0, 2, 0, 6), (1, 2, 6, 6)]
    for p in paths:   # the header is the global problem's
        g = host_rccl.read_snapshot_header(p)[0]
        assert list(g.ng) == list(cfg.ng) and list(g.bc_type) == list(cfg.bc_type) and list(g.xmin) == list(cfg.xmin)
    with orc_loop(cfg, setup) as s:
        s.restart(paths[::-1])
        got = run_steps(s, 3)
        assert got == steps[2:]
        assert np.array_equal(ongrid(s.download(0), cfg), ref)
    res3 = run_ranks(3, name, "restart", paths, 3)
    for r in range(3):
        assert res3[r][0]["simtime"] == steps[-1][1] and res3[r][0]["timestep"] == 5
    assert np.array_equal(assemble(res3, cfg, 3), ref)


def test_two_y_slabs_written_one_domain_restarts_2d(tmp_path):
    """2-D Cartesian, cut along y: the two slabs' files (each slab a sim of its own holding its rows of the step-2
    state -- the oracle's table has no 2-D halo, so the slabs do not step here; tests/test_gpu_host_snapshot.py runs
    ranks) restart the single domain"""
    name = "cart2d"
    cfg, P, setup = case(name)
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
            paths.append(str(tmp_path / ("y%d.pionraw" % r)))
            s.write_snapshot(paths[-1])
    with orc_loop(cfg, setup) as s:
        s.restart(paths)
        assert run_steps(s, 3) == steps[2:]
        assert np.array_equal(s.download(0), ref)


def test_slab_without_extent_refuses_to_write(tmp_path):
    cfg, P, setup = case("glm3d_z12")
    c = slab.slab_config(cfg, 0, 2)
    with orc_loop(c, setup) as s:
        s.init(slab.slab_slice(P, cfg, 0, 2))
        with pytest.raises(RuntimeError, match="set_slab_extent"):
            s.write_snapshot(str(tmp_path / "x.pionraw"))
    assert os.listdir(tmp_path) == []
