"""What the FITS tests share: a numpy restatement of the images the reference's FITS writer produces, a FITS parser of
a few lines that owes nothing to pion_amd/fits.py (so a writer bug and a reader bug cannot cancel), and the rank
worker of the two-rank tests.  Not a test module.

The restatement, expression by expression (reference lines; none of its text is copied):
  image list   dataIO/dataio_fits.cpp:147-320: the primitive variables, the tracers TR0.., then Eint without a
               microphysics object or Temp with one (EP.cooling != 0), then for MHD and GLM divB and Ptot
  Eint         p/(gamma-1)/rho                                  eqns_hydro_adiabatic.cpp:374-380, eqns_mhd_adiabatic.cpp:445-451
  Temp         p*Mu_tot_over_kB/rho, Mu_tot = 0.609 m_p         mp_only_cooling.cpp:274-280, :81-95; constants.h:53,64
  Ptot         p + 0.5*(Bx*Bx + By*By + Bz*Bz)                  eqns_mhd_adiabatic.cpp:474-480
  divB         Cartesian: 0.0 + sum_v (B_v[+1] - B_v[-1])/(2.0*dx)                                 VectorOps.cpp:377-439
               (z,R): (Bz[+z] - Bz[-z])/(2.0*dx) + 2.0*(rp*B_R[+R] - rn*B_R[-R])/(rp*rp - rn*rn)   VectorOps.cpp:891-965
               with rn, rp = R + dR*dR/12./R of the neighbours (VectorOps.h:414-418), R = xmin + (2 j + 1)*(dx/2)
               (cell_interface.cpp:506-512)
  B, divB      times sqrt(4.0*M_PI) (NEW_B_NORM, defines/functionality_flags.h:42); psi and Ptot are not scaled
numpy evaluates each of these element by element in IEEE double without contraction, in the order written."""
import os
import sys

import numpy as np

from pion_amd import abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BLOCK, CARD = 2880, 80
BSCALE = np.sqrt(4.0 * np.pi)
M_P, K_B = 1.672621898e-24, 1.38064852e-16
MU_TOT_OVER_KB = (0.609 * M_P) / K_B


def image_names(cfg):
    names = ["GasDens", "GasPres", "GasVX", "GasVY", "GasVZ"]
    if cfg.eqntype in (abi.EQMHD, abi.EQGLM):
        names += ["Bx", "By", "Bz"]
    if cfg.eqntype == abi.EQGLM:
        names += ["psi"]
    names += ["TR%d" % t for t in range(cfg.ntracer)]
    names += ["Temp" if cfg.cooling != 0 else "Eint"]
    if cfg.eqntype in (abi.EQMHD, abi.EQGLM):
        names += ["divB", "Ptot"]
    return names


def _shift(A, cfg, axis, d):
    """on-grid view of variable array A [nz_all][ny_all][nx_all] displaced by d cells along axis (0 = x)"""
    nb = cfg.nbc
    sl = []
    for a in (2, 1, 0):   # array axes z, y, x
        if a >= cfg.ndim:
            sl.append(slice(None))
        else:
            o = d if a == axis else 0
            sl.append(slice(nb + o, nb + o + cfg.ng[a]))
    return A[tuple(sl)]


def restate(cfg, A):
    """[(name, image)] from a whole array with ghosts A [nvar][nz_all][ny_all][nx_all]; image: on-grid cells,
    [nz][ny][nx] with the axes the grid lacks kept at length 1"""
    og = lambda X: _shift(X, cfg, -1, 0)
    mhd = cfg.eqntype in (abi.EQMHD, abi.EQGLM)
    names = image_names(cfg)
    out = []
    for v in range(cfg.nvar):
        img = og(A[v])
        if mhd and abi.BX <= v <= abi.BZ:
            img = img * BSCALE
        out.append((names[v], np.array(img)))
    rho, p = og(A[abi.RO]), og(A[abi.PG])
    if cfg.cooling != 0:
        out.append(("Temp", p * MU_TOT_OVER_KB / rho))
    else:
        out.append(("Eint", p / (cfg.gamma - 1.0) / rho))
    if mhd:
        dx = cfg.dx
        if cfg.coord_sys == 2:
            div = (_shift(A[abi.BX], cfg, 0, +1) - _shift(A[abi.BX], cfg, 0, -1)) / (2.0 * dx)
            j = np.arange(cfg.ng[1])
            Rn = cfg.xmin[1] + (2 * (j - 1) + 1) * (0.5 * dx)
            Rp = cfg.xmin[1] + (2 * (j + 1) + 1) * (0.5 * dx)
            rn = (Rn + dx * dx / 12. / Rn)[None, :, None]
            rp = (Rp + dx * dx / 12. / Rp)[None, :, None]
            div = div + 2.0 * (rp * _shift(A[abi.BY], cfg, 1, +1) - rn * _shift(A[abi.BY], cfg, 1, -1)) / (rp * rp - rn * rn)
        else:
            div = np.zeros(rho.shape)
            for ax in range(cfg.ndim):
                div = div + (_shift(A[abi.BX + ax], cfg, ax, +1) - _shift(A[abi.BX + ax], cfg, ax, -1)) / (2.0 * dx)
        out.append(("divB", div * BSCALE))
        bx, by, bz = og(A[abi.BX]), og(A[abi.BY]), og(A[abi.BZ])
        out.append(("Ptot", p + 0.5 * (bx * bx + by * by + bz * bz)))
    return out


def same_bits(a, b):
    """== on the 8 bytes of every element, NaNs by bit pattern"""
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def squeeze(img, cfg):
    """[nz][ny][nx] with unit axes -> the file's [NAXISn..1] shape"""
    return img.reshape([cfg.ng[a] for a in range(cfg.ndim)][::-1])


def parse(path):
    """(primary cards, [(extension cards, big-endian data bytes as float64 array)], notes): checks the block
    structure on the way.  cards: list of the 80-character strings up to and including END."""
    raw = open(path, "rb").read()
    assert len(raw) % BLOCK == 0, "length %d is no multiple of 2880" % len(raw)
    pos, hdus = 0, []
    while pos < len(raw):
        cards, end = [], False
        while not end:
            block = raw[pos:pos + BLOCK]
            assert len(block) == BLOCK, "header without END"
            pos += BLOCK
            for i in range(0, BLOCK, CARD):
                c = block[i:i + CARD]
                assert all(32 <= ch <= 126 for ch in c), "card with a non-printable byte: %r" % c
                c = c.decode("ascii")
                if end:
                    assert c == " " * CARD, "header padding after END is not blank"
                else:
                    cards.append(c)
                    end = (c == "END" + " " * 77)
        kv = {c[:8].strip(): c[10:30].strip() for c in cards if c[8:10] == "= "}
        n = 0
        if int(kv["NAXIS"]) > 0:
            n = 8
            for a in range(int(kv["NAXIS"])):
                n *= int(kv["NAXIS%d" % (a + 1)])
        data = np.frombuffer(raw, dtype=">f8", count=n // 8, offset=pos).astype("=f8")
        padded = (n + BLOCK - 1) // BLOCK * BLOCK
        assert raw[pos + n:pos + padded] == b"\0" * (padded - n), "data padding is not zero bytes"
        pos += padded
        hdus.append((cards, data))
    assert pos == len(raw)
    return hdus


def images_of(path):
    """{EXTNAME: array shaped [NAXISn..1]}, in file order, through parse()"""
    out = {}
    for cards, data in parse(path)[1:]:
        kv = {c[:8].strip(): c[10:].strip() for c in cards if c[8:10] == "= "}
        shape = [int(kv["NAXIS%d" % (a + 1)]) for a in range(int(kv["NAXIS"]))][::-1]
        out[kv["EXTNAME"].strip("'").strip()] = data.reshape(shape)
    return out


# ---- a rank of a two-rank run writing its FITS file (spawned; module-level so that the child can import it) ---------

def two_rank_case(name):
    from pion_amd import problems
    if name == "glm3d_z12":
        return problems.mhd_blast_generic([20, 12, 12], strict_fp=1)
    if name == "glm2d_y12":
        return problems.mhd_blast_generic([16, 12], strict_fp=1)
    raise KeyError(name)


def rank_worker(rank, world, shm, case_name, backend, nsteps, path, q):
    """backend "orc": the oracle-bound loop (CPU); "gpu": the product's loop on device 0"""
    try:
        if backend == "orc":
            os.environ["PION_NO_TORCH"] = "1"
        for p in (ROOT, os.path.join(ROOT, "tests")):
            if p not in sys.path:
                sys.path.insert(0, p)
        from pion_amd import host_rccl, slab
        cfg_g, P = two_rank_case(case_name)
        cfg = slab.slab_config(cfg_g, rank, world)
        ax = slab.slab_axis(cfg_g)
        kw = dict(rank=rank, world=world, periodic_z=slab.slab_periodic(cfg_g), shm_name=shm)
        if backend == "orc":
            from test_host_snapshot import OrcLoop
            loop = OrcLoop(cfg, lambda sim, c: None, **kw)
        else:
            loop = host_rccl.HostSim(cfg, 0, **kw)
        with loop as s:
            s.set_slab_extent(cfg_g.ng[ax], rank * cfg.ng[ax], cfg_g.bc_type[2 * ax], cfg_g.bc_type[2 * ax + 1])
            s.init(slab.slab_slice(P, cfg_g, rank, world))
            s.time_int(nsteps)
            s.write_fits(path)
            q.put((rank, s.get_time(), None))
    except Exception as e:   # noqa: BLE001
        q.put((rank, None, repr(e)))


def run_two_ranks(case_name, backend, nsteps, paths):
    import multiprocessing as mp
    import time
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    shm = "/pion_f%d_%d" % (os.getpid(), time.time_ns() % 1000000007)
    procs = [ctx.Process(target=rank_worker, args=(r, 2, shm, case_name, backend, nsteps, paths[r], q)) for r in range(2)]
    for p in procs:
        p.start()
    times = {}
    try:
        for _ in range(2):
            r, t, msg = q.get(timeout=300)
            assert t is not None, msg
            times[r] = t
    finally:
        for p in procs:
            p.join(timeout=120)
            if p.is_alive():
                p.kill()
    assert all(p.exitcode == 0 for p in procs)
    return times
