"""ctypes access to tests/native/libtiling_probe.so: the launch geometry of the stage kernel k_stage_rows2
(pion_amd/csrc/rows_tiling.h) run on the host.  Shared by tests/test_rows_tiling.py (exhaustive coverage, CPU) and
tests/test_gpu_launch_geometry.py (the plan each GPU case runs with)."""
import ctypes
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NATIVE = os.path.join(ROOT, "tests", "native")
SO = os.path.join(NATIVE, "libtiling_probe.so")

ST_NBLOCKS, ST_WAVES, ST_CMIN, ST_CMAX, ST_IXMIN, ST_IXMAX, ST_YMIN, ST_YMAX, ST_KMIN, ST_KMAX, ST_NCELL, \
    ST_BADWRITE, ST_BADLANE = range(13)
NV = {"euler": 5, "mhd": 8, "glm": 9}

_lib = None


def lib():
    """the probe library, built on demand (seconds)"""
    global _lib
    if _lib is None:
        src = os.path.join(NATIVE, "tiling_probe.cpp")
        hdr = os.path.join(ROOT, "pion_amd", "csrc", "rows_tiling.h")
        if not os.path.exists(SO) or os.path.getmtime(SO) < max(os.path.getmtime(src), os.path.getmtime(hdr)):
            subprocess.check_call(["make", "-C", NATIVE, "libtiling_probe.so"])
        L = ctypes.CDLL(SO)
        i, p, lp = ctypes.c_int, ctypes.c_void_p, ctypes.c_long
        L.tp_probe.argtypes = [i] * 14 + [p, p, p]
        L.tp_probe.restype = i
        L.tp_tiling.argtypes = [i, i, i, p]
        L.tp_decode.argtypes = [i] * 11 + [ctypes.c_uint, i, i, p]
        L.tp_zchunk_table.argtypes = [i, i, i, p, p]
        L.tp_zchunk_table.restype = i
        L.tp_xcd_table.argtypes = [lp, lp, p]
        L.tp_rmax_lds.argtypes = [i, i]
        L.tp_rmax_lds.restype = i
        L.tp_pick_rows_2d.argtypes = [i] * 5
        L.tp_pick_rows_2d.restype = i
        L.tp_plan.argtypes = [i] * 14 + [p]
        _lib = L
    return _lib


def tiling(nx, ny, rows):
    """dict of rows_tiling_of: ntx_full, rem, spw, nyg, nfull, nrem, per_chunk"""
    o = np.zeros(7, np.int32)
    lib().tp_tiling(nx, ny, rows, o.ctypes.data)
    return dict(zip(["ntx_full", "rem", "spw", "nyg", "nfull", "nrem", "per_chunk"], (int(v) for v in o)))


def zchunks(np_, cmax):
    """(number of chunks zchunk_bounds reports, [(k0, k1)] for cz = 0 .. that number, one past the end included)"""
    n_max = np_ + 2
    k0, k1 = np.zeros(n_max, np.int32), np.zeros(n_max, np.int32)
    n = lib().tp_zchunk_table(np_, cmax, n_max, k0.ctypes.data, k1.ctypes.data)
    return n, list(zip(k0[:n + 1].tolist(), k1[:n + 1].tolist()))


def xcd_table(nb, ntiles):
    out = np.zeros(nb, np.int64)
    lib().tp_xcd_table(nb, ntiles, out.ctypes.data)
    return out


def rmax_lds(nv, zsl):
    return lib().tp_rmax_lds(nv, int(zsl))


def plan(ndim, nx, ny, np_, nv, euler, second_order, ncu=256, zslope_lds=True, uneven=True, want_rows=0,
         want_rows1=0, want_zchunk=0, march=True):
    """rows2_plan: dict rows, rows_auto, zchunk, zcmax, nzb"""
    o = np.zeros(5, np.int32)
    lib().tp_plan(ndim, nx, ny, np_, ncu, nv, int(euler), int(march), int(zslope_lds), int(second_order), int(uneven),
                  want_rows, want_rows1, want_zchunk, o.ctypes.data)
    return dict(zip(["rows", "rows_auto", "zchunk", "zcmax", "nzb"], (int(v) for v in o)))


def launch_rows(p, ndim, nx, ny, nv, second_order, zslope_lds=True, wg_per_cu=2, ncu=256):
    """the rows a launch of the plan p runs with (stage_rows2.h rows2_launch: the 2-D refinement, the LDS clamp)"""
    rows = p["rows"]
    if ndim == 2 and p["rows_auto"]:
        rows = lib().tp_pick_rows_2d(nx, ny, rows, wg_per_cu, ncu)
    rmax = 64 if ndim == 2 else rmax_lds(nv, zslope_lds and second_order)
    return max(1, min(rows, rmax))


def probe(ndim, nx, ny, nz, nbc, rows, kz0, kz1, kz2=0, kz3=0, zchunk=8, nzb=0, zcmax=32, xwrap=False, count=None):
    """run one launch's decode on the host; returns (count [nz, ny, nx] uint8, ghost [2, nz, ny, nbc] uint8, stats).
    `count` may be passed in to accumulate several launches."""
    if count is None:
        count = np.zeros((nz, ny, nx), np.uint8)
    ghost = np.zeros((2, nz, ny, nbc), np.uint8)
    stats = np.zeros(16, np.int64)
    rc = lib().tp_probe(ndim, nx, ny, nz, nbc, rows, kz0, kz1, kz2, kz3, zchunk, nzb, zcmax, int(xwrap),
                        count.ctypes.data, ghost.ctypes.data, stats.ctypes.data)
    assert rc == 0, rc
    return count, ghost, stats


def first_bad(count, expect):
    """(x, y, z, count, expected) of the first cell whose write count is wrong, or None"""
    bad = np.argwhere(count != expect)
    if len(bad) == 0:
        return None
    z, y, x = (int(v) for v in bad[0])
    return "cell (x=%d, y=%d, z=%d) written %d times, expected %d (%d cells wrong)" % (
        x, y, z, count[z, y, x], expect[z, y, x], len(bad))


def check_launches(ndim, nx, ny, nz, nbc, launches, xwrap=False):
    """launches: list of probe kwargs (rows, kz0, kz1, kz2, kz3, zchunk, nzb, zcmax) that together make one stage.
    Asserts every on-grid cell is written exactly once, (xwrap) every x ghost image exactly once, and that every
    cell index a lane forms -- and its z neighbours -- lies in the array.  Returns the stats of the last launch."""
    count = np.zeros((nz, ny, nx), np.uint8)
    ghosts = np.zeros((2, nz, ny, nbc), np.uint8)
    sx = nx + 2 * nbc
    sz = sx * (ny + 2 * nbc) if ndim == 3 else 0
    desc = "ndim %d, %d x %d x %d, nbc %d, launches %s" % (ndim, nx, ny, nz, nbc, launches)
    for L in launches:
        _, g, st = probe(ndim, nx, ny, nz, nbc, xwrap=xwrap, count=count, **L)
        ghosts += g
        assert st[ST_BADWRITE] == 0, "%d writes outside the grid: %s" % (st[ST_BADWRITE], desc)
        assert st[ST_BADLANE] == 0, desc
        if st[ST_WAVES] == 0:
            continue
        assert 0 <= st[ST_CMIN] - sz and st[ST_CMAX] + sz < st[ST_NCELL], ("cell index out of the array", st[:11], desc)
        assert -1 <= st[ST_IXMIN] and st[ST_IXMAX] <= nx, ("column", st[ST_IXMIN], st[ST_IXMAX], desc)
        assert 0 <= st[ST_YMIN] and st[ST_YMAX] < ny, ("row", st[ST_YMIN], st[ST_YMAX], desc)
        klo = min(L["kz0"], L.get("kz2", 0) if L.get("kz3", 0) > L.get("kz2", 0) else L["kz0"])
        khi = max(L["kz1"], L.get("kz3", 0))
        assert klo - (1 if ndim == 3 else 0) <= st[ST_KMIN] and st[ST_KMAX] < khi, ("plane", st[ST_KMIN],
                                                                                       st[ST_KMAX], desc)
    expect = np.zeros_like(count)
    for L in launches:
        expect[L["kz0"]:L["kz1"]] += 1
        if L.get("kz3", 0) > L.get("kz2", 0):
            expect[L["kz2"]:L["kz3"]] += 1
    msg = first_bad(count, expect)
    assert msg is None, msg + ": " + desc
    if xwrap:
        gexp = np.broadcast_to(expect[None, :, :, :1], ghosts.shape)
        bad = np.argwhere(ghosts != gexp)
        assert len(bad) == 0, "x ghost image (side, z, y, g) = %s written %d times: %s" % (
            tuple(int(v) for v in bad[0]), ghosts[tuple(bad[0])], desc)
    return st


def uneven_nzb(np_, zcmax):
    """the number of uneven chunks the launcher uses for a strip of np_ planes (0: equal chunks)"""
    return zchunks(np_, zcmax)[0] if np_ >= 16 else 0
