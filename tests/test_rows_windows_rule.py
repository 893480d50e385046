"""The plane-window planner of the rows kernel (rows_tiling.h "plane windows") through pion_gpu_rows_windows: host
only, no GPU.

A launch of k_stage_rows2 reaches fewer than L cells of an array from the array's base (L = 2^29: 32-bit byte offsets
of doubles).  One that updates n planes of the slab axis touches n + 2 nbc planes of s cells each, so
W = floor((L - 1) / s) - 2 nbc planes fit in one window, and a range [lo, hi) takes ceil((hi - lo) / W) windows -- the
least any plan can do, since no window may hold more than W planes."""
import ctypes as C

import numpy as np
import pytest

from pion_amd import abi, lib

L0 = 1 << 29


def _cfg(ng, nbc=2, coord_sys=1):
    ndim = len(ng)
    return abi.make_config(ndim, list(ng), abi.EQEUL, abi.FLUX_RSroe, dx=1.0, nbc=nbc, coord_sys=coord_sys,
                           bcs=["outflow"] * (2 * ndim), refvec=[1.0] * 5)


def _stride(cfg):
    s = cfg.ng[0] + 2 * cfg.nbc
    return s * (cfg.ng[1] + 2 * cfg.nbc) if cfg.ndim == 3 else s


def _raw(cfg, limit, lo, hi, maxw, w_lo=None, w_hi=None):
    return lib.load_library().pion_gpu_rows_windows(C.byref(cfg) if cfg is not None else None, limit, lo, hi, maxw,
                                                    w_lo, w_hi)


def _check(cfg, lo, hi, L):
    """every property of the plan of [lo, hi) under the limit L; returns the windows"""
    s, nbc = _stride(cfg), cfg.nbc
    W = (L - 1) // s - 2 * nbc
    wins = lib.rows_windows(cfg, lo, hi, limit=L)
    if W < 1:
        assert wins == [], (s, nbc, lo, hi, L, wins)
        return wins
    n = hi - lo
    assert len(wins) == -(-n // W), (s, nbc, lo, hi, L, wins)
    # in order, no gap, no overlap
    assert wins[0][0] == lo and wins[-1][1] == hi
    for (a0, a1), (b0, b1) in zip(wins, wins[1:]):
        assert a1 == b0
    sizes = [b - a for a, b in wins]
    assert min(sizes) >= 1
    for m in sizes:
        assert (m + 2 * nbc) * s < L
    # balanced within one plane, longer ones first
    assert max(sizes) - min(sizes) <= 1 and sizes == sorted(sizes, reverse=True)
    if n <= W:
        assert wins == [(lo, hi)]
    return wins


def test_random_plans():
    rng = np.random.default_rng(20261018)
    for _ in range(400):
        ndim = int(rng.integers(2, 4))
        nbc = int(rng.integers(2, 4))
        ng = [int(rng.integers(1, 40)) for _ in range(ndim)]
        ng[-1] = int(rng.integers(1, 300))
        cfg = _cfg(ng, nbc)
        s = _stride(cfg)
        lo = int(rng.integers(0, ng[-1]))
        hi = int(rng.integers(lo + 1, ng[-1] + 1))
        # limits from "not one plane" through "a few planes" to "everything"
        planes = int(rng.integers(2 * nbc - 1, ng[-1] + 2 * nbc + 3))
        L = planes * s + int(rng.integers(0, s + 1))
        _check(cfg, lo, hi, L)


def test_edges_of_the_rule():
    cfg = _cfg([6, 5, 23])
    s, nbc, nz = _stride(cfg), 2, 23
    # W planes exactly: L - 1 = (W + 2 nbc) s; one cell less and the window loses a plane
    for W in (1, 2, 3, 11, 22, 23, 24):
        L = (W + 2 * nbc) * s + 1
        wins = _check(cfg, 0, nz, L)
        assert max(b - a for a, b in wins) <= W
        assert len(wins) == -(-nz // W)
        if W > 1:
            assert len(_check(cfg, 0, nz, L - 1)) == -(-nz // (W - 1))
    # one plane with its ghost planes does not fit: not admitted
    assert lib.rows_windows(cfg, 0, nz, limit=(1 + 2 * nbc) * s) == []
    assert _raw(cfg, (1 + 2 * nbc) * s, 0, nz, 0) == 0
    # a range that fits is the range itself, wherever it lies
    L = (5 + 2 * nbc) * s + 1
    assert lib.rows_windows(cfg, 9, 14, limit=L) == [(9, 14)]
    assert lib.rows_windows(cfg, 9, 15, limit=L) == [(9, 12), (12, 15)]
    assert lib.rows_windows(cfg, 0, 23, limit=L) == [(0, 5), (5, 10), (10, 15), (15, 19), (19, 23)]
    # the whole grid by default, the default limit for limit <= 0
    assert lib.rows_windows(cfg) == [(0, 23)]
    assert _raw(cfg, 0, 0, nz, 0) == 1 and _raw(cfg, -5, 0, nz, 0) == 1
    # max_windows truncates what is written, not what is returned
    w_lo, w_hi = (C.c_int * 2)(), (C.c_int * 2)()
    assert _raw(cfg, L, 0, 23, 2, w_lo, w_hi) == 5
    assert (list(w_lo), list(w_hi)) == ([0, 5], [5, 10])


def test_real_shapes():
    # s = 1028^2: floor((2^29 - 1) / s) = 508, W = 504
    wins = _check(_cfg([1024, 1024, 1024]), 0, 1024, L0)
    assert wins == lib.rows_windows(_cfg([1024, 1024, 1024])) and len(wins) == 3
    assert [b - a for a, b in wins] == [342, 341, 341]
    assert lib.rows_windows(_cfg([808, 808, 808])) == [(0, 808)]
    assert len(lib.rows_windows(_cfg([809, 809, 809]))) == 2
    assert lib.rows_windows(_cfg([32768, 16384])) == [(0, 8192), (8192, 16384)]
    assert lib.rows_windows(_cfg([32768, 16384], coord_sys=2)) == [(0, 8192), (8192, 16384)]   # cylindrical (z,R)
    # one 12004 x 12004 plane with its four ghost planes: 7.2e8 cells
    assert lib.rows_windows(_cfg([12000, 12000, 64])) == []
    # eight ranks of a 1600^3 grid: a slab of 200 planes fits, one of 1664^3 / 8 does not
    assert len(lib.rows_windows(_cfg([1600, 1600, 200]))) == 1
    assert len(lib.rows_windows(_cfg([1664, 1664, 208]))) == 2


def test_grids_the_rows_kernel_does_not_take():
    assert lib.rows_windows(_cfg([64])) == []                      # 1-D
    assert lib.rows_windows(_cfg([16, 16, 16], nbc=1)) == []       # one ghost layer
    c = abi.make_config(1, [32], abi.EQEUL, abi.FLUX_RSroe, dx=1.0, coord_sys=3, bcs=["reflecting", "outflow"],
                        refvec=[1.0] * 5)
    assert lib.rows_windows(c) == []                               # spherical


def test_bad_arguments():
    cfg = _cfg([8, 8, 8])
    w = (C.c_int * 4)()
    assert _raw(None, 0, 0, 8, 0) == abi.E_INVAL
    assert _raw(cfg, 0, -1, 8, 0) == abi.E_INVAL
    assert _raw(cfg, 0, 0, 9, 0) == abi.E_INVAL
    assert _raw(cfg, 0, 4, 4, 0) == abi.E_INVAL
    assert _raw(cfg, 0, 5, 4, 0) == abi.E_INVAL
    assert _raw(cfg, 0, 0, 8, -1) == abi.E_INVAL
    assert _raw(cfg, 0, 0, 8, 4, None, w) == abi.E_INVAL
    assert _raw(cfg, 0, 0, 8, 4, w, None) == abi.E_INVAL
    assert _raw(cfg, L0 + 1, 0, 8, 0) == abi.E_INVAL               # more than a 32-bit byte offset reaches
    assert _raw(cfg, L0, 0, 8, 0) == 1
    bad = _cfg([8, 8, 8])
    bad.ndim = 4
    assert _raw(bad, 0, 0, 8, 0) == abi.E_INVAL
    bad = _cfg([8, 8, 8])
    bad.ng[1] = 0
    assert _raw(bad, 0, 0, 8, 0) == abi.E_INVAL
    with pytest.raises(lib.PionGpuError):
        lib.rows_windows(cfg, 3, 3)
