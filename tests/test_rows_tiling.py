"""Launch geometry of the stage kernel k_stage_rows2 on the host (no GPU): the decode of workgroups, wavefronts and
lanes into columns, rows and planes (pion_amd/csrc/rows_tiling.h), run for every workgroup of the launch grid by
tests/native/libtiling_probe.so, must write every on-grid cell of the launched planes exactly once and form no cell
index outside the arrays -- at every x-tile, row-group and plane-chunk edge, for the launch plans the host picks."""
import glob
import os
import re

import numpy as np
import pytest

import tiling_probe as tp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RNG_SEED = 20261016


def _even(nz, zchunk):
    return dict(kz0=0, kz1=nz, zchunk=zchunk, nzb=0, zcmax=zchunk)


def _uneven(nz, zcmax, zchunk=8):
    return dict(kz0=0, kz1=nz, zchunk=zchunk, nzb=tp.uneven_nzb(nz, zcmax), zcmax=zcmax)


# ---- the x tiling: every remainder, every R ----

def test_x_remainders_cover_every_cell_2d():
    """every nx 1..200 (rem 0..61 several times) plus large ones, every R 1..8 and several 2-D R up to 64"""
    rng = np.random.default_rng(RNG_SEED)
    for nx in list(range(1, 201)) + [248, 256, 310, 512, 1000, 2048, 4096]:
        for R in list(range(1, 9)) + [int(rng.integers(9, 65)), 64]:
            ny = int(rng.integers(1, 41))
            tp.check_launches(2, nx, ny, 1, 2, [dict(rows=R, kz0=0, kz1=1, zchunk=1)], xwrap=(nx >= 4))


def test_rows_and_planes_cover_every_cell_3d():
    """randomised nx x ny x nz x R x chunking over nx 1..200 (+ large), ny 1..40, nz 1..140, R 1..8"""
    rng = np.random.default_rng(RNG_SEED + 1)
    nxs = list(range(1, 201)) + [248, 256, 310, 512]
    for nx in nxs:
        for rep in range(3):
            ny = int(rng.integers(1, 41))
            nz = int(rng.integers(1, 141)) if nx <= 200 else int(rng.integers(1, 24))
            R = int(rng.integers(1, 9))
            mode = rep % 3
            if mode == 0:
                L = _even(nz, int(rng.integers(1, 33)))
            elif mode == 1:
                L = _uneven(nz, int(rng.integers(1, 33)))
            else:
                L = _uneven(nz, int(rng.integers(8, 33)), zchunk=int(rng.integers(1, 129)))
            tp.check_launches(3, nx, ny, nz, 2, [dict(rows=R, **L)], xwrap=(nx >= 4 and rep == 0))


@pytest.mark.parametrize("nx", [1000, 2048, 4096])
def test_wide_grids_3d(nx):
    for R in (1, 2, 3, 4, 8):
        tp.check_launches(3, nx, 7, 3, 2, [dict(rows=R, **_even(3, 2))])


def test_every_row_count_and_group_size_3d():
    """ny 1..40 plus a few larger ones against every R 1..8, at the x edges rem 0, 1, 30, 31, 61"""
    for nx in (62, 63, 92, 93, 61, 124):
        for ny in list(range(1, 41)) + [63, 64, 65, 127, 130]:
            for R in range(1, 9):
                tp.check_launches(3, nx, ny, 3, 2, [dict(rows=R, **_even(3, 2))])


def test_every_plane_count_and_chunking_3d():
    """nz 1..140 plus 256 and 512: equal chunks of 1..32 planes, uneven chunks with zcmax 1..32 (PION_ZCHUNK)"""
    for nz in list(range(1, 141)) + [256, 512]:
        for zc in ([1, 2, 3, 7, 8, 16, 31, 32] if nz > 140 else range(1, 33)):
            tp.check_launches(3, 5, 3, nz, 2, [dict(rows=2, **_even(nz, zc))])
            tp.check_launches(3, 5, 3, nz, 2, [dict(rows=2, **_uneven(nz, zc))])


def test_split_stage_parts_3d():
    """the split stage: interior [nb, nz - nb) in one launch, both z-boundary strips in another (kz2 / kz3)"""
    rng = np.random.default_rng(RNG_SEED + 2)
    for nz in list(range(4, 141, 3)) + [256]:
        for rep in range(2):
            nx, ny, R, nb = int(rng.integers(1, 130)), int(rng.integers(1, 30)), int(rng.integers(1, 9)), 2
            zc = int(rng.integers(1, 33))
            inner = dict(rows=R, kz0=nb, kz1=nz - nb, zchunk=zc, nzb=tp.uneven_nzb(nz - 2 * nb, zc) if rep else 0,
                         zcmax=zc)
            strips = dict(rows=R, kz0=0, kz1=nb, kz2=nz - nb, kz3=nz, zchunk=zc, nzb=0, zcmax=zc)
            tp.check_launches(3, nx, ny, nz, nb, [inner, strips], xwrap=(nx >= 4))
            strips_uneven = dict(strips, zchunk=int(rng.integers(1, 5)))
            tp.check_launches(3, nx, ny, nz, nb, [inner, strips_uneven])


# ---- the chunk rule and the XCD decode ----

def test_zchunk_bounds_partitions_every_strip():
    for np_ in range(1, 1025):
        for cmax in range(1, 129):
            n, ch = tp.zchunks(np_, cmax)
            assert n >= 1, (np_, cmax)
            assert ch[0][0] == 0 and ch[n - 1][1] == np_, (np_, cmax, ch)
            for c in range(n):
                assert ch[c][1] > ch[c][0], ("empty chunk", np_, cmax, c, ch)
                if c:
                    assert ch[c][0] == ch[c - 1][1], ("gap or overlap", np_, cmax, c, ch)
            assert ch[n] == (np_, np_), ("a chunk past the end must be empty at np", np_, cmax, ch[n])


def test_xcd_tile_is_one_to_one():
    for n in list(range(1, 600)) + [1023, 1024, 1025, 4097, 65537]:
        nb = 8 * ((n + 7) // 8)
        t = tp.xcd_table(nb, n)
        assert len(np.unique(t)) == nb, n
        assert t.min() == 0 and t.max() == nb - 1, n
        assert set(range(n)) <= set(t.tolist()), n


# ---- the plans the launcher picks ----

def _stage_launches(ndim, ng, nv, euler, second_order, split=False, ncu=256, wg_per_cu=2, **want):
    nx, ny, nz = ng
    nb = 2
    parts = [(nb, nz - nb, 0, 0), (0, nb, nz - nb, nz)] if split else [(0, nz, 0, 0)]
    out = []
    for kz0, kz1, kz2, kz3 in parts:
        p = tp.plan(ndim, nx, ny, kz1 - kz0, nv, euler, second_order, ncu=ncu, **want)
        R = tp.launch_rows(p, ndim, nx, ny, nv, second_order, wg_per_cu=wg_per_cu, ncu=ncu,
                           zslope_lds=want.get("zslope_lds", True))
        out.append(dict(rows=R, kz0=kz0, kz1=kz1, kz2=kz2, kz3=kz3, zchunk=p["zchunk"], nzb=p["nzb"], zcmax=p["zcmax"]))
    return out


PRODUCTION = [
    # (name, ndim, ng, nv, euler, split)
    ("m1_glm_512", 3, [512, 512, 512], 9, False, False),
    ("m1_mhd_512", 3, [512, 512, 512], 8, False, False),
    ("m2_euler_512", 3, [512, 512, 512], 5, True, False),
    ("m2_euler_slab_512x512x64", 3, [512, 512, 64], 5, True, True),
    ("m3_euler_tr_256", 3, [256, 256, 256], 6, True, False),
    ("glm_slab_512x512x64", 3, [512, 512, 64], 9, False, True),
    ("euler_2d_4096x1260", 2, [4096, 1260, 1], 5, True, False),
    ("glm_2d_2048x630", 2, [2048, 630, 1], 9, False, False),
]


@pytest.mark.parametrize("name,ndim,ng,nv,euler,split", PRODUCTION, ids=[c[0] for c in PRODUCTION])
def test_production_plans_cover_every_cell(name, ndim, ng, nv, euler, split):
    for second_order in (False, True):
        for wg in ((2, 3) if ndim == 2 else (2,)):
            L = _stage_launches(ndim, ng, nv, euler, second_order, split=split, wg_per_cu=wg)
            tp.check_launches(ndim, ng[0], ng[1], ng[2], 2, L)


def test_production_plan_values():
    """pins what the plans above are (a retune shows up here, and the geometry tests still cover it)"""
    p = tp.plan(3, 512, 512, 512, 9, False, True)
    assert p["rows"] == tp.rmax_lds(9, True) and p["nzb"] > 1 and p["zcmax"] == 32, p
    p = tp.plan(3, 512, 512, 512, 5, True, True)
    assert p["rows"] >= 1 and p["nzb"] > 1, p
    p = tp.plan(3, 512, 512, 4, 9, False, True)
    assert p["nzb"] == 0, p             # strips of fewer than 16 planes: equal chunks
    p = tp.plan(2, 4096, 1260, 1, 5, True, True)
    assert p["rows_auto"] == 1 and p["nzb"] == 0, p
    assert tp.plan(3, 64, 64, 64, 9, False, True, want_rows=1)["rows"] == 1
    assert tp.plan(3, 64, 64, 64, 9, False, True, want_rows=3)["rows"] == tp.rmax_lds(9, True) == 2
    assert tp.plan(3, 64, 64, 64, 9, False, False, want_rows1=3)["rows"] == 3
    assert tp.plan(3, 64, 64, 64, 9, False, True, want_zchunk=5)["zcmax"] == 5
    assert tp.plan(3, 64, 64, 64, 9, False, True, uneven=False)["nzb"] == 0


# ---- the run-time switches have tests ----

def test_every_launch_switch_has_a_test():
    """every PION_* environment switch the library reads is exercised by a GPU test: listed in the knob table of
    tests/test_gpu_launch_geometry.py, or set by another test"""
    names = set()
    for f in glob.glob(os.path.join(ROOT, "pion_amd", "csrc", "*.hip")):
        names |= set(re.findall(r'getenv\("(PION_\w+)"\)', open(f).read()))
    assert "PION_ZCHUNK" in names and "PION_FUSE_DT" in names, names
    src = open(os.path.join(ROOT, "tests", "test_gpu_launch_geometry.py")).read()
    table = src[src.index("KNOBS = ["):src.index("]  # end of KNOBS")]
    others = ""
    for f in glob.glob(os.path.join(ROOT, "tests", "test_*.py")):
        if not f.endswith(("test_gpu_launch_geometry.py", "test_rows_tiling.py")):
            others += open(f).read()
    missing = [n for n in sorted(names)
               if '"%s"' % n not in table and not re.search(r'setenv\(\s*"%s"' % n, others)]
    assert not missing, "launch switches without a test: %s" % missing
