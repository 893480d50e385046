"""The rule of the screened HLLD -> HLL switch prepass (pion_amd/csrc/hll_screen.h) against a numpy model of the dense
flags: every cell of every block the rule calls quiet is not "steep" on any axis, ghost cells included -- with no
exception -- and the rule is not vacuous (a smooth field has no active block, a planted jump activates only the
blocks within one block of it).  The header is compiled as plain host code into a probe library built here."""
import ctypes as C
import itertools
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NBC = 2
GRIDS = [(70, 9, 12), (130, 8, 8), (62, 4, 8), (63, 5, 17)]
# per axis: "p" periodic, "r" reflecting / outflow (both copy the first on-grid cell of the column)
FACES = ["ppp", "rrr", "prp", "rpr"]


@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    cxx = shutil.which(os.environ.get("CXX", "g++")) or shutil.which("c++") or shutil.which("clang++")
    if cxx is None:
        pytest.fail("no host C++ compiler")
    so = str(tmp_path_factory.mktemp("hll_screen") / "libhll_screen_probe.so")
    src = os.path.join(ROOT, "tests", "native", "hll_screen_probe.cpp")
    subprocess.check_call([cxx, "-O1", "-std=c++14", "-fPIC", "-shared", "-ffp-contract=off", "-o", so, src])
    lib = C.CDLL(so)
    ip = C.POINTER(C.c_int)
    lib.hs_geom.argtypes = [ip, C.c_int, ip, ip]
    lib.hs_ext.argtypes = [ip, C.c_int, ip, ip, ip, ip]
    lib.hs_screen.argtypes = [ip, C.c_int, ip, C.POINTER(C.c_double), C.c_void_p]
    lib.hs_key_less.argtypes = [C.c_double, C.c_double]
    lib.hs_key_roundtrip.argtypes = [C.c_double]
    lib.hs_key_roundtrip.restype = C.c_double
    return lib


def _ints(v):
    return (C.c_int * len(v))(*v)


def fill_ghosts(p, faces):
    """ghost cells of the all-cell array p[z, y, x] in the order X, Y, Z (each over the full extent of the axes before
    it): periodic copies ng cells back onto the grid, every other admitted type copies the first on-grid cell"""
    for d, f in enumerate(faces):
        ax = 2 - d
        n = p.shape[ax] - 2 * NBC
        q = np.moveaxis(p, ax, 0)
        for g in range(NBC):
            if f == "p":
                q[g] = q[g + n]
                q[NBC + n + g] = q[NBC + g]
            else:
                q[g] = q[NBC]
                q[NBC + n + g] = q[NBC + n - 1]


def steep_model(p):
    """the dense kernels' screen per cell: on some axis !(|p+ - p-| <= 1.6 p+) or !(|p+ - p-| <= 1.6 p-), the missing
    neighbour of a cell on a face of the array being the cell itself"""
    steep = np.zeros(p.shape, dtype=bool)
    with np.errstate(invalid="ignore"):
        for ax in range(3):
            q = np.moveaxis(p, ax, 0)
            pn = np.concatenate([q[:1], q[:-1]])
            pp = np.concatenate([q[1:], q[-1:]])
            d = np.abs(pp - pn)
            s = ~(d <= 1.6 * pp) | ~(d <= 1.6 * pn)
            steep |= np.moveaxis(s, 0, ax)
    return steep


def screen(probe, ng, faces, p):
    per = [1 if f == "p" else 0 for f in faces]
    nb = _ints([0, 0, 0])
    assert probe.hs_geom(_ints(ng), NBC, _ints(per), nb) == 1
    nb = list(nb)
    quiet = np.zeros(nb[0] * nb[1] * nb[2], dtype=np.uint8)
    pc = np.ascontiguousarray(p, dtype=np.float64)
    probe.hs_screen(_ints(ng), NBC, _ints(per), pc.ctypes.data_as(C.POINTER(C.c_double)), quiet.ctypes.data)
    return nb, quiet.reshape(nb[2], nb[1], nb[0]).astype(bool)


def ext_box(probe, ng, faces, b):
    per = [1 if f == "p" else 0 for f in faces]
    lo, hi = _ints([0, 0, 0]), _ints([0, 0, 0])
    probe.hs_ext(_ints(ng), NBC, _ints(per), _ints(b), lo, hi)
    return list(lo), list(hi)


def make_field(kind, ng):
    nx, ny, nz = ng
    z, y, x = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij")
    p = 1.0 + 0.3 * np.sin(2 * np.pi * x / nx) * np.cos(2 * np.pi * y / ny) * np.cos(2 * np.pi * z / nz)
    spot = None
    if kind != "smooth":
        spot = (nz // 2, ny // 2, (2 * nx) // 3)
        p[spot] = {"jump": 100.0, "nan": np.nan, "zero": 0.0}[kind]
    full = np.zeros((nz + 2 * NBC, ny + 2 * NBC, nx + 2 * NBC))
    full[NBC:-NBC, NBC:-NBC, NBC:-NBC] = p
    return full, spot


def block_of(nb, i, d):
    return min(i // (62, 4, 8)[d], nb[d] - 1)


@pytest.mark.parametrize("faces", FACES)
@pytest.mark.parametrize("ng", GRIDS)
@pytest.mark.parametrize("kind", ["smooth", "jump", "nan", "zero"])
def test_quiet_blocks_have_no_steep_cell(probe, ng, faces, kind):
    p, spot = make_field(kind, ng)
    fill_ghosts(p, faces)
    steep = steep_model(p)
    nb, quiet = screen(probe, ng, faces, p)
    covered = np.zeros(p.shape, dtype=np.int32)
    for bz, by, bx in itertools.product(range(nb[2]), range(nb[1]), range(nb[0])):
        lo, hi = ext_box(probe, ng, faces, (bx, by, bz))
        box = (slice(lo[2], hi[2]), slice(lo[1], hi[1]), slice(lo[0], hi[0]))
        covered[box] += 1
        if quiet[bz, by, bx]:
            assert not steep[box].any(), (ng, faces, kind, (bx, by, bz))
    # the extended blocks tile the array: every cell is either cleared or evaluated, exactly once
    assert (covered == 1).all()
    if kind == "smooth":
        assert quiet.all()
        return
    # not vacuous: active blocks exist, and only within one block of the planted cell (wrapping on periodic axes)
    sb = [block_of(nb, spot[2 - d], d) for d in range(3)]
    active = ~quiet
    assert active[sb[2], sb[1], sb[0]]
    for bz, by, bx in zip(*np.nonzero(active)):
        for d, b in enumerate((bx, by, bz)):
            dist = abs(int(b) - sb[d])
            if faces[d] == "p":
                dist = min(dist, nb[d] - dist)
            assert dist <= 1, (ng, faces, kind, (bx, by, bz), sb)


def test_key_order_and_round_trip(probe):
    vals = [-np.inf, -3.5, -1e-300, -0.0, 0.0, 5e-324, 1.0, 1.0 + 2 ** -52, 1e300, np.inf]
    for a, b in zip(vals, vals[1:]):
        if a == b:   # -0.0 and 0.0 compare equal as doubles; their keys may differ, in this order
            assert not probe.hs_key_less(b, a)
        else:
            assert probe.hs_key_less(a, b) == 1 and probe.hs_key_less(b, a) == 0
    for v in vals:
        r = probe.hs_key_roundtrip(v)
        assert r == v and np.signbit(r) == np.signbit(v)
