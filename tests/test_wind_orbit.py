"""CPU tests of the orbital motion of wind sources: pion_gpu_wind_orbit_position (host code of libpion_gpu.so) is bit
for bit the reference's ellipse as tests/orbit_restate.py restates it, the NaN orbits included; the ctypes mirror of
pion_gpu_wind_source matches the C struct's layout."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

import orbit_restate as orr
from pion_amd import abi, wind

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
need_lib = pytest.mark.skipif(not os.path.exists(abi.library_path()),
                              reason="libpion_gpu.so not built (__graft_entry__.build())")


def _same(a, b):
    """bitwise equal, NaN == NaN"""
    return all((x == y and math.copysign(1.0, x) == math.copysign(1.0, y)) or (x != x and y != y)
               for x, y in zip(a, b))


ORBITS = [
    (1.2, -1.28e15, 1.0e14, 10.0),          # cwb2d_orbit's
    (1.2, 2.42e15, -2.0e14, 2.0),
    (1.0, 3.0e15, 4.0e15, 1.0),             # circular
    (2.5, -1.0e15, -3.0e15, 7.3),
    (0.6, 5.0e14, 5.0e14, 0.25),
    (0.4, 1.0e15, 2.0e15, 3.0),             # f < 1/2: a*a - e*e < 0, b is NaN
    (1.5, 1.0e-3, 1.0e16, 100.0),
    (1.5, 0.0, 2.0e15, 1.0),                # px == 0: 0/0
    (1.5, 2.0e15, 0.0, 1.0),                # py == 0: 0/0
    (0.0, 2.0e15, 1.0e15, 1.0),             # f == 0: 0/0
    (-1.2, 2.0e15, 1.0e15, -4.0),           # negative factor and period
]
TIMES = [0.0, 1.0, 3.7e5, 1.0e6, 3.1558150e7, 1.0e8, 2.5e9, 1.234567e11, -2.0e7] + \
    [float(t) for t in np.linspace(0.0, 3.0e8, 23)]


@need_lib
@pytest.mark.parametrize("ndim", [2, 3])
def test_orbit_position_bitwise_equals_restatement(ndim):
    n = 0
    for k, orbit in enumerate(ORBITS):
        src = wind.WindSource(pos=(2.56e15 * (k - 4), -1.7e15 + 3.0e14 * k, 4.1e14 * k), radius=1.0e15, orbit=orbit)
        for t in TIMES:
            a = wind.orbit_position(src, ndim, t)
            b = orr.orbit_position(src, ndim, t)
            assert _same(a, b), (orbit, t, a, b)
            assert a[2] == (src.pos[2] if ndim == 3 else 0.0)
            n += 1
    assert n == len(ORBITS) * len(TIMES)


@need_lib
def test_orbit_position_nan_cases_and_first_update():
    for orbit in [(1.5, 0.0, 2.0e15, 1.0), (1.5, 2.0e15, 0.0, 1.0), (0.0, 2.0e15, 1.0e15, 1.0)]:
        src = wind.WindSource(pos=(1.0e15, 2.0e15, 3.0e15), radius=1.0e15, orbit=orbit)
        for t in (0.0, 1.0e7):
            p = wind.orbit_position(src, 3, t)
            assert math.isnan(p[0]) and math.isnan(p[1]) and p[2] == 3.0e15
    # simtime = 0 is a real move: in general not bit-identical to the set-up position
    moved = 0
    for k in range(40):
        src = wind.WindSource(pos=(1.0e15 + 3.3e13 * k, -7.0e14 + 1.1e13 * k), radius=1.0e15,
                              orbit=(1.3, 1.1e15 + 1.0e13 * k, -4.0e14, 1.0))
        p = wind.orbit_position(src, 2, 0.0)
        assert _same(p, orr.orbit_position(src, 2, 0.0))
        assert abs(p[0] - src.pos[0]) < 1.0 and abs(p[1] - src.pos[1]) < 1.0
        moved += (p[0] != src.pos[0]) or (p[1] != src.pos[1])
    assert moved > 0


@need_lib
def test_fixed_source_position_is_its_pos():
    src = wind.WindSource(pos=(1.0e15, 2.0e15, 3.0e15), radius=1.0e15)
    assert wind.orbit_position(src, 3, 5.0e8) == (1.0e15, 2.0e15, 3.0e15)
    assert wind.orbit_position(src, 2, 5.0e8) == (1.0e15, 2.0e15, 0.0)
    src = wind.WindSource(pos=(1.0e15, 2.0e15, 3.0e15), radius=1.0e15, orbit=(1.2, 1.0e15, 1.0e15, 0.0))
    assert wind.orbit_position(src, 3, 5.0e8) == (1.0e15, 2.0e15, 3.0e15)


@need_lib
def test_orbit_position_einval():
    from pion_amd import lib
    L = lib.load_library()
    st, keep = wind.WindSource(pos=(0.0, 0.0), radius=1.0, orbit=(1.2, 1.0, 1.0, 1.0)).to_c()
    out = (C.c_double * 3)()
    for ndim in (0, 1, 4):
        assert L.pion_gpu_wind_orbit_position(C.byref(st), ndim, 0.0, out) == -1
    assert L.pion_gpu_wind_orbit_position(None, 2, 0.0, out) == -1
    assert L.pion_gpu_wind_orbit_position(C.byref(st), 2, 0.0, None) == -1
    assert L.pion_gpu_wind_orbit_position(C.byref(st), 2, 0.0, out) == 0
    for ndim in (1, 4):
        with pytest.raises(ValueError):
            wind.orbit_position(wind.WindSource(pos=(0.0,), radius=1.0, orbit=(1.2, 1.0, 1.0, 1.0)), ndim, 0.0)


def test_windsource_orbit_argument():
    s = wind.WindSource(pos=(1.0, 2.0), radius=1.0, orbit=(1.2, 3.0, 4.0, 5.0))
    st, _ = s.to_c()
    assert (st.orbit_ecc_fac, st.orbit_periastron[0], st.orbit_periastron[1], st.orbit_period) == (1.2, 3.0, 4.0, 5.0)
    st, _ = wind.WindSource(pos=(1.0, 2.0), radius=1.0).to_c()
    assert st.orbit_period == 0.0 and st.orbit_ecc_fac == 0.0
    with pytest.raises(ValueError):
        wind.WindSource(pos=(1.0, 2.0), radius=1.0, orbit=(1.2, 3.0, 4.0))


def test_ctypes_mirror_matches_the_header():
    """the fields of pion_gpu_wind_source in include/pion_gpu.h, in order, are those of the ctypes mirror; the orbit
    fields end the struct (C would read past a shorter mirror)"""
    txt = open(os.path.join(ROOT, "include", "pion_gpu.h")).read()
    body = re.search(r"typedef struct pion_gpu_wind_source \{(.*?)\} pion_gpu_wind_source;", txt, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = []
    for decl in body.split(";"):
        decl = decl.strip()
        if not decl:
            continue
        for part in decl.split(",")[0:1] + decl.split(",")[1:]:
            m = re.search(r"\**\s*(\w+)\s*(\[[^\]]*\])?\s*$", part.strip())
            names.append(m.group(1))
    assert [f[0] for f in wind.PionGpuWindSource._fields_] == names
    assert names[-4:] == ["update_freq", "orbit_ecc_fac", "orbit_periastron", "orbit_period"]
    assert wind.PionGpuWindSource.orbit_period.offset + 8 == C.sizeof(wind.PionGpuWindSource)
