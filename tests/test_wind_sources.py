"""CPU tests of the wind-source layer: the .wnd.txt reader (pion_host_read_wind_evolution) and the restated
root_find_linear_vec that the GPU wind-source tests check the device against."""
import math
import os

import numpy as np
import pytest

import wind_restate as wr
from pion_amd import wind

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WND = os.path.join(ROOT, "tests", "golden", "eta_car.wnd.txt")
HOST = os.path.join(ROOT, "pion_amd", "host", "libpion_host.so")

need_host = pytest.mark.skipif(not os.path.exists(HOST), reason="libpion_host.so not built (__graft_entry__.build())")


def _fixture_rows():
    rows = []
    for line in open(WND).read().splitlines()[2:]:
        f = line.split()
        if f and not f[0].startswith("#"):
            rows.append([float(v) for v in f])
    return np.array(rows)


@need_host
def test_reader_values_and_radius():
    ev = wind.read_wind_evolution(WND)
    rows = _fixture_rows()
    assert rows.shape == (6, 8) and ev.npt == 6
    for c, name in enumerate(wind.COLUMNS[:8]):
        assert np.array_equal(getattr(ev, name) if hasattr(ev, name) else ev.cols[name], rows[:, c]), name
    # R = sqrt(L/(4 pi sigma Teff^4)), pow_fast(Teff, 4) = exp(4 log Teff) (stellar_wind_BC.cpp:1079-1081)
    for i in range(6):
        L, T = rows[i, 2], rows[i, 3]
        R = math.sqrt(L / (4.0 * wr.PI * 5.670367e-5 * math.exp(4.0 * math.log(T))))
        assert ev.R[i] == R
    assert 1.8e12 < ev.R[0] < 2.0e12   # 9.666e39 erg/s at 44031 K


@need_host
def test_reader_offset_scale_and_missing_columns():
    ev = wind.read_wind_evolution(WND, time_offset=-5.79e10, t_scalefac=4.0)
    rows = _fixture_rows()
    assert np.array_equal(ev.time, (rows[:, 0] + -5.79e10) / 4.0)
    assert np.array_equal(ev.Mdot, rows[:, 4])          # only the time column moves
    for e in wind.ELEMENTS:                               # an 8-column file: the element columns stay 0
        assert np.array_equal(ev.cols[e], np.zeros(6)), e


@need_host
def test_reader_fifteen_columns_and_carry_over(tmp_path):
    p = tmp_path / "w.wnd.txt"
    p.write_text("# h1\n# h2\n"
                 "   1.0E+00 2.0E+00 3.0E+00 4.0E+00 5.0E+00 6.0E+00 7.0E+00 8.0E+00"
                 " 0.7E+00 0.28E+00 1.0E-03 2.0E-03 3.0E-03 4.0E-03 5.0E-03\n"
                 "   2.0E+00 2.0E+00 3.0E+00 4.0E+00 5.0E+00 6.0E+00 7.0E+00 9.0E+00\n\n")
    ev = wind.read_wind_evolution(str(p))
    assert ev.npt == 2
    assert list(ev.time) == [1.0, 2.0] and list(ev.vinf) == [8.0, 9.0]
    # sscanf leaves what a line lacks untouched: row 2 keeps row 1's element fractions
    assert list(ev.X_H) == [0.7, 0.7] and list(ev.X_D) == [5.0e-3, 5.0e-3]


def test_root_find_linear_vec_restatement():
    x = [0.0, 1.0, 3.0, 7.0]
    y = [10.0, 20.0, 0.0, 4.0]
    assert wr.root_find_linear_vec(x, y, 0.0) == 10.0          # nodes
    assert wr.root_find_linear_vec(x, y, 1.0) == 20.0
    assert wr.root_find_linear_vec(x, y, 3.0) == 0.0
    assert wr.root_find_linear_vec(x, y, 7.0) == 4.0
    assert wr.root_find_linear_vec(x, y, 0.5) == 15.0          # mid-interval
    assert wr.root_find_linear_vec(x, y, 2.0) == 10.0
    assert wr.root_find_linear_vec(x, y, 5.0) == 2.0
    assert wr.root_find_linear_vec(x, y, -3.0) == 10.0         # before the table: zero slope
    assert wr.root_find_linear_vec(x, y, 100.0) == 4.0         # after the table: zero slope
    # two nodes, at or before the first: the bisection collapses onto node 0 and the reference divides 0 by 0
    assert math.isnan(wr.root_find_linear_vec([1.0, 2.0], [3.0, 5.0], 1.0))
    assert wr.root_find_linear_vec([1.0, 2.0], [3.0, 5.0], 1.5) == 4.0


def test_equalD_restatement():
    assert wr.equalD(0.0, 0.0) and wr.equalD(1e-101, 0.0) and not wr.equalD(1e-50, 0.0)
    assert wr.equalD(1.0, 1.0 + 1e-13) and not wr.equalD(1.0, 1.0 + 1e-11)
