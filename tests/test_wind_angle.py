"""CPU tests of the rotating-star (LGM99) wind sources: pion_gpu_wind_angle_tables (host code of libpion_gpu.so) is
bit for bit stellar_wind_angle::setup_tables as tests/wind_angle_restate.py restates it; the ctypes bindings of the
new entry points match the headers; the host layer's entry point refuses what it can refuse without a device."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import wind_angle_restate as ar
from pion_amd import abi, lib, problems, wind

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WND = os.path.join(ROOT, "tests", "golden", "eta_car.wnd.txt")
HOST = os.path.join(ROOT, "pion_amd", "host", "libpion_host.so")
need_lib = pytest.mark.skipif(not os.path.exists(abi.library_path()),
                              reason="libpion_gpu.so not built (__graft_entry__.build())")


def test_restated_knots_are_the_documented_ones():
    T = ar.tables(0.0)
    assert len(T.theta) == 25 and len(T.omega) == 25 and len(T.Teff) == 22
    assert T.omega[0] == 0.0 and T.omega[-1] == 0.9999
    assert T.Teff == [1000.0, 3600.0, 4400.0, 4800.0, 5200.0, 5600.0, 6000.0, 6000.0, 7000.0, 7500.0, 8000.0,
                      8000.0, 9000.0, 9500.0, 10000.0, 10000.0, 20000.0, 21000.0, 21500.0, 22000.0, 22000.0, 150000.0]
    assert abs(T.theta[0] * 180.0 / ar.PI - 0.1) < 1e-12 and abs(T.theta[4] * 180.0 / ar.PI - 60.0) < 1e-12
    assert abs(T.theta[-1] * 180.0 / ar.PI - 89.9) < 1e-12


@need_lib
@pytest.mark.parametrize("xi", [0.0, -0.43])
def test_host_tables_are_bit_identical_to_the_restatement(xi):
    d = wind.angle_tables(xi)
    T = ar.tables(xi)
    for k in ("theta", "omega", "Teff", "delta", "alpha"):
        ref = np.array(getattr(T, k))
        assert d[k].shape == ref.shape, k
        assert np.array_equal(d[k].view(np.uint64), ref.view(np.uint64)), k
    assert d["delta"].size == 550 and d["alpha"].size == 13750
    assert np.isfinite(d["delta"]).all() and np.isfinite(d["alpha"]).all()


def test_xi_changes_delta_and_not_alpha():
    a, b = ar.tables(0.0), ar.tables(-0.43)
    assert a.alpha == b.alpha and a.delta != b.delta


def test_trilinear_restatement_refuses_what_the_reference_refuses():
    T = ar.tables(-0.43)
    th = T.theta
    with pytest.raises(ValueError):
        T.trilinear_alpha(0.0, th[3], 2.0e4)          # omega <= omega_vec[0]
    with pytest.raises(ValueError):
        T.trilinear_alpha(0.5, th[3], 1000.0)         # Teff <= Teff_vec[0]
    with pytest.raises(ValueError):
        T.trilinear_alpha(0.5, th[0], 2.0e4)          # theta <= theta_vec[0]
    with pytest.raises(ValueError):
        T.trilinear_alpha(0.5, ar.PI / 2.0, 2.0e4)    # theta = 90 deg: past the vector
    # on the knots the interpolation returns the table
    assert T.trilinear_alpha(T.omega[3], th[7], T.Teff[9]) == T.alpha[3][7][9]


def test_windsource_angle_fields():
    cfg, P, srcs = problems.etacar2d_lgm99(64, WND)
    s = srcs[0]
    assert s.type == wind.ANGLE == 2 and s.xi == -0.43
    st, keep = s.to_c()
    assert st.type == 2 and np.array_equal(keep[-1], s.evolution.vcrit)
    assert wind.WindSource(pos=(0, 0), radius=1.0).xi == 0.0


def _prototype(header, name):
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", header)).read(), flags=re.S)
    m = re.search(r"int\s+%s\s*\(([^)]*)\)\s*;" % name, txt)
    assert m, name
    return [" ".join(a.split()) for a in m.group(1).split(",")]


def test_rotating_entry_point_signatures_match_the_headers():
    assert _prototype("pion_gpu.h", "pion_gpu_add_rotating_wind_source") == [
        "void *handle", "const pion_gpu_wind_source *src", "const double *evo_vcrit", "double xi", "int *id"]
    assert _prototype("pion_gpu.h", "pion_gpu_wind_angle_tables") == [
        "double xi", "double *theta", "double *omega", "double *Teff", "double *delta", "double *alpha"]
    assert _prototype("pion_host.h", "pion_host_sim_add_rotating_wind_source") == [
        "void *sim", "const pion_gpu_wind_source *src", "const double *evo_vcrit", "double xi", "int *id"]


@need_lib
def test_ctypes_bindings_match_the_header():
    L = lib.load_library()
    dp = C.POINTER(C.c_double)
    assert L.pion_gpu_add_rotating_wind_source.argtypes == [C.c_void_p, C.c_void_p, dp, C.c_double,
                                                            C.POINTER(C.c_int)]
    assert L.pion_gpu_wind_angle_tables.argtypes == [C.c_double, dp, dp, dp, dp, dp]
    assert "pion_gpu_add_rotating_wind_source" in lib.EXPORTED_SYMBOLS
    assert "pion_gpu_wind_angle_tables" in lib.EXPORTED_SYMBOLS
    # no handle: EINVAL, nothing dereferenced
    src, keep = problems.etacar2d_lgm99(64, WND)[2][0].to_c()
    assert L.pion_gpu_add_rotating_wind_source(None, C.byref(src), keep[-1].ctypes.data_as(dp), -0.43, None) == -1
    assert L.pion_gpu_add_rotating_wind_source(None, None, None, 0.0, None) == -1


@pytest.mark.skipif(not os.path.exists(HOST), reason="libpion_host.so not built")
def test_host_entry_point_refuses_null_arguments():
    abi.share_torch_hip_runtime()
    C.CDLL(abi.library_path(), mode=C.RTLD_GLOBAL)
    host = C.CDLL(HOST)
    f = host.pion_host_sim_add_rotating_wind_source
    f.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(C.c_double), C.c_double, C.POINTER(C.c_int)]
    src, keep = problems.etacar2d_lgm99(64, WND)[2][0].to_c()
    i = C.c_int(-7)
    assert f(None, C.byref(src), keep[-1].ctypes.data_as(C.POINTER(C.c_double)), -0.43, C.byref(i)) == -1
    assert f(C.c_void_p(1), None, None, -0.43, C.byref(i)) == -1
    assert i.value == -7
