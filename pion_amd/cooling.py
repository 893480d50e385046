"""Host-side cooling data for mp_only_cooling: thin wrapper over pion_amd/host/libpion_host.so (cooling_tables.cpp).
EP.cooling = 8: the look-up tables, restating mp_only_cooling::gen_mpoc_lookup_tables
(microphysics/mp_only_cooling.cpp:528-579).  EP.cooling = 4..7: a total-CIE curve the caller supplies (knots in
log10 T, log10 Lambda), its natural spline and the evaluation of cooling_function_SD93CIE::cooling_rate_SD93CIE
(microphysics/cooling_SD93_cie.cpp:666-704)."""
import ctypes as C
import os

import numpy as np

from . import abi

_HERE = os.path.dirname(os.path.abspath(__file__))
_lib = None


def _load():
    global _lib
    if _lib is None:
        path = os.path.join(_HERE, "host", "libpion_host.so")
        if not os.path.exists(path):
            raise ImportError("%s not found: run __graft_entry__.build()" % path)
        abi.share_torch_hip_runtime()
        _lib = C.CDLL(path)
        dp = C.POINTER(C.c_double)
        _lib.pion_host_build_cooling_tables.argtypes = [C.c_double, C.c_double, C.c_int, dp, dp, dp]
        for f in ("pion_host_cooling_rate_wss09", "pion_host_hii_rrr", "pion_host_hii_total_cooling"):
            getattr(_lib, f).restype = C.c_double
            getattr(_lib, f).argtypes = [C.c_double]
        ip = C.POINTER(C.c_int)
        _lib.pion_host_build_cooling_curve.argtypes = [C.c_int, dp, dp, dp]
        _lib.pion_host_cooling_curve_set.argtypes = [C.c_int, dp, dp, C.c_double, C.c_double]
        _lib.pion_host_cooling_curve_rate.restype = C.c_double
        _lib.pion_host_cooling_curve_rate.argtypes = [C.c_double]
        _lib.pion_host_read_cooling_curve.argtypes = [C.c_char_p, C.c_int, dp, dp, ip, C.c_char_p, C.c_int]
    return _lib


def build_tables(min_temp, max_temp, nT=200):
    """Returns (T[nT], tabs[5,nT], slopes[5,nT]); rows: rrhp, C_rrh, C_ffhe, C_fbdn, C_cie."""
    lib = _load()
    T = np.zeros(nT)
    tabs = np.zeros(5 * nT)
    slopes = np.zeros(5 * nT)
    dp = C.POINTER(C.c_double)
    rc = lib.pion_host_build_cooling_tables(min_temp, max_temp, nT, T.ctypes.data_as(dp),
                                            tabs.ctypes.data_as(dp), slopes.ctypes.data_as(dp))
    if rc != 0:
        raise ValueError("bad temperature range")
    return T, tabs.reshape(5, nT), slopes.reshape(5, nT)


def cooling_rate_wss09(T):
    return _load().pion_host_cooling_rate_wss09(float(T))


def hii_rrr(T):
    return _load().pion_host_hii_rrr(float(T))


def hii_total_cooling(T):
    return _load().pion_host_hii_total_cooling(float(T))


MAX_KNOTS = 256
REF_MIN_SLOPE = 8.0   # cooling_SD93_cie.cpp:160, 621


def _dp(a):
    return a.ctypes.data_as(C.POINTER(C.c_double))


def ref_max_slope(logT, logL):
    """The reference's slope above the knots: that of the last interval (cooling_SD93_cie.cpp:161-164, 622-625)."""
    return (logL[-1] - logL[-2]) / (logT[-1] - logT[-2])


def build_curve(logT, logL, min_slope=None, max_slope=None):
    """The curve as pion_gpu_set_cooling_curve / GpuSim.set_cooling_curve take it:
    (logT[n], logL[n], c[n], min_slope, max_slope), c the natural-spline second-derivative coefficients.  The slopes
    default to the reference's (8 below, the last interval's above)."""
    logT = np.ascontiguousarray(logT, dtype=np.float64)
    logL = np.ascontiguousarray(logL, dtype=np.float64)
    if logT.ndim != 1 or logT.shape != logL.shape:
        raise ValueError("logT and logL must be 1-D arrays of one length")
    c = np.zeros_like(logT)
    if _load().pion_host_build_cooling_curve(logT.size, _dp(logT), _dp(logL), _dp(c)) != 0:
        raise ValueError("cooling curve: 2..%d finite knots, strictly increasing in log10 T" % MAX_KNOTS)
    if min_slope is None:
        min_slope = REF_MIN_SLOPE
    if max_slope is None:
        max_slope = ref_max_slope(logT, logL)
    return logT, logL, c, float(min_slope), float(max_slope)


def set_curve(logT, logL, min_slope=None, max_slope=None):
    """Sets the process-global curve that curve_rate evaluates; returns build_curve's tuple."""
    cv = build_curve(logT, logL, min_slope, max_slope)
    if _load().pion_host_cooling_curve_set(cv[0].size, _dp(cv[0]), _dp(cv[1]), cv[3], cv[4]) != 0:
        raise ValueError("cooling curve: finite slopes required")
    return cv


def curve_rate(T):
    """Lambda(T) of the curve set by set_curve (scalar or array); inf for T < 0 or a T that is not finite."""
    f = _load().pion_host_cooling_curve_rate
    if np.ndim(T) == 0:
        return f(float(T))
    T = np.asarray(T, dtype=np.float64)
    return np.array([f(float(t)) for t in T.ravel()]).reshape(T.shape)


def read_curve(path):
    """(logT, logL) from a text file of two columns, log10 T and log10 Lambda ('#' starts a comment)."""
    logT, logL = np.zeros(MAX_KNOTS), np.zeros(MAX_KNOTS)
    n = C.c_int(0)
    err = C.create_string_buffer(512)
    rc = _load().pion_host_read_cooling_curve(os.fsencode(path), MAX_KNOTS, _dp(logT), _dp(logL), C.byref(n), err, 512)
    if rc != 0:
        raise ValueError(err.value.decode())
    return logT[:n.value].copy(), logL[:n.value].copy()
