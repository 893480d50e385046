"""ctypes access to tests/native/libbc_probe.so: the rules of the boundary update (pion_amd/csrc/dev_bc.h) run in host
loops, in the three modes pion_gpu_update_bcs has.  Used by tests/test_bc_rule.py."""
import ctypes
import os
import subprocess

import numpy as np

from pion_amd import abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NATIVE = os.path.join(ROOT, "tests", "native")
SO = os.path.join(NATIVE, "libbc_probe.so")

PERIODIC_ALL, ONE_LAUNCH, FACE_SEQUENCE = range(3)   # BcMode

_lib = None


def lib():
    """the probe library, built on demand (seconds)"""
    global _lib
    if _lib is None:
        deps = [os.path.join(NATIVE, "bc_probe.cpp")] + [os.path.join(ROOT, "pion_amd", "csrc", f)
                                                         for f in ("dev_bc.h", "grid_desc.h")]
        if not os.path.exists(SO) or os.path.getmtime(SO) < max(os.path.getmtime(f) for f in deps):
            subprocess.check_call(["make", "-C", NATIVE, "libbc_probe.so"])
        L = ctypes.CDLL(SO)
        i, p, d = ctypes.c_int, ctypes.c_void_p, ctypes.c_double
        L.bcp_mode.argtypes = [p, i, i, i]
        L.bcp_dmr2_cols.argtypes = [p]
        L.bcp_capture_cell.argtypes = [p, i, i, p]
        L.bcp_capture_cell.restype = None
        L.bcp_cell_centre.argtypes = [p, i, i]
        L.bcp_cell_centre.restype = d
        L.bcp_update.argtypes = [p, i, d, i, p, p]
        _lib = L
    return _lib


def mode(cfg, fuse_bc=True, any_wind=False, assign=False):
    """the mode pion_gpu_update_bcs takes for this configuration"""
    return lib().bcp_mode(ctypes.addressof(cfg), int(fuse_bc), int(any_wind), int(assign))


def dmr2_cols(cfg):
    return lib().bcp_dmr2_cols(ctypes.addressof(cfg))


def capture_cell(cfg, d, inflow):
    """all-cell coordinates (x, y, z) of the cell an assignment of face d captures"""
    o = np.zeros(3, np.int32)
    lib().bcp_capture_cell(ctypes.addressof(cfg), d, int(inflow), o.ctypes.data)
    return tuple(int(v) for v in o)


def cell_centre(cfg, ax, i):
    return lib().bcp_cell_centre(ctypes.addressof(cfg), ax, i)


def new_refval():
    """the states the faces hold before any assignment"""
    return np.zeros((6, abi.PION_MAX_NVAR))


def update(cfg, mode_, P, refval, simtime=0.0, assign=False):
    """one boundary update of a copy of P ([nvar][nz][ny][nx], ghosts included) in the given mode; refval is read, and
    written by an assigning face sequence"""
    A = np.ascontiguousarray(P, dtype=np.float64).copy()
    assert A.size == cfg.nvar * abi.ncell_all(cfg) and refval.flags.c_contiguous
    rc = lib().bcp_update(ctypes.addressof(cfg), mode_, simtime, int(assign), A.ctypes.data, refval.ctypes.data)
    if rc != 0:
        raise ValueError("mode %d is not one this update admits" % mode_)
    return A
