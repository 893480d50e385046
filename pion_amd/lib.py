"""Thin ctypes wrapper around libpion_gpu.so (include/pion_gpu.h).

There is no CPU fallback: if the HIP library is missing or a GPU call fails the
wrapper raises.  Method names mirror the C-ABI, which mirrors the reference's
time_integrator / FV_solver_base entry points (see the header for file:line).
"""
import ctypes as C
import os

import numpy as np

from . import abi

_dp = C.POINTER(C.c_double)
_lib = None


class PionGpuError(RuntimeError):
    def __init__(self, what, rc, msg):
        super().__init__("pion_gpu_%s failed rc=%d: %s" % (what, rc, msg))
        self.rc = rc


def load_library():
    """Load pion_amd/csrc/libpion_gpu.so; loud failure when it has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    path = abi.library_path()
    if not os.path.exists(path):
        raise ImportError(
            "%s not found: build it with `make -C pion_amd/csrc` (or __graft_entry__.build()); "
            "pion_amd has no CPU fallback" % path)
    abi.share_torch_hip_runtime()
    lib = C.CDLL(path)
    lib.pion_gpu_create.argtypes = [C.POINTER(abi.PionGpuConfig), C.c_int, C.POINTER(C.c_void_p)]
    lib.pion_gpu_destroy.argtypes = [C.c_void_p]
    lib.pion_gpu_destroy.restype = None
    lib.pion_gpu_last_error.argtypes = [C.c_void_p, C.c_char_p, C.c_int]
    lib.pion_gpu_ncell_all.argtypes = [C.c_void_p]
    lib.pion_gpu_ncell_all.restype = C.c_long
    lib.pion_gpu_upload.argtypes = [C.c_void_p, _dp]
    lib.pion_gpu_download.argtypes = [C.c_void_p, C.c_int, _dp]
    lib.pion_gpu_bind_device_state.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
    lib.pion_gpu_device_ptr.argtypes = [C.c_void_p, C.c_int]
    lib.pion_gpu_device_ptr.restype = C.c_void_p
    lib.pion_gpu_set_stream.argtypes = [C.c_void_p, C.c_void_p]
    lib.pion_gpu_set_comm_stream.argtypes = [C.c_void_p, C.c_void_p]
    lib.pion_gpu_set_jet.argtypes = [C.c_void_p, C.c_int, _dp]
    lib.pion_gpu_stage_part.argtypes = [C.c_void_p, C.c_double, C.c_int, C.c_int, C.c_int]
    lib.pion_gpu_synchronize.argtypes = [C.c_void_p]
    lib.pion_gpu_set_wind_cells.argtypes = [C.c_void_p, C.c_long, C.POINTER(C.c_long), _dp]
    lib.pion_gpu_add_wind_source.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(C.c_int)]
    lib.pion_gpu_add_rotating_wind_source.argtypes = [C.c_void_p, C.c_void_p, _dp, C.c_double, C.POINTER(C.c_int)]
    lib.pion_gpu_wind_angle_tables.argtypes = [C.c_double, _dp, _dp, _dp, _dp, _dp]
    lib.pion_gpu_get_wind_cells.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_long), C.POINTER(C.c_long), _dp]
    lib.pion_gpu_get_wind_source_pos.argtypes = [C.c_void_p, C.c_int, _dp]
    lib.pion_gpu_wind_orbit_position.argtypes = [C.c_void_p, C.c_int, C.c_double, _dp]
    lib.pion_gpu_get_flags.argtypes = [C.c_void_p, C.c_void_p]
    if hasattr(lib, "pion_gpu_get_hll_switch"):   # (a PION_GPU_LIB build for A/B runs may predate these two read-backs)
        lib.pion_gpu_get_hll_switch.argtypes = [C.c_void_p, C.c_void_p]
        lib.pion_gpu_get_hll_screen_counts.argtypes = [C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_int)]
    if hasattr(lib, "pion_gpu_get_hcorr_eta"):   # (likewise)
        lib.pion_gpu_get_hcorr_eta.argtypes = [C.c_void_p, C.c_int, _dp]
    if hasattr(lib, "pion_gpu_rows_windows"):   # (likewise)
        _ip = C.POINTER(C.c_int)
        lib.pion_gpu_rows_windows.argtypes = [C.POINTER(abi.PionGpuConfig), C.c_long, C.c_int, C.c_int, C.c_int, _ip, _ip]
        lib.pion_gpu_get_rows_windows.argtypes = [C.c_void_p, C.POINTER(C.c_long), _ip, _ip]
    lib.pion_gpu_set_cooling_tables.argtypes = [C.c_void_p, C.c_int, _dp, _dp, _dp]
    if hasattr(lib, "pion_gpu_set_cooling_curve"):   # (likewise)
        lib.pion_gpu_set_cooling_curve.argtypes = [C.c_void_p, C.c_int, _dp, _dp, _dp, C.c_double, C.c_double]
        lib.pion_gpu_cooling_curve_eval.argtypes = [C.c_void_p, C.c_int, _dp, _dp]
    lib.pion_gpu_update_bcs.argtypes = [C.c_void_p, C.c_double, C.c_int, C.c_int, C.c_int]
    lib.pion_gpu_calc_dt.argtypes = [C.c_void_p, _dp, _dp]
    lib.pion_gpu_set_glm_speeds.argtypes = [C.c_void_p, C.c_double, C.c_double, C.c_double]
    lib.pion_gpu_stage.argtypes = [C.c_void_p, C.c_double, C.c_int, C.c_int]
    lib.pion_gpu_advance_time.argtypes = [C.c_void_p, C.c_double, C.c_double]
    lib.pion_gpu_halo_count.argtypes = [C.c_void_p]
    lib.pion_gpu_halo_count.restype = C.c_long
    lib.pion_gpu_pack_halo.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p]
    lib.pion_gpu_unpack_halo.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p]
    lib.pion_gpu_halo_spans.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
    lib.pion_gpu_halo_begin.argtypes = [C.c_void_p]
    lib.pion_gpu_halo_end.argtypes = [C.c_void_p]
    if hasattr(lib, "pion_gpu_pack_ongrid"):   # (likewise)
        lib.pion_gpu_ongrid_count.argtypes = [C.c_void_p, C.c_int]
        lib.pion_gpu_ongrid_count.restype = C.c_long
        lib.pion_gpu_pack_ongrid.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p]
        lib.pion_gpu_unpack_ongrid.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p]
    if hasattr(lib, "pion_gpu_pack_fits"):   # (likewise)
        lib.pion_gpu_fits_images.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(C.c_int)]
        lib.pion_gpu_fits_count.argtypes = [C.c_void_p, C.c_int]
        lib.pion_gpu_fits_count.restype = C.c_long
        lib.pion_gpu_pack_fits.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p]
    if hasattr(lib, "pion_gpu_unpack_fits"):   # (likewise)
        lib.pion_gpu_fits_prim_count.argtypes = [C.c_void_p, C.c_int]
        lib.pion_gpu_fits_prim_count.restype = C.c_long
        lib.pion_gpu_unpack_fits.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p]
        lib.pion_gpu_unpack_fits_status.argtypes = [C.c_void_p, C.POINTER(C.c_long)]
    if hasattr(lib, "pion_gpu_project"):   # (likewise)
        lib.pion_gpu_project_count.argtypes = [C.c_void_p, C.c_int, C.c_int]
        lib.pion_gpu_project_count.restype = C.c_long
        lib.pion_gpu_project.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]
    if hasattr(lib, "pion_gpu_project_part"):   # (likewise)
        lib.pion_gpu_project_part_count.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p]
        lib.pion_gpu_project_part_count.restype = C.c_long
        lib.pion_gpu_project_part.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
    if hasattr(lib, "pion_gpu_project_angle"):   # (likewise)
        lib.pion_gpu_project_angle_count.argtypes = [C.c_void_p, C.c_double, C.c_int, C.POINTER(C.c_int)]
        lib.pion_gpu_project_angle_count.restype = C.c_long
        lib.pion_gpu_project_angle.argtypes = [C.c_void_p, C.c_int, C.c_double, C.c_int, C.c_void_p, C.c_void_p]
        lib.pion_gpu_project_angle_status.argtypes = [C.c_void_p, C.POINTER(C.c_long)]
    if hasattr(lib, "pion_gpu_raytrace"):   # (likewise)
        _cfgp, _srcp = C.POINTER(abi.PionGpuConfig), C.POINTER(abi.RtSource)
        lib.pion_gpu_add_rt_source.argtypes = [C.c_void_p, _srcp, C.POINTER(C.c_int), _dp]
        lib.pion_gpu_raytrace.argtypes = [C.c_void_p, C.c_int]
        lib.pion_gpu_rt_columns.argtypes = [C.c_void_p, C.c_int, C.c_int, _dp]
        lib.pion_gpu_rt_count.argtypes = [C.c_void_p, C.c_int]
        lib.pion_gpu_rt_count.restype = C.c_long
        lib.pion_gpu_pack_columns.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p]
        lib.pion_gpu_rt_plan.argtypes = [_cfgp, _srcp, C.POINTER(C.c_int), C.POINTER(C.c_long), C.POINTER(C.c_long)]
        lib.pion_gpu_raytrace_host.argtypes = [_cfgp, _srcp, _dp, _dp, _dp]
        lib.pion_gpu_rt_refused.argtypes = [_cfgp, _srcp]
        lib.pion_gpu_rt_refused.restype = C.c_char_p
    if hasattr(lib, "pion_gpu_raytrace_part"):   # (likewise)
        _partp, _ip, _lp = C.POINTER(abi.RtPart), C.POINTER(C.c_int), C.POINTER(C.c_long)
        lib.pion_gpu_add_rt_source_part.argtypes = [C.c_void_p, _srcp, _partp, _ip, _dp]
        lib.pion_gpu_rt_chain.argtypes = [_cfgp, _srcp, _partp, _ip, _ip, _ip]
        lib.pion_gpu_raytrace_part.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
        lib.pion_gpu_raytrace_host_part.argtypes = [_cfgp, _srcp, _partp, _dp, _dp, _dp, _dp]
        lib.pion_gpu_rt_plan_part.argtypes = [_cfgp, _srcp, _partp, _lp, _lp, _lp]
        lib.pion_gpu_rt_part_refused.argtypes = [_cfgp, _srcp, _partp]
        lib.pion_gpu_rt_part_refused.restype = C.c_char_p
    lib.pion_gpu_interface_flux.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_double, _dp, _dp, _dp, _dp, _dp]
    if hasattr(lib, "pion_gpu_cell_advance"):   # (likewise)
        lib.pion_gpu_cell_advance.argtypes = [C.c_void_p, C.c_int, C.c_double, _dp, _dp, _dp, _dp]
    lib.pion_gpu_cooling_update.argtypes = [C.c_void_p, C.c_int, C.c_double, _dp, _dp]
    lib.pion_gpu_cooling_edot.argtypes = [C.c_void_p, C.c_int, _dp, _dp, _dp]
    lib.pion_gpu_cooling_timescale.argtypes = [C.c_void_p, C.c_int, _dp, _dp]
    lib.pion_gpu_enable_timing.argtypes = [C.c_void_p, C.c_int]
    lib.pion_gpu_get_timing.argtypes = [C.c_void_p, _dp, C.c_int]
    _lib = lib
    return lib


# every symbol include/pion_gpu.h declares (checked by the CPU test-suite)
EXPORTED_SYMBOLS = [
    "pion_gpu_create", "pion_gpu_destroy", "pion_gpu_last_error", "pion_gpu_ncell_all",
    "pion_gpu_ng_all", "pion_gpu_upload", "pion_gpu_download", "pion_gpu_bind_device_state",
    "pion_gpu_device_ptr", "pion_gpu_set_stream", "pion_gpu_synchronize", "pion_gpu_set_wind_cells",
    "pion_gpu_set_cooling_tables", "pion_gpu_set_cooling_curve", "pion_gpu_cooling_curve_eval", "pion_gpu_update_bcs", "pion_gpu_calc_dt",
    "pion_gpu_set_glm_speeds", "pion_gpu_stage", "pion_gpu_advance_time", "pion_gpu_halo_count",
    "pion_gpu_pack_halo", "pion_gpu_unpack_halo", "pion_gpu_interface_flux",
    "pion_gpu_cooling_update", "pion_gpu_cooling_edot", "pion_gpu_cooling_timescale", "pion_gpu_enable_timing",
    "pion_gpu_calc_dt_device", "pion_gpu_read_dt", "pion_gpu_get_stream", "pion_gpu_dt_request", "pion_gpu_dt_wait",
    "pion_gpu_halo_spans", "pion_gpu_halo_begin", "pion_gpu_halo_end",
    "pion_gpu_get_timing", "pion_gpu_stage_part", "pion_gpu_set_comm_stream", "pion_gpu_set_jet",
    "pion_gpu_add_wind_source", "pion_gpu_get_wind_cells", "pion_gpu_get_wind_source_pos",
    "pion_gpu_wind_orbit_position", "pion_gpu_get_flags", "pion_gpu_add_rotating_wind_source",
    "pion_gpu_wind_angle_tables", "pion_gpu_get_hll_switch", "pion_gpu_get_hll_screen_counts",
    "pion_gpu_get_hcorr_eta", "pion_gpu_rows_windows", "pion_gpu_get_rows_windows",
    "pion_gpu_ongrid_count", "pion_gpu_pack_ongrid", "pion_gpu_unpack_ongrid",
    "pion_gpu_fits_images", "pion_gpu_fits_count", "pion_gpu_pack_fits",
    "pion_gpu_fits_prim_count", "pion_gpu_unpack_fits", "pion_gpu_unpack_fits_status",
    "pion_gpu_cell_advance", "pion_gpu_project_count", "pion_gpu_project",
    "pion_gpu_project_part_count", "pion_gpu_project_part",
    "pion_gpu_project_angle_count", "pion_gpu_project_angle", "pion_gpu_project_angle_status",
    "pion_gpu_add_rt_source", "pion_gpu_raytrace", "pion_gpu_rt_columns", "pion_gpu_rt_count",
    "pion_gpu_pack_columns", "pion_gpu_rt_plan", "pion_gpu_raytrace_host", "pion_gpu_rt_refused",
    "pion_gpu_add_rt_source_part", "pion_gpu_rt_chain", "pion_gpu_raytrace_part", "pion_gpu_raytrace_host_part",
    "pion_gpu_rt_plan_part", "pion_gpu_rt_part_refused",
]


def project_angle_on_host(cfg, angle_deg, fields, A, trip_limit=None, info=None):
    """pion_host_project_angle_on_host: the images [nfields][NR][NI] of a cylindrical (z,R) grid seen at angle_deg to
    its axis, by the rule of pion_amd/csrc/dev_project_angle.h in a host loop over the whole array A ([nvar][ncell_all],
    ghosts included).  Host only: needs no GPU.  trip_limit: the ray loops' trip limit instead of the rule's own
    (pion_host_project_angle_rule); info (a dict) receives n_extra, ncapped, tan and inv_sin"""
    from . import host_rccl
    h = host_rccl.load_host_library()
    arr = fields if isinstance(fields, C.Array) else abi.proj_fields(fields)
    nf, ne, why = len(fields), C.c_int(-1), C.c_char_p()
    n = h.pion_host_project_angle_count(C.byref(cfg), float(angle_deg), max(1, min(nf, abi.PROJ_MAX_FIELDS)), C.byref(ne),
                                        C.byref(why))
    if n < 0:
        raise PionGpuError("project_angle_on_host", n, (why.value or b"").decode())
    A = np.ascontiguousarray(A, dtype=np.float64).reshape(-1)
    img = np.empty(n, dtype=np.float64)
    ncapped, tn, invst = C.c_long(0), C.c_double(), C.c_double()
    limit = 2 * (cfg.ng[0] + cfg.ng[1]) + 8 if trip_limit is None else int(trip_limit)
    rc = h.pion_host_project_angle_rule(C.byref(cfg), float(angle_deg), limit, nf, arr, A.ctypes.data_as(_dp),
                                        img.ctypes.data_as(_dp), C.byref(ncapped), C.byref(tn), C.byref(invst))
    if rc != 0:
        raise PionGpuError("project_angle_on_host", rc, "refused (a bad field, or a trip limit below 1)")
    if info is not None:
        info.update(n_extra=ne.value, ncapped=ncapped.value, tan=tn.value, inv_sin=invst.value)
    return img[:n].reshape(nf, cfg.ng[1], -1)


def rt_refused(cfg, src):
    """pion_gpu_rt_refused: the text with which the ray tracer refuses `src` (an abi.RtSource or what abi.rt_source
    takes) on the grid of `cfg`, or None.  Host only: needs no GPU."""
    t = load_library().pion_gpu_rt_refused(C.byref(cfg), C.byref(abi.rt_source(src)))
    return None if t is None else t.decode()


def rt_plan(cfg, src):
    """pion_gpu_rt_plan: (tile, launches, levels) -- the tile of the tiled kernel, its launches (tile-levels) and the
    launches of the per-level kernel for `src` on the grid of `cfg`.  Host only: needs no GPU."""
    tile, launches, levels = (C.c_int * 3)(), C.c_long(-1), C.c_long(-1)
    rc = load_library().pion_gpu_rt_plan(C.byref(cfg), C.byref(abi.rt_source(src)), tile, C.byref(launches), C.byref(levels))
    if rc != 0:
        raise PionGpuError("rt_plan", rc, rt_refused(cfg, src) or "invalid arguments")
    return tuple(tile), launches.value, levels.value


def raytrace_host(cfg, src, P):
    """pion_gpu_raytrace_host: (col, dcol), each [nz][ny][nx], of `src` on the host array P ([nvar][nz_all][ny_all]
    [nx_all], ghosts included) by the device's own rules in a host loop.  Host only: needs no GPU."""
    P = np.ascontiguousarray(P, dtype=np.float64).reshape(-1)
    assert P.size == cfg.nvar * abi.ncell_all(cfg)
    shape = (cfg.ng[2], cfg.ng[1], cfg.ng[0])
    col, dcol = np.zeros(shape), np.zeros(shape)
    rc = load_library().pion_gpu_raytrace_host(C.byref(cfg), C.byref(abi.rt_source(src)), _p(P), _p(col), _p(dcol))
    if rc != 0:
        raise PionGpuError("raytrace_host", rc, rt_refused(cfg, src) or "invalid arguments")
    return col, dcol


def _partp(part):
    return None if part is None else C.byref(abi.rt_part(part))


def rt_part_refused(cfg, src, part):
    """pion_gpu_rt_part_refused: the text with which the ray tracer refuses `src` on the part `part` (an abi.RtPart,
    (plane_lo, global_planes, global_xmin) or None) of a slab run, or None.  Host only: needs no GPU."""
    t = load_library().pion_gpu_rt_part_refused(C.byref(cfg), C.byref(abi.rt_source(src)), _partp(part))
    return None if t is None else t.decode()


def rt_chain(cfg, src, part):
    """pion_gpu_rt_chain: (recv_side, send_lo, send_hi) -- the role of the rank that holds `part` in the trace of
    `src`: abi.RT_RECV_NONE / _BELOW / _ABOVE, and whether its lowest / highest own plane goes to the neighbour below /
    above.  Host only: needs no GPU."""
    r, lo, hi = C.c_int(-1), C.c_int(-1), C.c_int(-1)
    rc = load_library().pion_gpu_rt_chain(C.byref(cfg), C.byref(abi.rt_source(src)), _partp(part), C.byref(r),
                                          C.byref(lo), C.byref(hi))
    if rc != 0:
        raise PionGpuError("rt_chain", rc, rt_part_refused(cfg, src, part) or "invalid arguments")
    return r.value, lo.value, hi.value


def rt_plan_part(cfg, src, part):
    """pion_gpu_rt_plan_part: (launches, workgroups, workgroups_from_vertex) of the tiled kernel for `src` on `part`"""
    l, w, w0 = C.c_long(-1), C.c_long(-1), C.c_long(-1)
    rc = load_library().pion_gpu_rt_plan_part(C.byref(cfg), C.byref(abi.rt_source(src)), _partp(part), C.byref(l),
                                              C.byref(w), C.byref(w0))
    if rc != 0:
        raise PionGpuError("rt_plan_part", rc, rt_part_refused(cfg, src, part) or "invalid arguments")
    return l.value, w.value, w0.value


def raytrace_host_part(cfg, src, part, P, face_in=None):
    """pion_gpu_raytrace_host_part: (col, dcol) of the planes of `part`, each [nz][ny][nx] of cfg, from the host array
    P of that part and the plane `face_in` the neighbouring rank handed over (None where rt_chain says nothing is
    received).  Host only: needs no GPU."""
    P = np.ascontiguousarray(P, dtype=np.float64).reshape(-1)
    assert P.size == cfg.nvar * abi.ncell_all(cfg)
    shape = (cfg.ng[2], cfg.ng[1], cfg.ng[0])
    col, dcol = np.zeros(shape), np.zeros(shape)
    if face_in is not None:
        face_in = np.ascontiguousarray(face_in, dtype=np.float64).reshape(-1)
        assert face_in.size == col.size // shape[0 if cfg.ndim == 3 else 1]
    rc = load_library().pion_gpu_raytrace_host_part(C.byref(cfg), C.byref(abi.rt_source(src)), _partp(part), _p(P),
                                                    None if face_in is None else _p(face_in), _p(col), _p(dcol))
    if rc != 0:
        raise PionGpuError("raytrace_host_part", rc, rt_part_refused(cfg, src, part)
                           or "invalid arguments (no face where the chain hands one over?)")
    return col, dcol


def rows_windows(cfg, lo=0, hi=None, limit=None):
    """pion_gpu_rows_windows: the plane windows [(w_lo, w_hi), ...] the rows kernel takes for the on-grid planes
    [lo, hi) of the slab axis of `cfg` (hi None: all of them) under a limit of `limit` cells per launch (None: the
    default, 2^29); [] where the grid stays on the cell-per-thread kernel.  Host only: needs no GPU."""
    lib = load_library()
    if hi is None:
        hi = cfg.ng[cfg.ndim - 1]
    lim = 0 if limit is None else int(limit)
    n = lib.pion_gpu_rows_windows(C.byref(cfg), lim, lo, hi, 0, None, None)
    if n < 0:
        raise PionGpuError("rows_windows", n, "invalid arguments")
    w_lo, w_hi = (C.c_int * max(n, 1))(), (C.c_int * max(n, 1))()
    n = lib.pion_gpu_rows_windows(C.byref(cfg), lim, lo, hi, n, w_lo, w_hi)
    return [(w_lo[i], w_hi[i]) for i in range(n)]


def _p(a):
    return a.ctypes.data_as(_dp)


class HaloSpans(C.Structure):
    """pion_gpu_halo_spans_t (include/pion_gpu.h)"""
    _fields_ = [("send_lo", C.c_void_p), ("send_hi", C.c_void_p), ("recv_lo", C.c_void_p), ("recv_hi", C.c_void_p),
                ("count_per_var", C.c_long), ("var_stride", C.c_long), ("nvar", C.c_int)]


class GpuSim:
    """One pion_gpu handle (one GPU)."""

    def __init__(self, cfg, device=0, borrowed_handle=None):
        """borrowed_handle: wrap a handle that somebody else owns (pion_host::sim_control_gpu's, see
        pion_amd/host_rccl.py) -- set-up calls and timing only; close() then leaves it alone."""
        self.lib = load_library()
        self.cfg = cfg
        self.owner = borrowed_handle is None
        if borrowed_handle is not None:
            self.h = C.c_void_p(borrowed_handle)
        else:
            self.h = C.c_void_p()
            rc = self.lib.pion_gpu_create(C.byref(cfg), device, C.byref(self.h))
            if rc != 0:
                msg = self._err() if self.h else "invalid configuration"
                self.h = None
                raise PionGpuError("create", rc, msg)
        self.nvar = cfg.nvar
        self.ncell = abi.ncell_all(cfg)
        nga = abi.ng_all(cfg)
        self.shape = (cfg.nvar, nga[2], nga[1], nga[0])

    def _err(self):
        buf = C.create_string_buffer(512)
        self.lib.pion_gpu_last_error(self.h, buf, 512)
        return buf.value.decode()

    def _chk(self, rc, what):
        if rc != 0:
            raise PionGpuError(what, rc, self._err())

    def close(self):
        if getattr(self, "h", None):
            if self.owner:
                self.lib.pion_gpu_destroy(self.h)
            self.h = None

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # --- state
    def upload(self, P):
        P = np.ascontiguousarray(P, dtype=np.float64).reshape(-1)
        assert P.size == self.nvar * self.ncell
        self._chk(self.lib.pion_gpu_upload(self.h, _p(P)), "upload")

    def download(self, which=0):
        out = np.empty(self.nvar * self.ncell)
        self._chk(self.lib.pion_gpu_download(self.h, which, _p(out)), "download")
        return out.reshape(self.shape)

    def bind_device_state(self, dP_ptr, dPh_ptr):
        self._chk(self.lib.pion_gpu_bind_device_state(self.h, C.c_void_p(dP_ptr), C.c_void_p(dPh_ptr)),
                  "bind_device_state")

    def device_ptr(self, which):
        return self.lib.pion_gpu_device_ptr(self.h, which)

    def set_stream(self, stream_ptr):
        self._chk(self.lib.pion_gpu_set_stream(self.h, C.c_void_p(stream_ptr)), "set_stream")

    def set_comm_stream(self, stream_ptr):
        self._chk(self.lib.pion_gpu_set_comm_stream(self.h, C.c_void_p(stream_ptr)), "set_comm_stream")

    def synchronize(self):
        self._chk(self.lib.pion_gpu_synchronize(self.h), "synchronize")

    def set_wind_cells(self, idx, states):
        idx = np.ascontiguousarray(idx, dtype=np.int64)
        states = np.ascontiguousarray(states, dtype=np.float64)
        self._chk(self.lib.pion_gpu_set_wind_cells(self.h, idx.size, idx.ctypes.data_as(C.POINTER(C.c_long)),
                                                   _p(states)), "set_wind_cells")

    def add_wind_source(self, src):
        """pion_gpu_add_wind_source: src is a pion_amd.wind.WindSource; returns its id"""
        st, keep = src.to_c()
        i = C.c_int(-1)
        self._chk(self.lib.pion_gpu_add_wind_source(self.h, C.byref(st), C.byref(i)), "add_wind_source")
        del keep
        return i.value

    def add_rotating_wind_source(self, src):
        """pion_gpu_add_rotating_wind_source: src is a pion_amd.wind.WindSource of type ANGLE with an evolution
        table (its vcrit column) and xi; returns its id"""
        st, keep = src.to_c()
        vcrit = keep[-1].ctypes.data_as(_dp) if src.evolution is not None else None
        i = C.c_int(-1)
        self._chk(self.lib.pion_gpu_add_rotating_wind_source(self.h, C.byref(st), vcrit, src.xi, C.byref(i)),
                  "add_rotating_wind_source")
        del keep
        return i.value

    def get_wind_cells(self, sid):
        """pion_gpu_get_wind_cells: (cell ids, states[n, nvar]) of source `sid`"""
        n = C.c_long(0)
        self._chk(self.lib.pion_gpu_get_wind_cells(self.h, sid, C.byref(n), None, None), "get_wind_cells")
        idx = np.zeros(n.value, dtype=np.int64)
        st = np.zeros((n.value, self.nvar))
        self._chk(self.lib.pion_gpu_get_wind_cells(self.h, sid, C.byref(n), idx.ctypes.data_as(C.POINTER(C.c_long)),
                                                   _p(st)), "get_wind_cells")
        return idx, st

    def get_wind_source_pos(self, sid):
        """pion_gpu_get_wind_source_pos: the current position of source `sid` (3 floats)"""
        out = np.zeros(3)
        self._chk(self.lib.pion_gpu_get_wind_source_pos(self.h, sid, _p(out)), "get_wind_source_pos")
        return tuple(out)

    def get_flags(self):
        """pion_gpu_get_flags: the device's cell flags (uint8, ncell_all, cell-id order)"""
        out = np.zeros(self.ncell, dtype=np.uint8)
        self._chk(self.lib.pion_gpu_get_flags(self.h, out.ctypes.data), "get_flags")
        return out

    def get_hll_switch(self):
        """pion_gpu_get_hll_switch: the HLLD -> HLL switch per cell as the last stage's prepass left it (uint8, ncell_all)"""
        out = np.zeros(self.ncell, dtype=np.uint8)
        self._chk(self.lib.pion_gpu_get_hll_switch(self.h, out.ctypes.data), "get_hll_switch")
        return out

    def get_hcorr_eta(self, axis):
        """pion_gpu_get_hcorr_eta: the H-correction eta along `axis` per cell as the last stage's prepass left it
        (float64, ncell_all; the value of interface (c | c+1) at c)"""
        out = np.zeros(self.ncell)
        self._chk(self.lib.pion_gpu_get_hcorr_eta(self.h, int(axis), _p(out)), "get_hcorr_eta")
        return out

    def get_hll_screen_counts(self):
        """pion_gpu_get_hll_screen_counts: (active blocks, blocks) of the last prepass; (-1, 0): it was the dense one"""
        a, t = C.c_int(0), C.c_int(0)
        self._chk(self.lib.pion_gpu_get_hll_screen_counts(self.h, C.byref(a), C.byref(t)), "get_hll_screen_counts")
        return a.value, t.value

    def rows_windows(self):
        """pion_gpu_get_rows_windows: dict limit_cells, windows_whole_stage (1: one launch per stage; 0: the
        cell-per-thread kernel runs), launches_last_part (stage-kernel launches of the last stage part issued)"""
        lim, nw, nl = C.c_long(0), C.c_int(0), C.c_int(0)
        self._chk(self.lib.pion_gpu_get_rows_windows(self.h, C.byref(lim), C.byref(nw), C.byref(nl)), "get_rows_windows")
        return {"limit_cells": lim.value, "windows_whole_stage": nw.value, "launches_last_part": nl.value}

    def set_jet(self, jetradius, jetstate):
        st = np.ascontiguousarray(jetstate, dtype=np.float64)
        self._chk(self.lib.pion_gpu_set_jet(self.h, int(jetradius), _p(st)), "set_jet")

    def set_cooling_tables(self, T, tabs, slopes):
        T = np.ascontiguousarray(T, dtype=np.float64)
        tabs = np.ascontiguousarray(tabs, dtype=np.float64)
        slopes = np.ascontiguousarray(slopes, dtype=np.float64)
        self._chk(self.lib.pion_gpu_set_cooling_tables(self.h, T.size, _p(T), _p(tabs), _p(slopes)),
                  "set_cooling_tables")

    def set_cooling_curve(self, logT, logL, c, min_slope, max_slope):
        """The total-CIE curve of EP.cooling = 4..7, as cooling.build_curve returns it."""
        logT = np.ascontiguousarray(logT, dtype=np.float64)
        logL = np.ascontiguousarray(logL, dtype=np.float64)
        c = np.ascontiguousarray(c, dtype=np.float64)
        if not (logT.shape == logL.shape == c.shape and logT.ndim == 1):
            raise ValueError("logT, logL and c must be 1-D arrays of one length")
        self._chk(self.lib.pion_gpu_set_cooling_curve(self.h, logT.size, _p(logT), _p(logL), _p(c), float(min_slope),
                                                      float(max_slope)), "set_cooling_curve")

    # --- the hot path
    def update_bcs(self, simtime=0.0, cstep=2, maxstep=2, assign=0):
        self._chk(self.lib.pion_gpu_update_bcs(self.h, simtime, cstep, maxstep, assign), "update_bcs")

    def calc_dt(self):
        a, b = C.c_double(), C.c_double()
        self._chk(self.lib.pion_gpu_calc_dt(self.h, C.byref(a), C.byref(b)), "calc_dt")
        return a.value, b.value

    def set_glm_speeds(self, dt, dx, cr):
        self._chk(self.lib.pion_gpu_set_glm_speeds(self.h, dt, dx, cr), "set_glm_speeds")

    def stage(self, dt, space_ooa, is_full):
        self._chk(self.lib.pion_gpu_stage(self.h, dt, space_ooa, is_full), "stage")

    def stage_part(self, dt, space_ooa, is_full, part):
        self._chk(self.lib.pion_gpu_stage_part(self.h, dt, space_ooa, is_full, part), "stage_part")

    def advance_time(self, dt, simtime):
        self._chk(self.lib.pion_gpu_advance_time(self.h, dt, simtime), "advance_time")

    # --- slab halos
    def halo_count(self):
        return self.lib.pion_gpu_halo_count(self.h)

    def pack_halo(self, which, face, dbuf_ptr):
        self._chk(self.lib.pion_gpu_pack_halo(self.h, which, face, C.c_void_p(dbuf_ptr)), "pack_halo")

    def unpack_halo(self, which, face, dbuf_ptr):
        self._chk(self.lib.pion_gpu_unpack_halo(self.h, which, face, C.c_void_p(dbuf_ptr)), "unpack_halo")

    def halo_spans(self, which):
        """pion_gpu_halo_spans: device addresses of the nbc planes (2-D: rows) next to the two faces of the slab axis
        of array `which` (0 = P, 1 = Ph): dict send_lo / send_hi / recv_lo / recv_hi (addresses), count_per_var,
        var_stride (doubles), nvar"""
        sp = HaloSpans()
        self._chk(self.lib.pion_gpu_halo_spans(self.h, which, C.byref(sp)), "halo_spans")
        return {k: getattr(sp, k) for k, _ in HaloSpans._fields_}

    def halo_begin(self):
        self._chk(self.lib.pion_gpu_halo_begin(self.h), "halo_begin")

    def halo_end(self):
        self._chk(self.lib.pion_gpu_halo_end(self.h), "halo_end")

    # --- on-grid planes (snapshots)
    def ongrid_count(self, planes):
        """pion_gpu_ongrid_count: doubles in a buffer of `planes` planes of the slab axis, all variables"""
        return self.lib.pion_gpu_ongrid_count(self.h, int(planes))

    def pack_ongrid(self, which, plane_lo, plane_hi, dbuf_ptr):
        """pion_gpu_pack_ongrid: on-grid cells of planes [plane_lo, plane_hi) of array `which` into the device buffer
        at dbuf_ptr, [nvar][planes][ny][nx]; enqueued on the handle's stream (synchronize() before reading it)"""
        self._chk(self.lib.pion_gpu_pack_ongrid(self.h, which, plane_lo, plane_hi, C.c_void_p(dbuf_ptr)), "pack_ongrid")

    def fits_images(self):
        """pion_gpu_fits_images: the names of the images a FITS file of this handle holds, in file order (no device
        call)"""
        n = C.c_int(0)
        names = ((C.c_char * 16) * (abi.PION_MAX_NVAR + 3))()
        self._chk(self.lib.pion_gpu_fits_images(self.h, names, C.byref(n)), "fits_images")
        return [names[i].value.decode() for i in range(n.value)]

    def fits_count(self, planes):
        """pion_gpu_fits_count: elements (8 bytes each) in a buffer of `planes` planes, all images"""
        return self.lib.pion_gpu_fits_count(self.h, int(planes))

    def pack_fits(self, plane_lo, plane_hi, dbuf_ptr):
        """pion_gpu_pack_fits: the images of planes [plane_lo, plane_hi) of P into the device buffer at dbuf_ptr,
        [nimage][planes][ny][nx], every element a big-endian double (view it as dtype '>f8'), B and divB times
        sqrt(4 pi); enqueued on the compute stream.  Call it after update_bcs: divB reads ghost cells."""
        self._chk(self.lib.pion_gpu_pack_fits(self.h, plane_lo, plane_hi, C.c_void_p(dbuf_ptr)), "pack_fits")

    def fits_prim_count(self, planes):
        """pion_gpu_fits_prim_count: elements (8 bytes each) of the primitive images of `planes` planes"""
        return self.lib.pion_gpu_fits_prim_count(self.h, int(planes))

    def unpack_fits(self, plane_lo, plane_hi, dbuf_ptr):
        """pion_gpu_unpack_fits: the big-endian elements [nvar][planes][ny][nx] of the primitive images at dbuf_ptr
        into the on-grid cells of planes [plane_lo, plane_hi) of P and Ph, B times 1/sqrt(4 pi); ghost cells are left
        alone; enqueued on the compute stream"""
        self._chk(self.lib.pion_gpu_unpack_fits(self.h, plane_lo, plane_hi, C.c_void_p(dbuf_ptr)), "unpack_fits")

    def unpack_fits_status(self):
        """pion_gpu_unpack_fits_status: synchronises; the number of elements unpacked since the last call that were
        not finite or the reference's null value -1e99 (the counter is cleared)"""
        n = C.c_long(-1)
        self._chk(self.lib.pion_gpu_unpack_fits_status(self.h, C.byref(n)), "unpack_fits_status")
        return n.value

    # --- ray-traced column densities
    def add_rt_source(self, src, part=None):
        """pion_gpu_add_rt_source: (id, pos_used) -- a finite source is moved to the nearest cell vertex per axis.
        part (an abi.RtPart or (plane_lo, global_planes, global_xmin)): pion_gpu_add_rt_source_part, the handle is a
        slab of a decomposed run and src a source of the whole domain"""
        sid, pos = C.c_int(-1), (C.c_double * 3)()
        if part is None:
            self._chk(self.lib.pion_gpu_add_rt_source(self.h, C.byref(abi.rt_source(src)), C.byref(sid), pos), "add_rt_source")
        else:
            self._chk(self.lib.pion_gpu_add_rt_source_part(self.h, C.byref(abi.rt_source(src)), C.byref(abi.rt_part(part)),
                                                           C.byref(sid), pos), "add_rt_source_part")
        return sid.value, tuple(pos)

    def raytrace_part(self, sid, which=0, face_in_ptr=None, face_out_lo_ptr=None, face_out_hi_ptr=None):
        """pion_gpu_raytrace_part: the columns of source sid alone; face_in_ptr: device buffer of the plane received
        (None where nothing is), face_out_*_ptr: device buffers for the lowest and highest own plane of col (None: not
        written), each rt_count(1) doubles; enqueued"""
        self._chk(self.lib.pion_gpu_raytrace_part(self.h, int(which), int(sid), C.c_void_p(face_in_ptr),
                                                  C.c_void_p(face_out_lo_ptr), C.c_void_p(face_out_hi_ptr)), "raytrace_part")

    def raytrace(self, which=0):
        """pion_gpu_raytrace: the columns of every source from array `which` (0 = P, 1 = Ph); enqueued"""
        self._chk(self.lib.pion_gpu_raytrace(self.h, int(which)), "raytrace")

    def rt_columns(self, sid, what=0):
        """pion_gpu_rt_columns: col (what = 0) or dcol (1) of source sid, [nz][ny][nx]; synchronises"""
        out = np.empty((self.cfg.ng[2], self.cfg.ng[1], self.cfg.ng[0]))
        self._chk(self.lib.pion_gpu_rt_columns(self.h, int(sid), int(what), _p(out)), "rt_columns")
        return out

    def rt_count(self, planes):
        """pion_gpu_rt_count: doubles of `planes` planes of the slab axis of one column array"""
        return self.lib.pion_gpu_rt_count(self.h, int(planes))

    def pack_columns(self, sid, what, plane_lo, plane_hi, dbuf_ptr):
        """pion_gpu_pack_columns: the planes [plane_lo, plane_hi) of a column array as big-endian doubles at dbuf_ptr"""
        self._chk(self.lib.pion_gpu_pack_columns(self.h, int(sid), int(what), int(plane_lo), int(plane_hi),
                                                 C.c_void_p(dbuf_ptr)), "pack_columns")

    def project_count(self, axis, nfields):
        """pion_gpu_project_count: doubles one project() call writes, [nfields][NJ][NI]; raises for a grid or an axis
        the projection refuses (no device call)"""
        n = self.lib.pion_gpu_project_count(self.h, int(axis), int(nfields))
        if n < 0:
            raise PionGpuError("project_count", n, self._err())
        return n

    def project(self, axis, fields, which=0, dbuf_ptr=None):
        """pion_gpu_project: the projected images of array `which` along `axis` (0, 1, 2 on a 3-D Cartesian grid:
        column sums times dx; abi.PROJ_AXIS_PERP on a cylindrical (z,R) grid: the perpendicular Abel integral).
        fields: what abi.proj_fields takes -- (name, a, var, coef, b) for coef rho^a T^b w.  With dbuf_ptr the images
        go into that device buffer, enqueued on the compute stream; without it they are returned as an ndarray
        [nfields][NJ][NI] (a torch buffer in between)."""
        arr = fields if isinstance(fields, C.Array) else abi.proj_fields(fields)
        nf = len(fields)
        if dbuf_ptr is not None:
            self._chk(self.lib.pion_gpu_project(self.h, int(which), int(axis), nf, arr, C.c_void_p(dbuf_ptr)), "project")
            return None
        n = self.lib.pion_gpu_project_count(self.h, int(axis), max(1, min(nf, abi.PROJ_MAX_FIELDS)))
        import torch
        buf = torch.empty((max(n, 1),), dtype=torch.float64, device="cuda:%d" % torch.cuda.current_device())
        self._chk(self.lib.pion_gpu_project(self.h, int(which), int(axis), nf, arr, C.c_void_p(buf.data_ptr())), "project")
        self.synchronize()
        return buf.cpu().numpy().reshape(nf, -1, self.project_shape(axis)[1])

    def project_part_count(self, axis, nfields, part):
        """pion_gpu_project_part_count: doubles of the image of the WHOLE domain a project_part() call works in; part:
        an abi.ProjPart or (plane_lo, global_planes, last, global_xmin).  Raises for what the call refuses"""
        n = self.lib.pion_gpu_project_part_count(self.h, int(axis), int(nfields), C.byref(abi.proj_part(part)))
        if n < 0:
            raise PionGpuError("project_part_count", n, self._err())
        return n

    def project_part(self, axis, fields, part, which=0, dimg_ptr=None, image=None):
        """pion_gpu_project_part: this handle's part of a slab run's image (the planes [plane_lo, plane_lo + n) of the
        slab axis out of global_planes), added into the image of the whole domain that the rank below left.  With
        dimg_ptr the image is that device buffer, in/out, enqueued on the compute stream.  Without it `image` is the
        image so far as an ndarray [nfields][NJ_global][NI_global] (None: zeros, rank 0) and the new one is returned.
        After the part with last = 1 the image is == project() on one handle of the whole domain."""
        arr = fields if isinstance(fields, C.Array) else abi.proj_fields(fields)
        nf = len(fields)
        p = abi.proj_part(part)
        if dimg_ptr is not None:
            self._chk(self.lib.pion_gpu_project_part(self.h, int(which), int(axis), nf, arr, C.byref(p),
                                                     C.c_void_p(dimg_ptr)), "project_part")
            return None
        n = self.project_part_count(axis, max(1, min(nf, abi.PROJ_MAX_FIELDS)), p)
        import torch
        dev = "cuda:%d" % torch.cuda.current_device()
        if image is None:
            buf = torch.zeros((n,), dtype=torch.float64, device=dev)
        else:
            buf = torch.from_numpy(np.ascontiguousarray(image, dtype=np.float64).reshape(-1)).to(dev)
        self._chk(self.lib.pion_gpu_project_part(self.h, int(which), int(axis), nf, arr, C.byref(p),
                                                 C.c_void_p(buf.data_ptr())), "project_part")
        self.synchronize()
        return buf.cpu().numpy().reshape(nf, -1, self.project_shape(axis)[1])

    def project_angle_count(self, angle_deg, nfields):
        """pion_gpu_project_angle_count: (doubles one project_angle() call writes, n_extra) -- [nfields][NR][NI] with
        NI = NZ + 2 n_extra; raises for a grid or an angle the inclined projection refuses (no device call)"""
        ne = C.c_int(-1)
        n = self.lib.pion_gpu_project_angle_count(self.h, float(angle_deg), int(nfields), C.byref(ne))
        if n < 0:
            raise PionGpuError("project_angle_count", n, self._err())
        return n, ne.value

    def project_angle(self, angle_deg, fields, which=0, dbuf_ptr=None):
        """pion_gpu_project_angle: the images of a cylindrical (z,R) grid seen at angle_deg (0 < angle_deg < 90) to its
        axis, every pixel's ray walked from cell to cell (the reference's angle_projection.cpp).  fields: as project()
        takes them.  With dbuf_ptr the images go into that device buffer, enqueued on the compute stream; without it
        they are returned as an ndarray [nfields][NR][NI], and a pixel whose ray loop reached its trip limit raises."""
        arr = fields if isinstance(fields, C.Array) else abi.proj_fields(fields)
        nf = len(fields)
        if dbuf_ptr is not None:
            self._chk(self.lib.pion_gpu_project_angle(self.h, int(which), float(angle_deg), nf, arr, C.c_void_p(dbuf_ptr)),
                      "project_angle")
            return None
        n = self.lib.pion_gpu_project_angle_count(self.h, float(angle_deg), max(1, min(nf, abi.PROJ_MAX_FIELDS)), None)
        import torch
        buf = torch.empty((max(n, 1),), dtype=torch.float64, device="cuda:%d" % torch.cuda.current_device())
        self._chk(self.lib.pion_gpu_project_angle(self.h, int(which), float(angle_deg), nf, arr, C.c_void_p(buf.data_ptr())),
                  "project_angle")
        ncapped = self.project_angle_status()
        if ncapped:
            raise PionGpuError("project_angle", abi.E_INVAL, "%d pixel(s) reached the trip limit of their ray loop" % ncapped)
        return buf.cpu().numpy().reshape(nf, self.cfg.ng[1], -1)

    def project_angle_status(self):
        """pion_gpu_project_angle_status: synchronises; the pixels since the last call whose ray loop reached its trip
        limit (none is expected), cleared"""
        n = C.c_long(-1)
        self._chk(self.lib.pion_gpu_project_angle_status(self.h, C.byref(n)), "project_angle_status")
        return n.value

    def project_shape(self, axis):
        """(NJ, NI) of an image along `axis`"""
        ng = list(self.cfg.ng)
        if self.cfg.coord_sys == 2:
            return ng[1], ng[0]
        return (ng[2], ng[1]) if axis == 0 else ((ng[2], ng[0]) if axis == 1 else (ng[1], ng[0]))

    def unpack_ongrid(self, plane_lo, plane_hi, dbuf_ptr):
        """pion_gpu_unpack_ongrid: the reverse, into P and Ph; ghost cells and other planes are left alone"""
        self._chk(self.lib.pion_gpu_unpack_ongrid(self.h, plane_lo, plane_hi, C.c_void_p(dbuf_ptr)), "unpack_ongrid")

    # --- seams
    def interface_flux(self, axis, Pl, Pr, aux=None, dt=1.0):
        Pl = np.ascontiguousarray(Pl, dtype=np.float64)
        Pr = np.ascontiguousarray(Pr, dtype=np.float64)
        n = Pl.shape[0]
        if aux is None:
            aux = np.zeros((n, 4))
        aux = np.ascontiguousarray(aux, dtype=np.float64)
        F = np.zeros((n, self.nvar))
        Ps = np.zeros((n, self.nvar))
        self._chk(self.lib.pion_gpu_interface_flux(self.h, n, axis, dt, _p(Pl), _p(Pr), _p(aux), _p(F), _p(Ps)),
                  "interface_flux")
        return F, Ps

    def cell_advance(self, Pin, dU, fv_dt=0.0):
        """pion_gpu_cell_advance: CellAdvanceTime + the temperature ceiling of n cells (Pin, dU: [n, nvar])"""
        Pin = np.ascontiguousarray(Pin, dtype=np.float64)
        dU = np.ascontiguousarray(dU, dtype=np.float64)
        assert Pin.ndim == 2 and Pin.shape[1] == self.nvar and dU.shape == Pin.shape
        out = np.zeros_like(Pin)
        self._chk(self.lib.pion_gpu_cell_advance(self.h, Pin.shape[0], fv_dt, _p(Pin), _p(dU), _p(out), None),
                  "cell_advance")
        return out

    def cell_timestep(self, Pin):
        """pion_gpu_cell_advance, the time step alone: CellTimeStep of n cells"""
        Pin = np.ascontiguousarray(Pin, dtype=np.float64)
        assert Pin.ndim == 2 and Pin.shape[1] == self.nvar
        out = np.zeros(Pin.shape[0])
        self._chk(self.lib.pion_gpu_cell_advance(self.h, Pin.shape[0], 0.0, _p(Pin), None, None, _p(out)),
                  "cell_timestep")
        return out

    def cooling_update(self, Pin, dt):
        Pin = np.ascontiguousarray(Pin, dtype=np.float64)
        out = np.zeros_like(Pin)
        self._chk(self.lib.pion_gpu_cooling_update(self.h, Pin.shape[0], dt, _p(Pin), _p(out)), "cooling_update")
        return out

    def cooling_edot(self, rho, T):
        rho = np.ascontiguousarray(rho, dtype=np.float64)
        T = np.ascontiguousarray(T, dtype=np.float64)
        out = np.zeros_like(rho)
        self._chk(self.lib.pion_gpu_cooling_edot(self.h, rho.size, _p(rho), _p(T), _p(out)), "cooling_edot")
        return out

    def cooling_curve_eval(self, T):
        """Lambda(T) of the curve set by set_cooling_curve, through the cooling kernels' own function"""
        T = np.ascontiguousarray(T, dtype=np.float64)
        out = np.zeros_like(T)
        self._chk(self.lib.pion_gpu_cooling_curve_eval(self.h, T.size, _p(T), _p(out)), "cooling_curve_eval")
        return out

    def cooling_timescale(self, Pin):
        Pin = np.ascontiguousarray(Pin, dtype=np.float64)
        out = np.zeros(Pin.shape[0])
        self._chk(self.lib.pion_gpu_cooling_timescale(self.h, Pin.shape[0], _p(Pin), _p(out)), "cooling_timescale")
        return out

    def enable_timing(self, on=True):
        self._chk(self.lib.pion_gpu_enable_timing(self.h, int(on)), "enable_timing")

    def get_timing(self):
        out = np.zeros(8)
        self._chk(self.lib.pion_gpu_get_timing(self.h, _p(out), 8), "get_timing")
        return {"stage_ms": out[0], "prepass_ms": out[1], "bc_ms": out[2], "dt_ms": out[3],
                "stage_n": int(out[4]), "prepass_n": int(out[5]), "bc_n": int(out[6]), "dt_n": int(out[7])}
