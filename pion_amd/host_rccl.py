"""ctypes view of the C++ host layer above the C-ABI (pion_amd/host/libpion_host.so):
pion_host::sim_control_gpu (the Time_Int / calculate_timestep / advance_time mirror) and
pion_host::slab_comm_rccl (z-slab halo exchange + time-step reduction over RCCL, driven from C++:
ncclGroupStart / ncclSend / ncclRecv / ncclGroupEnd on the communication stream, ncclAllReduce(ncclMin) on
the device-resident minima).  Python only hands over configuration, the initial state and -- for N > 1 -- the
128-byte ncclUniqueId it broadcast; every launch, transfer and reduction of the time loop is issued from C++.
"""
import ctypes as C
import os

import numpy as np

from . import abi

_HERE = os.path.dirname(os.path.abspath(__file__))
_dp = C.POINTER(C.c_double)
_host = None

UNIQUE_ID_BYTES = 128
FILE_PIONRAW, FILE_FITS = 0, 1   # PION_HOST_FILE_* (include/pion_host.h)


class SnapshotInfo(C.Structure):
    """pion_host_snapshot_info (include/pion_host.h)"""
    _fields_ = [("t_start", C.c_double), ("t_finish", C.c_double), ("t_sim", C.c_double), ("min_timestep", C.c_double),
                ("last_dt", C.c_double), ("opfreq_time", C.c_double), ("next_optime", C.c_double),
                ("t_step", C.c_int), ("op_criterion", C.c_int), ("op_freq", C.c_int),
                ("rank", C.c_int), ("world", C.c_int), ("slab_lo", C.c_int), ("slab_n", C.c_int),
                ("data_offset", C.c_long), ("outfile", C.c_char * 256)]


def _read_header(entry, path):
    lib = load_host_library()
    cfg, info = abi.PionGpuConfig(), SnapshotInfo()
    rc = getattr(lib, entry)(os.fsencode(path), C.byref(cfg), C.byref(info))
    if rc != 0:
        buf = C.create_string_buffer(600)
        lib.pion_host_sim_last_error(None, buf, 600)
        raise ValueError("%s rc=%d: %s" % (entry, rc, buf.value.decode(errors="replace")))
    d = {k: getattr(info, k) for k, _ in SnapshotInfo._fields_}
    d["outfile"] = d["outfile"].decode()
    return cfg, d


def read_snapshot_header(path):
    """pion_host_snapshot_read_header: (global cfg, dict of pion_host_snapshot_info); host only, needs no device"""
    return _read_header("pion_host_snapshot_read_header", path)


def read_fits_header(path):
    """pion_host_fits_read_header: the same of a FITS file (data_offset is 0)"""
    return _read_header("pion_host_fits_read_header", path)


def is_fits(path):
    """True where the file begins as a FITS file does (SIMPLE  =), whatever its name; False where it begins otherwise
    (the PIONRAW2 reader checks its own magic); None where it cannot be read (the C++ reader says so)"""
    try:
        with open(path, "rb") as f:
            return f.read(9) == b"SIMPLE  ="
    except OSError:
        return None


def load_host_library():
    global _host
    if _host is not None:
        return _host
    # PION_HOST_LIB: an alternative build of the same library (A/B runs, with PION_GPU_LIB naming the one it was linked to)
    path = os.environ.get("PION_HOST_LIB") or os.path.join(_HERE, "host", "libpion_host.so")
    if not os.path.exists(path):
        raise ImportError("%s not found: build it with `make -C pion_amd/host`" % path)
    abi.share_torch_hip_runtime()
    # libpion_host.so NEEDs "libpion_gpu.so" (soname): load the library this process is meant to use first, so
    # that an alternative build named by PION_GPU_LIB (A/B runs) also serves the C++ time loop
    C.CDLL(abi.library_path(), mode=C.RTLD_GLOBAL)
    h = C.CDLL(path)
    h.pion_host_sim_create.argtypes = [C.POINTER(abi.PionGpuConfig), C.c_int, C.POINTER(C.c_void_p)]
    h.pion_host_sim_create_backend.argtypes = [C.POINTER(abi.PionGpuConfig), C.c_int, C.c_void_p, C.POINTER(C.c_void_p)]
    h.pion_host_comm_shm_create.argtypes = [C.c_int, C.c_int, C.c_int, C.c_char_p, C.c_void_p, C.POINTER(C.c_void_p)]
    h.pion_host_sim_destroy.argtypes = [C.c_void_p]
    h.pion_host_sim_destroy.restype = None
    h.pion_host_sim_handle.argtypes = [C.c_void_p]
    h.pion_host_sim_handle.restype = C.c_void_p
    h.pion_host_sim_init.argtypes = [C.c_void_p, _dp, C.c_double, C.c_double, C.c_double]
    h.pion_host_sim_time_int.argtypes = [C.c_void_p, C.c_int, _dp, _dp]
    h.pion_host_sim_set_time.argtypes = [C.c_void_p, C.c_int, C.c_double]
    h.pion_host_sim_step.argtypes = [C.c_void_p, _dp]
    h.pion_host_sim_download.argtypes = [C.c_void_p, C.c_int, _dp]
    h.pion_host_sim_set_comm.argtypes = [C.c_void_p, C.c_void_p]
    h.pion_host_sim_finish_halo.argtypes = [C.c_void_p]
    h.pion_host_sim_last_error.argtypes = [C.c_void_p, C.c_char_p, C.c_int]
    h.pion_host_sim_add_wind_source.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(C.c_int)]
    if hasattr(h, "pion_host_sim_set_output"):   # (an older build swapped in for A/B runs has no snapshot entries)
        h.pion_host_sim_set_output.argtypes = [C.c_void_p, C.c_char_p, C.c_int, C.c_int, C.c_double, C.c_int]
        h.pion_host_sim_set_slab_extent.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int]
        h.pion_host_sim_write_snapshot.argtypes = [C.c_void_p, C.c_char_p]
        h.pion_host_sim_read_snapshot.argtypes = [C.c_void_p, C.POINTER(C.c_char_p), C.c_int]
        h.pion_host_snapshot_read_header.argtypes = [C.c_char_p, C.POINTER(abi.PionGpuConfig), C.POINTER(SnapshotInfo)]
        h.pion_host_sim_get_time.argtypes = [C.c_void_p, _dp]
    if hasattr(h, "pion_host_sim_write_fits"):   # (likewise)
        h.pion_host_sim_write_fits.argtypes = [C.c_void_p, C.c_char_p]
        h.pion_host_sim_set_output_filetype.argtypes = [C.c_void_p, C.c_int]
    if hasattr(h, "pion_host_sim_read_fits"):   # (likewise)
        h.pion_host_sim_read_fits.argtypes = [C.c_void_p, C.POINTER(C.c_char_p), C.c_int]
        h.pion_host_fits_read_header.argtypes = [C.c_char_p, C.POINTER(abi.PionGpuConfig), C.POINTER(SnapshotInfo)]
    if hasattr(h, "pion_host_sim_write_projection"):   # (likewise)
        h.pion_host_sim_write_projection.argtypes = [C.c_void_p, C.c_char_p, C.c_int, C.c_int, C.c_void_p]
        h.pion_host_sim_set_projection_output.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p]
    if hasattr(h, "pion_host_sim_add_rt_source"):   # (likewise)
        h.pion_host_sim_add_rt_source.argtypes = [C.c_void_p, C.POINTER(abi.RtSource), C.POINTER(C.c_int), _dp]
        h.pion_host_sim_write_columns.argtypes = [C.c_void_p, C.c_char_p]
        h.pion_host_sim_set_column_output.argtypes = [C.c_void_p, C.c_int]
    if hasattr(h, "pion_host_project_part_on_host"):   # (likewise)
        h.pion_host_project_part_refused.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
        h.pion_host_project_part_refused.restype = C.c_char_p
        h.pion_host_project_on_host.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, _dp, _dp]
        h.pion_host_project_part_on_host.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, _dp, _dp]
    if hasattr(h, "pion_host_sim_write_projection_angle"):   # (likewise)
        h.pion_host_sim_write_projection_angle.argtypes = [C.c_void_p, C.c_char_p, C.c_double, C.c_int, C.c_void_p]
        h.pion_host_sim_write_projection_angle_trips.argtypes = [C.c_void_p, C.c_char_p, C.c_double, C.c_int, C.c_void_p, C.c_int]
        h.pion_host_sim_set_projection_angle_output.argtypes = [C.c_void_p, C.c_double, C.c_int, C.c_void_p]
        h.pion_host_project_angle_count.argtypes = [C.c_void_p, C.c_double, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_char_p)]
        h.pion_host_project_angle_count.restype = C.c_long
        h.pion_host_project_angle_on_host.argtypes = [C.c_void_p, C.c_double, C.c_int, C.c_void_p, _dp, _dp]
        h.pion_host_project_angle_rule.argtypes = [C.c_void_p, C.c_double, C.c_int, C.c_int, C.c_void_p, _dp, _dp,
                                                   C.POINTER(C.c_long), _dp, _dp]
    h.pion_host_comm_unique_id.argtypes = [C.c_void_p]
    h.pion_host_comm_create.argtypes = [C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.POINTER(C.c_void_p)]
    h.pion_host_comm_destroy.argtypes = [C.c_void_p]
    h.pion_host_comm_destroy.restype = None
    _host = h
    return h


def new_unique_id():
    """ncclGetUniqueId on this rank (rank 0 calls it and broadcasts the 128 bytes)"""
    buf = (C.c_char * UNIQUE_ID_BYTES)()
    if load_host_library().pion_host_comm_unique_id(buf) != 0:
        raise RuntimeError("ncclGetUniqueId failed")
    return bytes(buf)


class HostSim:
    """pion_host::sim_control_gpu, optionally with a slab communicator: pion_host::slab_comm_rccl (unique_id: the
    128-byte ncclUniqueId) or pion_host::slab_comm_shm (shm_name: POSIX shared-memory name common to the ranks,
    "/name" -- the host-staged transport).  backend: address of a pion_backend table (pion_amd/host/pion_backend.h);
    None = libpion_gpu.so, the product's only backend (tests hand in the oracle's)."""

    def __init__(self, cfg, device=0, rank=0, world=1, periodic_z=True, unique_id=None, shm_name=None, backend=None):
        self.lib = load_host_library()
        self.cfg = cfg
        self.s = C.c_void_p()
        self.comm = C.c_void_p()
        if self.lib.pion_host_sim_create_backend(C.byref(cfg), device, backend, C.byref(self.s)) != 0:
            raise RuntimeError("pion_host_sim_create failed: " + self.last_error())
        if shm_name is not None:
            rc = self.lib.pion_host_comm_shm_create(rank, world, 1 if periodic_z else 0, shm_name.encode(), backend,
                                                    C.byref(self.comm))
            if rc != 0:
                self.close()
                raise RuntimeError("pion_host_comm_shm_create failed rc=%d" % rc)
            rc = self.lib.pion_host_sim_set_comm(self.s, self.comm)
            if rc != 0:
                self.close()
                raise RuntimeError("pion_host_sim_set_comm failed rc=%d" % rc)
        elif unique_id is not None:
            idb = (C.c_char * UNIQUE_ID_BYTES).from_buffer_copy(unique_id)
            # RCCL prints a version banner on stdout when a communicator is created: send it to stderr
            # (bench.py's stdout carries exactly one JSON line)
            import sys
            sys.stdout.flush()
            saved = os.dup(1)
            os.dup2(2, 1)
            try:
                rc = self.lib.pion_host_comm_create(rank, world, 1 if periodic_z else 0, idb, device, C.byref(self.comm))
            finally:
                os.dup2(saved, 1)
                os.close(saved)
            if rc != 0:
                self.close()
                raise RuntimeError("pion_host_comm_create failed")
            rc = self.lib.pion_host_sim_set_comm(self.s, self.comm)
            if rc != 0:
                self.close()
                raise RuntimeError("pion_host_sim_set_comm failed rc=%d" % rc)
        nga = abi.ng_all(cfg)
        self.shape = (cfg.nvar, nga[2], nga[1], nga[0])

    def last_error(self):
        buf = C.create_string_buffer(600)
        self.lib.pion_host_sim_last_error(self.s, buf, 600)
        return buf.value.decode(errors="replace")

    def gpu_handle(self):
        return self.lib.pion_host_sim_handle(self.s)

    def set_cooling_curve(self, logT, logL, c, min_slope, max_slope):
        """The total-CIE curve of EP.cooling = 4..7 (cooling.build_curve) on the loop's device handle: before init()
        or restart(), as the tables of EP.cooling = 8."""
        from . import lib as gpu_lib
        gpu_lib.GpuSim(self.cfg, 0, borrowed_handle=self.gpu_handle()).set_cooling_curve(logT, logL, c, min_slope,
                                                                                       max_slope)

    def init(self, P, simtime=0.0, finishtime=1e300, first_step_dt_limit=None, timestep=0, last_dt=1e100):
        """sim_init::Init; on a restart pass the snapshot's simtime / timestep / last_dt"""
        self.lib.pion_host_sim_set_time(self.s, int(timestep), float(last_dt))
        Pc = np.ascontiguousarray(P, dtype=np.float64).reshape(-1)
        rc = self.lib.pion_host_sim_init(self.s, Pc.ctypes.data_as(_dp), simtime, finishtime,
                                         -1.0 if first_step_dt_limit is None else first_step_dt_limit)
        if rc != 0:
            raise RuntimeError("pion_host_sim_init rc=%d: %s" % (rc, self.last_error()))

    def step(self):
        dt = C.c_double()
        rc = self.lib.pion_host_sim_step(self.s, C.byref(dt))
        if rc != 0:
            raise RuntimeError("pion_host_sim_step rc=%d: %s" % (rc, self.last_error()))
        return dt.value

    def finish_halo(self):
        rc = self.lib.pion_host_sim_finish_halo(self.s)
        if rc != 0:
            raise RuntimeError("pion_host_sim_finish_halo rc=%d" % rc)

    def time_int(self, nsteps):
        t, ldt = C.c_double(), C.c_double()
        n = self.lib.pion_host_sim_time_int(self.s, nsteps, C.byref(t), C.byref(ldt))
        if n < 0:
            raise RuntimeError("pion_host_sim_time_int: " + self.last_error())
        return n, t.value, ldt.value

    def add_wind_source(self, src):
        """pion_host_sim_add_wind_source: a device-built source (pion_amd.wind.WindSource, not a rotating one) and its
        first-step limit; before init() or restart().  Returns its id."""
        st, keep = src.to_c()
        i = C.c_int(-1)
        rc = self.lib.pion_host_sim_add_wind_source(self.s, C.byref(st), C.byref(i))
        del keep
        if rc != 0:
            raise RuntimeError("pion_host_sim_add_wind_source rc=%d: %s" % (rc, self.last_error()))
        return i.value

    def set_output(self, outfile_base, op_criterion=0, opfreq=0, opfreq_time=0.0, checkpoint_freq=0):
        """SimPM.outFileBase / op_criterion / opfreq / opfreq_time / checkpoint_freq: from now on time_int writes
        <base>_<rank>.<step>.pionraw snapshots and checkpoints (pion_host_sim_set_output).  After init(), before
        restart()."""
        rc = self.lib.pion_host_sim_set_output(self.s, os.fsencode(outfile_base), int(op_criterion), int(opfreq),
                                               float(opfreq_time), int(checkpoint_freq))
        if rc != 0:
            raise ValueError("pion_host_sim_set_output rc=%d (op_criterion 0 or 1, opfreq_time > 0 with criterion 1)" % rc)

    def set_slab_extent(self, global_planes, plane_lo, bc_lo, bc_hi):
        """where this rank's slab sits in the global problem, and the global problem's two slab-axis faces (abi.BC_*)"""
        rc = self.lib.pion_host_sim_set_slab_extent(self.s, int(global_planes), int(plane_lo), int(bc_lo), int(bc_hi))
        if rc != 0:
            raise ValueError("pion_host_sim_set_slab_extent rc=%d" % rc)

    def write_snapshot(self, path):
        """the PIONRAW2 file of this sim's on-grid cells (pion_host_sim_write_snapshot)"""
        rc = self.lib.pion_host_sim_write_snapshot(self.s, os.fsencode(path))
        if rc != 0:
            raise RuntimeError("pion_host_sim_write_snapshot rc=%d: %s" % (rc, self.last_error()))

    def write_fits(self, path):
        """the FITS file of this sim's on-grid cells, derived images included (pion_host_sim_write_fits);
        pion_amd.fits.read loads it, restart() continues a run from it"""
        rc = self.lib.pion_host_sim_write_fits(self.s, os.fsencode(path))
        if rc != 0:
            raise RuntimeError("pion_host_sim_write_fits rc=%d: %s" % (rc, self.last_error()))

    def write_projection(self, path, axis, fields):
        """the FITS file of the projected images of P along `axis` (pion_host_sim_write_projection): 0, 1, 2 on a 3-D
        Cartesian grid, abi.PROJ_AXIS_PERP on a cylindrical (z,R) one; fields as abi.proj_fields takes them, (name, a,
        var, coef, b) for coef rho^a T^b w.  pion_amd.fits.read returns the images by name."""
        rc = self.lib.pion_host_sim_write_projection(self.s, os.fsencode(path), int(axis), len(fields),
                                                     abi.proj_fields(fields))
        if rc != 0:
            raise RuntimeError("pion_host_sim_write_projection rc=%d: %s" % (rc, self.last_error()))

    def set_projection_output(self, axis, fields):
        """from now on every regular output of time_int is accompanied by <base>_proj_<rank>.<step>.fits with these
        images (pion_host_sim_set_projection_output); no fields turns it off"""
        rc = self.lib.pion_host_sim_set_projection_output(self.s, int(axis), len(fields), abi.proj_fields(fields))
        if rc != 0:
            raise ValueError("pion_host_sim_set_projection_output rc=%d: %s" % (rc, self.last_error()))

    def write_projection_angle(self, path, angle_deg, fields, trip_limit=None):
        """the FITS file of the images of a cylindrical (z,R) grid seen at angle_deg (0 < angle_deg < 90) to its axis
        (pion_host_sim_write_projection_angle): [NR][NZ + 2 n_extra] per field, pion_proj_angle, pion_proj_n_extra,
        pion_proj_pixdx and pion_proj_pixz0 in the header.  trip_limit: the host loop with that trip limit of the ray
        loops (pion_host_sim_write_projection_angle_trips; tests of the refusal)"""
        arr = abi.proj_fields(fields)
        if trip_limit is None:
            rc = self.lib.pion_host_sim_write_projection_angle(self.s, os.fsencode(path), float(angle_deg), len(fields), arr)
        else:
            rc = self.lib.pion_host_sim_write_projection_angle_trips(self.s, os.fsencode(path), float(angle_deg), len(fields),
                                                                     arr, int(trip_limit))
        if rc != 0:
            raise RuntimeError("pion_host_sim_write_projection_angle rc=%d: %s" % (rc, self.last_error()))

    def set_projection_angle_output(self, angle_deg, fields):
        """from now on every regular output of time_int is accompanied by <base>_proja_<rank>.<step>.fits with these
        images (pion_host_sim_set_projection_angle_output); no fields turns it off"""
        rc = self.lib.pion_host_sim_set_projection_angle_output(self.s, float(angle_deg), len(fields), abi.proj_fields(fields))
        if rc != 0:
            raise ValueError("pion_host_sim_set_projection_angle_output rc=%d: %s" % (rc, self.last_error()))

    def add_rt_source(self, src):
        """pion_host_sim_add_rt_source: a radiation source (an abi.RtSource, or what abi.rt_source takes) for the
        ray-traced column densities; returns (id, position used) -- a finite source is moved to a cell vertex"""
        i, pos = C.c_int(-1), (C.c_double * 3)()
        rc = self.lib.pion_host_sim_add_rt_source(self.s, C.byref(abi.rt_source(src)), C.byref(i), pos)
        if rc != 0:
            raise ValueError("pion_host_sim_add_rt_source rc=%d: %s" % (rc, self.last_error()))
        return i.value, tuple(pos)

    def write_columns(self, path):
        """the FITS file of the ray-traced columns of P, per source Col_Src_<id>_T0 and DCol_Src_<id>_T0
        (pion_host_sim_write_columns); pion_amd.fits.read returns the images by name"""
        rc = self.lib.pion_host_sim_write_columns(self.s, os.fsencode(path))
        if rc != 0:
            raise RuntimeError("pion_host_sim_write_columns rc=%d: %s" % (rc, self.last_error()))

    def set_column_output(self, on=True):
        """from now on every regular output of time_int is accompanied by <base>_cols_<rank>.<step>.fits
        (pion_host_sim_set_column_output); on = False turns it off"""
        rc = self.lib.pion_host_sim_set_column_output(self.s, 1 if on else 0)
        if rc != 0:
            raise ValueError("pion_host_sim_set_column_output rc=%d: %s" % (rc, self.last_error()))

    def set_output_filetype(self, filetype):
        """FILE_PIONRAW (the default) or FILE_FITS for the regular outputs of time_int; checkpoints stay PIONRAW2
        (pion_host_sim_set_output_filetype)"""
        rc = self.lib.pion_host_sim_set_output_filetype(self.s, int(filetype))
        if rc != 0:
            raise ValueError("pion_host_sim_set_output_filetype rc=%d: %s" % (rc, self.last_error()))

    def restart(self, paths):
        """restart from the file(s) that hold this sim's planes (one path or a list): PIONRAW2 files
        (pion_host_sim_read_snapshot) or FITS files (pion_host_sim_read_fits), told apart by the first bytes of the
        first file, not by its name; a list that mixes the two is an error.  Returns the note a FITS restart may leave
        (an image a file lacked, set to zero), else an empty string."""
        if isinstance(paths, (str, bytes, os.PathLike)):
            paths = [paths]
        if not paths:
            raise RuntimeError("restart: no files")
        kinds = [(p, k) for p, k in ((p, is_fits(p)) for p in paths) if k is not None]
        fits = bool(kinds) and kinds[0][1]
        for p, k in kinds[1:]:
            if k != fits:
                raise RuntimeError("restart: %s and %s are files of two types (FITS and PIONRAW2)"
                                   % (os.fsdecode(kinds[0][0]), os.fsdecode(p)))
        arr = (C.c_char_p * len(paths))(*[os.fsencode(p) for p in paths])
        entry = "pion_host_sim_read_fits" if fits else "pion_host_sim_read_snapshot"
        rc = getattr(self.lib, entry)(self.s, arr, len(paths))
        if rc != 0:
            raise RuntimeError("%s rc=%d: %s" % (entry, rc, self.last_error()))
        return self.last_error() if fits else ""

    def get_time(self):
        """dict simtime, last_dt, next_optime, finishtime, starttime, timestep of the loop"""
        out = np.zeros(6)
        self.lib.pion_host_sim_get_time(self.s, out.ctypes.data_as(_dp))
        d = dict(zip(["simtime", "last_dt", "next_optime", "finishtime", "starttime"], out[:5].tolist()))
        d["timestep"] = int(out[5])
        return d

    def download(self, which=0):
        out = np.empty(int(np.prod(self.shape)))
        rc = self.lib.pion_host_sim_download(self.s, which, out.ctypes.data_as(_dp))
        if rc != 0:
            raise RuntimeError("pion_host_sim_download rc=%d" % rc)
        return out.reshape(self.shape)

    def close(self):
        # the communicator detaches its stream from the handle: destroy it first
        if self.comm:
            self.lib.pion_host_comm_destroy(self.comm)
            self.comm = C.c_void_p()
        if self.s:
            self.lib.pion_host_sim_destroy(self.s)
            self.s = C.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()
