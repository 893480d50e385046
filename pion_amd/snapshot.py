"""Raw snapshot / restart files for the device state.

The reference writes Silo / FITS / text through dataIO/ (dataio_base.cpp:60-440 is the header registry);
none of those libraries is needed to checkpoint the path, so the format here is the minimum that makes a
restart bit-identical: a JSON header (the pion_gpu_config fields + simtime, timestep, last_dt, the
reference's SimParams names where one exists) followed by the fp64 SoA state [nvar][nz_all][ny_all][nx_all]
in the boundary layout of include/pion_gpu.h, ghost cells included.  B is stored in code units (no
sqrt(4 pi) rescaling, cf. dataio_silo.cpp:1468-1492), so a round trip changes no bit.

    write(path, cfg, P, simtime, timestep, last_dt)       read(path) -> (cfg, P, meta)

read() also takes the files of the C++ host loop, format PIONRAW2 (pion_amd/host/snapshot_io.h: a text header of
"name value" lines under the reference's parameter names, then the on-grid cells only): it returns the GLOBAL
configuration, the file's planes embedded in a zero-ghosted array of the boundary layout, and the header as a dict of
strings.
"""
import json
import struct

import numpy as np

from . import abi

MAGIC = b"PIONRAW1"
MAGIC2 = b"PIONRAW2"
_SCALARS = ["ndim", "nvar", "ntracer", "eqntype", "solver", "artvisc", "sp_ooa", "tm_ooa", "coord_sys", "nbc",
            "dx", "gamma", "cfl", "etav", "min_temp", "max_temp", "bc_dmach2", "cooling", "mp_timestep_limit",
            "strict_fp"]
_ARRAYS = ["ng", "xmin", "refvec", "bc_type"]


def _cfg_to_dict(cfg):
    d = {k: getattr(cfg, k) for k in _SCALARS}
    for k in _ARRAYS:
        d[k] = list(getattr(cfg, k))
    return d


def _dict_to_cfg(d):
    cfg = abi.PionGpuConfig()
    for k in _SCALARS:
        setattr(cfg, k, d[k])
    for k in _ARRAYS:
        arr = getattr(cfg, k)
        for i, v in enumerate(d[k]):
            arr[i] = v
    return cfg


def write(path, cfg, P, simtime, timestep, last_dt):
    P = np.ascontiguousarray(P, dtype=np.float64)
    nga = abi.ng_all(cfg)
    assert P.shape == (cfg.nvar, nga[2], nga[1], nga[0]), (P.shape, nga)
    header = {"config": _cfg_to_dict(cfg), "simtime": float(simtime), "timestep": int(timestep),
              "last_dt": float(last_dt), "shape": list(P.shape), "dtype": "<f8",
              "layout": "[nvar][nz_all][ny_all][nx_all], ghosts included, code units"}
    hb = json.dumps(header).encode()
    with open(path, "wb") as f:
        f.write(MAGIC)
        f.write(struct.pack("<q", len(hb)))
        f.write(hb)
        f.write(P.astype("<f8", copy=False).tobytes())


def _read2(f, path):
    """PIONRAW2 (written by pion_host_sim_write_snapshot)"""
    hd = {}
    while "pion_data_offset" not in hd:
        line = f.readline()
        if not line:
            raise ValueError("%s: PIONRAW2 header incomplete" % path)
        line = line.decode().rstrip("\n")
        if line:
            k, _, v = line.partition(" ")
            hd[k] = v
    ints = lambda k: [int(x) for x in hd[k].split()]
    flts = lambda k: [float(x) for x in hd[k].split()]
    cfg = abi.PionGpuConfig()
    for field, key in [("ndim", "gridndim"), ("nvar", "eqn_nvar"), ("ntracer", "num_tracer"), ("eqntype", "eqn_type"),
                       ("solver", "solver"), ("artvisc", "art_visc"), ("sp_ooa", "Space_OOA"), ("tm_ooa", "Time_OOA"),
                       ("coord_sys", "coord_sys"), ("nbc", "pion_nbc"), ("bc_dmach2", "pion_bc_dmach2"),
                       ("cooling", "EP_cooling"), ("mp_timestep_limit", "EP_MP_timestep_limit"),
                       ("strict_fp", "pion_strict_fp")]:
        setattr(cfg, field, int(hd[key]))
    for field, key in [("dx", "pion_dx"), ("gamma", "Gamma"), ("cfl", "CFL"), ("etav", "eta_visc"),
                       ("min_temp", "EP_Min_Temperature"), ("max_temp", "EP_Max_Temperature")]:
        setattr(cfg, field, float(hd[key]))
    for a in range(3):
        cfg.ng[a] = ints("NGrid")[a]
        cfg.xmin[a] = flts("Xmin")[a]
    for v, x in enumerate(flts("Ref_Vector")):
        cfg.refvec[v] = x
    names = dict(abi.BC_NAMES, NONE=0)
    for i, k in enumerate(["BC_XN", "BC_XP", "BC_YN", "BC_YP", "BC_ZN", "BC_ZP"]):
        cfg.bc_type[i] = names[hd[k]]
    # this file's planes of the slab axis (the last axis; 1-D: the one row), zero ghosts around them
    n, nb = int(hd["pion_slab_n"]), cfg.nbc
    ng = [cfg.ng[0], cfg.ng[1], cfg.ng[2]]
    if cfg.ndim > 1:
        ng[cfg.ndim - 1] = n
    f.seek(int(hd["pion_data_offset"]))
    count = cfg.nvar * ng[0] * ng[1] * ng[2]
    data = np.frombuffer(f.read(8 * count), dtype="<f8")
    if data.size != count:
        raise ValueError("%s: PIONRAW2 data truncated" % path)
    g = [nb if a < cfg.ndim else 0 for a in range(3)]
    P = np.zeros((cfg.nvar, ng[2] + 2 * g[2], ng[1] + 2 * g[1], ng[0] + 2 * g[0]))
    P[:, g[2]:g[2] + ng[2], g[1]:g[1] + ng[1], g[0]:g[0] + ng[0]] = data.reshape(cfg.nvar, ng[2], ng[1], ng[0])
    return cfg, P, hd


def read(path):
    with open(path, "rb") as f:
        magic = f.read(8)
        if magic == MAGIC2:
            return _read2(f, path)
        if magic != MAGIC:
            raise ValueError("%s is not a PIONRAW1 snapshot" % path)
        (n,) = struct.unpack("<q", f.read(8))
        header = json.loads(f.read(n).decode())
        P = np.frombuffer(f.read(), dtype="<f8").reshape(header["shape"]).copy()
    return _dict_to_cfg(header["config"]), P, header
