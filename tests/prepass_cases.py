"""Rough fields for the stage prepass (pion_amd/csrc/kernels_prepass.hip): the HLLD -> HLL switch and the H-correction eta.

Shared by test_prepass_cases.py (oracle only) and test_gpu_prepass.py.  Plain numpy, seeded.  A field is made of
  * a ROUGH region: p = exp(U(-a, a)), a = 1.2, per cell, so that the sum over the axes of |dp| / min p falls on both sides
    of 5 and a single axis' jump on both sides of the kernels' division-free pre-test 1.6; rho in [0.5, 2]; velocities
    U(-1, 1) 0.3 c_s (div v of either sign); a weak random B (plasma beta about 10); tracers in [0, 1];
  * a CALM region (1 % perturbations), where the screened prepass must find quiet blocks;
  * a STEEP region AT REST: the rough pressures with v = 0 exactly, so that div v == 0 exactly: steep and not flagged;
  * single-cell pressure SPIKES (x 50) inside the rough region with a converging or (every other one) a diverging
    velocity field around them, planted where the kernels change their code shape: the first and the last on-grid cell
    of every axis (the ghost copies become steep), the march kernel's x seams (all-cell x = 61, 62, 123, 124), the
    all-cell planes 15, 16 (its 16-plane chunks) and the last plane, the corners of the screen's blocks.
"""
import numpy as np

from pion_amd import abi, driver, problems

A_ROUGH = 1.2
SPIKE = 50.0
GAMMA = 5.0 / 3.0
ROUGH, CALM, REST = 0, 1, 2


def default_layout(ix, iy, iz, ng):
    """regions by the on-grid x index: rough | calm | steep at rest | rough (the x seams of the march kernel: rough)"""
    nx = ng[0]
    r = np.full(np.broadcast(ix, iy, iz).shape, ROUGH)
    r[np.broadcast_to((ix >= int(0.15 * nx)) & (ix < int(0.30 * nx)), r.shape)] = CALM
    r[np.broadcast_to((ix >= int(0.30 * nx)) & (ix < int(0.42 * nx)), r.shape)] = REST
    return r


def screen_join_layout(ix, iy, iz, ng):
    """calm: x >= 62 and z >= 8 (on-grid), which is the 3 x 3 x 3 neighbourhood of the screen's blocks (2, *, 2) of a
    130 x 9 x 20 grid without a periodic axis: those blocks stay quiet.  Steep at rest: a slab of the low-z part."""
    r = np.full(np.broadcast(ix, iy, iz).shape, ROUGH)
    r[np.broadcast_to((ix >= 62) & (iz >= 8), r.shape)] = CALM
    r[np.broadcast_to((ix >= 70) & (ix < 90) & (iz < 8), r.shape)] = REST
    return r


def build(ng, eq, geometry="cart", bcs=None, seed=0, **kw):
    """(cfg, P) of a rough field on ng on-grid cells; geometry "cart", "cyl" (z, R) or "sph" (1-D)"""
    return build_info(ng, eq, geometry, bcs, seed, **kw)[:2]


def build_info(ng, eq, geometry="cart", bcs=None, seed=0, solver=None, artvisc=abi.AV_FKJ98_1D, ntracer=0, strict_fp=1,
               layout=default_layout):
    """build() and a dict: region (per cell, -1 in ghosts), spikes (all-cell (x, y, z) of the planted ones)"""
    ndim = len(ng)
    if solver is None:
        solver = abi.FLUX_RS_HLLD if eq != abi.EQEUL else abi.FLUX_RSroe
    cfg = abi.make_config(ndim, list(ng), eq, solver, ntracer=ntracer, artvisc=artvisc, etav=0.1, gamma=GAMMA, cfl=0.3,
                          dx=1.0 / ng[0], xmin=(0.0, 0.0, 0.0), bcs=bcs or ["periodic"] * (2 * ndim), strict_fp=strict_fp,
                          coord_sys={"cart": 1, "cyl": 2, "sph": 3}[geometry])
    rng = np.random.default_rng(seed)
    P = problems.alloc(cfg)
    nga = abi.ng_all(cfg)
    shape = P.shape[1:]
    nb = [cfg.nbc if a < ndim else 0 for a in range(3)]
    n3 = [cfg.ng[a] for a in range(3)]
    iz, iy, ix = np.meshgrid(*[np.arange(nga[a]) - nb[a] for a in (2, 1, 0)], indexing="ij")   # on-grid indices
    on = np.ones(shape, dtype=bool)
    for a, i in ((0, ix), (1, iy), (2, iz)):
        on &= (i >= 0) & (i < n3[a])
    reg = np.where(on, layout(ix, iy, iz, n3), -1)
    calm = reg == CALM
    nvb = {abi.EQEUL: 5, abi.EQMHD: 8, abi.EQGLM: 9}[eq]

    # (ghost cells get the rough values too; the boundary update overwrites them)
    P[abi.PG] = np.where(calm, 1.0 + 0.01 * rng.uniform(-1, 1, shape), np.exp(rng.uniform(-A_ROUGH, A_ROUGH, shape)))
    P[abi.RO] = np.where(calm, 1.0 + 0.01 * rng.uniform(-1, 1, shape), rng.uniform(0.5, 2.0, shape))
    cs = np.sqrt(GAMMA * P[abi.PG] / P[abi.RO])
    for v in (abi.VX, abi.VY, abi.VZ):
        P[v] = np.where(calm, 0.01, 1.0) * rng.uniform(-1, 1, shape) * 0.3 * cs
    P[abi.VX:abi.VZ + 1, reg == REST] = 0.0
    if nvb >= 8:
        for v in (abi.BX, abi.BY, abi.BZ):
            P[v] = np.where(calm, 0.2 + 0.002 * rng.uniform(-1, 1, shape), 0.3 * rng.uniform(-1, 1, shape))
    if nvb == 9:
        P[abi.SI] = 0.01 * rng.uniform(-1, 1, shape) * np.where(calm, 0.01, 1.0)
    for t in range(ntracer):
        P[nvb + t] = rng.uniform(0, 1, shape)
    if geometry == "sph":
        P[abi.VY] = 0.0
        P[abi.VZ] = 0.0

    # one spike at rest, in the middle of the region at rest: its neighbours are steep whatever the seed, and div v == 0
    rz, ry, rx = np.nonzero(reg == REST)
    if rx.size:
        mid = np.nonzero((rx == (rx.min() + rx.max()) // 2) & (ry == (ry.min() + ry.max()) // 2)
                         & (rz == (rz.min() + rz.max()) // 2))[0][0]
        P[abi.PG][rz[mid], ry[mid], rx[mid]] *= SPIKE
    spikes = _plant_spikes(cfg, P, reg, rng)
    return cfg, P, {"region": reg, "spikes": spikes}


def _plant_spikes(cfg, P, reg, rng):
    """x 50 the pressure of single rough cells whose +-2 neighbourhood is rough, a linear velocity field around each
    (another slope on every axis: no cancellation to rounding at a reflecting face):
    converging for even-numbered spikes, diverging for odd-numbered ones.  Returns the all-cell (x, y, z) of each."""
    ndim = cfg.ndim
    nga = abi.ng_all(cfg)
    nb = cfg.nbc
    lo = [nb if a < ndim else 0 for a in range(3)]
    hi = [lo[a] + cfg.ng[a] - 1 for a in range(3)]     # first / last on-grid all-cell index
    rough = reg == ROUGH
    # {axis: all-cell index} constraints, the most constrained first
    wanted = []
    if ndim == 3:
        # corners of the screen's blocks: on-grid x 61 | 62, y multiples of 4, z multiples of 8
        for x, y, z in ((61, 3, 7), (62, 4, 8), (61, 4, 7), (62, 3, 8), (61, 3, 8), (62, 4, 7)):
            if x <= cfg.ng[0] - 1 and y <= cfg.ng[1] - 1 and z <= cfg.ng[2] - 1:
                wanted.append({0: x + nb, 1: y + nb, 2: z + nb})
    for x in (61, 62, 123, 124):
        if lo[0] <= x <= hi[0]:
            wanted += [{0: x}, {0: x}]
    if ndim == 3:
        for z in (15, 16, hi[2]):
            if lo[2] <= z <= hi[2]:
                wanted += [{2: z}, {2: z}]
    for a in range(ndim):
        wanted += [{a: lo[a]}, {a: hi[a]}, {a: lo[a]}, {a: hi[a]}]
    placed = []
    cs0 = np.sqrt(GAMMA)
    for want in wanted:
        cand = rough.copy()
        for a, i in want.items():
            m = np.zeros(nga[a], dtype=bool)
            m[i] = True
            cand &= m.reshape([-1 if (2 - a) == d else 1 for d in range(3)])
        idx = np.argwhere(cand)                          # (z, y, x)
        rng.shuffle(idx)
        for z, y, x in idx[:200]:
            c = (x, y, z)
            box = tuple(slice(max(c[a] - 2, lo[a]), min(c[a] + 2, hi[a]) + 1) for a in (2, 1, 0))
            if not rough[box].all():
                continue
            if any(max(abs(c[a] - q[a]) for a in range(3)) < 3 for q in placed):   # (two cells between spikes)
                continue
            sgn = -1.0 if len(placed) % 2 == 0 else 1.0  # -1: converging
            P[abi.PG][z, y, x] *= SPIKE
            for a in range(ndim):
                ia = np.arange(box[2 - a].start, box[2 - a].stop) - c[a]
                P[abi.VX + a][box] = (sgn * (0.3, 0.23, 0.17)[a] * cs0 * ia).reshape([-1 if (2 - a) == d else 1 for d in range(3)])
            placed.append(c)
            break
    return placed


# ---------------------------------------------------------------------------------------------------------------------
# The case table.  f: dt = f * calculate_timestep(), the largest f <= 0.1 for which the oracle's state stays finite
# with rho, p > 0 through both stages (test_prepass_cases.py asserts it).
MIX = ["reflecting", "outflow", "outflow", "reflecting", "reflecting", "outflow"]
CASES = {
    # --- the switch (HLLD)
    "march_3d":      dict(ng=(126, 7, 14), eq=abi.EQGLM, seed=11, f=0.1),
    "march_fit_120": dict(ng=(120, 8, 12), eq=abi.EQMHD, bcs=MIX, seed=12, f=0.1),
    "march_fit_121": dict(ng=(121, 8, 12), eq=abi.EQMHD, bcs=MIX, seed=13, f=0.1),
    "screen_join":   dict(ng=(130, 9, 20), eq=abi.EQGLM, bcs=MIX, seed=14, f=0.1, layout=screen_join_layout),
    "dense_3d_60":   dict(ng=(60, 6, 8), eq=abi.EQGLM, seed=15, f=0.1),
    "dense_3d_61":   dict(ng=(61, 6, 8), eq=abi.EQGLM, bcs=MIX, seed=16, f=0.1),
    # (No reflecting wall, because its states are compared in the fast build too.  The ghost state of a reflecting wall
    # mirrors v_n and B_n, so the interface has B_n = 0 and S_M = 0 in exact arithmetic, each side's own flux carries its
    # own B_n, and ideal-MHD HLLD returns +B_n v_t or -B_n v_t for the flux of B_t by the sign of S_M -- of its rounding
    # residue.  The strict build reproduces the reference's residue bit for bit (march_fit_*); a contracted
    # multiply-add need not: on this field with reflecting walls the fast rows kernel left 4 of ~1000 wall cells 1e-3
    # away from the oracle and from the fast cell-per-thread kernel.  Cf. tests/test_reference_conditioning.py.)
    "dense_hcorr":   dict(ng=(70, 6, 8), eq=abi.EQMHD, bcs=["outflow", "outflow", "periodic", "periodic", "outflow", "outflow"],
                          artvisc=abi.AV_HCORR_FKJ98, seed=17, f=0.1),
    "cart_2d":       dict(ng=(130, 37), eq=abi.EQGLM, seed=18, f=0.1),
    "cyl_2d":        dict(ng=(70, 24), eq=abi.EQGLM, geometry="cyl",
                          bcs=["outflow", "outflow", "axisymmetric", "outflow"], seed=19, f=0.1),
    "line_1d":       dict(ng=(130,), eq=abi.EQMHD, seed=20, f=0.1),
    "split_3d":      dict(ng=(70, 9, 12), eq=abi.EQGLM, seed=21, f=0.1),
    "split_2d":      dict(ng=(70, 41), eq=abi.EQGLM, seed=22, f=0.1),
    # --- eta alone (no HLLD)
    "roe_hcorr":     dict(ng=(70, 6, 8), eq=abi.EQEUL, bcs=MIX, artvisc=abi.AV_HCORR_FKJ98, seed=23, f=0.1),
    "roe_hcorr_tr":  dict(ng=(70, 6, 8), eq=abi.EQEUL, bcs=MIX, artvisc=abi.AV_HCORR_FKJ98, ntracer=1, seed=24, f=0.1),
    "cyl_hcorr":     dict(ng=(70, 24), eq=abi.EQEUL, geometry="cyl", bcs=["outflow", "outflow", "axisymmetric", "outflow"],
                          artvisc=abi.AV_HCORR_FKJ98, seed=25, f=0.1),
    "sph_hcorr":     dict(ng=(64,), eq=abi.EQEUL, geometry="sph", bcs=["reflecting", "outflow"],
                          artvisc=abi.AV_HCORR_FKJ98, seed=26, f=0.1),
}
SWITCH_CASES = [n for n, c in CASES.items() if c["eq"] != abi.EQEUL]
FAST_STATE_CASES = ["march_3d", "dense_3d_60", "dense_3d_61", "cyl_2d", "dense_hcorr"]   # states compared in the fast build too
ETA_CASES = [n for n, c in CASES.items() if c.get("artvisc", 0) == abi.AV_HCORR_FKJ98]
# the second stage's prepass is the screened one: 3-D GLM without the H-correction.  (Ideal MHD: the first-order instance
# of the 8-variable stage kernel takes 5 rows per wavefront, rows2_rows_3d, which do not divide the screen's block height
# of 4, so the half stage leaves no pressure summary and the march kernel runs both stages of march_fit_*.)
SCREENED_CASES = [n for n in SWITCH_CASES if len(CASES[n]["ng"]) == 3 and CASES[n]["eq"] == abi.EQGLM]


def make(name, strict_fp=1):
    c = dict(CASES[name])
    f = c.pop("f")
    cfg, P, info = build_info(c.pop("ng"), c.pop("eq"), strict_fp=strict_fp, **c)
    info["f"] = f
    return cfg, P, info


# ---------------------------------------------------------------------------------------------------------------------
def two_stages(sim, cfg, P, f, t_dyn=None, record=None, comm=None):
    """OA1 half stage, boundary update, OA2 full stage, boundary update, with dt = f * calculate_timestep() (t_dyn given:
    f * t_dyn instead, so that two backends take the same step).  record(sim, i, S) is called after stage i = 0, 1 with
    the stencil state S that stage's prepass read, and as record(sim, 2, None) at the end.  comm: a slab's halo exchange
    (driver.SimControl), every stage then in two parts.  Returns the backend's own calculate_timestep()."""
    sc = driver.SimControl(sim, cfg, comm=comm)
    sc.init(P)
    own = sc.calculate_timestep()
    if t_dyn is None:
        t_dyn = own
    if cfg.eqntype == abi.EQGLM:
        sim.set_glm_speeds(t_dyn, cfg.dx, 0.25 / cfg.dx)
    dt = f * t_dyn
    for i, (sdt, ooa, full) in enumerate(((0.5 * dt, abi.OA1, 0), (dt, abi.OA2, 1))):
        S = sim.download(i)                     # stage 0 reads P (== Ph), stage 1 reads Ph
        sc._stage(sdt, ooa, full)
        if record:
            record(sim, i, S)
        sc.update_bcs(ooa, abi.OA2)
    sc.finish_halo()
    if record:
        record(sim, 2, None)
    return own


_ORACLE = {}


def oracle_run(name):
    """The oracle's two stages of case `name`, computed once: dict with t_dyn and per stage i: S (stencil state), state
    (what the stage wrote: Ph after the half stage, P after the full one), eta[axis], divv, gradp -- arrays of all
    cells, [nz][ny][nx] (read-only); final: P after the last boundary update."""
    if name in _ORACLE:
        return _ORACLE[name]
    from cpu_backends import CpuSim
    cfg, P, info = make(name)
    nga = abi.ng_all(cfg)
    shp = (nga[2], nga[1], nga[0])
    out = {"cfg": cfg, "P": P, "info": info, "stages": []}

    def record(o, i, S):
        if i == 2:
            out["final"] = o.download(0).copy()
            out["final"].setflags(write=False)
            return
        st = {"S": S, "state": o.download(1 - i).copy()}
        if cfg.artvisc in (abi.AV_HCORRECTION, abi.AV_HCORR_FKJ98):
            st["eta"] = [o.get_aux(a).reshape(shp) for a in range(cfg.ndim)]
        if cfg.solver == abi.FLUX_RS_HLLD:
            st["divv"] = o.get_aux(3).reshape(shp)
            st["gradp"] = o.get_aux(4).reshape(shp)
        for v in st.values():
            for a in (v if isinstance(v, list) else [v]):
                a.setflags(write=False)
        out["stages"].append(st)

    with CpuSim(cfg, "orc") as o:
        out["t_dyn"] = two_stages(o, cfg, P, info["f"], record=record)
    _ORACLE[name] = out
    return out


# ---------------------------------------------------------------------------------------------------------------------
def cell_indices(cfg):
    """all-cell (ix, iy, iz) arrays, [nz][ny][nx]"""
    nga = abi.ng_all(cfg)
    iz, iy, ix = np.meshgrid(np.arange(nga[2]), np.arange(nga[1]), np.arange(nga[0]), indexing="ij")
    return ix, iy, iz


def class_masks(cfg):
    """the cell classes every case must populate with a flagged and with a steep-but-unflagged cell"""
    nga = abi.ng_all(cfg)
    idx = cell_indices(cfg)
    ghost = np.zeros(idx[0].shape, dtype=bool)
    face = np.zeros_like(ghost)
    for a in range(cfg.ndim):
        ghost |= (idx[a] < cfg.nbc) | (idx[a] >= cfg.nbc + cfg.ng[a])
        face |= (idx[a] == 0) | (idx[a] == nga[a] - 1)
    m = {"on-grid": ~ghost, "ghost": ghost, "array face": face}
    if nga[0] > 61:
        m["x seams"] = np.isin(idx[0], [61, 62, 123, 124])
    if cfg.ndim >= 2:
        m["last y tile"] = idx[1] >= 4 * ((nga[1] - 1) // 4)
    if cfg.ndim == 3 and nga[2] > 16:
        m["planes 15/16"] = np.isin(idx[2], [15, 16])
    return m


def near_threshold(cfg, st):
    """cells whose flag a few ulp could turn: |gradp - 5| <= 5e-12, or 0 < |div v| <= 1e-12 sum(|v+| + |v-|) / dx"""
    S = st["S"]
    vsum = np.zeros(S.shape[1:])
    for a in range(cfg.ndim):
        v = np.abs(S[abi.VX + a])
        ax = 2 - a
        hi = np.concatenate([np.take(v, range(1, v.shape[ax]), axis=ax), np.take(v, [-1], axis=ax)], axis=ax)
        lo = np.concatenate([np.take(v, [0], axis=ax), np.take(v, range(0, v.shape[ax] - 1), axis=ax)], axis=ax)
        vsum += hi + lo
    d = np.abs(st["divv"])
    return (np.abs(st["gradp"] - 5.0) <= 5e-12) | ((d > 0) & (d <= 1e-12 * vsum / cfg.dx))


def expected_switch(st):
    return ((st["divv"] < 0.0) & (st["gradp"] > 5.0)).astype(np.uint8)


def screen_blocks(cfg, Pnew):
    """The screen's rule (pion_amd/csrc/hll_screen.h) restated on the pressures `Pnew` a stage wrote: (active[bz][by][bx],
    block of every cell of the array or -1) -- a block is quiet when max - min <= 1.6 min over the on-grid cells of its
    3 x 3 x 3 block neighbourhood (wrapping along periodic axes); a block on a face also owns the ghost cells beyond."""
    B = (62, 4, 8)
    nb = cfg.nbc
    ng = [cfg.ng[a] for a in range(3)]
    nblk = []
    for a in range(3):
        r = ng[a] % B[a]
        nblk.append(max(1, -(-ng[a] // B[a]) if (r == 0 or r >= nb) else ng[a] // B[a]))
    blk_of = [np.minimum(np.arange(ng[a]) // B[a], nblk[a] - 1) for a in range(3)]
    p = Pnew[abi.PG][nb:-nb, nb:-nb, nb:-nb]
    bz, by, bx = np.meshgrid(blk_of[2], blk_of[1], blk_of[0], indexing="ij")
    flat = (bz * nblk[1] + by) * nblk[0] + bx
    nt = nblk[0] * nblk[1] * nblk[2]
    mn = np.full(nt, np.inf)
    mx = np.full(nt, -np.inf)
    np.minimum.at(mn, flat.ravel(), p.ravel())
    np.maximum.at(mx, flat.ravel(), p.ravel())
    mn, mx = mn.reshape(nblk[::-1]), mx.reshape(nblk[::-1])
    per = [cfg.bc_type[2 * a] == abi.BC_PERIODIC for a in range(3)]
    active = np.zeros(nblk[::-1], dtype=bool)
    for z in range(nblk[2]):
        for y in range(nblk[1]):
            for x in range(nblk[0]):
                m, M = np.inf, -np.inf
                for oz in (-1, 0, 1):
                    for oy in (-1, 0, 1):
                        for ox in (-1, 0, 1):
                            q = [x + ox, y + oy, z + oz]
                            ok = True
                            for a in range(3):
                                if q[a] < 0 or q[a] >= nblk[a]:
                                    if per[a]:
                                        q[a] %= nblk[a]
                                    else:
                                        ok = False
                            if ok:
                                m, M = min(m, mn[q[2], q[1], q[0]]), max(M, mx[q[2], q[1], q[0]])
                active[z, y, x] = not (M - m <= 1.6 * m)
    # block of every all-cell index: the ghosts join the first / last block
    ext = [np.concatenate([[0] * nb, blk_of[a], [nblk[a] - 1] * nb]) for a in range(3)]
    ez, ey, ex = np.meshgrid(ext[2], ext[1], ext[0], indexing="ij")
    return active, (ez, ey, ex)


def cfast_plus_vn(cfg, S, axis):
    """|v_n| + c_fast (Euler: + c_s) of every cell along `axis`"""
    a2 = cfg.gamma * S[abi.PG] / S[abi.RO]
    if cfg.eqntype == abi.EQEUL:
        c = np.sqrt(a2)
    else:
        b2 = (S[abi.BX] ** 2 + S[abi.BY] ** 2 + S[abi.BZ] ** 2) / S[abi.RO]
        bn2 = S[abi.BX + axis] ** 2 / S[abi.RO]
        c = np.sqrt(0.5 * (a2 + b2 + np.sqrt(np.maximum((a2 + b2) ** 2 - 4.0 * a2 * bn2, 0.0))))
    return np.abs(S[abi.VX + axis]) + c
