"""Numpy restatement of the projected images (pion_gpu_project, pion_host_sim_write_projection), written from the issue's
rules and the reference's source, sharing nothing with pion_amd/csrc/dev_project.h.  Every numpy operation below is one
IEEE-754 operation per element (no np.sum, which adds pairwise; no np.dot; nothing fused), so a loop over the summed
axis here performs the additions of one pixel in the order the loop has.

The field (the issue's integrand): coef * rho^a * T^b * w, left to right, powers of rho by multiplication,
  T = p * Mu_tot_over_kB / rho        mp_only_cooling.cpp:274-280 (Mu_tot = 0.609 m_p: :81-95, constants.h:53,64)
  T^b = exp(b * log(T)), skipped for b == 0;  w = P[var], skipped for var < 0.

3-D Cartesian: pixel = (sum over the on-grid cells of the column) * dx; along y and z in increasing index; along x 64
partial sums (lane l: cells l, l + 64, ... in increasing index, from 0.0), then the tree p[l] += p[l + h] for l < h,
h = 32, 16, .. 1.  Image axes: the two remaining axes in grid order, [j][i] with i on the lower-numbered one.

Cylindrical (z,R), analysis/projection/perp_projection.cpp:
  pixels        one ray per row, b = raw_data[DATA_R][ipix] = the cell-centre radius (:178, :230);
                img[npix[Zcyl] * ipix + iz] (:236): the image is [NR][NZ]
  r             the cell centre, cell_interface.cpp:506-512: xmin + (2 i + 1) * (dx / 2)
  slopes        s[i] = (v[i+1] - v[i]) / (r[i+1] - r[i]) for i < Nr-1 (:345-347), s[Nr-1] = s[Nr-2] (:368-370)
  the column    calc_projection_column, :404-487, line by line in abel_column below; dr = delr = the cell diameter
                (:115, :239)
"""
import numpy as np

from pion_amd import abi
from fits_restate import MU_TOT_OVER_KB

EPS = 2.0 ** -52
LANES = 64


CYL_BCS = ["outflow", "outflow", "axisymmetric", "outflow"]
COOL = dict(cooling=8, min_temp=5.0e3, max_temp=1.0e8)


def case(name, strict=1):
    """the configurations of tests/test_host_projection.py and tests/test_gpu_projection.py"""
    kw = dict(strict_fp=strict, dx=0.125)
    cyl = lambda ng, **k: abi.make_config(2, ng, abi.EQEUL, abi.FLUX_RSroe, ntracer=1, coord_sys=2,
                                          **dict(dict(kw, bcs=CYL_BCS), **k))
    if name == "euler_tr_70x9x6":
        return abi.make_config(3, [70, 9, 6], abi.EQEUL, abi.FLUX_RSroe, ntracer=1, **kw)
    if name == "glm_tr_66x5x4":
        return abi.make_config(3, [66, 5, 4], abi.EQGLM, abi.FLUX_RS_HLLD, ntracer=1, **kw)
    if name == "euler_tr_cool_70x9x6":
        return abi.make_config(3, [70, 9, 6], abi.EQEUL, abi.FLUX_RSroe, ntracer=1, **COOL, **kw)
    if name == "cyl_70x37":
        return cyl([70, 37])
    if name == "cyl_70x37_off_axis":      # a grid that does not start at the axis
        return cyl([70, 37], xmin=(0.0, 3 * 0.125), bcs=["outflow"] * 4)
    if name == "cyl_5x2":
        return cyl([5, 2])
    if name == "cyl_70x37_dx0p1":         # a dx that is no power of two: r and the slopes' dr round
        return cyl([70, 37], dx=0.1)
    if name == "cyl_cool_70x37":
        return cyl([70, 37], **COOL)
    raise KeyError(name)


def rough_state(cfg, seed=5):
    """a seeded rough positive state, velocities (and B, psi) of both signs, the tracer positive"""
    from pion_amd import problems
    P = np.random.default_rng(seed).uniform(0.5, 1.5, size=problems.alloc(cfg).shape)
    P[2:cfg.nvar - cfg.ntracer] -= 1.0
    return P


def fields_of(cfg):
    """rho, rho^2, rho TR0, p: (name, a, var, coef, b)"""
    tr0 = cfg.nvar - cfg.ntracer
    return [("coldens", 1, -1, 1.0, 0.0), ("emmeasure", 2, -1, 0.75, 0.0), ("windcol", 1, tr0, 1.0, 0.0),
            ("pressure", 0, abi.PG, 1.0, 0.0)]


HALPHA = ("halpha", 2, -1, 2.0e-3, -0.9)   # a power-law emissivity: rho^2 T^-0.9


def ongrid(cfg, X):
    """on-grid cells of one variable [nz_all][ny_all][nx_all] -> [nz][ny][nx] (unit axes where the grid has none)"""
    nb = cfg.nbc
    sl = [slice(nb, nb + cfg.ng[a]) if a < cfg.ndim else slice(None) for a in (2, 1, 0)]
    return X[tuple(sl)]


def field_value(cfg, A, f):
    """(v, rel): the field at every on-grid cell, and per cell the bound on the relative difference of v between two
    evaluations whose log and exp are each within 1 ulp of the true value (0 where b == 0: the same bits).
    With y = b log T:  |d log T| <= 2 eps |log T|;  the product rounds once more on either side: |dy| <= 3 eps |y|;
    exp(y) changes by dy relatively, the two exps differ by 2 eps, the last product by eps:  rel = eps (3 |y| + 3)."""
    name, a, var, coef, b = f
    rho = ongrid(cfg, A[abi.RO])
    v = np.full(rho.shape, float(coef))
    if a >= 1:
        v = v * rho
    if a == 2:
        v = v * rho
    rel = np.zeros(rho.shape)
    if b != 0.0:
        T = ongrid(cfg, A[abi.PG]) * MU_TOT_OVER_KB / rho
        y = b * np.log(T)
        v = v * np.exp(y)
        rel = EPS * (3.0 * np.abs(y) + 3.0)
    if var >= 0:
        v = v * ongrid(cfg, A[var])
    return v, rel


def column_sum(cfg, A, f, axis):
    """(image [NJ][NI], bound [NJ][NI]) of a 3-D Cartesian grid; bound: |difference| allowed between two evaluations
    of this sum whose fields differ by `rel` per cell (0 for b == 0):  dx (sum |v| rel + (n + 1) eps sum |v|), the
    second term for n additions and a product that round differently once their inputs differ."""
    v, rel = field_value(cfg, A, f)        # [nz][ny][nx]
    ax = 2 - axis                          # array axis of the line of sight
    n = v.shape[ax]
    take = lambda X, k: np.take(X, k, axis=ax)
    if axis != 0:
        s = np.zeros(take(v, 0).shape)
        for k in range(n):                 # increasing index
            s = s + take(v, k)
    else:
        p = []
        for l in range(LANES):
            pl = np.zeros(take(v, 0).shape)
            for ix in range(l, n, LANES):
                pl = pl + take(v, ix)
            p.append(pl)
        h = LANES // 2
        while h >= 1:
            for l in range(h):
                p[l] = p[l] + p[l + h]
            h //= 2
        s = p[0]
    img = s * cfg.dx
    mag, dev = np.zeros(img.shape), np.zeros(img.shape)
    for k in range(n):
        mag = mag + np.abs(take(v, k))
        dev = dev + np.abs(take(v, k)) * take(rel, k)
    bound = np.where(dev > 0.0, cfg.dx * (dev + (n + 1) * EPS * mag), 0.0)
    return img, bound   # [nz][ny] (x), [nz][nx] (y), [ny][nx] (z): i on the lower-numbered axis


def abel_column(r, v, s, Nr, b, dr):
    """calc_projection_column (perp_projection.cpp:404-487) for all z at once: v, s are [Nr][NZ].  Returns (result,
    gate): gate = 2 * sum over the segments of (|s| x2dx + |offset| |xdx|), the issue's measure of the sum."""
    grid_max = r[Nr - 1] + 0.5 * dr                     # :416
    if b > grid_max:                                    # :417-420
        return np.zeros(v.shape[1]), np.zeros(v.shape[1])
    if b < r[0]:                                        # :426-429
        b = r[0] * 1.00000001
    ir = 0
    while (r[ir] + dr) < b:                             # :434-435
        ir += 1
    result = np.zeros(v.shape[1])
    gate = np.zeros(v.shape[1])
    while True:                                         # do { :442
        Rmin = max(b, r[ir])                            # :446
        Rmax = min(grid_max, r[ir] + dr)                # :447
        Rmax2 = Rmax * Rmax
        Rmin2 = Rmin * Rmin
        maxd = np.sqrt(Rmax2 - b * b)                   # :450
        mind = np.sqrt(Rmin2 - b * b)                   # :451
        slope = s[ir]                                   # :456
        offset = v[ir] - s[ir] * Rmin                   # :457
        xdx = maxd - mind                               # :464
        x2dx = 0.5 * (Rmax * maxd - Rmin * mind + b * b * np.log((Rmax + maxd) / (Rmin + mind)))   # :465
        seg = slope * x2dx + offset * xdx               # :471
        result = result + seg                           # :477
        gate = gate + (np.abs(slope) * x2dx + np.abs(offset) * np.abs(xdx))
        ir += 1
        if not ir < Nr:                                 # } while (ir < Nr) :479
            break
    return result * 2.0, gate * 2.0                     # :484


def abel_image(cfg, A, f):
    """(image [NR][NZ], gate [NR][NZ], field bound [NR][NZ]) of a cylindrical (z,R) grid.  gate: the issue's
    4 eps * 2 sum (|s| x2dx + |offset| |xdx|).  field bound (0 for b == 0): what the per-cell `rel` of the field adds --
    dv = |v| rel, ds[i] = (dv[i+1] + dv[i]) / dr, per segment ds x2dx + (dv + ds Rmin) |xdx|, times 2."""
    v, rel = field_value(cfg, A, f)
    v, rel = v[0], rel[0]                               # [NR][NZ]
    Nr, dx = cfg.ng[1], cfg.dx
    r = [cfg.xmin[1] + (2 * i + 1) * (0.5 * dx) for i in range(Nr)]
    s = np.zeros(v.shape)
    for i in range(Nr - 1):
        dr = r[i + 1] - r[i]                            # :346
        s[i] = (v[i + 1] - v[i]) / dr                   # :347
    s[Nr - 1] = s[Nr - 2]                               # :370
    dv = np.abs(v) * rel
    ds = np.zeros(v.shape)
    for i in range(Nr - 1):
        ds[i] = (dv[i + 1] + dv[i]) / (r[i + 1] - r[i])
    ds[Nr - 1] = ds[Nr - 2]
    img, gate, fb = np.zeros(v.shape), np.zeros(v.shape), np.zeros(v.shape)
    for j in range(Nr):
        img[j], g = abel_column(r, v, s, Nr, r[j], dx)  # :230-239
        gate[j] = 4.0 * EPS * g
        if f[4] != 0.0:
            for ir, Rmin, xdx, x2dx in abel_segments(r, Nr, r[j], dx):
                fb[j] = fb[j] + (ds[ir] * x2dx + (dv[ir] + ds[ir] * Rmin) * abs(xdx))
            fb[j] = fb[j] * 2.0
    return img, gate, fb


def abel_segments(r, Nr, b, dr):
    """[(ir, Rmin, xdx, x2dx)] of the ray with impact parameter b: abel_column's geometry, for the bounds only"""
    grid_max = r[Nr - 1] + 0.5 * dr
    if b < r[0]:
        b = r[0] * 1.00000001
    ir = 0
    while (r[ir] + dr) < b:
        ir += 1
    out = []
    for ir in range(ir, Nr):
        Rmin, Rmax = max(b, r[ir]), min(grid_max, r[ir] + dr)
        maxd, mind = np.sqrt(Rmax * Rmax - b * b), np.sqrt(Rmin * Rmin - b * b)
        out.append((ir, Rmin, maxd - mind,
                    0.5 * (Rmax * maxd - Rmin * mind + b * b * np.log((Rmax + maxd) / (Rmin + mind)))))
    return out


def project(cfg, A, fields, axis):
    """[(name, image, allowed difference between two routes)]: the allowance is 0 where the routes must give the same
    bits (3-D, b == 0)"""
    out = []
    for f in fields:
        if cfg.coord_sys == 2:
            img, gate, fb = abel_image(cfg, A, f)
            out.append((f[0], img, gate + fb))
        else:
            img, bound = column_sum(cfg, A, f, axis)
            out.append((f[0], img, bound))
    return out
