"""Scalar Python restatement of the inclined projection of a cylindrical (z,R) grid (pion_gpu_project_angle,
pion_host_sim_write_projection_angle): the reference's analysis/projection/angle_projection.cpp in its own order, with
explicit loops, one IEEE-754 double operation per Python operation.  It shares nothing with
pion_amd/csrc/dev_project_angle.h.  Line numbers are angle_projection.cpp's unless another file is named.

The two stated departures of the project's rule are restated too (they are what makes every walk end):
  1. the cell `c` of an on-grid pixel is (i - n_extra, j) instead of the two equalD searches of :484-488;
  2. a cell outside [0, NZ) x [0, NR) is missing (None); a ray whose next cell is missing ends there, and an on-grid
     pixel whose incoming ray ended that way has no turning cell and no outgoing ray; each ray loop makes at most
     trip_limit trips (default 2 (NZ + NR) + 8), and a pixel whose loop gets there first is capped.

tan(angle) and 1 / sin(angle) come from math (the libm the host library uses here); a caller on a platform where the
two differ by an ulp passes the library's numbers in (tn, invst)."""
import math

TINYVALUE = 1.0e-100      # constants.h:152
SMALLVALUE = 1.0e-12      # constants.h:150
ONE_PLUS_EPS = 1.0 + SMALLVALUE    # constants.h:156
ONE_MINUS_EPS = 1.0 - SMALLVALUE   # constants.h:157
EPS = 2.0 ** -52


def equalD(a, b):
    """constants.cpp:48-69"""
    if a == b:                                                   # :53
        return True
    if abs(a) + abs(b) < TINYVALUE:                              # :56
        return True
    if (abs(a - b) / (abs(a) + abs(b) + TINYVALUE)) < SMALLVALUE:   # :63
        return True
    return False


def angle_numbers(angle_deg):
    """(angle, tan, 1 / sin): project2D.cpp:148, angle_projection.cpp:445"""
    angle = angle_deg * math.pi / 180.0
    return angle, math.tan(angle), 1.0 / math.sin(angle)


class Grid:
    """what the reference reads from SimPM and the grid: Xmin, Xmax = Xmin + NG dx, dx; cell centres as the library's
    cell_interface spells them (xmin + (2 k + 1) (dx / 2))"""

    def __init__(self, NZ, NR, zmin, rmin, dx):
        self.NZ, self.NR, self.dx = NZ, NR, dx
        self.zmin, self.rmin = zmin, rmin
        self.zmax = zmin + NZ * dx
        self.rmax = rmin + NR * dx

    def cz(self, iz):
        return self.zmin + (2 * iz + 1) * (0.5 * self.dx)

    def cr(self, ir):
        return self.rmin + (2 * ir + 1) * (0.5 * self.dx)

    def on(self, c):
        return c is not None and 0 <= c[0] < self.NZ and 0 <= c[1] < self.NR

    def next(self, c, dz, dr):
        """NextPt, a missing cell staying missing; the caller decides what an off-grid cell means"""
        return None if c is None else (c[0] + dz, c[1] + dr)


def n_extra_of(G, tn):
    return int(abs(G.rmax / tn / G.dx))                          # project2D.cpp:319


def pixel_centre(G, n_extra, i, j):
    """:41-54"""
    zmin = G.zmin - n_extra * G.dx                               # :50
    return (zmin + (i + 0.5) * G.dx, G.rmin + (j + 0.5) * G.dx)  # :51-52


def get_Z_from_R(pos, R, tn, inout):
    return pos[0] + inout * math.sqrt(R * R - pos[1] * pos[1]) / tn    # :76


def get_R_from_Z(pos, Z, tn):
    return math.sqrt(pos[1] * pos[1] + (Z - pos[0]) * (Z - pos[0]) * tn * tn)   # :98-99


def get_start_of_ray(G, pos, tn):
    """:115-171, angle < pi/2: inout = 1"""
    r_ini = G.rmax                                               # :128
    z_ini = get_Z_from_R(pos, r_ini, tn, 1)                      # :129
    if z_ini > G.zmax:                                           # :132
        z_ini = G.zmax
        r_ini = get_R_from_Z(pos, z_ini, tn)
    elif z_ini < G.zmin:                                         # :139
        z_ini = G.zmin
        r_ini = get_R_from_Z(pos, z_ini, tn)
    iz, ir = 0, 0                                                # :151 FirstPt
    while (G.cr(ir) + 0.5 * G.dx) < r_ini and ir + 1 < G.NR:     # :152-155
        ir += 1
    while (G.cz(iz) + 0.5 * G.dx) < z_ini and iz + 1 < G.NZ:     # :156-159
        iz += 1
    return (iz, ir)


def get_entry_exit_points(G, pos, tn, inout, ray):
    """:184-336, the angle < pi/2 branches.  Returns (entry, exit, next): two [z, R] lists and a cell or None"""
    cpos = (G.cz(ray[0]), G.cr(ray[1]))                          # :195-196
    dxo2 = 0.5 * G.dx                                            # :197
    dx = G.dx                                                    # :198
    flag = False
    dir_flag = inout
    entry = [cpos[0] + dxo2, 0.0]                                # :209
    exit_ = [cpos[0] - dxo2, 0.0]                                # :210
    entry[1] = get_R_from_Z(pos, entry[0], tn)                   # :218
    exit_[1] = get_R_from_Z(pos, exit_[0], tn)                   # :219
    if equalD(exit_[1], entry[1]) and equalD(pos[0], cpos[0]):   # :221
        if not equalD(pos[1], cpos[1]):                          # :224
            flag = True
    midpt = get_R_from_Z(pos, cpos[0], tn)                       # :232
    mn = (cpos[1] - dxo2) * ONE_MINUS_EPS                        # :236
    mx = (cpos[1] + dxo2) * ONE_PLUS_EPS                         # :237
    if (entry[1] < mn and exit_[1] < mn and midpt < mn) or (entry[1] > mx and exit_[1] > mx and midpt > mx):   # :242
        return [1.0e99, 1.0e99], [1.0e99, 1.0e99], None          # :247-250
    if entry[1] < cpos[1] - dxo2:                                # :257
        entry[1] = cpos[1] - dxo2
        if inout == 0:
            dir_flag = 1
        entry[0] = get_Z_from_R(pos, entry[1], tn, dir_flag)
    elif entry[1] > cpos[1] + dxo2:                              # :263
        entry[1] = cpos[1] + dxo2
        if inout == 0:
            dir_flag = 1
        entry[0] = get_Z_from_R(pos, entry[1], tn, dir_flag)
    if exit_[1] < cpos[1] - dxo2:                                # :274
        exit_[1] = cpos[1] - dxo2
        if inout == 0:
            dir_flag = -1
        exit_[0] = get_Z_from_R(pos, exit_[1], tn, dir_flag)
    elif exit_[1] > cpos[1] + dxo2:                              # :280
        exit_[1] = cpos[1] + dxo2
        if inout == 0:
            dir_flag = -1
        exit_[0] = get_Z_from_R(pos, exit_[1], tn, dir_flag)
    nxt = ray                                                    # :293
    if abs(exit_[1] - (cpos[1] + dxo2)) / dx < 1.0e-8 and dir_flag == -1:    # :297
        nxt = G.next(ray, 0, 1)
    elif abs(exit_[1] - (cpos[1] - dxo2)) / dx < 1.0e-8 and dir_flag == 1:   # :301
        nxt = G.next(ray, 0, -1)
    if abs(exit_[0] - (cpos[0] - dxo2)) / dx < 1.0e-8:           # :310 (angle < pi/2)
        nxt = G.next(nxt, -1, 0)
    if flag:                                                     # :318
        if inout == 1:
            exit_[1] = cpos[1] - dxo2
            exit_[0] = get_Z_from_R(pos, exit_[1], tn, inout)
            nxt = G.next(ray, 0, -1)
        elif inout == -1:
            entry[1] = cpos[1] - dxo2
            entry[0] = get_Z_from_R(pos, entry[1], tn, inout)
            if equalD(exit_[1], cpos[1] + dxo2):
                nxt = G.next(ray, 0, 1)
        return entry, exit_, (nxt if G.on(nxt) else None)        # :331; a cell off the grid is missing
    if not G.on(nxt):                                            # :334
        nxt = None
    return entry, exit_, nxt


def pixel(G, V, rel, n_extra, tn, invst, i, j, trip_limit):
    """the body of generate_angle_image's pixel loop, :456-681.  V: the fields, each [NR][NZ] (nested lists or arrays);
    rel: per field None or [NR][NZ] relative uncertainties of V.  Returns (ans, allowed, ncell, capped): allowed[f] is
    what `rel` and differently rounded additions may change, sum w |v| rel + (ncell + 1) eps sum w |v| (0 where rel is
    None: the same bits)"""
    nf = len(V)
    pos = pixel_centre(G, n_extra, i, j)                         # :458
    ray = get_start_of_ray(G, pos, tn)                           # :467
    pix_on_grid = False
    c = None
    if pos[0] < G.zmax and pos[0] > G.zmin:                      # :482
        pix_on_grid = True
        c = (i - n_extra, j)                                     # departure 1
    ans = [0.0] * nf                                             # :495-496
    mag, dev = [0.0] * nf, [0.0] * nf
    ncell = 0

    def add(integral, cell):                                     # add_cell_emission_to_ray's pattern, :372
        for f in range(nf):
            v = float(V[f][cell[1]][cell[0]])
            ans[f] = ans[f] + integral * v
            mag[f] += abs(integral * v)
            if rel[f] is not None:
                dev[f] += abs(integral * v) * float(rel[f][cell[1]][cell[0]])

    def done(capped):
        allowed = [0.0 if rel[f] is None else dev[f] + (ncell + 1) * EPS * mag[f] for f in range(nf)]
        return ans, allowed, ncell, capped

    if pos[0] < G.zmax - G.dx:                                   # :503
        inout = 1                                                # :509
        entry, exit_, next_cell = get_entry_exit_points(G, pos, tn, inout, ray)   # :511
        if not entry[1] > 1.0e90:                                # :513
            trips = 0
            while True:                                          # do { :520
                entry, exit_, next_cell = get_entry_exit_points(G, pos, tn, inout, ray)   # :524
                integral = invst * abs(math.sqrt(entry[1] * entry[1] - pos[1] * pos[1])
                                       - math.sqrt(exit_[1] * exit_[1] - pos[1] * pos[1]))   # :532-534
                add(integral, ray)                               # :536
                ray = next_cell                                  # :547
                ncell += 1
                trips += 1
                if pix_on_grid:                                  # :549-552, and departure 2
                    at_source = ray is None or ray == c
                else:                                            # :553-556
                    at_source = ray is None or equalD(G.cz(ray[0]), pos[0])
                if at_source:                                    # } while (!at_source) :557
                    break
                if trips >= trip_limit:
                    return done(True)
    if pix_on_grid and ray is not None:                          # :567, and departure 2
        inout = 0                                                # :579
        entry, exit_, next_cell = get_entry_exit_points(G, pos, tn, inout, ray)   # :581
        integral = invst * 2.0 * math.sqrt(entry[1] * entry[1] - pos[1] * pos[1])  # :584-585
        add(integral, ray)                                       # :587
        ray = next_cell                                          # :588
        ncell += 1
    if pos[0] > G.zmin + G.dx and ray is not None:               # :609
        inout = -1                                               # :617
        entry, exit_, next_cell = get_entry_exit_points(G, pos, tn, inout, ray)   # :619
        if not entry[1] > 1.0e90:                                # :621
            trips = 0
            while True:                                          # do { :633
                entry, exit_, next_cell = get_entry_exit_points(G, pos, tn, inout, ray)   # :640
                integral = invst * abs(math.sqrt(entry[1] * entry[1] - pos[1] * pos[1])
                                       - math.sqrt(exit_[1] * exit_[1] - pos[1] * pos[1]))   # :650-652
                add(integral, ray)                               # :654
                ray = next_cell                                  # :658
                ncell += 1
                trips += 1
                if ray is None:                                  # } while (ray != 0 && ray->isgd) :660
                    break
                if trips >= trip_limit:
                    return done(True)
    return done(False)


def image(NZ, NR, zmin, rmin, dx, angle_deg, V, rel=None, trip_limit=None, tn=None, invst=None):
    """generate_angle_image: returns a dict with n_extra, NI, img [nf][NR][NI] (nested lists, ipix = NI j + i, :675),
    allowed (the same shape), ncapped and the most cells any ray crossed"""
    G = Grid(NZ, NR, zmin, rmin, dx)
    _, t, s = angle_numbers(angle_deg)
    tn = t if tn is None else tn
    invst = s if invst is None else invst
    n_extra = n_extra_of(G, tn)
    NI = NZ + 2 * n_extra
    nf = len(V)
    rel = [None] * nf if rel is None else rel
    limit = 2 * (NZ + NR) + 8 if trip_limit is None else trip_limit
    img = [[[0.0] * NI for _ in range(NR)] for _ in range(nf)]
    allowed = [[[0.0] * NI for _ in range(NR)] for _ in range(nf)]
    ncapped, most = 0, 0
    for i in range(NI):                                          # :433
        for j in range(NR):                                      # :456
            ans, al, ncell, capped = pixel(G, V, rel, n_extra, tn, invst, i, j, limit)
            ncapped += 1 if capped else 0
            most = max(most, ncell)
            for f in range(nf):
                img[f][j][i] = ans[f]                            # :675-676
                allowed[f][j][i] = al[f]
    return dict(n_extra=n_extra, NI=NI, img=img, allowed=allowed, ncapped=ncapped, most_cells=most)


def chord(NZ, NR, zmin, rmin, dx, angle_deg, n_extra):
    """not a restatement: the exact length inside the cylinder zmin < z < zmax, R < rmax of the straight line of sight
    through pixel (i, j) -- in the (z,R) plane the hyperbola above.  With s the path length from the turning point,
    z = pos_z + s cos(angle) and R^2 = b^2 + s^2 sin^2(angle): |s| <= sqrt(rmax^2 - b^2) / sin and zmin <= z <= zmax.
    Only for a grid that starts at the axis (rmin == 0).  [NR][NI]"""
    angle = angle_deg * math.pi / 180.0
    ct, st = math.cos(angle), math.sin(angle)
    zmax, rmax = zmin + NZ * dx, rmin + NR * dx
    NI = NZ + 2 * n_extra
    out = [[0.0] * NI for _ in range(NR)]
    for j in range(NR):
        b = rmin + (j + 0.5) * dx
        S = math.sqrt(rmax * rmax - b * b) / st
        for i in range(NI):
            z0 = (zmin - n_extra * dx) + (i + 0.5) * dx
            lo, hi = max(-S, (zmin - z0) / ct), min(S, (zmax - z0) / ct)
            out[j][i] = max(0.0, hi - lo)
    return out
