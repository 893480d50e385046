// dev_bc.h -- the rules of the boundary update (boundaries/*.cpp of the reference), each stated once: which cells are
// ghost cells and in what order a launch enumerates them, which cell a ghost cell takes its value from, what a face
// does to that value, the double-Mach-reflection states, and which cell an assignment captures.  Plain
// __host__ __device__ index arithmetic, copies and multiplications by -1.0: the kernels of pion_bc.hip run them on the
// device, tests/native/bc_probe.cpp runs the same functions in host loops against the CPU oracle.  Needs only GridDesc
// and the PION_BC_* constants (the includer provides __host__ / __device__, as for rows_tiling.h).
#ifndef PION_DEV_BC_H
#define PION_DEV_BC_H

#include <cmath>

#include "../../include/pion_gpu.h"
#include "grid_desc.h"

namespace pion {

#define PION_BC_HD __host__ __device__ inline

// cell id from all-cell coordinates (ghosts included)
PION_BC_HD long all_cell_id(const GridDesc &g, const int *i) { return (long)i[0] + g.sy * i[1] + g.sz * i[2]; }

// ---- Ghost-slab enumeration.  All ghost cells of a grid as three disjoint slabs: A = z ghosts (all x, y), B = y
// ghosts on on-grid z (all x), C = x ghosts on on-grid y and z.  (An axis the grid does not have has nbc = 0 and
// ng = 1: its slab is empty.)  zghosts: slab A is included; skipx: slab C is left out.
PION_BC_HD long ghost_slab_a(const GridDesc &g, const bool zghosts)
{
  return zghosts ? (long)2 * g.nbc[2] * g.nga[0] * g.nga[1] : 0;
}
PION_BC_HD long ghost_slab_b(const GridDesc &g) { return (long)g.ng[2] * 2 * g.nbc[1] * g.nga[0]; }
PION_BC_HD long ghost_slab_count(const GridDesc &g, const bool zghosts, const bool skipx)
{
  return ghost_slab_a(g, zghosts) + ghost_slab_b(g) + (skipx ? 0 : (long)g.ng[2] * g.ng[1] * 2 * g.nbc[0]);
}
// all-cell coordinates of ghost cell t < ghost_slab_count
PION_BC_HD void ghost_slab_cell(const GridDesc &g, const bool zghosts, long t, int *i)
{
  const long nA = ghost_slab_a(g, zghosts), nB = ghost_slab_b(g);
  if (t < nA) {
    i[0] = (int)(t % g.nga[0]);
    i[1] = (int)((t / g.nga[0]) % g.nga[1]);
    const int kz = (int)(t / ((long)g.nga[0] * g.nga[1]));
    i[2] = (kz < g.nbc[2]) ? kz : g.ng[2] + kz;
  }
  else if (t < nA + nB) {
    t -= nA;
    i[0] = (int)(t % g.nga[0]);
    const int ky = (int)((t / g.nga[0]) % (2 * g.nbc[1]));
    i[1] = (ky < g.nbc[1]) ? ky : g.ng[1] + ky;
    i[2] = (int)(t / ((long)g.nga[0] * 2 * g.nbc[1])) + g.nbc[2];
  }
  else {
    t -= nA + nB;
    const int kx = (int)(t % (2 * g.nbc[0]));
    i[0] = (kx < g.nbc[0]) ? kx : g.ng[0] + kx;
    i[1] = (int)((t / (2 * g.nbc[0])) % g.ng[1]) + g.nbc[1];
    i[2] = (int)(t / ((long)2 * g.nbc[0] * g.ng[1])) + g.nbc[2];
  }
}

// All faces periodic: the X -> Y -> Z sequence of periodic copies (periodic_boundaries.cpp:42-50, corner cells through
// already filled ghosts) ends with every ghost cell holding the on-grid cell at its coordinates wrapped axis by axis
// (z only if zwrap: SLAB z faces belong to the neighbour ranks).
PION_BC_HD void periodic_wrap(const GridDesc &g, const bool zwrap, const int *i, int *s)
{
  for (int ax = 0; ax < 3; ax++) {
    s[ax] = i[ax];
    if (ax == 2 && !zwrap) continue;
    if (s[ax] < g.nbc[ax]) s[ax] += g.ng[ax];
    else if (s[ax] >= g.nbc[ax] + g.ng[ax]) s[ax] -= g.ng[ax];
  }
}

// ---- Cell list of face d = 2 * axis + side (UniformGrid::SetupBCs, grid/uniform_grid.cpp:1009-1216): the nbc ghost
// layers along the face's axis, the FULL extent of the lower axes and the ON-GRID extent of the higher ones, which
// together with the X -> Y -> Z order fills the corner ghosts as the reference does.
struct FaceList {
  int lo[3], n[3];   // first all-cell coordinate and extent per axis
  long total;
};
PION_BC_HD FaceList face_list(const GridDesc &g, const int d)
{
  const int ax = d / 2;
  FaceList f;
  for (int a = 0; a < 3; a++) {
    const bool full = (a < ax || a >= g.ndim);   // (an axis the grid does not have: its one cell)
    f.lo[a] = (a == ax) ? ((d & 1) ? g.nbc[a] + g.ng[a] : 0) : (full ? 0 : g.nbc[a]);
    f.n[a] = (a == ax) ? g.nbc[a] : (full ? g.nga[a] : g.ng[a]);
  }
  f.total = (long)f.n[0] * f.n[1] * f.n[2];
  return f;
}
// all-cell coordinates of list cell t < f.total
PION_BC_HD void face_list_cell(const FaceList &f, const long t, int *i)
{
  i[0] = (int)(t % f.n[0]) + f.lo[0];
  i[1] = (int)((t / f.n[0]) % f.n[1]) + f.lo[1];
  i[2] = (int)(t / ((long)f.n[0] * f.n[1])) + f.lo[2];
}

// ---- What a face does with a ghost cell
PION_BC_HD bool bc_is_constant(const int type)
{
  return type == PION_BC_INFLOW || type == PION_BC_FIXED || type == PION_BC_DMACH;
}
// every ghost layer copies the FIRST on-grid cell of its row (outflow_boundaries.cpp:50-59)
PION_BC_HD bool bc_copies_edge(const int type)
{
  return type == PION_BC_OUTFLOW || type == PION_BC_ONEWAY_OUT || type == PION_BC_REFLECTING
         || type == PION_BC_AXISYMMETRIC || type == PION_BC_JETREFLECT;
}
// nobody's to fill: unset, a neighbour rank's (SLAB), or no face type at all
PION_BC_HD bool bc_is_unset(const int type)
{
  return !(type == PION_BC_PERIODIC || bc_is_constant(type) || bc_copies_edge(type));
}

// The operation of one face (axis ax, side pos) on variable v of the state vector its ghost cell copied, x (for psi: of
// the psi source, bc_chain).  Sign flips: reflecting_boundaries.cpp:34-73,131-153 (normal velocity and normal B),
// axisymmetric_boundaries.cpp:34-52,98-137 (R = 0 axis: the radial and the theta components),
// jetreflect_boundaries.cpp:32-62 (v_n and the two tangential field components).
PION_BC_HD double bc_face_op(const int type, const int ax, const bool pos, const bool mhd, const bool glm, const int v,
                             const double x)
{
  const bool vn = (v == 2 + ax), bn = (mhd && v == 5 + ax), bt = (mhd && v >= 5 && v <= 7 && !bn);
  if (type == PION_BC_REFLECTING) return (vn || bn) ? x * -1.0 : x;
  if (type == PION_BC_AXISYMMETRIC) return (v == 3 || v == 4 || (mhd && (v == 6 || v == 7))) ? x * -1.0 : x;
  if (type == PION_BC_JETREFLECT) return (vn || bt) ? x * -1.0 : x;
  if (type == PION_BC_ONEWAY_OUT && vn) {
    // oneway_out_boundaries.cpp:75-138
    const double sg = pos ? 1.0 : -1.0, xs = x * sg;
    return sg * ((0.0 < xs) ? xs : 0.0);
  }
  // GLM_NEGATIVE_BOUNDARY (boundaries.h:21)
  if ((type == PION_BC_OUTFLOW || type == PION_BC_ONEWAY_OUT) && glm && v == 8) return -x;
  return x;
}

// ---- Double Mach reflection (double_Mach_ref_boundaries.cpp)
// variable v of the post-shock state: behind the shock line on the YP face (:168-204) and on the internal DMR2
// boundary (:98-147)
PION_BC_HD double dmr_post_shock(const int nvar, const int ntracer, const int v)
{
  if (v >= nvar - ntracer) return 1.0;
  return v == 0 ? 8.0 : (v == 1 ? 116.5 : (v == 2 ? 7.14470958 : (v == 3 ? -4.125 : 0.0)));
}
// of the pre-shock state BC_assign_DMACH gives the YP face (:36-44)
PION_BC_HD double dmr_pre_shock(const int nvar, const int ntracer, const int v)
{
  if (v >= nvar - ntracer) return -1.0;
  return v == 0 ? 1.4 : (v == 1 ? 1.0 : 0.0);
}
// centre of the cell with all-cell coordinate i along ax (cell_interface.cpp:506-512)
PION_BC_HD double cell_centre(const GridDesc &g, const int ax, const int i)
{
  return g.xmin[ax] + (2 * (i - g.nbc[ax]) + 1) * (0.5 * g.dx);
}
// is the cell (all-cell coordinates i0, i1; either may be a ghost) behind the shock line at the time of dmr_a0 ?
// dmr_a0 = 10 * simtime / sin(pi/3), dmr_t3 = tan(pi/3), both from the host's libm as the reference's
PION_BC_HD bool dmr_behind_shock(const GridDesc &g, const double dmr_a0, const double dmr_t3, int i0, int i1)
{
  const double x = cell_centre(g, 0, i0), y = cell_centre(g, 1, i1);
  const double bpos = dmr_a0 + 1.0 / 6.0 + y / dmr_t3;
  return x <= bpos;
}
// DMR2: the on-grid columns with x <= 1/6, whose y < 0 ghost cells hold the post-shock state
PION_BC_HD int dmr2_columns(const GridDesc &g)
{
  int n = 0;
  while (n < g.ng[0] && cell_centre(g, 0, g.nbc[0] + n) <= 1. / 6.) n++;
  return n;
}

// ---- What every rule below and every kernel of pion_bc.hip reads
struct BCArgs {
  GridDesc g;
  double *T;        // array whose ghosts are filled (sources are read from the same array)
  int nvar, eqntype, ntracer;
  int type[6];      // per face; 0 beyond the grid's axes
  double refval[6][PION_MAX_NVAR];   // inflow / fixed / pre-shock states as assigned
  double dmr_a0, dmr_t3;
  int dmr2_cols;    // > 0: internal DMR2 boundary over the first dmr2_cols on-grid columns
};
inline BCArgs bc_args(const GridDesc &g, const pion_gpu_config &cfg, const double (*refval)[PION_MAX_NVAR],
                      const int dmr2_cols, double *T, const double simtime)
{
  BCArgs a;
  a.g = g;
  a.T = T;
  a.nvar = cfg.nvar;
  a.eqntype = cfg.eqntype;
  a.ntracer = cfg.ntracer;
  for (int d = 0; d < 6; d++) {
    a.type[d] = (d < 2 * cfg.ndim) ? cfg.bc_type[d] : 0;
    for (int v = 0; v < PION_MAX_NVAR; v++) a.refval[d][v] = refval[d][v];
  }
  a.dmr_a0 = 10.0 * simtime / sin(M_PI / 3.0);
  a.dmr_t3 = tan(M_PI / 3.0);
  a.dmr2_cols = cfg.bc_dmach2 ? dmr2_cols : 0;
  return a;
}
// cell t < dmr2_cols * nbc[1] of the DMR2 boundary: the y < 0 ghost cells above its columns
PION_BC_HD void dmr2_cell(const BCArgs &a, const int t, int *i)
{
  i[0] = a.g.nbc[0] + t % a.dmr2_cols;
  i[1] = a.g.nbc[1] - 1 - t / a.dmr2_cols;
  i[2] = 0;
}
// does the DMR2 boundary hold cell i ?
PION_BC_HD bool dmr2_holds(const BCArgs &a, const int *i)
{
  return a.dmr2_cols > 0 && i[1] < a.g.nbc[1] && i[0] >= a.g.nbc[0] && i[0] < a.g.nbc[0] + a.dmr2_cols;
}

// ---- Source-cell chain.  The reference updates the faces one after the other in list order XN, XP, YN, YP, ZN, ZP
// (assign_update_bcs.cpp:185-252); a ghost cell belongs to the list of the HIGHEST axis along which it is a ghost, and
// a corner ghost takes its value from a ghost cell that a lower axis's update has just filled.  That chain of copies
// always ends on an on-grid cell (or on a constant state), which no boundary update writes.  So: walk the chain of one
// ghost cell down the axes ax_hi .. ax_lo, read the terminal cell, and apply the per-face operations on the way back
// up, lowest axis first -- the same values as the launches face by face, without their ordering.  psi of GLM-MHD
// follows its own chain: outflow and one-way faces take -psi of the MIRROR cell (outflow_boundaries.cpp:140-152),
// everything else of the copy source.  ax_hi = ax_lo = the axis of one face: that face's own update, its lower-axis
// neighbours read as they stand.
struct BcChain {
  int s[3], p[3];               // source cell of every variable but psi; of psi
  int op_type[3], op_pos[3];    // face met along each axis (type 0: none)
  int const_ax;                 // axis whose face gives a constant / analytic state: the chain ends there (-1: none)
};
// false: the cell is not ours to fill (the first ghost axis met is the list the cell belongs to; its face is unset)
PION_BC_HD bool bc_chain(const GridDesc &g, const int *type, const bool glm, const int *i, const int ax_hi,
                         const int ax_lo, BcChain &ch)
{
  for (int ax = 0; ax < 3; ax++) {
    ch.s[ax] = ch.p[ax] = i[ax];
    ch.op_type[ax] = ch.op_pos[ax] = 0;
  }
  ch.const_ax = -1;
  bool owned = false;
  for (int ax = ax_hi; ax >= ax_lo; ax--) {
    const int lo = g.nbc[ax], hi = g.nbc[ax] + g.ng[ax];
    int &s = ch.s[ax];
    if (s >= lo && s < hi) continue;   // on-grid along this axis
    const bool pos = (s >= hi);
    const int t = type[2 * ax + (pos ? 1 : 0)];
    if (bc_is_unset(t)) {
      // (below the owning axis: the source is that ghost cell as it stands)
      if (!owned) return false;
      break;
    }
    owned = true;
    ch.op_type[ax] = t;
    ch.op_pos[ax] = pos ? 1 : 0;
    if (bc_is_constant(t)) {
      ch.const_ax = ax;
      break;
    }
    if (t == PION_BC_PERIODIC) {
      // periodic_boundaries.cpp:42-50: NG(axis) cells back onto the grid
      s += pos ? -g.ng[ax] : g.ng[ax];
      ch.p[ax] = s;
      continue;
    }
    const int depth = pos ? s - hi + 1 : lo - s;   // distance from the grid = -isedge
    s = pos ? hi - 1 : lo;
    // psi_ghost(layer depth) = -psi(on-grid cell depth) on outflow / one-way faces
    if (glm && (t == PION_BC_OUTFLOW || t == PION_BC_ONEWAY_OUT)) ch.p[ax] = pos ? hi - depth : lo + depth - 1;
    else ch.p[ax] = s;
  }
  return true;
}

// The value of ghost cell i (all-cell coordinates) after the updates of the faces of axes ax_lo .. ax_hi, from the
// array T as it stands.  false: not ours to fill, val untouched.  (Loops over the variables: unrolled, so that val
// stays in registers.)
#define PION_BC_EACH_VAR(v, nvar) _Pragma("unroll") for (int v = 0; v < PION_MAX_NVAR; v++) if (v < (nvar))
PION_BC_HD bool bc_ghost_value(const BCArgs &a, const double *T, const int *i, const int ax_hi, const int ax_lo,
                               double *val)
{
  const GridDesc &g = a.g;
  const bool mhd = (a.eqntype == PION_EQMHD || a.eqntype == PION_EQGLM);
  const bool glm = (a.eqntype == PION_EQGLM);
  BcChain ch;
  if (!bc_chain(g, a.type, glm, i, ax_hi, ax_lo, ch)) return false;
  int from = ax_lo;   // first axis whose operation is applied on the way up
  if (ch.const_ax >= 0) {
    const int d = 2 * ch.const_ax + ch.op_pos[ch.const_ax];
    // (DMACH: position of the ghost cell of the Y list, x may be a ghost; double_Mach_ref_boundaries.cpp:168-204)
    const bool post = (a.type[d] == PION_BC_DMACH && dmr_behind_shock(g, a.dmr_a0, a.dmr_t3, ch.s[0], ch.s[1]));
    PION_BC_EACH_VAR(v, a.nvar) val[v] = post ? dmr_post_shock(a.nvar, a.ntracer, v) : a.refval[d][v];
    from = ch.const_ax + 1;
  }
  else {
    const long sc = all_cell_id(g, ch.s), pc = all_cell_id(g, ch.p);
    PION_BC_EACH_VAR(v, a.nvar) val[v] = T[v * g.ncell + ((glm && v == 8) ? pc : sc)];
  }
  for (int ax = from; ax <= ax_hi; ax++)
    PION_BC_EACH_VAR(v, a.nvar) val[v] = bc_face_op(ch.op_type[ax], ax, ch.op_pos[ax] != 0, mhd, glm, v, val[v]);
  return true;
}
PION_BC_HD void bc_store(double *T, const GridDesc &g, const int *i, const int nvar, const double *val)
{
  const long c = all_cell_id(g, i);
  PION_BC_EACH_VAR(v, nvar) T[v * g.ncell + c] = val[v];
}

// ---- Assignment.  BC_assign_INFLOW / BC_assign_FIXED read their constant state from the state array once, when the
// boundary is assigned: the source (first on-grid cell of the row) of the LAST cell of the face's list for inflow
// (inflow_boundaries.cpp), of the FIRST for fixed (fixed_boundaries.cpp:62-76).  All-cell coordinates.
PION_BC_HD void bc_capture_cell(const GridDesc &g, const int d, const bool inflow, int *i)
{
  const FaceList f = face_list(g, d);
  face_list_cell(f, inflow ? f.total - 1 : 0, i);
  const int ax = d / 2;
  i[ax] = (d & 1) ? g.nbc[ax] + g.ng[ax] - 1 : g.nbc[ax];
}

// ---- Which launches an update takes
enum BcMode { BC_MODE_PERIODIC_ALL, BC_MODE_ONE_LAUNCH, BC_MODE_FACE_SEQUENCE };
// fuse_bc: PION_FUSE_BC; any_wind: wind cells present (their ghost images are not fused into one launch); assign: the
// boundaries are being assigned (inflow / fixed states are captured face by face, after the lower faces were filled)
inline BcMode bc_mode(const pion_gpu_config &cfg, const bool fuse_bc, const bool any_wind, const bool assign)
{
  // every face periodic (z possibly handed to the neighbour ranks, both faces alike): one launch wraps all ghosts.
  // (A 2-D grid with SLAB y faces goes through the one launch for any mix.)
  bool all_periodic = (!any_wind && !cfg.bc_dmach2 && fuse_bc);
  for (int d = 0; d < 2 * cfg.ndim && all_periodic; d++) {
    const bool zface = (d >= 4);
    if (!(cfg.bc_type[d] == PION_BC_PERIODIC || (zface && cfg.bc_type[d] == PION_BC_SLAB))) all_periodic = false;
  }
  if (all_periodic && cfg.ndim == 3 && cfg.bc_type[4] != cfg.bc_type[5]) all_periodic = false;
  if (all_periodic) return BC_MODE_PERIODIC_ALL;
  return (!assign && fuse_bc) ? BC_MODE_ONE_LAUNCH : BC_MODE_FACE_SEQUENCE;
}

}  // namespace pion
#endif
