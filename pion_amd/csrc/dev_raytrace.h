// dev_raytrace.h -- the rules of the ray-traced column densities (pion_gpu_raytrace, pion_gpu_raytrace_host), each
// stated once: the reference's short-characteristics tracer raytracer_USC (source/raytracing/raytracer_SC.cpp; all
// line numbers below are that file's) for the opacity rules that need no microphysics object.  Plain
// __host__ __device__ functions of GridDesc, written the way dev_project.h is: the kernels of pion_raytrace.hip run
// them on the device, pion_gpu_raytrace_host runs the same functions in a host loop.  The includer provides
// __host__ / __device__.
//
// Every function that does arithmetic is compiled without FMA contraction, in both builds and on the host (the pragma
// below for clang; pion_raytrace.hip is built with -ffp-contract=off as well): columns are compared with == against a
// restatement.  Square root and division are correctly rounded on both sides; nothing else is called.
//
// ---- integer positions (cell_interface: cell size 2).  A cell with on-grid index i sits at 2 i + 1, a vertex at an
//      even number; a finite source is moved to the nearest vertex per axis (centre_source_on_cell, 1934-1996), so
//      every per-axis distance d_a = |2 i_a + 1 - ipos_a| is odd and >= 1.
// ---- a point source (cell_cols_2d 2132-2278, cell_cols_3d 2287-2486, col2cell_2d/3d 2495-2615, interpolate_2D/3D
//      2627-2682): rt_col2cell_2d / rt_col2cell_3d give the column TO the cell and the path length ds through it from
//      the finished columns of up to four neighbours one step nearer the source along the axis of the largest
//      distance.  A neighbour that is not an on-grid cell contributes 0 (ProcessCell 887-898 and the null-pointer
//      branches of col2cell_*): the caller's `colat` returns 0.0 there.  One exception, in a part of a decomposed run
//      (rt_role): a cell one plane beyond the slab face that looks towards the source, inside the grid on the other
//      axes, gives the column the neighbouring rank handed over -- unclamped (the reference clamps what it receives at
//      0, RT_MPI_boundaries.cpp:352,364; here a decomposed run gives the bits of the single grid).  A cell of that
//      plane that is off the grid on another axis still gives 0.0.
// ---- the column THROUGH the cell (ProcessCell 855-1057): rt_dcol, ds rho, ds rho (1 - y), ds rho y.
//      col = col_to_cell + dcol is what CI.get_col returns afterwards.
// ---- a source at infinity (trace_parallel_rays 695-792): ds = dx and col is the running sum along the axis from the
//      face the source lies beyond, the additions one after the other in ray order: col = col_before + dcol.  In a
//      part, along the slab axis, the sum starts from the plane handed over instead of 0.
// ---- the dependency.  With k_a = (d_a - 1) / 2 the cells of one level L = sum_a k_a read only cells of lower levels
//      in their own octant: rt_plan_of describes the levels and, for tiles of RT_TILE cells counted from the source
//      vertex outwards (tile index t_a = k_a / tile_a), the tile-levels T = sum_a t_a with the same property.
#ifndef PION_DEV_RAYTRACE_H
#define PION_DEV_RAYTRACE_H

#include <cmath>

#include "../../include/pion_gpu.h"
#include "grid_desc.h"

#if defined(__clang__)
#pragma clang fp contract(off)
#endif

namespace pion {

#define PION_RT_HD __host__ __device__ inline

// a source as the kernels take it
struct RtSrc {
  int ipos[3];      // the vertex, integer units from the low corner of the on-grid region (finite sources)
  int at_infinity;
  int dir;          // at infinity: the face the source lies beyond, 0..5 = XN XP YN YP ZN ZP
  int opacity;      // PION_RT_OPACITY_*
  int var;          // state index of the tracer y (first tracer + opacity_var); unused for TOTAL
  double taumin;    // set_TauMin_for_source, 1323-1336
};

// ---- what is refused: null, or the text of the refusal.  slab_ok: the caller describes the handle as a part of a
// decomposed domain (RtPart below), so a PION_BC_SLAB face of the slab axis is no reason to refuse.
inline const char *rt_refused_as(const pion_gpu_config &c, const pion_gpu_rt_source *s, const bool slab_ok)
{
  if (!s) return "raytrace: no source";
  if (c.ndim == 1 || c.coord_sys == 3) return "raytrace: 1-D and spherical grids are not traced";
  if (c.ndim < 2 || c.ndim > 3) return "raytrace: a grid has 2 or 3 dimensions";
  for (int d = 0; d < 2 * c.ndim; d++)
    if (c.bc_type[d] == PION_BC_SLAB && !(slab_ok && d / 2 == c.ndim - 1))
      return "raytrace: a slab of a decomposed run is not traced (columns are not handed from rank to rank)";
  if (s->opacity < PION_RT_OPACITY_TOTAL || s->opacity > PION_RT_OPACITY_TRACER)
    return "raytrace: the opacity rule needs a microphysics object (TOTAL, MINUS and TRACER are covered)";
  if (s->opacity != PION_RT_OPACITY_TOTAL && (s->opacity_var < 0 || s->opacity_var >= c.ntracer))
    return "raytrace: opacity_var is not a tracer of the state";
  if (s->at_infinity) {
    if (s->dir < 0 || s->dir >= 2 * c.ndim) return "raytrace: the direction of a source at infinity is a face of the grid";
  }
  else {
    for (int a = 0; a < c.ndim; a++)
      if (!(std::fabs(s->pos[a]) <= 1.0e100)) return "raytrace: the position of a finite source is finite";
  }
  return nullptr;
}
inline const char *rt_refused(const pion_gpu_config &c, const pion_gpu_rt_source *s) { return rt_refused_as(c, s, false); }

// a part: the handle holds the planes [plane_lo, plane_lo + n) of the slab axis (z in 3-D, y in 2-D; n = the handle's own
// ng of that axis) out of global_planes, and the whole domain starts at global_xmin along that axis.
inline const char *rt_part_refused(const pion_gpu_config &c, const pion_gpu_rt_source *s, const pion_gpu_rt_part *part)
{
  if (const char *e = rt_refused_as(c, s, true)) return e;
  if (!part) return "raytrace: no part";
  if (part->plane_lo < 0 || part->plane_lo + (long)c.ng[c.ndim - 1] > part->global_planes)
    return "raytrace: the part's planes lie outside the whole domain";
  if (!(std::fabs(part->global_xmin) <= 1.0e100)) return "raytrace: the part's global_xmin is not finite";
  return nullptr;
}

// constants::equalD (constants.cpp:48-69)
inline bool rt_equalD(const double a, const double b)
{
  if (a == b) return true;
  if (std::fabs(a) + std::fabs(b) < 1.0e-100) return true;
  return (std::fabs(a - b) / (std::fabs(a) + std::fabs(b) + 1.0e-100)) < 1.0e-12;
}

// centre_source_on_cell (1934-1996) for one axis: the moved position
inline double rt_centre_on_vertex(const double pos_in, const double xmin, const double dx)
{
  double pos = pos_in;
  double dist = pos - xmin;
  const int x = static_cast<int>(dist / dx);
  dist -= x * dx;
  dist /= dx;
  if (!rt_equalD(dist, 0.0)) {
    if (rt_equalD(dist, 0.5)) {
      if (dist > 0) pos -= dist * dx;
      else pos -= (1.0 + dist) * dx;
    }
    else if (dist > 0.0 && dist > 0.5) pos += (1.0 - dist) * dx;
    else if (dist > 0.0 && dist <= 0.5) pos -= dist * dx;
    else if (dist < 0.0 && dist <= -0.5) pos -= (1.0 + dist) * dx;
    else if (dist < 0.0 && dist > -0.5) pos -= dist * dx;
  }
  return pos;
}

// add_source_to_list (1217-1314) without the cell pointer: the moved position and the kernel's view of the source.
// cell_interface::get_ipos_vec (cell_interface.cpp:553-571) gives the integer position.
// A part (null: the grid of c is the whole domain): the position is one of the WHOLE domain.  Along the slab axis the
// vertex is found from global_xmin, exactly as on the whole grid, and then shifted by 2 plane_lo into the integer units
// of the slab; it is never found from the slab's own xmin, so that no two ranks can settle on different vertices.
// pos_used is the whole-domain position on every rank.
inline RtSrc rt_make_source(const pion_gpu_config &c, const pion_gpu_rt_source &s, double pos_used[3],
                            const pion_gpu_rt_part *part = nullptr)
{
  RtSrc r;
  r.at_infinity = s.at_infinity ? 1 : 0;
  r.dir = s.dir;
  r.opacity = s.opacity;
  r.var = c.nvar - c.ntracer + s.opacity_var;
  r.taumin = 0.7;
  if (c.ndim == 3) r.taumin *= 6.0 / 7.0;
  for (int a = 0; a < 3; a++) {
    r.ipos[a] = 0;
    double p = (a < c.ndim) ? s.pos[a] : 0.0;
    if (a < c.ndim && !r.at_infinity) {
      const bool slab_axis = part && a == c.ndim - 1;
      const double xmin = slab_axis ? part->global_xmin : c.xmin[a];
      p = rt_centre_on_vertex(p, xmin, c.dx);
      r.ipos[a] = static_cast<int>((1.0 + 1.0e-12) * ((p - xmin) / (0.5 * c.dx)));
      // (a vertex by construction; an odd number here could only come from a position beyond 2^52 cells)
      if (r.ipos[a] & 1) r.ipos[a] += (r.ipos[a] > 0) ? 1 : -1;
      if (slab_axis) r.ipos[a] -= 2 * part->plane_lo;
    }
    if (pos_used) pos_used[a] = p;
  }
  return r;
}

// ---- roles in the chain of a decomposed run.  The columns of a plane are finished by the rank that holds it; a cell
// reads cells one step nearer the source along the axis of its largest distance and 0 or 1 step along the others, so one
// plane of col per internal face is all that crosses.  The rank whose planes hold the source's vertex plane v
// (plane_lo <= v < plane_lo + n; a source beyond the domain: rank 0 or the last rank) receives nothing and sends both
// ways; a rank above it receives from below and sends upwards, a rank below it the other way round.  A vertex on an
// internal face: the cells beside it have d = 1 and never read across it, the message is sent all the same.  A source at
// infinity along the slab axis starts from the rank at the face it lies beyond; across the slab axis nothing crosses.
// recv_side: PION_RT_RECV_NONE / _BELOW / _ABOVE; send_lo, send_hi: 1 where the neighbour below / above is sent to.
struct RtRole { int recv_side, send_lo, send_hi; };

inline RtRole rt_role(const pion_gpu_config &c, const pion_gpu_rt_source &s, const pion_gpu_rt_part &part)
{
  RtRole r = {PION_RT_RECV_NONE, 0, 0};
  const int n = c.ng[c.ndim - 1];
  const bool first = part.plane_lo == 0, last = part.plane_lo + n == part.global_planes;
  int where;   // -1: the rank's planes lie below the one that starts the chain, 0: it starts it, 1: above
  if (s.at_infinity) {
    if (s.dir / 2 != c.ndim - 1) return r;
    where = (s.dir & 1) ? (last ? 0 : -1) : (first ? 0 : 1);
  }
  else {
    const RtSrc k = rt_make_source(c, s, nullptr, &part);
    const int v = k.ipos[c.ndim - 1] / 2;   // in the slab's own planes
    where = (v < 0 && !first) ? 1 : (v >= n && !last) ? -1 : 0;
  }
  if (where > 0) r.recv_side = PION_RT_RECV_BELOW;
  if (where < 0) r.recv_side = PION_RT_RECV_ABOVE;
  r.send_lo = where <= 0 && !first;
  r.send_hi = where >= 0 && !last;
  return r;
}

// ---- the column through the cell (ProcessCell 933-953)
PION_RT_HD double rt_dcol(const int opacity, const double ds, const double rho, const double y)
{
  if (opacity == PION_RT_OPACITY_MINUS) return ds * rho * (1.0 - y);
  if (opacity == PION_RT_OPACITY_TRACER) return ds * rho * y;
  return ds * rho;
}

PION_RT_HD double rt_max(const double a, const double b) { return (a < b) ? b : a; }   // std::max

// interpolate_2D (2627-2645)
PION_RT_HD double rt_interp2(const double taumin, const double delta0, const double tau1, const double tau2)
{
  double w1 = (1. - delta0) / rt_max(taumin, tau1);
  double w2 = delta0 / rt_max(taumin, tau2);
  const double sum = (w1 + w2);
  w1 /= sum;
  w2 /= sum;
  return w1 * tau1 + w2 * tau2;
}

// interpolate_3D (2658-2682)
PION_RT_HD double rt_interp3(const double taumin, const double delta0, const double delta1, const double tau1,
                             const double tau2, const double tau3, const double tau4)
{
  double w1 = (1. - delta0) * (1. - delta1) / rt_max(taumin, tau1);
  double w2 = delta0 * (1. - delta1) / rt_max(taumin, tau2);
  double w3 = (1. - delta0) * delta1 / rt_max(taumin, tau3);
  double w4 = delta0 * delta1 / rt_max(taumin, tau4);
  const double sum = (w1 + w2 + w3 + w4);
  w1 /= sum;
  w2 /= sum;
  w3 /= sum;
  w4 /= sum;
  return w1 * tau1 + w2 * tau2 + w3 * tau3 + w4 * tau4;
}

// the geometric factor of the source column (2245-2252, 2408-2420): idx = 2, idxo2 = 1
PION_RT_HD double rt_column_factor(const int dmax)
{
  const double maxd = static_cast<double>(dmax);
  const double maxmin2 = maxd - 2.0;
  return std::sqrt((maxd * maxd + 1.0 * 1.0) / (maxmin2 * maxmin2 + 1.0 * 1.0)) * maxmin2 / maxd;
}

// per-axis distance and the step towards the source, for the on-grid cell index i
PION_RT_HD int rt_dist(const int i, const int ipos) { const int d = 2 * i + 1 - ipos; return d < 0 ? -d : d; }
PION_RT_HD int rt_step(const int i, const int ipos) { return (2 * i + 1 > ipos) ? -1 : 1; }

// cell_cols_2d (2132-2278).  colat(ix, iy, iz): the finished column of an on-grid cell, 0.0 elsewhere.
template <class ColAt>
PION_RT_HD double rt_col2cell_2d(const RtSrc &s, const double dx, const int ix, const int iy, const ColAt &colat, double *ds)
{
  const int diffx = rt_dist(ix, s.ipos[0]), diffy = rt_dist(iy, s.ipos[1]);
  const int sx = rt_step(ix, s.ipos[0]), sy = rt_step(iy, s.ipos[1]);
  double delta;
  int mindiff, maxdiff, ex, ey, px, py;   // entry and perpendicular steps
  if (diffx >= diffy) {
    ex = sx; ey = 0; px = 0; py = sy;
    delta = static_cast<double>(diffy) / static_cast<double>(diffx);
    mindiff = diffy;
    maxdiff = diffx;
  }
  else {
    ex = 0; ey = sy; px = sx; py = 0;
    delta = static_cast<double>(diffx) / static_cast<double>(diffy);
    mindiff = diffx;
    maxdiff = diffy;
  }
  *ds = dx * std::sqrt(1.0 + delta * delta);
  if (mindiff < 2 && maxdiff < 2) return 0.0;
  if (mindiff < 2) {
    double N = rt_max(colat(ix + ex, iy + ey, 0), 0.0);
    if (maxdiff < 20) N *= rt_column_factor(maxdiff);
    return N;
  }
  const double col1 = colat(ix + ex, iy + ey, 0);
  const double col2 = colat(ix + ex + px, iy + ey + py, 0);
  return rt_interp2(s.taumin, delta, col1, col2);
}

// cell_cols_3d (2287-2486)
template <class ColAt>
PION_RT_HD double rt_col2cell_3d(const RtSrc &s, const double dx, const int ix, const int iy, const int iz,
                                 const ColAt &colat, double *ds)
{
  const int i[3] = {ix, iy, iz};
  int d[3], st[3];
  for (int a = 0; a < 3; a++) {
    d[a] = rt_dist(i[a], s.ipos[a]);
    st[a] = rt_step(i[a], s.ipos[a]);
  }
  int o0 = 0, o1 = 1, o2 = 2, t;
  if (d[o2] > d[o1]) { t = o2; o2 = o1; o1 = t; }
  if (d[o0] <= d[o1]) { t = o0; o0 = o1; o1 = t; }
  if (d[o1] <= d[o2]) { t = o1; o1 = o2; o2 = t; }
  const double delta0 = static_cast<double>(d[o1]) / static_cast<double>(d[o0]);
  const double delta1 = static_cast<double>(d[o2]) / static_cast<double>(d[o0]);
  *ds = dx * std::sqrt(1. + delta0 * delta0 + delta1 * delta1);

  if (d[o0] < 2) return 0.0;
  int c1[3] = {ix, iy, iz};
  c1[o0] += st[o0];
  if (d[o1] < 2) {
    double N = rt_max(colat(c1[0], c1[1], c1[2]), 0.0);
    if (d[o0] < 15) N *= rt_column_factor(d[o0]);
    return N;
  }
  int c2[3] = {c1[0], c1[1], c1[2]};
  c2[o1] += st[o1];
  const double col1 = colat(c1[0], c1[1], c1[2]);
  const double col2 = colat(c2[0], c2[1], c2[2]);
  if (d[o2] < 2) {
    double N = rt_interp2(s.taumin, delta0, col1, col2);
    if (d[o0] < 10) {
      if (d[o0] == 3) N *= 0.8388704928;
      else {
        const double one_over_r2 = 1.0 / (d[o0] * d[o0] + d[o1] * d[o1]);
        const double one_over_a2r2 = static_cast<double>(d[o0] * d[o0]) / ((d[o0] - 2.0) * (d[o0] - 2.0)) * one_over_r2;
        N *= (1.0 + one_over_r2) * (1.0 - one_over_a2r2);
      }
    }
    return N;
  }
  int c3[3] = {c1[0], c1[1], c1[2]};
  c3[o2] += st[o2];
  int c4[3] = {c2[0], c2[1], c2[2]};
  c4[o2] += st[o2];
  const double col3 = colat(c3[0], c3[1], c3[2]);
  const double col4 = colat(c4[0], c4[1], c4[2]);
  return rt_interp3(s.taumin, delta0, delta1, col1, col2, col3, col4);
}

// ---- levels and tiles.  Per axis and side (0: cells below the vertex, i = v - 1 - k; 1: cells above, i = v + k, with
// v = ipos / 2) the on-grid cells are k in [klo, khi]; khi < klo: that side has none.
struct RtPlan {
  int ndim;
  int v[3];
  int klo[3][2], khi[3][2];
  int tile[3];
  long level_lo, level_hi;   // cell levels L = sum k_a that hold cells
  long tlevel_lo, tlevel_hi; // tile-levels T = sum (k_a / tile_a) that hold tiles
};

constexpr int RT_TILE3[3] = {16, 8, 8};   // 3-D: lanes = the tile's 8 x 8 (y, z) columns, marched along x
constexpr int RT_TILE2[3] = {32, 64, 1};  // 2-D: lanes = the tile's 64 rows (48.5 KiB of LDS, under the 64 KiB of a static allocation)

PION_RT_HD int rt_k_to_i(const int v, const int side, const int k) { return side ? v + k : v - 1 - k; }

inline RtPlan rt_plan_of(const int ndim, const int ng[3], const RtSrc &s)
{
  RtPlan p;
  p.ndim = ndim;
  p.level_lo = p.level_hi = p.tlevel_lo = p.tlevel_hi = 0;
  for (int a = 0; a < 3; a++) {
    p.tile[a] = (ndim == 3) ? RT_TILE3[a] : RT_TILE2[a];
    p.v[a] = 0;
    p.klo[a][0] = 0; p.khi[a][0] = -1;   // unused axis: the one cell sits above vertex 0
    p.klo[a][1] = 0; p.khi[a][1] = 0;
    if (a >= ndim) continue;
    const int v = s.ipos[a] / 2;   // (even, so exact for negative positions too)
    p.v[a] = v;
    p.klo[a][0] = (v - ng[a] > 0) ? v - ng[a] : 0;
    p.khi[a][0] = v - 1;
    p.klo[a][1] = (-v > 0) ? -v : 0;
    p.khi[a][1] = ng[a] - 1 - v;
    int lo = -1, hi = -1;
    for (int sd = 0; sd < 2; sd++) {
      if (p.khi[a][sd] < p.klo[a][sd]) continue;
      if (lo < 0 || p.klo[a][sd] < lo) lo = p.klo[a][sd];
      if (p.khi[a][sd] > hi) hi = p.khi[a][sd];
    }
    p.level_lo += lo;
    p.level_hi += hi;
    p.tlevel_lo += lo / p.tile[a];
    p.tlevel_hi += hi / p.tile[a];
  }
  return p;
}

}  // namespace pion
#endif
