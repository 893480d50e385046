// dev_project.h -- the rules of the projected images (pion_gpu_project, pion_host_sim_write_projection), each stated
// once: the value a field has at a cell, which cells a pixel sums and in what order, and for a cylindrical (z,R) grid
// the reference's perpendicular Abel integral (analysis/projection/perp_projection.cpp: calc_projection_column,
// :404-487, with the slopes of the second loop of get_emission_absorption_data, :338-390, and the pixel list of
// :225-252).  Plain __host__ __device__ functions of GridDesc and OutputCfg, written the way dev_output.h is: the
// kernels of pion_project.hip run them on the device, the host writer (pion_amd/host/projection_io.cpp) runs the same
// functions in a host loop for a backend without the projection entries.  The includer provides __host__ /
// __device__, as for dev_output.h.
//
// Every function that does arithmetic is compiled without FMA contraction, in both builds and on the host (the pragma
// below for clang; the host library and pion_project.hip are built with -ffp-contract=off as well): images are
// compared with == against a restatement, and an image must not depend on which build or which route made it.  The
// only operations whose result may differ between the device and the host are log and exp (the device's and the
// host's math libraries); sqrt is correctly rounded on both.
//
// ---- the field.  f = coef rho^a T^b w, evaluated left to right as
//        f = coef;  a >= 1: f = f * rho;  a == 2: f = f * rho;  b != 0: f = f * exp(b * log(T));  var >= 0: f = f * P[var]
//      with T = p Mu_tot_over_kB / rho, dev_output.h's OUT_TEMP (mp_only_cooling.cpp:274-280).
//
// ---- 3-D Cartesian, line of sight along axis x, y or z.  pixel = (sum of f over the on-grid cells of the column) * dx:
//      one multiplication by dx, after the sum.  The image axes are the two remaining axes in grid order, element
//      [j][i] with i on the lower-numbered one.  The order of the additions:
//        along y, z:  s = 0.0; for k = 0 .. n-1 (increasing index): s = s + f_k.
//        along x:     PROJ_LANES = 64 partial sums, p_l = 0.0; for ix = l, l + 64, l + 128, .. < nx (increasing):
//                     p_l = p_l + f_ix (a lane without cells keeps 0.0); then the tree
//                     for h = 32, 16, 8, 4, 2, 1:  for l = 0 .. h-1:  p_l = p_l + p_(l+h);    s = p_0.
//      Neither depends on launch geometry, chunking or plane windows: a pixel is summed by one lane (y, z) or one
//      wavefront (x) from the state array itself.
//
// ---- 2-D cylindrical (z,R), line of sight perpendicular to the symmetry axis: see "the Abel integral" below.
#ifndef PION_DEV_PROJECT_H
#define PION_DEV_PROJECT_H

#include <cmath>

#include "../../include/pion_gpu.h"
#include "dev_output.h"
#include "grid_desc.h"

namespace pion {

#define PION_PRJ_HD __host__ __device__ inline

constexpr int PROJ_LANES = 64;

// the fields of one call, as the kernels take them
struct ProjFields {
  int n;
  pion_gpu_proj_field f[PION_PROJ_MAX_FIELDS];
};

// ---- what is refused: null, or the text of the refusal
inline const char *proj_refused_grid(const GridDesc &g, const int axis)
{
  if (g.cyl == 2) return "project: spherical grids have no projection";
  if (g.ndim == 1) return "project: 1-D grids have no projection";
  if (g.cyl == 1) {
    if (axis == 0) return "project: a line of sight along the symmetry axis of a cylindrical grid is not supported";
    if (axis != PION_PROJ_AXIS_PERP) return "project: a cylindrical grid takes axis PION_PROJ_AXIS_PERP only";
    if (g.ng[1] == 1) return "project: the Abel integral needs at least two rows in R (NR == 1)";
    return nullptr;
  }
  if (g.ndim == 2) return "project: 2-D Cartesian grids have no projection";
  if (axis < 0 || axis > 2) return "project: a 3-D Cartesian grid takes axis 0, 1 or 2";
  return nullptr;
}
inline const char *proj_refused_fields(const OutputCfg &o, const int nfields, const pion_gpu_proj_field *fields)
{
  if (nfields < 1 || nfields > PION_PROJ_MAX_FIELDS) return "project: between 1 and 8 fields per call";
  if (!fields) return "project: no fields";
  for (int i = 0; i < nfields; i++) {
    const pion_gpu_proj_field &f = fields[i];
    int len = 0;
    while (len < 16 && f.name[len]) len++;
    if (len == 0 || len == 16) return "project: a field's name has 1 to 15 characters and ends with NUL";
    for (int k = 0; k < len; k++)
      if (f.name[k] < 32 || f.name[k] > 126 || f.name[k] == '\'') return "project: a field's name is printable ASCII without quotes";
    if (f.a < 0 || f.a > 2) return "project: a field's power of rho is 0, 1 or 2";
    if (f.var >= o.nvar) return "project: a field's variable is not a variable of the state";
    if (!(std::fabs(f.coef) <= 1.7976931348623157e308) || !(std::fabs(f.b) <= 1.7976931348623157e308))
      return "project: a field's coef and b are finite";
    if (f.b != 0.0 && o.cooling == 0) return "project: b != 0 needs a temperature, and this handle has cooling == 0";
  }
  return nullptr;
}

// ---- the value of field f at cell c (all-cell id) of the state array S ([nvar][ncell])
PION_PRJ_HD double proj_value(const GridDesc &g, const OutputCfg &o, const pion_gpu_proj_field &f, const double *S, const long c)
{
#ifdef __clang__
#pragma clang fp contract(off)
#endif
  double v = f.coef;
  if (f.a >= 1) v = v * S[(long)OUT_RO * g.ncell + c];
  if (f.a == 2) v = v * S[(long)OUT_RO * g.ncell + c];
  if (f.b != 0.0) {
    OutImage temp;
    temp.kind = OUT_TEMP, temp.var = 0;
    v = v * exp(f.b * log(out_value(g, o, temp, S, c, 0)));
  }
  if (f.var >= 0) v = v * S[(long)f.var * g.ncell + c];
  return v;
}

// ---- the image: NI x NJ pixels; pixel (i, j) reads the cells c0 + i * si + j * sj + k * ss, k = 0 .. nsum-1.
// Cylindrical: i = z, j = R (the impact parameter's row), k = the rows of the column (nsum = NR)
struct ProjGeom {
  int ni, nj, nsum;
  long c0, si, sj, ss;
};
PION_PRJ_HD ProjGeom proj_geom(const GridDesc &g, const int axis)
{
  ProjGeom q;
  const long st[3] = {1, g.sy, g.sz};
  q.c0 = g.nbc[0] + g.sy * g.nbc[1] + g.sz * g.nbc[2];
  if (g.cyl == 1) {
    q.ni = g.ng[0], q.nj = g.ng[1], q.nsum = g.ng[1];
    q.si = 1, q.sj = 0, q.ss = g.sy;
    return q;
  }
  const int ai = (axis == 0) ? 1 : 0, aj = (axis == 2) ? 1 : 2;
  q.ni = g.ng[ai], q.nj = g.ng[aj], q.nsum = g.ng[axis];
  q.si = st[ai], q.sj = st[aj], q.ss = st[axis];
  return q;
}
PION_PRJ_HD long proj_count(const ProjGeom &q, const int nfields) { return (long)nfields * q.nj * q.ni; }

// ---- the two additions and the last multiplication of a column sum
PION_PRJ_HD double proj_add(const double s, const double f)
{
#ifdef __clang__
#pragma clang fp contract(off)
#endif
  return s + f;
}
PION_PRJ_HD double proj_times_dx(const GridDesc &g, const double s)
{
#ifdef __clang__
#pragma clang fp contract(off)
#endif
  return s * g.dx;
}
// a whole pixel in the rule's order, for the host loop; `first` is the pixel's first cell.  The kernels take the same
// steps with a lane per pixel (y, z) and a lane per partial sum (x)
inline double proj_column(const GridDesc &g, const OutputCfg &o, const pion_gpu_proj_field &f, const ProjGeom &q,
                          const int axis, const double *S, const long first)
{
  if (axis != 0) {
    double s = 0.0;
    for (int k = 0; k < q.nsum; k++) s = proj_add(s, proj_value(g, o, f, S, first + k * q.ss));
    return proj_times_dx(g, s);
  }
  double p[PROJ_LANES];
  for (int l = 0; l < PROJ_LANES; l++) {
    p[l] = 0.0;
    for (int ix = l; ix < q.nsum; ix += PROJ_LANES) p[l] = proj_add(p[l], proj_value(g, o, f, S, first + ix));
  }
  for (int h = PROJ_LANES / 2; h >= 1; h /= 2)
    for (int l = 0; l < h; l++) p[l] = proj_add(p[l], p[l + h]);
  return proj_times_dx(g, p[0]);
}

// ---- the Abel integral: calc_projection_column (perp_projection.cpp:404-487) as written.
//   r[ir]     the cell-centre radius of row ir (raw_data[DATA_R], :178: the library's own cell centre,
//             cell_interface.cpp:506-512, as dev_output.h's divergence spells it)
//   v[ir]     the field at the cell (ems[..][ir]);  s[ir] = (v[ir+1] - v[ir]) / (r[ir+1] - r[ir]) for ir < Nr-1 (:345-347),
//             s[Nr-1] = s[Nr-2] (:368-370)
//   dr        the cell diameter (delr, :115, :239): g.dx
//   b         the ray's impact parameter: one ray per row, b = r[j] (:230)
//   grid_max = r[Nr-1] + 0.5 dr (:416); b > grid_max gives 0 (:417-420; never for b = r[j]);
//   b < r[0]: b = r[0] * 1.00000001 (:426-429; never for b = r[j], kept as written)
//   ir = 0; while (r[ir] + dr < b) ir++ (:434-435)
//   per segment (:442-479), ir increasing up to Nr-1:
//     Rmin = max(b, r[ir]); Rmax = min(grid_max, r[ir] + dr);   (segments run from one cell centre to the next)
//     maxd = sqrt(Rmax Rmax - b b); mind = sqrt(Rmin Rmin - b b);
//     offset = v[ir] - s[ir] Rmin;
//     xdx = maxd - mind;  x2dx = 0.5 (Rmax maxd - Rmin mind + b b log((Rmax + maxd) / (Rmin + mind)));
//     result += s[ir] x2dx + offset xdx;
//   result *= 2 (:484).
// What depends only on (j, ir) -- Rmin, xdx, x2dx -- is AbelW: the same for every z of the row, so the kernel evaluates
// it once per (j, ir) and workgroup; these are the rule's own intermediate values, nothing is regrouped.
PION_PRJ_HD double abel_r(const GridDesc &g, const int ir)
{
#ifdef __clang__
#pragma clang fp contract(off)
#endif
  return g.xmin[1] + (2 * ir + 1) * (0.5 * g.dx);
}
PION_PRJ_HD double abel_grid_max(const GridDesc &g, const int nr)
{
#ifdef __clang__
#pragma clang fp contract(off)
#endif
  return abel_r(g, nr - 1) + 0.5 * g.dx;
}
// the impact parameter of row j, after the reset of :426-429
PION_PRJ_HD double abel_b(const GridDesc &g, const int j)
{
#ifdef __clang__
#pragma clang fp contract(off)
#endif
  double b = abel_r(g, j);
  if (b < abel_r(g, 0)) b = abel_r(g, 0) * 1.00000001;
  return b;
}
// the first segment of row j: the ir the loop `ir = 0; while (r[ir] + dr < b) ir++` stops at.  r[ir] + dr is
// non-decreasing in ir, so the condition holds for every ir below the first one it fails for, and the walk may start
// anywhere: from j - 3, downwards while the row below fails too, then upwards as the reference does.  ir < nr bounds a
// walk the reference leaves unbounded (it stops at nr - 1 at the latest, since b <= r[nr-1])
PION_PRJ_HD int abel_start(const GridDesc &g, const int nr, const int j)
{
#ifdef __clang__
#pragma clang fp contract(off)
#endif
  const double b = abel_b(g, j), dr = g.dx;
  int ir = (j > 3) ? j - 3 : 0;
  while (ir > 0 && !(abel_r(g, ir - 1) + dr < b)) ir--;
  while (ir < nr - 1 && (abel_r(g, ir) + dr) < b) ir++;
  return ir;
}
struct AbelW {
  double Rmin, xdx, x2dx;
};
PION_PRJ_HD AbelW abel_weights(const GridDesc &g, const int nr, const int j, const int ir)
{
#ifdef __clang__
#pragma clang fp contract(off)
#endif
  const double b = abel_b(g, j), dr = g.dx, grid_max = abel_grid_max(g, nr);
  const double rir = abel_r(g, ir);
  AbelW w;
  w.Rmin = (b > rir) ? b : rir;                                       // std::max(b, r[ir])
  const double Rmax = (grid_max < rir + dr) ? grid_max : rir + dr;    // std::min(grid_max, r[ir] + dr)
  const double Rmax2 = Rmax * Rmax, Rmin2 = w.Rmin * w.Rmin;
  const double maxd = sqrt(Rmax2 - b * b), mind = sqrt(Rmin2 - b * b);
  w.xdx = maxd - mind;
  w.x2dx = 0.5 * (Rmax * maxd - w.Rmin * mind + b * b * log((Rmax + maxd) / (w.Rmin + mind)));
  return w;
}
// s[m] for m < nr - 1, from the values of rows m and m + 1; row nr - 1 takes s[nr - 2]
PION_PRJ_HD double abel_slope(const GridDesc &g, const int m, const double v_m, const double v_m1)
{
#ifdef __clang__
#pragma clang fp contract(off)
#endif
  const double dr = abel_r(g, m + 1) - abel_r(g, m);
  return (v_m1 - v_m) / dr;
}
// one segment added to the result
PION_PRJ_HD double abel_add(const double result, const double v, const double s, const AbelW &w)
{
#ifdef __clang__
#pragma clang fp contract(off)
#endif
  const double offset = v - s * w.Rmin;
  const double seg = s * w.x2dx + offset * w.xdx;
  return result + seg;
}
PION_PRJ_HD double abel_finish(const double result)
{
#ifdef __clang__
#pragma clang fp contract(off)
#endif
  return result * 2.0;
}
// a whole pixel, for the host loop: row j (impact parameter), column whose row-0 cell is `first`
inline double abel_column(const GridDesc &g, const OutputCfg &o, const pion_gpu_proj_field &f, const ProjGeom &q,
                          const double *S, const long first, const int j)
{
  const int nr = q.nsum;
  if (abel_b(g, j) > abel_grid_max(g, nr)) return 0.0;
  double result = 0.0;
  for (int ir = abel_start(g, nr, j); ir < nr; ir++) {
    const int m = (ir < nr - 1) ? ir : nr - 2;
    const double s = abel_slope(g, m, proj_value(g, o, f, S, first + m * q.ss), proj_value(g, o, f, S, first + (m + 1) * q.ss));
    result = abel_add(result, proj_value(g, o, f, S, first + ir * q.ss), s, abel_weights(g, nr, j, ir));
  }
  return abel_finish(result);
}

// ---- parts: the image of a slab-decomposed run, the sums carried from rank to rank.  A rank holds the planes
// [plane_lo, plane_lo + n) of the slab axis (z in 3-D, y/R in 2-D; n = g.ng of that axis) out of global_planes.  It
// works into an image of the WHOLE domain that it receives from the rank below (rank 0: +0.0 everywhere) and hands to
// the rank above; after the last rank (`last`) the image is == the one a single grid of the whole domain gives.
//   3-D along z:      every pixel's running sum s is continued over the rank's planes in increasing index -- proj_add,
//                     entered with the s of the rank below; only the last rank applies proj_times_dx.
//   3-D along x, y:   a pixel lies wholly in one rank: the rank finishes its own image rows as proj_column does and
//                     writes them at row offset plane_lo of the whole image; the other rows stay as received.
//   cylindrical:      for every impact row j of the WHOLE grid below the rank's upper edge (j < plane_lo + n) the rank
//                     adds the segments ir of its own rows with ir >= abel_start(j), in increasing ir, into the running
//                     result[j] -- abel_add, unchanged.  abel_r, abel_b, abel_grid_max, abel_start, abel_weights and
//                     abel_slope take GLOBAL row indices and the whole grid's R origin and NR (proj_part_grid); the
//                     slope of the rank's last own row reads v of the next rank's first row from the first upper slab
//                     ghost row (the halo exchange has filled it); the global last row takes the slope of the row before
//                     it; only the last rank applies abel_finish and the b > grid_max zero.
//                     Nothing else outside the on-grid cells is read: no x ghost, no lower slab ghost.
// A part with plane_lo = 0, global_planes = n, last = 1 on an image of +0.0 takes exactly the steps of proj_column /
// abel_column.
struct ProjPart {
  int plane_lo, global_planes, last;
  double global_xmin;
};
inline const char *proj_refused_part(const GridDesc &g, const pion_gpu_proj_part *part)
{
  if (!part) return "project: no part";
  const int n = g.ng[g.ndim - 1];
  if (part->plane_lo < 0) return "project: a part's plane_lo is not negative";
  if ((long)part->plane_lo + n > (long)part->global_planes) return "project: a part's planes end above global_planes";
  if (!(std::fabs(part->global_xmin) <= 1.7976931348623157e308)) return "project: a part's global_xmin is finite";
  return nullptr;
}
// the grid the Abel geometry functions are evaluated with: the whole grid's R origin (its NR is part.global_planes)
PION_PRJ_HD GridDesc proj_part_grid(const GridDesc &g, const ProjPart &part)
{
  GridDesc gg = g;
  if (g.cyl == 1) gg.xmin[1] = part.global_xmin;
  return gg;
}
// the image of the whole domain: geometry of the rank's own cells, image rows of the whole grid
PION_PRJ_HD bool proj_part_along_slab(const GridDesc &g, const int axis) { return g.cyl != 1 && axis == g.ndim - 1; }
PION_PRJ_HD int proj_part_nj(const GridDesc &g, const ProjGeom &q, const int axis, const ProjPart &part)
{
  return proj_part_along_slab(g, axis) ? q.nj : part.global_planes;
}
PION_PRJ_HD long proj_part_count(const GridDesc &g, const ProjGeom &q, const int axis, const ProjPart &part, const int nfields)
{
  return (long)nfields * proj_part_nj(g, q, axis, part) * q.ni;
}
// 3-D along the slab axis: the pixel's sum continued from `carried`
inline double proj_column_part(const GridDesc &g, const OutputCfg &o, const pion_gpu_proj_field &f, const ProjGeom &q,
                               const ProjPart &part, const double *S, const long first, const double carried)
{
  double s = carried;
  for (int k = 0; k < q.nsum; k++) s = proj_add(s, proj_value(g, o, f, S, first + k * q.ss));
  return part.last ? proj_times_dx(g, s) : s;
}
// cylindrical: impact row j of the whole grid (j < plane_lo + n), column whose local row-0 cell is `first`; gg =
// proj_part_grid(g, part)
inline double abel_column_part(const GridDesc &g, const GridDesc &gg, const OutputCfg &o, const pion_gpu_proj_field &f,
                               const ProjGeom &q, const ProjPart &part, const double *S, const long first, const int j,
                               const double carried)
{
  const int nr = part.global_planes, lo = part.plane_lo, hi = part.plane_lo + q.nsum;
  double result = carried;
  const int ir0 = abel_start(gg, nr, j);
  for (int ir = (ir0 > lo) ? ir0 : lo; ir < hi; ir++) {
    const int m = (ir < nr - 1) ? ir : nr - 2;
    const double s = abel_slope(gg, m, proj_value(g, o, f, S, first + (long)(m - lo) * q.ss),
                                proj_value(g, o, f, S, first + (long)(m + 1 - lo) * q.ss));
    result = abel_add(result, proj_value(g, o, f, S, first + (long)(ir - lo) * q.ss), s, abel_weights(gg, nr, j, ir));
  }
  if (!part.last) return result;
  return (abel_b(gg, j) > abel_grid_max(gg, nr)) ? 0.0 : abel_finish(result);
}

}  // namespace pion
#endif
