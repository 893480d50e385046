// dev_project_angle.h -- the rule of the inclined projection of a cylindrical (z,R) grid (pion_gpu_project_angle,
// pion_host_sim_write_projection_angle), stated once: the image an observer sees whose line of sight makes the angle
// theta, 0 < theta < 90 degrees, with the symmetry axis.  It is the reference's analysis/projection/angle_projection.cpp
// (the second half of project2D) as written: pixel_centre (:41-54), get_Z_from_R / get_R_from_Z (:64-100),
// get_start_of_ray (:115-171), get_entry_exit_points (:184-336) and the three parts of generate_angle_image (:466-665),
// with equalD of constants.cpp:48-69 and the constants of constants.h:150-157.  Only the angle < pi/2 branches are
// stated: no other angle is admitted.  Plain __host__ __device__ functions written the way dev_project.h is: the kernel
// of pion_project.hip runs angle_pixel with a lane per pixel, the host writer (pion_amd/host/projection_io.cpp) runs the
// same function in a host loop.  Nothing is contracted (the pragma in every function; both builds and the host library
// are compiled -ffp-contract=off as well); sqrt and the divisions are IEEE on both sides, and there is no log, exp or
// trigonometric function on the device: the images of the two routes are equal bit for bit once the field values are.
//
// ---- the angle.  angle = angle_deg * M_PI / 180.0 (project2D.cpp:148).  tan(angle), 1.0 / sin(angle) and sin(angle)
//      are evaluated ONCE, on the host, in double (angle_numbers) and handed to the kernel and to the host loop as
//      numbers.
// ---- the pixels.  n_extra = (int) fabs(Xmax[R] / tan(angle) / dx) (project2D.cpp:319); NI = NZ + 2 n_extra, NJ = NR;
//      image [NR][NI], z fastest (:675).  The centre of pixel (i, j) (:41-54):
//        pos_z = (Xmin[Z] - n_extra * dx) + (i + 0.5) * dx,   pos_R = Xmin[R] + (j + 0.5) * dx.
//      Cell centres are xmin + (2 k + 1) * (0.5 * dx), as dev_output.h and the Abel path spell them.
// ---- the ray of a pixel is the hyperbola R(z)^2 = pos_R^2 + (z - pos_z)^2 tan^2: it comes in from z = +infinity
//      (inout = 1), turns at the pixel centre (inout = 0) and leaves towards z = -infinity (inout = -1).
//        R_from_Z(z)    = sqrt(pos_R * pos_R + (z - pos_z) * (z - pos_z) * tan * tan)               (:98-99)
//        Z_from_R(R,io) = pos_z + io * sqrt(R * R - pos_R * pos_R) / tan                            (:76)
//      start of the ray (:115-171): r_ini = Xmax[R], z_ini = Z_from_R(r_ini, 1); z_ini > Xmax[Z]: z_ini = Xmax[Z], r_ini =
//      R_from_Z(z_ini); else z_ini < Xmin[Z]: z_ini = Xmin[Z], r_ini = R_from_Z(z_ini).  The cell: from row 0 upwards while
//      (centre_R + 0.5 dx < r_ini and a row above exists), then from column 0 upwards while (centre_z + 0.5 dx < z_ini
//      and a column above exists) -- angle_search gives the index those loops stop at.
//      a cell of the ray (:184-336): angle_cell below, line by line.
//      the pixel (:466-665): angle_pixel below.  Per cell crossed, ans[f] = ans[f] + weight * V[f][cell] in ray order, all
//      fields in ONE walk; weight = invst * fabs(sqrt(en_R^2 - pos_R^2) - sqrt(ex_R^2 - pos_R^2)), for the turning cell
//      invst * 2.0 * sqrt(en_R^2 - pos_R^2) (:532-534, :584-585, :650-652).  V[f][ir][iz] is dev_project.h's proj_value of
//      field f at the cell, evaluated once per cell before the walk.  The square roots are left unclamped, as written.
//
// ---- where this departs from the reference, both so that no walk can fail to end:
//   1. the turning-point cell an on-grid pixel's incoming ray stops at (:480-489) is the cell (i - n_extra, j) whenever
//      Xmin[Z] < pos_z < Xmax[Z]: what the reference's two equalD searches find when they return (they walk off the grid
//      when no cell centre matches).
//   2. every walk is bounded: a cell outside the grid [0, NZ) x [0, NR) is "missing" (the reference's null, boundary or
//      off-grid cell), and a ray whose next cell is missing ends there -- also an on-grid pixel's incoming ray, which
//      the reference would follow through a null pointer; such a pixel then has no turning cell and no outgoing ray.
//      Each of the two ray loops runs at most `trip_limit` trips (the rule's own: angle_trip_limit = 2 (NZ + NR) + 8);
//      a pixel whose loop reaches the limit before its end condition stops there and is reported as capped.
// ---- a property of the reference that is kept: an incoming ray starts only for pos_z < Xmax[Z] - dx and an outgoing
//      one only for pos_z > Xmin[Z] + dx, so above 60 degrees (1 / cos > 2) the two end columns in z lose part of their
//      rays.
#ifndef PION_DEV_PROJECT_ANGLE_H
#define PION_DEV_PROJECT_ANGLE_H

#include <cmath>

#include "dev_project.h"

namespace pion {

struct AngleGeom {
  int nz, nr, n_extra, ni;          // ni = nz + 2 n_extra
  double tn, invst;                 // tan(angle), 1.0 / sin(angle): host values
  double dx, zmin, zmax, rmin, rmax;
};

// ---- host only: the three numbers of the angle, and what is refused
inline void angle_numbers(const double angle_deg, double *tn, double *invst, double *st)
{
  const double angle = angle_deg * M_PI / 180.0;   // project2D.cpp:148
  *tn = std::tan(angle);
  *st = std::sin(angle);
  *invst = 1.0 / std::sin(angle);                  // angle_projection.cpp:445
}
// null and the geometry in q, or the text of the refusal
inline const char *angle_refused(const GridDesc &g, const pion_gpu_config &c, const double angle_deg, const int nfields, AngleGeom *q)
{
#ifdef __clang__
#pragma clang fp contract(off)
#endif
  if (g.cyl != 1 || g.ndim != 2) return "project_angle: only a 2-D cylindrical (z,R) grid has an inclined projection";
  if (g.ng[1] == 1) return "project_angle: the rays need at least two rows in R (NR == 1)";
  for (int d = 0; d < 4; d++)
    if (c.bc_type[d] == PION_BC_SLAB)
      return "project_angle: this grid has a PION_BC_SLAB face, it is one rank of a slab run, and rays are not carried from rank to rank";
  if (angle_deg == 90.0) return "project_angle: 90 degrees is the perpendicular line of sight: use PION_PROJ_AXIS_PERP";
  if (!(angle_deg > 0.0 && angle_deg < 90.0)) return "project_angle: the angle is finite, above 0 and below 90 degrees";
  if (nfields < 1 || nfields > PION_PROJ_MAX_FIELDS) return "project: between 1 and 8 fields per call";
  double st;
  angle_numbers(angle_deg, &q->tn, &q->invst, &st);
  q->nz = g.ng[0], q->nr = g.ng[1], q->dx = g.dx;
  q->zmin = g.xmin[0], q->rmin = g.xmin[1];
  q->zmax = g.xmin[0] + g.ng[0] * g.dx, q->rmax = g.xmin[1] + g.ng[1] * g.dx;
  const double extra = std::fabs(q->rmax / q->tn / q->dx);   // project2D.cpp:319
  const char *many = "project_angle: nfields * NR * NI exceeds 2^31 - 1 (a small angle adds Xmax[R] / tan(angle) / dx columns at each end)";
  if (!(extra < 1073741824.0)) return many;
  q->n_extra = (int)extra;
  const long ni = (long)q->nz + 2L * q->n_extra;
  if ((long)nfields * q->nr * ni > 2147483647L) return many;
  q->ni = (int)ni;
  return nullptr;
}
PION_PRJ_HD long angle_count(const AngleGeom &q, const int nfields) { return (long)nfields * q.nr * q.ni; }
PION_PRJ_HD int angle_trip_limit(const AngleGeom &q) { return 2 * (q.nz + q.nr) + 8; }

// ---- constants.cpp:48-69 with TINYVALUE 1.0e-100, SMALLVALUE 1.0e-12 (constants.h:150-152)
PION_PRJ_HD bool angle_equalD(const double a, const double b)
{
#ifdef __clang__
#pragma clang fp contract(off)
#endif
  if (a == b) return true;
  if (fabs(a) + fabs(b) < 1.0e-100) return true;
  return (fabs(a - b) / (fabs(a) + fabs(b) + 1.0e-100)) < 1.0e-12;
}
PION_PRJ_HD double angle_cell_z(const AngleGeom &q, const int iz)
{
#ifdef __clang__
#pragma clang fp contract(off)
#endif
  return q.zmin + (2 * iz + 1) * (0.5 * q.dx);
}
PION_PRJ_HD double angle_cell_r(const AngleGeom &q, const int ir)
{
#ifdef __clang__
#pragma clang fp contract(off)
#endif
  return q.rmin + (2 * ir + 1) * (0.5 * q.dx);
}
// pixel_centre, :41-54
PION_PRJ_HD double angle_pos_z(const AngleGeom &q, const long i)
{
#ifdef __clang__
#pragma clang fp contract(off)
#endif
  const double zmin = q.zmin - q.n_extra * q.dx;
  return zmin + (i + 0.5) * q.dx;
}
PION_PRJ_HD double angle_pos_r(const AngleGeom &q, const int j)
{
#ifdef __clang__
#pragma clang fp contract(off)
#endif
  return q.rmin + (j + 0.5) * q.dx;
}
// get_Z_from_R (:76) and get_R_from_Z (:98-99); io = +1.0 or -1.0
PION_PRJ_HD double angle_Z_from_R(const AngleGeom &q, const double pz, const double pr, const double R, const double io)
{
#ifdef __clang__
#pragma clang fp contract(off)
#endif
  return pz + io * sqrt(R * R - pr * pr) / q.tn;
}
PION_PRJ_HD double angle_R_from_Z(const AngleGeom &q, const double pz, const double pr, const double Z)
{
#ifdef __clang__
#pragma clang fp contract(off)
#endif
  return sqrt(pr * pr + (Z - pz) * (Z - pz) * q.tn * q.tn);
}
// the index the loop `k = 0; while (centre(k) + 0.5 dx < x && k + 1 < n) k++` stops at (:151-159).  centre(k) + 0.5 dx does
// not decrease with k, so the condition holds for every k below the first one it fails for and the walk may start
// anywhere: from an estimate, downwards while the index below fails too, then upwards as the reference does.  Either
// walk makes at most n trips
PION_PRJ_HD int angle_search(const double x0, const double dx, const int n, const double x)
{
#ifdef __clang__
#pragma clang fp contract(off)
#endif
  const double t = (x - x0) / dx - 1.0;
  int k = 0;
  if (t >= (double)(n - 1)) k = n - 1;
  else if (t > 0.0) k = (int)t;
  while (k > 0 && !((x0 + (2 * (k - 1) + 1) * (0.5 * dx)) + 0.5 * dx < x)) k--;
  while (k + 1 < n && (x0 + (2 * k + 1) * (0.5 * dx)) + 0.5 * dx < x) k++;
  return k;
}
// get_start_of_ray, :115-171
PION_PRJ_HD void angle_start(const AngleGeom &q, const double pz, const double pr, int *iz, int *ir)
{
#ifdef __clang__
#pragma clang fp contract(off)
#endif
  double r_ini = q.rmax;                                        // :128
  double z_ini = angle_Z_from_R(q, pz, pr, r_ini, 1.0);         // :129
  if (z_ini > q.zmax) {                                         // :132-138
    z_ini = q.zmax;
    r_ini = angle_R_from_Z(q, pz, pr, z_ini);
  }
  else if (z_ini < q.zmin) {                                    // :139-145
    z_ini = q.zmin;
    r_ini = angle_R_from_Z(q, pz, pr, z_ini);
  }
  *ir = angle_search(q.rmin, q.dx, q.nr, r_ini);                // :152-155
  *iz = angle_search(q.zmin, q.dx, q.nz, z_ini);                // :156-159
}

// get_entry_exit_points, :184-336, for the cell (iz, ir) of the ray of the pixel at (pz, pr); inout 1, 0, -1.
// Out: the R of the entry and exit points, and the next cell (niz, nir) with ok = it is on the grid.  The z of the
// entry point is never read by the caller or by this function and is not evaluated; the z of the exit point is.
struct AngleCell {
  double en_r, ex_r;
  int niz, nir;
  bool ok;
};
PION_PRJ_HD AngleCell angle_cell(const AngleGeom &q, const double pz, const double pr, const int inout, const int iz, const int ir)
{
#ifdef __clang__
#pragma clang fp contract(off)
#endif
  AngleCell a;
  const double cz = angle_cell_z(q, iz), cr = angle_cell_r(q, ir);   // :195-196
  const double dxo2 = 0.5 * q.dx, dx = q.dx;                           // :197-198
  bool flag = false;
  int dir_flag = inout;
  const double en_z = cz + dxo2;                                       // :208-211
  double ex_z = cz - dxo2;
  a.en_r = angle_R_from_Z(q, pz, pr, en_z);                            // :218-219
  a.ex_r = angle_R_from_Z(q, pz, pr, ex_z);
  if (angle_equalD(a.ex_r, a.en_r) && angle_equalD(pz, cz)) {          // :221-227
    if (!angle_equalD(pr, cr)) flag = true;
  }
  const double midpt = angle_R_from_Z(q, pz, pr, cz);                  // :232
  const double mn = (cr - dxo2) * (1.0 - 1.0e-12);                     // :236-237
  const double mx = (cr + dxo2) * (1.0 + 1.0e-12);
  if ((a.en_r < mn && a.ex_r < mn && midpt < mn) || (a.en_r > mx && a.ex_r > mx && midpt > mx)) {   // :242-251
    a.ok = false, a.niz = iz, a.nir = ir;
    a.en_r = 1.0e99, a.ex_r = 1.0e99;
    return a;
  }
  if (a.en_r < cr - dxo2) {                                            // :257-262
    a.en_r = cr - dxo2;
    if (inout == 0) dir_flag = 1;
  }
  else if (a.en_r > cr + dxo2) {                                       // :263-268
    a.en_r = cr + dxo2;
    if (inout == 0) dir_flag = 1;
  }
  if (a.ex_r < cr - dxo2) {                                            // :274-279
    a.ex_r = cr - dxo2;
    if (inout == 0) dir_flag = -1;
    ex_z = angle_Z_from_R(q, pz, pr, a.ex_r, (double)dir_flag);
  }
  else if (a.ex_r > cr + dxo2) {                                       // :280-285
    a.ex_r = cr + dxo2;
    if (inout == 0) dir_flag = -1;
    ex_z = angle_Z_from_R(q, pz, pr, a.ex_r, (double)dir_flag);
  }
  a.niz = iz, a.nir = ir;                                              // :293
  if (fabs(a.ex_r - (cr + dxo2)) / dx < 1.0e-8 && dir_flag == -1) a.nir = ir + 1;        // :297-300
  else if (fabs(a.ex_r - (cr - dxo2)) / dx < 1.0e-8 && dir_flag == 1) a.nir = ir - 1;    // :301-304
  if (fabs(ex_z - (cz - dxo2)) / dx < 1.0e-8) a.niz = iz - 1;                            // :310-313 (angle < pi/2)
  if (flag) {                                                          // :318-332
    if (inout == 1) {
      a.ex_r = cr - dxo2;
      a.niz = iz, a.nir = ir - 1;
    }
    else if (inout == -1) {
      a.en_r = cr - dxo2;
      if (angle_equalD(a.ex_r, cr + dxo2)) a.niz = iz, a.nir = ir + 1;
    }
  }
  a.ok = a.niz >= 0 && a.niz < q.nz && a.nir >= 0 && a.nir < q.nr;     // :334, and departure 2
  return a;
}
// :532-534 / :650-652, and the turning cell's :584-585
PION_PRJ_HD double angle_weight(const AngleGeom &q, const double pr, const AngleCell &a)
{
#ifdef __clang__
#pragma clang fp contract(off)
#endif
  return q.invst * fabs(sqrt(a.en_r * a.en_r - pr * pr) - sqrt(a.ex_r * a.ex_r - pr * pr));
}
PION_PRJ_HD double angle_weight_turn(const AngleGeom &q, const double pr, const AngleCell &a)
{
#ifdef __clang__
#pragma clang fp contract(off)
#endif
  return q.invst * 2.0 * sqrt(a.en_r * a.en_r - pr * pr);
}
// add_cell_emission_to_ray's pattern (:372): every field of the cell, V = [nfields][NR][NZ]
PION_PRJ_HD void angle_add(const AngleGeom &q, const double *V, const int nfields, const int iz, const int ir, const double w,
                           double *ans)
{
#ifdef __clang__
#pragma clang fp contract(off)
#endif
  const long cell = (long)ir * q.nz + iz, ncells = (long)q.nr * q.nz;
#ifdef __clang__
#pragma unroll
#endif
  for (int f = 0; f < PION_PROJ_MAX_FIELDS; f++)
    if (f < nfields) ans[f] = ans[f] + w * V[f * ncells + cell];
}

// ---- one pixel: the body of generate_angle_image's loops, :456-681.  ans[PION_PROJ_MAX_FIELDS] receives the sums of
// the fields; returns 1 if one of the two ray loops reached trip_limit before its end condition (the pixel is capped
// and holds what had been added), else 0
PION_PRJ_HD int angle_pixel(const AngleGeom &q, const double *V, const int nfields, const long i, const int j, const int trip_limit,
                            double *ans)
{
#ifdef __clang__
#pragma clang fp contract(off)
#endif
  const double pz = angle_pos_z(q, i), pr = angle_pos_r(q, j);   // :458
#ifdef __clang__
#pragma unroll
#endif
  for (int f = 0; f < PION_PROJ_MAX_FIELDS; f++) ans[f] = 0.0;   // :495-496
  int iz, ir;
  angle_start(q, pz, pr, &iz, &ir);                              // :467
  bool have = true;                                              // `ray` is a cell
  const bool pix_on_grid = pz < q.zmax && pz > q.zmin;           // :482
  const int ciz = (int)(i - q.n_extra), cir = j;                 // departure 1: the cell c of :484-488

  if (pz < q.zmax - q.dx) {                                      // :503: an incoming ray
    AngleCell a = angle_cell(q, pz, pr, 1, iz, ir);              // :511
    if (!(a.en_r > 1.0e90)) {                                    // :513
      int trips = 0;
      for (;;) {                                                 // do { :520
        a = angle_cell(q, pz, pr, 1, iz, ir);                    // :524
        angle_add(q, V, nfields, iz, ir, angle_weight(q, pr, a), ans);   // :532-536
        iz = a.niz, ir = a.nir, have = a.ok;                     // :547
        trips++;
        bool at_source;
        if (pix_on_grid) at_source = !have || (iz == ciz && ir == cir);               // :549-552
        else at_source = !have || angle_equalD(angle_cell_z(q, iz), pz);              // :553-556
        if (at_source) break;                                    // } while (!at_source) :557
        if (trips >= trip_limit) return 1;
      }
    }
  }
  if (pix_on_grid && have) {                                     // :567: the turning-point cell
    const AngleCell a = angle_cell(q, pz, pr, 0, iz, ir);        // :579-582
    angle_add(q, V, nfields, iz, ir, angle_weight_turn(q, pr, a), ans);   // :584-587
    iz = a.niz, ir = a.nir, have = a.ok;                         // :588
  }
  if (pz > q.zmin + q.dx && have) {                              // :609: an outgoing ray
    AngleCell a = angle_cell(q, pz, pr, -1, iz, ir);             // :619
    if (!(a.en_r > 1.0e90)) {                                    // :621
      int trips = 0;
      for (;;) {                                                 // do { :633
        a = angle_cell(q, pz, pr, -1, iz, ir);                   // :640
        angle_add(q, V, nfields, iz, ir, angle_weight(q, pr, a), ans);   // :650-654
        iz = a.niz, ir = a.nir, have = a.ok;                     // :658
        trips++;
        if (!have) break;                                        // } while (ray != 0 && ray->isgd) :660
        if (trips >= trip_limit) return 1;
      }
    }
  }
  return 0;
}

}  // namespace pion
#endif
