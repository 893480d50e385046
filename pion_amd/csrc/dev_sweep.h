// dev_sweep.h -- helpers every floating-point kernel uses: the lab <-> sweep frame rotation (rotvar, to_sweep,
// from_sweep), the minmod average, the cylindrical and spherical radii, CellTimeStep (cell_dt) and the decode of an
// on-grid cell number; dev_addr.h comes in between them.
//
// Included by kernels_fp.hip, kernels_prepass.hip and kernels_dt.hip inside namespace pion::PION_FPNS, after
// dev_cooling.h and kernels.h.
#ifndef PION_DEV_SWEEP_H
#define PION_DEV_SWEEP_H

// SoA variable of sweep-frame slot s for a sweep along ax (run-time version of gvar<>)
template <bool MHD>
PDEV int rotvar(const int ax, const int s)
{
  if (s >= 2 && s <= 4) {
    int k = (s - 2) + ax;
    return 2 + (k >= 3 ? k - 3 : k);
  }
  if (MHD && s >= 5 && s <= 7) {
    int k = (s - 5) + ax;
    return 5 + (k >= 3 ? k - 3 : k);
  }
  return s;
}
template <int EQ, int NV>
PDEV void apply_axis(double *d, const double *q0, const double bnm, const double sim, const double bnp,
                     const double sip, const double *Fm, const double *Fp, const double dt, const double dx);
// BaseVectorOps::AvgFalle with AVG_MINMOD (coord_sys/VectorOps.cpp:37-59)
PDEV double avg_falle(const double a, const double b)
{
  if (a * b <= PION_VERY_TINY_VALUE) return 0.0;
#ifdef PION_FAST_MATH
  // a and b have the same sign here, so r = a/b > 0 and min(r,1)*b is a (if |a|<|b|) or b:
  // the fast build picks it without the division (differs from the reference form by <= 1 ulp)
  return (fabs(a) < fabs(b)) ? a : b;
#else
  double r = a / b;
  return (r > 0.0) ? dmin(r, 1.0) * b : 0.0;
#endif
}
// Cylindrical (z,R) grids: centre of a cell along R from its all-cell y index (cell_interface.cpp:506-512)
// and VectorOps_Cyl::R_com (coord_sys/VectorOps.h:414-418)
PDEV double cyl_R(const GridDesc &g, const int jy_all)
{
  return g.xmin[1] + (2 * (jy_all - g.nbc[1]) + 1) * (0.5 * g.dx);
}
PDEV double cyl_Rcom(const double R, const double dR) { return (R + dR * dR / 12. / R); }
// spherical symmetry (1-D): cell centre from the all-cell x index; R3 and R_com of VectorOps_Sph
// (coord_sys/VectorOps_spherical.h:172-196)
PDEV double sph_R(const GridDesc &g, const int ix_all)
{
  return g.xmin[0] + (2 * (ix_all - g.nbc[0]) + 1) * (0.5 * g.dx);
}
PDEV double sph_R3(const double R, const double dR) { return (R + dR * dR / 12.0 / R); }
PDEV double sph_Rcom(const double R, const double dR)
{
  double delta2 = dR / R;
  delta2 *= delta2;
  return R * (1.0 + 0.25 * delta2) / (1.0 + delta2 / 12.0);
}

// rotate the three vector components between the lab frame and the sweep frame
template <int NV, bool MHD>
PDEV void to_sweep(const int ax, const double *lab, double *sw)
{
#pragma unroll
  for (int v = 0; v < NV; v++) sw[v] = lab[v];
  if (ax == 1) {
    sw[2] = lab[3]; sw[3] = lab[4]; sw[4] = lab[2];
    if constexpr (MHD) { sw[5] = lab[6]; sw[6] = lab[7]; sw[7] = lab[5]; }
  }
  else if (ax == 2) {
    sw[2] = lab[4]; sw[3] = lab[2]; sw[4] = lab[3];
    if constexpr (MHD) { sw[5] = lab[7]; sw[6] = lab[5]; sw[7] = lab[6]; }
  }
}
template <int NV, bool MHD>
PDEV void from_sweep(const int ax, const double *sw, double *lab)
{
#pragma unroll
  for (int v = 0; v < NV; v++) lab[v] = sw[v];
  if (ax == 1) {
    lab[3] = sw[2]; lab[4] = sw[3]; lab[2] = sw[4];
    if constexpr (MHD) { lab[6] = sw[5]; lab[7] = sw[6]; lab[5] = sw[7]; }
  }
  else if (ax == 2) {
    lab[4] = sw[2]; lab[2] = sw[3]; lab[3] = sw[4];
    if constexpr (MHD) { lab[7] = sw[5]; lab[5] = sw[6]; lab[6] = sw[7]; }
  }
}

#include "dev_addr.h"

// CellTimeStep of a lab-frame state (solver_eqn_hydro_adi.cpp:460-502 / solver_eqn_mhd_adi.cpp:516-582);
// the same operations as k_dt, used by the stage kernel to leave the next step's dt behind.
template <int EQ>
PDEV double cell_dt(const double *P, const int ndim, const double g, const double dx, const double cfl)
{
  double p[8];
#pragma unroll
  for (int v = 0; v < 8; v++) p[v] = (EQ != EQEUL || v < 5) ? P[v] : 0.0;
  double temp;
  if constexpr (EQ == EQEUL) {
#ifdef PION_FAST_MATH
    // fast build: seeded root (of |v|^2 + 1e-200: a cell at rest would otherwise ask for the root of zero),
    // one reciprocal for dx / (|v| + c); multiply-adds written out (see below)
    temp = PION_VERY_TINY_VALUE;
    for (int v = 0; v < ndim; v++) temp = __builtin_fma(p[2 + v], p[2 + v], temp);
    temp = sqrt_pos(temp) + sqrt_pos((g * p[1]) * frcp(p[0]));
    return (dx * cfl) * frcp(temp);
#else
    temp = 0.0;
    for (int v = 0; v < ndim; v++) temp += p[2 + v] * p[2 + v];
    temp = sqrt(temp);
    temp += Eqn<EQEUL, 0>::chydro(p, g);
#endif
  }
#ifdef PION_FAST_MATH
  else if (ndim > 1) {
    // fast build: the fast speed along the weakest-field axis needs rho, p, |B|^2 and the smallest of the three
    // B_i^2 only -- no rotation of the state into that axis (the reference's sum of squares runs in the rotated
    // order: last-bit differences), shared reciprocal, seeded roots
    // (multiply-adds written out: this function is compiled into k_dt and into the stage kernels, and a restart
    // continues bit for bit only if both contract the same way)
    temp = fmx(fabs(p[2]), fabs(p[3]));
    if (ndim > 2) temp = fmx(temp, fabs(p[4]));
    const double bx2 = p[5] * p[5], by2 = p[6] * p[6], bz2 = p[7] * p[7];
    const double bn2 = fmn(fmn(bx2, by2), bz2);
    const double ir = frcp(p[0]);
    const double a2 = (g * p[1]) * ir;
    const double t1 = __builtin_fma((bx2 + by2) + bz2, ir, a2);
    const double t2 = fmx(PION_MACHINEACCURACY, __builtin_fma(t1, t1, -(4. * a2) * (bn2 * ir)));
    temp += sqrt_pos((t1 + sqrt_pos(t2)) * 0.5);
    return (dx * cfl) * frcp(temp);
  }
#endif
  else {
    temp = fabs(p[2]);
    if (ndim > 1) temp = dmax(temp, fabs(p[3]));
    if (ndim > 2) temp = dmax(temp, fabs(p[4]));
    if (ndim == 1) temp += Eqn<EQMHD, 0>::cfast(p, g);
    else {
      int newdir = 0;
      if (fabs(p[6]) < fabs(p[5])) {
        newdir = 1;
        if (fabs(p[7]) < fabs(p[6])) newdir = 2;
      }
      else if (fabs(p[7]) < fabs(p[5])) newdir = 2;
      double u1[8];
      to_sweep<8, true>(newdir, p, u1);
      temp += Eqn<EQMHD, 0>::cfast(u1, g);
    }
  }
  double t = dx / temp;
  t *= cfl;
  return t;
}

// all-cell index of on-grid cell number k (x fastest)
PDEV long ongrid_cell(const GridDesc &g, const long k)
{
  const int ix = (int)(k % g.ng[0]), iy = (int)((k / g.ng[0]) % g.ng[1]), iz = (int)(k / ((long)g.ng[0] * g.ng[1]));
  return (long)(ix + g.nbc[0]) + g.sy * (iy + g.nbc[1]) + g.sz * (iz + g.nbc[2]);
}

#endif
