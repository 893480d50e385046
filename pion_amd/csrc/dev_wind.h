// dev_wind.h -- stellar-wind sources built and updated on the device (pion_gpu_add_wind_source).
//
// Membership: BC_assign_STWIND_add_cells2src (boundaries/stellar_wind_boundaries.cpp:200-240) with the grid's
// distance_vertex2cell (grid/uniform_grid.cpp:1432-1461 Cartesian, :1764-1820 cylindrical, :2085-2120 spherical).
// States: stellar_wind::set_wind_cell_reference_state (grid/stellar_wind_BC.cpp:375-600) with the EOS gamma
// hard-coded to 5/3 (:331, :1360).
//
// Every function here is compiled without FMA contraction, in both builds: membership is decided by
// `dist <= radius`, and a contracted distance would move cells across a radius that lands on cell-centre distances.
// The states run once per boundary update over a few ten thousand cells, so the fast build gains nothing from
// contraction; both builds therefore give the same bits.
#ifndef PION_DEV_WIND_H
#define PION_DEV_WIND_H

#include <hip/hip_runtime.h>

#include "../../include/pion_gpu.h"
#include "kernels.h"

namespace pion {

// Geometry of one cell relative to a source: the per-axis differences cell - source
// (difference_vertex2cell; 0 on unused axes) and the distance.
struct WindGeo {
  double x, y, z, d;
};

__device__ inline WindGeo wind_geo(const GridDesc &g, const double *pos, const long c)
{
#pragma clang fp contract(off)
  const int i0 = (int)(c % g.nga[0]) - g.nbc[0];
  const int i1 = (int)((c / g.nga[0]) % g.nga[1]) - g.nbc[1];
  const int i2 = (int)(c / g.sz) - g.nbc[2];
  const double dxo2 = 0.5 * g.dx;
  // CI.get_dpos (cell_interface.cpp:506-512)
  const double x0 = g.xmin[0] + (2 * i0 + 1) * dxo2;
  WindGeo w;
  w.x = w.y = w.z = 0.0;
  if (g.cyl == 1) {
    // uniform_grid_cyl: z is Cartesian, R at the centre of volume, VectorOps_Cyl::R_com (VectorOps.h:414-418)
    const double R = g.xmin[1] + (2 * i1 + 1) * dxo2;
    const double Rc = R + g.dx * g.dx / 12. / R;
    double d = 0.0, t;
    t = pos[0] - x0;
    d += t * t;
    t = pos[1] - Rc;
    d += t * t;
    w.d = sqrt(d);
    w.x = x0 - pos[0];
    w.y = Rc - pos[1];
  }
  else if (g.cyl == 2) {
    // uniform_grid_sph: |r_src - R_com|, VectorOps_Sph::R_com (VectorOps_spherical.h:188-196)
    double delta2 = g.dx / x0;
    delta2 *= delta2;
    const double Rc = x0 * (1.0 + 0.25 * delta2) / (1.0 + delta2 / 12.0);
    w.d = fabs(pos[0] - Rc);
    w.x = Rc - pos[0];
  }
  else {
    // UniformGrid: sqrt(sum pow(v[i] - x[i], 2.0)), pow(a, 2.0) being a*a
    double temp = 0.0, t;
    t = pos[0] - x0;
    temp += t * t;
    w.x = x0 - pos[0];
    if (g.ndim > 1) {
      const double x1 = g.xmin[1] + (2 * i1 + 1) * dxo2;
      t = pos[1] - x1;
      temp += t * t;
      w.y = x1 - pos[1];
    }
    if (g.ndim > 2) {
      const double x2 = g.xmin[2] + (2 * i2 + 1) * dxo2;
      t = pos[2] - x2;
      temp += t * t;
      w.z = x2 - pos[2];
    }
    w.d = sqrt(temp);
  }
  return w;
}

// hipcub predicate / counting functor: is cell c within the source's radius?
struct WindMember {
  GridDesc g;
  double pos[3];
  double radius;
  __device__ bool operator()(const long c) const { return wind_geo(g, pos, c).d <= radius; }
};

// number of member cells (the count sizes the compacted list; the list itself comes from a scan)
__global__ __launch_bounds__(256) void k_wind_count(const WindMember m, unsigned long long *count)
{
  const long c = (long)blockIdx.x * blockDim.x + threadIdx.x;
  const int in = (c < m.g.ncell) ? (int)m(c) : 0;
  const int n = __syncthreads_count(in);
  if (threadIdx.x == 0 && n) atomicAdd(count, (unsigned long long)n);
}

// stellar_wind::add_cell's polar angle (stellar_wind_BC.cpp:286-318) from the offsets: 1-D 0, 2-D atan(|R / z|)
// (Rcyl = y, Zcyl = x), 3-D atan(|sqrt(x^2 + y^2) / z|)
__device__ inline double wind_theta(const int ndim, const WindGeo &w)
{
#pragma clang fp contract(off)
  if (ndim == 1) return 0.0;
  if (ndim == 2) return atan(fabs(w.y / w.x));
  return atan(fabs(sqrt(w.x * w.x + w.y * w.y) / w.z));
}

// per member cell: keep dist, the per-axis offsets and theta, mark it boundary data (stellar_wind_BC.cpp:277-278)
__global__ __launch_bounds__(256) void k_wind_cells(const WindMember m, const long *idx, const long n, double *dist,
                                                    double *off, double *theta, const long ntot, uint8_t *flags)
{
  const long k = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= n) return;
  const long c = idx[k];
  const WindGeo w = wind_geo(m.g, m.pos, c);
  dist[k] = w.d;
  off[k] = w.x;
  off[ntot + k] = w.y;
  off[2 * ntot + k] = w.z;
  theta[k] = wind_theta(m.g.ndim, w);
  flags[c] = (uint8_t)((flags[c] | PION_CELL_ISBD) & ~PION_CELL_ISDOMAIN);
}

// ---- moving sources (BC_update_STWIND, stellar_wind_boundaries.cpp:253-352) ------------------------------------
// A moving source's cells are found in an index box around its sphere instead of the whole grid: all-cell indices
// (ghosts included, 0 .. nga-1) lo[a] .. lo[a] + w[a] - 1, x fastest.  w is fixed when the source is added (the
// sphere's extent plus a margin of one cell each side); lo follows the source.  Box entries off the grid with ghosts
// are no cells.  Walking the box in its own order visits cells in increasing cell id.
struct WindBox {
  int lo[3], w[3];
  long n;   // w[0] * w[1] * w[2]
};

__device__ inline long wind_box_cell(const GridDesc &g, const WindBox &b, const long k)
{
  const int i0 = b.lo[0] + (int)(k % b.w[0]);
  const int i1 = b.lo[1] + (int)((k / b.w[0]) % b.w[1]);
  const int i2 = b.lo[2] + (int)(k / ((long)b.w[0] * b.w[1]));
  if (i0 < 0 || i0 >= g.nga[0] || i1 < 0 || i1 >= g.nga[1] || i2 < 0 || i2 >= g.nga[2]) return -1;
  return (long)i0 + g.sy * i1 + g.sz * i2;
}

// hipcub input: box entry -> cell id (-1: none); predicate: a cell within the radius (the exact membership test)
struct WindBoxCell {
  GridDesc g;
  WindBox b;
  __device__ long operator()(const long k) const { return wind_box_cell(g, b, k); }
};
struct WindBoxMember {
  WindMember m;
  __device__ bool operator()(const long c) const { return c >= 0 && m(c); }
};

// stellar_wind::remove_cells (stellar_wind_BC.cpp:349-367) for every cell (ghosts included) within the radius of the
// source's current position: isbd = false, isdomain = true, timestep = true -- whichever source the cell belongs to
__global__ __launch_bounds__(256) void k_wind_unflag(const WindMember m, const WindBox b, uint8_t *flags)
{
  const long k = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= b.n) return;
  const long c = wind_box_cell(m.g, b, k);
  if (c < 0 || !m(c)) return;
  flags[c] = (uint8_t)((flags[c] & ~PION_CELL_ISBD) | PION_CELL_ISDOMAIN | PION_CELL_TIMESTEP);
}

// k_wind_cells for a moving source, whose count the compaction left on the device (*dn <= the launch's capacity)
__global__ __launch_bounds__(256) void k_wind_cells_dn(const WindMember m, const long *idx, const long *dn,
                                                       double *dist, double *off, const long ntot, uint8_t *flags)
{
  const long k = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= *dn) return;
  const long c = idx[k];
  const WindGeo w = wind_geo(m.g, m.pos, c);
  dist[k] = w.d;
  off[k] = w.x;
  off[ntot + k] = w.y;
  off[2 * ntot + k] = w.z;
  flags[c] = (uint8_t)((flags[c] | PION_CELL_ISBD) & ~PION_CELL_ISDOMAIN);
}

// the legacy list of pion_gpu_set_wind_cells: mark its cells boundary data (stellar_wind_BC.cpp:277-278)
__global__ __launch_bounds__(256) void k_flag_wind_list(const long *idx, const long n, uint8_t *flags)
{
  const long k = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= n) return;
  const long c = idx[k];
  flags[c] = (uint8_t)((flags[c] | PION_CELL_ISBD) & ~PION_CELL_ISDOMAIN);
}

// Parameters of one source at the time of the update (cgs, as stored in wind_source)
struct WindSrcDev {
  double Mdot, Vinf, v_rot, Tw, Rstar, Bstar, radius;
  double tr[PION_MAX_NTR];
  long off, n;   // the source's range in the concatenated cell list (moving source: n = its capacity)
  const long *dn;   // moving source: its cell count, on the device (nullptr: n)
  int active;
};

struct WindStateArgs {
  double *P, *Ph, *states;   // states: [ncells][nvar], what get_wind_cells returns
  const long *idx;
  const double *dist, *off;  // off: [3][ntot]
  long ntot, ncell;
  int nsrc, nvar, ntracer, ndim, cart2d, eqntype, cooling;
  double Tmin, Mu_tot_over_kB;
  WindSrcDev s[PION_MAX_WIND_SOURCES];
};

// stellar_wind::set_wind_cell_reference_state (stellar_wind_BC.cpp:375-600) for one cell, then
// set_cell_values (:642-677): the state goes to P and Ph.  Expression order as in the reference;
// pconst.pow_fast(a, b) = exp(b*log(a)) (constants.cpp:78-84).
// One launch per source, in id order: where sources overlap, the later one's state stands, as in the reference.
__global__ __launch_bounds__(256) void k_wind_state(const WindStateArgs a, const int s)
{
#pragma clang fp contract(off)
  const WindSrcDev &W = a.s[s];
  const long k0 = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (k0 >= (W.dn ? *W.dn : W.n)) return;
  const long k = W.off + k0;
  const double gamma = 5. / 3.;
  const double kB = 1.38064852e-16, m_p = 1.672621898e-24, pi = 3.14159265358979324;
  const double dist = a.dist[k];
  const double x = a.off[k], y = a.off[a.ntot + k], z = a.off[2 * a.ntot + k];
  double p[PION_MAX_NVAR];
  bool set_rho = true;
  if (dist < 0.75 * W.radius && a.ndim > 1) {
    p[0] = 1.0e-31;
    p[1] = 1.0e-31;
    set_rho = false;
  }
  if (a.cart2d) {
    // 2-D slab symmetry: rho = Mdot/(2 pi R v_inf)
    p[0] = W.Mdot / (W.Vinf * 2.0 * pi * dist);
    p[1] = kB * W.Tw / m_p;
    p[1] *= exp((gamma - 1.0) * log(2.0 * pi * W.Rstar * W.Vinf / W.Mdot));
    p[1] *= exp((gamma)*log(p[0]));
  }
  else if (set_rho) {
    p[0] = 1.0 / (dist);
    p[0] *= p[0];
    p[0] *= W.Mdot / (W.Vinf * 4.0 * pi);
    p[1] = kB * W.Tw / m_p;
    p[1] *= exp((gamma - 1.0) * log(4.0 * pi * W.Rstar * W.Rstar * W.Vinf / W.Mdot));
    p[1] *= exp((gamma)*log(p[0]));
  }
  // velocities (:470-499); J along +z
  if (a.ndim == 1) {
    p[2] = W.Vinf * x / dist;
    p[3] = 0.0;
    p[4] = 0.0;
  }
  else if (a.ndim == 2) {
    p[2] = W.Vinf * x / dist;
    p[3] = W.Vinf * y / dist;
    p[4] = W.v_rot * W.Rstar * y / exp(2.0 * log(dist));
  }
  else {
    p[2] = W.Vinf * x / dist;
    p[3] = W.Vinf * y / dist;
    p[4] = W.Vinf * z / dist;
    p[2] += -W.v_rot * W.Rstar * y / exp(2.0 * log(dist));
    p[3] += W.v_rot * W.Rstar * x / exp(2.0 * log(dist));
  }
  // split monopole + toroidal field (:502-564); MHD in 1-D is refused when the source is added
  if (a.eqntype != PION_EQEUL) {
    const double B_s = W.Bstar / sqrt(4.0 * pi);
    const double D_s = W.Rstar / dist;
    const double D_2 = D_s * D_s;
    double beta_B_sint = (W.v_rot / W.Vinf) * B_s * D_s;
    if (a.ndim == 2) {
      p[5] = B_s * D_2 * fabs(x) / dist;
      p[6] = B_s * D_2 / dist;
      p[6] = (x > 0.0) ? y * p[6] : -y * p[6];
      beta_B_sint = beta_B_sint * y / dist;
      p[7] = (x > 0.0) ? -beta_B_sint : beta_B_sint;
    }
    else {
      p[5] = B_s * D_2 / dist;
      p[5] = (z > 0.0) ? x * p[5] : -x * p[5];
      p[6] = B_s * D_2 / dist;
      p[6] = (z > 0.0) ? y * p[6] : -y * p[6];
      p[7] = B_s * D_2 * fabs(z) / dist;
      beta_B_sint *= sqrt(x * x + y * y) / dist;
      beta_B_sint = (z > 0.0) ? -beta_B_sint : beta_B_sint;
      p[5] += -beta_B_sint * y / dist;
      p[6] += beta_B_sint * x / dist;
    }
    if (a.eqntype == PION_EQGLM) p[8] = 0.0;
  }
  const int ftr = a.nvar - a.ntracer;
  for (int v = 0; v < a.ntracer && v < PION_MAX_NTR; v++) p[ftr + v] = W.tr[v];
  // SET_NEGATIVE_PRESSURE_TO_FIXED_TEMPERATURE (:578-590): mp_only_cooling::Temperature / Set_Temp
  // (mp_only_cooling.cpp:244-280) with a microphysics object, else a neutral-gas floor
  if (a.cooling) {
    if (p[1] * a.Mu_tot_over_kB / p[0] < a.Tmin) p[1] = p[0] * a.Tmin / a.Mu_tot_over_kB;
  }
  else {
    const double floor_p = a.Tmin * p[0] * kB * 0.78625 / m_p;
    p[1] = (p[1] < floor_p) ? floor_p : p[1];
  }
  const long c = a.idx[k];
  for (int v = 0; v < a.nvar; v++) {
    a.P[v * a.ncell + c] = p[v];
    a.Ph[v * a.ncell + c] = p[v];
    a.states[k * a.nvar + v] = p[v];
  }
}

// ---- rotating stars, LGM99 (grid/stellar_wind_angle.cpp, WINDTYPE_ANGLE) ---------------------------------------
// The knots of stellar_wind_angle::setup_tables (:92-212)
#define PION_ANGLE_NTHETA 25
#define PION_ANGLE_NOMEGA 25
#define PION_ANGLE_NTEFF 22

// member cells of a rotating source whose theta lies outside (lo, hi]: root_find_trilinear_vec (tools/interpolate.cpp
// :385-470) calls rep.error below theta_vec[0] (NaN included) and runs past the vector above theta_vec[24]
__global__ __launch_bounds__(256) void k_wind_theta_bad(const WindMember m, const double lo, const double hi,
                                                        unsigned long long *count)
{
  const long c = (long)blockIdx.x * blockDim.x + threadIdx.x;
  int bad = 0;
  if (c < m.g.ncell) {
    const WindGeo w = wind_geo(m.g, m.pos, c);
    if (w.d <= m.radius) {
      const double t = wind_theta(m.g.ndim, w);
      bad = !(t > lo && t <= hi);
    }
  }
  const int n = __syncthreads_count(bad);
  if (threadIdx.x == 0 && n) atomicAdd(count, (unsigned long long)n);
}

// One rotating source at the time of the update.  Everything that does not depend on the cell comes from the host:
// omega = min(min(0.9999, v_rot/vcrit), 0.999), delta_interp (root_find_bilinear_vec), the omega and Teff fractions
// of root_find_trilinear_vec, and its alpha table at the omega and Teff brackets over all theta knots:
// a[0] = alpha[x0][*][z0], a[1] = alpha[x0][*][z1], a[2] = alpha[x1][*][z0], a[3] = alpha[x1][*][z1].
struct WindAngleDev {
  double Mdot, Vinf, v_rot, Tw, Rstar, Bstar, radius;
  double omega, delta, xi, dx, dz;
  double theta[PION_ANGLE_NTHETA];
  double a[4][PION_ANGLE_NTHETA];
  double tr[PION_MAX_NTR];
  long off, n;
};

struct WindAngleArgs {
  double *P, *Ph, *states;
  const long *idx;
  const double *dist, *off, *theta;
  long ntot, ncell;
  int nvar, ntracer, ndim, eqntype, cooling;
  double Tmin, Mu_tot_over_kB;
  WindAngleDev s;
};

// stellar_wind_angle::set_wind_cell_reference_state (stellar_wind_angle.cpp:464-691) for one cell of a 2-D or 3-D
// grid, then set_cell_values: the state goes to P and Ph.  fn_density_interp (:386-455) is evaluated at dist and at
// Rstar with the same alpha and delta; fn_v_inf (:343-353).  Expression order as in the reference; pow_fast(a, b) =
// exp(b*log(a)).  One launch per active rotating source, in id order with the k_wind_state launches.
__global__ __launch_bounds__(256) void k_wind_state_angle(const WindAngleArgs a)
{
#pragma clang fp contract(off)
  const WindAngleDev &W = a.s;
  const long k0 = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (k0 >= W.n) return;
  const long k = W.off + k0;
  const double gamma = 5. / 3., c_gamma = 0.35;
  const double kB = 1.38064852e-16, m_p = 1.672621898e-24, pi = 3.14159265358979324;
  const double dist = a.dist[k];
  const double x = a.off[k], y = a.off[a.ntot + k], z = a.off[2 * a.ntot + k];
  const double theta = a.theta[k];
  // root_find_trilinear_vec in theta: while (y > y_vec[j]) j++; set-up keeps theta in (theta_vec[0], theta_vec[24]]
  int j = 1;
  while (j < PION_ANGLE_NTHETA - 1 && theta > W.theta[j]) j++;
  const double dy = (theta - W.theta[j - 1]) / (W.theta[j] - W.theta[j - 1]);
  const double f000 = W.a[0][j - 1], f001 = W.a[1][j - 1], f010 = W.a[0][j], f100 = W.a[2][j - 1];
  const double f110 = W.a[2][j], f011 = W.a[1][j], f101 = W.a[3][j - 1], f111 = W.a[3][j];
  const double c0 = f000;
  const double c1 = f100 - f000;
  const double c2 = f010 - f000;
  const double c3 = f001 - f000;
  const double c4 = f110 - f010 - f100 + f000;
  const double c5 = f011 - f001 - f010 + f000;
  const double c6 = f101 - f001 - f100 + f000;
  const double c7 = f111 - f011 - f101 - f110 + f100 + f001 + f010 - f000;
  const double dx = W.dx, dz = W.dz;
  const double alpha = c0 + c1 * dx + c2 * dy + c3 * dz + c4 * dx * dy + c5 * dy * dz + c6 * dz * dx + c7 * dx * dy * dz;
  const double sint = sin(theta);
  const double fxi = exp(W.xi * log(1.0 - W.omega * sint));
  // fn_v_inf: std::max(0.5e5, v_inf pow_fast(1 - omega sin(theta), c_gamma))
  double Vinf = W.Vinf * exp(c_gamma * log(1.0 - W.omega * sint));
  Vinf = (0.5e5 < Vinf) ? Vinf : 0.5e5;
  double p[PION_MAX_NVAR];
  bool set_rho = true;
  if (dist < 0.75 * W.radius && a.ndim > 1) {
    p[0] = 1.0e-31;
    p[1] = 1.0e-31;
    set_rho = false;
  }
  if (set_rho) {
    p[0] = (W.Mdot * alpha * W.delta * fxi);
    p[0] /= (8.0 * pi * exp(2.0 * log(dist)) * Vinf);
    double rho_s = (W.Mdot * alpha * W.delta * fxi);
    rho_s /= (8.0 * pi * exp(2.0 * log(W.Rstar)) * Vinf);
    p[1] = W.Tw * kB / m_p;
    p[1] *= exp((1.0 - gamma) * log(rho_s));
    p[1] *= exp(gamma * log(p[0]));
  }
  // velocities (:546-577): no rotation term in 2-D; J along +z in 3-D
  p[2] = Vinf * x / dist;
  p[3] = Vinf * y / dist;
  if (a.ndim == 2) {
    p[4] = 0.0;
  }
  else {
    p[4] = Vinf * z / dist;
    p[2] += -W.v_rot * W.Rstar * y / exp(2.0 * log(dist));
    p[3] += W.v_rot * W.Rstar * x / exp(2.0 * log(dist));
  }
  // split monopole + toroidal field (:584-638) with the latitude-dependent Vinf
  if (a.eqntype != PION_EQEUL) {
    const double B_s = W.Bstar / sqrt(4.0 * pi);
    const double D_s = W.Rstar / dist;
    const double D_2 = D_s * D_s;
    double beta_B_sint = (W.v_rot / Vinf) * B_s * D_s;
    if (a.ndim == 2) {
      p[5] = B_s * D_2 * fabs(x) / dist;
      p[6] = B_s * D_2 / dist;
      p[6] = (x > 0.0) ? y * p[6] : -y * p[6];
      beta_B_sint = beta_B_sint * y / dist;
      p[7] = (x > 0.0) ? -beta_B_sint : beta_B_sint;
    }
    else {
      p[5] = B_s * D_2 / dist;
      p[5] = (z > 0.0) ? x * p[5] : -x * p[5];
      p[6] = B_s * D_2 / dist;
      p[6] = (z > 0.0) ? y * p[6] : -y * p[6];
      p[7] = B_s * D_2 * fabs(z) / dist;
      beta_B_sint *= sqrt(x * x + y * y) / dist;
      beta_B_sint = (z > 0.0) ? -beta_B_sint : beta_B_sint;
      p[5] += -beta_B_sint * y / dist;
      p[6] += beta_B_sint * x / dist;
    }
    if (a.eqntype == PION_EQGLM) p[8] = 0.0;
  }
  const int ftr = a.nvar - a.ntracer;
  for (int v = 0; v < a.ntracer && v < PION_MAX_NTR; v++) p[ftr + v] = W.tr[v];
  // SET_NEGATIVE_PRESSURE_TO_FIXED_TEMPERATURE (:661-675), as in k_wind_state
  if (a.cooling) {
    if (p[1] * a.Mu_tot_over_kB / p[0] < a.Tmin) p[1] = p[0] * a.Tmin / a.Mu_tot_over_kB;
  }
  else {
    const double floor_p = a.Tmin * p[0] * kB * 0.78625 / m_p;
    p[1] = (p[1] < floor_p) ? floor_p : p[1];
  }
  const long c = a.idx[k];
  for (int v = 0; v < a.nvar; v++) {
    a.P[v * a.ncell + c] = p[v];
    a.Ph[v * a.ncell + c] = p[v];
    a.states[k * a.nvar + v] = p[v];
  }
}

}  // namespace pion
#endif
