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

// per member cell: keep dist and the per-axis offsets, mark it boundary data (stellar_wind_BC.cpp:277-278)
__global__ __launch_bounds__(256) void k_wind_cells(const WindMember m, const long *idx, const long n, double *dist,
                                                    double *off, const long ntot, uint8_t *flags)
{
  const long k = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= n) return;
  const long c = idx[k];
  const WindGeo w = wind_geo(m.g, m.pos, c);
  dist[k] = w.d;
  off[k] = w.x;
  off[ntot + k] = w.y;
  off[2 * ntot + k] = w.z;
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

}  // namespace pion
#endif
