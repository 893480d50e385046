// pion_wind.hip -- the stellar-wind sources of the C-ABI (include/pion_gpu.h) where they touch the device: the member
// cells of a source, found and compacted on the device, the move along an orbit, the launches of a boundary update.
// The kernels: dev_wind.h.  Tables, set-up and the update step of a source are host code: wind_host.h.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstring>

#include <hipcub/hipcub.hpp>

#include "dev_wind.h"
#include "pion_handle.h"

using namespace pion;
using namespace pion::impl;
static_assert(ANGLE_NTHETA == PION_ANGLE_NTHETA && ANGLE_NOMEGA == PION_ANGLE_NOMEGA && ANGLE_NTEFF == PION_ANGLE_NTEFF);

namespace {

// Append n slots to the concatenated wind-source lists (cell ids, dist, offsets, states; the new states zeroed); the
// earlier sources' entries keep their place at the front.  h->nws grows by n.
int wind_lists_grow(Handle *h, const long n)
{
  const long o = h->nws, ntot = o + n;
  const int nvar = h->cfg.nvar;
  long *nidx = nullptr;
  double *ndist = nullptr, *noff = nullptr, *nstate = nullptr, *ntheta = nullptr;
  if (ntot > 0) {
    HCHECK(h, hipMalloc(&nidx, sizeof(long) * ntot));
    HCHECK(h, hipMalloc(&ndist, sizeof(double) * ntot));
    HCHECK(h, hipMalloc(&ntheta, sizeof(double) * ntot));
    HCHECK(h, hipMemsetAsync(ntheta, 0, sizeof(double) * ntot, h->stream));
    HCHECK(h, hipMalloc(&noff, sizeof(double) * 3 * ntot));
    HCHECK(h, hipMalloc(&nstate, sizeof(double) * ntot * nvar));
    HCHECK(h, hipMemsetAsync(nstate, 0, sizeof(double) * ntot * nvar, h->stream));
  }
  if (o > 0) {
    HCHECK(h, hipMemcpyAsync(nidx, h->dws_idx, sizeof(long) * o, hipMemcpyDeviceToDevice, h->stream));
    HCHECK(h, hipMemcpyAsync(ndist, h->dws_dist, sizeof(double) * o, hipMemcpyDeviceToDevice, h->stream));
    HCHECK(h, hipMemcpyAsync(ntheta, h->dws_theta, sizeof(double) * o, hipMemcpyDeviceToDevice, h->stream));
    for (int a = 0; a < 3; a++)
      HCHECK(h, hipMemcpyAsync(noff + a * ntot, h->dws_off + a * o, sizeof(double) * o, hipMemcpyDeviceToDevice,
                               h->stream));
    HCHECK(h, hipMemcpyAsync(nstate, h->dws_state, sizeof(double) * o * nvar, hipMemcpyDeviceToDevice, h->stream));
  }
  HCHECK(h, hipStreamSynchronize(h->stream));
  hipFree(h->dws_idx);
  hipFree(h->dws_dist);
  hipFree(h->dws_off);
  hipFree(h->dws_state);
  hipFree(h->dws_theta);
  h->dws_idx = nidx;
  h->dws_theta = ntheta;
  h->dws_dist = ndist;
  h->dws_off = noff;
  h->dws_state = nstate;
  h->nws = ntot;
  return 0;
}

// The box of moving source W centred on `pos`: per axis the w cells from one below the first cell whose centre can
// lie within the radius (the exact test runs in the kernels).  A NaN position gives some box; no cell passes there.
WindBox wind_box(const Handle *h, const WindSource &W, const double *pos)
{
  const GridDesc &g = h->g;
  WindBox b;
  b.n = 1;
  for (int a = 0; a < 3; a++) {
    b.w[a] = W.box_w[a];
    b.lo[a] = 0;
    if (a < g.ndim && b.w[a] < g.nga[a]) {
      // all-cell index i has its centre at xmin + (i - nbc + 0.5) dx
      double t = (pos[a] - W.radius - g.xmin[a]) / g.dx - 0.5 + g.nbc[a];
      if (!(t == t)) t = 0.0;
      t = std::min(std::max(t, -2.0 * g.nga[a]), 2.0 * g.nga[a]);
      b.lo[a] = (int)floor(t) - 1;
    }
    b.n *= b.w[a];
  }
  return b;
}

WindMember wind_member(const Handle *h, const WindSource &W)
{
  return WindMember{h->g, {W.pos[0], W.pos[1], W.pos[2]}, W.radius};
}

typedef hipcub::TransformInputIterator<long, WindBoxCell, hipcub::CountingInputIterator<long>> WindBoxIter;

// moving source W's box at W.pos compacted into its slot of the lists, the count in W.dn (no scratch: the size query)
hipError_t wind_select_box(Handle *h, const WindSource &W, void *scratch, size_t &bytes)
{
  const WindBoxCell bc = {h->g, wind_box(h, W, W.pos)};
  const WindBoxMember pred = {wind_member(h, W)};
  WindBoxIter cells(hipcub::CountingInputIterator<long>(0), bc);
  return hipcub::DeviceSelect::If(scratch, bytes, cells, h->dws_idx + W.off, W.dn, (int)W.n, pred, h->stream);
}

// BC_assign_STWIND_add_cells2src for a moving source at W.pos: the cells of its box within the radius, in cell-id
// order, compacted into its slot of the lists with the count left in W.dn; then dist, offsets and the flags
// (stellar_wind::add_cell, stellar_wind_BC.cpp:255-283).  Asynchronous, no allocation.
int wind_add_cells_box(Handle *h, const WindSource &W)
{
  size_t bytes = W.scan_bytes;
  HCHECK(h, wind_select_box(h, W, W.dscan, bytes));
  hipLaunchKernelGGL(k_wind_cells_dn, dim3((unsigned)((W.n + 255) / 256)), dim3(256), 0, h->stream, wind_member(h, W),
                     h->dws_idx + W.off, W.dn, h->dws_dist + W.off, h->dws_off + W.off, h->nws, h->dflags);
  return 0;
}

// A source with orbit_period != 0 (2-D / 3-D Cartesian): its slot in the lists, the count and the compaction scratch
// are sized once, to the box.  The cells at dpos_init join it now, as for a fixed source.
int add_moving_wind_source(Handle *h, WindSource &W, int *id)
{
  const GridDesc &g = h->g;
  long cap = 1;
  for (int a = 0; a < 3; a++) {
    W.box_w[a] = 1;
    if (a < g.ndim) {
      // the sphere spans at most floor(2 radius / dx) + 1 cell centres per axis; plus the margin, plus rounding
      const double w = floor(2.0 * W.radius / g.dx) + 5.0;
      W.box_w[a] = (w >= (double)g.nga[a]) ? g.nga[a] : (int)w;
    }
    cap *= W.box_w[a];
  }
  if (cap > 0x7fffffffL) {
    h->err = "wind source: the orbit box is too large";
    return PION_GPU_EINVAL;
  }
  if (int rc = wind_lists_grow(h, cap)) return rc;
  W.off = h->nws - cap;
  W.n = cap;
  HCHECK(h, hipMalloc(&W.dn, sizeof(long)));
  HCHECK(h, hipMemsetAsync(W.dn, 0, sizeof(long), h->stream));
  W.scan_bytes = 0;
  HCHECK(h, wind_select_box(h, W, nullptr, W.scan_bytes));
  HCHECK(h, hipMalloc(&W.dscan, W.scan_bytes > 0 ? W.scan_bytes : 1));
  h->wsrc.push_back(W);
  if (int rc = wind_add_cells_box(h, h->wsrc.back())) return rc;
  HCHECK(h, hipGetLastError());
  HCHECK(h, hipStreamSynchronize(h->stream));
  state_changed(h);   // the ISBD flags decide which cells enter the time-step reduction
  if (id) *id = (int)h->wsrc.size() - 1;
  return 0;
}

// BC_update_STWIND (stellar_wind_boundaries.cpp:270-322) for every moving source, in id order: remove_cells on the
// cells within the radius of the current position, the new position from simtime, then the cells within the radius
// of that position join the source.  Launches only, over the two boxes; nothing waits for the device.
int wind_sources_move(Handle *h, const double simtime)
{
  bool moved = false;
  for (size_t s = 0; s < h->wsrc.size(); s++) {
    WindSource &W = h->wsrc[s];
    if (!W.moving) continue;
    const WindBox ob = wind_box(h, W, W.pos);
    hipLaunchKernelGGL(k_wind_unflag, dim3((unsigned)((ob.n + 255) / 256)), dim3(256), 0, h->stream,
                       wind_member(h, W), ob, h->dflags);
    double np[3];
    wind_orbit_position(W.orbit, h->cfg.ndim, simtime, np);
    for (int a = 0; a < 3; a++) {
      moved = moved || !(np[a] == W.pos[a]);
      W.pos[a] = np[a];
    }
    if (int rc = wind_add_cells_box(h, W)) return rc;
  }
  // An unchanged position leaves the flags as they were: every cell an unflag touches lies in the sphere of that
  // moving source, which re-adds it at once.  A move changes them, and with them the cached time step.
  if (moved) state_changed(h);
  return 0;
}

// what WindSrcDev and WindAngleDev share: the source's values now and its range in the lists
template <class Dev>
void wind_dev_fill(const Handle *h, const WindSource &W, Dev &d)
{
  d.Mdot = W.now.Mdot;
  d.Vinf = W.now.Vinf;
  d.v_rot = W.now.vrot;
  d.Tw = W.now.Tw;
  d.Rstar = W.now.Rstar;
  d.Bstar = W.Bstar;
  d.radius = W.radius;
  for (int v = 0; v < PION_MAX_NTR; v++) d.tr[v] = (v < h->cfg.ntracer) ? W.now.tr[v] : 0.0;
  d.off = W.off;
  d.n = W.n;
}

// what WindStateArgs and WindAngleArgs share: the arrays and the grid's scalars
template <class Args>
void wind_args_fill(const Handle *h, Args &a)
{
  memset(&a, 0, sizeof a);
  a.P = h->dP;
  a.Ph = h->dPh;
  a.states = h->dws_state;
  a.idx = h->dws_idx;
  a.dist = h->dws_dist;
  a.off = h->dws_off;
  a.ntot = h->nws;
  a.ncell = h->g.ncell;
  a.nvar = h->cfg.nvar;
  a.ntracer = h->cfg.ntracer;
  a.ndim = h->cfg.ndim;
  a.eqntype = h->cfg.eqntype;
  a.cooling = (h->cfg.cooling != 0) ? 1 : 0;
  a.Tmin = h->cfg.min_temp;   // EP.MinTemperature, as handed to the stellar_wind constructor
  a.Mu_tot_over_kB = h->Mu_tot_over_kB;
}

// k_wind_state_angle's launch for rotating source W: the parts of fn_density_interp that do not depend on the cell
void wind_angle_launch(Handle *h, const WindSource &W)
{
  WindAngleArgs g;
  wind_args_fill(h, g);
  g.theta = h->dws_theta;
  WindAngleDev &d = g.s;
  wind_dev_fill(h, W, d);
  const AngleBracket b = angle_bracket(h->angle, W.now);
  d.xi = h->angle.xi;
  d.omega = b.omega;
  d.delta = b.delta;
  d.dx = b.dx;
  d.dz = b.dz;
  static_assert(sizeof d.a == sizeof b.a && sizeof d.theta == sizeof h->angle.theta);
  memcpy(d.a, b.a, sizeof d.a);
  memcpy(d.theta, h->angle.theta, sizeof d.theta);
  hipLaunchKernelGGL(k_wind_state_angle, dim3((unsigned)((W.n + 255) / 256)), dim3(256), 0, h->stream, g);
}

// Count on the device and read the count back: `kernel` runs over every cell of the grid and adds to the zeroed
// counter, its last argument.  Synchronises; the counter is freed on every return.
template <class Kernel, class... Args>
int wind_device_count(Handle *h, unsigned long long *cnt, Kernel kernel, const Args &...args)
{
  DevBuf<unsigned long long> d;
  HCHECK(h, hipMalloc(&d.p, sizeof *d.p));
  HCHECK(h, hipMemsetAsync(d.p, 0, sizeof *d.p, h->stream));
  hipLaunchKernelGGL(kernel, dim3((unsigned)((h->g.ncell + 255) / 256)), dim3(256), 0, h->stream, args..., d.p);
  HCHECK(h, hipGetLastError());
  HCHECK(h, hipMemcpyAsync(cnt, d.p, sizeof *cnt, hipMemcpyDeviceToHost, h->stream));
  HCHECK(h, hipStreamSynchronize(h->stream));
  return 0;
}

// BC_assign_STWIND_add_cells2src for a fixed source (orbit_period == 0): every cell, ghosts included, within the radius
// joins it in cell-id order (hipcub::DeviceSelect keeps it); then dist, offsets, theta and the flags.  Synchronises.
int add_fixed_wind_source(Handle *h, WindSource &W, int *id)
{
  const long ncell = h->g.ncell;
  const WindMember m = wind_member(h, W);
  unsigned long long cnt = 0;
  if (int rc = wind_device_count(h, &cnt, k_wind_count, m)) return rc;
  const long n = (long)cnt;
  if (int rc = wind_lists_grow(h, n)) return rc;
  const long o = h->nws - n, ntot = h->nws;
  if (n > 0) {
    long nsel = 0;
    {
      hipcub::CountingInputIterator<long> cells(0);
      DevBuf<long> dsel;
      DevBuf<void> tmp;
      HCHECK(h, hipMalloc(&dsel.p, sizeof(long)));
      size_t tmp_bytes = 0;
      HCHECK(h, hipcub::DeviceSelect::If(nullptr, tmp_bytes, cells, h->dws_idx + o, dsel.p, ncell, m, h->stream));
      HCHECK(h, hipMalloc(&tmp.p, tmp_bytes));
      HCHECK(h, hipcub::DeviceSelect::If(tmp.p, tmp_bytes, cells, h->dws_idx + o, dsel.p, ncell, m, h->stream));
      HCHECK(h, hipMemcpyAsync(&nsel, dsel.p, sizeof nsel, hipMemcpyDeviceToHost, h->stream));
      HCHECK(h, hipStreamSynchronize(h->stream));
    }
    if (nsel != n) {
      h->err = "wind source: membership count and compaction disagree";
      return PION_GPU_EDEVICE;
    }
    hipLaunchKernelGGL(k_wind_cells, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, h->stream, m, h->dws_idx + o,
                       n, h->dws_dist + o, h->dws_off + o, h->dws_theta + o, ntot, h->dflags);
  }
  HCHECK(h, hipGetLastError());
  HCHECK(h, hipStreamSynchronize(h->stream));
  W.off = o;
  W.n = n;
  h->wsrc.push_back(W);
  state_changed(h);   // the ISBD flags decide which cells enter the time-step reduction
  if (id) *id = (int)h->wsrc.size() - 1;
  return 0;
}

// Both entry points: set-up on the host, then the cells.  A rotating source: first the member cells whose theta lies
// outside (theta_vec[0], theta_vec[24]] are counted on the device, before anything changes.
int add_wind_source(void *handle, const pion_gpu_wind_source *src, const double *evo_vcrit, const bool rotating,
                    const double xi, int *id)
{
  Handle *h = use(handle);
  if (!h || !src) return PION_GPU_EINVAL;
  WindSource W;
  const char *msg = wind_source_setup(h->cfg, *src, evo_vcrit, rotating, xi, h->wsrc, h->angle, W);
  if (!msg && rotating) {
    h->have_angle = true;
    const double *theta = h->angle.theta;
    unsigned long long bad = 0;
    if (int rc = wind_device_count(h, &bad, k_wind_theta_bad, wind_member(h, W), theta[0], theta[ANGLE_NTHETA - 1]))
      return rc;
    if (bad > 0) msg = "rotating wind source: a member cell's theta lies outside the LGM99 table";
  }
  if (msg) {
    h->err = msg;
    return PION_GPU_EINVAL;
  }
  return W.moving ? add_moving_wind_source(h, W, id) : add_fixed_wind_source(h, W, id);
}

}  // namespace

// before any launch of a boundary update: a rotating source that cannot be evaluated makes it EINVAL, nothing written
int impl::wind_angle_check(Handle *h, const double simtime)
{
  for (const WindSource &W : h->wsrc) {
    if (W.type == 2 && !wind_angle_in_range(W, h->angle, h->cfg.ntracer, simtime)) {
      h->err = "rotating wind source: omega <= 0 or Tw <= 1000 K (stellar_wind_angle look-up out of range)";
      return PION_GPU_EINVAL;
    }
  }
  return 0;
}

// update_source, then stellar_wind_evolution::set_cell_values (stellar_wind_BC.cpp:1334-1372) for every source: one
// launch per active source, in id order, writes the reference states of its cells (no host synchronisation: the
// parameters are scalars of the host, the launch carries them)
int impl::wind_sources_update(Handle *h, const double simtime)
{
  if (int rc = wind_sources_move(h, simtime)) return rc;
  WindStateArgs a;
  wind_args_fill(h, a);
  a.nsrc = (int)h->wsrc.size();
  a.cart2d = (h->cfg.ndim == 2 && h->cfg.coord_sys == 1) ? 1 : 0;
  for (size_t s = 0; s < h->wsrc.size(); s++) {
    WindSource &W = h->wsrc[s];
    WindSrcDev &d = a.s[s];
    d.active = wind_source_update(W, h->angle, h->cfg.ntracer, simtime, W.now) ? 1 : 0;
    wind_dev_fill(h, W, d);
    d.dn = W.moving ? W.dn : nullptr;
  }
  // stellar_wind_evolution::set_cell_values: an inactive source keeps its cells flagged but does not write them
  for (int s = 0; s < a.nsrc; s++) {
    if (!(a.s[s].active && a.s[s].n > 0)) continue;
    if (h->wsrc[s].type == 2) wind_angle_launch(h, h->wsrc[s]);
    else hipLaunchKernelGGL(k_wind_state, dim3((unsigned)((a.s[s].n + 255) / 256)), dim3(256), 0, h->stream, a, s);
  }
  return 0;
}

void impl::wind_free(Handle *h)
{
  hipFree(h->dwind_idx);
  hipFree(h->dwind_state);
  hipFree(h->dws_idx);
  hipFree(h->dws_dist);
  hipFree(h->dws_off);
  hipFree(h->dws_state);
  hipFree(h->dws_theta);
  for (WindSource &W : h->wsrc) {
    hipFree(W.dn);
    hipFree(W.dscan);
  }
}

extern "C" {

int pion_gpu_set_wind_cells(void *handle, long n, const long *idx, const double *states)
{
  Handle *h = use(handle);
  state_changed(h);   // the ISBD flags decide which cells enter the time-step reduction
  hipFree(h->dwind_idx);
  hipFree(h->dwind_state);
  h->dwind_idx = nullptr;
  h->dwind_state = nullptr;
  h->nwind = n;
  if (n > 0) {
    for (long k = 0; k < n; k++) {
      if (idx[k] < 0 || idx[k] >= h->g.ncell) {
        h->nwind = 0;
        return PION_GPU_EINVAL;
      }
    }
    HCHECK(h, hipMalloc(&h->dwind_idx, sizeof(long) * n));
    HCHECK(h, hipMalloc(&h->dwind_state, sizeof(double) * n * h->cfg.nvar));
    HCHECK(h, hipMemcpy(h->dwind_idx, idx, sizeof(long) * n, hipMemcpyHostToDevice));
    HCHECK(h, hipMemcpy(h->dwind_state, states, sizeof(double) * n * h->cfg.nvar, hipMemcpyHostToDevice));
    // isbd = true, isdomain = false (stellar_wind_BC.cpp:277-278), on the device: the flags there are the only
    // current ones once a wind source has moved
    hipLaunchKernelGGL(k_flag_wind_list, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, h->stream, h->dwind_idx, n,
                       h->dflags);
    HCHECK(h, hipGetLastError());
    HCHECK(h, hipStreamSynchronize(h->stream));
  }
  return 0;
}

int pion_gpu_add_wind_source(void *handle, const pion_gpu_wind_source *src, int *id)
{
  return add_wind_source(handle, src, nullptr, false, 0.0, id);
}

int pion_gpu_add_rotating_wind_source(void *handle, const pion_gpu_wind_source *src, const double *evo_vcrit,
                                      double xi, int *id)
{
  return add_wind_source(handle, src, evo_vcrit, true, xi, id);
}

int pion_gpu_get_wind_source_pos(void *handle, int id, double *pos)
{
  Handle *h = use(handle);
  if (!h || !pos || id < 0 || id >= (int)h->wsrc.size()) return PION_GPU_EINVAL;
  for (int a = 0; a < PION_MAX_DIM; a++) pos[a] = (a < 3) ? h->wsrc[id].pos[a] : 0.0;
  return 0;
}

int pion_gpu_get_wind_cells(void *handle, int id, long *n, long *idx, double *states)
{
  Handle *h = use(handle);
  if (!h || !n || id < 0 || id >= (int)h->wsrc.size()) return PION_GPU_EINVAL;
  const WindSource &W = h->wsrc[id];
  long cnt = W.n;
  if (W.moving) {
    // the count the last move left on the device
    HCHECK(h, hipMemcpyAsync(&cnt, W.dn, sizeof cnt, hipMemcpyDeviceToHost, h->stream));
    HCHECK(h, hipStreamSynchronize(h->stream));
    if (cnt < 0 || cnt > W.n) {
      h->err = "wind source: device cell count out of range";
      return PION_GPU_EDEVICE;
    }
  }
  *n = cnt;
  if (!idx || cnt == 0) return 0;
  HCHECK(h, hipMemcpyAsync(idx, h->dws_idx + W.off, sizeof(long) * cnt, hipMemcpyDeviceToHost, h->stream));
  if (states)
    HCHECK(h, hipMemcpyAsync(states, h->dws_state + W.off * h->cfg.nvar, sizeof(double) * cnt * h->cfg.nvar,
                             hipMemcpyDeviceToHost, h->stream));
  HCHECK(h, hipStreamSynchronize(h->stream));
  return 0;
}

}  // extern "C"
