// pion_gpu.hip -- implementation of the C-ABI declared in include/pion_gpu.h.
//
// Owns device memory behind an opaque handle (pion_handle.h): set-up and tear-down, uploads and the on-grid pack
// kernels, cooling tables, the test seams and timing.  What a time step calls is pion_step.hip; the boundary update
// (ghost-cell fills, jet) is pion_bc.hip with the rules in dev_bc.h; the stellar-wind sources are pion_wind.hip and
// wind_host.cpp.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "pion_handle.h"

using namespace pion;
using namespace pion::impl;

int impl::order_after_unpack(Handle *h)
{
  if (h->comm_stream && h->comm_stream != h->stream && h->ev_unpacked_valid) {
    HCHECK(h, hipStreamWaitEvent(h->stream, h->ev_unpacked, 0));
    h->ev_unpacked_valid = false;
  }
  return 0;
}

long impl::cell_id(const GridDesc &g, int ix, int iy, int iz)
{
  return (long)(ix + g.nbc[0]) + g.sy * (iy + g.nbc[1]) + g.sz * (iz + g.nbc[2]);
}

void impl::time_begin(Handle *h, int slot)
{
  if (!h->timing || slot < 0) return;   // (slot -1: the test seams, which are not timed)
  hipEvent_t e;
  hipEventCreate(&e);
  hipEventRecord(e, h->stream);
  h->ev[slot].push_back(e);
}

FluxCtx impl::make_fluxctx(const Handle *h, double fv_dt)
{
  FluxCtx fc;
  fc.gamma = h->cfg.gamma;
  fc.dx = h->cfg.dx;
  fc.fv_dt = fv_dt;
  fc.etav = h->cfg.etav;
  fc.chyp = h->glm_chyp;
  fc.min_temp = h->cfg.min_temp;
  fc.refRO = h->refvec_avg[0];
  fc.refPG = h->refvec_avg[1];
  fc.refV = h->refvec_avg[2];
  fc.refB = h->refvec_avg[5];
  fc.gndim = h->cfg.ndim;
  fc.artvisc = h->cfg.artvisc;
  fc.mp.present = (h->cfg.cooling != 0);
  fc.mp.Mu_tot_over_kB = h->Mu_tot_over_kB;
  return fc;
}

int impl::check_errword(Handle *h)
{
  int e = 0;
  HCHECK(h, hipMemcpyAsync(&e, h->derr, sizeof(int), hipMemcpyDeviceToHost, h->stream));
  HCHECK(h, hipStreamSynchronize(h->stream));
  if (e) {
    char b[400];
    snprintf(b, sizeof b, "device physics error word 0x%x:%s%s%s%s%s", e,
             (e & ERR_NEG_DENSITY) ? " negative density (reference: rep.error -> exit)" : "",
             (e & ERR_RIEMANN_INPUT) ? " density/pressure too small in Riemann solver" : "",
             (e & ERR_COOLING) ? " cooling integration failed" : "", (e & ERR_BAD_DT) ? " invalid cell timestep" : "",
             (e & ERR_MHD_RIEMANN) ? " linear MHD Riemann solver: bad wave speeds (reference: rep.error -> exit)" : "");
    h->err = b;
    int z = 0;
    hipMemcpyAsync(h->derr, &z, sizeof(int), hipMemcpyHostToDevice, h->stream);
    return PION_GPU_EPHYSICS;
  }
  return 0;
}

namespace {

// On-grid cells of planes [plane_lo, plane_lo + planes) of the slab axis <-> a contiguous buffer
// [nvar][planes][rows][nx] (pion_gpu_pack_ongrid / _unpack_ongrid).  A plane of the slab axis is `rows` runs of nx
// on-grid cells (3-D: the ny rows of an x-y plane; 2-D: one row; 1-D: the one row there is).  A pure copy, bound by
// HBM: one lane per double, consecutive along x; a wavefront takes one stretch of up to ONGRID_SEG cells of one row,
// so the (64-bit) index arithmetic is paid once per stretch and the loads and stores are whole lines.  No LDS.
// blockIdx.y: the variable.  Every cell id and buffer index is 64-bit (grids of 2^29 cells and more).
constexpr int ONGRID_SEG = 1024, ONGRID_WAVES = 4;
struct OngridGeom {
  long off0;     // cell id of the first on-grid cell of plane 0
  long ps, rs;   // cell-id strides of a plane and of a row inside a plane
  long ncell;    // stride of a variable in the state arrays
  int nx, rows, nseg;   // nseg: stretches per row
};
template <bool PACK>
__global__ void __launch_bounds__(64 * ONGRID_WAVES)
k_pack_ongrid(double *__restrict__ A0, double *__restrict__ A1, double *__restrict__ buf, const OngridGeom q,
              const long plane_lo, const long planes)
{
  const long u = (long)blockIdx.x * ONGRID_WAVES + (threadIdx.x >> 6);   // stretch: (plane, row, segment)
  const long nunit = planes * q.rows * q.nseg;
  if (u >= nunit) return;
  const long row = u / q.nseg;
  const int seg = (int)(u - row * q.nseg);
  const long k = row / q.rows;
  const long j = row - k * q.rows;
  const long v = blockIdx.y;
  const long c0 = v * q.ncell + q.off0 + (plane_lo + k) * q.ps + j * q.rs;
  const long b0 = ((v * planes + k) * q.rows + j) * q.nx;
  const int x1 = min(q.nx, (seg + 1) * ONGRID_SEG);
  for (int ix = seg * ONGRID_SEG + (threadIdx.x & 63); ix < x1; ix += 64) {
    if (PACK) buf[b0 + ix] = A0[c0 + ix];
    else {
      const double x = buf[b0 + ix];
      A0[c0 + ix] = x;
      A1[c0 + ix] = x;
    }
  }
}

OngridGeom ongrid_geom(const Handle *h)
{
  const GridDesc &g = h->g;
  OngridGeom q;
  q.ncell = g.ncell;
  q.nx = g.ng[0];
  q.nseg = (q.nx + ONGRID_SEG - 1) / ONGRID_SEG;
  q.off0 = g.nbc[0];
  q.ps = q.rs = 0;
  q.rows = 1;
  if (g.ndim == 2) {
    q.off0 += g.sy * g.nbc[1];
    q.ps = g.sy;
  }
  else if (g.ndim == 3) {
    q.off0 += g.sy * g.nbc[1] + g.sz * g.nbc[2];
    q.ps = g.sz;
    q.rs = g.sy;
    q.rows = g.ng[1];
  }
  return q;
}
// planes of the slab axis (1-D: the one row)
inline int ongrid_planes(const Handle *h) { return h->g.ndim == 1 ? 1 : h->g.ng[h->g.ndim - 1]; }

int ongrid_go(Handle *h, double *A0, double *A1, int plane_lo, int plane_hi, void *dbuf, bool pack)
{
  if (!dbuf || plane_lo < 0 || plane_hi > ongrid_planes(h) || plane_lo >= plane_hi) {
    h->err = "pack / unpack_ongrid: plane range outside the grid, or no buffer";
    return PION_GPU_EINVAL;
  }
  const OngridGeom q = ongrid_geom(h);
  // the launch grid in long: one wavefront per stretch, ONGRID_WAVES per block.  (2^31 blocks are 2^33 stretches:
  // no grid that fits a card comes near; a range that did would have to be passed in parts.)
  const long planes = plane_hi - plane_lo;
  const long nblk = (planes * q.rows * q.nseg + ONGRID_WAVES - 1) / ONGRID_WAVES;
  if (nblk > (1L << 31) - 1) {
    h->err = "pack / unpack_ongrid: plane range too large for one launch; pass it in parts";
    return PION_GPU_EINVAL;
  }
  const dim3 grid((unsigned)nblk, (unsigned)h->cfg.nvar), block(64 * ONGRID_WAVES);
  if (pack) hipLaunchKernelGGL(k_pack_ongrid<true>, grid, block, 0, h->stream, A0, A1, (double *)dbuf, q, (long)plane_lo, planes);
  else hipLaunchKernelGGL(k_pack_ongrid<false>, grid, block, 0, h->stream, A0, A1, (double *)dbuf, q, (long)plane_lo, planes);
  HCHECK(h, hipGetLastError());
  return 0;
}

}  // namespace

extern "C" {

int pion_gpu_create(const pion_gpu_config *cfg, int device, void **handle)
{
  if (!cfg || !handle) return PION_GPU_EINVAL;
  if (cfg->ndim < 1 || cfg->ndim > 3 || cfg->nvar > PION_MAX_NVAR) return PION_GPU_EINVAL;
  // Cartesian, or cylindrical (z,R) axisymmetry in 2-D (the only cylindrical case the reference's solver
  // classes accept: solver_eqn_hydro_adi.cpp:540-545, solver_eqn_mhd_adi.cpp:985-990)
  // or spherical symmetry in 1-D, hydro only (sph_FV_solver_Hydro_Euler, solver_eqn_hydro_adi.cpp:620-640)
  if (!(cfg->coord_sys == 1 || (cfg->coord_sys == 2 && cfg->ndim == 2)
        || (cfg->coord_sys == 3 && cfg->ndim == 1 && cfg->eqntype == PION_EQEUL)))
    return PION_GPU_EINVAL;
  for (int d = 0; d < 2 * cfg->ndim; d++)
    if (cfg->bc_type[d] == PION_BC_AXISYMMETRIC && !(cfg->coord_sys == 2 && d == 2)) return PION_GPU_EINVAL;
  // a face owned by a neighbouring GPU: the two faces of the slab axis (the last axis) of a 3-D or 2-D grid only
  for (int d = 0; d < 2 * cfg->ndim; d++)
    if (cfg->bc_type[d] == PION_BC_SLAB && !(cfg->ndim >= 2 && d / 2 == cfg->ndim - 1)) return PION_GPU_EINVAL;
  const int base = (cfg->eqntype == PION_EQEUL) ? 5 : (cfg->eqntype == PION_EQMHD ? 8 : (cfg->eqntype == PION_EQGLM ? 9 : -1));
  if (base < 0 || cfg->nvar != base + cfg->ntracer || cfg->ntracer > PION_MAX_NTR) return PION_GPU_EINVAL;
  if (cfg->sp_ooa == 2 && cfg->nbc < 2) return PION_GPU_EINVAL;
  if (cfg->nbc < 1) return PION_GPU_EINVAL;
  if (cfg->eqntype == PION_EQEUL) {
    if (cfg->solver == 7 || cfg->solver < 0 || cfg->solver > 8) return PION_GPU_EINVAL;
  }
  // MHD: LF, FKJ98 linear, Roe, HLLD, HLL (exact/hybrid are fatal in riemannMHD.cpp:176-181)
  else if (!(cfg->solver == 0 || cfg->solver == 1 || cfg->solver == 4 || cfg->solver == 7 || cfg->solver == 8))
    return PION_GPU_EINVAL;
  // mp_only_cooling's cooling functions (mp_only_cooling.cpp:93-115): 3 (DMcC) has no case in Edot (:377-415) and stops there
  if (cfg->cooling != PION_COOL_NONE && cfg->cooling != PION_COOL_KI02
      && !(cfg->cooling >= PION_COOL_SD93_CIE && cfg->cooling <= PION_COOL_WSS09_CIE_LINE_HEAT_COOL))
    return PION_GPU_EINVAL;
  if (cfg->mp_timestep_limit < 0 || cfg->mp_timestep_limit > 4) return PION_GPU_EINVAL;  // calc_timestep.cpp:457

  Handle *h = new Handle;
  h->cfg = *cfg;
  if (const char *e = getenv("PION_STAGE_KERNEL"))
    h->use_march = (strcmp(e, "cell") == 0) ? 0 : 3;
  if (const char *e = getenv("PION_ZSLOPE_LDS")) h->zslope_lds = (atoi(e) != 0);
  if (const char *e = getenv("PION_CONCURRENT_STRIPS")) h->concurrent_strips = (atoi(e) != 0);
  if (const char *e = getenv("PION_FUSE_DT")) h->fuse_dt = (atoi(e) != 0);
  if (const char *e = getenv("PION_FUSE_BC")) h->fuse_bc = (atoi(e) != 0);
  if (const char *e = getenv("PION_UNEVEN_CHUNKS")) h->uneven_chunks = (atoi(e) != 0);
  if (const char *e = getenv("PION_HLL_SCREEN")) h->hll_screen = (atoi(e) != 0);
  if (const char *e = getenv("PION_SPLIT_DT_MP")) h->split_dt_mp = (atoi(e) != 0);
  if (const char *e = getenv("PION_ROWS")) h->rows = h->rows1 = (atoi(e) >= 1 && atoi(e) <= 64) ? atoi(e) : 0;
  if (const char *e = getenv("PION_ROWS1")) h->rows1 = (atoi(e) >= 1 && atoi(e) <= 8) ? atoi(e) : 0;
  if (const char *e = getenv("PION_ZCHUNK")) h->zchunk = atoi(e) > 0 ? atoi(e) : 0;
  h->device = device;
  if (hipSetDevice(device) != hipSuccess) {
    delete h;
    return PION_GPU_EDEVICE;
  }
  {
    int ncu = 0;
    if (hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, device) == hipSuccess) h->ncu = ncu;
  }
  GridDesc &g = h->g;
  g.ndim = cfg->ndim;
  g.ncell = 1;
  for (int a = 0; a < 3; a++) {
    g.ng[a] = (a < cfg->ndim) ? cfg->ng[a] : 1;
    g.nbc[a] = (a < cfg->ndim) ? cfg->nbc : 0;
    g.nga[a] = g.ng[a] + 2 * g.nbc[a];
    g.ncell *= g.nga[a];
    g.xmin[a] = cfg->xmin[a];
  }
  g.sy = g.nga[0];
  g.sz = (long)g.nga[0] * g.nga[1];
  g.dx = cfg->dx;
  g.cyl = (cfg->coord_sys == 2) ? 1 : ((cfg->coord_sys == 3) ? 2 : 0);
  g.sph_vol = nullptr;
  *handle = h;
  // k_stage_rows2 (3-D, two ghost layers) addresses every array as "uniform base + 32-bit byte offset of the
  // cell": one launch reaches fewer than 2^29 cells (ghosts included) of an array.  A larger grid runs it in plane
  // windows, one launch per window with the arrays' bases advanced on the host (rows_tiling.h, "plane windows";
  // stage_launch, pion_step.hip); a grid whose single plane with its ghost planes exceeds the limit, and with
  // PION_ROWS_WINDOWS=0 every grid of 2^29 cells or more, uses the cell-per-thread kernel with 64-bit addresses
  // (2-D grids run the rows kernel without the z part; PION_ROWS_2D=0 puts them back on the cell-per-thread kernel)
  const bool rows3d = (g.ndim == 3 && g.nbc[2] >= 2);
  bool rows2d = (g.ndim == 2 && g.cyl != 2 && g.nbc[1] >= 2 && g.nbc[0] >= 2);   // (cyl == 1: the CYL instance)
  if (const char *e = getenv("PION_ROWS_2D")) rows2d = rows2d && (atoi(e) != 0);
  bool windows = true;
  if (const char *e = getenv("PION_ROWS_WINDOWS")) windows = (atoi(e) != 0);
  if (const char *e = getenv("PION_ROWS_WINDOW_CELLS")) {
    const long v = atol(e);
    if (windows && v >= 1 && v <= PION_ROWS_WINDOW_CELLS) h->win_cells = v;   // (never more than the offsets can reach)
  }
  if (rows3d || rows2d) {
    const int sa = g.ndim - 1;
    h->win_whole = windows ? rows_windows_count(0, g.ng[sa], (sa == 2) ? g.sz : g.sy, g.nbc[sa], h->win_cells)
                           : (g.ncell < PION_ROWS_WINDOW_CELLS ? 1 : 0);
  }
  if (h->win_whole < 1) h->use_march = 0;
  if (h->use_march == 0) h->win_whole = 0;

  const size_t nb = sizeof(double) * (size_t)cfg->nvar * g.ncell;
  HCHECK(h, hipMalloc(&h->dP, nb));
  HCHECK(h, hipMalloc(&h->dPh, nb));
  HCHECK(h, hipMemset(h->dP, 0, nb));
  HCHECK(h, hipMemset(h->dPh, 0, nb));
  HCHECK(h, hipMalloc(&h->dflags, g.ncell));
  if (g.cyl == 2) {
    // VectorOps_Sph::DivStateVectorComponent: rc = (pow(rp,3.0) - pow(rn,3.0))/3.0 with the host's libm
    std::vector<double> vol(g.nga[0]);
    for (int i = 0; i < g.nga[0]; i++) {
      double rc = g.xmin[0] + (2 * (i - g.nbc[0]) + 1) * (0.5 * g.dx);
      const double rp = rc + 0.5 * g.dx;
      const double rn = rp - g.dx;
      vol[i] = (pow(rp, 3.0) - pow(rn, 3.0)) / 3.0;
    }
    HCHECK(h, hipMalloc(&h->dsphvol, sizeof(double) * vol.size()));
    HCHECK(h, hipMemcpy(h->dsphvol, vol.data(), sizeof(double) * vol.size(), hipMemcpyHostToDevice));
    g.sph_vol = h->dsphvol;
  }
  HCHECK(h, hipMalloc(&h->derr, 64));
  HCHECK(h, hipMemset(h->derr, 0, 64));
  HCHECK(h, hipMalloc(&h->ddt, 2 * sizeof(unsigned long long)));
  HCHECK(h, hipMalloc(&h->ddt_init, 2 * sizeof(unsigned long long)));
  {
    const double init[2] = {1.e100, 1.0e99};
    HCHECK(h, hipMemcpy(h->ddt_init, init, sizeof init, hipMemcpyHostToDevice));
  }
  if (cfg->eqntype != PION_EQEUL && cfg->solver == PION_FLUX_RS_HLLD) {
    HCHECK(h, hipMalloc(&h->dhll, g.ncell));
    HCHECK(h, hipMemset(h->dhll, 0, g.ncell));
  }
  if (cfg->cooling != 0) {
    HCHECK(h, hipMalloc(&h->ddE, sizeof(double) * g.ncell));
    HCHECK(h, hipMemset(h->ddE, 0, sizeof(double) * g.ncell));
  }
  if (cfg->artvisc == PION_AV_HCORRECTION || cfg->artvisc == PION_AV_HCORR_FKJ98) {
    HCHECK(h, hipMalloc(&h->deta, sizeof(double) * cfg->ndim * g.ncell));
    HCHECK(h, hipMemset(h->deta, 0, sizeof(double) * cfg->ndim * g.ncell));
  }

  // cell flags (uniform_grid.cpp:343-356,516-546; periodic ghosts are isdomain,
  // periodic_boundaries.cpp:35-36; everything else off-grid is not)
  h->hflags.assign(g.ncell, 0);
  for (long c = 0; c < g.ncell; c++) {
    int i[3];
    i[0] = (int)(c % g.nga[0]) - g.nbc[0];
    i[1] = (int)((c / g.nga[0]) % g.nga[1]) - g.nbc[1];
    i[2] = (int)(c / g.sz) - g.nbc[2];
    bool on = true;
    bool all_periodic_offgrid = true;
    for (int a = 0; a < cfg->ndim; a++) {
      if (i[a] < 0) {
        on = false;
        if (cfg->bc_type[2 * a] != PION_BC_PERIODIC) all_periodic_offgrid = false;
      }
      else if (i[a] >= g.ng[a]) {
        on = false;
        if (cfg->bc_type[2 * a + 1] != PION_BC_PERIODIC) all_periodic_offgrid = false;
      }
    }
    uint8_t f = PION_CELL_ISLEAF | PION_CELL_TIMESTEP;
    if (on) f |= PION_CELL_ISGD | PION_CELL_ISDOMAIN;
    else {
      f |= PION_CELL_ISBD;
      (void)all_periodic_offgrid;  // ghost isdomain never matters on the device: ghosts are not updated
    }
    h->hflags[c] = f;
  }
  HCHECK(h, hipMemcpy(h->dflags, h->hflags.data(), g.ncell, hipMemcpyHostToDevice));

  // microphysics constants (mp_only_cooling.cpp:81-95,140-146; constants.h:53,64)
  const double m_p = 1.672621898e-24, kB = 1.38064852e-16;
  const double Mu = 1.40 * m_p, Mu_tot = 0.609 * m_p, Mu_elec = 1.167 * m_p, Mu_ion = 1.273 * m_p;
  h->Mu_tot_over_kB = Mu_tot / kB;
  memset(&h->cool, 0, sizeof h->cool);
  h->cool.inv_Mu2 = 1.0 / (Mu * Mu);
  h->cool.inv_Mu2_elec_H = 1.0 / (Mu_elec * Mu);
  h->cool.Mu_tot_over_kB = h->Mu_tot_over_kB;
  h->cool.MinT_allowed = cfg->min_temp;
  h->cool.MaxT_allowed = cfg->max_temp;
  if (h->cool.MinT_allowed < 1.0 || h->cool.MinT_allowed > 1.0e6) h->cool.MinT_allowed = 1.0;
  if (h->cool.MaxT_allowed < 1.0e2 || h->cool.MaxT_allowed > 3.0e10) h->cool.MaxT_allowed = 1.0e8;
  memset(&h->form, 0, sizeof h->form);
  h->form.flag = cfg->cooling;
  h->form.Mu = Mu;
  h->form.Mu_elec = Mu_elec;
  h->form.Mu_ion = Mu_ion;
  h->form.Mu_tot_over_kB = h->Mu_tot_over_kB;
  h->form.MinT_allowed = h->cool.MinT_allowed;
  h->form.MaxT_allowed = h->cool.MaxT_allowed;

  // eq_refvec after SetAvgState (eqns_hydro_adiabatic.cpp:437-453); only the Euler Riemann
  // solvers (riemann.cpp) read it
  for (int v = 0; v < PION_MAX_NVAR; v++) h->refvec_avg[v] = cfg->refvec[v];
  if (cfg->eqntype == PION_EQEUL) {
    const double refvel = sqrt(cfg->gamma * cfg->refvec[1] / cfg->refvec[0]);
    h->refvec_avg[2] = h->refvec_avg[3] = h->refvec_avg[4] = 0.1 * refvel;
  }
  else {
    // eqns_mhd_ideal::SetAvgState (eqns_mhd_adiabatic.cpp:501-544): fast speed of the reference
    // state with the field rotated into the x-y plane's x axis; velocities <- 0.1 c_f, fields <- |B|
    double *rv = h->refvec_avg;
    const double gam = cfg->gamma;
    auto cfast = [&](const double *p) {
      const double ch = sqrt(gam * p[1] / p[0]);
      const double t1 = ch * ch + (p[5] * p[5] + p[6] * p[6] + p[7] * p[7]) / p[0];
      double t2 = 4. * ch * ch * p[5] * p[5] / p[0];
      t2 = std::max(5.e-16, t1 * t1 - t2);
      return sqrt((t1 + sqrt(t2)) / 2.);
    };
    auto rotate_xy = [&](double *v, double theta) {
      const double ct = cos(theta), st = sin(theta);
      double a = v[2] * ct - v[3] * st, b = v[2] * st + v[3] * ct;
      v[2] = a;
      v[3] = b;
      a = v[5] * ct - v[6] * st;
      b = v[5] * st + v[6] * ct;
      v[5] = a;
      v[6] = b;
    };
    double angle = rv[6] * rv[6] + rv[5] * rv[5], refvel;
    if (angle > 10. * 5.e-16) {
      angle = M_PI / 2. - asin(rv[6] / sqrt(angle));
      if (rv[5] < 0) angle = -angle;
      rotate_xy(rv, angle);
      refvel = cfast(rv);
      rotate_xy(rv, -angle);
    }
    else refvel = cfast(rv);
    const double refB = sqrt(rv[5] * rv[5] + rv[6] * rv[6] + rv[7] * rv[7]);
    rv[2] = rv[3] = rv[4] = 0.1 * refvel;
    rv[5] = rv[6] = rv[7] = refB;
  }
  bc_init(h);
  return PION_GPU_OK;
}

void pion_gpu_destroy(void *handle)
{
  Handle *h = use(handle);
  if (!h) return;
  hipSetDevice(h->device);
  hipDeviceSynchronize();
  if (h->own_state) {
    hipFree(h->dP);
    hipFree(h->dPh);
  }
  hipFree(h->dflags);
  hipFree(h->dhll);
  hipFree(h->dsum);
  hipFree(h->dscr_list);
  hipFree(h->dscr_count);
  hipFree(h->ddE);
  hipFree(h->dfits_bad);
  hipFree(h->dangle_vals);
  hipFree(h->dangle_capped);
  if (h->bstream) hipStreamDestroy(h->bstream);
  if (h->ev_pre) hipEventDestroy(h->ev_pre);
  if (h->ev_bdone) hipEventDestroy(h->ev_bdone);
  if (h->hdt) hipHostFree(h->hdt);
  if (h->ev_dt) hipEventDestroy(h->ev_dt);
  hipFree(h->deta);
  hipFree(h->dsphvol);
  hipFree(h->derr);
  hipFree(h->ddt);
  hipFree(h->ddt_init);
  wind_free(h);
  rt_free(h);
  hipFree(h->djet_idx);
  hipFree(h->djet_state);
  hipFree(h->dcoolT);
  hipFree(h->dcooltab);
  hipFree(h->dcoolslope);
  hipFree(h->dcurve);
  for (int s = 0; s < 4; s++)
    for (hipEvent_t e : h->ev[s]) hipEventDestroy(e);
  if (h->ev_packed_src) hipEventDestroy(h->ev_packed_src);
  if (h->ev_unpacked) hipEventDestroy(h->ev_unpacked);
  delete h;
}

int pion_gpu_last_error(void *handle, char *buf, int len)
{
  Handle *h = use(handle);
  if (!h || !buf || len <= 0) return PION_GPU_EINVAL;
  snprintf(buf, len, "%s", h->err.c_str());
  return 0;
}

long pion_gpu_ncell_all(void *handle) { return ((Handle *)handle)->g.ncell; }
int pion_gpu_ng_all(void *handle, int axis) { return ((Handle *)handle)->g.nga[axis]; }

int pion_gpu_upload(void *handle, const double *P_soa)
{
  Handle *h = use(handle);
  h->xghost_fresh = nullptr;
  const size_t nb = sizeof(double) * (size_t)h->cfg.nvar * h->g.ncell;
  HCHECK(h, hipMemcpyAsync(h->dP, P_soa, nb, hipMemcpyHostToDevice, h->stream));
  HCHECK(h, hipMemcpyAsync(h->dPh, h->dP, nb, hipMemcpyDeviceToDevice, h->stream));
  HCHECK(h, hipStreamSynchronize(h->stream));
  h->ph_valid = false;
  state_changed(h);
  h->dt_requested = false;   // a read-back requested for the previous state is void
  h->dt_mp_pending = false;
  return 0;
}

int pion_gpu_download(void *handle, int which, double *P_soa)
{
  Handle *h = use(handle);
  const size_t nb = sizeof(double) * (size_t)h->cfg.nvar * h->g.ncell;
  // after a full step the reference has Ph == P everywhere (time_integrator.cpp:938-939)
  const double *src = (which == 1 && h->ph_valid) ? h->dPh : h->dP;
  if (int rc = order_after_unpack(h)) return rc;
  HCHECK(h, hipMemcpyAsync(P_soa, src, nb, hipMemcpyDeviceToHost, h->stream));
  HCHECK(h, hipStreamSynchronize(h->stream));
  return check_errword(h);
}

long pion_gpu_ongrid_count(void *handle, int planes)
{
  Handle *h = use(handle);
  if (!h || planes < 0) return 0;
  const OngridGeom q = ongrid_geom(h);
  return (long)h->cfg.nvar * planes * q.rows * q.nx;
}

int pion_gpu_pack_ongrid(void *handle, int which, int plane_lo, int plane_hi, void *dbuf)
{
  Handle *h = use(handle);
  if (!h) return PION_GPU_EINVAL;
  // the array pion_gpu_download(which) reads
  double *src = (which == 1 && h->ph_valid) ? h->dPh : h->dP;
  if (int rc = order_after_unpack(h)) return rc;
  return ongrid_go(h, src, nullptr, plane_lo, plane_hi, dbuf, true);
}

int pion_gpu_unpack_ongrid(void *handle, int plane_lo, int plane_hi, void *dbuf)
{
  Handle *h = use(handle);
  if (!h) return PION_GPU_EINVAL;
  if (int rc = order_after_unpack(h)) return rc;
  if (int rc = ongrid_go(h, h->dP, h->dPh, plane_lo, plane_hi, dbuf, false)) return rc;
  // what pion_gpu_upload invalidates
  h->xghost_fresh = nullptr;
  h->ph_valid = false;
  state_changed(h);
  h->dt_requested = false;
  h->dt_mp_pending = false;
  return 0;
}

int pion_gpu_bind_device_state(void *handle, void *dP, void *dPh)
{
  Handle *h = use(handle);
  h->xghost_fresh = nullptr;
  if (!dP || !dPh) return PION_GPU_EINVAL;
  if (h->own_state) {
    hipFree(h->dP);
    hipFree(h->dPh);
  }
  h->own_state = false;
  h->dP = (double *)dP;
  h->dPh = (double *)dPh;
  h->ph_valid = false;
  state_changed(h);
  h->dt_requested = false;
  return 0;
}
void *pion_gpu_device_ptr(void *handle, int which)
{
  Handle *h = use(handle);
  h->xghost_fresh = nullptr;
  state_changed(h);  // the caller may write through the pointer
  return which == 0 ? (void *)h->dP : (void *)h->dPh;
}
int pion_gpu_set_stream(void *handle, void *stream)
{
  ((Handle *)handle)->stream = (hipStream_t)stream;
  return 0;
}
int pion_gpu_set_comm_stream(void *handle, void *stream)
{
  Handle *h = use(handle);
  h->comm_stream = (hipStream_t)stream;
  h->ev_unpacked_valid = false;
  return 0;
}
int pion_gpu_synchronize(void *handle)
{
  Handle *h = use(handle);
  HCHECK(h, hipStreamSynchronize(h->stream));
  if (h->comm_stream && h->comm_stream != h->stream) HCHECK(h, hipStreamSynchronize(h->comm_stream));
  if (h->bstream) HCHECK(h, hipStreamSynchronize(h->bstream));
  return 0;
}

int pion_gpu_get_flags(void *handle, unsigned char *out)
{
  Handle *h = use(handle);
  if (!h || !out) return PION_GPU_EINVAL;
  HCHECK(h, hipMemcpyAsync(out, h->dflags, h->g.ncell, hipMemcpyDeviceToHost, h->stream));
  HCHECK(h, hipStreamSynchronize(h->stream));
  return 0;
}

int pion_gpu_get_hll_switch(void *handle, unsigned char *out)
{
  Handle *h = use(handle);
  if (!h || !out || !h->dhll) return PION_GPU_EINVAL;
  HCHECK(h, hipMemcpyAsync(out, h->dhll, h->g.ncell, hipMemcpyDeviceToHost, h->stream));
  HCHECK(h, hipStreamSynchronize(h->stream));
  return 0;
}

int pion_gpu_get_hcorr_eta(void *handle, int axis, double *out)
{
  Handle *h = use(handle);
  if (!h || !out || !h->deta || axis < 0 || axis >= h->g.ndim) return PION_GPU_EINVAL;
  HCHECK(h, hipMemcpyAsync(out, h->deta + (size_t)axis * h->g.ncell, sizeof(double) * h->g.ncell, hipMemcpyDeviceToHost,
                           h->stream));
  HCHECK(h, hipStreamSynchronize(h->stream));
  return 0;
}

int pion_gpu_get_hll_screen_counts(void *handle, int *active, int *total)
{
  Handle *h = use(handle);
  if (!h || !active || !total) return PION_GPU_EINVAL;
  *active = -1;
  *total = 0;
  if (!h->last_prepass_screened) return 0;
  HCHECK(h, hipMemcpyAsync(active, h->dscr_count, sizeof(int), hipMemcpyDeviceToHost, h->stream));
  HCHECK(h, hipStreamSynchronize(h->stream));
  *total = (int)scr_total(h->scr);
  return 0;
}

int pion_gpu_set_cooling_tables(void *handle, int nT, const double *T, const double *tabs, const double *slopes)
{
  Handle *h = use(handle);
  state_changed(h);   // t_mp depends on the tables
  if (nT < 2 || nT > PION_COOL_NT_MAX) {
    // (k_cooling_dE keeps the tables in LDS: 11 x PION_COOL_NT_MAX doubles; mp_only_cooling builds 200 points)
    h->err = "cooling tables: 2 <= nT <= 256 required";
    return PION_GPU_EINVAL;
  }
  hipFree(h->dcoolT);
  hipFree(h->dcooltab);
  hipFree(h->dcoolslope);
  HCHECK(h, hipMalloc(&h->dcoolT, sizeof(double) * nT));
  HCHECK(h, hipMalloc(&h->dcooltab, sizeof(double) * 5 * nT));
  HCHECK(h, hipMalloc(&h->dcoolslope, sizeof(double) * 5 * nT));
  HCHECK(h, hipMemcpy(h->dcoolT, T, sizeof(double) * nT, hipMemcpyHostToDevice));
  HCHECK(h, hipMemcpy(h->dcooltab, tabs, sizeof(double) * 5 * nT, hipMemcpyHostToDevice));
  HCHECK(h, hipMemcpy(h->dcoolslope, slopes, sizeof(double) * 5 * nT, hipMemcpyHostToDevice));
  // log-spaced grid?  (mp_only_cooling's is: T_i = 10^(log10 Tmin + i dlogT), mp_only_cooling.cpp:533-537.)  Then the
  // device finds the table interval from a single-precision logarithm instead of bisecting; the guess only has to
  // land within a few entries of the truth -- it is corrected against the table -- so a loose check suffices.
  h->cool.lg0 = 0.0f;
  h->cool.inv_dlg = 0.0f;
  if (T[0] > 0.0 && T[nT - 1] > T[0]) {
    const double l0 = log2(T[0]), inv = (nT - 1) / (log2(T[nT - 1]) - l0);
    bool ok = true;
    for (int i = 0; i < nT && ok; i++) {
      if (!(T[i] > 0.0) || (i > 0 && !(T[i] > T[i - 1]))) ok = false;
      else if (fabs((log2(T[i]) - l0) * inv - i) > 0.25) ok = false;
    }
    if (ok) {
      h->cool.lg0 = (float)l0;
      h->cool.inv_dlg = (float)inv;
    }
  }
  if (const char *e = getenv("PION_COOL_BISECT")) {
    if (atoi(e) != 0) h->cool.inv_dlg = 0.0f;   // A/B and cross-check: the reference's bisection
  }
  h->cool.NT = nT;
  h->cool.T = h->dcoolT;
  h->cool.tab = h->dcooltab;
  h->cool.slope = h->dcoolslope;
  h->have_tables = true;
  return 0;
}

int pion_gpu_set_cooling_curve(void *handle, int n, const double *logT, const double *logL, const double *c,
                               double min_slope, double max_slope)
{
  Handle *h = use(handle);
  if (!h) return PION_GPU_EINVAL;
  state_changed(h);   // t_mp depends on the curve
  if (n < 2 || n > PION_COOL_NT_MAX || !logT || !logL || !c) {
    // (the cooling kernels keep the curve in LDS: 3 x PION_COOL_NT_MAX doubles)
    h->err = "cooling curve: 2 <= n <= 256 knots required";
    return PION_GPU_EINVAL;
  }
  bool ok = std::isfinite(min_slope) && std::isfinite(max_slope);
  for (int i = 0; i < n && ok; i++)
    ok = std::isfinite(logT[i]) && std::isfinite(logL[i]) && std::isfinite(c[i]) && (i == 0 || logT[i] > logT[i - 1]);
  if (!ok) {
    h->err = "cooling curve: knots must be finite and strictly increasing in log10 T, slopes finite";
    return PION_GPU_EINVAL;
  }
  std::vector<double> buf(3 * (size_t)n);
  for (int i = 0; i < n; i++) {
    buf[i] = logT[i];
    buf[n + i] = logL[i];
    buf[2 * n + i] = c[i];
  }
  h->have_curve = false;
  hipFree(h->dcurve);
  h->dcurve = nullptr;
  HCHECK(h, hipMalloc(&h->dcurve, sizeof(double) * buf.size()));
  HCHECK(h, hipMemcpy(h->dcurve, buf.data(), sizeof(double) * buf.size(), hipMemcpyHostToDevice));
  // uniformly spaced knots?  Then the device guesses the interval from the spacing; the guess is corrected against
  // the knots, so it only has to land near the truth.
  h->form.inv_dx = 0.0;
  {
    const double inv = (n - 1) / (logT[n - 1] - logT[0]);
    bool uni = std::isfinite(inv) && inv > 0.0;
    for (int i = 0; i < n && uni; i++) uni = fabs((logT[i] - logT[0]) * inv - i) <= 0.25;
    if (uni) h->form.inv_dx = inv;
  }
  if (const char *e = getenv("PION_COOL_BISECT")) {
    if (atoi(e) != 0) h->form.inv_dx = 0.0;   // A/B and cross-check: always bisect
  }
  h->form.n = n;
  h->form.x = h->dcurve;
  h->form.y = h->dcurve + n;
  h->form.c = h->dcurve + 2 * n;
  h->form.min_slope = min_slope;
  h->form.max_slope = max_slope;
  h->have_curve = true;
  return 0;
}

void *pion_gpu_get_stream(void *handle, int which)
{
  Handle *h = use(handle);
  return (void *)(which == 0 ? h->stream : (h->comm_stream ? h->comm_stream : h->stream));
}

int pion_gpu_interface_flux(void *handle, int n, int axis, double dt, const double *Pl, const double *Pr,
                            const double *aux, double *F, double *Pstar)
{
  Handle *h = use(handle);
  const int nv = h->cfg.nvar;
  DevBuf<double> bl, br, ba, bf, bp;
  const size_t nb = sizeof(double) * (size_t)n * nv;
  HCHECK(h, hipMalloc(&bl.p, nb));
  HCHECK(h, hipMalloc(&br.p, nb));
  HCHECK(h, hipMalloc(&bf.p, nb));
  HCHECK(h, hipMalloc(&bp.p, nb));
  HCHECK(h, hipMalloc(&ba.p, sizeof(double) * 4 * n));
  double *dl = bl.p, *dr = br.p, *da = ba.p, *df = bf.p, *dp = bp.p;
  HCHECK(h, hipMemcpy(dl, Pl, nb, hipMemcpyHostToDevice));
  HCHECK(h, hipMemcpy(dr, Pr, nb, hipMemcpyHostToDevice));
  HCHECK(h, hipMemcpy(da, aux, sizeof(double) * 4 * n, hipMemcpyHostToDevice));
  FluxTestArgs a;
  a.n = n;
  a.axis = axis;
  a.eqntype = h->cfg.eqntype;
  a.ntracer = h->cfg.ntracer;
  a.solver = h->cfg.solver;
  a.Pl = dl;
  a.Pr = dr;
  a.aux = da;
  a.F = df;
  a.Pstar = dp;
  a.errword = h->derr;
  a.fc = make_fluxctx(h, dt);
  if (int rc = fp_launch(h, -1, "interface-flux launch failed", fp_strict::launch_flux_test, fp_fast::launch_flux_test, a,
                         h->stream))
    return rc;
  HCHECK(h, hipStreamSynchronize(h->stream));
  HCHECK(h, hipMemcpy(F, df, nb, hipMemcpyDeviceToHost));
  HCHECK(h, hipMemcpy(Pstar, dp, nb, hipMemcpyDeviceToHost));
  // the physics error word is informational here (tests feed extreme states)
  int z = 0;
  hipMemcpy(h->derr, &z, sizeof(int), hipMemcpyHostToDevice);
  return 0;
}

int pion_gpu_cell_advance(void *handle, int n, double fv_dt, const double *P_in, const double *dU, double *P_out,
                          double *dt_out)
{
  Handle *h = use(handle);
  if (!h) return PION_GPU_EINVAL;
  if (n <= 0 || !P_in || (dU == nullptr) != (P_out == nullptr) || (!dU && !dt_out)) {
    h->err = "cell_advance: n > 0, P_in, and dU with P_out and / or dt_out required";
    return PION_GPU_EINVAL;
  }
  DevBuf<double> bp, bu, bo, bt;
  const size_t nb = sizeof(double) * (size_t)n * h->cfg.nvar;
  CellTestArgs a{};
  // fc, glm_damp, max_temp, cfl and the error word exactly as a full second-order stage of dt = fv_dt gets them
  stage_physics(h, StageStep{fv_dt, h->cfg.sp_ooa, 1}, a.st);
  a.n = n;
  a.eqntype = h->cfg.eqntype;
  a.ntracer = h->cfg.ntracer;
  HCHECK(h, hipMalloc(&bp.p, nb));
  HCHECK(h, hipMemcpy(bp.p, P_in, nb, hipMemcpyHostToDevice));
  a.Pin = bp.p;
  if (dU) {
    HCHECK(h, hipMalloc(&bu.p, nb));
    HCHECK(h, hipMalloc(&bo.p, nb));
    HCHECK(h, hipMemcpy(bu.p, dU, nb, hipMemcpyHostToDevice));
    a.dU = bu.p;
    a.Pout = bo.p;
  }
  if (dt_out) {
    HCHECK(h, hipMalloc(&bt.p, sizeof(double) * (size_t)n));
    a.dt = bt.p;
  }
  if (int rc = fp_launch(h, -1, "cell-update launch failed", fp_strict::launch_cell_test, fp_fast::launch_cell_test, a,
                         h->stream))
    return rc;
  HCHECK(h, hipStreamSynchronize(h->stream));
  if (dU) HCHECK(h, hipMemcpy(P_out, bo.p, nb, hipMemcpyDeviceToHost));
  if (dt_out) HCHECK(h, hipMemcpy(dt_out, bt.p, sizeof(double) * (size_t)n, hipMemcpyDeviceToHost));
  return check_errword(h);
}

static int cool_go(Handle *h, int n, double dt, const double *Pin, double *Pout, const double *rho, const double *T,
                   double *edot)
{
  const bool form = cool_is_form(h->cfg);
  if (const char *m = form ? cool_missing(h) : (h->have_tables ? nullptr : "cooling tables not set")) {
    h->err = m;
    return PION_GPU_EINVAL;
  }
  CoolTestArgs a;
  memset(&a, 0, sizeof a);
  a.n = n;
  a.nvar = h->cfg.nvar;
  a.dt = dt;
  a.gamma = h->cfg.gamma;
  a.errword = h->derr;
  a.cool = h->cool;
  // TimeUpdateMP (Pin -> Pout), the cooling time of each state (Pin -> edot) or Edot (rho, T -> edot); edot: n doubles
  const int what = !Pin ? 1 : (edot ? 2 : 0);
  DevBuf<double> b0, b1, b2;
  const size_t nb = sizeof(double) * (size_t)n * (Pin ? a.nvar : 1), ne = sizeof(double) * (size_t)n;
  HCHECK(h, hipMalloc(&b0.p, nb));
  HCHECK(h, hipMalloc(&b1.p, nb));
  HCHECK(h, hipMalloc(&b2.p, ne));
  HCHECK(h, hipMemcpy(b0.p, Pin ? Pin : rho, nb, hipMemcpyHostToDevice));
  if (!Pin) HCHECK(h, hipMemcpy(b1.p, T, nb, hipMemcpyHostToDevice));
  a.Pin = Pin ? b0.p : nullptr;
  a.Pout = Pin ? b1.p : nullptr;
  a.rho = Pin ? nullptr : b0.p;
  a.T = Pin ? nullptr : b1.p;
  a.edot = b2.p;
  const int rc = fp_launch(h, -1, "cooling seam launch failed", fp_strict::launch_cool, fp_fast::launch_cool, a, h->form,
                           what, h->stream);
  HCHECK(h, hipStreamSynchronize(h->stream));
  if (what == 0) HCHECK(h, hipMemcpy(Pout, b1.p, nb, hipMemcpyDeviceToHost));
  else HCHECK(h, hipMemcpy(edot, b2.p, ne, hipMemcpyDeviceToHost));
  if (rc != 0) return rc;
  return check_errword(h);
}
int pion_gpu_cooling_update(void *handle, int n, double dt, const double *P_in, double *P_out)
{
  return cool_go(use(handle), n, dt, P_in, P_out, nullptr, nullptr, nullptr);
}
int pion_gpu_cooling_edot(void *handle, int n, const double *rho, const double *T, double *edot)
{
  return cool_go(use(handle), n, 0.0, nullptr, nullptr, rho, T, edot);
}
int pion_gpu_cooling_timescale(void *handle, int n, const double *P_in, double *t_cool)
{
  return cool_go(use(handle), n, 0.0, P_in, nullptr, nullptr, nullptr, t_cool);
}

int pion_gpu_cooling_curve_eval(void *handle, int n, const double *T, double *lambda)
{
  Handle *h = use(handle);
  if (!h) return PION_GPU_EINVAL;
  if (!h->have_curve || n <= 0 || !T || !lambda) {
    h->err = h->have_curve ? "cooling_curve_eval: n > 0, T and lambda required" : "cooling curve not set";
    return PION_GPU_EINVAL;
  }
  CoolTestArgs a;
  memset(&a, 0, sizeof a);
  a.n = n;
  DevBuf<double> bt, bl;
  const size_t nb = sizeof(double) * (size_t)n;
  HCHECK(h, hipMalloc(&bt.p, nb));
  HCHECK(h, hipMalloc(&bl.p, nb));
  HCHECK(h, hipMemcpy(bt.p, T, nb, hipMemcpyHostToDevice));
  a.T = bt.p;
  a.edot = bl.p;
  CoolForm f = h->form;
  f.flag = PION_COOL_WSS09_CIE_ONLY_COOLING;   // (any of 4..7: the curve instance)
  if (int rc = fp_launch(h, -1, "cooling-curve launch failed", fp_strict::launch_cool, fp_fast::launch_cool, a, f, 3, h->stream))
    return rc;
  HCHECK(h, hipStreamSynchronize(h->stream));
  HCHECK(h, hipMemcpy(lambda, bl.p, nb, hipMemcpyDeviceToHost));
  return 0;
}

int pion_gpu_enable_timing(void *handle, int on)
{
  Handle *h = use(handle);
  h->timing = on != 0;
  for (int s = 0; s < 4; s++) {
    for (hipEvent_t e : h->ev[s]) hipEventDestroy(e);
    h->ev[s].clear();
  }
  return 0;
}
int pion_gpu_get_timing(void *handle, double *out, int n)
{
  Handle *h = use(handle);
  HCHECK(h, hipStreamSynchronize(h->stream));
  for (int s = 0; s < 4 && s < n; s++) {
    double tot = 0.0;
    int cnt = 0;
    for (size_t k = 0; k + 1 < h->ev[s].size(); k += 2) {
      float ms = 0.f;
      if (hipEventElapsedTime(&ms, h->ev[s][k], h->ev[s][k + 1]) == hipSuccess) {
        tot += ms;
        cnt++;
      }
    }
    out[s] = cnt ? tot / cnt : 0.0;
    if (4 + s < n) out[4 + s] = cnt;
  }
  return 0;
}

}  // extern "C"
