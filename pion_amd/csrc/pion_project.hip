// pion_project.hip -- the device part of the projected images: pion_gpu_project sums the fields of dev_project.h
// along one axis of a 3-D Cartesian grid, or applies the reference's perpendicular Abel integral
// (analysis/projection/perp_projection.cpp:404-487) to every z column of a cylindrical (z,R) grid, into a device
// buffer [nfields][NJ][NI] of native doubles.  The rules -- the field, the cells of a pixel, the order of the
// additions, the Abel segment -- are dev_project.h's; this file holds the three kernels that run them and the C-ABI
// entry points.  Nothing here is part of a step: no stage kernel, StageArgs or handle state is touched.  The whole
// file is compiled without FMA contraction (Makefile), like every function of dev_project.h.
//
//   k_project_yz    line of sight along y or z.  A lane per pixel, 64 consecutive x per wavefront (loads are whole
//                   lines), the column walked in increasing index by that one lane.  No LDS, no atomics.
//   k_project_x     line of sight along x.  A wavefront per pixel: lane l sums the cells l, l + 64, .. of the row
//                   (coalesced), then the rule's tree over the 64 partial sums by __shfl_down.  No LDS, no atomics.
//   k_project_abel  cylindrical.  A workgroup of 4 wavefronts owns ABEL_J impact rows x 256 z cells; a wavefront's
//                   lanes are 64 consecutive z.  The geometric weights of a segment (AbelW: Rmin, xdx, x2dx -- two
//                   sqrt and a log) depend on (j, ir) only, so per block of ABEL_IR rows each thread evaluates ONE
//                   (j, ir) pair into LDS and every lane reads them back as broadcasts; each v[ir][z], s[ir][z] a
//                   lane loads and evaluates is used for all ABEL_J impact rows, accumulators in registers.  Per
//                   pixel the additions are the rule's -- abel_add in increasing ir from abel_start(j) --, so the
//                   image does not depend on the tiling.  LDS: ABEL_J * ABEL_IR weights (6 KiB) and the rows' start
//                   indices; no table that grows with NR.
// Each has a PART twin for one rank of a slab run (pion_gpu_project_part; dev_project.h, "parts"), working in/out on the
// image of the whole domain: k_project_yz_along (the sum enters with the carried value), k_project_yz_rows /
// k_project_x_rows (the rank's rows at their row offset), k_project_abel_part.  The whole-grid kernels are left as they
// were, instruction for instruction.
// pion_gpu_project_angle is the same grid seen at an angle to the axis (dev_project_angle.h): k_angle_values and
// k_project_angle, described where they stand.
// blockIdx.y: the field.  Unit, cell and buffer indices are long; the launch grid is checked against 2^31 - 1.
#include <hip/hip_runtime.h>

#include "dev_project.h"
#include "dev_project_angle.h"
#include "pion_handle.h"

using namespace pion;
using namespace pion::impl;

namespace {

constexpr int PRJ_WAVES = 4;
constexpr int ABEL_J = 16, ABEL_IR = 16;   // ABEL_J * ABEL_IR = the workgroup's 256 threads: one weight each per block
static_assert(ABEL_J * ABEL_IR == 64 * PRJ_WAVES, "one (j, ir) pair per thread");

__global__ void __launch_bounds__(64 * PRJ_WAVES)
k_project_yz(const double *__restrict__ A, double *__restrict__ out, const GridDesc g, const OutputCfg o,
             const ProjFields F, const ProjGeom q)
{
  const int nseg = (q.ni + 63) / 64;
  const long u = (long)blockIdx.x * PRJ_WAVES + (threadIdx.x >> 6);   // unit: (image row j, 64 pixels of it)
  if (u >= (long)q.nj * nseg) return;
  const long j = u / nseg;
  const int i = (int)(u - j * nseg) * 64 + (int)(threadIdx.x & 63);
  if (i >= q.ni) return;
  const pion_gpu_proj_field &f = F.f[blockIdx.y];
  const long first = q.c0 + i * q.si + j * q.sj;
  double s = 0.0;
  for (int k = 0; k < q.nsum; k++) s = proj_add(s, proj_value(g, o, f, A, first + k * q.ss));
  out[((long)blockIdx.y * q.nj + j) * q.ni + i] = proj_times_dx(g, s);
}

__global__ void __launch_bounds__(64 * PRJ_WAVES)
k_project_x(const double *__restrict__ A, double *__restrict__ out, const GridDesc g, const OutputCfg o,
            const ProjFields F, const ProjGeom q)
{
  const long u = (long)blockIdx.x * PRJ_WAVES + (threadIdx.x >> 6);   // pixel: j * ni + i
  if (u >= (long)q.nj * q.ni) return;
  const long j = u / q.ni;
  const long i = u - j * q.ni;
  const int lane = (int)(threadIdx.x & 63);
  const pion_gpu_proj_field &f = F.f[blockIdx.y];
  const long first = q.c0 + i * q.si + j * q.sj;
  double p = 0.0;
  for (int ix = lane; ix < q.nsum; ix += PROJ_LANES) p = proj_add(p, proj_value(g, o, f, A, first + ix));
  // p_l = p_l + p_(l+h) for l < h; what the lanes l >= h compute is never read
  for (int h = PROJ_LANES / 2; h >= 1; h /= 2) p = proj_add(p, __shfl_down(p, h, 64));
  if (lane == 0) out[(long)blockIdx.y * q.nj * q.ni + u] = proj_times_dx(g, p);
}

__global__ void __launch_bounds__(64 * PRJ_WAVES)
k_project_abel(const double *__restrict__ A, double *__restrict__ out, const GridDesc g, const OutputCfg o,
               const ProjFields F, const ProjGeom q)
{
  __shared__ AbelW W[ABEL_IR][ABEL_J];
  __shared__ int start[ABEL_J];   // abel_start of the tile's rows; nr for a row past the grid
  __shared__ int nact[ABEL_IR];   // rows of the tile whose sum has begun at row ir of the block (they are the first ones)

  const int nr = q.nsum, nz = q.ni, t = (int)threadIdx.x;
  const int nzt = (nz + 64 * PRJ_WAVES - 1) / (64 * PRJ_WAVES);
  // z tiles fastest; the j tiles in increasing j, so that the longest sums are dispatched first
  const long jt = (long)blockIdx.x / nzt;
  const int j0 = (int)jt * ABEL_J;
  const int z = (int)((long)blockIdx.x - jt * nzt) * 64 * PRJ_WAVES + t;
  const bool zok = z < nz;
  const pion_gpu_proj_field &f = F.f[blockIdx.y];
  const long first = q.c0 + (zok ? z : 0);   // (a lane past the row reads nothing)

  if (t < ABEL_J) start[t] = (j0 + t < nr) ? abel_start(g, nr, j0 + t) : nr;
  __syncthreads();
  const int ir_lo = start[0];

  double acc[ABEL_J];
#pragma unroll
  for (int jj = 0; jj < ABEL_J; jj++) acc[jj] = 0.0;

  // v and s of the row the walk is at.  s[ir] needs v[ir + 1]; the last row takes the slope of the one before it
  double vcur = 0.0, s = 0.0;
  if (zok) {
    vcur = proj_value(g, o, f, A, first + ir_lo * q.ss);
    if (ir_lo == nr - 1) s = abel_slope(g, nr - 2, proj_value(g, o, f, A, first + (nr - 2) * q.ss), vcur);
  }

  for (int irb = ir_lo; irb < nr; irb += ABEL_IR) {
    __syncthreads();   // the previous block's weights have been read
    {
      const int jj = t % ABEL_J, k = t / ABEL_J, ir = irb + k;
      AbelW w;
      w.Rmin = w.xdx = w.x2dx = 0.0;
      if (ir < nr && ir >= start[jj]) w = abel_weights(g, nr, j0 + jj, ir);
      W[k][jj] = w;
      if (jj == 0) {
        int n = 0;
        for (int m = 0; m < ABEL_J; m++) n += (ir >= start[m]) ? 1 : 0;   // (start[] does not decrease along the tile)
        nact[k] = n;
      }
    }
    __syncthreads();
    const int kmax = min(ABEL_IR, nr - irb);
    for (int k = 0; k < kmax; k++) {
      const int ir = irb + k;
      double vnext = 0.0;
      if (ir + 1 < nr) {
        if (zok) vnext = proj_value(g, o, f, A, first + (long)(ir + 1) * q.ss);
        s = abel_slope(g, ir, vcur, vnext);
      }
      const int n = __builtin_amdgcn_readfirstlane(nact[k]);
#pragma unroll
      for (int jj = 0; jj < ABEL_J; jj++)
        if (jj < n) acc[jj] = abel_add(acc[jj], vcur, s, W[k][jj]);
      vcur = vnext;
    }
  }
  if (!zok) return;
#pragma unroll
  for (int jj = 0; jj < ABEL_J; jj++)
    if (j0 + jj < nr) {
      const bool none = abel_b(g, j0 + jj) > abel_grid_max(g, nr);   // perp_projection.cpp:417-420
      out[((long)blockIdx.y * q.nj + (j0 + jj)) * q.ni + z] = none ? 0.0 : abel_finish(acc[jj]);
    }
}

// ---- a rank's part of a slab run's image (dev_project.h, "parts"): the image is the WHOLE domain's, in/out.
// k_project_yz's steps.  ALONG: the line of sight is the slab axis -- the sum enters with the carried value and only
// `last` multiplies by dx; otherwise the rank's own rows go to row offset row0 of an image of njg rows
template <bool ALONG>
__device__ __forceinline__ void project_yz(const double *__restrict__ A, double *__restrict__ out, const GridDesc &g,
                                           const OutputCfg &o, const ProjFields &F, const ProjGeom &q, const int row0,
                                           const int njg, const int last)
{
  const int nseg = (q.ni + 63) / 64;
  const long u = (long)blockIdx.x * PRJ_WAVES + (threadIdx.x >> 6);   // unit: (image row j, 64 pixels of it)
  if (u >= (long)q.nj * nseg) return;
  const long j = u / nseg;
  const int i = (int)(u - j * nseg) * 64 + (int)(threadIdx.x & 63);
  if (i >= q.ni) return;
  const pion_gpu_proj_field &f = F.f[blockIdx.y];
  const long first = q.c0 + i * q.si + j * q.sj;
  const long at = ((long)blockIdx.y * njg + (j + row0)) * q.ni + i;
  double s = ALONG ? out[at] : 0.0;
  for (int k = 0; k < q.nsum; k++) s = proj_add(s, proj_value(g, o, f, A, first + k * q.ss));
  out[at] = (ALONG && !last) ? s : proj_times_dx(g, s);
}
__global__ void __launch_bounds__(64 * PRJ_WAVES)
k_project_yz_along(const double *__restrict__ A, double *out, const GridDesc g, const OutputCfg o, const ProjFields F,
                   const ProjGeom q, const int last)
{
  project_yz<true>(A, out, g, o, F, q, 0, q.nj, last);
}
__global__ void __launch_bounds__(64 * PRJ_WAVES)
k_project_yz_rows(const double *__restrict__ A, double *__restrict__ out, const GridDesc g, const OutputCfg o,
                  const ProjFields F, const ProjGeom q, const int row0, const int njg)
{
  project_yz<false>(A, out, g, o, F, q, row0, njg, 1);
}

// k_project_x's steps, the rank's own rows at row offset row0 of an image of njg rows
__global__ void __launch_bounds__(64 * PRJ_WAVES)
k_project_x_rows(const double *__restrict__ A, double *__restrict__ out, const GridDesc g, const OutputCfg o,
                 const ProjFields F, const ProjGeom q, const int row0, const int njg)
{
  const long u = (long)blockIdx.x * PRJ_WAVES + (threadIdx.x >> 6);   // pixel: j * ni + i
  if (u >= (long)q.nj * q.ni) return;
  const long j = u / q.ni;
  const long i = u - j * q.ni;
  const int lane = (int)(threadIdx.x & 63);
  const pion_gpu_proj_field &f = F.f[blockIdx.y];
  const long first = q.c0 + i * q.si + j * q.sj;
  double p = 0.0;
  for (int ix = lane; ix < q.nsum; ix += PROJ_LANES) p = proj_add(p, proj_value(g, o, f, A, first + ix));
  // p_l = p_l + p_(l+h) for l < h; what the lanes l >= h compute is never read
  for (int h = PROJ_LANES / 2; h >= 1; h /= 2) p = proj_add(p, __shfl_down(p, h, 64));
  if (lane == 0) out[((long)blockIdx.y * njg + row0) * q.ni + u] = proj_times_dx(g, p);
}

// k_project_abel's steps for a part: the rows of array A are the global rows lo .. hi - 1, the geometry (gg: the whole
// grid's R origin; nr: its NR) takes global indices, the impact rows are 0 .. hi - 1, their accumulators start from the
// carried image and only `last` finishes them.  The same LDS weight sharing, readfirstlane count and absence of atomics:
// a pixel is read and written by the one lane that owns it
__global__ void __launch_bounds__(64 * PRJ_WAVES)
k_project_abel_part(const double *__restrict__ A, double *out, const GridDesc g, const OutputCfg o, const ProjFields F,
                    const ProjGeom q, const ProjPart part)
{
  const GridDesc gg = proj_part_grid(g, part);
  const int nr = part.global_planes, lo = part.plane_lo, njg = part.global_planes, last = part.last;
  __shared__ AbelW W[ABEL_IR][ABEL_J];
  __shared__ int start[ABEL_J];   // first segment of the tile's rows that this grid holds; hi for a row past its upper edge
  __shared__ int nact[ABEL_IR];   // rows of the tile whose sum has begun at row ir of the block (they are the first ones)

  const int hi = lo + q.nsum, nz = q.ni, t = (int)threadIdx.x;
  const int nzt = (nz + 64 * PRJ_WAVES - 1) / (64 * PRJ_WAVES);
  // z tiles fastest; the j tiles in increasing j, so that the longest sums are dispatched first
  const long jt = (long)blockIdx.x / nzt;
  const int j0 = (int)jt * ABEL_J;
  const int z = (int)((long)blockIdx.x - jt * nzt) * 64 * PRJ_WAVES + t;
  const bool zok = z < nz;
  const pion_gpu_proj_field &f = F.f[blockIdx.y];
  const long first = q.c0 + (zok ? z : 0) - (long)lo * q.ss;   // global row 0 (a lane past the row reads nothing)

  if (t < ABEL_J) {
    int st = hi;
    if (j0 + t < hi) {
      st = abel_start(gg, nr, j0 + t);
      if (st < lo) st = lo;
    }
    start[t] = st;
  }
  __syncthreads();
  const int ir_lo = start[0];

  double acc[ABEL_J];
#pragma unroll
  for (int jj = 0; jj < ABEL_J; jj++)
    acc[jj] = (zok && j0 + jj < hi) ? out[((long)blockIdx.y * njg + (j0 + jj)) * q.ni + z] : 0.0;

  // v and s of the row the walk is at.  s[ir] needs v[ir + 1] (a part's last own row: the first upper ghost row); the
  // global last row takes the slope of the one before it
  double vcur = 0.0, s = 0.0;
  if (zok) {
    vcur = proj_value(g, o, f, A, first + ir_lo * q.ss);
    if (ir_lo == nr - 1) s = abel_slope(gg, nr - 2, proj_value(g, o, f, A, first + (nr - 2) * q.ss), vcur);
  }

  for (int irb = ir_lo; irb < hi; irb += ABEL_IR) {
    __syncthreads();   // the previous block's weights have been read
    {
      const int jj = t % ABEL_J, k = t / ABEL_J, ir = irb + k;
      AbelW w;
      w.Rmin = w.xdx = w.x2dx = 0.0;
      if (ir < hi && ir >= start[jj]) w = abel_weights(gg, nr, j0 + jj, ir);
      W[k][jj] = w;
      if (jj == 0) {
        int n = 0;
        for (int m = 0; m < ABEL_J; m++) n += (ir >= start[m]) ? 1 : 0;   // (start[] does not decrease along the tile)
        nact[k] = n;
      }
    }
    __syncthreads();
    const int kmax = min(ABEL_IR, hi - irb);
    for (int k = 0; k < kmax; k++) {
      const int ir = irb + k;
      double vnext = 0.0;
      if (ir + 1 < nr) {
        if (zok) vnext = proj_value(g, o, f, A, first + (long)(ir + 1) * q.ss);
        s = abel_slope(gg, ir, vcur, vnext);
      }
      const int n = __builtin_amdgcn_readfirstlane(nact[k]);
#pragma unroll
      for (int jj = 0; jj < ABEL_J; jj++)
        if (jj < n) acc[jj] = abel_add(acc[jj], vcur, s, W[k][jj]);
      vcur = vnext;
    }
  }
  if (!zok) return;
#pragma unroll
  for (int jj = 0; jj < ABEL_J; jj++)
    if (j0 + jj < hi) {
      const long at = ((long)blockIdx.y * njg + (j0 + jj)) * q.ni + z;
      if (!last) out[at] = acc[jj];
      else {
        const bool none = abel_b(gg, j0 + jj) > abel_grid_max(gg, nr);   // perp_projection.cpp:417-420
        out[at] = none ? 0.0 : abel_finish(acc[jj]);
      }
    }
}

// ---- the inclined projection of a cylindrical grid (dev_project_angle.h).  Two launches per call:
//   k_angle_values   dev_project.h's proj_value of every field at every on-grid cell, once, into V = [nfields][NR][NZ]
//                    (blockIdx.y: the field): the exp / log of T^b is paid per cell, not per visit, and the walk only loads.
//   k_project_angle  a lane per pixel, a wavefront = 64 consecutive i of one impact row j: the rays of neighbouring lanes
//                    are copies shifted by one cell in z, so they take the same branches and load adjacent cells.  All
//                    fields are summed in the one walk.  A pixel is a property of (i, j) alone: angle_pixel, the host
//                    loop's function.  No LDS, no waiting on another workgroup; a capped pixel adds 1 to *capped
//                    (a plain atomic that nothing polls).
__global__ void __launch_bounds__(64 * PRJ_WAVES)
k_angle_values(const double *__restrict__ A, double *__restrict__ V, const GridDesc g, const OutputCfg o, const ProjFields F)
{
  const long ncells = (long)g.ng[0] * g.ng[1];
  const long u = (long)blockIdx.x * (64 * PRJ_WAVES) + threadIdx.x;
  if (u >= ncells) return;
  const long ir = u / g.ng[0], iz = u - ir * g.ng[0];
  const long c = (g.nbc[0] + iz) + g.sy * (g.nbc[1] + ir);
  V[(long)blockIdx.y * ncells + u] = proj_value(g, o, F.f[blockIdx.y], A, c);
}

__global__ void __launch_bounds__(64 * PRJ_WAVES)
k_project_angle(const double *__restrict__ V, double *__restrict__ out, const AngleGeom q, const int nfields, const int trip_limit,
                unsigned long long *__restrict__ capped)
{
  const int nseg = (q.ni + 63) / 64;
  const long u = (long)blockIdx.x * PRJ_WAVES + (threadIdx.x >> 6);   // unit: (impact row j, 64 pixels of it)
  if (u >= (long)q.nr * nseg) return;
  const long j = u / nseg;
  const long i = (u - j * nseg) * 64 + (long)(threadIdx.x & 63);
  if (i >= q.ni) return;
  double ans[PION_PROJ_MAX_FIELDS];
  if (angle_pixel(q, V, nfields, i, (int)j, trip_limit, ans)) atomicAdd(capped, 1ULL);
#pragma unroll
  for (int f = 0; f < PION_PROJ_MAX_FIELDS; f++)
    if (f < nfields) out[((long)f * q.nr + j) * q.ni + i] = ans[f];
}

OutputCfg project_cfg(const Handle *h)
{
  OutputCfg o = out_cfg(h->cfg);
  o.Mu_tot_over_kB = h->Mu_tot_over_kB;
  return o;
}

}  // namespace

extern "C" {

long pion_gpu_project_count(void *handle, int axis, int nfields)
{
  Handle *h = (Handle *)handle;
  if (!h) return PION_GPU_EINVAL;
  if (const char *why = proj_refused_grid(h->g, axis)) {
    h->err = why;
    return PION_GPU_EINVAL;
  }
  if (nfields < 1 || nfields > PION_PROJ_MAX_FIELDS) {
    h->err = "project: between 1 and 8 fields per call";
    return PION_GPU_EINVAL;
  }
  return proj_count(proj_geom(h->g, axis), nfields);
}

int pion_gpu_project(void *handle, int which, int axis, int nfields, const pion_gpu_proj_field *fields, void *dbuf)
{
  Handle *h = use(handle);
  if (!h) return PION_GPU_EINVAL;
  const OutputCfg o = project_cfg(h);
  const char *why = proj_refused_grid(h->g, axis);
  if (!why) why = proj_refused_fields(o, nfields, fields);
  if (!why && (which < 0 || which > 1)) why = "project: which is 0 (P) or 1 (Ph)";
  if (!why && !dbuf) why = "project: no buffer";
  if (why) {
    h->err = why;
    return PION_GPU_EINVAL;
  }
  const ProjGeom q = proj_geom(h->g, axis);
  ProjFields F;
  F.n = nfields;
  for (int i = 0; i < PION_PROJ_MAX_FIELDS; i++) F.f[i] = fields[i < nfields ? i : 0];
  const double *A = which ? h->dPh : h->dP;
  long nblk;
  if (h->g.cyl == 1) nblk = (long)((q.ni + 64 * PRJ_WAVES - 1) / (64 * PRJ_WAVES)) * ((q.nj + ABEL_J - 1) / ABEL_J);
  else if (axis == 0) nblk = ((long)q.nj * q.ni + PRJ_WAVES - 1) / PRJ_WAVES;
  else nblk = ((long)q.nj * ((q.ni + 63) / 64) + PRJ_WAVES - 1) / PRJ_WAVES;
  if (nblk > (1L << 31) - 1) {
    h->err = "project: the image is too large for one launch";
    return PION_GPU_EINVAL;
  }
  const dim3 grid((unsigned)nblk, (unsigned)nfields), block(64 * PRJ_WAVES);
  if (h->g.cyl == 1)
    hipLaunchKernelGGL(k_project_abel, grid, block, 0, h->stream, A, (double *)dbuf, h->g, o, F, q);
  else if (axis == 0)
    hipLaunchKernelGGL(k_project_x, grid, block, 0, h->stream, A, (double *)dbuf, h->g, o, F, q);
  else
    hipLaunchKernelGGL(k_project_yz, grid, block, 0, h->stream, A, (double *)dbuf, h->g, o, F, q);
  HCHECK(h, hipGetLastError());
  return 0;
}

long pion_gpu_project_part_count(void *handle, int axis, int nfields, const pion_gpu_proj_part *part)
{
  Handle *h = (Handle *)handle;
  if (!h) return PION_GPU_EINVAL;
  const char *why = proj_refused_grid(h->g, axis);
  if (!why && (nfields < 1 || nfields > PION_PROJ_MAX_FIELDS)) why = "project: between 1 and 8 fields per call";
  if (!why) why = proj_refused_part(h->g, part);
  if (why) {
    h->err = why;
    return PION_GPU_EINVAL;
  }
  const ProjPart pp = {part->plane_lo, part->global_planes, part->last ? 1 : 0, part->global_xmin};
  return proj_part_count(h->g, proj_geom(h->g, axis), axis, pp, nfields);
}

int pion_gpu_project_part(void *handle, int which, int axis, int nfields, const pion_gpu_proj_field *fields,
                          const pion_gpu_proj_part *part, void *dimg)
{
  Handle *h = use(handle);
  if (!h) return PION_GPU_EINVAL;
  const OutputCfg o = project_cfg(h);
  const char *why = proj_refused_grid(h->g, axis);
  if (!why) why = proj_refused_fields(o, nfields, fields);
  if (!why && (which < 0 || which > 1)) why = "project: which is 0 (P) or 1 (Ph)";
  if (!why) why = proj_refused_part(h->g, part);
  if (!why && !dimg) why = "project: no buffer";
  if (why) {
    h->err = why;
    return PION_GPU_EINVAL;
  }
  const ProjGeom q = proj_geom(h->g, axis);
  const ProjPart pp = {part->plane_lo, part->global_planes, part->last ? 1 : 0, part->global_xmin};
  ProjFields F;
  F.n = nfields;
  for (int i = 0; i < PION_PROJ_MAX_FIELDS; i++) F.f[i] = fields[i < nfields ? i : 0];
  const double *A = which ? h->dPh : h->dP;
  const bool cyl = h->g.cyl == 1, along = proj_part_along_slab(h->g, axis);
  const int njg = proj_part_nj(h->g, q, axis, pp);
  long nblk;   // the impact rows of a cylindrical part: those below its upper edge
  if (cyl) nblk = (long)((q.ni + 64 * PRJ_WAVES - 1) / (64 * PRJ_WAVES)) * (((long)pp.plane_lo + q.nsum + ABEL_J - 1) / ABEL_J);
  else if (axis == 0) nblk = ((long)q.nj * q.ni + PRJ_WAVES - 1) / PRJ_WAVES;
  else nblk = ((long)q.nj * ((q.ni + 63) / 64) + PRJ_WAVES - 1) / PRJ_WAVES;
  if (nblk > (1L << 31) - 1) {
    h->err = "project: the image is too large for one launch";
    return PION_GPU_EINVAL;
  }
  const dim3 grid((unsigned)nblk, (unsigned)nfields), block(64 * PRJ_WAVES);
  double *img = (double *)dimg;
  if (cyl)
    hipLaunchKernelGGL(k_project_abel_part, grid, block, 0, h->stream, A, img, h->g, o, F, q, pp);
  else if (along)
    hipLaunchKernelGGL(k_project_yz_along, grid, block, 0, h->stream, A, img, h->g, o, F, q, pp.last);
  else if (axis == 0)
    hipLaunchKernelGGL(k_project_x_rows, grid, block, 0, h->stream, A, img, h->g, o, F, q, pp.plane_lo, njg);
  else
    hipLaunchKernelGGL(k_project_yz_rows, grid, block, 0, h->stream, A, img, h->g, o, F, q, pp.plane_lo, njg);
  HCHECK(h, hipGetLastError());
  return 0;
}

long pion_gpu_project_angle_count(void *handle, double angle_deg, int nfields, int *n_extra)
{
  Handle *h = (Handle *)handle;
  if (!h) return PION_GPU_EINVAL;
  AngleGeom q;
  if (const char *why = angle_refused(h->g, h->cfg, angle_deg, nfields, &q)) {
    h->err = why;
    return PION_GPU_EINVAL;
  }
  if (n_extra) *n_extra = q.n_extra;
  return angle_count(q, nfields);
}

int pion_gpu_project_angle(void *handle, int which, double angle_deg, int nfields, const pion_gpu_proj_field *fields, void *dbuf)
{
  Handle *h = use(handle);
  if (!h) return PION_GPU_EINVAL;
  const OutputCfg o = project_cfg(h);
  AngleGeom q;
  const char *why = angle_refused(h->g, h->cfg, angle_deg, nfields, &q);
  if (!why) why = proj_refused_fields(o, nfields, fields);
  if (!why && (which < 0 || which > 1)) why = "project: which is 0 (P) or 1 (Ph)";
  if (!why && !dbuf) why = "project: no buffer";
  if (why) {
    h->err = why;
    return PION_GPU_EINVAL;
  }
  const long ncells = (long)q.nr * q.nz;
  const long nblk_v = (ncells + 64 * PRJ_WAVES - 1) / (64 * PRJ_WAVES);
  const long nblk = ((long)q.nr * ((q.ni + 63) / 64) + PRJ_WAVES - 1) / PRJ_WAVES;
  if (nblk > (1L << 31) - 1 || nblk_v > (1L << 31) - 1) {
    h->err = "project: the image is too large for one launch";
    return PION_GPU_EINVAL;
  }
  // (the scratch of the handle: a launch of an earlier call that reads the old one has to end before it is freed, and
  // hipFree waits for it)
  if (h->angle_vals_n < (long)nfields * ncells) {
    if (h->dangle_vals) HCHECK(h, hipFree(h->dangle_vals));
    h->dangle_vals = nullptr, h->angle_vals_n = 0;
    HCHECK(h, hipMalloc((void **)&h->dangle_vals, (size_t)nfields * ncells * sizeof(double)));
    h->angle_vals_n = (long)nfields * ncells;
  }
  if (!h->dangle_capped) {
    HCHECK(h, hipMalloc((void **)&h->dangle_capped, sizeof(unsigned long long)));
    HCHECK(h, hipMemsetAsync(h->dangle_capped, 0, sizeof(unsigned long long), h->stream));
  }
  ProjFields F;
  F.n = nfields;
  for (int i = 0; i < PION_PROJ_MAX_FIELDS; i++) F.f[i] = fields[i < nfields ? i : 0];
  const double *A = which ? h->dPh : h->dP;
  const dim3 block(64 * PRJ_WAVES);
  hipLaunchKernelGGL(k_angle_values, dim3((unsigned)nblk_v, (unsigned)nfields), block, 0, h->stream, A, h->dangle_vals, h->g, o, F);
  HCHECK(h, hipGetLastError());
  hipLaunchKernelGGL(k_project_angle, dim3((unsigned)nblk), block, 0, h->stream, (const double *)h->dangle_vals, (double *)dbuf, q,
                     nfields, angle_trip_limit(q), h->dangle_capped);
  HCHECK(h, hipGetLastError());
  return 0;
}

int pion_gpu_project_angle_status(void *handle, long *ncapped)
{
  Handle *h = use(handle);
  if (!h || !ncapped) return PION_GPU_EINVAL;
  *ncapped = 0;
  if (!h->dangle_capped) return 0;   // nothing was projected yet
  unsigned long long n = 0;
  HCHECK(h, hipMemcpyAsync(&n, h->dangle_capped, sizeof n, hipMemcpyDeviceToHost, h->stream));
  HCHECK(h, hipMemsetAsync(h->dangle_capped, 0, sizeof n, h->stream));
  HCHECK(h, hipStreamSynchronize(h->stream));
  *ncapped = (long)n;
  return 0;
}
}
