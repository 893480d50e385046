// pion_raytrace.hip -- the device part of the ray-traced column densities: pion_gpu_raytrace leaves, per radiation
// source, the column density to + through every on-grid cell (col) and the column through it (dcol), as the
// reference's short-characteristics tracer raytracer_USC does in extra_data.  The rules -- the source's vertex, the
// neighbours a cell reads and their weights, the column through a cell -- are dev_raytrace.h's; this file holds the
// kernels that run them and the C-ABI entry points.  Nothing here is part of a step: the state is only read, no stage
// kernel, StageArgs or cached result of the handle is touched.  The whole file is compiled without FMA contraction
// (Makefile), like every function of dev_raytrace.h.
//
// A cell of a finite source reads up to four cells one step nearer the source (dev_raytrace.h, "the dependency").
// Ordering comes from launch boundaries on the handle's compute stream and from __syncthreads() inside a workgroup,
// from nothing else: no workgroup waits for another one of its launch, nothing polls memory.
//
//   k_rt_levels    the plain form and the cross-check (PION_RT_KERNEL=levels).  One launch per level L = sum_a k_a, a
//                  thread per (y, z) column and x side: it owns at most one cell of the level, k_x = L - k_y - k_z.
//   k_rt_tiles     the production form.  Tiles of TX x TY x TZ cells counted from the source vertex outwards, so that
//                  no tile straddles an octant; one launch per tile-level T = sum_a t_a.  A workgroup of ONE wavefront
//                  owns a tile: its 64 lanes are the tile's TY x TZ columns along x, and in-tile level l gives lane
//                  (ly, lz) the cell lx = l - ly - lz.  The tile's columns and the one-cell halo towards the source
//                  live in LDS, rho (and the tracer) are read once into LDS with whole runs along x, col and dcol are
//                  written once the same way.
//   k_rt_par_yz    a source at infinity along y or z: a lane per column, 64 consecutive x per wavefront.
//   k_rt_par_x     along x: a wavefront takes 64 rows and stages 64 x 32 blocks of rho (and the tracer) through LDS so
//                  that loads and stores are runs along x; each lane adds along its own row, one addition after the
//                  other in ray order (no scan: the association is the sequential one).
//   k_pack_columns big-endian copy of a plane range for the FITS writer.
// Cell ids and buffer indices are long; launch grids are checked against 2^31 - 1.
//
// A slab of a decomposed run (dev_raytrace.h, "a part"; pion_gpu_add_rt_source_part, pion_gpu_raytrace_part): every
// source's col array has one spare plane below and one above the on-grid planes, and the plane the neighbouring rank
// handed over is copied into the one that looks towards the source before the launches.  The kernels are given the
// first on-grid plane, so their loads stay as they are, and "readable" (rt_readable) is on-grid or in that spare plane.
// k_rt_levels and the host loop read it through ColGlobal, k_rt_par_yz starts its sum from it, and k_rt_tiles finds it
// inside the first tile that holds cells or in that tile's halo (see there).  The rank's lowest and highest own plane
// leave by copies on the same stream after the launches.
#include <hip/hip_runtime.h>

#include <cstdlib>
#include <cstring>

#include "dev_raytrace.h"
#include "pion_handle.h"

using namespace pion;
using namespace pion::impl;

namespace pion::impl {
struct RtState {
  std::vector<RtSrc> src;
  std::vector<double *> dcols;   // per source: a spare plane, col [nz][ny][nx], a spare plane, dcol [nz][ny][nx]
  std::vector<int> part;         // added with a part (pion_gpu_add_rt_source_part)
  std::vector<RtRole> role;      // its role in the chain (no part: receives nothing, sends nothing)
  int levels = 0;                // finite sources run k_rt_levels
};
}  // namespace pion::impl

namespace {

// what the kernels need of the grid besides GridDesc: on-grid extents and the on-grid cell count
struct RtGeom {
  int nx, ny, nz, ndim;
  long n;        // nx * ny * nz
  long off0;     // all-cell id of on-grid cell (0, 0, 0)
  long sy, sz;   // all-cell strides
  long ncell;    // cells per variable, ghosts included
  double dx;
  // a part of a decomposed run: the plane of the slab axis (z in 3-D, y in 2-D) one below (glo) or one above (ghi) the
  // on-grid planes holds the columns the neighbouring rank handed over.  The column array has both spare planes.
  int glo, ghi;
};

RtGeom rt_geom(const GridDesc &g)
{
  RtGeom q;
  q.ndim = g.ndim;
  q.nx = g.ng[0];
  q.ny = g.ng[1];
  q.nz = g.ng[2];
  q.n = (long)q.nx * q.ny * q.nz;
  q.sy = g.sy;
  q.sz = g.sz;
  q.off0 = g.nbc[0] + g.sy * g.nbc[1] + g.sz * g.nbc[2];
  q.ncell = g.ncell;
  q.dx = g.dx;
  q.glo = q.ghi = 0;
  return q;
}
RtGeom rt_geom(const GridDesc &g, const int recv_side)
{
  RtGeom q = rt_geom(g);
  q.glo = recv_side == PION_RT_RECV_BELOW;
  q.ghi = recv_side == PION_RT_RECV_ABOVE;
  return q;
}

__host__ __device__ inline long rt_state_id(const RtGeom &q, const int ix, const int iy, const int iz)
{
  return q.off0 + ix + q.sy * iy + q.sz * iz;
}
__host__ __device__ inline long rt_col_id(const RtGeom &q, const int ix, const int iy, const int iz)
{
  return ix + (long)q.nx * (iy + (long)q.ny * iz);
}
__host__ __device__ inline bool rt_ongrid(const RtGeom &q, const int ix, const int iy, const int iz)
{
  return ix >= 0 && ix < q.nx && iy >= 0 && iy < q.ny && iz >= 0 && iz < q.nz;
}

// on the grid, or in the spare plane that holds what was received (rt_col_id is valid there: plane -1 or n)
__host__ __device__ inline bool rt_readable(const RtGeom &q, const int ix, const int iy, const int iz)
{
  if (q.ndim == 3) return ix >= 0 && ix < q.nx && iy >= 0 && iy < q.ny && iz >= -q.glo && iz < q.nz + q.ghi;
  return ix >= 0 && ix < q.nx && iy >= -q.glo && iy < q.ny + q.ghi && iz == 0;
}

// the finished column of a neighbour in the column array itself
struct ColGlobal {
  const double *col;
  const RtGeom *q;
  __host__ __device__ double operator()(const int ix, const int iy, const int iz) const
  {
    return rt_readable(*q, ix, iy, iz) ? col[rt_col_id(*q, ix, iy, iz)] : 0.0;
  }
};

// one cell of a finite source from the column array: the host loop and k_rt_levels
template <class ColAt>
__host__ __device__ inline void rt_cell(const double *__restrict__ P, const RtGeom &q, const RtSrc &s, const int ix,
                                        const int iy, const int iz, const ColAt &colat, double *col, double *dcol)
{
  double ds;
  const double c2c = (q.ndim == 3) ? rt_col2cell_3d(s, q.dx, ix, iy, iz, colat, &ds)
                                   : rt_col2cell_2d(s, q.dx, ix, iy, colat, &ds);
  const long c = rt_state_id(q, ix, iy, iz);
  const double y = (s.opacity == PION_RT_OPACITY_TOTAL) ? 0.0 : P[(long)s.var * q.ncell + c];
  const double dc = rt_dcol(s.opacity, ds, P[c], y);
  *dcol = dc;
  *col = c2c + dc;
}

__global__ void __launch_bounds__(256)
k_rt_levels(const double *__restrict__ P, double *col, double *__restrict__ dcol, const RtGeom q, const RtSrc s,
            const long L)
{
  const long t = (long)blockIdx.x * blockDim.x + threadIdx.x;
  const long ncolumn = (long)q.ny * q.nz;
  if (t >= 2 * ncolumn) return;
  const int side = (int)(t / ncolumn);
  const long r = t - side * ncolumn;
  const int iz = (int)(r / q.ny), iy = (int)(r - (long)iz * q.ny);
  const long kx = L - (rt_dist(iy, s.ipos[1]) - 1) / 2 - (rt_dist(iz, s.ipos[2]) - 1) / 2;
  if (kx < 0 || kx >= (1L << 30)) return;
  const int ix = rt_k_to_i(s.ipos[0] / 2, side, (int)kx);
  if (ix < 0 || ix >= q.nx) return;
  const ColGlobal colat = {col, &q};
  const long c = rt_col_id(q, ix, iy, iz);
  rt_cell(P, q, s, ix, iy, iz, colat, &col[c], &dcol[c]);
}

// the tiles of one axis as a launch sees them: side 0 holds tiles lo0 .. lo0 + nt0 - 1, side 1 tiles lo1 .. lo1 + nt1 - 1,
// the tiles of [klo / tile, khi / tile] (a side without on-grid cells holds none)
struct RtTileAxis { int lo0, nt0, lo1, nt1; };

template <int TX, int TY, int TZ>
__global__ void __launch_bounds__(64)
k_rt_tiles(const double *__restrict__ P, double *col, double *__restrict__ dcol, const RtGeom q, const RtSrc s,
           const RtPlan p, const RtTileAxis ay, const RtTileAxis az, const long T)
{
  static_assert(TY * TZ == 64, "a lane per (y, z) column of the tile");
  constexpr int HZ = (TZ > 1) ? TZ + 1 : 1, OZ = (TZ > 1) ? 1 : 0;   // 2-D: no halo plane
  __shared__ double scol[HZ][TY + 1][TX + 1];
  __shared__ double srho[TZ][TY][TX];   // rho, then dcol
  __shared__ double sy_[TZ][TY][TX];    // the tracer (MINUS, TRACER)

  // the tile: (x side, signed y tile, signed z tile); t_x from the tile-level
  const int nty = ay.nt0 + ay.nt1, ntz = az.nt0 + az.nt1;
  long b = blockIdx.x;
  const int sidex = (int)(b % 2);
  b /= 2;
  const int jy = (int)(b % nty), jz = (int)(b / nty);
  if (jz >= ntz) return;
  const int sidey = (jy < ay.nt0) ? 0 : 1, ty = sidey ? ay.lo1 + jy - ay.nt0 : ay.lo0 + jy;
  const int sidez = (jz < az.nt0) ? 0 : 1, tz = sidez ? az.lo1 + jz - az.nt0 : az.lo0 + jz;
  const long tx = T - ty - tz;
  if (tx < 0 || tx > p.khi[0][sidex] / TX || p.khi[0][sidex] < p.klo[0][sidex]) return;
  const int k0x = (int)tx * TX, k0y = ty * TY, k0z = tz * TZ;
  // (whole-tile exits only: every lane of the workgroup takes the same way to here)
  if (k0x + TX - 1 < p.klo[0][sidex] || k0y + TY - 1 < p.klo[1][sidey] || k0y > p.khi[1][sidey]
      || k0z + TZ - 1 < p.klo[2][sidez] || k0z > p.khi[2][sidez])
    return;

  const int lane = (int)threadIdx.x;
  const bool tracer = s.opacity != PION_RT_OPACITY_TOTAL;

  // The plane received from the neighbouring rank (q.glo, q.ghi).  Tiles are counted from the source vertex, so that
  // plane lies in general INSIDE the first tile that holds on-grid cells (slot eg of the slab axis), and in the tile's
  // halo only where the slab's face falls on a tile boundary (eg = -1: the halo loads below read it as readable).
  constexpr int TS = (TZ > 1) ? TZ : TY;                      // the tile along the slab axis
  constexpr int NG = (TZ > 1) ? TX * TY : TX, GIT = (NG + 63) / 64;
  const int sides = (TZ > 1) ? sidez : sidey, k0s = (TZ > 1) ? k0z : k0y;
  const int kg = q.glo ? -1 - p.v[TZ > 1 ? 2 : 1] : p.v[TZ > 1 ? 2 : 1] - 1 - ((TZ > 1) ? q.nz : q.ny);
  const int eg = kg - k0s;
  const bool ghost_in = (q.glo || q.ghi) && sides == (q.glo ? 1 : 0) && eg >= 0 && eg < TS;

  // Every global load of the tile is issued before the first one is used: the loops below have constant trip counts and
  // are unrolled, and a lane without a cell loads from a valid address (on-grid cell 0) and discards the value, so
  // that no load sits behind a branch.
  // 1. the halo towards the source from the column array (0 across a source plane and off the grid): the x face
  //    (ex = 0), then the y face (ey = 0, ex >= 1), then in 3-D the z face (ez = 0, ex >= 1, ey >= 1)
  constexpr int NHX = (TY + 1) * HZ, NHY = TX * HZ, NHZ = OZ ? TX * TY : 0, NH = NHX + NHY + NHZ;
  constexpr int HIT = (NH + 63) / 64, CIT = TX * TY * TZ / 64;
  double hv[HIT];
#pragma unroll
  for (int it = 0; it < HIT; it++) {
    const int e = lane + 64 * it;
    int ex = 0, ey = 0, ez = 0;
    if (e < NHX) { ey = e % (TY + 1); ez = e / (TY + 1); }
    else if (e < NHX + NHY) { ex = 1 + (e - NHX) % TX; ez = (e - NHX) / TX; }
    else { ex = 1 + (e - NHX - NHY) % TX; ey = 1 + (e - NHX - NHY) / TX; }
    const int kx = k0x + ex - 1, ky = k0y + ey - 1, kz = k0z + ez - OZ;
    const int ix = rt_k_to_i(p.v[0], sidex, kx), iy = rt_k_to_i(p.v[1], sidey, ky), iz = rt_k_to_i(p.v[2], sidez, kz);
    const bool on = e < NH && kx >= 0 && ky >= 0 && kz >= 0 && rt_readable(q, ix, iy, iz);
    const double v = col[on ? rt_col_id(q, ix, iy, iz) : 0L];
    hv[it] = on ? v : 0.0;
  }
  //    the received plane inside the tile: the same way, from on-grid cell 0 where there is none
  double gv[GIT];
#pragma unroll
  for (int it = 0; it < GIT; it++) {
    const int e = lane + 64 * it;
    const int ex = e % TX, ey = (TZ > 1) ? e / TX : eg, ez = (TZ > 1) ? eg : 0;
    const int ix = rt_k_to_i(p.v[0], sidex, k0x + ex), iy = rt_k_to_i(p.v[1], sidey, k0y + ey),
              iz = rt_k_to_i(p.v[2], sidez, k0z + ez);
    const bool on = ghost_in && e < NG && rt_readable(q, ix, iy, iz);
    const double v = col[on ? rt_col_id(q, ix, iy, iz) : 0L];
    gv[it] = on ? v : 0.0;
  }
  // 2. rho and the tracer: consecutive lanes along x
  double rv[CIT], yv[CIT];
#pragma unroll
  for (int it = 0; it < CIT; it++) {
    const int e = lane + 64 * it;
    const int ex = e % TX, ey = (e / TX) % TY, ez = e / (TX * TY);
    const int ix = rt_k_to_i(p.v[0], sidex, k0x + ex), iy = rt_k_to_i(p.v[1], sidey, k0y + ey),
              iz = rt_k_to_i(p.v[2], sidez, k0z + ez);
    const bool on = rt_ongrid(q, ix, iy, iz);
    const long c = on ? rt_state_id(q, ix, iy, iz) : q.off0;
    const double r = P[c];
    const double y = tracer ? P[(long)s.var * q.ncell + c] : 0.0;
    rv[it] = on ? r : 0.0;
    yv[it] = on ? y : 0.0;
  }
#pragma unroll
  for (int it = 0; it < HIT; it++) {
    const int e = lane + 64 * it;
    int ex = 0, ey = 0, ez = 0;
    if (e < NHX) { ey = e % (TY + 1); ez = e / (TY + 1); }
    else if (e < NHX + NHY) { ex = 1 + (e - NHX) % TX; ez = (e - NHX) / TX; }
    else { ex = 1 + (e - NHX - NHY) % TX; ey = 1 + (e - NHX - NHY) / TX; }
    if (e < NH) scol[ez][ey][ex] = hv[it];
  }
#pragma unroll
  for (int it = 0; it < CIT; it++) {
    const int e = lane + 64 * it;
    const int ex = e % TX, ey = (e / TX) % TY, ez = e / (TX * TY);
    srho[ez][ey][ex] = rv[it];
    sy_[ez][ey][ex] = yv[it];
    // a cell of the tile that is off the grid contributes 0; the received plane's slots are written below
    if (!(ghost_in && ((TZ > 1) ? ez : ey) == eg)) scol[ez + OZ][ey + 1][ex + 1] = 0.0;
  }
#pragma unroll
  for (int it = 0; it < GIT; it++) {
    const int e = lane + 64 * it;
    const int ex = e % TX, ey = (TZ > 1) ? e / TX : eg, ez = (TZ > 1) ? eg : 0;
    if (ghost_in && e < NG) scol[ez + OZ][ey + 1][ex + 1] = gv[it];
  }
  __syncthreads();

  // the finished column of a neighbour in LDS: it lies in the tile's octant, one step nearer the source at most per axis
  const auto colat = [&](const int ix, const int iy, const int iz) -> double {
    const int ex = (rt_dist(ix, s.ipos[0]) - 1) / 2 - k0x + 1, ey = (rt_dist(iy, s.ipos[1]) - 1) / 2 - k0y + 1;
    const int ez = OZ ? (rt_dist(iz, s.ipos[2]) - 1) / 2 - k0z + 1 : 0;
    return scol[ez][ey][ex];
  };

  const int ly = lane % TY, lz = lane / TY;
  const int iy = rt_k_to_i(p.v[1], sidey, k0y + ly), iz = rt_k_to_i(p.v[2], sidez, k0z + lz);
  const bool column_on = iy >= 0 && iy < q.ny && iz >= 0 && iz < q.nz;
  for (int l = 0; l < TX + TY + TZ - 2; l++) {
    const int lx = l - ly - lz;
    if (column_on && lx >= 0 && lx < TX) {
      const int ix = rt_k_to_i(p.v[0], sidex, k0x + lx);
      if (ix >= 0 && ix < q.nx) {
        double ds;
        const double c2c = (TZ > 1) ? rt_col2cell_3d(s, q.dx, ix, iy, iz, colat, &ds)
                                    : rt_col2cell_2d(s, q.dx, ix, iy, colat, &ds);
        const double dc = rt_dcol(s.opacity, ds, srho[lz][ly][lx], sy_[lz][ly][lx]);
        srho[lz][ly][lx] = dc;
        scol[lz + OZ][ly + 1][lx + 1] = c2c + dc;
      }
    }
    __syncthreads();
  }

#pragma unroll
  for (int e = lane; e < TZ * TY * TX; e += 64) {
    const int ex = e % TX, ey = (e / TX) % TY, ez = e / (TX * TY);
    const int ix = rt_k_to_i(p.v[0], sidex, k0x + ex), jy2 = rt_k_to_i(p.v[1], sidey, k0y + ey),
              jz2 = rt_k_to_i(p.v[2], sidez, k0z + ez);
    if (rt_ongrid(q, ix, jy2, jz2)) {
      const long c = rt_col_id(q, ix, jy2, jz2);
      col[c] = scol[ez + OZ][ey + 1][ex + 1];
      dcol[c] = srho[ez][ey][ex];
    }
  }
}

// parallel rays along y or z: a lane per column, walked from the face the source lies beyond (decreasing index for a
// source beyond the upper face)
constexpr int PAR_WAVES = 4;
__global__ void __launch_bounds__(64 * PAR_WAVES)
k_rt_par_yz(const double *__restrict__ P, double *col, double *__restrict__ dcol, const RtGeom q, const RtSrc s,
            const int axis)
{
  // columns: (x, the other axis); x fastest
  const int nother = (axis == 1) ? q.nz : q.ny;
  const int n = (axis == 1) ? q.ny : q.nz;
  const int nseg = (q.nx + 63) / 64;
  const long u = (long)blockIdx.x * PAR_WAVES + (threadIdx.x >> 6);
  if (u >= (long)nother * nseg) return;
  const int j = (int)(u / nseg);
  const int ix = (int)(u - (long)j * nseg) * 64 + (int)(threadIdx.x & 63);
  if (ix >= q.nx) return;
  const bool up = (s.dir & 1) == 0;   // source beyond the lower face: rays run towards increasing index
  // a part: the sum starts from the plane received (the spare plane before the first cell), not from 0
  const int kb = up ? -1 : n;
  const bool recv = up ? q.glo : q.ghi;
  double N = recv ? col[rt_col_id(q, ix, (axis == 1) ? kb : j, (axis == 1) ? j : kb)] : 0.0;
  for (int m = 0; m < n; m++) {
    const int k = up ? m : n - 1 - m;
    const int iy = (axis == 1) ? k : j, iz = (axis == 1) ? j : k;
    const long c = rt_state_id(q, ix, iy, iz);
    const double y = (s.opacity == PION_RT_OPACITY_TOTAL) ? 0.0 : P[(long)s.var * q.ncell + c];
    const double dc = rt_dcol(s.opacity, q.dx, P[c], y);
    N = N + dc;
    const long o = rt_col_id(q, ix, iy, iz);
    col[o] = N;
    dcol[o] = dc;
  }
}

// parallel rays along x: a wavefront per 64 rows, blocks of PAR_XB cells of every row staged through LDS
constexpr int PAR_XB = 32;
__global__ void __launch_bounds__(64)
k_rt_par_x(const double *__restrict__ P, double *__restrict__ col, double *__restrict__ dcol, const RtGeom q,
           const RtSrc s)
{
  __shared__ double sa[64][PAR_XB + 1];   // rho, then dcol
  __shared__ double sb[64][PAR_XB + 1];   // the tracer, then col
  const long nrow = (long)q.ny * q.nz;
  const long r0 = (long)blockIdx.x * 64;
  const int lane = (int)threadIdx.x;
  const bool up = (s.dir & 1) == 0;
  const bool tracer = s.opacity != PION_RT_OPACITY_TOTAL;
  const int nblk = (q.nx + PAR_XB - 1) / PAR_XB;
  const int lx = lane % PAR_XB, lr = lane / PAR_XB;   // staging: 2 rows of 32 cells per trip
  double N = 0.0;
  for (int bm = 0; bm < nblk; bm++) {
    const int x0 = (up ? bm : nblk - 1 - bm) * PAR_XB;
    for (int rr = lr; rr < 64; rr += 64 / PAR_XB) {
      const long row = r0 + rr;
      const int ix = x0 + lx;
      double r = 0.0, y = 0.0;
      if (row < nrow && ix < q.nx) {
        const int iz = (int)(row / q.ny), iy = (int)(row - (long)iz * q.ny);
        const long c = rt_state_id(q, ix, iy, iz);
        r = P[c];
        if (tracer) y = P[(long)s.var * q.ncell + c];
      }
      sa[rr][lx] = r;
      sb[rr][lx] = y;
    }
    __syncthreads();
    if (r0 + lane < nrow) {
      for (int m = 0; m < PAR_XB; m++) {
        const int xx = up ? m : PAR_XB - 1 - m;
        if (x0 + xx < q.nx) {
          const double dc = rt_dcol(s.opacity, q.dx, sa[lane][xx], sb[lane][xx]);
          N = N + dc;
          sa[lane][xx] = dc;
          sb[lane][xx] = N;
        }
      }
    }
    __syncthreads();
    for (int rr = lr; rr < 64; rr += 64 / PAR_XB) {
      const long row = r0 + rr;
      const int ix = x0 + lx;
      if (row < nrow && ix < q.nx) {
        const long o = row * q.nx + ix;
        col[o] = sb[rr][lx];
        dcol[o] = sa[rr][lx];
      }
    }
    __syncthreads();
  }
}

__global__ void __launch_bounds__(256)
k_pack_columns(const double *__restrict__ a, unsigned long long *__restrict__ buf, const long n)
{
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  unsigned long long u;
  const double x = a[i];
  __builtin_memcpy(&u, &x, sizeof u);
  buf[i] = __builtin_bswap64(u);
}

bool grid_fits(Handle *h, const long nblk)
{
  if (nblk <= (1L << 31) - 1) return true;
  h->err = "raytrace: the grid is too large for one launch";
  return false;
}

RtTileAxis tile_axis(const RtPlan &p, const int a)
{
  RtTileAxis t;
  t.lo0 = p.klo[a][0] / p.tile[a];
  t.lo1 = p.klo[a][1] / p.tile[a];
  t.nt0 = (p.khi[a][0] >= p.klo[a][0]) ? p.khi[a][0] / p.tile[a] - t.lo0 + 1 : 0;
  t.nt1 = (p.khi[a][1] >= p.klo[a][1]) ? p.khi[a][1] / p.tile[a] - t.lo1 + 1 : 0;
  return t;
}

// workgroups of one launch of k_rt_tiles; untrimmed: counted from the vertex (khi / tile + 1 tiles per side)
long tile_workgroups(const RtPlan &p, const bool trimmed)
{
  long n = 2;
  for (int a = 1; a < 3; a++) {
    const RtTileAxis t = tile_axis(p, a);
    n *= trimmed ? t.nt0 + t.nt1 : (t.nt0 ? t.lo0 + t.nt0 : 0) + (t.nt1 ? t.lo1 + t.nt1 : 0);
  }
  return n;
}

// col points at the first on-grid plane of the source's array; the spare planes lie before and behind the on-grid ones
int trace_source(Handle *h, const RtSrc &s, const int recv_side, const double *P, double *col, double *dcol, long *launches)
{
  const RtGeom q = rt_geom(h->g, recv_side);
  if (s.at_infinity) {
    const int axis = s.dir / 2;
    if (axis == 0) {
      const long nblk = ((long)q.ny * q.nz + 63) / 64;
      if (!grid_fits(h, nblk)) return PION_GPU_EINVAL;
      hipLaunchKernelGGL(k_rt_par_x, dim3((unsigned)nblk), dim3(64), 0, h->stream, P, col, dcol, q, s);
    }
    else {
      const long nunit = (long)((axis == 1) ? q.nz : q.ny) * ((q.nx + 63) / 64);
      const long nblk = (nunit + PAR_WAVES - 1) / PAR_WAVES;
      if (!grid_fits(h, nblk)) return PION_GPU_EINVAL;
      hipLaunchKernelGGL(k_rt_par_yz, dim3((unsigned)nblk), dim3(64 * PAR_WAVES), 0, h->stream, P, col, dcol, q, s, axis);
    }
    HCHECK(h, hipGetLastError());
    *launches += 1;
    return 0;
  }
  const RtPlan p = rt_plan_of(h->g.ndim, h->g.ng, s);
  if (h->rt->levels) {
    const long nblk = (2L * q.ny * q.nz + 255) / 256;
    if (!grid_fits(h, nblk)) return PION_GPU_EINVAL;
    for (long L = p.level_lo; L <= p.level_hi; L++)
      hipLaunchKernelGGL(k_rt_levels, dim3((unsigned)nblk), dim3(256), 0, h->stream, P, col, dcol, q, s, L);
    HCHECK(h, hipGetLastError());
    *launches += p.level_hi - p.level_lo + 1;
    return 0;
  }
  const RtTileAxis ay = tile_axis(p, 1), az = tile_axis(p, 2);
  const long nblk = 2L * (ay.nt0 + ay.nt1) * (az.nt0 + az.nt1);
  if (nblk == 0) return 0;
  if (!grid_fits(h, nblk)) return PION_GPU_EINVAL;
  for (long T = p.tlevel_lo; T <= p.tlevel_hi; T++) {
    if (h->g.ndim == 3)
      hipLaunchKernelGGL((k_rt_tiles<RT_TILE3[0], RT_TILE3[1], RT_TILE3[2]>), dim3((unsigned)nblk), dim3(64), 0, h->stream,
                         P, col, dcol, q, s, p, ay, az, T);
    else
      hipLaunchKernelGGL((k_rt_tiles<RT_TILE2[0], RT_TILE2[1], RT_TILE2[2]>), dim3((unsigned)nblk), dim3(64), 0, h->stream,
                         P, col, dcol, q, s, p, ay, az, T);
  }
  HCHECK(h, hipGetLastError());
  *launches += p.tlevel_hi - p.tlevel_lo + 1;
  return 0;
}

int slab_planes(const Handle *h) { return h->g.ng[h->g.ndim - 1]; }
long plane_cells(const Handle *h) { return (h->g.ndim == 3) ? (long)h->g.ng[0] * h->g.ng[1] : (long)h->g.ng[0]; }

double *rt_col_of(const Handle *h, const int id) { return h->rt->dcols[id] + plane_cells(h); }
double *rt_dcol_of(const Handle *h, const int id) { return h->rt->dcols[id] + 2 * plane_cells(h) + rt_geom(h->g).n; }

// id and `what` of a column array, or null with the text set
double *column_array(Handle *h, const int id, const int what)
{
  if (!h->rt || id < 0 || id >= (int)h->rt->src.size() || what < 0 || what > 1) {
    h->err = "raytrace: no such source or array (what: 0 col, 1 dcol)";
    return nullptr;
  }
  return what ? rt_dcol_of(h, id) : rt_col_of(h, id);
}

}  // namespace

void impl::rt_free(Handle *h)
{
  if (!h->rt) return;
  for (double *d : h->rt->dcols) (void)hipFree(d);
  delete h->rt;
  h->rt = nullptr;
}

static int raytrace_host(const pion_gpu_config *cfg, const pion_gpu_rt_source *src, const pion_gpu_rt_part *part,
                         const double *P_soa, const double *face_in, double *col_out, double *dcol);

extern "C" {

const char *pion_gpu_rt_refused(const pion_gpu_config *cfg, const pion_gpu_rt_source *src)
{
  if (!cfg) return "raytrace: no configuration";
  if (cfg->ndim < 1 || cfg->ndim > 3 || cfg->nbc < 0 || cfg->ntracer < 0 || cfg->ntracer > cfg->nvar || !(cfg->dx > 0.0))
    return "raytrace: malformed configuration";
  for (int a = 0; a < cfg->ndim; a++)
    if (cfg->ng[a] < 1) return "raytrace: malformed configuration";
  return rt_refused(*cfg, src);
}

const char *pion_gpu_rt_part_refused(const pion_gpu_config *cfg, const pion_gpu_rt_source *src, const pion_gpu_rt_part *part)
{
  if (!cfg) return "raytrace: no configuration";
  if (cfg->ndim < 1 || cfg->ndim > 3 || cfg->nbc < 0 || cfg->ntracer < 0 || cfg->ntracer > cfg->nvar || !(cfg->dx > 0.0))
    return "raytrace: malformed configuration";
  for (int a = 0; a < cfg->ndim; a++)
    if (cfg->ng[a] < 1) return "raytrace: malformed configuration";
  return rt_part_refused(*cfg, src, part);
}

static int add_source(Handle *h, const pion_gpu_rt_source *src, const pion_gpu_rt_part *part, int *id, double *pos_used)
{
  if (h->rt && h->rt->src.size() >= PION_MAX_RT_SOURCES) {
    h->err = "raytrace: more than PION_MAX_RT_SOURCES (4) sources";
    return PION_GPU_EINVAL;
  }
  double *d = nullptr;
  const size_t bytes = sizeof(double) * (2 * (size_t)rt_geom(h->g).n + 2 * (size_t)plane_cells(h));
  if (hipMalloc((void **)&d, bytes) != hipSuccess) {
    h->err = "raytrace: no device memory for the column arrays";
    return PION_GPU_ENOMEM;
  }
  HCHECK(h, hipMemsetAsync(d, 0, bytes, h->stream));
  if (!h->rt) {
    h->rt = new RtState;
    if (const char *e = getenv("PION_RT_KERNEL")) h->rt->levels = (strcmp(e, "levels") == 0) ? 1 : 0;
  }
  h->rt->src.push_back(rt_make_source(h->cfg, *src, pos_used, part));
  h->rt->dcols.push_back(d);
  h->rt->part.push_back(part ? 1 : 0);
  const RtRole none = {PION_RT_RECV_NONE, 0, 0};
  h->rt->role.push_back(part ? rt_role(h->cfg, *src, *part) : none);
  if (id) *id = (int)h->rt->src.size() - 1;
  return 0;
}

int pion_gpu_add_rt_source(void *handle, const pion_gpu_rt_source *src, int *id, double *pos_used)
{
  Handle *h = use(handle);
  if (!h) return PION_GPU_EINVAL;
  if (const char *e = pion_gpu_rt_refused(&h->cfg, src)) {
    h->err = e;
    return PION_GPU_EINVAL;
  }
  return add_source(h, src, nullptr, id, pos_used);
}

int pion_gpu_add_rt_source_part(void *handle, const pion_gpu_rt_source *src, const pion_gpu_rt_part *part, int *id,
                                double *pos_used)
{
  Handle *h = use(handle);
  if (!h) return PION_GPU_EINVAL;
  if (const char *e = pion_gpu_rt_part_refused(&h->cfg, src, part)) {
    h->err = e;
    return PION_GPU_EINVAL;
  }
  return add_source(h, src, part, id, pos_used);
}

int pion_gpu_rt_chain(const pion_gpu_config *cfg, const pion_gpu_rt_source *src, const pion_gpu_rt_part *part,
                      int *recv_side, int *send_lo, int *send_hi)
{
  if (pion_gpu_rt_part_refused(cfg, src, part)) return PION_GPU_EINVAL;
  const RtRole r = rt_role(*cfg, *src, *part);
  if (recv_side) *recv_side = r.recv_side;
  if (send_lo) *send_lo = r.send_lo;
  if (send_hi) *send_hi = r.send_hi;
  return 0;
}

static bool has_slab_face(const Handle *h)
{
  for (int d = 0; d < 2 * h->cfg.ndim; d++)
    if (h->cfg.bc_type[d] == PION_BC_SLAB) return true;
  return false;
}

int pion_gpu_raytrace(void *handle, int which)
{
  Handle *h = use(handle);
  if (!h) return PION_GPU_EINVAL;
  if (!h->rt) return 0;
  if (which < 0 || which > 1) {
    h->err = "raytrace: which is 0 (P) or 1 (Ph)";
    return PION_GPU_EINVAL;
  }
  if (has_slab_face(h)) {
    h->err = "raytrace: a slab of a decomposed run is traced source by source with the planes of its neighbours (pion_gpu_raytrace_part)";
    return PION_GPU_EINVAL;
  }
  const double *P = (which == 1 && h->ph_valid) ? h->dPh : h->dP;
  long launches = 0;
  for (size_t i = 0; i < h->rt->src.size(); i++)
    if (int rc = trace_source(h, h->rt->src[i], PION_RT_RECV_NONE, P, rt_col_of(h, (int)i), rt_dcol_of(h, (int)i), &launches))
      return rc;
  return 0;
}

int pion_gpu_raytrace_part(void *handle, int which, int id, const void *dface_in, void *dface_out_lo, void *dface_out_hi)
{
  Handle *h = use(handle);
  if (!h) return PION_GPU_EINVAL;
  if (which < 0 || which > 1) {
    h->err = "raytrace: which is 0 (P) or 1 (Ph)";
    return PION_GPU_EINVAL;
  }
  if (!column_array(h, id, 0)) return PION_GPU_EINVAL;
  if (!h->rt->part[id] && has_slab_face(h)) {   // (cannot happen: such a source is refused when it is added)
    h->err = "raytrace: the source was added without a part";
    return PION_GPU_EINVAL;
  }
  const RtRole role = h->rt->role[id];
  if (role.recv_side != PION_RT_RECV_NONE && !dface_in) {
    h->err = "raytrace: the source's chain hands this part a plane, and there is no buffer of it";
    return PION_GPU_EINVAL;
  }
  const double *P = (which == 1 && h->ph_valid) ? h->dPh : h->dP;
  const size_t pbytes = sizeof(double) * (size_t)plane_cells(h);
  const long n = rt_geom(h->g).n, pc = plane_cells(h);
  double *col = rt_col_of(h, id);
  // the received plane goes into the spare plane beyond the face that looks towards the source
  if (role.recv_side == PION_RT_RECV_BELOW)
    HCHECK(h, hipMemcpyAsync(col - pc, dface_in, pbytes, hipMemcpyDeviceToDevice, h->stream));
  if (role.recv_side == PION_RT_RECV_ABOVE)
    HCHECK(h, hipMemcpyAsync(col + n, dface_in, pbytes, hipMemcpyDeviceToDevice, h->stream));
  long launches = 0;
  if (int rc = trace_source(h, h->rt->src[id], role.recv_side, P, col, rt_dcol_of(h, id), &launches)) return rc;
  // the rank's lowest and highest own plane, for the neighbours
  if (dface_out_lo) HCHECK(h, hipMemcpyAsync(dface_out_lo, col, pbytes, hipMemcpyDeviceToDevice, h->stream));
  if (dface_out_hi) HCHECK(h, hipMemcpyAsync(dface_out_hi, col + n - pc, pbytes, hipMemcpyDeviceToDevice, h->stream));
  return 0;
}

long pion_gpu_rt_count(void *handle, int planes)
{
  Handle *h = use(handle);
  if (!h || planes < 0 || h->g.ndim < 2) return 0;
  return planes * plane_cells(h);
}

int pion_gpu_rt_columns(void *handle, int id, int what, double *host)
{
  Handle *h = use(handle);
  if (!h) return PION_GPU_EINVAL;
  const double *a = column_array(h, id, what);
  if (!a) return PION_GPU_EINVAL;
  if (!host) {
    h->err = "raytrace: no host array";
    return PION_GPU_EINVAL;
  }
  HCHECK(h, hipMemcpyAsync(host, a, sizeof(double) * (size_t)rt_geom(h->g).n, hipMemcpyDeviceToHost, h->stream));
  HCHECK(h, hipStreamSynchronize(h->stream));
  return 0;
}

int pion_gpu_pack_columns(void *handle, int id, int what, int plane_lo, int plane_hi, void *dbuf)
{
  Handle *h = use(handle);
  if (!h) return PION_GPU_EINVAL;
  const double *a = column_array(h, id, what);
  if (!a) return PION_GPU_EINVAL;
  if (!dbuf || plane_lo < 0 || plane_hi > slab_planes(h) || plane_lo >= plane_hi) {
    h->err = "pack_columns: plane range outside the grid, or no buffer";
    return PION_GPU_EINVAL;
  }
  const long pc = plane_cells(h), n = (plane_hi - plane_lo) * pc;
  const long nblk = (n + 255) / 256;
  if (!grid_fits(h, nblk)) return PION_GPU_EINVAL;
  hipLaunchKernelGGL(k_pack_columns, dim3((unsigned)nblk), dim3(256), 0, h->stream, a + plane_lo * pc,
                     (unsigned long long *)dbuf, n);
  HCHECK(h, hipGetLastError());
  return 0;
}

int pion_gpu_rt_plan(const pion_gpu_config *cfg, const pion_gpu_rt_source *src, int tile[3], long *launches, long *levels)
{
  if (pion_gpu_rt_refused(cfg, src)) return PION_GPU_EINVAL;
  const RtSrc s = rt_make_source(*cfg, *src, nullptr);
  int ng[3];
  for (int a = 0; a < 3; a++) ng[a] = (a < cfg->ndim) ? cfg->ng[a] : 1;
  if (s.at_infinity) {
    for (int a = 0; a < 3 && tile; a++) tile[a] = 0;
    if (launches) *launches = 1;
    if (levels) *levels = 1;
    return 0;
  }
  const RtPlan p = rt_plan_of(cfg->ndim, ng, s);
  for (int a = 0; a < 3 && tile; a++) tile[a] = p.tile[a];
  if (launches) *launches = p.tlevel_hi - p.tlevel_lo + 1;
  if (levels) *levels = p.level_hi - p.level_lo + 1;
  return 0;
}

int pion_gpu_rt_plan_part(const pion_gpu_config *cfg, const pion_gpu_rt_source *src, const pion_gpu_rt_part *part,
                          long *launches, long *workgroups, long *workgroups_from_vertex)
{
  if (pion_gpu_rt_part_refused(cfg, src, part)) return PION_GPU_EINVAL;
  const RtSrc s = rt_make_source(*cfg, *src, nullptr, part);
  int ng[3];
  for (int a = 0; a < 3; a++) ng[a] = (a < cfg->ndim) ? cfg->ng[a] : 1;
  long l = 1, w = 0, w0 = 0;
  if (!s.at_infinity) {
    const RtPlan p = rt_plan_of(cfg->ndim, ng, s);
    l = p.tlevel_hi - p.tlevel_lo + 1;
    w = tile_workgroups(p, true);
    w0 = tile_workgroups(p, false);
  }
  if (launches) *launches = l;
  if (workgroups) *workgroups = w;
  if (workgroups_from_vertex) *workgroups_from_vertex = w0;
  return 0;
}

int pion_gpu_raytrace_host(const pion_gpu_config *cfg, const pion_gpu_rt_source *src, const double *P_soa, double *col,
                           double *dcol)
{
  if (pion_gpu_rt_refused(cfg, src)) return PION_GPU_EINVAL;
  return raytrace_host(cfg, src, nullptr, P_soa, nullptr, col, dcol);
}

int pion_gpu_raytrace_host_part(const pion_gpu_config *cfg, const pion_gpu_rt_source *src, const pion_gpu_rt_part *part,
                                const double *P_soa, const double *face_in, double *col, double *dcol)
{
  if (pion_gpu_rt_part_refused(cfg, src, part)) return PION_GPU_EINVAL;
  return raytrace_host(cfg, src, part, P_soa, face_in, col, dcol);
}

}  // extern "C"

// the host loop of both: col and dcol hold the on-grid cells only; with a part the columns are traced in an array that
// has the two spare planes and copied out
static int raytrace_host(const pion_gpu_config *cfg, const pion_gpu_rt_source *src, const pion_gpu_rt_part *part,
                         const double *P_soa, const double *face_in, double *col_out, double *dcol)
{
  if (!P_soa || !col_out || !dcol) return PION_GPU_EINVAL;
  GridDesc g;
  g.ndim = cfg->ndim;
  g.ncell = 1;
  for (int a = 0; a < 3; a++) {
    g.ng[a] = (a < cfg->ndim) ? cfg->ng[a] : 1;
    g.nbc[a] = (a < cfg->ndim) ? cfg->nbc : 0;
    g.nga[a] = g.ng[a] + 2 * g.nbc[a];
    g.ncell *= g.nga[a];
  }
  g.sy = g.nga[0];
  g.sz = (long)g.nga[0] * g.nga[1];
  g.dx = cfg->dx;
  const RtRole none = {PION_RT_RECV_NONE, 0, 0};
  const RtRole role = part ? rt_role(*cfg, *src, *part) : none;
  if (role.recv_side != PION_RT_RECV_NONE && !face_in) return PION_GPU_EINVAL;
  const RtGeom q = rt_geom(g, role.recv_side);
  const RtSrc s = rt_make_source(*cfg, *src, nullptr, part);
  const long pc = (g.ndim == 3) ? (long)g.ng[0] * g.ng[1] : (long)g.ng[0];
  std::vector<double> with_spares;
  double *col = col_out;
  if (role.recv_side != PION_RT_RECV_NONE) {
    with_spares.assign((size_t)(q.n + 2 * pc), 0.0);
    col = with_spares.data() + pc;
    memcpy(role.recv_side == PION_RT_RECV_BELOW ? col - pc : col + q.n, face_in, sizeof(double) * (size_t)pc);
  }
  const auto finish = [&]() {
    if (col != col_out) memcpy(col_out, col, sizeof(double) * (size_t)q.n);
    return 0;
  };
  if (s.at_infinity) {
    // trace_parallel_rays: every column of the axis, cell after cell from the face the source lies beyond
    const int axis = s.dir / 2, n = g.ng[axis];
    const bool up = (s.dir & 1) == 0;
    int i[3];
    const int a1 = (axis + 1) % 3, a2 = (axis + 2) % 3;
    for (i[a2] = 0; i[a2] < g.ng[a2]; i[a2]++)
      for (i[a1] = 0; i[a1] < g.ng[a1]; i[a1]++) {
        i[axis] = up ? -1 : n;
        double N = (axis == g.ndim - 1 && (up ? q.glo : q.ghi)) ? col[rt_col_id(q, i[0], i[1], i[2])] : 0.0;
        for (int m = 0; m < n; m++) {
          i[axis] = up ? m : n - 1 - m;
          const long c = rt_state_id(q, i[0], i[1], i[2]);
          const double y = (s.opacity == PION_RT_OPACITY_TOTAL) ? 0.0 : P_soa[(long)s.var * q.ncell + c];
          const double dc = rt_dcol(s.opacity, q.dx, P_soa[c], y);
          N = N + dc;
          const long o = rt_col_id(q, i[0], i[1], i[2]);
          col[o] = N;
          dcol[o] = dc;
        }
      }
    return finish();
  }
  // octant by octant, outwards from the source: one valid order among the many the dependency admits
  const RtPlan p = rt_plan_of(g.ndim, g.ng, s);
  const ColGlobal colat = {col, &q};
  for (int oct = 0; oct < 8; oct++) {
    const int sx = oct & 1, sy = (oct >> 1) & 1, sz = (oct >> 2) & 1;
    for (int kz = p.klo[2][sz]; kz <= p.khi[2][sz]; kz++)
      for (int ky = p.klo[1][sy]; ky <= p.khi[1][sy]; ky++)
        for (int kx = p.klo[0][sx]; kx <= p.khi[0][sx]; kx++) {
          const int ix = rt_k_to_i(p.v[0], sx, kx), iy = rt_k_to_i(p.v[1], sy, ky), iz = rt_k_to_i(p.v[2], sz, kz);
          const long o = rt_col_id(q, ix, iy, iz);
          rt_cell(P_soa, q, s, ix, iy, iz, colat, &col[o], &dcol[o]);
        }
  }
  return finish();
}
