// kernels_prepass.hip -- the pre-pass of a stage: the HLLD -> HLL switch per cell (div v < 0 && |grad p|/p > 5,
// solver_eqn_base.cpp:398-412) in its dense, row, marching and screened (hll_screen.h) forms, and the H-correction
// eta (calc_Hcorrection :423-570).  Nothing here depends on the equation set.
//
// Compiled twice (Makefile): -DPION_FPNS=fp_strict -ffp-contract=off and -DPION_FPNS=fp_fast -ffp-contract=fast.
#include "dev_cooling.h"
#include "kernels.h"

#ifndef PION_FPNS
#error "PION_FPNS must be defined (fp_strict or fp_fast)"
#endif

namespace pion {
namespace PION_FPNS {

#include "dev_sweep.h"

// ---------------------------------------------------------------------------
// pre-pass: HLLD switch and H-correction.  One thread per cell INCLUDING ghosts
// (the reference loops FirstPt_All..NextPt_All, solver_eqn_base.cpp:400-412).
// ---------------------------------------------------------------------------
// the switch of one cell i (all-cell indices): shared by k_prepass_hlld and k_prepass_hlld_blocks
PDEV void prepass_hlld_cell(const PrepassArgs &a, const int *i);

__global__ __launch_bounds__(256) void k_prepass_hlld(const PrepassArgs a)
{
  // 3-D launch (64 x 4 threads; grid = x tiles, y tiles, planes of [c0,c1)): the cell coordinates come
  // from the block and thread indices -- the flat-index form spent more on 64-bit div/mod than on physics
  // Workgroups are dealt round-robin to the 8 XCDs, each with its own L2: give every XCD a contiguous
  // range of (x,y,z) tiles (z slowest) so that the y and z neighbours it reads are lines its own L2 holds
  const long nc = a.g.ncell;
  const unsigned gx = (a.g.nga[0] + 63) / 64, gy = (a.g.nga[1] + 3) / 4;
  const long plane = (long)a.g.nga[0] * a.g.nga[1];
  const unsigned npl1 = (unsigned)((a.c1 - a.c0) / plane);
  const unsigned npl = npl1 + ((a.c3 > a.c2) ? (unsigned)((a.c3 - a.c2) / plane) : 0u);
  const unsigned ntile = gx * gy * npl;
  const unsigned t = (unsigned)xcd_tile(blockIdx.x, ntile);
  if (t >= ntile) return;
  int i[3];
  i[0] = (int)((t % gx) * 64 + (threadIdx.x & 63));
  i[1] = (int)(((t / gx) % gy) * 4 + (threadIdx.x >> 6));
  const unsigned pz = t / (gx * gy);
  i[2] = (pz < npl1) ? (int)(a.c0 / plane) + (int)pz : (int)(a.c2 / plane) + (int)(pz - npl1);
  if (i[0] >= a.g.nga[0] || i[1] >= a.g.nga[1]) return;
  prepass_hlld_cell(a, i);
}

// 2-D grids, a part of a split stage: the cells of all-cell rows [c0, c1) / nga[0] and, if c3 > c2, [c2, c3) / nga[0]
// (whole rows, x ghosts included), 64 x 4 threads per workgroup
__global__ __launch_bounds__(256) void k_prepass_hlld_rows(const PrepassArgs a)
{
  const long row = a.g.nga[0];
  const unsigned gx = (a.g.nga[0] + 63) / 64;
  const unsigned nr1 = (unsigned)((a.c1 - a.c0) / row);
  const unsigned nr = nr1 + ((a.c3 > a.c2) ? (unsigned)((a.c3 - a.c2) / row) : 0u);
  const unsigned t = blockIdx.x;
  int i[3];
  i[0] = (int)((t % gx) * 64 + (threadIdx.x & 63));
  const unsigned r = (t / gx) * 4 + (threadIdx.x >> 6);
  if (i[0] >= a.g.nga[0] || r >= nr) return;
  i[1] = (r < nr1) ? (int)(a.c0 / row) + (int)r : (int)(a.c2 / row) + (int)(r - nr1);
  i[2] = 0;
  prepass_hlld_cell(a, i);
}

PDEV void prepass_hlld_cell(const PrepassArgs &a, const int *i)
{
  const long nc = a.g.ncell;
  const long c = (long)i[0] + a.g.sy * i[1] + a.g.sz * i[2];
  const double dx = a.g.dx;
  // The switch is (div v < 0 && grad > 5): the pressure term decides for almost every cell (grad > 5 only
  // in strong shocks), so it is evaluated first and the three velocity arrays are read only where it can
  // matter -- the same flags from a quarter of the memory traffic.
  // ... and the pressure term itself is screened without its divisions: if |dp| <= 1.6 min(p-, p+) on every
  // axis the sum of the (at most three) quotients is <= 4.8 (1 + a few ulp) < 5 and the flag is 0 whatever
  // the exact value; only the other cells (and the debug outputs) pay for the divisions.
  double divv = 0.0, gradp = 0.0;
  double pp3[3], pn3[3];
  bool steep = (a.gradp != nullptr);
  for (int v = 0; v < a.g.ndim; v++) {
    const long st = (v == 0) ? 1 : ((v == 1) ? a.g.sy : a.g.sz);
    const long n = (i[v] > 0) ? c - st : c;
    const long p = (i[v] < a.g.nga[v] - 1) ? c + st : c;
    pp3[v] = a.S[1 * nc + p];
    pn3[v] = a.S[1 * nc + n];
    if (!(fabs(pp3[v] - pn3[v]) <= 1.6 * fmin(pp3[v], pn3[v]))) steep = true;   // (NaN counts as steep)
  }
  if (steep) {
    // GradZone (VectorOps.cpp:322-368) on the pressure
    for (int v = 0; v < a.g.ndim; v++) gradp += fabs(pp3[v] - pn3[v]) / fmin(pp3[v], pn3[v]);
  }
  if (gradp > 5. || a.divv) {
    for (int v = 0; v < a.g.ndim; v++) {
      const long st = (v == 0) ? 1 : ((v == 1) ? a.g.sy : a.g.sz);
      // Divergence (VectorOps.cpp:377-439): missing neighbour -> this cell, one-sided dx
      const long n = (i[v] > 0) ? c - st : c;
      const long p = (i[v] < a.g.nga[v] - 1) ? c + st : c;
      const double ddx = (n == c || p == c) ? dx : 2.0 * dx;
      if (a.g.cyl == 1 && v == 1) {
        // VectorOps_Cyl::Divergence (VectorOps.cpp:891-972): d(R V_R)/(R dR) between the neighbours' centres of mass
        const double rn = cyl_Rcom(cyl_R(a.g, (n == c) ? i[1] : i[1] - 1), dx);
        const double rp = cyl_Rcom(cyl_R(a.g, (p == c) ? i[1] : i[1] + 1), dx);
        divv += 2.0 * (rp * a.S[(2 + v) * nc + p] - rn * a.S[(2 + v) * nc + n]) / (rp * rp - rn * rn);
      }
      else divv += (a.S[(2 + v) * nc + p] - a.S[(2 + v) * nc + n]) / ddx;
    }
  }
  if (a.divv) a.divv[c] = divv;
  if (a.gradp) a.gradp[c] = gradp;
  // solver_eqn_mhd_adi.cpp:171: (DivV<0 && Grad>5) of either cell switches the interface to HLL
  a.hllflag[c] = (divv < 0. && gradp > 5.) ? 1 : 0;
}

// The same flags, one thread per (x,y) column of a chunk of PION_PREPASS_ZC planes (3-D Cartesian grids, whole
// plane ranges): the pressure of planes k-1, k, k+1 is carried in registers, so each plane of p is read once
// (+ 2 halo planes per chunk) instead of three times from beyond L2, and -- as in k_prepass_hlld -- the pressure
// term is screened without divisions and the velocities are read only in steep cells.
#define PION_PREPASS_ZC 16
__global__ __launch_bounds__(256) void k_prepass_hlld_march(const PrepassArgs a)
{
  const long nc = a.g.ncell;
  // x: 62 cells per wavefront; lanes 0 and 63 only supply their neighbours' x-1 / x+1 pressure through wavefront
  // shuffles (no loads for the x neighbours)
  const unsigned gx = (a.g.nga[0] + 61) / 62, gy = (a.g.nga[1] + 3) / 4;
  const long plane = (long)a.g.nga[0] * a.g.nga[1];
  const int kz0 = (int)(a.c0 / plane), kz1 = (int)(a.c1 / plane);
  const unsigned nch = (unsigned)((kz1 - kz0 + PION_PREPASS_ZC - 1) / PION_PREPASS_ZC);
  const unsigned ntile = gx * gy * nch;
  const unsigned t = (unsigned)xcd_tile(blockIdx.x, ntile);
  if (t >= ntile) return;
  const int lane = (int)(threadIdx.x & 63);
  int ix = (int)((t % gx) * 62) - 1 + lane;
  const bool xwriter = (lane >= 1 && lane <= 62 && ix < a.g.nga[0]);
  if (ix < 0) ix = 0;
  if (ix > a.g.nga[0] - 1) ix = a.g.nga[0] - 1;
  const int iy = (int)(((t / gx) % gy) * 4 + (threadIdx.x >> 6));
  const int k0 = kz0 + (int)(t / (gx * gy)) * PION_PREPASS_ZC;
  const int k1 = (k0 + PION_PREPASS_ZC < kz1) ? k0 + PION_PREPASS_ZC : kz1;
  if (iy >= a.g.nga[1]) return;   // (whole wavefront: iy is uniform)
  const long sy = a.g.sy, sz = a.g.sz;
  const double dx = a.g.dx;
  const double *P = a.S + 1 * nc;
  const bool xl = ix > 0, xh = ix < a.g.nga[0] - 1, yl = iy > 0, yh = iy < a.g.nga[1] - 1;
  // Addressing as in k_stage_rows2: uniform base (the pressure array, moved by the scalar unit from plane to
  // plane) + one 32-bit byte offset per lane and neighbour.  A cell on a face of the array takes itself for the
  // missing neighbour (the reference's one-sided difference): its neighbour offset IS its own offset, so the
  // loop has neither selects nor branches for the faces.  (launch_prepass uses this kernel only while 8 ncell
  // fits 32 bits.)
  const unsigned cb = (unsigned)((long)ix + sy * iy);   // cell inside a plane
  const unsigned o0 = cb * 8u;
  const unsigned oym = yl ? o0 - (unsigned)sy * 8u : o0, oyp = yh ? o0 + (unsigned)sy * 8u : o0;
  const char *Pk = reinterpret_cast<const char *>(P) + sz * 8 * k0;   // plane k (uniform)
  char *Hk = reinterpret_cast<char *>(a.hllflag) + sz * k0;
  double p0 = ldu(Pk, o0), pm = (k0 > 0) ? ldu(Pk - sz * 8, o0) : p0;
  for (int k = k0; k < k1; k++, Pk += sz * 8, Hk += sz) {
    const bool zl = k > 0, zh = k < a.g.nga[2] - 1;
    const unsigned q0 = pin_v(o0), qym = pin_v(oym), qyp = pin_v(oyp);
    const double pz = zh ? ldu(Pk + sz * 8, q0) : p0;
    double pn3[3], pp3[3];
    // x neighbours from the neighbouring lanes (a cell on an x face of the array takes itself; the halo lanes'
    // own results are not written)
    const double pl_ = lane_prev(p0), pr_ = lane_next(p0);
    pn3[0] = xl ? pl_ : p0;
    pp3[0] = xh ? pr_ : p0;
    pn3[1] = ldu(Pk, qym);
    pp3[1] = ldu(Pk, qyp);
    pn3[2] = zl ? pm : p0;
    pp3[2] = pz;
    // |pp - pn| <= 1.6 min(pp, pn), as two comparisons (a NaN fails both and counts as steep, as before)
    bool steep = false;
#pragma unroll
    for (int v = 0; v < 3; v++) {
      const double d = fabs(pp3[v] - pn3[v]);
      if (!(d <= 1.6 * pp3[v]) || !(d <= 1.6 * pn3[v])) steep = true;
    }
    uint8_t flag = 0;
    if (steep) {
      double gradp = 0.0, divv = 0.0;
      for (int v = 0; v < 3; v++) gradp += fabs(pp3[v] - pn3[v]) / fmin(pp3[v], pn3[v]);   // GradZone
      if (gradp > 5.) {
        // (rare: the cell's index is only formed here)
        const long c = (long)cb + sz * ((long)k + opaque_zero());
        const bool lo[3] = {xl, yl, zl}, hi[3] = {xh, yh, zh};
        for (int v = 0; v < 3; v++) {
          const long st = (v == 0) ? 1 : ((v == 1) ? sy : sz);
          const long n = lo[v] ? c - st : c, p = hi[v] ? c + st : c;
          const double ddx = (n == c || p == c) ? dx : 2.0 * dx;
          divv += (a.S[(2 + v) * nc + p] - a.S[(2 + v) * nc + n]) / ddx;   // Divergence (VectorOps.cpp:377-439)
        }
        flag = (divv < 0.) ? 1 : 0;
      }
    }
    if (xwriter) stub(Hk, pin_v(cb), flag);
    pm = p0;
    p0 = pz;
  }
}

// eta of interface (c | c+st) along each axis, stored at c (calc_Hcorrection; the last cell of a
// column gets no value and keeps 0; first/last cells of a column have zero slope)
template <int NVMAX>
__global__ __launch_bounds__(256) void k_prepass_hcorr(const PrepassArgs a)
{
  const long c = a.c0 + (long)blockIdx.x * blockDim.x + threadIdx.x;
  const long nc = a.g.ncell;
  if (c >= a.c1) return;
  int i[3];
  i[0] = (int)(c % a.g.nga[0]);
  i[1] = (int)((c / a.g.nga[0]) % a.g.nga[1]);
  i[2] = (int)(c / ((long)a.g.nga[0] * a.g.nga[1]));
  const double dx = a.g.dx, g = a.gamma;
  const bool mhd = (a.eqntype != EQEUL);
  const bool oa2 = (a.space_ooa == 2);
  for (int ax = 0; ax < a.g.ndim; ax++) {
    const long st = (ax == 0) ? 1 : ((ax == 1) ? a.g.sy : a.g.sz);
    const int n = a.g.nga[ax], k = i[ax];
    double eta = 0.0;
    if (k < n - 1) {
      // sweep-frame variables needed by maxspeed and v_n: rho, p, v_n, (B_n, B_t1, B_t2)
      double eL[8], eR[8];
      const int nvs = mhd ? 8 : 5;
      for (int s = 0; s < 8; s++) {
        if (s >= nvs) {
          eL[s] = eR[s] = 0.0;
          continue;
        }
        const double *b = a.S + (long)(mhd ? rotvar<true>(ax, s) : rotvar<false>(ax, s)) * nc + c;
        const double q0 = b[0], q1 = b[st];
        double s0 = 0.0, s1 = 0.0;
        if (oa2 && a.g.cyl == 2) {
          // VectorOps_Sph::SetSlope / SetEdgeState (VectorOps_spherical.cpp:294-440); k = all-cell R index
          const double R0 = sph_R(a.g, k), R1 = sph_R(a.g, k + 1);
          const double c0 = sph_Rcom(R0, dx), c1 = sph_Rcom(R1, dx);
          if (k > 0) s0 = avg_falle((q0 - b[-st]) / (c0 - sph_Rcom(sph_R(a.g, k - 1), dx)), (q1 - q0) / (c1 - c0));
          if (k + 1 < n - 1) s1 = avg_falle((q1 - q0) / (c1 - c0), (b[2 * st] - q1) / (sph_Rcom(sph_R(a.g, k + 2), dx) - c1));
          eL[s] = q0 + s0 * (R0 + 0.5 * dx - c0);
          eR[s] = q1 + s1 * (R1 - 0.5 * dx - c1);
        }
        else if (oa2 && a.g.cyl == 1 && ax == 1) {
          // VectorOps_Cyl::SetSlope / SetEdgeState along R (VectorOps.cpp:1052-1204); k = all-cell R index
          const double R0 = cyl_R(a.g, k), R1 = cyl_R(a.g, k + 1);
          const double c0 = cyl_Rcom(R0, dx), c1 = cyl_Rcom(R1, dx);
          if (k > 0) s0 = avg_falle((q0 - b[-st]) / (c0 - cyl_Rcom(cyl_R(a.g, k - 1), dx)), (q1 - q0) / (c1 - c0));
          if (k + 1 < n - 1) s1 = avg_falle((q1 - q0) / (c1 - c0), (b[2 * st] - q1) / (cyl_Rcom(cyl_R(a.g, k + 2), dx) - c1));
          eL[s] = q0 + s0 * (R0 + dx * 0.5 - c0);
          eR[s] = q1 + s1 * (R1 - dx * 0.5 - c1);
        }
        else if (oa2) {
          if (k > 0) s0 = avg_falle((q0 - b[-st]) / dx, (q1 - q0) / dx);   // first cell: zero slope
          if (k + 1 < n - 1) s1 = avg_falle((q1 - q0) / dx, (b[2 * st] - q1) / dx);  // last cell: zero slope
          eL[s] = q0 + s0 * dx * 0.5;
          eR[s] = q1 - s1 * dx * 0.5;
        }
        else {
          eL[s] = q0;
          eR[s] = q1;
        }
      }
      // set_Hcorrection (solver_eqn_base.cpp:579-599)
      double msL, msR;
      if (mhd) {
        msL = Eqn<EQMHD, 0>::cfast(eL, g);
        msR = Eqn<EQMHD, 0>::cfast(eR, g);
      }
      else {
        msL = Eqn<EQEUL, 0>::chydro(eL, g);
        msR = Eqn<EQEUL, 0>::chydro(eR, g);
      }
      eta = 0.5 * (fabs(eR[qVN] - eL[qVN]) + fabs(msR - msL));
    }
    a.eta[ax * nc + c] = eta;
  }
}

// Screened prepass (hll_screen.h).  k_prepass_screen: one thread per block of the summary the last stage kernel left of
// a.S; a block whose 3 x 3 x 3 neighbourhood is not provably calm goes onto the list of active blocks.
__global__ __launch_bounds__(256) void k_prepass_screen(const PrepassArgs a)
{
  const long nblk = scr_total(a.scr);
  const long t = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= nblk) return;
  const int bx = (int)(t % a.scr.nb[0]), by = (int)((t / a.scr.nb[0]) % a.scr.nb[1]);
  const int bz = (int)(t / ((long)a.scr.nb[0] * a.scr.nb[1]));
  if (!scr_block_quiet(a.scr, a.hsum, a.hsum + nblk, bx, by, bz)) a.scr_list[atomicAdd(a.scr_count, 1)] = (int)t;
}
// k_prepass_hlld_blocks: k_prepass_hlld's cell code on the cells of the listed blocks (the flags of all other cells were
// cleared); a block on a face of the grid also takes the ghost cells beyond it.  A fixed grid strides over the list,
// whose length stays on the device.  One wavefront per x row of the block.
__global__ __launch_bounds__(256) void k_prepass_hlld_blocks(const PrepassArgs a)
{
  const int n = *a.scr_count;
  for (int e = (int)blockIdx.x; e < n; e += (int)gridDim.x) {
    const int t = a.scr_list[e];
    const int bx = t % a.scr.nb[0], by = (t / a.scr.nb[0]) % a.scr.nb[1], bz = t / (a.scr.nb[0] * a.scr.nb[1]);
    int lo[3], hi[3];
    scr_cells_ext(a.scr, 0, bx, &lo[0], &hi[0]);
    scr_cells_ext(a.scr, 1, by, &lo[1], &hi[1]);
    scr_cells_ext(a.scr, 2, bz, &lo[2], &hi[2]);
    const int ny = hi[1] - lo[1], nrow = ny * (hi[2] - lo[2]);
    for (int r = (int)(threadIdx.x >> 6); r < nrow; r += 4) {
      int i[3];
      i[1] = lo[1] + r % ny;
      i[2] = lo[2] + r / ny;
      for (i[0] = lo[0] + (int)(threadIdx.x & 63); i[0] < hi[0]; i[0] += 64) prepass_hlld_cell(a, i);
    }
  }
}

int launch_prepass(const PrepassArgs &a, hipStream_t s)
{
  const unsigned nb = (unsigned)((a.c1 - a.c0 + 255) / 256);
  if (a.hllflag && a.hsum) {
    // (pion_step.hip passes a summary only for whole-array launches of a 3-D Cartesian grid without debug outputs)
    const long nblk = scr_total(a.scr);
    if (hipMemsetAsync(a.hllflag, 0, (size_t)a.g.ncell, s) != hipSuccess) return -1;
    if (hipMemsetAsync(a.scr_count, 0, sizeof(int), s) != hipSuccess) return -1;
    hipLaunchKernelGGL(k_prepass_screen, dim3((unsigned)((nblk + 255) / 256)), dim3(256), 0, s, a);
    const unsigned ngrid = (nblk < 4096) ? (unsigned)nblk : 4096u;
    hipLaunchKernelGGL(k_prepass_hlld_blocks, dim3(ngrid), dim3(256), 0, s, a);
  }
  else if (a.hllflag) {
    // [c0,c1) is a whole number of planes (pion_step.hip)
    const long plane = (long)a.g.nga[0] * a.g.nga[1];
    const unsigned npl = (unsigned)((a.c1 - a.c0) / plane) + ((a.c3 > a.c2) ? (unsigned)((a.c3 - a.c2) / plane) : 0u);
    const unsigned ntile = (unsigned)((a.g.nga[0] + 63) / 64) * ((a.g.nga[1] + 3) / 4) * npl;
    if (a.g.ndim == 2 && (a.c0 != 0 || a.c1 != a.g.ncell)) {
      // a part of a split 2-D stage (pion_step.hip): whole rows
      const long row = a.g.nga[0];
      const unsigned nr = (unsigned)((a.c1 - a.c0) / row) + ((a.c3 > a.c2) ? (unsigned)((a.c3 - a.c2) / row) : 0u);
      if (nr > 0)
        hipLaunchKernelGGL(k_prepass_hlld_rows, dim3((unsigned)((a.g.nga[0] + 63) / 64) * ((nr + 3) / 4)), dim3(256), 0,
                           s, a);
    }
    else if (a.g.ndim == 3 && a.g.cyl == 0 && !a.divv && !a.gradp && a.c3 <= a.c2 && npl >= PION_PREPASS_ZC
        && a.g.ncell * 8L < (1L << 32)) {
      const unsigned nch = (npl + PION_PREPASS_ZC - 1) / PION_PREPASS_ZC;
      const unsigned nt = (unsigned)((a.g.nga[0] + 61) / 62) * ((a.g.nga[1] + 3) / 4) * nch;   // 62 cells per wavefront along x
      hipLaunchKernelGGL(k_prepass_hlld_march, dim3(((nt + 7) / 8) * 8), dim3(256), 0, s, a);
    }
    else hipLaunchKernelGGL(k_prepass_hlld, dim3(((ntile + 7) / 8) * 8), dim3(256), 0, s, a);
  }
  if (a.eta) hipLaunchKernelGGL((k_prepass_hcorr<8>), dim3(nb), dim3(256), 0, s, a);
  return (int)hipGetLastError();
}

}  // namespace PION_FPNS
}  // namespace pion
