// hll_screen.h -- the rule that lets the HLLD -> HLL switch prepass skip calm regions of a 3-D grid.
//
// The stage kernel (stage_rows2.h) leaves the minimum and the maximum of the pressure it has just written for every
// BLOCK of on-grid cells; before the next stage a screen kernel (kernels_prepass.hip) calls a block QUIET when the range of
// the block and its 3 x 3 x 3 block neighbourhood satisfies  M - m <= 1.6 m, and the dense switch kernel runs on the
// other blocks only.  Shared by the producer, the consumer, the C-ABI layer (pion_step.hip) and the tests' host-side
// probe (tests/native/hll_screen_probe.cpp); it includes nothing, so that the probe compiles it as plain host code.
//
// Why quiet blocks need no evaluation: the dense kernels flag a cell only when, on some axis, its two neighbours
// p+ and p- have  !(|p+ - p-| <= 1.6 p+)  or  !(|p+ - p-| <= 1.6 p-)  ("steep").  Every cell of a block, the ghost
// cells next to a block on a face of the grid included, takes its neighbours from the cells of the neighbourhood:
// an on-grid neighbour is at most one cell outside the block, and a ghost cell of an admitted face type holds an
// exact copy of the pressure of an on-grid cell at most nbc cells from that face (periodic: from the far side,
// which is why the neighbourhood wraps along a periodic axis), which lies in a block of the neighbourhood because
// the first and the last block of an axis are at least nbc cells wide (scr_nblocks: a narrower remainder joins the
// block before it).  Rounding is monotone, so
// fl(|p+ - p-|) <= fl(M - m) <= fl(1.6 m) <= fl(1.6 min(p+, p-)): the very comparison of the dense kernels, no
// safety factor, no addition that a fused multiply-add could change.  m <= 0 fails both alike.  A NaN pressure is
// folded in as M = +inf by the producer (min / max instructions drop a NaN operand), so its block is active.
#ifndef PION_HLL_SCREEN_H
#define PION_HLL_SCREEN_H

#if defined(__HIPCC__) || defined(__CUDACC__)
#define PION_SCR_HD __host__ __device__ inline
#else
#define PION_SCR_HD inline
#endif

// cells per block along x (the stage kernel's x tile, PION_MARCH_XT), y and z.  The stage kernel's rows per wavefront
// must divide PION_SCR_BY (2 and 4 do: the two stages of the 3-D MHD scheme), so that a row group lies in one block.
// Tried on paper before settling: one plane per block costs a wavefront reduction per row group and plane (about
// 50 instructions against some 8 600 cycles per row: several tenths of a ms per step), eight planes a twentieth of it.
#define PION_SCR_BX 62
#define PION_SCR_BY 4
#define PION_SCR_BZ 8

namespace pion {

struct ScrGeom {
  int ng[3];    // on-grid cells
  int nbc[3];   // ghost layers
  int nb[3];    // blocks
  int per[3];   // 1: periodic axis (the neighbourhood wraps), 0: out-of-range neighbours are skipped
};

PION_SCR_HD int scr_bsize(const int d) { return (d == 0) ? PION_SCR_BX : ((d == 1) ? PION_SCR_BY : PION_SCR_BZ); }
// blocks along axis d of n on-grid cells: a remainder of fewer than nbc cells joins the last whole block, so that the
// last block holds the nbc cells that the ghost cells of a periodic axis copy
PION_SCR_HD int scr_nblocks(const int n, const int nbc, const int d)
{
  const int B = scr_bsize(d), r = n % B;
  const int nb = (r == 0 || r >= nbc) ? (n + B - 1) / B : n / B;
  return (nb < 1) ? 1 : nb;
}
// block of on-grid cell i along axis d, of nb blocks
PION_SCR_HD int scr_block_of(const int i, const int nb, const int d)
{
  const int b = i / scr_bsize(d);
  return (b < nb) ? b : nb - 1;
}
// an axis must hold the nbc cells its ghost cells copy
PION_SCR_HD bool scr_axis_ok(const int n, const int nbc) { return n >= nbc && n >= 1; }
PION_SCR_HD ScrGeom scr_geom(const int *ng, const int *nbc, const int *per)
{
  ScrGeom s;
  for (int d = 0; d < 3; d++) {
    s.ng[d] = ng[d];
    s.nbc[d] = nbc[d];
    s.nb[d] = scr_nblocks(ng[d], nbc[d], d);
    s.per[d] = per[d];
  }
  return s;
}
PION_SCR_HD long scr_total(const ScrGeom &s) { return (long)s.nb[0] * s.nb[1] * s.nb[2]; }
PION_SCR_HD long scr_index(const ScrGeom &s, const int bx, const int by, const int bz)
{
  return ((long)bz * s.nb[1] + by) * s.nb[0] + bx;
}
// on-grid cells [lo, hi) of block b along axis d
PION_SCR_HD void scr_cells(const ScrGeom &s, const int d, const int b, int *lo, int *hi)
{
  *lo = b * scr_bsize(d);
  *hi = (b == s.nb[d] - 1) ? s.ng[d] : *lo + scr_bsize(d);
}
// ... and the all-cell index range the dense kernel evaluates for it: a block on a face of the grid also takes the
// ghost cells beyond that face, so that the extended blocks tile the whole array, every cell exactly once
PION_SCR_HD void scr_cells_ext(const ScrGeom &s, const int d, const int b, int *lo, int *hi)
{
  scr_cells(s, d, b, lo, hi);
  *lo += (b == 0) ? 0 : s.nbc[d];
  *hi += (b == s.nb[d] - 1) ? 2 * s.nbc[d] : s.nbc[d];
}
// neighbour o = -1, 0, +1 of block b along axis d: its number, or -1 where there is none
PION_SCR_HD int scr_neighbour(const ScrGeom &s, const int d, const int b, const int o)
{
  int n = b + o;
  if (n < 0) n = s.per[d] ? s.nb[d] - 1 : -1;
  else if (n >= s.nb[d]) n = s.per[d] ? 0 : -1;
  return n;
}
// the rule: evaluated in fp64, exactly these operations
PION_SCR_HD bool scr_quiet(const double m, const double M) { return M - m <= 1.6 * m; }

// The summaries are kept as unsigned 64-bit keys so that wavefronts of different row groups can fold their values
// into one block with atomicMax: key() is increasing in the double (negative values and zeros included), the maximum is
// stored as key(M), the minimum as ~key(m); a cleared entry (0) decodes to NaN, i.e. to an active block.
PION_SCR_HD unsigned long long scr_key(const double x)
{
  unsigned long long b;
  __builtin_memcpy(&b, &x, 8);
  return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
}
PION_SCR_HD double scr_unkey(const unsigned long long k)
{
  const unsigned long long b = (k >> 63) ? (k & 0x7fffffffffffffffull) : ~k;
  double x;
  __builtin_memcpy(&x, &b, 8);
  return x;
}
// min and max over the neighbourhood of block (bx, by, bz) from the two key arrays, and the verdict
PION_SCR_HD bool scr_block_quiet(const ScrGeom &s, const unsigned long long *kmax, const unsigned long long *knmin,
                                 const int bx, const int by, const int bz)
{
  unsigned long long kM = 0, kN = 0;
  bool hole = false;
  for (int oz = -1; oz <= 1; oz++) {
    const int z = scr_neighbour(s, 2, bz, oz);
    if (z < 0) continue;
    for (int oy = -1; oy <= 1; oy++) {
      const int y = scr_neighbour(s, 1, by, oy);
      if (y < 0) continue;
      for (int ox = -1; ox <= 1; ox++) {
        const int x = scr_neighbour(s, 0, bx, ox);
        if (x < 0) continue;
        const long i = scr_index(s, x, y, z);
        const unsigned long long a = kmax[i], b = knmin[i];
        if (a == 0 || b == 0) hole = true;   // a block nothing was written to: no statement about it
        kM = (a > kM) ? a : kM;
        kN = (b > kN) ? b : kN;
      }
    }
  }
  if (hole) return false;
  return scr_quiet(scr_unkey(~kN), scr_unkey(kM));
}

}  // namespace pion
#endif
