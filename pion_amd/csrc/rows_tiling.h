// rows_tiling.h -- geometry of the 3-D / 2-D stage kernel k_stage_rows2 (stage_rows2.h): which cells, rows and planes
// a workgroup, wavefront and lane take, the grid that covers them, and the host's launch plan (rows per wavefront,
// plane chunks).  Shared by the kernel, its launcher (stage_rows2.h), the C-ABI layer (pion_step.hip) and the tests'
// host-side coverage probe (tests/native/tiling_probe.cpp); it includes nothing, so that the probe compiles it as
// plain host code.  The per-launch functions are templates over the argument struct: they read a.g.ng[0..1],
// a.rows, a.kz0..a.kz3, a.zchunk, a.nzb and a.zcmax, nothing else.
//
// x: full tiles of PION_MARCH_XT = 62 cells, one wavefront each (lanes 0 and 63 are halo lanes that only
// supply their neighbour's interface data).  The remaining `rem` cells of a row (16 of 512) would leave most
// of a wavefront idle, so a "remainder" wavefront packs the remainders of `spw` consecutive row groups side by
// side, each in a segment of rem + 2 lanes with its own two halo lanes (the x shuffles only ever cross a segment
// boundary into a halo lane).  y: groups of a.rows consecutive rows per wavefront.
//
// 2-D row ranges.  A 2-D launch has one "plane" and no z part; it updates a RANGE of on-grid rows [ky0, ky1) and, for
// the two boundary strips of a slab cut along y, a second range [ky2, ky3) of the same length.  The launcher
// (stage_ranges, pion_step.hip) encodes a range in the members the geometry already reads, so nothing here changes:
//   a.g.ng[1] = ky1 - ky0            the rows that are tiled: rows_tiling, rows2_nblocks and rows2_pick_rows_2d_rule
//                                    are sized from the range, row groups start at its first row;
//   a.kz0 = ky0, a.kz1 = ky0 + 1     one chunk (zchunk >= 1, nzb = 0) whose "plane" number k0 is the range's first row;
//   a.kz2 = ky2, a.kz3 = ky2 + 1     the second range as a second chunk (empty when kz3 <= kz2).
// A whole stage is the range [0, ny): ng[1] = ny, kz0 = 0, kz1 = 1, which is what 2-D launches always passed.
// rows2_decode returns j0 = jg * R RELATIVE to the range and k0 = the range's first row; the kernels (k_stage_rows2,
// k_cooling_dE) add k0 to the row and use plane 0 when a.g.ndim == 2 -- that one step is theirs alone (the argument
// structs of the host-side probe carry no ndim), so the probe pins the tiling of a range, not its placement.
#ifndef PION_ROWS_TILING_H
#define PION_ROWS_TILING_H

#define PION_MARCH_XT 62  // output cells per wavefront along x
// LDS a workgroup of k_stage_rows2 may use so that two fit a CU (160 KiB)
#define PION_ROWS2_LDS_BYTES (80 * 1024)
#ifndef PION_ROWS2_YWG
#define PION_ROWS2_YWG 1
#endif

namespace pion {

// Uneven plane chunks of a strip of np planes: chunk number cz covers [*k0, *k1) (relative to the strip); returns the
// number of chunks.  A rule instead of a table in the kernel arguments: indexing an argument array with a run-time
// index makes the compiler copy the whole argument struct to scratch memory (measured: the stage kernel 2x slower).
__host__ __device__ inline int zchunk_bounds(const int np, const int cmax, const int cz, int *k0, int *k1)
{
  int n = 0, pos = 0;
  *k0 = *k1 = np;
  while (pos < np) {
    const int rem = np - pos;
    const int cmin = (np <= 128) ? 2 : 4;   // (a slab of a few dozen planes: its tail is a larger share of the launch)
    int c = (rem > 2 * cmax) ? cmax : ((rem / 2 > cmin) ? rem / 2 : cmin);
    if (c > cmax) c = cmax;
    if (c > rem || rem - c < cmin) c = rem;
    if (n == cz) {
      *k0 = pos;
      *k1 = pos + c;
    }
    pos += c;
    n++;
  }
  return n;
}

// XCD-aware tile decode of the cell kernels (kernels_fp.hip, kernels_prepass.hip): workgroups are dealt round-robin to the 8 XCDs (b % 8
// share an XCD); give each XCD a contiguous range of tiles so that the halo re-reads of neighbouring tiles hit the
// same L2.  Placement only changes speed, never results.  (The caller launches 8 * ceil(ntiles / 8) workgroups and
// skips the tiles >= ntiles.)
__host__ __device__ __forceinline__ long xcd_tile(const long b, const long ntiles)
{
  const long chunk = (ntiles + 7) / 8;
  return (b % 8) * chunk + (b / 8);
}

// x/y tiling of one plane chunk, shared by the kernel and its launcher
struct RowsTiling {
  int ntx_full, rem, spw, nyg, nfull, nrem, per_chunk;
};
template <class A>
__host__ __device__ inline RowsTiling rows_tiling(const A &a)
{
  RowsTiling t;
  t.nyg = (a.g.ng[1] + a.rows - 1) / a.rows;
  t.ntx_full = a.g.ng[0] / PION_MARCH_XT;
  t.rem = a.g.ng[0] - t.ntx_full * PION_MARCH_XT;
  t.spw = (t.rem > 0) ? 64 / (t.rem + 2) : 0;   // row groups per remainder wavefront
  t.nfull = t.ntx_full * t.nyg;
  t.nrem = (t.rem > 0) ? (t.nyg + t.spw - 1) / t.spw : 0;
  t.per_chunk = t.nfull + t.nrem;
  return t;
}
inline RowsTiling rows_tiling_of(const int nx, const int ny, const int rows)
{
  struct {
    struct {
      int ng[2];
    } g;
    int rows;
  } a = {{{nx, ny}}, rows};
  return rows_tiling(a);
}

// plane chunks of one launch: nzc1 of the first strip [kz0, kz1) (uneven when nzb > 0), nzc of both strips
template <class A>
__host__ __device__ inline int rows2_nzc1(const A &a)
{
  return (a.nzb > 0) ? a.nzb : (a.kz1 - a.kz0 + a.zchunk - 1) / a.zchunk;
}
template <class A>
__host__ __device__ inline int rows2_nzc(const A &a)
{
  return rows2_nzc1(a) + (a.kz3 - a.kz2 + a.zchunk - 1) / a.zchunk;
}

// the launch grid: workgroups of four wavefronts, an eighth of each chunk's workgroups per XCD, through all chunks
template <class A>
__host__ __device__ inline long rows2_nblocks(const A &a)
{
  const int nb4 = (rows_tiling(a).per_chunk + 3) / 4, nb8 = (nb4 + 7) / 8;
  return 8L * nb8 * rows2_nzc(a);
}

// What one lane of k_stage_rows2 works on: the kernel's own decode (stage_rows2.h, kept inline there with the same
// expressions -- the kernel compiled from this function is not instruction for instruction the same), here for the
// tests' coverage probe.  leave: the whole wavefront has nothing to do (the other fields are then unset).  Else the
// lane's column ix (on-grid x index, -1 .. nx: halo lanes included), its row group jg (clamped into the grid for idle
// lanes), the wavefront's first row group jg_first, the lane's first row j0 = jg * R, the rows the wavefront marches
// (nrows, from jg_first) and the lane's own rows (nrows_l, from jg: fewer in a partial last group, whose missing rows
// the lane redoes as its last row without writing them), the planes [k0, k1) it updates (plane k0 - 1 primes the z
// carry), and whether it writes its cells.
struct Rows2Lane {
  int ix, jg, jg_first, j0, nrows, nrows_l, k0, k1;
  bool writer, leave;
};
template <class A>
__host__ __device__ inline Rows2Lane rows2_decode(const A &a, const unsigned block, const int wave, const int lane)
{
  Rows2Lane d;
  const RowsTiling tl = rows_tiling(a);
  const int R = a.rows;
  const int nyg = tl.nyg;
  const int nzc1 = rows2_nzc1(a);
  const int nzc = rows2_nzc(a);   // chunks of both strips
  // Workgroup -> (x-y tile group, plane chunk): an eighth of the x-y tiles per XCD (block % 8), through all chunks
  const int nb4 = (tl.per_chunk + 3) / 4, nb8 = (nb4 + 7) / 8;   // workgroups per chunk; per chunk and XCD
  const int lb = (int)(block >> 3);
  const int cz = lb / nb8, bq = (int)(block & 7) * nb8 + lb % nb8;
  const int tt = bq * 4 + wave;
  d.leave = (cz >= nzc || bq >= nb4 || tt >= tl.per_chunk);
  if (d.leave) return d;
  if (tt < tl.nfull) {
#if PION_ROWS2_YWG
    // the four wavefronts of a workgroup take four y-adjacent row groups of the same x tile
    const int per4 = 4 * tl.ntx_full, g4 = tt / per4, r4 = tt - g4 * per4;
    const int m = (nyg - 4 * g4 < 4) ? nyg - 4 * g4 : 4;
    const int tx = r4 / m;
    d.jg = d.jg_first = 4 * g4 + r4 % m;
#else
    const int tx = tt % tl.ntx_full;
    d.jg = d.jg_first = tt / tl.ntx_full;
#endif
    d.ix = tx * PION_MARCH_XT - 1 + lane;
    d.writer = (lane >= 1 && lane <= PION_MARCH_XT && d.ix < a.g.ng[0]);
  }
  else {
    const int seg = lane / (tl.rem + 2), pos = lane % (tl.rem + 2);
    d.jg_first = (tt - tl.nfull) * tl.spw;
    d.jg = d.jg_first + seg;
    d.ix = tl.ntx_full * PION_MARCH_XT - 1 + pos;
    d.writer = (seg < tl.spw && d.jg < nyg && pos >= 1 && pos <= tl.rem);
    if (d.jg >= nyg) d.jg = nyg - 1;   // idle lanes redo the last group, in bounds, and write nothing
  }
  if (d.ix > a.g.ng[0]) d.ix = a.g.ng[0];
  d.j0 = d.jg * R;
  d.nrows = (d.jg_first * R + R <= a.g.ng[1]) ? R : a.g.ng[1] - d.jg_first * R;
  d.nrows_l = (d.j0 + R <= a.g.ng[1]) ? R : a.g.ng[1] - d.j0;
  if (a.nzb > 0 && cz < nzc1) {
    zchunk_bounds(a.kz1 - a.kz0, a.zcmax, cz, &d.k0, &d.k1);
    d.k0 += a.kz0;
    d.k1 += a.kz0;
  }
  else {
    d.k0 = (cz < nzc1) ? a.kz0 + cz * a.zchunk : a.kz2 + (cz - nzc1) * a.zchunk;
    const int kend = (cz < nzc1) ? a.kz1 : a.kz3;
    d.k1 = (d.k0 + a.zchunk < kend) ? d.k0 + a.zchunk : kend;
  }
  return d;
}

// ---- host-side launch plan ----

// rows per wavefront the LDS budget allows an instance with nv variables (zsl: the z slope is carried in LDS too)
inline int rows2_rmax_lds(const int nv, const bool zsl)
{
  const int nz = zsl ? 2 * nv : nv;
  const int r = (int)(PION_ROWS2_LDS_BYTES / (sizeof(double) * 4 * nz * 64));
  return r > 8 ? 8 : r;
}

// 3-D: rows per wavefront k_stage_rows2 will use (want <= 0: automatic; PION_ROWS / PION_ROWS1 otherwise)
inline int rows2_rows_3d(const int nv, const bool euler, const bool zslope_lds, const int want)
{
  const int nz = zslope_lds ? 2 * nv : nv;
  int r = rows2_rmax_lds(nv, zslope_lds);
  if (want <= 0) {
    // automatic.  The MHD instances need the whole register file of two wavefronts per SIMD: as many rows as two
    // workgroups' LDS allows (fewer Riemann solves per cell).  The Euler instances take ~160 registers, so a
    // THIRD wavefront per SIMD fits if three workgroups' LDS does: rows for 160 KiB / 3 (measured at 512^3,
    // second-order stage with 2 rows instead of 4: Roe-CV 13.8 -> 12.8 ms/step, FVS + tracer + cooling 25.9 -> 23.6)
    if (euler) {
      int r3 = (int)((160 * 1024 / 3) / (sizeof(double) * 4 * nz * 64));
      if (r3 < 1) r3 = 1;
      if (r3 < r) r = r3;
    }
  }
  else if (want < r) r = want;
  return r < 1 ? 1 : r;
}

// 2-D: rows per wavefront marched along y (nothing in LDS): 2 + 1/R solves per cell against the number of
// wavefronts (measured, 4096 x 1260 Euler Roe-CV / 4096 x 6144 GLM-MHD HLLD, Mcell-updates/s: R = 4 7694 / 5940,
// 8 11360 / 7711, 16 12686 / 8034, 32 13076 / 7371; the cell-per-thread kernel 4680 / 2176); fewer rows on
// small grids so that every slot still gets a wavefront
inline int rows2_rows_2d(const int nx, const int ny, const int ncu)
{
  int r2 = 16;
  const long ntx = (nx + 61) / 62;
  while (r2 > 2 && ntx * ((ny + r2 - 1) / r2) < 8L * (ncu > 0 ? ncu : 256)) r2 /= 2;
  return r2;
}

// 2-D launches: rows per wavefront for the instance launched.  A 2-D launch is one to a few "rounds" of wavefronts
// (one wavefront marches its R rows from start to end), so what matters is how well the wavefronts fill the slots of
// the rounds they need: R is the value in [8, 64] with the best (filled share of the slots) / (2 + 1/R Riemann solves
// per cell) -- for launches of at most three rounds at the caller's R; the slots follow from the occupancy of the
// instance (wg_per_cu workgroups per CU).  Measured, Euler Roe-CV 4096 x 1260 (66 x-tiles, 3 wavefronts per SIMD):
// R = 16 (1.7 rounds) 12 790, 28 (0.97 of one round) 14 240-14 300, 32 13 150 Mcell-updates/s.  The result does not
// depend on R (tests/test_gpu_xtile.py).
inline int rows2_pick_rows_2d_rule(const int nx, const int ny, const int rows, const int wg_per_cu, const int ncu)
{
  const long slots = 4L * wg_per_cu * (ncu > 0 ? ncu : 256);
  int best = rows;
  double best_score = -1.0;
  // (a launch of many rounds is filled well enough at the caller's rows, and long columns cost it L2 locality:
  // 4096 x 6144 GLM-MHD HLLD, 12.4 rounds at R = 16: 8340 Mcell-updates/s, R = 50 -- one round fewer -- 7350)
  if ((rows_tiling_of(nx, ny, rows).per_chunk + slots - 1) / slots > 3) return rows;
  for (int R = 8; R <= 64; R++) {
    const long waves = rows_tiling_of(nx, ny, R).per_chunk;
    const long rounds = (waves + slots - 1) / slots;
    const double score = ((double)waves / (double)(rounds * slots)) / (2.0 + 1.0 / R);
    if (score > best_score * 1.0000001) {
      best_score = score;
      best = R;
    }
  }
  return best;
}

// Planes per wavefront (equal chunks) of a strip of np planes.  Every wavefront takes (zchunk + 1 priming plane)
// plane visits and a CU holds 8 wavefronts at a time; pick the chunk that minimises the launch cost model below.
inline int rows2_zchunk_model(const int nx, const int ny, int rows, const int np, const int ncu)
{
  if (rows < 1) rows = 1;
  const RowsTiling t = rows_tiling_of(nx, ny, rows);
  const long per_chunk = (long)t.ntx_full * t.nyg + ((t.rem > 0) ? (t.nyg + t.spw - 1) / t.spw : 0);
  const long slots = 8L * (ncu > 0 ? ncu : 256);   // two workgroups of four wavefronts per CU
  // cost in plane visits: wavefronts are dispatched as slots free up, so a launch takes about
  // (all wave-visits) / slots plus a tail of half a wavefront's length; short chunks balance better, long
  // chunks prime less (measured at 512^3: 16 and 32 planes 27.3 ms/step, 47: 28.4, 64: 28.0, 128: 31.7)
  double best_cost = -1.0;
  int zchunk = 8;
  for (int zc = 8; zc <= 128; zc++) {
    const long nzc = (np + zc - 1) / zc;
    const int longest = (zc < np ? zc : np) + 1;
    const int last = np - (int)(nzc - 1) * zc;           // planes of the last chunk
    if (nzc > 1 && 4 * last < 3 * zc) continue;          // a short last chunk unbalances the tail (22, 26: measured)
    double cost = (double)per_chunk * (double)(np + nzc) / (double)slots + 0.5 * longest;
    if (np % zc != 0) cost *= 1.005;                     // equal chunks first (512^3: 32 planes 25.5, 27 planes 25.8 ms/step)
    if (best_cost < 0 || cost < best_cost) {
      best_cost = cost;
      zchunk = zc;
    }
  }
  return zchunk;
}

// longest uneven chunk: at least ~4 wavefronts per slot over the launch (Euler instances run three workgroups per
// CU, the MHD ones two), between 8 and 32 planes (256^3 Euler: 11 planes; even chunks of the model 3.05 ms/step,
// uneven ones from 32 down 3.28)
inline int rows2_zcmax_model(const int nx, const int ny, int rows, const int np, const bool euler, const int ncu)
{
  if (rows < 1) rows = 1;
  const RowsTiling t = rows_tiling_of(nx, ny, rows);
  const long per_chunk = (long)t.ntx_full * t.nyg + ((t.rem > 0) ? (t.nyg + t.spw - 1) / t.spw : 0);
  const long slots = (euler ? 12L : 8L) * (ncu > 0 ? ncu : 256);
  const long c = (long)np * per_chunk / (4 * slots);
  return (int)(c < 8 ? 8 : (c > 32 ? 32 : c));
}

// uneven chunks of a strip of np planes (the number of chunks, 0 = equal chunks of a.zchunk planes): only strips of
// 16 planes or more are split unevenly
inline int rows2_nzb(const int np, const int zcmax, const bool uneven)
{
  int k0, k1;
  return (uneven && np >= 16) ? zchunk_bounds(np, zcmax, 0, &k0, &k1) : 0;
}

// The launch plan of one stage (stage_tiling, pion_step.hip): rows per wavefront, whether the 2-D launcher
// may refine them (rows2_pick_rows_2d_rule with the instance's occupancy), planes per equal chunk, the uneven chunks'
// longest length and their number.  march: k_stage_rows2 runs (else only zchunk is set, for the cell kernel).
struct Rows2PlanIn {
  int ndim, nx, ny;
  int np;               // planes of the first strip [kz0, kz1)
  int ncu;              // compute units (0: assume 256)
  int nv;               // variables of the instance
  bool euler, march, zslope_lds, second_order, uneven;
  int want_rows, want_rows1, want_zchunk;   // PION_ROWS, PION_ROWS1, PION_ZCHUNK (0: automatic)
};
struct Rows2Plan {
  int rows, rows_auto, zchunk, zcmax, nzb;
};
inline Rows2Plan rows2_plan(const Rows2PlanIn &p)
{
  Rows2Plan o;
  o.rows = p.want_rows;
  o.rows_auto = 0;
  if (p.march && p.ndim == 2) {
    // (PION_ROWS overrides; without it the launcher refines the choice for the instance it launches: its occupancy
    // decides how many wavefronts a "round" holds)
    o.rows = (p.want_rows > 0) ? p.want_rows : rows2_rows_2d(p.nx, p.ny, p.ncu);
    if (o.rows > 64) o.rows = 64;
    o.rows_auto = (p.want_rows > 0) ? 0 : 1;
  }
  else if (p.march)
    o.rows = rows2_rows_3d(p.nv, p.euler, p.zslope_lds && p.second_order, p.second_order ? p.want_rows : p.want_rows1);
  o.zchunk = (p.want_zchunk > 0) ? p.want_zchunk : rows2_zchunk_model(p.nx, p.ny, o.rows, p.np, p.ncu);
  // Uneven chunks (default; PION_UNEVEN_CHUNKS=0: equal chunks of zchunk planes): chunks of the model's length
  // while more than two of them remain, then halving down to 4 planes.  Wavefronts are dispatched in chunk order, so
  // the last ones to start are the shortest and the launch ends with (nearly) all slots busy; a priming plane costs
  // about a third of a plane visit (its z task only).  512 planes: 14 x 32, 32, 16, 8, 4, 4; a 64-plane slab:
  // 32, 16, 8, 4, 4 (equal chunks: 3.25 ms/step for 512 x 512 x 64, 88 % of the per-cell rate of 512^3).
  o.zcmax = 32;
  if (p.want_zchunk > 0) o.zcmax = p.want_zchunk;
  else if (p.march) o.zcmax = rows2_zcmax_model(p.nx, p.ny, o.rows, p.np, p.euler, p.ncu);
  o.nzb = p.march ? rows2_nzb(p.np, o.zcmax, p.uneven) : 0;
  return o;
}

// ---- plane windows ----
//
// k_stage_rows2 addresses a cell as "uniform base + one 32-bit byte offset per lane" (dev_addr.h): one launch reaches
// fewer than PION_ROWS_WINDOW_CELLS = 2^29 cells of a per-cell array from the array's base.  A larger grid is run in
// WINDOWS of planes of the slab axis (z planes in 3-D, rows in 2-D): the host (stage_launch, pion_step.hip) launches
// the kernel once per window, with every per-cell pointer advanced to the window's first plane in 64-bit host
// arithmetic and the window's planes numbered from 0 -- the kernel reads no absolute plane number.
//
// A launch that updates n planes touches n + 2 nbc planes of the all-cell array (its stencil, the priming plane
// included), counted from the all-cell plane the pointers were advanced to.  With s cells per plane and a limit of L
// cells, W = floor((L - 1) / s) - 2 nbc planes fit in one window: (W + 2 nbc) s <= L - 1 < L.  W < 1 -- one plane with
// its ghost planes already exceeds the limit -- is not admitted: such a grid stays on the cell-per-thread kernel.
// A range [lo, hi) of on-grid planes becomes ceil((hi - lo) / W) windows -- no plan has fewer --, in order, sizes
// balanced within one plane, the longer ones first.  A range that fits is ONE window, the range itself.
#define PION_ROWS_WINDOW_CELLS (1L << 29)

inline long rows_window_planes(const long s, const int nbc, const long L) { return (s > 0) ? (L - 1) / s - 2L * nbc : 0; }
// number of windows of [lo, hi) (0: not admitted, or an empty range)
inline int rows_windows_count(const int lo, const int hi, const long s, const int nbc, const long L)
{
  const long W = rows_window_planes(s, nbc, L);
  if (W < 1 || hi <= lo) return 0;
  return (int)(((long)(hi - lo) + W - 1) / W);
}
// window number i of the nw windows of [lo, hi): [*w_lo, *w_hi)
inline void rows_window(const int lo, const int hi, const int nw, const int i, int *w_lo, int *w_hi)
{
  const int n = hi - lo, base = n / nw, extra = n % nw;   // the first `extra` windows take one plane more
  *w_lo = lo + i * base + (i < extra ? i : extra);
  *w_hi = *w_lo + base + (i < extra ? 1 : 0);
}

}  // namespace pion

#endif
