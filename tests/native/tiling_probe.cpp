// TEST INFRASTRUCTURE: host-side probe of the stage kernel's launch geometry (pion_amd/csrc/rows_tiling.h).
//
// Runs the workgroup / wavefront / lane decode of k_stage_rows2 (rows2_decode) for every workgroup of a launch grid, and every row
// and plane each lane visits, exactly as the kernel's loops do, and counts which on-grid cells (and, for periodic x,
// which x ghost images) the lanes that write would write.  Also reports the extremes of every cell index the lanes
// form (priming plane k0 - 1 and clamped rows included) and exports the host's launch plan rules.  Used through
// ctypes by tests/test_rows_tiling.py and tests/test_gpu_launch_geometry.py.
#include <hip/hip_runtime.h>

#include "../../pion_amd/csrc/rows_tiling.h"

namespace {
// the members of StageArgs that the geometry reads
struct ProbeGrid {
  int ng[3], nbc[3];
};
struct ProbeArgs {
  ProbeGrid g;
  int rows, kz0, kz1, kz2, kz3, zchunk, nzb, zcmax;
};
}  // namespace
using namespace pion;

enum {
  ST_NBLOCKS, ST_WAVES, ST_CMIN, ST_CMAX, ST_IXMIN, ST_IXMAX, ST_YMIN, ST_YMAX, ST_KMIN, ST_KMAX, ST_NCELL,
  ST_BADWRITE, ST_BADLANE, ST_NSTAT = 16
};

extern "C" {

// One launch of k_stage_rows2 on an nx x ny x nz grid (nz = 1 and ndim = 2: the 2-D instance, no priming plane)
// with nbc ghost layers.  count: nx * ny * nz bytes (x fastest, zeroed by the caller), writes per cell; ghost (may be
// null): 2 * nbc * ny * nz bytes, x ghost images written when xwrap ([side][k][y][g]: side 0 the lower x ghosts, g
// their all-cell x index; side 1 the upper ones, g = all-cell x - nx - nbc).
// stats: ST_NSTAT longs.  Returns 0, or -1 for arguments the kernel would not be launched with.
int tp_probe(int ndim, int nx, int ny, int nz, int nbc, int rows, int kz0, int kz1, int kz2, int kz3, int zchunk,
             int nzb, int zcmax, int xwrap, unsigned char *count, unsigned char *ghost, long *stats)
{
  if (nx < 1 || ny < 1 || nz < 1 || rows < 1 || zchunk < 1 || nbc < 1) return -1;
  ProbeArgs a;
  a.g.ng[0] = nx;
  a.g.ng[1] = ny;
  a.g.ng[2] = nz;
  for (int d = 0; d < 3; d++) a.g.nbc[d] = (d < ndim) ? nbc : 0;
  a.rows = rows;
  a.kz0 = kz0;
  a.kz1 = kz1;
  a.kz2 = kz2;
  a.kz3 = (kz3 > kz2) ? kz3 : kz2;
  a.zchunk = zchunk;
  a.nzb = nzb;
  a.zcmax = zcmax;
  const bool noz = (ndim == 2);
  const long sx = nx + 2 * a.g.nbc[0], sy = sx * (ny + 2 * a.g.nbc[1]);
  const long ncell = sy * (nz + 2 * a.g.nbc[2]);
  for (int i = 0; i < ST_NSTAT; i++) stats[i] = 0;
  long cmin = ncell, cmax = -1, ixmin = 1L << 40, ixmax = -(1L << 40), ymin = ixmin, ymax = ixmax, kmin = ixmin,
       kmax = ixmax, badw = 0, badl = 0, waves = 0;
  const long nblocks = rows2_nblocks(a);
  stats[ST_NBLOCKS] = nblocks;
  for (long b = 0; b < nblocks; b++)
    for (int w = 0; w < 4; w++) {
      bool ran = false;
      for (int lane = 0; lane < 64; lane++) {
        const Rows2Lane d = rows2_decode(a, (unsigned)b, w, lane);
        if (d.leave) {
          if (lane > 0 && ran) badl++;   // the whole wavefront must leave together
          break;
        }
        ran = true;
        // the kernel's loops (stage_rows2.h): planes k0-1 (priming, 3-D) .. k1-1, rows 0 .. nrows-1 (clamped to
        // the lane's own last row past nrows_l)
        const long crow0 = (long)(d.ix + a.g.nbc[0]) + sx * (d.j0 + a.g.nbc[1]) + sy * (d.k0 - 1 + a.g.nbc[2]);
        for (int k = noz ? d.k0 : d.k0 - 1; k < d.k1; k++) {
          const bool prime = !noz && (k == d.k0 - 1);
          for (int r = 0; r < d.nrows; r++) {
            const bool row_ok = (r < d.nrows_l);
            const int rr = row_ok ? r : d.nrows_l - 1;
            const long c = crow0 + sx * rr + sy * (k - (d.k0 - 1));
            const long y = d.j0 + rr;
            cmin = c < cmin ? c : cmin;
            cmax = c > cmax ? c : cmax;
            ixmin = d.ix < ixmin ? d.ix : ixmin;
            ixmax = d.ix > ixmax ? d.ix : ixmax;
            ymin = y < ymin ? y : ymin;
            ymax = y > ymax ? y : ymax;
            kmin = k < kmin ? k : kmin;
            kmax = k > kmax ? k : kmax;
            if (prime || !d.writer || !row_ok) continue;
            if (d.ix < 0 || d.ix >= nx || y < 0 || y >= ny || k < 0 || k >= nz) {
              badw++;
              continue;
            }
            count[d.ix + (long)nx * (y + (long)ny * k)]++;
            if (xwrap && ghost) {
              // the periodic images (stage_rows2.h, a.xwrap): ix < nbc -> the upper ghost ix + nx, ix >= nx - nbc
              // -> the lower ghost ix - nx
              const int nb0 = a.g.nbc[0];
              if (d.ix < nb0) ghost[((1L * nz + k) * ny + y) * nb0 + d.ix]++;
              else if (d.ix >= nx - nb0) ghost[((0L * nz + k) * ny + y) * nb0 + (d.ix - (nx - nb0))]++;
            }
          }
        }
      }
      if (ran) waves++;
    }
  stats[ST_WAVES] = waves;
  stats[ST_CMIN] = cmin;
  stats[ST_CMAX] = cmax;
  stats[ST_IXMIN] = ixmin;
  stats[ST_IXMAX] = ixmax;
  stats[ST_YMIN] = ymin;
  stats[ST_YMAX] = ymax;
  stats[ST_KMIN] = kmin;
  stats[ST_KMAX] = kmax;
  stats[ST_NCELL] = ncell;
  stats[ST_BADWRITE] = badw;
  stats[ST_BADLANE] = badl;
  return 0;
}

// the x/y tiling of one plane chunk: ntx_full, rem, spw, nyg, nfull, nrem, per_chunk
void tp_tiling(int nx, int ny, int rows, int *out)
{
  const RowsTiling t = rows_tiling_of(nx, ny, rows);
  const int v[7] = {t.ntx_full, t.rem, t.spw, t.nyg, t.nfull, t.nrem, t.per_chunk};
  for (int i = 0; i < 7; i++) out[i] = v[i];
}

// the decode of one lane: ix, jg, jg_first, j0, nrows, nrows_l, k0, k1, writer, leave
void tp_decode(int nx, int ny, int nz, int rows, int kz0, int kz1, int kz2, int kz3, int zchunk, int nzb, int zcmax,
               unsigned block, int wave, int lane, int *out)
{
  ProbeArgs a;
  a.g.ng[0] = nx;
  a.g.ng[1] = ny;
  a.g.ng[2] = nz;
  a.rows = rows;
  a.kz0 = kz0;
  a.kz1 = kz1;
  a.kz2 = kz2;
  a.kz3 = (kz3 > kz2) ? kz3 : kz2;
  a.zchunk = zchunk;
  a.nzb = nzb;
  a.zcmax = zcmax;
  const Rows2Lane d = rows2_decode(a, block, wave, lane);
  const int v[10] = {d.ix, d.jg, d.jg_first, d.j0, d.nrows, d.nrows_l, d.k0, d.k1, d.writer, d.leave};
  for (int i = 0; i < 10; i++) out[i] = v[i];
}

// zchunk_bounds for chunks cz = 0 .. ncz-1 of a strip of np planes; returns the number of chunks it reports
int tp_zchunk_table(int np, int cmax, int ncz, int *k0, int *k1)
{
  int n = 0;
  for (int cz = 0; cz < ncz; cz++) n = zchunk_bounds(np, cmax, cz, &k0[cz], &k1[cz]);
  return n;
}

// xcd_tile of workgroups b = 0 .. nb-1 for ntiles tiles
void tp_xcd_table(long nb, long ntiles, long *out)
{
  for (long b = 0; b < nb; b++) out[b] = xcd_tile(b, ntiles);
}

int tp_rmax_lds(int nv, int zsl) { return rows2_rmax_lds(nv, zsl != 0); }

int tp_pick_rows_2d(int nx, int ny, int rows, int wg_per_cu, int ncu)
{
  return rows2_pick_rows_2d_rule(nx, ny, rows, wg_per_cu, ncu);
}

// the launch plan of one stage part: out = rows, rows_auto, zchunk, zcmax, nzb
void tp_plan(int ndim, int nx, int ny, int np, int ncu, int nv, int euler, int march, int zslope_lds, int second_order,
             int uneven, int want_rows, int want_rows1, int want_zchunk, int *out)
{
  Rows2PlanIn p;
  p.ndim = ndim;
  p.nx = nx;
  p.ny = ny;
  p.np = np;
  p.ncu = ncu;
  p.nv = nv;
  p.euler = euler != 0;
  p.march = march != 0;
  p.zslope_lds = zslope_lds != 0;
  p.second_order = second_order != 0;
  p.uneven = uneven != 0;
  p.want_rows = want_rows;
  p.want_rows1 = want_rows1;
  p.want_zchunk = want_zchunk;
  const Rows2Plan o = rows2_plan(p);
  out[0] = o.rows;
  out[1] = o.rows_auto;
  out[2] = o.zchunk;
  out[3] = o.zcmax;
  out[4] = o.nzb;
}

}  // extern "C"
