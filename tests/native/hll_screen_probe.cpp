// TEST INFRASTRUCTURE: host-side probe of the screened HLLD -> HLL switch prepass's rule (pion_amd/csrc/hll_screen.h).
//
// Builds the per-block pressure summaries the way the stage kernel does (min / max over the on-grid cells of a block,
// a NaN folded in as a maximum of +inf, stored as keys), applies the rule to every block and reports the blocks' extended
// cell ranges.  Plain host C++: tests/test_hll_screen_rule.py compiles this file with the host compiler and drives it
// through ctypes.
#include "../../pion_amd/csrc/hll_screen.h"

using namespace pion;

extern "C" {

// number of blocks per axis for a grid of ng[3] cells with nbc ghost layers; returns 0 when an axis cannot be screened
int hs_geom(const int *ng, int nbc, const int *per, int *nb)
{
  const int nb3[3] = {nbc, nbc, nbc};
  for (int d = 0; d < 3; d++)
    if (!scr_axis_ok(ng[d], nbc)) return 0;
  const ScrGeom s = scr_geom(ng, nb3, per);
  for (int d = 0; d < 3; d++) nb[d] = s.nb[d];
  return 1;
}

// all-cell index ranges [lo, hi) of the cells the dense kernel evaluates for block (b[0], b[1], b[2])
void hs_ext(const int *ng, int nbc, const int *per, const int *b, int *lo, int *hi)
{
  const int nb3[3] = {nbc, nbc, nbc};
  const ScrGeom s = scr_geom(ng, nb3, per);
  for (int d = 0; d < 3; d++) scr_cells_ext(s, d, b[d], &lo[d], &hi[d]);
}

// p: the pressure of every cell, ghosts included (x fastest).  quiet: one byte per block (x fastest), 1 = quiet.
void hs_screen(const int *ng, int nbc, const int *per, const double *p, unsigned char *quiet)
{
  const int nb3[3] = {nbc, nbc, nbc};
  const ScrGeom s = scr_geom(ng, nb3, per);
  const long n = scr_total(s);
  unsigned long long *kmax = new unsigned long long[2 * n];
  unsigned long long *knmin = kmax + n;
  for (long i = 0; i < 2 * n; i++) kmax[i] = 0;
  const long sy = ng[0] + 2 * nbc, sz = sy * (ng[1] + 2 * nbc);
  for (int k = 0; k < ng[2]; k++)
    for (int j = 0; j < ng[1]; j++)
      for (int i = 0; i < ng[0]; i++) {
        const double v = p[(i + nbc) + sy * (j + nbc) + sz * (k + nbc)];
        const long b = scr_index(s, scr_block_of(i, s.nb[0], 0), scr_block_of(j, s.nb[1], 1), scr_block_of(k, s.nb[2], 2));
        // the stage kernel's fold: running values start at +inf / -inf, comparisons drop a NaN, a NaN enters as +inf
        double m = (knmin[b] == 0) ? __builtin_inf() : scr_unkey(~knmin[b]);
        double M = (kmax[b] == 0) ? -__builtin_inf() : scr_unkey(kmax[b]);
        const double vM = (v == v) ? v : __builtin_inf();
        m = (v < m) ? v : m;
        M = (vM > M) ? vM : M;
        kmax[b] = scr_key(M);
        knmin[b] = ~scr_key(m);
      }
  for (int bz = 0; bz < s.nb[2]; bz++)
    for (int by = 0; by < s.nb[1]; by++)
      for (int bx = 0; bx < s.nb[0]; bx++)
        quiet[scr_index(s, bx, by, bz)] = scr_block_quiet(s, kmax, knmin, bx, by, bz) ? 1 : 0;
  delete[] kmax;
}

// round trip of the key encoding, and its order: returns 1 when key(a) < key(b)
int hs_key_less(double a, double b) { return scr_key(a) < scr_key(b) ? 1 : 0; }
double hs_key_roundtrip(double a) { return scr_unkey(scr_key(a)); }

}  // extern "C"
