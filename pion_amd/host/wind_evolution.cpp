// wind_evolution.cpp -- stellar_wind_evolution::read_evolution_file (grid/stellar_wind_BC.cpp:1026-1100) and the
// time shift of add_evolving_source (:1160-1170), for pion_gpu_wind_source tables.
#include <cmath>
#include <cstdio>
#include <vector>

#include "../../include/pion_host.h"

extern "C" long pion_host_read_wind_evolution(const char *path, double time_offset, double t_scalefac, long cap,
                                              double *table)
{
  if (!path || !(t_scalefac != 0.0)) return PION_GPU_EINVAL;
  FILE *wf = fopen(path, "r");
  if (!wf) return PION_GPU_EINVAL;
  char line[512];
  // two header lines
  if (!fgets(line, 512, wf) || !fgets(line, 512, wf)) {
    fclose(wf);
    return PION_GPU_EINVAL;
  }
  // format: time M L Teff Mdot vrot vcrit vinf [X_H X_He X_C X_N X_O X_Z X_D], cgs.  The values live outside the
  // loop, as in the reference: a column a line does not have keeps the previous line's value (0 at first).
  double time = 0.0, mass = 0.0, lumi = 0.0, teff = 0.0, mdot = 0.0, vrot = 0.0, vcrt = 0.0, vinf = 0.0;
  double xh = 0.0, xhe = 0.0, xc = 0.0, xn = 0.0, xo = 0.0, xz = 0.0, xd = 0.0;
  std::vector<double> rows;
  while (fgets(line, 512, wf)) {
    const int got = sscanf(line, "   %lE   %lE %lE %lE %lE %lE %lE %lE %lE %lE %lE %lE %lE %lE %lE", &time, &mass,
                           &lumi, &teff, &mdot, &vrot, &vcrt, &vinf, &xh, &xhe, &xc, &xn, &xo, &xz, &xd);
    // a line with no number at all (a further comment line, a blank line) is not a row here; the reference
    // would append a copy of the previous values for it (wind sources)
    if (got < 1) continue;
    // R = sqrt(L / (4 pi sigma Teff^4)), pconst.pow_fast(teff, 4.0) = exp(4*log(teff)) (constants.h:45,55)
    const double radi = sqrt(lumi / (4.0 * 3.14159265358979324 * 5.670367e-5 * exp(4.0 * log(teff))));
    const double r[PION_WND_NCOL] = {(time + time_offset) / t_scalefac, mass, lumi, teff, mdot, vrot, vcrt, vinf,
                                     xh, xhe, xc, xn, xo, xz, xd, radi};
    rows.insert(rows.end(), r, r + PION_WND_NCOL);
  }
  fclose(wf);
  const long n = (long)(rows.size() / PION_WND_NCOL);
  if (table) {
    if (cap < n) return PION_GPU_EINVAL;
    for (long i = 0; i < n; i++)
      for (int c = 0; c < PION_WND_NCOL; c++) table[c * cap + i] = rows[i * PION_WND_NCOL + c];
  }
  return n;
}
