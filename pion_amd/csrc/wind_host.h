// wind_host.h -- the host-only part of the wind sources (wind_host.cpp): tables and bookkeeping of a source, set-up,
// the update step, the LGM99 tables.  Plain C++, no HIP: it builds and runs without a device, under a sanitiser too
// (tests/native/wind_host_probe.cpp).  What touches the device is pion_wind.hip.
#ifndef PION_WIND_HOST_H
#define PION_WIND_HOST_H

#include <cstddef>
#include <vector>

#include "../../include/pion_gpu.h"

#pragma GCC visibility push(hidden)   // internal to libpion_gpu.so
namespace pion::impl {

// The knots of the LGM99 tables: dev_wind.h's PION_ANGLE_*.  That header defines kernels, so only pion_wind.hip
// includes it, and asserts there that these are its values.
constexpr int ANGLE_NTHETA = 25, ANGLE_NOMEGA = 25, ANGLE_NTEFF = 22;

// stellar_wind_angle's look-up tables for one xi (setup_tables, grid/stellar_wind_angle.cpp:92-212); empty: not built
struct AngleTables {
  double xi = 0.0;
  double theta[ANGLE_NTHETA], omega[ANGLE_NOMEGA], Teff[ANGLE_NTEFF];
  std::vector<double> delta;   // [omega][Teff]
  std::vector<double> alpha;   // [omega][theta][Teff]
};

// what the next boundary update writes with (wind_source, cgs) and evolving_wind_data's t_next_update, is_active
struct WindNow {
  double Mdot = 0.0, Vinf = 0.0, vrot = 0.0, vcrit = 0.0, Tw = 0.0, Rstar = 0.0;
  double tr[PION_MAX_NVAR];
  bool active = true;
  double t_next_update = 1.0e99;
};

// one pion_gpu_add_wind_source source: its table (evolving_wind_data: tstart, tfinish), its values now, its cells
struct WindSource {
  int type = 0;
  double pos[3] = {0.0, 0.0, 0.0};
  double radius = 0.0, Bstar = 0.0;
  std::vector<double> t, Teff, Mdot, vrot, vinf, R, X[7];
  std::vector<double> vcrit;   // rotating source (type 2): the vcrit column
  int elem[PION_MAX_NVAR];
  double tstart = 0.0, tfinish = 0.0;
  WindNow now;
  long off = 0, n = 0;   // range in the concatenated cell list (moving source: n = its capacity, the box size)
  // orbital motion (orbit_period != 0): the position at set-up (dpos_init), the orbit, the box the cells are found
  // in, the device count the compaction writes, and the compaction's scratch (all sized at set-up)
  bool moving = false;
  pion_gpu_wind_source orbit;   // pos = dpos_init, orbit_* (the pointers are not used)
  int box_w[3] = {1, 1, 1};
  long *dn = nullptr;
  void *dscan = nullptr;
  size_t scan_bytes = 0;
};

// BC_update_STWIND's new source position, pos[3]
void wind_orbit_position(const pion_gpu_wind_source &s, int ndim, double simtime, double *pos);

// Set-up of one source, for both entry points (rotating: pion_gpu_add_rotating_wind_source, with its evo_vcrit and
// xi): every EINVAL that needs no device, then T (re)built for xi where a rotating source needs it, then W filled,
// all but its cells.  Returns the error text, or nullptr.
const char *wind_source_setup(const pion_gpu_config &cfg, const pion_gpu_wind_source &src, const double *evo_vcrit,
                              bool rotating, double xi, const std::vector<WindSource> &present, AngleTables &T,
                              WindSource &W);

// update_source at simtime on N: W.now, or a copy of it.  Returns whether the source writes its cells.
bool wind_source_update(const WindSource &W, const AngleTables &T, int ntracer, double simtime, WindNow &N);

// false: rotating source W would write at simtime with omega <= omega_vec[0] or Tw <= Teff_vec[0], for which
// root_find_trilinear_vec calls rep.error (tools/interpolate.cpp:420-440).  W stays as it is.
bool wind_angle_in_range(const WindSource &W, const AngleTables &T, int ntracer, double simtime);

// the parts of fn_density_interp that do not depend on the cell, as dev_wind.h's WindAngleDev holds them
struct AngleBracket {
  double omega, delta, dx, dz;
  double a[4][ANGLE_NTHETA];
};
AngleBracket angle_bracket(const AngleTables &T, const WindNow &N);

}  // namespace pion::impl
#pragma GCC visibility pop
#endif
