// TEST INFRASTRUCTURE: the host part of the wind sources (pion_amd/csrc/wind_host.cpp, compiled together with this
// file) run without a device: set-up of one source, then update steps, as pion_wind.hip drives them.
//
// stdin, numbers separated by white space (doubles as C hex floats or decimals):
//   ndim coord_sys eqntype ntracer
//   npresent type[npresent] xi_present     sources already on the grid; the xi their LGM99 tables were built with
//   rotating xi                            the entry point: 1 = pion_gpu_add_rotating_wind_source
//   pos[3] radius type mdot vinf vrot Tw Rstar Bstar t_now update_freq orbit_ecc_fac periastron[2] orbit_period
//   tracers[ntracer] elem[ntracer] npt
//   14 columns (time Teff Mdot vrot vinf R vcrit X[7]), each: 0 (absent), or 1 and npt values
//   ntimes time[ntimes]
// stdout: "rc 0" or "rc -1 <error text>"; after set-up and after each time "state active t_next_update Mdot Vinf
// vrot vcrit Tw Rstar tr[ntracer]" (%a); before each time's state "check 0|1": whether the pre-check of a boundary
// update accepts the time (a refused time leaves the source as it is, as the update returns before it writes).
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <string>

#include "../../pion_amd/csrc/wind_host.h"

using namespace pion::impl;

static double num()
{
  std::string s;
  if (!(std::cin >> s)) {
    fprintf(stderr, "wind_host_probe: input ends early\n");
    exit(2);
  }
  return strtod(s.c_str(), nullptr);
}

static void print_state(const WindNow &N, const int ntracer)
{
  printf("state %d %a %a %a %a %a %a %a", N.active ? 1 : 0, N.t_next_update, N.Mdot, N.Vinf, N.vrot, N.vcrit, N.Tw,
         N.Rstar);
  for (int v = 0; v < ntracer; v++) printf(" %a", N.tr[v]);
  printf("\n");
}

int main()
{
  pion_gpu_config cfg = {};
  cfg.ndim = (int)num();
  cfg.coord_sys = (int)num();
  cfg.eqntype = (int)num();
  cfg.ntracer = (int)num();
  std::vector<WindSource> present((size_t)num());
  bool built = false;
  for (WindSource &o : present) {
    o.type = (int)num();
    built = built || o.type == 2;
  }
  AngleTables T;
  const double xi_present = num();
  if (built) {
    // what set-up of the first rotating source left: the tables for its xi
    T.xi = xi_present;
    T.delta.resize((size_t)ANGLE_NOMEGA * ANGLE_NTEFF);
    T.alpha.resize((size_t)ANGLE_NOMEGA * ANGLE_NTHETA * ANGLE_NTEFF);
    pion_gpu_wind_angle_tables(T.xi, T.theta, T.omega, T.Teff, T.delta.data(), T.alpha.data());
  }
  const bool rotating = num() != 0;
  const double xi = num();
  pion_gpu_wind_source src = {};
  for (int a = 0; a < 3; a++) src.pos[a] = num();
  src.radius = num();
  src.type = (int)num();
  src.mdot = num(), src.vinf = num(), src.vrot = num(), src.Tw = num(), src.Rstar = num(), src.Bstar = num();
  src.t_now = num(), src.update_freq = num();
  src.orbit_ecc_fac = num(), src.orbit_periastron[0] = num(), src.orbit_periastron[1] = num(), src.orbit_period = num();
  for (int v = 0; v < PION_MAX_NVAR; v++) src.evo_tracer_elem[v] = -1;
  for (int v = 0; v < cfg.ntracer; v++) src.tracers[v] = num();
  for (int v = 0; v < cfg.ntracer; v++) src.evo_tracer_elem[v] = (int)num();
  src.npt = (int)num();
  std::vector<double> col[14];
  const double *ptr[14];
  for (int c = 0; c < 14; c++) {
    const bool have = num() != 0;
    for (int k = 0; have && k < src.npt; k++) col[c].push_back(num());
    ptr[c] = have ? col[c].data() : nullptr;
  }
  src.evo_time = ptr[0], src.evo_Teff = ptr[1], src.evo_Mdot = ptr[2], src.evo_vrot = ptr[3], src.evo_vinf = ptr[4];
  src.evo_R = ptr[5];
  for (int e = 0; e < 7; e++) src.evo_X[e] = ptr[7 + e];

  WindSource W;
  if (const char *m = wind_source_setup(cfg, src, ptr[6], rotating, xi, present, T, W)) {
    printf("rc %d %s\n", PION_GPU_EINVAL, m);
    return 0;
  }
  printf("rc 0\n");
  print_state(W.now, cfg.ntracer);
  const int ntimes = (int)num();
  for (int k = 0; k < ntimes; k++) {
    const double t = num();
    const bool ok = W.type != 2 || wind_angle_in_range(W, T, cfg.ntracer, t);
    printf("check %d\n", ok ? 1 : 0);
    if (ok) wind_source_update(W, T, cfg.ntracer, t, W.now);
    print_state(W.now, cfg.ntracer);
  }
  return 0;
}
