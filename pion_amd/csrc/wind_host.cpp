// wind_host.cpp -- the host arithmetic and bookkeeping of the wind sources (wind_host.h), in plain double with the
// reference's expressions in their order.  Built with -ffp-contract=off: no expression here may be contracted.
#include "wind_host.h"

#include <algorithm>
#include <cmath>
#include <cstring>

namespace pion::impl {

// constants::equalD (constants.cpp:48-68)
static bool equalD(const double a, const double b)
{
  if (a == b) return true;
  if (fabs(a) + fabs(b) < 1.0e-100) return true;
  return (fabs(a - b) / (fabs(a) + fabs(b) + 1.0e-100)) < 1.0e-12;
}

// What the interpolations of interpolate_arrays start from, as written (tools/interpolate.cpp:121-150, :300-345):
// bisection to the nodes x[ilo], x[ihi] around xreq, and xreq clamped to them (zero slope outside the table)
static double bracket(const double *x, const size_t len, const double xreq, size_t &ilo, size_t &ihi)
{
  size_t imid = 0;
  ihi = len - 1, ilo = 0;
  do {
    imid = ilo + (size_t)floor((ihi - ilo) / 2.0);
    if (x[imid] < xreq) ilo = imid;
    else ihi = imid;
  } while (ihi - ilo > 1);
  if (xreq > x[ihi]) return x[ihi];
  if (xreq < x[ilo]) return x[ilo];
  return xreq;
}

// interpolate_arrays::root_find_linear_vec (tools/interpolate.cpp:121-161)
static double root_find_linear_vec(const std::vector<double> &xarr, const std::vector<double> &yarr, const double xreq)
{
  size_t ilo, ihi;
  const double xval = bracket(xarr.data(), xarr.size(), xreq, ilo, ihi);
  return yarr[ilo] + (yarr[ihi] - yarr[ilo]) * (xval - xarr[ilo]) / (xarr[ihi] - xarr[ilo]);
}

// BC_update_STWIND's new source position (stellar_wind_boundaries.cpp:294-314): the ellipse in the x-y plane.  abs is
// std::abs(double) there; pconst.pi() and pconst.year() are constants.h:45,107.  z stays at dpos_init.
void wind_orbit_position(const pion_gpu_wind_source &s, const int ndim, const double simtime, double *pos)
{
  for (int v = 0; v < 3; v++) pos[v] = (v < ndim) ? s.pos[v] : 0.0;
  if (s.orbit_period == 0) return;
  const double pi = 3.14159265358979324, year = 3.1558150e7;
  const double px = s.orbit_periastron[0], py = s.orbit_periastron[1];
  const double f = s.orbit_ecc_fac, P = s.orbit_period;
  const double cos_a = -1 * px / std::abs(px) * cos(atan(py / px));
  const double sin_a = sin(-1 * py / std::abs(py) * acos(cos_a));
  const double a = sqrt(px * px + py * py) * f;
  const double e = a * (f - 1) / f;
  const double b = sqrt(a * a - e * e);
  const double sin_t = sin(2 * pi * simtime / (P * year));
  const double cos_t = cos(2 * pi * simtime / (P * year));
  pos[0] = s.pos[0] - a * cos_a + cos_a * a * cos_t - sin_a * b * sin_t;
  pos[1] = s.pos[1] - a * sin_a + sin_a * a * cos_t + cos_a * b * sin_t;
}

// ---- rotating stars, LGM99 (grid/stellar_wind_angle.cpp): the tables of setup_tables (:92-212) and the fn_*
// functions.  pconst.pi(), sqrt2() are constants.h:45,48; pow_fast(a, b) = exp(b*log(a)) (constants.cpp:78-84);
// ONE_MINUS_EPS = 1 - 1e-12 (constants.h:157).  c_gamma = 0.35, c_beta = -1 (unused), c_xi = xi (:58-63).
namespace lgm99 {
const double pi = 3.14159265358979324, sqrt2 = 1.4142135623730950, c_gamma = 0.35;

static double pow_fast(const double a, const double b) { return exp(b * log(a)); }

// stellar_wind::beta (stellar_wind_BC.cpp:820-867)
static double beta(const double Teff)
{
  // its piecewise-linear knots (rsg = 0.125 below 3600 K)
  const double Tk[6] = {3600.0, 6000.0, 8000.0, 10000.0, 20000.0, 22000.0}, bk[6] = {0.125, 0.5, 0.7, 1.3, 1.3, 2.6};
  if (Teff <= Tk[0]) return bk[0];
  if (Teff >= Tk[5]) return bk[5];
  int i = 0;
  while (i < 4 && !(Teff < Tk[i + 1])) i++;
  return bk[i] + (Teff - Tk[i]) * (bk[i + 1] - bk[i]) / (Tk[i + 1] - Tk[i]);
}

// fn_phi (:286-294)
static double fn_phi(const double omega, const double theta, const double Teff)
{
  const double ans = (omega / (22.0 * sqrt2 * beta(Teff))) * sin(theta) * pow_fast(1.0 - omega * sin(theta), -c_gamma);
  const double cap = 0.5 * pi * (1.0 - 1.0e-12);
  return (cap < ans) ? cap : ans;   // std::min(ans, cap)
}

// fn_alpha (:304-315)
static double fn_alpha(const double omega, const double theta, const double Teff)
{
  return pow_fast(cos(fn_phi(omega, theta, Teff)) + pow_fast(tan(theta), -2.0) *
                                                        (1.0 + c_gamma * (omega * sin(theta) / (1.0 - omega * sin(theta)))) *
                                                        fn_phi(omega, theta, Teff) * sin(fn_phi(omega, theta, Teff)),
                  -1.0);
}

// integrand (:222-229), integrate_Simpson (:239-276), fn_delta (:325-333)
static double integrand(const double theta, const double omega, const double Teff, const double xi)
{
  return fn_alpha(omega, theta, Teff) * pow_fast(1.0 - omega * sin(theta), xi) * sin(theta);
}

static double fn_delta(const double omega, const double Teff, const double xi)
{
  const double min = 0.001, max = pi / 2.0;
  const long npt = 230;
  const double hh = (max - min) / npt;
  double ans = 0.0;
  ans += integrand(min, omega, Teff, xi);
  ans += integrand(max, omega, Teff, xi);
  int wt = 4;
  double x = 0.0;
  for (long i = 1; i < npt; i++) {
    x = min + i * hh;
    ans += wt * integrand(x, omega, Teff, xi);
    wt = 6 - wt;
  }
  ans *= hh / 3.0;
  return 2.0 * pow_fast(ans, -1.0);
}

// setup_tables (:92-212)
static void setup_tables(const double xi, AngleTables &T)
{
  T.xi = xi;
  const int nth = ANGLE_NTHETA, nom = ANGLE_NOMEGA, nT = ANGLE_NTEFF;
  const double theta_min = 0.1, theta_mid = 60.0, theta_max = 89.9;
  for (int k = 0; k < nth; k++) {
    if (k <= 4) T.theta[k] = (theta_min + k * ((theta_mid - theta_min) / 4.0)) * (pi / 180.0);
    else T.theta[k] = (theta_mid + (k - 4) * ((theta_max - theta_mid) / (nth - 5))) * (pi / 180.0);
  }
  double log_mu[ANGLE_NOMEGA];
  for (int i = 0; i < nom; i++) log_mu[nom - i - 1] = -4.0 + i * (4.0 / (nom - 1));
  for (int j = 0; j < nom; j++) T.omega[j] = 1 - pow_fast(10, log_mu[j]);
  const double T0 = 1000.0, T1 = 3600.0, T2 = 6000.0, T3 = 8000.0, T4 = 10000.0, T5 = 20000.0, T6 = 22000.0,
               T7 = 150000.0;
  for (int i = 0; i < nT; i++) {
    if (i == 0) T.Teff[i] = T0;
    if (i == 1) T.Teff[i] = T1;
    if (2 <= i && i <= 6) T.Teff[i] = T1 + i * ((T2 - T1) / 6);
    if (i == 7) T.Teff[i] = T2;
    if (8 <= i && i <= 10) T.Teff[i] = T2 + (i - 6) * ((T3 - T2) / 4);
    if (i == 11) T.Teff[i] = T3;
    if (12 <= i && i <= 14) T.Teff[i] = T3 + (i - 10) * ((T4 - T3) / 4);
    if (i == 15) T.Teff[i] = T4;
    if (i == 16) T.Teff[i] = T5;
    if (17 <= i && i <= 19) T.Teff[i] = T5 + (i - 15) * ((T6 - T5) / 4);
    if (i == 20) T.Teff[i] = T6;
    if (i == 21) T.Teff[i] = T7;
  }
  T.delta.assign((size_t)nom * nT, 0.0);
  for (int i = 0; i < nom; i++)
    for (int j = 0; j < nT; j++) T.delta[(size_t)i * nT + j] = fn_delta(T.omega[i], T.Teff[j], xi);
  T.alpha.assign((size_t)nom * nth * nT, 0.0);
  for (int i = 0; i < nom; i++)
    for (int j = 0; j < nth; j++)
      for (int k = 0; k < nT; k++) T.alpha[((size_t)i * nth + j) * nT + k] = fn_alpha(T.omega[i], T.theta[j], T.Teff[k]);
}

// interpolate_arrays::root_find_bilinear_vec (tools/interpolate.cpp:300-380) on delta(omega, Teff)
static double delta_interp(const AngleTables &T, const double xr, const double yr)
{
  const double *x = T.omega, *y = T.Teff;
  size_t ilo, ihi, jlo, jhi;
  const double xval = bracket(x, ANGLE_NOMEGA, xr, ilo, ihi), yval = bracket(y, ANGLE_NTEFF, yr, jlo, jhi);
  const size_t nT = ANGLE_NTEFF;
  const std::vector<double> &f = T.delta;
  double result = (f[ilo * nT + jlo] * (x[ihi] - xval) * (y[jhi] - yval) + f[ihi * nT + jlo] * (xval - x[ilo]) * (y[jhi] - yval) +
                   f[ilo * nT + jhi] * (x[ihi] - xval) * (yval - y[jlo]) + f[ihi * nT + jhi] * (xval - x[ilo]) * (yval - y[jlo]));
  result /= ((x[ihi] - x[ilo]) * (y[jhi] - y[jlo]));
  return result;
}
}  // namespace lgm99

// omega of a rotating source: fn_density_interp's std::min(std::min(0.9999, v_rot/vcrit), 0.999)
// (stellar_wind_angle.cpp:395, :493); fn_v_inf's clip (:350) gives the same value
static double angle_omega(const double vrot, const double vcrit)
{
  return std::min(std::min(0.9999, vrot / vcrit), 0.999);
}

AngleBracket angle_bracket(const AngleTables &T, const WindNow &N)
{
  AngleBracket b;
  const double om = angle_omega(N.vrot, N.vcrit), Tw = N.Tw;
  b.omega = om;
  b.delta = lgm99::delta_interp(T, om, Tw);
  // root_find_trilinear_vec's omega and Teff brackets (while (x > x_vec[i]) i++; wind_angle_in_range keeps i >= 1)
  int xi = 0, zi = 0;
  while (xi < ANGLE_NOMEGA - 1 && om > T.omega[xi]) xi++;
  while (zi < ANGLE_NTEFF - 1 && Tw > T.Teff[zi]) zi++;
  xi = std::max(xi, 1);
  zi = std::max(zi, 1);
  b.dx = (om - T.omega[xi - 1]) / (T.omega[xi] - T.omega[xi - 1]);
  b.dz = (Tw - T.Teff[zi - 1]) / (T.Teff[zi] - T.Teff[zi - 1]);
  const int nth = ANGLE_NTHETA, nT = ANGLE_NTEFF;
  for (int j = 0; j < nth; j++) {
    b.a[0][j] = T.alpha[((size_t)(xi - 1) * nth + j) * nT + zi - 1];
    b.a[1][j] = T.alpha[((size_t)(xi - 1) * nth + j) * nT + zi];
    b.a[2][j] = T.alpha[((size_t)xi * nth + j) * nT + zi - 1];
    b.a[3][j] = T.alpha[((size_t)xi * nth + j) * nT + zi];
  }
  return b;
}

// the table of an evolving or rotating source at time t (tr[v]: the element column tracer v follows, if any)
struct WindValues {
  double Teff, Mdot, vinf, vrot, R, vcrit;
  double tr[PION_MAX_NVAR];
};

static WindValues wind_table_at(const WindSource &W, const int ntracer, const double t)
{
  WindValues v;
  v.Teff = root_find_linear_vec(W.t, W.Teff, t);
  v.Mdot = root_find_linear_vec(W.t, W.Mdot, t);
  v.vinf = root_find_linear_vec(W.t, W.vinf, t);
  v.vrot = root_find_linear_vec(W.t, W.vrot, t);
  v.R = root_find_linear_vec(W.t, W.R, t);
  v.vcrit = (W.type == 2) ? root_find_linear_vec(W.t, W.vcrit, t) : 0.0;
  for (int k = 0; k < PION_MAX_NVAR; k++)
    v.tr[k] = (k < ntracer && W.elem[k] >= 0) ? root_find_linear_vec(W.t, W.X[W.elem[k]], t) : 0.0;
  return v;
}

// v, all cgs, become the values the source writes with; a rotating source: Tw = std::min(Twind, Teff_vec.back())
// and vcrit (stellar_wind_angle.cpp:972-984)
static void wind_now_set(const WindSource &W, const AngleTables &T, const int ntracer, const WindValues &v, WindNow &N)
{
  N.Tw = v.Teff;
  N.Mdot = v.Mdot;
  N.vrot = v.vrot;
  N.Vinf = v.vinf;
  N.Rstar = v.R;
  for (int k = 0; k < ntracer; k++)
    if (W.elem[k] >= 0) N.tr[k] = v.tr[k];
  if (W.type == 2) {
    N.Tw = std::min(N.Tw, T.Teff[ANGLE_NTEFF - 1]);
    N.vcrit = v.vcrit;
  }
}

// stellar_wind_evolution::update_source (stellar_wind_BC.cpp:1250-1330; rotating sources: stellar_wind_angle.cpp
// :941-1019): every step from tstart on (:1266), values clamped after tfinish
bool wind_source_update(const WindSource &W, const AngleTables &T, const int ntracer, const double simtime, WindNow &N)
{
  if ((W.type == 1 || W.type == 2) && simtime >= N.t_next_update) {
    N.active = true;
    N.t_next_update = std::min(simtime, W.tfinish);
    wind_now_set(W, T, ntracer, wind_table_at(W, ntracer, simtime), N);
  }
  return N.active;
}

bool wind_angle_in_range(const WindSource &W, const AngleTables &T, const int ntracer, const double simtime)
{
  WindNow N = W.now;
  if (!wind_source_update(W, T, ntracer, simtime, N)) return true;
  return angle_omega(N.vrot, N.vcrit) > T.omega[0] && N.Tw > T.Teff[0];
}

// the reference's rep.error conditions (stellar_wind_BC.cpp:140-217, :331-360, :1140-1145, :517-519;
// stellar_wind_angle.cpp:714-716, :912-923) and the limits of this path.  The first that holds wins.
static const char *wind_source_check(const pion_gpu_config &cfg, const pion_gpu_wind_source &src, const double *evo_vcrit,
                                     const bool rotating, const double xi, const std::vector<WindSource> &present,
                                     const AngleTables &T)
{
  auto beside = [&](const int type) {
    return std::any_of(present.begin(), present.end(), [=](const WindSource &o) { return o.type == type; });
  };
  // a divergence: in the reference's stellar_wind_angle object an evolving source would get LGM99 updates
  const char *const mixed = "wind source: evolving and rotating sources cannot share a grid";
  // (cylindrical grids are 2-D: pion_gpu_create)
  const char *const off_axis =
      (cfg.coord_sys == 2 && !equalD(src.pos[1], 0.0)) ? "Axisymmetry but source not at R=0!" : nullptr;
  if (present.size() >= PION_MAX_WIND_SOURCES) return "wind source: at most PION_MAX_WIND_SOURCES sources";
  if (!rotating) {
    if (src.type == 2 || src.type == 3) return "wind source: angle / latitude-dependent winds are not supported";
    if (src.type != 0 && src.type != 1) return "What type of source is this?  add a new type?";
    if (src.type == 1 && beside(2)) return mixed;
  }
  else {
    if (src.type != 2) return "Bad wind type for evolving stellar wind (rotating star)!";
    if (cfg.ndim < 2) return "rotating wind source: needs a 2-D or 3-D grid (theta = 0 in 1-D)";
    if (off_axis) return off_axis;
    if (src.orbit_period != 0) return "rotating wind source: add_rotating_source takes no orbit";
  }
  if (!(src.radius > 0.0)) return "wind source: radius must be > 0";
  if (!rotating) {
    if (cfg.coord_sys == 3 && !equalD(src.pos[0], 0.0)) return "Spherical symmetry but source not at origin!";
    if (off_axis) return off_axis;
    if (cfg.ndim == 1 && cfg.eqntype != PION_EQEUL) return "1D spherical but MHD?";
    // a divergence: the reference would move a source on the axis (cylindrical) or at the origin (spherical) off it
    if (src.orbit_period != 0 && (cfg.ndim < 2 || cfg.coord_sys != 1))
      return "wind source: orbital motion needs a 2-D or 3-D Cartesian grid";
  }
  if (src.type != 0) {
    if (src.npt < 2) return "evolving wind source: the table needs at least 2 rows";
    if (!src.evo_time || !src.evo_Teff || !src.evo_Mdot || !src.evo_vrot || !src.evo_vinf || !src.evo_R ||
        (rotating && !evo_vcrit))
      return "evolving wind source: missing table column";
    for (int v = 0; v < cfg.ntracer; v++) {
      const int e = src.evo_tracer_elem[v];
      if (e < -1 || e > 6 || (e >= 0 && !src.evo_X[e])) return "evolving wind source: bad tracer selector";
    }
  }
  if (rotating) {
    if (beside(1)) return mixed;
    // stellar_wind_angle holds one c_xi (the reference's errorTest on WIND_i_xi)
    if (beside(2) && !(xi == T.xi)) return "rotating wind source: xi differs from an earlier source's";
  }
  return nullptr;
}

const char *wind_source_setup(const pion_gpu_config &cfg, const pion_gpu_wind_source &src, const double *evo_vcrit,
                              const bool rotating, const double xi, const std::vector<WindSource> &present,
                              AngleTables &T, WindSource &W)
{
  if (const char *m = wind_source_check(cfg, src, evo_vcrit, rotating, xi, present, T)) return m;
  if (rotating && (T.delta.empty() || !(xi == T.xi))) lgm99::setup_tables(xi, T);
  W.type = src.type;
  for (int a = 0; a < 3; a++) W.pos[a] = (a < cfg.ndim) ? src.pos[a] : 0.0;
  W.radius = src.radius;
  W.Bstar = src.Bstar;
  WindNow &N = W.now;
  for (int v = 0; v < PION_MAX_NVAR; v++) {
    N.tr[v] = (v < cfg.ntracer) ? src.tracers[v] : 0.0;
    W.elem[v] = (W.type != 0 && v < cfg.ntracer) ? src.evo_tracer_elem[v] : -1;
  }
  // Teff, Mdot, vinf, vrot, R, vcrit
  WindValues v = {src.Tw, src.mdot, src.vinf, src.vrot, src.Rstar, 0.0, {}};
  if (W.type != 0) {
    // add_evolving_source (stellar_wind_BC.cpp:1109-1245; stellar_wind_angle.cpp:700-827 + add_rotating_source
    // :836-932): the source is active at set-up if it starts within one update interval
    const int n = src.npt;
    auto col = [n](const double *p) { return p ? std::vector<double>(p, p + n) : std::vector<double>(); };
    W.t = col(src.evo_time), W.Teff = col(src.evo_Teff), W.Mdot = col(src.evo_Mdot), W.vrot = col(src.evo_vrot);
    W.vinf = col(src.evo_vinf), W.R = col(src.evo_R), W.vcrit = col(rotating ? evo_vcrit : nullptr);
    for (int e = 0; e < 7; e++) W.X[e] = col(src.evo_X[e]);
    W.tstart = W.t[0];
    W.tfinish = W.t[n - 1];
    const double t_now = src.t_now;
    N.t_next_update = std::max(W.tstart, t_now);
    N.active = ((t_now + src.update_freq) > W.tstart || equalD(W.tstart, t_now)) && t_now < W.tfinish;
    // an inactive source's sentinels; its element tracers are 0
    const WindValues off_evolving = {-100.0, -100.0, -100.0, 0.0, 0.0, 0.0, {}};
    const WindValues off_rotating = {-100.0, -100.0, -100.0, -100.0, 0.0, 0.0, {}};
    v = N.active ? wind_table_at(W, cfg.ntracer, t_now) : (W.type == 1 ? off_evolving : off_rotating);
  }
  wind_now_set(W, T, cfg.ntracer, v, N);
  if (W.type != 2) {
    // stellar_wind::add_source (:166-176): Msun/yr and km/s to cgs.  An evolving source's table values, already cgs,
    // pass through it too (update_source overwrites them at the first update); a rotating source's do not.
    N.Mdot = N.Mdot * 1.9891e33 / 3.1558150e7;
    N.Vinf = N.Vinf * 1.0e5;
    N.vrot = N.vrot * 1.0e5;
  }
  if (src.orbit_period != 0) {
    W.moving = true;
    W.orbit = src;
    for (int a = 0; a < 3; a++) W.orbit.pos[a] = W.pos[a];   // dpos_init
  }
  return nullptr;
}

}  // namespace pion::impl

extern "C" {

int pion_gpu_wind_angle_tables(double xi, double *theta, double *omega, double *Teff, double *delta, double *alpha)
{
  pion::impl::AngleTables T;
  pion::impl::lgm99::setup_tables(xi, T);
  if (theta) memcpy(theta, T.theta, sizeof T.theta);
  if (omega) memcpy(omega, T.omega, sizeof T.omega);
  if (Teff) memcpy(Teff, T.Teff, sizeof T.Teff);
  if (delta) memcpy(delta, T.delta.data(), sizeof(double) * T.delta.size());
  if (alpha) memcpy(alpha, T.alpha.data(), sizeof(double) * T.alpha.size());
  return 0;
}

int pion_gpu_wind_orbit_position(const pion_gpu_wind_source *src, int ndim, double simtime, double *pos)
{
  if (!src || !pos || ndim < 2 || ndim > 3) return PION_GPU_EINVAL;
  double p[3];
  pion::impl::wind_orbit_position(*src, ndim, simtime, p);
  for (int a = 0; a < PION_MAX_DIM; a++) pos[a] = (a < 3) ? p[a] : 0.0;
  return 0;
}

}  // extern "C"
