// cooling_tables.cpp -- host-side builder of the mp_only_cooling look-up tables.
//
// Restates, for EP.cooling = 8 (WSS09_CIE_LINE_HEAT_COOL), what the reference does once at
// start-up: mp_only_cooling::gen_mpoc_lookup_tables (microphysics/mp_only_cooling.cpp:528-579)
// on top of cooling_function_SD93CIE::cooling_rate_SD93CIE (cooling_SD93_cie.cpp:666-704, natural
// cubic spline through the WSS09 metals-only curve in log-log space, power-law extrapolation)
// and Hummer94_Hrecomb::{Hii_rad_recomb_rate, Hii_total_cooling}
// (hydrogen_recomb_Hummer94.cpp:38-147,165-278, natural cubic splines of rate/sqrt(T) in T).
//
// The reference evaluates its splines with GSL's gsl_interp_cspline (natural boundary
// conditions; tools/interpolate.cpp:73-110).  GSL is not available here, so the spline is
// restated from its published definition and this boundary is "parity unpinned": it is
// cross-checked against scipy's natural CubicSpline (tests/test_cooling.py), not against the
// reference.
//
// C-ABI (plain pointers), called by the host driver before pion_gpu_set_cooling_tables.
#include <cmath>
#include <cstdio>
#include <fstream>
#include <sstream>
#include <string>
#include <vector>

#include "cooling_data.h"

namespace {

// natural cubic spline in the representation GSL uses (cspline.c): second-derivative
// coefficients c[i] with c[0]=c[n-1]=0; eval: y_i + d*(b_i + d*(c_i + d*d_i))
struct Spline {
  std::vector<double> x, y, c;
  void init(const double *xa, const double *ya, int n)
  {
    x.assign(xa, xa + n);
    y.assign(ya, ya + n);
    c.assign(n, 0.0);
    const int sys = n - 2;  // unknowns c[1..n-2]
    if (sys <= 0) return;
    std::vector<double> diag(sys), off(sys), g(sys);
    for (int i = 0; i < sys; i++) {
      const double h_i = x[i + 1] - x[i];
      const double h_ip1 = x[i + 2] - x[i + 1];
      const double ydiff_i = y[i + 1] - y[i];
      const double ydiff_ip1 = y[i + 2] - y[i + 1];
      const double g_i = (h_i != 0.0) ? 1.0 / h_i : 0.0;
      const double g_ip1 = (h_ip1 != 0.0) ? 1.0 / h_ip1 : 0.0;
      off[i] = h_ip1;
      diag[i] = 2.0 * (h_ip1 + h_i);
      g[i] = 3.0 * (ydiff_ip1 * g_ip1 - ydiff_i * g_i);
    }
    // symmetric tridiagonal solve (Cholesky-like LDL^T, as gsl_linalg_solve_symm_tridiag)
    std::vector<double> gamma(sys), alpha(sys), cc(sys), z(sys);
    alpha[0] = diag[0];
    gamma[0] = (sys > 1) ? off[0] / alpha[0] : 0.0;
    for (int i = 1; i < sys - 1; i++) {
      alpha[i] = diag[i] - off[i - 1] * gamma[i - 1];
      gamma[i] = off[i] / alpha[i];
    }
    if (sys > 1) alpha[sys - 1] = diag[sys - 1] - off[sys - 2] * gamma[sys - 2];
    z[0] = g[0];
    for (int i = 1; i < sys; i++) z[i] = g[i] - gamma[i - 1] * z[i - 1];
    for (int i = 0; i < sys; i++) cc[i] = z[i] / alpha[i];
    std::vector<double> sol(sys);
    sol[sys - 1] = cc[sys - 1];
    for (int i = sys - 2; i >= 0; i--) sol[i] = cc[i] - gamma[i] * sol[i + 1];
    for (int i = 0; i < sys; i++) c[i + 1] = sol[i];
  }
  double eval(double xv) const
  {
    const int n = (int)x.size();
    int lo = 0, hi = n - 1;
    while (hi > lo + 1) {  // gsl_interp_bsearch
      const int i = (hi + lo) / 2;
      if (x[i] > xv) hi = i;
      else lo = i;
    }
    const int i = lo;
    const double dx = x[i + 1] - x[i];
    const double dy = y[i + 1] - y[i];
    const double delx = xv - x[i];
    const double b_i = (dy / dx) - dx * (c[i + 1] + 2.0 * c[i]) / 3.0;
    const double d_i = (c[i + 1] - c[i]) / (3.0 * dx);
    return y[i] + delx * (b_i + delx * (c[i] + delx * d_i));
  }
};

struct Tables {
  Spline wss, ha, hb, ht;
  double wssMinT, wssMaxT, wssMinSlope, wssMaxSlope;
  double hT[31], halpha[31], hbeta[31], hbtot[31];
  double hMinT, hMaxT, minA, maxA, minT_, maxT_;
  Tables()
  {
    wss.init(WSS09_logT, WSS09_logL, 91);
    wssMinT = WSS09_logT[0];
    wssMaxT = WSS09_logT[90];
    wssMinSlope = 8.0;  // cooling_SD93_cie.cpp:530
    wssMaxSlope = (WSS09_logL[90] - WSS09_logL[89]) / (WSS09_logT[90] - WSS09_logT[89]);
    for (int i = 0; i < 31; i++) {
      hT[i] = std::exp(std::log(10.0) * (1.0 + 0.2 * static_cast<double>(i)));
      halpha[i] = H94_caseB[i] / std::sqrt(hT[i]);
      hbeta[i] = H94_coolB[i] / std::sqrt(hT[i]);
      hbtot[i] = H94_coolTot[i] / std::sqrt(hT[i]);
    }
    ha.init(hT, halpha, 31);
    ht.init(hT, hbtot, 31);
    hMinT = hT[0];
    hMaxT = hT[30];
    minA = (std::log10(halpha[1]) - std::log10(halpha[0])) / (std::log10(hT[1]) - std::log10(hT[0]));
    maxA = (std::log10(halpha[30]) - std::log10(halpha[29])) / (std::log10(hT[30]) - std::log10(hT[29]));
    minT_ = (std::log10(hbtot[1]) - std::log10(hbtot[0])) / (std::log10(hT[1]) - std::log10(hT[0]));
    maxT_ = (std::log10(hbtot[30]) - std::log10(hbtot[29])) / (std::log10(hT[30]) - std::log10(hT[29]));
  }
  // cooling_function_SD93CIE::cooling_rate_SD93CIE
  double cooling_rate(double T) const
  {
    if (T < 0.0 || !std::isfinite(T)) return HUGE_VAL;
    double rate;
    T = std::log10(T);
    if (T > wssMaxT) rate = WSS09_logL[90] + wssMaxSlope * (T - wssMaxT);
    else if (T < wssMinT) rate = WSS09_logL[0] + wssMinSlope * (T - wssMinT);
    else rate = wss.eval(T);
    return std::exp(2.3025850929940459 * rate);  // pconst.ln10(), constants.h:44
  }
  double rrr(double T) const
  {
    if (T < 0.0 || !std::isfinite(T)) return HUGE_VAL;
    if (T > hMaxT) return halpha[30] * std::pow(T / hMaxT, maxA);
    if (T < hMinT) return halpha[0] * std::pow(T / hMinT, minA);
    return ha.eval(T);
  }
  double total_cooling(double T) const
  {
    const double kB = 1.381e-16;  // Hummer94_Hrecomb::kB
    if (T < 0.0 || !std::isfinite(T)) return HUGE_VAL;
    double rate;
    if (T > hMaxT) rate = hbtot[30] * std::pow(T / hMaxT, maxT_);
    else if (T < hMinT) rate = hbtot[0] * std::pow(T / hMinT, minT_);
    else rate = ht.eval(T);
    return rate * kB * T;
  }
};

// A total-CIE cooling curve handed over by the caller (EP.cooling = 4..7): the natural spline through (log10 T,
// log10 Lambda) and the two linear extrapolations of cooling_function_SD93CIE (cooling_SD93_cie.cpp:160-164,
// 621-625 set-up; :666-704 evaluation)
struct Curve {
  Spline s;
  double min_slope = 0.0, max_slope = 0.0;
  bool set = false;
  double rate(double T) const
  {
    if (T < 0.0 || !std::isfinite(T) || !set) return HUGE_VAL;
    const int n = (int)s.x.size();
    double rate;
    T = std::log10(T);
    if (T > s.x[n - 1]) rate = s.y[n - 1] + max_slope * (T - s.x[n - 1]);
    else if (T < s.x[0]) rate = s.y[0] + min_slope * (T - s.x[0]);
    else rate = s.eval(T);
    return std::exp(2.3025850929940459 * rate);  // pconst.ln10(), constants.h:44
  }
};
Curve g_curve;

bool curve_ok(int n, const double *logT, const double *logL)
{
  if (n < 2 || n > 256 || !logT || !logL) return false;
  for (int i = 0; i < n; i++) {
    if (!std::isfinite(logT[i]) || !std::isfinite(logL[i])) return false;
    if (i > 0 && !(logT[i] > logT[i - 1])) return false;
  }
  return true;
}

}  // namespace

extern "C" {

// The natural-spline second-derivative coefficients c_out[n] (GSL's cspline representation, c[0] = c[n-1] = 0) of
// the curve (logT[n], logL[n]); 2 <= n <= 256 knots, strictly increasing and finite, else -1.  What
// cooling_function_SD93CIE's set-up leaves in its spline (cooling_SD93_cie.cpp:150-166, 611-627).
int pion_host_build_cooling_curve(int n, const double *logT, const double *logL, double *c_out)
{
  if (!curve_ok(n, logT, logL) || !c_out) return -1;
  Spline s;
  s.init(logT, logL, n);
  for (int i = 0; i < n; i++) c_out[i] = s.c[i];
  return 0;
}

// the process-global curve pion_host_cooling_curve_rate evaluates (tests and fixtures: the one-argument evaluator is
// what a double(double) rate-curve hook takes); -1 and the curve unset for bad input
int pion_host_cooling_curve_set(int n, const double *logT, const double *logL, double min_slope, double max_slope)
{
  g_curve.set = false;
  if (!curve_ok(n, logT, logL) || !std::isfinite(min_slope) || !std::isfinite(max_slope)) return -1;
  g_curve.s.init(logT, logL, n);
  g_curve.min_slope = min_slope;
  g_curve.max_slope = max_slope;
  g_curve.set = true;
  return 0;
}

// cooling_function_SD93CIE::cooling_rate_SD93CIE (cooling_SD93_cie.cpp:666-704) on the curve set above: HUGE_VAL for
// T < 0 or non-finite T (and with no curve set)
double pion_host_cooling_curve_rate(double T) { return g_curve.rate(T); }

// Text file of a curve: two columns, log10 T and log10 Lambda, one knot per line; '#' starts a comment, blank lines
// are skipped.  Fills logT[], logL[] (max_n each) and *n.  Returns 0, or -1 and a message in err[errlen]: unreadable
// file, a line that is not two finite numbers (or has more), fewer than 2 or more than max_n / 256 knots, knots not
// strictly increasing.
int pion_host_read_cooling_curve(const char *path, int max_n, double *logT, double *logL, int *n, char *err, int errlen)
{
  auto fail = [&](const std::string &m) {
    if (err && errlen > 0) std::snprintf(err, (size_t)errlen, "%s", m.c_str());
    return -1;
  };
  if (n) *n = 0;
  if (!path || !logT || !logL || !n || max_n < 2) return fail("read_cooling_curve: bad arguments");
  if (max_n > 256) max_n = 256;
  std::ifstream f(path);
  if (!f) return fail(std::string("cannot open ") + path);
  std::string line;
  int lineno = 0, k = 0;
  while (std::getline(f, line)) {
    lineno++;
    const size_t hash = line.find('#');
    if (hash != std::string::npos) line.erase(hash);
    if (line.find_first_not_of(" \t\r\n") == std::string::npos) continue;
    const std::string where = std::string(path) + ":" + std::to_string(lineno);
    std::istringstream is(line);
    double x, y;
    std::string rest;
    if (!(is >> x >> y) || (is >> rest)) return fail(where + ": expected two numbers (log10 T, log10 Lambda)");
    if (!std::isfinite(x) || !std::isfinite(y)) return fail(where + ": non-finite value");
    if (k > 0 && !(x > logT[k - 1])) return fail(where + ": log10 T must increase strictly");
    if (k >= max_n) return fail(where + ": more than " + std::to_string(max_n) + " knots");
    logT[k] = x;
    logL[k] = y;
    k++;
  }
  if (k < 2) return fail(std::string(path) + ": fewer than 2 knots");
  *n = k;
  return 0;
}

// mp_only_cooling::gen_mpoc_lookup_tables: T[nT], tabs[5][nT] = {rrhp, C_rrh, C_ffhe, C_fbdn, C_cie},
// slopes[5][nT].  Returns 0.
int pion_host_build_cooling_tables(double min_temp, double max_temp, int nT, double *T, double *tabs, double *slopes)
{
  if (nT < 2 || !(min_temp > 0.0) || !(max_temp > min_temp)) return -1;
  static const Tables tb;
  const double dlogT = (std::log10(max_temp) - std::log10(min_temp)) / (nT - 1);
  for (int i = 0; i < nT; i++) T[i] = std::pow(10.0, std::log10(min_temp) + i * dlogT);
  double *rrhp = tabs, *C_rrh = tabs + nT, *C_ffhe = tabs + 2 * nT, *C_fbdn = tabs + 3 * nT, *C_cie = tabs + 4 * nT;
  for (int i = 0; i < nT; i++) {
    rrhp[i] = tb.rrr(T[i]);
    C_rrh[i] = tb.total_cooling(T[i]);
    C_ffhe[i] = 6.72e-28 * std::sqrt(T[i]);
    C_fbdn[i] = 1.20e-22 * std::exp(-33610.0 / T[i] - (2180.0 * 2180.0 / T[i] / T[i])) * std::exp(-T[i] * T[i] / 5.0e10);
    C_cie[i] = tb.cooling_rate(T[i]);
  }
  for (int k = 0; k < 5; k++) {
    const double *t = tabs + k * nT;
    double *s = slopes + k * nT;
    for (int i = 0; i < nT - 1; i++) s[i] = (t[i + 1] - t[i]) / (T[i + 1] - T[i]);
    s[nT - 1] = 0.0;
  }
  return 0;
}

double pion_host_cooling_rate_wss09(double T)
{
  static const Tables tb;
  return tb.cooling_rate(T);
}
double pion_host_hii_rrr(double T)
{
  static const Tables tb;
  return tb.rrr(T);
}
double pion_host_hii_total_cooling(double T)
{
  static const Tables tb;
  return tb.total_cooling(T);
}
}
