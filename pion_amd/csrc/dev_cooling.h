// dev_cooling.h -- per-cell radiative cooling/heating on the device.
//
// mp_only_cooling with EP.cooling = 8 (WSS09_CIE_LINE_HEAT_COOL):
//   Edot            microphysics/mp_only_cooling.cpp:491-521 (bisection in a 200-point
//                   log-T table + linear interpolation of 5 rate tables)
//   TimeUpdateMP    microphysics/mp_only_cooling.cpp:167-218
//   timescales      microphysics/mp_only_cooling.cpp:333-368
//   Cash-Karp RK5   microphysics/integrator.cpp:42-84 (tableau), 285-392 (Step_RK5CK incl. the
//                   first-order shortcut), 401-531 (Stepper_RKCK, BISECTION_STEPPER),
//                   540-602 (Int_Adaptive_RKCK)
// For EP.cooling = 8 no transcendental function is evaluated per cell: the tables are built once on
// the host and handed over through pion_gpu_set_cooling_tables.
//
// The other cooling functions of mp_only_cooling::Edot (mp_only_cooling.cpp:377-415) share everything but Edot:
//   EP.cooling = 4..7  Edot_SD93CIE_cool, _heat_cool, Edot_WSS09CIE_cool, _heat_cool (:424-482) on a total-CIE curve the
//                      caller supplies (pion_gpu_set_cooling_curve), evaluated as
//                      cooling_function_SD93CIE::cooling_rate_SD93CIE (cooling_SD93_cie.cpp:666-704): log10 T, a
//                      natural cubic spline in GSL's cspline representation, exp
//   EP.cooling = 2     Koyama & Inutsuka (2002), CoolingFn::CoolingRate (cooling.cpp:333-336, 373-399)
// They travel in a CoolForm (kernels.h).  TimeUpdateMP, the Cash-Karp driver and timescales below are templates on the
// type that holds the rate's constants (CoolOf<FORM>::type) and call the matching edot overload; the cooling kernels are
// templates on FORM the same way, one instance per form.
#ifndef PION_DEV_COOLING_H
#define PION_DEV_COOLING_H

#include "kernels.h"

namespace pion {

struct Cooling {
  static PDEV double edot(const CoolDev &c, const double rho, const double T)
  {
    const int NT = c.NT;
    // The table interval: the reference bisects (mp_only_cooling.cpp:496-503), which ends on the largest i in
    // [0, NT-2] with T[i] < T (0 if there is none; NaN -> 0).  On the log-spaced grid the same i comes from a
    // single-precision logarithm as a first guess, corrected by stepping along the table itself until exactly that
    // condition holds: the same index for every T, bit-identical results, an eighth of the dependent look-ups.
    int ilo = 0;
    if (c.inv_dlg > 0.0f) {
      float gi = (T > 0.0) ? (__log2f((float)T) - c.lg0) * c.inv_dlg : 0.0f;
      gi = fminf(fmaxf(gi, 0.0f), (float)(NT - 2));
      ilo = (int)gi;
      while (ilo > 0 && !(c.T[ilo] < T)) ilo--;
      while (ilo < NT - 2 && c.T[ilo + 1] < T) ilo++;
    }
    else {
      int ihi = NT - 1, imid = 0;
      do {
        imid = ilo + (int)floor((ihi - ilo) / 2.0);
        if (c.T[imid] < T) ilo = imid;
        else ihi = imid;
      } while (ihi - ilo > 1);
    }
    const int iT = ilo;
    const double dT = T - c.T[iT];
    const double rho2 = rho * rho;
    double rate = 0.0;
    // tab rows: 0 rrhp, 1 C_rrh, 2 C_ffhe, 3 C_fbdn, 4 C_cie
    rate = -(c.tab[3 * NT + iT] + dT * c.slope[3 * NT + iT]) * rho2 * c.inv_Mu2_elec_H;
    rate = dmin(rate, -(c.tab[4 * NT + iT] + dT * c.slope[4 * NT + iT]) * rho2 * c.inv_Mu2);
    rate -= (c.tab[1 * NT + iT] + dT * c.slope[1 * NT + iT]) * rho2 * c.inv_Mu2_elec_H;
    rate -= (c.tab[2 * NT + iT] + dT * c.slope[2 * NT + iT]) * rho2 * c.inv_Mu2_elec_H;
    rate += 8.01e-12 * (c.tab[0 * NT + iT] + dT * c.slope[0 * NT + iT]) * rho2 * c.inv_Mu2_elec_H;
    return rate;
  }
  // The interval of a CIE curve that holds x, x[0] <= x <= x[n-1]: the largest i in [0, n-2] with x[i] <= x, which is
  // what gsl_interp_bsearch ends on (x[i] <= x < x[i+1], the last interval at the upper end).  Uniform knots: a first
  // guess from the spacing, corrected against the knots themselves; else the bisection.
  static PDEV int curve_interval(const CoolForm &f, const double x)
  {
    const int n = f.n;
    int lo = 0;
    if (f.inv_dx > 0.0) {
      const double gi = fmin(fmax((x - f.x[0]) * f.inv_dx, 0.0), (double)(n - 2));
      lo = (int)gi;
      while (lo > 0 && f.x[lo] > x) lo--;
      while (lo < n - 2 && !(f.x[lo + 1] > x)) lo++;
    }
    else {
      int hi = n - 1;
      while (hi > lo + 1) {
        const int i = (hi + lo) / 2;
        if (f.x[i] > x) hi = i;
        else lo = i;
      }
    }
    return lo;
  }
  // cooling_function_SD93CIE::cooling_rate_SD93CIE (cooling_SD93_cie.cpp:666-704) on the caller's curve; the spline
  // polynomial in the expressions and order of the host evaluator (cooling_tables.cpp, Spline::eval = GSL's cspline)
  static PDEV double curve_rate(const CoolForm &f, double T)
  {
    if (T < 0.0 || !isfinite(T)) return HUGE_VAL;
    const int n = f.n;
    double rate;
    T = log10(T);
    if (T > f.x[n - 1]) rate = f.y[n - 1] + f.max_slope * (T - f.x[n - 1]);
    else if (T < f.x[0]) rate = f.y[0] + f.min_slope * (T - f.x[0]);
    else {
      const int i = curve_interval(f, T);
      const double dx = f.x[i + 1] - f.x[i];
      const double dy = f.y[i + 1] - f.y[i];
      const double delx = T - f.x[i];
      const double b_i = (dy / dx) - dx * (f.c[i + 1] + 2.0 * f.c[i]) / 3.0;
      const double d_i = (f.c[i + 1] - f.c[i]) / (3.0 * dx);
      rate = f.y[i] + delx * (b_i + delx * (f.c[i] + delx * d_i));
    }
    return exp(2.3025850929940459 * rate);  // pconst.ln10(), constants.h:44
  }
  // mp_only_cooling::Edot (mp_only_cooling.cpp:377-415), EP.cooling = 4..7: the four combinations of :424-482, each in
  // the reference's statement order.  An infinite or NaN rate (T < 0 after an overshoot) goes back unchanged: the
  // integrator's !isfinite branch halves the step on it.
  static PDEV double edot(const CoolFormT<COOL_FORM_CURVE> &f, const double rho, const double T)
  {
    // (Lambda once, ahead of the uniform switch: the same values as the reference's four expressions, one inlined
    // copy of the curve evaluation per call site instead of four)
    const double L = curve_rate(f, T);
    switch (f.flag) {
      case 4:   // Edot_SD93CIE_cool :429
        return -(rho * rho / f.Mu_elec / f.Mu_ion) * L;
      case 5:   // Edot_SD93CIE_heat_cool :446-447
        return (rho * rho) * (2.733e-21 * exp(-0.782991 * log(T)) / f.Mu_elec / f.Mu - L / f.Mu_elec / f.Mu_ion);
      case 7:   // Edot_WSS09CIE_cool :463
        return 2e-26 * rho / f.Mu - (rho * rho / f.Mu / f.Mu) * L;
      default:  // 6: Edot_WSS09CIE_heat_cool :481
        return (rho * rho) * (2.733e-21 * exp(-0.782991 * log(T)) / f.Mu_elec / f.Mu - L / f.Mu / f.Mu);
    }
  }
  // EP.cooling = 2: -CoolingFn::CoolingRate(T, 0, rho/Mu, 0, 0) with WhichFunction = 2, Koyama & Inutsuka (2002) as
  // corrected by Vazquez-Semadeni et al. (2007) (mp_only_cooling.cpp:387; cooling.cpp:333-336, 373-399; MinTemp = 5 K,
  // cooling.cpp:110)
  static PDEV double edot(const CoolFormT<COOL_FORM_KI02> &f, const double rho, const double T)
  {
    const double nH = rho / f.Mu;
    if (T <= 0.0 || isnan(T) || isinf(T)) return -0.0;
    double rate = 0.0;
    if (T > 5.0) rate += nH * nH * (2.0e-19 * exp(-1.184e5 / (T + 1.0e3)) + 2.8e-28 * sqrt(T) * exp(-92.0 / T));
    rate -= nH * 2.0e-26;
    return -rate;
  }
  // mp_only_cooling::dPdt
  template <class C>
  static PDEV double dPdt(const C &c, const double rho, const double gamma, const double E)
  {
    return edot(c, rho, E * (gamma - 1.0) * c.Mu_tot_over_kB / rho);
  }
  template <class C>
  static PDEV void step_rk5ck(const C &c, const double rho, const double gamma, const double p0,
                              const double dt, double *pf, double *dp)
  {
    const double b21 = 0.2, b31 = 3. / 40., b32 = 9. / 40., b41 = 0.3, b42 = -0.9, b43 = 1.2, b51 = -11. / 54.,
                 b52 = 2.5, b53 = -70. / 27., b54 = 35. / 27., b61 = 1631. / 55296., b62 = 175. / 512.,
                 b63 = 575. / 13824., b64 = 44275. / 110592., b65 = 253. / 4096., c1 = 37. / 378.,
                 c3 = 250. / 621., c4 = 125. / 594., c6 = 512. / 1771.;
    const double dc1 = c1 - 2825. / 27648., dc3 = c3 - 18575. / 48384., dc4 = c4 - 13525. / 55296.,
                 dc5 = -277. / 14336., dc6 = c6 - 0.25;
    double k1, k2, k3, k4, k5, k6, ptemp;
    k1 = dPdt(c, rho, gamma, p0);
    ptemp = 0.0;
    ptemp += fabs(k1) * dt / (p0 + 1.0e-100);
    if (ptemp < 1.e-6) {
      *pf = p0 + k1 * dt;
      *dp = k1 * dt;
      return;
    }
    k1 *= dt;
    ptemp = p0 + b21 * k1;
    k2 = dPdt(c, rho, gamma, ptemp);
    k2 *= dt;
    ptemp = p0 + b31 * k1 + b32 * k2;
    k3 = dPdt(c, rho, gamma, ptemp);
    k3 *= dt;
    ptemp = p0 + b41 * k1 + b42 * k2 + b43 * k3;
    k4 = dPdt(c, rho, gamma, ptemp);
    k4 *= dt;
    ptemp = p0 + b51 * k1 + b52 * k2 + b53 * k3 + b54 * k4;
    k5 = dPdt(c, rho, gamma, ptemp);
    k5 *= dt;
    ptemp = p0 + b61 * k1 + b62 * k2 + b63 * k3 + b64 * k4 + b65 * k5;
    k6 = dPdt(c, rho, gamma, ptemp);
    k6 *= dt;
    *pf = p0 + c1 * k1 + c3 * k3 + c4 * k4 + c6 * k6;
    *dp = dc1 * k1 + dc3 * k3 + dc4 * k4 + dc5 * k5 + dc6 * k6;
  }
  template <class C>
  static PDEV int stepper_rkck(const C &c, const double rho, const double gamma, const double p0,
                               const double t0, const double htry, const double errtol, double *p1,
                               double *hdid, double *hnext)
  {
    int rval = 0;
    double h = htry;
    if (h < 0) return 1;
    double tnew = t0;
    const double eps = 1.e-100;
    double maxerr, err = 0.0, ptemp = 0.0;
    int ct = 0;
    do {
      step_rk5ck(c, rho, gamma, p0, h, &ptemp, &err);
      maxerr = 0;
      if (!isfinite(err) || !isfinite(ptemp) || ptemp < 0.0) {
        maxerr = dmax(maxerr, 1000.0);
      }
      else {
        err /= fabs(ptemp) + eps;
        err = fabs(err / errtol);
        maxerr = dmax(maxerr, err);
      }
      if (maxerr > 1.) h /= 2.0;
      tnew = t0 + h;
      if (tnew == t0) return -2;
      ct++;
    } while (maxerr > 1.0 && ct < 50);
    if (maxerr > 1.0) rval += ct + static_cast<int>(fabs(maxerr));
    *hnext = h * 2.0;
    *hdid = h;
    *p1 = ptemp;
    if (isnan(*p1) || isinf(*p1)) {
      *p1 = -1.e100;
      rval++;
    }
    return rval;
  }
  template <class C>
  static PDEV int int_adaptive_rkck(const C &c, const double rho, const double gamma, const double p0,
                                    const double t0, const double dt, const double errtol, double *pf)
  {
    double t = t0, p1 = p0, p2 = 0.0;
    const double tf = t0 + dt;
    double h = dt, hdid = 0.0, hnext = 0.0;
    int err = 0, ct = 0;
    const int ctmax = 25;
    do {
      err += stepper_rkck(c, rho, gamma, p1, t, h, errtol, &p2, &hdid, &hnext);
      t += hdid;
      h = dmin(hnext, tf - t);
      ct++;
      p1 = p2;
    } while (t < tf && (err == 0) && (ct < ctmax));
    *pf = p1;
    return err;
  }
  // TimeUpdateMP: returns the new pressure (all other primitives are unchanged)
  template <class C>
  static PDEV double time_update(const C &c, const double rho, const double pg_in, const double dt,
                                 const double g, int &errbits)
  {
    if (!isfinite(rho) || !isfinite(pg_in)) errbits |= ERR_COOLING;
    const double Eint0 = pg_in / (g - 1.0);
    double Eint = Eint0;
    int e = int_adaptive_rkck(c, rho, g, Eint, 0.0, dt, 1.0e-2, &Eint);
    if (e) errbits |= ERR_COOLING;
    double pg = Eint * (g - 1);
    double Tf = pg * c.Mu_tot_over_kB / rho;
    if (Tf > c.MaxT_allowed) pg *= c.MaxT_allowed / (Tf);
    else if (Tf < c.MinT_allowed) pg *= c.MinT_allowed / (Tf);
    return pg;
  }
  template <class C>
  static PDEV double timescale(const C &c, const double rho, const double pg, const double gam)
  {
    double Eint = pg / (gam - 1.0);
    double T = pg * c.Mu_tot_over_kB / rho;
    double mintime = 1.0e99;
    if (T >= 1.1 * c.MinT_allowed) {
      double rate = dmax(fabs(edot(c, rho, T)), fabs(edot(c, rho, dmax(c.MinT_allowed, 0.5 * T))));
      mintime = dmin(mintime, Eint / rate);
    }
    return mintime;
  }
};


// The rate's constants as a workgroup of 256 threads uses them, what a thread chases per Edot staged in lds
// (CoolOf<FORM>::lds doubles): an Edot is an interval search of dependent look-ups plus the reads of that interval, a
// Cash-Karp step six of those, and a thread is bound by the latency of that chain -- LDS answers several times sooner
// than the L1 / L2 path.  The tables of EP.cooling = 8 (temperature grid, five rates and their slopes: 11 NT doubles,
// 17.6 KB at NT = 200), the CIE curve of 4..7 (knots, values and spline coefficients: 3 n doubles); KI02 stages nothing.
template <int FORM>
PDEV void stage_cool(const CoolDev &t, const CoolForm &f, double *lds, typename CoolOf<FORM>::type &cool)
{
  if constexpr (FORM == COOL_FORM_TABLE) {
    const int NT = t.NT;
    for (int i = threadIdx.x; i < NT; i += 256) lds[i] = t.T[i];
    for (int i = threadIdx.x; i < 5 * NT; i += 256) {
      lds[NT + i] = t.tab[i];
      lds[6 * NT + i] = t.slope[i];
    }
    __syncthreads();
    cool = t;
    cool.T = lds;
    cool.tab = lds + NT;
    cool.slope = lds + 6 * NT;
  }
  else {
    static_cast<CoolForm &>(cool) = f;
    if constexpr (FORM == COOL_FORM_CURVE) {
      const int n = f.n;
      for (int i = threadIdx.x; i < n; i += blockDim.x) {
        lds[i] = f.x[i];
        lds[n + i] = f.y[i];
        lds[2 * n + i] = f.c[i];
      }
      __syncthreads();
      cool.x = lds;
      cool.y = lds + n;
      cool.c = lds + 2 * n;
    }
  }
}

}  // namespace pion
#endif
