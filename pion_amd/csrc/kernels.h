// kernels.h -- launch interface between the C-ABI layer (pion_gpu.hip, pion_step.hip, pion_bc.hip) and the
// floating-point kernels: kernels_fp.hip (stage, cooling source, flux and cell test, one object per equation set),
// kernels_prepass.hip and kernels_dt.hip.  Each is compiled twice, once per floating-point mode, into namespaces
// pion::fp_strict (-ffp-contract=off: bit-parity with the reference's x86-64 -O3 build) and pion::fp_fast (FMA
// contraction allowed); pion_gpu_config::strict_fp selects at run time.
#ifndef PION_KERNELS_H
#define PION_KERNELS_H

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "dev_riemann.h"
#include "grid_desc.h"
#include "rows_tiling.h"
#include "hll_screen.h"

namespace pion {

#define PION_MAX_NTR 2
#define PION_COOL_NT_MAX 256

struct CoolDev {
  int NT;
  const double *T;       // [NT]
  const double *tab;     // [5][NT]  rrhp, C_rrh, C_ffhe, C_fbdn, C_cie
  const double *slope;   // [5][NT]
  double inv_Mu2, inv_Mu2_elec_H, Mu_tot_over_kB;
  double MinT_allowed, MaxT_allowed;
  // log-spaced temperature grid (what gen_mpoc_lookup_tables builds): first guess of the table interval,
  // (log2 T - lg0) * inv_dlg, corrected against the table itself; inv_dlg = 0: not log-spaced, bisect
  float lg0, inv_dlg;
};

// The cooling functions of mp_only_cooling other than the tabulated one (EP.cooling = 2, 4..7).  CoolDev and StageArgs
// are by-value arguments of the stage kernels, whose code is pinned, so this travels as an argument of its own, to every
// cooling kernel; the instances of the tabulated rate (COOL_FORM_TABLE: EP.cooling = 8, constants in CoolDev) ignore it.
enum { COOL_FORM_TABLE = 0, COOL_FORM_CURVE = 1, COOL_FORM_KI02 = 2 };
struct CoolForm {
  int flag;              // EP.cooling: 2 (KI02), 4..7 (a uniform run-time switch within COOL_FORM_CURVE), else the tables
  int n;                 // knots of the CIE curve (0 for KI02)
  const double *x;       // [n] log10 T, strictly increasing
  const double *y;       // [n] log10 Lambda
  const double *c;       // [n] natural-spline second-derivative coefficients (GSL's cspline representation)
  double min_slope, max_slope;   // linear extrapolation in log-log space below / above the knots
  double inv_dx;         // uniformly spaced knots: 1 / spacing (first guess of the interval), else 0: bisect
  double Mu, Mu_elec, Mu_ion;    // mean masses per H nucleus / electron / ion (mp_only_cooling.cpp:81-85)
  double Mu_tot_over_kB, MinT_allowed, MaxT_allowed;   // as CoolDev's
};
template <int FORM>
struct CoolFormT : CoolForm {};
// the kernel instance an EP.cooling runs on (the launchers' dispatch)
static inline int cool_form_of(const int flag)
{
  return (flag == 2) ? COOL_FORM_KI02 : (flag >= 4 && flag <= 7) ? COOL_FORM_CURVE : COOL_FORM_TABLE;
}
// per form: the type that holds the rate's constants (dev_cooling.h: Cooling::edot is overloaded on it) and the doubles
// a workgroup stages in LDS -- temperature grid, five rates and their slopes; knots, values and coefficients; nothing
template <int FORM>
struct CoolOf {
  typedef CoolFormT<FORM> type;
  static constexpr int lds = (FORM == COOL_FORM_CURVE) ? 3 * PION_COOL_NT_MAX : 1;
};
template <>
struct CoolOf<COOL_FORM_TABLE> {
  typedef CoolDev type;
  static constexpr int lds = 11 * PION_COOL_NT_MAX;
};

struct StageArgs {
  GridDesc g;
  const double *S;    // stencil state ("Ph")      [nvar][ncell]
  const double *Pc;   // start-of-step state ("P") [nvar][ncell]
  double *out;        // destination                [nvar][ncell]
  const uint8_t *flags;
  const uint8_t *hllflag;   // HLLD->HLL switch per cell (may be null)
  const double *eta;        // H-correction [ndim][ncell] (may be null)
  int *errword;
  FluxCtx fc;
  int eqntype, ntracer, solver;
  int space_ooa;
  int cooling;        // EP.cooling
  double dt;          // stage dt (= FV_dt)
  double glm_damp;    // exp(-FV_dt*chyp*cr), evaluated on the host
  double max_temp;    // EP.MaxTemperature
  int use_march;      // != 0: k_stage_rows2 (3-D, nbc >= 2: production), 0: k_stage (cell per thread; 1-D / 2-D, cross-check)
  int xwrap;          // k_stage_rows2: x faces periodic -> also write the x ghost images of the rows it updates
  int zslope_lds;     // k_stage_rows2: carry the z slope in LDS (else rebuild it from plane k-1)
  double *dE;         // k_stage_rows2: cooling source PtoU(p_new)[ERG]-PtoU(P)[ERG] per cell from k_cooling_dE (or null)
  int zchunk;         // planes per wavefront in the marching kernels
  // k_stage_rows2, first strip [kz0,kz1): nzb > 0 = uneven chunks (zchunk_bounds, rows_tiling.h: chunks of `zcmax` planes,
  // then halving down to 4 -- long chunks first, short ones last: the launch's last wavefronts are short, so its
  // tail is), nzb of them
  int nzb, zcmax;
  int rows;           // y-rows per wavefront in k_stage_rows2
  int rows_auto;      // 2-D: the launcher may pick the rows per wavefront for the instance it launches (its occupancy)
  int ncu;            // compute units of the device (for that choice)
  int kz0, kz1;       // on-grid z planes [kz0,kz1) this launch updates (k_stage_rows2; k_stage: whole grid)
  int kz2, kz3;       // and a second strip [kz2,kz3) (empty when kz3 <= kz2): the two z-boundary strips
  unsigned long long *dtres;  // k_stage_rows2, full step: min t_dyn / t_mp bits of the new state (or null)
  double cfl;
  int dt_mp;          // also reduce the cooling time (EP.MP_timestep_limit)
  int plain_cells;    // every on-grid cell is an ordinary domain cell (no stellar-wind cells): flags need not be read
  CoolDev cool;
  // k_stage_rows2, 3-D MHD / GLM with HLLD: pressure-range summary per block of cells (hll_screen.h) for the next
  // stage's prepass, keys of the maxima [hsum_n] then of the minima [hsum_n], cleared by the caller (or null)
  unsigned long long *hsum;
  long hsum_n;
  int hsum_nbx, hsum_nby, hsum_nbz;
};

struct PrepassArgs {
  GridDesc g;
  const double *S;
  uint8_t *hllflag;
  double *divv, *gradp;   // optional debug outputs (null in production)
  double *eta;            // [ndim][ncell]
  int eqntype, nvar, space_ooa;
  double gamma;
  long c0, c1;            // cell range [c0,c1) (whole planes) this launch covers
  long c2, c3;            // k_prepass_hlld: a second range [c2,c3) in the same launch (empty when c3 <= c2)
  // screened prepass (hll_screen.h; whole-array launches only): the summary the last stage kernel left of S (or null),
  // its geometry, the list of active blocks and its counter (both written here)
  const unsigned long long *hsum;
  ScrGeom scr;
  int *scr_list, *scr_count;
};

struct DtArgs {
  GridDesc g;
  const double *P;
  const double *Ph;
  const uint8_t *flags;
  unsigned long long *result;  // [0]=t_dyn bits, [1]=t_mp bits (min over positive doubles)
  int *errword;
  int eqntype, nvar;
  double gamma, cfl;
  int do_mp;
  CoolDev cool;
};

struct FluxTestArgs {
  int n, axis, eqntype, ntracer, solver;
  const double *Pl, *Pr, *aux;
  double *F, *Pstar;
  int *errword;
  FluxCtx fc;
};

// cell-update test seam (k_cell_test): n independent cells through the stage kernels' cell_update and cell_dt
struct CellTestArgs {
  int n, eqntype, ntracer;
  const double *Pin, *dU;   // [n][nvar]; dU null: no update
  double *Pout, *dt;        // [n][nvar], [n]; dt null: no time step
  StageArgs st;             // as a stage launch fills it: fc, glm_damp, max_temp, g, cfl, errword
};

struct CoolTestArgs {
  int n, nvar;
  double dt, gamma;
  const double *Pin;
  double *Pout;
  const double *rho, *T;
  double *edot;
  int *errword;
  CoolDev cool;
};

// a launcher kernels_fp.hip defines once per equation set (-DPION_EQSEL), and its dispatcher on a.eqntype; after ARGS:
// the type of one more parameter between the arguments and the stream, if the launcher has one
#define PION_PER_EQN(FN, ARGS, ...)                                            \
  int FN##_hd(const ARGS &a, __VA_OPT__(__VA_ARGS__ x, ) hipStream_t s);       \
  int FN##_mhd(const ARGS &a, __VA_OPT__(__VA_ARGS__ x, ) hipStream_t s);      \
  int FN##_glm(const ARGS &a, __VA_OPT__(__VA_ARGS__ x, ) hipStream_t s);      \
  inline int FN(const ARGS &a, __VA_OPT__(__VA_ARGS__ x, ) hipStream_t s)      \
  {                                                                            \
    if (a.eqntype == EQEUL) return FN##_hd(a, __VA_OPT__(x, ) s);              \
    if (a.eqntype == EQMHD) return FN##_mhd(a, __VA_OPT__(x, ) s);             \
    if (a.eqntype == EQGLM) return FN##_glm(a, __VA_OPT__(x, ) s);             \
    return -1;                                                                 \
  }

// the cooling launchers pick the instance of f.flag (cool_form_of); launch_cool: what = 0 TimeUpdateMP, 1 Edot,
// 2 timescales, 3 the CIE curve itself
#define PION_DECLARE_FP(NS)                                        \
  namespace NS {                                                   \
  PION_PER_EQN(launch_stage, StageArgs)                            \
  PION_PER_EQN(launch_stage_dE, StageArgs)                         \
  PION_PER_EQN(launch_cooling_dE, StageArgs, const CoolForm &)     \
  PION_PER_EQN(launch_flux_test, FluxTestArgs)                     \
  PION_PER_EQN(launch_cell_test, CellTestArgs)                     \
  int launch_prepass(const PrepassArgs &a, hipStream_t s);         \
  int launch_dt(const DtArgs &a, hipStream_t s);                   \
  int launch_dt_mp(const DtArgs &a, const CoolForm &f, hipStream_t s);   \
  int launch_cool(const CoolTestArgs &a, const CoolForm &f, int what, hipStream_t s);   \
  }

PION_DECLARE_FP(fp_strict)
PION_DECLARE_FP(fp_fast)

}  // namespace pion
#endif
