// kernels_dt.hip -- the time-step reductions and the cooling test seams; nothing here depends on the equation set.
//
//   k_dt       CellTimeStep + cooling-time reduction (calc_timestep.cpp:271-507).
//   k_dt_mp    the cooling time alone, the rate's constants in LDS.
//   k_cool     mp_only_cooling on n independent cells (test seam).
//
// Compiled twice (Makefile): -DPION_FPNS=fp_strict -ffp-contract=off and -DPION_FPNS=fp_fast -ffp-contract=fast.
#include "dev_cooling.h"
#include "kernels.h"

#ifndef PION_FPNS
#error "PION_FPNS must be defined (fp_strict or fp_fast)"
#endif

namespace pion {
namespace PION_FPNS {

#include "dev_sweep.h"

// ---------------------------------------------------------------------------
// time-step reduction
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_dt(const DtArgs a)
{
  const long nc = a.g.ncell;
  const long non = (long)a.g.ng[0] * a.g.ng[1] * a.g.ng[2];
  double tdyn = 1.e100, tmp = 1.0e99;
  int err = 0;
  const bool mhd = (a.eqntype != EQEUL);
  const double g = a.gamma;
  for (long k = (long)blockIdx.x * blockDim.x + threadIdx.x; k < non; k += (long)gridDim.x * blockDim.x) {
    const long c = ongrid_cell(a.g, k);
    const uint8_t fl = a.flags[c];
    if ((fl & 8 /*TIMESTEP*/) && !(fl & 2 /*ISBD*/)) {
      // CellTimeStep: solver_eqn_hydro_adi.cpp:460-502 / solver_eqn_mhd_adi.cpp:516-582
      double p[8];
      const int nvs = mhd ? 8 : 5;
      for (int v = 0; v < 8; v++) p[v] = (v < nvs) ? a.P[v * nc + c] : 0.0;
      // (the function the stage kernel's fused reduction calls: a restart, which comes through here, continues bit
      // for bit)
      const double t = mhd ? cell_dt<EQMHD>(p, a.g.ndim, g, a.g.dx, a.cfl) : cell_dt<EQEUL>(p, a.g.ndim, g, a.g.dx, a.cfl);
      if (!(t > 0.0)) err |= ERR_BAD_DT;
      tdyn = (t < tdyn) ? t : tdyn;
    }
    if (a.do_mp && !(fl & 2) && (fl & 16)) {
      const double t = Cooling::timescale(a.cool, a.Ph[0 * nc + c], a.Ph[1 * nc + c], g);
      tmp = (t < tmp) ? t : tmp;
    }
  }
  tdyn = wave_min64(tdyn);
  tmp = wave_min64(tmp);
  if ((threadIdx.x & 63) == 0) {
    // positive doubles order like their bit patterns
    atomicMin(&a.result[0], (unsigned long long)__double_as_longlong(tdyn));
    atomicMin(&a.result[1], (unsigned long long)__double_as_longlong(tmp));
  }
  if (err) atomicOr(a.errword, err);
}

// The cooling time alone (calc_microphysics_dt -> get_mp_timescales_no_radiation, calc_timestep.cpp:405-507;
// mp_only_cooling::timescales, mp_only_cooling.cpp:333-368), the rate's constants in LDS as in k_cooling_dE: a time scale
// is two Edot evaluations = two bisections of eight dependent look-ups each, which through global memory cost the fused
// reduction of the stage kernel a third of its run time (Wind3D 256^3, second-order instance: 1.58 ms with it, 1.03
// without; this kernel: see DESIGN.md s4.1).  Min over cells with !isbd && isleaf into result[1].  One instance per
// form of the rate; that of the tables ignores f.  (The full reduction of EP.cooling = 2, 4..7 is k_dt with do_mp = 0
// followed by this kernel: pion_gpu_calc_dt_device.)
template <int FORM>
__global__ __launch_bounds__(256) void k_dt_mp(const DtArgs a, const CoolForm f)
{
  __shared__ double clds[CoolOf<FORM>::lds];
  typename CoolOf<FORM>::type cool;
  stage_cool<FORM>(a.cool, f, clds, cool);
  const long nc = a.g.ncell;
  const long non = (long)a.g.ng[0] * a.g.ng[1] * a.g.ng[2];
  double tmp = 1.0e99;
  for (long k = (long)blockIdx.x * blockDim.x + threadIdx.x; k < non; k += (long)gridDim.x * blockDim.x) {
    const long c = ongrid_cell(a.g, k);
    const uint8_t fl = a.flags[c];
    if (!(fl & 2) && (fl & 16)) {
      const double t = Cooling::timescale(cool, a.Ph[0 * nc + c], a.Ph[1 * nc + c], a.gamma);
      tmp = (t < tmp) ? t : tmp;
    }
  }
  tmp = wave_min64(tmp);
  if ((threadIdx.x & 63) == 0) atomicMin(&a.result[1], (unsigned long long)__double_as_longlong(tmp));
}
// grid-stride, eight blocks per CU: the rate's constants are staged once per block
static inline dim3 dt_blocks(const DtArgs &a)
{
  const long non = (long)a.g.ng[0] * a.g.ng[1] * a.g.ng[2];
  const long nb = (non + 255) / 256;
  return dim3((unsigned)((nb > 2048) ? 2048 : nb));
}
int launch_dt_mp(const DtArgs &a, const CoolForm &f, hipStream_t s)
{
  const int form = cool_form_of(f.flag);
  if (form == COOL_FORM_KI02) hipLaunchKernelGGL(k_dt_mp<COOL_FORM_KI02>, dt_blocks(a), dim3(256), 0, s, a, f);
  else if (form == COOL_FORM_CURVE) hipLaunchKernelGGL(k_dt_mp<COOL_FORM_CURVE>, dt_blocks(a), dim3(256), 0, s, a, f);
  else hipLaunchKernelGGL(k_dt_mp<COOL_FORM_TABLE>, dt_blocks(a), dim3(256), 0, s, a, f);
  return (int)hipGetLastError();
}
int launch_dt(const DtArgs &a, hipStream_t s)
{
  hipLaunchKernelGGL(k_dt, dt_blocks(a), dim3(256), 0, s, a);
  return (int)hipGetLastError();
}

// ---------------------------------------------------------------------------
// cooling test seam: mp_only_cooling on n independent cells, the rate's constants in LDS as the production kernels hold
// them.  what: 0 TimeUpdateMP, 1 Edot, 2 timescales (cooling time only: edot[i] = t_cool), 3 the CIE curve itself,
// edot[i] = Lambda(T[i]) through the kernels' own curve_rate.
// ---------------------------------------------------------------------------
template <int FORM>
__global__ __launch_bounds__(256) void k_cool(const CoolTestArgs a, const CoolForm f, const int what)
{
  __shared__ double clds[CoolOf<FORM>::lds];
  typename CoolOf<FORM>::type cool;
  stage_cool<FORM>(a.cool, f, clds, cool);
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= a.n) return;
  if (what == 0) {
    int err = 0;
    const double *p = a.Pin + (long)i * a.nvar;
    double *o = a.Pout + (long)i * a.nvar;
    for (int v = 0; v < a.nvar; v++) o[v] = p[v];
    o[1] = Cooling::time_update(cool, p[0], p[1], a.dt, a.gamma, err);
    if (err) atomicOr(a.errword, err);
  }
  else if (what == 1) a.edot[i] = Cooling::edot(cool, a.rho[i], a.T[i]);
  else if (what == 2) {
    const double *p = a.Pin + (long)i * a.nvar;
    a.edot[i] = Cooling::timescale(cool, p[0], p[1], a.gamma);
  }
  else {
    if constexpr (FORM == COOL_FORM_CURVE) a.edot[i] = Cooling::curve_rate(cool, a.T[i]);
    else a.edot[i] = 0.0;
  }
}
int launch_cool(const CoolTestArgs &a, const CoolForm &f, int what, hipStream_t s)
{
  const int form = cool_form_of(f.flag);
  if (what < 0 || what > 3 || (what == 3 && form != COOL_FORM_CURVE)) return -1;
  const dim3 nb((a.n + 255) / 256);
  if (form == COOL_FORM_KI02) hipLaunchKernelGGL(k_cool<COOL_FORM_KI02>, nb, dim3(256), 0, s, a, f, what);
  else if (form == COOL_FORM_CURVE) hipLaunchKernelGGL(k_cool<COOL_FORM_CURVE>, nb, dim3(256), 0, s, a, f, what);
  else hipLaunchKernelGGL(k_cool<COOL_FORM_TABLE>, nb, dim3(256), 0, s, a, f, what);
  return (int)hipGetLastError();
}

}  // namespace PION_FPNS
}  // namespace pion
