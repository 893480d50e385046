// kernels_fp.hip -- the per-equation kernels of the flux-update path for gfx950.
//
// Compiled twice (Makefile): -DPION_FPNS=fp_strict -ffp-contract=off and -DPION_FPNS=fp_fast -ffp-contract=fast,
// and once per equation set: -DPION_EQSEL=1 (Euler), 2 (ideal MHD) or 3 (GLM-MHD).  What does not depend on the
// equation set is in kernels_prepass.hip and kernels_dt.hip; the helpers all three share are in dev_sweep.h.
//
//   k_stage    one fused stage of the time integrator for every on-grid cell:
//              cooling source (time_integrator.cpp:438-489), the directionally-unsplit sweeps
//              (set_dynamics_dU/dynamics_dU_column, time_integrator.cpp:553-873) and the
//              state update (grid_update_state_vector + CellAdvanceTime, :881-958).
//              The reference accumulates cell->dU in memory sweep by sweep; here one
//              thread owns one cell, rebuilds the two interface fluxes of each axis from
//              a 5-point stencil per axis, and applies the contributions to its dU in
//              registers in exactly the reference's order (x,y,z; per axis: Powell/GLM term
//              of the lower interface, of the upper interface, then the flux difference).
//              HBM sees: read the stencil state (cached re-reads), read the start-of-step
//              state, write the new state.
//   k_stage_rows2  the production form of the same stage (stage_rows2.h), k_cooling_dE its cooling source,
//   k_flux_test    the interface-flux test seam, k_cell_test the cell-update one.
#include "dev_cooling.h"
#include "kernels.h"

#ifndef PION_FPNS
#error "PION_FPNS must be defined (fp_strict or fp_fast)"
#endif
#if !defined(PION_EQSEL) || PION_EQSEL < 1 || PION_EQSEL > 3
#error "PION_EQSEL must be 1 (Euler), 2 (ideal MHD) or 3 (GLM-MHD)"
#endif

namespace pion {
namespace PION_FPNS {

#include "dev_sweep.h"

// ---------------------------------------------------------------------------
// select_Hcorr_eta (solver_eqn_base.cpp:608-678) for the interface (cl | cl+st) along ax.
// The "negative direction" look-ups step back along the SWEEP axis (negdir = 2*axis, :661),
// as in the reference.
// ---------------------------------------------------------------------------
PDEV double select_hcorr_eta(const StageArgs &a, const int ax, const long cl, const long st)
{
  const long nc = a.g.ncell;
  const long cr = cl + st;
  const int nd = a.g.ndim;
  double eta = a.eta[ax * nc + cl];
  if (nd == 1) return eta;
  int perp = (ax + 1) % nd;
  eta = dmax(eta, a.eta[perp * nc + cl]);
  eta = dmax(eta, a.eta[perp * nc + cr]);
  if (nd > 2) {
    perp = (ax + 2) % nd;
    eta = dmax(eta, a.eta[perp * nc + cl]);
    eta = dmax(eta, a.eta[perp * nc + cr]);
  }
  for (int idim = 1; idim < nd; idim++) {
    perp = (ax + idim) % nd;
    // cl-st and cr-st exist for every interface an on-grid cell needs (nbc >= 2)
    eta = dmax(eta, a.eta[perp * nc + (cl - st)]);
    eta = dmax(eta, a.eta[perp * nc + (cr - st)]);
  }
  return eta;
}

// ---------------------------------------------------------------------------
// the fused stage kernel
// ---------------------------------------------------------------------------
template <int EQ, int NTR, int SOLVER>
__global__ __launch_bounds__(256) void k_stage(const StageArgs a)
{
#include "stage_cell.h"
}
// EP.cooling = 2, 4..7 on the cell-per-thread path: the same stage with the cooling source read from a.dE
#define PION_STAGE_DE
template <int EQ, int NTR, int SOLVER>
__global__ __launch_bounds__(256) void k_stage_dE(const StageArgs a)
{
#include "stage_cell.h"
}
#undef PION_STAGE_DE

// ---------------------------------------------------------------------------
// interface-flux test seam: FV_solver_base::InterCellFlux on n independent interfaces
// ---------------------------------------------------------------------------
template <int EQ, int NTR, int SOLVER>
__global__ __launch_bounds__(256) void k_flux_test(const FluxTestArgs a)
{
  typedef Eqn<EQ, NTR> E;
  typedef Flux<EQ, NTR, SOLVER> FX;
  constexpr int NV = E::NV;
  constexpr bool MHD = E::MHD;
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= a.n) return;
  double l[NV], r[NV], ls[NV], rs[NV], f[NV], ps[NV], fl[NV], pl[NV];
#pragma unroll
  for (int v = 0; v < NV; v++) {
    l[v] = a.Pl[(long)i * NV + v];
    r[v] = a.Pr[(long)i * NV + v];
  }
  to_sweep<NV, MHD>(a.axis, l, ls);
  to_sweep<NV, MHD>(a.axis, r, rs);
  int err = 0;
  FX::intercell_flux(ls, rs, f, ps, a.fc, a.aux[4 * i + 0], a.aux[4 * i + 1] != 0.0, err);
  from_sweep<NV, MHD>(a.axis, f, fl);
  from_sweep<NV, MHD>(a.axis, ps, pl);
#pragma unroll
  for (int v = 0; v < NV; v++) {
    a.F[(long)i * NV + v] = fl[v];
    a.Pstar[(long)i * NV + v] = pl[v];
  }
  if (err) atomicOr(a.errword, err);
}

#include "stage_helpers.h"
#include "stage_rows2.h"

// ---------------------------------------------------------------------------
// cell-update test seam: CellAdvanceTime + the temperature ceiling (the stage kernels' cell_update) and
// CellTimeStep (cell_dt) on n independent cells
// ---------------------------------------------------------------------------
template <int EQ, int NTR>
__global__ __launch_bounds__(256) void k_cell_test(const CellTestArgs a)
{
  constexpr int NV = Eqn<EQ, NTR>::NV;
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= a.n) return;
  double P0[NV];
#pragma unroll
  for (int v = 0; v < NV; v++) P0[v] = a.Pin[(long)i * NV + v];
  if (a.dU) {
    double dU[NV], Pf[NV];
#pragma unroll
    for (int v = 0; v < NV; v++) dU[v] = a.dU[(long)i * NV + v];
    int err = 0;
    cell_update<EQ, NTR>(a.st, P0, dU, err, Pf);
#pragma unroll
    for (int v = 0; v < NV; v++) a.Pout[(long)i * NV + v] = Pf[v];
    if (err) atomicOr(a.st.errword, err);
  }
  if (a.dt) a.dt[i] = cell_dt<EQ>(P0, a.st.g.ndim, a.st.fc.gamma, a.st.g.dx, a.st.cfl);
}

// ---------------------------------------------------------------------------
// cooling source term, one thread per on-grid cell of the planes a stage launch updates:
// calc_noRT_microphysics_dU (time_integrator.cpp:438-489) -> mp_only_cooling::TimeUpdateMP.  Only the
// energy component of dU changes, so the kernel leaves dE = PtoU(p_new)[ERG] - PtoU(P)[ERG] (the same two
// PtoU evaluations the reference subtracts) for k_stage_rows2 to start its dU from.  The adaptive
// Cash-Karp loop diverges from cell to cell: here it runs at full occupancy, outside the stage kernel.
// The rate's constants reach LDS first (stage_cool, dev_cooling.h); one instance per form of the rate, that of the tables
// (EP.cooling = 8) ignores f.
// ---------------------------------------------------------------------------
template <int EQ, int NTR, int FORM>
__global__ __launch_bounds__(256) void k_cooling_dE(const StageArgs a, const CoolForm f)
{
  typedef Eqn<EQ, NTR> E;
  constexpr int NV = E::NV;
  const unsigned gx = (a.g.ng[0] + 63) / 64, gy = (a.g.ng[1] + 3) / 4;
  const unsigned np1 = (unsigned)(a.kz1 - a.kz0), np2 = (a.kz3 > a.kz2) ? (unsigned)(a.kz3 - a.kz2) : 0u;
  const unsigned ntile = gx * gy * (np1 + np2);
  __shared__ double clds[CoolOf<FORM>::lds];
  typename CoolOf<FORM>::type cool;
  stage_cool<FORM>(a.cool, f, clds, cool);
  const unsigned t = (unsigned)xcd_tile(blockIdx.x, ntile);
  if (t >= ntile) return;
  const int ix = (int)((t % gx) * 64 + (threadIdx.x & 63));
  const int iy = (int)(((t / gx) % gy) * 4 + (threadIdx.x >> 6));
  const unsigned pz = t / (gx * gy);
  const int iz = (pz < np1) ? a.kz0 + (int)pz : a.kz2 + (int)(pz - np1);
  if (ix >= a.g.ng[0] || iy >= a.g.ng[1]) return;
  const long nc = a.g.ncell;
  // (a 2-D launch of the rows kernel: a.g.ng[1] rows per range and the "plane" of a strip is the first row of its
  // range, rows_tiling.h "2-D row ranges")
  const long c = (a.g.ndim == 2) ? (long)(ix + a.g.nbc[0]) + a.g.sy * (iy + iz + a.g.nbc[1])
                                 : (long)(ix + a.g.nbc[0]) + a.g.sy * (iy + a.g.nbc[1]) + a.g.sz * (iz + a.g.nbc[2]);
  double dE = 0.0;
  if (a.flags[c] & 4 /*ISDOMAIN*/) {
    const double g = a.fc.gamma;
    int err = 0;
#ifdef PION_FAST_MATH
    // fast build: only the pressure changes, so PtoU(p_new)[ERG] - PtoU(P)[ERG] = (p_new - p) / (gamma - 1) -- the
    // kinetic (and magnetic) energy the reference adds to both terms and subtracts again is not read at all (two
    // variables instead of NV per cell; the difference to the reference form is the rounding of that cancellation)
    const double ro = a.Pc[qRO * nc + c], pg = a.Pc[qPG * nc + c];
    const double pnew = Cooling::time_update(cool, ro, pg, a.dt, g, err);
    dE = (pnew - pg) / (g - 1.0);
#else
    double P0[NV], pn[NV], ui[NV], uf[NV];
#pragma unroll
    for (int v = 0; v < NV; v++) pn[v] = P0[v] = a.Pc[v * nc + c];
    pn[qPG] = Cooling::time_update(cool, P0[qRO], P0[qPG], a.dt, g, err);
    E::PtoU(P0, ui, g);
    E::PtoU(pn, uf, g);
    dE = uf[uERG] - ui[uERG];
#endif
    if (err) atomicOr(a.errword, err);
  }
  a.dE[c] = dE;
}
template <int EQ, int NTR>
static int cooling_go(const StageArgs &a, const CoolForm &f, hipStream_t s)
{
  const unsigned gx = (a.g.ng[0] + 63) / 64, gy = (a.g.ng[1] + 3) / 4;
  const unsigned np = (unsigned)(a.kz1 - a.kz0) + ((a.kz3 > a.kz2) ? (unsigned)(a.kz3 - a.kz2) : 0u);
  const unsigned ntile = gx * gy * np;
  const dim3 nb(((ntile + 7) / 8) * 8);
  const int form = cool_form_of(f.flag);
  if (form == COOL_FORM_KI02) hipLaunchKernelGGL((k_cooling_dE<EQ, NTR, COOL_FORM_KI02>), nb, dim3(256), 0, s, a, f);
  else if (form == COOL_FORM_CURVE) hipLaunchKernelGGL((k_cooling_dE<EQ, NTR, COOL_FORM_CURVE>), nb, dim3(256), 0, s, a, f);
  else hipLaunchKernelGGL((k_cooling_dE<EQ, NTR, COOL_FORM_TABLE>), nb, dim3(256), 0, s, a, f);
  return (int)hipGetLastError();
}

template <int EQ, int NTR, int SOLVER>
static int stage_go(const StageArgs &a, hipStream_t s)
{
  if (a.use_march != 0 && ((a.g.ndim == 3 && a.g.nbc[2] >= 2) || (a.g.ndim == 2 && a.g.cyl != 2 && a.g.nbc[1] >= 2)))
    return stage_rows2_go<EQ, NTR, SOLVER>(a, s);
  const int nbx = (a.g.ng[0] + 63) / 64, nby = (a.g.ng[1] + 3) / 4;
  const long ntiles = (long)nbx * nby * a.g.ng[2];
  const long nblocks = ((ntiles + 7) / 8) * 8;
  hipLaunchKernelGGL((k_stage<EQ, NTR, SOLVER>), dim3((unsigned)nblocks), dim3(256), 0, s, a);
  return (int)hipGetLastError();
}
// the cell-per-thread kernel with the cooling source read from a.dE (whole grid)
template <int EQ, int NTR, int SOLVER>
static int stage_dE_go(const StageArgs &a, hipStream_t s)
{
  const int nbx = (a.g.ng[0] + 63) / 64, nby = (a.g.ng[1] + 3) / 4;
  const long ntiles = (long)nbx * nby * a.g.ng[2];
  const long nblocks = ((ntiles + 7) / 8) * 8;
  hipLaunchKernelGGL((k_stage_dE<EQ, NTR, SOLVER>), dim3((unsigned)nblocks), dim3(256), 0, s, a);
  return (int)hipGetLastError();
}
template <int EQ, int NTR, int SOLVER>
static int flux_go(const FluxTestArgs &a, hipStream_t s)
{
  hipLaunchKernelGGL((k_flux_test<EQ, NTR, SOLVER>), dim3((a.n + 255) / 256), dim3(256), 0, s, a);
  return (int)hipGetLastError();
}

template <int EQ, int NTR>
static int cell_go(const CellTestArgs &a, hipStream_t s)
{
  hipLaunchKernelGGL((k_cell_test<EQ, NTR>), dim3((a.n + 255) / 256), dim3(256), 0, s, a);
  return (int)hipGetLastError();
}

#define PION_SOLVER_CASES_HD(FN, EQ, NTR, A, S)          \
  switch (A.solver) {                                    \
    case 0: return FN<EQ, NTR, 0>(A, S);                 \
    case 1: return FN<EQ, NTR, 1>(A, S);                 \
    case 2: return FN<EQ, NTR, 2>(A, S);                 \
    case 3: return FN<EQ, NTR, 3>(A, S);                 \
    case 4: return FN<EQ, NTR, 4>(A, S);                 \
    case 5: return FN<EQ, NTR, 5>(A, S);                 \
    case 6: return FN<EQ, NTR, 6>(A, S);                 \
    case 8: return FN<EQ, NTR, 8>(A, S);                 \
    default: return -1;                                  \
  }
#define PION_SOLVER_CASES_MHD(FN, EQ, NTR, A, S)         \
  switch (A.solver) {                                    \
    case 0: return FN<EQ, NTR, 0>(A, S);                 \
    case 1: return FN<EQ, NTR, 1>(A, S);                 \
    case 4: return FN<EQ, NTR, 4>(A, S);                 \
    case 7: return FN<EQ, NTR, 7>(A, S);                 \
    case 8: return FN<EQ, NTR, 8>(A, S);                 \
    default: return -1;                                  \
  }

#if PION_EQSEL == 1
#define PION_EQ EQEUL
#define PION_CASES PION_SOLVER_CASES_HD
#define PION_SUFFIX hd
#elif PION_EQSEL == 2
#define PION_EQ EQMHD
#define PION_CASES PION_SOLVER_CASES_MHD
#define PION_SUFFIX mhd
#else
#define PION_EQ EQGLM
#define PION_CASES PION_SOLVER_CASES_MHD
#define PION_SUFFIX glm
#endif
#define PION_CAT2(a, b) a##b
#define PION_CAT(a, b) PION_CAT2(a, b)

#ifdef PION_PROBE
// register / ISA probe builds (profiles/tools/probe_regs.sh): instantiate the production instances only
int PION_CAT(launch_stage_, PION_SUFFIX)(const StageArgs &a, hipStream_t s)
{
  return stage_rows2_go<PION_EQ, 0, (PION_EQSEL == 1 ? 4 : 7)>(a, s);
}
#else
int PION_CAT(launch_stage_, PION_SUFFIX)(const StageArgs &a, hipStream_t s)
{
  switch (a.ntracer) {
    case 0: PION_CASES(stage_go, PION_EQ, 0, a, s)
    case 1: PION_CASES(stage_go, PION_EQ, 1, a, s)
    case 2: PION_CASES(stage_go, PION_EQ, 2, a, s)
    default: return -1;
  }
}
int PION_CAT(launch_cooling_dE_, PION_SUFFIX)(const StageArgs &a, const CoolForm &f, hipStream_t s)
{
  switch (a.ntracer) {
    case 0: return cooling_go<PION_EQ, 0>(a, f, s);
    case 1: return cooling_go<PION_EQ, 1>(a, f, s);
    case 2: return cooling_go<PION_EQ, 2>(a, f, s);
    default: return -1;
  }
}
int PION_CAT(launch_stage_dE_, PION_SUFFIX)(const StageArgs &a, hipStream_t s)
{
  switch (a.ntracer) {
    case 0: PION_CASES(stage_dE_go, PION_EQ, 0, a, s)
    case 1: PION_CASES(stage_dE_go, PION_EQ, 1, a, s)
    case 2: PION_CASES(stage_dE_go, PION_EQ, 2, a, s)
    default: return -1;
  }
}
int PION_CAT(launch_flux_test_, PION_SUFFIX)(const FluxTestArgs &a, hipStream_t s)
{
  switch (a.ntracer) {
    case 0: PION_CASES(flux_go, PION_EQ, 0, a, s)
    case 1: PION_CASES(flux_go, PION_EQ, 1, a, s)
    case 2: PION_CASES(flux_go, PION_EQ, 2, a, s)
    default: return -1;
  }
}
int PION_CAT(launch_cell_test_, PION_SUFFIX)(const CellTestArgs &a, hipStream_t s)
{
  switch (a.ntracer) {
    case 0: return cell_go<PION_EQ, 0>(a, s);
    case 1: return cell_go<PION_EQ, 1>(a, s);
    case 2: return cell_go<PION_EQ, 2>(a, s);
    default: return -1;
  }
}
#endif  // PION_PROBE

}  // namespace PION_FPNS
}  // namespace pion
