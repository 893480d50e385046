// pion_bc.hip -- the boundary update of the C-ABI declared in include/pion_gpu.h: pion_gpu_update_bcs and
// pion_gpu_set_jet, and the data-movement kernels they launch: ghost-cell fills (boundaries/*.cpp of the reference),
// the cell reset of the legacy wind list and the jet.  The rules themselves -- which cells, from where, with what
// operation -- are dev_bc.h; a kernel here decodes its cell, calls the rule and stores.  The stellar-wind sources are
// pion_wind.hip.
#include <hip/hip_runtime.h>

#include <cmath>
#include <utility>
#include <vector>

#include "pion_handle.h"
#include "dev_bc.h"

using namespace pion;
using namespace pion::impl;

namespace {

// All periodic faces of a grid in ONE launch (the bench configuration): every ghost cell reads the on-grid cell at its
// wrapped coordinates (periodic_wrap), the same values as the six launches.  zwrap = 0: z faces of kind SLAB, only
// ghosts on on-grid z planes are filled; skipx: the stage kernel has already written the x ghosts of the on-grid rows.
__global__ __launch_bounds__(256) void k_bc_periodic_all(double *T, const GridDesc g, const int nvar, const int zwrap,
                                                         const int skipx)
{
  const long t = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= ghost_slab_count(g, zwrap, skipx)) return;
  int i[3], s[3];
  ghost_slab_cell(g, zwrap, t, i);
  periodic_wrap(g, zwrap, i, s);
  const long c = all_cell_id(g, i), sc = all_cell_id(g, s);
  for (int v = 0; v < nvar; v++) T[v * g.ncell + c] = T[v * g.ncell + sc];
}

// Every external face of a grid in ONE launch, any mix of boundary types: each thread resolves the chain of ITS ghost
// cell down all axes (bc_ghost_value), then the internal DMR2 boundary, which the reference applies last
// (double_Mach_ref_boundaries.cpp:98-147).  Faces of kind SLAB (the faces of the slab axis, z in 3-D and y in 2-D) are
// left alone: the x (and, in 3-D, y) ghosts are still filled over the rows / planes the rank owns, so that what it
// sends carries them.
__global__ __launch_bounds__(256) void k_bc_all(const BCArgs a)
{
  const GridDesc &g = a.g;
  const bool zghosts = (g.ndim == 3);
  const long t = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= ghost_slab_count(g, zghosts, false)) return;
  int i[3];
  ghost_slab_cell(g, zghosts, t, i);
  double val[PION_MAX_NVAR];
  if (!bc_ghost_value(a, a.T, i, g.ndim - 1, 0, val)) return;
  if (dmr2_holds(a, i)) PION_BC_EACH_VAR(v, a.nvar) val[v] = dmr_post_shock(a.nvar, a.ntracer, v);
  bc_store(a.T, g, i, a.nvar, val);
}

// One thread per ghost cell of the list of face d; launched face by face in the order X -> Y -> Z.
__global__ __launch_bounds__(256) void k_bc_face(const BCArgs a, const int d)
{
  const FaceList f = face_list(a.g, d);
  const long t = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= f.total) return;
  int i[3];
  face_list_cell(f, t, i);
  double val[PION_MAX_NVAR];
  if (!bc_ghost_value(a, a.T, i, d / 2, d / 2, val)) return;
  bc_store(a.T, a.g, i, a.nvar, val);
}

// internal DMR2 boundary: y<0 ghost cells above on-grid columns with x<=1/6 get the post-shock state
__global__ void k_bc_dmr2(const BCArgs a)
{
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= a.dmr2_cols * a.g.nbc[1]) return;
  int i[3];
  dmr2_cell(a, t, i);
  const long c = all_cell_id(a.g, i);
  for (int v = 0; v < a.nvar; v++) a.T[v * a.g.ncell + c] = dmr_post_shock(a.nvar, a.ntracer, v);
}

__global__ void k_wind(double *T, const long *idx, const double *states, const long n, const int nvar,
                       const long nc)
{
  const long t = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= n) return;
  const long c = idx[t];
  for (int v = 0; v < nvar; v++) T[v * nc + c] = states[t * nvar + v];
}

// one thread per item, 256 to a block, on the handle's stream
template <class K, class... A>
void launch(Handle *h, K kernel, const long n, A... args)
{
  hipLaunchKernelGGL(kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, h->stream, args...);
}

BCArgs args_of(const Handle *h, double *T, double simtime)
{
  return bc_args(h->g, h->cfg, h->refval, h->dmr2_cols, T, simtime);
}

// The state face d holds from now on, set when the boundaries are assigned (assign_update_bcs.cpp:58-131): inflow and
// fixed faces capture a cell of P as it stands, i.e. after the lower faces have been filled; DMACH the pre-shock state
int assign_face(Handle *h, int d)
{
  const int type = h->cfg.bc_type[d], nvar = h->cfg.nvar;
  if (type == PION_BC_INFLOW || type == PION_BC_FIXED) {
    int i[3];
    bc_capture_cell(h->g, d, type == PION_BC_INFLOW, i);
    const long c = all_cell_id(h->g, i);
    HCHECK(h, hipStreamSynchronize(h->stream));
    for (int v = 0; v < nvar; v++)
      HCHECK(h, hipMemcpy(&h->refval[d][v], h->dP + v * h->g.ncell + c, sizeof(double), hipMemcpyDeviceToHost));
  }
  else if (type == PION_BC_DMACH)
    for (int v = 0; v < nvar; v++) h->refval[d][v] = dmr_pre_shock(nvar, h->cfg.ntracer, v);
  return 0;
}

// TimeUpdateExternalBCs in list order XN,XP,YN,YP,ZN,ZP (assign_update_bcs.cpp:185-252), one launch per face
int face_sequence(Handle *h, double *T, double simtime, bool assign)
{
  for (int d = 0; d < 2 * h->cfg.ndim; d++) {
    if (bc_is_unset(h->cfg.bc_type[d])) continue;
    if (assign) {
      if (int rc = assign_face(h, d)) return rc;
    }
    launch(h, k_bc_face, face_list(h->g, d).total, args_of(h, T, simtime), d);
  }
  return 0;
}

// What pion_gpu_update_bcs puts on the stream, in the reference's order: internal boundaries (stellar wind), external
// faces, DMR2, jet
int update_launches(Handle *h, double *T, double simtime, bool assign)
{
  const GridDesc &g = h->g;
  const int nvar = h->cfg.nvar;
  // TimeUpdateInternalBCs: stellar wind only (assign_update_bcs.cpp:134-183); the legacy cell list, then the wind
  // sources in id order (-> stellar_wind_boundaries.cpp:326-350)
  if (h->nwind > 0) launch(h, k_wind, h->nwind, T, h->dwind_idx, h->dwind_state, h->nwind, nvar, g.ncell);
  if (h->nws > 0) {
    if (int rc = wind_sources_update(h, simtime)) return rc;
  }
  const BcMode mode = bc_mode(h->cfg, h->fuse_bc, any_wind(h), assign);
  // x ghosts of the on-grid rows: already in place when the stage kernel that wrote T also wrote them
  const int skipx = (h->xghost_fresh == T) ? 1 : 0;
  h->xghost_fresh = nullptr;
  if (mode == BC_MODE_PERIODIC_ALL) {
    const int zwrap = (h->cfg.ndim == 3 && h->cfg.bc_type[4] == PION_BC_PERIODIC) ? 1 : 0;
    launch(h, k_bc_periodic_all, ghost_slab_count(g, zwrap, skipx), T, g, nvar, zwrap, skipx);
  }
  else if (mode == BC_MODE_ONE_LAUNCH)
    launch(h, k_bc_all, ghost_slab_count(g, g.ndim == 3, false), args_of(h, T, simtime));
  else if (int rc = face_sequence(h, T, simtime, assign)) return rc;
  // (the one launch holds the DMR2 cells itself)
  if (h->cfg.bc_dmach2 && h->dmr2_cols > 0 && mode != BC_MODE_ONE_LAUNCH)
    launch(h, k_bc_dmr2, (long)h->dmr2_cols * g.nbc[1], args_of(h, T, simtime));
  // internal JETBC, listed after the external boundaries (jet_boundaries.cpp:212-262)
  if (h->njet > 0) launch(h, k_wind, h->njet, T, h->djet_idx, h->djet_state, h->njet, nvar, g.ncell);
  return 0;
}

// cells of the jet inflow: XN ghosts
std::vector<long> jet_cells(const GridDesc &g, bool cart3d, int jetradius)
{
  std::vector<long> idx;
  if (cart3d) {
    // BC_assign_JETBC, 3-D Cartesian (jet_boundaries.cpp:170-201)
    const double jr = jetradius * g.dx;
    for (int iz = 0; iz < g.ng[2]; iz++)
      for (int iy = 0; iy < g.ng[1]; iy++) {
        const double y = g.xmin[1] + (2 * iy + 1) * (0.5 * g.dx), z = g.xmin[2] + (2 * iz + 1) * (0.5 * g.dx);
        if (sqrt(y * y + z * z) <= jr)
          for (int k = 1; k <= g.nbc[0]; k++) idx.push_back(cell_id(g, -k, iy, iz));
      }
  }
  else {
    // 2-D axisymmetric (:96-168): the first jetradius rows above the axis; the profile written at
    // assignment does not survive the first update (:212-262), so the uniform state is all there is
    for (int iy = 0; iy < jetradius; iy++)
      for (int k = 1; k <= g.nbc[0]; k++) idx.push_back(cell_id(g, -k, iy, 0));
  }
  return idx;
}

}  // namespace

void impl::bc_init(Handle *h)
{
  for (int d = 0; d < 6; d++)
    for (int v = 0; v < PION_MAX_NVAR; v++) h->refval[d][v] = 0.0;
  if (h->cfg.bc_dmach2) h->dmr2_cols = dmr2_columns(h->g);
}

extern "C" {

int pion_gpu_set_jet(void *handle, int jetradius, const double *jetstate)
{
  Handle *h = use(handle);
  state_changed(h);   // (cell flags change)
  const pion_gpu_config &cfg = h->cfg;
  const bool cart3d = (cfg.ndim == 3 && cfg.coord_sys == 1 && cfg.eqntype == PION_EQEUL);
  const bool cyl2d = (cfg.ndim == 2 && cfg.coord_sys == 2);
  if ((!cart3d && !cyl2d) || !jetstate) {
    h->err = "jet boundary: 3-D Cartesian Euler or 2-D cylindrical only (jet_boundaries.cpp:88-91,203-206)";
    return PION_GPU_EINVAL;
  }
  if (cyl2d && jetradius > h->g.ng[1]) {
    h->err = "Not enough cells for jet";
    return PION_GPU_EINVAL;
  }
  const std::vector<long> idx = jet_cells(h->g, cart3d, jetradius);
  // refval (jet_boundaries.cpp:60-93): 2-D MHD keeps B along the axis and the toroidal component
  std::vector<double> rv(jetstate, jetstate + cfg.nvar);
  if (cfg.eqntype != PION_EQEUL) {
    rv[5] = jetstate[5];
    rv[6] = 0.0;
    rv[7] = jetstate[6];
  }
  // k_wind takes one state per cell
  const long n = (long)idx.size();
  std::vector<double> st((size_t)n * cfg.nvar);
  for (long k = 0; k < n; k++)
    for (int v = 0; v < cfg.nvar; v++) st[(size_t)k * cfg.nvar + v] = rv[v];
  // the new lists are published, with their count, only once they are whole: a failure leaves the jet as it was
  DevBuf<long> bidx;
  DevBuf<double> bstate;
  if (n > 0) {
    HCHECK(h, hipMalloc(&bidx.p, sizeof(long) * n));
    HCHECK(h, hipMalloc(&bstate.p, sizeof(double) * st.size()));
    HCHECK(h, hipMemcpy(bidx.p, idx.data(), sizeof(long) * n, hipMemcpyHostToDevice));
    HCHECK(h, hipMemcpy(bstate.p, st.data(), sizeof(double) * st.size(), hipMemcpyHostToDevice));
  }
  std::swap(h->djet_idx, bidx.p);   // (the old lists go with the DevBufs)
  std::swap(h->djet_state, bstate.p);
  h->njet = n;
  return 0;
}

int pion_gpu_update_bcs(void *handle, double simtime, int cstep, int maxstep, int assign)
{
  Handle *h = use(handle);
  const bool full = (cstep == maxstep);
  // after a partial step only Ph's ghosts are refreshed, after the full step P's (and Ph=P)
  double *T = full ? h->dP : h->dPh;
  // the pressure summary of T (if any) describes its on-grid cells: this update makes the ghost cells copies of them
  if (h->sum_arr == T && !any_wind(h)) h->sum_bc = true;
  else if (h->sum_arr == T) h->sum_arr = nullptr;
  // a rotating source that cannot be evaluated at simtime: EINVAL before anything is written
  if (h->nws > 0 && h->have_angle) {
    if (int rc = wind_angle_check(h, simtime)) return rc;
  }
  time_begin(h, 2);
  const int rc = update_launches(h, T, simtime, assign != 0);
  time_end(h, 2);
  if (rc) return rc;
  HCHECK(h, hipGetLastError());
  if (full) h->ph_valid = false;
  return 0;
}

}  // extern "C"
