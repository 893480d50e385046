// TEST INFRASTRUCTURE: host-side probe of the boundary update's rules (pion_amd/csrc/dev_bc.h).
//
// Runs the functions the kernels of pion_bc.hip call -- ghost-slab enumeration, face lists, source-cell chains, face
// operations, the DMR states, the capture cell of an assignment -- in host loops over a host array, in the three modes
// pion_gpu_update_bcs has: all periodic faces in one pass, every face in one pass (each cell's chain read from a copy
// of the input, so that the pass does not depend on the order of the cells, as the launch does not), and face by face
// in list order with the capture at assignment.  Used through ctypes by tests/test_bc_rule.py, which compares with
// the CPU oracle.  No device code, nothing contracted.
#include <hip/hip_runtime.h>

#include <vector>

#include "../../pion_amd/csrc/dev_bc.h"

using namespace pion;

namespace {
// the grid of a configuration, as pion_gpu_create lays it out
GridDesc grid_of(const pion_gpu_config &cfg)
{
  GridDesc g;
  g.ndim = cfg.ndim;
  g.ncell = 1;
  for (int a = 0; a < 3; a++) {
    g.ng[a] = (a < cfg.ndim) ? cfg.ng[a] : 1;
    g.nbc[a] = (a < cfg.ndim) ? cfg.nbc : 0;
    g.nga[a] = g.ng[a] + 2 * g.nbc[a];
    g.ncell *= g.nga[a];
    g.xmin[a] = cfg.xmin[a];
  }
  g.sy = g.nga[0];
  g.sz = (long)g.nga[0] * g.nga[1];
  g.dx = cfg.dx;
  g.cyl = 0;
  g.sph_vol = nullptr;
  return g;
}

void periodic_all(const GridDesc &g, const pion_gpu_config &cfg, double *P)
{
  const bool zwrap = (cfg.ndim == 3 && cfg.bc_type[4] == PION_BC_PERIODIC);
  const long n = ghost_slab_count(g, zwrap, false);
  for (long t = 0; t < n; t++) {
    int i[3], s[3];
    ghost_slab_cell(g, zwrap, t, i);
    periodic_wrap(g, zwrap, i, s);
    for (int v = 0; v < cfg.nvar; v++) P[v * g.ncell + all_cell_id(g, i)] = P[v * g.ncell + all_cell_id(g, s)];
  }
}

void one_launch(const BCArgs &a)
{
  const GridDesc &g = a.g;
  const std::vector<double> in(a.T, a.T + (size_t)a.nvar * g.ncell);
  const long n = ghost_slab_count(g, g.ndim == 3, false);
  for (long t = 0; t < n; t++) {
    int i[3];
    double val[PION_MAX_NVAR];
    ghost_slab_cell(g, g.ndim == 3, t, i);
    if (!bc_ghost_value(a, in.data(), i, g.ndim - 1, 0, val)) continue;
    if (dmr2_holds(a, i))
      for (int v = 0; v < a.nvar; v++) val[v] = dmr_post_shock(a.nvar, a.ntracer, v);
    bc_store(a.T, g, i, a.nvar, val);
  }
}

void face_sequence(const GridDesc &g, const pion_gpu_config &cfg, double simtime, bool assign, double *P,
                   double (*refval)[PION_MAX_NVAR], int dmr2_cols)
{
  for (int d = 0; d < 2 * cfg.ndim; d++) {
    const int type = cfg.bc_type[d];
    if (bc_is_unset(type)) continue;
    if (assign && (type == PION_BC_INFLOW || type == PION_BC_FIXED)) {
      int i[3];
      bc_capture_cell(g, d, type == PION_BC_INFLOW, i);
      for (int v = 0; v < cfg.nvar; v++) refval[d][v] = P[v * g.ncell + all_cell_id(g, i)];
    }
    else if (assign && type == PION_BC_DMACH)
      for (int v = 0; v < cfg.nvar; v++) refval[d][v] = dmr_pre_shock(cfg.nvar, cfg.ntracer, v);
    const BCArgs a = bc_args(g, cfg, refval, dmr2_cols, P, simtime);
    const FaceList f = face_list(g, d);
    for (long t = 0; t < f.total; t++) {
      int i[3];
      double val[PION_MAX_NVAR];
      face_list_cell(f, t, i);
      if (bc_ghost_value(a, P, i, d / 2, d / 2, val)) bc_store(P, g, i, a.nvar, val);
    }
  }
  const BCArgs a = bc_args(g, cfg, refval, dmr2_cols, P, simtime);
  for (int t = 0; t < a.dmr2_cols * g.nbc[1]; t++) {
    int i[3];
    dmr2_cell(a, t, i);
    for (int v = 0; v < a.nvar; v++) P[v * g.ncell + all_cell_id(g, i)] = dmr_post_shock(a.nvar, a.ntracer, v);
  }
}
}  // namespace

extern "C" {

// the mode pion_gpu_update_bcs takes (BcMode)
int bcp_mode(const pion_gpu_config *cfg, int fuse_bc, int any_wind, int assign)
{
  return (int)bc_mode(*cfg, fuse_bc != 0, any_wind != 0, assign != 0);
}

int bcp_dmr2_cols(const pion_gpu_config *cfg) { return cfg->bc_dmach2 ? dmr2_columns(grid_of(*cfg)) : 0; }

// all-cell coordinates of the cell an assignment of face d captures
void bcp_capture_cell(const pion_gpu_config *cfg, int d, int inflow, int *i)
{
  bc_capture_cell(grid_of(*cfg), d, inflow != 0, i);
}

// centre of the cell with all-cell coordinate i along ax
double bcp_cell_centre(const pion_gpu_config *cfg, int ax, int i) { return cell_centre(grid_of(*cfg), ax, i); }

// One boundary update of P ([nvar][ncell], ghosts included) in the given mode (BcMode).  refval: [6][PION_MAX_NVAR],
// the states the faces hold, written by an assigning face sequence.  Returns 0, or -1 for a mode the arguments do not
// admit (the one launch never assigns; periodic-all needs bc_mode to say so).
int bcp_update(const pion_gpu_config *cfg, int mode, double simtime, int assign, double *P, double *refval)
{
  const GridDesc g = grid_of(*cfg);
  double(*rv)[PION_MAX_NVAR] = (double(*)[PION_MAX_NVAR])refval;
  const int dmr2_cols = bcp_dmr2_cols(cfg);
  if (mode == BC_MODE_PERIODIC_ALL) {
    if (bc_mode(*cfg, true, false, assign != 0) != BC_MODE_PERIODIC_ALL) return -1;
    periodic_all(g, *cfg, P);
  }
  else if (mode == BC_MODE_ONE_LAUNCH) {
    if (assign) return -1;
    one_launch(bc_args(g, *cfg, rv, dmr2_cols, P, simtime));
  }
  else if (mode == BC_MODE_FACE_SEQUENCE) face_sequence(g, *cfg, simtime, assign != 0, P, rv, dmr2_cols);
  else return -1;
  return 0;
}

}  // extern "C"
