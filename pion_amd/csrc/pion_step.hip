// pion_step.hip -- the part of the C-ABI (include/pion_gpu.h) that a time step calls: the time-step reduction, the
// stages and their parts, the halo of a slab.  The handle and the helpers shared with pion_gpu.hip: pion_handle.h.
#include <algorithm>
#include <cmath>
#include <cstring>

#include "pion_handle.h"

using namespace pion;
using namespace pion::impl;

// everything of StageArgs that is the same for every part of a stage
void impl::stage_physics(const Handle *h, const StageStep &st, StageArgs &a)
{
  const pion_gpu_config &cfg = h->cfg;
  a.g = h->g;
  a.flags = h->dflags;
  a.hllflag = h->dhll;
  a.eta = h->deta;
  a.errword = h->derr;
  a.fc = make_fluxctx(h, st.dt);
  a.eqntype = cfg.eqntype;
  a.ntracer = cfg.ntracer;
  a.solver = cfg.solver;
  a.space_ooa = st.space_ooa;
  a.cooling = cfg.cooling;
  a.dt = st.dt;
  a.glm_damp = exp(-st.dt * h->glm_chyp * h->glm_cr);
  a.max_temp = cfg.max_temp;
  a.cool = h->cool;
  a.use_march = h->use_march;
  a.zslope_lds = h->zslope_lds;
  a.plain_cells = any_wind(h) ? 0 : 1;
  // periodic x: k_stage_rows2 writes the x ghost images of its rows (the boundary launch then skips them)
  a.xwrap = (a.use_march != 0 && h->fuse_bc && cfg.bc_type[0] == PION_BC_PERIODIC
             && cfg.bc_type[1] == PION_BC_PERIODIC && h->g.ng[0] >= 2 * h->g.nbc[0]) ? 1 : 0;
  a.ncu = h->ncu;
  a.cfl = cfg.cfl;
}

namespace {

// halo planes of the slab axis (the last axis: z planes in 3-D, y rows in 2-D): buffer layout
// [nvar][nbc][ny_all][nx_all] (2-D: [nvar][nbc][nx_all])
__global__ void k_halo(double *A, double *buf, const GridDesc g, const int nvar, const int face, const int pack)
{
  const int sa = g.ndim - 1;
  const long plane = (sa == 2) ? (long)g.nga[0] * g.nga[1] : (long)g.nga[0];
  const long per = plane * g.nbc[sa];
  const long t = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= per * nvar) return;
  const int v = (int)(t / per);
  const long r = t % per;
  const int k = (int)(r / plane);
  const long xy = r % plane;
  int izall;
  if (pack) izall = (face == 2 * sa) ? g.nbc[sa] + k : g.ng[sa] + k;       // on-grid planes next to the face
  else izall = (face == 2 * sa) ? k : g.nbc[sa] + g.ng[sa] + k;            // ghost planes of the face
  const long c = xy + plane * izall;
  if (pack) buf[t] = A[v * g.ncell + c];
  else A[v * g.ncell + c] = buf[t];
}

// the arguments of the time-step kernels (k_dt, k_dt_mp); Ph: the array the cooling time is taken from
DtArgs dt_args(const Handle *h, const double *Ph, const int do_mp)
{
  DtArgs a;
  a.g = h->g;
  a.P = h->dP;
  a.Ph = Ph;
  a.flags = h->dflags;
  a.result = h->ddt;
  a.errword = h->derr;
  a.eqntype = h->cfg.eqntype;
  a.nvar = h->cfg.nvar;
  a.gamma = h->cfg.gamma;
  a.cfl = h->cfg.cfl;
  a.do_mp = do_mp;
  a.cool = h->cool;
  return a;
}


// One stage, or a part of one (PION_STAGE_WHOLE / _INTERIOR / _SLABBOUNDARY).  The split lets the halo
// exchange of a slab run under the interior: the interior part reads no ghost plane of the slab axis (the last
// axis: z planes in 3-D, y rows in 2-D), the boundary part (the nbc on-grid planes / rows next to each face of
// that axis) waits for the unpacked halo.
static inline int slab_axis(const Handle *h) { return h->g.ndim - 1; }
static bool stage_can_split(const Handle *h)
{
  const int sa = slab_axis(h);
  return h->use_march != 0 && !h->deta && (h->g.ndim == 3 || h->g.ndim == 2)
         && h->g.ng[sa] > 2 * h->g.nbc[sa] && !(h->cfg.tm_ooa == 1 && h->cfg.sp_ooa == 1);
}

// min of the cooling time over the array d.Ph into ddt[1]: k_dt_mp
static int launch_cooling_time(Handle *h, const DtArgs &d, hipStream_t s)
{
  return fp_launch(h, 3, "cooling-time kernel launch failed", fp_strict::launch_dt_mp, fp_fast::launch_dt_mp, d, h->form, s);
}

// Does this handle admit the screened prepass?  3-D Cartesian grid run by k_stage_rows2 with HLLD; every face periodic,
// outflow, one-way outflow, reflecting or axis-reflecting (k_bc_all / k_bc_face / k_bc_periodic_all leave exact copies
// of on-grid pressures in the ghost cells of those, and of no other type); no wind, jet or DMR2 cells; blocks at
// the faces wide enough to hold the copied cells.
static bool screen_admitted(Handle *h)
{
  const pion_gpu_config &cfg = h->cfg;
  if (!h->hll_screen || !h->dhll || cfg.ndim != 3 || h->g.cyl != 0 || h->use_march == 0 || h->g.nbc[2] < 2) return false;
  if (any_wind(h) || h->njet > 0 || cfg.bc_dmach2) return false;
  // (plane windows: the summary's block indices are absolute plane numbers, which a rebased launch does not know)
  if (h->g.ncell * 8L >= (1L << 32) || h->win_whole > 1) return false;
  int per[3];
  for (int d = 0; d < 3; d++) {
    for (int f = 2 * d; f < 2 * d + 2; f++) {
      const int t = cfg.bc_type[f];
      if (!(t == PION_BC_PERIODIC || t == PION_BC_OUTFLOW || t == PION_BC_ONEWAY_OUT || t == PION_BC_REFLECTING
            || t == PION_BC_AXISYMMETRIC))
        return false;
    }
    if ((cfg.bc_type[2 * d] == PION_BC_PERIODIC) != (cfg.bc_type[2 * d + 1] == PION_BC_PERIODIC)) return false;
    per[d] = (cfg.bc_type[2 * d] == PION_BC_PERIODIC) ? 1 : 0;
    if (!scr_axis_ok(h->g.ng[d], h->g.nbc[d])) return false;
  }
  h->scr = scr_geom(h->g.ng, h->g.nbc, per);
  if (!h->dsum) {
    const size_t n = (size_t)scr_total(h->scr);
    if (hipMalloc(&h->dsum, 2 * n * sizeof(unsigned long long)) != hipSuccess) return false;
    if (hipMalloc(&h->dscr_list, n * sizeof(int)) != hipSuccess) return false;
    if (hipMalloc(&h->dscr_count, sizeof(int)) != hipSuccess) return false;
    if (hipMemset(h->dscr_count, 0, sizeof(int)) != hipSuccess) return false;
  }
  return true;
}

// [lo, hi) of on-grid indices along the slab axis: planes in 3-D, rows in 2-D
struct Range {
  int lo = 0, hi = 0;
  bool empty() const { return hi <= lo; }
  int n() const { return empty() ? 0 : hi - lo; }
};

// What one launch of the stage kernel updates: r[0] and, for the two boundary strips (ONE launch), r[1]; whether it is
// the first / last part of its stage; its launch stream, and whether that runs beside the compute stream.
struct StagePart {
  Range r[2];
  bool first, last;
  hipStream_t stream;
  bool beside;
  bool whole() const { return first && last; }
};

// The three parts: a whole stage, the interior [nb, nz-nb), which reads no ghost plane of the slab axis, and both
// strips [0, nb) and [nz-nb, nz), on the compute stream or beside it on `side`.  A 1-D grid has no slab axis and never
// splits: its (whole) stages take the z axis -- one plane, no ghosts -- and nothing reads the range.
int part_axis(const Handle *h) { return slab_axis(h) > 0 ? slab_axis(h) : 2; }
StagePart part_whole(const Handle *h) { return {{{0, h->g.ng[part_axis(h)]}, {}}, true, true, h->stream, false}; }
StagePart part_interior(const Handle *h)
{
  const int nz = h->g.ng[part_axis(h)], nb = h->g.nbc[part_axis(h)];
  return {{{nb, nz - nb}, {}}, true, false, h->stream, false};
}
StagePart part_strips(const Handle *h, hipStream_t side)
{
  const int nz = h->g.ng[part_axis(h)], nb = h->g.nbc[part_axis(h)];
  return {{{0, nb}, {nz - nb, nz}}, false, true, side ? side : h->stream, side != nullptr};
}

// The all-cell planes whose flags a part of a split stage is the first to need for its range r: the faces of updated
// planes [lo, hi) touch the flags of [lo-1, hi+1); of those the interior part, which goes first, evaluated
// [nb-1, nz-nb+1).  (A stage splits only if nz > 2 nb, stage_can_split: a strip then ends below or starts above that.)
Range flag_planes(const StagePart &pt, const Range r, const int nb, const int nz)
{
  Range f = {r.lo - 1, r.hi + 1};
  if (!pt.first && f.lo < nb - 1) f.hi = std::min(f.hi, nb - 1);        // what lies below the interior part's
  else if (!pt.first) f.lo = std::max(f.lo, nz - nb + 1);               // what lies above
  return r.empty() ? Range{} : Range{f.lo + nb, f.hi + nb};
}
// as cells, [c0, c1) for r[0] and [c2, c3) for r[1]; a whole stage covers every cell incl. ghosts like the reference's loop
void flag_cells(const Handle *h, const StagePart &pt, PrepassArgs &p)
{
  p.c1 = h->g.ncell;
  if (pt.whole()) return;
  const int sa = slab_axis(h), nb = h->g.nbc[sa], nz = h->g.ng[sa];
  const long sst = (sa == 2) ? h->g.sz : h->g.sy;   // cells per plane (3-D) / row (2-D) of the slab axis
  const Range f0 = flag_planes(pt, pt.r[0], nb, nz), f1 = flag_planes(pt, pt.r[1], nb, nz);
  p.c0 = f0.lo * sst;
  p.c1 = f0.hi * sst;
  p.c2 = f1.lo * sst;
  p.c3 = f1.hi * sst;
}

// preprocess_data (solver_eqn_base.cpp:353-415): the HLLD -> HLL switch and the H-correction of the stencil state S
int run_prepass(Handle *h, const StageStep &st, const StagePart &pt, const double *S)
{
  const pion_gpu_config &cfg = h->cfg;
  PrepassArgs p{};   // (divv, gradp: debug outputs, null; no second range, no summary)
  p.g = h->g;
  p.S = S;
  p.hllflag = h->dhll;
  p.eta = h->deta;
  p.eqntype = cfg.eqntype;
  p.nvar = cfg.nvar;
  p.space_ooa = st.space_ooa;
  p.gamma = cfg.gamma;
  flag_cells(h, pt, p);
  // the summary the last stage left of S, if nothing but the boundary update has touched S since
  h->screen_ok = screen_admitted(h);
  if (pt.whole() && h->screen_ok && h->sum_arr == S && h->sum_bc) {
    p.hsum = h->dsum;
    p.scr = h->scr;
    p.scr_list = h->dscr_list;
    p.scr_count = h->dscr_count;
  }
  h->last_prepass_screened = (p.hsum != nullptr);
  return fp_launch(h, 1, "prepass launch failed", fp_strict::launch_prepass, fp_fast::launch_prepass, p, pt.stream);
}

// stencil state, start-of-step state and destination
int stage_arrays(Handle *h, const StageStep &st, const double *S, StageArgs &a)
{
  a.S = S;
  a.Pc = h->dP;
  // first half step: P -> Ph.  Full step: in place on P (each thread reads P only at its own cell).
  a.out = st.is_full_step ? h->dP : h->dPh;
  if (st.is_full_step && !h->ph_valid && h->cfg.sp_ooa == 2 && st.space_ooa == 2) {
    // a full second-order stage straight from P would read neighbours that are being overwritten
    h->err = "full-step stage requires a preceding half-step stage";
    return PION_GPU_EINVAL;
  }
  // first-order scheme (OA1/OA1): stencil and destination coincide -> go through Ph
  if (st.is_full_step && S == h->dP) a.out = h->dPh;
  return 0;
}

// The ranges as the kernels read them, the one place that knows the three encodings.  3-D: planes [kz0, kz1) and, if
// kz3 > kz2, [kz2, kz3).  2-D rows kernel: rows_tiling.h, "2-D row ranges" -- a grid of as many rows as a range has,
// its one "plane" per range numbered by the range's first row.  Other grids: whole stages only, ranges not read.
int stage_ranges(Handle *h, const StagePart &pt, StageArgs &a)
{
  const Range &r0 = pt.r[0], &r1 = pt.r[1];
  a.kz1 = 1;
  if (h->g.ndim == 3) {
    a.kz0 = r0.lo;
    a.kz1 = r0.hi;
    a.kz2 = r1.lo;
    a.kz3 = r1.empty() ? r1.lo : r1.hi;
  }
  else if (h->g.ndim == 2 && h->use_march != 0) {
    if (!r1.empty() && r1.n() != r0.n()) {
      h->err = "stage: the two row strips of a 2-D launch must have the same number of rows";
      return PION_GPU_EINVAL;
    }
    a.g.ng[1] = r0.n();
    a.kz0 = r0.lo;
    a.kz1 = r0.lo + 1;
    a.kz2 = r1.lo;
    a.kz3 = r1.empty() ? r1.lo : r1.lo + 1;
  }
  return 0;
}

// rows per wavefront, plane chunks (rows_tiling.h; PION_ROWS / PION_ROWS1 / PION_ZCHUNK / PION_UNEVEN_CHUNKS override)
void stage_tiling(const Handle *h, const int np, StageArgs &a)
{
  Rows2PlanIn p;
  p.ndim = h->g.ndim;
  p.nx = h->g.ng[0];
  p.ny = a.g.ng[1];                        // (2-D: the rows of the range, which is what the launch tiles)
  p.np = (h->g.ndim == 3) ? np : 1;        // (the planes of the first range)
  p.ncu = h->ncu;
  p.nv = h->cfg.nvar;
  p.euler = (h->cfg.eqntype == PION_EQEUL);
  p.march = (a.use_march != 0);
  p.zslope_lds = (a.zslope_lds != 0);
  p.second_order = (a.space_ooa == 2);
  p.uneven = h->uneven_chunks;
  p.want_rows = h->rows;
  p.want_rows1 = h->rows1;
  p.want_zchunk = h->zchunk;
  const Rows2Plan pl = rows2_plan(p);
  a.rows = pl.rows;
  a.rows_auto = pl.rows_auto;
  a.zchunk = pl.zchunk;
  a.zcmax = pl.zcmax;
  a.nzb = pl.nzb;
}

// Plane windows (rows_tiling.h, "plane windows"): while a whole stage of the handle takes more than one window, every
// range of a part is launched window by window -- the two strips of a split stage as launches of their own --, each
// launch a copy of the part's arguments REBASED to its window [w_lo, w_hi): every per-cell pointer advanced by w_lo
// planes (3-D) / rows (2-D) of the slab axis in 64-bit host arithmetic, the window's planes numbered from 0, the tiling
// planned for the window.  g.ncell, the stride from variable to variable, stays the grid's.  The cylindrical instance
// takes R from the row number: its copy of xmin[1] moves with the window (the slab rule, DESIGN.md s5 "Positions").
bool stage_windowed(const Handle *h) { return h->use_march != 0 && h->win_whole > 1 && h->g.ndim >= 2; }
StageArgs stage_window(const Handle *h, const StageArgs &part, const int w_lo, const int w_hi)
{
  StageArgs a = part;
  const long off = (long)w_lo * ((h->g.ndim == 3) ? h->g.sz : h->g.sy);   // cells from the array's base to the window's
  a.S += off;
  a.Pc += off;
  a.out += off;
  a.flags += off;
  if (a.hllflag) a.hllflag += off;
  if (a.eta) a.eta += off;
  if (a.dE) a.dE += off;
  a.kz0 = a.kz2 = a.kz3 = 0;
  if (h->g.ndim == 3) a.kz1 = w_hi - w_lo;
  else {
    a.g.ng[1] = w_hi - w_lo;   // (rows_tiling.h, "2-D row ranges": the range [0, w_hi - w_lo) of the rebased array)
    a.kz1 = 1;
    if (h->g.cyl == 1) a.g.xmin[1] = h->g.xmin[1] + w_lo * h->g.dx;
  }
  stage_tiling(h, w_hi - w_lo, a);
  return a;
}

// what a launch does besides the update: decided, then into StageArgs and onto the stream
struct StageExtras { bool fuse_dt, split_mp, leave_sum; };
int stage_extras(Handle *h, const StageStep &st, const StagePart &pt, StageArgs &a, StageExtras &x)
{
  const pion_gpu_config &cfg = h->cfg;
  // fused time-step reduction: the full stage leaves min(t_dyn), min(t_mp) of the new state in ddt
  // (second-order stages only: the first-order instances of k_stage_rows2 carry no reduction code)
  x.fuse_dt = h->fuse_dt && st.is_full_step && st.space_ooa == 2 && a.use_march != 0
              && ((h->g.ndim == 3 && h->g.nbc[2] >= 2) || h->g.ndim == 2) && a.out == h->dP;
  // the cooling time: not in the stage kernel's fused reduction but in its own launch behind the last part of the
  // stage (k_dt_mp, rate tables in LDS; PION_SPLIT_DT_MP=0: fused, A/B)
  // (EP.cooling = 2, 4..7: always split -- the stage kernels carry the tabulated rate only)
  x.split_mp = x.fuse_dt && mp_dt_limited(cfg) && (h->split_dt_mp || cool_is_form(cfg));
  // pressure-range summary of the array this launch writes: whole stages of the rows kernel on a grid of ordinary
  // cells, rows per wavefront dividing the block height
  x.leave_sum = pt.whole() && h->dhll && h->screen_ok && a.plain_cells && a.rows >= 1 && cfg.cooling == 0
                && !h->deta && !a.fc.mp.present
                && PION_SCR_BY % a.rows == 0 && !(st.is_full_step && a.out == h->dPh);
  state_changed(h);   // (every part: stage_end renews what holds of the new state)
  if (x.leave_sum) {
    a.hsum = h->dsum;
    a.hsum_n = scr_total(h->scr);
    a.hsum_nbx = h->scr.nb[0];
    a.hsum_nby = h->scr.nb[1];
    a.hsum_nbz = h->scr.nb[2];
    HCHECK(h, hipMemsetAsync(h->dsum, 0, 2 * (size_t)a.hsum_n * sizeof(unsigned long long), pt.stream));
  }
  a.dt_mp = (mp_dt_limited(cfg) && !x.split_mp) ? 1 : 0;
  if (x.fuse_dt) {
    if (pt.first)
      HCHECK(h, hipMemcpyAsync(h->ddt, h->ddt_init, 2 * sizeof(double), hipMemcpyDeviceToDevice, pt.stream));
    a.dtres = h->ddt;
  }
  return 0;
}

// behind the last part of a stage: what the stage owes, and what it left on the handle
int stage_end(Handle *h, const StageStep &st, const StagePart &pt, const StageExtras &x, const StageArgs &a)
{
  if (x.split_mp) {
    // (a part launched on the side stream runs beside the interior part: the launch then follows where the compute
    // stream has joined both, pion_gpu_stage_part)
    if (pt.beside) h->dt_mp_pending = true;
    else if (int rc = launch_cooling_time(h, dt_args(h, h->dP, 1), pt.stream)) return rc;
  }
  if (st.is_full_step && a.out == h->dPh) {
    // OA1/OA1: copy the result back to P ("P = Ph", time_integrator.cpp:938-939)
    const size_t nb = sizeof(double) * (size_t)h->cfg.nvar * h->g.ncell;
    HCHECK(h, hipMemcpyAsync(h->dP, h->dPh, nb, hipMemcpyDeviceToDevice, pt.stream));
  }
  h->ph_valid = !st.is_full_step;
  h->dt_cached = x.fuse_dt;
  if (x.leave_sum) h->sum_arr = a.out;
  h->xghost_fresh = a.xwrap ? ((st.is_full_step && a.out == h->dPh) ? h->dP : a.out) : nullptr;
  return 0;
}

// One part of a stage, as the list of its steps, in the order their work goes onto the part's stream
int stage_launch(Handle *h, const StageStep &st, const StagePart &pt)
{
  if (const char *m = cool_missing(h)) {
    h->err = m;
    return PION_GPU_EINVAL;
  }
  // the stencil state: Ph.  At the start of a step Ph == P in every cell.
  const double *S = h->ph_valid ? h->dPh : h->dP;
  if (int rc = (h->dhll || h->deta) ? run_prepass(h, st, pt, S) : 0) return rc;
  StageArgs a{};   // (what no step sets: null / 0)
  if (int rc = stage_arrays(h, st, S, a)) return rc;
  stage_physics(h, st, a);
  if (int rc = stage_ranges(h, pt, a)) return rc;
  stage_tiling(h, pt.r[0].n(), a);
  const bool form = cool_is_form(h->cfg);
  if (h->cfg.cooling != 0 && (form || a.use_march != 0)) {
    // calc_noRT_microphysics_dU as its own launch (thread per cell, full occupancy): dE per cell.  EP.cooling = 2, 4..7
    // take their source from it for the cell-per-thread kernel too, over the whole grid (k_stage integrates flag 8 itself)
    a.dE = h->ddE;
    StageArgs ac = a;
    if (a.use_march == 0) {
      ac.kz0 = 0;
      ac.kz1 = h->g.ng[2];
      ac.kz2 = ac.kz3 = 0;
    }
    if (int rc = fp_launch(h, 1, "cooling kernel launch failed", fp_strict::launch_cooling_dE, fp_fast::launch_cooling_dE,
                           ac, h->form, pt.stream))
      return rc;
  }
  StageExtras x;
  if (int rc = stage_extras(h, st, pt, a, x)) return rc;
  if (pt.first && !pt.last && h->concurrent_strips && !h->timing && h->comm_stream && h->comm_stream != h->stream) {
    // interior part of a split stage: everything the z-boundary strips depend on besides the halo (the
    // previous stage, its boundary update, this part's flags, the reset of the dt minima) is on the stream up
    // to here -- the strips may run beside the interior kernel from this point on (pion_gpu_stage_part)
    if (!h->ev_pre) HCHECK(h, hipEventCreateWithFlags(&h->ev_pre, hipEventDisableTiming));
    HCHECK(h, hipEventRecord(h->ev_pre, pt.stream));
    h->ev_pre_valid = true;
  }
  const char *const failed = "stage kernel launch failed (unsupported eqn/solver/tracer combination?)";
  h->launches_last_part = 0;
  if (form && a.use_march == 0) {
    if (int rc = fp_launch(h, 0, failed, fp_strict::launch_stage_dE, fp_fast::launch_stage_dE, a, pt.stream)) return rc;
    h->launches_last_part = 1;
  }
  else if (!stage_windowed(h)) {
    if (int rc = fp_launch(h, 0, failed, fp_strict::launch_stage, fp_fast::launch_stage, a, pt.stream)) return rc;
    h->launches_last_part = 1;
  }
  else {
    const int sa = slab_axis(h);
    const long sst = (sa == 2) ? h->g.sz : h->g.sy;
    for (const Range &r : pt.r) {
      const int nw = rows_windows_count(r.lo, r.hi, sst, h->g.nbc[sa], h->win_cells);   // (0 for an empty range)
      for (int i = 0; i < nw; i++) {
        int w_lo, w_hi;
        rows_window(r.lo, r.hi, nw, i, &w_lo, &w_hi);
        const StageArgs w = stage_window(h, a, w_lo, w_hi);
        if (int rc = fp_launch(h, 0, failed, fp_strict::launch_stage, fp_fast::launch_stage, w, pt.stream)) return rc;
        h->launches_last_part++;
      }
    }
  }
  return pt.last ? stage_end(h, st, pt, x, a) : 0;
}

// the communication stream, and the two events that order it against the compute stream
hipStream_t halo_stream(const Handle *h) { return h->comm_stream ? h->comm_stream : h->stream; }
int halo_src_ready(Handle *h)
{
  if (halo_stream(h) == h->stream) return 0;
  // the planes to send were written (stage) and their x/y ghosts filled (BCs) on the compute stream
  if (!h->ev_packed_src) HCHECK(h, hipEventCreateWithFlags(&h->ev_packed_src, hipEventDisableTiming));
  HCHECK(h, hipEventRecord(h->ev_packed_src, h->stream));
  HCHECK(h, hipStreamWaitEvent(halo_stream(h), h->ev_packed_src, 0));
  return 0;
}
int halo_arrived(Handle *h)
{
  if (halo_stream(h) == h->stream) return 0;
  if (!h->ev_unpacked) HCHECK(h, hipEventCreateWithFlags(&h->ev_unpacked, hipEventDisableTiming));
  HCHECK(h, hipEventRecord(h->ev_unpacked, halo_stream(h)));
  h->ev_unpacked_valid = true;
  return 0;
}

}  // namespace

extern "C" {

int pion_gpu_calc_dt_device(void *handle, void **dptr)
{
  Handle *h = use(handle);
  const DtArgs a = dt_args(h, h->ph_valid ? h->dPh : h->dP, mp_dt_limited(h->cfg) ? 1 : 0);
  if (const char *m = a.do_mp ? cool_missing(h) : nullptr) {
    h->err = m;
    return PION_GPU_EINVAL;
  }
  if (!h->dt_cached) {
    // (after a full step through k_stage_rows2 the minima of the new state are already in ddt)
    HCHECK(h, hipMemcpyAsync(h->ddt, h->ddt_init, 2 * sizeof(double), hipMemcpyDeviceToDevice, h->stream));
    // EP.cooling = 2, 4..7: k_dt, which carries the tabulated rate only, for the dynamics alone, then the cooling time of
    // the same array from k_dt_mp
    const bool form = cool_is_form(h->cfg);
    DtArgs d = a;
    if (form) d.do_mp = 0;
    if (int rc = fp_launch(h, 3, "dt kernel launch failed", fp_strict::launch_dt, fp_fast::launch_dt, d, h->stream)) return rc;
    if (int rc = (form && a.do_mp) ? launch_cooling_time(h, a, h->stream) : 0) return rc;
    h->dt_cached = true;
  }
  if (dptr) *dptr = h->ddt;
  return 0;
}

int pion_gpu_dt_request(void *handle)
{
  Handle *h = use(handle);
  if (!h->hdt) HCHECK(h, hipHostMalloc((void **)&h->hdt, 4 * sizeof(double), hipHostMallocDefault));
  if (!h->ev_dt) HCHECK(h, hipEventCreateWithFlags(&h->ev_dt, hipEventDisableTiming));
  // {min t_dyn, min t_mp} and the device error word, one event for both
  HCHECK(h, hipMemcpyAsync(h->hdt, h->ddt, 2 * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  HCHECK(h, hipMemcpyAsync(h->hdt + 2, h->derr, sizeof(int), hipMemcpyDeviceToHost, h->stream));
  HCHECK(h, hipEventRecord(h->ev_dt, h->stream));
  h->dt_requested = true;
  return 0;
}

int pion_gpu_dt_wait(void *handle, double *t_dyn, double *t_mp)
{
  Handle *h = use(handle);
  if (!h->dt_requested) {
    h->err = "pion_gpu_dt_wait without pion_gpu_dt_request";
    return PION_GPU_EINVAL;
  }
  HCHECK(h, hipEventSynchronize(h->ev_dt));
  h->dt_requested = false;
  *t_dyn = h->hdt[0];
  *t_mp = h->hdt[1];
  int e;
  memcpy(&e, h->hdt + 2, sizeof e);
  if (e) return check_errword(h);   // (re-reads and clears the word, builds the message)
  return 0;
}

int pion_gpu_read_dt(void *handle, double *t_dyn, double *t_mp)
{
  if (int rc = pion_gpu_dt_request(handle)) return rc;
  return pion_gpu_dt_wait(handle, t_dyn, t_mp);
}

int pion_gpu_calc_dt(void *handle, double *t_dyn, double *t_mp)
{
  if (int rc = pion_gpu_calc_dt_device(handle, nullptr)) return rc;
  return pion_gpu_read_dt(handle, t_dyn, t_mp);
}

int pion_gpu_set_glm_speeds(void *handle, double dt, double dx, double cr)
{
  Handle *h = use(handle);
  h->glm_chyp = h->cfg.cfl * dx / dt;  // GLMsetPsiSpeed(FV_cfl*delx/delt, cr)
  h->glm_cr = cr;
  return 0;
}

int pion_gpu_stage_part(void *handle, double dt_stage, int space_ooa, int is_full_step, int part)
{
  Handle *h = use(handle);
  const StageStep st = {dt_stage, space_ooa, is_full_step};
  if (part == PION_STAGE_WHOLE) {
    if (int rc = order_after_unpack(h)) return rc;
    return stage_launch(h, st, part_whole(h));
  }
  const bool split = stage_can_split(h);
  if (part == PION_STAGE_INTERIOR) {
    if (!split) return 0;  // everything happens in the boundary call
    return stage_launch(h, st, part_interior(h));
  }
  if (part != PION_STAGE_SLABBOUNDARY) return PION_GPU_EINVAL;
  if (split && h->ev_pre_valid && h->ev_unpacked_valid) {
    // Two-stream mode: the strips (4 of the slab's planes: a launch of ~2100 short wavefronts on 2048 slots)
    // go to a third stream that waits for the halo and for the point of the compute stream just before the
    // interior kernel, so that they fill the slots the interior launch leaves idle in its last round instead
    // of running after it; the compute stream continues behind both.
    h->ev_pre_valid = false;
    if (!h->bstream) HCHECK(h, hipStreamCreateWithFlags(&h->bstream, hipStreamNonBlocking));
    if (!h->ev_bdone) HCHECK(h, hipEventCreateWithFlags(&h->ev_bdone, hipEventDisableTiming));
    HCHECK(h, hipStreamWaitEvent(h->bstream, h->ev_pre, 0));
    HCHECK(h, hipStreamWaitEvent(h->bstream, h->ev_unpacked, 0));
    if (int rc = stage_launch(h, st, part_strips(h, h->bstream))) return rc;
    HCHECK(h, hipEventRecord(h->ev_bdone, h->bstream));
    HCHECK(h, hipStreamWaitEvent(h->stream, h->ev_bdone, 0));
    if (h->dt_mp_pending) {
      h->dt_mp_pending = false;
      if (int rc2 = launch_cooling_time(h, dt_args(h, h->dP, 1), h->stream)) return rc2;
    }
    return order_after_unpack(h);
  }
  h->ev_pre_valid = false;
  // the z ghost planes must have arrived: order the compute stream after the last unpack
  if (int rc = order_after_unpack(h)) return rc;
  if (!split) return stage_launch(h, st, part_whole(h));
  return stage_launch(h, st, part_strips(h, nullptr));
}

int pion_gpu_stage(void *handle, double dt_stage, int space_ooa, int is_full_step)
{
  return pion_gpu_stage_part(handle, dt_stage, space_ooa, is_full_step, PION_STAGE_WHOLE);
}

int pion_gpu_rows_windows(const pion_gpu_config *cfg, long limit_cells, int lo, int hi, int max_windows, int *w_lo,
                          int *w_hi)
{
  if (!cfg || cfg->ndim < 1 || cfg->ndim > 3 || cfg->nbc < 1 || max_windows < 0) return PION_GPU_EINVAL;
  if (max_windows > 0 && (!w_lo || !w_hi)) return PION_GPU_EINVAL;
  if (limit_cells > PION_ROWS_WINDOW_CELLS) return PION_GPU_EINVAL;   // (more than a 32-bit byte offset reaches)
  for (int a = 0; a < cfg->ndim; a++)
    if (cfg->ng[a] < 1) return PION_GPU_EINVAL;
  const int sa = cfg->ndim - 1;
  if (lo < 0 || hi > cfg->ng[sa] || lo >= hi) return PION_GPU_EINVAL;
  // the grids pion_gpu_create gives to the rows kernel: 3-D and 2-D (not spherical) with two ghost layers
  if (cfg->ndim == 1 || cfg->nbc < 2 || cfg->coord_sys == 3) return 0;
  const long L = (limit_cells <= 0) ? PION_ROWS_WINDOW_CELLS : limit_cells;
  long s = cfg->ng[0] + 2L * cfg->nbc;
  if (sa == 2) s *= cfg->ng[1] + 2L * cfg->nbc;
  const int nw = rows_windows_count(lo, hi, s, cfg->nbc, L);
  for (int i = 0; i < nw && i < max_windows; i++) rows_window(lo, hi, nw, i, &w_lo[i], &w_hi[i]);
  return nw;
}

int pion_gpu_get_rows_windows(void *handle, long *limit_cells, int *windows_whole_stage, int *launches_last_part)
{
  const Handle *h = (const Handle *)handle;
  if (!h) return PION_GPU_EINVAL;
  if (limit_cells) *limit_cells = h->win_cells;
  if (windows_whole_stage) *windows_whole_stage = h->win_whole;
  if (launches_last_part) *launches_last_part = h->launches_last_part;
  return 0;
}

int pion_gpu_advance_time(void *handle, double dt, double simtime)
{
  Handle *h = use(handle);
  int rc;
  if (h->cfg.tm_ooa == 1 && h->cfg.sp_ooa == 1) {
    if ((rc = pion_gpu_stage(handle, dt, 1, 1))) return rc;
    return pion_gpu_update_bcs(handle, simtime, 1, 1, 0);
  }
  if (h->cfg.tm_ooa == 2 && h->cfg.sp_ooa == 2) {
    if ((rc = pion_gpu_stage(handle, 0.5 * dt, 1, 0))) return rc;
    if ((rc = pion_gpu_update_bcs(handle, simtime, 1, 2, 0))) return rc;
    if ((rc = pion_gpu_stage(handle, dt, 2, 1))) return rc;
    return pion_gpu_update_bcs(handle, simtime, 2, 2, 0);
  }
  h->err = "Bad OOA requests; choose (1,1) or (2,2)";
  return PION_GPU_EINVAL;
}

long pion_gpu_halo_count(void *handle)
{
  Handle *h = use(handle);
  if (h->g.ndim == 2) return (long)h->cfg.nvar * h->g.nbc[1] * h->g.nga[0];   // rows of the slab axis y
  return (long)h->cfg.nvar * h->g.nbc[2] * h->g.nga[0] * h->g.nga[1];         // (0 for a 1-D grid)
}
static int halo_go(Handle *h, int which, int face, void *dbuf, int pack)
{
  const int sa = slab_axis(h);
  if (sa < 1 || (face != 2 * sa && face != 2 * sa + 1)) return PION_GPU_EINVAL;
  double *A = (which == 0) ? h->dP : h->dPh;
  const long n = pion_gpu_halo_count(h);
  if (int rc = pack ? halo_src_ready(h) : 0) return rc;
  hipLaunchKernelGGL(k_halo, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, halo_stream(h), A, (double *)dbuf, h->g,
                     h->cfg.nvar, face, pack);
  HCHECK(h, hipGetLastError());
  return pack ? 0 : halo_arrived(h);
}
int pion_gpu_halo_spans(void *handle, int which, pion_gpu_halo_spans_t *out)
{
  Handle *h = use(handle);
  const int sa = slab_axis(h);
  if (sa < 1 || !out) return PION_GPU_EINVAL;
  double *A = (which == 0) ? h->dP : h->dPh;
  // (sz: cells per plane of the slab axis -- an x-y plane in 3-D, a row with its x ghosts in 2-D)
  const long nb = h->g.nbc[sa], nz = h->g.ng[sa], sz = (sa == 2) ? h->g.sz : h->g.sy;
  out->recv_lo = A;                       // ghost planes 0 .. nb-1
  out->send_lo = A + nb * sz;             // first on-grid planes
  out->send_hi = A + nz * sz;             // last on-grid planes (all-cell planes nz .. nz+nb-1)
  out->recv_hi = A + (nz + nb) * sz;      // ghost planes nz+nb ..
  out->count_per_var = nb * sz;
  out->var_stride = h->g.ncell;
  out->nvar = h->cfg.nvar;
  return 0;
}
int pion_gpu_halo_begin(void *handle) { return halo_src_ready(use(handle)); }
int pion_gpu_halo_end(void *handle) { return halo_arrived(use(handle)); }
int pion_gpu_pack_halo(void *handle, int which, int face, void *dbuf) { return halo_go(use(handle), which, face, dbuf, 1); }
int pion_gpu_unpack_halo(void *handle, int which, int face, void *dbuf) { return halo_go(use(handle), which, face, dbuf, 0); }

}  // extern "C"
