// pion_handle.h -- shared by the translation units of the C-ABI layer: the handle behind include/pion_gpu.h's opaque
// pointer and the helpers every entry point uses (defined in pion_gpu.hip, used there, in pion_step.hip, in
// pion_bc.hip, in pion_wind.hip, in pion_output.hip, in pion_project.hip and in pion_raytrace.hip).  The kernels
// behind kernels.h's launchers are in kernels_fp.hip, kernels_prepass.hip and kernels_dt.hip.
#ifndef PION_HANDLE_H
#define PION_HANDLE_H

#include <string>
#include <vector>

#include "../../include/pion_gpu.h"
#include "kernels.h"
#include "wind_host.h"

namespace pion::impl {

struct Handle {
  pion_gpu_config cfg;
  GridDesc g;
  int device = 0;
  int ncu = 0;            // compute units of the device (launch shaping)
  hipStream_t stream = 0;
  hipStream_t comm_stream = 0;     // pack/unpack of the z halo (0: the compute stream)
  hipEvent_t ev_packed_src = nullptr, ev_unpacked = nullptr;
  hipStream_t bstream = 0;         // the z-boundary strips of a split stage (two-stream mode): beside the interior part
  hipEvent_t ev_pre = nullptr, ev_bdone = nullptr;
  bool ev_pre_valid = false;
  bool concurrent_strips = true;   // PION_CONCURRENT_STRIPS=0: strips after the interior part on the compute stream
  bool ev_unpacked_valid = false;
  double *dP = nullptr, *dPh = nullptr;
  bool own_state = true;
  uint8_t *dflags = nullptr, *dhll = nullptr;
  double *deta = nullptr;
  double *dsphvol = nullptr;   // spherical 1-D: shell volumes/(4 pi) per cell
  int *derr = nullptr;
  unsigned long long *ddt = nullptr;   // [0]=min t_dyn, [1]=min t_mp (bit patterns)
  unsigned long long *ddt_init = nullptr;  // {1e100, 1e99} on the device: reset source (no host buffer in flight)
  double *hdt = nullptr;               // pinned host staging of {t_dyn, t_mp, error word} (pion_gpu_dt_request)
  hipEvent_t ev_dt = nullptr;
  bool dt_requested = false;
  std::vector<uint8_t> hflags;
  // boundary state
  double refval[6][PION_MAX_NVAR];
  int dmr2_cols = 0;
  long nwind = 0;
  long njet = 0;          // jet inflow cells (XN ghosts), one state for all
  long *djet_idx = nullptr;
  double *djet_state = nullptr;
  long *dwind_idx = nullptr;
  double *dwind_state = nullptr;
  // wind sources (pion_gpu_add_wind_source): cells of all sources concatenated in id order, each in cell-id order
  std::vector<WindSource> wsrc;
  long nws = 0;              // cells of all sources
  long *dws_idx = nullptr;
  double *dws_dist = nullptr, *dws_off = nullptr, *dws_state = nullptr;   // off: [3][nws]; state: [nws][nvar]
  double *dws_theta = nullptr;   // stellar_wind::add_cell's theta (fixed sources; read by rotating ones)
  // rotating sources (pion_gpu_add_rotating_wind_source): the LGM99 tables, built at the first one, for its xi
  bool have_angle = false;
  AngleTables angle;
  // cooling
  CoolDev cool;
  double *dcoolT = nullptr, *dcooltab = nullptr, *dcoolslope = nullptr;
  bool have_tables = false;
  // the cooling functions other than the tabulated one (EP.cooling = 2, 4..7): constants, and for 4..7 the caller's CIE
  // curve (pion_gpu_set_cooling_curve) in dcurve [3][n]: knots, values, spline coefficients
  CoolForm form;
  double *dcurve = nullptr;
  bool have_curve = false;
  // solver state
  double glm_chyp = 0.0, glm_cr = 0.0;
  double refvec_avg[PION_MAX_NVAR];
  bool ph_valid = false;  // dPh holds a genuine half-step state
  bool dt_cached = false; // ddt holds the time-step minima of the current P (left by the last full stage)
  std::string err;
  // timing
  bool timing = false;
  std::vector<hipEvent_t> ev[4];
  double Mu_tot_over_kB = 0.0;
  int use_march = 3, zchunk = 0, rows = 0;  // zchunk 0: chosen per launch; rows 0: chosen per instance (rows2_plan, rows_tiling.h)
  int rows1 = 0;                            // rows of the first-order stage (PION_ROWS1)
  // Plane windows of the rows kernel (rows_tiling.h, "plane windows"): the cells one launch may reach (2^29;
  // PION_ROWS_WINDOW_CELLS: tests and measurements), the windows a whole stage takes (1: today's one launch; 0: the
  // cell-per-thread kernel runs) and the stage-kernel launches of the last part that was issued
  long win_cells = PION_ROWS_WINDOW_CELLS;
  int win_whole = 0;
  int launches_last_part = 0;
  const double *xghost_fresh = nullptr;   // array whose x ghosts (periodic x) the last stage kernel wrote itself
  int zslope_lds = 1;     // k_stage_rows2: carry the z slope in LDS (default; PION_ZSLOPE_LDS=0: rebuild it from plane k-1, R = 4)
  double *ddE = nullptr;  // cooling source per cell (k_cooling_dE -> k_stage_rows2)
  bool fuse_dt = true;    // PION_FUSE_DT=0: always run k_dt (A/B)
  bool uneven_chunks = true;   // PION_UNEVEN_CHUNKS=0: equal plane chunks (A/B)
  bool dt_mp_pending = false;  // k_dt_mp owed after the two streams of a split stage have joined
  bool split_dt_mp = true;     // PION_SPLIT_DT_MP=0: cooling time inside the stage kernel's fused reduction (A/B)
  bool fuse_bc = true;    // PION_FUSE_BC=0: periodic faces one launch per face (A/B)
  // Screened HLLD -> HLL switch prepass (hll_screen.h): a whole-stage launch of k_stage_rows2 leaves the pressure range
  // of every block of the array it writes in dsum; the next stage's prepass evaluates only the blocks that are not
  // provably calm.  sum_arr: the array dsum describes (null: none), valid for the prepass once sum_bc says that the
  // boundary update has refilled that array's ghost cells; dropped by everything else that writes the state.
  bool hll_screen = true;      // PION_HLL_SCREEN=0: always the dense prepass (A/B)
  bool screen_ok = false;      // grid, boundary types and cell lists admit the screen (screen_admitted)
  ScrGeom scr;
  unsigned long long *dsum = nullptr;   // [2][blocks]: keys of the maxima, of the minima
  int *dscr_list = nullptr, *dscr_count = nullptr;
  const double *sum_arr = nullptr;
  bool sum_bc = false;
  bool last_prepass_screened = false;
  // FITS read (pion_output.hip): rejected elements counted by k_unpack_fits since the last pion_gpu_unpack_fits_status;
  // allocated at the first unpack
  unsigned long long *dfits_bad = nullptr;
  // inclined projection (pion_project.hip): the field values of every on-grid cell, [nfields][NR][NZ], grown at the call
  // that needs more, and the pixels whose ray loop reached its trip limit since the last pion_gpu_project_angle_status;
  // both allocated at the first pion_gpu_project_angle
  double *dangle_vals = nullptr;
  long angle_vals_n = 0;
  unsigned long long *dangle_capped = nullptr;
  // radiation sources (pion_raytrace.hip): the sources and their column arrays, created by the first
  // pion_gpu_add_rt_source; null: the handle traces nothing
  struct RtState *rt = nullptr;
};

// the state arrays, the cell flags or the tables were written from outside the stages: what the last stage left
// about its result (time-step minima, pressure summary) no longer holds
static inline void state_changed(Handle *h)
{
  h->dt_cached = false;
  h->sum_arr = nullptr;
  h->sum_bc = false;
}

#define HCHECK(h, call)                                                            \
  do {                                                                             \
    hipError_t e_ = (call);                                                        \
    if (e_ != hipSuccess) {                                                        \
      (h)->err = std::string(#call) + ": " + hipGetErrorString(e_);                \
      return PION_GPU_EDEVICE;                                                     \
    }                                                                              \
  } while (0)

// Every entry point selects the handle's device first: the current device is per-thread state, and
// distinct handles may be driven from distinct host threads (or interleaved on one thread).
static inline Handle *use(void *handle)
{
  Handle *h = (Handle *)handle;
  if (h) (void)hipSetDevice(h->device);
  return h;
}

// Two-stream mode: everything on the compute stream that touches the z ghost planes must run after
// the last unpack on the comm stream.  One wait is enough, later work is ordered behind it.
int order_after_unpack(Handle *h);
long cell_id(const GridDesc &g, int ix, int iy, int iz);
void time_begin(Handle *h, int slot);
inline void time_end(Handle *h, int slot) { time_begin(h, slot); }
FluxCtx make_fluxctx(const Handle *h, double fv_dt);
int check_errword(Handle *h);
// a stage as the kernels see it, and everything of StageArgs that is the same for every part of it (pion_step.hip;
// the cell-update test seam fills its arguments through it too)
struct StageStep { double dt; int space_ooa, is_full_step; };   // dt: the stage's (= FV_dt)
void stage_physics(const Handle *h, const StageStep &st, StageArgs &a);

// one of kernels.h's launchers, in the handle's floating-point build and inside the timing slot (-1: none); a: what it
// takes, the stream last
template <class F, class... A>
int fp_launch(Handle *h, int slot, const char *failed, F *strict, F *fast, const A &... a)
{
  time_begin(h, slot);
  const int rc = h->cfg.strict_fp ? strict(a...) : fast(a...);
  time_end(h, slot);
  if (rc != 0) h->err = failed;
  return (rc != 0) ? PION_GPU_EDEVICE : 0;
}

// get_mp_timescales_no_radiation (calc_timestep.cpp:445-459): EP.MP_timestep_limit 1, 2, 3 ask
// mp_only_cooling::timescales for the cooling time (tc = true); 4 (recombination time only) gets 1e99
// from it (mp_only_cooling.cpp:338), i.e. no limit; anything else is fatal there (EINVAL in create).
static inline bool mp_dt_limited(const pion_gpu_config &cfg)
{
  return cfg.cooling != 0 && cfg.mp_timestep_limit >= 1 && cfg.mp_timestep_limit <= 3;
}

// EP.cooling = 2, 4..7: the kernel instances that take a CoolForm
static inline bool cool_is_form(const pion_gpu_config &cfg)
{
  return cfg.cooling != 0 && cfg.cooling != PION_COOL_WSS09_CIE_LINE_HEAT_COOL;
}
// what a handle with cooling still lacks before anything may be launched (null: nothing).  Flag 8 needs its tables,
// flags 4..7 their curve, KI02 nothing.
static inline const char *cool_missing(const Handle *h)
{
  const int f = h->cfg.cooling;
  if (f == PION_COOL_WSS09_CIE_LINE_HEAT_COOL && !h->have_tables) return "cooling tables not set";
  if (f >= PION_COOL_SD93_CIE && f <= PION_COOL_WSS09_CIE_ONLY_COOLING && !h->have_curve) return "cooling curve not set";
  return nullptr;
}

// device scratch of one call: freed on every return path
template <class T>
struct DevBuf {
  T *p = nullptr;
  ~DevBuf() { if (p) (void)hipFree(p); }
};

// The wind sources (pion_wind.hip) as pion_gpu_update_bcs and pion_gpu_destroy need them: EINVAL if a rotating source
// cannot be evaluated at simtime (before anything is written), the sources' part of the update, their memory freed
int wind_angle_check(Handle *h, double simtime);
int wind_sources_update(Handle *h, double simtime);
void wind_free(Handle *h);
// The radiation sources (pion_raytrace.hip) as pion_gpu_destroy needs them: their memory freed
void rt_free(Handle *h);

// The boundary part of pion_gpu_create (pion_bc.hip): no face holds a state yet, the columns of the DMR2 boundary
void bc_init(Handle *h);

// legacy wind list or wind sources present: the stage kernels read the cell flags, and the periodic ghost images
// are not fused into one launch
static inline bool any_wind(const Handle *h) { return h->nwind > 0 || h->nws > 0; }
}  // namespace pion::impl
#endif
