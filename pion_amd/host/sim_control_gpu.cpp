// sim_control_gpu.cpp -- see sim_control_gpu.h
#include "sim_control_gpu.h"

#include "fits_io.h"
#include "slab_comm.h"
#include "snapshot_io.h"

#include <algorithm>
#include <cstdio>
#include <stdexcept>
#include <string>

namespace pion_host {

sim_control_gpu::sim_control_gpu(const pion_gpu_config &c, int device, const pion_backend *backend)
    : cfg(c), be_(backend ? backend : pion_backend_gpu()), h_(nullptr)
{
  const int rc = be_->create(&cfg, device, &h_);
  if (rc != 0) {
    std::string m = h_ ? last_error() : std::string("invalid configuration");
    if (h_) be_->destroy(h_);
    h_ = nullptr;
    throw std::runtime_error(std::string(be_->name) + ": create failed (" + std::to_string(rc) + "): " + m);
  }
}
sim_control_gpu::~sim_control_gpu()
{
  if (h_) be_->destroy(h_);
}
std::string sim_control_gpu::last_error() const
{
  char buf[512] = {0};
  be_->last_error(h_, buf, sizeof buf);
  return buf;
}

int sim_control_gpu::set_comm(slab_comm *c)
{
  comm_ = c;
  return c ? c->attach(h_) : 0;
}

// TimeUpdateInternalBCs + TimeUpdateExternalBCs, then (slab runs) the start of BC_update_BCMPI for the
// array that was just written; stage() completes it between its two parts
int sim_control_gpu::update_boundaries(int cstep, int maxstep, int assign)
{
  int err = be_->update_bcs(h_, T.simtime, cstep, maxstep, assign);
  if (comm_ && !err) err += comm_->start(cstep == maxstep ? 0 : 1);
  return err;
}

int sim_control_gpu::stage(double dt, int space_ooa, int is_full)
{
  if (!comm_) return be_->stage(h_, dt, space_ooa, is_full);
  int err = be_->stage_part(h_, dt, space_ooa, is_full, PION_STAGE_INTERIOR);
  err += comm_->finish();
  err += be_->stage_part(h_, dt, space_ooa, is_full, PION_STAGE_SLABBOUNDARY);
  return err;
}

int sim_control_gpu::finish_halo() { return comm_ ? comm_->finish() : 0; }

// The next step's time step depends on the state the full-step stage has just written (on-grid cells only,
// so not on the boundary update that follows): start its reduction / read-back now, wait for it in
// calculate_timestep -- the boundary kernels and the halo exchange are queued behind it meanwhile.
int sim_control_gpu::request_next_dt()
{
  if (comm_) return comm_->request_min();
  const int err = be_->dt_begin(h_);
  dt_requested_ = (err == 0);
  return err;
}

int sim_control_gpu::Init(const double *P_soa, double simtime)
{
  T.simtime = simtime;
  // a second Init on the same object (restart, new problem): the time-step read-back requested at the end of
  // the last advance_time() belongs to the old state -- discard it here, in the communicator and (upload) in
  // the library, so that calculate_timestep() reduces the state uploaded now
  dt_requested_ = false;
  if (comm_) comm_->reset();
  int err = be_->upload(h_, P_soa);
  // assign_boundary_data + TimeUpdateInternalBCs/ExternalBCs (sim_init.cpp:246-267)
  err += update_boundaries(cfg.tm_ooa, cfg.tm_ooa, 1);
  return err;
}

int sim_control_gpu::add_wind_source(const pion_gpu_wind_source &src, int *id, const double *evo_vcrit, double xi,
                                     bool rotating)
{
  if (be_ != pion_backend_gpu()) return PION_GPU_EINVAL;   // the wind sources live in libpion_gpu.so
  const int err = rotating ? pion_gpu_add_rotating_wind_source(h_, &src, evo_vcrit, xi, id)
                           : pion_gpu_add_wind_source(h_, &src, id);
  if (err) return err;
  n_wind_sources_++;
  // SWP.params[v]->Vinf is the parameter-file value in km/s (0 for most evolving sources: no limit)
  const double lim = 0.1 * cfg.cfl * cfg.dx / (src.vinf * 1.0e5);
  T.wind_dt_limit = (T.wind_dt_limit < 0.0) ? lim : std::min(T.wind_dt_limit, lim);
  return 0;
}

int sim_control_gpu::calculate_timestep()
{
  double t_dyn = 0.0, t_mp = 0.0;
  // slab runs: the minima stay on the device until they are reduced over the ranks
  // (COMM->global_operation_double("MIN", .), sim_control_MPI.cpp:503-504)
  int err;
  if (comm_) err = comm_->allreduce_min(&t_dyn, &t_mp);
  else if (dt_requested_) err = be_->dt_wait(h_, &t_dyn, &t_mp);
  else err = be_->calc_dt(h_, &t_dyn, &t_mp);
  dt_requested_ = false;
  if (err) return err;
  if (T.timestep == 0 && T.first_step_dt_limit > 0.0) t_dyn = std::min(t_dyn, T.first_step_dt_limit);
  if (T.timestep == 0 && T.wind_dt_limit >= 0.0) t_dyn = std::min(t_dyn, T.wind_dt_limit);
  T.dt = std::min(t_dyn, t_mp);
  // Set_GLM_Speeds(td, dx, 0.25/dx) with the *dynamical* step (calc_timestep.cpp:119-131)
  if (cfg.eqntype == PION_EQGLM) err += be_->set_glm_speeds(h_, t_dyn, cfg.dx, 0.25 / cfg.dx);
  // timestep_checking_and_limiting (calc_timestep.cpp:219-262)
  if (T.dt < T.min_timestep) throw std::runtime_error("Timestep too short!");
  T.dt = std::min(T.dt, 1.3 * T.last_dt);  // TIMESTEP_LIMITING
  // outputting every opfreq_time: land on the next output time (calc_timestep.cpp:245-249)
  if (!T.outfile.empty() && T.op_criterion == 1) {
    T.dt = std::min(T.dt, T.next_optime - T.simtime);
    if (T.dt <= 0.0) throw std::runtime_error("Went past output time without outputting!");
  }
  T.dt = std::min(T.dt, T.finishtime - T.simtime);
  if (T.dt <= 0.0) throw std::runtime_error("Negative timestep!");
  return err;
}

int sim_control_gpu::first_order_update(double dt, int ooa)
{
  // Setdt, calc_microphysics_dU, calc_dynamics_dU(OA1), grid_update_state_vector(dt, OA1, ooa)
  return stage(dt, 1, ooa == 1 ? 1 : 0);
}
int sim_control_gpu::second_order_update(double dt, int)
{
  return stage(dt, 2, 1);
}

double sim_control_gpu::advance_time()
{
  int err = 0;
  if (cfg.tm_ooa == 1 && cfg.sp_ooa == 1) {
    err += first_order_update(T.dt, cfg.tm_ooa);
    err += request_next_dt();
    err += update_boundaries(1, 1, 0);
  }
  else if (cfg.tm_ooa == 2 && cfg.sp_ooa == 2) {
    err += first_order_update(0.5 * T.dt, 2);
    err += update_boundaries(1, 2, 0);
    err += second_order_update(T.dt, 2);
    err += request_next_dt();
    err += update_boundaries(2, 2, 0);
  }
  else throw std::runtime_error("Bad OOA requests; choose (1,1) or (2,2)");
  if (err) throw std::runtime_error("advance_time: " + last_error());
  T.simtime += T.dt;
  T.last_dt = T.dt;
  T.timestep++;
  return T.dt;
}

int sim_control_gpu::set_output(const char *base, int op_criterion, int opfreq, double opfreq_time, int checkpoint_freq)
{
  if (!base || !*base || (op_criterion != 0 && op_criterion != 1) || opfreq < 0
      || (op_criterion == 1 && !(opfreq_time > 0.0)))
    return PION_GPU_EINVAL;
  T.outfile = base;
  T.op_criterion = op_criterion;
  T.opfreq = opfreq;
  T.opfreq_time = opfreq_time;
  T.checkpoint_freq = checkpoint_freq;
  // (sim_init::Init sets next_optime from the start time; a restart takes it from the file)
  T.next_optime = T.simtime + opfreq_time;
  T.starttime = T.simtime;
  last_output_step_ = -1;
  return 0;
}

int sim_control_gpu::set_slab_extent(int global_planes, int plane_lo, int bc_lo, int bc_hi)
{
  if (cfg.ndim < 2) return PION_GPU_EINVAL;
  const int n = cfg.ng[cfg.ndim - 1];
  if (plane_lo < 0 || plane_lo + n > global_planes || bc_lo == PION_BC_SLAB || bc_hi == PION_BC_SLAB) return PION_GPU_EINVAL;
  slab.set = true;
  slab.global_planes = global_planes;
  slab.plane_lo = plane_lo;
  slab.bc_lo = bc_lo;
  slab.bc_hi = bc_hi;
  return 0;
}

std::string sim_control_gpu::snapshot_name(long id) const
{
  char b[64];
  snprintf(b, sizeof b, "_%04d.%08ld.pionraw", comm_ ? comm_->rank() : 0, id);
  return T.outfile + b;
}

int sim_control_gpu::set_output_filetype(int type)
{
  if (type != PION_HOST_FILE_PIONRAW && type != PION_HOST_FILE_FITS) {
    io_error_ = "set_output_filetype: unknown file type " + std::to_string(type) + " (PION_HOST_FILE_PIONRAW or PION_HOST_FILE_FITS)";
    return PION_GPU_EINVAL;
  }
  filetype_ = type;
  return 0;
}

std::string sim_control_gpu::output_name(long step) const
{
  if (filetype_ != PION_HOST_FILE_FITS) return snapshot_name(step);
  char b[64];
  snprintf(b, sizeof b, "_%04d.%08ld.fits", comm_ ? comm_->rank() : 0, step);
  return T.outfile + b;
}

std::string sim_control_gpu::projection_name(long step) const
{
  char b[64];
  // the one file of a slab run (written by the last rank) carries rank 0000: the same name whatever the rank count
  snprintf(b, sizeof b, "_proj_%04d.%08ld.fits", (comm_ && !projection_collective()) ? comm_->rank() : 0, step);
  return T.outfile + b;
}

std::string sim_control_gpu::projection_angle_name(long step) const
{
  char b[64];
  snprintf(b, sizeof b, "_proja_%04d.%08ld.fits", comm_ ? comm_->rank() : 0, step);
  return T.outfile + b;
}

std::string sim_control_gpu::columns_name(long step) const
{
  char b[64];
  snprintf(b, sizeof b, "_cols_%04d.%08ld.fits", comm_ ? comm_->rank() : 0, step);
  return T.outfile + b;
}

int sim_control_gpu::write_output(const char *path)
{
  return (filetype_ == PION_HOST_FILE_FITS) ? write_fits(path) : write_snapshot(path);
}

// sim_init::output_data (sim_init.cpp:671-760)
int sim_control_gpu::output_data()
{
  if (T.outfile.empty()) return 0;
  // first the checkpoint, alternating between two files
  const int checkpoint_freq = (T.checkpoint_freq > 0) ? T.checkpoint_freq : 250;
  if (T.timestep != 0 && (T.timestep % checkpoint_freq) == 0) {
    const long id = ((T.timestep % (2 * checkpoint_freq)) == 0) ? 99999998L : 99999999L;
    if (int rc = write_snapshot(snapshot_name(id).c_str())) return rc;
  }
  // always output at the start
  if (T.timestep == 0) {}
  // every opfreq steps (0: only the final state)
  else if (T.op_criterion == 0) {
    if (T.opfreq == 0 && !T.maxtime) return 0;
    if (!T.maxtime && (T.timestep % T.opfreq) != 0) return 0;
  }
  // every opfreq_time time units: at an output time advance the 'next' counter and go on
  else if (T.op_criterion == 1) {
    if (!equalD(T.simtime, T.next_optime) && !T.maxtime) return 0;
    T.next_optime += T.opfreq_time;
  }
  else {
    io_error_ = "op_criterion must be 0 or 1";
    return PION_GPU_EINVAL;
  }
  // (the reference writes a final state that is also a regular output twice, from Time_Int and from Finalise; once here)
  if (last_output_step_ == T.timestep) return 0;
  if (int rc = write_output(output_name(T.timestep).c_str())) return rc;
  if (!proj_fields_.empty())
    if (int rc = write_projection(projection_name(T.timestep).c_str(), proj_axis_, (int)proj_fields_.size(), proj_fields_.data()))
      return rc;
  if (!proja_fields_.empty())
    if (int rc = write_projection_angle(projection_angle_name(T.timestep).c_str(), proja_angle_, (int)proja_fields_.size(),
                                        proja_fields_.data()))
      return rc;
  if (column_output_)
    if (int rc = write_columns(columns_name(T.timestep).c_str())) return rc;
  last_output_step_ = T.timestep;
  return 0;
}

int sim_control_gpu::Time_Int(int nsteps)
{
  int n = 0;
  const bool output = !T.outfile.empty();
  T.maxtime = false;
  if (output && output_data()) throw std::runtime_error("output_data: " + io_error_);
  while (T.simtime < T.finishtime && (nsteps < 0 || n < nsteps)) {
    int err = calculate_timestep();
    if (err) throw std::runtime_error("calculate_timestep: " + last_error());
    advance_time();
    n++;
    if (output) {
      if (output_data()) throw std::runtime_error("output_data: " + io_error_);
      // the end of the run: the final state (the reference: Finalise -> output_data with maxtime set)
      if (T.simtime >= T.finishtime) {
        T.maxtime = true;
        if (output_data()) throw std::runtime_error("output_data: " + io_error_);
      }
    }
  }
  if (finish_halo()) throw std::runtime_error("finish_halo: " + last_error());
  return n;
}

}  // namespace pion_host

// ---- C view of the adapter (used by tests/bench through ctypes) -------------------------------
static thread_local std::string g_last_exception;
extern "C" {
// backend: null = libpion_gpu.so (the product); tests hand in another table (pion_backend.h)
int pion_host_sim_create_backend(const pion_gpu_config *cfg, int device, const pion_backend *backend, void **sim)
{
  try {
    *sim = new pion_host::sim_control_gpu(*cfg, device, backend);
    return 0;
  }
  catch (const std::exception &e) {
    *sim = nullptr;
    g_last_exception = e.what();
    return PION_GPU_EDEVICE;
  }
}
int pion_host_sim_create(const pion_gpu_config *cfg, int device, void **sim)
{
  try {
    *sim = new pion_host::sim_control_gpu(*cfg, device);
    return 0;
  }
  catch (const std::exception &e) {
    *sim = nullptr;
    g_last_exception = e.what();
    return PION_GPU_EDEVICE;
  }
}
void pion_host_sim_destroy(void *s) { delete static_cast<pion_host::sim_control_gpu *>(s); }
void *pion_host_sim_handle(void *s) { return static_cast<pion_host::sim_control_gpu *>(s)->handle(); }
int pion_host_sim_add_wind_source(void *s, const pion_gpu_wind_source *src, int *id)
{
  if (!s || !src) return PION_GPU_EINVAL;
  return static_cast<pion_host::sim_control_gpu *>(s)->add_wind_source(*src, id);
}
int pion_host_sim_add_rotating_wind_source(void *s, const pion_gpu_wind_source *src, const double *evo_vcrit,
                                           double xi, int *id)
{
  if (!s || !src) return PION_GPU_EINVAL;
  return static_cast<pion_host::sim_control_gpu *>(s)->add_wind_source(*src, id, evo_vcrit, xi, true);
}
int pion_host_sim_init(void *s, const double *P, double simtime, double finishtime, double first_dt_limit)
{
  auto *c = static_cast<pion_host::sim_control_gpu *>(s);
  c->T.finishtime = finishtime;
  c->T.first_step_dt_limit = first_dt_limit;
  return c->Init(P, simtime);
}
// restart: step counter and the previous step (SimParams::timestep / last_dt, read back from a snapshot header);
// a fresh problem on a re-used object: (0, 1e100)
int pion_host_sim_set_time(void *s, int timestep, double last_dt)
{
  auto *c = static_cast<pion_host::sim_control_gpu *>(s);
  c->T.timestep = timestep;
  c->T.last_dt = last_dt;
  return 0;
}
int pion_host_sim_time_int(void *s, int nsteps, double *simtime, double *last_dt)
{
  auto *c = static_cast<pion_host::sim_control_gpu *>(s);
  try {
    int n = c->Time_Int(nsteps);
    *simtime = c->T.simtime;
    *last_dt = c->T.last_dt;
    return n;
  }
  catch (const std::exception &e) {
    g_last_exception = e.what();   // the reference prints the rep.error text before exit(1); keep it readable
    return -1;
  }
}
// text of the last exception a pion_host_* call swallowed (empty if none), plus the handle's own error
int pion_host_sim_last_error(void *s, char *buf, int len)
{
  if (!buf || len <= 0) return PION_GPU_EINVAL;
  std::string m = g_last_exception;
  if (s) {
    const std::string h = static_cast<pion_host::sim_control_gpu *>(s)->last_error();
    if (!h.empty()) m += (m.empty() ? "" : " | ") + h;
  }
  snprintf(buf, (size_t)len, "%s", m.c_str());
  return 0;
}
static int io_result(pion_host::sim_control_gpu *c, int rc)
{
  if (rc) g_last_exception = c->io_error();
  return rc;
}
int pion_host_sim_set_output(void *s, const char *base, int op_criterion, int opfreq, double opfreq_time, int checkpoint_freq)
{
  if (!s) return PION_GPU_EINVAL;
  return static_cast<pion_host::sim_control_gpu *>(s)->set_output(base, op_criterion, opfreq, opfreq_time, checkpoint_freq);
}
int pion_host_sim_set_slab_extent(void *s, int global_planes, int plane_lo, int bc_lo, int bc_hi)
{
  if (!s) return PION_GPU_EINVAL;
  return static_cast<pion_host::sim_control_gpu *>(s)->set_slab_extent(global_planes, plane_lo, bc_lo, bc_hi);
}
int pion_host_sim_write_snapshot(void *s, const char *path)
{
  if (!s) return PION_GPU_EINVAL;
  auto *c = static_cast<pion_host::sim_control_gpu *>(s);
  try {
    return io_result(c, c->write_snapshot(path));
  }
  catch (const std::exception &e) {
    g_last_exception = e.what();
    return PION_GPU_EINVAL;
  }
}
int pion_host_sim_write_fits(void *s, const char *path)
{
  if (!s) return PION_GPU_EINVAL;
  auto *c = static_cast<pion_host::sim_control_gpu *>(s);
  try {
    return io_result(c, c->write_fits(path));
  }
  catch (const std::exception &e) {
    g_last_exception = e.what();
    return PION_GPU_EINVAL;
  }
}
int pion_host_sim_write_projection(void *s, const char *path, int axis, int nfields, const pion_gpu_proj_field *fields)
{
  if (!s) return PION_GPU_EINVAL;
  auto *c = static_cast<pion_host::sim_control_gpu *>(s);
  try {
    return io_result(c, c->write_projection(path, axis, nfields, fields));
  }
  catch (const std::exception &e) {
    g_last_exception = e.what();
    return PION_GPU_EINVAL;
  }
}
int pion_host_sim_set_projection_output(void *s, int axis, int nfields, const pion_gpu_proj_field *fields)
{
  if (!s) return PION_GPU_EINVAL;
  auto *c = static_cast<pion_host::sim_control_gpu *>(s);
  try {
    return io_result(c, c->set_projection_output(axis, nfields, fields));
  }
  catch (const std::exception &e) {
    g_last_exception = e.what();
    return PION_GPU_EINVAL;
  }
}
int pion_host_sim_write_projection_angle_trips(void *s, const char *path, double angle_deg, int nfields,
                                               const pion_gpu_proj_field *fields, int trip_limit)
{
  if (!s) return PION_GPU_EINVAL;
  auto *c = static_cast<pion_host::sim_control_gpu *>(s);
  try {
    return io_result(c, c->write_projection_angle(path, angle_deg, nfields, fields, trip_limit));
  }
  catch (const std::exception &e) {
    g_last_exception = e.what();
    return PION_GPU_EINVAL;
  }
}
int pion_host_sim_write_projection_angle(void *s, const char *path, double angle_deg, int nfields, const pion_gpu_proj_field *fields)
{
  return pion_host_sim_write_projection_angle_trips(s, path, angle_deg, nfields, fields, 0);
}
int pion_host_sim_set_projection_angle_output(void *s, double angle_deg, int nfields, const pion_gpu_proj_field *fields)
{
  if (!s) return PION_GPU_EINVAL;
  auto *c = static_cast<pion_host::sim_control_gpu *>(s);
  try {
    return io_result(c, c->set_projection_angle_output(angle_deg, nfields, fields));
  }
  catch (const std::exception &e) {
    g_last_exception = e.what();
    return PION_GPU_EINVAL;
  }
}
int pion_host_sim_add_rt_source(void *s, const pion_gpu_rt_source *src, int *id, double *pos_used)
{
  if (!s || !src) return PION_GPU_EINVAL;
  auto *c = static_cast<pion_host::sim_control_gpu *>(s);
  return io_result(c, c->add_rt_source(*src, id, pos_used));
}
int pion_host_sim_set_column_output(void *s, int on)
{
  if (!s) return PION_GPU_EINVAL;
  auto *c = static_cast<pion_host::sim_control_gpu *>(s);
  return io_result(c, c->set_column_output(on));
}
int pion_host_sim_write_columns(void *s, const char *path)
{
  if (!s) return PION_GPU_EINVAL;
  auto *c = static_cast<pion_host::sim_control_gpu *>(s);
  try {
    return io_result(c, c->write_columns(path));
  }
  catch (const std::exception &e) {
    g_last_exception = e.what();
    return PION_GPU_EINVAL;
  }
}
int pion_host_sim_set_output_filetype(void *s, int type)
{
  if (!s) return PION_GPU_EINVAL;
  auto *c = static_cast<pion_host::sim_control_gpu *>(s);
  return io_result(c, c->set_output_filetype(type));
}
int pion_host_sim_read_snapshot(void *s, const char *const *paths, int npaths)
{
  if (!s) return PION_GPU_EINVAL;
  auto *c = static_cast<pion_host::sim_control_gpu *>(s);
  try {
    return io_result(c, c->read_snapshot(paths, npaths));
  }
  catch (const std::exception &e) {
    g_last_exception = e.what();
    return PION_GPU_EINVAL;
  }
}
int pion_host_sim_read_fits(void *s, const char *const *paths, int npaths)
{
  if (!s) return PION_GPU_EINVAL;
  auto *c = static_cast<pion_host::sim_control_gpu *>(s);
  try {
    const int rc = c->read_fits(paths, npaths);
    g_last_exception = c->io_error();   // on success: empty, or what the files lacked (an image set to zero)
    return rc;
  }
  catch (const std::exception &e) {
    g_last_exception = e.what();
    return PION_GPU_EINVAL;
  }
}
static int read_header(bool fits, const char *path, pion_gpu_config *cfg, pion_host_snapshot_info *info)
{
  try {
    pion_host::snapshot_header hd;
    std::string err;
    const int rc = fits ? pion_host::fits_read_header(path, hd, nullptr, nullptr, err) : pion_host::snapshot_read_header(path, hd, err);
    if (rc) {
      g_last_exception = err;
      return rc;
    }
    if (cfg) *cfg = hd.cfg;
    if (info) *info = hd.info;
    return 0;
  }
  catch (const std::exception &e) {
    g_last_exception = e.what();
    return PION_GPU_EINVAL;
  }
}
int pion_host_snapshot_read_header(const char *path, pion_gpu_config *cfg, pion_host_snapshot_info *info)
{
  return read_header(false, path, cfg, info);
}
int pion_host_fits_read_header(const char *path, pion_gpu_config *cfg, pion_host_snapshot_info *info)
{
  return read_header(true, path, cfg, info);
}
int pion_host_sim_get_time(void *s, double *out)
{
  if (!s || !out) return PION_GPU_EINVAL;
  const pion_host::SimTime &T = static_cast<pion_host::sim_control_gpu *>(s)->T;
  out[0] = T.simtime, out[1] = T.last_dt, out[2] = T.next_optime, out[3] = T.finishtime, out[4] = T.starttime;
  out[5] = (double)T.timestep;
  return 0;
}
int pion_host_sim_download(void *s, int which, double *P)
{
  auto *c = static_cast<pion_host::sim_control_gpu *>(s);
  if (int rc = c->finish_halo()) return rc;
  return c->download(which, P);
}
int pion_host_sim_finish_halo(void *s) { return static_cast<pion_host::sim_control_gpu *>(s)->finish_halo(); }
// hand the sim a slab communicator (pion_host_comm_create); call before pion_host_sim_init
int pion_host_sim_set_comm(void *s, void *comm)
{
  return static_cast<pion_host::sim_control_gpu *>(s)->set_comm(static_cast<pion_host::slab_comm *>(comm));
}
// one step at a time (bench.py times K of them between barriers)
int pion_host_sim_step(void *s, double *dt)
{
  auto *c = static_cast<pion_host::sim_control_gpu *>(s);
  try {
    int err = c->calculate_timestep();
    if (err) {
      g_last_exception = "calculate_timestep: " + c->last_error();
      return err;
    }
    *dt = c->advance_time();
    return 0;
  }
  catch (const std::exception &e) {
    g_last_exception = e.what();
    return -1;
  }
}
}
