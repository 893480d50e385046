// sim_control_gpu.h -- C++ host adapter above the C-ABI (include/pion_gpu.h).
//
// Mirrors the reference's caller side of the hot path, same member names and argument meaning:
//   sim_control::Time_Int            source/sim_control/sim_control.cpp:202-281
//   calc_timestep::calculate_timestep, timestep_checking_and_limiting
//                                     source/sim_control/calc_timestep.cpp:68-153, 219-262
//   time_integrator::advance_time, first_order_update, second_order_update
//                                     source/sim_control/time_integrator.cpp:72-250
//   sim_init::output_data             source/sim_control/sim_init.cpp:671-760   (output times, cadence, checkpoints;
//                                     the file it writes and the restart that reads it: snapshot_io.h)
// so that a maintainer can swap these three functions in a PION build and
// sim_control drives the GPU path unchanged.  Errors follow the reference's convention:
// int error counts are returned and accumulated; unrecoverable conditions throw (the reference
// calls rep.error -> exit(1)).
#ifndef PION_SIM_CONTROL_GPU_H
#define PION_SIM_CONTROL_GPU_H

#include <functional>
#include <string>
#include <vector>

#include "../../include/pion_gpu.h"
#include "pion_backend.h"

namespace pion_host {

struct snapshot_param;   // snapshot_io.h
class PartFile;          // out_file.h
class slab_comm;   // slab_comm.h: slab_comm_rccl (RCCL over xGMI) or slab_comm_shm (host-staged)

// the slice of SimParams (sim_params.h:200-285) the time loop itself reads/writes
struct SimTime {
  double simtime = 0.0, finishtime = 1e300, dt = 0.0, last_dt = 1e100, min_timestep = 0.0;
  int timestep = 0;
  double first_step_dt_limit = -1.0;  // wind / jet limit of calc_dynamics_dt (calc_timestep.cpp:313-323); <0: none
  double wind_dt_limit = -1.0;        // the same for the sources of add_wind_source, min over them; <0: none
  // output (SimParams::op_criterion, opfreq, opfreq_time, next_optime, checkpoint_freq, starttime, maxtime,
  // outFileBase; sim_params.h:200-285).  outfile empty: no output is configured -- nothing is written and
  // calculate_timestep has no output-time clip, whatever the other fields hold
  int op_criterion = 0;        // 0: every opfreq steps (0: the final state only); 1: every opfreq_time time units
  int opfreq = 0;
  double opfreq_time = 0.0, next_optime = 0.0;
  int checkpoint_freq = 0;     // steps between checkpoints; <= 0: 250
  double starttime = 0.0;
  bool maxtime = false;        // the run has reached finishtime (set by Time_Int; check_eosim, sim_control.cpp:289-318)
  std::string outfile;         // outFileBase
};

// where this sim's grid sits in the global problem along the slab axis (the last axis), and the global problem's two
// faces of that axis (PION_BC_*): what a snapshot header describes (set_slab_extent)
struct SlabExtent {
  bool set = false;
  int global_planes = 0, plane_lo = 0, bc_lo = 0, bc_hi = 0;
};

class sim_control_gpu {
 public:
  // backend: what runs below the time loop; null = the product's only one, libpion_gpu.so (pion_backend_gpu())
  sim_control_gpu(const pion_gpu_config &cfg, int device, const pion_backend *backend = nullptr);
  ~sim_control_gpu();
  sim_control_gpu(const sim_control_gpu &) = delete;

  // sim_init::Init (sim_init.cpp:219-267): ReadData, Ph=P, assign + update boundaries
  int Init(const double *P_soa, double simtime);
  // calc_timestep::calculate_timestep
  int calculate_timestep();
  // time_integrator::advance_time and its two stages
  double advance_time();
  int first_order_update(double dt, int ooa);
  int second_order_update(double dt, int ooa);
  // sim_control::Time_Int (sim_control.cpp:202-281); nsteps<0: until finishtime.  With output configured
  // (set_output) it calls output_data() before the loop and after every advance_time, and writes the final state
  // once when simtime reaches finishtime (the reference does that from Finalise with maxtime set)
  int Time_Int(int nsteps);

  // output times and cadence: SimPM.op_criterion / opfreq / opfreq_time / checkpoint_freq / outFileBase; with
  // op_criterion 1, next_optime = simtime + opfreq_time.  EINVAL: op_criterion outside {0, 1}, opfreq < 0,
  // opfreq_time <= 0 with criterion 1, a null or empty base
  int set_output(const char *outfile_base, int op_criterion, int opfreq, double opfreq_time, int checkpoint_freq);
  // a rank of a slab run: the global number of planes of the slab axis, the first one this sim owns, and the global
  // problem's boundary types on the two faces of that axis.  Default: this sim is the whole domain
  int set_slab_extent(int global_planes, int plane_lo, int bc_lo, int bc_hi);
  // sim_init::output_data (sim_init.cpp:671-760): checkpoint, then the regular output if this step is due
  int output_data();
  // <base>_<rank, 4 digits>.<id, 8 digits>.pionraw
  std::string snapshot_name(long id) const;
  // SimPM.typeofop for the regular outputs of output_data(): PION_HOST_FILE_PIONRAW (the default) or
  // PION_HOST_FILE_FITS (<base>_<rank, 4 digits>.<step, 8 digits>.fits).  Checkpoints stay PIONRAW2 (a restart reads
  // either: read_snapshot, read_fits).  EINVAL: any other value
  int set_output_filetype(int type);
  // the regular output of step `step`: its name and the writer the file type selects
  std::string output_name(long step) const;
  int write_output(const char *path);
  // the FITS file (fits_io.h) of this sim's on-grid cells, derived images included; streamed like write_snapshot
  int write_fits(const char *path);
  // the PIONRAW2 file (snapshot_io.h) of this sim's on-grid cells; completes a halo exchange in flight first
  int write_snapshot(const char *path);
  // Projected images (projection_io.cpp; the rules: pion_amd/csrc/dev_project.h, after the reference's
  // analysis/projection/perp_projection.cpp:404-487): a FITS file with write_fits' primary header plus pion_proj_axis
  // and per field pion_proj_<n>_{a,var,coef,b}, and one double-precision IMAGE extension [NJ][NI] per field, EXTNAME =
  // the field's name, in units of code * dx.  Projected on the device (backend entries project_*), or -- a table
  // without them -- from a download by the same functions in a host loop.  EINVAL and a text: what pion_gpu_project
  // refuses; a path that cannot be created; one rank of a slab run with only one of a slab extent and a communicator of
  // more than one rank (or a communicator without send_to_above / recv_from_below).  With both the call is collective:
  // the image of the whole domain is received from the rank below, gains this rank's part and is handed to the rank
  // above; the last rank writes the one file, byte for byte the single-rank file of the global problem
  int write_projection(const char *path, int axis, int nfields, const pion_gpu_proj_field *fields);
  // from now on every regular output of output_data() is accompanied by <base>_proj_<rank, 4 digits>.<step, 8
  // digits>.fits (the one file of a slab run: rank 0000); nfields 0 turns it off again.  The same refusals, made here.  Cadence and time steps are untouched
  int set_projection_output(int axis, int nfields, const pion_gpu_proj_field *fields);
  std::string projection_name(long step) const;
  // A cylindrical (z,R) grid seen at angle_deg (0 < angle_deg < 90) to its axis (projection_io.cpp; the rule:
  // pion_amd/csrc/dev_project_angle.h, after the reference's analysis/projection/angle_projection.cpp): write_fits'
  // primary header plus pion_proj_angle, pion_proj_n_extra, pion_proj_pixdx, pion_proj_pixz0 and the per-field keys, and
  // one double-precision IMAGE extension [NR][NZ + 2 n_extra] per field.  Projected on the device (backend entries
  // project_angle_*), or -- a table without them, or trip_limit > 0 -- from a download by the same rule in a host loop
  // (trip_limit 0: the rule's own limit).  EINVAL, a text and no file: what pion_gpu_project_angle refuses; one rank of
  // several; a pixel whose ray loop reached the trip limit
  int write_projection_angle(const char *path, double angle_deg, int nfields, const pion_gpu_proj_field *fields, int trip_limit = 0);
  // from now on every regular output of output_data() is accompanied by <base>_proja_<rank, 4 digits>.<step, 8
  // digits>.fits; nfields 0 turns it off again.  Independent of set_projection_output
  int set_projection_angle_output(double angle_deg, int nfields, const pion_gpu_proj_field *fields);
  std::string projection_angle_name(long step) const;
  // Ray-traced column densities (columns_io.cpp; pion_gpu_raytrace; the rules: pion_amd/csrc/dev_raytrace.h, after the reference's
  // raytracer_USC).  add_rt_source: Add_Source for one radiation source -- on the backend's handle (entry
  // add_rt_source), or, a table without it, kept here; pos_used (PION_MAX_DIM doubles, may be null): the cell vertex a
  // finite source was moved to.  write_columns: a FITS file with write_fits' primary header plus RT_Nsources and, per
  // source n, RT_position_<n>_<d>, RT_at_infty_<n>, RT_Opacity__<n>, RT_Tau_var__<n> (the reference's names,
  // dataIO/dataio_base.cpp:1267-1282), and per source two double-precision IMAGE extensions of the on-grid cells,
  // Col_Src_<n>_T0 (column to + through the cell) and DCol_Src_<n>_T0 (through it), traced from P as it stands (after
  // the boundary update) and streamed a chunk of planes at a time; a table without the entries downloads array 0 and runs
  // pion_gpu_raytrace_host.  EINVAL and a text: what pion_gpu_add_rt_source refuses; no sources; one rank of a slab run
  // with only one of a slab extent and a communicator of more than one rank (or a communicator without both relay
  // directions).  With both (set before the first source) the calls are collective (columns_io.cpp): sources are given
  // at positions of the whole domain, per source the planes of col are handed from rank to rank away from the source,
  // and every rank writes its own file with its own planes -- images and RT_* keys == the single-rank file's
  int add_rt_source(const pion_gpu_rt_source &src, int *id, double *pos_used);
  int write_columns(const char *path);
  // from now on every regular output of output_data() is accompanied by <base>_cols_<rank, 4 digits>.<step, 8
  // digits>.fits; on = 0 turns it off again.  Cadence and time steps are untouched
  int set_column_output(int on);
  std::string columns_name(long step) const;
  // restart from the files that hold this sim's planes (written by any number of ranks); sets P, Ph, simtime,
  // timestep, last_dt, next_optime, starttime, finishtime and min_timestep, then assigns and updates the boundaries as
  // Init does.  Wind sources, jets and cooling tables are set up by the caller first, as before Init.
  int read_snapshot(const char *const *paths, int npaths);
  // the same restart from FITS files (fits_io.h): the primitive images, found by EXTNAME, unpacked on the device
  // (B times 1/sqrt(4 pi)); an image a file lacks is zeros and a note in io_error(); an element that is not finite or
  // is the reference's null value -1e99 is EINVAL
  int read_fits(const char *const *paths, int npaths);

  // z-slab of a larger domain: exchange the z ghost planes after every boundary update (under the
  // interior part of the next stage) and min-reduce the time step over the ranks
  // (sim_control_pllel, sim_control_MPI.cpp:482-583; MCMD_boundaries.cpp:122-237)
  int set_comm(slab_comm *c);
  // stellar_wind_bc::BC_assign_STWIND (stellar_wind_boundaries.cpp:120-190) for one SWP source: a device-built wind
  // source (pion_gpu_add_wind_source), and its first-step limit 0.1 CFL dx / (Vinf 1e5) (calc_timestep.cpp:318-322).
  // Before Init.  rotating: a type-2 source (pion_gpu_add_rotating_wind_source with evo_vcrit and xi).
  int add_wind_source(const pion_gpu_wind_source &src, int *id, const double *evo_vcrit = nullptr, double xi = 0.0,
                      bool rotating = false);
  int update_boundaries(int cstep, int maxstep, int assign);
  int stage(double dt, int space_ooa, int is_full);
  int finish_halo();
  int request_next_dt();

  int download(int which, double *P_soa) { return be_->download(h_, which, P_soa); }
  const pion_backend *backend() const { return be_; }
  void *handle() { return h_; }
  std::string last_error() const;
  const std::string &io_error() const { return io_error_; }   // text of the last output / snapshot failure

  SimTime T;
  pion_gpu_config cfg;
  SlabExtent slab;

 private:
  const pion_backend *be_;
  void *h_;
  slab_comm *comm_ = nullptr;
  bool dt_requested_ = false;
  int n_wind_sources_ = 0;
  long last_output_step_ = -1;   // step whose regular output has been written
  std::string io_error_;
  int filetype_ = 0;             // PION_HOST_FILE_*
  int proj_axis_ = 0;            // set_projection_output: the images that accompany a regular output (none: empty)
  std::vector<pion_gpu_proj_field> proj_fields_;
  double proja_angle_ = 0.0;     // set_projection_angle_output, likewise
  std::vector<pion_gpu_proj_field> proja_fields_;
  std::vector<pion_gpu_rt_source> rt_sources_, rt_moved_;   // add_rt_source: the sources as given, and at the positions used
  bool rt_on_backend_ = false;                   // they live on the backend's handle too
  bool column_output_ = false;                   // set_column_output
  // columns_io.cpp
  int columns_refused(const char *who);
  bool columns_collective() const;   // one rank of a slab run whose columns are handed along the ranks
  pion_gpu_rt_part columns_part() const;
  int relay_columns(int rc, int id, bool on_device, const double *A, double *col, double *dcol);
  int agree_on(int rc);
  bool rt_as_parts_ = false;         // the sources were added as sources of the whole domain (collective)
  // projection_io.cpp
  bool projection_collective() const;   // one rank of a slab run whose images are assembled along the ranks
  int project_images(int axis, int nfields, const pion_gpu_proj_field *fields, const pion_gpu_proj_part *part, long n, double *img);
  int relay_part(int rc, int axis, int nfields, const pion_gpu_proj_field *fields, const pion_gpu_proj_part &part,
                 std::vector<double> &img);
  int projection_refused(int axis, int nfields, const pion_gpu_proj_field *fields, const char *who);
  int projection_angle_refused(double angle_deg, int nfields, const pion_gpu_proj_field *fields, const char *who);
  // snapshot_io.cpp: what the four writers share (the file itself: out_file.h)
  int path_refused(const char *who, const char *path);
  int snapshot_params(std::vector<snapshot_param> &out, long &slab_n);
  int writer_params(const char *who, std::vector<snapshot_param> &out, long &slab_n);
  int stream_jobs(long njob, const std::function<int(long, int)> &begin, const std::function<int(long, const double *)> &put);
  int stream_runs(PartFile &f, bool fits, int nrun, long nloc, long plane, long off, long stride, const char *who);
  // and what both restarts share: everything but the header reader and the meaning of an element
  int read_files(const char *const *paths, int npaths, bool fits);
};

}  // namespace pion_host
#endif
