/* pion_host.h -- C view of the C++ host layer above include/pion_gpu.h (libpion_host.so, pion_amd/host/).
 *
 * The host layer mirrors the reference's CALLER side of the hot path -- the three functions of sim_control that a PION
 * build overrides and the MPI-side pieces they use:
 *   pion_host_sim_*   pion_host::sim_control_gpu   sim_control::Time_Int                sim_control/sim_control.cpp:202-281
 *                                                  calc_timestep::calculate_timestep    sim_control/calc_timestep.cpp:68-262
 *                                                  time_integrator::advance_time        sim_control/time_integrator.cpp:72-250
 *   pion_host_comm_*  pion_host::slab_comm         comm_mpi::send/receive_cell_data     comms/comm_mpi.cpp:287-425
 *                     (slab_comm_rccl: RCCL;       comm_mpi::global_operation_double    comms/comm_mpi.cpp:182-209
 *                      slab_comm_shm: host memory) MCMD_bc::BC_update_BCMPI             boundaries/MCMD_boundaries.cpp:122-237
 *   pion_host_build_cooling_tables                 mp_only_cooling::gen_mpoc_lookup_tables  microphysics/mp_only_cooling.cpp:528-579
 * C++ callers use the classes directly (sim_control_gpu.h, slab_comm.h); this view is what ctypes / a C driver binds.
 * All functions return 0 or a negative PION_GPU_* code unless stated; none exits. */
#ifndef PION_HOST_H
#define PION_HOST_H

#include "pion_gpu.h"

#ifdef __cplusplus
extern "C" {
#endif

struct pion_backend;   /* pion_amd/host/pion_backend.h: what the loop calls below itself; NULL = libpion_gpu.so */

/* ---- the time loop (one object per rank / GPU) */
int pion_host_sim_create(const pion_gpu_config *cfg, int device, void **sim);
int pion_host_sim_create_backend(const pion_gpu_config *cfg, int device, const struct pion_backend *backend, void **sim);
void pion_host_sim_destroy(void *sim);
void *pion_host_sim_handle(void *sim);                       /* the pion_gpu handle (set-up calls: wind cells, tables) */
/* sim_init::Init: upload P ([nvar][nz_all][ny_all][nx_all]), Ph = P, assign + update boundaries.  A second call on
 * the same object discards the time-step request of the previous state. */
int pion_host_sim_init(void *sim, const double *P, double simtime, double finishtime, double first_step_dt_limit);
int pion_host_sim_set_time(void *sim, int timestep, double last_dt);   /* restart: SimParams::timestep / last_dt */
int pion_host_sim_step(void *sim, double *dt);                /* calculate_timestep + advance_time */
int pion_host_sim_time_int(void *sim, int nsteps, double *simtime, double *last_dt);   /* returns steps taken, < 0 on error */
int pion_host_sim_download(void *sim, int which, double *P);
int pion_host_sim_finish_halo(void *sim);
int pion_host_sim_set_comm(void *sim, void *comm);            /* before pion_host_sim_init */
/* stellar_wind_bc::BC_assign_STWIND for one source (pion_gpu_add_wind_source on the loop's handle), before
 * pion_host_sim_init; also the first-step limit 0.1 CFL dx / (vinf 1e5) of calc_timestep.cpp:318-322 (src->vinf in
 * km/s, 0 = no limit), combined by min with init's first_step_dt_limit.  EINVAL on a backend other than
 * libpion_gpu.so. */
int pion_host_sim_add_wind_source(void *sim, const pion_gpu_wind_source *src, int *id);
/* The same for a rotating star (pion_gpu_add_rotating_wind_source: type 2, the table's vcrit column, xi), with the
 * same first-step limit.  A boundary update the source cannot evaluate (omega <= 0 or Tw <= 1000 K at that time:
 * pion_gpu_update_bcs returns EINVAL) stops pion_host_sim_time_int with -1 and the text in pion_host_sim_last_error. */
int pion_host_sim_add_rotating_wind_source(void *sim, const pion_gpu_wind_source *src, const double *evo_vcrit,
                                           double xi, int *id);
int pion_host_sim_last_error(void *sim, char *buf, int len);

/* ---- output times, checkpoints, snapshot and restart (pion_amd/host/snapshot_io.h)
 *   sim_init::output_data                          sim_control/sim_init.cpp:671-760
 *   the output-time clip of the time step          sim_control/calc_timestep.cpp:245-249
 *   constants::equalD                              constants.cpp:48-70
 *   the header names                               dataIO/dataio_base.cpp:60-440, 1372-1390
 * pion_host_sim_set_output: SimPM.outFileBase, op_criterion (0: every opfreq steps, opfreq 0 = only the final state;
 * 1: every opfreq_time time units, next_optime = simtime + opfreq_time), checkpoint_freq (<= 0: 250 steps).  From then
 * on pion_host_sim_time_int writes <base>_<rank, 4 digits>.<step, 8 digits>.pionraw at step 0, at every output step /
 * time and once when simtime reaches finishtime, and the checkpoints <base>_<rank>.99999998 / 99999999.pionraw in turn;
 * with op_criterion 1 the time step is clipped to land on next_optime ("Went past output time without outputting!"
 * when it cannot).  Without this call nothing is written and the time steps are unchanged.  Call it after
 * pion_host_sim_init and before pion_host_sim_read_snapshot (a restart takes next_optime from the file).
 * EINVAL: op_criterion outside {0, 1}, opfreq < 0, opfreq_time <= 0 with criterion 1, a NULL or empty base. */
int pion_host_sim_set_output(void *sim, const char *outfile_base, int op_criterion, int opfreq, double opfreq_time,
                             int checkpoint_freq);
/* A rank of a slab run: the planes of the slab axis in the global problem, the first one this sim owns, and the
 * global problem's boundary types (PION_BC_*) on the two faces of that axis -- a rank's PION_BC_SLAB faces are not a
 * property of the problem.  Default: the sim is the whole domain.  EINVAL: a 1-D grid, a range outside the global
 * planes, PION_BC_SLAB as a global face. */
int pion_host_sim_set_slab_extent(void *sim, int global_planes, int plane_lo, int bc_lo, int bc_hi);
/* The PIONRAW2 file of this sim's on-grid cells: 8-byte magic, a text header of "name value" lines (the reference's
 * parameter names where one exists, pion_-prefixed keys otherwise; NGrid, Xmin, Xmax and BC_* describe the GLOBAL
 * problem), then fp64 little-endian [nvar][slab_n][ny][nx] at pion_data_offset, code units, no ghost cells.  The
 * planes leave the device a chunk at a time (pion_gpu_pack_ongrid): host memory is two chunks whatever the grid. */
int pion_host_sim_write_snapshot(void *sim, const char *path);
/* The FITS file of this sim's on-grid cells (pion_amd/host/fits_io.h; FITS standard 4.0, after the reference's
 * dataio_fits::OutputData): a primary HDU without data whose header carries every parameter of the PIONRAW2 header
 * (pion_data_offset excepted) as "HIERARCH <name> = <value>" cards under the same names (arrays element-numbered:
 * NGrid0..2, Xmin0..2, Xmax0..2, Ref_Vector0..; doubles %.17G), then one double-precision IMAGE extension per image
 * of pion_gpu_fits_images -- the primitive variables, Eint or Temp, and for MHD / GLM divB and Ptot --, NAXIS1 = nx,
 * the rank's own extent, EXTNAME = the image's name.  Bx, By, Bz and divB carry the reference's sqrt(4 pi); psi and
 * Ptot do not.  The images are packed on the device, derived fields and byte order included (pion_gpu_pack_fits), and
 * leave it a chunk of planes at a time: host memory is two chunks.  divB reads the ghost cells the last boundary
 * update and halo exchange left.  Every rank writes its own file.  EINVAL and a text: more than five tracers, a path
 * that cannot be created.  Never exits.  Read back by pion_host_sim_read_fits. */
int pion_host_sim_write_fits(void *sim, const char *path);
/* File type of the regular outputs of pion_host_sim_time_int (step 0, every output step or time, the final state):
 * PION_HOST_FILE_PIONRAW (the default) or PION_HOST_FILE_FITS, <base>_<rank, 4 digits>.<step, 8 digits>.fits.  The
 * checkpoints stay PIONRAW2 (a restart reads either file type).  Cadence, the time-step clip and every dt are untouched.
 * EINVAL and a text: any other value. */
#define PION_HOST_FILE_PIONRAW 0
#define PION_HOST_FILE_FITS 1
int pion_host_sim_set_output_filetype(void *sim, int type);
/* Projected images of the state (pion_gpu_project; the rules: pion_amd/csrc/dev_project.h): column sums of a 3-D
 * Cartesian grid along axis 0, 1 or 2, or, for a cylindrical (z,R) grid and axis PION_PROJ_AXIS_PERP, the reference's
 * perpendicular Abel integral (analysis/projection/perp_projection.cpp: calc_projection_column, :404-487, slopes
 * :338-390, pixels :225-252).  Up to 8 fields coef rho^a T^b w per file.
 * pion_host_sim_write_projection: a FITS file with the primary header of pion_host_sim_write_fits plus pion_proj_axis
 *   and, per field n = 0 .., pion_proj_<n>_a, _var, _coef, _b; then one double-precision IMAGE extension per field,
 *   NAXIS1 = NI, NAXIS2 = NJ, EXTNAME = the field's name, big-endian, in units of (code units of the field) * dx (the
 *   Abel images: * length).  Written under a ".part" name and renamed; pion_amd/fits.py reads it.  The images are made
 *   on the device and only they cross to the host; a backend table without the projection entries downloads the state
 *   and runs the same functions in a host loop.
 * pion_host_sim_set_projection_output: from now on every regular output of pion_host_sim_time_int (step 0, each output
 *   step or time, the final state) is accompanied by <base>_proj_<rank, 4 digits>.<step, 8 digits>.fits; nfields = 0
 *   turns that off.  Cadence, the time-step clip, checkpoints and every dt are untouched.
 * EINVAL and a text, never an exit: everything pion_gpu_project refuses (1-D, spherical and 2-D Cartesian grids, a
 * line of sight along the axis of a cylindrical grid, NR == 1, a bad field, b != 0 without cooling); a path that cannot
 * be created; one rank of a slab run that has a slab extent but no communicator of more than one rank, or such a
 * communicator but no extent, or a communicator without the send / receive pair.
 * One rank of a slab run with both (pion_host_sim_set_slab_extent, pion_host_sim_set_comm): the call is COLLECTIVE, every
 *   rank makes it with the same arguments.  The image of the whole domain travels from rank 0 upwards, each rank
 *   continuing the running sums over its own planes (pion_gpu_project_part; dev_project.h, "parts"); the last rank
 *   writes the one file -- byte for byte the file a single-rank sim of the global problem writes, its header stating
 *   the global NGrid / Xmin / Xmax and nothing rank-local -- and the other ranks create nothing.  Byte for byte holds
 *   where dx and the slab axis' xmin are dyadic (every rank's xmin - plane_lo dx is then the global Xmin exactly, as
 *   the slab decomposition of a (z,R) grid requires anyway); otherwise the header's Xmin and the Abel geometry are
 *   evaluated with that difference, which may be an ulp off the single grid's.  The column sums of a 3-D grid use no
 *   position and are bit for bit in any case.  The regular outputs
 *   name it <base>_proj_0000.<step>.fits whatever the rank count.  A rank that fails passes the failure on: every rank
 *   above it returns EINVAL, no file appears, no rank blocks. */
int pion_host_sim_write_projection(void *sim, const char *path, int axis, int nfields, const pion_gpu_proj_field *fields);
int pion_host_sim_set_projection_output(void *sim, int axis, int nfields, const pion_gpu_proj_field *fields);
/* A cylindrical (z,R) grid seen at angle_deg (0 < angle_deg < 90) to its symmetry axis (pion_gpu_project_angle; the rule:
 * pion_amd/csrc/dev_project_angle.h, the reference's analysis/projection/angle_projection.cpp as written).
 * pion_host_sim_write_projection_angle: a FITS file with the primary header of pion_host_sim_write_fits plus
 *   pion_proj_angle (degrees), pion_proj_n_extra, pion_proj_pixdx (the pixel size along image x, dx sin(angle)),
 *   pion_proj_pixz0 (the image's origin in z: the centre of pixel (0, 0) times sin(angle); project2D.cpp:446-449) and
 *   the per-field keys of pion_host_sim_write_projection; then one double-precision IMAGE extension per field, NAXIS1 =
 *   NI = NZ + 2 n_extra, NAXIS2 = NR, EXTNAME = the field's name, big-endian, in units of (code units of the field) *
 *   length.  Written under a ".part" name and renamed.  The images are made on the device; a backend table without the
 *   two project_angle entries downloads the state and runs the same rule in a host loop.
 * pion_host_sim_set_projection_angle_output: from now on every regular output of pion_host_sim_time_int is accompanied
 *   by <base>_proja_<rank, 4 digits>.<step, 8 digits>.fits; nfields = 0 turns that off.  Independent of
 *   pion_host_sim_set_projection_output.  Cadence, the time-step clip, checkpoints and every dt are untouched.
 * pion_host_sim_write_projection_angle_trips: the writer over the host loop with the ray loops' trip limit given instead
 *   of the rule's own 2 (NZ + NR) + 8 (trip_limit >= 1): for tests of the refusal below.
 * EINVAL and a text, never an exit, and no file: everything pion_gpu_project_angle refuses; a path that cannot be
 * created; a sim that is one rank of several (a slab extent or a communicator of more than one rank: rays are not
 * carried from rank to rank); an image with a pixel whose ray loop reached the trip limit. */
int pion_host_sim_write_projection_angle(void *sim, const char *path, double angle_deg, int nfields, const pion_gpu_proj_field *fields);
int pion_host_sim_set_projection_angle_output(void *sim, double angle_deg, int nfields, const pion_gpu_proj_field *fields);
int pion_host_sim_write_projection_angle_trips(void *sim, const char *path, double angle_deg, int nfields,
                                               const pion_gpu_proj_field *fields, int trip_limit);
/* Ray-traced column densities (pion_gpu_raytrace; the rules: pion_amd/csrc/dev_raytrace.h, after the reference's
 * short-characteristics tracer raytracing/raytracer_SC.cpp).
 * pion_host_sim_add_rt_source: Add_Source (:1183-1314) for one radiation source, pion_gpu_add_rt_source on the loop's
 *   handle; pos_used (PION_MAX_DIM doubles, may be NULL): the cell vertex a finite source was moved to.  A backend table
 *   without the entry keeps the source in the sim.
 * pion_host_sim_write_columns: a FITS file with the primary header of pion_host_sim_write_fits plus RT_Nsources and, per
 *   source n, RT_position_<n>_<d> (d = 0, 1, 2; a source at infinity: -/+1e200 on its axis), RT_at_infty_<n>,
 *   RT_Opacity__<n>, RT_Tau_var__<n> -- the reference's names (dataIO/dataio_base.cpp:1267-1282) --; then per source two
 *   double-precision IMAGE extensions of the on-grid cells, EXTNAME Col_Src_<n>_T0 (the column to + through the cell,
 *   what the reference writes under that name) and DCol_Src_<n>_T0 (the column through it), big-endian.  The columns
 *   are traced from P as it stands, after the boundary update, on the device, and streamed a chunk of planes at a time;
 *   a backend table without the entries downloads the state and runs pion_gpu_raytrace_host.  Written under a ".part"
 *   name and renamed; pion_amd/fits.py reads it.
 * pion_host_sim_set_column_output: from now on (on != 0) every regular output of pion_host_sim_time_int is accompanied
 *   by <base>_cols_<rank, 4 digits>.<step, 8 digits>.fits; on = 0 turns that off.  Cadence, the time-step clip,
 *   checkpoints, every dt and the regular outputs themselves are untouched: tracing only reads the state.
 * One rank of a slab run (pion_host_sim_set_slab_extent AND a communicator of more than one rank that relays both ways,
 *   both set before the first source): the three calls are collective.  Sources are given at positions of the WHOLE
 *   domain, and pos_used is that position on every rank.  write_columns takes the sources in id order: receive the plane
 *   of col the rank's role names (pion_gpu_rt_chain), trace, send the own lowest / highest plane on -- one plane per
 *   internal face and source, away from the source.  Every rank writes its own file (<base>_cols_<rank>...) with its own
 *   planes: the header of its FITS snapshot plus the RT_* keys, the images == those planes of the single-rank file.  A
 *   rank that fails passes the failure on and the ranks then agree: every rank returns EINVAL, no file appears, no rank
 *   blocks.
 * EINVAL and a text, never an exit: everything pion_gpu_add_rt_source refuses; no source; a path that cannot be created;
 * one rank of a slab run with only one of a slab extent and such a communicator, or one that became a rank after its
 * sources were added. */
int pion_host_sim_add_rt_source(void *sim, const pion_gpu_rt_source *src, int *id, double *pos_used);
int pion_host_sim_write_columns(void *sim, const char *path);
int pion_host_sim_set_column_output(void *sim, int on);
/* The rules of the images as host functions (pion_amd/csrc/dev_project.h), without a sim or a device: cfg describes the
 * grid, A is a whole array [nvar][ncell_all] with its ghost cells.  What a backend table without projection entries gets.
 *   pion_host_project_on_host:      every pixel by proj_column / abel_column, img = [nfields][NJ][NI]
 *   pion_host_project_part_on_host: this grid as one rank's part (pion_gpu_project_part), added into the image of the
 *                                   whole domain img = [nfields][NJ_global][NI_global], in/out
 *   pion_host_project_part_refused: NULL, or the text with which pion_gpu_project_part refuses these arguments
 * EINVAL for what is refused or null. */
const char *pion_host_project_part_refused(const pion_gpu_config *cfg, int axis, int nfields, const pion_gpu_proj_field *fields,
                                           const pion_gpu_proj_part *part, const void *img);
int pion_host_project_on_host(const pion_gpu_config *cfg, int axis, int nfields, const pion_gpu_proj_field *fields,
                              const double *A, double *img);
int pion_host_project_part_on_host(const pion_gpu_config *cfg, int axis, int nfields, const pion_gpu_proj_field *fields,
                                   const pion_gpu_proj_part *part, const double *A, double *img);
/* The rule of the inclined projection as host functions (pion_amd/csrc/dev_project_angle.h), likewise.
 *   pion_host_project_angle_count:   doubles of the images, nfields NR NI, and *n_extra (may be NULL); < 0 for what
 *                                    pion_gpu_project_angle_count refuses, *why (may be NULL) then points to the text
 *   pion_host_project_angle_on_host: every pixel by angle_pixel in a host loop, img = [nfields][NR][NI]
 *   pion_host_project_angle_rule:    the same with the ray loops' trip limit given (trip_limit >= 1), *ncapped = the
 *                                    pixels whose loop reached it; tan_angle, inv_sin (either may be NULL): the two
 *                                    numbers of the angle the rule was handed
 * EINVAL for what is refused or null. */
long pion_host_project_angle_count(const pion_gpu_config *cfg, double angle_deg, int nfields, int *n_extra, const char **why);
int pion_host_project_angle_on_host(const pion_gpu_config *cfg, double angle_deg, int nfields, const pion_gpu_proj_field *fields,
                                    const double *A, double *img);
int pion_host_project_angle_rule(const pion_gpu_config *cfg, double angle_deg, int trip_limit, int nfields,
                                 const pion_gpu_proj_field *fields, const double *A, double *img, long *ncapped,
                                 double *tan_angle, double *inv_sin);
typedef struct pion_host_snapshot_info {
  double t_start, t_finish, t_sim, min_timestep, last_dt;   /* SimPM.starttime, finishtime, simtime, min_timestep, last_dt */
  double opfreq_time, next_optime;
  int t_step, op_criterion, op_freq;                         /* SimPM.timestep, op_criterion, opfreq */
  int rank, world;                                           /* the writer's */
  int slab_lo, slab_n;                                       /* planes of the slab axis the file holds */
  long data_offset;
  char outfile[256];
} pion_host_snapshot_info;
/* Header of a snapshot: cfg = the GLOBAL configuration (ng, xmin, bc_type of the whole problem).  Host only: needs no
 * device.  Returns EINVAL for a file that is not a complete PIONRAW2 header; sim == NULL here, so the text is in
 * pion_host_sim_last_error(NULL, .). */
int pion_host_snapshot_read_header(const char *path, pion_gpu_config *cfg, pion_host_snapshot_info *info);
/* Restart (dataio->ReadData + sim_init::Init, sim_init.cpp:219-267): checks every header against the sim's own
 * configuration (geometry, equations, nvar, solver, orders, gamma, dx, global extents; EINVAL with a text otherwise),
 * takes the planes this sim owns from whichever of the files hold them -- a run written by M ranks restarts on N --,
 * sets P and Ph, simtime, timestep, last_dt, next_optime, t_start (and finishtime, min_timestep), discards a pending
 * time-step request, and assigns + updates the boundaries.  Inflow and fixed faces capture their state again from the
 * on-grid neighbour, as in the reference's restart.  Wind sources (an evolving one with t_now = the file's t_sim),
 * jets and cooling tables are set up by the caller first, as before pion_host_sim_init; the header only counts them.
 * Never exits: a wrong magic, a missing key, truncated data, planes no file covers, files of different times all
 * return EINVAL and a text. */
int pion_host_sim_read_snapshot(void *sim, const char *const *paths, int npaths);
/* Header of a FITS file of pion_host_sim_write_fits' kind: the outputs of pion_host_snapshot_read_header (the same
 * checks, made by the same function), data_offset = 0.  A primary header without pion_slab_lo / pion_slab_n describes
 * a file that holds the whole slab axis.  Host only.  EINVAL and a text (pion_host_sim_last_error(NULL, .)): not a
 * FITS file, a header without END, a missing key. */
int pion_host_fits_read_header(const char *path, pion_gpu_config *cfg, pion_host_snapshot_info *info);
/* Restart from FITS files (the reference's DataIOFits::ReadData / read_fits_image, dataIO/dataio_fits.cpp:433-548,
 * 865-929): pion_host_sim_read_snapshot's contract word for word -- the same header checks, planes taken from the
 * first file that holds them (M writers, N readers), the same fields of the loop set, a pending time-step request
 * dropped, boundaries assigned and updated, sources and tables set up by the caller first.  What differs is the file:
 * the nvar primitive images are found by EXTNAME, not by position (the derived images Eint / Temp, divB, Ptot are
 * never read; HDUs and cards the reader does not know are skipped by the sizes their headers give), and enter the
 * device as the big-endian bytes the file holds, a chunk of planes at a time (PION_SNAPSHOT_CHUNK_PLANES; host memory
 * is two chunks): pion_gpu_unpack_fits swaps them and multiplies Bx, By, Bz by 1/sqrt(4 pi).  That is a multiplication,
 * as in the reference: a B written and read back need not have the bits it started with; every other variable has.
 * A primitive image a file does not hold is zeros, as in the reference: the call returns 0 and says so in
 * pion_host_sim_last_error.  EINVAL and a text, never an exit: everything pion_host_sim_read_snapshot refuses; a needed
 * image whose BITPIX is not -64 or whose NAXISn are not the header's extents; a data unit that runs past the end of
 * the file; more than five tracers; any element that is not finite or is the reference's null value -1e99 (the text
 * names their number; the state is then what the files held). */
int pion_host_sim_read_fits(void *sim, const char *const *paths, int npaths);
/* SimTime of the loop: out[0..5] = simtime, last_dt, next_optime, finishtime, starttime, (double) timestep */
int pion_host_sim_get_time(void *sim, double *out6);

/* ---- slab communicators (both return a pion_host::slab_comm*).  A grid is cut along its slab axis, the last one:
 * z of a 3-D grid, y of a 2-D grid (Cartesian or cylindrical (z,R)).  periodic_z: the global problem is periodic along the slab
 * axis (rank 0 <-> world-1 exchange); physical faces of the slab axis apply on the end ranks only. */
int pion_host_comm_unique_id(void *out128);                   /* ncclGetUniqueId on rank 0 */
int pion_host_comm_create(int rank, int world, int periodic_z, const void *unique_id, int device, void **comm);   /* RCCL */
int pion_host_comm_shm_create(int rank, int world, int periodic_z, const char *name, const struct pion_backend *backend,
                              void **comm);                   /* host-staged: POSIX shared memory "/name" */
void pion_host_comm_destroy(void *comm);
int pion_host_comm_attach(void *comm, void *gpu_handle);
int pion_host_comm_start(void *comm, int which);
int pion_host_comm_finish(void *comm);
int pion_host_comm_allreduce_min(void *comm, double *t_dyn, double *t_mp);
int pion_host_comm_last_error(void *comm, char *buf, int len);

/* ---- cooling tables of mp_only_cooling (EP.cooling = 8): T[nT], tabs[5][nT] = {rrhp, C_rrh, C_ffhe, C_fbdn, C_cie},
 * slopes[5][nT]; and the three spline-backed rate curves they are built from */
int pion_host_build_cooling_tables(double min_temp, double max_temp, int nT, double *T, double *tabs, double *slopes);
double pion_host_cooling_rate_wss09(double T);
double pion_host_hii_rrr(double T);
double pion_host_hii_total_cooling(double T);

/* ---- a total-CIE cooling curve supplied by the caller (EP.cooling = 4..7; pion_gpu_set_cooling_curve): knots
 * (log10 T, log10 Lambda), 2 <= n <= 256, strictly increasing in log10 T, not necessarily uniform.
 * build: the natural-spline second-derivative coefficients c_out[n] (GSL's cspline representation), what
 *   cooling_function_SD93CIE's set-up leaves in its spline (microphysics/cooling_SD93_cie.cpp:150-166, 611-627).
 * set / rate: a process-global curve and cooling_function_SD93CIE::cooling_rate_SD93CIE on it (:666-704):
 *   HUGE_VAL for T < 0 or non-finite T, linear extrapolation in log-log space with min_slope below and max_slope
 *   above the knots, the spline inside, exp(ln10 s).  The reference's slopes: 8.0 below, the slope of the last
 *   interval above (:160-164, 621-625).
 * read: a text file of two columns (log10 T, log10 Lambda), '#' starts a comment; -1 and a message in err for a file
 *   that cannot be opened, a malformed line, fewer than 2 or more than min(max_n, 256) knots, unsorted knots. */
int pion_host_build_cooling_curve(int n, const double *logT, const double *logL, double *c_out);
int pion_host_cooling_curve_set(int n, const double *logT, const double *logL, double min_slope, double max_slope);
double pion_host_cooling_curve_rate(double T);
int pion_host_read_cooling_curve(const char *path, int max_n, double *logT, double *logL, int *n, char *err, int errlen);

/* ---- stellar_wind_evolution::read_evolution_file (grid/stellar_wind_BC.cpp:1026-1100): two header lines, then rows
 * of 8 or 15 columns (time M L Teff Mdot vrot vcrit vinf [X_H X_He X_C X_N X_O X_Z X_D], cgs); a column a row lacks
 * keeps the previous row's value (0 at first), as sscanf leaves it untouched; lines without any number are skipped.
 * Writes table[col * cap + row] for the PION_WND_* columns, with time = (t + time_offset) / t_scalefac and
 * R = sqrt(L / (4 pi sigma Teff^4)); table == NULL: count only.  Returns the number of rows, or < 0. */
#define PION_WND_TIME 0
#define PION_WND_M 1
#define PION_WND_L 2
#define PION_WND_TEFF 3
#define PION_WND_MDOT 4
#define PION_WND_VROT 5
#define PION_WND_VCRIT 6
#define PION_WND_VINF 7
#define PION_WND_X 8      /* 8..14: X_H X_He X_C X_N X_O X_Z X_D */
#define PION_WND_R 15
#define PION_WND_NCOL 16
long pion_host_read_wind_evolution(const char *path, double time_offset, double t_scalefac, long cap, double *table);

/* the product's only backend table: libpion_gpu.so */
const struct pion_backend *pion_backend_gpu(void);

#ifdef __cplusplus
}
#endif
#endif /* PION_HOST_H */
