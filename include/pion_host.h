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
