// pion_backend.h -- the calls the host time loop (sim_control_gpu) and the staged slab transport
// (slab_comm_shm) make below themselves, as a table of function pointers.
//
// The product has ONE implementation: pion_backend_gpu(), bound to the C-ABI of libpion_gpu.so
// (include/pion_gpu.h) -- there is no CPU implementation in the product.  The table exists so that the C++ time
// loop and its transport can be rehearsed where no GPU is (tests/native/orc_backend.cpp binds it to the test
// oracle for the world_size-2 CPU test), the way the reference's sim_control is written against the virtual
// FV_solver_base / GridBaseClass interfaces rather than one concrete class.
#ifndef PION_BACKEND_H
#define PION_BACKEND_H

#include "../../include/pion_gpu.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct pion_backend {
  const char *name;
  int (*create)(const pion_gpu_config *cfg, int device, void **handle);
  void (*destroy)(void *handle);
  int (*last_error)(void *handle, char *buf, int len);
  int (*upload)(void *handle, const double *P_soa);
  int (*download)(void *handle, int which, double *P_soa);
  int (*update_bcs)(void *handle, double simtime, int cstep, int maxstep, int assign);
  int (*stage)(void *handle, double dt_stage, int space_ooa, int is_full_step);
  int (*stage_part)(void *handle, double dt_stage, int space_ooa, int is_full_step, int part);
  int (*set_glm_speeds)(void *handle, double dt, double dx, double cr);
  /* time step: calc_dt = reduce and read back now; dt_begin / dt_wait = the same, split so that the read-back of
   * the minima a full-step stage left behind overlaps the boundary update that follows it */
  int (*calc_dt)(void *handle, double *t_dyn, double *t_mp);
  int (*dt_begin)(void *handle);
  int (*dt_wait)(void *handle, double *t_dyn, double *t_mp);
  /* z-slab halos through host memory (staged transports).  One face = nvar runs of halo_count()/nvar doubles
   * (the nbc planes next to the face, full x-y extent, variable slowest).
   *   halo_to_host_begin: start copying the ON-GRID planes next to the ZN face (lo) and / or the ZP face (hi) of
   *                       array `which` (0 = P, 1 = Ph) into host buffers (either may be null); returns at once
   *   halo_to_host_end:   the host buffers are complete
   *   halo_from_host:     copy host buffers into the GHOST planes of the ZN (lo) / ZP (hi) face; the z-boundary
   *                       part of the next stage is ordered after it (the host buffers may be reused on return) */
  long (*halo_count)(void *handle);
  int (*halo_to_host_begin)(void *handle, int which, double *lo, double *hi);
  int (*halo_to_host_end)(void *handle);
  int (*halo_from_host)(void *handle, int which, const double *lo, const double *hi);
  /* Snapshots (snapshot_io.h): the ON-GRID cells of planes [plane_lo, plane_hi) of the slab axis, all variables, as
   * [nvar][planes][ny][nx] (pion_gpu_pack_ongrid's layout), streamed through two staging slots (0, 1) the backend owns,
   * so that a write or a read keeps two chunks on the host whatever the grid.  All four NULL (a table initialised
   * before they existed): the snapshot code takes the whole array through download / upload and strips / embeds the
   * ghost cells on the host.
   *   ongrid_count:         doubles of a chunk of `planes` planes
   *   ongrid_to_host_begin: start copying the planes of array `which` into staging slot `slot`; returns at once
   *   ongrid_to_host_end:   slot `slot` has arrived; *host = its buffer, valid until the slot's next _begin
   *   ongrid_from_host:     wait until slot `slot` is free, have fill(ctx, buffer) write the planes into its host
   *                         buffer (non-zero: give up and return it), then start copying them into P and Ph (ghost
   *                         cells untouched); returns without waiting for the copy -- the boundary update that
   *                         follows is ordered after it */
  long (*ongrid_count)(void *handle, int planes);
  int (*ongrid_to_host_begin)(void *handle, int which, int plane_lo, int plane_hi, int slot);
  int (*ongrid_to_host_end)(void *handle, int slot, const double **host);
  int (*ongrid_from_host)(void *handle, int plane_lo, int plane_hi, int slot, int (*fill)(void *ctx, double *host),
                          void *ctx);
  /* FITS output (fits_io.h): the images of planes [plane_lo, plane_hi) as [nimage][planes][ny][nx], every element
   * already big-endian (pion_gpu_pack_fits' layout), through the same two staging slots.  Both NULL (a table
   * initialised before they existed): the writer takes array 0 through download and evaluates the images on the host.
   *   fits_count:         elements (8 bytes each) of a chunk of `planes` planes
   *   fits_to_host_begin: start packing and copying the planes into staging slot `slot`; returns at once.  Arrival
   *                       is ongrid_to_host_end's */
  long (*fits_count)(void *handle, int planes);
  int (*fits_to_host_begin)(void *handle, int plane_lo, int plane_hi, int slot);
  /* FITS input (fits_io.h): the nvar primitive images of planes [plane_lo, plane_hi) as [nvar][planes][ny][nx], every
   * element big-endian as the file holds it (pion_gpu_unpack_fits' layout), through the same two staging slots.  These
   * two entries are read ONLY inside sim_control_gpu::read_fits: a caller that never restarts from a FITS file may
   * hand the loop a table that ends before them.  Both NULL: the reader takes the images whole, converts them on the
   * host and goes through upload.
   *   fits_from_host:   ongrid_from_host's contract -- wait until slot `slot` is free, have fill(ctx, buffer) write
   *                     the chunk's bytes into its host buffer (non-zero: give up and return it), start the copy and
   *                     the unpack into P and Ph (B rescaled, ghost cells untouched); returns without waiting
   *   fits_read_status: wait for the unpacks; *nbad = elements that were not finite or the reference's null value
   *                     since the last call (pion_gpu_unpack_fits_status) */
  int (*fits_from_host)(void *handle, int plane_lo, int plane_hi, int slot, int (*fill)(void *ctx, double *host),
                        void *ctx);
  int (*fits_read_status)(void *handle, long *nbad);
  /* Projected images (projection_io.cpp; the rules: pion_amd/csrc/dev_project.h): the images of pion_gpu_project, native
   * doubles [nfields][NJ][NI].  These two entries are read ONLY inside sim_control_gpu::write_projection: a caller
   * that never writes a projection may hand the loop a table that ends before them.  Both NULL: the writer takes
   * array 0 through download and runs dev_project.h's functions in a host loop.
   *   project_count:   doubles of one call, < 0 for a configuration pion_gpu_project refuses (text in last_error)
   *   project_to_host: project array P on the device and copy the images into `host`; complete on return */
  long (*project_count)(void *handle, int axis, int nfields);
  int (*project_to_host)(void *handle, int axis, int nfields, const pion_gpu_proj_field *fields, double *host);
  /* A rank's part of a slab run's image (dev_project.h, "parts"; pion_gpu_project_part).  These two entries are read
   * ONLY inside sim_control_gpu::write_projection of a sim that is one rank of a slab run: any other caller may hand the
   * loop a table that ends before them.  Both NULL: the writer takes array 0 through download and runs dev_project.h's
   * part functions in a host loop.
   *   project_part_count:   doubles of the image of the WHOLE domain, < 0 for what pion_gpu_project_part refuses
   *   project_part_to_host: `host` holds the image as the rank below left it (rank 0: zeros); copy it to the device,
   *                         run this rank's part on array P, copy it back; complete on return */
  long (*project_part_count)(void *handle, int axis, int nfields, const pion_gpu_proj_part *part);
  int (*project_part_to_host)(void *handle, int axis, int nfields, const pion_gpu_proj_field *fields,
                              const pion_gpu_proj_part *part, double *host);
  /* Ray-traced column densities (columns_io.cpp; the rules: pion_amd/csrc/dev_raytrace.h).  These four entries are read ONLY
   * inside sim_control_gpu::add_rt_source and write_columns: a caller that never adds a radiation source may hand the
   * loop a table that ends before them.  All NULL: the sim keeps the sources itself, and the writer takes array 0
   * through download and runs pion_gpu_raytrace_host on it.
   *   add_rt_source:         pion_gpu_add_rt_source
   *   raytrace:              pion_gpu_raytrace: trace every source from array `which`; enqueued
   *   rt_count:              doubles of `planes` planes of one column array
   *   columns_to_host_begin: start packing (big-endian, pion_gpu_pack_columns) and copying the planes of array `what`
   *                          (0 col, 1 dcol) of source `id` into staging slot `slot`; returns at once.  Arrival is
   *                          ongrid_to_host_end's */
  int (*add_rt_source)(void *handle, const pion_gpu_rt_source *src, int *id, double *pos_used);
  int (*raytrace)(void *handle, int which);
  long (*rt_count)(void *handle, int planes);
  int (*columns_to_host_begin)(void *handle, int id, int what, int plane_lo, int plane_hi, int slot);
  /* The ray tracer of a slab run (dev_raytrace.h, "a part"; pion_gpu_add_rt_source_part, pion_gpu_raytrace_part).  These
   * two entries are read ONLY inside add_rt_source and write_columns of a sim that is one rank of a slab run: any other
   * caller may hand the loop a table that ends before them.  Both NULL: the sim keeps the sources itself, and the
   * writer takes array 0 through download and runs pion_gpu_raytrace_host_part on it.
   *   add_rt_source_part:   pion_gpu_add_rt_source_part
   *   raytrace_part_faces:  the plane received travels host -> device (face_in; NULL where the source's chain hands this
   *                         rank none), source `id` is traced from array `which`, the rank's lowest and highest own
   *                         plane of col travel device -> host (face_lo, face_hi; either may be NULL); each
   *                         rt_count(handle, 1) doubles; complete on return */
  int (*add_rt_source_part)(void *handle, const pion_gpu_rt_source *src, const pion_gpu_rt_part *part, int *id,
                            double *pos_used);
  int (*raytrace_part_faces)(void *handle, int which, int id, const double *face_in, double *face_lo, double *face_hi);
  /* The inclined projection of a (z,R) grid (projection_io.cpp; the rule: pion_amd/csrc/dev_project_angle.h;
   * pion_gpu_project_angle).  These two entries are read ONLY inside sim_control_gpu::write_projection_angle: any
   * other caller may hand the loop a table that ends before them.  Both NULL: the writer takes array 0 through
   * download and runs the rule in a host loop.
   *   project_angle_count:   pion_gpu_project_angle_count
   *   project_angle_to_host: project array P on the device, copy the images into `host`, wait; *ncapped = the pixels
   *                          whose ray loop reached the trip limit (pion_gpu_project_angle_status) */
  long (*project_angle_count)(void *handle, double angle_deg, int nfields, int *n_extra);
  int (*project_angle_to_host)(void *handle, double angle_deg, int nfields, const pion_gpu_proj_field *fields, double *host,
                               long *ncapped);
} pion_backend;

/* the product's backend: libpion_gpu.so */
const pion_backend *pion_backend_gpu(void);

#ifdef __cplusplus
}
#endif
#endif
