/*
 * pion_gpu.h -- C-ABI of libpion_gpu.so: the MI355X (gfx950) replacement for
 * PION's finite-volume flux-update hot path.
 *
 * Every entry point is stage-granular: it replaces one of the loops that the
 * reference's time_integrator / calc_timestep run cell-by-cell through the
 * virtual FV_solver_base interface.  The reference interface each function
 * replaces is cited as file:line relative to the PION source tree (source/).
 *
 * Conventions (mirroring the reference):
 *   - pion_flt is double (defines/functionality_flags.h: PION_DATATYPE_DOUBLE).
 *   - primitive vector P = {RO,PG,VX,VY,VZ,BX,BY,BZ,SI,tracers...},
 *     conserved U = {RHO,ERG,MMX,MMY,MMZ,BBX,BBY,BBZ,PSI,...}  (constants.h:256-281).
 *   - all functions return 0 on success or a negative PION_GPU_E* code; they
 *     never exit().  Fatal physics conditions of the reference (rep.error ->
 *     exit(1), tools/reporting.h:57-70) come back as PION_GPU_EPHYSICS and a
 *     text from pion_gpu_last_error().
 *   - host arrays are owned by the caller, device memory by the handle.
 *   - a handle is not thread-safe (like the reference's solver object,
 *     solver_eqn_base.h:52), distinct handles may be used from distinct threads.
 *
 * Grid layout handed over the boundary ("SoA"): double [nvar][nz_all][ny_all][nx_all],
 * x fastest, including nbc ghost cells on every used axis, i.e. the order in
 * which UniformGrid numbers its cells (grid/uniform_grid.cpp:482-636, id =
 * ix + nx_all*(iy + ny_all*iz) counted from the most negative ghost corner),
 * with the state-vector index as the slowest index.  Unused axes have extent 1
 * and no ghosts.
 */
#ifndef PION_GPU_H
#define PION_GPU_H

#ifdef __cplusplus
extern "C" {
#endif

#define PION_MAX_NVAR 16
#define PION_MAX_DIM 3

/* equation types (constants.h:163-170) */
#define PION_EQEUL 1
#define PION_EQMHD 2
#define PION_EQGLM 3

/* flux solvers (constants.h:238-246) */
#define PION_FLUX_LF 0
#define PION_FLUX_RSlinear 1
#define PION_FLUX_RSexact 2
#define PION_FLUX_RShybrid 3
#define PION_FLUX_RSroe 4
#define PION_FLUX_RSroe_pv 5
#define PION_FLUX_FVS 6
#define PION_FLUX_RS_HLLD 7
#define PION_FLUX_RS_HLL 8

/* artificial viscosity (constants.h:321-326) */
#define PION_AV_NONE 0
#define PION_AV_FKJ98_1D 1
#define PION_AV_HCORRECTION 3
#define PION_AV_HCORR_FKJ98 4

/* boundary types handled on the device (boundaries/boundaries.h) */
#define PION_BC_PERIODIC 1
#define PION_BC_OUTFLOW 2
#define PION_BC_INFLOW 3
#define PION_BC_REFLECTING 4
#define PION_BC_FIXED 5
#define PION_BC_ONEWAY_OUT 6
#define PION_BC_DMACH 7   /* YP boundary of the double Mach reflection test */
#define PION_BC_DMACH2 8  /* internal: fixed post-shock state in y<0, x<=1/6 */
#define PION_BC_STWIND 9  /* internal: stellar-wind cells (fixed per-cell state) */
#define PION_BC_SLAB 10   /* face of the slab axis owned by a neighbouring GPU (halo exchange).  The slab axis is the
                           * last axis: faces 4, 5 (ZN, ZP) of a 3-D grid, faces 2, 3 (YN, YP) of a 2-D grid, Cartesian
                           * or cylindrical (z,R); on any other face, and on a 1-D grid, pion_gpu_create returns EINVAL.
                           * A cylindrical slab other than the lowest has SLAB at YN and no axis. */
#define PION_BC_JET 11    /* internal: jet inflow cells on the XN face (pion_gpu_set_jet) */
#define PION_BC_JETREFLECT 13   /* reflecting wall behind a jet: v_n and the TANGENTIAL field change sign
                                 * (jetreflect_boundaries.cpp:32-62) */
#define PION_BC_AXISYMMETRIC 12 /* R = 0 axis of a cylindrical (z,R) grid, face YN only (axisymmetric_boundaries.cpp) */

/* cooling functions of mp_only_cooling (microphysics/mp_only_cooling.h) */
#define PION_COOL_NONE 0
#define PION_COOL_KI02 2                     /* Koyama & Inutsuka (2002): no table, no curve */
#define PION_COOL_SD93_CIE 4                 /* 4..7: a total-CIE curve the caller supplies, pion_gpu_set_cooling_curve */
#define PION_COOL_SD93_PLUS_HEATING 5
#define PION_COOL_WSS09_CIE_PLUS_HEATING 6
#define PION_COOL_WSS09_CIE_ONLY_COOLING 7
#define PION_COOL_WSS09_CIE_LINE_HEAT_COOL 8 /* tables, pion_gpu_set_cooling_tables */
/* (3, Dalgarno & McCray: mp_only_cooling::Edot has no case for it and stops, mp_only_cooling.cpp:410-412 -- EINVAL) */

/* cell flag bits (grid/cell_interface.h:83-121) */
#define PION_CELL_ISGD 1
#define PION_CELL_ISBD 2
#define PION_CELL_ISDOMAIN 4
#define PION_CELL_TIMESTEP 8
#define PION_CELL_ISLEAF 16

/* error codes */
#define PION_GPU_OK 0
#define PION_GPU_EINVAL (-1)   /* bad argument / unsupported configuration */
#define PION_GPU_EDEVICE (-2)  /* HIP runtime error */
#define PION_GPU_EPHYSICS (-3) /* negative density etc. (reference: rep.error) */
#define PION_GPU_ENOMEM (-4)

/*
 * The subset of SimParams (sim_params.h:200-285) the hot path reads.
 */
typedef struct pion_gpu_config {
  int ndim;      /* SimParams::ndim */
  int nvar;      /* SimParams::nvar (includes tracers) */
  int ntracer;   /* SimParams::ntracer; tracers are the last ntracer variables */
  int eqntype;   /* PION_EQ* */
  int solver;    /* SimParams::solverType, PION_FLUX_* */
  int artvisc;   /* SimParams::artviscosity, PION_AV_* */
  int sp_ooa;    /* SimParams::spOOA */
  int tm_ooa;    /* SimParams::tmOOA */
  int coord_sys; /* 1 = Cartesian; 2 = cylindrical (z,R), 2-D axisymmetric: x axis = z, y axis = R
                  * (coord_sys/VectorOps.cpp:662-1245 and the cyl_FV_solver_* classes); 3 = spherical
                  * symmetry, 1-D, Euler only (VectorOps_spherical.cpp, sph_FV_solver_Hydro_Euler) */
  int nbc;       /* ghost depth, SimParams::Nbc (2 for second order) */
  int ng[PION_MAX_DIM];      /* on-grid cells per axis (1 on unused axes) */
  double xmin[PION_MAX_DIM]; /* physical position of the low corner of the ON-GRID region */
  double dx;                 /* cell size */
  double gamma;              /* SimParams::gamma */
  double cfl;                /* SimParams::CFL */
  double etav;               /* SimParams::etav */
  double min_temp;           /* EP.MinTemperature */
  double max_temp;           /* EP.MaxTemperature */
  double refvec[PION_MAX_NVAR]; /* SimParams::RefVec */
  int bc_type[6];            /* PION_BC_* for XN,XP,YN,YP,ZN,ZP (0 on unused axes) */
  int bc_dmach2;             /* 1: internal DMR2 boundary active */
  int cooling;               /* EP.cooling (PION_COOL_*), 0 = no microphysics object */
  int mp_timestep_limit;     /* EP.MP_timestep_limit: 0 none; 1,2,3 cooling time; 4 none (recombination only); else EINVAL */
  int strict_fp;             /* 1: kernels built without FMA contraction (bit-parity build) */
} pion_gpu_config;

/* ---- lifetime --------------------------------------------------------- */

/* setup_fixed_grid::set_equations (grid/setup_fixed_grid.cpp:1067-1191) +
 * setup_grid (:161-245): creates solver state and device arrays on `device`. */
int pion_gpu_create(const pion_gpu_config *cfg, int device, void **handle);
void pion_gpu_destroy(void *handle);
int pion_gpu_last_error(void *handle, char *buf, int len);

/* total cells including ghosts, and extents with ghosts */
long pion_gpu_ncell_all(void *handle);
int pion_gpu_ng_all(void *handle, int axis);

/* ---- state transfer ---------------------------------------------------- */

/* dataio->ReadData + "Ph=P" (sim_control/sim_init.cpp:219-241): copies a host
 * SoA array into P and Ph.  Ghost values in the input are ignored once
 * pion_gpu_update_bcs has run. */
int pion_gpu_upload(void *handle, const double *P_soa);
/* which = 0: P, 1: Ph */
int pion_gpu_download(void *handle, int which, double *P_soa);
/* The on-grid cells of planes [plane_lo, plane_hi) of the slab axis (the last axis: x-y planes of a 3-D grid, rows of
 * a 2-D grid; a 1-D grid has the one "plane" [0, 1), its row), for all variables, as a contiguous DEVICE buffer
 * [nvar][planes][ny][nx] (2-D: [nvar][planes][nx]; 1-D: [nvar][nx]) of pion_gpu_ongrid_count(handle, planes) doubles
 * -- what dataio's writers visit with FirstPt / NextPt (no ghost cells), a chunk of planes at a time, so that a
 * snapshot never needs a host array of the whole grid (pion_host_sim_write_snapshot streams through these).
 *   pion_gpu_pack_ongrid    copies from the array pion_gpu_download(which) reads; enqueued on the compute stream,
 *                           returns at once (synchronise, or order a copy on that stream, before reading dbuf).
 *   pion_gpu_unpack_ongrid  the reverse, into BOTH P and Ph as pion_gpu_upload does; ghost cells and other planes keep
 *                           their bits; discards what upload discards (cached time step, a requested read-back, the
 *                           HLL-screen summary).  Between steps only; a boundary update with assign != 0 must follow.
 * Cell ids and buffer indices are 64-bit.  EINVAL: a range outside [0, planes of the grid], an empty one, NULL dbuf. */
long pion_gpu_ongrid_count(void *handle, int planes);
int pion_gpu_pack_ongrid(void *handle, int which, int plane_lo, int plane_hi, void *dbuf);
int pion_gpu_unpack_ongrid(void *handle, int plane_lo, int plane_hi, void *dbuf);
/* FITS output (pion_amd/csrc/dev_output.h states the rules; the reference's dataio_fits::OutputData,
 * dataIO/dataio_fits.cpp:147-320): the images of planes [plane_lo, plane_hi) as a contiguous DEVICE buffer
 * [nimage][planes][ny][nx] (2-D: [nimage][planes][nx]; 1-D: [nimage][nx]) of pion_gpu_fits_count(handle, planes)
 * elements.  Images: the primitive variables in state order (GasDens GasPres GasVX GasVY GasVZ [Bx By Bz [psi]] TR0 ..),
 * then Eint = p/(gamma-1)/rho (no microphysics) or Temp = p Mu_tot_over_kB / rho (cooling != 0), then for MHD and GLM
 * divB (centred differences; d(R B_R)/(R dR) between the neighbours' centres of mass on a cylindrical grid) and
 * Ptot = p + 0.5 B^2.  Bx, By, Bz and divB are multiplied by sqrt(4 pi) (the reference's NEW_B_NORM); psi and Ptot
 * are not.  Every element is the IEEE-754 double ALREADY BYTE-SWAPPED to big-endian: a FITS writer stores the bytes
 * as they arrive.  Both floating-point builds give the same bits.
 *   pion_gpu_pack_fits    packs from array P only; enqueued on the compute stream, returns at once.  divB reads the
 *                         2 ndim neighbours of B, ghost cells and ghost planes included: they hold whatever the last
 *                         pion_gpu_update_bcs (and halo exchange) left, so call it after the boundary update.
 *   pion_gpu_fits_images  the image list (names: NUL-padded, may be NULL) without a device call.
 * EINVAL: more than five tracers (as the reference), a plane range outside the grid or empty, NULL dbuf. */
int pion_gpu_fits_images(void *handle, char names[][16], int *n);
long pion_gpu_fits_count(void *handle, int planes);
int pion_gpu_pack_fits(void *handle, int plane_lo, int plane_hi, void *dbuf);
/* FITS input, the same rules run backwards (dev_output.h; the reference's DataIOFits::ReadData / read_fits_image,
 * dataIO/dataio_fits.cpp:433-548, 865-929): the nvar PRIMITIVE images of the list above -- the derived ones are never
 * read -- of planes [plane_lo, plane_hi) as a contiguous DEVICE buffer [nvar][planes][ny][nx] of
 * pion_gpu_fits_prim_count(handle, planes) elements, every element the big-endian double as the file holds it.
 *   pion_gpu_unpack_fits         swaps each element to a native double, multiplies Bx, By, Bz by 1/sqrt(4 pi) (a
 *                                multiplication as in the reference: a B written and read back need not have the bits
 *                                it started with; psi is not scaled) and stores it into the on-grid cell of BOTH P and
 *                                Ph.  Ghost cells and other planes keep their bits.  Enqueued on the compute stream,
 *                                returns at once; discards what pion_gpu_upload and pion_gpu_unpack_ongrid discard.
 *                                Between steps only; a boundary update with assign != 0 must follow.  An element that
 *                                is not finite, or that constants::equalD(x, -1.e99) holds for (the reference's null
 *                                value), is stored all the same and counted in a device counter of the handle.
 *   pion_gpu_unpack_fits_status  synchronises, returns the number of such elements since the last call and clears it.
 * Both floating-point builds give the same bits.  EINVAL as for pion_gpu_pack_fits. */
long pion_gpu_fits_prim_count(void *handle, int planes);
int pion_gpu_unpack_fits(void *handle, int plane_lo, int plane_hi, const void *dbuf);
int pion_gpu_unpack_fits_status(void *handle, long *nbad);
/* Projected images (pion_amd/csrc/dev_project.h states the rules): up to PION_PROJ_MAX_FIELDS fields
 * coef rho^a T^b w per call, a in {0, 1, 2} by multiplication, w = 1 (var < 0) or primitive variable `var`,
 * T = p Mu_tot_over_kB / rho (the Temp image's rule), T^b = exp(b log T), skipped for b == 0.
 *   3-D Cartesian, axis 0, 1, 2 (line of sight along x, y, z): the image value is (sum of the field over the on-grid
 *     cells of the column) dx, the additions in the fixed order dev_project.h states (y, z: increasing index; x: 64
 *     partial sums of every 64th cell, then a pairwise tree), whatever the launch geometry.  The image axes are the
 *     two remaining axes in grid order: element [j][i] has i on the lower-numbered one.
 *   2-D cylindrical (z,R), axis PION_PROJ_AXIS_PERP (line of sight perpendicular to the symmetry axis): the reference's
 *     calc_projection_column (analysis/projection/perp_projection.cpp:404-487) as written, with the slopes of :338-390,
 *     one ray per cell (z_i, impact parameter b_j = R_j): the image is [NR][NZ], z fastest (:236).
 * pion_gpu_project writes [nfields][NJ][NI] native-endian doubles, pion_gpu_project_count(handle, axis, nfields) of
 * them, into the DEVICE buffer dbuf from array `which` (0 = P, 1 = Ph); enqueued on the compute stream, returns at once.
 * Only on-grid cells are read.  Both floating-point builds give the same bits.  `name` (NUL-terminated, 1 to 15
 * printable characters, no quote) becomes the image's EXTNAME in pion_host_sim_write_projection's file.
 * pion_gpu_project_count returns < 0, and both EINVAL with a text, for: 1-D, spherical and 2-D Cartesian grids; a line
 * of sight along the axis of a cylindrical grid (or any axis but PION_PROJ_AXIS_PERP there); PION_PROJ_AXIS_PERP on a
 * Cartesian grid; NR == 1; nfields outside 1 .. 8; a outside {0, 1, 2}; var >= nvar; a name that is empty, not
 * terminated or not printable; coef or b not finite; b != 0 on a handle with cooling == 0 (it has no temperature). */
#define PION_PROJ_MAX_FIELDS 8
#define PION_PROJ_AXIS_PERP 3
typedef struct pion_gpu_proj_field {
  char name[16];
  int a;          /* power of rho: 0, 1, 2 */
  int var;        /* < 0: w = 1; else w = primitive variable var */
  double coef, b; /* b: power of T */
} pion_gpu_proj_field;
long pion_gpu_project_count(void *handle, int axis, int nfields);
int pion_gpu_project(void *handle, int which, int axis, int nfields, const pion_gpu_proj_field *fields, void *dbuf);
/* The same images of a slab-decomposed run, the sums carried from rank to rank (dev_project.h, "parts"): this handle
 * holds the planes [plane_lo, plane_lo + n) of the slab axis (z in 3-D, R in (z,R); n = the handle's own ng of that axis)
 * out of global_planes.  dimg is the image of the WHOLE domain, [nfields][NJ_global][NI_global] doubles in DEVICE memory,
 * pion_gpu_project_part_count of them: in/out.  Rank 0 starts from +0.0 everywhere; every rank runs its part on what
 * the rank below left, in increasing rank; after the rank with last = 1 the image is == pion_gpu_project on one handle
 * of the whole domain.  3-D along z: the running sums are continued, only `last` multiplies by dx.  3-D along x, y: the
 * rank's own rows are written at row offset plane_lo, the others are left as they are.  (z,R): every impact row below
 * the rank's upper edge gains the segments of the rank's own rows; the geometry takes global row indices and
 * global_xmin, the R origin of the whole grid; the slope of the rank's last own row reads the first upper slab ghost
 * row of the array (the halo exchange has filled it), no other ghost cell is read; only `last` finishes.
 * Enqueued on the compute stream, returns at once.  A part with plane_lo = 0, global_planes = n, last = 1 on a buffer of
 * +0.0 is == pion_gpu_project.  EINVAL and a text: everything pion_gpu_project refuses; plane_lo < 0; plane_lo + n >
 * global_planes; a global_xmin that is not finite; a null part or buffer. */
typedef struct pion_gpu_proj_part {
  int plane_lo, global_planes, last;
  double global_xmin;
} pion_gpu_proj_part;
long pion_gpu_project_part_count(void *handle, int axis, int nfields, const pion_gpu_proj_part *part);
int pion_gpu_project_part(void *handle, int which, int axis, int nfields, const pion_gpu_proj_field *fields,
                          const pion_gpu_proj_part *part, void *dimg);
/* A 2-D cylindrical (z,R) grid seen at an angle to its symmetry axis (pion_amd/csrc/dev_project_angle.h states the rule):
 * the reference's analysis/projection/angle_projection.cpp as written -- per pixel the ray, a hyperbola in the (z,R)
 * plane, is walked from cell to cell (get_start_of_ray, get_entry_exit_points, generate_angle_image) and every field
 * gains weight * (its value at the cell), weight = |sqrt(R_entry^2 - b^2) - sqrt(R_exit^2 - b^2)| / sin(angle).
 * angle_deg: the angle between the line of sight and the axis, finite, 0 < angle_deg < 90; tan and 1 / sin of it are
 * evaluated once on the host.  n_extra = (int) fabs(Xmax[R] / tan(angle) / dx) columns are added at each end in z:
 * NI = NZ + 2 n_extra, NJ = NR, pixel (i, j) centred at z = Xmin[Z] + (i - n_extra + 0.5) dx, R = Xmin[R] + (j + 0.5) dx;
 * the image's pixels are dx sin(angle) wide on the sky.  The fields are pion_gpu_project's.
 *   pion_gpu_project_angle_count   doubles of one call, nfields NR NI; *n_extra (may be null) receives n_extra
 *   pion_gpu_project_angle         writes [nfields][NR][NI] native-endian doubles into the DEVICE buffer dbuf from array
 *                                  `which`; enqueued on the compute stream, returns at once.  Only on-grid cells are read.
 *                                  Both floating-point builds give the same bits, and the bits of
 *                                  pion_host_project_angle_on_host wherever the fields have b == 0.
 *   pion_gpu_project_angle_status  synchronises; *ncapped = the pixels since the last call one of whose ray loops reached
 *                                  the rule's limit of 2 (NZ + NR) + 8 trips before its end (none is expected: such an
 *                                  image is not to be used), and clears the count.
 * The count returns < 0, and both EINVAL with a text, for: every grid that is not 2-D cylindrical; NR == 1; a handle
 * with a PION_BC_SLAB face (rays are not carried from rank to rank); an angle that is not finite or outside (0, 90) -- 90
 * is PION_PROJ_AXIS_PERP's --; nfields NR NI above 2^31 - 1 (small angles); every field pion_gpu_project refuses; a null
 * buffer. */
long pion_gpu_project_angle_count(void *handle, double angle_deg, int nfields, int *n_extra);
int pion_gpu_project_angle(void *handle, int which, double angle_deg, int nfields, const pion_gpu_proj_field *fields, void *dbuf);
int pion_gpu_project_angle_status(void *handle, long *ncapped);
/* Ray-traced column densities (pion_amd/csrc/dev_raytrace.h states the rules): the reference's short-characteristics
 * tracer raytracer_USC (raytracing/raytracer_SC.cpp), which leaves per cell and source the column density TO the cell and
 * the column THROUGH it in extra_data.  Here, per source, two arrays of the ON-GRID cells only, [nz][ny][nx] doubles:
 *   col   what CI.get_col returns after a trace: column to the cell + column through it (the reference's Col_Src_<id>_T0)
 *   dcol  the column through the cell, ds rho, ds rho (1 - y) or ds rho y with y = tracer opacity_var (ProcessCell, :855-1057)
 * 2-D Cartesian, 2-D cylindrical (z,R) (the reference runs the same cell_cols_2d there) and 3-D Cartesian grids; a
 * finite source anywhere, on or off the grid, or a source at infinity beyond one of the 2 ndim faces.  Both
 * floating-point builds give the same bits.  Tracing only reads the state: a step after it is the step without it.
 *   pion_gpu_add_rt_source  Add_Source / add_source_to_list (:1183-1314): moves a finite source to the nearest cell
 *                           vertex per axis (centre_source_on_cell, :1934-1996) and reports the position used
 *                           (pos_used, PION_MAX_DIM doubles, may be NULL); *id = 0, 1, ...  Allocates the source's two
 *                           arrays.  PION_RT_KERNEL=levels in the environment at the handle's first source selects the
 *                           launch-per-level kernel for finite sources (a cross-check; default: tiles).
 *   pion_gpu_raytrace       RT_all_sources (sim_control/sim_init.cpp:806-829): every source in id order, from array
 *                           `which` (0 = P, 1 = Ph; what pion_gpu_download(which) reads); enqueued on the compute
 *                           stream, returns at once.  A handle without sources launches nothing.
 *   pion_gpu_rt_columns     CI.get_col / get_cell_col: `what` = 0 col, 1 dcol of source id into a host array of
 *                           pion_gpu_rt_count(handle, all planes) doubles; synchronises.
 *   pion_gpu_rt_count       doubles of `planes` planes of the slab axis (x-y planes in 3-D, rows in 2-D) of one array
 *   pion_gpu_pack_columns   the planes [plane_lo, plane_hi) of that array as big-endian doubles in the DEVICE buffer
 *                           dbuf, as pion_gpu_pack_fits packs an image; enqueued, returns at once.
 *   pion_gpu_rt_plan        host only, no device: the tile of the tiled kernel (cells per axis, counted from the source
 *                           vertex outwards), its launches (tile-levels that hold tiles) and the launches of the
 *                           per-level kernel (levels that hold cells) for `src` on the grid of cfg.  A source at
 *                           infinity: tile 0, one launch.
 *   pion_gpu_raytrace_host  host only: the rules of dev_raytrace.h in a host loop over P_soa (the layout of
 *                           pion_gpu_upload, ghosts included; only on-grid cells are read) into col and dcol.
 *   pion_gpu_rt_refused     host only: the text with which the calls above refuse (cfg, src), or NULL.
 * EINVAL and a text: 1-D and spherical grids; a handle with a PION_BC_SLAB face (a slab of a decomposed run is traced
 * through the part calls below); an opacity rule other than
 * PION_RT_OPACITY_TOTAL, MINUS, TRACER (VSHELL, HALPHA, RR, HHE and MP need a microphysics object); opacity_var outside
 * the tracers (MINUS, TRACER); more than PION_MAX_RT_SOURCES sources; a direction that is not a face of the grid; a
 * position that is not finite; an unknown id, `what` or plane range; a NULL pointer. */
#define PION_MAX_RT_SOURCES 4
#define PION_RT_OPACITY_TOTAL 1   /* constants of raytracing/rad_src_info / constants.h: RT_OPACITY_* */
#define PION_RT_OPACITY_MINUS 2
#define PION_RT_OPACITY_TRACER 3
typedef struct pion_gpu_rt_source {
  double pos[PION_MAX_DIM]; /* finite source: position, physical units */
  int at_infinity;          /* 1: parallel rays */
  int dir;                  /* at infinity: the face the source lies beyond, 0..5 = XN XP YN YP ZN ZP */
  int opacity;              /* PION_RT_OPACITY_* */
  int opacity_var;          /* tracer index (0 = first tracer) for MINUS and TRACER */
} pion_gpu_rt_source;
int pion_gpu_add_rt_source(void *handle, const pion_gpu_rt_source *src, int *id, double *pos_used);
int pion_gpu_raytrace(void *handle, int which);
int pion_gpu_rt_columns(void *handle, int id, int what, double *host);
long pion_gpu_rt_count(void *handle, int planes);
int pion_gpu_pack_columns(void *handle, int id, int what, int plane_lo, int plane_hi, void *dbuf);
int pion_gpu_rt_plan(const pion_gpu_config *cfg, const pion_gpu_rt_source *src, int tile[3], long *launches, long *levels);
int pion_gpu_raytrace_host(const pion_gpu_config *cfg, const pion_gpu_rt_source *src, const double *P_soa, double *col,
                           double *dcol);
const char *pion_gpu_rt_refused(const pion_gpu_config *cfg, const pion_gpu_rt_source *src);
/* The ray tracer in a slab run, columns handed from rank to rank (dev_raytrace.h: "a part", rt_role).  The handle
 * holds the planes [plane_lo, plane_lo + n) of the slab axis (z in 3-D, y in 2-D; n = the handle's own ng of that axis)
 * out of global_planes; global_xmin is the whole domain's xmin of that axis.  One plane of col per internal face and
 * source crosses: pion_gpu_rt_count(handle, 1) doubles.  Traced in the order of the chain -- receive, trace, send, from
 * the rank that holds the source outwards -- the ranks' arrays are == the planes of one handle of the whole domain.
 * Received columns are not clamped at 0 (the reference does, RT_MPI_boundaries.cpp:352,364).
 *   pion_gpu_add_rt_source_part  pion_gpu_add_rt_source for a part: accepted on a handle with PION_BC_SLAB faces of the
 *                           slab axis, and on a whole-domain handle (plane_lo = 0, global_planes = n), where it equals
 *                           pion_gpu_add_rt_source.  pos and pos_used are positions of the WHOLE domain; the vertex
 *                           along the slab axis is found from global_xmin on every rank.
 *   pion_gpu_rt_chain       host only: the rank's role for `src`.  *recv_side = PION_RT_RECV_NONE, _BELOW or _ABOVE;
 *                           *send_lo, *send_hi = 1 where the rank's lowest / highest own plane goes to the neighbour
 *                           below / above.  A source at infinity across the slab axis: no message at all.
 *   pion_gpu_raytrace_part  traces source id alone from array `which`.  dface_in: the plane received (DEVICE memory;
 *                           may be NULL where recv_side is NONE, is not read there); dface_out_lo, dface_out_hi: DEVICE
 *                           buffers that take the rank's lowest and highest own plane of col afterwards (either may be
 *                           NULL: not written).  Enqueued on the compute stream, returns at once.
 *   pion_gpu_raytrace_host_part  host only: the same functions in a host loop; face_in as above, in host memory.
 *   pion_gpu_rt_plan_part   host only: for a finite source the launches of the tiled kernel on this part (tile-levels
 *                           that hold tiles), the workgroups of one launch -- the tiles of [klo / tile, khi / tile] per
 *                           axis and side, klo and khi the nearest and farthest on-grid cell -- and what that count
 *                           would be with tiles counted from the vertex.  A source at infinity: 1, 0, 0.
 *   pion_gpu_rt_part_refused  host only: the text with which the calls above refuse (cfg, src, part), or NULL.
 * pion_gpu_raytrace refuses a handle that has part sources and a slab face: it cannot know the faces.
 * EINVAL and a text: everything pion_gpu_add_rt_source refuses except the slab face of the slab axis; plane_lo < 0;
 * plane_lo + n > global_planes; a global_xmin that is not finite; a null part; a NULL dface_in where a plane is received;
 * pion_gpu_raytrace_part for a source that was added without a part on a handle with a slab face. */
#define PION_RT_RECV_NONE 0
#define PION_RT_RECV_BELOW 1
#define PION_RT_RECV_ABOVE 2
typedef struct pion_gpu_rt_part {
  int plane_lo, global_planes;
  double global_xmin;
} pion_gpu_rt_part;
int pion_gpu_add_rt_source_part(void *handle, const pion_gpu_rt_source *src, const pion_gpu_rt_part *part, int *id,
                                double *pos_used);
int pion_gpu_rt_chain(const pion_gpu_config *cfg, const pion_gpu_rt_source *src, const pion_gpu_rt_part *part,
                      int *recv_side, int *send_lo, int *send_hi);
int pion_gpu_raytrace_part(void *handle, int which, int id, const void *dface_in, void *dface_out_lo, void *dface_out_hi);
int pion_gpu_raytrace_host_part(const pion_gpu_config *cfg, const pion_gpu_rt_source *src, const pion_gpu_rt_part *part,
                                const double *P_soa, const double *face_in, double *col, double *dcol);
int pion_gpu_rt_plan_part(const pion_gpu_config *cfg, const pion_gpu_rt_source *src, const pion_gpu_rt_part *part,
                          long *launches, long *workgroups, long *workgroups_from_vertex);
const char *pion_gpu_rt_part_refused(const pion_gpu_config *cfg, const pion_gpu_rt_source *src, const pion_gpu_rt_part *part);
/* adopt caller-owned device buffers (e.g. torch tensors) instead of internal ones;
 * both must hold nvar*ncell_all doubles */
int pion_gpu_bind_device_state(void *handle, void *dP, void *dPh);
void *pion_gpu_device_ptr(void *handle, int which);
/* HIP stream all subsequent work of this handle is issued on (hipStream_t) */
int pion_gpu_set_stream(void *handle, void *stream);
/* Second HIP stream for pion_gpu_pack_halo / pion_gpu_unpack_halo (NULL: the compute stream).
 * The library orders pack after the compute stream's work so far and PION_STAGE_SLABBOUNDARY after the
 * last unpack; the caller's transfer (RCCL/MPI) must be enqueued on, or ordered with, this stream. */
int pion_gpu_set_comm_stream(void *handle, void *stream);
/* the handle's streams (hipStream_t): which = 0 compute, 1 comm */
void *pion_gpu_get_stream(void *handle, int which);
int pion_gpu_synchronize(void *handle);

/* internal fixed-state cells: stellar wind (grid/stellar_wind_BC.cpp:642-677,
 * boundaries/stellar_wind_boundaries.cpp:244-350).  idx = cell ids (with
 * ghosts), states = n*nvar doubles (cell-major).  Marks the cells
 * isbd=true,isdomain=false (stellar_wind_BC.cpp:277-278). */
int pion_gpu_set_wind_cells(void *handle, long n, const long *idx, const double *states);

/* Stellar-wind sources the device builds and updates itself (grid/stellar_wind_BC.cpp, stellar_wind and
 * stellar_wind_evolution; boundaries/stellar_wind_boundaries.cpp).  WINDTYPE_CONSTANT (type 0) and
 * WINDTYPE_EVOLVING (type 1) of grid/stellar_wind_BC.h:41-42, every geometry of pion_gpu_config:
 * 1-D spherical (source at r = 0), 2-D cylindrical (z,R) (source on the axis), 2-D Cartesian (slab symmetry),
 * 3-D Cartesian.  Euler, ideal MHD and GLM (not MHD in 1-D). */
#define PION_MAX_WIND_SOURCES 8
typedef struct pion_gpu_wind_source {
  double pos[PION_MAX_DIM];   /* source position, physical units (unused axes ignored) */
  double radius;              /* radius of the wind region, physical units (> 0) */
  int type;                   /* 0 = constant, 1 = evolving (here 2, 3: EINVAL; 2 = rotating star, through
                               * pion_gpu_add_rotating_wind_source; 3 = latitude-dependent: not supported) */
  double mdot;                /* Msun/yr   (constant: converted to g/s as add_source does, stellar_wind_BC.cpp:166-172) */
  double vinf, vrot;          /* km/s      (constant) */
  double Tw, Rstar, Bstar;    /* K, cm, G  (constant; Bstar also for evolving sources) */
  double tracers[PION_MAX_NVAR];  /* wind tracer values (the first ntracer are used) */
  /* evolving sources (add_evolving_source, stellar_wind_BC.cpp:1109-1245): a table of npt >= 2 rows, cgs, the
   * times already offset and scaled ((t + time_offset)/t_scalefactor, see pion_host_read_wind_evolution).
   * The arrays are copied by pion_gpu_add_wind_source. */
  int npt;
  const double *evo_time, *evo_Teff, *evo_Mdot, *evo_vrot, *evo_vinf, *evo_R;
  const double *evo_X[7];     /* element columns X_H, X_He, X_C, X_N, X_O, X_Z, X_D (NULL: not selected) */
  int evo_tracer_elem[PION_MAX_NVAR];  /* per tracer: -1 = the constant value above, 0..6 = the evo_X column
                                        * (set_element_indices, :992-1024; the caller maps the tracer names) */
  double t_now;               /* simulation time when the source is set up (add_evolving_source's t_now) */
  double update_freq;         /* SWP update_freq / t_scalefactor (only decides activity at set-up) */
  /* orbital motion (BC_update_STWIND, boundaries/stellar_wind_boundaries.cpp:253-352; WIND_i_ecentricity_fac,
   * WIND_i_periastron_vec_x/y, WIND_i_orbital_period of dataIO/dataio_base.cpp:934-980): with orbit_period != 0
   * the source moves on an ellipse in the x-y plane around `pos`, re-placed at every boundary update from that
   * update's simtime (pion_gpu_wind_orbit_position).  orbit_period = 0: the source stays at `pos`.
   * Both periastron components and orbit_ecc_fac must be non-zero, else the position is NaN (as in the
   * reference) and the source loses its cells at the first update. */
  double orbit_ecc_fac;       /* ecentricity_fac */
  double orbit_periastron[2]; /* periastron vector (x, y), cm */
  double orbit_period;        /* years; 0 = fixed */
} pion_gpu_wind_source;

/* stellar_wind::add_source / stellar_wind_evolution::add_evolving_source + BC_assign_STWIND_add_cells2src: every
 * cell (ghosts included) with distance_vertex2cell <= radius joins the source, in cell-id order; the cells are
 * marked isbd = true, isdomain = false.  Call after create, any number of times; sources are applied in id order
 * (*id = 0, 1, ...).  EINVAL where the reference calls rep.error: a source off the axis (cylindrical) or off r = 0
 * (spherical), MHD in 1-D, type 2 or 3, radius <= 0, an evolving table with npt < 2, more than
 * PION_MAX_WIND_SOURCES sources.  Also EINVAL (a divergence: the reference would move the source off the axis or
 * the origin) for orbit_period != 0 on a 1-D grid or a cylindrical or spherical one.
 * A source with orbit_period != 0 is re-placed at every pion_gpu_update_bcs, before any state is written, in id
 * order: the cells within `radius` of its current position lose isbd and become isdomain (whichever source they
 * belong to, ghosts included), then the cells within `radius` of the new position join it in cell-id order. */
int pion_gpu_add_wind_source(void *handle, const pion_gpu_wind_source *src, int *id);
/* Current position of source `id` (PION_MAX_DIM doubles; unused axes 0). */
int pion_gpu_get_wind_source_pos(void *handle, int id, double *pos);
/* The cell flags (PION_CELL_*, ncell_all bytes, ghosts included) as the device holds them now (synchronises). */
int pion_gpu_get_flags(void *handle, unsigned char *out);
/* The HLLD -> HLL switch of every cell (ncell_all bytes, ghosts included) as the prepass of the last stage left it
 * (synchronises; read-only).  EINVAL for a handle without the switch (not MHD / GLM with HLLD). */
int pion_gpu_get_hll_switch(void *handle, unsigned char *out);
/* The H-correction eta of every cell along `axis` (ncell_all doubles, ghosts included; the value of interface
 * (c | c+1 along axis) is stored at c, the last cell of a column holds 0) as the prepass of the last stage left it
 * (synchronises; read-only).  EINVAL for a handle without the H-correction (artvisc 3 / 4) or axis outside 0..ndim-1. */
int pion_gpu_get_hcorr_eta(void *handle, int axis, double *out);
/* The screened prepass (3-D MHD / GLM with HLLD; PION_HLL_SCREEN=0 in the environment switches it off): number of
 * blocks of cells the last stage's prepass evaluated, and number of blocks.  active = -1, total = 0 when that prepass
 * was the dense one.  Synchronises: call it outside timed regions. */
int pion_gpu_get_hll_screen_counts(void *handle, int *active, int *total);
/* The position the orbit of `src` gives at `simtime` on a grid of `ndim` (2 or 3) dimensions, in plain double as
 * BC_update_STWIND computes it (src->pos for orbit_period == 0).  Host only: needs no device or handle.  EINVAL for
 * ndim outside 2..3 or a NULL pointer. */
int pion_gpu_wind_orbit_position(const pion_gpu_wind_source *src, int ndim, double simtime, double *pos);
/* WINDTYPE_ANGLE (type 2): the rotating star of Langer, Garcia-Segura & Mac Low (1999), grid/stellar_wind_angle.cpp
 * (add_evolving_source :700, add_rotating_source :836, update_source :941, set_wind_cell_reference_state :464).
 * src->type must be 2; the evolving-table fields carry the table as for type 1 (cgs, times offset and scaled) and
 * evo_vcrit its vcrit column (npt rows); Bstar, tracers, evo_tracer_elem, t_now and update_freq as for type 1.
 * Membership, flags, id order and pion_gpu_get_wind_cells as for the other sources.  xi = WIND_i_xi, the exponent
 * of the equatorial enhancement; the LGM99 tables are built for it at the first rotating source of the handle.
 * EINVAL: a 1-D grid, a source off the axis (cylindrical), orbit_period != 0, npt < 2, radius <= 0, a NULL column,
 * an xi other than an earlier rotating source's, an evolving (type 1) source on the same handle (either order;
 * constant sources may sit beside rotating ones), more than PION_MAX_WIND_SOURCES sources, or a member cell whose
 * polar angle lies outside (0.1 deg, 89.9 deg] -- e.g. a source on a plane of cell centres (theta = 90 deg). */
int pion_gpu_add_rotating_wind_source(void *handle, const pion_gpu_wind_source *src, const double *evo_vcrit,
                                      double xi, int *id);
/* stellar_wind_angle::setup_tables (stellar_wind_angle.cpp:92-212) for `xi`, in plain double: theta[25] (rad),
 * omega[25], Teff[22] (K), delta[25][22] (omega, Teff) and alpha[25][25][22] (omega, theta, Teff); NULL arrays are
 * skipped.  Host only: needs no device or handle. */
int pion_gpu_wind_angle_tables(double xi, double *theta, double *omega, double *Teff, double *delta, double *alpha);
/* The cells of source `id` in cell-id order and the states (n*nvar doubles, cell-major) the last boundary update
 * wrote (zeros before the first one, or while an evolving source is inactive).  *n = number of cells; idx ==
 * NULL: size query only; states may be NULL.  For a moving source: its current cells (synchronises the stream). */
int pion_gpu_get_wind_cells(void *handle, int id, long *n, long *idx, double *states);

/* jet_bc::BC_assign_JETBC / BC_update_JETBC (boundaries/jet_boundaries.cpp:36-208, 3-D Cartesian
 * branch :170-201, update :212-262) with JetParams (sim_params.h:331-341): every XN ghost cell of an
 * on-grid (y,z) column whose centre lies within jetradius*dx of the x axis holds `jetstate`
 * (rho, p_g, v, then tracers), re-imposed after the external boundaries at every boundary update.
 * 3-D Cartesian (Euler only, as in the reference) or 2-D cylindrical: there the first jetradius rows above
 * the axis, with B = (jetstate[BX], 0, jetstate[BY]) for MHD (:74-83; the radial JETPROFILE of the
 * assignment is overwritten by the uniform state in every update, so it is not reproduced). */
int pion_gpu_set_jet(void *handle, int jetradius, const double *jetstate);

/* mp_only_cooling look-up tables (microphysics/mp_only_cooling.cpp:528-579):
 * nT temperatures, 5 value tables and 5 slope tables in the order
 * rrhp, C_rrh, C_ffhe, C_fbdn, C_cie.  2 <= nT <= 256 (the reference builds 200 points; the cooling kernel
 * keeps the tables in LDS), else PION_GPU_EINVAL. */
int pion_gpu_set_cooling_tables(void *handle, int nT, const double *T,
                                const double *tabs, const double *slopes);

/* The total-CIE cooling curve of EP.cooling = 4..7 (SD93 or WSS09; cooling_function_SD93CIE,
 * microphysics/cooling_SD93_cie.cpp): n knots (log10 T, log10 Lambda), strictly increasing in log10 T and not
 * necessarily uniform, with the natural-spline second-derivative coefficients c[n] that pion_host_build_cooling_curve
 * computes (GSL's cspline representation, what setup_SD93_cie / setup_WSS09_CIE leave in the spline, :150-166, 611-627).
 * Outside the knots the curve is extrapolated linearly in log-log space with min_slope below and max_slope above; the
 * reference's choices are 8.0 below and the slope of the last interval above, (logL[n-1] - logL[n-2]) /
 * (logT[n-1] - logT[n-2]) (:160-164, 621-625).  Evaluated per cell as cooling_rate_SD93CIE (:666-704) and combined as
 * mp_only_cooling::Edot_* (microphysics/mp_only_cooling.cpp:424-482).  2 <= n <= 256 (the cooling kernels keep the
 * curve in LDS); EINVAL for any other n, knots that do not increase, or a value that is not finite.  Discards the cached
 * time step and the screen summary, as pion_gpu_set_cooling_tables does.  (PION_COOL_BISECT=1 in the environment: the
 * device bisects even uniformly spaced knots, as it does for the tables; a cross-check.)  A stage, a time step or a cooling seam of a
 * handle with cooling 4..7 and no curve is EINVAL with a text; 0, 2 and 8 need no curve. */
int pion_gpu_set_cooling_curve(void *handle, int n, const double *logT, const double *logL, const double *c,
                               double min_slope, double max_slope);

/* ---- the hot path ------------------------------------------------------ */

/* assign_update_bcs::TimeUpdateInternalBCs + TimeUpdateExternalBCs
 * (boundaries/assign_update_bcs.cpp:134-252): fills ghost cells of Ph, and of
 * P too when cstep==maxstep.  Internal boundaries first: the set_wind_cells list, then the wind sources of
 * pion_gpu_add_wind_source at `simtime` (written to P and Ph), then the external faces.
 * EINVAL, with nothing written, when an active rotating source (pion_gpu_add_rotating_wind_source) would write
 * with omega = min(v_rot/vcrit, 0.999) <= 0 or Tw <= 1000 K at `simtime`: the reference's look-up stops there.  `assign`!=0 additionally captures the constant
 * inflow/fixed reference states from P (BC_assign_*, inflow_boundaries.cpp,
 * fixed_boundaries.cpp) and must be used for the first call after upload. */
int pion_gpu_update_bcs(void *handle, double simtime, int cstep, int maxstep, int assign);

/* calc_timestep::calc_dynamics_dt (sim_control/calc_timestep.cpp:271-333) and
 * get_mp_timescales_no_radiation (:405-507): min over on-grid cells of
 * FV_solver_*::CellTimeStep (solver_eqn_hydro_adi.cpp:460-502,
 * solver_eqn_mhd_adi.cpp:516-582) and MP->timescales
 * (mp_only_cooling.cpp:333-368).  No limiting is applied here. */
int pion_gpu_calc_dt(void *handle, double *t_dyn, double *t_mp);
/* The same reduction in two halves, for slab-decomposed runs (sim_control_MPI.cpp:503-504 does
 * COMM->global_operation_double("MIN", .) on the host value; here the minimum stays on the device
 * until it has been reduced over the ranks):
 *   pion_gpu_calc_dt_device  enqueues the reduction (nothing, when the last full stage left the minima
 *                            behind) and returns the device address of {min t_dyn, min t_mp} (2 doubles);
 *                            no host synchronisation.  The caller may all-reduce(min) that buffer in place
 *                            on the handle's compute stream (ncclAllReduce(ncclMin)).
 *   pion_gpu_read_dt         the single 16-byte read-back + the device error word. */
int pion_gpu_calc_dt_device(void *handle, void **dptr);
int pion_gpu_read_dt(void *handle, double *t_dyn, double *t_mp);
/* pion_gpu_read_dt in two halves: _request enqueues the copy of the minima and of the error word into pinned
 * host memory (compute stream) and returns; _wait blocks until it has arrived.  A host loop requests the
 * minima right after the full-step stage, enqueues the boundary update and the halo exchange, and only then
 * waits: the read-back latency hides under work the next step needs anyway. */
int pion_gpu_dt_request(void *handle);
int pion_gpu_dt_wait(void *handle, double *t_dyn, double *t_mp);

/* FV_solver_mhd_mixedGLM_adi::Set_GLM_Speeds (solver_eqn_mhd_adi.cpp:906-922):
 * c_h = CFL*dx/dt, c_r = cr. */
int pion_gpu_set_glm_speeds(void *handle, double dt, double dx, double cr);

/* One stage of time_integrator::first_order_update / second_order_update
 * (sim_control/time_integrator.cpp:151-250) without the boundary update:
 *   Setdt(dt_stage); calc_microphysics_dU (:253-296,438-489);
 *   calc_dynamics_dU = preprocess_data + set_dynamics_dU (:498-873);
 *   grid_update_state_vector (:881-958).
 * space_ooa: OA1 (first half step) or OA2; is_full_step: step==ooa (P=Ph). */
int pion_gpu_stage(void *handle, double dt_stage, int space_ooa, int is_full_step);

/* The same stage in two parts, so that a slab's halo exchange (MCMD_boundaries.cpp:122-237, which
 * the reference completes before calc_dynamics_dU starts) runs underneath most of the work.  The slab axis is
 * the last axis of the grid; its "planes" are x-y planes of a 3-D grid and rows (along x) of a 2-D grid:
 *   PION_STAGE_WHOLE         every on-grid plane of the slab axis, after the last unpacked halo;
 *   PION_STAGE_INTERIOR      the on-grid planes [nbc, n - nbc) that read no ghost plane of the slab axis; may
 *                            be issued while the halo of the stencil array is still in flight;
 *   PION_STAGE_SLABBOUNDARY  the nbc planes next to each face of the slab axis (one launch for both strips; one
 *                            launch per strip on a handle that runs its stages in plane windows, see
 *                            pion_gpu_rows_windows); ordered after the last pion_gpu_unpack_halo /
 *                            pion_gpu_halo_end (comm stream) inside the library.
 * INTERIOR followed by SLABBOUNDARY gives bit for bit the result of PION_STAGE_WHOLE (= pion_gpu_stage), and so does
 * every part run window by window.
 * Configurations the split does not cover (1-D grids, 2-D grids not run by the rows kernel -- PION_ROWS_2D=0,
 * nbc < 2 --, H-correction, first-order scheme, <= 2*nbc planes) do all the work in the SLABBOUNDARY call. */
#define PION_STAGE_WHOLE 0
#define PION_STAGE_INTERIOR 1
#define PION_STAGE_ZBOUNDARY 2
#define PION_STAGE_SLABBOUNDARY PION_STAGE_ZBOUNDARY
int pion_gpu_stage_part(void *handle, double dt_stage, int space_ooa, int is_full_step, int part);

/* Plane windows of the rows kernel.  k_stage_rows2 reaches fewer than 2^29 cells of an array from the array's base (a
 * 32-bit byte offset per lane), so a grid of 2^29 cells or more per variable (ghosts included) is run in windows of
 * planes of the slab axis (x-y planes in 3-D, rows in 2-D, Cartesian or cylindrical), one launch per window with the
 * arrays' bases advanced to the window on the host; the result is bit for bit that of one launch.  With s cells per
 * plane, W = floor((limit - 1) / s) - 2 nbc planes fit in one window; a range [lo, hi) of on-grid planes becomes
 * ceil((hi - lo) / W) windows, in order, sizes balanced within one plane, longer ones first.  W < 1 (one plane with
 * its ghost planes exceeds the limit), 1-D grids and grids with nbc < 2 stay on the cell-per-thread kernel.
 *   pion_gpu_rows_windows      the plan for the slab axis of `cfg`: returns the number of windows of [lo, hi) and
 *                              writes the first max_windows of them to w_lo[] / w_hi[] (NULL allowed for
 *                              max_windows = 0); 0: not admitted, the cell-per-thread kernel runs.  limit_cells
 *                              <= 0: the default, 2^29.  Host only: needs no device or handle.  EINVAL: a NULL or
 *                              malformed cfg, lo < 0, hi > ng of the slab axis, lo >= hi, limit_cells > 2^29,
 *                              max_windows < 0.
 *   pion_gpu_get_rows_windows  what a handle does: its limit (2^29; PION_ROWS_WINDOW_CELLS in the environment at
 *                              create, for tests and measurements; PION_ROWS_WINDOWS=0: no windows, the
 *                              cell-per-thread kernel from 2^29 cells), the windows of a whole stage (1: one launch;
 *                              0: the handle runs the cell-per-thread kernel) and the number of stage-kernel
 *                              launches the last stage part issued.  NULL outputs are skipped. */
int pion_gpu_rows_windows(const pion_gpu_config *cfg, long limit_cells, int lo, int hi, int max_windows, int *w_lo,
                          int *w_hi);
int pion_gpu_get_rows_windows(void *handle, long *limit_cells, int *windows_whole_stage, int *launches_last_part);

/* time_integrator::advance_time (time_integrator.cpp:72-142) for OA1/OA1 and
 * OA2/OA2: stages + boundary updates. */
int pion_gpu_advance_time(void *handle, double dt, double simtime);

/* ---- slab decomposition (replaces decomposition/MCMD_control.cpp:231-309 and
 * comms/comm_mpi.cpp:287-636 for this path) -------------------------------- */

/* Copy the nbc on-grid planes of the slab axis adjacent to face (3-D: 4=ZN, 5=ZP; 2-D: 2=YN, 3=YP) of `which`
 * (0=P,1=Ph) into a contiguous device buffer [nvar][nbc][ny_all][nx_all] (2-D: [nvar][nbc][nx_all]), or
 * write such a buffer into the ghost planes of that face. */
long pion_gpu_halo_count(void *handle); /* doubles per halo buffer */
/* In-place exchange (no pack / unpack kernels): in the [nvar][nz_all][ny_all][nx_all] layout the nbc planes
 * next to a face of the slab axis (z planes in 3-D; in 2-D the nbc rows next to a y face, nbc * nx_all doubles)
 * are ONE contiguous run of count_per_var doubles per variable, so a transport can send
 * from, and receive into, the state array directly (variable v: pointer + v * var_stride doubles):
 *   send_lo / send_hi  the first / last nbc on-grid planes (x/y ghosts included; 2-D: rows, x ghosts included)
 *   recv_lo / recv_hi  the ghost planes of the lower / upper face (ZN / ZP; 2-D: YN / YP).
 * EINVAL for a 1-D grid.
 * pion_gpu_halo_begin orders the communication stream after the compute stream's work so far (what
 * pion_gpu_pack_halo does first), pion_gpu_halo_end marks the point of the communication stream after
 * which the ghost planes are complete (what pion_gpu_unpack_halo does last): PION_STAGE_SLABBOUNDARY and
 * whole stages wait for it inside the library. */
typedef struct {
  double *send_lo, *send_hi, *recv_lo, *recv_hi;
  long count_per_var, var_stride;
  int nvar;
} pion_gpu_halo_spans_t;
int pion_gpu_halo_spans(void *handle, int which, pion_gpu_halo_spans_t *out);
int pion_gpu_halo_begin(void *handle);
int pion_gpu_halo_end(void *handle);
int pion_gpu_pack_halo(void *handle, int which, int face, void *dbuf);
int pion_gpu_unpack_halo(void *handle, int which, int face, void *dbuf);

/* ---- test seams -------------------------------------------------------- */

/* FV_solver_base::InterCellFlux (spatial_solvers/solver_eqn_base.cpp:152-204)
 * for n independent interfaces along `axis`.  Pl, Pr: n*nvar (interface-major)
 * edge states; aux: n*4 doubles {HC_etamax, use_HLL(0/1), unused, unused};
 * F, Pstar: n*nvar outputs.  dt is the value of FV_dt (Lax-Friedrichs only). */
int pion_gpu_interface_flux(void *handle, int n, int axis, double dt, const double *Pl,
                            const double *Pr, const double *aux, double *F, double *Pstar);

/* The cell update of a stage for n independent cells, through the stage kernels' own device functions.
 * P_out (n*nvar): FV_solver_*::CellAdvanceTime (solver_eqn_hydro_adi.cpp:372-448, solver_eqn_mhd_adi.cpp:452-504,
 * :822-844) of (P_in, dU), both n*nvar, then grid_update_state_vector's T > MaxTemperature ceiling
 * (time_integrator.cpp:926-932), with FV_dt = fv_dt and the GLM speeds of pion_gpu_set_glm_speeds.
 * dt_out (n): CellTimeStep of P_in.  dU and P_out may both be NULL (no update), or dt_out (no time step).
 * Returns PION_GPU_EPHYSICS, with the outputs written, when a cell's density came out <= 0. */
int pion_gpu_cell_advance(void *handle, int n, double fv_dt, const double *P_in, const double *dU,
                          double *P_out, double *dt_out);

/* mp_only_cooling::TimeUpdateMP (microphysics/mp_only_cooling.cpp:167-218) for n
 * independent cells: P_in n*nvar, P_out n*nvar. */
int pion_gpu_cooling_update(void *handle, int n, double dt, const double *P_in, double *P_out);
/* mp_only_cooling::Edot (:377-415; the handle's EP.cooling: :424-482, :491-521, cooling.cpp:373-399) for n (rho,T) pairs */
int pion_gpu_cooling_edot(void *handle, int n, const double *rho, const double *T, double *edot);
/* cooling_function_SD93CIE::cooling_rate_SD93CIE (cooling_SD93_cie.cpp:666-704) on the curve of
 * pion_gpu_set_cooling_curve, through the cooling kernels' own function with the curve staged in LDS: lambda[i] =
 * Lambda(T[i]) for n temperatures (infinity for T < 0 or a T that is not finite).  Any handle with a curve set. */
int pion_gpu_cooling_curve_eval(void *handle, int n, const double *T, double *lambda);
/* mp_only_cooling::timescales(P, gamma, tc=true, ...) (:333-368) for n independent cells: P_in n*nvar,
 * t_cool n doubles (1e99 below 1.1 MinT_allowed) */
int pion_gpu_cooling_timescale(void *handle, int n, const double *P_in, double *t_cool);

/* last kernel timings, milliseconds, measured with HIP events on the handle's stream:
 * out[0]=stage kernel, out[1]=prepass, out[2]=bc fill, out[3]=dt reduction (mean per launch);
 * with n >= 8 also out[4..7] = the number of launches each mean was taken over */
int pion_gpu_enable_timing(void *handle, int on);
int pion_gpu_get_timing(void *handle, double *out, int n);

#ifdef __cplusplus
}
#endif
#endif /* PION_GPU_H */
