// projection_io.cpp -- projected images of the C++ host loop (sim_control_gpu::write_projection,
// set_projection_output; the rules: pion_amd/csrc/dev_project.h).  The file is a FITS file of fits_io.h's kind: the
// primary header of write_fits with pion_proj_axis and pion_proj_<n>_{a,var,coef,b} appended, then one two-dimensional
// IMAGE extension per field (NAXIS1 = NI, NAXIS2 = NJ, EXTNAME = the field's name).  The images come from the backend's
// project_* entries; a table without them downloads array 0 and runs dev_project.h's functions in a host loop.  An
// image is small, so it is written whole, through the file object of out_file.h.  One rank of a slab run hands the
// image of the whole domain from rank to rank (relay_part), and the last rank writes the one file.
// write_projection_angle / set_projection_angle_output: a (z,R) grid seen at an angle to its axis (the rule:
// pion_amd/csrc/dev_project_angle.h), the same kind of file with pion_proj_angle, _n_extra, _pixdx, _pixz0 in place of
// pion_proj_axis; single rank only.
#include <string>
#include <vector>

#include "dev_rules.h"
#include "fits_io.h"
#include "sim_control_gpu.h"
#include "slab_comm.h"

namespace pion_host {

// ---- dev_project.h's functions in a host loop, over a whole array A ([nvar][ncell], ghosts included): what a backend
// table without projection entries gets, and the C view at the end of this file
// the images of a single grid, [nfields][NJ][NI]
static void project_on_host(const pion::GridDesc &g, const pion::OutputCfg &o, int axis, int nfields, const pion_gpu_proj_field *fields,
                     const double *A, double *img)
{
  const pion::ProjGeom q = pion::proj_geom(g, axis);
  for (int f = 0; f < nfields; f++)
    for (long j = 0; j < q.nj; j++)
      for (long i = 0; i < q.ni; i++) {
        const long first = q.c0 + i * q.si + j * q.sj;
        img[((long)f * q.nj + j) * q.ni + i] = (g.cyl == 1) ? pion::abel_column(g, o, fields[f], q, A, first, (int)j)
                                                            : pion::proj_column(g, o, fields[f], q, axis, A, first);
      }
}
// one rank's part, into the image of the whole domain [nfields][NJ_global][NI_global] (in/out)
static void project_part_on_host(const pion::GridDesc &g, const pion::OutputCfg &o, int axis, int nfields,
                          const pion_gpu_proj_field *fields, const pion::ProjPart &pp, const double *A, double *img)
{
  const pion::ProjGeom q = pion::proj_geom(g, axis);
  const pion::GridDesc gg = pion::proj_part_grid(g, pp);
  const bool along = pion::proj_part_along_slab(g, axis);
  const long npix = (long)pion::proj_part_nj(g, q, axis, pp) * q.ni;
  for (int f = 0; f < nfields; f++) {
    double *out = img + (long)f * npix;
    if (g.cyl == 1) {
      for (long j = 0; j < pp.plane_lo + q.nsum; j++)   // the impact rows below this rank's upper edge
        for (long i = 0; i < q.ni; i++)
          out[j * q.ni + i] = pion::abel_column_part(g, gg, o, fields[f], q, pp, A, q.c0 + i * q.si, (int)j, out[j * q.ni + i]);
      continue;
    }
    for (long j = 0; j < q.nj; j++)
      for (long i = 0; i < q.ni; i++) {
        const long first = q.c0 + i * q.si + j * q.sj;
        double &px = out[(j + (along ? 0 : pp.plane_lo)) * q.ni + i];
        px = along ? pion::proj_column_part(g, o, fields[f], q, pp, A, first, px)
                   : pion::proj_column(g, o, fields[f], q, axis, A, first);
      }
  }
}

// the file of both writers: `params` (the primary header so far) gains the per-field keys; then one big-endian
// double-precision IMAGE extension [nj][ni] per field, img = [nfields][nj][ni] native doubles
static int write_image_file(const char *who, const char *path, std::string &err, std::vector<snapshot_param> &params, int nfields,
                            const pion_gpu_proj_field *fields, long ni, long nj, const std::vector<double> &img)
{
  for (int i = 0; i < nfields; i++) {
    const std::string k = "pion_proj_" + std::to_string(i) + "_";
    params.push_back({k + "a", std::to_string(fields[i].a), 'i'});
    params.push_back({k + "var", std::to_string(fields[i].var), 'i'});
    params.push_back({k + "coef", fmt_d(fields[i].coef), 'd'});
    params.push_back({k + "b", fmt_d(fields[i].b), 'd'});
  }
  const long npix = nj * ni, n = nfields * npix;
  std::vector<unsigned long long> R((size_t)n);
  for (long k = 0; k < n; k++) R[(size_t)k] = pion::out_be64(img[(size_t)k]);
  const std::string primary = fits_primary_header(params);
  const long naxis[2] = {ni, nj};
  std::vector<std::string> ext((size_t)nfields);
  for (int i = 0; i < nfields; i++) ext[(size_t)i] = fits_image_header(fields[i].name, 2, naxis);
  const fits_layout L(primary, ext, npix * (long)sizeof(double));

  PartFile f(who, path, err);
  if (!f.ok()) return PION_GPU_EINVAL;
  int rc = L.start(f);
  for (int i = 0; i < nfields && !rc; i++) rc = f.write(R.data() + (size_t)i * npix, (size_t)npix * sizeof(double), L.data_at(i));
  return f.commit(rc);
}

// dev_project_angle.h in a host loop: the field values of every on-grid cell once, then angle_pixel per pixel.
// img = [nfields][NR][NI]; returns the pixels whose ray loop reached trip_limit
static long project_angle_on_host(const pion::GridDesc &g, const pion::OutputCfg &o, const pion::AngleGeom &q, int nfields,
                                  const pion_gpu_proj_field *fields, const double *A, int trip_limit, double *img)
{
  const long ncells = (long)q.nr * q.nz;
  std::vector<double> V((size_t)nfields * ncells);
  for (int f = 0; f < nfields; f++)
    for (long ir = 0; ir < q.nr; ir++)
      for (long iz = 0; iz < q.nz; iz++)
        V[(size_t)(f * ncells + ir * q.nz + iz)] = pion::proj_value(g, o, fields[f], A, (g.nbc[0] + iz) + g.sy * (g.nbc[1] + ir));
  long ncapped = 0;
  for (int j = 0; j < q.nr; j++)
    for (long i = 0; i < q.ni; i++) {
      double ans[PION_PROJ_MAX_FIELDS];
      ncapped += pion::angle_pixel(q, V.data(), nfields, i, j, trip_limit, ans);
      for (int f = 0; f < nfields; f++) img[((long)f * q.nr + j) * q.ni + i] = ans[f];
    }
  return ncapped;
}

// one rank of a slab run whose images are assembled along the ranks: a slab extent AND a communicator of more than
// one rank that has the send / receive pair
bool sim_control_gpu::projection_collective() const
{
  return slab.set && comm_ && comm_->world() > 1 && comm_->has_relay();
}

int sim_control_gpu::projection_refused(int axis, int nfields, const pion_gpu_proj_field *fields, const char *who)
{
  const char *why = nullptr;
  if ((slab.set || (comm_ && comm_->world() > 1)) && !projection_collective()) {
    if (!slab.set)
      why = "project: this sim is one rank of a slab run without a slab extent (set_slab_extent), and its part of the image "
            "cannot be placed";
    else if (!comm_ || comm_->world() < 2)
      why = "project: this sim is one rank of a slab run without a communicator of more than one rank, and the images of "
            "more than one rank are assembled along the communicator";
    else
      why = "project: this sim is one rank of a slab run, and its communicator's send / receive is not supported";
  }
  if (!why) why = pion::proj_refused_grid(grid_desc(cfg), axis);
  if (!why) why = pion::proj_refused_fields(pion::out_cfg(cfg), nfields, fields);
  if (!why) return 0;
  io_error_ = std::string(who) + ": " + why;
  return PION_GPU_EINVAL;
}

int sim_control_gpu::set_projection_output(int axis, int nfields, const pion_gpu_proj_field *fields)
{
  io_error_.clear();
  if (nfields == 0) {
    proj_fields_.clear();
    return 0;
  }
  if (int rc = projection_refused(axis, nfields, fields, "set_projection_output")) return rc;
  proj_axis_ = axis;
  proj_fields_.assign(fields, fields + nfields);
  return 0;
}

// this sim's images -- a whole grid's, or (part) this rank's part added into `img` --, on the device where the backend
// has the entries, else from a download by the functions above
int sim_control_gpu::project_images(int axis, int nfields, const pion_gpu_proj_field *fields, const pion_gpu_proj_part *part,
                                    long n, double *img)
{
  if (!part && be_->project_count && be_->project_to_host) {
    if (be_->project_count(h_, axis, nfields) != n) {
      io_error_ = "write_projection: the backend refuses: " + last_error();
      return PION_GPU_EINVAL;
    }
    const int rc = be_->project_to_host(h_, axis, nfields, fields, img);
    if (rc) io_error_ = "write_projection: project_to_host failed: " + last_error();
    return rc;
  }
  if (part && be_->project_part_count && be_->project_part_to_host) {
    if (be_->project_part_count(h_, axis, nfields, part) != n) {
      io_error_ = "write_projection: the backend refuses: " + last_error();
      return PION_GPU_EINVAL;
    }
    const int rc = be_->project_part_to_host(h_, axis, nfields, fields, part, img);
    if (rc) io_error_ = "write_projection: project_part_to_host failed: " + last_error();
    return rc;
  }
  const pion::GridDesc g = grid_desc(cfg);
  std::vector<double> A((size_t)cfg.nvar * g.ncell);
  if (int rc = be_->download(h_, 0, A.data())) {
    io_error_ = "write_projection: download failed: " + last_error();
    return rc;
  }
  if (!part) project_on_host(g, pion::out_cfg(cfg), axis, nfields, fields, A.data(), img);
  else {
    const pion::ProjPart pp = {part->plane_lo, part->global_planes, part->last, part->global_xmin};
    project_part_on_host(g, pion::out_cfg(cfg), axis, nfields, fields, pp, A.data(), img);
  }
  return 0;
}

// One rank of a slab run (dev_project.h, "parts"): the image of the whole domain comes from the rank below, gains this
// rank's part and goes to the rank above.  The invariant that keeps every rank from waiting for ever: whatever `rc`
// this rank arrives with and whatever happens here, it ALWAYS takes the message of the rank below and ALWAYS sends one
// to the rank above -- the image, or a failure.  Returns 0 with the image in `img` (complete on the last rank)
int sim_control_gpu::relay_part(int rc, int axis, int nfields, const pion_gpu_proj_field *fields, const pion_gpu_proj_part &part,
                                std::vector<double> &img)
{
  // (refused here: the length is unknown, and the message of the rank below is taken off the wire without a buffer)
  const size_t bytes = rc ? 0 : img.size() * sizeof(double);
  int below = 0;
  const int rrc = comm_->recv_from_below(rc ? nullptr : img.data(), bytes, &below);
  if (!rc && below) {
    io_error_ = "write_projection: a rank below failed, no image is written";
    rc = PION_GPU_EINVAL;
  }
  if (!rc && rrc) {
    io_error_ = "write_projection: receiving the image of the rank below failed: " + comm_->last_error();
    rc = rrc;
  }
  if (!rc) rc = project_images(axis, nfields, fields, &part, (long)img.size(), img.data());
  const int src = comm_->send_to_above(rc ? nullptr : img.data(), bytes, rc ? 1 : 0);
  if (!rc && src) {
    io_error_ = "write_projection: handing the image to the rank above failed: " + comm_->last_error();
    rc = src;
  }
  return rc;
}

int sim_control_gpu::write_projection(const char *path, int axis, int nfields, const pion_gpu_proj_field *fields)
{
  if (int rc = path_refused("write_projection", path)) return rc;
  // one rank of a slab run: the call is collective, and the last rank writes the one file
  const bool chain = projection_collective();
  std::vector<snapshot_param> params;
  long nloc = 0;
  int rc = projection_refused(axis, nfields, fields, "write_projection");
  if (!rc) rc = writer_params("write_projection", params, nloc);
  if (rc && !chain) return rc;

  // 1. the images, native doubles [nfields][NJ][NI] of the whole domain
  const pion::GridDesc g = grid_desc(cfg);
  pion::ProjGeom q = pion::ProjGeom();
  std::vector<double> img;
  if (!rc) {
    q = pion::proj_geom(g, axis);
    if (chain) q.nj = pion::proj_part_along_slab(g, axis) ? q.nj : slab.global_planes;
    img.assign((size_t)pion::proj_count(q, nfields), 0.0);
  }
  if (!chain) rc = project_images(axis, nfields, fields, nullptr, (long)img.size(), img.data());
  else {
    // global_xmin: the header's Xmin (snapshot_io.cpp: global_view), equal to the single grid's where dx and xmin are dyadic
    const pion_gpu_proj_part part = {slab.plane_lo, slab.global_planes, comm_->rank() == comm_->world() - 1 ? 1 : 0,
                                     cfg.xmin[cfg.ndim - 1] - slab.plane_lo * cfg.dx};
    rc = relay_part(rc, axis, nfields, fields, part, img);
    if (rc || !part.last) return rc;
    // the header of a single-rank sim of the whole problem: nothing rank-local
    for (snapshot_param &p : params) {
      if (p.key == "pion_rank" || p.key == "pion_slab_lo") p.value = "0";
      if (p.key == "pion_world") p.value = "1";
      if (p.key == "pion_slab_n") p.value = std::to_string(slab.global_planes);
    }
  }
  if (rc) return rc;
  params.push_back({"pion_proj_axis", std::to_string(axis), 'i'});
  // 2. the file
  return write_image_file("write_projection", path, io_error_, params, nfields, fields, q.ni, q.nj, img);
}

// ---- the inclined projection of a (z,R) grid (dev_project_angle.h)
int sim_control_gpu::projection_angle_refused(double angle_deg, int nfields, const pion_gpu_proj_field *fields, const char *who)
{
  const char *why = nullptr;
  if (slab.set || (comm_ && comm_->world() > 1))
    why = "project_angle: this sim is one rank of several, and rays are not carried from rank to rank";
  pion::AngleGeom q;
  if (!why) why = pion::angle_refused(grid_desc(cfg), cfg, angle_deg, nfields, &q);
  if (!why) why = pion::proj_refused_fields(pion::out_cfg(cfg), nfields, fields);
  if (!why) return 0;
  io_error_ = std::string(who) + ": " + why;
  return PION_GPU_EINVAL;
}

int sim_control_gpu::set_projection_angle_output(double angle_deg, int nfields, const pion_gpu_proj_field *fields)
{
  io_error_.clear();
  if (nfields == 0) {
    proja_fields_.clear();
    return 0;
  }
  if (int rc = projection_angle_refused(angle_deg, nfields, fields, "set_projection_angle_output")) return rc;
  proja_angle_ = angle_deg;
  proja_fields_.assign(fields, fields + nfields);
  return 0;
}

int sim_control_gpu::write_projection_angle(const char *path, double angle_deg, int nfields, const pion_gpu_proj_field *fields,
                                            int trip_limit)
{
  const char *who = "write_projection_angle";
  if (int rc = path_refused(who, path)) return rc;
  if (int rc = projection_angle_refused(angle_deg, nfields, fields, who)) return rc;
  if (trip_limit < 0) {
    io_error_ = std::string(who) + ": the trip limit is not negative";
    return PION_GPU_EINVAL;
  }
  std::vector<snapshot_param> params;
  long nloc = 0;
  if (int rc = writer_params(who, params, nloc)) return rc;

  // 1. the images, native doubles [nfields][NR][NI]
  const pion::GridDesc g = grid_desc(cfg);
  pion::AngleGeom q;
  (void)pion::angle_refused(g, cfg, angle_deg, nfields, &q);
  const long n = pion::angle_count(q, nfields);
  std::vector<double> img((size_t)n, 0.0);
  long ncapped = 0;
  if (trip_limit == 0 && be_->project_angle_count && be_->project_angle_to_host) {
    int n_extra = -1;
    if (be_->project_angle_count(h_, angle_deg, nfields, &n_extra) != n || n_extra != q.n_extra) {
      io_error_ = std::string(who) + ": the backend refuses: " + last_error();
      return PION_GPU_EINVAL;
    }
    if (int rc = be_->project_angle_to_host(h_, angle_deg, nfields, fields, img.data(), &ncapped)) {
      io_error_ = std::string(who) + ": project_angle_to_host failed: " + last_error();
      return rc;
    }
  }
  else {
    std::vector<double> A((size_t)cfg.nvar * g.ncell);
    if (int rc = be_->download(h_, 0, A.data())) {
      io_error_ = std::string(who) + ": download failed: " + last_error();
      return rc;
    }
    ncapped = project_angle_on_host(g, pion::out_cfg(cfg), q, nfields, fields, A.data(),
                                    trip_limit ? trip_limit : pion::angle_trip_limit(q), img.data());
  }
  if (ncapped) {
    io_error_ = std::string(who) + ": " + std::to_string(ncapped) + " pixel(s) reached the trip limit of their ray loop: "
                "the image is not complete and no file is written";
    return PION_GPU_EINVAL;
  }
  double tn, invst, st;
  pion::angle_numbers(angle_deg, &tn, &invst, &st);
  params.push_back({"pion_proj_angle", fmt_d(angle_deg), 'd'});
  params.push_back({"pion_proj_n_extra", std::to_string(q.n_extra), 'i'});
  params.push_back({"pion_proj_pixdx", fmt_d(q.dx * st), 'd'});                        // project2D.cpp:449
  params.push_back({"pion_proj_pixz0", fmt_d(pion::angle_pos_z(q, 0) * st), 'd'});     // project2D.cpp:446-447
  return write_image_file(who, path, io_error_, params, nfields, fields, q.ni, q.nr, img);
}

// ---- C view of dev_project.h's host functions (ctypes: tests; a caller that assembles images with a transport of its
// own and no device): no sim, no backend -- a configuration and a whole array [nvar][ncell_all]
extern "C" {
// null, or the text with which pion_gpu_project_part refuses these arguments (`img`: the caller's image buffer)
const char *pion_host_project_part_refused(const pion_gpu_config *cfg, int axis, int nfields, const pion_gpu_proj_field *fields,
                                           const pion_gpu_proj_part *part, const void *img)
{
  if (!cfg) return "project: no configuration";
  const pion::GridDesc g = grid_desc(*cfg);
  const char *why = pion::proj_refused_grid(g, axis);
  if (!why) why = pion::proj_refused_fields(pion::out_cfg(*cfg), nfields, fields);
  if (!why) why = pion::proj_refused_part(g, part);
  if (!why && !img) why = "project: no buffer";
  return why;
}
// proj_column / abel_column over every pixel: img = [nfields][NJ][NI]
int pion_host_project_on_host(const pion_gpu_config *cfg, int axis, int nfields, const pion_gpu_proj_field *fields,
                              const double *A, double *img)
{
  if (!cfg || !A || !img) return PION_GPU_EINVAL;
  const pion::GridDesc g = grid_desc(*cfg);
  if (pion::proj_refused_grid(g, axis) || pion::proj_refused_fields(pion::out_cfg(*cfg), nfields, fields)) return PION_GPU_EINVAL;
  project_on_host(g, pion::out_cfg(*cfg), axis, nfields, fields, A, img);
  return 0;
}
// proj_column_part / abel_column_part: this grid's part added into img = [nfields][NJ_global][NI_global] (in/out)
int pion_host_project_part_on_host(const pion_gpu_config *cfg, int axis, int nfields, const pion_gpu_proj_field *fields,
                                   const pion_gpu_proj_part *part, const double *A, double *img)
{
  if (!A || pion_host_project_part_refused(cfg, axis, nfields, fields, part, img)) return PION_GPU_EINVAL;
  const pion::ProjPart pp = {part->plane_lo, part->global_planes, part->last ? 1 : 0, part->global_xmin};
  project_part_on_host(grid_desc(*cfg), pion::out_cfg(*cfg), axis, nfields, fields, pp, A, img);
  return 0;
}
// dev_project_angle.h: the count, and angle_pixel over every pixel
long pion_host_project_angle_count(const pion_gpu_config *cfg, double angle_deg, int nfields, int *n_extra, const char **why)
{
  if (why) *why = nullptr;
  if (!cfg) return PION_GPU_EINVAL;
  pion::AngleGeom q;
  if (const char *w = pion::angle_refused(grid_desc(*cfg), *cfg, angle_deg, nfields, &q)) {
    if (why) *why = w;
    return PION_GPU_EINVAL;
  }
  if (n_extra) *n_extra = q.n_extra;
  return pion::angle_count(q, nfields);
}
// trip_limit 0: the rule's own
static int angle_rule(const pion_gpu_config *cfg, double angle_deg, int trip_limit, int nfields, const pion_gpu_proj_field *fields,
                      const double *A, double *img, long *ncapped, double *tan_angle, double *inv_sin)
{
  if (!cfg || !A || !img) return PION_GPU_EINVAL;
  const pion::GridDesc g = grid_desc(*cfg);
  pion::AngleGeom q;
  if (pion::angle_refused(g, *cfg, angle_deg, nfields, &q) || pion::proj_refused_fields(pion::out_cfg(*cfg), nfields, fields))
    return PION_GPU_EINVAL;
  if (tan_angle) *tan_angle = q.tn;
  if (inv_sin) *inv_sin = q.invst;
  const long n = project_angle_on_host(g, pion::out_cfg(*cfg), q, nfields, fields, A,
                                       trip_limit ? trip_limit : pion::angle_trip_limit(q), img);
  if (ncapped) *ncapped = n;
  return 0;
}
int pion_host_project_angle_rule(const pion_gpu_config *cfg, double angle_deg, int trip_limit, int nfields,
                                 const pion_gpu_proj_field *fields, const double *A, double *img, long *ncapped,
                                 double *tan_angle, double *inv_sin)
{
  if (!ncapped || trip_limit < 1) return PION_GPU_EINVAL;
  return angle_rule(cfg, angle_deg, trip_limit, nfields, fields, A, img, ncapped, tan_angle, inv_sin);
}
int pion_host_project_angle_on_host(const pion_gpu_config *cfg, double angle_deg, int nfields, const pion_gpu_proj_field *fields,
                                    const double *A, double *img)
{
  return angle_rule(cfg, angle_deg, 0, nfields, fields, A, img, nullptr, nullptr, nullptr);
}
}

}  // namespace pion_host
