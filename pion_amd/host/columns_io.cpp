// columns_io.cpp -- ray-traced column densities of the C++ host loop (sim_control_gpu::add_rt_source,
// set_column_output, write_columns; the rules: pion_amd/csrc/dev_raytrace.h).  The file is a FITS file of fits_io.h's
// kind: the primary header of write_fits with RT_Nsources and, per source n, RT_position_<n>_<d>, RT_at_infty_<n>,
// RT_Opacity__<n>, RT_Tau_var__<n> appended, then per source the images Col_Src_<n>_T0 and DCol_Src_<n>_T0 of the
// on-grid cells, traced on the device and streamed image after image, a chunk of planes at a time (backend entries
// raytrace / rt_count / columns_to_host_begin), or by pion_gpu_raytrace_host on a downloaded array where the table has
// no such entries.
#include <algorithm>
#include <string>
#include <vector>

#include "dev_rules.h"
#include "fits_io.h"
#include "sim_control_gpu.h"
#include "slab_comm.h"

namespace pion_host {

int sim_control_gpu::columns_refused(const char *who)
{
  const char *why = nullptr;
  if (slab.set || (comm_ && comm_->world() > 1))
    why = "raytrace: this sim is one rank of a slab run, and columns are not handed from rank to rank";
  if (!why) return 0;
  io_error_ = std::string(who) + ": " + why;
  return PION_GPU_EINVAL;
}

int sim_control_gpu::add_rt_source(const pion_gpu_rt_source &src, int *id, double *pos_used)
{
  io_error_.clear();
  if (int rc = columns_refused("add_rt_source")) return rc;
  if (const char *why = pion::rt_refused(cfg, &src)) {
    io_error_ = std::string("add_rt_source: ") + why;
    return PION_GPU_EINVAL;
  }
  if (rt_sources_.size() >= PION_MAX_RT_SOURCES) {
    io_error_ = "add_rt_source: raytrace: more than PION_MAX_RT_SOURCES (4) sources";
    return PION_GPU_EINVAL;
  }
  pion_gpu_rt_source moved = src;
  double used[PION_MAX_DIM];
  if (be_->add_rt_source) {
    int i = -1;
    if (int rc = be_->add_rt_source(h_, &src, &i, used)) {
      io_error_ = "add_rt_source: the backend refuses: " + last_error();
      return rc;
    }
    rt_on_backend_ = true;
  }
  else (void)pion::rt_make_source(cfg, src, used);
  for (int a = 0; a < PION_MAX_DIM; a++) {
    moved.pos[a] = used[a];
    if (pos_used) pos_used[a] = used[a];
  }
  rt_sources_.push_back(src);
  rt_moved_.push_back(moved);
  if (id) *id = (int)rt_sources_.size() - 1;
  return 0;
}

int sim_control_gpu::set_column_output(int on)
{
  io_error_.clear();
  if (!on) {
    column_output_ = false;
    return 0;
  }
  if (int rc = columns_refused("set_column_output")) return rc;
  if (rt_sources_.empty()) {
    io_error_ = "set_column_output: raytrace: the sim has no radiation source (add_rt_source)";
    return PION_GPU_EINVAL;
  }
  column_output_ = true;
  return 0;
}

int sim_control_gpu::write_columns(const char *path)
{
  if (int rc = path_refused("write_columns", path)) return rc;
  if (int rc = columns_refused("write_columns")) return rc;
  if (rt_sources_.empty()) {
    io_error_ = "write_columns: raytrace: the sim has no radiation source (add_rt_source)";
    return PION_GPU_EINVAL;
  }
  std::vector<snapshot_param> params;
  long nloc = 0;
  if (int rc = writer_params("write_columns", params, nloc)) return rc;
  const pion::GridDesc g = grid_desc(cfg);
  const pion::OutGeom q = pion::out_geom(g);
  const int nsrc = (int)rt_sources_.size(), nimage = 2 * nsrc;
  const long plane = (long)q.rows * q.nx;
  const long naxis[3] = {q.nx, (cfg.ndim == 3) ? (long)q.rows : nloc, nloc};

  // the sources, under the reference's names (set_rt_src_params, dataio_base.cpp:1267-1282)
  params.push_back({"RT_Nsources", std::to_string(nsrc), 'i'});
  for (int n = 0; n < nsrc; n++) {
    const pion_gpu_rt_source &s = rt_moved_[(size_t)n];
    const std::string k = std::to_string(n);
    std::string pos;
    for (int a = 0; a < PION_MAX_DIM; a++) {
      double p = s.pos[a];
      if (s.at_infinity) p = (a == s.dir / 2) ? ((s.dir & 1) ? 1.0e200 : -1.0e200) : 0.0;
      pos += (a ? " " : "") + fmt_d(p);
    }
    params.push_back({"RT_position_" + k + "_", pos, 'd'});
    params.push_back({"RT_at_infty_" + k, std::to_string(s.at_infinity ? 1 : 0), 'i'});
    params.push_back({"RT_Opacity__" + k, std::to_string(s.opacity), 'i'});
    params.push_back({"RT_Tau_var__" + k, std::to_string(s.opacity_var), 'i'});
  }

  const std::string primary = fits_primary_header(params);
  std::vector<std::string> ext((size_t)nimage);
  for (int i = 0; i < nimage; i++) {
    const std::string name = std::string((i & 1) ? "DCol_Src_" : "Col_Src_") + std::to_string(i / 2) + "_T0";
    ext[(size_t)i] = fits_image_header(name.c_str(), cfg.ndim, naxis);
  }
  const long run_bytes = nloc * plane * (long)sizeof(double);
  const fits_layout L(primary, ext, run_bytes);

  PartFile f("write_columns", path, io_error_);
  if (!f.ok()) return PION_GPU_EINVAL;
  int rc = L.start(f);
  if (!rc && rt_on_backend_ && be_->raytrace && be_->rt_count && be_->columns_to_host_begin && be_->ongrid_to_host_end) {
    // traced on the device; then image-major, a job one chunk of planes of one image
    const long cp = chunk_planes(be_->rt_count(h_, 1), nloc), nchunk = (nloc + cp - 1) / cp;
    auto begin = [&](long job, int slot) {
      const long i = job / nchunk, a = (job % nchunk) * cp;
      return be_->columns_to_host_begin(h_, (int)(i / 2), (int)(i & 1), (int)a, (int)std::min(nloc, a + cp), slot);
    };
    auto put = [&](long job, const double *src) {
      const long i = job / nchunk, a = (job % nchunk) * cp, b = std::min(nloc, a + cp);
      return f.write(src, (size_t)((b - a) * plane) * sizeof(double), L.data_at(i) + a * plane * (long)sizeof(double));
    };
    rc = be_->raytrace(h_, 0);
    if (!rc) rc = stream_jobs(nimage * nchunk, begin, put);
    if (rc && io_error_.empty() && !last_error().empty()) io_error_ = "write_columns: tracing or staging the planes failed: " + last_error();
  }
  else if (!rc) {
    // no entries: array 0 whole, traced by the same rules in a host loop, swapped here
    std::vector<double> A((size_t)cfg.nvar * g.ncell), col((size_t)(nloc * plane)), dcol((size_t)(nloc * plane));
    std::vector<unsigned long long> R((size_t)(nloc * plane));
    rc = be_->download(h_, 0, A.data());
    if (rc) io_error_ = "write_columns: download failed: " + last_error();
    for (int n = 0; n < nsrc && !rc; n++) {
      if (pion_gpu_raytrace_host(&cfg, &rt_sources_[(size_t)n], A.data(), col.data(), dcol.data())) {
        io_error_ = "write_columns: pion_gpu_raytrace_host refuses the source";
        rc = PION_GPU_EINVAL;
      }
      for (int w = 0; w < 2 && !rc; w++) {
        const std::vector<double> &src = w ? dcol : col;
        for (size_t k = 0; k < R.size(); k++) R[k] = pion::out_be64(src[k]);
        rc = f.write(R.data(), (size_t)run_bytes, L.data_at(2 * n + w));
      }
    }
  }
  return f.commit(rc);
}

}  // namespace pion_host
