// columns_io.cpp -- ray-traced column densities of the C++ host loop (sim_control_gpu::add_rt_source,
// set_column_output, write_columns; the rules: pion_amd/csrc/dev_raytrace.h).  The file is a FITS file of fits_io.h's
// kind: the primary header of write_fits with RT_Nsources and, per source n, RT_position_<n>_<d>, RT_at_infty_<n>,
// RT_Opacity__<n>, RT_Tau_var__<n> appended, then per source the images Col_Src_<n>_T0 and DCol_Src_<n>_T0 of the
// on-grid cells, traced on the device and streamed image after image, a chunk of planes at a time (backend entries
// raytrace / rt_count / columns_to_host_begin), or by pion_gpu_raytrace_host on a downloaded array where the table has
// no such entries.
//
// One rank of a slab run (a slab extent AND a communicator of more than one rank that relays both ways): the calls are
// collective.  Sources are given at positions of the WHOLE domain (dev_raytrace.h, "a part").  write_columns takes the
// sources in id order and for each one receives the plane of col its role names (rt_role), traces, and sends its own
// lowest / highest plane on; then every rank writes its own file with its own planes.  The invariant that keeps every
// rank from waiting for ever: whatever happened before, a rank ALWAYS takes the message its role names and ALWAYS sends
// the ones its role names -- the plane, or a failure.  A failure travels away from the source only, so the ranks then
// agree (agree_on): one status word up the chain and one down, and no rank keeps a file if any rank failed.
#include <algorithm>
#include <memory>
#include <string>
#include <vector>

#include "dev_rules.h"
#include "fits_io.h"
#include "sim_control_gpu.h"
#include "slab_comm.h"

namespace pion_host {

bool sim_control_gpu::columns_collective() const
{
  return slab.set && comm_ && comm_->world() > 1 && comm_->has_relay() && comm_->has_relay_down();
}

// global_xmin: the header's Xmin (snapshot_io.cpp: global_view), equal to the single grid's where dx and xmin are dyadic
pion_gpu_rt_part sim_control_gpu::columns_part() const
{
  const pion_gpu_rt_part part = {slab.plane_lo, slab.global_planes, cfg.xmin[cfg.ndim - 1] - slab.plane_lo * cfg.dx};
  return part;
}

int sim_control_gpu::columns_refused(const char *who)
{
  const char *why = nullptr;
  const bool chain = columns_collective();
  if ((slab.set || (comm_ && comm_->world() > 1)) && !chain)
    why = "raytrace: this sim is one rank of a slab run without both a slab extent and a communicator of more than one rank "
          "that hands planes up and down, and columns are handed from rank to rank along it";
  else if (!rt_sources_.empty() && rt_as_parts_ != chain)
    why = "raytrace: this sim became one rank of a slab run after its sources were added (set the slab extent and the "
          "communicator first)";
  if (!why) return 0;
  io_error_ = std::string(who) + ": " + why;
  return PION_GPU_EINVAL;
}

int sim_control_gpu::add_rt_source(const pion_gpu_rt_source &src, int *id, double *pos_used)
{
  io_error_.clear();
  if (int rc = columns_refused("add_rt_source")) return rc;
  const bool chain = columns_collective();
  const pion_gpu_rt_part part = columns_part();
  if (const char *why = chain ? pion::rt_part_refused(cfg, &src, &part) : pion::rt_refused(cfg, &src)) {
    io_error_ = std::string("add_rt_source: ") + why;
    return PION_GPU_EINVAL;
  }
  if (rt_sources_.size() >= PION_MAX_RT_SOURCES) {
    io_error_ = "add_rt_source: raytrace: more than PION_MAX_RT_SOURCES (4) sources";
    return PION_GPU_EINVAL;
  }
  pion_gpu_rt_source moved = src;
  double used[PION_MAX_DIM];
  const bool on_backend = chain ? (be_->add_rt_source_part && be_->raytrace_part_faces) : (be_->add_rt_source != nullptr);
  if (on_backend) {
    int i = -1;
    if (int rc = chain ? be_->add_rt_source_part(h_, &src, &part, &i, used) : be_->add_rt_source(h_, &src, &i, used)) {
      io_error_ = "add_rt_source: the backend refuses: " + last_error();
      return rc;
    }
    rt_on_backend_ = true;
  }
  else (void)pion::rt_make_source(cfg, src, used, chain ? &part : nullptr);
  for (int a = 0; a < PION_MAX_DIM; a++) {
    moved.pos[a] = used[a];
    if (pos_used) pos_used[a] = used[a];
  }
  rt_sources_.push_back(src);
  rt_moved_.push_back(moved);
  rt_as_parts_ = chain;
  if (id) *id = (int)rt_sources_.size() - 1;
  return 0;
}

// One source of a slab run: receive, trace, send (the invariant above).  rc: what this rank arrives with.  on_device:
// traced by the backend into its own arrays; else from the downloaded array A into col, dcol.
int sim_control_gpu::relay_columns(int rc, int id, bool on_device, const double *A, double *col, double *dcol)
{
  const pion_gpu_rt_part part = columns_part();
  const pion::RtRole role = pion::rt_role(cfg, rt_sources_[(size_t)id], part);
  const pion::GridDesc g = grid_desc(cfg);
  const long plane = (cfg.ndim == 3) ? (long)g.ng[0] * g.ng[1] : (long)g.ng[0], nloc = g.ng[cfg.ndim - 1];
  const size_t bytes = (size_t)plane * sizeof(double);
  std::vector<double> in((size_t)plane), lo((size_t)plane), hi((size_t)plane);
  if (role.recv_side != PION_RT_RECV_NONE) {
    const bool below = role.recv_side == PION_RT_RECV_BELOW;
    int st = 0;
    // (refused here: the message is taken off the wire without a buffer)
    const int rrc = below ? comm_->recv_from_below(rc ? nullptr : in.data(), bytes, &st)
                          : comm_->recv_from_above(rc ? nullptr : in.data(), bytes, &st);
    if (!rc && st) {
      io_error_ = "write_columns: a rank nearer the source failed, no file is written";
      rc = PION_GPU_EINVAL;
    }
    if (!rc && rrc) {
      io_error_ = "write_columns: receiving the plane of the neighbouring rank failed: " + comm_->last_error();
      rc = rrc;
    }
  }
  if (!rc) {
    const double *fin = (role.recv_side != PION_RT_RECV_NONE) ? in.data() : nullptr;
    if (on_device) {
      rc = be_->raytrace_part_faces(h_, 0, id, fin, role.send_lo ? lo.data() : nullptr, role.send_hi ? hi.data() : nullptr);
      if (rc) io_error_ = "write_columns: tracing the part failed: " + last_error();
    }
    else if (pion_gpu_raytrace_host_part(&cfg, &rt_sources_[(size_t)id], &part, A, fin, col, dcol)) {
      io_error_ = "write_columns: pion_gpu_raytrace_host_part refuses the source";
      rc = PION_GPU_EINVAL;
    }
    else {
      std::copy(col, col + plane, lo.begin());
      std::copy(col + (nloc - 1) * plane, col + nloc * plane, hi.begin());
    }
  }
  int src = 0;
  if (role.send_lo) src = comm_->send_to_below(rc ? nullptr : lo.data(), bytes, rc ? 1 : 0);
  if (role.send_hi) {
    const int s2 = comm_->send_to_above(rc ? nullptr : hi.data(), bytes, rc ? 1 : 0);
    if (!src) src = s2;
  }
  if (!rc && src) {
    io_error_ = "write_columns: handing the plane to the neighbouring rank failed: " + comm_->last_error();
    rc = src;
  }
  return rc;
}

// every rank learns whether any rank failed: a status word from rank 0 upwards, gathering, and from the last rank down
int sim_control_gpu::agree_on(int rc)
{
  long long word = 0;
  int st = 0;
  int bad = rc;
  if (comm_->recv_from_below(&word, sizeof word, &st) || st) bad = bad ? bad : PION_GPU_EINVAL;
  if (comm_->send_to_above(bad ? nullptr : &word, sizeof word, bad ? 1 : 0)) bad = bad ? bad : PION_GPU_EINVAL;
  st = 0;
  if (comm_->recv_from_above(&word, sizeof word, &st) || st) bad = bad ? bad : PION_GPU_EINVAL;
  if (comm_->send_to_below(bad ? nullptr : &word, sizeof word, bad ? 1 : 0)) bad = bad ? bad : PION_GPU_EINVAL;
  if (bad && !rc) io_error_ = "write_columns: another rank failed, no file is written";
  return bad;
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
  io_error_.clear();
  if (int rc = columns_refused("write_columns")) return rc;
  if (rt_sources_.empty()) {
    io_error_ = "write_columns: raytrace: the sim has no radiation source (add_rt_source)";
    return PION_GPU_EINVAL;
  }
  // one rank of a slab run: the call is collective from here on, whatever fails (the two refusals above depend on
  // what every rank was set up with, not on this call)
  const bool chain = columns_collective();
  std::vector<snapshot_param> params;
  long nloc = 0;
  int rc = path_refused("write_columns", path);
  if (!rc) rc = writer_params("write_columns", params, nloc);
  if (rc && !chain) return rc;
  const pion::GridDesc g = grid_desc(cfg);
  const pion::OutGeom q = pion::out_geom(g);
  const int nsrc = (int)rt_sources_.size(), nimage = 2 * nsrc;
  const long plane = (long)q.rows * q.nx;
  if (rc) nloc = g.ng[cfg.ndim - 1];
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

  std::unique_ptr<PartFile> file;   // (none where the call has failed already: a collective call goes on without it)
  if (!rc) {
    file.reset(new PartFile("write_columns", path, io_error_));
    if (!file->ok()) {
      if (!chain) return PION_GPU_EINVAL;
      rc = PION_GPU_EINVAL;
    }
  }
  PartFile *const fp = file.get();
  if (!rc) rc = L.start(*fp);
  const bool device = rt_on_backend_ && be_->rt_count && be_->columns_to_host_begin && be_->ongrid_to_host_end
                      && (chain ? be_->raytrace_part_faces != nullptr : be_->raytrace != nullptr);
  if (device) {
    // traced on the device; then image-major, a job one chunk of planes of one image
    if (chain)
      for (int n = 0; n < nsrc; n++) rc = relay_columns(rc, n, true, nullptr, nullptr, nullptr);
    else if (!rc) rc = be_->raytrace(h_, 0);
    if (!rc) {
      const long cp = chunk_planes(be_->rt_count(h_, 1), nloc), nchunk = (nloc + cp - 1) / cp;
      auto begin = [&](long job, int slot) {
        const long i = job / nchunk, a = (job % nchunk) * cp;
        return be_->columns_to_host_begin(h_, (int)(i / 2), (int)(i & 1), (int)a, (int)std::min(nloc, a + cp), slot);
      };
      auto put = [&](long job, const double *src) {
        const long i = job / nchunk, a = (job % nchunk) * cp, b = std::min(nloc, a + cp);
        return fp->write(src, (size_t)((b - a) * plane) * sizeof(double), L.data_at(i) + a * plane * (long)sizeof(double));
      };
      rc = stream_jobs(nimage * nchunk, begin, put);
    }
    if (rc && io_error_.empty() && !last_error().empty()) io_error_ = "write_columns: tracing or staging the planes failed: " + last_error();
  }
  else {
    // no entries: array 0 whole, traced by the same rules in a host loop, swapped here
    std::vector<double> A((size_t)cfg.nvar * g.ncell), col((size_t)(nloc * plane)), dcol((size_t)(nloc * plane));
    std::vector<unsigned long long> R((size_t)(nloc * plane));
    if (!rc) {
      rc = be_->download(h_, 0, A.data());
      if (rc) io_error_ = "write_columns: download failed: " + last_error();
    }
    for (int n = 0; n < nsrc && (chain || !rc); n++) {
      if (chain) rc = relay_columns(rc, n, false, A.data(), col.data(), dcol.data());
      else if (pion_gpu_raytrace_host(&cfg, &rt_sources_[(size_t)n], A.data(), col.data(), dcol.data())) {
        io_error_ = "write_columns: pion_gpu_raytrace_host refuses the source";
        rc = PION_GPU_EINVAL;
      }
      for (int w = 0; w < 2 && !rc; w++) {
        const std::vector<double> &src = w ? dcol : col;
        for (size_t k = 0; k < R.size(); k++) R[k] = pion::out_be64(src[k]);
        rc = fp->write(R.data(), (size_t)run_bytes, L.data_at(2 * n + w));
      }
    }
  }
  if (chain) rc = agree_on(rc);
  if (!fp || !fp->ok()) return rc;
  return fp->commit(rc);
}

}  // namespace pion_host
