// fits_io.cpp -- see fits_io.h
#include "fits_io.h"

#include <fcntl.h>
#include <unistd.h>

#include <algorithm>
#include <cerrno>
#include <cstdio>
#include <cstring>

#ifndef __host__
#define __host__
#define __device__
#endif
#include "../csrc/dev_output.h"
#include "sim_control_gpu.h"
#include "snapshot_io.h"

namespace pion_host {

namespace {

const long BLOCK = 2880, CARD = 80;

long padded(long n) { return (n + BLOCK - 1) / BLOCK * BLOCK; }

void card(std::string &h, std::string c)
{
  c.resize((size_t)CARD, ' ');
  h += c;
}
// a mandatory keyword in fixed format: the value right-justified in columns 11-30
void fixed(std::string &h, const char *key, const std::string &value)
{
  char b[96];
  snprintf(b, sizeof b, "%-8s= %20s", key, value.c_str());
  card(h, b);
}
// a character string in fixed format: the opening quote in column 11, the closing one in column 20 or later
void fixed_string(std::string &h, const char *key, const std::string &value)
{
  char b[96];
  snprintf(b, sizeof b, "%-8s= '%-8s'", key, value.c_str());
  card(h, b);
}
void finish(std::string &h)
{
  card(h, "END");
  h.resize((size_t)padded((long)h.size()), ' ');
}

// %.17G reads back bit for bit; a value printed without '.' or exponent gets its decimal point (a FITS real)
std::string fits_double(const std::string &g17)
{
  char b[64];
  snprintf(b, sizeof b, "%.17G", strtod(g17.c_str(), nullptr));
  std::string s = b;
  if (s.find_first_of(".EN") == std::string::npos) s += ".";
  return s;
}

// HIERARCH <name> = '<text>': quotes doubled; a text too long for the card goes on in CONTINUE cards, each piece but
// the last ending in '&'
void hierarch_string(std::string &h, const std::string &name, const std::string &text)
{
  std::vector<std::string> tok;
  for (const char ch : text) tok.push_back(ch == '\'' ? std::string("''") : std::string(1, ch));
  const std::string first = "HIERARCH " + name + " = ", cont = "CONTINUE  ";
  const std::string *lead = &first;
  size_t i = 0;
  do {
    const size_t room = (size_t)CARD - lead->size() - 2;   // between the quotes
    size_t rest = 0;
    for (size_t k = i; k < tok.size(); k++) rest += tok[k].size();
    std::string piece;
    if (rest <= room)
      while (i < tok.size()) piece += tok[i++];
    else {
      while (piece.size() + tok[i].size() <= room - 1) piece += tok[i++];
      piece += '&';
    }
    card(h, *lead + "'" + piece + "'");
    lead = &cont;
  } while (i < tok.size());
}

void hierarch(std::string &h, const std::string &name, const std::string &value, char type)
{
  if (type == 's') hierarch_string(h, name, value);
  else card(h, "HIERARCH " + name + " = " + (type == 'd' ? fits_double(value) : value));
}

// the grid as dev_output.h's functions see it (pion_gpu_create's GridDesc)
pion::GridDesc grid_desc(const pion_gpu_config &c)
{
  pion::GridDesc g;
  g.ndim = c.ndim;
  g.ncell = 1;
  for (int a = 0; a < 3; a++) {
    g.ng[a] = (a < c.ndim) ? c.ng[a] : 1;
    g.nbc[a] = (a < c.ndim) ? c.nbc : 0;
    g.nga[a] = g.ng[a] + 2 * g.nbc[a];
    g.ncell *= g.nga[a];
    g.xmin[a] = c.xmin[a];
  }
  g.sy = g.nga[0];
  g.sz = (long)g.nga[0] * g.nga[1];
  g.dx = c.dx;
  g.cyl = (c.coord_sys == 2) ? 1 : ((c.coord_sys == 3) ? 2 : 0);
  g.sph_vol = nullptr;
  return g;
}

}  // namespace

std::string fits_primary_header(const std::vector<snapshot_param> &params)
{
  std::string h;
  fixed(h, "SIMPLE", "T");
  fixed(h, "BITPIX", "-64");
  fixed(h, "NAXIS", "0");
  fixed(h, "EXTEND", "T");
  for (const snapshot_param &p : params) {
    // an array: element-numbered names (write_header_param of the reference)
    const bool array = (p.type != 's' && p.value.find(' ') != std::string::npos);
    if (!array) {
      hierarch(h, p.key, p.value, p.type);
      continue;
    }
    size_t pos = 0;
    for (int i = 0; pos <= p.value.size(); i++) {
      const size_t e = std::min(p.value.find(' ', pos), p.value.size());
      hierarch(h, p.key + std::to_string(i), p.value.substr(pos, e - pos), p.type);
      pos = e + 1;
    }
  }
  finish(h);
  return h;
}

std::string fits_image_header(const char *extname, int ndim, const long *naxis)
{
  std::string h;
  fixed_string(h, "XTENSION", "IMAGE");
  fixed(h, "BITPIX", "-64");
  fixed(h, "NAXIS", std::to_string(ndim));
  for (int a = 0; a < ndim; a++) fixed(h, ("NAXIS" + std::to_string(a + 1)).c_str(), std::to_string(naxis[a]));
  fixed(h, "PCOUNT", "0");
  fixed(h, "GCOUNT", "1");
  fixed_string(h, "EXTNAME", extname);
  finish(h);
  return h;
}

int sim_control_gpu::write_fits(const char *path)
{
  io_error_.clear();
  if (!path || !*path) {
    io_error_ = "write_fits: no path";
    return PION_GPU_EINVAL;
  }
  if (cfg.ntracer > pion::OUT_MAX_TRACERS) {
    io_error_ = "write_fits: only accepts <= 5 tracers (this sim has " + std::to_string(cfg.ntracer) + ")";
    return PION_GPU_EINVAL;
  }
  std::vector<snapshot_param> params;
  long nloc = 0;
  if (int rc = snapshot_params(params, nloc)) return rc;
  if (int rc = finish_halo()) {
    io_error_ = "write_fits: finish_halo failed";
    return rc;
  }
  const pion::GridDesc g = grid_desc(cfg);
  const pion::OutputCfg o = pion::out_cfg(cfg);
  const pion::OutGeom q = pion::out_geom(g);
  const int nimage = pion::out_nimage(o);
  const long plane = (long)q.rows * q.nx;
  const long naxis[3] = {q.nx, (cfg.ndim == 3) ? (long)q.rows : nloc, nloc};

  // 1. the header blocks; every extension's header has the same length
  const std::string primary = fits_primary_header(params);
  std::vector<std::string> ext((size_t)nimage);
  for (int i = 0; i < nimage; i++) {
    char name[pion::OUT_NAME_LEN];
    pion::out_image_name(o, i, name);
    ext[i] = fits_image_header(name, cfg.ndim, naxis);
  }
  const long run_bytes = nloc * plane * (long)sizeof(double);
  const long stride = (long)ext[0].size() + padded(run_bytes);   // from one image's data to the next one's
  const long off = (long)primary.size() + (long)ext[0].size();   // the first image's data
  const long total = (long)primary.size() + nimage * stride;

  const std::string tmp = std::string(path) + ".part";
  int fd = open(tmp.c_str(), O_WRONLY | O_CREAT | O_TRUNC, 0644);
  if (fd < 0) {
    io_error_ = "write_fits: cannot create " + tmp + ": " + strerror(errno);
    return PION_GPU_EINVAL;
  }
  // 3. (first) the file at its full length: what no write below covers -- the padding after each data unit -- reads
  // as zero bytes
  int rc = (ftruncate(fd, (off_t)total) != 0) ? PION_GPU_EINVAL : 0;
  if (!rc && full_pwrite(fd, primary.data(), primary.size(), 0)) rc = PION_GPU_EINVAL;
  for (int i = 0; i < nimage && !rc; i++)
    if (full_pwrite(fd, ext[i].data(), ext[i].size(), (off_t)((long)primary.size() + i * stride))) rc = PION_GPU_EINVAL;
  // 2. the data
  if (!rc && be_->fits_to_host_begin && be_->fits_count && be_->ongrid_to_host_end)
    rc = stream_runs(fd, true, nimage, nloc, plane, off, stride, "write_fits");
  else if (!rc) {
    // no streaming entries: array 0 whole, the images evaluated and swapped here
    std::vector<double> A((size_t)cfg.nvar * g.ncell);
    std::vector<unsigned long long> R((size_t)(nloc * plane));
    rc = be_->download(h_, 0, A.data());
    if (rc) io_error_ = "write_fits: download failed: " + last_error();
    for (int i = 0; i < nimage && !rc; i++) {
      const pion::OutImage im = pion::out_image(o, i);
      for (long k = 0; k < nloc; k++)
        for (long j = 0; j < q.rows; j++) {
          const long c0 = pion::out_row_cell(q, k, j), b0 = pion::out_row_buf(q, 0, nloc, k, j);
          const int jy = pion::out_row_jy(g, k, j);
          for (long ix = 0; ix < q.nx; ix++) R[(size_t)(b0 + ix)] = pion::out_be64(pion::out_value(g, o, im, A.data(), c0 + ix, jy));
        }
      if (full_pwrite(fd, R.data(), (size_t)run_bytes, (off_t)(off + i * stride))) rc = PION_GPU_EINVAL;
    }
  }
  if (rc && io_error_.empty()) io_error_ = "write_fits: writing " + tmp + " failed: " + strerror(errno);
  close(fd);
  // 4.
  if (!rc && rename(tmp.c_str(), path) != 0) {
    io_error_ = std::string("write_fits: cannot rename to ") + path + ": " + strerror(errno);
    rc = PION_GPU_EINVAL;
  }
  if (rc) unlink(tmp.c_str());
  return rc;
}

}  // namespace pion_host
