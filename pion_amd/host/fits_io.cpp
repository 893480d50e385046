// fits_io.cpp -- see fits_io.h
#include "fits_io.h"

#include <fcntl.h>
#include <unistd.h>

#include <algorithm>
#include <cerrno>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>

#ifndef __host__
#define __host__
#define __device__
#endif
#include "../csrc/dev_output.h"
#include "../csrc/dev_project.h"
#include "../csrc/dev_raytrace.h"
#include "sim_control_gpu.h"
#include "slab_comm.h"
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

// ---- the reader --------------------------------------------------------------------------------------------------
namespace {

struct Card {
  std::string key, value;   // value: a string without its quotes, anything else as the card spells it
  bool is_string;
};
struct Hdu {
  std::vector<Card> cards;
  long data_off = 0, data_bytes = 0;   // the data unit, without its padding
  const Card *find(const char *key) const
  {
    for (const Card &c : cards)
      if (c.key == key) return &c;
    return nullptr;
  }
  // an integer keyword, or dflt where the header has none
  long integer(const char *key, long dflt) const
  {
    const Card *c = find(key);
    return (c && !c->is_string && !c->value.empty()) ? strtol(c->value.c_str(), nullptr, 10) : dflt;
  }
};

std::string trimmed(const std::string &s)
{
  const size_t a = s.find_first_not_of(' '), b = s.find_last_not_of(' ');
  return (a == std::string::npos) ? std::string() : s.substr(a, b - a + 1);
}

// the value field of a card: a quoted string (doubled quotes are quotes, trailing blanks are not significant, a last
// '&' says that a CONTINUE card goes on) or the text up to a comment
void parse_value(const std::string &field, std::string &out, bool &is_string, bool &more)
{
  out.clear();
  is_string = more = false;
  size_t i = field.find_first_not_of(' ');
  if (i == std::string::npos) return;
  if (field[i] != '\'') {
    out = trimmed(field.substr(i, field.find('/', i) - i));
    return;
  }
  is_string = true;
  for (i++; i < field.size(); i++) {
    if (field[i] == '\'') {
      if (i + 1 < field.size() && field[i + 1] == '\'') i++;
      else break;
    }
    out += field[i];
  }
  while (!out.empty() && out.back() == ' ') out.pop_back();
  if (!out.empty() && out.back() == '&') {
    out.pop_back();
    more = true;
  }
}

// one header from byte pos: its cards up to END, and its data unit sized from them; pos moves to the next HDU
int read_hdu(int fd, long size, long &pos, Hdu &H, const char *path, std::string &err)
{
  H = Hdu();
  char block[2880];
  bool end = false, more = false;
  while (!end) {
    if (pos + BLOCK > size || pread(fd, block, (size_t)BLOCK, (off_t)pos) != (ssize_t)BLOCK) {
      err = std::string("FITS file ") + path + ": a header has no END card (the file is truncated, or no FITS file)";
      return PION_GPU_EINVAL;
    }
    pos += BLOCK;
    for (long i = 0; i < BLOCK && !end; i += CARD) {
      const std::string c(block + i, (size_t)CARD);
      std::string key, field;
      if (c.compare(0, 3, "END") == 0 && c.find_first_not_of(' ', 3) == std::string::npos) end = true;
      else if (c.compare(0, 8, "CONTINUE") == 0) {
        if (!more || H.cards.empty()) continue;
        std::string v;
        bool str;
        parse_value(c.substr(8), v, str, more);
        H.cards.back().value += v;
      }
      else {
        const size_t eq = c.find('=');
        if (c.compare(0, 9, "HIERARCH ") == 0 && eq != std::string::npos) key = trimmed(c.substr(9, eq - 9)), field = c.substr(eq + 1);
        else if (c[8] == '=' && c[9] == ' ') key = trimmed(c.substr(0, 8)), field = c.substr(10);
        else {
          more = false;
          continue;   // a comment, a blank card, a card this reader does not know
        }
        Card k;
        k.key = key;
        parse_value(field, k.value, k.is_string, more);
        H.cards.push_back(k);
      }
    }
  }
  // |BITPIX|/8 * GCOUNT * (PCOUNT + prod NAXISn) (FITS standard 4.0, eq. 2)
  const long naxis = H.integer("NAXIS", 0), bitpix = H.integer("BITPIX", 8);
  long n = (naxis > 0) ? 1 : 0;
  bool bad = naxis < 0 || naxis > 999;
  for (long a = 1; a <= naxis && !bad; a++) {
    const long m = H.integer(("NAXIS" + std::to_string(a)).c_str(), -1);
    bad = m < 0 || (m > 0 && n > size / m);   // (more elements than the file has bytes)
    if (!bad) n *= m;
  }
  bad = bad || bitpix < -64 || bitpix > 64;
  const long pcount = H.integer("PCOUNT", 0), gcount = H.integer("GCOUNT", 1), width = bad ? 0 : labs(bitpix) / 8;
  bad = bad || pcount < 0 || gcount < 0 || pcount > size || width > 8 || (gcount > 0 && n + pcount > size / gcount);
  if (!bad) {
    n = gcount * (pcount + n);
    bad = width > 0 && n > size / width;
  }
  if (!bad) {
    H.data_off = pos;
    H.data_bytes = width * n;
    bad = pos + H.data_bytes > size;
  }
  if (bad) {
    err = std::string("FITS file ") + path + " is truncated: the data unit that starts at byte " + std::to_string(pos)
          + " runs past the end of the file, or its header's BITPIX / NAXISn / PCOUNT / GCOUNT make no sense";
    return PION_GPU_EINVAL;
  }
  pos += padded(H.data_bytes);
  return 0;
}

}  // namespace

int fits_read_header(const char *path, snapshot_header &hd, std::vector<long> *image_off, std::string *note,
                     std::string &err)
{
  hd = snapshot_header();
  if (!path) {
    err = "FITS file: no path";
    return PION_GPU_EINVAL;
  }
  const int fd = open(path, O_RDONLY);
  if (fd < 0) {
    err = std::string("FITS file: cannot open ") + path + ": " + strerror(errno);
    return PION_GPU_EINVAL;
  }
  struct Closer {
    int fd;
    ~Closer() { close(fd); }
  } closer{fd};
  const long size = (long)lseek(fd, 0, SEEK_END);
  long pos = 0;
  Hdu P;
  char magic[10] = {0};
  if (size < 9 || pread(fd, magic, 9, 0) != 9 || memcmp(magic, "SIMPLE  =", 9) != 0) {
    err = std::string("FITS file: ") + path + " is not a FITS file (it does not begin with SIMPLE  =)";
    return PION_GPU_EINVAL;
  }
  if (int rc = read_hdu(fd, size, pos, P, path, err)) return rc;
  // the primary header's cards as the PIONRAW2 header's lines; an array's element-numbered cards joined
  for (const Card &c : P.cards) {
    std::string v = c.value;
    if (!c.is_string && v.find_first_of("0123456789") != std::string::npos)
      std::replace(v.begin(), v.end(), 'D', 'E');   // (a FITS real may spell its exponent with D)
    hd.kv[c.key] = v;
  }
  for (const char *base : {"NGrid", "Xmin", "Xmax", "Ref_Vector"}) {
    if (hd.kv.count(base)) continue;
    std::string joined;
    for (int i = 0;; i++) {
      auto it = hd.kv.find(base + std::to_string(i));
      if (it == hd.kv.end()) break;
      joined += (i ? " " : "") + it->second;
    }
    if (!joined.empty()) hd.kv[base] = joined;
  }
  hd.kv["pion_data_offset"] = "0";
  if (!hd.kv.count("pion_slab_lo") && !hd.kv.count("pion_slab_n") && hd.kv.count("gridndim") && hd.kv.count("NGrid")) {
    // the whole slab axis
    const long ndim = strtol(hd.kv["gridndim"].c_str(), nullptr, 10);
    long np = 1;
    const char *p = hd.kv["NGrid"].c_str();
    for (long a = 0; a < std::min(ndim, 3L); a++) {
      char *e = nullptr;
      np = strtol(p, &e, 10);
      p = e;
    }
    hd.kv["pion_slab_lo"] = "0";
    hd.kv["pion_slab_n"] = std::to_string(ndim <= 1 ? 1 : np);
  }
  if (int rc = snapshot_header_from_kv(path, hd, 0, err)) return rc;
  if (!image_off) return 0;

  // every other HDU: one that carries the name of a primitive image -- the first of that name -- is checked and
  // remembered, every other one is skipped by the size its own header gives
  const pion_gpu_config &c = hd.cfg;
  // (the header has not been compared with a sim yet: the image list needs a variable count that has names)
  if (c.ntracer < 0 || c.ntracer > pion::OUT_MAX_TRACERS || c.nvar - c.ntracer < 5 || c.nvar - c.ntracer > 9) {
    err = std::string("FITS file ") + path + ": eqn_nvar / num_tracer describe no list of images (at most five tracers)";
    return PION_GPU_EINVAL;
  }
  const pion::OutputCfg o = pion::out_cfg(c);
  const long want[3] = {c.ng[0], (c.ndim == 3) ? (long)c.ng[1] : (long)hd.info.slab_n, hd.info.slab_n};
  std::vector<std::string> names((size_t)c.nvar);
  for (int v = 0; v < c.nvar; v++) {
    char name[pion::OUT_NAME_LEN];
    pion::out_image_name(o, v, name);
    names[(size_t)v] = name;
  }
  image_off->assign((size_t)c.nvar, -1);
  while (pos < size) {
    Hdu X;
    if (int rc = read_hdu(fd, size, pos, X, path, err)) return rc;
    const Card *n = X.find("EXTNAME");
    const size_t v = (n && n->is_string) ? (size_t)(std::find(names.begin(), names.end(), n->value) - names.begin()) : names.size();
    if (v == names.size() || (*image_off)[v] >= 0) continue;
    if (X.integer("BITPIX", 0) != -64) {
      err = std::string("FITS file ") + path + ": image " + names[v] + " has BITPIX = " + std::to_string(X.integer("BITPIX", 0))
            + "; only double-precision images (BITPIX = -64) are read";
      return PION_GPU_EINVAL;
    }
    bool same = X.integer("NAXIS", 0) == c.ndim && X.integer("PCOUNT", 0) == 0 && X.integer("GCOUNT", 1) == 1;
    for (int a = 0; a < c.ndim && same; a++) same = X.integer(("NAXIS" + std::to_string(a + 1)).c_str(), -1) == want[a];
    if (!same) {
      err = std::string("FITS file ") + path + ": image " + names[v]
            + " has other extents (NAXIS, NAXISn) than NGrid and pion_slab_n of the primary header give";
      return PION_GPU_EINVAL;
    }
    (*image_off)[v] = X.data_off;
  }
  for (int v = 0; v < c.nvar && note; v++)
    if ((*image_off)[(size_t)v] < 0)
      *note += std::string(note->empty() ? "" : " ") + "read_fits: " + path + " holds no image " + names[(size_t)v]
               + ": the variable is set to zero.";
  return 0;
}

long fits_convert_run(const pion_gpu_config &cfg, int var, double *run, size_t n)
{
  const pion::InputCfg in = pion::in_cfg(cfg);
  const pion::OutImage im = pion::out_image(in.o, var);
  long bad = 0;
  for (size_t i = 0; i < n; i++) {
    unsigned long long u;
    memcpy(&u, &run[i], sizeof u);
    const double x = pion::in_be64(u);
    bad += pion::in_rejected(x) ? 1 : 0;
    run[i] = pion::in_value(in, im, x);
  }
  return bad;
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

// ---- projected images (the rules: dev_project.h) -----------------------------------------------------------------
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
  io_error_.clear();
  if (!path || !*path) {
    io_error_ = "write_projection: no path";
    return PION_GPU_EINVAL;
  }
  // one rank of a slab run: the call is collective, and the last rank writes the one file
  const bool chain = projection_collective();
  std::vector<snapshot_param> params;
  long nloc = 0;
  int rc = projection_refused(axis, nfields, fields, "write_projection");
  if (!rc) rc = snapshot_params(params, nloc);
  if (!rc && (rc = finish_halo())) io_error_ = "write_projection: finish_halo failed";
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
  const long npix = (long)q.nj * q.ni, n = pion::proj_count(q, nfields);
  auto real = [](double x) {
    char b[64];
    snprintf(b, sizeof b, "%.17g", x);
    return std::string(b);
  };
  params.push_back({"pion_proj_axis", std::to_string(axis), 'i'});
  for (int i = 0; i < nfields; i++) {
    const std::string k = "pion_proj_" + std::to_string(i) + "_";
    params.push_back({k + "a", std::to_string(fields[i].a), 'i'});
    params.push_back({k + "var", std::to_string(fields[i].var), 'i'});
    params.push_back({k + "coef", real(fields[i].coef), 'd'});
    params.push_back({k + "b", real(fields[i].b), 'd'});
  }
  // 2. the file: big-endian, every extension's header of the same length
  std::vector<unsigned long long> R((size_t)n);
  for (long k = 0; k < n; k++) R[(size_t)k] = pion::out_be64(img[(size_t)k]);
  const std::string primary = fits_primary_header(params);
  const long naxis[2] = {q.ni, q.nj};
  std::vector<std::string> ext((size_t)nfields);
  for (int i = 0; i < nfields; i++) ext[(size_t)i] = fits_image_header(fields[i].name, 2, naxis);
  const long run_bytes = npix * (long)sizeof(double);
  const long stride = (long)ext[0].size() + padded(run_bytes);
  const long total = (long)primary.size() + nfields * stride;

  const std::string tmp = std::string(path) + ".part";
  int fd = open(tmp.c_str(), O_WRONLY | O_CREAT | O_TRUNC, 0644);
  if (fd < 0) {
    io_error_ = "write_projection: cannot create " + tmp + ": " + strerror(errno);
    return PION_GPU_EINVAL;
  }
  rc = (ftruncate(fd, (off_t)total) != 0) ? PION_GPU_EINVAL : 0;   // (the padding reads as zero bytes)
  if (!rc && full_pwrite(fd, primary.data(), primary.size(), 0)) rc = PION_GPU_EINVAL;
  for (int i = 0; i < nfields && !rc; i++) {
    const long at = (long)primary.size() + i * stride;
    if (full_pwrite(fd, ext[(size_t)i].data(), ext[(size_t)i].size(), (off_t)at)) rc = PION_GPU_EINVAL;
    if (!rc && full_pwrite(fd, R.data() + (size_t)i * npix, (size_t)run_bytes, (off_t)(at + (long)ext[(size_t)i].size())))
      rc = PION_GPU_EINVAL;
  }
  if (rc) io_error_ = "write_projection: writing " + tmp + " failed: " + strerror(errno);
  close(fd);
  if (!rc && rename(tmp.c_str(), path) != 0) {
    io_error_ = std::string("write_projection: cannot rename to ") + path + ": " + strerror(errno);
    rc = PION_GPU_EINVAL;
  }
  if (rc) unlink(tmp.c_str());
  return rc;
}

// ---- ray-traced column densities (the rules: dev_raytrace.h) -------------------------------------------------------
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
  io_error_.clear();
  if (!path || !*path) {
    io_error_ = "write_columns: no path";
    return PION_GPU_EINVAL;
  }
  if (int rc = columns_refused("write_columns")) return rc;
  if (rt_sources_.empty()) {
    io_error_ = "write_columns: raytrace: the sim has no radiation source (add_rt_source)";
    return PION_GPU_EINVAL;
  }
  std::vector<snapshot_param> params;
  long nloc = 0;
  if (int rc = snapshot_params(params, nloc)) return rc;
  if (int rc = finish_halo()) {
    io_error_ = "write_columns: finish_halo failed";
    return rc;
  }
  const pion::GridDesc g = grid_desc(cfg);
  const pion::OutGeom q = pion::out_geom(g);
  const int nsrc = (int)rt_sources_.size(), nimage = 2 * nsrc;
  const long plane = (long)q.rows * q.nx;
  const long naxis[3] = {q.nx, (cfg.ndim == 3) ? (long)q.rows : nloc, nloc};

  // the sources, under the reference's names (set_rt_src_params, dataio_base.cpp:1267-1282)
  auto real = [](double x) {
    char b[64];
    snprintf(b, sizeof b, "%.17g", x);
    return std::string(b);
  };
  params.push_back({"RT_Nsources", std::to_string(nsrc), 'i'});
  for (int n = 0; n < nsrc; n++) {
    const pion_gpu_rt_source &s = rt_moved_[(size_t)n];
    const std::string k = std::to_string(n);
    std::string pos;
    for (int a = 0; a < PION_MAX_DIM; a++) {
      double p = s.pos[a];
      if (s.at_infinity) p = (a == s.dir / 2) ? ((s.dir & 1) ? 1.0e200 : -1.0e200) : 0.0;
      pos += (a ? " " : "") + real(p);
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
  const long stride = (long)ext[0].size() + padded(run_bytes);
  const long off = (long)primary.size() + (long)ext[0].size();
  const long total = (long)primary.size() + nimage * stride;

  const std::string tmp = std::string(path) + ".part";
  int fd = open(tmp.c_str(), O_WRONLY | O_CREAT | O_TRUNC, 0644);
  if (fd < 0) {
    io_error_ = "write_columns: cannot create " + tmp + ": " + strerror(errno);
    return PION_GPU_EINVAL;
  }
  int rc = (ftruncate(fd, (off_t)total) != 0) ? PION_GPU_EINVAL : 0;   // (the padding reads as zero bytes)
  if (!rc && full_pwrite(fd, primary.data(), primary.size(), 0)) rc = PION_GPU_EINVAL;
  for (int i = 0; i < nimage && !rc; i++)
    if (full_pwrite(fd, ext[(size_t)i].data(), ext[(size_t)i].size(), (off_t)((long)primary.size() + i * stride))) rc = PION_GPU_EINVAL;

  if (!rc && rt_on_backend_ && be_->raytrace && be_->rt_count && be_->columns_to_host_begin && be_->ongrid_to_host_end) {
    // traced on the device; then image after image, a chunk of planes at a time: the pack and the copy of the next
    // chunk are enqueued while this one is written
    long cp = (64L << 20) / (long)sizeof(double) / std::max(1L, be_->rt_count(h_, 1));
    if (const char *e = getenv("PION_SNAPSHOT_CHUNK_PLANES"))
      if (atol(e) > 0) cp = atol(e);
    cp = std::max(1L, std::min(cp, nloc));
    const long nchunk = (nloc + cp - 1) / cp, njob = nimage * nchunk;
    auto begin = [&](long job) {
      const long i = job / nchunk, a = (job % nchunk) * cp;
      return be_->columns_to_host_begin(h_, (int)(i / 2), (int)(i & 1), (int)a, (int)std::min(nloc, a + cp), (int)(job & 1));
    };
    rc = be_->raytrace(h_, 0);
    if (!rc) rc = begin(0);
    for (long job = 0; job < njob && !rc; job++) {
      if (job + 1 < njob) rc = begin(job + 1);
      const double *src = nullptr;
      if (!rc) rc = be_->ongrid_to_host_end(h_, (int)(job & 1), &src);
      if (rc) break;
      const long i = job / nchunk, a = (job % nchunk) * cp, b = std::min(nloc, a + cp);
      if (full_pwrite(fd, src, (size_t)((b - a) * plane) * sizeof(double), (off_t)(off + i * stride + a * plane * (long)sizeof(double))))
        rc = PION_GPU_EINVAL;
    }
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
        if (full_pwrite(fd, R.data(), (size_t)run_bytes, (off_t)(off + (2 * n + w) * stride))) rc = PION_GPU_EINVAL;
      }
    }
  }
  if (rc && io_error_.empty()) io_error_ = "write_columns: writing " + tmp + " failed: " + strerror(errno);
  close(fd);
  if (!rc && rename(tmp.c_str(), path) != 0) {
    io_error_ = std::string("write_columns: cannot rename to ") + path + ": " + strerror(errno);
    rc = PION_GPU_EINVAL;
  }
  if (rc) unlink(tmp.c_str());
  return rc;
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
}

}  // namespace pion_host
