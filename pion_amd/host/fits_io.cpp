// fits_io.cpp -- see fits_io.h
#include "fits_io.h"

#include <fcntl.h>
#include <unistd.h>

#include <algorithm>
#include <cerrno>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <stdexcept>

#include "dev_rules.h"
#include "sim_control_gpu.h"

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

}  // namespace

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

fits_layout::fits_layout(const std::string &primary_, const std::vector<std::string> &ext_, long run_bytes)
    : primary(primary_), ext(ext_), data_padded(padded(run_bytes)),
      stride((ext_.empty() ? 0 : (long)ext_[0].size()) + data_padded), total((long)primary_.size() + (long)ext_.size() * stride)
{
  for (const std::string &h : ext)
    if (h.size() != ext[0].size()) throw std::logic_error("fits_layout: the extension headers differ in length");
}

int fits_layout::start(PartFile &f) const
{
  int rc = f.resize(total);
  if (!rc) rc = f.write(primary.data(), primary.size(), 0);
  for (size_t i = 0; i < ext.size() && !rc; i++) rc = f.write(ext[i].data(), ext[i].size(), header_at((long)i));
  return rc;
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
  if (int rc = path_refused("write_fits", path)) return rc;
  if (cfg.ntracer > pion::OUT_MAX_TRACERS) {
    io_error_ = "write_fits: only accepts <= 5 tracers (this sim has " + std::to_string(cfg.ntracer) + ")";
    return PION_GPU_EINVAL;
  }
  std::vector<snapshot_param> params;
  long nloc = 0;
  if (int rc = writer_params("write_fits", params, nloc)) return rc;
  const pion::GridDesc g = grid_desc(cfg);
  const pion::OutputCfg o = pion::out_cfg(cfg);
  const pion::OutGeom q = pion::out_geom(g);
  const int nimage = pion::out_nimage(o);
  const long plane = (long)q.rows * q.nx;
  const long naxis[3] = {q.nx, (cfg.ndim == 3) ? (long)q.rows : nloc, nloc};

  const std::string primary = fits_primary_header(params);
  std::vector<std::string> ext((size_t)nimage);
  for (int i = 0; i < nimage; i++) {
    char name[pion::OUT_NAME_LEN];
    pion::out_image_name(o, i, name);
    ext[i] = fits_image_header(name, cfg.ndim, naxis);
  }
  const long run_bytes = nloc * plane * (long)sizeof(double);
  const fits_layout L(primary, ext, run_bytes);

  PartFile f("write_fits", path, io_error_);
  if (!f.ok()) return PION_GPU_EINVAL;
  int rc = L.start(f);
  if (!rc && be_->fits_to_host_begin && be_->fits_count && be_->ongrid_to_host_end)
    rc = stream_runs(f, true, nimage, nloc, plane, L.data_at(0), L.stride, "write_fits");
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
      rc = f.write(R.data(), (size_t)run_bytes, L.data_at(i));
    }
  }
  return f.commit(rc);
}

}  // namespace pion_host
