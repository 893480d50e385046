// snapshot_io.cpp -- see snapshot_io.h
#include "snapshot_io.h"

#include <fcntl.h>
#include <sys/stat.h>
#include <unistd.h>

#include <algorithm>
#include <cerrno>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <sstream>

#include "fits_io.h"
#include "out_file.h"
#include "sim_control_gpu.h"
#include "slab_comm.h"

namespace pion_host {

namespace {

const char MAGIC[9] = "PIONRAW2";
const long HEADER_MAX = 1 << 16;        // a header is a few KiB
const long CHUNK_BYTES = 64L << 20;     // per staging buffer

// constants.h:150-152
const double SMALLVALUE = 1.0e-12, TINYVALUE = 1.0e-100;

// boundary types <-> the reference's strings (SimPM.BC_XN ..., setup_fixed_grid.cpp:912-944); "NONE" on unused axes
// (get_sim_info.cpp:386-395)
struct BcName { int type; const char *name; };
const BcName BC_TABLE[] = {{0, "NONE"}, {PION_BC_PERIODIC, "periodic"}, {PION_BC_OUTFLOW, "outflow"},
                           {PION_BC_INFLOW, "inflow"}, {PION_BC_REFLECTING, "reflecting"}, {PION_BC_FIXED, "fixed"},
                           {PION_BC_ONEWAY_OUT, "one-way-outflow"}, {PION_BC_DMACH, "DMR"},
                           {PION_BC_AXISYMMETRIC, "axisymmetric"}, {PION_BC_JETREFLECT, "jetreflect"}};
const char *bc_name(int t)
{
  for (const BcName &b : BC_TABLE)
    if (b.type == t) return b.name;
  return nullptr;
}
int bc_type(const std::string &s)
{
  for (const BcName &b : BC_TABLE)
    if (s == b.name) return b.type;
  return -1;
}
const char *const BC_KEYS[6] = {"BC_XN", "BC_XP", "BC_YN", "BC_YP", "BC_ZN", "BC_ZP"};

// geometry of the on-grid data of one sim / one file
struct Shape {
  int sa;            // slab axis (-1: 1-D, the one row is the one plane)
  long nx, rows;     // cells per row, rows per plane
  long plane() const { return nx * rows; }
};
Shape shape_of(const pion_gpu_config &c)
{
  Shape s;
  s.sa = (c.ndim == 1) ? -1 : c.ndim - 1;
  s.nx = c.ng[0];
  s.rows = (c.ndim == 3) ? c.ng[1] : 1;
  return s;
}

int full_pread(int fd, void *p, size_t n, off_t off)
{
  char *c = (char *)p;
  while (n > 0) {
    const ssize_t r = pread(fd, c, n, off);
    if (r < 0 && errno == EINTR) continue;
    if (r <= 0) return -1;
    c += r, off += r, n -= (size_t)r;
  }
  return 0;
}

struct Fd {
  int fd = -1;
  ~Fd()
  {
    if (fd >= 0) close(fd);
  }
};

bool get(const snapshot_header &hd, const char *key, std::string &v, std::string &err)
{
  auto it = hd.kv.find(key);
  if (it == hd.kv.end()) {
    err = std::string("snapshot header: key '") + key + "' is missing";
    return false;
  }
  v = it->second;
  return true;
}
bool get_doubles(const snapshot_header &hd, const char *key, double *out, int n, std::string &err)
{
  std::string v;
  if (!get(hd, key, v, err)) return false;
  const char *p = v.c_str();
  for (int i = 0; i < n; i++) {
    char *e = nullptr;
    out[i] = strtod(p, &e);
    if (e == p) {
      err = std::string("snapshot header: key '") + key + "' holds too few numbers";
      return false;
    }
    p = e;
  }
  return true;
}
bool get_longs(const snapshot_header &hd, const char *key, long *out, int n, std::string &err)
{
  std::string v;
  if (!get(hd, key, v, err)) return false;
  const char *p = v.c_str();
  for (int i = 0; i < n; i++) {
    char *e = nullptr;
    out[i] = strtol(p, &e, 10);
    if (e == p) {
      err = std::string("snapshot header: key '") + key + "' holds too few numbers";
      return false;
    }
    p = e;
  }
  return true;
}
bool get_int(const snapshot_header &hd, const char *key, int &out, std::string &err)
{
  long v;
  if (!get_longs(hd, key, &v, 1, err)) return false;
  out = (int)v;
  return true;
}

}  // namespace

long chunk_planes(long doubles_per_plane_all_runs, long planes)
{
  long c = CHUNK_BYTES / (long)sizeof(double) / std::max(1L, doubles_per_plane_all_runs);
  if (const char *e = getenv("PION_SNAPSHOT_CHUNK_PLANES")) {
    const long f = atol(e);
    if (f > 0) c = f;
  }
  return std::max(1L, std::min(c, planes));
}

bool equalD(const double a, const double b)
{
  if (a == b) return true;
  if (fabs(a) + fabs(b) < TINYVALUE) return true;
  return (fabs(a - b) / (fabs(a) + fabs(b) + TINYVALUE)) < SMALLVALUE;
}

const std::vector<std::string> &snapshot_header_keys()
{
  static const std::vector<std::string> k = {
      "gridndim", "NGrid", "Ncell", "Xmin", "Xmax", "eqn_type", "eqn_nvar", "num_tracer", "solver", "coord_sys",
      "Space_OOA", "Time_OOA", "Gamma", "CFL", "art_visc", "eta_visc", "Ref_Vector", "EP_cooling",
      "EP_MP_timestep_limit", "EP_Min_Temperature", "EP_Max_Temperature", "t_start", "t_finish", "t_step", "t_sim",
      "min_timestep", "last_dt", "op_freq", "opfreq_time", "op_criterion", "outfile", "BC_XN", "BC_XP", "BC_YN",
      "BC_YP", "BC_ZN", "BC_ZP", "BC_Ninternal", "JetSim", "WIND_Nsources", "pion_nbc", "pion_strict_fp",
      "pion_bc_dmach2", "pion_dx", "pion_next_optime", "pion_rank", "pion_world", "pion_slab_lo", "pion_slab_n",
      "pion_data_offset"};
  return k;
}

int snapshot_read_header(const char *path, snapshot_header &hd, std::string &err)
{
  hd = snapshot_header();
  if (!path) {
    err = "snapshot: no path";
    return PION_GPU_EINVAL;
  }
  Fd f;
  f.fd = open(path, O_RDONLY);
  if (f.fd < 0) {
    err = std::string("snapshot: cannot open ") + path + ": " + strerror(errno);
    return PION_GPU_EINVAL;
  }
  std::string buf((size_t)HEADER_MAX, '\0');
  ssize_t n = pread(f.fd, &buf[0], (size_t)HEADER_MAX, 0);
  if (n < 8 || memcmp(buf.data(), MAGIC, 8) != 0) {
    err = std::string("snapshot: ") + path + " is not a PIONRAW2 file (wrong magic)";
    return PION_GPU_EINVAL;
  }
  buf.resize((size_t)n);
  // "name value" lines up to and including pion_data_offset
  size_t pos = 8;
  bool complete = false;
  while (pos < buf.size() && !complete) {
    size_t eol = buf.find('\n', pos);
    if (eol == std::string::npos) break;
    const std::string line = buf.substr(pos, eol - pos);
    pos = eol + 1;
    if (line.empty()) continue;
    const size_t sp = line.find(' ');
    const std::string key = line.substr(0, sp);
    const std::string val = (sp == std::string::npos) ? "" : line.substr(sp + 1);
    hd.kv[key] = val;
    complete = (key == "pion_data_offset");
  }
  if (!complete) {
    err = std::string("snapshot header of ") + path + ": key 'pion_data_offset' is missing (header incomplete)";
    return PION_GPU_EINVAL;
  }
  return snapshot_header_from_kv(path, hd, (long)pos, err);
}

int snapshot_header_from_kv(const char *path, snapshot_header &hd, long header_end, std::string &err)
{
  for (const std::string &k : snapshot_header_keys())
    if (!hd.kv.count(k)) {
      err = std::string("snapshot header of ") + path + ": key '" + k + "' is missing";
      return PION_GPU_EINVAL;
    }
  pion_gpu_config &c = hd.cfg;
  pion_host_snapshot_info &I = hd.info;
  memset(&c, 0, sizeof c);
  memset(&I, 0, sizeof I);
  long ng[3], l;
  double xmax[3];
  bool ok = get_int(hd, "gridndim", c.ndim, err) && get_longs(hd, "NGrid", ng, 3, err)
            && get_doubles(hd, "Xmin", c.xmin, 3, err) && get_doubles(hd, "Xmax", xmax, 3, err)
            && get_int(hd, "eqn_type", c.eqntype, err) && get_int(hd, "eqn_nvar", c.nvar, err)
            && get_int(hd, "num_tracer", c.ntracer, err) && get_int(hd, "solver", c.solver, err)
            && get_int(hd, "coord_sys", c.coord_sys, err) && get_int(hd, "Space_OOA", c.sp_ooa, err)
            && get_int(hd, "Time_OOA", c.tm_ooa, err) && get_doubles(hd, "Gamma", &c.gamma, 1, err)
            && get_doubles(hd, "CFL", &c.cfl, 1, err) && get_int(hd, "art_visc", c.artvisc, err)
            && get_doubles(hd, "eta_visc", &c.etav, 1, err) && get_int(hd, "EP_cooling", c.cooling, err)
            && get_int(hd, "EP_MP_timestep_limit", c.mp_timestep_limit, err)
            && get_doubles(hd, "EP_Min_Temperature", &c.min_temp, 1, err)
            && get_doubles(hd, "EP_Max_Temperature", &c.max_temp, 1, err) && get_int(hd, "pion_nbc", c.nbc, err)
            && get_int(hd, "pion_strict_fp", c.strict_fp, err) && get_int(hd, "pion_bc_dmach2", c.bc_dmach2, err)
            && get_doubles(hd, "pion_dx", &c.dx, 1, err);
  if (ok && (c.ndim < 1 || c.ndim > 3 || c.nvar < 1 || c.nvar > PION_MAX_NVAR)) {
    err = std::string("snapshot header of ") + path + ": gridndim / eqn_nvar out of range";
    return PION_GPU_EINVAL;
  }
  ok = ok && get_doubles(hd, "Ref_Vector", c.refvec, c.nvar, err);
  for (int i = 0; ok && i < 3; i++) c.ng[i] = (int)ng[i];
  for (int fc = 0; ok && fc < 6; fc++) {
    std::string v;
    ok = get(hd, BC_KEYS[fc], v, err);
    if (ok && (c.bc_type[fc] = bc_type(v)) < 0) {
      err = std::string("snapshot header: unknown boundary '") + v + "' for " + BC_KEYS[fc];
      ok = false;
    }
  }
  ok = ok && get_doubles(hd, "t_start", &I.t_start, 1, err) && get_doubles(hd, "t_finish", &I.t_finish, 1, err)
       && get_int(hd, "t_step", I.t_step, err) && get_doubles(hd, "t_sim", &I.t_sim, 1, err)
       && get_doubles(hd, "min_timestep", &I.min_timestep, 1, err) && get_doubles(hd, "last_dt", &I.last_dt, 1, err)
       && get_int(hd, "op_freq", I.op_freq, err) && get_doubles(hd, "opfreq_time", &I.opfreq_time, 1, err)
       && get_int(hd, "op_criterion", I.op_criterion, err)
       && get_doubles(hd, "pion_next_optime", &I.next_optime, 1, err) && get_int(hd, "pion_rank", I.rank, err)
       && get_int(hd, "pion_world", I.world, err) && get_int(hd, "pion_slab_lo", I.slab_lo, err)
       && get_int(hd, "pion_slab_n", I.slab_n, err) && get_longs(hd, "pion_data_offset", &l, 1, err);
  if (!ok) {
    err += std::string(" (") + path + ")";
    return PION_GPU_EINVAL;
  }
  I.data_offset = l;
  snprintf(I.outfile, sizeof I.outfile, "%s", hd.kv["outfile"].c_str());
  const int np = (c.ndim == 1) ? 1 : c.ng[c.ndim - 1];
  bool sane = I.slab_lo >= 0 && I.slab_n >= 1 && I.slab_lo + I.slab_n <= np && I.data_offset >= header_end;
  for (int a = 0; a < 3; a++) sane = sane && c.ng[a] >= 1;
  if (!sane) {
    err = std::string("snapshot header of ") + path + ": plane range, NGrid or data offset out of range";
    return PION_GPU_EINVAL;
  }
  return 0;
}

// ---- the sim's view of the global problem ------------------------------------------------------
namespace {
struct Global {
  int ng[3], bc[6];
  double xmin[3], xmax[3];
  int slab_lo, slab_n;   // this sim's planes
};
int global_view(const sim_control_gpu &sim, Global &G, std::string &err)
{
  const pion_gpu_config &c = sim.cfg;
  const Shape s = shape_of(c);
  for (int a = 0; a < 3; a++) G.ng[a] = c.ng[a], G.xmin[a] = c.xmin[a];
  for (int f = 0; f < 6; f++) G.bc[f] = c.bc_type[f];
  G.slab_lo = 0;
  G.slab_n = (s.sa < 0) ? 1 : c.ng[s.sa];
  if (sim.slab.set && s.sa >= 0) {
    G.ng[s.sa] = sim.slab.global_planes;
    G.xmin[s.sa] = c.xmin[s.sa] - sim.slab.plane_lo * c.dx;
    G.bc[2 * s.sa] = sim.slab.bc_lo;
    G.bc[2 * s.sa + 1] = sim.slab.bc_hi;
    G.slab_lo = sim.slab.plane_lo;
  }
  for (int f = 0; f < 6; f++)
    if (G.bc[f] == PION_BC_SLAB || !bc_name(G.bc[f])) {
      err = "snapshot: this sim is a slab of a larger problem (or has a boundary type without a name): say where it "
            "sits with set_slab_extent first";
      return PION_GPU_EINVAL;
    }
  for (int a = 0; a < 3; a++) G.xmax[a] = (a < c.ndim) ? G.xmin[a] + G.ng[a] * c.dx : G.xmin[a];
  return 0;
}
}  // namespace

// how every writer opens: the text of the last failure cleared, a null or empty path refused
int sim_control_gpu::path_refused(const char *who, const char *path)
{
  io_error_.clear();
  if (path && *path) return 0;
  io_error_ = std::string(who) + ": no path";
  return PION_GPU_EINVAL;
}

// every parameter a file of this sim carries, in snapshot_header_keys() order (pion_data_offset, the PIONRAW2 file's
// own, excepted): the one list every writer uses
int sim_control_gpu::snapshot_params(std::vector<snapshot_param> &out, long &slab_n)
{
  Global G;
  if (int rc = global_view(*this, G, io_error_)) return rc;
  slab_n = G.slab_n;
  out.clear();
  auto I = [&](const char *k, long v) { out.push_back({k, std::to_string(v), 'i'}); };
  auto D = [&](const char *k, double v) { out.push_back({k, fmt_d(v), 'd'}); };
  auto S = [&](const char *k, const std::string &v) { out.push_back({k, v, 's'}); };
  I("gridndim", cfg.ndim);
  out.push_back({"NGrid", std::to_string(G.ng[0]) + " " + std::to_string(G.ng[1]) + " " + std::to_string(G.ng[2]), 'i'});
  I("Ncell", (long)G.ng[0] * G.ng[1] * G.ng[2]);
  out.push_back({"Xmin", fmt_d(G.xmin[0]) + " " + fmt_d(G.xmin[1]) + " " + fmt_d(G.xmin[2]), 'd'});
  out.push_back({"Xmax", fmt_d(G.xmax[0]) + " " + fmt_d(G.xmax[1]) + " " + fmt_d(G.xmax[2]), 'd'});
  I("eqn_type", cfg.eqntype), I("eqn_nvar", cfg.nvar), I("num_tracer", cfg.ntracer);
  I("solver", cfg.solver), I("coord_sys", cfg.coord_sys);
  I("Space_OOA", cfg.sp_ooa), I("Time_OOA", cfg.tm_ooa);
  D("Gamma", cfg.gamma), D("CFL", cfg.cfl);
  I("art_visc", cfg.artvisc), D("eta_visc", cfg.etav);
  std::string rv;
  for (int v = 0; v < cfg.nvar; v++) rv += (v ? " " : "") + fmt_d(cfg.refvec[v]);
  out.push_back({"Ref_Vector", rv, 'd'});
  I("EP_cooling", cfg.cooling), I("EP_MP_timestep_limit", cfg.mp_timestep_limit);
  D("EP_Min_Temperature", cfg.min_temp), D("EP_Max_Temperature", cfg.max_temp);
  D("t_start", T.starttime), D("t_finish", T.finishtime);
  I("t_step", T.timestep), D("t_sim", T.simtime);
  D("min_timestep", T.min_timestep), D("last_dt", T.last_dt);
  I("op_freq", T.opfreq), D("opfreq_time", T.opfreq_time);
  I("op_criterion", T.op_criterion);
  S("outfile", T.outfile.empty() ? "NONE" : T.outfile);
  for (int f = 0; f < 6; f++) S(BC_KEYS[f], bc_name(G.bc[f]));
  // internal boundaries and sources are set up by the caller before a restart: the header only counts them
  I("BC_Ninternal", (cfg.bc_dmach2 ? 1 : 0) + (n_wind_sources_ > 0 ? 1 : 0));
  I("JetSim", 0);
  I("WIND_Nsources", n_wind_sources_);
  I("pion_nbc", cfg.nbc), I("pion_strict_fp", cfg.strict_fp), I("pion_bc_dmach2", cfg.bc_dmach2);
  D("pion_dx", cfg.dx);
  D("pion_next_optime", T.next_optime);
  I("pion_rank", comm_ ? comm_->rank() : 0), I("pion_world", comm_ ? comm_->world() : 1);
  I("pion_slab_lo", G.slab_lo), I("pion_slab_n", G.slab_n);
  return 0;
}

// what every writer does before it reads the state: the parameters, and a halo exchange in flight completed
int sim_control_gpu::writer_params(const char *who, std::vector<snapshot_param> &out, long &slab_n)
{
  if (int rc = snapshot_params(out, slab_n)) return rc;
  const int rc = finish_halo();
  if (rc) io_error_ = std::string(who) + ": finish_halo failed";
  return rc;
}

// The streamed loop of every writer whose data leave the backend through its two staging slots: job after job, begin(job,
// slot) enqueues the pack and the copy of one, ongrid_to_host_end waits for it, put(job, src) writes it.  Job + 1 is
// begun BEFORE job is ended: its pack and copy run while this code writes -- the overlap the slots exist for
int sim_control_gpu::stream_jobs(long njob, const std::function<int(long, int)> &begin,
                                 const std::function<int(long, const double *)> &put)
{
  int rc = begin(0, 0);
  for (long job = 0; job < njob && !rc; job++) {
    if (job + 1 < njob) rc = begin(job + 1, (int)((job + 1) & 1));
    const double *src = nullptr;
    if (!rc) rc = be_->ongrid_to_host_end(h_, (int)(job & 1), &src);
    if (!rc) rc = put(job, src);
  }
  return rc;
}

// The planes [0, nloc) of a snapshot, chunk-major: a job is a chunk of whole planes and holds all the runs, one per
// variable (PIONRAW2) or image (FITS), run r of a chunk at off + r * stride + (its first plane's byte offset inside a
// run).  A chunk is the largest number of planes whose runs fit one staging slot.
int sim_control_gpu::stream_runs(PartFile &f, bool fits, int nrun, long nloc, long plane, long off, long stride, const char *who)
{
  const long cp = chunk_planes((fits ? be_->fits_count : be_->ongrid_count)(h_, 1), nloc);
  auto begin = [&](long i, int slot) {
    const long a = i * cp, b = std::min(nloc, a + cp);
    return fits ? be_->fits_to_host_begin(h_, (int)a, (int)b, slot) : be_->ongrid_to_host_begin(h_, 0, (int)a, (int)b, slot);
  };
  auto put = [&](long i, const double *src) {
    const long a = i * cp;
    const size_t n = (size_t)(std::min(nloc, a + cp) - a) * plane;
    int rc = 0;
    for (int v = 0; v < nrun && !rc; v++)
      rc = f.write(src + (size_t)v * n, n * sizeof(double), off + (long)v * stride + a * plane * (long)sizeof(double));
    return rc;
  };
  const int rc = stream_jobs((nloc + cp - 1) / cp, begin, put);
  if (rc && io_error_.empty()) io_error_ = std::string(who) + ": staging the planes failed: " + last_error();
  return rc;
}

int sim_control_gpu::write_snapshot(const char *path)
{
  if (int rc = path_refused("write_snapshot", path)) return rc;
  std::vector<snapshot_param> params;
  long nloc = 0;
  if (int rc = writer_params("write_snapshot", params, nloc)) return rc;
  const Shape s = shape_of(cfg);
  const long plane = s.plane();

  std::string head = std::string(MAGIC, 8);
  for (const snapshot_param &p : params) head += p.key + " " + p.value + "\n";
  // the data start at a multiple of 4096 bytes
  long off = ((long)head.size() + 64 + 4095) / 4096 * 4096;
  head += "pion_data_offset " + std::to_string(off) + "\n";
  head.resize((size_t)off, '\n');

  PartFile f("write_snapshot", path, io_error_);
  if (!f.ok()) return PION_GPU_EINVAL;
  int rc = f.write(head.data(), head.size(), 0);
  const size_t run = (size_t)nloc * plane;   // doubles of one variable in the file
  if (!rc && be_->ongrid_to_host_begin && be_->ongrid_to_host_end && be_->ongrid_count)
    rc = stream_runs(f, false, cfg.nvar, nloc, plane, off, (long)(run * sizeof(double)), "write_snapshot");
  else if (!rc) {
    // no streaming entries: the whole array with its ghosts, stripped here
    const long nb = cfg.nbc, nxa = cfg.ng[0] + 2 * nb, nya = (cfg.ndim >= 2) ? cfg.ng[1] + 2 * nb : 1,
               nza = (cfg.ndim == 3) ? cfg.ng[2] + 2 * nb : 1;
    const size_t ncell = (size_t)nxa * nya * nza;
    std::vector<double> A((size_t)cfg.nvar * ncell), R(run);
    rc = be_->download(h_, 0, A.data());
    if (rc) io_error_ = "write_snapshot: download failed: " + last_error();
    for (int v = 0; v < cfg.nvar && !rc; v++) {
      size_t o = 0;
      for (long k = 0; k < (cfg.ndim == 3 ? cfg.ng[2] : 1); k++)
        for (long j = 0; j < (cfg.ndim >= 2 ? cfg.ng[1] : 1); j++) {
          const size_t c0 = (size_t)v * ncell + nb + (size_t)nxa * ((cfg.ndim >= 2 ? j + nb : 0) + (size_t)nya * (cfg.ndim == 3 ? k + nb : 0));
          memcpy(&R[o], &A[c0], (size_t)cfg.ng[0] * sizeof(double));
          o += cfg.ng[0];
        }
      rc = f.write(R.data(), run * sizeof(double), off + (long)((size_t)v * run * sizeof(double)));
    }
  }
  return f.commit(rc);
}

namespace {
struct FillCtx {
  int fd;
  int nvar;
  size_t n;           // doubles of the chunk per variable
  // byte offset in the file of the chunk's first double of each variable; < 0: the file has no image of that variable
  // (a FITS file may lack one) and its run is zero bytes
  off_t var_off[PION_MAX_NVAR];
};
int fill_chunk(void *p, double *dst)
{
  const FillCtx *c = (const FillCtx *)p;
  for (int v = 0; v < c->nvar; v++) {
    if (c->var_off[v] < 0) memset(dst + (size_t)v * c->n, 0, c->n * sizeof(double));
    else if (full_pread(c->fd, dst + (size_t)v * c->n, c->n * sizeof(double), c->var_off[v])) return PION_GPU_EINVAL;
  }
  return 0;
}
}  // namespace

int sim_control_gpu::read_snapshot(const char *const *paths, int npaths) { return read_files(paths, npaths, false); }
int sim_control_gpu::read_fits(const char *const *paths, int npaths) { return read_files(paths, npaths, true); }

// The restart from either file type: PIONRAW2 (fits false) or FITS (fits_io.h).  What differs is how a header is read,
// where a variable's run lies in a file, and what an element is: the native double itself, or the big-endian file
// element of dev_output.h's read rules -- converted by the backend's fits_from_host (k_unpack_fits), or, without that
// entry, by fits_convert_run in a host loop.
int sim_control_gpu::read_files(const char *const *paths, int npaths, bool fits)
{
  const std::string who = fits ? "read_fits" : "read_snapshot";
  io_error_.clear();
  if (!paths || npaths < 1) {
    io_error_ = who + ": no files";
    return PION_GPU_EINVAL;
  }
  if (fits && cfg.ntracer > 5) {   // (dataio_fits.cpp:157, as write_fits)
    io_error_ = who + ": only accepts <= 5 tracers (this sim has " + std::to_string(cfg.ntracer) + ")";
    return PION_GPU_EINVAL;
  }
  Global G;
  if (int rc = global_view(*this, G, io_error_)) return rc;
  const Shape s = shape_of(cfg);
  const long nloc = G.slab_n, plane = s.plane();

  // every header: the same problem as this sim's, and the same moment as the first file's
  std::vector<snapshot_header> H((size_t)npaths);
  std::vector<std::vector<long>> image_off((size_t)npaths);   // FITS: where each variable's data unit starts (-1: absent)
  std::string note;                                           // FITS: the images a file lacks
  for (int i = 0; i < npaths; i++) {
    if (int rc = fits ? fits_read_header(paths[i], H[i], &image_off[i], &note, io_error_)
                      : snapshot_read_header(paths[i], H[i], io_error_))
      return rc;
    const pion_gpu_config &c = H[i].cfg;
    const char *bad = nullptr;
    if (c.ndim != cfg.ndim || c.coord_sys != cfg.coord_sys) bad = "gridndim / coord_sys";
    else if (c.eqntype != cfg.eqntype || c.nvar != cfg.nvar || c.ntracer != cfg.ntracer) bad = "eqn_type / eqn_nvar / num_tracer";
    else if (c.solver != cfg.solver) bad = "solver";
    else if (c.sp_ooa != cfg.sp_ooa || c.tm_ooa != cfg.tm_ooa) bad = "Space_OOA / Time_OOA";
    else if (c.gamma != cfg.gamma) bad = "Gamma";
    else if (c.dx != cfg.dx) bad = "pion_dx";
    else if (c.ng[0] != G.ng[0] || c.ng[1] != G.ng[1] || c.ng[2] != G.ng[2]) bad = "NGrid";
    // (a slab's own xmin is the global one plus plane_lo * dx, rounded: compare to a small fraction of a cell)
    for (int a = 0; a < cfg.ndim && !bad; a++)
      if (fabs(c.xmin[a] - G.xmin[a]) > 1.0e-9 * cfg.dx) bad = "Xmin";
    if (bad) {
      io_error_ = who + ": " + paths[i] + " does not match this sim's configuration: " + bad;
      return PION_GPU_EINVAL;
    }
    const pion_host_snapshot_info &a = H[0].info, &b = H[i].info;
    if (a.t_sim != b.t_sim || a.t_step != b.t_step || a.last_dt != b.last_dt || a.next_optime != b.next_optime
        || a.t_start != b.t_start) {
      io_error_ = who + ": " + paths[i] + " and " + paths[0] + " are of different moments of a run (t_sim, t_step, last_dt, pion_next_optime or t_start differ)";
      return PION_GPU_EINVAL;
    }
    if (fits) continue;   // (fits_read_header has sized every data unit against the file)
    struct stat st;
    const long need = b.data_offset + (long)cfg.nvar * b.slab_n * plane * (long)sizeof(double);
    if (stat(paths[i], &st) != 0 || (long)st.st_size < need) {
      io_error_ = who + ": " + paths[i] + " is truncated: its header promises " + std::to_string(need) + " bytes";
      return PION_GPU_EINVAL;
    }
  }
  // which file gives which of this sim's planes (the first that holds a plane)
  std::vector<int> owner((size_t)nloc, -1);
  for (int i = 0; i < npaths; i++)
    for (long p = 0; p < nloc; p++) {
      const long gp = G.slab_lo + p;
      if (owner[p] < 0 && gp >= H[i].info.slab_lo && gp < H[i].info.slab_lo + H[i].info.slab_n) owner[p] = i;
    }
  for (long p = 0; p < nloc; p++)
    if (owner[p] < 0) {
      io_error_ = who + ": plane " + std::to_string(G.slab_lo + p) + " of the slab axis is in none of the files given";
      return PION_GPU_EINVAL;
    }

  // as Init: the previous state's time-step request and halo exchange are void
  dt_requested_ = false;
  if (comm_) comm_->reset();

  // (the two FITS entries of the table are read here and nowhere else: pion_backend.h)
  const bool stream = fits ? (be_->ongrid_count && be_->fits_from_host && be_->fits_read_status)
                           : (be_->ongrid_from_host && be_->ongrid_count);
  long nbad = 0;   // FITS: rejected elements
  std::vector<double> A;   // the whole array with zero ghosts, when the backend cannot stream
  const long nb = cfg.nbc, nxa = cfg.ng[0] + 2 * nb, nya = (cfg.ndim >= 2) ? cfg.ng[1] + 2 * nb : 1,
             nza = (cfg.ndim == 3) ? cfg.ng[2] + 2 * nb : 1;
  const size_t ncell = (size_t)nxa * nya * nza;
  if (!stream) A.assign((size_t)cfg.nvar * ncell, 0.0);
  int rc = 0, slot = 0;
  for (long p0 = 0; p0 < nloc && !rc;) {
    const int i = owner[p0];
    long p1 = p0;
    while (p1 < nloc && owner[p1] == i) p1++;
    Fd f;
    f.fd = open(paths[i], O_RDONLY);
    if (f.fd < 0) {
      io_error_ = who + ": cannot open " + paths[i];
      rc = PION_GPU_EINVAL;
      break;
    }
    const pion_host_snapshot_info &I = H[i].info;
    FillCtx c;
    c.fd = f.fd, c.nvar = cfg.nvar;
    const size_t frun = (size_t)I.slab_n * plane;   // doubles of one variable in the file
    // (a chunk of the primitive images of a FITS file has the size of a chunk of variables)
    const long cp = stream ? chunk_planes(be_->ongrid_count(h_, 1), p1 - p0) : p1 - p0;
    for (long a = p0; a < p1 && !rc; a += cp) {
      const long b = std::min(p1, a + cp);
      const size_t first = (size_t)(G.slab_lo + a - I.slab_lo) * plane;   // first double of the chunk inside a run
      c.n = (size_t)(b - a) * plane;
      for (int v = 0; v < cfg.nvar; v++) {
        if (!fits) c.var_off[v] = I.data_offset + (off_t)(((size_t)v * frun + first) * sizeof(double));
        else c.var_off[v] = (image_off[i][v] < 0) ? -1 : (off_t)(image_off[i][v] + (long)(first * sizeof(double)));
      }
      if (stream) {
        rc = fits ? be_->fits_from_host(h_, (int)a, (int)b, slot, fill_chunk, &c)
                  : be_->ongrid_from_host(h_, (int)a, (int)b, slot, fill_chunk, &c);
        slot ^= 1;
      }
      else {
        std::vector<double> R((size_t)cfg.nvar * c.n);
        rc = fill_chunk(&c, R.data());
        for (int v = 0; fits && v < cfg.nvar && !rc; v++) nbad += fits_convert_run(cfg, v, &R[(size_t)v * c.n], c.n);
        for (int v = 0; v < cfg.nvar && !rc; v++) {
          size_t o = (size_t)v * c.n;
          for (long pl = a; pl < b; pl++)
            for (long j = 0; j < s.rows; j++) {
              // plane pl, row j -> (iy, iz) of the ghosted array
              const long iy = (cfg.ndim == 3) ? j + nb : (cfg.ndim == 2 ? pl + nb : 0);
              const long iz = (cfg.ndim == 3) ? pl + nb : 0;
              memcpy(&A[(size_t)v * ncell + nb + (size_t)nxa * (iy + (size_t)nya * iz)], &R[o], (size_t)s.nx * sizeof(double));
              o += s.nx;
            }
        }
      }
      if (rc) io_error_ = who + ": reading the planes from " + paths[i] + " failed: " + last_error();
    }
    p0 = p1;
  }
  if (!rc && !stream) {
    rc = be_->upload(h_, A.data());
    if (rc) io_error_ = who + ": upload failed: " + last_error();
  }
  if (fits && stream) {
    // (after a failure too: the count of the chunks that were unpacked must not reach the next read)
    const int rs = be_->fits_read_status(h_, &nbad);
    if (!rc && rs) {
      rc = rs;
      io_error_ = who + ": reading the count of rejected elements failed: " + last_error();
    }
  }
  if (rc) return rc;
  if (nbad != 0) {
    io_error_ = who + ": " + std::to_string(nbad) + " element(s) of the files are not finite or hold the null value -1e99";
    return PION_GPU_EINVAL;
  }
  const pion_host_snapshot_info &I = H[0].info;
  T.simtime = I.t_sim;
  T.timestep = I.t_step;
  T.last_dt = I.last_dt;
  T.starttime = I.t_start;
  T.finishtime = I.t_finish;
  T.min_timestep = I.min_timestep;
  T.maxtime = false;
  if (T.op_criterion == 1 && I.op_criterion == 1) T.next_optime = I.next_optime;
  else if (T.op_criterion == 1) T.next_optime = T.simtime + T.opfreq_time;
  last_output_step_ = -1;
  // assign_boundary_data + TimeUpdateInternalBCs/ExternalBCs (sim_init.cpp:246-267)
  rc = update_boundaries(cfg.tm_ooa, cfg.tm_ooa, 1);
  if (rc) io_error_ = who + ": boundary update failed: " + last_error();
  else io_error_ = note;   // not a failure: what the files lacked
  return rc;
}

}  // namespace pion_host
