// dev_output.h -- the rules of the FITS output (the reference's dataio_fits::OutputData, dataIO/dataio_fits.cpp:147-320,
// and put_variable_into_data_array, :748-856), each stated once: which images a file holds and in what order, the value
// of one image at one cell, the byte order of a stored value, and how the on-grid cells map to the image buffer.
// At the end of the file the same rules for the read direction (DataIOFits::ReadData and read_fits_image, :433-548,
// 865-929): which images a restart reads, what the state holds for a file element, which elements it refuses.
// Plain __host__ __device__ functions of GridDesc and OutputCfg: the kernels of pion_output.hip run them on the device,
// the host writer and reader (pion_amd/host/fits_io.cpp) run the same functions in a host loop for a backend without
// the streaming entries.  Needs only GridDesc and the PION_* constants (the includer provides __host__ / __device__, as
// for dev_bc.h).
//
// Every function that does arithmetic is compiled without FMA contraction, in both builds and on the host: the images
// are compared with == against a restatement of the reference's expressions, and a file must not depend on which
// build or which route wrote it.
//
// The ghost cells the divB stencil reads hold whatever the last boundary update (and, for a slab, the last halo
// exchange) left: the loop writes its outputs after update_bcs, and a caller of pion_gpu_pack_fits must do the same.
//
// The divergence is NOT shared with the HLL-switch prepass (prepass_hlld_cell, kernels_prepass.hip): that one is compiled
// per floating-point mode (contracted in the fast build), falls back to a one-sided difference where the all-cell
// array ends, and runs on velocities; this one has both neighbours by construction (an on-grid cell always has them,
// ghosts included) and must give the same bits in both builds.
#ifndef PION_DEV_OUTPUT_H
#define PION_DEV_OUTPUT_H

#include <cmath>

#include "../../include/pion_gpu.h"
#include "grid_desc.h"

namespace pion {

#define PION_OUT_HD __host__ __device__ inline

// kinds of image
enum OutKind {
  OUT_PRIM = 0,     // a primitive variable as it is stored
  OUT_PRIM_B = 1,   // a component of B: times sqrt(4 pi) (NEW_B_NORM, defines/functionality_flags.h:42)
  OUT_EINT = 2,     // p / (gamma - 1) / rho                 eqns_hydro_adiabatic.cpp:374-380, eqns_mhd_adiabatic.cpp:445-451
  OUT_TEMP = 3,     // p Mu_tot_over_kB / rho                mp_only_cooling.cpp:274-280
  OUT_DIVB = 4,     // Divergence(c, 0, {BX, BY, BZ}) times sqrt(4 pi)    VectorOps.cpp:377-439, 891-965
  OUT_PTOT = 5      // p + 0.5 (Bx^2 + By^2 + Bz^2), code units            eqns_mhd_adiabatic.cpp:474-480
};
constexpr int OUT_MAX_TRACERS = 5;                    // dataio_fits.cpp:157
constexpr int OUT_MAX_IMAGES = PION_MAX_NVAR + 3;
constexpr int OUT_NAME_LEN = 16;
// state-vector positions (the library's order: rho, p, v, B, psi, tracers)
constexpr int OUT_RO = 0, OUT_PG = 1, OUT_BX = 5;

struct OutputCfg {
  int eqntype, nvar, ntracer, cooling;
  double gamma, Mu_tot_over_kB, bscale;   // bscale: sqrt(4 pi), evaluated once on the host
};

// the configuration's part of the rules.  Host only (libm sqrt); the constants are mp_only_cooling's
// (mp_only_cooling.cpp:81-95, constants.h:53,64), the expression is pion_gpu_create's
inline OutputCfg out_cfg(const pion_gpu_config &c)
{
  OutputCfg o;
  o.eqntype = c.eqntype;
  o.nvar = c.nvar;
  o.ntracer = c.ntracer;
  o.cooling = c.cooling;
  o.gamma = c.gamma;
  const double m_p = 1.672621898e-24, kB = 1.38064852e-16;
  const double Mu_tot = 0.609 * m_p;
  o.Mu_tot_over_kB = Mu_tot / kB;
  o.bscale = std::sqrt(4.0 * M_PI);
  return o;
}

// ---- the image list: the primitive variables in state order (GasDens GasPres GasVX GasVY GasVZ [Bx By Bz [psi]]
// TR0 ...), then Eint (no microphysics) or Temp (EP.cooling != 0), then for MHD and GLM divB and Ptot
PION_OUT_HD bool out_is_mhd(const OutputCfg &o) { return o.eqntype == PION_EQMHD || o.eqntype == PION_EQGLM; }
PION_OUT_HD int out_nderived(const OutputCfg &o) { return out_is_mhd(o) ? 3 : 1; }
PION_OUT_HD int out_nimage(const OutputCfg &o) { return o.nvar + out_nderived(o); }

struct OutImage {
  int kind, var;   // var: the variable of a primitive image
};
PION_OUT_HD OutImage out_image(const OutputCfg &o, const int i)
{
  OutImage im;
  im.var = 0;
  if (i < o.nvar) {
    im.var = i;
    im.kind = (out_is_mhd(o) && i >= OUT_BX && i < OUT_BX + 3) ? OUT_PRIM_B : OUT_PRIM;
  }
  else if (i == o.nvar) im.kind = (o.cooling != 0) ? OUT_TEMP : OUT_EINT;
  else im.kind = (i == o.nvar + 1) ? OUT_DIVB : OUT_PTOT;
  return im;
}
// EXTNAME of image i, NUL-terminated
PION_OUT_HD void out_image_name(const OutputCfg &o, const int i, char *name)
{
  const char *const prim[9] = {"GasDens", "GasPres", "GasVX", "GasVY", "GasVZ", "Bx", "By", "Bz", "psi"};
  const int nbase = o.nvar - o.ntracer;
  const OutImage im = out_image(o, i);
  const char *s = nullptr;
  if (i < nbase) s = prim[i];
  else if (i < o.nvar) {
    name[0] = 'T', name[1] = 'R', name[2] = (char)('0' + (i - nbase)), name[3] = 0;
    return;
  }
  else s = (im.kind == OUT_EINT) ? "Eint" : (im.kind == OUT_TEMP) ? "Temp" : (im.kind == OUT_DIVB) ? "divB" : "Ptot";
  int k = 0;
  for (; s[k] && k < OUT_NAME_LEN - 1; k++) name[k] = s[k];
  name[k] = 0;
}

// ---- the value of one image at cell c (all-cell id) of the state array S ([nvar][ncell]); jy_all: the cell's
// all-cell y index (read on cylindrical grids only).  The expressions in the reference's order of operations.
PION_OUT_HD double out_divB(const GridDesc &g, const double *S, const long c, const int jy_all)
{
#ifdef __clang__
#pragma clang fp contract(off)
#endif
  const long nc = g.ncell;
  const double dx = g.dx;
  double divv = 0.0;
  if (g.cyl == 1) {
    // VectorOps_Cyl::Divergence: d(B_z)/dz + d(R B_R)/(R dR) between the neighbours' centres of mass
    divv = (S[(long)OUT_BX * nc + c + 1] - S[(long)OUT_BX * nc + c - 1]) / (2.0 * dx);
    // cell centre along R (cell_interface.cpp:506-512) and VectorOps_Cyl::R_com (VectorOps.h:414-418)
    const double Rn = g.xmin[1] + (2 * (jy_all - 1 - g.nbc[1]) + 1) * (0.5 * dx);
    const double Rp = g.xmin[1] + (2 * (jy_all + 1 - g.nbc[1]) + 1) * (0.5 * dx);
    const double rn = Rn + dx * dx / 12. / Rn;
    const double rp = Rp + dx * dx / 12. / Rp;
    divv += 2.0 * (rp * S[(long)(OUT_BX + 1) * nc + c + g.sy] - rn * S[(long)(OUT_BX + 1) * nc + c - g.sy]) / (rp * rp - rn * rn);
    return divv;
  }
  // VectorOps_Cart::Divergence: both neighbours exist, dx[v] = 2.0 * dx
  for (int v = 0; v < g.ndim; v++) {
    const long st = (v == 0) ? 1 : ((v == 1) ? g.sy : g.sz);
    divv += (S[(long)(OUT_BX + v) * nc + c + st] - S[(long)(OUT_BX + v) * nc + c - st]) / (2.0 * dx);
  }
  return divv;
}

PION_OUT_HD double out_value(const GridDesc &g, const OutputCfg &o, const OutImage im, const double *S, const long c,
                             const int jy_all)
{
#ifdef __clang__
#pragma clang fp contract(off)
#endif
  const long nc = g.ncell;
  switch (im.kind) {
    case OUT_PRIM: return S[(long)im.var * nc + c];
    case OUT_PRIM_B: return S[(long)im.var * nc + c] * o.bscale;
    case OUT_EINT: return S[(long)OUT_PG * nc + c] / (o.gamma - 1.0) / S[(long)OUT_RO * nc + c];
    case OUT_TEMP: return S[(long)OUT_PG * nc + c] * o.Mu_tot_over_kB / S[(long)OUT_RO * nc + c];
    case OUT_DIVB: return out_divB(g, S, c, jy_all) * o.bscale;
    default: {
      const double bx = S[(long)OUT_BX * nc + c], by = S[(long)(OUT_BX + 1) * nc + c], bz = S[(long)(OUT_BX + 2) * nc + c];
      return S[(long)OUT_PG * nc + c] + 0.5 * (bx * bx + by * by + bz * bz);
    }
  }
}

// a stored element: the IEEE-754 double, most significant byte first (FITS standard 4.0, s5.3), as the 8 bytes of the
// returned integer in this machine's (little-endian) memory order
PION_OUT_HD unsigned long long out_be64(const double x)
{
  unsigned long long u;
  __builtin_memcpy(&u, &x, sizeof u);
  return __builtin_bswap64(u);
}

// ---- the image buffer [nimage][planes][rows][nx]: a plane of the slab axis (the last axis) is `rows` runs of nx
// on-grid cells (3-D: the ny rows of an x-y plane; 2-D: one row; 1-D: the one row there is) -- pion_gpu_pack_ongrid's
// layout with images in place of variables.  A stretch is up to OUT_SEG cells of one row.
constexpr int OUT_SEG = 1024;
struct OutGeom {
  long off0;     // cell id of the first on-grid cell of plane 0
  long ps, rs;   // cell-id strides of a plane and of a row inside a plane
  int nx, rows, nseg, nplanes;   // nseg: stretches per row; nplanes: planes of the grid
};
PION_OUT_HD OutGeom out_geom(const GridDesc &g)
{
  OutGeom q;
  q.nx = g.ng[0];
  q.nseg = (q.nx + OUT_SEG - 1) / OUT_SEG;
  q.off0 = g.nbc[0];
  q.ps = q.rs = 0;
  q.rows = 1;
  q.nplanes = 1;
  if (g.ndim == 2) {
    q.off0 += g.sy * g.nbc[1];
    q.ps = g.sy;
    q.nplanes = g.ng[1];
  }
  else if (g.ndim == 3) {
    q.off0 += g.sy * g.nbc[1] + g.sz * g.nbc[2];
    q.ps = g.sz;
    q.rs = g.sy;
    q.rows = g.ng[1];
    q.nplanes = g.ng[2];
  }
  return q;
}
// first cell of row j of plane k, and its all-cell y index
PION_OUT_HD long out_row_cell(const OutGeom &q, const long k, const long j) { return q.off0 + k * q.ps + j * q.rs; }
PION_OUT_HD int out_row_jy(const GridDesc &g, const long k, const long j)
{
  return (g.ndim == 3) ? (int)j + g.nbc[1] : ((g.ndim == 2) ? (int)k + g.nbc[1] : 0);
}
// first buffer element of row j of plane k (counted from the chunk's first plane) of image im
PION_OUT_HD long out_row_buf(const OutGeom &q, const long im, const long planes, const long k, const long j)
{
  return ((im * planes + k) * q.rows + j) * q.nx;
}
PION_OUT_HD long out_count(const OutputCfg &o, const OutGeom &q, const long planes)
{
  return (long)out_nimage(o) * planes * q.rows * q.nx;
}

// ---- the read direction (the reference's DataIOFits::ReadData and read_fits_image, dataio_fits.cpp:433-548,
// 865-929): a restart reads the nvar primitive images of out_image's list -- images 0 .. nvar-1, found by their
// out_image_name -- and never the derived ones (:901-903).
//
// InputCfg: OutputCfg and what only a read needs.  OutputCfg keeps its layout: it is an argument of the pack kernels.
struct InputCfg {
  OutputCfg o;
  double binv;   // 1.0 / sqrt(4.0 * M_PI), evaluated once on the host (the reference's `norm`, :911)
};
inline InputCfg in_cfg(const pion_gpu_config &c)
{
  InputCfg in;
  in.o = out_cfg(c);
  in.binv = 1.0 / std::sqrt(4.0 * M_PI);
  return in;
}

// the inverse of out_be64: the double whose big-endian bytes are the 8 bytes of u in memory order
PION_OUT_HD double in_be64(const unsigned long long u)
{
  const unsigned long long s = __builtin_bswap64(u);
  double x;
  __builtin_memcpy(&x, &s, sizeof x);
  return x;
}
// the value the state holds for file element x of image im: B times binv (:911-916; a multiplication, so that a B
// written and read back may differ from the one that was written in the last bit), everything else -- psi included --
// as it is stored
PION_OUT_HD double in_value(const InputCfg &in, const OutImage im, const double x)
{
#ifdef __clang__
#pragma clang fp contract(off)
#endif
  return (im.kind == OUT_PRIM_B) ? x * in.binv : x;
}
// a file element no restart accepts: not finite, or the reference's null value -- constants::equalD(x, -1.e99)
// (constants.cpp:48-70; :908-921).  The reference tests the element as the file holds it, before the B scaling.
PION_OUT_HD bool in_rejected(const double x)
{
#ifdef __clang__
#pragma clang fp contract(off)
#endif
  const double nulval = -1.e99, ax = fabs(x);
  if (!(ax <= 1.7976931348623157e308)) return true;   // NaN or infinity
  if (x == nulval) return true;
  return (fabs(x - nulval) / (ax + fabs(nulval) + 1.0e-100)) < 1.0e-12;   // (|x| + 1e99 < 1e-100 never holds)
}
// the buffer of a read, [nvar][planes][rows][nx]: out_row_buf with the variable in place of the image
PION_OUT_HD long in_count(const OutputCfg &o, const OutGeom &q, const long planes)
{
  return (long)o.nvar * planes * q.rows * q.nx;
}

}  // namespace pion
#endif
