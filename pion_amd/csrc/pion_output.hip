// pion_output.hip -- the device part of the FITS output: pion_gpu_pack_fits packs the images of a chunk of planes
// (primitive variables, derived fields; B and divB scaled, every element already big-endian) into a device buffer the
// host writes as it arrives.  The rules -- image list, values, byte order, buffer layout -- are dev_output.h's; this
// file holds the two kernels that run them, the kernel of the read direction (k_unpack_fits: pion_gpu_unpack_fits, a
// restart from a FITS file) and the C-ABI entry points.
//
// All three kernels take k_pack_ongrid's mapping (pion_gpu.hip): one lane per double, consecutive along x, a wavefront
// per stretch of up to OUT_SEG cells of one row, so the 64-bit index arithmetic is paid once per stretch and loads and
// stores are whole lines; blockIdx.y: the image.  No LDS; no atomics in the pack kernels, at most one per wavefront in
// k_unpack_fits.  They are kernels of their own and not further instances of k_pack_ongrid: a transform parameter on
// that template renames its two existing instances, and their code objects are pinned.
#include <hip/hip_runtime.h>

#include <cstring>

#include "dev_output.h"
#include "pion_handle.h"

using namespace pion;
using namespace pion::impl;

namespace {

constexpr int OUT_WAVES = 4;

// one stretch of image `im`: cells [seg * OUT_SEG, ...) of row j of plane plane_lo + k
__device__ __forceinline__ void fits_stretch(const double *__restrict__ A, unsigned long long *__restrict__ buf,
                                             const GridDesc &g, const OutputCfg &o, const OutGeom &q, const int im,
                                             const long plane_lo, const long planes)
{
  const long u = (long)blockIdx.x * OUT_WAVES + (threadIdx.x >> 6);   // stretch: (plane, row, segment)
  const long nunit = planes * q.rows * q.nseg;
  if (u >= nunit) return;
  const long row = u / q.nseg;
  const int seg = (int)(u - row * q.nseg);
  const long k = row / q.rows;
  const long j = row - k * q.rows;
  const OutImage I = out_image(o, im);
  const long c0 = out_row_cell(q, plane_lo + k, j);
  const long b0 = out_row_buf(q, im, planes, k, j);
  const int jy = out_row_jy(g, plane_lo + k, j);
  const int x1 = min(q.nx, (seg + 1) * OUT_SEG);
  for (int ix = seg * OUT_SEG + (threadIdx.x & 63); ix < x1; ix += 64)
    buf[b0 + ix] = out_be64(out_value(g, o, I, A, c0 + ix, jy));
}

// images 0 .. nvar-1: the primitive variables (B scaled)
__global__ void __launch_bounds__(64 * OUT_WAVES)
k_pack_fits_prim(const double *__restrict__ A, unsigned long long *__restrict__ buf, const GridDesc g,
                 const OutputCfg o, const OutGeom q, const long plane_lo, const long planes)
{
  fits_stretch(A, buf, g, o, q, (int)blockIdx.y, plane_lo, planes);
}
// images nvar ..: Eint / Temp, divB, Ptot.  divB reads the 2 ndim neighbours of B: ghost cells of the rows' ends,
// ghost rows, and the planes next to [plane_lo, plane_lo + planes) -- on-grid planes of the neighbouring chunk or
// ghost planes, all inside the state array since nbc >= 1 on every axis the grid has
__global__ void __launch_bounds__(64 * OUT_WAVES)
k_pack_fits_derived(const double *__restrict__ A, unsigned long long *__restrict__ buf, const GridDesc g,
                    const OutputCfg o, const OutGeom q, const long plane_lo, const long planes)
{
  fits_stretch(A, buf, g, o, q, o.nvar + (int)blockIdx.y, plane_lo, planes);
}

// The read direction: the big-endian elements of the nvar primitive images of planes [plane_lo, plane_lo + planes),
// [nvar][planes][rows][nx], into the on-grid cells of BOTH state arrays (B times binv; ghost cells are not touched).
// fits_stretch's mapping -- a wavefront per stretch, 64-bit ids once per stretch, no LDS --; blockIdx.y: the variable.
// Rejected elements (in_rejected) are stored like any other and counted: a ballot per trip of the loop, summed by the
// wavefront's lane 0 (the lowest x, so it takes every trip a lane of the wavefront takes), one atomic add per wavefront
// that saw any.  A kernel of its own, for the reason the head of the file gives.
__global__ void __launch_bounds__(64 * OUT_WAVES)
k_unpack_fits(double *__restrict__ A0, double *__restrict__ A1, const unsigned long long *__restrict__ buf,
              const InputCfg in, const OutGeom q, const long ncell, const long plane_lo, const long planes,
              unsigned long long *__restrict__ nbad)
{
  const long u = (long)blockIdx.x * OUT_WAVES + (threadIdx.x >> 6);   // stretch: (plane, row, segment)
  const long nunit = planes * q.rows * q.nseg;
  if (u >= nunit) return;
  const long row = u / q.nseg;
  const int seg = (int)(u - row * q.nseg);
  const long k = row / q.rows;
  const long j = row - k * q.rows;
  const int v = (int)blockIdx.y;
  const OutImage I = out_image(in.o, v);
  const long c0 = (long)v * ncell + out_row_cell(q, plane_lo + k, j);
  const long b0 = out_row_buf(q, v, planes, k, j);
  const int x1 = min(q.nx, (seg + 1) * OUT_SEG);
  unsigned int n = 0;
  for (int ix = seg * OUT_SEG + (threadIdx.x & 63); ix < x1; ix += 64) {
    const double x = in_be64(buf[b0 + ix]);
    n += (unsigned int)__popcll(__ballot(in_rejected(x)));
    const double s = in_value(in, I, x);
    A0[c0 + ix] = s;
    A1[c0 + ix] = s;
  }
  if ((threadIdx.x & 63) == 0 && n) atomicAdd(nbad, (unsigned long long)n);
}

OutputCfg output_cfg(const Handle *h)
{
  OutputCfg o = out_cfg(h->cfg);
  o.Mu_tot_over_kB = h->Mu_tot_over_kB;
  return o;
}
bool too_many_tracers(Handle *h)
{
  if (h->cfg.ntracer <= OUT_MAX_TRACERS) return false;
  h->err = "FITS output: only accepts <= 5 tracers";
  return true;
}

}  // namespace

extern "C" {

int pion_gpu_fits_images(void *handle, char names[][16], int *n)
{
  Handle *h = (Handle *)handle;
  if (!h || !n) return PION_GPU_EINVAL;
  if (too_many_tracers(h)) return PION_GPU_EINVAL;
  const OutputCfg o = output_cfg(h);
  *n = out_nimage(o);
  if (names)
    for (int i = 0; i < *n; i++) {
      memset(names[i], 0, OUT_NAME_LEN);
      out_image_name(o, i, names[i]);
    }
  return 0;
}

long pion_gpu_fits_count(void *handle, int planes)
{
  Handle *h = (Handle *)handle;
  if (!h || planes < 0 || h->cfg.ntracer > OUT_MAX_TRACERS) return 0;
  return out_count(output_cfg(h), out_geom(h->g), planes);
}

int pion_gpu_pack_fits(void *handle, int plane_lo, int plane_hi, void *dbuf)
{
  Handle *h = use(handle);
  if (!h) return PION_GPU_EINVAL;
  if (too_many_tracers(h)) return PION_GPU_EINVAL;
  const OutGeom q = out_geom(h->g);
  if (!dbuf || plane_lo < 0 || plane_hi > q.nplanes || plane_lo >= plane_hi) {
    h->err = "pack_fits: plane range outside the grid, or no buffer";
    return PION_GPU_EINVAL;
  }
  if (int rc = order_after_unpack(h)) return rc;   // the ghost planes of a slab arrive on the communication stream
  const OutputCfg o = output_cfg(h);
  const long planes = plane_hi - plane_lo;
  const long nblk = (planes * q.rows * q.nseg + OUT_WAVES - 1) / OUT_WAVES;
  if (nblk > (1L << 31) - 1) {
    h->err = "pack_fits: plane range too large for one launch; pass it in parts";
    return PION_GPU_EINVAL;
  }
  const dim3 block(64 * OUT_WAVES);
  hipLaunchKernelGGL(k_pack_fits_prim, dim3((unsigned)nblk, (unsigned)o.nvar), block, 0, h->stream, h->dP,
                     (unsigned long long *)dbuf, h->g, o, q, (long)plane_lo, planes);
  HCHECK(h, hipGetLastError());
  hipLaunchKernelGGL(k_pack_fits_derived, dim3((unsigned)nblk, (unsigned)out_nderived(o)), block, 0, h->stream, h->dP,
                     (unsigned long long *)dbuf, h->g, o, q, (long)plane_lo, planes);
  HCHECK(h, hipGetLastError());
  return 0;
}

long pion_gpu_fits_prim_count(void *handle, int planes)
{
  Handle *h = (Handle *)handle;
  if (!h || planes < 0 || h->cfg.ntracer > OUT_MAX_TRACERS) return 0;
  return in_count(output_cfg(h), out_geom(h->g), planes);
}

int pion_gpu_unpack_fits(void *handle, int plane_lo, int plane_hi, const void *dbuf)
{
  Handle *h = use(handle);
  if (!h) return PION_GPU_EINVAL;
  if (too_many_tracers(h)) return PION_GPU_EINVAL;
  const OutGeom q = out_geom(h->g);
  if (!dbuf || plane_lo < 0 || plane_hi > q.nplanes || plane_lo >= plane_hi) {
    h->err = "unpack_fits: plane range outside the grid, or no buffer";
    return PION_GPU_EINVAL;
  }
  if (int rc = order_after_unpack(h)) return rc;
  InputCfg in = in_cfg(h->cfg);
  in.o = output_cfg(h);
  const long planes = plane_hi - plane_lo;
  const long nblk = (planes * q.rows * q.nseg + OUT_WAVES - 1) / OUT_WAVES;
  if (nblk > (1L << 31) - 1) {
    h->err = "unpack_fits: plane range too large for one launch; pass it in parts";
    return PION_GPU_EINVAL;
  }
  if (!h->dfits_bad) {
    HCHECK(h, hipMalloc((void **)&h->dfits_bad, sizeof(unsigned long long)));
    HCHECK(h, hipMemsetAsync(h->dfits_bad, 0, sizeof(unsigned long long), h->stream));
  }
  hipLaunchKernelGGL(k_unpack_fits, dim3((unsigned)nblk, (unsigned)in.o.nvar), dim3(64 * OUT_WAVES), 0, h->stream, h->dP,
                     h->dPh, (const unsigned long long *)dbuf, in, q, h->g.ncell, (long)plane_lo, planes, h->dfits_bad);
  HCHECK(h, hipGetLastError());
  // what pion_gpu_upload and pion_gpu_unpack_ongrid invalidate
  h->xghost_fresh = nullptr;
  h->ph_valid = false;
  state_changed(h);
  h->dt_requested = false;
  h->dt_mp_pending = false;
  return 0;
}

int pion_gpu_unpack_fits_status(void *handle, long *nbad)
{
  Handle *h = use(handle);
  if (!h || !nbad) return PION_GPU_EINVAL;
  *nbad = 0;
  HCHECK(h, hipStreamSynchronize(h->stream));
  if (!h->dfits_bad) return 0;   // nothing was unpacked yet
  unsigned long long n = 0;
  HCHECK(h, hipMemcpyAsync(&n, h->dfits_bad, sizeof n, hipMemcpyDeviceToHost, h->stream));
  HCHECK(h, hipMemsetAsync(h->dfits_bad, 0, sizeof n, h->stream));
  HCHECK(h, hipStreamSynchronize(h->stream));
  *nbad = (long)n;
  return 0;
}
}
