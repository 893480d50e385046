// pion_backend_gpu.cpp -- pion_backend bound to libpion_gpu.so (include/pion_gpu.h): the only backend of the product.
#include "pion_backend.h"

#include <hip/hip_runtime_api.h>

#include <map>
#include <mutex>

namespace {

int gpu_dt_begin(void *h)
{
  void *d = nullptr;
  if (int rc = pion_gpu_calc_dt_device(h, &d)) return rc;
  return pion_gpu_dt_request(h);
}

// staged halos: in place from / into the state arrays (pion_gpu_halo_spans), on the communication stream the
// library orders against the compute stream (pion_gpu_halo_begin / _end)
hipStream_t comm_stream_of(void *h)
{
  void *cs = pion_gpu_get_stream(h, 1);
  return (hipStream_t)(cs ? cs : pion_gpu_get_stream(h, 0));
}
int gpu_halo_to_host_begin(void *h, int which, double *lo, double *hi)
{
  pion_gpu_halo_spans_t sp;
  if (int rc = pion_gpu_halo_spans(h, which, &sp)) return rc;
  if (int rc = pion_gpu_halo_begin(h)) return rc;   // after the stage + boundary kernels that wrote the planes
  hipStream_t s = comm_stream_of(h);
  const size_t n = (size_t)sp.count_per_var, nb = n * sizeof(double);
  for (int v = 0; v < sp.nvar; v++) {
    const long o = (long)v * sp.var_stride;
    if (lo && hipMemcpyAsync(lo + (size_t)v * n, sp.send_lo + o, nb, hipMemcpyDeviceToHost, s) != hipSuccess)
      return PION_GPU_EDEVICE;
    if (hi && hipMemcpyAsync(hi + (size_t)v * n, sp.send_hi + o, nb, hipMemcpyDeviceToHost, s) != hipSuccess)
      return PION_GPU_EDEVICE;
  }
  return 0;
}
int gpu_halo_to_host_end(void *h)
{
  return hipStreamSynchronize(comm_stream_of(h)) == hipSuccess ? 0 : PION_GPU_EDEVICE;
}
int gpu_halo_from_host(void *h, int which, const double *lo, const double *hi)
{
  pion_gpu_halo_spans_t sp;
  if (int rc = pion_gpu_halo_spans(h, which, &sp)) return rc;
  hipStream_t s = comm_stream_of(h);
  const size_t n = (size_t)sp.count_per_var, nb = n * sizeof(double);
  for (int v = 0; v < sp.nvar; v++) {
    const long o = (long)v * sp.var_stride;
    if (lo && hipMemcpyAsync(sp.recv_lo + o, lo + (size_t)v * n, nb, hipMemcpyHostToDevice, s) != hipSuccess)
      return PION_GPU_EDEVICE;
    if (hi && hipMemcpyAsync(sp.recv_hi + o, hi + (size_t)v * n, nb, hipMemcpyHostToDevice, s) != hipSuccess)
      return PION_GPU_EDEVICE;
  }
  // the host buffers may be reused by the caller: the copies must have left them
  if (hipStreamSynchronize(s) != hipSuccess) return PION_GPU_EDEVICE;
  return pion_gpu_halo_end(h);   // the z-boundary part of the next stage waits for this point
}

// Snapshot streaming: per handle, two device staging buffers and two pinned host buffers of one chunk each,
// allocated at the first chunk (grown if a later chunk is larger) and freed with the handle.  Everything is enqueued
// on the handle's compute stream -- a snapshot is taken between steps, so there is nothing to overlap with on the
// device; what overlaps is the host's file I/O on one slot with the pack + copy of the other.
struct Staging {
  double *dev[2] = {nullptr, nullptr}, *host[2] = {nullptr, nullptr};
  long cap[2] = {0, 0};              // doubles
  hipEvent_t ev[2] = {nullptr, nullptr};
  bool busy[2] = {false, false};     // an event was recorded for the slot and not waited for yet
};
std::mutex g_staging_mu;
std::map<void *, Staging> g_staging;

void staging_free(Staging &st)
{
  for (int i = 0; i < 2; i++) {
    if (st.ev[i]) (void)hipEventDestroy(st.ev[i]);
    if (st.dev[i]) (void)hipFree(st.dev[i]);
    if (st.host[i]) (void)hipHostFree(st.host[i]);
  }
  st = Staging();
}
// the slot's buffers, holding at least n doubles; a slot in flight is waited for before it is touched
int staging_slot(void *h, int slot, long n, Staging **out)
{
  if (slot < 0 || slot > 1 || n <= 0) return PION_GPU_EINVAL;
  Staging *st;
  {
    std::lock_guard<std::mutex> lk(g_staging_mu);
    st = &g_staging[h];   // (std::map: the address stays valid)
  }
  if (st->busy[slot]) {
    if (hipEventSynchronize(st->ev[slot]) != hipSuccess) return PION_GPU_EDEVICE;
    st->busy[slot] = false;
  }
  if (!st->ev[slot] && hipEventCreateWithFlags(&st->ev[slot], hipEventDisableTiming) != hipSuccess) return PION_GPU_EDEVICE;
  if (st->cap[slot] < n) {
    if (st->dev[slot]) (void)hipFree(st->dev[slot]);
    if (st->host[slot]) (void)hipHostFree(st->host[slot]);
    st->dev[slot] = st->host[slot] = nullptr;
    st->cap[slot] = 0;
    if (hipMalloc((void **)&st->dev[slot], (size_t)n * sizeof(double)) != hipSuccess) return PION_GPU_ENOMEM;
    if (hipHostMalloc((void **)&st->host[slot], (size_t)n * sizeof(double), hipHostMallocDefault) != hipSuccess)
      return PION_GPU_ENOMEM;
    st->cap[slot] = n;
  }
  *out = st;
  return 0;
}
hipStream_t compute_stream_of(void *h) { return (hipStream_t)pion_gpu_get_stream(h, 0); }
// what a slot holds for a chunk of `planes` planes: the largest of the three buffers that pass through it, so that a
// write and a read of either file type in turn do not reallocate it
long slot_elems(void *h, int planes)
{
  long n = pion_gpu_ongrid_count(h, planes);
  if (pion_gpu_fits_count(h, planes) > n) n = pion_gpu_fits_count(h, planes);
  if (pion_gpu_fits_prim_count(h, planes) > n) n = pion_gpu_fits_prim_count(h, planes);
  return n;
}

// pack (the variables of array `which`, or the FITS images of P) into the slot's device buffer, then copy
int gpu_to_host_begin(void *h, bool fits, int which, int plane_lo, int plane_hi, int slot)
{
  const long n = fits ? pion_gpu_fits_count(h, plane_hi - plane_lo) : pion_gpu_ongrid_count(h, plane_hi - plane_lo);
  Staging *st;
  if (int rc = staging_slot(h, slot, n > 0 ? slot_elems(h, plane_hi - plane_lo) : n, &st)) return rc;
  if (int rc = fits ? pion_gpu_pack_fits(h, plane_lo, plane_hi, st->dev[slot])
                    : pion_gpu_pack_ongrid(h, which, plane_lo, plane_hi, st->dev[slot]))
    return rc;
  hipStream_t s = compute_stream_of(h);
  if (hipMemcpyAsync(st->host[slot], st->dev[slot], (size_t)n * sizeof(double), hipMemcpyDeviceToHost, s) != hipSuccess)
    return PION_GPU_EDEVICE;
  if (hipEventRecord(st->ev[slot], s) != hipSuccess) return PION_GPU_EDEVICE;
  st->busy[slot] = true;
  return 0;
}
int gpu_ongrid_to_host_begin(void *h, int which, int plane_lo, int plane_hi, int slot)
{
  return gpu_to_host_begin(h, false, which, plane_lo, plane_hi, slot);
}
int gpu_fits_to_host_begin(void *h, int plane_lo, int plane_hi, int slot)
{
  return gpu_to_host_begin(h, true, 0, plane_lo, plane_hi, slot);
}
int gpu_ongrid_to_host_end(void *h, int slot, const double **host)
{
  if (slot < 0 || slot > 1 || !host) return PION_GPU_EINVAL;
  Staging *st;
  {
    std::lock_guard<std::mutex> lk(g_staging_mu);
    auto it = g_staging.find(h);
    if (it == g_staging.end()) return PION_GPU_EINVAL;
    st = &it->second;
  }
  if (!st->busy[slot]) return PION_GPU_EINVAL;   // no _begin for this slot
  if (hipEventSynchronize(st->ev[slot]) != hipSuccess) return PION_GPU_EDEVICE;
  st->busy[slot] = false;
  *host = st->host[slot];
  return 0;
}
// fill the slot's host buffer, copy, then unpack (the variables as they are, or the big-endian elements of a FITS file)
int gpu_from_host(void *h, bool fits, int plane_lo, int plane_hi, int slot, int (*fill)(void *, double *), void *ctx)
{
  if (!fill) return PION_GPU_EINVAL;
  const long n = fits ? pion_gpu_fits_prim_count(h, plane_hi - plane_lo) : pion_gpu_ongrid_count(h, plane_hi - plane_lo);
  Staging *st;
  // (waits for the slot's previous copy)
  if (int rc = staging_slot(h, slot, n > 0 ? slot_elems(h, plane_hi - plane_lo) : n, &st)) return rc;
  if (int rc = fill(ctx, st->host[slot])) return rc;
  hipStream_t s = compute_stream_of(h);
  if (hipMemcpyAsync(st->dev[slot], st->host[slot], (size_t)n * sizeof(double), hipMemcpyHostToDevice, s) != hipSuccess)
    return PION_GPU_EDEVICE;
  if (int rc = fits ? pion_gpu_unpack_fits(h, plane_lo, plane_hi, st->dev[slot])
                    : pion_gpu_unpack_ongrid(h, plane_lo, plane_hi, st->dev[slot]))
    return rc;
  if (hipEventRecord(st->ev[slot], s) != hipSuccess) return PION_GPU_EDEVICE;
  st->busy[slot] = true;
  return 0;
}
int gpu_ongrid_from_host(void *h, int plane_lo, int plane_hi, int slot, int (*fill)(void *, double *), void *ctx)
{
  return gpu_from_host(h, false, plane_lo, plane_hi, slot, fill, ctx);
}
int gpu_fits_from_host(void *h, int plane_lo, int plane_hi, int slot, int (*fill)(void *, double *), void *ctx)
{
  return gpu_from_host(h, true, plane_lo, plane_hi, slot, fill, ctx);
}
// the images of one call: projected into slot 0's device buffer, copied into the caller's memory, waited for
int gpu_project_to_host(void *h, int axis, int nfields, const pion_gpu_proj_field *fields, double *host)
{
  const long n = pion_gpu_project_count(h, axis, nfields);
  if (n < 0) return (int)n;
  if (!host) return PION_GPU_EINVAL;
  Staging *st;
  if (int rc = staging_slot(h, 0, n, &st)) return rc;
  if (int rc = pion_gpu_project(h, 0, axis, nfields, fields, st->dev[0])) return rc;
  hipStream_t s = compute_stream_of(h);
  if (hipMemcpyAsync(host, st->dev[0], (size_t)n * sizeof(double), hipMemcpyDeviceToHost, s) != hipSuccess)
    return PION_GPU_EDEVICE;
  return hipStreamSynchronize(s) == hipSuccess ? 0 : PION_GPU_EDEVICE;
}
// a rank's part: the image travels host -> slot 0's device buffer -> (the part's kernel) -> host
int gpu_project_part_to_host(void *h, int axis, int nfields, const pion_gpu_proj_field *fields, const pion_gpu_proj_part *part,
                             double *host)
{
  const long n = pion_gpu_project_part_count(h, axis, nfields, part);
  if (n < 0) return (int)n;
  if (!host) return PION_GPU_EINVAL;
  Staging *st;
  if (int rc = staging_slot(h, 0, n, &st)) return rc;
  hipStream_t s = compute_stream_of(h);
  if (hipMemcpyAsync(st->dev[0], host, (size_t)n * sizeof(double), hipMemcpyHostToDevice, s) != hipSuccess)
    return PION_GPU_EDEVICE;
  if (int rc = pion_gpu_project_part(h, 0, axis, nfields, fields, part, st->dev[0])) return rc;
  if (hipMemcpyAsync(host, st->dev[0], (size_t)n * sizeof(double), hipMemcpyDeviceToHost, s) != hipSuccess)
    return PION_GPU_EDEVICE;
  return hipStreamSynchronize(s) == hipSuccess ? 0 : PION_GPU_EDEVICE;
}
// the inclined images of one call: projected into slot 0's device buffer, copied, waited for (by the status call)
int gpu_project_angle_to_host(void *h, double angle_deg, int nfields, const pion_gpu_proj_field *fields, double *host, long *ncapped)
{
  const long n = pion_gpu_project_angle_count(h, angle_deg, nfields, nullptr);
  if (n < 0) return (int)n;
  if (!host || !ncapped) return PION_GPU_EINVAL;
  Staging *st;
  if (int rc = staging_slot(h, 0, n, &st)) return rc;
  if (int rc = pion_gpu_project_angle(h, 0, angle_deg, nfields, fields, st->dev[0])) return rc;
  hipStream_t s = compute_stream_of(h);
  if (hipMemcpyAsync(host, st->dev[0], (size_t)n * sizeof(double), hipMemcpyDeviceToHost, s) != hipSuccess)
    return PION_GPU_EDEVICE;
  return pion_gpu_project_angle_status(h, ncapped);
}
// a plane range of one column array: packed big-endian into the slot's device buffer, then copied
int gpu_columns_to_host_begin(void *h, int id, int what, int plane_lo, int plane_hi, int slot)
{
  const long n = pion_gpu_rt_count(h, plane_hi - plane_lo);
  Staging *st;
  if (int rc = staging_slot(h, slot, n, &st)) return rc;
  if (int rc = pion_gpu_pack_columns(h, id, what, plane_lo, plane_hi, st->dev[slot])) return rc;
  hipStream_t s = compute_stream_of(h);
  if (hipMemcpyAsync(st->host[slot], st->dev[slot], (size_t)n * sizeof(double), hipMemcpyDeviceToHost, s) != hipSuccess)
    return PION_GPU_EDEVICE;
  if (hipEventRecord(st->ev[slot], s) != hipSuccess) return PION_GPU_EDEVICE;
  st->busy[slot] = true;
  return 0;
}
// one source of a slab run: slot 0's device buffer holds the three planes [received][lowest own][highest own]
int gpu_raytrace_part_faces(void *h, int which, int id, const double *face_in, double *face_lo, double *face_hi)
{
  const long n = pion_gpu_rt_count(h, 1);
  Staging *st;
  if (int rc = staging_slot(h, 0, 3 * n, &st)) return rc;
  hipStream_t s = compute_stream_of(h);
  double *d = st->dev[0];
  const size_t bytes = (size_t)n * sizeof(double);
  if (face_in && hipMemcpyAsync(d, face_in, bytes, hipMemcpyHostToDevice, s) != hipSuccess) return PION_GPU_EDEVICE;
  if (int rc = pion_gpu_raytrace_part(h, which, id, face_in ? d : nullptr, face_lo ? d + n : nullptr, face_hi ? d + 2 * n : nullptr))
    return rc;
  if (face_lo && hipMemcpyAsync(face_lo, d + n, bytes, hipMemcpyDeviceToHost, s) != hipSuccess) return PION_GPU_EDEVICE;
  if (face_hi && hipMemcpyAsync(face_hi, d + 2 * n, bytes, hipMemcpyDeviceToHost, s) != hipSuccess) return PION_GPU_EDEVICE;
  return hipStreamSynchronize(s) == hipSuccess ? 0 : PION_GPU_EDEVICE;
}
void gpu_destroy(void *h)
{
  Staging st;
  bool have = false;
  {
    std::lock_guard<std::mutex> lk(g_staging_mu);
    auto it = g_staging.find(h);
    if (it != g_staging.end()) {
      st = it->second;
      have = true;
      g_staging.erase(it);
    }
  }
  if (have) {
    (void)pion_gpu_synchronize(h);
    staging_free(st);
  }
  pion_gpu_destroy(h);
}

const pion_backend k_gpu = {
    "libpion_gpu.so",
    pion_gpu_create,
    gpu_destroy,
    pion_gpu_last_error,
    pion_gpu_upload,
    pion_gpu_download,
    pion_gpu_update_bcs,
    pion_gpu_stage,
    pion_gpu_stage_part,
    pion_gpu_set_glm_speeds,
    pion_gpu_calc_dt,
    gpu_dt_begin,
    pion_gpu_dt_wait,
    pion_gpu_halo_count,
    gpu_halo_to_host_begin,
    gpu_halo_to_host_end,
    gpu_halo_from_host,
    pion_gpu_ongrid_count,
    gpu_ongrid_to_host_begin,
    gpu_ongrid_to_host_end,
    gpu_ongrid_from_host,
    pion_gpu_fits_count,
    gpu_fits_to_host_begin,
    gpu_fits_from_host,
    pion_gpu_unpack_fits_status,
    pion_gpu_project_count,
    gpu_project_to_host,
    pion_gpu_project_part_count,
    gpu_project_part_to_host,
    pion_gpu_add_rt_source,
    pion_gpu_raytrace,
    pion_gpu_rt_count,
    gpu_columns_to_host_begin,
    pion_gpu_add_rt_source_part,
    gpu_raytrace_part_faces,
    pion_gpu_project_angle_count,
    gpu_project_angle_to_host,
};

}  // namespace

extern "C" const pion_backend *pion_backend_gpu(void) { return &k_gpu; }
