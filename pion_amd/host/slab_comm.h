// slab_comm.h -- what sim_control_gpu needs from a slab communicator (one process per GPU): the halo
// exchange of BC_update_BCMPI (boundaries/MCMD_boundaries.cpp:122-237) split into a start and a finish around the
// interior part of a stage, and the global minimum of the time step (sim_control_MPI.cpp:503-504).
// Beside the step path: a buffer handed one rank up (the projected image of a slab run, write_projection) or one
// rank up or down (a plane of column densities per source, write_columns).
// The slab axis is the grid's last axis: z in 3-D, y in 2-D, where the "planes" below are rows.
//
// Two implementations:
//   slab_comm_rccl  (slab_comm_rccl.h)  device-resident transfers over RCCL / xGMI -- the production transport;
//   slab_comm_shm   (slab_comm_shm.h)   the same protocol through host memory shared by the ranks of one node
//                                       (pinned staging buffers, POSIX shared-memory mailboxes): for ranks that
//                                       share one GPU, for boxes without an RCCL peer, and as the fall-back
//                                       transport (`bench.py --transport shm`).
#ifndef PION_SLAB_COMM_H
#define PION_SLAB_COMM_H

#include <cstddef>
#include <string>

namespace pion_host {

class slab_comm {
 public:
  virtual ~slab_comm() {}
  // bind to the backend handle whose state is exchanged; must precede start()
  virtual int attach(void *handle) = 0;
  // first half: the on-grid planes next to the internal slab-axis faces of array `which` (0 = P, 1 = Ph) leave.
  // Returns at once.
  virtual int start(int which) = 0;
  // second half: the ghost planes are (ordered to be) filled before the slab-boundary part of the next stage
  virtual int finish() = 0;
  // global minimum of the device-resident {t_dyn, t_mp}: request_min() starts it (right after the full-step
  // stage), allreduce_min() waits for it -- the single host synchronisation of a step
  virtual int request_min() = 0;
  virtual int allreduce_min(double *t_dyn, double *t_mp) = 0;
  // a new state was uploaded (sim_control_gpu::Init): complete an exchange in flight, forget a pending request
  virtual int reset() = 0;
  // A buffer of any length moved one rank up the chain (the projected image of a slab run, dev_project.h "parts"):
  // recv_from_below takes the message of rank - 1 into `host`, send_to_above hands one to rank + 1.  Not periodic:
  // rank 0 receives from nobody and the last rank sends to nobody (both return 0 at once; *status = 0).  Every message
  // is preceded by a status word: a rank that failed sends status != 0 and no data, the receiver gets it in *status
  // (and 0 as its own return value), so a failure travels down the chain and no rank blocks.  send_to_above returns
  // once the receiver has taken the message.  A message whose length is not `bytes` (or any message, with host ==
  // nullptr) is taken off the wire and EINVAL.  has_relay() tells whether the transport has the pair; the default has
  // not, and its two calls return "not supported" (PION_GPU_EINVAL).  Nothing of the step path calls them.
  virtual bool has_relay() const { return false; }
  virtual int recv_from_below(void *host, size_t bytes, int *status)
  {
    (void)host, (void)bytes, (void)status;
    return -1;
  }
  virtual int send_to_above(const void *host, size_t bytes, int status)
  {
    (void)host, (void)bytes, (void)status;
    return -1;
  }
  // The same pair one rank DOWN the chain (the planes of the ray tracer travel away from the source, both ways:
  // columns_io.cpp): recv_from_above takes the message of rank + 1, send_to_below hands one to rank - 1; the last rank
  // receives from nobody and rank 0 sends to nobody.  The same status-word protocol: a failing rank sends a status and
  // no data, no rank blocks.  has_relay_down() tells whether the transport has the pair; the default has not.
  virtual bool has_relay_down() const { return false; }
  virtual int recv_from_above(void *host, size_t bytes, int *status)
  {
    (void)host, (void)bytes, (void)status;
    return -1;
  }
  virtual int send_to_below(const void *host, size_t bytes, int status)
  {
    (void)host, (void)bytes, (void)status;
    return -1;
  }
  virtual const std::string &last_error() const = 0;
  // this process's place among the ranks (file names and headers of snapshots)
  virtual int rank() const { return 0; }
  virtual int world() const { return 1; }
};

}  // namespace pion_host
#endif
