// slab_comm_shm.h -- the slab protocol of slab_comm.h through host memory shared by the ranks of one node.
//
// Same role as slab_comm_rccl (it replaces comm_mpi::send_cell_data / receive_cell_data, comms/comm_mpi.cpp:287-425,
// and global_operation_double("MIN"), :182-209, for this path), different wire: the planes of a face leave the
// device into a pinned staging buffer (pion_backend::halo_to_host_begin, on the communication stream, while the
// compute stream runs the interior part of the next stage), are copied into the neighbour's mailbox in a POSIX
// shared-memory segment, and enter the neighbour's ghost planes from there (halo_from_host).  The time-step
// minimum is reduced through the same segment.  No MPI, no RCCL, no torch: ranks need only a common segment name.
// Use: ranks that share one GPU (tests), boxes without an RCCL peer, fall-back transport of bench.py.
#ifndef PION_SLAB_COMM_SHM_H
#define PION_SLAB_COMM_SHM_H

#include <string>

#include "pion_backend.h"
#include "slab_comm.h"

namespace pion_host {

class slab_comm_shm : public slab_comm {
 public:
  // name: POSIX shared-memory name common to the ranks of this run ("/pion_<launcher pid>"); every rank calls
  // with the same world / periodic_z.  backend: null = libpion_gpu.so.
  slab_comm_shm(int rank, int world, bool periodic_z, const char *name, const pion_backend *backend = nullptr);
  ~slab_comm_shm() override;
  slab_comm_shm(const slab_comm_shm &) = delete;

  int attach(void *handle) override;
  int start(int which) override;
  int finish() override;
  int request_min() override;
  int allreduce_min(double *t_dyn, double *t_mp) override;
  int reset() override;
  // the image relay (slab_comm.h): through segments of its own ("<name>_img<r>": the channel rank r receives in, used
  // by the ranks r - 1 and r only, a message in pieces of at most IMG_PIECE bytes), so that neither a halo exchange in
  // flight nor a pending request_min is disturbed; it needs no attach().  Either rank of a channel creates its segment
  // and both unlink it when they are destroyed: a send or a receive returns only when the peer has mapped it, and a
  // rank whose peer never came (a timeout) leaves nothing behind
  bool has_relay() const override { return true; }
  int recv_from_below(void *host, size_t bytes, int *status) override;
  int send_to_above(const void *host, size_t bytes, int status) override;
  // the same downwards, through segments "<name>_dwn<r>" (the channel rank r receives in, used by r and r + 1)
  bool has_relay_down() const override { return true; }
  int recv_from_above(void *host, size_t bytes, int *status) override;
  int send_to_below(const void *host, size_t bytes, int status) override;
  const std::string &last_error() const override { return err_; }
  int rank() const override { return rank_; }
  int world() const override { return world_; }

 private:
  struct Box;   // one mailbox (header + planes) inside the segment
  Box *box(int rank, int side) const;
  int wait_until(const volatile void *counter, unsigned long long want, const char *what);
  struct Chan;  // one channel of the image relay
  Chan *chan(int down, int rank);
  int relay_send(int down, const void *host, size_t bytes, int status);
  int relay_recv(int down, void *host, size_t bytes, int *status);
  static size_t img_chan_bytes();

  int rank_, world_, up_, down_;
  std::string name_;
  const pion_backend *be_;
  void *h_;
  long count_;                 // doubles per face
  size_t box_bytes_, seg_bytes_;
  char *seg_;                  // the mapped segment
  // the relay's channels [upwards, downwards], mapped at the first receive [.][0] / send [.][1]
  char *img_seg_[2][2] = {{nullptr, nullptr}, {nullptr, nullptr}};
  unsigned long long img_sent_[2] = {0, 0}, img_taken_[2] = {0, 0};   // pieces this rank has written / taken, per direction
  double *stage_lo_, *stage_hi_;   // pinned staging: my bottom / top on-grid planes (out), then the ghosts (in)
  bool pinned_;
  int pending_;                // array of the exchange in flight, or -1
  unsigned long long seq_;     // exchanges completed
  unsigned long long red_seq_; // reductions completed
  bool requested_;
  std::string err_;
};

}  // namespace pion_host
#endif
