// norelay_comm.cpp -- TEST INFRASTRUCTURE: a slab communicator (pion_amd/host/slab_comm.h) of `world` ranks that
// exchanges nothing and leaves the image relay at the interface's default ("not supported"), so that
// tests/test_host_projection_ranks.py can reach the refusal of a communicator without send_to_above / recv_from_below.
// Compiled by that test into its temporary directory; never loaded by the product.
#include <string>

#include "../../pion_amd/host/slab_comm.h"

namespace {
class norelay_comm : public pion_host::slab_comm {
 public:
  norelay_comm(int rank, int world) : rank_(rank), world_(world) {}
  int attach(void *) override { return 0; }
  int start(int) override { return 0; }
  int finish() override { return 0; }
  int request_min() override { return 0; }
  int allreduce_min(double *, double *) override { return -1; }   // (no step is taken in the test)
  int reset() override { return 0; }
  const std::string &last_error() const override { return err_; }
  int rank() const override { return rank_; }
  int world() const override { return world_; }

 private:
  int rank_, world_;
  std::string err_;
};
}  // namespace

extern "C" void *norelay_comm_create(int rank, int world)
{
  return static_cast<pion_host::slab_comm *>(new norelay_comm(rank, world));
}
// the interface's defaults, called directly
extern "C" int norelay_comm_recv(void *c, void *host, unsigned long bytes, int *status)
{
  return static_cast<pion_host::slab_comm *>(c)->recv_from_below(host, bytes, status);
}
extern "C" int norelay_comm_send(void *c, const void *host, unsigned long bytes, int status)
{
  return static_cast<pion_host::slab_comm *>(c)->send_to_above(host, bytes, status);
}
