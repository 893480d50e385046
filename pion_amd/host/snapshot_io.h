// snapshot_io.h -- the snapshot file of the C++ host loop, format "PIONRAW2", written and read without Python.
//
// Stands where the reference has dataIO/ (dataio_base.cpp:60-440 is its registry of header parameters; the Silo /
// FITS / text writers are not reproduced): enough to leave the state of a run on disk and restart from it bit for
// bit.  The file has three parts:
//   1. the 8-byte magic "PIONRAW2";
//   2. a text header of "name value" lines, the way the reference's parameter files and its text writer spell them.
//      The names are the reference's wherever it has one (snapshot_header_keys()); what it has no name for carries a
//      pion_ prefix.  NGrid, Ncell, Xmin, Xmax and BC_XN .. BC_ZP describe the GLOBAL problem -- the faces a rank
//      shares with a neighbour are not a property of the problem --, pion_slab_lo / pion_slab_n say which planes of
//      the slab axis (the last axis) this file holds.  Doubles are printed with %.17g and read back bit for bit.  The
//      last line is "pion_data_offset N"; newlines pad the header up to byte N.
//   3. from byte N, fp64 little-endian, ON-GRID cells only: [nvar][slab_n][ny][nx] (2-D: [nvar][slab_n][nx]; 1-D:
//      [nvar][nx]) in code units (no sqrt(4 pi) rescaling of B, cf. dataio_silo.cpp:1468-1492).  Ghost cells are not
//      stored: the restart refills them with a boundary assignment, exactly as the reference's does.
//
// The data leave and enter the device a chunk of whole planes at a time through the backend's ongrid_* entries
// (pion_backend.h): a chunk is the largest number of planes that fits 64 MiB (at least one; PION_SNAPSHOT_CHUNK_PLANES
// in the environment forces it, for tests), the backend packs and copies chunk i+1 while this code pwrite()s chunk i,
// one run per variable at its file offset; the read path mirrors it.  A backend without those entries (the test
// oracle's table) goes through its whole-array download / upload, ghosts stripped / embedded here.
//
// The members sim_control_gpu::write_snapshot / read_snapshot are defined in snapshot_io.cpp, and with them what the
// other writers (fits_io.cpp, projection_io.cpp, columns_io.cpp) and the FITS reader share: how a writer opens
// (path_refused, writer_params with the list of parameters, snapshot_params), the streamed write loop (stream_jobs; its
// chunk-major caller stream_runs; the size of a chunk, chunk_planes), the checks of a header (snapshot_header_from_kv)
// and the whole restart but the meaning of a file element (read_files).  The file a writer writes into: out_file.h.
#ifndef PION_SNAPSHOT_IO_H
#define PION_SNAPSHOT_IO_H

#include <sys/types.h>

#include <map>
#include <string>
#include <vector>

#include "../../include/pion_host.h"

namespace pion_host {

// constants::equalD (constants.cpp:48-70): equal, both tiny (< 1e-100), or relative difference < 1e-12
bool equalD(double a, double b);

struct snapshot_header {
  pion_gpu_config cfg;             // the global problem
  pion_host_snapshot_info info;
  std::map<std::string, std::string> kv;   // every line of the header
};

// returns 0 or PION_GPU_EINVAL with a text in err; never throws
int snapshot_read_header(const char *path, snapshot_header &hd, std::string &err);
// hd.kv -> hd.cfg and hd.info with every check of a header, for both file types (the FITS reader of fits_io.h fills
// hd.kv from the cards of the primary header); header_end: the byte the header's text ends at (pion_data_offset must
// not lie before it)
int snapshot_header_from_kv(const char *path, snapshot_header &hd, long header_end, std::string &err);
// the header names every file carries, in file order
const std::vector<std::string> &snapshot_header_keys();

// one parameter of a file as sim_control_gpu::snapshot_params lists it: the PIONRAW2 line is "key value"; type 'i'
// (integers), 'd' (doubles, %.17g) or 's' (a string); an array is its elements separated by one blank
struct snapshot_param {
  std::string key, value;
  char type;
};

// planes per chunk of a streamed file: the largest number that fits one 64 MiB staging slot, at least one and at most
// `planes`; PION_SNAPSHOT_CHUNK_PLANES in the environment forces it
long chunk_planes(long doubles_per_plane_all_runs, long planes);

}  // namespace pion_host
#endif
