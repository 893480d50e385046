// fits_io.h -- the FITS file of the C++ host loop (sim_control_gpu::write_fits, defined in fits_io.cpp), written
// without CFITSIO after the model of the reference's dataio_fits::OutputData (dataIO/dataio_fits.cpp:147-320).
//
// Layout (FITS standard 4.0): 2880-byte blocks; headers are 80-character ASCII cards, blank-padded, ending with END.
//   1. Primary HDU without data: SIMPLE = T, BITPIX = -64, NAXIS = 0, EXTEND = T, then the simulation parameters.
//      Every key of the PIONRAW2 header (snapshot_header_keys(); the list itself is sim_control_gpu::snapshot_params,
//      used by both writers) except pion_data_offset becomes a card "HIERARCH <name> = <value>" under the same name
//      and case; arrays get element-numbered names as the reference's write_header_param gives them (NGrid0..2,
//      Xmin0..2, Xmax0..2, Ref_Vector0..).  Doubles are printed with %.17G and read back bit for bit; strings are
//      quoted, one longer than a card continues on CONTINUE cards (standard 4.0, s4.2.1.2).  As in PIONRAW2, NGrid,
//      Xmin, Xmax and BC_* describe the GLOBAL problem; pion_slab_lo / pion_slab_n say which planes the file holds.
//   2. One IMAGE extension per image of dev_output.h's list, in its order: XTENSION = 'IMAGE   ', BITPIX = -64,
//      NAXIS = ndim, NAXIS1 = nx (x fastest), NAXIS2, NAXIS3 (the rank's own extent), PCOUNT = 0, GCOUNT = 1, EXTNAME;
//      then the big-endian doubles of the on-grid cells, zero-padded to a multiple of 2880 bytes.  Bx, By, Bz and divB
//      carry the reference's sqrt(4 pi) (NEW_B_NORM); psi and Ptot do not.
//
// The images leave the device already in file byte order through the backend's fits_* entries (pion_backend.h), a
// chunk of whole planes at a time through the PIONRAW2 writer's loop (stream_runs): host memory is two chunks.  A
// backend without those entries (the test oracle's table) downloads array 0 whole and evaluates the same
// dev_output.h functions in a host loop.  Every rank writes its own file; nothing is collective.  The file is written
// under a ".part" name and renamed (out_file.h).
//
// Read back (sim_control_gpu::read_fits, the reference's DataIOFits::ReadHeader / ReadData / read_fits_image,
// dataio_fits.cpp:340-385, 433-548, 865-929), again without CFITSIO.  The reader walks 2880-byte blocks and
// 80-character cards up to END and understands SIMPLE, XTENSION, BITPIX, NAXIS, NAXISn, PCOUNT, GCOUNT, EXTNAME,
// "HIERARCH <name> = <value>" cards, quoted strings with doubled quotes and CONTINUE cards, integers, and doubles as
// %.17G prints them.  Every data unit is sized from its own header, |BITPIX|/8 * GCOUNT * (PCOUNT + prod NAXISn) padded
// to 2880, so HDUs the restart does not need are skipped whatever they are; cards it does not know are skipped too.
// The nvar primitive images of dev_output.h's list are found by EXTNAME, not by position; the derived images are
// never read.  A needed image must have BITPIX = -64 and the extents the primary header implies.  A primitive image
// the file does not hold is zeros, as in the reference (:505-512).  A primary header without pion_slab_lo /
// pion_slab_n describes a file that holds the whole slab axis.  The key/value list of the primary header becomes the
// configuration through the PIONRAW2 reader's own function (snapshot_header_from_kv): one set of checks.
//
// The elements enter the device as the file holds them, a chunk of planes at a time through the backend's
// fits_from_host (the PIONRAW2 reader's loop: sim_control_gpu::read_files, host memory two chunks); k_unpack_fits swaps
// them, multiplies B by 1/sqrt(4 pi) and counts the elements that are not finite or hold the reference's null value
// -1e99, which fail the restart.  A backend without that entry takes the same dev_output.h functions in a host loop
// (fits_convert_run) and goes through upload.
//
// The other files of this format -- projected images (projection_io.cpp) and ray-traced column densities
// (columns_io.cpp) -- have the same shape: one primary header, N image headers of one length and N data units of one
// length.  fits_layout states where each lies and starts a file of that shape.
#ifndef PION_FITS_IO_H
#define PION_FITS_IO_H

#include <string>
#include <vector>

#include "../../include/pion_host.h"
#include "out_file.h"
#include "snapshot_io.h"

namespace pion_host {

// the header blocks of the primary HDU for these parameters, and of one image extension: multiples of 2880 bytes
std::string fits_primary_header(const std::vector<snapshot_param> &params);
std::string fits_image_header(const char *extname, int ndim, const long *naxis);

// A file of one primary header and ext.size() image extensions, each with run_bytes of data zero-padded to a multiple
// of 2880: where the pieces lie.  Every extension header must have the same length (fits_image_header gives that for
// one ndim): the one stride from image to image rests on it, and the constructor checks it
struct fits_layout {
  fits_layout(const std::string &primary, const std::vector<std::string> &ext, long run_bytes);
  long header_at(long i) const { return (long)primary.size() + i * stride; }
  long data_at(long i) const { return header_at(i) + (stride - data_padded); }
  // The file at its full length first -- what no write covers, the padding after each data unit, reads as zero bytes
  // --, then every header.  The data follow.  0 or PION_GPU_EINVAL, as PartFile::write
  int start(PartFile &f) const;
  const std::string &primary;
  const std::vector<std::string> &ext;
  const long data_padded, stride, total;   // stride: from one image's header (or data) to the next one's
};

// Header of a FITS file of this writer's kind: hd as snapshot_read_header fills it (info.data_offset = 0).  image_off
// (may be null): per primitive variable, the byte its image's data unit starts at, or -1 where the file has no image
// of that name -- then note (may be null) gains a sentence that says so.  EINVAL and a text in err: not a FITS file, a
// header without END, a data unit that runs past the end of the file, a missing or malformed key, a needed image with
// BITPIX other than -64 or with other extents than the header's.  Never throws.
int fits_read_header(const char *path, snapshot_header &hd, std::vector<long> *image_off, std::string *note,
                     std::string &err);
// the n file elements (big-endian doubles) of variable `var` in place to what the state holds (dev_output.h's
// in_be64 / in_value: what k_unpack_fits does); returns how many of them in_rejected holds for
long fits_convert_run(const pion_gpu_config &cfg, int var, double *run, size_t n);

}  // namespace pion_host
#endif
