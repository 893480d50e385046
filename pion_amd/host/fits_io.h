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
// under a ".part" name and renamed.  Not read back: a restart reads PIONRAW2.
#ifndef PION_FITS_IO_H
#define PION_FITS_IO_H

#include <string>
#include <vector>

#include "../../include/pion_host.h"

namespace pion_host {

struct snapshot_param;

// the header blocks of the primary HDU for these parameters, and of one image extension: multiples of 2880 bytes
std::string fits_primary_header(const std::vector<snapshot_param> &params);
std::string fits_image_header(const char *extname, int ndim, const long *naxis);

}  // namespace pion_host
#endif
