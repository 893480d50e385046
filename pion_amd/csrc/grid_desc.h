// grid_desc.h -- the grid as every kernel sees it.  Includes nothing, so that host-only builds (tests/native) can use
// it without the device headers.
#ifndef PION_GRID_DESC_H
#define PION_GRID_DESC_H

namespace pion {

struct GridDesc {
  int ndim;
  int ng[3], nbc[3], nga[3];
  long ncell;   // cells incl. ghosts
  long sy, sz;  // strides of y and z in cells
  double dx;
  double xmin[3];
  int cyl;      // 1: cylindrical (z,R) axisymmetry, axis 1 = R (2-D only); 2: spherical symmetry, axis 0 = R (1-D)
  const double *sph_vol;  // spherical: (rp^3 - rn^3)/3 per all-cell x index, evaluated on the host (libm pow)
};

}  // namespace pion
#endif
