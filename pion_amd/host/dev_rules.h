// dev_rules.h -- the rule headers of pion_amd/csrc in host code: the functions the kernels run, compiled for the CPU
// (their __host__ __device__ marks defined away) for the host routes of fits_io.cpp, projection_io.cpp and
// columns_io.cpp, and the grid of a configuration as those functions see it.
#ifndef PION_DEV_RULES_H
#define PION_DEV_RULES_H

#ifndef __host__
#define __host__
#define __device__
#endif
#include "../csrc/dev_output.h"
#include "../csrc/dev_project.h"
#include "../csrc/dev_project_angle.h"
#include "../csrc/dev_raytrace.h"

namespace pion_host {

// pion_gpu_create's GridDesc (defined in fits_io.cpp)
pion::GridDesc grid_desc(const pion_gpu_config &c);

}  // namespace pion_host
#endif
