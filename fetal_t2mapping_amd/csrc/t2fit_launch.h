// t2fit_launch.h -- how the host seam (t2fit_host.hip) reaches the fit (t2fit_kernels.hip): host-only declarations, no
// device code and none of the lane headers.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/t2fit.h"

namespace t2fit {

// What the voxel seam has a fit write beside the maps, all on the device.  (The kernels' own record of their outputs,
// DevMaps, stays inside t2fit_kernels.hip: its name is spelled in every fit kernel's symbol.)
struct VoxelOutputs {
  double* xd = nullptr;          // float64 parameters, 3 per voxel
  double* fund = nullptr;        // float64 objective value
  double* trace = nullptr;       // trace kernels only: [n_vox][trace_cap][4] doubles (k, T2, sigma, f)
  int32_t* trace_len = nullptr;  //                     iterations recorded per voxel
  int trace_cap = 0;
};

// the argument checks every entry point that takes a stack shares; records the error and returns its code
int check_common(const t2fit_config* cfg, const void* echoes, int layout, int64_t n_vox);

// above the size (T2FIT_SMALL_VOLUME) up to which a volume runs the generic small-chunk kernels
bool is_large_volume(int64_t n_vox);

// Queues the fit of n_vox voxels on `st`; `maps` holds device pointers.  part_of_large: this call fits one slab of a
// large volume (the host seam): the large-volume kernels whatever its size.
int launch_fit(const t2fit_config* cfg, const float* echoes, int layout, const uint8_t* mask, int64_t n_vox,
               const t2fit_maps& maps, hipStream_t st, bool part_of_large = false, const VoxelOutputs& vox = {});

}  // namespace t2fit
