// voxel_cell.h -- the cell of a coordinate, shared by voxel_stage.hip (the hard voxelizer) and dyn_voxel.hip (dynamic
// voxelization): floor((p - lo) / vs) in float32.  `/` is the correctly rounded float32 division (HIP's default
// -fhip-fp32-correctly-rounded-divide-sqrt): a reciprocal multiply would move points that lie on a voxel face into the
// neighbouring cell.
#pragma once
#include "ragged_scene.h"

namespace pda {

// false when the coordinate is NaN or its cell falls outside [0, n).
__device__ __forceinline__ bool cell_axis(float p, float lo, float vs, int32_t n, uint32_t& c) {
    const float f = __builtin_floorf((p - lo) / vs);
    if (is_nan_bits(f) || f < 0.f || f >= (float)n) return false;
    c = (uint32_t)(int)f;
    return true;
}

}  // namespace pda
