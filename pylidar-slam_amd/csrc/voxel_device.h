// The voxel rounding of the reference's `voxelise` (slam/common/pointcloud.py:55-62), shared by the grid sample
// (grid_sample.hip) and the aggregated map (aggmap.hip): int(np.round_(p / voxel)), numba promoting f32 / f64 to f64.
#pragma once
#include <hip/hip_runtime.h>

namespace icp {

// the rounded quotient while it is still a double (rint = round half to even): a caller that cannot rule out a coordinate
// beyond int64 tests the range here, before the conversion
template <typename T>
__device__ inline double voxel_coord_real(T v, double voxel) {
    return rint((double)v / voxel);
}

template <typename T>
__device__ inline long long voxel_coord(T v, double voxel) {
    return (long long)voxel_coord_real(v, voxel);
}

}  // namespace icp
