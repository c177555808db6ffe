// ragged_scene.h -- what every device data stage asks of a batch of ragged scenes (packed rows + (B + 1) int64 offsets +
// n_cap): the two status bits they share, the validated view of one scene, and the size limits of the entry points.
// Included by input_stage.hip, frame_stage.hip, voxel_stage.hip, augment.hip and augment_steps.hip; the bits a stage adds
// (EMPTY / NO_BOX = 1, BAD_DRAW / OVER_BOXES / BAD_CAND = 8, VOXEL_CAP = 16) stay in its file.
#pragma once
#include "pda_common.h"

namespace pda {

// info[b][3] status bits (include/pda_train.h)
constexpr int ST_BAD_OFFSETS = 2, ST_OVER_CAP = 4;

struct Scene {
    int64_t start;
    int n;       // raw points this scene holds (0 when its offsets are unusable)
    int status;  // ST_BAD_OFFSETS / ST_OVER_CAP
};

__device__ __forceinline__ Scene scene_of(const int64_t* __restrict__ off, int b, int64_t n_total, int64_t n_cap) {
    const int64_t s = off[b], e = off[b + 1];
    Scene r{0, 0, 0};
    if (s < 0 || e < s || e > n_total) r.status = ST_BAD_OFFSETS;
    else if (e - s > n_cap) r.status = ST_OVER_CAP;
    else { r.start = s; r.n = (int)(e - s); }
    return r;
}

__device__ __forceinline__ bool offsets_ok(const int64_t* off, int b, int64_t total) {
    const int64_t s = off[b], e = off[b + 1];
    return s >= 0 && e >= s && e <= total;
}

// host side: the batch and n_cap every stage entry accepts (grid.y = batch; tiles of n_cap fit an int)
inline bool stage_sizes_ok(int batch, int64_t n_cap) { return batch >= 0 && batch <= 65535 && n_cap >= 1 && n_cap <= (1 << 30); }

}  // namespace pda
