// sfm_metres.h -- the one check of a per-scene length in metres that the batch's sensors take (a sense range, a maximum range, a
// radius): finite, positive (strictly or not) and at most SFM_BATCH_MAX_SENSE_RANGE; what the kernels get is its square, formed in
// double and rounded once like thr2 -- and the packing of a grid's row mask into compact slots.  Needs the standard library and include/sfm_hip.h only (a plain host compiler will do).
#pragma once
#include "sfm_hip.h"

#include <cmath>
#include <cstddef>
#include <cstdint>
#include <string>

namespace sfm {

// The reason `r` is refused as scene `scene`'s `name`, or an empty string and r^2 in *sq (sq may be null: the check alone).  strict: 0
// is refused too (-0 counts as 0).
inline std::string check_metres(int scene, const char* name, float r, bool strict, float* sq) {
    if (!std::isfinite(r) || !(strict ? r > 0.f : r >= 0.f) || r > SFM_BATCH_MAX_SENSE_RANGE)
        return "scene " + std::to_string(scene) + ": " + name + " must be finite, " + (strict ? "> 0" : ">= 0") + " and <= 1e6 metres";
    if (sq) *sq = (float)((double)r * (double)r);
    return std::string();
}

// The compact slots of sfm_batch_set_grid: slot[r] = the rank of row r among the masked rows (mask[r] != 0) of all n rows in
// ascending order, -1 for a row that is masked out.  Returns the number of slots.
inline size_t pack_grid_slots(const uint8_t* mask, size_t n, int32_t* slot) {
    size_t m = 0;
    for (size_t r = 0; r < n; ++r) slot[r] = mask[r] ? (int32_t)m++ : -1;
    return m;
}

}  // namespace sfm
