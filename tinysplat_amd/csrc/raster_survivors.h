// raster_survivors.h - the compositing launches with SURVIVOR LISTS (raster.hip), for the frame executor (frame.hip).
// Not part of the C ABI: ts_raster_fwd_sort / ts_raster_bwd_planes are these entries with survivors = NULL.
//
// survivors (int32): survivor_counts(num_tiles) words of counts - word 8 t: the number of entries the forward pass staged
// for tile t; word 8 t + s (s = 1 .. S-1, cut tiles): those in front of list-segment boundary s - then one word per list
// entry (the tile's survivors from its list offset on: (list index - tile start) << 8 | staged block mask).  The
// survivors' Gaussian ids go to bucket_ids, which the forward pass has read by then.  The backward pass must run on the
// lists, records and camera hints the forward pass saw.
#pragma once

#include <cstddef>
#include <cstdint>

#include "../../include/tinysplat_hip.h"

namespace ts_surv {

inline size_t survivor_counts(int num_tiles) { return ((size_t)8 * (size_t)(num_tiles > 0 ? num_tiles : 0) + 63) & ~(size_t)63; }

int raster_fwd_sort(int32_t channels, int32_t flags, const ts_camera* cam, const int32_t* tile_bins,
                    const int32_t* bucket_ids, const float* depths, int32_t* gaussian_ids_sorted,
                    const float* splats, const float* background, float* out_img, float* out_depth,
                    float* final_Ts, int32_t* final_index, uint8_t* clamp_mask, int32_t* survivors, void* stream);

int raster_bwd(int32_t channels, int32_t flags, int64_t num_intersects, const ts_camera* cam,
               const int32_t* tile_bins, const int32_t* gaussian_ids_sorted, const float* splats,
               const float* background, const float* final_Ts, const int32_t* final_index,
               const float* v_out_img, const float* v_out_depth, int32_t planes,
               const float* v_out_alpha, const uint8_t* clamp_mask,
               float* partials, uint8_t* row_flags, const int32_t* bucket_ids, const int32_t* survivors,
               void* stream);

}  // namespace ts_surv
