/*
 * tinysplat_hip.h - C ABI of libtinysplat_hip.so (HIP, gfx950 / MI355X).
 *
 * This is the drop-in boundary below tinysplat's render adapter.  tinysplat reaches its rasterizer
 * through three Python callables imported from the third-party gsplat package
 * (/root/reference/tinysplat/splatting/rasterize.py:3-4):
 *
 *     project_gaussians(...)      rasterize.py:32   (13 positional args built at rasterize.py:64-73)
 *     spherical_harmonics(...)    rasterize.py:38   (3 args built at rasterize.py:75-81)
 *     rasterize_gaussians(...)    rasterize.py:44,50 (10 args built at rasterize.py:83-86)
 *
 * gsplat binds those callables to a C++/CUDA extension; the entry points below are what a binding
 * for the same three callables (forward and backward) binds on MI355X.  Each group is labelled with
 * the callable it implements.  tinysplat_amd/_lib.py is the ctypes binding, tinysplat_amd/ops.py the
 * torch.autograd.Function layer that restores the exact Python signatures.
 *
 * Conventions
 *   - every pointer is a DEVICE pointer unless its name ends in _host;
 *   - all arrays are dense, row-major, float32 / int32 / uint64 as typed;
 *   - `stream` is a hipStream_t passed as void*; every entry only enqueues work on it, never
 *     synchronises, never allocates, never frees; workspaces are caller-provided;
 *   - return value: 0 on success, a negative TS_E_* code for an argument error, otherwise the
 *     positive hipError_t of the failed launch;
 *   - tile = 16x16 pixels (rasterize.py:19-20).  `tile_row0/tile_rows` select a stripe of tile rows
 *     [tile_row0, tile_row0 + tile_rows) for multi-GPU tile-stripe sharding; a single GPU passes
 *     (0, tile_bounds_y).  Pixel coordinates stay global; image buffers hold only the stripe's rows.
 */
#ifndef TINYSPLAT_HIP_H
#define TINYSPLAT_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define TS_ABI_VERSION 9

#define TS_E_BADARG (-1)  /* null pointer / negative size / unsupported channel count */
#define TS_E_DEGREE (-2)  /* SH degree out of range or exceeds stored coefficients */

#define TS_TILE 16
#define TS_SPLAT_RECORD_FLOATS 12   /* packed per-Gaussian record, see ts_pack_splats */
#define TS_PARTIAL_ROW_FLOATS 12    /* per-(tile,Gaussian) gradient row, see ts_raster_bwd */

int ts_abi_version(void);

/* ---- camera block ---------------------------------------------------------------------------
 * Scalars of rasterize.py:64-73 (fx, fy, cx, cy, img_height, img_width, tile_bounds, glob_scale)
 * plus the near-plane threshold of gsplat's project_gaussians (clip_thresh, default 0.01). */
typedef struct ts_camera {
    float fx, fy, cx, cy;
    int32_t img_width, img_height;
    int32_t tile_bounds_x, tile_bounds_y;
    int32_t tile_row0, tile_rows;
    float glob_scale;
    float clip_thresh;
    /* Tile shape of the LISTS only (binning, sorting): 0 = gsplat's 16x16 tiles; 1 = wide 32x16 tiles, each the
     * union of two horizontally adjacent 16x16 tiles (column pairs 2j, 2j+1; the last one may be a single
     * column).  Compositing always runs one wave per 16x16 tile: with wide lists ts_raster_fwd / _fwd_planes /
     * _bwd / _bwd_planes need TS_RASTER_NARROW_WAVES (TS_E_BADARG without it).  Projection, num_tiles_hit /
     * cum_tiles_hit and tile_row0 / tile_rows always count 16x16 tiles; images and gradients do not depend on the
     * shape (a Gaussian is composited only into the 16x16 tiles of its tile box either way), only the number of
     * list entries does. */
    int32_t wide_tiles;
    /* bits 0..7: performance hints (formerly `reserved`, 0 = none); results never depend on them.
     * TS_HINT_BALANCED_WALK: a Gaussian covers many tiles (>= ~10 bounding-box tiles on average): ts_bin_scatter
     * expands (Gaussian, tile row) items over the lanes instead of looping per Gaussian.
     * bits 8..11: LIST SEGMENTS S of the compositing passes (TS_CAM_LIST_SEGMENTS(S), 0 / 1 = off, S <= 8; 16x16
     * lists only).  The backward pass of a tile is a chain over its sorted list; with S > 1 ts_raster_fwd* additionally
     * stores, for every CUT tile, the per-pixel state at up to S - 1 boundaries of its list (lists of >= 65 entries)
     * behind final_Ts - which must then hold ts_final_floats(cam, channels) floats - and ts_raster_bwd* WITHOUT
     * TS_RASTER_SPLIT_BLOCKS replays a cut tile's list as up to S independent one-wave work items (one row per pair,
     * the plain ts_reduce_partials).  Same image; gradients equal to the uncut pass's up to rounding (a segment
     * starts from the forward pass's own transmittance).  Both passes must see the same S and W16.  With
     * TS_RASTER_SPLIT_BLOCKS or wide lists ts_raster_bwd* ignores the field.
     * bits 12..15: W16 (TS_CAM_WHOLE_TILES(W16), 0..15) - which tiles are cut: 0 = all of them (launches of fewer
     * tiles than the GPU has SIMDs: instead of TS_RASTER_SPLIT_BLOCKS in the backward pass); 1..15 = a HYBRID
     * launch for full frames: the tiles are handed out in eight bands (one per XCD) and the first W16/16 of every
     * band stay whole, only the tiles dispatched last are cut, so that their small work items fill the wave slots
     * the whole tiles leave behind at the end of the launch (ts_cut_tiles tells which).
     * bits 16..19: C16 (TS_CAM_COOP_TILES(C16), 0..15; a pure performance hint of ts_raster_fwd*, one wave per 16x16
     * tile on 16x16 lists) - COOPERATIVE TILES: the first C16/16 of every band, which the forward launch hands out
     * last, are composited by a workgroup of four waves each (shared staging and sort, one 8x8 block per wave), so
     * that the forward launch's tail is filled with items a quarter as long.  Never a cut tile (C16 is capped by
     * W16; with S > 1 and W16 = 0 it is ignored).  Image, final_Ts, final_index: bit for bit the same.
     * TS_HINT_COOP_SPLIT (bit 20; a pure performance hint of ts_raster_fwd*): a launch that asks for
     * TS_RASTER_SPLIT_BLOCKS on 16x16 lists composites every tile as a cooperative workgroup instead - four waves per
     * tile as the split mapping has, but each list is staged and sorted ONCE by the four of them instead of walked by
     * each.  With S > 1 the boundary records are the ones the split launch would leave (W16 = 0: every tile; W16 > 0:
     * the cut tiles are the cooperative ones and the others one wave each).  Same bits in every output. */
    int32_t hints;
} ts_camera;
#define TS_HINT_BALANCED_WALK 1
#define TS_HINT_COOP_SPLIT (1 << 20)
#define TS_CAM_LIST_SEGMENTS(s) (((s) & 15) << 8)
#define TS_CAM_WHOLE_TILES(w16) (((w16) & 15) << 12)
#define TS_CAM_COOP_TILES(c16) (((c16) & 15) << 16)
/* floats final_Ts must hold: the rows*W transmittances, then (S > 1, 16x16 lists) one checkpoint block of
 * S records of (1+channels) 256 floats per cut tile, from a 64-float aligned offset; < 0: bad argument */
int64_t ts_final_floats(const ts_camera* cam_host, int32_t channels);
/* -> number of checkpoint blocks (>= cut tiles) of a launch under cam's S / W16; *band = tiles per band (tile t lies
 * in band t / band), *whole = the first `whole` tiles of every band are composited whole (either may be NULL) */
int32_t ts_cut_tiles(const ts_camera* cam_host, int32_t* band, int32_t* whole);
/* tiles (= lists) of a launch: tile_rows * tile_bounds_x, or tile_rows * ceil(tile_bounds_x / 2) when wide */
int32_t ts_num_tiles(const ts_camera* cam_host);

/* ============================ project_gaussians (rasterize.py:32) ============================ */

/* flags: fold the adapter's argument preparation (rasterize.py:72-73) into the kernels */
#define TS_PROJECT_LOG_SCALES 1  /* `scales` holds log-scales: the kernel uses exp(scales)          */
#define TS_PROJECT_RAW_QUATS 2   /* `quats` is unnormalised: the kernel uses quats / |quats|;        */
                                 /* backward then returns gradients w.r.t. the raw tensors           */

/* Forward.  viewmat: 12 floats (rows of the 3x4 view matrix, rasterize.py:73 passes
 * view_matrix[:3,:]); projmat: 16 floats (P @ V).  Outputs are fully written for every Gaussian;
 * culled ones (z <= clip, singular cov2d, no tile hit) get zeros.  cov3d may be NULL (the adapter
 * discards it, rasterize.py:32; the forward-only viewer path, viewer.py:89-93, passes NULL). */
int ts_project_fwd(int32_t n, const float* means3d, const float* scales, const float* quats,
                   const float* viewmat, const float* projmat, const ts_camera* cam_host,
                   int32_t flags, float* xys, float* depths, int32_t* radii, float* conics,
                   int32_t* num_tiles_hit, float* cov3d, void* stream);

/* Backward.  v_conic uses the true-partial convention for the off-diagonal entry.  v_cov3d may be
 * NULL (tinysplat discards cov3d, rasterize.py:32); v_depth may be NULL (no gradient reaches depths).  Gaussians with radii == 0 receive zeros. */
int ts_project_bwd(int32_t n, const float* means3d, const float* scales, const float* quats,
                   const float* viewmat, const float* projmat, const ts_camera* cam_host,
                   int32_t flags, const int32_t* radii, const float* v_xy, const float* v_depth,
                   const float* v_conic, const float* v_cov3d,
                   float* v_means3d, float* v_scales, float* v_quats, void* stream);

/* ========================= gsplat.sh.spherical_harmonics (rasterize.py:38) ==================== */

/* colors[n,3] = sum over bands <= degrees_to_use of Y_k(normalize(viewdirs)) * coeffs[n,k,:].
 * num_bases = K of the stored coefficients (1,4,9,16,25). */
int ts_sh_fwd(int32_t n, int32_t degrees_to_use, int32_t num_bases, const float* viewdirs,
              const float* coeffs, float* colors, void* stream);

/* v_coeffs[n,K,3]: Y_k * v_colors for active bands, zero for inactive ones (fully written). */
int ts_sh_bwd(int32_t n, int32_t degrees_to_use, int32_t num_bases, const float* viewdirs,
              const float* v_colors, float* v_coeffs, void* stream);

/* Fused colour stage of the render adapter = rasterize.py:75-81 (view directions
 * normalize(means - origin), origin = view_matrix[:3,3]; coefficients given as the two parameter
 * tensors colors_dc[n,3] and colors_rest[n,K-1,3] instead of their torch.cat) + rasterize.py:38-39
 * (SH evaluation, clamp(rgb + 0.5, min=0)).  clamp_mask[n]: bit c set where channel c passes
 * gradient (NULL in forward-only use).  origin: 3 device floats.  colors_rest may be NULL when
 * num_bases == 1. */
int ts_sh_colors_fwd(int32_t n, int32_t degrees_to_use, int32_t num_bases, const float* means3d,
                     const float* origin, const float* colors_dc, const float* colors_rest,
                     float* colors, uint8_t* clamp_mask, const int32_t* live, void* stream);
/* live: NULL, or num_tiles_hit of a tile-row stripe - only Gaussians with live[i] != 0 are evaluated (each
 * reads its own coefficient row) and the colours / masks of the others are left unwritten: the colour stage
 * of one rank of a multi-GPU frame touches the 1/G of the Gaussians that its stripe lists.
 * ts_sh_colors_bwd: clamp_mask may be NULL (all channels pass) when the mask was already applied by
 * ts_reduce_partials(color_mask) - the multi-GPU order, where the 2-D gradients are summed over ranks
 * between the two and a rank holds masks for its own stripe's Gaussians only. */
int ts_sh_colors_bwd(int32_t n, int32_t degrees_to_use, int32_t num_bases, const float* means3d,
                     const float* origin, const uint8_t* clamp_mask, const float* v_colors,
                     float* v_colors_dc, float* v_colors_rest, void* stream);
/* ts_sh_colors_fwd + ts_pack_splats in one launch for the RGB / RGB + depth frame: the colour stage
 * writes the packed record of every listed Gaussian itself (arguments as for ts_pack_splats; the colours
 * stay in registers, no colors[n,3] array exists).  channels == 4 takes channel 3 from depths[]. */
int ts_colors_pack_fwd(int32_t n, int32_t degrees_to_use, int32_t num_bases, const float* means3d,
                       const float* origin, const float* colors_dc, const float* colors_rest,
                       uint8_t* clamp_mask, const int32_t* live, int32_t channels, int32_t flags,
                       const float* xys, const int32_t* radii, const float* conics, const float* opacity,
                       const int32_t* cum_tiles_hit, const ts_camera* cam_host, const float* depths,
                       float* splats, void* stream);
/* The same launch, which also leaves one 16-byte SPAN RECORD per Gaussian in row_spans (4 n int32 words, 16-byte
 * aligned; layout in csrc/row_spans.h): the 16x16 tile columns [lo, hi) of every tile row of its box in this camera's
 * stripe, as ts::TightTest::row_range leaves them (tight != 0) or the bounding box's (tight = 0) - what the list build
 * would compute from xys, radii and the record.  Every Gaussian gets one: the empty record where nothing is listed
 * (culled, outside the stripe, live[i] == 0), a "not representable" mark beyond six rows or 256 columns.  The records
 * are computed while the coefficient loads are in flight.  row_spans = NULL: ts_colors_pack_fwd. */
int ts_colors_pack_spans_fwd(int32_t n, int32_t degrees_to_use, int32_t num_bases, const float* means3d,
                             const float* origin, const float* colors_dc, const float* colors_rest,
                             uint8_t* clamp_mask, const int32_t* live, int32_t channels, int32_t flags,
                             const float* xys, const int32_t* radii, const float* conics, const float* opacity,
                             const int32_t* cum_tiles_hit, const ts_camera* cam_host, const float* depths,
                             float* splats, int32_t tight, int32_t* row_spans, void* stream);

/* ========================= rasterize_gaussians (rasterize.py:44,50) =========================== */
/* Stage order: ts_scan_tiles -> (read total) -> ts_bin_count -> ts_tile_offsets -> ts_bin_scatter
 * -> ts_sort_tiles -> ts_pack_splats -> ts_raster_fwd ; backward: ts_raster_bwd -> ts_reduce_partials */

/* Inclusive int32 prefix sum of num_tiles_hit -> cum_tiles_hit[n]; the grand total (number of
 * tile/Gaussian intersections I) is cum_tiles_hit[n-1].  scan_ws: >= ts_scan_ws_ints(n) int32.
 * total_out: NULL, or a DEVICE-VISIBLE address (the device pointer of mapped pinned host memory, see
 * hipHostGetDevicePointer) that receives the grand total with a system-scope store from the scan itself:
 * the host can poll it there instead of queueing a 4-byte copy behind the scan. */
int64_t ts_scan_ws_ints(int32_t n);
int ts_scan_tiles(int32_t n, const int32_t* num_tiles_hit, int32_t* cum_tiles_hit,
                  int32_t* scan_ws, int32_t* total_out, void* stream);

/* Tile bucketing without global atomics.  The Gaussians are cut into B = ts_bin_chunks(n) contiguous
 * chunks; bin_ws (>= ts_bin_ws_ints(n, num_tiles) int32, num_tiles = tile_rows * tile_bounds_x) holds
 * the B x num_tiles count matrix, num_tiles + 1 tile starts and one spare word.  Stripe-local tile index
 * t = (ty - tile_row0) * tile_bounds_x + tx. */
int64_t ts_bin_ws_ints(int32_t n, int32_t num_tiles);

/* bin_ws[b][t] = number of Gaussians of chunk b whose tile rectangle covers tile t (LDS histograms).
 * splats: NULL -> gsplat's bounding-box lists (what the bit-exact binning checks compare).
 * Non-NULL (the packed records of ts_pack_splats) -> TIGHT lists: a (Gaussian, tile) pair is dropped
 * when the record proves that no pixel of the tile can reach alpha >= 1/255; such pairs contribute
 * exactly nothing, so image and gradients are bit-identical while ~1/3 of the pairs never reach the
 * scatter, the sort and the compositing kernels.  ts_bin_scatter must be given the same pointer.
 * Buffers stay sized by the bounding-box total I = cum_tiles_hit[n-1]. */
int ts_bin_count(int32_t n, const float* xys, const int32_t* radii, const float* splats,
                 const ts_camera* cam_host, int32_t* bin_ws, void* stream);

/* Turns the counts into bases in place (exclusive scan down the chunk axis, then over tiles) and
 * writes tile_bins[t] = {start, end} (both 0 for an empty tile).
 * Capacity guard (cum_tiles_hit non-NULL and capacity >= 0): a caller that sized bucket_ids / gaussian_ids_sorted /
 * partials from an ESTIMATE instead of waiting for the count passes that size; if the frame's total
 * cum_tiles_hit[n-1] exceeds it, every list is left empty and ts_bin_scatter returns without writing, so nothing
 * is touched beyond the buffers - the caller reads the count later, sees the same excess and repeats the frame
 * with exact sizes.  NULL / -1: no guard. */
int ts_tile_offsets(int32_t n, int32_t num_tiles, int32_t* bin_ws, int32_t* tile_bins,
                    const int32_t* cum_tiles_hit, int64_t capacity, void* stream);
/* ... and the length of the frame's LONGEST list stored to *longest_list (device-visible memory - e.g. the word behind
 * the caller's mapped pinned count word; NULL: ts_tile_offsets): a scene statistic for the caller's launch policy
 * (frame.py: list shape and hybrid shares), read a frame later, never waited for. */
int ts_tile_offsets_stats(int32_t n, int32_t num_tiles, int32_t* bin_ws, int32_t* tile_bins,
                          const int32_t* cum_tiles_hit, int64_t capacity, int32_t* longest_list, void* stream);

/* Writes the id of every Gaussian into the bucket of each tile its rectangle covers (bucket_ids[I];
 * order inside a bucket is arbitrary until ts_sort_tiles).  scratch: NULL, or I more int32 (the
 * gaussian_ids_sorted buffer may be passed: it is dead until ts_sort_tiles) - the ids then reach their buckets in
 * two coalesced hops (tile group, then tile) instead of one 4-byte store per cache line; same buckets. */
int ts_bin_scatter(int32_t n, const float* xys, const int32_t* radii, const float* splats,
                   const ts_camera* cam_host, const int32_t* bin_ws, int32_t* bucket_ids, int32_t* scratch,
                   void* stream);

/* Sorts every tile bucket ascending by (depth bits, gaussian id) - i.e. the order of a stable sort
 * of (tile<<32 | depth-bits) keys emitted Gaussian-major - reading bucket_ids[I] and depths[n] and
 * writing gaussian_ids_sorted[I] (a different buffer).  sort_ws: >= num_tiles + 1 int32 of scratch
 * (bin_ws may be passed: its contents are dead once ts_bin_scatter has run). */
int ts_sort_tiles(int32_t num_tiles, const int32_t* tile_bins, const float* depths,
                  const int32_t* bucket_ids, int32_t* gaussian_ids_sorted, int32_t* sort_ws,
                  int32_t* zeroed_counter, void* stream);
/* ABI 5: ts_sort_tiles for the tiles of MORE than 1024 entries only - the companion of ts_raster_fwd_sort, which
 * sorts the shorter lists itself (one wave per tile) right before it composites them. */
int ts_sort_tiles_above(int32_t num_tiles, const int32_t* tile_bins, const float* depths,
                        const int32_t* bucket_ids, int32_t* gaussian_ids_sorted, int32_t* sort_ws,
                        int32_t* zeroed_counter, void* stream);
/* sort_ws, zeroed_counter: DEPRECATED and ignored (pass NULL) - every tile has its own workgroup now, there is
 * no queue of oversized tiles.  ts_sort_tiles still uses them (its zeroed_counter: NULL, or a device word
 * known to be zero; ts_tile_offsets zeroes bin_ws[ts_bin_ws_ints(n, num_tiles) - 1] for this purpose). */

/* GROUP FORM of ts_bin_count -> ts_tile_offsets_stats -> ts_bin_scatter (additive entries, ABI 8).  A frame whose
 * scatter runs in two hops - ts_bin_group_form(n) != 0: n >= 2^18 and n < 2^27, scratch given - needs a base per
 * (chunk, GROUP of 32 consecutive lists) for its coarse hop only, and the fine hop counts the lists of its group from
 * the region it streams anyway.  bin_ws (same size, ts_bin_ws_ints) then holds a B x G count matrix instead of the
 * B x T one; the tile starts, the guard word and the spare word stay where they are, with the same meaning.
 *   ts_bin_count_groups    bin_ws[b][g] = pairs of chunk b in the lists of group g (same decisions as ts_bin_count)
 *   ts_group_offsets       bases in place, the start of every group's region, the grand total (tile_start[T]), the
 *                          capacity guard and the zeroed spare word; tile_bins is written here ONLY when the guard trips
 *                          or nothing at all is listed (all lists empty; *longest_list = 0 in the latter case)
 *   ts_bin_scatter_groups  both hops; the fine hop writes tile_bins and the remaining tile starts.  scratch as for
 *                          ts_bin_scatter, not NULL
 *   ts_sort_tiles_stats / ts_sort_tiles_above_stats
 *                          ts_sort_tiles / ts_sort_tiles_above; with longest_list != NULL they also store the length of
 *                          the frame's longest list there (what ts_tile_offsets_stats stores in the matrix form; n and
 *                          bin_ws are those of ts_bin_scatter_groups, which left one maximum per group in bin_ws).
 *                          longest_list == NULL: n and bin_ws are ignored
 * All of them return TS_E_BADARG for an n the group form does not apply to.  The three stages of a frame must be taken
 * from the same form (the frame executor decides it in one place: list_form, csrc/frame.hip).  The fine hop is the same
 * code in every form; the layout of bin_ws in all of them is described once, at BinGeometry in csrc/binning.hip. */
int32_t ts_bin_group_form(int32_t n);
int ts_bin_count_groups(int32_t n, const float* xys, const int32_t* radii, const float* splats,
                        const ts_camera* cam_host, int32_t* bin_ws, void* stream);
int ts_group_offsets(int32_t n, int32_t num_tiles, int32_t* bin_ws, int32_t* tile_bins,
                     const int32_t* cum_tiles_hit, int64_t capacity, int32_t* longest_list, void* stream);
int ts_bin_scatter_groups(int32_t n, const float* xys, const int32_t* radii, const float* splats,
                          const ts_camera* cam_host, int32_t* bin_ws, int32_t* tile_bins, int32_t* bucket_ids,
                          int32_t* scratch, void* stream);
/* ONE WALK form of the same three stages (additive entries, ABI 8): the Gaussians are walked once.  Every chunk writes
 * its entries, ordered by group, into its own part of scratch - it starts at cum_tiles_hit[first Gaussian - 1], and a
 * chunk lists at most its bounding-box slots - and leaves its counts and run starts per group in bin_ws; the fine hop
 * gathers a group's runs.  Applies where ts_bin_one_walk_form(n, num_tiles) != 0 (a group-form n whose groups fit the
 * emit launch: num_tiles <= 65536 and not a handful) and the camera carries no TS_HINT_BALANCED_WALK; TS_E_BADARG,
 * before any launch, otherwise.  Same lists, tile starts, guard, spare and longest-list words as the group form.
 *   ts_bin_emit_groups     the walk.  Reads cum_tiles_hit[n-1] against capacity itself (it runs BEFORE the offsets) and
 *                          writes nothing when the guard would trip.  scratch: as for ts_bin_scatter_groups
 *   ts_emit_offsets        ts_group_offsets' duties except the bases; cum_tiles_hit not NULL
 *   ts_bin_gather_groups   the fine hop (ts_bin_scatter_groups', fed run by run): tile_bins, the remaining tile starts,
 *                          bucket_ids, one maximum per group
 * ts_bin_stage_capacity(): pairs a chunk can stage in LDS; a chunk that lists more walks twice inside its workgroup. */
int32_t ts_bin_one_walk_form(int32_t n, int32_t num_tiles);
int32_t ts_bin_stage_capacity(void);
int ts_bin_emit_groups(int32_t n, const float* xys, const int32_t* radii, const float* splats,
                       const ts_camera* cam_host, const int32_t* cum_tiles_hit, int64_t capacity, int32_t* bin_ws,
                       int32_t* scratch, void* stream);
/* ts_bin_emit_groups with the SPAN RECORDS the colour stage left (ts_colors_pack_spans_fwd; 4 n int32 words, 16-byte
 * aligned): the walk reads one record per Gaussian instead of xys, radii and splats, which it touches only for a
 * Gaussian whose record says "not representable".  Same lists.  row_spans = NULL: ts_bin_emit_groups.  The records must
 * come from the same camera, and from tight != 0 exactly where splats != NULL here. */
int ts_bin_emit_groups_spans(int32_t n, const float* xys, const int32_t* radii, const float* splats,
                             const int32_t* row_spans, const ts_camera* cam_host, const int32_t* cum_tiles_hit,
                             int64_t capacity, int32_t* bin_ws, int32_t* scratch, void* stream);
int ts_emit_offsets(int32_t n, int32_t num_tiles, int32_t* bin_ws, int32_t* tile_bins,
                    const int32_t* cum_tiles_hit, int64_t capacity, int32_t* longest_list, void* stream);
int ts_bin_gather_groups(int32_t n, int32_t num_tiles, int32_t* bin_ws, int32_t* tile_bins, int32_t* bucket_ids,
                         const int32_t* scratch, void* stream);
int ts_sort_tiles_stats(int32_t num_tiles, const int32_t* tile_bins, const float* depths,
                        const int32_t* bucket_ids, int32_t* gaussian_ids_sorted, int32_t* sort_ws,
                        int32_t* zeroed_counter, int32_t n, const int32_t* bin_ws, int32_t* longest_list,
                        void* stream);
int ts_sort_tiles_above_stats(int32_t num_tiles, const int32_t* tile_bins, const float* depths,
                              const int32_t* bucket_ids, int32_t* gaussian_ids_sorted, int32_t n,
                              const int32_t* bin_ws, int32_t* longest_list, void* stream);

#define TS_RASTER_LOGIT_OPACITY 1 /* `opacity` holds logits: sigmoid (rasterize.py:86) is applied while */
                                  /* packing, and ts_reduce_partials returns the gradient w.r.t. logits */

/* Packs the per-Gaussian operands of the compositing kernels into one 48-byte record:
 *   {x, y, opacity, conic.xx | conic.xy, conic.yy, c0, c1 | c2, c3, slot_base(int), bbox_w | bbox_minx << 16 (int)}
 * channels = 3 (colors[n,3]; c3 = 0) or 4 (colors[n,4]; or, with `depths` non-NULL, colors[n,3] and
 * c3 = depths[i]: the RGB + depth frame of rasterize.py:42-51 in one pass).  slot_base/bbox_w locate the
 * (tile,Gaussian) row of the backward partial buffer: slot = slot_base + ty*bbox_w + tx (16x16 tile column tx,
 * whatever the shape of the lists). */
int ts_pack_splats(int32_t n, int32_t channels, int32_t flags, const float* xys, const int32_t* radii,
                   const float* conics, const float* colors, const float* opacity,
                   const int32_t* cum_tiles_hit, const ts_camera* cam_host, const float* depths,
                   float* splats, void* stream);

/* Front-to-back compositing.  out_img[rows,W,channels], final_Ts[rows,W], final_index[rows,W]
 * where rows = min(16*tile_rows, H - 16*tile_row0).  background: `channels` floats.  final_Ts and
 * final_index exist for the backward pass; both may be NULL together (forward-only rendering). */
/* flags: TS_RASTER_CLAMP_RGB folds the adapter's clamp(rgb, max=1) (rasterize.py:45) into the store of
 * channels 0..2; clamp_mask[rows,W] (bytes, may be NULL when no backward follows) then receives bit c
 * where channel c passes gradient (value <= 1, torch's rule) for ts_raster_bwd. */
#define TS_RASTER_CLAMP_RGB 2
/* TS_RASTER_SPLIT_BLOCKS: four waves per tile, one per 8x8 block (same results per pixel).  For launches
 * with fewer tiles than the GPU has SIMDs (a tile-row stripe of a multi-GPU frame, a small image).  In
 * ts_raster_bwd / ts_reduce_partials the flag makes every (tile, Gaussian) own FOUR partial rows (slot
 * 4 s + block): partials must hold 4 * num_intersects rows and row_flags 4 * num_intersects bytes. */
#define TS_RASTER_SPLIT_BLOCKS 4
/* required with ts_camera.wide_tiles != 0 (TS_E_BADARG without it), meaningless otherwise: one wave per 16x16
 * tile, each walks the list of the wide tile it lies in and skips the Gaussians whose tile box does not hold it */
#define TS_RASTER_NARROW_WAVES 8
/* ts_raster_bwd / ts_reduce_partials(_rows): ROW-FLAG GENERATION.  Without it (g = 0) ts_raster_bwd zeroes
 * row_flags and marks the rows it writes with 1.  A caller that keeps ONE row_flags array alive across passes
 * (all zero at first) can pass a fresh g in 1..255 to both entries of a pass instead: rows are marked with g, only
 * rows marked g count, and nothing is zeroed (the caller zeroes the array itself before reusing a value). */
#define TS_RASTER_FLAG_GEN(g) (((g) & 0xff) << 8)
int ts_raster_fwd(int32_t channels, int32_t flags, const ts_camera* cam_host, const int32_t* tile_bins,
                  const int32_t* gaussian_ids_sorted, const float* splats, const float* background,
                  float* out_img, float* final_Ts, int32_t* final_index, uint8_t* clamp_mask,
                  void* stream);
/* The RGB + depth image as TWO planes (channels = 4 with out_depth != NULL): out_img[P,3] and out_depth[P] - what
 * the adapter hands out as `rgb` and `extras["depth"]` (rasterize.py:45, :51), both contiguous, so that losses on
 * them and their gradients need no slicing of an interleaved image.  out_depth = NULL: ts_raster_fwd. */
int ts_raster_fwd_planes(int32_t channels, int32_t flags, const ts_camera* cam_host, const int32_t* tile_bins,
                         const int32_t* gaussian_ids_sorted, const float* splats, const float* background,
                         float* out_img, float* out_depth, float* final_Ts, int32_t* final_index,
                         uint8_t* clamp_mask, void* stream);

/* ABI 5: ts_raster_fwd_planes with the per-tile sort of the lists of <= 1024 entries inside (bucket_ids[I] ->
 * gaussian_ids_sorted[I], which ts_raster_bwd reads later; ts_sort_tiles_above must have run for the longer lists).
 * Only on 16x16 lists (cam->wide_tiles = 0, no TS_RASTER_NARROW_WAVES: TS_E_BADARG otherwise), with one wave per tile
 * or - TS_RASTER_SPLIT_BLOCKS - one workgroup per tile (its first wave sorts).  Same image, same sorted lists; the latency-bound sort overlaps
 * the VALU-bound compositing of other tiles instead of running as a phase of its own. */
int ts_raster_fwd_sort(int32_t channels, int32_t flags, const ts_camera* cam_host, const int32_t* tile_bins,
                       const int32_t* bucket_ids, const float* depths, int32_t* gaussian_ids_sorted,
                       const float* splats, const float* background, float* out_img, float* out_depth,
                       float* final_Ts, int32_t* final_index, uint8_t* clamp_mask, void* stream);

/* Back-to-front replay.  Writes one TS_PARTIAL_ROW_FLOATS row of raw per-tile sums per contributing
 * (tile,Gaussian), with v_s = dL/dsigma of a pixel and d = xy - pixel:
 *   {S v_s, S v_s dx, S v_s dy, S v_s dx^2, S v_s dx dy, S v_s dy^2, v_c0, v_c1, v_c2, v_c3, -, -}
 * row_flags[I] (bytes) is zeroed by this call and set to 1 for every row written; rows whose flag
 * stays 0 keep stale contents and must be ignored (ts_reduce_partials does).  v_out_alpha may be NULL.
 * clamp_mask: NULL, or the mask ts_raster_fwd wrote under TS_RASTER_CLAMP_RGB (v_out_img is then the
 * gradient w.r.t. the clamped image and is zeroed where the clamp was active). */
int ts_raster_bwd(int32_t channels, int32_t flags, int64_t num_intersects, const ts_camera* cam_host,
                  const int32_t* tile_bins, const int32_t* gaussian_ids_sorted, const float* splats,
                  const float* background, const float* final_Ts, const int32_t* final_index,
                  const float* v_out_img, const float* v_out_alpha, const uint8_t* clamp_mask,
                  float* partials, uint8_t* row_flags, void* stream);
/* planes != 0 (channels = 4): the image gradient as two planes, v_out_img[P,3] and v_out_depth[P]; either may be
 * NULL (that output took no part in the loss: its gradient is zero).  planes = 0: ts_raster_bwd. */
int ts_raster_bwd_planes(int32_t channels, int32_t flags, int64_t num_intersects, const ts_camera* cam_host,
                         const int32_t* tile_bins, const int32_t* gaussian_ids_sorted, const float* splats,
                         const float* background, const float* final_Ts, const int32_t* final_index,
                         const float* v_out_img, const float* v_out_depth, int32_t planes,
                         const float* v_out_alpha, const uint8_t* clamp_mask,
                         float* partials, uint8_t* row_flags, void* stream);

/* Sums each Gaussian's flagged rows (a contiguous range of `partials`, fixed order => run-to-run
 * bit-reproducible gradients), applies the conic / opacity factors read from `splats`, and writes
 * v_xy[n,2], v_conic[n,3] (true partials), v_colors[n,channels], v_opacity[n]. */
int ts_reduce_partials(int32_t n, int32_t channels, int32_t flags, const int32_t* num_tiles_hit,
                       const int32_t* cum_tiles_hit, const float* partials,
                       const uint8_t* row_flags, const float* splats, float* v_xy, float* v_conic,
                       float* v_colors, float* v_opacity, float* v_depth, const uint8_t* color_mask,
                       void* stream);
/* v_depth: NULL, or (channels == 4) the gradient of channel 3 as its own array [n]; v_colors is then
 * [n,3] - the layout the RGB + depth frame hands to ts_sh_colors_bwd / ts_project_bwd.
 * color_mask: NULL, or the colour stage's clamp mask: v_colors[i][c] = 0 where bit c is clear. */

/* ============== whole-frame executor (the adapter's recipe, rasterize.py:26-62, in five calls) ======
 * The reference's GaussianRasterizer.__call__ enqueues ~30 small operations per frame from Python; on
 * scenes of 100 k Gaussians and on multi-GPU tile stripes that host time exceeds the GPU time.  These
 * entries enqueue the same kernels, in the same order, as the per-stage entries above - nothing else -
 * from native code: one ts_frame describes a frame (all buffers caller-allocated; device pointers
 * unless noted), and a frame costs five calls instead of thirty:
 *   ts_frame_fwd_project    project_fwd, scan_tiles; the scan stores the intersection count cum_tiles_hit[n-1]
 *                           into total_host (mapped pinned host memory; a 4-byte copy is queued instead when the
 *                           word is not device-visible) - the caller polls the word, or waits for an event it
 *                           records behind this call, only before step 3
 *   ts_frame_fwd_prepare    colors_pack_fwd (= sh_colors_fwd + pack_splats), bin_count, tile_offsets   (do not need the count)
 *   ts_frame_fwd_composite  bin_scatter, sort_tiles, raster_fwd   (needs bucket_ids / gaussian_ids_sorted
 *                           sized by the count; num_intersects must be set)
 *   ts_frame_bwd_composite  raster_bwd, reduce_partials -> the flat 2-D gradients v_xy | v_conic |
 *                           v_colors | [v_depth] | v_opacity (multi-GPU: all-reduce them after this call)
 *   ts_frame_bwd_params     sh_colors_bwd, project_bwd -> gradients of the six parameter tensors
 * flags: TS_FRAME_TIGHT (tight tile lists: drop (Gaussian, tile) pairs that cannot reach alpha >= 1/255),
 * TS_FRAME_SPLIT (TS_RASTER_SPLIT_BLOCKS for the compositing launches).  channels = 3 (RGB) or 4 (RGB +
 * depth composited in one pass).  Forward-only rendering: final_Ts = final_index = clamp_mask = sh_mask = NULL. */
#define TS_FRAME_TIGHT 1
#define TS_FRAME_SPLIT 2
#define TS_FRAME_NARROW_WAVES 8        /* TS_RASTER_NARROW_WAVES for the compositing launches (cam.wide_tiles) */
#define TS_FRAME_DIRECT_SCATTER 32     /* one-hop ts_bin_scatter (scratch = NULL): A/B timing */
#define TS_FRAME_PLANES 64             /* channels = 4: RGB and depth as two planes (out_img[P,3] + out_depth[P];
                                          v_out_img / v_out_depth, either may be NULL), see ts_raster_fwd_planes */
#define TS_FRAME_LIST_STATS 256        /* total_host points at (at least) TWO mapped words: ts_frame_fwd_prepare stores the
                                        * length of the frame's longest list into word 1 (ts_tile_offsets_stats) */
#define TS_FRAME_SEPARATE_SORT 128     /* ts_sort_tiles + ts_raster_fwd_planes even where ts_raster_fwd_sort applies: A/B */
#define TS_FRAME_STRIPE 16             /* one stripe of a multi-GPU frame: colour stage only for the Gaussians the
                                          stripe lists, clamp mask applied in reduce_partials (before the all-reduce) */
#define TS_FRAME_GROUP_COUNTS 1024      /* the GROUP FORM of the list-building launches (ts_bin_count_groups ...) where it
                                          applies: ts_bin_group_form(n) and no TS_FRAME_DIRECT_SCATTER; ignored otherwise.
                                          Same lists, same image, bit for bit.  For frames whose lists ts_frame_fwd_prepare
                                          counts: ts_shard_stripe_fwd_import counts in the matrix form, so the stripe
                                          frame of a sharded step must not set it */
#define TS_FRAME_ONE_WALK 2048          /* the ONE WALK form (ts_bin_emit_groups ...) where TS_FRAME_GROUP_COUNTS is honoured,
                                          ts_bin_one_walk_form(n, tiles) holds and cam.hints carries no
                                          TS_HINT_BALANCED_WALK; ignored otherwise.  ts_frame_fwd_prepare then enqueues
                                          the colour stage only; ts_frame_fwd_composite emit, offsets, fine hop, sort,
                                          raster.  Same lists, same frame */
#define TS_FRAME_ROW_SPANS (4096)       /* SPAN RECORDS (csrc/row_spans.h) in a ONE WALK frame with `row_spans` set: the colour
                                          stage writes every Gaussian's tile columns per row, the emit launch walks those
                                          instead of computing them (ts_colors_pack_spans_fwd, ts_bin_emit_groups_spans).
                                          Ignored in every other form: no record is computed there.  Same lists */
#define TS_FRAME_SURVIVORS 512         /* SURVIVOR LISTS (csrc/raster.hip): the forward compositing pass hands the entries
                                          it staged to the backward pass, which replays those instead of re-culling the
                                          lists (same rows, same gradients).  Only with the in-kernel sort on 16x16 lists
                                          without TS_FRAME_SPLIT / NARROW_WAVES / SEPARATE_SORT (ignored otherwise), and
                                          `survivors` set; bucket_ids then holds the survivors' ids after the forward pass */
#define TS_FRAME_LINEAR_OPACITY (8192)   /* `opacities` holds opacities, not logits: the executor drops TS_RASTER_LOGIT_OPACITY
                                          from the flag words of the colour / pack stage, of ts_reduce_partials (v_opacity
                                          is then the gradient of the opacity itself) and of the sharded owner stage.  The
                                          antialiased mode renders with the compensated opacities of ts_antialias_fwd this
                                          way; the kernels test the bit at run time */
typedef struct ts_frame {
    int32_t n, num_bases, sh_degree, channels, flags;
    int32_t flag_gen;                         /* row-flag generation of the backward pass (0: zero row_flags) */
    ts_camera cam;
    /* parameters and camera (rasterize.py:64-86): log-scales, raw quaternions, opacity logits */
    const float *means, *scales, *quats, *opacities, *colors_dc, *colors_rest;
    const float *view34, *projview, *origin, *background;     /* background: `channels` floats */
    /* per-Gaussian outputs / intermediates */
    float *xys, *depths, *conics, *colors, *splats;
    int32_t *radii, *num_tiles_hit, *cum_tiles_hit;
    uint8_t* sh_mask;
    int32_t *scan_ws, *bin_ws, *tile_bins;
    int32_t* total_host;                      /* pinned HOST int32 */
    /* per-intersection buffers and the count they are sized by; capacity >= 0: the buffers were sized from an
     * estimate before the count was known (ts_tile_offsets' guard), -1: from the count itself */
    int64_t num_intersects;
    int64_t capacity;
    int32_t *bucket_ids, *gaussian_ids_sorted;
    /* image outputs */
    float *out_img, *final_Ts;
    int32_t* final_index;
    uint8_t* clamp_mask;
    /* backward */
    const float* v_out_img;
    float* partials;
    uint8_t* row_flags;
    float *v_xy, *v_conic, *v_colors, *v_depth, *v_opacity;
    float *v_means, *v_scales, *v_quats, *v_colors_dc, *v_colors_rest;
    /* TS_FRAME_PLANES: the depth plane of the image and of its gradient */
    float* out_depth;
    const float* v_out_depth;
    /* TS_FRAME_SURVIVORS: int32 workspace, 8 * num_tiles rounded up to 64, plus one word per list entry (the buffers'
     * capacity) - written by ts_frame_fwd_composite, read by ts_frame_bwd_composite */
    int32_t* survivors;
    /* TS_FRAME_ROW_SPANS: 4 n int32 words (one 16-byte record per Gaussian, 16-byte aligned), or NULL - written by
     * ts_frame_fwd_prepare, read by ts_frame_fwd_composite */
    int32_t* row_spans;
} ts_frame;
int32_t ts_frame_struct_bytes(void);       /* sizeof(ts_frame): bindings check their mirror against it */
int ts_frame_fwd_project(const ts_frame* f, void* stream);
int ts_frame_fwd_prepare(const ts_frame* f, void* stream);
int ts_frame_fwd_composite(const ts_frame* f, void* stream);
int ts_frame_bwd_composite(const ts_frame* f, void* stream);
int ts_frame_bwd_params(const ts_frame* f, void* stream);

/* ENTRY PROBE: while one is set, every executor function (ts_frame_*, ts_shard_*) calls fn(entry, 0, user) before and
 * fn(entry, 1, user) after each per-stage entry it issues - also when that entry fails and the executor returns early,
 * so the calls always pair up.  `entry` is the entry's name in a per-entry table: ts_tile_offsets also stands for
 * ts_tile_offsets_stats, ts_sort_tiles for ts_sort_tiles_above, ts_raster_fwd / ts_raster_bwd for whichever compositing
 * launch the frame takes, ts_route_count for ts_route_count_padded, ts_owner_fwd_fused / ts_owner_bwd_fused for
 * ts_shard_owner_*_fused.  The executor's own copies and fills (the count word, the send buffer) lie outside every
 * pair.  What ops.kernel_timer records events with: the table times the frame that runs.  One probe per process, seen by
 * every thread (a frame's backward pass may run on another thread than its forward pass); fn must not throw.  NULL
 * switches it off: an entry then costs one relaxed load.  Returns 0. */
typedef void (*ts_entry_probe)(const char* entry, int32_t end, void* user);
int ts_set_entry_probe(ts_entry_probe fn, void* user);

/* ============== Gaussian-sharded multi-GPU frame (csrc/shard.hip) =====================
 * One rank per GPU owns a contiguous range of Gaussians and one stripe of tile rows.  Per frame it projects and
 * colours its own Gaussians (ts_project_fwd / ts_colors_pack_fwd with the FULL-frame camera), routes a 64-byte
 * export record of each visible one to the rank(s) whose stripe its tile box reaches, and composites the
 * records it receives; backward returns one 48-byte gradient row per record to the owner.  The exchange itself
 * (two all_to_all calls) is the caller's: these entries produce and consume its buffers.
 *
 * Export record (TS_EXPORT_RECORD_FLOATS floats): {x, y, opacity, conic.xx | conic.xy, conic.yy, c0, c1 |
 * c2, c3, depth, radius (int) | global id (int), -, -, -}: the first ten floats are those of the packed
 * compositing record (ts_pack_splats).
 * Gradient row (TS_PARTIAL_ROW_FLOATS floats): {v_x, v_y, v_conic.xx, v_conic.xy | v_conic.yy, v_c0, v_c1, v_c2 |
 * v_c3 (depth channel), v_opacity (w.r.t. the sigmoid's output), -, -}. */
#define TS_MAX_RANKS 16
#define TS_EXPORT_RECORD_FLOATS 16
typedef struct ts_stripes {   /* rank d renders tile rows [row[d], row[d+1]) */
    int32_t num;
    int32_t row[TS_MAX_RANKS + 1];
} ts_stripes;
/* route_ws: >= ts_route_ws_ints(n, num_ranks) int32; written by ts_route_count, read by ts_route_pack and
 * ts_route_accumulate of the same frame.  counts (device, num_ranks int32) <- records per destination. */
int64_t ts_route_ws_ints(int32_t n, int32_t num_ranks);
int ts_route_count(int32_t n, const float* xys, const int32_t* radii, const ts_camera* cam_host,
                   const ts_stripes* stripes_host, int32_t* route_ws, int32_t* counts, void* stream);
/* PADDED groups: group_base_host[num_ranks + 1] (ascending, host memory, read during the call) fixes where every
 * destination's group starts in the send buffer and in the returned gradient rows - capacities the caller chose
 * BEFORE this frame's counts exist (e.g. from the previous frame), so that the exchange can be enqueued without a
 * host read of the counts.  The caller zeroes the send buffer (an all-zero record lists nothing at its destination:
 * radius 0), checks counts[d] <= group_base_host[d+1] - group_base_host[d] when it reads them - e.g. together with
 * the stripe's pair count at the end of the forward pass - and runs the frame again with exact groups if not.
 * group_base_host = NULL: ts_route_count. */
int ts_route_count_padded(int32_t n, const float* xys, const int32_t* radii, const ts_camera* cam_host,
                          const ts_stripes* stripes_host, const int32_t* group_base_host, int32_t* route_ws,
                          int32_t* counts, void* stream);
/* records[sum(counts), 16]: grouped by destination (ascending), ascending Gaussian index inside a group;
 * splats = the owner's packed records (colours, sigmoid opacity), gid_base = global index of Gaussian 0. */
int ts_route_pack(int32_t n, int32_t gid_base, const float* xys, const int32_t* radii, const float* depths,
                  const float* splats, const ts_camera* cam_host, const ts_stripes* stripes_host,
                  const int32_t* route_ws, float* records, void* stream);
/* importing rank, m received records: the arrays binning takes (num_tiles_hit for cam's stripe) ... */
int ts_import_records(int32_t m, const float* records, const ts_camera* cam_host, float* xys, float* depths,
                      int32_t* radii, int32_t* num_tiles_hit, void* stream);
/* ... and, after ts_scan_tiles, the 48-byte compositing records */
int ts_import_pack(int32_t m, const float* records, const int32_t* cum_tiles_hit, const ts_camera* cam_host,
                   float* splats, void* stream);
/* ts_reduce_partials writing one gradient row per (imported) Gaussian instead of the five arrays */
int ts_reduce_partials_rows(int32_t n, int32_t channels, int32_t flags, const int32_t* num_tiles_hit,
                            const int32_t* cum_tiles_hit, const float* partials, const uint8_t* row_flags,
                            const float* splats, float* grad_rows, void* stream);
/* owner: grad_rows[sum(counts), 12] in the order of ts_route_pack's records -> dense 2-D gradients of the owned
 * Gaussians (rows of a Gaussian summed in ascending stripe order; clamp mask of the colour stage and the
 * sigmoid's derivative applied: v_opacity is w.r.t. the logits).  v_depth may be NULL (channels == 3). */
int ts_route_accumulate(int32_t n, int32_t channels, const float* xys, const int32_t* radii, const float* splats,
                        const uint8_t* color_mask, const ts_camera* cam_host, const ts_stripes* stripes_host,
                        const int32_t* route_ws, const float* grad_rows, float* v_xy, float* v_conic,
                        float* v_colors, float* v_depth, float* v_opacity, void* stream);

/* Executor entries of the sharded frame (one native call per group of launches, as ts_frame_* above).  Two
 * ts_frame describe a rank's frame: fo = its OWNED Gaussians with the full-frame camera, fs = the records its
 * stripe imported (n = number of records, cam = the stripe).
 *   ts_shard_owner_fwd          project_fwd, colors_pack_fwd, route_count            (fo)
 *   ts_route_pack               once the caller knows the counts
 *   ts_shard_stripe_fwd_import  import_records, scan_tiles (total -> fs->total_host), import_pack, bin_count,
 *                               tile_offsets                                          (fs)
 *   ts_frame_fwd_composite      bin_scatter, sort_tiles, raster_fwd                   (fs)
 *   ts_shard_stripe_bwd         raster_bwd, reduce_partials_rows -> grad_rows[n, 12]  (fs)
 *   ts_shard_owner_bwd          route_accumulate, sh_colors_bwd, project_bwd          (fo) */
int ts_shard_owner_fwd(const ts_frame* fo, const ts_stripes* stripes_host, int32_t* route_ws, int32_t* counts,
                       void* stream);
int ts_shard_owner_fwd_padded(const ts_frame* fo, const ts_stripes* stripes_host, const int32_t* group_base_host,
                              int32_t* route_ws, int32_t* counts, void* stream);   /* see ts_route_count_padded */
/* The owner stage's forward pass in ONE launch + the route scan (round 5; what ts_shard_owner_fwd* issue when the rank
 * owns at most TS_SMALL_N_FUSED Gaussians - environment, default 262144, 0 = never -: a rank of 8 on a 1 M scene is
 * bound by launch floors there): projection (project_flags as ts_project_fwd), colour stage on the split coefficient
 * tensors, packed records (cum_tiles_hit := num_tiles_hit, as the owner stage packs them) and the destination counts
 * of ts_route_count_padded - the same bits in every array the three launches write. */
int ts_shard_owner_fwd_fused(int32_t n, int32_t degrees_to_use, int32_t num_bases, const float* means3d,
                             const float* scales, const float* quats, const float* view34, const float* projview,
                             const ts_camera* cam_host, int32_t project_flags, const float* origin,
                             const float* colors_dc, const float* colors_rest, const float* opacity, int32_t channels,
                             int32_t raster_flags, float* xys, float* depths, int32_t* radii, float* conics,
                             int32_t* num_tiles_hit, uint8_t* clamp_mask, float* splats, const ts_stripes* stripes_host,
                             const int32_t* group_base_host, int32_t* route_ws, int32_t* counts, void* stream);
/* ... and its backward pass in one launch (what ts_shard_owner_bwd issues for such a shard): ts_route_accumulate,
 * ts_sh_colors_bwd (no mask: it was applied to the sums) and ts_project_bwd (flags 3) in the lane that owns the Gaussian;
 * the same bits in v_xy / v_conic / v_colors / v_depth / v_opacity and the six parameter gradients. */
int ts_shard_owner_bwd_fused(int32_t n, int32_t channels, int32_t degrees_to_use, int32_t num_bases, const float* means3d,
                             const float* scales, const float* quats, const float* view34, const float* projview,
                             const float* origin, const float* xys, const int32_t* radii, const float* splats,
                             const uint8_t* color_mask, const ts_camera* cam_host, const ts_stripes* stripes_host,
                             const int32_t* route_ws, const float* grad_rows, float* v_xy, float* v_conic,
                             float* v_colors, float* v_depth, float* v_opacity, float* v_colors_dc, float* v_colors_rest,
                             float* v_means3d, float* v_scales, float* v_quats, void* stream);
int ts_shard_stripe_fwd_import(const ts_frame* fs, const float* records, void* stream);
int ts_shard_stripe_bwd(const ts_frame* fs, float* grad_rows, void* stream);
int ts_shard_owner_bwd(const ts_frame* fo, const ts_stripes* stripes_host, const int32_t* route_ws,
                       const float* grad_rows, void* stream);

/* ABI 6 - the WHOLE STEP of one rank in four calls, split only where the two collectives sit:
 *   ts_shard_rank_fwd_a   owner stage: project_fwd, colors_pack_fwd, route_count (padded groups), the send buffer zeroed,
 *                         route_pack                                  -> send[send_rows, 16], counts[ranks]
 *      (caller: all_to_all of the records with the groups' capacities as split sizes, all_gather of the counts)
 *   ts_shard_rank_fwd_b   stripe stage: import_records, scan_tiles (total -> fs->total_host), import_pack, bin_count,
 *                         tile_offsets (capacity guard), bin_scatter, sort_tiles, raster_fwd   <- recv[recv_rows, 16]
 *   ts_shard_rank_bwd_a   raster_bwd, reduce_partials_rows            -> grad_rows[recv_rows, 12]
 *      (caller: the reverse all_to_all)
 *   ts_shard_rank_bwd_b   route_accumulate, sh_colors_bwd, project_bwd <- back[send_rows, 12]
 * Nothing of a frame is looked at by the host between the calls: the groups of the exchange have the CAPACITIES the
 * caller derived from an earlier frame (group_base_host: ranks + 1 ascending offsets into send / back), the lists of the
 * stripe the capacity fs->capacity (ts_tile_offsets' guard).  The caller reads the counts and the stripe's pair count
 * once the forward pass is enqueued and runs the frame again with exact sizes (the separate entries above) if a group
 * or the lists outgrew their capacity.  fo / fs as for the entries above; fs->n = recv_rows. */
typedef struct ts_rank_step {
    ts_stripes stripes;
    int32_t group_base[TS_MAX_RANKS + 1];      /* HOST: offsets of the destination groups in send / back */
    int32_t gid_base;                           /* global index of the rank's first Gaussian */
    int32_t send_rows, recv_rows;               /* = group_base[ranks]; sum of the capacities of the groups received */
    int32_t* route_ws;                          /* >= ts_route_ws_ints(fo->n, ranks) */
    int32_t* counts;                            /* device, ranks int32: records per destination of THIS frame */
    float *send, *recv;                         /* [send_rows, 16], [recv_rows, 16] */
    float *grad_rows, *back;                    /* [recv_rows, 12], [send_rows, 12] */
} ts_rank_step;
int32_t ts_rank_step_struct_bytes(void);
int ts_shard_rank_fwd_a(const ts_frame* fo, const ts_rank_step* r, void* stream);
int ts_shard_rank_fwd_b(const ts_frame* fs, const ts_rank_step* r, void* stream);
int ts_shard_rank_bwd_a(const ts_frame* fs, const ts_rank_step* r, void* stream);
int ts_shard_rank_bwd_b(const ts_frame* fo, const ts_rank_step* r, void* stream);

/* ============ training-step ops around the path (scripts/train.py:58-63,97) ===== */

/* Photometric loss of the training step (train.py:58-69) and its gradient w.r.t. the rendered image, one descriptor
 * for every image layout, with or without a mask:
 *   L = c_l1 * mean|X - Y| + c_ssim * (1 - SSIM(X, Y)) [+ c_depth * mean|depth - D|]   (c = 1-lambda, lambda, lambda_depth)
 * X = the first three floats of every pixel of `image`, Y = target[H,W,3], D = depth_target[H,W], float32.  SSIM as
 * pytorch_msssim.SSIM(data_range=1, size_average=True, channel=3) (model_gaussian.py:57): 11-tap Gaussian window
 * (sigma 1.5), valid filtering, K = (0.01, 0.03).  The rendered depth is channel 3 of `image` (pixel_floats == 4: the
 * compositing kernels' own RGB + depth output, no slicing / re-packing of a 33 MB image and its gradient per step) or
 * the plane `depth` (pixel_floats == 3: ts_raster_fwd_planes); without either there is no depth term.
 * The entry leaves the three partial-derivative maps and the partial sums in `ws` - {ssim, l1, depth l1} per wave of
 * pass 1 at ws + 9 (H-10)(W-10), (ts_photometric_ws_floats - 9 (H-10)(W-10)) / 3 triples - and, if v_image != NULL,
 *   v_image[..., :3] = w_l1 * sign(X - Y) + w_ssim * dSSIMsum/dX      (caller passes w_l1 = c_l1 / (3 H W),
 *   depth gradient   = w_depth * sign(depth - D)                        w_ssim = -c_ssim / (3 (H-10)(W-10)),
 *                                                                       w_depth = c_depth / (H W))
 * the depth gradient going to v_image[..., 3] (pixel_floats == 4) or to the plane v_depth; it is 0 everywhere without
 * a depth target.
 * TS_LOSS_MASKED (csrc/mask_math.h): byte b of mask[H,W] weighs its pixel by m = b / 255.0f
 * (255: the pixel counts, 0: it is ignored).  The loss is then evaluated on the substituted image X' = blend(X, Y, m)
 * - X where b == 255, fmaf(m, X - Y, Y) otherwise - with the depth term m |depth - D| and the gradients
 *   v_image = m * dL/dX',   depth gradient = m * w_depth * sign(depth - D).
 * Same weights (NOT renormalised by the mask's area), same workspace and partial sums.  An all-255 mask gives the
 * unmasked bits; a pixel with b == 0 gets a gradient of exactly zero.
 * TS_E_BADARG, before any launch: a NULL descriptor, image, target or ws; height or width <= 10; pixel_floats other
 * than 3 or 4; unknown flag bits; TS_LOSS_MASKED with a NULL mask, or a mask without the flag; a depth plane with
 * pixel_floats == 4; a depth target with neither a fourth channel nor a depth plane; v_depth without a depth plane or
 * without v_image. */
int64_t ts_photometric_ws_floats(int32_t height, int32_t width);
#define TS_LOSS_MASKED 1
typedef struct ts_loss {
    int32_t height, width;
    int32_t pixel_floats;        /* 3 or 4: floats per pixel of image and v_image; 4: channel 3 is the depth */
    int32_t flags;               /* TS_LOSS_MASKED: mask is read (the masked kernels); 0: mask must be NULL */
    const float* image;          /* [H, W, pixel_floats] */
    const float* depth;          /* [H, W] plane, only with pixel_floats == 3; NULL otherwise */
    const float* target;         /* [H, W, 3] */
    const float* depth_target;   /* [H, W] or NULL: no depth term */
    const uint8_t* mask;         /* [H, W] */
    float w_l1, w_ssim, w_depth;
    float* ws;                   /* >= ts_photometric_ws_floats(H, W) */
    float* v_image;              /* layout of image, or NULL: forward only */
    float* v_depth;              /* [H, W] or NULL; only with a depth plane and v_image */
} ts_loss;
int32_t ts_loss_struct_bytes(void);      /* sizeof(ts_loss): bindings check their mirror against it */
int ts_photometric_loss_rgbd(const ts_loss* loss, void* stream);
/* ABI 8: the loss VALUE from the partial sums the entry above left in `ws` (same height, width and weights):
 *   out4 = {loss, mean|X - Y|, SSIM, mean|depth - depth_target|}   (device floats; sums taken in double, fixed order)
 * with loss = (1 - lambda) * out4[1] + lambda * (1 - out4[2]) + lambda_depth * out4[3] as the weights encode it
 * (train.py:58-69).  One small launch instead of a dozen one-element tensor operations on the caller's side. */
int ts_photometric_loss_reduce(int32_t height, int32_t width, float w_l1, float w_ssim, float w_depth,
                               const float* ws, float* out4, void* stream);
/* ts_mask_blend: out[height, width, 3] <- the substituted image X' of TS_LOSS_MASKED for image, target
 * [height, width, 3] (height, width >= 1). */
int ts_mask_blend(int32_t height, int32_t width, const float* image, const float* target, const uint8_t* mask,
                  float* out, void* stream);

/* torch.optim.Adam (defaults: no amsgrad, no weight decay; train.py:26) on up to TS_ADAM_MAX_TENSORS
 * tensors with per-tensor learning rates (model_gaussian.py:112-120) in one launch.  The pointer
 * tables are HOST arrays of device pointers.  steps_host[i] >= 1 is tensor i's own 1-based step count
 * (torch keeps it per parameter: a tensor without a gradient is skipped and does not age). */
#define TS_ADAM_MAX_TENSORS 8
int ts_adam_step(int32_t num_tensors, float* const* params_host, const float* const* grads_host,
                 float* const* exp_avg_host, float* const* exp_avg_sq_host, const int64_t* numel_host,
                 const float* lr_host, const int32_t* steps_host, float beta1, float beta2, float eps,
                 void* stream);

/* FUSED ADAM (round 6; scripts/train.py:93-97): the parameter-stage backward kernels apply the optimiser to the gradient
 * they hold in registers - the very update of ts_adam_step, bit for bit - instead of writing six gradient tensors that
 * the optimiser launch reads once.  ts_adam: the six groups in the order of the model's parameters() (model_gaussian.py:
 * 112-120): means, colors_dc, colors_rest, scales, quats, opacities; step[k] >= 1 is group k's own 1-based step count.
 *   ts_sh_colors_bwd_adam   ts_sh_colors_bwd with colors_dc / colors_rest (and their moments) updated in place
 *   ts_project_bwd_adam     ts_project_bwd (no v_cov3d) with means3d / scales / quats updated in place - the RAW tensors:
 *                           pass the flags the forward pass used (TS_PROJECT_LOG_SCALES | TS_PROJECT_RAW_QUATS) - and,
 *                           when `opacities` is not NULL, the opacity logits from v_opacity (ts_reduce_partials with
 *                           TS_RASTER_LOGIT_OPACITY)
 *   ts_frame_bwd_params_adam  what ts_frame_bwd_params enqueues, with the two entries above: no parameter gradient is
 *                           written (f->v_means ... f->v_colors_rest are not read); f->v_xy - xys.grad - still is */
#define TS_ADAM_MEANS 0
#define TS_ADAM_COLORS_DC 1
#define TS_ADAM_COLORS_REST 2
#define TS_ADAM_SCALES 3
#define TS_ADAM_QUATS 4
#define TS_ADAM_OPACITIES 5
typedef struct ts_adam {
    float* exp_avg[6];
    float* exp_avg_sq[6];
    float lr[6];
    int32_t step[6];
    float beta1, beta2, eps;
} ts_adam;
int ts_sh_colors_bwd_adam(int32_t n, int32_t degrees_to_use, int32_t num_bases, const float* means3d,
                          const float* origin, const uint8_t* clamp_mask, const float* v_colors,
                          float* colors_dc, float* colors_rest, const ts_adam* adam_host, void* stream);
int ts_project_bwd_adam(int32_t n, float* means3d, float* scales, float* quats, const float* viewmat,
                        const float* projmat, const ts_camera* cam_host, int32_t flags, const int32_t* radii,
                        const float* v_xy, const float* v_depth, const float* v_conic, float* opacities,
                        const float* v_opacity, const ts_adam* adam_host, void* stream);
int ts_frame_bwd_params_adam(const ts_frame* f, const ts_adam* adam_host, void* stream);

/* ================== densification hooks (model_gaussian.py:130-242) ========= */
/* Call order of one densify_and_prune (model_gaussian.py:138-195):
 *   ts_densify_classify -> ts_densify_plan -> (host reads counts[4]) -> ts_gather_rows x 3 tables
 *   (parameters: copy_rows = N'; exp_avg, exp_avg_sq: copy_rows = K, the new rows are zero)
 *   -> ts_split_fixup on rows [K + C, N').  update_state(optim, mask) alone (train.py:103-105) is
 *   flags = mask ? TS_DENSIFY_PRUNE : 0 -> ts_densify_plan -> ts_gather_rows x 3.               */
#define TS_DENSIFY_CLONE 1   /* small scale, large mean 2-D gradient (:152-153): row is duplicated       */
#define TS_DENSIFY_SPLIT 2   /* large scale, large gradient (:164-165): two samples replace the row      */
#define TS_DENSIFY_PRUNE 4   /* row is dropped (:181-183; every split row is also pruned)                 */

typedef struct ts_densify_policy {
    float interval_densify;  /* model.interval_densify (:148)                                   */
    float max_dim;           /* max(width, height) of the last rendered camera (:146-148)       */
    float tau_means;         /* --tau-means, train.py:212                                       */
    float scale_thresh;      /* --densify-scale-thresh, train.py:213                            */
} ts_densify_policy;

/* update_grad_accum (:132): accum[i] += ||v_xy[i]||_2.  v_xy [n,2] is extras['xys'].grad. */
int ts_grad_accum(int32_t n, const float* v_xy, float* accum, void* stream);

/* Per-Gaussian policy bits (:148-183).  scales are log-scales [n,3], opacities logits [n]. */
int ts_densify_classify(int32_t n, const float* accum, const float* scales, const float* opacities,
                        const ts_densify_policy* policy, uint8_t* flags, void* stream);

/* Row map of the rebuilt tensors.  counts (device, 4 int32) <- {K kept, C cloned, S split, N' = K + C + 2S};
 * src_of (device, capacity >= 2 n int32; N' <= 2 n always) <- source row of every new row, laid out
 * [kept | cloned | split sample 0 | split sample 1], source order within each part - the order of
 * torch.cat((param[~mask], cat(cloned, split.repeat(2)))) at :187-192, :213-226.
 * ws: >= ts_densify_ws_ints(n) int32. */
int64_t ts_densify_ws_ints(int32_t n);
int ts_densify_plan(int32_t n, const uint8_t* flags, int32_t* ws, int32_t* counts, int32_t* src_of,
                    void* stream);

/* dst_i[r, :] = r < copy_rows ? src_i[src_of[r], :] : 0  for up to TS_GATHER_MAX_TENSORS row-major
 * float32 tensors (row_floats_host[i] floats per row) in one launch.  Pointer tables are HOST arrays. */
#define TS_GATHER_MAX_TENSORS 8
int ts_gather_rows(int32_t num_tensors, const float* const* src_host, float* const* dst_host,
                   const int32_t* row_floats_host, int32_t dst_rows, int32_t copy_rows,
                   const int32_t* src_of, void* stream);

/* GaussianDistribution.sample (:547-557) for the 2S sampled rows: with i = src_of_split[j],
 * means_out[j] = R(quats[i] / |quats[i]|) (z[j] * exp(scales[i])) + means[i],
 * scales_out[j] = log(exp(scales[i]) / 1.6).  z [rows,3] are unit normal draws (the reference's
 * torch.normal(0, std) is z * std).  src_of_split = src_of + K + C; *_out point at row K + C. */
int ts_split_fixup(int32_t rows, const int32_t* src_of_split, const float* means, const float* scales,
                   const float* quats, const float* z, float* means_out, float* scales_out,
                   void* stream);

/* ======================== PLY record layout (model_gaussian.py:330-361) ===== */
/* export_ply's per-Gaussian float32 record: x y z | nx ny nz (zeros) | f_dc_0..2 |
 * f_rest_0..3*k_rest-1 (channel-major: f_rest[c * k_rest + k] = colors_rest[i, k, c], :351) | opacity |
 * scale_0..2 | rot_0..3  ->  ts_ply_row_floats(k_rest) = 17 + 3 k_rest floats (62 at SH degree 3).
 * pack: six tensors -> rows [n, W]; unpack: the inverse (the normals are ignored).  Device pointers. */
int32_t ts_ply_row_floats(int32_t k_rest);
int ts_ply_pack_rows(int32_t n, int32_t k_rest, const float* means, const float* colors_dc,
                     const float* colors_rest, const float* opacities, const float* scales,
                     const float* quats, float* rows, void* stream);
int ts_ply_unpack_rows(int32_t n, int32_t k_rest, const float* rows, float* means, float* colors_dc,
                       float* colors_rest, float* opacities, float* scales, float* quats,
                       void* stream);

/* ============== point-cloud initialisation (GaussianModel.from_pcd, model_gaussian.py:66-90) ===== */
/* Exact k nearest neighbours: for each of the m queries (float32 [m,3]) the k <= TS_KNN_MAX_K nearest of
 * the n points (float32 [n,3]), ascending in (distance, index), distances sqrt(dx*dx + dy*dy + dz*dz)
 * evaluated in double and rounded to float32 -> dist float32 [m,k], idx int32 [m,k].  queries == points
 * with m == n is the self-search (every point finds itself at distance 0).  The result is a fixed
 * function of the input (bit-identical from run to run).  ws: >= ts_knn_ws_bytes(n, m, k) bytes, 256-byte
 * aligned.  stats: NULL, or a device int32[2] <- {queries that took the brute-force fallback, rings of
 * grid cells the longest ring search visited}.  TS_E_BADARG (device untouched): n < 1, k outside
 * 1..TS_KNN_MAX_K, k > n, m < 0, NULL points / ws, NULL queries / dist / idx with m > 0. */
#define TS_KNN_MAX_K 16
int64_t ts_knn_ws_bytes(int32_t n, int32_t m, int32_t k);
int ts_knn(int32_t n, const float* points, int32_t m, const float* queries, int32_t k, float* dist,
           int32_t* idx, void* ws, int32_t* stats, void* stream);

/* The six tensors of from_pcd in one launch: means = xyz; colors_dc = RGB2SH(colors / 255) (colors:
 * float32 [n,3] holding 0..255); colors_rest [n, k_rest, 3] = 0; scales [n,3] = log(float32(mean of the
 * double distances to neighbours 1..3)) from knn_idx, the int32 [n,4] k = 4 self-search (column 0, the
 * point itself or a coincident one, is dropped); quats [n,4] = random_quat_tensor's formula of the
 * uniforms u, v, w [n] (utils.py:15-27); opacities [n,1] = logit(0.1).  mean_dist: NULL, or float32 [n]
 * <- the mean distance before the log.  TS_E_BADARG: n < 4, k_rest < 0, a NULL pointer
 * (colors_rest may be NULL when k_rest == 0). */
int ts_init_from_points(int32_t n, int32_t k_rest, const float* xyz, const float* colors, const float* u,
                        const float* v, const float* w, const int32_t* knn_idx, float* means,
                        float* colors_dc, float* colors_rest, float* scales, float* quats,
                        float* opacities, float* mean_dist, void* stream);

/* ================= surface regularisers of the training loop (scripts/train.py:71-75) ============== */
/* Opacity entropy: o = sigmoid(opacities[i]), loss[0] <- -mean(o log(o + 1e-10) + (1 - o) log(1 - o + 1e-10))
 * over the n logits (float32 [n]; a [n,1] tensor is the same memory); v_opacities: NULL, or float32 [n] <-
 * d loss / d opacities (autograd's chain of that expression).  Deterministic (no atomics; fixed-order sums in
 * double).  ws: >= ts_opacity_entropy_ws_bytes(n) bytes, 8-byte aligned.  TS_E_BADARG: n < 1, a NULL pointer
 * (v_opacities may be NULL). */
int64_t ts_opacity_entropy_ws_bytes(int32_t n);
int ts_opacity_entropy(int32_t n, const float* opacities, float* loss, float* v_opacities, void* ws, void* stream);

/* SuGaR density regulariser (scripts/train.py:77-91, model_gaussian.py:244-326).
 * ts_density_sample: m sample points of the n Gaussians.  Rows: rows_in (int32 [m], given), or the inverse CDF of
 * uniforms (float32 [m] in [0, 1)) over the weights prod(exp(scales)) (TS_DENSITY_WEIGHTS_AREA) or their inclusive
 * prefix sums (TS_DENSITY_WEIGHTS_REFERENCE, the reference's quirk), prefix sums in double by a fixed tree.
 * points[i] = means[r] + R(quats[r] / |quats[r]|) (exp(scales[r]) * normals[i]); rows <- r (-1 and NaN points for a
 * given row outside [0, n)); frozen float32 [m, TS_DENSITY_FROZEN] <- {normals, exp(scales[r]), quats[r]}.
 * ws: >= ts_density_sample_ws_bytes(n) bytes, 256-byte aligned.
 * ts_density_loss: with knn int32 [m, TS_DENSITY_K] (the points' neighbours among the means), depth float32 [H, W]
 * and view_proj_host (host float[32]: the row-major 4x4 view, then projection matrix): out float32[3] <- {mean of
 * |d - approx| over the masked points (NaN if none), 1 / count (0 if none), count}.  density / beta / approx /
 * mask: all NULL or all float32 [m] (mask uint8) <- the per-point values.  grad_rows / tap_keys / tap_vals: all NULL
 * (forward only) or float32 [m * (TS_DENSITY_K + 1), TS_DENSITY_ROW] <- the unscaled gradient rows {means, scales,
 * quats, opacities} of every (point, neighbour) pair, then of every point's sampling source (through frozen), and
 * int32 / float32 [m, 4] <- the bilinear depth taps (pixel y * W + x, or H * W for none; d loss / d depth there,
 * unscaled).  ws: >= ts_density_loss_ws_bytes(m) bytes.  TS_E_BADARG: n < TS_DENSITY_K, m < 1, H * W >= 2^31.
 * ts_segment_sum: out float32 [num_keys, width] <- scale[0] * the sum over e of vals[perm[e], :] for
 * keys_sorted[e] == key (keys >= num_keys dropped), entries summed in their sorted order in double, in chunks;
 * width 1 or TS_DENSITY_ROW.  ws: >= ts_segment_sum_ws_bytes(entries, width) bytes, 256-byte aligned.
 * All three are deterministic (no atomics). */
#define TS_DENSITY_K 16
#define TS_DENSITY_ROW 11
#define TS_DENSITY_FROZEN 10
#define TS_DENSITY_PROJ_REFERENCE 0
#define TS_DENSITY_PROJ_SCREEN 1
#define TS_DENSITY_WEIGHTS_REFERENCE 0
#define TS_DENSITY_WEIGHTS_AREA 1
int64_t ts_density_sample_ws_bytes(int32_t n);
int ts_density_sample(int32_t n, int32_t m, int32_t weights, const float* means, const float* scales, const float* quats,
                      const float* uniforms, const int32_t* rows_in, const float* normals, int32_t* rows, float* points,
                      float* frozen, void* ws, void* stream);
int64_t ts_density_loss_ws_bytes(int32_t m);
int ts_density_loss(int32_t n, int32_t m, const float* points, const int32_t* rows, const float* frozen,
                    const int32_t* knn, const float* means, const float* scales, const float* quats,
                    const float* opacities, int32_t height, int32_t width, const float* depth,
                    const float* view_proj_host, int32_t projection, float znear, float* out, float* density,
                    float* beta, float* approx, uint8_t* mask, float* grad_rows, int32_t* tap_keys, float* tap_vals,
                    void* ws, void* stream);
int64_t ts_segment_sum_ws_bytes(int64_t entries, int32_t width);
int ts_segment_sum(int64_t entries, int32_t width, int32_t num_keys, const int32_t* keys_sorted, const int64_t* perm,
                   const float* vals, const float* scale, float* out, void* ws, void* stream);

/* SuGaR level-set surface points (model_gaussian.py:401-460, scene.py:165-192).  Additive
 * entries: the ABI version is unchanged.  None of them allocates, synchronises or needs a workspace of its own; all
 * are deterministic (plain stores, no atomics).
 * ts_extract_pack: per Gaussian, records float32 [n, TS_EXTRACT_RECORD] <- {mean, U00 U01 U02 U11 U12 U22, sigmoid(o)}
 * with Sigma^-1 = R diag(exp(-2 s)) R^T = U^T U (U upper triangular, evaluated in double, rounded once), and
 * p_std float32 [n] <- |exp(scales)|.  TS_E_BADARG: n < 1, a NULL pointer.
 * ts_extract_rays: per flat pixel index pixel_ids[i] (int64 [m]; an index outside [0, H * W) is an empty pixel and
 * reads nothing): depth z = depth[f], NDC x / y by the convention (TS_EXTRACT_PIX_REFERENCE: x = f % H, y = f / H,
 * ((x + 0.5) - W / 2) / H * 2 and ((y + 0.5) - H / 2) / W * 2 with integer halves, the reference as it stands;
 * TS_EXTRACT_PIX_SCREEN: column f % W, row f / W, (col + 0.5 - W/2) * 2 / W), z_ndc = (P22 z + P23) / z, the product with
 * inverse(P V) and the divide by w.  camera_host: host float[TS_EXTRACT_CAMERA_FLOATS] = {inverse(P V) row-major,
 * camera position xyz, P22, P23}.  p_world / dirs float32 [m,3] <- the point and normalize(point - position) (eps
 * 1e-12); valid int32 [m] <- 1, or 0 for depth <= 0, a non-finite depth or result: then p_world = anchor[0..2] (a
 * device float[3], the first mean: its neighbours are found at once) and dirs = 0, so everything downstream stays finite.  TS_E_BADARG: m < 1, H or W < 1, H * W >= 2^31, an unknown
 * convention, a NULL pointer, a non-finite camera value.
 * ts_extract_samples: nearest int32 [m] (the k = 1 search of p_world among the means) -> p_std [m] <-
 * p_std_table[nearest], samples float32 [m, steps, 3] <- p_world + (linspace(-e, e, steps)[s] * p_std) * dirs
 * (torch's float32 linspace).  TS_E_BADARG: n < 1, m < 1, steps outside 2..TS_EXTRACT_MAX_STEPS, m * steps >= 2^31,
 * extent_sigmas not positive and finite, a NULL pointer.
 * ts_extract_march: knn int32 [m * steps, TS_EXTRACT_K] (the samples' neighbours, 64-byte aligned rows) -> per ray
 * first int32 <- the first sample with d > level (0 if none), keep int32 <- valid && d[0] < level && first >= 1,
 * t float32 <- the linear interpolation of the level between samples first - 1 and first, points float32 [m,3] <-
 * p_world + t * dirs (t and points 0 where keep is 0); density: NULL, or float32 [m, steps] <- d.  d = sum over the
 * neighbours of sigmoid(o) exp(-clamp(q, 0, 1e8) / 2), q = |U (p - mu)|^2 (a q that is NaN - an infinite entry of U
 * from an extreme scale times a zero offset - counts as 1e8: no contribution; the reference gives NaN there), values
 * above 1 set to 1.  A wave handles
 * floor(64 / steps) rays.  TS_E_BADARG: as ts_extract_samples, a non-finite level, a NULL pointer (density may be).
 * ts_extract_normals: points float32 [m,3] with their own neighbours knn int32 [m, TS_EXTRACT_K] -> normals float32
 * [m,3] <- -grad d / |grad d| (the analytic gradient of d above; 0 where d was clamped to 1 or the gradient is 0).
 * TS_E_BADARG: n < 1, m < 1, a NULL pointer.
 * ts_extract_chunk_bytes: the bytes of one chunk of `rays` rays: ts_knn's workspace for rays * steps queries, then
 * 256-byte aligned p_world, dirs, points (12 B per ray), seven 4-byte per-ray arrays, the samples and the k-NN
 * distance and index outputs.  TS_E_BADARG: n < TS_EXTRACT_K, rays < 1, steps out of range, rays * steps >= 2^31. */
#define TS_EXTRACT_K 16
#define TS_EXTRACT_RECORD 10
#define TS_EXTRACT_MAX_STEPS 64
#define TS_EXTRACT_CAMERA_FLOATS 21
#define TS_EXTRACT_PIX_REFERENCE 0
#define TS_EXTRACT_PIX_SCREEN 1
int ts_extract_pack(int32_t n, const float* means, const float* scales, const float* quats, const float* opacities,
                    float* records, float* p_std, void* stream);
int ts_extract_rays(int32_t m, const int64_t* pixel_ids, int32_t height, int32_t width, const float* depth,
                    int32_t convention, const float* camera_host, const float* anchor, float* p_world, float* dirs,
                    int32_t* valid, void* stream);
int ts_extract_samples(int32_t n, int32_t m, int32_t steps, float extent_sigmas, const float* p_world, const float* dirs,
                       const int32_t* nearest, const float* p_std_table, float* p_std, float* samples, void* stream);
int ts_extract_march(int32_t n, int32_t m, int32_t steps, float extent_sigmas, float level, const float* samples,
                     const int32_t* knn, const float* records, const float* p_world, const float* dirs,
                     const float* p_std, const int32_t* valid, int32_t* keep, int32_t* first, float* t, float* points,
                     float* density, void* stream);
int ts_extract_normals(int32_t n, int32_t m, const float* points, const int32_t* knn, const float* records,
                       float* normals, void* stream);
int64_t ts_extract_chunk_bytes(int32_t n, int32_t rays, int32_t steps);

/* Sparse-grid iso-surface mesh of the same density (marching tetrahedra; DESIGN.md section 6g, csrc/mesh_cells.h).
 * Additive entries: the ABI version is unchanged.  None allocates or synchronises; all are deterministic (plain
 * stores).  The grid: grid_host = host float[4] {lo x y z, cell edge h > 0}, cells_host = host int32[3], the cells per
 * axis (>= 1; (nx + 1)(ny + 1)(nz + 1) * 8 must fit int64).  Corner (i, j, k) sits at lo + (i, j, k) * h (float32, product
 * and sum rounded separately) and has the id (k (ny + 1) + j)(nx + 1) + i; bricks are 8^3 cells, brick (bx, by, bz) has
 * the id (bz nby + by) nbx + bx with nb = ceil(n / 8); a brick has 9^3 = TS_MESH_BRICK_CORNERS corners, x fastest.
 * ts_mesh_boxes: boxes float32 [n,6] <- {lo xyz, hi xyz} = mean -+ extent_sigmas * sqrt(Sigma_aa), Sigma = R diag(exp(2 s))
 * R^T in double, rounded outwards.  TS_E_BADARG: n < 1, extent_sigmas not positive and finite, a NULL pointer.
 * ts_mesh_mark: flags uint8 [number of bricks] (zeroed by the caller) <- 1 for every brick holding a cell with a corner
 * inside a Gaussian's box.  TS_E_BADARG: n < 1, a bad grid, a NULL pointer.
 * ts_mesh_chunk_bytes: the bytes of one chunk of `bricks` bricks: ts_knn's workspace for bricks * 729 queries, then
 * 256-byte aligned corner positions, k-NN distances and indices, densities, and per brick a count (int32), an offset
 * (int64) and a k-NN stats pair (int32[2]).  TS_E_BADARG: n < TS_EXTRACT_K, bricks < 1 or bricks * 729 * 16 >= 2^31.
 * ts_mesh_corners: corners float32 [bricks * 729, 3] <- the positions of the listed bricks' corners (brick_ids int64
 * [bricks]); a corner beyond the grid's last cell takes the last corner's coordinate on that axis.
 * ts_mesh_density: density float32 [bricks * 729] <- d of ts_extract_march at every corner over its neighbours knn
 * int32 [bricks * 729, TS_EXTRACT_K]; 0 at a corner beyond the grid's last cell.  TS_E_BADARG: also n < TS_EXTRACT_K.
 * ts_mesh_count: counts int32 [bricks] <- the triangles of every brick (a corner is above when d > level).
 * ts_mesh_emit: with offsets int64 [bricks] (the exclusive prefix sums of counts): keys int64 [T,3] <- per triangle
 * vertex the edge key id(lower corner) * 8 + direction (1..7: bit 0 x, bit 1 y, bit 2 z), positions float32 [T,3,3] <-
 * the vertex, interpolated from the lower corner to the higher; cells: NULL, or int64 [T] <- the triangle's cell
 * (k ny + j) nx + i.  Triangles in (brick, cell, tetrahedron, triangle) order, wound so that the normal points towards
 * falling density.  count / emit run one workgroup of 512 threads per brick.  TS_E_BADARG (all four): bricks out of
 * range, a bad grid, a non-finite level, a NULL pointer (cells may be). */
#define TS_MESH_BRICK_CORNERS 729
int ts_mesh_boxes(int32_t n, const float* means, const float* scales, const float* quats, float extent_sigmas,
                  float* boxes, void* stream);
int ts_mesh_mark(int32_t n, const float* boxes, const float* grid_host, const int32_t* cells_host, uint8_t* flags,
                 void* stream);
int64_t ts_mesh_chunk_bytes(int32_t n, int32_t bricks);
int ts_mesh_corners(int32_t bricks, const int64_t* brick_ids, const float* grid_host, const int32_t* cells_host,
                    float* corners, void* stream);
int ts_mesh_density(int32_t n, int32_t bricks, const int64_t* brick_ids, const float* grid_host,
                    const int32_t* cells_host, const float* corners, const int32_t* knn, const float* records,
                    float* density, void* stream);
int ts_mesh_count(int32_t bricks, const int64_t* brick_ids, const float* grid_host, const int32_t* cells_host,
                  float level, const float* density, int32_t* counts, void* stream);
int ts_mesh_emit(int32_t bricks, const int64_t* brick_ids, const float* grid_host, const int32_t* cells_host,
                 float level, const float* density, const int64_t* offsets, int64_t* keys, float* positions,
                 int64_t* cells, void* stream);

/* Truncated signed distance fusion of depth maps on the same brick grid (csrc/tsdf_math.h).
 * Additive entries: the ABI version is unchanged.  None allocates or synchronises; all are deterministic (plain
 * stores, no atomics).  camera_table: device memory, `cameras` records of struct ts_tsdf_camera (csrc/tsdf_math.h,
 * ts_tsdf_camera_bytes() bytes each, 8-byte aligned): the view matrix's 3 x 4 top, rows 0, 1 and 3 of proj @ view, six
 * culling planes {n xyz, d, |n|}, width, height and the device pointer of the float32 [height, width] map of view-space
 * z (not finite or <= 0: no depth).  trunc > 0 in world units; depth_max > 0 (+inf: no limit).
 * ts_tsdf_mark: flags uint8 [number of bricks] (zeroed by the caller) <- 1 for every brick that touches the box of a
 * pixel's frustum piece (its four corner rays at the depths d and d + trunc, in double), widened by one cell edge;
 * max_pixels: the largest width * height of the table.  TS_E_BADARG: cameras outside 1..65535, max_pixels outside
 * 1..2^31 - 1, a bad grid, trunc or depth_max, a NULL pointer.
 * ts_tsdf_chunk_bytes: the bytes of one chunk of `bricks` bricks: 256-byte aligned sums (double), counts (int32) and
 * field (float32) of bricks * 729 corners, and per brick a triangle count (int32) and an offset (int64).  TS_E_BADARG:
 * bricks < 1 or bricks * 729 >= 2^31.
 * ts_tsdf_integrate: sum double [bricks * 729] and count int32 [bricks * 729] (zeroed by the caller before the first
 * batch) += the observations min(1, (d - z) / trunc) of the cameras [c0, c1) of the table at every corner of the listed
 * bricks, in the table's order; a corner beyond the grid's last cell observes nothing.  One workgroup of 256 threads per
 * brick; flags: TS_TSDF_NO_CULL projects every corner for every camera instead of testing the brick's bounding sphere
 * against the camera first (the same result).  c0 == c1: returns 0, launches nothing.  TS_E_BADARG: bricks out of range,
 * a bad grid, c0 < 0, c1 < c0, a bad trunc, znear or depth_max, an unknown flag, a NULL or misaligned pointer.
 * ts_tsdf_field: field float32 [bricks * 729] <- -(float)(sum / count), NaN where count < min_observations (>= 1).
 * ts_mesh_count_observed, ts_mesh_emit_observed: ts_mesh_count and ts_mesh_emit over a field that may hold NaN: a cell
 * with a NaN corner emits nothing; everything else as there. */
#define TS_TSDF_NO_CULL 1
int32_t ts_tsdf_camera_bytes(void);
int ts_tsdf_mark(int32_t cameras, const void* camera_table, int64_t max_pixels, const float* grid_host,
                 const int32_t* cells_host, float trunc, float depth_max, uint8_t* flags, void* stream);
int64_t ts_tsdf_chunk_bytes(int32_t bricks);
int ts_tsdf_integrate(int32_t bricks, const int64_t* brick_ids, const float* grid_host, const int32_t* cells_host,
                      const void* camera_table, int32_t c0, int32_t c1, float trunc, float znear, float depth_max,
                      int32_t flags, double* sum, int32_t* count, void* stream);
int ts_tsdf_field(int32_t bricks, const double* sum, const int32_t* count, int32_t min_observations, float* field,
                  void* stream);
int ts_mesh_count_observed(int32_t bricks, const int64_t* brick_ids, const float* grid_host, const int32_t* cells_host,
                           float level, const float* field, int32_t* counts, void* stream);
int ts_mesh_emit_observed(int32_t bricks, const int64_t* brick_ids, const float* grid_host, const int32_t* cells_host,
                          float level, const float* field, const int64_t* offsets, int64_t* keys, float* positions,
                          int64_t* cells, void* stream);

/* The colour of points of the same density field from the Gaussians' spherical harmonics.  An
 * additive entry: the ABI version is unchanged.  points float32 [m,3] with their own neighbours knn int32
 * [m, TS_EXTRACT_K] (ts_knn's: ascending in distance), normals float32 [m,3] (unit, outward) or NULL, records as
 * ts_extract_pack wrote them, colors_dc float32 [n,3], colors_rest float32 [n, k_rest, 3] (may be NULL at degree 0) ->
 * colors float32 [m,3] <- min(sum_j w_j c_j / sum_j w_j, 1) over the neighbours, w_j the neighbour's term of d above,
 * c_j = max(sum_k Y_k(-normal) coeffs[j, k, :] + 0.5, 0) over the bands <= degree.  Only band 0 where the normal is
 * zero, not finite or absent; a neighbour outside [0, n) has weight 0 and colour 0; where sum_j w_j is not positive
 * and finite, the colour c_j of the first listed neighbour.  One 16-lane row per point, a fixed reduction order:
 * a point's colour does not depend on m or on its place in the call.  m == 0: returns 0, launches nothing.
 * TS_E_BADARG: n < 1, m < 0, k_rest < 0, a NULL pointer with m > 0; TS_E_DEGREE: degree outside 0..3 or
 * (degree + 1)^2 > k_rest + 1. */
int ts_field_colors(int32_t n, int32_t m, const float* points, const float* normals, const int32_t* knn,
                    const float* records, const float* colors_dc, const float* colors_rest, int32_t k_rest,
                    int32_t degree, float* colors, void* stream);

/* Triangle-budget simplification of a mesh by vertex clustering with quadric-optimal representatives (DESIGN.md section
 * 6i, csrc/simplify_math.h).  Additive entries: the ABI version is unchanged.  None allocates or synchronises; all are
 * deterministic (plain stores, no atomics).  vertices float32 [v,3], faces int32 [f,3] with every index in [0, v) (the
 * caller's duty: the kernels gather through them unchecked).  The grid: grid_host = host float[4] {lo x y z, cell edge
 * c > 0}, cells_host = host int32[3], the cells per axis (>= 1; nx ny nz must stay below 4.6e18).  A coordinate's cell
 * is min(floor((p - lo) / c), n - 1) (float32, difference and quotient rounded separately; 0 below lo), a vertex's key
 * the int64 (iz ny + iy) nx + ix, a cell's centre lo + (i + 0.5) c in double.
 * ts_simplify_count: block_counts int32 [ceil(f / 256)] <- per workgroup of 256 faces, the faces whose three corner keys
 * are pairwise distinct.  f == 0: returns 0, launches nothing.  TS_E_BADARG: v < 0, f < 0, a bad grid; with f > 0 also
 * v < 1 or a NULL pointer.
 * ts_simplify_keys: keys int64 [v] <- every vertex's key.  v == 0: returns 0, launches nothing.  TS_E_BADARG: v < 0, a
 * bad grid, a NULL pointer with v > 0.
 * ts_simplify_accumulate: sums over the entries of one cluster, in double.  what = TS_SIMPLIFY_FACE_CORNERS: the
 * entries are the 3 f face corners (entry = face * 3 + corner) and sums is double [clusters, TS_SIMPLIFY_QUADRIC]: per
 * corner, with g the centre of the corner's cell, n = (b - a) x (c - a) and d = -n . (a - g) of its face (a, b, c), the
 * ten numbers n n^T (xx xy xz yy yz zz), n d, d^2.  what = TS_SIMPLIFY_VERTICES: the entries are the v vertices and sums
 * is double [clusters, TS_SIMPLIFY_VSUM]: p - g and 1.  clusters_sorted int32 [entries] ascending and order int64
 * [entries] (the entry at each sorted place) are a stable sort of the entries' clusters.  Chunks of TS_SIMPLIFY_CHUNK
 * consecutive sorted entries are summed serially from zero; a cluster's run that crosses chunk ends is the sum, in chunk
 * order, of its parts.  One call covers the chunks [chunk0, chunk0 + chunks) with a workspace of
 * ts_simplify_ws_bytes(chunks) bytes and stores every cluster whose run starts in them; the sums of a cluster do not
 * depend on how the chunks are spread over calls.  A cluster without entries keeps what sums held (zero it first); an
 * entry whose cluster lies outside [0, clusters) is skipped.  entries == 0 or chunks == 0: returns 0, launches nothing.
 * TS_E_BADARG: a negative size, a bad grid, an unknown `what`, entries != 3 f (or v), a chunk range outside
 * [0, ceil(entries / TS_SIMPLIFY_CHUNK)]; with work to do also v < 1, clusters < 1 or a NULL pointer (faces may be NULL
 * for the vertices).
 * ts_simplify_ws_bytes: two partial rows of TS_SIMPLIFY_QUADRIC doubles and an int32 flag per chunk, 256-byte aligned.
 * TS_E_BADARG: chunks < 1 or > 2^40.
 * ts_simplify_solve: representatives float32 [clusters,3] <- float32(g + x) per cluster, cluster_keys int64 [clusters]
 * its cell's key, x = ts_simplify_representative of its sums (csrc/simplify_math.h: the mean m of p - g moved along the
 * eigen-directions of A with lambda > singular_threshold * lambda_max, cyclic Jacobi in double; m where A has no
 * positive finite eigenvalue or the result is not finite or leaves the cell).  clusters == 0: returns 0.
 * TS_E_BADARG: clusters < 0, a bad grid, singular_threshold outside (0, 1), a NULL pointer with clusters > 0.
 * ts_simplify_faces: out_faces int32 [f,3] <- vertex_cluster int32 [v] at the face's corners, rotated so that the
 * smallest comes first (the orientation stays); keep uint8 [f] <- 1 where the three differ.  f == 0: returns 0.
 * TS_E_BADARG: v < 0, f < 0; with f > 0 also v < 1 or a NULL pointer. */
#define TS_SIMPLIFY_CHUNK 128
#define TS_SIMPLIFY_QUADRIC 10
#define TS_SIMPLIFY_VSUM 4
#define TS_SIMPLIFY_FACE_CORNERS 0
#define TS_SIMPLIFY_VERTICES 1
int ts_simplify_count(int32_t v, int32_t f, const float* vertices, const int32_t* faces, const float* grid_host,
                      const int32_t* cells_host, int32_t* block_counts, void* stream);
int ts_simplify_keys(int32_t v, const float* vertices, const float* grid_host, const int32_t* cells_host, int64_t* keys,
                     void* stream);
int64_t ts_simplify_ws_bytes(int64_t chunks);
int ts_simplify_accumulate(int32_t v, int32_t f, int32_t clusters, const float* vertices, const int32_t* faces,
                           const float* grid_host, const int32_t* cells_host, int32_t what, int64_t entries,
                           const int32_t* clusters_sorted, const int64_t* order, int64_t chunk0, int64_t chunks,
                           double* sums, void* ws, void* stream);
int ts_simplify_solve(int32_t clusters, const int64_t* cluster_keys, const float* grid_host, const int32_t* cells_host,
                      const double* quadrics, const double* vertex_sums, double singular_threshold,
                      float* representatives, void* stream);
int ts_simplify_faces(int32_t v, int32_t f, const int32_t* faces, const int32_t* vertex_cluster, int32_t* out_faces,
                      uint8_t* keep, void* stream);

/* Mesh clean-up: the faces at edges of valence above two, and the connected components (DESIGN.md section 6j,
 * csrc/clean_math.h).  Additive entries: the ABI version is unchanged.  None allocates or synchronises; all are integer
 * work (the face weights: fixed IEEE operations in double) and give the same bits on every run.  vertices float32 [v,3],
 * faces int32 [f,3]; no entry reads or writes memory at an index a face names without checking it against v.
 * ts_clean_degenerate: flags uint8 [f] <- 1 where two of the face's indices are equal, else 0.  f == 0: returns 0,
 * launches nothing.  TS_E_BADARG: f < 0, a NULL pointer with f > 0.
 * ts_clean_edge_keys: keys int64 [3 f] <- entry 3 face + k: min(a, b) v + max(a, b) of the edge from corner k to corner
 * (k + 1) % 3.  f == 0: returns 0.  TS_E_BADARG: v < 0, f < 0; with f > 0 also v < 1 or a NULL pointer.
 * ts_clean_face_weights: weights double [f] <- A2 = (n_x n_x + n_y n_y) + n_z n_z, n = (b - a) x (c - a) in double from
 * the float32 positions, uncontracted (0 for a face with an index outside [0, v)).  f == 0: returns 0.  TS_E_BADARG as
 * ts_clean_edge_keys.
 * ts_clean_mark: sorted_keys int64 [entries] and order int64 [entries] (the entry at each sorted place) are the edge
 * list sorted by (key, weight descending, face); marks uint8 [f] (zero it first) <- 1, by plain byte stores, for the face
 * order[i] / 3 of every place i >= 2 with sorted_keys[i] == sorted_keys[i - 2]: the faces of rank two and above at an
 * edge.  f == 0: returns 0.  TS_E_BADARG: f < 0, entries != 3 f, a NULL pointer with f > 0.
 * ts_clean_components: labels int32 [v] <- the smallest vertex index of the vertex's connected component, two vertices
 * being connected when a face holds both (a vertex in no face: itself; a face with an index outside [0, v) joins
 * nothing).  parent int32 [v] is scratch: the union-find forest (set to the identity here; afterwards parent[x] <= x
 * and lies in x's component).  Three launches: identity, one thread per face joining (a, b) and (b, c) with integer
 * compare-and-swap at agent scope, the roots.  v == 0 (and f == 0): returns 0, launches nothing; f == 0: every vertex
 * its own label.  TS_E_BADARG: v < 0, f < 0, f > 0 with v < 1, a NULL parent or labels with v > 0, NULL faces with
 * f > 0. */
int ts_clean_degenerate(int32_t f, const int32_t* faces, uint8_t* flags, void* stream);
int ts_clean_edge_keys(int32_t v, int32_t f, const int32_t* faces, int64_t* keys, void* stream);
int ts_clean_face_weights(int32_t v, int32_t f, const float* vertices, const int32_t* faces, double* weights,
                          void* stream);
int ts_clean_mark(int32_t f, int64_t entries, const int64_t* sorted_keys, const int64_t* order, uint8_t* marks,
                  void* stream);
int ts_clean_components(int32_t v, int32_t f, const int32_t* faces, int32_t* parent, int32_t* labels, void* stream);

/* The 32-byte .splat record (csrc/splat_record.h): x y z float32 | exp(scales) float32 x 3 |
 * r g b a uint8 | rotation w x y z uint8.  Additive entries: the ABI version is unchanged.  None allocates or
 * synchronises; one thread per record, no atomics.  means, scales, colors_dc float32 [n,3], opacities float32 [n],
 * quats float32 [n,4]; records: 32 m bytes, 16-byte aligned.
 * ts_splat_keys: keys float32 [n] <- exp((s0 + s1) + s2) sigmoid(opacity).  n == 0: returns 0, launches nothing.
 * TS_E_BADARG: n < 0, a NULL pointer with n > 0.
 * ts_splat_pack: record i of m <- the encoding of Gaussian order[i] (int64 [m]), or of Gaussian i where order is NULL; an
 * order[i] outside [0, n) reads nothing and gives a record of zeros.  m == 0: returns 0.  TS_E_BADARG: n < 0, m < 0,
 * m > n without an order; with m > 0 also a NULL pointer (order may be) or records not 16-byte aligned.
 * ts_splat_unpack: the five tensors' rows <- the decoding of n records.  n == 0: returns 0.  TS_E_BADARG: n < 0; with
 * n > 0 a NULL pointer or records not 16-byte aligned. */
int ts_splat_keys(int32_t n, const float* scales, const float* opacities, float* keys, void* stream);
int ts_splat_pack(int32_t n, int32_t m, const float* means, const float* scales, const float* colors_dc,
                  const float* opacities, const float* quats, const int64_t* order, void* records, void* stream);
int ts_splat_unpack(int32_t n, const void* records, float* means, float* scales, float* colors_dc, float* opacities,
                    float* quats, void* stream);

/* Image undistortion and resampling (csrc/undistort_math.h).  An additive entry: the ABI version
 * is unchanged.  It neither allocates nor synchronises; one thread per 4 output pixels, no atomics, the same bits on
 * every run.
 * ts_undistort_image: src uint8 [src_h, src_w, 3] on the device; src_k and dst_k (fx fy cx cy, in pixel indices: the
 * first pixel's centre is 0) and dist (k1 k2 p1 p2 k3 k4 k5 k6) are float32 arrays in HOST memory, read before the call
 * returns.  Output pixel (u, v) is the mean of n x n bilinear samples of the source at the distorted positions of
 * (u, v) + ((a + 0.5) / n - 0.5, (b + 0.5) / n - 0.5), n = min(8, ceil(max(src_w / out_w, src_h / out_h))), source
 * positions clamped to the frame.  out (16-byte aligned, on the device): uint8 [out_h, out_w, 3], the mean rounded half
 * to even, or with out_float != 0 float32 [out_h, out_w, 3], the unrounded mean / 255.  TS_E_BADARG, before any launch:
 * a NULL pointer, a size below 1, src_h src_w or out_h out_w of 2^31 or more, out not 16-byte aligned. */
int ts_undistort_image(const uint8_t* src, int32_t src_h, int32_t src_w, const float* src_k, const float* dst_k,
                       const float* dist, int32_t out_h, int32_t out_w, int32_t out_float, void* out, void* stream);

/* Baseline JPEG of a device image (csrc/jpeg_math.h).  Additive entries: the ABI version is
 * unchanged.  subsampling: 0 = 4:4:4, 1 = 4:2:0; restart_interval in MCUs, 1..65535, or 0 for one MCU row.  All four return
 * TS_E_BADARG, before any launch, for a width or height outside 1..65535, an unknown subsampling, an interval outside
 * 0..65535, or an image of so many blocks that the scan's bits leave 31 bits.
 * ts_jpeg_ws_bytes: the bytes of `workspace`.  ts_jpeg_max_bytes: the largest file of this shape (every block at its
 * longest, every byte stuffed).  ts_jpeg_header: host only, no device is touched: the file's bytes up to the entropy-coded
 * data (629 of them) to `out` in host memory -> their number; TS_E_BADARG also for a quality outside 1..100 or a capacity
 * below 629.
 * ts_jpeg_encode: image on the device, dtype 0 = uint8 [height, width, 3] (pixel_stride 3) or 1 = float32 with a pixel
 * stride of 3 or 4 floats, whose samples become rint(clamp(255 x, 0, 255)); workspace: >= ts_jpeg_ws_bytes bytes, 256-byte
 * aligned; out: device bytes, out_capacity >= ts_jpeg_max_bytes (TS_E_BADARG otherwise: the kernels do not check);
 * size_word: a device int32 <- the file's size; coefficients: NULL, or device int16 [blocks, 64] <- the quantised
 * coefficients in zigzag order, blocks in scan order.  It neither allocates nor synchronises; the same bytes on every run.
 * TS_E_BADARG also for a quality outside 1..100, another dtype or stride, a NULL pointer. */
int64_t ts_jpeg_ws_bytes(int32_t width, int32_t height, int32_t subsampling, int32_t restart_interval);
int64_t ts_jpeg_max_bytes(int32_t width, int32_t height, int32_t subsampling, int32_t restart_interval);
int64_t ts_jpeg_header(int32_t width, int32_t height, int32_t quality, int32_t subsampling, int32_t restart_interval,
                       uint8_t* out, int64_t out_capacity);
int ts_jpeg_encode(const void* image, int32_t dtype, int32_t pixel_stride, int32_t width, int32_t height, int32_t quality,
                   int32_t subsampling, int32_t restart_interval, void* workspace, uint8_t* out, int64_t out_capacity,
                   int32_t* size_word, int16_t* coefficients, void* stream);

/* The quality of one image against one target (csrc/metrics_math.h).  Additive entries: the ABI
 * version is unchanged.
 * image: float32 [height, width, pixel_floats], pixel_floats 3 or 4 (channel 3, the compositing kernels' depth, is never
 * read); target: [height, width, 3], float32 or, with target_is_u8 != 0, uint8 whose byte b stands for the float32
 * quotient b / 255.0f - both targets of the same values give the same 32 bytes of output.  Byte rows need no alignment.
 * out4 <- four device doubles {mse, l1, ssim, psnr}: the means of (x - y)^2 and |x - y| over the 3 H W elements (each
 * difference one float32 subtraction, everything after it double), the SSIM of the training loss
 * (pytorch_msssim.SSIM(data_range=1, size_average=True, channel=3): 11-tap sigma-1.5 window, valid filtering, K = (0.01,
 * 0.03), mean over 3 (H-10)(W-10) - NOT the zero-padded SSIM of the 3DGS papers' tables), and -10 log10(mse), +inf
 * where mse == 0.  Two launches, no allocation, no synchronisation, no atomics; the workspace size and the order of
 * every sum depend on (height, width) alone, so the same inputs give the same bytes on every run and device.
 * ws: >= ts_image_metrics_ws_bytes bytes (24 per wave of the first launch; 0 where height or width <= 10), and like out4
 * 8-byte aligned.  TS_E_BADARG, before any launch: height or width <= 10, pixel_floats not 3 or 4, a NULL or misaligned
 * pointer. */
int64_t ts_image_metrics_ws_bytes(int32_t height, int32_t width);
int ts_image_metrics(int32_t height, int32_t width, int32_t pixel_floats, const float* image, const void* target,
                     int32_t target_is_u8, void* ws, double* out4, void* stream);
/* The same four values over the pixels a mask keeps: mask uint8 [height, width], m = b / 255.0f,
 *   mse = sum m (x - y)^2 / (3 sum m),  l1 = sum m |x - y| / (3 sum m),  ssim = sum m_c S(x', y) / (3 sum m_c),
 * m_c the weight of the window's centre pixel, x' the substituted image of the masked loss; psnr from mse.  A mask
 * that keeps nothing gives NaN.  An all-255 mask gives ts_image_metrics' bytes.  ws: >= ts_image_metrics_masked_ws_bytes
 * bytes (40 per wave).  TS_E_BADARG as ts_image_metrics, and for a NULL mask. */
int64_t ts_image_metrics_masked_ws_bytes(int32_t height, int32_t width);
int ts_image_metrics_masked(int32_t height, int32_t width, int32_t pixel_floats, const float* image, const void* target,
                            int32_t target_is_u8, const uint8_t* mask, void* ws, double* out4, void* stream);

/* Depth priors: stored dense depth maps scale-matched to the SfM points (csrc/depth_prior_math.h:
 * the arithmetic, the key's layout, the fit's row and its status codes).  Additive entries: the ABI version is unchanged.
 * None allocates or synchronises; no atomics, the same bytes on every run.  All pointers are device pointers.
 * ts_depth_prior_project: `cameras` <= 2^15 cameras whose visible points are spans of one list: offsets int64
 * [cameras + 1], ascending from 0 to n, a span of at most 2^20 entries; indices int64 [n] into xyz float32 [points, 3] and
 * errors float64 [points] (an index outside 0 .. points - 1 is a dropped point); cam_f float32 [cameras, 14]: the view
 * matrix's 3 x 4 top row-major, f_x, f_y; cam_size int32 [cameras, 2]: width, height, width x height < 2^28 - 1.
 * -> keys int64 [n], z float32 [n], w float64 [n] = 1 / error (0 for a dropped point).
 * ts_depth_prior_mark: the keys sorted ascending -> flags int64 [n], 1 at the last entry of every (camera, pixel) run.
 * ts_depth_prior_gather: order int64 [n]: the sort's permutation; running int64 [n]: the inclusive sums of flags; maps:
 * NULL, or int64 [cameras]: the device address of every camera's float32 dense map (0: none, x = NaN) of map_size int32
 * [cameras, 2] = rows, columns.  Survivor number j (0-based, in sorted order) -> pixel int32 [j] = py W + px, z [j],
 * w [j] and, with maps, x float32 [j]: the map sampled at the pixel.  The outputs hold n entries.
 * ts_depth_prior_fit: one fit per span of offsets int64 [cameras + 1] over x, z float32 and w float64; with disparity != 0
 * y = 1 / z, else y = z.  fits float64 [cameras, 6] <- {s, t, f(s, t), m, evaluations, status}.
 * ts_depth_prior_apply: out float32 [height, width] (16-byte aligned) <- float32(s sample + t), or its reciprocal with
 * disparity != 0, of the map float32 [map_h, map_w] sampled at every pixel; fit: the device address of a fit's row.
 * TS_E_BADARG, before any launch: a negative count, a NULL or misaligned pointer, a size out of range. */
int ts_depth_prior_project(int32_t cameras, int64_t n, int64_t points, const int64_t* offsets, const int64_t* indices,
                           const float* xyz, const double* errors, const float* cam_f, const int32_t* cam_size,
                           int64_t* keys, float* z, double* w, void* stream);
int ts_depth_prior_mark(int64_t n, const int64_t* sorted_keys, int64_t* flags, void* stream);
int ts_depth_prior_gather(int64_t n, const int64_t* sorted_keys, const int64_t* order, const int64_t* flags,
                          const int64_t* running, const float* z_in, const double* w_in, const int64_t* maps,
                          const int32_t* map_size, const int32_t* cam_size, int32_t* pixel, float* z, double* w, float* x,
                          void* stream);
int ts_depth_prior_fit(int32_t cameras, const int64_t* offsets, const float* x, const float* z, const double* w,
                       int32_t disparity, double* fits, void* stream);
int ts_depth_prior_apply(const float* map, int32_t map_h, int32_t map_w, int32_t height, int32_t width, const double* fit,
                         int32_t disparity, float* out, void* stream);

/* Label votes: which class every Gaussian belongs to, from per-view label maps (DESIGN.md section 6q,
 * csrc/vote_math.h).  Additive entries: the ABI version is unchanged.  Neither allocates or synchronises.
 * ts_label_votes: one view.  cam, tile_bins, gaussian_ids_sorted, splats: the 16x16 lists and 48-byte records of the
 * forward compositing launch (ts_sort_tiles, ts_pack_splats); the colours of the records are not read.  labels: uint8
 * [img_height, img_width] with class_map uint8 [256] (both device pointers, both or neither): a pixel of label l votes
 * in column class_map[l], or not at all where that is 255 (or >= num_classes).  Without them every pixel of the image
 * votes in column 0.  votes int64 [n, num_classes], n > every listed id, is ACCUMULATED into:
 *   votes[g, c] += sum over the pixels p of column c of rint(2^24 vis_g(p))
 * with vis_g(p) the float32 weight ts_raster_fwd blends g into p with, bit for bit.  Integer atomics only: the same
 * bytes whatever the order of tiles, views and calls.  flags: 0.  TS_E_BADARG, before any launch: flags != 0, a NULL
 * cam, cam->wide_tiles != 0, num_classes outside 1..255, one of labels / class_map without the other, an image size
 * < 1 or tile bounds that are not the image's, and (where the camera has tiles) a NULL tile_bins,
 * gaussian_ids_sorted, splats or votes.
 * ts_votes_labels: labels_out uint8 [n] <- the first largest column of every row where the row's sum is positive and
 * double(top) >= min_share * double(sum), else 255; confidence_out float32 [n] (may be NULL) <- float32(double(top) /
 * double(sum)), 0 for an empty row.  n == 0: returns 0, launches nothing.  TS_E_BADARG: n < 0, num_classes outside
 * 1..255, a NaN min_share, a NULL votes or labels_out with n > 0. */
int ts_label_votes(int32_t flags, const ts_camera* cam_host, const int32_t* tile_bins, const int32_t* gaussian_ids_sorted,
                   const float* splats, const uint8_t* labels, const uint8_t* class_map, int32_t num_classes,
                   int64_t* votes, void* stream);
int ts_votes_labels(int32_t n, int32_t num_classes, const int64_t* votes, double min_share, uint8_t* labels_out,
                    float* confidence_out, void* stream);

/* Budgeted (MCMC) densification: relocation of dead Gaussians, growth to a cap, position noise and the two mean
 * regularisers (csrc/mcmc_math.h).  Additive entries: the ABI version is unchanged.  None allocates
 * or synchronises; every result is the same bits on every run.  All return TS_E_BADARG, before any launch, for a count
 * below 1 or a NULL pointer that is not said to be optional.
 * ts_mcmc_noise: means float32 [n,3] += scale * g(1 - o) * (Sigma z) with o = sigmoid(opacities), g(x) = 1 / (1 + exp(-100
 * (x - 0.995))) and Sigma = R diag(exp(2 scales)) R^T of the normalised quats (w, x, y, z), all float32; a row whose g is
 * 0 (the exponent overflowed) or NaN keeps its bits.  z: float32 [n,3] unit normals, or NULL: row i then draws its own
 * from Philox4x32-10 with key = seed and counter (i, step, 0, 0), the words mapped to u = ((x >> 8) + 0.5) 2^-24 and
 * Box-Muller applied to (u0, u1) and (u2, u3), of which the first three normals are used.  quats must be 16-byte aligned.
 * ts_mcmc_normals: out float32 [n,3] <- exactly the normals ts_mcmc_noise draws for (seed, step).
 * ts_mcmc_mean: value (device float) <- mean f(x) over count float32 elements, and grad float32 [count] (may be NULL) <-
 * f'(x) / count; kind TS_MCMC_MEAN_SIGMOID: f = sigmoid, TS_MCMC_MEAN_EXP: f = exp.  The sum is taken in double in a fixed
 * order.  ws: >= ts_mcmc_mean_ws_bytes(count) bytes, 8-byte aligned.
 * ts_mcmc_weights: weights double [n] <- o_i, the float32 nearest to sigmoid(opacities_i) (evaluated in double), or 0
 * where o_i is 0 or NaN and, with zero_dead != 0, where row i is dead (not o_i > min_opacity).  flags uint8 [n] (may be
 * NULL) <- 0 for a dead row and TS_DENSIFY_PRUNE for a live one: ts_densify_plan then lists the dead rows in ascending
 * order as its kept rows, with their number in counts[0].  TS_E_BADARG also for a negative or NaN min_opacity.
 * ts_mcmc_sample_rows: m draws over n rows.  P = the inclusive prefix of weights in double, in the fixed order
 * ts_density_sample uses; draw j picks the first row with P_i > (double)uniforms[j] * P_{n-1} (uniforms float32 [m] in
 * [0,1)) by bisection, and from a row of weight 0 moves to the nearest earlier row of positive weight, else the nearest
 * later one; -1 when every weight is 0.  picks int32 [m] <- the rows; counts int32 [n] <- how many draws picked each row
 * (zeroed here, integer atomics).  ws: >= ts_mcmc_sample_ws_bytes(n) bytes, 256-byte aligned.
 * ts_mcmc_rewrite: every row with counts[i] > 0 is rewritten in place from its old values: M = min(counts[i] + 1,
 * TS_MCMC_N_MAX), o' = 1 - (1 - o)^(1/M), D = sum_{a=1..M} sum_{k<a} C(a-1,k) (-1)^k o'^(k+1) / sqrt(k+1) (both in
 * double, each rounded to float32 once), opacities[i] <- logit(clamp(o', min_opacity, 1 - 2^-23)), scales[i, :] += log(o /
 * D); and row i of the num_tensors (0..TS_GATHER_MAX_TENSORS) moment pairs exp_avg / exp_avg_sq (HOST tables of device
 * pointers, row_floats_host[k] floats per row) is set to zero.  Other rows are not touched.
 * ts_mcmc_copy_rows: for j < m and every tensor k: params[k][dst_rows[j], :] <- params[k][src_rows[j], :] and, where the
 * tables are given (both or neither), both moments of row dst_rows[j] <- 0.  Rows are in [0, n); a pair with a row
 * outside is skipped.  No row may be both a destination and a source. */
#define TS_MCMC_N_MAX 51
#define TS_MCMC_MEAN_SIGMOID 0
#define TS_MCMC_MEAN_EXP 1
int ts_mcmc_noise(int32_t n, float* means, const float* scales, const float* quats, const float* opacities, float scale,
                  const float* z, uint64_t seed, uint32_t step, void* stream);
int ts_mcmc_normals(int32_t n, uint64_t seed, uint32_t step, float* out, void* stream);
int64_t ts_mcmc_mean_ws_bytes(int64_t count);
int ts_mcmc_mean(int32_t kind, int64_t count, const float* x, float* value, float* grad, void* ws, void* stream);
int ts_mcmc_weights(int32_t n, const float* opacities, float min_opacity, int32_t zero_dead, double* weights,
                    uint8_t* flags, void* stream);
int64_t ts_mcmc_sample_ws_bytes(int32_t n);
int ts_mcmc_sample_rows(int32_t n, int32_t m, const double* weights, const float* uniforms, int32_t* picks,
                        int32_t* counts, void* ws, void* stream);
int ts_mcmc_rewrite(int32_t n, const int32_t* counts, float min_opacity, float* opacities, float* scales,
                    int32_t num_tensors, float* const* exp_avg_host, float* const* exp_avg_sq_host,
                    const int32_t* row_floats_host, void* stream);
int ts_mcmc_copy_rows(int32_t n, int32_t m, const int32_t* dst_rows, const int32_t* src_rows, int32_t num_tensors,
                      float* const* params_host, float* const* exp_avg_host, float* const* exp_avg_sq_host,
                      const int32_t* row_floats_host, void* stream);

/* ======================================= per-view appearance ================================== */
/* DESIGN.md section 6s; the arithmetic is csrc/appearance_math.h's.  image, out, v_out, v_image: float32 [height, width, 3],
 * contiguous; grid, v_grid: float32 [levels, grid_h, grid_w, 12] of one view, the grid 16-byte aligned; every size >= 1.
 * All results are the same bits on every run (no float atomics).  TS_E_BADARG for a NULL pointer or a non-positive size.
 * ts_appearance_fwd: out <- the sliced affine map of every pixel (not clamped); out may not alias image.
 * ts_appearance_bwd: v_image <- d loss / d image from v_out = d loss / d out, v_grid <- d loss / d grid (overwritten; the
 * sums in double, rounded to float32 once).  Two launches.  ws: >= ts_appearance_ws_bytes bytes, 8-byte aligned.
 * ts_grid_tv: value[0] (double) <- tv(grid), the sum over the axes of size > 1 of the mean squared difference of
 * neighbouring vertices; v_out[e] <- (v_in ? v_in[e] : 0) + weight * (float) d tv / d grid[e].  One workgroup; v_out may
 * alias v_in, not grid.
 * ts_affine_fit_sums: out22 (double) <- over all pixels, phi = (r, g, b, 1) of image and t of target (float32 or uint8
 * [height, width, 3], a byte standing for b / 255 as in ts_image_metrics): the sums rr rg rb r gg gb g bb b 1, then
 * phi_k t_c at 10 + 3 k + c.  Two launches.  ws: >= ts_affine_fit_ws_bytes bytes, 8-byte aligned like out22. */
int64_t ts_appearance_ws_bytes(int32_t height, int32_t width, int32_t levels, int32_t grid_h, int32_t grid_w);
int ts_appearance_fwd(int32_t height, int32_t width, int32_t levels, int32_t grid_h, int32_t grid_w, const float* image,
                      const float* grid, float* out, void* stream);
int ts_appearance_bwd(int32_t height, int32_t width, int32_t levels, int32_t grid_h, int32_t grid_w, const float* image,
                      const float* grid, const float* v_out, float* v_image, void* ws, float* v_grid, void* stream);
int ts_grid_tv(int32_t levels, int32_t grid_h, int32_t grid_w, const float* grid, float weight, const float* v_in,
               double* value, float* v_out, void* stream);
int64_t ts_affine_fit_ws_bytes(int32_t height, int32_t width);
int ts_affine_fit_sums(int32_t height, int32_t width, const float* image, const void* target, int32_t target_is_u8,
                       void* ws, double* out22, void* stream);

/* ========================================= scene editing ====================================== */
/* DESIGN.md section 6t; the arithmetic is csrc/transform_math.h's, plain float32 with every product and sum rounded on its
 * own, and the results are the bits of that header's host build.  The similarity x' = s R x + t arrives as host arrays that
 * are read inside the call and travel as kernel arguments: no upload, no allocation, no synchronisation.
 * ts_transform_gaussians: means_out <- M m + t, scales_out <- scales + log_scale, quats_out <- r (x) q (Hamilton product,
 * w x y z, the norm of q kept, no sign rule), colors_rest_out <- D_l c_l per stored band and colour channel; colors_dc and
 * opacities do not change and are not arguments.  xform_host: 12 floats, M = fl32(s R) row-major, then fl32(t).
 * quat_host: 4 floats, the unit quaternion r of R.  log_scale: fl32(log s).  sh_host: D_1 (9) | D_2 (25) | D_3 (49) |
 * D_4 (81), row-major, as many bands as k_rest needs (NULL where k_rest == 0); D_l is defined by sum_j Y_lj(d) D_l[j,k] =
 * Y_lk(R^T d) in the basis of ts_sh_fwd.  k_rest: 0, 3, 8, 15 or 24 coefficients per channel, colors_rest [n, k_rest, 3]
 * (may be NULL where k_rest == 0).  mask: uint8 [n] on the device or NULL; a row whose byte is 0 is copied.  Each *_out
 * pointer may equal its input pointer; any other overlap is the caller's error.  One launch, no atomics, the same bits on
 * every run.  n == 0: returns 0, launches nothing.  TS_E_BADARG before any launch: n < 0, another k_rest, a NULL required
 * pointer with n > 0, a non-finite entry in a host array.
 * ts_box_mask: inside[i] (uint8) <- 1 where |A m_i + b|_k <= 1 for k = 0, 1, 2, else 0 (a NaN mean is outside).  box_host:
 * 12 floats, A (3x3 row-major) then b; for a box of centre c, half extents h and axes R_box: A = diag(1/h) R_box^T,
 * b = -A c.  n == 0: returns 0.  TS_E_BADARG: n < 0; with n > 0 a NULL pointer or a non-finite entry of box_host. */
int ts_transform_gaussians(int32_t n, int32_t k_rest, const float* xform_host, const float* quat_host, float log_scale,
                           const float* sh_host, const uint8_t* mask, const float* means, const float* scales,
                           const float* quats, const float* colors_rest, float* means_out, float* scales_out,
                           float* quats_out, float* colors_rest_out, void* stream);
int ts_box_mask(int32_t n, const float* box_host, const float* means, uint8_t* inside, void* stream);

/* ======================================== camera pose gradient ================================ */
/* DESIGN.md section 6u; the arithmetic and the order of the sum are csrc/pose_math.h's, and the result is the bits of that
 * header's host build.  ts_pose_grad: out6 (double, device) <- (dL/dv [3], dL/domega [3]) at delta = 0 of the left
 * perturbation V(delta) = Exp(delta) V of the view matrix V = [R | t], from means [n, 3], quats [n, 4] (raw, w x y z) and
 * the gradient rows v_means [n, 3] = dL/dmeans, v_quats [n, 4] = dL/dquats of a backward pass through a frame rendered
 * with V (float32, device).  view34_host: the 12 floats of V's first three rows, row-major, on the host; read inside
 * the call and passed as a kernel argument.  R must be orthonormal for the result to be the pose gradient.  Every product
 * and sum is a double operation; the rows are added in an order that depends on n alone, without atomics: the same 48
 * bytes on every run, stream and workspace.  Two launches.  ws: >= ts_pose_ws_bytes(n) bytes (48 per 1024 rows), 8-byte
 * aligned like out6.  n == 0: out6 <- six zeros (the row pointers and ws may be NULL).  TS_E_BADARG before any launch:
 * n < 0, a NULL view34_host or out6, with n > 0 a NULL row pointer or ws, a misaligned pointer. */
int64_t ts_pose_ws_bytes(int32_t n);
int ts_pose_grad(int32_t n, const float* view34_host, const float* means, const float* quats, const float* v_means,
                 const float* v_quats, void* ws, double* out6, void* stream);

/* ============================ antialiased rendering: opacity compensation ===================== */
/* DESIGN.md section 6w; the arithmetic is csrc/antialias_math.h's, and every result is the bits of that header's host
 * build.  With (a_o, b, c_o) a Gaussian's projected covariance before the 0.3 blur of the projection and det_o, det_b
 * the determinants before and after it, comp = sqrt(max(0, det_o / det_b)); behind the clip plane and where the max
 * clamps comp = 0 and so is every derivative.  One lane per Gaussian, no atomics, no workspace.
 * ts_antialias_fwd: from means3d [n, 3], scales [n, 3] and quats [n, 4] under project_flags (TS_PROJECT_*), viewmat (12
 * floats, device) and the camera -> comp [n], o_eff [n] = opacity * comp with `opacity` [n] a logit (raster_flags =
 * TS_RASTER_LOGIT_OPACITY) or an opacity (0), and rows [n, 4] = (a_o, b, c_o, comp), 16-byte aligned, for ts_antialias_bwd.
 * Any of the three outputs may be NULL, not all; opacity may be NULL without o_eff.
 * ts_antialias_bwd: between ts_frame_bwd_composite and ts_frame_bwd_params[_adam] of a frame rendered with o_eff
 * (TS_FRAME_LINEAR_OPACITY).  For every Gaussian with radii > 0, in place: v_conic [n, 3] += the compensation's gradient
 * in v_conic's convention (true partials of the stored entries) for v_comp = v_opacity * opacity, and v_opacity [n] (on
 * entry dL/do_eff) <- dL/d(opacity argument): times comp, and through the sigmoid for a logit.  Other rows are not touched.
 * ts_compensation_bwd: v_comp [n] -> v_means3d [n, 3], v_scales [n, 3], v_quats [n, 4] (gradients of the stored tensors
 * under project_flags) through the projection's own VJP; every row is written.
 * n == 0: returns 0.  TS_E_BADARG before any launch: n < 0, a NULL camera, unknown flag bits, with n > 0 a NULL or
 * misaligned pointer. */
int ts_antialias_fwd(int32_t n, const float* means3d, const float* scales, const float* quats, const float* viewmat,
                     const ts_camera* cam_host, int32_t project_flags, const float* opacity, int32_t raster_flags,
                     float* comp, float* o_eff, float* rows, void* stream);
int ts_antialias_bwd(int32_t n, const int32_t* radii, const float* rows, const float* opacity, int32_t raster_flags,
                     float* v_opacity, float* v_conic, void* stream);
int ts_compensation_bwd(int32_t n, const float* means3d, const float* scales, const float* quats, const float* viewmat,
                        const ts_camera* cam_host, int32_t project_flags, const float* v_comp, float* v_means3d,
                        float* v_scales, float* v_quats, void* stream);

/* ======================================= measurement utility ================================== */
/* Streaming read of n_floats float32 (16-byte loads, grid-stride): the read-bandwidth microbenchmark
 * that SURVEY.md 8(d) D1 asks the roofline to be quoted against as well.  sink: >= 1 float. */
int ts_bench_stream_read(const float* src, int64_t n_floats, float* sink, void* stream);
/* Gather of m 48-byte records records[ids[j]] (three 16-byte loads per lane, the compositing kernels' access
 * pattern) on a known record count: calibrates rocprofv3's FETCH_SIZE for gathers.  sink: >= 1 float. */
int ts_bench_gather48(const float* records, const int32_t* ids, int64_t m, float* sink, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* TINYSPLAT_HIP_H */
