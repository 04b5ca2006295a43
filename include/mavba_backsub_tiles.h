/*
 * mavba_backsub_tiles.h - test entry of the point back-substitution's wave tiles (C ABI, same library as mavba.h).
 *
 * A header of its own: mavba.h is the interface the drop-in replacement of bundle_adjustment.cc is compiled against, and
 * that translation unit needs nothing of this.
 */
#ifndef MAVBA_BACKSUB_TILES_H_
#define MAVBA_BACKSUB_TILES_H_

#include "mavba.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Test entry (no device needed): the wave tiles of the point back-substitution (k_backsub_points_tiles) for points whose
 * observations are [pt_start[q], pt_start[q + 1]), q < num_points. tiles_out [4 * cap]: first point, points, first observation,
 * observations of every tile, in order. Returns the number of tiles (at most num_points) or a negative error code. */
int mavba_debug_backsub_tiles(int32_t num_points, const int32_t* pt_start, int32_t* tiles_out, int32_t cap);

#ifdef __cplusplus
}
#endif
#endif
