// nlr_shape.h -- the grid of a z stage that ends in a reduction, and the rows ONE launch of it may take.  Plain arithmetic: no HIP
// call, no device (the emulator group `nlrshape` includes this file alone).
#pragma once
#include <stdint.h>

namespace mfft {

struct NlrShape {
  int ngroups = 0;        // workgroups of the launch: a workgroup takes 2 * tile rows per pass, then strides by the grid
  int64_t waves = 0;      // its waves (the kinds that sum doubles write one group of partial values per wave)
  int64_t max_rows = 0;   // rows ONE launch may take; a longer run of rows is split into launches of at most that many
  int tile = 0;           // pairs of rows per workgroup = row slots of a workgroup (the profiles write one partial profile per row slot)
};
constexpr int64_t NLR_UNLIMITED = INT64_MAX;

// The launch over nrows >= 1 rows of length n by a kernel of `tile` pairs of rows per workgroup and `threads` threads, `cap`
// workgroups resident at once: never more workgroups than are resident, never more than there are pairs of rows to start on.
// counts: a workgroup counts into unsigned slots, passes x 2 tile x n values at the most -- max_rows keeps that below 2^32, so that
// nothing wraps silently; a kind that sums doubles has no such limit.  false: one pass of a workgroup alone counts 2^32 values.
inline bool nlr_shape(int tile, int threads, int64_t n, int cap, int64_t nrows, bool counts, NlrShape* out) {
  out->max_rows = NLR_UNLIMITED;
  out->tile = tile;
  if (counts) {
    const int64_t per_pass = 2 * (int64_t)tile * n;                   // values per field of one workgroup's pass
    const int64_t passes = ((int64_t)1 << 32) / per_pass - 1;
    if (passes < 1) return false;
    out->max_rows = passes * cap * 2 * tile;
  }
  const int64_t rows = nrows < out->max_rows ? nrows : out->max_rows;
  const int64_t units = (rows + 2 * tile - 1) / (2 * tile);
  out->ngroups = (int)(units < cap ? units : cap);
  out->waves = (int64_t)out->ngroups * ((threads + 63) / 64);
  return true;
}
// what one workgroup of a launch of ngroups workgroups over nrows rows counts per field: passes x 2 tile x n
inline int64_t nlr_counted(int tile, int64_t n, int64_t nrows, int ngroups) {
  const int64_t units = (nrows + 2 * tile - 1) / (2 * tile);
  return (units + ngroups - 1) / ngroups * 2 * tile * n;
}

}  // namespace mfft
