// emulator group nlrshape: the grid and split arithmetic of the z stages that end in a reduction (nlr_shape.h), as the loop over
// the rows of a batch (core.hip nlr_rows) uses it -- no kernel runs and nothing is allocated: with few resident workgroups and long
// rows, 2^32 values per workgroup are reached at row counts that are plain integers here.
#include "emu.h"
#include "nlr_shape.h"

// the launches nlr_rows makes over nrows rows; false: a launch breaks a rule
static bool split_ok(int tile, int threads, int64_t n, int cap, int64_t nrows, bool counts, int* nlaunch) {
  int64_t covered = 0;
  *nlaunch = 0;
  for (int64_t r0 = 0; r0 < nrows; ++*nlaunch) {
    NlrShape s;
    if (!nlr_shape(tile, threads, n, cap, nrows - r0, counts, &s)) return false;
    const int64_t rows = std::min(nrows - r0, s.max_rows);
    if (rows < 1 || r0 != covered) return false;                  // every row exactly once: the launches tile [0, nrows) in order
    const int64_t units = (rows + 2 * tile - 1) / (2 * tile);
    if (s.ngroups < 1 || s.ngroups > std::min<int64_t>(units, cap)) return false;
    if (s.waves != (int64_t)s.ngroups * ((threads + 63) / 64)) return false;
    const int64_t passes = (units + s.ngroups - 1) / s.ngroups;
    if (counts && passes * 2 * tile * n >= ((int64_t)1 << 32)) return false;
    if (counts && nlr_counted(tile, n, rows, s.ngroups) != passes * 2 * tile * n) return false;
    covered += rows;
    r0 += rows;
  }
  return covered == nrows;
}

static void emu_group() {
  for (int cap : {1, 7, 1024})
    for (int tile : {1, 4, 16})
      for (int64_t n : {(int64_t)64, (int64_t)4096, (int64_t)65535}) {
        NlrShape one;
        bool ok = nlr_shape(tile, 256, n, cap, 1, true, &one) && one.max_rows > 0 && one.max_rows % (2 * tile) == 0;
        const int64_t mr = ok ? one.max_rows : 1;
        // one row, odd counts, a ragged last pass, the limit and one row either side of it, three launches and more
        const int64_t rows[] = {1, 2, 3, 2 * tile, 2 * tile + 1, (int64_t)cap * 2 * tile, (int64_t)cap * 2 * tile + 1, 12345, mr - 1, mr, mr + 1,
                                2 * mr, 2 * mr + 1, 3 * mr - 1, 3 * mr, 3 * mr + 7, 5 * mr + 2 * tile + 1};
        int most = 0, bad = 0;
        for (int64_t nrows : rows) {
          if (nrows < 1) continue;
          int nl = 0;
          if (!split_ok(tile, 256, n, cap, nrows, true, &nl)) ++bad;
          if (nl != (nrows + mr - 1) / mr) ++bad;                  // no launch more than the limit asks for
          most = std::max(most, nl);
          if (!split_ok(tile, 192, n, cap, nrows, false, &nl) || nl != 1) ++bad;      // sums of doubles: exactly one launch
        }
        if (!ok || most < 3) ++bad;
        char name[64];
        snprintf(name, sizeof name, "nlr_shape cap=%d tile=%d", cap, tile);
        report(name, (int)n, "-", (double)bad, 0.5);
      }
  // one pass of a workgroup alone would count 2^32 values: refused, not split
  NlrShape s;
  report("nlr_shape pass too long", 1 << 30, "-", nlr_shape(16, 256, (int64_t)1 << 30, 7, 100, true, &s) ? 1.0 : 0.0, 0.5);
}
