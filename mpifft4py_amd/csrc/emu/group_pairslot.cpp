// emulator group pairslot: the slot order of the pair-row kernels (fft_kernels.h pair_slot), and those kernels with tiled order on
// the transposed work array of the split-last route (real side blocked in y with one row per block)
#include "test_row.h"

// pair_slot is a bijection of [0, nx * n1) onto the nx x n1 slot grid, nx = n0 / 2 + 1, and G = 0 is the row order.  One line per
// G and order inside the tiles; the error column counts the (n0, n1) for which it is not.
static void test_pair_slot_bijection(bool xfast) {
  for (unsigned G : {0u, 1u, 2u, 3u, 4u, 8u, 16u, 32u}) {
    int bad = 0;
    for (unsigned n0 = 1; n0 <= 20; ++n0)
      for (unsigned n1 = 1; n1 <= 20; ++n1) {
        const unsigned nx = n0 / 2 + 1;
        std::vector<int> seen(nx * n1, 0);
        bool ok = true;
        for (unsigned q = 0; q < nx * n1; ++q) {
          unsigned kx = ~0u, ky = ~0u;
          pair_slot(q, nx, n1, G, xfast, &kx, &ky);
          if (kx >= nx || ky >= n1 || seen[kx * n1 + ky]++) ok = false;
          if (G == 0 && (kx != q / n1 || ky != q % n1)) ok = false;
          // tiled: inside a tile the slots follow each other with ky fastest (xfast: kx fastest)
          if (G > 0 && ok && q > 0) {
            unsigned px, py;
            pair_slot(q - 1, nx, n1, G, xfast, &px, &py);
            const bool same_tile = px / G == kx / G && py / G == ky / G;
            const bool next = xfast ? (ky == py && kx == px + 1) || (ky == py + 1 && kx == kx / G * G)
                                    : (kx == px && ky == py + 1) || (kx == px + 1 && ky == ky / G * G);
            if (same_tile && !next) ok = false;
          }
        }
        if (!ok) ++bad;
      }
    char name[64];
    snprintf(name, sizeof name, "pair_slot bijection G=%u%s", G, xfast ? " xfast" : "");
    report(name, 20, "-", (double)bad, 0.5);
  }
}

static void emu_group() {
  test_pair_slot_bijection(false);
  test_pair_slot_bijection(true);
  // transposed real side (one row per y block), tiles smaller than, equal to and larger than the grid, partial edge tiles in both
  // directions, self-paired planes and rows, a partial last workgroup, the shipped shapes
  test_pair<Spec<32, 8, 4>, double, 4, true>(4, 6, 1, 2);
  test_pair<Spec<32, 8, 4>, double, 4, true>(3, 5, 1, 2);
  test_pair<Spec<32, 8, 4>, double, 4, false>(5, 4, 1, 3);
  test_pair<Spec<32, 8, 4>, double, 2, true>(2, 2, 1, 1);
  test_pair<Spec<32, 8, 4>, double, 64, true>(9, 15, 1, 4);
  test_pair<Spec<32, 8, 4>, double, 4, true>(34, 18, 1, 4);
  test_pair<Spec<32, 8, 4>, float, 8, true>(6, 3, 1, 16);
  test_pair<Spec<128, 16, 8>, double, 32, true>(12, 20, 1, 4);
  test_pair<Spec<128, 16, 8>, double, 32, true>(12, 20, 1, 16);
  test_pair<Spec<512, 8, 8, 8>, double, 4, true>(3, 4, 1, 2);
  test_pair<Spec<1024, 16, 8, 8>, double, 2, false>(2, 3, 1, 8);
  // kx fastest inside the tiles
  test_pair<Spec<32, 8, 4>, double, 4, true>(34, 18, 1, 4, true);
  test_pair<Spec<32, 8, 4>, double, 64, true>(9, 15, 1, 4, true);
  test_pair<Spec<128, 16, 8>, double, 32, true>(12, 20, 1, 16, true);
  test_pair<Spec<512, 8, 8, 8>, double, 4, true>(3, 4, 1, 2, true);
  // tiled order on the plain and on a blocked real side
  test_pair<Spec<32, 8, 4>, double, 4, true>(4, 6, 0, 4);
  test_pair<Spec<32, 8, 4>, double, 4, true>(4, 6, 3, 2);
}
