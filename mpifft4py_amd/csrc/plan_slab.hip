// plan_slab.hip -- the slab routes: blocking, and the two exchange pipelines (kz slices, batches of x rows).
#include "plan_impl.h"

using namespace mfft;

#ifndef MFFT_FWD_OOP_DEFAULT
#define MFFT_FWD_OOP_DEFAULT 0      // one-rank forward y / x passes out of place: see mfft_plan_s::fwd_out_of_place
#endif

// One-rank forward transform: y and x passes out of place through a work buffer of the size of the spectrum instead
// of in place on the result.  MFFT_FWD_OOP=1 / 0 forces it on / off; default: off (measured).
// When on by default it would still need room: the buffer exists already (the inverse uses the same one), or a
// quarter of the free HBM covers it.
bool mfft_plan_s::fwd_out_of_place(size_t cbytes) {
  static const int mode = (int)env_int("MFFT_FWD_OOP", MFFT_FWD_OOP_DEFAULT);
  if (mode <= 0) return false;
  if (work[0].bytes >= cbytes) return true;
  size_t fr = 0, tot = 0;
  if (hipMemGetInfo(&fr, &tot) != hipSuccess) { (void)hipGetLastError(); return false; }
  return cbytes <= fr / 4;
}

// ===========================================================================
// one rank, real data: real / complex split at the spectrum end
// ===========================================================================
// The regular route turns real rows into half-spectrum rows FIRST, so both strided passes run on rows of N2/2 + 1 bins:
// 8208 bytes at 1024^3 in double precision, every 128-byte tile row across two lines, no non-temporal build.  Here the
// real array is read as the complex field w[x, y, m] = u[x, y, 2m] + i u[x, y, 2m+1] (no copy), x and y are transformed as
// c2c passes on rows of N2/2 complex values -- whole lines for N2 >= 16 -- between u and a work array W of (N0, N1, N2/2)
// whose planes the plan may pad (split_last_pad), and the z pass does the real / complex split LAST: per row a length-N2/2
// c2c and the split post-pass with the mirrored value taken from the Hermitian partner row (fft_kernels.h PAIR).  Only the
// contiguous-axis kernels ever touch the caller's compact rows.  Same six launches, same bytes (2 * 6 R against 2 (R + 5 C)).
// The inverse mirrors it: pair-merge z pass fu -> W, y in place on W, x out of place into u -- the pass that READS
// power-of-two planes is the slow one (profiles/r02_power_of_two_stride.txt), so the padded W is what x reads.
// (That is the order "x first"; split_last_layout below may pick y first -- y, x, z forward and z, x, y inverse, both x passes in
// place on W -- and another layout of W.)
// Results differ from the regular route's in the last bits (another order of the same sums).
bool mfft_plan_s::split_last_eligible() const {
  if (d.decomp != MFFT_SLAB || P != 1 || !r2c || nat_pitch() || d.line2d || d.drop_nyquist || split_last == 0) return false;
  if (N0 < 2 || N1 < 2 || N2 % 2 || !pair_rows_supported(N2, prec)) return false;
  if (split_last > 0) return true;
  // by rule: only where it was measured to pay (profiles/split_last_ab.txt), which is the 1024^3 mesh in double precision.  Other
  // large meshes with z rows of 8 KiB and more probably gain as well (same kernels, same strides in y); nobody has measured them.
  return prec == MFFT_DOUBLE && N0 == 1024 && N1 == 1024 && N2 == 1024;
}
// Layout of W and order of the passes.  By rule: the plain array (one block), planes plane_pad further apart, x first -- except on
// the mesh the route is on for by itself (1024^3 in double precision), where the sweep of profiles/split_last_blocked_ab.txt picked
// y first with the planes 16 KiB further apart (both x passes in place on W: 3.40 ms each against 3.81 / 3.46 with x first and one
// line; no block came out ahead of that: small blocks bring the x passes to 3.03 - 3.11 ms and give it back in the y and z passes).
// The switches of plan_impl.h choose another block, pad or order.  A block that does not divide N1 falls back to the plain array.  Blocked, SR and SB follow
// the slow-pitch rules of the exchanged layouts (slow_pitch_pad: 64 KiB multiples, 2^a + 2^(a-7)); pads are whole cache lines, so
// the non-temporal builds stay eligible.
mfft_plan_s::SplitLastLayout mfft_plan_s::split_last_layout() const {
  const int64_t M = N2 / 2;
  SplitLastLayout l;
  l.B = N1;
  if (split_last_yblock > 0 && split_last_yblock < N1 && N1 % split_last_yblock == 0 && N1 < 65536) l.B = split_last_yblock;
  l.nblk = N1 / l.B;
  const bool rule_mesh = prec == MFFT_DOUBLE && N0 == 1024 && N1 == 1024 && N2 == 1024;
  l.yfirst = split_last_yfirst >= 0 ? std::min(split_last_yfirst, 2) : rule_mesh ? 1 : 0;
  int64_t pad_r = l.B == N1 ? (rule_mesh && l.yfirst > 0 ? (int64_t)(16384 / es) : split_last_pad()) : slow_pitch_pad(l.B * M);
  if (split_last_pad_bytes >= 0 && split_last_pad_bytes % 128 == 0) pad_r = split_last_pad_bytes / (int64_t)es;
  l.SR = l.B * M + pad_r;
  l.SB = N0 * l.SR + (l.nblk > 1 ? slow_pitch_pad(N0 * l.SR) : 0);
  return l;
}
// Route "x near": the transposed array W_T next to W.  With ONE work array a transpose is paid on one side or the other
// (profiles/split_last_blocked_ab.txt section 3); with two, the x pass is the transposing pass, out of place, and a strided pass that
// READS far rows and writes near ones is the cheap kind (bwd_y on B = 1: 2.92 - 3.12 ms against fwd_y's 3.40 - 3.46).  Forward: y
// u -> W as ever, x W -> W_T (one outer batch per y: rows a plane of W apart in, SR apart out), z W_T -> fu.  Inverse: the existing
// order "B = 1, y first" on W_T alone -- z fu -> W_T, x in place on near rows, y W_T -> u.  The z passes take their slots in tiles
// (fft_kernels.h pair_slot; the forward one with kx fastest: measured) so that the rows they move are near on both sides.  Same kernels, same order of sums: the results are the
// bits of the route without it.  MFFT_SPLIT_LAST_XNEAR chooses the directions (plan_impl.h); the forward direction needs the plain W
// with y first.  By rule (profiles/split_last_xnear_ab.txt) only on the mesh the split-last route is on for by itself.
#ifndef MFFT_SPLIT_LAST_XNEAR_DEFAULT
#define MFFT_SPLIT_LAST_XNEAR_DEFAULT 1
#endif
#ifndef MFFT_SPLIT_LAST_PAIRBLOCK_DEFAULT
#define MFFT_SPLIT_LAST_PAIRBLOCK_DEFAULT 16
#endif
#ifndef MFFT_SPLIT_LAST_PAIRXFAST_DEFAULT
#define MFFT_SPLIT_LAST_PAIRXFAST_DEFAULT 1
#endif
static int xnear_wanted(const mfft_plan_s* p) {
  if (p->N1 >= 65536) return 0;          // (the pair kernels' blocked real side: core.hip launch_real)
  if (p->split_last_xnear >= 0) return std::min(p->split_last_xnear, 3);
  return p->prec == MFFT_DOUBLE && p->N0 == 1024 && p->N1 == 1024 && p->N2 == 1024 ? MFFT_SPLIT_LAST_XNEAR_DEFAULT : 0;
}
mfft_plan_s::SplitLastLayout mfft_plan_s::split_last_layout_t() const {
  const int64_t M = N2 / 2;
  SplitLastLayout l;
  l.B = 1;
  l.nblk = N1;
  l.yfirst = 1;
  l.SR = M + slow_pitch_pad(M);
  int64_t pad_b = slow_pitch_pad(N0 * l.SR);
  if (split_last_xnear_pad_bytes >= 0 && split_last_xnear_pad_bytes % 128 == 0) pad_b = split_last_xnear_pad_bytes / (int64_t)es;
  l.SB = N0 * l.SR + pad_b;
  return l;
}
int mfft_plan_s::split_last_xnear_mode() {
  if (!split_last_route() || split_last_xnear_fit != 1) return 0;
  const int want = xnear_wanted(this);
  const SplitLastLayout l = split_last_layout();
  const bool fwd = (want == 1 || want == 2) && l.B == N1 && l.yfirst_fwd(), bwd = want == 1 || want == 3;
  return fwd && bwd ? 1 : fwd ? 2 : bwd ? 3 : 0;
}
// G of pair_slot for a z pass of the route: what MFFT_SPLIT_LAST_PAIRBLOCK says; by rule tiles for the route "x near" alone
int mfft_plan_s::split_last_pair_tile(bool xnear) const {
  const int64_t g = split_last_pairblock >= 0 ? std::min(split_last_pairblock, 32768) : xnear ? MFFT_SPLIT_LAST_PAIRBLOCK_DEFAULT : 0;
  return g * N1 < ((int64_t)1 << 31) ? (int)g : 0;
}
// ... and whether kx runs fastest inside a tile (bit 0: forward, bit 1: inverse)
bool mfft_plan_s::split_last_pair_xfast(bool xnear, bool inv) const {
  const int mask = split_last_pairxfast >= 0 ? split_last_pairxfast : xnear ? MFFT_SPLIT_LAST_PAIRXFAST_DEFAULT : 0;
  return (mask >> (inv ? 1 : 0)) & 1;
}
bool mfft_plan_s::split_last_route() {
  if (!split_last_eligible()) return false;
  if (split_last_fit < 0) {      // the forward transform needs a work buffer now: as fwd_out_of_place decides
    // (both arrays of the route "x near" inside the same quarter of the free memory, or the plan goes without W_T)
    const size_t need = (size_t)split_last_layout().elems() * es;
    const size_t need_t = xnear_wanted(this) ? (size_t)split_last_layout_t().elems() * es : 0;
    const size_t miss = work[0].bytes >= need ? 0 : need, miss_t = work[1].bytes >= need_t ? 0 : need_t;
    size_t fr = 0, tot = 0;
    if (miss + miss_t > 0 && hipMemGetInfo(&fr, &tot) != hipSuccess) { (void)hipGetLastError(); fr = 0; }
    split_last_fit = miss <= fr / 4 ? 1 : 0;
    split_last_xnear_fit = need_t > 0 && split_last_fit == 1 && miss + miss_t <= fr / 4 ? 1 : 0;
  }
  return split_last_fit == 1;
}
// The two strided passes on W = (N1 / B blocks) x (N0 x rows) x (B y rows of M).  The x pass takes one outer batch per block, its
// B * M columns contiguous on W's side (on the caller's side, x first, the same columns of the compact planes); the y pass one
// outer batch per x, its rows on W's side two-level: B of them M apart, then the next block.  yfirst: y carries the caller's array
// `user` (rows M apart: the fast case) and x runs in place on W; else x carries it and y runs in place.
int mfft_plan_s::split_last_x(const SplitLastLayout& l, const void* user_in, void* user_out, void* W, bool inv) {
  const int64_t M = N2 / 2;
  const void* in = user_in ? user_in : W;
  void* out = user_out ? user_out : W;
  return col(in, out, N0, inv, l.nblk, l.B * M, user_in ? l.B * M : l.SB, plain(user_in ? N1 * M : l.SR),
             user_out ? l.B * M : l.SB, plain(user_out ? N1 * M : l.SR));
}
int mfft_plan_s::split_last_y(const SplitLastLayout& l, const void* user_in, void* user_out, void* W, bool inv) {
  const int64_t M = N2 / 2;
  const void* in = user_in ? user_in : W;
  void* out = user_out ? user_out : W;
  const RowSpec wrows = two_level(l.B, l.SB, M);
  return col(in, out, N1, inv, N0, M, user_in ? N1 * M : l.SR, user_in ? plain(M) : wrows, user_out ? N1 * M : l.SR,
             user_out ? plain(M) : wrows);
}
int mfft_plan_s::split_last_z(const SplitLastLayout& l, const void* in, void* out, bool inv, bool xnear) {
  RealArgs a = inv ? real_args(in, out, N0 * N1, N2, Nf, N2, 1.0 / (double)N2) : real_args(in, out, N0 * N1, N2, N2, Nf, 1.0);
  a.pair_n0 = (int)N0; a.pair_n1 = (int)N1; a.pair_rplane = 2 * l.SR; a.pair_cplane = N1 * Nf;
  a.pair_yblock = (int)l.B; a.pair_rblock = 2 * l.SB;
  a.pair_tile = split_last_pair_tile(xnear);
  a.pair_tile_xfast = split_last_pair_xfast(xnear, inv);
  return inv ? mfft::launch_c2r(a, stream) : mfft::launch_r2c(a, stream);
}
int mfft_plan_s::slab_forward_split_last(const void* u, void* fu) {
  const SplitLastLayout l = split_last_layout();
  const double Wb = (double)(N0 * N1 * (N2 / 2)) * es;
  const int xnear = split_last_xnear_mode();
  MFFT_TRY(ensure(work[0], (size_t)l.elems() * es));
  void* W = work[0].p;
  if (xnear == 1 || xnear == 2) {
    const SplitLastLayout t = split_last_layout_t();
    const int64_t M = N2 / 2;
    MFFT_TRY(ensure(work[1], (size_t)t.elems() * es));
    void* WT = work[1].p;
    MFFT_TRY(stage("fwd_y", 2 * Wb, [&] { return split_last_y(l, u, nullptr, W, false); }));
    MFFT_TRY(stage("fwd_x", 2 * Wb, [&] { return col(W, WT, N0, false, N1, M, M, plain(l.SR), t.SB, plain(t.SR)); }));
    return stage("fwd_z", Wb + (double)(N0 * N1 * Nf) * es, [&] { return split_last_z(t, WT, fu, false, true); });
  }
  if (l.yfirst_fwd()) {
    MFFT_TRY(stage("fwd_y", 2 * Wb, [&] { return split_last_y(l, u, nullptr, W, false); }));
    MFFT_TRY(stage("fwd_x", 2 * Wb, [&] { return split_last_x(l, nullptr, nullptr, W, false); }));
  } else {
    MFFT_TRY(stage("fwd_x", 2 * Wb, [&] { return split_last_x(l, u, nullptr, W, false); }));
    MFFT_TRY(stage("fwd_y", 2 * Wb, [&] { return split_last_y(l, nullptr, nullptr, W, false); }));
  }
  return stage("fwd_z", Wb + (double)(N0 * N1 * Nf) * es, [&] { return split_last_z(l, W, fu, false); });
}
int mfft_plan_s::slab_backward_split_last(const void* fu, void* u) {
  const SplitLastLayout l = split_last_layout();
  const double Wb = (double)(N0 * N1 * (N2 / 2)) * es;
  const int xnear = split_last_xnear_mode();
  if (xnear == 1 || xnear == 3) {
    const SplitLastLayout t = split_last_layout_t();
    MFFT_TRY(ensure(work[1], (size_t)t.elems() * es));
    void* WT = work[1].p;
    MFFT_TRY(stage("bwd_z", Wb + (double)(N0 * N1 * Nf) * es, [&] { return split_last_z(t, fu, WT, true, true); }));
    MFFT_TRY(stage("bwd_x", 2 * Wb, [&] { return split_last_x(t, nullptr, nullptr, WT, true); }));
    return stage("bwd_y", 2 * Wb, [&] { return split_last_y(t, nullptr, u, WT, true); });
  }
  MFFT_TRY(ensure(work[0], (size_t)l.elems() * es));
  void* W = work[0].p;
  MFFT_TRY(stage("bwd_z", Wb + (double)(N0 * N1 * Nf) * es, [&] { return split_last_z(l, fu, W, true); }));
  if (l.yfirst_bwd()) {
    MFFT_TRY(stage("bwd_x", 2 * Wb, [&] { return split_last_x(l, nullptr, nullptr, W, true); }));
    return stage("bwd_y", 2 * Wb, [&] { return split_last_y(l, nullptr, u, W, true); });
  }
  MFFT_TRY(stage("bwd_y", 2 * Wb, [&] { return split_last_y(l, nullptr, nullptr, W, true); }));
  return stage("bwd_x", 2 * Wb, [&] { return split_last_x(l, nullptr, u, W, true); });
}

// ===========================================================================
// slab
// ===========================================================================
int mfft_plan_s::slab_forward(const void* u, void* fu) {
  const double Cb = (double)(N0 * Np1 * Nf) * es;            // local complex bytes
  const double Rb = (double)(Np0 * N1 * N2) * rs;            // local real-space bytes
  if (P == 1 && split_last_route()) return slab_forward_split_last(u, fu);
  if (P == 1) {
    const int64_t Z = Zc();          // row pitch of the spectrum and of the intermediates: Nf, or the caller's pitch
    if (const int64_t xpad = p1_plane_pad()) {
      MFFT_TRY(stage("fwd_z", Rb + Cb, [&] { return z_forward(u, fu, N0 * N1, N2, Z); }));
      // power-of-two plane stride: the y transform writes planes one cache line apart from that, the x transform reads them
      const int64_t pl = N1 * Z + xpad;
      MFFT_TRY(ensure(work[0], (size_t)(N0 * pl) * es));
      void* A = work[0].p;
      MFFT_TRY(stage("fwd_y", 2 * Cb, [&] { return col(fu, A, N1, false, N0, Nf, N1 * Z, plain(Z), pl, plain(Z)); }));
      MFFT_TRY(stage("fwd_x", 2 * Cb, [&] { return col(A, fu, N0, false, 1, N1 * Z, 0, plain(pl), 0, plain(N1 * Z)); }));
      return 0;
    }
    MFFT_TRY(stage("fwd_z", Rb + Cb, [&] { return z_forward(u, fu, N0 * N1, N2, Z); }));
    if (fwd_out_of_place((size_t)Cb)) {
      // y transform into the work buffer (the one the inverse uses anyway), x transform out of it into the result: both
      // passes out of place (MFFT_FWD_OOP, see fwd_out_of_place)
      MFFT_TRY(ensure(work[0], (size_t)(N0 * N1 * Z) * es));
      void* A = work[0].p;
      MFFT_TRY(stage("fwd_y", 2 * Cb, [&] { return col(fu, A, N1, false, N0, Nf, N1 * Z, plain(Z), N1 * Z, plain(Z)); }));
      MFFT_TRY(stage("fwd_x", 2 * Cb, [&] { return col(A, fu, N0, false, 1, N1 * Z, 0, plain(N1 * Z), 0, plain(N1 * Z)); }));
      return 0;
    }
    MFFT_TRY(stage("fwd_y", 2 * Cb, [&] { return col(fu, fu, N1, false, N0, Nf, N1 * Z, plain(Z), N1 * Z, plain(Z)); }));
    MFFT_TRY(stage("fwd_x", 2 * Cb, [&] { return col(fu, fu, N0, false, 1, N1 * Z, 0, plain(N1 * Z), 0, plain(N1 * Z)); }));
    return 0;
  }
  if (nbatch > 1) return slab_forward_rows(u, fu);
  if (nslice > 1) return slab_forward_pipelined(u, fu);
  // x rows of the exchanged layout lie S elements apart: Np1 * Nf, plus one cache line where that is a 64 KiB multiple
  const int64_t S = Np1 * Nf + xplane_pad(true);
  const size_t cb = (size_t)std::max(Np0 * N1 * Nf, N0 * S) * es;
  MFFT_TRY(ensure(work[0], cb));
  MFFT_TRY(ensure(work[1], cb));
  void *A = work[0].p, *B = work[1].p;
  MFFT_TRY(stage("fwd_z", Rb + Cb, [&] { return z_forward(u, A, Np0 * N1, N2, Nf); }));
  // y transform writes straight into the packed (P, Np0, Np1, Nf) send layout (slab.py:403)
  MFFT_TRY(stage("fwd_y", 2 * Cb, [&] {
    return col(A, B, N1, false, Np0, Nf, N1 * Nf, plain(Nf), S, two_level(Np1, Np0 * S, Nf));
  }));
  if (xpass_inplace && S == Np1 * Nf) {           // round 1 - 3: receive into the result, x transform in place
    MFFT_TRY(stage("fwd_a2a", 0, [&] { return xchg(0, true, false, B, fu); }));
    MFFT_TRY(stage("fwd_x", 2 * Cb, [&] { return col(fu, fu, N0, false, 1, Np1 * Nf, 0, plain(Np1 * Nf), 0, plain(Np1 * Nf)); }));
    return 0;
  }
  // A is free again (the y transform has read it): the chunks land there and the x transform runs OUT of place into the
  // result -- no more memory, and an out-of-place pass is the faster one (1024 fp64: 3.19 against 3.35 ms)
  MFFT_TRY(stage("fwd_a2a", 0, [&] { return xchg(0, true, false, B, A); }));
  MFFT_TRY(stage("fwd_x", 2 * Cb, [&] { return col(A, fu, N0, false, 1, Np1 * Nf, 0, plain(S), 0, plain(Np1 * Nf)); }));
  return 0;
}

// 2/3-rule with the rule's own mask (detect_band; every rank agreed on the band when the mask was set): the pruned inverse
int mfft_plan_s::slab_backward_pruned(const void* fu, void* u) {
  const double Cb = (double)(N0 * Np1 * Nf) * es, Rb = (double)(Np0 * N1 * N2) * rs;
  double keep0, keep1, keep2;
  band_keep(&keep0, &keep1, &keep2);
  if (P == 1) {
    const int64_t Z = Zc();
    MFFT_TRY(ensure(work[0], (size_t)(N0 * N1 * Z) * es));
    void* Aw = work[0].p;
    ColArgs::Band bx, by;
    bx.row_lo = ba0; bx.row_hi = bb0; bx.g_off = 0; bx.g_lo = ba1; bx.g_hi = bb1;
    by.row_lo = ba1; by.row_hi = bb1; by.c_lim = ba2;        // columns = kz of one x plane: only the first a2 are launched
    MFFT_TRY(stage("bwd_x", Cb * keep1 * keep2 * (keep0 + 1.0), [&] {
      if (nat_pitch()) {
        // pitched rows (round 6): the tile list below was made for rows of Nf bins, so the x pass takes one outer batch per ky
        // (removed ky: nothing launched does anything) with the kept kz of it as its columns -- the form the pruned exchange uses
        bx.g_step = 1;
        return col_band(fu, Aw, N0, N1, ba2, Z, plain(N1 * Z), Z, plain(N1 * Z), bx);
      }
      bx.c_off = 0; bx.c_per = (int)Nf; bx.c_lim = ba2; bx.g_step = 0;
      bx.tile_list = band_tiles; bx.ntiles_listed = band_ntiles;
      return col_band(fu, Aw, N0, 1, N1 * Nf, 0, plain(N1 * Nf), 0, plain(N1 * Nf), bx);
    }));
    MFFT_TRY(stage("bwd_y", Cb * keep2 * (keep1 + 1.0), [&] {
      return col_band(Aw, Aw, N1, N0, ba2, N1 * Z, plain(Z), N1 * Z, plain(Z), by);
    }));
    MFFT_TRY(stage("bwd_z", Rb + Cb * keep2, [&] { return c2r_rows(Aw, u, N0 * N1, N2, Z, N2, 1.0 / (double)N2, ba2); }));
    return 0;
  }
  if (nbatch > 1) return slab_backward_rows(fu, u, true);          // the row-batch exchange pipeline, pruned
  if (nslice > 1) return slab_backward_pipelined(fu, u, true);     // the kz-slice exchange pipeline, pruned
  // pruned inverse over P ranks (blocking exchange): the x pass reads the kept kx rows and writes (N0, Np1, a2) -- the
  // kept kz bins only, zeros for the ky this rank's mask removes --, so the exchange carries a2 / Nf of the bytes; the y
  // pass and c2r work on rows of a2 bins
  const int64_t a2 = ba2, per_line = (int64_t)(128 / es);
  const int64_t ap = (a2 + per_line - 1) / per_line * per_line;      // rows of the compact layout start on cache lines
  const size_t cbp = (size_t)(Np0 * N1 * ap) * es;
  MFFT_TRY(ensure(work[0], cbp));
  MFFT_TRY(ensure(work[1], cbp));
  void *Aw = work[0].p, *Bw = work[1].p;
  ColArgs::Band bx;
  bx.row_lo = ba0; bx.row_hi = bb0; bx.g_off = 0; bx.g_step = 1; bx.g_lo = ba1; bx.g_hi = bb1; bx.g_zero = 1;
  MFFT_TRY(stage("bwd_x", Cb * keep2 * (keep0 + 1.0), [&] {
    if (band_allzero) return zero(Aw, cbp);        // nothing of this rank's spectrum survives the mask
    return col_band(fu, Aw, N0, Np1, a2, Nf, plain(Np1 * Nf), ap, plain(Np1 * ap), bx);
  }));
  MFFT_TRY(stage("bwd_a2a", 0, [&] { return exchange_equal(world, Aw, Bw, (size_t)(Np0 * Np1 * ap) * es); }));
  MFFT_TRY(stage("bwd_y", 2 * Cb * keep2, [&] {
    return col(Bw, Aw, N1, true, Np0, a2, Np1 * ap, two_level(Np1, Np0 * Np1 * ap, ap), N1 * ap, plain(ap));
  }));
  MFFT_TRY(stage("bwd_z", Rb + Cb * keep2, [&] { return c2r_rows(Aw, u, Np0 * N1, N2, ap, N2, 1.0 / (double)N2, (int)a2); }));
  return 0;
}

int mfft_plan_s::slab_backward(const void* fu, void* u, bool masked) {
  const double Cb = (double)(N0 * Np1 * Nf) * es;
  const double Rb = (double)(Np0 * N1 * N2) * rs;
  const void* src = fu;
  MaskScope mask_scope{this};
  if (!masked && P == 1 && split_last_route()) return slab_backward_split_last(fu, u);
  if (masked && band_ok && prune_enabled()) {
    MFFT_TRY(require_mask());
    return slab_backward_pruned(fu, u);
  }
  if (masked) {
    bool fused = false;
    MFFT_TRY(fuse_mask(fu, (P == 1 && p1_plane_pad()) ? N1 : N0, &fused));
    if (!fused) {
      void* m = nullptr;
      MFFT_TRY(stage("bwd_mask", 2 * Cb, [&] { return apply_mask_copy(fu, &m); }));
      src = m;
    }
  }
  const int64_t Z = P == 1 ? Zc() : Nf;
  const size_t cb = (size_t)(Np0 * N1 * Z) * es;
  if (const int64_t xpad = P == 1 ? p1_plane_pad() : 0) {
    // slow plane stride (p1_plane_pad): y first (into padded planes), x out of them -- complex data: into the result, z in
    // place there; real data: into a second work buffer that c2r reads
    const int64_t pl = N1 * Z + xpad;
    MFFT_TRY(ensure(work[0], (size_t)(N0 * pl) * es));
    void* Ap = work[0].p;
    void* X = u;
    if (r2c) {
      MFFT_TRY(ensure(work[1], cb));
      X = work[1].p;
    }
    MFFT_TRY(stage("bwd_y", 2 * Cb, [&] { return col(src, Ap, N1, true, N0, Nf, N1 * Z, plain(Z), pl, plain(Z)); }));
    MFFT_TRY(stage("bwd_x", 2 * Cb, [&] { return col(Ap, X, N0, true, 1, N1 * Z, 0, plain(pl), 0, plain(N1 * Z)); }));
    MFFT_TRY(stage("bwd_z", Rb + Cb, [&] { return z_backward(X, u, N0 * N1, N2, Z); }));
    return 0;
  }
  MFFT_TRY(ensure(work[0], cb));
  void* A = work[0].p;
  if (P == 1) {                  // Z: the caller's pitch, kept in the intermediate as well, or compact rows of Nf
    // (Round 4 measured two more one-rank routes and removed them again -- a line-aligned intermediate (rows of N2/2 + 1 bins
    // rounded up to whole cache lines: one per cent at 1024^3 for the inverse, a loss forward and at 512^3) and a forward
    // transform whose x pass alone runs out of place (gains only at 2048^3 in single precision): profiles/r04_aligned_route_ab.txt,
    // r04_fwd_oop_ab.txt; the last commit that has the switches MFFT_ALIGNED / MFFT_FWD_OOP=2 is a7fb791.)
    MFFT_TRY(stage("bwd_x", 2 * Cb, [&] { return col(src, A, N0, true, 1, N1 * Z, 0, plain(N1 * Z), 0, plain(N1 * Z)); }));
    MFFT_TRY(stage("bwd_y", 2 * Cb, [&] { return col(A, A, N1, true, N0, Nf, N1 * Z, plain(Z), N1 * Z, plain(Z)); }));
    MFFT_TRY(stage("bwd_z", Rb + Cb, [&] { return z_backward(A, u, N0 * N1, N2, Z); }));
    return 0;
  }
  if (nbatch > 1) return slab_backward_rows(src, u);
  if (nslice > 1) return slab_backward_pipelined(src, u);
  MFFT_TRY(ensure(work[1], cb));
  void* B = work[1].p;
  MFFT_TRY(stage("bwd_x", 2 * Cb, [&] { return col(src, A, N0, true, 1, Np1 * Nf, 0, plain(Np1 * Nf), 0, plain(Np1 * Nf)); }));
  MFFT_TRY(stage("bwd_a2a", 0, [&] { return xchg(0, false, false, A, B); }));
  // y transform reads the (P, Np0, Np1, Nf) receive layout directly (transpose_Uc fused, maths.pyx:21-31)
  MFFT_TRY(stage("bwd_y", 2 * Cb, [&] {
    return col(B, A, N1, true, Np0, Nf, Np1 * Nf, two_level(Np1, Np0 * Np1 * Nf, Nf), N1 * Nf, plain(Nf));
  }));
  MFFT_TRY(stage("bwd_z", Rb + Cb, [&] { return z_backward(A, u, Np0 * N1, N2, Nf); }));
  return 0;
}

// ---- exchange pipeline (P > 1): the spectrum is cut into kz slices; slice s is
// transformed along y (written packed), exchanged on the communication stream
// while slice s+1 is transformed, and the x transform of slice s starts as soon
// as its exchange has landed.  Per slice the send layout is (P, Np0, Np1, kzs),
// the receive layout (N0, Np1, kzs).
int mfft_plan_s::slab_forward_pipelined(const void* u, void* fu) {
  const double Cb = (double)(N0 * Np1 * Nf) * es, Rb = (double)(Np0 * N1 * N2) * rs;
  // per slice the x rows of the exchanged layout lie slice_pitch() elements apart (Np1 * kz, plus a cache line where that
  // pitch reads slowly: xplane_pad's rule, slice by slice)
  const size_t cb = std::max((size_t)(Np0 * N1 * Nf), slice_offset(nslice, true)) * es;
  for (int i = 0; i < 3; ++i) MFFT_TRY(ensure(work[i], cb));
  char *A = static_cast<char*>(work[0].p), *B = static_cast<char*>(work[1].p), *Cr = static_cast<char*>(work[2].p);
  char* out = static_cast<char*>(fu);
  MFFT_TRY(stage("fwd_z", Rb + Cb, [&] { return z_forward(u, A, Np0 * N1, N2, Nf); }));
  for (int s = 0; s < nslice; ++s) {
    const int64_t k0 = kslice[s].start, kz = kslice[s].len, S = slice_pitch(s, true);
    const size_t boff = slice_offset(s, true) * es;
    MFFT_TRY(stage("fwd_y", 2 * Cb / nslice, [&] {
      return col(A + (size_t)k0 * es, B + boff, N1, false, Np0, kz, N1 * Nf, plain(Nf), S, two_level(Np1, Np0 * S, kz));
    }));
    MFFT_TRY(comm_waits(ev_compute[s]));
    MFFT_TRY(exchange_piece("fwd_a2a", 0, true, s, B, Cr, ev_comm[s]));
  }
  for (int s = 0; s < nslice; ++s) {
    const int64_t k0 = kslice[s].start, kz = kslice[s].len;
    const size_t boff = slice_offset(s, true) * es;
    MFFT_HIP(hipStreamWaitEvent(stream, ev_comm[s], 0));
    MFFT_TRY(stage("fwd_x", 2 * Cb / nslice, [&] {
      return col(Cr + boff, out + (size_t)k0 * es, N0, false, Np1, kz, kz, plain(slice_pitch(s, true)), Nf, plain(Np1 * Nf));
    }));
  }
  return 0;
}

// pruned (2/3-rule, band mask): slices that start at or beyond the a2 kept kz bins are not transformed or exchanged at
// all (every rank knows a2), the x pass does not load the removed kx rows and writes zeros for the ky its rank's mask
// removes, c2r reads a2 bins per row.
int mfft_plan_s::slab_backward_pipelined(const void* src, void* u, bool pruned) {
  const double Cb = (double)(N0 * Np1 * Nf) * es, Rb = (double)(Np0 * N1 * N2) * rs;
  ColArgs::Band bx;
  bx.row_lo = ba0; bx.row_hi = bb0; bx.g_off = 0; bx.g_step = 1; bx.g_lo = ba1; bx.g_hi = bb1; bx.g_zero = 1;
  auto kept = [&](int s) { return !pruned || kslice[s].start < ba2; };
  const size_t cb = (size_t)(Np0 * N1 * Nf) * es;
  for (int i = 0; i < 2; ++i) MFFT_TRY(ensure(work[i], cb));
  // work[2].p may hold the masked copy of the spectrum (src): use a 4th buffer for the y output
  MFFT_TRY(ensure(work3, cb));
  char *A = static_cast<char*>(work[0].p), *B = static_cast<char*>(work[1].p), *A2 = static_cast<char*>(work3.p);
  const char* in = static_cast<const char*>(src);
  for (int s = 0; s < nslice; ++s) {
    if (!kept(s)) continue;
    const int64_t k0 = kslice[s].start, kz = kslice[s].len;
    const size_t boff = (size_t)(P * Np0 * Np1 * k0) * es;
    MFFT_TRY(stage("bwd_x", 2 * Cb / nslice, [&] {
      if (pruned && band_allzero) return zero(A + boff, (size_t)(N0 * Np1 * kz) * es);
      if (pruned) return col_band(in + (size_t)k0 * es, A + boff, N0, Np1, kz, Nf, plain(Np1 * Nf), kz, plain(Np1 * kz), bx);
      return col(in + (size_t)k0 * es, A + boff, N0, true, Np1, kz, Nf, plain(Np1 * Nf), kz, plain(Np1 * kz));
    }));
    MFFT_TRY(comm_waits(ev_compute[s]));
    MFFT_TRY(exchange_piece("bwd_a2a", 0, false, s, A, B, ev_comm[s]));
  }
  for (int s = 0; s < nslice; ++s) {
    if (!kept(s)) continue;
    const int64_t k0 = kslice[s].start, kz = kslice[s].len;
    const size_t boff = (size_t)(P * Np0 * Np1 * k0) * es;
    MFFT_HIP(hipStreamWaitEvent(stream, ev_comm[s], 0));
    MFFT_TRY(stage("bwd_y", 2 * Cb / nslice, [&] {
      return col(B + boff, A2 + (size_t)k0 * es, N1, true, Np0, kz, Np1 * kz, two_level(Np1, Np0 * Np1 * kz, kz),
                 N1 * Nf, plain(Nf));
    }));
  }
  if (pruned) {
    MFFT_TRY(stage("bwd_z", Rb + Cb * (double)ba2 / (double)Nf, [&] {
      return c2r_rows(A2, u, Np0 * N1, N2, Nf, N2, 1.0 / (double)N2, ba2);
    }));
    return 0;
  }
  MFFT_TRY(stage("bwd_z", Rb + Cb, [&] { return z_backward(A2, u, Np0 * N1, N2, Nf); }));
  return 0;
}

// ---- slab, second pipeline flavour (`pipeline` < 0): batches of local x rows -----------------------------
// z and y transforms of batch b+1 overlap the exchange of batch b; the exchange delivers straight into the output
// array (its receive layout (N0, Np1, Nf) IS the output layout), where the x transform then runs in place over whole
// rows.  Compared with the kz slices: the z transform is overlapped instead of the x transform, no strided kz
// sub-columns, one work buffer less in the forward direction.  Which one is faster depends on the links; bench.py
// measures both.
int mfft_plan_s::slab_forward_rows(const void* u, void* fu) {
  const double Cb = (double)(N0 * Np1 * Nf) * es, Rb = (double)(Np0 * N1 * N2) * rs;
  const size_t cb = (size_t)(Np0 * N1 * Nf) * es;
  for (int i = 0; i < 2; ++i) MFFT_TRY(ensure(work[i], cb));
  char *A = static_cast<char*>(work[0].p), *Bk = static_cast<char*>(work[1].p);
  const char* in = static_cast<const char*>(u);
  const int B = nbatch;
  for (int b = 0; b < B; ++b) {
    const int64_t i0 = Np0 * b / B, mb = Np0 * (b + 1) / B - i0;
    MFFT_TRY(stage("fwd_z", (Rb + Cb) / B, [&] {
      return z_forward(in + (size_t)(i0 * N1 * N2) * rs, A + (size_t)(i0 * N1 * Nf) * es, mb * N1, N2, Nf);
    }));
    MFFT_TRY(stage("fwd_y", 2 * Cb / B, [&] {
      return col(A + (size_t)(i0 * N1 * Nf) * es, Bk + (size_t)(i0 * Np1 * Nf) * es, N1, false, mb, Nf, N1 * Nf, plain(Nf),
                 Np1 * Nf, two_level(Np1, Np0 * Np1 * Nf, Nf));
    }));
    MFFT_TRY(comm_waits(ev_compute[b]));
    MFFT_TRY(exchange_piece("fwd_a2a", 0, true, b, Bk, fu, ev_comm[b]));
  }
  MFFT_HIP(hipStreamWaitEvent(stream, ev_comm[B - 1], 0));
  MFFT_TRY(stage("fwd_x", 2 * Cb, [&] { return col(fu, fu, N0, false, 1, Np1 * Nf, 0, plain(Np1 * Nf), 0, plain(Np1 * Nf)); }));
  return 0;
}

int mfft_plan_s::slab_backward_rows(const void* src, void* u, bool pruned) {
  const double Cb = (double)(N0 * Np1 * Nf) * es, Rb = (double)(Np0 * N1 * N2) * rs;
  // pruned (2/3-rule, band mask): every array between the x pass and c2r holds rows of `w` = a2 (padded to a cache line)
  // kept kz bins instead of Nf, the exchange pieces shrink with them; see slab_backward
  const int64_t per_line = (int64_t)(128 / es);
  const int64_t w = pruned ? ((int64_t)ba2 + per_line - 1) / per_line * per_line : Nf, nz = pruned ? (int64_t)ba2 : Nf;
  const size_t cb = (size_t)(Np0 * N1 * w) * es;
  for (int i = 0; i < 2; ++i) MFFT_TRY(ensure(work[i], cb));
  const bool src_in_work2 = work[2].p != nullptr && src == work[2].p;     // the masked copy of the spectrum
  if (src_in_work2) MFFT_TRY(ensure(work3, cb));
  else MFFT_TRY(ensure(work[2], cb));
  char *A = static_cast<char*>(work[0].p), *Bk = static_cast<char*>(work[1].p);
  char* A2 = static_cast<char*>(src_in_work2 ? work3.p : work[2].p);
  char* out = static_cast<char*>(u);
  const int B = nbatch;
  MFFT_TRY(stage("bwd_x", 2 * Cb, [&] {
    if (pruned && band_allzero) return zero(A, cb);
    if (pruned) {
      ColArgs::Band bx;
      bx.row_lo = ba0; bx.row_hi = bb0; bx.g_off = 0; bx.g_step = 1; bx.g_lo = ba1; bx.g_hi = bb1; bx.g_zero = 1;
      return col_band(src, A, N0, Np1, nz, Nf, plain(Np1 * Nf), w, plain(Np1 * w), bx);
    }
    return col(src, A, N0, true, 1, Np1 * Nf, 0, plain(Np1 * Nf), 0, plain(Np1 * Nf));
  }));
  MFFT_TRY(comm_waits(ev_compute[0]));
  for (int b = 0; b < B; ++b) {
    MFFT_TRY(stage_on(cstream, "bwd_a2a", 0, [&] {
      Sched sc;
      if (pruned) {      // the same blocks as piece_sched's, with rows of w bins
        const int64_t i0 = Np0 * b / B, mb = Np0 * (b + 1) / B - i0;
        sc.peers = world;
        sc.sc.assign(P, (size_t)(mb * Np1 * w) * es);
        sc.rc = sc.sc;
        sc.sd.resize(P);
        sc.rd.resize(P);
        for (int r = 0; r < P; ++r) sc.sd[r] = sc.rd[r] = (size_t)((r * Np0 + i0) * Np1 * w) * es;
      } else {
        MFFT_TRY(piece_sched(0, false, b, &sc));
      }
      return run_sched(sc, A, Bk, cstream);
    }));
    MFFT_HIP(hipEventRecord(ev_comm[b], cstream));
  }
  for (int b = 0; b < B; ++b) {
    const int64_t i0 = Np0 * b / B, mb = Np0 * (b + 1) / B - i0;
    MFFT_HIP(hipStreamWaitEvent(stream, ev_comm[b], 0));
    MFFT_TRY(stage("bwd_y", 2 * Cb / B, [&] {
      return col(Bk + (size_t)(i0 * Np1 * w) * es, A2 + (size_t)(i0 * N1 * w) * es, N1, true, mb, nz, Np1 * w,
                 two_level(Np1, Np0 * Np1 * w, w), N1 * w, plain(w));
    }));
    MFFT_TRY(stage("bwd_z", (Rb + Cb) / B, [&] {
      if (pruned)
        return c2r_rows(A2 + (size_t)(i0 * N1 * w) * es, out + (size_t)(i0 * N1 * N2) * rs, mb * N1, N2, w, N2, 1.0 / (double)N2, ba2);
      return z_backward(A2 + (size_t)(i0 * N1 * Nf) * es, out + (size_t)(i0 * N1 * N2) * rs, mb * N1, N2, Nf);
    }));
  }
  return 0;
}

