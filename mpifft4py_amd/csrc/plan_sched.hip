// plan_sched.hip -- host-only side of a plan: the decomposition bookkeeping (decomp_init), the layout rules that say how
// far apart the rows of the intermediates lie (each with the measurements behind it), the exchange schedules derived
// from both, and the C entry points that answer schedule questions without a device.
#include "plan_impl.h"
#include "relay_plan.h"

using namespace mfft;

namespace {

std::vector<Chunk> pencil_chunks(int64_t n, int size) {   // pencil.py:80-90
  std::vector<Chunk> c(size);
  const int64_t q = n / size, r = n % size;
  for (int i = 0; i < size; ++i) c[i] = Chunk{q + ((r == 1 && i == size - 1) ? 1 : 0), q * i};
  return c;
}

void compute_dims(int n, int* p1, int* p2) {   // MPI.Compute_dims(n, 2): balanced, non-increasing
  int best1 = n, best2 = 1;
  for (int a = 1; a * a <= n; ++a)
    if (n % a == 0) {
      best1 = n / a;
      best2 = a;
    }
  *p1 = best1;
  *p2 = best2;
}

// a schedule into the caller's arrays (any of which may be null)
int copy_out(const Sched& sc, int max_peers, int* npeers, int* peers, size_t* scount, size_t* sdisp, size_t* rcount, size_t* rdisp) {
  *npeers = (int)sc.peers.size();
  if (*npeers > max_peers) return set_error(MFFT_ERR_INVALID, "schedule has %d peers, room for %d", *npeers, max_peers);
  for (int i = 0; i < *npeers; ++i) {
    if (peers) peers[i] = sc.peers[i];
    if (scount) scount[i] = sc.sc[i];
    if (sdisp) sdisp[i] = sc.sd[i];
    if (rcount) rcount[i] = sc.rc[i];
    if (rdisp) rdisp[i] = sc.rd[i];
  }
  return 0;
}

}  // namespace

// ===========================================================================
// layout rules
// ===========================================================================
// Row pitch of a z chunk of `len` columns in the blocks of the FORWARD z-splitting exchange of the Y-ALIGNED pencil
// (round 4).  The rank that holds the Nyquist column has q = 129 (257 ...) columns; its x pass -- in place on the received
// (N0, N1/P2, q) -- then reads rows N1/P2 * q elements apart: 512 * 129 * 16 bytes = 2^20 + 2^13 at 1024^3 on the 4 x 2 grid,
// the slowest pitch there is (xplane_pad: 0.64 against 0.47 ms, profiles/r04_rank_shapes.txt), and the slowest rank sets
// the pace of the transform.  The z kernel therefore writes such rows a whole number of cache lines apart (fft_kernels.h
// ZSplit pitch: 129 -> 136 columns, the chunk of that one destination grows by 5 %), the x pass runs over N1/P2 * 136
// columns (the unused ones ride along), the pitch stays through the second exchange and the y pass reads it.
// NOT for the x-aligned pencil: there only the y pass would see the pitch, and a strided pass that reads line-aligned
// rows but must write compact ones is SLOWER than compact -> compact (scripts/ypass_pitch_ab.py, profiles/r04_ypass_pitch.txt:
// (256, 1024, 257) 0.49 -> 0.56 ms; aligned on both sides it would be 0.41, but the result's layout is the caller's) --
// the y-aligned plan pays the same 0.04 ms in its y pass and wins 0.17 in the x pass.  Only the fused z kernels, only
// chunks of 64 columns and more, only forward.
// Round 5, the x-aligned pencil after all -- for the one case where its y pass gains: chunks whose rows are a multiple of 2^13
// bytes (BASELINE config 5: 1024 complex64 columns per rank of the 4 x 2 grid).  Such rows are line-aligned already; what
// hurts is that the 2048 rows a y transform gathers then lie a power of two apart (the memory-channel hash folds them onto
// few channels): (512, 2048, 1024) axis 1 takes 4.10 ms per rank, 3.82 with the rows one cache line further apart
// (profiles/r04_rank_shapes.txt).  The z kernel leaves that line between its rows, the chunk grows by 1.6 %, the y pass
// reads the pitch and writes the compact blocks of the second exchange as before (a store-side pitch costs nothing).
int64_t mfft_plan_s::zrow_pitch(int64_t len, bool forward) const {
  if (!forward || !zpitch_on || !zfuse || d.drop_nyquist || zc.size() < 2 || len < 64) return len;
  const int64_t per_line = (int64_t)(128 / es);
  if (d.decomp == MFFT_PENCIL_Y) return (len + per_line - 1) / per_line * per_line;
  if (d.decomp == MFFT_PENCIL_X && (len * (int64_t)es) % 8192 == 0) return len + per_line;
  return len;
}

// A strided pass whose rows lie a multiple of 64 KiB apart reads 12 - 30 % slower than one whose rows are one 128-byte
// line further apart (every row of a tile meets the same memory channels; profiles/r02_power_of_two_stride.txt);
// the store side does not care.  Elements to add to such a row stride in an intermediate buffer, 0 when it is harmless.
int64_t mfft_plan_s::plane_pad(int64_t stride_elems) const {
  return (stride_elems * (int64_t)es) % 65536 == 0 ? (int64_t)(128 / es) : 0;
}
// The same idea carried THROUGH an exchange (round 4): the strided x pass that follows an exchange reads the received
// chunks, whose x rows lie N1/P * Nf (slab; N1/P * kz in the kz-slice pipeline), N1/P1 * q (x-aligned pencil, forward) or
// N1/P2 * q (y-aligned pencil, inverse) elements apart.  Measured alone on the device (profiles/r04_xpass_stride_map.txt,
// r04_xpass_kernel_ab.txt; 1024 and 2048 rows, out of place, GB/s of algorithmic traffic against ~5000 for a pitch with
// one more cache line): a power of two 4100 - 4700; 2^a + 2^(a-7) -- the Nyquist-holding ranks of the 4 x 2 pencil grid at
// 1024^3: 512 * 129 elements -- 2100 - 3300 (the memory-channel hash folds address bits seven apart: every row of a tile
// lands on the same channels); 2^a + 2^(a-8) 4100 - 4500 (256 * 257 elements); 2^20 + 2^11 (the slab over 8 ranks:
// 128 * 513) 4600.  For those pitches the transform that WRITES the send blocks leaves one cache line between
// consecutive x rows (a store-side pitch costs nothing), every chunk grows by that line per x row
// (mfft_plan_exchange_schedule / _pieces report it: 64 KiB on a 2 GiB chunk at BASELINE config 5), and the x pass reads
// the padded rows out of place into the caller's compact array: config 5's x pass 5.52 -> 4.46 ms per rank, the y-aligned
// pencil's at 1024^3 0.63 -> 0.47.  MFFT_NO_XPAD=1 switches it off (every rank alike).
// One rank (round 4): the x rows (planes) of a rank's own spectrum lie N1 * Nf elements apart -- for a power-of-two mesh
// N * (N/2 + 1) * es = 2^a + 2^(a - log2 N + 1) bytes, which for N = 256 and 512 (N = 1024 in single precision) is one of
// the pitches the strided x pass reads slowly (slow_pitch_pad).  The caller's array keeps its layout, so the route puts the
// pass that READS it first or last and gives the intermediate planes `lines` cache lines more: forward y out of place into
// padded planes, x out of them into the result; inverse y first (it reads rows, the plane pitch does not matter to it)
// into padded planes, x out of them.  Complex data with power-of-two planes took this route since round 2 (plane_pad) and
// keeps it.  For real data it is OFF: the x pass alone gains 4 - 10 % from the pad when it is timed by itself
// (profiles/r04_xpass_stride_map.txt), inside the transform the pairs of 256^3, 512^3 (fp64, fp32) and 1024^3 fp32 come
// out the same to +-1 % with 0 - 3 lines (profiles/r04_p1_xpad_ab.txt) -- the y pass that has to go first / out of place
// gives back what the x pass wins.  MFFT_P1_XPAD = lines switches it on (read when a plan is created).
int64_t mfft_plan_s::p1_plane_pad() const {
  if (nat_pitch()) return slow_pitch_pad(N1 * Zp);      // pitched rows: 1024 x 520 x 16 B is a multiple of 64 KiB
  if (const int64_t c = r2c ? 0 : plane_pad(N1 * Nf)) return c;
  if (p1_xpad_lines <= 0 || d.line2d) return 0;
  return slow_pitch_pad(N1 * Nf) ? (int64_t)p1_xpad_lines * (int64_t)(128 / es) : 0;
}
int64_t mfft_plan_s::slow_pitch_pad(int64_t stride_elems) const {
  const unsigned long long b = (unsigned long long)stride_elems * (unsigned long long)es;
  if (b < 65536) return 0;                              // small blocks live in the caches
  bool slow = b % 65536 == 0;
  if (!slow && __builtin_popcountll(b) == 2) {
    const int hi = 63 - __builtin_clzll(b), lo = __builtin_ctzll(b);
    slow = hi - lo == 7 || hi - lo == 8 || (hi - lo == 9 && hi <= 20);
  }
  return slow ? (int64_t)(128 / es) : 0;
}
int64_t mfft_plan_s::xplane_pad(bool forward) const {                // one pitch for the whole exchange (not the kz-slice pipeline)
  if (!xpad_on || P == 1 || d.line2d || d.drop_nyquist) return 0;
  if (d.decomp == MFFT_SLAB) return (forward && nbatch <= 1 && nslice <= 1) ? slow_pitch_pad(Np1 * Nf) : 0;
  if (d.decomp == MFFT_PENCIL_X) return (forward && P1 > 1) ? slow_pitch_pad(N1_1 * q) : 0;
  return (!forward && P2 > 1) ? slow_pitch_pad(N2_1 * q) : 0;
}
// kz-slice pipeline of the slab: x-row pitch of slice s in the exchanged layout, and where the slice starts
int64_t mfft_plan_s::slice_pitch(int s, bool forward) const {
  const int64_t w = Np1 * kslice[s].len;
  return w + ((forward && xpad_on) ? slow_pitch_pad(w) : 0);
}
size_t mfft_plan_s::slice_offset(int s, bool forward) const {        // elements of all earlier slices in the send / receive buffers
  size_t o = 0;
  for (int t = 0; t < s; ++t) o += (size_t)(P * Np0 * slice_pitch(t, forward));
  return o;
}

// ===========================================================================
// exchange schedules (host only)
//   slab:   which = 0, equal chunks over all ranks (padded: x extent M0/P)
//   pencil: which = 0 -> the z-splitting exchange (uneven last chunk), X: comm1, Y: comm0
//           which = 1 -> the other exchange (equal chunks),            X: comm0, Y: comm1
// ===========================================================================
int mfft_plan_s::sched(int which, bool forward, bool padded, Sched* o) const {
  auto equal = [&](const std::vector<int>& grp, size_t chunk) {
    const int n = (int)grp.size();
    o->peers = grp;
    o->sc.assign(n, chunk);
    o->rc.assign(n, chunk);
    o->sd.resize(n);
    o->rd.resize(n);
    for (int i = 0; i < n; ++i) o->sd[i] = o->rd[i] = (size_t)i * chunk;
  };
  if (d.decomp == MFFT_SLAB) {
    if (which != 0) return set_error(MFFT_ERR_INVALID, "slab plans have one exchange");
    const int64_t x = padded ? M0 / P : Np0;
    equal(world, (size_t)(x * (Np1 * Nf + (padded ? 0 : xplane_pad(forward)))) * es);
    return 0;
  }
  const bool X = d.decomp == MFFT_PENCIL_X;
  const int64_t m = padded ? M0 / P1 : N1_0, n = padded ? M1 / P2 : N2_1;
  fill_part(which == 0 ? !X : X, &o->part);
  if (which == 0) {
    const std::vector<int>& gz = X ? group1 : group0;
    const int Pz = (int)gz.size();
    o->peers = gz;
    o->sc.resize(Pz); o->sd.resize(Pz); o->rc.resize(Pz); o->rd.resize(Pz);
    size_t off = 0;
    for (int l = 0; l < Pz; ++l) {
      // (the fused 3/2-rule transforms have chunked kernels of their own and keep compact rows: padded -> no pitch)
      const int64_t pl = padded ? zc[l].len : zrow_pitch(zc[l].len, forward), pq = padded ? q : zrow_pitch(q, forward);
      const size_t uneven = (size_t)(m * n * pl) * es, even = (size_t)(m * n * pq) * es;
      if (forward) { o->sc[l] = uneven; o->sd[l] = off; o->rc[l] = even; o->rd[l] = (size_t)l * even; }
      else         { o->sc[l] = even; o->sd[l] = (size_t)l * even; o->rc[l] = uneven; o->rd[l] = off; }
      off += uneven;
    }
    return 0;
  }
  if (which == 1) {
    const int64_t xp = padded ? 0 : xplane_pad(forward);     // one cache line between x rows when they are 64 KiB multiples apart
    if (X) equal(group0, (size_t)(m * (N1_1 * q + xp)) * es);
    else   equal(group1, (size_t)(N2_0 * (n * (padded ? q : zrow_pitch(q, forward)) + xp)) * es);   // forward: the z kernel's row pitch travels on
    return 0;
  }
  return set_error(MFFT_ERR_INVALID, "pencil plans have two exchanges");
}

// Schedule of ONE piece of a pipelined exchange, displacements relative to the whole send / receive buffers:
//   slab, kz slices   : slice s of the packed [s][p][i][j][kz_s] layout (equal chunks)
//   slab, row batches : rows [i0, i0+mb) of every peer block of the packed (P, Np0, Np1, Nf) layout
//   pencil X          : rows [i0, i0+mb) of the blocks of exchange `which`
// An un-pipelined plan has one piece: the whole exchange.
int mfft_plan_s::piece_sched(int which, bool forward, int piece, Sched* o) const {
  if (piece < 0 || piece >= npieces()) return set_error(MFFT_ERR_INVALID, "piece %d of %d", piece, npieces());
  if (npieces() == 1) return sched(which, forward, false, o);
  if (d.decomp == MFFT_SLAB) {
    if (which != 0) return set_error(MFFT_ERR_INVALID, "slab plans have one exchange");
    if (nbatch > 1) {
      const int64_t i0 = Np0 * piece / nbatch, mb = Np0 * (piece + 1) / nbatch - i0;
      o->peers = world;
      o->sc.assign(P, (size_t)(mb * Np1 * Nf) * es);
      o->rc = o->sc;
      o->sd.resize(P);
      o->rd.resize(P);
      // [r][i][j][k] of the packed layout IS row r*Np0 + i of (N0, Np1, Nf): same blocks in both directions
      for (int r = 0; r < P; ++r) o->sd[r] = o->rd[r] = (size_t)((r * Np0 + i0) * Np1 * Nf) * es;
      return 0;
    }
    const size_t boff = slice_offset(piece, forward) * es, chunk = (size_t)(Np0 * slice_pitch(piece, forward)) * es;
    o->peers = world;
    o->sc.assign(P, chunk);
    o->rc = o->sc;
    o->sd.resize(P);
    o->rd.resize(P);
    for (int r = 0; r < P; ++r) o->sd[r] = o->rd[r] = boff + (size_t)r * chunk;
    return 0;
  }
  // X: both exchanges in batches of the m local x rows; Y: the z-splitting exchange in batches of the m local x rows,
  // the x-chunk exchange in batches of the N2_0 rows a rank owns after it
  const int64_t m = (d.decomp == MFFT_PENCIL_Y && which == 1) ? N2_0 : N1_0;
  const int64_t i0 = m * piece / nbatch, mb = m * (piece + 1) / nbatch - i0;
  return sched_rows(which, forward, i0, mb, o);
}

// Sub-schedules of one batch [i0, i0+mb) of the m local rows (bytes):
int mfft_plan_s::sched_rows(int which, bool forward, int64_t i0, int64_t mb, Sched* o) const {
  const int64_t m = N1_0, n = N2_1;
  const bool X = d.decomp == MFFT_PENCIL_X;
  fill_part(which == 0 ? !X : X, &o->part);
  if (which == 0) {            // z-splitting exchange (X: group1, Y: group0): uneven chunks <-> (m, n, q) blocks, rows [i0, i0+mb) of m
    const std::vector<int>& gz = X ? group1 : group0;
    const int Pz = (int)gz.size();
    o->peers = gz;
    o->sc.resize(Pz); o->sd.resize(Pz); o->rc.resize(Pz); o->rd.resize(Pz);
    size_t base = 0;
    const int64_t pq = zrow_pitch(q, forward);
    for (int l = 0; l < Pz; ++l) {
      const int64_t pl = zrow_pitch(zc[l].len, forward);
      const size_t usz = (size_t)(mb * n * pl) * es, uoff = base + (size_t)(i0 * n * pl) * es;
      const size_t esz = (size_t)(mb * n * pq) * es, eoff = (size_t)(l * m * n * pq + i0 * n * pq) * es;
      if (forward) { o->sc[l] = usz; o->sd[l] = uoff; o->rc[l] = esz; o->rd[l] = eoff; }
      else         { o->sc[l] = esz; o->sd[l] = eoff; o->rc[l] = usz; o->rd[l] = uoff; }
      base += (size_t)(m * n * pl) * es;
    }
    return 0;
  }
  if (!X) {
    // Y alignment, x-chunk exchange over group1 (P2 ranks): rows [i0, i0+mb) of the N2_0 rows of every block
    // [c][x'][j][k] (N2_0, n, q); the send block c is rows c*N2_0.. of (N0, n, q), the receive block c' the same shape
    const int Pg = (int)group1.size();
    // x-row pitch (inverse: padded where the compact one reads slowly; forward: rows at the z kernel's pitch)
    const int64_t SY = n * zrow_pitch(q, forward) + xplane_pad(forward);
    o->peers = group1;
    o->sc.assign(Pg, (size_t)(mb * SY) * es);
    o->rc = o->sc;
    o->sd.resize(Pg); o->rd.resize(Pg);
    for (int g = 0; g < Pg; ++g) o->sd[g] = o->rd[g] = (size_t)((g * N2_0 + i0) * SY) * es;
    return 0;
  }
  // X alignment, y-chunk exchange over group0 (P1 ranks): P1 blocks (m, N1_1, q) <-> rows of (N0, N1_1, q)
  const int Pg = (int)group0.size();
  const int64_t SX = N1_1 * q + xplane_pad(forward);        // x-row pitch (forward: padded where the compact one reads slowly)
  o->peers = group0;
  o->sc.assign(Pg, (size_t)(mb * SX) * es);
  o->rc = o->sc;
  o->sd.resize(Pg); o->rd.resize(Pg);
  for (int g = 0; g < Pg; ++g) {
    const size_t blk = (size_t)((g * m + i0) * SX) * es;                     // [g][i][j'][k]
    const size_t row = (size_t)((g * m + i0) * SX) * es;                     // x = g*m + i
    if (forward) { o->sd[g] = blk; o->rd[g] = row; }
    else         { o->sd[g] = row; o->rd[g] = blk; }
  }
  return 0;
}

// host-only part of plan construction: decomposition bookkeeping (no HIP call)
int mfft::decomp_init(mfft_plan_s* p, const mfft_plan_desc* desc, int nranks, int rank) {
  p->d = *desc;
  p->P = nranks;
  p->rank = rank;
  p->prec = desc->precision;
  p->r2c = desc->kind == MFFT_R2C;
  p->N0 = desc->n[0];
  p->N1 = desc->n[1];
  p->N2 = desc->n[2];
  if (nranks < 1 || rank < 0 || rank >= nranks) return set_error(MFFT_ERR_INVALID, "bad rank %d of %d", rank, nranks);
  if (p->N0 < 1 || p->N1 < 1 || p->N2 < 1) return set_error(MFFT_ERR_INVALID, "bad mesh");
  if (desc->precision != MFFT_SINGLE && desc->precision != MFFT_DOUBLE) return set_error(MFFT_ERR_INVALID, "bad precision");
  p->Nf = p->r2c ? p->N2 / 2 + 1 : p->N2;
  p->es = elem_bytes(p->prec, true);
  p->rs = p->r2c ? elem_bytes(p->prec, false) : p->es;
  const double ps = desc->padsize > 0 ? desc->padsize : 1.5;
  p->d.padsize = ps;
  p->M0 = (int64_t)(ps * p->N0);
  p->M1 = (int64_t)(ps * p->N1);
  p->M2 = (int64_t)(ps * p->N2);
  p->Mf = p->r2c ? (int64_t)(ps * p->N2) / 2 + 1 : p->M2;
  p->world.resize(p->P);
  for (int i = 0; i < p->P; ++i) p->world[i] = i;
  p->xpad_on = !env_on("MFFT_NO_XPAD");
  p->xpass_inplace = env_on("MFFT_XPASS_INPLACE");
  p->p1_xpad_lines = (int)env_int("MFFT_P1_XPAD", p->p1_xpad_lines);
  p->zpitch_on = !env_on("MFFT_NO_ZPITCH");
  if (getenv("MFFT_SPLIT_LAST")) p->split_last = env_on("MFFT_SPLIT_LAST") ? 1 : 0;
  p->split_last_yblock = (int)env_int("MFFT_SPLIT_LAST_YBLOCK", p->split_last_yblock);
  p->split_last_yfirst = (int)env_int("MFFT_SPLIT_LAST_YFIRST", p->split_last_yfirst);
  p->split_last_pad_bytes = env_int("MFFT_SPLIT_LAST_PAD", p->split_last_pad_bytes);
  p->split_last_xnear = (int)env_int("MFFT_SPLIT_LAST_XNEAR", p->split_last_xnear);
  p->split_last_xnear_pad_bytes = env_int("MFFT_SPLIT_LAST_XNEAR_PAD", p->split_last_xnear_pad_bytes);
  p->split_last_pairblock = (int)env_int("MFFT_SPLIT_LAST_PAIRBLOCK", p->split_last_pairblock);
  p->split_last_pairxfast = (int)env_int("MFFT_SPLIT_LAST_PAIRXFAST", p->split_last_pairxfast);
  if (getenv("MFFT_PAD_ALIGN")) p->pad_align = env_on("MFFT_PAD_ALIGN") ? 1 : 0;
  p->pad_align_inv = (int)env_int("MFFT_PAD_ALIGN_INV", p->pad_align_inv);
  const int P = p->P;
  if (p->r2c && p->N2 % 2) return set_error(MFFT_ERR_UNSUPPORTED, "odd N[2]=%lld is not supported for R2C", (long long)p->N2);
  p->Zp = 0;                     // complex_pitch: resolved below, once the local z extent is known
  if (desc->decomp == MFFT_SLAB) {
    if (p->N0 % P || p->N1 % P) return set_error(MFFT_ERR_INVALID, "N[0]=%lld and N[1]=%lld must be divisible by the number of ranks %d", (long long)p->N0, (long long)p->N1, P);
    p->Np0 = p->N0 / P;
    p->Np1 = p->N1 / P;
    if (P > 1 && desc->pipeline < 0) {
      p->nbatch = (int)std::min<int64_t>(-(int64_t)desc->pipeline, p->Np0);      // batches of local x rows
    } else if (P > 1) {
      // kz slices for the exchange pipeline: boundaries on 16-column (tile) multiples
      const int want = desc->pipeline > 0 ? desc->pipeline : 4;
      const int64_t unit = 16;
      const int64_t per = (p->Nf / want) / unit * unit;
      if (want > 1 && per >= unit) {
        for (int s = 0; s < want; ++s) {
          const int64_t st = per * s;
          p->kslice.push_back(Chunk{s == want - 1 ? p->Nf - st : per, st});
        }
        p->nslice = want;
      }
    }
  } else if (desc->decomp == MFFT_PENCIL_X || desc->decomp == MFFT_PENCIL_Y) {
    int P1 = desc->p1, P2;
    if (P1 <= 0) compute_dims(P, &P1, &P2);
    else {
      if (P % P1) return set_error(MFFT_ERR_INVALID, "P1=%d does not divide %d ranks", P1, P);
      P2 = P / P1;
    }
    p->P1 = P1;
    p->P2 = P2;
    p->c0 = p->rank % P1;       // comm0 = consecutive ranks (pencil.py:192-195)
    p->c1 = p->rank / P1;
    // real (N0/P1, N1/P2, N2); X: complex (N0, N1/P1, N2/P2-chunk); Y: complex (N0/P2, N1, N2/P1-chunk)
    const bool alignX = desc->decomp == MFFT_PENCIL_X;
    if (p->N0 % P1 || p->N1 % P2 || (alignX ? (p->N1 % P1 || p->N2 % P2) : (p->N0 % P2 || p->N2 % P1)))
      return set_error(MFFT_ERR_INVALID, "mesh not divisible by the %dx%d process grid", P1, P2);
    if (desc->line2d && !(alignX && P1 == 1 && p->N0 == 1 && p->r2c))
      return set_error(MFFT_ERR_INVALID, "line2d is an x-aligned R2C pencil plan of a (1, Nx, Ny) mesh on a 1 x P grid");
    p->N1_0 = p->N0 / P1;
    p->N1_1 = p->N1 / P1;
    p->N2_0 = p->N0 / P2;
    p->N2_1 = p->N1 / P2;
    for (int i = 0; i < P1; ++i) p->group0.push_back(p->c1 * P1 + i);
    for (int i = 0; i < P2; ++i) p->group1.push_back(p->c0 + i * P1);
    const int Pz = desc->decomp == MFFT_PENCIL_X ? P2 : P1;
    const int cz = desc->decomp == MFFT_PENCIL_X ? p->c1 : p->c0;
    if (p->r2c && Pz > 1 && ((p->N2 / Pz) % 2)) return set_error(MFFT_ERR_UNSUPPORTED, "N[2]/%d must be even for the pencil z split", Pz);
    if (p->Nf % Pz > 1) return set_error(MFFT_ERR_UNSUPPORTED, "Nf=%lld cannot be split over %d ranks", (long long)p->Nf, Pz);
    p->zc = pencil_chunks(p->Nf, Pz);
    if (desc->drop_nyquist) {      // 'AlltoallN': equal chunks of the N2/2 non-Nyquist columns
      if (!p->r2c) return set_error(MFFT_ERR_INVALID, "drop_nyquist is an R2C mode");
      p->zc = pencil_chunks(p->N2 / 2, Pz);
    }
    p->q = p->zc[cz].len;
    p->zstart = p->zc[cz].start;
    // z-chunk pack / unpack fused into the z transform when a radix kernel with chunked stores / loads exists
    // (MFFT_NO_ZFUSE: the copy-based path, kept for A/B runs and for the lengths that go through chirp-z)
    p->zfuse = !desc->line2d && getenv("MFFT_NO_ZFUSE") == nullptr &&
               zsplit_supported(p->N2, p->prec, p->r2c) &&
               (!p->r2c || p->N2 % 2 == 0) && p->zc[0].len < 65536;
    // exchange pipeline of the x-aligned pencil: batches of local x rows (`pipeline`, default 4 like the slab's)
    const int want = desc->pipeline > 0 ? desc->pipeline : desc->pipeline < 0 ? -desc->pipeline : 4;
    if (desc->decomp == MFFT_PENCIL_X && want > 1 && P > 1 && !desc->drop_nyquist && !desc->line2d)
      p->nbatch = (int)std::min<int64_t>(want, p->N1_0);
    // ... and of the y-aligned one (pencil_forward_pipelined_y): two halves around the x transform
    if (desc->decomp == MFFT_PENCIL_Y && want > 1 && P1 > 1 && P2 > 1 && p->zfuse && !desc->drop_nyquist)
      p->nbatch = (int)std::min<int64_t>(want, std::min(p->N1_0, p->N2_0));
  } else {
    return set_error(MFFT_ERR_INVALID, "bad decomposition %d", desc->decomp);
  }
  // pitched spectrum (complex_pitch): -1 = whole cache lines, > 0 = that many elements (at least the local z extent)
  if (desc->complex_pitch != 0) {
    int64_t a_, b_, zloc = 0;
    p->cdims(&a_, &b_, &zloc);
    const int64_t line = (int64_t)(128 / p->es);
    const int64_t want = desc->complex_pitch < 0 ? (zloc + line - 1) / line * line : (int64_t)desc->complex_pitch;
    if (want < zloc) return set_error(MFFT_ERR_INVALID, "complex_pitch %lld is shorter than the local z extent %lld", (long long)want, (long long)zloc);
    p->Zp = want;
  }
  // every transform length must have a kernel
  auto need = [&](int64_t n, bool real) -> int {
    if (n == 1 && !real) return 0;
    if (!length_supported(n, real)) return set_error(MFFT_ERR_UNSUPPORTED, "transform length %lld%s is not supported (lengths run from 1 to 2^20: include/mpifft4py_amd.h mfft_length_route)", (long long)n, real ? " (real)" : "");
    return 0;
  };
  MFFT_TRY(need(p->N0, false));
  MFFT_TRY(need(p->N1, false));
  MFFT_TRY(need(p->N2, p->r2c));
  return 0;
}

extern "C" {

// Exchange schedule of a transform, computed WITHOUT a device: which peers a rank
// exchanges with and the byte counts / displacements of every chunk.  This is the
// same code the executor uses (mfft_plan_s::sched); tests drive it from CPU-only
// multi-process runs (gloo) to validate the distributed bookkeeping.
int mfft_plan_exchange_schedule(const mfft_plan_desc* desc, int nranks, int rank, int which, int forward, int padded,
                                int max_peers, int* npeers, int* peers, size_t* scount, size_t* sdisp, size_t* rcount,
                                size_t* rdisp) {
  if (!desc || !npeers) return set_error(MFFT_ERR_INVALID, "null argument");
  mfft_plan_s p;
  MFFT_TRY(decomp_init(&p, desc, nranks, rank));
  Sched sc;
  MFFT_TRY(p.sched(which, forward != 0, padded != 0, &sc));
  return copy_out(sc, max_peers, npeers, peers, scount, sdisp, rcount, rdisp);
}

int mfft_plan_exchange_pieces(const mfft_plan_desc* desc, int nranks, int rank, int which, int forward, int piece,
                              int max_peers, int* npieces, int* npeers, int* peers, size_t* scount, size_t* sdisp,
                              size_t* rcount, size_t* rdisp) {
  if (!desc || !npeers || !npieces) return set_error(MFFT_ERR_INVALID, "null argument");
  mfft_plan_s p;
  MFFT_TRY(decomp_init(&p, desc, nranks, rank));
  *npieces = p.npieces();
  Sched sc;
  MFFT_TRY(p.piece_sched(which, forward != 0, piece, &sc));
  return copy_out(sc, max_peers, npeers, peers, scount, sdisp, rcount, rdisp);
}

// What `rank` pulls, phase by phase, when exchange `which` of a pencil plan runs over the IPC transport with relay
// striping (relay_plan.h) -- device-free, the same enumeration the transport executes (relay_moves): tests replay it on
// host buffers and count the bytes per link.
int mfft_plan_relay_schedule(const mfft_plan_desc* desc, int nranks, int rank, int which, int forward, int max_moves,
                             int* nmoves, int* phase, int* kind, int* from, int* msg_src, int* msg_dst, size_t* msg_off,
                             size_t* bytes) {
  if (!desc || !nmoves) return set_error(MFFT_ERR_INVALID, "null argument");
  if (desc->decomp == MFFT_SLAB) return set_error(MFFT_ERR_INVALID, "slab plans exchange over all ranks: nothing to relay");
  std::vector<size_t> B((size_t)nranks * nranks, 0);
  std::vector<int> part;
  for (int s = 0; s < nranks; ++s) {
    mfft_plan_s p;
    MFFT_TRY(decomp_init(&p, desc, nranks, s));
    Sched sc;
    MFFT_TRY(p.sched(which, forward != 0, false, &sc));
    for (size_t i = 0; i < sc.peers.size(); ++i) B[(size_t)s * nranks + sc.peers[i]] = sc.sc[i];
    if (s == rank) part = sc.part;
  }
  if ((int)part.size() != nranks) return set_error(MFFT_ERR_INTERNAL, "no partition for this exchange");
  std::vector<RelayMove> mv;
  relay_moves(nranks, rank, part.data(), [&](int s, int d) { return B[(size_t)s * nranks + d]; }, &mv);
  *nmoves = (int)mv.size();
  if (*nmoves > max_moves) return set_error(MFFT_ERR_INVALID, "relay schedule has %d moves, room for %d", *nmoves, max_moves);
  for (int i = 0; i < *nmoves; ++i) {
    if (phase) phase[i] = mv[i].phase;
    if (kind) kind[i] = mv[i].kind;
    if (from) from[i] = mv[i].from;
    if (msg_src) msg_src[i] = mv[i].msg_src;
    if (msg_dst) msg_dst[i] = mv[i].msg_dst;
    if (msg_off) msg_off[i] = mv[i].msg_off;
    if (bytes) bytes[i] = mv[i].bytes;
  }
  return 0;
}

}  // extern "C"
