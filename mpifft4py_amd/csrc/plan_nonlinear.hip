// plan_nonlinear.hip -- the nonlinear term of a pseudo-spectral step as one plan-level operation.
#include <cmath>
#include "plan_impl.h"
#include "fft_nlz.h"
#include "nlz_moments.h"

using namespace mfft;

// ===========================================================================
// Round 6: the nonlinear term of a pseudo-spectral step, out = fftn(ifftn(a) x ifftn(b)), as ONE plan-level operation
// (what demo/spectral_dns_solver.py:53-71 composes from six ifftn, a cross product in real space and three fftn).
// ===========================================================================
extern "C" int mfft_ew_cross(mfft_plan_t plan, const void* a, const void* b, void* out, size_t n, int precision);
extern "C" int mfft_ew_dot(mfft_plan_t plan, const void* a, const void* b, void* out, size_t n, int precision);
extern "C" int mfft_ew_mul(mfft_plan_t plan, const void* a, const void* b, void* out, size_t n, int precision);
// Three products (mfft_internal.h NL_PRODUCTS) share every route below: the cross product (three result components); the dot
// product sum_f ifftn(a_f) ifftn(b_f) of a transported scalar's u . grad(theta) (ONE result component: nout = 1 -- one forward y
// pass, one forward exchange, one forward x pass; seven work arrays instead of nine in the composition); and both at once for a
// velocity that carries a scalar, a x b AND sum_f a_f c_f with a third field c -- NINE fields in (nin), FOUR results (the scalar
// one, `outs`, is the fourth): ifftn(a) is computed once where the two calls compute it twice.
// The outer product, all nine a_i b_j (the Elsasser products of MHD, a stress u_i u_j): six fields in, NINE results -- the first
// product with nout > nin, so the fused routes size their buffers and batches by max(nin, nout) fields: the z kernel writes results
// 0..5 in place on the six inputs and 6..8 into three more fields of the batch, nine forward passes follow.
// The routes read nin and nout from the table of products (mfft_internal.h NlProduct) and the caller's arrays through NlFields;
// only the composed route, which chooses the element-wise products, names a product.
// The REDUCTIONS are the table's entries with nout == 0 (moments, histograms, quadratic forms, increments, joint histograms, profiles): the
// fused routes run their inverse passes and end the z stage in reduce_batch -- nothing forward is launched -- and a call is
// real_reduce: mask, begin, fused or reduce_composed, end.  What a new kind supplies: its header (nlz_*.h: parameters, rule, body), its row of NL_PRODUCTS and its kernels'
// registration; its members of NlrCall with their copy and checks in launch_nlr, its partials' size and its fold (core.hip); its
// sweep over a real array for reduce_composed; *_begin / *_end around its accumulator; its real_* entry.

int64_t mfft_plan_s::local_real_count(bool padded) const {
  if (d.line2d) return 0;
  if (d.decomp == MFFT_SLAB) return padded ? (int64_t)(d.padsize * Np0) * M1 * M2 : Np0 * N1 * N2;
  return padded ? (int64_t)(d.padsize * N1_0) * (int64_t)(d.padsize * N2_1) * M2 : N1_0 * N2_1 * N2;
}

// Composed route (every decomposition and length): the transforms the caller would run, on nine (dot product: seven) work
// arrays of the plan: the nin real fields, then the results.
// Both products: twelve -- the dot product of a and c goes over c_0 (mfft_ew_dot allows it), the cross product into three more
// arrays (mfft_ew_cross does not alias).
// The outer product: seven -- the six real fields and ONE more, which takes each product a_i b_j in turn (mfft_ew_mul) and is
// transformed forward before the next.
int mfft_plan_s::nonlinear_composed(const NlFields& u, int dealias, Op product, bool stats) {
  const NlProduct& q = nl_product(product);
  const int nout = q.nout, nin = q.nin;
  const bool both = product == Op::CrossDot, dot = product == Op::Dot;
  const bool pad = dealias == MFFT_DEALIAS_3_2, masked = dealias == MFFT_DEALIAS_2_3;
  const int64_t nr = local_real_count(pad), nc = local_complex_alloc();       // (pitched arrays: a component is that much larger)
  if (nr <= 0 || !r2c) return set_error(MFFT_ERR_UNSUPPORTED, "nonlinear_%s needs a 3-D real-to-complex plan", q.name);
  const bool outer = product == Op::Outer;
  const int narr = both ? 12 : outer ? 7 : nin + nout;
  MFFT_TRY(ensure(nlr, (size_t)(narr * nr) * rs));
  char* R = static_cast<char*>(nlr.p);
  auto arr = [&](int k) { return R + (size_t)(k * nr) * rs; };
  auto back = [&](const void* in, void* o) { return exec(false, in, o, dealias); };
  auto fwd = [&](const void* in, void* o) { return exec(true, in, o, masked ? (int)MFFT_DEALIAS_NONE : dealias); };
  for (int f = 0; f < 3; ++f)                      // (component by component, as before: a_f, b_f, then c_f)
    for (int g = 0; g < nin / 3; ++g) MFFT_TRY(back(u.src(3 * g + f, nc, es), arr(3 * g + f)));
  // statistics: the six real arrays exist here, one streaming sweep over them (absmax.hip) into the same accumulator
  if (stats) MFFT_TRY(stage("nl_absmax", 6.0 * (double)nr * rs, [&] { return absmax_sweep(R, 6, (size_t)nr, static_cast<double*>(nlmacc.p)); }));
  // the element-wise products and where their results lie: res[f] is the work array forward transform f starts from
  int res[4] = {6, 7, 8, 0};
  if (outer) {
    for (int c = 0; c < nout; ++c) {
      MFFT_TRY(stage("nl_mul", 3.0 * (double)nr * rs, [&] { return mfft_ew_mul(this, arr(c / 3), arr(3 + c % 3), arr(6), (size_t)nr, prec); }));
      MFFT_TRY(fwd(arr(6), u.dst(c, nc, es)));
    }
    return 0;
  }
  if (both) {
    MFFT_TRY(stage("nl_dot", 7.0 * (double)nr * rs, [&] { return mfft_ew_dot(this, arr(0), arr(6), arr(6), (size_t)nr, prec); }));
    MFFT_TRY(stage("nl_cross", 9.0 * (double)nr * rs, [&] { return mfft_ew_cross(this, arr(0), arr(3), arr(9), (size_t)nr, prec); }));
    res[0] = 9; res[1] = 10; res[2] = 11; res[3] = 6;
  } else {
    MFFT_TRY(stage(dot ? "nl_dot" : "nl_cross", (6.0 + nout) * (double)nr * rs, [&] {
      return (dot ? mfft_ew_dot : mfft_ew_cross)(this, arr(0), arr(3), arr(6), (size_t)nr, prec);
    }));
  }
  for (int f = 0; f < nout; ++f) MFFT_TRY(fwd(arr(res[f]), u.dst(f, nc, es)));
  return 0;
}

// x planes per batch of the fused routes: `planes` planes whose six y-pass outputs take plane6 bytes each, cut into
// equal batches of at most MFFT_NLZ_BATCH_MB (read once per process; default 16 GiB, see nonlinear_fused)
static int64_t nlz_batch_planes(size_t plane6, int64_t planes) {
  static const long batch_mb = env_int("MFFT_NLZ_BATCH_MB", 16384);
  const int64_t nbat = (int64_t)((plane6 * (size_t)planes + ((size_t)batch_mb << 20) - 1) / ((size_t)batch_mb << 20));
  return (planes + std::max<int64_t>(nbat, 1) - 1) / std::max<int64_t>(nbat, 1);
}

// the fused z stage on a batch: rows of the six fields in Y (yelems apart, pitch Za) in, the three rows of the cross product
// (the one row of the dot product) out, in place on the first three (the first); both products: nine fields in, four rows out
// (stats: the Build::AbsMax kernel, its partial maxima into nlm, folded into the plan's accumulator with 1 / L2 -- the kernel's
// inverse transforms are un-normalised -- after the launch: the maxima accumulate over the batches)
static int nlz_rows(mfft_plan_s* p, char* Y, size_t yelems, int64_t L2, int64_t Za, int64_t nrows, int valid_in, Op product, bool stats) {
  NlzArgs z;
  int64_t waves = 0;
  if (stats) {
    waves = nlz_absmax_waves(L2, p->prec, product, nrows);
    if (waves < 1) return set_error(MFFT_ERR_INTERNAL, "no fused z kernel with maxima of length %lld", (long long)L2);
    MFFT_TRY(p->ensure(p->nlm, absmax_fold_scratch_bytes() + (size_t)waves * NLM_SLOTS * p->rs));
    z.part = static_cast<char*>(p->nlm.p) + absmax_fold_scratch_bytes();
  }
  const NlProduct& q = nl_product(product);
  auto Yf = [&](int f) { return Y + (size_t)f * yelems * p->es; };
  for (int f = 0; f < 3; ++f) {
    z.a[f] = Yf(f);
    z.b[f] = Yf(3 + f);
    if (q.nin > 6) z.c[f] = Yf(6 + f);
  }
  for (int f = 0; f < q.nout; ++f) z.out[f] = Yf(f);      // (four results: the scalar row over b_0; nine: 6..8 in three more fields)
  z.product = product;
  z.n = (int)L2; z.prec = p->prec; z.in_stride = Za; z.out_stride = Za; z.nrows = nrows; z.valid = (int)p->Nf;
  z.valid_in = valid_in;
  z.scale = 1.0 / ((double)L2 * (double)L2);
  MFFT_TRY(launch_nlz(z, p->stream));
  if (stats)      // 2 * waves groups of [a, b][field]: period 6, the accumulator's order
    MFFT_TRY(absmax_fold(z.part, (size_t)(2 * waves), 6, p->prec, 1.0 / (double)L2, static_cast<double*>(p->nlm.p),
                         static_cast<double*>(p->nlmacc.p), p->stream));
  return 0;
}

// The z stage that ends in a reduction, on a batch: rows of the call's fields in Y (yelems apart, pitch Za) in, bound to their
// slots; the call's parameters from nlcall; the partial results of each launch into nlm, folded into the kind's accumulator (its
// *_begin cleared it) after the launch, so that the statistics accumulate over the batches (core.hip nlr_rows).  The inverse z
// transform is un-normalised: norm = 1 / L2.
int mfft_plan_s::reduce_batch(Op kind, const NlFields& u, char* Y, size_t yelems, int64_t L2, int64_t Za, int64_t nrows, int valid_in) {
  NlrArgs z;
  z.kind = kind;
  z.call = nlcall;
  for (int f = 0; f < u.nfields; ++f) {
    const int slot = nls_slot(u, f);
    (slot % 2 ? z.b : z.a)[slot / 2] = Y + (size_t)f * yelems * es;
  }
  z.npairs = (u.nfields + 1) / 2;
  z.n = (int)L2; z.prec = prec; z.in_stride = Za; z.nrows = nrows; z.valid = (int)Nf; z.valid_in = valid_in;
  z.norm = 1.0 / (double)L2;
  NlrShape shape;
  MFFT_TRY(nlr_launch_shape(kind, L2, prec, nrows, &shape));
  MFFT_TRY(ensure(nlm, nlr_part_bytes(z, shape)));
  z.part = nlm.p;
  Buf& acc = kind == Op::Histogram ? nlhacc : kind == Op::JointHistogram ? nljacc : kind == Op::Increments ? nliacc : kind == Op::Profiles ? nlpacc : kind == Op::IncrementHistogram ? nlkacc : nlsacc;
  return nlr_rows(z, acc.p, nlhacc.p, stream);      // (the counts of a quadratic form: the second accumulator)
}

// Fused route: one rank, slab, real data, radix kernels on every axis.
bool mfft_plan_s::nonlinear_fusable(int dealias, Op product, bool stats) const {
  static const bool off = env_on("MFFT_NO_NLZ"), ranks_off = env_on("MFFT_NO_NLZ_RANKS");      // read once per process
  if (off || d.decomp != MFFT_SLAB || !r2c || d.line2d || d.drop_nyquist || N0 < 2 || N1 < 2 || N2 < 2) return false;
  if (P > 1 && (ranks_off || pitched() || (dealias == MFFT_DEALIAS_3_2 && P > N0 / 2))) return false;
  if (stats && !nlz_supported(dealias == MFFT_DEALIAS_3_2 ? M2 : N2, prec, product, true)) return false;
  if (dealias == MFFT_DEALIAS_3_2) return can_fuse_pad() && nlz_supported(M2, prec, product);
  auto plain_ok = [&](int64_t n) {
    return n < 65536 && find_kernel(FAM_COL, (int)n, prec, 0) && find_kernel(FAM_COL, (int)n, prec, 1);
  };
  if (!plain_ok(N0) || !plain_ok(N1) || !nlz_supported(N2, prec, product)) return false;
  if (dealias == MFFT_DEALIAS_2_3) return mask_set() && mask_fusable(N0, prec);
  return dealias == MFFT_DEALIAS_NONE;
}

// The six spectra go through their inverse x passes into (L0, N1, Za) buffers of the plan (L = the padded mesh under the
// 3/2-rule; Za = the row pitch, whole cache lines where rows are long).  Everything after that is local to an x plane, so
// batches of x planes then run: inverse y pass of the six fields -> NlzFft (six z rows in, the three rows of the cross
// product out, in place on the first three) -> forward y pass of the three results back into the x-pass buffers, whose
// planes of that batch are free by then.  Three forward x passes finish.  The real-space arrays never exist; the batch
// buffers are at most 16 GiB (1024^3 with the 3/2-rule: 6 x 13.1 GB of x-pass buffers + 14.7 GB of batch buffers, where the
// composed route needs 9 x 29 GB of real work arrays).
// The dot product: the same with ONE result -- the z kernel writes the rows of the dot product in place on the first field, one forward
// y pass per batch, one forward x pass.
// Both products: nine fields through the inverse passes, the z kernel's four result rows in place on the first four (the cross
// product over a, the scalar row over b_0), four forward passes.
int mfft_plan_s::nonlinear_fused(const NlFields& u, int dealias, Op product, bool stats) {
  const int nout = nl_product(product).nout, nin = u.nin(nl_product(product));
  const bool pad = dealias == MFFT_DEALIAS_3_2, masked = dealias == MFFT_DEALIAS_2_3;
  const Op ld = pad ? Op::PadLoad : Op::Plain, st = pad ? Op::TruncStore : Op::Plain;      // the 3/2-rule's passes pad on load, truncate on store
  const int64_t L0 = pad ? M0 : N0, L1 = pad ? M1 : N1, L2 = pad ? M2 : N2;
  const int64_t line = (int64_t)(128 / es);
  static const int align_mode = (int)env_int("MFFT_NLZ_ALIGN", -1);     // 0 compact rows, 1 aligned, unset: rows of 2 KiB and more
  const bool aligned = align_mode > 0 || (align_mode < 0 && Nf * (int64_t)es >= 2048);
  const int64_t Zi = Zc();                         // row pitch of the caller's arrays
  const int64_t Za = nat_pitch() ? Zp : aligned ? (Nf + line - 1) / line * line : Nf;
  const int64_t C = N0 * N1 * Zi;                  // elements of one component of the caller's arrays
  const size_t xelems = (size_t)(L0 * N1 * Za);    // ... of one x-pass buffer
  // Batch of x planes.  Large batches win (512^3 with the 3/2-rule, ms per Runge-Kutta step against the MiB of a batch's six
  // y-pass outputs: 80: 181, 160: 157, 320: 143, 640: 130, 1536: 117, 6000: 111 -- batches that would fit the 256 MB Infinity Cache
  // gain nothing from it and pay for their short launches: profiles/r06_dns_batch.txt), so: batches of 16 GiB -- ONE batch up to
  // 512^3 with the 3/2-rule (14.9 GB), four at 768^3, eight at 1024^3 (14.7 GB of batch buffers beside 78.5 GB of x-pass
  // buffers).  MFFT_NLZ_BATCH_MB overrides.
  const int nf = std::max(nin, nout);                     // fields of the buffers: the outer product has more results than inputs
  const size_t plane6 = (size_t)(nf * L1 * Za) * es;      // (the bytes of a plane of every field: six, or nine)
  const int64_t mb = std::min(std::max<int64_t>(nlz_batch_planes(plane6, L0), 1), L0);
  MFFT_TRY(ensure(nlx, (size_t)nf * xelems * es));
  MFFT_TRY(ensure(nly, (size_t)mb * plane6));
  const size_t yelems = (size_t)(mb * L1 * Za);
  // field f of the x-pass buffers from element `off` of it on, of the batch buffers; where the batch of planes from i0 on starts
  auto Xf = [&, X = static_cast<char*>(nlx.p)](int f, size_t off = 0) { return X + ((size_t)f * xelems + off) * es; };
  auto Yf = [&, Y = static_cast<char*>(nly.p)](int f) { return Y + (size_t)f * yelems * es; };
  auto batch = [&](int64_t i0) { return (size_t)(i0 * N1 * Za); };
  const double sc3 = pad ? padscale() : 1.0;
  const double Cb = (double)C * es, Xb = (double)(L0 * N1 * Nf) * es, Yb = (double)(L0 * L1 * Nf) * es;
  MaskScope mask_scope{this};
  lband_use = false;
  // 2/3-rule with the reference's own filter (detect_band): the six inverse transforms are PRUNED as in slab_backward -- the x
  // pass neither loads the removed kx rows nor touches the removed ky and kz columns, the y pass works on the kept kz columns
  // and does not load the removed ky rows, the fused z kernel reads ba2 bins per row (NlzParams::valid_in) and stores all Nf.
  // 512^3, per Taylor-Green step: nl_x_inv 12.9 -> 5.9 ms, nl_y_inv 9.3 -> 5.2, nl_z 8.2 -> 7.1; step 60.3 -> 45.5 ms
  // (profiles/r06_dns_23rule.txt).  MFFT_NO_PRUNE=1: the masked loads below.
  const bool pruned = masked && band_ok && prune_enabled();
  double keep0 = 1.0, keep1 = 1.0, keep2 = 1.0;
  if (pruned) band_keep(&keep0, &keep1, &keep2);
  MFFT_TRY(stage("nl_x_inv", nin * (Cb * keep0 + Xb) * keep1 * keep2, [&] {
    for (int f = 0; f < nin; ++f) {
      const void* src = u.src(f, C, es);
      void* dst = Xf(f);
      if (pruned) {                                // one outer batch per ky, the kept kz columns of it
        ColArgs::Band bx;
        bx.row_lo = ba0; bx.row_hi = bb0; bx.g_off = 0; bx.g_step = 1; bx.g_lo = ba1; bx.g_hi = bb1;
        MFFT_TRY(col_band(src, dst, N0, N1, ba2, Zi, plain(N1 * Zi), Za, plain(N1 * Za), bx));
      } else if (masked) {                                // `fu * dealias` (slab.py:237-245) applied while the spectrum is loaded
        mask_src = src;
        MFFT_TRY(col(src, dst, N0, true, N1, Nf, Zi, plain(N1 * Zi), Za, plain(N1 * Za)));
        mask_src = nullptr;
      } else if (Zi == Za && Za != Nf) {           // pitched caller rows: whole planes of N1 * Za columns
        MFFT_TRY(col_pad(src, dst, L0, true, ld, false, 1, N1 * Za, 0, plain(N1 * Za), 0, plain(N1 * Za), sc3 / (double)L0));
      } else if (Za != Nf) {                       // one outer batch per y row: compact rows in, pitched rows out
        MFFT_TRY(col_pad(src, dst, L0, true, ld, false, N1, Nf, Nf, plain(N1 * Nf), Za, plain(N1 * Za), sc3 / (double)L0,
                         0, 0, 1));
      } else {
        MFFT_TRY(col_pad(src, dst, L0, true, ld, false, 1, N1 * Nf, 0, plain(N1 * Nf), 0, plain(N1 * Nf), sc3 / (double)L0));
      }
    }
    return 0;
  }));
  for (int64_t i0 = 0; i0 < L0; i0 += mb) {
    const int64_t m = std::min(mb, L0 - i0);
    const double frac = (double)m / (double)L0;
    MFFT_TRY(stage("nl_y_inv", nin * (Xb * keep1 + Yb) * keep2 * frac, [&] {
      for (int f = 0; f < nin; ++f) {
        const void* src = Xf(f, batch(i0));
        void* dst = Yf(f);
        if (pruned) {
          ColArgs::Band by;
          by.row_lo = ba1; by.row_hi = bb1; by.c_lim = ba2;
          MFFT_TRY(col_band(src, dst, N1, m, ba2, N1 * Za, plain(Za), L1 * Za, plain(Za), by));
        } else {
          MFFT_TRY(col_pad(src, dst, L1, true, ld, false, m, Nf, N1 * Za, plain(Za), L1 * Za, plain(Za), 1.0 / (double)L1));
        }
      }
      return 0;
    }));
    MFFT_TRY(stage("nl_z", (nin * keep2 + nout) * Yb * frac, [&] {
      if (nout == 0) return reduce_batch(product, u, Yf(0), yelems, L2, Za, m * L1, pruned ? ba2 : 0);
      return nlz_rows(this, Yf(0), yelems, L2, Za, m * L1, pruned ? ba2 : 0, product, stats);
    }));
    if (nout) MFFT_TRY(stage("nl_y_fwd", nout * (Xb + Yb) * frac, [&] {
      for (int f = 0; f < nout; ++f)
        MFFT_TRY(col_pad(Yf(f), Xf(f, batch(i0)), L1, false, st, pad, m, Nf, L1 * Za, plain(Za), N1 * Za, plain(Za), 1.0));
      return 0;
    }));
  }
  if (nout) MFFT_TRY(stage("nl_x_fwd", nout * (Cb + Xb), [&] {
    for (int f = 0; f < nout; ++f) {
      const void* src = Xf(f);
      void* dst = u.dst(f, C, es);
      if (Zi == Za && Za != Nf)                    // pitched result
        MFFT_TRY(col_pad(src, dst, L0, false, st, pad, 1, N1 * Za, 0, plain(N1 * Za), 0, plain(N1 * Za), 1.0 / sc3));
      else if (Za != Nf)                           // tiles of the compact result; input column (y, z) sits at y * Za + z
        MFFT_TRY(col_pad(src, dst, L0, false, st, pad, 1, N1 * Nf, 0, plain(N1 * Za), 0, plain(N1 * Nf), 1.0 / sc3, Nf, Za - Nf));
      else
        MFFT_TRY(col_pad(src, dst, L0, false, st, pad, 1, N1 * Nf, 0, plain(N1 * Nf), 0, plain(N1 * Nf), 1.0 / sc3));
    }
    return 0;
  }));
  return 0;
}

// The same over several ranks of a slab plan (blocking exchanges, whatever pipeline the plan's transforms use): six inverse x
// passes, six all-to-alls, then batches of the rank's x planes -- inverse y passes reading the receive layout through the
// two-level row map (transpose_Uc fused, maths.pyx:21-31), the fused z kernel, forward y passes writing the packed send
// layout (slab.py:403) -- three all-to-alls, three forward x passes.  Nine exchanges as in the composition, no real arrays.
// (The dot product: six inverse exchanges and one forward exchange.)
// (Both products: nine inverse exchanges and four forward ones.)
int mfft_plan_s::nonlinear_fused_ranks(const NlFields& u, int dealias, Op product, bool stats) {
  const int nout = nl_product(product).nout, nin = u.nin(nl_product(product));
  const bool pad = dealias == MFFT_DEALIAS_3_2, masked = dealias == MFFT_DEALIAS_2_3;
  const Op ld = pad ? Op::PadLoad : Op::Plain, st = pad ? Op::TruncStore : Op::Plain;      // the 3/2-rule's passes pad on load, truncate on store
  const int64_t L0 = pad ? M0 : N0, L1 = pad ? M1 : N1, L2 = pad ? M2 : N2, Lp0 = L0 / P;
  const int64_t line = (int64_t)(128 / es);
  const int64_t Za = Nf * (int64_t)es >= 2048 ? (Nf + line - 1) / line * line : Nf;        // batch buffers: line-aligned rows
  const int64_t S = Np1 * Nf + (pad ? 0 : xplane_pad(true));      // x-row pitch of the forward exchange's layout (sched())
  const int64_t C = N0 * Np1 * Nf;                                 // one component of the caller's arrays
  const size_t xelems = (size_t)(L0 * S);                          // one field in any of the exchanged layouts
  const int nf = std::max(nin, nout);                     // fields of the buffers: the outer product has more results than inputs
  const size_t plane6 = (size_t)(nf * L1 * Za) * es;      // (the bytes of a plane of every field: six, or nine)
  const int64_t mb = nlz_batch_planes(plane6, Lp0);
  MFFT_TRY(ensure(nlw[0], (size_t)nf * xelems * es));
  MFFT_TRY(ensure(nlw[1], (size_t)nf * xelems * es));
  MFFT_TRY(ensure(nly, (size_t)mb * plane6));
  const size_t yelems = (size_t)(mb * L1 * Za);
  // field f of the two exchange buffers from element `off` of it on, of the batch buffers; where the batch of planes from i0 on
  // starts in a layout of x rows `pitch` apart
  auto Xf = [&, X = static_cast<char*>(nlw[0].p)](int f, size_t off = 0) { return X + ((size_t)f * xelems + off) * es; };
  auto Rf = [&, R = static_cast<char*>(nlw[1].p)](int f, size_t off = 0) { return R + ((size_t)f * xelems + off) * es; };
  auto Yf = [&, Y = static_cast<char*>(nly.p)](int f) { return Y + (size_t)f * yelems * es; };
  auto batch = [&](int64_t i0, int64_t pitch) { return (size_t)(i0 * pitch); };
  const double sc3 = pad ? padscale() : 1.0;
  MaskScope mask_scope{this};
  lband_use = false;
  // 2/3-rule with the reference's own filter: the six inverse transforms pruned as in slab_backward's blocking route -- the x
  // pass reads the kept kx rows and writes (N0, Np1, ap) with the kept kz only (zeros for the ky this rank's mask removes), the
  // six inverse exchanges carry ap / Nf of the bytes, the y pass and the fused z kernel work on a2 bins per row
  const int64_t a2 = ba2, ap = (a2 + line - 1) / line * line;      // rows of the pruned layout start on cache lines
  const bool pruned = masked && band_ok && ap <= Nf && prune_enabled();
  MFFT_TRY(stage("nl_x_inv", 0, [&] {
    for (int f = 0; f < nin; ++f) {
      const void* src = u.src(f, C, es);
      void* dst = Xf(f);
      if (pruned) {
        if (band_allzero) {                        // nothing of this rank's spectrum survives the mask
          MFFT_TRY(zero(dst, (size_t)(N0 * Np1 * ap) * es));
        } else {
          ColArgs::Band bx;
          bx.row_lo = ba0; bx.row_hi = bb0; bx.g_off = 0; bx.g_step = 1; bx.g_lo = ba1; bx.g_hi = bb1; bx.g_zero = 1;
          MFFT_TRY(col_band(src, dst, N0, Np1, a2, Nf, plain(Np1 * Nf), ap, plain(Np1 * ap), bx));
        }
      } else if (masked) {
        mask_src = src;
        MFFT_TRY(col(src, dst, N0, true, 1, Np1 * Nf, 0, plain(Np1 * Nf), 0, plain(Np1 * Nf)));
        mask_src = nullptr;
      } else {
        MFFT_TRY(col_pad(src, dst, L0, true, ld, false, 1, Np1 * Nf, 0, plain(Np1 * Nf), 0, plain(Np1 * Nf), sc3 / (double)L0));
      }
    }
    return 0;
  }));
  MFFT_TRY(stage("nl_a2a_inv", 0, [&] {
    for (int f = 0; f < nin; ++f) {
      if (pruned) MFFT_TRY(exchange_equal(world, Xf(f), Rf(f), (size_t)(Np0 * Np1 * ap) * es));
      else MFFT_TRY(xchg(0, false, pad, Xf(f), Rf(f)));
    }
    return 0;
  }));
  for (int64_t i0 = 0; i0 < Lp0; i0 += mb) {
    const int64_t m = std::min(mb, Lp0 - i0);
    MFFT_TRY(stage("nl_y_inv", 0, [&] {
      for (int f = 0; f < nin; ++f) {
        if (pruned)
          MFFT_TRY(col(Rf(f, batch(i0, Np1 * ap)), Yf(f), N1, true, m, a2, Np1 * ap, two_level(Np1, Np0 * Np1 * ap, ap), L1 * Za, plain(Za)));
        else
          MFFT_TRY(col_pad(Rf(f, batch(i0, Np1 * Nf)), Yf(f), L1, true, ld, false, m, Nf, Np1 * Nf, two_level(Np1, Lp0 * Np1 * Nf, Nf), L1 * Za,
                           plain(Za), 1.0 / (double)L1));
      }
      return 0;
    }));
    MFFT_TRY(stage("nl_z", 0, [&] {
      if (nout == 0) return reduce_batch(product, u, Yf(0), yelems, L2, Za, m * L1, pruned ? (int)a2 : 0);
      return nlz_rows(this, Yf(0), yelems, L2, Za, m * L1, pruned ? (int)a2 : 0, product, stats);
    }));
    if (nout) MFFT_TRY(stage("nl_y_fwd", 0, [&] {      // truncate + fold in y, straight into the packed (P, Lp0, S) send layout
      for (int f = 0; f < nout; ++f)
        MFFT_TRY(col_pad(Yf(f), Xf(f, batch(i0, S)), L1, false, st, pad, m, Nf, L1 * Za, plain(Za), S, two_level(Np1, Lp0 * S, Nf), 1.0));
      return 0;
    }));
  }
  if (nout) MFFT_TRY(stage("nl_a2a_fwd", 0, [&] {
    for (int f = 0; f < nout; ++f) MFFT_TRY(xchg(0, true, pad, Xf(f), Rf(f)));
    return 0;
  }));
  if (nout) MFFT_TRY(stage("nl_x_fwd", 0, [&] {
    for (int f = 0; f < nout; ++f)
      MFFT_TRY(col_pad(Rf(f), u.dst(f, C, es), L0, false, st, pad, 1, Np1 * Nf, 0, plain(S), 0, plain(Np1 * Nf), 1.0 / sc3));
    return 0;
  }));
  return 0;
}

// stats: the call also leaves max |ifftn(a_f, dealias)|, max |ifftn(b_f, dealias)| over this rank's part of the real-space grid
// the product is formed on (the padded one under the 3/2-rule) in the plan's accumulator, nlmacc[0..5] = [a, b][f]: cleared on
// the stream here, raised by every batch's fold (or the composed route's sweep), read by nonlinear_absmax.  A call without
// stats does not touch it.
int mfft_plan_s::nonlinear(const NlFields& u, int dealias, Op product, bool stats) {
  const NlProduct& q = nl_product(product);
  if ((stats && !q.absmax) || (q.nin > 6 && !u.c) || (q.nout > u.nres && !u.outs))
    return set_error(MFFT_ERR_INVALID, "nonlinear_%s: %d fields in, %d components out, %s", q.name, q.nin, q.nout, q.absmax ? "statistics" : "no statistics");
  if (dealias == MFFT_DEALIAS_2_3) MFFT_TRY(require_mask());
  if (stats) {
    MFFT_TRY(ensure(nlmacc, 12 * sizeof(double)));
    MFFT_HIP(hipMemsetAsync(nlmacc.p, 0, 6 * sizeof(double), stream));
    nlm_valid = false;          // cleared, and partial until every batch has folded: valid only once the route has enqueued it all
  }
  const int rc = nonlinear_fusable(dealias, product, stats)
                     ? (P == 1 ? nonlinear_fused(u, dealias, product, stats) : nonlinear_fused_ranks(u, dealias, product, stats))
                     : nonlinear_composed(u, dealias, product, stats);
  if (stats && rc == 0) nlm_valid = true;
  return rc;
}
int mfft_plan_s::nonlinear_absmax(double out6[6]) {
  if (!nlm_valid) return set_error(MFFT_ERR_INVALID, "no nonlinear operation with statistics has run on this plan");
  MFFT_HIP(hipMemcpyAsync(out6, nlmacc.p, 6 * sizeof(double), hipMemcpyDeviceToHost, stream));
  MFFT_HIP(hipStreamSynchronize(stream));
  return 0;
}

// The reductions: statistics of x = ifftn(field, dealias) of up to six spectra over this rank's part of the grid a product would be
// formed on (the padded one under the 3/2-rule, the masked field under the 2/3-rule).  A call is: its own arguments checked, the
// mask, begin (the kind's accumulator cleared on the stream, the call's parameters parked in nlcall), the route, end (the
// accumulator read back: this synchronises the plan's stream), the result taken out of slot order.  Everything is checked before
// anything is enqueued; the inputs are preserved.  The route is the products': fused, their inverse passes and the z stage that ends
// in the kind's reduction (reduce_batch above; no real array); composed (pencils, lengths without a kernel, MFFT_NO_NLZ), below.
template <class Begin, class End>
int mfft_plan_s::real_reduce(const NlFields& u, int dealias, Op kind, int64_t* count, Begin begin, End end) {
  if (dealias == MFFT_DEALIAS_2_3) MFFT_TRY(require_mask());
  MFFT_TRY(begin());
  MFFT_TRY(nonlinear_fusable(dealias, kind, false)
               ? (P == 1 ? nonlinear_fused(u, dealias, kind, false) : nonlinear_fused_ranks(u, dealias, kind, false))
               : reduce_composed(u, dealias, kind));
  MFFT_TRY(end());
  *count = local_real_count(dealias == MFFT_DEALIAS_3_2);
  return 0;
}
// Composed route: the statistics are per field, so ONE real work array serves the fields in turn -- inverse transform into nlr, the
// kind's sweep, next field.  Three kinds keep a loop of their own: the quadratic form adds each field's term into the plan's ONE array
// of doubles, in slot order (the order the fused kernel adds in), and sweeps that once; the joint histogram needs a pair at a
// time, a_p in nlr and b_p in nlr2 (two real work arrays, the least a pair can do with); the profiles take the same two arrays and
// sweep their rows along z (z is whole on every rank of a slab and of a pencil plan).
int mfft_plan_s::reduce_composed(const NlFields& u, int dealias, Op kind) {
  const bool pad = dealias == MFFT_DEALIAS_3_2;
  const int64_t nr = local_real_count(pad), nc = local_complex_alloc(), M = pad ? M2 : N2;
  if (nr <= 0 || !r2c) return set_error(MFFT_ERR_UNSUPPORTED, "real_%s needs a 3-D real-to-complex plan", nl_product(kind).name);
  MFFT_TRY(ensure(nlr, (size_t)nr * rs));
  const NlrCall& c = nlcall;
  auto back = [&](int f, Buf& to) { return exec(false, u.src(f, nc, es), to.p, dealias); };
  if (kind == Op::JointHistogram) {
    MFFT_TRY(ensure(nlr2, (size_t)nr * rs));
    int64_t* acc = static_cast<int64_t*>(nljacc.p);
    for (int p = 0; p < u.ncomp; ++p) {
      MFFT_TRY(back(p, nlr));
      MFFT_TRY(back(u.ncomp + p, nlr2));
      MFFT_TRY(stage("nl_joint", 2.0 * (double)nr * rs, [&] {
        return joint_sweep(nlr.p, nlr2.p, (size_t)nr, c.lo + 2 * p, c.inv + 2 * p, c.nba, c.nbb, acc + (size_t)p * joint_cells(c.nba, c.nbb));
      }));
    }
    return 0;
  }
  if (kind == Op::Profiles) {
    MFFT_TRY(ensure(nlr2, (size_t)nr * rs));
    double* acc = static_cast<double*>(nlpacc.p);
    for (int p = 0; p < u.ncomp; ++p) {
      MFFT_TRY(back(p, nlr));
      MFFT_TRY(back(u.ncomp + p, nlr2));
      MFFT_TRY(stage("nl_profiles", 2.0 * (double)nr * rs, [&] {
        return prof_sweep(nlr.p, nlr2.p, 1, nr / M, M, c.center + 2 * p, acc + (size_t)p * MFFT_PROFILE_STATS * (size_t)M);
      }));
    }
    return 0;
  }
  if (kind == Op::Quadratic) {
    MFFT_TRY(ensure(nlq, (size_t)nr * sizeof(double)));
    double* q = static_cast<double*>(nlq.p);
    bool first = true;
    for (int slot = 0; slot < 6; ++slot)
      for (int f = 0; f < u.nfields; ++f) {
        if (nls_slot(u, f) != slot) continue;
        MFFT_TRY(back(f, nlr));
        MFFT_TRY(stage("nl_quadratic_add", (double)nr * (rs + 16), [&] { return quad_accum(nlr.p, q, (size_t)nr, c.w[slot], first); }));
        first = false;
      }
    const double one[1] = {1.0};
    return stage("nl_quadratic", (double)nr * 8, [&] { return quad_sweep(q, true, 1, (size_t)nr, (size_t)nr, one, false); });
  }
  for (int f = 0; f < u.nfields; ++f) {
    const int slot = nls_slot(u, f);
    MFFT_TRY(back(f, nlr));
    if (kind == Op::Moments) {
      double* acc = static_cast<double*>(nlsacc.p);
      MFFT_TRY(stage("nl_moments", (double)nr * rs, [&] { return moments_sweep(nlr.p, 1, (size_t)nr, acc + NLS_SLOTS + slot, acc + slot * NLS_STATS); }));
    } else if (kind == Op::Histogram) {
      int64_t* acc = static_cast<int64_t*>(nlhacc.p);
      MFFT_TRY(stage("nl_histogram", (double)nr * rs, [&] {
        return hist_sweep(nlr.p, 1, (size_t)nr, c.lo + slot, c.inv + slot, c.nbins, acc + (size_t)slot * (c.nbins + 3));
      }));
    } else if (kind == Op::IncrementHistogram) {      // (z is whole on every rank, as for the increments below)
      int64_t* acc = static_cast<int64_t*>(nlkacc.p);
      MFFT_TRY(stage("nl_incr_hist", (double)nr * rs, [&] {
        return incr_hist_sweep(nlr.p, 1, nr / M, M, M, slot, acc + (size_t)slot * c.nsep * (c.nbins + 3));
      }));
    } else {      // Op::Increments: z is whole on every rank of a slab and of a pencil plan, so no halo is needed
      double* acc = static_cast<double*>(nliacc.p);
      MFFT_TRY(stage("nl_increments", (double)nr * rs, [&] { return incr_sweep(nlr.p, 1, nr / M, M, M, acc + slot * INCR_FIELD); }));
    }
  }
  return 0;
}

// [min, max, S1 .. S4] per field, S_p = sum (x - center)^p
int mfft_plan_s::real_moments(const NlFields& u, int dealias, const double* center, double* out, int64_t* count) {
  double c6[6] = {0, 0, 0, 0, 0, 0}, host[NLS_SLOTS];
  for (int f = 0; center && f < u.nfields; ++f) c6[nls_slot(u, f)] = center[f];
  MFFT_TRY(real_reduce(u, dealias, Op::Moments, count, [&] { return moments_begin(c6); }, [&] { return moments_end(host); }));
  for (int f = 0; f < u.nfields; ++f)
    for (int k = 0; k < NLS_STATS; ++k) out[f * NLS_STATS + k] = host[nls_slot(u, f) * NLS_STATS + k];
  return 0;
}

// per field nbins + 3 counts: below lo, the nbins equal bins of [lo, hi), at or above hi, not finite (nlz_reduce.h hist_slot).  Counts are
// integers: the same bits on every route that computes the same values.
int mfft_plan_s::real_histogram(const NlFields& u, int dealias, const double* lo, const double* hi, int nbins, int64_t* out, int64_t* count) {
  double l6[6] = {0, 0, 0, 0, 0, 0}, i6[6] = {1, 1, 1, 1, 1, 1};
  for (int f = 0; f < u.nfields; ++f) {
    const int slot = nls_slot(u, f);
    MFFT_TRY(hist_range(lo[f], hi[f], nbins, &i6[slot]));
    l6[slot] = lo[f];
  }
  const int nb3 = nbins + 3, nslots = 2 * ((u.nfields + 1) / 2);
  std::vector<int64_t> host((size_t)nslots * nb3);
  MFFT_TRY(real_reduce(u, dealias, Op::Histogram, count, [&] { return hist_begin(l6, i6, nbins); }, [&] { return hist_end(host.data(), nslots); }));
  for (int f = 0; f < u.nfields; ++f)
    memcpy(out + (size_t)f * nb3, host.data() + (size_t)nls_slot(u, f) * nb3, (size_t)nb3 * sizeof(int64_t));
  return 0;
}

// q(x) = sum_f w_f r_f(x)^2, r_f = ifftn(field f, dealias), by the one rule of include/mpifft4py_amd.h: [min, max, S1 .. S4] of q about
// `center` and, nbins > 0, its nbins + 3 counts over [lo, hi) (nlz_quad.h NlzQuad::body)
int mfft_plan_s::real_quadratic(const NlFields& u, int dealias, const double* weights, double center, double lo, double hi, int nbins, double* out6,
                                int64_t* counts, int64_t* count) {
  if (!std::isfinite(center)) return set_error(MFFT_ERR_INVALID, "the centre is not finite");
  double inv = 1.0;
  MFFT_TRY(quad_check(weights, u.nfields, lo, hi, nbins, &inv));
  auto begin = [&] {
    for (int i = 0; i < 6; ++i) nlcall.w[i] = 0.0;
    for (int f = 0; f < u.nfields; ++f) nlcall.w[nls_slot(u, f)] = weights[f];
    return quad_begin(center, lo, inv, nbins);
  };
  return real_reduce(u, dealias, Op::Quadratic, count, begin, [&] { return quad_end(out6, counts); });
}

// per field and separation the sums S2, S3, S4 of d = x(z + s) - x(z), rows periodic (nlz_incr.h NlzIncr::body)
int mfft_plan_s::real_increments(const NlFields& u, int dealias, const int64_t* seps, int nsep, double* out, int64_t* count) {
  const bool pad = dealias == MFFT_DEALIAS_3_2;
  const int64_t nr = local_real_count(pad), M = pad ? M2 : N2;
  if (nr <= 0 || !r2c || M < 2 || nr % M != 0) return set_error(MFFT_ERR_UNSUPPORTED, "real_increments needs a 3-D real-to-complex plan");
  MFFT_TRY(incr_check(seps, nsep, M));
  double host[INCR_SLOTS];
  MFFT_TRY(real_reduce(u, dealias, Op::Increments, count, [&] { return incr_begin(seps, nsep); }, [&] { return incr_end(host); }));
  for (int f = 0; f < u.nfields; ++f)
    for (int i = 0; i < nsep; ++i)
      for (int k = 0; k < 3; ++k) out[(f * nsep + i) * 3 + k] = host[(nls_slot(u, f) * MFFT_INCR_MAXSEP + i) * 3 + k];
  return 0;
}

// per field and separation the nbins + 3 counts of d = x(z + s) - x(z) over [lo, hi) of that field and separation, rows periodic
// (nlz_incr_hist.h NlzIncrHist::body)
int mfft_plan_s::real_increment_histogram(const NlFields& u, int dealias, const int64_t* seps, int nsep, const double* lo, const double* hi,
                                          int nbins, int64_t* out, int64_t* count) {
  const bool pad = dealias == MFFT_DEALIAS_3_2;
  const int64_t nr = local_real_count(pad), M = pad ? M2 : N2;
  if (nr <= 0 || !r2c || M < 2 || nr % M != 0) return set_error(MFFT_ERR_UNSUPPORTED, "real_increment_histogram needs a 3-D real-to-complex plan");
  MFFT_TRY(incr_check(seps, nsep, M));
  double l6[6][MFFT_INCR_MAXSEP] = {}, i6[6][MFFT_INCR_MAXSEP];
  for (int f = 0; f < 6; ++f)
    for (int i = 0; i < MFFT_INCR_MAXSEP; ++i) i6[f][i] = 1.0;
  if (nbins < 1 || nbins > MFFT_INCR_HIST_MAXBINS) return set_error(MFFT_ERR_INVALID, "nbins must be 1 .. %d, not %d", MFFT_INCR_HIST_MAXBINS, nbins);
  for (int f = 0; f < u.nfields; ++f)
    for (int i = 0; i < nsep; ++i) {
      const int slot = nls_slot(u, f);
      MFFT_TRY(incr_hist_range(lo[f * nsep + i], hi[f * nsep + i], nbins, &i6[slot][i]));
      l6[slot][i] = lo[f * nsep + i];
    }
  const size_t row = (size_t)nsep * (nbins + 3);
  const int nslots = 2 * ((u.nfields + 1) / 2);
  std::vector<int64_t> host((size_t)nslots * row);      // (out is written on success only)
  MFFT_TRY(real_reduce(u, dealias, Op::IncrementHistogram, count, [&] { return incr_hist_begin(seps, nsep, l6, i6, nbins); },
                       [&] { return incr_hist_end(host.data(), nslots); }));
  for (int f = 0; f < u.nfields; ++f) memcpy(out + (size_t)f * row, host.data() + (size_t)nls_slot(u, f) * row, row * sizeof(int64_t));
  return 0;
}

// per PAIR (x_a, x_b) = (ifftn(a_p), ifftn(b_p)) the (nba + 3)(nbb + 3) counts, cell = slot of x_a * (nbb + 3) + slot of x_b (nlz_joint.h
// joint_cell); the pairs lie in slot order already
int mfft_plan_s::real_joint_histogram(const NlFields& u, int dealias, const double* lo, const double* hi, int nba, int nbb, int64_t* out,
                                      int64_t* count) {
  double l6[6] = {0, 0, 0, 0, 0, 0}, i6[6] = {1, 1, 1, 1, 1, 1};
  for (int f = 0; f < u.nfields; ++f) {
    const int slot = nls_slot(u, f);
    MFFT_TRY(joint_range(lo[f], hi[f], slot % 2 ? nbb : nba, &i6[slot]));
    l6[slot] = lo[f];
  }
  return real_reduce(u, dealias, Op::JointHistogram, count, [&] { return joint_begin(l6, i6, nba, nbb); }, [&] { return joint_end(out, u.ncomp); });
}

// per PAIR (x, y) = (ifftn(a_p), ifftn(b_p)) and per z index m the sums over the plane of d_x, d_y, d_x^2, d_y^2, d_x d_y, d = value -
// centre (nlz_prof.h NlzProf::body, prof_add); the pairs lie in slot order already
int mfft_plan_s::real_profiles(const NlFields& u, int dealias, const double* center, double* out, int64_t* count) {
  const bool pad = dealias == MFFT_DEALIAS_3_2;
  const int64_t nr = local_real_count(pad), M = pad ? M2 : N2;
  if (nr <= 0 || !r2c || M < 2 || nr % M != 0) return set_error(MFFT_ERR_UNSUPPORTED, "real_profiles needs a 3-D real-to-complex plan");
  MFFT_TRY(prof_check(center, u.nfields));
  double c6[6] = {0, 0, 0, 0, 0, 0};
  for (int f = 0; center && f < u.nfields; ++f) c6[nls_slot(u, f)] = center[f];
  std::vector<double> host((size_t)u.ncomp * MFFT_PROFILE_STATS * (size_t)M);      // (out is written on success only)
  int64_t points = 0;
  MFFT_TRY(real_reduce(u, dealias, Op::Profiles, &points, [&] { return prof_begin(c6, u.ncomp, M); }, [&] { return prof_end(host.data(), u.ncomp, M); }));
  memcpy(out, host.data(), host.size() * sizeof(double));
  *count = points / M;                             // points per plane on this rank
  return 0;
}
