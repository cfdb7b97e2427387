// plan_dealias.hip -- dealiasing.  2/3-rule: the mask, its recognition as a band (pruned inverse passes) and its
// hand-down to the first inverse pass.  3/2-rule: the copy-based and the fused padded routes of slab and pencil.
#include "plan_impl.h"

using namespace mfft;

namespace {

// Is the byte mask of shape (n0, n1, n2) the product f0[i] & f1[j] & f2[k] of three 1-D 0/1 filters (it must BE the product:
// values other than 0 / 1 are weights, not a filter)?  0: no, 1: yes, 2: the mask is all zeros (and so are the three)
int separable(const uint8_t* m, int64_t n0, int64_t n1, int64_t n2, std::vector<uint8_t> f[3]) {
  f[0].assign(n0, 0); f[1].assign(n1, 0); f[2].assign(n2, 0);
  for (int64_t i = 0; i < n0; ++i)
    for (int64_t j = 0; j < n1; ++j) {
      const uint8_t* row = m + (i * n1 + j) * n2;
      uint8_t any = 0;
      for (int64_t k = 0; k < n2; ++k) { any |= row[k]; f[2][k] |= row[k]; }
      f[0][i] |= any; f[1][j] |= any;
    }
  bool any = false;
  for (int a = 0; a < 3; ++a) for (auto& x : f[a]) { x = x ? 1 : 0; any = any || x; }
  if (!any) return 2;
  for (int64_t i = 0; i < n0; ++i)
    for (int64_t j = 0; j < n1; ++j) {
      const uint8_t* row = m + (i * n1 + j) * n2;
      const uint8_t ij = f[0][i] & f[1][j];
      for (int64_t k = 0; k < n2; ++k) if (row[k] != (uint8_t)(ij & f[2][k])) return 0;
    }
  return 1;
}

// the zeros of v form one run [a, b) (none: a = b = first index after the ones)
bool zero_run(const std::vector<uint8_t>& v, int* a, int* b) {
  const int n = (int)v.size();
  int lo = 0;
  while (lo < n && v[lo]) ++lo;
  int hi = lo;
  while (hi < n && !v[hi]) ++hi;
  for (int i = hi; i < n; ++i) if (!v[i]) return false;
  *a = lo; *b = hi;
  return true;
}

}  // namespace

void mfft_plan_s::detect_band(const uint8_t* m) {
  band_ok = false;
  band_allzero = false;
  // every rank must take the same route (the pruned exchange has other counts): agree on the outcome below.
  // status: 0 = not a band mask (or no kernels), 1 = band mask, 2 = this rank's local mask is all zeros -- its ky range
  // lies wholly inside the removed band (1024^3 over 8 ranks: ky in [342, 683) covers ranks 3 and 4) -- which is
  // compatible with whatever band the others see: it adopts their (a0, b0, a2) and contributes zeros.
  int st = 0, a0 = 0, b0 = 0, a1 = 0, b1 = 0, a2 = 0;
  std::vector<int> list;
  if (d.decomp == MFFT_SLAB && r2c && N0 >= 2 && N1 >= 2 && N2 >= 4 && N2 % 2 == 0 && band_fusable(N0, prec) &&
      band_fusable(N1, prec) && c2r_limit_supported(N2, prec))
    st = analyse_band(m, &a0, &b0, &a1, &b1, &a2, &list);
  if (P > 1) {
    const double none = -1e18;                 // neutral element of the max-reduction
    double v[8] = {st == 0 ? 1.0 : 0.0, st == 1 ? 1.0 : 0.0, none, none, none, none, none, none};
    if (st == 1) { v[2] = a0; v[3] = -a0; v[4] = b0; v[5] = -b0; v[6] = a2; v[7] = -a2; }
    if (comm->allreduce_host(v, 8, 1) != 0) return;
    if (v[0] != 0.0 || v[1] != 1.0 || v[2] != -v[3] || v[4] != -v[5] || v[6] != -v[7]) return;   // somebody disagrees, has another mask, or nobody has a band
    if (st == 2) {                             // all my ky are removed: [g_lo, g_hi) = every local ky
      a0 = (int)v[2]; b0 = (int)v[4]; a2 = (int)v[6]; a1 = 0; b1 = (int)Np1;
      band_allzero = true;
    }
  } else if (st != 1) {
    return;
  }
  ba0 = a0; bb0 = b0; ba1 = a1; bb1 = b1; ba2 = a2;
  if (P == 1) {
    if (a1 < 1) return;                      // the y pass redirects removed rows to row 0, which must be a kept one
    if (band_tiles) (void)hipFree(band_tiles);
    band_tiles = nullptr;
    band_ntiles = (int)list.size();
    if (list.empty() || hipMalloc(reinterpret_cast<void**>(&band_tiles), list.size() * sizeof(int)) != hipSuccess ||
        hipMemcpy(band_tiles, list.data(), list.size() * sizeof(int), hipMemcpyHostToDevice) != hipSuccess) {
      (void)hipGetLastError();
      return;
    }
  }
  band_ok = true;
}
// local mask (N0, Np1, Nf) == m0[kx] & m1[ky] & m2[kz] with the zeros of m0 and m1 one run each and those of m2 a tail?
// 0: no, 1: yes, 2: the local mask is all zeros
int mfft_plan_s::analyse_band(const uint8_t* m, int* a0, int* b0, int* a1, int* b1, int* a2, std::vector<int>* list) const {
  std::vector<uint8_t> f[3];
  const int st = separable(m, N0, Np1, Nf, f);
  if (st != 1) return st;
  int z0 = 0, z1 = 0;
  if (!zero_run(f[0], a0, b0) || *a0 < 1 || !zero_run(f[1], a1, b1) || !zero_run(f[2], &z0, &z1) || z1 != (int)Nf || z0 < 1) return 0;
  *a2 = z0;
  if (P == 1) {      // x pass: tiles of the flattened (ky, kz) columns that hold a kept column, in memory order
    const int w = col_tile_width(N0, prec, true, Op::Band);
    if (w <= 0) return 0;
    const int64_t ncols = Np1 * Nf, ntile = (ncols + w - 1) / w;
    for (int64_t t = 0; t < ntile; ++t) {
      bool any = false;
      for (int64_t c = t * w; c < std::min(ncols, (t + 1) * w) && !any; ++c) any = f[1][c / Nf] && f[2][c % Nf];
      if (any) list->push_back((int)t);
    }
  }
  return 1;
}
void mfft_plan_s::detect_band_local(const uint8_t* m) {
  lband_ok = false;
  if (d.decomp == MFFT_SLAB || !r2c || d.drop_nyquist || d.line2d) return;
  const bool X = d.decomp == MFFT_PENCIL_X;
  const int64_t D0 = X ? N0 : N2_0, D1 = X ? N1_1 : N1, D2 = q;
  if (D0 < 1 || D1 < 1 || D2 < 1 || !band_fusable(X ? N0 : N1, prec) || (X ? N0 : N1) < 2) return;
  std::vector<uint8_t> f[3];
  if (separable(m, D0, D1, D2, f) == 0) return;      // not a product of 1-D filters
  int a0, b0, a1, b1, z0, z1;
  if (!zero_run(f[0], &a0, &b0) || !zero_run(f[1], &a1, &b1) || !zero_run(f[2], &z0, &z1) || z1 != (int)D2) return;   // kz: a kept prefix
  if (X) { lb_row_lo = a0; lb_row_hi = b0; lb_g_lo = a1; lb_g_hi = b1; }
  else   { lb_row_lo = a1; lb_row_hi = b1; lb_g_lo = a0; lb_g_hi = b0; }
  lb_c_lim = z0;
  lband_ok = prune_enabled();          // read when the mask is SET; fuse_mask reads it again at the call
}
// `fu * dealias` of the reference's ifftn (slab.py:237-245, pencil.py:455-462) without the masked copy: when the first
// inverse pass (length first_len, reading fu) has a masked-load kernel, remember fu and let col() hand the mask down.
// Returns false when the copy is needed after all (chirp-z lengths, unit axes, MFFT_NO_MASK_FUSION=1).
int mfft_plan_s::fuse_mask(const void* fu, int64_t first_len, bool* fused) {
  MFFT_TRY(require_mask());
  *fused = !env_on("MFFT_NO_MASK_FUSION") && first_len >= 2 && mask_fusable(first_len, prec);
  mask_src = *fused ? fu : nullptr;
  lband_use = *fused && lband_ok && d.decomp != MFFT_SLAB && prune_enabled();
  return 0;
}

int mfft_plan_s::apply_mask_copy(const void* fu, void** masked_out) {
  MFFT_TRY(require_mask());
  const size_t cna = (size_t)local_complex_alloc_native();      // pitched rows: the device mask has the same pitch
  MFFT_TRY(ensure(work[2], cna * es));
  MFFT_HIP(hipMemcpyAsync(work[2].p, fu, cna * es, hipMemcpyDeviceToDevice, stream));
  MFFT_TRY(launch_mask(work[2].p, mask, cna, prec, stream));
  *masked_out = work[2].p;
  return 0;
}

extern "C" {

int mfft_plan_set_dealias_mask(mfft_plan_t p, const uint8_t* mask_host, size_t count) {
  if (!p || !mask_host) return set_error(MFFT_ERR_INVALID, "null argument");
  if ((int64_t)count != p->local_complex_count()) return set_error(MFFT_ERR_INVALID, "mask has %zu entries, local spectrum has %lld", count, (long long)p->local_complex_count());
  p->drop_graphs();              // captured sequences hold the old mask pointer
  if (p->mask) MFFT_HIP(hipFree(p->mask));
  p->mask = nullptr;
  if (p->nat_pitch()) {          // the masked-load kernels index the mask like the spectrum: same row pitch, zeros between
    const size_t rows = (size_t)(p->N0 * p->Np1);
    MFFT_HIP(hipMalloc(reinterpret_cast<void**>(&p->mask), rows * (size_t)p->Zp));
    MFFT_HIP(hipMemset(p->mask, 0, rows * (size_t)p->Zp));
    MFFT_HIP(hipMemcpy2D(p->mask, (size_t)p->Zp, mask_host, (size_t)p->Nf, (size_t)p->Nf, rows, hipMemcpyHostToDevice));
  } else {
    MFFT_HIP(hipMalloc(reinterpret_cast<void**>(&p->mask), count));
    MFFT_HIP(hipMemcpy(p->mask, mask_host, count, hipMemcpyHostToDevice));
  }
  p->mask_count = count;
  p->detect_band(mask_host);
  p->detect_band_local(mask_host);
  return 0;
}

}  // extern "C"

// copy src (n along `axis`) into the zero-initialised padded dst (npad along
// axis): low half to the front, high half to the back (slab.py:518-523).
// shapes: src (a0, n, a2) -> dst (a0, npad, a2) viewed with the axis in the middle.
int mfft_plan_s::pad_axis(const void* src, void* dst, int64_t a0, int64_t n, int64_t npad, int64_t a2, double scale) {
  const char* s = static_cast<const char*>(src);
  char* dd = static_cast<char*>(dst);
  MFFT_TRY(zero(dst, (size_t)(a0 * npad * a2) * es));
  const int64_t h = n / 2;
  MFFT_TRY(box(s, dd, a0, 1, h * a2, n * a2, 0, npad * a2, 0, 0, scale));
  MFFT_TRY(box(s + (size_t)(h * a2) * es, dd + (size_t)((npad - (n - h)) * a2) * es, a0, 1, (n - h) * a2, n * a2, 0,
               npad * a2, 0, 0, scale));
  return 0;
}
// truncation with Nyquist fold (slab.py:529-533): dst[:n/2+1] = src[:n/2+1]; dst[n/2:] += src[-n/2:]
// src may have a longer contiguous run (a2s >= a2): only the first a2 are taken.
int mfft_plan_s::trunc_axis(const void* src, void* dst, int64_t a0, int64_t n, int64_t npad, int64_t a2, int64_t a2s, double scale,
               bool fold) {
  const char* s = static_cast<const char*>(src);
  char* dd = static_cast<char*>(dst);
  const int64_t h = n / 2;
  if (!fold) {   // plain corner copies: dst[:n/2] = src[:n/2]; dst[n/2:] = src[-n/2:]   (slab.py:736-739, 796-797)
    MFFT_TRY(box(s, dd, a0, h, a2, npad * a2s, a2s, n * a2, a2, 0, scale));
    MFFT_TRY(box(s + (size_t)((npad - (n - h)) * a2s) * es, dd + (size_t)(h * a2) * es, a0, n - h, a2, npad * a2s, a2s,
                 n * a2, a2, 0, scale));
    return 0;
  }
  MFFT_TRY(zero(dst, (size_t)(a0 * n * a2) * es));
  MFFT_TRY(box(s, dd, a0, h + 1, a2, npad * a2s, a2s, n * a2, a2, 0, scale));
  MFFT_TRY(box(s + (size_t)((npad - h) * a2s) * es, dd + (size_t)(h * a2) * es, a0, h, a2, npad * a2s, a2s, n * a2, a2, 1, scale));
  return 0;
}

// One-rank fused 3/2-rule transforms (round 5): the two intermediates belong to the plan, so their z rows get a pitch of
// whole cache lines (513 bins -> 520 in double precision: rows of 8208 bytes never start on a line, and a 128-byte tile
// row then costs two lines on either side of the y pass).  The plain transform measured the same idea in round 4
// (profiles/r04_ypass_pitch.txt: y pass 3.46 -> 2.96 ms with rows of 520 on both sides) and could not use it -- it has
// one work buffer less and its x passes touch the caller's compact array on the wrong side; here the inverse x pass
// stores whole lines per y row (its loads straddle), the y pass and the real transform see aligned rows, and the
// forward x pass tiles the compact OUTPUT and wraps its input columns (ColParams::in_wrap).  MFFT_PAD_ALIGN=0: compact.
// Measured (profiles/r05_pad_align_ab.txt, 3/2-rule pair): 1024^3 fp64 45.3 -> 43.9 ms (y passes 8.7 / 7.8 -> 6.9 / 7.0 ms, the x
// passes give part of it back: their misaligned side costs 0.3 - 1.1 ms); 768^3 fp64 even; 512^3 fp64 and 1024^3 fp32 LOSE
// 2 - 3 % (rows of 4 KiB: the y pass gains less than the x pass pays).  Default: double precision, rows of 8 KiB and more.
int64_t mfft_plan_s::pad_pitch() const {
  if (pad_align == 0 || P != 1) return Nf;
  if (pad_align < 0 && !(prec == MFFT_DOUBLE && Nf * (int64_t)es >= 8192)) return Nf;
  const int64_t line = 128 / (int64_t)es;
  return (Nf + line - 1) / line * line;
}

// ---- 3/2-rule, slab (R2C: slab.py:310-344, 445-483; P == 1: 250-268, 372-386) ----
// fused 3/2-rule (R2C, padsize 1.5): the zero band is never materialised -- the x and y
// inverse transforms read the un-padded rows and skip the band (ColFft PAD = 1), c2r reads the
// missing kz columns as zeros; forward: r2c stores only the kept columns, the y and x transforms
// store only the kept rows and fold the Nyquist row in registers (PAD = 2).  Six kernels per
// pair, like the un-padded path; pack / unpack ride on the two-level row maps.
bool mfft_plan_s::can_fuse_pad() const {
  if (!r2c || d.padsize != 1.5 || d.drop_nyquist || d.line2d) return false;
  if (N0 % 2 || N1 % 2 || 2 * M0 != 3 * N0 || 2 * M1 != 3 * N1 || 2 * M2 != 3 * N2) return false;
  return find_kernel(FAM_COL, (int)M0, prec, 1, Op::PadLoad) && find_kernel(FAM_COL, (int)M0, prec, 0, Op::TruncStore) &&
         find_kernel(FAM_COL, (int)M1, prec, 1, Op::PadLoad) && find_kernel(FAM_COL, (int)M1, prec, 0, Op::TruncStore) &&
         find_kernel(FAM_R2C, (int)M2, prec, 0, Op::Limited) && find_kernel(FAM_C2R, (int)M2, prec, 1, Op::Limited) &&
         getenv("MFFT_NO_PAD_FUSION") == nullptr;
}

int mfft_plan_s::slab_backward_padded_fused(const void* fu, void* u) {
  const double sc3 = padscale();
  const int64_t Mp0 = M0 / P;
  if (const int64_t Za = nat_pitch() ? Zp : pad_pitch(); Za != Nf) {          // one rank, line-aligned z rows in both intermediates
    MFFT_TRY(ensure(work[0], (size_t)(M0 * N1 * Za) * es));
    MFFT_TRY(ensure(work[2], (size_t)(M0 * M1 * Za) * es));
    void *W0 = work[0].p, *W2 = work[2].p;
    // Who absorbs the misaligned side.  The caller's rows have the pitch already (nat_pitch), or the y pass converts
    // (pad_align_inv == 3: x compact -> compact, y compact -> pitched): the x pass takes whole planes of N1 * Zx columns.
    // Otherwise the x pass converts, one outer batch per y row: compact rows in, pitched rows out.
    const bool xconv = !nat_pitch() && pad_align_inv != 3;
    const int64_t Zx = (nat_pitch() || xconv) ? Za : Nf;       // row pitch of the x pass's output
    MFFT_TRY(stage("bwd_x", 0, [&] {
      if (xconv)
        return col_pad(fu, W0, M0, true, Op::PadLoad, false, N1, Nf, Nf, plain(N1 * Nf), Za, plain(N1 * Za), sc3 / (double)M0, 0, 0,
                       pad_align_inv == 2 ? -1 : 1);
      return col_pad(fu, W0, M0, true, Op::PadLoad, false, 1, N1 * Zx, 0, plain(N1 * Zx), 0, plain(N1 * Zx), sc3 / (double)M0);
    }));
    MFFT_TRY(stage("bwd_y", 0, [&] {
      return col_pad(W0, W2, M1, true, Op::PadLoad, false, M0, Nf, N1 * Zx, plain(Zx), M1 * Za, plain(Za), 1.0 / (double)M1);
    }));
    MFFT_TRY(stage("bwd_z", 0, [&] { return c2r_rows(W2, u, M0 * M1, M2, Za, M2, 1.0 / (double)M2, (int)Nf); }));
    return 0;
  }
  MFFT_TRY(ensure(work[0], (size_t)(M0 * Np1 * Nf) * es));
  MFFT_TRY(ensure(work[1], (size_t)(M0 * Np1 * Nf) * es));
  MFFT_TRY(ensure(work[2], (size_t)(Mp0 * M1 * Nf) * es));
  void *W0 = work[0].p, *W1 = work[1].p, *W2 = work[2].p;
  MFFT_TRY(stage("bwd_x", 0, [&] {
    return col_pad(fu, W0, M0, true, Op::PadLoad, false, 1, Np1 * Nf, 0, plain(Np1 * Nf), 0, plain(Np1 * Nf), sc3 / (double)M0);
  }));
  const void* yin = W0;
  RowSpec yrows = plain(Nf);
  if (P > 1) {                  // the y pass reads the (P, Mp0, Np1, Nf) receive layout through its row map
    MFFT_TRY(stage("bwd_a2a", 0, [&] { return xchg(0, false, true, W0, W1); }));
    yin = W1;
    yrows = two_level(Np1, Mp0 * Np1 * Nf, Nf);
  }
  MFFT_TRY(stage("bwd_y", 0, [&] {
    return col_pad(yin, W2, M1, true, Op::PadLoad, false, Mp0, Nf, Np1 * Nf, yrows, M1 * Nf, plain(Nf), 1.0 / (double)M1);
  }));
  MFFT_TRY(stage("bwd_z", 0, [&] { return c2r_rows(W2, u, Mp0 * M1, M2, Nf, M2, 1.0 / (double)M2, (int)Nf); }));
  return 0;
}

int mfft_plan_s::slab_forward_padded_fused(const void* u, void* fu) {
  const double isc3 = 1.0 / padscale();
  const int64_t Mp0 = M0 / P;
  if (const int64_t Za = nat_pitch() ? Zp : pad_pitch(); Za != Nf) {          // one rank, line-aligned z rows in both intermediates
    MFFT_TRY(ensure(work[0], (size_t)(M0 * N1 * Za) * es));
    MFFT_TRY(ensure(work[2], (size_t)(M0 * M1 * Za) * es));
    void *W0 = work[0].p, *W2 = work[2].p;
    MFFT_TRY(stage("fwd_z", 0, [&] { return r2c_rows(u, W2, M0 * M1, M2, M2, Za, 1.0, (int)Nf); }));
    MFFT_TRY(stage("fwd_y", 0, [&] {
      return col_pad(W2, W0, M1, false, Op::TruncStore, true, M0, Nf, M1 * Za, plain(Za), N1 * Za, plain(Za), 1.0);
    }));
    // pitched result (nat_pitch): whole planes of N1 * Za columns, no conversion.  Compact result: its tiles, the input
    // column c = (y, z) sits at y * Za + z (ColParams::in_wrap)
    const int64_t Zo = nat_pitch() ? Za : Nf;
    MFFT_TRY(stage("fwd_x", 0, [&] {
      return col_pad(W0, fu, M0, false, Op::TruncStore, true, 1, N1 * Zo, 0, plain(N1 * Za), 0, plain(N1 * Zo), isc3, Zo == Za ? 0 : Nf, Za - Zo);
    }));
    return 0;
  }
  MFFT_TRY(ensure(work[0], (size_t)(M0 * Np1 * Nf) * es));
  MFFT_TRY(ensure(work[1], (size_t)(M0 * Np1 * Nf) * es));
  MFFT_TRY(ensure(work[2], (size_t)(Mp0 * M1 * Nf) * es));
  void *W0 = work[0].p, *W1 = work[1].p, *W2 = work[2].p;
  MFFT_TRY(stage("fwd_z", 0, [&] { return r2c_rows(u, W2, Mp0 * M1, M2, M2, Nf, 1.0, (int)Nf); }));
  // truncate + fold in y; P > 1: written straight into the packed (P, Mp0, Np1, Nf) send layout
  MFFT_TRY(stage("fwd_y", 0, [&] {
    return col_pad(W2, W0, M1, false, Op::TruncStore, true, Mp0, Nf, M1 * Nf, plain(Nf), Np1 * Nf,
                   P > 1 ? two_level(Np1, Mp0 * Np1 * Nf, Nf) : plain(Nf), 1.0);
  }));
  void* xin = W0;
  if (P > 1) {
    MFFT_TRY(stage("fwd_a2a", 0, [&] { return xchg(0, true, true, W0, W1); }));
    xin = W1;
  }
  MFFT_TRY(stage("fwd_x", 0, [&] {
    return col_pad(xin, fu, M0, false, Op::TruncStore, true, 1, Np1 * Nf, 0, plain(Np1 * Nf), 0, plain(Np1 * Nf), isc3);
  }));
  return 0;
}

int mfft_plan_s::slab_backward_padded(const void* fu, void* u) {
  if (P > 1 && P > N0 / 2) return set_error(MFFT_ERR_INVALID, "number of ranks cannot exceed N[0]/2 for the 3/2-rule");
  if (can_fuse_pad()) return slab_backward_padded_fused(fu, u);
  const double sc3 = padscale();
  const int64_t Mp0 = M0 / P;
  // W0: (M0, Np1, Nf) padded in x; W1: (Mp0, N1, Nf) after the exchange; then (Mp0, M1, Nf), (Mp0, M1, Mf)
  MFFT_TRY(ensure(work[0], (size_t)std::max(M0 * Np1 * Nf, Mp0 * M1 * Mf) * es));
  MFFT_TRY(ensure(work[1], (size_t)std::max(Mp0 * N1 * Nf, Mp0 * M1 * Nf) * es));
  MFFT_TRY(ensure(work[2], (size_t)(Mp0 * M1 * Nf) * es));
  void *W0 = work[0].p, *W1 = work[1].p, *W2 = work[2].p;
  MFFT_TRY(stage("pad_x", 0, [&] { return pad_axis(fu, W0, 1, N0, M0, Np1 * Nf, sc3); }));
  MFFT_TRY(stage("bwd_x", 0, [&] { return col(W0, W0, M0, true, 1, Np1 * Nf, 0, plain(Np1 * Nf), 0, plain(Np1 * Nf)); }));
  const void* yin = W0;
  if (P > 1) {
    MFFT_TRY(stage("bwd_a2a", 0, [&] { return xchg(0, false, true, W0, W1); }));
    // unpack (P, Mp0, Np1, Nf) -> (Mp0, N1, Nf)
    MFFT_TRY(stage("unpack", 0, [&] {
      for (int p = 0; p < P; ++p)
        MFFT_TRY(box(static_cast<char*>(W1) + (size_t)p * (Mp0 * Np1 * Nf) * es,
                     static_cast<char*>(W2) + (size_t)(p * Np1 * Nf) * es, Mp0, 1, Np1 * Nf, Np1 * Nf, 0, N1 * Nf, 0));
      return 0;
    }));
    yin = W2;
  }
  // pad y: (Mp0, N1, Nf) -> (Mp0, M1, Nf)
  void* ypad = (yin == W2) ? W1 : W2;
  MFFT_TRY(stage("pad_y", 0, [&] { return pad_axis(yin, ypad, Mp0, N1, M1, Nf, 1.0); }));
  MFFT_TRY(stage("bwd_y", 0, [&] { return col(ypad, ypad, M1, true, Mp0, Nf, M1 * Nf, plain(Nf), M1 * Nf, plain(Nf)); }));
  // pad z: (Mp0*M1, Nf) -> (Mp0*M1, Mf); one-sided for the half spectrum, two-sided for C2C (slab.py:815-817)
  MFFT_TRY(stage("pad_z", 0, [&] {
    if (!r2c) return pad_axis(ypad, W0, Mp0 * M1, N2, M2, 1, 1.0);
    MFFT_TRY(zero(W0, (size_t)(Mp0 * M1 * Mf) * es));
    return box(ypad, W0, 1, Mp0 * M1, Nf, 0, Nf, 0, Mf);
  }));
  MFFT_TRY(stage("bwd_z", 0, [&] {
    if (!r2c) return c2c_rows(W0, u, Mp0 * M1, M2, M2, M2, true, 1.0 / (double)M2);
    return c2r_rows(W0, u, Mp0 * M1, M2, Mf, M2, 1.0 / (double)M2);
  }));
  return 0;
}

int mfft_plan_s::slab_forward_padded(const void* u, void* fu) {
  if (P > 1 && P > N0 / 2) return set_error(MFFT_ERR_INVALID, "number of ranks cannot exceed N[0]/2 for the 3/2-rule");
  if (can_fuse_pad()) return slab_forward_padded_fused(u, fu);
  const double isc3 = 1.0 / padscale();
  const int64_t Mp0 = M0 / P;
  MFFT_TRY(ensure(work[0], (size_t)std::max(Mp0 * M1 * Mf, M0 * Np1 * Nf) * es));
  MFFT_TRY(ensure(work[1], (size_t)std::max(Mp0 * N1 * Nf, M0 * Np1 * Nf) * es));
  MFFT_TRY(ensure(work[2], (size_t)std::max(M0 * Np1 * Nf, r2c ? (int64_t)0 : Mp0 * M1 * Nf) * es));
  void *W0 = work[0].p, *W1 = work[1].p, *W2 = work[2].p;
  MFFT_TRY(stage("fwd_z", 0, [&] {
    if (!r2c) return c2c_rows(u, W0, Mp0 * M1, M2, M2, M2, false, 1.0);
    return r2c_rows(u, W0, Mp0 * M1, M2, M2, Mf);
  }));
  MFFT_TRY(stage("fwd_y", 0, [&] { return col(W0, W0, M1, false, Mp0, Mf, M1 * Mf, plain(Mf), M1 * Mf, plain(Mf)); }));
  // truncate y and z: (Mp0, M1, Mf) -> (Mp0, N1, Nf)   (slab.py:459 / C2C: 782 copy_from_padded axis 1).
  // The reference's C2C folds the Nyquist modes of y and z for P > 1 and does plain corner
  // copies (no fold) on one rank (slab.py:736-739); both are reproduced.
  const bool c2c_fold = P > 1;
  MFFT_TRY(stage("trunc_y", 0, [&] {
    if (r2c) return trunc_axis(W0, W1, Mp0, N1, M1, Nf, Mf, 1.0);
    MFFT_TRY(trunc_axis(W0, W2, Mp0 * M1, N2, M2, 1, 1, 1.0, c2c_fold));
    return trunc_axis(W2, W1, Mp0, N1, M1, N2, N2, 1.0, c2c_fold);
  }));
  void* xin = W1;
  if (P > 1) {
    // pack (Mp0, P, Np1, Nf) -> (P, Mp0, Np1, Nf) and exchange
    MFFT_TRY(stage("pack", 0, [&] {
      for (int p = 0; p < P; ++p)
        MFFT_TRY(box(static_cast<char*>(W1) + (size_t)(p * Np1 * Nf) * es,
                     static_cast<char*>(W0) + (size_t)p * (Mp0 * Np1 * Nf) * es, Mp0, 1, Np1 * Nf, N1 * Nf, 0, Np1 * Nf, 0));
      return 0;
    }));
    MFFT_TRY(stage("fwd_a2a", 0, [&] { return xchg(0, true, true, W0, W2); }));
    xin = W2;
  }
  MFFT_TRY(stage("fwd_x", 0, [&] { return col(xin, xin, M0, false, 1, Np1 * Nf, 0, plain(Np1 * Nf), 0, plain(Np1 * Nf)); }));
  // R2C folds the x Nyquist plane (slab.py:480-482); C2C copies the two halves (slab.py:796-797)
  MFFT_TRY(stage("trunc_x", 0, [&] { return trunc_axis(xin, fu, 1, N0, M0, Np1 * Nf, Np1 * Nf, isc3, r2c); }));
  return 0;
}

// the same for the fused 3/2-rule pencil transforms: real length M2, the Nf kept columns split into the z chunks
bool mfft_plan_s::zfuse_pad() const {
  return getenv("MFFT_NO_ZFUSE") == nullptr && !d.line2d && !d.drop_nyquist && !zc.empty() && zc[0].len < 65536 &&
         M2 % 2 == 0 && zsplit_limit_supported(M2, prec);
}

// ---- fused 3/2-rule, pencil: same idea as the slab (see can_fuse_pad): pad-on-load / truncate-on-store
// column kernels whose two-level row maps also do the y-chunk pack / unpack, column-limited real kernels.
// Only the z-chunk pack / unpack around the z-splitting exchange remain as copies.
int mfft_plan_s::pencil_backward_padded_fused(const void* fu, void* u) {
  const double sc3 = padscale();
  const bool X = d.decomp == MFFT_PENCIL_X;
  const int64_t mp = M0 / P1, np = M1 / P2;          // padded local real rows in x, y
  const size_t wb = (size_t)std::max(std::max(M0 * N1_1 * q, mp * M1 * q), std::max(std::max(N2_0 * M1 * q, M0 * np * q), mp * np * Nf)) * es;
  for (int i = 0; i < 3; ++i) MFFT_TRY(ensure(work[i], wb));
  void *W0 = work[0].p, *W1 = work[1].p, *W2 = work[2].p;
  // a group of one rank exchanges nothing: with the fused z kernels its exchange is skipped altogether (the transform
  // on the far side reads the buffer the near side wrote)
  const bool fz = zfuse_pad();
  const bool zsolo = fz && (X ? P2 : P1) == 1, g2solo = fz && (X ? P1 : P2) == 1;
  void* cur = W0;                                    // what the next stage reads
  auto other = [&](void* b) { return b == W0 ? W1 : W0; };
  if (X) {
    // fu (N0, N1_1, q) -> ifft x over M0 rows, the zero band never read
    MFFT_TRY(stage("bwd_x", 0, [&] {
      return col_pad(fu, W0, M0, true, Op::PadLoad, false, 1, N1_1 * q, 0, plain(N1_1 * q), 0, plain(N1_1 * q), sc3 / (double)M0);
    }));
    if (!g2solo) {
      MFFT_TRY(stage("bwd_a2a_2", 0, [&] { return xchg(1, false, true, W0, W1); }));
      cur = W1;
    }
    // cur = P1 blocks (mp, N1_1, q): gather y through the input row map, pad on load, write P2 blocks (mp, np, q)
    void* dst = other(cur);
    MFFT_TRY(stage("bwd_y", 0, [&] {
      return col_pad(cur, dst, M1, true, Op::PadLoad, false, mp, q, N1_1 * q, two_level(N1_1, mp * N1_1 * q, q), np * q,
                     two_level(np, mp * np * q, q), 1.0 / (double)M1);
    }));
    cur = dst;
  } else {
    // fu (N2_0, N1, q) -> ifft y over M1 rows, written as P2 blocks (N2_0, np, q)
    MFFT_TRY(stage("bwd_y", 0, [&] {
      return col_pad(fu, W0, M1, true, Op::PadLoad, false, N2_0, q, N1 * q, plain(q), np * q, two_level(np, N2_0 * np * q, q),
                     sc3 / (double)M1);
    }));
    if (!g2solo) {
      MFFT_TRY(stage("bwd_a2a_2", 0, [&] { return xchg(1, false, true, W0, W1); }));
      cur = W1;
    }
    // cur = (N0, np, q) -> ifft x over M0 rows; its x chunks (mp rows) are the blocks of the next exchange
    void* dst = other(cur);
    MFFT_TRY(stage("bwd_x", 0, [&] {
      return col_pad(cur, dst, M0, true, Op::PadLoad, false, 1, np * q, 0, plain(np * q), 0, plain(np * q), 1.0 / (double)M0);
    }));
    cur = dst;
  }
  if (!zsolo) {
    void* dst = other(cur);
    MFFT_TRY(stage("bwd_a2a_1", 0, [&] { return xchg(0, false, true, cur, dst); }));
    cur = dst;
  }
  // only the Nf kept columns exist: c2r reads the others as zeros
  if (fz) {                     // ... and reads the kept ones out of the received z-chunk blocks itself
    MFFT_TRY(stage("bwd_z", 0, [&] {
      RealArgs a = real_args(cur, u, mp * np, M2, Nf, M2, 1.0 / (double)M2, (int)Nf);
      a.zs = zsplit(mp * np, 0);
      return launch_c2r(a, stream);
    }));
    return 0;
  }
  MFFT_TRY(stage("bwd_unpackz", 0, [&] { return pack_z(W2, cur, mp * np, Nf, true); }));
  MFFT_TRY(stage("bwd_z", 0, [&] { return c2r_rows(W2, u, mp * np, M2, Nf, M2, 1.0 / (double)M2, (int)Nf); }));
  return 0;
}

int mfft_plan_s::pencil_forward_padded_fused(const void* u, void* fu) {
  const double isc3 = 1.0 / padscale();
  const bool X = d.decomp == MFFT_PENCIL_X;
  const int64_t mp = M0 / P1, np = M1 / P2;
  const size_t wb = (size_t)std::max(std::max(M0 * N1_1 * q, mp * M1 * q), std::max(std::max(N2_0 * M1 * q, M0 * np * q), mp * np * Nf)) * es;
  for (int i = 0; i < 3; ++i) MFFT_TRY(ensure(work[i], wb));
  void *W0 = work[0].p, *W1 = work[1].p;
  const bool fz = zfuse_pad();
  const bool zsolo = fz && (X ? P2 : P1) == 1, g2solo = fz && (X ? P1 : P2) == 1;
  auto other = [&](void* b) { return b == W0 ? W1 : W0; };
  if (fz) {                     // r2c stores the kept columns straight into the z-chunk send blocks
    MFFT_TRY(stage("fwd_z", 0, [&] {
      RealArgs a = real_args(u, W1, mp * np, M2, M2, Nf, 1.0, (int)Nf);
      a.zs = zsplit(mp * np, 0);
      return launch_r2c(a, stream);
    }));
  } else {
    MFFT_TRY(stage("fwd_z", 0, [&] { return r2c_rows(u, W0, mp * np, M2, M2, Nf, 1.0, (int)Nf); }));
    MFFT_TRY(stage("fwd_packz", 0, [&] { return pack_z(W0, W1, mp * np, Nf, false); }));
  }
  void* cur = W1;
  if (!zsolo) {
    MFFT_TRY(stage("fwd_a2a_1", 0, [&] { return xchg(0, true, true, W1, W0); }));
    cur = W0;
  }
  if (X) {
    // cur = P2 blocks (mp, np, q): fft y gathering over M1 rows, truncate + fold on store, straight into
    // the P1 blocks (mp, N1_1, q) of the next exchange
    void* dst = other(cur);
    MFFT_TRY(stage("fwd_y", 0, [&] {
      return col_pad(cur, dst, M1, false, Op::TruncStore, true, mp, q, np * q, two_level(np, mp * np * q, q), N1_1 * q,
                     two_level(N1_1, mp * N1_1 * q, q), 1.0);
    }));
    cur = dst;
    if (!g2solo) {
      dst = other(cur);
      MFFT_TRY(stage("fwd_a2a_2", 0, [&] { return xchg(1, true, true, cur, dst); }));
      cur = dst;
    }
    MFFT_TRY(stage("fwd_x", 0, [&] {
      return col_pad(cur, fu, M0, false, Op::TruncStore, true, 1, N1_1 * q, 0, plain(N1_1 * q), 0, plain(N1_1 * q), isc3);
    }));
  } else {
    // cur = (M0, np, q): fft x, truncate + fold to (N0, np, q)
    void* dst = other(cur);
    MFFT_TRY(stage("fwd_x", 0, [&] {
      return col_pad(cur, dst, M0, false, Op::TruncStore, true, 1, np * q, 0, plain(np * q), 0, plain(np * q), 1.0);
    }));
    cur = dst;
    if (!g2solo) {
      dst = other(cur);
      MFFT_TRY(stage("fwd_a2a_2", 0, [&] { return xchg(1, true, true, cur, dst); }));
      cur = dst;
    }
    // cur = P2 blocks (N2_0, np, q): fft y gathering over M1 rows, truncate + fold into fu (N2_0, N1, q)
    MFFT_TRY(stage("fwd_y", 0, [&] {
      return col_pad(cur, fu, M1, false, Op::TruncStore, true, N2_0, q, np * q, two_level(np, N2_0 * np * q, q), N1 * q, plain(q), isc3);
    }));
  }
  return 0;
}

// ---- 3/2-rule, pencil (Alltoallw branches; padding of an axis happens right
// before the transform along it, when the axis is locally complete) -------------
int mfft_plan_s::pencil_backward_padded(const void* fu, void* u) {
  if (!r2c) return set_error(MFFT_ERR_UNSUPPORTED, "3/2-rule is implemented for R2C plans");
  if (d.drop_nyquist) return set_error(MFFT_ERR_UNSUPPORTED, "3/2-rule with communication='AlltoallN' is not implemented");
  if (can_fuse_pad()) return pencil_backward_padded_fused(fu, u);
  const double sc3 = padscale();
  const bool X = d.decomp == MFFT_PENCIL_X;
  const int64_t mp = M0 / P1, np = M1 / P2;          // padded local real rows in x, y
  const size_t wb = (size_t)std::max(std::max(M0 * N1_1 * q, mp * M1 * q), std::max(std::max(N2_0 * M1 * q, M0 * np * q), mp * np * Mf)) * es;
  for (int i = 0; i < 3; ++i) MFFT_TRY(ensure(work[i], wb));
  void *W0 = work[0].p, *W1 = work[1].p, *W2 = work[2].p;
  if (X) {
    // fu (N0, N1_1, q): pad x -> (M0, N1_1, q), ifft x
    MFFT_TRY(stage("pad_x", 0, [&] { return pad_axis(fu, W0, 1, N0, M0, N1_1 * q, sc3); }));
    MFFT_TRY(stage("bwd_x", 0, [&] { return col(W0, W0, M0, true, 1, N1_1 * q, 0, plain(N1_1 * q), 0, plain(N1_1 * q)); }));
    MFFT_TRY(stage("bwd_a2a_2", 0, [&] { return xchg(1, false, true, W0, W1); }));
    // W1 = P1 blocks (mp, N1_1, q) -> gather to (mp, N1, q)
    MFFT_TRY(stage("unpack", 0, [&] {
      for (int g = 0; g < P1; ++g)
        MFFT_TRY(box(static_cast<char*>(W1) + (size_t)g * (mp * N1_1 * q) * es, static_cast<char*>(W2) + (size_t)(g * N1_1 * q) * es,
                     mp, 1, N1_1 * q, N1_1 * q, 0, N1 * q, 0));
      return 0;
    }));
    MFFT_TRY(stage("pad_y", 0, [&] { return pad_axis(W2, W0, mp, N1, M1, q, 1.0); }));
    // ifft y on (mp, M1, q), writing P2 blocks (mp, np, q)
    MFFT_TRY(stage("bwd_y", 0, [&] {
      return col(W0, W1, M1, true, mp, q, M1 * q, plain(q), np * q, two_level(np, mp * np * q, q));
    }));
  } else {
    // fu (N2_0, N1, q): pad y -> (N2_0, M1, q), ifft y writing P2 blocks (N2_0, np, q)
    MFFT_TRY(stage("pad_y", 0, [&] { return pad_axis(fu, W0, N2_0, N1, M1, q, sc3); }));
    MFFT_TRY(stage("bwd_y", 0, [&] {
      return col(W0, W1, M1, true, N2_0, q, M1 * q, plain(q), np * q, two_level(np, N2_0 * np * q, q));
    }));
    MFFT_TRY(stage("bwd_a2a_2", 0, [&] { return xchg(1, false, true, W1, W0); }));
    // W0 = (N0, np, q): pad x -> (M0, np, q), ifft x
    MFFT_TRY(stage("pad_x", 0, [&] { return pad_axis(W0, W1, 1, N0, M0, np * q, 1.0); }));
    MFFT_TRY(stage("bwd_x", 0, [&] { return col(W1, W1, M0, true, 1, np * q, 0, plain(np * q), 0, plain(np * q)); }));
  }
  // W1 holds Pz blocks (mp, np, q) (X: y chunks; Y: contiguous x chunks)
  MFFT_TRY(stage("bwd_a2a_1", 0, [&] { return xchg(0, false, true, W1, W0); }));
  // unpack z into the zero-padded (mp*np, Mf) rows
  MFFT_TRY(stage("bwd_unpackz", 0, [&] {
    MFFT_TRY(zero(W2, (size_t)(mp * np * Mf) * es));
    return pack_z(W2, W0, mp * np, Mf, true);
  }));
  MFFT_TRY(stage("bwd_z", 0, [&] { return c2r_rows(W2, u, mp * np, M2, Mf, M2, 1.0 / (double)M2); }));
  return 0;
}

int mfft_plan_s::pencil_forward_padded(const void* u, void* fu) {
  if (!r2c) return set_error(MFFT_ERR_UNSUPPORTED, "3/2-rule is implemented for R2C plans");
  if (d.drop_nyquist) return set_error(MFFT_ERR_UNSUPPORTED, "3/2-rule with communication='AlltoallN' is not implemented");
  if (can_fuse_pad()) return pencil_forward_padded_fused(u, fu);
  const double isc3 = 1.0 / padscale();
  const bool X = d.decomp == MFFT_PENCIL_X;
  const int64_t mp = M0 / P1, np = M1 / P2;
  const size_t wb = (size_t)std::max(std::max(M0 * N1_1 * q, mp * M1 * q), std::max(std::max(N2_0 * M1 * q, M0 * np * q), mp * np * Mf)) * es;
  for (int i = 0; i < 3; ++i) MFFT_TRY(ensure(work[i], wb));
  void *W0 = work[0].p, *W1 = work[1].p, *W2 = work[2].p;
  MFFT_TRY(stage("fwd_z", 0, [&] { return r2c_rows(u, W0, mp * np, M2, M2, Mf); }));
  if (d.line2d && P > 1)   // line.py:231 + swap_Nq: c0 <- Re c0 - Im cN, cN <- Re cN (cN = column Nf-1, not real here)
    MFFT_TRY(stage("fwd_nyq", 0, [&] { return launch_line_nyquist(W0, mp * np, Mf, Nf - 1, prec, stream); }));
  // only the first Nf modes travel (truncation in z); pack z chunks
  MFFT_TRY(stage("fwd_packz", 0, [&] { return pack_z(W0, W1, mp * np, Mf, false); }));
  MFFT_TRY(stage("fwd_a2a_1", 0, [&] { return xchg(0, true, true, W1, W0); }));
  if (X) {
    // W0 = P2 blocks (mp, np, q): fft y over M1 = P2*np (gather), out (mp, M1, q)
    MFFT_TRY(stage("fwd_y", 0, [&] {
      return col(W0, W1, M1, false, mp, q, np * q, two_level(np, mp * np * q, q), M1 * q, plain(q));
    }));
    // (the 2-D class truncates without the Nyquist fold on one rank: line.py:185 `fu_padded[ks, :Nf]`)
    MFFT_TRY(stage("trunc_y", 0, [&] { return trunc_axis(W1, W0, mp, N1, M1, q, q, 1.0, !(d.line2d && P == 1)); }));
    // pack y chunks (mp, P1, N1_1, q) -> (P1, mp, N1_1, q)
    MFFT_TRY(stage("pack", 0, [&] {
      for (int g = 0; g < P1; ++g)
        MFFT_TRY(box(static_cast<char*>(W0) + (size_t)(g * N1_1 * q) * es, static_cast<char*>(W1) + (size_t)g * (mp * N1_1 * q) * es,
                     mp, 1, N1_1 * q, N1 * q, 0, N1_1 * q, 0));
      return 0;
    }));
    MFFT_TRY(stage("fwd_a2a_2", 0, [&] { return xchg(1, true, true, W1, W2); }));
    MFFT_TRY(stage("fwd_x", 0, [&] { return col(W2, W2, M0, false, 1, N1_1 * q, 0, plain(N1_1 * q), 0, plain(N1_1 * q)); }));
    MFFT_TRY(stage("trunc_x", 0, [&] { return trunc_axis(W2, fu, 1, N0, M0, N1_1 * q, N1_1 * q, isc3); }));
  } else {
    // W0 = (M0, np, q): fft x, truncate to (N0, np, q)
    MFFT_TRY(stage("fwd_x", 0, [&] { return col(W0, W0, M0, false, 1, np * q, 0, plain(np * q), 0, plain(np * q)); }));
    MFFT_TRY(stage("trunc_x", 0, [&] { return trunc_axis(W0, W1, 1, N0, M0, np * q, np * q, 1.0); }));
    MFFT_TRY(stage("fwd_a2a_2", 0, [&] { return xchg(1, true, true, W1, W0); }));
    // W0 = P2 blocks (N2_0, np, q): fft y over M1 gathering, out (N2_0, M1, q)
    MFFT_TRY(stage("fwd_y", 0, [&] {
      return col(W0, W1, M1, false, N2_0, q, np * q, two_level(np, N2_0 * np * q, q), M1 * q, plain(q));
    }));
    MFFT_TRY(stage("trunc_y", 0, [&] { return trunc_axis(W1, fu, N2_0, N1, M1, q, q, isc3); }));
  }
  return 0;
}
