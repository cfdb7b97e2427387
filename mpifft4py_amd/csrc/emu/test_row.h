// test_row.h -- emulator tests of the contiguous-axis kernels: RowFft, R2CFft / C2RFft (plain, column-limited, z-chunked,
// pair-row, wave-packed) and the chirp-z RowFftZ
#pragma once
#include <algorithm>
#include "emu.h"
#include "fft_chirpz.h"

// The comparisons the row tests share.  Complex rows `out` against s times the long-double DFT of the n-point rows `in`:
template <typename T>
static double c2c_rows_error(const std::vector<cx<T>>& in, int pin, const std::vector<cx<T>>& out, int pout, int nrows, int n, bool inv) {
  RelL2 err;
  for (int r = 0; r < nrows; ++r) {
    lvec X = naive_dft(l_vec(&in[(size_t)r * pin], n), inv ? +1 : -1);
    for (int i = 0; i < n; ++i) err.add(out[(size_t)r * pout + i], scaled(X[i], inv ? 1.0L / n : 1.0L));
  }
  return err.value();
}
// ... bins 0 .. nh of the half-spectrum rows `out` against the DFT of the real n-point rows `in`:
template <typename T>
static double r2c_rows_error(const std::vector<T>& in, int pin, const std::vector<cx<T>>& out, int pout, int nrows, int n, int nh) {
  RelL2 err;
  for (int r = 0; r < nrows; ++r) {
    lvec X = naive_dft(l_real_vec(&in[(size_t)r * pin], n), -1);
    for (int k = 0; k <= nh; ++k) err.add(out[(size_t)r * pout + k], X[k]);
  }
  return err.value();
}
// ... real rows `got` against real rows `want` of the same pitch (c2r of r2c against the input; one kernel against another):
template <typename T>
static double real_rows_error(const std::vector<T>& got, const std::vector<T>& want, int pitch, int nrows, int n) {
  RelL2 err;
  for (int r = 0; r < nrows; ++r)
    for (int i = 0; i < n; ++i) err.add(got[(size_t)r * pitch + i], want[(size_t)r * pitch + i]);
  return err.value();
}
// ... real rows `got` against the inverse DFT / N of the first nbins bins of the rows `spec` (N = 2 M points), extended to a
// Hermitian spectrum: the imaginary parts of bins 0 and M are ignored, bins from nbins on are zero
template <typename T>
static double c2r_rows_error(const std::vector<cx<T>>& spec, int pspec, int nbins, const std::vector<T>& got, int pgot, int nrows, int N) {
  const int M = N / 2;
  RelL2 err;
  for (int r = 0; r < nrows; ++r) {
    lvec X(N);
    for (int k = 0; k < N; ++k) { X[k].x = 0; X[k].y = 0; }
    for (int k = 0; k < nbins; ++k) {
      const cx<T> z = spec[(size_t)r * pspec + k];
      X[k].x = z.x; X[k].y = (k == 0 || k == M) ? 0 : z.y;
      if (k > 0 && k < M) { X[N - k].x = z.x; X[N - k].y = -z.y; }
    }
    lvec x = naive_dft(X, +1);
    for (int i = 0; i < N; ++i) err.add(got[(size_t)r * pgot + i], x[i].x / N);
  }
  return err.value();
}

template <class S, typename T, int ROWS, bool INV, bool TWLDS, bool SPLIT = false>
static void test_row() {
  typedef RowFft<S, T, ROWS, INV, TWLDS, false, SPLIT> K;
  const int N = S::N;
  const int nrows = ROWS * 2 + 1;
  Uniform U(99 + N);
  const int pin = N + 3, pout = N + 1;
  std::vector<cx<T>> in((size_t)nrows * pin), out((size_t)nrows * pout);
  U.fill(in);
  auto tw = build_pass_twiddles<S, T>();
  RowParams<T> P{in.data(), out.data(), tw.data(), pin, pout, nrows, INV ? (T)(1.0 / N) : (T)1};
  emu_launch((nrows + ROWS - 1) / ROWS, K::THREADS, K::LDS_BYTES,
             [&](int b, int t, char* lds) { K::body(P, b, t, lds); });
  char name[64];
  snprintf(name, sizeof name, "row r%d %s%s%s", ROWS, INV ? "inv" : "fwd", TWLDS ? " twlds" : "", SPLIT ? " split" : "");
  report(name, N, pname<T>(), c2c_rows_error(in, pin, out, pout, nrows, N, INV), tol_of<T>());
  // z-chunked side (pencil C2C): forward stores into / inverse loads out of nch equal blocks (rows_total, q)
  if (N % 4 == 0 && N >= 8) {
    const int nch = 4, q = N / nch, rows_total = nrows + 2, row0 = 1;
    const ZSplit zs = make_zsplit(q, nch, q, rows_total);
    std::vector<cx<T>> blocks((size_t)rows_total * N, mk<T>((T)3, (T)3)), out2((size_t)nrows * pout);
    typedef RowFft<S, T, ROWS, INV, TWLDS, true, SPLIT> K;
    RowParams<T> Pc{in.data(), out2.data(), tw.data(), pin, pout, nrows, INV ? (T)(1.0 / N) : (T)1, zs, row0};
    if (INV) {       // scatter the plain input rows into the blocks, transform out of them
      for (int r = 0; r < nrows; ++r)
        for (int k = 0; k < N; ++k) blocks[(size_t)(k / q) * rows_total * q + (size_t)(row0 + r) * q + k % q] = in[(size_t)r * pin + k];
      Pc.in = blocks.data();
    } else {
      Pc.out = blocks.data();
    }
    emu_launch((nrows + ROWS - 1) / ROWS, K::THREADS, K::LDS_BYTES, [&](int b, int t, char* lds) { K::body(Pc, b, t, lds); });
    RelL2 err;
    for (int r = 0; r < nrows; ++r)
      for (int k = 0; k < N; ++k)
        err.add(INV ? out2[(size_t)r * pout + k] : blocks[(size_t)(k / q) * rows_total * q + (size_t)(row0 + r) * q + k % q], out[(size_t)r * pout + k]);
    snprintf(name, sizeof name, "row r%d %s z-chunked", ROWS, INV ? "inv" : "fwd");
    report(name, N, pname<T>(), err.value(), 1e-30 + (double)0);   // same arithmetic, other addresses: identical
  }
}

template <class S, typename T, int ROWS, bool TWLDS, bool SPLIT = false, bool MLDS = false>
static void test_real() {
  const int M = S::N, N = 2 * M;
  const int nrows = ROWS + 2;
  Uniform U(7 + N);
  const int pin = N + 2, pout = M + 1 + 2;
  std::vector<T> in((size_t)nrows * pin);
  std::vector<cx<T>> out((size_t)nrows * pout);
  U.fill(in);
  auto tw = build_pass_twiddles<S, T>();
  auto rtw = build_real_twiddles<T>(N);
  {
    typedef R2CFft<S, T, ROWS, TWLDS, false, false, SPLIT> K;
    RealParams<T> P{in.data(), out.data(), tw.data(), rtw.data(), pin, pout, nrows, M + 1, (T)1};
    emu_launch((nrows + ROWS - 1) / ROWS, K::THREADS, K::LDS_BYTES,
               [&](int b, int t, char* lds) { K::body(P, b, t, lds); });
  }
  char name[64];
  snprintf(name, sizeof name, "r2c r%d%s%s", ROWS, TWLDS ? " twlds" : "", SPLIT ? " split" : "");
  report(name, N, pname<T>(), r2c_rows_error(in, pin, out, pout, nrows, N, M), tol_of<T>());
  // c2r of (the r2c result with garbage imaginary parts in bins 0 and M) must return the input
  std::vector<T> back((size_t)nrows * pin, (T)0);
  for (int r = 0; r < nrows; ++r) {
    out[(size_t)r * pout + 0].y = (T)3.5;
    out[(size_t)r * pout + M].y = (T)-2.25;
  }
  {
    typedef C2RFft<S, T, ROWS, TWLDS, false, false, SPLIT, false, MLDS> K;
    RealParams<T> P{out.data(), back.data(), tw.data(), rtw.data(), pout, pin, nrows, M + 1, (T)(1.0 / N)};
    emu_launch((nrows + ROWS - 1) / ROWS, K::THREADS, K::LDS_BYTES,
               [&](int b, int t, char* lds) { K::body(P, b, t, lds); });
  }
  snprintf(name, sizeof name, "c2r(r2c) r%d%s%s%s", ROWS, TWLDS ? " twlds" : "", SPLIT ? " split" : "", MLDS ? " mlds" : "");
  report(name, N, pname<T>(), real_rows_error(back, in, pin, nrows, N), 4 * tol_of<T>());
  // 3/2-rule column handling: r2c keeps only the first `valid` bins, c2r treats the missing ones as zero
  if (M >= 4) {
    const int valid = M / 2 + 1;
    std::vector<cx<T>> part((size_t)nrows * valid, mk<T>((T)9, (T)9));
    {
      typedef R2CFft<S, T, ROWS, TWLDS, true, false, SPLIT> K;
      RealParams<T> P{in.data(), part.data(), tw.data(), rtw.data(), pin, valid, nrows, valid, (T)1};
      emu_launch((nrows + ROWS - 1) / ROWS, K::THREADS, K::LDS_BYTES,
                 [&](int b, int t, char* lds) { K::body(P, b, t, lds); });
    }
    RelL2 err;
    for (int r = 0; r < nrows; ++r)
      for (int k = 0; k < valid; ++k) {
        cx<T> e = out[(size_t)r * pout + k];
        if (k == 0) e.y = 0;        // out[] had its bin-0 imaginary part poisoned above
        err.add(part[(size_t)r * valid + k], e);
      }
    snprintf(name, sizeof name, "r2c valid<M+1 r%d", ROWS);
    report(name, N, pname<T>(), err.value(), 4 * tol_of<T>());
    std::vector<T> b2((size_t)nrows * pin, (T)0);
    {
      typedef C2RFft<S, T, ROWS, TWLDS, true, false, SPLIT, false, MLDS> K;
      RealParams<T> P{part.data(), b2.data(), tw.data(), rtw.data(), valid, pin, nrows, valid, (T)(1.0 / N)};
      emu_launch((nrows + ROWS - 1) / ROWS, K::THREADS, K::LDS_BYTES,
                 [&](int b, int t, char* lds) { K::body(P, b, t, lds); });
    }
    snprintf(name, sizeof name, "c2r valid<M+1 r%d", ROWS);
    report(name, N, pname<T>(), c2r_rows_error(part, valid, valid, b2, pin, nrows, N), 4 * tol_of<T>());
  }
  // z-chunked complex side (fused pencil pack / unpack): the M + 1 bins of a row go to nch blocks (rows_total, len_l);
  // `drop`: the last block has no room for the Nyquist bin (the 'AlltoallN' mode), which then reads back as zero
  if (M >= 4 && M % 2 == 0) {
    for (int dp = 0; dp < 3; ++dp) {        // dp == 2: rows of the blocks further apart than their length (ZSplit pitch)
      const int drop = dp == 1;
      const int nch = 2, q = M / nch, last = q + (drop ? 0 : 1), rows_total = nrows + 3, row0 = 2;
      const int pq = dp == 2 ? q + 3 : q, plast = dp == 2 ? last + 5 : last;
      const ZSplit zs = dp == 2 ? make_zsplit(q, nch, last, rows_total, pq, plast) : make_zsplit(q, nch, last, rows_total);
      std::vector<cx<T>> blocks((size_t)rows_total * (pq * (nch - 1) + plast), mk<T>((T)7, (T)7));
      {
        typedef R2CFft<S, T, ROWS, TWLDS, false, true, SPLIT> K;
        RealParams<T> P{in.data(), blocks.data(), tw.data(), rtw.data(), pin, 0, nrows, M + 1, (T)1, zs, row0};
        emu_launch((nrows + ROWS - 1) / ROWS, K::THREADS, K::LDS_BYTES, [&](int b, int t, char* lds) { K::body(P, b, t, lds); });
      }
      RelL2 err;
      for (int r = 0; r < nrows; ++r)
        for (int k = 0; k <= M - drop; ++k) {
          const int l = std::min(k / q, nch - 1), len = l == nch - 1 ? plast : pq;
          cx<T> e = out[(size_t)r * pout + k];
          if (k == 0 || k == M) e.y = 0;
          err.add(blocks[(size_t)l * rows_total * pq + (size_t)(row0 + r) * len + (k - l * q)], e);
        }
      snprintf(name, sizeof name, "r2c z-chunked%s r%d", drop ? " drop" : dp == 2 ? " pitched" : "", ROWS);
      report(name, N, pname<T>(), err.value(), 4 * tol_of<T>());
      std::vector<T> b3((size_t)nrows * pin, (T)0);
      {
        typedef C2RFft<S, T, ROWS, TWLDS, false, true, SPLIT, false, MLDS> K;
        RealParams<T> P{blocks.data(), b3.data(), tw.data(), rtw.data(), 0, pin, nrows, M + 1, (T)(1.0 / N), zs, row0};
        emu_launch((nrows + ROWS - 1) / ROWS, K::THREADS, K::LDS_BYTES, [&](int b, int t, char* lds) { K::body(P, b, t, lds); });
      }
      snprintf(name, sizeof name, "c2r z-chunked%s r%d", drop ? " drop" : dp == 2 ? " pitched" : "", ROWS);
      report(name, N, pname<T>(), c2r_rows_error(out, pout, M + 1 - drop, b3, pin, nrows, N), 4 * tol_of<T>());
    }
  }
  // column-limited AND z-chunked (the 3/2-rule pencil transforms): only the first `valid` bins exist, split into
  // nch blocks with an uneven last one (valid = 2 * q + 1: the un-padded mesh's Nyquist column on the last rank)
  if (M >= 12 && M % 3 == 0) {
    const int valid = M / 3 * 2 / 2 * 2 + 1 <= M ? (M / 3) / 2 * 2 + 1 : 3;      // odd, about a third of the bins
    const int nch = 2, q = (valid - 1) / nch, last = q + 1, rows_total = nrows + 2, row0 = 1;
    const ZSplit zs = make_zsplit(q, nch, last, rows_total);
    std::vector<cx<T>> blocks((size_t)rows_total * (q * (nch - 1) + last), mk<T>((T)7, (T)7));
    {
      typedef R2CFft<S, T, ROWS, TWLDS, true, true, SPLIT> K;
      RealParams<T> P{in.data(), blocks.data(), tw.data(), rtw.data(), pin, 0, nrows, valid, (T)1, zs, row0};
      emu_launch((nrows + ROWS - 1) / ROWS, K::THREADS, K::LDS_BYTES, [&](int b, int t, char* lds) { K::body(P, b, t, lds); });
    }
    RelL2 err;
    for (int r = 0; r < nrows; ++r)
      for (int k = 0; k < valid; ++k) {
        const int l = std::min(k / q, nch - 1), len = l == nch - 1 ? last : q;
        cx<T> e = out[(size_t)r * pout + k];
        if (k == 0) e.y = 0;
        err.add(blocks[(size_t)l * rows_total * q + (size_t)(row0 + r) * len + (k - l * q)], e);
      }
    snprintf(name, sizeof name, "r2c valid<M+1 z-chunked r%d", ROWS);
    report(name, N, pname<T>(), err.value(), 4 * tol_of<T>());
    std::vector<T> b4((size_t)nrows * pin, (T)0);
    {
      typedef C2RFft<S, T, ROWS, TWLDS, true, true, SPLIT, false, MLDS> K;
      RealParams<T> P{blocks.data(), b4.data(), tw.data(), rtw.data(), 0, pin, nrows, valid, (T)(1.0 / N), zs, row0};
      emu_launch((nrows + ROWS - 1) / ROWS, K::THREADS, K::LDS_BYTES, [&](int b, int t, char* lds) { K::body(P, b, t, lds); });
    }
    snprintf(name, sizeof name, "c2r valid<M+1 z-chunked r%d", ROWS);
    report(name, N, pname<T>(), c2r_rows_error(out, pout, valid, b4, pin, nrows, N), 4 * tol_of<T>());
  }
}

// Pair-row kernels (R2CFft / C2RFft PAIR): the z pass of the route that splits real / complex LAST.  Forward: the x and y
// transforms of a real (n0, n1, N) field read as complex pairs go in, its half-spectrum must come out.  Inverse: an ARBITRARY
// complex (n0, n1, N/2 + 1) array goes in (not the transform of a real field: the planes kz = 0 and N/2 are not Hermitian); the
// inverse x and y transforms of what comes out, read as reals, must be numpy's irfftn of it (inverse c2c over x and y, then the
// c2r that ignores the imaginary parts of bins 0 and N/2).  Rows and planes of both sides are pitched.  yb > 0: the real side is
// blocked in y (RealPairParams::p_ymap): blocks of yb rows per x, pitched x rows inside a block, pitched blocks.  tile > 0: the
// workgroups take the slots in tiles of tile x tile (pair_slot), xfast: kx fastest inside a tile.
template <class S, typename T, int ROWS, bool TWLDS>
static void test_pair(int n0, int n1, int yb = 0, int tile = 0, bool xfast = false) {
  const int M = S::N, N = 2 * M, Nf = M + 1;
  Uniform U(11 + N + 7 * n0 + n1);
  const int wrow = M + 1, wplane = (yb ? yb : n1) * wrow + 3, crow = Nf + 2, cplane = n1 * crow + 5;      // complex elements
  const int wblock = n0 * wplane + 5;                       // blocked: complex elements between the y blocks
  const size_t wsize = yb ? (size_t)(n1 / yb) * wblock : (size_t)n0 * wplane;
  auto woff = [&](int x, int y) { return yb ? (size_t)(y / yb) * wblock + (size_t)x * wplane + (size_t)(y % yb) * wrow
                                            : (size_t)x * wplane + (size_t)y * wrow; };
  const RowMap ymap = make_rowmap(2 * (i64)wblock, 2 * wrow, yb, n1);
  std::vector<long> wlog(wsize, -1);                        // element of W -> element of the logical (n0, n1, M) array, -1: a gap
  for (int x = 0; x < n0; ++x)
    for (int y = 0; y < n1; ++y)
      for (int k = 0; k < M; ++k) wlog[woff(x, y) + k] = ((long)x * n1 + y) * M + k;
  auto tw = build_pass_twiddles<S, T>();
  auto rtw = build_real_twiddles<T>(N);
  // the long-double transform of axis `ax` (0: x, 1: y) of an (n0, n1, len) array
  auto xy = [&](std::vector<cx<long double>>& a, int len, int ax, int sign) {
    const int n = ax == 0 ? n0 : n1;
    for (int o = 0; o < (ax == 0 ? n1 : n0); ++o)
      for (int k = 0; k < len; ++k) {
        lvec v(n);
        for (int i = 0; i < n; ++i) v[i] = a[((size_t)(ax == 0 ? i : o) * n1 + (ax == 0 ? o : i)) * len + k];
        v = naive_dft(v, sign);
        for (int i = 0; i < n; ++i) a[((size_t)(ax == 0 ? i : o) * n1 + (ax == 0 ? o : i)) * len + k] = v[i];
      }
  };
  const int slots = (n0 / 2 + 1) * n1, grid = (slots + ROWS / 2 - 1) / (ROWS / 2);
  char name[64];
  {
    std::vector<long double> u((size_t)n0 * n1 * N);
    U.fill(u);
    std::vector<cx<long double>> w((size_t)n0 * n1 * M), ref((size_t)n0 * n1 * Nf);
    for (size_t i = 0; i < w.size(); ++i) { w[i].x = u[2 * i]; w[i].y = u[2 * i + 1]; }
    xy(w, M, 1, -1);
    xy(w, M, 0, -1);
    for (int r = 0; r < n0 * n1; ++r) {
      lvec X = naive_dft(l_real_vec(&u[(size_t)r * N], N), -1);
      for (int k = 0; k < Nf; ++k) ref[(size_t)r * Nf + k] = X[k];
    }
    xy(ref, Nf, 1, -1);
    xy(ref, Nf, 0, -1);
    std::vector<cx<T>> W(wsize, mk<T>((T)9, (T)9)), fu((size_t)n0 * cplane, mk<T>((T)7, (T)7));
    for (int x = 0; x < n0; ++x)
      for (int y = 0; y < n1; ++y)
        for (int k = 0; k < M; ++k) {
          const cx<long double> z = w[((size_t)x * n1 + y) * M + k];
          W[woff(x, y) + k] = mk<T>((T)z.x, (T)z.y);
        }
    typedef R2CFft<S, T, ROWS, TWLDS, false, false, false, false, true> K;
    RealPairParams<T> P{{W.data(), fu.data(), tw.data(), rtw.data(), 2 * wrow, crow, slots, Nf, (T)1}};
    P.pn0 = n0; P.pn1 = n1; P.p_rplane = 2 * wplane; P.p_cplane = cplane; P.p_ymap = ymap; P.p_tile = tile; P.p_tile_xfast = xfast;
    emu_launch(grid, K::THREADS, K::LDS_BYTES, [&](int b, int t, char* lds) { K::body(P, b, t, lds); });
    RelL2 err;
    bool gaps = true;        // nothing outside the rows is written
    for (size_t i = 0; i < fu.size(); ++i) {
      const int x = (int)(i / cplane), rem = (int)(i % cplane), y = rem / crow, k = rem % crow;
      if (y < n1 && k < Nf) err.add(fu[i], ref[((size_t)x * n1 + y) * Nf + k]);
      else if (fu[i].x != (T)7 || fu[i].y != (T)7) gaps = false;
    }
    snprintf(name, sizeof name, "r2c pair r%d %dx%d b%d g%d%s%s", ROWS, n0, n1, yb, tile, xfast ? "x" : "", TWLDS ? " twlds" : "");
    report(name, N, pname<T>(), gaps ? err.value() : 1.0, tol_of<T>());
  }
  {
    std::vector<cx<long double>> f((size_t)n0 * n1 * Nf);
    for (auto& z : f) { z.x = U(); z.y = U(); }
    std::vector<cx<T>> fu((size_t)n0 * cplane, mk<T>((T)7, (T)7)), W(wsize, mk<T>((T)9, (T)9));
    for (int r = 0; r < n0 * n1; ++r)
      for (int k = 0; k < Nf; ++k) {
        const cx<T> z = mk<T>((T)f[(size_t)r * Nf + k].x, (T)f[(size_t)r * Nf + k].y);
        fu[(size_t)(r / n1) * cplane + (size_t)(r % n1) * crow + k] = z;
        f[(size_t)r * Nf + k].x = z.x;
        f[(size_t)r * Nf + k].y = z.y;
      }
    // irfftn: inverse x and y, then c2r row by row
    std::vector<cx<long double>> g = f;
    xy(g, Nf, 0, +1);
    xy(g, Nf, 1, +1);
    std::vector<long double> ref((size_t)n0 * n1 * N);
    for (int r = 0; r < n0 * n1; ++r) {
      lvec X(N);
      for (int k = 0; k < Nf; ++k) X[k] = g[(size_t)r * Nf + k];
      X[0].y = 0;
      X[M].y = 0;
      for (int k = 1; k < M; ++k) { X[N - k].x = X[k].x; X[N - k].y = -X[k].y; }
      lvec x = naive_dft(X, +1);
      for (int i = 0; i < N; ++i) ref[(size_t)r * N + i] = x[i].x / ((long double)N * n0 * n1);
    }
    typedef C2RFft<S, T, ROWS, TWLDS, false, false, false, false, false, true> K;
    RealPairParams<T> P{{fu.data(), W.data(), tw.data(), rtw.data(), crow, 2 * wrow, slots, Nf, (T)(1.0 / N)}};
    P.pn0 = n0; P.pn1 = n1; P.p_rplane = 2 * wplane; P.p_cplane = cplane; P.p_ymap = ymap; P.p_tile = tile; P.p_tile_xfast = xfast;
    emu_launch(grid, K::THREADS, K::LDS_BYTES, [&](int b, int t, char* lds) { K::body(P, b, t, lds); });
    bool gaps = true;
    std::vector<cx<long double>> w((size_t)n0 * n1 * M);
    for (size_t i = 0; i < W.size(); ++i) {
      if (wlog[i] >= 0) { w[wlog[i]].x = W[i].x; w[wlog[i]].y = W[i].y; }
      else if (W[i].x != (T)9 || W[i].y != (T)9) gaps = false;
    }
    xy(w, M, 1, +1);
    xy(w, M, 0, +1);
    RelL2 err;
    for (size_t i = 0; i < w.size(); ++i) {
      const cx<long double> got = {w[i].x / ((long double)n0 * n1), w[i].y / ((long double)n0 * n1)}, want = {ref[2 * i], ref[2 * i + 1]};
      err.add(got, want);
    }
    snprintf(name, sizeof name, "c2r pair r%d %dx%d b%d g%d%s%s", ROWS, n0, n1, yb, tile, xfast ? "x" : "", TWLDS ? " twlds" : "");
    report(name, N, pname<T>(), gaps ? err.value() : 1.0, 4 * tol_of<T>());
  }
}

// chirp-z (Bluestein) kernels: runtime length n on the compiled plan S of length M >= 2n-1
template <class S, typename T, int ROWS, bool INV>
static void test_row_z(int n) {
  typedef RowFftZ<S, T, ROWS, 0, INV> K;
  const int nrows = ROWS * 2 + 1;
  Uniform U(990 + n);
  const int pin = n + 3, pout = n + 1;
  std::vector<cx<T>> in((size_t)nrows * pin), out((size_t)nrows * pout);
  U.fill(in);
  auto tw = build_pass_twiddles<S, T>();
  auto ch = build_chirp<T>(n);
  auto bh = build_chirp_filter<T>(n, S::N);
  RowParamsZ<T> P;
  P.in = in.data(); P.out = out.data(); P.tw = tw.data(); P.in_stride = pin; P.out_stride = pout; P.nrows = nrows;
  P.scale = INV ? (T)(1.0 / n) : (T)1; P.chirp = ch.data(); P.bhat = bh.data(); P.n = n;
  emu_launch((nrows + ROWS - 1) / ROWS, K::THREADS, K::LDS_BYTES, [&](int b, int t, char* lds) { K::body(P, b, t, lds); });
  char name[64];
  snprintf(name, sizeof name, "chirpz row M=%d r%d %s", S::N, ROWS, INV ? "inv" : "fwd");
  report(name, n, pname<T>(), c2c_rows_error(in, pin, out, pout, nrows, n, INV), 8 * tol_of<T>());
}

template <class S, typename T, int ROWS>
static void test_real_z(int n) {
  const int nh = n / 2, nrows = ROWS + 2;
  Uniform U(70 + n);
  const int pin = n + 1, pout = nh + 1 + 2;         // odd real pitch on purpose
  std::vector<T> in((size_t)nrows * pin), back((size_t)nrows * pin, (T)0);
  std::vector<cx<T>> out((size_t)nrows * pout);
  U.fill(in);
  auto tw = build_pass_twiddles<S, T>();
  auto ch = build_chirp<T>(n);
  auto bh = build_chirp_filter<T>(n, S::N);
  RealParamsZ<T> P;
  P.in = in.data(); P.out = out.data(); P.tw = tw.data(); P.rtw = nullptr; P.in_stride = pin; P.out_stride = pout;
  P.nrows = nrows; P.valid = nh + 1; P.scale = (T)1; P.chirp = ch.data(); P.bhat = bh.data(); P.n = n;
  {
    typedef RowFftZ<S, T, ROWS, 1, false> K;
    emu_launch((nrows + ROWS - 1) / ROWS, K::THREADS, K::LDS_BYTES, [&](int b, int t, char* lds) { K::body(P, b, t, lds); });
  }
  char name[64];
  snprintf(name, sizeof name, "chirpz r2c M=%d r%d", S::N, ROWS);
  report(name, n, pname<T>(), r2c_rows_error(in, pin, out, pout, nrows, n, nh), 8 * tol_of<T>());
  for (int r = 0; r < nrows; ++r) {                 // garbage where c2r must not look
    out[(size_t)r * pout + 0].y = (T)3.5;
    if (n % 2 == 0) out[(size_t)r * pout + nh].y = (T)-2.25;
  }
  P.in = out.data(); P.out = back.data(); P.in_stride = pout; P.out_stride = pin; P.scale = (T)(1.0 / n);
  {
    typedef RowFftZ<S, T, ROWS, 2, true> K;
    emu_launch((nrows + ROWS - 1) / ROWS, K::THREADS, K::LDS_BYTES, [&](int b, int t, char* lds) { K::body(P, b, t, lds); });
  }
  snprintf(name, sizeof name, "chirpz c2r(r2c) M=%d r%d", S::N, ROWS);
  report(name, n, pname<T>(), real_rows_error(back, in, pin, nrows, n), 16 * tol_of<T>());
}

// half-length real chirp-z (KIND 3 / 4): even real length n = 2m, chirp-z of length m on the plan S (M >= 2m-1)
template <class S, typename T, int ROWS>
static void test_real_zh(int m) {
  const int n = 2 * m, nrows = ROWS + 2;
  Uniform U(170 + n);
  const int pin = n + 2, pout = m + 1 + 2;
  std::vector<T> in((size_t)nrows * pin), back((size_t)nrows * pin, (T)0);
  std::vector<cx<T>> out((size_t)nrows * pout);
  U.fill(in);
  auto tw = build_pass_twiddles<S, T>();
  auto ch = build_chirp<T>(m);
  auto bh = build_chirp_filter<T>(m, S::N);
  auto rtw = build_real_twiddles<T>(n);
  RealParamsZ<T> P;
  P.in = in.data(); P.out = out.data(); P.tw = tw.data(); P.rtw = rtw.data(); P.in_stride = pin; P.out_stride = pout;
  P.nrows = nrows; P.valid = m + 1; P.scale = (T)1; P.chirp = ch.data(); P.bhat = bh.data(); P.n = n;
  {
    typedef RowFftZ<S, T, ROWS, 3, false> K;
    emu_launch((nrows + ROWS - 1) / ROWS, K::THREADS, K::LDS_BYTES, [&](int b, int t, char* lds) { K::body(P, b, t, lds); });
  }
  char name[64];
  snprintf(name, sizeof name, "chirpz/2 r2c M=%d r%d", S::N, ROWS);
  report(name, n, pname<T>(), r2c_rows_error(in, pin, out, pout, nrows, n, m), 8 * tol_of<T>());
  for (int r = 0; r < nrows; ++r) {
    out[(size_t)r * pout + 0].y = (T)3.5;
    out[(size_t)r * pout + m].y = (T)-2.25;
  }
  P.in = out.data(); P.out = back.data(); P.in_stride = pout; P.out_stride = pin; P.scale = (T)(1.0 / n);
  {
    typedef RowFftZ<S, T, ROWS, 4, true> K;
    emu_launch((nrows + ROWS - 1) / ROWS, K::THREADS, K::LDS_BYTES, [&](int b, int t, char* lds) { K::body(P, b, t, lds); });
  }
  snprintf(name, sizeof name, "chirpz/2 c2r(r2c) M=%d r%d", S::N, ROWS);
  report(name, n, pname<T>(), real_rows_error(back, in, pin, nrows, n), 16 * tol_of<T>());
}

// wave-packed c2r (fft_kernels.h C2RFft WP): plain, column-limited and z-chunked, against the input of the r2c kernels
template <class S, typename T, int WAVES, bool SPLIT>
static void test_c2r_wave_packed() {
  if constexpr (S::TPT < 64 && 64 % S::TPT != 0 && S::E % 2 == 0) {      // (register pairing: even E -- registry.h wave_packable)
    constexpr int RPW = 64 / S::TPT, ROWS = WAVES * RPW;
    const int M = S::N, N = 2 * M, nrows = 2 * ROWS + 1;       // the last workgroup is ragged, its last wave too
    Uniform U(99 + N);
    const int pin = N + 2, pout = M + 1 + 2;
    std::vector<T> in((size_t)nrows * pin), back((size_t)nrows * pin, (T)0);
    std::vector<cx<T>> out((size_t)nrows * pout);
    U.fill(in);
    auto tw = build_pass_twiddles<S, T>();
    auto rtw = build_real_twiddles<T>(N);
    {
      typedef R2CFft<S, T, 2, false, false, false, false> K;
      RealParams<T> P{in.data(), out.data(), tw.data(), rtw.data(), pin, pout, nrows, M + 1, (T)1};
      emu_launch((nrows + 1) / 2, K::THREADS, K::LDS_BYTES, [&](int b, int t, char* lds) { K::body(P, b, t, lds); });
    }
    char name[64];
    {     // r2c, wave-packed, against the dense kernel's output (and, column-limited, its first bins)
      std::vector<cx<T>> o2((size_t)nrows * pout, mk<T>((T)7, (T)7)), o3((size_t)nrows * (M / 2 + 1), mk<T>((T)7, (T)7));
      {
        typedef R2CFft<S, T, ROWS, false, false, false, SPLIT, true> K;
        static_assert(K::THREADS == WAVES * 64, "whole waves");
        RealParams<T> P{in.data(), o2.data(), tw.data(), rtw.data(), pin, pout, nrows, M + 1, (T)1};
        emu_launch((nrows + ROWS - 1) / ROWS, K::THREADS, K::LDS_BYTES, [&](int b, int t, char* lds) { K::body(P, b, t, lds); });
      }
      {
        typedef R2CFft<S, T, ROWS, false, true, false, SPLIT, true> K;
        RealParams<T> P{in.data(), o3.data(), tw.data(), rtw.data(), pin, M / 2 + 1, nrows, M / 2 + 1, (T)1};
        emu_launch((nrows + ROWS - 1) / ROWS, K::THREADS, K::LDS_BYTES, [&](int b, int t, char* lds) { K::body(P, b, t, lds); });
      }
      long double nn = 0, dd = 0, n3 = 0;      // (the differences in T, their squares in long double: not RelL2::add)
      for (int r = 0; r < nrows; ++r)
        for (int k = 0; k <= M; ++k) {
          const cx<T> a = o2[(size_t)r * pout + k], e = out[(size_t)r * pout + k];
          nn += (long double)(a.x - e.x) * (a.x - e.x) + (long double)(a.y - e.y) * (a.y - e.y);
          dd += (long double)e.x * e.x + (long double)e.y * e.y;
          if (k <= M / 2) {
            const cx<T> c = o3[(size_t)r * (M / 2 + 1) + k];
            n3 += (long double)(c.x - e.x) * (c.x - e.x) + (long double)(c.y - e.y) * (c.y - e.y);
          }
        }
      snprintf(name, sizeof name, "r2c wave-packed w%d%s", WAVES, SPLIT ? " split" : "");
      report(name, N, pname<T>(), (double)sqrtl(nn / dd), 4 * tol_of<T>());
      snprintf(name, sizeof name, "r2c wave-packed valid<M+1 w%d", WAVES);
      report(name, N, pname<T>(), (double)sqrtl(n3 / dd), 4 * tol_of<T>());
    }
    for (int r = 0; r < nrows; ++r) { out[(size_t)r * pout].y = (T)3.5; out[(size_t)r * pout + M].y = (T)-2.25; }
    {
      typedef C2RFft<S, T, ROWS, false, false, false, SPLIT, true> K;
      static_assert(K::THREADS == WAVES * 64, "whole waves");
      RealParams<T> P{out.data(), back.data(), tw.data(), rtw.data(), pout, pin, nrows, M + 1, (T)(1.0 / N)};
      emu_launch((nrows + ROWS - 1) / ROWS, K::THREADS, K::LDS_BYTES, [&](int b, int t, char* lds) { K::body(P, b, t, lds); });
    }
    snprintf(name, sizeof name, "c2r wave-packed w%d%s", WAVES, SPLIT ? " split" : "");
    report(name, N, pname<T>(), real_rows_error(back, in, pin, nrows, N), 4 * tol_of<T>());
    // column-limited: bins >= valid read as zero
    const int valid = M / 2 + 1;
    std::vector<cx<T>> part((size_t)nrows * valid);
    for (int r = 0; r < nrows; ++r)
      for (int k = 0; k < valid; ++k) part[(size_t)r * valid + k] = out[(size_t)r * pout + k];
    std::vector<T> b1((size_t)nrows * pin, (T)0), b2((size_t)nrows * pin, (T)0);
    {
      typedef C2RFft<S, T, ROWS, false, true, false, SPLIT, true> K;
      RealParams<T> P{part.data(), b1.data(), tw.data(), rtw.data(), valid, pin, nrows, valid, (T)(1.0 / N)};
      emu_launch((nrows + ROWS - 1) / ROWS, K::THREADS, K::LDS_BYTES, [&](int b, int t, char* lds) { K::body(P, b, t, lds); });
    }
    {
      typedef C2RFft<S, T, 2, false, true, false, false, false> K;      // the unpacked kernel as the reference
      RealParams<T> P{part.data(), b2.data(), tw.data(), rtw.data(), valid, pin, nrows, valid, (T)(1.0 / N)};
      emu_launch((nrows + 1) / 2, K::THREADS, K::LDS_BYTES, [&](int b, int t, char* lds) { K::body(P, b, t, lds); });
    }
    snprintf(name, sizeof name, "c2r wave-packed valid<M+1 w%d", WAVES);
    report(name, N, pname<T>(), real_rows_error(b1, b2, pin, nrows, pin), 4 * tol_of<T>());      // (the whole pitch: the gaps stay 0)
  }
}
