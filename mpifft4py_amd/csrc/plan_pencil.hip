// plan_pencil.hip -- the pencil routes (x- and y-aligned): blocking, and their exchange pipelines.
#include "plan_impl.h"

using namespace mfft;

// ===========================================================================
// pencil
// ===========================================================================
// pack the z chunks of Z (rows, nf) into consecutive (rows, len_l) blocks / the reverse
int mfft_plan_s::pack_z(const void* Z, void* S, int64_t rows, int64_t nf, bool unpack) {
  size_t off = 0;
  for (const Chunk& c : zc) {
    const char* zp = static_cast<const char*>(Z) + (size_t)c.start * es;
    char* sp = static_cast<char*>(S) + off;
    if (!unpack) MFFT_TRY(box(zp, sp, 1, rows, c.len, 0, nf, 0, c.len));
    else MFFT_TRY(box(sp, const_cast<char*>(zp), 1, rows, c.len, 0, c.len, 0, nf));
    off += (size_t)(rows * c.len) * es;
  }
  return 0;
}

// z chunks of rows [r0, r0+nr) of Z (rows_total, nf) <-> the matching sub-blocks of the packed chunk blocks
static int pack_z_rows(mfft_plan_s* p, const void* Z, void* S, int64_t rows_total, int64_t r0, int64_t nr, int64_t nf,
                       const std::vector<Chunk>& zc, bool unpack) {
  size_t base = 0;
  for (const Chunk& c : zc) {
    const char* zp = static_cast<const char*>(Z) + (size_t)(r0 * nf + c.start) * p->es;
    char* sp = static_cast<char*>(S) + base + (size_t)(r0 * c.len) * p->es;
    if (!unpack) MFFT_TRY(p->box(zp, sp, 1, nr, c.len, 0, nf, 0, c.len));
    else MFFT_TRY(p->box(sp, const_cast<char*>(zp), 1, nr, c.len, 0, c.len, 0, nf));
    base += (size_t)(rows_total * c.len) * p->es;
  }
  return 0;
}

// ---- pencil, X alignment: batches of local x rows pipelined through BOTH exchanges -------------------
// Everything up to the final x transform (forward) / after the first x transform (inverse) is independent per
// local x row i, and the blocks a row batch contributes to either exchange are contiguous in the packed layouts,
// so batch b's exchanges run on the communication stream while batch b+1 is transformed on the compute stream.
int mfft_plan_s::pencil_forward_pipelined_x(const void* u, void* fu) {
  const int64_t m = N1_0, n = N2_1;
  const double Cb = (double)(m * n * Nf) * es, Rb = (double)(m * n * N2) * rs;
  const bool zsolo = P2 == 1, g2solo = P1 == 1;
  // x-row pitch of the blocks of the second exchange: N1_1 * q, plus a cache line where that pitch reads slowly
  // (xplane_pad); then the chunks land in a work buffer and the x transform runs out of place into the result
  const int64_t SX = N1_1 * q + xplane_pad(true);
  const bool xoop = SX != N1_1 * q;
  const int64_t PQ = zrow_pitch(q, true);        // row pitch of the received z blocks (zrow_pitch: q, or whole cache lines)
  const size_t wb = (size_t)std::max(std::max(std::max(m * n * Nf, zsend_elems(m * n)), m * N1 * PQ), xoop ? N0 * SX : (int64_t)0) * es;
  for (int i = 0; i < 3; ++i) MFFT_TRY(ensure(work[i], wb));
  char *W0 = static_cast<char*>(work[0].p), *W1 = static_cast<char*>(work[1].p), *W2 = static_cast<char*>(work[2].p);
  const char* in = static_cast<const char*>(u);
  char* out = static_cast<char*>(fu);
  const int B = nbatch;
  auto rows = [&](int b, int64_t* i0, int64_t* mb) { *i0 = m * b / B; *mb = m * (b + 1) / B - *i0; };
  // z transform + z-chunk pack of a batch on the compute stream, its exchange on the communication stream
  for (int b = 0; b < B; ++b) {
    int64_t i0, mb;
    rows(b, &i0, &mb);
    if (!zsolo && zfuse) {          // the z transform writes the batch's rows of the send blocks itself
      MFFT_TRY(stage("fwd_z", (Rb + Cb) / B, [&] {
        return z_forward_chunked(in + (size_t)(i0 * n * N2) * rs, W1, mb * n, i0 * n, m * n);
      }));
    } else {
      MFFT_TRY(stage("fwd_z", (Rb + Cb) / B, [&] {
        return z_forward(in + (size_t)(i0 * n * N2) * rs, W0 + (size_t)(i0 * n * Nf) * es, mb * n, N2, Nf);
      }));
      if (zsolo) continue;
      MFFT_TRY(stage("fwd_packz", 0, [&] { return pack_z_rows(this, W0, W1, m * n, i0 * n, mb * n, Nf, zc, false); }));
    }
    MFFT_TRY(comm_waits(ev_compute[b]));
    MFFT_TRY(exchange_piece("fwd_a2a_1", 0, true, b, W1, W2, ev_comm[b]));
  }
  // y transform of a batch as soon as its z chunks have arrived; W0 is free again (all packs are behind us on
  // this stream) and takes the P1 blocks (m, N1_1, q) that feed the second exchange
  const char* ysrc = zsolo ? W0 : W2;
  char* ydst = g2solo ? out : (zsolo ? W1 : W0);
  // padded pitch: where the second exchange delivers.  W1 was the send buffer of the z exchanges, all of which are ahead
  // of every second exchange on the communication stream; on a P1 x 1 grid (no z exchange) W1 is ydst and W2 is unused
  char* xrecv = xoop ? (zsolo ? W2 : W1) : out;
  for (int b = 0; b < B; ++b) {
    int64_t i0, mb;
    rows(b, &i0, &mb);
    if (!zsolo) MFFT_HIP(hipStreamWaitEvent(stream, ev_comm[b], 0));
    MFFT_TRY(stage("fwd_y", 2 * Cb / B, [&] {
      return col(ysrc + (size_t)(i0 * n * PQ) * es, ydst + (size_t)(i0 * SX) * es, N1, false, mb, q, n * PQ,
                 two_level(n, m * n * PQ, PQ), SX, two_level(N1_1, m * SX, q));
    }));
    if (g2solo) continue;
    MFFT_TRY(comm_waits(ev2_compute[b]));
    MFFT_TRY(exchange_piece("fwd_a2a_2", 1, true, b, ydst, xrecv, ev2_comm[b]));
  }
  if (!g2solo) MFFT_HIP(hipStreamWaitEvent(stream, ev2_comm[B - 1], 0));     // in order on the comm stream: all batches
  if (xoop) {
    MFFT_TRY(stage("fwd_x", 2 * Cb, [&] { return col(xrecv, fu, N0, false, 1, N1_1 * q, 0, plain(SX), 0, plain(N1_1 * q)); }));
    return 0;
  }
  MFFT_TRY(stage("fwd_x", 2 * Cb, [&] { return col(fu, fu, N0, false, 1, N1_1 * q, 0, plain(N1_1 * q), 0, plain(N1_1 * q)); }));
  return 0;
}

int mfft_plan_s::pencil_backward_pipelined_x(const void* src, void* u) {
  const int64_t m = N1_0, n = N2_1;
  const double Cb = (double)(m * n * Nf) * es, Rb = (double)(m * n * N2) * rs;
  const bool zsolo = P2 == 1, g2solo = P1 == 1;
  const size_t wb = (size_t)std::max(m * n * Nf, m * N1 * q) * es;
  for (int i = 0; i < 2; ++i) MFFT_TRY(ensure(work[i], wb));
  // third buffer: work[2].p, unless it holds the masked copy of the spectrum (src)
  const bool src_in_work2 = work[2].p != nullptr && src == work[2].p;
  if (src_in_work2) MFFT_TRY(ensure(work3, wb));
  else MFFT_TRY(ensure(work[2], wb));
  char *W0 = static_cast<char*>(work[0].p), *W1 = static_cast<char*>(work[1].p);
  char* W2 = static_cast<char*>(src_in_work2 ? work3.p : work[2].p);
  char* out = static_cast<char*>(u);
  const int B = nbatch;
  auto rows = [&](int b, int64_t* i0, int64_t* mb) { *i0 = m * b / B; *mb = m * (b + 1) / B - *i0; };
  MFFT_TRY(stage("bwd_x", 2 * Cb, [&] { return col(src, W0, N0, true, 1, N1_1 * q, 0, plain(N1_1 * q), 0, plain(N1_1 * q)); }));
  if (!g2solo) {
    MFFT_TRY(comm_waits(ev2_compute[0]));
    for (int b = 0; b < B; ++b) {
      int64_t i0, mb;
      rows(b, &i0, &mb);
      MFFT_TRY(exchange_piece("bwd_a2a_2", 1, false, b, W0, W1, ev2_comm[b]));
    }
  }
  // y transform of a batch (P1 blocks gathered through the row map) -> P2 blocks (m, n, q) in W2, then its z exchange
  const char* ysrc = g2solo ? W0 : W1;
  // Where the z exchange delivers its chunks.  With a second exchange (P1 > 1) every bwd_a2a_2 is ahead of it on the
  // communication stream and the y transforms read W1, so W0 is free.  On a 1 x P2 grid there is no second exchange and
  // the y transforms of LATER batches still read W0 on the compute stream: the chunks go to W1 (unused there) and are
  // unpacked into W0 once every y transform is behind the unpack on the compute stream.
  char* zrecv = g2solo ? W1 : W0;
  char* zfull = g2solo ? W0 : W1;
  for (int b = 0; b < B; ++b) {
    int64_t i0, mb;
    rows(b, &i0, &mb);
    if (!g2solo) MFFT_HIP(hipStreamWaitEvent(stream, ev2_comm[b], 0));
    MFFT_TRY(stage("bwd_y", 2 * Cb / B, [&] {
      return col(ysrc + (size_t)(i0 * N1_1 * q) * es, W2 + (size_t)(i0 * n * q) * es, N1, true, mb, q, N1_1 * q,
                 two_level(N1_1, m * N1_1 * q, q), n * q, two_level(n, m * n * q, q));
    }));
    if (zsolo) continue;
    MFFT_TRY(comm_waits(ev_compute[b]));
    MFFT_TRY(exchange_piece("bwd_a2a_1", 0, false, b, W2, zrecv, ev_comm[b]));
  }
  // z chunks of a batch back into full rows (zfull: every y transform that read it is behind us on this stream), c2r
  for (int b = 0; b < B; ++b) {
    int64_t i0, mb;
    rows(b, &i0, &mb);
    const char* zin = W2 + (size_t)(i0 * n * Nf) * es;
    if (!zsolo) {
      MFFT_HIP(hipStreamWaitEvent(stream, ev_comm[b], 0));
      if (zfuse) {                    // the z transform reads the batch's rows out of the received blocks itself
        MFFT_TRY(stage("bwd_z", (Rb + Cb) / B, [&] {
          return z_backward_chunked(zrecv, out + (size_t)(i0 * n * N2) * rs, mb * n, i0 * n, m * n);
        }));
        continue;
      }
      MFFT_TRY(stage("bwd_unpackz", 0, [&] { return pack_z_rows(this, zfull, zrecv, m * n, i0 * n, mb * n, Nf, zc, true); }));
      zin = zfull + (size_t)(i0 * n * Nf) * es;
    }
    MFFT_TRY(stage("bwd_z", (Rb + Cb) / B, [&] {
      return z_backward(zin, out + (size_t)(i0 * n * N2) * rs, mb * n, N2, Nf);
    }));
  }
  return 0;
}

// ---- pencil, Y alignment: exchange pipeline in two halves ------------------------------------------------------
// (pencil.py:730-754 forward, 483-507 inverse).  The x transform between the two exchanges needs every row of both,
// so the pipeline is cut there: the z stage runs in batches of the local x rows, each batch's z-splitting exchange on
// the communication stream while the next batch is transformed (the z transform writes the send blocks itself: zfuse);
// after the x transform the x-chunk exchange goes out in batches of the rows a rank owns afterwards, and the y
// transform of a batch starts as soon as that batch has landed.  Compute order z0 z1 .. x y0 y1 ..; only z0, the x
// transform and the last y batch are not overlapped.  Needs P1 > 1, P2 > 1 and the fused z-chunk kernels.
int mfft_plan_s::pencil_forward_pipelined_y(const void* u, void* fu) {
  const int64_t m = N1_0, n = N2_1;
  const double Cb = (double)(m * n * Nf) * es, Rb = (double)(m * n * N2) * rs;
  const int64_t PQ = zrow_pitch(q, true);        // row pitch of the z blocks: it stays through the x pass and the second exchange
  const size_t wb = (size_t)std::max(std::max(m * n * Nf, zsend_elems(m * n)), N0 * n * PQ) * es;
  for (int i = 0; i < 2; ++i) MFFT_TRY(ensure(work[i], wb));
  char *W0 = static_cast<char*>(work[0].p), *W1 = static_cast<char*>(work[1].p);
  const char* in = static_cast<const char*>(u);
  char* out = static_cast<char*>(fu);
  const int B = nbatch;
  for (int b = 0; b < B; ++b) {
    const int64_t i0 = m * b / B, mb = m * (b + 1) / B - i0;
    MFFT_TRY(stage("fwd_z", (Rb + Cb) / B, [&] {
      return z_forward_chunked(in + (size_t)(i0 * n * N2) * rs, W1, mb * n, i0 * n, m * n);
    }));
    MFFT_TRY(comm_waits(ev_compute[b]));
    MFFT_TRY(exchange_piece("fwd_a2a_1", 0, true, b, W1, W0, ev_comm[b]));
  }
  MFFT_HIP(hipStreamWaitEvent(stream, ev_comm[B - 1], 0));                    // in order on the comm stream: all batches
  MFFT_TRY(stage("fwd_x", 2 * Cb, [&] { return col(W0, W0, N0, false, 1, n * PQ, 0, plain(n * PQ), 0, plain(n * PQ)); }));
  MFFT_TRY(comm_waits(ev2_compute[0]));
  for (int b = 0; b < B; ++b) {
    MFFT_TRY(exchange_piece("fwd_a2a_2", 1, true, b, W0, W1, ev2_comm[b]));      // W1: every z exchange read it long ago
  }
  for (int b = 0; b < B; ++b) {
    const int64_t x0 = N2_0 * b / B, xb = N2_0 * (b + 1) / B - x0;
    MFFT_HIP(hipStreamWaitEvent(stream, ev2_comm[b], 0));
    MFFT_TRY(stage("fwd_y", 2 * Cb / B, [&] {
      return col(W1 + (size_t)(x0 * n * PQ) * es, out + (size_t)(x0 * N1 * q) * es, N1, false, xb, q, n * PQ,
                 two_level(n, N2_0 * n * PQ, PQ), N1 * q, plain(q));
    }));
  }
  return 0;
}

int mfft_plan_s::pencil_backward_pipelined_y(const void* src, void* u) {
  const int64_t m = N1_0, n = N2_1;
  const double Cb = (double)(m * n * Nf) * es, Rb = (double)(m * n * N2) * rs;
  const int64_t SY = n * q + xplane_pad(false);        // x-row pitch of the blocks of the x-chunk exchange (see xplane_pad)
  const bool xoop = SY != n * q;
  const size_t wb = (size_t)std::max(m * n * Nf, N0 * SY) * es;
  for (int i = 0; i < 2; ++i) MFFT_TRY(ensure(work[i], wb));
  char *W0 = static_cast<char*>(work[0].p), *W1 = static_cast<char*>(work[1].p);
  const char* in = static_cast<const char*>(src);
  char* out = static_cast<char*>(u);
  const int B = nbatch;
  // y transform of a batch of my rows (written as P2 blocks (N2_0, n, q)), its x-chunk exchange behind it
  for (int b = 0; b < B; ++b) {
    const int64_t x0 = N2_0 * b / B, xb = N2_0 * (b + 1) / B - x0;
    MFFT_TRY(stage("bwd_y", 2 * Cb / B, [&] {
      return col(in + (size_t)(x0 * N1 * q) * es, W0 + (size_t)(x0 * SY) * es, N1, true, xb, q, N1 * q, plain(q), SY,
                 two_level(n, N2_0 * SY, q));
    }));
    MFFT_TRY(comm_waits(ev2_compute[b]));
    MFFT_TRY(exchange_piece("bwd_a2a_2", 1, false, b, W0, W1, ev2_comm[b]));
  }
  MFFT_HIP(hipStreamWaitEvent(stream, ev2_comm[B - 1], 0));
  // x transform: in place on the received (N0, n, q), or -- rows SY apart -- out of place into W0, which every x-chunk
  // exchange has read by now; the z-gathering exchange then goes the other way round
  char *xsend = W1, *zrecv = W0;
  if (xoop) {
    MFFT_TRY(stage("bwd_x", 2 * Cb, [&] { return col(W1, W0, N0, true, 1, n * q, 0, plain(SY), 0, plain(n * q)); }));
    xsend = W0;
    zrecv = W1;
  } else {
    MFFT_TRY(stage("bwd_x", 2 * Cb, [&] { return col(W1, W1, N0, true, 1, n * q, 0, plain(n * q), 0, plain(n * q)); }));
  }
  MFFT_TRY(comm_waits(ev_compute[0]));
  for (int b = 0; b < B; ++b) {
    MFFT_TRY(exchange_piece("bwd_a2a_1", 0, false, b, xsend, zrecv, ev_comm[b]));
  }
  for (int b = 0; b < B; ++b) {
    const int64_t i0 = m * b / B, mb = m * (b + 1) / B - i0;
    MFFT_HIP(hipStreamWaitEvent(stream, ev_comm[b], 0));
    MFFT_TRY(stage("bwd_z", (Rb + Cb) / B, [&] {
      return z_backward_chunked(zrecv, out + (size_t)(i0 * n * N2) * rs, mb * n, i0 * n, m * n);
    }));
  }
  return 0;
}

int mfft_plan_s::pencil_forward(const void* u, void* fu) {
  if (nbatch > 1) return d.decomp == MFFT_PENCIL_X ? pencil_forward_pipelined_x(u, fu) : pencil_forward_pipelined_y(u, fu);
  const int64_t m = N1_0, n = N2_1;                 // local real rows in x, y
  const double Cb = (double)(m * n * Nf) * es, Rb = (double)(m * n * N2) * rs;
  const bool X = d.decomp == MFFT_PENCIL_X;
  // a group of one rank exchanges nothing: its pack / copy steps are skipped altogether
  const bool zsolo = (X ? P2 : P1) == 1 && !d.drop_nyquist, g2solo = (X ? P1 : P2) == 1;
  // largest intermediate of this alignment: X: (m, N1, q) after the z exchange; Y: (N0, n, q) after it
  const int64_t SX = N1_1 * q + (X ? xplane_pad(true) : 0);     // x-row pitch of the blocks of the second exchange (X)
  // row pitch of the received z blocks: q, or whole cache lines where the fused z kernel wrote them so (zrow_pitch)
  const int64_t PQ = (!zsolo && zfuse) ? zrow_pitch(q, true) : q;
  const size_t wb = (size_t)std::max(std::max(m * n * Nf, zsend_elems(m * n)), X ? std::max(m * N1 * PQ, N0 * SX) : N0 * n * PQ) * es;
  MFFT_TRY(ensure(work[0], wb));
  MFFT_TRY(ensure(work[1], wb));
  void *W0 = work[0].p, *W1 = work[1].p;
  if (!zsolo && zfuse) {            // z transform straight into the Pz send blocks (pencil.py:218-246 fused)
    MFFT_TRY(stage("fwd_z", Rb + Cb, [&] { return z_forward_chunked(u, W1, m * n, 0, m * n); }));
    MFFT_TRY(stage("fwd_a2a_1", 0, [&] { return xchg(0, true, false, W1, W0); }));
  } else {
    MFFT_TRY(stage("fwd_z", Rb + Cb, [&] { return z_forward(u, W0, m * n, N2, Nf); }));
    if (!zsolo) {
      MFFT_TRY(stage("fwd_packz", 0, [&] { return pack_z(W0, W1, m * n, Nf, false); }));
      MFFT_TRY(stage("fwd_a2a_1", 0, [&] { return xchg(0, true, false, W1, W0); }));
    }
  }
  if (X) {
    // W0 = P2 blocks (m, n, q) -> y transform (gathers y through two-level rows) -> P1 blocks (m, N1_1, q)
    void* ydst = g2solo ? fu : W1;
    MFFT_TRY(stage("fwd_y", 2 * Cb, [&] {
      return col(W0, ydst, N1, false, m, q, n * PQ, two_level(n, m * n * PQ, PQ), SX, two_level(N1_1, m * SX, q));
    }));
    if (g2solo || (xpass_inplace && SX == N1_1 * q)) {
      if (!g2solo) MFFT_TRY(stage("fwd_a2a_2", 0, [&] { return xchg(1, true, false, W1, fu); }));
      MFFT_TRY(stage("fwd_x", 2 * Cb, [&] { return col(fu, fu, N0, false, 1, N1_1 * q, 0, plain(N1_1 * q), 0, plain(N1_1 * q)); }));
    } else {
      // the chunks land in W0 (free: the y transform has read it), rows SX apart; x transform out of place into the result
      MFFT_TRY(stage("fwd_a2a_2", 0, [&] { return xchg(1, true, false, W1, W0); }));
      MFFT_TRY(stage("fwd_x", 2 * Cb, [&] { return col(W0, fu, N0, false, 1, N1_1 * q, 0, plain(SX), 0, plain(N1_1 * q)); }));
    }
  } else {
    // W0 = (N0, n, q): x transform in place, x chunks are contiguous -> exchange -> y transform gathers
    MFFT_TRY(stage("fwd_x", 2 * Cb, [&] { return col(W0, W0, N0, false, 1, n * PQ, 0, plain(n * PQ), 0, plain(n * PQ)); }));
    void* ysrc = W0;
    if (!g2solo) {
      MFFT_TRY(stage("fwd_a2a_2", 0, [&] { return xchg(1, true, false, W0, W1); }));
      ysrc = W1;
    }
    MFFT_TRY(stage("fwd_y", 2 * Cb, [&] {
      return col(ysrc, fu, N1, false, N2_0, q, n * PQ, two_level(n, N2_0 * n * PQ, PQ), N1 * q, plain(q));
    }));
  }
  return 0;
}

int mfft_plan_s::pencil_backward(const void* fu, void* u, bool masked) {
  const int64_t m = N1_0, n = N2_1;
  const double Cb = (double)(m * n * Nf) * es, Rb = (double)(m * n * N2) * rs;
  const bool X = d.decomp == MFFT_PENCIL_X;
  const bool zsolo = (X ? P2 : P1) == 1 && !d.drop_nyquist, g2solo = (X ? P1 : P2) == 1;
  const void* src = fu;
  MaskScope mask_scope{this};
  if (masked) {
    bool fused = false;
    MFFT_TRY(fuse_mask(fu, X ? N0 : N1, &fused));
    if (!fused) {
      void* mm = nullptr;
      MFFT_TRY(stage("bwd_mask", 2 * Cb, [&] { return apply_mask_copy(fu, &mm); }));
      src = mm;
    }
  }
  if (nbatch > 1) return d.decomp == MFFT_PENCIL_X ? pencil_backward_pipelined_x(src, u) : pencil_backward_pipelined_y(src, u);
  // largest intermediate of this alignment: X: (m, N1, q) after the z exchange; Y: (N0, n, q) after it
  const int64_t SY = n * q + (X ? 0 : xplane_pad(false));       // x-row pitch of the blocks of the second exchange (Y)
  const size_t wb = (size_t)std::max(m * n * Nf, X ? m * N1 * q : N0 * SY) * es;
  MFFT_TRY(ensure(work[0], wb));
  MFFT_TRY(ensure(work[1], wb));
  void *W0 = work[0].p, *W1 = work[1].p;
  void* cur = nullptr;     // buffer holding the Pz blocks (m, n, q) that enter the z-gathering exchange
  if (X) {
    MFFT_TRY(stage("bwd_x", 2 * Cb, [&] { return col(src, W0, N0, true, 1, N1_1 * q, 0, plain(N1_1 * q), 0, plain(N1_1 * q)); }));
    void* ysrc = W0;
    if (!g2solo) {
      MFFT_TRY(stage("bwd_a2a_2", 0, [&] { return xchg(1, false, false, W0, W1); }));
      ysrc = W1;
    }
    cur = ysrc == W0 ? W1 : W0;
    MFFT_TRY(stage("bwd_y", 2 * Cb, [&] {
      return col(ysrc, cur, N1, true, m, q, N1_1 * q, two_level(N1_1, m * N1_1 * q, q), n * q, two_level(n, m * n * q, q));
    }));
  } else {
    MFFT_TRY(stage("bwd_y", 2 * Cb, [&] {
      return col(src, W0, N1, true, N2_0, q, N1 * q, plain(q), SY, two_level(n, N2_0 * SY, q));
    }));
    cur = W0;
    if (!g2solo) {
      MFFT_TRY(stage("bwd_a2a_2", 0, [&] { return xchg(1, false, false, W0, W1); }));
      cur = W1;
    }
    if (g2solo || (xpass_inplace && SY == n * q)) {
      // (N0, n, q): x transform in place; its x chunks are the contiguous blocks of the next exchange
      MFFT_TRY(stage("bwd_x", 2 * Cb, [&] { return col(cur, cur, N0, true, 1, n * q, 0, plain(n * q), 0, plain(n * q)); }));
    } else {
      // rows SY apart in W1 -> compact (N0, n, q) in W0 (free: the exchange has sent it), out of place
      MFFT_TRY(stage("bwd_x", 2 * Cb, [&] { return col(W1, W0, N0, true, 1, n * q, 0, plain(SY), 0, plain(n * q)); }));
      cur = W0;
    }
  }
  if (!zsolo) {
    void* other = cur == W0 ? W1 : W0;
    MFFT_TRY(stage("bwd_a2a_1", 0, [&] { return xchg(0, false, false, cur, other); }));
    if (zfuse) {      // the z transform reads the received Pz blocks itself (a dropped Nyquist column reads as zero)
      MFFT_TRY(stage("bwd_z", Rb + Cb, [&] { return z_backward_chunked(other, u, m * n, 0, m * n); }));
      return 0;
    }
    MFFT_TRY(stage("bwd_unpackz", 0, [&] { return pack_z(cur, other, m * n, Nf, true); }));
  }
  if (d.drop_nyquist)   // the neglected Nyquist column counts as zero (pencil.py:430, 1045)
    MFFT_HIP(hipMemset2DAsync(static_cast<char*>(cur) + (size_t)(Nf - 1) * es, (size_t)Nf * es, 0, es, (size_t)(m * n), stream));
  MFFT_TRY(stage("bwd_z", Rb + Cb, [&] { return z_backward(cur, u, m * n, N2, Nf); }));
  return 0;
}

