// plan_impl.h -- what a plan is: the data behind mfft_plan_t and the small helpers every route uses.
//
// Internal to the executor's own units (plan_create.hip: how a plan is made and entered; plan_sched.hip: decomposition,
// layout rules, exchange schedules; plan_slab.hip, plan_pencil.hip, plan_dealias.hip, plan_nonlinear.hip: one route
// family each).  Everything else sees mfft_plan_s as an opaque type and goes through mfft_internal.h.
//
// The routes restate, for device-resident data and HIP kernels, the stage ordering of
//   slab  R2C/C2C : mpiFFT4py/slab.py:349-443 (fftn), 214-308 (ifftn), 743-772, 638-669
//   pencil R2CY   : mpiFFT4py/pencil.py:730-754 (fftn), 483-507 (ifftn)
//   pencil R2CX   : mpiFFT4py/pencil.py:1312-1337 (fftn), 1082-1105 (ifftn)
//   3/2-rule      : slab.py:250-268, 310-344, 372-386, 445-483; pencil.py:604-632,
//                   858-883, 1196-1224, 1440-1475
// with the pack / unpack copies (slab.py:403, cython/maths.pyx:21-31 and the
// Alltoallw sub-array types) folded into the strided FFT kernels' two-level row
// addressing wherever the split axis is not the contiguous one.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include "comm.h"
#include "mfft_internal.h"

#ifndef MFFT_P1_XPAD_DEFAULT
#define MFFT_P1_XPAD_DEFAULT 0      // one-rank real transforms: cache lines added to slow plane pitches of the intermediate (p1_plane_pad; measured: no gain)
#endif

namespace mfft {

// Environment switches.  WHEN a switch is read is part of its meaning: at plan creation (decomp_init, mfft_plan_create),
// once per process (function-local statics) or at every call (MFFT_NO_PRUNE, MFFT_NO_MASK_FUSION).
inline bool env_on(const char* name) {               // set and non-zero
  const char* e = getenv(name);
  return e && atoi(e) != 0;
}
inline long env_int(const char* name, long dflt) {
  const char* e = getenv(name);
  return e ? atol(e) : dflt;
}

struct StageTimer {
  std::string name;
  double alg_bytes = 0;
  std::vector<std::pair<hipEvent_t, hipEvent_t>> pending;
  std::vector<std::pair<hipEvent_t, hipEvent_t>> pool;
  double total_ms = 0;
  int64_t calls = 0;
};

struct Chunk {
  int64_t len, start;
};

struct GraphEntry {            // a captured transform: same direction, buffers and dealias mode
  bool forward;
  const void* in;
  void* out;
  int dealias;
  hipGraphExec_t exec;
};

struct Sched {                 // one all-to-all-v inside a group, bytes
  std::vector<int> peers;
  std::vector<size_t> sc, sd, rc, rd;
  std::vector<int> part;       // pencils: group id of EVERY rank for this exchange (all groups exchange at once); empty: none
};

struct Buf {                   // a device buffer of the plan that only grows (mfft_plan_s::ensure)
  bool arena;                  // from the communicator (work buffers are what exchanges send from) / plain device memory
  bool in_graphs;              // captured sequences hold its address: growing it drops them
  void* p = nullptr;
  size_t bytes = 0;
};

// host-only part of plan construction: decomposition bookkeeping (no HIP call; plan_sched.hip)
int decomp_init(mfft_plan_s* p, const mfft_plan_desc* desc, int nranks, int rank);

}  // namespace mfft

struct mfft_plan_s {
  using Chunk = mfft::Chunk;
  using Sched = mfft::Sched;
  using Buf = mfft::Buf;
  using RowSpec = mfft::RowSpec;
  using ColArgs = mfft::ColArgs;
  using Op = mfft::Op;
  using RealArgs = mfft::RealArgs;
  using RowArgs = mfft::RowArgs;

  mfft_comm_s* comm = nullptr;
  mfft_plan_desc d;
  int P = 1, rank = 0, dev = 0;
  hipStream_t stream = nullptr;
  int prec = MFFT_DOUBLE;
  bool r2c = true;
  int64_t N0 = 0, N1 = 0, N2 = 0, Nf = 0;
  size_t es = 16, rs = 8;       // bytes per complex / per "real-space" element
  // slab
  int64_t Np0 = 0, Np1 = 0;
  // pencil
  int P1 = 1, P2 = 1, c0 = 0, c1 = 0;
  int64_t N1_0 = 0, N1_1 = 0, N2_0 = 0, N2_1 = 0;   // N0/P1, N1/P1, N0/P2, N1/P2
  std::vector<int> group0, group1, world;
  std::vector<Chunk> zc;        // z chunks of the first exchange
  int64_t q = 0, zstart = 0;    // my z extent in spectral space
  // 3/2-rule
  int64_t M0 = 0, M1 = 0, M2 = 0, Mf = 0;
  // Buffers.  From the communicator: the work buffers, work3 (y output of the pipelined inverse; P > 1 only, and captured
  // graphs are P == 1 only, so it never dropped them and still does not) and nlw (several ranks: the six x-pass outputs /
  // exchange buffers of the nonlinear route).  Plain device memory: nlx (fused nonlinear route: the six spectra after their
  // inverse x pass, (L0, N1, Za) each), nly (a batch of their x planes after the inverse y pass, (mb, L1, Za) each), nlr
  // (composed route: nine real-space work arrays), pcomp (compact copy for the plans that do not run on pitched rows natively),
  // shl (mfft_ew_shell_sums: the workgroups' histograms and the result; no captured sequence holds it), nlm (the partial maxima
  // of a statistics call, absmax.hip: fold scratch, then the waves' slots) and nlmacc (twelve doubles that never move: the six
  // maxima of the last statistics call, the result of mfft_ew_absmax); no captured sequence holds them either.
  Buf work[3] = {{true, true}, {true, true}, {true, true}}, work3{true, false}, nlw[2] = {{true, true}, {true, true}};
  Buf nlx{false, true}, nly{false, true}, nlr{false, true}, pcomp{false, true}, shl{false, false}, nlm{false, false}, nlmacc{false, false};
  // mfft_real_moments / mfft_ew_moments (moments.hip): 36 statistics in slot order, then the six centres; the partials go to nlm
  Buf nlsacc{false, false};
  // mfft_real_histogram / mfft_ew_histogram (hist.hip): 6 x (NLH_MAXBINS + 3) int64 counts in slot order, rows nbins + 3 apart,
  // cleared on the stream when a call starts; the workgroups' partial histograms go to nlm.
  Buf nlhacc{false, false};
  // mfft_real_joint_histogram / mfft_ew_joint_histogram (joint.hip): 3 x (MFFT_JOINT_MAXBINS + 3)^2 int64 counts, pairs cells apart,
  // cleared on the stream when a call starts; the workgroups' partial grids go to nlm.
  // nlr2: the SECOND real work array of the composed route (a_p in nlr, b_p here: two is the minimum for a pair).
  Buf nljacc{false, false};
  Buf nlr2{false, false};
  // mfft_real_quadratic / mfft_ew_quadratic (quad.hip): the statistics of q in slot 0 of nlsacc, its counts in the first nbins + 3
  // of nlhacc, the partials in nlm; nlq is the ONE array of doubles the composed route adds the fields' terms into.
  Buf nlq{false, false};
  // mfft_real_increments / mfft_ew_increments (incr.hip): the sums in slot order, [slot][MFFT_INCR_MAXSEP][S2, S3, S4]; the partials
  // go to nlm.
  Buf nliacc{false, false};
  // mfft_real_increment_histogram / mfft_ew_increment_histogram (incrhist.hip): 6 x MFFT_INCR_MAXSEP x (MFFT_INCR_HIST_MAXBINS + 3) int64
  // counts in slot order, [slot][separation][nbins + 3] packed by the call's nsep and nbins, cleared on the stream when a call starts;
  // the workgroups' partial histograms go to nlm.
  Buf nlkacc{false, false};
  // mfft_real_profiles / mfft_ew_profiles (profiles.hip): (npairs, 5, M) doubles, pairs in slot order, zeroed on the stream when a call
  // starts; the partial profiles go to nlm -- one per row slot of the launch, (npairs, 5, M) doubles each, which the plan keeps as it
  // keeps the joint grids.
  Buf nlpacc{false, false};
  // The parameters of the reduction call that is running, in slot order (centres, ranges, weights, separations: whichever its kind
  // has), parked by its *_begin for the batches of the fused routes and the sweeps of the composed one.
  mfft::NlrCall nlcall;
  bool nlm_valid = false;       // a statistics call has run: nlmacc[0..5] hold max |ifftn(a_f)|, max |ifftn(b_f)| of this rank
  uint8_t* mask = nullptr;
  size_t mask_count = 0;
  bool timing = false;
  std::vector<mfft::StageTimer> timers;
  bool use_graphs = false;      // single rank, small mesh: replay captured hipGraphs
  std::vector<mfft::GraphEntry> graphs;
  // exchange pipeline (slab, P > 1): kz slices, a communication stream and events
  int nslice = 1;
  int nbatch = 1;               // pencils: batches of rows pipelined through the exchanges (X: both together, Y: one after the other)
  std::vector<hipEvent_t> ev2_compute, ev2_comm;
  hipStream_t cstream = nullptr;
  int comm_cus = 0;             // CUs reserved for the communication stream (0: no CU masks)
  std::vector<hipEvent_t> ev_compute, ev_comm;
  std::vector<Chunk> kslice;    // (len, start) of each kz slice

  ~mfft_plan_s();               // a plan that never allocated (the host-only entry points) touches neither HIP nor a communicator

  int walloc(void** p, size_t bytes) { return comm ? comm->work_alloc(p, bytes) : mfft::dev_alloc(p, bytes); }
  int wfree(void* p) { return comm ? comm->work_free(p) : mfft::dev_free(p); }
  void drop_graphs();
  int ensure(Buf& b, size_t bytes);

  // ---- stage timers (plan_create.hip) -----------------------------------------
  mfft::StageTimer* timer(const char* name, double alg_bytes);
  int collect_timing();

  template <class F>
  int stage(const char* name, double alg_bytes, F f) { return stage_on(stream, name, alg_bytes, f); }

  template <class F>
  int stage_on(hipStream_t stream, const char* name, double alg_bytes, F f) {
    if (!timing) return f();
    // NOTE: pointers into `timers` are not kept across calls (vector may grow)
    mfft::StageTimer* t = timer(name, alg_bytes);
    std::pair<hipEvent_t, hipEvent_t> ev;
    if (!t->pool.empty()) {
      ev = t->pool.back();
      t->pool.pop_back();
    } else {
      MFFT_HIP(hipEventCreate(&ev.first));
      MFFT_HIP(hipEventCreate(&ev.second));
    }
    MFFT_HIP(hipEventRecord(ev.first, stream));
    int rc = f();
    MFFT_HIP(hipEventRecord(ev.second, stream));
    t = timer(name, alg_bytes);
    t->pending.push_back(ev);
    return rc;
  }

  // ---- kernel helpers (all on this->stream) -----------------------------------
  RealArgs real_args(const void* in, void* out, int64_t nrows, int64_t n, int64_t in_stride, int64_t out_stride, double scale,
                     int valid = 0) const {
    RealArgs a;
    a.in = in; a.out = out; a.n = (int)n; a.prec = prec; a.in_stride = in_stride; a.out_stride = out_stride;
    a.nrows = nrows; a.scale = scale; a.valid = valid;
    return a;
  }
  RowArgs row_args(const void* in, void* out, int64_t nrows, int64_t n, int64_t in_stride, int64_t out_stride, bool inv,
                   double scale) const {
    RowArgs a;
    a.in = in; a.out = out; a.n = (int)n; a.prec = prec; a.inverse = inv; a.in_stride = in_stride;
    a.out_stride = out_stride; a.nrows = nrows; a.scale = scale;
    return a;
  }
  int r2c_rows(const void* in, void* out, int64_t nrows, int64_t n, int64_t in_stride, int64_t out_stride, double scale = 1.0,
               int valid = 0) {
    return mfft::launch_r2c(real_args(in, out, nrows, n, in_stride, out_stride, scale, valid), stream);
  }
  int c2r_rows(const void* in, void* out, int64_t nrows, int64_t n, int64_t in_stride, int64_t out_stride, double scale,
               int valid = 0) {
    return mfft::launch_c2r(real_args(in, out, nrows, n, in_stride, out_stride, scale, valid), stream);
  }
  int c2c_rows(const void* in, void* out, int64_t nrows, int64_t n, int64_t in_stride, int64_t out_stride, bool inv, double scale) {
    return mfft::launch_row(row_args(in, out, nrows, n, in_stride, out_stride, inv, scale), stream);
  }
  // z-axis stage of the forward / backward transform (real or complex flavour)
  int z_forward(const void* in, void* out, int64_t nrows, int64_t nz, int64_t nzf) {
    if (r2c) return r2c_rows(in, out, nrows, nz, nz, nzf);
    return c2c_rows(in, out, nrows, nz, nz, nzf, false, 1.0);
  }
  int z_backward(const void* in, void* out, int64_t nrows, int64_t nz, int64_t nzf) {
    if (r2c) return c2r_rows(in, out, nrows, nz, nzf, nz, 1.0 / (double)nz);
    return c2c_rows(in, out, nrows, nz, nzf, nz, true, 1.0 / (double)nz);
  }
  // z stage with the z-chunk pack / unpack of the pencils fused in (fft_kernels.h, ZSplit): rows [row0, row0 + nrows)
  // of the Pz blocks (rows_total, len_l) that the z-splitting exchange sends / has received
  bool zfuse = false;
  bool xpad_on = true;          // xplane_pad(): MFFT_NO_XPAD=1 clears it (A/B runs; must be the same on every rank)
  bool zpitch_on = true;        // zrow_pitch(): MFFT_NO_ZPITCH=1 clears it (likewise)
  int pad_align = -1;           // pad_pitch(): MFFT_PAD_ALIGN = 0 never, 1 always, unset: where it was measured to pay
  int pad_align_inv = 1;        // inverse flavour of that route (MFFT_PAD_ALIGN_INV = 1 | 2 | 3, see slab_backward_padded_fused)
  bool xpass_inplace = false;   // MFFT_XPASS_INPLACE=1: the x pass behind an exchange runs in place on the receive buffer (rounds 1 - 3)
  int p1_xpad_lines = MFFT_P1_XPAD_DEFAULT;     // p1_plane_pad(): MFFT_P1_XPAD, read when the plan is created
  int64_t zsend_elems(int64_t rows) const {      // elements of the forward z exchange's send blocks for `rows` rows
    int64_t t = 0;
    for (const Chunk& c : zc) t += rows * zrow_pitch(c.len, true);
    return t;
  }
  mfft::ZSplitArgs zsplit(int64_t rows_total, int64_t row0, bool forward = false) const {
    mfft::ZSplitArgs z;
    z.nchunk = (int)zc.size(); z.q = zc[0].len; z.last_len = zc.back().len; z.rows_total = rows_total; z.row0 = row0;
    z.pitch = zrow_pitch(z.q, forward); z.last_pitch = zrow_pitch(z.last_len, forward);
    return z;
  }
  int z_forward_chunked(const void* in, void* blocks, int64_t nrows, int64_t row0, int64_t rows_total) {
    if (r2c) {
      RealArgs a = real_args(in, blocks, nrows, N2, N2, Nf, 1.0);
      a.zs = zsplit(rows_total, row0, true);
      return mfft::launch_r2c(a, stream);
    }
    RowArgs a = row_args(in, blocks, nrows, N2, N2, Nf, false, 1.0);
    a.zs = zsplit(rows_total, row0, true);
    return mfft::launch_row(a, stream);
  }
  int z_backward_chunked(const void* blocks, void* out, int64_t nrows, int64_t row0, int64_t rows_total) {
    if (r2c) {
      RealArgs a = real_args(blocks, out, nrows, N2, Nf, N2, 1.0 / (double)N2);
      a.zs = zsplit(rows_total, row0);
      return mfft::launch_c2r(a, stream);
    }
    RowArgs a = row_args(blocks, out, nrows, N2, Nf, N2, true, 1.0 / (double)N2);
    a.zs = zsplit(rows_total, row0);
    return mfft::launch_row(a, stream);
  }
  // the fields every strided pass fills; col, col_band and col_pad add what is theirs
  ColArgs col_args(const void* in, void* out, int64_t n, bool inv, int64_t nouter, int64_t ncols, int64_t in_outer, RowSpec in_rows,
                   int64_t out_outer, RowSpec out_rows, double scale) const {
    ColArgs a;
    a.in = in; a.out = out; a.n = (int)n; a.prec = prec; a.inverse = inv; a.nouter = nouter; a.ncols = ncols;
    a.in_outer = in_outer; a.out_outer = out_outer; a.in_rows = in_rows; a.out_rows = out_rows;
    a.scale = scale;
    return a;
  }
  int col(const void* in, void* out, int64_t n, bool inv, int64_t nouter, int64_t ncols, int64_t in_outer, RowSpec in_rows,
          int64_t out_outer, RowSpec out_rows, double scale = 0.0) {
    ColArgs a = col_args(in, out, n, inv, nouter, ncols, in_outer, in_rows, out_outer, out_rows,
                         scale != 0.0 ? scale : (inv ? 1.0 / (double)n : 1.0));
    // 2/3-rule (fuse_mask, plan_dealias.hip): a pass that reads the caller's spectrum applies the dealias mask while it loads
    if (mask_src && in >= mask_src && static_cast<const char*>(in) < static_cast<const char*>(mask_src) + (size_t)local_complex_alloc_native() * es) {
      const int64_t off = (static_cast<const char*>(in) - static_cast<const char*>(mask_src)) / (int64_t)es;
      if (lband_use) {           // pencils, the reference's own filter: its three 1-D conditions instead of the bytes
        a.band = local_band(d.decomp == MFFT_PENCIL_Y ? off / (N1 * q) : 0);
        a.scale = scale != 0.0 ? scale : 1.0 / (double)n;
      } else {
        a.mask = mask + off;
      }
    }
    return mfft::launch_col(a, stream);
  }
  int col_band(const void* in, void* out, int64_t n, int64_t nouter, int64_t ncols, int64_t in_outer, RowSpec in_rows,
               int64_t out_outer, RowSpec out_rows, const ColArgs::Band& b) {
    ColArgs a = col_args(in, out, n, true, nouter, ncols, in_outer, in_rows, out_outer, out_rows, 1.0 / (double)n);
    a.band = b;
    a.band.on = true;
    return mfft::launch_col(a, stream);
  }
  int col_pad(const void* in, void* out, int64_t n, bool inv, Op pad, bool fold, int64_t nouter, int64_t ncols,
              int64_t in_outer, RowSpec in_rows, int64_t out_outer, RowSpec out_rows, double scale, int64_t in_wrap = 0,
              int64_t in_wrap_gap = 0, int thirds = -1) {
    ColArgs a = col_args(in, out, n, inv, nouter, ncols, in_outer, in_rows, out_outer, out_rows, scale);
    a.pad = pad; a.fold = fold;
    a.in_wrap = in_wrap; a.in_wrap_gap = in_wrap_gap; a.thirds = thirds;
    return mfft::launch_col(a, stream);
  }
  static RowSpec plain(int64_t stride) { RowSpec r; r.lo = stride; r.hi = 0; r.split = 0; return r; }
  static RowSpec two_level(int64_t split, int64_t hi, int64_t lo) { RowSpec r; r.split = split; r.hi = hi; r.lo = lo; return r; }
  int box(const void* src, void* dst, int64_t e0, int64_t e1, int64_t e2, int64_t s0, int64_t s1, int64_t d0, int64_t d1,
          int mode = 0, double scale = 1.0) {
    mfft::BoxArgs b;
    b.src = src; b.dst = dst; b.e0 = e0; b.e1 = e1; b.e2 = e2; b.s0 = s0; b.s1 = s1; b.d0 = d0; b.d1 = d1;
    b.elem = (int)es; b.mode = mode; b.scale = scale; b.prec = prec;
    return mfft::launch_box_copy(b, stream);
  }
  int zero(void* p, size_t bytes) {
    MFFT_HIP(hipMemsetAsync(p, 0, bytes, stream));
    return 0;
  }

  // ---- layout rules (plan_sched.hip: each with the measurements behind it) -----
  int64_t zrow_pitch(int64_t len, bool forward) const;
  int64_t plane_pad(int64_t stride_elems) const;
  int64_t p1_plane_pad() const;
  int64_t slow_pitch_pad(int64_t stride_elems) const;
  int64_t xplane_pad(bool forward) const;
  int64_t slice_pitch(int s, bool forward) const;
  size_t slice_offset(int s, bool forward) const;

  // ---- exchanges -----------------------------------------------------------------
  int exchange(const std::vector<int>& grp, const void* send, const std::vector<size_t>& sc, const std::vector<size_t>& sd,
               void* recv, const std::vector<size_t>& rc, const std::vector<size_t>& rd, hipStream_t on = nullptr) {
    return comm->alltoallv(send, sc.data(), sd.data(), recv, rc.data(), rd.data(), grp.data(), (int)grp.size(),
                           on ? on : stream, on && on != stream ? 1 : 0);
  }
  int exchange_equal(const std::vector<int>& grp, const void* send, void* recv, size_t chunk_bytes, hipStream_t on = nullptr) {
    const int n = (int)grp.size();
    std::vector<size_t> c(n, chunk_bytes), dsp(n);
    for (int i = 0; i < n; ++i) dsp[i] = (size_t)i * chunk_bytes;
    return exchange(grp, send, c, dsp, recv, c, dsp, on);
  }
  int sched(int which, bool forward, bool padded, Sched* out) const;
  int run_sched(const Sched& sc, const void* send, void* recv, hipStream_t on = nullptr) {
    return comm->alltoallv_part(send, sc.sc.data(), sc.sd.data(), recv, sc.rc.data(), sc.rd.data(), sc.peers.data(),
                                (int)sc.peers.size(), on ? on : stream, on && on != stream ? 1 : 0,
                                sc.part.empty() ? nullptr : sc.part.data());
  }
  // group id of every rank for the exchange inside comm0 (consecutive ranks: same rank / P1) or comm1 (same rank % P1)
  void fill_part(bool comm0, std::vector<int>* part) const {
    part->resize(P);
    for (int r = 0; r < P; ++r) (*part)[r] = comm0 ? r / P1 : r % P1;
  }
  int xchg(int which, bool forward, bool padded, const void* send, void* recv) {
    Sched sc;
    MFFT_TRY(sched(which, forward, padded, &sc));
    return run_sched(sc, send, recv);
  }
  int sched_rows(int which, bool forward, int64_t i0, int64_t mb, Sched* out) const;
  // exchange pipelines: the communication stream waits for what the compute stream has enqueued so far ...
  int comm_waits(hipEvent_t e) {
    MFFT_HIP(hipEventRecord(e, stream));
    MFFT_HIP(hipStreamWaitEvent(cstream, e, 0));
    return 0;
  }
  // ... and runs piece `piece` of exchange `which` (piece_sched), `done` recorded behind it
  int exchange_piece(const char* name, int which, bool forward, int piece, const void* send, void* recv, hipEvent_t done) {
    MFFT_TRY(stage_on(cstream, name, 0, [&] {
      Sched sc;
      MFFT_TRY(piece_sched(which, forward, piece, &sc));
      return run_sched(sc, send, recv, cstream);
    }));
    MFFT_HIP(hipEventRecord(done, cstream));
    return 0;
  }
  // pieces of the pipelined exchanges (host only; the executors and mfft_plan_exchange_pieces share it)
  int npieces() const { return nbatch > 1 ? nbatch : nslice > 1 ? nslice : 1; }
  int piece_sched(int which, bool forward, int piece, Sched* out) const;

  // ---- slab (plan_slab.hip) ------------------------------------------------------
  bool fwd_out_of_place(size_t cbytes);
  // one rank, real data: real / complex split at the SPECTRUM end of the transform (slab_forward_split_last)
  int split_last = -1;          // MFFT_SPLIT_LAST, read when the plan is created: 0 never, 1 wherever the kernels exist, unset: by rule
  int split_last_fit = -1;      // the work buffer fits: decided at the first call
  int64_t split_last_pad() const { return plane_pad(N1 * (N2 / 2)); }
  // The work array W of that route, logical shape (N0, N1, M = N2 / 2), may be blocked in y: element (x, y, m) lies at
  // (y / B) * SB + x * SR + (y % B) * M + m.  B = N1 is the plain array (SR = its plane pitch), B = 1 the transposed one.
  int split_last_yblock = -1;   // MFFT_SPLIT_LAST_YBLOCK, read when the plan is created: B; unset or not a divisor of N1: by rule
  int split_last_yfirst = -1;   // MFFT_SPLIT_LAST_YFIRST: 1 = y, x, z forward and z, x, y inverse with both x passes in place on W,
                                // 0 = x first (forward x and inverse x carry the caller's arrays), 2 = forward as 1, inverse as 0;
                                // unset: by rule
  int64_t split_last_pad_bytes = -1;   // MFFT_SPLIT_LAST_PAD: bytes added to B * M for SR (whole cache lines); unset: by rule
  struct SplitLastLayout {
    int64_t B, SR, SB, nblk;    // rows per block, elements from x row to x row of a block and from block to block, N1 / B
    int yfirst;                 // 0, 1, 2 as split_last_yfirst
    bool yfirst_fwd() const { return yfirst > 0; }
    bool yfirst_bwd() const { return yfirst == 1; }
    int64_t elems() const { return nblk * SB; }
  };
  SplitLastLayout split_last_layout() const;
  bool split_last_eligible() const;
  bool split_last_route();
  // Route "x near" (plan_slab.hip): a second work array W_T, the transposed layout (B = 1: element (x, y, m) at y * SB + x * SR + m),
  // so that the x pass reads or writes rows 8 KiB apart.  Forward: y u -> W, x W -> W_T out of place, z W_T -> fu; inverse: z fu -> W_T,
  // x in place on W_T, y W_T -> u.
  int split_last_xnear = -1;    // MFFT_SPLIT_LAST_XNEAR, read when the plan is created: 0 off, 1 both directions, 2 forward only,
                                // 3 inverse only; unset: by rule
  int split_last_xnear_fit = -1;       // both arrays fit: decided with split_last_fit
  int64_t split_last_xnear_pad_bytes = -1;   // MFFT_SPLIT_LAST_XNEAR_PAD: bytes added to N0 * SR for W_T's SB (whole cache lines); unset: by rule
  int split_last_pairblock = -1;       // MFFT_SPLIT_LAST_PAIRBLOCK: G of fft_kernels.h pair_slot for the z passes of the route; unset: by rule
  int split_last_pairxfast = -1;       // MFFT_SPLIT_LAST_PAIRXFAST: kx fastest inside a tile in the forward (1), the inverse (2) or both (3) z passes; unset: by rule
  SplitLastLayout split_last_layout_t() const;
  int split_last_xnear_mode();         // what runs: 0 ... 3 as above
  int split_last_pair_tile(bool xnear) const;
  bool split_last_pair_xfast(bool xnear, bool inv) const;
  int split_last_x(const SplitLastLayout& l, const void* user_in, void* user_out, void* W, bool inv);
  int split_last_y(const SplitLastLayout& l, const void* user_in, void* user_out, void* W, bool inv);
  int split_last_z(const SplitLastLayout& l, const void* in, void* out, bool inv, bool xnear = false);
  int slab_forward_split_last(const void* u, void* fu);
  int slab_backward_split_last(const void* fu, void* u);
  int slab_forward(const void* u, void* fu);
  int slab_backward(const void* fu, void* u, bool masked);
  int slab_backward_pruned(const void* fu, void* u);
  int slab_forward_pipelined(const void* u, void* fu);
  int slab_backward_pipelined(const void* src, void* u, bool pruned = false);
  int slab_forward_rows(const void* u, void* fu);
  int slab_backward_rows(const void* src, void* u, bool pruned = false);

  // ---- pencil (plan_pencil.hip) --------------------------------------------------
  int pack_z(const void* Z, void* S, int64_t rows, int64_t nf, bool unpack);
  int pencil_forward_pipelined_x(const void* u, void* fu);
  int pencil_backward_pipelined_x(const void* src, void* u);
  int pencil_forward_pipelined_y(const void* u, void* fu);
  int pencil_backward_pipelined_y(const void* src, void* u);
  int pencil_forward(const void* u, void* fu);
  int pencil_backward(const void* fu, void* u, bool masked);

  // ---- dealiasing (plan_dealias.hip) ---------------------------------------------
  // 2/3-rule.  The rule's own mask (get_dealias_filter: three 1-D conditions |k| < kmax) recognised when it is set: x and y
  // keep [0, a) and [b, N), z keeps [0, a2).  One GPU, real data: the inverse then never loads the removed rows, skips
  // the tiles of removed columns and reads a2 bins per z row (pruned passes).
  bool band_ok = false;
  bool band_allzero = false;    // P > 1: every ky of this rank is removed (its x pass is a memset)
  int ba0 = 0, bb0 = 0, ba1 = 0, bb1 = 0, ba2 = 0;
  int* band_tiles = nullptr;
  int band_ntiles = 0;
  // Pencils (R2C): the same recognition, LOCAL to the rank and without any change of layout -- the first inverse pass
  // (x for the X alignment, y for Y) runs the band kernel in its "complete output" mode (ColFft PAD == 4, b_gzero = 2)
  // instead of loading one mask byte per element: removed rows are not loaded, removed columns are transformed as zeros.
  bool lband_ok = false;
  int lb_row_lo = 0, lb_row_hi = 0, lb_g_lo = 0, lb_g_hi = 0, lb_c_lim = 0;
  const void* mask_src = nullptr;
  bool lband_use = false;       // this call's first pass takes the band kernel (set by fuse_mask, cleared with mask_src)
  bool prune_enabled() const { return !mfft::env_on("MFFT_NO_PRUNE"); }      // read at every call
  bool mask_set() const { return mask && mask_count == (size_t)local_complex_count(); }
  int require_mask() const {
    if (mask_set()) return 0;
    return mfft::set_error(MFFT_ERR_INVALID, "2/3-rule requested but no dealias mask of %zu entries was set", (size_t)local_complex_count());
  }
  void band_keep(double* keep0, double* keep1, double* keep2) const {       // fractions of kx, ky, kz that the band keeps
    *keep0 = 1.0 - (double)(bb0 - ba0) / (double)N0;
    *keep1 = 1.0 - (double)(bb1 - ba1) / (double)N1;
    *keep2 = (double)ba2 / (double)Nf;
  }
  void detect_band(const uint8_t* m);
  int analyse_band(const uint8_t* m, int* a0, int* b0, int* a1, int* b1, int* a2, std::vector<int>* list) const;
  void detect_band_local(const uint8_t* m);
  // first inverse pass of a pencil plan over rows [g0, g0 + nouter) of the g axis (X: one launch, the g axis is folded
  // into the columns; Y: batches of local kx rows)
  ColArgs::Band local_band(int64_t g0) const {
    ColArgs::Band b;
    b.on = true;
    b.row_lo = lb_row_lo; b.row_hi = lb_row_hi; b.c_lim = lb_c_lim; b.g_lo = lb_g_lo; b.g_hi = lb_g_hi; b.g_zero = 2;
    if (d.decomp == MFFT_PENCIL_X) { b.c_off = 0; b.c_per = (int)q; b.g_off = 0; b.g_step = 0; }
    else                           { b.c_off = 0; b.c_per = 1 << 30; b.g_off = (int)g0; b.g_step = 1; }
    return b;
  }
  int fuse_mask(const void* fu, int64_t first_len, bool* fused);
  int apply_mask_copy(const void* fu, void** masked_out);
  // 3/2-rule
  bool zfuse_pad() const;
  int64_t pad_pitch() const;
  int pad_axis(const void* src, void* dst, int64_t a0, int64_t n, int64_t npad, int64_t a2, double scale);
  int trunc_axis(const void* src, void* dst, int64_t a0, int64_t n, int64_t npad, int64_t a2, int64_t a2s, double scale,
                 bool fold = true);
  // normalisation: padsize per padded axis (slab.py:256, 330; line.py:184, 287 for the 2-D class)
  double padscale() const {
    double v = 1.0;
    for (int64_t n : {N0, N1, N2}) if (n > 1) v *= d.padsize;
    return v;
  }
  bool can_fuse_pad() const;
  int slab_forward_padded(const void* u, void* fu);
  int slab_backward_padded(const void* fu, void* u);
  int slab_forward_padded_fused(const void* u, void* fu);
  int slab_backward_padded_fused(const void* fu, void* u);
  int pencil_forward_padded(const void* u, void* fu);
  int pencil_backward_padded(const void* fu, void* u);
  int pencil_forward_padded_fused(const void* u, void* fu);
  int pencil_backward_padded_fused(const void* fu, void* u);

  // ---- round 6: pitched spectrum (mfft_plan_desc::complex_pitch) ----
  // The caller's complex array keeps its logical shape but its z rows lie Zp >= Nf elements apart (whole cache lines:
  // 513 -> 520 bins in double precision), so that every strided pass and both real transforms meet line-aligned rows.
  // One-rank slab R2C plans run on such arrays natively (nat_pitch); every other plan converts at the boundary through a
  // compact copy of its own (correct everywhere, fast where it was asked for).
  int64_t Zp = 0;               // row pitch of the caller's spectrum in complex elements; 0: compact rows of Nf
  bool conv_now = false;        // exec(): this call runs on the compact copy (a route without a pitched flavour)
  bool pitched() const { return Zp > 0; }
  bool nat_pitch() const { return Zp > 0 && !conv_now && d.decomp == MFFT_SLAB && P == 1 && r2c && !d.line2d && !d.drop_nyquist; }
  int64_t Zc() const { return nat_pitch() ? Zp : Nf; }          // row pitch the one-rank slab routes run with
  void cdims(int64_t* d0, int64_t* d1, int64_t* d2) const {     // local complex extents
    if (d.decomp == MFFT_SLAB) { *d0 = N0; *d1 = Np1; *d2 = Nf; }
    else if (d.decomp == MFFT_PENCIL_X) { *d0 = N0; *d1 = N1_1; *d2 = q; }
    else { *d0 = N2_0; *d1 = N1; *d2 = q; }
  }
  int64_t local_complex_count() const {
    int64_t a, b, c;
    cdims(&a, &b, &c);
    return a * b * c;
  }
  int64_t local_complex_alloc_native() const { return nat_pitch() ? N0 * Np1 * Zp : local_complex_count(); }   // what the routes see
  int64_t local_complex_alloc() const {                          // elements of the caller's (possibly pitched) spectrum
    int64_t a, b, c;
    cdims(&a, &b, &c);
    return a * b * (pitched() ? Zp : c);
  }
  int repitch(const void* src, void* dst, bool to_pitched) {     // compact <-> pitched copy of one local spectrum
    int64_t a, b, c;
    cdims(&a, &b, &c);
    return to_pitched ? box(src, dst, a, b, c, b * c, c, b * Zp, Zp) : box(src, dst, a, b, c, b * Zp, Zp, b * c, c);
  }
  int exec(bool forward, const void* in, void* out, int dealias);       // one transform, pitched callers' arrays converted where needed

  // ---- round 6: the nonlinear term a x b of a pseudo-spectral step as one operation (fft_nlz.h; plan_nonlinear.hip) ----
  // (product: one of mfft::NL_PRODUCTS -- the cross product, three result components; the dot product, one; both at once with a
  // third field, four)
  // (stats: also the six real-space maxima, into nlmacc -- the Build::AbsMax z kernel on the fused routes, a sweep over the
  // real work arrays on the composed one)
  bool nonlinear_fusable(int dealias, mfft::Op product = mfft::Op::Plain, bool stats = false) const;
  int64_t local_real_count(bool padded) const;
  int nonlinear(const mfft::NlFields& u, int dealias, mfft::Op product, bool stats);
  int nonlinear_fused(const mfft::NlFields& u, int dealias, mfft::Op product, bool stats);
  int nonlinear_fused_ranks(const mfft::NlFields& u, int dealias, mfft::Op product, bool stats);
  int nonlinear_composed(const mfft::NlFields& u, int dealias, mfft::Op product, bool stats);
  int nonlinear_absmax(double out6[6]);                                   // this rank's maxima of the last statistics call
  int absmax_sweep(const void* x, int ncomp, size_t n, double* acc);      // absmax.hip
  // The reductions (mfft::NL_PRODUCTS with nout == 0): statistics of ifftn(field, dealias) of up to six fields given as spectra, over
  // this rank's part of the grid a product would be formed on.  ONE route (plan_nonlinear.hip): real_reduce is a call from its
  // begin to its end -- the fused routes above with the z stage that ends in the kind's reduction, or reduce_composed, inverse
  // transforms into a real work array and the kind's sweep; reduce_batch is that z stage on a batch of the fused routes.
  template <class Begin, class End>
  int real_reduce(const mfft::NlFields& u, int dealias, mfft::Op kind, int64_t* count, Begin begin, End end);
  int reduce_composed(const mfft::NlFields& u, int dealias, mfft::Op kind);
  int reduce_batch(mfft::Op kind, const mfft::NlFields& u, char* Y, size_t yelems, int64_t L2, int64_t Za, int64_t nrows, int valid_in);
  // What a kind supplies: its entry, begin / end around its accumulator, and its sweep (moments.hip, hist.hip, joint.hip, quad.hip,
  // incr.hip, incrhist.hip).  [min, max, S1 .. S4] per field:
  int real_moments(const mfft::NlFields& u, int dealias, const double* center, double* out, int64_t* count);
  int moments_sweep(const void* x, int ncomp, size_t n, const double* center, double* acc);
  int moments_begin(const double center_slots[6]);
  int moments_end(double host[36]);
  // histograms, out: (nfields, nbins + 3)
  int real_histogram(const mfft::NlFields& u, int dealias, const double* lo, const double* hi, int nbins, int64_t* out, int64_t* count);
  int hist_sweep(const void* x, int ncomp, size_t n, const double* lo, const double* inv, int nbins, int64_t* acc);
  int hist_begin(const double lo_slots[6], const double inv_slots[6], int nbins);
  int hist_end(int64_t* host, int nslots);
  // joint histograms of one or three pairs, out: (npairs, nba + 3, nbb + 3).  lo, hi: 2 ncomp entries, a_0.., then b_0..
  int real_joint_histogram(const mfft::NlFields& u, int dealias, const double* lo, const double* hi, int nba, int nbb, int64_t* out, int64_t* count);
  int joint_sweep(const void* x, const void* y, size_t n, const double lo[2], const double inv[2], int nba, int nbb, int64_t* acc);
  int joint_begin(const double lo_slots[6], const double inv_slots[6], int nba, int nbb);
  int joint_end(int64_t* host, int npairs);
  // q = sum_f w_f ifftn(field f)^2 (composed: each field's term added into nlq, one sweep of nlq).  out6: [min, max, S1 .. S4];
  // counts: nbins + 3, may be null if nbins == 0
  int real_quadratic(const mfft::NlFields& u, int dealias, const double* weights, double center, double lo, double hi, int nbins, double* out6,
                     int64_t* counts, int64_t* count);
  int quad_begin(double center, double lo, double inv, int nbins);
  int quad_end(double out6[6], int64_t* counts);
  int quad_sweep(const void* x, bool as_double, int ncomp, size_t stride, size_t n, const double* w, bool square);
  int quad_accum(const void* r, double* q, size_t n, double w, bool first);
  // structure functions along z, out[(f * nsep + i) * 3 + {0, 1, 2}] = S2, S3, S4
  int real_increments(const mfft::NlFields& u, int dealias, const int64_t* seps, int nsep, double* out, int64_t* count);
  int incr_sweep(const void* x, int ncomp, int64_t nrows, int64_t n, int64_t pitch, double* acc);
  int incr_begin(const int64_t* seps, int nsep);
  int incr_end(double* host);
  // increment PDFs along z, out: (nfields, nsep, nbins + 3).  lo, hi: [f * nsep + i]
  int real_increment_histogram(const mfft::NlFields& u, int dealias, const int64_t* seps, int nsep, const double* lo, const double* hi, int nbins,
                               int64_t* out, int64_t* count);
  int incr_hist_sweep(const void* x, int ncomp, int64_t nrows, int64_t n, int64_t pitch, int slot0, int64_t* acc);
  int incr_hist_begin(const int64_t* seps, int nsep, const double (*lo_slots)[MFFT_INCR_MAXSEP], const double (*inv_slots)[MFFT_INCR_MAXSEP], int nbins);
  int incr_hist_end(int64_t* host, int nslots);
  // profiles along z of one or three pairs, out: (npairs, 5, M).  center: 2 ncomp entries, a_0.., then b_0.. (null: zeros)
  int real_profiles(const mfft::NlFields& u, int dealias, const double* center, double* out, int64_t* count);
  int prof_sweep(const void* x, const void* y, int ncomp, int64_t nrows, int64_t n, const double* center, double* acc);
  int prof_begin(const double center_slots[6], int npairs, int64_t n);
  int prof_end(double* host, int npairs, int64_t n);
};

namespace mfft {
struct MaskScope {             // the dealias mask handed to col() belongs to one call only
  mfft_plan_s* p;
  ~MaskScope() { p->mask_src = nullptr; p->lband_use = false; }
};
}  // namespace mfft
