// plan_create.hip -- how a plan is made and entered: creation and destruction, buffers, stage timers, layout and
// workspace queries, the dispatch of a transform to its route, hipGraph replay and the C entry points around them.
#include "plan_impl.h"

using namespace mfft;

#ifndef MFFT_DEFAULT_COMM_CUS
#define MFFT_DEFAULT_COMM_CUS 0
#endif

mfft_plan_s::~mfft_plan_s() {
  for (Buf* b : {&work[0], &work[1], &work[2], &work3, &nlw[0], &nlw[1], &nlx, &nly, &nlr, &pcomp, &shl, &nlm, &nlmacc, &nlsacc, &nlhacc, &nlq, &nliacc, &nljacc, &nlr2, &nlpacc, &nlkacc})
    if (b->p) (void)(b->arena ? wfree(b->p) : dev_free(b->p));
  if (mask) (void)hipFree(mask);
  if (band_tiles) (void)hipFree(band_tiles);
  for (auto& t : timers) {
    for (auto& e : t.pending) { (void)hipEventDestroy(e.first); (void)hipEventDestroy(e.second); }
    for (auto& e : t.pool) { (void)hipEventDestroy(e.first); (void)hipEventDestroy(e.second); }
  }
  drop_graphs();
  for (hipEvent_t e : ev_compute) (void)hipEventDestroy(e);
  for (hipEvent_t e : ev_comm) (void)hipEventDestroy(e);
  for (hipEvent_t e : ev2_compute) (void)hipEventDestroy(e);
  for (hipEvent_t e : ev2_comm) (void)hipEventDestroy(e);
  if (cstream) { big_release_stream(cstream); (void)hipStreamDestroy(cstream); }
  if (stream) { big_release_stream(stream); (void)hipStreamDestroy(stream); }
}

void mfft_plan_s::drop_graphs() {
  for (auto& g : graphs)
    if (g.exec) (void)hipGraphExecDestroy(g.exec);
  graphs.clear();
}

// Every size asked for is a product of positive extents, so "large enough" alone decides (a buffer that does not exist has
// 0 bytes).  Which allocator a buffer comes from and whether growing it drops the captured graphs are the buffer's own.
int mfft_plan_s::ensure(Buf& b, size_t bytes) {
  if (b.bytes >= bytes) return 0;
  if (b.in_graphs) drop_graphs();           // captured sequences hold the old buffer address
  if (b.p) MFFT_TRY(b.arena ? wfree(b.p) : dev_free(b.p));
  b.p = nullptr;
  b.bytes = 0;
  MFFT_TRY(b.arena ? walloc(&b.p, bytes) : dev_alloc(&b.p, bytes));
  b.bytes = bytes;
  return 0;
}

StageTimer* mfft_plan_s::timer(const char* name, double alg_bytes) {
  for (auto& t : timers)
    if (t.name == name) return &t;
  timers.emplace_back();
  timers.back().name = name;
  timers.back().alg_bytes = alg_bytes;
  return &timers.back();
}

int mfft_plan_s::collect_timing() {
  for (auto& t : timers) {
    for (auto& e : t.pending) {
      MFFT_HIP(hipEventSynchronize(e.second));
      float ms = 0;
      MFFT_HIP(hipEventElapsedTime(&ms, e.first, e.second));
      t.total_ms += ms;
      t.calls += 1;
      t.pool.push_back(e);
    }
    t.pending.clear();
  }
  return 0;
}

namespace mfft {
hipStream_t plan_stream(mfft_plan_t plan) { return plan ? plan->stream : nullptr; }
}  // namespace mfft

// ===========================================================================
// C ABI
// ===========================================================================
extern "C" {

int mfft_plan_create(mfft_comm_t comm, const mfft_plan_desc* desc, mfft_plan_t* out) {
  if (!comm || !desc || !out) return set_error(MFFT_ERR_INVALID, "null argument");
  std::unique_ptr<mfft_plan_s> p(new mfft_plan_s());
  p->comm = comm;
  MFFT_TRY(decomp_init(p.get(), desc, comm->size, comm->rank));
  comm->plan_refs++;                       // released by mfft_plan_destroy / the error path below
  struct Unref {
    mfft_comm_s* c; bool armed;
    ~Unref() { if (armed) c->plan_refs--; }
  } unref{comm, true};
  MFFT_HIP(hipGetDevice(&p->dev));
  const int nev = std::max(p->nslice > 1 ? p->nslice : 0, p->nbatch > 1 ? p->nbatch : 0);
  // Pipelined plans: the exchange runs on a stream of its own, and that stream gets CUs of its own.  The transform
  // kernels fill every CU (two 1024-thread workgroups with 80 KB of LDS each), so whatever the exchange launches -- the
  // IPC transport's pull kernel, RCCL's send / recv kernels -- would otherwise wait for transform workgroups to retire
  // and then take a whole CU away from them, workgroup by workgroup.  With comm_cus = K > 0 the communication stream
  // is confined to K CUs and the compute stream to the other ones (hipExtStreamCreateWithCUMask; KFD deals the bits of
  // a mask round-robin over the XCDs, so the last K = 8k bits are k CUs of every XCD); measured in
  // profiles/r03_cu_mask_probe.txt.  desc.comm_cus: 0 = $MFFT_COMM_CUS or the default, < 0 = no masks.
  int comm_cus = desc->comm_cus;
  if (comm_cus == 0) comm_cus = (int)env_int("MFFT_COMM_CUS", MFFT_DEFAULT_COMM_CUS);
  int ncu = 0;
  (void)hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, p->dev);
  auto masked = [&](int lo, int hi, hipStream_t* st) {
    std::vector<uint32_t> m((size_t)(ncu + 31) / 32, 0u);
    for (int i = lo; i < hi; ++i) m[i / 32] |= 1u << (i % 32);
    if (hipExtStreamCreateWithCUMask(st, (uint32_t)m.size(), m.data()) == hipSuccess) return true;
    (void)hipGetLastError();
    *st = nullptr;
    return false;
  };
  if (nev > 0 && comm_cus > 0 && ncu >= 16 && comm_cus <= ncu / 2) {
    if (masked(ncu - comm_cus, ncu, &p->cstream)) {
      if (masked(0, ncu - comm_cus, &p->stream)) {
        p->comm_cus = comm_cus;
      } else {
        (void)hipStreamDestroy(p->cstream);
        p->cstream = nullptr;
      }
    }
  }
  if (!p->stream) MFFT_HIP(hipStreamCreateWithFlags(&p->stream, hipStreamNonBlocking));
  {
    // Opt-in (MFFT_GRAPH=1), single rank only (no host-side rendezvous inside the sequence).  Measured:
    // a transform is only three kernels, and replaying a 3-node graph (~16 us) costs more than three
    // direct launches (64^3: 41.5k pairs/s direct vs 30k replayed); it pays when the caller's own
    // kernels ride on the same stream between transforms (32^3 Taylor-Green step 1.29 -> 1.02 ms).
    p->use_graphs = p->P == 1 && env_on("MFFT_GRAPH");
  }
  if (nev > 0) {
    if (!p->cstream) {
      // no CU masks.  The communication stream is created at the LOWEST priority of the device's range (HIP: least = 1 =
      // low, 0 = normal, greatest = -1 = high; the compute stream is a plain non-blocking stream = normal) -- this is
      // what every round-3 profile was taken with (its notes call it "normal": ADVICE r03), and it is kept because it is
      // the measured configuration.  MFFT_COMM_PRIORITY=0 asks for normal, 1 for the highest priority: measured
      // (profiles/r03_cu_mask_probe.txt) the highest changes nothing for the pull kernel -- workgroups of a second queue
      // are admitted as transform workgroups retire, with or without it -- and with several ranks on ONE device it
      // inverts priorities (a high-priority queue polling for a flag that a lower-priority queue of another process has
      // yet to write: 0.8 -> 45 ms per pair at two processes, profiles/r03_shared_gpu_pipeline_latency.txt).
      int prio_least = 0, prio_greatest = 0;
      MFFT_HIP(hipDeviceGetStreamPriorityRange(&prio_least, &prio_greatest));
      int prio = prio_least;
      if (const char* e = getenv("MFFT_COMM_PRIORITY")) prio = atoi(e) > 0 ? prio_greatest : atoi(e) == 0 ? 0 : prio_least;
      prio = std::max(prio_greatest, std::min(prio_least, prio));
      MFFT_HIP(hipStreamCreateWithPriority(&p->cstream, hipStreamNonBlocking, prio));
    }
    for (std::vector<hipEvent_t>* v : {&p->ev_compute, &p->ev_comm, &p->ev2_compute, &p->ev2_comm}) {
      if ((v == &p->ev2_compute || v == &p->ev2_comm) && p->nbatch <= 1) continue;
      v->resize(nev);
      for (int s = 0; s < nev; ++s) MFFT_HIP(hipEventCreateWithFlags(&(*v)[s], hipEventDisableTiming));
    }
  }
  unref.armed = false;
  *out = p.release();
  return 0;
}

int mfft_plan_destroy(mfft_plan_t plan) {
  if (!plan) return 0;
  (void)hipStreamSynchronize(plan->stream);
  mfft_comm_s* c = plan->comm;
  delete plan;                             // returns its work buffers to the communicator
  if (c && --c->plan_refs == 0 && c->destroy_requested) delete c;
  return 0;
}

static int layout_of(const mfft_plan_s* p, int64_t rshape[3], int64_t cshape[3], int64_t rstart[3], int64_t cstart[3],
                     int64_t rshape_pad[3], int64_t grid[2], int64_t sub[2]) {
  int64_t rs_[3], cs_[3], r0[3], c0_[3], rp[3];
  if (p->d.decomp == MFFT_SLAB) {
    rs_[0] = p->Np0; rs_[1] = p->N1; rs_[2] = p->N2;
    cs_[0] = p->N0; cs_[1] = p->Np1; cs_[2] = p->Nf;
    r0[0] = p->rank * p->Np0; r0[1] = 0; r0[2] = 0;
    c0_[0] = 0; c0_[1] = p->rank * p->Np1; c0_[2] = 0;
    rp[0] = p->M0 / p->P; rp[1] = p->M1; rp[2] = p->M2;
    if (grid) { grid[0] = p->P; grid[1] = 1; }
    if (sub) { sub[0] = p->rank; sub[1] = 0; }
  } else {
    rs_[0] = p->N1_0; rs_[1] = p->N2_1; rs_[2] = p->N2;
    r0[0] = p->c0 * p->N1_0; r0[1] = p->c1 * p->N2_1; r0[2] = 0;
    rp[0] = p->M0 / p->P1; rp[1] = p->M1 / p->P2; rp[2] = p->M2;
    if (p->d.decomp == MFFT_PENCIL_X) {
      cs_[0] = p->N0; cs_[1] = p->N1_1; cs_[2] = p->q;
      c0_[0] = 0; c0_[1] = p->c0 * p->N1_1; c0_[2] = p->zstart;
    } else {
      cs_[0] = p->N2_0; cs_[1] = p->N1; cs_[2] = p->q;
      c0_[0] = p->c1 * p->N2_0; c0_[1] = 0; c0_[2] = p->zstart;
    }
    if (grid) { grid[0] = p->P1; grid[1] = p->P2; }
    if (sub) { sub[0] = p->c0; sub[1] = p->c1; }
  }
  for (int i = 0; i < 3; ++i) {
    if (rshape) rshape[i] = rs_[i];
    if (cshape) cshape[i] = cs_[i];
    if (rstart) rstart[i] = r0[i];
    if (cstart) cstart[i] = c0_[i];
    if (rshape_pad) rshape_pad[i] = rp[i];
  }
  return 0;
}

int mfft_plan_layout(mfft_plan_t p, int64_t rshape[3], int64_t cshape[3], int64_t rstart[3], int64_t cstart[3],
                     int64_t rshape_pad[3], int64_t grid[2], int64_t sub[2]) {
  if (!p) return set_error(MFFT_ERR_INVALID, "null plan");
  return layout_of(p, rshape, cshape, rstart, cstart, rshape_pad, grid, sub);
}

// The same answers for rank `rank` of `nranks` WITHOUT a plan, a communicator or a device: the decomposition
// bookkeeping of the constructors (slab.py:82-96, pencil.py:187-216, 903-913) is host arithmetic.
int mfft_layout_query(const mfft_plan_desc* desc, int nranks, int rank, int64_t rshape[3], int64_t cshape[3],
                      int64_t rstart[3], int64_t cstart[3], int64_t rshape_pad[3], int64_t grid[2], int64_t sub[2]) {
  if (!desc) return set_error(MFFT_ERR_INVALID, "null argument");
  mfft_plan_s p;
  MFFT_TRY(decomp_init(&p, desc, nranks, rank));
  return layout_of(&p, rshape, cshape, rstart, cstart, rshape_pad, grid, sub);
}

// Row pitch (complex elements) and allocation size (elements) of this rank's spectrum under desc->complex_pitch: what a
// caller must allocate -- shape (d0, d1, pitch) physically, (d0, d1, d2) logically.  Device-free.
int mfft_layout_complex_pitch(const mfft_plan_desc* desc, int nranks, int rank, int64_t* pitch, int64_t* alloc_elems) {
  if (!desc || !pitch || !alloc_elems) return set_error(MFFT_ERR_INVALID, "null argument");
  mfft_plan_s p;
  MFFT_TRY(decomp_init(&p, desc, nranks, rank));
  int64_t a, b, c;
  p.cdims(&a, &b, &c);
  *pitch = p.pitched() ? p.Zp : c;
  *alloc_elems = p.local_complex_alloc();
  return 0;
}

int mfft_plan_workspace_bytes(mfft_plan_t p, size_t* bytes) {
  if (!p || !bytes) return set_error(MFFT_ERR_INVALID, "null argument");
  *bytes = p->work[0].bytes + p->work[1].bytes + p->work[2].bytes + p->work3.bytes + p->pcomp.bytes;
  return 0;
}

static int check_ready(mfft_plan_t p, const void* a, const void* b) {
  if (!p || !a || !b) return set_error(MFFT_ERR_INVALID, "null argument");
  int dev = -1;
  MFFT_HIP(hipGetDevice(&dev));
  if (dev != p->dev) MFFT_HIP(hipSetDevice(p->dev));
  return 0;
}

static int run_route(mfft_plan_t p, bool forward, const void* in, void* out, int dealias) {
  const bool pad = dealias == MFFT_DEALIAS_3_2, masked = dealias == MFFT_DEALIAS_2_3;
  if (forward) {
    if (p->d.decomp == MFFT_SLAB) return pad ? p->slab_forward_padded(in, out) : p->slab_forward(in, out);
    return pad ? p->pencil_forward_padded(in, out) : p->pencil_forward(in, out);
  }
  if (p->d.decomp == MFFT_SLAB) return pad ? p->slab_backward_padded(in, out) : p->slab_backward(in, out, masked);
  return pad ? p->pencil_backward_padded(in, out) : p->pencil_backward(in, out, masked);
}

// A pitched spectrum on a plan whose routes want compact rows (several ranks, pencils, complex data): converted at the
// boundary through the plan's compact copy -- one more pass over the spectrum, every decomposition served.
int mfft_plan_s::exec(bool forward, const void* in, void* out, int dealias) {
  // (a one-rank plan whose 3/2-rule route is the copy-based one -- lengths without pad / truncate kernels -- converts too)
  const bool native = nat_pitch() && (dealias != MFFT_DEALIAS_3_2 || can_fuse_pad());
  if (!pitched() || native) return run_route(this, forward, in, out, dealias);
  MFFT_TRY(ensure(pcomp, (size_t)local_complex_count() * es));
  struct Scope {
    mfft_plan_s* p;
    ~Scope() { p->conv_now = false; }
  } scope{this};
  if (forward) {
    conv_now = true;
    MFFT_TRY(run_route(this, true, in, pcomp.p, dealias));
    conv_now = false;
    return stage("fwd_pitch", 0, [&] { return repitch(pcomp.p, out, true); });
  }
  MFFT_TRY(stage("bwd_pitch", 0, [&] { return repitch(in, pcomp.p, false); }));
  conv_now = true;
  return run_route(this, false, pcomp.p, out, dealias);
}

static int run_direct(mfft_plan_t p, bool forward, const void* in, void* out, int dealias) { return p->exec(forward, in, out, dealias); }

// Small single-rank transforms are launch-bound (six ~10 us kernels per pair): the kernel sequence of
// a (direction, in, out, dealias) combination is captured into a hipGraph the second time it is seen
// and replayed afterwards.  The first execution runs directly so that work buffers, twiddle tables
// and function attributes exist before anything is captured.
static int run_graphed(mfft_plan_t p, bool forward, const void* in, void* out, int dealias) {
  for (auto& g : p->graphs)
    if (g.forward == forward && g.in == in && g.out == out && g.dealias == dealias) {
      if (g.exec) {
        MFFT_HIP(hipGraphLaunch(g.exec, p->stream));
        return 0;
      }
      // second sighting: capture
      hipGraph_t graph = nullptr;
      MFFT_HIP(hipStreamBeginCapture(p->stream, hipStreamCaptureModeThreadLocal));
      const int rc = run_direct(p, forward, in, out, dealias);
      const hipError_t e = hipStreamEndCapture(p->stream, &graph);
      if (rc != 0) {
        if (graph) (void)hipGraphDestroy(graph);
        return rc;
      }
      if (e != hipSuccess || !graph) {      // capture not possible: fall back to direct launches for good
        (void)hipGetLastError();
        p->use_graphs = false;
        return run_direct(p, forward, in, out, dealias);
      }
      hipGraphExec_t exec = nullptr;
      const hipError_t ei = hipGraphInstantiate(&exec, graph, nullptr, nullptr, 0);
      (void)hipGraphDestroy(graph);
      if (ei != hipSuccess) {
        (void)hipGetLastError();
        p->use_graphs = false;
        return run_direct(p, forward, in, out, dealias);
      }
      g.exec = exec;
      MFFT_HIP(hipGraphLaunch(g.exec, p->stream));
      return 0;
    }
  if (p->graphs.size() >= 64) {              // bounded cache (callers that cycle through many buffers)
    p->drop_graphs();
  }
  p->graphs.push_back(GraphEntry{forward, in, out, dealias, nullptr});
  return run_direct(p, forward, in, out, dealias);
}

int mfft_forward(mfft_plan_t p, const void* u, void* fu, int dealias) {
  MFFT_TRY(check_ready(p, u, fu));
  if (p->use_graphs && !p->timing) return run_graphed(p, true, u, fu, dealias);
  return run_direct(p, true, u, fu, dealias);
}

int mfft_backward(mfft_plan_t p, const void* fu, void* u, int dealias) {
  MFFT_TRY(check_ready(p, fu, u));
  if (p->use_graphs && !p->timing) return run_graphed(p, false, fu, u, dealias);
  return run_direct(p, false, fu, u, dealias);
}

// The five entries to the nonlinear term: the plan on its device, exactly the pointers the product needs, a known dealias mode.
static int run_nonlinear(mfft_plan_t p, Op product, bool stats, const NlFields& u, int dealias) {
  const NlProduct& q = nl_product(product);
  MFFT_TRY(check_ready(p, u.a, u.b));
  if (!u.out || (q.nin > 6 && !u.c) || (q.nout > u.nres && !u.outs)) return set_error(MFFT_ERR_INVALID, "null argument");
  if (dealias != MFFT_DEALIAS_NONE && dealias != MFFT_DEALIAS_2_3 && dealias != MFFT_DEALIAS_3_2)
    return set_error(MFFT_ERR_INVALID, "unknown dealias mode %d", dealias);
  return p->nonlinear(u, dealias, product, stats);
}

// out = fftn(ifftn(a) x ifftn(b)) with the plan's transforms under the given dealias mode: a, b, out are vector fields of
// shape (3,) + the local complex shape, component-major; out may be a or b.  See include/mpifft4py_amd.h.
int mfft_nonlinear_cross(mfft_plan_t p, const void* a_hat, const void* b_hat, void* out_hat, int dealias) {
  return run_nonlinear(p, Op::Plain, false, {a_hat, b_hat, nullptr, out_hat, nullptr}, dealias);
}

// out = fftn(sum_f ifftn(a_f) ifftn(b_f)): a, b as above, out ONE component (the local complex shape); out may be any one
// component of a or b.  See include/mpifft4py_amd.h.
int mfft_nonlinear_dot(mfft_plan_t p, const void* a_hat, const void* b_hat, void* out_hat, int dealias) {
  return run_nonlinear(p, Op::Dot, false, {a_hat, b_hat, nullptr, out_hat, nullptr}, dealias);
}

// out = fftn(ifftn(a) x ifftn(b)) AND s = fftn(sum_f ifftn(a_f) ifftn(c_f)) in one pass: a, b, c, out vector fields, s ONE
// component; out may be a or b, s any one component of c.  See include/mpifft4py_amd.h.
int mfft_nonlinear_cross_dot(mfft_plan_t p, const void* a_hat, const void* b_hat, const void* c_hat, void* out_hat, void* s_hat, int dealias) {
  return run_nonlinear(p, Op::CrossDot, false, {a_hat, b_hat, c_hat, out_hat, s_hat}, dealias);
}

// out[3 i + j] = fftn(ifftn(a_i) ifftn(b_j)), all nine: a, b vector fields, out NINE components; a may be b (the symmetric tensor,
// all nine computed); out may not overlap an input -- rejected before anything is enqueued.  See include/mpifft4py_amd.h.
int mfft_nonlinear_outer(mfft_plan_t p, const void* a_hat, const void* b_hat, void* out_hat, int dealias) {
  MFFT_TRY(check_ready(p, a_hat, b_hat));
  if (!out_hat) return set_error(MFFT_ERR_INVALID, "null argument");
  const size_t comp = (size_t)p->local_complex_alloc() * p->es;
  const char *o = static_cast<const char*>(out_hat), *ins[2] = {static_cast<const char*>(a_hat), static_cast<const char*>(b_hat)};
  for (const char* i : ins)
    if (o < i + 3 * comp && i < o + 9 * comp) return set_error(MFFT_ERR_INVALID, "nonlinear_outer: out_hat overlaps an input");
  NlFields u{a_hat, b_hat, nullptr, out_hat, nullptr};
  u.nres = 9;
  return run_nonlinear(p, Op::Outer, false, u, dealias);
}

// ... and the first two with statistics: the call also leaves the six real-space maxima in the plan (mfft_plan_nonlinear_absmax)
int mfft_nonlinear_cross_absmax(mfft_plan_t p, const void* a_hat, const void* b_hat, void* out_hat, int dealias) {
  return run_nonlinear(p, Op::Plain, true, {a_hat, b_hat, nullptr, out_hat, nullptr}, dealias);
}
int mfft_nonlinear_dot_absmax(mfft_plan_t p, const void* a_hat, const void* b_hat, void* out_hat, int dealias) {
  return run_nonlinear(p, Op::Dot, true, {a_hat, b_hat, nullptr, out_hat, nullptr}, dealias);
}
int mfft_plan_nonlinear_absmax(mfft_plan_t p, double out6[6]) {
  if (!p || !out6) return set_error(MFFT_ERR_INVALID, "null argument");
  return p->nonlinear_absmax(out6);
}

// The seven reductions: the plan on its device, a (and b, where given) of ncomp components, a known dealias mode -> the call's fields
static int reduce_fields(mfft_plan_t p, const void* a_hat, const void* b_hat, int ncomp, int dealias, NlFields* u) {
  MFFT_TRY(check_ready(p, a_hat, a_hat));
  if (ncomp != 1 && ncomp != 3) return set_error(MFFT_ERR_INVALID, "ncomp must be 1 or 3, not %d", ncomp);
  if (dealias != MFFT_DEALIAS_NONE && dealias != MFFT_DEALIAS_2_3 && dealias != MFFT_DEALIAS_3_2)
    return set_error(MFFT_ERR_INVALID, "unknown dealias mode %d", dealias);
  *u = NlFields{a_hat, b_hat, nullptr, nullptr, nullptr};
  u->ncomp = ncomp;
  u->nfields = b_hat ? 2 * ncomp : ncomp;
  return 0;
}

// [min, max, S1 .. S4] of ifftn(field, dealias) for the ncomp components of a and, where given, of b: see include/mpifft4py_amd.h
int mfft_real_moments(mfft_plan_t p, const void* a_hat, const void* b_hat, int ncomp, int dealias, const double* center, double* out,
                      int64_t* count) {
  if (!out || !count) return set_error(MFFT_ERR_INVALID, "null argument");
  NlFields u;
  MFFT_TRY(reduce_fields(p, a_hat, b_hat, ncomp, dealias, &u));
  return p->real_moments(u, dealias, center, out, count);
}

// counts of ifftn(field, dealias) in nbins equal bins per field, for the ncomp components of a and, where given, of b: see
// include/mpifft4py_amd.h
int mfft_real_histogram(mfft_plan_t p, const void* a_hat, const void* b_hat, int ncomp, int dealias, const double* lo, const double* hi,
                        int nbins, int64_t* out, int64_t* count) {
  if (!out || !count || !lo || !hi) return set_error(MFFT_ERR_INVALID, "null argument");
  NlFields u;
  MFFT_TRY(reduce_fields(p, a_hat, b_hat, ncomp, dealias, &u));
  return p->real_histogram(u, dealias, lo, hi, nbins, out, count);
}

// moments and counts of q = sum_f w_f ifftn(field f, dealias)^2 over the ncomp components of a and, where given, of b: see
// include/mpifft4py_amd.h
int mfft_real_quadratic(mfft_plan_t p, const void* a_hat, const void* b_hat, int ncomp, int dealias, const double* weights, double center,
                        double lo, double hi, int nbins, double* out6, int64_t* counts, int64_t* count) {
  if (!out6 || !count || !weights || (nbins > 0 && !counts)) return set_error(MFFT_ERR_INVALID, "null argument");
  NlFields u;
  MFFT_TRY(reduce_fields(p, a_hat, b_hat, ncomp, dealias, &u));
  return p->real_quadratic(u, dealias, weights, center, lo, hi, nbins, out6, counts, count);
}

// sums of the powers of the increments along z of ifftn(field f, dealias), for the ncomp components of a and, where given, of b:
// see include/mpifft4py_amd.h
int mfft_real_increments(mfft_plan_t p, const void* a_hat, const void* b_hat, int ncomp, int dealias, const int64_t* seps, int nsep,
                         double* out, int64_t* count) {
  if (!out || !count || !seps) return set_error(MFFT_ERR_INVALID, "null argument");
  NlFields u;
  MFFT_TRY(reduce_fields(p, a_hat, b_hat, ncomp, dealias, &u));
  return p->real_increments(u, dealias, seps, nsep, out, count);
}

// counts of the increments along z of ifftn(field f, dealias) in nbins equal bins per field and separation: see include/mpifft4py_amd.h
int mfft_real_increment_histogram(mfft_plan_t p, const void* a_hat, const void* b_hat, int ncomp, int dealias, const int64_t* seps, int nsep,
                                  const double* lo, const double* hi, int nbins, int64_t* out, int64_t* count) {
  if (!out || !count || !seps || !lo || !hi) return set_error(MFFT_ERR_INVALID, "null argument");
  NlFields u;
  MFFT_TRY(reduce_fields(p, a_hat, b_hat, ncomp, dealias, &u));
  return p->real_increment_histogram(u, dealias, seps, nsep, lo, hi, nbins, out, count);
}

// counts of the pairs (ifftn(a_f), ifftn(b_f)) in a grid of nba x nbb equal bins per pair: see include/mpifft4py_amd.h
int mfft_real_joint_histogram(mfft_plan_t p, const void* a_hat, const void* b_hat, int ncomp, int dealias, const double* lo, const double* hi,
                              int nba, int nbb, int64_t* out, int64_t* count) {
  if (!out || !count || !lo || !hi) return set_error(MFFT_ERR_INVALID, "null argument");
  if (!b_hat) return set_error(MFFT_ERR_INVALID, "a joint histogram counts pairs of fields: b_hat must not be NULL");
  NlFields u;
  MFFT_TRY(reduce_fields(p, a_hat, b_hat, ncomp, dealias, &u));
  return p->real_joint_histogram(u, dealias, lo, hi, nba, nbb, out, count);
}

// per pair (ifftn(a_f), ifftn(b_f)) and per z index the five plane sums: see include/mpifft4py_amd.h
int mfft_real_profiles(mfft_plan_t p, const void* a_hat, const void* b_hat, int ncomp, int dealias, const double* center, double* out,
                       int64_t* count) {
  if (!out || !count) return set_error(MFFT_ERR_INVALID, "null argument");
  if (!b_hat) return set_error(MFFT_ERR_INVALID, "a profile takes pairs of fields: b_hat must not be NULL (it may be a_hat)");
  NlFields u;
  MFFT_TRY(reduce_fields(p, a_hat, b_hat, ncomp, dealias, &u));
  return p->real_profiles(u, dealias, center, out, count);
}

int mfft_plan_sync(mfft_plan_t p) {
  if (!p) return set_error(MFFT_ERR_INVALID, "null plan");
  if (p->cstream) MFFT_HIP(hipStreamSynchronize(p->cstream));
  MFFT_HIP(hipStreamSynchronize(p->stream));
  return 0;
}

// "nonlinear[_dot|_cross_dot][_absmax]_fused_{none,2_3,3_2}": does the fused route take that product (with statistics) under that
// dealias mode?  One key per product, build it has and mode -- a product without a maxima build has no such key.
static bool nonlinear_fused_key(mfft_plan_t p, const std::string& k, int64_t* value) {
  static const struct { const char* name; int mode; } modes[] = {{"none", MFFT_DEALIAS_NONE}, {"2_3", MFFT_DEALIAS_2_3}, {"3_2", MFFT_DEALIAS_3_2}};
  for (const NlProduct& q : NL_PRODUCTS) {
    const std::string named = q.op == Op::Plain ? "nonlinear" : std::string("nonlinear_") + q.name;      // (the cross product's keys go unnamed)
    for (int stats = 0; stats <= (q.absmax ? 1 : 0); ++stats)
      for (const auto& m : modes)
        if (k == named + (stats ? "_absmax" : "") + "_fused_" + m.name) {
          *value = p->nonlinear_fusable(m.mode, q.op, stats != 0) ? 1 : 0;
          return true;
        }
  }
  return false;
}

int mfft_plan_get_info(mfft_plan_t p, const char* key, int64_t* value) {
  if (!p || !key || !value) return set_error(MFFT_ERR_INVALID, "null argument");
  const std::string k(key);
  if (k == "pruned_route") *value = p->band_ok ? (p->band_allzero ? 2 : 1) : 0;
  else if (k == "local_band") *value = p->lband_ok ? 1 : 0;
  else if (k == "comm_cus") *value = p->comm_cus;
  else if (k == "kz_slices") *value = p->nslice;
  else if (k == "row_batches") *value = p->nbatch;
  else if (k == "zfuse") *value = p->zfuse ? 1 : 0;
  else if (k == "ranks") *value = p->P;
  else if (k == "complex_pitch") *value = p->pitched() ? p->Zp : 0;        // row pitch of the caller's spectrum (elements), 0 = compact
  else if (k == "complex_pitch_native") *value = p->nat_pitch() ? 1 : 0;  // 1: the routes run on the pitched rows themselves
  else if (nonlinear_fused_key(p, k, value)) return 0;
  else if (k == "nonlinear_bytes") *value = (int64_t)(p->nlx.bytes + p->nly.bytes + p->nlr.bytes + p->nlw[0].bytes + p->nlw[1].bytes + p->nlq.bytes);
  else if (k == "split_last") *value = p->split_last_route() ? 1 : 0;   // the one-rank route that splits real / complex last (decides whether the work buffer fits, if no call has yet)
  // layout of that route's work array (plan_impl.h SplitLastLayout; 0 where the plan does not take the route): rows per y block,
  // elements between the x rows of a block and between blocks, the order (0 x first, 1 y first, 2 y first forward only); and the bytes of the work buffer as allocated
  else if (k == "split_last_yblock") *value = p->split_last_route() ? p->split_last_layout().B : 0;
  else if (k == "split_last_row_pitch") *value = p->split_last_route() ? p->split_last_layout().SR : 0;
  else if (k == "split_last_block_pitch") *value = p->split_last_route() ? p->split_last_layout().SB : 0;
  else if (k == "split_last_yfirst") *value = p->split_last_route() ? p->split_last_layout().yfirst : 0;
  // route "x near" (plan_slab.hip): the directions that take it (0 none, 1 both, 2 forward, 3 inverse), the pitches of its transposed
  // array W_T, the tile of the z passes' slot order on it, and the bytes of W_T as allocated
  else if (k == "split_last_xnear") *value = p->split_last_xnear_mode();
  else if (k == "split_last_xnear_row_pitch") *value = p->split_last_xnear_mode() ? p->split_last_layout_t().SR : 0;
  else if (k == "split_last_xnear_block_pitch") *value = p->split_last_xnear_mode() ? p->split_last_layout_t().SB : 0;
  else if (k == "split_last_pairblock") *value = p->split_last_route() ? p->split_last_pair_tile(p->split_last_xnear_mode() != 0) : 0;
  else if (k == "split_last_pairxfast") *value = !p->split_last_route() ? 0 : (p->split_last_pair_xfast(p->split_last_xnear_mode() != 0, false) ? 1 : 0) + (p->split_last_pair_xfast(p->split_last_xnear_mode() != 0, true) ? 2 : 0);
  else if (k == "split_last_xnear_work_bytes") *value = p->split_last_xnear_mode() ? (int64_t)p->work[1].bytes : 0;
  else if (k == "work_bytes") *value = (int64_t)p->work[0].bytes;
  else if (k == "plane_pad") *value = (p->P == 1 && p->d.decomp == MFFT_SLAB) ? p->p1_plane_pad() : 0;   // elements added to the intermediate's plane pitch
  else return set_error(MFFT_ERR_INVALID, "mfft_plan_get_info: unknown key '%s'", key);
  return 0;
}

int mfft_plan_timing(mfft_plan_t p, int enable) {
  if (!p) return set_error(MFFT_ERR_INVALID, "null plan");
  p->timing = enable != 0;
  return 0;
}

int mfft_plan_timing_reset(mfft_plan_t p) {
  if (!p) return set_error(MFFT_ERR_INVALID, "null plan");
  MFFT_TRY(p->collect_timing());
  for (auto& t : p->timers) {
    t.total_ms = 0;
    t.calls = 0;
  }
  return 0;
}

int mfft_plan_timing_get(mfft_plan_t p, int max_stages, char names[][32], double* total_ms, int64_t* calls, double* alg_bytes) {
  if (!p) return set_error(MFFT_ERR_INVALID, "null plan");
  MFFT_TRY(p->collect_timing());
  const int n = (int)p->timers.size();
  for (int i = 0; i < n && i < max_stages; ++i) {
    if (names) {
      strncpy(names[i], p->timers[i].name.c_str(), 31);
      names[i][31] = 0;
    }
    if (total_ms) total_ms[i] = p->timers[i].total_ms;
    if (calls) calls[i] = p->timers[i].calls;
    if (alg_bytes) alg_bytes[i] = p->timers[i].alg_bytes;
  }
  return n;
}

}  // extern "C"
