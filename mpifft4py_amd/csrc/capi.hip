// capi.hip -- the extern "C" surface of libmpifft4py_amd.so that is not the plan
// executor (plan_*.hip): device/memory helpers, communicators, the stage-level
// "serialFFT seam" entry points and HIP-event timers.
#include <cmath>
#include <cstring>
#include "comm.h"
#include "mfft_internal.h"
#include "fft_nlz.h"
#include "nlz_moments.h"

using namespace mfft;

extern "C" {

int mfft_version(void) { return 100; }   // 0.1.0
const char* mfft_last_error(void) { return last_error(); }

int mfft_device_count(int* count) {
  if (!count) return set_error(MFFT_ERR_INVALID, "null argument");
  hipError_t e = hipGetDeviceCount(count);
  if (e != hipSuccess) {
    *count = 0;
    return set_error(MFFT_ERR_HIP, "hipGetDeviceCount: %s", hipGetErrorString(e));
  }
  return 0;
}
int mfft_set_device(int device) {
  MFFT_HIP(hipSetDevice(device));
  return 0;
}
int mfft_get_device(int* device) {
  MFFT_HIP(hipGetDevice(device));
  return 0;
}
int mfft_device_name(char* buf, size_t buflen) {
  int dev = 0;
  MFFT_HIP(hipGetDevice(&dev));
  hipDeviceProp_t prop;
  MFFT_HIP(hipGetDeviceProperties(&prop, dev));
  snprintf(buf, buflen, "%s (%s, %d CUs)", prop.name, prop.gcnArchName, prop.multiProcessorCount);
  return 0;
}
int mfft_device_sync(void) {
  MFFT_HIP(hipDeviceSynchronize());
  return 0;
}

int mfft_malloc(void** dptr, size_t bytes) {
  if (!dptr) return set_error(MFFT_ERR_INVALID, "null argument");
  *dptr = nullptr;
  return dev_alloc(dptr, bytes);      // registered: the buffer may be the source or target of an exchange
}
int mfft_free(void* dptr) { return dev_free(dptr); }
// The transforms run asynchronously on their plan's own non-blocking stream, which the null stream does not order
// against.  These helpers therefore wait for ALL work of the device (every plan's streams) before they touch memory,
// and return when the copy is complete: a copy issued after mfft_forward sees its result, a transform issued after
// a copy sees the copied data.
int mfft_memset(void* dptr, int value, size_t bytes) {
  MFFT_HIP(hipDeviceSynchronize());
  MFFT_HIP(hipMemset(dptr, value, bytes));
  MFFT_HIP(hipDeviceSynchronize());
  return 0;
}
int mfft_memcpy_h2d(void* dst, const void* src, size_t bytes) {
  MFFT_HIP(hipDeviceSynchronize());
  MFFT_HIP(hipMemcpy(dst, src, bytes, hipMemcpyHostToDevice));
  return 0;
}
int mfft_memcpy_d2h(void* dst, const void* src, size_t bytes) {
  MFFT_HIP(hipDeviceSynchronize());
  MFFT_HIP(hipMemcpy(dst, src, bytes, hipMemcpyDeviceToHost));
  return 0;
}
// rows of `width_bytes` bytes, `rows` of them: device rows dev_pitch_bytes apart <-> packed host rows (pitched spectra)
int mfft_memcpy_rows_h2d(void* dst, size_t dev_pitch_bytes, const void* src_host, size_t width_bytes, size_t rows) {
  if (width_bytes > dev_pitch_bytes) return set_error(MFFT_ERR_INVALID, "row wider than its pitch");
  MFFT_HIP(hipDeviceSynchronize());
  MFFT_HIP(hipMemcpy2D(dst, dev_pitch_bytes, src_host, width_bytes, width_bytes, rows, hipMemcpyHostToDevice));
  return 0;
}
int mfft_memcpy_rows_d2h(void* dst_host, const void* src, size_t dev_pitch_bytes, size_t width_bytes, size_t rows) {
  if (width_bytes > dev_pitch_bytes) return set_error(MFFT_ERR_INVALID, "row wider than its pitch");
  MFFT_HIP(hipDeviceSynchronize());
  MFFT_HIP(hipMemcpy2D(dst_host, width_bytes, src, dev_pitch_bytes, width_bytes, rows, hipMemcpyDeviceToHost));
  return 0;
}
int mfft_memcpy_d2d(void* dst, const void* src, size_t bytes) {
  MFFT_HIP(hipDeviceSynchronize());
  MFFT_HIP(hipMemcpy(dst, src, bytes, hipMemcpyDeviceToDevice));
  MFFT_HIP(hipDeviceSynchronize());
  return 0;
}
int mfft_fill_uniform(void* dptr, size_t count, int precision, uint64_t seed) {
  MFFT_TRY(launch_fill_uniform(dptr, count, precision, seed, nullptr));
  MFFT_HIP(hipStreamSynchronize(nullptr));
  return 0;
}

// ---- communicators -------------------------------------------------------------
int mfft_comm_create_self(mfft_comm_t* comm) {
  if (!comm) return set_error(MFFT_ERR_INVALID, "null argument");
  return comm_create_self(comm);
}
int mfft_get_unique_id(void* id128) { return comm_get_unique_id(id128); }
int mfft_comm_create_rccl(int nranks, int rank, const void* id128, mfft_comm_t* comm) {
  if (!comm || !id128) return set_error(MFFT_ERR_INVALID, "null argument");
  return comm_create_rccl(nranks, rank, id128, comm);
}
int mfft_comm_create_local(int nranks, const int* devices, mfft_comm_t* comms_out) {
  if (!comms_out) return set_error(MFFT_ERR_INVALID, "null argument");
  return comm_create_local(nranks, devices, comms_out);
}
int mfft_comm_size(mfft_comm_t c, int* size) {
  if (!c || !size) return set_error(MFFT_ERR_INVALID, "null argument");
  *size = c->size;
  return 0;
}
int mfft_comm_rank(mfft_comm_t c, int* rank) {
  if (!c || !rank) return set_error(MFFT_ERR_INVALID, "null argument");
  *rank = c->rank;
  return 0;
}
int mfft_comm_barrier(mfft_comm_t c) { return c ? c->barrier() : set_error(MFFT_ERR_INVALID, "null comm"); }
int mfft_comm_bcast_host(mfft_comm_t c, void* buf, size_t bytes, int root) {
  return c ? c->bcast_host(buf, bytes, root) : set_error(MFFT_ERR_INVALID, "null comm");
}
int mfft_comm_allreduce_sum_host(mfft_comm_t c, double* v, int n) {
  return c ? c->allreduce_host(v, n, 0) : set_error(MFFT_ERR_INVALID, "null comm");
}
int mfft_comm_allreduce_max_host(mfft_comm_t c, double* v, int n) {
  return c ? c->allreduce_host(v, n, 1) : set_error(MFFT_ERR_INVALID, "null comm");
}
int mfft_comm_selftest(mfft_comm_t c, size_t bytes_per_peer, int timeout_ms) {
  if (!c || timeout_ms <= 0) return set_error(MFFT_ERR_INVALID, "bad argument");
  return c->selftest(bytes_per_peer ? bytes_per_peer : 4096, timeout_ms);
}
int mfft_comm_set_option(mfft_comm_t c, const char* key, int64_t value) {
  if (!c || !key) return set_error(MFFT_ERR_INVALID, "null argument");
  return c->set_option(key, (long long)value);
}
// PCI bus id of a device ("0000:05:00.0"): names the physical GPU behind a rank in a bench line
int mfft_device_pci_bus_id(int device, char* buf, size_t buflen) {
  if (!buf || buflen < 16) return set_error(MFFT_ERR_INVALID, "buffer of at least 16 bytes needed");
  MFFT_HIP(hipDeviceGetPCIBusId(buf, (int)buflen, device));
  return 0;
}

int mfft_comm_get_option(mfft_comm_t c, const char* key, int64_t* value) {
  if (!c || !key || !value) return set_error(MFFT_ERR_INVALID, "null argument");
  *value = (int64_t)c->get_option(key);
  return 0;
}
int mfft_comm_abort(mfft_comm_t c) {
  if (c) c->abort();
  return 0;
}
int mfft_comm_destroy(mfft_comm_t c) {
  if (!c) return 0;
  if (c->plan_refs > 0) {                  // plans still use it (their work buffers live in it): the last one frees it
    c->destroy_requested = true;
    return 0;
  }
  delete c;
  return 0;
}

// ---- stage level ------------------------------------------------------------------
int mfft_length_supported(int64_t n, int real_transform) { return length_supported(n, real_transform != 0) ? 1 : 0; }
int mfft_length_route(int64_t n, int real_transform) { return length_route(n, real_transform != 0); }
int mfft_length_route_precision(int64_t n, int real_transform, int precision) {
  if (precision != MFFT_DOUBLE && precision != MFFT_SINGLE) return 0;
  return length_route(n, real_transform != 0, precision);
}

int mfft_kernel_name(int family, int64_t n, int precision, int inverse, int nt, char* buf, size_t buflen) {
  if (!buf || buflen == 0 || family < FAM_COL || family > FAM_C2R) return set_error(MFFT_ERR_INVALID, "bad argument");
  const KernelEntry* e = find_kernel(family, (int)n, precision, family == FAM_C2R ? 1 : (inverse ? 1 : 0), Op::Plain, nt ? Build::NonTemporal : Build::Default);
  if (!e) return set_error(MFFT_ERR_UNSUPPORTED, "no radix kernel of family %d for length %lld", family, (long long)n);
  snprintf(buf, buflen, "%s tile=%d threads=%d lds=%d%s", e->name, e->tile, e->threads, e->lds_bytes, e->build == Build::NonTemporal ? " nt" : "");
  return 0;
}

int mfft_c2c_axis(const void* in, void* out, const int64_t shape[3], int axis, int inverse, int precision) {
  if (!in || !out || !shape) return set_error(MFFT_ERR_INVALID, "null argument");
  const int64_t s0 = shape[0], s1 = shape[1], s2 = shape[2];
  if (s0 < 1 || s1 < 1 || s2 < 1) return set_error(MFFT_ERR_INVALID, "bad shape");
  const int64_t n = shape[axis];
  const size_t es = elem_bytes(precision, true);
  if (n == 1) {
    if (in != out) MFFT_HIP(hipMemcpy(out, in, (size_t)(s0 * s1 * s2) * es, hipMemcpyDeviceToDevice));
    return 0;
  }
  if (axis == 2) {
    RowArgs a;
    a.in = in; a.out = out; a.n = (int)n; a.prec = precision; a.inverse = inverse != 0;
    a.in_stride = a.out_stride = s2; a.nrows = s0 * s1; a.scale = inverse ? 1.0 / (double)n : 1.0;
    MFFT_TRY(launch_row(a, nullptr));
  } else if (axis == 0 || axis == 1) {
    ColArgs a;
    a.in = in; a.out = out; a.n = (int)n; a.prec = precision; a.inverse = inverse != 0;
    a.scale = inverse ? 1.0 / (double)n : 1.0;
    if (axis == 1) {
      a.nouter = s0; a.ncols = s2; a.in_outer = a.out_outer = s1 * s2;
      a.in_rows.lo = a.out_rows.lo = s2;
    } else {
      a.nouter = 1; a.ncols = s1 * s2; a.in_outer = a.out_outer = 0;
      a.in_rows.lo = a.out_rows.lo = s1 * s2;
    }
    MFFT_TRY(launch_col(a, nullptr));
  } else {
    return set_error(MFFT_ERR_INVALID, "bad axis %d", axis);
  }
  MFFT_HIP(hipStreamSynchronize(nullptr));
  return 0;
}

// The strided transform with every stride spelled out (the "advanced" layout of a stage-level call: what numpy does for a
// non-contiguous view, numpy_fft.py:25-37): nouter batches in_outer / out_outer elements apart, each ncols contiguous
// columns wide, rows in_pitch / out_pitch elements apart.
int mfft_c2c_strided(const void* in, void* out, int64_t n, int64_t nouter, int64_t ncols, int64_t in_outer, int64_t in_pitch,
                     int64_t out_outer, int64_t out_pitch, int inverse, int precision) {
  if (!in || !out) return set_error(MFFT_ERR_INVALID, "null argument");
  if (n < 1 || nouter < 1 || ncols < 1 || in_pitch < ncols || out_pitch < ncols)
    return set_error(MFFT_ERR_INVALID, "bad extents: n %lld, %lld batches of %lld columns, pitches %lld / %lld", (long long)n,
                     (long long)nouter, (long long)ncols, (long long)in_pitch, (long long)out_pitch);
  ColArgs a;
  a.in = in; a.out = out; a.n = (int)n; a.prec = precision; a.inverse = inverse != 0;
  a.scale = inverse ? 1.0 / (double)n : 1.0;
  a.nouter = nouter; a.ncols = ncols; a.in_outer = in_outer; a.out_outer = out_outer;
  a.in_rows.lo = in_pitch; a.out_rows.lo = out_pitch;
  MFFT_TRY(launch_col(a, nullptr));
  MFFT_HIP(hipStreamSynchronize(nullptr));
  return 0;
}

int mfft_r2c_last(const void* in, void* out, const int64_t rshape[3], int precision) {
  if (!in || !out || !rshape) return set_error(MFFT_ERR_INVALID, "null argument");
  RealArgs a;
  a.in = in; a.out = out; a.n = (int)rshape[2]; a.prec = precision;
  a.in_stride = rshape[2]; a.out_stride = rshape[2] / 2 + 1; a.nrows = rshape[0] * rshape[1]; a.scale = 1.0;
  MFFT_TRY(launch_r2c(a, nullptr));
  MFFT_HIP(hipStreamSynchronize(nullptr));
  return 0;
}

int mfft_c2r_last(const void* in, void* out, const int64_t rshape[3], int precision) {
  if (!in || !out || !rshape) return set_error(MFFT_ERR_INVALID, "null argument");
  RealArgs a;
  a.in = in; a.out = out; a.n = (int)rshape[2]; a.prec = precision;
  a.in_stride = rshape[2] / 2 + 1; a.out_stride = rshape[2]; a.nrows = rshape[0] * rshape[1];
  a.scale = 1.0 / (double)rshape[2];
  MFFT_TRY(launch_c2r(a, nullptr));
  MFFT_HIP(hipStreamSynchronize(nullptr));
  return 0;
}

// the rows of one product for launch_nlz: a, b (and c) are (3, nrows, pitch) complex, out the product's vector result (nullptr:
// none), s its scalar row (nrows, pitch), the row after the vector's
static NlzArgs nlz_args(Op product, const void* a, const void* b, const void* c, void* out, void* s, int64_t nrows, int64_t n, int64_t pitch,
                        int64_t valid, int precision) {
  const size_t comp = (size_t)(nrows * pitch) * elem_bytes(precision, true);
  NlzArgs z;
  for (int f = 0; f < 3; ++f) {
    z.a[f] = static_cast<const char*>(a) + f * comp;
    z.b[f] = static_cast<const char*>(b) + f * comp;
    if (c) z.c[f] = static_cast<const char*>(c) + f * comp;
    if (out) z.out[f] = static_cast<char*>(out) + f * comp;
  }
  z.out[out ? 3 : 0] = s;
  z.product = product;
  z.n = (int)n; z.prec = precision; z.in_stride = pitch; z.out_stride = pitch; z.nrows = nrows; z.valid = (int)valid;
  z.scale = 1.0 / ((double)n * (double)n);
  return z;
}
static int nlz_run(const NlzArgs& z, int sync) {
  MFFT_TRY(launch_nlz(z, nullptr));
  if (sync) MFFT_HIP(hipStreamSynchronize(nullptr));
  return 0;
}

// fused nonlinear z stage on rows (csrc/fft_nlz.h): a, b, out are (3, nrows, pitch) complex, `valid` bins per row exist
int mfft_nlz_rows(const void* a, const void* b, void* out, int64_t nrows, int64_t n, int64_t pitch, int64_t valid, int precision,
                  int sync) {
  if (!a || !b || !out || nrows < 1 || n < 2 || pitch < valid || valid < 1) return set_error(MFFT_ERR_INVALID, "bad argument");
  return nlz_run(nlz_args(Op::Plain, a, b, nullptr, out, nullptr, nrows, n, pitch, valid, precision), sync);
}

// ... and with the dot product: a, b (3, nrows, pitch), out (nrows, pitch); out may be any one component of a or b
int mfft_nlz_dot_rows(const void* a, const void* b, void* out, int64_t nrows, int64_t n, int64_t pitch, int64_t valid, int precision,
                      int sync) {
  if (!a || !b || !out || nrows < 1 || n < 2 || pitch < valid || valid < 1) return set_error(MFFT_ERR_INVALID, "bad argument");
  return nlz_run(nlz_args(Op::Dot, a, b, nullptr, nullptr, out, nrows, n, pitch, valid, precision), sync);
}

// ... and with both products (fft_nlz.h body_cross_dot): a, b, c, out (3, nrows, pitch), s (nrows, pitch); out may be a or b, s any
// one component they leave alone
int mfft_nlz_cross_dot_rows(const void* a, const void* b, const void* c, void* out, void* s, int64_t nrows, int64_t n, int64_t pitch,
                            int64_t valid, int precision, int sync) {
  if (!a || !b || !c || !out || !s || nrows < 1 || n < 2 || pitch < valid || valid < 1) return set_error(MFFT_ERR_INVALID, "bad argument");
  return nlz_run(nlz_args(Op::CrossDot, a, b, c, out, s, nrows, n, pitch, valid, precision), sync);
}

// ... and with the outer product (fft_nlz.h body_outer): a, b (3, nrows, pitch), out (9, nrows, pitch), component 3 i + j the rows of
// a_i b_j; out's components 0..5 may be the six input components (a's, then b's), row for row
int mfft_nlz_outer_rows(const void* a, const void* b, void* out, int64_t nrows, int64_t n, int64_t pitch, int64_t valid, int precision,
                        int sync) {
  if (!a || !b || !out || nrows < 1 || n < 2 || pitch < valid || valid < 1) return set_error(MFFT_ERR_INVALID, "bad argument");
  NlzArgs z = nlz_args(Op::Outer, a, b, nullptr, out, nullptr, nrows, n, pitch, valid, precision);
  const size_t comp = (size_t)(nrows * pitch) * elem_bytes(precision, true);
  for (int c = 3; c < 9; ++c) z.out[c] = static_cast<char*>(out) + c * comp;
  return nlz_run(z, sync);
}

// The stage with the maxima of its six real rows (fft_nlz.h NlzAbsMax), synchronous: out as mfft_nlz_rows (dot = 0) or
// mfft_nlz_dot_rows (dot = 1) leave it, out6 = [max |irfft(a_f)|, f = 0..2, max |irfft(b_f)|, f = 0..2] over all rows.
int mfft_nlz_rows_absmax(const void* a, const void* b, void* out, int64_t nrows, int64_t n, int64_t pitch, int64_t valid, int precision,
                         int dot, double out6[6]) {
  if (!a || !b || !out || !out6 || nrows < 1 || n < 2 || pitch < valid || valid < 1) return set_error(MFFT_ERR_INVALID, "bad argument");
  if (precision != MFFT_DOUBLE && precision != MFFT_SINGLE) return set_error(MFFT_ERR_INVALID, "unknown precision %d", precision);
  const size_t es = elem_bytes(precision, true);
  NlzArgs z = dot ? nlz_args(Op::Dot, a, b, nullptr, nullptr, out, nrows, n, pitch, valid, precision)
                  : nlz_args(Op::Plain, a, b, nullptr, out, nullptr, nrows, n, pitch, valid, precision);
  const int64_t waves = nlz_absmax_waves(n, precision, z.product, nrows);
  if (waves < 1) return set_error(MFFT_ERR_UNSUPPORTED, "no fused nonlinear z-stage kernel of length %lld with maxima", (long long)n);
  const size_t head = absmax_fold_scratch_bytes() + 6 * sizeof(double);
  char* buf = nullptr;
  MFFT_HIP(hipMalloc(reinterpret_cast<void**>(&buf), head + (size_t)waves * NLM_SLOTS * (es / 2)));
  double* acc = reinterpret_cast<double*>(buf + absmax_fold_scratch_bytes());
  z.part = buf + head;
  int rc = hipMemsetAsync(acc, 0, 6 * sizeof(double), nullptr) == hipSuccess ? 0 : set_error(MFFT_ERR_HIP, "hipMemsetAsync failed");
  if (!rc) rc = launch_nlz(z, nullptr);
  if (!rc) rc = absmax_fold(z.part, (size_t)(2 * waves), 6, precision, 1.0 / (double)n, reinterpret_cast<double*>(buf), acc, nullptr);
  if (!rc && hipMemcpy(out6, acc, 6 * sizeof(double), hipMemcpyDeviceToHost) != hipSuccess) rc = set_error(MFFT_ERR_HIP, "hipMemcpy failed");
  if (hipStreamSynchronize(nullptr) != hipSuccess && !rc) rc = set_error(MFFT_ERR_HIP, "hipStreamSynchronize failed");
  (void)hipFree(buf);
  return rc;
}

// The stages that end in a reduction (the body of NlzMoments, NlzHist, NlzJoint, NlzQuad, NlzIncr, NlzIncrHist, NlzProf: a header each, nlz_*.h), synchronous; what
// their seven entry points share.  nfields = 1: a is (nrows, pitch); 2: a and b are; 3: a is (3, nrows, pitch); 6: a and b are.  `valid`
// bins per row exist, the first valid_in of them are read (0: all of them).  Fields in the order a_0.., then b_0..; field f rides in
// slot nls_slot(u, f), the plan's rule.  Everything is checked before the first launch; the outputs are written on success only.
static int nlr_stage_args(Op kind, const void* a, const void* b, int nfields, int64_t nrows, int64_t n, int64_t pitch, int64_t valid,
                          int64_t valid_in, int precision, NlFields* u, NlrArgs* z) {
  if (!a || nrows < 1 || n < 2 || n >= 65536 || pitch < valid || valid < 1 || valid > n / 2 + 1 || valid_in < 0 || valid_in > valid)
    return set_error(MFFT_ERR_INVALID, "bad argument");
  if (precision != MFFT_DOUBLE && precision != MFFT_SINGLE) return set_error(MFFT_ERR_INVALID, "unknown precision %d", precision);
  if ((nfields != 1 && nfields != 2 && nfields != 3 && nfields != 6) || ((nfields % 2 == 0) != (b != nullptr)))
    return set_error(MFFT_ERR_INVALID, "nfields must be 1 or 3 (a alone) or 2 or 6 (a and b), not %d", nfields);
  *u = NlFields{a, b, nullptr, nullptr, nullptr};
  u->nfields = nfields;
  u->ncomp = b ? nfields / 2 : nfields;
  z->kind = kind;
  for (int f = 0; f < nfields; ++f) {
    const int slot = nls_slot(*u, f);
    (slot % 2 ? z->b : z->a)[slot / 2] = u->src(f, nrows * pitch, elem_bytes(precision, true));
  }
  z->npairs = (nfields + 1) / 2;
  z->n = (int)n; z->prec = precision; z->in_stride = pitch; z->nrows = nrows; z->valid = (int)valid; z->valid_in = (int)valid_in;
  z->norm = 1.0 / (double)n;
  return 0;
}
// One device buffer [acc | acc2 | part]: the accumulators cleared (statistics: the identity of moments_clear; sums and counts:
// zeros), all rows run and folded (nlr_rows), the accumulators copied to host and host2.
static int nlr_stage_run(NlrArgs& z, size_t acc_bytes, void* host, size_t acc2_bytes, void* host2) {
  NlrShape shape;
  MFFT_TRY(nlr_launch_shape(z.kind, z.n, z.prec, z.nrows, &shape));
  const size_t off2 = (acc_bytes + 127) / 128 * 128, offp = off2 + (acc2_bytes + 127) / 128 * 128;
  char* buf = nullptr;
  MFFT_HIP(hipMalloc(reinterpret_cast<void**>(&buf), offp + nlr_part_bytes(z, shape)));
  z.part = buf + offp;
  const bool stats = z.kind == Op::Moments || z.kind == Op::Quadratic;
  int rc = stats ? moments_clear(reinterpret_cast<double*>(buf), (int)(acc_bytes / sizeof(double)), nullptr) : 0;
  if (!rc && !stats && hipMemsetAsync(buf, 0, acc_bytes, nullptr) != hipSuccess) rc = set_error(MFFT_ERR_HIP, "hipMemsetAsync failed");
  if (!rc && acc2_bytes && hipMemsetAsync(buf + off2, 0, acc2_bytes, nullptr) != hipSuccess) rc = set_error(MFFT_ERR_HIP, "hipMemsetAsync failed");
  if (!rc) rc = nlr_rows(z, buf, buf + off2, nullptr);
  if (!rc && hipMemcpy(host, buf, acc_bytes, hipMemcpyDeviceToHost) != hipSuccess) rc = set_error(MFFT_ERR_HIP, "hipMemcpy failed");
  if (!rc && acc2_bytes && hipMemcpy(host2, buf + off2, acc2_bytes, hipMemcpyDeviceToHost) != hipSuccess) rc = set_error(MFFT_ERR_HIP, "hipMemcpy failed");
  if (hipStreamSynchronize(nullptr) != hipSuccess && !rc) rc = set_error(MFFT_ERR_HIP, "hipStreamSynchronize failed");
  (void)hipFree(buf);
  return rc;
}
// workgroups of the first launch over those rows: a caller that wants more rows than one pass of the grid asks here (0: no kernel
// of that length)
static int64_t nlr_stage_groups(Op kind, int64_t nrows, int64_t n, int precision) {
  NlrShape shape;
  return nlr_launch_shape(kind, n, precision, nrows, &shape) == 0 ? shape.ngroups : 0;
}

// out[f * 6 + {0: min, 1: max, 2..5: S1..S4}] of irfft(row, n) over all rows; S_p = sum (x - center[f])^p (center null: zeros).
int mfft_nlz_moments_rows(const void* a, const void* b, int nfields, int64_t nrows, int64_t n, int64_t pitch, int64_t valid,
                          int64_t valid_in, int precision, const double* center, double* out) {
  if (!out) return set_error(MFFT_ERR_INVALID, "bad argument");
  NlFields u;
  NlrArgs z;
  MFFT_TRY(nlr_stage_args(Op::Moments, a, b, nfields, nrows, n, pitch, valid, valid_in, precision, &u, &z));
  for (int f = 0; center && f < nfields; ++f) z.call.center[nls_slot(u, f)] = center[f];
  double host[NLS_SLOTS];
  MFFT_TRY(nlr_stage_run(z, sizeof host, host, 0, nullptr));
  for (int f = 0; f < nfields; ++f)
    for (int k = 0; k < NLS_STATS; ++k) out[f * NLS_STATS + k] = host[nls_slot(u, f) * NLS_STATS + k];
  return 0;
}
int64_t mfft_nlz_moments_groups(int64_t nrows, int64_t n, int precision) { return nlr_stage_groups(Op::Moments, nrows, n, precision); }

// out[(f * nsep + i) * 3 + {0, 1, 2}] = S2, S3, S4 of the increments of irfft(row, n) at seps[i] over all rows
int mfft_nlz_incr_rows(const void* a, const void* b, int nfields, int64_t nrows, int64_t n, int64_t pitch, int64_t valid, int64_t valid_in,
                       int precision, const int64_t* seps, int nsep, double* out) {
  if (!out || !seps) return set_error(MFFT_ERR_INVALID, "bad argument");
  NlFields u;
  NlrArgs z;
  MFFT_TRY(nlr_stage_args(Op::Increments, a, b, nfields, nrows, n, pitch, valid, valid_in, precision, &u, &z));
  MFFT_TRY(incr_check(seps, nsep, n));
  for (int i = 0; i < nsep; ++i) z.call.sep[i] = (int)seps[i];
  z.call.nsep = nsep;
  double host[INCR_SLOTS];
  MFFT_TRY(nlr_stage_run(z, sizeof host, host, 0, nullptr));
  for (int f = 0; f < nfields; ++f)
    for (int i = 0; i < nsep; ++i)
      for (int k = 0; k < 3; ++k) out[(f * nsep + i) * 3 + k] = host[(nls_slot(u, f) * MFFT_INCR_MAXSEP + i) * 3 + k];
  return 0;
}
int64_t mfft_nlz_incr_groups(int64_t nrows, int64_t n, int precision) { return nlr_stage_groups(Op::Increments, nrows, n, precision); }

// out[(f * nsep + i) * (nbins + 3) + slot] = counts of the increments of irfft(row, n) at seps[i] over all rows; lo, hi: [f * nsep + i]
int mfft_nlz_incr_hist_rows(const void* a, const void* b, int nfields, int64_t nrows, int64_t n, int64_t pitch, int64_t valid, int64_t valid_in,
                            int precision, const int64_t* seps, int nsep, const double* lo, const double* hi, int nbins, int64_t* out) {
  if (!out || !seps || !lo || !hi) return set_error(MFFT_ERR_INVALID, "bad argument");
  NlFields u;
  NlrArgs z;
  MFFT_TRY(nlr_stage_args(Op::IncrementHistogram, a, b, nfields, nrows, n, pitch, valid, valid_in, precision, &u, &z));
  MFFT_TRY(incr_check(seps, nsep, n));
  if (nbins < 1 || nbins > MFFT_INCR_HIST_MAXBINS) return set_error(MFFT_ERR_INVALID, "nbins must be 1 .. %d, not %d", MFFT_INCR_HIST_MAXBINS, nbins);
  for (int f = 0; f < 6; ++f)
    for (int i = 0; i < MFFT_INCR_MAXSEP; ++i) { z.call.ilo[f][i] = 0.0; z.call.iinv[f][i] = 1.0; }
  for (int f = 0; f < nfields; ++f)
    for (int i = 0; i < nsep; ++i) {
      const int slot = nls_slot(u, f);
      MFFT_TRY(incr_hist_range(lo[f * nsep + i], hi[f * nsep + i], nbins, &z.call.iinv[slot][i]));
      z.call.ilo[slot][i] = lo[f * nsep + i];
    }
  for (int i = 0; i < nsep; ++i) z.call.sep[i] = (int)seps[i];
  z.call.nsep = nsep;
  z.call.nbins = nbins;
  const size_t row = (size_t)nsep * (nbins + 3);
  std::vector<int64_t> host((size_t)2 * z.npairs * row);
  MFFT_TRY(nlr_stage_run(z, host.size() * sizeof(int64_t), host.data(), 0, nullptr));
  for (int f = 0; f < nfields; ++f) memcpy(out + (size_t)f * row, host.data() + (size_t)nls_slot(u, f) * row, row * sizeof(int64_t));
  return 0;
}
int64_t mfft_nlz_incr_hist_groups(int64_t nrows, int64_t n, int precision) { return nlr_stage_groups(Op::IncrementHistogram, nrows, n, precision); }

// a, b: (ncomp, nrows, pitch), ncomp 1 or 3, pair p = (a_p, b_p); center: a_0.., then b_0.. (null: zeros)
// out[(p * 5 + s) * n + m] = the sums over all rows of d_a, d_b, d_a^2, d_b^2, d_a d_b at position m of (irfft(a_p row, n), irfft(b_p row, n))
int mfft_nlz_profile_rows(const void* a, const void* b, int ncomp, int64_t nrows, int64_t n, int64_t pitch, int64_t valid, int64_t valid_in,
                          int precision, const double* center, double* out) {
  if (!b || !out) return set_error(MFFT_ERR_INVALID, "bad argument");
  if (ncomp != 1 && ncomp != 3) return set_error(MFFT_ERR_INVALID, "ncomp must be 1 or 3, not %d", ncomp);
  NlFields u;
  NlrArgs z;
  MFFT_TRY(nlr_stage_args(Op::Profiles, a, b, 2 * ncomp, nrows, n, pitch, valid, valid_in, precision, &u, &z));
  MFFT_TRY(prof_check(center, 2 * ncomp));
  for (int f = 0; center && f < 2 * ncomp; ++f) z.call.center[nls_slot(u, f)] = center[f];
  std::vector<double> host((size_t)ncomp * MFFT_PROFILE_STATS * (size_t)n);      // (the pairs lie in slot order already)
  MFFT_TRY(nlr_stage_run(z, host.size() * sizeof(double), host.data(), 0, nullptr));
  memcpy(out, host.data(), host.size() * sizeof(double));
  return 0;
}
int64_t mfft_nlz_profile_groups(int64_t nrows, int64_t n, int precision) { return nlr_stage_groups(Op::Profiles, nrows, n, precision); }

// out[f * (nbins + 3) + slot] = counts of irfft(row, n) over all rows
int mfft_nlz_hist_rows(const void* a, const void* b, int nfields, int64_t nrows, int64_t n, int64_t pitch, int64_t valid, int64_t valid_in,
                       int precision, const double* lo, const double* hi, int nbins, int64_t* out) {
  if (!out || !lo || !hi) return set_error(MFFT_ERR_INVALID, "bad argument");
  NlFields u;
  NlrArgs z;
  MFFT_TRY(nlr_stage_args(Op::Histogram, a, b, nfields, nrows, n, pitch, valid, valid_in, precision, &u, &z));
  for (int f = 0; f < nfields; ++f) {
    const int slot = nls_slot(u, f);
    MFFT_TRY(hist_range(lo[f], hi[f], nbins, &z.call.inv[slot]));
    z.call.lo[slot] = lo[f];
  }
  z.call.nbins = nbins;
  const int nb3 = nbins + 3;
  std::vector<int64_t> host((size_t)2 * z.npairs * nb3);
  MFFT_TRY(nlr_stage_run(z, host.size() * sizeof(int64_t), host.data(), 0, nullptr));
  for (int f = 0; f < nfields; ++f)
    for (int k = 0; k < nb3; ++k) out[(size_t)f * nb3 + k] = host[(size_t)nls_slot(u, f) * nb3 + k];
  return 0;
}
int64_t mfft_nlz_hist_groups(int64_t nrows, int64_t n, int precision) { return nlr_stage_groups(Op::Histogram, nrows, n, precision); }

// a, b: (ncomp, nrows, pitch), ncomp 1 or 3, pair p = (a_p, b_p); lo, hi: a_0.., then b_0..
// out[p * cells + sa * (nbb + 3) + sb] = counts of the points of (irfft(a_p row, n), irfft(b_p row, n)) over all rows.
int mfft_nlz_joint_rows(const void* a, const void* b, int ncomp, int64_t nrows, int64_t n, int64_t pitch, int64_t valid, int64_t valid_in,
                        int precision, const double* lo, const double* hi, int nba, int nbb, int64_t* out) {
  if (!b || !out || !lo || !hi) return set_error(MFFT_ERR_INVALID, "bad argument");
  if (ncomp != 1 && ncomp != 3) return set_error(MFFT_ERR_INVALID, "ncomp must be 1 or 3, not %d", ncomp);
  NlFields u;
  NlrArgs z;
  MFFT_TRY(nlr_stage_args(Op::JointHistogram, a, b, 2 * ncomp, nrows, n, pitch, valid, valid_in, precision, &u, &z));
  for (int f = 0; f < 2 * ncomp; ++f) {
    const int slot = nls_slot(u, f);
    MFFT_TRY(joint_range(lo[f], hi[f], slot % 2 ? nbb : nba, &z.call.inv[slot]));
    z.call.lo[slot] = lo[f];
  }
  z.call.nba = nba; z.call.nbb = nbb;
  std::vector<int64_t> host((size_t)ncomp * joint_cells(nba, nbb));      // (the pairs lie in slot order already)
  MFFT_TRY(nlr_stage_run(z, host.size() * sizeof(int64_t), host.data(), 0, nullptr));
  memcpy(out, host.data(), host.size() * sizeof(int64_t));
  return 0;
}
int64_t mfft_nlz_joint_groups(int64_t nrows, int64_t n, int precision) { return nlr_stage_groups(Op::JointHistogram, nrows, n, precision); }

// q = sum_f weights[f] irfft(row of field f, n)^2; out6 = [min, max, S1 .. S4] of q about center over all rows, counts[nbins + 3] its
// histogram over [lo, hi) (null allowed where nbins == 0).
int mfft_nlz_quad_rows(const void* a, const void* b, int nfields, int64_t nrows, int64_t n, int64_t pitch, int64_t valid, int64_t valid_in,
                       int precision, const double* weights, double center, double lo, double hi, int nbins, double* out6, int64_t* counts) {
  if (!out6 || !weights || (nbins > 0 && !counts) || !std::isfinite(center)) return set_error(MFFT_ERR_INVALID, "bad argument");
  NlFields u;
  NlrArgs z;
  MFFT_TRY(nlr_stage_args(Op::Quadratic, a, b, nfields, nrows, n, pitch, valid, valid_in, precision, &u, &z));
  MFFT_TRY(quad_check(weights, nfields, lo, hi, nbins, &z.call.inv[0]));
  for (int f = 0; f < nfields; ++f) z.call.w[nls_slot(u, f)] = weights[f];
  z.call.nbins = nbins; z.call.lo[0] = lo; z.call.center[0] = center;
  double m6[NLS_STATS];
  std::vector<int64_t> host((size_t)nbins + 3);
  MFFT_TRY(nlr_stage_run(z, sizeof m6, m6, host.size() * sizeof(int64_t), host.data()));
  for (int k = 0; k < NLS_STATS; ++k) out6[k] = m6[k];
  for (int k = 0; nbins > 0 && k < nbins + 3; ++k) counts[k] = host[k];
  return 0;
}
int64_t mfft_nlz_quad_groups(int64_t nrows, int64_t n, int precision) { return nlr_stage_groups(Op::Quadratic, nrows, n, precision); }

// U_mpi[p, i, j, k] = Uc_hatT[i, p*Np1 + j, k]   (slab.py:403)
int mfft_slab_pack(const void* uc_hatT, void* u_mpi, int P, int64_t np0, int64_t np1, int64_t nf, int precision) {
  if (!uc_hatT || !u_mpi || P < 1) return set_error(MFFT_ERR_INVALID, "bad argument");
  const size_t es = elem_bytes(precision, true);
  for (int p = 0; p < P; ++p) {
    BoxArgs b;
    b.src = static_cast<const char*>(uc_hatT) + (size_t)(p * np1 * nf) * es;
    b.dst = static_cast<char*>(u_mpi) + (size_t)p * (np0 * np1 * nf) * es;
    b.e0 = np0; b.e1 = 1; b.e2 = np1 * nf; b.s0 = (int64_t)P * np1 * nf; b.d0 = np1 * nf;
    b.elem = (int)es; b.prec = precision;
    MFFT_TRY(launch_box_copy(b, nullptr));
  }
  MFFT_HIP(hipStreamSynchronize(nullptr));
  return 0;
}

// Uc_hatT[i, p*Np1 + j, k] = U_mpi[p, i, j, k]   (cython/maths.pyx:21-31)
int mfft_slab_unpack(const void* u_mpi, void* uc_hatT, int P, int64_t np0, int64_t np1, int64_t nf, int precision) {
  if (!uc_hatT || !u_mpi || P < 1) return set_error(MFFT_ERR_INVALID, "bad argument");
  const size_t es = elem_bytes(precision, true);
  for (int p = 0; p < P; ++p) {
    BoxArgs b;
    b.src = static_cast<const char*>(u_mpi) + (size_t)p * (np0 * np1 * nf) * es;
    b.dst = static_cast<char*>(uc_hatT) + (size_t)(p * np1 * nf) * es;
    b.e0 = np0; b.e1 = 1; b.e2 = np1 * nf; b.s0 = np1 * nf; b.d0 = (int64_t)P * np1 * nf;
    b.elem = (int)es; b.prec = precision;
    MFFT_TRY(launch_box_copy(b, nullptr));
  }
  MFFT_HIP(hipStreamSynchronize(nullptr));
  return 0;
}

int mfft_dealias_filter(void* fu, const uint8_t* mask_dev, size_t count, int precision) {
  if (!fu || !mask_dev) return set_error(MFFT_ERR_INVALID, "null argument");
  MFFT_TRY(launch_mask(fu, mask_dev, count, precision, nullptr));
  MFFT_HIP(hipStreamSynchronize(nullptr));
  return 0;
}

// ---- timers ---------------------------------------------------------------------
struct mfft_timer_s {
  hipEvent_t a = nullptr, b = nullptr;
};
int mfft_timer_create(mfft_timer_t* t) {
  if (!t) return set_error(MFFT_ERR_INVALID, "null argument");
  mfft_timer_s* x = new mfft_timer_s();
  hipError_t e1 = hipEventCreate(&x->a), e2 = hipEventCreate(&x->b);
  if (e1 != hipSuccess || e2 != hipSuccess) {
    delete x;
    return set_error(MFFT_ERR_HIP, "hipEventCreate failed");
  }
  *t = x;
  return 0;
}
int mfft_timer_start(mfft_timer_t t) {
  MFFT_HIP(hipEventRecord(t->a, nullptr));
  return 0;
}
int mfft_timer_stop(mfft_timer_t t, float* ms) {
  MFFT_HIP(hipEventRecord(t->b, nullptr));
  MFFT_HIP(hipEventSynchronize(t->b));
  MFFT_HIP(hipEventElapsedTime(ms, t->a, t->b));
  return 0;
}
int mfft_timer_destroy(mfft_timer_t t) {
  if (t) {
    (void)hipEventDestroy(t->a);
    (void)hipEventDestroy(t->b);
    delete t;
  }
  return 0;
}

}  // extern "C"
