// core.hip -- kernel registry, twiddle cache, launch layer and the small
// data-movement kernels (box copy / mask / scale / synthetic fill).
#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <type_traits>
#include <cstdio>
#include <cstdlib>
#include <map>
#include <mutex>
#include <unordered_map>
#include <tuple>
#include "mfft_internal.h"
#include "fft_nlz.h"
#include "nlz_moments.h"
#include "nlz_hist.h"
#include "nlz_joint.h"
#include "nlz_quad.h"
#include "nlz_incr.h"
#include "nlz_incr_hist.h"
#include "nlz_prof.h"

namespace mfft {

// ---------------------------------------------------------------------------
static thread_local std::string g_err;

int set_error(int code, const char* fmt, ...) {
  char buf[1024];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof buf, fmt, ap);
  va_end(ap);
  g_err = buf;
  return code;
}
const char* last_error() { return g_err.c_str(); }

std::vector<KernelEntry>& kernel_registry() {
  static std::vector<KernelEntry> reg;
  return reg;
}

// The registry is complete once the static initialisers of the kernels_*.hip units have run; lookups go
// through hash maps built on first use (a linear scan of ~2000 entries per launch costs ~0.3 us, visible at 32^3).
constexpr int OP_BITS = 6, BUILD_BITS = 4, FAMILY_BITS = 6;
static_assert(2 * (unsigned)Op::TopFlag <= (1u << OP_BITS) && (unsigned)Op::Band < (unsigned)Op::Limited, "Op does not fit its key field");
static_assert((unsigned)Build::Last < (1u << BUILD_BITS), "Build does not fit its key field");
static_assert((unsigned)FAM_NLZ < (1u << FAMILY_BITS), "Family does not fit its key field");
static uint64_t kernel_key(int family, int n, int prec, int inv, Op op, Build build) {
  uint64_t k = (unsigned)n;
  k = k << FAMILY_BITS | (uint64_t)family;
  k = k << OP_BITS | (uint64_t)op;
  k = k << BUILD_BITS | (uint64_t)build;
  return k << 2 | (uint64_t)(inv << 1 | prec);
}

const KernelEntry* find_kernel(int family, int n, int prec, int inv, Op op, Build build) {
  static std::unordered_map<uint64_t, const KernelEntry*> index;
  static std::once_flag once;
  std::call_once(once, [] {
    for (const KernelEntry& e : kernel_registry()) {
      auto ins = index.emplace(kernel_key(e.family, e.n, e.prec, e.inv, e.op, e.build), &e);
      if (!ins.second) {      // two entries under one key: a registration error, which of them ran would depend on link order
        fprintf(stderr, "mpifft4py_amd: kernel registry holds '%s' and '%s' under one key (family %d, n %d, prec %d, inv %d, op %u, build %u)\n",
                ins.first->second->name, e.name, e.family, e.n, e.prec, e.inv, (unsigned)e.op, (unsigned)e.build);
        abort();
      }
    }
  });
  auto it = index.find(kernel_key(family, n, prec, inv, op, build));
  return it == index.end() ? nullptr : it->second;
}

const KernelEntry* find_chirpz(int family, int n, int prec, int inv) {
  static std::unordered_map<uint64_t, const KernelEntry*> cache;
  static std::mutex mu;
  const uint64_t key = kernel_key(family, n, prec, inv, Op::Plain, Build::Default);
  std::lock_guard<std::mutex> lk(mu);
  auto it = cache.find(key);
  if (it != cache.end()) return it->second;
  const KernelEntry* best = nullptr;
  for (const KernelEntry& e : kernel_registry())
    if (e.family == family && e.prec == prec && e.inv == inv && e.n >= 2 * n - 1 && (!best || e.n < best->n)) best = &e;
  cache.emplace(key, best);
  return best;
}

bool length_supported(int64_t n, bool real_transform) {
  if (n <= 0 || n > (1 << 20)) return false;
  if (real_transform)
    return find_kernel(FAM_R2C, (int)n, MFFT_DOUBLE, 0) != nullptr || find_chirpz(FAM_R2CZ, (int)n, MFFT_DOUBLE, 0) != nullptr ||
           (n % 2 == 0 && n >= 4 && find_chirpz(FAM_R2CZH, (int)(n / 2), MFFT_DOUBLE, 0) != nullptr) || big_length_ok(n);
  return n == 1 || find_kernel(FAM_COL, (int)n, MFFT_DOUBLE, 0) != nullptr ||
         find_chirpz(FAM_COLZ, (int)n, MFFT_DOUBLE, 0) != nullptr || big_length_ok(n);
}
bool radix_plan_exists(int contiguous, int64_t n, int prec) {
  if (n < 2 || n >= 65536) return false;
  return find_kernel(contiguous ? FAM_ROW : FAM_COL, (int)n, prec, 0) != nullptr && find_kernel(contiguous ? FAM_ROW : FAM_COL, (int)n, prec, 1) != nullptr;
}
// 1: a radix plan, 2: the one-workgroup chirp-z kernels, 3: the scratch-buffer fallback (bigfft.hip), 0: none
int length_route(int64_t n, bool real_transform, int prec) {
  if (n <= 0 || n > (1 << 20)) return 0;
  if (real_transform) {
    if (find_kernel(FAM_R2C, (int)n, prec, 0)) return 1;
    if (find_chirpz(FAM_R2CZ, (int)n, prec, 0) || (n % 2 == 0 && n >= 4 && find_chirpz(FAM_R2CZH, (int)(n / 2), prec, 0))) return 2;
  } else {
    if (n == 1 || find_kernel(FAM_COL, (int)n, prec, 0)) return 1;
    if (find_chirpz(FAM_COLZ, (int)n, prec, 0)) return 2;
  }
  return big_length_ok(n) ? 3 : 0;
}

// ---------------------------------------------------------------------------
// per-device caches: inter-pass twiddles per kernel entry, real twiddles per
// (n, prec); kernels with > 64 KiB dynamic LDS get the opt-in attribute once.
// ---------------------------------------------------------------------------
struct DevCache {
  std::map<const KernelEntry*, void*> tw;
  std::map<std::pair<int, int>, void*> rtw;
  std::map<const void*, bool> attr_done;
  std::map<std::tuple<int, int, int>, void*> zchirp, zbhat;            // (n, M, prec) -> chirp, filter of the chirp-z kernels
  std::map<std::pair<int, int>, void*> rt3;                            // (L, prec) -> twiddles of the pruned nonlinear z stage
};
static std::mutex g_cache_mu;
static std::map<int, DevCache> g_cache;

template <class F> static auto by_prec(int prec, F f) { return prec == MFFT_DOUBLE ? f(double{}) : f(float{}); }
template <class V> static std::vector<char> bytes_of(const V& v) {
  const char* p = reinterpret_cast<const char*>(v.data());
  return std::vector<char>(p, p + v.size() * sizeof(v[0]));
}
// One table of the current device's cache (a member of DevCache): built on the host and uploaded the first time its key is
// asked for, remembered after.  `before` runs under the same lock on every call.
template <class Key, class Fill, class Before>
static int device_table(std::map<Key, void*> DevCache::*table, Key key, Fill fill, void** out, Before before) {
  int dev = 0;
  MFFT_HIP(hipGetDevice(&dev));
  std::lock_guard<std::mutex> lk(g_cache_mu);
  DevCache& c = g_cache[dev];
  MFFT_TRY(before(c));
  auto& m = c.*table;
  auto it = m.find(key);
  if (it == m.end()) {
    const std::vector<char> host = fill();
    void* d = nullptr;
    MFFT_HIP(hipMalloc(&d, host.size()));
    MFFT_HIP(hipMemcpy(d, host.data(), host.size(), hipMemcpyHostToDevice));
    it = m.emplace(key, d).first;
  }
  *out = it->second;
  return 0;
}
template <class Key, class Fill>
static int device_table(std::map<Key, void*> DevCache::*table, Key key, Fill fill, void** out) {
  return device_table(table, key, fill, out, [](DevCache&) { return 0; });
}

static int prepare_kernel(const KernelEntry* e, void** tw_out) {
  auto fill = [&] {
    std::vector<char> host((size_t)e->tw_count * elem_bytes(e->prec, true));
    e->build_tw(host.data());
    return host;
  };
  return device_table(&DevCache::tw, e, fill, tw_out, [&](DevCache& c) {
    if (!c.attr_done[e->func]) {
      if (e->lds_bytes > 65536)
        MFFT_HIP(hipFuncSetAttribute(e->func, hipFuncAttributeMaxDynamicSharedMemorySize, e->lds_bytes));
      c.attr_done[e->func] = true;
    }
    return 0;
  });
}

static int real_twiddles(int n, int prec, void** out) {
  return device_table(&DevCache::rtw, std::make_pair(n, prec),
                      [&] { return by_prec(prec, [&](auto t) { return bytes_of(build_real_twiddles<decltype(t)>(n)); }); }, out);
}

static int nlz3_twiddles(int L, int prec, void** out) {
  return device_table(&DevCache::rt3, std::make_pair(L, prec),
                      [&] { return by_prec(prec, [&](auto t) { return bytes_of(build_nlz3_twiddles<decltype(t)>(L)); }); }, out);
}

// chirp-z tables of logical length n on convolution length M (fft_chirpz.h)
static int chirpz_tables(int n, int M, int prec, void** chirp, void** bhat) {
  const auto key = std::make_tuple(n, M, prec);
  MFFT_TRY(device_table(&DevCache::zchirp, key, [&] { return by_prec(prec, [&](auto t) { return bytes_of(build_chirp<decltype(t)>(n)); }); }, chirp));
  return device_table(&DevCache::zbhat, key, [&] { return by_prec(prec, [&](auto t) { return bytes_of(build_chirp_filter<decltype(t)>(n, M)); }); }, bhat);
}

static RowMap to_map(const RowSpec& r, int n) { return make_rowmap(r.hi, r.lo, r.split, n); }

// ---------------------------------------------------------------------------
template <typename T, class PT = ColParams<T>>
static int launch_col_t(const KernelEntry* e, const ColArgs& a, void* tw, hipStream_t s, const void* chirp = nullptr,
                        const void* bhat = nullptr) {
  PT P;
  if constexpr (!std::is_same<PT, ColParams<T>>::value) {
    P.chirp = static_cast<const cx<T>*>(chirp);
    P.bhat = static_cast<const cx<T>*>(bhat);
    P.n = a.n;
  }
  P.in = static_cast<const cx<T>*>(a.in);
  P.out = static_cast<cx<T>*>(a.out);
  P.tw = static_cast<const cx<T>*>(tw);
  P.in_outer = a.in_outer;
  P.out_outer = a.out_outer;
  P.in_map = to_map(a.in_rows, a.n);
  P.out_map = to_map(a.out_rows, a.n);
  P.ncols = (int)a.ncols;
  P.ntile_c = (int)((a.ncols + e->tile - 1) / e->tile);
  P.nouter = (int)a.nouter;
  static const int remap_env = getenv("MFFT_REMAP") ? atoi(getenv("MFFT_REMAP")) : -1;      // experiments: 0 none, 1 XCD-aware, 2 skewed
  P.remap = remap_env >= 0 ? remap_env : a.remap;
  P.fold = a.fold ? 1 : 0;
  P.scale = (T)a.scale;
  P.nblocks = 0;
  P.mask = a.mask;
  P.b_row_lo = a.band.row_lo; P.b_row_hi = a.band.row_hi; P.b_coff = a.band.c_off; P.b_cper = a.band.c_per;
  P.b_clim = a.band.c_lim; P.b_goff = a.band.g_off; P.b_gstep = a.band.g_step; P.b_glo = a.band.g_lo; P.b_ghi = a.band.g_hi;
  P.tile_list = a.band.on ? a.band.tile_list : nullptr;
  P.ntiles_listed = a.band.ntiles_listed;
  P.b_gzero = a.band.on ? a.band.g_zero : 0;
  if constexpr (std::is_same<PT, ColParams<T>>::value) {
    P.in_wrap = (int)a.in_wrap;
    P.in_wrap_gap = (int)a.in_wrap_gap;
  } else {
    if (a.in_wrap > 0) return set_error(MFFT_ERR_UNSUPPORTED, "wrapped input columns need a radix kernel (length %d has none)", a.n);
  }
  const int64_t grid = P.tile_list ? (int64_t)P.ntiles_listed : (int64_t)P.ntile_c * a.nouter * (e->grid_mult > 1 ? e->grid_mult : 1);
  if (grid <= 0) return 0;
  if (grid > 0x7FFFFFFF) return set_error(MFFT_ERR_UNSUPPORTED, "grid too large (%lld tiles)", (long long)grid);
  e->launch(&P, (int)grid, s);
  MFFT_HIP(hipGetLastError());
  return 0;
}

#ifndef MFFT_COL3S_DEFAULT
#define MFFT_COL3S_DEFAULT 1
#endif
// Which kernel runs the strided pass `a` (2 <= n < 65536): a radix entry, a chirp-z entry (family FAM_COLZ), or none where the
// scratch-buffer fallback of bigfft.hip serves the length.
static int select_col(const ColArgs& a, const KernelEntry** out) {
  const int inv = a.inverse ? 1 : 0;
  // non-temporal variant only when every row segment of the tile is a whole, private L2 line
  const int64_t per_line = 128 / (int64_t)elem_bytes(a.prec, true);
  auto aligned = [&](const void* p, int64_t outer, const RowSpec& r) {
    return ((uintptr_t)p % 128 == 0) && outer % per_line == 0 && r.lo % per_line == 0 && r.hi % per_line == 0;
  };
  // Out of place the NT variant is always ahead (1024^3 x pass 3.70 -> 3.63 ms at one workgroup per CU, 3.24 -> 3.19 ms at
  // two); in place only the kernels that run two workgroups per CU gain from it (3.42 -> 3.35 ms; one per CU: 3.57 -> 3.84 ms)
  static const int nt_mode = getenv("MFFT_NT") ? atoi(getenv("MFFT_NT")) : 1;   // 0 never, 1 by that rule, 2 always
  auto find_nt = [&](Op op) {
    const KernelEntry* k = find_kernel(FAM_COL, a.n, a.prec, inv, op, Build::NonTemporal);
    return k && a.in == a.out && !(k->nt_inplace || nt_mode == 2) ? nullptr : k;
  };
  const bool nt_ok = a.allow_nt && nt_mode > 0 && a.pad == Op::Plain && aligned(a.in, a.in_outer, a.in_rows) && aligned(a.out, a.out_outer, a.out_rows);
  const KernelEntry* ent = nt_ok ? find_nt(Op::Plain) : nullptr;
  const KernelEntry* e = nullptr;
  if (a.mask || a.band.on) {
    const Op op = a.band.on ? Op::Band : Op::MaskLoad;
    if (!a.inverse || a.pad != Op::Plain || (a.mask && a.band.on)) return set_error(MFFT_ERR_INVALID, "a dealias mask is applied by inverse, un-padded transforms only");
    if (ent) e = find_nt(op);      // the same alignment rule picks the non-temporal build
    if (!e) e = find_kernel(FAM_COL, a.n, a.prec, 1, op);
    if (!e) return set_error(MFFT_ERR_UNSUPPORTED, "no masked-load kernel for length %d", a.n);
    ent = nullptr;
  }
  if (a.pad != Op::Plain) {
    if ((a.pad == Op::PadLoad) != a.inverse) return set_error(MFFT_ERR_INVALID, "pad-on-load is an inverse-transform mode, truncate-on-store a forward one");
    e = find_kernel(FAM_COL, a.n, a.prec, inv, a.pad);
    if (!e) return set_error(MFFT_ERR_UNSUPPORTED, "no fused 3/2-rule kernel for length %d", a.n);
  }
  // N = 3 L as three sub-transforms per workgroup (fft_col3.h; Build::Col3), plain and 3/2-rule passes.  Measured at
  // 1536 (profiles/r04_col3_1536.txt): even with the ColFft plan in double precision (1536^3 pair 75.1 - 81.0 against 76.9 -
  // 78.1 ms, 3/2-rule pair of 1024^3 45.5 - 47.7 against 47.9 - 48.1), ahead in single precision on the x passes (rows a whole
  // plane apart: 9.0 -> 7.3 ms inverse, 7.5 -> 6.8 forward) and behind on the y passes (6.9 -> 7.7 - 8.1).  Default: single
  // precision, passes without an outer batch (the x passes); MFFT_COL3=1 always, MFFT_COL3=0 never.
  static const int col3_mode = getenv("MFFT_COL3") ? atoi(getenv("MFFT_COL3")) : -1;
  const bool col3_on = col3_mode > 0 || (col3_mode < 0 && a.prec == MFFT_SINGLE && (a.nouter == 1 || a.thirds > 0));
  if (col3_on && !a.mask && !a.band.on) {
    const KernelEntry* e3 = nullptr;
    if (nt_ok) e3 = find_kernel(FAM_COL, a.n, a.prec, inv, Op::Plain, Build::Col3NT);      // same alignment rule, NT build
    if (!e3) e3 = find_kernel(FAM_COL, a.n, a.prec, inv, a.pad, Build::Col3);
    if (e3) e = e3;
  }
  // The pad-on-load inverse with one third of a tile's transform per workgroup (fft_col3.h ColFft3S, Build::Col3Thirds): out of
  // place only (its passes are).  3/2-rule ifftn + fftn pair of 1024^3 (profiles/r04_col3s_ab.txt): double precision x pass
  // 5.31 -> 5.16 ms, y pass 8.47 -> 9.17 (not taken); single precision x 2.99 -> 2.54, y 4.98 -> 4.35.  Default on; MFFT_COL3S=0 never.
  static const int col3s_mode = getenv("MFFT_COL3S") ? atoi(getenv("MFFT_COL3S")) : MFFT_COL3S_DEFAULT;
  // double precision: the passes without an outer batch only (y pass 8.4 -> 9.1 ms with it); MFFT_COL3S=2: every pass
  if (col3s_mode > 0 && a.thirds != 0 && a.pad == Op::PadLoad && a.inverse && a.in != a.out && !a.mask && !a.band.on &&
      (col3s_mode > 1 || a.thirds > 0 || a.prec == MFFT_SINGLE || a.nouter == 1)) {
    if (const KernelEntry* es = find_kernel(FAM_COL, a.n, a.prec, 1, Op::PadLoad, Build::Col3Thirds)) e = es;
  }
  if (!e && ent) e = ent;
  if (!e) e = find_kernel(FAM_COL, a.n, a.prec, inv);
  // Round 5: the y-pass builds (registry.h register_col_ytile, Build::YTile: 64-byte tiles, LDS twiddles, two workgroups per
  // CU) where the rows of a tile lie at most 64 KB apart on both sides -- the y passes of every decomposition; the x passes,
  // rows a plane apart, lose with them (1440 / 1536 fp64: y 12.95 -> 9.62 / 13.74 -> 11.55 ms, x 12.85 -> 14.49 / 12.56 -> 14.41).  Not for the
  // pruned 2/3-rule passes (their tile lists are built for the width of the general kernel).  MFFT_YTILE=0 never, 2 always.
  static const int ytile_mode = getenv("MFFT_YTILE") ? atoi(getenv("MFFT_YTILE")) : 1;
  if (ytile_mode > 0 && e && !a.band.on && (e->build == Build::Default || e->build == Build::NonTemporal) &&
      (e->op == Op::Plain || e->op == Op::PadLoad || e->op == Op::TruncStore || e->op == Op::MaskLoad)) {
    const int64_t es = (int64_t)elem_bytes(a.prec, true);
    const bool near_rows = std::llabs(a.in_rows.lo) * es <= 65536 && std::llabs(a.out_rows.lo) * es <= 65536;
    if (near_rows || ytile_mode > 1)
      if (const KernelEntry* ey = find_kernel(FAM_COL, a.n, a.prec, inv, e->op, Build::YTile)) e = ey;
  }
  if (!e) {   // no radix plan for this length: chirp-z on the next compiled length >= 2n-1
    e = find_chirpz(FAM_COLZ, a.n, a.prec, inv);
    if (!e && !big_length_ok(a.n)) return set_error(MFFT_ERR_UNSUPPORTED, "no kernel for a complex transform of length %d", a.n);
  }
  *out = e;
  return 0;
}

int launch_col(const ColArgs& a, hipStream_t s) {
  if (a.n == 1) {   // a length-1 transform is a (scaled) copy of its single row
    if (a.in == a.out && a.in_outer == a.out_outer && a.scale == 1.0) return 0;
    BoxArgs b;
    b.src = a.in; b.dst = a.out; b.e0 = a.nouter; b.e1 = 1; b.e2 = a.ncols; b.s0 = a.in_outer; b.d0 = a.out_outer;
    b.elem = (int)elem_bytes(a.prec, true); b.scale = a.scale; b.prec = a.prec;
    return launch_box_copy(b, s);
  }
  if (a.n >= 65536)      // beyond the radix kernels' 16-bit row arithmetic: the scratch-buffer fallback or nothing
    return big_length_ok(a.n) ? big_col(a, s) : set_error(MFFT_ERR_UNSUPPORTED, "transform length %d too large", a.n);
  if (a.ncols >= (1ll << 31)) return set_error(MFFT_ERR_UNSUPPORTED, "too many columns");
  const KernelEntry* e = nullptr;
  MFFT_TRY(select_col(a, &e));
  if (!e) return big_col(a, s);
  void *tw = nullptr, *chirp = nullptr, *bhat = nullptr;
  MFFT_TRY(prepare_kernel(e, &tw));
  if (e->family == FAM_COLZ) {
    MFFT_TRY(chirpz_tables(a.n, e->n, a.prec, &chirp, &bhat));
    return by_prec(a.prec, [&](auto t) { return launch_col_t<decltype(t), ColParamsZ<decltype(t)>>(e, a, tw, s, chirp, bhat); });
  }
  return by_prec(a.prec, [&](auto t) { return launch_col_t<decltype(t)>(e, a, tw, s); });
}

// ---- contiguous-axis kernels: shared pieces of their parameter blocks and launches ----
template <class P>
static void set_zsplit(P& p, const ZSplitArgs& zs) {
  p.zs = zs.nchunk ? make_zsplit(zs.q, zs.nchunk, zs.last_len, zs.rows_total, zs.pitch, zs.last_pitch) : ZSplit{1, 1, 0, 0, 0, 1, 0};
  p.row0 = zs.row0;
}
template <class P>
static int launch_rows(const KernelEntry* e, const P& p, int64_t nrows, int rows_per_wg, hipStream_t s) {
  const int64_t grid = (nrows + rows_per_wg - 1) / rows_per_wg;
  if (grid <= 0) return 0;
  if (grid > 0x7FFFFFFF) return set_error(MFFT_ERR_UNSUPPORTED, "grid too large");
  e->launch(&p, (int)grid, s);
  MFFT_HIP(hipGetLastError());
  return 0;
}

template <typename T, class PT = RowParams<T>>
static int launch_row_t(const KernelEntry* e, const RowArgs& a, void* tw, hipStream_t s, const void* chirp = nullptr,
                        const void* bhat = nullptr) {
  PT P;
  if constexpr (!std::is_same<PT, RowParams<T>>::value) {
    P.chirp = static_cast<const cx<T>*>(chirp);
    P.bhat = static_cast<const cx<T>*>(bhat);
    P.n = a.n;
  }
  P.in = static_cast<const cx<T>*>(a.in);
  P.out = static_cast<cx<T>*>(a.out);
  P.tw = static_cast<const cx<T>*>(tw);
  P.in_stride = a.in_stride;
  P.out_stride = a.out_stride;
  P.nrows = a.nrows;
  P.scale = (T)a.scale;
  if constexpr (std::is_same<PT, RowParams<T>>::value) set_zsplit(P, a.zs);
  return launch_rows(e, P, a.nrows, e->tile, s);
}

int col_tile_width(int64_t n, int prec, bool inverse, Op op) {
  const KernelEntry* e = find_kernel(FAM_COL, (int)n, prec, inverse ? 1 : 0, op);
  return e ? e->tile : 0;
}
bool c2r_limit_supported(int64_t n, int prec) { return n >= 4 && n < 65536 && find_kernel(FAM_C2R, (int)n, prec, 1, Op::Limited) != nullptr; }
bool band_fusable(int64_t n, int prec) { return n >= 2 && n < 65536 && find_kernel(FAM_COL, (int)n, prec, 1, Op::Band) != nullptr; }
bool mask_fusable(int64_t n, int prec) { return n >= 2 && n < 65536 && find_kernel(FAM_COL, (int)n, prec, 1, Op::MaskLoad) != nullptr; }

bool zsplit_limit_supported(int64_t n, int prec) {
  return n >= 2 && n < 65536 && find_kernel(FAM_R2C, (int)n, prec, 0, Op::Limited | Op::ZChunk) && find_kernel(FAM_C2R, (int)n, prec, 1, Op::Limited | Op::ZChunk);
}

bool zsplit_supported(int64_t n, int prec, bool real_transform) {
  if (n < 2 || n > 65536) return false;
  if (real_transform) return find_kernel(FAM_R2C, (int)n, prec, 0, Op::ZChunk) && find_kernel(FAM_C2R, (int)n, prec, 1, Op::ZChunk);
  return find_kernel(FAM_ROW, (int)n, prec, 0, Op::ZChunk) && find_kernel(FAM_ROW, (int)n, prec, 1, Op::ZChunk);
}

int launch_row(const RowArgs& a, hipStream_t s) {
  const int inv = a.inverse ? 1 : 0;
  const KernelEntry* e = find_kernel(FAM_ROW, a.n, a.prec, inv, a.zs.nchunk ? Op::ZChunk : Op::Plain);
  if (!e && a.zs.nchunk) return set_error(MFFT_ERR_UNSUPPORTED, "no z-chunked row kernel of length %d", a.n);
  void *tw = nullptr, *chirp = nullptr, *bhat = nullptr;
  if (!e) {
    e = find_chirpz(FAM_ROWZ, a.n, a.prec, inv);
    if (!e && big_length_ok(a.n)) return big_row(a, s);
    if (!e) return set_error(MFFT_ERR_UNSUPPORTED, "no kernel for a complex transform of length %d", a.n);
    MFFT_TRY(prepare_kernel(e, &tw));
    MFFT_TRY(chirpz_tables(a.n, e->n, a.prec, &chirp, &bhat));
    return by_prec(a.prec, [&](auto t) { return launch_row_t<decltype(t), RowParamsZ<decltype(t)>>(e, a, tw, s, chirp, bhat); });
  }
  MFFT_TRY(prepare_kernel(e, &tw));
  return by_prec(a.prec, [&](auto t) { return launch_row_t<decltype(t)>(e, a, tw, s); });
}

template <typename T, class PT = RealParams<T>>
static int launch_real_t(const KernelEntry* e, const RealArgs& a, void* tw, void* rtw, hipStream_t s,
                         const void* chirp = nullptr, const void* bhat = nullptr) {
  PT P;
  if constexpr (!std::is_same<PT, RealParams<T>>::value) {
    P.chirp = static_cast<const cx<T>*>(chirp);
    P.bhat = static_cast<const cx<T>*>(bhat);
    P.n = a.n;
  }
  P.in = a.in;
  P.out = a.out;
  P.tw = static_cast<const cx<T>*>(tw);
  P.rtw = static_cast<const cx<T>*>(rtw);
  P.in_stride = a.in_stride;
  P.out_stride = a.out_stride;
  P.nrows = a.nrows;
  P.valid = a.valid > 0 ? a.valid : a.n / 2 + 1;
  P.scale = (T)a.scale;
  if constexpr (std::is_same<PT, RealParams<T>>::value) set_zsplit(P, a.zs);
  return launch_rows(e, P, a.nrows, e->tile, s);
}
// pair-row kernels (Op::PairRows): a workgroup holds tile / 2 of the (n0 / 2 + 1) * n1 pair slots (fft_kernels.h pair_row)
template <typename T>
static int launch_pair_t(const KernelEntry* e, const RealArgs& a, int64_t real_stride, void* tw, void* rtw, hipStream_t s) {
  RealPairParams<T> P;
  P.in = a.in;
  P.out = a.out;
  P.tw = static_cast<const cx<T>*>(tw);
  P.rtw = static_cast<const cx<T>*>(rtw);
  P.in_stride = a.in_stride;
  P.out_stride = a.out_stride;
  P.nrows = (int64_t)(a.pair_n0 / 2 + 1) * a.pair_n1;
  P.valid = a.n / 2 + 1;
  P.scale = (T)a.scale;
  set_zsplit(P, a.zs);
  P.pn0 = a.pair_n0;
  P.pn1 = a.pair_n1;
  P.p_rplane = a.pair_rplane;
  P.p_cplane = a.pair_cplane;
  P.p_ymap = make_rowmap(a.pair_rblock, real_stride, a.pair_yblock, a.pair_n1);
  P.p_tile = a.pair_tile;
  P.p_tile_xfast = a.pair_tile_xfast ? 1 : 0;
  return launch_rows(e, P, P.nrows, e->tile / 2, s);
}

// c2r kernels with the mirrors through LDS (registry.h c2r_mlds_candidate: built where they were measured ahead): taken where
// they exist; MFFT_C2R_MLDS=0: never
static int c2r_mlds_mode() {
  static const int m = getenv("MFFT_C2R_MLDS") ? atoi(getenv("MFFT_C2R_MLDS")) : 1;
  return m;
}
// MFFT_C2R_MLDS: 0 never, 1 (default) where measured ahead, 2 wherever a build exists, 3 the column-limited kernels of the 3/2-rule
// only.  profiles/r06_c2r_mlds.txt: the 12-values plans of 288 ... 3456 complex points that no shuffle serves gain 1 - 15 % on plain
// rows and 15 - 47 % on column-limited ones (3/2-rule pair of 576^3 fp64: bwd_z 3.08 -> 1.65 ms, of 768^3: 6.60 -> 3.91); rows of more
// than a wave's threads: real 6144 / 8192 +4 ... +15 %, real 4096 in double precision only (+10 %; single -5 %), real 3072 only
// column-limited in single precision (+5 %; plain -2 ... -9 %).  The 30- / 42-values plans have no such build (registers: -2.2 x).
static bool c2r_mlds_take(int n, int prec, bool limited) {
  const int m = c2r_mlds_mode();
  if (m <= 0) return false;
  if (m == 2) return true;
  if (m == 3) return limited;
  const int c = n / 2;
  if (c == 1000 || c == 2000) return prec == MFFT_SINGLE;      // the 20-values plans: 400 / 500 / 800 gain in both precisions
  // (800^3 bwd_z 1.75 -> 1.50 ms, under the 2/3-rule 1.65 -> 1.32; 1000^3 3.28 -> 3.07 / 3.45 -> 2.99; 1600^3 13.7 -> 13.3 / 13.2 -> 12.2),
  // real 2000 / 4000 in single precision only (double: -6 ... -11 %)
  if (c == 1536) return limited && prec == MFFT_SINGLE;
  if (c == 2048) return !limited && prec == MFFT_DOUBLE;
  return true;
}
// Which kernel runs the real transform `a`: a radix entry of family `fam`, an entry of one of the chirp-z families, or none
// where the scratch-buffer fallback of bigfft.hip serves the length.
static int select_real(int fam, const RealArgs& a, const KernelEntry** out) {
  // column-limited (3/2-rule: only the first `valid` of the n/2+1 bins exist; z-chunked, those are what is chunked)
  const bool limited = a.valid > 0 && a.valid < a.n / 2 + 1;
  const Op op = (limited ? Op::Limited : Op::Plain) | (a.zs.nchunk ? Op::ZChunk : Op::Plain);
  const KernelEntry* e = find_kernel(fam, a.n, a.prec, fam == FAM_C2R ? 1 : 0, op);
  if (fam == FAM_C2R && c2r_mlds_take(a.n, a.prec, limited))
    if (const KernelEntry* em = find_kernel(fam, a.n, a.prec, 1, op, Build::LdsMirrors)) e = em;
  // the radix kernels read a real row as (n/2) complex values: rows must stay 2-element aligned
  const int64_t real_stride = fam == FAM_R2C ? a.in_stride : a.out_stride;
  if (a.zs.nchunk && (!e || real_stride % 2 != 0)) return set_error(MFFT_ERR_UNSUPPORTED, "no z-chunked real kernel of length %d", a.n);
  if (!e && limited) return set_error(MFFT_ERR_UNSUPPORTED, "no column-limited real kernel of length %d", a.n);
  if (!e || (real_stride % 2 != 0 && !limited)) {   // no radix plan (or an odd pitch): chirp-z on the real row
    const bool r2c = fam == FAM_R2C;
    // even length and pitch: n/2 complex values + split pass (half the convolution length); else full length
    const bool half = a.n % 2 == 0 && a.n >= 4 && real_stride % 2 == 0;
    e = find_chirpz(half ? (r2c ? FAM_R2CZH : FAM_C2RZH) : (r2c ? FAM_R2CZ : FAM_C2RZ), half ? a.n / 2 : a.n, a.prec, r2c ? 0 : 1);
    if (!e && !big_length_ok(a.n)) return set_error(MFFT_ERR_UNSUPPORTED, "no kernel for a real transform of length %d", a.n);
  } else if (real_stride % 2 != 0) {
    return set_error(MFFT_ERR_UNSUPPORTED, "real row stride %lld must be even", (long long)real_stride);
  }
  *out = e;
  return 0;
}
bool pair_rows_supported(int64_t n, int prec) {
  return n >= 2 && n < 65536 && find_kernel(FAM_R2C, (int)n, prec, 0, Op::PairRows) && find_kernel(FAM_C2R, (int)n, prec, 1, Op::PairRows);
}
static int launch_real(int fam, const RealArgs& a, hipStream_t s) {
  const KernelEntry* e = nullptr;
  if (a.pair_n0 > 0) {
    e = find_kernel(fam, a.n, a.prec, fam == FAM_C2R ? 1 : 0, Op::PairRows);
    const int64_t real_stride = fam == FAM_R2C ? a.in_stride : a.out_stride;
    const bool blocked = a.pair_yblock > 0 && a.pair_yblock < a.pair_n1;      // (its fastdiv: rows and block below 2^16)
    if (!e || a.zs.nchunk || a.valid > 0 || real_stride % 2 != 0 || a.pair_rplane % 2 != 0 ||
        a.nrows != (int64_t)a.pair_n0 * a.pair_n1 || a.nrows >= (int64_t)1 << 31 ||
        a.pair_tile < 0 || a.pair_tile > 32768 || (int64_t)a.pair_tile * a.pair_n1 >= (int64_t)1 << 31 ||
        (blocked && (a.pair_n1 >= 65536 || a.pair_n1 % a.pair_yblock != 0 || a.pair_rblock % 2 != 0)))
      return set_error(MFFT_ERR_UNSUPPORTED, "no pair-row real kernel of length %d for this layout", a.n);
    void *tw = nullptr, *rtw = nullptr;
    MFFT_TRY(prepare_kernel(e, &tw));
    MFFT_TRY(real_twiddles(a.n, a.prec, &rtw));
    return by_prec(a.prec, [&](auto t) { return launch_pair_t<decltype(t)>(e, a, real_stride, tw, rtw, s); });
  }
  MFFT_TRY(select_real(fam, a, &e));
  if (!e) return big_real(fam == FAM_C2R, a, s);
  void *tw = nullptr, *rtw = nullptr, *chirp = nullptr, *bhat = nullptr;
  MFFT_TRY(prepare_kernel(e, &tw));
  if (e->family != fam) {
    const bool half = e->family == FAM_R2CZH || e->family == FAM_C2RZH;
    MFFT_TRY(chirpz_tables(half ? a.n / 2 : a.n, e->n, a.prec, &chirp, &bhat));
    if (half) MFFT_TRY(real_twiddles(a.n, a.prec, &rtw));
    return by_prec(a.prec, [&](auto t) { return launch_real_t<decltype(t), RealParamsZ<decltype(t)>>(e, a, tw, rtw, s, chirp, bhat); });
  }
  MFFT_TRY(real_twiddles(a.n, a.prec, &rtw));
  return by_prec(a.prec, [&](auto t) { return launch_real_t<decltype(t)>(e, a, tw, rtw, s); });
}

int launch_r2c(const RealArgs& a, hipStream_t s) { return launch_real(FAM_R2C, a, s); }
int launch_c2r(const RealArgs& a, hipStream_t s) { return launch_real(FAM_C2R, a, s); }

// fused nonlinear z stage (fft_nlz.h): out_f = rfft((irfft(a) x irfft(b))_f) along the contiguous axis, row by row
// the kernel of one product in one build; a z row has 2 <= n < 65536 (no kernel exists outside that), and the table of
// products (mfft_internal.h) says which builds a product has
static const KernelEntry* find_nlz(int64_t n, int prec, Op product, Build build = Build::Default) {
  const NlProduct& q = nl_product(product);
  if (n < 2 || n >= 65536 || (build == Build::AbsMax && !q.absmax) || (build == Build::Nlz3 && !q.nlz3)) return nullptr;
  return find_kernel(FAM_NLZ, (int)n, prec, 0, product, build);
}
bool nlz_supported(int64_t n, int prec, Op product, bool absmax) {
  if (absmax) return find_nlz(n, prec, product, Build::AbsMax) != nullptr;
  return find_nlz(n, prec, product) != nullptr || find_nlz(n, prec, product, Build::Nlz3) != nullptr;
}
// waves of the Build::AbsMax launch over nrows rows = groups of NLM_SLOTS values it writes to NlzArgs::part (0: no such kernel)
int64_t nlz_absmax_waves(int64_t n, int prec, Op product, int64_t nrows) {
  const KernelEntry* e = find_nlz(n, prec, product, Build::AbsMax);
  if (!e || nrows < 1) return 0;
  return (nrows + 2 * e->tile - 1) / (2 * e->tile) * ((e->threads + 63) / 64);
}
template <typename T, class PT = NlzParams<T>>
static int launch_nlz_t(const KernelEntry* e, const NlzArgs& a, void* tw, void* rt3, hipStream_t s) {
  PT P;
  if constexpr (std::is_same<PT, NlmParams<T>>::value) P.part = static_cast<T*>(a.part);
  if constexpr (std::is_same<PT, NlcParams<T>>::value) {
    for (int f = 0; f < 3; ++f) P.c[f] = static_cast<const cx<T>*>(a.c[f]);
    P.outs = static_cast<cx<T>*>(a.out[3]);
  }
  if constexpr (std::is_same<PT, NloParams<T>>::value)
    for (int c = 0; c < 9; ++c) P.out9[c] = static_cast<cx<T>*>(a.out[c]);
  P.rt3 = static_cast<const cx<T>*>(rt3);
  for (int f = 0; f < 3; ++f) {
    P.a[f] = static_cast<const cx<T>*>(a.a[f]);
    P.b[f] = static_cast<const cx<T>*>(a.b[f]);
    P.out[f] = static_cast<cx<T>*>(a.out[f]);
  }
  P.tw = static_cast<const cx<T>*>(tw);
  P.in_stride = a.in_stride;
  P.out_stride = a.out_stride;
  P.nrows = a.nrows;
  P.valid = a.valid > 0 && a.valid < a.n / 2 + 1 ? a.valid : a.n / 2 + 1;
  P.valid_in = a.valid_in > 0 && a.valid_in < P.valid ? a.valid_in : P.valid;
  P.scale = (T)a.scale;
  return launch_rows(e, P, a.nrows, 2 * e->tile, s);      // a thread group works through a PAIR of rows
}
int launch_nlz(const NlzArgs& a, hipStream_t s) {
  const NlProduct& q = nl_product(a.product);
  // a.part: Build::AbsMax, the same rows and the partial maxima of the six real fields
  const KernelEntry* e = find_nlz(a.n, a.prec, a.product, a.part ? Build::AbsMax : Build::Default);
  // 3/2-rule rows (n = 3 L with the L + 1 bins of the un-padded mesh) also have the pruned kernel (fft_nlz.h Nlz3Fft: three
  // sub-transforms of length L in three thread groups, a third of the registers).  Measured EVEN with NlzFft at 768 (1.36 ms per
  // 73,728 rows both) and behind at 1536 (1.80 - 1.91 against 1.59 ms per 36,864 rows): profiles/r06_nlz_variants.txt -- its
  // staging and combination cost what the skipped radix-3 pass saves.  MFFT_NLZ3=1 takes it; where NlzFft has no plan it runs anyway.
  // (Nlz3Fft has the cross product only and no maxima: MFFT_NLZ3 touches neither the other products nor a statistics call)
  static const int nlz3_on = getenv("MFFT_NLZ3") ? atoi(getenv("MFFT_NLZ3")) : 0;
  const bool rows3 = a.n % 3 == 0 && a.valid == a.n / 3 + 1;
  if ((nlz3_on || !e) && rows3 && !a.part)
    if (const KernelEntry* e3 = find_nlz(a.n, a.prec, a.product, Build::Nlz3)) e = e3;
  if (!e) return set_error(MFFT_ERR_UNSUPPORTED, "no fused nonlinear z-stage kernel of length %d%s (%s product)", a.n, a.part ? " with maxima" : "", q.name);
  for (int f = 0; f < 3; ++f)
    if (!a.a[f] || !a.b[f] || (q.nin > 6 && !a.c[f])) return set_error(MFFT_ERR_INVALID, "null argument");
  for (int f = 0; f < q.nout; ++f)
    if (!a.out[f]) return set_error(MFFT_ERR_INVALID, "null argument");
  void *tw = nullptr, *rt3 = nullptr;
  MFFT_TRY(prepare_kernel(e, &tw));
  if (e->build == Build::Nlz3) MFFT_TRY(nlz3_twiddles(a.n / 3, a.prec, &rt3));
  return by_prec(a.prec, [&](auto t) {
    using T = decltype(t);
    if (a.part) return launch_nlz_t<T, NlmParams<T>>(e, a, tw, rt3, s);
    if (q.nin > 6) return launch_nlz_t<T, NlcParams<T>>(e, a, tw, rt3, s);      // (a third field in, a fourth row out)
    if (q.op == Op::Outer) return launch_nlz_t<T, NloParams<T>>(e, a, tw, rt3, s);      // (nine rows out)
    return launch_nlz_t<T>(e, a, tw, rt3, s);
  });
}

// The stages that end in a reduction (the body of NlzMoments, NlzHist, NlzJoint, NlzQuad, NlzIncr, NlzIncrHist, NlzProf, a header each, nlz_*.h: the table entries with
// nout == 0; NlrArgs of mfft_internal.h).  Their grid does not follow the rows: the workgroups that are resident at once, CUs x
// min(what the runtime says fits, NLS_WG_PER_CU), asked once per device and kernel, and never more than there are pairs of rows to
// start on.
constexpr int NLS_WG_PER_CU = 4;
static int nls_resident(const KernelEntry* e, int* cap) {
  struct Key { int dev; const void* fn; int cap; };
  static std::mutex mu;
  static std::vector<Key> known;
  int dev = 0;
  MFFT_HIP(hipGetDevice(&dev));
  std::lock_guard<std::mutex> lock(mu);
  for (const Key& k : known)
    if (k.dev == dev && k.fn == e->func) { *cap = k.cap; return 0; }
  int ncu = 0, occ = 0;
  MFFT_HIP(hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, dev));
  MFFT_HIP(hipOccupancyMaxActiveBlocksPerMultiprocessor(&occ, e->func, e->threads, (size_t)e->lds_bytes));
  if (occ < 1 || ncu < 1) return set_error(MFFT_ERR_INTERNAL, "%s: no resident workgroup (%d CUs, %d per CU)", e->name, ncu, occ);
  *cap = ncu * (occ < NLS_WG_PER_CU ? occ : NLS_WG_PER_CU);
  known.push_back(Key{dev, e->func, *cap});
  return 0;
}
static_assert(NLK_MAXBINS == MFFT_INCR_HIST_MAXBINS, "the public header states the kernels' limit");
static_assert(NLI_MAXSEP == MFFT_INCR_MAXSEP && NLI_FIELD == INCR_FIELD && NLI_SLOTS == INCR_SLOTS, "one number of separations per launch");
static int find_nlr(Op kind, int64_t n, int prec, const KernelEntry** e) {
  const NlProduct& q = nl_product(kind);
  *e = q.op == kind && q.nout == 0 ? find_nlz(n, prec, kind) : nullptr;
  if (!*e) return set_error(MFFT_ERR_UNSUPPORTED, "no fused z-stage kernel with %s of length %lld", q.name, (long long)n);
  return 0;
}
// The arithmetic is nlr_shape.h's; only the resident workgroups come from the runtime.
int nlr_launch_shape(Op kind, int64_t n, int prec, int64_t nrows, NlrShape* shape) {
  const KernelEntry* e = nullptr;
  MFFT_TRY(find_nlr(kind, n, prec, &e));
  if (nrows < 1) return set_error(MFFT_ERR_INVALID, "no rows");
  void* tw = nullptr;
  MFFT_TRY(prepare_kernel(e, &tw));                // (the LDS attribute is set before the occupancy is asked for)
  int cap = 0;
  MFFT_TRY(nls_resident(e, &cap));
  if (!nlr_shape(e->tile, e->threads, n, cap, nrows, nl_product(kind).counts, shape))
    return set_error(MFFT_ERR_INTERNAL, "%s: one pass of a workgroup counts 2^32 values", e->name);
  return 0;
}
// what the parameters of every reduction kernel share: the head (NlzParams<T>; out, scale and rt3 are not used) and the three
// members each Nl?Params ends in
template <typename T, template <typename> class PT>
static PT<T> nlr_params(const NlrArgs& a, void* tw) {
  PT<T> P;
  for (int f = 0; f < 3; ++f) {
    P.a[f] = static_cast<const cx<T>*>(f < a.npairs ? a.a[f] : nullptr);
    P.b[f] = static_cast<const cx<T>*>(f < a.npairs ? a.b[f] : nullptr);
    P.out[f] = nullptr;
  }
  P.tw = static_cast<const cx<T>*>(tw);
  P.rt3 = nullptr;
  P.in_stride = a.in_stride;
  P.out_stride = 0;
  P.nrows = a.nrows;
  P.valid = a.valid > 0 && a.valid < a.n / 2 + 1 ? a.valid : a.n / 2 + 1;
  P.valid_in = a.valid_in > 0 && a.valid_in < P.valid ? a.valid_in : P.valid;
  P.scale = (T)1;
  P.norm = a.norm;
  P.npairs = a.npairs;
  P.ngroups = a.ngroups;
  return P;
}
template <typename T>
static int launch_nlr_t(const KernelEntry* e, const NlrArgs& a, void* tw, hipStream_t s) {
  const NlrCall& c = a.call;
  auto run = [&](const auto& P) {
    e->launch(&P, a.ngroups, s);
    MFFT_HIP(hipGetLastError());
    return 0;
  };
  if (a.kind == Op::Moments) {
    auto P = nlr_params<T, NlsParams>(a, tw);
    P.part = static_cast<double*>(a.part);
    for (int i = 0; i < 2 * NLS_PAIRS; ++i) P.center[i] = c.center[i];
    return run(P);
  }
  if (a.kind == Op::Histogram) {
    auto P = nlr_params<T, NlhParams>(a, tw);
    P.part = static_cast<unsigned*>(a.part);
    for (int i = 0; i < 2 * NLS_PAIRS; ++i) { P.lo[i] = c.lo[i]; P.inv[i] = c.inv[i]; }
    P.nbins = c.nbins;
    return run(P);
  }
  if (a.kind == Op::JointHistogram) {
    auto P = nlr_params<T, NljParams>(a, tw);
    P.part = static_cast<unsigned*>(a.part);
    for (int i = 0; i < 2 * NLS_PAIRS; ++i) { P.lo[i] = c.lo[i]; P.inv[i] = c.inv[i]; }
    P.nba = c.nba;
    P.nbb = c.nbb;
    return run(P);
  }
  if (a.kind == Op::Quadratic) {
    auto P = nlr_params<T, NlqParams>(a, tw);
    P.mpart = static_cast<double*>(a.part);
    P.hpart = static_cast<unsigned*>(a.part2);
    for (int i = 0; i < 2 * NLS_PAIRS; ++i) {        // (a slot without a field has weight 0)
      const bool used = i / 2 < a.npairs && (i % 2 == 0 || a.b[i / 2]);
      P.w[i] = used ? c.w[i] : 0.0;
    }
    P.center = c.center[0];
    P.lo = c.lo[0];
    P.inv = c.inv[0];
    P.nbins = c.nbins;
    return run(P);
  }
  if (a.kind == Op::Profiles) {
    auto P = nlr_params<T, NlpParams>(a, tw);
    P.part = static_cast<double*>(a.part);
    for (int i = 0; i < 2 * NLS_PAIRS; ++i) P.center[i] = c.center[i];
    return run(P);
  }
  if (a.kind == Op::IncrementHistogram) {
    auto P = nlr_params<T, NlkParams>(a, tw);
    P.part = static_cast<unsigned*>(a.part);
    for (int f = 0; f < 2 * NLS_PAIRS; ++f)
      for (int i = 0; i < NLI_MAXSEP; ++i) {
        P.lo[f][i] = i < c.nsep ? c.ilo[f][i] : 0.0;
        P.inv[f][i] = i < c.nsep ? c.iinv[f][i] : 1.0;
      }
    for (int i = 0; i < NLI_MAXSEP; ++i) P.sep[i] = i < c.nsep ? c.sep[i] : 1;
    P.nsep = c.nsep;
    P.nbins = c.nbins;
    return run(P);
  }
  auto P = nlr_params<T, NliParams>(a, tw);          // Op::Increments
  P.part = static_cast<double*>(a.part);
  for (int i = 0; i < NLI_MAXSEP; ++i) P.sep[i] = i < c.nsep ? c.sep[i] : 1;
  P.nsep = c.nsep;
  return run(P);
}
// Everything is checked before the launch: the common arguments, then the kind's own, then that no count can wrap.
int launch_nlr(const NlrArgs& a, hipStream_t s) {
  const KernelEntry* e = nullptr;
  MFFT_TRY(find_nlr(a.kind, a.n, a.prec, &e));
  const NlrCall& c = a.call;
  const int64_t units = (a.nrows + 2 * e->tile - 1) / (2 * e->tile);
  if (a.npairs < 1 || a.npairs > NLS_PAIRS || !a.part || a.nrows < 1 || a.ngroups < 1 || a.ngroups > units)
    return set_error(MFFT_ERR_INVALID, "bad argument");
  for (int p = 0; p < a.npairs; ++p)
    if (!a.a[p]) return set_error(MFFT_ERR_INVALID, "null argument");
  auto range_ok = [&](int i) { return c.inv[i] > 0.0 && std::isfinite(c.inv[i]) && std::isfinite(c.lo[i]); };
  if (a.kind == Op::Histogram || a.kind == Op::JointHistogram) {
    const bool joint = a.kind == Op::JointHistogram;
    if (joint ? c.nba < 1 || c.nba > NLJ_MAXBINS || c.nbb < 1 || c.nbb > NLJ_MAXBINS : c.nbins < 1 || c.nbins > NLH_MAXBINS)
      return set_error(MFFT_ERR_INVALID, "bad argument");
    for (int p = 0; p < a.npairs; ++p) {
      if (joint && !a.b[p]) return set_error(MFFT_ERR_INVALID, "null argument: a joint histogram counts pairs of fields");
      if (!range_ok(2 * p) || !range_ok(2 * p + 1)) return set_error(MFFT_ERR_INVALID, "bad histogram range");
    }
  } else if (a.kind == Op::Quadratic) {
    if (!a.part2 || c.nbins < 0 || c.nbins > NLH_MAXBINS) return set_error(MFFT_ERR_INVALID, "bad argument");
    for (int i = 0; i < 2 * a.npairs; ++i)
      if (!std::isfinite(c.w[i])) return set_error(MFFT_ERR_INVALID, "a weight is not finite");
    if (c.nbins > 0 && !range_ok(0)) return set_error(MFFT_ERR_INVALID, "bad histogram range");
  } else if (a.kind == Op::Profiles) {
    for (int p = 0; p < a.npairs; ++p) {
      if (!a.b[p]) return set_error(MFFT_ERR_INVALID, "null argument: a profile takes pairs of fields");
      if (!std::isfinite(c.center[2 * p]) || !std::isfinite(c.center[2 * p + 1])) return set_error(MFFT_ERR_INVALID, "a centre is not finite");
    }
  } else if (a.kind == Op::Increments || a.kind == Op::IncrementHistogram) {
    if (c.nsep < 1 || c.nsep > NLI_MAXSEP) return set_error(MFFT_ERR_INVALID, "bad argument");
    for (int i = 0; i < c.nsep; ++i)               // (the kernel reads the row's exchange buffer at (position + sep) mod n)
      if (c.sep[i] < 1 || c.sep[i] >= a.n) return set_error(MFFT_ERR_INVALID, "separation %d outside 1 .. %d", c.sep[i], a.n - 1);
    if (a.kind == Op::IncrementHistogram) {
      if (c.nbins < 1 || c.nbins > NLK_MAXBINS) return set_error(MFFT_ERR_INVALID, "bad argument");
      for (int f = 0; f < 2 * a.npairs; ++f)
        for (int i = 0; i < c.nsep; ++i)
          if (!(c.iinv[f][i] > 0.0) || !std::isfinite(c.iinv[f][i]) || !std::isfinite(c.ilo[f][i])) return set_error(MFFT_ERR_INVALID, "bad histogram range");
    }
  }
  // what one workgroup counts per field stays below 2^32: passes x 2 x rows per workgroup x n
  if (nl_product(a.kind).counts && nlr_counted(e->tile, a.n, a.nrows, a.ngroups) >= ((int64_t)1 << 32))
    return set_error(MFFT_ERR_INVALID, "%lld rows in one %s launch of %d workgroups: a count could wrap", (long long)a.nrows,
                     nl_product(a.kind).name, a.ngroups);
  void* tw = nullptr;
  MFFT_TRY(prepare_kernel(e, &tw));
  return by_prec(a.prec, [&](auto t) { return launch_nlr_t<decltype(t)>(e, a, tw, s); });
}

size_t nlr_part_bytes(const NlrArgs& z, const NlrShape& shape) {
  if (z.kind == Op::Histogram) return hist_part_bytes(shape.ngroups, 2 * z.npairs, z.call.nbins);
  if (z.kind == Op::JointHistogram) return joint_part_bytes(shape.ngroups, z.npairs, z.call.nba, z.call.nbb);
  if (z.kind == Op::Quadratic) return quad_mpart_bytes(shape.waves) + quad_hpart_bytes(shape.ngroups, z.call.nbins);
  if (z.kind == Op::Profiles) return prof_part_bytes(shape.ngroups, shape.tile, z.npairs, z.n);
  if (z.kind == Op::IncrementHistogram) return incr_hist_part_bytes(shape.ngroups, 2 * z.npairs, z.call.nsep, z.call.nbins);
  return (size_t)shape.waves * (z.kind == Op::Increments ? INCR_SLOTS : NLS_SLOTS) * sizeof(double);
}
// The ONE loop over the rows of a batch.  The kinds that sum doubles have no limit on the rows of a launch: one launch, one fold.
int nlr_rows(const NlrArgs& z0, void* acc, void* acc2, hipStream_t s) {
  const size_t es = elem_bytes(z0.prec, true);
  NlrShape all, shape;
  MFFT_TRY(nlr_launch_shape(z0.kind, z0.n, z0.prec, z0.nrows, &all));      // (the shape `part` was sized by: the largest of the launches)
  for (int64_t r0 = 0; r0 < z0.nrows;) {
    MFFT_TRY(nlr_launch_shape(z0.kind, z0.n, z0.prec, z0.nrows - r0, &shape));
    NlrArgs z = z0;
    z.nrows = std::min(z0.nrows - r0, shape.max_rows);
    z.ngroups = shape.ngroups;
    if (z.kind == Op::Quadratic) z.part2 = static_cast<char*>(z0.part) + quad_mpart_bytes(all.waves);
    for (int p = 0; p < z.npairs; ++p) {
      if (z.a[p]) z.a[p] = static_cast<const char*>(z0.a[p]) + (size_t)(r0 * z0.in_stride) * es;
      if (z.b[p]) z.b[p] = static_cast<const char*>(z0.b[p]) + (size_t)(r0 * z0.in_stride) * es;
    }
    MFFT_TRY(launch_nlr(z, s));
    const size_t groups = (size_t)shape.ngroups, waves = (size_t)shape.waves;
    const NlrCall& c = z.call;
    if (z.kind == Op::Moments) {
      MFFT_TRY(moments_fold(static_cast<const double*>(z.part), waves, NLS_SLOTS, static_cast<double*>(acc), s));
    } else if (z.kind == Op::Histogram) {
      MFFT_TRY(hist_fold(static_cast<const unsigned*>(z.part), groups, 2 * z.npairs, c.nbins, static_cast<int64_t*>(acc), s));
    } else if (z.kind == Op::JointHistogram) {
      MFFT_TRY(hist_fold_slots(static_cast<const unsigned*>(z.part), groups, z.npairs, joint_cells(c.nba, c.nbb), static_cast<int64_t*>(acc), s));
    } else if (z.kind == Op::Quadratic) {
      MFFT_TRY(moments_fold(static_cast<const double*>(z.part), waves, NLS_STATS, static_cast<double*>(acc), s));
      if (c.nbins > 0) MFFT_TRY(hist_fold(static_cast<const unsigned*>(z.part2), groups, 1, c.nbins, static_cast<int64_t*>(acc2), s));
    } else if (z.kind == Op::IncrementHistogram) {  // rows of nsep (nbins + 3) counts per slot: the histograms' fold
      MFFT_TRY(hist_fold_slots(static_cast<const unsigned*>(z.part), groups, 2 * z.npairs, c.nsep * (c.nbins + 3), static_cast<int64_t*>(acc), s));
    } else if (z.kind == Op::Profiles) {            // one partial profile per row slot of the launch
      MFFT_TRY(prof_fold(static_cast<const double*>(z.part), groups * (size_t)shape.tile, (size_t)z.npairs * NLP_STATS * (size_t)z.n,
                         static_cast<double*>(acc), s));
    } else {
      MFFT_TRY(incr_fold(static_cast<const double*>(z.part), waves, INCR_SLOTS, static_cast<double*>(acc), s));
    }
    r0 += z.nrows;
  }
  return 0;
}

// ---------------------------------------------------------------------------
// data-movement kernels
// ---------------------------------------------------------------------------
// Work unit = (row (i, j), chunk of CHUNK contiguous elements of that row); threads of
// blockDim.x stride over the chunk, blockDim.y units per block, grid-stride over units.
// Long rows (pad / truncate of whole planes) and many short rows (z chunks) both fill the chip.
constexpr int64_t BOX_CHUNK = 2048;

template <typename R, int MODE>
__global__ __launch_bounds__(256) void box_copy_kernel(const R* __restrict__ src, R* __restrict__ dst,
                                                       int64_t e1, int64_t e2, int64_t s0, int64_t s1,
                                                       int64_t d0, int64_t d1, R scale, int64_t nunits, int64_t nchunks) {
  for (int64_t u = (int64_t)blockIdx.x * blockDim.y + threadIdx.y; u < nunits; u += (int64_t)gridDim.x * blockDim.y) {
    const int64_t row = u / nchunks, c = u - row * nchunks;
    const int64_t i = row / e1, j = row - i * e1;
    const R* sp = src + i * s0 + j * s1;
    R* dp = dst + i * d0 + j * d1;
    const int64_t k1 = (c + 1) * BOX_CHUNK < e2 ? (c + 1) * BOX_CHUNK : e2;
    for (int64_t k = c * BOX_CHUNK + threadIdx.x; k < k1; k += blockDim.x) {
      R v = sp[k] * scale;
      if (MODE == 1) v += dp[k];
      dp[k] = v;
    }
  }
}

struct alignas(16) vec16 { double a, b; };
template <int MODE>
__global__ __launch_bounds__(256) void box_copy16_kernel(const vec16* __restrict__ src, vec16* __restrict__ dst,
                                                         int64_t e1, int64_t e2, int64_t s0, int64_t s1,
                                                         int64_t d0, int64_t d1, int64_t nunits, int64_t nchunks) {
  for (int64_t u = (int64_t)blockIdx.x * blockDim.y + threadIdx.y; u < nunits; u += (int64_t)gridDim.x * blockDim.y) {
    const int64_t row = u / nchunks, c = u - row * nchunks;
    const int64_t i = row / e1, j = row - i * e1;
    const vec16* sp = src + i * s0 + j * s1;
    vec16* dp = dst + i * d0 + j * d1;
    const int64_t k1 = (c + 1) * BOX_CHUNK < e2 ? (c + 1) * BOX_CHUNK : e2;
    for (int64_t k = c * BOX_CHUNK + threadIdx.x; k < k1; k += blockDim.x) dp[k] = sp[k];
  }
}

int launch_box_copy(const BoxArgs& a, hipStream_t s) {
  const int64_t nrows = a.e0 * a.e1;
  if (nrows <= 0 || a.e2 <= 0) return 0;
  const int unit = a.elem;    // bytes per element
  const bool plain = (a.mode == 0 && a.scale == 1.0);
  auto shape = [&](int64_t e2, int* bx, int* by, int64_t* nchunks, int64_t* nunits, unsigned* grid) {
    *nchunks = (e2 + BOX_CHUNK - 1) / BOX_CHUNK;
    const int64_t run = e2 < BOX_CHUNK ? e2 : BOX_CHUNK;
    int x = 64;
    while (x < 256 && x < run) x *= 2;
    *bx = x;
    *by = 256 / x;
    *nunits = nrows * *nchunks;
    int64_t g = (*nunits + *by - 1) / *by;
    if (g > 65536 * 2) g = 65536 * 2;
    *grid = (unsigned)g;
  };
  int bx, by;
  int64_t nchunks, nunits;
  unsigned grid;
  if (plain && unit == 16) {
    shape(a.e2, &bx, &by, &nchunks, &nunits, &grid);
    hipLaunchKernelGGL(box_copy16_kernel<0>, dim3(grid), dim3(bx, by), 0, s, static_cast<const vec16*>(a.src),
                       static_cast<vec16*>(a.dst), a.e1, a.e2, a.s0, a.s1, a.d0, a.d1, nunits, nchunks);
    MFFT_HIP(hipGetLastError());
    return 0;
  }
  // scalar path in units of the real type
  const int rbytes = a.prec == MFFT_DOUBLE ? 8 : 4;
  const int per = unit / rbytes;            // reals per element
  const int64_t e2 = a.e2 * per;
  shape(e2, &bx, &by, &nchunks, &nunits, &grid);
#define MFFT_BOX(R, MODE)                                                                                   \
  hipLaunchKernelGGL((box_copy_kernel<R, MODE>), dim3(grid), dim3(bx, by), 0, s,                            \
                     static_cast<const R*>(a.src), static_cast<R*>(a.dst), a.e1, e2, a.s0 * per, a.s1 * per, \
                     a.d0 * per, a.d1 * per, (R)a.scale, nunits, nchunks)
  if (a.prec == MFFT_DOUBLE) {
    if (a.mode == 1) MFFT_BOX(double, 1); else MFFT_BOX(double, 0);
  } else {
    if (a.mode == 1) MFFT_BOX(float, 1); else MFFT_BOX(float, 0);
  }
#undef MFFT_BOX
  MFFT_HIP(hipGetLastError());
  return 0;
}

template <typename T>
__global__ __launch_bounds__(256) void mask_kernel(cx<T>* fu, const uint8_t* mask, size_t count) {
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < count; i += (size_t)gridDim.x * blockDim.x) {
    const T m = (T)mask[i];
    cx<T> v = fu[i];
    v.x *= m;
    v.y *= m;
    fu[i] = v;
  }
}

int launch_mask(void* fu, const uint8_t* mask, size_t count, int prec, hipStream_t s) {
  if (count == 0) return 0;
  size_t grid = (count + 255) / 256;
  if (grid > 16384) grid = 16384;
  if (prec == MFFT_DOUBLE)
    hipLaunchKernelGGL(mask_kernel<double>, dim3((unsigned)grid), dim3(256), 0, s, static_cast<cx<double>*>(fu), mask, count);
  else
    hipLaunchKernelGGL(mask_kernel<float>, dim3((unsigned)grid), dim3(256), 0, s, static_cast<cx<float>*>(fu), mask, count);
  MFFT_HIP(hipGetLastError());
  return 0;
}

template <typename T>
__global__ __launch_bounds__(256) void line_nyquist_kernel(cx<T>* rows, int64_t nrows, int64_t pitch, int64_t coln) {
  for (int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; r < nrows; r += (int64_t)gridDim.x * blockDim.x) {
    cx<T>* p = rows + r * pitch;
    const cx<T> c0 = p[0], cn = p[coln];
    p[0] = mk<T>(c0.x - cn.y, (T)0);
    p[coln] = mk<T>(cn.x, (T)0);
  }
}

int launch_line_nyquist(void* rows, int64_t nrows, int64_t pitch, int64_t coln, int prec, hipStream_t s) {
  if (nrows <= 0) return 0;
  const unsigned grid = (unsigned)std::min<int64_t>((nrows + 255) / 256, 4096);
  if (prec == MFFT_DOUBLE)
    hipLaunchKernelGGL(line_nyquist_kernel<double>, dim3(grid), dim3(256), 0, s, static_cast<cx<double>*>(rows), nrows, pitch, coln);
  else
    hipLaunchKernelGGL(line_nyquist_kernel<float>, dim3(grid), dim3(256), 0, s, static_cast<cx<float>*>(rows), nrows, pitch, coln);
  MFFT_HIP(hipGetLastError());
  return 0;
}

template <typename T>
__global__ __launch_bounds__(256) void scale_kernel(T* d, size_t count, T sc) {
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < count; i += (size_t)gridDim.x * blockDim.x)
    d[i] *= sc;
}

int launch_scale(void* data, size_t count, double scale, int prec, hipStream_t s) {
  if (count == 0) return 0;
  size_t grid = (count + 255) / 256;
  if (grid > 16384) grid = 16384;
  if (prec == MFFT_DOUBLE)
    hipLaunchKernelGGL(scale_kernel<double>, dim3((unsigned)grid), dim3(256), 0, s, static_cast<double*>(data), count, scale);
  else
    hipLaunchKernelGGL(scale_kernel<float>, dim3((unsigned)grid), dim3(256), 0, s, static_cast<float*>(data), count, (float)scale);
  MFFT_HIP(hipGetLastError());
  return 0;
}

// counter-based uniform [0,1) generator (splitmix64 of the element index)
__device__ __forceinline__ uint64_t splitmix64(uint64_t x) {
  x += 0x9E3779B97F4A7C15ull;
  x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
  x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
  return x ^ (x >> 31);
}
template <typename T>
__global__ __launch_bounds__(256) void fill_kernel(T* d, size_t count, uint64_t seed) {
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < count; i += (size_t)gridDim.x * blockDim.x) {
    const uint64_t r = splitmix64(seed * 0xD1B54A32D192ED03ull + i);
    d[i] = (T)((double)(r >> 11) * (1.0 / 9007199254740992.0));
  }
}

int launch_fill_uniform(void* data, size_t count, int prec, uint64_t seed, hipStream_t s) {
  if (count == 0) return 0;
  size_t grid = (count + 255) / 256;
  if (grid > 16384) grid = 16384;
  if (prec == MFFT_DOUBLE)
    hipLaunchKernelGGL(fill_kernel<double>, dim3((unsigned)grid), dim3(256), 0, s, static_cast<double*>(data), count, seed);
  else
    hipLaunchKernelGGL(fill_kernel<float>, dim3((unsigned)grid), dim3(256), 0, s, static_cast<float*>(data), count, seed);
  MFFT_HIP(hipGetLastError());
  return 0;
}

}  // namespace mfft
