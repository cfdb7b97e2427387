// mfft_internal.h -- internal C++ interfaces of libmpifft4py_amd.so
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string>
#include <vector>
#include "../../include/mpifft4py_amd.h"
#include "registry.h"
#include "nlr_shape.h"

namespace mfft {

// ---- errors ------------------------------------------------------------------
int set_error(int code, const char* fmt, ...) __attribute__((format(printf, 2, 3)));
const char* last_error();

#define MFFT_HIP(call)                                                                   \
  do {                                                                                   \
    hipError_t e_ = (call);                                                              \
    if (e_ != hipSuccess)                                                                \
      return ::mfft::set_error(MFFT_ERR_HIP, "%s failed: %s (%s:%d)", #call,             \
                               hipGetErrorString(e_), __FILE__, __LINE__);               \
  } while (0)

#define MFFT_TRY(call)                  \
  do {                                  \
    int rc_ = (call);                   \
    if (rc_ != 0) return rc_;           \
  } while (0)

inline size_t elem_bytes(int prec, bool complex_) { return (prec == MFFT_DOUBLE ? 8 : 4) * (complex_ ? 2 : 1); }

// ---- kernel launch layer -------------------------------------------------------
struct RowSpec {       // row r -> (r / split) * hi + (r % split) * lo   (elements)
  int64_t hi = 0, lo = 0, split = 0;   // split <= 0: single group
};

struct ColArgs {
  const void* in = nullptr;
  void* out = nullptr;
  int n = 0;             // transform length
  int prec = MFFT_DOUBLE;
  bool inverse = false;
  int64_t in_outer = 0, out_outer = 0;
  RowSpec in_rows, out_rows;
  int64_t ncols = 0;     // contiguous columns per outer batch
  int64_t nouter = 1;
  double scale = 1.0;
  int remap = 1;         // XCD-aware tile order
  bool allow_nt = true;  // use the non-temporal variant when the layout is 128-byte aligned
  Op pad = Op::Plain;    // PadLoad: input has 2n/3 physical rows (zero band skipped); TruncStore: output truncated to 2n/3 rows
                         // (mask-on-load and band-pruned passes are asked for through `mask` and `band` below)
  bool fold = false;     // TruncStore: sum the two Nyquist rows (R2C convention)
  int64_t in_wrap = 0, in_wrap_gap = 0;   // wrapped input columns (fft_kernels.h ColParams::in_wrap): column c is read from
                                          // c + (c / in_wrap) * in_wrap_gap; radix kernels only
  int thirds = -1;       // PadLoad inverse: one third of a tile's transform per workgroup (ColFft3S)?  -1: launch_col's rule
                         // (single precision, or a pass without an outer batch), 1: yes where the kernel exists, 0: no
  const uint8_t* mask = nullptr;   // inverse transforms: one byte per element of `in` (same element offsets), 0 = reads as zero
                                   // (the 2/3-rule `fu * dealias` of slab.py:237-245 without a masked copy of the spectrum)
  // inverse transforms, 2/3-rule mask of band form (fft_kernels.h ColParams b_*): rows [row_lo, row_hi) are zero and
  // not loaded, tiles whose columns are all removed are skipped
  struct Band {
    bool on = false;
    int row_lo = 0, row_hi = 0, c_off = 0, c_per = 1 << 30, c_lim = 1 << 30, g_off = 0, g_step = 0, g_lo = 1 << 30, g_hi = 1 << 30;
    const int* tile_list = nullptr;     // device array of the tiles with a kept column (tile = outer * ntile_c + tc), or null
    int ntiles_listed = 0;
    int g_zero = 0;                     // 1: columns of a removed y are transformed as zeros and written instead of skipped;
                                        // 2: columns of a removed z as well, no tile is skipped (complete output)
  } band;
};
bool c2r_limit_supported(int64_t n, int prec);   // a c2r kernel of real length n that reads only the first `valid` bins exists
bool band_fusable(int64_t n, int prec);          // a pruned (band) strided inverse kernel of length n exists
int col_tile_width(int64_t n, int prec, bool inverse, Op op);   // columns per tile of the default build of that strided kernel, 0: none
int launch_col(const ColArgs& a, hipStream_t s);
bool mask_fusable(int64_t n, int prec);   // a strided inverse kernel of length n that applies a mask on load exists

// complex side of a contiguous-axis transform split into z chunks (fft_kernels.h, ZSplit): the pack / unpack of the
// pencils' z-splitting exchange fused into the transform.  nchunk = 0: plain rows.
struct ZSplitArgs {
  int nchunk = 0;
  int64_t q = 0, last_len = 0;       // chunk length; length of the last chunk
  int64_t rows_total = 0, row0 = 0;  // rows of every chunk block; first row of this launch inside them
  int64_t pitch = 0, last_pitch = 0; // elements between the rows of a block / of the last block; 0 = its chunk length
};

struct RowArgs {
  const void* in = nullptr;
  void* out = nullptr;
  int n = 0;
  int prec = MFFT_DOUBLE;
  bool inverse = false;
  int64_t in_stride = 0, out_stride = 0, nrows = 0;
  double scale = 1.0;
  ZSplitArgs zs;         // forward: of `out`, inverse: of `in`
};
int launch_row(const RowArgs& a, hipStream_t s);

struct RealArgs {
  const void* in = nullptr;
  void* out = nullptr;
  int n = 0;             // REAL length
  int prec = MFFT_DOUBLE;
  int64_t in_stride = 0, out_stride = 0, nrows = 0;   // in elements of the respective types
  double scale = 1.0;
  int valid = 0;         // complex columns present in memory (0 = all n/2+1)
  ZSplitArgs zs;         // of the complex side
  // pair-row kernels (Op::PairRows): the rows are the (x, y) lines of a (pair_n0, pair_n1) mesh, nrows = pair_n0 * pair_n1, the
  // strides above are the row pitches inside a plane and the planes lie pair_rplane reals / pair_cplane complex elements apart
  int pair_n0 = 0, pair_n1 = 0;      // 0: plain rows
  int64_t pair_rplane = 0, pair_cplane = 0;
  // real side blocked in y: blocks of pair_yblock rows per plane, pair_rblock reals from block to block, pair_rplane from x row to
  // x row INSIDE a block (fft_kernels.h RealPairParams::p_ymap); 0 or pair_n1: one block, the plain layout
  int pair_yblock = 0;
  int64_t pair_rblock = 0;
  // order in which the workgroups take the pair slots (fft_kernels.h pair_slot): tiles of pair_tile x pair_tile slots; 0: row order
  int pair_tile = 0;
  bool pair_tile_xfast = false;      // kx fastest inside a tile (ky: the default)
};
int launch_r2c(const RealArgs& a, hipStream_t s);
int launch_c2r(const RealArgs& a, hipStream_t s);
bool pair_rows_supported(int64_t n, int prec);     // both pair-row kernels of real length n exist

// fused nonlinear z stage (fft_nlz.h): rows of half-spectra of two vector fields in, rows of the half-spectra of their
// cross product out (may alias the inputs row for row) -- or, product = Op::Dot, the ONE row out[0] of their dot product -- or,
// product = Op::CrossDot, the cross product AND the row out[3] of the dot product of a with a third field c
struct NlzArgs {
  const void* a[3] = {nullptr, nullptr, nullptr};
  const void* b[3] = {nullptr, nullptr, nullptr};
  const void* c[3] = {nullptr, nullptr, nullptr};   // Op::CrossDot only
  void* out[9] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};   // (nine: Op::Outer)
  int n = 0;             // REAL length of a z row
  int prec = MFFT_DOUBLE;
  int64_t in_stride = 0, out_stride = 0, nrows = 0;   // complex elements
  int valid = 0;         // bins per row present in memory (0 = all n/2+1)
  int valid_in = 0;      // bins per INPUT row, where fewer than `valid` exist (pruned 2/3-rule); 0 = valid
  double scale = 1.0;    // applied to the product (1 / n^2: both inverse transforms normalised)
  Op product = Op::Plain;  // Op::Plain: a x b into out[0..2];  Op::Dot: sum_f a_f b_f into out[0], out[1..2] unused;
                           // Op::CrossDot: a x b into out[0..2] and sum_f a_f c_f into out[3];
                           // Op::Outer: a_i b_j into out[3 i + j]; out[0..2] may be a[0..2], out[3..5] b[0..2]
  void* part = nullptr;    // not null: the Build::AbsMax kernel runs and writes nlz_absmax_waves() groups of 12 un-normalised
                           // partial maxima here, in the rows' precision: [wave][row of the pair][a, b][field] (fft_nlz.h NlmParams)
};
// What a product of the nonlinear term is, written down ONCE: every route, entry point, key and message reads this table.
struct NlProduct {
  Op op;
  const char* name;      // in error texts; in plan_info keys "nonlinear[_<name>][_absmax]_fused_<mode>", the cross product unnamed
  int nin, nout;         // fields in (a, b, then c), rows / components out (out, then the scalar one)
  bool absmax;           // a Build::AbsMax kernel family exists (the call with real-space maxima)
  bool nlz3;             // Build::Nlz3, the pruned 3/2-rule kernel, may stand in
  bool counts = false;   // a reduction whose workgroups count into unsigned slots: one launch stays below 2^32 values (nlr_shape.h)
};
constexpr NlProduct NL_PRODUCTS[] = {
    {Op::Plain, "cross", 6, 3, true, true},
    {Op::Dot, "dot", 6, 1, true, false},
    {Op::CrossDot, "cross_dot", 9, 4, false, false},
    {Op::Outer, "outer", 6, 9, false, false},
    // nout == 0: the reductions (NlrArgs below).  Up to six fields: the call says how many, NlFields::nfields
    {Op::Moments, "moments", 6, 0, false, false},
    {Op::Histogram, "histogram", 6, 0, false, false, true},
    {Op::Quadratic, "quadratic", 6, 0, false, false, true},
    {Op::Increments, "increments", 6, 0, false, false},
    {Op::JointHistogram, "joint", 6, 0, false, false, true},       // (one or three PAIRS of fields: a_p with b_p)
    {Op::Profiles, "profiles", 6, 0, false, false},                // (one or three PAIRS again; sums of doubles: no 2^32 limit)
    {Op::IncrementHistogram, "incr_hist", 6, 0, false, false, true},
};
inline const NlProduct& nl_product(Op op) {
  for (const NlProduct& q : NL_PRODUCTS)
    if (q.op == op) return q;
  return NL_PRODUCTS[0];
}
// The caller's arrays of one nonlinear operation (plan_nonlinear.hip): vector fields a, b and -- where the product has one -- c
// in, the result out (three components, the ONE of the dot product, or the NINE of the outer product) and, of the product with
// both, the scalar result outs.
// An operation whose number of fields belongs to the call (the reductions): nfields of them, ncomp components of a, then of b.
struct NlFields {
  const void *a, *b, *c;
  void *out, *outs;
  int ncomp = 3;               // components per field
  int nfields = 0;             // 0: what the table of products says (NlProduct::nin)
  int nres = 3;                // components `out` holds (nine: the outer product); results beyond them are outs
  int nin(const NlProduct& q) const { return nfields > 0 ? nfields : q.nin; }
  // component f of the inputs (a, b, then c) / of the results (out, then outs), C elements of es bytes per component
  const void* src(int f, int64_t C, size_t es) const {
    return static_cast<const char*>(f < ncomp ? a : f < 2 * ncomp ? b : c) + (size_t)((f % ncomp) * C) * es;
  }
  void* dst(int f, int64_t C, size_t es) const { return f < nres ? static_cast<char*>(out) + (size_t)(f * C) * es : outs; }
};
// Where field f of a reduction (ncomp components of a, then of b) rides: slot 2 p is the first half of pair p, 2 p + 1 the
// second.  With two fields a_f and b_f share a transform, as in the products; with one the components pair up among themselves.
// THE slot rule: the plan's routes, the stage-level entry points and the un-slotting of every result call this.
inline int nls_slot(const NlFields& u, int f) {
  const int ncomp = u.ncomp;
  return u.b ? (f < ncomp ? 2 * f : 2 * (f - ncomp) + 1) : f;
}
bool nlz_supported(int64_t n, int prec, Op product = Op::Plain, bool absmax = false);
int64_t nlz_absmax_waves(int64_t n, int prec, Op product, int64_t nrows);
int launch_nlz(const NlzArgs& a, hipStream_t s);
// The z stages that end in a REDUCTION instead of a product (the table entries with nout == 0; a header each, nlz_*.h: the body of NlzMoments,
// NlzHist, NlzJoint, NlzQuad, NlzIncr, NlzProf), described ONCE: the launch, its shape, the loop over the rows and the routes of the plan read
// NlrArgs.  Pair p is the rows a[p] + i b[p] on one complex transform, p < npairs <= 3; b[p] may be null (an odd field count) except
// in a joint histogram and in a profile.  x = norm * (the un-normalised inverse transform).  Slots are [pair][a, b].
// What a call of one kind adds to that -- the plan parks it between a call's begin and its batches (mfft_plan_s::nlcall):
struct NlrCall {
  double center[6] = {0, 0, 0, 0, 0, 0};   // Moments, Profiles: sums about center[slot]; Quadratic: about center[0]
  double lo[6] = {0, 0, 0, 0, 0, 0}, inv[6] = {1, 1, 1, 1, 1, 1};   // Histogram, JointHistogram: lower edge and bins / (hi - lo) per
                                                                    // slot; Quadratic: lo[0], inv[0] of q
  double w[6] = {0, 0, 0, 0, 0, 0};        // Quadratic: q = sum over the slots of w[slot] x^2
  int nbins = 0;                           // Histogram: 1 .. NLH_MAXBINS; Quadratic: 0 .. NLH_MAXBINS, 0: no histogram
  int nba = 0, nbb = 0;                    // JointHistogram: 1 .. MFFT_JOINT_MAXBINS bins of the a fields / of the b fields
  int sep[MFFT_INCR_MAXSEP] = {0};         // Increments: 1 <= sep[i] < n, i < nsep
  int nsep = 0;                            // 1 .. MFFT_INCR_MAXSEP
  // IncrementHistogram: sep, nsep as Increments, nbins 1 .. MFFT_INCR_HIST_MAXBINS, and a range per slot AND separation
  double ilo[6][MFFT_INCR_MAXSEP] = {}, iinv[6][MFFT_INCR_MAXSEP] = {};
};
struct NlrArgs {
  Op kind = Op::Moments;
  const void* a[3] = {nullptr, nullptr, nullptr};
  const void* b[3] = {nullptr, nullptr, nullptr};
  int npairs = 0;
  int n = 0;             // REAL length of a z row
  int prec = MFFT_DOUBLE;
  int64_t in_stride = 0, nrows = 0;   // complex elements
  int valid = 0;         // bins per row present in memory (0 = all n/2+1)
  int valid_in = 0;      // bins per row that are read, where fewer (pruned 2/3-rule); 0 = valid
  double norm = 1.0;
  int ngroups = 0;       // workgroups of the launch, from nlr_launch_shape(): nlr_rows sets it
  void* part = nullptr;  // the launch's partial results, nlr_part_bytes() of the shape of all rows: per wave NLS_SLOTS (Moments),
                         // INCR_SLOTS (Increments), NLS_STATS (Quadratic) doubles; per workgroup the unsigned counts (npairs, 2, nbins
                         // + 3) (Histogram), (npairs, cells) (JointHistogram), (npairs, 2, nsep, nbins + 3) (IncrementHistogram); per ROW
                         // SLOT of a workgroup (npairs, 5, n) doubles
                         // (Profiles: prof_part_bytes)
  void* part2 = nullptr; // Quadratic: per workgroup nbins + 3 unsigned counts of q, behind the doubles; nlr_rows sets it
  NlrCall call;
};
// {workgroups, waves, rows one launch may take} of the launch over nrows rows (nlr_shape.h; the resident workgroups from the runtime)
int nlr_launch_shape(Op kind, int64_t n, int prec, int64_t nrows, NlrShape* shape);
int launch_nlr(const NlrArgs& a, hipStream_t s);
// bytes of `part` for a launch of that shape
size_t nlr_part_bytes(const NlrArgs& z, const NlrShape& shape);
// All rows of z (ngroups, part2 not set): launches of at most max_rows rows, each folded into acc with the kind's fold below --
// statistics and counts accumulate over launches, batches and calls.  acc2: the int64 counts of a Quadratic call.
int nlr_rows(const NlrArgs& z, void* acc, void* acc2, hipStream_t s);
// Statistics [min, max, S1 .. S4] per slot (moments.hip).  acc: device doubles, nvals = 6 * slots of them.  moments_clear: the
// identity (+Inf, -Inf, zeros); moments_fold: acc[v] = merge(acc[v], the groups' part[g * nvals + v] in a fixed order), NaNs kept.
int moments_clear(double* acc, int nvals, hipStream_t s);
int moments_fold(const double* part, size_t groups, int nvals, double* acc, hipStream_t s);
// Histograms (hist.hip): per field nbins + 3 counts -- below lo, the nbins bins of [lo, hi), at or above hi, not finite (nlz_reduce.h
// hist_slot).  acc: device int64, (nfields, nbins + 3).  hist_fold: acc[f][s] += sum over the groups g, in fixed order, of
// part[(g * nfields + f) * (nbins + 3) + s]; nfields <= 6.
size_t hist_part_bytes(int ngroups, int nslots, int nbins);
int hist_fold(const unsigned* part, size_t groups, int nfields, int nbins, int64_t* acc, hipStream_t s);
// ... for rows of any length nslots (the grids of the joint histograms): part[(g * nfields + f) * nslots + s]
int hist_fold_slots(const unsigned* part, size_t groups, int nfields, int nslots, int64_t* acc, hipStream_t s);
// inv = nbins / (hi - lo) of a valid range; MFFT_ERR_INVALID for nbins outside 1 .. NLH_MAXBINS, hi <= lo, a range that is not finite
int hist_range(double lo, double hi, int nbins, double* inv);
int hist_max_bins();
// Joint histograms (joint.hip): per pair (nba + 3)(nbb + 3) counts, cell = slot of a_p * (nbb + 3) + slot of b_p (nlz_joint.h joint_cell)
inline int joint_cells(int nba, int nbb) { return (nba + 3) * (nbb + 3); }
size_t joint_part_bytes(int ngroups, int npairs, int nba, int nbb);
// inv of a valid range; MFFT_ERR_INVALID for a bin count outside 1 .. MFFT_JOINT_MAXBINS, hi <= lo, a range that is not finite
int joint_range(double lo, double hi, int nb, double* inv);
// Quadratic forms (quad.hip): bytes of the doubles and of the counts in `part`, the doubles first
size_t quad_mpart_bytes(int64_t waves);
size_t quad_hpart_bytes(int ngroups, int nbins);
// finite weights, 0 <= nbins <= NLH_MAXBINS, and with nbins > 0 a valid range (hist_range); *inv = 1 where nbins == 0
int quad_check(const double* weights, int nfields, double lo, double hi, int nbins, double* inv);
// Sums of increment powers (incr.hip): per field and separation S2, S3, S4 of d = x(z + sep) - x(z), rows periodic.  acc: device
// doubles, [slot][MFFT_INCR_MAXSEP][S2, S3, S4], six slots (nlz_incr.h NLI_SLOTS).
// incr_fold: acc[v] += the groups' part[g * nvals + v] added in a fixed order, nvals = whole slots
constexpr int INCR_FIELD = MFFT_INCR_MAXSEP * 3, INCR_SLOTS = 6 * INCR_FIELD;
int incr_fold(const double* part, size_t groups, int nvals, double* acc, hipStream_t s);
// MFFT_ERR_INVALID for nsep outside 1 .. MFFT_INCR_MAXSEP or a separation outside 1 .. m - 1
int incr_check(const int64_t* seps, int nsep, int64_t m);
// Histograms of the increments (incrhist.hip): per field and separation nbins + 3 counts of d = x(z + sep) - x(z) by hist_slot.  acc:
// device int64, [slot][nsep][nbins + 3], six slots; the fold is hist_fold_slots over rows of nsep (nbins + 3) counts.
size_t incr_hist_part_bytes(int ngroups, int nslots, int nsep, int nbins);
// inv = nbins / (hi - lo) of a valid range; MFFT_ERR_INVALID for nbins outside 1 .. MFFT_INCR_HIST_MAXBINS, hi <= lo, a range that is
// not finite
int incr_hist_range(double lo, double hi, int nbins, double* inv);
// Plane-averaged profiles along z (profiles.hip): per pair and position of the row the sums of d_a, d_b, d_a^2, d_b^2, d_a d_b over
// all rows (nlz_prof.h prof_add).  acc: device doubles, (npairs, 5, n), pairs in slot order.
// prof_fold: acc[v] += the nslots partial profiles part[g * nvals + v], added in a fixed order
int prof_fold(const double* part, size_t nslots, size_t nvals, double* acc, hipStream_t s);
// bytes of the partial profiles of a launch: one per row slot, ngroups x tile of them
size_t prof_part_bytes(int ngroups, int tile, int npairs, int64_t n);
// MFFT_ERR_INVALID for a centre that is not finite (center may be null: zeros)
int prof_check(const double* center, int nfields);
// max |x| reductions (absmax.hip): acc[s] = max(acc[s], scale * max_g part[g * period + s]), NaNs kept; `scratch` holds
// absmax_fold_scratch_bytes(), `part` is in precision `prec`, acc in double
size_t absmax_fold_scratch_bytes();
int absmax_fold(const void* part, size_t groups, int period, int prec, double scale, double* scratch, double* acc, hipStream_t s);

// strided 3-D box copy: dst[i][j][k] = src[i][j][k] over extents e0,e1,e2 with
// element strides (k contiguous); elem = bytes per element (8 or 16)
struct BoxArgs {
  const void* src = nullptr;
  void* dst = nullptr;
  int64_t e0 = 1, e1 = 1, e2 = 1;
  int64_t s0 = 0, s1 = 0;     // src strides of dims 0,1 (dim 2 contiguous)
  int64_t d0 = 0, d1 = 0;     // dst strides
  int elem = 16;
  int mode = 0;               // 0 copy, 1 accumulate (dst += src)
  double scale = 1.0;         // applied to src (complex/real agnostic)
  int prec = MFFT_DOUBLE;
};
int launch_box_copy(const BoxArgs& a, hipStream_t s);
// rows (nrows, pitch) of complex values: col0 <- (Re col0 - Im colN, 0), colN <- (Re colN, 0)   (line.py:231, 27-39)
int launch_line_nyquist(void* rows, int64_t nrows, int64_t pitch, int64_t coln, int prec, hipStream_t s);
int launch_mask(void* fu, const uint8_t* mask, size_t count, int prec, hipStream_t s);
int launch_scale(void* data, size_t count_real, double scale, int prec, hipStream_t s);
int launch_fill_uniform(void* data, size_t count, int prec, uint64_t seed, hipStream_t s);

bool length_supported(int64_t n, bool real_transform);
int length_route(int64_t n, bool real_transform, int prec = MFFT_DOUBLE);   // 1 radix plan, 2 one-workgroup chirp-z, 3 bigfft.hip, 0 none
// bigfft.hip: any length up to MFFT_BIG_MAX_LENGTH through Bluestein's convolution over a four-step power-of-two transform in
// a scratch buffer (the fallback behind the radix plans and the one-workgroup chirp-z kernels); plain transforms only
#define MFFT_BIG_MAX_LENGTH (1 << 20)
bool big_length_ok(int64_t n);
void big_release_stream(hipStream_t s);   // frees the scratch buffer bigfft.hip keeps for a stream (plan destruction)
bool radix_plan_exists(int contiguous, int64_t n, int prec);   // a plain strided (0) / contiguous-axis c2c (1) radix kernel of length n
int big_col(const ColArgs& a, hipStream_t s);
int big_row(const RowArgs& a, hipStream_t s);
int big_real(bool c2r, const RealArgs& a, hipStream_t s);
bool zsplit_supported(int64_t n, int prec, bool real_transform);   // radix kernels with fused z-chunk pack exist for n
bool zsplit_limit_supported(int64_t n, int prec);                  // ... that are column-limited as well (3/2-rule pencils)
hipStream_t plan_stream(mfft_plan_t plan);   // the plan's compute stream (nullptr plan -> default stream)

}  // namespace mfft
