/* mpifft4py_amd.h -- C ABI of libmpifft4py_amd.so
 *
 * MI355X-native (gfx950) distributed 3-D FFT: the drop-in boundary for the hot
 * path of spectralDNS/mpiFFT4py (slab / pencil R2C.fftn / ifftn).  The
 * reference has no C ABI of its own; its backend seam is the Python module
 * `mpiFFT4py/serialFFT` (serialFFT/__init__.py:1-6) plus the mpi4py
 * communicator handed to the constructors.  Every entry point below names the
 * reference interface it replaces.  The Python package `mpifft4py_amd` binds
 * this file with ctypes (mpifft4py_amd/_lib.py); INTEGRATION.md shows the stub
 * a reference maintainer would add.
 *
 * Conventions
 *   - plain C: pointers, sizes, ints.  No C++/torch types cross the boundary.
 *   - every function returns 0 on success or a negative mfft_status; the text of
 *     the last failure on the calling thread is mfft_last_error().
 *   - all data pointers are DEVICE pointers (HBM) unless named *_host.
 *   - arrays are C-order; complex = interleaved (re, im).
 *   - a plan is bound to the device current at creation and to one comm.
 */
#ifndef MPIFFT4PY_AMD_H
#define MPIFFT4PY_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MFFT_API __attribute__((visibility("default")))

typedef enum {
  MFFT_OK = 0,
  MFFT_ERR_INVALID = -1,      /* bad argument */
  MFFT_ERR_UNSUPPORTED = -2,  /* e.g. a transform length beyond mfft_length_supported */
  MFFT_ERR_HIP = -3,          /* HIP runtime failure */
  MFFT_ERR_RCCL = -4,         /* RCCL failure / library not loadable */
  MFFT_ERR_NOMEM = -5,
  MFFT_ERR_INTERNAL = -6
} mfft_status;

typedef enum { MFFT_SINGLE = 0, MFFT_DOUBLE = 1 } mfft_precision;     /* mpibase.py:133-137 */
typedef enum { MFFT_R2C = 0, MFFT_C2C = 1 } mfft_kind;                 /* slab.R2C / slab.C2C */
typedef enum { MFFT_SLAB = 0, MFFT_PENCIL_X = 1, MFFT_PENCIL_Y = 2 } mfft_decomp;
typedef enum { MFFT_DEALIAS_NONE = 0, MFFT_DEALIAS_2_3 = 1, MFFT_DEALIAS_3_2 = 2 } mfft_dealias;

typedef struct mfft_comm_s* mfft_comm_t;
typedef struct mfft_plan_s* mfft_plan_t;

/* ---- library / device ------------------------------------------------- */
MFFT_API int mfft_version(void);
MFFT_API const char* mfft_last_error(void);
MFFT_API int mfft_device_count(int* count);
MFFT_API int mfft_set_device(int device);
MFFT_API int mfft_get_device(int* device);
MFFT_API int mfft_device_name(char* buf, size_t buflen);
MFFT_API int mfft_device_sync(void);
MFFT_API int mfft_device_pci_bus_id(int device, char* buf, size_t buflen);   /* "0000:05:00.0": which physical GPU a rank ran on */

/* ---- device memory (replaces mpibase.py:38-51 empty/zeros and the
 *      work_arrays cache, mpibase.py:53-131, for device-resident buffers) ---
 * mfft_memset / mfft_memcpy_* wait for ALL work of the current device (the transforms run asynchronously on their
 * plan's own stream, see mfft_forward) before they touch memory and return when the copy is complete. */
MFFT_API int mfft_malloc(void** dptr, size_t bytes);
MFFT_API int mfft_free(void* dptr);
MFFT_API int mfft_memset(void* dptr, int value, size_t bytes);
MFFT_API int mfft_memcpy_h2d(void* dst, const void* src_host, size_t bytes);
MFFT_API int mfft_memcpy_d2h(void* dst_host, const void* src, size_t bytes);
MFFT_API int mfft_memcpy_d2d(void* dst, const void* src, size_t bytes);
/* rows of width_bytes, device rows dev_pitch_bytes apart <-> packed host rows: how numpy arrays of the reference's shapes
 * (slab.py:102-104) go into / come out of a pitched spectrum (mfft_plan_desc::complex_pitch) */
MFFT_API int mfft_memcpy_rows_h2d(void* dst, size_t dev_pitch_bytes, const void* src_host, size_t width_bytes, size_t rows);
MFFT_API int mfft_memcpy_rows_d2h(void* dst_host, const void* src, size_t dev_pitch_bytes, size_t width_bytes, size_t rows);
MFFT_API int mfft_fill_uniform(void* dptr, size_t count, int precision, uint64_t seed); /* U[0,1) synthetic input */

/* ---- communicators (replace the mpi4py Comm injected at slab.py:77-81,
 *      pencil.py:173-195: Get_size/Get_rank/Split + Alltoall(w)) ----------- */
#define MFFT_UNIQUE_ID_BYTES 128
MFFT_API int mfft_comm_create_self(mfft_comm_t* comm);                 /* P = 1, no RCCL */
MFFT_API int mfft_get_unique_id(void* id128);                           /* rank 0; ncclGetUniqueId */
MFFT_API int mfft_comm_create_rccl(int nranks, int rank, const void* id128, mfft_comm_t* comm);
/* in-process group: nranks virtual ranks, each driven by its own host thread,
 * rank r living on devices[r] (NULL = all on the current device); exchange is
 * peer-to-peer device copies. */
MFFT_API int mfft_comm_create_local(int nranks, const int* devices, mfft_comm_t* comms_out);
MFFT_API int mfft_comm_size(mfft_comm_t comm, int* size);
MFFT_API int mfft_comm_rank(mfft_comm_t comm, int* rank);
MFFT_API int mfft_comm_barrier(mfft_comm_t comm);
/* One small all-to-all of a known byte pattern over all ranks (collective), verified on the host, waiting at most
 * timeout_ms for the device: 0 = the transport moves data correctly here.  A hung IPC exchange is released from the
 * host and reported as an error instead of blocking forever. */
MFFT_API int mfft_comm_selftest(mfft_comm_t comm, size_t bytes_per_peer, int timeout_ms);
/* Transport knobs, per communicator.  The IPC transport (the stand-in for the MPI library's intra-node all-to-all,
 * slab.py:406/281, pencil.py:741-750) knows "ipc_pull" = how a rank fetches its chunks from the peers' buffers: 1 one
 * pull kernel over all peers at once (default), 2 one copy-engine transfer per peer on per-peer streams (EXPERIMENTAL: the one
 * mode that ever stalled -- twice, with ranks sharing a device, round 4 -- and that the default test run therefore does not sweep:
 * MP_WORKER_STREAMS=1 / MFFT_BENCH_PULL_STREAMS=1 add it; do not rely on it before it has run on a node with a GPU per rank), 0 copy-engine
 * transfers one after the other; and "ipc_pull_wgs" = workgroups per peer of that kernel.  A rank-local choice (the
 * flag protocol is the same).  "ipc_relay" = 1 / 0: sub-group exchanges of pencil plans use the links to the ranks
 * outside the group as well (mfft_plan_relay_schedule) -- every rank must set the same value.  Other transports reject
 * every key; get returns -1 in *value for an unknown key. */
MFFT_API int mfft_comm_set_option(mfft_comm_t comm, const char* key, int64_t value);
MFFT_API int mfft_comm_get_option(mfft_comm_t comm, const char* key, int64_t* value);
/* host-buffer helpers for tests/demos (tests/test_FFT.py:77-78 Bcast; demo:103 reduce) */
MFFT_API int mfft_comm_bcast_host(mfft_comm_t comm, void* buf_host, size_t bytes, int root);
MFFT_API int mfft_comm_allreduce_sum_host(mfft_comm_t comm, double* vals_host, int count);
MFFT_API int mfft_comm_allreduce_max_host(mfft_comm_t comm, double* vals_host, int count);
/* mark an in-process group broken so that ranks blocked in its barriers return an error
 * (called when one rank's thread fails); no-op for the other transports */
MFFT_API int mfft_comm_abort(mfft_comm_t comm);
MFFT_API int mfft_comm_destroy(mfft_comm_t comm);

/* ---- plans: slab.R2C / slab.C2C / pencil.R2CX / pencil.R2CY --------------
 * (constructors slab.py:67-96, 556-574; pencil.py:167-216, 903-913) */
typedef struct {
  int64_t n[3];       /* global real mesh N0,N1,N2 */
  int precision;      /* mfft_precision */
  int kind;           /* mfft_kind */
  int decomp;         /* mfft_decomp */
  int p1;             /* pencil: ranks along the first axis, 0 = Compute_dims default.  Any p1 that divides the number
                         of ranks is accepted (also 1 x P, P x 1 and odd grids); the reference, and the Python classes
                         by default, insist on even P1 and P2 (pencil.py:204-208) */
  double padsize;     /* 3/2-rule pad factor (1.5) */
  int pipeline;       /* exchange pipeline: slab: n > 1 = n kz slices, n < -1 = |n| batches of local x rows; x-aligned
                         pencil: |n| batches of local x rows; each piece is exchanged on a second stream while the
                         next one is transformed; 0 = default (4), 1 = off */
  int drop_nyquist;   /* pencil 'AlltoallN' mode (pencil.py:410-432, 647-668): the kz = N2/2 column is
                         neither exchanged nor returned; the inverse treats it as zero */
  int line2d;         /* 1: the 2-D class of line.py:41-340, expressed as an x-aligned pencil plan of the mesh
                         (1, Nx, Ny) on a 1 x P grid: padsize^2 scaling, no Nyquist fold on one rank (line.py:185)
                         and, for P > 1, the Nyquist packing of line.py:231 in the padded forward transform */
  int comm_cus;       /* pipelined plans: compute units set aside for the communication stream (the compute stream gets
                         the others): > 0 that many, 0 = $MFFT_COMM_CUS or the library default, < 0 = no CU masks.
                         CU-masked streams are BLOCKING streams (hipExtStreamCreateWithCUMask takes no flags): work
                         on the legacy null stream of the device then orders against the plan's streams, which the
                         plain (non-blocking) plan streams do not.  The library itself never relies on either. */
  int complex_pitch;  /* PITCHED SPECTRUM (round 6; SURVEY 7 "padded device pitch internally, exact Nf at the API boundary"): 0 =
                         the caller's complex array is compact, rows of the local z extent (Nf = N2/2 + 1 bins: 8208 bytes
                         at 1024^3, never a whole cache line); -1 = rows a whole number of 128-byte lines apart (513 -> 520
                         bins); n > 0 = rows n elements apart.  The logical shape stays the reference's (slab.py:102-104);
                         mfft_layout_complex_pitch says what to allocate.  One-rank slab R2C plans run every pass on the
                         pitched rows; all other plans convert at the boundary (one more pass, same results). */
  int reserved[3];
} mfft_plan_desc;

MFFT_API int mfft_plan_create(mfft_comm_t comm, const mfft_plan_desc* desc, mfft_plan_t* plan);
MFFT_API int mfft_plan_destroy(mfft_plan_t plan);
/* local shapes and global start offsets (slab.py:98-144, pencil.py:248-287, 915-943) */
MFFT_API int mfft_plan_layout(mfft_plan_t plan, int64_t real_shape[3], int64_t complex_shape[3],
                              int64_t real_start[3], int64_t complex_start[3],
                              int64_t real_shape_padded[3], int64_t grid[2], int64_t subranks[2]);
/* The same layout for rank `rank` of `nranks`, computed on the host WITHOUT a plan, a communicator or a device (the
 * decomposition bookkeeping of slab.py:82-144, pencil.py:187-287, 903-943 is integer arithmetic); it also rejects what
 * mfft_plan_create would reject (indivisible meshes, lengths without a kernel).  The Python classes build their shape,
 * slice and mesh helpers (slab.py:146-197, pencil.py:289-349) on it, so those work on a machine without a GPU. */
MFFT_API int mfft_layout_query(const mfft_plan_desc* desc, int nranks, int rank, int64_t real_shape[3],
                               int64_t complex_shape[3], int64_t real_start[3], int64_t complex_start[3],
                               int64_t real_shape_padded[3], int64_t grid[2], int64_t subranks[2]);
MFFT_API int mfft_layout_complex_pitch(const mfft_plan_desc* desc, int nranks, int rank, int64_t* pitch_elems, int64_t* alloc_elems);
MFFT_API int mfft_plan_workspace_bytes(mfft_plan_t plan, size_t* bytes);
/* The all-to-all-v a rank performs, computed on the host WITHOUT a device: the peer
 * list (world ranks, in group order) and byte counts / displacements of every chunk.
 * slab: which = 0.  pencil: which = 0 is the z-splitting exchange (uneven last chunk;
 * comm1 for X, comm0 for Y), which = 1 the other one.  It is the schedule the executor
 * itself uses; it describes what the reference expresses with Alltoall counts and the
 * Alltoallw sub-array types (slab.py:199-211, 406, 281; pencil.py:218-246, 971-999). */
MFFT_API int mfft_plan_exchange_schedule(const mfft_plan_desc* desc, int nranks, int rank, int which,
                                         int forward, int padded, int max_peers, int* npeers, int* peers,
                                         size_t* scount, size_t* sdisp, size_t* rcount, size_t* rdisp);
/* The same for ONE piece of the pipelined exchange that `desc->pipeline` selects (slab: kz slice or batch of local
 * x rows; x-aligned pencil: batch of local x rows of exchange `which`): displacements are relative to the whole send /
 * receive buffers, *npieces returns how many pieces the exchange has (1 = not pipelined: the whole exchange). */
MFFT_API int mfft_plan_exchange_pieces(const mfft_plan_desc* desc, int nranks, int rank, int which, int forward,
                                       int piece, int max_peers, int* npieces, int* npeers, int* peers,
                                       size_t* scount, size_t* sdisp, size_t* rcount, size_t* rdisp);

/* Relay striping of the pencils' sub-group exchanges over the IPC transport (csrc/relay_plan.h): on a fully connected
 * xGMI node a rank that exchanges with the g - 1 peers of its comm0 / comm1 group (pencil.py:741-750, 1324-1333) leaves
 * its links to the other P - g ranks idle; a message is therefore cut into a direct part and P - g stripes that travel
 * through those ranks in two hops.  This query lists, device-free, what `rank` PULLS in exchange `which`: phase (1, 2),
 * kind (0 own chunk, 1 direct part read from msg_src's send buffer, 2 first hop: rank is the relay and stages the stripe
 * of msg_src -> msg_dst, 3 second hop: read from relay `from`'s staging area), the offset inside the message and the
 * byte count.  It is the enumeration the transport executes when the "ipc_relay" option of mfft_comm_set_option (or
 * MFFT_IPC_RELAY=1) is on; the default is off. */
MFFT_API int mfft_plan_relay_schedule(const mfft_plan_desc* desc, int nranks, int rank, int which, int forward,
                                      int max_moves, int* nmoves, int* phase, int* kind, int* from, int* msg_src,
                                      int* msg_dst, size_t* msg_off, size_t* bytes);

/* mfft_forward / mfft_backward ENQUEUE the transform on the plan's own (non-blocking) HIP stream and return; calls on
 * one plan execute in order.  Before the host or another stream reads the result (or reuses the input), call
 * mfft_plan_sync -- or one of the mfft_memcpy_* helpers, which synchronise the device themselves.
 * fftn: slab.py:349-485 / pencil.py:634-883, 1228-1475.  `u` is never written. */
MFFT_API int mfft_forward(mfft_plan_t plan, const void* u, void* fu, int dealias);
/* ifftn: slab.py:214-346 / pencil.py:386-632, 1001-1224.  `fu` is never written. */
MFFT_API int mfft_backward(mfft_plan_t plan, const void* fu, void* u, int dealias);
/* block the host until everything the plan enqueued has finished */
MFFT_API int mfft_plan_sync(mfft_plan_t plan);

/* 2/3-rule mask (slab.py:191-197; applied by cython/maths.pyx:9-19): uint8 per local complex element, copied from
 * the host array.  mfft_backward(..., MFFT_DEALIAS_2_3) transforms `fu * mask` without writing fu: the first inverse
 * pass applies the mask while it loads.  A mask of the form get_dealias_filter builds (the product of three 1-D band
 * conditions) is recognised here and lets slab R2C plans run pruned passes and, over P ranks, a smaller exchange; the
 * ranks agree on that with a host all-reduce, so for plans over more than one rank this call is COLLECTIVE. */
MFFT_API int mfft_plan_set_dealias_mask(mfft_plan_t plan, const uint8_t* mask_host, size_t count);

/* What a plan decided, by key: "pruned_route" (after mfft_plan_set_dealias_mask: 0 = the mask is applied on load,
 * 1 = pruned passes and a smaller exchange, 2 = the same with every ky of THIS rank removed), "comm_cus" (CUs set aside
 * for the communication stream, 0 = no masks), "kz_slices", "row_batches" (pieces of the exchange pipeline), "zfuse"
 * (pencils: z-chunk pack fused into the z transform), "ranks", "plane_pad" (one-rank slab plans: elements added to the
 * plane pitch of the intermediate because the mesh's own plane pitch is one the strided x pass reads slowly),
 * "split_last" (one-rank slab R2C plans: 1 = the plain transforms split real / complex at the spectrum end, MFFT_SPLIT_LAST;
 * asked before the first transform, the key decides then whether the route's work buffer fits), "split_last_yblock",
 * "split_last_row_pitch", "split_last_block_pitch" (that route's work array: rows per y block, elements between the x rows of a
 * block and between blocks; 0 where the plan does not take the route), "split_last_yfirst" (1: its y passes carry the caller's
 * arrays, both x passes run in place on the work array), "work_bytes" (bytes of the first work buffer as allocated so far).
 * Unknown keys are MFFT_ERR_INVALID. */
MFFT_API int mfft_plan_get_info(mfft_plan_t plan, const char* key, int64_t* value);

/* per-stage timing with HIP events on the plan's own streams (bench roofline) */
MFFT_API int mfft_plan_timing(mfft_plan_t plan, int enable);
MFFT_API int mfft_plan_timing_reset(mfft_plan_t plan);
/* returns number of stages; arrays may be NULL to query the count */
MFFT_API int mfft_plan_timing_get(mfft_plan_t plan, int max_stages, char names[][32],
                                  double* total_ms, int64_t* calls, double* alg_bytes_per_call);

/* ---- stage level: the serialFFT seam (numpy_fft.py:25-107 / pyfftw_fft.py:26-203)
 * batched transforms of one axis of a contiguous C-order 3-D array on the
 * current device, default stream; synchronous w.r.t. the host on return. */
MFFT_API int mfft_c2c_axis(const void* in, void* out, const int64_t shape[3], int axis,
                           int inverse, int precision);                 /* fft / ifft  (ifft scaled 1/n) */
/* the same along a strided axis with every stride spelled out (a non-contiguous view in numpy's terms): `nouter` batches
 * in_outer / out_outer elements apart, each `ncols` contiguous columns wide, rows in_pitch / out_pitch elements apart */
MFFT_API int mfft_c2c_strided(const void* in, void* out, int64_t n, int64_t nouter, int64_t ncols, int64_t in_outer,
                              int64_t in_pitch, int64_t out_outer, int64_t out_pitch, int inverse, int precision);
MFFT_API int mfft_r2c_last(const void* in, void* out, const int64_t real_shape[3], int precision);    /* rfft axis=2 */
MFFT_API int mfft_c2r_last(const void* in, void* out, const int64_t real_shape[3], int precision);    /* irfft axis=2, scaled 1/n */
/* The fused nonlinear z stage on its own (csrc/fft_nlz.h; the z stages of mfft_nonlinear_cross): a, b, out are
 * (3, nrows, pitch) complex arrays of half-spectra rows of real length n of which the first `valid` bins exist
 * (n/2 + 1, or fewer: 3/2-rule); out_f[row] = rfft((irfft(a[:, row]) x irfft(b[:, row]))_f)[:valid], irfft as numpy's.
 * out may be a or b.  sync = 0: enqueued on the default stream and left running (timing loops).  Replaces the z stages
 * of six FFT.ifftn + three FFT.fftn around the demo's cross product (demo/spectral_dns_solver.py:53-71). */
MFFT_API int mfft_nlz_rows(const void* a, const void* b, void* out, int64_t nrows, int64_t n, int64_t pitch, int64_t valid,
                           int precision, int sync);
/* The same stage with the DOT product (the z stages of mfft_nonlinear_dot): a, b are (3, nrows, pitch) as above, out is ONE
 * (nrows, pitch) array; out[row] = rfft(sum_f irfft(a[f, row]) irfft(b[f, row]))[:valid].  out may be any one component of a
 * or b.  MFFT_ERR_UNSUPPORTED for lengths without a kernel.  Replaces the z stages of six FFT.ifftn + one FFT.fftn around
 * a caller's np.sum(U * gradT, 0). */
MFFT_API int mfft_nlz_dot_rows(const void* a, const void* b, void* out, int64_t nrows, int64_t n, int64_t pitch, int64_t valid,
                               int precision, int sync);
/* The same stage with BOTH products (the z stages of mfft_nonlinear_cross_dot): a, b, c, out are (3, nrows, pitch) as above, s
 * is ONE (nrows, pitch) array; out_f[row] = rfft((irfft(a[:, row]) x irfft(b[:, row]))_f)[:valid] and s[row] =
 * rfft(sum_f irfft(a[f, row]) irfft(c[f, row]))[:valid], with irfft(a) computed once.  out may be a or b, s any one component
 * of a, b or c that out does not take.  MFFT_ERR_UNSUPPORTED for lengths without a kernel.  Replaces the z stages of nine
 * FFT.ifftn + four FFT.fftn around a caller's np.cross(U, W) and np.sum(U * gradT, 0). */
MFFT_API int mfft_nlz_cross_dot_rows(const void* a, const void* b, const void* c, void* out, void* s, int64_t nrows, int64_t n,
                                     int64_t pitch, int64_t valid, int precision, int sync);
/* The same stage with the OUTER product (the z stages of mfft_nonlinear_outer): a, b are (3, nrows, pitch) as above, out is
 * (9, nrows, pitch); out[3 i + j][row] = rfft(irfft(a[i, row]) irfft(b[j, row]))[:valid], all nine.  out's components 0..5 may be
 * the six input components (a's three, then b's three), row for row -- every load of a row precedes its first store --;
 * components 6..8 may not be an input.  MFFT_ERR_UNSUPPORTED for lengths without a kernel.  Replaces the z stages of six
 * FFT.ifftn + nine FFT.fftn around a caller's A[:, None] * B[None, :]. */
MFFT_API int mfft_nlz_outer_rows(const void* a, const void* b, void* out, int64_t nrows, int64_t n, int64_t pitch, int64_t valid,
                                 int precision, int sync);
/* Either stage with the maxima of its six real rows, synchronous: `out` as mfft_nlz_rows (dot = 0) or mfft_nlz_dot_rows
 * (dot = 1) leave it, and out6 = [max |irfft(a[f])|, f = 0..2, then max |irfft(b[f])|, f = 0..2] over all rows and all n
 * points (numpy's normalisation).  A NaN in a field gives NaN for that field.  The z stage of mfft_nonlinear_cross_absmax /
 * mfft_nonlinear_dot_absmax on its own, for tests. */
MFFT_API int mfft_nlz_rows_absmax(const void* a, const void* b, void* out, int64_t nrows, int64_t n, int64_t pitch, int64_t valid,
                                  int precision, int dot, double out6[6]);
/* The z stage that ends in a reduction (csrc/nlz_moments.h NlzMoments::body), synchronous: the one-point statistics of the real rows
 * irfft(row, n) without the real rows.  nfields = 1: a is (nrows, pitch) complex; 2: a and b are; 3: a is (3, nrows, pitch), b
 * NULL; 6: a and b are.  `valid` bins per row exist, the first valid_in of them are read (0: all).  Per field, over all rows and
 * all n points (numpy's normalisation):  out[f * 6 + 0] = min, [1] = max, [2 + p - 1] = sum (x - center[f])^p, p = 1..4 (center
 * NULL: zeros); fields in the order a_0.., then b_0...  Powers and sums in double in both precisions.  A NaN or Inf bin of a field
 * gives NaN sums and NaN / +-Inf extremes for THAT field; the others stay right.  Bitwise reproducible run to run on one device.
 * MFFT_ERR_UNSUPPORTED for lengths without a kernel, MFFT_ERR_INVALID for valid > n / 2 + 1.  The z stage of mfft_real_moments on
 * its own, for tests.
 * mfft_nlz_moments_groups: the workgroups of that launch (it strides over the rows; 0: no kernel of that length). */
MFFT_API int mfft_nlz_moments_rows(const void* a, const void* b, int nfields, int64_t nrows, int64_t n, int64_t pitch, int64_t valid,
                                   int64_t valid_in, int precision, const double* center, double* out);
MFFT_API int64_t mfft_nlz_moments_groups(int64_t nrows, int64_t n, int precision);
/* Histograms: the slot rule that the host, the sweep, the fused kernel and the tests share.  For a real value x (numpy's
 * normalisation, taken to double in both precisions), a field's lo < hi (both finite) and 1 <= nbins <= MFFT_HIST_MAXBINS:
 *     inv  = nbins / (hi - lo)            formed once on the host, in double
 *     t    = (x - lo) * inv               a subtraction, then a multiplication
 *     slot = x != x      ? nbins + 2      not finite; tested first
 *          : t <  0      ? 0              below lo (-Inf lands here)
 *          : t >= nbins  ? nbins + 1      at or above hi (+Inf lands here); compared before the cast to int
 *          :               1 + (int)t
 * A result is nbins + 3 int64 counts per field; they always sum to the number of points. */
#define MFFT_HIST_MAXBINS 512
/* The z stage that ends in a histogram (csrc/nlz_hist.h NlzHist::body), synchronous: the histograms of the real rows irfft(row, n)
 * without the real rows.  Fields, rows, valid and valid_in as mfft_nlz_moments_rows; lo[f], hi[f] per field, in the order a_0..,
 * then b_0..; out[f * (nbins + 3) + slot].  Counts are integers: bitwise reproducible, whatever the launch looks like.  A NaN or
 * Inf bin of a field puts at least one count into THAT field's slot nbins + 2, its slots still sum to nrows * n; every other
 * field, the partner on the same transform included, has exactly the counts of the run without the bad bin.
 * MFFT_ERR_UNSUPPORTED for lengths without a kernel, MFFT_ERR_INVALID for nbins outside 1 .. MFFT_HIST_MAXBINS, hi <= lo and
 * valid > n / 2 + 1.  The z stage of mfft_real_histogram on its own, for tests.
 * mfft_nlz_hist_groups: the workgroups of that launch (it strides over the rows; 0: no kernel of that length). */
MFFT_API int mfft_nlz_hist_rows(const void* a, const void* b, int nfields, int64_t nrows, int64_t n, int64_t pitch, int64_t valid,
                                int64_t valid_in, int precision, const double* lo, const double* hi, int nbins, int64_t* out);
MFFT_API int64_t mfft_nlz_hist_groups(int64_t nrows, int64_t n, int precision);
/* Joint histograms: the cell rule that the host, the sweep, the fused kernel and the tests share.  For a pair of real values
 * (x_a, x_b) of the same grid point, normalised as in the histograms; each field has its own lo < hi (both finite) and its own bin
 * count, 1 <= nba, nbb <= MFFT_JOINT_MAXBINS; inv_a = nba / (hi_a - lo_a) and inv_b = nbb / (hi_b - lo_b) are formed once on the
 * host, in double:
 *     sa   = slot(x_a, lo_a, inv_a, nba)      the slot rule above, unchanged: 0 below, 1 .. nba, nba + 1 above, nba + 2 not finite
 *     sb   = slot(x_b, lo_b, inv_b, nbb)
 *     cell = sa * (nbb + 3) + sb
 * A pair's result is (nba + 3) * (nbb + 3) int64 counts; they always sum to the number of points.  A non-finite bin of a spectrum
 * marks ITS field's slot only: the bad field goes to nba + 2 (or nbb + 2), the partner keeps its exact slot.  64 bins per field
 * is what a workgroup can hold next to its exchange buffers: (64 + 3)^2 x 4 = 17956 bytes of LDS.  A finer PDF is had by a second
 * call on a narrower range. */
#define MFFT_JOINT_MAXBINS 64
/* The z stage that ends in a joint histogram (csrc/nlz_joint.h NlzJoint::body), synchronous: a and b are (ncomp, nrows, pitch) complex
 * rows, ncomp 1 or 3; pair p is (a_p, b_p), both ride ONE inverse transform.  Rows, valid and valid_in as mfft_nlz_hist_rows; lo
 * and hi have 2 ncomp entries in the order a_0.., then b_0..; out[p * cells + cell], cells = (nba + 3)(nbb + 3).  Integers: bitwise
 * reproducible, whatever the launch looks like.  MFFT_ERR_UNSUPPORTED for lengths without a kernel; MFFT_ERR_INVALID for a bin count
 * outside 1 .. MFFT_JOINT_MAXBINS, hi <= lo, ranges that are not finite, a NULL b and valid > n / 2 + 1: reported before anything
 * is enqueued, out untouched.  The z stage of mfft_real_joint_histogram on its own, for tests.
 * mfft_nlz_joint_groups: the workgroups of that launch (it strides over the rows; 0: no kernel of that length). */
MFFT_API int mfft_nlz_joint_rows(const void* a, const void* b, int ncomp, int64_t nrows, int64_t n, int64_t pitch, int64_t valid,
                                 int64_t valid_in, int precision, const double* lo, const double* hi, int nba, int nbb, int64_t* out);
MFFT_API int64_t mfft_nlz_joint_groups(int64_t nrows, int64_t n, int precision);
/* Quadratic forms: the evaluation rule that the fused kernel, the sweeps, the emulator and the tests share.  For n = 1, 2, 3 or 6
 * real fields r_f at a point and weights w_f (finite doubles of either sign):
 *     r_f = (double)v * norm                          the transform's value in the plan's precision, taken to double, then
 *                                                     normalised (a real array that is given as such: r_f = (double)x)
 *     q   = 0
 *     q   = q + (w_f * r_f) * r_f                     for each field in SLOT order (a alone: a_0, a_1, ..; a and b: a_0, b_0, a_1,
 *                                                     b_1, a_2, b_2 -- the pairs that share a transform)
 * Every product and every sum is rounded on its own, in double: nothing is contracted into a fused multiply-add, on the device
 * or on the host.  q is a double in both precisions; its statistics are the six of mfft_real_moments about one centre, its counts
 * follow the slot rule above with one lo < hi. */
/* The z stage that ends in the statistics of a quadratic form (csrc/nlz_quad.h NlzQuad::body), synchronous: q over the real rows
 * irfft(row, n) of the fields without the real rows.  Fields, rows, valid and valid_in as mfft_nlz_moments_rows; weights[f] in the
 * order a_0.., then b_0..; out6 = [min, max, S1 .. S4] of q, S_p = sum (q - center)^p; counts[nbins + 3] by the slot rule (may be
 * NULL where nbins == 0).  A NaN or Inf bin in ANY field makes q NaN where that bin was loaded: NaN sums, NaN min and max, counts
 * in slot nbins + 2.  MFFT_ERR_INVALID for nbins outside 0 .. MFFT_HIST_MAXBINS, a weight or centre that is not finite, and with
 * nbins > 0 hi <= lo; MFFT_ERR_UNSUPPORTED for lengths without a kernel; the outputs are untouched on error.  The z stage of
 * mfft_real_quadratic on its own, for tests.  mfft_nlz_quad_groups: the workgroups of that launch (0: no kernel of that length). */
MFFT_API int mfft_nlz_quad_rows(const void* a, const void* b, int nfields, int64_t nrows, int64_t n, int64_t pitch, int64_t valid,
                                int64_t valid_in, int precision, const double* weights, double center, double lo, double hi, int nbins,
                                double* out6, int64_t* counts);
MFFT_API int64_t mfft_nlz_quad_groups(int64_t nrows, int64_t n, int precision);
/* Structure functions along z: the rule that the fused kernel, the sweep, the emulator and the tests share.  For a real z row of
 * length M (N2 for dealias None and the 2/3-rule, 3 N2 / 2 for the 3/2-rule) and a separation s, 1 <= s <= M - 1, in grid points of
 * that row, periodic:
 *     r(z) = (double)v(z) * norm          the transform's value in the plan's precision, taken to double, then normalised (one
 *                                         rounded product; a real array that is given as such: r = (double)x)
 *     d    = r((z + s) mod M) - r(z)
 *     d2 = d * d;   S2 += d2;   S3 += d2 * d;   S4 += d2 * d2
 * Powers and sums in double in both precisions, over all rows and all M positions; S1 is identically zero on a periodic row and
 * is not computed.  Per field and separation the result is three doubles, [S2, S3, S4].  One launch takes up to MFFT_INCR_MAXSEP
 * separations; duplicates are allowed. */
#define MFFT_INCR_MAXSEP 8
/* The z stage that ends in structure functions (csrc/nlz_incr.h NlzIncr::body), synchronous: the increment sums of the real rows
 * irfft(row, n) without the real rows.  Fields, rows, valid and valid_in as mfft_nlz_moments_rows; out[(f * nsep + i) * 3 + {0, 1,
 * 2}] = S2, S3, S4 of field f at seps[i], fields in the order a_0.., then b_0...  No atomics: bitwise reproducible run to run.  A
 * NaN or Inf bin of a field makes all of THAT field's sums NaN; the partner on the same transform stays exact.
 * MFFT_ERR_INVALID for nsep outside 1 .. MFFT_INCR_MAXSEP and any seps[i] < 1 or >= n; MFFT_ERR_UNSUPPORTED for lengths without a
 * kernel; reported before anything is enqueued, the outputs untouched.  The z stage of mfft_real_increments on its own, for tests.
 * mfft_nlz_incr_groups: the workgroups of that launch (it strides over the rows; 0: no kernel of that length). */
MFFT_API int mfft_nlz_incr_rows(const void* a, const void* b, int nfields, int64_t nrows, int64_t n, int64_t pitch, int64_t valid,
                                int64_t valid_in, int precision, const int64_t* seps, int nsep, double* out);
MFFT_API int64_t mfft_nlz_incr_groups(int64_t nrows, int64_t n, int precision);
/* Increment PDFs along z: the ONE rule that the fused kernel, the sweep, the emulator, numpy (spectral.incr_hist_rule) and the tests
 * share.  For a real z row of length M and a separation s, 1 <= s <= M - 1, periodic:
 *     r(z) = (double)v(z) * norm          the increments' value rule above (one rounded product; a real array: r = (double)x)
 *     d    = r((z + s) mod M) - r(z)      in double
 *     slot = the histograms' unchanged slot rule applied to d with lo[f][i], inv[f][i] = nbins / (hi[f][i] - lo[f][i]):
 *            d is NaN -> nbins + 2;  t = (d - lo) * inv;  t < 0 -> 0;  t >= nbins -> nbins + 1;  else 1 + (int)t
 * Every field f and every separation i has its own lo < hi.  Per (field, separation) the result is nbins + 3 int64 counts: below lo,
 * the nbins equal bins of [lo, hi), at or above hi, not finite; they always sum to the points.  1 <= nbins <=
 * MFFT_INCR_HIST_MAXBINS, at most MFFT_INCR_MAXSEP separations per launch (duplicates allowed), increments along z only.  Counts
 * are integers: the same bits run to run and for every number of ranks that computes the same values. */
#define MFFT_INCR_HIST_MAXBINS 256
/* The z stage that ends in increment histograms (csrc/nlz_incr_hist.h NlzIncrHist::body), synchronous: the counts of the increments of the
 * real rows irfft(row, n) without the real rows.  Fields, rows, valid and valid_in as mfft_nlz_moments_rows; lo, hi: [(f * nsep + i)],
 * fields in the order a_0.., then b_0..; out[(f * nsep + i) * (nbins + 3) + slot].  No global atomics: a workgroup counts in LDS,
 * stores its rows by plain stores, one fold in fixed order into int64.  A thread whose load took a NaN or Inf bin out of a field
 * counts its own increments of THAT field in slot nbins + 2; the partner on the same transform keeps its exact counts.
 * MFFT_ERR_INVALID for nbins outside 1 .. MFFT_INCR_HIST_MAXBINS, nsep outside 1 .. MFFT_INCR_MAXSEP, any seps[i] < 1 or >= n, hi <=
 * lo or a range that is not finite, valid > n / 2 + 1; MFFT_ERR_UNSUPPORTED for lengths without a kernel; reported before anything is
 * enqueued, the outputs untouched.  The z stage of mfft_real_increment_histogram on its own, for tests.
 * mfft_nlz_incr_hist_groups: the workgroups of that launch (it strides over the rows; 0: no kernel of that length). */
MFFT_API int mfft_nlz_incr_hist_rows(const void* a, const void* b, int nfields, int64_t nrows, int64_t n, int64_t pitch, int64_t valid,
                                     int64_t valid_in, int precision, const int64_t* seps, int nsep, const double* lo, const double* hi,
                                     int nbins, int64_t* out);
MFFT_API int64_t mfft_nlz_incr_hist_groups(int64_t nrows, int64_t n, int precision);
/* Plane-averaged profiles along z: the rule that the fused kernel, the sweep, the emulator and the tests share.  For a pair of real
 * fields (x, y), the centres (ca, cb) and every z index m of the real row of length M (N2 for dealias None and the 2/3-rule,
 * 3 N2 / 2 for the 3/2-rule), over all rows -- a row is one (x, y) point, so over the plane z = m:
 *     r    = (double)v * norm             the transform's value in the plan's precision, taken to double, then normalised (one
 *                                         rounded product, as for the increments; a real array that is given as such: r = (double)x)
 *     da = r_x - ca;   db = r_y - cb
 *     sums[0] += da;  sums[1] += db;  sums[2] += da * da;  sums[3] += db * db;  sums[4] += da * db
 * Products and sums in double in both precisions.  Per pair and z index the result is MFFT_PROFILE_STATS doubles.  No atomics:
 * partial profiles go out by plain stores and are added in a fixed order, so the sums are bitwise reproducible run to run; they
 * are sums of doubles, so they are NOT claimed identical for different numbers of ranks. */
#define MFFT_PROFILE_STATS 5
/* The z stage that ends in profiles (csrc/nlz_prof.h NlzProf::body), synchronous: a and b are (ncomp, nrows, pitch) complex device arrays,
 * ncomp = 1 or 3, pair p = (a_p, b_p); rows, valid and valid_in as mfft_nlz_moments_rows; center: 2 ncomp centres, a_0.., then
 * b_0.. (NULL: zeros).  out[(p * 5 + s) * n + m] = sum s of pair p at position m of the rows irfft(row, n), without the real rows.
 * A NaN or Inf bin of a field makes that field's two sums and the cross sum NaN at the positions of the thread that loaded it; the
 * partner's own two sums keep the bytes of the run with that bin zero.  MFFT_ERR_INVALID for ncomp outside {1, 3}, a NULL b, a
 * centre that is not finite and valid > n / 2 + 1; MFFT_ERR_UNSUPPORTED for lengths without a kernel; reported before anything is
 * enqueued, out untouched.  The z stage of mfft_real_profiles on its own, for tests.
 * mfft_nlz_profile_groups: the workgroups of that launch (it strides over the rows; 0: no kernel of that length). */
MFFT_API int mfft_nlz_profile_rows(const void* a, const void* b, int ncomp, int64_t nrows, int64_t n, int64_t pitch, int64_t valid,
                                   int64_t valid_in, int precision, const double* center, double* out);
MFFT_API int64_t mfft_nlz_profile_groups(int64_t nrows, int64_t n, int precision);
/* slab pack / unpack (slab.py:403; cython/maths.pyx:21-31 transpose_Uc) */
MFFT_API int mfft_slab_pack(const void* uc_hatT, void* u_mpi, int P, int64_t np0, int64_t np1, int64_t nf, int precision);
MFFT_API int mfft_slab_unpack(const void* u_mpi, void* uc_hatT, int P, int64_t np0, int64_t np1, int64_t nf, int precision);
/* fu[i] *= mask[i] (cython/maths.pyx:9-19 dealias_filter) */
MFFT_API int mfft_dealias_filter(void* fu, const uint8_t* mask_dev, size_t count, int precision);
/* 1 if a transform of length n along an axis is supported -- every n from 1 to 2^20, as numpy.fft / FFTW, the reference's
 * backends, take every n (numpy_fft.py:25-46).  mfft_length_route tells HOW: 1 = a radix plan (one kernel, register-resident:
 * 2^a <= 8192, 3*2^a <= 6144, 5*2^a <= 5120, 7*2^a <= 7168, 9*2^a <= 4608, 21*2^a <= 2688, 63*2^a <= 2016, 25*2^a <= 1600, 27*2^a <= 3456, 81*2^a <= 2592,
 * 125*2^a <= 2000, 15*2^a <= 3840, 45*2^a <= 1440, 75*2^a <= 2400, 135*2^a <= 2160, 225*2^a <= 1800, 375*2^a <= 3000, 675*2^a <= 2700,
 * 1125*2^a <= 2250, in single precision also 35*2^a <= 2240; real: twice that), 2 = the one-workgroup chirp-z kernels
 * (every other length up to 4096, even real lengths up to 8192; ~0.17 of the roofline), 3 = Bluestein's convolution over a
 * four-step power-of-two transform in a scratch buffer (csrc/bigfft.hip: every other length; plain transforms only -- the
 * 3/2-rule and 2/3-rule then take their copy-based routes; ~0.05 - 0.1 of the roofline), 0 = not supported (n > 2^20). */
MFFT_API int mfft_length_supported(int64_t n, int real_transform);
MFFT_API int mfft_length_route(int64_t n, int real_transform);
/* ... for one precision: the 35 * 2^a lengths have radix plans in single precision only (mfft_length_route answers for double) */
MFFT_API int mfft_length_route_precision(int64_t n, int real_transform, int precision);
/* Which compiled kernel a strided-axis (family 0), contiguous-axis c2c (1), r2c (2) or c2r (3) transform of length n
 * runs: "<plan name> tile=<columns or rows> threads=<n> lds=<bytes>[ nt]", e.g.
 * "cols n1024(8, 8, 4, 4)double tile=8 threads=1024 lds=81792".  Device-free.  bench.py uses it to check that a
 * committed rocprof profile belongs to the kernel it has just timed.  Returns MFFT_ERR_UNSUPPORTED for lengths that
 * go through the chirp-z kernels. */
MFFT_API int mfft_kernel_name(int family, int64_t n, int precision, int inverse, int nt, char* buf, size_t buflen);

/* ---- element-wise pieces of a pseudo-spectral Navier-Stokes step on device-resident
 * fields (what the reference demo does with numpy on the host,
 * demo/spectral_dns_solver.py:53-80).  Vector fields are (3, n) component-major; kx/ky/kz
 * are 1-D device vectors of the local spectral extents shape[0..2].  Enqueued on the
 * plan's stream (in order with its transforms); plan may be NULL (default stream). */
MFFT_API int mfft_ew_cross(mfft_plan_t plan, const void* a, const void* b, void* out, size_t n, int precision);          /* demo:53-58 */
MFFT_API int mfft_ew_curl_hat(mfft_plan_t plan, const void* U_hat, void* out, const void* kx, const void* ky, const void* kz,
                              const int64_t shape[3], int precision);                                   /* demo:60-64 */
/* out = sum_f a_f b_f on real fields, a and b (3, n) component-major, out (n): what a caller writes as np.sum(a * b, 0);
 * out may be a component of a or b */
MFFT_API int mfft_ew_dot(mfft_plan_t plan, const void* a, const void* b, void* out, size_t n, int precision);
/* out = a b on real fields of n values: ONE product a_i b_j of the composed outer product; out may be a or b */
MFFT_API int mfft_ew_mul(mfft_plan_t plan, const void* a, const void* b, void* out, size_t n, int precision);
/* The right-hand sides of incompressible MHD in Elsasser variables z+- = u +- b in ONE sweep.  T_hat is (9,) + shape, the nine
 * products T[3 i + j] = fftn(z+_i z-_j) of mfft_nonlinear_outer(Zp_hat, Zm_hat); Zp_hat, Zm_hat, dZp, dZm are (3,) + shape.  Per bin
 *     N+_i = -i sum_j K_j T[3 i + j],   N-_i = -i sum_j K_j T[3 j + i],   each projected: N - K (K . N) / |K|^2 (0 at K = 0),
 *     dZ+-_i = N+-_i - |K|^2 (np Z+-_i + nm Z-+_i),   np = (nu + eta) / 2,  nm = (nu - eta) / 2.
 * dZp and dZm are arrays of their own (MFFT_ERR_INVALID where one is an input or the other).  kx / ky / kz and `shape` as for
 * mfft_ew_curl_hat (pitched spectra: shape[2] = the row pitch, swept as they lie). */
MFFT_API int mfft_ew_elsasser_rhs(mfft_plan_t plan, const void* T_hat, const void* Zp_hat, const void* Zm_hat, void* dZp, void* dZm,
                                  const void* kx, const void* ky, const void* kz, const int64_t shape[3], double nu, double eta,
                                  int precision);
/* out_f = i K_f s_hat, the gradient of a scalar in spectral space: s_hat has `shape`, out is (3,) + shape; kx / ky / kz and
 * `shape` as for mfft_ew_curl_hat (pitched spectra: shape[2] = the row pitch, kz padded to it).  What a caller writes as
 * 1j * K * s_hat. */
MFFT_API int mfft_ew_grad_hat(mfft_plan_t plan, const void* s_hat, void* out, const void* kx, const void* ky, const void* kz,
                              const int64_t shape[3], int precision);
/* out_f = i K_f U_hat_f, the three LONGITUDINAL derivatives du_f / dx_f of a vector field in spectral space (the field whose
 * skewness a DNS is judged by): U_hat and out are (3,) + shape; the rest as mfft_ew_grad_hat.  What a caller writes as
 * 1j * K * U_hat. */
MFFT_API int mfft_ew_diag_grad_hat(mfft_plan_t plan, const void* U_hat, void* out, const void* kx, const void* ky, const void* kz,
                                   const int64_t shape[3], int precision);
/* The strain-rate tensor S_ij = (du_i/dx_j + du_j/dx_i) / 2 of a vector field in spectral space, U_hat read ONCE: diag_f =
 * i K_f U_hat_f (S_00, S_11, S_22) and off = (S_01, S_02, S_12) with S_ij = i (K_i U_hat_j + K_j U_hat_i) / 2; U_hat, diag and off
 * are (3,) + shape and distinct; the rest as mfft_ew_grad_hat (pitched spectra are swept as they lie).  The dissipation is
 * 2 nu S_ij S_ij = mfft_real_quadratic(diag, off, weights = 2 nu (1, 1, 1, 2, 2, 2)). */
MFFT_API int mfft_ew_strain_hat(mfft_plan_t plan, const void* U_hat, void* diag, void* off, const void* kx, const void* ky, const void* kz,
                                const int64_t shape[3], int precision);
MFFT_API int mfft_ew_ns_rhs(mfft_plan_t plan, void* dU, const void* U_hat, const void* kx, const void* ky, const void* kz,
                            const int64_t shape[3], double nu, int precision);                          /* demo:73-77 */
MFFT_API int mfft_ew_axpbz(mfft_plan_t plan, void* y, const void* x, const void* z, double alpha, double beta, size_t n_real,
                           int precision);                                                              /* demo:94-97 */
/* One Runge-Kutta stage of the demo's loop in one sweep (demo:73-77 compute_rhs' projection and viscous term, :94-97 the two
 * updates, :60-64 the curl the NEXT stage transforms): on entry N_hat holds the nonlinear term (mfft_nonlinear_cross);
 *   dU = N_hat - K (K . N_hat)/|K|^2 - nu |K|^2 U_hat;   U_hat1 += a_dt dU;
 *   last == 0: U_hat = U_hat0 + b_dt dU        last != 0: U_hat = U_hat0 = U_hat1   (the next step's `U_hat1[:] = U_hat0[:] = U_hat`)
 *   N_hat = i K x U_hat (new).
 * All four fields (3,) + shape, component-major; a_dt = a[rk] dt, b_dt = b[rk] dt. */
MFFT_API int mfft_ew_ns_rk_stage(mfft_plan_t plan, void* N_hat, void* U_hat, void* U_hat0, void* U_hat1, const void* kx,
                                 const void* ky, const void* kz, const int64_t shape[3], double nu, double a_dt, double b_dt,
                                 int last, int precision);
MFFT_API int mfft_ew_sumsq(mfft_plan_t plan, const void* x, size_t n_real, int precision, double* result_host);           /* demo:103 */
/* out_host[c] = max |x[c, :]| of a real device array (ncomp, n), ncomp = 1, 2, 3 or 6, in the plan's precision: np.abs(x).max(1).
 * One sweep, 16 bytes per lane, no atomics; a NaN in a component gives NaN for it; bitwise reproducible.  The plan must not be
 * null (partial maxima live in a buffer of the plan); synchronises the plan's stream. */
MFFT_API int mfft_ew_absmax(mfft_plan_t plan, const void* x, int ncomp, size_t n, int precision, double* out_host);

/* out_host[c * 6 + {0: min, 1: max, 2..5: S1..S4}] of a real device array (ncomp, n), ncomp = 1, 2, 3 or 6, in the plan's
 * precision; S_p = sum (x[c, :] - center[c])^p, center NULL: zeros.  The companion of mfft_ew_absmax / mfft_ew_sumsq: one
 * sweep, 16 bytes per lane, powers and sums in double, no atomics, bitwise reproducible; a NaN in a component gives NaN in all six
 * of its statistics.  The plan must not be null; synchronises the plan's stream. */
MFFT_API int mfft_ew_moments(mfft_plan_t plan, const void* x, int ncomp, size_t n, int precision, const double* center, double* out_host);

/* One-point statistics of fields that exist as spectra only: for the ncomp (1 or 3) components of a_hat and, where b_hat is not
 * NULL, of b_hat -- 1, 2, 3 or 6 fields, in that order --
 *     out[f * 6 + 0] = min x,  [1] = max x,  [2 + p - 1] = sum (x - center[f])^p, p = 1..4,     x = ifftn(field f, dealias)
 * over THIS RANK's part of the real-space grid (the padded grid under the 3/2-rule, the masked field under the 2/3-rule, as
 * mfft_nonlinear_cross_absmax), *count = the points summed.  center NULL: zeros; a centre near the mean keeps the digits of the
 * central moments (about 0 they cancel as (mean / sigma)^p).  The routes are those of mfft_nonlinear_cross (mfft_plan_get_info
 * "nonlinear_moments_fused_3_2" / "_none" / "_2_3"): on slab R2C plans with radix kernels on every axis the inverse x and y passes
 * and ONE z kernel per batch of x planes that ends in a reduction (csrc/nlz_moments.h NlzMoments::body) -- no real-space array exists;
 * every other plan transforms one field at a time into ONE real work array and sweeps it (mfft_ew_moments).  Powers and sums in
 * double in both precisions, no atomics: bitwise reproducible run to run on one plan and device.  A NaN or Inf bin gives NaN sums
 * and NaN / +-Inf extremes for its field.  The inputs are preserved.  Synchronises the plan's stream. */
MFFT_API int mfft_real_moments(mfft_plan_t plan, const void* a_hat, const void* b_hat, int ncomp, int dealias, const double* center,
                               double* out, int64_t* count);

/* out_host[c * (nbins + 3) + slot]: the histogram of a real device array (ncomp, n), ncomp = 1, 2, 3 or 6, in the plan's
 * precision, by the slot rule above with lo[c], hi[c].  The companion of mfft_ew_moments: one sweep, 16 bytes per lane, counts
 * in a workgroup's LDS, plain stores, one fold in fixed order into int64; no global atomics.  The plan must not be null;
 * synchronises the plan's stream. */
MFFT_API int mfft_ew_histogram(mfft_plan_t plan, const void* x, int ncomp, size_t n, int precision, const double* lo, const double* hi,
                               int nbins, int64_t* out_host);

/* Histograms of fields that exist as spectra only: for the ncomp (1 or 3) components of a_hat and, where b_hat is not NULL, of
 * b_hat -- 1, 2, 3 or 6 fields, in that order -- out[f * (nbins + 3) + slot] = the counts of x = ifftn(field f, dealias) by the
 * slot rule above with lo[f], hi[f], over THIS RANK's part of the real-space grid (as mfft_real_moments), *count = the points
 * counted (every field's slots sum to it).  The routes are those of mfft_real_moments (mfft_plan_get_info
 * "nonlinear_histogram_fused_3_2" / "_none" / "_2_3"): fused, the z kernel ends in a histogram (csrc/nlz_hist.h NlzHist::body) and no
 * real-space array exists; every other plan transforms one field at a time into ONE real work array and sweeps it
 * (mfft_ew_histogram).  Integers: bitwise reproducible run to run, and the same on every device and for every number of ranks of
 * a fused slab plan.  The inputs are preserved.  Synchronises the plan's stream. */
MFFT_API int mfft_real_histogram(mfft_plan_t plan, const void* a_hat, const void* b_hat, int ncomp, int dealias, const double* lo,
                                 const double* hi, int nbins, int64_t* out, int64_t* count);

/* out_host[c * cells + cell]: the joint histogram of the pairs (x[c, i], y[c, i]) of two real device arrays (ncomp, n) of equal
 * length, ncomp = 1 or 3, in the plan's precision, by the cell rule above; lo and hi have 2 ncomp entries, x_0.., then y_0...  The
 * companion of mfft_ew_histogram: one sweep, 16 bytes per lane of each array, counts in ONE LDS grid per workgroup, plain
 * stores, one fold in fixed order into int64; no global atomics.  The plan must not be null; synchronises the plan's stream. */
MFFT_API int mfft_ew_joint_histogram(mfft_plan_t plan, const void* x, const void* y, int ncomp, size_t n, int precision, const double* lo,
                                     const double* hi, int nba, int nbb, int64_t* out_host);

/* Joint PDFs of fields that exist as spectra only: for the ncomp (1 or 3) components of a_hat and b_hat, pair p = (a_p, b_p),
 * out[p * cells + cell] = the counts of the points (ifftn(a_p, dealias), ifftn(b_p, dealias)) by the cell rule above, over THIS
 * RANK's part of the real-space grid (as mfft_real_histogram), *count = the points counted (every pair's cells sum to it).  lo, hi:
 * 2 ncomp entries, a_0.., then b_0...  b_hat must not be NULL; a_hat == b_hat is allowed; the inputs are read only.  Routes
 * (mfft_plan_get_info "nonlinear_joint_fused_3_2" / "_none" / "_2_3"): fused, the z kernel ends in a joint histogram (csrc/nlz_joint.h
 * NlzJoint::body; the pair rides one transform, so one thread holds both values) and no real-space array exists; every other plan
 * transforms a_p and b_p into TWO real work arrays -- the least a pair can do with -- and sweeps them (mfft_ew_joint_histogram).
 * Integers: bitwise reproducible run to run, and the same for every number of ranks of a fused slab plan.  Errors
 * (MFFT_ERR_INVALID: bins outside 1 .. MFFT_JOINT_MAXBINS, hi <= lo, ranges not finite, NULL b_hat) are reported before anything
 * is enqueued and leave out and count untouched.  Synchronises the plan's stream. */
MFFT_API int mfft_real_joint_histogram(mfft_plan_t plan, const void* a_hat, const void* b_hat, int ncomp, int dealias, const double* lo,
                                       const double* hi, int nba, int nbb, int64_t* out, int64_t* count);

/* Statistics of q = sum_c weights[c] x[c, :]^2 of a real device array (ncomp, n), ncomp = 1, 2, 3 or 6, in the plan's precision,
 * by the evaluation rule above: out6 = [min, max, S1 .. S4] about `center`, counts[nbins + 3] over [lo, hi) (NULL allowed where
 * nbins == 0).  q is formed on the fly in ONE sweep, there is no q array; partials by plain stores, folds in fixed order, no global
 * atomics.  The plan must not be null; synchronises the plan's stream. */
MFFT_API int mfft_ew_quadratic(mfft_plan_t plan, const void* x, int ncomp, size_t n, int precision, const double* weights, double center,
                               double lo, double hi, int nbins, double* out6, int64_t* counts);

/* Statistics of a quadratic form of fields that exist as spectra only -- enstrophy, dissipation, energy density: for the ncomp (1 or
 * 3) components of a_hat and, where b_hat is not NULL, of b_hat -- 1, 2, 3 or 6 fields, weights[f] in that order --
 *     q(x) = sum_f weights[f] * ifftn(field f, dealias)(x)^2
 * by the evaluation rule above, over THIS RANK's part of the grid a product would be formed on (as mfft_real_moments): out6 =
 * [min, max, S1 .. S4] of q about `center`, counts[nbins + 3] by the slot rule over [lo, hi) (nbins == 0: no histogram, counts may
 * be NULL, lo and hi are ignored), *count = the points.  Routes (mfft_plan_get_info "nonlinear_quadratic_fused_3_2" / "_none" /
 * "_2_3"): fused, the z kernel accumulates q in registers across the inverse transforms of a row and ends in the reductions
 * (csrc/nlz_quad.h NlzQuad::body), no real-space array exists; every other plan transforms one field at a time into ONE real work array,
 * adds its term into ONE array of doubles and sweeps that once.  Bitwise reproducible run to run; the counts of a fused slab plan
 * are the same for every number of ranks.  MFFT_ERR_INVALID as for mfft_nlz_quad_rows, the outputs untouched on error.  The
 * inputs are preserved.  Synchronises the plan's stream. */
MFFT_API int mfft_real_quadratic(mfft_plan_t plan, const void* a_hat, const void* b_hat, int ncomp, int dealias, const double* weights,
                                 double center, double lo, double hi, int nbins, double* out6, int64_t* counts, int64_t* count);

/* out_host[(c * nsep + i) * 3 + {0, 1, 2}] = S2, S3, S4 of the increments along the rows of a real device array of ncomp x nrows
 * rows of n elements, row_pitch elements apart (>= n; component c starts c * nrows * row_pitch elements in), ncomp = 1, 2, 3 or 6,
 * in the plan's precision, by the rule above with norm = 1.  One sweep: every element is read once per separation and once for
 * itself, out of the caches where the row is short; partials by plain stores, one fold in fixed order, no atomics.  Errors as
 * mfft_nlz_incr_rows (any n >= 2 is supported).  The plan must not be null; synchronises the plan's stream. */
MFFT_API int mfft_ew_increments(mfft_plan_t plan, const void* x, int ncomp, int64_t nrows, int64_t n, int64_t row_pitch, int precision,
                                const int64_t* seps, int nsep, double* out_host);

/* Structure functions of fields that exist as spectra only: for the ncomp (1 or 3) components of a_hat and, where b_hat is not
 * NULL, of b_hat -- 1, 2, 3 or 6 fields, in that order -- out[(f * nsep + i) * 3 + {0, 1, 2}] = the sums S2, S3, S4 of the
 * increments of x = ifftn(field f, dealias) along z at the separation seps[i], by the rule above, over THIS RANK's part of the
 * real-space grid (as mfft_real_moments; z is local to a rank on slabs and pencils alike: no halo), *count = the points per field
 * (S_p / count is the structure function).  Routes (mfft_plan_get_info "nonlinear_increments_fused_3_2" / "_none" / "_2_3"):
 * fused, the z kernel keeps the real row in its exchange buffer and reads it back shifted (csrc/nlz_incr.h NlzIncr::body), no
 * real-space array exists; every other plan transforms one field at a time into ONE real work array and sweeps it
 * (mfft_ew_increments).  Bitwise reproducible run to run on one plan and device.  Errors as mfft_nlz_incr_rows with n = M,
 * reported before anything is enqueued.  The inputs are preserved.  Synchronises the plan's stream. */
MFFT_API int mfft_real_increments(mfft_plan_t plan, const void* a_hat, const void* b_hat, int ncomp, int dealias, const int64_t* seps,
                                  int nsep, double* out, int64_t* count);

/* out_host[(c * nsep + i) * (nbins + 3) + slot]: the counts of the increments along the rows of a real device array of ncomp x
 * nrows rows of n elements, row_pitch elements apart (>= n; component c starts c * nrows * row_pitch elements in), ncomp = 1, 2, 3
 * or 6, in the plan's precision, by the rule of the increment PDFs above with norm = 1; lo, hi: [(c * nsep + i)].  One sweep: a
 * workgroup takes a stripe of rows, stages each row in LDS, reads the shifted values from LDS and counts into an LDS histogram of its
 * own -- every element is read from memory once, no 64-bit division per element; partial histograms by plain stores, one fold in
 * fixed order, no global atomics.  Errors as mfft_nlz_incr_hist_rows (any n >= 2 is supported).  The plan must not be null;
 * synchronises the plan's stream. */
MFFT_API int mfft_ew_increment_histogram(mfft_plan_t plan, const void* x, int ncomp, int64_t nrows, int64_t n, int64_t row_pitch,
                                         int precision, const int64_t* seps, int nsep, const double* lo, const double* hi, int nbins,
                                         int64_t* out_host);

/* Increment PDFs of fields that exist as spectra only: for the ncomp (1 or 3) components of a_hat and, where b_hat is not NULL, of
 * b_hat -- 1, 2, 3 or 6 fields, in that order -- out[(f * nsep + i) * (nbins + 3) + slot] = the counts of the increments of x =
 * ifftn(field f, dealias) along z at the separation seps[i] in nbins equal bins of [lo[f * nsep + i], hi[f * nsep + i]), by the rule
 * above, over THIS RANK's part of the real-space grid (as mfft_real_increments: z is local to a rank, no halo), *count = the points
 * per field.  Routes (mfft_plan_get_info "nonlinear_incr_hist_fused_3_2" / "_none" / "_2_3"): fused, the z kernel keeps the real row
 * in its exchange buffer, reads it back shifted and counts into LDS (csrc/nlz_incr_hist.h NlzIncrHist::body), no real-space array exists;
 * every other plan transforms one field at a time into ONE real work array and sweeps it (mfft_ew_increment_histogram).  The fused
 * counts are the same for every number of ranks.  Errors as mfft_nlz_incr_hist_rows with n = M, reported before anything is
 * enqueued, out and count untouched.  The inputs are preserved.  Synchronises the plan's stream. */
MFFT_API int mfft_real_increment_histogram(mfft_plan_t plan, const void* a_hat, const void* b_hat, int ncomp, int dealias,
                                           const int64_t* seps, int nsep, const double* lo, const double* hi, int nbins, int64_t* out,
                                           int64_t* count);

/* out_host[(c * 5 + s) * n + m]: the five sums of the pairs (x[c, r, m], y[c, r, m]) over the nrows rows r of two real device
 * arrays (ncomp, nrows, n) of equal shape, ncomp = 1 or 3, rows contiguous, in the plan's precision, by the rule above with norm
 * = 1; center: 2 ncomp centres, x_0.., then y_0.. (NULL: zeros).  One sweep: threads run across z (coalesced loads), a workgroup
 * takes a stripe of rows, partials by plain stores, one fold in fixed order, no atomics.  MFFT_ERR_INVALID for ncomp outside
 * {1, 3}, no rows and a centre that is not finite.  The plan must not be null; synchronises the plan's stream. */
MFFT_API int mfft_ew_profiles(mfft_plan_t plan, const void* x, const void* y, int ncomp, int64_t nrows, int64_t n, int precision,
                              const double* center, double* out_host);

/* Profiles of horizontal averages of fields that exist as spectra only: for the ncomp (1 or 3) components of a_hat and b_hat, pair
 * p = (a_p, b_p), b_hat required (it may be a_hat), out[(p * 5 + s) * M + m] = sum s of (ifftn(a_p, dealias), ifftn(b_p, dealias))
 * over the (x, y) plane z = m of THIS RANK's part of the real-space grid (as mfft_real_moments; z is whole on every rank of slabs
 * and pencils alike), by the rule above about center (2 ncomp centres, a_0.., then b_0..; NULL: zeros); out holds ncomp * 5 * M
 * host doubles, *count = the points per plane on this rank (sums / count, added over the ranks, are the plane averages).  Routes
 * (mfft_plan_get_info "nonlinear_profiles_fused_3_2" / "_none" / "_2_3"): fused, a thread of the z kernel holds the same z
 * positions for every row it meets, so the plane sums are its running sums (csrc/nlz_prof.h NlzProf::body) and no real-space array
 * exists; every other plan transforms a_p and b_p into TWO real work arrays and sweeps them (mfft_ew_profiles).  Bitwise
 * reproducible run to run on one plan and device.  MFFT_ERR_INVALID for a NULL b_hat, ncomp outside {1, 3} and a centre that is not
 * finite, reported before anything is enqueued, out and count untouched.  The inputs are preserved.  Synchronises the plan's
 * stream. */
MFFT_API int mfft_real_profiles(mfft_plan_t plan, const void* a_hat, const void* b_hat, int ncomp, int dealias, const double* center,
                                double* out, int64_t* count);

/* The nonlinear term of a pseudo-spectral step as ONE operation:
 *     out_hat = fftn(ifftn(a_hat) x ifftn(b_hat))        (cross product in real space, component by component)
 * with the plan's own transforms under `dealias` -- what demo/spectral_dns_solver.py:53-71 composes from six
 * FFT.ifftn(.., dealias), numpy products and three FFT.fftn(.., dealias).  a_hat, b_hat, out_hat: (3,) + local complex
 * shape, component-major, device-resident; out_hat may be a_hat or b_hat.  On one rank with radix kernels on every axis
 * (slab R2C plans; mfft_plan_get_info "nonlinear_fused_3_2" / "_none" / "_2_3") the z stages are ONE kernel per batch of x
 * planes (csrc/fft_nlz.h): six half-spectra rows in, the cross product formed in registers, three rows out -- the nine
 * real-space work arrays of the composition (9 x 1536^3 x 8 B at 1024^3 with the 3/2-rule) never exist.  Every other plan
 * runs the composition on work arrays of its own.  Enqueued on the plan's stream like mfft_forward. */
MFFT_API int mfft_nonlinear_cross(mfft_plan_t plan, const void* a_hat, const void* b_hat, void* out_hat, int dealias);

/* The advection term of a transported scalar as ONE operation:
 *     out_hat = fftn(sum_f ifftn(a_hat[f]) * ifftn(b_hat[f]))        (dot product in real space: u . grad(theta))
 * with the plan's own transforms under `dealias` -- what a caller composes from six FFT.ifftn(.., dealias), np.sum(A * B, 0)
 * and one FFT.fftn(.., dealias).  a_hat, b_hat: (3,) + local complex shape, component-major; out_hat: the local complex
 * shape (ONE component), which may be any one component of a_hat or b_hat; the inputs are otherwise preserved.  The routes
 * are those of mfft_nonlinear_cross (mfft_plan_get_info "nonlinear_dot_fused_3_2" / "_none" / "_2_3"): on slab R2C plans with
 * radix kernels on every axis the z stages are ONE kernel (csrc/fft_nlz.h body_dot: the products are accumulated in
 * registers as the three inverse pairs finish, two rows' sums ride on one forward transform) and the seven real-space
 * arrays of the composition never exist; every other plan composes it on seven work arrays of its own. */
MFFT_API int mfft_nonlinear_dot(mfft_plan_t plan, const void* a_hat, const void* b_hat, void* out_hat, int dealias);

/* Both terms of a velocity that carries a scalar (Boussinesq, a tracer in a DNS) as ONE operation:
 *     out_hat = fftn(ifftn(a_hat) x ifftn(b_hat))                       (u x omega)
 *     s_hat   = fftn(sum_f ifftn(a_hat[f]) * ifftn(c_hat[f]))           (u . grad(theta))
 * = mfft_nonlinear_cross(a, b, out) and mfft_nonlinear_dot(a, c, s) with ifftn(a_hat) computed ONCE: nine inverse and four
 * forward transforms instead of twelve and four.  a_hat, b_hat, c_hat, out_hat: (3,) + local complex shape; s_hat: the local
 * complex shape (ONE component).  out_hat may be a_hat or b_hat, s_hat any one component of c_hat; the inputs are otherwise
 * preserved.  Dealias conventions and routes are those of the two calls (mfft_plan_get_info "nonlinear_cross_dot_fused_3_2" /
 * "_none" / "_2_3"): on slab R2C plans with radix kernels on every axis the z stages are ONE kernel (csrc/fft_nlz.h
 * body_cross_dot: 6.5 complex transforms per (x, y) row instead of 8) and no real-space array exists; every other plan
 * composes it on twelve work arrays of its own.  No statistics variant: take the maxima from mfft_nonlinear_cross_absmax. */
MFFT_API int mfft_nonlinear_cross_dot(mfft_plan_t plan, const void* a_hat, const void* b_hat, const void* c_hat, void* out_hat,
                                      void* s_hat, int dealias);

/* The OUTER product of two vector fields as ONE operation, all nine components:
 *     out_hat[3 i + j] = fftn(ifftn(a_hat[i]) * ifftn(b_hat[j])),   i, j = 0..2
 * -- the Elsasser products z+_i z-_j of incompressible MHD, a convective term in conservative form, a Reynolds or sub-grid
 * stress u_i u_j, a scalar flux: six inverse and nine forward transforms, where three mfft_nonlinear_cross calls (u x omega,
 * j x b, u x b) take eighteen and nine.  a_hat, b_hat: (3,) + local complex shape; out_hat: (9,) + local complex shape,
 * component 3 i + j.  a_hat == b_hat is allowed and gives the symmetric tensor, all nine components computed.  out_hat may NOT
 * overlap an input: MFFT_ERR_INVALID before anything is enqueued.  The inputs are preserved.  Dealias conventions are those of
 * mfft_nonlinear_cross; routes (mfft_plan_get_info "nonlinear_outer_fused_3_2" / "_none" / "_2_3"): on slab R2C plans with
 * radix kernels on every axis the z stages are ONE kernel (csrc/fft_nlz.h body_outer: 7.5 complex transforms per (x, y) row,
 * the minimum for fifteen real rows; results 0..5 in place on the six inputs of the batch, 6..8 into three more fields) and
 * no real-space array exists; every other plan -- pencils, z lengths without a kernel, MFFT_NO_NLZ=1 -- composes it on seven
 * real work arrays of its own: six inverse transforms, then per (i, j) one product (mfft_ew_mul) and one forward transform. */
MFFT_API int mfft_nonlinear_outer(mfft_plan_t plan, const void* a_hat, const void* b_hat, void* out_hat, int dealias);

/* The two operations above WITH STATISTICS: the call also records, on the device,
 *     absmax[0][f] = max |ifftn(a_hat[f], dealias)|,   absmax[1][f] = max |ifftn(b_hat[f], dealias)|,   f = 0..2
 * over this rank's part of the real-space grid on which the product is formed (the padded grid with the reference's pad scale
 * under the 3/2-rule, the masked field under the 2/3-rule) -- what FFT.ifftn(a_hat[f], u, dealias); np.abs(u).max() gives.  It
 * is the number an advective time step needs (velocity and vorticity for the cross product, velocity and grad(theta) for the
 * dot product), taken where the real values sit in registers anyway (mfft_plan_get_info "nonlinear_absmax_fused_*" /
 * "nonlinear_dot_absmax_fused_*"); plans on the composed route sweep their six real work arrays instead.  Both calls enqueue
 * and return like the plain ones and compute the same out_hat.  mfft_plan_nonlinear_absmax synchronises the plan's stream and
 * returns THIS RANK's six values of the LAST statistics call, out6 = [a0, a1, a2, b0, b1, b2] (MFFT_ERR_INVALID if none has run;
 * a call without statistics leaves them alone).  A NaN anywhere in a field gives NaN, Inf gives Inf; the values are bitwise
 * reproducible run to run.  Over several ranks reduce with a maximum that keeps NaNs (spectral.nonlinear_absmax does). */
MFFT_API int mfft_nonlinear_cross_absmax(mfft_plan_t plan, const void* a_hat, const void* b_hat, void* out_hat, int dealias);
MFFT_API int mfft_nonlinear_dot_absmax(mfft_plan_t plan, const void* a_hat, const void* b_hat, void* out_hat, int dealias);
MFFT_API int mfft_plan_nonlinear_absmax(mfft_plan_t plan, double out6[6]);

/* Direct evaluation of up to 16 DFT bins of a distributed field, for checking transforms of meshes that no host
 * transform can hold (BASELINE config 5, 2048^3): result[2b], result[2b+1] = Re, Im of
 *   sum over this rank's block u[x][y][z] * exp(-/+ 2 pi i (k0 (start0 + x) / n0 + k1 (start1 + y) / n1 + k2 (start2 + z) / n2)),
 * bins[3b .. 3b+2] = (k0, k1, k2), sign - for inverse = 0; products and sums in double precision, phase tables exact
 * (integer reduction mod n, long double).  The global bin is the sum of the ranks' results.  Synchronous.  What the
 * reference's tests do by comparing with a serial transform of the same data (tests/test_FFT.py:66-91). */
MFFT_API int mfft_ew_dft_bins(mfft_plan_t plan, const void* u, int is_complex, const int64_t shape[3], const int64_t start[3],
                              const int64_t n[3], int inverse, int nbins, const int64_t* bins_host, int precision,
                              double* result_host);

/* Shell-binned sums of device-resident spectra: the energy, transfer, enstrophy / dissipation and variance spectra of a
 * run whose fields no host copy can hold.  Over the local spectral block, for fields a, b of ncomp (1 or 3) components,
 * component-major and shape[0] * shape[1] * shape[2] elements apart (b may be a: it is then read once),
 *   result[s] = sum over the modes k with shell(k) = s of  h(k) w(k) sum_c Re(conj(a_c[k]) b_c[k]),   0 <= s < nshell.
 * shell(k) is the integer nearest to |k| of the INTEGER wave numbers ikx[x], iky[y], ikz[z], decided in integer
 * arithmetic: 0 for m = kx^2 + ky^2 + kz^2 = 0, else the s >= 1 with (2s-1)^2 <= 4m < (2s+1)^2.  h = hz[z]: the Hermitian
 * weight of a real transform's half axis (1 for kz = 0 and the Nyquist mode of an even axis, 2 otherwise; 1 everywhere on
 * complex plans); elements with hz = 0 (between the rows of a pitched spectrum: shape[2] is the row length as it lies in
 * memory and the four z vectors have that length) are skipped, whatever they hold.  w = 1 for k2 == 0 (kx, ky, kz may
 * then be null), else kx^2 + ky^2 + kz^2 of the scaled wave numbers (the vectors of mfft_ew_curl_hat), squared in double.
 * Products and sums are in double whatever `precision`.  result_host receives THIS RANK's nshell partial sums (the caller
 * adds the ranks'); the call synchronises the plan's stream.  One streaming sweep with a per-workgroup histogram in LDS
 * (csrc/shells.hip); the workgroups' histograms live in a buffer of the plan and are summed in fixed order.  Every lane
 * loads 16 bytes; in single precision that needs a and b 16-byte aligned and, for ncomp = 3, an even number of elements
 * per component -- otherwise the call is as correct and loads 8 bytes per lane.
 * MFFT_ERR_INVALID: null arguments (the plan included), ncomp not 1 or 3, nshell < 1, or a mode of the block in a shell
 * >= nshell (found on the device, nothing is written out of range); MFFT_ERR_UNSUPPORTED: nshell * 8 bytes > 64 KiB. */
MFFT_API int mfft_ew_shell_sums(mfft_plan_t plan, const void* a, const void* b, int ncomp, const int32_t* ikx,
                                const int32_t* iky, const int32_t* ikz, const uint8_t* hz, const void* kx, const void* ky,
                                const void* kz, int k2, const int64_t shape[3], int nshell, int precision,
                                double* result_host);

/* (k_perp, k_z) sums of device-resident spectra: cylindrical bins, for flows with one special direction (z: gravity, a mean
 * field).  THE RULE, which the kernel, the Python layer and the tests quote: for a local spectral block of shape (s0, s1, s2),
 * z contiguous and s2 the row length as it lies in memory (the pitch, where the spectrum is pitched),
 *   R[p, q] = sum over the local modes k with  shell(kx^2 + ky^2) = p  and  |kz| = q
 *             of  h(k) w(k) sum_c Re(conj(a_c[k]) b_c[k]),      0 <= p < nperp, 0 <= q < npar.
 * shell is the integer rule of mfft_ew_shell_sums applied to m = kx^2 + ky^2 of the INTEGER wave numbers; |kz| is taken from
 * ikz[z], which covers the half axis of the real transforms and the full axis of the complex slab plan, where kz and -kz share
 * a bin; h = hz[z] is the Hermitian weight along z, and its 0 between pitched rows means "skip, whatever lies there";
 * w = kx^2 + ky^2 + kz^2 of the scaled wave numbers, squared in double, with k2, else 1 (kx, ky, kz may then be null); ncomp is
 * 1 or 3, components shape[0] * shape[1] * shape[2] elements apart; b may be a, which is then read once.  Products and sums are
 * in double whatever `precision`.  For the global mesh nperp = shell((N0/2)^2 + (N1/2)^2) + 1 and npar = N2/2 + 1 (integer
 * halves); the result is nperp x npar doubles, row-major; its sum is the Parseval sum, that of mfft_ew_shell_sums' result; its
 * row sums are the k_perp spectrum and its column sums the k_z spectrum.
 *
 * The perp bin is constant along a memory row and the z bin is the position in the row, so R is a sum of rows grouped by a
 * key the host knows (csrc/cylspec.hip): `rows` holds the local rows l * s1 + j sorted by (perp shell, l, j) and
 * row_start[p] .. row_start[p + 1] are shell p's entries (nperp + 1 offsets; a shell without local rows is empty and its bins
 * come back as 0.0).  Every list is cut into segments of at most seg_rows rows (0: MFFT_CYL_SEG_ROWS); a wave sums one
 * (segment, run of z positions) in registers and stores it once; a second kernel adds the partial rows in fixed order.  No
 * atomics on global memory; bitwise reproducible run to run for a given seg_rows.  Every lane loads 16 bytes; in single
 * precision that needs every row to start at a multiple of 16 bytes (a, b 16-byte aligned and s2 even) -- otherwise, as for
 * the compact rows of N2/2 + 1 elements with N2/2 even, the call is as correct and loads 8 bytes per lane.  The partial rows
 * live in a buffer of the plan: segments * s2 + nperp * npar doubles. */
#define MFFT_CYL_SEG_ROWS 256

/* Host only, no device call: the lists of mfft_ew_cyl_sums for a block whose integer wave numbers along x and y are
 * ikx_host[s0], iky_host[s1].  rows_out: s0 * s1 entries; row_start_out: nperp + 1.  MFFT_ERR_INVALID for null arguments, an
 * empty block and a row whose shell is >= nperp. */
MFFT_API int mfft_cyl_row_lists(const int32_t* ikx_host, const int32_t* iky_host, int64_t s0, int64_t s1, int nperp,
                                int32_t* rows_out, int32_t* row_start_out);

/* result_host receives THIS RANK's nperp * npar partial sums (the caller adds the ranks'); the call synchronises the plan's
 * stream.  rows_dev is on the device, row_start_host on the host; ikz, hz, kx, ky, kz, shape as for mfft_ew_shell_sums.
 * Reported before anything is enqueued, result_host untouched: MFFT_ERR_INVALID for null arguments (the plan included), ncomp
 * not 1 or 3, an unknown precision, nperp or npar < 1, seg_rows < 0, an empty block, k2 without the scaled vectors, and a
 * row_start that does not begin at 0, is not monotone or does not end at shape[0] * shape[1].  A mode with weight whose |kz| is
 * >= npar, and an entry of rows_dev that is no row of the block, are found on the device (nothing is loaded or stored out of
 * range) and reported as MFFT_ERR_INVALID, result_host untouched. */
MFFT_API int mfft_ew_cyl_sums(mfft_plan_t plan, const void* a, const void* b, int ncomp, const int32_t* rows_dev,
                              const int32_t* row_start_host, int nperp, const int32_t* ikz, const uint8_t* hz, const void* kx,
                              const void* ky, const void* kz, int k2, const int64_t shape[3], int npar, int seg_rows,
                              int precision, double* result_host);

/* ---- HIP-event timers on the default stream (bench.py) ------------------ */
typedef struct mfft_timer_s* mfft_timer_t;
MFFT_API int mfft_timer_create(mfft_timer_t* t);
MFFT_API int mfft_timer_start(mfft_timer_t t);
MFFT_API int mfft_timer_stop(mfft_timer_t t, float* elapsed_ms);   /* synchronises on the stop event */
MFFT_API int mfft_timer_destroy(mfft_timer_t t);

#ifdef __cplusplus
}
#endif
#endif /* MPIFFT4PY_AMD_H */
