"""Guard bands and poison for the GPU tests (an ordinary module, like gpu_util.py).

`guarded(shape, dtype, pitch, fill)` returns a non-owning DeviceArray in the middle of ONE owning allocation laid out as
guard | payload | guard.  The guards hold a fixed pseudo-random byte pattern (never zeros: a stray zero store must show); the
payload of an OUTPUT is poisoned with 0xFF bytes -- a NaN in both precisions, real and imaginary part --, the payload of an INPUT
is the test data (the elements between the rows of a pitched input are poisoned).  `check(view, what)` copies both guards back
and compares them byte for byte; for an output it also asserts that no logical element is still NaN, for an input that
get().tobytes() is what was uploaded.

The comparisons (`guard_report`, `poison_report`) are pure numpy functions, tested without a device (tests/test_guard_util.py).
The guard is the larger of 64 KiB and twice the array's leading-axis plane, rounded up to 256 B, so the payload keeps the
256-byte alignment an allocation of its own has; a store one tile too wide or one row too many lands inside it."""
import numpy as np

GUARD_MIN = 64 << 10
ALIGN = 256
SEED = 0x67756172
POISON = 0xFF

_PATTERN = {}


class GuardError(AssertionError):
    pass


def guard_size(shape, dtype, pitch=None):
    """Bytes of one guard: max(64 KiB, 2 x the largest leading-axis plane) rounded up to 256 B."""
    nbytes = payload_bytes(shape, dtype, pitch)
    plane = nbytes // max(int(shape[0]), 1) if len(shape) else nbytes
    g = max(GUARD_MIN, 2 * plane)
    return (g + ALIGN - 1) // ALIGN * ALIGN


def payload_bytes(shape, dtype, pitch=None):
    """What a DeviceArray of this shape and pitch occupies (device.py): the whole pitched extent."""
    shape = tuple(int(s) for s in shape)
    size = int(np.prod(shape)) if shape else 1
    if pitch is not None and shape and int(pitch) != shape[-1]:
        size = size // shape[-1] * int(pitch)
    return size * np.dtype(dtype).itemsize


def pattern(nbytes, seed=SEED):
    """The guard fill: `nbytes` pseudo-random bytes, the same for a given size and seed (cached, read-only)."""
    key = (int(nbytes), seed)
    if key not in _PATTERN:
        p = np.random.default_rng(seed).integers(0, 256, int(nbytes), dtype=np.uint8)
        p.setflags(write=False)
        _PATTERN[key] = p
    return _PATTERN[key]


# ---- the comparisons: pure numpy, no device -------------------------------------------------------------------------------
def guard_report(guard_before, guard_after, expected_pattern):
    """Compare the two guards, as copied back, with the pattern both were filled with.  Returns a list of findings, one per
    violated side: dict(side, first, last, count) with byte offsets RELATIVE TO THE PAYLOAD EDGE -- before: -1 is the byte just
    below the payload's first byte, -G the far end; after: 0 is the first byte past the payload's last."""
    exp = np.asarray(expected_pattern, dtype=np.uint8).reshape(-1)
    out = []
    for side, got in (("before", guard_before), ("after", guard_after)):
        got = np.asarray(got, dtype=np.uint8).reshape(-1)
        if got.size != exp.size:
            raise ValueError("guard of %d bytes against a pattern of %d" % (got.size, exp.size))
        bad = np.flatnonzero(got != exp)
        if bad.size:
            shift = exp.size if side == "before" else 0
            out.append(dict(side=side, first=int(bad[0]) - shift, last=int(bad[-1]) - shift, count=int(bad.size)))
    return out


def format_guard_report(findings):
    return "; ".join("guard %s the payload overwritten: %d bytes, offsets %d .. %d from the payload's edge"
                     % (f["side"], f["count"], f["first"], f["last"]) for f in findings)


def poison_report(logical):
    """An output's logical elements, as get() returns them: None if none is NaN, else dict(count, first, last) with flat C-order
    element indices (a complex element counts when either part is NaN)."""
    bad = np.flatnonzero(np.isnan(np.asarray(logical)).reshape(-1))
    if not bad.size:
        return None
    return dict(count=int(bad.size), first=int(bad[0]), last=int(bad[-1]))


# ---- the device side ------------------------------------------------------------------------------------------------------
def guarded(shape, dtype, pitch=None, fill=None):
    """A DeviceArray view (ptr=, owner=False) of `shape` / `dtype` / `pitch` between two guards.  fill=None: an output, payload
    poisoned; fill=array: an input holding that data (converted to `dtype`)."""
    from mpifft4py_amd import DeviceArray, _lib
    shape = tuple(int(s) for s in shape)
    dtype = np.dtype(dtype)
    if pitch is not None and (not shape or int(pitch) == shape[-1]):
        pitch = None
    G = guard_size(shape, dtype, pitch)
    nbytes = payload_bytes(shape, dtype, pitch)
    host = np.empty(2 * G + nbytes, dtype=np.uint8)
    host[:G] = pattern(G)
    host[G + nbytes:] = pattern(G)
    pay = host[G:G + nbytes]
    pay[:] = POISON
    uploaded = None
    if fill is not None:
        data = np.ascontiguousarray(fill, dtype=dtype)
        if data.shape != shape:
            raise ValueError("fill of shape %s for an array of shape %s" % (data.shape, shape))
        uploaded = data.tobytes()
        if pitch is None:
            pay[:] = np.frombuffer(uploaded, dtype=np.uint8)
        else:
            w = shape[-1] * dtype.itemsize
            pay.reshape(-1, int(pitch) * dtype.itemsize)[:, :w] = np.frombuffer(uploaded, dtype=np.uint8).reshape(-1, w)
    base = DeviceArray((host.size,), np.uint8)
    assert base.ptr % ALIGN == 0, "allocation not %d-byte aligned: 0x%x" % (ALIGN, base.ptr)
    _lib.call("mfft_memcpy_h2d", base.ptr, host.ctypes.data, host.size)
    view = DeviceArray(shape, dtype, ptr=base.ptr + G, owner=False, pitch=pitch)
    assert view.nbytes == nbytes
    view._base = base
    view._guard = dict(G=G, uploaded=uploaded, kind="output" if fill is None else "input")
    return view


def read_guards(view):
    """(guard_before, guard_after) of a guarded view, copied to the host."""
    from mpifft4py_amd import _lib
    G = view._guard["G"]
    before, after = np.empty(G, dtype=np.uint8), np.empty(G, dtype=np.uint8)
    _lib.call("mfft_memcpy_d2h", before.ctypes.data, view._base.ptr, G)
    _lib.call("mfft_memcpy_d2h", after.ctypes.data, view._base.ptr + G + view.nbytes, G)
    return before, after


def check(view, what, expect=None):
    """Raise GuardError unless both guards of `view` are intact and, by `expect`,
      "output" (default for fill=None):  no logical element is NaN (the elements between the rows of a pitched array are not looked at);
      "input"  (default for fill=data):  get().tobytes() equals the uploaded bytes;
      "guards": nothing more (arrays an operation updates in place)."""
    g = view._guard
    expect = expect or g["kind"]
    assert expect in ("output", "input", "guards"), expect
    problems = []
    findings = guard_report(*read_guards(view), pattern(g["G"]))
    if findings:
        problems.append(format_guard_report(findings))
    if expect == "output":
        left = poison_report(view.get())
        if left:
            problems.append("poisoned element left: %d of %d elements never written, flat indices %d .. %d of shape %s"
                            % (left["count"], view.size, left["first"], left["last"], view.shape))
    elif expect == "input":
        got = view.get().tobytes()
        if got != g["uploaded"]:
            a, b = np.frombuffer(got, dtype=np.uint8), np.frombuffer(g["uploaded"], dtype=np.uint8)
            bad = np.flatnonzero(a != b)
            problems.append("input modified: %d bytes differ, byte offsets %d .. %d of %d" % (bad.size, bad[0], bad[-1], a.size))
    if problems:
        raise GuardError("%s (%s, shape %s, pitch %s): %s" % (what, view.dtype, view.shape, view.pitch, "; ".join(problems)))


def collect(problems, view, what, expect=None):
    """check() that appends the message to `problems` instead of raising (rank bodies: every rank finishes its checks)."""
    try:
        check(view, what, expect)
    except GuardError as e:
        problems.append(str(e))
