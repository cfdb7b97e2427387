"""GPU: the memory no other test looks at.  Every case puts its inputs into guarded arrays and its outputs into guarded, poisoned
arrays (tests/guard_util.py: guard | payload | guard in one allocation, the guards a pseudo-random byte pattern, an output's payload
0xFF bytes = NaN), runs one operation, synchronises and then asserts
  (a) both guards of every output are intact and no logical element of it is still NaN -- no stray write, nothing left unwritten;
  (b) both guards of every input are intact and the input comes back bit for bit where the header (include/mpifft4py_amd.h) or the
      docstring promises that it is preserved;
  (c) the result against the oracle / numpy composition and the bound the existing test of that operation uses (no new tolerance).
The meshes are the suite's smallest that still run edge tiles and partial workgroups: [8, 16, 32] (radix, Nf = 17), [20, 12, 44] and
[24, 40, 20] (non-power-of-two radix lengths), [7, 9, 22] (chirp-z on every axis, odd row counts), [36, 60, 100] (several ranks),
[8, 4, 8194] and [4100, 8, 6] (one axis through the scratch-buffer route), [1, 8, 8] and [8, 1, 8] (unit axes).  Every case prints
the route it ran (plan_info keys, mfft_length_route per axis).  Several ranks run through run_ranks; each rank guards its own
arrays, finishes its operations, and only then checks (the findings come back to the test, which asserts)."""
import ctypes

import numpy as np
import pytest

import nonlinear_util as nl
from gpu_util import L, TOL, cdtype, have_gpu, orc, rdtype, run_ranks
from guard_util import GuardError, check, collect, guarded, pattern

pytestmark = pytest.mark.gpu

L3 = np.array([2 * np.pi, 4 * np.pi, 2 * np.pi])        # the box of the element-wise tests (tests/test_gpu_demo.py)
L2 = np.array([2 * np.pi, 4 * np.pi])                    # ... and of the 2-D class (tests/test_gpu_line.py)
DEALIAS = [None, "2/3-rule", "3/2-rule"]


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not have_gpu():
        pytest.fail("no GPU visible")


def _id(v):
    if isinstance(v, (list, tuple)):
        return "x".join(str(x) for x in v)
    return str(v)


# ---- the harness on the device --------------------------------------------------------------------------------------------
def test_harness_reports_on_the_device():
    """One guard byte on each side overwritten through mfft_memcpy_h2d (memory this test owns): check reports both with side and
    offset; one payload element left poisoned is reported; a changed input byte is reported; everything restored passes."""
    from mpifft4py_amd import _lib
    v = guarded((5, 7), np.complex128)
    G, base = v._guard["G"], v._base.ptr
    assert G == 64 << 10 and v.ptr == base + G and v.ptr % 256 == 0
    p = pattern(G)

    def poke(addr, byte):
        b = np.array([byte], dtype=np.uint8)
        _lib.call("mfft_memcpy_h2d", addr, b.ctypes.data, 1)

    ones = np.ones((5, 7), dtype=np.complex128)
    _lib.call("mfft_memcpy_h2d", v.ptr, ones.ctypes.data, v.nbytes)
    check(v, "untouched")
    poke(base + G - 3, int(p[G - 3]) ^ 0x01)                             # 3 bytes below the payload
    poke(base + G + v.nbytes + 5, 0 if p[5] else 1)                      # a stray (zero) store 5 bytes past its end
    with pytest.raises(GuardError) as e:
        check(v, "selftest")
    msg = str(e.value)
    assert "guard before the payload overwritten: 1 bytes, offsets -3 .. -3" in msg, msg
    assert "guard after the payload overwritten: 1 bytes, offsets 5 .. 5" in msg, msg
    poke(base + G - 3, int(p[G - 3]))
    with pytest.raises(GuardError) as e:
        check(v, "selftest")
    assert "guard before" not in str(e.value) and "guard after" in str(e.value)
    poke(base + G + v.nbytes + 5, int(p[5]))
    check(v, "restored")
    # an output of which the last element was never written
    w = guarded((5, 7), np.complex128)
    _lib.call("mfft_memcpy_h2d", w.ptr, ones.ctypes.data, w.nbytes - 16)
    with pytest.raises(GuardError) as e:
        check(w, "selftest")
    assert "poisoned element left: 1 of 35 elements never written, flat indices 34 .. 34" in str(e.value), str(e.value)
    check(w, "guards only", expect="guards")
    _lib.call("mfft_memcpy_h2d", w.ptr, ones.ctypes.data, w.nbytes)
    check(w, "written")
    # a pitched output: the elements between the rows stay poisoned and are not looked at
    q = guarded((5, 7), np.complex64, pitch=10)
    assert q.nbytes == 5 * 10 * 8
    q.set(np.ones((5, 7), dtype=np.complex64))
    check(q, "pitched")
    whole = np.empty((5, 10), dtype=np.complex64)
    _lib.call("mfft_memcpy_d2h", whole.ctypes.data, q.ptr, q.nbytes)
    assert np.all(np.isnan(whole[:, 7:])) and np.all(whole[:, :7] == 1)
    # an input
    data = np.random.default_rng(1).random((3, 4, 5))
    x = guarded(data.shape, data.dtype, fill=data)
    check(x, "input")
    assert np.array_equal(x.get(), data)
    poke(x.ptr + 17, data.view(np.uint8).reshape(-1)[17] ^ 0x80)
    with pytest.raises(GuardError) as e:
        check(x, "selftest")
    assert "input modified: 1 bytes differ, byte offsets 17 .. 17" in str(e.value), str(e.value)
    check(x, "in place", expect="guards")


# ---- routes ---------------------------------------------------------------------------------------------------------------
def _route(F, N, real=True):
    """What ran: mfft_length_route per axis (1 radix, 2 chirp-z, 3 scratch buffer) and what the plan decided."""
    from mpifft4py_amd import _lib
    lib = _lib.load()
    pc = _lib.precision_code(F.precision)
    axes = [int(lib.mfft_length_route_precision(int(n), 1 if (real and i == len(N) - 1) else 0, pc)) for i, n in enumerate(N)]
    info = {}
    for key in ("complex_pitch", "complex_pitch_native", "pruned_route", "split_last", "plane_pad", "local_band"):
        try:
            info[key] = F.plan_info(key)
        except Exception:      # noqa: BLE001 - a key this kind of plan does not have
            pass
    return "length routes %s, plan %s" % (axes, info)


# ---- references: computed once per case on the host, shared, never written again -------------------------------------------
_REF = {}


def _cached(key, make):
    if key not in _REF:
        ref = make()
        for v in ref.values():
            for x in (v if isinstance(v, list) else [v]):
                if isinstance(x, np.ndarray):
                    x.setflags(write=False)
        _REF[key] = ref
    return _REF[key]


def _host_class(decomp, N, P, r, prec):
    """The class on a LayoutComm (no device): shapes, slices and the dealias filter of rank r."""
    from mpifft4py_amd import LayoutComm, Pencil_R2C, Slab_R2C
    if decomp == "slab":
        return Slab_R2C(np.array(N), L, LayoutComm(P, r), prec)
    return Pencil_R2C(np.array(N), L, LayoutComm(P, r), prec, communication="Alltoallw", alignment=decomp[-1])


def _r2c_reference(decomp, N, P, prec, dealias):
    """Inputs and expected results of fftn and ifftn per rank, as the existing parity tests form them (tests/test_gpu_parity.py):
      None      test_slab_r2c / test_pencil_r2c: a random real field against the oracle within TOL; the oracle's spectrum back to the
                field within 4 TOL;
      2/3-rule  test_two_thirds_rule: forward is the regular transform; the spectrum of a real field back, against
                numpy.fft.irfftn(C * mask) with the classes' own filter, within 4 TOL;
      3/2-rule  test_padded_generic_data: a random padded real field forward, a random spectrum backward, against the oracle within
                4 TOL."""
    N = [int(n) for n in N]

    def make():
        rt, ct = rdtype(prec), cdtype(prec)
        rng = np.random.default_rng(sum(N) + 7 * P)
        align = decomp[-1]
        lay = orc.SlabLayout(N, P) if decomp == "slab" else orc.PencilLayout(N, P, None, align)
        if decomp == "slab":
            fwd = lambda us: orc.slab_r2c_forward(us, N, prec)
            fwd_p = lambda us: orc.slab_r2c_forward_padded(us, N, prec)
            bwd_p = lambda fus: orc.slab_r2c_backward_padded(fus, N, prec)
        else:
            fwd = lambda us: orc.pencil_r2c_forward(us, N, None, align, prec)
            fwd_p = lambda us: orc.pencil_r2c_forward_padded(us, N, None, align, prec)
            bwd_p = lambda fus: orc.pencil_r2c_backward_padded(fus, N, None, align, prec)
        if dealias == "3/2-rule":
            Ap = rng.random([int(1.5 * n) for n in N]).astype(rt)
            nf = N[2] // 2 + 1
            Cr = (rng.random((N[0], N[1], nf)) - 0.5 + 1j * (rng.random((N[0], N[1], nf)) - 0.5)).astype(ct)
            fwd_in, bwd_in = orc.scatter_real(Ap, lay, 1.5), orc.scatter_complex(Cr, lay)
            return dict(fwd_in=fwd_in, fwd_want=fwd_p(fwd_in), fwd_tol=4 * TOL[prec],
                        bwd_in=bwd_in, bwd_want=bwd_p(bwd_in), bwd_tol=4 * TOL[prec])
        A = rng.random(N).astype(rt)
        fwd_in = orc.scatter_real(A, lay)
        want = fwd(fwd_in)
        if dealias is None:
            return dict(fwd_in=fwd_in, fwd_want=want, fwd_tol=TOL[prec], bwd_in=want, bwd_want=fwd_in, bwd_tol=4 * TOL[prec])
        C = np.fft.rfftn(A.astype(np.float64)).astype(ct)
        M = np.zeros(C.shape, dtype=np.uint8)
        for r in range(P):
            H = _host_class(decomp, N, P, r, prec)
            M[lay.complex_local_slice(r)] = np.broadcast_to(H.get_dealias_filter(), H.complex_shape())
        assert 0 < int(M.sum()) < M.size
        back = np.fft.irfftn(C.astype(np.complex128) * M, s=N, axes=(0, 1, 2))
        return dict(fwd_in=fwd_in, fwd_want=want, fwd_tol=TOL[prec], bwd_in=orc.scatter_complex(C, lay),
                    bwd_want=[np.ascontiguousarray(back[lay.real_local_slice(r)]).astype(rt) for r in range(P)], bwd_tol=4 * TOL[prec])
    return _cached(("r2c", decomp, tuple(N), P, prec, dealias), make)


def _transform_case(P, make, ref, dealias, N, fwd="fftn", bwd="ifftn", expect=None, real=True):
    """fftn and ifftn of one object per rank, both between guards; `expect(F)`: route assertions."""
    def body(comm):
        F = make(comm)
        r = comm.Get_rank()
        pitch = getattr(F, "complex_pitch", None)
        u = guarded(ref["fwd_in"][r].shape, ref["fwd_in"][r].dtype, fill=ref["fwd_in"][r])
        fu = guarded(ref["fwd_want"][r].shape, F.complex, pitch=pitch)
        c = guarded(ref["bwd_in"][r].shape, F.complex, pitch=pitch, fill=ref["bwd_in"][r])
        out = guarded(ref["bwd_want"][r].shape, ref["bwd_want"][r].dtype)
        assert getattr(F, fwd)(u, fu, dealias) is fu
        getattr(F, bwd)(c, out, dealias)
        F.sync()
        problems = []
        collect(problems, fu, "rank %d %s output" % (r, fwd))
        collect(problems, u, "rank %d %s input" % (r, fwd))
        collect(problems, out, "rank %d %s output" % (r, bwd))
        collect(problems, c, "rank %d %s input" % (r, bwd))
        if expect is not None:
            expect(F)
        return problems, orc.rel_l2(fu.get(), ref["fwd_want"][r]), orc.rel_l2(out.get(), ref["bwd_want"][r]), _route(F, N, real)
    res = run_ranks(P, body)
    print("route:", res[0][3])
    problems = [p for r in res for p in r[0]]
    assert not problems, "\n".join(problems)
    for r, (_, e1, e2, _) in enumerate(res):
        print("rank %d: %s rel-L2 %.3e (bound %.1e), %s rel-L2 %.3e (bound %.1e)" % (r, fwd, e1, ref["fwd_tol"], bwd, e2, ref["bwd_tol"]))
        assert e1 < ref["fwd_tol"] and e2 < ref["bwd_tol"], (r, e1, e2)


# ---- Slab_R2C ---------------------------------------------------------------------------------------------------------------
# mesh -> (rank counts, dealias modes, precisions); the arbitrary-length and unit-axis meshes keep what the existing tests of those
# meshes run (test_slab_r2c_arbitrary_lengths, test_meshes_with_an_axis_beyond_the_radix_plans with its rank counts,
# test_meshes_with_unit_axes)
SLAB_MESHES = [([8, 16, 32], (1, 2, 4), DEALIAS, ("double", "single")),
               ([20, 12, 44], (1, 2, 4), DEALIAS, ("double", "single")),
               ([24, 40, 20], (1, 2, 4), DEALIAS, ("double", "single")),
               ([36, 60, 100], (1, 2, 4), DEALIAS, ("double", "single")),
               ([7, 9, 22], (1,), [None, "2/3-rule"], ("double", "single")),
               ([8, 4, 8194], (2,), [None, "2/3-rule"], ("double",)),
               ([4100, 8, 6], (1,), [None, "2/3-rule"], ("double",)),
               ([1, 8, 8], (1,), [None], ("double", "single")),
               ([8, 1, 8], (1,), [None], ("double", "single"))]


def _slab_cases():
    """Every mesh with its rank counts, modes and precisions (the whole file takes well under a minute: nothing is thinned)."""
    out = []
    for N, ranks, modes, precs in SLAB_MESHES:
        for P in ranks:
            for prec in precs:
                for dealias in modes:
                    if dealias == "3/2-rule" and (N[0] // P) % 2:
                        continue                         # 1.5 x an odd number of local x planes: the reference has no such layout
                    out.append(pytest.param(N, P, prec, dealias, id="%s-P%d-%s-%s" % (_id(N), P, prec, dealias)))
    return out


@pytest.mark.parametrize("N,P,prec,dealias", _slab_cases())
def test_slab_r2c_compact(N, P, prec, dealias):
    from mpifft4py_amd import Slab_R2C
    ref = _r2c_reference("slab", N, P, prec, dealias)
    _transform_case(P, lambda comm: Slab_R2C(np.array(N), L, comm, prec), ref, dealias, N)


def _pitched_cases():
    """(the odd mesh keeps the modes of SLAB_MESHES: the existing tests run no 3/2-rule on it)"""
    return [pytest.param(N, pitch, prec, dealias, id="%s-%s-%s-%s" % (_id(N), pitch, prec, dealias))
            for N, _, modes, precs in SLAB_MESHES if N in ([8, 16, 32], [20, 12, 44], [36, 60, 100], [7, 9, 22])
            for pitch in ("auto", "plus3") for prec in precs for dealias in modes]


@pytest.mark.parametrize("N,pitch,prec,dealias", _pitched_cases())
def test_slab_r2c_pitched_one_rank(N, pitch, prec, dealias):
    """complex_pitch="auto" (rows a whole number of cache lines apart) and Nf + 3: the spectrum's payload is the whole pitched
    extent, the elements between the rows stay out of the NaN check."""
    from mpifft4py_amd import Slab_R2C
    nf = N[2] // 2 + 1
    ref = _r2c_reference("slab", N, 1, prec, dealias)

    def expect(F):
        line = 128 // np.dtype(F.complex).itemsize
        assert F.complex_pitch == ((nf + line - 1) // line * line if pitch == "auto" else nf + 3)
        assert F.plan_info("complex_pitch") == F.complex_pitch
    _transform_case(1, lambda comm: Slab_R2C(np.array(N), L, comm, prec, complex_pitch="auto" if pitch == "auto" else nf + 3),
                    ref, dealias, N, expect=expect)


@pytest.mark.parametrize("prune", [True, False], ids=["pruned", "MFFT_NO_PRUNE"])
@pytest.mark.parametrize("N,P,prec", [([8, 16, 32], 2, "double"), ([8, 16, 32], 4, "double"), ([8, 16, 32], 2, "single"),
                                      ([8, 16, 32], 4, "single"), ([36, 60, 100], 2, "double"), ([36, 60, 100], 4, "double"),
                                      ([20, 12, 44], 4, "double")], ids=_id)
def test_slab_r2c_two_thirds_rule_over_ranks(N, P, prec, prune, monkeypatch):
    """The 2/3-rule over 2 and 4 ranks with the default separable mask: the pruned route (the x pass writes the kept kz bins only,
    a smaller exchange) and, with MFFT_NO_PRUNE=1 (read at every call, as test_two_thirds_rule_pruned sets it), the masked-load route."""
    from mpifft4py_amd import Slab_R2C
    if prune:
        monkeypatch.delenv("MFFT_NO_PRUNE", raising=False)
    else:
        monkeypatch.setenv("MFFT_NO_PRUNE", "1")
    ref = _r2c_reference("slab", N, P, prec, "2/3-rule")

    def expect(F):
        route = F.plan_info("pruned_route")
        if prune and N == [8, 16, 32]:
            assert route > 0, route                      # radix kernels exist: the pruned route must engage
    _transform_case(P, lambda comm: Slab_R2C(np.array(N), L, comm, prec), ref, "2/3-rule", N, expect=expect)


@pytest.mark.parametrize("N,switch", [([8, 16, 32], "0"), ([8, 16, 32], None), ([20, 12, 44], "0"), ([20, 12, 44], None),
                                      ([16, 32, 64], "1")], ids=_id)
def test_slab_r2c_split_last_switch(N, switch, monkeypatch):
    """One rank: MFFT_SPLIT_LAST=0 and the default (both the regular route on these meshes), and -- on a mesh of
    tests/test_gpu_split_last.py -- the route that splits real / complex at the spectrum end, forced on."""
    from mpifft4py_amd import Slab_R2C
    if switch is None:
        monkeypatch.delenv("MFFT_SPLIT_LAST", raising=False)
    else:
        monkeypatch.setenv("MFFT_SPLIT_LAST", switch)
    ref = _r2c_reference("slab", N, 1, "double", None)

    def expect(F):
        assert F.plan_info("split_last") == (1 if switch == "1" else 0)
    _transform_case(1, lambda comm: Slab_R2C(np.array(N), L, comm, "double"), ref, None, N, expect=expect)


# ---- Pencil_R2C -------------------------------------------------------------------------------------------------------------
def _pencil_cases():
    out = []
    for N in ([8, 16, 32], [20, 12, 44], [36, 60, 100]):
        for align in ("X", "Y"):
            for prec, dealias in (("double", None), ("single", None), ("double", "3/2-rule"), ("single", "3/2-rule"), ("double", "2/3-rule"),
                                  ("single", "2/3-rule")):
                out.append(pytest.param(N, align, prec, dealias, id="%s-%s-%s-%s" % (_id(N), align, prec, dealias)))
    return out


@pytest.mark.parametrize("N,align,prec,dealias", _pencil_cases())
def test_pencil_r2c(N, align, prec, dealias):
    from mpifft4py_amd import Pencil_R2C
    ref = _r2c_reference("pencil" + align, N, 4, prec, dealias)
    _transform_case(4, lambda comm: Pencil_R2C(np.array(N), L, comm, prec, communication="Alltoallw", alignment=align), ref, dealias, N)


# ---- Slab_C2C, Line_R2C -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", ["double", "single"])
@pytest.mark.parametrize("N,P", [([8, 16, 32], 1), ([8, 16, 32], 2), ([20, 12, 44], 1), ([20, 12, 44], 2), ([7, 9, 22], 1)], ids=_id)
def test_slab_c2c(N, P, prec):
    """As test_slab_c2c of the parity suite: against the oracle (numpy.fft.fftn) within TOL, back to the field within 4 TOL."""
    from mpifft4py_amd import Slab_C2C

    def make():
        rng = np.random.default_rng(300 + sum(N) + P)
        A = (rng.random(N) + 1j * rng.random(N)).astype(cdtype(prec))
        lay = orc.SlabLayout(N, P, kind="C2C")
        fwd_in = orc.scatter_real(A, lay)
        want = orc.slab_c2c_forward(fwd_in, N, prec)
        B2 = np.fft.fftn(A.astype(np.complex128))
        for r in range(P):
            assert orc.rel_l2(want[r], B2[lay.complex_local_slice(r)]) < TOL[prec]
        return dict(fwd_in=fwd_in, fwd_want=want, fwd_tol=TOL[prec], bwd_in=want, bwd_want=fwd_in, bwd_tol=4 * TOL[prec])
    ref = _cached(("c2c", tuple(N), P, prec), make)
    _transform_case(P, lambda comm: Slab_C2C(np.array(N), L, comm, prec), ref, None, N, real=False)


@pytest.mark.parametrize("dealias", DEALIAS, ids=_id)
@pytest.mark.parametrize("prec", ["double", "single"])
@pytest.mark.parametrize("P", [1, 2])
def test_line_r2c(P, prec, dealias):
    """The 2-D class on the mesh of tests/test_gpu_line.py, with that file's references: test_line_r2c (plain) and
    test_line_r2c_dealiased (random spectra backward, a random padded field forward; 4 TOL)."""
    from mpifft4py_amd import Line_R2C
    N = [32, 64]

    def make():
        rt, ct = rdtype(prec), cdtype(prec)
        lay = orc.LineLayout(N, P)
        rng = np.random.default_rng(7 * sum(N) + P)
        A = rng.random(N).astype(rt)
        fwd_in = [np.ascontiguousarray(A[lay.real_slice(r)]) for r in range(P)]
        want = orc.line_r2c_forward(fwd_in, N, prec)
        if dealias is None:
            return dict(fwd_in=fwd_in, fwd_want=want, fwd_tol=TOL[prec], bwd_in=want, bwd_want=fwd_in, bwd_tol=4 * TOL[prec])
        crnd = [(rng.random(lay.complex_shape(r)) + 1j * rng.random(lay.complex_shape(r))).astype(ct) for r in range(P)]
        if dealias == "3/2-rule":
            Ap = rng.random((int(1.5 * N[0]), int(1.5 * N[1]))).astype(rt)
            pin = [np.ascontiguousarray(Ap[lay.real_slice(r, 1.5)]) for r in range(P)]
            return dict(fwd_in=pin, fwd_want=orc.line_r2c_forward_padded(pin, N, prec), fwd_tol=4 * TOL[prec],
                        bwd_in=crnd, bwd_want=orc.line_r2c_backward_padded(crnd, N, prec), bwd_tol=4 * TOL[prec])
        masks = [orc.line_dealias_mask(N, L2, lay, r) for r in range(P)]
        return dict(fwd_in=fwd_in, fwd_want=want, fwd_tol=TOL[prec], bwd_in=crnd,
                    bwd_want=orc.line_r2c_backward([(c * m).astype(ct) for c, m in zip(crnd, masks)], N, prec), bwd_tol=4 * TOL[prec])
    ref = _cached(("line", P, prec, dealias), make)
    _transform_case(P, lambda comm: Line_R2C(np.array(N), L2, comm, prec), ref, dealias, N, fwd="fft2", bwd="ifft2")


# ---- the nonlinear products ---------------------------------------------------------------------------------------------------
NFIELDS = {"cross": 2, "dot": 2, "cross_dot": 3}


def _nl_reference(product, N, prec, dealias):
    """Global spectra of real fields and the oracle's one-rank composition (tests/nonlinear_util.py), as the one-rank tests and
    test_nonlinear_*_ranks_against_oracle use them: 4 TOL."""
    N = [int(n) for n in N]

    def make():
        H = _host_class("slab", N, 1, 0, prec)
        fields = nl.spectra(tuple(H.complex_shape()), np.array(N), prec, 13 + N[2], True, NFIELDS[product])
        mask = H.get_dealias_filter() if dealias == "2/3-rule" else None
        want = nl.oracle(product, fields, np.array(N), prec, dealias, mask)
        want = list(want) if product == "cross_dot" else [want]
        ref = dict(fields=list(fields), want=[np.asarray(w) for w in want])
        if product != "cross_dot":          # the six real-space maxima of an absmax call
            ref["absmax"] = np.array([[np.abs(c).max() for c in nl.oracle_back(x, np.array(N), prec, dealias, mask)] for x in fields])
        return ref
    return _cached(("nl", product, tuple(N), prec, dealias), make)


def _nl_call(F, product, d, outs, dealias, absmax=False):
    from mpifft4py_amd import spectral
    if product == "cross":
        spectral.cross_transform(F, d[0], d[1], outs[0], dealias, absmax)
    elif product == "dot":
        spectral.dot_transform(F, d[0], d[1], outs[0], dealias, absmax)
    else:
        assert not absmax
        spectral.cross_dot_transform(F, d[0], d[1], d[2], outs[0], outs[1], dealias)


def _nl_out_shapes(product, cs):
    return {"cross": [(3,) + cs], "dot": [cs], "cross_dot": [(3,) + cs, cs]}[product]


def _nl_slab_case(product, N, P, prec, dealias, fused, absmax=False, complex_pitch=None):
    """Slab plans, one rank or several: inputs and outputs between guards, the gathered oracle sliced per rank."""
    from mpifft4py_amd import Slab_R2C, spectral
    ref = _nl_reference(product, N, prec, dealias)

    def body(comm):
        F = Slab_R2C(np.array(N), L, comm, prec, complex_pitch=complex_pitch)
        cs = tuple(int(x) for x in F.complex_shape())
        sl = tuple(F.complex_local_slice())
        d = [guarded((3,) + cs, F.complex, pitch=F.complex_pitch, fill=X[(slice(None),) + sl]) for X in ref["fields"]]
        outs = [guarded(s, F.complex, pitch=F.complex_pitch) for s in _nl_out_shapes(product, cs)]
        _nl_call(F, product, d, outs, dealias, absmax)
        F.sync()
        flag = F.plan_info(nl.info_key(product, dealias, absmax))
        problems = []
        for i, o in enumerate(outs):
            collect(problems, o, "rank %d %s output %d" % (comm.Get_rank(), product, i))
        for i, x in enumerate(d):
            collect(problems, x, "rank %d %s input %d" % (comm.Get_rank(), product, i))
        errs = [orc.rel_l2(o.get(), w[((slice(None),) + sl) if w.ndim == 4 else sl]) for o, w in zip(outs, ref["want"])]
        mx = spectral.nonlinear_absmax(F) if absmax else None
        return problems, errs, flag, mx, _route(F, N)
    res = run_ranks(P, body)
    print("route:", res[0][4], "fused flag", [r[2] for r in res])
    problems = [p for r in res for p in r[0]]
    assert not problems, "\n".join(problems)
    for _, errs, flag, mx, _ in res:
        assert flag == (1 if fused else 0), (flag, fused)
        print("%s P=%d %s %s: rel-L2 %s (bound %.1e)" % (product, P, dealias, prec, errs, 4 * TOL[prec]))
        assert max(errs) < 4 * TOL[prec], errs
        if absmax:                                       # the maxima tests' bound (tests/test_gpu_nonlinear_absmax.py): 4 TOL max|x|
            assert mx.shape == (2, 3) and np.all(np.abs(mx - ref["absmax"]) <= 4 * TOL[prec] * ref["absmax"]), (mx, ref["absmax"])


@pytest.mark.parametrize("prec", ["double", "single"])
@pytest.mark.parametrize("dealias", DEALIAS, ids=_id)
@pytest.mark.parametrize("N,fused", [([8, 16, 32], True), ([24, 40, 20], False)], ids=_id)
@pytest.mark.parametrize("product", nl.PRODUCTS)
def test_nonlinear_one_rank(product, N, fused, dealias, prec):
    """One rank: the fused route on [8, 16, 32] (flag 1) and the plan's own composition on [24, 40, 20] (no fused z kernel of length
    20 or 30: flag 0)."""
    _nl_slab_case(product, N, 1, prec, dealias, fused)


@pytest.mark.parametrize("prec", ["double", "single"])
@pytest.mark.parametrize("dealias", DEALIAS, ids=_id)
@pytest.mark.parametrize("product", nl.PRODUCTS)
def test_nonlinear_two_slab_ranks(product, dealias, prec):
    """Two slab ranks, the fused route behind the exchanges (flag 1, as test_nonlinear_cross_ranks asserts for slab plans)."""
    _nl_slab_case(product, [8, 16, 32], 2, prec, dealias, True)


@pytest.mark.parametrize("dealias", DEALIAS, ids=_id)
@pytest.mark.parametrize("product", nl.PRODUCTS)
def test_nonlinear_pitched_plan(product, dealias):
    """A plan with pitched spectra (rows a whole number of cache lines apart): the fused route runs on the pitched rows."""
    _nl_slab_case(product, [8, 16, 32], 1, "double", dealias, True, complex_pitch="auto")


@pytest.mark.parametrize("product", ["cross", "dot"])
def test_nonlinear_absmax_once(product):
    """absmax=True once per product that has it: the same arrays, the six maxima beside them."""
    _nl_slab_case(product, [8, 16, 32], 1, "double", "3/2-rule", True, absmax=True)


@pytest.mark.parametrize("dealias", DEALIAS, ids=_id)
@pytest.mark.parametrize("product", nl.PRODUCTS)
def test_nonlinear_pencil_grid(product, dealias):
    """A 2 x 2 pencil grid: the plan composes the operation (flag 0).  As test_nonlinear_cross_ranks / test_nonlinear_cross_dot_ranks:
    spectra of real fields made by the plan's own fftn, the result against the caller's composition from the same plan's ifftn,
    spectral.cross / spectral.dot and fftn on ordinary arrays, within 1e-13 (double)."""
    from mpifft4py_amd import DeviceArray, Pencil_R2C, spectral
    N = [8, 16, 32]

    def body(comm):
        F = Pencil_R2C(np.array(N), L, comm, "double", communication="Alltoallw", alignment="X")
        rng = np.random.default_rng(78 + comm.Get_rank())
        cs, ws = tuple(int(x) for x in F.complex_shape()), tuple(int(x) for x in F.work_shape(dealias))
        plain = [DeviceArray.empty((3,) + cs, F.complex) for _ in range(NFIELDS[product])]
        for x in plain:
            for i in range(3):
                F.fftn(DeviceArray.from_numpy(rng.random(F.real_shape()) - 0.5), x.component(i))
        real = [DeviceArray.empty((3,) + ws, F.float) for _ in plain]
        for x, u in zip(plain, real):
            for i in range(3):
                F.ifftn(x.component(i), u.component(i), dealias)
        want = []
        if product in ("cross", "cross_dot"):
            r, w = DeviceArray.empty((3,) + ws, F.float), DeviceArray.empty((3,) + cs, F.complex)
            spectral.cross(F, real[0], real[1], r)
            for i in range(3):
                F.fftn(r.component(i), w.component(i), dealias)
            want.append(w)
        if product in ("dot", "cross_dot"):
            r, w = DeviceArray.empty(ws, F.float), DeviceArray.empty(cs, F.complex)
            spectral.dot(F, real[0], real[-1], r)
            F.fftn(r, w, dealias)
            want.append(w)
        F.sync()
        d = [guarded((3,) + cs, F.complex, fill=x.get()) for x in plain]
        outs = [guarded(s, F.complex) for s in _nl_out_shapes(product, cs)]
        _nl_call(F, product, d, outs, dealias)
        F.sync()
        flag = F.plan_info(nl.info_key(product, dealias))
        problems = []
        for i, o in enumerate(outs):
            collect(problems, o, "rank %d %s output %d" % (comm.Get_rank(), product, i))
        for i, x in enumerate(d):
            collect(problems, x, "rank %d %s input %d" % (comm.Get_rank(), product, i))
        return problems, [orc.rel_l2(o.get(), w.get()) for o, w in zip(outs, want)], flag, _route(F, N)
    res = run_ranks(4, body)
    print("route:", res[0][3], "fused flag", [r[2] for r in res])
    problems = [p for r in res for p in r[0]]
    assert not problems, "\n".join(problems)
    for _, errs, flag, _ in res:
        assert flag == 0, flag
        assert max(errs) < 1e-13, errs


@pytest.mark.parametrize("product", nl.PRODUCTS)
def test_nonlinear_documented_aliasing(product):
    """The aliasing the docstrings allow (spectral.py): out_hat is a_hat (cross, cross_dot), out_hat / s_hat is one component of the
    last field (dot: b_hat.component(1); cross_dot: c_hat.component(1)).  The parent array is the guarded one; the fields not
    aliased come back bit for bit, and so do the other two components of the field that takes the scalar."""
    from mpifft4py_amd import SelfComm, Slab_R2C
    N, prec, dealias = [8, 16, 32], "double", "3/2-rule"
    ref = _nl_reference(product, N, prec, dealias)
    F = Slab_R2C(np.array(N), L, SelfComm(0), prec)
    cs = tuple(int(x) for x in F.complex_shape())
    d = [guarded((3,) + cs, F.complex, fill=X) for X in ref["fields"]]
    outs = ([d[0]] if product != "dot" else []) + ([d[-1].component(1)] if product != "cross" else [])
    _nl_call(F, product, d, outs, dealias)
    F.sync()
    assert F.plan_info(nl.info_key(product, dealias)) == 1
    print("route:", _route(F, N))
    last = ref["fields"][-1]
    if product in ("cross", "cross_dot"):
        check(d[0], "%s: out_hat over a_hat" % product, expect="output")
        assert orc.rel_l2(d[0].get(), ref["want"][0]) < 4 * TOL[prec]
    if product == "cross":
        check(d[1], "cross: b_hat", expect="input")
    if product == "cross_dot":
        check(d[1], "cross_dot: b_hat", expect="input")
    if product == "dot":
        check(d[0], "dot: a_hat", expect="input")
    if product in ("dot", "cross_dot"):
        check(d[-1], "%s: the field that takes the scalar" % product, expect="guards")
        got = d[-1].get()
        assert not np.isnan(got).any()
        assert orc.rel_l2(got[1], ref["want"][-1]) < 4 * TOL[prec]
        assert got[0].tobytes() == last[0].tobytes() and got[2].tobytes() == last[2].tobytes()


# ---- real_moments: inputs preserved, no output array --------------------------------------------------------------------------
@pytest.mark.parametrize("prec", ["double", "single"])
@pytest.mark.parametrize("dealias", DEALIAS, ids=_id)
@pytest.mark.parametrize("nfields", [1, 3, 6])
@pytest.mark.parametrize("N,fused", [([8, 16, 32], True), ([24, 40, 20], False)], ids=_id)
def test_real_moments_inputs_preserved(N, fused, nfields, dealias, prec):
    """1, 3 and 6 fields on the fused route (the z stage ends in a reduction) and on the composed one (one field at a time into one
    work array): the statistics within the bounds of tests/test_gpu_real_moments.py (its reference and its check), the guarded
    spectra untouched."""
    import test_gpu_real_moments as rm
    from mpifft4py_amd import SelfComm, Slab_R2C, spectral
    F = Slab_R2C(np.array(N), L, SelfComm(0), prec)
    a, b, ua, ub = rm._reference(N, prec, dealias)
    cs = tuple(int(x) for x in F.complex_shape())
    if nfields == 1:
        da, db = guarded(cs, F.complex, fill=a[0]), None
    else:
        da = guarded((3,) + cs, F.complex, fill=a)
        db = guarded((3,) + cs, F.complex, fill=b) if nfields == 6 else None
    m = spectral.real_moments(F, da, db, dealias)
    assert F.plan_info(rm.INFO(dealias)) == (1 if fused else 0)
    print("route:", _route(F, N), "fused flag", F.plan_info(rm.INFO(dealias)))
    check(da, "real_moments a_hat")
    if db is not None:
        check(db, "real_moments b_hat")
    fields = (list(ua) + list(ub))[:nfields]
    assert m.count == fields[0].size
    rm._check(rm._raw(m), fields, np.zeros(nfields), prec, "guarded %s %s nfields=%d" % (N, dealias, nfields),
              keys=rm._keys(N, prec, dealias)[:nfields])


# ---- element-wise kernels ---------------------------------------------------------------------------------------------------
# the local sizes of [8, 16, 32] and [7, 9, 22] (not a multiple of 256), one beyond 8192 * 256 elements (the grid-stride loop of
# ew_grid takes a second trip with a partial tail), and a pitched spectrum
EW_LAYOUTS = [([8, 16, 32], None), ([7, 9, 22], None), ([130, 130, 250], None), ([8, 16, 32], "auto")]
_EW_PLAN = {}


def _ew_plan(N, pitch, prec):
    from mpifft4py_amd import SelfComm, Slab_R2C
    key = (tuple(N), pitch, prec)
    if key not in _EW_PLAN:
        _EW_PLAN.clear()                                 # one plan at a time (the large mesh's work buffers)
        _EW_PLAN[key] = Slab_R2C(np.array(N), L3, SelfComm(0), prec, complex_pitch=pitch)
    return _EW_PLAN[key]


def _ew_wavenumbers(F):
    """spectral.Wavenumbers with its three device vectors between guards; (Kd, the vectors on the host, K broadcast in float64)."""
    from mpifft4py_amd import spectral
    Kd = spectral.Wavenumbers(F)
    Kd.dev = [guarded(v.shape, v.dtype, fill=v.get()) for v in Kd.dev]
    K = np.array(F.get_local_wavenumbermesh(scaled=True, broadcast=True)).astype(np.float64)
    return Kd, K


def _ew_close(got, want, prec, double_tol, single_tol, what):
    """double: np.allclose with rtol = atol = double_tol, as the existing double-precision test of the kernel; single: the same with
    the existing single-precision test's figure, or, where there is none (single_tol None), TOL["single"] as relative L2."""
    assert not np.isnan(got).any(), what
    if prec == "double" or single_tol is not None:
        tol = double_tol if prec == "double" else single_tol
        kw = {} if tol is None else dict(rtol=tol, atol=tol)
        assert np.allclose(got, want, **kw), (what, float(np.abs(got - want).max()))
    else:
        assert orc.rel_l2(got, want) < TOL["single"], (what, orc.rel_l2(got, want))


def _rnd(rng, shape, dtype):
    if np.dtype(dtype).kind == "c":
        return (rng.random(shape) + 1j * rng.random(shape)).astype(dtype)
    return rng.random(shape).astype(dtype)


def _ew_checks(arrays, Kd=None):
    """arrays: (view, what, expect) triples; the wavenumber vectors are read-only operands."""
    for v, what, expect in arrays:
        check(v, what, expect)
    if Kd is not None:
        for i, v in enumerate(Kd.dev):
            check(v, "wavenumber vector %d" % i, "input")


@pytest.mark.parametrize("prec", ["double", "single"])
@pytest.mark.parametrize("N", [x[0] for x in EW_LAYOUTS[:3]], ids=_id)
@pytest.mark.parametrize("kernel", ["cross", "dot"])
def test_ew_real_space(kernel, N, prec):
    """spectral.cross / spectral.dot on real vector fields (compact by contract) against numpy in float64; bounds of
    test_spectral_ops_match_numpy (cross, double: 1e-14) and test_ew_dot_and_grad_hat_against_numpy (dot: 1e-14 / 1e-6)."""
    from mpifft4py_amd import spectral
    F = _ew_plan(N, None, prec)
    rs = tuple(int(x) for x in F.real_shape())
    rng = np.random.default_rng(5 + sum(N))
    a, b = _rnd(rng, (3,) + rs, F.float) - 0.5, _rnd(rng, (3,) + rs, F.float) - 0.5
    da, db = guarded(a.shape, a.dtype, fill=a), guarded(b.shape, b.dtype, fill=b)
    a64, b64 = a.astype(np.float64), b.astype(np.float64)
    if kernel == "cross":
        out = guarded((3,) + rs, F.float)
        spectral.cross(F, da, db, out)
        want, tols = np.cross(a64, b64, axis=0), (1e-14, None)
    else:
        out = guarded(rs, F.float)
        spectral.dot(F, da, db, out)
        want, tols = np.sum(a64 * b64, 0), (1e-14, 1e-6)
    F.sync()
    print("route: mfft_ew_%s, %d elements per component, %s" % (kernel, a.size // 3, prec))
    _ew_checks([(out, kernel + " out", "output"), (da, kernel + " a", "input"), (db, kernel + " b", "input")])
    _ew_close(out.get(), want, prec, tols[0], tols[1], kernel)


@pytest.mark.parametrize("prec", ["double", "single"])
@pytest.mark.parametrize("N,pitch", EW_LAYOUTS, ids=_id)
@pytest.mark.parametrize("kernel", ["curl_hat", "grad_hat", "diag_grad_hat", "ns_rhs", "ns_rk_stage", "ns_rk_stage_last", "axpbz"])
def test_ew_spectral(kernel, N, pitch, prec):
    """The spectral-space kernels against numpy in float64, compact and on a pitched spectrum (swept as it lies in memory).  curl_hat,
    grad_hat, diag_grad_hat and axpbz write an output (poisoned); ns_rhs and ns_rk_stage update in place by contract (guards only);
    their read-only operands -- U_hat of ns_rhs, the wavenumber vectors -- come back bit for bit.  Double-precision bounds:
    test_spectral_ops_match_numpy (curl_hat, ns_rhs 1e-13; axpbz numpy's default), test_ew_dot_and_grad_hat_against_numpy (grad_hat
    1e-14), test_taylor_green_known_moments (diag_grad_hat: 1e-12 of the largest element), test_rk_stage_matches_numpy (1e-13);
    single: grad_hat 1e-6 and ns_rk_stage 2e-5 from the same tests, the others TOL["single"] as relative L2."""
    from mpifft4py_amd import spectral
    F = _ew_plan(N, pitch, prec)
    cs = tuple(int(x) for x in F.complex_shape())
    vs = (3,) + cs
    p = F.complex_pitch
    ct = F.complex
    rng = np.random.default_rng(8 + sum(N))
    Kd, K = _ew_wavenumbers(F)
    K2 = np.sum(K * K, 0)
    inp = lambda x: guarded(x.shape, x.dtype, pitch=p, fill=x)
    print("route: mfft_ew_%s, %d elements per component (in memory %d), pitch %s, %s"
          % (kernel, int(np.prod(cs)), int(np.prod(cs[:-1])) * (p or cs[-1]), p, prec))
    if kernel == "curl_hat":
        U = _rnd(rng, vs, ct)
        dU, W = inp(U), guarded(vs, ct, pitch=p)
        spectral.curl_hat(F, Kd, dU, W)
        F.sync()
        _ew_checks([(W, "curl_hat out", "output"), (dU, "curl_hat U_hat", "input")], Kd)
        _ew_close(W.get(), 1j * np.cross(K, U.astype(np.complex128), axis=0), prec, 1e-13, None, kernel)
    elif kernel == "grad_hat":
        s = _rnd(rng, cs, ct) - (0.5 + 0.5j)
        ds, dg = inp(s), guarded(vs, ct, pitch=p)
        spectral.grad_hat(F, Kd, ds, dg)
        F.sync()
        _ew_checks([(dg, "grad_hat out", "output"), (ds, "grad_hat s_hat", "input")], Kd)
        _ew_close(dg.get(), 1j * K * s.astype(np.complex128), prec, 1e-14, 1e-6, kernel)
    elif kernel == "diag_grad_hat":
        U = _rnd(rng, vs, ct)
        dU, G = inp(U), guarded(vs, ct, pitch=p)
        spectral.diag_grad_hat(F, Kd, dU, G)
        F.sync()
        _ew_checks([(G, "diag_grad_hat out", "output"), (dU, "diag_grad_hat U_hat", "input")], Kd)
        want, got = 1j * K * U.astype(np.complex128), G.get()
        assert not np.isnan(got).any()
        if prec == "double":
            assert np.allclose(got, want, rtol=0, atol=1e-12 * np.abs(want).max())
        else:
            assert orc.rel_l2(got, want) < TOL["single"]
    elif kernel == "ns_rhs":
        U, dU = _rnd(rng, vs, ct), _rnd(rng, vs, ct)
        d, u = inp(dU), inp(U)
        spectral.ns_rhs(F, Kd, d, u, 0.01)
        F.sync()
        _ew_checks([(d, "ns_rhs dU", "guards"), (u, "ns_rhs U_hat", "input")], Kd)
        U64, dU64 = U.astype(np.complex128), dU.astype(np.complex128)
        P_hat = np.sum(dU64 * K / np.where(K2 == 0, 1, K2), 0)
        _ew_close(d.get(), dU64 - P_hat * K - 0.01 * K2 * U64, prec, 1e-13, None, kernel)
    elif kernel.startswith("ns_rk_stage"):
        last = kernel.endswith("last")
        Nh, U, U0, U1 = (_rnd(rng, vs, ct) for _ in range(4))
        nu, a_dt, b_dt = 0.01, 0.02, 0.005
        h = [x.astype(np.complex128) for x in (Nh, U, U0, U1)]
        P_hat = np.sum(h[0] * K / np.where(K2 == 0, 1, K2), 0)
        dU = h[0] - P_hat * K - nu * K2 * h[1]
        U1n = h[3] + a_dt * dU
        Un = U1n if last else h[2] + b_dt * dU
        U0n = U1n if last else h[2]
        d = [inp(x) for x in (Nh, U, U0, U1)]
        spectral.ns_rk_stage(F, Kd, d[0], d[1], d[2], d[3], nu, a_dt, b_dt, last)
        F.sync()
        _ew_checks([(x, "ns_rk_stage array %d" % i, "guards") for i, x in enumerate(d)], Kd)
        for i, (got, want) in enumerate(zip(d, (1j * np.cross(K, Un, axis=0), Un, U0n, U1n))):
            _ew_close(got.get(), want, prec, 1e-13, 2e-5, "%s array %d" % (kernel, i))
    else:
        x, z = _rnd(rng, vs, ct), _rnd(rng, vs, ct)
        dx, dz, y = inp(x), inp(z), guarded(vs, ct, pitch=p)
        spectral.axpbz(F, y, dx, dz, 2.0, -0.5)
        F.sync()
        _ew_checks([(y, "axpbz y", "output"), (dx, "axpbz x", "input"), (dz, "axpbz z", "input")])
        _ew_close(y.get(), 2.0 * x.astype(np.complex128) - 0.5 * z.astype(np.complex128), prec, None, None, kernel)


# ---- stage level, straight through _lib.call ----------------------------------------------------------------------------------
# one length per mechanism and thread-value group: radix; chirp-z; the scratch-buffer route
STAGE_LENGTHS = [2, 8, 96, 240, 336, 448, 675, 1125, 2240, 4096, 8192, 7, 127, 1001, 4099, 8193]


def _stage_tol(n, real, prec):
    """TOL as test_c2c_every_length_every_axis / test_c2c_arbitrary_length_every_axis; 2 TOL for the lengths through the scratch
    buffer, as test_c2c_lengths_through_the_scratch_buffer_fallback.  Returns (bound, route)."""
    from mpifft4py_amd import _lib
    route = _lib.call("mfft_length_route_precision", n, 1 if real else 0, _lib.precision_code(prec))
    assert route in (1, 2, 3), (n, route)
    return (2 if route == 3 else 1) * TOL[prec], route


@pytest.mark.parametrize("prec", ["double", "single"])
@pytest.mark.parametrize("n", STAGE_LENGTHS)
def test_stage_c2c_axis(n, prec):
    """mfft_c2c_axis on each axis of a [3, 5, 7] batch with the length on the transformed axis, forward and inverse, out of place."""
    from mpifft4py_amd import _lib
    tol, route = _stage_tol(n, False, prec)
    print("route: mfft_length_route(%d, complex, %s) = %d" % (n, prec, route))
    rng = np.random.default_rng(n)
    for axis in (0, 1, 2):
        shape = [3, 5, 7]
        shape[axis] = n
        a = (rng.random(shape) - 0.5 + 1j * (rng.random(shape) - 0.5)).astype(cdtype(prec))
        a128 = a.astype(np.complex128)
        for inverse in (0, 1):
            din, out = guarded(a.shape, a.dtype, fill=a), guarded(a.shape, a.dtype)
            _lib.call("mfft_c2c_axis", din.ptr, out.ptr, (ctypes.c_int64 * 3)(*shape), axis, inverse, _lib.precision_code(prec))
            check(out, "c2c_axis n=%d axis %d inverse %d out" % (n, axis, inverse))
            check(din, "c2c_axis n=%d axis %d inverse %d in" % (n, axis, inverse))
            want = (np.fft.ifft if inverse else np.fft.fft)(a128, axis=axis)
            assert orc.rel_l2(out.get(), want) < tol, (n, axis, inverse, orc.rel_l2(out.get(), want))


@pytest.mark.parametrize("prec", ["double", "single"])
@pytest.mark.parametrize("n", STAGE_LENGTHS)
def test_stage_c2c_strided(n, prec):
    """mfft_c2c_strided: 3 batches of 5 columns in rows 8 (in) and 7 (out) elements apart, forward and inverse; the columns of the
    output that lie between the rows stay poisoned -- every byte of them --, the 5 transformed ones hold no NaN."""
    from mpifft4py_amd import _lib
    tol, route = _stage_tol(n, False, prec)
    print("route: mfft_length_route(%d, complex, %s) = %d" % (n, prec, route))
    rng = np.random.default_rng(n + 3)
    nouter, ncols, ip, op = 3, 5, 8, 7
    a = (rng.random((nouter, n, ip)) - 0.5 + 1j * (rng.random((nouter, n, ip)) - 0.5)).astype(cdtype(prec))
    for inverse in (0, 1):
        din, out = guarded(a.shape, a.dtype, fill=a), guarded((nouter, n, op), a.dtype)
        _lib.call("mfft_c2c_strided", din.ptr, out.ptr, n, nouter, ncols, n * ip, ip, n * op, op, inverse, _lib.precision_code(prec))
        check(out, "c2c_strided n=%d inverse %d out" % (n, inverse), expect="guards")
        check(din, "c2c_strided n=%d inverse %d in" % (n, inverse))
        got = out.get()
        assert not np.isnan(got[:, :, :ncols]).any(), "poisoned element left in the transformed columns"
        assert np.all(np.ascontiguousarray(got[:, :, ncols:]).view(np.uint8) == 0xFF), "a column between the rows was written"
        want = (np.fft.ifft if inverse else np.fft.fft)(a[:, :, :ncols].astype(np.complex128), axis=1)
        assert orc.rel_l2(got[:, :, :ncols], want) < tol, (n, inverse, orc.rel_l2(got[:, :, :ncols], want))


def _real_lengths():
    """Twice the complex lengths, where the library says the real length is supported (mfft_length_route, device-free); where the
    library cannot be asked at collection time, all of them: the test then fails by itself."""
    try:
        from mpifft4py_amd import _lib
        return [2 * m for m in STAGE_LENGTHS if _lib.call("mfft_length_route", 2 * m, 1) != 0]
    except Exception:      # noqa: BLE001
        return [2 * m for m in STAGE_LENGTHS]


@pytest.mark.parametrize("prec", ["double", "single"])
@pytest.mark.parametrize("n", _real_lengths())
def test_stage_real_pair(n, prec):
    """mfft_r2c_last / mfft_c2r_last at twice the complex lengths, where mfft_length_route says the real length is supported, on a
    [3, 5, n] batch; c2r ignores the imaginary parts of bins 0 and n/2 (as test_rfft_irfft_every_length feeds them)."""
    from mpifft4py_amd import _lib
    tol, route = _stage_tol(n, True, prec)
    print("route: mfft_length_route(%d, real, %s) = %d" % (n, prec, route))
    rng = np.random.default_rng(n + 1)
    a = (rng.random((3, 5, n)) - 0.5).astype(rdtype(prec))
    shape = (ctypes.c_int64 * 3)(3, 5, n)
    din, out = guarded(a.shape, a.dtype, fill=a), guarded((3, 5, n // 2 + 1), cdtype(prec))
    _lib.call("mfft_r2c_last", din.ptr, out.ptr, shape, _lib.precision_code(prec))
    check(out, "r2c_last n=%d out" % n)
    check(din, "r2c_last n=%d in" % n)
    ref = np.fft.rfft(a.astype(np.float64), axis=2)
    assert orc.rel_l2(out.get(), ref) < tol, orc.rel_l2(out.get(), ref)
    c = ref.astype(cdtype(prec)).copy()
    c[..., 0] += 1j * 0.7
    c[..., -1] -= 1j * 0.3
    dc, back = guarded(c.shape, c.dtype, fill=c), guarded(a.shape, a.dtype)
    _lib.call("mfft_c2r_last", dc.ptr, back.ptr, shape, _lib.precision_code(prec))
    check(back, "c2r_last n=%d out" % n)
    check(dc, "c2r_last n=%d in" % n)
    got = back.get()
    assert orc.rel_l2(got, np.fft.irfft(c.astype(np.complex128), n=n, axis=2)) < tol
    assert orc.rel_l2(got, a) < 4 * TOL[prec]


@pytest.mark.parametrize("prec", ["double", "single"])
def test_stage_pack_unpack_and_filter(prec):
    """mfft_slab_pack, mfft_slab_unpack and mfft_dealias_filter with the shapes and the bit-exact checks of tests/test_gpu_stages.py;
    the filter works in place (guards only), its mask is read-only."""
    from mpifft4py_amd import _lib
    rng = np.random.default_rng(3)
    P, Np0, Np1, Nf = 4, 6, 5, 17
    T = (rng.random((Np0, P * Np1, Nf)) + 1j * rng.random((Np0, P * Np1, Nf))).astype(cdtype(prec))
    dT, dM = guarded(T.shape, T.dtype, fill=T), guarded((P, Np0, Np1, Nf), T.dtype)
    _lib.call("mfft_slab_pack", dT.ptr, dM.ptr, P, Np0, Np1, Nf, _lib.precision_code(prec))
    check(dM, "slab_pack out")
    check(dT, "slab_pack in")
    assert np.array_equal(dM.get(), orc.slab_pack(T, P))
    packed = orc.slab_pack(T, P)
    dP, dT2 = guarded(packed.shape, packed.dtype, fill=packed), guarded(T.shape, T.dtype)
    _lib.call("mfft_slab_unpack", dP.ptr, dT2.ptr, P, Np0, Np1, Nf, _lib.precision_code(prec))
    check(dT2, "slab_unpack out")
    check(dP, "slab_unpack in")
    assert np.array_equal(dT2.get(), T)
    fu = (rng.random((9, 10, 11)) + 1j * rng.random((9, 10, 11))).astype(cdtype(prec))
    mask = (rng.random(fu.shape) > 0.4).astype(np.uint8)
    d, dm = guarded(fu.shape, fu.dtype, fill=fu), guarded(mask.shape, mask.dtype, fill=mask)
    _lib.call("mfft_dealias_filter", d.ptr, dm.ptr, fu.size, _lib.precision_code(prec))
    check(d, "dealias_filter fu", expect="guards")
    check(dm, "dealias_filter mask")
    assert np.array_equal(d.get(), orc.apply_mask(fu, mask).astype(fu.dtype))
