"""What the tests of the nonlinear term (test_gpu_nonlinear*.py) share: the seeded spectra, the oracle's composition of the
three products, the plan_info keys and the fresh child process the once-per-process switches need.  An ordinary module, like
gpu_util.py; the child processes import it too."""
import os
import subprocess
import sys

import numpy as np

from gpu_util import cdtype, orc, rdtype

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RULE = {"3/2-rule": "3_2", "2/3-rule": "2_3", None: "none"}
PRODUCTS = ("cross", "dot", "cross_dot")       # as in csrc/mfft_internal.h NL_PRODUCTS; the first two also with maxima


def info_key(product, dealias, absmax=False):
    """The plan_info key "does the fused route take this product (with maxima) in this mode": the cross product goes unnamed."""
    assert product in PRODUCTS
    return "nonlinear%s%s_fused_%s" % ("" if product == "cross" else "_" + product, "_absmax" if absmax else "", RULE[dealias])


def fused_keys():
    """Every such key the plan knows: three products and two with maxima, three modes each."""
    return [info_key(p, d, m) for p in PRODUCTS for m in ((False,) if p == "cross_dot" else (False, True)) for d in RULE]


def spectra(cs, N, prec, seed, hermitian, nfields=2):
    """`nfields` vector fields in spectral space: transforms of random real fields (what a solver holds), or arbitrary complex
    numbers of the local complex shape `cs` (the transforms' conventions for the bins a real field would not have: c2r ignores
    Im of kz = 0, N/2).  Drawn field by field from one generator."""
    rng = np.random.default_rng(seed)
    if hermitian:
        f = [np.stack([np.fft.rfftn(rng.random(tuple(N)) - 0.5) for _ in range(3)]) for _ in range(nfields)]
    else:
        f = [rng.random((3,) + cs) - 0.5 + 1j * (rng.random((3,) + cs) - 0.5) for _ in range(nfields)]
    return tuple(x.astype(cdtype(prec)) for x in f)


def oracle_back(x, N, prec, dealias, mask=None):
    """ifftn of the three components of x with the oracle's one-rank transform in the mode `dealias` (2/3-rule: `mask`), float64."""
    if dealias == "3/2-rule":
        back = lambda y: orc.slab_r2c_backward_padded([y], N, prec)[0]
    else:
        back = lambda y: orc.slab_r2c_backward([y if mask is None else orc.apply_mask(y, mask)], N, prec)[0]
    return np.stack([np.asarray(back(x[i]), dtype=np.float64) for i in range(3)])


def oracle_product(product, u, N, prec, dealias):
    """fftn of the product of the real vector fields u = (ua, ub[, uc]): the cross product ua x ub (three components), the dot
    product sum_f ua_f ub_f (one), or for "cross_dot" the pair (ua x ub, sum_f ua_f uc_f)."""
    if dealias == "3/2-rule":
        fwd = lambda x: orc.slab_r2c_forward_padded([x], N, prec)[0]
    else:
        fwd = lambda x: orc.slab_r2c_forward([x], N, prec)[0]

    def cross(ua, ub):
        r = np.cross(ua, ub, axis=0).astype(rdtype(prec))
        return np.stack([fwd(r[i]) for i in range(3)])

    def dot(ua, ub):
        return fwd(np.sum(ua * ub, 0).astype(rdtype(prec)))
    if product == "cross_dot":
        return cross(u[0], u[1]), dot(u[0], u[2])
    return {"cross": cross, "dot": dot}[product](u[0], u[1])


def oracle(product, fields, N, prec, dealias, mask=None):
    """What a caller composes from the oracle's transforms: back-transform every field, the product, forward-transform."""
    return oracle_product(product, [oracle_back(x, N, prec, dealias, mask) for x in fields], N, prec, dealias)


def transform(F, product, fields, dealias):
    """The plan operation of `product` on host spectra, out of place: the result(s) as a tuple of host arrays."""
    from mpifft4py_amd import spectral
    d = [F.empty_complex(3).set(x) for x in fields]
    if product == "cross_dot":
        out = (F.empty_complex(3), F.empty_complex())
        spectral.cross_dot_transform(F, d[0], d[1], d[2], out[0], out[1], dealias)
    else:
        out = (F.empty_complex(3) if product == "cross" else F.empty_complex(),)
        (spectral.cross_transform if product == "cross" else spectral.dot_transform)(F, d[0], d[1], out[0], dealias)
    F.sync()
    return tuple(x.get() for x in out)


_CHILD = """
import sys, numpy as np
sys.path.insert(0, %r); sys.path.insert(0, %r)
from gpu_util import L, TOL, orc
from mpifft4py_amd import DeviceArray, SelfComm, Slab_R2C, spectral
import nonlinear_util as nl
""" % (ROOT, os.path.join(ROOT, "tests"))


def run_child(code, timeout=600, **env):
    """`code`, after the imports above, in a fresh Python process with the environment switches `env` (the library reads them
    once per process).  The code ends by printing ok."""
    r = subprocess.run([sys.executable, "-c", _CHILD + code], env=dict(os.environ, **env), capture_output=True, text=True, timeout=timeout)
    assert r.returncode == 0 and "ok" in r.stdout.splitlines()[-1:], r.stdout[-3000:] + r.stderr[-3000:]
    return r.stdout


def check_cases_in_child(product, cases, fused, bound, **env):
    """In a fresh process under `env`: every (N, dealias) of `cases` on a one-rank double-precision slab plan, spectra of real
    fields from seed 3, against the oracle within `bound`; the fused flag of the plan is `fused`."""
    return run_child("""
product, nfields = %r, %d
for N, dealias in %r:
    N = np.array(N)
    F = Slab_R2C(N, L, SelfComm(0), 'double')
    fields = nl.spectra(tuple(F.complex_shape()), N, 'double', 3, True, nfields)
    want = nl.oracle(product, fields, N, 'double', dealias, F.get_dealias_filter() if dealias == '2/3-rule' else None)
    got = nl.transform(F, product, fields, dealias)
    assert F.plan_info(nl.info_key(product, dealias)) == %d
    errs = [orc.rel_l2(g, w) for g, w in zip(got, want if product == 'cross_dot' else (want,))]
    print(list(N), dealias, errs)
    assert max(errs) < %r, errs
print('ok')
""" % (product, 3 if product == "cross_dot" else 2, tuple(cases), fused, bound), **env)
