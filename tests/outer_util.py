"""What the tests of the outer product (test_gpu_nonlinear_outer.py, test_gpu_guarded_outer.py) share: the oracle's composition
of the nine products, the plan_info keys and the fresh child process the once-per-process switches need.  An ordinary module,
like nonlinear_util.py, which it builds on; the child processes import it too."""
import numpy as np

import nonlinear_util as nl
from gpu_util import orc, rdtype

RULE = nl.RULE


def info_key(dealias):
    """The plan_info key "does the fused route take the outer product in this mode"."""
    return "nonlinear_outer_fused_%s" % RULE[dealias]


def oracle_outer(ua, ub, N, prec, dealias):
    """fftn of the nine products ua[i] * ub[j] of two real vector fields with the oracle's forward transform in the mode
    `dealias`: component 3 i + j."""
    if dealias == "3/2-rule":
        fwd = lambda x: orc.slab_r2c_forward_padded([x], N, prec)[0]
    else:
        fwd = lambda x: orc.slab_r2c_forward([x], N, prec)[0]
    return np.stack([fwd((ua[i] * ub[j]).astype(rdtype(prec))) for i in range(3) for j in range(3)])


def oracle(a, b, N, prec, dealias, mask=None):
    """What a caller composes from the oracle's transforms: back-transform both fields, the nine products, forward-transform."""
    ua = nl.oracle_back(a, N, prec, dealias, mask)
    ub = ua if b is a else nl.oracle_back(b, N, prec, dealias, mask)
    return oracle_outer(ua, ub, N, prec, dealias)


def transform(F, a, b, dealias):
    """The plan operation on host spectra, out of place: the nine components as a host array."""
    from mpifft4py_amd import spectral
    da, db = F.empty_complex(3).set(a), F.empty_complex(3).set(b)
    out = F.empty_complex(9)
    spectral.outer_transform(F, da, db, out, dealias)
    F.sync()
    return out.get()


def check_cases_in_child(cases, fused, bound, **env):
    """In a fresh process under `env`: every (N, dealias) of `cases` on a one-rank double-precision slab plan, spectra of real
    fields from seed 3, against the oracle within `bound`; the fused flag of the plan is `fused`."""
    return nl.run_child("""
import outer_util as ou
for N, dealias in %r:
    N = np.array(N)
    F = Slab_R2C(N, L, SelfComm(0), 'double')
    a, b = nl.spectra(tuple(F.complex_shape()), N, 'double', 3, True, 2)
    want = ou.oracle(a, b, N, 'double', dealias, F.get_dealias_filter() if dealias == '2/3-rule' else None)
    got = ou.transform(F, a, b, dealias)
    assert F.plan_info(ou.info_key(dealias)) == %d
    errs = [orc.rel_l2(got[c], want[c]) for c in range(9)]
    print(list(N), dealias, errs)
    assert max(errs) < %r, errs
print('ok')
""" % (tuple(cases), fused, bound), **env)
