"""GPU (MI355X): the likelihood kernels of the Vecchia-Laplace path per datum, through the test entry gpb_hip_laplace_lik_check, against the 60-digit restatement
of tests/lik_terms_ref.py and its a-priori bound  u (E_arith + sum_f eps_f E_lib,f).

First the probe: the device's exp / log / log1p / erfc / lgamma / sqrt (compiled with the kernels' flags) against mpmath at every argument at which the grid calls
them; eps_f = max(2, 2 x the worst relative error in units of u = 2^-53) -- the factor 2 allows for arguments between the sampled ones -- and every eps_f <= 16.
Then every output of the entry, element by element, at its bound with no further factor: per-row log-likelihood, W, rhs, dw, rdw, dW3, both boosting gradients,
out2 and out3."""
import numpy as np
import pytest

import gpboost_amd
from gpboost_amd import shim
from tests import lik_terms_ref as R

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eps(lib_built):
    """eps_f of the device's library functions, measured once per session over the arguments the grid hands them"""
    assert gpboost_amd.device_count() > 0
    for lik in range(9):       # fills R.LIB_ARGS
        for ci in range(len(R.cases(lik))):
            R.reference(lik, ci)
    out = {}
    for f in R.LIB:
        args = sorted(R.LIB_ARGS[f]) if R.LIB_ARGS[f] else sorted(abs(a) for a in R.LIB_ARGS["log"])      # (no kernel of this family calls sqrt)
        x = np.array(args, dtype=np.float64)
        dev = shim.math_probe(f, x)
        worst, at = 0.0, None
        for a, d in zip(args, dev):
            t = R._MPFN[f](R.MP.mpf(a))
            e = float(abs(R.MP.mpf(float(d)) - t) / (R.MP.mpf(R.U) * max(abs(t), R.MP.mpf(R.TINY)))) if np.isfinite(d) else np.inf
            if e > worst:
                worst, at = e, a
        out[f] = max(2.0, 2.0 * worst)
        print("probe %-6s %4d arguments in [%.3g, %.3g]: worst error %.3f u at %r -> eps_%s = %.3f" % (f, len(args), args[0], args[-1], worst, at, f, out[f]))
    return out


def test_device_math_library_is_within_16_u(eps):
    for f, e in eps.items():
        assert e <= 16.0, "device %s: eps = %.3g > 16 over the grid's arguments; see the printed range" % (f, e)


@pytest.mark.parametrize("lik", list(range(9)), ids=R.LIK_NAMES)
def test_every_output_at_its_bound(lik, eps):
    worst, failures = {}, []
    for ci, c in enumerate(R.cases(lik)):
        ref = R.reference(lik, ci)
        assert ref.finite and not ref.defects
        case = ref.case
        res = shim.laplace_lik_check(**case.entry_kwargs())
        assert R.HAS_AUX[lik] or np.all(np.isnan(res["out3"])), "out3 of a likelihood without auxiliary parameters stays as the entry pre-set it"
        got = ref.outputs_of_entry(res)
        assert set(got) == set(ref.out)
        for name, g in got.items():
            r = ref.ratio(name, g, eps)
            if not r.size:
                continue
            worst[name] = max(worst.get(name, 0.0), float(r.max()))
            if r.max() > 1.0:
                bad = np.argsort(-r)[:3]
                o = ref.out[name]
                failures.append("%s case %s output %s: %d of %d over the bound; worst %s" % (
                    R.LIK_NAMES[lik], c, name, int((r > 1.0).sum()), r.size,
                    ["[%d] ratio %.3g device %.17g truth %.17g (%s)" % (int(b), r[b], np.asarray(g)[b], o["hi"][b], ref.where(name, int(b))) for b in bad]))
    print("GPU ratios %-18s %s" % (R.LIK_NAMES[lik], "  ".join("%s %.2f" % kv for kv in sorted(worst.items()))))
    assert not failures, "\n".join(failures)


def test_entry_refuses_what_it_cannot_run(lib_built):
    one = np.ones(3)
    with pytest.raises(gpboost_amd.GPBoostError):
        shim.laplace_lik_check("poisson", one, one, one, one, y_real=one)                       # counts are never real-valued
    with pytest.raises(gpboost_amd.GPBoostError):
        shim.laplace_lik_check("gamma", one, one, one, one, y_int=np.ones(3, dtype=np.int32))  # a real-only likelihood
    with pytest.raises(gpboost_amd.GPBoostError):
        shim.laplace_lik_check("poisson", one, one, one, one, y_int=np.ones(5, dtype=np.int32), re_ptr=[0, 2, 1, 5])
    with pytest.raises(gpboost_amd.GPBoostError):
        shim.laplace_lik_check(9, one, one, one, one, y_int=np.ones(3, dtype=np.int32))
