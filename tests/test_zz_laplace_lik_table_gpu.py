"""GPU (MI355X): the host paths of the Vecchia-Laplace C ABI that ask the likelihood table (gpboost_amd/csrc/lik_table.h) what a likelihood is --
which response setter it takes, the domain of the response, the number and labels of its auxiliary parameters -- for every id 0 .. 8.
The expected messages are written out here, per id, as the library printed them when each of these entry points still kept its own list of ids;
none of them is assembled from the table or from shim._LIKELIHOODS.  Nothing is evaluated: beyond creating the handle (n = 64, m = 10) no kernel runs."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N, M, POS = 64, 10, 5        # POS: where the one out-of-domain value sits

NAMES = ["bernoulli_logit", "bernoulli_probit", "poisson", "gamma", "negative_binomial", "beta", "t", "lognormal", "gaussian_latent"]
NUM_AUX = [0, 0, 0, 1, 1, 1, 2, 1, 1]
REAL_ONLY = {3: "gamma", 5: "beta", 6: "t", 7: "lognormal", 8: "gaussian_latent"}          # set_labels refused
COUNTS = {2: "poisson", 4: "negative_binomial"}                                             # set_response_real refused
# a response the likelihood accepts (constant vector), and one value outside its domain with the message it gets
GOOD_REAL = {0: 0.25, 1: 0.25, 3: 1.5, 5: 0.25, 6: -2.0, 7: 1.5, 8: -2.0}
BAD_REAL = {
    0: (1.5, " Must have 0 <= y <= 1 for the response variable ('y') (found 1.5 at Vecchia position 5)"),
    1: (1.5, " Must have 0 <= y <= 1 for the response variable ('y') (found 1.5 at Vecchia position 5)"),
    3: (0.0, "gamma: the response must be > 0 (found 0 at Vecchia position 5)"),
    5: (1.0, " Must have 0 < y < 1 for the response variable ('y') for likelihood = 'beta', found 1 "),
    6: (np.inf, "t: the response must be finite (found inf at Vecchia position 5)"),
    7: (0.0, "lognormal: the response must be > 0 (found 0 at Vecchia position 5)"),
    8: (np.inf, "gaussian_latent: the response must be finite (found inf at Vecchia position 5)"),
}
BAD_COUNT = {2: "poisson: the response must be >= 0 (found -1 at Vecchia position 5)",
             4: "negative_binomial: the response must be >= 0 (found -1 at Vecchia position 5)"}
REAL_REFUSED = ("gpb_hip_vecchia_laplace_set_response_real: a real-valued response is for gamma, beta, t, lognormal, gaussian_latent and for proportions "
                "under the logit / probit links (likelihood id %d)")
LABELS_REFUSED = "%s: the response is real-valued (call gpb_hip_vecchia_laplace_set_response_real)"
NO_AUX = "gpb_hip_vecchia_laplace_set_aux_pars: likelihood id %d has no auxiliary parameters"
WRONG_COUNT = ("gpb_hip_vecchia_laplace_set_aux_pars: %d parameters (gamma / negative_binomial have one, the shape; beta one, the precision; t two: scale, df; "
               "lognormal one, the variance of log y)")
AUX_LABEL = {3: "shape", 4: "shape", 5: "shape", 6: "scale", 7: "log_variance", 8: "error_variance"}
BAD_ID = ("gpb_hip_vecchia_laplace_set_likelihood: id %d (0 = bernoulli_logit, 1 = bernoulli_probit, 2 = poisson, 3 = gamma, 4 = negative_binomial, 5 = beta, "
          "6 = t, 7 = lognormal, 8 = gaussian_latent)")


@pytest.fixture(scope="module")
def st(lib_built):
    import gpboost_amd
    from gpboost_amd import shim
    assert gpboost_amd.device_count() > 0, "no GPU visible: the -m gpu tests must run on the MI355X box"
    s = shim.VecchiaState(np.random.default_rng(3).uniform(size=(N, 2)), M)
    yield s
    s.close()


def _refused(call, *args):
    from gpboost_amd.basic import GPBoostError
    with pytest.raises(GPBoostError) as e:
        call(*args)
    return str(e.value)


def _num_aux(st):
    from gpboost_amd.basic import _lib
    k = C.c_int32(-1)
    assert _lib().gpb_hip_vecchia_laplace_get_aux_pars(st.h, None, C.byref(k)) == 0
    return k.value


@pytest.mark.parametrize("lid", range(9))
def test_response_setters_follow_the_likelihood(st, lid):
    st.laplace_set_likelihood(NAMES[lid])
    labels = np.ones(N, dtype=np.int32)
    if lid in REAL_ONLY:
        assert _refused(st.laplace_set_labels, labels) == LABELS_REFUSED % REAL_ONLY[lid]
    else:
        st.laplace_set_labels(labels)
    if lid in COUNTS:
        assert _refused(st.laplace_set_response_real, np.full(N, 2.0)) == REAL_REFUSED % lid
        bad = labels.copy(); bad[POS] = -1
        assert _refused(st.laplace_set_labels, bad) == BAD_COUNT[lid]
    else:
        st.laplace_set_response_real(np.full(N, GOOD_REAL[lid]))
        value, msg = BAD_REAL[lid]
        bad = np.full(N, GOOD_REAL[lid]); bad[POS] = value
        assert _refused(st.laplace_set_response_real, bad) == msg


@pytest.mark.parametrize("lid", range(9))
def test_auxiliary_parameters_follow_the_likelihood(st, lid):
    st.laplace_set_likelihood(NAMES[lid])
    k = NUM_AUX[lid]
    assert _num_aux(st) == k
    if k == 0:
        assert _refused(st.laplace_set_aux, 1.0) == NO_AUX % lid
        assert _refused(st.laplace_set_aux, [1.0, 2.0]) == NO_AUX % lid
        return
    wrong = 1 if k == 2 else 2
    assert _refused(st.laplace_set_aux, [1.5, 3.0][:wrong]) == WRONG_COUNT % wrong
    assert _refused(st.laplace_set_aux, [-0.5, 3.0][:k]) == "The %s parameter is not > 0 (found -0.5)" % AUX_LABEL[lid]
    if k == 2:
        assert _refused(st.laplace_set_aux, [1.5, 0.0]) == "The df parameter is not > 0 (found 0)"
    st.laplace_set_aux([1.5, 3.0][:k])
    assert _num_aux(st) == k


@pytest.mark.parametrize("bad", [-1, 9])
def test_unknown_likelihood_id_is_refused(st, bad):
    from gpboost_amd.basic import _lib, _shim_call
    assert _refused(lambda: _shim_call(_lib().gpb_hip_vecchia_laplace_set_likelihood(st.h, C.c_int(bad)))) == BAD_ID % bad
    st.laplace_set_likelihood("t")        # ... and the handle keeps working
    assert _num_aux(st) == 2
