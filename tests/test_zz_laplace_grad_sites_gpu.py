"""GPU (MI355X): every entry point of the gradient half of gpboost_amd/csrc/gpb_laplace.inc returns what it returned at the commit before that half was cut into
stages (tests/golden/laplace_grad_sites_parent.npz; tests/laplace_grad_sites.py lists the calls, scripts/record_laplace_grad_sites.py records them, twice).

A quantity whose two parent recordings agree bit for bit is held to those bits.  One whose recordings differ is held to the parent's own spread, widened to no
more than the tolerance of the existing test of that path (laplace_grad_sites.EXISTING_TOL).  At the recorded parent all 54 quantities fell into the first class:
the gradient's kernels are fixed-order and atomic-free, and so are the mode finding and the log-determinant before them.  The refusals' messages compare exactly."""
import os

import numpy as np
import pytest

from tests import laplace_grad_sites as S

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", S.FIXTURE)


@pytest.fixture(scope="module")
def gpb(lib_built):
    import gpboost_amd
    assert gpboost_amd.device_count() > 0, "no GPU visible: the -m gpu tests must run on the MI355X box"
    return gpboost_amd


@pytest.fixture(scope="module")
def golden():
    with np.load(GOLDEN) as f:
        return {k: f[k] for k in f.files}


@pytest.fixture(scope="module")
def got(gpb):
    return S.collect()


@pytest.fixture(scope="module")
def messages(gpb):
    return S.refusals()


def test_the_fixture_holds_exactly_these_quantities(golden):
    assert sorted(k[2:] for k in golden if k.startswith("a/")) == sorted(S.NAMES) == sorted(k[2:] for k in golden if k.startswith("b/"))
    assert sorted(k[len("refusal/"):] for k in golden if k.startswith("refusal/")) == sorted(S.REFUSALS)


def test_every_quantity_is_produced(got, messages):
    assert sorted(got) == sorted(S.NAMES) and sorted(messages) == sorted(S.REFUSALS)


@pytest.mark.parametrize("name", S.NAMES)
def test_site_as_at_the_parent(got, golden, name):
    a, b, v = golden["a/" + name], golden["b/" + name], got[name]
    assert v.shape == a.shape and np.all(np.isfinite(a))
    diff = np.abs(v - a).max()
    print("%s: largest difference from the parent %.3e (largest magnitude %.3e)" % (name, diff, np.abs(a).max()))
    if np.array_equal(a.view(np.uint64), b.view(np.uint64)):
        assert np.array_equal(v.view(np.uint64), a.view(np.uint64)), "%s differs from commit %s by up to %.3e" % (name, str(golden["parent"]), diff)
    else:
        bound = max(np.abs(a - b).max(), S.EXISTING_TOL[name.split("/")[1]] * np.abs(a).max())
        assert min(diff, np.abs(v - b).max()) <= bound, (name, diff, bound)


@pytest.mark.parametrize("name", S.REFUSALS)
def test_refusal_in_the_same_words(messages, golden, name):
    assert messages[name] == str(golden["refusal/" + name]) != ""
