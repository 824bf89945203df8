"""GPU (MI355X): every device-side site whose k x k host algebra moved into gpboost_amd/csrc/gpb_smallmat.h returns what it returned at the commit before the header
existed (tests/golden/smallmat_sites_parent.npz; tests/smallmat_sites.py lists the calls, scripts/record_smallmat_sites.py records them, twice).

A quantity whose two parent recordings agree bit for bit is held to those bits.  One whose recordings differ -- a device reduction whose order is not fixed -- is
held to the parent's own spread, widened to no more than the tolerance of the existing test of that path (smallmat_sites.EXISTING_TOL).  At the recorded parent
all 14 quantities fell into the first class."""
import os

import numpy as np
import pytest

from tests import smallmat_sites as S

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


NAMES = ["vif_gauss/nll", "vif_gauss/grad", "vif_gauss/pred_mu", "vif_gauss/pred_var", "vif_fitc/nll", "vif_fitc/grad", "vif_fitc/parts",
         "lap_pivchol/nll", "lap_pivchol/grad", "lap_pivchol/parts", "leaf/values", "fisher/cov_pars_std", "coef/cov_pars", "coef/coef_std"]


def test_the_fixture_holds_exactly_these_quantities(golden):
    assert sorted(k[2:] for k in golden if k.startswith("a/")) == sorted(NAMES) == sorted(k[2:] for k in golden if k.startswith("b/"))


@pytest.mark.parametrize("name", NAMES)
def test_site_as_at_the_parent(got, golden, name):
    a, b, v = golden["a/" + name], golden["b/" + name], got[name]
    assert v.shape == a.shape and np.all(np.isfinite(a))
    diff = np.abs(v - a).max()
    print("%s: largest difference from the parent %.3e (largest magnitude %.3e)" % (name, diff, np.abs(a).max()))
    if np.array_equal(a.view(np.uint64), b.view(np.uint64)):
        assert np.array_equal(v.view(np.uint64), a.view(np.uint64)), "%s differs from commit %s by up to %.3e" % (name, str(golden["parent"]), diff)
    else:
        bound = max(np.abs(a - b).max(), S.EXISTING_TOL[name.split("/")[0]] * np.abs(a).max())
        assert min(diff, np.abs(v - b).max()) <= bound, (name, diff, bound)


def test_full_scale_model_refuses_pivoted_cholesky_in_the_same_words(gpb):
    assert S.vif_pivchol_refusal() == S.VIF_PIVCHOL_REFUSAL
