"""GPU (MI355X), and the same file on the CPU restatement of the shim: the prediction host code (gpboost_amd/csrc/gpb_predict.inc: pred_resolve, the dispatch pred_path,
one function per model path, the shared forward substitution / lower solve / second-moment store) returns the SAME BITS and the SAME MESSAGES as the commit before
GPB_PredictREModel was split into it.

The other prediction tests hold every path to the reference within tolerances; a reordered sum or a reordered pair of checks can pass them.  tests/predict_paths.py lists
small cases (n = 300, 10 neighbours, 12 prediction points of which six lie within 0.01 of each other) through every model path, prediction type and refusal, and calls that
meet two refusals at once.  Every returned number is compared by its float64 bit pattern, every message as a string, with a recording made at that commit:
  tests/golden/predict_paths_mi355x.npz   the real library on an MI355X, three separate processes that agreed in every field
  tests/golden/predict_paths_mock.npz     the CPU restatement of the shim (tests/mock_shim), without the cases it does not restate (exact GP, inducing points);
                                          glibc and compiler of the recording host are stored in it ("@glibc", "@compiler")
The file is chosen by whether GPBOOST_AMD_LIB names the mock library.  A field that had not reproduced at the parent would carry "<key>@spread" in the file and be held to
four times that spread; there is none."""
import numpy as np
import pytest

from tests import predict_paths as pp

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gold(lib_built):
    import gpboost_amd
    assert pp.on_mock() or gpboost_amd.device_count() > 0, "no GPU visible: the -m gpu tests must run on the MI355X box"
    return dict(np.load(pp.fixture_path()))


def test_the_recording_covers_the_table(gold):
    recorded = {k.split("/")[0] for k in gold if not k.startswith("@")}
    assert recorded == set(pp.case_names())
    spread = [k for k in gold if k.endswith("@spread")]
    assert len(spread) <= 0.05 * len(gold)
    for name in pp.case_names():           # the twelve refusals every path shares (predict_paths.common_refusals) are messages in the record, not numbers
        if name.endswith("-refusals"):
            assert sum(k.startswith(name + "/") and k.endswith("/error") for k in gold) >= 12, name


@pytest.mark.parametrize("name", sorted(pp.CASES))
def test_same_bits_and_messages_as_the_recording(gold, name):
    if name not in pp.case_names():
        assert pp.on_mock() and name in pp.DEVICE_ONLY
        return
    got = pp.run(name)
    want = {k: v for k, v in gold.items() if k.startswith(name + "/") and not k.endswith("@spread")}
    assert set(got) == set(want)
    for key in sorted(want):
        g, w = got[key], want[key]
        print(key, g.shape, str(g) if g.dtype.kind == "U" else "")
        assert g.shape == w.shape and g.dtype.kind == w.dtype.kind, key
        if w.dtype.kind == "U":
            assert str(g) == str(w), key
        elif key + "@spread" in gold:
            assert np.all(np.abs(g - w) <= 4.0 * float(gold[key + "@spread"])), (key, np.abs(g - w).max(), float(gold[key + "@spread"]))
        else:
            assert np.array_equal(g.view(np.uint64), w.view(np.uint64)), (key, np.abs(g - w).max())
