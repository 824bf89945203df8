"""The neighbour table of every prediction-time search mode, read straight off the device and compared entry by entry with the oracle's
restatement of find_nearest_neighbors_Vecchia_fast with its start_at / end_search_at arguments (orc.neighbors_range).  The predicted
values of the other test files depend on these tables only through sums; here the tables themselves are pinned, for every search mode whose
table an entry point returns (predict_obs_only returns none: its search, start_at = n_obs with the observed candidates, is covered by the rows
>= n_obs of the every-row search, which are the same rows):

  mode                      start_at, end_search_at     device side
  obs_first_cond_obs_only   n_obs,  n_obs - 1           predict_joint_factor(layout 0, cond_all 0), rows >= n_obs
  obs_first_cond_all        n_obs,  -1                  predict_cond_all (the appended rows)
  all_rows_cond_obs_only    0,      n_obs - 1           predict_joint_factor(layout 0, cond_all 0), every row
  pred_first                0,      -1 on [pred; obs]   predict_joint_factor(layout 1, cond_all 1), every row

Shapes (n_obs, n_pred, d, m): d = 5 takes the (d + 1)-wide records of d > 3; m = 90 > 85 raises the search's dynamic LDS limit; (12, 5, 1, 30)
has m capped by the number of candidates (12 observed points / 16 preceding points).  Three prediction points sit exactly on observed
points in every case: the search must report the zero distances."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SHAPES = [(300, 40, 2, 10), (200, 30, 5, 10), (150, 20, 3, 90), (12, 5, 1, 30)]
MODES = ["obs_first_cond_obs_only", "obs_first_cond_all", "all_rows_cond_obs_only", "pred_first"]


@pytest.fixture(scope="module")
def gpb(lib_built):
    import gpboost_amd
    assert gpboost_amd.device_count() > 0, "no GPU visible: the -m gpu tests must run on the MI355X box"
    return gpboost_amd


def data(n_obs, n_pred, d, m):
    rng = np.random.default_rng(1000 * n_obs + d)
    co = rng.uniform(size=(n_obs, d)); cp = rng.uniform(size=(n_pred, d))
    cp[[0, n_pred // 2, n_pred - 1]] = co[[1, n_obs // 2, n_obs - 1]]
    return co, cp, rng.standard_normal(n_obs)


@pytest.fixture(scope="module")
def states(gpb):
    """One handle per shape, shared by its four modes and freed with the module."""
    from gpboost_amd import shim
    sts = {}
    for shape in SHAPES:
        co, cp, y = data(*shape)
        sts[shape] = shim.VecchiaState(co, shape[3]); sts[shape].set_y(y)
    yield sts
    for st in sts.values():
        st.close()


def device_table(st, shape, mode):
    """-> (rows of the device's table, has_duplicates); exponential covariance, Gaussian likelihood (the factor is not looked at)."""
    n_obs, n_pred, d, m = shape
    cp = data(*shape)[1]
    if mode == "obs_first_cond_all":
        nn, _, _, dup = st.predict_cond_all(cp, m, 0, 1.0, 5.0)
        return nn, dup
    pred_first = mode == "pred_first"
    nn, _, _, _, dup = st.predict_joint_factor(cp, m, pred_first, pred_first, True, 0, 1.0, 5.0)
    return (nn[n_obs:] if mode == "obs_first_cond_obs_only" else nn), dup


def oracle_table(orc, shape, mode):
    n_obs, n_pred, d, m = shape
    co, cp, _ = data(*shape)
    if mode == "pred_first":
        ref = orc.neighbors_range(np.vstack([cp, co]), m, 0, -1)
        assert np.array_equal(ref, orc.neighbors(np.vstack([cp, co]), min(m, n_obs + n_pred - 1)))      # the table orc.predict_pred_first builds
        return ref
    joint = np.vstack([co, cp])
    if mode == "all_rows_cond_obs_only":
        return orc.neighbors_range(joint, m, 0, n_obs - 1)
    return orc.neighbors_range(joint, m, n_obs, n_obs - 1 if mode == "obs_first_cond_obs_only" else -1)[n_obs:]


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "n%d_p%d_d%d_m%d" % s)
def test_prediction_search_table_equals_oracle(states, orc, shape, mode):
    nn, dup = device_table(states[shape], shape, mode)
    ref = oracle_table(orc, shape, mode)
    assert nn.shape == ref.shape, (nn.shape, ref.shape)
    assert np.array_equal(nn, ref), "rows that differ: %s" % np.flatnonzero((nn != ref).any(axis=1))[:10]
    assert dup is True
