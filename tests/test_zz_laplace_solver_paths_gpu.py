"""GPU (MI355X): the host orchestration of the Vecchia-Laplace path (gpboost_amd/csrc/gpb_laplace.inc: the workspace map LapWork, the three solver forms of LapSolver, the one
conjugate-gradient driver lap_cg) returns the SAME BITS and the SAME ITERATION COUNTS as the commit before the seven hand-written CG loops became that driver.

The other Laplace tests hold every form to the reference and the oracle within tolerances, at generous iteration caps; a change of loop control can pass them and still change
which exit a loop takes.  tests/laplace_solver_paths.py lists small cases (n = 192, m = 10, six probe vectors = two chunks with two padding columns) that take every exit:
converged, cap reached (3 CG iterations, 4 Lanczos steps; cold and warm start), the one-step likelihood, the three full-scale Vecchia forms, gradients, and block solves of the
predictive variances with a partial last block.  Every returned number -- out9[0..5], the mode, gradients and their parts, predictive means / variances / covariances, every
iteration count -- is compared with tests/golden/laplace_solver_paths_mi355x.npz, recorded at that commit on an MI355X by laplace_solver_paths.record in five separate
processes.  The dot products of these kernels are summed in a fixed order without atomics (laplace_kernels.hip, pivchol_kernels.hip), and the five recordings agree bit for bit
in every field: the comparison is exact (np.array_equal).  A field that had not reproduced would carry "<key>@spread" in the file and be held to twice that spread."""
import os

import numpy as np
import pytest

from tests import laplace_solver_paths as lsp

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(__file__), "golden", "laplace_solver_paths_mi355x.npz")


@pytest.fixture(scope="module")
def gold(lib_built):
    import gpboost_amd
    assert gpboost_amd.device_count() > 0, "no GPU visible: the -m gpu tests must run on the MI355X box"
    return dict(np.load(GOLD))


def test_the_recording_covers_the_table(gold):
    recorded = {k.split("/")[0] for k in gold}
    assert recorded == set(lsp.CASES)
    # the caps are reached where the table means them to be: the Lanczos process of every capped run ends at its 4 steps, that of every other run before min(1000, n)
    for name in lsp.CASES:
        if name.startswith(("cap-", "vif-cap-")):
            for tag in ("cold_", "warm_"):
                assert int(gold["%s/%slanczos_it" % (name, tag)]) == lsp.CAP["cg_max_num_it_tridiag"]
        elif name.startswith("conv-"):
            assert int(gold[name + "/lanczos_it"]) < lsp.N


@pytest.mark.parametrize("name", sorted(lsp.CASES))
def test_same_bits_and_iteration_counts_as_the_recording(gold, name):
    got = lsp.run(name)
    want = {k: v for k, v in gold.items() if k.startswith(name + "/") and not k.endswith("@spread")}
    assert set(got) == set(want)
    for key in sorted(want):
        g, w = got[key], want[key]
        assert g.shape == w.shape and g.dtype == w.dtype, key
        if key.endswith("_it"):
            assert int(g) == int(w), (key, int(g), int(w))
        elif key + "@spread" in gold:
            assert np.all(np.abs(g - w) <= 2.0 * float(gold[key + "@spread"])), (key, np.abs(g - w).max(), float(gold[key + "@spread"]))
        else:
            assert np.array_equal(g, w), (key, np.abs(g - w).max() if g.shape else (float(g), float(w)))


def test_block_solve_that_cannot_converge_is_refused(gold):
    from gpboost_amd import shim
    rc, msg = lsp.quad_forms_refusal(shim)
    assert rc != 0
    assert msg == "the conjugate gradient algorithm of the predictive variances has not converged after 1 iterations (residual norm above 1e-12)"
