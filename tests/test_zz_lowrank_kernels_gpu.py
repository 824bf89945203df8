"""GPU (MI355X): the block operations of the low-rank preconditioners one by one -- pc_gram, pc_ltwx, pc_combine of gpboost_amd/csrc/pivchol_kernels.hip through
gpb_hip_lowrank_ops_check, which sizes and launches them as the model path does -- against the same operation in long double (tests/lowrank_ref.py) within the
componentwise bound derived there: |device - reference| <= 4 N u sum|terms|.  The model-path tests (test_zz_laplace_pivchol_gpu.py) reach these kernels only on the
shapes their cases happen to have; here: n around the row tiles (4 / 64 / 256 rows) and beyond 262144 (row slices longer than 256: pc_parts stops at 1024 slices), k
around the 4- and 16-column tiles and around 256 (the second pass of pc_ltwx_mfma_kernel over the columns of L), 1 .. 33 chunks of 4 columns (CT = 1, 2, 4 tiles per launch;
more than 16 chunks: one launch per group of 16 with moved pointers), the plain-column kernels (nc = 1), the five modes of pc_combine each also with out == X.
On the device every input lies between NaNs, the scratch starts as NaN, the last column of the last chunk of X is NaN and the result lies between sentinels."""
import functools

import numpy as np
import pytest

from tests import lowrank_ref as lr

pytestmark = pytest.mark.gpu

# (n, k, chunks, nc): every value of each axis at least once --
#   n: 1, 3, 63, 64, 65, 255, 256, 257, 1000, 4099, 262148;  k: 1, 3, 4, 5, 15, 16, 17, 50, 200, 255, 256, 257, 300;  chunks (nc = 4): 1, 4, 5, 8, 9, 13, 16, 17, 32, 33;
#   nc = 1 with 1 and 4 columns -- and the corners n = 1 & k = 1, k = 257 & 17 chunks, n = 65 & k = 17 & 5 chunks
SHAPES = [(1, 1, 1, 4), (1, 1, 1, 1), (3, 3, 4, 4), (3, 1, 17, 4), (63, 4, 5, 4), (64, 5, 8, 4), (64, 256, 1, 4), (65, 17, 5, 4), (65, 3, 1, 1), (255, 15, 9, 4),
          (256, 16, 13, 4), (257, 50, 16, 4), (257, 300, 4, 1), (1000, 257, 17, 4), (1000, 200, 32, 4), (1000, 300, 33, 4), (1000, 50, 1, 1), (4099, 255, 4, 4),
          (4099, 256, 9, 4), (4099, 17, 4, 1), (262145 + 3, 17, 5, 4)]
OPS = ["gram", "ltwx"] + ["combine%d%s" % (mode, ip) for mode in range(5) for ip in ("", "_in_place")]


@pytest.fixture(scope="module")
def shim(lib_built):
    import gpboost_amd
    assert gpboost_amd.device_count() > 0, "no GPU visible: the -m gpu tests must run on the MI355X box"
    from gpboost_amd import shim
    return shim


@functools.lru_cache(maxsize=2)
def _case(shape):
    assert lr.long_double_is_wider()
    n, k, ncol, nc = shape
    d = lr.make_inputs(n, k, ncol, nc, seed=1000 * ncol + 10 * k + nc + n % 7)
    return d, lr.combine_parts(d["L"], d["x2"])


@pytest.mark.parametrize("op", OPS)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "n%d_k%d_ch%d_nc%d" % s)
def test_block_operation_against_long_double(shim, shape, op):
    n, k, ncol, nc = shape
    d, parts = _case(shape)
    L, W, M, X, x2 = d["L"], d["W"], d["M"], d["X"], d["x2"]
    if op == "gram":
        dev, intact = shim.lowrank_ops_check("gram", L, W)
        ref, bound = lr.ref_gram(L, W)
    elif op == "ltwx":
        dev, intact = shim.lowrank_ops_check("ltwx", L, W, ncol, nc, M=M, X=X)
        ref, bound = lr.ref_ltwx(L, W, M, X)
    else:
        mode = int(op[7])
        dev, intact = shim.lowrank_ops_check("combine", L, W, ncol, nc, X=X, x2=x2, mode=mode, in_place=op.endswith("_in_place"))
        ref, bound = lr.ref_combine(L, W, X, x2, mode, parts)
    assert intact, "a store outside the result"
    worst = lr.check(dev, ref, bound, what="%s n=%d k=%d chunks=%d nc=%d" % (op, n, k, ncol, nc))
    print("%s n=%d k=%d chunks=%d nc=%d: worst |device - reference| / (N u sum|terms|) = %.3f" % (op, n, k, ncol, nc, worst))


def test_rank_beyond_the_limit_is_refused_by_the_entry(shim):
    import gpboost_amd
    with pytest.raises(gpboost_amd.GPBoostError, match="invalid argument"):
        shim.lowrank_ops_check("ltwx", np.ones((4, 2049)), np.ones(4), 1, 4, M=np.eye(2049), X=np.ones((1, 4, 4)))
