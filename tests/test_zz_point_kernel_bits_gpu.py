"""GPU (MI355X): vecchia_point_kernel returns, for every instance <MT, COV, D3, MODE, WT>, exactly the bits it returned at the commit recorded in
tests/golden/point_kernel_bits.npz (tests/point_kernel_bits.py describes the file, scripts/record_point_kernel_bits.py writes it).  Changes that move, merge or
delete instructions which compute no result -- address arithmetic, selects, moves, wait states -- are held to this, not to a tolerance.

The cases are those of tests/test_zz_vecchia_point_instances_gpu.py: a few dozen to a few hundred points, a partial last group, rows shorter than m, m < MT,
both record widths, weights; the shards [0, n) and [7, n - 9), each with the default grid (one trip per worker) and with two workers (several uneven trips)."""
import os

import numpy as np
import pytest

from tests import point_kernel_bits as B

pytestmark = pytest.mark.gpu
CASES = B.cases()
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", B.FIXTURE)


@pytest.fixture(scope="module")
def gpb(lib_built):
    import gpboost_amd
    assert gpboost_amd.device_count() > 0, "no GPU visible: the -m gpu tests must run on the MI355X box"
    return gpboost_amd


@pytest.fixture(scope="module")
def golden(gpb):
    """The fixture, after the guard: the kernel's exp table is exp2(j / 256) of the HOST's libm.  With another libm the table differs in the last bit of some
    entries and no comparison below means anything: that is a failure of the fixture, not of the kernel."""
    data = B.load(GOLDEN)
    tab = B.host_exp2_table()
    assert np.array_equal(tab, data["exp2_table"]), (
        "exp2(j / 256) of the libm this library links differs from the recorded table in %d of 256 entries: a different libm.  Re-record "
        "tests/golden/point_kernel_bits.npz with scripts/record_point_kernel_bits.py from the parent commit %s on this system."
        % (int(np.count_nonzero(tab != data["exp2_table"])), str(data["parent"])))
    return data


def _compare(got, golden, where=""):
    assert got, "no values collected"
    for key, val in got.items():
        assert key in golden, "the fixture has no entry %s" % key
        assert val.dtype == golden[key].dtype and np.array_equal(val, golden[key]), "%s differs from commit %s%s" % (key, str(golden["parent"]), where)


@pytest.mark.parametrize("case", CASES, ids=[c.id for c in CASES])
def test_every_bit_as_recorded(gpb, golden, case):
    _compare(B.collect(case), golden)
