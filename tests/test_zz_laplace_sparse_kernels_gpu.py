"""GPU (MI355X): the sparse machinery of the Vecchia-Laplace path (laplace_kernels.hip) per element, through gpb_hip_vecchia_laplace_ops_check, which calls the launchers
the model path calls (lap_B, lap_Bt, lap_apply, lap_vadu, lap_fwd_solve, lap_mul) on the caller's factor -- against the long-double operations and the a-priori bounds of
tests/laplace_sparse_ref.py (derived there before any device run; tests/test_laplace_sparse_ref.py checks the model on the CPU).

The graphs (laplace_sparse_ref.GRAPHS) are built so that the host schedule takes the branches no model-sized test reaches: rows split over several slots, padding
slots, slots of more than 64 entries, wide levels launched on their own, runs of narrow levels outside a dense block, solves with and without overflow entries, dense
blocks in one piece and next to sparse levels.  For every (graph, operation, nc, ncol):
  * `info` equals the restated schedule field by field (a graph that does not reach its branch fails tests/test_laplace_sparse_ref.py);
  * every element lies inside its bound, for each solver form the operation has: 0 = one launch per level (lap_sptrsv_kernel), 1 = barrier-free single vectors
    (lap_sptrsv_sf_kernel, nc = 1), 4 = barrier-free probe block (lap_sptrsv_sfw_kernel, nc = 4);
  * the forms return the same bits, t of lap_vadu included;
  * the bits of a column do not depend on the columns solved with it, nor on what the output and the scratch held before (zeros, NaN, +Inf, the pending-row pattern);
  * the error word of the solves is 0.  A give-up fails the test and stops every later launch of that solver form (BROKEN), so that a defect costs one bounded spin.
The largest difference from the long-double SOLUTION is printed, not asserted (it carries the condition of B)."""
import json
import os

import numpy as np
import pytest

from tests import laplace_sparse_ref as R

pytestmark = pytest.mark.gpu
LD = R.LD
PREFILLS = ("nan", "inf", "sentinel")
CASES = [(g, op, nc, ncol) for g in R.GRAPHS for op in R.OPS for nc, ncol in R.SHAPES]
WORST = {}          # "form <f> / <class>" -> (largest error / bound, graph, row, column)
BROKEN = {}         # solver form -> the test in which one of its solves gave up
_STATES = {}


@pytest.fixture(scope="module")
def gpb(lib_built):
    import gpboost_amd
    assert gpboost_amd.device_count() > 0, "no GPU visible: the -m gpu tests must run on the MI355X box"
    return gpboost_amd


def _state(name):
    if name not in _STATES:
        from gpboost_amd import shim
        g = R.graph(name)
        st = shim.VecchiaState(g.coords, g.m)
        assert st.m == g.m
        st.set_neighbors(g.nn)
        _STATES[name] = st
    return _STATES[name], R.graph(name)


def _note(form, cls, q, name):
    r, c = np.unravel_index(int(np.argmax(q)), q.shape)
    key = "form %d / %s" % (form, cls)
    if float(q[r, c]) >= WORST.get(key, (-1.0,))[0]:
        WORST[key] = (float(q[r, c]), name, int(r), int(c))


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


def _run(st, g, op, X, nc, form, prefill="zeros"):
    if form in BROKEN:
        pytest.fail("solver form %d gave up in %s: not launched again" % (form, BROKEN[form]))
    out, out2, info = st.laplace_ops_check(op, g.A, X, nc=nc, form=form, prefill=prefill, D=g.D, W=g.W, scale=g.scale, A2=g.A2)
    if info["err"] != 0:
        BROKEN[form] = "%s %s nc=%d ncol=%d prefill=%s" % (g.name, op, nc, X.shape[1] // nc, prefill)
        pytest.fail("a barrier-free solve gave up (error word %d): %s" % (info["err"], BROKEN[form]))
    return out, out2, info


def _check(g, op, X, nc, form, out, out2):
    """every element against its bound; -> the largest ratio"""
    fw, bw = g.sched(False), g.sched(True)
    worst = 0.0

    def product(cls, s, A, Xin, mode, got, **kw):
        val, bound = R.product_ref(s, A, Xin, mode, **kw)
        q = R.ratio_of(got.astype(LD) - val, bound)
        _note(form, cls, q, g.name)
        return float(q.max())

    def solve(s, num, den, xh):
        q, dense = R.solve_check(s, g.A, num, den, xh, nc)
        for cls, mask in (("solve sparse rows", ~dense), ("solve dense rows", dense)):
            if mask.any():
                _note(form, cls, q[mask], g.name)
        exact = R.solve_exact(s, g.A, num, den)
        print("%s %s form %d: largest |x - x_ld| / max |x_ld| = %.3g" % (g.name, "bwd" if s.backward else "fwd", form,
                                                                        float(np.max(np.abs(xh.astype(LD) - exact)) / np.max(np.abs(exact)))))
        return float(q.max())

    if op == "B":
        worst = product("B", fw, g.A, X, 0, out)
    elif op == "Bt":
        worst = product("Bt", bw, g.A, X, 2, out)
    elif op == "apply":
        worst = max(product("apply first half", fw, g.A, X, 1, out2, D=g.D), product("apply second half", bw, g.A, out2, 2, out, W=g.W, H=X))
    elif op == "vadu":
        worst = max(solve(bw, X, None, out2), solve(fw, out2, g.scale, out))
    elif op == "fwd_solve":
        worst = solve(fw, X, g.scale, out)
    elif op == "mul_fwd":
        worst = product("mul_fwd", fw, g.A2, X, 3, out)
    else:
        worst = product("mul_bwd", bw, g.A2, X, 3, out)
    return worst


def _forms(op, nc):
    return (0, 1 if nc == 1 else 4) if op in R.SOLVE_OPS else (0,)


def _all(st, g, op, X, nc):
    """all forms and prefills of one (operation, operand): bounds, same bits.  -> the result of form 0"""
    base = None
    for form in _forms(op, nc):
        out, out2, info = _run(st, g, op, X, nc, form)
        for solve, s in (("fwd", g.sched(False)), ("bwd", g.sched(True))):
            assert info[solve] == s.info, (solve, info[solve], s.info)
        assert np.all(np.isfinite(out)) and (out2 is None or np.all(np.isfinite(out2)))
        worst = _check(g, op, X, nc, form, out, out2)
        assert worst <= 1.0, (g.name, op, nc, form, worst)
        if base is None:
            base = (out, out2)
        else:
            assert np.array_equal(_bits(out), _bits(base[0])), "form %d and form 0 differ" % form
            assert out2 is None or np.array_equal(_bits(out2), _bits(base[1])), "t of form %d and form 0 differ" % form
        for prefill in PREFILLS:
            o, o2, _ = _run(st, g, op, X, nc, form, prefill)
            assert np.array_equal(_bits(o), _bits(out)), "form %d: the result depends on what the output held before (%s)" % (form, prefill)
            assert o2 is None or np.array_equal(_bits(o2), _bits(out2)), "form %d: the intermediate depends on what it held before (%s)" % (form, prefill)
    return base


@pytest.mark.parametrize("name,op,nc,ncol", CASES, ids=["%s-%s-nc%d-ncol%d" % c for c in CASES])
def test_per_element(gpb, name, op, nc, ncol):
    st, g = _state(name)
    X = g.operand(nc * ncol, seed=ncol)
    base = _all(st, g, op, X, nc)
    if ncol > 1:        # a column's bits do not depend on the chunks solved with it: the first and the last chunk alone
        for c0 in (0, (ncol - 1) * nc):
            for form in _forms(op, nc):
                o, o2, _ = _run(st, g, op, X[:, c0:c0 + nc], nc, form)
                assert np.array_equal(_bits(o), _bits(base[0][:, c0:c0 + nc])), (form, c0)
                assert o2 is None or np.array_equal(_bits(o2), _bits(base[1][:, c0:c0 + nc])), (form, c0)


@pytest.mark.parametrize("op", R.SOLVE_OPS)
def test_more_columns_than_resident_workgroups(gpb, op):
    """nc = 1 with resident + 3 columns: the barrier-free launcher for single vectors then takes the columns in two passes"""
    st, g = _state("layers-m126")
    _, _, info = _run(st, g, "B", g.operand(1), 1, 0)
    resident = info["resident"][0]
    assert 1 <= resident <= 8192, resident
    X = g.operand(resident + 3, seed=11)
    base = _all(st, g, op, X, 1)
    o, _, _ = _run(st, g, op, X[:, -1:], 1, 1)
    assert np.array_equal(_bits(o), _bits(base[0][:, -1:]))


def test_zz_report_worst_ratios(gpb):
    """Not a check: the largest error / bound per kernel form and class seen by the tests above, written to the file named by
    GPB_LAPLACE_SPARSE_RATIOS_OUT if that is set."""
    txt = json.dumps({k: [round(v[0], 4)] + list(v[1:]) for k, v in sorted(WORST.items())}, indent=1)
    print("sparse Vecchia-Laplace kernels, largest error / bound per form and class [ratio, graph, row, column]:\n" + txt)
    out = os.environ.get("GPB_LAPLACE_SPARSE_RATIOS_OUT")
    if out:
        with open(out, "w") as f:
            f.write(txt + "\n")
    for st in _STATES.values():
        st.close()
    _STATES.clear()
