"""The dfh_lbfgs object against a float64 numpy restatement of FMLoss + LBFGSUpdater on the reference's test data, on a model
with mixed lens (V_threshold > 0: some keys carry V, some do not): the gradient through gather / forward / backward /
scatter, PrepareCalcDirection folded into the product pass (g = g_new + grad r, y = g - g_old, s_last *= alpha) and gamma."""
import os

import numpy as np
import pytest

import bcd_ref as R
from lbfgs_ref import Model

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DATA = os.path.join(ROOT, "tests", "golden", "rcv1_100.libsvm")
K, VTH, L2, VL2 = 3, 2, 0.1, 0.01


@pytest.fixture(scope="module")
def capi():
    from difacto_amd import capi as m
    m.lib()
    return m


@pytest.fixture(scope="module")
def ctx(capi):
    c = capi.Context(0)
    yield c
    c.close()


def _rcv1():
    return R.read_libsvm(DATA)


def _model(data):
    """the float64 reference of the one-chunk model these tests drive; nothing of it comes from the device"""
    return Model([data], V_dim=K, V_threshold=VTH, l2=L2, V_l2=VL2)


def _obj(capi, ctx, data):
    obj = capi.Lbfgs(ctx, K, 5)
    off, idx, val, lab = data
    obj.add_chunk(off, idx, val, lab)
    obj.init_model(tail_feature_filter=0, V_threshold=VTH, V_init_scale=0.5, l2=L2, V_l2=VL2)
    return obj


def test_mixed_lens_gradient_and_prepared_history(capi, ctx):
    data = _rcv1()
    obj = _obj(capi, ctx, data)
    try:
        M = _model(data)
        assert 0 < (M.lens > 1).sum() < len(M.lens), "the model must mix keys with and without V"
        m = obj.get_model()
        assert np.array_equal(m["keys"], M.keys) and np.array_equal(m["lens"], M.lens) and np.array_equal(m["cnt"], M.cnt)
        assert np.array_equal(M.lens > 1, m["cnt"] > VTH)
        w0 = m["w"]
        loss0, gl0 = M.loss_grad(w0)
        got_loss, _ = obj.calc_grad()
        assert abs(got_loss - loss0) <= 1e-5 * abs(loss0)
        r0, rg0 = M.reg(w0)
        g0 = gl0 + rg0
        assert obj.prepare_direction() is None
        p = np.clip(-g0, -5, 5)
        pg = obj.calc_direction(None)
        assert abs(pg - g0 @ p) <= 1e-4 * np.abs(g0 * p).sum()
        alpha = 0.25
        w1 = w0 + alpha * p
        f, pg1, _ = obj.line_search(alpha)
        loss1, gl1 = M.loss_grad(w1)
        r1, rg1 = M.reg(w1)
        assert abs(f - (loss1 + r1)) <= 1e-5 * abs(loss1 + r1)
        assert abs(pg1 - (gl1 + rg1) @ p) <= 1e-4 * np.abs((gl1 + rg1) * p).sum()
        assert np.allclose(obj.get_model()["w"], w1, rtol=1e-6, atol=1e-7)
        # PrepareCalcDirection: g = g_new + grad r, y = g - g_old, s_last = alpha p; CalcIncreB with one pair
        incr = obj.prepare_direction()
        g1 = gl1 + rg1
        s, yv = alpha * p, g1 - g0
        want = [s @ s, s @ yv, yv @ s, yv @ yv, g1 @ s, g1 @ yv, g1 @ g1]
        mags = [np.abs(a * b).sum() for a, b in ((s, s), (s, yv), (yv, s), (yv, yv), (g1, s), (g1, yv), (g1, g1))]
        assert incr is not None and len(incr) == 7
        for got, wv, mg in zip(incr, want, mags):
            assert abs(got - wv) <= 1e-4 * mg, (incr, want)
    finally:
        obj.close()


def test_gamma(capi, ctx):
    """CalcGrad's g = sign(g) |g|^gamma (lbfgs_learner.cc:300-302) before the regulariser is added"""
    data = _rcv1()
    obj = _obj(capi, ctx, data)
    try:
        M = _model(data)
        w0 = obj.get_model()["w"]
        _, gl = M.loss_grad(w0)
        gg = np.where(gl > 0, 1.0, -1.0) * np.abs(gl) ** 0.5
        g0 = gg + M.reg(w0)[1]
        obj.calc_grad(gamma=0.5)
        assert obj.prepare_direction() is None
        pg = obj.calc_direction(None)
        p = np.clip(-g0, -5, 5)
        assert abs(pg - g0 @ p) <= 1e-4 * np.abs(g0 * p).sum()
    finally:
        obj.close()
