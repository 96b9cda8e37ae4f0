"""The vector kernels of learner = lbfgs (difacto_amd/csrc/dfh_lbfgs.hip) against host restatements of the reference's
lbfgs::Inner / Add / Times and LBFGSUpdater (src/lbfgs/lbfgs_utils.h:62-98, lbfgs_updater.h:107-203), via the C ABI."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


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


def _dev(capi, ctx, a):
    return capi.DeviceBuffer.from_numpy(ctx, np.ascontiguousarray(a, np.float32))


def _inner_ref(a, b):
    """lbfgs::Inner: float products, double sum; and the sum of |products| the error is measured against"""
    p = (a * b).astype(np.float64)
    return p.sum(), np.abs(p).sum()


@pytest.mark.parametrize("n", [1, 1000, 1000003, 2 ** 26 + 5])
@pytest.mark.parametrize("m", [1, 5, 10, 16])
def test_inner_multi_matches_fp64_sums(capi, ctx, n, m):
    """CalcIncreB's shape: 3 left-hand vectors (two of them among the right-hand ones, read once) against 2m+1"""
    rng = np.random.default_rng(n + m)
    nd = min(2 * m + 1, 5)   # distinct buffers, cycled through the right-hand list (n = 2^26 + 5 stays in host memory)
    host = [(rng.standard_normal(n) * rng.choice([1e-3, 1.0, 40.0])).astype(np.float32) for _ in range(nd + 1)]
    bufs = [_dev(capi, ctx, h) for h in host]
    try:
        bi = [j % nd for j in range(2 * m + 1)]
        ai = [bi[m - 1], nd, bi[2 * m]]          # s_last-like alias, a vector of its own, g-like alias
        got = capi.vec_inner_multi(ctx, n, [bufs[i] for i in ai], [bufs[j] for j in bi])
        cache = {}
        for x, i in enumerate(ai):
            for y, j in enumerate(bi):
                key = (min(i, j), max(i, j))
                if key not in cache:
                    cache[key] = _inner_ref(host[i], host[j])
                want, mag = cache[key]
                assert abs(got[x, y] - want) <= 1e-10 * mag + 1e-300, (x, y, got[x, y], want)
        again = capi.vec_inner_multi(ctx, n, [bufs[i] for i in ai], [bufs[j] for j in bi])
        assert np.array_equal(got.view(np.uint64), again.view(np.uint64)), "not the same answer on a second run"
    finally:
        for b in bufs:
            b.close()


def _combine_ref(vecs, coef, clamp=5.0):
    """CalcDirection's lbfgs::Add chain in float32, in order, then the clamp (lbfgs_updater.h:117)"""
    p = np.zeros_like(vecs[0])
    for c, v in zip(np.asarray(coef, np.float32), vecs):
        if c == 0:
            continue
        p = p + v if c == 1 else p + c * v
    return np.where(p > clamp, np.float32(clamp), np.where(p < -clamp, np.float32(-clamp), p)).astype(np.float32)


@pytest.mark.parametrize("n", [1, 1000, 1000003])
@pytest.mark.parametrize("in_place", [False, True])
def test_combine_bit_identical_to_add_chain(capi, ctx, n, in_place):
    rng = np.random.default_rng(7 + n)
    m = 5
    vecs = [(rng.standard_normal(n) * 3).astype(np.float32) for _ in range(2 * m + 1)]   # values beyond +-5 included
    vecs[3][: max(1, n // 3)] *= 10
    coef = np.array([0.0, 1.0, -0.37, 2.5e-3, 1.0, 0.0, -1.0, 0.8125, 3.3, -1e-4, -1.0], np.float32)
    want = _combine_ref(vecs, coef)
    g = vecs[-1]
    bufs = [_dev(capi, ctx, v) for v in vecs]
    out = bufs[0] if in_place else capi.DeviceBuffer.from_numpy(ctx, np.full(n, np.nan, np.float32))
    try:
        dot = capi.vec_combine(ctx, n, bufs, coef, out, dot=bufs[-1])
        got = out.to_numpy(np.float32, n)
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), "direction differs from the float32 Add chain"
        ref, mag = _inner_ref(g, want)
        assert abs(dot - ref) <= 1e-10 * mag + 1e-300
        assert np.abs(got).max() <= 5
    finally:
        for b in bufs:
            b.close()
        if not in_place:
            out.close()


def test_combine_first_epoch_is_minus_g(capi, ctx):
    """epoch 0: dir = -grads, clamped (lbfgs_updater.h:113-117)"""
    rng = np.random.default_rng(3)
    g = (rng.standard_normal(4097) * 4).astype(np.float32)
    gb = _dev(capi, ctx, g)
    out = capi.DeviceBuffer.from_numpy(ctx, np.zeros(g.size, np.float32))
    try:
        capi.vec_combine(ctx, g.size, [gb], [-1.0], out, dot=gb)
        assert np.array_equal(out.to_numpy(np.float32, g.size), np.clip(-g, -5, 5))
    finally:
        gb.close()
        out.close()


@pytest.mark.parametrize("x", [0.0, 1.0, 0.3671875, -2.75])
@pytest.mark.parametrize("with_mask", [False, True])
def test_line_step(capi, ctx, x, with_mask):
    n = 1000003
    rng = np.random.default_rng(11)
    w = (rng.standard_normal(n) * 0.5).astype(np.float32)
    w[rng.random(n) < 0.2] = 0
    p = rng.standard_normal(n).astype(np.float32)
    isV = rng.random(n) < 0.6
    l2, V_l2 = np.float32(0.1), np.float32(0.01)
    mask = np.zeros((n + 31) // 32 + 1, np.uint32)
    idx = np.nonzero(isV)[0]
    np.bitwise_or.at(mask, idx >> 5, (np.uint32(1) << (idx & 31).astype(np.uint32)).astype(np.uint32))
    coef = np.where(isV, V_l2, l2).astype(np.float32) if with_mask else np.full(n, l2, np.float32)
    xf = np.float32(x)
    want = w if x == 0 else (w + p if x == 1 else w + xf * p)
    wb, pb, mb = _dev(capi, ctx, w), _dev(capi, ctx, p), capi.DeviceBuffer.from_numpy(ctx, mask)
    try:
        r, rp, nnz = capi.vec_line_step(ctx, n, wb, pb, x, vmask=mb if with_mask else None, l2=float(l2), V_l2=float(V_l2))
        got = wb.to_numpy(np.float32, n)
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), "w differs from lbfgs::Add"
        c64, w64 = coef.astype(np.float64), want.astype(np.float64)
        r_ref = (0.5 * c64 * w64 * w64).sum()
        assert abs(r - r_ref) <= 1e-12 * abs(r_ref) + 1e-300
        rp_terms = ((coef * want) * p).astype(np.float64)
        assert abs(rp - rp_terms.sum()) <= 1e-10 * np.abs(rp_terms).sum() + 1e-300
        assert nnz == np.count_nonzero(want)
    finally:
        for b in (wb, pb, mb):
            b.close()
