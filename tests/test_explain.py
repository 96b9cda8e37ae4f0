"""Each row's top-k FM interaction pairs (csrc/dfh_explain.hip) through capi.Explain, against numpy float64: per row, over
the positions whose key has V, C = (x x^T) o (V V^T), upper triangle.

A returned c may differ from C[i, j] by at most gamma_m |x_i x_j| sum_d |V_id V_jd|, m = V_dim + 3, gamma_m = m u / (1 - m u),
u = 2^-24: an fp32 dot product in any order plus the two scalings.  inter: gamma_{P + m} over the sum of those magnitudes, P the
row's pairs.  Exact inputs (small integers): lists, scores and inter EQUAL the reference's under the tie rule (key descending,
then (i, j) ascending).  Row lengths sit on the panel of 32 and the 64-lane staging step."""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
U64, F64 = np.uint64, np.float64
LENS = [0, 1, 2, 31, 32, 33, 63, 64, 65, 100]
ERR_ARG, ERR_STATE = 1, 4   # DFH_ERR_ARG, DFH_ERR_STATE of include/difacto_hip.h


def rev(x):   # ReverseBytes (include/difacto/base.h): the nibbles of a 64-bit word in reverse order
    x = np.asarray(x, U64).byteswap()
    return ((x & U64(0x0F0F0F0F0F0F0F0F)) << U64(4)) | ((x & U64(0xF0F0F0F0F0F0F0F0)) >> U64(4))


@pytest.fixture(scope="module")
def dev():
    from difacto_amd import build, capi
    build.build_hip()
    ctx = capi.Context(0)
    yield capi, ctx
    ctx.close()


def close(*objs):
    for o in objs:
        o.close()


def model(dev, k, seed, integers=False, m=150, inf_at=None):
    """m keys, about a quarter of them without V (inf_at: one coordinate of the key with that number among those with V is
    inf) -> table, feature ids, has_V, V"""
    capi, ctx = dev
    rng = np.random.default_rng(seed)
    has = (rng.random(m) >= 0.25).astype(np.int32)
    V = (rng.integers(-2, 3, (m, k)) if integers else rng.normal(size=(m, k))).astype(np.float32)
    if inf_at is not None:
        V[np.flatnonzero(has)[inf_at], 2] = np.inf
    ids = np.arange(1, m + 1, dtype=U64) * U64(7919)
    scal = np.zeros((m, 4), np.float32)
    scal[:, 1] = 1.0
    tb = capi.Table(ctx, 1024, V_dim=k, init_mode=capi.INIT_HASH, V_threshold=0, l1=0.0, seed=1)
    tb.import_(rev(ids), scal, has, np.concatenate([V, np.zeros_like(V)], 1))
    return tb, ids, has, V


def rows_of(rng, m, lens, integers=False):
    """-> offset, key number per position, x per position; row 3 repeats a key"""
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    idx = rng.integers(0, m, off[-1])
    if len(lens) > 3 and lens[3] > 6:
        idx[off[3] + 6] = idx[off[3] + 1]
    x = (rng.integers(1, 3, off[-1]) if integers else rng.normal(size=off[-1])).astype(np.float32)
    return off, idx, x


def step(tb, b, ids, off, idx, x, n=1):
    """load, localize, look up and (n = 1) take the prediction step"""
    b.load_host(off, ids[idx], x, np.ones(len(off) - 1, np.float32))
    b.localize()
    b.lookup(tb)
    for _ in range(n):
        b.sgd_step(tb, is_train=False)


def pairs64(has, V, idx, x):
    """a row's finite pairs in (i, j) order: positions i, j, float64 c, magnitude sum; and the count of the others"""
    pos = np.flatnonzero(has[idx])
    Vr, xr = V[idx[pos]].astype(F64), x[pos].astype(F64)
    with np.errstate(all="ignore"):
        C, B = np.outer(xr, xr) * (Vr @ Vr.T), np.outer(np.abs(xr), np.abs(xr)) * (np.abs(Vr) @ np.abs(Vr).T)
    i, j = np.triu_indices(pos.size, 1)
    i, j, bad = i[np.isfinite(C[i, j])], j[np.isfinite(C[i, j])], int((~np.isfinite(C[i, j])).sum())
    return pos[i], pos[j], C[i, j], B[i, j], bad


def check(got, r0, off, idx, x, ids, has, V, K, by_pos):
    """the rows of one minibatch, got's rows r0 ..; -> the pairs left out as non-finite"""
    m = V.shape[1] + 3
    g = lambda n: n * 2.0 ** -24 / (1 - n * 2.0 ** -24)
    left_out = 0
    for r in range(len(off) - 1):
        ri, rx = idx[off[r]:off[r + 1]], x[off[r]:off[r + 1]]
        pi, pj, c64, mag, bad = pairs64(has, V, ri, rx)
        left_out, n, q = left_out + bad, int(got["n"][r0 + r]), r0 + r
        assert n == min(K, c64.size), (r, n)
        assert not got["c"][q, n:].any() and not got["ids_i"][q, n:].any()
        at = {(a, b): t for t, (a, b) in enumerate(zip(pi, pj))}
        t = np.array([at[(a, b)] for a, b in zip(got["pos_i"][q, :n], got["pos_j"][q, :n])], np.int64)   # KeyError: no pair i < j with V
        c = got["c"][q, :n].astype(F64)
        assert np.unique(t).size == n
        assert (np.abs(c - c64[t]) <= g(m) * mag[t]).all(), (r, np.abs(c - c64[t]).max())
        keys, key64 = (c, c64) if by_pos else (np.abs(c), np.abs(c64))
        assert (np.diff(keys) <= 0).all(), "the list is sorted by the returned keys"
        rest = np.setdiff1d(np.arange(c64.size), t)
        if rest.size:
            assert (key64[rest] <= keys[-1] + g(m) * mag[rest]).all(), (r, (key64[rest] - keys[-1] - g(m) * mag[rest]).max())
        assert abs(float(got["inter"][q]) - c64.sum()) <= g(c64.size + m) * mag.sum(), (r, got["inter"][q], c64.sum())
        assert np.array_equal(got["ids_i"][q, :n], ids[ri[pi[t]]]) and np.array_equal(got["ids_j"][q, :n], ids[ri[pj[t]]])
    return left_out


@pytest.mark.parametrize("K,by_pos", [(1, 0), (10, 1), (32, 0)])
@pytest.mark.parametrize("k", [1, 5, 8, 64, 100])
def test_scores_and_selection(dev, k, K, by_pos):
    capi, ctx = dev
    tb, ids, has, V = model(dev, k, 100 * k + K)
    b, e = capi.Batch(ctx, len(LENS), sum(LENS)), capi.Explain(ctx, K, by_pos)
    off, idx, x = rows_of(np.random.default_rng(k + K), len(ids), LENS)
    assert np.unique(idx[off[3]:off[4]]).size < LENS[3] and 0.1 < 1 - has[idx].mean() < 0.4
    for xs in (x, None):   # with a value array; without: x = 1
        step(tb, b, ids, off, idx, xs)
        e.reset()
        e.append_batch(b, tb)
        got = e.read()
        assert e.count() == len(LENS) and got["nonfinite"] == 0 and check(got, 0, off, idx, x if xs is not None else np.ones_like(x), ids, has, V, K, by_pos) == 0
    close(e, b, tb)


@pytest.mark.parametrize("by_pos", [0, 1])
def test_exact_ties(dev, by_pos):
    """V in [-2, 2], x in {1, 2}, V_dim 8: |c| <= 128 and every partial sum is an integer below 2^24"""
    capi, ctx = dev
    K, lens = 10, list(range(3, 71, 2))
    tb, ids, has, V = model(dev, 8, 5, integers=True)
    b, e = capi.Batch(ctx, len(lens), sum(lens)), capi.Explain(ctx, K, by_pos)
    off, idx, x = rows_of(np.random.default_rng(6), len(ids), lens, integers=True)
    step(tb, b, ids, off, idx, x)
    e.append_batch(b, tb)
    got = e.read()
    ties = 0
    for r in range(len(lens)):
        pi, pj, c64, _, _ = pairs64(has, V, idx[off[r]:off[r + 1]], x[off[r]:off[r + 1]])
        key = c64 if by_pos else np.abs(c64)
        order = np.lexsort((pj, pi, -key))
        top, ties = order[:K], ties + int(order.size > K and key[order[K - 1]] == key[order[K]])
        assert got["n"][r] == top.size and np.array_equal(got["pos_i"][r, :top.size], pi[top]) and np.array_equal(got["pos_j"][r, :top.size], pj[top]), r
        assert np.array_equal(got["c"][r, :top.size], c64[top].astype(np.float32)) and got["inter"][r] == np.float32(c64.sum())
    assert ties > 10, "equal keys across the K boundary"
    close(e, b, tb)


def test_several_minibatches_in_append_order(dev):
    """three appends over two batch objects in rotation, the pipeline on, the arrays growing from 16 rows; again after a reset"""
    capi, _ = dev
    ctx = capi.Context(0)
    ctx.set_pipeline(True)
    K, lens = 10, [40, 3, 70, 0, 33, 64, 1, 39, 39, 39, 12]
    tb, ids, has, V = model((capi, ctx), 8, 9)
    bs = [capi.Batch(ctx, len(lens), sum(lens)) for _ in range(2)]
    e = capi.Explain(ctx, K, 0, capacity_hint=16)
    mbs = [rows_of(np.random.default_rng(20 + t), len(ids), lens) for t in range(3)]
    for order in ((0, 1, 2), (2, 0, 1)):
        e.reset()
        step(tb, bs[0], ids, *mbs[order[0]])
        for t in range(3):
            if t + 1 < 3:   # the next minibatch is loaded while this one is stepped and explained
                step(tb, bs[(t + 1) % 2], ids, *mbs[order[t + 1]], n=0)
            if t:
                bs[t % 2].sgd_step(tb, is_train=False)
            e.append_batch(bs[t % 2], tb)
        got = e.read()
        assert e.count() == 3 * len(lens)
        for t in range(3):
            assert check(got, t * len(lens), *mbs[order[t]], ids, has, V, K, 0) == 0
    close(e, *bs, tb, ctx)


def test_non_finite_pairs_are_left_out_and_counted(dev):
    (capi, ctx), K = dev, 10
    tb, ids, has, V = model(dev, 8, 11, inf_at=7)
    bad = int(np.flatnonzero(has)[7])
    b, e = capi.Batch(ctx, len(LENS), sum(LENS)), capi.Explain(ctx, K, 0)
    off, idx, x = rows_of(np.random.default_rng(12), len(ids), LENS)
    for r in (4, 5, 8, 9):   # several rows use the key, row 9 twice
        idx[off[r] + 2] = bad
    idx[off[9] + 50] = bad
    step(tb, b, ids, off, idx, x)
    e.append_batch(b, tb)
    got = e.read()
    want = check(got, 0, off, idx, x, ids, has, V, K, 0)   # (the reference leaves the non-finite pairs out too)
    assert want > 4 * 20 and got["nonfinite"] == want
    assert not (got["ids_i"] == ids[bad]).any() and not (got["ids_j"] == ids[bad]).any() and np.isfinite(got["inter"]).all()
    close(e, b, tb)


def test_arguments_are_refused(dev):
    capi, ctx = dev
    L, C = capi.lib(), ctypes
    h = C.c_void_p()
    for topk, by, word in ((0, 0, "topk must be in [1, 32]"), (33, 0, "topk must be in [1, 32]"), (3, 2, "by must be")):
        assert L.dfh_explain_create(ctx.h, topk, by, 0, C.byref(h)) == ERR_ARG and word in L.dfh_last_error().decode()
    assert L.dfh_explain_create(None, 3, 0, 0, C.byref(h)) == ERR_ARG and L.dfh_explain_create(ctx.h, 3, 0, 0, None) == ERR_ARG
    tb, ids, has, V = model(dev, 8, 13)
    b, e = capi.Batch(ctx, 4, 200), capi.Explain(ctx, 3, 0)
    off, idx, x = rows_of(np.random.default_rng(14), len(ids), [5, 40, 0, 9])
    assert L.dfh_explain_append_batch(e.h, None, tb.h) == ERR_ARG and L.dfh_explain_append_batch(e.h, b.h, None) == ERR_ARG
    assert L.dfh_explain_read(e.h, None, None, None, None, None, None) == ERR_ARG and "NULL argument" in L.dfh_last_error().decode()
    step(tb, b, ids, off, idx, x, n=0)
    assert L.dfh_explain_append_batch(e.h, b.h, tb.h) == ERR_STATE and "dfh_sgd_step" in L.dfh_last_error().decode()   # not stepped
    b.sgd_step(tb, is_train=False)
    b.localize()   # a new view of the minibatch: the step's row words are gone
    assert L.dfh_explain_append_batch(e.h, b.h, tb.h) == ERR_STATE and e.count() == 0
    b.lookup(tb)
    b.sgd_step(tb, is_train=False)
    e.append_batch(b, tb)   # still usable
    assert check(e.read(), 0, off, idx, x, ids, has, V, 3, 0) == 0
    close(e, b, tb)
