"""Each query row's top-k catalogue items (csrc/dfh_recommend.hip) through capi.Recommend, against numpy float64 evaluating the
definition: S_r = sum_j x_j V_j over the row's positions whose key has V, b_r = sum_j x_j w_j + 1/2 sum_d (S_r[d]^2 -
sum_j (x_j V_j[d])^2), s(q, i) = b_i + <S_q, S_i>, logit = a_q + s; s descending, equal s by ascending item number.

Exact cases: w, V and x are small multiples of 2^-3 (so of 2^-6), rows hold at most 12 ids: every product is a multiple of 2^-9
below 2^14 and every fp32 sum is exact, so items, order and the logits' bits must equal the reference's.  General floats: a
logit may differ from float64 by (nnz_q + nnz_i + V_dim + 4) 2^-24 T, T = the float64 sum of the absolute values of all terms of
that logit (the chains' lengths: two rows' position sums, the d sum, the final adds)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
U64, F64, F32 = np.uint64, np.float64, np.float32
M_KEYS, ABSENT = 60, 8   # keys the model holds (about a quarter without V) / keys it does not


def rev(x):   # ReverseBytes (include/difacto/base.h)
    x = np.asarray(x, U64).byteswap()
    return ((x & U64(0x0F0F0F0F0F0F0F0F)) << U64(4)) | ((x & U64(0xF0F0F0F0F0F0F0F0)) >> U64(4))


@pytest.fixture(scope="module")
def dev():
    from difacto_amd import build, capi
    build.build_hip()
    ctx = capi.Context(0)
    yield capi, ctx
    ctx.close()


def model(dev, k, seed, exact=True):
    """-> table, ids, w, has_V, V over M_KEYS + ABSENT keys; the last ABSENT are not in the table (w = 0, no V); the last key
    that is in the table has V and is drawn by no row (the non-finite case puts an Inf there)"""
    capi, ctx = dev
    rng = np.random.default_rng(seed)
    n = M_KEYS + ABSENT
    has = (rng.random(n) >= 0.25).astype(np.int32) if k else np.zeros(n, np.int32)
    w = (rng.integers(-2, 3, n) / 8 if exact else rng.normal(size=n)).astype(F32)
    V = (rng.integers(-2, 3, (n, k)) / 8 if exact else 0.3 * rng.normal(size=(n, k))).astype(F32)
    has[M_KEYS - 1], has[M_KEYS:], w[M_KEYS:] = int(k > 0), 0, 0
    ids = np.arange(1, n + 1, dtype=U64) * U64(7919)
    tb = capi.Table(ctx, 1024, V_dim=k, init_mode=capi.INIT_HASH, V_threshold=0, l1=0.0, seed=1)
    return tb, ids, w, has, V


def load(tb, ids, w, has, V):
    scal = np.zeros((M_KEYS, 4), F32)
    scal[:, 1] = w[:M_KEYS]
    tb.import_(rev(ids[:M_KEYS]), scal, has[:M_KEYS], np.concatenate([V[:M_KEYS], np.zeros_like(V[:M_KEYS])], 1) if V.shape[1] else None)


def rows_of(rng, R, exact=True, dup=(), lens=None):
    """R rows of 0 .. 12 ids (row 1 is empty), or of the given lengths -> offset, key number and x per position; dup: (a, b)
    pairs, row a repeats row b"""
    if lens is None:
        lens = rng.integers(1, 13, R)
        lens[1:2] = 0
    lens = np.array(lens, np.int64)
    assert len(lens) == R
    for a, b in dup:
        lens[a] = lens[b]
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    idx = rng.integers(0, M_KEYS + ABSENT, off[-1])
    idx[idx == M_KEYS - 1] = 0
    x = (rng.integers(1, 5, off[-1]) / 2 if exact else rng.normal(size=off[-1])).astype(F32)
    for a, b in dup:
        idx[off[a]:off[a + 1]], x[off[a]:off[a + 1]] = idx[off[b]:off[b + 1]], x[off[b]:off[b + 1]]
    return off, idx, x


def step(tb, b, ids, off, idx, x):
    b.load_host(off, ids[idx], x, np.ones(len(off) - 1, F32))
    b.localize()
    b.lookup(tb)
    b.sgd_step(tb, is_train=False)


def embed64(w, has, V, off, idx, x):
    """-> S [R, k], b [R], and the sums of absolute values: |S| [R, k], of b's terms [R]; nnz [R]"""
    R, k = len(off) - 1, V.shape[1]
    S, Sa, b, ba = np.zeros((R, k)), np.zeros((R, k)), np.zeros(R), np.zeros(R)
    with np.errstate(all="ignore"):
        for r in range(R):
            j = idx[off[r]:off[r + 1]]
            xr, xv = x[off[r]:off[r + 1]].astype(F64), (x[off[r]:off[r + 1], None].astype(F64) * V[j])[has[j] != 0]
            S[r], Sa[r], lin = xv.sum(0), np.abs(xv).sum(0), xr * w[j]
            b[r] = lin.sum() + 0.5 * (S[r] ** 2 - (xv ** 2).sum(0)).sum()
            ba[r] = np.abs(lin).sum() + 0.5 * (Sa[r] ** 2 + (xv ** 2).sum(0)).sum()
    return S, b, Sa, ba, np.diff(off)


def catalogue(dev, tb, ids, items, K, cuts=None, valued=True):
    """a Recommend whose catalogue is `items`, appended in batches that end at `cuts`"""
    capi, ctx = dev
    off, idx, x = items
    rec, b = capi.Recommend(ctx, K, capacity_hint=1), capi.Batch(ctx, len(off), max(int(off[-1]), 1))
    lo = 0
    for hi in list(cuts or []) + [len(off) - 1]:
        step(tb, b, ids, off[lo:hi + 1] - off[lo], idx[off[lo]:off[hi]], x[off[lo]:off[hi]] if valued else None)
        rec.add_items(b, tb)
        lo = hi
    assert rec.item_count() == len(off) - 1
    b.close()
    return rec


def recommend(dev, tb, ids, rec, queries):
    capi, ctx = dev
    off, idx, x = queries
    b = capi.Batch(ctx, len(off), max(int(off[-1]), 1))
    step(tb, b, ids, off, idx, x)
    rec.reset()
    rec.append_batch(b, tb)
    got = rec.read()
    assert rec.count() == len(off) - 1
    b.close()
    return got


CASES = [(0, 1, 1, 1), (0, 129, 33, 10), (1, 5, 33, 10), (1, 128, 1, 1), (1, 300, 1, 32), (7, 127, 1, 32), (7, 300, 33, 10),
         (8, 5, 1, 32), (8, 128, 129, 10), (64, 129, 33, 1), (64, 127, 129, 10), (64, 300, 129, 32)]


@pytest.mark.parametrize("k,M,R,K", CASES)
def test_exact(dev, k, M, R, K):
    """items, order (ties by number) and the logits' bits; the items carry values when M is even, x = 1 otherwise"""
    tb, ids, w, has, V = model(dev, k, 1000 * k + M)
    load(tb, ids, w, has, V)
    rng = np.random.default_rng(M + R + K)
    dup = [(a, c) for a, c in ((M - 1, 0), (129, 2), (3, 2)) if c < a < M]   # equal rows, across a tile edge too
    items, queries = rows_of(rng, M, dup=dup), rows_of(rng, R)
    valued = M % 2 == 0
    rec = catalogue(dev, tb, ids, items, K, valued=valued)
    got = recommend(dev, tb, ids, rec, queries)
    Si, bi, _, _, _ = embed64(w, has, V, items[0], items[1], items[2] if valued else np.ones_like(items[2]))
    Sq, aq, _, _, _ = embed64(w, has, V, *queries)
    s, ties = bi[None, :] + Sq @ Si.T, 0
    assert got["nonfinite"] == 0
    for q in range(R):
        order = np.lexsort((np.arange(M), -s[q]))
        top, ties = order[:K], ties + int(M > K and s[q, order[K - 1]] == s[q, order[K]])
        assert got["n"][q] == top.size and np.array_equal(got["items"][q, :top.size], top), q
        assert np.array_equal(got["logits"][q, :top.size].view(np.uint32), (aq[q] + s[q, top]).astype(F32).view(np.uint32)), q
        assert not got["items"][q, top.size:].any() and not got["logits"][q, top.size:].any()
    assert ties or k > 8 or R == 1 or M <= K, "equal scores across the K boundary"
    rec.close()
    tb.close()


def test_batches_and_splits_change_no_bit(dev):
    capi, ctx = dev
    tb, ids, w, has, V = model(dev, 64, 7, exact=False)
    load(tb, ids, w, has, V)
    rng = np.random.default_rng(8)
    items, queries = rows_of(rng, 300, exact=False, dup=[(299, 0)]), rows_of(rng, 129, exact=False)
    outs = []
    for cuts, split in ((None, 1), ([7, 200], 1), (None, 3), ([130, 131], 0)):
        ctx.set_option("rec_split", split)
        rec = catalogue(dev, tb, ids, items, 10, cuts)
        got = recommend(dev, tb, ids, rec, queries)
        outs.append(b"".join(got[f].tobytes() for f in ("n", "items", "logits")))
        rec.close()
    ctx.set_option("rec_split", 0)
    assert outs[0] == outs[1] == outs[2] == outs[3]
    tb.close()


def test_general_floats(dev):
    k, M, R, K = 64, 300, 33, 10
    tb, ids, w, has, V = model(dev, k, 21, exact=False)
    load(tb, ids, w, has, V)
    rng = np.random.default_rng(22)
    items, queries = rows_of(rng, M, exact=False), rows_of(rng, R, exact=False)
    rec = catalogue(dev, tb, ids, items, K)
    got = recommend(dev, tb, ids, rec, queries)
    Si, bi, Sai, bai, ni = embed64(w, has, V, *items)
    Sq, aq, Saq, baq, nq = embed64(w, has, V, *queries)
    logit = aq[:, None] + bi[None, :] + Sq @ Si.T
    bound = (nq[:, None] + ni[None, :] + k + 4) * 2.0 ** -24 * (baq[:, None] + bai[None, :] + Saq @ Sai.T)
    for q in range(R):
        it = got["items"][q].astype(np.int64)
        err = np.abs(got["logits"][q].astype(F64) - logit[q, it])
        print(q, "max error / bound", (err / bound[q, it]).max())
        assert got["n"][q] == K and np.unique(it).size == K and (err <= bound[q, it]).all(), (q, err, bound[q, it])
        order = np.argsort(-logit[q], kind="stable")
        clear = [i for i in order[:K] if logit[q, i] - logit[q, order[K]] > 2 * bound[q, i]]
        assert len(clear) >= 1 and np.isin(clear, it).all(), q
    rec.close()
    tb.close()


def test_non_finite_item_is_left_out_and_counted(dev):
    k, M, R, K = 8, 5, 33, 10
    tb, ids, w, has, V = model(dev, k, 31)
    V[M_KEYS - 1, 2] = np.inf   # the key no drawn row holds
    load(tb, ids, w, has, V)
    rng = np.random.default_rng(32)
    items, queries = rows_of(rng, M), rows_of(rng, R)
    items[1][items[0][3]] = M_KEYS - 1   # item 3's first position (every row but row 1 has one)
    rec = catalogue(dev, tb, ids, items, K)
    got = recommend(dev, tb, ids, rec, queries)
    assert got["nonfinite"] == R and (got["n"] == M - 1).all()
    assert not (got["items"][:, :M - 1] == 3).any() and np.isfinite(got["logits"]).all()
    rec.close()
    tb.close()
