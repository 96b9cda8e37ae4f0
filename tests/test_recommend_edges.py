"""capi.Recommend (csrc/dfh_recommend.hip) on the inputs tests/test_recommend*.py do not reach: rows over 64 positions, V_dim 252 ..
256, designed score orders, several appends over rotating batch objects, a catalogue regrown behind a reset, non-finite queries
and the C ABI's refusals; every case at rec_precision 0 and 1, with the models, rows and float64 reference (embed64) of
tests/test_recommend.py: s = b_i + <S_q, S_i>, logit = a_q + s, s descending, equal s by ascending item number.

EXACT CASES.  Exactness is a property of the inputs and prove_exact asserts it from float64 alone before the device runs: for
every chain (S, Q, lin per row; the sum over d and b; s per pair) the float64 sum of the terms' absolute values times 2^g is below
2^24, 2^-g the coarsest binary grid all terms of the chain lie on.  Then every partial sum, in any order, is a multiple of 2^-g
below 2^(24 - g): an fp32 number, so fp32 computes float64's value and items, order, n and the logits' bits (one rounding of the
exact a_q + s) must be the reference's.  For rec_precision = 1 also: every S[d] is a bf16 number (at most 8 significant bits),
every b the sum of its three bf16 pieces, and the s^ chain over S and the pieces fits in the same way, so s^ = s."""
import ctypes
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import test_recommend as T   # noqa: E402

pytestmark = pytest.mark.gpu
F32, F64 = np.float32, np.float64
ERR_ARG, ERR_STATE = 1, 4   # DFH_ERR_ARG, DFH_ERR_STATE of include/difacto_hip.h
OPTIONS = ("rec_precision", "rec_shortlist", "rec_split")
LONG = [0, 1, 63, 64, 65, 66, 67, 68, 127, 128, 129, 130]   # around k_rec_embed's staging rounds of 64 and its groups of four
PRECISIONS = pytest.mark.parametrize("prec", [0, 1])
dev = T.dev
_cache = {}


@pytest.fixture
def use(dev):
    """-> use(prec, shortlist, split): the module's context creates such objects until the test ends"""
    yield lambda prec, shortlist=0, split=0: [dev[1].set_option(n, v) for n, v in zip(OPTIONS, (prec, shortlist, split))]
    for n in OPTIONS:
        dev[1].set_option(n, 0)


def close(*objs):
    for o in objs:
        o.close()


def grid(*terms):
    """the smallest g with every term a multiple of 2^-g"""
    v = np.concatenate([np.ravel(np.asarray(t, F64)) for t in terms])
    assert np.isfinite(v).all()
    for g in range(64):
        if np.array_equal(np.rint(v * 2.0 ** g), v * 2.0 ** g):
            return g
    raise AssertionError("the terms lie on no binary grid")


def fits(abs_sum, *terms):
    """a chain of these terms, whose absolute values sum to abs_sum (the largest counts), is exact in fp32 in any order"""
    return float(np.max(abs_sum, initial=0.0)) * 2.0 ** grid(*terms) < 2.0 ** 24


def bf16(v):
    """finite fp32 numbers rounded to bf16, to nearest even, as fp32"""
    u = np.asarray(v, F32).view(np.uint32).astype(np.uint64)
    return (((u + 0x7FFF + ((u >> 16) & 1)) >> 16) << 16).astype(np.uint32).view(F32)


def ones_if_none(rows):
    off, idx, x = rows
    return off, idx, np.ones(len(idx), F32) if x is None else x


def prove_exact(w, has, V, items, queries, prec):
    """asserts the module docstring's conditions from float64 alone -> embed64's s [R, M] and a_q [R]"""
    E = []
    for rows in (items, queries):
        off, idx, x = ones_if_none(rows)
        R, k = len(off) - 1, V.shape[1]
        rid = np.repeat(np.arange(R), np.diff(off))
        xv = x[:, None].astype(F64) * V[idx].astype(F64) * (has[idx] != 0)[:, None]
        lin = x.astype(F64) * w[idx].astype(F64)
        S, Sa, Q, L, La = np.zeros((R, k)), np.zeros((R, k)), np.zeros((R, k)), np.zeros(R), np.zeros(R)
        for acc, t in ((S, xv), (Sa, np.abs(xv)), (Q, xv ** 2), (L, lin), (La, np.abs(lin))):
            np.add.at(acc, rid, t)
        assert fits(Sa, xv), "S"
        assert fits(Q, xv ** 2), "Q"
        assert fits(La, lin), "lin"
        assert fits((S ** 2 + Q).sum(1), S ** 2, Q), "fma(S, S, -Q) and its sum over d"
        quad = (S ** 2 - Q).sum(1)
        assert fits(np.abs(L) + np.abs(0.5 * quad), L, 0.5 * quad), "b"
        S64, b64, _, _, _ = T.embed64(w, has, V, off, idx, x)
        assert np.array_equal(S64, S) and np.array_equal(b64, L + 0.5 * quad)
        E.append((S64, b64))
    (Si, bi), (Sq, aq) = E
    ta = np.abs(Sq) @ np.abs(Si).T
    prods = [np.multiply.outer(Sq[:, d], Si[:, d]) for d in range(Si.shape[1])]
    assert fits(np.abs(bi)[None, :] + ta, bi, *prods), "s"
    if prec:
        for S in (Si, Sq):
            assert np.array_equal(bf16(S).astype(F64), S), "S is not a bf16 number"
        rest, pieces = bi.astype(F32), []
        assert np.array_equal(rest.astype(F64), bi)
        for _ in range(3):   # k_rec_tobf16's loop
            pieces.append(bf16(rest))
            rest = rest - pieces[-1]
        assert not rest.any(), "b is not three bf16 pieces"
        assert fits(sum(np.abs(p.astype(F64)) for p in pieces)[None, :] + ta, *pieces, *prods), "the candidate score"
    return bi[None, :] + Sq @ Si.T, aq


def check(got, s, aq, K, r0=0):
    """rows r0 .. of got are the lists of the float64 scores s [R, M]: items, order, n, the logits' bits, zeros behind n; a pair
    whose s is not finite is in no list"""
    R, M = s.shape
    fin = np.isfinite(s)
    order = np.argsort(np.where(fin, -s, np.inf), axis=1, kind="stable")[:, :K]   # stable: equal s by ascending item number
    n = np.minimum(fin.sum(1), K)
    live = np.arange(order.shape[1])[None, :] < n[:, None]
    items, logits = np.zeros((R, K), np.uint32), np.zeros((R, K), F32)
    with np.errstate(all="ignore"):
        items[:, :order.shape[1]] = np.where(live, order, 0)
        logits[:, :order.shape[1]] = np.where(live, (aq[:, None] + np.take_along_axis(s, order, 1)).astype(F32), 0)
    assert np.array_equal(got["n"][r0:r0 + R], n), np.flatnonzero(got["n"][r0:r0 + R] != n)[:8]
    bad = np.flatnonzero((got["items"][r0:r0 + R] != items).any(1))
    assert bad.size == 0, (bad[:8], got["items"][r0 + bad[0]], items[bad[0]])
    bad = np.flatnonzero((got["logits"][r0:r0 + R].view(np.uint32) != logits.view(np.uint32)).any(1))
    assert bad.size == 0, (bad[:8], got["logits"][r0 + bad[0]], logits[bad[0]])


def out_bytes(got):
    return b"".join(got[f].tobytes() for f in ("n", "items", "logits"))


# ---------------------------------------------------------------- 1. rows over 64 positions
def long_model(dev, k, seed, exact=True):
    """test_recommend's model; exact: V in {-1/4, 0, 1/4}, w a multiple of 1/8 in [-1/4, 1/4]"""
    tb, ids, w, has, V = T.model(dev, k, seed, exact)
    if exact:
        V = (np.random.default_rng(seed + 1).integers(-1, 2, V.shape) / 4).astype(F32)
    T.load(tb, ids, w, has, V)
    return tb, ids, w, has, V


def long_rows(rng, has, exact=True):
    """rows of LONG positions; the last one holds a key with V at positions 3 and 70, on both sides of the staging edge"""
    off, idx, x = T.rows_of(rng, len(LONG), exact, lens=LONG)
    kv = int(np.flatnonzero(has[:T.M_KEYS - 1])[0]) if has.any() else 0
    idx[off[-2] + 3] = idx[off[-2] + 70] = kv
    return off, idx, x if not exact else np.ones_like(x)


@PRECISIONS
@pytest.mark.parametrize("valued", [True, False])
@pytest.mark.parametrize("k", [0, 5, 16])
def test_long_rows_exact(dev, use, prec, k, valued):
    """x = 1 (a value array of ones, or none), V in {-1/4, 0, 1/4}, w in multiples of 1/8, rows of up to 130 positions: |S| <=
    32.5 on a grid of 2^-2 (8 bits), S^2 and Q on 2^-4 below 2^11, the sum over 16 d and b below 2^15 on 2^-5, s below 2^16 on
    2^-5; prove_exact asserts it"""
    use(prec)
    K = 10
    tb, ids, w, has, V = long_model(dev, k, 100 + k)
    rng = np.random.default_rng(7 + k)
    items, queries = long_rows(rng, has), long_rows(rng, has)
    assert k == 0 or (has[items[1][items[0][-2] + 3]] and has[queries[1][queries[0][-2] + 70]])
    s, aq = prove_exact(w, has, V, items, queries, prec)
    bare = lambda rows: rows if valued else (rows[0], rows[1], None)
    rec = T.catalogue(dev, tb, ids, items, K, valued=valued)
    got = T.recommend(dev, tb, ids, rec, bare(queries))
    assert got["nonfinite"] == 0
    check(got, s, aq, K)
    close(rec, tb)


@PRECISIONS
def test_long_rows_general_floats(dev, use, prec):
    """normal w, V and x on the rows of LONG positions, V_dim 16: each logit within test_recommend's bound (nnz_q + nnz_i + V_dim
    + 4) 2^-24 T of float64, T the sum of the absolute values of the logit's terms; M = 12 < C, so at either precision the list
    is the fp32 list: the items float64 puts clear of the K-th place by twice the bound are there"""
    use(prec)
    k, K, M = 16, 10, len(LONG)
    tb, ids, w, has, V = long_model(dev, k, 61, exact=False)
    rng = np.random.default_rng(62)
    items, queries = long_rows(rng, has, exact=False), long_rows(rng, has, exact=False)
    rec = T.catalogue(dev, tb, ids, items, K)
    got = T.recommend(dev, tb, ids, rec, queries)
    Si, bi, Sai, bai, ni = T.embed64(w, has, V, *items)
    Sq, aq, Saq, baq, nq = T.embed64(w, has, V, *queries)
    logit = aq[:, None] + bi[None, :] + Sq @ Si.T
    bound = (nq[:, None] + ni[None, :] + k + 4) * 2.0 ** -24 * (baq[:, None] + bai[None, :] + Saq @ Sai.T)
    clear = 0
    for q in range(M):
        it = got["items"][q].astype(np.int64)
        err = np.abs(got["logits"][q].astype(F64) - logit[q, it])
        print(q, "max error / bound", (err / np.maximum(bound[q, it], 1e-300)).max())   # (empty query, empty item: 0 within 0)
        assert got["n"][q] == K and np.unique(it).size == K and (err <= bound[q, it]).all(), (q, err, bound[q, it])
        order = np.argsort(-logit[q], kind="stable")
        must = [i for i in order[:K] if logit[q, i] - logit[q, order[K]] > 2 * bound[q, i]]
        clear += len(must)
        assert np.isin(must, it).all(), q
    assert got["nonfinite"] == 0 and clear >= M
    close(rec, tb)


# ---------------------------------------------------------------- 2. V_dim 252 .. 256
@PRECISIONS
@pytest.mark.parametrize("k", [252, 253, 255, 256])
def test_wide_V_exact(dev, use, prec, k):
    """test_recommend.test_exact's grids (w, V in multiples of 1/8 up to 1/4, x in multiples of 1/2 up to 2, rows of at most 12
    ids): x V on 2^-4 with |S| <= 6 (7 bits), S^2 on 2^-8 below 2^6, the sum over 256 d and b on 2^-9 below 2^13, s on 2^-9 below
    2^14; prove_exact asserts it at 256 d, so the grid is not halved.  Column V_dim is held back in lane 63's group (252 .. 255) or
    is lane 0 of the second round (256): the last d before it must carry numbers"""
    use(prec)
    M, R, K = 129, 33, 10
    tb, ids, w, has, V = T.model(dev, k, 1000 * k + M)
    T.load(tb, ids, w, has, V)
    rng = np.random.default_rng(M + R + K)
    items, queries = T.rows_of(rng, M, dup=[(M - 1, 0), (3, 2)]), T.rows_of(rng, R)
    s, aq = prove_exact(w, has, V, items, queries, prec)
    Si, bi, _, _, _ = T.embed64(w, has, V, *items)
    Sq, _, _, _, _ = T.embed64(w, has, V, *queries)
    for d in (251, 255)[:1 + (k == 256)]:
        assert Si[:, d].any() and Sq[:, d].any(), d
    assert np.unique(bi).size > M // 2   # the held column carries the item's own number
    rec = T.catalogue(dev, tb, ids, items, K)
    got = T.recommend(dev, tb, ids, rec, queries)
    assert got["nonfinite"] == 0
    check(got, s, aq, K)
    close(rec, tb)


# ---------------------------------------------------------------- 3. designed orders
def designed(dev, kind, M):
    """V_dim 8; key 0 has V = e_0, key 1 has V = e_1, both w = 0; an item is the row {key 0: x0, key 1: x1}: S_i = (x0, x1, 0, ..),
    b_i = 0 (one position per coordinate: S^2 = Q); the queries (16, 1) and (-16, -1), and the empty row -> table, ids, model,
    items, queries"""
    tb, ids, w, has, V = T.model(dev, 8, 5)
    w[:2], has[:2], V[:2] = 0, 1, 0
    V[0, 0] = V[1, 1] = 1
    T.load(tb, ids, w, has, V)
    i = np.arange(M)
    x0, x1 = {"ramp": (i // 16, i % 16), "equal": (i * 0 + 1, i * 0 + 3), "plateaus": (i // 40, i * 0)}[kind]
    rows = lambda a, b: (2 * np.arange(len(a) + 1, dtype=np.int64), np.tile([0, 1], len(a)), np.stack([a, b], 1).ravel().astype(F32))
    off, idx, x = rows(np.array([16, -16]), np.array([1, -1]))
    return tb, ids, w, has, V, rows(x0, x1), (np.concatenate([off, off[-1:]]), idx, x)


@PRECISIONS
@pytest.mark.parametrize("K", [1, 10, 32])
@pytest.mark.parametrize("kind", ["ramp", "equal", "plateaus"])
def test_designed_orders(dev, use, prec, kind, K):
    """small integers in two coordinates: every S[d] is an integer of at most 5 bits, b = 0 and s an integer below 2^9
    (prove_exact asserts it).  ramp: s = i under the first query (every item enters at the head of the list and moves all of it),
    s = -i under the second (nothing enters behind the first K); equal: one score over three tiles; plateaus: s = +-(i // 40),
    runs of 40 equal scores across the tile edges at 128 and 256 and across the K-th and the C-th place of both queries.  The
    third query is the empty row: s = b_i = 0 for every item.  Every split and every cut of the catalogue gives the same bytes"""
    M = 300
    tb, ids, w, has, V, items, queries = designed(dev, kind, M)
    s, aq = prove_exact(w, has, V, items, queries, prec)
    i = np.arange(M)
    want = {"ramp": i, "equal": i * 0 + 19, "plateaus": 16 * (i // 40)}[kind]
    assert np.array_equal(s, np.stack([want, -want, 0 * want]).astype(F64)) and not aq.any()
    outs = set()
    for shortlist in sorted({0, K, 64}) if prec else [0]:   # (rec_shortlist is not read at rec_precision 0)
        for cuts in (None, [1], [128, 129]):
            use(prec, shortlist)
            rec = T.catalogue(dev, tb, ids, items, K, cuts)
            for split in (0, 1, 3, 64):
                use(prec, shortlist, split)
                got = T.recommend(dev, tb, ids, rec, queries)
                assert got["nonfinite"] == 0
                check(got, s, aq, K)
                outs.add(out_bytes(got))
            rec.close()
    assert len(outs) == 1
    tb.close()


# ---------------------------------------------------------------- 4. several appends
def stage(tb, b, ids, rows, stepped):
    """load, localize and look up; stepped: take the prediction step too"""
    off, idx, x = rows
    b.load_host(off, ids[idx], x, np.ones(len(off) - 1, F32))
    b.localize()
    b.lookup(tb)
    if stepped:
        b.sgd_step(tb, is_train=False)


@PRECISIONS
@pytest.mark.parametrize("k", [8, 64])
def test_several_appends_in_append_order(dev, prec, k):
    """appends of 5, 300, 1 and 129 rows without a reset, the pipeline on, two batch objects in rotation, the next minibatch
    loaded while this one is queried (the workspaces grow from the small append to the large one and are used again by the
    smaller ones); again in another order behind a reset.  test_recommend's exact grids; prove_exact asserts them"""
    capi, _ = dev
    ctx = capi.Context(0)
    ctx.set_pipeline(True)
    ctx.set_option("rec_precision", prec)
    own = (capi, ctx)
    K, M, sizes = 10, 130, [5, 300, 1, 129]
    tb, ids, w, has, V = T.model(own, k, 400 + k)
    T.load(tb, ids, w, has, V)
    rng = np.random.default_rng(41)
    items = T.rows_of(rng, M)
    mbs = [T.rows_of(rng, R) for R in sizes]
    want = [prove_exact(w, has, V, items, mb, prec) for mb in mbs]
    rec = T.catalogue(own, tb, ids, items, K)
    bs = [capi.Batch(ctx, max(sizes) + 1, 12 * max(sizes)) for _ in range(2)]
    for order in ((0, 1, 2, 3), (1, 3, 0, 2)):
        rec.reset()
        stage(tb, bs[0], ids, mbs[order[0]], True)
        for t in range(4):
            if t + 1 < 4:
                stage(tb, bs[(t + 1) % 2], ids, mbs[order[t + 1]], False)
            if t:
                bs[t % 2].sgd_step(tb, is_train=False)
            rec.append_batch(bs[t % 2], tb)
            assert rec.count() == sum(sizes[o] for o in order[:t + 1])
        got = rec.read()
        assert rec.count() == sum(sizes) == len(got["n"]) and got["nonfinite"] == 0
        r0 = 0
        for o in order:
            check(got, *want[o], K, r0)
            r0 += sizes[o]
    close(rec, *bs, tb, ctx)


@PRECISIONS
def test_out_arrays_grow_past_16384_rows(dev, use, prec):
    """three appends of 6 000 rows of 1 .. 3 ids against 5 items: the third moves the out arrays from 16 384 rows to 32 768, and
    the 12 000 rows written before keep their bytes.  test_recommend's exact grids; prove_exact asserts them"""
    capi, ctx = dev
    use(prec)
    k, K, M, R = 8, 3, 5, 6000
    tb, ids, w, has, V = T.model(dev, k, 77)
    T.load(tb, ids, w, has, V)
    rng = np.random.default_rng(78)
    items = T.rows_of(rng, M)
    off, idx, x = T.rows_of(rng, 3 * R, lens=rng.integers(1, 4, 3 * R))
    if "grow" not in _cache:
        _cache["grow"] = prove_exact(w, has, V, items, (off, idx, x), 1)
    s, aq = _cache["grow"]
    rec = T.catalogue(dev, tb, ids, items, K)
    b = capi.Batch(ctx, R + 1, 3 * R)
    for t in range(3):
        lo, hi = off[t * R], off[(t + 1) * R]
        T.step(tb, b, ids, off[t * R:(t + 1) * R + 1] - lo, idx[lo:hi], x[lo:hi])
        rec.append_batch(b, tb)
        if t == 1:
            first = rec.read()
    got = rec.read()
    assert rec.count() == 3 * R and len(first["n"]) == 2 * R and got["nonfinite"] == 0
    for f in ("n", "items", "logits"):
        assert got[f][:2 * R].tobytes() == first[f].tobytes(), f
    check(got, s, aq, K)
    close(rec, b, tb)


# ---------------------------------------------------------------- 5. a catalogue grown behind a reset
@PRECISIONS
def test_catalogue_grows_behind_a_reset(dev, use, prec):
    """capacity_hint = 1: a store of 128 items; 100 items, a query, a reset, 200 more (the store, both arrays at rec_precision 1,
    doubles twice and its rows are copied), the query again: the bytes of a catalogue of the 300 built at once.  test_recommend's
    exact grids; prove_exact asserts them"""
    capi, ctx = dev
    use(prec)
    k, K, M, R = 8, 10, 300, 33
    tb, ids, w, has, V = T.model(dev, k, 91)
    T.load(tb, ids, w, has, V)
    rng = np.random.default_rng(92)
    items, queries = T.rows_of(rng, M, dup=[(299, 0), (129, 2)]), T.rows_of(rng, R)
    s, aq = prove_exact(w, has, V, items, queries, prec)
    cut = lambda lo, hi: (items[0][lo:hi + 1] - items[0][lo], items[1][items[0][lo]:items[0][hi]], items[2][items[0][lo]:items[0][hi]])
    rec, b = capi.Recommend(ctx, K, capacity_hint=1), capi.Batch(ctx, M + 1, 12 * M)
    T.step(tb, b, ids, *cut(0, 100))
    rec.add_items(b, tb)
    got = T.recommend(dev, tb, ids, rec, queries)
    assert rec.item_count() == 100 and got["nonfinite"] == 0
    check(got, s[:, :100], aq, K)
    rec.reset()
    T.step(tb, b, ids, *cut(100, 300))
    rec.add_items(b, tb)
    assert rec.item_count() == 300 and rec.count() == 0
    got = T.recommend(dev, tb, ids, rec, queries)
    check(got, s, aq, K)
    whole = T.catalogue(dev, tb, ids, items, K)
    assert out_bytes(T.recommend(dev, tb, ids, whole, queries)) == out_bytes(got)
    close(whole, rec, b, tb)


# ---------------------------------------------------------------- 6. non-finite
def with_inf(dev, seed):
    tb, ids, w, has, V = T.model(dev, 8, seed)
    V[T.M_KEYS - 1, 2] = np.inf   # the key no drawn row holds
    T.load(tb, ids, w, has, V)
    return tb, ids, w, has, V


def scores64(w, has, V, items, queries):
    Si, bi, _, _, _ = T.embed64(w, has, V, *items)
    Sq, aq, _, _, _ = T.embed64(w, has, V, *queries)
    with np.errstate(all="ignore"):
        return bi[None, :] + Sq @ Si.T, aq


@PRECISIONS
@pytest.mark.parametrize("M", [5, 300])
def test_non_finite_queries_get_empty_rows(dev, use, prec, M):
    """two of 33 query rows hold a key with an Inf in V: S_q[2] = Inf makes every s of the row Inf or NaN (Inf 0 = NaN against an
    item's zero, and against the zero rows that pad the last item tile, which are not counted): n = 0, a row of zeros, M pairs
    counted per row; the other rows keep the bytes of a run without the key.  test_recommend's exact grids; prove_exact asserts
    them on the run without the key"""
    use(prec)
    K, R, bad = 10, 33, (0, 20)
    tb, ids, w, has, V = with_inf(dev, 31)
    rng = np.random.default_rng(32 + M)
    items, queries = T.rows_of(rng, M), T.rows_of(rng, R)
    clean = (queries[0], queries[1].copy(), queries[2])
    for r in bad:
        queries[1][queries[0][r]] = T.M_KEYS - 1
    assert not (clean[1] == T.M_KEYS - 1).any() and not (items[1] == T.M_KEYS - 1).any()
    s0, aq0 = prove_exact(w, has, np.where(np.isfinite(V), V, 0), items, clean, prec)
    s, aq = scores64(w, has, V, items, queries)
    assert int((~np.isfinite(s)).sum()) == 2 * M and np.array_equal(np.delete(s, bad, 0), np.delete(s0, bad, 0))
    rec = T.catalogue(dev, tb, ids, items, K)
    got0 = T.recommend(dev, tb, ids, rec, clean)
    got = T.recommend(dev, tb, ids, rec, queries)
    assert got0["nonfinite"] == 0 and got["nonfinite"] == 2 * M
    check(got0, s0, aq0, K)
    check(got, s, aq, K)
    for r in bad:
        assert got["n"][r] == 0 and not got["items"][r].any() and not got["logits"][r].view(np.uint32).any()
    for f in ("n", "items", "logits"):
        assert np.delete(got[f], bad, 0).tobytes() == np.delete(got0[f], bad, 0).tobytes(), f
    close(rec, tb)


@PRECISIONS
def test_non_finite_item_in_the_third_tile_of_a_split(dev, use, prec):
    """item 260 of 300 holds the Inf key, rec_split = 3 (one tile per split): absent from every list, one pair counted per query,
    all logits finite, the other items as float64 has them"""
    use(prec, 0, 3)
    K, M, R = 10, 300, 33
    tb, ids, w, has, V = with_inf(dev, 35)
    rng = np.random.default_rng(36)
    items, queries = T.rows_of(rng, M), T.rows_of(rng, R)
    items[1][items[0][260]] = T.M_KEYS - 1
    s, aq = scores64(w, has, V, items, queries)
    assert np.array_equal(np.argwhere(~np.isfinite(s))[:, 1], np.full(R, 260))
    s0, _ = prove_exact(w, has, np.where(np.isfinite(V), V, 0), items, queries, prec)
    assert np.array_equal(np.delete(s, 260, 1), np.delete(s0, 260, 1))
    rec = T.catalogue(dev, tb, ids, items, K)
    got = T.recommend(dev, tb, ids, rec, queries)
    assert got["nonfinite"] == R and (got["n"] == K).all() and not (got["items"] == 260).any() and np.isfinite(got["logits"]).all()
    check(got, s, aq, K)
    close(rec, tb)


# ---------------------------------------------------------------- 7. refusals
@PRECISIONS
def test_arguments_are_refused(dev, use, prec):
    """codes and the words of the messages; behind each refusal the object answers a good query as before"""
    capi, ctx = dev
    use(prec)
    L, C = capi.lib(), ctypes
    said = lambda word: word in L.dfh_last_error().decode()
    h, u64 = C.c_void_p(), C.c_uint64(0)
    for topk in (0, 33):
        assert L.dfh_recommend_create(ctx.h, topk, 0, C.byref(h)) == ERR_ARG and said("topk must be in [1, 32]")
    assert L.dfh_recommend_create(None, 3, 0, C.byref(h)) == ERR_ARG and said("NULL argument")
    assert L.dfh_recommend_create(ctx.h, 3, 0, None) == ERR_ARG and said("NULL argument")
    assert L.dfh_recommend_create(ctx.h, 3, 2 ** 31, C.byref(h)) == ERR_ARG and said("capacity_hint must be below 2^31 - 128 items")
    assert not h.value
    k, K, M, R = 8, 3, 5, 9
    tb, ids, w, has, V = T.model(dev, k, 13)
    T.load(tb, ids, w, has, V)
    tb2 = capi.Table(ctx, 1024, V_dim=k, init_mode=capi.INIT_HASH, V_threshold=0, l1=0.0, seed=1)
    T.load(tb2, ids, w, has, V)
    rng = np.random.default_rng(14)
    items, queries, more = T.rows_of(rng, M), T.rows_of(rng, R), T.rows_of(rng, 4)
    both = (np.concatenate([items[0], items[0][-1] + more[0][1:]]), np.concatenate([items[1], more[1]]), np.concatenate([items[2], more[2]]))
    s, aq = prove_exact(w, has, V, both, queries, prec)
    rec, b = capi.Recommend(ctx, K), capi.Batch(ctx, 16, 200)

    def good(m):
        got = T.recommend(dev, tb, ids, rec, queries)
        assert rec.item_count() == m and got["nonfinite"] == 0
        check(got, s[:, :m], aq, K)

    T.step(tb, b, ids, *items)
    assert L.dfh_recommend_append_batch(rec.h, b.h, tb.h) == ERR_STATE and said("the catalogue is empty")
    assert L.dfh_recommend_add_items(None, b.h, tb.h) == ERR_ARG and said("NULL argument")
    assert L.dfh_recommend_add_items(rec.h, None, tb.h) == ERR_ARG and L.dfh_recommend_add_items(rec.h, b.h, None) == ERR_ARG
    assert rec.item_count() == 0 and rec.count() == 0
    rec.add_items(b, tb)
    good(M)
    assert L.dfh_recommend_append_batch(None, b.h, tb.h) == ERR_ARG and said("NULL argument")
    assert L.dfh_recommend_append_batch(rec.h, None, tb.h) == ERR_ARG and L.dfh_recommend_append_batch(rec.h, b.h, None) == ERR_ARG
    assert L.dfh_recommend_count(rec.h, None) == ERR_ARG and L.dfh_recommend_item_count(rec.h, None) == ERR_ARG
    assert L.dfh_recommend_read(rec.h, None, None, None, C.byref(u64)) == ERR_ARG and said("NULL argument")   # rows are held
    assert L.dfh_recommend_read(rec.h, None, None, None, None) == ERR_ARG and L.dfh_recommend_reset(None) == ERR_ARG
    assert rec.count() == R
    good(M)
    stage(tb, b, ids, queries, False)   # loaded, not stepped
    for call in (L.dfh_recommend_append_batch, L.dfh_recommend_add_items):
        assert call(rec.h, b.h, tb.h) == ERR_STATE and said("dfh_sgd_step")
    b.sgd_step(tb, is_train=False)
    b.localize()   # a new view of the minibatch: the step's row words are gone
    assert L.dfh_recommend_append_batch(rec.h, b.h, tb.h) == ERR_STATE and said("dfh_sgd_step") and rec.count() == R
    good(M)
    T.step(tb2, b, ids, *queries)   # another table than the catalogue's
    assert L.dfh_recommend_append_batch(rec.h, b.h, tb2.h) == ERR_ARG and said("the catalogue was built on another table")
    assert L.dfh_recommend_append_batch(rec.h, b.h, tb.h) == ERR_STATE and said("dfh_sgd_step")
    good(M)
    ctx2 = capi.Context(0)
    b2 = capi.Batch(ctx2, 16, 200)
    assert L.dfh_recommend_append_batch(rec.h, b2.h, tb.h) == ERR_ARG and said("belongs to another context")
    close(b2, ctx2)
    good(M)
    T.step(tb, b, ids, *more)
    assert L.dfh_recommend_add_items(rec.h, b.h, tb.h) == ERR_STATE and said("queries are held")
    good(M)
    rec.reset()
    rec.add_items(b, tb)   # behind a reset the catalogue grows again
    good(M + 4)
    close(rec, b, tb2, tb)
