"""Each entry's top-k FM interaction partners (csrc/dfh_pairs.hip) through capi.ModelDump.pairs,
against numpy float64: S = V64 @ V64.T over the rows dfh_dump_entries returns.

A returned score may differ from S[i, j] by at most gamma_n * sum_d |V_i[d] V_j[d]|, gamma_n = n u / (1 - n u), n = V_dim + 1,
u = 2^-24: the bound of an fp32 dot product in any summation order, products rounded or fused.  The selection is checked over
ALL pairs with the same bound; where every score is exact in fp32 (small integers) lists must EQUAL the reference's under the
tie rule (key descending, then ascending id).  Shapes sit on the tile of 128 (127, 129, 300), the staged chunk of 8 floats
(V_dim 1, 5, 8, 100) and on windows that start and end inside a tile."""
import ctypes

import numpy as np
import pytest

U64 = np.uint64


def rev(x):
    """ReverseBytes (include/difacto/base.h): the nibbles of a 64-bit word in reverse order"""
    x = np.asarray(x, U64).byteswap()
    return ((x & U64(0x0F0F0F0F0F0F0F0F)) << U64(4)) | ((x & U64(0xF0F0F0F0F0F0F0F0)) >> U64(4))


def check_lists(ids, has, V, got, first, K, by_pos):
    """checks 2 and 3 of every list of `got` (ModelDump.pairs of the window at `first`) against float64; -> the queries with V"""
    cand = np.flatnonzero(has)
    pos_of = {int(ids[e]): p for p, e in enumerate(cand)}
    V64 = V[cand].astype(np.float64)
    nu = (V.shape[1] + 1) * 2.0 ** -24
    S, B = V64 @ V64.T, nu / (1 - nu) * (np.abs(V64) @ np.abs(V64).T)
    key64 = S if by_pos else np.abs(S)
    seen = 0
    for x in range(len(got["n"])):
        e, n = first + x, int(got["n"][x])
        if not has[e]:
            assert n == 0
            continue
        seen += 1
        i = pos_of[int(ids[e])]
        assert n == min(K, cand.size - 1), (e, n)
        js = np.array([pos_of[int(t)] for t in got["ids"][x, :n]], np.int64)   # a KeyError: a partner without V
        sc = got["scores"][x, :n].astype(np.float64)
        assert i not in js and np.unique(js).size == n
        assert (np.abs(sc - S[i, js]) <= B[i, js]).all(), (e, np.abs(sc - S[i, js]).max())
        keys = sc if by_pos else np.abs(sc)
        assert (np.diff(keys) <= 0).all(), "the list is sorted by the returned keys"
        rest = np.setdiff1d(np.arange(cand.size), np.append(js, i))
        if n:
            assert (key64[i, rest] <= keys[-1] + B[i, rest]).all(), (e, (key64[i, rest] - keys[-1] - B[i, rest]).max())
    return seen


def exact_lists(ids, has, V, first, count, K, by_pos):
    """the reference's lists under the tie rule, for V whose scores are exact: -> ids, scores [count x K], n"""
    cand = np.flatnonzero(has)
    V64 = V[cand].astype(np.float64)
    S = V64 @ V64.T
    o_id, o_s, o_n = np.zeros((count, K), U64), np.zeros((count, K), np.float32), np.zeros(count, np.uint32)
    for x in range(count):
        if has[first + x]:
            i = int(np.searchsorted(cand, first + x))
            key = np.where(np.arange(cand.size) == i, -np.inf, S[i] if by_pos else np.abs(S[i]))
            top = np.lexsort((np.arange(cand.size), -key))[:min(K, cand.size - 1)]
            o_id[x, :top.size], o_s[x, :top.size], o_n[x] = ids[cand[top]], S[i, top], top.size
    return o_id, o_s, o_n


@pytest.fixture(scope="module")
def dev():
    from difacto_amd import build, capi
    build.build_hip()
    ctx = capi.Context(0)
    yield capi, ctx
    ctx.close()


def open_model(dev, nV, k, seed, integers=False):
    """nV entries with V and nV // 3 + 2 without, interleaved, all kept (w = 1); -> table, dump, its entries"""
    capi, ctx = dev
    rng = np.random.default_rng(seed)
    m = nV + nV // 3 + 2
    has = np.zeros(m, np.int32)
    has[rng.permutation(m)[:nV]] = 1
    V = (rng.integers(-2, 3, (m, k)) if integers else rng.normal(size=(m, k))).astype(np.float32)
    scal = np.zeros((m, 4), np.float32)
    scal[:, 1] = 1.0
    tb = capi.Table(ctx, max(1024, 2 * m), V_dim=k, init_mode=capi.INIT_HASH, V_threshold=0, l1=0.0, seed=1)
    tb.import_(rev(np.arange(1, m + 1, dtype=U64) * U64(7919)), scal, has, np.concatenate([V, np.zeros_like(V)], 1))
    d = capi.ModelDump(tb)
    ent = d.entries()
    assert d.shape() == (m, nV, k) and np.array_equal(ent["has_V"], has) and np.array_equal(ent["V"][has == 1], V[has == 1])
    assert all(np.array_equal(a, b) for a, b in zip(d.ids(1, m - 1), (ent["ids"][1:], has[1:])))   # dfh_dump_ids: the same, without the rows
    return tb, d, ent


@pytest.mark.gpu
@pytest.mark.parametrize("nV,k,K,by_pos", [(0, 8, 10, 0), (1, 5, 1, 0), (2, 1, 10, 1), (127, 64, 32, 0), (129, 100, 10, 1), (129, 8, 1, 0),
                                           (300, 256, 10, 0), (300, 5, 32, 1)])
def test_shapes_scores_selection(dev, nV, k, K, by_pos):
    tb, d, ent = open_model(dev, nV, k, 10 * nV + k)
    try:
        m = d.n
        for first, count in ((0, m), (m // 3 + 1, m // 2), (m - 1, 1), (0, 0)):   # whole; starts and ends inside a tile; one; none
            got = d.pairs(first, count, K, by_pos)
            assert got["nonfinite"] == 0 and got["n"].shape == (count,)
            assert check_lists(ent["ids"], ent["has_V"], ent["V"], got, first, K, by_pos) == int(ent["has_V"][first:first + count].sum())
    finally:
        d.close()
        tb.close()


@pytest.mark.gpu
@pytest.mark.parametrize("nV,first,count", [(300, 5, None), (1100, 600, 70)])
@pytest.mark.parametrize("integers", [False, True])
@pytest.mark.parametrize("by_pos", [0, 1])
def test_exact_ties_and_split_invariance(dev, nV, first, count, integers, by_pos):
    """integers: every partial sum is below 2^24, so every score is exact and the lists are the reference's, ties at the K
    boundary included; either way pairs_split 1, 3 and 0 give the same arrays bit for bit.  The automatic choice is
    min(2 CUs / query tiles, candidate tiles // 4): 1 at nV = 300 (3 candidate tiles), 2 at nV = 1100 (9) with its one query tile"""
    capi, ctx = dev
    k, K = 8, 10
    tb, d, ent = open_model(dev, nV, k, 77, integers)
    count = d.n - 9 if count is None else count
    try:
        outs = []
        for split in (1, 3, 0):
            ctx.set_option("pairs_split", split)
            outs.append(d.pairs(first, count, K, by_pos))
        for o in outs[1:]:
            assert all(np.array_equal(np.atleast_1d(o[x]).view(np.uint8), np.atleast_1d(outs[0][x]).view(np.uint8)) for x in ("ids", "scores", "n"))
        if integers:
            has, V = ent["has_V"], ent["V"]
            assert (np.abs(V[has == 1]).astype(np.float64) @ np.abs(V[has == 1]).astype(np.float64).T).max() < 2 ** 24
            w_id, w_s, w_n = exact_lists(ent["ids"], has, V, first, count, K, by_pos)
            full = exact_lists(ent["ids"], has, V, first, count, K + 1, by_pos)[1]
            full = full if by_pos else np.abs(full)
            assert ((full[:, K - 1] == full[:, K]) & (w_n == K)).sum() > 10, "equal keys across the K boundary"
            assert np.array_equal(outs[0]["n"], w_n) and np.array_equal(outs[0]["ids"], w_id) and np.array_equal(outs[0]["scores"], w_s)
    finally:
        ctx.set_option("pairs_split", 0)
        d.close()
        tb.close()


@pytest.mark.gpu
def test_non_finite_pairs_are_left_out_and_counted(dev):
    capi, ctx = dev
    nV, k, K = 129, 8, 10
    rng = np.random.default_rng(3)
    m = nV + 5
    has = (np.arange(m) % 27 != 4).astype(np.int32)
    V = rng.normal(size=(m, k)).astype(np.float32)
    bad = 70
    V[bad, 2] = np.inf
    scal = np.ones((m, 4), np.float32)
    ids = np.arange(1, m + 1, dtype=U64) * U64(7919)
    tb = capi.Table(ctx, 1024, V_dim=k, init_mode=capi.INIT_HASH, V_threshold=0, l1=0.0, seed=1)
    tb.import_(rev(ids), scal, has, np.concatenate([V, np.zeros_like(V)], 1))
    d = capi.ModelDump(tb)
    try:
        assert has.sum() == nV and has[bad]
        got = d.pairs(0, m, K, 0)
        assert got["nonfinite"] == 2 * (nV - 1)                      # (q, bad) for every other query, (bad, j) for every j
        assert got["n"][bad] == 0 and not (got["ids"] == ids[bad]).any()
        assert (got["n"][has == 1].sum(), got["n"][has == 0].sum()) == ((nV - 1) * K, 0)
        sub = d.pairs(bad + 1, 20, K, 0)                             # a window without the row itself
        assert sub["nonfinite"] == int(has[bad + 1:bad + 21].sum()) and not (sub["ids"] == ids[bad]).any()
        keep = np.arange(m) != bad                                   # the lists are those of the model without the row
        g2 = dict(ids=got["ids"][keep], scores=got["scores"][keep], n=got["n"][keep])
        assert check_lists(ids[keep], has[keep], V[keep], g2, 0, K, 0) == nV - 1
    finally:
        d.close()
        tb.close()


@pytest.mark.gpu
def test_arguments_are_refused(dev):
    capi, ctx = dev
    tb, d, ent = open_model(dev, 5, 2, 1)
    L, C = capi.lib(), ctypes
    buf, nf = C.create_string_buffer(4096), C.c_uint64(0)
    for args, word in (((0, 1, 0, 0), "topk must be in [1, 32]"), ((0, 1, 33, 0), "topk must be in [1, 32]"), ((0, 1, 3, 2), "by must be"),
                       ((0, d.n + 1, 3, 0), "first + count exceeds"), ((d.n, 1, 3, 0), "first + count exceeds")):
        assert L.dfh_dump_pairs(d.h, args[0], args[1], args[2], args[3], buf, buf, buf, C.byref(nf)) == 1 and word in L.dfh_last_error().decode()
    assert L.dfh_dump_pairs(d.h, 0, 1, 3, 0, None, buf, buf, C.byref(nf)) == 1 and L.dfh_dump_pairs(None, 0, 1, 3, 0, buf, buf, buf, C.byref(nf)) == 1
    with pytest.raises(Exception):
        ctx.set_option("pairs_split", 65)
    assert d.pairs(0, d.n, 3, 0)["n"].sum() == 5 * 3   # still usable
    d.close()
    tb.close()
