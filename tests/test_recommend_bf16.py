"""rec_precision = 1 of capi.Recommend (k_rec_tobf16, k_rec_cand, k_rec_rescore of csrc/dfh_recommend.hip) against numpy float64
evaluating the definition, with the models, rows and reference of tests/test_recommend.py.
Exact cases: every S[d] is a multiple of 2^-4 below 8 (a bf16 number), every b a multiple of 2^-9 below 2^14 (three bf16 pieces),
every partial sum exact in fp32: the candidate scores ARE the scores, so items, order and the logits' bits must equal float64's.
General floats: a logit within test_recommend's bound; an item of the float64 top K must be there whenever fewer than C items
come within 2 E(q) + tol of it, E(q) = 2^-7 max_i sum_d |S_q[d] S_i[d]| (operand rounding; the bias is exact) + the fp32 bound."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import test_recommend as T   # noqa: E402
import test_recommend_cli as TC   # noqa: E402

pytestmark = pytest.mark.gpu
F32, F64 = np.float32, np.float64
dev, built = T.dev, TC.built


@pytest.fixture
def bf16(dev):
    """-> use(shortlist, split): the context creates bf16 objects until the test ends"""
    names = ("rec_precision", "rec_shortlist", "rec_split")
    yield lambda shortlist=0, split=0: [dev[1].set_option(n, v) for n, v in zip(names, (1, shortlist, split))]
    for n in names:
        dev[1].set_option(n, 0)


def exact_case(dev, k, M, R, K, cuts=None):
    """test_recommend.test_exact's model, items (equal rows, across a tile edge too) and queries -> got, float64 s, a_q"""
    tb, ids, w, has, V = T.model(dev, k, 1000 * k + M)
    T.load(tb, ids, w, has, V)
    rng = np.random.default_rng(M + R + K)
    dup = [(a, c) for a, c in ((M - 1, 0), (129, 2), (3, 2)) if c < a < M]
    items, queries = T.rows_of(rng, M, dup=dup), T.rows_of(rng, R)
    rec = T.catalogue(dev, tb, ids, items, K, cuts)
    got = T.recommend(dev, tb, ids, rec, queries)
    Si, bi, _, _, _ = T.embed64(w, has, V, *items)
    Sq, aq, _, _, _ = T.embed64(w, has, V, *queries)
    rec.close()
    tb.close()
    return got, bi[None, :] + Sq @ Si.T, aq


# V_dim 0, 1, 13, 14, 64, 125: kb - V_dim = 16, 15, 3, 18, 16, 3 (the bias pieces are the whole operand / start a chunk / straddle
# a chunk edge); shortlist 0 = min(64, max(16, 4 K)).  (1, 5, 33, 10): M < K; (0, 1, 1, 1): M < C
CASES = [(0, 1, 1, 1, 0), (0, 129, 33, 10, 10), (1, 128, 1, 1, 1), (1, 5, 33, 10, 0), (13, 127, 129, 10, 64), (13, 300, 33, 32, 32),
         (14, 129, 33, 10, 0), (14, 300, 1, 32, 64), (64, 128, 129, 10, 0), (64, 300, 33, 1, 0), (125, 127, 33, 10, 10),
         (125, 300, 129, 32, 0)]


@pytest.mark.parametrize("k,M,R,K,shortlist", CASES)
def test_exact(dev, bf16, k, M, R, K, shortlist):
    """items, order (ties by number) and the logits' bits"""
    bf16(shortlist)
    got, s, aq = exact_case(dev, k, M, R, K)
    assert got["nonfinite"] == 0
    for q in range(R):
        top = np.lexsort((np.arange(M), -s[q]))[:K]
        assert got["n"][q] == top.size and np.array_equal(got["items"][q, :top.size], top), q
        assert np.array_equal(got["logits"][q, :top.size].view(np.uint32), (aq[q] + s[q, top]).astype(F32).view(np.uint32)), q
        assert not got["items"][q, top.size:].any() and not got["logits"][q, top.size:].any()


def test_batches_and_splits_change_no_bit(dev, bf16):
    outs = set()
    for cuts in (None, [1], [128], [129]):
        for split in (0, 1, 3, 64):
            bf16(0, split)
            got, _, _ = exact_case(dev, 64, 300, 33, 10, cuts)
            outs.add(b"".join(got[f].tobytes() for f in ("n", "items", "logits")))
    assert len(outs) == 1


def test_general_floats(dev, bf16):
    k, M, R, K, C = 64, 300, 33, 10, 40
    tb, ids, w, has, V = T.model(dev, k, 51, exact=False)
    T.load(tb, ids, w, has, V)
    rng = np.random.default_rng(52)
    items, queries = T.rows_of(rng, M, exact=False), T.rows_of(rng, R, exact=False)
    Si, bi, Sai, bai, ni = T.embed64(w, has, V, *items)
    Sq, aq, Saq, baq, nq = T.embed64(w, has, V, *queries)
    s = bi[None, :] + Sq @ Si.T
    bound = (nq[:, None] + ni[None, :] + k + 4) * 2.0 ** -24 * (baq[:, None] + bai[None, :] + Saq @ Sai.T)
    E = 2.0 ** -7 * (np.abs(Sq) @ np.abs(Si).T).max(1) + bound.max(1)
    top = [np.argsort(-s[q], kind="stable")[:K] for q in range(R)]
    must = [[i for i in top[q] if (s[q] > s[q, i] - 2 * E[q] - bound[q, i]).sum() < C] for q in range(R)]
    assert sum(map(len, must)) >= 0.9 * R * K   # of the inputs alone: the check below is not hollow
    bf16(C)
    rec = T.catalogue(dev, tb, ids, items, K)
    got = T.recommend(dev, tb, ids, rec, queries)
    for q in range(R):
        it = got["items"][q].astype(np.int64)
        err = np.abs(got["logits"][q].astype(F64) - (aq[q] + s[q, it]))
        assert got["n"][q] == K and np.unique(it).size == K and (err <= bound[q, it]).all(), (q, err, bound[q, it])
        key = got["logits"][q]   # a_q + s: the add may round two s to one logit, so equal logits say nothing about the numbers
        assert all(key[j] > key[j + 1] or (key[j] == key[j + 1] and (it[j] < it[j + 1] or s[q, it[j]] != s[q, it[j + 1]]))
                   for j in range(K - 1)), q
        assert np.isin(must[q], it).all(), q
    rec.close()
    tb.close()


def test_non_finite_item_is_left_out_and_counted(dev, bf16):
    """an Inf in a V entry one item draws.  The count is taken over the SWEEP (a pair whose bf16 score is not finite is never a
    candidate) plus the candidates whose exact s is not finite in the re-rank: disjoint sets, none here in the second"""
    k, M, R, K = 8, 5, 33, 10
    tb, ids, w, has, V = T.model(dev, k, 31)
    V[T.M_KEYS - 1, 2] = np.inf
    T.load(tb, ids, w, has, V)
    rng = np.random.default_rng(32)
    items, queries = T.rows_of(rng, M), T.rows_of(rng, R)
    items[1][items[0][3]] = T.M_KEYS - 1
    bf16(0)
    rec = T.catalogue(dev, tb, ids, items, K)
    got = T.recommend(dev, tb, ids, rec, queries)
    Si, bi, _, _, _ = T.embed64(w, has, V, *items)
    Sq, _, _, _, _ = T.embed64(w, has, V, *queries)
    with np.errstate(all="ignore"):
        want = int((~np.isfinite(bi[None, :] + Sq @ Si.T)).sum())
    assert want == R and got["nonfinite"] == want and (got["n"] == M - 1).all()
    assert not (got["items"][:, :M - 1] == 3).any() and np.isfinite(got["logits"]).all()
    rec.close()
    tb.close()


def test_refused_options(dev, bf16):
    capi, ctx = dev
    for name, v in (("rec_precision", 2), ("rec_shortlist", 65)):
        with pytest.raises(capi.DfhError, match=name) as e:
            ctx.set_option(name, v)
        assert e.value.code == 1   # DFH_ERR_ARG
    bf16(9)
    with pytest.raises(capi.DfhError, match="rec_shortlist = 9 below topk = 10") as e:
        capi.Recommend(ctx, 10)
    assert e.value.code == 1


def test_command_line(built, tmp_path):
    """recommend_out parses, <= K entries in descending order; pred_out keeps its bytes; an unknown precision is fatal"""
    model, items, K = str(tmp_path / "model"), str(tmp_path / "items.libsvm"), 10
    r = TC.run(built, "model_out=" + model, "max_num_epochs=2", "lr=.05", "stop_rel_objv=0", "stop_val_auc=-1e30", *TC.COMMON)
    assert r.returncode == 0, r.stderr[-3000:]
    pool, rng = np.unique(TC.libsvm(TC.DATA)[1]), np.random.default_rng(3)
    with open(items, "w") as f:
        f.write("".join("1 " + " ".join("%d:1" % i for i in np.sort(rng.choice(pool, 3, replace=False))) + "\n" for _ in range(TC.M)))
    pred = []
    for extra in ([], ["items_in=" + items, "recommend_out=" + str(tmp_path / "rec"), "recommend_precision=bf16", "recommend_shortlist=20"]):
        p = str(tmp_path / ("pred%d" % len(pred)))
        r = TC.run(built, "task=predict", "model_in=" + model, "pred_out=" + p, *extra, *TC.COMMON)
        assert r.returncode == 0, r.stderr[-3000:]
        pred.append(open(p, "rb").read())
    assert pred[0] == pred[1] and pred[0].count(b"\n") == 100
    lines = open(str(tmp_path / "rec")).read().split("\n")[:-1]
    assert len(lines) == 100
    for line in lines:
        tok = [t.split(":") for t in line.split("\t")]
        v = [np.float32(x) for _, x in tok]
        assert 1 <= len(tok) <= K and all(0 <= int(i) < TC.M for i, _ in tok) and all(a >= b for a, b in zip(v, v[1:])), line
    r = TC.run(built, *TC.PRED, "recommend_out=x", "items_in=y", "recommend_precision=half", *TC.COMMON)
    assert r.returncode != 0 and "recommend_precision=half" in r.stderr and "fp32" in r.stderr and "bf16" in r.stderr, r.stderr[-2000:]
