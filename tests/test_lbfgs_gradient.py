"""The dfh_lbfgs gradient pass (k_lb_gather -> forward -> backward -> k_lb_scatter per chunk, k_lb_gamma) element by
element against the float64 reference of tests/lbfgs_ref.py, on data built by rule (lbfgs_ref.designed_case / big_case:
every occurrence class of k_backward_all, empty rows, a feature twice in a row, clamped rows, keys in one, two and three
chunks, filtered keys inside a wave and at a chunk's end, keys with and without V, a binary chunk, validation keys
outside the model) at every lane layout of gather / scatter: row strides 4, 8, 12, 16, 20, 64, 68 and 260, chunks whose
key count lies on both sides of a wave and of a block, and one chunk large enough for the grid cap.

The pass is deterministic (no float atomics; a key occurs once per chunk and the chunks run in order on one stream): a
second pass must return the same bits, and does here.  The designs are asserted on the CPU (test_designs, not marked gpu)
and so is the checker: test_checker_rejects_wrong_gradients perturbs the reference as the kernels could be wrong."""
import numpy as np
import pytest

import lbfgs_ref as L

L2, VL2 = 0.1, 0.01
# (V_dim, tail_feature_filter, V_threshold): row strides 4 (no mask), 8, 12, 16, 20, 64, 68 (the c += 64 loop), 260
CASES = [(0, 1, 4), (3, 1, 4), (5, 0, 0), (12, 1, 4), (13, 2, 6), (60, 1, 4), (61, 0, 3), (256, 1, 4)]
BIG = (60, 8192 * 4 + 5, 20)     # V_dim, U, entries per row: one key per wave, (waves + 3) / 4 = 8194 blocks asked for
_cache = {}
_worst = {}


def case(name):
    """the designed chunks, the reference model and the weights of a case, built once"""
    if name not in _cache:
        if name == "big":
            C = L.big_case(BIG[0], BIG[1], BIG[2], seed=77)
        else:
            V_dim, tail, vth = name
            C = L.designed_case(V_dim, seed=100 + V_dim, tail=tail, vth=vth)
        M, w = L.prepare(C, wseed=5)
        _cache[name] = (C, M, w, M.grad(w))
    return _cache[name]


@pytest.mark.parametrize("name", CASES, ids=lambda c: "V%d-tail%d-vth%d" % c)
def test_designs(name):
    C, M, w, R = case(name)
    L.census(C, M, w)
    assert C.stride == {0: 4, 3: 8, 5: 12, 12: 16, 13: 20, 60: 64, 61: 68, 256: 260}[C.V_dim]
    assert len(M.tr) >= 3 and len(M.va) == 2
    assert (R["mag"] == 0).sum() >= 1 and R["touched"].all()


def test_big_design():
    C, M, w, R = case("big")
    assert C.pw == 1 and C.stride == 64 and [c.U for c in M.tr] == [BIG[1]] and len(M.keys) == BIG[1]
    waves = (BIG[1] + C.pw - 1) // C.pw
    assert (waves + 3) // 4 == 8194 > 8192, "k_lb_gather's grid is capped at 8192 blocks: keys 32768 .. take u += ustep"
    assert 8192 * 4 * C.pw < BIG[1]
    assert M.hasV.all() and (np.diff(M.tr[0].off) == 0).any()
    for (f, ff), c in zip(M.logits(w, M.tr + M.va), M.tr + M.va):
        assert L.min_class_gap(f, ff, c.lab) > 1


def test_checker_rejects_wrong_gradients():
    """check_gradient on the V_dim = 3 case must pass the float32 rounding of its own reference and reject that vector
    perturbed as a wrong kernel would leave it"""
    C, M, w, R = case((3, 1, 4))
    k = M.k
    base = R["g"].astype(np.float32)
    assert L.check_gradient(base, R) <= 1.0
    pos = M.pos
    at = lambda key: int(np.searchsorted(M.keys, np.uint64(key)))   # noqa: E731

    def rejected(bad, what):
        with pytest.raises(AssertionError):
            L.check_gradient(bad, R)
            pytest.fail("not rejected: " + what, pytrace=False)

    # 1. one key's V gradient shifted by one float
    i = at(C.all3[0])
    assert M.hasV[i]
    bad = base.copy()
    bad[pos[i] + 1:pos[i] + 1 + k] = np.roll(base[pos[i] + 1:pos[i] + 1 + k], 1)
    rejected(bad, "V gradient shifted by one float")
    # 2. one chunk's contribution to a key that lies in two chunks left out
    i = at(C.pair[0][0])
    assert sum(bool((c.map == i).any()) for c in M.tr[:3]) == 2
    bad = base.copy()
    bad[pos[i]:pos[i + 1]] = (R["g"] - R["contrib"][0])[pos[i]:pos[i + 1]]
    rejected(bad, "a chunk's contribution lost")
    # 3. a filtered key's gradient added to its neighbour in the chunk
    c = M.tr[0]
    u = int(np.flatnonzero((c.map[:-1] < 0) & (c.map[1:] >= 0))[0])
    bad = base.copy()
    bad[pos[c.map[u + 1]]] += np.float32(R["raw"][0][0][u])
    rejected(bad, "a filtered key's gradient in its neighbour")
    # 4. V gradient written for a key without V: the vector grows, or the floats land on what follows the key's w
    u = int(np.flatnonzero((c.map >= 0) & ~M.hasV[np.maximum(c.map, 0)] & (c.cnt >= 2))[0])
    f, _ = R["pred"][0]
    p = -c.y / (1.0 + np.exp(c.y * f))
    Wd, Vd = M.split(w)
    _, Vc, _ = M.chunk_rows(c, Wd, Vd)
    would = np.asarray(c.D.XT[u] @ ((c.D.X @ Vc) * p[:, None])).ravel()
    assert np.abs(would).min() > 0
    rejected(np.concatenate([base, would.astype(np.float32)]), "a longer vector")
    i = int(c.map[u])
    bad = base.copy()
    bad[pos[i] + 1:pos[i] + 1 + k] += would.astype(np.float32)
    rejected(bad, "V gradient spilled behind a key without V")
    # 5. the last key of a wave left at zero
    c2 = M.tr[2]
    u = next(u for u in range(C.pw - 1, c2.U, C.pw) if c2.map[u] >= 0)
    i = int(c2.map[u])
    bad = base.copy()
    bad[pos[i]:pos[i + 1]] = (R["g"] - R["contrib"][2])[pos[i]:pos[i + 1]]
    rejected(bad, "the last key of a wave not scattered")
    # 6. the hot key's gw short of one of its 200+ addends (the median one)
    i = at(C.hot)
    x = np.asarray(c.D.XT[0].todense()).ravel()
    add = np.abs(x * p)
    r = int(np.argsort(add)[len(add) // 2])
    assert (x != 0).sum() >= 200 and add[r] > 0
    bad = base.copy()
    bad[pos[i]] = np.float32(R["g"][pos[i]] - x[r] * p[r])
    rejected(bad, "one addend of the hot key lost")


# ------------------------------------------------------------------------------------------------ on the device

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


def _auc_sum(oracle, chunks, preds):
    """AUC x n per chunk on the float64 logits, summed over the chunks in float as the object sums them"""
    a = np.float32(0)
    for c, (f, _) in zip(chunks, preds):
        a = np.float32(a + np.float32(oracle.auc_times_n(c.lab, f.astype(np.float32))))
    return float(a)


def _device_case(capi, ctx, oracle, name):
    C, M, w, R = case(name)
    obj = capi.Lbfgs(ctx, C.V_dim, 2)
    try:
        for c in C.train:
            obj.add_chunk(*c)
        for c in C.val:
            obj.add_chunk(*c, is_val=True)
        obj.init_model(tail_feature_filter=C.tail, V_threshold=C.vth, V_init_scale=0.01, l2=L2, V_l2=VL2)
        m = obj.get_model()
        assert np.array_equal(m["keys"], M.keys), "keys"
        assert np.array_equal(m["lens"], M.lens), "lens"
        assert np.array_equal(m["cnt"], M.cnt), "cnt"
        obj.set_weights(w)
        loss, auc = obj.calc_grad()
        g1 = obj.vector(0)
        worst = L.check_gradient(g1, R, "g_new of %r" % (name,))
        _worst[name] = worst
        print("\n%r: worst err / tol of g_new %.3f; loss err / tol %.3f" % (
            name, worst, abs(loss - R["loss"]) / (1e-5 * abs(R["loss"]) + R["loss_floor"])))
        assert abs(loss - R["loss"]) <= 1e-5 * abs(R["loss"]) + R["loss_floor"], (loss, R["loss"])
        assert auc == pytest.approx(_auc_sum(oracle, M.tr, R["pred"]), rel=1e-5), "training AUC x n"
        va = obj.evaluate(val=True)[0]
        assert va == pytest.approx(_auc_sum(oracle, M.va, M.logits(w, M.va)), rel=1e-5), "validation AUC x n"
        loss2, auc2 = obj.calc_grad()
        assert L.same_bits(obj.vector(0), g1) and loss2 == loss and auc2 == auc, "a second pass differs"
        # k_lb_gamma on the device's own gradient: sign(x) |x|^gamma in double, rounded to float; an exact 0 stays (-)0
        x = g1.astype(np.float64)
        for gamma in (0.5, 2.0):
            obj.calc_grad(gamma)
            got = obj.vector(0)
            want = (np.where(x > 0, 1.0, -1.0) * np.abs(x) ** gamma).astype(np.float32)
            ulp = np.spacing(np.abs(want)).astype(np.float64)
            err = np.abs(got.astype(np.float64) - want.astype(np.float64))
            assert (err <= ulp).all(), "gamma %g: %d elements beyond one ulp" % (gamma, int((err > ulp).sum()))
            assert not (got[g1 == 0] != 0).any()
        return worst
    finally:
        obj.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", CASES, ids=lambda c: "V%d-tail%d-vth%d" % c)
def test_gradient_elementwise(capi, ctx, oracle, name):
    _device_case(capi, ctx, oracle, name)


@pytest.mark.gpu
def test_gradient_grid_cap(capi, ctx, oracle):
    """U = 8192 * 4 + 5 keys at one key per wave: gb = min((32773 + 3) / 4, 8192) = 8192, the last five keys take the
    u += ustep step of k_lb_gather and k_lb_scatter"""
    _device_case(capi, ctx, oracle, "big")


@pytest.mark.gpu
def test_worst_ratio_report(capi, ctx, oracle):
    """prints the worst err / tol over the cases run in this session (-s shows it); every case asserted its own <= 1"""
    if not _worst:
        _device_case(capi, ctx, oracle, CASES[1])
    name = max(_worst, key=_worst.get)
    print("\nworst err / tol of the gradient comparison over %d cases: %.3f (%r); recorded on an MI355X: %r" % (
        len(_worst), _worst[name], name, L.GRAD_WORST_MEASURED))
    assert _worst[name] <= 1.0
