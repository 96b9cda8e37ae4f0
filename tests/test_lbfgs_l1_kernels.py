"""l1 on w for learner = lbfgs (orthant-wise L-BFGS, difacto_amd/csrc/dfh_owlqn.hip) on the C ABI against the float32 mirror
of tests/owlqn_ref.py: the pseudo-gradient, the aligned direction, every trial w, w0, s_last and y_last bit for bit over
three epochs with two backtracks each, and the scalars (<pg, p>, sum pg (w - w0), r(w), the 6m+1 products) against float64
sums of the mirror's float32 terms within 2^-23 |value| + n 2^-52 sum |terms|.

Shapes: a mixed-lens model (V elements between w elements, the mask path), n in {1, 3, 1024, 1025} (scalar tails, one block
and two), and n = 2048 * 256 * 4 + 3, just past the grid cap, where the grid-stride loop takes a second trip."""
import numpy as np
import pytest

import lbfgs_ref as L
import owlqn_ref as O

L2, VL2 = 0.1, 0.01
f32 = np.float32
BIG_N = 2048 * 256 * 4 + 3
TRIALS = (1.0, 0.5, 0.25)           # two backtracks in every epoch
EPOCHS = 3
_cache = {}


class _Flat:
    """what the drive needs of a model: n, isV, keys, lens"""


def flat_case(U, seed, per_key):
    """V_dim = 0: keys 1 .. U, each in per_key random rows; the last row empty; no validation chunk"""
    rng = np.random.default_rng(seed)
    C = L.Case()
    C.V_dim, C.tail, C.vth = 0, 0, 0
    if per_key == 1:
        nrows = (U + 63) // 64 + 1
        rows, keys = np.arange(U) // 64, rng.permutation(np.arange(1, U + 1))
    else:
        nrows = max(3, U // 8 + 2)
        keys = np.tile(np.arange(1, U + 1), per_key)
        rows = rng.integers(0, nrows - 1, len(keys))
    off, ids, v = L._csr(nrows, rows, keys, L._values(rng, len(keys)), rng)
    C.train, C.val = [[off, ids, v, (rng.random(nrows) < 0.5).astype(np.float32)]], []
    M = _Flat()
    M.n, M.isV = U, np.zeros(U, bool)
    M.keys, M.lens = np.arange(1, U + 1, dtype=np.uint64), np.ones(U, np.int32)
    w = rng.uniform(-0.3, 0.3, U).astype(np.float32)
    w[::7] = 0
    if U > 14:
        w[14] = -0.0
    return C, M, w


def data(name):
    if name not in _cache:
        if name == "mixed":
            for pad in (0, 1):
                C = L.designed_case(3, seed=31, tail=1, vth=4, pad_keys=pad)
                if L.make_model(C).n % 2:
                    break
            M, w = L.prepare(C, wseed=3)
            w = w.copy()
            z = np.flatnonzero((w == 0) & ~M.isV)
            w[z[1]] = -0.0                                   # -0.0 behaves as zero
        elif name == "big":
            C, M, w = flat_case(BIG_N, 5, 1)
        else:
            C, M, w = flat_case(int(name[1:]), 7, 2)
        _cache[name] = (C, M, w)
    return _cache[name]


L1 = {"mixed": 0.3, "big": 0.2, "n1": 0.2, "n3": 0.2, "n1024": 0.2, "n1025": 0.2}


def test_design_mixed():
    """on the reference's float64 gradient: the mixed case has V elements between w elements, an odd size, and its weights
    and l1 reach all five pseudo-gradient branches; a V element has |g'| < l1"""
    C, M, w = data("mixed")
    assert M.n % 2 == 1 and 0 < M.hasV.sum() < len(M.keys)
    inner_w = np.flatnonzero(~M.isV[1:-1] & M.isV[:-2] & M.isV[2:])
    assert len(inner_w), "a w element with V elements on both sides"
    mir = O.Mirror(w, M.isV, L2, VL2, 2, L1["mixed"])
    gp = (M.grad(w)["g"] + np.where(M.isV, VL2, L2) * w).astype(np.float32)
    br = mir.branches(gp)
    for b in range(5):
        assert (br == b).sum() >= 3, "branch %d" % b
    assert (np.abs(gp[M.isV]) < mir.l1).any()
    assert np.signbit(w[(w == 0) & ~M.isV]).any(), "a -0.0 weight"


def test_design_sizes():
    assert BIG_N > 2048 * 256 * 4 and BIG_N % 4 == 3
    for n in (1, 3, 1024, 1025):
        assert data("n%d" % n)[1].n == n
    assert (1024 + 1023) // 1024 == 1 and (1025 + 1023) // 1024 == 2, "one block and two of the float4 passes"


def test_mirror_pseudo_gradient_rules():
    """the mirror's own rules on hand-made numbers, on the CPU"""
    w = np.array([0.5, -0.5, 0, 0, 0, -0.0, 0, 0.25], np.float32)
    isV = np.array([0, 0, 0, 0, 0, 0, 0, 1], bool)
    mir = O.Mirror(w, isV, 0.0, 0.0, 2, 0.25)
    g = np.array([1, 1, -1, 1, 0.1, -0.25, 0.25, 0.1], np.float32)
    assert mir.prepare(g) is None
    want = np.array([1.25, 0.75, -0.75, 0.75, 0, 0, 0, 0.1], np.float32)
    assert L.same_bits(mir.pg, want), mir.pg                # +0 at the boundary |g'| == l1 and inside it
    mir.direction(None)
    assert L.same_bits(mir.s[-1], -want + f32(0))
    mir.line_search(1.0)
    # 0.5 - 1.25 crosses zero: projected to +0; -0.5 - 0.75 stays; zeros move off along -pg; the V element moves freely
    assert L.same_bits(mir.w, np.array([0, -1.25, 0.75, -0.75, 0, 0, 0, f32(0.25) + f32(-0.1)], np.float32)), mir.w
    assert mir.projected == 1 and mir.sums()["moved"] == 5


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


def _close(got, want, n, what):
    v, mag = want
    tol = O.sum_tol(v, n, mag)
    assert abs(got - v) <= tol, "%s: got %r want %r, |diff| %.3g > %.3g" % (what, got, v, abs(got - v), tol)


def _make(capi, ctx, C, M, w, m, l1):
    obj = capi.Lbfgs(ctx, C.V_dim, m)
    for c in C.train:
        obj.add_chunk(*c)
    for c in C.val:
        obj.add_chunk(*c, is_val=True)
    obj.init_model(tail_feature_filter=C.tail, V_threshold=C.vth, V_init_scale=0.01, l2=L2, V_l2=VL2)
    mdl = obj.get_model()
    assert np.array_equal(mdl["keys"], M.keys) and np.array_equal(mdl["lens"], M.lens)
    obj.set_weights(w)
    if l1 is not None:
        obj.set_l1(l1)
    return obj


def _coefficients(mir, rng):
    k = len(mir.y)
    d = rng.choice(L.FREE, 2 * k + 1).astype(np.float32)
    d[0], d[-1] = 1, -0.37                                   # an exact 1 (no shortcut is taken) and pg always in the chain
    if k > 1:
        d[1] = 0
    return d


def drive(capi, ctx, name, l1, m=2, drop_at=None, record=None):
    """three epochs, three trials each, every vector against the mirror bit for bit -> the mirror"""
    C, M, w = data(name)
    n = M.n
    obj = _make(capi, ctx, C, M, w, m, l1)
    seen = set()
    try:
        mir = O.Mirror(w, M.isV, L2, VL2, m, l1)
        rng = np.random.default_rng(23)
        obj.calc_grad()
        gnew = obj.vector(0)
        for e in range(EPOCHS):
            tag = "%s epoch %d" % (name, e)
            incr = obj.prepare_direction()
            want = mir.prepare(gnew)
            seen |= set(np.unique(mir.branches(mir.gp_last)).tolist())
            pg = obj.owlqn_vector(0)
            assert L.same_bits(pg, mir.pg), tag + ": pg"
            assert L.same_bits(obj.vector(1), mir.g), tag + ": g stays the smooth gradient"
            vsel = mir.isV & (np.abs(mir.g) < mir.l1)
            assert L.same_bits(pg[vsel], mir.g[vsel]), tag + ": a V element below l1 keeps its gradient"
            if e == 0:
                assert incr is None and want is None
            else:
                k = len(mir.y)
                assert len(incr) == 6 * k + 1
                for i, wv in enumerate(want):
                    _close(float(incr[i]), wv, n, "%s: incr_B[%d] (k = %d)" % (tag, i, k))
                assert L.same_bits(obj.vector(2, k - 1), mir.s[-1]), tag + ": s_last = w - w0"
                assert L.same_bits(obj.vector(3, k - 1), mir.y[-1]), tag + ": y_last"
                assert L.same_bits(mir.s[-1], mir.w - mir.w0)
                if drop_at == e:
                    assert k == 2
                    keep = obj.vector(2, 0)
                    obj.drop_last_pair()
                    mir.drop_last()
                    with pytest.raises(capi.DfhError, match="s index is outside the history"):
                        obj.vector(2, 1)
                    with pytest.raises(capi.DfhError, match="y index is outside the history"):
                        obj.vector(3, 1)
                    assert L.same_bits(obj.vector(2, 0), keep) and L.same_bits(keep, mir.s[0])
                    assert L.same_bits(obj.vector(3, 0), mir.y[0])
            d = _coefficients(mir, rng) if mir.y else None
            pgp = obj.calc_direction(d)
            _close(pgp, mir.direction(d), n, tag + ": <pg, p>")
            p = obj.vector(2, len(mir.s) - 1)
            assert L.same_bits(p, mir.s[-1]), tag + ": the aligned p"
            assert L.same_bits(obj.owlqn_vector(1), mir.w0), tag + ": w0"
            if n >= 1000:
                assert e == 0 or mir.dropped > 0, tag + ": the alignment dropped nothing"
                assert p[vsel].any() or not vsel.any(), tag + ": a V element below l1 keeps its step"
            for alpha in TRIALS:
                mir.line_search(alpha)
                f, armijo, _ = obj.line_search(alpha)
                gnew = obj.vector(0)
                wd = obj.get_model()["w"]
                assert L.same_bits(wd, mir.w), "%s: w after the trial alpha = %g" % (tag, alpha)
                S = mir.sums()
                _close(armijo, S["armijo"], n, "%s: sum pg (w - w0) at alpha = %g" % (tag, alpha))
                _, nnz, r = obj.evaluate()
                _close(r, S["r"], n, "%s: r(w) at alpha = %g" % (tag, alpha))
                assert nnz == S["nnz"] and obj.owlqn_moved() == S["moved"], tag
                zeros = wd[~mir.isV] == 0
                assert not np.signbit(wd[~mir.isV][zeros & (mir.w0[~mir.isV] != 0)]).any(), tag + ": a projected zero is +0.0"
                if record is not None:
                    record.append((tag, alpha, f, armijo, r, wd.tobytes(), gnew.tobytes()))
            if record is not None:
                record.append((tag, pgp, pg.tobytes(), p.tobytes()))
        mir.seen = seen
        return mir
    finally:
        obj.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["mixed", "n1", "n3", "n1024", "n1025", "big"])
def test_owlqn_against_the_mirror(capi, ctx, name):
    mir = drive(capi, ctx, name, L1[name])
    if name in ("mixed", "big"):
        assert mir.seen >= {0, 1, 2, 3, 4}, "pseudo-gradient branches reached: %s" % sorted(mir.seen)
    if name == "mixed":
        assert -1 in mir.seen


@pytest.mark.gpu
def test_drop_last_pair(capi, ctx):
    """two pairs, the newer one dropped: the ring forgets it, the older keeps its bits, the direction uses one pair"""
    drive(capi, ctx, "mixed", L1["mixed"], m=3, drop_at=2)


@pytest.mark.gpu
def test_second_run_gives_the_same_bits(capi, ctx):
    a, b = [], []
    drive(capi, ctx, "n1025", L1["n1025"], record=a)
    drive(capi, ctx, "n1025", L1["n1025"], record=b)
    assert a == b and len(a) == EPOCHS * (len(TRIALS) + 1)


@pytest.mark.gpu
def test_boundary_l1_equals_the_gradient(capi, ctx):
    """l1 set to exactly |g'_j| read back for a w_j = 0: pg_j is +0.0, and the element stays at +0.0 through a trial"""
    C, M, w = data("mixed")
    probe = _make(capi, ctx, C, M, w, 2, None)
    try:
        probe.calc_grad()
        gnew = probe.vector(0)
    finally:
        probe.close()
    gp = gnew + np.where(M.isV, f32(VL2), f32(L2)).astype(np.float32) * w
    cand = np.flatnonzero((w == 0) & ~M.isV & (gp != 0))
    j = int(cand[np.argsort(np.abs(gp[cand]))[len(cand) // 2]])
    l1 = float(abs(gp[j]))
    obj = _make(capi, ctx, C, M, w, 2, l1)
    try:
        obj.calc_grad()
        assert L.same_bits(obj.vector(0), gnew), "the gradient pass is deterministic"
        mir = O.Mirror(w, M.isV, L2, VL2, 2, l1)
        assert obj.prepare_direction() is None and mir.prepare(gnew) is None
        pg = obj.owlqn_vector(0)
        assert L.same_bits(pg, mir.pg)
        assert pg[j:j + 1].view(np.uint32)[0] == 0, "pg_j = %r at the boundary" % pg[j]
        assert {2, 3, 4} <= set(np.unique(mir.branches(mir.gp_last)).tolist())
        _close(obj.calc_direction(None), mir.direction(None), M.n, "<pg, p>")
        obj.line_search(0.5)
        mir.line_search(0.5)
        wd = obj.get_model()["w"]
        assert L.same_bits(wd, mir.w) and wd[j:j + 1].view(np.uint32)[0] == 0
    finally:
        obj.close()


def _plain_drive(capi, ctx, call_set_l1):
    """three epochs of the plain learner's calls on the mixed case -> every vector and scalar"""
    C, M, w = data("mixed")
    obj = _make(capi, ctx, C, M, w, 2, 0.0 if call_set_l1 else None)
    out = []
    try:
        mir = L.Mirror(w, M.isV, L2, VL2, 2)
        rng = np.random.default_rng(17)
        out.append(obj.calc_grad())
        gnew = obj.vector(0)
        for e in range(EPOCHS):
            incr = obj.prepare_direction()
            mir.prepare(gnew)
            out.append(None if incr is None else incr.tobytes())
            d = L.draw_coefficients(mir, rng) if e else None
            out.append(obj.calc_direction(d))
            mir.direction(d)
            for alpha in L.ALPHAS[e % 4]:
                mir.line_search(alpha)
                out.append(obj.line_search(alpha))
                gnew = obj.vector(0)
                out.append(obj.evaluate())
                out.append(obj.get_model()["w"].tobytes())
            out.append(obj.vector(1).tobytes())
            out += [obj.vector(2, i).tobytes() for i in range(len(mir.s))]
            out += [obj.vector(3, i).tobytes() for i in range(len(mir.y))]
            out.append(gnew.tobytes())
        with pytest.raises(capi.DfhError, match="has no l1"):
            obj.owlqn_vector(0)
        return out
    finally:
        obj.close()


@pytest.mark.gpu
def test_set_l1_zero_changes_nothing(capi, ctx):
    assert _plain_drive(capi, ctx, True) == _plain_drive(capi, ctx, False)


@pytest.mark.gpu
def test_set_l1_arguments(capi, ctx):
    C, M, w = data("n3")
    obj = _make(capi, ctx, C, M, w, 2, None)
    try:
        for bad in (-1.0, float("nan")):
            with pytest.raises(capi.DfhError, match="l1 must be >= 0"):
                obj.set_l1(bad)
        obj.set_l1(0.25)
        with pytest.raises(capi.DfhError, match="before the first dfh_lbfgs_prepare_direction"):
            obj.owlqn_vector(0)
        with pytest.raises(capi.DfhError, match="which must be 0"):
            obj.owlqn_vector(2)
        with pytest.raises(capi.DfhError, match="no complete"):
            obj.drop_last_pair()
        obj.calc_grad()
        with pytest.raises(capi.DfhError, match="before the first dfh_lbfgs_calc_grad"):
            obj.set_l1(0.5)
        with pytest.raises(capi.DfhError, match="before the first dfh_lbfgs_calc_grad"):
            obj.set_l1(0.0)
        obj.prepare_direction()
        with pytest.raises(capi.DfhError, match="no w0 before"):
            obj.owlqn_vector(1)
    finally:
        obj.close()
