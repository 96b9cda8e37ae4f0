"""The dfh_lbfgs object's history against the float32 mirror of tests/lbfgs_ref.py, vector by vector and bit for bit:
PrepareCalcDirection folded into k_lb_inner<NBT, V, true> (all four instantiations, with tails), the s / y rings at every
wrap position, CalcDirection's Add chain into the ring (k_lb_combine), the line-search step (k_lb_wstep), and the scalar
results against the mirror's fp64 sums.  The test drives the object with coefficients and steps of its own
(lbfgs_ref.draw_coefficients, lbfgs_ref.ALPHAS); the mirror's gradient input is the device's g_new, so nothing but the
vector algebra is compared.

The <grad f, p> that line_search returns is (float) a + (float) b of two fp64 sums, a float add as the reference's
scheduler adds the worker's and the server's floats.  It is compared with the mirror's restatement of exactly that,
float32(float32(a) + float32(b)), within 2^-24 (|a| + |b|) + 1e-10 sum |products|.  (Against the unrounded a + b the three
roundings allow 2^-24 (|a| + |b| + |a + b|); the test prints the worst ratio of both readings.)"""
import numpy as np
import pytest

import lbfgs_ref as L

L2, VL2 = 0.1, 0.01
f32 = np.float32
U24 = 2.0 ** -24
# name -> m, epochs, epochs at which every vector is compared bit for bit (None: all)
RING = {"m1": (1, 4, None), "m2": (2, 5, None), "m3": (3, 6, None), "m16": (16, 19, None),
        "wide": (11, 13, (1, 5, 6, 10, 11, 12))}
WIDE_U = 8201          # keys, all with V at V_dim = 256: n = 8201 * 257 = 2 107 657, odd, above 2048 * 256 * 4
_cache = {}


def data(name):
    if name not in _cache:
        if name == "wide":
            C = L.big_case(256, WIDE_U, 28, seed=9, nval_rows=20)
        else:
            for pad in (0, 1):       # the model size must be odd: the (21, 2) form and both V = 4 forms then have a tail
                C = L.designed_case(3, seed=31, tail=1, vth=4, pad_keys=pad)
                if L.make_model(C).n % 2:
                    break
        M, w = L.prepare(C, wseed=3)
        _cache[name] = (C, M, w)
    return _cache[name]


def nb_form(k):
    """the k_lb_inner<NBT, V, true> instantiation that 2k + 1 right-hand vectors select"""
    nb = 2 * k + 1
    return (3, 4) if nb <= 3 else (11, 4) if nb <= 11 else (21, 2) if nb <= 21 else (33, 1)


@pytest.mark.parametrize("name", sorted(RING))
def test_ring_design(name):
    """what the case must reach, from the model size and the schedule alone"""
    C, M, w = data(name)
    m, epochs, _ = RING[name]
    n = M.n
    ks = [min(e, m) for e in range(1, epochs)]
    assert n % 2 == 1 and n % 4 in (1, 3), n
    assert 0 < M.hasV.sum() and (name == "wide" or M.hasV.sum() < len(M.keys)), "mixed lens"
    assert epochs >= m + 2, "at least two prepares on a full ring: s_first / y_first wrap"
    forms = {nb_form(k) for k in ks}
    if name == "m16":
        assert forms == {(3, 4), (11, 4), (21, 2), (33, 1)} and ks[:16] == list(range(1, 17)) and ks.count(16) >= 3
    if name == "wide":
        assert n == WIDE_U * 257 > 2048 * 256 * 4 and forms == {(3, 4), (11, 4), (21, 2), (33, 1)}
        for V in (4, 2, 1):
            assert (n + 256 * V - 1) // (256 * V) > 2048, "MAXBLOCKS reached: the grid-stride loop runs"
        assert 200 <= M.tr[0].n <= 400
    pats = [L.ALPHAS[e % 4] for e in range(epochs)]
    xs = [f32(a) - f32(b) for p in pats for a, b in zip(p, [0.0] + p[:-1])]
    assert any(x == 0 for x in xs) and any(x == 1 for x in xs)
    assert any(p[-1] == 1 for p in pats[:-1]) and any(p[-1] != 1 for p in pats[:-1])


def test_mirror_schedule_on_the_reference_gradient():
    """the m = 3 schedule with the float64 reference gradient (rounded to float) in the device's place: the mirror's own
    bookkeeping (ring lengths, the drop-oldest rule, the clamp share that draw_coefficients promises), on the CPU"""
    C, M, w = data("m3")
    m, epochs, _ = RING["m3"]
    mir = L.Mirror(w, M.isV, L2, VL2, m)
    rng = np.random.default_rng(1)
    gnew = M.grad(mir.w)["g"].astype(np.float32)
    for e in range(epochs):
        want = mir.prepare(gnew)
        assert (want is None) == (e == 0) and len(mir.y) == min(e, m)
        if e:
            assert len(want) == 6 * len(mir.y) + 1
            d = L.draw_coefficients(mir, rng)
            assert (d == 0).any() and (d[:len(mir.y)] == 1).any()
        old = [v.copy() for v in mir.s]
        mir.direction(d if e else None)
        assert len(mir.s) == min(e + 1, m)
        if e:
            assert 0.01 <= mir.clamped <= 0.5
        keep = old[1:] if len(old) == m else old
        assert all(L.same_bits(a, b) for a, b in zip(keep, mir.s[:-1]))
        for alpha in L.ALPHAS[e % 4]:
            w0 = mir.w
            x = mir.line_search(alpha)
            assert (x == 0) == L.same_bits(w0, mir.w) or not mir.s[-1].any()
        gnew = M.grad(mir.w)["g"].astype(np.float32)


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


def _close(got, want, mag, what):
    tol = L.inner_tol(want, mag)
    assert abs(got - want) <= tol, "%s: got %r want %r, |diff| %.3g > %.3g" % (what, got, want, abs(got - want), tol)


def _history(obj, mir, what):
    """every live vector of both rings and g against the mirror's, bit for bit: a wrong ring index shows as an old vector
    in the wrong logical place"""
    assert L.same_bits(obj.vector(1), mir.g), "%s: g" % what
    for i, v in enumerate(mir.y):
        assert L.same_bits(obj.vector(3, i), v), "%s: y[%d] of %d" % (what, i, len(mir.y))
    for i, v in enumerate(mir.s):
        assert L.same_bits(obj.vector(2, i), v), "%s: s[%d] of %d" % (what, i, len(mir.s))


def _arg_errors_before(capi, obj):
    with pytest.raises(capi.DfhError, match="which must be 0"):
        obj.vector(4)
    with pytest.raises(capi.DfhError, match="before the first dfh_lbfgs_prepare_direction"):
        obj.vector(1)
    with pytest.raises(capi.DfhError, match="s index is outside the history"):
        obj.vector(2, 0)


def _arg_errors_after(capi, obj, mir):
    with pytest.raises(capi.DfhError, match="s index is outside the history"):
        obj.vector(2, len(mir.s))
    with pytest.raises(capi.DfhError, match="y index is outside the history"):
        obj.vector(3, len(mir.y))
    with pytest.raises(capi.DfhError, match="s index is outside the history"):
        obj.vector(2, -1)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["m1", "m2", "m3", "m16", "wide"])
def test_ring(capi, ctx, name):
    C, M, w = data(name)
    m, epochs, full_at = RING[name]
    obj = capi.Lbfgs(ctx, C.V_dim, m)
    worst_pg = worst_pg_unrounded = 0.0
    try:
        for c in C.train:
            obj.add_chunk(*c)
        for c in C.val:
            obj.add_chunk(*c, is_val=True)
        obj.init_model(tail_feature_filter=C.tail, V_threshold=C.vth, V_init_scale=0.01, l2=L2, V_l2=VL2)
        mdl = obj.get_model()
        assert np.array_equal(mdl["keys"], M.keys) and np.array_equal(mdl["lens"], M.lens)
        obj.set_weights(w)
        mir = L.Mirror(w, M.isV, L2, VL2, m)
        rng = np.random.default_rng(17)
        if name == "m2":
            _arg_errors_before(capi, obj)
        obj.calc_grad()
        gnew = obj.vector(0)
        forms = set()
        for e in range(epochs):
            full = full_at is None or e in full_at
            tag = "%s epoch %d" % (name, e)
            # PrepareCalcDirection + CalcIncreB
            incr = obj.prepare_direction()
            want = mir.prepare(gnew)
            k = len(mir.y)
            if e == 0:
                assert incr is None and want is None
            else:
                forms.add(nb_form(k))
                assert len(incr) == 6 * k + 1, "%s: incr_B has %d entries for k = %d" % (tag, len(incr), k)
                for i, (wv, mg) in enumerate(want):
                    _close(float(incr[i]), wv, mg, "%s: incr_B[%d] (k = %d)" % (tag, i, k))
            if full:
                _history(obj, mir, tag + " after prepare_direction")
            # CalcDirection
            d = L.draw_coefficients(mir, rng) if e else None
            pg = obj.calc_direction(d)
            wpg, mg = mir.direction(d)
            if e:
                assert 0.01 <= mir.clamped <= 0.5, "%s: %.3f of the direction clamped" % (tag, mir.clamped)
            _close(pg, wpg, mg, tag + ": <g, p>")
            if full:
                _history(obj, mir, tag + " after calc_direction")   # the new s last, the older ones untouched
            if name == "m2" and e == 1:
                _arg_errors_after(capi, obj, mir)
            # LineSearch
            for alpha in L.ALPHAS[e % 4]:
                before = mir.w
                x = mir.line_search(alpha)
                f, pg1, _ = obj.line_search(alpha)
                gnew = obj.vector(0)
                wd = obj.get_model()["w"]
                assert L.same_bits(wd, mir.w), "%s: w after line_search(%g), x = %g" % (tag, alpha, x)
                if x == 0:
                    assert L.same_bits(wd, before), "%s: w moved on x == 0" % tag
                _, nnz, r = obj.evaluate()
                rw, (b, bm), nz = mir.reg()
                assert nnz == nz, "%s: nnz %r against %d" % (tag, nnz, nz)
                assert abs(r - rw) <= U24 * abs(rw) + 1e-12 * abs(rw), "%s: r(w) %r against %r" % (tag, r, rw)
                a, am = L.inner(gnew, mir.s[-1])
                tol = U24 * (abs(a) + abs(b)) + 1e-10 * (am + bm)
                want32 = float(f32(f32(a) + f32(b)))
                worst_pg = max(worst_pg, abs(pg1 - want32) / tol)
                worst_pg_unrounded = max(worst_pg_unrounded, abs(pg1 - (a + b)) / tol)
                assert abs(pg1 - want32) <= tol, "%s: <grad f, p> %r against %r (a %r, b %r)" % (tag, pg1, want32, a, b)
        print("\n%s: n = %d, forms %s; worst <grad f, p> err / tol %.3f (against the unrounded a + b: %.3f)" % (
            name, M.n, sorted(forms), worst_pg, worst_pg_unrounded))
        if name in ("m16", "wide"):
            assert forms == {(3, 4), (11, 4), (21, 2), (33, 1)}
    finally:
        obj.close()
