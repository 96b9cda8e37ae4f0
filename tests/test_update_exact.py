"""The update arithmetic, bit for bit.

dfh_kernels.hip claims that ftrl_update_w / adagrad_update_v are the reference's SGDUpdater operation for operation, so that
"given the same gradient the new V and accumulator are the reference's, bit for bit"; dfh_update.hip adds that every key is
updated by exactly one role and that the result is deterministic.  Two families of tests hold the project to it, with no
tolerance, no skipped key and no mask:

  raw pushes        Table.push(keys, GRADIENT, ...) and the owner-side dfh_shard_* forms feed an arbitrary gradient to the
                    update kernels; the C oracle (built with -ffp-contract=off, correctly rounded sqrt) applies the same
                    operations, so every field of every key must agree as 32-bit patterns after every push.
  exact-sum steps   minibatches on which forward, gradient and update have exactly one right answer (exact_step_design.py):
                    one fused step from an imported model, through every role and every switch of the step.

The MIXED instantiation of k_update_fused is reached only through a communicator: test_sharded_exact.py pins it, with the
mixed forward, the others' row words and the owner side inside a step, on the same designs against scripted peers, and
test_sharded_overlap_exact.py pins the schedule that keeps two minibatches in flight on streams of three such designs with
disjoint keys.  A second step on the SAME keys is pinned in test_second_step_exact.py.

  progress sums     every step of a design here is also held to the one right Progress (exact_step_design.exact_progress): row
                    count, the loss (the floats of the three values log1pf(1.0f) may take), AUC x n of the exact logits, and
                    — under the "pen" variant, whose l1, l2 and V_l2 put every term on one grid — the penalty, bit for bit;
                    the packed path counts none (+0), a validation step counts it through k_penalty.  Two reads give the same
                    bits, a reset leaves zeros, and two steps in one batch object add up as doubles before the cast.

Still not pinned: the V-dependent logits of a second step; the loss of the zero rows at V_dim = 0 (below the float's
resolution there: the V_dim > 0 designs pin that term); l2's penalty term beside the drivers (pinned on the driverless copy
exact_step_design.l2_copy alone); the penalty under the other variants' hyper-parameters, which are on no grid.
"""
import numpy as np
import pytest

import exact_step_design as X
from split_testlib import split_entries_expected


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


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def same_bits(got, want, what):
    got, want = bits(got), bits(want)
    assert got.shape == want.shape, what
    if got.size == 0:
        return
    bad = np.flatnonzero((got != want).reshape(len(got), -1).any(1)) if got.ndim > 1 else np.flatnonzero(got != want)
    assert len(bad) == 0, "%s: %d of %d differ, first at %d: got %r want %r" % (
        what, len(bad), len(got), bad[0], got[bad[0]].view(np.float32), want[bad[0]].view(np.float32))


# ------------------------------------------------------------------ models as arrays
def oracle_model(so, keys, V_dim):
    """OracleStore.peek of every key -> (scal [n, 4] = {fea_cnt, w, sqrt_g, z}, has_V [n], V [n, 2 V_dim], zero without V)"""
    n = len(keys)
    scal = np.zeros((n, 4), np.float32)
    has = np.zeros(n, np.int32)
    V = np.zeros((n, 2 * V_dim), np.float32)
    for i, key in enumerate(keys):
        e = so.peek(int(key))
        assert e is not None, "key %d is not in the oracle store" % key
        scal[i] = [e["fea_cnt"], e["w"], e["sqrt_g"], e["z"]]
        if e["V"] is not None:
            has[i] = 1
            V[i] = e["V"]
    return scal, has, V


def device_model(tb):
    """Table.export() sorted by key -> (keys, scal, has_V, V [n, 2 V_dim])"""
    e = tb.export()
    o = np.argsort(e["keys"])
    V = e["V"][o] if e["V"] is not None else np.zeros((len(o), 0), np.float32)
    return e["keys"][o], e["scal"][o], e["has_V"][o], V


def assert_model_equals_oracle(tb, so, V_dim, what, nkeys=None):
    """every key of the device table against the oracle's entry, every field, as bit patterns"""
    keys, scal, has, V = device_model(tb)
    if nkeys is not None:
        assert len(keys) == nkeys, "%s: %d keys on the device, %d pushed" % (what, len(keys), nkeys)
    oscal, ohas, oV = oracle_model(so, keys, V_dim)
    assert np.array_equal(has != 0, ohas != 0), "%s: has_V differs at keys %r" % (what, keys[(has != 0) != (ohas != 0)][:5])
    for j, name in enumerate(("fea_cnt", "w", "sqrt_g", "z")):
        same_bits(scal[:, j], oscal[:, j], "%s: %s" % (what, name))
    if V_dim:
        same_bits(V[:, :V_dim], oV[:, :V_dim], "%s: V" % what)
        same_bits(V[:, V_dim:], oV[:, V_dim:], "%s: accumulators" % what)
    return keys, scal, has, V


# ================================================================== raw pushes
RAW_KW = dict(l1=0.25, l2=0.01, lr=0.3, V_lr=0.05, V_l2=0.02, V_threshold=2, V_init_scale=0.25, seed=7)
RAW_KEYS = 2000
RAW_ROUNDS = 3
L1 = np.float32(RAW_KW["l1"])
OUT = np.nextafter(L1, np.float32(1))       # one representable step outside +l1


def _ftrl32(gw, w, sg, z, kw):
    """SGDUpdater::UpdateW in numpy fp32 scalars — used ONLY to search for gradients that land z on +-l1; what the landing
    has to be is asserted on the oracle's state afterwards"""
    f = np.float32
    gw, w, sg, z = f(gw), f(w), f(sg), f(z)
    gw = gw + w * f(kw["l2"])
    nsg = np.sqrt(sg * sg + gw * gw)
    return z - (gw - (nsg - sg) / f(kw["lr"]) * w)


def _land_z(e, target, kw):
    """a gradient after which z of the entry e is exactly `target`, or None"""
    w, sg, z = e["w"], e["sqrt_g"], e["z"]
    target = np.float32(target)
    g = np.float32(z) - target
    with np.errstate(all="ignore"):
        for _ in range(40):      # dz / dg is about -1: walk the residual down ...
            r = _ftrl32(g, w, sg, z, kw) - target
            if r == 0:
                return g
            g = np.float32(g + r)
        lo = hi = g              # ... then try the neighbouring floats
        for _ in range(200):
            lo, hi = np.nextafter(lo, np.float32(-np.inf)), np.nextafter(hi, np.float32(np.inf))
            for c in (lo, hi):
                if _ftrl32(c, w, sg, z, kw) == target:
                    return c
    return None


def _random_grad(rng, n):
    """full mantissas over 1e-6 .. 1e3, either sign"""
    return (np.exp(rng.uniform(np.log(1e-6), np.log(1e3), n)) * rng.choice([-1.0, 1.0], n)).astype(np.float32)


def raw_ops(so, V_dim, rng, kw=RAW_KW, nkeys=RAW_KEYS, rounds=RAW_ROUNDS):
    """generator of Store::Push operations from an empty store, applied to the oracle store `so` before they are yielded:
    ("count", keys, vals, None, marks) and ("grad", keys, ragged vals, lens | None, marks).  marks: {name: keys} of the designed
    rows in the operation just applied (asserted by check_marks on whatever store replays them).

    Round 0 designs keys that are new (w = 0, z = 0): gw = -+l1 puts z exactly on +-l1 (w stays 0, no V), gw one representable
    step larger in magnitude puts it one step outside (w leaves 0; V appears iff fea_cnt > V_threshold: the count push gave
    these keys V_threshold or V_threshold + 1).  Rounds 1 and 2 take keys with w != 0 and search a gradient that brings z back
    exactly onto +-l1 (w becomes 0, V kept), and choose counts that land V-less keys with w != 0 on V_threshold and on
    V_threshold + 1 at count-push time.

    (What these rows can and cannot show: with z exactly on +-l1 the other branch of the comparison, (z -+ l1) / eta, is +0 as
    well, so "<=" against "<" at |z| <= l1 leaves the same bits by arithmetic; the rows hold the landing itself, the sign
    of the zero, that no V appears, and one step outside that w leaves zero by the smallest amount.)"""
    from oracle import bindings as ob
    thr = kw["V_threshold"]
    keys = np.unique(rng.integers(1, 2 ** 63, size=nkeys + 64, dtype=np.uint64))[:nkeys]
    keys = keys[rng.permutation(nkeys)]          # push order is not key order
    designed = keys[:16]
    for rnd in range(rounds):
        part = keys if rnd == 0 else keys[rng.random(nkeys) < 0.8]
        # ---- Push(kFeaCount)
        cnt = rng.integers(1, 5, len(part)).astype(np.float32)
        marks = {}
        if rnd == 0:
            cnt[:16] = [thr, thr + 1] * 8
        else:
            # V-less keys with w != 0: land the stored count on the threshold (no V) and one beyond it (V appears)
            cand = []
            for i, key in enumerate(part):
                e = so.peek(int(key))
                if e["w"] != 0 and e["V"] is None and e["fea_cnt"] < thr:
                    cand.append(i)
            assert len(cand) >= 4, "the design lost its V-less keys with w != 0 below the threshold"
            on, beyond = cand[0:2], cand[2:4]
            for i in on:
                cnt[i] = thr - so.peek(int(part[i]))["fea_cnt"]
            for i in beyond:
                cnt[i] = thr + 1 - so.peek(int(part[i]))["fea_cnt"]
            marks = dict(count_on=part[on], count_beyond=part[beyond])
        so.push(part, ob.FEA_COUNT, cnt)
        yield "count", part, cnt, None, marks
        # ---- Push(kGradient)
        vals, lens = so.pull(part)
        lens = lens if V_dim else np.ones(len(part), np.int32)
        gw = _random_grad(rng, len(part))
        gw[rng.random(len(part)) < 0.2] = 0.0
        marks = {}
        if rnd == 0:
            gw[:16] = np.repeat(np.array([-L1, L1, -OUT, OUT], np.float32), 2).tolist() * 2
            d = designed.reshape(2, 4, 2)     # [copy, landing, count on / beyond]
            marks = dict(on_l1=d[:, :2].reshape(-1), outside_at_thr=d[:, 2:, 0].reshape(-1), outside_beyond_thr=d[:, 2:, 1].reshape(-1))
        else:
            found = {L1: [], -L1: []}
            for i, key in enumerate(part):
                e = so.peek(int(key))
                if e["w"] == 0 or (V_dim and e["V"] is None):
                    continue
                t = L1 if len(found[L1]) <= len(found[-L1]) else -L1
                g = _land_z(e, t, kw)
                if g is not None and np.isfinite(g):
                    gw[i] = g
                    found[t].append(i)
                if min(len(found[L1]), len(found[-L1])) >= 2:
                    break
            assert min(len(found[L1]), len(found[-L1])) >= 2, "no gradient found that lands z on +-l1"
            marks = dict(back_on_plus=part[found[L1]], back_on_minus=part[found[-L1]])
        pos = np.concatenate([[0], np.cumsum(lens)[:-1]])
        grad = _random_grad(rng, int(lens.sum()))
        grad[pos] = gw
        so.push(part, ob.GRADIENT, grad, lens if V_dim else None)
        yield "grad", part, grad, (lens if V_dim else None), marks


def check_marks(marks, peek, V_dim, kw, hash_value=None):
    """the designed rows did what they were designed to do, on the store whose entries `peek(key)` returns"""
    thr = kw["V_threshold"]
    for name, keys in marks.items():
        for key in keys:
            e = peek(int(key))
            new_V = None
            if name == "on_l1":
                assert abs(e["z"]) == L1 and e["w"] == 0 and e["V"] is None, (name, e)
            elif name == "outside_at_thr":
                assert abs(e["z"]) == OUT and e["w"] != 0 and e["fea_cnt"] == thr and e["V"] is None, (name, e)
            elif name == "outside_beyond_thr":
                assert abs(e["z"]) == OUT and e["w"] != 0 and e["fea_cnt"] == thr + 1 and (e["V"] is not None) == (V_dim > 0), (name, e)
                new_V = e["V"]
            elif name in ("back_on_plus", "back_on_minus"):
                assert e["z"] == (L1 if name == "back_on_plus" else -L1) and e["w"] == 0 and (e["V"] is not None) == (V_dim > 0), (name, e)
            elif name == "count_on":
                assert e["fea_cnt"] == thr and e["w"] != 0 and e["V"] is None, (name, e)
            elif name == "count_beyond":
                assert e["fea_cnt"] == thr + 1 and e["w"] != 0 and (e["V"] is not None) == (V_dim > 0), (name, e)
                new_V = e["V"]
            if new_V is not None:   # a fresh row: zero accumulators; in hash mode the values of orc_hash_init_value
                assert not bits(new_V[V_dim:]).any(), (name, "accumulators of a new row")
                if hash_value is not None:
                    want = np.array([hash_value(int(key), j) for j in range(V_dim)], np.float32)
                    same_bits(new_V[:V_dim], want, "%s: new V row of key %d" % (name, key))


def _device_peek(model):
    keys, scal, has, V = model

    def peek(key):
        i = int(np.searchsorted(keys, np.uint64(key)))
        assert keys[i] == key
        return dict(fea_cnt=scal[i, 0], w=scal[i, 1], sqrt_g=scal[i, 2], z=scal[i, 3], V=V[i] if has[i] else None)
    return peek


def _modes():
    from oracle import bindings as ob
    return {"hash": ob.INIT_HASH, "refrand": ob.INIT_REFRAND}


@pytest.mark.parametrize("V_dim", [0, 1, 4, 5, 64])
@pytest.mark.parametrize("mode", ["hash", "refrand"])
def test_raw_ops_designed_rows_on_the_oracle(oracle, V_dim, mode):
    """CPU: the raw-push operations the GPU tests replay hold their designed rows (z on +-l1 and one step outside, counts on
    and beyond the threshold), judged on the oracle's own state"""
    so = oracle.store_create(init_mode=_modes()[mode], V_dim=V_dim, **RAW_KW)
    seen = set()
    hv = (lambda key, j: oracle.L.orc_hash_init_value(key, j, RAW_KW["seed"], RAW_KW["V_init_scale"])) if mode == "hash" else None
    for kind, keys, vals, lens, marks in raw_ops(so, V_dim, np.random.default_rng(40 + V_dim), nkeys=600):
        check_marks(marks, so.peek, V_dim, RAW_KW, hv)
        seen |= set(marks)
    assert seen == {"on_l1", "outside_at_thr", "outside_beyond_thr", "back_on_plus", "back_on_minus", "count_on", "count_beyond"}


@pytest.mark.parametrize("V_dim", [0, 1, 4, 5, 64, 100])
def test_raw_pushes_oracle_vs_reference_updater(oracle, V_dim):
    """CPU: the same operations through the reference's own SGDUpdater (its rand_r init) and through the C oracle in REFRAND
    mode: every pulled value and length bit-identical after every push.  (If they differ the oracle is wrong.)"""
    from oracle import bindings as ob
    if not ob.have_ref():
        pytest.skip("oracle/_ref not built (needs the reference's sources)")
    kw = dict(RAW_KW, V_dim=V_dim)
    so = oracle.store_create(init_mode=ob.INIT_REFRAND, **kw)
    rs = ob.Ref().store_create(**kw)
    pushed = np.zeros(0, np.uint64)
    for kind, keys, vals, lens, _ in raw_ops(so, V_dim, np.random.default_rng(40 + V_dim), nkeys=600):
        rs.push(keys, ob.FEA_COUNT if kind == "count" else ob.GRADIENT, vals, lens)
        pushed = np.union1d(pushed, keys)
        vo, lo = so.pull(pushed)
        vr, lr = rs.pull(pushed)
        assert np.array_equal(lo, lr), kind
        same_bits(vr, vo, "pulled values after a %s push" % kind)
        assert V_dim == 0 or (lo > 1).any() or kind == "count"


@pytest.mark.gpu
@pytest.mark.parametrize("V_dim", [0, 1, 4, 5, 64, 100, 256])
@pytest.mark.parametrize("mode", ["hash", "refrand"])
def test_raw_pushes_bit_exact(capi, ctx, oracle, V_dim, mode):
    """Table.push (k_push_count / k_push_grad): three rounds of count push then gradient push over 2 000 keys; after every
    push the whole export equals the oracle's entries as bit patterns, and the designed rows did what they were designed for"""
    from oracle import bindings as ob
    so = oracle.store_create(init_mode=_modes()[mode], V_dim=V_dim, **RAW_KW)
    tb = capi.Table(ctx, 4096, V_dim=V_dim, init_mode=capi.INIT_HASH if mode == "hash" else capi.INIT_REFRAND, **RAW_KW)
    hv = (lambda key, j: oracle.L.orc_hash_init_value(key, j, RAW_KW["seed"], RAW_KW["V_init_scale"])) if mode == "hash" else None
    pushed = np.zeros(0, np.uint64)
    try:
        for step, (kind, keys, vals, lens, marks) in enumerate(raw_ops(so, V_dim, np.random.default_rng(40 + V_dim))):
            tb.push(keys, capi.FEA_COUNT if kind == "count" else capi.GRADIENT, vals, lens)
            tb.check()
            pushed = np.union1d(pushed, keys)
            model = assert_model_equals_oracle(tb, so, V_dim, "%s push %d" % (kind, step), nkeys=len(pushed))
            check_marks(marks, _device_peek(model), V_dim, RAW_KW, hv)
        assert V_dim == 0 or 50 < model[2].sum() < len(pushed)
    finally:
        tb.close()


class _Dev:
    """device arrays of one step of the owner-side forms"""

    def __init__(self, capi, ctx):
        self.capi, self.ctx, self.bufs = capi, ctx, []

    def put(self, arr):
        b = self.capi.DeviceBuffer.from_numpy(self.ctx, arr)
        self.bufs.append(b)
        return b

    def zeros(self, nbytes):
        return self.put(np.zeros(max(nbytes, 16), np.uint8))

    def close(self):
        for b in self.bufs:
            b.close()
        self.bufs = []


def _owner_step(capi, ctx, tb, form, srcs, cnts, grad_rows_of, stride):
    """one step of the owner side in the given form: count push of every source (cnts, or None), pull, gradient push.
    grad_rows_of(flags [n]) -> the gradient rows [n, stride] for the has_V flags as pulled.  Returns (pulled rows, grads)"""
    seg = np.concatenate([[0], np.cumsum([len(x) for x in srcs])]).astype(np.int64)
    n, G = int(seg[-1]), len(srcs)
    D = _Dev(capi, ctx)
    try:
        keys = D.put(np.concatenate(srcs).astype(np.uint64))
        cnt = D.put(np.concatenate(cnts).astype(np.float32)) if cnts is not None else None
        rows = D.zeros(n * stride * 4)
        rowid = D.zeros(4 * max(capi.multi_words(n, G), n, 1))
        spans = [(int(seg[s]), int(seg[s + 1])) for s in range(G) if seg[s + 1] > seg[s]]
        if form in ("multi", "listed"):
            tb.shard_resolve_multi(keys.ptr, seg, rowid.ptr)
        elif form == "resolved":
            tb.shard_resolve(keys.ptr, n, rowid.ptr)
        if cnt is not None:
            if form == "multi":
                tb.shard_push_count_multi(rowid.ptr, keys.ptr, seg, cnt.ptr)
            for a, b in spans:
                if form == "plain":
                    tb.shard_push_count(keys.at(8 * a), b - a, cnt.at(4 * a))
                elif form == "resolved":
                    tb.shard_push_count_resolved(rowid.at(4 * a), keys.at(8 * a), b - a, cnt.at(4 * a))
        if form == "listed":
            tb.shard_count_pull_multi(rowid.ptr, keys.ptr, seg, cnt.ptr if cnt is not None else None, rows.ptr)
        elif form == "plain":
            for a, b in spans:
                tb.shard_pull(keys.at(8 * a), b - a, rows.at(4 * stride * a))
        else:
            tb.shard_pull_resolved(rowid.ptr, n, rows.ptr)
        ctx.sync()
        pulled = rows.to_numpy(np.float32, n * stride).reshape(n, stride)
        g = grad_rows_of(pulled[:, 1])
        grads = D.put(g)
        if form == "multi":
            tb.shard_push_grad_multi(rowid.ptr, keys.ptr, seg, grads.ptr)
        elif form == "listed":
            tb.shard_push_grad_listed(rowid.ptr, keys.ptr, seg, grads.ptr)
        else:
            for a, b in spans:
                if form == "plain":
                    tb.shard_push_grad(keys.at(8 * a), b - a, grads.at(4 * stride * a))
                else:
                    tb.shard_push_grad_resolved(rowid.at(4 * a), keys.at(8 * a), b - a, grads.at(4 * stride * a))
        ctx.sync()
        tb.check()
        return pulled, g
    finally:
        D.close()


def _rows_from_ragged(vals, lens, flags, V_dim, stride):
    """Store::Push(kGradient) layout -> gradient rows [gw, has_V as pulled, 0, 0 | gV]"""
    n = len(flags)
    g = np.zeros((n, stride), np.float32)
    g[:, 1] = flags
    if V_dim == 0 or n == 0:
        g[:, 0] = vals
        return g
    pos = np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.int64)
    g[:, 0] = vals[pos]
    for i in np.flatnonzero(lens > 1):
        g[i, 4:4 + V_dim] = vals[pos[i] + 1:pos[i] + 1 + V_dim]
    return g


@pytest.mark.gpu
@pytest.mark.parametrize("V_dim", [0, 5, 64])
@pytest.mark.parametrize("form,mode", [("plain", "hash"), ("plain", "refrand"), ("resolved", "hash"), ("multi", "hash"), ("listed", "hash")])
def test_owner_side_forms_one_source_bit_exact(capi, ctx, oracle, V_dim, mode, form):
    """the operations of test_raw_pushes_bit_exact, designed rows included, through the owner-side entry points with ONE
    source: shard_push_count / shard_pull / shard_push_grad and their resolved, multi and listed forms (which take the
    order-independent hash init only: the REFRAND chain runs through the plain form)"""
    so = oracle.store_create(init_mode=_modes()[mode], V_dim=V_dim, **RAW_KW)
    tb = capi.Table(ctx, 4096, V_dim=V_dim, init_mode=capi.INIT_HASH if mode == "hash" else capi.INIT_REFRAND, **RAW_KW)
    hv = (lambda key, j: oracle.L.orc_hash_init_value(key, j, RAW_KW["seed"], RAW_KW["V_init_scale"])) if mode == "hash" else None
    stride = capi.row_stride(V_dim)
    ops = raw_ops(so, V_dim, np.random.default_rng(40 + V_dim), nkeys=1200)
    pushed = np.zeros(0, np.uint64)
    try:
        for rnd in range(RAW_ROUNDS):
            # the oracle has to stand one operation back while the device does count push + pull + gradient push: it is
            # advanced by the generator, so the count push is compared through a second store that stops after it
            kind, keys, cnt, _, cmarks = next(ops)
            assert kind == "count"
            after_count = oracle_model(so, np.sort(np.union1d(pushed, keys)), V_dim)
            kind, keys2, vals, lens, gmarks = next(ops)
            assert kind == "grad" and np.array_equal(keys, keys2)
            lens_ = lens if V_dim else np.ones(len(keys), np.int32)
            seen = {}

            def grad_rows_of(flags):
                # between the count push and the gradient push: the device's table against the oracle's state after the count push
                dk, dscal, dhas, dV = device_model(tb)
                seen["model"] = (dk, dscal, dhas, dV)
                assert np.array_equal(dk, np.sort(np.union1d(pushed, keys)))
                same_bits(dscal, after_count[0], "after the count push: scalars")
                assert np.array_equal(dhas != 0, after_count[1] != 0)
                same_bits(dV, after_count[2], "after the count push: V")
                assert np.array_equal(flags != 0, lens_ > 1), "has_V as pulled"
                return _rows_from_ragged(vals, lens_, flags, V_dim, stride)

            _owner_step(capi, ctx, tb, form, [keys], [cnt], grad_rows_of, stride)
            check_marks(cmarks, _device_peek(seen["model"]), V_dim, RAW_KW, hv)
            pushed = np.union1d(pushed, keys)
            model = assert_model_equals_oracle(tb, so, V_dim, "%s, round %d" % (form, rnd), nkeys=len(pushed))
            check_marks(gmarks, _device_peek(model), V_dim, RAW_KW, hv)
    finally:
        tb.close()


# G = 9: a key of all sources has m = 8 other entries (XS = 8), the one m at which the per-entry push leaves its register path
# while the per-key count + pull still takes its own; G = 5: m = 4 = XS, the second read of four extras is masked.
_SEVERAL_FORMS = [("plain", 3, "hash"), ("plain", 3, "refrand"), ("resolved", 3, "hash"), ("multi", 3, "hash"), ("listed", 3, "hash"),
                  ("multi", 11, "hash"), ("listed", 11, "hash"), ("multi", 9, "hash"), ("listed", 9, "hash"), ("multi", 5, "hash"),
                  ("listed", 5, "hash")]
# V_dim 0, 5, 64: lane groups of 1, 2, 16 that all lie inside the row.  9 (kp = 12, 4 lanes: lane 3 beyond the row, lane 2 with a
# tail of three zeroed elements) and 100 (32 lanes, 25 - 31 beyond the row): lanes beyond a non-empty row, in the lane-group forms
_SEVERAL_CASES = ([(f, G, m, V) for f, G, m in _SEVERAL_FORMS for V in (0, 5, 64)]
                  + [(f, 3, "hash", V) for f in ("resolved", "multi", "listed") for V in (9, 100)])


@pytest.mark.gpu
@pytest.mark.parametrize("form,G,mode,V_dim", _SEVERAL_CASES)
def test_owner_side_forms_several_sources_bit_exact(capi, ctx, oracle, V_dim, mode, form, G):
    """several sources carrying the same keys in one step: the result equals the oracle's pushes applied in source order
    (each source's gradient with the has_V flags as pulled at the start of the step), by full export, bit for bit"""
    from oracle import bindings as ob
    rng = np.random.default_rng(300 + V_dim + G)
    so = oracle.store_create(init_mode=_modes()[mode], V_dim=V_dim, **RAW_KW)
    tb = capi.Table(ctx, 4096, V_dim=V_dim, init_mode=capi.INIT_HASH if mode == "hash" else capi.INIT_REFRAND, **RAW_KW)
    stride = capi.row_stride(V_dim)
    universe = np.unique(rng.integers(1, 2 ** 63, size=900, dtype=np.uint64))
    pushed = np.zeros(0, np.uint64)
    try:
        for step in range(4):
            srcs = [np.sort(rng.choice(universe, size=int(rng.integers(150, 500)), replace=False)) for _ in range(G)]
            srcs = [np.union1d(x, universe[step * 5:step * 5 + 4]) for x in srcs]    # keys EVERY source carries
            if step == 2:
                srcs[1] = srcs[1][:0]     # a source with nothing for this owner
            cnts = [rng.integers(1, 4, len(x)).astype(np.float32) for x in srcs]
            with_cnt = step < 3
            if with_cnt:
                for x, c in zip(srcs, cnts):
                    so.push(x, ob.FEA_COUNT, c)
            allk = np.concatenate(srcs)
            lens = []
            for x in srcs:
                _, l = so.pull(x)
                lens.append(l if V_dim else np.ones(len(x), np.int32))
            ragged = []
            for x, l in zip(srcs, lens):
                v = _random_grad(rng, int(l.sum()))
                pos = np.concatenate([[0], np.cumsum(l)[:-1]]).astype(np.int64)
                if len(x):
                    v[pos[rng.random(len(x)) < 0.2]] = 0.0
                ragged.append(v)

            def grad_rows_of(flags):
                assert np.array_equal(flags != 0, np.concatenate(lens) > 1), "has_V as pulled"
                out, a = [], 0
                for x, l, v in zip(srcs, lens, ragged):
                    out.append(_rows_from_ragged(v, l, flags[a:a + len(x)], V_dim, stride))
                    a += len(x)
                return np.concatenate(out)

            _owner_step(capi, ctx, tb, form, srcs, cnts if with_cnt else None, grad_rows_of, stride)
            for x, l, v in zip(srcs, lens, ragged):
                if len(x):
                    so.push(x, ob.GRADIENT, v, l if V_dim else None)
            pushed = np.union1d(pushed, allk)
            model = assert_model_equals_oracle(tb, so, V_dim, "%s x %d sources, step %d" % (form, G, step), nkeys=len(pushed))
        assert V_dim == 0 or model[2].sum() > 50
    finally:
        tb.close()


# ================================================================== exact-sum steps
_DESIGNS = {}


def design(lengths, V_dim, binary, push_cnt, variant="base", seed=0):
    key = (tuple(lengths), V_dim, binary, push_cnt, variant, seed)
    if key not in _DESIGNS:
        _DESIGNS[key] = X.build(lengths, V_dim, binary, push_cnt, variant, seed=seed)
    return _DESIGNS[key]


def _poked_store(oracle, D):
    from oracle import bindings as ob
    so = oracle.store_create(init_mode=ob.INIT_HASH, V_dim=D["V_dim"], **D["hyper"])
    for u, key in enumerate(D["keys"]):
        so.poke(int(key), *D["scal"][u], D["V"][u] if D["has_V"][u] else None)
    return so


_EXPECTED = {}


def expected(oracle, D):
    """the one right answer of the design's step: check(D) on the weights the step sees, then oracle poke + (count push +) push
    of the exact gradient -> dict(pred, gw, gV, lens, pulled = the ragged values the step sees, model = (scal, has_V, V) of
    D["keys"])"""
    from oracle import bindings as ob
    if id(D) in _EXPECTED:
        return _EXPECTED[id(D)]
    k = D["V_dim"]
    so = _poked_store(oracle, D)
    if D["push_cnt"]:
        so.push(D["keys"], ob.FEA_COUNT, D["cnt"])
    pulled = so.pull(D["keys"])
    lens = pulled[1] if k else np.ones(len(D["keys"]), np.int32)
    got = X.check(D, pulled, lengths=D["lengths"])
    so.push(D["keys"], ob.GRADIENT, X.ragged_gradient(got["gw"], got["gV"], lens, k), lens if k else None)
    assert so.size() == len(D["keys"])
    out = dict(got, lens=lens, pulled=np.array(pulled[0], np.float32), model=oracle_model(so, D["keys"], k),
               progress=X.exact_progress(D, pulled))
    # what the design promises of the update: keys whose V the update initialises, keys that stay without although w left zero
    scal, has, V = out["model"]
    c = D["cls"]
    if k:
        lazy = (has != 0) & (c == "Z")
        assert lazy.sum() >= 3 and not bits(V[lazy][:, k:]).any()
        left_zero_no_V = (c == "Z") & (scal[:, 1] != 0) & (has == 0)
        assert left_zero_no_V.any() and np.all(scal[left_zero_no_V, 0] <= D["hyper"]["V_threshold"])
        assert (scal[lazy, 0] == D["hyper"]["V_threshold"] + 1).any() and (scal[left_zero_no_V, 0] == D["hyper"]["V_threshold"]).any()
        assert np.array_equal(has != 0, (lens > 1) | lazy)
    _EXPECTED[id(D)] = out
    return out


STEP_VDIMS = [0, 1, 4, 5, 8, 64, 100, 128, 256]
SWITCH_VDIMS = [0, 5, 64]
VARIANT_CASES = [(V_dim, push_cnt, v) for V_dim in SWITCH_VDIMS for push_cnt in (False, True) for v in ("l1_0", "Vl2_0", "beta", "pen")]


@pytest.mark.parametrize("V_dim", STEP_VDIMS)
@pytest.mark.parametrize("binary", [False, True], ids=["valued", "binary"])
@pytest.mark.parametrize("push_cnt", [False, True], ids=["nocnt", "cnt"])
def test_designs_pass_check_and_the_oracle_step_is_the_exact_one(oracle, V_dim, binary, push_cnt):
    """CPU: every design passes check() on the weights its step sees, and the oracle's own sgd_step from the poked model gives
    logits equal to clip(exact) and a model bit-identical to poke + (count push +) push of exact_gradient"""
    _oracle_step_is_exact(oracle, design(X.FULL_LENGTHS, V_dim, binary, push_cnt))


@pytest.mark.parametrize("V_dim,push_cnt,variant", VARIANT_CASES)
def test_variant_designs_pass_check_and_the_oracle_step_is_the_exact_one(oracle, V_dim, push_cnt, variant):
    """CPU: the same for l1 = 0, V_l2 = 0 and non-default lr_beta / V_lr_beta"""
    _oracle_step_is_exact(oracle, design(X.FULL_LENGTHS, V_dim, False, push_cnt, variant))


def _oracle_step_is_exact(oracle, D):
    k = D["V_dim"]
    want = expected(oracle, D)
    loc = oracle.localize(D["offset"], D["index"])
    assert np.array_equal(loc["feaids"], D["keys"]) and np.array_equal(loc["index"], D["cidx"]) and np.array_equal(loc["feacnt"], D["cnt"])
    so = _poked_store(oracle, D)
    pred, _ = so.sgd_step(loc["offset"], loc["index"], D["value"], D["label"], D["keys"], feacnt=D["cnt"] if D["push_cnt"] else None)
    same_bits(pred, want["pred"], "the oracle's logits against clip(exact)")
    scal, has, V = oracle_model(so, D["keys"], k)
    assert np.array_equal(has, want["model"][1])
    same_bits(scal, want["model"][0], "the oracle's step against the push of the exact gradient: scalars")
    same_bits(V, want["model"][2], "the oracle's step against the push of the exact gradient: V | acc")
    assert so.size() == len(D["keys"])


def _device_step(capi, D, path="device", options=(), auc=True, is_train=True):
    """one step of the design from the imported model on a context of its own -> dict(pred, model = (scal, has_V, V),
    split_entries, progress = what progress(reset=True) returned after the step, reads = two progress(reset=False) before it
    and one after it, and for the packed path grads [U, stride], rows_after).  auc: the batch option compute_auc, as the
    learners set it; is_train = False: a validation step"""
    k = D["V_dim"]
    nrows, nnz, U = len(D["label"]), len(D["index"]), len(D["keys"])
    c = capi.Context(0)
    objs = []
    try:
        for name, v in options:
            c.set_option(name, v)
        tb = capi.Table(c, 4096, V_dim=k, init_mode=capi.INIT_HASH, **D["hyper"])
        objs.append(tb)
        tb.import_(D["keys"], D["scal"], D["has_V"], D["V"] if k else None)
        bt = capi.Batch(c, nrows, nnz + 64)
        objs.append(bt)
        if auc:
            bt.set_option("compute_auc", 1)
        out = {}
        if path == "host_localized":
            bt.load_localized_host(D["offset"], D["cidx"], D["value"], D["label"], D["keys"], D["cnt"] if D["push_cnt"] else None)
        else:
            bt.load_host(D["offset"], D["index"], D["value"], D["label"])
            bt.localize()
        if path == "packed":
            stride = capi.row_stride(k)
            d_rows = capi.DeviceBuffer(c, nnz * stride * 4)
            d_grads = capi.DeviceBuffer(c, nnz * stride * 4)
            objs += [d_rows, d_grads]
            d_keys, d_cnt, U_dev = bt.device_keys()
            assert U_dev == U
            if D["push_cnt"]:
                tb.shard_push_count(d_keys, U, d_cnt)
            tb.shard_pull(d_keys, U, d_rows.ptr)
            bt.forward(k, d_rows.ptr)
            bt.backward(k, d_rows.ptr, d_grads.ptr)
            c.sync()
            out["rows"] = d_rows.to_numpy(np.float32, U * stride).reshape(U, stride)
            out["grads"] = d_grads.to_numpy(np.float32, U * stride).reshape(U, stride)
            tb.shard_push_grad(d_keys, U, d_grads.ptr)
            tb.shard_pull(d_keys, U, d_rows.ptr)
            c.sync()
            out["rows_after"] = d_rows.to_numpy(np.float32, U * stride).reshape(U, stride)
        else:
            bt.sgd_step(tb, is_train=is_train, push_cnt=D["push_cnt"] and is_train)    # (a validation step pushes no counts)
        reads = [bt.progress(reset=False), bt.progress(reset=False)]
        out["progress"] = bt.progress(reset=True)
        out["reads"] = reads + [bt.progress(reset=False)]
        out["pred"] = bt.pred()
        out["split_entries"] = bt.split_entries()
        tb.check()
        keys, scal, has, V = device_model(tb)
        assert np.array_equal(keys, D["keys"]), "the step added or lost keys"
        out["model"] = (scal, has, V)
        return out
    finally:
        for o in objs[::-1]:
            o.close()
        c.close()


PROGRESS_FIELDS = ("loss", "penalty", "auc", "nnz_w", "nrows")


def progress_bits(p):
    return tuple(X.f32bits(getattr(p, f)) for f in PROGRESS_FIELDS)


def assert_reads(got, what):
    """reading does not change the sums (two reads without reset and the one with it: the same bits); after the reset: zeros"""
    a, b, z = got["reads"]
    assert progress_bits(a) == progress_bits(b) == progress_bits(got["progress"]), "%s: two reads of the progress differ" % what
    assert progress_bits(z) == (0, 0, 0, 0, 0), "%s: the progress after its reset: %r" % (what, progress_bits(z))


def assert_step_progress(got, P, what, auc=True, penalty=True):
    """the step's Progress against the design's one right answer P (X.exact_progress).  auc = False: a batch without
    compute_auc leaves the AUC at +0; penalty = False: a path that counts none (Batch.forward / Batch.backward) leaves +0"""
    P = dict(P)
    if not auc:
        P["auc"] = 0.0
    if not penalty:
        P["penalty"] = dict(exact=0.0, err=0.0)
    X.assert_progress(got["progress"], X.accepted([P]), what)
    assert_reads(got, what)


def _assert_step(got, want, D, what, split=True, auc=True, penalty=True):
    assert_step_progress(got, want["progress"], what, auc=auc, penalty=penalty)
    same_bits(got["pred"], want["pred"], "%s: logits against clip(exact)" % what)
    _assert_model(got["model"], want["model"], D, what)
    if split is not None:
        assert got["split_entries"] == (split_entries_expected(D["cnt"]) if split else 0), what
    if split:
        assert got["split_entries"] == 5 + 6      # 4 097 and 5 121 occurrences; 4 096 stays whole


def _assert_model(model, wmodel, D, what):
    k = D["V_dim"]
    scal, has, V = model
    wscal, whas, wV = wmodel
    assert np.array_equal(has != 0, whas != 0), "%s: has_V differs at keys of %r occurrences" % (what, D["cnt"][(has != 0) != (whas != 0)][:8])
    for j, name in enumerate(("fea_cnt", "w", "sqrt_g", "z")):
        bad = bits(scal[:, j]) != bits(wscal[:, j])
        assert not bad.any(), "%s: %s differs at %d keys; their occurrences %r, classes %r; first got %r want %r" % (
            what, name, bad.sum(), np.unique(D["cnt"][bad]).astype(int).tolist(), np.unique(D["cls"][bad]).tolist(), scal[bad, j][0], wscal[bad, j][0])
    if k:
        for name, a, b in (("V", V[:, :k], wV[:, :k]), ("accumulators", V[:, k:], wV[:, k:])):
            bad = (bits(a) != bits(b)).any(1)
            assert not bad.any(), "%s: %s differ at %d keys; their occurrences %r, classes %r" % (
                what, name, bad.sum(), np.unique(D["cnt"][bad]).astype(int).tolist(), np.unique(D["cls"][bad]).tolist())


@pytest.mark.gpu
@pytest.mark.parametrize("V_dim", STEP_VDIMS)
@pytest.mark.parametrize("binary", [False, True], ids=["valued", "binary"])
@pytest.mark.parametrize("push_cnt", [False, True], ids=["nocnt", "cnt"])
def test_exact_step_default_path(capi, oracle, V_dim, binary, push_cnt):
    """the default step (device Localizer, k_update_fused with the split role): every L, both EXACT values and both HAS_VAL
    values of k_update_fused<..., false>; logits equal clip(exact), every field of every key equals the oracle's push of the
    exact gradient as bit patterns, new hash-initialised rows included"""
    D = design(X.FULL_LENGTHS, V_dim, binary, push_cnt)
    _assert_step(_device_step(capi, D), expected(oracle, D), D, "default path")


@pytest.mark.gpu
@pytest.mark.parametrize("V_dim,push_cnt,variant", VARIANT_CASES)
def test_exact_step_hyper_parameter_variants(capi, oracle, V_dim, push_cnt, variant):
    """l1 = 0, V_l2 = 0 and non-default lr_beta / V_lr_beta through the default step"""
    D = design(X.FULL_LENGTHS, V_dim, False, push_cnt, variant)
    _assert_step(_device_step(capi, D), expected(oracle, D), D, "default path, %s" % variant)


SWITCHES = {
    "host_localized": dict(path="host_localized"),                       # k_seg_lists
    "upd_split0": dict(options=(("upd_split", 0),), split=False),        # the hot role walks the long keys whole
    "upd_kernel0": dict(options=(("upd_kernel", 0),), split=False),      # k_backward_all fused
    "hot_blocks1": dict(options=(("upd_hot_blocks", 1),)),
    "hot_blocks8": dict(options=(("upd_hot_blocks", 8),)),
    "single_queue": dict(options=(("single_queue", 1),)),
}


# the routes of the minibatch's AUC into the progress block: riding in the update launch (the default), a launch of its own
# behind the forward, and a batch that computes none
AUC_ROUTES = {
    "auc_in_update0": dict(options=(("auc_in_update", 0),)),
    "no_auc": dict(auc=False),
}
PEN_VDIMS = [0, 1, 5, 64, 256]
PEN_CASES = [(V_dim, push_cnt) for V_dim in PEN_VDIMS for push_cnt in (False, True)]
# the l2 copy's total is small (an ulp of 5e-7): a C key's 24-bit V would put a rounding boundary inside the accepted interval,
# so the copies that carry V are those without a count push (the l2 term is w's alone)
L2_CASES = [(0, False), (0, True), (5, False), (64, False)]


_VALIDATION = {}


def validation_progress(D):
    """the one right Progress of a validation step on the design's own model (no count push: a C key is still without V)"""
    if id(D) not in _VALIDATION:
        _VALIDATION[id(D)] = X.exact_progress(D)
    return _VALIDATION[id(D)]


def _assert_validation(got, D, what):
    """a validation step: clip(exact) logits, loss and AUC of these, the penalty (k_penalty) of the model as imported, and the
    model bit-identical to the import"""
    same_bits(got["pred"], X.exact_pred(D), "%s: logits against clip(exact)" % what)
    assert_step_progress(got, validation_progress(D), what)
    scal, has, V = got["model"]
    same_bits(scal, D["scal"], "%s: scalars against the import" % what)
    assert np.array_equal(has != 0, D["has_V"] != 0), what
    if D["V_dim"]:
        same_bits(V, D["V"], "%s: V | acc against the import" % what)


def _switch_matrix(capi, oracle, D):
    want = expected(oracle, D)
    k = D["V_dim"]
    runs = {"default": _device_step(capi, D)}
    for name, sw in list(SWITCHES.items()) + list(AUC_ROUTES.items()):
        runs[name] = _device_step(capi, D, path=sw.get("path", "device"), options=sw.get("options", ()), auc=sw.get("auc", True))
    runs["packed"] = _device_step(capi, D, path="packed")
    # -- all of them one and the same model and the same logits
    base = runs["default"]
    for name, r in runs.items():
        same_bits(r["pred"], base["pred"], "%s against the default path: logits" % name)
        assert np.array_equal(r["model"][1], base["model"][1]), name
        same_bits(r["model"][0], base["model"][0], "%s against the default path: scalars" % name)
        same_bits(r["model"][2], base["model"][2], "%s against the default path: V | acc" % name)
    # -- each against the oracle; the progress sums: the packed path's forward leaves the loss and counts the rows, nothing
    # there computes an AUC, and backward<false> without the penalty bit counts no penalty: exactly +0
    for name, r in runs.items():
        _assert_step(r, want, D, name, split=None if name == "packed" else SWITCHES.get(name, {}).get("split", True),
                     auc=name not in ("packed", "no_auc"), penalty=name != "packed")
    # -- the packed path's gradient rows: [gw, has_V as pulled, 0, 0 | gV], padded coordinates zero
    p = runs["packed"]
    stride = p["grads"].shape[1]
    assert np.array_equal(p["rows"][:, 1] != 0, want["lens"] > 1)
    g = np.zeros((len(D["keys"]), stride), np.float32)
    g[:, 0] = want["gw"]
    g[:, 1] = p["rows"][:, 1]
    if k:
        g[:, 4:4 + k] = want["gV"]
    same_bits(p["grads"], g, "gradient rows of the packed path against exact_gradient")
    # -- padded coordinates (k <= d < kp) of the rows pulled after the step stay zero
    assert not bits(p["rows_after"][:, 4 + k:]).any() and not bits(p["rows_after"][:, 2:4]).any()
    same_bits(p["rows_after"][:, 0], want["model"][0][:, 1], "w as pulled after the step")
    # -- a validation step on the same design
    _assert_validation(_device_step(capi, D, is_train=False), D, "validation step")


@pytest.mark.gpu
@pytest.mark.parametrize("V_dim", SWITCH_VDIMS)
@pytest.mark.parametrize("push_cnt", [False, True], ids=["nocnt", "cnt"])
def test_exact_step_every_switch_gives_one_model(capi, oracle, V_dim, push_cnt):
    """the other ways through the step — host-localized load (k_seg_lists), upd_split = 0, upd_kernel = 0 (k_backward_all),
    upd_hot_blocks = 1 and 8, single_queue = 1, auc_in_update = 0, a batch without compute_auc, and the packed path
    shard_pull -> Batch.forward -> Batch.backward -> shard_push_grad — each against the oracle, and all of them one and the
    same model as the default path; loss, AUC and row count of every one of them, and of a validation step, against
    exact_progress (the penalty of these hyper-parameters is on no grid: the next test)"""
    _switch_matrix(capi, oracle, design(X.FULL_LENGTHS, V_dim, False, push_cnt))


# ================================================================== the progress sums
@pytest.mark.parametrize("V_dim", STEP_VDIMS)
@pytest.mark.parametrize("binary", [False, True], ids=["valued", "binary"])
@pytest.mark.parametrize("push_cnt", [False, True], ids=["nocnt", "cnt"])
def test_loss_sums_are_exact_and_every_row_shows(oracle, V_dim, binary, push_cnt):
    """CPU: for every design the GPU tests step, training (the weights after the count push) and validation (the model as
    imported): the loss terms are on one grid and their double sum is exact in any order, one row of a class dropped or counted
    twice changes the float, and the three candidates of log1pf(1.0f) give the accepted floats (exact_step_design.loss_of).  At
    V_dim = 0 the zero rows are below the float's resolution (the total is about 2e7): their term is pinned by the V_dim > 0
    designs — the forward's loss code does not depend on V_dim"""
    D = design(X.FULL_LENGTHS, V_dim, binary, push_cnt)
    for P in (expected(oracle, D)["progress"], validation_progress(D)):
        acc = X.accepted([P])
        assert P["nrows"] == len(D["label"]) and 1 <= len(acc["loss"]) <= 3 and acc["auc"] != 0
        assert P["penalty"] is None       # l1 = 0.02, V_l2 = 0.02: no grid; the "pen" designs pin the penalty
        if V_dim:
            nz = int((D["row_class"] == "z").sum())
            assert P["loss"][1] == 20.0 * int((D["row_class"] == "s").sum()) + nz * float(X.LN2)


@pytest.mark.parametrize("V_dim,push_cnt", PEN_CASES)
def test_penalty_sums_are_exact_and_every_key_shows(oracle, V_dim, push_cnt):
    """CPU: the "pen" designs (l1 = 2^-6, l2 = 0, V_l2 = 2^-5) pass check() like the others, and exact_step_design.penalty_of
    holds on the weights their training step and their validation step see: every term on one grid with fewer than 2^24 grid
    steps in all (exact in any grouping of fp32 partials), a key's non-zero term at least 2 ulp of the float total, the C
    keys' interval below half the smallest term.  The keys with w = 0 and no V have penalty 0: inherently invisible"""
    D = design(X.FULL_LENGTHS, V_dim, False, push_cnt, "pen")
    want = expected(oracle, D)
    for P in (want["progress"], validation_progress(D)):
        pen = P["penalty"]
        assert pen is not None and pen["exact"] > 0 and pen["zero_keys"] == int(((D["cls"] == "Z") | (D["scal"][:, 1] == 0)).sum())
        assert 1 <= len(X.accepted([P])["penalty"]) <= 3
    train, valid = want["progress"]["penalty"], validation_progress(D)["penalty"]
    if V_dim and push_cnt:      # the C keys' V is in the training step's penalty only
        assert train["err"] > 0 and valid["err"] == 0 and train["exact"] > valid["exact"]
    else:
        assert train["err"] == 0 and train["exact"] == valid["exact"]


def _l2_pulled(oracle, C, train):
    """the weights a step of the l2 copy sees: its own model, after the count push where the training step makes one"""
    from oracle import bindings as ob
    if not (train and C["push_cnt"]):
        return None
    so = _poked_store(oracle, C)
    so.push(C["keys"], ob.FEA_COUNT, C["cnt"])
    return so.pull(C["keys"])


@pytest.mark.parametrize("V_dim,push_cnt", L2_CASES)
def test_l2_copy_penalty_is_exact_and_every_key_shows(oracle, V_dim, push_cnt):
    """CPU: on the copy with the drivers at +-2 and l2 = 2^-3 penalty_of's conditions hold with the l2 term in the sum"""
    C = X.l2_copy(design(X.FULL_LENGTHS, V_dim, False, push_cnt, "pen"))
    for train in (True, False):
        pen = X.penalty_of(C, _l2_pulled(oracle, C, train))
        w = C["scal"][:, 1].astype(np.float64)
        assert pen is not None and pen["exact"] > float(np.sum(2.0 ** -6 * np.abs(w))) and np.abs(w).max() == 2.0


@pytest.mark.gpu
@pytest.mark.parametrize("V_dim,push_cnt", PEN_CASES)
def test_exact_step_penalty_default_path(capi, oracle, V_dim, push_cnt):
    """the "pen" design through the default step and a validation step: everything test_exact_step_default_path asserts, and
    the penalty sum (upd_apply's fp32 lane partials through upd_flush_penalty; k_penalty) as bit patterns"""
    D = design(X.FULL_LENGTHS, V_dim, False, push_cnt, "pen")
    _assert_step(_device_step(capi, D), expected(oracle, D), D, "default path, pen")
    _assert_validation(_device_step(capi, D, is_train=False), D, "validation step, pen")


@pytest.mark.gpu
@pytest.mark.parametrize("V_dim", SWITCH_VDIMS)
@pytest.mark.parametrize("push_cnt", [False, True], ids=["nocnt", "cnt"])
def test_exact_step_every_switch_gives_one_penalty(capi, oracle, V_dim, push_cnt):
    """the switch matrix on the "pen" design: the penalty of upd_apply in every role (upd_split = 0: the hot role takes the
    long keys), of finish_key and small_role_lean (upd_kernel = 0), under upd_hot_blocks = 1 and 8, the single queue and both
    AUC routes: one float; the packed path: +0"""
    _switch_matrix(capi, oracle, design(X.FULL_LENGTHS, V_dim, False, push_cnt, "pen"))


@pytest.mark.gpu
@pytest.mark.parametrize("V_dim,push_cnt", L2_CASES)
def test_l2_penalty_term_on_the_driverless_copy(capi, oracle, V_dim, push_cnt):
    """0.5 l2 w^2 in the penalty of upd_apply, finish_key (upd_kernel = 0) and k_penalty (a validation step): only penalty and
    nrows are asserted on the copy — its rows are in no class, so its loss, logits and model have no one right answer"""
    C = X.l2_copy(design(X.FULL_LENGTHS, V_dim, False, push_cnt, "pen"))
    for name, kw, train in (("default", {}, True), ("upd_kernel0", dict(options=(("upd_kernel", 0),)), True), ("validation", dict(is_train=False), False)):
        P = X.exact_progress(C, _l2_pulled(oracle, C, train), loss=False)
        got = _device_step(capi, C, **kw)
        X.assert_progress(got["progress"], X.accepted([P]), "l2 copy, %s" % name)
        assert_reads(got, "l2 copy, %s" % name)


def _two_minibatches_one_batch_object(capi, A, B, read_between, options=()):
    """the designs A and B (disjoint keys, one set of hyper-parameters) imported into one table and stepped one after the
    other through ONE batch object -> dict(between = progress(reset=False) after A's step | None, progress = progress(reset=True)
    after B's, after = a read behind it, model = (keys, scal, has_V, V)).  Without the read between the steps B's lookup takes up
    the AUC slots A's update launch left pending"""
    k = A["V_dim"]
    assert B["V_dim"] == k and A["hyper"] == B["hyper"] and not np.isin(A["keys"], B["keys"]).any()
    c = capi.Context(0)
    objs = []
    try:
        for name, v in options:
            c.set_option(name, v)
        tb = capi.Table(c, 4096, V_dim=k, init_mode=capi.INIT_HASH, **A["hyper"])
        objs.append(tb)
        keys = np.concatenate([A["keys"], B["keys"]])
        o = np.argsort(keys)
        tb.import_(keys[o], np.concatenate([A["scal"], B["scal"]])[o], np.concatenate([A["has_V"], B["has_V"]])[o],
                   np.concatenate([A["V"], B["V"]])[o] if k else None)
        bt = capi.Batch(c, max(len(A["label"]), len(B["label"])), max(len(A["index"]), len(B["index"])) + 64)
        objs.append(bt)
        bt.set_option("compute_auc", 1)
        out = dict(between=None)
        for i, D in enumerate((A, B)):
            bt.load_host(D["offset"], D["index"], D["value"], D["label"])
            bt.localize()
            bt.sgd_step(tb, is_train=True, push_cnt=D["push_cnt"])
            if i == 0 and read_between:
                out["between"] = bt.progress(reset=False)
        out["progress"] = bt.progress(reset=True)
        out["after"] = bt.progress(reset=False)
        tb.check()
        out["model"] = device_model(tb)
        return out
    finally:
        for o_ in objs[::-1]:
            o_.close()
        c.close()


TWO_STEP_ROUTES = {"default": (), "auc_in_update0": (("auc_in_update", 0),), "upd_kernel0": (("upd_kernel", 0),), "single_queue": (("single_queue", 1),)}


TWO_STEP_CASES = dict(argvalues=[(0, False), (5, True), (64, False)], ids=["V0-nocnt", "V5-cnt", "V64-nocnt"])


@pytest.mark.parametrize("V_dim,push_cnt", **TWO_STEP_CASES)
def test_two_step_designs_hold_their_conditions(oracle, V_dim, push_cnt):
    """CPU: the second design of test_two_steps_in_one_batch_object_add_up (seed 1, binary, "pen") passes check() and
    exact_progress's conditions, shares no key with the first, and the sum of the two steps' doubles is accepted as at most
    three floats, none of them a single step's"""
    A = design(X.FULL_LENGTHS, V_dim, False, push_cnt, "pen")
    B = design(X.FULL_LENGTHS, V_dim, True, push_cnt, "pen", seed=1)
    assert not np.isin(A["keys"], B["keys"]).any() and A["hyper"] == B["hyper"]
    pa, pb = expected(oracle, A)["progress"], expected(oracle, B)["progress"]
    both, one = X.accepted([pa, pb]), (X.accepted([pa]), X.accepted([pb]))
    for f in ("loss", "penalty"):
        assert 1 <= len(both[f]) <= 3 and not (both[f] & one[0][f]) and not (both[f] & one[1][f])
    assert both["auc"] not in (one[0]["auc"], one[1]["auc"]) and both["nrows"] != one[0]["nrows"]


@pytest.mark.gpu
@pytest.mark.parametrize("V_dim,push_cnt", **TWO_STEP_CASES)
def test_two_steps_in_one_batch_object_add_up(capi, oracle, V_dim, push_cnt):
    """two "pen" designs with disjoint keys through one batch object: the progress after both is float(the doubles of the two
    steps added up) — read between the steps and at the end, and read only at the end, where the first step's AUC reaches the
    sum through the second step's lookup (auc_pending), not through a read; with the AUC in a launch of its own, k_backward_all
    and the single queue as well.  Both designs' keys afterwards: their own expected models"""
    A = design(X.FULL_LENGTHS, V_dim, False, push_cnt, "pen")
    B = design(X.FULL_LENGTHS, V_dim, True, push_cnt, "pen", seed=1)
    wa, wb = expected(oracle, A), expected(oracle, B)
    both = X.accepted([wa["progress"], wb["progress"]])
    assert both["auc"] not in (X.accepted([wa["progress"]])["auc"], X.accepted([wb["progress"]])["auc"])
    for name, options in TWO_STEP_ROUTES.items():
        for read_between in (False, True):
            what = "%s, %s" % (name, "read between the steps" if read_between else "read at the end")
            got = _two_minibatches_one_batch_object(capi, A, B, read_between, options)
            if read_between:
                X.assert_progress(got["between"], X.accepted([wa["progress"]]), what + ": after the first step")
            X.assert_progress(got["progress"], both, what)
            assert progress_bits(got["after"]) == (0, 0, 0, 0, 0), what
            dk, scal, has, V = got["model"]
            for D, w in ((A, wa), (B, wb)):
                m = np.isin(dk, D["keys"])
                assert m.sum() == len(D["keys"])
                _assert_model((scal[m], has[m], V[m]), w["model"], D, what)
