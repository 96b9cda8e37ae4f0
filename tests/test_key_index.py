"""The open-addressing key index (dfh_kernels.hip: find_or_insert, find_or_insert_block, find_only, k_rehash) on DESIGNED
probe chains.  Random 64-bit keys spread evenly over an index that is at most half full: chains of one to three slots, never
past the last slot.  Here the keys are built through the exact inverse of splitmix64 (keyindex_testlib.py), so that a chain
runs past slot H - 1 and goes on at slot 0, a whole launch contends for one chain, two clusters merge, a growth rebuilds a
chain that wraps again in the larger index, preparation streams carry the same unseen keys, and the REFRAND scan crosses its
1024-thread boundary — each deterministic and tiny.  A wrong row id does not crash: it merges two features' state or loses one,
so every check is on row ids and per-key state, and every comparison is exact.

A change of the hash function must revisit keyindex_testlib.py."""
import functools

import numpy as np
import pytest

import keyindex_testlib as K

gpu = pytest.mark.gpu
H, ROWS = 1024, 512


# ------------------------------------------------------------------------------------------------------------------
# 1. key designer and host model (CPU)
# ------------------------------------------------------------------------------------------------------------------
def _probe_values():
    rng = np.random.default_rng(20)
    return [int(v) for v in rng.integers(0, K.M64, size=10000, dtype=np.uint64, endpoint=True)] + [0, 2 ** 64 - 1, 1023]


def test_unsplitmix64_round_trips_both_ways():
    for v in _probe_values():
        assert K.unsplitmix64(K.splitmix64(v)) == v
        assert K.splitmix64(K.unsplitmix64(v)) == v


def test_splitmix64_is_the_projects(oracle):
    from difacto_amd import synth
    vals = _probe_values()
    inv = [K.unsplitmix64(v) for v in vals]
    for xs in (vals, inv):
        got = synth.splitmix64(np.array(xs, dtype=np.uint64))
        assert [int(g) for g in got] == [K.splitmix64(x) for x in xs]
        for x in xs[:2000] + xs[-3:]:
            assert int(oracle.L.orc_splitmix64(x)) == K.splitmix64(x)
    # the inverse against the two other statements of the hash, not only against the one in the test library
    assert [int(g) for g in synth.splitmix64(np.array(inv, dtype=np.uint64))] == vals
    for v, k in list(zip(vals, inv))[-2003:]:
        assert int(oracle.L.orc_splitmix64(k)) == v


def test_modular_inverses_are_computed():
    assert (K._M1 * K._M1_INV) % (1 << 64) == 1 and (K._M2 * K._M2_INV) % (1 << 64) == 1


def test_keys_for_homes():
    rng = np.random.default_rng(21)
    homes = [int(h) for h in rng.integers(0, 1 << 20, size=300)] + [0, K.LAST20, 1023, 1024]
    keys = K.keys_for_homes(homes)
    assert keys.dtype == np.uint64 and len(set(keys.tolist())) == len(homes)
    assert K.EMPTY_KEY not in keys.tolist()
    for j, (k, h) in enumerate(zip(keys.tolist(), homes)):
        assert K.splitmix64(k) == ((j + 1) << 20) | h
        for b in range(10, 21):   # every table size from 1 024 to 2^20 slots
            assert K.home_of(k, 1 << b) == h & ((1 << b) - 1)
    homes10 = [h & 1023 for h in homes]
    for k, h in zip(K.keys_for_homes(homes10, bits=10).tolist(), homes10):
        assert K.home_of(k, 1024) == h
    # a second list with shifted tags shares no key with the first
    assert not set(K.keys_for_homes(homes, start=len(homes)).tolist()) & set(keys.tolist())


def test_index_model_is_linear_probing_with_wrap():
    m = K.IndexModel(8)
    a, b, c = K.keys_for_homes([7, 7, 0], bits=3).tolist()
    assert (m.insert(a), m.insert(b), m.insert(c)) == (7, 0, 1)
    assert m.insert(b) == 0 and m.n == 3
    assert (m.find(a), m.find(b), m.find(c)) == (7, 0, 1)
    assert m.find(K.keys_for_homes([7], bits=3, start=5)[0]) is None
    assert (m.probes(a), m.probes(b), m.probes(c)) == (1, 2, 2)
    assert m.occupied() == [0, 1, 7]


def _model(keys, Hs=H, order=None):
    m = K.IndexModel(Hs)
    for i in (range(len(keys)) if order is None else order):
        m.insert(keys[i])
    return m


@pytest.mark.parametrize("n", K.ONE_HOME_SIZES)
def test_shape_one_home_wrap(n):
    keys = K.one_home_wrap(n, H)
    assert len(keys) == n and all(K.home_of(k, H) == H - 1 for k in keys)
    want = sorted([H - 1] + list(range(n - 1)))
    for order in (None, list(reversed(range(n)))):
        m = _model(keys, order=order)
        assert m.occupied() == want                                       # H - 1, 0, 1, ..., n - 2
        assert sorted(m.probes(k) for k in keys) == list(range(1, n + 1))   # the k-th key of the chain is k probes away


def test_shape_straddle():
    keys = K.straddle(H)
    assert len(keys) == 300
    assert [K.home_of(k, H) for k in keys[:6]] == [H - 3, H - 2, H - 1, 0, 1, 2]
    want = sorted([H - 3, H - 2, H - 1] + list(range(297)))
    rng = np.random.default_rng(22)
    for order in (None, rng.permutation(300)):
        m = _model(keys, order=order)
        assert m.occupied() == want   # ONE chain from H - 3 across the wrap to slot 296
        assert max(m.probes(k) for k in keys) > 250


def test_shape_merging_clusters():
    keys = K.merging_clusters(H)
    c = K.MERGE_C
    assert [K.home_of(k, H) for k in keys] == [c] * 100 + [c + 60] * 100
    m = _model(keys)
    assert m.occupied() == list(range(c, c + 200))
    assert K.home_of(m.slot[c + 60], H) == c           # the second cluster's home lies inside the first one's chain ...
    assert all(m.find(k) >= c + 100 for k in keys[100:])   # ... so its keys walk 40 foreign slots and more
    m2 = _model(keys, order=list(range(100, 200)) + list(range(100)))   # the other order: the first cluster jumps the second
    assert m2.occupied() == list(range(c, c + 200))
    assert max(m2.probes(k) for k in keys[:100]) == 200


def test_shape_random_control():
    keys = K.random_control()
    assert len(keys) == 500 and len(set(keys.tolist())) == 500
    m = _model(keys)
    assert np.mean([m.probes(k) for k in keys]) < 2.0   # what the rest of the suite sees: short chains


def test_shape_every_size_last_slot():
    keys = K.every_size_last_slot(2112)
    assert len(set(keys.tolist())) == 2112
    for b in range(10, 21):
        assert all(K.home_of(k, 1 << b) == (1 << b) - 1 for k in keys[::97])
    m = _model(keys[:2048], 4096)   # 2 048 rows: the whole table is one chain that wraps
    assert m.occupied() == sorted([4095] + list(range(2047)))
    for Hs in (8192, 16384):        # ... and in the indices its growths build
        assert _model(keys[:300], Hs).occupied() == sorted([Hs - 1] + list(range(299)))
    assert not set(K.every_size_last_slot(10, start=2112).tolist()) & set(keys.tolist())


@pytest.mark.parametrize("shape", K.SHAPES)
def test_unseen_keys_start_inside_the_chain(shape):
    keys = K.shape_keys(shape, H)
    extra = K.unseen_in_chain(keys, H)
    occ = set(_model(keys).occupied())
    assert len(extra) == 40 and all(K.home_of(k, H) in occ for k in extra)
    assert not set(extra.tolist()) & set(keys.tolist())


def test_reverse_bytes_is_the_projects(oracle):
    for v in _probe_values()[:500] + [0, 2 ** 64 - 1, 1023]:
        assert K.reverse_bytes(v) == oracle.reverse_bytes(v) and K.reverse_bytes(K.reverse_bytes(v)) == v


# ------------------------------------------------------------------------------------------------------------------
# device side
# ------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def capi():
    from difacto_amd import capi as m
    m.lib()
    return m


@pytest.fixture(scope="module")
def ctx(capi):
    c = capi.Context(0)
    yield c
    for bt in _BATCHES.pop(id(c), ()):
        bt.close()
    c.close()


@functools.lru_cache(maxsize=None)
def _shape(name):
    keys = K.shape_keys(name, H)
    return keys, K.unseen_in_chain(keys, H)


VD = 4    # V_dim of the tables of sections 3 and 4
# V_threshold beyond any count: no count push initialises V, so that state is exactly what was imported
KW_PLAIN = dict(l1=0.0, l2=0.0, lr=0.1, V_lr=0.05, V_l2=0.0, V_threshold=1 << 30, V_init_scale=0.25, seed=4)
W0, CNT0 = 0.25, 7.0   # warm start


def _designed_state(n, first=0):
    """distinct, exactly representable state per key: (scal[n, 4] = {fea_cnt, w, sqrt_g, z}, has_V[n], V[n, 2 VD])"""
    j = np.arange(first, first + n, dtype=np.float64)
    scal = np.stack([3 + j, 1 + j * 2.0 ** -10, 0.5 + j * 2.0 ** -8, -(j + 1) * 2.0 ** -6], 1).astype(np.float32)
    has = (np.arange(first, first + n) % 3 == 0).astype(np.int32)
    V = ((j[:, None] + 1) * 2.0 ** -12 * (np.arange(2 * VD)[None, :] + 1)).astype(np.float32)
    V[has == 0] = 0
    return scal, has, V


def _sorted_export(tb):
    """(keys, scal, has_V, V) in key order: export lists the slots in whatever order its threads arrive"""
    e = tb.export()
    o = np.argsort(e["keys"])
    return e["keys"][o], e["scal"][o], e["has_V"][o], e["V"][o]


class _Env:
    """one table, its keys in a canonical order, and the state every key must have"""

    def __init__(self, capi, ctx, oracle, keys, tb):
        self.capi, self.ctx, self.oracle, self.tb = capi, ctx, oracle, tb
        self.keys = keys
        self.n = len(keys)
        self.scal = np.zeros((self.n, 4), np.float32)
        self.has = np.zeros(self.n, np.int32)
        self.V = np.zeros((self.n, 2 * VD), np.float32)
        self.rows = None          # row id per key, once first asked for
        self.extra = 0            # keys in the table that are not in self.keys
        self.stride = capi.row_stride(VD)
        self.rng = np.random.default_rng(5 + self.n)
        self.bufs = []

    def dev(self, arr):
        b = self.capi.DeviceBuffer.from_numpy(self.ctx, arr)
        self.bufs.append(b)
        return b

    def free(self):
        for b in self.bufs:
            b.close()
        self.bufs = []

    def perm(self):
        return self.rng.permutation(self.n)

    def saw_rows(self, idx, rows, what):
        """row ids are identical whenever they are asked for again"""
        rows = np.asarray(rows, np.uint32)
        if self.rows is None:
            self.rows = np.full(self.n, 0xFFFFFFFF, np.uint32)
        known = self.rows[idx] != 0xFFFFFFFF
        assert np.array_equal(rows[known], self.rows[idx][known]), "%s: row ids differ from an earlier answer" % what
        self.rows[idx] = rows

    def expected_rows(self, idx):
        """[w, has_V, 0, 0 | V] per key: the exchange layout of k_pull_rows / k_pull_resolved"""
        out = np.zeros((len(idx), 4 + VD), np.float32)
        out[:, 0] = self.scal[idx, 1]
        out[:, 1] = self.has[idx]
        out[:, 4:] = self.V[idx, :VD] * self.has[idx, None]
        return out

    # ---- the ways in -------------------------------------------------------------------------------------------
    def shard_resolve(self, idx=None, what="shard_resolve"):
        idx = self.perm() if idx is None else idx
        d_keys, d_rows = self.dev(self.keys[idx]), self.dev(np.zeros(len(idx), np.uint32))
        self.tb.shard_resolve(d_keys.ptr, len(idx), d_rows.ptr)
        self.saw_rows(idx, d_rows.to_numpy(np.uint32, len(idx)), what)

    def pull(self, idx=None):
        idx = self.perm() if idx is None else idx
        vals, lens = self.tb.pull(self.keys[idx])
        want = self.expected_rows(idx)
        assert np.array_equal(lens, np.where(self.has[idx] != 0, 1 + VD, 1)), "pull: lens"
        ragged = np.concatenate([np.concatenate([r[:1], r[4:]]) if h else r[:1] for r, h in zip(want, self.has[idx])])
        assert np.array_equal(vals, ragged), "pull: a key's weights are not its own"

    def push_count(self, idx=None):
        idx = self.perm() if idx is None else idx
        cnt = (idx + 1).astype(np.float32)      # a distinct count per key
        self.tb.push(self.keys[idx], self.capi.FEA_COUNT, cnt)
        self.scal[idx, 0] += cnt                # small integers: exact

    def import_(self, idx=None):
        idx = self.perm() if idx is None else idx
        scal, has, V = _designed_state(self.n)
        self.tb.import_(self.keys[idx], scal[idx], has[idx], V[idx])
        self.scal, self.has, self.V = scal, has, V

    def warm_start(self, idx=None):
        idx = self.perm() if idx is None else idx
        self.tb.warm_start(self.dev(self.keys[idx]).ptr, len(idx), W0, CNT0)
        self.scal[:] = [CNT0, W0, 0, 0]
        self.has[:] = 1
        self.V[:] = 0
        hv = self.oracle.L.orc_hash_init_value
        for i, k in enumerate(self.keys.tolist()):
            self.V[i, :VD] = [hv(k, d, KW_PLAIN["seed"], KW_PLAIN["V_init_scale"]) for d in range(VD)]

    def resolve_multi(self, G=4):
        """G sources that ALL carry the full key list: the same key sits in G lanes of one launch"""
        n = self.n
        idxs = [self.perm() for _ in range(G)]
        allidx = np.concatenate(idxs)
        seg = np.arange(G + 1) * n
        d_keys = self.dev(self.keys[allidx])
        words = self.capi.multi_words(G * n, G)
        d_rowid = self.dev(np.zeros(words, np.uint32))
        self.tb.shard_resolve_multi(d_keys.ptr, seg, d_rowid.ptr)
        rw = d_rowid.to_numpy(np.uint32, words)[:G * n]
        self.tb.shard_release(d_rowid.ptr, G * n)
        rows = rw & np.uint32(0x0FFFFFFF)
        for g in range(G):
            self.saw_rows(idxs[g], rows[g * n:(g + 1) * n], "shard_resolve_multi, source %d" % g)
        workers = np.zeros(n, np.int64)
        np.add.at(workers, allidx, (rw >> np.uint32(31)).astype(np.int64))
        assert np.all(workers == 1), "shard_resolve_multi: every key has exactly one worker entry"

    def _minibatch(self, bt, min_pairs):
        """rows 0 .. n - 1 hold ONE key each (binary: x = 1), in a permutation; further rows of 128 ids bring the minibatch
        beyond min_pairs.  Returns the permutation."""
        idx = self.perm()
        raw = K.raw_ids(self.keys)
        ids = [raw[idx]]
        lens = [np.ones(self.n, np.int64)]
        fill = max(0, min_pairs - self.n)
        nfill = (fill + 127) // 128
        if nfill:
            ids.append(raw[self.rng.integers(0, self.n, size=nfill * 128)])
            lens.append(np.full(nfill, 128, np.int64))
        off = np.concatenate([[0], np.cumsum(np.concatenate(lens))]).astype(np.uint64)
        lab = np.where(np.arange(len(off) - 1) % 2 == 0, 1.0, -1.0).astype(np.float32)
        bt.load_host(off, np.concatenate(ids), None, lab)
        return idx

    def _check_step(self, bt, idx, what):
        """a validation step reads the rows the lookup found: the logit of a one-key row of a key without V is that key's w
        (1 * w, nothing to round)"""
        before = _sorted_export(self.tb)
        bt.sgd_step(self.tb, is_train=False)
        pred = bt.pred()[:self.n]
        bt.progress(reset=True)
        nov = self.has[idx] == 0
        assert np.array_equal(pred[nov], self.scal[idx, 1][nov]), "%s: a row's logit is not its key's w" % what
        after = _sorted_export(self.tb)
        assert all(np.array_equal(a, b) for a, b in zip(before, after)), "%s: a validation step moved the model" % what

    def localize_probe(self):
        """Batch.localize(table=tb): the PROBE path of k_loc_emit"""
        bt = _batches(self.capi, self.ctx)[0]
        idx = self._minibatch(bt, 0)
        bt.localize(table=self.tb)
        self._check_step(bt, idx, "localize(table=)")

    def localize_lookup(self):
        """Batch.localize() then Batch.lookup(tb): k_lookup in 256-thread blocks (a minibatch of 16 384 pairs or fewer leaves
        the probe to the step, so this one is larger)"""
        bt = _batches(self.capi, self.ctx)[1]
        idx = self._minibatch(bt, 16385)
        bt.localize()
        bt.lookup(self.tb)
        self._check_step(bt, idx, "localize() + lookup()")

    # ---- what must hold after every one of them ------------------------------------------------------------------
    def verify(self, what):
        tb, n = self.tb, self.n
        assert tb.size() == n + self.extra, what
        tb.check()
        self.shard_resolve(what=what)
        assert np.all(self.rows < n + self.extra), "%s: a row id beyond size()" % what
        assert len(np.unique(self.rows)) == n, "%s: two keys share a row" % what
        e = tb.export()
        o = np.argsort(e["keys"])
        mine = np.isin(e["keys"][o], self.keys)
        assert int(mine.sum()) == n and len(o) == n + self.extra, what
        ks = np.argsort(self.keys)
        assert np.array_equal(e["keys"][o][mine], self.keys[ks]), what
        assert np.array_equal(e["scal"][o][mine], self.scal[ks]), "%s: export: a key's scalars are not its own" % what
        assert np.array_equal(e["has_V"][o][mine], self.has[ks]), what
        assert np.array_equal(e["V"][o][mine], self.V[ks] * self.has[ks, None]), "%s: export: V" % what
        self.pull()
        idx = self.perm()
        d_keys, d_rows = self.dev(self.keys[idx]), self.dev(np.zeros((n, self.stride), np.float32))
        tb.shard_pull(d_keys.ptr, n, d_rows.ptr)
        got = d_rows.to_numpy(np.float32, n * self.stride).reshape(n, self.stride)[:, :4 + VD]
        assert np.array_equal(got, self.expected_rows(idx)), "%s: shard_pull" % what
        d_rid, d_rows2 = self.dev(self.rows[idx]), self.dev(np.zeros((n, self.stride), np.float32))
        tb.shard_pull_resolved(d_rid.ptr, n, d_rows2.ptr)
        got = d_rows2.to_numpy(np.float32, n * self.stride).reshape(n, self.stride)[:, :4 + VD]
        assert np.array_equal(got, self.expected_rows(idx)), "%s: shard_pull_resolved" % what
        self.free()


_BATCHES = {}


def _batches(capi, ctx):
    """two batch objects for the whole module: (one key per row, beyond 16 384 pairs)"""
    if id(ctx) not in _BATCHES:
        _BATCHES[id(ctx)] = (capi.Batch(ctx, ROWS, ROWS), capi.Batch(ctx, ROWS + 136, ROWS + 136 * 128))
    return _BATCHES[id(ctx)]


INSERTERS = ["shard_resolve", "pull", "push_count", "import_", "warm_start", "resolve_multi", "localize_probe",
             "localize_lookup"]
# after the first: the two that overwrite a row's state, then the import of the designed state on the rows that exist, then
# everything that must leave it alone
ORDER = ["warm_start", "push_count", "import_", "shard_resolve", "pull", "resolve_multi", "localize_probe", "localize_lookup",
         "push_count"]


# ------------------------------------------------------------------------------------------------------------------
# 3. every way in, same answers
# ------------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("first", INSERTERS)
@pytest.mark.parametrize("shape", K.SHAPES)
def test_every_way_in_gives_the_same_rows(capi, ctx, oracle, shape, first):
    """One table of 512 rows (1 024 slots), one designed shape, one first inserter; then every other reader and inserter on the
    same keys in another permutation.  size() is the number of distinct keys, check() is clean (one_home_wrap-512 fills the
    table exactly: no capacity error), row ids are distinct, inside [0, size) and the same whenever asked for again
    (shard_resolve, the row words of shard_resolve_multi), export holds exactly the keys, and state is per key: what was
    imported (w = 1 + j 2^-10, a distinct fea_cnt, V for every third key), warm-started or pushed for key j is what pull,
    shard_pull, shard_pull_resolved and export return for key j.  With push_count first on one_home_wrap-257 / -512 the
    block-wide row hand-out of find_or_insert_block spans several blocks and all four waves of a block.

    Unseen keys whose homes lie inside the chain then pull zeros, size() grows by their number and nothing else moves.
    The table has 512 rows: 40 of them where 40 fit, 512 - n otherwise (12 behind the 500 random keys, none behind
    one_home_wrap-512)."""
    keys, unseen = _shape(shape)
    tb = capi.Table(ctx, ROWS, V_dim=VD, **KW_PLAIN)
    assert tb.capacity() == (ROWS, 0)
    env = _Env(capi, ctx, oracle, keys, tb)
    try:
        getattr(env, first)()
        env.verify("after %s first" % first)
        for name in ORDER:
            getattr(env, name)()
            env.verify("%s after %s first" % (name, first))
        assert np.array_equal(env.scal[:, 1], _designed_state(env.n)[0][:, 1])   # the designed w is what all of this saw
        extra = unseen[:min(40, ROWS - env.n)]
        if len(extra):
            vals, lens = tb.pull(extra)
            assert not vals.any() and np.all(lens == 1) and len(vals) == len(extra)
            env.extra = len(extra)
        env.verify("after %d unseen keys" % len(extra))
    finally:
        env.free()
        tb.close()


# ------------------------------------------------------------------------------------------------------------------
# 4. growth
# ------------------------------------------------------------------------------------------------------------------
@gpu
def test_growth_rebuilds_a_chain_that_wraps_again(capi, oracle):
    """A growing table (first allocation 16 rows) takes every_size_last_slot keys in imports of 64, with count pushes and
    pulls of old and new keys in between: ONE chain that starts at the last slot of every index the table ever has, so k_rehash
    rebuilds a single-home chain that wraps in the new index — at the end one of more than 2 048 keys.  Row ids must be the
    same before and after every growth (all keys so far are resolved again after every call that grew the table, and once
    per import), and at the end every key's scal, has_V and V from export equal what was imported plus the pushed counts,
    bit for bit."""
    ctx = capi.Context(0)
    ctx.set_option("grow_initial_rows", 16)
    tb = capi.Table(ctx, 0, V_dim=VD, **KW_PLAIN)
    NMAX, CH = 3008, 64
    keys = K.every_size_last_slot(NMAX)
    scal, has, V = _designed_state(NMAX)
    has = (np.arange(NMAX) % 2).astype(np.int32)
    V = ((np.arange(NMAX)[:, None] + 1) * 2.0 ** -12 * (np.arange(2 * VD)[None, :] + 1)).astype(np.float32) * has[:, None]
    d_keys = capi.DeviceBuffer.from_numpy(ctx, keys)
    d_rows = capi.DeviceBuffer(ctx, 4 * CH)
    rows = np.zeros(0, np.uint32)
    grown_at = []       # keys in the table at each growth

    def grew(n_in):
        if tb.capacity()[1] == len(grown_at):
            return False
        assert tb.capacity()[1] == len(grown_at) + 1
        grown_at.append(n_in)
        return True

    def resolve_all(n, what):
        """all keys so far, in calls of 64 (a call's size is what the growth policy reserves for); a call that grows the
        table starts the pass again, so that the last pass is one over an index nothing rebuilt meanwhile"""
        nonlocal rows
        if n == 0:
            return
        for _ in range(4):
            got = np.zeros(n, np.uint32)
            again = False
            for a in range(0, n, CH):
                m = min(CH, n - a)
                tb.shard_resolve(d_keys.at(8 * a), m, d_rows.ptr)
                got[a:a + m] = d_rows.to_numpy(np.uint32, m)
                again = grew(n) or again
            assert np.array_equal(got[:len(rows)], rows), "%s: row ids moved" % what
            assert len(np.unique(got)) == n and got.max() < n, what
            rows = got
            if not again:
                return
        raise AssertionError("the table grew in four passes in a row")

    def call(n_in, fn):
        fn()
        if grew(n_in):
            resolve_all(n_in, "after growth %d" % tb.capacity()[1])

    n = 0
    rng = np.random.default_rng(44)
    try:
        while n < NMAX and not (len(grown_at) >= 2 and grown_at[-1] >= 2048):
            a, b = n, n + CH
            call(a, lambda: tb.import_(keys[a:b], scal[a:b], has[a:b], V[a:b]))
            n = b
            resolve_all(n, "after the import of keys %d..%d" % (a, b))
            old = rng.permutation(n)[:CH]                    # count push: keys from anywhere in the chain
            cnt = (1 + old % 5).astype(np.float32)
            call(n, lambda: tb.push(keys[old], capi.FEA_COUNT, cnt))
            scal[old, 0] += cnt
            old = rng.permutation(np.union1d(rng.permutation(n)[:CH // 2], np.arange(b - CH // 2, b)))   # old and new keys
            res = []
            call(n, lambda: res.append(tb.pull(keys[old])))
            vals, lens = res[0]
            assert np.array_equal(lens, np.where(has[old] != 0, 1 + VD, 1))
            want = np.concatenate([np.concatenate([scal[i, 1:2], V[i, :VD]]) if has[i] else scal[i, 1:2] for i in old])
            assert np.array_equal(vals, want), "pull with %d keys in the table" % n
        assert tb.capacity()[1] >= 2 and grown_at[-1] >= 2048, (tb.capacity(), grown_at, n)
        resolve_all(n, "at the end")
        assert tb.size() == n
        tb.check()
        e = tb.export()
        o = np.argsort(e["keys"])
        ks = np.argsort(keys[:n])
        assert np.array_equal(e["keys"][o], keys[:n][ks])
        assert np.array_equal(e["scal"][o], scal[:n][ks]), "a key's scalars are not what was imported plus its counts"
        assert np.array_equal(e["has_V"][o], has[:n][ks])
        assert np.array_equal(e["V"][o], V[:n][ks])
    finally:
        d_keys.close()
        d_rows.close()
        tb.close()
        ctx.close()


# ------------------------------------------------------------------------------------------------------------------
# 5. the training step on colliding keys
# ------------------------------------------------------------------------------------------------------------------
def _colliding_batches(seed, keys, nbatch=3, nrows=120, max_row=30):
    rng = np.random.default_rng(seed)
    raw = K.raw_ids(keys)
    out = []
    for i in range(nbatch):
        lens = rng.integers(0, max_row + 1, size=nrows)
        off = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)
        nnz = int(off[-1])
        out.append(dict(offset=off, index=raw[rng.integers(0, len(raw), size=nnz)],
                        value=None if i % 2 == 1 else rng.normal(size=nnz).astype(np.float32),
                        label=np.where(rng.random(nrows) < 0.4, 1.0, -1.0).astype(np.float32)))
    return out


@gpu
@pytest.mark.parametrize("V_dim", [0, 8])
@pytest.mark.parametrize("variant", ["hash", "refrand", "hash_growing"])
def test_fused_step_on_colliding_keys(capi, ctx, oracle, V_dim, variant):
    """the training step against the oracle, step by step from identical state (test_gpu_parity._run_fused_vs_oracle, its
    tolerances), on minibatches whose 500 keys are 200 of one_home_wrap and 300 of straddle: one chain across the wrap of a
    512-row table, or of every index a growing table has"""
    from test_gpu_parity import _run_fused_vs_oracle
    keys = np.concatenate([K.one_home_wrap(200, H), K.straddle(H, 300, start=200)])
    assert len(set(keys.tolist())) == 500
    batches = _colliding_batches(60 + V_dim, keys)
    kw = dict(l1=0.02, l2=0.01, lr=0.3, V_lr=0.05, V_l2=0.02, V_threshold=1, V_init_scale=0.2, seed=9)
    if variant == "hash_growing":
        gctx = capi.Context(0)
        gctx.set_option("grow_initial_rows", 16)
        tb = capi.Table(gctx, 0, V_dim=V_dim, init_mode=capi.INIT_HASH, **kw)
        try:
            n_with_v = _run_fused_vs_oracle(capi, gctx, oracle, V_dim, "hash", batches, 3, kw, table=tb)
            assert tb.capacity()[1] >= 1
            tb.check()
            assert tb.size() == len(np.unique(np.concatenate([b["index"] for b in batches])))
        finally:
            tb.close()
            gctx.close()
    else:
        n_with_v = _run_fused_vs_oracle(capi, ctx, oracle, V_dim, variant, batches, 3, kw, capacity=ROWS)
    assert (n_with_v > 0) == (V_dim > 0)


# ------------------------------------------------------------------------------------------------------------------
# 6. shared new keys across streams
# ------------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("streams,nbatch,form", [(2, 4, "fused"), (3, 6, "fused"), (2, 5, "lookup"), (3, 4, "lookup")])
def test_shared_new_keys_across_streams(capi, streams, nbatch, form):
    """Consecutive minibatches share most of their never-seen keys, all of them every_size_last_slot keys (one chain), and are
    probed on 2 or 3 preparation streams (the emit pass's own probe, or k_lookup on minibatches beyond 16 384 pairs) while
    earlier ones train: two launches can meet at a slot whose key is claimed and whose row id is not yet published.  That is
    the `pending` branch of find_or_insert_block and the wait of find_or_insert; this test EXERCISES it but cannot force it
    — which launch claims a slot first is up to the hardware.  Whatever the interleaving, the pipelined run must equal the
    serial run bit for bit, in every prediction and in the exported model, and check() must be clean."""
    from test_gpu_parity import _export_index
    rng = np.random.default_rng(80 + streams + nbatch)
    keys = K.every_size_last_slot(400 + 80 * nbatch)
    raw = K.raw_ids(keys)
    batches = []
    for i in range(nbatch):   # minibatch i draws from keys [80 i, 80 i + 400): 320 of them shared with the next
        nrows, per = 150, 120
        off = (np.arange(nrows + 1) * per).astype(np.uint64)
        idx = raw[80 * i + rng.integers(0, 400, size=nrows * per)]
        batches.append(dict(offset=off, index=idx, value=None if i % 2 == 0 else rng.normal(size=nrows * per).astype(np.float32),
                            label=np.where(rng.random(nrows) < 0.4, 1.0, -1.0).astype(np.float32)))
    kw = dict(l1=0.02, l2=0.01, lr=0.3, V_lr=0.05, V_l2=0.02, V_threshold=0, V_init_scale=0.2, seed=5)
    results = []
    for depth in (0, streams):
        ctx = capi.Context(0)
        ctx.set_pipeline(depth)
        ahead = max(depth, 1)
        tb = capi.Table(ctx, 1 << 13, V_dim=8, **kw)
        bts = [capi.Batch(ctx, 150, 150 * 120) for _ in range(nbatch if depth else 2)]

        def prep(i):
            b, bt = batches[i % nbatch], bts[i % len(bts)]
            bt.load_host(b["offset"], b["index"], b["value"], b["label"])
            if form == "fused" and depth:
                bt.localize(table=tb)
                return
            bt.localize()
            bt.lookup(tb)

        preds = []
        nsteps = 2 * nbatch
        for i in range(ahead):
            prep(i)
        for i in range(nsteps):
            if i + ahead < nsteps:
                prep(i + ahead)
            bts[i % len(bts)].sgd_step(tb, is_train=True, push_cnt=(i < nbatch))
            preds.append(bts[i % len(bts)].pred())
        tb.check()
        assert tb.size() == len(np.unique(np.concatenate([b["index"] for b in batches])))
        results.append((preds, _export_index(tb)))
        for o in bts + [tb]:
            o.close()
        ctx.close()
    (p0, e0), (p1, e1) = results
    for i, (a, b) in enumerate(zip(p0, p1)):
        assert np.array_equal(a, b), "predictions of step %d" % i
    for name, a, b in zip(("keys", "scal", "has_V", "V"), e0, e1):
        assert np.array_equal(a, b), "exported %s" % name


# ------------------------------------------------------------------------------------------------------------------
# 7. REFRAND order across the scan's block boundary
# ------------------------------------------------------------------------------------------------------------------
def _subset(name, U):
    idx = {"none": [], "all": range(U), "1023_1024": [1023, 1024], "every_7th": range(0, U, 7), "last": [U - 1]}[name]
    return np.array([i for i in idx if i < U], dtype=np.int64)


@gpu
@pytest.mark.parametrize("subset", ["none", "all", "1023_1024", "every_7th", "last"])
@pytest.mark.parametrize("U", [1, 1023, 1024, 1025, 2049, 3000])
def test_refrand_order_across_the_scan_boundary(capi, ctx, oracle, U, subset):
    """INIT_REFRAND draws V from ONE rand_r chain in key order: k_refrand_scan ranks the keys that need V in a single block
    of 1 024 threads and carries the count from one 1 024-key iteration to the next; k_refrand_init finds the row again
    through find_only; k_refrand_advance moves the chain on.  U ascending keys around the iteration boundary, a chosen subset
    preset to w != 0 and fea_cnt = 2 = V_threshold, one Push(kFeaCount) of ones: exactly the subset gets V, with the values
    the oracle's serial loop draws, bit for bit.  A second push after presetting a further subset must go on where the first
    chain ended."""
    from oracle import bindings as ob
    kw = dict(V_dim=3, l1=0.0, l2=0.0, lr=0.1, V_lr=0.05, V_l2=0.0, V_threshold=2, V_init_scale=0.3, seed=11)
    rng = np.random.default_rng(7000 + U)
    keys = np.unique(rng.integers(1, 2 ** 63, size=U + 50, dtype=np.uint64))[:U]
    assert len(keys) == U
    tb = capi.Table(ctx, 4096, init_mode=capi.INIT_REFRAND, **kw)
    so = oracle.store_create(init_mode=ob.INIT_REFRAND, **kw)
    first = _subset(subset, U)
    rest = np.setdiff1d(np.arange(U), first)
    second = rest[rest % 3 == 1]
    if U > 1025:   # the further subset reaches across the boundary too
        second = np.union1d(second, np.intersect1d(rest, [1022, 1023, 1024, 1025]))
    ones = np.ones(U, np.float32)
    try:
        for rnd, sub in enumerate((first, second)):
            if len(sub):
                scal = np.zeros((len(sub), 4), np.float32)
                scal[:, 0] = 2.0
                scal[:, 1] = 0.5 + (sub % 64) * 2.0 ** -7
                tb.import_(keys[sub], scal, np.zeros(len(sub), np.int32), np.zeros((len(sub), 6), np.float32))
                for i, s in zip(sub, scal):
                    so.poke(int(keys[i]), *s, None)
            tb.push(keys, capi.FEA_COUNT, ones)
            so.push(keys, ob.FEA_COUNT, ones)
            vg, lg = tb.pull(keys)
            vo, lo = so.pull(keys)
            want = np.ones(U, np.int32)
            want[first] = 4
            if rnd:
                want[second] = 4
            assert np.array_equal(lo, want)
            assert np.array_equal(lg, lo), "push %d: not exactly the preset keys got V" % rnd
            assert np.array_equal(vg, vo), "push %d: V is not what the serial rand_r chain draws" % rnd
        tb.check()
        assert tb.size() == U
    finally:
        tb.close()
