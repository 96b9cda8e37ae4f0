"""The overlap schedule of the sharded step (shard_step_overlap, csrc/dfh_shard.hip), bit for bit: two minibatches in flight,
exchange slots in alternation, the others' row words folded into the own keys' lookup, the order of its stages.

One process is rank r of a 3-rank job whose peers are a script (scripted_peers.StreamPeers through capi.Comm.callback).  A
stream is three exact-sum designs A, B, C (exact_step_design.build with seeds 0, 1, 2; valued, binary, valued; one V_dim, one
push_cnt, one set of hyper-parameters): their key sets are disjoint, the other owners' rows are what the script supplies, so
every step of the stream has exactly one right answer although after the first step the touched part of the model is generic
(test_update_exact.expected per design).  The rank owns one key range [s0, s1) out of the union of the three key lists.

  worker side   ranks 1 (every V_dim of the switches' list, with and without counts), 0 and 2: per step the COUNTS words, KEYS,
                CNT and every word of every GRADS row the rank sends, the logits and the split list; afterwards the whole shard.
  owner side    the peers also send keys of rank 1's range that are in no minibatch — imported with V, imported without, never
                seen, some from both peers, most of them in several steps — with arbitrary full-mantissa gradient rows, and
                own keys of an earlier minibatch.  ONE oracle store takes the documented order (emulate_overlap,
                test_shard_native.py): L(t)'s own count push, at the first step the peers' count push and the pull, the own
                keys' exact gradient, R(t+1) = the peers' count push and pull of the NEXT minibatch, then P(t) = the peers'
                gradients of step t in ascending source rank.  The rows the rank answers with, per step and peer, and its whole
                shard must equal that store.  A key that received GRADS(t) and is asked for in KEYS(t+1) shows the state
                before P(t), in KEYS(t+2) the state after it; with counts, a key without V whose count crosses V_threshold
                through CNT(1) while GRADS(0) still carry its row as pulled without V: ROWS(1) show the hash-initialised V
                with zero accumulators and P(0) applies w's gradient alone (the oracle's push of length 1).
  switches      shard_mixed_update = 0, upd_split = 0, upd_kernel = 0, single_queue = 1, set_pipeline(1): the same bytes.
  degenerate    a range in which B has no own key (no L launch, k_uw_remote in F; C folds again), the rank out of data,
                a validation step B, the epoch's end, and the sync schedule on the same stream — whose answered rows differ
                from the overlap run's at the designed keys, which is asserted: the keys discriminate the two orders.
  replay        the owner-side stream once more over capi.Comm.loopback with a modelled wire of 200 us per exchange.

Found by these tests: without preparation streams (no set_pipeline: every run here but one) nothing ordered the collectives'
stream behind the Localizer of the announced minibatch, queued on the main stream or, on the single queue, only noted; from
the third minibatch on COUNTS and KEYS carried the batch object's previous key list.  shard_step_overlap now waits for the
main stream there (cs_behind_prep).

Every comparison is on bit patterns: no tolerance, no mask, no skipped key.  The progress sums of every batch object — over the
minibatches it took, the doubles added up before the cast — are held to the designs' exact_progress in every run (loss, AUC,
rows), and the penalty on the "pen" streams (section f): the narrow range, the validation step with both k_penalty launches,
every switch, read at the end and after every step.  A second step on the SAME keys is pinned in test_second_step_exact.py (the
sync schedule, rank 1); not pinned: its V-dependent logits, the zero rows' loss at V_dim = 0, l2's penalty term beside the
drivers.  (What no bit comparison can tell apart: a step whose fold is switched off takes k_uw_remote in
F, which is built to leave the same row words — the degenerate case holds both ways to the same answer.)
"""
import numpy as np
import pytest

import exact_step_design as X
import test_sharded_exact as T
import test_update_exact as E
from scripted_peers import StreamPeers
from split_testlib import split_entries_expected

same_bits, bits = E.same_bits, E.bits
W = T.W
SEEDS = (0, 1, 2)
BINARY = (False, True, False)
STREAMS = [(V_dim, push_cnt) for V_dim in E.SWITCH_VDIMS for push_cnt in (False, True)]
STREAM_IDS = ["V%d-%s" % (k, "cnt" if c else "nocnt") for k, c in STREAMS]
WIRE_GBPS, WIRE_LATENCY_US = 64.0, 200.0     # the modelled wire of the replay: an input, several times a step's kernels


@pytest.fixture(scope="module")
def capi():
    from difacto_amd import capi as m
    m.lib()
    return m


# ------------------------------------------------------------------ the streams
_SDESIGNS, _STREAMS = {}, {}


def sdesign(V_dim, binary, push_cnt, seed, variant="base"):
    if seed == 0:
        return E.design(X.FULL_LENGTHS, V_dim, binary, push_cnt, variant)     # shared with the one-step tests (and its expected())
    key = (V_dim, binary, push_cnt, seed, variant)
    if key not in _SDESIGNS:
        _SDESIGNS[key] = X.build(X.FULL_LENGTHS, V_dim, binary, push_cnt, variant, seed=seed)
    return _SDESIGNS[key]


def offs_of(designs, splits):
    return [[0, int(np.searchsorted(D["keys"], splits[0])), int(np.searchsorted(D["keys"], splits[1])), len(D["keys"])] for D in designs]


def rank1_classes(designs, offs):
    """per class of occurrences: (rank 1 owns such a key in some minibatch, it has such a remote key — two of one occurrence)"""
    out = []
    for _, a, b in T.CLASSES:
        own = rem = False
        for D, off in zip(designs, offs):
            m = (D["cnt"] >= a) & (D["cnt"] <= b)
            mine = np.zeros(len(m), bool)
            mine[off[1]:off[2]] = True
            own = own or bool((m & mine).any())
            rem = rem or int((m & ~mine).sum()) >= (2 if b == 1 else 1)
        out.append((own, rem))
    return out


def stream_ok(designs, offs):
    """required of every stream: every minibatch has own keys of rank 1 and remote keys on both sides, and over the stream
    every class of occurrences has an own and a remote key"""
    return all(0 < o[1] < o[2] < o[3] for o in offs) and all(a and b for a, b in rank1_classes(designs, offs))


def make_stream(V_dim, push_cnt, variant="base"):
    """-> dict(designs [A, B, C], union, splits u64 [2], offs, per_minibatch): the split keys nearest to thirds of the union of
    the key lists that satisfy stream_ok and, where such a pair exists, split_ok of every minibatch on its own.  (A variant
    changes the hyper-parameters alone: the minibatches, keys and ranges are the base stream's)"""
    key = (V_dim, push_cnt, variant)
    if key in _STREAMS:
        return _STREAMS[key]
    designs = [sdesign(V_dim, BINARY[i], push_cnt, SEEDS[i], variant) for i in range(3)]
    union = np.concatenate([D["keys"] for D in designs])
    assert len(np.unique(union)) == len(union), "the designs of a stream share a key"
    union = np.sort(union)
    n = len(union)
    pos = [np.searchsorted(D["keys"], union) for D in designs]
    cnts = [D["cnt"].astype(np.int64) for D in designs]
    found = {}
    for _, a, b in sorted((abs(a - n // 3) + abs(b - 2 * n // 3), a, b) for a in range(1, n - 1) for b in range(a + 1, n)):
        offs = [[0, int(p[a]), int(p[b]), len(D["keys"])] for p, D in zip(pos, designs)]
        if not all(0 < o[1] < o[2] < o[3] for o in offs):
            continue
        if not stream_ok(designs, offs):
            continue
        found.setdefault(False, (a, b))
        if all(T.split_ok(c, o) for c, o in zip(cnts, offs)):
            found[True] = (a, b)
            break
        if abs(a - n // 3) + abs(b - 2 * n // 3) > n // 3:
            break
    assert found, "no pair of split keys gives the stream's rank 1 an own and a remote key of every class"
    per = True in found
    a, b = found[per]
    splits = union[[a, b]]
    S = dict(V_dim=V_dim, push_cnt=push_cnt, designs=designs, union=union, splits=splits, offs=offs_of(designs, splits), per_minibatch=per,
             at=(a, b), variant=variant)
    _STREAMS[key] = S
    return S


def narrow_stream(S):
    """the same designs with a range [s0, s1) in which B has no key while A and C have: the longest run of the union without a
    key of B that holds a key of A and one of C and leaves keys of every design on both sides"""
    designs, union = S["designs"], S["union"]
    n = len(union)
    of = np.zeros(n, np.int64)
    for i, D in enumerate(designs):
        of[np.isin(union, D["keys"])] = i
    best = None
    a = 0
    while a < n:
        if of[a] == 1:
            a += 1
            continue
        b = a
        while b < n and of[b] != 1:
            b += 1
        run = of[a:b]
        if (run == 0).any() and (run == 2).any() and a > 0 and b < n and (best is None or b - a > best[1] - best[0]):
            if all((of[:a] == i).any() and (of[b:] == i).any() for i in range(3)):
                best = (a, b)
        a = b
    assert best is not None, "no run of the union without a key of B that holds keys of A and C"
    splits = union[[best[0], best[1]]]
    offs = offs_of(designs, splits)
    assert offs[1][1] == offs[1][2] and offs[0][2] > offs[0][1] and offs[2][2] > offs[2][1]
    return dict(S, splits=splits, offs=offs, per_minibatch=False, at=best)


# ------------------------------------------------------------------ what the peers send rank 1
# the j-th key of a kind (PV, PN: four keys, PU: three) -> {peer: the minibatches it asks for the key with}
ASKED = ({0: (0, 1, 2), 2: (0, 1, 2)}, {0: (0, 2)}, {2: (1, 2), 0: (2,)}, {2: (0, 1), 0: (1,)})


def peer_plan(S):
    """-> dict(keys [t]{p}, cnt [t]{p}, imported = (keys, scal, has_V, V), kinds {name: keys}, own_asked [t]): the keys peers 0
    and 2 send rank 1 with minibatch t, all inside its range.

    Peer-only keys (the successors of own keys: ids are 63 random bits, they are free): PV imported with V (at V_dim 0: with
    w != 0), PN imported without V, PU never seen, and with counts and V_dim > 0 one key PX imported without V, w != 0, at
    V_threshold - 1: CNT(0) puts it ON the threshold (pulled without V), CNT(1) beyond it.  Who asks for the j-th key of a kind
    with which minibatch is ASKED[j]: one key from both peers with every minibatch, one from peer 0 with the first and the
    third, one that appears with the second, one that leaves after it — none appears with the third only (a validation step
    B must leave the table as it was).  PX comes from peer 0 with every minibatch.
    Own keys asked for by a peer: one of minibatch 0 (peer 2, with minibatches 1 and 2) and one of minibatch 1 (both peers, with
    minibatch 2), of classes V and N whose counts stay below the threshold."""
    k, push_cnt, designs, offs = S["V_dim"], S["push_cnt"], S["designs"], S["offs"]
    s0, s1 = S["splits"]
    rng = np.random.default_rng([77, k, int(push_cnt)])
    thr = designs[0]["hyper"]["V_threshold"]
    own = S["union"][(S["union"] >= s0) & (S["union"] < s1)]
    nq = 12
    at = np.linspace(0, len(own) - 2, nq).astype(np.int64)
    Q = own[at] + np.uint64(1)
    assert len(np.unique(Q)) == nq and not np.isin(Q, S["union"]).any() and Q.min() > s0 and Q.max() < s1
    kinds = dict(PV=Q[0:4], PN=Q[4:8], PU=Q[8:11])
    with_px = bool(push_cnt and k > 0)
    if with_px:
        kinds["PX"] = Q[11:12]
    # the imported model of PV, PN (and PX): generic values
    ikeys = np.concatenate([kinds["PV"], kinds["PN"]] + ([kinds["PX"]] if with_px else []))
    ni = len(ikeys)
    w = (rng.normal(size=ni) * 0.5).astype(np.float32)
    w[w == 0] = 0.25
    scal = np.stack([np.floor(rng.random(ni) * 50), w, np.abs(rng.normal(size=ni)) + 0.01, rng.normal(size=ni) * 0.3], 1).astype(np.float32)
    has = np.zeros(ni, np.int32)
    V = np.zeros((ni, 2 * k), np.float32)
    if k:
        has[:4] = 1
        V[:4, :k] = rng.normal(size=(4, k)) * 0.1
        V[:4, k:] = np.abs(rng.normal(size=(4, k))) * 0.5 + 0.01
    if with_px:
        scal[-1, 0] = thr - 1
    # own keys of minibatches 0 and 1 a peer asks for later
    own_asked = []
    for t, c in ((0, "V"), (1, "N")):
        D, off = designs[t], offs[t]
        u = np.arange(off[1], off[2])
        fea1 = D["scal"][u, 0].astype(np.float64) + (D["cnt"][u] if push_cnt else 0)
        ok = (D["cls"][u] == c) & (fea1 + 4 < thr) & ~np.isin(u, D["drivers"])
        if not ok.any():
            ok = np.isin(D["cls"][u], ("V", "N")) & (fea1 + 4 < thr) & ~np.isin(u, D["drivers"])
        assert ok.any(), "minibatch %d: rank 1 owns no quiet key of class V or N" % t
        own_asked.append(D["keys"][u[ok][0]])
    keys, cnt = [], []
    for t in range(3):
        kt = {}
        for p in (0, 2):
            mine = [q[j] for q in (kinds["PV"], kinds["PN"], kinds["PU"]) for j in range(len(q)) if t in ASKED[j].get(p, ())]
            if with_px and p == 0:
                mine.append(Q[11])
            if t >= 1 and p == 2:
                mine.append(own_asked[0])
            if t == 2:
                mine.append(own_asked[1])
            kt[p] = np.unique(np.array(mine, np.uint64))
        keys.append(kt)
        cnt.append({p: np.ones(len(kt[p]), np.float32) for p in kt})
    o = np.argsort(ikeys)
    return dict(keys=keys, cnt=cnt, imported=(ikeys[o], scal[o], has[o], V[o]), kinds=kinds, own_asked=own_asked, Q=Q)


def walk(oracle, S, r=1, plan=None, order="overlap", train=(True, True, True), have=(True, True, True)):
    """ONE oracle store through the stream in the documented order of the schedule -> dict(so, rows [t]{p} = the rows rank r
    answers with, grads [t]{p} = the gradient rows the peers push (flags as pulled), keys, cnt, imported, shard_keys, train, have).
    order "overlap": L(t) count push | t = 0: R(0) | own gradient | R(t+1) | P(t);  "sync": L(t) | R(t) | own gradient | P(t).
    The weights every step sees are asserted to be, bit for bit, what its design's check() ran on."""
    from oracle import bindings as ob
    k, push_cnt, designs = S["V_dim"], S["push_cnt"], S["designs"]
    stride = _stride(k)
    so = oracle.store_create(init_mode=ob.INIT_HASH, V_dim=k, **designs[0]["hyper"])
    for D in designs:
        assert D["hyper"] == designs[0]["hyper"]
        for u, key in enumerate(D["keys"]):
            so.poke(int(key), *D["scal"][u], D["V"][u] if D["has_V"][u] else None)
    none = {p: np.zeros(0, np.uint64) for p in range(W) if p != r}
    pkeys = plan["keys"] if plan else [none] * 3
    pcnt = plan["cnt"] if plan else [{p: np.zeros(0, np.float32) for p in none}] * 3
    imported = plan["imported"] if plan else (np.zeros(0, np.uint64), np.zeros((0, 4), np.float32), np.zeros(0, np.int32), np.zeros((0, 2 * k), np.float32))
    for i, key in enumerate(imported[0]):
        so.poke(int(key), *imported[1][i], imported[3][i] if imported[2][i] else None)
    peers = sorted(none)
    rows, grads, push = [{} for _ in range(3)], [{} for _ in range(3)], [{} for _ in range(3)]
    grng = [np.random.default_rng([911, k, int(push_cnt), t]) for t in range(3)]

    def R(t):
        if push_cnt:
            for p in peers:
                if len(pkeys[t][p]):
                    so.push(pkeys[t][p], ob.FEA_COUNT, pcnt[t][p])
        for p in peers:
            n = len(pkeys[t][p])
            G = E._random_grad(grng[t], n * (1 + k)).reshape(n, 1 + k)     # drawn whatever the lengths: the same in both orders
            if n == 0:
                rows[t][p], grads[t][p], push[t][p] = np.zeros((0, stride), np.float32), np.zeros((0, stride), np.float32), None
                continue
            vals, lens = so.pull(pkeys[t][p])
            lens = lens if k else np.ones(n, np.int32)
            rows[t][p] = T.exchange_rows(vals, lens, k, stride)
            ragged = np.concatenate([G[i, :1 + (k if lens[i] > 1 else 0)] for i in range(n)])
            grads[t][p] = E._rows_from_ragged(ragged, lens, rows[t][p][:, 1], k, stride)
            push[t][p] = (ragged, lens)

    def P(t):
        for p in peers:     # ascending source rank
            if push[t][p] is not None:
                so.push(pkeys[t][p], ob.GRADIENT, push[t][p][0], push[t][p][1] if k else None)

    for t, D in enumerate(designs):
        want = E.expected(oracle, D)
        if have[t]:
            if push_cnt:
                so.push(D["keys"], ob.FEA_COUNT, D["cnt"])
            vals, lens = so.pull(D["keys"])
            assert k == 0 or np.array_equal(lens, want["lens"]), "minibatch %d: the lengths the step sees" % t
            same_bits(vals, want["pulled"], "minibatch %d: the weights the step sees against those check() ran on" % t)
        if order == "sync" or t == 0:
            R(t)
        if have[t] and train[t]:
            so.push(D["keys"], ob.GRADIENT, X.ragged_gradient(want["gw"], want["gV"], want["lens"], k), want["lens"] if k else None)
        if order == "overlap" and t + 1 < 3:
            R(t + 1)
        if train[t]:
            P(t)
    lo, hi = _range(S, r)
    asked = np.concatenate([pkeys[t][p] for t in range(3) for p in peers] + [np.zeros(0, np.uint64)])
    mine = np.concatenate([D["keys"][(D["keys"] >= lo) & (D["keys"] <= hi)] for D in designs])
    return dict(so=so, rows=rows, grads=grads, keys=pkeys, cnt=pcnt, imported=imported, train=tuple(train), have=tuple(have), order=order,
                shard_keys=np.unique(np.concatenate([mine, imported[0], asked])), rank=r)


def _stride(k):
    """dfh_row_stride: [w, has_V, 0, 0 | V padded to a multiple of 4] (run_stream asserts it against the library's)"""
    return 4 + ((k + 3) // 4) * 4


def _range(S, r):
    """[lo, hi] of rank r, both inclusive"""
    s0, s1 = S["splits"]
    return (np.uint64(0) if r == 0 else (s0 if r == 1 else s1)), (np.uint64(2 ** 64 - 1) if r == 2 else ((s0 if r == 0 else s1) - np.uint64(1)))


# ================================================================== CPU: the script
def test_stream_peers_refuse_a_wrong_size_and_a_wrong_turn():
    """CPU: the stream script's state machine — three steps of rank 1 of 3 under the overlap schedule with the right sizes in
    the right order pass; four bytes more in any exchange raise; an exchange of the right size in another minibatch's turn
    raises (ROWS(t+1) ahead of GRADS(t), GRADS(t) ahead of KEYS(t+1))"""
    stride = 8
    npeer = [2, 1, 3]        # keys peer 0 sends with minibatch t (peer 2: none)
    nsend = [(3, 1), (2, 2), (1, 4)]

    def stream():
        return [dict(peer_keys={0: np.arange(npeer[t], dtype=np.uint64) + 10 * t}, peer_cnt={0: np.ones(npeer[t], np.float32)},
                     peer_grads={0: np.full((npeer[t], stride), t, np.float32)},
                     rows_of=lambda p, keys, t=t: np.full((len(keys), stride), 10 * t + p, np.float32)) for t in range(3)]

    plan = StreamPeers.make_plan([True] * 3, [True] * 3, True)
    assert plan == [("COUNTS", 0), ("KEYS", 0), ("CNT", 0), ("ROWS", 0), ("COUNTS", 1), ("KEYS", 1), ("CNT", 1), ("GRADS", 0), ("ROWS", 1),
                    ("COUNTS", 2), ("KEYS", 2), ("CNT", 2), ("GRADS", 1), ("ROWS", 2), ("GRADS", 2)]
    assert StreamPeers.make_plan([True] * 3, [True, False, True], False) == [
        ("COUNTS", 0), ("KEYS", 0), ("ROWS", 0), ("COUNTS", 1), ("KEYS", 1), ("GRADS", 0), ("ROWS", 1), ("COUNTS", 2), ("KEYS", 2), ("ROWS", 2), ("GRADS", 2)]
    assert StreamPeers.make_plan([True, True, False], [True] * 3, False) == [
        ("COUNTS", 0), ("KEYS", 0), ("ROWS", 0), ("COUNTS", 1), ("KEYS", 1), ("GRADS", 0), ("ROWS", 1), ("COUNTS", 2), ("GRADS", 1)]
    assert StreamPeers.make_plan([True] * 2, [True] * 2, True, "sync") == [
        ("COUNTS", 0), ("KEYS", 0), ("CNT", 0), ("ROWS", 0), ("GRADS", 0), ("COUNTS", 1), ("KEYS", 1), ("CNT", 1), ("ROWS", 1), ("GRADS", 1)]

    def sizes(kind, t):
        a, c = nsend[t]
        n = npeer[t]
        unit = {"KEYS": 8, "CNT": 4, "ROWS": 4 * stride, "GRADS": 4 * stride}.get(kind)
        if kind == "COUNTS":
            return [16] * 3, [16] * 3
        if kind == "ROWS":
            return [unit * n, 0, 0], [unit * a, 0, unit * c]
        return [unit * a, 0, unit * c], [unit * n, 0, 0]

    def play(order, tamper=None):
        sp = StreamPeers(1, 3, stride, True, stream())
        for kind, t in order:
            sb, rb = sizes(kind, t)
            send = np.zeros(sum(sb), np.uint8)
            if kind == "COUNTS":
                send[:] = np.array([[nsend[t][0], 1], [7, 1], [nsend[t][1], 1]], np.int64).view(np.uint8).reshape(-1)
            if (kind, t) == tamper:
                sb = [sb[0] + 4] + sb[1:]
                send = np.concatenate([send, np.zeros(4, np.uint8)])
            recv = np.zeros(sum(rb), np.uint8)
            sp.exchange(send, sb, recv, rb)
            if kind == "COUNTS":
                assert recv.view(np.int64).reshape(3, 2).tolist() == [[npeer[t], 1], [7, 1], [0, 1]]
            if kind == "ROWS":
                assert recv.view(np.float32).reshape(-1, stride)[:, 0].tolist() == [10 * t] * nsend[t][0] + [10 * t + 2] * nsend[t][1]
            if kind == "GRADS":
                assert recv.view(np.float32).reshape(-1, stride)[:, 0].tolist() == [t] * npeer[t]
        assert sp.finished() and sorted(sp.sent) == sorted((t, kind) for kind, t in plan if kind != "COUNTS")
        assert sorted(sp.supplied) == sorted((t, kind) for kind, t in plan)
        with pytest.raises(AssertionError):
            sp.exchange(np.zeros(48, np.uint8), [16] * 3, np.zeros(48, np.uint8), [16] * 3)

    play(plan)
    for x in plan:
        with pytest.raises(AssertionError):
            play(plan, tamper=x)
    # the right sizes in the wrong turn.  (minibatches 0 and 1 differ in every size, so the size check sees the swap as well:
    # make the turn the only difference by giving both minibatches one shape)
    npeer[:] = [2, 2, 2]
    nsend[:] = [(3, 1)] * 3
    play(plan)
    i, j = plan.index(("GRADS", 0)), plan.index(("ROWS", 1))
    swapped = plan[:i] + [plan[j], plan[i]] + plan[j + 1:]
    assert j == i + 1 and sizes("GRADS", 0)[0] == sizes("ROWS", 1)[1]
    with pytest.raises(AssertionError):
        play(swapped)
    i, j = plan.index(("KEYS", 1)), plan.index(("GRADS", 0))
    with pytest.raises(AssertionError):
        play(plan[:i] + [plan[j]] + plan[i:j] + plan[j + 1:])
    # a rank that says it has a minibatch where the stream has none for it
    sp = StreamPeers(1, 3, stride, False, [dict(have=False)])
    with pytest.raises(AssertionError):
        sp.exchange(np.array([[0, 1]] * 3, np.int64).view(np.uint8).reshape(-1), [16] * 3, np.zeros(48, np.uint8), [16] * 3)
    assert sp.error is not None


# ================================================================== CPU: the streams
@pytest.mark.parametrize("V_dim,push_cnt", STREAMS, ids=STREAM_IDS)
def test_streams_hold_their_design_conditions(oracle, V_dim, push_cnt):
    """CPU: three disjoint designs (valued, binary, valued); split keys near thirds with own keys and remote keys on both sides in
    every minibatch and every class of occurrences own and remote over the stream (per minibatch where the search found it);
    11 split entries per minibatch; the peers' keys are of every kind, in no minibatch, inside the range; the designed keys
    exist and do what they are designed for on the oracle store; the weights every step sees are those of its check()"""
    S = make_stream(V_dim, push_cnt)
    designs, offs, union = S["designs"], S["offs"], S["union"]
    k = V_dim
    assert [D["binary"] for D in designs] == list(BINARY) and all(D["push_cnt"] == push_cnt and D["V_dim"] == V_dim for D in designs)
    assert len(union) == sum(len(D["keys"]) for D in designs)
    a, b = S["at"]
    assert abs(a - len(union) // 3) + abs(b - 2 * len(union) // 3) <= len(union) // 3, "the range is far from thirds: %r of %d" % (S["at"], len(union))
    assert stream_ok(designs, offs)
    if S["per_minibatch"]:
        assert all(T.split_ok(D["cnt"].astype(np.int64), o) for D, o in zip(designs, offs))
    for D in designs:
        assert split_entries_expected(D["cnt"]) == 5 + 6
    plan = peer_plan(S)
    s0, s1 = S["splits"]
    kinds = plan["kinds"]
    for name, q in kinds.items():
        assert not np.isin(q, union).any() and q.min() >= s0 and q.max() < s1, name
    ik, iscal, ihas, iV = plan["imported"]
    assert not np.isin(kinds["PU"], ik).any() and np.isin(kinds["PV"], ik).all() and np.isin(kinds["PN"], ik).all()
    assert k == 0 or (ihas[np.isin(ik, kinds["PV"])].all() and not ihas[~np.isin(ik, kinds["PV"])].any())
    assert np.all(iscal[:, 1] != 0)
    sent = [{p: plan["keys"][t][p] for p in (0, 2)} for t in range(3)]
    for t in range(3):
        for p in (0, 2):
            q = sent[t][p]
            assert len(q) and np.all(q[1:] > q[:-1]) and q.min() >= s0 and q.max() < s1
            assert not np.isin(q, designs[t]["keys"]).any(), "a peer asks for a key of the minibatch under way"
            for name in ("PV", "PN", "PU"):
                assert np.isin(kinds[name], q).any(), (t, p, name)
        both = np.intersect1d(sent[t][0], sent[t][2])
        for name in ("PV", "PN", "PU"):
            assert np.isin(kinds[name], both).any(), "minibatch %d: no key of kind %s from both peers" % (t, name)
    asked = lambda t: np.union1d(sent[t][0], sent[t][2])
    every = np.intersect1d(np.intersect1d(asked(0), asked(1)), asked(2))
    for name in ("PV", "PN", "PU"):
        assert np.isin(kinds[name], every).any(), "no key of kind %s is asked for in every step" % name
    late = np.setdiff1d(asked(1), asked(0))
    assert np.isin(kinds["PU"], late).any() or np.isin(kinds["PN"], late).any()
    assert np.isin(asked(2), np.union1d(np.union1d(asked(0), asked(1)), union)).all(), "a key appears with the third minibatch only"
    o0, o1 = plan["own_asked"]
    assert o0 in designs[0]["keys"][offs[0][1]:offs[0][2]] and o0 in sent[1][2] and o0 in sent[2][2] and o0 not in asked(0)
    assert o1 in designs[1]["keys"][offs[1][1]:offs[1][2]] and o1 in sent[2][0] and o1 in sent[2][2] and o1 not in asked(1)

    over = walk(oracle, S, 1, plan)
    sync = walk(oracle, S, 1, plan, order="sync")
    stride = _stride(k)
    # a key with GRADS(0) asked for again with minibatch 1: the overlap order answers with the state BEFORE P(0), the sync order
    # with the state after it; with minibatch 2 both have applied P(0), but the overlap order not yet P(1)
    differ = 0
    for t in (1, 2):
        for p in (0, 2):
            again = np.isin(sent[t][p], asked(t - 1))
            d = (bits(over["rows"][t][p]) != bits(sync["rows"][t][p])).any(1)
            assert not d[~again & ~np.isin(sent[t][p], union)].any(), "a key without a gradient under way differs between the orders"
            assert d[again].any(), "minibatch %d, peer %d: the two orders answer with the same rows" % (t, p)
            differ += int(d.sum())
    assert differ >= 8
    for p in (0, 2):     # ROWS(1) of a key asked for in steps 0 and 1 = ROWS(0) but for the count: w, V untouched by P(0)
        j1 = np.flatnonzero(np.isin(sent[1][p], sent[0][p]) & np.isin(sent[1][p], np.concatenate([kinds["PV"], kinds["PN"]])))
        j0 = np.searchsorted(sent[0][p], sent[1][p][j1])
        assert len(j1)
        same_bits(over["rows"][1][p][j1], over["rows"][0][p][j0], "ROWS(1) against ROWS(0) at the keys asked for twice")
    # the own key of minibatch 0: the row answered with minibatch 1 shows the own in-place update of step 0
    want0 = E.expected(oracle, designs[0])
    u = int(np.searchsorted(designs[0]["keys"], o0))
    j = int(np.searchsorted(sent[1][2], o0))
    w_after = want0["model"][0][u, 1]
    same_bits(over["rows"][1][2][j, :1], np.array([w_after], np.float32), "the own key of step 0 as answered in ROWS(1)")
    assert bits(designs[0]["scal"][u, 1:2])[0] != bits(np.array([w_after], np.float32))[0], "step 0 does not move the own key a peer asks for"
    if "PX" in kinds:
        x = kinds["PX"][0]
        thr = designs[0]["hyper"]["V_threshold"]
        j0, j1 = int(np.searchsorted(sent[0][0], x)), int(np.searchsorted(sent[1][0], x))
        r0, r1 = over["rows"][0][0][j0], over["rows"][1][0][j1]
        assert r0[1] == 0 and not bits(r0[4:]).any() and r0[0] != 0, "PX is pulled without V with minibatch 0"
        hv = np.array([oracle.L.orc_hash_init_value(int(x), d, designs[0]["hyper"]["seed"], designs[0]["hyper"]["V_init_scale"]) for d in range(k)], np.float32)
        assert r1[1] == 1 and bits(r1[0:1])[0] == bits(r0[0:1])[0], "PX has its V with minibatch 1, w as before P(0)"
        same_bits(r1[4:4 + k], hv, "PX: the freshly initialised V in ROWS(1)")
        g0 = over["grads"][0][0][j0]
        assert g0[1] == 0 and g0[0] != 0 and not bits(g0[4:]).any(), "GRADS(0) carry PX's row as pulled without V"
        e = over["so"].peek(int(x))
        assert e["fea_cnt"] == thr + 2 and e["V"] is not None
        j2 = int(np.searchsorted(sent[2][0], x))
        r2 = over["rows"][2][0][j2]
        assert bits(r2[0:1])[0] != bits(r1[0:1])[0], "P(0) moved PX's w"
        same_bits(r2[4:4 + k], hv, "PX: P(0) is a push of length 1, V stays the initial one until P(1)")
    else:
        assert not (push_cnt and k > 0)
    assert np.array_equal(over["shard_keys"], np.unique(np.concatenate([union[(union >= s0) & (union < s1)], ik, kinds["PU"]])))


def test_narrow_range_leaves_b_without_own_keys():
    """CPU: the range of the degenerate case — B has no key in it, A and C have, every minibatch has remote keys on both sides"""
    S = narrow_stream(make_stream(5, True))
    offs = S["offs"]
    assert offs[1][1] == offs[1][2] and all(o[1] > 0 and o[2] < o[3] for o in offs)
    assert offs[0][2] - offs[0][1] >= 1 and offs[2][2] - offs[2][1] >= 1


# ================================================================== one rank, one stream
class _StepView:
    """what scripted_peers.ScriptedPeers holds after one step, out of a StreamPeers: for test_sharded_exact.assert_worker_side"""

    def __init__(self, sp, t):
        self.peers, self.counts = sp.peers, sp.counts[t]
        self.sent = {kind: v for (m, kind), v in sp.sent.items() if m == t}


def run_stream(capi, S, exp, options=(), pipeline=False, schedule="overlap", end=False, snapshots=False, replay=None, read_between=False):
    """rank exp["rank"] of W through the stream on a context of its own: the model of its range imported (the designs' keys and
    the peers' imported ones), two batch objects in rotation, every following minibatch announced before the step (overlap),
    the peers a StreamPeers script — or, replay = a finished script: the loop-back transport fed with what that script
    supplied, a batch object per minibatch and no read between the steps (the host waits for the counts alone).
    -> dict(pred [t], split_entries [t], peers, model, snaps, progress [j] = progress(reset=True) of batch object j once the
    stream is through, steps_of [j] = the minibatches it took).  read_between: progress(reset=False) of the step's batch object
    after every step, which adds the step's AUC slots up; without it the batch object's next step takes them up"""
    r = exp["rank"]
    k, push_cnt, designs, offs = S["V_dim"], S["push_cnt"], S["designs"], S["offs"]
    stride = capi.row_stride(k)
    assert stride == _stride(k)
    lo, hi = _range(S, r)
    rows_all = [T.pulled_rows(capi, D, E._EXPECTED[id(D)]) for D in designs]

    def rows_of_step(t):
        def rows_of(p, sent):
            i = np.searchsorted(designs[t]["keys"], sent)
            assert np.array_equal(designs[t]["keys"][i], sent), "keys sent to rank %d that are not minibatch %d's" % (p, t)
            return rows_all[t][i]
        return rows_of

    stream = [dict(have=exp["have"][t], is_train=exp["train"][t], peer_keys=exp["keys"][t], peer_cnt=exp["cnt"][t],
                   peer_grads=exp["grads"][t] if exp["train"][t] else None, rows_of=rows_of_step(t)) for t in range(3)]
    if end:
        stream.append(dict(have=False, peers_have=False))
    peers = StreamPeers(r, W, stride, push_cnt, stream, schedule)
    c = capi.Context(0)
    objs = []
    try:
        for name, v in options:
            c.set_option(name, v)
        if replay is None:
            comm = capi.Comm.callback(c, r, W, peers.exchange)
        else:
            comm = capi.Comm.loopback(c, r, W)
            comm.wire(WIRE_GBPS, WIRE_LATENCY_US)
        objs.append(comm)
        tb = capi.Table(c, 4096, V_dim=k, init_mode=capi.INIT_HASH, **designs[0]["hyper"])
        objs.append(tb)
        parts = [(D["keys"][m], D["scal"][m], D["has_V"][m], D["V"][m]) for D in designs for m in [(D["keys"] >= lo) & (D["keys"] <= hi)]]
        parts.append(exp["imported"])
        ikeys = np.concatenate([x[0] for x in parts])
        o = np.argsort(ikeys)
        tb.import_(ikeys[o], np.concatenate([x[1] for x in parts])[o], np.concatenate([x[2] for x in parts])[o],
                   np.concatenate([x[3] for x in parts])[o] if k else None)
        nrows = max(len(D["label"]) for D in designs)
        nnz = max(len(D["index"]) for D in designs)
        nbt = 2 if replay is None else 3       # the replay reloads no batch object: nothing makes the host wait between its steps
        bts = [capi.Batch(c, nrows, nnz + 64) for _ in range(nbt)]
        objs += bts
        for b_ in bts:
            b_.set_option("compute_auc", 1)       # as the sharded learner sets it
        sh = capi.Shard(tb, comm, S["splits"])
        objs.append(sh)
        if schedule == "overlap":
            sh.set_exchange("overlap")
        if pipeline:
            c.set_pipeline(1)
        if replay is not None:
            _feed(capi, c, comm, replay, S, r, stride, objs)

        def prepare(t):
            if t >= 3 or not exp["have"][t]:
                return None
            D = designs[t]
            bts[t % nbt].load_host(D["offset"], D["index"], D["value"], D["label"])
            bts[t % nbt].localize()
            return bts[t % nbt]

        def step(bt, **kw):
            try:
                return sh.step(bt, **kw)
            except capi.DfhError:
                if peers.error is not None:
                    raise peers.error
                raise

        out = dict(pred=[], split_entries=[], peers=peers, snaps=[])
        used = []

        def read(t):
            out["pred"].append(used[t].pred().copy() if used[t] is not None else None)
            out["split_entries"].append(used[t].split_entries() if used[t] is not None and exp["train"][t] else None)

        cur = prepare(0)
        for t in range(3):
            nxt = prepare(t + 1)
            if schedule == "overlap" and (t + 1 < 3 or end):
                sh.prefetch_counts(nxt)
            assert step(cur, is_train=exp["train"][t], push_cnt=push_cnt), "step %d says that nobody had a minibatch" % t
            used.append(cur)
            cur = nxt
            if replay is not None:
                continue        # logits and split lists are read once the whole stream is queued
            assert peers.done_steps(t + 1), "step %d stopped after %d exchanges of %r" % (t, peers.pos, peers.steps)
            c.sync()
            read(t)
            if read_between and used[t] is not None:
                used[t].progress(reset=False)
            if snapshots:
                out["snaps"].append(E.device_model(tb))
        if end:
            before = peers.pos
            assert not step(None, is_train=True, push_cnt=push_cnt), "a step after the epoch's end says that somebody has a minibatch"
            assert peers.pos == before, "the step after the epoch's end made an exchange"
            sh.set_exchange("sync")      # refused while a minibatch is under way
        assert replay is not None or peers.finished(), "the stream stopped after %d exchanges of %r" % (peers.pos, peers.plan)
        c.sync()
        if replay is not None:
            for t in range(3):
                read(t)
            out["wire_us"] = comm.wire_time_us()
        out["steps_of"] = [[t for t in range(3) if used[t] is bts[j]] for j in range(nbt)]
        reads = [(b_.progress(reset=False), b_.progress(reset=False)) for b_ in bts]
        out["progress"] = [b_.progress(reset=True) for b_ in bts]
        out["reads"] = [reads[j] + (bts[j].progress(reset=False),) for j in range(nbt)]
        tb.check()
        out["model"] = E.device_model(tb)
        assert tb.size() == len(out["model"][0])
        return out
    finally:
        for o_ in objs[::-1]:
            o_.close()
        c.close()


def _feed(capi, c, comm, sp, S, r, stride, keep):
    """every exchange of the finished script `sp`, per kind in minibatch order, with exactly the bytes it supplied: laid out
    like the receive side — one peer after the other, ROWS at the place of the peer's keys among the minibatch's"""
    kind_id = dict(COUNTS=capi.XCHG_COUNTS, KEYS=capi.XCHG_KEYS, CNT=capi.XCHG_CNT, ROWS=capi.XCHG_ROWS, GRADS=capi.XCHG_GRADS)
    for kind, m in sp.plan:
        data, rb = sp.supplied[(m, kind)]
        if kind == "ROWS":
            off = np.concatenate([[0], np.cumsum(sp.counts[m][:, 0])]).astype(np.int64)
            full = np.zeros((int(off[-1]), 4 * stride), np.uint8)
            o = 0
            for p in range(W):
                assert rb[p] == (0 if p == r else 4 * stride * (off[p + 1] - off[p]))
                full[off[p]:off[p] + rb[p] // (4 * stride)] = data[o:o + rb[p]].reshape(-1, 4 * stride)
                o += rb[p]
            data = full.reshape(-1)
        if len(data) < 16:
            data = np.concatenate([data, np.zeros(16 - len(data), np.uint8)])
        d = capi.DeviceBuffer.from_numpy(c, np.ascontiguousarray(data))
        keep.append(d)
        comm.feed(kind_id[kind], d.ptr)


def assert_steps_sent(capi, oracle, got, S, exp, what, split=True, model=True):
    """per step: the COUNTS words, KEYS, CNT and every word of the GRADS rows sent, the logits, the split list
    (test_sharded_exact.assert_worker_side on the step's part of the script's record); model: the step's own keys out of the
    final table against the design's own expected model (a run in which no peer asks for them)"""
    r = exp["rank"]
    for t, D in enumerate(S["designs"]):
        if not exp["have"][t]:
            assert got["pred"][t] is None
            continue
        want = E.expected(oracle, D)
        off = S["offs"][t]
        w = "%s, step %d" % (what, t)
        view = dict(peers=_StepView(got["peers"], t), pred=got["pred"][t], split_entries=got["split_entries"][t])
        same_bits(view["pred"], want["pred"], "%s: logits against clip(exact)" % w)
        lo, hi = off[r], off[r + 1]
        if exp["train"][t]:
            if model:
                dk = got["model"][0]
                m = np.isin(dk, D["keys"][lo:hi])
                view["model"] = tuple(x[m] for x in got["model"])
            else:       # the step's own keys are compared with the whole shard against the stream's oracle store
                view["model"] = (D["keys"][lo:hi],) + tuple(x[lo:hi] for x in want["model"])
            T.assert_worker_side(capi, view, D, want, r, off, w, split=split)
        else:
            peers = view["peers"]
            assert peers.counts.tolist() == [[off[p + 1] - off[p], 1] for p in range(W)] and "GRADS" not in peers.sent
            for p in peers.peers:
                assert np.array_equal(peers.sent["KEYS"][p], D["keys"][off[p]:off[p + 1]])
    assert_stream_progress(oracle, got, S, what)


def assert_stream_progress(oracle, got, S, what):
    """per batch object: the sums over the minibatches it took, as the API rounds them (the doubles added up, then the cast),
    against the designs' exact_progress — a validation step's among them: the same loss, its penalty through k_penalty, once
    for the pulled rows and once for the own keys"""
    for j, steps in enumerate(got["steps_of"]):
        want = X.accepted([E.expected(oracle, S["designs"][t])["progress"] for t in steps])
        w = "%s, batch object %d (minibatches %r)" % (what, j, steps)
        X.assert_progress(got["progress"][j], want, w)
        E.assert_reads(dict(reads=got["reads"][j], progress=got["progress"][j]), w)


def assert_owner_side(got, exp, k, what):
    """the rows answered per step and peer and the whole shard against the oracle store that took the schedule's order"""
    sp = got["peers"]
    for t in range(3):
        for p in sp.peers:
            same_bits(sp.sent[(t, "ROWS")][p], exp["rows"][t][p], "%s: ROWS(%d) answered to rank %d" % (what, t, p))
    T.assert_shard(got["model"], exp["shard_keys"], E.oracle_model(exp["so"], exp["shard_keys"], k), k, what)


def same_run(a, b, what):
    """two runs of one stream: logits, everything sent, the shard"""
    for t in range(3):
        assert (a["pred"][t] is None) == (b["pred"][t] is None)
        if a["pred"][t] is not None:
            same_bits(a["pred"][t], b["pred"][t], "%s: logits of step %d" % (what, t))
    assert sorted(a["peers"].sent) == sorted(b["peers"].sent), what
    for key, by_peer in a["peers"].sent.items():
        for p, v in by_peer.items():
            w = b["peers"].sent[key][p]
            assert v.shape == w.shape and np.array_equal(v.view(np.uint8), w.view(np.uint8)), "%s: %s(%d) sent to rank %d" % (what, key[1], key[0], p)
    same_model(a["model"], b["model"], what)


def same_model(a, b, what):
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[2] != 0, b[2] != 0), "%s: keys, has_V" % what
    same_bits(a[1], b[1], "%s: scalars" % what)
    same_bits(a[3], b[3], "%s: V | acc" % what)


_EXP = {}


def expectations(oracle, S, r=1, owner=True, order="overlap", train=(True, True, True), have=(True, True, True)):
    key = (S["V_dim"], S["push_cnt"], S["variant"], tuple(S["splits"].tolist()), r, owner, order, train, have)
    if key not in _EXP:
        _EXP[key] = walk(oracle, S, r, peer_plan(S) if owner else None, order, train, have)
    return _EXP[key]


# ================================================================== a. the worker side
@pytest.mark.gpu
@pytest.mark.parametrize("V_dim,push_cnt", STREAMS, ids=STREAM_IDS)
def test_worker_side_of_a_stream_bit_exact(capi, oracle, V_dim, push_cnt):
    """rank 1 runs A, B, C under the overlap schedule, the peers sending no keys: per step the COUNTS words, KEYS, CNT, every
    word of every GRADS row, the logits and 11 split entries; afterwards the whole shard — exactly the imported keys — against
    the oracle store of the stream and each step's own keys against its design's expected model"""
    S = make_stream(V_dim, push_cnt)
    exp = expectations(oracle, S, 1, owner=False)
    got = run_stream(capi, S, exp)
    assert_steps_sent(capi, oracle, got, S, exp, "rank 1")
    assert_owner_side(got, exp, V_dim, "rank 1")


@pytest.mark.gpu
@pytest.mark.parametrize("r", [0, 2])
def test_worker_side_of_a_stream_as_the_outer_ranks(capi, oracle, r):
    """the same as ranks 0 and 2 (V_dim 5, with counts): every key takes the remote path under the folded lookup"""
    S = make_stream(5, True)
    exp = expectations(oracle, S, r, owner=False)
    got = run_stream(capi, S, exp)
    assert_steps_sent(capi, oracle, got, S, exp, "rank %d" % r)
    assert_owner_side(got, exp, 5, "rank %d" % r)


# ================================================================== b. the owner side
@pytest.mark.gpu
@pytest.mark.parametrize("V_dim,push_cnt", STREAMS, ids=STREAM_IDS)
@pytest.mark.parametrize("per_key", [0, 1], ids=["per_entry", "per_key"])
def test_owner_side_of_a_stream_bit_exact(capi, oracle, V_dim, push_cnt, per_key):
    """rank 1 serves its peers while two minibatches are in flight (owner_per_key 0 and 1): ROWS(t) answered per step and peer
    — before P(t-1), after P(t-2), the freshly initialised V of the key whose count crosses the threshold — and the final shard,
    peer-only and new keys included, against the one oracle store in the documented order; the worker side as without peers' keys"""
    S = make_stream(V_dim, push_cnt)
    exp = expectations(oracle, S)
    got = run_stream(capi, S, exp, options=(("owner_per_key", per_key),))
    what = "owner side, %s" % ("per key" if per_key else "per entry")
    assert_owner_side(got, exp, V_dim, what)
    assert_steps_sent(capi, oracle, got, S, exp, what, model=False)


# ================================================================== c. the switches
STREAM_SWITCHES = {
    "mixed_update0": dict(options=(("shard_mixed_update", 0),)),
    "upd_split0": dict(options=(("upd_split", 0),), split=False),
    "upd_kernel0": dict(options=(("upd_kernel", 0),), split=False),
    "single_queue": dict(options=(("single_queue", 1),)),
    "pipeline": dict(pipeline=True),
}


@pytest.mark.gpu
def test_stream_under_every_switch_gives_the_same_bytes(capi, oracle):
    """V_dim 5 with counts, peers' keys included, under shard_mixed_update = 0, upd_split = 0, upd_kernel = 0, single_queue = 1
    and set_pipeline(1): the default run's bytes and the oracle's; without splitting the split list stays empty"""
    S = make_stream(5, True)
    exp = expectations(oracle, S)
    base = run_stream(capi, S, exp)
    assert_owner_side(base, exp, 5, "default")
    for name, sw in STREAM_SWITCHES.items():
        got = run_stream(capi, S, exp, options=sw.get("options", ()), pipeline=sw.get("pipeline", False))
        same_run(got, base, "%s against the default" % name)
        assert_owner_side(got, exp, 5, name)
        assert_steps_sent(capi, oracle, got, S, exp, name, split=sw.get("split", True), model=False)
        assert got["split_entries"] == [11 if sw.get("split", True) else 0] * 3


# ================================================================== d. degenerate flights
@pytest.mark.gpu
def test_minibatch_without_own_keys(capi, oracle):
    """a range in which B has no key: its step launches no L and takes k_uw_remote in F, C folds again; every byte as ever"""
    S = narrow_stream(make_stream(5, True))
    exp = expectations(oracle, S, 1, owner=False)
    got = run_stream(capi, S, exp)
    assert got["peers"].counts[1][1, 0] == 0 and got["peers"].counts[0][1, 0] > 0 and got["peers"].counts[2][1, 0] > 0
    assert_steps_sent(capi, oracle, got, S, exp, "narrow range")
    assert_owner_side(got, exp, 5, "narrow range")


@pytest.mark.gpu
def test_rank_out_of_data_still_serves_its_range(capi, oracle):
    """step(None) for the third minibatch while the peers have one and send keys: only R and P run; rows and shard exact"""
    S = make_stream(5, True)
    exp = expectations(oracle, S, have=(True, True, False))
    got = run_stream(capi, S, exp)
    assert got["peers"].counts[2].tolist() == [[0, 0]] * 3 and got["pred"][2] is None
    assert_owner_side(got, exp, 5, "out of data")
    assert_steps_sent(capi, oracle, got, S, exp, "out of data", model=False)


@pytest.mark.gpu
def test_validation_step_between_two_training_steps(capi, oracle):
    """B with is_train = False (no counts: a validation pass pushes none): its logits are exact, the table is bit-identical
    before and after it, no GRADS(1) is exchanged (the script's plan has none), the rows R resolved are released — C afterwards
    is exact and the table's check passes"""
    S = make_stream(5, False)
    exp = expectations(oracle, S, train=(True, False, True))
    got = run_stream(capi, S, exp, snapshots=True)
    assert ("GRADS", 1) not in got["peers"].plan and (1, "GRADS") not in got["peers"].sent
    same_model(got["snaps"][1], got["snaps"][0], "the table after the validation step against the table before it")
    assert_owner_side(got, exp, 5, "validation step")
    assert_steps_sent(capi, oracle, got, S, exp, "validation step", model=False)


@pytest.mark.gpu
def test_epoch_end_leaves_nothing_under_way(capi, oracle):
    """prefetch_counts(None) before the last step with peers that have nothing either: the step after it returns False without
    an exchange, and set_exchange("sync") is accepted: no minibatch is under way"""
    S = make_stream(5, True)
    exp = expectations(oracle, S)
    got = run_stream(capi, S, exp, end=True)
    assert got["peers"].plan[-2:] == [("COUNTS", 3), ("GRADS", 2)]
    assert_owner_side(got, exp, 5, "epoch's end")


@pytest.mark.gpu
def test_sync_schedule_on_the_same_stream(capi, oracle):
    """the same stream under the sync schedule: the worker side sends the overlap run's bytes (the keys are disjoint, the rows
    scripted); the rows answered are those of the sync order (test_shard_native.emulate) and DIFFER from the overlap order's at
    the keys asked for while their gradient is under way — the designed keys tell the two orders apart"""
    S = make_stream(5, True)
    over, sync = expectations(oracle, S), expectations(oracle, S, order="sync")
    a = run_stream(capi, S, over)
    b = run_stream(capi, S, sync, schedule="sync")
    assert_owner_side(a, over, 5, "overlap")
    assert_owner_side(b, sync, 5, "sync")
    assert_steps_sent(capi, oracle, b, S, sync, "sync", model=False)
    differ = 0
    for t in range(3):
        same_bits(a["pred"][t], b["pred"][t], "logits of step %d, sync against overlap" % t)
        for p in (0, 2):
            for kind in ("KEYS", "CNT", "GRADS"):
                x, y = a["peers"].sent[(t, kind)][p], b["peers"].sent[(t, kind)][p]
                assert np.array_equal(x.view(np.uint8), y.view(np.uint8)), "%s(%d) to rank %d, sync against overlap" % (kind, t, p)
            differ += int((bits(a["peers"].sent[(t, "ROWS")][p]) != bits(b["peers"].sent[(t, "ROWS")][p])).any(1).sum())
    assert differ >= 8, "the two schedules answered with the same rows: the designed keys do not discriminate"


# ================================================================== e. asynchronous replay
@pytest.mark.gpu
@pytest.mark.parametrize("V_dim,push_cnt", [(5, True), (64, False)], ids=["V5-cnt", "V64-nocnt"])
def test_owner_side_stream_replayed_over_the_loopback_transport(capi, oracle, V_dim, push_cnt):
    """The callback transport drains the collectives' stream at every exchange: it pins arithmetic, bookkeeping and order, and
    hides a missing event between the two streams.  Here the owner-side stream runs once against the script and then over
    capi.Comm.loopback, fed per kind in minibatch order with exactly the bytes the script supplied, where nothing waits on
    the host but the counts and every exchange holds its stream for a modelled 200 us (several times a step's kernels): a
    stage that does not wait for the exchange it needs reads the buffer before the bytes are there.  Logits per step, split
    entries and the final shard must be the script run's bits; they are read once the whole stream is queued (a batch object
    per minibatch), so that nothing but the counts makes the host wait between the steps.  What it cannot show: this transport
    drops what the rank sends, so GRADS and ROWS are seen through the script run alone; and an event whose absence lets a
    stage start early by less than the exchanges queued in front of it on its stream take (the `freed` event of K: two
    exchanges of 200 us lie between P(t) and K(t+2)) — dropping that one was tried and changes no bit here."""
    S = make_stream(V_dim, push_cnt)
    exp = expectations(oracle, S)
    a = run_stream(capi, S, exp)
    assert_owner_side(a, exp, V_dim, "script run")
    b = run_stream(capi, S, exp, replay=a["peers"])
    nonempty = sum(1 for key, (data, rb) in a["peers"].supplied.items() if len(data) or any(len(v) for v in a["peers"].sent.get(key, {}).values()))
    assert nonempty >= 12 and b["wire_us"] >= WIRE_LATENCY_US * nonempty, "the modelled wire held %.0f us for %d exchanges" % (b["wire_us"], nonempty)
    for t in range(3):
        same_bits(b["pred"][t], a["pred"][t], "replay: logits of step %d" % t)
    assert b["split_entries"] == a["split_entries"] == [11] * 3
    same_model(b["model"], a["model"], "replay: the final shard")
    T.assert_shard(b["model"], exp["shard_keys"], E.oracle_model(exp["so"], exp["shard_keys"], V_dim), V_dim, "replay")


# ================================================================== f. the progress sums of a stream
# Every run above asserts loss, AUC and row count per batch object (assert_steps_sent); the streams' hyper-parameters put the
# penalty on no grid.  The "pen" streams are the same minibatches, keys and ranges under l1 = 2^-6, l2 = 0, V_l2 = 2^-5.
@pytest.mark.parametrize("V_dim,push_cnt", STREAMS, ids=STREAM_IDS)
def test_pen_streams_hold_the_progress_conditions(oracle, V_dim, push_cnt):
    """CPU: every design of the "pen" streams passes check() and exact_progress's conditions (expected() runs both), the
    stream's ranges are the base stream's, and the sum of A's and C's doubles — what batch object 0 returns — is accepted as
    at most three floats"""
    S, B = make_stream(V_dim, push_cnt, "pen"), make_stream(V_dim, push_cnt)
    assert np.array_equal(S["splits"], B["splits"]) and S["offs"] == B["offs"]
    P = [E.expected(oracle, D)["progress"] for D in S["designs"]]
    assert all(p["penalty"] is not None for p in P)
    for steps in ([0, 2], [1], [0], [2]):
        acc = X.accepted([P[t] for t in steps])
        assert 1 <= len(acc["penalty"]) <= 3 and 1 <= len(acc["loss"]) <= 3
    if V_dim == 5 and push_cnt:
        N = narrow_stream(S)
        assert N["offs"][1][1] == N["offs"][1][2]


@pytest.mark.gpu
@pytest.mark.parametrize("V_dim,push_cnt", STREAMS, ids=STREAM_IDS)
def test_stream_progress_sums_bit_exact(capi, oracle, V_dim, push_cnt):
    """rank 1 through the "pen" stream, the peers' keys included: batch object 0's sums over A and C and batch object 1's over
    B — loss, penalty (the MIXED update's, own and remote keys), AUC, rows — read only at the end, so that C's step takes up
    A's AUC slots, and in a second run read after every step; the bytes sent and the shard as ever"""
    S = make_stream(V_dim, push_cnt, "pen")
    exp = expectations(oracle, S)
    for rb in (False, True):
        got = run_stream(capi, S, exp, read_between=rb)
        what = "pen stream, read %s" % ("after every step" if rb else "at the end")
        assert got["steps_of"] == [[0, 2], [1]]
        assert_owner_side(got, exp, V_dim, what)
        assert_steps_sent(capi, oracle, got, S, exp, what, model=False)


@pytest.mark.gpu
def test_stream_progress_sums_under_every_switch(capi, oracle):
    """the "pen" stream of V_dim 5 with counts under shard_mixed_update = 0 (two launches: no key's penalty in both, none in
    neither), upd_split = 0, upd_kernel = 0, single_queue = 1 and set_pipeline(1)"""
    S = make_stream(5, True, "pen")
    exp = expectations(oracle, S)
    for name, sw in STREAM_SWITCHES.items():
        got = run_stream(capi, S, exp, options=sw.get("options", ()), pipeline=sw.get("pipeline", False))
        assert_owner_side(got, exp, 5, name)
        assert_steps_sent(capi, oracle, got, S, exp, "pen stream, %s" % name, split=sw.get("split", True), model=False)


@pytest.mark.gpu
def test_stream_progress_sums_without_own_keys_and_in_validation(capi, oracle):
    """the "pen" stream in the narrow range (B has no own key: its penalty is the pulled rows' alone), and with B a validation
    step between two training steps (both k_penalty launches: the pulled rows', then the own keys'), under the mixed update
    and under shard_mixed_update = 0"""
    S = narrow_stream(make_stream(5, True, "pen"))
    exp = expectations(oracle, S, 1, owner=False)
    for opts in ((), (("shard_mixed_update", 0),)):
        assert_steps_sent(capi, oracle, run_stream(capi, S, exp, options=opts), S, exp, "pen stream, narrow range %r" % (opts,))
    S = make_stream(5, False, "pen")
    exp = expectations(oracle, S, train=(True, False, True))
    for opts in ((), (("shard_mixed_update", 0),)):
        got = run_stream(capi, S, exp, options=opts, snapshots=True)
        same_model(got["snaps"][1], got["snaps"][0], "the table after the validation step against the table before it")
        assert_steps_sent(capi, oracle, got, S, exp, "pen stream, validation step %r" % (opts,), model=False)
