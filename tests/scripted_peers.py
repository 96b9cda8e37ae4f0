"""All peers of one rank of the sharded step, played by a script (no second process, no GPU of their own).

capi.Comm.callback hands every exchange of the communicator to a Python function, synchronously, on the calling thread: the
function sees the bytes this rank sends, peer by peer, and supplies the bytes it receives.  ScriptedPeers.exchange is such a
function for the SYNC schedule of dfh_shard_step (shard_step_sync, csrc/dfh_shard.hip), whose exchanges per step are, in
this order:

  COUNTS  16 B per rank, own slot included: int64 {keys I send you, I have a minibatch}
  KEYS    8 B per key: the keys of the minibatch the peer owns, ascending
  CNT     4 B per key, only with push_cnt: their occurrences
  ROWS    row_stride(V_dim) floats per key: sent are the rows of the keys RECEIVED in KEYS, received the rows of the keys SENT
  GRADS   the same sizes the other way round, only when training

The script walks that order, checks the byte counts of every exchange per peer against what the earlier exchanges of the step
imply, records what the rank sent (per kind and peer) and fills the receive side from what the test prepared.  Any mismatch
raises: the trampoline of Comm.callback turns that into a non-zero return code and the step fails with "the host exchange
callback failed" — nothing waits for anybody, so nothing can hang.  The exception itself is kept in `error`.

StreamPeers scripts a STREAM of minibatches 0 .. M-1, under either schedule.  The callback transport drains the stream an
exchange is queued on, calls the function and copies back, so the order in which the host sees the exchanges is the program
order of the schedule.  For the OVERLAP schedule (shard_step_overlap, two minibatches in flight) with every following
minibatch announced by dfh_shard_prefetch_counts before the step that precedes it, that order is

  first step, not announced   COUNTS(0) KEYS(0) [CNT(0)] ROWS(0), then
  step t                      COUNTS(t+1) KEYS(t+1) [CNT(t+1)] GRADS(t) ROWS(t+1)
  last step, nothing announced    GRADS(t)

CNT only with push_cnt, GRADS(t) only when step t trains; after a COUNTS(m) in which nobody has a minibatch no KEYS, CNT or
ROWS of m follow, and no step m: the epoch is over.  (An epoch's end announced with prefetch_counts(None) is a last entry of
the stream that nobody has.)  For the SYNC schedule without announcements every step is COUNTS KEYS [CNT] ROWS [GRADS] of its
own minibatch.  Every exchange of the plan names its minibatch: its byte counts per peer are checked against THAT minibatch's
COUNTS, what was sent is recorded per (minibatch, kind, peer), the receive side is filled from what the test prepared for that
minibatch and kept (per minibatch and kind, as received) for a replay over another transport.
"""
import numpy as np

ORDER = ("COUNTS", "KEYS", "CNT", "ROWS", "GRADS")


class ScriptedPeers:
    def __init__(self, rank, world, stride, push_cnt, is_train=True, peer_keys=None, peer_cnt=None, rows_of=None, peer_grads=None):
        """peer_keys {p: u64 [n_p]}: the keys peer p sends this rank (missing: none; every peer announces a minibatch);
        peer_cnt {p: f32 [n_p]}: their counts (with push_cnt); rows_of(p, keys) -> f32 [len(keys), stride]: peer p's answer to
        the keys this rank sent it; peer_grads {p: f32 [n_p, stride]}: the gradient rows peer p pushes for peer_keys[p]"""
        self.rank, self.world, self.stride = int(rank), int(world), int(stride)
        self.push_cnt, self.is_train = bool(push_cnt), bool(is_train)
        self.peers = [p for p in range(self.world) if p != self.rank]
        self.peer_keys = {p: np.ascontiguousarray((peer_keys or {}).get(p, np.zeros(0, np.uint64)), np.uint64) for p in self.peers}
        self.peer_cnt = {p: np.ascontiguousarray((peer_cnt or {}).get(p, np.zeros(0, np.float32)), np.float32) for p in self.peers}
        self.peer_grads = {p: np.ascontiguousarray((peer_grads or {}).get(p, np.zeros((0, self.stride), np.float32)), np.float32)
                           for p in self.peers}
        for p in self.peers:
            n = len(self.peer_keys[p])
            assert not self.push_cnt or len(self.peer_cnt[p]) == n
            assert not self.is_train or self.peer_grads[p].shape == (n, self.stride)
        self.rows_of = rows_of
        self.plan = [k for k in ORDER if (k != "CNT" or self.push_cnt) and (k != "GRADS" or self.is_train)]
        self.pos = 0
        self.sent = {}          # kind -> {peer: the bytes sent, as the kind's type}
        self.counts = None      # the COUNTS words this rank sent: int64 [world, 2]
        self.nsend = None       # keys this rank sends every peer (0 for itself)
        self.error = None

    # -- the function handed to capi.Comm.callback
    def exchange(self, send, send_bytes, recv, recv_bytes):
        try:
            self._exchange(send, send_bytes, recv, recv_bytes)
        except BaseException as e:
            self.error = e
            raise

    def finished(self):
        return self.pos == len(self.plan)

    def _exchange(self, send, sb, recv, rb):
        if self.error is not None:
            raise AssertionError("an exchange after a failed one")
        if self.pos >= len(self.plan):
            raise AssertionError("exchange number %d of a step that has %d" % (self.pos + 1, len(self.plan)))
        kind = self.plan[self.pos]
        W, me = self.world, self.rank
        if len(sb) != W or len(rb) != W:
            raise AssertionError("%s: %d / %d byte counts for %d ranks" % (kind, len(sb), len(rb), W))
        if kind == "COUNTS":
            if list(sb) != [16] * W or list(rb) != [16] * W:
                raise AssertionError("COUNTS: send %r recv %r, 16 B per rank expected" % (list(sb), list(rb)))
            c = np.array(send, copy=True).view(np.int64).reshape(W, 2)
            self.counts = c
            self.nsend = [0 if p == me else int(c[p, 0]) for p in range(W)]
            if min(self.nsend) < 0:
                raise AssertionError("COUNTS: a negative number of keys: %r" % (c[:, 0].tolist(),))
            out = np.zeros((W, 2), np.int64)
            out[me] = c[me]      # the rank's own slot comes back as it was sent
            for p in self.peers:
                out[p] = (len(self.peer_keys[p]), 1)
            recv[:] = out.view(np.uint8).reshape(-1)
            self.pos += 1
            return
        nrecv = [0 if p == me else len(self.peer_keys[p]) for p in range(W)]
        row_b = 4 * self.stride
        # (bytes per key this rank sends for its nsend keys or for the nrecv it received, dtype, and the same for the receive side)
        unit = {"KEYS": (8, self.nsend, nrecv, np.uint64), "CNT": (4, self.nsend, nrecv, np.float32),
                "ROWS": (row_b, nrecv, self.nsend, np.float32), "GRADS": (row_b, self.nsend, nrecv, np.float32)}[kind]
        nb, n_out, n_in, dt = unit
        want_sb, want_rb = [nb * n for n in n_out], [nb * n for n in n_in]
        if list(sb) != want_sb or list(rb) != want_rb:
            raise AssertionError("%s: send %r recv %r bytes, expected %r and %r" % (kind, list(sb), list(rb), want_sb, want_rb))
        got, o = {}, 0
        for p in range(W):
            part = np.array(send[o:o + sb[p]], copy=True).view(dt)
            o += sb[p]
            if p != me:
                got[p] = part.reshape(-1, self.stride) if nb == row_b else part
        self.sent[kind] = got
        parts = []
        for p in self.peers:
            if kind == "KEYS":
                a = self.peer_keys[p]
            elif kind == "CNT":
                a = self.peer_cnt[p]
            elif kind == "GRADS":
                a = self.peer_grads[p]
            else:
                keys = self.sent["KEYS"][p]
                a = np.zeros((0, self.stride), np.float32)
                if len(keys):
                    a = np.ascontiguousarray(self.rows_of(p, keys), np.float32)
                    if a.shape != (len(keys), self.stride):
                        raise AssertionError("rows_of(%d): shape %r for %d keys" % (p, a.shape, len(keys)))
            parts.append(np.ascontiguousarray(a).view(np.uint8).reshape(-1))
        out = np.concatenate(parts) if parts else np.zeros(0, np.uint8)
        if len(out) != len(recv):
            raise AssertionError("%s: %d bytes prepared, %d to receive" % (kind, len(out), len(recv)))
        recv[:] = out
        self.pos += 1


class StreamPeers:
    def __init__(self, rank, world, stride, push_cnt, stream, schedule="overlap"):
        """stream: one dict per minibatch — have (this rank has a minibatch: True), peers_have (True), is_train (True),
        peer_keys {p: u64 [n_p]}, peer_cnt {p: f32 [n_p]}, peer_grads {p: f32 [n_p, stride]}, rows_of(p, keys) -> the rows peer
        p answers with.  schedule: "overlap" (every entry after the first announced before the step in front of it) or
        "sync" (nothing announced)"""
        self.rank, self.world, self.stride = int(rank), int(world), int(stride)
        self.push_cnt = bool(push_cnt)
        self.peers = [p for p in range(self.world) if p != self.rank]
        self.stream = []
        for m in stream:
            e = dict(have=bool(m.get("have", True)), peers_have=bool(m.get("peers_have", True)), is_train=bool(m.get("is_train", True)),
                     rows_of=m.get("rows_of"))
            e["active"] = e["have"] or e["peers_have"]
            e["peer_keys"] = {p: np.ascontiguousarray((m.get("peer_keys") or {}).get(p, np.zeros(0, np.uint64)), np.uint64) for p in self.peers}
            e["peer_cnt"] = {p: np.ascontiguousarray((m.get("peer_cnt") or {}).get(p, np.zeros(0, np.float32)), np.float32) for p in self.peers}
            e["peer_grads"] = {p: np.ascontiguousarray((m.get("peer_grads") or {}).get(p, np.zeros((0, self.stride), np.float32)), np.float32)
                               for p in self.peers}
            for p in self.peers:
                n = len(e["peer_keys"][p])
                assert e["peers_have"] or n == 0, "a peer without a minibatch sends no keys"
                assert not self.push_cnt or len(e["peer_cnt"][p]) == n
                assert not (e["is_train"] and e["active"]) or e["peer_grads"][p].shape == (n, self.stride)
            self.stream.append(e)
        self.steps = self.make_steps([e["active"] for e in self.stream], [e["is_train"] for e in self.stream], self.push_cnt, schedule)
        self.plan = [x for one in self.steps for x in one]
        self.pos = 0
        self.sent = {}          # (minibatch, kind) -> {peer: what the rank sent, as the kind's type}
        self.supplied = {}      # (minibatch, kind) -> (the bytes received, the byte counts per rank)
        self.counts = {}        # minibatch -> the COUNTS words the rank sent: int64 [world, 2]
        self.nsend = {}
        self.error = None

    @staticmethod
    def make_steps(active, is_train, push_cnt, schedule="overlap"):
        """per call of dfh_shard_step, the exchanges it makes: [[(kind, minibatch)]]; nothing after a minibatch nobody has"""
        M = len(active)
        head = lambda m: [("KEYS", m)] + ([("CNT", m)] if push_cnt else [])
        steps = []
        for t in range(M):
            if t and not active[t - 1]:
                break
            if schedule == "sync":
                steps.append([("COUNTS", t)] + (head(t) + [("ROWS", t)] + ([("GRADS", t)] if is_train[t] else []) if active[t] else []))
                continue
            assert schedule == "overlap"
            one = [("COUNTS", 0)] + (head(0) + [("ROWS", 0)] if active[0] else []) if t == 0 else []
            if active[t]:
                ahead = t + 1 < M and active[t + 1]
                if t + 1 < M:
                    one.append(("COUNTS", t + 1))
                if ahead:
                    one += head(t + 1)
                if is_train[t]:
                    one.append(("GRADS", t))
                if ahead:
                    one.append(("ROWS", t + 1))
            steps.append(one)
        return steps

    @classmethod
    def make_plan(cls, active, is_train, push_cnt, schedule="overlap"):
        """[(kind, minibatch)] in the order the schedule makes its exchanges"""
        return [x for one in cls.make_steps(active, is_train, push_cnt, schedule) for x in one]

    # -- the function handed to capi.Comm.callback
    def exchange(self, send, send_bytes, recv, recv_bytes):
        try:
            self._exchange(send, send_bytes, recv, recv_bytes)
        except BaseException as e:
            self.error = e
            raise

    def finished(self):
        return self.pos == len(self.plan)

    def done_steps(self, n):
        """exactly the exchanges of the first n calls of dfh_shard_step have been made"""
        return self.pos == sum(len(one) for one in self.steps[:n])

    def _exchange(self, send, sb, recv, rb):
        if self.error is not None:
            raise AssertionError("an exchange after a failed one")
        if self.pos >= len(self.plan):
            raise AssertionError("exchange number %d of a stream that has %d" % (self.pos + 1, len(self.plan)))
        kind, m = self.plan[self.pos]
        what = "%s(%d)" % (kind, m)
        e = self.stream[m]
        W, me = self.world, self.rank
        if len(sb) != W or len(rb) != W:
            raise AssertionError("%s: %d / %d byte counts for %d ranks" % (what, len(sb), len(rb), W))
        if kind == "COUNTS":
            if list(sb) != [16] * W or list(rb) != [16] * W:
                raise AssertionError("%s: send %r recv %r, 16 B per rank expected" % (what, list(sb), list(rb)))
            c = np.array(send, copy=True).view(np.int64).reshape(W, 2)
            if c[:, 1].tolist() != [int(e["have"])] * W:
                raise AssertionError("%s: the rank says %r about having a minibatch, the stream %r" % (what, c[:, 1].tolist(), e["have"]))
            self.counts[m] = c
            self.nsend[m] = [0 if p == me else int(c[p, 0]) for p in range(W)]
            if min(self.nsend[m]) < 0 or (not e["have"] and c[:, 0].any()):
                raise AssertionError("%s: the numbers of keys %r" % (what, c[:, 0].tolist()))
            out = np.zeros((W, 2), np.int64)
            out[me] = c[me]      # the rank's own slot comes back as it was sent
            for p in self.peers:
                out[p] = (len(e["peer_keys"][p]), int(e["peers_have"]))
            recv[:] = out.view(np.uint8).reshape(-1)
            self.supplied[(m, kind)] = (np.array(recv, copy=True), list(rb))
            self.pos += 1
            return
        nsend = self.nsend[m]
        nrecv = [0 if p == me else len(e["peer_keys"][p]) for p in range(W)]
        row_b = 4 * self.stride
        nb, n_out, n_in, dt = {"KEYS": (8, nsend, nrecv, np.uint64), "CNT": (4, nsend, nrecv, np.float32),
                               "ROWS": (row_b, nrecv, nsend, np.float32), "GRADS": (row_b, nsend, nrecv, np.float32)}[kind]
        want_sb, want_rb = [nb * n for n in n_out], [nb * n for n in n_in]
        if list(sb) != want_sb or list(rb) != want_rb:
            raise AssertionError("%s: send %r recv %r bytes, expected %r and %r" % (what, list(sb), list(rb), want_sb, want_rb))
        got, o = {}, 0
        for p in range(W):
            part = np.array(send[o:o + sb[p]], copy=True).view(dt)
            o += sb[p]
            if p != me:
                got[p] = part.reshape(-1, self.stride) if nb == row_b else part
        self.sent[(m, kind)] = got
        parts = []
        for p in self.peers:
            if kind == "KEYS":
                a = e["peer_keys"][p]
            elif kind == "CNT":
                a = e["peer_cnt"][p]
            elif kind == "GRADS":
                a = e["peer_grads"][p]
            else:
                keys = self.sent[(m, "KEYS")][p]
                a = np.zeros((0, self.stride), np.float32)
                if len(keys):
                    a = np.ascontiguousarray(e["rows_of"](p, keys), np.float32)
                    if a.shape != (len(keys), self.stride):
                        raise AssertionError("%s: rows_of(%d) has shape %r for %d keys" % (what, p, a.shape, len(keys)))
            parts.append(np.ascontiguousarray(a).view(np.uint8).reshape(-1))
        out = np.concatenate(parts) if parts else np.zeros(0, np.uint8)
        if len(out) != len(recv):
            raise AssertionError("%s: %d bytes prepared, %d to receive" % (what, len(out), len(recv)))
        recv[:] = out
        self.supplied[(m, kind)] = (np.array(recv, copy=True), list(rb))
        self.pos += 1
