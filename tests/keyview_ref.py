"""The second product of the device Localizer, restated in numpy, and minibatches designed to reach its edges.

The Localizer's first product (feaids, feacnt, the compact index) is what Localizer::Compact returns.  Its second product is what
the backward and the update pass walk: the key-ordered view (col_ptr, s_row, s_val), the three length-class lists of segments
(few / mid / hot, entries {u, beg, end, 0} in per-bucket slot ranges) and the split list a training step adds
({u, beg_p, end_p, p << 16 | nparts}).  `reference` computes all of it from the CSR offsets, the compact index and the values;
`check_key_view` compares what Batch.get_key_view() read back with it, exactly.

Minibatches are DESIGNED in key order: `lens[u]` is the number of occurrences of the key of rank u, and the raw id of that key
is reverse_bytes((u + 1) << SHIFT) — ReverseBytes is an involution, so the Localizer's key of that id is (u + 1) << SHIFT and
the sorted order is the designed rank order.  Where the occurrences sit in the rows is drawn at random; the key-ordered view
does not depend on it beyond the order inside a key.
"""
import numpy as np

SHIFT = 8                 # designed keys are (rank + 1) << SHIFT: the keys of a stale primer (below) fit in between
SMALL_AVG = 192           # dfh_localize_api.hip: pairs per bucket a first call with up to 65 536 pairs aims for
LDS_CAP = 1024            # dfh_localize.hip: LOC_LDS_CAP


def reverse_bytes(ids):
    """ReverseBytes of the reference: the 16 four-bit digits of the id in reverse order"""
    x = np.ascontiguousarray(ids, np.uint64).byteswap()
    lo = np.uint64(0x0F0F0F0F0F0F0F0F)
    return ((x & lo) << np.uint64(4)) | ((x >> np.uint64(4)) & lo)


def cold_buckets(N):
    """buckets a first call takes for N <= 65 536 pairs (localize_impl)"""
    assert 1 <= N <= 65536
    return max(1, (N + SMALL_AVG - 1) // SMALL_AVG)


# ------------------------------------------------------------------------------------------------ the reference
def reference(offset, cidx, value, bounds):
    """offset [nrows + 1], cidx [nnz] = the compact index (rank of every pair's key), value [nnz] or None;
    bounds = dict(BWD_SMALL, BWD_MID, HOT_SPLIT, HOT_SPLIT_MIN)"""
    offset = np.asarray(offset).astype(np.int64)
    cidx = np.asarray(cidx).astype(np.int64)
    nnz = int(offset[-1])
    assert len(cidx) == nnz
    U = int(cidx.max()) + 1 if nnz else 0
    cnt = np.bincount(cidx, minlength=U).astype(np.int64)
    col_ptr = np.zeros(U + 1, np.int64)
    col_ptr[1:] = np.cumsum(cnt)
    order = np.argsort(cidx, kind="stable")      # ties in position order, which is row order
    rows = np.repeat(np.arange(len(offset) - 1, dtype=np.int64), np.diff(offset))
    S, M, HS, HSM = (int(bounds[k]) for k in ("BWD_SMALL", "BWD_MID", "HOT_SPLIT", "HOT_SPLIT_MIN"))
    u = np.arange(U, dtype=np.int64)
    ent = np.stack([u, col_ptr[:-1], col_ptr[1:], np.zeros(U, np.int64)], 1).astype(np.uint32) if U else np.zeros((0, 4), np.uint32)
    split = []
    for k in u[cnt > HSM]:
        beg, end = int(col_ptr[k]), int(col_ptr[k + 1])
        nparts = (end - beg + HS - 1) // HS
        split += [(int(k), beg + p * HS, min(beg + (p + 1) * HS, end), p << 16 | nparts) for p in range(nparts)]
    return dict(U=U, nnz=nnz, col_ptr=col_ptr.astype(np.uint32), s_row=rows[order].astype(np.uint32),
                s_val=None if value is None else np.ascontiguousarray(value, np.float32)[order],
                few=ent[(cnt >= 2) & (cnt <= S)], mid=ent[(cnt > S) & (cnt <= M)], hot=ent[cnt > M],
                split=np.array(split, np.uint32).reshape(-1, 4), bounds=dict(bounds))


def brute_force(offset, cidx, value, bounds):
    """the same by plain loops: for tiny inputs"""
    nrows, nnz = len(offset) - 1, int(offset[-1])
    U = max([int(c) for c in cidx], default=-1) + 1
    occ = [[] for _ in range(U)]
    for r in range(nrows):
        for j in range(int(offset[r]), int(offset[r + 1])):
            occ[int(cidx[j])].append((r, j))
    col_ptr, s_row, s_val, lists, split = [0], [], [], dict(few=[], mid=[], hot=[]), []
    for k in range(U):
        beg = col_ptr[-1]
        for r, j in occ[k]:
            s_row.append(r)
            if value is not None:
                s_val.append(value[j])
        end = beg + len(occ[k])
        col_ptr.append(end)
        n = end - beg
        if n > bounds["BWD_MID"]:
            lists["hot"].append((k, beg, end, 0))
        elif n > bounds["BWD_SMALL"]:
            lists["mid"].append((k, beg, end, 0))
        elif n > 1:
            lists["few"].append((k, beg, end, 0))
        if n > bounds["HOT_SPLIT_MIN"]:
            h = bounds["HOT_SPLIT"]
            nparts = -(-n // h)
            for p in range(nparts):
                split.append((k, beg + p * h, min(beg + (p + 1) * h, end), p << 16 | nparts))
    out = dict(U=U, nnz=nnz, col_ptr=np.array(col_ptr, np.uint32), s_row=np.array(s_row, np.uint32).reshape(-1),
               s_val=None if value is None else np.array(s_val, np.float32).reshape(-1),
               split=np.array(split, np.uint32).reshape(-1, 4), bounds=dict(bounds))
    for k, v in lists.items():
        out[k] = np.array(v, np.uint32).reshape(-1, 4)
    return out


def _rows_sorted(a):
    a = np.asarray(a, np.uint32).reshape(-1, 4)
    return a[np.lexsort((a[:, 3], a[:, 2], a[:, 1], a[:, 0]))]


def same_reference(a, b):
    """two results of reference / brute_force agree (the lists as sets)"""
    assert a["U"] == b["U"] and a["nnz"] == b["nnz"]
    assert np.array_equal(a["col_ptr"], b["col_ptr"]) and np.array_equal(a["s_row"], b["s_row"])
    assert (a["s_val"] is None) == (b["s_val"] is None)
    if a["s_val"] is not None:
        assert np.array_equal(a["s_val"].view(np.uint32), b["s_val"].view(np.uint32))
    for k in ("few", "mid", "hot"):
        assert np.array_equal(_rows_sorted(a[k]), _rows_sorted(b[k])), k
    assert np.array_equal(a["split"], b["split"])


# ------------------------------------------------------------------------------------------------ the checker
def check_key_view(got, ref, split="skip", split_entries=None):
    """got: Batch.get_key_view(); ref: reference(...) with the bounds taken from `got`.  split: "listed" after a training
    step (the list holds exactly the parts of the minibatch's very hot keys, split_entries = Batch.split_entries()), "empty"
    for a fresh batch object that was never stepped, "skip" otherwise"""
    for k in ("BWD_SMALL", "BWD_MID", "HOT_SPLIT", "HOT_SPLIT_MIN"):
        assert got[k] == ref["bounds"][k], "reference computed with another %s than the library's" % k
    S, M = got["BWD_SMALL"], got["BWD_MID"]
    N = ref["nnz"]
    assert got["U"] == ref["U"] and got["nnz"] == N
    assert np.array_equal(got["col_ptr"], ref["col_ptr"]), "col_ptr"
    assert np.array_equal(got["s_row"], ref["s_row"]), "s_row (the order inside a key is row order)"
    assert (got["s_val"] is None) == (ref["s_val"] is None), "s_val present"
    if ref["s_val"] is not None:
        assert np.array_equal(got["s_val"].view(np.uint32), ref["s_val"].view(np.uint32)), "s_val, as bits"
    nb, bstart = got["seg_nb"], got["bstart"]
    if got["P"]:
        assert nb == got["P"] and len(bstart) == nb + 1
        bs = bstart.astype(np.int64)
        assert bs[0] == 0 and bs[-1] == N and np.all(np.diff(bs) >= 0), "bstart"
        n_b = np.diff(bs)
    bound = dict(few=lambda n: n // 2 + 2, mid=lambda n: n // (S + 1) + 2, hot=lambda n: n // (M + 1) + 2)
    for name in ("few", "mid", "hot"):
        lst = got[name]
        desc = lst["desc"].astype(np.int64)
        assert desc.shape == (nb, 2), name
        for q, e in enumerate(lst["buckets"]):
            assert e is not None, "%s: bucket %d's range [%d, %d) leaves the array of %d" % (
                name, q, desc[q, 1], desc[q, 1] + desc[q, 0], lst["cap"])
        # the slot ranges of different buckets do not meet
        live = desc[desc[:, 0] > 0]
        live = live[np.argsort(live[:, 1], kind="stable")]
        assert np.all(live[:-1, 1] + live[:-1, 0] <= live[1:, 1]), "%s: slot ranges of two buckets overlap" % name
        ent = np.concatenate([e for e in lst["buckets"]] + [np.zeros((0, 4), np.uint32)])
        want = _rows_sorted(ref[name])
        assert np.all(ent[:, 3] == 0), "%s: fourth word" % name
        assert np.all(ent[:, 2].astype(np.int64) - ent[:, 1] > 1), "%s: an entry of length 1 (or less)" % name
        assert len(np.unique(ent[:, 0])) == len(ent), "%s: a key listed twice" % name
        have = _rows_sorted(ent)
        assert have.shape == want.shape and np.array_equal(have, want), "%s: got %d entries, want %d; first got %s, first want %s" % (
            name, len(have), len(want), have[:3].tolist(), want[:3].tolist())
        if got["P"]:
            for q in range(nb):
                if n_b[q] == 0:
                    assert tuple(desc[q]) == (0, 0), "%s: empty sort bucket %d has descriptor %s" % (name, q, desc[q])
                assert desc[q, 0] <= bound[name](int(n_b[q])), "%s: bucket %d of %d pairs lists %d" % (name, q, n_b[q], desc[q, 0])
                e = lst["buckets"][q].astype(np.int64)
                if len(e):
                    at = np.where(e[:, 2] == N, N - 1, e[:, 2])   # the position whose thread closed the segment
                    home = np.searchsorted(bs, at, side="right") - 1
                    assert np.all(home == q), "%s: bucket %d lists a segment that ends in bucket %s" % (name, q, home[home != q][:1])
    if split == "skip":
        return
    want = ref["split"] if split == "listed" else np.zeros((0, 4), np.uint32)
    have = got["split"]
    assert got["split_n"] == len(want) and got["split_n"] <= got["split_cap"], "split list: %d entries, want %d" % (got["split_n"], len(want))
    if split_entries is not None:
        assert split_entries == got["split_n"], "dfh_batch_split_entries reads another count"
    assert np.array_equal(_rows_sorted(have), _rows_sorted(want)), "split list: the set of parts"
    i = 0
    while i < len(have):   # the parts of one key are consecutive and in order of p
        nparts = int(have[i, 3]) & 0xFFFF
        blk = have[i:i + nparts]
        assert len(blk) == nparts and np.all(blk[:, 0] == have[i, 0]), "split list: parts of key %d not consecutive" % have[i, 0]
        assert np.array_equal(blk[:, 3] >> 16, np.arange(nparts)), "split list: parts of key %d out of order" % have[i, 0]
        i += nparts


# ------------------------------------------------------------------------------------------------ designed minibatches
def batch_from_lens(lens, seed, nrows=None, binary=False, one_row=False, special_values=False):
    """the minibatch whose key of rank u occurs lens[u] times: dict(offset, index, value, label, cidx = the compact index it
    must localize to, lens)"""
    rng = np.random.default_rng(seed)
    lens = np.asarray(lens, np.int64)
    assert np.all(lens >= 1)
    N = int(lens.sum())
    ranks = np.repeat(np.arange(len(lens), dtype=np.int64), lens)
    cidx = ranks[rng.permutation(N)]
    if one_row:
        off = np.array([0, N], np.uint64)
    else:
        nrows = nrows or max(2, N // 5)
        cuts = np.sort(rng.integers(0, N + 1, size=nrows - 1))
        cuts[: max(1, nrows // 50)] = 0                      # empty first rows
        cuts[nrows - 1 - max(1, nrows // 50):] = N           # empty last rows
        off = np.concatenate([[0], np.sort(cuts), [N]]).astype(np.uint64)
    val = None
    if not binary:
        val = rng.normal(size=N).astype(np.float32)
        if special_values:
            sp = np.array([0x80000000, 0x7F800000, 0xFF800000, 0x7FC01234, 0xFFA00001, 0x00000001, 0x807FFFFF, 0x00000000],
                          np.uint32).view(np.float32)        # -0, +-inf, two NaNs with payloads, two denormals, +0
            at = rng.permutation(N)[: min(N, 4 * len(sp))]
            val[at] = np.resize(sp, len(at))
    ids = reverse_bytes((cidx.astype(np.uint64) + np.uint64(1)) << np.uint64(SHIFT))
    lab = np.where(rng.random(len(off) - 1) < 0.4, 1.0, -1.0).astype(np.float32)
    return dict(offset=off, index=ids, value=val, label=lab, cidx=cidx.astype(np.uint32), lens=lens)


class Layout:
    """run lengths in key order, built position by position"""
    FILL = (1, 1, 2, 1, 3, 1, 1, 4, 1, 2)

    def __init__(self):
        self.lens, self.at, self.marks, self._f = [], 0, {}, 0

    def run(self, n, mark=None):
        if mark:
            self.marks[mark] = (self.at, self.at + n)
        self.lens.append(n)
        self.at += n
        return self

    def fill_to(self, pos):
        """short runs (1 .. 4) up to position pos"""
        assert pos >= self.at
        while self.at < pos:
            n = min(self.FILL[self._f % len(self.FILL)], pos - self.at)
            self._f += 1
            self.run(n)
        return self


def class_edge_lens(bounds, first, last, lone_tail=False):
    """segments of the six lengths at the class edges in mixed order, every one of them at least twice inside; `first` /
    `last` (0 .. 5) choose which of the six is the first / the last key.  lone_tail: a lone pair at the very end, after a
    hot key"""
    S, M = bounds["BWD_SMALL"], bounds["BWD_MID"]
    six = [1, 2, S, S + 1, M, M + 1]
    mid = [six[i] for i in (3, 0, 5, 1, 4, 2, 2, 5, 0, 3, 1, 4, 0, 0, 5, 5, 1)]
    lens = [six[first]] + mid + [six[last]]
    if lone_tail:
        lens += [M + 1, 1]
    return lens


def stored_bstart(s_row, N, P):
    """bucket starts when a minibatch is localized a second time.  The splitters are then its own exact quantiles, splitter
    m - 1 = the pair at sorted position m * N // P, and bucket m holds what is not below it.  The count pass compares a pair
    by (key, position << tb) WITHOUT the row bits a splitter's tag carries in its low tb bits (dfh_localize.hip: "the pair
    that IS a splitter ... may fall on either side"), so the splitter pair itself stays in bucket m - 1 unless its row is a
    multiple of 2^tb: the cut is one beyond the quantile for every pair outside row 0 (tb = 16 up to 65 536 pairs)"""
    tb = 16 if N <= 1 else min(16, 32 - int(N - 1).bit_length())
    at = [m * N // P for m in range(1, P)]
    return np.array([0] + [i + (1 if int(s_row[i]) % (1 << tb) else 0) for i in at] + [N])


def stitch_layout(bounds, ending):
    """N = 16 * 192 pairs whose sorted order meets the cuts of 16 stored-splitter buckets in every way.  Row 0 of a designed
    minibatch is empty, so the cuts are at 192 m + 1 (stored_bstart).  ending "inside_run": the minibatch ends inside a run
    that began two buckets earlier; "single": it ends on a single"""
    B, S, M = SMALL_AVG, bounds["BWD_SMALL"], bounds["BWD_MID"]
    assert S + 1 < 60 and 40 < M + 1 < 150
    cut = lambda m: m * B + 1
    L = Layout()
    L.fill_to(cut(1) - 5).run(5, "ends_on_cut")
    L.run(4, "begins_on_cut").fill_to(cut(2) - 1)
    L.run(2, "pair_1_1").fill_to(cut(3) - S)
    L.run(S + 1, "mid_S_1").fill_to(cut(4) - 1)                  # BWD_SMALL | 1
    L.run(S + 1, "mid_1_S").fill_to(cut(5) - 30)                 # 1 | BWD_SMALL
    L.run(M + 1, "hot_straddles").fill_to(cut(6) + 100)
    L.run(cut(10) + 50 - (cut(6) + 100), "three_whole_buckets")  # buckets 7, 8, 9 whole
    L.fill_to(cut(11)).run(2 * B, "two_whole_buckets")
    L.fill_to(cut(13) + 104)
    if ending == "inside_run":
        L.run(16 * B - L.at, "open_at_the_end")                  # begins in bucket 13, the last bucket is 15
    else:
        L.run(16 * B - 1 - L.at, "before_the_single").run(1, "last_single")
    assert L.at == 16 * B
    L.cuts = [0] + [cut(m) for m in range(1, 16)] + [16 * B]
    return L


def chunk_carry_layout():
    """N = 16 * 192 pairs and the bucket sizes a stale primer must cut them into: empty buckets, one of 800 pairs and one of
    1 100 (beyond the LDS capacity), with runs across the 256-element chunks of emit inside them"""
    sizes = [0, 0, 800, 0, 1100, 0, 0, 0] + [147, 146, 147, 146, 147, 146, 147, 146]
    assert sum(sizes) == 16 * SMALL_AVG and len(sizes) == 16
    L = Layout()
    L.fill_to(255).run(2, "pair_255_1").fill_to(508).run(9, "nine_over_512").fill_to(760).run(12, "twelve_over_768").fill_to(800)
    b1 = 800
    L.fill_to(b1 + 250).run(300, "run_300_over_two_chunks").fill_to(b1 + 767).run(2, "pair_767_1")
    L.fill_to(b1 + 1020).run(9, "nine_over_1024").fill_to(b1 + 1100)
    for cut in np.cumsum(sizes)[5:]:                 # a run ends at every cut
        L.fill_to(int(cut))
    return L, sizes


def snap_cuts(lens, cuts):
    """every cut moved up to the next run head (or to N): a stale primer can only cut between two keys"""
    heads = np.concatenate([[0], np.cumsum(lens)])
    return [int(heads[np.searchsorted(heads, c, side="left")]) for c in cuts]


def generic_stale_sizes(lens):
    """bucket sizes for a minibatch of any design: an empty first bucket, one that takes 45 % of the pairs or 1 100 of them,
    an empty one, the rest in equal shares"""
    N = int(np.sum(lens))
    P = cold_buckets(N)
    if P < 4:
        return [0] * (P - 1) + [N]
    big = min(N, max(1100 if N >= 2400 else 0, (45 * N) // 100))
    rest = P - 3
    cuts = snap_cuts(lens, [0, 0, big, big] + [big + ((N - big) * (i + 1)) // rest for i in range(rest)])
    cuts[-1] = N
    return [int(n) for n in np.diff(cuts)]


def stale_primer(lens, sizes, seed):
    """the minibatch after which the exact-quantile splitters cut the design `lens` into buckets of `sizes` pairs: as many
    pairs as the design has (the same bucket count), its keys one below the design's key at every cut"""
    rng = np.random.default_rng(seed)
    N, P = int(np.sum(lens)), len(sizes)
    assert sum(sizes) == N and P == cold_buckets(N)
    rank_at = np.repeat(np.arange(len(lens), dtype=np.int64), lens)      # rank of the pair at every sorted position
    cuts = np.cumsum(sizes)[:-1]
    for c in cuts:
        assert c == 0 or c == N or rank_at[c] != rank_at[c - 1], "a stale primer cannot cut inside a run (%d)" % c
    # splitter m - 1 is the pair at sorted position m * N // P of the primer
    skey = [((int(rank_at[c]) if c < N else len(lens)) + 1 << SHIFT) - 1 for c in cuts]
    m_of = np.zeros(N, np.int64)
    for m in range(1, P):
        m_of[m * N // P:] = m
    keys = np.array(skey, np.uint64)[np.maximum(1, m_of) - 1] if P > 1 else np.ones(N, np.uint64)
    ids = reverse_bytes(keys[rng.permutation(N)])
    nrows = max(2, N // 7)
    off = np.concatenate([[0], np.sort(rng.integers(0, N + 1, size=nrows - 1)), [N]]).astype(np.uint64)
    return dict(offset=off, index=ids, value=rng.normal(size=N).astype(np.float32), label=np.ones(nrows, np.float32))


def buckets_of(keys_sorted, primer_keys_sorted, P):
    """bucket starts the exact P-quantiles of a primer give a minibatch none of whose keys is a key of the primer"""
    N = len(primer_keys_sorted)
    spl = np.array([primer_keys_sorted[m * N // P] for m in range(1, P)], np.uint64)
    b = np.searchsorted(spl, keys_sorted, side="left")     # splitters below the key
    return np.concatenate([[0], np.cumsum(np.bincount(b, minlength=P))])
