"""A numpy restatement of the reference's BCD learner (src/bcd/), the yardstick of learner = bcd: the feature-group
statistics and PartitionFeature (bcd_utils.h:65-131), the block counts of RunScheduler (bcd_learner.cc:62-69), the block
shuffle (std::random_shuffle on glibc's rand(), restated as RefRand), the gradient (logit_loss_delta.h:90-146: float
terms, fp64 sums), BCDUpdater::UpdateWeight (bcd_updater.h:138-162) in float and the float prediction update
(TransTimes, spmv.h:139-167)."""
import math

import numpy as np

f32 = np.float32
U64 = (1 << 64) - 1


def reverse_bytes(x):
    """include/difacto/base.h: nibble reversal of a 64-bit id"""
    x = ((x << 32) | (x >> 32)) & U64
    x = ((x & 0x0000FFFF0000FFFF) << 16) | ((x & 0xFFFF0000FFFF0000) >> 16)
    x = ((x & 0x00FF00FF00FF00FF) << 8) | ((x & 0xFF00FF00FF00FF00) >> 8)
    x = ((x & 0x0F0F0F0F0F0F0F0F) << 4) | ((x & 0xF0F0F0F0F0F0F0F0) >> 4)
    return x & U64


def reverse_bytes_np(x):
    """reverse_bytes on a uint64 array"""
    x = np.asarray(x, np.uint64)
    s = lambda v: np.uint64(v)
    x = (x << s(32)) | (x >> s(32))
    x = ((x & s(0x0000FFFF0000FFFF)) << s(16)) | ((x & s(0xFFFF0000FFFF0000)) >> s(16))
    x = ((x & s(0x00FF00FF00FF00FF)) << s(8)) | ((x & s(0xFF00FF00FF00FF00)) >> s(8))
    return ((x & s(0x0F0F0F0F0F0F0F0F)) << s(4)) | ((x & s(0xF0F0F0F0F0F0F0F0)) >> s(4))


class RefRand:
    """glibc's rand() in its default state (random_r TYPE_3), as difacto_amd/host/batch_reader.h restates it"""

    def __init__(self, seed=1):
        r = [seed or 1]
        for i in range(1, 31):
            x = (16807 * r[i - 1]) % 2147483647
            r.append(x + 2147483647 if x < 0 else x)
        self.st = [v & 0xFFFFFFFF for v in r]
        self.f, self.b = 3, 0
        for _ in range(310):
            self.next()

    def next(self):
        self.st[self.f] = (self.st[self.f] + self.st[self.b]) & 0xFFFFFFFF
        out = self.st[self.f] >> 1
        self.f = 0 if self.f == 30 else self.f + 1
        self.b = 0 if self.b == 30 else self.b + 1
        return out

    def shuffle(self, v):
        """libstdc++'s std::random_shuffle"""
        for i in range(1, len(v)):
            j = self.next() % (i + 1)
            if i != j:
                v[i], v[j] = v[j], v[i]


def read_libsvm(path):
    """-> offset (uint64), raw ids (uint64), values (float32), labels (float32)"""
    off, idx, val, lab = [0], [], [], []
    for line in open(path):
        t = line.split()
        if not t:
            continue
        lab.append(float(t[0]))
        for kv in t[1:]:
            i, x = kv.split(":")
            idx.append(int(i))
            val.append(float(x))
        off.append(len(idx))
    return (np.array(off, np.uint64), np.array(idx, np.uint64), np.array(val, np.float32), np.array(lab, np.float32))


def fea_group_stats(chunks, nbits):
    """FeaGroupStats over the training chunks [(offset, ids)]: every 10th row of each chunk counted"""
    v = np.zeros((1 << nbits) + 2, np.float32)
    for off, ids in chunks:
        n = len(off) - 1
        rows = range(0, n, 10)
        for i in rows:
            for j in range(int(off[i]), int(off[i + 1])):
                v[int(ids[j]) % (1 << nbits)] += f32(1)
        v[1 << nbits] += f32(len(rows))
        v[(1 << nbits) + 1] += f32(n)
    return v


def block_counts(stats, block_ratio):
    """RunScheduler's (group, nblk) list: ceil(count / rows counted * block_ratio) in float"""
    nf = len(stats) - 2
    out = []
    for i in range(nf):
        nblk = int(math.ceil(float(f32(f32(stats[i]) / f32(stats[nf])) * f32(block_ratio))))
        if nblk > 0:
            out.append((i, nblk))
    return out


def partition_feature(nbits, feagrps):
    """PartitionFeature with Range::Segment's double arithmetic and the ++before.end fix-up"""
    blks = []
    for gid, n in feagrps:
        b = reverse_bytes(((0 << nbits) | gid) & U64)
        e = reverse_bytes(((U64 << nbits) | gid) & U64)
        itv = float(e - b) / float(n)
        for i in range(n):
            lo = int(float(b) + itv * i)
            hi = e if i == n - 1 else int(float(b) + itv * (i + 1))
            assert hi > lo
            blks.append([lo, hi])
    blks.sort(key=lambda r: r[0])
    for i in range(1, len(blks)):
        if blks[i - 1][1] < blks[i][0]:
            blks[i - 1][1] += 1
        assert blks[i - 1][1] <= blks[i][0]
    return [tuple(r) for r in blks]


def update_weight(g, h, w, delta, l1, lr):
    """BCDUpdater::UpdateWeight + bcd::Delta::Update, elementwise in float32 as written -> (w, delta, dw)"""
    g, h, w, delta = (np.asarray(a, np.float32) for a in (g, h, w, delta))
    g_pos, g_neg = g + f32(l1), g - f32(l1)
    u = ((h / f32(lr)).astype(np.float64) + 1e-10).astype(np.float32)
    uw = u * w
    with np.errstate(divide="ignore", invalid="ignore"):
        d = np.where(g_pos <= uw, -g_pos / u, np.where(g_neg >= uw, -g_neg / u, -w)).astype(np.float32)
    d = np.where(d < -delta, -delta, d)
    d = np.where(delta < d, delta, d).astype(np.float32)
    nd = (np.abs(d).astype(np.float64) * 2.0 + .1).astype(np.float32)
    return (w + d).astype(np.float32), np.where(nd < f32(5), nd, f32(5)).astype(np.float32), d


class Chunk:
    """a chunk localized as Localizer(-1) does: keys = ReverseBytes(id) ascending; entries (row, key position, value)"""

    def __init__(self, off, ids, val, lab):
        self.n = len(off) - 1
        self.lab = np.asarray(lab, np.float32)
        rk = reverse_bytes_np(ids)
        self.keys, inv = np.unique(rk, return_inverse=True)
        rows = np.repeat(np.arange(self.n), np.diff(off.astype(np.int64)))
        self.cnt = np.bincount(inv, minlength=len(self.keys)).astype(np.float32)
        o = np.lexsort((np.arange(len(inv)), inv))    # key order, ties in position order (= row order)
        self.col, self.row, self.val = inv[o], rows[o], (None if val is None else np.asarray(val, np.float32)[o])
        self.pred = np.zeros(self.n, np.float32)


class BCD:
    """the learner on a list of training chunks (and validation chunks); stream: the RefRand the shuffles draw from"""

    def __init__(self, train, val=(), l1=1.0, lr=0.9, block_ratio=4.0, tail_feature_filter=4, nbits=0, stats=None):
        self.tr, self.va, self.l1, self.lr = [Chunk(*c) for c in train], [Chunk(*c) for c in val], l1, lr
        st = fea_group_stats([(c[0], c[1]) for c in train], nbits) if stats is None else stats
        self.ranges = partition_feature(nbits, block_counts(st, block_ratio))
        keys = np.concatenate([c.keys for c in self.tr])
        cnts = np.concatenate([c.cnt for c in self.tr])
        uk, inv = np.unique(keys, return_inverse=True)
        tot = np.zeros(len(uk), np.float32)
        np.add.at(tot, inv, cnts)
        self.keys = uk[tot > f32(tail_feature_filter)]
        K = len(self.keys)
        self.w, self.delta, self.dw = np.zeros(K, np.float32), np.ones(K, np.float32), np.zeros(K, np.float32)
        self.pos = [(int(np.searchsorted(self.keys, np.uint64(b))), int(np.searchsorted(self.keys, np.uint64(e))))
                    for b, e in self.ranges]
        for c in self.tr + list(self.va):
            gp = np.searchsorted(self.keys, c.keys)
            hit = (gp < K) & (self.keys[np.minimum(gp, K - 1)] == c.keys)
            c.gk = np.where(hit, gp, -1)[c.col]   # model position of every entry, -1 filtered

    def grad(self, blk, mag=False):
        """the block's g, h summed in fp64 over the training chunks (mag: and the sums of |terms|)"""
        pb, pe = self.pos[blk]
        g, h = np.zeros(pe - pb), np.zeros(pe - pb)
        ga, ha = np.zeros(pe - pb), np.zeros(pe - pb)
        for c in self.tr:
            y = np.where(c.lab > 0, f32(1), f32(-1)).astype(np.float32)
            p = (-y / (f32(1) + np.exp(y * c.pred))).astype(np.float32)
            t = (-p * (y + p)).astype(np.float32)
            m = (c.gk >= pb) & (c.gk < pe)
            r = c.row[m]
            if c.val is None:
                cg, ch = p[r], t[r]
            else:
                x = c.val[m]
                cg, ch = p[r] * x, t[r] * (x * x)
            np.add.at(g, c.gk[m] - pb, cg.astype(np.float64))
            np.add.at(h, c.gk[m] - pb, ch.astype(np.float64))
            np.add.at(ga, c.gk[m] - pb, np.abs(cg.astype(np.float64)))
            np.add.at(ha, c.gk[m] - pb, np.abs(ch.astype(np.float64)))
        return (g, h, ga, ha) if mag else (g, h)

    def update_pred(self, blk):
        """pred_r += dw_j x_rj in float, keys ascending, dw == 0 skipped"""
        pb, pe = self.pos[blk]
        for c in self.tr + list(self.va):
            m = (c.gk >= pb) & (c.gk < pe)
            gk, r = c.gk[m], c.row[m]
            x = None if c.val is None else c.val[m]
            # entries are in key order; one key's rows at a time keeps every row's adds in ascending key order
            starts = np.flatnonzero(np.r_[True, gk[1:] != gk[:-1]]) if len(gk) else []
            ends = list(starts[1:]) + [len(gk)]
            for s, e in zip(starts, ends):
                d = self.dw[gk[s]]
                if d == 0:
                    continue
                add = np.full(e - s, d, np.float32) if x is None else (d * x[s:e]).astype(np.float32)
                np.add.at(c.pred, r[s:e], add)

    def step(self, blk):
        g, h = self.grad(blk)
        pb, pe = self.pos[blk]
        self.w[pb:pe], self.delta[pb:pe], self.dw[pb:pe] = update_weight(
            g.astype(np.float32), h.astype(np.float32), self.w[pb:pe], self.delta[pb:pe], self.l1, self.lr)
        self.update_pred(blk)
        return g, h

    def progress(self):
        """{count, LogitObjv, Accuracy(.5)} summed in float per chunk (AUC left out)"""
        cnt, objv, acc = f32(0), f32(0), f32(0)
        for c in self.tr + list(self.va):
            y = np.where(c.lab > 0, 1.0, -1.0)
            o = np.log(1.0 + np.exp(-y * c.pred.astype(np.float64))).sum()
            ok = float((((c.lab > 0) & (c.pred > f32(.5))) | ((c.lab <= 0) & (c.pred <= f32(.5)))).sum())
            cnt += f32(c.n)
            objv += f32(o)
            acc += f32(ok if ok > 0.5 * c.n else c.n - ok)
        return cnt, objv, acc

    def run(self, epochs, stream):
        """-> per-epoch objective; the block order of each epoch shuffles the previous one, as the reference's does"""
        order = list(range(len(self.ranges)))
        out = []
        for _ in range(epochs):
            stream.shuffle(order)
            for b in order:
                self.step(b)
            out.append(float(self.progress()[1]))
        return out


def split_rows(off, ids, val, lab, rows):
    """training chunks of the given row counts"""
    out, r0 = [], 0
    for n in rows:
        a, b = int(off[r0]), int(off[r0 + n])
        out.append((off[r0:r0 + n + 1] - off[r0], ids[a:b], None if val is None else val[a:b], lab[r0:r0 + n]))
        r0 += n
    assert r0 == len(off) - 1
    return out
