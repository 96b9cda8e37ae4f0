"""Designed keys for the open-addressing key index (dfh_kernels.hip find_or_insert / find_or_insert_block / find_only /
k_rehash).  No GPU, no native library: plain Python integers and numpy.

The index hashes a key with splitmix64 (dfh_internal.h) and masks the hash with H - 1.  splitmix64 is a bijection of the
64-bit integers, so a test can CHOOSE a hash and compute the key that has it: unsplitmix64.  keys_for_homes builds keys whose
home slot is given at every table size up to 2^bits slots; the shapes below name the probe chains the device tests need
(a chain that wraps past slot H - 1, clusters that merge, one chain for the whole table).  IndexModel is a plain model of
linear probing with wrap, used only to PROVE on the CPU that a shape has the chain it claims — the device tests never compare
slot positions: the API does not show them, and which key gets which slot of a chain is a race.

A change of the hash function must revisit this file: the keys are built through the exact inverse of splitmix64."""
import numpy as np

M64 = (1 << 64) - 1
EMPTY_KEY = M64   # kEmptyKey: reserved, never a feature id

_INC = 0x9E3779B97F4A7C15
_M1 = 0xBF58476D1CE4E5B9
_M2 = 0x94D049BB133111EB
_M1_INV = pow(_M1, -1, 1 << 64)
_M2_INV = pow(_M2, -1, 1 << 64)


def splitmix64(x):
    """dfh_internal.h splitmix64 on one Python integer"""
    z = (x + _INC) & M64
    z = ((z ^ (z >> 30)) * _M1) & M64
    z = ((z ^ (z >> 27)) * _M2) & M64
    return z ^ (z >> 31)


def _unxorshift(y, s):
    """x with x ^ (x >> s) == y: the top s bits of x are y's, every further block of s bits follows from the one above it"""
    x = y
    for _ in range(64 // s + 1):
        x = y ^ (x >> s)
    return x


def unsplitmix64(h):
    """the key whose splitmix64 is h (exact inverse: undo the xor-shifts 31, 27, 30, multiply by the modular inverses of
    the two multipliers, subtract the increment)"""
    z = _unxorshift(h & M64, 31)
    z = (z * _M2_INV) & M64
    z = _unxorshift(z, 27)
    z = (z * _M1_INV) & M64
    z = _unxorshift(z, 30)
    return (z - _INC) & M64


def keys_for_homes(homes, bits=20, start=0):
    """one key per entry of homes: key j = unsplitmix64((start + j + 1) << bits | home_j).  The keys are distinct (their
    hashes differ above bit `bits`), key j's home slot is home_j at every table size up to 2^bits slots, and the reserved
    key ~0 is not among them.  `start` shifts the tags: a second list built with start >= len(first) shares no key with it."""
    homes = [int(h) for h in homes]
    assert all(0 <= h < (1 << bits) for h in homes)
    assert (start + len(homes) + 1) << bits <= M64
    keys = [unsplitmix64(((start + j + 1) << bits) | h) for j, h in enumerate(homes)]
    assert EMPTY_KEY not in keys
    assert len(set(keys)) == len(keys)
    return np.array(keys, dtype=np.uint64)


def home_of(key, H):
    return splitmix64(int(key)) & (H - 1)


class IndexModel:
    """linear probing with wrap in a table of H slots (H a power of two), one key per slot: the host model of the device
    index.  insert() returns the slot a key ends up in when the inserts happen one after the other in call order."""

    def __init__(self, H):
        assert H > 0 and H & (H - 1) == 0
        self.H = H
        self.slot = [None] * H
        self.n = 0

    def insert(self, key):
        key = int(key)
        assert key != EMPTY_KEY and self.n < self.H
        h = home_of(key, self.H)
        while self.slot[h] is not None:
            if self.slot[h] == key:
                return h
            h = (h + 1) & (self.H - 1)
        self.slot[h] = key
        self.n += 1
        return h

    def find(self, key):
        key = int(key)
        h = home_of(key, self.H)
        while self.slot[h] is not None:
            if self.slot[h] == key:
                return h
            h = (h + 1) & (self.H - 1)
        return None

    def probes(self, key):
        """slots looked at until the key (or the empty slot that ends its chain) is found"""
        s = self.find(key)
        h = home_of(key, self.H)
        if s is None:
            s = h
            while self.slot[s] is not None:
                s = (s + 1) & (self.H - 1)
        return ((s - h) & (self.H - 1)) + 1

    def occupied(self):
        return [s for s in range(self.H) if self.slot[s] is not None]


# ---------------------------------------------------------------- shapes (H: slots of the table they are designed for)
LAST20 = (1 << 20) - 1
ONE_HOME_SIZES = (1, 2, 64, 65, 256, 257, 512)
MERGE_C = 400   # first home of merging_clusters


def one_home_wrap(n, H=1024):
    """n keys whose home is the LAST slot: the chain occupies H - 1, 0, 1, ..., n - 2"""
    return keys_for_homes([H - 1] * n)


def straddle(H=1024, n=300, start=0):
    """homes cycling over H - 3, H - 2, H - 1, 0, 1, 2: six chains that merge into one across the wrap"""
    cyc = [H - 3, H - 2, H - 1, 0, 1, 2]
    return keys_for_homes([cyc[j % 6] for j in range(n)], start=start)


def merging_clusters(H=1024, c=MERGE_C, n=100):
    """two runs of n keys with homes c and c + 60: the second cluster starts inside the first one's chain"""
    assert c + 60 + 2 * n < H
    return keys_for_homes([c] * n + [c + 60] * n)


def random_control(n=500, seed=12345):
    rng = np.random.default_rng(seed)
    keys = np.unique(rng.integers(0, M64, size=2 * n, dtype=np.uint64, endpoint=False))
    keys = rng.permutation(keys)[:n]
    assert len(keys) == n and EMPTY_KEY not in keys.tolist()
    return keys


def every_size_last_slot(n, start=0):
    """the hash has all of its low 20 bits set: the home is the last slot at EVERY table size up to 2^20 slots, so the
    chain wraps in the table a growth builds as it did in the one before"""
    return keys_for_homes([LAST20] * n, bits=20, start=start)


def unseen_in_chain(keys, H, m=40, start=1 << 30):
    """m keys that are not in `keys` and whose homes are occupied slots of the index that holds `keys`, spread evenly over
    them: inserting one walks an existing chain to its end"""
    model = IndexModel(H)
    for k in keys:
        model.insert(k)
    occ = model.occupied()
    extra = keys_for_homes([occ[i * len(occ) // m] for i in range(m)], start=start)
    assert not set(extra.tolist()) & set(int(k) for k in keys)
    return extra


def shape_keys(name, H=1024):
    """the keys of a named shape: one_home_wrap-<n>, straddle, merging_clusters, random_control"""
    if name.startswith("one_home_wrap-"):
        return one_home_wrap(int(name.split("-")[1]), H)
    return {"straddle": lambda: straddle(H), "merging_clusters": lambda: merging_clusters(H),
            "random_control": random_control}[name]()


SHAPES = ["one_home_wrap-%d" % n for n in ONE_HOME_SIZES] + ["straddle", "merging_clusters", "random_control"]


def reverse_bytes(x):
    """ReverseBytes (include/difacto/base.h:39-51), its own inverse: the raw id whose localized key is x"""
    x = int(x)
    x = ((x << 32) | (x >> 32)) & M64
    x = ((x & 0x0000FFFF0000FFFF) << 16) | ((x & 0xFFFF0000FFFF0000) >> 16)
    x = ((x & 0x00FF00FF00FF00FF) << 8) | ((x & 0xFF00FF00FF00FF00) >> 8)
    x = ((x & 0x0F0F0F0F0F0F0F0F) << 4) | ((x & 0xF0F0F0F0F0F0F0F0) >> 4)
    return x


def raw_ids(keys):
    return np.array([reverse_bytes(k) for k in keys], dtype=np.uint64)
