"""The resident NodeCache's model and constructed key sets (dhtgpu_nc_*, opendht_amd/csrc/ncache.hip),
shared by test_ncache_cpu.py and test_gpu_ncache.py.

The model is std::map<InfoHash, handle> as a Python dict (key bytes -> handle) plus the set of
accepted handles.  A lookup's expected answer is the project's own oracle, O.cached_nodes_batch
(NodeCache::getCachedNodes restated, built by build()), over the model's sorted keys with the
accept bytes in sorted order, its sorted positions mapped to handles."""
import numpy as np

import oracle as O

NONE = 0xFFFFFFFF
SIZES = (0, 1, 2, 63, 64, 65, 4095, 4096, 4097, 70000)   # the 64-ary search changes depth at 64 and 4096
COUNTS = (1, 8, 14, 32)
ACCEPTS = ("all", "none", "reject30", "ends")
MAX_HANDLE = 1 << 28   # DHTGPU_NC_MAX_HANDLE


def as_ids(rows):
    return np.ascontiguousarray(rows, dtype=np.uint8).reshape(-1, 20)


def key_int(k):
    return int.from_bytes(bytes(k), "big")


def int_key(x):
    return np.frombuffer(int(x).to_bytes(20, "big"), dtype=np.uint8)


class Model:
    def __init__(self):
        self.map = {}
        self.acc = set()

    def set(self, ids, handles=None):
        ids = as_ids(ids)
        handles = range(ids.shape[0]) if handles is None else [int(h) for h in handles]
        self.map = {bytes(k): h for k, h in zip(ids, handles)}
        assert len(self.map) == ids.shape[0], "duplicate keys"
        self.acc = set(handles)

    def insert(self, ids, handles, accept=None):
        """std::map::emplace in batch order; returns the per-key 'inserted' bytes"""
        ids = as_ids(ids)
        new = np.zeros(ids.shape[0], np.uint8)
        for j, (k, h) in enumerate(zip(ids, handles)):
            k = bytes(k)
            if k in self.map:
                continue
            self.map[k] = int(h)
            new[j] = 1
            if accept is None or accept[j]:
                self.acc.add(int(h))
            else:
                self.acc.discard(int(h))
        return new

    def erase(self, ids):
        """map.erase(key) in batch order; returns the per-key 'erased' bytes"""
        ids = as_ids(ids)
        found = np.zeros(ids.shape[0], np.uint8)
        for j, k in enumerate(ids):
            if self.map.pop(bytes(k), None) is not None:
                found[j] = 1
        return found

    def update_accept(self, handles, val):
        for h, v in zip(handles, np.broadcast_to(np.asarray(val), (len(handles),))):
            (self.acc.add if v else self.acc.discard)(int(h))

    def set_accept(self, by_handle):
        for h, v in enumerate(by_handle):
            (self.acc.add if v else self.acc.discard)(h)

    def sorted(self):
        """(n, 20) keys in lexicographic order, (n,) their handles"""
        items = sorted(self.map.items())
        keys = as_ids(np.frombuffer(b"".join(k for k, _ in items), dtype=np.uint8)) if items else np.zeros((0, 20), np.uint8)
        return keys, np.array([h for _, h in items], dtype=np.uint32)

    def expected(self, targets, count):
        """(q, count) handles in the reference's walk order (NONE padded), (q,) counts"""
        keys, handles = self.sorted()
        q = len(targets)
        if keys.shape[0] == 0:
            return np.full((q, count), NONE, np.uint32), np.zeros(q, np.uint32)
        acc = np.array([h in self.acc for h in handles], dtype=np.uint8)
        pos, cnt = O.cached_nodes_batch(keys, acc, as_ids(targets), count, threads=8)
        out = np.where(pos == NONE, NONE, handles[np.minimum(pos, keys.shape[0] - 1)]).astype(np.uint32)
        return out, cnt


def accept_handles(kind, sorted_handles, seed=5):
    """the accepted handles of one accept kind over a mirror's handles in sorted-key order"""
    h = np.asarray(sorted_handles, dtype=np.uint32)
    if kind == "all":
        return set(int(x) for x in h)
    if kind == "none":
        return set()
    if kind == "reject30":
        keep = np.random.default_rng(seed).random(h.shape[0]) >= 0.3
        return set(int(x) for x in h[keep])
    if kind == "ends":   # only the lowest and the highest key: the walk crosses the whole array from both ends
        return set(int(x) for x in h[[0, -1]]) if h.size else set()
    raise ValueError(kind)


def targets_for(keys, seed, nrand=12):
    """random targets, targets equal to a key, one below the minimum, one above the maximum, all-zero, all-ones"""
    keys = as_ids(keys)
    rows = [O.gen_ids(seed + 1000, nrand)]
    if keys.shape[0]:
        srt = sorted(key_int(k) for k in keys)
        pick = np.random.default_rng(seed).integers(0, keys.shape[0], size=min(6, keys.shape[0]))
        rows.append(keys[pick])
        rows.append(keys[[0, keys.shape[0] - 1]])
        rows.append(as_ids(int_key(max(srt[0] - 1, 0))))
        rows.append(as_ids(int_key(min(srt[-1] + 1, (1 << 160) - 1))))
        rows.append(as_ids(int_key(srt[0])))
        rows.append(as_ids(int_key(srt[-1])))
    rows.append(np.zeros((1, 20), np.uint8))
    rows.append(np.full((1, 20), 0xFF, np.uint8))
    return np.ascontiguousarray(np.concatenate(rows))


def prefix_key(nibble, rest=0):
    """a key whose top 4 bits are `nibble`, the other 156 bits `rest`"""
    return int_key((nibble << 156) | rest)


def non_monotone():
    """Keys on 4-bit prefixes around the target 0111...: the previous side holds 0000..., the next
    side 1000..., 1001..., then filler 1010... 1111....  The walk takes 0000... (distance 0111...),
    then the next side in KEY order -- distances 1111..., 1110..., 1101..., ... -- while a sort by
    distance would reverse that side.  Returns (keys, target)."""
    nibbles = [0x0, 0x8, 0x9, 0xA, 0xB, 0xC, 0xD, 0xE, 0xF]
    keys = as_ids(np.stack([prefix_key(nb) for nb in nibbles]))
    target = as_ids(int_key((0x7 << 156) | ((1 << 156) - 1)))
    return keys, target


def distance_sorted(keys, accept, target, count):
    """what a kernel that sorts by XOR distance would return: sorted positions"""
    t = key_int(target)
    order = sorted((key_int(k) ^ t, i) for i, k in enumerate(keys) if accept[i])
    return [i for _, i in order[:count]]


def clustered(seed=17, n=200):
    """n keys equal in words 0..3 that differ only in word 4, and targets inside the cluster
    (some equal to a key).  Returns (keys, targets)."""
    rng = np.random.default_rng(seed)
    head = rng.integers(0, 256, size=16, dtype=np.uint8)
    tails = rng.choice(1 << 32, size=n + 24, replace=False).astype(">u4")
    rows = np.zeros((n + 24, 20), np.uint8)
    rows[:, :16] = head
    rows[:, 16:] = tails.view(np.uint8).reshape(-1, 4)
    keys, extra = rows[:n], rows[n:]
    targets = np.concatenate([extra, keys[::25]])
    return np.ascontiguousarray(keys), np.ascontiguousarray(targets)


def mutation_batch(model, m, seed, next_handle):
    """An insert batch of m keys over the model's current keys: fresh random keys, keys already
    present, one key twice with different handles (the first must win), the smallest and the
    largest possible key.  Returns (ids, handles, accept)."""
    rng = np.random.default_rng(seed)
    fresh = O.gen_ids(seed + 77, m)
    ids = fresh.copy()
    present = list(model.map.keys())
    if present and m >= 8:
        for j in rng.choice(m, size=min(m // 4, len(present)), replace=False):
            ids[j] = np.frombuffer(present[int(rng.integers(0, len(present)))], dtype=np.uint8)
    if m >= 4:
        ids[m - 1] = ids[0]          # the same key twice, different handles
        ids[1] = 0                   # the smallest possible key
        ids[2] = 0xFF                # the largest possible key
    handles = np.arange(next_handle, next_handle + m, dtype=np.uint32)
    accept = (rng.random(m) >= 0.25).astype(np.uint8)
    return np.ascontiguousarray(ids), handles, accept
