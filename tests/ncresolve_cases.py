"""The model and constructed cases of keys-to-handles over the resident NodeCache (dhtgpu_ncr_*,
opendht_amd/csrc/ncresolve.hip), shared by test_ncresolve_cpu.py and test_gpu_ncresolve.py.

The model wraps ncache_cases.Model (std::map<InfoHash, handle> as a dict + the accepted handles)
and states find, get_nodes and extract as the sequential loops of their semantics: what
NodeCache::NodeMap::getNode (src/node_cache.cpp:87-111) does node by node."""
import numpy as np

import ncache_cases as NC
import oracle as O

NONE = NC.NONE
# the lanes per key k_ncr_find ships (kNcrNarrowLanes / kNcrWideLanes) and the largest batch the wide
# form takes (kNcrWideMaxBatch) of opendht_amd/csrc/dhtgpu_internal.h, mirrored: the CPU test
# compares them
G_NARROW, G_WIDE = 16, 64
WIDE_MAX_BATCH = 5040


def find_sizes():
    """the n at which a G-lane descent changes depth, for each shipped G, and the sizes of the nc tests"""
    out = {0, 1, 2, 63, 64, 65, 4095, 4096, 4097, 70000}
    for g in (G_NARROW, G_WIDE):
        out |= {g - 1, g, g + 1, (g + 1) ** 2 - 1, (g + 1) ** 2, (g + 1) ** 2 + 1}
    return tuple(sorted(out))


FIND_SIZES = find_sizes()
FIND_BATCHES = (1, 63, 64, 65, 257, WIDE_MAX_BATCH, WIDE_MAX_BATCH + 1)   # both sides of the G switch
GET_SIZES = (0, 1, 64, 4096, 70000)
GET_BATCHES = (1, 4, 63, 64, 65, 257, 4097)


class Exhausted(Exception):
    def __init__(self, needed):
        Exception.__init__(self, f"needs {needed} free handles")
        self.needed = needed


class Model:
    """ncache_cases.Model + find / get_nodes / extract"""

    def __init__(self, nc=None):
        self.nc = nc if nc is not None else NC.Model()

    def find(self, ids):
        """(m,) handles (NONE: absent), (m,) accept bytes"""
        ids = NC.as_ids(ids)
        h = np.full(ids.shape[0], NONE, np.uint32)
        a = np.zeros(ids.shape[0], np.uint8)
        for j, k in enumerate(ids):
            got = self.nc.map.get(bytes(k))
            if got is not None:
                h[j] = got
                a[j] = got in self.nc.acc
        return h, a

    def get_nodes(self, ids, free, accept=None):
        """the emplace in batch order, an absent key under the next free handle: (m,) handles, (m,)
        new bytes, handles used.  Too few free handles: Exhausted(needed), the model untouched."""
        ids = NC.as_ids(ids)
        free = [int(f) for f in free]
        needed = len({bytes(k) for k in ids if bytes(k) not in self.nc.map})
        if needed > len(free):
            raise Exhausted(needed)
        h = np.full(ids.shape[0], NONE, np.uint32)
        new = np.zeros(ids.shape[0], np.uint8)
        used = 0
        for j, k in enumerate(ids):
            k = bytes(k)
            if k not in self.nc.map:
                f = free[used]
                used += 1
                self.nc.map[k] = f
                new[j] = 1
                if accept is None or accept[j]:
                    self.nc.acc.add(f)
                else:
                    self.nc.acc.discard(f)
            h[j] = self.nc.map[k]
        return h, new, used

    def extract(self, ids):
        """map.erase(key) in batch order: (m,) the handle each erased key held, else NONE"""
        ids = NC.as_ids(ids)
        h = np.full(ids.shape[0], NONE, np.uint32)
        for j, k in enumerate(ids):
            got = self.nc.map.pop(bytes(k), None)
            if got is not None:
                h[j] = got
        return h


def free_list(model, count, seed):
    """count distinct handles the model does not use, shuffled and non-contiguous"""
    used = set(model.nc.map.values())
    top = max(used) + 1 if used else 0
    pool = [h for h in range(0, top + 3 * count + 8, 2) if h not in used]
    pool += [h for h in range(1, top + 3 * count + 8, 2) if h not in used]
    rng = np.random.default_rng(seed)
    pick = rng.choice(len(pool), size=count, replace=False)
    return np.array([pool[i] for i in pick], dtype=np.uint32)


def find_probes(keys, m, seed):
    """Probe ids over a key set: all-zero, all-ones, the minimum - 1 and the maximum + 1, 96 sampled
    keys +- 1, the first and the last key, then every key when the set is small (else a sample of
    2,048).  m = None: all of them; else cut (the constructed probes are kept first) or padded (with
    random ids and repeats) to exactly m.  Shuffled, and the last probe repeats the first."""
    keys = NC.as_ids(keys)
    n = keys.shape[0]
    rng = np.random.default_rng(seed)
    rows = [np.zeros((1, 20), np.uint8), np.full((1, 20), 0xFF, np.uint8)]
    top = (1 << 160) - 1
    if n:
        ints = sorted(NC.key_int(k) for k in keys)
        rows.append(NC.as_ids(NC.int_key(max(ints[0] - 1, 0))))
        rows.append(NC.as_ids(NC.int_key(min(ints[-1] + 1, top))))
        sample = keys if n <= 4097 else keys[rng.choice(n, size=2048, replace=False)]
        for k in sample[rng.choice(sample.shape[0], size=min(sample.shape[0], 96), replace=False)]:
            x = NC.key_int(k)
            rows.append(NC.as_ids(NC.int_key(max(x - 1, 0))))
            rows.append(NC.as_ids(NC.int_key(min(x + 1, top))))
        rows.append(keys[[0, n - 1]])
        rows.append(sample)
    out = np.concatenate(rows)
    if m is not None and out.shape[0] < m:
        extra = m - out.shape[0]
        fresh = O.gen_ids(seed + 500, (extra + 1) // 2)
        out = np.concatenate([out, fresh, out[rng.integers(0, out.shape[0], size=extra - fresh.shape[0])]])
    out = out[: out.shape[0] if m is None else m]
    out = out[rng.permutation(out.shape[0])]
    if out.shape[0] >= 2:
        out[-1] = out[0]
    return np.ascontiguousarray(out)


def clustered_probes():
    """NC.clustered(): keys equal in words 0..3; probes that are keys, and absent probes that differ
    from a key in word 4 only.  Returns (keys, probes)."""
    keys, targets = NC.clustered()
    return keys, np.ascontiguousarray(np.concatenate([targets, keys[::7], keys[:3]]))


def id_planes(ids, stride):
    """(5 * stride,) uint32 word planes of (m, 20) ids, zero padded"""
    import opendht_amd
    ids = NC.as_ids(ids)
    planes = np.zeros((5, stride), np.uint32)
    if ids.shape[0]:
        planes[:, : ids.shape[0]] = opendht_amd.id_words(ids)
    return planes.reshape(-1)
