"""opendht_amd -- Python host binding for libdhtgpu, the MI355X engine behind
OpenDHT's XOR-closest-node lookup.

This is a thin ctypes layer over the C ABI declared in include/dhtgpu.h; every
compute call runs the hand-written HIP kernels in opendht_amd/libdhtgpu.so.  There is
no CPU fallback: if the native library is missing or cannot be loaded, import of the
compute API raises.

Reference interfaces mirrored (OpenDHT tree paths):
  Context.topk            std::partial_sort(.., InfoHash::xorCmp)  (include/opendht/infohash.h:179-194)
  Context.find_closest    RoutingTable::findClosestNodes            (src/routing_table.cpp:110-150)
  Context.cached_nodes    NodeCache::getCachedNodes                 (src/node_cache.cpp:42-74)
  Context.cache_set/_nodes  the NodeCache mirror: unsorted keys sorted on the device (node_cache.h:43)
  Context.classify        RoutingTable::findBucket + InfoHash::commonBits
  Context.rt_set / rt_reply / rt_closer  the routing table resident on the device: onFindNode / onGetValues'
                          findClosestNodes + bufferNodes fused; maintainStorage / onAnnounce closeness tests
  Context.nc_set / nc_insert / nc_erase / nc_nodes  NodeCache's map resident on the device, changed
                          incrementally; getCachedNodes one wave per target (src/node_cache.cpp:42-123)
  Context.ncr_find / ncr_get_nodes / ncr_extract  NodeMap::getNode in batches over it: ids to handles
  Context.sr_reset / sr_open / sr_insert / sr_refill / sr_status / sr_lists  the searches' node lists
  Context.srs_set_clock / srs_set_request / srs_step / srs_entries  Dht::searchStep on those lists
  Context.srm_set / srm_set_done / srm_offer / srm_export  Dht::trySearchInsert over their ordered map
                          resident on the device: Search::insertNode one wave per search
                          (src/search.h:636-722), Dht::refill fused with getCachedNodes (src/dht.cpp:656-677)
"""
import ctypes
import os

import numpy as np

__all__ = ["Context", "DhtGpuError", "NONE", "MAX_K", "lib", "LIB_PATH", "id_words", "batch_plan"]

# DHTGPU_LIB: another build of the same library (A/B experiments, tools/experiments/gpu_ab_lib.sh)
LIB_PATH = os.environ.get("DHTGPU_LIB") or os.path.join(os.path.dirname(os.path.abspath(__file__)), "libdhtgpu.so")
NONE = 0xFFFFFFFF
MAX_K = 32
SR_CAP = 64   # DHTGPU_SR_CAP: entries per resident search row
# DHTGPU_RTG_*: the results of rtg_on_new_node
RTG_NONE, RTG_KNOWN, RTG_PLACED, RTG_REPLACED, RTG_FULL, RTG_UNAPPLIED = range(6)
RTG_MAX_HANDLE = 65536
# status codes (include/dhtgpu.h)
EINVAL, ENOMEM, EDEVICE, ENOIDS, EUNSORTED, ERANGE = -1, -2, -3, -4, -5, -6

_u8p = ctypes.POINTER(ctypes.c_uint8)
_u32p = ctypes.POINTER(ctypes.c_uint32)
_u64p = ctypes.POINTER(ctypes.c_uint64)
_vp = ctypes.c_void_p
_lib = None


class DhtGpuError(RuntimeError):
    def __init__(self, code, what=""):
        msg = _lib.dhtgpu_strerror(code).decode() if _lib is not None else str(code)
        super().__init__(f"libdhtgpu: {what}: {msg} ({code})")
        self.code = code


def _check(code, what):
    if code != 0:
        raise DhtGpuError(code, what)


# Every entry point of include/dhtgpu.h: argument types, result type.
_SIG = {
        "dhtgpu_strerror": ([ctypes.c_int], ctypes.c_char_p),
        "dhtgpu_device_count": ([ctypes.POINTER(ctypes.c_int)], ctypes.c_int),
        "dhtgpu_ctx_create": ([ctypes.c_int, ctypes.POINTER(_vp)], ctypes.c_int),
        "dhtgpu_ctx_destroy": ([_vp], None),
        "dhtgpu_ctx_stream": ([_vp], _vp),
        "dhtgpu_set_ids": ([_vp, _u8p, ctypes.c_uint64], ctypes.c_int),
        "dhtgpu_gen_ids": ([_vp, ctypes.c_uint64, ctypes.c_uint64, ctypes.c_uint64], ctypes.c_int),
        "dhtgpu_num_ids": ([_vp], ctypes.c_uint64),
        "dhtgpu_set_accept": ([_vp, _u8p], ctypes.c_int),
        "dhtgpu_set_accept_bits_dev": ([_vp, _vp, _vp], ctypes.c_int),
        "dhtgpu_update_accept": ([_vp, _u32p, _u8p, ctypes.c_uint64], ctypes.c_int),
        "dhtgpu_num_accepted": ([_vp, _u64p], ctypes.c_int),
        "dhtgpu_write_ids": ([_vp, ctypes.c_uint64, _u8p, ctypes.c_uint64], ctypes.c_int),
        "dhtgpu_set_global_indices": ([_vp, ctypes.c_int], ctypes.c_int),
        "dhtgpu_set_sub_handles": ([_vp, ctypes.c_int], ctypes.c_int),
        "dhtgpu_sub_handles_active": ([_vp, ctypes.c_uint32, ctypes.c_uint32], ctypes.c_int),
        "dhtgpu_handles_to_indices_dev": ([_vp, _vp, ctypes.c_uint64, _vp, ctypes.c_uint32, _vp], ctypes.c_int),
        "dhtgpu_set_search_alpha": ([_vp, ctypes.c_uint32], ctypes.c_int),
        "dhtgpu_get_ids": ([_vp, ctypes.c_uint64, ctypes.c_uint64, _u8p], ctypes.c_int),
        "dhtgpu_ids_dev": ([_vp, ctypes.POINTER(_vp), ctypes.POINTER(ctypes.c_uint64)], ctypes.c_int),
        "dhtgpu_topk": ([_vp, _u8p, ctypes.c_uint32, ctypes.c_uint32, _u32p, _u32p], ctypes.c_int),
        "dhtgpu_topk_dev": ([_vp, _vp, ctypes.c_uint64, ctypes.c_uint32, ctypes.c_uint32, _vp, _vp, _vp,
                             ctypes.c_uint32, _vp], ctypes.c_int),
        "dhtgpu_merge_dev": ([_vp, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32, _vp, ctypes.c_uint64,
                              ctypes.c_uint32, _vp, _vp, _vp, ctypes.c_uint32, _vp], ctypes.c_int),
        "dhtgpu_tie_words_dev": ([_vp, _vp, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32, _vp, ctypes.c_uint32,
                                  ctypes.c_uint32, _vp, _vp], ctypes.c_int),
        "dhtgpu_merge_ties_dev": ([_vp, _vp, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32, _vp, ctypes.c_uint64,
                                   ctypes.c_uint32, _vp, ctypes.c_uint32, _vp, _vp, _vp], ctypes.c_int),
        "dhtgpu_pack_dev": ([_vp, ctypes.c_uint64, _vp, ctypes.c_uint64, _vp], ctypes.c_int),
        "dhtgpu_gen_dev": ([ctypes.c_uint64, ctypes.c_uint64, ctypes.c_uint64, _vp, ctypes.c_uint64, _vp],
                           ctypes.c_int),
        "dhtgpu_find_closest": ([_vp, ctypes.c_uint32, _u8p, _u32p, _u8p, _u8p, _u8p, ctypes.c_uint32,
                                 ctypes.c_uint32, _u32p, _u32p], ctypes.c_int),
        "dhtgpu_classify": ([_vp, ctypes.c_uint32, _u8p, _u8p, _u8p, _u64p], ctypes.c_int),
        "dhtgpu_classify_dev": ([_vp, ctypes.c_uint64, ctypes.c_uint64, ctypes.c_uint32, _vp, _u32p, _vp, _vp,
                                 _vp], ctypes.c_int),
        "dhtgpu_cached_nodes": ([_vp, _u8p, _u8p, ctypes.c_uint32, ctypes.c_uint32, _u32p, _u32p],
                                ctypes.c_int),
        "dhtgpu_cache_set": ([_vp, _u8p, ctypes.c_uint64, ctypes.c_uint64], ctypes.c_int),
        "dhtgpu_batch_events": ([_vp, ctypes.POINTER(_vp)], ctypes.c_int),
        "dhtgpu_search_insert": ([_vp, _u8p, _u8p, ctypes.c_uint32, _u8p, ctypes.c_uint32, ctypes.c_uint32, _u32p, _u8p,
                                  _u32p, _u8p, _u64p, _u32p, _u8p, _u8p], ctypes.c_int),
        "dhtgpu_table_stats": ([_vp, ctypes.c_uint32, _u8p, ctypes.POINTER(ctypes.c_int32), _u32p], ctypes.c_int),
        "dhtgpu_cache_nodes": ([_vp, _u8p, _u8p, ctypes.c_uint32, ctypes.c_uint32, _u32p, _u32p], ctypes.c_int),
        "dhtgpu_cache_sorted": ([_vp, _u32p], ctypes.c_int),
        "dhtgpu_buffer_nodes_ids": ([_vp, _u8p, _u8p, ctypes.c_uint32, ctypes.c_uint32, _u8p, ctypes.c_uint32, _u32p,
                                     ctypes.c_uint32, _u8p, _u32p], ctypes.c_int),
        "dhtgpu_index_build": ([_vp, _vp], ctypes.c_int),
        "dhtgpu_index_topk_dev": ([_vp, _vp, ctypes.c_uint64, ctypes.c_uint32, ctypes.c_uint32, _vp, _vp, _vp,
                                   ctypes.c_uint32, _vp], ctypes.c_int),
        "dhtgpu_index_topk": ([_vp, _u8p, ctypes.c_uint32, ctypes.c_uint32, _u32p, _u32p], ctypes.c_int),
        "dhtgpu_index_build_timed": ([_vp, _vp, ctypes.POINTER(ctypes.c_float)], ctypes.c_int),
        "dhtgpu_gen_ids_prefix": ([_vp, ctypes.c_uint64, ctypes.c_uint64, ctypes.c_uint64, ctypes.c_uint32,
                                   ctypes.c_uint32], ctypes.c_int),
        "dhtgpu_select_prefix_dev": ([_vp, _vp, ctypes.c_uint64, ctypes.c_uint64, ctypes.c_uint32, ctypes.c_uint32,
                                      _vp, ctypes.c_uint64, _vp, _u64p, _vp], ctypes.c_int),
        "dhtgpu_batch_topk_dev": ([_vp, _vp, ctypes.c_uint64, ctypes.c_uint32, ctypes.c_uint32, _vp, _vp, _vp,
                                   ctypes.c_uint32, _vp], ctypes.c_int),
        "dhtgpu_batch_topk_timed": ([_vp, _vp, ctypes.c_uint64, ctypes.c_uint32, ctypes.c_uint32, _vp, _vp, _vp,
                                     ctypes.POINTER(ctypes.c_float), _u32p], ctypes.c_int),
        "dhtgpu_batch_topk": ([_vp, _u8p, ctypes.c_uint32, ctypes.c_uint32, _u32p, _u32p], ctypes.c_int),
        "dhtgpu_batch_plan": ([_vp, ctypes.c_int, ctypes.c_uint64, ctypes.c_uint32, ctypes.c_uint32, _u32p],
                              ctypes.c_int),
        "dhtgpu_table_depth": ([ctypes.c_uint32, _u8p, ctypes.c_uint32, _u32p], ctypes.c_int),
        "dhtgpu_buffer_nodes_dev": ([_vp, _vp, ctypes.c_uint32, _vp, ctypes.c_uint64, ctypes.c_uint32, _vp,
                                     ctypes.c_uint32, _vp, _vp, _vp], ctypes.c_int),
        "dhtgpu_buffer_nodes": ([_vp, _u8p, ctypes.c_uint32, _u8p, ctypes.c_uint32, _u32p, ctypes.c_uint32, _u8p,
                                 _u32p], ctypes.c_int),
        "dhtgpu_deserialize_nodes": ([_vp, ctypes.c_uint32, _u8p, _u8p, _u64p, ctypes.c_uint32, _u8p, _u8p, _u8p,
                                      _u8p, _u8p, _u8p, _u32p], ctypes.c_int),
        "dhtgpu_net_prepare": ([_vp, _u8p, ctypes.c_uint64], ctypes.c_int),
        "dhtgpu_search_batch": ([_vp, _u8p, ctypes.c_uint32, _u32p, ctypes.c_uint32, _u32p, _u8p, _u32p, _u32p,
                                 _u32p], ctypes.c_int),
        "dhtgpu_search_batch_dev": ([_vp, _vp, ctypes.c_uint64, ctypes.c_uint32, _vp, ctypes.c_uint32, _vp, _vp,
                                     _vp, _vp, _vp, _vp], ctypes.c_int),
        "dhtgpu_rt_set": ([_vp, _u8p, ctypes.c_uint32, _u8p, _u32p, _u8p, _u8p, ctypes.c_uint32, ctypes.c_uint64],
                          ctypes.c_int),
        "dhtgpu_rt_set_good": ([_vp, _u8p], ctypes.c_int),
        "dhtgpu_rt_update_good": ([_vp, _u32p, _u8p, ctypes.c_uint32], ctypes.c_int),
        "dhtgpu_rt_find_closest_dev": ([_vp, _vp, ctypes.c_uint64, ctypes.c_uint32, ctypes.c_uint32, _vp, _vp, _vp],
                                       ctypes.c_int),
        "dhtgpu_rt_find_closest": ([_vp, _u8p, ctypes.c_uint32, ctypes.c_uint32, _u32p, _u32p], ctypes.c_int),
        "dhtgpu_rt_reply_dev": ([_vp, _vp, ctypes.c_uint64, ctypes.c_uint32, _vp, _vp, _vp, _vp], ctypes.c_int),
        "dhtgpu_rt_reply": ([_vp, _u8p, ctypes.c_uint32, _u8p, _u32p, _u32p], ctypes.c_int),
        "dhtgpu_rt_closer_dev": ([_vp, _vp, ctypes.c_uint64, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32, _vp,
                                  _vp, _vp], ctypes.c_int),
        "dhtgpu_rt_closer": ([_vp, _u8p, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32, _u8p, _u32p],
                             ctypes.c_int),
        "dhtgpu_rtg_on_new_node": ([_vp, _u8p, _u32p, _u8p, _u8p, ctypes.c_uint32, ctypes.c_uint32, _u8p, _u32p, _u32p],
                                   ctypes.c_int),
        "dhtgpu_rtg_expire": ([_vp, _u32p, _u32p], ctypes.c_int),
        "dhtgpu_rtg_set_state": ([_vp, _u8p, ctypes.c_uint32], ctypes.c_int),
        "dhtgpu_rtg_update_state": ([_vp, _u32p, _u8p, ctypes.c_uint32], ctypes.c_int),
        "dhtgpu_rtg_size": ([_vp, _u32p, _u32p], ctypes.c_int),
        "dhtgpu_rtg_export": ([_vp, _u8p, _u32p, _u8p, _u32p, _u8p], ctypes.c_int),
        "dhtgpu_nc_set": ([_vp, _u8p, _u32p, ctypes.c_uint64], ctypes.c_int),
        "dhtgpu_nc_insert": ([_vp, _u8p, _u32p, _u8p, ctypes.c_uint32, _u8p], ctypes.c_int),
        "dhtgpu_nc_erase": ([_vp, _u8p, ctypes.c_uint32, _u8p], ctypes.c_int),
        "dhtgpu_nc_update_accept": ([_vp, _u32p, _u8p, ctypes.c_uint32], ctypes.c_int),
        "dhtgpu_nc_set_accept": ([_vp, _u8p, ctypes.c_uint32], ctypes.c_int),
        "dhtgpu_nc_size": ([_vp, _u64p], ctypes.c_int),
        "dhtgpu_nc_export": ([_vp, _u8p, _u32p], ctypes.c_int),
        "dhtgpu_nc_nodes_dev": ([_vp, _vp, ctypes.c_uint64, ctypes.c_uint32, ctypes.c_uint32, _vp, _vp, _vp],
                                ctypes.c_int),
        "dhtgpu_nc_nodes": ([_vp, _u8p, ctypes.c_uint32, ctypes.c_uint32, _u32p, _u32p], ctypes.c_int),
        "dhtgpu_ncr_find": ([_vp, _u8p, ctypes.c_uint32, _u32p, _u8p], ctypes.c_int),
        "dhtgpu_ncr_find_dev": ([_vp, _vp, ctypes.c_uint64, ctypes.c_uint32, _vp, _vp, _vp], ctypes.c_int),
        "dhtgpu_ncr_get_nodes": ([_vp, _u8p, ctypes.c_uint32, _u32p, ctypes.c_uint32, _u8p, _u32p, _u8p, _u32p],
                                 ctypes.c_int),
        "dhtgpu_ncr_extract": ([_vp, _u8p, ctypes.c_uint32, _u32p], ctypes.c_int),
        "dhtgpu_sr_reset": ([_vp, ctypes.c_uint32], ctypes.c_int),
        "dhtgpu_sr_open": ([_vp, _u32p, _u8p, ctypes.c_uint32], ctypes.c_int),
        "dhtgpu_sr_expire": ([_vp, _u32p, ctypes.c_uint32], ctypes.c_int),
        "dhtgpu_sr_set_state": ([_vp, _u8p, ctypes.c_uint32], ctypes.c_int),
        "dhtgpu_sr_update_state": ([_vp, _u32p, _u8p, ctypes.c_uint32], ctypes.c_int),
        "dhtgpu_sr_set_candidate": ([_vp, _u32p, _u32p, _u8p, ctypes.c_uint32], ctypes.c_int),
        "dhtgpu_sr_insert": ([_vp, _u32p, ctypes.c_uint32, _u64p, _u32p, _u8p, _u8p, _u8p], ctypes.c_int),
        "dhtgpu_sr_insert_dev": ([_vp, _vp, ctypes.c_uint32, _vp, _vp, _vp, ctypes.c_uint64, _vp, _vp, _vp],
                                 ctypes.c_int),
        "dhtgpu_sr_refill": ([_vp, _u32p, ctypes.c_uint32, ctypes.c_uint32, _u32p], ctypes.c_int),
        "dhtgpu_sr_refill_dev": ([_vp, _vp, ctypes.c_uint32, ctypes.c_uint32, _vp, _vp], ctypes.c_int),
        "dhtgpu_sr_status": ([_vp, _u32p, ctypes.c_uint32, _u32p], ctypes.c_int),
        "dhtgpu_sr_status_dev": ([_vp, _vp, ctypes.c_uint32, _vp, _vp], ctypes.c_int),
        "dhtgpu_sr_lists": ([_vp, _u32p, ctypes.c_uint32, _u32p, _u8p, _u32p], ctypes.c_int),
        "dhtgpu_sr_lists_dev": ([_vp, _vp, ctypes.c_uint32, _vp, _vp, _vp, _vp], ctypes.c_int),
        "dhtgpu_srs_set_clock": ([_vp, ctypes.c_uint32], ctypes.c_int),
        "dhtgpu_srs_set_request": ([_vp, _u32p, _u32p, _u8p, ctypes.c_uint32], ctypes.c_int),
        "dhtgpu_srs_step": ([_vp, _u32p, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32, _u32p, _u32p], ctypes.c_int),
        "dhtgpu_srs_step_dev": ([_vp, _vp, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32, _vp, _vp, _vp], ctypes.c_int),
        "dhtgpu_srs_entries": ([_vp, _u32p, ctypes.c_uint32, _u8p, _u32p], ctypes.c_int),
        "dhtgpu_srs_entries_dev": ([_vp, _vp, ctypes.c_uint32, _vp, _vp, _vp], ctypes.c_int),
        "dhtgpu_srm_set": ([_vp, _u32p, ctypes.c_uint32], ctypes.c_int),
        "dhtgpu_srm_set_done": ([_vp, _u32p, _u8p, ctypes.c_uint32], ctypes.c_int),
        "dhtgpu_srm_offer": ([_vp, _u32p, _u8p, ctypes.c_uint32, _u32p, _u32p, _u32p], ctypes.c_int),
        "dhtgpu_srm_offer_dev": ([_vp, _vp, _vp, ctypes.c_uint64, ctypes.c_uint32, _vp, _vp, _vp, _vp], ctypes.c_int),
        "dhtgpu_srm_export": ([_vp, _u32p, _u8p, _u32p], ctypes.c_int),
}


def lib():
    """Load libdhtgpu.so (raises if absent: there is no fallback path)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError(f"libdhtgpu.so not built at {LIB_PATH}: run `python -c 'import __graft_entry__ as g; g.build()'`")
    try:  # share the HIP runtime with torch when both live in the process
        import torch  # noqa: F401
    except Exception:
        pass
    L = ctypes.CDLL(LIB_PATH)
    for name, (args, res) in _SIG.items():
        if os.environ.get("DHTGPU_LIB") and not hasattr(L, name):
            continue   # an A/B build of an earlier commit (yardstick runs): calling the entry raises
        f = getattr(L, name)
        f.argtypes = args
        f.restype = res
    _lib = L
    return L


def exported_symbols():
    """Names of every entry point declared in include/dhtgpu.h (for the ABI test)."""
    return list(_SIG)


def _ids(a, name="ids"):
    a = np.ascontiguousarray(a, dtype=np.uint8)
    if a.ndim == 1:
        a = a.reshape(-1, 20)
    if a.ndim != 2 or a.shape[1] != 20:
        raise ValueError(f"{name}: expected (n, 20) uint8 big-endian InfoHash bytes, got {a.shape}")
    return a


def _p(a, t):
    return a.ctypes.data_as(t)


def id_words(ids):
    """(n,20) big-endian bytes -> (5, n) uint32 word planes (the device layout)."""
    ids = _ids(ids)
    return ids.view(">u4").reshape(-1, 5).astype(np.uint32).T.copy()


class Context:
    """One device context (mirrors the reference's single dht_thread ownership:
    not thread-safe, calls are synchronous)."""

    def __init__(self, device=0):
        L = lib()
        h = _vp()
        _check(L.dhtgpu_ctx_create(int(device), ctypes.byref(h)), "ctx_create")
        self._h = h
        self.device = device

    def close(self):
        if getattr(self, "_h", None):
            lib().dhtgpu_ctx_destroy(self._h)
            self._h = None

    def __del__(self):
        self.close()

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    @property
    def stream(self):
        return lib().dhtgpu_ctx_stream(self._h)

    # ---- id set -------------------------------------------------------------
    def set_ids(self, ids):
        ids = _ids(ids)
        _check(lib().dhtgpu_set_ids(self._h, _p(ids, _u8p), ids.shape[0]), "set_ids")

    def gen_ids(self, seed, n, start=0):
        _check(lib().dhtgpu_gen_ids(self._h, seed, start, n), "gen_ids")

    def gen_ids_prefix(self, seed, n, pbits, pval, start=0):
        """Keep the ids of the stream [start, start+n) whose top pbits bits == pval
        (a prefix shard); result indices refer to the global stream."""
        _check(lib().dhtgpu_gen_ids_prefix(self._h, seed, start, n, pbits, pval), "gen_ids_prefix")

    def set_global_indices(self, on):
        """Prefix shards: results as global stream indices (True, default) or shard-local."""
        _check(lib().dhtgpu_set_global_indices(self._h, int(bool(on))), "set_global_indices")

    def set_sub_handles(self, on):
        """Sub-partitioned calls (sets one K6 plan cannot serve) return sub-partition handles
        instead of indices (no per-result index-map read); see include/dhtgpu.h."""
        _check(lib().dhtgpu_set_sub_handles(self._h, int(bool(on))), "set_sub_handles")

    def sub_handles_active(self, q, k):
        """True when a call of q targets at k returns handles."""
        return bool(lib().dhtgpu_sub_handles_active(self._h, q, k))

    def handles_to_indices_dev(self, handles_ptr, m, out_ptr, idx_base=0, stream=None):
        """m handles -> the indices the call would have returned (device pointers)."""
        _check(lib().dhtgpu_handles_to_indices_dev(self._h, handles_ptr, m, out_ptr, idx_base, stream),
               "handles_to_indices_dev")

    def select_prefix_dev(self, planes_ptr, stride, n, pbits, pval, out_planes_ptr, out_stride, out_gidx_ptr=None,
                          stream=None):
        cnt = ctypes.c_uint64()
        _check(lib().dhtgpu_select_prefix_dev(self._h, planes_ptr, stride, n, pbits, pval, out_planes_ptr, out_stride,
                                              out_gidx_ptr, ctypes.byref(cnt), stream), "select_prefix_dev")
        return cnt.value

    # ---- accept mask (Node::isGood for the flat k-NN) --------------------------
    def set_accept(self, mask):
        """(n,) bool/uint8 mask over the id set (nonzero = accepted), or None to clear it.  While a
        mask is set topk / index_topk / batch_topk (and their _dev forms) answer from the accepted
        ids only; indices stay those of the original set."""
        m = None
        if mask is not None:
            m = np.ascontiguousarray(np.asarray(mask).reshape(-1) != 0, dtype=np.uint8)
            if m.shape[0] != self.num_ids:
                raise ValueError("accept mask must have one byte per id")
        _check(lib().dhtgpu_set_accept(self._h, _p(m, _u8p) if m is not None else None), "set_accept")

    def set_accept_bits_dev(self, bits_ptr, stream=None):
        """Device bitmask of ceil(n/32) uint32 words (id i = bit i & 31 of word i >> 5), copied
        stream-ordered."""
        _check(lib().dhtgpu_set_accept_bits_dev(self._h, bits_ptr, stream), "set_accept_bits_dev")

    def update_accept(self, idx, val):
        """accept[idx[j]] = val[j] (val: array or one value for all)."""
        i = np.ascontiguousarray(idx, dtype=np.uint32).reshape(-1)
        v = np.ascontiguousarray(np.broadcast_to(np.asarray(val), i.shape)).astype(np.uint8).reshape(-1)
        _check(lib().dhtgpu_update_accept(self._h, _p(i, _u32p), _p(v, _u8p), i.shape[0]), "update_accept")

    @property
    def num_accepted(self):
        """Ids currently accepted (brings the mask's view up to date)."""
        out = ctypes.c_uint64()
        _check(lib().dhtgpu_num_accepted(self._h, ctypes.byref(out)), "num_accepted")
        return int(out.value)

    def write_ids(self, first, ids):
        """Overwrite ids [first, first + len(ids)) in place (slot reuse); keeps the mask."""
        ids = _ids(ids)
        _check(lib().dhtgpu_write_ids(self._h, int(first), _p(ids, _u8p), ids.shape[0]), "write_ids")

    @property
    def num_ids(self):
        return int(lib().dhtgpu_num_ids(self._h))

    def get_ids(self, first=0, n=None):
        if n is None:
            n = self.num_ids - first
        out = np.empty((n, 20), dtype=np.uint8)
        _check(lib().dhtgpu_get_ids(self._h, first, n, _p(out, _u8p)), "get_ids")
        return out

    def ids_dev(self):
        p, s = _vp(), ctypes.c_uint64()
        _check(lib().dhtgpu_ids_dev(self._h, ctypes.byref(p), ctypes.byref(s)), "ids_dev")
        return p.value, s.value

    # ---- K1: flat exact top-k ---------------------------------------------------
    def topk(self, targets, k=8):
        """findClosestNodesBatch(targets[], k): (q,k) uint32 indices (NONE padded), (q,) counts."""
        t = _ids(targets, "targets")
        q = t.shape[0]
        out = np.empty((q, k), dtype=np.uint32)
        cnt = np.empty(q, dtype=np.uint32)
        _check(lib().dhtgpu_topk(self._h, _p(t, _u8p), q, k, _p(out, _u32p), _p(cnt, _u32p)), "topk")
        return out, cnt

    def index_topk(self, targets, k=8):
        """Same result as topk() through the K4/K5 bucket index (built on first use)."""
        t = _ids(targets, "targets")
        q = t.shape[0]
        out = np.empty((q, k), dtype=np.uint32)
        cnt = np.empty(q, dtype=np.uint32)
        _check(lib().dhtgpu_index_topk(self._h, _p(t, _u8p), q, k, _p(out, _u32p), _p(cnt, _u32p)), "index_topk")
        return out, cnt

    def index_build(self, stream=None):
        _check(lib().dhtgpu_index_build(self._h, stream), "index_build")

    def index_build_timed(self, stream=None):
        """Build with HIP events between kernels; returns device ms per phase:
        (P0 histogram, P0 scans, P1 partition scatter, P2 bucket gather)."""
        ms = (ctypes.c_float * 4)()
        _check(lib().dhtgpu_index_build_timed(self._h, stream, ms), "index_build_timed")
        return tuple(ms)

    def index_topk_dev(self, t_planes_ptr, t_stride, q, k, out_idx_ptr=None, out_cnt_ptr=None, out_rec_ptr=None,
                       idx_base=0, stream=None):
        _check(lib().dhtgpu_index_topk_dev(self._h, t_planes_ptr, t_stride, q, k, out_idx_ptr, out_cnt_ptr,
                                           out_rec_ptr, idx_base, stream), "index_topk_dev")

    def batch_topk(self, targets, k=8):
        """Same result as topk() through the K6 per-batch target-prefix filter."""
        t = _ids(targets, "targets")
        q = t.shape[0]
        out = np.empty((q, k), dtype=np.uint32)
        cnt = np.empty(q, dtype=np.uint32)
        _check(lib().dhtgpu_batch_topk(self._h, _p(t, _u8p), q, k, _p(out, _u32p), _p(cnt, _u32p)), "batch_topk")
        return out, cnt

    def batch_topk_dev(self, t_planes_ptr, t_stride, q, k, out_idx_ptr=None, out_cnt_ptr=None, out_rec_ptr=None,
                       idx_base=0, stream=None):
        _check(lib().dhtgpu_batch_topk_dev(self._h, t_planes_ptr, t_stride, q, k, out_idx_ptr, out_cnt_ptr,
                                           out_rec_ptr, idx_base, stream), "batch_topk_dev")

    def batch_topk_timed(self, t_planes_ptr, t_stride, q, k, out_idx_ptr, out_cnt_ptr, stream=None):
        """One K6 call with HIP events between its kernels; returns (device ms per phase
        (F1 mark targets, F2 filter ids, F3 answer, F4 fallback), fallback targets, survivors,
        targets answered by F3's exact wave path)."""
        ms = (ctypes.c_float * 4)()
        st = (ctypes.c_uint32 * 4)()
        _check(lib().dhtgpu_batch_topk_timed(self._h, t_planes_ptr, t_stride, q, k, out_idx_ptr, out_cnt_ptr,
                                             stream, ms, st), "batch_topk_timed")
        return tuple(ms), int(st[0]), int(st[1]), int(st[2])

    def batch_events(self, events):
        """Arm per-kernel timing of the next K6 call: `events` = 8 torch.cuda.Event(enable_timing=True)
        (F1..F4 start/stop, recorded by the kernels' own dispatches; no synchronisation)."""
        arr = (_vp * 8)(*[e.cuda_event for e in events])
        _check(lib().dhtgpu_batch_events(self._h, arr), "batch_events")

    def tie_words_dev(self, rec_ptr, q, k, idx_base, ties_ptr, tie_cap, row_base, out_words_ptr, stream=None):
        """Words 2..4 of this context's candidates (its own q x k compact records) in the rows a merge
        listed as 64-bit ties (ties_ptr None: every row) -- the second exchange's payload."""
        _check(lib().dhtgpu_tie_words_dev(self._h, rec_ptr, q, k, idx_base, ties_ptr, tie_cap, row_base,
                                          out_words_ptr, stream), "tie_words_dev")

    def topk_dev(self, t_planes_ptr, t_stride, q, k, out_idx_ptr=None, out_cnt_ptr=None, out_rec_ptr=None,
                 idx_base=0, stream=None):
        _check(lib().dhtgpu_topk_dev(self._h, t_planes_ptr, t_stride, q, k, out_idx_ptr, out_cnt_ptr,
                                     out_rec_ptr, idx_base, stream), "topk_dev")

    # ---- K1r: RoutingTable::findClosestNodes -------------------------------------
    def find_closest(self, firsts, bucket_off, node_ids, good, targets, count=8):
        firsts = _ids(firsts, "firsts") if len(firsts) else np.zeros((0, 20), np.uint8)
        off = np.ascontiguousarray(bucket_off, dtype=np.uint32)
        nodes = _ids(node_ids, "node_ids") if len(node_ids) else np.zeros((1, 20), np.uint8)
        good = np.ascontiguousarray(good, dtype=np.uint8) if len(good) else np.zeros(1, np.uint8)
        t = _ids(targets, "targets")
        q = t.shape[0]
        out = np.empty((q, count), dtype=np.uint32)
        cnt = np.empty(q, dtype=np.uint32)
        _check(lib().dhtgpu_find_closest(self._h, firsts.shape[0], _p(firsts, _u8p), _p(off, _u32p),
                                         _p(nodes, _u8p), _p(good, _u8p), _p(t, _u8p), q, count,
                                         _p(out, _u32p), _p(cnt, _u32p)), "find_closest")
        return out, cnt

    # ---- K1w: the resident routing table ------------------------------------------
    def rt_set(self, myid, firsts, bucket_off, node_ids, node_tail=None, af=0, version=0):
        """Upload a table snapshot (the arguments of find_closest) with myid and, optionally, the
        nodes' address || port tails (af 4 / 6); every node starts good.  version != 0 equal to
        the last upload's (same bucket and node counts) skips the upload."""
        my = np.ascontiguousarray(myid, dtype=np.uint8).reshape(20)
        firsts = _ids(firsts, "firsts") if len(firsts) else np.zeros((0, 20), np.uint8)
        off = np.ascontiguousarray(bucket_off, dtype=np.uint32)
        nodes = _ids(node_ids, "node_ids") if len(node_ids) else np.zeros((0, 20), np.uint8)
        tail = None
        if node_tail is not None:
            tail = np.ascontiguousarray(node_tail, dtype=np.uint8).reshape(-1, (4 if af == 4 else 16) + 2)
            if tail.shape[0] != nodes.shape[0]:
                raise ValueError("node_tail must have one row per node")
            if tail.shape[0] == 0:
                tail = np.zeros((1, tail.shape[1]), np.uint8)
        _check(lib().dhtgpu_rt_set(self._h, _p(my, _u8p), firsts.shape[0], _p(firsts, _u8p), _p(off, _u32p),
                                   _p(nodes, _u8p), _p(tail, _u8p) if tail is not None else None, af, int(version)),
               "rt_set")
        self._rt = (nodes.shape[0], 0 if tail is None else tail.shape[1])

    def rt_set_good(self, good):
        """The Node::isGood(now) snapshot: (nn,) bool/uint8, nonzero = good."""
        g = np.ascontiguousarray(np.asarray(good).reshape(-1) != 0, dtype=np.uint8)
        if g.shape[0] != getattr(self, "_rt", (g.shape[0], 0))[0]:
            raise ValueError("good must have one byte per node")
        _check(lib().dhtgpu_rt_set_good(self._h, _p(g, _u8p) if g.size else None), "rt_set_good")

    def rt_update_good(self, idx, val):
        """good[idx[j]] = val[j] (val: array or one value for all)."""
        i = np.ascontiguousarray(idx, dtype=np.uint32).reshape(-1)
        v = np.ascontiguousarray(np.broadcast_to(np.asarray(val), i.shape)).astype(np.uint8).reshape(-1)
        _check(lib().dhtgpu_rt_update_good(self._h, _p(i, _u32p), _p(v, _u8p), i.shape[0]), "rt_update_good")

    def rt_find_closest(self, targets, count=8):
        """find_closest over the resident table: (q, count) indices (NONE padded), (q,) counts."""
        t = _ids(targets, "targets")
        q = t.shape[0]
        out = np.empty((q, count), dtype=np.uint32)
        cnt = np.empty(q, dtype=np.uint32)
        _check(lib().dhtgpu_rt_find_closest(self._h, _p(t, _u8p), q, count, _p(out, _u32p), _p(cnt, _u32p)),
               "rt_find_closest")
        return out, cnt

    def rt_reply(self, targets, indices=False):
        """The find_node reply per target: (q, 8*rec) uint8 blobs (bytes past the length
        unspecified) and (q,) byte lengths; with indices=True also the (q, 8) node indices."""
        t = _ids(targets, "targets")
        q = t.shape[0]
        rec = 20 + getattr(self, "_rt", (0, 6))[1]
        out = np.zeros((q, 8 * rec), dtype=np.uint8)
        ln = np.zeros(q, dtype=np.uint32)
        idx = np.empty((q, 8), dtype=np.uint32) if indices else None
        _check(lib().dhtgpu_rt_reply(self._h, _p(t, _u8p), q, _p(out, _u8p), _p(ln, _u32p),
                                     _p(idx, _u32p) if indices else None), "rt_reply")
        return (out, ln, idx) if indices else (out, ln)

    def rt_closer(self, targets, count=8, min_nodes=1):
        """The closeness test: (q,) uint8 flags -- the count-node result holds >= max(min_nodes, 1)
        nodes and its last node is closer to the target than myid -- and (q,) result sizes."""
        t = _ids(targets, "targets")
        q = t.shape[0]
        flag = np.empty(q, dtype=np.uint8)
        cnt = np.empty(q, dtype=np.uint32)
        _check(lib().dhtgpu_rt_closer(self._h, _p(t, _u8p), q, count, min_nodes, _p(flag, _u8p), _p(cnt, _u32p)),
               "rt_closer")
        return flag, cnt

    def rt_find_closest_dev(self, t_planes_ptr, t_stride, q, count, out_idx_ptr, out_cnt_ptr, stream=None):
        _check(lib().dhtgpu_rt_find_closest_dev(self._h, t_planes_ptr, t_stride, q, count, out_idx_ptr, out_cnt_ptr,
                                                stream), "rt_find_closest_dev")

    def rt_reply_dev(self, t_planes_ptr, t_stride, q, out_ptr, out_len_ptr, out_idx_ptr=None, stream=None):
        _check(lib().dhtgpu_rt_reply_dev(self._h, t_planes_ptr, t_stride, q, out_ptr, out_len_ptr, out_idx_ptr,
                                         stream), "rt_reply_dev")

    def rt_closer_dev(self, t_planes_ptr, t_stride, q, count, min_nodes, out_flag_ptr, out_cnt_ptr=None, stream=None):
        _check(lib().dhtgpu_rt_closer_dev(self._h, t_planes_ptr, t_stride, q, count, min_nodes, out_flag_ptr,
                                          out_cnt_ptr, stream), "rt_closer_dev")

    # ---- K1g: growing the resident table -------------------------------------------
    def rtg_on_new_node(self, ids, handles, state=None, node_tail=None, client=False):
        """RoutingTable::onNewNode for m nodes, in order, on the resident table: ((m,) uint8
        RTG_* results, (m,) uint32 aux -- evicted handle / ping pick / NONE --, (3,) uint32 nb, nn,
        splits).  state (m,): bit 0 good, 1 expired, 2 pending (None: good).  A batch that meets
        the 256-bucket limit raises ERANGE after applying what came before it, as sr_insert does:
        the three arrays are then the exception's `res`, `aux` and `stat`."""
        ids = _ids(ids) if len(ids) else np.zeros((0, 20), np.uint8)
        m = ids.shape[0]
        h = np.ascontiguousarray(handles, dtype=np.uint32).reshape(-1)
        if h.shape[0] != m:
            raise ValueError("handles must have one entry per node")
        s = None
        if state is not None:
            s = np.ascontiguousarray(state, dtype=np.uint8).reshape(-1)
            if s.shape[0] != m:
                raise ValueError("state must have one entry per node")
        t = None
        if node_tail is not None:
            t = np.ascontiguousarray(node_tail, dtype=np.uint8).reshape(m, -1)
            if m and t.shape[1] != getattr(self, "_rt", (0, t.shape[1]))[1]:
                raise ValueError("node_tail rows must be as long as the table's")
        res = np.zeros(m, dtype=np.uint8)
        aux = np.full(m, NONE, dtype=np.uint32)
        stat = np.zeros(3, dtype=np.uint32)
        code = lib().dhtgpu_rtg_on_new_node(self._h, _p(ids, _u8p), _p(h, _u32p), _p(s, _u8p) if s is not None else None,
                                            _p(t, _u8p) if t is not None and m else None, m, int(bool(client)),
                                            _p(res, _u8p), _p(aux, _u32p), _p(stat, _u32p))
        if code != 0:
            e = DhtGpuError(code, "rtg_on_new_node")
            e.res, e.aux, e.stat = res, aux, stat
            raise e
        return res, aux, stat

    def rtg_expire(self):
        """Dht::expireBuckets on the resident table: the removed handles, (r,) uint32, in no particular order."""
        nb, nn = self.rtg_size()
        out = np.zeros(max(nn, 1), dtype=np.uint32)
        r = ctypes.c_uint32(0)
        _check(lib().dhtgpu_rtg_expire(self._h, _p(out, _u32p), ctypes.byref(r)), "rtg_expire")
        return out[: r.value].copy()

    def rtg_set_state(self, state_by_handle):
        """State bytes by handle, (nh,) uint8, for every resident node whose handle is below nh."""
        s = np.ascontiguousarray(state_by_handle, dtype=np.uint8).reshape(-1)
        _check(lib().dhtgpu_rtg_set_state(self._h, _p(s, _u8p) if s.size else None, s.shape[0]), "rtg_set_state")

    def rtg_update_state(self, handles, val):
        """state[handles[j]] = val[j] (val: array or one value for all); handles not resident are ignored."""
        h = np.ascontiguousarray(handles, dtype=np.uint32).reshape(-1)
        v = np.ascontiguousarray(np.broadcast_to(np.asarray(val), h.shape)).astype(np.uint8).reshape(-1)
        _check(lib().dhtgpu_rtg_update_state(self._h, _p(h, _u32p), _p(v, _u8p), h.shape[0]), "rtg_update_state")

    def rtg_size(self):
        """(buckets, nodes) of the resident table."""
        nb, nn = ctypes.c_uint32(0), ctypes.c_uint32(0)
        _check(lib().dhtgpu_rtg_size(self._h, ctypes.byref(nb), ctypes.byref(nn)), "rtg_size")
        return nb.value, nn.value

    def rtg_export(self):
        """The resident table: firsts (nb, 20), bucket_off (nb + 1,), ids (nn, 20), handles (nn,),
        state (nn,) -- bucket list order, in-bucket list order."""
        nb, nn = self.rtg_size()
        firsts = np.zeros((nb, 20), dtype=np.uint8)
        off = np.zeros(nb + 1, dtype=np.uint32)
        ids = np.zeros((max(nn, 1), 20), dtype=np.uint8)
        h = np.zeros(max(nn, 1), dtype=np.uint32)
        st = np.zeros(max(nn, 1), dtype=np.uint8)
        _check(lib().dhtgpu_rtg_export(self._h, _p(firsts, _u8p) if nb else None, _p(off, _u32p), _p(ids, _u8p),
                                       _p(h, _u32p), _p(st, _u8p)), "rtg_export")
        return firsts, off, ids[:nn], h[:nn], st[:nn]

    # ---- K8w: the resident NodeCache ------------------------------------------------
    def nc_set(self, ids, handles=None):
        """Replace the mirror with (n, 20) keys in any order; handles (n,) uint32 (None: key i has
        handle i).  Every handle starts accepted."""
        ids = _ids(ids) if len(ids) else np.zeros((0, 20), np.uint8)
        h = None
        if handles is not None:
            h = np.ascontiguousarray(handles, dtype=np.uint32).reshape(-1)
            if h.shape[0] != ids.shape[0]:
                raise ValueError("handles must have one entry per key")
        _check(lib().dhtgpu_nc_set(self._h, _p(ids, _u8p), _p(h, _u32p) if h is not None else None, ids.shape[0]),
               "nc_set")

    def nc_insert(self, ids, handles, accept=None):
        """std::map::emplace for m keys: (m,) uint8, 1 where the key was inserted (else it was
        present, or an earlier key of the batch equals it).  accept (m,) sets the new keys' bits."""
        ids = _ids(ids) if len(ids) else np.zeros((0, 20), np.uint8)
        h = np.ascontiguousarray(handles, dtype=np.uint32).reshape(-1)
        if h.shape[0] != ids.shape[0]:
            raise ValueError("handles must have one entry per key")
        a = None
        if accept is not None:
            a = np.ascontiguousarray(np.asarray(accept).reshape(-1) != 0, dtype=np.uint8)
            if a.shape[0] != ids.shape[0]:
                raise ValueError("accept must have one entry per key")
        new = np.zeros(ids.shape[0], dtype=np.uint8)
        _check(lib().dhtgpu_nc_insert(self._h, _p(ids, _u8p), _p(h, _u32p), _p(a, _u8p) if a is not None else None,
                                      ids.shape[0], _p(new, _u8p)), "nc_insert")
        return new

    def nc_erase(self, ids):
        """map.erase(key) for m keys: (m,) uint8, 1 where the key was erased."""
        ids = _ids(ids) if len(ids) else np.zeros((0, 20), np.uint8)
        found = np.zeros(ids.shape[0], dtype=np.uint8)
        _check(lib().dhtgpu_nc_erase(self._h, _p(ids, _u8p), ids.shape[0], _p(found, _u8p)), "nc_erase")
        return found

    def nc_update_accept(self, handles, val):
        """accept bit of handles[j] = val[j] (val: array or one value for all); stream-ordered."""
        h = np.ascontiguousarray(handles, dtype=np.uint32).reshape(-1)
        v = np.ascontiguousarray(np.broadcast_to(np.asarray(val), h.shape)).astype(np.uint8).reshape(-1)
        _check(lib().dhtgpu_nc_update_accept(self._h, _p(h, _u32p), _p(v, _u8p), h.shape[0]), "nc_update_accept")

    def nc_set_accept(self, accept_by_handle):
        """accept bit of handle h = accept_by_handle[h] for h < len; stream-ordered."""
        a = np.ascontiguousarray(np.asarray(accept_by_handle).reshape(-1) != 0, dtype=np.uint8)
        _check(lib().dhtgpu_nc_set_accept(self._h, _p(a, _u8p) if a.size else None, a.shape[0]), "nc_set_accept")

    def nc_size(self):
        n = ctypes.c_uint64(0)
        _check(lib().dhtgpu_nc_size(self._h, ctypes.byref(n)), "nc_size")
        return int(n.value)

    def nc_export(self):
        """The mirror in lexicographic order: (n, 20) keys, (n,) handles."""
        n = self.nc_size()
        ids = np.zeros((n, 20), dtype=np.uint8)
        h = np.zeros(n, dtype=np.uint32)
        _check(lib().dhtgpu_nc_export(self._h, _p(ids, _u8p), _p(h, _u32p)), "nc_export")
        return ids, h

    def nc_nodes(self, targets, count=8):
        """getCachedNodes over the mirror: (q, count) handles in walk order (NONE padded), (q,) counts."""
        t = _ids(targets, "targets") if len(targets) else np.zeros((0, 20), np.uint8)
        q = t.shape[0]
        out = np.empty((q, count), dtype=np.uint32)
        cnt = np.empty(q, dtype=np.uint32)
        _check(lib().dhtgpu_nc_nodes(self._h, _p(t, _u8p), q, count, _p(out, _u32p), _p(cnt, _u32p)), "nc_nodes")
        return out, cnt

    def nc_nodes_dev(self, t_planes_ptr, t_stride, q, count, out_handle_ptr, out_cnt_ptr, stream=None):
        _check(lib().dhtgpu_nc_nodes_dev(self._h, t_planes_ptr, t_stride, q, count, out_handle_ptr, out_cnt_ptr,
                                         stream), "nc_nodes_dev")

    # ---- K8r: keys to handles over the resident NodeCache ---------------------------
    def ncr_find(self, ids, accept=False):
        """NodeMap::find for m keys (any order, repeats allowed): (m,) uint32 handles, NONE where the
        mirror does not hold the key; with accept=True also (m,) uint8, the handles' accept bits."""
        ids = _ids(ids) if len(ids) else np.zeros((0, 20), np.uint8)
        m = ids.shape[0]
        h = np.full(m, 0xFFFFFFFF, dtype=np.uint32)
        a = np.zeros(m, dtype=np.uint8) if accept else None
        _check(lib().dhtgpu_ncr_find(self._h, _p(ids, _u8p), m, _p(h, _u32p), _p(a, _u8p) if accept else None),
               "ncr_find")
        return (h, a) if accept else h

    def ncr_find_dev(self, id_planes_ptr, id_stride, m, out_handle_ptr, out_accept_ptr=None, stream=None):
        _check(lib().dhtgpu_ncr_find_dev(self._h, id_planes_ptr, id_stride, m, out_handle_ptr, out_accept_ptr, stream),
               "ncr_find_dev")

    def ncr_get_nodes(self, ids, free_handles, accept=None):
        """NodeMap::getNode's emplace for m keys in batch order, absent keys under free_handles in
        order: (m,) uint32 handles, (m,) uint8 new bytes, the number of free handles used.  Too few
        free handles: DhtGpuError (ERANGE) with .needed set, nothing applied."""
        ids = _ids(ids) if len(ids) else np.zeros((0, 20), np.uint8)
        m = ids.shape[0]
        f = np.ascontiguousarray(free_handles, dtype=np.uint32).reshape(-1)
        a = None
        if accept is not None:
            a = np.ascontiguousarray(np.asarray(accept).reshape(-1) != 0, dtype=np.uint8)
            if a.shape[0] != m:
                raise ValueError("accept must have one entry per key")
        h = np.full(m, 0xFFFFFFFF, dtype=np.uint32)
        new = np.zeros(m, dtype=np.uint8)
        used = ctypes.c_uint32(0)
        code = lib().dhtgpu_ncr_get_nodes(self._h, _p(ids, _u8p), m, _p(f, _u32p) if f.size else None, f.shape[0],
                                          _p(a, _u8p) if a is not None else None, _p(h, _u32p), _p(new, _u8p),
                                          ctypes.byref(used))
        if code:
            err = DhtGpuError(code, "ncr_get_nodes")
            err.needed = int(used.value)
            raise err
        return h, new, int(used.value)

    def ncr_extract(self, ids):
        """map.erase(key) for m keys: (m,) uint32, the handle each erased key held (NONE: absent, or a
        repeat of an earlier key of the batch)."""
        ids = _ids(ids) if len(ids) else np.zeros((0, 20), np.uint8)
        h = np.full(ids.shape[0], 0xFFFFFFFF, dtype=np.uint32)
        _check(lib().dhtgpu_ncr_extract(self._h, _p(ids, _u8p), ids.shape[0], _p(h, _u32p)), "ncr_extract")
        return h

    # ---- K10w: the resident searches ------------------------------------------------
    @staticmethod
    def _u32(a):
        return np.ascontiguousarray(a, dtype=np.uint32).reshape(-1)

    def sr_reset(self, nslots):
        """nslots empty searches; drops any earlier set and the state array."""
        _check(lib().dhtgpu_sr_reset(self._h, nslots), "sr_reset")
        self._sr_nslots = int(nslots)

    def sr_open(self, slots, targets):
        """A new Search (target, empty list, not expired) in each listed slot; stream-ordered."""
        s = self._u32(slots)
        t = _ids(targets, "targets") if len(targets) else np.zeros((0, 20), np.uint8)
        if t.shape[0] != s.shape[0]:
            raise ValueError("targets must have one row per slot")
        _check(lib().dhtgpu_sr_open(self._h, _p(s, _u32p), _p(t, _u8p), s.shape[0]), "sr_open")

    def sr_expire(self, slots):
        """Search::expire(): expired = 1 and the list cleared; stream-ordered."""
        s = self._u32(slots)
        _check(lib().dhtgpu_sr_expire(self._h, _p(s, _u32p), s.shape[0]), "sr_expire")

    def sr_set_state(self, state_by_handle):
        """node state byte (bit0 isExpired, bit1 isRemovable) of handle h = state_by_handle[h]; replaces the array."""
        a = np.ascontiguousarray(state_by_handle, dtype=np.uint8).reshape(-1)
        _check(lib().dhtgpu_sr_set_state(self._h, _p(a, _u8p) if a.size else None, a.shape[0]), "sr_set_state")

    def sr_update_state(self, handles, val):
        """state byte of handles[j] = val[j] (val: array or one value for all); grows the array."""
        h = self._u32(handles)
        v = np.ascontiguousarray(np.broadcast_to(np.asarray(val), h.shape)).astype(np.uint8).reshape(-1)
        _check(lib().dhtgpu_sr_update_state(self._h, _p(h, _u32p), _p(v, _u8p), h.shape[0]), "sr_update_state")

    def sr_set_candidate(self, slots, handles, val):
        """candidate flag of handles[j]'s entry in slots[j] = val[j]; an absent handle changes nothing."""
        s, h = self._u32(slots), self._u32(handles)
        if s.shape[0] != h.shape[0]:
            raise ValueError("one handle per slot")
        v = np.ascontiguousarray(np.broadcast_to(np.asarray(val), h.shape)).astype(np.uint8).reshape(-1)
        _check(lib().dhtgpu_sr_set_candidate(self._h, _p(s, _u32p), _p(h, _u32p), _p(v, _u8p), s.shape[0]),
               "sr_set_candidate")

    def sr_insert(self, slots, ins_off, ins_handle, ins_ids, ins_token=None):
        """Search::insertNode: slots[j] takes insertions [ins_off[j], ins_off[j+1]) in order.  Returns
        the (total,) uint8 insertNode results; raises ERANGE (after applying everything else) when a
        list overflowed -- the results are then in the exception's `added`."""
        s = self._u32(slots)
        off = np.ascontiguousarray(ins_off, dtype=np.uint64).reshape(-1)
        if off.shape[0] != s.shape[0] + 1:
            raise ValueError("ins_off must have len(slots) + 1 entries")
        h = self._u32(ins_handle)
        ids = _ids(ins_ids) if len(ins_ids) else np.zeros((0, 20), np.uint8)
        tot = int(off[-1])
        if h.shape[0] < tot or ids.shape[0] < tot:
            raise ValueError("ins_handle / ins_ids shorter than ins_off[-1]")
        tok = None if ins_token is None else np.ascontiguousarray(ins_token, dtype=np.uint8).reshape(-1)
        if tok is not None and tok.shape[0] < tot:
            raise ValueError("ins_token shorter than ins_off[-1]")
        added = np.zeros(tot, dtype=np.uint8)
        code = lib().dhtgpu_sr_insert(self._h, _p(s, _u32p), s.shape[0], _p(off, _u64p), _p(h, _u32p), _p(ids, _u8p),
                                      _p(tok, _u8p) if tok is not None else None, _p(added, _u8p))
        if code != 0:
            e = DhtGpuError(code, "sr_insert")
            e.added = added
            raise e
        return added

    def sr_refill(self, slots, count=14):
        """Dht::refill per slot over the nc mirror: (m,) uint32 inserted counts; ERANGE as sr_insert
        (the counts in the exception's `inserted`)."""
        s = self._u32(slots)
        out = np.zeros(s.shape[0], dtype=np.uint32)
        code = lib().dhtgpu_sr_refill(self._h, _p(s, _u32p), s.shape[0], count, _p(out, _u32p))
        if code != 0:
            e = DhtGpuError(code, "sr_refill")
            e.inserted = out
            raise e
        return out

    def sr_status(self, slots):
        """(m, 4) uint32: len, bad nodes, leading bad nodes, bits (bit0 expired, bit1 overflowed)."""
        s = self._u32(slots)
        out = np.zeros((s.shape[0], 4), dtype=np.uint32)
        _check(lib().dhtgpu_sr_status(self._h, _p(s, _u32p), s.shape[0], _p(out, _u32p)), "sr_status")
        return out

    def sr_lists(self, slots):
        """The rows closest first: (m, 64) handles (NONE padded), (m, 64) flags, (m,) lengths."""
        s = self._u32(slots)
        m = s.shape[0]
        h = np.full((m, SR_CAP), NONE, dtype=np.uint32)
        fl = np.zeros((m, SR_CAP), dtype=np.uint8)
        ln = np.zeros(m, dtype=np.uint32)
        _check(lib().dhtgpu_sr_lists(self._h, _p(s, _u32p), m, _p(h, _u32p), _p(fl, _u8p), _p(ln, _u32p)), "sr_lists")
        return h, fl, ln

    def sr_insert_dev(self, slots_ptr, m, ins_off_ptr, ins_handle_ptr, id_planes_ptr, id_stride, ins_token_ptr,
                      ins_added_ptr, stream=None):
        _check(lib().dhtgpu_sr_insert_dev(self._h, slots_ptr, m, ins_off_ptr, ins_handle_ptr, id_planes_ptr, id_stride,
                                          ins_token_ptr, ins_added_ptr, stream), "sr_insert_dev")

    def sr_refill_dev(self, slots_ptr, m, count, out_inserted_ptr, stream=None):
        _check(lib().dhtgpu_sr_refill_dev(self._h, slots_ptr, m, count, out_inserted_ptr, stream), "sr_refill_dev")

    def sr_status_dev(self, slots_ptr, m, out4_ptr, stream=None):
        _check(lib().dhtgpu_sr_status_dev(self._h, slots_ptr, m, out4_ptr, stream), "sr_status_dev")

    def sr_lists_dev(self, slots_ptr, m, out_handle_ptr, out_flags_ptr=None, out_len_ptr=None, stream=None):
        _check(lib().dhtgpu_sr_lists_dev(self._h, slots_ptr, m, out_handle_ptr, out_flags_ptr, out_len_ptr, stream),
               "sr_lists_dev")

    # ---- K10s: Dht::searchStep on the resident searches -----------------------------------
    def srs_set_clock(self, now):
        """scheduler.time() in the caller's ticks (> 0): what token insertions, refills and steps read."""
        _check(lib().dhtgpu_srs_set_clock(self._h, int(now)), "srs_set_clock")

    def srs_set_request(self, slots, handles, val):
        """req (0 none, 1 pending, 2 completed) of handles[j]'s entry in slots[j] = val[j]; an absent
        handle changes nothing."""
        s, h = self._u32(slots), self._u32(handles)
        if s.shape[0] != h.shape[0]:
            raise ValueError("one handle per slot")
        v = np.ascontiguousarray(np.broadcast_to(np.asarray(val), h.shape)).astype(np.uint8).reshape(-1)
        _check(lib().dhtgpu_srs_set_request(self._h, _p(s, _u32p), _p(h, _u32p), _p(v, _u8p), s.shape[0]),
               "srs_set_request")

    def srs_step(self, slots, node_expire, refill_count=14):
        """Dht::searchStep per slot: ((m, 64) handles to send find_node to, NONE padded; (m, 4) uint32
        sends, pending non-bad entries after, refill's inserted count, bits).  Raises ERANGE (after
        applying everything) when a refill overflowed a row -- the results in the exception's `result`."""
        s = self._u32(slots)
        m = s.shape[0]
        send = np.full((m, SR_CAP), NONE, dtype=np.uint32)
        out4 = np.zeros((m, 4), dtype=np.uint32)
        code = lib().dhtgpu_srs_step(self._h, _p(s, _u32p), m, node_expire, refill_count, _p(send, _u32p), _p(out4, _u32p))
        if code != 0:
            e = DhtGpuError(code, "srs_step")
            e.result = (send, out4)
            raise e
        return send, out4

    def srs_entries(self, slots):
        """The rows' request state and ticks: (m, 64) uint8 req, (m, 64) uint32 tick, 0 past a row's end."""
        s = self._u32(slots)
        m = s.shape[0]
        req = np.zeros((m, SR_CAP), dtype=np.uint8)
        tick = np.zeros((m, SR_CAP), dtype=np.uint32)
        _check(lib().dhtgpu_srs_entries(self._h, _p(s, _u32p), m, _p(req, _u8p), _p(tick, _u32p)), "srs_entries")
        return req, tick

    def srs_step_dev(self, slots_ptr, m, node_expire, refill_count, out_send_ptr, out4_ptr, stream=None):
        _check(lib().dhtgpu_srs_step_dev(self._h, slots_ptr, m, node_expire, refill_count, out_send_ptr, out4_ptr, stream),
               "srs_step_dev")

    def srs_entries_dev(self, slots_ptr, m, out_req_ptr, out_tick_ptr, stream=None):
        _check(lib().dhtgpu_srs_entries_dev(self._h, slots_ptr, m, out_req_ptr, out_tick_ptr, stream), "srs_entries_dev")

    # ---- K10m: Dht::trySearchInsert over the searches' ordered map -----------------------
    def srm_set(self, slots):
        """The searches' map = these slots (any order), sorted by target on the device; EUNSORTED on
        equal targets, EINVAL on a repeated or unknown slot."""
        s = self._u32(slots)
        _check(lib().dhtgpu_srm_set(self._h, _p(s, _u32p) if s.size else None, s.shape[0]), "srm_set")

    def srm_set_done(self, slots, val):
        """Search::done of slots[j] = val[j] (array or one value for all); stream-ordered."""
        s = self._u32(slots)
        v = np.ascontiguousarray(np.broadcast_to(np.asarray(val), s.shape)).astype(np.uint8).reshape(-1)
        _check(lib().dhtgpu_srm_set_done(self._h, _p(s, _u32p), _p(v, _u8p), s.shape[0]), "srm_set_done")

    def srm_offer(self, handles, ids):
        """Dht::trySearchInsert for the nodes in order.  Returns (cnt, touched, stats): (m,) uint32
        searches that took each node, the (ceil(nslots / 32),) uint32 bitmask of the slots that took
        one, and {filtered, walk insertNode calls, hazard, overflow}; raises ERANGE (after applying
        everything) when a row overflowed -- the three results are then in the exception's `result`."""
        h = self._u32(handles)
        m = h.shape[0]
        k = _ids(ids) if m else np.zeros((0, 20), np.uint8)
        if k.shape[0] != m:
            raise ValueError("one id per handle")
        cnt = np.zeros(m, dtype=np.uint32)
        touched = np.zeros((getattr(self, "_sr_nslots", 0) + 31) // 32, dtype=np.uint32)
        stats = np.zeros(4, dtype=np.uint32)
        code = lib().dhtgpu_srm_offer(self._h, _p(h, _u32p), _p(k, _u8p), m, _p(cnt, _u32p),
                                      _p(touched, _u32p) if touched.size else None, _p(stats, _u32p))
        if code != 0:
            e = DhtGpuError(code, "srm_offer")
            e.result = (cnt, touched, stats)
            raise e
        return cnt, touched, stats

    def srm_offer_dev(self, handles_ptr, id_planes_ptr, id_stride, m, out_cnt_ptr, out_touched_ptr=None,
                      out_stats_ptr=None, stream=None):
        _check(lib().dhtgpu_srm_offer_dev(self._h, handles_ptr, id_planes_ptr, id_stride, m, out_cnt_ptr, out_touched_ptr,
                                          out_stats_ptr, stream), "srm_offer_dev")

    def srm_export(self):
        """The map in target order: (ns,) uint32 slots and (ns,) uint8 done bits."""
        ns = ctypes.c_uint32(0)
        _check(lib().dhtgpu_srm_export(self._h, None, None, ctypes.byref(ns)), "srm_export")
        slots = np.zeros(ns.value, dtype=np.uint32)
        done = np.zeros(ns.value, dtype=np.uint8)
        if ns.value:
            _check(lib().dhtgpu_srm_export(self._h, _p(slots, _u32p), _p(done, _u8p), ctypes.byref(ns)), "srm_export")
        return slots, done

    # ---- a11 / f4: compact node wire format ---------------------------------------
    def buffer_nodes(self, node_tail, af, targets, cand):
        """NetworkEngine::bufferNodes, batched: (q, 8*rec) uint8 blobs and (q,) byte lengths."""
        t = _ids(targets, "targets")
        q = t.shape[0]
        cand = np.ascontiguousarray(cand, dtype=np.uint32).reshape(q, -1)
        alen = 4 if af == 4 else 16
        tail = np.ascontiguousarray(node_tail, dtype=np.uint8).reshape(-1, alen + 2)
        rec = 20 + alen + 2
        out = np.zeros((q, 8 * rec), dtype=np.uint8)
        ln = np.zeros(q, dtype=np.uint32)
        _check(lib().dhtgpu_buffer_nodes(self._h, _p(tail, _u8p), af, _p(t, _u8p), q, _p(cand, _u32p),
                                         cand.shape[1], _p(out, _u8p), _p(ln, _u32p)), "buffer_nodes")
        return out, ln

    def deserialize_nodes(self, af, myid, blobs, from_af, from_addr):
        """NetworkEngine::deserializeNodes over a list of received blobs: returns
        (ids (r,20), tails (r, alen+2), status (r,), msg_status (m,))."""
        alen = 4 if af == 4 else 16
        m = len(blobs)
        off = np.zeros(m + 1, dtype=np.uint64)
        for i, b in enumerate(blobs):
            off[i + 1] = off[i] + len(b)
        blob = np.frombuffer(b"".join(bytes(b) for b in blobs) or b"\0", dtype=np.uint8).copy()
        fa = np.ascontiguousarray(from_af, dtype=np.uint8).reshape(m) if m else np.zeros(1, np.uint8)
        fad = np.ascontiguousarray(from_addr, dtype=np.uint8).reshape(m, 16) if m else np.zeros((1, 16), np.uint8)
        cap = max(1, int(off[-1]) // (20 + alen + 2))
        ids = np.zeros((cap, 20), np.uint8)
        tail = np.zeros((cap, alen + 2), np.uint8)
        st = np.zeros(cap, np.uint8)
        ms = np.zeros(max(m, 1), np.uint8)
        nrec = ctypes.c_uint32()
        my = np.ascontiguousarray(myid, dtype=np.uint8).reshape(20)
        _check(lib().dhtgpu_deserialize_nodes(self._h, af, _p(my, _u8p), _p(blob, _u8p), _p(off, _u64p), m,
                                              _p(fa, _u8p), _p(fad, _u8p), _p(ids, _u8p), _p(tail, _u8p),
                                              _p(st, _u8p), _p(ms, _u8p), ctypes.byref(nrec)), "deserialize_nodes")
        r = nrec.value
        return ids[:r], tail[:r], st[:r], ms[:m]

    # ---- f3: crawl replay ------------------------------------------------------------
    def net_prepare(self, dead=None, table_seed=0x5EED):
        """Turn the uploaded id set into the crawl-model network (dead: (n,) bool/uint8)."""
        d = None
        if dead is not None:
            d = np.ascontiguousarray(dead, dtype=np.uint8)
            if d.shape[0] != self.num_ids:
                raise ValueError("dead mask must have one byte per id")
        _check(lib().dhtgpu_net_prepare(self._h, _p(d, _u8p) if d is not None else None, table_seed), "net_prepare")

    def set_search_alpha(self, alpha):
        """Requests per search round for later search_batch calls (default 4 =
        MAX_REQUESTED_SEARCH_NODES, include/opendht/dht.h:321)."""
        _check(lib().dhtgpu_set_search_alpha(self._h, int(alpha)), "set_search_alpha")
        self._alpha = int(alpha)

    def search_batch(self, targets, searchers, max_rounds=64, alpha=None):
        """Iterative searches: (idx (q,64), flags (q,64), len (q,), rounds (q,), queries (q,)).
        alpha (optional): requests per round for THIS call only (the context's setting,
        set_search_alpha, default 4 = MAX_REQUESTED_SEARCH_NODES, is restored afterwards)."""
        t = _ids(targets, "targets")
        q = t.shape[0]
        sr = np.ascontiguousarray(searchers, dtype=np.uint32).reshape(q)
        idx = np.empty((q, 64), np.uint32)
        fl = np.empty((q, 64), np.uint8)
        ln, rd, qs = (np.empty(q, np.uint32) for _ in range(3))
        saved = getattr(self, "_alpha", 4)
        if alpha is not None:
            _check(lib().dhtgpu_set_search_alpha(self._h, int(alpha)), "set_search_alpha")
        try:
            _check(lib().dhtgpu_search_batch(self._h, _p(t, _u8p), q, _p(sr, _u32p), max_rounds, _p(idx, _u32p),
                                             _p(fl, _u8p), _p(ln, _u32p), _p(rd, _u32p), _p(qs, _u32p)),
                   "search_batch")
        finally:
            if alpha is not None:
                _check(lib().dhtgpu_set_search_alpha(self._h, int(saved)), "set_search_alpha")
        return idx, fl, ln, rd, qs

    # ---- K2: classification -------------------------------------------------------
    def classify(self, firsts, myid, buckets=True):
        firsts = _ids(firsts, "firsts")
        myid = np.ascontiguousarray(myid, dtype=np.uint8).reshape(20)
        hist = np.zeros(161, dtype=np.uint64)
        out = np.empty(max(self.num_ids, 1), dtype=np.uint8) if buckets else None
        _check(lib().dhtgpu_classify(self._h, firsts.shape[0], _p(firsts, _u8p), _p(myid, _u8p),
                                     _p(out, _u8p) if buckets else None, _p(hist, _u64p)), "classify")
        return (out[: self.num_ids] if buckets else None), hist

    # ---- a8: NodeCache::getCachedNodes ------------------------------------------------
    def cached_nodes(self, targets, count=14, accept=None):
        t = _ids(targets, "targets")
        q = t.shape[0]
        out = np.empty((q, count), dtype=np.uint32)
        cnt = np.empty(q, dtype=np.uint32)
        acc = None
        if accept is not None:
            acc = np.ascontiguousarray(accept, dtype=np.uint8)
            if acc.shape[0] != self.num_ids:
                raise ValueError("accept mask must have one byte per id")
        _check(lib().dhtgpu_cached_nodes(self._h, _p(acc, _u8p) if acc is not None else None, _p(t, _u8p), q,
                                         count, _p(out, _u32p), _p(cnt, _u32p)), "cached_nodes")
        return out, cnt


    # ---- f2: the NodeCache mirror (a second id set, sorted on the device) ----------------
    def cache_set(self, ids, version=0):
        """Upload NodeCache map keys in any order (unique); version != 0 equal to the last
        upload's skips the upload."""
        ids = _ids(ids)
        _check(lib().dhtgpu_cache_set(self._h, _p(ids, _u8p), ids.shape[0], int(version)), "cache_set")
        self._cache_n = ids.shape[0]

    def cache_nodes(self, targets, count=14, accept=None):
        """getCachedNodes over the mirror: (q, count) caller-order indices (NONE padded), (q,) counts."""
        t = _ids(targets, "targets")
        q = t.shape[0]
        out = np.empty((q, count), dtype=np.uint32)
        cnt = np.empty(q, dtype=np.uint32)
        acc = None
        if accept is not None:
            acc = np.ascontiguousarray(accept, dtype=np.uint8)
            if acc.shape[0] != getattr(self, "_cache_n", acc.shape[0]):
                raise ValueError("accept mask must have one byte per cache key")
        _check(lib().dhtgpu_cache_nodes(self._h, _p(acc, _u8p) if acc is not None else None, _p(t, _u8p), q, count,
                                        _p(out, _u32p), _p(cnt, _u32p)), "cache_nodes")
        return out, cnt

    def cache_sorted(self):
        """The mirror's lexicographic order as caller indices."""
        perm = np.empty(max(getattr(self, "_cache_n", 0), 1), dtype=np.uint32)
        _check(lib().dhtgpu_cache_sorted(self._h, _p(perm, _u32p)), "cache_sorted")
        return perm[: getattr(self, "_cache_n", 0)]

    def buffer_nodes_ids(self, node_ids, node_tail, af, targets, cand):
        """bufferNodes over the caller's own nodes (the context's id set is not used)."""
        t = _ids(targets, "targets")
        q = t.shape[0]
        nodes = _ids(node_ids, "node_ids")
        cand = np.ascontiguousarray(cand, dtype=np.uint32).reshape(q, -1)
        alen = 4 if af == 4 else 16
        tail = np.ascontiguousarray(node_tail, dtype=np.uint8).reshape(-1, alen + 2)
        rec = 20 + alen + 2
        out = np.zeros((q, 8 * rec), dtype=np.uint8)
        ln = np.zeros(q, dtype=np.uint32)
        _check(lib().dhtgpu_buffer_nodes_ids(self._h, _p(nodes, _u8p), _p(tail, _u8p), nodes.shape[0], af,
                                             _p(t, _u8p), q, _p(cand, _u32p), cand.shape[1], _p(out, _u8p),
                                             _p(ln, _u32p)), "buffer_nodes_ids")
        return out, ln


    # ---- a10: Search::insertNode, batched -----------------------------------------------------
    def search_insert(self, node_ids, node_state, targets, lists, flags, lens, expired, ins_off, ins_node,
                      ins_token):
        """Apply insertions (CSR ins_off over searches) to the search lists in place-copies:
        returns (lists, flags, lens, expired, added)."""
        nodes = _ids(node_ids, "node_ids")
        st = np.ascontiguousarray(node_state, dtype=np.uint8)
        t = _ids(targets, "targets")
        q = t.shape[0]
        lists = np.ascontiguousarray(lists, dtype=np.uint32).copy()
        cap = lists.shape[1]
        flags = np.ascontiguousarray(flags, dtype=np.uint8).copy()
        lens = np.ascontiguousarray(lens, dtype=np.uint32).copy()
        expired = np.ascontiguousarray(expired, dtype=np.uint8).copy()
        off = np.ascontiguousarray(ins_off, dtype=np.uint64)
        node = np.ascontiguousarray(ins_node, dtype=np.uint32)
        tok = np.ascontiguousarray(ins_token, dtype=np.uint8)
        added = np.zeros(max(node.size, 1), np.uint8)
        _check(lib().dhtgpu_search_insert(self._h, _p(nodes, _u8p), _p(st, _u8p), nodes.shape[0], _p(t, _u8p), q, cap,
                                          _p(lists, _u32p), _p(flags, _u8p), _p(lens, _u32p), _p(expired, _u8p),
                                          _p(off, _u64p), _p(node, _u32p) if node.size else None,
                                          _p(tok, _u8p) if tok.size else None, _p(added, _u8p)), "search_insert")
        return lists, flags, lens, expired, added[: node.size]

    def table_stats(self, firsts):
        """(lowbit, depth) of every bucket of a table snapshot, computed on the device."""
        f = _ids(firsts, "firsts")
        nb = f.shape[0]
        lb = np.zeros(max(nb, 1), np.int32)
        dp = np.zeros(max(nb, 1), np.uint32)
        _check(lib().dhtgpu_table_stats(self._h, nb, _p(f, _u8p), lb.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)),
                                        _p(dp, _u32p)), "table_stats")
        return lb[:nb], dp[:nb]


def table_depth(firsts, b):
    """RoutingTable::depth of bucket b of a table snapshot (src/routing_table.cpp:100-107)."""
    f = _ids(firsts, "firsts") if len(firsts) else np.zeros((0, 20), np.uint8)
    d = ctypes.c_uint32()
    _check(lib().dhtgpu_table_depth(f.shape[0], _p(f, _u8p), b, ctypes.byref(d)), "table_depth")
    return d.value


PLAN_FIELDS = ("route", "Lm", "Lmin", "b1", "Lq", "tcap", "scap", "nsets", "f3_stage", "f2_mode", "f2_stage",
               "per_blk", "nblk2", "f1_two_pass", "Ls")
ROUTE_KS, ROUTE_K6, ROUTE_SUBS, ROUTE_REFUSED = 0, 1, 2, 3
F2_DENSE, F2_SPARSE, F2_SEG, F2_NARROW = 0, 1, 3, 4


def batch_plan(n, q, k, ctx=None, num_cus=256):
    """The plan a batch_topk call of q targets at k over n ids runs with (host only, no device
    work): a dict of PLAN_FIELDS (include/dhtgpu.h, dhtgpu_batch_plan).  ctx: a Context, whose
    device's CU count is used; else num_cus.  Fields past `route` are defined for ROUTE_K6 (Ls for
    ROUTE_KS) and 0 otherwise."""
    out = (ctypes.c_uint32 * 16)()
    _check(lib().dhtgpu_batch_plan(ctx._h if ctx is not None else None, int(num_cus), int(n), int(q), int(k), out),
           "batch_plan")
    return {name: int(out[i]) for i, name in enumerate(PLAN_FIELDS)}


def device_count():
    n = ctypes.c_int()
    _check(lib().dhtgpu_device_count(ctypes.byref(n)), "device_count")
    return n.value
