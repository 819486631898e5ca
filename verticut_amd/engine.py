"""ctypes binding of include/verticut_gpu.h -- the only way Python reaches the kernels.

There is no Python or CPU implementation of any search here: if libverticut_gpu.so is missing
or no gfx950 device is usable, construction raises.
"""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("VERTICUT_GPU_LIB") or os.path.join(_HERE, "lib", "libverticut_gpu.so")   # env: A/B builds

VC_ABI_VERSION = 2
VC_OK, VC_NOT_FOUND = 0, 1
VC_ERR_INVALID, VC_ERR_NO_DEVICE, VC_ERR_HIP, VC_ERR_NOMEM, VC_ERR_STATE, VC_ERR_CAPACITY = -1, -2, -3, -4, -5, -6
MODE_LINEAR, MODE_MIH_EXACT, MODE_MIH_APPROX = 0, 1, 2
FLAG_USE_BITMAP, FLAG_REF_SIGNEXT_KEYS, FLAG_REF_STOP_LITERAL4, FLAG_LEAN_TIMING = 1, 2, 4, 8
FLAG_GLOBAL_STOP = 0x10   # sharded store, exact MIH: stop where one engine over the union stops (same rows and statistics)
FLAG_GLOBAL_APPROX = 0x20 # sharded store, approximate MIH: stop where one engine over the union stops (same rows and statistics)
SYNTH_UNIFORM, SYNTH_CLUSTERED = 0, 1
ORDER_ASCENDING, ORDER_FARTHEST_FIRST = 0, 1
IDS_EXCLUDE_SELF = 0x1    # VC_IDS_EXCLUDE_SELF: a by-id row holds the k nearest items other than the query's own record
IDS_ONLY_GREATER = 0x2    # VC_IDS_ONLY_GREATER (radius-by-id calls only): a segment keeps the entries whose id exceeds the query's own
LEADER_ROUND_GROUP = 4            # VC_LEADER_ROUND_GROUP (vc_internal.hpp): decision rounds between two read-backs of the undecided counter
RETAIN_MASK, RETAIN_ROOTS = 0, 1   # VC_RETAIN_MASK: record i survives iff sel[i] != 0; VC_RETAIN_ROOTS: iff sel[i] == id_base + i (cluster labels)
PACK_INF = np.uint64(0xFFFFFFFFFFFFFFFF)
STREAM_OWN = C.c_void_p(-1)   # VC_STREAM_OWN; None / 0 = the HIP null stream (PyTorch's default stream)

# every symbol include/verticut_gpu.h declares (tests check the .so exports exactly these)
EXPORTS = [
    "vc_create", "vc_destroy", "vc_last_error", "vc_strerror", "vc_abi_version", "vc_add_codes", "vc_add_synthetic",
    "vc_size", "vc_get_code", "vc_build_index", "vc_get_bucket", "vc_bitmap_test", "vc_bitmap_read", "vc_search_knn",
    "vc_search_knn_dev", "vc_search_radius", "vc_merge_topk_dev", "vc_get_timing", "vc_set_stream",
    "vc_load_code_file", "vc_save_code_file", "vc_write_bitmap_file", "vc_device_status",
    "vc_search_radius_dev", "vc_read_bitmap_file", "vc_save_index", "vc_load_index",
    "vc_sharded_create", "vc_sharded_destroy", "vc_sharded_last_error", "vc_sharded_exchange", "vc_sharded_add_codes",
    "vc_sharded_add_synthetic", "vc_sharded_size", "vc_sharded_build_index", "vc_sharded_get_code", "vc_sharded_get_bucket",
    "vc_sharded_search_knn", "vc_sharded_shard", "vc_sharded_search_knn_dev", "vc_sharded_root_device", "vc_search_knn_dev_stats", "vc_sharded_search_radius",
    "vc_sharded_search_radius_dev",
    "vc_get_codes_dev", "vc_search_knn_ids", "vc_search_knn_ids_dev",
    "vc_sharded_get_codes_dev", "vc_sharded_search_knn_ids", "vc_sharded_search_knn_ids_dev",
    "vc_search_radius_ids", "vc_search_radius_ids_dev", "vc_sharded_search_radius_ids", "vc_sharded_search_radius_ids_dev",
    "vc_update_index", "vc_sharded_update_index", "vc_build_scan_stream", "vc_scan_stream_info",
    "vc_cluster_radius", "vc_cluster_radius_dev", "vc_sharded_cluster_radius", "vc_sharded_cluster_radius_dev",
    "vc_retain", "vc_retain_dev", "vc_sharded_retain", "vc_sharded_retain_dev",
    "vc_leaders_radius", "vc_leaders_radius_dev", "vc_sharded_leaders_radius", "vc_sharded_leaders_radius_dev",
    "vc_dbscan_radius", "vc_dbscan_radius_dev", "vc_sharded_dbscan_radius", "vc_sharded_dbscan_radius_dev",
    "vc_group_summary", "vc_group_summary_dev", "vc_sharded_group_summary", "vc_sharded_group_summary_dev",
    "vc_cluster_levels", "vc_cluster_levels_dev", "vc_sharded_cluster_levels", "vc_sharded_cluster_levels_dev",
    "vc_dbscan_levels", "vc_dbscan_levels_dev", "vc_sharded_dbscan_levels", "vc_sharded_dbscan_levels_dev",
    "vc_assign_nearest", "vc_assign_nearest_dev", "vc_sharded_assign_nearest", "vc_sharded_assign_nearest_dev",
    "vc_kmajority", "vc_kmajority_dev", "vc_sharded_kmajority", "vc_sharded_kmajority_dev",
    "vc_seed_centres", "vc_seed_centres_dev", "vc_sharded_seed_centres", "vc_sharded_seed_centres_dev",
    "vc_search_knn_distinct", "vc_search_knn_distinct_dev", "vc_sharded_search_knn_distinct", "vc_sharded_search_knn_distinct_dev",
    "vc_search_knn_filtered", "vc_search_knn_filtered_dev", "vc_sharded_search_knn_filtered", "vc_sharded_search_knn_filtered_dev",
    "vc_search_knn_scoped", "vc_search_knn_scoped_dev", "vc_sharded_search_knn_scoped", "vc_sharded_search_knn_scoped_dev",
    "vc_knn_graph", "vc_knn_graph_dev", "vc_sharded_knn_graph", "vc_sharded_knn_graph_dev",
    "vc_cluster_knn", "vc_cluster_knn_dev", "vc_sharded_cluster_knn", "vc_sharded_cluster_knn_dev",
    "vc_knn_graph_update", "vc_knn_graph_update_dev", "vc_sharded_knn_graph_update", "vc_sharded_knn_graph_update_dev",
    "vc_knn_graph_retain", "vc_knn_graph_retain_dev", "vc_sharded_knn_graph_retain", "vc_sharded_knn_graph_retain_dev",
    "vc_cluster_snn", "vc_cluster_snn_dev", "vc_sharded_cluster_snn", "vc_sharded_cluster_snn_dev",
    "vc_knn_adjacency", "vc_knn_adjacency_dev", "vc_sharded_knn_adjacency", "vc_sharded_knn_adjacency_dev",
    "vc_knn_mst", "vc_knn_mst_dev", "vc_sharded_knn_mst", "vc_sharded_knn_mst_dev",
    "vc_mst_cut", "vc_mst_cut_dev", "vc_sharded_mst_cut", "vc_sharded_mst_cut_dev",
    "vc_knn_vote", "vc_knn_vote_dev", "vc_sharded_knn_vote", "vc_sharded_knn_vote_dev",
    "vc_label_propagate", "vc_label_propagate_dev", "vc_sharded_label_propagate", "vc_sharded_label_propagate_dev",
    "vc_mst_condense", "vc_mst_condense_dev", "vc_sharded_mst_condense", "vc_sharded_mst_condense_dev",
]
KNN_MUTUAL, KNN_EITHER = 0, 1   # VC_KNN_*: cluster_knn joins i and j iff each lists the other / iff one lists the other
KNN_REVERSE = 2                 # VC_KNN_REVERSE: knn_adjacency only -- segment j holds every record that lists j
VOTE_NONE = 0xFFFFFFFF               # VC_VOTE_NONE: the label word of an unlabelled record; such an entry does not vote
VOTE_COUNT, VOTE_CLOSENESS = 0, 1    # VC_VOTE_*: a voting entry weighs 1 / bits + 1 - its distance
LP_CLAMP_SEEDS, LP_MAX_ITERS = 1, 64   # VC_LP_*: label_propagate keeps every labelled record of labels_in fixed; the most rounds of a call
CONDENSE_EOM, CONDENSE_LEAF = 0, 1     # VC_CONDENSE_*: mst_condense selects by excess of mass / selects the leaves of the condensed tree
CONDENSE_NONE = 0xFFFFFFFF             # VC_CONDENSE_NONE: no node -- a root's parent, a noise record's node, own and leave
CONDENSE_SELECTED, CONDENSE_KEEP, CONDENSE_ROOT = 1, 2, 4   # bits of CONDENSED_NODE's flags
MST_DISTANCE, MST_REACHABILITY = 0, 1   # VC_MST_*: knn_mst weighs an edge by its distance / by max(distance, the two core distances at min_pts)
SNN_NONE, SNN_MAX_KK = 0xFFFFFFFF, 1024   # VC_SNN_NONE: the weight word of an entry that is not listed; VC_SNN_MAX_KK: the widest kk of cluster_snn
FILTER_MASK, FILTER_ROOTS, FILTER_EQUAL, FILTER_NOT_EQUAL, FILTER_BITS = 0, 1, 2, 3, 4   # VC_FILTER_*: how search_knn_filtered reads `sel`
FILTER_RAN_POST, FILTER_RAN_PRE = 1, 2   # VC_FILTER_RAN_*: bits of VcFilterStats.routes
DISTINCT_TRUNCATED = 0x80000000   # VC_DISTINCT_TRUNCATED: flag in a count of search_knn_distinct -- the row holds the groups found within the 8192 nearest records
SEED_FARTHEST, SEED_WEIGHTED = 0, 1   # VC_SEED_FARTHEST: farthest-first traversal; VC_SEED_WEIGHTED: distance-weighted sampling ("k-majority++")
KMAJ_MAX_ITERS = 64       # VC_KMAJ_MAX_ITERS: kmajority takes max_iters 0 .. 64
LEVELS_MAX = 64           # VC_LEVELS_MAX: cluster_levels and dbscan_levels take max_radius 0 .. 63
CORE_NEVER = 0xFFFFFFFF   # VC_CORE_NEVER: dbscan_levels' core_dist of a record with fewer than min_pts records within max_radius
MAX_SHARDS = 16
EXCHANGE_AUTO, EXCHANGE_PEER_COPY, EXCHANGE_RCCL = 0, 1, 2


class VcConfig(C.Structure):
    _fields_ = [
        ("abi_version", C.c_uint32), ("bits", C.c_uint32), ("n_tables", C.c_uint32), ("flags", C.c_uint32),
        ("capacity", C.c_uint64), ("id_base", C.c_uint32), ("device", C.c_int32), ("cand_cap", C.c_uint32),
        ("scan_blocks", C.c_uint32), ("query_tile", C.c_uint32), ("timing_sample", C.c_uint32), ("reserved", C.c_uint32 * 4),
    ]


class VcShardedConfig(C.Structure):
    _fields_ = [
        ("abi_version", C.c_uint32), ("n_shards", C.c_uint32), ("n_devices", C.c_uint32), ("exchange", C.c_uint32),
        ("device_ids", C.c_int32 * 16), ("engine", VcConfig),
    ]


class VcQueryStats(C.Structure):
    _fields_ = [
        ("radius", C.c_uint32), ("n_results", C.c_uint32), ("n_main_reads", C.c_uint64), ("n_sub_reads", C.c_uint64),
        ("n_local_reads", C.c_uint64), ("n_candidates", C.c_uint64),
    ]


class VcClusterStats(C.Structure):
    _fields_ = [("n_pairs", C.c_uint64), ("n_clusters", C.c_uint64)]


class VcLevelsStats(C.Structure):
    _fields_ = [("n_pairs", C.c_uint64 * LEVELS_MAX), ("n_clusters", C.c_uint64 * LEVELS_MAX)]


class VcLeaderStats(C.Structure):
    _fields_ = [("n_pairs", C.c_uint64), ("n_leaders", C.c_uint64), ("n_rounds", C.c_uint64)]


class VcDbscanStats(C.Structure):
    _fields_ = [("n_pairs", C.c_uint64), ("n_clusters", C.c_uint64), ("n_core", C.c_uint64), ("n_border", C.c_uint64), ("n_noise", C.c_uint64)]

    def as_dict(self):
        return {name: int(getattr(self, name)) for name, _ in self._fields_}


class VcDbscanLevelsStats(C.Structure):
    _fields_ = [("n_pairs", C.c_uint64 * LEVELS_MAX), ("n_clusters", C.c_uint64 * LEVELS_MAX), ("n_core", C.c_uint64 * LEVELS_MAX),
                ("n_border", C.c_uint64 * LEVELS_MAX), ("n_noise", C.c_uint64 * LEVELS_MAX)]

    def as_dict(self, max_radius):
        """{field: uint64 [max_radius + 1]}"""
        return {name: np.array(getattr(self, name)[:max_radius + 1], dtype=np.uint64) for name, _ in self._fields_}


class VcKmajorityStats(C.Structure):
    _fields_ = [("n_iters", C.c_uint32), ("converged", C.c_uint32), ("n_empty", C.c_uint64), ("cost_final", C.c_uint64),
                ("cost", C.c_uint64 * KMAJ_MAX_ITERS), ("n_changed", C.c_uint64 * KMAJ_MAX_ITERS)]

    def as_dict(self):
        """{n_iters, converged, n_empty, cost_final: int; cost, n_changed: uint64 [KMAJ_MAX_ITERS], zero from n_iters on}"""
        return {name: (np.array(getattr(self, name)[:], dtype=np.uint64) if name in ("cost", "n_changed") else int(getattr(self, name)))
                for name, _ in self._fields_}


class VcSeedStats(C.Structure):
    _fields_ = [("cost", C.c_uint64), ("radius", C.c_uint32), ("n_zero_picks", C.c_uint32)]

    def as_dict(self):
        """{cost, radius, n_zero_picks: int}"""
        return {name: int(getattr(self, name)) for name, _ in self._fields_}


class VcDistinctStats(C.Structure):
    _fields_ = [("n_rounds", C.c_uint32), ("k_last", C.c_uint32), ("n_searched", C.c_uint64), ("n_truncated", C.c_uint64), ("n_short", C.c_uint64)]

    def as_dict(self):
        """{n_rounds, k_last, n_searched, n_truncated, n_short: int}"""
        return {name: int(getattr(self, name)) for name, _ in self._fields_}


class VcFilterStats(C.Structure):
    _fields_ = [("n_allowed", C.c_uint64), ("routes", C.c_uint32), ("n_rounds", C.c_uint32), ("k_last", C.c_uint32), ("n_windows", C.c_uint32),
                ("n_searched", C.c_uint64), ("n_fallback", C.c_uint64), ("n_short", C.c_uint64)]

    def as_dict(self):
        """{n_allowed, routes, n_rounds, k_last, n_windows, n_searched, n_fallback, n_short: int}"""
        return {name: int(getattr(self, name)) for name, _ in self._fields_}


class VcScopeStats(C.Structure):
    _fields_ = [("n_matched", C.c_uint64), ("n_pairs", C.c_uint64), ("n_scopes", C.c_uint32), ("n_windows", C.c_uint32), ("n_short", C.c_uint64),
                ("n_empty", C.c_uint64)]

    def as_dict(self):
        """{n_matched, n_pairs, n_scopes, n_windows, n_short, n_empty: int}"""
        return {name: int(getattr(self, name)) for name, _ in self._fields_}


class VcKnnGraphStats(C.Structure):
    _fields_ = [("n_rounds_max", C.c_uint32), ("k_last", C.c_uint32), ("n_searched", C.c_uint64), ("n_linear", C.c_uint64), ("n_gave_up", C.c_uint64)]

    def as_dict(self):
        """{n_rounds_max, k_last, n_searched, n_linear, n_gave_up: int}"""
        return {name: int(getattr(self, name)) for name, _ in self._fields_}


class VcKnnGraphUpdateStats(C.Structure):
    _fields_ = [("build", VcKnnGraphStats), ("n_rows_changed", C.c_uint64), ("n_inserted", C.c_uint64), ("n_hits", C.c_uint64),
                ("n_windows", C.c_uint32), ("n_halvings", C.c_uint32)]

    def as_dict(self):
        """{build: VcKnnGraphStats' dict, n_rows_changed, n_inserted, n_hits, n_windows, n_halvings: int}"""
        return {name: getattr(self, name).as_dict() if name == "build" else int(getattr(self, name)) for name, _ in self._fields_}


class VcKnnGraphRetainStats(C.Structure):
    _fields_ = [("repair", VcKnnGraphStats), ("n_rows_kept", C.c_uint64), ("n_rows_short", C.c_uint64), ("n_entries_dropped", C.c_uint64),
                ("pad", C.c_uint64)]

    def as_dict(self):
        """{repair: VcKnnGraphStats' dict, n_rows_kept, n_rows_short, n_entries_dropped: int}"""
        return {name: getattr(self, name).as_dict() if name == "repair" else int(getattr(self, name)) for name, _ in self._fields_ if name != "pad"}


class VcClusterKnnStats(C.Structure):
    _fields_ = [("n_edges", C.c_uint64), ("n_mutual", C.c_uint64), ("n_clusters", C.c_uint64), ("max_in_degree", C.c_uint32), ("pad", C.c_uint32)]

    def as_dict(self):
        """{n_edges, n_mutual, n_clusters, max_in_degree: int}"""
        return {name: int(getattr(self, name)) for name, _ in self._fields_ if name != "pad"}


class VcClusterSnnStats(C.Structure):
    _fields_ = [("n_edges", C.c_uint64), ("n_mutual", C.c_uint64), ("n_joined", C.c_uint64), ("n_clusters", C.c_uint64), ("max_shared", C.c_uint32),
                ("pad", C.c_uint32)]

    def as_dict(self):
        """{n_edges, n_mutual, n_joined, n_clusters, max_shared: int}"""
        return {name: int(getattr(self, name)) for name, _ in self._fields_ if name != "pad"}


class VcKnnAdjacencyStats(C.Structure):
    _fields_ = [("n_edges", C.c_uint64), ("n_entries", C.c_uint64), ("n_empty", C.c_uint64), ("max_degree", C.c_uint32), ("pad", C.c_uint32)]

    def as_dict(self):
        """{n_edges, n_entries, n_empty, max_degree: int}"""
        return {name: int(getattr(self, name)) for name, _ in self._fields_ if name != "pad"}


class VcKnnMstStats(C.Structure):
    _fields_ = [("n_edges", C.c_uint64), ("n_graph_edges", C.c_uint64), ("n_tree", C.c_uint64), ("n_clusters", C.c_uint64), ("total_weight", C.c_uint64),
                ("max_weight", C.c_uint32), ("n_rounds", C.c_uint32)]

    def as_dict(self):
        """{n_edges, n_graph_edges, n_tree, n_clusters, total_weight, max_weight, n_rounds: int}"""
        return {name: int(getattr(self, name)) for name, _ in self._fields_}


class VcKnnVoteStats(C.Structure):
    _fields_ = [("n_voted", C.c_uint64), ("n_unlabelled", C.c_uint64), ("n_ties", C.c_uint64), ("n_entries", C.c_uint64)]

    def as_dict(self):
        """{n_voted, n_unlabelled, n_ties, n_entries: int}"""
        return {name: int(getattr(self, name)) for name, _ in self._fields_}


class VcLabelPropagateStats(C.Structure):
    _fields_ = [("n_iters", C.c_uint32), ("converged", C.c_uint32), ("n_changed_last", C.c_uint64), ("n_labelled", C.c_uint64), ("n_ties_last", C.c_uint64)]

    def as_dict(self):
        """{n_iters, converged, n_changed_last, n_labelled, n_ties_last: int}"""
        return {name: int(getattr(self, name)) for name, _ in self._fields_}


MST_EDGE = np.dtype([("a", np.uint32), ("b", np.uint32), ("weight", np.uint32), ("dist", np.uint32)])   # vc_mst_edge, 16 bytes
CONDENSED_NODE = np.dtype([("parent", np.uint32), ("rep", np.uint32), ("form", np.uint32), ("end", np.uint32), ("size", np.uint32), ("n_children", np.uint32),
                           ("flags", np.uint32), ("pad", np.uint32), ("stability", np.uint64), ("best", np.uint64)])   # vc_condensed_node, 48 bytes


class VcMstCondenseStats(C.Structure):
    _fields_ = [("n_nodes", C.c_uint64), ("n_leaves", C.c_uint64), ("n_roots", C.c_uint64), ("n_selected", C.c_uint64), ("n_clustered", C.c_uint64),
                ("n_noise", C.c_uint64), ("total_stability", C.c_uint64), ("n_levels", C.c_uint32), ("pad", C.c_uint32)]

    def as_dict(self):
        """{n_nodes, n_leaves, n_roots, n_selected, n_clustered, n_noise, total_stability, n_levels: int}"""
        return {name: int(getattr(self, name)) for name, _ in self._fields_ if name != "pad"}


class VcTiming(C.Structure):
    _fields_ = [
        ("total_ms", C.c_float), ("scan_ms", C.c_float), ("scan_launches", C.c_uint32), ("calls", C.c_uint32),
        ("scan_bytes", C.c_uint64),
        ("mih_ms", C.c_float), ("mih_launches", C.c_uint32), ("mih_queries", C.c_uint64), ("mih_probes", C.c_uint64),
        ("mih_hits", C.c_uint64), ("mih_entries", C.c_uint64),
    ]


class VcScanStreamState(C.Structure):
    """vc_scan_stream_state: what vc_scan_stream_info reports of an engine's prefix-sorted scan stream"""
    _fields_ = [
        ("built", C.c_uint32), ("reserved", C.c_uint32), ("items", C.c_uint64), ("granules", C.c_uint64), ("bytes", C.c_uint64),
        ("launches", C.c_uint64), ("bound_passes", C.c_uint64), ("exact_passes", C.c_uint64),
    ]

    def as_dict(self):
        return {name: int(getattr(self, name)) for name, _ in self._fields_ if name != "reserved"}


class VcError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__("verticut_gpu error %d: %s" % (code, msg))
        self.code = code


_lib = None


def load_library():
    """dlopen the in-tree HIP library; raises (never falls back) when it is absent."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            "%s is missing: build it with `python -m verticut_amd.build` (hipcc, gfx950). "
            "verticut_amd has no CPU fallback." % LIB_PATH)
    # One HIP runtime per process: the PyTorch-ROCm wheel bundles its own libamdhip64.so (soname libamdhip64.so.7) and
    # asks for it as "libamdhip64.so"; if our library pulled in /opt/rocm's copy first, torch would load a second
    # runtime next to it and find no GPU.  Loading torch first makes our NEEDED libamdhip64.so.7 resolve to that copy.
    import importlib.util
    import sys
    if "torch" not in sys.modules and importlib.util.find_spec("torch") is not None:
        import torch  # noqa: F401
    L = C.CDLL(LIB_PATH)
    vp, u32, u64 = C.c_void_p, C.c_uint32, C.c_uint64
    L.vc_create.argtypes = [C.POINTER(VcConfig), C.POINTER(vp)]
    L.vc_destroy.argtypes = [vp]
    L.vc_last_error.restype = C.c_char_p
    L.vc_last_error.argtypes = [vp]
    L.vc_strerror.restype = C.c_char_p
    L.vc_strerror.argtypes = [C.c_int]
    L.vc_add_codes.argtypes = [vp, vp, u64]
    L.vc_add_synthetic.argtypes = [vp, u64, u64, u32, u32, u32]
    L.vc_size.argtypes = [vp, C.POINTER(u64)]
    L.vc_get_code.argtypes = [vp, u32, vp]
    L.vc_build_index.argtypes = [vp]
    L.vc_update_index.argtypes = [vp]
    L.vc_build_scan_stream.argtypes = [vp]
    L.vc_scan_stream_info.argtypes = [vp, C.POINTER(VcScanStreamState)]
    L.vc_get_bucket.argtypes = [vp, u32, u32, vp, vp, u32, C.POINTER(u32)]
    L.vc_bitmap_test.argtypes = [vp, u32, u32, C.POINTER(C.c_int)]
    L.vc_bitmap_read.argtypes = [vp, u32, u64, u64, vp]
    L.vc_search_knn.argtypes = [vp, vp, u32, u32, u32, u32, vp, vp, vp]
    L.vc_search_knn_dev.argtypes = [vp, vp, u32, u32, u32, vp, vp, vp]
    L.vc_search_knn_dev_stats.argtypes = [vp, vp, u32, u32, u32, vp, vp, vp, vp]
    L.vc_search_radius.argtypes = [vp, vp, u32, u32, u32, vp, u64, vp]
    L.vc_search_radius_dev.argtypes = [vp, vp, u32, u32, u32, vp, u64, vp, vp]
    L.vc_merge_topk_dev.argtypes = [vp, u32, u32, u32, vp, vp, vp]
    L.vc_load_code_file.argtypes = [vp, C.c_char_p, u64, C.POINTER(u64)]
    L.vc_save_code_file.argtypes = [vp, C.c_char_p]
    L.vc_write_bitmap_file.argtypes = [vp, u32, C.c_char_p]
    L.vc_read_bitmap_file.argtypes = [vp, u32, C.c_char_p, C.POINTER(u64)]
    L.vc_save_index.argtypes = [vp, C.c_char_p]
    L.vc_load_index.argtypes = [vp, C.c_char_p]
    L.vc_get_timing.argtypes = [vp, C.POINTER(VcTiming)]
    L.vc_set_stream.argtypes = [vp, vp]
    L.vc_device_status.argtypes = [vp, C.POINTER(u32)]
    L.vc_sharded_create.argtypes = [C.POINTER(VcShardedConfig), C.POINTER(vp)]
    L.vc_sharded_destroy.argtypes = [vp]
    L.vc_sharded_last_error.restype = C.c_char_p
    L.vc_sharded_last_error.argtypes = [vp]
    L.vc_sharded_exchange.argtypes = [vp, C.POINTER(u32)]
    L.vc_sharded_add_codes.argtypes = [vp, vp, u64]
    L.vc_sharded_add_synthetic.argtypes = [vp, u64, u64, u32, u32, u32]
    L.vc_sharded_size.argtypes = [vp, C.POINTER(u64)]
    L.vc_sharded_build_index.argtypes = [vp]
    L.vc_sharded_update_index.argtypes = [vp]
    L.vc_sharded_get_code.argtypes = [vp, u32, vp]
    L.vc_sharded_get_bucket.argtypes = [vp, u32, u32, vp, vp, u32, C.POINTER(u32)]
    L.vc_sharded_search_knn.argtypes = [vp, vp, u32, u32, u32, u32, vp, vp, vp]
    L.vc_sharded_shard.argtypes = [vp, u32, C.POINTER(vp), C.POINTER(u64), C.POINTER(u64)]
    L.vc_sharded_search_knn_dev.argtypes = [vp, vp, u32, u32, u32, vp, vp, vp, vp]
    L.vc_sharded_root_device.argtypes = [vp, C.POINTER(C.c_int)]
    L.vc_sharded_search_radius.argtypes = [vp, vp, u32, u32, u32, vp, u64, vp]
    L.vc_sharded_search_radius_dev.argtypes = [vp, vp, u32, u32, u32, vp, u64, vp, vp]
    L.vc_get_codes_dev.argtypes = [vp, vp, u32, vp, vp, vp]
    L.vc_search_knn_ids.argtypes = [vp, vp, u32, u32, u32, u32, u32, vp, vp, vp]
    L.vc_search_knn_ids_dev.argtypes = [vp, vp, u32, u32, u32, u32, vp, vp, vp, vp]
    L.vc_sharded_get_codes_dev.argtypes = [vp, vp, u32, vp, vp, vp]
    L.vc_sharded_search_knn_ids.argtypes = [vp, vp, u32, u32, u32, u32, u32, vp, vp, vp]
    L.vc_sharded_search_knn_ids_dev.argtypes = [vp, vp, u32, u32, u32, u32, vp, vp, vp, vp]
    L.vc_search_radius_ids.argtypes = [vp, vp, u32, u32, u32, u32, vp, u64, vp]
    L.vc_search_radius_ids_dev.argtypes = [vp, vp, u32, u32, u32, u32, vp, u64, vp, vp]
    L.vc_sharded_search_radius_ids.argtypes = [vp, vp, u32, u32, u32, u32, vp, u64, vp]
    L.vc_sharded_search_radius_ids_dev.argtypes = [vp, vp, u32, u32, u32, u32, vp, u64, vp, vp]
    L.vc_cluster_radius.argtypes = [vp, u32, u32, u32, u64, vp, vp]
    L.vc_cluster_radius_dev.argtypes = [vp, u32, u32, u32, u64, vp, vp, vp]
    L.vc_sharded_cluster_radius.argtypes = [vp, u32, u32, u32, u64, vp, vp]
    L.vc_sharded_cluster_radius_dev.argtypes = [vp, u32, u32, u32, u64, vp, vp, vp]
    L.vc_retain.argtypes = [vp, vp, u32, vp, vp]
    L.vc_retain_dev.argtypes = [vp, vp, u32, vp, vp, vp]
    L.vc_sharded_retain.argtypes = [vp, vp, u32, vp, vp]
    L.vc_sharded_retain_dev.argtypes = [vp, vp, u32, vp, vp, vp]
    L.vc_leaders_radius.argtypes = [vp, u32, u32, u32, u64, vp, vp]
    L.vc_leaders_radius_dev.argtypes = [vp, u32, u32, u32, u64, vp, vp, vp]
    L.vc_sharded_leaders_radius.argtypes = [vp, u32, u32, u32, u64, vp, vp]
    L.vc_sharded_leaders_radius_dev.argtypes = [vp, u32, u32, u32, u64, vp, vp, vp]
    L.vc_dbscan_radius.argtypes = [vp, u32, u32, u32, u32, vp, vp, vp]
    L.vc_dbscan_radius_dev.argtypes = [vp, u32, u32, u32, u32, vp, vp, vp, vp]
    L.vc_sharded_dbscan_radius.argtypes = [vp, u32, u32, u32, u32, vp, vp, vp]
    L.vc_sharded_dbscan_radius_dev.argtypes = [vp, u32, u32, u32, u32, vp, vp, vp, vp]
    L.vc_group_summary.argtypes = [vp, vp, u64, vp, vp, vp, vp, C.POINTER(u64)]
    L.vc_group_summary_dev.argtypes = [vp, vp, u64, vp, vp, vp, vp, C.POINTER(u64), vp]
    L.vc_sharded_group_summary.argtypes = [vp, vp, u64, vp, vp, vp, vp, C.POINTER(u64)]
    L.vc_sharded_group_summary_dev.argtypes = [vp, vp, u64, vp, vp, vp, vp, C.POINTER(u64), vp]
    L.vc_cluster_levels.argtypes = [vp, u32, u32, u32, u64, vp, vp]
    L.vc_cluster_levels_dev.argtypes = [vp, u32, u32, u32, u64, vp, vp, vp]
    L.vc_sharded_cluster_levels.argtypes = [vp, u32, u32, u32, u64, vp, vp]
    L.vc_sharded_cluster_levels_dev.argtypes = [vp, u32, u32, u32, u64, vp, vp, vp]
    L.vc_dbscan_levels.argtypes = [vp, u32, u32, u32, u32, vp, vp, vp]
    L.vc_dbscan_levels_dev.argtypes = [vp, u32, u32, u32, u32, vp, vp, vp, vp]
    L.vc_sharded_dbscan_levels.argtypes = [vp, u32, u32, u32, u32, vp, vp, vp]
    L.vc_sharded_dbscan_levels_dev.argtypes = [vp, u32, u32, u32, u32, vp, vp, vp, vp]
    L.vc_assign_nearest.argtypes = [vp, vp, u32, u64, u64, vp]
    L.vc_assign_nearest_dev.argtypes = [vp, vp, u32, u64, u64, vp, vp]
    L.vc_sharded_assign_nearest.argtypes = [vp, vp, u32, u64, u64, vp]
    L.vc_sharded_assign_nearest_dev.argtypes = [vp, vp, u32, u64, u64, vp, vp]
    L.vc_kmajority.argtypes = [vp, u32, u32, vp, vp, vp, vp]
    L.vc_kmajority_dev.argtypes = [vp, u32, u32, vp, vp, vp, vp, vp]
    L.vc_sharded_kmajority.argtypes = [vp, u32, u32, vp, vp, vp, vp]
    L.vc_sharded_kmajority_dev.argtypes = [vp, u32, u32, vp, vp, vp, vp, vp]
    L.vc_seed_centres.argtypes = [vp, u32, u32, u64, vp, vp, vp, vp]
    L.vc_seed_centres_dev.argtypes = [vp, u32, u32, u64, vp, vp, vp, vp, vp]
    L.vc_sharded_seed_centres.argtypes = [vp, u32, u32, u64, vp, vp, vp, vp]
    L.vc_sharded_seed_centres_dev.argtypes = [vp, u32, u32, u64, vp, vp, vp, vp, vp]
    L.vc_search_knn_filtered.argtypes = [vp, vp, u32, u32, u32, u32, vp, u32, u32, u32, vp, vp, vp]
    L.vc_search_knn_filtered_dev.argtypes = [vp, vp, u32, u32, u32, vp, u32, u32, u32, vp, vp, vp, vp]
    L.vc_sharded_search_knn_filtered.argtypes = [vp, vp, u32, u32, u32, u32, vp, u32, u32, u32, vp, vp, vp]
    L.vc_sharded_search_knn_filtered_dev.argtypes = [vp, vp, u32, u32, u32, vp, u32, u32, u32, vp, vp, vp, vp]
    L.vc_search_knn_scoped.argtypes = [vp, vp, u32, u32, u32, vp, vp, u32, vp, vp, vp]
    L.vc_search_knn_scoped_dev.argtypes = [vp, vp, u32, u32, vp, vp, u32, vp, vp, vp, vp]
    L.vc_sharded_search_knn_scoped.argtypes = [vp, vp, u32, u32, u32, vp, vp, u32, vp, vp, vp]
    L.vc_sharded_search_knn_scoped_dev.argtypes = [vp, vp, u32, u32, vp, vp, u32, vp, vp, vp, vp]
    L.vc_search_knn_distinct.argtypes = [vp, vp, u32, u32, u32, u32, vp, u32, vp, vp, vp, vp]
    L.vc_search_knn_distinct_dev.argtypes = [vp, vp, u32, u32, u32, vp, u32, vp, vp, vp, vp, vp]
    L.vc_sharded_search_knn_distinct.argtypes = [vp, vp, u32, u32, u32, u32, vp, u32, vp, vp, vp, vp]
    L.vc_sharded_search_knn_distinct_dev.argtypes = [vp, vp, u32, u32, u32, vp, u32, vp, vp, vp, vp, vp]
    L.vc_knn_graph.argtypes = [vp, u32, u32, u32, u64, u64, u32, vp, vp, vp]
    L.vc_knn_graph_dev.argtypes = [vp, u32, u32, u32, u64, u64, u32, vp, vp, vp, vp]
    L.vc_sharded_knn_graph.argtypes = [vp, u32, u32, u32, u64, u64, u32, vp, vp, vp]
    L.vc_sharded_knn_graph_dev.argtypes = [vp, u32, u32, u32, u64, u64, u32, vp, vp, vp, vp]
    L.vc_knn_graph_update.argtypes = [vp, u32, u32, u32, u64, u32, vp, vp, vp]
    L.vc_knn_graph_update_dev.argtypes = [vp, u32, u32, u32, u64, u32, vp, vp, vp, vp]
    L.vc_sharded_knn_graph_update.argtypes = [vp, u32, u32, u32, u64, u32, vp, vp, vp]
    L.vc_sharded_knn_graph_update_dev.argtypes = [vp, u32, u32, u32, u64, u32, vp, vp, vp, vp]
    L.vc_knn_graph_retain.argtypes = [vp, u32, u32, u32, u64, u32, vp, vp, vp, vp]
    L.vc_knn_graph_retain_dev.argtypes = [vp, u32, u32, u32, u64, u32, vp, vp, vp, vp, vp]
    L.vc_sharded_knn_graph_retain.argtypes = [vp, u32, u32, u32, u64, u32, vp, vp, vp, vp]
    L.vc_sharded_knn_graph_retain_dev.argtypes = [vp, u32, u32, u32, u64, u32, vp, vp, vp, vp, vp]
    L.vc_cluster_knn.argtypes = [vp, vp, vp, u32, u32, u32, u32, vp, vp, vp]
    L.vc_cluster_knn_dev.argtypes = [vp, vp, vp, u32, u32, u32, u32, vp, vp, vp, vp]
    L.vc_sharded_cluster_knn.argtypes = [vp, vp, vp, u32, u32, u32, u32, vp, vp, vp]
    L.vc_sharded_cluster_knn_dev.argtypes = [vp, vp, vp, u32, u32, u32, u32, vp, vp, vp, vp]
    L.vc_cluster_snn.argtypes = [vp, vp, vp, u32, u32, u32, u32, u32, vp, vp, vp, vp]
    L.vc_cluster_snn_dev.argtypes = [vp, vp, vp, u32, u32, u32, u32, u32, vp, vp, vp, vp, vp]
    L.vc_sharded_cluster_snn.argtypes = [vp, vp, vp, u32, u32, u32, u32, u32, vp, vp, vp, vp]
    L.vc_sharded_cluster_snn_dev.argtypes = [vp, vp, vp, u32, u32, u32, u32, u32, vp, vp, vp, vp, vp]
    L.vc_knn_adjacency.argtypes = [vp, vp, vp, u32, u32, u32, u32, vp, u64, vp, vp]
    L.vc_knn_adjacency_dev.argtypes = [vp, vp, vp, u32, u32, u32, u32, vp, u64, vp, vp, vp]
    L.vc_sharded_knn_adjacency.argtypes = [vp, vp, vp, u32, u32, u32, u32, vp, u64, vp, vp]
    L.vc_sharded_knn_adjacency_dev.argtypes = [vp, vp, vp, u32, u32, u32, u32, vp, u64, vp, vp, vp]
    for pre in ("vc_", "vc_sharded_"):
        getattr(L, pre + "knn_mst").argtypes = [vp, vp, vp, u32, u32, u32, u32, u32, u32, vp, vp, vp, vp]
        getattr(L, pre + "knn_mst_dev").argtypes = [vp, vp, vp, u32, u32, u32, u32, u32, u32, vp, vp, vp, vp, vp]
        getattr(L, pre + "mst_cut").argtypes = [vp, vp, u64, u32, vp, vp]
        getattr(L, pre + "mst_cut_dev").argtypes = [vp, vp, u64, u32, vp, vp, vp]
        getattr(L, pre + "mst_condense").argtypes = [vp, vp, u64, u32, u32, u32, vp, vp, vp, vp, vp, vp]
        getattr(L, pre + "mst_condense_dev").argtypes = [vp, vp, u64, u32, u32, u32, vp, vp, vp, vp, vp, vp, vp]
        getattr(L, pre + "knn_vote").argtypes = [vp, vp, vp, u64, u32, u32, u32, vp, u32, vp, vp, vp, vp]
        getattr(L, pre + "knn_vote_dev").argtypes = [vp, vp, vp, u64, u32, u32, u32, vp, u32, vp, vp, vp, vp, vp]
        getattr(L, pre + "label_propagate").argtypes = [vp, vp, vp, u64, vp, u32, u32, u32, vp, vp, vp, vp]
        getattr(L, pre + "label_propagate_dev").argtypes = [vp, vp, vp, u64, vp, u32, u32, u32, vp, vp, vp, vp, vp]
    for name in EXPORTS:
        if getattr(L, name).restype is not C.c_char_p:
            getattr(L, name).restype = C.c_int
    _lib = L
    return L


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def _search_knn_ids(self, fn, ids, k, mode, order, id_flags, with_stats):
    """shared by Engine.search_knn_ids and ShardedEngine.search_knn_ids: numpy ids in, (rows, counts[, stats]) out"""
    ids = np.ascontiguousarray(ids, dtype=np.uint32).reshape(-1)
    nq = ids.shape[0]
    out = np.empty((nq, k), dtype=np.uint64)
    counts = np.zeros(nq, dtype=np.uint32)
    stats = (VcQueryStats * nq)() if with_stats else None
    self._check(fn(self._h, _p(ids), nq, k, mode, order, id_flags, _p(out), _p(counts), C.cast(stats, C.c_void_p) if with_stats else None))
    if with_stats:
        return out, counts, list(stats)
    return out, counts


def _search_radius_ids(self, fn, ids, radius, mode, id_flags, cap_per_query):
    """shared by Engine.search_radius_ids and ShardedEngine.search_radius_ids: numpy ids in, a list of ascending packed arrays out;
    one retry with offsets[nq] entries on VC_ERR_CAPACITY, as search_radius does"""
    ids = np.ascontiguousarray(ids, dtype=np.uint32).reshape(-1)
    nq = ids.shape[0]
    offs = np.zeros(nq + 1, dtype=np.uint64)
    cap = nq * cap_per_query
    for _ in range(2):
        out = np.empty(max(cap, 1), dtype=np.uint64)
        rc = self._check(fn(self._h, _p(ids), nq, radius, mode, id_flags, _p(out), cap, _p(offs)), ok=(VC_OK, VC_ERR_CAPACITY))
        if rc == VC_OK:
            return [out[int(offs[i]):int(offs[i + 1])].copy() for i in range(nq)]
        cap = int(offs[nq])
    raise VcError(VC_ERR_CAPACITY, "radius search output does not fit")


def _cluster_radius(self, fn, radius, mode, batch, labels):
    """shared by Engine.cluster_radius and ShardedEngine.cluster_radius: (labels [N] uint32, n_pairs, n_clusters)"""
    n = len(self)
    out = np.empty(n, dtype=np.uint32)
    n_labelled = 0
    if labels is not None:
        old = np.ascontiguousarray(labels, dtype=np.uint32).reshape(-1)
        n_labelled = old.shape[0]
        if n_labelled > n:
            raise VcError(VC_ERR_INVALID, "more labels than resident records")
        out[:n_labelled] = old
    st = VcClusterStats()
    self._check(fn(self._h, radius, mode, batch, n_labelled, _p(out), C.byref(st)))
    return out, int(st.n_pairs), int(st.n_clusters)


def _cluster_radius_dev(self, fn, radius, d_labels, mode, batch, n_labelled, stream):
    st = VcClusterStats()
    self._check(fn(self._h, radius, mode, batch, n_labelled, d_labels, C.byref(st), stream))
    return int(st.n_pairs), int(st.n_clusters)


def _levels_arrays(st, max_radius):
    return (np.array(st.n_pairs[:max_radius + 1], dtype=np.uint64), np.array(st.n_clusters[:max_radius + 1], dtype=np.uint64))


def _cluster_levels(self, fn, max_radius, mode, batch, labels):
    """shared by Engine.cluster_levels and ShardedEngine.cluster_levels: (labels [max_radius + 1, N] uint32, n_pairs [max_radius + 1],
    n_clusters [max_radius + 1]); `labels` [max_radius + 1, n_labelled] of an earlier call is re-laid to the stride N here"""
    n = len(self)
    out = np.empty((max_radius + 1, n), dtype=np.uint32)
    n_labelled = 0
    if labels is not None:
        old = np.ascontiguousarray(labels, dtype=np.uint32)
        if old.ndim != 2 or old.shape[0] != max_radius + 1:
            raise VcError(VC_ERR_INVALID, "the labels must have one row per level 0 .. max_radius")
        n_labelled = old.shape[1]
        if n_labelled > n:
            raise VcError(VC_ERR_INVALID, "more labels than resident records")
        out[:, :n_labelled] = old
    st = VcLevelsStats()
    self._check(fn(self._h, max_radius, mode, batch, n_labelled, _p(out), C.byref(st)))
    return (out,) + _levels_arrays(st, max_radius)


def _cluster_levels_dev(self, fn, max_radius, d_labels, mode, batch, n_labelled, stream):
    st = VcLevelsStats()
    self._check(fn(self._h, max_radius, mode, batch, n_labelled, d_labels, C.byref(st), stream))
    return _levels_arrays(st, max_radius)


def _leaders_radius(self, fn, radius, mode, batch, labels):
    """shared by Engine.leaders_radius and ShardedEngine.leaders_radius: (labels [N] uint32, n_pairs, n_leaders, n_rounds)"""
    n = len(self)
    out = np.empty(n, dtype=np.uint32)
    n_labelled = 0
    if labels is not None:
        old = np.ascontiguousarray(labels, dtype=np.uint32).reshape(-1)
        n_labelled = old.shape[0]
        if n_labelled > n:
            raise VcError(VC_ERR_INVALID, "more labels than resident records")
        out[:n_labelled] = old
    st = VcLeaderStats()
    self._check(fn(self._h, radius, mode, batch, n_labelled, _p(out), C.byref(st)))
    return out, int(st.n_pairs), int(st.n_leaders), int(st.n_rounds)


def _leaders_radius_dev(self, fn, radius, d_labels, mode, batch, n_labelled, stream):
    st = VcLeaderStats()
    self._check(fn(self._h, radius, mode, batch, n_labelled, d_labels, C.byref(st), stream))
    return int(st.n_pairs), int(st.n_leaders), int(st.n_rounds)


def _dbscan_radius(self, fn, radius, min_pts, mode, batch):
    """shared by Engine.dbscan_radius and ShardedEngine.dbscan_radius: (labels [N] uint32, degrees [N] uint32, stats dict)"""
    n = len(self)
    labels, degrees = np.empty(n, dtype=np.uint32), np.empty(n, dtype=np.uint32)
    st = VcDbscanStats()
    self._check(fn(self._h, radius, min_pts, mode, batch, _p(labels), _p(degrees), C.byref(st)))
    return labels, degrees, st.as_dict()


def _dbscan_radius_dev(self, fn, radius, min_pts, d_labels, d_degrees, mode, batch, stream):
    st = VcDbscanStats()
    self._check(fn(self._h, radius, min_pts, mode, batch, d_labels, d_degrees, C.byref(st), stream))
    return st.as_dict()


def _dbscan_levels(self, fn, max_radius, min_pts, mode, batch):
    """shared by Engine.dbscan_levels and ShardedEngine.dbscan_levels: (labels [max_radius + 1, N] uint32, core_dist [N] uint32,
    stats dict of [max_radius + 1] arrays)"""
    n = len(self)
    labels, core_dist = np.empty((max_radius + 1, n), dtype=np.uint32), np.empty(n, dtype=np.uint32)
    st = VcDbscanLevelsStats()
    self._check(fn(self._h, max_radius, min_pts, mode, batch, _p(labels), _p(core_dist), C.byref(st)))
    return labels, core_dist, st.as_dict(max_radius)


def _dbscan_levels_dev(self, fn, max_radius, min_pts, d_labels, d_core_dist, mode, batch, stream):
    st = VcDbscanLevelsStats()
    self._check(fn(self._h, max_radius, min_pts, mode, batch, d_labels, d_core_dist, C.byref(st), stream))
    return st.as_dict(max_radius)


# vc_group, field for field
GROUP_DTYPE = np.dtype([("label", "<u4"), ("size", "<u4"), ("rep", "<u4"), ("rep_dist", "<u4"), ("max_dist", "<u4"), ("reserved", "<u4")])


def _group_summary(self, fn, labels):
    """shared by Engine.group_summary and ShardedEngine.group_summary: (groups [G] GROUP_DTYPE, centroids [G, bits / 8] uint8,
    rep_labels [N] uint32, group_index [N] uint32); called with groups_cap = N, so there is no second call"""
    n = len(self)
    labels = np.ascontiguousarray(labels, dtype=np.uint32).reshape(-1)
    if labels.shape[0] != n:
        raise VcError(VC_ERR_INVALID, "the labels must have one word per resident record")
    groups = np.zeros(n, dtype=GROUP_DTYPE)
    cents = np.zeros((n, self.bits // 8), dtype=np.uint8)
    rep_labels, group_index = np.empty(n, dtype=np.uint32), np.empty(n, dtype=np.uint32)
    g = C.c_uint64(0)
    self._check(fn(self._h, _p(labels) if n else None, n, _p(groups) if n else None, _p(cents) if n else None, _p(rep_labels) if n else None,
                   _p(group_index) if n else None, C.byref(g)))
    return groups[:g.value].copy(), cents[:g.value].copy(), rep_labels, group_index


def _group_summary_dev(self, fn, d_labels, groups_cap, d_groups, d_centroids, d_rep_labels, d_group_index, stream):
    """returns (rc, G): rc is VC_OK or VC_ERR_CAPACITY (G > groups_cap: no output was written)"""
    g = C.c_uint64(0)
    rc = self._check(fn(self._h, d_labels, groups_cap, d_groups, d_centroids, d_rep_labels, d_group_index, C.byref(g), stream), ok=(VC_OK, VC_ERR_CAPACITY))
    return rc, int(g.value)


def _assign_nearest(self, fn, centres, first, count):
    """shared by Engine.assign_nearest and ShardedEngine.assign_nearest: packed uint64 [count], centre index | distance << 32"""
    centres = np.ascontiguousarray(centres, dtype=np.uint8).reshape(-1, self.nbytes)
    if count is None:
        count = len(self) - first
    if count < 0:
        raise VcError(VC_ERR_INVALID, "the range starts behind the last resident record")
    out = np.empty(count, dtype=np.uint64)
    self._check(fn(self._h, _p(centres), centres.shape[0], first, count, _p(out) if count else None))
    return out


def _get_codes(self, ids):
    """uint8 [len(ids), bits / 8]: the codes of resident ids, by get_code"""
    out = np.empty((len(ids), self.nbytes), dtype=np.uint8)
    for j, gid in enumerate(ids):
        code = self.get_code(int(gid))
        if code is None:
            raise VcError(VC_NOT_FOUND, "id %d is not resident" % int(gid))
        out[j] = code
    return out


def _kmajority(self, fn, k, seed_ids, seeds, max_iters):
    """shared by Engine.kmajority and ShardedEngine.kmajority: (centres uint8 [k, bits / 8], assign uint64 [N], labels uint32 [N],
    stats dict).  seeds: the k start codes; else seed_ids: the ids whose codes are the seeds; else k ids spread evenly over the store."""
    n = len(self)
    if seeds is not None:
        centres = np.array(seeds, dtype=np.uint8).reshape(-1, self.nbytes)
        if centres.shape[0] != k:
            raise VcError(VC_ERR_INVALID, "the seeds must be k codes")
    else:
        if seed_ids is None:
            if not 0 < k <= max(n, 1) or n == 0:
                raise VcError(VC_ERR_INVALID, "k must be in 1 .. the number of resident records")
            seed_ids = self.id_base + np.arange(k, dtype=np.int64) * n // k
        if len(seed_ids) != k:
            raise VcError(VC_ERR_INVALID, "the seed ids must be k ids")
        centres = _get_codes(self, seed_ids)
    assign, labels = np.empty(n, dtype=np.uint64), np.empty(n, dtype=np.uint32)
    st = VcKmajorityStats()
    self._check(fn(self._h, k, max_iters, _p(centres), _p(assign), _p(labels), C.byref(st)))
    return centres, assign, labels, st.as_dict()


def _kmajority_dev(self, fn, k, d_centres, d_assign, d_labels, max_iters, stream):
    st = VcKmajorityStats()
    self._check(fn(self._h, k, max_iters, d_centres, d_assign, d_labels, C.byref(st), stream))
    return st.as_dict()


def _seed_centres(self, fn, k, method, seed, with_assign):
    """shared by Engine.seed_centres and ShardedEngine.seed_centres: (centres uint8 [k, bits / 8], picks uint64 [k], assign uint64 [N] |
    None, stats dict)"""
    n = len(self)
    centres, picks = np.zeros((k, self.nbytes), dtype=np.uint8), np.zeros(k, dtype=np.uint64)
    assign = np.empty(n, dtype=np.uint64) if with_assign else None
    st = VcSeedStats()
    self._check(fn(self._h, k, method, seed, _p(centres), _p(picks), _p(assign) if with_assign and n else None, C.byref(st)))
    return centres, picks, assign, st.as_dict()


def _seed_centres_dev(self, fn, k, d_centres, d_picks, d_assign, method, seed, with_stats, stream):
    st = VcSeedStats()
    self._check(fn(self._h, k, method, seed, d_centres, d_picks, d_assign, C.byref(st) if with_stats else None, stream))
    return st.as_dict() if with_stats else None


def _search_knn_distinct(self, fn, queries, k, labels, mode, order, k_first, with_stats):
    """shared by Engine.search_knn_distinct and ShardedEngine.search_knn_distinct: (out uint64 [nq, k], row_labels uint32 [nq, k], counts
    uint32 [nq][, stats dict])"""
    q = np.ascontiguousarray(queries, dtype=np.uint8).reshape(-1, self.nbytes)
    nq = q.shape[0]
    labels = np.ascontiguousarray(labels, dtype=np.uint32).reshape(-1)
    if labels.shape[0] != len(self):
        raise VcError(VC_ERR_INVALID, "the labels must have one word per resident record")
    if labels.shape[0] == 0:
        labels = np.zeros(1, dtype=np.uint32)       # (an empty store: the call reads no label, but takes no null pointer)
    out, row_labels, counts = np.empty((nq, k), dtype=np.uint64), np.empty((nq, k), dtype=np.uint32), np.zeros(nq, dtype=np.uint32)
    st = VcDistinctStats()
    self._check(fn(self._h, _p(q), nq, k, mode, order, _p(labels), k_first, _p(out), _p(row_labels), _p(counts), C.byref(st)))
    return (out, row_labels, counts, st.as_dict()) if with_stats else (out, row_labels, counts)


def _search_knn_distinct_dev(self, fn, d_queries, nq, k, d_labels, d_out, d_row_labels, d_counts, mode, k_first, with_stats, stream):
    st = VcDistinctStats()
    self._check(fn(self._h, d_queries, nq, k, mode, d_labels, k_first, d_out, d_row_labels, d_counts, C.byref(st) if with_stats else None, stream))
    return st.as_dict() if with_stats else None


def _search_knn_filtered(self, fn, queries, k, sel, kind, value, mode, order, k_first, with_stats):
    """shared by Engine.search_knn_filtered and ShardedEngine.search_knn_filtered: (out uint64 [nq, k], counts uint32 [nq][, stats dict])"""
    q = np.ascontiguousarray(queries, dtype=np.uint8).reshape(-1, self.nbytes)
    nq = q.shape[0]
    sel = np.ascontiguousarray(sel, dtype=np.uint32).reshape(-1)
    need = (len(self) + 31) // 32 if kind == FILTER_BITS else len(self)
    if sel.shape[0] != need:
        raise VcError(VC_ERR_INVALID, "sel must have one word per resident record (FILTER_BITS: one bit)")
    if sel.shape[0] == 0:
        sel = np.zeros(1, dtype=np.uint32)       # (an empty store: the call reads no word, but takes no null pointer)
    out, counts = np.empty((nq, k), dtype=np.uint64), np.zeros(nq, dtype=np.uint32)
    st = VcFilterStats()
    self._check(fn(self._h, _p(q), nq, k, mode, order, _p(sel), kind, value, k_first, _p(out), _p(counts), C.byref(st)))
    return (out, counts, st.as_dict()) if with_stats else (out, counts)


def _search_knn_filtered_dev(self, fn, d_queries, nq, k, d_sel, kind, value, d_out, d_counts, mode, k_first, with_stats, stream):
    st = VcFilterStats()
    self._check(fn(self._h, d_queries, nq, k, mode, d_sel, kind, value, k_first, d_out, d_counts, C.byref(st) if with_stats else None, stream))
    return st.as_dict() if with_stats else None


def _search_knn_scoped(self, fn, queries, k, scope, qscope, order, with_stats):
    """shared by Engine.search_knn_scoped and ShardedEngine.search_knn_scoped: (out uint64 [nq, k], counts uint32 [nq][, stats dict])"""
    q = np.ascontiguousarray(queries, dtype=np.uint8).reshape(-1, self.nbytes)
    nq = q.shape[0]
    scope = np.ascontiguousarray(scope, dtype=np.uint32).reshape(-1)
    qscope = np.ascontiguousarray(qscope, dtype=np.uint32).reshape(-1)
    if scope.shape[0] != len(self):
        raise VcError(VC_ERR_INVALID, "scope must have one word per resident record")
    if qscope.shape[0] != nq:
        raise VcError(VC_ERR_INVALID, "qscope must have one word per query")
    if scope.shape[0] == 0:
        scope = np.zeros(1, dtype=np.uint32)       # (an empty store: the call reads no word, but takes no null pointer)
    out, counts = np.empty((nq, k), dtype=np.uint64), np.zeros(nq, dtype=np.uint32)
    st = VcScopeStats()
    self._check(fn(self._h, _p(q), nq, k, order, _p(scope), _p(qscope), 0, _p(out), _p(counts), C.byref(st)))
    return (out, counts, st.as_dict()) if with_stats else (out, counts)


def _search_knn_scoped_dev(self, fn, d_queries, nq, k, d_scope, d_qscope, d_out, d_counts, with_stats, stream):
    st = VcScopeStats()
    self._check(fn(self._h, d_queries, nq, k, d_scope, d_qscope, 0, d_out, d_counts, C.byref(st) if with_stats else None, stream))
    return st.as_dict() if with_stats else None


def _knn_graph(self, fn, k, mode, batch, first, count, k_first, with_stats):
    """shared by Engine.knn_graph and ShardedEngine.knn_graph: (rows uint64 [n, k], counts uint32 [n][, stats dict]), n the positions covered"""
    n = len(self)
    if first > n or count > n - first:
        raise VcError(VC_ERR_INVALID, "the range leaves the resident records")
    rows_n = count if count else n - first
    rows, counts = np.empty((rows_n, k), dtype=np.uint64), np.zeros(rows_n, dtype=np.uint32)
    keep = rows if rows_n else np.zeros(1, dtype=np.uint64)   # (an empty range: the call writes no word, but takes no null pointer)
    st = VcKnnGraphStats()
    self._check(fn(self._h, k, mode, batch, first, count, k_first, _p(keep), _p(counts) if rows_n else None, C.byref(st)))
    return (rows, counts, st.as_dict()) if with_stats else (rows, counts)


def _knn_graph_dev(self, fn, k, d_rows, d_counts, mode, batch, first, count, k_first, with_stats, stream):
    st = VcKnnGraphStats()
    self._check(fn(self._h, k, mode, batch, first, count, k_first, d_rows, d_counts, C.byref(st) if with_stats else None, stream))
    return st.as_dict() if with_stats else None


def _knn_graph_update(self, fn, rows, counts, k, mode, batch, k_first, with_stats):
    """shared by Engine.knn_graph_update and ShardedEngine.knn_graph_update: (rows uint64 [N, k], counts uint32 [N] | None[, stats dict])"""
    n = len(self)
    old = np.ascontiguousarray(rows, dtype=np.uint64)
    if old.ndim != 2 or old.shape[0] > n or (k is not None and old.shape[1] != k):
        raise VcError(VC_ERR_INVALID, "rows must be the [n_old, k] graph of knn_graph over the store before the append")
    n_old, k = old.shape
    if counts is not None:
        counts = np.ascontiguousarray(counts, dtype=np.uint32).reshape(-1)
        if counts.shape[0] != n_old:
            raise VcError(VC_ERR_INVALID, "counts must have one word per old row")
    out = np.empty((max(n, 1), k), dtype=np.uint64)        # (an empty store: the call writes no word, but takes no null pointer)
    out[:n_old] = old
    cnt = None
    if counts is not None:
        cnt = np.zeros(max(n, 1), dtype=np.uint32)
        cnt[:n_old] = counts
    st = VcKnnGraphUpdateStats()
    self._check(fn(self._h, k, mode, batch, n_old, k_first, _p(out), _p(cnt) if cnt is not None else None, C.byref(st)))
    out, cnt = out[:n], cnt[:n] if cnt is not None else None
    return (out, cnt, st.as_dict()) if with_stats else (out, cnt)


def _knn_graph_update_dev(self, fn, k, n_old, d_rows, d_counts, mode, batch, k_first, with_stats, stream):
    st = VcKnnGraphUpdateStats()
    self._check(fn(self._h, k, mode, batch, n_old, k_first, d_rows, d_counts, C.byref(st) if with_stats else None, stream))
    return st.as_dict() if with_stats else None


def _knn_graph_retain(self, fn, rows, new_ids, counts, mode, batch, k_first, with_stats):
    """shared by Engine.knn_graph_retain and ShardedEngine.knn_graph_retain: (rows uint64 [K, k], counts uint32 [K] | None[, stats dict])"""
    n = len(self)
    out = np.array(rows, dtype=np.uint64, order="C")            # a copy: the call works in place
    new_ids = np.ascontiguousarray(new_ids, dtype=np.uint32).reshape(-1)
    if out.ndim != 2 or out.shape[0] < n or out.shape[1] == 0 or new_ids.shape[0] != out.shape[0]:
        raise VcError(VC_ERR_INVALID, "rows must be the [n_old, k] graph of knn_graph over the store before retain, new_ids the map retain returned")
    n_old, k = out.shape
    cnt = None
    if counts is not None:
        cnt = np.array(counts, dtype=np.uint32).reshape(-1)
        if cnt.shape[0] != n_old:
            raise VcError(VC_ERR_INVALID, "counts must have one word per old row")
    if n_old == 0:
        out, new_ids = np.empty((1, k), dtype=np.uint64), np.zeros(1, dtype=np.uint32)   # (the call writes no word, but takes no null pointer)
    st = VcKnnGraphRetainStats()
    self._check(fn(self._h, k, mode, batch, n_old, k_first, _p(new_ids), _p(out), _p(cnt) if cnt is not None and n_old else None, C.byref(st)))
    out, cnt = out[:n], cnt[:n] if cnt is not None else None
    return (out, cnt, st.as_dict()) if with_stats else (out, cnt)


def _knn_graph_retain_dev(self, fn, k, n_old, d_new_ids, d_rows, d_counts, mode, batch, k_first, with_stats, stream):
    st = VcKnnGraphRetainStats()
    self._check(fn(self._h, k, mode, batch, n_old, k_first, d_new_ids, d_rows, d_counts, C.byref(st) if with_stats else None, stream))
    return st.as_dict() if with_stats else None


def _cluster_knn(self, fn, rows, counts, kk, flags, max_dist, with_in_degree):
    """shared by Engine.cluster_knn and ShardedEngine.cluster_knn: (labels uint32 [N], in_degree uint32 [N] | None, stats dict)"""
    n = len(self)
    rows = np.ascontiguousarray(rows, dtype=np.uint64)
    if rows.ndim != 2 or rows.shape[0] != n:
        raise VcError(VC_ERR_INVALID, "rows must be the [N, k] graph of knn_graph over the whole store")
    k = rows.shape[1]
    if counts is not None:
        counts = np.ascontiguousarray(counts, dtype=np.uint32).reshape(-1)
        if counts.shape[0] != n:
            raise VcError(VC_ERR_INVALID, "counts must have one word per resident record")
    labels = np.empty(n, dtype=np.uint32)
    deg = np.zeros(n, dtype=np.uint32) if with_in_degree else None
    keep = rows if n else np.zeros(1, dtype=np.uint64)
    st = VcClusterKnnStats()
    self._check(fn(self._h, _p(keep), _p(counts) if counts is not None and n else None, k, kk, flags, max_dist,
                   _p(labels) if n else _p(np.zeros(1, dtype=np.uint32)), _p(deg) if with_in_degree and n else None, C.byref(st)))
    return labels, deg, st.as_dict()


def _cluster_knn_dev(self, fn, d_rows, d_counts, k, kk, flags, max_dist, d_labels, d_in_degree, with_stats, stream):
    st = VcClusterKnnStats()
    self._check(fn(self._h, d_rows, d_counts, k, kk, flags, max_dist, d_labels, d_in_degree, C.byref(st) if with_stats else None, stream))
    return st.as_dict() if with_stats else None


def _cluster_snn(self, fn, rows, counts, kk, min_shared, flags, max_dist, with_shared, with_hist):
    """shared by Engine.cluster_snn and ShardedEngine.cluster_snn: (labels uint32 [N], shared uint32 [N, kk] | None, hist uint64 [kk] | None, stats dict)"""
    n = len(self)
    rows = np.ascontiguousarray(rows, dtype=np.uint64)
    if rows.ndim != 2 or rows.shape[0] != n:
        raise VcError(VC_ERR_INVALID, "rows must be the [N, k] graph of knn_graph over the whole store")
    k = rows.shape[1]
    if counts is not None:
        counts = np.ascontiguousarray(counts, dtype=np.uint32).reshape(-1)
        if counts.shape[0] != n:
            raise VcError(VC_ERR_INVALID, "counts must have one word per resident record")
    labels = np.empty(n, dtype=np.uint32)
    width = kk if 1 <= kk <= SNN_MAX_KK else 1                       # (a refused kk writes nothing)
    shared = np.full((n, width), SNN_NONE, dtype=np.uint32) if with_shared else None
    hist = np.zeros(width, dtype=np.uint64) if with_hist else None
    keep = rows if n else np.zeros(1, dtype=np.uint64)
    st = VcClusterSnnStats()
    self._check(fn(self._h, _p(keep), _p(counts) if counts is not None and n else None, k, kk, flags, max_dist, min_shared,
                   _p(labels) if n else _p(np.zeros(1, dtype=np.uint32)), _p(shared) if with_shared and n else None, _p(hist) if with_hist and n else None,
                   C.byref(st)))
    return labels, shared, hist, st.as_dict()


def _cluster_snn_dev(self, fn, d_rows, d_counts, k, kk, min_shared, flags, max_dist, d_labels, d_shared, d_hist, with_stats, stream):
    st = VcClusterSnnStats()
    self._check(fn(self._h, d_rows, d_counts, k, kk, flags, max_dist, min_shared, d_labels, d_shared, d_hist, C.byref(st) if with_stats else None, stream))
    return st.as_dict() if with_stats else None


def _knn_adjacency(self, fn, rows, counts, kk, flags, max_dist):
    """shared by Engine.knn_adjacency and ShardedEngine.knn_adjacency: (offsets uint64 [N + 1], adj uint64 [T], stats dict); the
    output is sized by the bound, N kk words, twice that under KNN_EITHER"""
    n = len(self)
    rows = np.ascontiguousarray(rows, dtype=np.uint64)
    if rows.ndim != 2 or rows.shape[0] != n:
        raise VcError(VC_ERR_INVALID, "rows must be the [N, k] graph of knn_graph over the whole store")
    k = rows.shape[1]
    if counts is not None:
        counts = np.ascontiguousarray(counts, dtype=np.uint32).reshape(-1)
        if counts.shape[0] != n:
            raise VcError(VC_ERR_INVALID, "counts must have one word per resident record")
    cap = (2 if flags == KNN_EITHER else 1) * n * kk if 1 <= kk <= k else 0     # (a refused kk writes nothing)
    offsets = np.zeros(n + 1, dtype=np.uint64)
    adj = np.empty(max(cap, 1), dtype=np.uint64)
    keep = rows if n else np.zeros(1, dtype=np.uint64)
    st = VcKnnAdjacencyStats()
    self._check(fn(self._h, _p(keep), _p(counts) if counts is not None and n else None, k, kk, flags, max_dist, _p(adj), cap, _p(offsets), C.byref(st)))
    return offsets, adj[:int(offsets[n])].copy(), st.as_dict()


def _knn_adjacency_dev(self, fn, d_rows, d_counts, k, kk, flags, max_dist, d_adj, adj_cap, d_offsets, with_stats, stream):
    """returns (rc, stats): rc is VC_OK or VC_ERR_CAPACITY (T > adj_cap: the offsets and the stats are filled, d_adj is untouched)"""
    st = VcKnnAdjacencyStats()
    rc = self._check(fn(self._h, d_rows, d_counts, k, kk, flags, max_dist, d_adj, adj_cap, d_offsets, C.byref(st) if with_stats else None, stream),
                     ok=(VC_OK, VC_ERR_CAPACITY))
    return rc, st.as_dict() if with_stats else None


def _knn_mst(self, fn, rows, counts, kk, flags, max_dist, weight_kind, min_pts, with_labels, with_hist):
    """shared by Engine.knn_mst and ShardedEngine.knn_mst: (edges MST_EDGE [M], labels uint32 [N] | None, hist uint64 [bits + 1] | None,
    stats dict)"""
    n = len(self)
    rows = np.ascontiguousarray(rows, dtype=np.uint64)
    if rows.ndim != 2 or rows.shape[0] != n:
        raise VcError(VC_ERR_INVALID, "rows must be the [N, k] graph of knn_graph over the whole store")
    k = rows.shape[1]
    if counts is not None:
        counts = np.ascontiguousarray(counts, dtype=np.uint32).reshape(-1)
        if counts.shape[0] != n:
            raise VcError(VC_ERR_INVALID, "counts must have one word per resident record")
    edges = np.zeros(max(n - 1, 1), dtype=MST_EDGE)
    labels = np.empty(n, dtype=np.uint32) if with_labels else None
    hist = np.zeros(self.bits + 1, dtype=np.uint64) if with_hist else None
    keep = rows if n else np.zeros(1, dtype=np.uint64)
    st = VcKnnMstStats()
    self._check(fn(self._h, _p(keep), _p(counts) if counts is not None and n else None, k, kk, flags, max_dist, weight_kind, min_pts, _p(edges),
                   _p(labels) if with_labels and n else None, _p(hist) if with_hist else None, C.byref(st)))
    return edges[:int(st.n_tree)].copy(), labels, hist, st.as_dict()


def _knn_mst_dev(self, fn, d_rows, d_counts, k, kk, flags, max_dist, weight_kind, min_pts, d_edges, d_labels, d_hist, with_stats, stream):
    st = VcKnnMstStats()
    self._check(fn(self._h, d_rows, d_counts, k, kk, flags, max_dist, weight_kind, min_pts, d_edges, d_labels, d_hist, C.byref(st) if with_stats else None, stream))
    return st.as_dict() if with_stats else None


def _mst_cut(self, fn, edges, max_weight):
    """shared by Engine.mst_cut and ShardedEngine.mst_cut: (labels uint32 [N], n_clusters)"""
    n = len(self)
    edges = np.ascontiguousarray(edges, dtype=MST_EDGE).reshape(-1)
    labels = np.empty(n, dtype=np.uint32)
    count = C.c_uint64(0)
    self._check(fn(self._h, _p(edges) if len(edges) else None, len(edges), max_weight, _p(labels) if n else _p(np.zeros(1, dtype=np.uint32)), C.byref(count)))
    return labels, int(count.value)


def _mst_cut_dev(self, fn, d_edges, n_edges, max_weight, d_labels, stream):
    count = C.c_uint64(0)
    self._check(fn(self._h, d_edges, n_edges, max_weight, d_labels, C.byref(count), stream))
    return int(count.value)


def _mst_condense(self, fn, edges, min_cluster_size, root_weight, method, with_node, with_own, with_leave):
    """shared by Engine.mst_condense and ShardedEngine.mst_condense: (nodes CONDENSED_NODE [n_nodes], labels uint32 [N], node [N] | None,
    own [N] | None, leave [N] | None, stats dict)"""
    n = len(self)
    edges = np.ascontiguousarray(edges, dtype=MST_EDGE).reshape(-1)
    nodes = np.zeros(max(n - 1, 1), dtype=CONDENSED_NODE)
    one = np.zeros(1, dtype=np.uint32)
    labels = np.empty(n, dtype=np.uint32)
    node = np.empty(n, dtype=np.uint32) if with_node else None
    own = np.empty(n, dtype=np.uint32) if with_own else None
    leave = np.empty(n, dtype=np.uint32) if with_leave else None
    st = VcMstCondenseStats()
    self._check(fn(self._h, _p(edges) if len(edges) else None, len(edges), min_cluster_size, root_weight, method, _p(nodes), _p(labels if n else one),
                   _p(node) if with_node and n else None, _p(own) if with_own and n else None, _p(leave) if with_leave and n else None, C.byref(st)))
    return nodes[:int(st.n_nodes)].copy(), labels, node, own, leave, st.as_dict()


def _mst_condense_dev(self, fn, d_edges, n_edges, min_cluster_size, root_weight, method, d_nodes, d_labels, d_node, d_own, d_leave, with_stats, stream):
    st = VcMstCondenseStats()
    self._check(fn(self._h, d_edges, n_edges, min_cluster_size, root_weight, method, d_nodes, d_labels, d_node, d_own, d_leave,
                   C.byref(st) if with_stats else None, stream))
    return st.as_dict() if with_stats else None


def _knn_vote(self, fn, rows, counts, kk, labels, weight_kind, max_dist, with_votes):
    """shared by Engine.knn_vote and ShardedEngine.knn_vote: (label uint32 [n_rows], votes [n_rows] | None, total [n_rows] | None, stats dict)"""
    n = len(self)
    rows = np.ascontiguousarray(rows, dtype=np.uint64)
    if rows.ndim != 2:
        raise VcError(VC_ERR_INVALID, "rows must be [n_rows, k]")
    n_rows, k = rows.shape
    if counts is not None:
        counts = np.ascontiguousarray(counts, dtype=np.uint32).reshape(-1)
        if counts.shape[0] != n_rows:
            raise VcError(VC_ERR_INVALID, "counts must have one word per row")
    labels = np.ascontiguousarray(labels, dtype=np.uint32).reshape(-1)
    if labels.shape[0] != n:
        raise VcError(VC_ERR_INVALID, "labels must have one word per resident record")
    out = np.empty(n_rows, dtype=np.uint32)
    votes = np.empty(n_rows, dtype=np.uint32) if with_votes else None
    total = np.empty(n_rows, dtype=np.uint32) if with_votes else None
    one = np.zeros(1, dtype=np.uint64)
    st = VcKnnVoteStats()
    self._check(fn(self._h, _p(rows if rows.size else one), _p(counts) if counts is not None and n_rows else None, n_rows, k, kk, max_dist,
                   _p(labels if n else one), weight_kind, _p(out if n_rows else one), _p(votes) if with_votes and n_rows else None,
                   _p(total) if with_votes and n_rows else None, C.byref(st)))
    return out, votes, total, st.as_dict()


def _knn_vote_dev(self, fn, d_rows, d_counts, n_rows, k, kk, d_labels, weight_kind, max_dist, d_out_label, d_out_votes, d_out_total, with_stats, stream):
    st = VcKnnVoteStats()
    self._check(fn(self._h, d_rows, d_counts, n_rows, k, kk, max_dist, d_labels, weight_kind, d_out_label, d_out_votes, d_out_total,
                   C.byref(st) if with_stats else None, stream))
    return st.as_dict() if with_stats else None


def _label_propagate(self, fn, offsets, adj, labels, weight_kind, flags, max_iters, with_votes):
    """shared by Engine.label_propagate and ShardedEngine.label_propagate: (labels uint32 [N], votes [N] | None, total [N] | None, stats dict)"""
    n = len(self)
    offsets = np.ascontiguousarray(offsets, dtype=np.uint64).reshape(-1)
    adj = np.ascontiguousarray(adj, dtype=np.uint64).reshape(-1)
    labels = np.ascontiguousarray(labels, dtype=np.uint32).reshape(-1)
    if offsets.shape[0] != n + 1 or labels.shape[0] != n:
        raise VcError(VC_ERR_INVALID, "offsets must have N + 1 words and labels N")
    out = np.empty(n, dtype=np.uint32)
    votes = np.empty(n, dtype=np.uint32) if with_votes else None
    total = np.empty(n, dtype=np.uint32) if with_votes else None
    one = np.zeros(1, dtype=np.uint64)
    st = VcLabelPropagateStats()
    self._check(fn(self._h, _p(offsets), _p(adj) if len(adj) else None, len(adj), _p(labels if n else one), weight_kind, flags, max_iters,
                   _p(out if n else one), _p(votes) if with_votes and n else None, _p(total) if with_votes and n else None, C.byref(st)))
    return out, votes, total, st.as_dict()


def _label_propagate_dev(self, fn, d_offsets, d_adj, n_entries, d_labels_in, weight_kind, flags, max_iters, d_labels_out, d_votes, d_total, with_stats, stream):
    st = VcLabelPropagateStats()
    self._check(fn(self._h, d_offsets, d_adj, n_entries, d_labels_in, weight_kind, flags, max_iters, d_labels_out, d_votes, d_total,
                   C.byref(st) if with_stats else None, stream))
    return st.as_dict() if with_stats else None


def _retain(self, fn, sel, kind, with_map):
    """shared by Engine.retain and ShardedEngine.retain: (n_kept, new_ids [N] uint32 | None)"""
    n = len(self)
    sel = np.ascontiguousarray(sel, dtype=np.uint32).reshape(-1)
    if sel.shape[0] != n:
        raise VcError(VC_ERR_INVALID, "the selection must have one word per resident record")
    new_ids = np.empty(n, dtype=np.uint32) if with_map else None
    kept = C.c_uint64(0)
    self._check(fn(self._h, _p(sel) if n else None, kind, _p(new_ids) if with_map and n else None, C.byref(kept)))
    return int(kept.value), new_ids


def _retain_dev(self, fn, d_sel, kind, d_new_ids, stream):
    kept = C.c_uint64(0)
    self._check(fn(self._h, d_sel, kind, d_new_ids, C.byref(kept), stream))
    return int(kept.value)


def split(packed):
    """packed uint64 -> (ids uint32, dists uint32)  (GET_ID / GET_DIST, search_worker.cc:12-13)."""
    packed = np.asarray(packed, dtype=np.uint64)
    return (packed & np.uint64(0xFFFFFFFF)).astype(np.uint32), (packed >> np.uint64(32)).astype(np.uint32)


class Engine:
    """One HBM-resident shard of the code database plus its MIH index (one per GPU/process)."""

    def __init__(self, bits, capacity, n_tables=0, flags=0, id_base=0, device=-1, cand_cap=0, scan_blocks=0,
                 query_tile=0, timing_sample=0):
        self._L = load_library()
        self.bits, self.nbytes, self.n_tables, self.id_base = bits, bits // 8, n_tables, id_base
        cfg = VcConfig(abi_version=VC_ABI_VERSION, bits=bits, n_tables=n_tables, flags=flags, capacity=capacity,
                       id_base=id_base, device=device, cand_cap=cand_cap, scan_blocks=scan_blocks,
                       query_tile=query_tile, timing_sample=timing_sample)
        h = C.c_void_p()
        rc = self._L.vc_create(C.byref(cfg), C.byref(h))
        if rc != VC_OK:
            raise VcError(rc, self._L.vc_last_error(None).decode())
        self._h = h

    # -- plumbing
    def _check(self, rc, ok=(VC_OK,)):
        if rc not in ok:
            raise VcError(rc, self._L.vc_last_error(self._h).decode() or self._L.vc_strerror(rc).decode())
        return rc

    @classmethod
    def borrowed(cls, handle, bits, n_tables=0, id_base=0):
        """a view of an engine somebody else owns (a shard of a ShardedEngine): every call works, close() does not destroy"""
        e = cls.__new__(cls)
        e._L = load_library()
        e.bits, e.nbytes, e.n_tables, e.id_base = bits, bits // 8, n_tables, id_base
        e._h, e._borrowed = handle, True
        return e

    def close(self):
        if getattr(self, "_h", None):
            if not getattr(self, "_borrowed", False):
                self._L.vc_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def _queries(self, q):
        q = np.ascontiguousarray(q, dtype=np.uint8)
        if q.ndim == 1:
            q = q[None, :]
        if q.shape[1] != self.nbytes:
            raise ValueError("query must be %d bytes" % self.nbytes)
        return q

    # -- ingest
    def add_codes(self, codes):
        codes = np.ascontiguousarray(codes, dtype=np.uint8)
        assert codes.ndim == 2 and codes.shape[1] == self.nbytes
        self._check(self._L.vc_add_codes(self._h, _p(codes), codes.shape[0]))

    def add_synthetic(self, n, seed, kind=SYNTH_UNIFORM, n_centres=0, max_flips=0):
        self._check(self._L.vc_add_synthetic(self._h, n, seed, kind, n_centres, max_flips))

    def load_code_file(self, path, max_records=0):
        """headerless records of bits/8 bytes (the reference's BINARY_CODE_FILE); returns records appended"""
        n = C.c_uint64()
        self._check(self._L.vc_load_code_file(self._h, os.fsencode(path), max_records, C.byref(n)))
        return n.value

    def save_code_file(self, path):
        self._check(self._L.vc_save_code_file(self._h, os.fsencode(path)))

    def write_bitmap_file(self, table, path):
        """raw LSB-first uint32 words of one table's occupancy bitmap (generate_bitmap.cc:122-125 format)"""
        self._check(self._L.vc_write_bitmap_file(self._h, table, os.fsencode(path)))

    def read_bitmap_file(self, table, path):
        """checks a generate_bitmap.cc-format file against the index's bitmap; returns the number of differing words
        (0 = the file belongs to this database); raises for unreadable / wrongly sized files"""
        bad = C.c_uint64()
        self._check(self._L.vc_read_bitmap_file(self._h, table, os.fsencode(path), C.byref(bad)), ok=(VC_OK, VC_ERR_STATE))
        return bad.value

    def save_index(self, path):
        self._check(self._L.vc_save_index(self._h, os.fsencode(path)))

    def load_index(self, path):
        self._check(self._L.vc_load_index(self._h, os.fsencode(path)))

    def __len__(self):
        n = C.c_uint64()
        self._check(self._L.vc_size(self._h, C.byref(n)))
        return n.value

    def get_code(self, gid):
        out = np.empty(self.nbytes, dtype=np.uint8)
        rc = self._check(self._L.vc_get_code(self._h, gid, _p(out)), ok=(VC_OK, VC_NOT_FOUND))
        return out if rc == VC_OK else None

    # -- index
    def build_index(self):
        self._check(self._L.vc_build_index(self._h))

    def update_index(self):
        """Merge the records added since the index was built, loaded or last updated into it (a build when there is none)."""
        self._check(self._L.vc_update_index(self._h))

    # -- scan stream
    def build_scan_stream(self):
        """Build the prefix-sorted scan stream of a 128-bit store (vc_build_scan_stream): linear k-NN passes of up to 8
        queries then stream 12 bytes per record instead of 16, results unchanged.  About 20 bytes per record of device memory;
        raises VcError with code VC_ERR_NOMEM when that does not fit.  Every call that changes the store drops it."""
        self._check(self._L.vc_build_scan_stream(self._h))

    def scan_stream_info(self):
        """{built, items, granules, bytes, launches, bound_passes, exact_passes} of the scan stream (all 0 when there is none)"""
        st = VcScanStreamState()
        self._check(self._L.vc_scan_stream_info(self._h, C.byref(st)))
        return st.as_dict()

    def get_bucket(self, table, index, cap=1 << 16, with_codes=True):
        """BaseProxy.get(HashIndex{table,index}) -> (ids, codes) or None (PROXY_NOT_FOUND)."""
        ids = np.empty(cap, dtype=np.uint32)
        codes = np.empty((cap, self.nbytes), dtype=np.uint8) if with_codes else None
        n = C.c_uint32()
        rc = self._check(self._L.vc_get_bucket(self._h, table, index, _p(ids), _p(codes) if with_codes else None, cap,
                                               C.byref(n)), ok=(VC_OK, VC_NOT_FOUND))
        if rc == VC_NOT_FOUND:
            return None
        m = min(n.value, cap)
        return ids[:m].copy(), (codes[:m].copy() if with_codes else None), n.value

    def bitmap_test(self, table, index):
        b = C.c_int()
        self._check(self._L.vc_bitmap_test(self._h, table, index, C.byref(b)))
        return b.value

    def bitmap_read(self, table, word_off, n_words):
        out = np.empty(n_words, dtype=np.uint32)
        self._check(self._L.vc_bitmap_read(self._h, table, word_off, n_words, _p(out)))
        return out

    # -- search
    def search_knn(self, queries, k, mode=MODE_LINEAR, order=ORDER_ASCENDING, with_stats=False, out=None, counts=None):
        """Returns (packed [nq,k] uint64, counts [nq]) (+ list of VcQueryStats).
        out / counts: optional preallocated C-contiguous arrays ([nq,k] uint64, [nq] uint32) to receive the results -- e.g. views
        of page-locked memory (torch.empty(...).pin_memory().numpy()): a large batch then leaves the device in one DMA instead of
        through the library's staging chunks (13 MB of rows per 16 384-query top-100 call)."""
        q = self._queries(queries)
        nq = q.shape[0]
        if out is None:
            out = np.empty((nq, k), dtype=np.uint64)     # (the call writes every row in full, PACK_INF behind counts[i] entries)
        elif out.dtype != np.uint64 or out.shape != (nq, k) or not out.flags.c_contiguous:
            raise ValueError("out must be a C-contiguous [nq, k] uint64 array")
        if counts is None:
            counts = np.zeros(nq, dtype=np.uint32)
        elif counts.dtype != np.uint32 or counts.shape != (nq,) or not counts.flags.c_contiguous:
            raise ValueError("counts must be a C-contiguous [nq] uint32 array")
        stats = (VcQueryStats * nq)() if with_stats else None
        self._check(self._L.vc_search_knn(self._h, _p(q), nq, k, mode, order, _p(out), _p(counts),
                                          C.cast(stats, C.c_void_p) if with_stats else None))
        if with_stats:
            return out, counts, list(stats)
        return out, counts

    def search_knn_dev(self, d_queries, nq, k, d_out, d_counts=None, mode=MODE_LINEAR, stream=None):
        """Device-pointer variant: arguments are raw device addresses (ints), e.g. tensor.data_ptr().
        stream: raw hipStream_t (torch.cuda.current_stream().cuda_stream); None/0 = the null stream, which is
        PyTorch's default stream, so the call is ordered with torch work either way."""
        self._check(self._L.vc_search_knn_dev(self._h, d_queries, nq, k, mode, d_out, d_counts, stream))

    def search_knn_dev_stats(self, d_queries, nq, k, d_out, d_counts, d_stats, mode=MODE_LINEAR, stream=None):
        """vc_search_knn_dev_stats: the same + nq VcQueryStats records written to device memory (d_stats, raw address) in stream order"""
        self._check(self._L.vc_search_knn_dev_stats(self._h, d_queries, nq, k, mode, d_out, d_counts, d_stats, stream))

    # -- queries named by id (image_search_client::search_image_by_id for a batch; the codes never leave HBM)
    def get_codes_dev(self, d_ids, nq, d_codes, d_found=None, stream=None):
        """vc_get_codes_dev on raw device addresses: nq uint32 ids -> nq * bits/8 code bytes (+ nq uint32 found words)"""
        self._check(self._L.vc_get_codes_dev(self._h, d_ids, nq, d_codes, d_found, stream))

    def search_knn_ids(self, ids, k, mode=MODE_LINEAR, order=ORDER_ASCENDING, id_flags=0, with_stats=False):
        """vc_search_knn_ids: numpy ids; returns like search_knn.  An id that is not resident gives count 0 and a PACK_INF row."""
        return _search_knn_ids(self, self._L.vc_search_knn_ids, ids, k, mode, order, id_flags, with_stats)

    def search_knn_ids_dev(self, d_ids, nq, k, d_out, d_counts=None, d_stats=None, mode=MODE_LINEAR, id_flags=0, stream=None):
        """vc_search_knn_ids_dev on raw device addresses; results valid in `stream` order"""
        self._check(self._L.vc_search_knn_ids_dev(self._h, d_ids, nq, k, mode, id_flags, d_out, d_counts, d_stats, stream))

    def search_radius(self, queries, radius, mode=MODE_LINEAR, cap_per_query=4096):
        q = self._queries(queries)
        nq = q.shape[0]
        offs = np.zeros(nq + 1, dtype=np.uint64)
        cap = nq * cap_per_query
        for _ in range(2):
            out = np.empty(max(cap, 1), dtype=np.uint64)
            rc = self._check(self._L.vc_search_radius(self._h, _p(q), nq, radius, mode, _p(out), cap, _p(offs)),
                             ok=(VC_OK, VC_ERR_CAPACITY))
            if rc == VC_OK:
                return [out[int(offs[i]):int(offs[i + 1])].copy() for i in range(nq)]
            cap = int(offs[nq])
        raise VcError(VC_ERR_CAPACITY, "radius search output does not fit")

    def search_radius_dev(self, d_queries, nq, radius, d_out, out_cap, d_offsets, mode=MODE_MIH_EXACT, stream=None):
        """Device-pointer radius search (raw device addresses); returns VC_OK or VC_ERR_CAPACITY (d_offsets[nq] = needed)."""
        return self._check(self._L.vc_search_radius_dev(self._h, d_queries, nq, radius, mode, d_out, out_cap, d_offsets, stream),
                           ok=(VC_OK, VC_ERR_CAPACITY))

    def search_radius_ids(self, ids, radius, mode=MODE_LINEAR, id_flags=0, cap_per_query=4096):
        """vc_search_radius_ids: numpy ids; a list of ascending packed arrays, one per id (empty for an id that is not resident)"""
        return _search_radius_ids(self, self._L.vc_search_radius_ids, ids, radius, mode, id_flags, cap_per_query)

    def search_radius_ids_dev(self, d_ids, nq, radius, d_out, out_cap, d_offsets, mode=MODE_MIH_EXACT, id_flags=0, stream=None):
        """vc_search_radius_ids_dev on raw device addresses, results valid in `stream` order; returns VC_OK or VC_ERR_CAPACITY
        (d_offsets then holds the compacted prefix sums, d_offsets[nq] the total; d_out is untouched)."""
        return self._check(self._L.vc_search_radius_ids_dev(self._h, d_ids, nq, radius, mode, id_flags, d_out, out_cap, d_offsets, stream),
                           ok=(VC_OK, VC_ERR_CAPACITY))

    def retain(self, sel, kind=RETAIN_MASK, with_map=True):
        """vc_retain: the records `sel` selects survive (RETAIN_MASK: sel[i] != 0; RETAIN_ROOTS: sel is a labels array of
        cluster_radius and the groups' representatives survive), renumbered in order; a current index is filtered to them.  Returns
        (n_kept, new_ids): new_ids[i] = the new global id of old record id_base + i or 0xFFFFFFFF (None without with_map)."""
        return _retain(self, self._L.vc_retain, sel, kind, with_map)

    def retain_dev(self, d_sel, kind=RETAIN_MASK, d_new_ids=None, stream=None):
        """vc_retain_dev: d_sel / d_new_ids = raw device addresses of len(self) uint32 (d_new_ids may be None).  Returns n_kept."""
        return _retain_dev(self, self._L.vc_retain_dev, d_sel, kind, d_new_ids, stream)

    def cluster_radius(self, radius, mode=MODE_LINEAR, batch=0, labels=None):
        """vc_cluster_radius: the connected components of the radius graph over all resident records.  Returns (labels, n_pairs,
        n_clusters): labels[i] = the global id of the smallest-id record of the component of record id_base + i.  `labels`: what
        an earlier call at this radius returned for the first len(labels) records alone -- only the records behind them are
        queried (the incremental form, after add_codes + update_index); the result equals a call from scratch."""
        return _cluster_radius(self, self._L.vc_cluster_radius, radius, mode, batch, labels)

    def cluster_radius_dev(self, radius, d_labels, mode=MODE_MIH_EXACT, batch=0, n_labelled=0, stream=None):
        """vc_cluster_radius_dev: d_labels = the raw device address of len(self) uint32, the union-find forest in place (its first n_labelled
        entries come in); labels valid in `stream` order.  Returns (n_pairs, n_clusters)."""
        return _cluster_radius_dev(self, self._L.vc_cluster_radius_dev, radius, d_labels, mode, batch, n_labelled, stream)

    def cluster_levels(self, max_radius, mode=MODE_LINEAR, batch=0, labels=None):
        """vc_cluster_levels: cluster_radius at EVERY radius 0 .. max_radius (< LEVELS_MAX) from one walk of the radius search.
        Returns (labels [max_radius + 1, N], n_pairs, n_clusters): row r equals cluster_radius(r)'s labels, n_clusters[r] its cluster
        count, n_pairs[d] the pairs at distance exactly d (their prefix sums are cluster_radius' n_pairs).  `labels`: the
        [max_radius + 1, n_labelled] rows an earlier call returned for the first n_labelled records alone (the incremental form,
        after add_codes + update_index); the result equals a call from scratch."""
        return _cluster_levels(self, self._L.vc_cluster_levels, max_radius, mode, batch, labels)

    def cluster_levels_dev(self, max_radius, d_labels, mode=MODE_MIH_EXACT, batch=0, n_labelled=0, stream=None):
        """vc_cluster_levels_dev: d_labels = the raw device address of (max_radius + 1) * len(self) uint32, level-major, one
        forest per level in place (of every level the first n_labelled entries come in, at the stride len(self)); labels valid in
        `stream` order.  Returns (n_pairs, n_clusters), max_radius + 1 entries each."""
        return _cluster_levels_dev(self, self._L.vc_cluster_levels_dev, max_radius, d_labels, mode, batch, n_labelled, stream)

    def leaders_radius(self, radius, mode=MODE_LINEAR, batch=0, labels=None):
        """vc_leaders_radius: the greedy one-pass dedup over all resident records in id order.  Returns (labels, n_pairs, n_leaders,
        n_rounds): labels[i] = the record's own global id for a LEADER (no leader with a smaller id within `radius`), else the
        smallest-id leader within `radius`.  `labels`: what an earlier call at this radius returned for the first len(labels)
        records -- they are only read and only the records behind them are queried (the incremental form, after add_codes +
        update_index); the result equals a call from scratch.  retain(labels, RETAIN_ROOTS) keeps exactly the leaders."""
        return _leaders_radius(self, self._L.vc_leaders_radius, radius, mode, batch, labels)

    def leaders_radius_dev(self, radius, d_labels, mode=MODE_MIH_EXACT, batch=0, n_labelled=0, stream=None):
        """vc_leaders_radius_dev: d_labels = the raw device address of len(self) uint32 (its first n_labelled entries come in and are
        only read); labels valid in `stream` order.  Returns (n_pairs, n_leaders, n_rounds)."""
        return _leaders_radius_dev(self, self._L.vc_leaders_radius_dev, radius, d_labels, mode, batch, n_labelled, stream)

    def dbscan_radius(self, radius, min_pts, mode=MODE_LINEAR, batch=0):
        """vc_dbscan_radius: DBSCAN over all resident records.  Returns (labels, degrees, stats): degrees[i] = the records within
        `radius` of record i, itself included; a record is a CORE iff degrees[i] >= min_pts; labels[i] = the smallest global id among
        the cores of a core's component, the label of its smallest-id core neighbour for a BORDER (a non-core record with a core
        within `radius`), the record's own global id for NOISE.  A record labelled with itself is noise iff degrees[i] < min_pts, a
        cluster's representative otherwise.  stats: dict of n_pairs, n_clusters, n_core, n_border, n_noise.  There is no incremental
        form.  retain(labels, RETAIN_ROOTS) keeps one representative per cluster and every noise record."""
        return _dbscan_radius(self, self._L.vc_dbscan_radius, radius, min_pts, mode, batch)

    def dbscan_radius_dev(self, radius, min_pts, d_labels, d_degrees=None, mode=MODE_MIH_EXACT, batch=0, stream=None):
        """vc_dbscan_radius_dev: d_labels / d_degrees = the raw device addresses of len(self) uint32 each (d_degrees None: scratch of
        the handle); both valid in `stream` order.  Returns the stats dict."""
        return _dbscan_radius_dev(self, self._L.vc_dbscan_radius_dev, radius, min_pts, d_labels, d_degrees, mode, batch, stream)

    def dbscan_levels(self, max_radius, min_pts, mode=MODE_LINEAR, batch=0):
        """vc_dbscan_levels: dbscan_radius at EVERY radius 0 .. max_radius (< LEVELS_MAX) from one walk of the radius search.
        Returns (labels [max_radius + 1, N], core_dist [N], stats): row r equals dbscan_radius(r, min_pts)'s labels; core_dist[i] =
        the distance to record i's min_pts-th nearest record, itself counted, or CORE_NEVER if there is none within max_radius --
        record i is a core at level r iff core_dist[i] <= r; stats: dict of n_pairs (the pairs at distance exactly d), n_clusters,
        n_core, n_border, n_noise, max_radius + 1 entries each.  There is no incremental form.  retain(labels[r], RETAIN_ROOTS)
        takes any one level."""
        return _dbscan_levels(self, self._L.vc_dbscan_levels, max_radius, min_pts, mode, batch)

    def dbscan_levels_dev(self, max_radius, min_pts, d_labels, d_core_dist=None, mode=MODE_MIH_EXACT, batch=0, stream=None):
        """vc_dbscan_levels_dev: d_labels = the raw device address of (max_radius + 1) * len(self) uint32, level-major; d_core_dist
        = that of len(self) uint32 (None: scratch of the handle); both valid in `stream` order.  Returns the stats dict."""
        return _dbscan_levels_dev(self, self._L.vc_dbscan_levels_dev, max_radius, min_pts, d_labels, d_core_dist, mode, batch, stream)

    def group_summary(self, labels):
        """vc_group_summary: the groups of equal labels (any of the clustering calls' output, or any partition with values in the resident
        id range) summarised.  Returns (groups, centroids, rep_labels, group_index): groups = structured array GROUP_DTYPE, one entry per
        group by ascending label (label, size, rep, rep_dist, max_dist); centroids = uint8 [G, bits / 8], the per-bit strict-majority
        codes; rep_labels[i] = the representative (the member nearest its group's centroid, the smaller id on a tie) of record i's
        group; group_index[i] = its group's number.  retain(rep_labels, RETAIN_ROOTS) keeps exactly the representatives."""
        return _group_summary(self, self._L.vc_group_summary, labels)

    def group_summary_dev(self, d_labels, groups_cap, d_groups, d_centroids=None, d_rep_labels=None, d_group_index=None, stream=None):
        """vc_group_summary_dev: raw device addresses (None for an output that is not wanted); outputs valid in `stream` order.  Returns
        (rc, G) with rc VC_OK, or VC_ERR_CAPACITY when G > groups_cap (nothing was written)."""
        return _group_summary_dev(self, self._L.vc_group_summary_dev, d_labels, groups_cap, d_groups, d_centroids, d_rep_labels, d_group_index, stream)

    def get_codes(self, ids):
        """the codes of resident ids, uint8 [len(ids), bits / 8]"""
        return _get_codes(self, ids)

    def assign_nearest(self, centres, first=0, count=None):
        """vc_assign_nearest: for the records id_base + first .. + count - 1 (default: to the end) the nearest of the given codes
        (uint8 [K, bits / 8]) as packed uint64, centre index | distance << 32; a tie in distance goes to the smaller index -- row for row
        search_knn(k=1, MODE_LINEAR) of an engine that holds the centres with id_base 0.  first=n_old after add_codes assigns the new records."""
        return _assign_nearest(self, self._L.vc_assign_nearest, centres, first, count)

    def assign_nearest_dev(self, d_centres, n_centres, first, count, d_out, stream=None):
        """vc_assign_nearest_dev: raw device addresses; d_out valid in `stream` order, nothing is waited for"""
        self._check(self._L.vc_assign_nearest_dev(self._h, d_centres, n_centres, first, count, d_out, stream))

    def kmajority(self, k, seed_ids=None, seeds=None, max_iters=KMAJ_MAX_ITERS):
        """vc_kmajority: Hamming k-means over all resident records -- assign to the nearest centre, move each centre to the per-bit
        strict majority of its members, until a round changes nothing or max_iters rounds ran.  Returns (centres, assign, labels, stats):
        assign == assign_nearest(centres), labels = id_base + centre index (an input of group_summary), stats a dict of n_iters,
        converged, n_empty, cost_final and the per-round cost and n_changed.  The seeds are `seeds` (k codes), the codes of `seed_ids`,
        or by default of k ids spread evenly over the store; seed_centres makes better ones on the device."""
        return _kmajority(self, self._L.vc_kmajority, k, seed_ids, seeds, max_iters)

    def kmajority_dev(self, k, d_centres, d_assign, d_labels=None, max_iters=KMAJ_MAX_ITERS, stream=None):
        """vc_kmajority_dev: raw device addresses -- d_centres holds the seeds on entry and the final centres afterwards;
        outputs valid in `stream` order.  Returns the stats dict."""
        return _kmajority_dev(self, self._L.vc_kmajority_dev, k, d_centres, d_assign, d_labels, max_iters, stream)

    def seed_centres(self, k, method=SEED_FARTHEST, seed=0, with_assign=False):
        """vc_seed_centres: k seeds for kmajority made on the device -- SEED_FARTHEST, the farthest-first traversal, or SEED_WEIGHTED, a record
        sampled with probability proportional to its distance to the nearest chosen seed (SplitMix64 from `seed`; the first record is
        draw(0) % N in both).  Returns (centres, picks, assign, stats): picks[t] = id | distance to the seeds before it << 32, assign ==
        assign_nearest(centres) (None unless with_assign), stats a dict of cost, radius, n_zero_picks.  A function of the codes, k, the
        method and `seed` only."""
        return _seed_centres(self, self._L.vc_seed_centres, k, method, seed, with_assign)

    def seed_centres_dev(self, k, d_centres, d_picks=None, d_assign=None, method=SEED_FARTHEST, seed=0, with_stats=True, stream=None):
        """vc_seed_centres_dev: raw device addresses; outputs valid in `stream` order.  Returns the stats dict; with_stats=False returns
        None and the host waits for nothing."""
        return _seed_centres_dev(self, self._L.vc_seed_centres_dev, k, d_centres, d_picks, d_assign, method, seed, with_stats, stream)

    def search_knn_distinct(self, queries, k, labels, mode=MODE_LINEAR, order=ORDER_ASCENDING, k_first=0, with_stats=False):
        """vc_search_knn_distinct: the k nearest label GROUPS of every query, each by its member nearest to the query.  labels: one
        uint32 per resident record as cluster_radius, leaders_radius, dbscan_radius, kmajority or group_summary's group_index write
        them -- only equality matters.  Returns (out [nq, k] uint64, row_labels [nq, k] uint32, counts [nq][, stats dict]); a count
        may carry DISTINCT_TRUNCATED.  mode MODE_LINEAR or MODE_MIH_EXACT; k_first: the first round's k' (0 = min(8192, 2 k)), which
        changes the statistics, never a finished row.  Stages the labels on every call: search_knn_distinct_dev keeps them in HBM."""
        return _search_knn_distinct(self, self._L.vc_search_knn_distinct, queries, k, labels, mode, order, k_first, with_stats)

    def search_knn_distinct_dev(self, d_queries, nq, k, d_labels, d_out, d_row_labels=None, d_counts=None, mode=MODE_LINEAR, k_first=0, with_stats=True,
                                stream=None):
        """vc_search_knn_distinct_dev: raw device addresses; the host waits once per round, results valid in `stream` order.
        Returns the stats dict; with_stats=False returns None."""
        return _search_knn_distinct_dev(self, self._L.vc_search_knn_distinct_dev, d_queries, nq, k, d_labels, d_out, d_row_labels, d_counts, mode, k_first,
                                        with_stats, stream)

    def search_knn_filtered(self, queries, k, sel, kind=FILTER_MASK, value=0, mode=MODE_LINEAR, order=ORDER_ASCENDING, k_first=0, with_stats=False):
        """vc_search_knn_filtered: the k nearest among the records the filter allows, exact for every selectivity.  sel: one uint32 per
        resident record -- FILTER_MASK (nonzero), FILTER_ROOTS (a grouper's labels: the representatives), FILTER_EQUAL / FILTER_NOT_EQUAL
        (against `value`) -- or one bit per record (FILTER_BITS, ceil(N / 32) words).  Returns (out [nq, k] uint64, counts [nq][, stats
        dict]); counts = min(k, allowed).  mode MODE_LINEAR or MODE_MIH_EXACT; k_first: the first post-filter round's k' (0 = the plan's),
        which changes the statistics, never a row.  Stages sel on every call: search_knn_filtered_dev keeps it in HBM."""
        return _search_knn_filtered(self, self._L.vc_search_knn_filtered, queries, k, sel, kind, value, mode, order, k_first, with_stats)

    def search_knn_filtered_dev(self, d_queries, nq, k, d_sel, d_out, d_counts=None, kind=FILTER_MASK, value=0, mode=MODE_LINEAR, k_first=0, with_stats=True,
                                stream=None):
        """vc_search_knn_filtered_dev: raw device addresses; the host waits once for the allowed count and once per post-filter round, results
        valid in `stream` order.  Returns the stats dict; with_stats=False returns None."""
        return _search_knn_filtered_dev(self, self._L.vc_search_knn_filtered_dev, d_queries, nq, k, d_sel, kind, value, d_out, d_counts, mode, k_first, with_stats,
                                        stream)

    def search_knn_scoped(self, queries, k, scope, qscope, order=ORDER_ASCENDING, with_stats=False):
        """vc_search_knn_scoped: for every query the k nearest among the records whose scope word equals the query's own.  scope: one
        uint32 per resident record, qscope: one per query; every value is legal.  Returns (out uint64 [nq, k], counts uint32 [nq][, stats
        dict]); counts = min(k, size of the query's scope).  Exact brute force over the scope, no index.  Stages scope on every call:
        search_knn_scoped_dev keeps it in HBM."""
        return _search_knn_scoped(self, self._L.vc_search_knn_scoped, queries, k, scope, qscope, order, with_stats)

    def search_knn_scoped_dev(self, d_queries, nq, k, d_scope, d_qscope, d_out, d_counts=None, with_stats=True, stream=None):
        """vc_search_knn_scoped_dev: raw device addresses; the host waits twice (the matched count, the segment table), results valid in
        `stream` order.  Returns the stats dict; with_stats=False returns None."""
        return _search_knn_scoped_dev(self, self._L.vc_search_knn_scoped_dev, d_queries, nq, k, d_scope, d_qscope, d_out, d_counts, with_stats, stream)

    def knn_graph(self, k, mode=MODE_LINEAR, batch=0, first=0, count=0, k_first=0, with_stats=False):
        """vc_knn_graph: the exact k-NN graph of the store.  Row p - first holds the k smallest packed (dist << 32 | id) over all resident
        records other than record id_base + p, ascending, UINT64_MAX padded; counts = min(k, N - 1).  The same words in MODE_LINEAR and
        MODE_MIH_EXACT, for every batch and k_first.  count == 0: to the end.  Returns (rows [n, k], counts [n][, stats dict])."""
        return _knn_graph(self, self._L.vc_knn_graph, k, mode, batch, first, count, k_first, with_stats)

    def knn_graph_dev(self, k, d_rows, d_counts=None, mode=MODE_MIH_EXACT, batch=0, first=0, count=0, k_first=0, with_stats=True, stream=None):
        """vc_knn_graph_dev: raw device addresses (d_rows n * k uint64, d_counts n uint32 or None); results valid in `stream`
        order.  Returns the stats dict (None without with_stats)."""
        return _knn_graph_dev(self, self._L.vc_knn_graph_dev, k, d_rows, d_counts, mode, batch, first, count, k_first, with_stats, stream)

    def knn_graph_update(self, rows, counts=None, mode=MODE_LINEAR, batch=0, k_first=0, with_stats=False):
        """vc_knn_graph_update: the graph after an append.  rows [n_old, k] (and counts [n_old] or None) are knn_graph's over the store
        when it held its first n_old records; returns the rows [N, k] and counts [N] (None without counts) of knn_graph over the store
        now, the same words.  In MODE_MIH_EXACT run update_index() first."""
        return _knn_graph_update(self, self._L.vc_knn_graph_update, rows, counts, None, mode, batch, k_first, with_stats)

    def knn_graph_update_dev(self, k, n_old, d_rows, d_counts=None, mode=MODE_MIH_EXACT, batch=0, k_first=0, with_stats=True, stream=None):
        """vc_knn_graph_update_dev: raw device addresses (d_rows N * k uint64 whose first n_old rows are the graph as it was, d_counts
        N uint32 or None); results valid in `stream` order.  Returns the stats dict (or None)."""
        return _knn_graph_update_dev(self, self._L.vc_knn_graph_update_dev, k, n_old, d_rows, d_counts, mode, batch, k_first, with_stats, stream)

    def knn_graph_retain(self, rows, new_ids, counts=None, mode=MODE_LINEAR, batch=0, k_first=0, with_stats=False):
        """vc_knn_graph_retain: the graph after a removal.  rows [n_old, k] (and counts [n_old] or None) are knn_graph's over the store
        before retain(), new_ids the map retain() returned; returns the rows [K, k] and counts [K] (None without counts) of knn_graph
        over the store now, the same words.  Only the rows that lost too many entries are searched again."""
        return _knn_graph_retain(self, self._L.vc_knn_graph_retain, rows, new_ids, counts, mode, batch, k_first, with_stats)

    def knn_graph_retain_dev(self, k, n_old, d_new_ids, d_rows, d_counts=None, mode=MODE_MIH_EXACT, batch=0, k_first=0, with_stats=True, stream=None):
        """vc_knn_graph_retain_dev: raw device addresses (d_new_ids n_old uint32 as retain_dev wrote it, d_rows n_old * k uint64 and
        d_counts n_old uint32 or None, the graph as it was); results valid in `stream` order.  Returns the stats dict (or None)."""
        return _knn_graph_retain_dev(self, self._L.vc_knn_graph_retain_dev, k, n_old, d_new_ids, d_rows, d_counts, mode, batch, k_first, with_stats, stream)

    def cluster_knn(self, rows, counts, kk, flags=KNN_MUTUAL, max_dist=0xFFFFFFFF, with_in_degree=True):
        """vc_cluster_knn: components and in-degrees of a graph knn_graph built over the whole store (rows [N, k], counts [N] or None).
        Row i lists j iff j is among its first kk entries at a distance <= max_dist; KNN_MUTUAL joins i and j iff each lists the other,
        KNN_EITHER iff one does.  Returns (labels [N] -- the smallest id of each component, as cluster_radius --, in_degree [N] | None,
        stats dict of n_edges, n_mutual, n_clusters, max_in_degree)."""
        return _cluster_knn(self, self._L.vc_cluster_knn, rows, counts, kk, flags, max_dist, with_in_degree)

    def cluster_knn_dev(self, d_rows, d_counts, k, kk, d_labels, d_in_degree=None, flags=KNN_MUTUAL, max_dist=0xFFFFFFFF, with_stats=True, stream=None):
        """vc_cluster_knn_dev: raw device addresses; nothing is searched, the host waits once.  Returns the stats dict (None without
        with_stats)."""
        return _cluster_knn_dev(self, self._L.vc_cluster_knn_dev, d_rows, d_counts, k, kk, flags, max_dist, d_labels, d_in_degree, with_stats, stream)

    def cluster_snn(self, rows, counts, kk, min_shared, flags=KNN_MUTUAL, max_dist=0xFFFFFFFF, with_shared=True, with_hist=True):
        """vc_cluster_snn: shared-nearest-neighbour clusters of a graph knn_graph built over the whole store (rows [N, k], counts [N] or None).
        "Lists" and the candidate pairs are cluster_knn's; a candidate pair is joined iff the two lists of kk share at least min_shared
        records.  Returns (labels [N], shared [N, kk] | None -- the weight of every listed entry, SNN_NONE elsewhere --, hist [kk] | None
        -- the listed entries by weight --, stats dict of n_edges, n_mutual, n_joined, n_clusters, max_shared)."""
        return _cluster_snn(self, self._L.vc_cluster_snn, rows, counts, kk, min_shared, flags, max_dist, with_shared, with_hist)

    def cluster_snn_dev(self, d_rows, d_counts, k, kk, min_shared, d_labels, d_shared=None, d_hist=None, flags=KNN_MUTUAL, max_dist=0xFFFFFFFF, with_stats=True,
                        stream=None):
        """vc_cluster_snn_dev: raw device addresses; nothing is searched, the host waits once.  Returns the stats dict (None without
        with_stats)."""
        return _cluster_snn_dev(self, self._L.vc_cluster_snn_dev, d_rows, d_counts, k, kk, min_shared, flags, max_dist, d_labels, d_shared, d_hist, with_stats, stream)

    def knn_adjacency(self, rows, counts, kk, flags=KNN_REVERSE, max_dist=0xFFFFFFFF):
        """vc_knn_adjacency: the reverse (KNN_REVERSE: who lists j), mutual (KNN_MUTUAL) or symmetrised (KNN_EITHER) graph of a graph
        knn_graph built over the whole store (rows [N, k], counts [N] or None), in CSR form; "lists" is cluster_knn's.  Returns
        (offsets [N + 1], adj [T], stats dict of n_edges, n_entries, n_empty, max_degree): segment j is adj[offsets[j]:offsets[j + 1]],
        packed dist << 32 | id, ascending."""
        return _knn_adjacency(self, self._L.vc_knn_adjacency, rows, counts, kk, flags, max_dist)

    def knn_adjacency_dev(self, d_rows, d_counts, k, kk, d_adj, adj_cap, d_offsets, flags=KNN_REVERSE, max_dist=0xFFFFFFFF, with_stats=True, stream=None):
        """vc_knn_adjacency_dev: raw device addresses; nothing is searched, the host waits once.  Returns (rc, stats dict | None): rc is
        VC_OK, or VC_ERR_CAPACITY when T > adj_cap (d_offsets and the stats are filled, d_adj is untouched; adj_cap = 0 with d_adj None
        is the sizing call)."""
        return _knn_adjacency_dev(self, self._L.vc_knn_adjacency_dev, d_rows, d_counts, k, kk, flags, max_dist, d_adj, adj_cap, d_offsets, with_stats, stream)

    def knn_mst(self, rows, counts, kk, flags=KNN_MUTUAL, max_dist=0xFFFFFFFF, weight_kind=MST_DISTANCE, min_pts=1, with_labels=True, with_hist=True):
        """vc_knn_mst: the minimum spanning forest, in Kruskal order, of the mutual (KNN_MUTUAL) or symmetrised (KNN_EITHER) graph of a
        graph knn_graph built over the whole store (rows [N, k], counts [N] or None); "lists" is cluster_knn's.  weight_kind
        MST_DISTANCE weighs an edge by its distance, MST_REACHABILITY by max(distance, the two core distances at min_pts).  Returns
        (edges MST_EDGE [M] ascending in (weight, a, dist, b), labels [N] | None, hist [bits + 1] | None, stats dict of n_edges,
        n_graph_edges, n_tree, n_clusters, total_weight, max_weight, n_rounds)."""
        return _knn_mst(self, self._L.vc_knn_mst, rows, counts, kk, flags, max_dist, weight_kind, min_pts, with_labels, with_hist)

    def knn_mst_dev(self, d_rows, d_counts, k, kk, d_edges, d_labels=None, d_hist=None, flags=KNN_MUTUAL, max_dist=0xFFFFFFFF, weight_kind=MST_DISTANCE,
                    min_pts=1, with_stats=True, stream=None):
        """vc_knn_mst_dev: raw device addresses; d_edges has room for max(N, 1) - 1 vc_mst_edge; nothing is searched, the host
        waits once per Boruvka round and once at the end.  Returns the stats dict (None without with_stats)."""
        return _knn_mst_dev(self, self._L.vc_knn_mst_dev, d_rows, d_counts, k, kk, flags, max_dist, weight_kind, min_pts, d_edges, d_labels, d_hist, with_stats,
                            stream)

    def mst_cut(self, edges, max_weight):
        """vc_mst_cut: the components of the store under the edges (MST_EDGE records, any order) of weight <= max_weight.  Returns
        (labels [N] -- the smallest id of each component --, n_clusters)."""
        return _mst_cut(self, self._L.vc_mst_cut, edges, max_weight)

    def mst_cut_dev(self, d_edges, n_edges, max_weight, d_labels, stream=None):
        """vc_mst_cut_dev: raw device addresses; the host waits once.  Returns n_clusters."""
        return _mst_cut_dev(self, self._L.vc_mst_cut_dev, d_edges, n_edges, max_weight, d_labels, stream)

    def mst_condense(self, edges, min_cluster_size, root_weight=0, method=CONDENSE_EOM, with_node=True, with_own=True, with_leave=True):
        """vc_mst_condense: the HDBSCAN-style clusters of a spanning forest (MST_EDGE records ascending in weight, as knn_mst returns them,
        best under MST_REACHABILITY): the condensed tree at min_cluster_size, the integer stability of every node, the excess-of-mass
        (CONDENSE_EOM) or leaf (CONDENSE_LEAF) selection and the flat labels.  root_weight 0 never selects a whole component of the forest;
        otherwise it is the height, above every edge, at which the components are deemed to merge.  Returns (nodes CONDENSED_NODE [n_nodes]
        ascending in (form, rep), labels [N] -- rep of the record's selected cluster, its own id for noise --, node [N] | None -- that
        cluster's index, CONDENSE_NONE for noise --, own [N] | None, leave [N] | None, stats dict of n_nodes, n_leaves, n_roots, n_selected,
        n_clustered, n_noise, total_stability, n_levels)."""
        return _mst_condense(self, self._L.vc_mst_condense, edges, min_cluster_size, root_weight, method, with_node, with_own, with_leave)

    def mst_condense_dev(self, d_edges, n_edges, min_cluster_size, d_nodes, d_labels, d_node=None, d_own=None, d_leave=None, root_weight=0, method=CONDENSE_EOM,
                         with_stats=True, stream=None):
        """vc_mst_condense_dev: raw device addresses; d_nodes has room for max(N, 1) - 1 vc_condensed_node; the host waits three times for a
        few words.  Returns the stats dict (n_nodes says how many nodes were written) or None."""
        return _mst_condense_dev(self, self._L.vc_mst_condense_dev, d_edges, n_edges, min_cluster_size, root_weight, method, d_nodes, d_labels, d_node, d_own,
                                 d_leave, with_stats, stream)

    def knn_vote(self, rows, counts, kk, labels, weight_kind=VOTE_COUNT, max_dist=0xFFFFFFFF, with_votes=True):
        """vc_knn_vote: the k-NN classifier over any rows [n_rows, k] whose ids are resident (counts [n_rows] or None: min(k, N) entries
        each) -- a graph of knn_graph or the rows of a search.  Row r's label is the winner among its first min(kk, count) entries
        within max_dist under labels [N] (VOTE_NONE does not vote): the larger tally (VOTE_COUNT: 1 an entry, VOTE_CLOSENESS:
        bits + 1 - distance), ties to the label met first.  Returns (label [n_rows], votes | None, total | None, stats dict of
        n_voted, n_unlabelled, n_ties, n_entries)."""
        return _knn_vote(self, self._L.vc_knn_vote, rows, counts, kk, labels, weight_kind, max_dist, with_votes)

    def knn_vote_dev(self, d_rows, d_counts, n_rows, k, kk, d_labels, d_out_label, d_out_votes=None, d_out_total=None, weight_kind=VOTE_COUNT,
                     max_dist=0xFFFFFFFF, with_stats=True, stream=None):
        """vc_knn_vote_dev: raw device addresses; one launch and one wait.  Returns the stats dict (None without with_stats)."""
        return _knn_vote_dev(self, self._L.vc_knn_vote_dev, d_rows, d_counts, n_rows, k, kk, d_labels, weight_kind, max_dist, d_out_label, d_out_votes,
                             d_out_total, with_stats, stream)

    def label_propagate(self, offsets, adj, labels, weight_kind=VOTE_COUNT, flags=0, max_iters=LP_MAX_ITERS, with_votes=True):
        """vc_label_propagate: synchronous label propagation over the CSR (offsets [N + 1], adj) of knn_adjacency from labels [N]:
        every round each record takes the winner of its segment under the previous round's labels (the larger tally, then its
        current label, then the label met first) or keeps its label when nothing votes; LP_CLAMP_SEEDS keeps every labelled record
        of `labels` fixed (semi-supervised), labels = id_base + arange(N) without it is community detection.  Stops after the first
        round without a change or after max_iters <= LP_MAX_ITERS.  Returns (labels [N], votes | None, total | None of the last round,
        stats dict of n_iters, converged, n_changed_last, n_labelled, n_ties_last)."""
        return _label_propagate(self, self._L.vc_label_propagate, offsets, adj, labels, weight_kind, flags, max_iters, with_votes)

    def label_propagate_dev(self, d_offsets, d_adj, n_entries, d_labels_in, d_labels_out, d_votes=None, d_total=None, weight_kind=VOTE_COUNT, flags=0,
                            max_iters=LP_MAX_ITERS, with_stats=True, stream=None):
        """vc_label_propagate_dev: raw device addresses; one wait for the plan and one small read-back per round.  Returns the
        stats dict (None without with_stats)."""
        return _label_propagate_dev(self, self._L.vc_label_propagate_dev, d_offsets, d_adj, n_entries, d_labels_in, weight_kind, flags, max_iters,
                                    d_labels_out, d_votes, d_total, with_stats, stream)

    def timing(self):
        t = VcTiming()
        self._check(self._L.vc_get_timing(self._h, C.byref(t)))
        return t

    def device_status(self):
        """calls since the last query whose device-side ring-overflow recovery gave up (0 in normal operation)"""
        n = C.c_uint32()
        self._check(self._L.vc_device_status(self._h, C.byref(n)))
        return n.value

    def set_stream(self, stream):
        self._check(self._L.vc_set_stream(self._h, stream))


def merge_topk_dev(d_lists, n_lists, nq, k, d_out, d_counts=None, stream=None):
    """vc_merge_topk_dev on raw device addresses (replaces gather_vectors + master heap)."""
    L = load_library()
    rc = L.vc_merge_topk_dev(d_lists, n_lists, nq, k, d_out, d_counts, stream)
    if rc != VC_OK:
        raise VcError(rc, L.vc_last_error(None).decode())


class ShardedEngine:
    """The vc_sharded_* family: one process, the database split by id range over `n_shards` engines on `devices`
    (replaces mpirun ranks + MPI gathers + the master heap, search_worker.cc:99-101,177-207)."""

    def __init__(self, bits, capacity, n_shards, n_tables=0, devices=None, exchange=EXCHANGE_AUTO, flags=0, id_base=0,
                 cand_cap=0, query_tile=0, timing_sample=0):
        self._L = load_library()
        self.bits, self.nbytes, self.n_shards, self.n_tables = bits, bits // 8, n_shards, n_tables
        self.id_base = id_base
        cfg = VcShardedConfig(abi_version=VC_ABI_VERSION, n_shards=n_shards, n_devices=len(devices or []), exchange=exchange)
        for i, d in enumerate(devices or []):
            cfg.device_ids[i] = d
        cfg.engine = VcConfig(abi_version=VC_ABI_VERSION, bits=bits, n_tables=n_tables, flags=flags, capacity=capacity,
                              id_base=id_base, device=-1, cand_cap=cand_cap, query_tile=query_tile, timing_sample=timing_sample)
        h = C.c_void_p()
        rc = self._L.vc_sharded_create(C.byref(cfg), C.byref(h))
        if rc != VC_OK:
            raise VcError(rc, self._L.vc_sharded_last_error(None).decode())
        self._h = h

    def _check(self, rc, ok=(VC_OK,)):
        if rc not in ok:
            raise VcError(rc, self._L.vc_sharded_last_error(self._h).decode() or self._L.vc_strerror(rc).decode())
        return rc

    def close(self):
        if getattr(self, "_h", None):
            self._L.vc_sharded_destroy(self._h)
            self._h = None

    __del__ = close

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    @property
    def exchange(self):
        k = C.c_uint32()
        self._check(self._L.vc_sharded_exchange(self._h, C.byref(k)))
        return k.value

    def add_codes(self, codes):
        codes = np.ascontiguousarray(codes, dtype=np.uint8)
        self._check(self._L.vc_sharded_add_codes(self._h, _p(codes), codes.shape[0]))

    def add_synthetic(self, n, seed, kind=SYNTH_UNIFORM, n_centres=0, max_flips=0):
        self._check(self._L.vc_sharded_add_synthetic(self._h, n, seed, kind, n_centres, max_flips))

    def __len__(self):
        n = C.c_uint64()
        self._check(self._L.vc_sharded_size(self._h, C.byref(n)))
        return n.value

    def build_index(self):
        self._check(self._L.vc_sharded_build_index(self._h))

    def update_index(self):
        """Engine.update_index on every non-empty shard (shards the appended ids did not reach have nothing to do)."""
        self._check(self._L.vc_sharded_update_index(self._h))

    def get_code(self, gid):
        out = np.empty(self.nbytes, dtype=np.uint8)
        rc = self._check(self._L.vc_sharded_get_code(self._h, gid, _p(out)), ok=(VC_OK, VC_NOT_FOUND))
        return out if rc == VC_OK else None

    def get_bucket(self, table, index, cap=1 << 16):
        ids = np.empty(cap, dtype=np.uint32)
        codes = np.empty((cap, self.nbytes), dtype=np.uint8)
        n = C.c_uint32()
        rc = self._check(self._L.vc_sharded_get_bucket(self._h, table, index, _p(ids), _p(codes), cap, C.byref(n)),
                         ok=(VC_OK, VC_NOT_FOUND))
        if rc == VC_NOT_FOUND:
            return None
        m = min(n.value, cap)
        return ids[:m].copy(), codes[:m].copy(), n.value

    def shard_range(self, g):
        first, cnt = C.c_uint64(), C.c_uint64()
        self._check(self._L.vc_sharded_shard(self._h, g, None, C.byref(first), C.byref(cnt)))
        return first.value, cnt.value

    def shard(self, g):
        """shard g's engine, borrowed (timing, bucket views, files); valid while this store lives"""
        e, first = C.c_void_p(), C.c_uint64()
        self._check(self._L.vc_sharded_shard(self._h, g, C.byref(e), C.byref(first), None))
        return Engine.borrowed(e, self.bits, self.n_tables, first.value)

    @property
    def root_device(self):
        d = C.c_int()
        self._check(self._L.vc_sharded_root_device(self._h, C.byref(d)))
        return d.value

    def search_knn_dev(self, d_queries, nq, k, d_out, d_counts=None, d_stats=None, mode=MODE_LINEAR, stream=None):
        """vc_sharded_search_knn_dev: raw device addresses on the root device; results valid in `stream` order"""
        self._check(self._L.vc_sharded_search_knn_dev(self._h, d_queries, nq, k, mode, d_out, d_counts, d_stats, stream))

    # -- queries named by id, over all shards (device addresses on the root device)
    def get_codes_dev(self, d_ids, nq, d_codes, d_found=None, stream=None):
        """vc_sharded_get_codes_dev: nq uint32 global ids -> nq * bits/8 code bytes (+ nq uint32 found words) on the root device"""
        self._check(self._L.vc_sharded_get_codes_dev(self._h, d_ids, nq, d_codes, d_found, stream))

    def search_knn_ids(self, ids, k, mode=MODE_LINEAR, order=ORDER_ASCENDING, id_flags=0, with_stats=False):
        """vc_sharded_search_knn_ids: numpy ids; returns like search_knn"""
        return _search_knn_ids(self, self._L.vc_sharded_search_knn_ids, ids, k, mode, order, id_flags, with_stats)

    def search_knn_ids_dev(self, d_ids, nq, k, d_out, d_counts=None, d_stats=None, mode=MODE_LINEAR, id_flags=0, stream=None):
        """vc_sharded_search_knn_ids_dev: raw device addresses on the root device; results valid in `stream` order"""
        self._check(self._L.vc_sharded_search_knn_ids_dev(self._h, d_ids, nq, k, mode, id_flags, d_out, d_counts, d_stats, stream))

    def search_radius(self, queries, radius, mode=MODE_LINEAR, cap_per_query=64):
        """vc_sharded_search_radius: list of ascending packed arrays, one per query"""
        q = np.ascontiguousarray(queries, dtype=np.uint8)
        if q.ndim == 1:
            q = q[None, :]
        nq = q.shape[0]
        offs = np.zeros(nq + 1, dtype=np.uint64)
        cap = nq * cap_per_query
        for _ in range(2):
            out = np.empty(max(cap, 1), dtype=np.uint64)
            rc = self._check(self._L.vc_sharded_search_radius(self._h, _p(q), nq, radius, mode, _p(out), cap, _p(offs)),
                             ok=(VC_OK, VC_ERR_CAPACITY))
            if rc == VC_OK:
                return [out[int(offs[i]):int(offs[i + 1])].copy() for i in range(nq)]
            cap = int(offs[nq])
        raise VcError(VC_ERR_CAPACITY, "radius search output does not fit")

    def search_radius_dev(self, d_queries, nq, radius, d_out, out_cap, d_offsets, mode=MODE_MIH_EXACT, stream=None):
        """vc_sharded_search_radius_dev: raw device addresses on the root device, results valid in `stream` order; returns VC_OK
        or VC_ERR_CAPACITY (d_offsets then holds the needed counts, d_offsets[nq] the total; d_out is untouched)."""
        return self._check(self._L.vc_sharded_search_radius_dev(self._h, d_queries, nq, radius, mode, d_out, out_cap, d_offsets, stream),
                           ok=(VC_OK, VC_ERR_CAPACITY))

    def search_radius_ids(self, ids, radius, mode=MODE_LINEAR, id_flags=0, cap_per_query=64):
        """vc_sharded_search_radius_ids: numpy global ids; a list of ascending packed arrays, one per id"""
        return _search_radius_ids(self, self._L.vc_sharded_search_radius_ids, ids, radius, mode, id_flags, cap_per_query)

    def search_radius_ids_dev(self, d_ids, nq, radius, d_out, out_cap, d_offsets, mode=MODE_MIH_EXACT, id_flags=0, stream=None):
        """vc_sharded_search_radius_ids_dev: raw device addresses on the root device, results valid in `stream` order; returns VC_OK
        or VC_ERR_CAPACITY (d_offsets then holds the compacted prefix sums, d_offsets[nq] the total; d_out is untouched)."""
        return self._check(self._L.vc_sharded_search_radius_ids_dev(self._h, d_ids, nq, radius, mode, id_flags, d_out, out_cap, d_offsets,
                                                                    stream), ok=(VC_OK, VC_ERR_CAPACITY))

    def retain(self, sel, kind=RETAIN_MASK, with_map=True):
        """vc_sharded_retain: the records `sel` selects survive (RETAIN_MASK: sel[i] != 0; RETAIN_ROOTS: sel is a labels array of
        cluster_radius and the groups' representatives survive), renumbered in order; a current index is filtered to them.  Returns
        (n_kept, new_ids): new_ids[i] = the new global id of old record id_base + i or 0xFFFFFFFF (None without with_map)."""
        return _retain(self, self._L.vc_sharded_retain, sel, kind, with_map)

    def retain_dev(self, d_sel, kind=RETAIN_MASK, d_new_ids=None, stream=None):
        """vc_sharded_retain_dev: d_sel / d_new_ids = raw device addresses of len(self) uint32 on the root device (d_new_ids may be None).  Returns n_kept."""
        return _retain_dev(self, self._L.vc_sharded_retain_dev, d_sel, kind, d_new_ids, stream)

    def cluster_radius(self, radius, mode=MODE_LINEAR, batch=0, labels=None):
        """vc_sharded_cluster_radius: the connected components of the radius graph over all resident records.  Returns (labels, n_pairs,
        n_clusters): labels[i] = the global id of the smallest-id record of the component of record id_base + i.  `labels`: what
        an earlier call at this radius returned for the first len(labels) records alone -- only the records behind them are
        queried (the incremental form, after add_codes + update_index); the result equals a call from scratch."""
        return _cluster_radius(self, self._L.vc_sharded_cluster_radius, radius, mode, batch, labels)

    def cluster_radius_dev(self, radius, d_labels, mode=MODE_MIH_EXACT, batch=0, n_labelled=0, stream=None):
        """vc_sharded_cluster_radius_dev: d_labels = the raw device address of len(self) uint32 on the root device, the union-find forest in place (its first n_labelled
        entries come in); labels valid in `stream` order.  Returns (n_pairs, n_clusters)."""
        return _cluster_radius_dev(self, self._L.vc_sharded_cluster_radius_dev, radius, d_labels, mode, batch, n_labelled, stream)

    def cluster_levels(self, max_radius, mode=MODE_LINEAR, batch=0, labels=None):
        """vc_sharded_cluster_levels: cluster_radius at EVERY radius 0 .. max_radius (< LEVELS_MAX) from one walk of the radius search.
        Returns (labels [max_radius + 1, N], n_pairs, n_clusters): row r equals cluster_radius(r)'s labels, n_clusters[r] its cluster
        count, n_pairs[d] the pairs at distance exactly d (their prefix sums are cluster_radius' n_pairs).  `labels`: the
        [max_radius + 1, n_labelled] rows an earlier call returned for the first n_labelled records alone (the incremental form,
        after add_codes + update_index); the result equals a call from scratch."""
        return _cluster_levels(self, self._L.vc_sharded_cluster_levels, max_radius, mode, batch, labels)

    def cluster_levels_dev(self, max_radius, d_labels, mode=MODE_MIH_EXACT, batch=0, n_labelled=0, stream=None):
        """vc_sharded_cluster_levels_dev: d_labels = the raw device address of (max_radius + 1) * len(self) uint32 on the root device, level-major, one
        forest per level in place (of every level the first n_labelled entries come in, at the stride len(self)); labels valid in
        `stream` order.  Returns (n_pairs, n_clusters), max_radius + 1 entries each."""
        return _cluster_levels_dev(self, self._L.vc_sharded_cluster_levels_dev, max_radius, d_labels, mode, batch, n_labelled, stream)

    def leaders_radius(self, radius, mode=MODE_LINEAR, batch=0, labels=None):
        """vc_sharded_leaders_radius: the greedy one-pass dedup over all resident records in id order.  Returns (labels, n_pairs, n_leaders,
        n_rounds): labels[i] = the record's own global id for a LEADER (no leader with a smaller id within `radius`), else the
        smallest-id leader within `radius`.  `labels`: what an earlier call at this radius returned for the first len(labels)
        records -- they are only read and only the records behind them are queried (the incremental form, after add_codes +
        update_index); the result equals a call from scratch.  retain(labels, RETAIN_ROOTS) keeps exactly the leaders."""
        return _leaders_radius(self, self._L.vc_sharded_leaders_radius, radius, mode, batch, labels)

    def leaders_radius_dev(self, radius, d_labels, mode=MODE_MIH_EXACT, batch=0, n_labelled=0, stream=None):
        """vc_sharded_leaders_radius_dev: d_labels = the raw device address of len(self) uint32 on the root device (its first n_labelled entries come in and are
        only read); labels valid in `stream` order.  Returns (n_pairs, n_leaders, n_rounds)."""
        return _leaders_radius_dev(self, self._L.vc_sharded_leaders_radius_dev, radius, d_labels, mode, batch, n_labelled, stream)

    def dbscan_radius(self, radius, min_pts, mode=MODE_LINEAR, batch=0):
        """vc_sharded_dbscan_radius: DBSCAN over all resident records.  Returns (labels, degrees, stats): degrees[i] = the records within
        `radius` of record i, itself included; a record is a CORE iff degrees[i] >= min_pts; labels[i] = the smallest global id among
        the cores of a core's component, the label of its smallest-id core neighbour for a BORDER (a non-core record with a core
        within `radius`), the record's own global id for NOISE.  A record labelled with itself is noise iff degrees[i] < min_pts, a
        cluster's representative otherwise.  stats: dict of n_pairs, n_clusters, n_core, n_border, n_noise.  There is no incremental
        form.  retain(labels, RETAIN_ROOTS) keeps one representative per cluster and every noise record."""
        return _dbscan_radius(self, self._L.vc_sharded_dbscan_radius, radius, min_pts, mode, batch)

    def dbscan_radius_dev(self, radius, min_pts, d_labels, d_degrees=None, mode=MODE_MIH_EXACT, batch=0, stream=None):
        """vc_sharded_dbscan_radius_dev: d_labels / d_degrees = the raw device addresses of len(self) uint32 each on the root device (d_degrees None: scratch of
        the handle); both valid in `stream` order.  Returns the stats dict."""
        return _dbscan_radius_dev(self, self._L.vc_sharded_dbscan_radius_dev, radius, min_pts, d_labels, d_degrees, mode, batch, stream)

    def dbscan_levels(self, max_radius, min_pts, mode=MODE_LINEAR, batch=0):
        """vc_sharded_dbscan_levels: dbscan_radius at EVERY radius 0 .. max_radius (< LEVELS_MAX) from one walk of the radius search.
        Returns (labels [max_radius + 1, N], core_dist [N], stats): row r equals dbscan_radius(r, min_pts)'s labels; core_dist[i] =
        the distance to record i's min_pts-th nearest record, itself counted, or CORE_NEVER if there is none within max_radius --
        record i is a core at level r iff core_dist[i] <= r; stats: dict of n_pairs (the pairs at distance exactly d), n_clusters,
        n_core, n_border, n_noise, max_radius + 1 entries each.  There is no incremental form.  retain(labels[r], RETAIN_ROOTS)
        takes any one level."""
        return _dbscan_levels(self, self._L.vc_sharded_dbscan_levels, max_radius, min_pts, mode, batch)

    def dbscan_levels_dev(self, max_radius, min_pts, d_labels, d_core_dist=None, mode=MODE_MIH_EXACT, batch=0, stream=None):
        """vc_sharded_dbscan_levels_dev: d_labels = the raw device address of (max_radius + 1) * len(self) uint32 on the root device, level-major; d_core_dist
        = that of len(self) uint32 (None: scratch of the handle); both valid in `stream` order.  Returns the stats dict."""
        return _dbscan_levels_dev(self, self._L.vc_sharded_dbscan_levels_dev, max_radius, min_pts, d_labels, d_core_dist, mode, batch, stream)

    def group_summary(self, labels):
        """vc_sharded_group_summary: the groups of equal labels (any of the clustering calls' output, or any partition with values in the resident
        id range) summarised.  Returns (groups, centroids, rep_labels, group_index): groups = structured array GROUP_DTYPE, one entry per
        group by ascending label (label, size, rep, rep_dist, max_dist); centroids = uint8 [G, bits / 8], the per-bit strict-majority
        codes; rep_labels[i] = the representative (the member nearest its group's centroid, the smaller id on a tie) of record i's
        group; group_index[i] = its group's number.  retain(rep_labels, RETAIN_ROOTS) keeps exactly the representatives."""
        return _group_summary(self, self._L.vc_sharded_group_summary, labels)

    def group_summary_dev(self, d_labels, groups_cap, d_groups, d_centroids=None, d_rep_labels=None, d_group_index=None, stream=None):
        """vc_sharded_group_summary_dev: raw device addresses on the root device (None for an output that is not wanted); outputs valid in
        `stream` order.  Returns (rc, G) with rc VC_OK, or VC_ERR_CAPACITY when G > groups_cap (nothing was written)."""
        return _group_summary_dev(self, self._L.vc_sharded_group_summary_dev, d_labels, groups_cap, d_groups, d_centroids, d_rep_labels, d_group_index, stream)

    def get_codes(self, ids):
        """the codes of resident ids, uint8 [len(ids), bits / 8]"""
        return _get_codes(self, ids)

    def assign_nearest(self, centres, first=0, count=None):
        """vc_sharded_assign_nearest: for the records id_base + first .. + count - 1 (default: to the end) the nearest of the given codes
        (uint8 [K, bits / 8]) as packed uint64, centre index | distance << 32; a tie in distance goes to the smaller index -- row for row
        search_knn(k=1, MODE_LINEAR) of an engine that holds the centres with id_base 0.  first=n_old after add_codes assigns the new records."""
        return _assign_nearest(self, self._L.vc_sharded_assign_nearest, centres, first, count)

    def assign_nearest_dev(self, d_centres, n_centres, first, count, d_out, stream=None):
        """vc_sharded_assign_nearest_dev: raw device addresses on the root device; d_out valid in `stream` order, nothing is waited for"""
        self._check(self._L.vc_sharded_assign_nearest_dev(self._h, d_centres, n_centres, first, count, d_out, stream))

    def kmajority(self, k, seed_ids=None, seeds=None, max_iters=KMAJ_MAX_ITERS):
        """vc_sharded_kmajority: Hamming k-means over all resident records -- assign to the nearest centre, move each centre to the per-bit
        strict majority of its members, until a round changes nothing or max_iters rounds ran.  Returns (centres, assign, labels, stats):
        assign == assign_nearest(centres), labels = id_base + centre index (an input of group_summary), stats a dict of n_iters,
        converged, n_empty, cost_final and the per-round cost and n_changed.  The seeds are `seeds` (k codes), the codes of `seed_ids`,
        or by default of k ids spread evenly over the store; seed_centres makes better ones on the device."""
        return _kmajority(self, self._L.vc_sharded_kmajority, k, seed_ids, seeds, max_iters)

    def kmajority_dev(self, k, d_centres, d_assign, d_labels=None, max_iters=KMAJ_MAX_ITERS, stream=None):
        """vc_sharded_kmajority_dev: raw device addresses on the root device -- d_centres holds the seeds on entry and the final centres afterwards;
        outputs valid in `stream` order.  Returns the stats dict."""
        return _kmajority_dev(self, self._L.vc_sharded_kmajority_dev, k, d_centres, d_assign, d_labels, max_iters, stream)

    def seed_centres(self, k, method=SEED_FARTHEST, seed=0, with_assign=False):
        """vc_sharded_seed_centres: k seeds for kmajority made on the device -- SEED_FARTHEST, the farthest-first traversal, or SEED_WEIGHTED, a record
        sampled with probability proportional to its distance to the nearest chosen seed (SplitMix64 from `seed`; the first record is
        draw(0) % N in both).  Returns (centres, picks, assign, stats): picks[t] = id | distance to the seeds before it << 32, assign ==
        assign_nearest(centres) (None unless with_assign), stats a dict of cost, radius, n_zero_picks.  A function of the codes, k, the
        method and `seed` only."""
        return _seed_centres(self, self._L.vc_sharded_seed_centres, k, method, seed, with_assign)

    def seed_centres_dev(self, k, d_centres, d_picks=None, d_assign=None, method=SEED_FARTHEST, seed=0, with_stats=True, stream=None):
        """vc_sharded_seed_centres_dev: raw device addresses on the root device; outputs valid in `stream` order.  Returns the stats dict; with_stats=False returns
        None (the root still waits once or twice per round)."""
        return _seed_centres_dev(self, self._L.vc_sharded_seed_centres_dev, k, d_centres, d_picks, d_assign, method, seed, with_stats, stream)

    def search_knn_distinct(self, queries, k, labels, mode=MODE_LINEAR, order=ORDER_ASCENDING, k_first=0, with_stats=False):
        """vc_sharded_search_knn_distinct: the k nearest label GROUPS of every query, each by its member nearest to the query.  labels: one
        uint32 per resident record as cluster_radius, leaders_radius, dbscan_radius, kmajority or group_summary's group_index write
        them -- only equality matters.  Returns (out [nq, k] uint64, row_labels [nq, k] uint32, counts [nq][, stats dict]); a count
        may carry DISTINCT_TRUNCATED.  mode MODE_LINEAR or MODE_MIH_EXACT; k_first: the first round's k' (0 = min(8192, 2 k)), which
        changes the statistics, never a finished row.  Stages the labels on every call: search_knn_distinct_dev keeps them in HBM."""
        return _search_knn_distinct(self, self._L.vc_sharded_search_knn_distinct, queries, k, labels, mode, order, k_first, with_stats)

    def search_knn_distinct_dev(self, d_queries, nq, k, d_labels, d_out, d_row_labels=None, d_counts=None, mode=MODE_LINEAR, k_first=0, with_stats=True,
                                stream=None):
        """vc_sharded_search_knn_distinct_dev: raw device addresses on the root device; the host waits once per round, results valid in `stream` order.
        Returns the stats dict; with_stats=False returns None."""
        return _search_knn_distinct_dev(self, self._L.vc_sharded_search_knn_distinct_dev, d_queries, nq, k, d_labels, d_out, d_row_labels, d_counts, mode, k_first,
                                        with_stats, stream)

    def search_knn_filtered(self, queries, k, sel, kind=FILTER_MASK, value=0, mode=MODE_LINEAR, order=ORDER_ASCENDING, k_first=0, with_stats=False):
        """vc_sharded_search_knn_filtered: the k nearest among the records the filter allows, exact for every selectivity.  sel: one uint32 per
        resident record -- FILTER_MASK (nonzero), FILTER_ROOTS (a grouper's labels: the representatives), FILTER_EQUAL / FILTER_NOT_EQUAL
        (against `value`) -- or one bit per record (FILTER_BITS, ceil(N / 32) words).  Returns (out [nq, k] uint64, counts [nq][, stats
        dict]); counts = min(k, allowed).  mode MODE_LINEAR or MODE_MIH_EXACT; k_first: the first post-filter round's k' (0 = the plan's),
        which changes the statistics, never a row.  Stages sel on every call: search_knn_filtered_dev keeps it in HBM."""
        return _search_knn_filtered(self, self._L.vc_sharded_search_knn_filtered, queries, k, sel, kind, value, mode, order, k_first, with_stats)

    def search_knn_filtered_dev(self, d_queries, nq, k, d_sel, d_out, d_counts=None, kind=FILTER_MASK, value=0, mode=MODE_LINEAR, k_first=0, with_stats=True,
                                stream=None):
        """vc_sharded_search_knn_filtered_dev: raw device addresses on the root device; the host waits once for the allowed count and once per post-filter round, results
        valid in `stream` order.  Returns the stats dict; with_stats=False returns None."""
        return _search_knn_filtered_dev(self, self._L.vc_sharded_search_knn_filtered_dev, d_queries, nq, k, d_sel, kind, value, d_out, d_counts, mode, k_first, with_stats,
                                        stream)

    def search_knn_scoped(self, queries, k, scope, qscope, order=ORDER_ASCENDING, with_stats=False):
        """vc_sharded_search_knn_scoped: for every query the k nearest among the records whose scope word equals the query's own, ids global
        over the store.  Returns (out uint64 [nq, k], counts uint32 [nq][, stats dict]); counts = min(k, size of the query's scope)."""
        return _search_knn_scoped(self, self._L.vc_sharded_search_knn_scoped, queries, k, scope, qscope, order, with_stats)

    def search_knn_scoped_dev(self, d_queries, nq, k, d_scope, d_qscope, d_out, d_counts=None, with_stats=True, stream=None):
        """vc_sharded_search_knn_scoped_dev: raw device addresses on the root device; the host waits twice, results valid in `stream` order.
        Returns the stats dict; with_stats=False returns None."""
        return _search_knn_scoped_dev(self, self._L.vc_sharded_search_knn_scoped_dev, d_queries, nq, k, d_scope, d_qscope, d_out, d_counts, with_stats, stream)

    def knn_graph(self, k, mode=MODE_LINEAR, batch=0, first=0, count=0, k_first=0, with_stats=False):
        """vc_sharded_knn_graph: the exact k-NN graph of the store.  Row p - first holds the k smallest packed (dist << 32 | id) over all resident
        records other than record id_base + p, ascending, UINT64_MAX padded; counts = min(k, N - 1).  The same words in MODE_LINEAR and
        MODE_MIH_EXACT, for every batch and k_first.  count == 0: to the end.  Returns (rows [n, k], counts [n][, stats dict])."""
        return _knn_graph(self, self._L.vc_sharded_knn_graph, k, mode, batch, first, count, k_first, with_stats)

    def knn_graph_dev(self, k, d_rows, d_counts=None, mode=MODE_MIH_EXACT, batch=0, first=0, count=0, k_first=0, with_stats=True, stream=None):
        """vc_sharded_knn_graph_dev: raw device addresses on the root device (d_rows n * k uint64, d_counts n uint32 or None); results valid in `stream`
        order.  Returns the stats dict (None without with_stats)."""
        return _knn_graph_dev(self, self._L.vc_sharded_knn_graph_dev, k, d_rows, d_counts, mode, batch, first, count, k_first, with_stats, stream)

    def knn_graph_update(self, rows, counts=None, mode=MODE_LINEAR, batch=0, k_first=0, with_stats=False):
        """vc_sharded_knn_graph_update: the graph after an append.  rows [n_old, k] (and counts [n_old] or None) are knn_graph's over the
        store when it held its first n_old records; returns the rows [N, k] and counts [N] (None without counts) of knn_graph over the
        store now, the same words.  In MODE_MIH_EXACT run update_index() first."""
        return _knn_graph_update(self, self._L.vc_sharded_knn_graph_update, rows, counts, None, mode, batch, k_first, with_stats)

    def knn_graph_update_dev(self, k, n_old, d_rows, d_counts=None, mode=MODE_MIH_EXACT, batch=0, k_first=0, with_stats=True, stream=None):
        """vc_sharded_knn_graph_update_dev: raw device addresses on the root device (d_rows N * k uint64 whose first n_old rows are the
        graph as it was, d_counts N uint32 or None); results valid in `stream` order.  Returns the stats dict (or None)."""
        return _knn_graph_update_dev(self, self._L.vc_sharded_knn_graph_update_dev, k, n_old, d_rows, d_counts, mode, batch, k_first, with_stats, stream)

    def knn_graph_retain(self, rows, new_ids, counts=None, mode=MODE_LINEAR, batch=0, k_first=0, with_stats=False):
        """vc_sharded_knn_graph_retain: the graph after a removal.  rows [n_old, k] (and counts [n_old] or None) are knn_graph's over the store
        before retain(), new_ids the map retain() returned; returns the rows [K, k] and counts [K] (None without counts) of knn_graph
        over the store now, the same words.  Only the rows that lost too many entries are searched again."""
        return _knn_graph_retain(self, self._L.vc_sharded_knn_graph_retain, rows, new_ids, counts, mode, batch, k_first, with_stats)

    def knn_graph_retain_dev(self, k, n_old, d_new_ids, d_rows, d_counts=None, mode=MODE_MIH_EXACT, batch=0, k_first=0, with_stats=True, stream=None):
        """vc_sharded_knn_graph_retain_dev: raw device addresses on the root device (d_new_ids n_old uint32 as retain_dev wrote it, d_rows n_old * k uint64 and
        d_counts n_old uint32 or None, the graph as it was); results valid in `stream` order.  Returns the stats dict (or None)."""
        return _knn_graph_retain_dev(self, self._L.vc_sharded_knn_graph_retain_dev, k, n_old, d_new_ids, d_rows, d_counts, mode, batch, k_first, with_stats, stream)

    def cluster_knn(self, rows, counts, kk, flags=KNN_MUTUAL, max_dist=0xFFFFFFFF, with_in_degree=True):
        """vc_sharded_cluster_knn: components and in-degrees of a graph knn_graph built over the whole store (rows [N, k], counts [N] or None).
        Row i lists j iff j is among its first kk entries at a distance <= max_dist; KNN_MUTUAL joins i and j iff each lists the other,
        KNN_EITHER iff one does.  Returns (labels [N] -- the smallest id of each component, as cluster_radius --, in_degree [N] | None,
        stats dict of n_edges, n_mutual, n_clusters, max_in_degree)."""
        return _cluster_knn(self, self._L.vc_sharded_cluster_knn, rows, counts, kk, flags, max_dist, with_in_degree)

    def cluster_knn_dev(self, d_rows, d_counts, k, kk, d_labels, d_in_degree=None, flags=KNN_MUTUAL, max_dist=0xFFFFFFFF, with_stats=True, stream=None):
        """vc_sharded_cluster_knn_dev: raw device addresses on the root device; nothing is searched, the host waits once.  Returns the stats dict (None without
        with_stats)."""
        return _cluster_knn_dev(self, self._L.vc_sharded_cluster_knn_dev, d_rows, d_counts, k, kk, flags, max_dist, d_labels, d_in_degree, with_stats, stream)

    def cluster_snn(self, rows, counts, kk, min_shared, flags=KNN_MUTUAL, max_dist=0xFFFFFFFF, with_shared=True, with_hist=True):
        """vc_sharded_cluster_snn: shared-nearest-neighbour clusters of a graph knn_graph built over the whole store (rows [N, k], counts [N] or None).
        "Lists" and the candidate pairs are cluster_knn's; a candidate pair is joined iff the two lists of kk share at least min_shared
        records.  Returns (labels [N], shared [N, kk] | None -- the weight of every listed entry, SNN_NONE elsewhere --, hist [kk] | None
        -- the listed entries by weight --, stats dict of n_edges, n_mutual, n_joined, n_clusters, max_shared)."""
        return _cluster_snn(self, self._L.vc_sharded_cluster_snn, rows, counts, kk, min_shared, flags, max_dist, with_shared, with_hist)

    def cluster_snn_dev(self, d_rows, d_counts, k, kk, min_shared, d_labels, d_shared=None, d_hist=None, flags=KNN_MUTUAL, max_dist=0xFFFFFFFF, with_stats=True,
                        stream=None):
        """vc_sharded_cluster_snn_dev: raw device addresses on the root device; nothing is searched, the host waits once.  Returns the stats dict (None without
        with_stats)."""
        return _cluster_snn_dev(self, self._L.vc_sharded_cluster_snn_dev, d_rows, d_counts, k, kk, min_shared, flags, max_dist, d_labels, d_shared, d_hist, with_stats, stream)

    def knn_adjacency(self, rows, counts, kk, flags=KNN_REVERSE, max_dist=0xFFFFFFFF):
        """vc_sharded_knn_adjacency: the reverse (KNN_REVERSE), mutual (KNN_MUTUAL) or symmetrised (KNN_EITHER) graph of a graph knn_graph
        built over the whole store, in CSR form.  Returns (offsets [N + 1], adj [T], stats dict), word for word Engine.knn_adjacency's."""
        return _knn_adjacency(self, self._L.vc_sharded_knn_adjacency, rows, counts, kk, flags, max_dist)

    def knn_adjacency_dev(self, d_rows, d_counts, k, kk, d_adj, adj_cap, d_offsets, flags=KNN_REVERSE, max_dist=0xFFFFFFFF, with_stats=True, stream=None):
        """vc_sharded_knn_adjacency_dev: raw device addresses on the root device; no shard is touched, the host waits once.  Returns
        (rc, stats dict | None) as Engine.knn_adjacency_dev."""
        return _knn_adjacency_dev(self, self._L.vc_sharded_knn_adjacency_dev, d_rows, d_counts, k, kk, flags, max_dist, d_adj, adj_cap, d_offsets, with_stats,
                                  stream)

    def knn_mst(self, rows, counts, kk, flags=KNN_MUTUAL, max_dist=0xFFFFFFFF, weight_kind=MST_DISTANCE, min_pts=1, with_labels=True, with_hist=True):
        """vc_sharded_knn_mst: the minimum spanning forest, in Kruskal order, of the mutual (KNN_MUTUAL) or symmetrised (KNN_EITHER) graph of a
        graph knn_graph built over the whole store (rows [N, k], counts [N] or None); "lists" is cluster_knn's.  weight_kind
        MST_DISTANCE weighs an edge by its distance, MST_REACHABILITY by max(distance, the two core distances at min_pts).  Returns
        (edges MST_EDGE [M] ascending in (weight, a, dist, b), labels [N] | None, hist [bits + 1] | None, stats dict of n_edges,
        n_graph_edges, n_tree, n_clusters, total_weight, max_weight, n_rounds)."""
        return _knn_mst(self, self._L.vc_sharded_knn_mst, rows, counts, kk, flags, max_dist, weight_kind, min_pts, with_labels, with_hist)

    def knn_mst_dev(self, d_rows, d_counts, k, kk, d_edges, d_labels=None, d_hist=None, flags=KNN_MUTUAL, max_dist=0xFFFFFFFF, weight_kind=MST_DISTANCE,
                    min_pts=1, with_stats=True, stream=None):
        """vc_sharded_knn_mst_dev: raw device addresses on the root device; d_edges has room for max(N, 1) - 1 vc_mst_edge; nothing is searched, the host
        waits once per Boruvka round and once at the end.  Returns the stats dict (None without with_stats)."""
        return _knn_mst_dev(self, self._L.vc_sharded_knn_mst_dev, d_rows, d_counts, k, kk, flags, max_dist, weight_kind, min_pts, d_edges, d_labels, d_hist, with_stats,
                            stream)

    def mst_cut(self, edges, max_weight):
        """vc_sharded_mst_cut: the components of the store under the edges (MST_EDGE records, any order) of weight <= max_weight.  Returns
        (labels [N] -- the smallest id of each component --, n_clusters)."""
        return _mst_cut(self, self._L.vc_sharded_mst_cut, edges, max_weight)

    def mst_cut_dev(self, d_edges, n_edges, max_weight, d_labels, stream=None):
        """vc_sharded_mst_cut_dev: raw device addresses on the root device; the host waits once.  Returns n_clusters."""
        return _mst_cut_dev(self, self._L.vc_sharded_mst_cut_dev, d_edges, n_edges, max_weight, d_labels, stream)

    def mst_condense(self, edges, min_cluster_size, root_weight=0, method=CONDENSE_EOM, with_node=True, with_own=True, with_leave=True):
        """vc_sharded_mst_condense: the HDBSCAN-style clusters of a spanning forest (MST_EDGE records ascending in weight, as knn_mst returns them,
        best under MST_REACHABILITY): the condensed tree at min_cluster_size, the integer stability of every node, the excess-of-mass
        (CONDENSE_EOM) or leaf (CONDENSE_LEAF) selection and the flat labels.  root_weight 0 never selects a whole component of the forest;
        otherwise it is the height, above every edge, at which the components are deemed to merge.  Returns (nodes CONDENSED_NODE [n_nodes]
        ascending in (form, rep), labels [N] -- rep of the record's selected cluster, its own id for noise --, node [N] | None -- that
        cluster's index, CONDENSE_NONE for noise --, own [N] | None, leave [N] | None, stats dict of n_nodes, n_leaves, n_roots, n_selected,
        n_clustered, n_noise, total_stability, n_levels)."""
        return _mst_condense(self, self._L.vc_sharded_mst_condense, edges, min_cluster_size, root_weight, method, with_node, with_own, with_leave)

    def mst_condense_dev(self, d_edges, n_edges, min_cluster_size, d_nodes, d_labels, d_node=None, d_own=None, d_leave=None, root_weight=0, method=CONDENSE_EOM,
                         with_stats=True, stream=None):
        """vc_sharded_mst_condense_dev: raw device addresses on the root device; d_nodes has room for max(N, 1) - 1 vc_condensed_node; the host waits three times for a
        few words.  Returns the stats dict (n_nodes says how many nodes were written) or None."""
        return _mst_condense_dev(self, self._L.vc_sharded_mst_condense_dev, d_edges, n_edges, min_cluster_size, root_weight, method, d_nodes, d_labels, d_node, d_own,
                                 d_leave, with_stats, stream)

    def knn_vote(self, rows, counts, kk, labels, weight_kind=VOTE_COUNT, max_dist=0xFFFFFFFF, with_votes=True):
        """vc_sharded_knn_vote: the k-NN classifier over any rows [n_rows, k] whose ids are resident (counts [n_rows] or None: min(k, N) entries
        each) -- a graph of knn_graph or the rows of a search.  Row r's label is the winner among its first min(kk, count) entries
        within max_dist under labels [N] (VOTE_NONE does not vote): the larger tally (VOTE_COUNT: 1 an entry, VOTE_CLOSENESS:
        bits + 1 - distance), ties to the label met first.  Returns (label [n_rows], votes | None, total | None, stats dict of
        n_voted, n_unlabelled, n_ties, n_entries)."""
        return _knn_vote(self, self._L.vc_sharded_knn_vote, rows, counts, kk, labels, weight_kind, max_dist, with_votes)

    def knn_vote_dev(self, d_rows, d_counts, n_rows, k, kk, d_labels, d_out_label, d_out_votes=None, d_out_total=None, weight_kind=VOTE_COUNT,
                     max_dist=0xFFFFFFFF, with_stats=True, stream=None):
        """vc_sharded_knn_vote_dev: raw device addresses on the root device; one launch and one wait.  Returns the stats dict (None without with_stats)."""
        return _knn_vote_dev(self, self._L.vc_sharded_knn_vote_dev, d_rows, d_counts, n_rows, k, kk, d_labels, weight_kind, max_dist, d_out_label, d_out_votes,
                             d_out_total, with_stats, stream)

    def label_propagate(self, offsets, adj, labels, weight_kind=VOTE_COUNT, flags=0, max_iters=LP_MAX_ITERS, with_votes=True):
        """vc_sharded_label_propagate: synchronous label propagation over the CSR (offsets [N + 1], adj) of knn_adjacency from labels [N]:
        every round each record takes the winner of its segment under the previous round's labels (the larger tally, then its
        current label, then the label met first) or keeps its label when nothing votes; LP_CLAMP_SEEDS keeps every labelled record
        of `labels` fixed (semi-supervised), labels = id_base + arange(N) without it is community detection.  Stops after the first
        round without a change or after max_iters <= LP_MAX_ITERS.  Returns (labels [N], votes | None, total | None of the last round,
        stats dict of n_iters, converged, n_changed_last, n_labelled, n_ties_last)."""
        return _label_propagate(self, self._L.vc_sharded_label_propagate, offsets, adj, labels, weight_kind, flags, max_iters, with_votes)

    def label_propagate_dev(self, d_offsets, d_adj, n_entries, d_labels_in, d_labels_out, d_votes=None, d_total=None, weight_kind=VOTE_COUNT, flags=0,
                            max_iters=LP_MAX_ITERS, with_stats=True, stream=None):
        """vc_sharded_label_propagate_dev: raw device addresses on the root device; one wait for the plan and one small read-back per round.  Returns the
        stats dict (None without with_stats)."""
        return _label_propagate_dev(self, self._L.vc_sharded_label_propagate_dev, d_offsets, d_adj, n_entries, d_labels_in, weight_kind, flags, max_iters,
                                    d_labels_out, d_votes, d_total, with_stats, stream)

    def search_knn(self, queries, k, mode=MODE_LINEAR, order=ORDER_ASCENDING, with_stats=False):
        q = np.ascontiguousarray(queries, dtype=np.uint8)
        if q.ndim == 1:
            q = q[None, :]
        nq = q.shape[0]
        out = np.full((nq, k), PACK_INF, dtype=np.uint64)
        counts = np.zeros(nq, dtype=np.uint32)
        stats = (VcQueryStats * nq)() if with_stats else None
        self._check(self._L.vc_sharded_search_knn(self._h, _p(q), nq, k, mode, order, _p(out), _p(counts),
                                                  C.cast(stats, C.c_void_p) if with_stats else None))
        if with_stats:
            return out, counts, list(stats)
        return out, counts
