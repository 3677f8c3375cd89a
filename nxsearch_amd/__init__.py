"""nxsearch_amd -- MI355X-native query/ranking path behind nxsearch's C API.

Thin ctypes binding over ``csrc/libnxsearch_gpu.so`` (C11 host code + HIP
kernels for gfx950).  The class layout mirrors the reference's Lua binding
(`nxs.open(basedir)`, `index:search(query, params)`, reference
src/core/lua.c:341-366) and, underneath, its C API (include/nxs.h).

There is no CPU fallback: importing works anywhere, but opening an index
without a HIP device raises, and a missing shared library raises on import of
the binding (`lib()`).
"""
import ctypes as C
import os

__all__ = ["Nxs", "Index", "NxsError", "Results", "Suggestions", "lib", "build", "LIB_PATH"]

_HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(_HERE, "csrc")
LIB_PATH = os.environ.get("NXS_GPU_LIB") or os.path.join(CSRC, "libnxsearch_gpu.so")
SYNTH_PATH = os.path.join(CSRC, "libnxssynth.so")

MAX_TOKENS, MAX_PROG, FAST_K = 32, 256, 64
TF_IDF, BM25 = 0, 1
ERR_NAMES = ["SUCCESS", "FATAL", "SYSTEM", "INVALID", "EXISTS", "MISSING", "LIMIT"]


class NxsError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__("NXS_ERR_%s: %s" % (ERR_NAMES[code] if 0 <= code < 7 else code, msg))
        self.code = code
        self.msg = msg


class GpuQuery(C.Structure):
    """nxsgpu_query_t (include/nxs_gpu.h)"""
    _fields_ = [("n_tokens", C.c_uint32),
                ("term_id", C.c_uint32 * MAX_TOKENS),
                ("prog_len", C.c_uint32),
                ("prog", C.c_uint8 * MAX_PROG),
                ("truth", C.c_uint32 * 8)]


class GpuBkNode(C.Structure):
    """nxsgpu_bknode_t"""
    _fields_ = [("bitmap", C.c_uint64), ("first_child", C.c_uint32),
                ("term_id", C.c_uint32), ("str_off", C.c_uint32),
                ("str_len", C.c_uint16), ("flags", C.c_uint16),
                ("inl", C.c_uint8 * 8)]


class BkImage(C.Structure):
    """nxs_bkimage_t (csrc/nxs_impl.h)"""
    _fields_ = [("nodes", C.POINTER(GpuBkNode)), ("n", C.c_uint32),
                ("depth", C.c_uint32), ("bytes", C.POINTER(C.c_uint8)),
                ("bytes_len", C.c_uint64)]


class GpuResults(C.Structure):
    """nxsgpu_results_t"""
    _fields_ = [("n_queries", C.c_uint32), ("counts", C.POINTER(C.c_uint32)),
                ("offsets", C.POINTER(C.c_uint64)), ("doc_ids", C.POINTER(C.c_uint64)),
                ("scores", C.POINTER(C.c_float)), ("postings", C.c_uint64),
                ("candidates", C.c_uint64), ("exact_requeries", C.c_uint32)]


class GpuProfile(C.Structure):
    """nxsgpu_profile_t"""
    _fields_ = [("launches", C.c_uint64), ("scan_ms", C.c_double),
                ("replay_ms", C.c_double), ("fuzzy_ms", C.c_double),
                ("postings", C.c_uint64), ("fuzzy_visits", C.c_uint64),
                ("fuzzy_pairs", C.c_uint64), ("fuzzy_level", C.c_uint64 * 40),
                ("fuzzy_filter_ms", C.c_double), ("fuzzy_dist_ms", C.c_double),
                ("fuzzy_chain_ms", C.c_double), ("fuzzy_checked", C.c_uint64),
                ("n_cls", C.c_uint32), ("cls_key", C.c_uint32 * 16), ("cls_launches", C.c_uint64 * 16),
                ("cls_ms", C.c_double * 16), ("cls_postings", C.c_uint64 * 16), ("cls_queries", C.c_uint64 * 16)]


# every symbol include/nxs.h and include/nxs_gpu.h declare
NXS_H_SYMBOLS = [
    "nxs_open", "nxs_close", "nxs_get_error", "nxs_params_create", "nxs_params_fromjson",
    "nxs_params_set_str", "nxs_params_set_uint", "nxs_params_set_bool",
    "nxs_params_release", "nxs_index_open", "nxs_index_close",
    "nxs_index_search", "nxs_resp_iter_reset", "nxs_resp_iter_result",
    "nxs_resp_resultcount", "nxs_resp_tojson", "nxs_resp_release",
    "nxs_index_search_batch", "nxs_index_open_files",
    "nxs_index_plan_batch", "nxs_index_search_batch_begin",
    "nxs_index_search_batch_end", "nxs_shard_unique_id", "nxs_index_shard",
    "nxs_index_shard_local", "nxs_index_shard_slice",
    "nxs_index_open_shard", "nxs_docshard_search_batch",
    "nxs_docshard_attach", "nxs_docshard_search_batch_rank",
    "nxs_docshard_refresh", "nxs_docshard_refresh_rank", "nxs_resp_total",
    "nxs_index_suggest", "nxs_index_suggest_batch", "nxs_sugg_count", "nxs_sugg_matches", "nxs_sugg_dropped",
    "nxs_sugg_get", "nxs_sugg_tojson", "nxs_sugg_release",
    "nxs_index_complete", "nxs_index_complete_batch",
    "nxs_index_wildcard", "nxs_index_wildcard_batch",
    "nxs_resp_tokens", "nxs_resp_token", "nxs_resp_explain",
    "nxs_index_doc_terms", "nxs_index_doc_terms_batch", "nxs_sugg_score",
    "nxs_index_similar", "nxs_index_similar_batch",
    "nxs_index_related", "nxs_index_related_batch", "nxs_sugg_docs",
    "nxs_index_search_docs", "nxs_index_search_docs_batch",
    "nxs_index_match_docs", "nxs_index_match_docs_batch", "nxs_docs_count", "nxs_docs_ids", "nxs_docs_total",
    "nxs_docs_next", "nxs_docs_tojson", "nxs_docs_release",
]
# csrc/nxs_hooks.h: test hooks + bench accessors, only in builds with -DNXS_TEST_HOOKS (the default)
NXS_HOOK_SYMBOLS = ["nxs_index_device", "nxs_index_host_profile", "nxs_index_shard_info", "nxs_test_pool", "nxs_test_assemble",
                    "nxs_test_index_image", "nxsgpu_test_index_image",
                    "nxs_test_term_image", "nxsgpu_test_term_image",
                    "nxs_test_fixup_scan", "nxs_test_inject_failure", "nxs_test_count_tile_widths",
                    "nxs_test_suggest_host", "nxs_test_suggest_params", "nxs_test_sugg_build",
                    "nxs_test_complete_host", "nxs_test_complete_params", "nxs_test_compl_build",
                    "nxs_test_prefix_query", "nxs_test_filter_prefix",
                    "nxs_test_wild_match", "nxs_test_wild_match_inl", "nxs_test_wild_host", "nxs_test_wild_params",
                    "nxs_test_wild_normalize", "nxs_test_wild_build", "nxs_test_wild_query",
                    "nxs_test_explain_params", "nxs_test_resp_build", "nxs_test_explain_search",
                    "nxs_test_explain_ordinal",
                    "nxs_test_docterms_params", "nxs_test_docterms_build", "nxs_test_docterms_lane",
                    "nxs_test_docterms_key", "nxs_test_similar_drop",
                    "nxs_test_related_params", "nxs_test_related_build", "nxs_test_related_key",
                    "nxs_test_related_share", "nxs_test_related_eligible", "nxs_test_related_rank",
                    "nxs_test_docset_sort", "nxs_test_docset_lane",
                    "nxs_test_match_params", "nxs_test_docs_build", "nxs_test_md_lower_bound", "nxs_test_md_page"]
NXS_GPU_H_SYMBOLS = [
    "nxsgpu_device_count", "nxsgpu_last_error", "nxsgpu_index_create",
    "nxsgpu_index_destroy", "nxsgpu_index_df", "nxsgpu_index_postings",
    "nxsgpu_index_docs", "nxsgpu_index_first_bad_doc", "nxsgpu_search",
    "nxsgpu_results_free", "nxsgpu_search_dev", "nxsgpu_search_dev_begin",
    "nxsgpu_search_dev_end", "nxsgpu_fuzzy", "nxsgpu_fuzzy_begin", "nxsgpu_fuzzy_end",
    "nxsgpu_set_profiling", "nxsgpu_get_profile", "nxsgpu_synchronize",
    "nxsgpu_search_wide", "nxsgpu_shard_slice", "nxsgpu_shard_capacity",
    "nxsgpu_comm_unique_id", "nxsgpu_comm_create", "nxsgpu_comm_destroy",
    "nxsgpu_comm_rank", "nxsgpu_comm_world", "nxsgpu_comm_rccl_count", "nxsgpu_comm_stats", "nxsgpu_comm_allgather",
    "nxsgpu_index_set_comm", "nxsgpu_batch_begin", "nxsgpu_batch_end",
    "nxsgpu_batches_in_flight", "nxsgpu_index_reconfigure", "nxsgpu_index_set_parallel", "nxsgpu_hbm_read_gbs",
    "nxsgpu_hbm_calibrate",
    "nxsgpu_index_apply", "nxsgpu_index_set_bk", "nxsgpu_index_set_global_df", "nxsgpu_index_impact_passes",
    "nxsgpu_search_candidates", "nxsgpu_merge_candidates",
    "nxsgpu_count", "nxsgpu_count_wide", "nxsgpu_search_totals", "nxsgpu_search_wide_totals", "nxsgpu_batch_begin_opts",
    "nxsgpu_batch_end_totals", "nxsgpu_count_tile_widths", "nxsgpu_count_profile",
    "nxsgpu_suggest", "nxsgpu_suggest_profile",
    "nxsgpu_complete", "nxsgpu_complete_profile",
    "nxsgpu_wildcard", "nxsgpu_wildcard_profile",
    "nxsgpu_explain", "nxsgpu_explain_profile",
    "nxsgpu_doc_terms", "nxsgpu_doc_terms_profile",
    "nxsgpu_related", "nxsgpu_related_profile",
    "nxsgpu_search_docs", "nxsgpu_search_docs_profile",
    "nxsgpu_match_docs", "nxsgpu_match_docs_profile",
]

# nxs_test_index_image (csrc/nxs_hooks.h): part numbers and the order of the scalars, as nxsgpu_test_index_image
# (csrc/nxs_gpu_index.hip) has them
IMG_SCALARS = 0
IMG_SCALAR_NAMES = ["n_docs", "n_post", "n_terms", "hdr_doc_count", "hdr_token_count", "max_tf", "bm_words",
                    "dense_q8_stride", "cap_post", "scanm_dens", "outl_share", "bm_share", "algo_on", "switches"]
IMG_PARTS = {"doc_ids": (1, "<u8"), "doc_len": (2, "<u4"), "post_off": (3, "<u8"), "post_dt": (4, "<u8"),
             "post": (5, "post"), "outl_post": (6, "post"), "maximp": (7, "<u4"), "dense_terms": (8, "<u4"),
             "dense_col": (9, "<u4"), "dense_q8": (10, "u1"), "outl_off": (11, "<u8"), "outl_cap": (12, "<u4"),
             "outl_max": (13, "<u4"), "bm_terms": (14, "<u4"), "blkmap": (15, "<u8"), "bmrank": (16, "<u4")}
IMG_DF_GLOBAL = 17      # u32[T + 2], a doc shard's collection-wide df (N4); no bytes on a whole index
IMG_PER_ALGO = (5, 7, 9)
# nxs_test_term_image: the same for the term-side state, as nxsgpu_test_term_image (csrc/nxs_gpu_fuzzy.hip) has them
TIMG_SCALARS = 0
TIMG_SCALAR_NAMES = ["n_bk", "bk_depth", "bk_bytes_len", "n_fz", "sg_gen", "sg_built", "sg_built_gen", "sg_n_c",
                     "px_gen", "px_built", "px_built_gen", "px_n_e", "px_builds"]
TIMG_PARTS = {"bk": (1, "bk"), "bk_bytes": (2, "u1"), "bk_parent": (3, "<u4"), "bk_slot": (4, "u1"),
              "fz_node": (5, "<u4"), "fz_sig": (6, "<u4"), "fz_len": (7, "u1"), "fz_len_start": (8, "<u4"),
              "sg_node": (9, "<u4"), "sg_sig": (10, "<u4"), "sg_len": (11, "u1"),
              "px_node": (12, "<u4"), "px_key": (13, "<u8")}
# nxsgpu_bknode_t (include/nxs_gpu.h) as a numpy record
TIMG_BK_DTYPE = [("bitmap", "<u8"), ("first_child", "<u4"), ("term_id", "<u4"), ("str_off", "<u4"),
                 ("str_len", "<u2"), ("flags", "<u2"), ("inl", "u1", (8,))]

_lib = None


def build():
    """(Re)build the shared libraries in-tree with make + hipcc."""
    import subprocess
    subprocess.run(["make", "-C", CSRC], check=True, stdout=subprocess.DEVNULL)


def lib():
    """The loaded libnxsearch_gpu.so; raises if it has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            "%s is missing: build it with `make -C %s` (hipcc, gfx950). "
            "There is no CPU fallback for the query path." % (LIB_PATH, CSRC))
    L = C.CDLL(LIB_PATH, mode=C.RTLD_GLOBAL)
    vp, cp = C.c_void_p, C.c_char_p
    L.nxs_open.restype = vp
    L.nxs_open.argtypes = [cp]
    L.nxs_close.argtypes = [vp]
    L.nxs_get_error.restype = C.c_int
    L.nxs_get_error.argtypes = [vp, C.POINTER(cp)]
    L.nxs_params_create.restype = vp
    L.nxs_params_fromjson.restype = vp
    L.nxs_params_fromjson.argtypes = [vp, cp, C.c_size_t]
    L.nxs_params_get_str.restype = cp
    L.nxs_params_get_str.argtypes = [vp, cp]
    L.nxs_params_get_uint.argtypes = [vp, cp, C.POINTER(C.c_uint64)]
    L.nxs_params_get_bool.argtypes = [vp, cp, C.POINTER(C.c_bool)]
    L.nxs_params_set_str.argtypes = [vp, cp, cp]
    L.nxs_params_set_uint.argtypes = [vp, cp, C.c_uint64]
    L.nxs_params_set_bool.argtypes = [vp, cp, C.c_bool]
    L.nxs_params_release.argtypes = [vp]
    L.nxs_index_open.restype = vp
    L.nxs_index_open.argtypes = [vp, cp]
    L.nxs_index_open_files.restype = vp
    L.nxs_index_open_files.argtypes = [vp, cp, cp, cp, C.c_bool]
    L.nxs_index_close.argtypes = [vp]
    L.nxs_index_device.restype = vp
    L.nxs_index_device.argtypes = [vp]
    L.nxs_index_search.restype = vp
    L.nxs_index_search.argtypes = [vp, vp, cp, C.c_size_t]
    L.nxs_index_search_batch.restype = C.c_int
    L.nxs_index_search_batch.argtypes = [vp, vp, C.POINTER(cp), C.c_size_t,
                                         C.POINTER(vp), C.POINTER(C.c_int)]
    L.nxs_index_search_batch_begin.restype = C.c_int
    L.nxs_index_search_batch_begin.argtypes = [vp, vp, C.POINTER(cp), C.c_size_t]
    L.nxs_index_search_batch_end.restype = C.c_int
    L.nxs_index_search_batch_end.argtypes = [vp, C.POINTER(vp), C.POINTER(C.c_int)]
    L.nxs_shard_unique_id.restype = C.c_int
    L.nxs_shard_unique_id.argtypes = [vp, C.c_char_p]
    L.nxs_index_shard.restype = C.c_int
    L.nxs_index_shard.argtypes = [vp, C.c_int, C.c_int, C.c_char_p]
    L.nxs_index_plan_batch.restype = C.c_int
    L.nxs_index_plan_batch.argtypes = [vp, vp, C.POINTER(cp), C.c_size_t,
                                       C.POINTER(GpuQuery), C.POINTER(C.c_int)]
    L.nxs_resp_iter_reset.argtypes = [vp]
    L.nxs_resp_iter_result.restype = C.c_bool
    L.nxs_resp_iter_result.argtypes = [vp, C.POINTER(C.c_uint64), C.POINTER(C.c_float)]
    L.nxs_resp_resultcount.restype = C.c_uint
    L.nxs_resp_resultcount.argtypes = [vp]
    L.nxs_resp_tojson.restype = vp
    L.nxs_resp_tojson.argtypes = [vp, C.POINTER(C.c_size_t)]
    L.nxs_resp_release.argtypes = [vp]
    L.nxs_resp_total.restype = C.c_bool
    L.nxs_resp_total.argtypes = [vp, C.POINTER(C.c_uint64)]
    L.nxs_resp_tokens.restype = C.c_uint
    L.nxs_resp_tokens.argtypes = [vp]
    L.nxs_resp_token.restype = C.c_bool
    L.nxs_resp_token.argtypes = [vp, C.c_uint, C.POINTER(vp), C.POINTER(C.c_size_t)]
    L.nxs_resp_explain.restype = C.c_bool
    L.nxs_resp_explain.argtypes = [vp, C.c_uint, C.c_uint, C.POINTER(C.c_float), C.POINTER(C.c_uint32)]
    L.nxs_index_suggest.restype = vp
    L.nxs_index_suggest.argtypes = [vp, vp, cp, C.c_size_t]
    L.nxs_index_suggest_batch.restype = C.c_int
    L.nxs_index_suggest_batch.argtypes = [vp, vp, C.POINTER(cp), C.c_size_t, C.POINTER(vp), C.POINTER(C.c_int)]
    L.nxs_index_complete.restype = vp
    L.nxs_index_complete.argtypes = [vp, vp, cp, C.c_size_t]
    L.nxs_index_complete_batch.restype = C.c_int
    L.nxs_index_complete_batch.argtypes = [vp, vp, C.POINTER(cp), C.c_size_t, C.POINTER(vp), C.POINTER(C.c_int)]
    L.nxs_index_wildcard.restype = vp
    L.nxs_index_wildcard.argtypes = [vp, vp, cp, C.c_size_t]
    L.nxs_index_wildcard_batch.restype = C.c_int
    L.nxs_index_wildcard_batch.argtypes = [vp, vp, C.POINTER(cp), C.c_size_t, C.POINTER(vp), C.POINTER(C.c_int)]
    L.nxs_sugg_count.restype = C.c_uint
    L.nxs_sugg_count.argtypes = [vp]
    L.nxs_sugg_matches.restype = C.c_uint64
    L.nxs_sugg_matches.argtypes = [vp]
    L.nxs_sugg_dropped.restype = C.c_bool
    L.nxs_sugg_dropped.argtypes = [vp]
    L.nxs_sugg_get.restype = C.c_bool
    L.nxs_sugg_get.argtypes = [vp, C.c_uint, C.POINTER(vp), C.POINTER(C.c_size_t), C.POINTER(C.c_uint),
                               C.POINTER(C.c_uint64)]
    L.nxs_sugg_tojson.restype = vp
    L.nxs_sugg_tojson.argtypes = [vp, C.POINTER(C.c_size_t)]
    L.nxs_sugg_release.argtypes = [vp]
    # device shim
    L.nxsgpu_device_count.restype = C.c_int
    L.nxsgpu_last_error.restype = cp
    L.nxsgpu_index_df.argtypes = [vp, C.POINTER(C.c_uint32)]
    L.nxsgpu_index_postings.restype = C.c_uint64
    L.nxsgpu_index_postings.argtypes = [vp]
    L.nxsgpu_index_docs.restype = C.c_uint64
    L.nxsgpu_index_docs.argtypes = [vp]
    L.nxsgpu_search.restype = C.c_int
    L.nxsgpu_search.argtypes = [vp, C.c_int, C.c_uint64, C.POINTER(GpuQuery),
                                C.c_uint32, C.POINTER(GpuResults)]
    L.nxsgpu_results_free.argtypes = [C.POINTER(GpuResults)]
    L.nxsgpu_search_dev.restype = C.c_int
    L.nxsgpu_search_dev.argtypes = [vp, C.c_int, C.c_uint32, C.POINTER(GpuQuery),
                                    C.c_uint32, vp, vp, vp]
    L.nxsgpu_search_dev_begin.restype = C.c_int
    L.nxsgpu_search_dev_begin.argtypes = L.nxsgpu_search_dev.argtypes
    L.nxsgpu_search_dev_end.restype = C.c_int
    L.nxsgpu_search_dev_end.argtypes = [vp]
    L.nxsgpu_fuzzy.restype = C.c_int
    L.nxsgpu_fuzzy.argtypes = [vp, cp, C.POINTER(C.c_uint32), C.c_uint32,
                               C.POINTER(C.c_uint32), C.POINTER(C.c_uint64)]
    L.nxsgpu_shard_slice.argtypes = [C.c_uint64, C.c_int, C.c_int,
                                     C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
    L.nxsgpu_shard_capacity.restype = C.c_uint64
    L.nxsgpu_shard_capacity.argtypes = [C.c_uint64, C.c_int]
    L.nxsgpu_batches_in_flight.restype = C.c_int
    L.nxsgpu_batches_in_flight.argtypes = [vp]
    L.nxsgpu_index_reconfigure.argtypes = [vp]
    L.nxsgpu_hbm_read_gbs.restype = C.c_double
    L.nxsgpu_hbm_read_gbs.argtypes = [vp, C.c_int]
    L.nxsgpu_set_profiling.argtypes = [vp, C.c_int]
    L.nxsgpu_get_profile.argtypes = [vp, C.POINTER(GpuProfile), C.c_int]
    L.nxsgpu_synchronize.argtypes = [vp]
    L.nxsgpu_count.restype = C.c_int
    L.nxsgpu_count.argtypes = [vp, C.c_int, C.POINTER(GpuQuery), C.c_uint32, C.POINTER(C.c_uint32)]
    L.nxsgpu_count_tile_widths.argtypes = [C.POINTER(C.c_uint32)]
    L.nxsgpu_count_profile.argtypes = [vp, C.POINTER(C.c_double), C.c_int]
    L.nxsgpu_suggest.restype = C.c_int
    L.nxsgpu_suggest.argtypes = [vp, cp, C.POINTER(C.c_uint32), C.c_uint32, C.c_uint32, C.c_uint32,
                                 C.POINTER(C.c_uint32), C.POINTER(C.c_uint8), C.POINTER(C.c_uint32),
                                 C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]
    L.nxsgpu_suggest_profile.argtypes = [vp, C.POINTER(C.c_double), C.c_int]
    L.nxsgpu_complete.restype = C.c_int
    L.nxsgpu_complete.argtypes = [vp, cp, C.POINTER(C.c_uint32), C.c_uint32, C.c_uint32,
                                  C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), C.POINTER(C.c_uint32),
                                  C.POINTER(C.c_uint32)]
    L.nxsgpu_complete_profile.restype = None
    L.nxsgpu_complete_profile.argtypes = [vp, C.POINTER(C.c_double), C.c_int]
    L.nxsgpu_wildcard.restype = C.c_int
    L.nxsgpu_wildcard.argtypes = [vp, cp, C.POINTER(C.c_uint32), C.c_uint32, C.c_uint32,
                                  C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), C.POINTER(C.c_uint32),
                                  C.POINTER(C.c_uint32)]
    L.nxs_index_doc_terms.restype = vp
    L.nxs_index_doc_terms.argtypes = [vp, vp, C.c_uint64]
    L.nxs_index_doc_terms_batch.restype = C.c_int
    L.nxs_index_doc_terms_batch.argtypes = [vp, vp, C.POINTER(C.c_uint64), C.c_size_t, C.POINTER(vp), C.POINTER(C.c_int)]
    L.nxs_sugg_score.restype = C.c_bool
    L.nxs_sugg_score.argtypes = [vp, C.c_uint, C.POINTER(C.c_float)]
    L.nxs_index_similar.restype = vp
    L.nxs_index_similar.argtypes = [vp, vp, C.c_uint64]
    L.nxs_index_similar_batch.restype = C.c_int
    L.nxs_index_similar_batch.argtypes = [vp, vp, C.POINTER(C.c_uint64), C.c_size_t, C.POINTER(vp), C.POINTER(C.c_int)]
    L.nxsgpu_doc_terms.restype = C.c_int
    L.nxsgpu_doc_terms.argtypes = [vp, C.c_int, C.POINTER(C.c_uint64), C.c_uint32, C.c_uint32, C.c_uint32,
                                   C.POINTER(C.c_uint32), C.POINTER(C.c_float), C.POINTER(C.c_uint32),
                                   C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), C.POINTER(C.c_uint32),
                                   C.POINTER(C.c_uint8)]
    L.nxsgpu_doc_terms_profile.restype = None
    L.nxsgpu_doc_terms_profile.argtypes = [vp, C.POINTER(C.c_double), C.c_int]
    if hasattr(L, "nxs_test_docterms_params"):
        L.nxs_test_docterms_params.restype = C.c_int
        L.nxs_test_docterms_params.argtypes = [vp, vp, C.POINTER(C.c_uint), C.POINTER(C.c_uint), C.POINTER(C.c_uint),
                                               C.POINTER(C.c_uint), C.POINTER(C.c_int)]
        L.nxs_test_docterms_build.restype = vp
        L.nxs_test_docterms_build.argtypes = [C.c_uint64, C.c_uint64, C.c_uint, C.POINTER(C.c_char_p),
                                              C.POINTER(C.c_size_t), C.POINTER(C.c_uint), C.POINTER(C.c_uint64),
                                              C.POINTER(C.c_float)]
        L.nxs_test_docterms_lane.restype = C.c_int
        L.nxs_test_docterms_lane.argtypes = [C.POINTER(C.c_uint64), C.c_uint64, C.c_bool, C.c_uint32,
                                             C.POINTER(C.c_uint32), C.c_uint32, C.c_int, C.POINTER(C.c_uint64)]
        L.nxs_test_docterms_key.restype = C.c_uint64
        L.nxs_test_docterms_key.argtypes = [C.c_float, C.c_uint32]
        L.nxs_test_similar_drop.restype = None
        L.nxs_test_similar_drop.argtypes = [vp, C.c_uint64, C.c_uint64]
    L.nxs_index_related.restype = vp
    L.nxs_index_related.argtypes = [vp, vp, C.c_char_p, C.c_size_t]
    L.nxs_index_related_batch.restype = C.c_int
    L.nxs_index_related_batch.argtypes = [vp, vp, C.POINTER(C.c_char_p), C.c_size_t, C.POINTER(vp), C.POINTER(C.c_int)]
    L.nxs_sugg_docs.restype = C.c_bool
    L.nxs_sugg_docs.argtypes = [vp, C.POINTER(C.c_uint64)]
    u32p = C.POINTER(C.c_uint32)
    L.nxsgpu_related.restype = C.c_int
    L.nxsgpu_related.argtypes = [vp, C.c_int, C.POINTER(GpuQuery), C.c_uint32, C.c_int, C.c_uint32, C.c_uint32, C.c_int,
                                 C.c_uint32, u32p, u32p, u32p, u32p, u32p, u32p]
    L.nxsgpu_related_profile.restype = None
    L.nxsgpu_related_profile.argtypes = [vp, C.POINTER(C.c_double), C.c_int]
    if hasattr(L, "nxs_test_related_params"):
        L.nxs_test_related_params.restype = C.c_int
        L.nxs_test_related_params.argtypes = [vp, vp, C.POINTER(C.c_uint), C.POINTER(C.c_int), C.POINTER(C.c_uint),
                                              C.POINTER(C.c_uint), C.POINTER(C.c_int)]
        L.nxs_test_related_build.restype = vp
        L.nxs_test_related_build.argtypes = [C.c_char_p, C.c_size_t, C.c_uint64, C.c_uint64, C.c_uint,
                                             C.POINTER(C.c_char_p), C.POINTER(C.c_size_t), C.POINTER(C.c_uint),
                                             C.POINTER(C.c_uint64)]
        L.nxs_test_related_key.restype = C.c_uint64
        L.nxs_test_related_key.argtypes = [C.c_int, C.c_uint32, C.c_uint32, C.c_uint32]
        L.nxs_test_related_share.restype = C.c_float
        L.nxs_test_related_share.argtypes = [C.c_uint32, C.c_uint32]
        L.nxs_test_related_eligible.restype = C.c_bool
        L.nxs_test_related_eligible.argtypes = [C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, u32p, C.c_uint32]
        L.nxs_test_related_rank.restype = C.c_int
        L.nxs_test_related_rank.argtypes = [C.c_int, u32p, u32p, C.c_uint32, C.c_uint32, C.c_uint32, u32p, C.c_uint32,
                                            C.c_uint32, u32p, C.POINTER(C.c_uint64)]
    u64p = C.POINTER(C.c_uint64)
    L.nxs_index_search_docs.restype = vp
    L.nxs_index_search_docs.argtypes = [vp, vp, C.c_char_p, C.c_size_t, u64p, C.c_size_t]
    L.nxs_index_search_docs_batch.restype = C.c_int
    L.nxs_index_search_docs_batch.argtypes = [vp, vp, C.POINTER(C.c_char_p), C.c_size_t, C.POINTER(u64p),
                                              C.POINTER(C.c_size_t), C.POINTER(vp), C.POINTER(C.c_int)]
    L.nxsgpu_search_docs.restype = C.c_int
    L.nxsgpu_search_docs.argtypes = [vp, C.c_int, C.c_uint64, C.POINTER(GpuQuery), C.c_uint32, C.POINTER(u64p), u32p,
                                     C.c_uint32, u32p, C.POINTER(GpuResults), u32p]
    L.nxsgpu_search_docs_profile.restype = None
    L.nxsgpu_search_docs_profile.argtypes = [vp, C.POINTER(C.c_double), C.c_int]
    L.nxs_index_match_docs.restype = vp
    L.nxs_index_match_docs.argtypes = [vp, vp, C.c_char_p, C.c_size_t]
    L.nxs_index_match_docs_batch.restype = C.c_int
    L.nxs_index_match_docs_batch.argtypes = [vp, vp, C.POINTER(C.c_char_p), C.c_size_t, u64p, C.POINTER(vp),
                                             C.POINTER(C.c_int)]
    L.nxs_docs_count.restype = C.c_size_t
    L.nxs_docs_count.argtypes = [vp]
    L.nxs_docs_ids.restype = u64p
    L.nxs_docs_ids.argtypes = [vp]
    L.nxs_docs_total.restype = C.c_uint64
    L.nxs_docs_total.argtypes = [vp]
    L.nxs_docs_next.restype = C.c_bool
    L.nxs_docs_next.argtypes = [vp, u64p]
    L.nxs_docs_tojson.restype = vp
    L.nxs_docs_tojson.argtypes = [vp, C.POINTER(C.c_size_t)]
    L.nxs_docs_release.restype = None
    L.nxs_docs_release.argtypes = [vp]
    L.nxsgpu_match_docs.restype = C.c_int
    L.nxsgpu_match_docs.argtypes = [vp, C.c_int, C.POINTER(GpuQuery), C.c_uint32, u64p, C.c_uint32, u64p, u32p,
                                    C.POINTER(C.c_uint8), u32p]
    L.nxsgpu_match_docs_profile.restype = None
    L.nxsgpu_match_docs_profile.argtypes = [vp, C.POINTER(C.c_double), C.c_int]
    if hasattr(L, "nxs_test_match_params"):
        L.nxs_test_match_params.restype = C.c_int
        L.nxs_test_match_params.argtypes = [vp, vp, C.POINTER(C.c_uint), u64p]
        L.nxs_test_docs_build.restype = vp
        L.nxs_test_docs_build.argtypes = [C.c_char_p, u64p, C.c_size_t, C.c_uint64, C.c_bool]
        L.nxs_test_md_lower_bound.restype = C.c_uint64
        L.nxs_test_md_lower_bound.argtypes = [u64p, C.c_uint64, C.c_uint64]
        L.nxs_test_md_page.restype = C.c_uint64
        L.nxs_test_md_page.argtypes = [u32p, u64p, C.c_uint64, C.c_uint64, C.c_uint64, u64p, C.POINTER(C.c_bool)]
    if hasattr(L, "nxs_test_docset_sort"):
        L.nxs_test_docset_sort.restype = C.c_size_t
        L.nxs_test_docset_sort.argtypes = [u64p, C.c_size_t]
        L.nxs_test_docset_lane.restype = C.c_int
        L.nxs_test_docset_lane.argtypes = [u64p, C.POINTER(C.c_float), u64p, C.c_uint32, C.c_bool, C.c_uint32, u32p,
                                           C.POINTER(C.c_uint8), C.c_uint32, u32p, C.c_size_t, C.POINTER(C.c_uint8),
                                           C.POINTER(C.c_float)]
    L.nxsgpu_wildcard_profile.restype = None
    L.nxsgpu_wildcard_profile.argtypes = [vp, C.POINTER(C.c_double), C.c_int]
    L.nxsgpu_explain_profile.restype = None
    L.nxsgpu_explain_profile.argtypes = [vp, C.POINTER(C.c_double), C.c_int]
    # host-only test hooks
    L.nxs_test_query_repr.restype = vp
    L.nxs_test_query_repr.argtypes = [cp, C.POINTER(vp)]
    L.nxs_query_lex.restype = C.c_int
    L.nxs_query_lex.argtypes = [cp, C.POINTER(C.c_int), C.c_size_t]
    L.nxs_test_compile.restype = C.c_int
    L.nxs_test_compile.argtypes = [cp, C.POINTER(cp), C.c_uint32, C.c_bool,
                                   C.POINTER(GpuQuery), C.POINTER(C.c_int),
                                   cp, C.c_size_t]
    L.nxs_test_compile_wide.restype = C.c_int
    L.nxs_test_compile_wide.argtypes = [cp, C.POINTER(cp), C.c_uint32, C.POINTER(C.c_int),
                                        C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), C.c_uint32,
                                        C.POINTER(C.c_uint32), C.POINTER(C.c_uint16), C.c_uint32]
    L.nxs_test_bk_image.restype = C.c_int
    L.nxs_test_bk_image.argtypes = [C.POINTER(cp), C.c_uint32, C.POINTER(BkImage)]
    L.nxs_bk_free.argtypes = [C.POINTER(BkImage)]
    L.nxs_test_levdist.restype = C.c_int
    L.nxs_test_levdist.argtypes = [cp, C.c_size_t, cp, C.c_size_t]
    _lib = L
    return L


_libc = C.CDLL(None)
_libc.free.argtypes = [C.c_void_p]


def _take(ptr):
    if not ptr:
        return None
    s = C.string_at(ptr).decode("utf-8", "surrogateescape")
    _libc.free(ptr)
    return s


def _b(s):
    return s.encode("utf-8", "surrogateescape") if isinstance(s, str) else s


class Nxs:
    """`nxs_t`: a library instance bound to a base directory."""

    def __init__(self, basedir):
        self._h = lib().nxs_open(os.fsencode(basedir))
        if not self._h:
            raise NxsError(2, "nxs_open(%r) failed" % (basedir,))

    def error(self):
        msg = C.c_char_p()
        code = lib().nxs_get_error(self._h, C.byref(msg))
        return code, (msg.value or b"").decode("utf-8", "replace")

    def _raise(self):
        raise NxsError(*self.error())

    def open_index(self, name):
        h = lib().nxs_index_open(self._h, _b(name))
        if not h:
            self._raise()
        return Index(self, h)

    def open_files(self, terms_path, dtmap_path, algo="BM25", lowercase=False):
        h = lib().nxs_index_open_files(self._h, os.fsencode(terms_path),
                                       os.fsencode(dtmap_path), _b(algo), lowercase)
        if not h:
            self._raise()
        return Index(self, h)

    def open_shard(self, terms_path, dtmap_path, shard, n_shards, algo="BM25", lowercase=False,
                   device=-1):
        """nxs_index_open_shard(): shard `shard` of a doc-sharded collection (N4)."""
        L = lib()
        L.nxs_index_open_shard.restype = C.c_void_p
        L.nxs_index_open_shard.argtypes = [C.c_void_p, C.c_char_p, C.c_char_p, C.c_char_p, C.c_bool,
                                           C.c_uint, C.c_uint, C.c_int]
        h = L.nxs_index_open_shard(self._h, os.fsencode(terms_path), os.fsencode(dtmap_path),
                                   _b(algo), lowercase, shard, n_shards, device)
        if not h:
            self._raise()
        return Index(self, h)

    def docshard_search_batch(self, shards, queries, limit=None, algo=None, fuzzymatch=None, total=False,
                              prefixmatch=None, explain=False, wildcardmatch=None):
        """nxs_docshard_search_batch(): one batch over all shards, merged exactly.
        total: every result list also carries `.total` (the sum of the shards' counts).
        (prefixmatch / wildcardmatch: a batch with a prefix / wildcard leaf is refused -- NXS_ERR_INVALID.)
        explain: every list carries `.tokens` and `.explain` (each row from the shard that holds the doc)."""
        L = lib()
        L.nxs_docshard_search_batch.restype = C.c_int
        L.nxs_docshard_search_batch.argtypes = [C.POINTER(C.c_void_p), C.c_uint, C.c_void_p,
                                                C.POINTER(C.c_char_p), C.c_size_t,
                                                C.POINTER(C.c_void_p), C.POINTER(C.c_int)]
        n = len(queries)
        hs = (C.c_void_p * len(shards))(*[s._h for s in shards])
        qs = (C.c_char_p * max(n, 1))(*[_b(q) for q in queries])
        resps = (C.c_void_p * max(n, 1))()
        errs = (C.c_int * max(n, 1))()
        p = _make_params(limit, algo, fuzzymatch, total, prefixmatch, explain=explain, wildcardmatch=wildcardmatch)
        try:
            r = L.nxs_docshard_search_batch(hs, len(shards), p, qs, n, resps, errs)
        finally:
            if p:
                L.nxs_params_release(p)
        if r < 0:
            self._raise()
        out = []
        for i in range(n):
            if resps[i]:
                out.append(_drain(resps[i], explain))
                L.nxs_resp_release(resps[i])
            else:
                out.append(NxsError(errs[i], "query %d failed" % i))
        return out

    def _collect(self, r, n, resps, errs):
        L = lib()
        if r < 0:
            self._raise()
        out = []
        for i in range(n):
            if resps[i]:
                out.append(_drain(resps[i]))
                L.nxs_resp_release(resps[i])
            else:
                out.append(NxsError(errs[i], "query %d failed" % i))
        return out

    def docshard_search_batch_rank(self, shard, queries, limit=None, algo=None, fuzzymatch=None, total=False,
                                   explain=False):
        """nxs_docshard_search_batch_rank(): this rank's shard + one all-gather + merge.
        (total, explain: refused -- NXS_ERR_INVALID.)"""
        L = lib()
        L.nxs_docshard_search_batch_rank.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(C.c_char_p), C.c_size_t,
                                                     C.POINTER(C.c_void_p), C.POINTER(C.c_int)]
        n = len(queries)
        qs = (C.c_char_p * max(n, 1))(*[_b(q) for q in queries])
        resps, errs = (C.c_void_p * max(n, 1))(), (C.c_int * max(n, 1))()
        p = _make_params(limit, algo, fuzzymatch, total, explain=explain)
        try:
            r = L.nxs_docshard_search_batch_rank(shard._h, p, qs, n, resps, errs)
        finally:
            if p:
                L.nxs_params_release(p)
        return self._collect(r, n, resps, errs)

    def docshard_attach(self, shard):
        """nxs_docshard_attach(): collective; collection-wide df for this rank's shard."""
        L = lib()
        L.nxs_docshard_attach.argtypes = [C.c_void_p]
        if L.nxs_docshard_attach(shard._h) != 0:
            self._raise()

    def docshard_emulated_ranks(self, shards, queries, cap=512, limit=None, algo=None, fuzzymatch=None):
        """tests: the one-process-per-shard form with the ranks played one after the
        other on this GPU -- every rank's candidate block (nxs_test_docshard_block),
        the blocks concatenated as the all-gather would, then every rank's merge
        (nxs_test_docshard_finish).  -> one result list per rank."""
        L = lib()
        vp = C.c_void_p
        L.nxs_test_docshard_set_df.argtypes = [C.POINTER(vp), C.c_uint]
        L.nxs_test_docshard_block.argtypes = [vp, vp, C.POINTER(C.c_char_p), C.c_size_t, C.c_uint32,
                                              C.POINTER(C.POINTER(C.c_uint8)), C.POINTER(C.c_size_t)]
        L.nxs_test_docshard_finish.argtypes = [vp, vp, C.POINTER(C.c_char_p), C.c_size_t, C.c_uint32,
                                               C.c_char_p, C.POINTER(vp), C.POINTER(C.c_int)]
        libc = C.CDLL(None)
        libc.free.argtypes = [C.c_void_p]
        hs = (vp * len(shards))(*[s._h for s in shards])
        if L.nxs_test_docshard_set_df(hs, len(shards)) != 0:
            self._raise()
        n = len(queries)
        qs = (C.c_char_p * max(n, 1))(*[_b(q) for q in queries])
        p = _make_params(limit, algo, fuzzymatch)
        try:
            gathered = b""
            for sh in shards:
                blk, ln = C.POINTER(C.c_uint8)(), C.c_size_t()
                if L.nxs_test_docshard_block(sh._h, p, qs, n, cap, C.byref(blk), C.byref(ln)) != 0:
                    self._raise()
                gathered += C.string_at(blk, ln.value)
                libc.free(blk)
            outs = []
            for sh in shards:
                resps, errs = (vp * max(n, 1))(), (C.c_int * max(n, 1))()
                r = L.nxs_test_docshard_finish(sh._h, p, qs, n, cap, gathered, resps, errs)
                outs.append(self._collect(r, n, resps, errs))
        finally:
            if p:
                L.nxs_params_release(p)
        return outs

    def docshard_refresh(self, shards):
        """nxs_docshard_refresh(): every shard of the collection follows the files to
        one snapshot.  -> True if anything had moved."""
        L = lib()
        L.nxs_docshard_refresh.argtypes = [C.POINTER(C.c_void_p), C.c_uint]
        hs = (C.c_void_p * len(shards))(*[s._h for s in shards])
        r = L.nxs_docshard_refresh(hs, len(shards))
        if r < 0:
            self._raise()
        return r == 1

    def docshard_refresh_rank(self, shard):
        """nxs_docshard_refresh_rank(): collective; this rank's shard follows the files."""
        L = lib()
        L.nxs_docshard_refresh_rank.argtypes = [C.c_void_p]
        r = L.nxs_docshard_refresh_rank(shard._h)
        if r < 0:
            self._raise()
        return r == 1

    def docshard_emulated_refresh(self, shards, after_record=None):
        """tests: nxs_docshard_refresh_rank() with the ranks played one after the other on
        this GPU and the collectives done here -- every rank's snapshot record
        (after_record(rank) runs after each), every rank's merge and df block, every
        rank's impact pass on the gathered blocks, every rank's outcome.  -> the value
        each rank returns (1 / 0 / -1)."""
        L = lib()
        vp = C.c_void_p
        u64p = C.POINTER(C.c_uint64)
        L.nxs_test_docshard_refresh_record.argtypes = [vp, u64p]
        L.nxs_test_docshard_refresh_merge.argtypes = [vp, u64p, C.c_uint, C.POINTER(C.POINTER(C.c_uint8)),
                                                      C.POINTER(C.c_size_t)]
        L.nxs_test_docshard_refresh_finish.restype = C.c_uint32
        L.nxs_test_docshard_refresh_finish.argtypes = [vp, C.c_char_p, C.c_uint, C.c_size_t]
        L.nxs_test_docshard_refresh_settle.argtypes = [vp, C.POINTER(C.c_uint32), C.c_uint]
        libc = C.CDLL(None)
        libc.free.argtypes = [C.c_void_p]
        W = len(shards)
        recs = (C.c_uint64 * (8 * W))()
        for r, sh in enumerate(shards):
            L.nxs_test_docshard_refresh_record(sh._h, C.cast(C.byref(recs, 8 * 8 * r), u64p))
            if after_record:
                after_record(r)
        rets, blocks = [], []
        for sh in shards:
            blk, ln = C.POINTER(C.c_uint8)(), C.c_size_t()
            rets.append(L.nxs_test_docshard_refresh_merge(sh._h, recs, W, C.byref(blk), C.byref(ln)))
            blocks.append(C.string_at(blk, ln.value) if blk else b"")
            libc.free(blk)
        if any(x <= 0 for x in rets):
            assert len(set(rets)) == 1, rets       # the agreement is the same on every rank
            return rets
        assert len(set(len(b) for b in blocks)) == 1
        gathered = b"".join(blocks)
        fin = (C.c_uint32 * W)(*[L.nxs_test_docshard_refresh_finish(sh._h, gathered, W, len(blocks[0]))
                                 for sh in shards])
        return [L.nxs_test_docshard_refresh_settle(sh._h, fin, W) for sh in shards]

    def shard_unique_id(self):
        """nxs_shard_unique_id(): the bytes rank 0 hands to the other ranks."""
        buf = C.create_string_buffer(128)
        if lib().nxs_shard_unique_id(self._h, buf) != 0:
            self._raise()
        return buf.raw

    def close(self):
        if self._h:
            lib().nxs_close(self._h)
            self._h = None

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()


class Results(list):
    """The result list of a search that asked for the total match count: a list like any
    other, with `.total` = how many docs matched (nxs_resp_total).  Of a search that asked for explanations:
    `.tokens` = the dictionary terms the query's token list resolved to ([bytes, ...], nxs_resp_token) and
    `.explain` = per result the present tokens [(j, tf, score), ...] in ascending j (nxs_resp_explain); both
    empty if nothing matched."""
    total = None
    tokens = None
    explain = None


class Suggestions(list):
    """The suggestions for one token (nxs_sugg_t): [(term: bytes, distance, df), ...] best first, with
    `.matches` = the exact number of eligible terms and `.dropped` = the filters dropped the token (a stop
    word)."""
    matches = 0
    dropped = False


class DocTerms(list):
    """The term vector of one doc (nxs_sugg_t of nxs_index_doc_terms): [(term: bytes, tf, df, score), ...] best
    first, with `.matches` = the exact number of eligible terms."""
    matches = 0


def _drain_docterms(sg, json=False):
    """nxs_sugg_t of the term-vector kind -> DocTerms (or its JSON text); releases the object"""
    L = lib()
    try:
        if json:
            n = C.c_size_t()
            return _take(L.nxs_sugg_tojson(sg, C.byref(n)))
        out = DocTerms()
        term, ln, tf, df, sc = C.c_void_p(), C.c_size_t(), C.c_uint(), C.c_uint64(), C.c_float()
        i = 0
        while L.nxs_sugg_get(sg, i, C.byref(term), C.byref(ln), C.byref(tf), C.byref(df)):
            assert L.nxs_sugg_score(sg, i, C.byref(sc))
            out.append((C.string_at(term.value, ln.value), tf.value, df.value, sc.value))
            i += 1
        assert i == L.nxs_sugg_count(sg) and not L.nxs_sugg_dropped(sg)
        out.matches = L.nxs_sugg_matches(sg)
        return out
    finally:
        L.nxs_sugg_release(sg)


class Related(list):
    """The related terms of one query (nxs_sugg_t of nxs_index_related): [(term: bytes, count, df, score), ...]
    best first, with `.matches` = the exact number of eligible terms and `.docs` = the size of the query's doc
    set."""
    matches = 0
    docs = 0


def _drain_related(sg, json=False):
    """nxs_sugg_t of the related kind -> Related (or its JSON text); releases the object"""
    L = lib()
    try:
        if json:
            n = C.c_size_t()
            return _take(L.nxs_sugg_tojson(sg, C.byref(n)))
        out = Related()
        term, ln, c, df, sc, docs = C.c_void_p(), C.c_size_t(), C.c_uint(), C.c_uint64(), C.c_float(), C.c_uint64()
        i = 0
        while L.nxs_sugg_get(sg, i, C.byref(term), C.byref(ln), C.byref(c), C.byref(df)):
            assert L.nxs_sugg_score(sg, i, C.byref(sc))
            out.append((C.string_at(term.value, ln.value), c.value, df.value, sc.value))
            i += 1
        assert i == L.nxs_sugg_count(sg) and not L.nxs_sugg_dropped(sg) and L.nxs_sugg_docs(sg, C.byref(docs))
        out.matches = L.nxs_sugg_matches(sg)
        out.docs = docs.value
        return out
    finally:
        L.nxs_sugg_release(sg)


class Docs(list):
    """A page of a query's matches (nxs_docs_t of nxs_index_match_docs): doc ids, ascending, with `.total` = the
    size of the query's doc set whatever the cursor and `.next` = the cursor of the next page (None: the set is
    exhausted)."""
    total = 0
    next = None


def _drain_docs(d, json=False):
    """nxs_docs_t -> Docs (or its JSON text); releases the object"""
    L = lib()
    try:
        if json:
            n = C.c_size_t()
            return _take(L.nxs_docs_tojson(d, C.byref(n)))
        out = Docs()
        n = L.nxs_docs_count(d)
        if n:
            import numpy as np
            out.extend(np.ctypeslib.as_array(L.nxs_docs_ids(d), shape=(n,)).tolist())
        out.total = L.nxs_docs_total(d)
        nxt = C.c_uint64()
        out.next = nxt.value if L.nxs_docs_next(d, C.byref(nxt)) else None
        return out
    finally:
        L.nxs_docs_release(d)


def _drain_sugg(sg, json=False):
    """nxs_sugg_t -> Suggestions (or its JSON text); releases the object"""
    L = lib()
    try:
        if json:
            n = C.c_size_t()
            return _take(L.nxs_sugg_tojson(sg, C.byref(n)))
        out = Suggestions()
        term, ln, d, df = C.c_void_p(), C.c_size_t(), C.c_uint(), C.c_uint64()
        i = 0
        while L.nxs_sugg_get(sg, i, C.byref(term), C.byref(ln), C.byref(d), C.byref(df)):
            out.append((C.string_at(term.value, ln.value), d.value, df.value))
            i += 1
        assert i == L.nxs_sugg_count(sg)
        out.matches = L.nxs_sugg_matches(sg)
        out.dropped = bool(L.nxs_sugg_dropped(sg))
        return out
    finally:
        L.nxs_sugg_release(sg)


def _suggest_params(limit=None, maxdist=None):
    if limit is None and maxdist is None:
        return None
    L = lib()
    p = L.nxs_params_create()
    if limit is not None:
        L.nxs_params_set_uint(p, b"suggest_limit", limit)
    if maxdist is not None:
        L.nxs_params_set_uint(p, b"suggest_maxdist", maxdist)
    return p


def _make_params(limit=None, algo=None, fuzzymatch=None, total=False, prefixmatch=None, prefix_limit=None,
                 explain=False, wildcardmatch=None, wildcard_terms=None):
    if limit is None and algo is None and fuzzymatch is None and not total and prefixmatch is None \
            and prefix_limit is None and not explain and wildcardmatch is None and wildcard_terms is None:
        return None
    L = lib()
    p = L.nxs_params_create()
    if limit is not None:
        L.nxs_params_set_uint(p, b"limit", limit)
    if algo is not None:
        L.nxs_params_set_str(p, b"algo", _b(algo))
    if fuzzymatch is not None:
        L.nxs_params_set_bool(p, b"fuzzymatch", bool(fuzzymatch))
    if total:
        L.nxs_params_set_bool(p, b"total", True)
    if prefixmatch is not None:
        L.nxs_params_set_bool(p, b"prefixmatch", bool(prefixmatch))
    if prefix_limit is not None:
        L.nxs_params_set_uint(p, b"prefix_limit", prefix_limit)
    if explain:
        L.nxs_params_set_bool(p, b"explain", True)
    if wildcardmatch is not None:
        L.nxs_params_set_bool(p, b"wildcardmatch", bool(wildcardmatch))
    if wildcard_terms is not None:
        L.nxs_params_set_uint(p, b"wildcard_terms", wildcard_terms)
    return p


def _drain(resp, explain=False):
    L = lib()
    out = []
    d, s = C.c_uint64(), C.c_float()
    L.nxs_resp_iter_reset(resp)
    while L.nxs_resp_iter_result(resp, C.byref(d), C.byref(s)):
        out.append((d.value, s.value))
    assert len(out) == L.nxs_resp_resultcount(resp)
    t = C.c_uint64()
    if L.nxs_resp_total(resp, C.byref(t)):
        out = Results(out)
        out.total = t.value
    m = L.nxs_resp_tokens(resp)
    if explain or m:
        if not isinstance(out, Results):
            out = Results(out)
        term, ln, sc, tf = C.c_void_p(), C.c_size_t(), C.c_float(), C.c_uint32()
        out.tokens = []
        for j in range(m):
            assert L.nxs_resp_token(resp, j, C.byref(term), C.byref(ln))
            out.tokens.append(C.string_at(term.value, ln.value))
        out.explain = []
        for i in range(len(out)):
            row = []
            for j in range(m):
                if L.nxs_resp_explain(resp, i, j, C.byref(sc), C.byref(tf)):
                    row.append((j, tf.value, sc.value))
            out.explain.append(row)
    return out


class Index:
    """`nxs_index_t` opened for searching on the GPU."""

    def __init__(self, nxs, h):
        self.nxs = nxs
        self._h = h

    @property
    def device(self):
        return lib().nxs_index_device(self._h)

    def search(self, query, limit=None, algo=None, fuzzymatch=None, json=False, params_json=None, total=False,
               prefixmatch=None, prefix_limit=None, explain=False, wildcardmatch=None, wildcard_terms=None):
        """nxs_index_search(): -> [(doc_id, score), ...] (or the JSON text).
        params_json: the parameters as the Lua binding passes them (nxs_params_fromjson).
        total: also count the matches -- the list then carries `.total` (the JSON a "total" member).
        prefixmatch: a free-form leaf `term*` stands for the OR of its `prefix_limit` (1..32, default 8) best
        completions.
        wildcardmatch: a free-form leaf with a `*` / `?` (and another byte) stands for the OR of its
        `wildcard_terms` (1..32, default 8) best matching terms.
        explain: the list also carries `.tokens` and `.explain` (class Results; the JSON "terms" / "tokens")."""
        L = lib()
        if params_json is not None:
            pj = _b(params_json)
            p = L.nxs_params_fromjson(self.nxs._h, pj, len(pj))
            if not p:
                self.nxs._raise()
        else:
            p = _make_params(limit, algo, fuzzymatch, total, prefixmatch, prefix_limit, explain, wildcardmatch, wildcard_terms)
        q = _b(query)
        try:
            resp = L.nxs_index_search(self._h, p, q, len(q))
        finally:
            if p:
                L.nxs_params_release(p)
        if not resp:
            self.nxs._raise()
        try:
            if json:
                n = C.c_size_t()
                return _take(L.nxs_resp_tojson(resp, C.byref(n)))
            return _drain(resp, explain)
        finally:
            L.nxs_resp_release(resp)

    def search_batch(self, queries, limit=None, algo=None, fuzzymatch=None, total=False,
                     prefixmatch=None, prefix_limit=None, explain=False, wildcardmatch=None, wildcard_terms=None):
        """nxs_index_search_batch(): list of result lists; a failed query
        yields an NxsError instance in its slot.  total: every list carries `.total`; explain: `.tokens` and
        `.explain`."""
        L = lib()
        n = len(queries)
        qs = (C.c_char_p * n)(*[_b(q) for q in queries])
        resps = (C.c_void_p * n)()
        errs = (C.c_int * n)()
        p = _make_params(limit, algo, fuzzymatch, total, prefixmatch, prefix_limit, explain, wildcardmatch, wildcard_terms)
        try:
            r = L.nxs_index_search_batch(self._h, p, qs, n, resps, errs)
        finally:
            if p:
                L.nxs_params_release(p)
        if r < 0:
            self.nxs._raise()
        out = []
        for i in range(n):
            if resps[i]:
                out.append(_drain(resps[i], explain))
                L.nxs_resp_release(resps[i])
            else:
                out.append(NxsError(errs[i], "query %d failed" % i))
        return out

    def search_batch_begin(self, queries, limit=None, algo=None, fuzzymatch=None, total=False,
                           prefixmatch=None, prefix_limit=None, explain=False, wildcardmatch=None,
                           wildcard_terms=None):
        """nxs_index_search_batch_begin(): queue a batch (at most NXS_BATCHES_INFLIGHT = 4 in flight).
        total: the lists search_batch_end() returns for this batch carry `.total`; explain: `.tokens` and
        `.explain`."""
        L = lib()
        n = len(queries)
        qs = (C.c_char_p * max(n, 1))(*[_b(q) for q in queries])
        p = _make_params(limit, algo, fuzzymatch, total, prefixmatch, prefix_limit, explain, wildcardmatch, wildcard_terms)
        try:
            r = L.nxs_index_search_batch_begin(self._h, p, qs, n)
        finally:
            if p:
                L.nxs_params_release(p)
        if r != 0:
            self.nxs._raise()
        self._pending = getattr(self, "_pending", []) + [n]
        self._pending_explain = getattr(self, "_pending_explain", []) + [bool(explain)]

    def search_batch_end(self):
        """nxs_index_search_batch_end(): the oldest batch's result lists."""
        L = lib()
        pend = getattr(self, "_pending", [])
        n = pend[0] if pend else 1
        resps = (C.c_void_p * max(n, 1))()
        errs = (C.c_int * max(n, 1))()
        r = L.nxs_index_search_batch_end(self._h, resps, errs)
        if r < 0:
            self.nxs._raise()
        self._pending = pend[1:]
        pex = getattr(self, "_pending_explain", [])
        if len(pex) != len(pend):       # (a caller edited _pending: the flag only matters for empty results)
            pex = [False] * len(pend)
        explain = pex[0] if pex else False
        self._pending_explain = pex[1:]
        out = []
        for i in range(n):
            if resps[i]:
                out.append(_drain(resps[i], explain))
                L.nxs_resp_release(resps[i])
            else:
                out.append(NxsError(errs[i], "query %d failed" % i))
        return out

    def shard(self, rank, world, uid):
        """nxs_index_shard(): collective; `uid` from shard_unique_id() of rank 0."""
        if lib().nxs_index_shard(self._h, rank, world, uid) != 0:
            self.nxs._raise()

    def shard_local(self, on=True):
        """nxs_index_shard_local(): responses of the own slice only (others None)."""
        L = lib()
        L.nxs_index_shard_local.argtypes = [C.c_void_p, C.c_bool]
        if L.nxs_index_shard_local(self._h, on) != 0:
            self.nxs._raise()

    def shard_slice(self, n):
        """nxs_index_shard_slice(): the part of an n-query batch whose responses this index delivers."""
        lo, hi = C.c_size_t(), C.c_size_t()
        L = lib()
        L.nxs_index_shard_slice.argtypes = [C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t), C.POINTER(C.c_size_t)]
        L.nxs_index_shard_slice(self._h, n, C.byref(lo), C.byref(hi))
        return lo.value, hi.value

    def shard_info(self):
        """What the attached communicator is and has carried (bench evidence): RCCL's own rank count
        (ncclCommCount), the library's world, all-gathers queued, bytes this rank contributed."""
        out = (C.c_uint64 * 4)()
        L = lib()
        L.nxs_index_shard_info.argtypes = [C.c_void_p, C.POINTER(C.c_uint64)]
        L.nxs_index_shard_info(self._h, out)
        return {"rccl_ranks": int(C.c_int64(out[0]).value), "world": int(out[1]), "allgathers": int(out[2]),
                "bytes_contributed": int(out[3])}

    def host_profile(self):
        """nxs_index_host_profile(): per-batch host phase times in ms."""
        out = (C.c_double * 12)()
        L = lib()
        L.nxs_index_host_profile.argtypes = [C.c_void_p, C.POINTER(C.c_double)]
        L.nxs_index_host_profile(self._h, out)
        n = max(out[4], 1.0)
        return {"plan_ms": round(1e3 * out[0] / n, 4), "queue_ms": round(1e3 * out[1] / n, 4),
                "wait_ms": round(1e3 * out[2] / n, 4), "resps_ms": round(1e3 * out[3] / n, 4),
                "begin_ms": round(1e3 * out[6] / n, 4), "end_ms": round(1e3 * out[7] / n, 4),
                "fuzzy_wait_ms": round(1e3 * out[8] / n, 4), "front_ms": round(1e3 * out[9] / n, 4),
                "fuzzy_launch_ms": round(1e3 * out[10] / n, 4), "back_ms": round(1e3 * out[11] / n, 4),
                "batches": int(out[4]), "exact_requeries": int(out[5])}

    def device_image(self, algos=(0, 1)):
        """nxs_test_index_image(): the device index read back as numpy arrays, for the tests that compare it
        with a host model.  -> {"scalars": {...}, name: array, ...}; the parts of a ranking function are keyed
        (name, algo) with algo 0 = TF-IDF, 1 = BM25.  A part that is not materialised is an empty array;
        "df_global" (a doc shard's collection-wide df) is None on an index that is not a shard.
        Postings are structured arrays (doc u32, imp u32 = the f32's bits).  Not while batches are in flight."""
        import numpy as np
        L = lib()
        L.nxs_test_index_image.restype = C.c_int
        L.nxs_test_index_image.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t)]

        def part(no, dtype, algo=0):
            need = C.c_size_t()
            if L.nxs_test_index_image(self._h, no, algo, None, 0, C.byref(need)) != 0:
                self.nxs._raise()
            buf = np.empty(need.value, dtype=np.uint8)
            if need.value:
                got = C.c_size_t()
                if L.nxs_test_index_image(self._h, no, algo, buf.ctypes.data, buf.nbytes, C.byref(got)) != 0:
                    self.nxs._raise()
                assert got.value == need.value, (no, algo, got.value, need.value)
            return buf.view(dtype)

        raw = part(IMG_SCALARS, np.uint64)
        sc = {name: int(raw[i]) for i, name in enumerate(IMG_SCALAR_NAMES)}
        sc["scanm_dens"] = float(raw[9:10].view(np.float64)[0])
        out = {"scalars": sc}
        post_t = np.dtype([("doc", "<u4"), ("imp", "<u4")])
        for name, (no, dtype) in IMG_PARTS.items():
            dtype = post_t if dtype == "post" else np.dtype(dtype)
            if no in IMG_PER_ALGO:
                for a in algos:
                    out[(name, a)] = part(no, dtype, a)
            else:
                out[name] = part(no, dtype)
        if sc["dense_q8_stride"] and len(out["dense_q8"]):
            out["dense_q8"] = out["dense_q8"].reshape(-1, sc["dense_q8_stride"])
        dfg = part(IMG_DF_GLOBAL, np.dtype("<u4"))
        out["df_global"] = dfg if dfg.size else None
        return out

    def term_image(self):
        """nxs_test_term_image(): the term-side device state read back as numpy arrays, for the test that compares
        it with a host model: {"scalars": {...}, "bk": the nodes (records of nxsgpu_bknode_t), "bk_bytes",
        "bk_parent", "bk_slot", "fz_node", "fz_sig", "fz_len", "fz_len_start", "sg_node", "sg_sig", "sg_len",
        "px_node", "px_key"}.  Nothing is built by the call: a part that is not materialised is an empty array, and
        the scalars say which generation suggest's candidates and the completion order were built for.  Not while
        batches are in flight."""
        import numpy as np
        L = lib()
        L.nxs_test_term_image.restype = C.c_int
        L.nxs_test_term_image.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t)]

        def part(no, dtype):
            need = C.c_size_t()
            if L.nxs_test_term_image(self._h, no, None, 0, C.byref(need)) != 0:
                self.nxs._raise()
            buf = np.empty(need.value, dtype=np.uint8)
            if need.value:
                got = C.c_size_t()
                if L.nxs_test_term_image(self._h, no, buf.ctypes.data, buf.nbytes, C.byref(got)) != 0:
                    self.nxs._raise()
                assert got.value == need.value, (no, got.value, need.value)
            return buf.view(dtype)

        raw = part(TIMG_SCALARS, np.uint64)
        out = {"scalars": {name: int(raw[i]) for i, name in enumerate(TIMG_SCALAR_NAMES)}}
        for name, (no, dtype) in TIMG_PARTS.items():
            out[name] = part(no, np.dtype(TIMG_BK_DTYPE if dtype == "bk" else dtype))
        return out

    def reconfigure(self):
        """Re-read the NXS_GPU_* switches (parsed once at open); tests/tools."""
        lib().nxsgpu_index_reconfigure(self.device)

    def plan_batch(self, queries, limit=None, algo=None, fuzzymatch=None, prefixmatch=None, prefix_limit=None,
                   wildcardmatch=None, wildcard_terms=None):
        """nxs_index_plan_batch(): -> (ctypes array of GpuQuery, [err codes])."""
        L = lib()
        n = len(queries)
        qs = (C.c_char_p * n)(*[_b(q) for q in queries])
        plans = (GpuQuery * max(n, 1))()
        errs = (C.c_int * max(n, 1))()
        p = _make_params(limit, algo, fuzzymatch, False, prefixmatch, prefix_limit, False, wildcardmatch, wildcard_terms)
        try:
            r = L.nxs_index_plan_batch(self._h, p, qs, n, plans, errs)
        finally:
            if p:
                L.nxs_params_release(p)
        if r < 0:
            self.nxs._raise()
        return plans, list(errs[:n])

    def search_dev(self, plans, n, limit, algo, d_ids, d_scores, d_counts):
        """nxsgpu_search_dev(): results stay on the device at the given raw
        device pointers ([n][limit] u64 / f32, [n] u32).  Returns 0, or 1 if
        some query needs the exact two-pass path."""
        r = lib().nxsgpu_search_dev(self.device, algo, limit, plans, n,
                                    d_ids, d_scores, d_counts)
        if r < 0:
            raise NxsError(1, lib().nxsgpu_last_error().decode())
        return r

    def search_dev_begin(self, plans, n, limit, algo, d_ids, d_scores, d_counts):
        """nxsgpu_search_dev_begin(): queue a batch (at most NXS_BATCHES_INFLIGHT = 4 in flight)."""
        if lib().nxsgpu_search_dev_begin(self.device, algo, limit, plans, n,
                                         d_ids, d_scores, d_counts) != 0:
            raise NxsError(1, lib().nxsgpu_last_error().decode())

    def search_dev_end(self):
        """nxsgpu_search_dev_end(): wait for the oldest batch in flight -> 0 / 1."""
        r = lib().nxsgpu_search_dev_end(self.device)
        if r < 0:
            raise NxsError(1, lib().nxsgpu_last_error().decode())
        return r

    def fuzzy(self, tokens, want_visited=False):
        """Device BK-tree search for raw tokens -> term ids (0 = none)."""
        L = lib()
        toks = [_b(t) for t in tokens]
        blob = b"".join(toks)
        offs = [0]
        for t in toks:
            offs.append(offs[-1] + len(t))
        n = len(toks)
        ids = (C.c_uint32 * max(n, 1))()
        vis = (C.c_uint64 * max(n, 1))() if want_visited else None
        L.nxs_index_bk_sync.argtypes = [C.c_void_p]
        L.nxs_index_bk_sync(self._h)        # terms appended since the last image (N1)
        r = L.nxsgpu_fuzzy(self.device, blob, (C.c_uint32 * (n + 1))(*offs), n, ids, vis)
        if r != 0:
            raise NxsError(1, L.nxsgpu_last_error().decode())
        if want_visited:
            return list(ids[:n]), list(vis[:n])
        return list(ids[:n])

    def _lookup_batch(self, call, strings, p, noun, json):
        """One nxs_index_suggest_batch / _complete_batch call: `strings` in, params `p` (released here, may be
        None) -> a list of Suggestions, one per string (an NxsError instance in the slot of one that failed)."""
        n = len(strings)
        out = (C.c_void_p * max(n, 1))()
        errs = (C.c_int * max(n, 1))()
        try:
            ss = (C.c_char_p * max(n, 1))(*[_b(t) for t in strings])
            r = call(self._h, p, ss, n, out, errs)
        finally:
            if p:
                lib().nxs_params_release(p)
        if r < 0:
            self.nxs._raise()
        return [_drain_sugg(out[i], json) if out[i] else NxsError(errs[i], "%s %d failed" % (noun, i))
                for i in range(n)]

    def suggest(self, tokens, limit=None, maxdist=None, json=False):
        """nxs_index_suggest_batch(): for every raw token (not a query; it goes through the index's filters)
        the dictionary terms within `maxdist` (1 or 2, default 2) that some live doc holds, best `limit`
        (1..32, default 5) by distance, then df descending, then term id -> a list of Suggestions, one per
        token (an NxsError instance in the slot of a token that failed); json: their JSON texts."""
        return self._lookup_batch(lib().nxs_index_suggest_batch, tokens, _suggest_params(limit, maxdist), "token", json)

    def suggest_profile(self, reset=False):
        """nxsgpu_suggest_profile(): HIP-event times of the suggest pass per kernel (profiling on), its queue
        counts, tokens ranked on the host and passes repeated after a queue overflow."""
        out = (C.c_double * 10)()
        lib().nxsgpu_suggest_profile(self.device, out, 1 if reset else 0)
        return {"passes": int(out[0]), "ms": out[1], "screen_ms": out[2], "dist_ms": out[3], "group_ms": out[4],
                "select_ms": out[5], "survivors": int(out[6]), "matches": int(out[7]), "host_tokens": int(out[8]),
                "overflow_reruns": int(out[9])}

    def complete(self, prefixes, limit=None, json=False):
        """nxs_index_complete_batch(): for every prefix (normalised, never stemmed or dropped as a stop word)
        the dictionary terms that begin with it and that some live doc holds, best `limit` (1..32, default 5)
        by df descending, then term id -> a list of Suggestions, one per prefix, entries (term, distance =
        len(term) - len(prefix), df), `.matches` exact (an NxsError instance in the slot of a prefix that
        failed: an empty one); json: their JSON texts."""
        p = None
        if limit is not None:
            p = lib().nxs_params_create()
            lib().nxs_params_set_uint(p, b"complete_limit", limit)
        return self._lookup_batch(lib().nxs_index_complete_batch, prefixes, p, "prefix", json)

    def complete_profile(self, reset=False):
        """nxsgpu_complete_profile(): HIP-event times of the completion pass per kernel (profiling on), the
        last build of the term order, its entries, prefixes answered on the host and order builds."""
        out = (C.c_double * 8)()
        lib().nxsgpu_complete_profile(self.device, out, 1 if reset else 0)
        return {"passes": int(out[0]), "ms": out[1], "range_ms": out[2], "select_ms": out[3], "build_ms": out[4],
                "entries": int(out[5]), "host_prefixes": int(out[6]), "builds": int(out[7])}

    def wildcard(self, patterns, limit=None, json=False):
        """nxs_index_wildcard_batch(): for every pattern (`*` any run of bytes, `?` one byte; its literal pieces
        normalised, never stemmed or dropped as stop words) the dictionary terms that match it and that some
        live doc holds, best `limit` (1..32, default 5) by df descending, then term id -> a list of
        Suggestions, one per pattern, entries (term, distance = len(term) - the pattern's literal bytes, df),
        `.matches` exact (an NxsError instance in the slot of a pattern that failed: one without a literal
        byte, or longer than 255 bytes); json: their JSON texts."""
        p = None
        if limit is not None:
            p = lib().nxs_params_create()
            lib().nxs_params_set_uint(p, b"wildcard_limit", limit)
        return self._lookup_batch(lib().nxs_index_wildcard_batch, patterns, p, "pattern", json)

    def wildcard_profile(self, reset=False):
        """nxsgpu_wildcard_profile(): device passes and their HIP-event times per kernel (profiling on),
        patterns answered on the host / on the device; the entries of the term order and its builds since the
        index was opened (never reset)."""
        out = (C.c_double * 10)()
        lib().nxsgpu_wildcard_profile(self.device, out, 1 if reset else 0)
        return {"passes": int(out[0]), "ms": out[1], "range_ms": out[2], "match_ms": out[3], "merge_ms": out[4],
                "entries": int(out[5]), "host_patterns": int(out[6]), "builds": int(out[7]),
                "device_patterns": int(out[8])}

    def doc_terms(self, docs, limit=None, mindf=None, algo=None, json=False):
        """nxs_index_doc_terms_batch(): for every doc id the dictionary terms the doc holds whose live df is at
        least `mindf` (default 1) and whose rank under `algo` is not negative, best `limit` (1..32, default 5)
        by score descending, then term id -> a list of DocTerms, one per doc, entries (term, tf, df, score),
        `.matches` exact (an NxsError instance in the slot of a doc that is not live); json: their JSON
        texts."""
        L = lib()
        n = len(docs)
        p = None
        if limit is not None or mindf is not None or algo is not None:
            p = L.nxs_params_create()
            if limit is not None:
                L.nxs_params_set_uint(p, b"docterms_limit", limit)
            if mindf is not None:
                L.nxs_params_set_uint(p, b"docterms_mindf", mindf)
            if algo is not None:
                L.nxs_params_set_str(p, b"algo", _b(algo))
        out = (C.c_void_p * max(n, 1))()
        errs = (C.c_int * max(n, 1))()
        ds = (C.c_uint64 * max(n, 1))(*docs)
        try:
            r = L.nxs_index_doc_terms_batch(self._h, p, ds, n, out, errs)
        finally:
            if p:
                L.nxs_params_release(p)
        if r < 0:
            self.nxs._raise()
        return [_drain_docterms(out[i], json) if out[i] else NxsError(errs[i], "doc %d failed" % i) for i in range(n)]

    def similar(self, docs, limit=None, algo=None, terms=None, mindf=None, include_self=None, total=False,
                explain=False):
        """nxs_index_similar_batch(): for every doc id the docs most like it -- the results of the OR of its
        `terms` (1..32, default 8) best terms of df >= `mindf` (default 2), without the doc itself unless
        `include_self` -> result lists as search_batch returns them (an NxsError instance in the slot of a doc
        that is not live)."""
        L = lib()
        n = len(docs)
        p = _make_params(limit, algo, None, total, explain=explain)
        if terms is not None or mindf is not None or include_self is not None:
            p = p or L.nxs_params_create()
            if terms is not None:
                L.nxs_params_set_uint(p, b"similar_terms", terms)
            if mindf is not None:
                L.nxs_params_set_uint(p, b"similar_mindf", mindf)
            if include_self is not None:
                L.nxs_params_set_bool(p, b"similar_self", bool(include_self))
        resps = (C.c_void_p * max(n, 1))()
        errs = (C.c_int * max(n, 1))()
        ds = (C.c_uint64 * max(n, 1))(*docs)
        try:
            r = L.nxs_index_similar_batch(self._h, p, ds, n, resps, errs)
        finally:
            if p:
                L.nxs_params_release(p)
        if r < 0:
            self.nxs._raise()
        out = []
        for i in range(n):
            if resps[i]:
                out.append(_drain(resps[i], explain))
                L.nxs_resp_release(resps[i])
            else:
                out.append(NxsError(errs[i], "doc %d failed" % i))
        return out

    def doc_terms_profile(self, reset=False):
        """nxsgpu_doc_terms_profile(): calls that reached the device, HIP-event ms per kernel (profiling on),
        passes, distinct docs answered on the device / docs answered on the host, eligible pairs counted."""
        out = (C.c_double * 8)()
        lib().nxsgpu_doc_terms_profile(self.device, out, 1 if reset else 0)
        return {"calls": int(out[0]), "ord_ms": out[1], "scan_ms": out[2], "merge_ms": out[3], "passes": int(out[4]),
                "device_docs": int(out[5]), "host_docs": int(out[6]), "eligible": int(out[7])}

    def related(self, queries, limit=None, order=None, mindf=None, mincount=None, include_self=None, fuzzymatch=None,
                prefixmatch=None, wildcardmatch=None, algo=None, json=False):
        """nxs_index_related_batch(): for every query string the dictionary terms that occur in the docs the
        query matches, with count = the matching docs that hold the term and the live df, best `limit` (1..32,
        default 5) by `order` -- "count" (the default): count descending, or "share": count / df descending --
        then term id; terms with count < `mincount` or df < `mindf` (default 1 each) and, unless `include_self`,
        the query's own resolved terms are left out -> a list of Related, one per query, entries (term, count,
        df, score = count / df), `.matches` exact, `.docs` the number of matching docs (an NxsError instance
        in the slot of a query that failed: a parse error, more than 32 terms); json: their JSON texts."""
        L = lib()
        n = len(queries)
        p = _make_params(None, algo, fuzzymatch, False, prefixmatch, None, False, wildcardmatch, None)
        if any(v is not None for v in (limit, order, mindf, mincount, include_self)):
            p = p or L.nxs_params_create()
            for key, v in ((b"related_limit", limit), (b"related_mindf", mindf), (b"related_mincount", mincount)):
                if v is not None:
                    L.nxs_params_set_uint(p, key, v)
            if order is not None:
                L.nxs_params_set_str(p, b"related_order", _b(order))
            if include_self is not None:
                L.nxs_params_set_bool(p, b"related_self", bool(include_self))
        out = (C.c_void_p * max(n, 1))()
        errs = (C.c_int * max(n, 1))()
        qs = (C.c_char_p * max(n, 1))(*[_b(q) for q in queries])
        try:
            r = L.nxs_index_related_batch(self._h, p, qs, n, out, errs)
        finally:
            if p:
                L.nxs_params_release(p)
        if r < 0:
            self.nxs._raise()
        return [_drain_related(out[i], json) if out[i] else NxsError(errs[i], "query %d failed" % i) for i in range(n)]

    def related_profile(self, reset=False):
        """nxsgpu_related_profile(): distinct plans answered on the device / on the host, passes, HIP-event ms per
        kernel (profiling on), calls that had a plan to answer."""
        out = (C.c_double * 8)()
        lib().nxsgpu_related_profile(self.device, out, 1 if reset else 0)
        return {"device_queries": int(out[0]), "host_queries": int(out[1]), "passes": int(out[2]), "mask_ms": out[3],
                "scan_ms": out[4], "select_ms": out[5], "merge_ms": out[6], "calls": int(out[7])}

    def search_docs(self, queries, docs, limit=None, algo=None, fuzzymatch=None, total=False, prefixmatch=None,
                    prefix_limit=None, explain=False, wildcardmatch=None, wildcard_terms=None, json=False):
        """nxs_index_search_docs_batch(): every query ranked within a set of doc ids -> result lists as search_batch
        returns them (an NxsError instance in the slot of a query that failed: a parse error, more than 32 terms, a
        set of more than 2^22 ids).  `docs`: one sequence of ids (a list, or a numpy uint64 array) shared by all
        queries, or a sequence with one such sequence (or None: the empty set) per query -- entries that are the
        same object share one set, which is then sorted and resolved once.  Duplicates count once, ids that are not
        live docs are ignored.  json: the responses' JSON texts."""
        L = lib()
        n = len(queries)
        per_query = len(docs) > 0 and (docs[0] is None or hasattr(docs[0], "__len__"))
        if per_query and len(docs) != n:
            raise ValueError("search_docs: one doc set per query, or one set for all")
        u64p = C.POINTER(C.c_uint64)
        made = {}

        def c_set(d):
            if d is None or len(d) == 0:
                return (None, u64p(), 0)
            if id(d) not in made:
                if hasattr(d, "ctypes"):
                    import numpy as np
                    a = np.ascontiguousarray(d, dtype=np.uint64)
                    made[id(d)] = (a, a.ctypes.data_as(u64p), len(a))
                else:
                    a = (C.c_uint64 * len(d))(*d)
                    made[id(d)] = (a, C.cast(a, u64p), len(d))
            return made[id(d)]
        sets = [c_set(docs[i] if per_query else docs) for i in range(n)]
        ptrs = (u64p * max(n, 1))(*[x[1] for x in sets])
        lens = (C.c_size_t * max(n, 1))(*[x[2] for x in sets])
        qs = (C.c_char_p * max(n, 1))(*[_b(q) for q in queries])
        resps = (C.c_void_p * max(n, 1))()
        errs = (C.c_int * max(n, 1))()
        p = _make_params(limit, algo, fuzzymatch, total, prefixmatch, prefix_limit, explain, wildcardmatch, wildcard_terms)
        try:
            r = L.nxs_index_search_docs_batch(self._h, p, qs, n, ptrs, lens, resps, errs)
        finally:
            if p:
                L.nxs_params_release(p)
        if r < 0:
            self.nxs._raise()
        out = []
        for i in range(n):
            if resps[i]:
                out.append(_take(L.nxs_resp_tojson(resps[i], None)) if json else _drain(resps[i], explain))
                L.nxs_resp_release(resps[i])
            else:
                out.append(NxsError(errs[i], "query %d failed" % i))
        return out

    def match_docs(self, queries, limit=None, start=None, algo=None, fuzzymatch=None, prefixmatch=None,
                   wildcardmatch=None, json=False):
        """nxs_index_match_docs_batch(): for every query string the docs its expression matches -- the set "total"
        counts -- with id >= `start` (one id for all queries, or one per query; default 0) in ascending doc id, the
        first `limit` (1..2^22, default 1000) of them -> a list of Docs, one per query: a list of ints with
        `.total` = the size of the whole set and `.next` = the cursor of the next page, None when the set is
        exhausted (an NxsError instance in the slot of a query that failed: a parse error, more than 32 terms);
        json: their JSON texts."""
        L = lib()
        n = len(queries)
        p = _make_params(None, algo, fuzzymatch, False, prefixmatch, None, False, wildcardmatch, None)
        frm = None
        if start is not None and hasattr(start, "__len__"):
            if len(start) != n:
                raise ValueError("match_docs: one start for all queries, or one per query")
            frm = (C.c_uint64 * max(n, 1))(*start)
        if limit is not None or (start is not None and frm is None):
            p = p or L.nxs_params_create()
            if limit is not None:
                L.nxs_params_set_uint(p, b"match_limit", limit)
            if start is not None and frm is None:
                L.nxs_params_set_uint(p, b"match_from", start)
        out = (C.c_void_p * max(n, 1))()
        errs = (C.c_int * max(n, 1))()
        qs = (C.c_char_p * max(n, 1))(*[_b(q) for q in queries])
        try:
            r = L.nxs_index_match_docs_batch(self._h, p, qs, n, frm, out, errs)
        finally:
            if p:
                L.nxs_params_release(p)
        if r < 0:
            self.nxs._raise()
        return [_drain_docs(out[i], json) if out[i] else NxsError(errs[i], "query %d failed" % i) for i in range(n)]

    def match_docs_profile(self, reset=False):
        """nxsgpu_match_docs_profile(): distinct (plan, cursor) pairs answered on the device / on the host, passes,
        ids emitted, HIP-event ms per kernel (profiling on), calls that had a pair to answer."""
        out = (C.c_double * 10)()
        lib().nxsgpu_match_docs_profile(self.device, out, 1 if reset else 0)
        return {"device_pairs": int(out[0]), "host_pairs": int(out[1]), "passes": int(out[2]), "ids": int(out[3]),
                "mask_ms": out[4], "from_ms": out[5], "count_ms": out[6], "scan_ms": out[7], "emit_ms": out[8],
                "calls": int(out[9])}

    def search_docs_profile(self, reset=False):
        """nxsgpu_search_docs_profile(): calls that reached the device, passes, distinct sets and ids resolved,
        (query, doc) cells scored on the device / on the host, candidates, HIP-event ms per kernel (profiling on)."""
        out = (C.c_double * 12)()
        lib().nxsgpu_search_docs_profile(self.device, out, 1 if reset else 0)
        return {"calls": int(out[0]), "passes": int(out[1]), "sets": int(out[2]), "ids": int(out[3]),
                "device_cells": int(out[4]), "host_cells": int(out[5]), "candidates": int(out[6]), "ord_ms": out[7],
                "score_ms": out[8], "replay_ms": out[9]}

    def explain_profile(self, reset=False):
        """nxsgpu_explain_profile(): explain passes, HIP-event ms of k_explain (profiling on), (result, token)
        cells, cells present, chunks (kernel launches)."""
        out = (C.c_double * 8)()
        lib().nxsgpu_explain_profile(self.device, out, 1 if reset else 0)
        return {"passes": int(out[0]), "ms": out[1], "cells": int(out[2]), "present": int(out[3]),
                "chunks": int(out[4])}

    def set_plan_cache(self, on=True):
        """bench: the index's plan cache (query string -> compiled plan) on / off."""
        L = lib()
        L.nxs_index_set_plan_cache.argtypes = [C.c_void_p, C.c_int]
        L.nxs_index_set_plan_cache(self._h, 1 if on else 0)

    def set_profiling(self, on=True):
        lib().nxsgpu_set_profiling(self.device, 1 if on else 0)

    def count_profile(self, reset=False):
        """nxsgpu_count_profile(): HIP-event time of the count kernels alone (profiling on)."""
        out = (C.c_double * 6)()
        lib().nxsgpu_count_profile(self.device, out, 1 if reset else 0)
        return {"tile": {"launches": int(out[0]), "ms": out[1], "queries": int(out[4])},
                "req": {"launches": int(out[2]), "ms": out[3], "queries": int(out[5])}}

    def profile(self, reset=False):
        p = GpuProfile()
        lib().nxsgpu_get_profile(self.device, C.byref(p), 1 if reset else 0)
        d = {k: getattr(p, k) for k, _ in GpuProfile._fields_}
        d["fuzzy_level"] = list(d["fuzzy_level"])
        n = d.pop("n_cls")
        cls = [{"key": p.cls_key[i], "launches": p.cls_launches[i], "ms": p.cls_ms[i],
                "postings": p.cls_postings[i], "queries": p.cls_queries[i]} for i in range(n)]
        for k in ("cls_key", "cls_launches", "cls_ms", "cls_postings", "cls_queries"):
            d.pop(k)
        d["classes"] = cls
        return d

    def close(self):
        if self._h:
            lib().nxs_index_close(self._h)
            self._h = None


# ---- host-only helpers (run without a GPU; used by the CPU test tier) ------

def query_repr(q):
    err = C.c_void_p()
    r = lib().nxs_test_query_repr(_b(q), C.byref(err))
    return _take(r), _take(err.value)


def query_lex(q):
    kinds = (C.c_int * 512)()
    n = lib().nxs_query_lex(_b(q), kinds, 512)
    return list(kinds[:n])


def compile_query(q, words, lowercase=False):
    """-> (code, errmsg, empty, GpuQuery) against a word list (ids 1..n)."""
    arr = (C.c_char_p * max(len(words), 1))(*[_b(w) for w in words])
    plan = GpuQuery()
    empty = C.c_int()
    err = C.create_string_buffer(256)
    code = lib().nxs_test_compile(_b(q), arr, len(words), lowercase,
                                  C.byref(plan), C.byref(empty), err, 256)
    return code, err.value.decode(), bool(empty.value), plan


def filter_token(s, basedir=None, stopwords=False, stemmer=False):
    """The query-token filter pipeline on one string -> (action, result):
    action 1 keep, 0 discarded (stop word), -1 error."""
    L = lib()
    L.nxs_test_filter.restype = C.c_void_p
    L.nxs_test_filter.argtypes = [C.c_char_p, C.c_int, C.c_char_p, C.POINTER(C.c_int)]
    act = C.c_int()
    r = L.nxs_test_filter(os.fsencode(basedir) if basedir else None, (1 if stopwords else 0) | (2 if stemmer else 0),
                          _b(s), C.byref(act))
    return act.value, _take(r)


def compile_wide(q, words):
    """-> (code, wide, term_ids, prog) for a query over words "w1".."wN"."""
    arr = (C.c_char_p * max(len(words), 1))(*[_b(w) for w in words])
    wide, nt, pl = C.c_int(), C.c_uint32(), C.c_uint32()
    tids = (C.c_uint32 * 4096)()
    prog = (C.c_uint16 * 8192)()
    code = lib().nxs_test_compile_wide(_b(q), arr, len(words), C.byref(wide), C.byref(nt),
                                       tids, 4096, C.byref(pl), prog, 8192)
    return code, bool(wide.value), list(tids[:nt.value]), list(prog[:pl.value])


def bk_image(words):
    """Flattened BK-tree of a word list -> list of node dicts in BFS order."""
    arr = (C.c_char_p * max(len(words), 1))(*[_b(w) for w in words])
    img = BkImage()
    if lib().nxs_test_bk_image(arr, len(words), C.byref(img)) != 0:
        raise MemoryError
    nodes = []
    for i in range(img.n):
        nd = img.nodes[i]
        s = bytes(img.bytes[nd.str_off:nd.str_off + nd.str_len])
        nodes.append(dict(bitmap=nd.bitmap, first_child=nd.first_child,
                          term_id=nd.term_id, term=s, flags=nd.flags,
                          inl=bytes(nd.inl)))
    depth = img.depth
    lib().nxs_bk_free(C.byref(img))
    return nodes, depth


def levdist(a, b):
    a, b = _b(a), _b(b)
    return lib().nxs_test_levdist(a, len(a), b, len(b))
