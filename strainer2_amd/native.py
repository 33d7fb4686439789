"""ctypes binding of include/strainer_kmer.h (see that header for the contract of each call).

Fails loudly when the native library is absent: there is no fallback implementation.
"""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))


def library_path():
    # SK_LIBRARY: another build of the same library (A/B timing of kernel variants)
    return os.environ.get("SK_LIBRARY") or os.path.join(_HERE, "lib", "libstrainer_kmer.so")


def cli_path(name="kmer_scrub_count"):
    return os.path.join(_HERE, "bin", name)


def _load():
    p = library_path()
    if not os.path.exists(p):
        raise ImportError(
            f"{p} not found: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "or `make -C strainer2_amd/csrc` (there is no non-native fallback)")
    return C.CDLL(p, mode=C.RTLD_GLOBAL)


lib = _load()

SK_K = 31
SK_UNION_MAX = 32
SK_REF_TABLE_SLOTS = 8000000
SK_KEY_NONE = 0xFFFFFFFFFFFFFFFF
SK_OK = 0
SK_E_NODEVICE = -1
SK_E_OPEN = -5
SK_E_STATE = -7
SK_E_SPLIT = -9
SK_E_PLAN = -10
SK_E_CACHE = -11

# every symbol include/strainer_kmer.h declares (tests check that the library exports all of them)
ABI_SYMBOLS = [
    "sk_text_parse_device", "sk_scan_text_pinned", "sk_scan_text_pinned_many", "sk_text_stats", "sk_text_release", "sk_text_option",
    "sk_text_enabled", "sk_text_timing",
    "sk_ctx_create", "sk_ctx_destroy", "sk_last_error", "sk_strerror", "sk_table_load", "sk_table_load_ex",
    "sk_table_load_wide", "sk_table_load_text", "sk_table_build_from_text", "sk_table_export_keys", "sk_table_export_keys_of", "sk_scan_stream", "sk_scan_device", "sk_pinned_alloc", "sk_pinned_free", "sk_scan_pinned", "sk_scan_pinned_packed", "sk_scan_pinned_many", "sk_scan_pinned_packed_many", "sk_device_memory", "sk_scan_device_packed", "sk_pack_stream", "sk_packed_bytes",
    "sk_ticket_wait", "sk_tally_batch", "sk_sync", "sk_counts_fetch",
    "sk_counts_set", "sk_counts_set_rows", "sk_counts_zero", "sk_counts_device_ptr", "sk_table_rows", "sk_table_cols",
    "sk_counts_allreduce", "sk_comm_init", "sk_comm_init_ex", "sk_rendezvous_exchange", "sk_comm_destroy", "sk_comm_sum_u32", "sk_comm_agree_u64", "sk_comm_max_u64", "sk_comm_world", "sk_scan_timing", "sk_set_option", "sk_dev_alloc", "sk_dev_free",
    "sk_dev_upload", "sk_dev_download",
    "skh_keyset_from_file", "skh_keyset_from_stream", "skh_keyset_free", "skh_keyset_key",
    "skh_keyset_load", "skh_scan_file", "skh_scan_list", "skh_scan_list_many", "skh_scan_list_uncut", "skh_list_plan_hash", "skh_list_plan_owners", "skh_print_counts",
    "skh_kmer_scrub_count_main", "skh_strain_detect_main", "skh_strain_detect_resident", "skh_strain_detect_resident_many", "skh_decode_file",
    "sk_filter_create", "sk_filter_destroy", "sk_filter_load", "sk_filter_load_counts", "sk_filter_sums",
    "sk_filter_hist", "sk_filter_joint", "sk_filter_above", "skh_scrub_filter_main", "skh_scrub_filter_resident",
    "sk_distinct_count", "sk_first_seen_count", "skh_coverage_depth_main",
    "sk_batch_create", "sk_batch_destroy", "sk_batch_sync", "sk_batch_fill", "sk_batch_fill_packed", "sk_batch_fill_text", "sk_batch_text_finish", "sk_tally_launch", "sk_tally_collect", "sk_tally_collect_sparse",
    "sk_union_create", "sk_union_destroy", "sk_union_tally_launch", "sk_union_tally_collect", "sk_union_last_error", "sk_union_scan_timing", "sk_union_sync",
    "sk_union_members", "sk_union_rows", "sk_union_count_enable", "sk_union_context", "sk_union_counts_fold",
    "skh_kmer_scrub_count_multi_main",
    "sk_pack_device", "sk_scan_pinned_pack_many", "sk_pack_ticket_wait", "sk_pack_release", "skh_pack_cache_set", "skh_pack_cache_stats",
    "sk_batch_pack_home", "sk_batch_pack_wait", "skh_target_cache_stats",
    "sk_covacc_create", "sk_covacc_destroy", "sk_covacc_hold", "sk_covacc_add", "sk_covacc_add_rows", "sk_covacc_finish_target", "sk_covacc_rows",
    "sk_covacc_pick", "sk_covacc_fetch_hold", "skh_coverage_only_stats",
    "sk_tally_collect_counts", "sk_tally_fetch_held", "sk_union_tally_launch_ex", "sk_union_tally_collect_counts", "sk_union_tally_fetch_held",
    "skh_regions_from_file", "skh_regions_free", "sk_table_first_pos", "sk_covacc_set_regions", "sk_covacc_region_rows",
    "sk_covacc_finish_target_regions",
    "sk_covacc_set_spectrum", "sk_covacc_finish_target_spectrum", "sk_distinct_spectrum",
    "sk_union_share",
    "sk_recur_create", "sk_recur_destroy", "sk_recur_mark_bits", "sk_recur_finish", "sk_covacc_set_recurrence", "sk_covacc_mark_target",
    "sk_distinct_recurrence",
    "sk_covacc_set_thresholds", "sk_covacc_add_rows_hits", "sk_covacc_finish_target_thresholds", "sk_distinct_thresholds",
    "sk_filter_classes_joint", "sk_filter_classes_above", "skh_scrub_filter_resident_sweep",
    "sk_covacc_set_classes", "sk_covacc_finish_target_classes", "sk_distinct_classes",
    "sk_covacc_set_support", "sk_covacc_finish_target_support",
    "sk_scan_batch", "sk_background_finish", "sk_union_background_finish",
    "sk_covacc_set_rarefaction", "sk_covacc_set_pair_base", "sk_covacc_add_pairs", "sk_covacc_add_rows_hits_pairs",
    "sk_covacc_finish_target_rarefaction", "skh_rarefaction_parse", "skh_rarefaction_draw", "skh_rarefaction_class",
    "skh_rarefaction_fold", "skh_rarefaction_write",
    "sk_item_slots", "sk_item_slot", "sk_item_fold", "skh_scan_list_prevalence", "skh_prev_items_free", "skh_scrub_filter_resident_cols",
    "sk_union_item_fold", "skh_scan_list_many_prevalence",
]


class _KeysetStruct(C.Structure):
    _fields_ = [("nrows", C.c_uint32), ("nwide", C.c_uint32),
                ("packed", C.POINTER(C.c_uint64)), ("first_count", C.POINTER(C.c_uint32)),
                ("locality", C.POINTER(C.c_uint32)),
                ("wide_keys", C.POINTER(C.c_char)), ("wide_rows", C.POINTER(C.c_uint32)),
                ("final_slots", C.c_uint32), ("short_records", C.c_uint64),
                ("text2", C.POINTER(C.c_uint32)), ("text_bases", C.c_uint32), ("first_pos", C.POINTER(C.c_uint32))]


_SINK = C.CFUNCTYPE(C.c_int, C.c_void_p, C.POINTER(C.c_uint8), C.c_uint64)

lib.sk_ctx_create.argtypes = [C.POINTER(C.c_void_p), C.c_int]
lib.sk_ctx_destroy.argtypes = [C.c_void_p]
lib.sk_ctx_destroy.restype = None
lib.sk_last_error.argtypes = [C.c_void_p]
lib.sk_last_error.restype = C.c_char_p
lib.sk_strerror.argtypes = [C.c_int]
lib.sk_strerror.restype = C.c_char_p
lib.sk_table_load.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32]
lib.sk_table_load_ex.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p]
lib.sk_table_load_wide.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32]
lib.sk_table_load_text.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p]
lib.sk_scan_stream.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint32]
lib.sk_scan_device.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint32]
lib.sk_pinned_alloc.argtypes = [C.c_void_p, C.POINTER(C.c_void_p), C.c_uint64]
lib.sk_pinned_free.argtypes = [C.c_void_p, C.c_void_p]
lib.sk_scan_pinned.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint32, C.POINTER(C.c_uint64)]
lib.sk_ticket_wait.argtypes = [C.c_void_p, C.c_uint64]
lib.sk_scan_pinned_packed.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint32, C.POINTER(C.c_uint64)]
lib.sk_scan_pinned_many.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint64, C.c_uint32, C.POINTER(C.c_uint64)]
lib.sk_scan_pinned_packed_many.argtypes = lib.sk_scan_pinned_many.argtypes
lib.sk_device_memory.argtypes = [C.c_void_p, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
lib.sk_scan_device_packed.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint32]
lib.sk_pack_stream.argtypes = [C.c_void_p, C.c_uint64, C.c_void_p, C.POINTER(C.c_int)]
lib.sk_packed_bytes.argtypes = [C.c_uint64]
lib.sk_packed_bytes.restype = C.c_uint64
lib.sk_pack_device.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.POINTER(C.c_int)]
lib.sk_scan_pinned_pack_many.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint64, C.c_uint32, C.c_void_p, C.c_void_p, C.POINTER(C.c_uint64)]
lib.sk_pack_ticket_wait.argtypes = [C.c_void_p, C.c_uint64]
lib.sk_pack_release.argtypes = [C.c_void_p]
lib.sk_pack_release.restype = None
lib.skh_pack_cache_set.argtypes = [C.c_void_p, C.c_char_p, C.c_char_p]
lib.skh_pack_cache_stats.argtypes = [C.c_void_p] + [C.POINTER(C.c_uint64)] * 4 + [C.c_int]
lib.skh_target_cache_stats.argtypes = [C.POINTER(C.c_uint64)] * 4 + [C.c_int]
lib.sk_batch_pack_home.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
lib.sk_batch_pack_wait.argtypes = [C.c_void_p]
lib.sk_tally_batch.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32,
                               C.c_void_p, C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64)]
lib.sk_sync.argtypes = [C.c_void_p]


class TextInfo(C.Structure):
    """sk_text_info"""
    _fields_ = [("status", C.c_uint32), ("form", C.c_uint32), ("consumed", C.c_uint64), ("stream_bytes", C.c_uint64),
                ("nrecords", C.c_uint64), ("bases", C.c_uint64)]


SK_TEXT_OK, SK_TEXT_DECLINED = 0, 1
SK_TEXT_FASTA, SK_TEXT_FASTQ4 = 1, 2
SK_TEXT_TILE = 16384
lib.sk_text_parse_device.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_int, C.c_void_p, C.c_void_p, C.c_uint64, C.POINTER(TextInfo)]
lib.sk_scan_text_pinned.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_int, C.c_uint32, C.POINTER(TextInfo)]
lib.sk_text_stats.argtypes = [C.c_void_p, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.c_int]
lib.sk_text_release.argtypes = [C.c_void_p]
lib.sk_text_release.restype = None
lib.sk_text_option.argtypes = [C.c_void_p, C.c_int]
lib.sk_text_enabled.argtypes = [C.c_void_p]
lib.sk_text_timing.argtypes = [C.c_void_p, C.POINTER(C.c_double)]
lib.sk_item_slots.argtypes = [C.c_void_p, C.c_uint32]
lib.sk_item_slot.argtypes = [C.c_void_p, C.c_int]
lib.sk_item_fold.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p]
lib.sk_union_item_fold.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p]
lib.sk_counts_fetch.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p]
lib.sk_counts_set.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p]
lib.sk_counts_set_rows.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_uint32]
lib.sk_counts_zero.argtypes = [C.c_void_p, C.c_uint32]
lib.sk_counts_device_ptr.argtypes = [C.c_void_p]
lib.sk_counts_device_ptr.restype = C.c_void_p
lib.sk_table_rows.argtypes = [C.c_void_p]
lib.sk_table_rows.restype = C.c_uint32
lib.sk_table_cols.argtypes = [C.c_void_p]
lib.sk_table_cols.restype = C.c_uint32
lib.sk_counts_allreduce.argtypes = [C.c_void_p, C.c_void_p]
lib.sk_rendezvous_exchange.argtypes = [C.c_int, C.c_int, C.c_char_p, C.c_int, C.c_void_p, C.c_double]
lib.sk_scan_timing.argtypes = [C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_uint64), C.c_int]
lib.sk_set_option.argtypes = [C.c_void_p, C.c_char_p, C.c_long]
lib.sk_dev_alloc.argtypes = [C.c_void_p, C.POINTER(C.c_void_p), C.c_uint64]
lib.sk_dev_free.argtypes = [C.c_void_p, C.c_void_p]
lib.sk_dev_upload.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64]
lib.sk_dev_download.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64]
lib.skh_keyset_from_file.argtypes = [C.POINTER(_KeysetStruct), C.c_char_p, C.c_uint32, C.c_uint32, C.c_uint32]
lib.skh_keyset_from_stream.argtypes = [C.POINTER(_KeysetStruct), C.c_char_p, C.c_size_t, C.c_uint32, C.c_uint32, C.c_uint32]
lib.skh_keyset_free.argtypes = [C.POINTER(_KeysetStruct)]
lib.skh_keyset_free.restype = None
lib.skh_keyset_key.argtypes = [C.POINTER(_KeysetStruct), C.c_uint32, C.c_char_p]
lib.skh_keyset_key.restype = None
lib.skh_keyset_load.argtypes = [C.c_void_p, C.POINTER(_KeysetStruct), C.c_uint32]
lib.skh_scan_file.argtypes = [C.c_void_p, C.c_char_p, C.c_uint32, C.POINTER(C.c_uint64)]
lib.skh_list_plan_hash.argtypes = [C.c_char_p, C.c_char_p, C.c_uint32, C.POINTER(C.c_uint64)]
lib.skh_list_plan_hash.restype = C.c_int
lib.skh_list_plan_owners.argtypes = [C.c_char_p, C.c_char_p, C.c_uint32, C.c_void_p, C.c_uint32, C.POINTER(C.c_uint32)]
lib.skh_list_plan_owners.restype = C.c_int
lib.skh_scan_list.argtypes = [C.c_void_p, C.c_char_p, C.c_char_p, C.c_uint32, C.c_void_p, C.c_void_p,
                              C.c_uint32, C.c_uint32, C.POINTER(C.c_uint64)]
lib.skh_scan_list_uncut.argtypes = lib.skh_scan_list.argtypes
lib.skh_scan_list_many.argtypes = [C.c_void_p, C.c_uint32] + lib.skh_scan_list.argtypes[1:]
lib.skh_print_counts.argtypes = [C.c_void_p, C.POINTER(_KeysetStruct), C.c_void_p, C.c_int]
lib.skh_kmer_scrub_count_main.argtypes = [C.c_int, C.POINTER(C.c_char_p), C.c_void_p, C.c_void_p]
lib.skh_strain_detect_main.argtypes = [C.c_int, C.POINTER(C.c_char_p), C.c_void_p, C.c_void_p]
lib.skh_decode_file.argtypes = [C.c_char_p, C.c_uint64, _SINK, C.c_void_p, C.POINTER(C.c_uint64)]
lib.skh_decode_file.restype = C.c_int64

lib.sk_filter_create.argtypes = [C.c_void_p, C.POINTER(C.c_void_p)]
lib.sk_filter_destroy.argtypes = [C.c_void_p]
lib.sk_filter_destroy.restype = None
lib.sk_filter_load.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64]
lib.sk_filter_load_counts.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_int32]
lib.sk_filter_sums.argtypes = [C.c_void_p, C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.POINTER(C.c_uint64),
                               C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
lib.sk_filter_hist.argtypes = [C.c_void_p, C.c_int, C.c_int64, C.c_uint32, C.c_void_p]
lib.sk_filter_joint.argtypes = [C.c_void_p, C.c_int64, C.c_int64, C.c_uint64, C.c_void_p]
lib.sk_filter_above.argtypes = [C.c_void_p, C.c_int64, C.c_int64, C.c_void_p]
SK_SCRUB_SWEEP_MAX = 16
lib.sk_filter_classes_joint.argtypes = [C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p]
lib.sk_filter_classes_above.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p]
lib.skh_scrub_filter_resident_sweep.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_char_p, C.c_int, C.c_char_p, C.c_void_p, C.c_void_p]
lib.skh_scrub_filter_main.argtypes = [C.c_int, C.POINTER(C.c_char_p), C.c_void_p, C.c_void_p]
lib.skh_scrub_filter_resident.argtypes = [C.c_void_p, C.POINTER(_KeysetStruct), C.c_int, C.c_double, C.c_int, C.c_void_p, C.c_void_p]

lib.sk_distinct_count.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint32, C.c_void_p, C.c_void_p]
lib.sk_first_seen_count.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p]
lib.skh_coverage_depth_main.argtypes = [C.c_int, C.POINTER(C.c_char_p), C.c_void_p, C.c_void_p]

lib.sk_batch_create.argtypes = [C.c_void_p, C.POINTER(C.c_void_p)]
lib.sk_batch_destroy.argtypes = [C.c_void_p]
lib.sk_batch_destroy.restype = None
lib.sk_batch_fill.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint32]
lib.sk_batch_fill_packed.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint32]
lib.sk_batch_fill_text.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_int]
lib.sk_batch_text_finish.argtypes = [C.c_void_p, C.POINTER(TextInfo), C.POINTER(C.POINTER(C.c_uint32))]
lib.sk_tally_launch.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint64]
lib.sk_tally_collect.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_uint64)]
lib.sk_tally_collect_sparse.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64), C.c_void_p, C.POINTER(C.c_uint64)]
lib.sk_union_create.argtypes = [C.POINTER(C.c_void_p), C.c_uint32, C.c_uint32, C.c_uint32, C.POINTER(C.c_void_p)]
lib.sk_union_destroy.argtypes = [C.c_void_p]
lib.sk_union_destroy.restype = None
lib.sk_union_scan_timing.argtypes = [C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_uint64), C.c_int]
lib.sk_union_tally_launch.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64]
lib.sk_union_tally_collect.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64), C.c_void_p, C.POINTER(C.c_uint64)]
lib.sk_union_last_error.argtypes = [C.c_void_p]
lib.sk_union_last_error.restype = C.c_char_p


class CovaccMate(C.Structure):
    _fields_ = [("held", C.c_int), ("b0", C.c_uint32), ("bstep", C.c_uint32)]


lib.sk_tally_collect_counts.argtypes = [C.c_void_p, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
lib.sk_tally_fetch_held.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p]
lib.sk_union_tally_launch_ex.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_int]
lib.sk_union_tally_collect_counts.argtypes = [C.c_void_p, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
lib.sk_union_tally_fetch_held.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p]
lib.sk_covacc_create.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_int64, C.POINTER(C.c_void_p)]
lib.sk_covacc_destroy.argtypes = [C.c_void_p]
lib.sk_covacc_destroy.restype = None
lib.sk_covacc_hold.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
lib.sk_covacc_add.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.POINTER(CovaccMate)]
lib.sk_covacc_add_rows.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint64]
lib.sk_covacc_finish_target.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
lib.sk_covacc_rows.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p]
lib.sk_covacc_pick.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_uint32, C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64),
                               C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64)]
lib.sk_covacc_fetch_hold.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64), C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64)]
lib.skh_coverage_only_stats.argtypes = [C.POINTER(C.c_uint64)] * 3 + [C.c_int]
lib.skh_coverage_only_stats.restype = None
lib.sk_union_count_enable.argtypes = [C.c_void_p, C.c_uint32]
lib.sk_union_context.argtypes = [C.c_void_p]
lib.sk_union_context.restype = C.c_void_p
lib.sk_union_counts_fold.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_int]
lib.sk_union_members.argtypes = [C.c_void_p]
lib.sk_union_members.restype = C.c_uint32
lib.sk_union_rows.argtypes = [C.c_void_p]
lib.sk_union_rows.restype = C.c_uint32
lib.sk_union_share.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
SK_BACKGROUND_MAX_DEPTH = 255
SK_BACKGROUND_HEAD = 5
lib.sk_scan_batch.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32]
lib.sk_background_finish.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p]
lib.sk_union_background_finish.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p]

_libc = C.CDLL(None)
_libc.fopen.argtypes = [C.c_char_p, C.c_char_p]
_libc.fopen.restype = C.c_void_p
_libc.fclose.argtypes = [C.c_void_p]


class SKError(RuntimeError):
    def __init__(self, code, detail=""):
        self.code = code
        msg = lib.sk_strerror(code).decode()
        super().__init__(f"libstrainer_kmer error {code}: {msg}" + (f" ({detail})" if detail else ""))


class Keyset:
    """Strain key set in reference output order (host layer: skh_keyset_*)."""

    def __init__(self):
        self._s = _KeysetStruct()
        self._live = False

    @classmethod
    def from_file(cls, path, initial_slots=SK_REF_TABLE_SLOTS, default_val=1, incr=1):
        ks = cls()
        rc = lib.skh_keyset_from_file(C.byref(ks._s), os.fsencode(path), initial_slots, default_val, incr)
        if rc:
            raise SKError(rc, path)
        ks._live = True
        return ks

    @classmethod
    def from_stream(cls, stream: bytes, initial_slots=SK_REF_TABLE_SLOTS, default_val=1, incr=1):
        ks = cls()
        rc = lib.skh_keyset_from_stream(C.byref(ks._s), stream, len(stream), initial_slots, default_val, incr)
        if rc:
            raise SKError(rc)
        ks._live = True
        return ks

    nrows = property(lambda self: self._s.nrows)
    nwide = property(lambda self: self._s.nwide)
    final_slots = property(lambda self: self._s.final_slots)
    short_records = property(lambda self: self._s.short_records)

    def packed(self):
        return np.ctypeslib.as_array(self._s.packed, shape=(max(self.nrows, 1),))[: self.nrows].copy()

    def first_count(self):
        return np.ctypeslib.as_array(self._s.first_count, shape=(max(self.nrows, 1),))[: self.nrows].copy()

    def first_pos(self):
        """text position of each row's first all-ACGT occurrence along the strain, 0xFFFFFFFF for none"""
        return np.ctypeslib.as_array(self._s.first_pos, shape=(max(self.nrows, 1),))[: self.nrows].copy()

    def key(self, row):
        buf = C.create_string_buffer(32)
        lib.skh_keyset_key(C.byref(self._s), row, buf)
        return buf.value

    def keys(self):
        """All keys as bytes, in row order (vectorised decode of the packed ones)."""
        pk = self.packed()
        out = np.empty((self.nrows, SK_K), dtype=np.uint8)
        lut = np.frombuffer(b"ACGT", dtype=np.uint8)
        for i in range(SK_K):
            out[:, i] = lut[((pk >> np.uint64(2 * (SK_K - 1 - i))) & np.uint64(3)).astype(np.int64)]
        keys = [bytes(r) for r in out]
        for r in np.nonzero(pk == np.uint64(SK_KEY_NONE))[0]:
            keys[int(r)] = self.key(int(r))
        return keys

    def close(self):
        if self._live:
            lib.skh_keyset_free(C.byref(self._s))
            self._live = False

    def __del__(self):
        self.close()


class KmerContext:
    """One device context (device layer: sk_*)."""

    def __init__(self, device=0):
        self._h = C.c_void_p()
        rc = lib.sk_ctx_create(C.byref(self._h), device)
        if rc:
            self._h = None
            raise SKError(rc, "sk_ctx_create: this library needs an MI355X-class GPU; there is no CPU path")
        self._bufs = []

    def _ck(self, rc):
        if rc == SK_E_CACHE:            # (a host-layer code: the device layer's texts do not know it)
            raise SKError(rc, "a packed input cache file is damaged (stderr names it); part of it may have been counted")
        if rc:
            raise SKError(rc, lib.sk_last_error(self._h).decode())

    def set_option(self, name, value):
        if name == "device_parse":          # plain text parsed on the device (sk_text_option): the list scan's items, and the targets of
            # strain_detect run on this context (strain_detect_resident: the streams follow the context that owns the device's batches)
            self._ck(lib.sk_text_option(self._h, int(value)))
            return
        self._ck(lib.sk_set_option(self._h, name.encode(), value))

    def parse_text_device(self, dev_text, nbytes, is_eof, want_rec_start=False):
        """sk_text_parse_device on text resident at device pointer dev_text: returns (info, dev_stream, dev_rec_start) -- device
        buffers of this context (dev_free), nbytes + 1 bytes and, with want_rec_start, room for nbytes // 2 + 1 record starts
        (else None).  info.status == SK_TEXT_DECLINED: nothing in them may be used."""
        info = TextInfo()
        out = self.dev_alloc(nbytes + 16)
        cap = nbytes // 2 + 1 if want_rec_start else 0
        rs = self.dev_alloc(cap * 4) if want_rec_start else None
        self._ck(lib.sk_text_parse_device(self._h, dev_text, nbytes, int(bool(is_eof)), out, rs, cap, C.byref(info)))
        return info, out, rs

    def scan_text(self, data, col, is_eof=True):
        """sk_scan_text_pinned: plain FASTA/FASTQ text (bytes or a uint8 array) goes up as it is, is parsed on the device and counted
        into column `col`; returns the sk_text_info (status DECLINED: nothing was counted)."""
        data = np.frombuffer(data, dtype=np.uint8) if not isinstance(data, np.ndarray) else np.ascontiguousarray(data, dtype=np.uint8)
        info = TextInfo()
        buf = self.pinned_alloc(max(data.size, 16))
        try:
            buf[: data.size] = data
            self._ck(lib.sk_scan_text_pinned(self._h, buf.ctypes.data, data.size, int(bool(is_eof)), col, C.byref(info)))
        finally:
            self.pinned_free(buf)
        return info

    def text_timing(self):
        """device milliseconds of this context's last text parse (sk_text_timing)"""
        ms = C.c_double(0)
        self._ck(lib.sk_text_timing(self._h, C.byref(ms)))
        return ms.value

    def text_stats(self, reset=False):
        """(pieces parsed on the device, pieces it declined) since the last reset (sk_text_stats)"""
        a, b = C.c_uint64(0), C.c_uint64(0)
        self._ck(lib.sk_text_stats(self._h, C.byref(a), C.byref(b), int(reset)))
        return a.value, b.value

    def load_keyset(self, ks: Keyset, ncols=4):
        self._ck(lib.skh_keyset_load(self._h, C.byref(ks._s), ncols))

    def build_from_text(self, records, ncols=4, col0_value=1):
        """sk_table_build_from_text from records of A/C/G/T/N bytes (those of 30 bases or more make the text, end to end): the whole
        table is made on the device, rows in strain order; returns the row count"""
        text, ok = [], []
        for r in records:
            if len(r) + 1 < SK_K:
                continue
            a = np.frombuffer(bytes(r).upper(), dtype=np.uint8)
            good = np.isin(a, np.frombuffer(b"ACGT", dtype=np.uint8))
            run = np.zeros(len(a) + 1, dtype=np.int64)
            for i in range(len(a)):
                run[i + 1] = run[i] + 1 if good[i] else 0
            st = np.zeros(len(a), dtype=bool)
            st[: max(len(a) - SK_K + 1, 0)] = run[SK_K:] >= SK_K
            text.append(np.where(good, (a >> 1) & 3, 0).astype(np.uint32))      # (A 0, C 1, T 2, G 3 by bits 1..2 of the letter ...)
            ok.append(st)
        code = np.concatenate(text)
        lut = np.zeros(4, dtype=np.uint32)
        lut[[0, 1, 2, 3]] = [0, 1, 3, 2]                                           # (... to A 0, C 1, G 2, T 3)
        code = lut[code]
        ok = np.concatenate(ok)
        n = len(code)
        pad = np.zeros((-n) % 16, dtype=np.uint32)
        words = np.concatenate([code, pad]).reshape(-1, 16)
        text2 = np.zeros(len(words) + 4, dtype=np.uint32)
        for j in range(16):
            text2[: len(words)] |= words[:, j] << np.uint32(2 * (15 - j))
        okw = np.zeros((n + 31) // 32 + 2, dtype=np.uint32)
        idx = np.nonzero(ok)[0]
        np.bitwise_or.at(okw, idx >> 5, (np.uint32(1) << (idx & 31).astype(np.uint32)))
        nrows = C.c_uint32(0)
        self._ck(lib.sk_table_build_from_text(self._h, text2.ctypes.data, okw.ctypes.data, n, len(idx), ncols, col0_value, C.byref(nrows)))
        return int(nrows.value)

    def first_pos(self):
        """sk_table_first_pos: every row's first text position as the table on the device has it (0xFFFFFFFF: none)"""
        n = int(lib.sk_table_rows(self._h))
        out = np.zeros(max(n, 1), dtype=np.uint32)
        self._ck(lib.sk_table_first_pos(self._h, out.ctypes.data))
        return out[:n]

    def load_table(self, keys: np.ndarray, ncols=4):
        keys = np.ascontiguousarray(keys, dtype=np.uint64)
        self._ck(lib.sk_table_load(self._h, keys.ctypes.data, len(keys), ncols))

    def scan_stream(self, stream, col):
        if isinstance(stream, np.ndarray):
            stream = np.ascontiguousarray(stream, dtype=np.uint8)
            self._ck(lib.sk_scan_stream(self._h, stream.ctypes.data, stream.size, col))
        else:
            self._ck(lib.sk_scan_stream(self._h, stream, len(stream), col))

    def scan_batch(self, batch, col):
        """sk_scan_batch: a COUNT scan of a filled TallyBatch, as it lies on the device, into column col (returns at once; sync()
        before the batch is refilled)"""
        self._ck(lib.sk_scan_batch(self._h, batch._h, col))

    def background_finish(self, col, type_col=0, informative_value=2, max_depth=63):
        """sk_background_finish: uint64[2, 5 + max_depth + 1] -- row 0 the informative rows, row 1 the background rows; columns
        kmers, covered_kmers, total_hits, rows above max_depth, hits above max_depth, then the rows at depth 0..max_depth.  Column
        col is zero afterwards."""
        out = np.zeros((2, SK_BACKGROUND_HEAD + max_depth + 1), dtype=np.uint64)
        self._ck(lib.sk_background_finish(self._h, col, type_col, informative_value, max_depth, out.ctypes.data))
        return out

    def item_slots(self, nslots):
        """sk_item_slots: nslots item slots (a scratch column and a difference array each) for the loaded table; 0 frees them"""
        self._ck(lib.sk_item_slots(self._h, nslots))

    def item_slot(self, slot):
        """sk_item_slot: every COUNT scan from now on adds into item slot `slot`, whatever column it names; -1: into its column"""
        self._ck(lib.sk_item_slot(self._h, slot))

    def item_fold(self, slot, count_col, prev_col, min_count=1, record=None):
        """sk_item_fold: the slot's values v go into counts[count_col] += v and counts[prev_col] += (v >= min_count), the slot is
        zero again; record: a device pointer (dev_alloc) to two u64 that {rows with v >= min_count, sum of v} are added to.
        Asynchronous."""
        self._ck(lib.sk_item_fold(self._h, slot, count_col, prev_col, min_count, record))

    def tally_batch(self, stream: bytes, rec_start, type_col=0, informative_value=2):
        """Per-record tallies (strain_detect): returns (tally[nrec, 2], hits[n, 2] sorted by position)."""
        rec_start = np.ascontiguousarray(rec_start, dtype=np.uint32)
        nrec = len(rec_start)
        tally = np.zeros((nrec, 2), dtype=np.uint32)
        cap = max(len(stream), 16)
        hits = np.zeros((cap, 2), dtype=np.uint32)
        nh = C.c_uint64(0)
        self._ck(lib.sk_tally_batch(self._h, stream, len(stream), rec_start.ctypes.data, nrec, type_col, informative_value,
                                    tally.ctypes.data, hits.ctypes.data, cap, C.byref(nh)))
        hits = hits[: nh.value]
        return tally, hits[np.argsort(hits[:, 0], kind="stable")]

    def tally_launch(self, batch, type_col=0, informative_value=2, hits_cap=None):
        """sk_tally_launch on a filled TallyBatch (returns at once; hits_cap default: one entry per byte of the batch)"""
        cap = max(batch.nbytes, 16) if hits_cap is None else hits_cap
        self._ck(lib.sk_tally_launch(self._h, batch._h, type_col, informative_value, cap))
        self._inflight = (batch.nrec, cap)

    def tally_collect(self):
        """sk_tally_collect of the launch in flight: (tally[nrec, 2], hits[min(n, cap), 2] as stored, n = the true count)"""
        nrec, cap = self._inflight
        tally = np.zeros((nrec, 2), dtype=np.uint32)
        hits = np.zeros((max(cap, 1), 2), dtype=np.uint32)
        nh = C.c_uint64(0)
        self._ck(lib.sk_tally_collect(self._h, tally.ctypes.data, hits.ctypes.data, C.byref(nh)))
        return tally, hits[: min(nh.value, cap)], nh.value

    def tally_collect_sparse(self):
        """sk_tally_collect_sparse of the launch in flight: (recs[m, 3] = (record, all, informative) as stored, hits, n)"""
        nrec, cap = self._inflight
        recs = np.zeros((max(nrec, 1), 3), dtype=np.uint32)
        hits = np.zeros((max(cap, 1), 2), dtype=np.uint32)
        nr, nh = C.c_uint64(0), C.c_uint64(0)
        self._ck(lib.sk_tally_collect_sparse(self._h, recs.ctypes.data, nrec, C.byref(nr), hits.ctypes.data, C.byref(nh)))
        assert nr.value <= nrec
        return recs[: nr.value], hits[: min(nh.value, cap)], nh.value

    def tally_collect_counts(self):
        """sk_tally_collect_counts of the launch in flight: (hit records, log entries); the results themselves stay on the device
        for CoverageAcc.add / tally_fetch_held until this context's next launch"""
        nr, nh = C.c_uint64(0), C.c_uint64(0)
        self._ck(lib.sk_tally_collect_counts(self._h, C.byref(nr), C.byref(nh)))
        self._held = (nr.value, nh.value, self._inflight[1])
        return nr.value, nh.value

    def tally_fetch_held(self):
        """sk_tally_fetch_held: the held results in tally_collect_sparse's form, (recs[m, 3], hits as stored)"""
        nr, nh, cap = self._held
        recs = np.zeros((max(nr, 1), 3), dtype=np.uint32)
        hits = np.zeros((max(min(nh, cap), 1), 2), dtype=np.uint32)
        self._ck(lib.sk_tally_fetch_held(self._h, recs.ctypes.data, nr, hits.ctypes.data))
        return recs[:nr], hits[: min(nh, cap)]

    def pinned_alloc(self, nbytes):
        """A pinned host buffer as a writable numpy uint8 array (free with pinned_free(arr))."""
        p = C.c_void_p()
        self._ck(lib.sk_pinned_alloc(self._h, C.byref(p), nbytes))
        arr = np.ctypeslib.as_array(C.cast(p, C.POINTER(C.c_uint8)), shape=(nbytes,))
        self._pinned = getattr(self, "_pinned", {})
        self._pinned[arr.ctypes.data] = p.value
        return arr

    def pinned_free(self, arr):
        self._ck(lib.sk_pinned_free(self._h, self._pinned.pop(arr.ctypes.data)))

    def scan_pinned(self, arr, nbytes, col, offset=0):
        t = C.c_uint64(0)
        self._ck(lib.sk_scan_pinned(self._h, arr.ctypes.data + offset, nbytes, col, C.byref(t)))
        return t.value

    def scan_device_packed(self, dev_ptr, nbytes, col):
        self._ck(lib.sk_scan_device_packed(self._h, dev_ptr, nbytes, col))

    def scan_pinned_packed(self, packed_arr, nbytes, col):
        """a batch packed by pack_stream() into page-locked memory (pinned_alloc): returns the ticket"""
        t = C.c_uint64(0)
        self._ck(lib.sk_scan_pinned_packed(self._h, packed_arr.ctypes.data, nbytes, col, C.byref(t)))
        return t.value

    def _many(self, others):
        """self's handle, then those of `others` (KmerContext or KmerUnion: the union's own context), as a C array"""
        hs = [self._h] + [o.context_handle if isinstance(o, KmerUnion) else o._h for o in others]
        return (C.c_void_p * len(hs))(*hs), len(hs)

    def scan_pinned_many(self, others, arr, nbytes, col, offset=0):
        """sk_scan_pinned_many: one upload of a pinned batch (this context's staging ring and ticket), scanned into column `col` of
        this context and of every one in `others`; returns the ticket (ticket_wait on this context)"""
        t = C.c_uint64(0)
        hs, n = self._many(others)
        self._ck(lib.sk_scan_pinned_many(hs, n, arr.ctypes.data + offset, nbytes, col, C.byref(t)))
        return t.value

    def scan_pinned_packed_many(self, others, packed_arr, nbytes, col):
        """sk_scan_pinned_packed_many: scan_pinned_many for a batch packed by pack_stream() into page-locked memory"""
        t = C.c_uint64(0)
        hs, n = self._many(others)
        self._ck(lib.sk_scan_pinned_packed_many(hs, n, packed_arr.ctypes.data, nbytes, col, C.byref(t)))
        return t.value

    def pack_device(self, dev_stream, nbytes, dev_packed):
        """sk_pack_device: the record stream at device pointer dev_stream packed into dev_packed (packed_bytes(nbytes) bytes, 8-byte
        aligned) as pack_stream() packs it on the host; returns the odd flag"""
        odd = C.c_int(0)
        self._ck(lib.sk_pack_device(self._h, dev_stream, nbytes, dev_packed, C.byref(odd)))
        return bool(odd.value)

    def scan_pinned_pack_many(self, others, arr, nbytes, col, packed_out, odd_out):
        """sk_scan_pinned_pack_many: scan_pinned_many plus the device's pack of the same bytes, sent home into packed_out (pinned uint8
        array, packed_bytes(nbytes)) and odd_out (pinned, 4 bytes: a u32); returns the ticket for pack_ticket_wait"""
        t = C.c_uint64(0)
        hs, n = self._many(others)
        self._ck(lib.sk_scan_pinned_pack_many(hs, n, arr.ctypes.data, nbytes, col, packed_out.ctypes.data, odd_out.ctypes.data, C.byref(t)))
        return t.value

    def pack_ticket_wait(self, ticket):
        self._ck(lib.sk_pack_ticket_wait(self._h, ticket))

    def pack_cache(self, directory, mode="rw"):
        """skh_pack_cache_set: the packed input cache of scan_file / scan_list[_many] on this context; None: follow the process-wide
        default (SK_PACK_CACHE) again, "": off for this context"""
        if directory is None:
            self._ck(lib.skh_pack_cache_set(self._h, None, None))
        else:
            self._ck(lib.skh_pack_cache_set(self._h, os.fsencode(directory), mode.encode()))

    def pack_cache_stats(self, reset=False):
        """list items (served, written, stale, not_cached) since the last reset"""
        v = [C.c_uint64(0) for _ in range(4)]
        self._ck(lib.skh_pack_cache_stats(self._h, *[C.byref(x) for x in v], int(reset)))
        return tuple(x.value for x in v)

    def device_memory(self):
        """(free, total) bytes of HBM on this context's device"""
        f, t = C.c_uint64(0), C.c_uint64(0)
        self._ck(lib.sk_device_memory(self._h, C.byref(f), C.byref(t)))
        return f.value, t.value

    def ticket_wait(self, ticket):
        self._ck(lib.sk_ticket_wait(self._h, ticket))

    def scan_device(self, dev_ptr, nbytes, col):
        self._ck(lib.sk_scan_device(self._h, dev_ptr, nbytes, col))

    def scan_file(self, path, col):
        bases = C.c_uint64(0)
        self._ck(lib.skh_scan_file(self._h, os.fsencode(path), col, C.byref(bases)))
        return bases.value

    def scan_list(self, list_path, col, skip=None, rank=0, world=1, uncut=False, progress_path=None, err_path=None):
        """skh_scan_list; uncut=True: the whole-file plan (skh_scan_list_uncut).  With world > 1 and no in-library communicator
        a cut that does not hold raises SKError(SK_E_SPLIT): use strainer2_amd.dist.scan_list_sharded, which agrees across
        the ranks and scans again uncut."""
        bases = C.c_uint64(0)
        fn = lib.skh_scan_list_uncut if uncut else lib.skh_scan_list
        prog = _libc.fopen(os.fsencode(progress_path), b"w") if progress_path is not None else None
        err = _libc.fopen(os.fsencode(err_path), b"w") if err_path is not None else None
        try:
            self._ck(fn(self._h, os.fsencode(list_path), None if skip is None else os.fsencode(skip),
                        col, prog, err, rank, world, C.byref(bases)))
        finally:
            for f in (prog, err):
                if f:
                    _libc.fclose(f)
        return bases.value

    def scan_list_many(self, others, list_path, col, skip=None):
        """skh_scan_list_many: one decode of the list into column `col` of this context and of every one in `others`; returns the
        bases decoded"""
        bases = C.c_uint64(0)
        hs, n = self._many(others)
        self._ck(lib.skh_scan_list_many(hs, n, os.fsencode(list_path), None if skip is None else os.fsencode(skip),
                                        col, None, None, 0, 1, C.byref(bases)))
        return bases.value

    @staticmethod
    def list_plan_owners(list_path, world, skip=None):
        """per list line the rank that scans it (skh_list_plan_owners; 0xFFFFFFFF skipped, 0xFFFFFFFE cut across ranks)"""
        n = C.c_uint32(0)
        args = (os.fsencode(list_path), None if skip is None else os.fsencode(skip), world)
        rc = lib.skh_list_plan_owners(*args, None, 0, C.byref(n))
        own = np.empty(max(n.value, 1), dtype=np.uint32)
        if rc == SK_OK:
            rc = lib.skh_list_plan_owners(*args, own.ctypes.data, n.value, C.byref(n))
        if rc != SK_OK:
            raise OSError(f"skh_list_plan_owners({list_path}) failed: {rc}")
        return own[: n.value]

    def sync(self):
        self._ck(lib.sk_sync(self._h))

    @staticmethod
    def list_plan_hash(list_path, world, skip=None):
        """hash of the work plan scan_list(list_path, .., world=world) follows on every rank (skh_list_plan_hash)"""
        h = C.c_uint64(0)
        rc = lib.skh_list_plan_hash(os.fsencode(list_path), None if skip is None else os.fsencode(skip), world, C.byref(h))
        if rc != SK_OK:
            raise OSError(f"skh_list_plan_hash({list_path}) failed: {rc}")
        return h.value

    def counts(self, col):
        out = np.empty(self.nrows, dtype=np.uint32)
        if self.nrows:
            self._ck(lib.sk_counts_fetch(self._h, col, out.ctypes.data))
        return out

    def set_counts(self, col, values):
        values = np.ascontiguousarray(values, dtype=np.uint32)
        assert values.size == self.nrows
        self._ck(lib.sk_counts_set(self._h, col, values.ctypes.data))

    def set_counts_rows(self, col, rows, value):
        """counts[col][rows[i]] = value (sk_counts_set_rows)"""
        rows = np.ascontiguousarray(rows, dtype=np.uint32)
        self._ck(lib.sk_counts_set_rows(self._h, col, rows.ctypes.data, rows.size, value))

    def zero_counts(self, col):
        self._ck(lib.sk_counts_zero(self._h, col))

    nrows = property(lambda self: lib.sk_table_rows(self._h))
    ncols = property(lambda self: lib.sk_table_cols(self._h))

    def counts_device_ptr(self):
        return lib.sk_counts_device_ptr(self._h)

    def scan_timing(self, reset=False):
        ms = C.c_double(0)
        n = C.c_uint64(0)
        self._ck(lib.sk_scan_timing(self._h, C.byref(ms), C.byref(n), int(reset)))
        return ms.value, n.value

    def dev_alloc(self, nbytes):
        p = C.c_void_p()
        self._ck(lib.sk_dev_alloc(self._h, C.byref(p), nbytes))
        self._bufs.append(p.value)
        return p.value

    def dev_free(self, ptr):
        self._ck(lib.sk_dev_free(self._h, ptr))
        self._bufs.remove(ptr)

    def dev_upload(self, ptr, arr, offset=0):
        arr = np.ascontiguousarray(arr)
        self._ck(lib.sk_dev_upload(self._h, ptr + offset, arr.ctypes.data, arr.nbytes))

    def dev_download(self, ptr, nbytes):
        out = np.empty(nbytes, dtype=np.uint8)
        self._ck(lib.sk_dev_download(self._h, out.ctypes.data, ptr, nbytes))
        return out

    def distinct_count(self, keys, sample, nsamples):
        keys = np.ascontiguousarray(keys, dtype=np.uint64)
        sample = np.ascontiguousarray(sample, dtype=np.uint32)
        assert len(keys) == len(sample)
        uniq = np.zeros(nsamples, dtype=np.uint64)
        total = np.zeros(nsamples, dtype=np.uint64)
        self._ck(lib.sk_distinct_count(self._h, keys.ctypes.data, sample.ctypes.data, len(keys), nsamples,
                                       uniq.ctypes.data, total.ctypes.data))
        return uniq, total

    def first_seen_count(self, ids, sample, nids, nsamples):
        """sk_first_seen_count: (unique[nsamples], total[nsamples]) -- every line counts for its sample; an id (< nids) counts once, for
        the sample of the first line that shows it"""
        ids = np.ascontiguousarray(ids, dtype=np.uint32)
        sample = np.ascontiguousarray(sample, dtype=np.uint32)
        assert len(ids) == len(sample)
        uniq = np.zeros(nsamples, dtype=np.uint64)
        total = np.zeros(nsamples, dtype=np.uint64)
        self._ck(lib.sk_first_seen_count(self._h, ids.ctypes.data, sample.ctypes.data, len(ids), nids, nsamples,
                                         uniq.ctypes.data, total.ctypes.data))
        return uniq, total

    def distinct_spectrum(self, keys, sample, nsamples, max_depth):
        """sk_distinct_spectrum: (unique[nsamples], total[nsamples], spec[nsamples, max_depth + 1], deep[nsamples]) -- distinct_count,
        and per sample how many of its keys came 1, 2, ..., max_depth and (last column) more than max_depth times; deep = the sum of
        the multiplicities above max_depth"""
        keys = np.ascontiguousarray(keys, dtype=np.uint64)
        sample = np.ascontiguousarray(sample, dtype=np.uint32)
        assert len(keys) == len(sample)
        nb = max(int(max_depth), 0) + 1
        uniq, total, deep = (np.zeros(nsamples, dtype=np.uint64) for _ in range(3))
        spec = np.zeros((nsamples, nb), dtype=np.uint64)
        self._ck(lib.sk_distinct_spectrum(self._h, keys.ctypes.data, sample.ctypes.data, len(keys), nsamples, int(max_depth),
                                          uniq.ctypes.data, total.ctypes.data, spec.ctypes.data, deep.ctypes.data))
        return uniq, total, spec, deep

    def distinct_recurrence(self, keys, sample, nsamples, pairs=False):
        """sk_distinct_recurrence: hist[nsamples + 1] -- hist[m] = distinct keys seen in exactly m samples, hist[0] left 0 -- and, with
        pairs, shared[nsamples, nsamples]: the distinct keys two samples have in common (the diagonal: a sample's own)"""
        keys = np.ascontiguousarray(keys, dtype=np.uint64)
        sample = np.ascontiguousarray(sample, dtype=np.uint32)
        assert len(keys) == len(sample)
        hist = np.zeros(max(int(nsamples), 0) + 1, dtype=np.uint64)
        pr = np.zeros((max(int(nsamples), 0),) * 2, dtype=np.uint64) if pairs else None
        self._ck(lib.sk_distinct_recurrence(self._h, keys.ctypes.data, sample.ctypes.data, len(keys), int(nsamples), hist.ctypes.data,
                                            pr.ctypes.data if pairs else None))
        return (hist, pr) if pairs else hist

    def distinct_thresholds(self, keys, sample, total_hits, nsamples, thresholds):
        """sk_distinct_thresholds: (unique[nsamples, nt], total[nsamples, nt]) -- for every sample and threshold t the hits whose
        total_hits exceeds t, and the distinct keys they name"""
        keys = np.ascontiguousarray(keys, dtype=np.uint64)
        sample = np.ascontiguousarray(sample, dtype=np.uint32)
        total_hits = np.ascontiguousarray(total_hits, dtype=np.uint32)
        t = np.ascontiguousarray(thresholds, dtype=np.int64).reshape(-1)
        assert len(keys) == len(sample) == len(total_hits)
        uniq = np.zeros((max(int(nsamples), 0), len(t)), dtype=np.uint64)
        total = np.zeros_like(uniq)
        self._ck(lib.sk_distinct_thresholds(self._h, keys.ctypes.data, sample.ctypes.data, total_hits.ctypes.data, len(keys), int(nsamples),
                                            t.ctypes.data, len(t), uniq.ctypes.data, total.ctypes.data))
        return uniq, total

    def distinct_classes(self, keys, sample, cls, nsamples, ncls):
        """sk_distinct_classes: (unique[nsamples, ncls], total[nsamples, ncls]) -- for every sample and fraction q the hits of class
        >= q + 1, and the distinct keys they name; classes run from 1 to ncls"""
        keys = np.ascontiguousarray(keys, dtype=np.uint64)
        sample = np.ascontiguousarray(sample, dtype=np.uint32)
        cls = np.ascontiguousarray(cls, dtype=np.uint8)
        assert len(keys) == len(sample) == len(cls)
        uniq = np.zeros((max(int(nsamples), 0), max(int(ncls), 1)), dtype=np.uint64)
        total = np.zeros_like(uniq)
        self._ck(lib.sk_distinct_classes(self._h, keys.ctypes.data, sample.ctypes.data, cls.ctypes.data, len(keys), int(nsamples), int(ncls),
                                         uniq.ctypes.data, total.ctypes.data))
        return uniq, total

    def print_counts(self, ks: Keyset, path, with_drug_column=False):
        fp = _libc.fopen(os.fsencode(path), b"w")
        try:
            self._ck(lib.skh_print_counts(self._h, C.byref(ks._s), fp, int(with_drug_column)))
        finally:
            _libc.fclose(fp)

    def close(self):
        if self._h:
            for p in list(self._bufs):
                lib.sk_dev_free(self._h, p)
            self._bufs = []
            lib.sk_text_release(self._h)
            lib.sk_pack_release(self._h)
            lib.skh_pack_cache_set(self._h, None, None)
            lib.sk_ctx_destroy(self._h)
            self._h = None

    def __del__(self):
        self.close()

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()


def target_cache_stats(reset=False):
    """skh_target_cache_stats: (served, written, stale, not cached) targets of strain_detect runs in this process"""
    v = [C.c_uint64(0) for _ in range(4)]
    lib.skh_target_cache_stats(*[C.byref(x) for x in v], int(reset))
    return tuple(int(x.value) for x in v)


def coverage_only_stats(reset=False):
    """skh_coverage_only_stats: (runs counted on the device, runs replayed on the host, targets counted by the host accumulator) of
    the strain_detect --coverage-only runs in this process"""
    v = [C.c_uint64(0) for _ in range(3)]
    lib.skh_coverage_only_stats(*[C.byref(x) for x in v], int(reset))
    return tuple(int(x.value) for x in v)


SKH_REGIONS_MAX = 1 << 20


class _RegionsStruct(C.Structure):
    """skh_regions"""
    _fields_ = [("n", C.c_uint32), ("nnames", C.c_uint32), ("text_bases", C.c_uint64), ("text_off", C.POINTER(C.c_uint64)),
                ("record", C.POINTER(C.c_uint32)), ("rec_off", C.POINTER(C.c_uint64)), ("len", C.POINTER(C.c_uint64)),
                ("name", C.POINTER(C.c_char_p)), ("names", C.POINTER(C.c_char_p)), ("too_many", C.c_int)]


lib.skh_regions_from_file.argtypes = [C.c_char_p, C.c_uint64, C.POINTER(_RegionsStruct)]
lib.skh_regions_free.argtypes = [C.POINTER(_RegionsStruct)]
lib.skh_regions_free.restype = None
lib.sk_table_first_pos.argtypes = [C.c_void_p, C.c_void_p]
lib.sk_table_build_from_text.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.POINTER(C.c_uint32)]
lib.sk_covacc_set_regions.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_uint32]
lib.sk_covacc_region_rows.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p]
lib.sk_covacc_finish_target_regions.argtypes = [C.c_void_p] * 5
SK_COVACC_SPECTRUM_MAX = 1023
lib.sk_covacc_set_spectrum.argtypes = [C.c_void_p, C.c_uint32]
lib.sk_covacc_finish_target_spectrum.argtypes = [C.c_void_p] * 7
lib.sk_distinct_spectrum.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint32, C.c_uint32] + [C.c_void_p] * 4


SK_RECUR_SAMPLES_MAX = 4096
SK_RECUR_PAIRS_MAX = 256
SK_RECUR_MEMBERS_MAX = 65535
lib.sk_recur_create.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_void_p]
lib.sk_recur_destroy.argtypes = [C.c_void_p]
lib.sk_recur_destroy.restype = None
lib.sk_recur_mark_bits.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_uint64]
lib.sk_recur_finish.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
lib.sk_covacc_set_recurrence.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p]
lib.sk_covacc_mark_target.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p]
lib.sk_distinct_recurrence.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint32, C.c_void_p, C.c_void_p]
SK_COVACC_THRESHOLDS_MAX = 16
DEFAULT_THRESHOLDS = (0, 1, 2, 3, 5, 10, 20, 50)
lib.sk_covacc_set_thresholds.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32]
lib.sk_covacc_add_rows_hits.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_uint64]
lib.sk_covacc_finish_target_thresholds.argtypes = [C.c_void_p] * 3
lib.sk_distinct_thresholds.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint32, C.c_void_p, C.c_uint32,
                                       C.c_void_p, C.c_void_p]
lib.sk_covacc_set_classes.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint32]
lib.sk_covacc_finish_target_classes.argtypes = [C.c_void_p] * 4
lib.sk_distinct_classes.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p]
SK_COVACC_SUPPORT_MEMBERS_MAX = 1024
lib.sk_covacc_set_support.argtypes = [C.c_void_p, C.c_int]
lib.sk_covacc_finish_target_support.argtypes = [C.c_void_p] * 6
SK_COVACC_RAREFACTION_MAX = 16
DEFAULT_RAREFACTION = "1,0.5,0.25,0.125,0.0625,0.03125"
lib.sk_covacc_set_rarefaction.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32]
lib.sk_covacc_set_pair_base.argtypes = [C.c_void_p, C.c_uint64]
lib.sk_covacc_add_pairs.argtypes = [C.c_void_p, C.c_uint64, C.c_uint64]
lib.sk_covacc_add_rows_hits_pairs.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64]
lib.sk_covacc_finish_target_rarefaction.argtypes = [C.c_void_p] * 4
lib.sk_covacc_rarefaction_timing_.argtypes = [C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_double)]


class RarefactionList(C.Structure):
    """skh_rarefaction: the parsed --rarefaction-list"""
    _fields_ = [("n", C.c_uint32), ("seed", C.c_uint32), ("T", C.c_uint64 * 16), ("text", (C.c_char * 40) * 16)]


lib.skh_rarefaction_parse.argtypes = [C.c_char_p, C.c_uint32, C.POINTER(RarefactionList)]
lib.skh_rarefaction_draw.argtypes = [C.c_uint64, C.c_uint32]
lib.skh_rarefaction_draw.restype = C.c_uint32
lib.skh_rarefaction_class.argtypes = [C.POINTER(RarefactionList), C.c_uint64]
lib.skh_rarefaction_class.restype = C.c_uint32
lib.skh_rarefaction_fold.argtypes = [C.POINTER(RarefactionList), C.c_int64, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64,
                                     C.c_uint64, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p]


def rarefaction_parse(text=None, seed=0):
    """skh_rarefaction_parse: (T list, the fields' texts) of a --rarefaction-list (None: the default); SKError(SK_E_ARG) for a list
    the rule refuses"""
    r = RarefactionList()
    rc = lib.skh_rarefaction_parse(None if text is None else text.encode(), seed, C.byref(r))
    if rc != SK_OK:
        raise SKError(rc, "rarefaction list %r" % (text,))
    return [int(r.T[q]) for q in range(r.n)], [r.text[q].value.decode() for q in range(r.n)]


lib.sk_covacc_timing_.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_double), C.POINTER(C.c_double)]
lib.sk_covacc_support_timing_.argtypes = [C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_double)]


def regions_from_file(path, window=100000):
    """skh_regions_from_file: (regions, text_bases); regions = [(text offset, record number from 1, offset in the record, length,
    record name as bytes)] in text order -- the strain's records of 30 bases or more cut into windows of `window` bases (0: one
    region per record).  More than SKH_REGIONS_MAX regions: SKError."""
    s = _RegionsStruct()
    rc = lib.skh_regions_from_file(os.fsencode(path), int(window), C.byref(s))
    if rc:
        raise SKError(rc, f"{path}: more than {SKH_REGIONS_MAX} regions" if s.too_many else str(path))
    try:
        return [(int(s.text_off[i]), int(s.record[i]), int(s.rec_off[i]), int(s.len[i]), s.name[i]) for i in range(s.n)], int(s.text_bases)
    finally:
        lib.skh_regions_free(C.byref(s))


def distinct_thresholds(ctx, keys, sample, total_hits, nsamples, thresholds=DEFAULT_THRESHOLDS):
    """KmerContext.distinct_thresholds on ctx"""
    return ctx.distinct_thresholds(keys, sample, total_hits, nsamples, thresholds)


def distinct_spectrum(ctx, keys, sample, nsamples, max_depth=255):
    """KmerContext.distinct_spectrum on ctx"""
    return ctx.distinct_spectrum(keys, sample, nsamples, max_depth)


class TallyBatch:
    """A batch of records resident on a context's device (sk_batch_*), to be tallied against one or more tables."""

    def __init__(self, ctx: KmerContext):
        self._ctx = ctx
        self._h = C.c_void_p()
        ctx._ck(lib.sk_batch_create(ctx._h, C.byref(self._h)))
        self.nbytes = self.nrec = 0

    def fill(self, stream: bytes, rec_start, packed=False):
        """upload a record stream (packed: in sk_pack_stream's form, which must hold no odd byte); rec_start as in tally_batch"""
        rec_start = np.ascontiguousarray(rec_start, dtype=np.uint32)
        if packed:
            buf, odd = pack_stream(stream)
            assert not odd, "a packed batch holds only A/C/G/T, N and newlines"
            rc = lib.sk_batch_fill_packed(self._h, buf.ctypes.data, len(stream), rec_start.ctypes.data, len(rec_start))
        else:
            buf = np.frombuffer(stream, dtype=np.uint8) if isinstance(stream, (bytes, bytearray)) else np.ascontiguousarray(stream, dtype=np.uint8)
            rc = lib.sk_batch_fill(self._h, buf.ctypes.data, buf.size, rec_start.ctypes.data, len(rec_start))
        self._ctx._ck(rc)
        self._ctx._ck(lib.sk_batch_sync(self._h))        # (the upload is done: buf may go)
        self.nbytes, self.nrec = len(stream), len(rec_start)

    def fill_text(self, text, is_eof=True, lookahead=b""):
        """sk_batch_fill_text + sk_batch_text_finish: a piece of plain FASTA/FASTQ text goes up as it is and the device parses it into
        this batch.  is_eof False: `lookahead` is the one byte that follows the piece in its file.  Returns (TextInfo, rec_start) --
        the starts of EVERY record of the piece, short and empty ones included; with status DECLINED (or no records) the batch
        cannot be launched on."""
        data = np.frombuffer(bytes(text) + (b"" if is_eof else bytes(lookahead)), dtype=np.uint8)
        buf = self._ctx.pinned_alloc(max(data.size, 16))
        info = TextInfo()
        rs = C.POINTER(C.c_uint32)()
        try:
            buf[: data.size] = data
            self._ctx._ck(lib.sk_batch_fill_text(self._h, buf.ctypes.data, data.size, int(bool(is_eof))))
            self._ctx._ck(lib.sk_batch_text_finish(self._h, C.byref(info), C.byref(rs)))
        finally:
            self._ctx.pinned_free(buf)
        ok = info.status == 0 and info.nrecords > 0
        starts = np.ctypeslib.as_array(rs, shape=(int(info.nrecords),)).copy() if ok else np.zeros(0, dtype=np.uint32)
        self.nbytes, self.nrec = (int(info.stream_bytes), int(info.nrecords)) if ok else (0, 0)
        return info, starts

    def pack_home_begin(self, out, flag):
        """sk_batch_pack_home alone: the device pack of the bytes this batch holds is enqueued behind their upload; `out` (a pinned
        uint8 array of at least sk_packed_bytes(nbytes)) and `flag` (a pinned uint32 array) hold the result once pack_home_wait returned"""
        self._ctx._ck(lib.sk_batch_pack_home(self._h, out.ctypes.data, flag.ctypes.data))

    def pack_home_wait(self):
        self._ctx._ck(lib.sk_batch_pack_wait(self._h))

    def pack_home(self, guard=0):
        """the bytes this batch holds, packed on the device into sk_pack_stream's form: (packed bytes as a uint8 array, odd).
        guard > 0: that many bytes behind the packed form are returned as well, filled with 0xA5 before the call (tests: the
        copy home must leave them alone)"""
        n = int(lib.sk_packed_bytes(self.nbytes))
        buf = self._ctx.pinned_alloc(n + guard + 16)
        try:
            buf[:] = 0xA5
            flag = buf[(n + guard + 7) // 8 * 8:][:4].view(np.uint32)
            self.pack_home_begin(buf, flag)
            self.pack_home_wait()
            return buf[: n + guard].copy(), bool(flag[0])
        finally:
            self._ctx.pinned_free(buf)

    def close(self):
        if getattr(self, "_h", None):
            lib.sk_batch_destroy(self._h)
            self._h = None

    def __del__(self):
        self.close()

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()


class KmerUnion:
    """One table for several resident strains (sk_union_*): a batch is tallied against all of them in one launch."""

    def __init__(self, contexts, type_col=0, informative_value=2):
        self._members = list(contexts)                    # (they must outlive the union)
        arr = (C.c_void_p * len(self._members))(*[c._h for c in self._members])
        self._h = C.c_void_p()
        rc = lib.sk_union_create(arr, len(self._members), type_col, informative_value, C.byref(self._h))
        if rc:
            self._h = None
            raise SKError(rc, lib.sk_last_error(self._members[0]._h).decode() if self._members else "no members")
        self._batch = C.c_void_p()
        rc = lib.sk_batch_create(self._members[0]._h, C.byref(self._batch))
        if rc:
            raise SKError(rc, "sk_batch_create")

    @property
    def rows(self):
        return lib.sk_union_rows(self._h)

    @property
    def context_handle(self):
        """the union's own context (sk_union_context): what the COUNT scans take"""
        return lib.sk_union_context(self._h)

    def counts(self, col=0):
        """union column `col` in global-row order (sk_counts_fetch on the union's context)"""
        out = np.zeros(self.rows, dtype=np.uint32)
        self._uck(lib.sk_counts_fetch(lib.sk_union_context(self._h), col, out.ctypes.data))
        return out

    def set_option(self, name, value):
        """sk_set_option on the union's own context (e.g. "odd_list_cap" for its scans)"""
        self._uck(lib.sk_set_option(lib.sk_union_context(self._h), name.encode(), value))

    def tally_batch(self, stream: bytes, rec_start, hits_cap=None, packed=False):
        """returns (tally[nrec, members, 2], hits[n, 3] = (member, window-end offset, the member's row) sorted);
        packed: the batch goes up in sk_pack_stream's form (it must hold no odd byte)"""
        rec_start = np.ascontiguousarray(rec_start, dtype=np.uint32)
        nrec, n = len(rec_start), len(self._members)
        if packed:
            pk, odd = pack_stream(stream)
            assert not odd, "a packed batch holds only A/C/G/T, N and newlines"
            rc = lib.sk_batch_fill_packed(self._batch, pk.ctypes.data, len(stream), rec_start.ctypes.data, nrec)
        else:
            rc = lib.sk_batch_fill(self._batch, stream, len(stream), rec_start.ctypes.data, nrec)
        if rc:
            raise SKError(rc, lib.sk_last_error(self._members[0]._h).decode())
        return self._tally(self._batch, nrec, len(stream), hits_cap)

    def tally_filled(self, batch, hits_cap=None):
        """tally_batch for a TallyBatch that is filled already (fill or fill_text) on this union's device"""
        return self._tally(batch._h, batch.nrec, batch.nbytes, hits_cap)

    def _tally(self, batch_h, nrec, nbytes, hits_cap):
        n = len(self._members)
        cap = hits_cap if hits_cap is not None else max(nbytes * 2, 16)
        while True:
            rc = lib.sk_union_tally_launch(self._h, batch_h, cap)
            if rc:
                raise SKError(rc, lib.sk_union_last_error(self._h).decode())
            recs = np.zeros((nrec * n + 1, 3), dtype=np.uint32)
            hits = np.zeros((max(cap, 1), 2), dtype=np.uint32)
            nr, nh = C.c_uint64(0), C.c_uint64(0)
            rc = lib.sk_union_tally_collect(self._h, recs.ctypes.data, nrec * n, C.byref(nr), hits.ctypes.data, C.byref(nh))
            if rc:
                raise SKError(rc, lib.sk_union_last_error(self._h).decode())
            if nh.value <= cap:
                break
            cap = nh.value + 16                           # the log overflowed: once more with room
        tally = np.zeros((nrec * n, 2), dtype=np.uint32)
        recs = recs[: nr.value]
        tally[recs[:, 0]] = recs[:, 1:]
        hits = hits[: nh.value]
        out = np.stack([hits[:, 1] >> 27, hits[:, 0], hits[:, 1] & ((1 << 27) - 1)], axis=1) if len(hits) else np.zeros((0, 3), dtype=np.uint32)
        order = np.lexsort((out[:, 2], out[:, 1], out[:, 0]))
        return tally.reshape(nrec, n, 2), out[order]

    def tally_launch(self, batch, hits_cap=None, results_stay=False):
        """sk_union_tally_launch[_ex] on a filled TallyBatch; returns at once.  results_stay: only the counters travel home with
        the launch (for tally_collect_counts)"""
        cap = max(batch.nbytes * 2, 16) if hits_cap is None else hits_cap
        self._uck(lib.sk_union_tally_launch_ex(self._h, batch._h, cap, int(bool(results_stay))))
        self._inflight = (batch.nrec, cap)

    def tally_collect_counts(self):
        """sk_union_tally_collect_counts: ((record, member) pairs hit, log entries); the results stay on the device"""
        nr, nh = C.c_uint64(0), C.c_uint64(0)
        self._uck(lib.sk_union_tally_collect_counts(self._h, C.byref(nr), C.byref(nh)))
        self._held = (nr.value, nh.value, self._inflight[1])
        return nr.value, nh.value

    def tally_fetch_held(self):
        """sk_union_tally_fetch_held: (recs[m, 3] = (record * members + member, all, informative), hits[n, 2] as stored)"""
        nr, nh, cap = self._held
        recs = np.zeros((max(nr, 1), 3), dtype=np.uint32)
        hits = np.zeros((max(min(nh, cap), 1), 2), dtype=np.uint32)
        self._uck(lib.sk_union_tally_fetch_held(self._h, recs.ctypes.data, nr, hits.ctypes.data))
        return recs[:nr], hits[: min(nh, cap)]

    # ---- COUNT on the union (sk_union_count_enable / sk_union_context / sk_union_counts_fold)
    def _uck(self, rc):
        if rc:
            raise SKError(rc, lib.sk_union_last_error(self._h).decode())

    def count_enable(self, ncols=1):
        """give the union's context ncols zeroed count columns of global rows (needed before scan_stream / fold_counts)"""
        self._uck(lib.sk_union_count_enable(self._h, ncols))

    def scan_stream(self, stream, col=0):
        """count a host record stream into union column `col` (sk_scan_stream on the union's context)"""
        ctx = lib.sk_union_context(self._h)
        if isinstance(stream, np.ndarray):
            stream = np.ascontiguousarray(stream, dtype=np.uint8)
            self._uck(lib.sk_scan_stream(ctx, stream.ctypes.data, stream.size, col))
        else:
            self._uck(lib.sk_scan_stream(ctx, stream, len(stream), col))

    def fold_counts(self, ucol, member_col, member_mask=None, subtract=False):
        """fold union column `ucol` into column `member_col` of the members in member_mask (default: all), then zero it"""
        if member_mask is None:
            member_mask = (1 << len(self._members)) - 1
        self._uck(lib.sk_union_counts_fold(self._h, ucol, member_col, member_mask & 0xFFFFFFFF, int(bool(subtract))))

    def item_slots(self, nslots):
        """sk_item_slots on the union's context: nslots item slots of global rows (8 bytes x rows each); 0 frees them"""
        self._uck(lib.sk_item_slots(lib.sk_union_context(self._h), nslots))

    def item_slot(self, slot):
        """sk_item_slot on the union's context: its COUNT scans add into item slot `slot` from now on; -1: into the column they name"""
        self._uck(lib.sk_item_slot(lib.sk_union_context(self._h), slot))

    def item_fold(self, slot, count_col, prev_col, member_mask=None, min_count=1, records=None):
        """sk_union_item_fold: with V a key's count in the slot, every member of member_mask (default: all) gets
        counts[count_col] += V and counts[prev_col] += (V >= min_count) on its rows, the slot is zero again; records: a device
        pointer to [members][2] u64 that {rows with V >= min_count, sum of V} of each such member are added to.  Asynchronous."""
        if member_mask is None:
            member_mask = (1 << len(self._members)) - 1
        self._uck(lib.sk_union_item_fold(self._h, slot, count_col, prev_col, member_mask & 0xFFFFFFFF, min_count, records))

    def scan_batch(self, batch, col=0):
        """sk_scan_batch on the union's context: ONE count scan of a filled TallyBatch into union column col"""
        self._uck(lib.sk_scan_batch(lib.sk_union_context(self._h), batch._h, col))

    def sync(self):
        self._uck(lib.sk_sync(lib.sk_union_context(self._h)))

    def background_finish(self, ucol=0, max_depth=63):
        """sk_union_background_finish: uint64[members, 2, 5 + max_depth + 1], each member's block as KmerContext.background_finish
        returns it; union column ucol is zero afterwards"""
        out = np.zeros((len(self._members), 2, SK_BACKGROUND_HEAD + max_depth + 1), dtype=np.uint64)
        self._uck(lib.sk_union_background_finish(self._h, ucol, max_depth, out.ctypes.data))
        return out

    def share(self, other=None):
        """sk_union_share: (shared, informative_in_other, informative_both), three uint64 arrays [members of self, members of
        other or self] -- distinct keys member i and member j both hold, keys informative in i that j holds, keys informative
        in both.  The cells beyond the members (all zero) are kept in .share_raw for the tests."""
        raw = np.zeros((3, SK_UNION_MAX, SK_UNION_MAX), dtype=np.uint64)
        self._uck(lib.sk_union_share(self._h, other._h if other is not None else None, raw.ctypes.data))
        self.share_raw = raw
        n, m = len(self._members), len((self if other is None else other)._members)
        return tuple(raw[k, :n, :m].copy() for k in range(3))

    def scan_timing(self, reset=False):
        """(milliseconds, launches) of the union's scan kernels since the last reset, from HIP events"""
        ms = C.c_double(0)
        n = C.c_uint64(0)
        self._uck(lib.sk_union_scan_timing(self._h, C.byref(ms), C.byref(n), int(reset)))
        return ms.value, n.value

    def close(self):
        if getattr(self, "_batch", None):
            lib.sk_batch_destroy(self._batch)
            self._batch = None
        if getattr(self, "_h", None):
            lib.sk_union_destroy(self._h)
            self._h = None

    def __del__(self):
        self.close()

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()


class CoverageAcc:
    """The coverage accumulator (sk_covacc_*): per member (strain) and target, how many hit lines pass --min-kmer-hits and how
    many distinct rows they name, folded on the device from the results a tally launch leaves there
    (KmerContext/KmerUnion.tally_collect_counts)."""

    def __init__(self, ctx: KmerContext, nrows, min_kmer_hits=0):
        self._ctx = ctx
        self.nrows = np.ascontiguousarray(nrows, dtype=np.uint32).reshape(-1)
        self._h = C.c_void_p()
        ctx._ck(lib.sk_covacc_create(ctx._h, len(self.nrows), self.nrows.ctypes.data, int(min_kmer_hits), C.byref(self._h)))

    @staticmethod
    def _who(src):
        return (None, src._h) if isinstance(src, KmerUnion) else (src._h, None)

    def hold(self, src):
        """sk_covacc_hold: keep a copy of the held results of src's launch (a KmerContext or a KmerUnion) for a later add(mate=('held', ..))"""
        c, u = self._who(src)
        self._ctx._ck(lib.sk_covacc_hold(self._h, c, u))

    def add(self, src, a0, astep, npairs, mate=None, member0=0):
        """sk_covacc_add: fold the held results of src's launch.  mate: None (single reads), ('same', b0, bstep) or ('held', b0, bstep)"""
        c, u = self._who(src)
        m = None
        if mate is not None:
            m = C.byref(CovaccMate({"same": 0, "held": 1}[mate[0]], mate[1], mate[2]))
        self._ctx._ck(lib.sk_covacc_add(self._h, c, u, member0, a0, astep, npairs, m))

    def pick(self, src=None, first=False, ntail=1, from_hold=False, cap=4096, hits_cap=65536):
        """sk_covacc_pick: (records[n, 3], hits[m, 2]) of record 0 (first) and the last ntail records of src's held launch, or of
        the launch held here (from_hold), in the collect calls' form"""
        c, u = (None, None) if from_hold else self._who(src)
        recs = np.zeros((cap, 3), dtype=np.uint32)
        hits = np.zeros((hits_cap, 2), dtype=np.uint32)
        n, nh = C.c_uint64(0), C.c_uint64(0)
        self._ctx._ck(lib.sk_covacc_pick(self._h, c, u, int(from_hold), int(first), ntail, recs.ctypes.data, cap, C.byref(n),
                                         hits.ctypes.data, hits_cap, C.byref(nh)))
        if n.value > cap or nh.value > hits_cap:
            return self.pick(src, first, ntail, from_hold, max(cap, int(n.value)), max(hits_cap, int(nh.value)))
        return recs[: n.value], hits[: nh.value]

    def fetch_hold(self, cap=1 << 16, hits_cap=1 << 18):
        """sk_covacc_fetch_hold: the launch held here, in full, in the collect calls' form"""
        recs = np.zeros((cap, 3), dtype=np.uint32)
        hits = np.zeros((hits_cap, 2), dtype=np.uint32)
        n, nh = C.c_uint64(0), C.c_uint64(0)
        self._ctx._ck(lib.sk_covacc_fetch_hold(self._h, recs.ctypes.data, cap, C.byref(n), hits.ctypes.data, hits_cap, C.byref(nh)))
        if n.value > cap or nh.value > hits_cap:
            return self.fetch_hold(max(cap, int(n.value)), max(hits_cap, int(nh.value)))
        return recs[: n.value], hits[: nh.value]

    def add_rows(self, member, rows):
        rows = np.ascontiguousarray(rows, dtype=np.uint32)
        self._ctx._ck(lib.sk_covacc_add_rows(self._h, member, rows.ctypes.data, len(rows)))

    def add_rows_hits(self, member, rows, total_hits):
        """sk_covacc_add_rows_hits: unfiltered hits on these rows of member, each with its pair's total h1 + h2"""
        rows = np.ascontiguousarray(rows, dtype=np.uint32)
        total_hits = np.ascontiguousarray(total_hits, dtype=np.uint32)
        assert len(rows) == len(total_hits)
        self._ctx._ck(lib.sk_covacc_add_rows_hits(self._h, member, rows.ctypes.data, total_hits.ctypes.data, len(rows)))

    def set_thresholds(self, thresholds):
        """sk_covacc_set_thresholds: an empty list turns thresholds off; otherwise 1..SK_COVACC_THRESHOLDS_MAX strictly ascending
        integers from 0 to 2^31 - 2.  Whatever was classified since the last finish is discarded."""
        t = np.ascontiguousarray(thresholds, dtype=np.int64).reshape(-1)
        self._ctx._ck(lib.sk_covacc_set_thresholds(self._h, t.ctypes.data if len(t) else None, len(t)))
        self._thr_n = len(t)

    def finish_target_thresholds(self):
        """sk_covacc_finish_target_thresholds: (unique[nmembers, nt], total[nmembers, nt]); the depth counters are not touched, the
        threshold state is zero afterwards.  Call it before the sweep that ends the target."""
        nt = getattr(self, "_thr_n", 0)
        uq = np.zeros((len(self.nrows), max(nt, 1)), dtype=np.uint64)
        tot = np.zeros_like(uq)
        self._ctx._ck(lib.sk_covacc_finish_target_thresholds(self._h, uq.ctypes.data, tot.ctypes.data))
        return uq[:, :nt], tot[:, :nt]

    def set_rarefaction(self, T, seed=0):
        """sk_covacc_set_rarefaction: an empty list turns rarefaction off; otherwise 1..SK_COVACC_RAREFACTION_MAX strictly descending
        T[q] = floor(fraction * 2^32).  Whatever was classified since the last finish is discarded."""
        t = np.ascontiguousarray(T, dtype=np.uint64).reshape(-1)
        self._ctx._ck(lib.sk_covacc_set_rarefaction(self._h, t.ctypes.data if len(t) else None, len(t), int(seed) & 0xFFFFFFFF))
        self._rar_n = len(t)

    def set_pair_base(self, first_pair):
        """sk_covacc_set_pair_base: the target's ordinal of pair 0 of the next add()'s run"""
        self._ctx._ck(lib.sk_covacc_set_pair_base(self._h, int(first_pair)))

    def add_pairs(self, first, n):
        """sk_covacc_add_pairs: pairs first .. first + n - 1 of the target counted by class (replayed runs' pairs)"""
        self._ctx._ck(lib.sk_covacc_add_pairs(self._h, int(first), int(n)))

    def add_rows_hits_pairs(self, member, rows, total_hits, pair_ordinal):
        """sk_covacc_add_rows_hits_pairs: add_rows_hits, each hit also with its pair's ordinal in the target (u64)"""
        rows = np.ascontiguousarray(rows, dtype=np.uint32)
        total_hits = np.ascontiguousarray(total_hits, dtype=np.uint32)
        pair_ordinal = np.ascontiguousarray(pair_ordinal, dtype=np.uint64)
        assert len(rows) == len(total_hits) == len(pair_ordinal)
        self._ctx._ck(lib.sk_covacc_add_rows_hits_pairs(self._h, member, rows.ctypes.data, total_hits.ctypes.data,
                                                        pair_ordinal.ctypes.data, len(rows)))

    def finish_target_rarefaction(self):
        """sk_covacc_finish_target_rarefaction: (pairs[nq], unique[nmembers, nq], total[nmembers, nq]); the depth counters are not
        touched, the rarefaction state is zero afterwards.  Call it before the sweep that ends the target."""
        nq = getattr(self, "_rar_n", 0)
        pairs = np.zeros(max(nq, 1), dtype=np.uint64)
        uq = np.zeros((len(self.nrows), max(nq, 1)), dtype=np.uint64)
        tot = np.zeros_like(uq)
        self._ctx._ck(lib.sk_covacc_finish_target_rarefaction(self._h, pairs.ctypes.data, uq.ctypes.data, tot.ctypes.data))
        return pairs[:nq], uq[:, :nq], tot[:, :nq]

    def rarefaction_timing(self):
        """(classifying passes ms, finishing passes ms) summed while timing() is on"""
        a, b = C.c_double(0), C.c_double(0)
        self._ctx._ck(lib.sk_covacc_rarefaction_timing_(self._h, C.byref(a), C.byref(b)))
        return a.value, b.value

    def set_classes(self, member, rows, cls, ncls):
        """sk_covacc_set_classes: member's rows[i] gets the scrub class cls[i] (1..ncls), every other row class 0; ncls = 0 (and no
        rows) turns the member's classes off"""
        rows = np.ascontiguousarray(rows, dtype=np.uint32)
        cls = np.ascontiguousarray(cls, dtype=np.uint8)
        assert len(rows) == len(cls)
        self._ctx._ck(lib.sk_covacc_set_classes(self._h, member, rows.ctypes.data if len(rows) else None,
                                                cls.ctypes.data if len(cls) else None, len(rows), int(ncls)))
        self._ncls = getattr(self, "_ncls", None) or [0] * len(self.nrows)
        self._ncls[member] = int(ncls)

    def finish_target_classes(self):
        """sk_covacc_finish_target_classes: (unique[nmembers, F], total[nmembers, F], stray), F = the largest ncls set; it changes no
        counter.  Call it before the sweep that ends the target."""
        F = max(getattr(self, "_ncls", None) or [0])
        uq = np.zeros((len(self.nrows), max(F, 1)), dtype=np.uint64)
        tot = np.zeros_like(uq)
        stray = C.c_uint64()
        self._ctx._ck(lib.sk_covacc_finish_target_classes(self._h, uq.ctypes.data, tot.ctypes.data, C.byref(stray)))
        return uq[:, :F], tot[:, :F], int(stray.value)

    def rows(self, member):
        """member's per-row counters as they stand"""
        out = np.zeros(max(int(self.nrows[member]), 1), dtype=np.uint32)
        self._ctx._ck(lib.sk_covacc_rows(self._h, member, out.ctypes.data))
        return out[: int(self.nrows[member])]

    def finish_target(self):
        """(unique[nmembers], total[nmembers]) as uint64 arrays; the counters are zero afterwards"""
        uq = np.zeros(len(self.nrows), dtype=np.uint64)
        tot = np.zeros(len(self.nrows), dtype=np.uint64)
        self._ctx._ck(lib.sk_covacc_finish_target(self._h, uq.ctypes.data, tot.ctypes.data))
        return uq, tot

    def set_regions(self, member, ctx, region_start):
        """sk_covacc_set_regions: member's rows are the rows of ctx's table; each goes to the last region that starts at or before
        its first text position, rows without one to region len(region_start)"""
        rs = np.ascontiguousarray(region_start, dtype=np.uint32).reshape(-1)
        self._ctx._ck(lib.sk_covacc_set_regions(self._h, member, ctx._h, rs.ctypes.data, len(rs)))
        self._nreg = getattr(self, "_nreg", None) or [0] * len(self.nrows)
        self._nreg[member] = len(rs)

    def region_rows(self, member, ctx, type_col=0, informative_value=2):
        """sk_covacc_region_rows: (rows, informative rows) per region of member, the unplaced ones last"""
        nb = (getattr(self, "_nreg", None) or [0] * len(self.nrows))[member] + 1
        rows, inf = np.zeros(nb, dtype=np.uint64), np.zeros(nb, dtype=np.uint64)
        self._ctx._ck(lib.sk_covacc_region_rows(self._h, member, ctx._h, type_col, informative_value, rows.ctypes.data, inf.ctypes.data))
        return rows, inf

    def finish_target_regions(self):
        """sk_covacc_finish_target_regions: (unique[nmembers], total[nmembers], [per member: (unique, total) per region, the unplaced
        rows' last]); the counters are zero afterwards"""
        nreg = getattr(self, "_nreg", None) or [0] * len(self.nrows)
        uq = np.zeros(len(self.nrows), dtype=np.uint64)
        tot = np.zeros(len(self.nrows), dtype=np.uint64)
        bins = sum(n + 1 for n in nreg)
        ru, rt = np.zeros(bins, dtype=np.uint64), np.zeros(bins, dtype=np.uint64)
        self._ctx._ck(lib.sk_covacc_finish_target_regions(self._h, uq.ctypes.data, tot.ctypes.data, ru.ctypes.data, rt.ctypes.data))
        per, at = [], 0
        for n in nreg:
            per.append((ru[at: at + n + 1].copy(), rt[at: at + n + 1].copy()))
            at += n + 1
        return uq, tot, per

    def set_spectrum(self, max_depth):
        """sk_covacc_set_spectrum: 0 turns the depth spectrum off, 1..SK_COVACC_SPECTRUM_MAX on with that maximum depth"""
        self._ctx._ck(lib.sk_covacc_set_spectrum(self._h, int(max_depth)))
        self._spec_d = int(max_depth)

    def finish_target_spectrum(self, regions=False):
        """sk_covacc_finish_target_spectrum: (unique[nmembers], total[nmembers], spec[nmembers, D + 1], deep[nmembers][, per region as
        finish_target_regions has it]) from one sweep: spec[m, d - 1] rows of member m with count d <= D, spec[m, D] those above D,
        deep[m] the sum of the counts above D; the counters are zero afterwards"""
        nm, nb = len(self.nrows), getattr(self, "_spec_d", 0) + 1
        uq, tot, deep = (np.zeros(nm, dtype=np.uint64) for _ in range(3))
        spec = np.zeros((nm, nb), dtype=np.uint64)
        nreg = getattr(self, "_nreg", None) or [0] * nm
        bins = sum(n + 1 for n in nreg)
        ru, rt = np.zeros(bins, dtype=np.uint64), np.zeros(bins, dtype=np.uint64)
        self._ctx._ck(lib.sk_covacc_finish_target_spectrum(self._h, uq.ctypes.data, tot.ctypes.data, spec.ctypes.data, deep.ctypes.data,
                                                           ru.ctypes.data if regions else None, rt.ctypes.data if regions else None))
        if not regions:
            return uq, tot, spec, deep
        per, at = [], 0
        for n in nreg:
            per.append((ru[at: at + n + 1].copy(), rt[at: at + n + 1].copy()))
            at += n + 1
        return uq, tot, spec, deep, per

    def set_support(self, on=True):
        """sk_covacc_set_support: from here on every add() also counts the read pairs behind the numbers (off after create)"""
        self._ctx._ck(lib.sk_covacc_set_support(self._h, int(bool(on))))

    def finish_target_support(self):
        """sk_covacc_finish_target_support: (supporting_pairs[nmembers], lines[nmembers], both_mates[nmembers],
        shared_pairs[nmembers, nmembers], lines_a[nmembers, nmembers]) of the folds since the last call, as uint64 arrays; the diagonal
        of the two matrices holds the exclusive pairs and their lines; everything is zero afterwards.  SKError (SK_E_STATE) while
        support is off."""
        nm = len(self.nrows)
        pairs, lines, both = (np.zeros(nm, dtype=np.uint64) for _ in range(3))
        shared, lines_a = np.zeros((nm, nm), dtype=np.uint64), np.zeros((nm, nm), dtype=np.uint64)
        self._ctx._ck(lib.sk_covacc_finish_target_support(self._h, pairs.ctypes.data, lines.ctypes.data, both.ctypes.data,
                                                          shared.ctypes.data, lines_a.ctypes.data))
        return pairs, lines, both, shared, lines_a

    def timing(self, on=True):
        """sk_covacc_timing_: start the device clocks (on) and return (ms in folds, ms in sweeps) so far"""
        f, w = C.c_double(0), C.c_double(0)
        self._ctx._ck(lib.sk_covacc_timing_(self._h, int(bool(on)), C.byref(f), C.byref(w)))
        return f.value, w.value

    def support_timing(self):
        """sk_covacc_support_timing_: (ms in the takes inside the folds, ms in finish_target_support), kept while timing() is on"""
        t, f = C.c_double(0), C.c_double(0)
        self._ctx._ck(lib.sk_covacc_support_timing_(self._h, C.byref(t), C.byref(f)))
        return t.value, f.value

    def set_recurrence(self, member, ctx, type_col=0, informative_value=2):
        """sk_covacc_set_recurrence: rank member's informative rows (those whose counter in type_col of ctx's table equals
        informative_value); returns their number, the member's bits in a Recurrence"""
        n = C.c_uint32(0)
        self._ctx._ck(lib.sk_covacc_set_recurrence(self._h, member, ctx._h, type_col, informative_value, C.byref(n)))
        return int(n.value)

    def mark_target(self, recur, sample):
        """sk_covacc_mark_target: every row with a non-zero counter sets its bit of plane sample of recur; the counters stay.  Returns
        the non-zero rows that have no rank (they mark nothing)"""
        stray = C.c_uint64(0)
        self._ctx._ck(lib.sk_covacc_mark_target(self._h, recur._h, int(sample), C.byref(stray)))
        return int(stray.value)

    def close(self):
        if getattr(self, "_h", None):
            lib.sk_covacc_destroy(self._h)
            self._h = None

    def __del__(self):
        self.close()

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()


class Recurrence:
    """The recurrence engine (sk_recur_*): bit planes of len(nbits) members over nsamples samples on ctx's device, and the two tables
    over them -- per member how many bits are set in exactly m planes, and how many bits two planes share."""

    def __init__(self, ctx: KmerContext, nbits, nsamples):
        self._ctx = ctx
        self.nbits = np.ascontiguousarray(nbits, dtype=np.uint32).reshape(-1)
        self.nsamples = int(nsamples)
        self._h = C.c_void_p()
        ctx._ck(lib.sk_recur_create(ctx._h, len(self.nbits), self.nbits.ctypes.data, self.nsamples, C.byref(self._h)))

    def mark_bits(self, member, sample, bits):
        """sk_recur_mark_bits: OR these bits of member into plane sample"""
        bits = np.ascontiguousarray(bits, dtype=np.uint32).reshape(-1)
        self._ctx._ck(lib.sk_recur_mark_bits(self._h, int(member), int(sample), bits.ctypes.data, len(bits)))

    def finish(self, pairs=False):
        """sk_recur_finish: hist[nmembers, nsamples + 1] (column 0: the member's bits set in no plane) and, with pairs,
        shared[nmembers, nsamples, nsamples]; the planes are only read"""
        nm, T = len(self.nbits), self.nsamples
        hist = np.zeros((nm, T + 1), dtype=np.uint64)
        pr = np.zeros((nm, T, T), dtype=np.uint64) if pairs else None
        self._ctx._ck(lib.sk_recur_finish(self._h, hist.ctypes.data, pr.ctypes.data if pairs else None))
        return (hist, pr) if pairs else hist

    def close(self):
        if getattr(self, "_h", None):
            lib.sk_recur_destroy(self._h)
            self._h = None

    def __del__(self):
        self.close()

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()


def pack_stream(stream, out=None):
    """the host-side 2-bit pre-pack (sk_pack_stream): returns (packed bytes as a uint8 array -- code words, then masks --, odd)"""
    buf = np.frombuffer(stream, dtype=np.uint8) if isinstance(stream, (bytes, bytearray)) else np.ascontiguousarray(stream, dtype=np.uint8)
    n = int(lib.sk_packed_bytes(buf.size))
    if out is None:
        out = np.empty(max(n, 1), dtype=np.uint8)
    odd = C.c_int(0)
    rc = lib.sk_pack_stream(buf.ctypes.data, buf.size, out.ctypes.data, C.byref(odd))
    if rc:
        raise SKError(rc)
    return out[:n], bool(odd.value)


class ScrubFilter:
    """Device side of the scrub filter (sk_filter_*): count columns resident on the GPU."""

    def __init__(self, ctx: KmerContext):
        self._ctx = ctx
        self._h = C.c_void_p()
        ctx._ck(lib.sk_filter_create(ctx._h, C.byref(self._h)))
        self.n = 0

    def load(self, pan, meta, gone=None):
        pan = np.ascontiguousarray(pan, dtype=np.int64)
        meta = np.ascontiguousarray(meta, dtype=np.int64)
        assert len(pan) == len(meta)
        g = None if gone is None else np.ascontiguousarray(gone, dtype=np.uint8)
        self._ctx._ck(lib.sk_filter_load(self._h, pan.ctypes.data, meta.ctypes.data, None if g is None else g.ctypes.data, len(pan)))
        self.n = len(pan)

    def load_counts(self, pan_col=1, meta_col=2, drug_col=-1):
        self._ctx._ck(lib.sk_filter_load_counts(self._h, pan_col, meta_col, drug_col))
        self.n = lib.sk_table_rows(self._ctx._h)

    def sums(self):
        v = [C.c_int64(), C.c_int64(), C.c_uint64(), C.c_uint64(), C.c_uint64()]
        self._ctx._ck(lib.sk_filter_sums(self._h, *[C.byref(x) for x in v]))
        return tuple(int(x.value) for x in v)

    def hist(self, which, lo, nbins):
        out = np.zeros(nbins + 1, dtype=np.uint64)
        self._ctx._ck(lib.sk_filter_hist(self._h, which, lo, nbins, out.ctypes.data))
        return out

    def joint(self, pan_sum, meta_sum, n_scrub):
        out = np.zeros(self.n, dtype=np.uint8)
        self._ctx._ck(lib.sk_filter_joint(self._h, pan_sum, meta_sum, n_scrub, out.ctypes.data))
        return out

    def above(self, pan_thr, meta_thr):
        out = np.zeros(self.n, dtype=np.uint8)
        self._ctx._ck(lib.sk_filter_above(self._h, pan_thr, meta_thr, out.ctypes.data))
        return out

    def classes_joint(self, pan_sum, meta_sum, n_scrub):
        """sk_filter_classes_joint: (class[n] bytes, kept[F]) for the non-decreasing list n_scrub of joint scrubs"""
        ns = np.ascontiguousarray(n_scrub, dtype=np.uint64).reshape(-1)
        out = np.zeros(max(self.n, 1), dtype=np.uint8)
        kept = np.zeros(max(len(ns), 1), dtype=np.uint64)
        self._ctx._ck(lib.sk_filter_classes_joint(self._h, pan_sum, meta_sum, ns.ctypes.data, len(ns), out.ctypes.data, kept.ctypes.data))
        return out[: self.n], kept[: len(ns)]

    def classes_above(self, pan_thr, meta_thr):
        """sk_filter_classes_above: (class[n] bytes, kept[F]) for the non-increasing lists of thresholds"""
        tp = np.ascontiguousarray(pan_thr, dtype=np.int64).reshape(-1)
        tm = np.ascontiguousarray(meta_thr, dtype=np.int64).reshape(-1)
        assert len(tp) == len(tm)
        out = np.zeros(max(self.n, 1), dtype=np.uint8)
        kept = np.zeros(max(len(tp), 1), dtype=np.uint64)
        self._ctx._ck(lib.sk_filter_classes_above(self._h, tp.ctypes.data, tm.ctypes.data, len(tp), out.ctypes.data, kept.ctypes.data))
        return out[: self.n], kept[: len(tp)]

    def close(self):
        if self._h:
            lib.sk_filter_destroy(self._h)
            self._h = None

    def __del__(self):
        self.close()


def decode_file(path, chunk_bytes=1 << 26):
    """Host reader only (no GPU): the record stream the scan would be fed, as a list of chunks."""
    chunks = []

    def sink(_user, ptr, n):
        chunks.append(C.string_at(ptr, n))
        return 0

    bases = C.c_uint64(0)
    nrec = lib.skh_decode_file(os.fsencode(path), chunk_bytes, _SINK(sink), None, C.byref(bases))
    if nrec < 0:
        raise SKError(int(nrec), path)
    return chunks, int(nrec), bases.value


def run_strain_detect_inprocess(argv, stdout_path, stderr_path):
    """Call strain_detect's main() in this process (bin/strain_detect is the same function): what coverage_only_stats() and
    target_cache_stats() count afterwards is that run's."""
    args = [b"strain_detect"] + [os.fsencode(a) for a in argv]
    arr = (C.c_char_p * (len(args) + 1))(*args, None)
    fo = _libc.fopen(os.fsencode(stdout_path), b"w")
    fe = _libc.fopen(os.fsencode(stderr_path), b"w")
    try:
        return lib.skh_strain_detect_main(len(args), arr, fo, fe)
    finally:
        _libc.fclose(fo)
        _libc.fclose(fe)


def run_cli_inprocess(argv, stdout_path, stderr_path):
    """Call the program's main() in this process (the bin/ program is the same function)."""
    args = [b"kmer_scrub_count"] + [os.fsencode(a) for a in argv]
    arr = (C.c_char_p * (len(args) + 1))(*args, None)
    fo = _libc.fopen(os.fsencode(stdout_path), b"w")
    fe = _libc.fopen(os.fsencode(stderr_path), b"w")
    try:
        return lib.skh_kmer_scrub_count_main(len(args), arr, fo, fe)
    finally:
        _libc.fclose(fo)
        _libc.fclose(fe)
