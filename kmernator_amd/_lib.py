"""ctypes binding of the C-ABI in include/kmernator_amd.h.

The shared library is built in-tree (kmernator_amd/csrc/libkmernator_amd.so) by
__graft_entry__.build() / `make -C kmernator_amd/csrc`.  There is no fallback: if the
library is missing, load() raises.
"""
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "csrc", "libkmernator_amd.so")

KMR_VALUE_COUNT_DIR, KMR_VALUE_EXT = 0, 1
KMR_MAP_WEAK, KMR_MAP_SINGLETON, KMR_MAP_SOLID = 0, 1, 2

STATUS = {0: "KMR_OK", -1: "KMR_ERR_INVALID_ARG", -2: "KMR_ERR_NO_DEVICE", -3: "KMR_ERR_HIP", -4: "KMR_ERR_OOM",
          -5: "KMR_ERR_STATE", -6: "KMR_ERR_CAPACITY", -7: "KMR_ERR_UNSUPPORTED"}


class KmrConfig(C.Structure):
    """kmr_config"""
    _fields_ = [
        ("struct_size", C.c_uint32), ("k", C.c_uint32),
        ("num_buckets_weak", C.c_uint64), ("num_buckets_singleton", C.c_uint64),
        ("estimated_raw_kmers", C.c_uint64),
        ("value_kind", C.c_uint32), ("min_weight", C.c_float),
        ("min_quality_score", C.c_uint32), ("fastq_start_char", C.c_uint32),
        ("ext_min_quality", C.c_uint32), ("separate_singletons", C.c_uint32),
        ("kmer_subsample", C.c_uint32), ("device", C.c_int32),
        ("rank", C.c_uint32), ("world_size", C.c_uint32),
        ("estimated_depth", C.c_double), ("estimated_error_rate", C.c_double),
        ("kmers_per_bucket", C.c_uint32), ("num_parts", C.c_uint32),
        ("part_idx", C.c_uint32), ("build_mode", C.c_uint32),
        ("max_table_entries", C.c_uint64),
        ("hash_kind", C.c_uint32), ("size_tracker", C.c_uint32),
    ]


class KmrStats(C.Structure):
    """kmr_stats"""
    _fields_ = [(n, C.c_uint64) for n in (
        "raw_kmers", "raw_good_kmers", "unique_kmers", "singleton_kmers",
        "discarded", "weak_entries", "singleton_entries", "reads")]

    def as_dict(self):
        return {n: int(getattr(self, n)) for n, _ in self._fields_}


class KmrDigest(C.Structure):
    """kmr_digest"""
    _fields_ = [(n, C.c_uint64) for n in ("entries", "count_sum", "dir_sum", "hash_sum", "hash_xor")] + [("weighted_sum", C.c_double)]

    def as_dict(self):
        return {n: getattr(self, n) for n, _ in self._fields_}


class KmrArtifactConfig(C.Structure):
    """kmr_artifact_config"""
    _fields_ = [(n, C.c_uint32) for n in ("match_length", "edit_distance", "build_edits", "simple_repeat_begin", "simple_repeat_end",
                                          "phix_idx", "reference_begin", "min_quality", "fastq_start_char")] + [("min_read_length", C.c_float)]


class KmrArtifactReportConfig(C.Structure):
    """kmr_artifact_report_config"""
    _fields_ = [(n, C.c_uint32) for n in ("struct_size", "artifact_output", "phix_output", "output_quality_base", "print_bases")]


class KmrDedupConfig(C.Structure):
    """kmr_dedup_config"""
    _fields_ = [(n, C.c_uint32) for n in ("struct_size", "dedup_mode", "paired", "dedup_length", "start_offset", "edit_distance", "consensus")]


class KmrCompareCounts(C.Structure):
    """kmr_compare_counts"""
    _fields_ = [(n, C.c_uint64) for n in ("size1", "size2", "common", "common_count1", "common_count2", "total_count1", "total_count2", "saturated")]

    def as_dict(self):
        return {n: int(getattr(self, n)) for n, _ in self._fields_}


class KmrMatchConfig(C.Structure):
    """kmr_match_config"""
    _fields_ = [("struct_size", C.c_uint32), ("max_positions_from_edge", C.c_int32), ("max_read_matches", C.c_uint32), ("include_mate", C.c_uint32), ("seed", C.c_uint64)]


class KmrExtendConfig(C.Structure):
    """kmr_extend_config"""
    _fields_ = [("struct_size", C.c_uint32), ("max_extend", C.c_uint32), ("minimum_consensus", C.c_double), ("minimum_coverage", C.c_double),
                ("maximum_delta_ratio", C.c_double), ("use_weights", C.c_uint32), ("reserved", C.c_uint32)]


class KmrExtendStop(C.Structure):
    """kmr_extend_stop"""
    _fields_ = [("reason", C.c_uint32), ("reserved", C.c_uint32), ("edge", C.c_double), ("ext", C.c_double * 4), ("total", C.c_double)]


# kmr_extend_stop_reason
KMR_EXTEND_STOP_LIMIT, KMR_EXTEND_STOP_SHORT, KMR_EXTEND_STOP_NO_EDGE, KMR_EXTEND_STOP_COVERAGE, KMR_EXTEND_STOP_AMBIGUOUS, KMR_EXTEND_STOP_REPEAT, KMR_EXTEND_STOP_INACTIVE = range(7)
KMR_EXTEND_MAX_EXTEND = 65536

KMR_TNF_EUCLIDEAN, KMR_TNF_SPEARMAN = 0, 1


class KmrTnfLikelihoodConfig(C.Structure):
    """kmr_tnf_likelihood_config"""
    _fields_ = [("struct_size", C.c_uint32), ("formula", C.c_uint32), ("window", C.c_uint64), ("step", C.c_uint64), ("window2", C.c_uint64), ("step2", C.c_uint64),
                ("bins", C.c_uint32), ("reserved", C.c_uint32), ("max_samples", C.c_int64)]


class KmrSelectConfig(C.Structure):
    """kmr_select_config"""
    _fields_ = [("struct_size", C.c_uint32), ("both_pass", C.c_uint32), ("minimum_score", C.c_double), ("min_read_length", C.c_float),
                ("output_quality_base", C.c_uint32), ("format", C.c_uint32), ("scoring_type", C.c_uint32)]


class KmrPartitionConfig(C.Structure):
    """kmr_partition_config"""
    _fields_ = [("struct_size", C.c_uint32), ("select", KmrSelectConfig), ("partition_by_depth", C.c_uint32), ("remainder_trim", C.c_float)]


class KmrNormalizeConfig(C.Structure):
    """kmr_normalize_config"""
    _fields_ = [("struct_size", C.c_uint32), ("select", KmrSelectConfig), ("target_depth", C.c_uint64), ("seed", C.c_uint64), ("first_global_read_idx", C.c_uint64),
                ("by_pair", C.c_uint32), ("method", C.c_uint32), ("use_logscale", C.c_uint32)]


# every symbol include/kmernator_amd.h declares
EXPORTS = [
    "kmr_abi_version", "kmr_config_init", "kmr_create", "kmr_destroy", "kmr_last_error", "kmr_num_buckets",
    "kmr_add_reads", "kmr_add_reads_dev", "kmr_add_reads_twobit", "kmr_add_reads_twobit_dev", "kmr_sync", "kmr_finalize", "kmr_get_stats", "kmr_lookup",
    "kmr_lookup_reads", "kmr_image_size", "kmr_write_image", "kmr_load_image", "kmr_count_histogram",
    "kmr_dump_mercount", "kmr_dump_mergraph", "kmr_hash", "kmr_hash_of_kind", "kmr_bucket_idx", "kmr_local_thread_id",
    "kmr_distributed_thread_id", "kmr_compress_sequence", "kmr_least_complement", "kmr_extract_by_owner_dev",
    "kmr_insert_records_dev", "kmr_stream", "kmr_kernel_time", "kmr_kernel_time_reset", "kmr_reset", "kmr_release_table", "kmr_score_reads",
    "kmr_ingest_fastq", "kmr_ingest_fastq_dev", "kmr_ingest_fasta", "kmr_ingest_fasta_dev", "kmr_reads_info", "kmr_reads_device_ptrs", "kmr_reads_copy",
    "kmr_add_read_batch", "kmr_reads_free", "kmr_histogram", "kmr_histogram_bins", "kmr_merge_image", "kmr_subtract_reference", "kmr_subtracted", "kmr_score_read_batch",
    "kmr_artifact_config_init", "kmr_artifact_filter_create", "kmr_artifact_filter_info", "kmr_artifact_filter_entries",
    "kmr_artifact_filter_free", "kmr_artifact_filter_apply", "kmr_artifact_filter_name",
    "kmr_artifact_report_config_init", "kmr_artifact_filter_report", "kmr_artifact_filter_report_dev", "kmr_artifact_filter_apply_report", "kmr_artifact_filter_apply_report_dev",
    "kmr_artifact_report_counts", "kmr_artifact_report_picks", "kmr_artifact_report_free",
    "kmr_tune", "kmr_set_stream_origin", "kmr_size_tracker", "kmr_exchange_unique_id", "kmr_exchange_init", "kmr_exchange_init_transport", "kmr_exchange_add_reads_dev", "kmr_exchange_add_read_batch", "kmr_exchange_stats", "kmr_copy_to_host", "kmr_copy_to_device", "kmr_sk_exchange_begin", "kmr_sk_exchange_counts", "kmr_sk_exchange_pack_dev", "kmr_sk_exchange_adopt_dev", "kmr_extract_by_owner_host", "kmr_insert_records", "kmr_reads_from_host", "kmr_reads_from_twobit", "kmr_reads_twobit", "kmr_lookup_requests_dev", "kmr_lookup_keys_dev", "kmr_scatter_counts_dev", "kmr_score_counts_dev",
    "kmr_lookup_weighted", "kmr_lookup_reads_weighted", "kmr_lookup_keys_weighted_dev",
    "kmr_select_config_init", "kmr_select_reads", "kmr_select_reads_dev", "kmr_filter_read_batch", "kmr_filter_read_batch_dev",
    "kmr_picks_info", "kmr_picks_copy", "kmr_picks_device_ptr", "kmr_picks_free",
    "kmr_partition_config_init", "kmr_partition_rounds", "kmr_partition_reads", "kmr_partition_reads_dev", "kmr_partition_read_batch", "kmr_partition_read_batch_dev",
    "kmr_picks_segments_info", "kmr_picks_segments_copy",
    "kmr_normalize_config_init", "kmr_normalize_reads", "kmr_normalize_reads_dev", "kmr_normalize_read_batch", "kmr_normalize_read_batch_dev", "kmr_normalize_info",
    "kmr_set_bimodal_sigmas", "kmr_bimodal_copy", "kmr_select_bimodal",
    "kmr_dump_text_size", "kmr_dump_text", "kmr_text_info", "kmr_text_copy", "kmr_text_device_ptr", "kmr_text_free",
    "kmr_identify_pairs", "kmr_identify_pairs_dev", "kmr_pairs_info", "kmr_pairs_copy", "kmr_pairs_device_ptrs", "kmr_pairs_free",
    "kmr_dedup_config_init", "kmr_dedup_fragments", "kmr_dedup_fragments_dev", "kmr_dedup_info", "kmr_dedup_copy", "kmr_dedup_device_ptrs",
    "kmr_dedup_reads", "kmr_dedup_names_copy", "kmr_dedup_free", "kmr_consensus_qual",
    "kmr_compare_spectrums", "kmr_compare_reads", "kmr_compare_reads_dev", "kmr_compare_line", "kmr_reads_circularize",
    "kmr_tnf_dims", "kmr_tnf_columns", "kmr_tnf_header", "kmr_tnf_reads", "kmr_tnf_windows", "kmr_tnf_group_sums", "kmr_tnf_info", "kmr_tnf_copy", "kmr_tnf_free",
    "kmr_tnf_distances", "kmr_tnf_distances_dev", "kmr_tnf_likelihood_config_init", "kmr_tnf_likelihoods",
    "kmr_match_config_init", "kmr_match_create", "kmr_match_edge_info", "kmr_match_add_read_batch", "kmr_match_finish", "kmr_match_info", "kmr_match_copy",
    "kmr_match_device_ptrs", "kmr_match_free",
    "kmr_extend_config_init", "kmr_extend_contigs", "kmr_extend_contigs_dev", "kmr_extend_info", "kmr_extend_copy", "kmr_extend_reads", "kmr_extend_free",
    "kmr_extend_new_name", "kmr_extend_min_max_kmer_size",
    "kmr_map_digest", "kmr_synth_reads_dev", "kmr_build_info", "kmr_sk_exchange_uniform", "kmr_sk_exchange_peer_uniform", "kmr_sk_exchange_range", "kmr_count_lists_prefix",
]

_lib = None


def load():
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError("%s is missing: run `python -c 'import __graft_entry__ as g; g.build()'` "
                           "(there is no CPU fallback)" % LIB_PATH)
    lib = C.CDLL(LIB_PATH)
    vp, u8p, u32p, u64p, f64p = C.c_void_p, C.POINTER(C.c_uint8), C.POINTER(C.c_uint32), C.POINTER(C.c_uint64), C.POINTER(C.c_double)
    lib.kmr_abi_version.restype = C.c_uint32
    lib.kmr_config_init.argtypes = [C.POINTER(KmrConfig)]
    lib.kmr_create.argtypes = [C.POINTER(KmrConfig), C.POINTER(vp)]
    lib.kmr_destroy.argtypes = [vp]
    lib.kmr_destroy.restype = None
    lib.kmr_last_error.argtypes = [vp]
    lib.kmr_last_error.restype = C.c_char_p
    lib.kmr_num_buckets.argtypes = [vp, C.c_int, u64p]
    lib.kmr_add_reads.argtypes = [vp, vp, vp, u64p, C.c_uint64, C.c_uint64, u8p]
    lib.kmr_add_reads_dev.argtypes = [vp, vp, vp, vp, C.c_uint64, C.c_uint64, C.c_uint64, vp]
    lib.kmr_reads_from_twobit.argtypes = [vp, vp, vp, vp, vp, vp, vp, vp, C.c_int, C.c_uint64, C.POINTER(vp)]
    lib.kmr_add_reads_twobit.argtypes = [vp, vp, vp, vp, vp, vp, vp, vp, C.c_int, C.c_uint64, C.c_uint64, vp]
    lib.kmr_add_reads_twobit_dev.argtypes = [vp, vp, vp, vp, vp, vp, vp, vp, C.c_int, C.c_uint64, C.c_uint64, C.c_uint64, vp]
    lib.kmr_sync.argtypes = [vp]
    lib.kmr_finalize.argtypes = [vp, C.c_uint32]
    lib.kmr_get_stats.argtypes = [vp, C.POINTER(KmrStats)]
    lib.kmr_lookup.argtypes = [vp, u8p, C.c_uint64, u32p]
    lib.kmr_lookup_reads.argtypes = [vp, vp, u64p, C.c_uint64, u32p, u64p]
    lib.kmr_lookup_weighted.argtypes = [vp, u8p, C.c_uint64, f64p]
    lib.kmr_lookup_reads_weighted.argtypes = [vp, vp, u64p, C.c_uint64, f64p, u64p]
    lib.kmr_image_size.argtypes = [vp, C.c_int, u64p]
    lib.kmr_write_image.argtypes = [vp, C.c_int, vp, C.c_uint64]
    lib.kmr_load_image.argtypes = [vp, C.c_int, vp, C.c_uint64]
    lib.kmr_count_histogram.argtypes = [vp, u64p, f64p, C.c_uint32]
    lib.kmr_dump_mercount.argtypes = [vp, C.c_char_p, C.c_uint32]
    lib.kmr_dump_mergraph.argtypes = [vp, C.c_char_p, C.c_uint32]
    lib.kmr_hash.restype = C.c_uint64
    lib.kmr_hash.argtypes = [C.c_char_p, C.c_uint32]
    lib.kmr_bucket_idx.restype = C.c_uint64
    lib.kmr_bucket_idx.argtypes = [C.c_uint64, C.c_uint64]
    lib.kmr_local_thread_id.restype = C.c_uint32
    lib.kmr_local_thread_id.argtypes = [C.c_uint64, C.c_uint64, C.c_uint32]
    lib.kmr_distributed_thread_id.restype = C.c_uint32
    lib.kmr_distributed_thread_id.argtypes = [C.c_uint64, C.c_uint32]
    lib.kmr_compress_sequence.restype = C.c_int64
    lib.kmr_compress_sequence.argtypes = [C.c_char_p, C.c_uint64, u8p, u32p, C.c_char_p, C.c_uint64]
    lib.kmr_least_complement.argtypes = [u8p, C.c_uint32, u8p]
    lib.kmr_extract_by_owner_dev.argtypes = [vp, vp, vp, vp, C.c_uint64, C.c_uint64, C.c_uint64, vp, vp, C.c_uint64, vp]
    lib.kmr_insert_records_dev.argtypes = [vp, vp, C.c_uint64]
    lib.kmr_stream.restype = vp
    lib.kmr_stream.argtypes = [vp]
    lib.kmr_kernel_time.argtypes = [vp, C.c_int, f64p, u64p]
    lib.kmr_kernel_time_reset.argtypes = [vp]
    lib.kmr_score_reads.argtypes = [vp, vp, u64p, C.c_uint64, C.c_double, C.c_int, u32p, u32p, C.POINTER(C.c_float), u8p]
    lib.kmr_reset.argtypes = [vp]
    lib.kmr_release_table.argtypes = [vp]
    lib.kmr_ingest_fastq.argtypes = [vp, vp, C.c_uint64, C.c_uint32, C.c_int, C.POINTER(vp)]
    lib.kmr_ingest_fastq_dev.argtypes = [vp, vp, C.c_uint64, C.c_uint32, C.c_int, C.POINTER(vp)]
    lib.kmr_ingest_fasta.argtypes = [vp, vp, C.c_uint64, vp, C.c_uint64, C.c_int, C.POINTER(vp)]
    lib.kmr_ingest_fasta_dev.argtypes = [vp, vp, C.c_uint64, vp, C.c_uint64, C.c_int, C.POINTER(vp)]
    lib.kmr_reads_info.argtypes = [vp, u64p, u64p, u32p, u64p]
    lib.kmr_reads_device_ptrs.argtypes = [vp, C.POINTER(vp), C.POINTER(vp), C.POINTER(vp)]
    lib.kmr_reads_copy.argtypes = [vp, vp, vp, u64p, u64p, u32p]
    lib.kmr_add_read_batch.argtypes = [vp, vp, C.c_uint64]
    lib.kmr_reads_free.argtypes = [vp]
    lib.kmr_reads_free.restype = None
    lib.kmr_score_read_batch.argtypes = [vp, vp, C.c_double, C.c_int, u32p, u32p, C.POINTER(C.c_float), u8p]
    lib.kmr_reads_twobit.argtypes = [vp, vp, vp, C.c_uint64, C.POINTER(C.c_uint64), u32p, vp, C.c_uint64, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
    lib.kmr_reads_from_host.argtypes = [vp, vp, vp, C.POINTER(C.c_uint64), C.c_uint64, C.POINTER(vp)]
    lib.kmr_lookup_requests_dev.argtypes = [vp, vp, vp, C.c_uint64, C.c_uint64, vp, vp, C.c_uint64, vp]
    lib.kmr_lookup_keys_dev.argtypes = [vp, vp, C.c_uint64, vp]
    lib.kmr_lookup_keys_weighted_dev.argtypes = [vp, vp, C.c_uint64, vp]
    lib.kmr_scatter_counts_dev.argtypes = [vp, vp, vp, C.c_uint64, vp]
    lib.kmr_score_counts_dev.argtypes = [vp, vp, vp, C.c_uint64, vp, C.c_double, C.c_int, u32p, u32p, C.POINTER(C.c_float), u8p]
    lib.kmr_artifact_config_init.argtypes = [C.POINTER(KmrArtifactConfig)]
    lib.kmr_artifact_config_init.restype = None
    lib.kmr_artifact_filter_create.argtypes = [vp, C.POINTER(KmrArtifactConfig), C.c_char_p, C.c_uint64, C.POINTER(vp)]
    lib.kmr_artifact_filter_info.argtypes = [vp, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.POINTER(C.c_uint32)]
    lib.kmr_artifact_filter_entries.argtypes = [vp, C.POINTER(C.c_uint64), u32p, C.c_uint64]
    lib.kmr_artifact_filter_free.argtypes = [vp]
    lib.kmr_artifact_filter_free.restype = None
    lib.kmr_artifact_filter_apply.argtypes = [vp, vp, vp, C.POINTER(C.c_int64), u32p, u32p, u32p, u8p, u32p, u32p, C.POINTER(vp)]
    lib.kmr_artifact_filter_name.argtypes = [vp, C.c_uint32, C.c_char_p, C.c_uint64]
    rcp, i64 = C.POINTER(KmrArtifactReportConfig), C.POINTER(C.c_int64)
    lib.kmr_artifact_report_config_init.argtypes = [rcp]
    for name in ("kmr_artifact_filter_report", "kmr_artifact_filter_report_dev"):
        getattr(lib, name).argtypes = [vp, vp, vp, vp, C.c_uint64, i64, i64, C.c_uint64, u32p, u8p, u32p, u32p, u64p, C.c_uint32, rcp, C.POINTER(vp)]
    for name in ("kmr_artifact_filter_apply_report", "kmr_artifact_filter_apply_report_dev"):
        getattr(lib, name).argtypes = [vp, vp, vp, vp, C.c_uint64, i64, i64, C.c_uint64, u32p, u32p, u32p, u8p, u32p, u32p, C.POINTER(vp), u64p, C.c_uint32, rcp, C.POINTER(vp)]
    lib.kmr_artifact_report_counts.argtypes = [vp, u64p, u64p, u64p, C.c_uint64]
    lib.kmr_artifact_report_picks.argtypes = [vp, C.POINTER(vp)]
    lib.kmr_artifact_report_free.argtypes = [vp]
    lib.kmr_artifact_report_free.restype = None
    lib.kmr_extract_by_owner_host.argtypes = [vp, vp, C.c_uint64, u64p, vp, C.c_uint64]
    lib.kmr_insert_records.argtypes = [vp, vp, C.c_uint64]
    lib.kmr_sk_exchange_begin.argtypes = [vp]
    lib.kmr_size_tracker.argtypes = [vp, C.c_int, u64p, C.c_uint64, u64p]
    lib.kmr_exchange_unique_id.argtypes = [vp]
    lib.kmr_exchange_init.argtypes = [vp, vp]
    lib.kmr_exchange_init_transport.argtypes = [vp, vp]
    lib.kmr_exchange_add_reads_dev.argtypes = [vp, vp, vp, vp, C.c_uint64, C.c_uint64, C.c_uint64, vp]
    lib.kmr_exchange_add_read_batch.argtypes = [vp, vp, C.c_uint64]
    lib.kmr_exchange_stats.argtypes = [vp, u64p, C.POINTER(C.c_double)]
    lib.kmr_sk_exchange_counts.argtypes = [vp, u64p, u64p]
    lib.kmr_sk_exchange_pack_dev.argtypes = [vp, vp, vp, u64p, u64p]
    lib.kmr_sk_exchange_adopt_dev.argtypes = [vp, vp, vp, C.c_uint64, C.c_uint64]
    lib.kmr_set_stream_origin.argtypes = [vp, C.c_uint64]
    lib.kmr_tune.argtypes = [vp, C.c_char_p, C.c_double]
    lib.kmr_merge_image.argtypes = [vp, C.c_int, vp, C.c_uint64]
    lib.kmr_subtract_reference.argtypes = [vp, vp]
    lib.kmr_subtracted.argtypes = [vp, u64p]
    lib.kmr_histogram_bins.restype = C.c_uint32
    lib.kmr_histogram_bins.argtypes = [C.c_uint32]
    lib.kmr_histogram.argtypes = [vp, C.c_uint32, C.c_double, u64p, u64p, f64p, C.c_uint32]
    lib.kmr_map_digest.argtypes = [vp, C.c_int, C.POINTER(KmrDigest)]
    lib.kmr_build_info.argtypes = [vp, C.c_char_p, f64p]
    lib.kmr_sk_exchange_uniform.argtypes = [vp, u64p]
    lib.kmr_sk_exchange_peer_uniform.argtypes = [vp, C.c_uint64]
    lib.kmr_sk_exchange_range.argtypes = [vp, C.c_uint64, C.c_uint64]
    lib.kmr_count_lists_prefix.argtypes = [vp, C.c_uint32, C.c_uint64]
    lib.kmr_synth_reads_dev.argtypes = [C.c_uint64, C.c_uint64, C.c_uint64, C.c_uint32, C.c_uint64, C.c_uint32, vp, vp, vp]
    i64p, f32p, scp = C.POINTER(C.c_int64), C.POINTER(C.c_float), C.POINTER(KmrSelectConfig)
    lib.kmr_select_config_init.argtypes = [scp]
    for name in ("kmr_select_reads", "kmr_select_reads_dev"):
        getattr(lib, name).argtypes = [vp, vp, vp, C.c_uint64, i64p, u8p, u32p, u32p, u32p, u32p, f32p, u8p, scp, C.POINTER(vp)]
    for name in ("kmr_filter_read_batch", "kmr_filter_read_batch_dev"):
        getattr(lib, name).argtypes = [vp, vp, vp, C.c_uint64, i64p, u8p, u32p, u32p, scp, C.POINTER(vp)]
    pcp = C.POINTER(KmrPartitionConfig)
    lib.kmr_partition_config_init.argtypes = [pcp]
    lib.kmr_partition_rounds.argtypes = [pcp, u32p, f32p, f32p, u32p, u8p]
    for name in ("kmr_partition_reads", "kmr_partition_reads_dev"):
        getattr(lib, name).argtypes = [vp, vp, vp, C.c_uint64, i64p, u8p, u32p, u32p, u32p, u32p, f32p, u8p, u64p, C.c_uint32, pcp, C.POINTER(vp)]
    for name in ("kmr_partition_read_batch", "kmr_partition_read_batch_dev"):
        getattr(lib, name).argtypes = [vp, vp, vp, C.c_uint64, i64p, u8p, u32p, u32p, u64p, C.c_uint32, pcp, C.POINTER(vp)]
    ncp = C.POINTER(KmrNormalizeConfig)
    lib.kmr_normalize_config_init.argtypes = [ncp]
    for name in ("kmr_normalize_reads", "kmr_normalize_reads_dev"):
        getattr(lib, name).argtypes = [vp, vp, vp, C.c_uint64, i64p, i64p, C.c_uint64, u8p, u32p, u32p, u32p, u32p, f32p, u8p, u64p, C.c_uint32, ncp, C.POINTER(vp)]
    for name in ("kmr_normalize_read_batch", "kmr_normalize_read_batch_dev"):
        getattr(lib, name).argtypes = [vp, vp, vp, C.c_uint64, i64p, i64p, C.c_uint64, u8p, u32p, u32p, u64p, C.c_uint32, ncp, C.POINTER(vp)]
    lib.kmr_normalize_info.argtypes = [vp, u64p, u64p, u64p]
    lib.kmr_set_bimodal_sigmas.argtypes = [vp, C.c_double]
    lib.kmr_bimodal_copy.argtypes = [vp, u64p, C.c_uint64]
    lib.kmr_select_bimodal.argtypes = [vp, u64p, C.c_uint64]
    lib.kmr_picks_segments_info.argtypes = [vp, u32p, u32p]
    lib.kmr_picks_segments_copy.argtypes = [vp, f32p, u8p, u64p, u64p, u64p, u64p, C.POINTER(C.c_int32)]
    lib.kmr_picks_info.argtypes = [vp, u64p, u64p]
    lib.kmr_picks_copy.argtypes = [vp, vp, C.c_uint64, u8p]
    lib.kmr_picks_device_ptr.argtypes = [vp, C.POINTER(vp)]
    lib.kmr_picks_free.argtypes = [vp]
    lib.kmr_picks_free.restype = None
    lib.kmr_dump_text_size.argtypes = [vp, C.c_int, C.c_uint32, C.c_uint64, C.c_uint64, u64p, u64p]
    lib.kmr_dump_text.argtypes = [vp, C.c_int, C.c_uint32, C.c_uint64, C.c_uint64, C.POINTER(vp)]
    lib.kmr_text_info.argtypes = [vp, u64p, u64p]
    lib.kmr_text_copy.argtypes = [vp, vp, C.c_uint64]
    lib.kmr_text_device_ptr.argtypes = [vp, C.POINTER(vp)]
    lib.kmr_text_free.argtypes = [vp]
    lib.kmr_text_free.restype = None
    for name in ("kmr_identify_pairs", "kmr_identify_pairs_dev"):
        getattr(lib, name).argtypes = [vp, vp, vp, C.c_uint64, C.c_int, C.POINTER(vp)]
    lib.kmr_pairs_info.argtypes = [vp, u64p, u64p, u64p, u64p, u64p, C.POINTER(C.c_int)]
    lib.kmr_pairs_copy.argtypes = [vp, i64p, i64p, i64p]
    lib.kmr_pairs_device_ptrs.argtypes = [vp, C.POINTER(vp), C.POINTER(vp), C.POINTER(vp)]
    lib.kmr_pairs_free.argtypes = [vp]
    lib.kmr_pairs_free.restype = None
    dcp = C.POINTER(KmrDedupConfig)
    lib.kmr_dedup_config_init.argtypes = [dcp]
    for name in ("kmr_dedup_fragments", "kmr_dedup_fragments_dev"):
        getattr(lib, name).argtypes = [vp, vp, vp, C.c_uint64, vp, u8p, dcp, C.POINTER(vp)]
    lib.kmr_dedup_info.argtypes = [vp, u64p, u64p, u64p, u64p]
    lib.kmr_dedup_copy.argtypes = [vp, u8p, u64p, u32p]
    lib.kmr_dedup_device_ptrs.argtypes = [vp, C.POINTER(vp), C.POINTER(vp), C.POINTER(vp)]
    lib.kmr_dedup_reads.argtypes = [vp, C.POINTER(vp), C.POINTER(vp), u64p]
    lib.kmr_dedup_names_copy.argtypes = [vp, vp, C.c_uint64]
    lib.kmr_dedup_free.argtypes = [vp]
    lib.kmr_dedup_free.restype = None
    lib.kmr_consensus_qual.argtypes = [C.c_double]
    lib.kmr_consensus_qual.restype = C.c_char
    ccp = C.POINTER(KmrCompareCounts)
    lib.kmr_compare_spectrums.argtypes = [vp, vp, ccp]
    lib.kmr_compare_reads.argtypes = [vp, vp, vp]
    lib.kmr_compare_reads_dev.argtypes = [vp, vp, vp]
    lib.kmr_compare_line.argtypes = [ccp, C.c_char_p, C.c_uint64, C.c_char_p, C.c_uint64, u64p]
    lib.kmr_reads_circularize.argtypes = [vp, vp, C.c_uint32, C.POINTER(vp)]
    u16p, lcp = C.POINTER(C.c_uint16), C.POINTER(KmrTnfLikelihoodConfig)
    lib.kmr_tnf_dims.argtypes = [C.c_uint32, u32p]
    lib.kmr_tnf_columns.argtypes = [C.c_uint32, C.c_uint32, u16p]
    lib.kmr_tnf_header.argtypes = [C.c_uint32, C.c_uint32, C.c_char_p, C.c_uint64, u64p]
    lib.kmr_tnf_reads.argtypes = [vp, vp, u64p, C.c_uint32, C.POINTER(vp)]
    lib.kmr_tnf_windows.argtypes = [vp, vp, u64p, C.c_uint32, C.c_uint64, C.c_uint64, C.c_int64, C.POINTER(vp)]
    lib.kmr_tnf_group_sums.argtypes = [vp, vp, C.POINTER(vp)]
    lib.kmr_tnf_info.argtypes = [vp, u64p, u32p, u32p, u64p]
    lib.kmr_tnf_copy.argtypes = [vp, u64p, C.POINTER(C.c_float), u64p, u64p]
    lib.kmr_tnf_free.argtypes = [vp]
    lib.kmr_tnf_free.restype = None
    lib.kmr_tnf_distances.argtypes = [vp, vp, vp, C.c_int, C.c_uint64, C.c_uint64, C.POINTER(C.c_float)]
    lib.kmr_tnf_distances_dev.argtypes = [vp, vp, vp, C.c_int, C.c_uint64, C.c_uint64, vp]
    lib.kmr_tnf_likelihood_config_init.argtypes = [lcp]
    lib.kmr_tnf_likelihoods.argtypes = [vp, vp, u64p, C.c_uint32, lcp, u64p]
    mcp = C.POINTER(KmrMatchConfig)
    lib.kmr_match_config_init.argtypes = [mcp]
    lib.kmr_match_create.argtypes = [vp, vp, mcp, C.POINTER(vp)]
    lib.kmr_match_edge_info.argtypes = [vp, u64p, u64p, u64p, u64p]
    lib.kmr_match_add_read_batch.argtypes = [vp, vp, C.c_uint64, vp, u8p]
    lib.kmr_match_finish.argtypes = [vp]
    lib.kmr_match_info.argtypes = [vp, u64p, u64p, u64p]
    lib.kmr_match_copy.argtypes = [vp, u64p, u64p, u64p, u64p]
    lib.kmr_match_device_ptrs.argtypes = [vp, C.POINTER(vp), C.POINTER(vp), C.POINTER(vp), C.POINTER(vp)]
    lib.kmr_match_free.argtypes = [vp]
    lib.kmr_match_free.restype = None
    ecp = C.POINTER(KmrExtendConfig)
    lib.kmr_extend_config_init.argtypes = [ecp]
    lib.kmr_extend_contigs.argtypes = [vp, vp, vp, u64p, u64p, u8p, ecp, C.POINTER(vp)]
    lib.kmr_extend_contigs_dev.argtypes = [vp, vp, vp, vp, vp, vp, ecp, C.POINTER(vp)]
    lib.kmr_extend_info.argtypes = [vp, u64p, u64p, u64p]
    lib.kmr_extend_copy.argtypes = [vp, u32p, u32p, u32p, C.POINTER(KmrExtendStop)]
    lib.kmr_extend_reads.argtypes = [vp, C.POINTER(vp)]
    lib.kmr_extend_free.argtypes = [vp]
    lib.kmr_extend_free.restype = None
    lib.kmr_extend_new_name.argtypes = [C.c_char_p, C.c_uint64, C.c_uint64, C.c_char_p, C.c_uint64]
    lib.kmr_extend_min_max_kmer_size.argtypes = [C.c_uint32, C.c_uint32, C.c_uint64, C.c_uint64, C.c_uint32, u32p, u32p, u32p]
    _lib = lib
    return lib


def default_config(k, **kw):
    c = KmrConfig()
    load().kmr_config_init(C.byref(c))
    c.k = k
    for name, v in kw.items():
        setattr(c, name, v)
    return c


def record_bytes(k, value_kind=KMR_VALUE_COUNT_DIR):
    """KMR_RECORD_BYTES(k, value_kind)"""
    return 8 * ((((k + 3) // 4) + 7) // 8) + (8 if value_kind == KMR_VALUE_EXT else 4)
