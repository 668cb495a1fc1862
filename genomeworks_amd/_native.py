"""ctypes bindings of the two native libraries. Fails loudly when they are missing: there is no CPU fallback."""
import ctypes as C
import os

PKG = os.path.dirname(os.path.abspath(__file__))
LIBDIR = os.path.join(PKG, "lib")


class NativeLibraryMissing(ImportError):
    pass


class PoaConfig(C.Structure):
    """gwhip_poa_config (include/gwhip.h)"""
    _fields_ = [(n, C.c_int32) for n in (
        "max_sequence_size", "max_consensus_size", "max_nodes_per_graph", "matrix_sequence_dimension",
        "alignment_band_width", "max_sequences_per_poa", "band_mode", "max_banded_pred_distance",
        "gap_score", "mismatch_score", "match_score", "output_mask", "score32", "size32", "trace16", "spoa_accurate")]


class WindowDetails(C.Structure):
    """gwhip_window_details == WindowDetails (cudapoa_structs.cuh:70-87)"""
    _fields_ = [("num_seqs", C.c_uint16), ("seq_len_buffer_offset", C.c_int32), ("seq_starts", C.c_int32),
                ("scores_offset", C.c_uint64), ("scores_width", C.c_int32)]


class PoaArgs(C.Structure):
    _fields_ = [("cfg", PoaConfig), ("total_windows", C.c_int32), ("sequences", C.c_void_p),
                ("base_weights", C.c_void_p), ("sequence_lengths", C.c_void_p), ("window_details", C.c_void_p),
                ("consensus", C.c_void_p), ("coverage", C.c_void_p), ("msa", C.c_void_p), ("workspace", C.c_void_p),
                ("workspace_bytes", C.c_size_t), ("cells", C.c_void_p), ("event_after_graph_build", C.c_void_p), ("phase_cycles", C.c_void_p), ("work_counters", C.c_void_p), ("shared_device", C.c_int32)]


class MyersArgs(C.Structure):
    _fields_ = [("n_alignments", C.c_int32), ("sequences", C.c_void_p), ("sequence_starts", C.c_void_p),
                ("max_bandwidths", C.c_void_p), ("results", C.c_void_p), ("result_counts", C.c_void_p),
                ("result_starts", C.c_void_p), ("result_metadata", C.c_void_p), ("results_capacity", C.c_int64),
                ("workspace", C.c_void_p), ("workspace_bytes", C.c_size_t), ("total_sequence_length", C.c_int64),
                ("scheduling_index", C.c_void_p), ("band_cells", C.c_void_p), ("run_counts_out", C.c_void_p),
                ("max_query_length", C.c_int32), ("max_bandwidth_hint", C.c_int32),
                # chunked batches (include/gwhip.h); all zero = one call for the whole batch
                ("index_base", C.c_int32), ("first_sequence_offset", C.c_int64), ("result_starts_base", C.c_void_p),
                # pipelined chunks: second stream, phases of the call, pinned host mirrors of the results; all zero = none
                ("side_stream", C.c_void_p), ("phases", C.c_int32), ("results_host", C.c_void_p), ("result_counts_host", C.c_void_p),
                ("results_host_capacity", C.c_int64), ("result_starts_host", C.c_void_p), ("result_metadata_host", C.c_void_p)]


class PoaBatchConfig(C.Structure):
    """gw_poa_batch_config (include/gw_capi.h) == cudapoa::BatchConfig fields"""
    _fields_ = [(n, C.c_int32) for n in (
        "max_sequence_size", "max_consensus_size", "max_nodes_per_graph", "matrix_sequence_dimension",
        "alignment_band_width", "max_sequences_per_poa", "band_mode", "max_banded_pred_distance")]


_gwhip = None
_host = None
_extender = None
_mapper = None


def _load(name):
    path = os.path.join(LIBDIR, name)
    if not os.path.exists(path):
        raise NativeLibraryMissing(
            f"{path} not found: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "(hipcc --offload-arch=gfx950). genomeworks_amd has no CPU fallback.")
    return C.CDLL(path, mode=C.RTLD_GLOBAL)


def gwhip():
    """libgwhip.so: HIP kernels behind the thin C-ABI."""
    global _gwhip
    if _gwhip is None:
        L = _load("libgwhip.so")
        L.gwhip_poa_workspace_bytes.restype = C.c_size_t
        L.gwhip_poa_workspace_bytes.argtypes = [C.POINTER(PoaConfig), C.c_int32, C.c_uint64]
        L.gwhip_poa_bytes_per_window.argtypes = [C.POINTER(PoaConfig), C.POINTER(C.c_int64), C.POINTER(C.c_int64)]
        L.gwhip_poa_generate.restype = C.c_int
        L.gwhip_poa_generate.argtypes = [C.POINTER(PoaArgs), C.c_void_p]
        L.gwhip_poa_export_graphs.restype = C.c_int
        L.gwhip_poa_export_graphs.argtypes = [C.POINTER(PoaArgs)] + [C.c_void_p] * 7
        L.gwhip_last_error_string.restype = C.c_int
        L.gwhip_last_error_string.argtypes = [C.c_char_p, C.c_size_t]
        L.gwhip_build_arch.restype = C.c_char_p
        L.gwhip_abi_version.restype = C.c_int
        _gwhip = L
    return _gwhip


def host():
    """libgenomeworks_amd.so: host C++ classes behind the object-level C API."""
    global _host
    if _host is None:
        gwhip()
        L = _load("libgenomeworks_amd.so")
        L.gw_last_error.restype = C.c_char_p
        L.gw_generate_window.restype = C.c_int64
        L.gw_generate_window.argtypes = [C.c_uint32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32,
                                         C.c_void_p, C.c_int64, C.c_void_p]
        L.gw_generate_pairs.restype = C.c_int64
        L.gw_generate_pairs.argtypes = [C.c_uint32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32,
                                        C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]
        _host = L
    return _host


def extender():
    """libcudaextender.so: the cudaextender kernels (include/gwhip_extender.h) and the Extender behind the flat C API
    (include/gw_extender_capi.h)."""
    global _extender
    if _extender is None:
        host()
        L = _load("libcudaextender.so")
        vp, i32, i64 = C.c_void_p, C.c_int32, C.c_int64
        L.gw_extender_last_error.restype = C.c_char_p
        L.gw_extender_create.restype = vp
        L.gw_extender_create.argtypes = [vp, i32, i32, i32, vp, i32, i64, i32]
        L.gw_extender_extend_host.argtypes = [vp, vp, i32, vp, i32, i32, vp, i64]
        L.gw_extender_extend_device.argtypes = [vp, vp, i32, vp, i32, i32, vp, i32, vp, vp]
        L.gw_extender_sync.argtypes = [vp]
        L.gw_extender_result_count.restype = i64
        L.gw_extender_result_count.argtypes = [vp]
        L.gw_extender_copy_results.argtypes = [vp, vp, i64]
        L.gw_extender_reset.restype = None
        L.gw_extender_reset.argtypes = [vp]
        L.gw_extender_destroy.restype = None
        L.gw_extender_destroy.argtypes = [vp]
        L.gw_extender_set_chunk_size.argtypes = [vp, i32]
        L.gw_extender_set_instrumentation.argtypes = [vp, i32]
        L.gw_extender_last_timing.argtypes = [vp, C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(i64)]
        L.gw_extender_sort_unique_hook.argtypes = [vp, vp, i32, vp, C.POINTER(i32), vp]
        L.gwx_workspace_bytes.restype = C.c_size_t
        L.gwx_workspace_bytes.argtypes = [i32]
        L.gwx_last_error.restype = C.c_char_p
        _extender = L
    return _extender


_poa_hooks = None


def poa_hooks():
    """libgwhip_poa_hooks.so: test-only hook of the production POA merge (include/gwhip_poa_hooks.h)."""
    global _poa_hooks
    if _poa_hooks is None:
        L = _load("libgwhip_poa_hooks.so")
        vp, i32 = C.c_void_p, C.c_int32
        L.gwhip_poa_test_add_alignment_parallel_scratch_bytes.restype = C.c_size_t
        L.gwhip_poa_test_add_alignment_parallel_scratch_bytes.argtypes = [i32, i32, i32]
        L.gwhip_poa_test_add_alignment_parallel.argtypes = [vp] * 9 + [i32] + [vp] * 5 + [i32, i32, i32, vp, vp, vp]
        _poa_hooks = L
    return _poa_hooks


def gwhip_error():
    buf = C.create_string_buffer(512)
    gwhip().gwhip_last_error_string(buf, 512)
    return buf.value.decode(errors="replace")


GWHIP_SYMBOLS = [
    "gwhip_poa_workspace_bytes", "gwhip_poa_bytes_per_window", "gwhip_poa_generate", "gwhip_poa_export_graphs",
    "gwhip_last_error_string", "gwhip_build_arch", "gwhip_abi_version",
]


def mapper():
    """libcudamapper.so: the cudamapper kernels (include/gwhip_mapper.h) and the Index / Matcher handles behind the flat
    C API (include/gw_mapper_capi.h)."""
    global _mapper
    if _mapper is None:
        vp, i32, i64, f32 = C.c_void_p, C.c_int32, C.c_int64, C.c_float
        gwhip()  # libcudamapper.so links it for the aligner behind gwm_align_overlaps
        L = _load("libcudamapper.so")
        L.gw_mapper_last_error.restype = C.c_char_p
        L.gw_mapper_index_create.restype = vp
        L.gw_mapper_index_create.argtypes = [vp, vp, i32, C.c_uint32, i32, i32, i32, C.c_double, vp]
        L.gw_mapper_index_destroy.restype = None
        L.gw_mapper_index_destroy.argtypes = [vp]
        L.gw_mapper_index_info.argtypes = [vp, vp, vp, vp]
        L.gw_mapper_index_copy.argtypes = [vp] * 7
        L.gw_mapper_index_from_arrays.restype = vp
        L.gw_mapper_index_from_arrays.argtypes = [i64, vp, vp, i64, vp, vp, C.c_uint32, C.c_uint32, C.c_uint32]
        L.gw_mapper_matcher_create.restype = vp
        L.gw_mapper_matcher_create.argtypes = [vp, vp, vp]
        L.gw_mapper_matcher_destroy.restype = None
        L.gw_mapper_matcher_destroy.argtypes = [vp]
        L.gw_mapper_matcher_anchor_count.restype = i64
        L.gw_mapper_matcher_anchor_count.argtypes = [vp]
        L.gw_mapper_matcher_copy_anchors.argtypes = [vp, vp, i64, vp]
        L.gw_mapper_get_overlaps.restype = i64
        L.gw_mapper_get_overlaps.argtypes = [vp, i32, i64, i64, i64, f32, vp, vp, vp]
        L.gw_mapper_get_overlaps_host.restype = i64
        L.gw_mapper_get_overlaps_host.argtypes = [vp, i64, i32, i64, i64, i64, f32, vp, vp]
        L.gw_mapper_map.restype = i64
        L.gw_mapper_map.argtypes = [vp, vp, i32, vp, vp, i32, i32, i32, C.c_double, i64, i64, i64, f32, vp, i64, vp]
        u32 = C.c_uint32
        L.gw_mapper_post_process_overlaps.restype = i64
        L.gw_mapper_post_process_overlaps.argtypes = [vp, i64, i32, vp, i64, vp, vp]
        L.gw_mapper_rescue_overlap_ends.argtypes = [vp, i64, vp, vp, i32, vp, vp, i32, u32, u32, i32, f32, vp, vp]
        L.gw_mapper_extend_overlaps.argtypes = [vp, i64, vp, vp, i32, vp, vp, i32, u32, u32, vp, i32, i64, vp, vp, vp]
        L.gw_mapper_group_reads_into_indices.restype = i64
        L.gw_mapper_group_reads_into_indices.argtypes = [vp, i64, i64, vp, i64]
        L.gw_mapper_map_batched.restype = vp
        L.gw_mapper_map_batched.argtypes = [vp, vp, i32, vp, vp, i32, i32, i32, C.c_double, i64, i64, i64, f32, i64, i64,
                                            i32, i32, i32, vp]
        L.gw_mapper_overlaps_count.restype = i64
        L.gw_mapper_overlaps_count.argtypes = [vp]
        L.gw_mapper_overlaps_copy.argtypes = [vp, vp, i64, vp, vp]
        L.gw_mapper_overlaps_destroy.restype = None
        L.gw_mapper_overlaps_destroy.argtypes = [vp]
        L.gw_mapper_align_overlaps.restype = vp
        L.gw_mapper_align_overlaps.argtypes = [vp, i64, vp, vp, i32, u32, vp, vp, i32, u32, i64, vp]
        L.gw_mapper_align_overlaps_scored.restype = vp
        L.gw_mapper_align_overlaps_scored.argtypes = [vp, i64, vp, vp, i32, u32, vp, vp, i32, u32, vp, i64, vp]
        L.gw_mapper_align_overlaps_scored2.restype = vp
        L.gw_mapper_align_overlaps_scored2.argtypes = [vp, i64, vp, vp, i32, u32, vp, vp, i32, u32, vp, i64, vp]
        L.gw_mapper_cigars_count.restype = i64
        L.gw_mapper_cigars_count.argtypes = [vp]
        L.gw_mapper_cigars_text_bytes.restype = i64
        L.gw_mapper_cigars_text_bytes.argtypes = [vp]
        L.gw_mapper_cigars_copy.argtypes = [vp, vp, vp, vp, vp]
        L.gw_mapper_cigars_destroy.restype = None
        L.gw_mapper_cigars_destroy.argtypes = [vp]
        L.gw_mapper_map_batched_aligned.restype = vp
        L.gw_mapper_map_batched_aligned.argtypes = L.gw_mapper_map_batched.argtypes[:-1] + [i32, i64, vp]
        L.gw_mapper_overlaps_cigar_text_bytes.restype = i64
        L.gw_mapper_overlaps_cigar_text_bytes.argtypes = [vp]
        L.gw_mapper_overlaps_copy_cigars.argtypes = [vp, vp, vp, vp, vp]
        L.gw_mapper_map_batched_cached.restype = vp
        L.gw_mapper_map_batched_cached.argtypes = L.gw_mapper_map_batched.argtypes[:-1] + [i32, i64, i32, i32, i32, i32, vp]
        L.gw_mapper_overlaps_cache_counts.argtypes = [vp, vp, vp, vp]
        L.gw_mapper_chain_overlaps.restype = i64
        L.gw_mapper_chain_overlaps.argtypes = [vp, vp, i32, i64, i64, i64, f32, vp, vp, i64, vp, vp]
        L.gw_mapper_chain_overlaps_host.restype = i64
        L.gw_mapper_chain_overlaps_host.argtypes = [vp, i64, vp, i32, i64, i64, i64, f32, vp, vp, i64, vp, vp]
        L.gw_mapper_chain_overlaps_anchored.restype = i64
        L.gw_mapper_chain_overlaps_anchored.argtypes = [vp, vp, i32, i64, i64, i64, f32, vp, vp, i64, vp, vp, i64, vp, vp, vp]
        L.gw_mapper_chain_overlaps_anchored_host.restype = i64
        L.gw_mapper_chain_overlaps_anchored_host.argtypes = [vp, i64, vp, i32, i64, i64, i64, f32, vp, vp, i64, vp, vp, i64,
                                                             vp, vp, vp]
        L.gw_mapper_align_overlaps_anchored.restype = vp
        L.gw_mapper_align_overlaps_anchored.argtypes = [vp, i64, vp, vp, i32, u32, vp, vp, i32, u32, vp, vp, i64, i32, i32, vp,
                                                        i32, i64, vp]
        L.gw_mapper_map_batched_chained.restype = vp
        L.gw_mapper_map_batched_chained.argtypes = L.gw_mapper_map_batched_cached.argtypes[:-1] + [i32, i32, i32, i32, vp]
        L.gw_mapper_generate_batches_of_indices.restype = i64
        L.gw_mapper_generate_batches_of_indices.argtypes = [vp, i64, vp, i64, i64, i64, i32, i32, i32, i32, vp, i64]
        L.gw_mapper_index_host_copy_create.restype = vp
        L.gw_mapper_index_host_copy_create.argtypes = [vp, vp, vp]
        L.gw_mapper_index_host_copy_bytes.restype = i64
        L.gw_mapper_index_host_copy_bytes.argtypes = [vp]
        L.gw_mapper_index_host_copy_to_device.restype = vp
        L.gw_mapper_index_host_copy_to_device.argtypes = [vp, vp, vp]
        L.gw_mapper_index_host_copy_destroy.restype = None
        L.gw_mapper_index_host_copy_destroy.argtypes = [vp]
        L.gw_mapper_window_overlaps.restype = vp
        L.gw_mapper_window_overlaps.argtypes = [vp, i64, vp, vp, i32, u32, vp, vp, i32, u32, i32, i32, i64, vp]
        L.gw_mapper_window_segments.restype = vp
        L.gw_mapper_window_segments.argtypes = [vp, i64, vp, vp, i32, u32, vp, vp, i32, u32, i32, i64, vp]
        L.gw_mapper_windows_counts.argtypes = [vp, vp]
        L.gw_mapper_windows_copy_segments.argtypes = [vp, vp, vp, vp, vp]
        L.gw_mapper_windows_copy_windows.argtypes = [vp, vp, vp, vp, vp, vp]
        L.gw_mapper_windows_destroy.restype = None
        L.gw_mapper_windows_destroy.argtypes = [vp]
        L.gw_mapper_select_layers.restype = i64
        L.gw_mapper_select_layers.argtypes = [vp, i64, vp, i64, i32, u32, vp, i32, u32, i32, i32, vp, i64, vp, vp, i64]
        L.gw_mapper_select_pairs.restype = i64
        L.gw_mapper_select_pairs.argtypes = [vp, i64, vp, i64]
        L.gw_mapper_select_correction_layers.restype = i64
        L.gw_mapper_select_correction_layers.argtypes = [vp, i64, vp, i64, vp, i64, vp, i32, u32, i32, i32, vp, i64, vp,
                                                         vp, i64]
        L.gw_mapper_correction_windows.restype = vp
        L.gw_mapper_correction_windows.argtypes = [vp, i64, vp, vp, i32, u32, i32, i32, i64, vp]
        L.gw_mapper_pair_segments.restype = vp
        L.gw_mapper_pair_segments.argtypes = [vp, i64, vp, vp, i32, u32, i32, i64, vp]
        L.gw_mapper_windows_copy_query_role_segments.restype = i64
        L.gw_mapper_windows_copy_query_role_segments.argtypes = [vp, vp, i64, vp, vp, vp, vp]
        L.gw_mapper_window_overlaps_weighted.restype = vp
        L.gw_mapper_window_overlaps_weighted.argtypes = [vp, i64, vp, vp, i32, u32, vp, vp, i32, u32, vp, vp, i32, i32, i32,
                                                         i64, vp]
        L.gw_mapper_correction_windows_weighted.restype = vp
        L.gw_mapper_correction_windows_weighted.argtypes = [vp, i64, vp, vp, i32, u32, vp, i32, i32, i32, i64, vp]
        L.gw_mapper_windows_copy_weights.argtypes = [vp, vp, vp, vp, vp]
        L.gw_mapper_select_layers_weighted.restype = i64
        L.gw_mapper_select_layers_weighted.argtypes = [vp, i64, vp, i64, i32, u32, vp, i32, u32, i32, i32, vp, i32, vp, i64,
                                                       vp, vp, i64]
        L.gw_mapper_select_correction_layers_weighted.restype = i64
        L.gw_mapper_select_correction_layers_weighted.argtypes = [vp, i64, vp, i64, vp, i64, vp, i32, u32, i32, i32, vp, vp,
                                                                  i32, vp, i64, vp, vp, i64]
        L.gw_mapper_segment_quality_sums.argtypes = [vp, i64, vp, i64, i32, vp, vp, i32, u32, vp, vp, vp]
        L.gw_mapper_overlap_pileup.restype = vp
        L.gw_mapper_overlap_pileup.argtypes = [vp, i64, vp, vp, i32, u32, vp, vp, i32, u32, i64, vp]
        L.gw_mapper_pair_pileup.restype = vp
        L.gw_mapper_pair_pileup.argtypes = [vp, i64, vp, vp, i32, u32, i64, vp]
        L.gw_mapper_pileup_bases.restype = i64
        L.gw_mapper_pileup_bases.argtypes = [vp]
        L.gw_mapper_pileup_copy.argtypes = [vp, vp, vp]
        L.gw_mapper_pileup_destroy.restype = None
        L.gw_mapper_pileup_destroy.argtypes = [vp]
        L.gw_mapper_overlap_variants.restype = vp
        L.gw_mapper_overlap_variants.argtypes = [vp, i64, vp, vp, i32, u32, vp, vp, i32, u32, i32, i32, i64, vp]
        L.gw_mapper_overlap_variants_scored.restype = vp
        L.gw_mapper_overlap_variants_scored.argtypes = [vp, i64, vp, vp, i32, u32, vp, vp, i32, u32, i32, i32, vp, i64, vp]
        L.gw_mapper_overlap_variants_scored2.restype = vp
        L.gw_mapper_overlap_variants_scored2.argtypes = [vp, i64, vp, vp, i32, u32, vp, vp, i32, u32, i32, i32, vp, i64, vp]
        L.gw_mapper_variants_count.restype = i64
        L.gw_mapper_variants_count.argtypes = [vp]
        L.gw_mapper_variants_copy.argtypes = [vp, vp, vp]
        L.gw_mapper_variants_pileup_copy.argtypes = [vp, vp]
        L.gw_mapper_variants_destroy.restype = None
        L.gw_mapper_variants_destroy.argtypes = [vp]
        L.gwm_align_bytes_needed.restype = i64
        L.gwm_align_bytes_needed.argtypes = [i32, i32, i32]
        L.gwm_align_bytes_needed_scored.restype = i64
        L.gwm_align_bytes_needed_scored.argtypes = [i32, i32, i32]
        L.gwm_align_bytes_needed_anchored.restype = i64
        L.gwm_align_bytes_needed_anchored.argtypes = [vp, i32, i32, i32, i32]
        _mapper = L
    return _mapper
