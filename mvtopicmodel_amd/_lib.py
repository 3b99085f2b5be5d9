"""ctypes loader of libmvhdp.so (the C ABI of include/mvhdp.h)."""
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "lib", "libmvhdp.so")

MAX_M = 8

# every symbol include/mvhdp.h declares
ABI_SYMBOLS = [
    "mvhdp_create", "mvhdp_destroy", "mvhdp_last_error", "mvhdp_version",
    "mvhdp_set_corpus", "mvhdp_set_assignments", "mvhdp_set_view_presence", "mvhdp_get_assignments",
    "mvhdp_set_hyper", "mvhdp_get_alpha", "mvhdp_build_counts", "mvhdp_build_trees",
    "mvhdp_build_inference_trees", "mvhdp_init_assignments_from_trees",
    "mvhdp_get_counts", "mvhdp_set_counts", "mvhdp_get_tree", "mvhdp_get_doc_topic_hist",
    "mvhdp_get_count_histogram", "mvhdp_view_overlap_sums", "mvhdp_model_log_likelihood", "mvhdp_doc_topic_proportions",
    "mvhdp_doc_topics_top", "mvhdp_entity_topic_distributions", "mvhdp_similar_pairs", "mvhdp_sim_probe",
    "mvhdp_topic_phrases", "mvhdp_heldout_left_to_right", "mvhdp_fold_in", "mvhdp_predict_items", "mvhdp_score_items",
    "mvhdp_nearest_entities", "mvhdp_nearest_probe", "mvhdp_topic_top_entities", "mvhdp_predict_entities", "mvhdp_rank_entities",
    "mvhdp_topic_gram", "mvhdp_cohort_top_words", "mvhdp_word_cooccurrence", "mvhdp_remap_topics", "mvhdp_split_topic",
    "mvhdp_gamma_doc_statistics", "mvhdp_dp_table_statistics", "mvhdp_antoniak_draws",
    "mvhdp_top_words", "mvhdp_discr_weights", "mvhdp_diagnostics",
    "mvhdp_emb_init", "mvhdp_emb_count_words", "mvhdp_emb_train", "mvhdp_emb_get_vectors", "mvhdp_emb_set_vectors",
    "mvhdp_emb_word_stats", "mvhdp_emb_sampling_table", "mvhdp_emb_softmax", "mvhdp_emb_nearest", "mvhdp_emb_release",
    "mvhdp_set_vectors_mix", "mvhdp_get_vectors_mix",
    "mvhdp_sweep", "mvhdp_sweep_many", "mvhdp_get_tuning", "mvhdp_set_tuning", "mvhdp_plan_probe", "mvhdp_tuner_probe",
    "mvhdp_sweep_census",
    "mvhdp_apply_delta", "mvhdp_apply_delta_begin", "mvhdp_apply_delta_rows", "mvhdp_apply_delta_end",
    "mvhdp_get_birth_keys", "mvhdp_activate_births",
    "mvhdp_trees_current", "mvhdp_get_view_weights",
    "mvhdp_device_buffer", "mvhdp_counts_written", "mvhdp_set_stream", "mvhdp_synchronize",
    "mvhdp_group_create", "mvhdp_group_unique_id", "mvhdp_group_create_rank", "mvhdp_group_destroy", "mvhdp_group_last_error",
    "mvhdp_group_get_info", "mvhdp_group_set_exchange_chunks", "mvhdp_group_build_counts", "mvhdp_group_sweep", "mvhdp_group_abort", "mvhdp_group_drain",
    "mvhdp_group_set_hyper", "mvhdp_group_remap_topics", "mvhdp_group_log_likelihood", "mvhdp_group_doc_topic_hist", "mvhdp_group_count_histogram",
    "mvhdp_group_view_overlap_sums", "mvhdp_group_gamma_doc_statistics", "mvhdp_group_diagnostics",
]

UNIQUE_ID_BYTES = 128


class MvhdpError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"mvhdp error {code}: {msg}")
        self.code = code


class Config(C.Structure):
    _fields_ = [("num_topics", C.c_int32), ("num_modalities", C.c_int32),
                ("num_types", C.c_int32 * MAX_M), ("device", C.c_int32),
                ("doc_id_base", C.c_int64), ("flags", C.c_uint32)]


class HyperC(C.Structure):
    _fields_ = [("alpha", C.c_void_p),
                ("alpha_sum", C.c_double * MAX_M), ("beta", C.c_double * MAX_M),
                ("beta_sum", C.c_double * MAX_M), ("gamma", C.c_double * MAX_M),
                ("p_a", (C.c_double * MAX_M) * MAX_M), ("p_b", (C.c_double * MAX_M) * MAX_M),
                ("inactive", C.c_void_p)]


class SweepStatsC(C.Structure):
    _fields_ = [("tokens", C.c_int64), ("changed", C.c_int64), ("new_mass_cnt", C.c_int64),
                ("topic_doc_mass_cnt", C.c_int64), ("word_ftree_mass_cnt", C.c_int64),
                ("oov_skipped", C.c_int64), ("aborted_docs", C.c_int64), ("exact_fallbacks", C.c_int64),
                ("activated_topic", C.c_int32), ("activated_modality", C.c_int32),
                ("activation_key", C.c_int64), ("sweep_kernel_ms", C.c_double), ("total_ms", C.c_double),
                ("activations", C.c_int32), ("reserved", C.c_int32)]


class DebugC(C.Structure):
    _fields_ = [("tok_dbg", C.c_void_p * MAX_M), ("n_trace", C.c_int32),
                ("trace_doc", C.c_void_p), ("trace_view", C.c_void_p), ("trace_pos", C.c_void_p),
                ("trace_out", C.c_void_p)]


class TuningC(C.Structure):
    _fields_ = [("force_primary", C.c_int32), ("narrow", C.c_int32), ("walk_fixed", C.c_int32), ("single_stream", C.c_int32),
                ("live16", C.c_int32), ("single_wave", C.c_int32),
                ("walk_theta", C.c_double * MAX_M), ("primary_min_share", C.c_double),
                ("learnt_walk_step", C.c_int32 * 4), ("tree_branch_share", C.c_double * MAX_M),
                ("live_overlap", C.c_int32), ("live_rows", C.c_int32)]


class CensusRowC(C.Structure):
    _fields_ = [("rmax", C.c_int32), ("debug", C.c_int32), ("walk", C.c_int32), ("narrow", C.c_int32), ("roomy", C.c_int32),
                ("liverows", C.c_int32), ("mix", C.c_int32), ("reserved", C.c_int32), ("launches", C.c_int64), ("tokens", C.c_int64)]


class GroupInfoC(C.Structure):
    _fields_ = [("local_members", C.c_int32), ("local_devices", C.c_int32), ("ranks", C.c_int32), ("first_rank", C.c_int32),
                ("rccl", C.c_int32), ("rccl_version", C.c_int32), ("exchange_chunks", C.c_int32), ("exchange_packed", C.c_int32),
                ("last_exchange_ms", C.c_double), ("last_exchange_bytes", C.c_int64)]


class PlanInputC(C.Structure):
    _fields_ = [("num_topics", C.c_int32), ("num_modalities", C.c_int32), ("num_entities", C.c_int64),
                ("max_entity_tokens", C.c_int64), ("entities_longer_than", C.c_int64 * 5),
                ("tokens_by_list_rounds", C.c_uint64 * 17), ("entities_by_class", C.c_uint64 * 8),
                ("flags", C.c_uint32), ("debug", C.c_int32), ("batch", C.c_int32), ("trees_current", C.c_int32),
                ("num_cus", C.c_int32), ("kernel_registers", (C.c_int32 * 3) * 6), ("inactive_topics", C.c_int32),
                ("vectors_mix", C.c_int32), ("kernel_registers_mix", (C.c_int32 * 3) * 6), ("unassigned", C.c_int32)]


class PlanOutputC(C.Structure):
    _fields_ = [("status", C.c_int32), ("segments", C.c_int32), ("primary_class", C.c_int32), ("register_resident", C.c_int32),
                ("need_full_trees", C.c_int32), ("dominant_class", C.c_int32), ("routed_prefix", C.c_int64),
                ("class_used", C.c_int32 * 6), ("class_map", C.c_int32 * 6), ("class_stream", C.c_int32 * 6),
                ("class_grid", C.c_int32 * 6), ("class_walk", C.c_int32 * 6), ("class_narrow", C.c_int32 * 6),
                ("class_register_resident", C.c_int32 * 6), ("class_lds_bytes", C.c_int64 * 6), ("class_theta0", C.c_double * 6),
                ("delta16", C.c_int32), ("live_rows", C.c_int32)]


DIAG_MAX_TOP_WORDS = 64
DIAG_PROPORTIONS = 7
# the score rows of mvhdp_diagnostics, in the order of DIAG:104-116 (MVHDP_DIAG_* of include/mvhdp.h)
DIAG_ROWS = ["tokens", "document_entropy", "word-length", "coherence", "normDiscrWeight", "discrWeight", "uniform_dist",
             "corpus_dist", "eff_num_words", "token-doc-diff", "rank_1_docs", "allocation_ratio", "allocation_count"]


class DiagArgsC(C.Structure):
    _fields_ = [("num_top_words", C.c_int32), ("word_length", C.c_void_p)]


class DiagOutC(C.Structure):
    _fields_ = [("scores", C.c_void_p), ("word_scores", C.c_void_p), ("codoc", C.c_void_p), ("top_types", C.c_void_p),
                ("top_counts", C.c_void_p), ("nonzero", C.c_void_p), ("num_rank1_docs", C.c_void_p), ("num_nonzero_docs", C.c_void_p),
                ("num_docs_at_proportions", C.c_void_p), ("sum_count_log_count", C.c_void_p), ("word_type_counts", C.c_void_p),
                ("num_tokens", C.c_void_p), ("discr_weight_per_view", C.c_void_p)]


class EmbConfigC(C.Structure):
    _fields_ = [("num_columns", C.c_int32), ("num_context_columns", C.c_int32), ("with_topics", C.c_int32), ("window", C.c_int32),
                ("num_samples", C.c_int32), ("min_doc_length", C.c_int32), ("sampling_table_size", C.c_int64),
                ("sampling_factor", C.c_double), ("min_exp", C.c_double), ("max_exp", C.c_double),
                ("sigmoid_cache_size", C.c_int32), ("reserved", C.c_int32)]


class EmbStatsC(C.Structure):
    _fields_ = [("words_so_far", C.c_int64), ("words_sampled", C.c_int64), ("words_considered", C.c_int64),
                ("docs_skipped", C.c_int64), ("calls", C.c_int64), ("negatives_skipped", C.c_int64),
                ("residual", C.c_double), ("last_epoch_residual", C.c_double), ("last_epoch_calls", C.c_int64),
                ("kernel_ms", C.c_double)]


SIM_COS_FOLDED, SIM_COS, SIM_JSD = 0, 1, 2          # mvhdp_sim_metric


class SimArgsC(C.Structure):
    _fields_ = [("metric", C.c_int32), ("n", C.c_int32), ("dim", C.c_int32), ("x", C.c_void_p), ("min_weight", C.c_double),
                ("threshold", C.c_double), ("stripe_rows", C.c_int32), ("candidate_capacity", C.c_int64)]


class SimStatsC(C.Structure):
    _fields_ = [("pairs_screened", C.c_int64), ("candidates", C.c_int64), ("emitted", C.c_int64), ("stripes", C.c_int32),
                ("regrown", C.c_int32), ("margin", C.c_double)]


class PhraseArgsC(C.Structure):
    _fields_ = [("max_per_topic", C.c_int32), ("hash_bits", C.c_int32)]


class PhraseStatsC(C.Structure):
    _fields_ = [("runs", C.c_int64), ("occurrences", C.c_int64), ("distinct", C.c_int64), ("kept", C.c_int64), ("hash_collisions", C.c_int64)]


class HeldoutArgsC(C.Structure):
    _fields_ = [("m", C.c_int32), ("particles", C.c_int32), ("resample", C.c_int32), ("seed", C.c_uint64), ("doc_base", C.c_int64),
                ("alpha", C.c_void_p), ("alpha_sum", C.c_double)]


class HeldoutStatsC(C.Structure):
    _fields_ = [("log_likelihood", C.c_double), ("tokens", C.c_int64), ("oov", C.c_int64), ("visits", C.c_int64)]


class FoldinArgsC(C.Structure):
    _fields_ = [("iterations", C.c_int32), ("samples", C.c_int32), ("thin", C.c_int32), ("seed", C.c_uint64), ("doc_base", C.c_int64),
                ("coupling", C.c_void_p), ("view_weights", C.c_void_p)]


class FoldinStatsC(C.Structure):
    _fields_ = [("tokens", C.c_int64), ("oov", C.c_int64), ("visits", C.c_int64), ("kernel_ms", C.c_double)]


class PredictArgsC(C.Structure):
    _fields_ = [("m", C.c_int32), ("exclude_present", C.c_int32), ("view_weights", C.c_void_p), ("theta", C.c_void_p)]


class EntitiesArgsC(C.Structure):
    _fields_ = [("m", C.c_int32), ("exclude_present", C.c_int32), ("view_weights", C.c_void_p), ("c0", C.c_int64), ("c1", C.c_int64),
                ("nq", C.c_int64), ("q_off", C.c_void_p), ("q_items", C.c_void_p), ("q_weights", C.c_void_p), ("psi", C.c_void_p),
                ("block_entities", C.c_int64), ("block_queries", C.c_int64)]


class EntitiesStatsC(C.Structure):
    _fields_ = [("cells", C.c_int64), ("excluded", C.c_int64), ("blocks", C.c_int32), ("kernel_ms", C.c_double)]


class TopicGramArgsC(C.Structure):
    _fields_ = [("source", C.c_int32), ("m", C.c_int32), ("transform", C.c_int32), ("blocks_per_pass", C.c_int32),
                ("view_weights", C.c_void_p), ("x", C.c_void_p), ("r0", C.c_int64), ("r1", C.c_int64), ("threshold", C.c_double)]


class TopicGramStatsC(C.Structure):
    _fields_ = [("rows", C.c_int64), ("blocks", C.c_int32), ("passes", C.c_int32), ("kernel_ms", C.c_double)]


COHORT_BY_COUNT, COHORT_BY_SHARE = 0, 1             # mvhdp_cohort_order


class CohortArgsC(C.Structure):
    _fields_ = [("m", C.c_int32), ("n", C.c_int32), ("order", C.c_int32), ("min_count", C.c_int32), ("scratch_bytes", C.c_int64)]


class CohortStatsC(C.Structure):
    _fields_ = [("listings", C.c_int64), ("tokens", C.c_int64), ("skipped", C.c_int64), ("passes", C.c_int32),
                ("cohorts_per_pass", C.c_int32), ("kernel_ms", C.c_double)]


class CoocArgsC(C.Structure):
    _fields_ = [("m", C.c_int32), ("n", C.c_int32), ("window", C.c_int32), ("d0", C.c_int64), ("d1", C.c_int64)]


class CoocStatsC(C.Structure):
    _fields_ = [("entities", C.c_int64), ("tokens", C.c_int64), ("hits", C.c_int64), ("oov", C.c_int64),
                ("distinct_words", C.c_int32), ("memberships", C.c_int32), ("kernel_ms", C.c_double)]


REMAP_RETIRE = 0x1                                  # MVHDP_REMAP_RETIRE


class RemapArgsC(C.Structure):
    _fields_ = [("map", C.c_void_p), ("flags", C.c_uint32)]


class RemapStatsC(C.Structure):
    _fields_ = [("moved", C.c_int64 * MAX_M), ("dropped", C.c_int64 * MAX_M), ("vacated", C.c_int32), ("retired", C.c_int32),
                ("kernel_ms", C.c_double)]


SPLIT_KEEP_ALPHA = 0x1                              # MVHDP_SPLIT_KEEP_ALPHA


class SplitArgsC(C.Structure):
    _fields_ = [("source", C.c_int32), ("target", C.c_int32), ("iterations", C.c_int32), ("flags", C.c_uint32), ("seed", C.c_uint64),
                ("coupling", C.c_void_p), ("type_hint", C.c_void_p)]


class SplitStatsC(C.Structure):
    _fields_ = [("split", C.c_int64 * MAX_M), ("moved", C.c_int64 * MAX_M), ("flips_last", C.c_int64), ("target", C.c_int32),
                ("activated", C.c_int32), ("kernel_ms", C.c_double)]


class NearestArgsC(C.Structure):
    _fields_ = [("view_weights", C.c_void_p), ("c0", C.c_int64), ("c1", C.c_int64), ("queries", C.c_void_p), ("nq", C.c_int64),
                ("q0", C.c_int64), ("q1", C.c_int64), ("exclude_self", C.c_int32), ("n", C.c_int32), ("min_weight", C.c_double),
                ("block_queries", C.c_int32), ("stripe_candidates", C.c_int32), ("candidate_capacity", C.c_int64)]


class NearestStatsC(C.Structure):
    _fields_ = [("cells_screened", C.c_int64), ("candidates", C.c_int64), ("exact_only_rows", C.c_int64), ("blocks", C.c_int32),
                ("regrown", C.c_int32), ("margin", C.c_double)]


_lib = None
_preloaded = []            # keeps the handles of the runtime libraries loaded on the library's behalf alive


def _torch_lib_dir():
    """Directory of the ROCm runtime libraries a PyTorch-ROCm wheel bundles (None when torch is not installed).
    Found from the package's location alone: torch is NOT imported here."""
    import importlib.util
    try:
        spec = importlib.util.find_spec("torch")
    except (ImportError, ValueError):
        return None
    if spec is None or not spec.submodule_search_locations:
        return None
    d = os.path.join(list(spec.submodule_search_locations)[0], "lib")
    return d if os.path.isdir(d) else None


def mapped_runtime_libraries():
    """{'libamdhip64': [paths], 'libhsa-runtime64': [paths], 'librccl': [paths]} from /proc/self/maps: the distinct
    files of each ROCm runtime library mapped into this process."""
    found = {"libamdhip64": set(), "libhsa-runtime64": set(), "librccl": set()}
    try:
        with open("/proc/self/maps") as f:
            for line in f:
                path = line.rsplit(None, 1)[-1] if "/" in line else ""
                base = os.path.basename(path)
                for name in found:
                    if base.startswith(name + ".so"):
                        found[name].add(os.path.realpath(path))
    except OSError:
        pass
    return {k: sorted(v) for k, v in found.items()}


def _preload_one_hip_runtime():
    """One HIP runtime per process, whatever is imported first.

    libmvhdp.so needs `libamdhip64.so.7` (RUNPATH /opt/rocm/lib); a PyTorch-ROCm wheel bundles its own copy with the
    SAME soname but asks for it by the file name `libamdhip64.so`, which the loader does not match against an already
    mapped `libamdhip64.so.7` from /opt/rocm: a process that creates a sampler first and touches torch.cuda later ends up
    with two HIP runtimes over two ROCr copies, and torch then fails with "No HIP GPUs are available".  The other order
    is fine (libmvhdp's `libamdhip64.so.7` matches the soname of torch's copy).  So when a torch wheel with a bundled
    runtime is installed, its libamdhip64.so is mapped FIRST,
    process-wide, and both libmvhdp.so and a later `import torch` resolve to that one copy.  A host without torch (the
    Java host of INTEGRATION.md) is not affected: the library then runs on /opt/rocm's runtime."""
    d = _torch_lib_dir()
    if d is None:
        return False
    already = mapped_runtime_libraries()
    if already["libamdhip64"] or already["libhsa-runtime64"]:
        # a HIP runtime is mapped already (torch imported first -- fine, libmvhdp.so will use that copy -- or a profiler's
        # preloaded tool library brought /opt/rocm's): nothing to choose any more
        return False
    path = os.path.join(d, "libamdhip64.so")
    if not os.path.exists(path):
        return False
    _preloaded.append(C.CDLL(path, mode=C.RTLD_GLOBAL))
    # RCCL is opened by the library itself, lazily, in mvhdp_group_create (dlopen by soname: a copy torch has mapped
    # already is re-used).  When torch is installed but not imported yet, point the library at the wheel's copy so that
    # a later `import torch` maps the same file (mapping it here, process-wide and ahead of torch, aborts at exit).
    rccl = os.path.join(d, "librccl.so")
    if os.path.exists(rccl):
        os.environ.setdefault("MVHDP_RCCL_LIB", rccl)
    return True


def load_library():
    """Load libmvhdp.so; fails loudly when the HIP extension has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            f"{LIB_PATH} is missing: build it with `make -C mvtopicmodel_amd/csrc` "
            "(or __graft_entry__.build()).  There is no CPU fallback.")
    chose = _preload_one_hip_runtime()
    L = C.CDLL(LIB_PATH)
    maps = mapped_runtime_libraries()
    for name in ("libamdhip64", "libhsa-runtime64"):
        if chose and len(maps[name]) > 1:
            raise ImportError(
                f"two copies of {name} are mapped into this process ({', '.join(maps[name])}): a HIP runtime was loaded "
                "before mvtopicmodel_amd could pick one.  Import mvtopicmodel_amd (or torch) before any other library "
                "that links /opt/rocm's libamdhip64 in a process that also uses torch.")
    vp, i32, i64, u32, u64 = C.c_void_p, C.c_int32, C.c_int64, C.c_uint32, C.c_uint64
    L.mvhdp_create.argtypes = [C.POINTER(Config), C.POINTER(vp)]
    L.mvhdp_destroy.argtypes = [vp]
    L.mvhdp_last_error.argtypes = [vp]; L.mvhdp_last_error.restype = C.c_char_p
    L.mvhdp_version.restype = C.c_char_p
    L.mvhdp_set_corpus.argtypes = [vp, i32, i64, vp, vp]
    L.mvhdp_set_assignments.argtypes = [vp, i32, vp]
    L.mvhdp_set_view_presence.argtypes = [vp, i32, vp]
    L.mvhdp_get_assignments.argtypes = [vp, i32, vp]
    L.mvhdp_set_hyper.argtypes = [vp, C.POINTER(HyperC)]
    L.mvhdp_get_alpha.argtypes = [vp, vp, vp]
    L.mvhdp_build_counts.argtypes = [vp]
    L.mvhdp_build_trees.argtypes = [vp]
    L.mvhdp_build_inference_trees.argtypes = [vp]
    L.mvhdp_init_assignments_from_trees.argtypes = [vp, u64]
    L.mvhdp_get_counts.argtypes = [vp, i32, vp, vp]
    L.mvhdp_set_counts.argtypes = [vp, i32, vp, vp]
    L.mvhdp_get_tree.argtypes = [vp, i32, i32, vp]
    L.mvhdp_get_doc_topic_hist.argtypes = [vp, i32, vp, i32, vp, i32]
    L.mvhdp_get_count_histogram.argtypes = [vp, i32, vp, i32]
    L.mvhdp_view_overlap_sums.argtypes = [vp, vp]
    L.mvhdp_model_log_likelihood.argtypes = [vp, vp]
    L.mvhdp_doc_topic_proportions.argtypes = [vp, vp, i64, i64, vp]
    L.mvhdp_doc_topics_top.argtypes = [vp, vp, i64, i64, C.c_double, i32, i64, vp, vp, vp, C.POINTER(i64)]
    L.mvhdp_entity_topic_distributions.argtypes = [vp, vp, C.c_double, i32, i32, i64, vp, vp, vp]
    L.mvhdp_similar_pairs.argtypes = [vp, C.POINTER(SimArgsC), i64, vp, vp, vp, C.POINTER(i64), C.POINTER(SimStatsC)]
    L.mvhdp_sim_probe.argtypes = [i32, i32, i32, C.POINTER(SimStatsC)]
    L.mvhdp_topic_phrases.argtypes = [vp, C.POINTER(PhraseArgsC), i64, i64, vp, vp, vp, vp, vp, vp, C.POINTER(i64), C.POINTER(i64), C.POINTER(PhraseStatsC)]
    L.mvhdp_heldout_left_to_right.argtypes = [vp, C.POINTER(HeldoutArgsC), i64, vp, vp, vp, vp, vp, C.POINTER(HeldoutStatsC)]
    L.mvhdp_fold_in.argtypes = [vp, C.POINTER(FoldinArgsC), i64, vp, vp, vp, vp, vp, C.POINTER(FoldinStatsC)]
    L.mvhdp_predict_items.argtypes = [vp, C.POINTER(PredictArgsC), i64, i64, i32, vp, vp, vp]
    L.mvhdp_score_items.argtypes = [vp, C.POINTER(PredictArgsC), i64, i64, i64, vp, vp, vp, vp]
    L.mvhdp_predict_entities.argtypes = [vp, C.POINTER(EntitiesArgsC), i32, vp, vp, vp, C.POINTER(EntitiesStatsC)]
    L.mvhdp_rank_entities.argtypes = [vp, C.POINTER(EntitiesArgsC), i64, vp, vp, vp, vp]
    L.mvhdp_topic_gram.argtypes = [vp, C.POINTER(TopicGramArgsC), vp, vp, vp, vp, C.POINTER(TopicGramStatsC)]
    L.mvhdp_cohort_top_words.argtypes = [vp, C.POINTER(CohortArgsC), i64, vp, vp, vp, vp, vp, vp, vp, C.POINTER(CohortStatsC)]
    L.mvhdp_word_cooccurrence.argtypes = [vp, C.POINTER(CoocArgsC), i64, vp, i64, vp, vp, vp, vp, C.POINTER(CoocStatsC)]
    L.mvhdp_remap_topics.argtypes = [vp, C.POINTER(RemapArgsC), C.POINTER(RemapStatsC)]
    L.mvhdp_group_remap_topics.argtypes = [vp, C.POINTER(RemapArgsC), C.POINTER(RemapStatsC)]
    L.mvhdp_split_topic.argtypes = [vp, C.POINTER(SplitArgsC), vp, C.POINTER(SplitStatsC)]
    L.mvhdp_nearest_entities.argtypes = [vp, C.POINTER(NearestArgsC), vp, vp, vp, C.POINTER(NearestStatsC)]
    L.mvhdp_nearest_probe.argtypes = [i64, i64, i32, i32, i32, C.POINTER(NearestStatsC)]
    L.mvhdp_topic_top_entities.argtypes = [vp, vp, i64, i64, i32, C.c_double, i64, i64, vp, vp, vp]
    L.mvhdp_gamma_doc_statistics.argtypes = [vp, i32, C.c_double, u64, u32, C.POINTER(C.c_double), C.POINTER(C.c_double)]
    L.mvhdp_dp_table_statistics.argtypes = [vp, i32, vp, i32, vp, u64, u32, vp, vp]
    L.mvhdp_antoniak_draws.argtypes = [vp, i32, vp, vp, u64, u32, vp]
    L.mvhdp_top_words.argtypes = [vp, i32, i32, vp, vp, vp]
    L.mvhdp_discr_weights.argtypes = [vp, vp, i32, vp]
    L.mvhdp_diagnostics.argtypes = [vp, C.POINTER(DiagArgsC), C.POINTER(DiagOutC)]
    L.mvhdp_emb_init.argtypes = [vp, C.POINTER(EmbConfigC), vp, u64]
    L.mvhdp_emb_count_words.argtypes = [vp]
    L.mvhdp_emb_train.argtypes = [vp, i32, u64, u32, u32, C.POINTER(EmbStatsC)]
    L.mvhdp_emb_get_vectors.argtypes = [vp, vp, vp]
    L.mvhdp_emb_set_vectors.argtypes = [vp, vp, vp]
    L.mvhdp_emb_word_stats.argtypes = [vp, vp, vp, vp]
    L.mvhdp_emb_sampling_table.argtypes = [vp, i64, i64, vp]
    L.mvhdp_emb_softmax.argtypes = [vp, i32, vp, vp]
    L.mvhdp_emb_nearest.argtypes = [vp, vp, i32, vp, vp, vp, vp]
    L.mvhdp_emb_release.argtypes = [vp]
    L.mvhdp_set_vectors_mix.argtypes = [vp, C.c_double, vp, vp]
    L.mvhdp_get_vectors_mix.argtypes = [vp, C.POINTER(C.c_double), vp]
    L.mvhdp_sweep.argtypes = [vp, u32, u64, u32, vp, C.POINTER(DebugC), C.POINTER(SweepStatsC)]
    L.mvhdp_sweep_many.argtypes = [vp, u32, i32, u64, u32, vp]
    L.mvhdp_get_tuning.argtypes = [vp, C.POINTER(TuningC)]
    L.mvhdp_set_tuning.argtypes = [vp, C.POINTER(TuningC)]
    L.mvhdp_plan_probe.argtypes = [C.POINTER(PlanInputC), C.POINTER(TuningC), C.POINTER(PlanOutputC)]
    L.mvhdp_tuner_probe.argtypes = [i32, vp, vp, vp, i32, i32, vp]
    L.mvhdp_sweep_census.argtypes = [vp, i32, i32, C.POINTER(CensusRowC), i32, C.POINTER(i32)]
    L.mvhdp_apply_delta.argtypes = [vp, i32, i32]
    L.mvhdp_apply_delta_begin.argtypes = [vp]
    L.mvhdp_apply_delta_rows.argtypes = [vp, i64, i64]
    L.mvhdp_apply_delta_end.argtypes = [vp, i32, i32]
    L.mvhdp_get_birth_keys.argtypes = [vp, vp]
    L.mvhdp_activate_births.argtypes = [vp, vp]
    L.mvhdp_trees_current.argtypes = [vp]
    L.mvhdp_get_view_weights.argtypes = [vp, vp]
    L.mvhdp_device_buffer.argtypes = [vp, C.c_int, C.POINTER(vp), C.POINTER(C.c_size_t)]
    L.mvhdp_counts_written.argtypes = [vp]
    L.mvhdp_set_stream.argtypes = [vp, vp]
    L.mvhdp_synchronize.argtypes = [vp]
    L.mvhdp_group_create.argtypes = [i32, C.POINTER(vp), C.POINTER(vp)]
    L.mvhdp_group_unique_id.argtypes = [vp]
    L.mvhdp_group_create_rank.argtypes = [vp, vp, i32, i32, C.POINTER(vp)]
    L.mvhdp_group_destroy.argtypes = [vp]
    L.mvhdp_group_last_error.argtypes = [vp]; L.mvhdp_group_last_error.restype = C.c_char_p
    L.mvhdp_group_get_info.argtypes = [vp, C.POINTER(GroupInfoC)]
    L.mvhdp_group_set_exchange_chunks.argtypes = [vp, i32]
    L.mvhdp_group_build_counts.argtypes = [vp]
    L.mvhdp_group_sweep.argtypes = [vp, u32, u64, u32, vp]
    L.mvhdp_group_abort.argtypes = [vp]
    L.mvhdp_group_drain.argtypes = [vp]
    L.mvhdp_group_set_hyper.argtypes = [vp, C.POINTER(HyperC)]
    L.mvhdp_group_log_likelihood.argtypes = [vp, vp]
    L.mvhdp_group_doc_topic_hist.argtypes = [vp, i32, vp, i32, vp, i32]
    L.mvhdp_group_count_histogram.argtypes = [vp, i32, vp, i32]
    L.mvhdp_group_view_overlap_sums.argtypes = [vp, vp]
    L.mvhdp_group_gamma_doc_statistics.argtypes = [vp, i32, C.c_double, u64, u32, C.POINTER(C.c_double), C.POINTER(C.c_double)]
    L.mvhdp_group_diagnostics.argtypes = [vp, C.POINTER(DiagArgsC), C.POINTER(DiagOutC)]
    for name in ABI_SYMBOLS:
        f = getattr(L, name)  # raises AttributeError if the symbol is not exported
        if name not in ("mvhdp_last_error", "mvhdp_version", "mvhdp_group_last_error"):
            f.restype = C.c_int
    _lib = L
    return L
