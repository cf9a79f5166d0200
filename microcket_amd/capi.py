"""ctypes binding of include/mkt.h (libmkt_hip.so).  Plumbing only: no record is ever touched here."""
import collections
import ctypes as C
import os
import sys
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
MODE_FLASH, MODE_UNC = 0, 1
TILES_AUTO, TILES_FAST, TILES_SMALL = 0, 1, 2
EXT_KEYS = 1
EXT_LANES = 2
KEY_BYTES = 24
EXPORTS = [
    "mkt_abi_version", "mkt_strerror", "mkt_last_error", "mkt_device_count", "mkt_create", "mkt_destroy",
    "mkt_input_window", "mkt_submit_window",
    "mkt_submit", "mkt_drain", "mkt_drain_wait", "mkt_submit_device", "mkt_sync", "mkt_fetch_last_block", "mkt_finish",
    "mkt_format_log", "mkt_get_timing", "mkt_reset_timing", "mkt_get_replays", "mkt_synth_device", "mkt_copy_to_host", "mkt_device_text",
    "mkt_reset", "mkt_ext_dedup", "mkt_ext_chrstat", "mkt_ext_chr_names", "mkt_ext_keys_fetch", "mkt_ext_dedup_keys", "mkt_ext_keys_device", "mkt_ext_partition", "mkt_ext_dedup_device", "mkt_ext_unpartition", "mkt_ext_dedup_multi", "mkt_dataset_create", "mkt_dataset_info", "mkt_dataset_block", "mkt_dataset_destroy", "mkt_group_count",
    "mkt_sorter_create", "mkt_sorter_destroy", "mkt_sorter_error", "mkt_sorter_add", "mkt_sorter_add_device", "mkt_sorter_sort", "mkt_sorter_fetch",
    "mkt_rmdup_create", "mkt_rmdup_destroy", "mkt_rmdup_error", "mkt_rmdup_reserve", "mkt_rmdup_add", "mkt_rmdup_run", "mkt_rmdup_fetch",
    "mkt_rmdup_begin", "mkt_rmdup_push", "mkt_rmdup_stats",
    "mkt_stitch_create", "mkt_stitch_destroy", "mkt_stitch_error", "mkt_stitch_check", "mkt_stitch_segment_pairs", "mkt_stitch_begin", "mkt_stitch_push",
    "mkt_stitch_fetch", "mkt_stitch_stats", "mkt_stitch_timing",
    "mkt_trim_default_opts", "mkt_trim_create", "mkt_trim_destroy", "mkt_trim_error", "mkt_trim_check", "mkt_trim_segment_pairs", "mkt_trim_begin", "mkt_trim_push",
    "mkt_trim_fetch", "mkt_trim_stats", "mkt_trim_timing",
    "mkt_bam_create", "mkt_bam_destroy", "mkt_bam_error", "mkt_bam_note", "mkt_bam_add", "mkt_bam_add_device", "mkt_bam_run", "mkt_bam_fetch",
    "mkt_bam_reserve", "mkt_bam_window", "mkt_bam_commit", "mkt_bam_read", "mkt_bam_spill", "mkt_bam_pull", "mkt_bam_stats",
    "mkt_matrix_create", "mkt_matrix_destroy", "mkt_matrix_error", "mkt_matrix_add", "mkt_matrix_add_device", "mkt_matrix_add_keys", "mkt_matrix_run",
    "mkt_matrix_info", "mkt_matrix_fetch", "mkt_matrix_fetch_text", "mkt_matrix_timing",
    "mkt_balance_opts_default", "mkt_matrix_balance", "mkt_matrix_fetch_weights", "mkt_matrix_balance_timing",
    "mkt_expected_opts_default", "mkt_matrix_expected", "mkt_matrix_fetch_expected_cis", "mkt_matrix_fetch_expected_trans", "mkt_matrix_fetch_expected_genome",
    "mkt_matrix_fetch_values", "mkt_matrix_expected_timing",
    "mkt_loops_opts_default", "mkt_matrix_loops", "mkt_matrix_fetch_loop_cells", "mkt_matrix_fetch_loop_hist", "mkt_matrix_fetch_loop_thresholds",
    "mkt_matrix_fetch_loops", "mkt_matrix_loops_timing",
    "mkt_eigs_opts_default", "mkt_matrix_eigs", "mkt_matrix_fetch_eigvecs", "mkt_matrix_fetch_eigvals", "mkt_matrix_eigs_apply", "mkt_matrix_eigs_timing",
    "mkt_insulation_opts_default", "mkt_matrix_insulation", "mkt_matrix_fetch_insulation", "mkt_matrix_insulation_timing",
    "mkt_pileup_opts_default", "mkt_matrix_pileup", "mkt_matrix_fetch_pileup", "mkt_matrix_fetch_pileup_status", "mkt_matrix_pileup_timing",
    "mkt_saddle_opts_default", "mkt_matrix_saddle", "mkt_matrix_fetch_saddle", "mkt_matrix_fetch_saddle_groups", "mkt_matrix_fetch_saddle_edges",
    "mkt_matrix_fetch_saddle_profile", "mkt_matrix_saddle_timing",
    "mkt_scc_opts_default", "mkt_matrix_scc", "mkt_matrix_fetch_scc_strata", "mkt_matrix_fetch_scc_chrom", "mkt_matrix_scc_timing",
    "mkt_viewpoint_opts_default", "mkt_matrix_viewpoint", "mkt_matrix_fetch_viewpoint_links", "mkt_matrix_fetch_viewpoint_track",
    "mkt_matrix_fetch_viewpoint_partners", "mkt_matrix_viewpoint_timing",
    "mkt_hic_opts_default", "mkt_matrix_hic", "mkt_matrix_fetch_hic", "mkt_matrix_hic_timing",
    "mkt_paircmp_create", "mkt_paircmp_destroy", "mkt_paircmp_error", "mkt_paircmp_add", "mkt_paircmp_add_device", "mkt_paircmp_opts_default", "mkt_paircmp_run",
    "mkt_paircmp_fetch_classes", "mkt_paircmp_fetch_lines", "mkt_paircmp_report", "mkt_paircmp_timing",
    "mkt_pairsgz_create", "mkt_pairsgz_destroy", "mkt_pairsgz_error", "mkt_pairsgz_add", "mkt_pairsgz_opts_default", "mkt_pairsgz_run", "mkt_pairsgz_fetch_gz",
    "mkt_pairsgz_fetch_px2", "mkt_pairsgz_timing",
    "mkt_bgzf_create", "mkt_bgzf_destroy", "mkt_bgzf_error", "mkt_bgzf_add", "mkt_bgzf_opts_default", "mkt_bgzf_run", "mkt_bgzf_fetch_text", "mkt_bgzf_device_text",
    "mkt_bgzf_load_index", "mkt_bgzf_count", "mkt_bgzf_timing", "mkt_bgzf_query", "mkt_bgzf_fetch_query", "mkt_bgzf_fetch_query_offsets", "mkt_bgzf_fetch_query_counts",
    "mkt_bgzf_query_device", "mkt_bgzf_names", "mkt_bgzf_clear",
    "mkt_bamtext_create", "mkt_bamtext_destroy", "mkt_bamtext_error", "mkt_bamtext_add", "mkt_bamtext_add_device", "mkt_bamtext_opts_default", "mkt_bamtext_run",
    "mkt_bamtext_finish", "mkt_bamtext_fetch_header", "mkt_bamtext_fetch_ref", "mkt_bamtext_fetch_text", "mkt_bamtext_device_text", "mkt_bamtext_timing",
    "mkt_pairstat_create", "mkt_pairstat_destroy", "mkt_pairstat_error", "mkt_pairstat_add", "mkt_pairstat_add_device", "mkt_pairstat_add_keys", "mkt_pairstat_opts_default",
    "mkt_pairstat_run", "mkt_pairstat_fetch_dist", "mkt_pairstat_fetch_chrom", "mkt_pairstat_fetch_scaling", "mkt_pairstat_text", "mkt_pairstat_timing",
]


class MktError(RuntimeError):
    pass


class Params(C.Structure):
    _fields_ = [("mode", C.c_int32), ("min_mapped_ratio", C.c_float), ("min_mapq", C.c_int32), ("write_sam", C.c_int32),
                ("ref_threads", C.c_int32), ("device", C.c_int32), ("block_bytes", C.c_uint64), ("tiles", C.c_int32),
                ("ordered", C.c_int32), ("extensions", C.c_uint32), ("reserved2", C.c_uint32)]


class Stats(C.Structure):
    _fields_ = [(k, C.c_uint32) for k in ("lowMap", "manyHits", "unpaired", "selfCircle", "trans", "cis10K", "cis1K", "cis0",
                                           "selfCircle_all", "reserved")] + \
               [(k, C.c_uint64) for k in ("groups", "pairs", "pair_bytes", "sam_bytes", "lines_in", "bytes_in", "blocks")]

    def counters(self):
        return {k: getattr(self, k) for k in ("lowMap", "manyHits", "unpaired", "selfCircle", "trans", "cis10K", "cis1K", "cis0")}


class Out(C.Structure):
    _fields_ = [("pairs", C.c_void_p), ("pairs_len", C.c_size_t), ("sam", C.c_void_p), ("sam_len", C.c_size_t)]


class BalanceOpts(C.Structure):
    """mkt_balance_opts of include/mkt.h"""
    _fields_ = [("ignore_diags", C.c_int32), ("min_nnz", C.c_int32), ("min_count", C.c_double), ("mad_max", C.c_double), ("tol", C.c_double),
                ("max_iters", C.c_int32), ("reserved", C.c_uint32)]


class _BalanceStatsC(C.Structure):
    _fields_ = [("iterations", C.c_uint32), ("converged", C.c_int32), ("var", C.c_double), ("scale", C.c_double), ("masked", C.c_uint64)]


BalanceStats = collections.namedtuple("BalanceStats", "iterations converged var scale masked")


class ExpectedOpts(C.Structure):
    """mkt_expected_opts of include/mkt.h"""
    _fields_ = [("use_weights", C.c_int32), ("reserved", C.c_uint32)]


class _ExpectedInfoC(C.Structure):
    _fields_ = [("cis_rows", C.c_uint64), ("trans_rows", C.c_uint64), ("genome_rows", C.c_uint64), ("n_chrom", C.c_uint32), ("smooth_groups", C.c_uint32)]


ExpectedCis = collections.namedtuple("ExpectedCis", "n_valid count_sum balanced_sum")
ExpectedTrans = collections.namedtuple("ExpectedTrans", "n_valid count_sum balanced_sum expected")
ExpectedGenome = collections.namedtuple("ExpectedGenome", "n_valid count_sum balanced_sum expected expected_smooth")
Expected = collections.namedtuple("Expected", "cis trans genome n_chrom smooth_groups")
VALUE_KINDS = {"balanced": 0, "oe": 1, "oe_smooth": 2}


class LoopsOpts(C.Structure):
    """mkt_loops_opts of include/mkt.h"""
    _fields_ = [("peak", C.c_int32), ("window", C.c_int32), ("window_max", C.c_int32), ("min_ll_count", C.c_int32), ("min_dist", C.c_int32),
                ("max_dist", C.c_int32), ("fdr", C.c_double), ("cluster_radius", C.c_int32), ("reserved", C.c_uint32)]


class _LoopsInfoC(C.Structure):
    _fields_ = [(k, C.c_uint64) for k in ("cells", "candidates", "tested", "undefined", "over", "grew", "at_max", "enriched", "loops")]


class _LoopC(C.Structure):
    _fields_ = [("cell", C.c_uint64), ("bin1", C.c_uint32), ("bin2", C.c_uint32), ("count", C.c_uint32), ("window", C.c_uint32), ("n_cells", C.c_uint32),
                ("box", C.c_uint32 * 4), ("reserved", C.c_uint32), ("r", C.c_double * 4)]


LoopsInfo = collections.namedtuple("LoopsInfo", "cells candidates tested undefined over grew at_max enriched loops")
Loop = collections.namedtuple("Loop", "cell bin1 bin2 count window r n_cells box")
Loops = collections.namedtuple("Loops", "loops info")
LoopCells = collections.namedtuple("LoopCells", "status window chunk r enriched csum_ll kept bsum esum e")
LOOP_NONE, LOOP_TESTED, LOOP_UNDEFINED, LOOP_OVER = 0, 1, 2, 3


class EigsOpts(C.Structure):
    """mkt_eigs_opts of include/mkt.h"""
    _fields_ = [("n_eigs", C.c_int32), ("ignore_diags", C.c_int32), ("min_good", C.c_int32), ("max_iters", C.c_int32), ("tol", C.c_double), ("clip", C.c_double),
                ("reserved", C.c_uint32)]


class _EigsInfoC(C.Structure):
    _fields_ = [(k, C.c_uint32) for k in ("n_chrom", "solved", "converged", "skipped", "max_iterations")]


EigsInfo = collections.namedtuple("EigsInfo", "n_chrom solved converged skipped max_iterations")
Eigs = collections.namedtuple("Eigs", "info vectors lambdas resid n_good iterations converged")
EIGS_OPTS = ("n_eigs", "ignore_diags", "min_good", "max_iters", "tol", "clip")


class InsulationOpts(C.Structure):
    """mkt_insulation_opts of include/mkt.h"""
    _fields_ = [("n_windows", C.c_int32), ("window", C.c_int32 * 4), ("ignore_diags", C.c_int32), ("use_weights", C.c_int32), ("reserved", C.c_uint32),
                ("min_frac_valid", C.c_double), ("min_strength", C.c_double)]


class _InsulationInfoC(C.Structure):
    _fields_ = [("defined", C.c_uint64 * 4), ("minima", C.c_uint64 * 4), ("boundaries", C.c_uint64 * 4), ("n_chrom", C.c_uint32), ("reserved", C.c_uint32)]


InsulationInfo = collections.namedtuple("InsulationInfo", "n_chrom windows defined minima boundaries")
InsulationTrack = collections.namedtuple("InsulationTrack", "n_valid csum bsum score log2_score strength boundary")
INSULATION_OPTS = ("ignore_diags", "use_weights", "min_frac_valid", "min_strength")


class PileupOpts(C.Structure):
    """mkt_pileup_opts of include/mkt.h"""
    _fields_ = [("flank", C.c_int32), ("corner", C.c_int32), ("kind", C.c_int32), ("ignore_diags", C.c_int32), ("edges", C.c_int32), ("min_dist", C.c_int32),
                ("max_dist", C.c_int32), ("reserved", C.c_uint32)]


class _PileupInfoC(C.Structure):
    _fields_ = [(k, C.c_uint64) for k in ("features", "used", "trans", "edge", "dist")] + [("side", C.c_uint32), ("chunks", C.c_uint32)] + \
               [(k, C.c_double) for k in ("peak", "p2ll", "p2ul", "p2ur", "p2lr", "p2m", "z_ll")]


PileupInfo = collections.namedtuple("PileupInfo", "features used trans edge dist side chunks peak p2ll p2ul p2ur p2lr p2m z_ll")
Pileup = collections.namedtuple("Pileup", "n csum vsum mean status")
PILEUP_OPTS = ("flank", "corner", "kind", "ignore_diags", "edges", "min_dist", "max_dist")
PILE_USED, PILE_TRANS, PILE_EDGE, PILE_DIST = 1, 2, 3, 4


class SaddleOpts(C.Structure):
    """mkt_saddle_opts of include/mkt.h"""
    _fields_ = [(k, C.c_int32) for k in ("n_groups", "trim_lo", "trim_hi", "contact", "kind", "min_diag", "max_diag", "corner")] + [("reserved", C.c_uint32)]


class _SaddleInfoC(C.Structure):
    _fields_ = [(k, C.c_uint64) for k in ("candidates", "kept", "cells_used")] + [(k, C.c_uint32) for k in ("n_groups", "chunks", "corner", "reserved")] + \
               [(k, C.c_double) for k in ("strength", "aa_ab", "bb_ab")]


SaddleInfo = collections.namedtuple("SaddleInfo", "n_groups candidates kept cells_used chunks corner strength aa_ab bb_ab")
Saddle = collections.namedtuple("Saddle", "n nnz csum vsum mean groups group_bins group_lo group_hi strength aa_ab bb_ab")
SADDLE_OPTS = ("n_groups", "trim_lo", "trim_hi", "contact", "kind", "min_diag", "max_diag", "corner")
SADDLE_CONTACTS = {"cis": 0, "trans": 1}
SADDLE_NONE = 255


class SccOpts(C.Structure):
    """mkt_scc_opts of include/mkt.h"""
    _fields_ = [(k, C.c_int32) for k in ("h", "min_diag", "max_diag", "use_weights", "weighting", "min_n", "slab_rows")] + [("reserved", C.c_uint32 * 3)]


class _SccInfoC(C.Structure):
    _fields_ = [(k, C.c_uint32) for k in ("n_chrom", "strata")] + [(k, C.c_uint64) for k in ("candidates", "used", "scored", "count_a", "count_b")] + [("scc", C.c_double)]


SccInfo = collections.namedtuple("SccInfo", "n_chrom strata candidates used scored count_a count_b scc")
Scc = collections.namedtuple("Scc", "n_cand n sx sy sxx syy sxy rho w scc num den n_scored")
SCC_OPTS = ("h", "min_diag", "max_diag", "use_weights", "weighting", "min_n", "slab_rows")
SCC_WEIGHTINGS = {"n": 0, "var": 1}


class ViewpointOpts(C.Structure):
    """mkt_viewpoint_opts of include/mkt.h"""
    _fields_ = [("partner_mask", C.c_void_p), ("hotspot_ratio", C.c_double)] + [(k, C.c_uint32) for k in ("viewpoint", "vbin", "pbin", "min_count")] + \
               [("origin", C.c_int32), ("second_side_only", C.c_int32), ("reserved", C.c_uint32 * 2)]


class HicOpts(C.Structure):
    """mkt_hic_opts of include/mkt.h"""
    _fields_ = [("genome_id", C.c_char_p), ("norm_label", C.c_char_p), ("block_bins", C.c_uint32), ("level", C.c_int32), ("norm", C.c_int32), ("reserved", C.c_uint32)]


class _HicInfoC(C.Structure):
    _fields_ = [(k, C.c_uint64) for k in ("file_bytes", "matrices", "blocks", "float_blocks", "pieces", "raw_bytes", "deflated_bytes")]


class _ViewpointInfoC(C.Structure):
    _fields_ = [(k, C.c_uint64) for k in ("total", "links", "links_kept", "partner_cells", "partner_cells_kept")] + [(k, C.c_uint32) for k in ("min_loop", "viewpoint_bins")]


ViewpointInfo = collections.namedtuple("ViewpointInfo", "total links links_kept partner_cells partner_cells_kept min_loop viewpoint_bins")
Viewpoint = collections.namedtuple("Viewpoint", "link_vbin link_chrom link_pbin link_count track partner_chrom partner_pbin partner_count info")
VIEWPOINT_OPTS = ("vbin", "pbin", "origin", "second_side_only", "min_count", "hotspot_ratio", "reserved")


class PairStatsOpts(C.Structure):
    """mkt_pairstat_opts of include/mkt.h"""
    _fields_ = [("tol_permille", C.c_uint32), ("reserved0", C.c_uint32), ("min_count", C.c_uint64), ("reserved", C.c_uint32 * 4)]


class _PairStatsInfoC(C.Structure):
    _fields_ = [(k, C.c_uint64) for k in ("total", "skipped", "counted", "cis", "trans", "no_strand", "header_lines")] + \
               [("cis_ge", C.c_uint64 * 6), ("cis0", C.c_uint64), ("cis1K", C.c_uint64), ("cis10K", C.c_uint64), ("ref_trans", C.c_uint64), ("convergence_dist", C.c_int64),
                ("n_chrom", C.c_uint32), ("reserved", C.c_uint32)]


PairStatsScaling = collections.namedtuple("PairStatsScaling", "edges area P")


class PairCompareOpts(C.Structure):
    _fields_ = [("max_dist", C.c_uint32), ("want_lines", C.c_uint32), ("hash_bits", C.c_uint32), ("reserved", C.c_uint32 * 5)]


class _PairCompareInfoC(C.Structure):
    _fields_ = [("lines", C.c_uint64 * 2), ("data_lines", C.c_uint64 * 2), ("distinct_a", C.c_uint64), ("consistent", C.c_uint64), ("discordant", C.c_uint64),
                ("a_only", C.c_uint64), ("b_only", C.c_uint64), ("dist", (C.c_uint64 * 4) * 2), ("host_runs", C.c_uint64), ("lines_bytes", C.c_uint64)]


class PairsGzOpts(C.Structure):
    """mkt_pairsgz_opts of include/mkt.h"""
    _fields_ = [("level", C.c_int32), ("preset", C.c_uint32), ("reserved", C.c_uint32 * 6)]


class _PairsGzInfoC(C.Structure):
    _fields_ = [(k, C.c_uint64) for k in ("lines", "records", "names", "bins", "chunks", "blocks", "gz_bytes", "px2_bytes")]


PairsGzInfo = collections.namedtuple("PairsGzInfo", "lines records names bins chunks blocks gz_bytes px2_bytes")


class _BgzfInfoC(C.Structure):
    _fields_ = [(k, C.c_uint64) for k in ("blocks", "gz_bytes", "text_bytes", "stored", "fixed", "dynamic")] + [("has_eof", C.c_uint32), ("reason", C.c_uint32), ("bad_offset", C.c_uint64)]


BgzfInfo = collections.namedtuple("BgzfInfo", "blocks gz_bytes text_bytes stored fixed dynamic has_eof")


class BgzfQueryOpts(C.Structure):
    _fields_ = [("autoflip", C.c_uint32), ("reserved", C.c_uint32 * 7)]


class _BgzfQueryInfoC(C.Structure):
    _fields_ = [(k, C.c_uint64) for k in ("regions", "subqueries", "chunks", "blocks_inflated", "bytes_inflated", "candidate_lines", "lines", "answer_bytes", "unparsed")] + \
               [("reason", C.c_uint32), ("pad", C.c_uint32), ("bad_offset", C.c_uint64)]


BgzfQueryInfo = collections.namedtuple("BgzfQueryInfo", "regions subqueries chunks blocks_inflated bytes_inflated candidate_lines lines answer_bytes unparsed")


class BamTextOpts(C.Structure):
    """mkt_bamtext_opts of include/mkt.h"""
    _fields_ = [("segment_bytes", C.c_uint32), ("max_record", C.c_uint32), ("reserved", C.c_uint32 * 6)]


class _BamTextInfoC(C.Structure):
    _fields_ = [(k, C.c_uint64) for k in ("records", "text_bytes", "segments", "repairs", "float_records", "carry_bytes")] + \
               [("reason", C.c_uint32), ("header_done", C.c_uint32), ("bad_record", C.c_uint64), ("bad_offset", C.c_uint64)]


BamTextInfo = collections.namedtuple("BamTextInfo", "records text_bytes segments repairs float_records carry_bytes header_done")


class Timing(C.Structure):
    _fields_ = [("tile_kernel_ms", C.c_double), ("tile_launches", C.c_uint64), ("tile_bytes", C.c_uint64), ("other_ms", C.c_double),
                ("tiles", C.c_uint64), ("deferred_tiles", C.c_uint64)]


class _ReplaysC(C.Structure):
    """mkt_replays of include/mkt.h"""
    _fields_ = [(k, C.c_uint64) for k in ("geometry", "pairs_cap", "sam_cap", "sc_cap", "jobs_rerun")]


Replays = collections.namedtuple("Replays", "geometry pairs_cap sam_cap sc_cap jobs_rerun")


def lib_path():
    # MKT_LIB selects a diagnostic build (e.g. the phase-stamp build); never needed in production
    return os.environ.get("MKT_LIB") or os.path.join(HERE, "libmkt_hip.so")


def exe_path():
    return os.path.join(HERE, "bin", "sam2pairs")


_lib = None


def hip_runtimes():
    """The HIP runtime libraries mapped into this process (paths of libamdhip64.so*)."""
    found = set()
    try:
        with open("/proc/self/maps") as f:
            for line in f:
                if "libamdhip64" in line:
                    found.add(os.path.realpath(line.split()[-1]))
    except OSError:
        pass
    return sorted(found)


def check_single_hip_runtime():
    """One HIP runtime per process.  PyTorch bundles its own libamdhip64.so and loads it by file name; libmkt_hip.so asks for the
    soname.  torch imported FIRST: its copy satisfies the library, one runtime.  The library loaded first: it binds /opt/rocm's
    copy, torch later maps its own as a SECOND runtime, and one of the two then sees no GPU ("No HIP GPUs are available",
    hipErrorNoDevice from mkt_create).  Say so instead."""
    rts = hip_runtimes()
    if len(rts) > 1:
        raise MktError("two HIP runtimes are mapped into this process (" + ", ".join(rts) + "): import torch BEFORE microcket_amd "
                       "(or not at all), so that libmkt_hip.so shares torch's runtime; with two, one of them sees no GPU")


def load_library():
    """Loads libmkt_hip.so (raises if it has not been built: there is no fallback)."""
    global _lib
    if _lib is not None:
        return _lib
    path = lib_path()
    if not os.path.exists(path):
        raise MktError(f"{path} is missing: run `python -m microcket_amd.build` (hipcc, gfx950). No CPU path exists.")
    L = C.CDLL(path)
    if "torch" in sys.modules:
        check_single_hip_runtime()           # torch came first and the library still brought a second runtime: say so now
    L.mkt_strerror.restype = C.c_char_p
    L.mkt_last_error.restype = C.c_char_p
    L.mkt_last_error.argtypes = [C.c_void_p]
    L.mkt_create.argtypes = [C.POINTER(Params), C.POINTER(C.c_void_p)]
    L.mkt_destroy.argtypes = [C.c_void_p]
    L.mkt_destroy.restype = None
    L.mkt_submit.argtypes = [C.c_void_p, C.c_char_p, C.c_size_t, C.c_int]
    L.mkt_drain.argtypes = [C.c_void_p, C.POINTER(Out)]
    L.mkt_drain_wait.argtypes = [C.c_void_p, C.POINTER(Out), C.POINTER(C.c_int)]
    L.mkt_input_window.argtypes = [C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_size_t)]
    L.mkt_submit_window.argtypes = [C.c_void_p, C.c_size_t, C.c_int]
    L.mkt_submit_device.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t]
    L.mkt_sync.argtypes = [C.c_void_p]
    L.mkt_fetch_last_block.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t), C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t)]
    L.mkt_finish.argtypes = [C.c_void_p, C.c_int, C.c_uint64, C.c_uint64, C.POINTER(Stats)]
    L.mkt_format_log.argtypes = [C.POINTER(Stats), C.c_char_p, C.c_size_t]
    L.mkt_get_timing.argtypes = [C.c_void_p, C.POINTER(Timing)]
    L.mkt_reset_timing.argtypes = [C.c_void_p]
    L.mkt_get_replays.argtypes = [C.c_void_p, C.POINTER(_ReplaysC)]
    L.mkt_synth_device.argtypes = [C.c_void_p, C.c_uint64, C.c_int, C.c_int, C.c_int, C.c_int, C.c_uint64, C.c_uint64, C.c_int,
                                   C.POINTER(C.c_void_p), C.POINTER(C.c_size_t)]
    L.mkt_copy_to_host.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t]
    L.mkt_device_text.argtypes = [C.c_void_p, C.c_char_p, C.c_size_t, C.POINTER(C.c_void_p)]
    L.mkt_dataset_create.argtypes = [C.c_void_p, C.c_uint64, C.c_int, C.c_int, C.c_int, C.c_int, C.c_uint64, C.c_uint64, C.c_uint64, C.c_int,
                                     C.POINTER(C.c_void_p)]
    L.mkt_dataset_info.argtypes = [C.c_void_p, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
    L.mkt_dataset_block.argtypes = [C.c_void_p, C.c_uint64, C.POINTER(C.c_void_p), C.POINTER(C.c_size_t), C.POINTER(C.c_uint64)]
    L.mkt_dataset_destroy.argtypes = [C.c_void_p]
    L.mkt_dataset_destroy.restype = None
    L.mkt_reset.argtypes = [C.c_void_p]
    L.mkt_ext_dedup.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.c_void_p, C.c_size_t]
    L.mkt_ext_chrstat.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t)]
    L.mkt_ext_chr_names.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t)]
    L.mkt_ext_keys_fetch.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_size_t, C.POINTER(C.c_uint64)]
    L.mkt_ext_dedup_keys.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.POINTER(C.c_uint64)]
    L.mkt_group_count.argtypes = [C.c_void_p, C.POINTER(C.c_uint64)]
    L.mkt_ext_keys_device.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_void_p), C.POINTER(C.c_uint64)]
    L.mkt_ext_partition.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_uint32, C.c_void_p, C.POINTER(C.c_uint64)]
    L.mkt_ext_dedup_device.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.POINTER(C.c_uint64)]
    L.mkt_ext_unpartition.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.POINTER(C.c_uint64)]
    L.mkt_sorter_create.argtypes = [C.c_int, C.POINTER(C.c_void_p)]
    L.mkt_sorter_destroy.argtypes = [C.c_void_p]
    L.mkt_sorter_destroy.restype = None
    L.mkt_sorter_error.argtypes = [C.c_void_p]
    L.mkt_sorter_error.restype = C.c_char_p
    L.mkt_sorter_add.argtypes = [C.c_void_p, C.c_char_p, C.c_size_t]
    L.mkt_sorter_add_device.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t]
    L.mkt_sorter_sort.argtypes = [C.c_void_p, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
    L.mkt_sorter_fetch.argtypes = [C.c_void_p, C.c_uint64, C.c_void_p, C.c_size_t]
    L.mkt_pairsgz_create.argtypes = [C.c_int, C.POINTER(C.c_void_p)]
    L.mkt_pairsgz_destroy.argtypes = [C.c_void_p]
    L.mkt_pairsgz_destroy.restype = None
    L.mkt_pairsgz_error.argtypes = [C.c_void_p]
    L.mkt_pairsgz_error.restype = C.c_char_p
    L.mkt_pairsgz_add.argtypes = [C.c_void_p, C.c_char_p, C.c_size_t]
    L.mkt_pairsgz_opts_default.argtypes = [C.POINTER(PairsGzOpts)]
    L.mkt_pairsgz_opts_default.restype = None
    L.mkt_pairsgz_run.argtypes = [C.c_void_p, C.POINTER(PairsGzOpts), C.POINTER(_PairsGzInfoC)]
    L.mkt_pairsgz_fetch_gz.argtypes = [C.c_void_p, C.c_uint64, C.c_void_p, C.c_size_t]
    L.mkt_pairsgz_fetch_px2.argtypes = [C.c_void_p, C.c_uint64, C.c_void_p, C.c_size_t]
    L.mkt_pairsgz_timing.argtypes = [C.c_void_p, C.POINTER(C.c_double * 5)]
    L.mkt_bgzf_create.argtypes = [C.c_int, C.POINTER(C.c_void_p)]
    L.mkt_bgzf_destroy.argtypes = [C.c_void_p]
    L.mkt_bgzf_destroy.restype = None
    L.mkt_bgzf_error.argtypes = [C.c_void_p]
    L.mkt_bgzf_error.restype = C.c_char_p
    L.mkt_bgzf_add.argtypes = [C.c_void_p, C.c_char_p, C.c_size_t]
    L.mkt_bgzf_run.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(_BgzfInfoC)]
    L.mkt_bgzf_fetch_text.argtypes = [C.c_void_p, C.c_uint64, C.c_void_p, C.c_size_t]
    L.mkt_bgzf_device_text.argtypes = [C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_uint64)]
    L.mkt_bgzf_load_index.argtypes = [C.c_void_p, C.c_char_p, C.c_size_t]
    L.mkt_bgzf_count.argtypes = [C.c_void_p, C.POINTER(C.c_uint64)]
    L.mkt_bgzf_timing.argtypes = [C.c_void_p, C.POINTER(C.c_double * 5)]
    L.mkt_bgzf_query.argtypes = [C.c_void_p, C.POINTER(C.c_char_p), C.c_uint32, C.POINTER(BgzfQueryOpts), C.POINTER(_BgzfQueryInfoC)]
    L.mkt_bgzf_fetch_query.argtypes = [C.c_void_p, C.c_uint64, C.c_void_p, C.c_size_t]
    L.mkt_bgzf_fetch_query_offsets.argtypes = [C.c_void_p, C.POINTER(C.c_uint64)]
    L.mkt_bgzf_fetch_query_counts.argtypes = [C.c_void_p, C.POINTER(C.c_uint64)]
    L.mkt_bgzf_query_device.argtypes = [C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_uint64)]
    L.mkt_bgzf_names.argtypes = [C.c_void_p, C.c_uint64, C.c_void_p, C.c_size_t, C.POINTER(C.c_uint64)]
    L.mkt_bgzf_clear.argtypes = [C.c_void_p]
    L.mkt_bamtext_create.argtypes = [C.c_int, C.POINTER(C.c_void_p)]
    L.mkt_bamtext_destroy.argtypes = [C.c_void_p]
    L.mkt_bamtext_destroy.restype = None
    L.mkt_bamtext_error.argtypes = [C.c_void_p]
    L.mkt_bamtext_error.restype = C.c_char_p
    L.mkt_bamtext_add.argtypes = [C.c_void_p, C.c_char_p, C.c_size_t]
    L.mkt_bamtext_add_device.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64]
    L.mkt_bamtext_opts_default.argtypes = [C.POINTER(BamTextOpts)]
    L.mkt_bamtext_opts_default.restype = None
    L.mkt_bamtext_run.argtypes = [C.c_void_p, C.POINTER(BamTextOpts), C.POINTER(_BamTextInfoC)]
    L.mkt_bamtext_finish.argtypes = [C.c_void_p, C.POINTER(_BamTextInfoC)]
    L.mkt_bamtext_fetch_header.argtypes = [C.c_void_p, C.c_uint64, C.c_void_p, C.c_size_t, C.POINTER(C.c_uint64)]
    L.mkt_bamtext_fetch_ref.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_size_t, C.POINTER(C.c_int32), C.POINTER(C.c_uint32)]
    L.mkt_bamtext_fetch_text.argtypes = [C.c_void_p, C.c_uint64, C.c_void_p, C.c_size_t]
    L.mkt_bamtext_device_text.argtypes = [C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_uint64)]
    L.mkt_bamtext_timing.argtypes = [C.c_void_p, C.POINTER(C.c_double)]
    L.mkt_paircmp_create.argtypes = [C.c_int, C.POINTER(C.c_void_p)]
    L.mkt_paircmp_destroy.argtypes = [C.c_void_p]
    L.mkt_paircmp_destroy.restype = None
    L.mkt_paircmp_error.argtypes = [C.c_void_p]
    L.mkt_paircmp_error.restype = C.c_char_p
    L.mkt_paircmp_add.argtypes = [C.c_void_p, C.c_int, C.c_char_p, C.c_size_t]
    L.mkt_paircmp_add_device.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_size_t]
    L.mkt_paircmp_opts_default.argtypes = [C.POINTER(PairCompareOpts)]
    L.mkt_paircmp_opts_default.restype = None
    L.mkt_paircmp_run.argtypes = [C.c_void_p, C.POINTER(PairCompareOpts), C.POINTER(_PairCompareInfoC)]
    L.mkt_paircmp_fetch_classes.argtypes = [C.c_void_p, C.c_int, C.c_uint64, C.c_uint64, C.c_void_p]
    L.mkt_paircmp_fetch_lines.argtypes = [C.c_void_p, C.c_uint64, C.c_void_p, C.c_size_t]
    L.mkt_paircmp_report.argtypes = [C.POINTER(_PairCompareInfoC), C.c_uint32, C.c_char_p, C.c_char_p, C.c_void_p, C.c_size_t]
    L.mkt_paircmp_report.restype = C.c_long
    L.mkt_paircmp_timing.argtypes = [C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_double)]
    L.mkt_pairstat_create.argtypes = [C.c_int, C.c_char_p, C.c_size_t, C.POINTER(C.c_void_p)]
    L.mkt_pairstat_destroy.argtypes = [C.c_void_p]
    L.mkt_pairstat_destroy.restype = None
    L.mkt_pairstat_error.argtypes = [C.c_void_p]
    L.mkt_pairstat_error.restype = C.c_char_p
    L.mkt_pairstat_add.argtypes = [C.c_void_p, C.c_char_p, C.c_size_t]
    L.mkt_pairstat_add_device.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t]
    L.mkt_pairstat_add_keys.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_char_p, C.c_size_t]
    L.mkt_pairstat_opts_default.argtypes = [C.POINTER(PairStatsOpts)]
    L.mkt_pairstat_opts_default.restype = None
    L.mkt_pairstat_run.argtypes = [C.c_void_p, C.POINTER(PairStatsOpts), C.POINTER(_PairStatsInfoC)]
    L.mkt_pairstat_fetch_dist.argtypes = [C.c_void_p, C.c_void_p]
    L.mkt_pairstat_fetch_chrom.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p]
    L.mkt_pairstat_fetch_scaling.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    L.mkt_pairstat_text.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_size_t]
    L.mkt_pairstat_text.restype = C.c_long
    L.mkt_pairstat_timing.argtypes = [C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_double)]
    L.mkt_rmdup_create.argtypes = [C.c_int, C.POINTER(C.c_void_p)]
    L.mkt_rmdup_destroy.argtypes = [C.c_void_p]
    L.mkt_rmdup_destroy.restype = None
    L.mkt_rmdup_error.argtypes = [C.c_void_p]
    L.mkt_rmdup_error.restype = C.c_char_p
    L.mkt_rmdup_add.argtypes = [C.c_void_p, C.c_char_p, C.c_size_t]
    L.mkt_rmdup_run.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_int, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
    L.mkt_rmdup_fetch.argtypes = [C.c_void_p, C.c_int, C.c_uint64, C.c_void_p, C.c_size_t]
    L.mkt_rmdup_begin.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_int]
    L.mkt_rmdup_push.argtypes = [C.c_void_p, C.c_char_p, C.c_size_t, C.c_int, C.POINTER(C.c_uint64)]
    L.mkt_rmdup_stats.argtypes = [C.c_void_p, C.POINTER(C.c_uint64)]
    L.mkt_stitch_create.argtypes = [C.c_int, C.POINTER(C.c_void_p)]
    L.mkt_stitch_destroy.argtypes = [C.c_void_p]
    L.mkt_stitch_destroy.restype = None
    L.mkt_stitch_error.argtypes = [C.c_void_p]
    L.mkt_stitch_error.restype = C.c_char_p
    L.mkt_stitch_check.argtypes = [C.c_uint32, C.c_uint32, C.c_double, C.c_uint32, C.c_uint32, C.c_uint32, C.c_char_p, C.c_size_t]
    L.mkt_stitch_segment_pairs.argtypes = [C.c_void_p, C.c_uint64]
    L.mkt_stitch_begin.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_double, C.c_uint32, C.c_uint32, C.c_uint32]
    L.mkt_stitch_push.argtypes = [C.c_void_p, C.c_char_p, C.c_size_t, C.c_int, C.POINTER(C.c_uint64)]
    L.mkt_stitch_fetch.argtypes = [C.c_void_p, C.c_int, C.c_uint64, C.c_void_p, C.c_size_t]
    L.mkt_stitch_stats.argtypes = [C.c_void_p, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
    L.mkt_stitch_timing.argtypes = [C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_double)]
    L.mkt_trim_default_opts.argtypes = [C.POINTER(TrimOpts)]
    L.mkt_trim_default_opts.restype = None
    L.mkt_trim_create.argtypes = [C.c_int, C.POINTER(C.c_void_p)]
    L.mkt_trim_destroy.argtypes = [C.c_void_p]
    L.mkt_trim_destroy.restype = None
    L.mkt_trim_error.argtypes = [C.c_void_p]
    L.mkt_trim_error.restype = C.c_char_p
    L.mkt_trim_check.argtypes = [C.POINTER(TrimOpts), C.c_char_p, C.c_size_t]
    L.mkt_trim_segment_pairs.argtypes = [C.c_void_p, C.c_uint64]
    L.mkt_trim_begin.argtypes = [C.c_void_p, C.POINTER(TrimOpts)]
    L.mkt_trim_push.argtypes = [C.c_void_p, C.c_char_p, C.c_size_t, C.c_char_p, C.c_size_t, C.c_int, C.POINTER(C.c_uint64)]
    L.mkt_trim_fetch.argtypes = [C.c_void_p, C.c_int, C.c_uint64, C.c_void_p, C.c_size_t]
    L.mkt_trim_stats.argtypes = [C.c_void_p] + [C.POINTER(C.c_uint64)] * 6
    L.mkt_trim_timing.argtypes = [C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_double)]
    L.mkt_bam_create.argtypes = [C.c_int, C.POINTER(C.c_void_p)]
    L.mkt_bam_destroy.argtypes = [C.c_void_p]
    L.mkt_bam_destroy.restype = None
    L.mkt_bam_error.argtypes = [C.c_void_p]
    L.mkt_bam_error.restype = C.c_char_p
    L.mkt_bam_note.argtypes = [C.c_void_p]
    L.mkt_bam_note.restype = C.c_char_p
    L.mkt_bam_add.argtypes = [C.c_void_p, C.c_char_p, C.c_size_t]
    L.mkt_bam_add_device.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t]
    L.mkt_bam_run.argtypes = [C.c_void_p, C.c_int, C.c_int, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
    L.mkt_bam_fetch.argtypes = [C.c_void_p, C.c_int, C.c_uint64, C.c_void_p, C.c_size_t]
    L.mkt_bam_reserve.argtypes = [C.c_void_p, C.c_size_t]
    L.mkt_bam_window.argtypes = [C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_size_t)]
    L.mkt_bam_commit.argtypes = [C.c_void_p, C.c_size_t]
    L.mkt_bam_read.argtypes = [C.c_void_p, C.c_int, C.c_uint64, C.c_size_t, C.POINTER(C.c_void_p)]
    L.mkt_bam_spill.argtypes = [C.c_void_p, C.c_uint64, C.c_char_p, C.c_int, C.c_int]
    L.mkt_bam_pull.argtypes = [C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_size_t)]
    L.mkt_bam_stats.argtypes = [C.c_void_p, C.POINTER(C.c_uint64)]
    L.mkt_matrix_create.argtypes = [C.c_int, C.c_char_p, C.c_size_t, C.POINTER(C.c_uint32), C.c_uint32, C.POINTER(C.c_void_p)]
    L.mkt_matrix_destroy.argtypes = [C.c_void_p]
    L.mkt_matrix_destroy.restype = None
    L.mkt_matrix_error.argtypes = [C.c_void_p]
    L.mkt_matrix_error.restype = C.c_char_p
    L.mkt_matrix_add.argtypes = [C.c_void_p, C.c_char_p, C.c_size_t]
    L.mkt_matrix_add_device.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t]
    L.mkt_matrix_add_keys.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_char_p, C.c_size_t]
    L.mkt_matrix_run.argtypes = [C.c_void_p, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
    L.mkt_matrix_info.argtypes = [C.c_void_p, C.c_uint32, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
    L.mkt_matrix_fetch.argtypes = [C.c_void_p, C.c_uint32, C.c_uint64, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p]
    L.mkt_matrix_fetch_text.argtypes = [C.c_void_p, C.c_uint32, C.c_uint64, C.c_void_p, C.c_size_t]
    L.mkt_matrix_timing.argtypes = [C.c_void_p, C.c_uint32, C.POINTER(C.c_double)]
    L.mkt_balance_opts_default.argtypes = [C.POINTER(BalanceOpts)]
    L.mkt_balance_opts_default.restype = None
    L.mkt_matrix_balance.argtypes = [C.c_void_p, C.c_uint32, C.POINTER(BalanceOpts), C.POINTER(_BalanceStatsC)]
    L.mkt_matrix_fetch_weights.argtypes = [C.c_void_p, C.c_uint32, C.c_uint64, C.c_uint64, C.c_void_p]
    L.mkt_matrix_balance_timing.argtypes = [C.c_void_p, C.c_uint32, C.POINTER(C.c_double), C.POINTER(C.c_double)]
    L.mkt_expected_opts_default.argtypes = [C.POINTER(ExpectedOpts)]
    L.mkt_expected_opts_default.restype = None
    L.mkt_matrix_expected.argtypes = [C.c_void_p, C.c_uint32, C.POINTER(ExpectedOpts), C.POINTER(_ExpectedInfoC)]
    L.mkt_matrix_fetch_expected_cis.argtypes = [C.c_void_p, C.c_uint32, C.c_uint64, C.c_uint64] + [C.c_void_p] * 3
    L.mkt_matrix_fetch_expected_trans.argtypes = [C.c_void_p, C.c_uint32, C.c_uint64, C.c_uint64] + [C.c_void_p] * 4
    L.mkt_matrix_fetch_expected_genome.argtypes = [C.c_void_p, C.c_uint32, C.c_uint64, C.c_uint64] + [C.c_void_p] * 5
    L.mkt_matrix_fetch_values.argtypes = [C.c_void_p, C.c_uint32, C.c_int, C.c_uint64, C.c_uint64, C.c_void_p]
    L.mkt_matrix_expected_timing.argtypes = [C.c_void_p, C.c_uint32, C.POINTER(C.c_double), C.POINTER(C.c_double)]
    L.mkt_loops_opts_default.argtypes = [C.POINTER(LoopsOpts)]
    L.mkt_loops_opts_default.restype = None
    L.mkt_matrix_loops.argtypes = [C.c_void_p, C.c_uint32, C.POINTER(LoopsOpts), C.POINTER(_LoopsInfoC)]
    L.mkt_matrix_fetch_loop_cells.argtypes = [C.c_void_p, C.c_uint32, C.c_uint64, C.c_uint64] + [C.c_void_p] * 10
    L.mkt_matrix_fetch_loop_hist.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p]
    L.mkt_matrix_fetch_loop_thresholds.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p]
    L.mkt_matrix_fetch_loops.argtypes = [C.c_void_p, C.c_uint32, C.c_uint64, C.c_uint64, C.c_void_p]
    L.mkt_matrix_loops_timing.argtypes = [C.c_void_p, C.c_uint32] + [C.POINTER(C.c_double)] * 3
    L.mkt_eigs_opts_default.argtypes = [C.POINTER(EigsOpts)]
    L.mkt_eigs_opts_default.restype = None
    L.mkt_matrix_eigs.argtypes = [C.c_void_p, C.c_uint32, C.POINTER(EigsOpts), C.c_void_p, C.POINTER(_EigsInfoC)]
    L.mkt_matrix_fetch_eigvecs.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint64, C.c_uint64, C.c_void_p]
    L.mkt_matrix_fetch_eigvals.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32] + [C.c_void_p] * 5
    L.mkt_matrix_eigs_apply.argtypes = [C.c_void_p, C.c_uint32, C.POINTER(EigsOpts), C.c_void_p, C.c_uint32, C.c_void_p]
    L.mkt_matrix_eigs_timing.argtypes = [C.c_void_p, C.c_uint32] + [C.POINTER(C.c_double)] * 3
    L.mkt_insulation_opts_default.argtypes = [C.POINTER(InsulationOpts)]
    L.mkt_insulation_opts_default.restype = None
    L.mkt_matrix_insulation.argtypes = [C.c_void_p, C.c_uint32, C.POINTER(InsulationOpts), C.POINTER(_InsulationInfoC)]
    L.mkt_matrix_fetch_insulation.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint64, C.c_uint64] + [C.c_void_p] * 7
    L.mkt_matrix_insulation_timing.argtypes = [C.c_void_p, C.c_uint32, C.POINTER(C.c_double), C.POINTER(C.c_double)]
    L.mkt_pileup_opts_default.argtypes = [C.POINTER(PileupOpts)]
    L.mkt_pileup_opts_default.restype = None
    L.mkt_matrix_pileup.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_uint64, C.POINTER(PileupOpts), C.POINTER(_PileupInfoC)]
    L.mkt_matrix_fetch_pileup.argtypes = [C.c_void_p, C.c_uint32] + [C.c_void_p] * 4
    L.mkt_matrix_fetch_pileup_status.argtypes = [C.c_void_p, C.c_uint32, C.c_uint64, C.c_uint64, C.c_void_p]
    L.mkt_matrix_pileup_timing.argtypes = [C.c_void_p, C.c_uint32, C.POINTER(C.c_double), C.POINTER(C.c_double)]
    L.mkt_saddle_opts_default.argtypes = [C.POINTER(SaddleOpts)]
    L.mkt_saddle_opts_default.restype = None
    L.mkt_matrix_saddle.argtypes = [C.c_void_p, C.c_uint32, C.POINTER(SaddleOpts), C.c_void_p, C.POINTER(_SaddleInfoC)]
    L.mkt_matrix_fetch_saddle.argtypes = [C.c_void_p, C.c_uint32] + [C.c_void_p] * 5
    L.mkt_matrix_fetch_saddle_groups.argtypes = [C.c_void_p, C.c_uint32, C.c_uint64, C.c_uint64, C.c_void_p]
    L.mkt_matrix_fetch_saddle_edges.argtypes = [C.c_void_p, C.c_uint32] + [C.c_void_p] * 3
    L.mkt_matrix_fetch_saddle_profile.argtypes = [C.c_void_p, C.c_uint32] + [C.c_void_p] * 3
    L.mkt_matrix_saddle_timing.argtypes = [C.c_void_p, C.c_uint32, C.POINTER(C.c_double), C.POINTER(C.c_double)]
    L.mkt_scc_opts_default.argtypes = [C.POINTER(SccOpts)]
    L.mkt_scc_opts_default.restype = None
    L.mkt_matrix_scc.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.POINTER(SccOpts), C.POINTER(_SccInfoC)]
    L.mkt_matrix_fetch_scc_strata.argtypes = [C.c_void_p, C.c_uint32, C.c_uint64, C.c_uint64] + [C.c_void_p] * 9
    L.mkt_matrix_fetch_scc_chrom.argtypes = [C.c_void_p, C.c_uint32, C.c_uint64, C.c_uint64] + [C.c_void_p] * 4
    L.mkt_matrix_scc_timing.argtypes = [C.c_void_p, C.c_uint32, C.POINTER(C.c_double), C.POINTER(C.c_double)]
    L.mkt_viewpoint_opts_default.argtypes = [C.POINTER(ViewpointOpts)]
    L.mkt_viewpoint_opts_default.restype = None
    L.mkt_matrix_viewpoint.argtypes = [C.c_void_p, C.POINTER(ViewpointOpts), C.POINTER(_ViewpointInfoC)]
    L.mkt_matrix_fetch_viewpoint_links.argtypes = [C.c_void_p, C.c_uint64, C.c_uint64] + [C.c_void_p] * 4
    L.mkt_matrix_fetch_viewpoint_track.argtypes = [C.c_void_p, C.c_uint64, C.c_uint64, C.c_void_p]
    L.mkt_matrix_fetch_viewpoint_partners.argtypes = [C.c_void_p, C.c_uint64, C.c_uint64] + [C.c_void_p] * 3
    L.mkt_matrix_viewpoint_timing.argtypes = [C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_double)]
    L.mkt_hic_opts_default.argtypes = [C.POINTER(HicOpts)]
    L.mkt_hic_opts_default.restype = None
    L.mkt_matrix_hic.argtypes = [C.c_void_p, C.POINTER(HicOpts), C.POINTER(_HicInfoC)]
    L.mkt_matrix_fetch_hic.argtypes = [C.c_void_p, C.c_uint64, C.c_void_p, C.c_size_t]
    L.mkt_matrix_hic_timing.argtypes = [C.c_void_p, C.c_uint32] + [C.POINTER(C.c_double)] * 4
    _lib = L
    return L


def device_count():
    return int(load_library().mkt_device_count())


class Context:
    """One GPU context = one input stream (mirrors one bin/sam2pairs process of the reference)."""

    def __init__(self, mode, ratio=0.5, min_mapq=10, write_sam=True, ref_threads=4, device=0, block_bytes=0, tiles=TILES_AUTO,
                 ordered=False, extensions=0):
        self.L = load_library()
        if isinstance(mode, str):
            mode = {"flash": MODE_FLASH, "unc": MODE_UNC}[mode]
        self.params = Params(mode, ratio, min_mapq, 1 if write_sam else 0, ref_threads, device, block_bytes, tiles, 1 if ordered else 0, extensions, 0)
        self.h = C.c_void_p()
        rc = self.L.mkt_create(C.byref(self.params), C.byref(self.h))
        if rc != 0:
            hint = ""
            if len(hip_runtimes()) > 1:      # (this package loaded before torch: the usual reason for "no device" on a GPU box)
                hint = " [two HIP runtimes are mapped into this process (" + ", ".join(hip_runtimes()) + "): import torch BEFORE microcket_amd]"
            raise MktError(f"mkt_create: {self.L.mkt_strerror(rc).decode()}: {self.L.mkt_last_error(None).decode()}{hint}")

    def _chk(self, rc, what):
        if rc != 0:
            raise MktError(f"{what}: {self.L.mkt_strerror(rc).decode()}: {self.L.mkt_last_error(self.h).decode()}")

    def close(self):
        if self.h:
            self.L.mkt_destroy(self.h)
            self.h = C.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    # ---- streaming path
    def submit(self, data: bytes, last=False):
        self._chk(self.L.mkt_submit(self.h, data, len(data), 1 if last else 0), "mkt_submit")

    def drain(self):
        o = Out()
        self._chk(self.L.mkt_drain(self.h, C.byref(o)), "mkt_drain")
        pairs = C.string_at(o.pairs, o.pairs_len) if o.pairs_len else b""
        sam = C.string_at(o.sam, o.sam_len) if o.sam_len else b""
        return pairs, sam

    def finish(self, drop_last=True, group_offset=0, total_groups=0):
        st = Stats()
        self._chk(self.L.mkt_finish(self.h, 1 if drop_last else 0, group_offset, total_groups, C.byref(st)), "mkt_finish")
        return st

    def format_log(self, st):
        buf = C.create_string_buffer(512)
        self.L.mkt_format_log(C.byref(st), buf, 512)
        return buf.value

    def run_bytes(self, text: bytes, chunk=0):
        """Whole input -> (pairs, sam, stats, log)."""
        pairs, sam = [], []
        if chunk <= 0:
            chunk = max(len(text), 1)
        pos = 0
        while True:
            part = text[pos:pos + chunk]
            pos += len(part)
            last = pos >= len(text)
            self.submit(part, last)
            a, b = self.drain()
            pairs.append(a)
            sam.append(b)
            if last:
                break
        st = self.finish(True)
        a, b = self.drain()
        pairs.append(a)
        sam.append(b)
        return b"".join(pairs), b"".join(sam), st, self.format_log(st)

    def run_bytes_window(self, text: bytes, piece=0):
        """The same through the zero-copy input window (mkt_input_window / mkt_submit_window), `piece` bytes per commit."""
        pairs, sam = [], []
        pos = 0
        while True:
            buf, cap = C.c_void_p(), C.c_size_t()
            self._chk(self.L.mkt_input_window(self.h, C.byref(buf), C.byref(cap)), "mkt_input_window")
            take = min(cap.value, len(text) - pos, piece if piece > 0 else cap.value)
            if take:
                C.memmove(buf.value, text[pos:pos + take], take)
            pos += take
            last = pos >= len(text)
            self._chk(self.L.mkt_submit_window(self.h, C.c_size_t(take), 1 if last else 0), "mkt_submit_window")
            a, b = self.drain()
            pairs.append(a)
            sam.append(b)
            if last:
                break
        st = self.finish(True)
        a, b = self.drain()
        pairs.append(a)
        sam.append(b)
        return b"".join(pairs), b"".join(sam), st, self.format_log(st)

    # ---- resident path
    def synth_device(self, seed, profile, n_groups, first_group=0, genome=0, read_len=150, lanes=1, tail_group=False):
        p = C.c_void_p()
        n = C.c_size_t()
        self._chk(self.L.mkt_synth_device(self.h, seed, profile, genome, read_len, lanes, first_group, n_groups, 1 if tail_group else 0,
                                          C.byref(p), C.byref(n)), "mkt_synth_device")
        return p.value, n.value

    def submit_device(self, d_ptr, n):
        self._chk(self.L.mkt_submit_device(self.h, C.c_void_p(d_ptr), n), "mkt_submit_device")

    def sync(self):
        self._chk(self.L.mkt_sync(self.h), "mkt_sync")

    def fetch_last_block(self):
        np_, ns_ = C.c_size_t(), C.c_size_t()
        self._chk(self.L.mkt_fetch_last_block(self.h, None, 0, C.byref(np_), None, 0, C.byref(ns_)), "mkt_fetch_last_block")
        pb = C.create_string_buffer(max(np_.value, 1))
        sb = C.create_string_buffer(max(ns_.value, 1))
        self._chk(self.L.mkt_fetch_last_block(self.h, pb, np_.value, C.byref(np_), sb, ns_.value, C.byref(ns_)), "mkt_fetch_last_block")
        return pb.raw[:np_.value], sb.raw[:ns_.value]

    def fetch_last_block_np(self):
        """the same as numpy uint8 arrays (no extra copies: the blocks of the bench are 100 MB of .pairs)"""
        import numpy as np
        np_, ns_ = C.c_size_t(), C.c_size_t()
        self._chk(self.L.mkt_fetch_last_block(self.h, None, 0, C.byref(np_), None, 0, C.byref(ns_)), "mkt_fetch_last_block")
        pb = np.empty(max(np_.value, 1), dtype=np.uint8)
        sb = np.empty(max(ns_.value, 1), dtype=np.uint8)
        self._chk(self.L.mkt_fetch_last_block(self.h, pb.ctypes.data_as(C.c_void_p), np_.value, C.byref(np_), sb.ctypes.data_as(C.c_void_p), ns_.value, C.byref(ns_)),
                  "mkt_fetch_last_block")
        return pb[:np_.value], sb[:ns_.value]

    def copy_to_host_np(self, d_ptr, n):
        import numpy as np
        buf = np.empty(max(n, 1), dtype=np.uint8)
        self._chk(self.L.mkt_copy_to_host(self.h, C.c_void_p(d_ptr), buf.ctypes.data_as(C.c_void_p), n), "mkt_copy_to_host")
        return buf[:n]

    def copy_to_host(self, d_ptr, n):
        buf = C.create_string_buffer(max(n, 1))
        self._chk(self.L.mkt_copy_to_host(self.h, C.c_void_p(d_ptr), buf, n), "mkt_copy_to_host")
        return buf.raw[:n]

    def device_text(self, data: bytes):
        """host text -> device buffer owned by the context; returns the device pointer (a block for submit_device)"""
        p = C.c_void_p()
        self._chk(self.L.mkt_device_text(self.h, data, len(data), C.byref(p)), "mkt_device_text")
        return p.value

    def reset(self):
        self._chk(self.L.mkt_reset(self.h), "mkt_reset")

    def ext_dedup(self, drop_last=True, want_flags=True):
        """(total reported pairs, duplicates, flags bytes in input order)"""
        tot, dup = C.c_uint64(), C.c_uint64()
        self._chk(self.L.mkt_ext_dedup(self.h, 1 if drop_last else 0, C.byref(tot), C.byref(dup), None, 0), "mkt_ext_dedup")
        if not want_flags or tot.value == 0:
            return tot.value, dup.value, b""
        buf = C.create_string_buffer(tot.value)
        self._chk(self.L.mkt_ext_dedup(self.h, 1 if drop_last else 0, C.byref(tot), C.byref(dup), buf, tot.value), "mkt_ext_dedup")
        return tot.value, dup.value, buf.raw[:tot.value]

    def ext_chr_names(self):
        """{slot: name} of this context's chromosome-name table"""
        n = C.c_size_t()
        self._chk(self.L.mkt_ext_chr_names(self.h, None, 0, C.byref(n)), "mkt_ext_chr_names")
        buf = C.create_string_buffer(max(n.value, 1))
        self._chk(self.L.mkt_ext_chr_names(self.h, buf, n.value, C.byref(n)), "mkt_ext_chr_names")
        out = {}
        for line in buf.raw[:n.value].split(b"\n"):
            if line:
                s, name = line.split(b"\t", 1)
                out[int(s)] = name
        return out

    def ext_keys_fetch(self, drop_last=True):
        """key records as a numpy uint64 array of shape (n, 3): k0, k1, ordinal (input order)"""
        import numpy as np
        n = C.c_uint64()
        self._chk(self.L.mkt_ext_keys_fetch(self.h, 1 if drop_last else 0, None, 0, C.byref(n)), "mkt_ext_keys_fetch")
        arr = np.zeros((n.value, 3), dtype=np.uint64)
        if n.value:
            self._chk(self.L.mkt_ext_keys_fetch(self.h, 1 if drop_last else 0, arr.ctypes.data_as(C.c_void_p), arr.nbytes, C.byref(n)), "mkt_ext_keys_fetch")
        return arr

    def ext_dedup_keys(self, keys):
        """duplicate flags (numpy uint8) for a (n, 3) uint64 key array in input order; runs on this context's GPU"""
        import numpy as np
        keys = np.ascontiguousarray(keys, dtype=np.uint64)
        n = keys.shape[0]
        flags = np.zeros(n, dtype=np.uint8)
        dups = C.c_uint64()
        if n:
            self._chk(self.L.mkt_ext_dedup_keys(self.h, keys.ctypes.data_as(C.c_void_p), n, flags.ctypes.data_as(C.c_void_p), C.byref(dups)), "mkt_ext_dedup_keys")
        return flags, dups.value

    # ---- sharded duplicate marking: the device side of microcket_amd.shard.dedup_exchange (torch tensors carry the buffers)
    def ext_key_count(self, drop_last=True):
        p, n = C.c_void_p(), C.c_uint64()
        self._chk(self.L.mkt_ext_keys_device(self.h, 1 if drop_last else 0, C.byref(p), C.byref(n)), "mkt_ext_keys_device")
        return n.value

    def ext_partition(self, drop_last, lut, world, torch, device):
        """Key records grouped by destination rank (stable) in a uint8 device tensor of 24 n bytes; returns (tensor, counts)."""
        import numpy as np
        n = self.ext_key_count(drop_last)
        send = torch.empty(max(n, 1) * KEY_BYTES, dtype=torch.uint8, device=device)
        counts = (C.c_uint64 * 16)()
        lut = None if lut is None else np.ascontiguousarray(lut, dtype=np.uint16)
        assert lut is None or lut.shape[0] == 8192
        self._chk(self.L.mkt_ext_partition(self.h, 1 if drop_last else 0, None if lut is None else lut.ctypes.data_as(C.c_void_p), world,
                                           C.c_void_p(send.data_ptr()), counts), "mkt_ext_partition")
        return send[:n * KEY_BYTES], [int(counts[r]) for r in range(world)]

    def ext_dedup_tensor(self, recv, torch):
        """Duplicate flags (uint8 device tensor) for the key records lying in the uint8 device tensor recv, first in buffer order wins."""
        n = recv.numel() // KEY_BYTES
        flags = torch.zeros(max(n, 1), dtype=torch.uint8, device=recv.device)
        dups = C.c_uint64()
        if n:
            self._chk(self.L.mkt_ext_dedup_device(self.h, C.c_void_p(recv.data_ptr()), n, C.c_void_p(flags.data_ptr()), C.byref(dups)), "mkt_ext_dedup_device")
        return flags[:n], dups.value

    def ext_unpartition(self, flags_part, want_flags=True):
        """Flags that came back in ext_partition's order -> input order (bytes) and the number of duplicates among this context's pairs."""
        n = flags_part.numel()
        dups = C.c_uint64()
        buf = C.create_string_buffer(max(n, 1)) if want_flags else None
        self._chk(self.L.mkt_ext_unpartition(self.h, C.c_void_p(flags_part.data_ptr()) if n else None, buf, n if want_flags else 0, C.byref(dups)), "mkt_ext_unpartition")
        return (buf.raw[:n] if want_flags else b""), dups.value

    def ext_chrstat(self, drop_last=True):
        n = C.c_size_t()
        cap = 1 << 20                          # one call in the usual case (the table is a few KB)
        buf = C.create_string_buffer(cap)
        rc = self.L.mkt_ext_chrstat(self.h, 1 if drop_last else 0, buf, cap, C.byref(n))
        if rc != 0 and n.value > cap:          # too small: *len holds the size needed
            buf = C.create_string_buffer(n.value)
            rc = self.L.mkt_ext_chrstat(self.h, 1 if drop_last else 0, buf, n.value, C.byref(n))
        self._chk(rc, "mkt_ext_chrstat")
        return buf.raw[:n.value]

    def group_count(self):
        g = C.c_uint64()
        self._chk(self.L.mkt_group_count(self.h, C.byref(g)), "mkt_group_count")
        return g.value

    def dataset(self, seed, profile, n_groups, groups_per_block, first_group=0, genome=0, read_len=150, lanes=1, tail_group=False):
        return Dataset(self, seed, profile, n_groups, groups_per_block, first_group, genome, read_len, lanes, tail_group)

    def timing(self):
        t = Timing()
        self._chk(self.L.mkt_get_timing(self.h, C.byref(t)), "mkt_get_timing")
        return t

    def reset_timing(self):
        self._chk(self.L.mkt_reset_timing(self.h), "mkt_reset_timing")

    def replays(self):
        """Replays(geometry, pairs_cap, sam_cap, sc_cap, jobs_rerun): repairs by cause and blocks run again since reset_timing()"""
        r = _ReplaysC()
        self._chk(self.L.mkt_get_replays(self.h, C.byref(r)), "mkt_get_replays")
        return Replays(*[getattr(r, k) for k in Replays._fields])


class Dataset:
    """Synthetic SAM resident in HBM, cut into group-aligned blocks (see mkt_dataset_create)."""

    def __init__(self, ctx, seed, profile, n_groups, groups_per_block, first_group, genome, read_len, lanes, tail_group):
        self.ctx = ctx
        self.h = C.c_void_p()
        ctx._chk(ctx.L.mkt_dataset_create(ctx.h, seed, profile, genome, read_len, lanes, first_group, n_groups, groups_per_block,
                                          1 if tail_group else 0, C.byref(self.h)), "mkt_dataset_create")
        nb, tb, tg = C.c_uint64(), C.c_uint64(), C.c_uint64()
        ctx.L.mkt_dataset_info(self.h, C.byref(nb), C.byref(tb), C.byref(tg))
        self.n_blocks, self.total_bytes, self.total_groups = nb.value, tb.value, tg.value
        self.blocks = []
        for i in range(self.n_blocks):
            p, n, g = C.c_void_p(), C.c_size_t(), C.c_uint64()
            ctx.L.mkt_dataset_block(self.h, i, C.byref(p), C.byref(n), C.byref(g))
            self.blocks.append((p.value, n.value, g.value))

    def close(self):
        if self.h:
            self.ctx.L.mkt_dataset_destroy(self.h)
            self.h = C.c_void_p()


class PairsSorter:
    """.pairs text in the driver's order (LANG=C sort -k2,2d -k4,4d -k3,3n -k5,5n) on the GPU: see mkt_sorter_* in include/mkt.h."""

    def __init__(self, device=0):
        self.L = load_library()
        self.h = C.c_void_p()
        rc = self.L.mkt_sorter_create(device, C.byref(self.h))
        if rc != 0:
            raise MktError(f"mkt_sorter_create: {self.L.mkt_strerror(rc).decode()}")

    def _chk(self, rc, what):
        if rc != 0:
            raise MktError(f"{what}: {self.L.mkt_strerror(rc).decode()}: {self.L.mkt_sorter_error(self.h).decode()}")

    def add(self, data: bytes):
        self._chk(self.L.mkt_sorter_add(self.h, data, len(data)), "mkt_sorter_add")

    def add_device(self, d_ptr, n):
        self._chk(self.L.mkt_sorter_add_device(self.h, C.c_void_p(d_ptr), n), "mkt_sorter_add_device")

    def sort(self):
        """Sorts what was added; returns the sorted text."""
        lines, nbytes = C.c_uint64(), C.c_uint64()
        self._chk(self.L.mkt_sorter_sort(self.h, C.byref(lines), C.byref(nbytes)), "mkt_sorter_sort")
        self.lines = lines.value
        buf = C.create_string_buffer(max(nbytes.value, 1))
        self._chk(self.L.mkt_sorter_fetch(self.h, 0, buf, nbytes.value), "mkt_sorter_fetch")
        return buf.raw[:nbytes.value]

    def close(self):
        if self.h:
            self.L.mkt_sorter_destroy(self.h)
            self.h = C.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()


class PairsGz:
    """final.pairs.gz (BGZF) and its pairix index .px2 from a sorted .pairs text on the GPU (the driver's bgzip | pairix tail): see
    mkt_pairsgz_* in include/mkt.h, where the definition stands."""

    def __init__(self, device=0):
        self.L = load_library()
        self.h = C.c_void_p()
        self.info = None
        rc = self.L.mkt_pairsgz_create(device, C.byref(self.h))
        if rc != 0:
            raise MktError(f"mkt_pairsgz_create: {self.L.mkt_strerror(rc).decode()}")

    def _chk(self, rc, what):
        if rc != 0:
            raise MktError(f"{what}: {self.L.mkt_strerror(rc).decode()}: {self.L.mkt_pairsgz_error(self.h).decode()}")

    def add(self, data: bytes):
        """A piece of the text; it need not end at a line end."""
        self._chk(self.L.mkt_pairsgz_add(self.h, data, len(data)), "mkt_pairsgz_add")
        self.info = None

    def run(self, level=1):
        """Compresses and indexes what was added; returns the counters (also kept in .info).  A text that is refused (unsorted, a pair
        that reappears, a malformed line) raises MktError with "line N:" in its message and leaves nothing to fetch."""
        o = PairsGzOpts()
        self.L.mkt_pairsgz_opts_default(C.byref(o))
        o.level = level
        info = _PairsGzInfoC()
        self.info = None
        self._chk(self.L.mkt_pairsgz_run(self.h, C.byref(o), C.byref(info)), "mkt_pairsgz_run")
        self.info = PairsGzInfo(*(int(getattr(info, k)) for k in PairsGzInfo._fields))
        return self.info

    def _fetch(self, fn, what, n):
        buf = C.create_string_buffer(max(n, 1))
        self._chk(fn(self.h, 0, buf, n), what)
        return buf.raw[:n]

    def gz_bytes(self):
        if self.info is None:
            raise MktError("gz_bytes before a run that succeeded")
        return self._fetch(self.L.mkt_pairsgz_fetch_gz, "mkt_pairsgz_fetch_gz", self.info.gz_bytes)

    def px2_bytes(self):
        if self.info is None:
            raise MktError("px2_bytes before a run that succeeded")
        return self._fetch(self.L.mkt_pairsgz_fetch_px2, "mkt_pairsgz_fetch_px2", self.info.px2_bytes)

    def write(self, path):
        """Writes `path` and `path + ".px2"`."""
        gz, px2 = self.gz_bytes(), self.px2_bytes()
        with open(path, "wb") as f:
            f.write(gz)
        with open(os.fspath(path) + ".px2", "wb") as f:
            f.write(px2)

    def timing_ms(self):
        t = (C.c_double * 5)()
        self._chk(self.L.mkt_pairsgz_timing(self.h, C.byref(t)), "mkt_pairsgz_timing")
        return dict(zip(("deflate", "line_index", "lines", "names_chunks", "index"), (float(x) for x in t)))

    def close(self):
        if self.h:
            self.L.mkt_pairsgz_destroy(self.h)
            self.h = C.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()


class BgzfRefused(MktError):
    """A BGZF file the reader refuses: .reason is the key of the reason (e.g. "crc", "ll_oversubscribed"; the list stands in
    csrc/mkt_inflate.h), .offset the file offset of the refused block."""

    def __init__(self, msg, reason, offset):
        MktError.__init__(self, msg)
        self.reason = reason
        self.offset = offset


class BgzfReader:
    """A BGZF file (final.pairs.gz, its .px2, a BAM as bytes) inflated on the GPU: see mkt_bgzf_* in include/mkt.h, where the
    definition and the limits stand (resident only, BGZF only).  With the file's .px2 loaded, `query` answers regions the way
    `pairix file.pairs.gz REGION ...` prints them: without a `run` only the blocks the index points to are inflated, after a `run` the
    resident text is used; the bytes are the same."""

    def __init__(self, device=0):
        self.L = load_library()
        self.h = C.c_void_p()
        self.info = None
        self.query_info = None
        rc = self.L.mkt_bgzf_create(device, C.byref(self.h))
        if rc != 0:
            raise MktError(f"mkt_bgzf_create: {self.L.mkt_strerror(rc).decode()}")

    def _chk(self, rc, what):
        if rc != 0:
            raise MktError(f"{what}: {self.L.mkt_strerror(rc).decode()}: {self.L.mkt_bgzf_error(self.h).decode()}")

    def add(self, data: bytes):
        """A piece of the compressed file, cut anywhere."""
        self._chk(self.L.mkt_bgzf_add(self.h, data, len(data)), "mkt_bgzf_add")
        self.info = None

    def run(self):
        """Inflates what was added and checks every CRC-32 and ISIZE; returns the counters (also kept in .info).  A refused file
        raises BgzfRefused with the reason and the block's offset and leaves no text."""
        info = _BgzfInfoC()
        self.info = None
        rc = self.L.mkt_bgzf_run(self.h, None, C.byref(info))
        if rc == -9:
            msg = self.L.mkt_bgzf_error(self.h).decode()
            raise BgzfRefused(f"mkt_bgzf_run: {msg}", msg[msg.rfind("[") + 1:msg.rfind("]")], int(info.bad_offset))
        self._chk(rc, "mkt_bgzf_run")
        self.info = BgzfInfo(*(int(getattr(info, k)) for k in BgzfInfo._fields))
        return self.info

    def text(self):
        if self.info is None:
            raise MktError("text before a run that succeeded")
        n = self.info.text_bytes
        buf = C.create_string_buffer(max(n, 1))
        self._chk(self.L.mkt_bgzf_fetch_text(self.h, 0, buf, n), "mkt_bgzf_fetch_text")
        return buf.raw[:n]

    def device_text(self):
        """(device pointer, bytes) of the text: what PairCompare.add_device and Matrix.add_device take; valid until the next add, run or close."""
        d, n = C.c_void_p(), C.c_uint64()
        self._chk(self.L.mkt_bgzf_device_text(self.h, C.byref(d), C.byref(n)), "mkt_bgzf_device_text")
        return d.value or 0, int(n.value)

    def load_index(self, px2: bytes):
        """The bytes of the file's .px2 (inflated by the same kernel and checked field by field)."""
        self._chk(self.L.mkt_bgzf_load_index(self.h, px2, len(px2)), "mkt_bgzf_load_index")

    def count(self):
        """`pairix -n`: the line count the loaded index records."""
        n = C.c_uint64()
        self._chk(self.L.mkt_bgzf_count(self.h, C.byref(n)), "mkt_bgzf_count")
        return int(n.value)

    def names(self):
        """`pairix -l`: the pairs of the loaded index in the order of its name table, as bytes."""
        total = C.c_uint64()
        self._chk(self.L.mkt_bgzf_names(self.h, 0, None, 0, C.byref(total)), "mkt_bgzf_names")
        buf = C.create_string_buffer(max(total.value, 1))
        self._chk(self.L.mkt_bgzf_names(self.h, 0, buf, total.value, None), "mkt_bgzf_names")
        return buf.raw[:total.value].split(b"\0")[:-1]

    def query(self, regions, autoflip=False):
        """One `bytes` per region ('chrA:b-e|chrB:b-e', a side may be '*' or lack its range; str or bytes): the lines pairix prints for
        it.  Needs add and load_index; the counters are kept in .query_info.  A refused region raises MktError naming its index in
        the batch, a refused block BgzfRefused, an index of another file MktError."""
        regs = [r if isinstance(r, bytes) else r.encode("latin-1") for r in regions]
        arr = (C.c_char_p * max(len(regs), 1))(*regs)
        o = BgzfQueryOpts()
        o.autoflip = 1 if autoflip else 0
        info = _BgzfQueryInfoC()
        self.query_info = None
        rc = self.L.mkt_bgzf_query(self.h, arr, len(regs), C.byref(o), C.byref(info))
        if rc == -9 and info.reason:
            msg = self.L.mkt_bgzf_error(self.h).decode()
            raise BgzfRefused(f"mkt_bgzf_query: {msg}", msg[msg.rfind("[") + 1:msg.rfind("]")], int(info.bad_offset))
        self._chk(rc, "mkt_bgzf_query")
        self.query_info = BgzfQueryInfo(*(int(getattr(info, k)) for k in BgzfQueryInfo._fields))
        n = self.query_info.answer_bytes
        buf = C.create_string_buffer(max(n, 1))
        self._chk(self.L.mkt_bgzf_fetch_query(self.h, 0, buf, n), "mkt_bgzf_fetch_query")
        off = (C.c_uint64 * (len(regs) + 1))()
        self._chk(self.L.mkt_bgzf_fetch_query_offsets(self.h, off), "mkt_bgzf_fetch_query_offsets")
        return [buf.raw[off[k]:off[k + 1]] for k in range(len(regs))]

    def query_counts(self):
        """Lines per region of the last query."""
        n = self.query_info.regions if self.query_info else 0
        out = (C.c_uint64 * max(n, 1))()
        self._chk(self.L.mkt_bgzf_fetch_query_counts(self.h, out), "mkt_bgzf_fetch_query_counts")
        return [int(out[k]) for k in range(n)]

    def query_device(self):
        """(device pointer, bytes) of the last query's concatenated answer: what Matrix.add_device takes; valid until the next add, run,
        query or close."""
        d, n = C.c_void_p(), C.c_uint64()
        self._chk(self.L.mkt_bgzf_query_device(self.h, C.byref(d), C.byref(n)), "mkt_bgzf_query_device")
        return d.value or 0, int(n.value)

    def timing_ms(self):
        t = (C.c_double * 5)()
        self._chk(self.L.mkt_bgzf_timing(self.h, C.byref(t)), "mkt_bgzf_timing")
        return dict(zip(("table_upload", "inflate", "crc"), (float(x) for x in t)))

    def query_timing_ms(self):
        """Of the last query: plan upload, inflate and CRC of the selected blocks; line index, filter, scan and gather."""
        t = (C.c_double * 5)()
        self._chk(self.L.mkt_bgzf_timing(self.h, C.byref(t)), "mkt_bgzf_timing")
        return {"inflate_selected": float(t[3]), "filter_gather": float(t[4])}

    def clear(self):
        """Forgets the file, the text, a loaded index and the last answer."""
        self._chk(self.L.mkt_bgzf_clear(self.h), "mkt_bgzf_clear")
        self.info = self.query_info = None

    def close(self):
        if self.h:
            self.L.mkt_bgzf_destroy(self.h)
            self.h = C.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()


class BamRefused(MktError):
    """A BAM stream the decoder refuses: .reason is the key of the reason (the list stands in include/mkt.h), .record the ordinal of the
    record in the whole stream, .offset its offset in the inflated stream."""

    def __init__(self, msg, reason, record, offset):
        MktError.__init__(self, msg)
        self.reason = reason
        self.record = record
        self.offset = offset


class BamReader:
    """The inflated stream of a BAM decoded to SAM text on the GPU, what `samtools view` prints: see mkt_bamtext_* in include/mkt.h,
    where the definition stands.  add / add_device take the stream in any chunking, every run decodes the complete records held and
    carries the rest, finish ends the stream."""

    def __init__(self, device=0):
        self.L = load_library()
        self.h = C.c_void_p()
        self.info = None
        rc = self.L.mkt_bamtext_create(device, C.byref(self.h))
        if rc != 0:
            raise MktError(f"mkt_bamtext_create: {self.L.mkt_strerror(rc).decode()}")

    def _chk(self, rc, what, info=None):
        if rc == -9 and info is not None:
            msg = self.L.mkt_bamtext_error(self.h).decode()
            raise BamRefused(f"{what}: {msg}", msg[msg.rfind("[") + 1:msg.rfind("]")], int(info.bad_record), int(info.bad_offset))
        if rc != 0:
            raise MktError(f"{what}: {self.L.mkt_strerror(rc).decode()}: {self.L.mkt_bamtext_error(self.h).decode()}")

    def add(self, data: bytes):
        self._chk(self.L.mkt_bamtext_add(self.h, data, len(data)), "mkt_bamtext_add")

    def add_device(self, d_ptr, n):
        self._chk(self.L.mkt_bamtext_add_device(self.h, C.c_void_p(d_ptr), n), "mkt_bamtext_add_device")

    def run(self, segment_bytes=0, max_record=0):
        """Decodes every complete record held; returns the counters (also kept in .info).  A refused stream raises BamRefused and
        leaves no text; the reader then takes a new stream."""
        o = BamTextOpts()
        o.segment_bytes, o.max_record = segment_bytes, max_record
        info = _BamTextInfoC()
        self.info = None
        self._chk(self.L.mkt_bamtext_run(self.h, C.byref(o), C.byref(info)), "mkt_bamtext_run", info)
        self.info = BamTextInfo(*(int(getattr(info, k)) for k in BamTextInfo._fields))
        return self.info

    def finish(self):
        """The end of the stream: BamRefused (truncated / header_truncated) where a partial record or header is held."""
        info = _BamTextInfoC()
        rc = self.L.mkt_bamtext_finish(self.h, C.byref(info))
        if rc != 0:
            self.info = None                             # a refused stream leaves no text
        self._chk(rc, "mkt_bamtext_finish", info)

    def header(self):
        """The header text as `samtools view -H` prints it."""
        total = C.c_uint64()
        self._chk(self.L.mkt_bamtext_fetch_header(self.h, 0, None, 0, C.byref(total)), "mkt_bamtext_fetch_header")
        buf = C.create_string_buffer(max(total.value, 1))
        self._chk(self.L.mkt_bamtext_fetch_header(self.h, 0, buf, total.value, None), "mkt_bamtext_fetch_header")
        return buf.raw[:total.value]

    def refs(self):
        """[(name, length)] of the references."""
        n, ln = C.c_uint32(), C.c_int32()
        self._chk(self.L.mkt_bamtext_fetch_ref(self.h, 0, None, 0, None, C.byref(n)), "mkt_bamtext_fetch_ref")
        out = []
        buf = C.create_string_buffer(1 << 16)
        for k in range(n.value):
            self._chk(self.L.mkt_bamtext_fetch_ref(self.h, k, buf, len(buf), C.byref(ln), None), "mkt_bamtext_fetch_ref")
            out.append((buf.value, int(ln.value)))
        return out

    def text(self):
        """The SAM lines of the last run."""
        if self.info is None:
            raise MktError("text before a run that succeeded")
        n = self.info.text_bytes
        buf = C.create_string_buffer(max(n, 1))
        self._chk(self.L.mkt_bamtext_fetch_text(self.h, 0, buf, n), "mkt_bamtext_fetch_text")
        return buf.raw[:n]

    def device_text(self):
        """(device pointer, bytes) of the last run's text; valid until the next run or close."""
        d, n = C.c_void_p(), C.c_uint64()
        self._chk(self.L.mkt_bamtext_device_text(self.h, C.byref(d), C.byref(n)), "mkt_bamtext_device_text")
        return d.value or 0, int(n.value)

    def timing_ms(self):
        t = (C.c_double * 6)()
        self._chk(self.L.mkt_bamtext_timing(self.h, t), "mkt_bamtext_timing")
        return dict(zip(("header", "index_guess", "resolve", "length", "scan", "emit"), (float(x) for x in t)))

    def close(self):
        if self.h:
            self.L.mkt_bamtext_destroy(self.h)
            self.h = C.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()


def bam_to_sam(bam: bytes, header=False, piece=None, device=0, **opts):
    """The bytes of a BAM file -> what `samtools view` (header=True: `view -h`) prints: BgzfReader inflates the file, BamReader decodes
    the inflated stream from device memory, `piece` inflated bytes per run (None: all at once)."""
    with BgzfReader(device) as z, BamReader(device) as r:
        z.add(bam)
        z.run()
        d, n = z.device_text()
        out = []
        step = piece or max(n, 1)
        for k in range(0, max(n, 1), step):
            r.add_device(d + k, min(step, n - k))
            r.run(**opts)
            out.append(r.text())
        r.finish()
        return (r.header() if header else b"") + b"".join(out)


class PairCompare:
    """Pair-level concordance of two .pairs texts (the reference's benchmarking/check.consistency.pl) on the GPU: see mkt_paircmp_* in
    include/mkt.h, where the definition stands."""
    DIST_KEYS = ("cis_lt_1k", "cis_1_10k", "cis_gt_10k", "trans")

    def __init__(self, device=0):
        self.L = load_library()
        self.h = C.c_void_p()
        self._info = None
        self._max_dist = 200
        rc = self.L.mkt_paircmp_create(device, C.byref(self.h))
        if rc != 0:
            raise MktError(f"mkt_paircmp_create: {self.L.mkt_strerror(rc).decode()}")

    def _chk(self, rc, what):
        if rc != 0:
            raise MktError(f"{what}: {self.L.mkt_strerror(rc).decode()}: {self.L.mkt_paircmp_error(self.h).decode()}")

    def add_a(self, data: bytes):
        self._chk(self.L.mkt_paircmp_add(self.h, 0, data, len(data)), "mkt_paircmp_add")

    def add_b(self, data: bytes):
        self._chk(self.L.mkt_paircmp_add(self.h, 1, data, len(data)), "mkt_paircmp_add")

    def add_device(self, side, d_ptr, n):
        """n bytes of device memory at d_ptr to side "a" or "b" """
        self._chk(self.L.mkt_paircmp_add_device(self.h, {"a": 0, "b": 1}[side], C.c_void_p(d_ptr), n), "mkt_paircmp_add_device")

    def run(self, max_dist=200, want_lines=True, hash_bits=0):
        """The join of what was added; returns the counters as a dict.  Repeatable with other options."""
        o = PairCompareOpts()
        self.L.mkt_paircmp_opts_default(C.byref(o))
        o.max_dist, o.want_lines, o.hash_bits = max_dist, 1 if want_lines else 0, hash_bits
        info = _PairCompareInfoC()
        self._info = None
        self._chk(self.L.mkt_paircmp_run(self.h, C.byref(o), C.byref(info)), "mkt_paircmp_run")
        self._info, self._max_dist = info, max_dist
        d = {k: int(getattr(info, k)) for k in ("distinct_a", "consistent", "discordant", "a_only", "b_only", "host_runs", "lines_bytes")}
        d["lines"] = [int(x) for x in info.lines]
        d["data_lines"] = [int(x) for x in info.data_lines]
        d["dist"] = [dict(zip(self.DIST_KEYS, (int(x) for x in info.dist[s]))) for s in range(2)]
        return d

    def report(self, name_a, name_b):
        """The report of the last run as the script prints it (bytes)."""
        if self._info is None:
            raise MktError("report before run")
        na, nb = os.fsencode(name_a), os.fsencode(name_b)
        buf = C.create_string_buffer(4096 + len(na) + len(nb))
        n = self.L.mkt_paircmp_report(C.byref(self._info), self._max_dist, na, nb, buf, len(buf))
        if n < 0:
            raise MktError("mkt_paircmp_report: the buffer is too small")
        return buf.raw[:n]

    def classes(self, side):
        """One class byte per input line of side "a" or "b" (numpy uint8)."""
        import numpy as np
        if self._info is None:
            raise MktError("classes before run")
        s = {"a": 0, "b": 1}[side]
        out = np.zeros(int(self._info.lines[s]), dtype=np.uint8)
        self._chk(self.L.mkt_paircmp_fetch_classes(self.h, s, 0, out.size, C.c_void_p(out.ctypes.data)), "mkt_paircmp_fetch_classes")
        return out

    def lines(self):
        """The inconsistent text of the last run (b"" without want_lines)."""
        if self._info is None:
            raise MktError("lines before run")
        n = int(self._info.lines_bytes)
        buf = C.create_string_buffer(max(n, 1))
        self._chk(self.L.mkt_paircmp_fetch_lines(self.h, 0, buf, n), "mkt_paircmp_fetch_lines")
        return buf.raw[:n]

    def timing_ms(self):
        t = [C.c_double() for _ in range(4)]
        self._chk(self.L.mkt_paircmp_timing(self.h, *[C.byref(x) for x in t]), "mkt_paircmp_timing")
        return dict(zip(("parse", "sort", "join", "emit"), (x.value for x in t)))

    def close(self):
        if self.h:
            self.L.mkt_paircmp_destroy(self.h)
            self.h = C.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()


class PairStats:
    """Pair-level QC of .pairs text on the GPU in one streaming pass: totals, distance thresholds, the reference's cis0 / cis1K / cis10K /
    trans, chromosome-pair counts, distance by strand orientation and P(s): see mkt_pairstat_* in include/mkt.h, where the definition
    and the limits stand (at most 2048 names in the table).  chromsizes: bytes of name<TAB>length lines."""
    GE_KEYS = ("cis_1kb+", "cis_2kb+", "cis_4kb+", "cis_10kb+", "cis_20kb+", "cis_40kb+")
    ORIENTATIONS = ("++", "+-", "-+", "--")
    BINS = 74

    def __init__(self, chromsizes: bytes, device=0):
        self.L = load_library()
        self.names = [ln.split(b"\t")[0].decode("latin-1") for ln in (x.rstrip(b"\r") for x in bytes(chromsizes).split(b"\n")) if ln and not ln.startswith(b"#")]
        self.h = C.c_void_p()
        self.info = None
        rc = self.L.mkt_pairstat_create(device, bytes(chromsizes), len(chromsizes), C.byref(self.h))
        if rc != 0:
            raise MktError(f"mkt_pairstat_create: {self.L.mkt_strerror(rc).decode()}: {self.L.mkt_pairstat_error(None).decode()}")

    def _chk(self, rc, what):
        if rc < 0:
            raise MktError(f"{what}: {self.L.mkt_strerror(rc).decode()}: {self.L.mkt_pairstat_error(self.h).decode()}")
        return rc

    def add(self, data: bytes):
        """A piece of the text, cut anywhere."""
        self._chk(self.L.mkt_pairstat_add(self.h, data, len(data)), "mkt_pairstat_add")
        self.info = None

    def add_device(self, d_ptr, n):
        """n bytes of device memory at d_ptr (e.g. BgzfReader.device_text())."""
        self._chk(self.L.mkt_pairstat_add_device(self.h, C.c_void_p(d_ptr), n), "mkt_pairstat_add_device")
        self.info = None

    def add_keys(self, ctx, drop_last=True, flags=None):
        """The reported pairs of a Context created with EXT_KEYS; flags (bytes, one per reported pair, e.g. from ext_dedup): leave those out."""
        self._chk(self.L.mkt_pairstat_add_keys(self.h, ctx.h, 1 if drop_last else 0, flags, len(flags) if flags is not None else 0), "mkt_pairstat_add_keys")
        self.info = None

    def run(self, tol_permille=50, min_count=1000):
        """Closes the carried line and computes everything; returns the counters as a dict (also kept in .info)."""
        o = PairStatsOpts()
        self.L.mkt_pairstat_opts_default(C.byref(o))
        o.tol_permille, o.min_count = tol_permille, min_count
        info = _PairStatsInfoC()
        self.info = None
        self._chk(self.L.mkt_pairstat_run(self.h, C.byref(o), C.byref(info)), "mkt_pairstat_run")
        d = {k: int(getattr(info, k)) for k in ("total", "skipped", "counted", "cis", "trans", "no_strand", "header_lines", "cis0", "cis1K", "cis10K", "ref_trans", "convergence_dist")}
        d.update(zip(self.GE_KEYS, (int(x) for x in info.cis_ge)))
        self.info = d
        return d

    def _ran(self, what):
        if self.info is None:
            raise MktError(f"{what} before a run that succeeded")

    @property
    def dist_freq(self):
        """numpy uint64 [74, 4]: cis pairs by distance bin and orientation (++ +- -+ --)"""
        import numpy as np
        self._ran("dist_freq")
        out = np.zeros((self.BINS, 4), dtype=np.uint64)
        self._chk(self.L.mkt_pairstat_fetch_dist(self.h, C.c_void_p(out.ctypes.data)), "mkt_pairstat_fetch_dist")
        return out

    @property
    def chrom_freq(self):
        """numpy uint64 [n, n]: counted pairs per ordered (chr1, chr2) in table order"""
        import numpy as np
        self._ran("chrom_freq")
        n = len(self.names)
        out = np.zeros((n, n), dtype=np.uint64)
        self._chk(self.L.mkt_pairstat_fetch_chrom(self.h, 0, n, C.c_void_p(out.ctypes.data)), "mkt_pairstat_fetch_chrom")
        return out

    @property
    def scaling(self):
        """(edges uint64 [75], area float64 [74], P float64 [74])"""
        import numpy as np
        self._ran("scaling")
        e, a, p = np.zeros(self.BINS + 1, dtype=np.uint64), np.zeros(self.BINS, dtype=np.float64), np.zeros(self.BINS, dtype=np.float64)
        self._chk(self.L.mkt_pairstat_fetch_scaling(self.h, C.c_void_p(e.ctypes.data), C.c_void_p(a.ctypes.data), C.c_void_p(p.ctypes.data)), "mkt_pairstat_fetch_scaling")
        return PairStatsScaling(e, a, p)

    def _text(self, which):
        self._ran("text")
        n = self._chk(self.L.mkt_pairstat_text(self.h, which, None, 0), "mkt_pairstat_text")
        buf = C.create_string_buffer(max(n, 1))
        self._chk(self.L.mkt_pairstat_text(self.h, which, buf, n), "mkt_pairstat_text")
        return buf.raw[:n]

    def stat_text(self):
        """The bytes of PREFIX.pairs.stat"""
        return self._text(0)

    def scaling_text(self):
        """The bytes of PREFIX.scaling.tsv"""
        return self._text(1)

    def timing_ms(self):
        t = [C.c_double() for _ in range(3)]
        self._chk(self.L.mkt_pairstat_timing(self.h, *[C.byref(x) for x in t]), "mkt_pairstat_timing")
        return dict(zip(("index", "kernel", "total"), (x.value for x in t)))

    def close(self):
        if self.h:
            self.L.mkt_pairstat_destroy(self.h)
            self.h = C.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()


class Matrix:
    """Reported pairs -> binned contact matrices at several resolutions on the GPU: see mkt_matrix_* in include/mkt.h (where the
    binning is defined).  chromsizes: bytes of name<TAB>length lines, file order = bin order; resolutions: 1 .. 16 bin sizes in bp."""

    def __init__(self, chromsizes: bytes, resolutions, device=0):
        self.L = load_library()
        self.resolutions = [int(r) for r in resolutions]
        # the names of the table in order, as the library reads them ('#' lines and empty lines are no chromosomes)
        self.names = [ln.split(b"\t")[0].decode("latin-1") for ln in (x.rstrip(b"\r") for x in bytes(chromsizes).split(b"\n")) if ln and not ln.startswith(b"#")]
        arr = (C.c_uint32 * max(len(self.resolutions), 1))(*self.resolutions)
        self.h = C.c_void_p()
        rc = self.L.mkt_matrix_create(device, chromsizes, len(chromsizes), arr, len(self.resolutions), C.byref(self.h))
        if rc != 0:
            raise MktError(f"mkt_matrix_create: {self.L.mkt_strerror(rc).decode()}: {self.L.mkt_matrix_error(None).decode()}")

    def _chk(self, rc, what):
        if rc != 0:
            raise MktError(f"{what}: {self.L.mkt_strerror(rc).decode()}: {self.L.mkt_matrix_error(self.h).decode()}")

    def add(self, data: bytes):
        """.pairs text in any chunking (a partial last line is carried)"""
        self._chk(self.L.mkt_matrix_add(self.h, data, len(data)), "mkt_matrix_add")

    def add_device(self, d_ptr, n):
        self._chk(self.L.mkt_matrix_add_device(self.h, C.c_void_p(d_ptr), n), "mkt_matrix_add_device")

    def add_keys(self, ctx, drop_last=True, flags=None):
        """The reported pairs of a Context created with EXT_KEYS; flags (bytes, one per reported pair, e.g. from ext_dedup): leave those out."""
        self._chk(self.L.mkt_matrix_add_keys(self.h, ctx.h, 1 if drop_last else 0, flags, len(flags) if flags is not None else 0), "mkt_matrix_add_keys")

    def run(self):
        """(pairs seen, pairs skipped)"""
        p, s = C.c_uint64(), C.c_uint64()
        self._chk(self.L.mkt_matrix_run(self.h, C.byref(p), C.byref(s)), "mkt_matrix_run")
        return p.value, s.value

    def info(self, res):
        """(nbins, non-empty cells, bytes of COO text) of resolution index res"""
        a, b, c = C.c_uint64(), C.c_uint64(), C.c_uint64()
        self._chk(self.L.mkt_matrix_info(self.h, res, C.byref(a), C.byref(b), C.byref(c)), "mkt_matrix_info")
        return a.value, b.value, c.value

    def cells(self, res):
        """(bin1, bin2, count): three numpy uint32 arrays, ascending in (bin1, bin2)"""
        import numpy as np
        nnz = self.info(res)[1]
        out = [np.zeros(nnz, dtype=np.uint32) for _ in range(3)]
        if nnz:
            self._chk(self.L.mkt_matrix_fetch(self.h, res, 0, nnz, *[a.ctypes.data_as(C.c_void_p) for a in out]), "mkt_matrix_fetch")
        return tuple(out)

    def text(self, res):
        """the lines bin1<TAB>bin2<TAB>count of resolution index res, as made on the device"""
        n = self.info(res)[2]
        buf = C.create_string_buffer(max(n, 1))
        self._chk(self.L.mkt_matrix_fetch_text(self.h, res, 0, buf, n), "mkt_matrix_fetch_text")
        return buf.raw[:n]

    def timing_ms(self, res):
        ms = C.c_double()
        self._chk(self.L.mkt_matrix_timing(self.h, res, C.byref(ms)), "mkt_matrix_timing")
        return ms.value

    def balance(self, res, **opts):
        """Iterative correction of resolution index res after run() (the definition: mkt_matrix_balance in include/mkt.h).
        opts: ignore_diags, min_nnz, min_count, mad_max, tol, max_iters; returns BalanceStats."""
        o = BalanceOpts()
        self.L.mkt_balance_opts_default(C.byref(o))
        for k, v in opts.items():
            if k not in ("ignore_diags", "min_nnz", "min_count", "mad_max", "tol", "max_iters"):
                raise TypeError(f"balance: unknown option {k}")
            setattr(o, k, v)
        s = _BalanceStatsC()
        self._chk(self.L.mkt_matrix_balance(self.h, res, C.byref(o), C.byref(s)), "mkt_matrix_balance")
        return BalanceStats(s.iterations, bool(s.converged), s.var, s.scale, s.masked)

    def weights(self, res):
        """the balancing weights of resolution index res: numpy float64[nbins], NaN for a masked bin"""
        import numpy as np
        out = np.zeros(self.info(res)[0], dtype=np.float64)
        self._chk(self.L.mkt_matrix_fetch_weights(self.h, res, 0, out.size, out.ctypes.data_as(C.c_void_p)), "mkt_matrix_fetch_weights")
        return out

    def balance_timing_ms(self, res):
        """(setup ms, iteration loop ms) of the last balance(res): device time, HIP events"""
        a, b = C.c_double(), C.c_double()
        self._chk(self.L.mkt_matrix_balance_timing(self.h, res, C.byref(a), C.byref(b)), "mkt_matrix_balance_timing")
        return a.value, b.value

    def expected(self, res, use_weights=True):
        """Expected-contact tables of resolution index res after run() (and balance(res) when use_weights): the definition is
        mkt_matrix_expected in include/mkt.h.  Returns Expected(cis, trans, genome, n_chrom, smooth_groups), the three tables as
        namedtuples of numpy arrays (n_valid and count_sum uint64, the others float64)."""
        import numpy as np
        o = ExpectedOpts()
        self.L.mkt_expected_opts_default(C.byref(o))
        o.use_weights = 1 if use_weights else 0
        info = _ExpectedInfoC()
        self._chk(self.L.mkt_matrix_expected(self.h, res, C.byref(o), C.byref(info)), "mkt_matrix_expected")

        def table(fn, what, rows, cls):
            cols = [np.zeros(rows, dtype=np.uint64 if k < 2 else np.float64) for k in range(len(cls._fields))]
            self._chk(fn(self.h, res, 0, rows, *[a.ctypes.data_as(C.c_void_p) for a in cols]), what)
            return cls(*cols)
        return Expected(table(self.L.mkt_matrix_fetch_expected_cis, "mkt_matrix_fetch_expected_cis", info.cis_rows, ExpectedCis),
                        table(self.L.mkt_matrix_fetch_expected_trans, "mkt_matrix_fetch_expected_trans", info.trans_rows, ExpectedTrans),
                        table(self.L.mkt_matrix_fetch_expected_genome, "mkt_matrix_fetch_expected_genome", info.genome_rows, ExpectedGenome),
                        info.n_chrom, info.smooth_groups)

    def values(self, res, kind="balanced"):
        """per-cell values in the order of cells(res): numpy float64[nnz]; kind "balanced" (count * w[bin1] * w[bin2]), "oe" or
        "oe_smooth" (divided by the expected / smoothed expected of the last expected(res)); NaN for a cell with a masked bin"""
        import numpy as np
        if kind not in VALUE_KINDS:
            raise ValueError(f"values: kind {kind!r} (one of {', '.join(VALUE_KINDS)})")
        out = np.zeros(self.info(res)[1], dtype=np.float64)
        self._chk(self.L.mkt_matrix_fetch_values(self.h, res, VALUE_KINDS[kind], 0, out.size, out.ctypes.data_as(C.c_void_p)), "mkt_matrix_fetch_values")
        return out

    def expected_timing_ms(self, res):
        """(setup ms, sums ms) of the last expected(res): device time, HIP events"""
        a, b = C.c_double(), C.c_double()
        self._chk(self.L.mkt_matrix_expected_timing(self.h, res, C.byref(a), C.byref(b)), "mkt_matrix_expected_timing")
        return a.value, b.value

    def loops(self, res, **opts):
        """Loop calling on resolution index res after expected(res): the definition is mkt_matrix_loops in include/mkt.h.  opts: peak,
        window, window_max, min_ll_count, min_dist, max_dist, fdr, cluster_radius.  Returns Loops(loops, info): the loop table as a list
        of Loop(cell, bin1, bin2, count, window, r, n_cells, box) ascending by peak cell index, and LoopsInfo."""
        o = LoopsOpts()
        self.L.mkt_loops_opts_default(C.byref(o))
        for k, v in opts.items():
            if k not in ("peak", "window", "window_max", "min_ll_count", "min_dist", "max_dist", "fdr", "cluster_radius"):
                raise TypeError(f"loops: unknown option {k}")
            setattr(o, k, v)
        info = _LoopsInfoC()
        self._chk(self.L.mkt_matrix_loops(self.h, res, C.byref(o), C.byref(info)), "mkt_matrix_loops")
        rows = (_LoopC * max(info.loops, 1))()
        self._chk(self.L.mkt_matrix_fetch_loops(self.h, res, 0, info.loops, rows), "mkt_matrix_fetch_loops")
        table = [Loop(x.cell, x.bin1, x.bin2, x.count, x.window, tuple(x.r), x.n_cells, tuple(x.box)) for x in rows[:info.loops]]
        self._n_loops = getattr(self, "_n_loops", {})
        self._n_loops[res] = info.loops                                     # pileup_loops reads the table again
        return Loops(table, LoopsInfo(*[getattr(info, k) for k in LoopsInfo._fields]))

    def loop_cells(self, res):
        """per-cell results of the last loops(res) in the order of cells(res): LoopCells of numpy arrays (status, window, enriched uint8 [nnz];
        chunk uint8, kept uint16, r, bsum, esum, e float64 [nnz, 4] for DONUT, LL, H, V; csum_ll uint64 [nnz])"""
        import numpy as np
        nnz = self.info(res)[1]
        out = LoopCells(np.zeros(nnz, np.uint8), np.zeros(nnz, np.uint8), np.zeros((nnz, 4), np.uint8), np.zeros((nnz, 4), np.float64), np.zeros(nnz, np.uint8),
                        np.zeros(nnz, np.uint64), np.zeros((nnz, 4), np.uint16), np.zeros((nnz, 4), np.float64), np.zeros((nnz, 4), np.float64), np.zeros((nnz, 4), np.float64))
        self._chk(self.L.mkt_matrix_fetch_loop_cells(self.h, res, 0, nnz, *[a.ctypes.data_as(C.c_void_p) for a in out]), "mkt_matrix_fetch_loop_cells")
        return out

    def loop_hist(self, res):
        """the histogram of the last loops(res): numpy uint64 [4, 28, 2048] (region, expected chunk, min(count, 2047))"""
        import numpy as np
        out = np.zeros((4, 28, 2048), dtype=np.uint64)
        self._chk(self.L.mkt_matrix_fetch_loop_hist(self.h, res, out.ctypes.data_as(C.c_void_p)), "mkt_matrix_fetch_loop_hist")
        return out

    def loop_thresholds(self, res):
        """the count thresholds of the last loops(res): numpy uint32 [4, 28]; 2048 = none"""
        import numpy as np
        out = np.zeros((4, 28), dtype=np.uint32)
        self._chk(self.L.mkt_matrix_fetch_loop_thresholds(self.h, res, out.ctypes.data_as(C.c_void_p)), "mkt_matrix_fetch_loop_thresholds")
        return out

    def loops_timing_ms(self, res):
        """(neighbourhood pass ms, histogram ms, flagging ms) of the last loops(res): device time, HIP events"""
        a, b, c = C.c_double(), C.c_double(), C.c_double()
        self._chk(self.L.mkt_matrix_loops_timing(self.h, res, C.byref(a), C.byref(b), C.byref(c)), "mkt_matrix_loops_timing")
        return a.value, b.value, c.value

    def _eigs_opts(self, what, opts):
        o = EigsOpts()
        self.L.mkt_eigs_opts_default(C.byref(o))
        for k, v in opts.items():
            if k not in EIGS_OPTS:
                raise TypeError(f"{what}: unknown option {k}")
            setattr(o, k, v)
        return o

    def eigs(self, res, phasing=None, **opts):
        """Compartment eigenvectors of resolution index res after expected(res): the definition is mkt_matrix_eigs in include/mkt.h.
        phasing: nbins values (NaN = none) that fix the sign, or None.  opts: n_eigs, ignore_diags, min_good, max_iters, tol, clip.
        Returns Eigs(info, vectors [n_eigs, nbins], lambdas and resid [n_chrom, n_eigs], n_good, iterations, converged [n_chrom])."""
        import numpy as np
        o = self._eigs_opts("eigs", opts)
        nb = self.info(res)[0]
        p = None
        if phasing is not None:
            p = np.ascontiguousarray(phasing, dtype=np.float64)
            if p.shape != (nb,):
                raise ValueError(f"eigs: phasing has shape {p.shape}, ({nb},) is needed")
        info = _EigsInfoC()
        self._chk(self.L.mkt_matrix_eigs(self.h, res, C.byref(o), p.ctypes.data_as(C.c_void_p) if p is not None else None, C.byref(info)), "mkt_matrix_eigs")
        vec = np.zeros((o.n_eigs, nb), dtype=np.float64)
        for k in range(o.n_eigs):
            self._chk(self.L.mkt_matrix_fetch_eigvecs(self.h, res, k, 0, nb, vec[k].ctypes.data_as(C.c_void_p)), "mkt_matrix_fetch_eigvecs")
        nc = info.n_chrom
        lam, rs = np.zeros((nc, o.n_eigs), dtype=np.float64), np.zeros((nc, o.n_eigs), dtype=np.float64)
        ng, it, cv = np.zeros(nc, dtype=np.uint32), np.zeros(nc, dtype=np.uint32), np.zeros(nc, dtype=np.uint8)
        self._chk(self.L.mkt_matrix_fetch_eigvals(self.h, res, 0, nc, *[a.ctypes.data_as(C.c_void_p) for a in (lam, rs, ng, it, cv)]), "mkt_matrix_fetch_eigvals")
        return Eigs(EigsInfo(*[getattr(info, k) for k in EigsInfo._fields]), vec, lam, rs, ng, it, cv.astype(bool))

    def eigs_apply(self, res, x, **opts):
        """y = A x for every chromosome at once through the sweep kernel of eigs(): x is [nbins] or [nbins, ncols <= 8], used as given
        on good bins and as 0 elsewhere; y has x's shape and is 0 on the other bins and on skipped chromosomes."""
        import numpy as np
        o = self._eigs_opts("eigs_apply", opts)
        x = np.asarray(x, dtype=np.float64)
        x2 = np.ascontiguousarray(x.reshape(x.shape[0], -1))
        if x2.shape[0] != self.info(res)[0]:
            raise ValueError(f"eigs_apply: x has {x2.shape[0]} rows, {self.info(res)[0]} are needed")
        y = np.zeros_like(x2)
        self._chk(self.L.mkt_matrix_eigs_apply(self.h, res, C.byref(o), x2.ctypes.data_as(C.c_void_p), x2.shape[1], y.ctypes.data_as(C.c_void_p)), "mkt_matrix_eigs_apply")
        return y.reshape(x.shape)

    def eigs_timing_ms(self, res):
        """(setup ms, sweeps ms, rest of the iteration loop ms) of the last eigs(res)"""
        a, b, c = C.c_double(), C.c_double(), C.c_double()
        self._chk(self.L.mkt_matrix_eigs_timing(self.h, res, C.byref(a), C.byref(b), C.byref(c)), "mkt_matrix_eigs_timing")
        return a.value, b.value, c.value

    def insulation(self, res, windows=(5, 10, 25), **opts):
        """Insulation scores and boundaries of resolution index res after run() (and balance(res) unless use_weights=0): the definition
        is mkt_matrix_insulation in include/mkt.h.  windows: 1 .. 4 sizes in bins, strictly ascending.  opts: ignore_diags, use_weights,
        min_frac_valid, min_strength.  Returns InsulationInfo(n_chrom, windows, defined, minima, boundaries), the last three per window."""
        o = InsulationOpts()
        self.L.mkt_insulation_opts_default(C.byref(o))
        windows = [int(w) for w in windows]
        o.n_windows = len(windows)
        for k in range(4):
            o.window[k] = windows[k] if k < len(windows) else 0
        for k, v in opts.items():
            if k not in INSULATION_OPTS:
                raise TypeError(f"insulation: unknown option {k}")
            setattr(o, k, int(v) if k == "use_weights" else v)
        info = _InsulationInfoC()
        self._chk(self.L.mkt_matrix_insulation(self.h, res, C.byref(o), C.byref(info)), "mkt_matrix_insulation")
        n = min(len(windows), 4)
        return InsulationInfo(info.n_chrom, tuple(windows), tuple(info.defined[:n]), tuple(info.minima[:n]), tuple(info.boundaries[:n]))

    def insulation_track(self, res, k):
        """window k of the last insulation(res): InsulationTrack of numpy arrays over the bins (n_valid, csum uint64; bsum, score, log2_score,
        strength float64, NaN where undefined; boundary bool)"""
        import numpy as np
        nb = self.info(res)[0]
        cols = [np.zeros(nb, np.uint64), np.zeros(nb, np.uint64)] + [np.zeros(nb, np.float64) for _ in range(4)] + [np.zeros(nb, np.uint8)]
        self._chk(self.L.mkt_matrix_fetch_insulation(self.h, res, k, 0, nb, *[a.ctypes.data_as(C.c_void_p) for a in cols]), "mkt_matrix_fetch_insulation")
        return InsulationTrack(*cols[:6], cols[6].astype(bool))

    def insulation_timing_ms(self, res):
        """(setup ms, sweep ms) of the last insulation(res): device time, HIP events"""
        a, b = C.c_double(), C.c_double()
        self._chk(self.L.mkt_matrix_insulation_timing(self.h, res, C.byref(a), C.byref(b)), "mkt_matrix_insulation_timing")
        return a.value, b.value

    def pileup(self, res, bin1, bin2, **opts):
        """Pileup of resolution index res around the features (bin1[f], bin2[f]) (global bin ids, bin1 <= bin2) after expected(res): the
        definition is mkt_matrix_pileup in include/mkt.h.  opts: flank, corner, kind ("balanced", "oe", "oe_smooth" or its number),
        ignore_diags, edges, min_dist, max_dist.  Returns PileupInfo (the counts per status, side, chunks and the seven scores)."""
        import numpy as np
        o = PileupOpts()
        self.L.mkt_pileup_opts_default(C.byref(o))
        for k, v in opts.items():
            if k not in PILEUP_OPTS:
                raise TypeError(f"pileup: unknown option {k}")
            if k == "kind" and isinstance(v, str):
                if v not in VALUE_KINDS:
                    raise ValueError(f"pileup: kind {v!r} (one of {', '.join(VALUE_KINDS)})")
                v = VALUE_KINDS[v]
            setattr(o, k, int(v))
        a, b = np.ascontiguousarray(bin1, dtype=np.uint32).ravel(), np.ascontiguousarray(bin2, dtype=np.uint32).ravel()
        if a.shape != b.shape:
            raise ValueError(f"pileup: {a.size} first bins and {b.size} second bins")
        info = _PileupInfoC()
        self._chk(self.L.mkt_matrix_pileup(self.h, res, a.ctypes.data_as(C.c_void_p), b.ctypes.data_as(C.c_void_p), a.size, C.byref(o), C.byref(info)), "mkt_matrix_pileup")
        self._pile_shape = getattr(self, "_pile_shape", {})
        self._pile_shape[res] = (info.side, info.features)
        return PileupInfo(*[getattr(info, k) for k in PileupInfo._fields])

    def pileup_result(self, res):
        """the arrays of the last pileup(res): Pileup(n, csum uint64 [side, side]; vsum, mean float64 [side, side], row p + flank, column
        q + flank; status uint8 [features], the PILE_* of every feature)"""
        import numpy as np
        cap = 65 * 65
        cols = [np.zeros(cap, np.uint64), np.zeros(cap, np.uint64), np.zeros(cap, np.float64), np.zeros(cap, np.float64)]
        self._chk(self.L.mkt_matrix_fetch_pileup(self.h, res, *[a.ctypes.data_as(C.c_void_p) for a in cols]), "mkt_matrix_fetch_pileup")
        side, nf = getattr(self, "_pile_shape", {}).get(res, (0, 0))
        if not side:
            raise MktError("pileup_result: the pileup of this resolution was not made through pileup()")
        st = np.zeros(nf, np.uint8)
        self._chk(self.L.mkt_matrix_fetch_pileup_status(self.h, res, 0, nf, st.ctypes.data_as(C.c_void_p)), "mkt_matrix_fetch_pileup_status")
        return Pileup(*[a[:side * side].reshape(side, side).copy() for a in cols], st)

    def pileup_timing_ms(self, res):
        """(setup ms, sweep ms) of the last pileup(res): device time, HIP events"""
        a, b = C.c_double(), C.c_double()
        self._chk(self.L.mkt_matrix_pileup_timing(self.h, res, C.byref(a), C.byref(b)), "mkt_matrix_pileup_timing")
        return a.value, b.value

    def pileup_loops(self, res, **opts):
        """APA: pileup(res) around the peak cells of the last loops(res), in loop order"""
        self._chk(self.L.mkt_matrix_fetch_loops(self.h, res, 0, 0, None), "mkt_matrix_fetch_loops")      # "loops first" when there are none
        n = getattr(self, "_n_loops", {}).get(res, 0)
        rows = (_LoopC * max(n, 1))()
        self._chk(self.L.mkt_matrix_fetch_loops(self.h, res, 0, n, rows), "mkt_matrix_fetch_loops")
        b1, b2 = [x.bin1 for x in rows[:n]], [x.bin2 for x in rows[:n]]
        return self.pileup(res, b1, b2, **opts)

    def pileup_boundaries(self, res, k, **opts):
        """on-diagonal pileup(res) around (i, i) for the boundary bins of window k of the last insulation(res), ascending"""
        import numpy as np
        i = np.flatnonzero(self.insulation_track(res, k).boundary).astype(np.uint32)
        return self.pileup(res, i, i, **opts)

    def saddle(self, res, track, **opts):
        """Saddle tables of resolution index res after expected(res) for the track (nbins values, NaN = none): the definition is
        mkt_matrix_saddle in include/mkt.h.  opts: n_groups, trim_lo, trim_hi (basis points), contact ("cis", "trans" or its number), kind
        ("oe", "oe_smooth" or its number), min_diag, max_diag, corner.  Returns SaddleInfo (the counts, the corner and the three scores)."""
        import numpy as np
        o = SaddleOpts()
        self.L.mkt_saddle_opts_default(C.byref(o))
        for k, v in opts.items():
            if k not in SADDLE_OPTS:
                raise TypeError(f"saddle: unknown option {k}")
            if k == "kind" and isinstance(v, str):
                if v not in VALUE_KINDS:
                    raise ValueError(f"saddle: kind {v!r} (one of {', '.join(VALUE_KINDS)})")
                v = VALUE_KINDS[v]
            if k == "contact" and isinstance(v, str):
                if v not in SADDLE_CONTACTS:
                    raise ValueError(f"saddle: contact {v!r} (cis or trans)")
                v = SADDLE_CONTACTS[v]
            setattr(o, k, int(v))
        t = np.ascontiguousarray(track, dtype=np.float64)
        nb = self.info(res)[0]
        if t.shape != (nb,):
            raise ValueError(f"saddle: the track has shape {t.shape}, ({nb},) is needed")
        info = _SaddleInfoC()
        self._chk(self.L.mkt_matrix_saddle(self.h, res, C.byref(o), t.ctypes.data_as(C.c_void_p), C.byref(info)), "mkt_matrix_saddle")
        self._saddle_q = getattr(self, "_saddle_q", {})
        self._saddle_q[res] = info.n_groups
        return SaddleInfo(*[getattr(info, k) for k in SaddleInfo._fields])

    def saddle_result(self, res):
        """the arrays of the last saddle(res): Saddle(n, nnz, csum uint64 [Q, Q]; vsum, mean float64 [Q, Q]; groups uint8 [nbins], 255 = none;
        group_bins uint64, group_lo, group_hi float64 [Q]; strength, aa_ab, bb_ab float64 [Q // 2], index k - 1)"""
        import numpy as np
        cap = 64 * 64
        tabs = [np.zeros(cap, np.uint64), np.zeros(cap, np.uint64), np.zeros(cap, np.uint64), np.zeros(cap, np.float64), np.zeros(cap, np.float64)]
        self._chk(self.L.mkt_matrix_fetch_saddle(self.h, res, *[a.ctypes.data_as(C.c_void_p) for a in tabs]), "mkt_matrix_fetch_saddle")
        q = getattr(self, "_saddle_q", {}).get(res, 0)
        if not q:
            raise MktError("saddle_result: the saddle tables of this resolution were not made through saddle()")
        g = np.zeros(self.info(res)[0], np.uint8)
        self._chk(self.L.mkt_matrix_fetch_saddle_groups(self.h, res, 0, g.size, g.ctypes.data_as(C.c_void_p)), "mkt_matrix_fetch_saddle_groups")
        edges = [np.zeros(q, np.uint64), np.zeros(q, np.float64), np.zeros(q, np.float64)]
        self._chk(self.L.mkt_matrix_fetch_saddle_edges(self.h, res, *[a.ctypes.data_as(C.c_void_p) for a in edges]), "mkt_matrix_fetch_saddle_edges")
        prof = [np.zeros(q // 2, np.float64) for _ in range(3)]
        self._chk(self.L.mkt_matrix_fetch_saddle_profile(self.h, res, *[a.ctypes.data_as(C.c_void_p) for a in prof]), "mkt_matrix_fetch_saddle_profile")
        return Saddle(*[a[:q * q].reshape(q, q).copy() for a in tabs], g, *edges, *prof)

    def saddle_timing_ms(self, res):
        """(setup ms on the host, sweep + fold ms on the device) of the last saddle(res)"""
        a, b = C.c_double(), C.c_double()
        self._chk(self.L.mkt_matrix_saddle_timing(self.h, res, C.byref(a), C.byref(b)), "mkt_matrix_saddle_timing")
        return a.value, b.value

    def saddle_eigs(self, res, k=0, **opts):
        """saddle(res) with eigenvector k of the last eigs(res) as the track"""
        import numpy as np
        v = np.zeros(self.info(res)[0], dtype=np.float64)
        self._chk(self.L.mkt_matrix_fetch_eigvecs(self.h, res, k, 0, v.size, v.ctypes.data_as(C.c_void_p)), "mkt_matrix_fetch_eigvecs")
        return self.saddle(res, v, **opts)

    def scc(self, other, res, **opts):
        """Replicate comparison: the stratum-adjusted correlation of resolution index res of this matrix (A) and the same resolution of
        `other` (B, found there by its value); the definition is mkt_matrix_scc in include/mkt.h.  opts: h, min_diag, max_diag,
        use_weights, weighting ("n", "var" or its number), min_n, slab_rows.  The results live on this matrix.  Returns SccInfo."""
        o = SccOpts()
        self.L.mkt_scc_opts_default(C.byref(o))
        for k, v in opts.items():
            if k not in SCC_OPTS:
                raise TypeError(f"scc: unknown option {k}")
            if k == "weighting" and isinstance(v, str):
                if v not in SCC_WEIGHTINGS:
                    raise ValueError(f"scc: weighting {v!r} (n or var)")
                v = SCC_WEIGHTINGS[v]
            setattr(o, k, int(v))
        if not 0 <= res < len(self.resolutions):
            raise MktError(f"scc: resolution index {res} of {len(self.resolutions)}")
        if self.resolutions[res] not in other.resolutions:
            raise MktError(f"scc: the other matrix has no resolution {self.resolutions[res]}")
        info = _SccInfoC()
        self._chk(self.L.mkt_matrix_scc(self.h, res, other.h, other.resolutions.index(self.resolutions[res]), C.byref(o), C.byref(info)), "mkt_matrix_scc")
        self._scc_shape = getattr(self, "_scc_shape", {})
        self._scc_shape[res] = (info.n_chrom, info.strata)
        return SccInfo(*[getattr(info, k) for k in SccInfo._fields])

    def scc_result(self, res):
        """the arrays of the last scc(.., res): Scc(n_cand, n uint64; sx, sy, sxx, syy, sxy, rho, w float64: the strata table
        [n_chrom * strata], chromosome-major; scc, num, den float64 and n_scored uint64 per chromosome)"""
        import numpy as np
        self._chk(self.L.mkt_matrix_fetch_scc_chrom(self.h, res, 0, 0, None, None, None, None), "mkt_matrix_fetch_scc_chrom")
        shape = getattr(self, "_scc_shape", {}).get(res)
        if not shape:
            raise MktError("scc_result: the comparison of this resolution was not made through scc()")
        rows = shape[0] * shape[1]
        tab = [np.zeros(rows, np.uint64), np.zeros(rows, np.uint64)] + [np.zeros(rows, np.float64) for _ in range(7)]
        self._chk(self.L.mkt_matrix_fetch_scc_strata(self.h, res, 0, rows, *[a.ctypes.data_as(C.c_void_p) for a in tab]), "mkt_matrix_fetch_scc_strata")
        ch = [np.zeros(shape[0], np.float64) for _ in range(3)] + [np.zeros(shape[0], np.uint64)]
        self._chk(self.L.mkt_matrix_fetch_scc_chrom(self.h, res, 0, shape[0], *[a.ctypes.data_as(C.c_void_p) for a in ch]), "mkt_matrix_fetch_scc_chrom")
        return Scc(*tab, *ch)

    def scc_timing_ms(self, res):
        """(fill ms, sweep + fold ms) on the device of the last scc(.., res)"""
        a, b = C.c_double(), C.c_double()
        self._chk(self.L.mkt_matrix_scc_timing(self.h, res, C.byref(a), C.byref(b)), "mkt_matrix_scc_timing")
        return a.value, b.value

    def viewpoint(self, name, partners=None, **opts):
        """Viewpoint contact profile (a virtual 4C) of chromosome `name` over the resident pairs: mkt_matrix_viewpoint in include/mkt.h.
        partners: None = every other chromosome, a string = a regular expression applied to the names with re.search (the viewpoint
        itself is never a partner), else a list of names.  opts: vbin, pbin, origin, second_side_only, min_count, hotspot_ratio.
        Returns ViewpointInfo."""
        import re
        if name not in self.names:
            raise MktError(f"viewpoint: no chromosome {name!r} in the table")
        v = self.names.index(name)
        if partners is None:
            mask = [i != v for i in range(len(self.names))]
        elif isinstance(partners, str):
            mask = [i != v and re.search(partners, n) is not None for i, n in enumerate(self.names)]
        else:
            partners = list(partners)
            for n in partners:
                if n not in self.names:
                    raise MktError(f"viewpoint: no chromosome {n!r} in the table")
            mask = [n in partners for n in self.names]                            # (the viewpoint among them: the library refuses)
        o = ViewpointOpts()
        self.L.mkt_viewpoint_opts_default(C.byref(o))
        for k, x in opts.items():
            if k not in VIEWPOINT_OPTS:
                raise TypeError(f"viewpoint: unknown option {k}")
            if k == "reserved":
                o.reserved[0] = int(x)
            else:
                setattr(o, k, float(x) if k == "hotspot_ratio" else int(x))
        mb = (C.c_uint8 * len(mask))(*[1 if x else 0 for x in mask])
        o.partner_mask = C.cast(mb, C.c_void_p)
        o.viewpoint = v
        info = _ViewpointInfoC()
        self._chk(self.L.mkt_matrix_viewpoint(self.h, C.byref(o), C.byref(info)), "mkt_matrix_viewpoint")
        self._vp_info = ViewpointInfo(*[getattr(info, k) for k in ViewpointInfo._fields])
        return self._vp_info

    def viewpoint_result(self):
        """the arrays of the last viewpoint(): Viewpoint(link_vbin, link_chrom, link_pbin, link_count: the link table, ascending; track: the
        dense viewpoint track; partner_chrom, partner_pbin, partner_count: the partner track, by (name, bin); info), all uint32"""
        import numpy as np
        self._chk(self.L.mkt_matrix_fetch_viewpoint_track(self.h, 0, 0, None), "mkt_matrix_fetch_viewpoint_track")
        info = getattr(self, "_vp_info", None)
        if info is None:
            raise MktError("viewpoint_result: the profile was not made through viewpoint()")
        links = [np.zeros(info.links, np.uint32) for _ in range(4)]
        track = np.zeros(info.viewpoint_bins, np.uint32)
        part = [np.zeros(info.partner_cells_kept, np.uint32) for _ in range(3)]
        self._chk(self.L.mkt_matrix_fetch_viewpoint_links(self.h, 0, info.links, *[a.ctypes.data_as(C.c_void_p) for a in links]), "mkt_matrix_fetch_viewpoint_links")
        self._chk(self.L.mkt_matrix_fetch_viewpoint_track(self.h, 0, track.size, track.ctypes.data_as(C.c_void_p)), "mkt_matrix_fetch_viewpoint_track")
        self._chk(self.L.mkt_matrix_fetch_viewpoint_partners(self.h, 0, info.partner_cells_kept, *[a.ctypes.data_as(C.c_void_p) for a in part]), "mkt_matrix_fetch_viewpoint_partners")
        return Viewpoint(*links, track, *part, info)

    def viewpoint_timing_ms(self):
        """(scan ms, sort + run-length ms) on the device of the last viewpoint()"""
        a, b = C.c_double(), C.c_double()
        self._chk(self.L.mkt_matrix_viewpoint_timing(self.h, C.byref(a), C.byref(b)), "mkt_matrix_viewpoint_timing")
        return a.value, b.value

    def hic(self, **opts):
        """The .hic container of every resolution (and, with norm, of the weights the balanced ones hold): mkt_matrix_hic in
        include/mkt.h.  opts: block_bins, level, norm, genome_id, norm_label (str or bytes).  Returns the info as a dict."""
        o = HicOpts()
        self.L.mkt_hic_opts_default(C.byref(o))
        for k, v in opts.items():
            if k not in ("block_bins", "level", "norm", "genome_id", "norm_label"):
                raise TypeError(f"hic: unknown option {k}")
            if k in ("genome_id", "norm_label"):
                v = v.encode() if isinstance(v, str) else v
            elif k == "norm":
                v = 1 if v is True else 0 if v is False else v
            setattr(o, k, v)
        info = _HicInfoC()
        self._chk(self.L.mkt_matrix_hic(self.h, C.byref(o), C.byref(info)), "mkt_matrix_hic")
        self._hic_bytes = info.file_bytes
        return {k: getattr(info, k) for k, _ in _HicInfoC._fields_}

    def hic_bytes(self):
        """the file of the last hic(), as made on the device"""
        self._chk(self.L.mkt_matrix_fetch_hic(self.h, 0, None, 0), "mkt_matrix_fetch_hic")
        n = getattr(self, "_hic_bytes", None)
        if n is None:
            raise MktError("hic_bytes: the file was not made through hic()")
        buf = C.create_string_buffer(max(n, 1))
        self._chk(self.L.mkt_matrix_fetch_hic(self.h, 0, buf, n), "mkt_matrix_fetch_hic")
        return buf.raw[:n]

    def write_hic(self, path, **opts):
        """hic(**opts), then the file to `path` in pieces of 64 MiB; returns the info"""
        info = self.hic(**opts)
        n, step = info["file_bytes"], 64 << 20
        buf = C.create_string_buffer(min(step, max(n, 1)))
        with open(path, "wb") as f:
            for off in range(0, n, step):
                k = min(step, n - off)
                self._chk(self.L.mkt_matrix_fetch_hic(self.h, off, buf, k), "mkt_matrix_fetch_hic")
                f.write(buf.raw[:k])
        return info

    def hic_timing_ms(self, res):
        """(sort, serialise, deflate, pack) ms on the device of resolution index res in the last hic()"""
        t = [C.c_double() for _ in range(4)]
        self._chk(self.L.mkt_matrix_hic_timing(self.h, res, *[C.byref(x) for x in t]), "mkt_matrix_hic_timing")
        return tuple(x.value for x in t)

    def close(self):
        if self.h:
            self.L.mkt_matrix_destroy(self.h)
            self.h = C.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()


def rmdup(text: bytes, hskip1=5, keylen1=16, hskip2=5, keylen2=16, interleaved=False, device=0, piece=1 << 24, stream=False):
    """The reference's krmdup on the GPU (mkt_rmdup_*): returns (read1 | interleaved bytes, read2 bytes, (total, uniq, dup, discard)).
    stream=False: everything added, then ONE run (the resident form).  stream=True: begin / push piece by piece / push(final), the
    outputs of every segment taken as they come (MKT_RMDUP_SEGMENT_MB sets the segment size; what bin/krmdup does)."""
    L = load_library()
    h = C.c_void_p()
    rc = L.mkt_rmdup_create(device, C.byref(h))
    if rc != 0:
        raise MktError(f"mkt_rmdup_create: {L.mkt_strerror(rc).decode()}")

    def fetch(ob, outs):
        for which in (0, 1):
            if ob[which]:
                buf = C.create_string_buffer(ob[which])
                rc = L.mkt_rmdup_fetch(h, which, 0, buf, ob[which])
                if rc != 0:
                    raise MktError(f"mkt_rmdup_fetch: {L.mkt_strerror(rc).decode()}: {L.mkt_rmdup_error(h).decode()}")
                outs[which].append(buf.raw[:ob[which]])

    try:
        st = (C.c_uint64 * 4)()
        ob = (C.c_uint64 * 2)()
        outs = ([], [])
        if stream:
            rc = L.mkt_rmdup_begin(h, hskip1, keylen1, hskip2, keylen2, 1 if interleaved else 0)
            if rc != 0:
                raise MktError(f"mkt_rmdup_begin: {L.mkt_strerror(rc).decode()}: {L.mkt_rmdup_error(h).decode()}")
            for k in list(range(0, len(text), piece)) + [None]:
                part = b"" if k is None else text[k:k + piece]
                rc = L.mkt_rmdup_push(h, part, len(part), 1 if k is None else 0, ob)
                if rc != 0:
                    raise MktError(f"mkt_rmdup_push: {L.mkt_strerror(rc).decode()}: {L.mkt_rmdup_error(h).decode()}")
                fetch(ob, outs)
            L.mkt_rmdup_stats(h, st)
        else:
            for k in range(0, len(text), piece):
                part = text[k:k + piece]
                rc = L.mkt_rmdup_add(h, part, len(part))
                if rc != 0:
                    raise MktError(f"mkt_rmdup_add: {L.mkt_strerror(rc).decode()}: {L.mkt_rmdup_error(h).decode()}")
            rc = L.mkt_rmdup_run(h, hskip1, keylen1, hskip2, keylen2, 1 if interleaved else 0, st, ob)
            if rc != 0:
                raise MktError(f"mkt_rmdup_run: {L.mkt_strerror(rc).decode()}: {L.mkt_rmdup_error(h).decode()}")
            fetch(ob, outs)
        return b"".join(outs[0]), b"".join(outs[1]), tuple(int(x) for x in st)
    finally:
        L.mkt_rmdup_destroy(h)


STITCH_MAX_READ, STITCH_MAX_M = 512, 255
StitchStats = collections.namedtuple("StitchStats", "total combined uncombined passed")


def stitch_check(min_overlap=10, max_overlap=150, max_mismatch_density=0.25, phred_offset=33, cut_tail=10, min_size=36):
    """mkt_stitch_check: the argument check of Stitcher, which needs no device.  Returns None or the refusal's text."""
    L = load_library()
    msg = C.create_string_buffer(256)
    rc = L.mkt_stitch_check(min_overlap, max_overlap, max_mismatch_density, phred_offset, cut_tail, min_size, msg, 256)
    return None if rc == 0 else msg.value.decode()


class Stitcher:
    """Read stitching on the GPU (mkt_stitch_*, include/mkt.h): the driver's `flash | deal.flash.pl` step.  push() the interleaved
    FASTQ in any pieces, finish() at its end; tab / ext / cut1 / cut2 collect the four streams (input order), stats() the counters.
    segment_pairs: pairs per segment (default 2^20)."""

    STREAMS = ("tab", "ext", "cut1", "cut2")

    def __init__(self, min_overlap=10, max_overlap=150, max_mismatch_density=0.25, phred_offset=33, cut_tail=10, min_size=36, device=0, segment_pairs=None):
        self._L = L = load_library()
        self._h = C.c_void_p()
        rc = L.mkt_stitch_create(device, C.byref(self._h))
        if rc != 0:
            self._h = None
            raise MktError(f"mkt_stitch_create: {L.mkt_strerror(rc).decode()} (no GPU, no CPU path)")
        self._parts = ([], [], [], [])
        try:
            if segment_pairs is not None:
                self._check(L.mkt_stitch_segment_pairs(self._h, segment_pairs), "mkt_stitch_segment_pairs")
            self._check(L.mkt_stitch_begin(self._h, min_overlap, max_overlap, max_mismatch_density, phred_offset, cut_tail, min_size), "mkt_stitch_begin")
        except MktError:
            self.close()
            raise

    def _check(self, rc, what):
        if rc != 0:
            raise MktError(f"{what}: {self._L.mkt_strerror(rc).decode()}: {self._L.mkt_stitch_error(self._h).decode()}")

    def push(self, data: bytes, final=False):
        ob = (C.c_uint64 * 4)()
        self._check(self._L.mkt_stitch_push(self._h, data, len(data), 1 if final else 0, ob), "mkt_stitch_push")
        for which in range(4):
            if ob[which]:
                buf = C.create_string_buffer(ob[which])
                self._check(self._L.mkt_stitch_fetch(self._h, which, 0, buf, ob[which]), "mkt_stitch_fetch")
                self._parts[which].append(buf.raw[:ob[which]])

    def finish(self):
        self.push(b"", final=True)
        return self

    def stream(self, which):
        return b"".join(self._parts[which])

    tab = property(lambda self: self.stream(0))
    ext = property(lambda self: self.stream(1))
    cut1 = property(lambda self: self.stream(2))
    cut2 = property(lambda self: self.stream(3))

    def stats(self):
        v = [C.c_uint64() for _ in range(4)]
        self._check(self._L.mkt_stitch_stats(self._h, *[C.byref(x) for x in v]), "mkt_stitch_stats")
        return StitchStats(*[int(x.value) for x in v])

    def stat_line(self):
        st = self.stats()
        return b"Combined\t%d\tUncombined\t%d\tPass\t%d\n" % (st.combined, st.uncombined, st.passed)

    def timing(self):
        """ms so far: (line index, scoring, sizes and scans, writing)"""
        v = [C.c_double() for _ in range(4)]
        self._check(self._L.mkt_stitch_timing(self._h, *[C.byref(x) for x in v]), "mkt_stitch_timing")
        return tuple(x.value for x in v)

    def close(self):
        if self._h:
            self._L.mkt_stitch_destroy(self._h)
            self._h = None

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()


TRIM_MAX_READ, TRIM_MAX_HEADER = 510, 126
TRIM_INTERLEAVED, TRIM_READ1, TRIM_READ2 = 0, 1, 2
TrimStats = collections.namedtuple("TrimStats", "total dropped adapter tailhit dimer passed")


class TrimOpts(C.Structure):
    """mkt_trim_opts (include/mkt.h)"""
    _fields_ = [("adapter1", C.c_char_p), ("adapter2", C.c_char_p), ("kit", C.c_char_p), ("min_size", C.c_uint32), ("phred", C.c_uint32),
                ("min_qual", C.c_uint32), ("window", C.c_uint32), ("mismatch", C.c_double), ("interleaved_input", C.c_int)]


def _trim_opts(L, adapter1=None, adapter2=None, kit=None, min_size=36, phred=33, min_qual=20, window=5, mismatch=0.125, interleaved_input=False):
    o = TrimOpts()
    L.mkt_trim_default_opts(C.byref(o))
    enc = lambda v: v.encode() if isinstance(v, str) else v
    o.adapter1, o.adapter2, o.kit = enc(adapter1), enc(adapter2), enc(kit)
    for name, v in (("min_size", min_size), ("phred", phred), ("min_qual", min_qual), ("window", window)):
        if not 0 <= int(v) <= 0xFFFFFFFF:
            raise MktError(f"{name} {v}: need a number of 0 .. 2^32 - 1")
        setattr(o, name, int(v))
    o.mismatch = float(mismatch)
    o.interleaved_input = 1 if interleaved_input else 0
    return o


def trim_check(**opts):
    """mkt_trim_check: the argument check of Trimmer.begin, which needs no device.  Returns None or the refusal's text."""
    L = load_library()
    try:
        o = _trim_opts(L, **opts)
    except MktError as e:
        return str(e)
    msg = C.create_string_buffer(256)
    rc = L.mkt_trim_check(C.byref(o), msg, 256)
    return None if rc == 0 else msg.value.decode()


class Trimmer:
    """Adapter and quality trimming on the GPU (mkt_trim_*, include/mkt.h): the driver's `ktrim` step.  begin(**opts), push(r1, r2) the
    two FASTQ streams in any pieces (or the interleaved stream as r1 with interleaved_input=True), the last one with final=True;
    interleaved() / read1() / read2() collect the three streams (input order), stats() the counters, log_text() PREFIX.trim.log.
    One object serves any number of runs.  segment_pairs: pairs per segment (default 2^20)."""

    def __init__(self, device=0, segment_pairs=None):
        self._L = L = load_library()
        self._h = C.c_void_p()
        rc = L.mkt_trim_create(device, C.byref(self._h))
        if rc != 0:
            self._h = None
            raise MktError(f"mkt_trim_create: {L.mkt_strerror(rc).decode()} (no GPU, no CPU path)")
        self._parts = ([], [], [])
        if segment_pairs is not None:
            try:
                self._check(L.mkt_trim_segment_pairs(self._h, segment_pairs), "mkt_trim_segment_pairs")
            except MktError:
                self.close()
                raise

    def _check(self, rc, what):
        if rc != 0:
            raise MktError(f"{what}: {self._L.mkt_strerror(rc).decode()}: {self._L.mkt_trim_error(self._h).decode()}")

    def begin(self, **opts):
        self._opts = _trim_opts(self._L, **opts)      # (kept: the strings it points to live as long as it does)
        self._check(self._L.mkt_trim_begin(self._h, C.byref(self._opts)), "mkt_trim_begin")
        self._parts = ([], [], [])
        return self

    def push(self, r1: bytes = b"", r2: bytes = b"", final=False):
        ob = (C.c_uint64 * 3)()
        self._check(self._L.mkt_trim_push(self._h, r1, len(r1), r2, len(r2), 1 if final else 0, ob), "mkt_trim_push")
        for which in range(3):
            if ob[which]:
                buf = C.create_string_buffer(ob[which])
                self._check(self._L.mkt_trim_fetch(self._h, which, 0, buf, ob[which]), "mkt_trim_fetch")
                self._parts[which].append(buf.raw[:ob[which]])
        return self

    def interleaved(self):
        return b"".join(self._parts[TRIM_INTERLEAVED])

    def read1(self):
        return b"".join(self._parts[TRIM_READ1])

    def read2(self):
        return b"".join(self._parts[TRIM_READ2])

    def stats(self):
        v = [C.c_uint64() for _ in range(6)]
        self._check(self._L.mkt_trim_stats(self._h, *[C.byref(x) for x in v]), "mkt_trim_stats")
        return TrimStats(*[int(x.value) for x in v])

    def log_text(self):
        """PREFIX.trim.log"""
        return "".join(f"{n}\t{v}\n" for n, v in zip(("Total", "Dropped", "Aadaptor", "TailHit", "Dimer", "Pass"), self.stats()))

    def timing_ms(self):
        """ms so far: (line indexes, decisions, sizes and scans, writing)"""
        v = [C.c_double() for _ in range(4)]
        self._check(self._L.mkt_trim_timing(self._h, *[C.byref(x) for x in v]), "mkt_trim_timing")
        return tuple(x.value for x in v)

    def close(self):
        if self._h:
            self._L.mkt_trim_destroy(self._h)
            self._h = None

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()


def trim(r1: bytes, r2: bytes, device=0, **opts):
    """One-shot trimming of two FASTQ streams -> (interleaved, read1, read2, TrimStats)."""
    with Trimmer(device=device) as t:
        t.begin(**opts).push(r1, r2, final=True)
        return t.interleaved(), t.read1(), t.read2(), t.stats()


def run_sam2pairs(in_sam, mode, prefix, threads=4, ratio=0.5, mapq=10, sam="yes", env=None, exe=None):
    """Runs the drop-in executable with the reference's argv (microcket:479,483,501,505).  Returns (rc, stdout, stderr)."""
    exe = exe or exe_path()
    if not os.path.exists(exe):
        raise MktError(f"{exe} is missing: run `python -m microcket_amd.build`")
    e = dict(os.environ)
    if env:
        e.update(env)
    p = subprocess.run([exe, in_sam, mode, prefix, str(threads), str(ratio), str(mapq), sam], stdout=subprocess.PIPE,
                       stderr=subprocess.PIPE, env=e)
    return p.returncode, p.stdout, p.stderr


BAM_RUNS_AUTO = (1 << 64) - 1      # MKT_BAM_RUNS_AUTO: one pass while the text fits the GPU, sorted runs from where it would not
_tmp_seq = [0]


def sam_to_bam(sam: bytes, sorted=True, level=2, device=0, piece=1 << 24, notes=None, run_bytes=None, tmp=None, stats=None):
    """SAM text (header lines + alignment lines) -> (BAM bytes, BAI bytes or b"", records) on the GPU: mkt_bam_* in include/mkt.h.
    notes: a list that receives mkt_bam_note() (why no index was made), if given.
    run_bytes: out-of-core mode (mkt_bam_spill): alignment text per sorted run ("auto" or BAM_RUNS_AUTO: runs only where the text
    would not fit); tmp: prefix of the temporary files (default: a fresh name in the system's temporary directory).  stats: a dict
    that receives runs, tmp_bytes and peak_device_bytes, if given."""
    L = load_library()
    h = C.c_void_p()
    rc = L.mkt_bam_create(device, C.byref(h))
    if rc != 0:
        raise MktError(f"mkt_bam_create: {L.mkt_strerror(rc).decode()}")

    def check(rc, what):
        if rc != 0:
            raise MktError(f"{what}: {L.mkt_strerror(rc).decode()}: {L.mkt_bam_error(h).decode()}")

    try:
        if run_bytes is None:
            for k in range(0, len(sam), piece):
                part = sam[k:k + piece]
                check(L.mkt_bam_add(h, part, len(part)), "mkt_bam_add")
            nrec, nbam, nbai = C.c_uint64(), C.c_uint64(), C.c_uint64()
            check(L.mkt_bam_run(h, 1 if sorted else 0, level, C.byref(nrec), C.byref(nbam), C.byref(nbai)), "mkt_bam_run")
            outs = []
            for which, n in ((0, nbam.value), (1, nbai.value)):
                buf = C.create_string_buffer(max(n, 1))
                check(L.mkt_bam_fetch(h, which, 0, buf, n), "mkt_bam_fetch")
                outs.append(buf.raw[:n])
            bam, bai = outs
        else:
            if tmp is None:
                import tempfile
                _tmp_seq[0] += 1
                tmp = os.path.join(tempfile.gettempdir(), f"mkt_bam.{os.getpid()}.{_tmp_seq[0]}")
            budget = BAM_RUNS_AUTO if run_bytes == "auto" else int(run_bytes)
            check(L.mkt_bam_spill(h, budget, str(tmp).encode(), 1 if sorted else 0, level), "mkt_bam_spill")
            parts = []

            def drain():
                ptr, n = C.c_void_p(), C.c_size_t()
                while True:
                    check(L.mkt_bam_pull(h, C.byref(ptr), C.byref(n)), "mkt_bam_pull")
                    if not n.value:
                        return
                    parts.append(C.string_at(ptr.value, n.value))

            for k in range(0, len(sam), piece):
                part = sam[k:k + piece]
                check(L.mkt_bam_add(h, part, len(part)), "mkt_bam_add")
                drain()                    # (input order: pieces are ready while the input arrives)
            nrec, nbam, nbai = C.c_uint64(), C.c_uint64(), C.c_uint64()
            check(L.mkt_bam_run(h, 1 if sorted else 0, level, C.byref(nrec), C.byref(nbam), C.byref(nbai)), "mkt_bam_run")
            drain()
            st = (C.c_uint64 * 5)()
            check(L.mkt_bam_stats(h, st), "mkt_bam_stats")
            buf = C.create_string_buffer(max(st[4], 1))
            check(L.mkt_bam_fetch(h, 1, 0, buf, st[4]), "mkt_bam_fetch")
            bam, bai = b"".join(parts), buf.raw[:st[4]]
        if stats is not None:
            st = (C.c_uint64 * 5)()
            check(L.mkt_bam_stats(h, st), "mkt_bam_stats")
            stats.update(runs=st[0], tmp_bytes=st[1], peak_device_bytes=st[2])
        if notes is not None:
            notes.append(L.mkt_bam_note(h).decode())
        return bam, bai, nrec.value
    finally:
        L.mkt_bam_destroy(h)
