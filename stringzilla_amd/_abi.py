"""ctypes declarations of the C-ABI exported by `libstringzillas_rocm_shared.so` (include/stringzillas/*.h).

This is the reference-side binding a maintainer would write for the ROCm slot: the reference's CPython module
(/root/reference/python/stringzillas/similarities.c:235-428) calls exactly these functions with exactly these
argument lists.  There is no fallback: if the shared library (and the gfx950 code object inside it) is missing,
importing this module raises.
"""

from __future__ import annotations

import ctypes
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIBRARY_PATH = os.environ.get("STRINGZILLAS_ROCM_LIBRARY", os.path.join(_HERE, "lib", "libstringzillas_rocm_shared.so"))

c_size_t, c_void_p, c_char_p, c_int = ctypes.c_size_t, ctypes.c_void_p, ctypes.c_char_p, ctypes.c_int
c_int8 = ctypes.c_int8

# sz_status_t (include/stringzillas/stringzillas.h; reference include/stringzilla/types.h:810-833)
STATUS_NAMES = {
    0: "success", -10: "bad_alloc", -12: "invalid_utf8", -13: "contains_duplicates", -14: "overflow_risk",
    -15: "unexpected_dimensions", -16: "missing_gpu", -17: "device_code_mismatch", -18: "device_memory_mismatch",
    -19: "authentication_failed", -1: "unknown",
}

# sz_capability_t bits this build reports or reads
CAP_SERIAL = 1
CAP_PARALLEL = 1 << 2
CAP_CUDA = 1 << 21  # "a GPU engine exists" - the bit the ROCm build reports
CAPS_CPUS = 0x011FFCFD
CAPS_CUDA = (1 << 21) | (1 << 22) | (1 << 23)


class U32Tape(ctypes.Structure):
    _fields_ = [("data", c_void_p), ("offsets", c_void_p), ("count", c_size_t)]


class U64Tape(ctypes.Structure):
    _fields_ = [("data", c_void_p), ("offsets", c_void_p), ("count", c_size_t)]


MEMBER_START = ctypes.CFUNCTYPE(c_void_p, c_void_p, c_size_t)
MEMBER_LENGTH = ctypes.CFUNCTYPE(c_size_t, c_void_p, c_size_t)


class Sequence(ctypes.Structure):
    _fields_ = [("handle", c_void_p), ("count", c_size_t), ("get_start", MEMBER_START), ("get_length", MEMBER_LENGTH)]


class CallProfile(ctypes.Structure):
    _fields_ = [
        ("kernel_milliseconds", ctypes.c_double), ("host_milliseconds", ctypes.c_double),
        ("cells", ctypes.c_uint64), ("pairs", ctypes.c_uint64), ("algorithmic_bytes", ctypes.c_uint64),
        ("unique_bytes", ctypes.c_uint64), ("launches", ctypes.c_uint32), ("longest_query", ctypes.c_uint32),
        ("longest_candidate", ctypes.c_uint32), ("tier", ctypes.c_uint32), ("transposed", ctypes.c_uint32), ("cell_bits", ctypes.c_uint32),
        ("planner", ctypes.c_uint32), ("team", ctypes.c_uint32), ("team_wide", ctypes.c_uint32), ("streams", ctypes.c_uint32),
        ("queue_items", ctypes.c_uint32), ("queue_tiles", ctypes.c_uint32),
    ]


NODE_MOST_GPUS = 16


class NodeStats(ctypes.Structure):
    _fields_ = [
        ("gpus", c_size_t), ("wall_milliseconds", ctypes.c_double),
        ("busy_milliseconds", ctypes.c_double * NODE_MOST_GPUS), ("kernel_milliseconds", ctypes.c_double * NODE_MOST_GPUS),
        ("cells", ctypes.c_uint64 * NODE_MOST_GPUS), ("row_weights", ctypes.c_uint64 * NODE_MOST_GPUS),
        ("rows", ctypes.c_uint32 * NODE_MOST_GPUS),
        ("peer_copies", ctypes.c_uint32 * NODE_MOST_GPUS), ("staged_copies", ctypes.c_uint32 * NODE_MOST_GPUS),
        ("peer_pairs", ctypes.c_uint32), ("symmetric", ctypes.c_uint32),
    ]


ERR = ctypes.POINTER(c_char_p)
ENGINE_OUT = ctypes.POINTER(c_void_p)

# name -> (restype, argtypes); every symbol of include/stringzillas/stringzillas.h and stringzillas_rocm.h
_LEV_INIT = (c_int, [c_int8, c_int8, c_int8, c_int8, c_void_p, c_int, ENGINE_OUT, ERR])
_SCORE_INIT = (c_int, [c_void_p, c_void_p, c_int8, c_int8, c_void_p, c_int, ENGINE_OUT, ERR])
_CALL = (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_size_t, ERR])
_FP_CALL = (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_size_t, c_void_p, c_size_t, ERR])
_TOP_K = (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_size_t, c_void_p, c_void_p, c_size_t, ERR])
_RERANK = (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_size_t, c_void_p, c_size_t, ERR])
_FUZZY_FIND = (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_size_t, c_void_p, c_void_p, c_size_t, ERR])
_FUZZY_FIND_SPANS = (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_size_t, c_void_p, c_void_p, c_void_p, c_size_t, ERR])
_FUZZY_SEARCH = (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_size_t, c_void_p, c_void_p, c_void_p, c_void_p, c_size_t, ERR])
_WITHIN = (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, ctypes.c_ssize_t, c_size_t, c_void_p, c_void_p, c_void_p, c_size_t, ERR])
_CLUSTERS = (c_int, [c_void_p, c_void_p, c_void_p, ctypes.c_ssize_t, c_void_p, c_void_p, ERR])
_FUZZY_SEARCH_WITHIN = (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_size_t, c_size_t, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                c_size_t, ERR])
_FUZZY_SCAN = (c_int,[c_void_p, c_void_p, c_void_p, c_void_p, c_size_t, c_void_p, c_void_p, ERR])
_FUZZY_SCAN_SPANS = (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_size_t, c_void_p, c_void_p, c_void_p, ERR])
_FUZZY_SCAN_MATCHES = (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_size_t, c_size_t, c_size_t, c_void_p, c_void_p, c_void_p, ERR])
_ALIGNMENTS = (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_size_t, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                        c_size_t, c_size_t, ERR])
_FUZZY_SCAN_OCCURRENCES = (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_size_t, c_size_t, c_size_t, c_void_p, c_void_p, c_void_p, c_void_p,
                                   ERR])

SIGNATURES = {
    "szs_version_major": (c_int, []), "szs_version_minor": (c_int, []), "szs_version_patch": (c_int, []),
    "szs_capabilities_comptime": (c_int, []), "szs_capabilities_runtime": (c_int, []), "szs_capabilities": (c_int, []),
    "sz_memory_allocator_init_unified": (c_int, [c_void_p, ERR]),
    "szs_unified_alloc": (c_void_p, [c_size_t]), "szs_unified_free": (None, [c_void_p, c_size_t]),
    "szs_device_scope_init_default": (c_int, [ENGINE_OUT, ERR]),
    "szs_device_scope_init_cpu_cores": (c_int, [c_size_t, ENGINE_OUT, ERR]),
    "szs_device_scope_init_gpu_device": (c_int, [c_size_t, ENGINE_OUT, ERR]),
    "szs_device_scope_get_cpu_cores": (c_int, [c_void_p, ctypes.POINTER(c_size_t), ERR]),
    "szs_device_scope_get_gpu_device": (c_int, [c_void_p, ctypes.POINTER(c_size_t), ERR]),
    "szs_device_scope_get_capabilities": (c_int, [c_void_p, ctypes.POINTER(c_int), ERR]),
    "szs_device_scope_free": (None, [c_void_p]),
    "szs_levenshtein_distances_init": _LEV_INIT, "szs_levenshtein_distances": _CALL,
    "szs_levenshtein_distances_u32tape": _CALL, "szs_levenshtein_distances_u64tape": _CALL,
    "szs_levenshtein_distances_free": (None, [c_void_p]),
    "szs_levenshtein_distances_utf8_init": _LEV_INIT, "szs_levenshtein_distances_utf8": _CALL,
    "szs_levenshtein_distances_utf8_u32tape": _CALL, "szs_levenshtein_distances_utf8_u64tape": _CALL,
    "szs_levenshtein_distances_utf8_free": (None, [c_void_p]),
    "szs_needleman_wunsch_scores_init": _SCORE_INIT, "szs_needleman_wunsch_scores": _CALL,
    "szs_needleman_wunsch_scores_u32tape": _CALL, "szs_needleman_wunsch_scores_u64tape": _CALL,
    "szs_needleman_wunsch_scores_free": (None, [c_void_p]),
    "szs_smith_waterman_scores_init": _SCORE_INIT, "szs_smith_waterman_scores": _CALL,
    "szs_smith_waterman_scores_u32tape": _CALL, "szs_smith_waterman_scores_u64tape": _CALL,
    "szs_smith_waterman_scores_free": (None, [c_void_p]),
    "szs_fingerprints_init": (c_int, [c_size_t, c_size_t, c_void_p, c_size_t, ctypes.c_uint64, c_void_p, c_int, ENGINE_OUT, ERR]),
    "szs_fingerprints_sequence": _FP_CALL, "szs_fingerprints_u64tape": _FP_CALL, "szs_fingerprints_u32tape": _FP_CALL,
    "szs_fingerprints_free": (None, [c_void_p]),
    # ROCm-only additions (include/stringzillas/stringzillas_rocm.h)
    "szs_rocm_last_call_profile": (c_int, [c_void_p, ctypes.POINTER(CallProfile)]),
    "szs_rocm_last_pairing": (ctypes.c_uint32, [c_void_p]),
    "szs_rocm_pair_rule_probe": (c_int, [c_void_p, c_size_t, ctypes.POINTER(ctypes.c_uint32), ctypes.POINTER(ctypes.c_uint64), c_void_p]),
    "szs_rocm_corner_cut_probe": (c_int, [ctypes.c_uint32] * 5 + [ctypes.POINTER(ctypes.c_uint32)] * 2),
    "szs_rocm_shard_rows": (c_int, [c_void_p, c_size_t, c_size_t, c_void_p, c_void_p]),
    "szs_rocm_shard_triangle": (c_int, [c_void_p, c_size_t, c_size_t, c_void_p, c_void_p]),
    "szs_rocm_plan_probe": (c_int, [c_int, c_int, c_void_p, c_size_t, c_void_p, c_size_t, c_void_p, c_void_p, c_void_p, c_void_p]),
    "szs_rocm_orientation_probe": (c_int, [c_int, c_int, c_int, c_int, c_void_p, c_size_t, c_void_p, c_size_t, c_void_p, c_void_p]),
    "szs_rocm_team_orientation_probe": (c_int, [c_int, c_int, c_void_p, c_size_t, c_void_p, c_size_t, c_void_p, c_void_p, c_void_p]),
    "szs_rocm_launch_order_probe": (c_int, [c_int, c_void_p, c_size_t, c_size_t, c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]),
    "szs_rocm_queue_probe": (c_int, [c_int, ctypes.c_uint32, c_void_p, c_size_t, c_void_p, c_size_t, c_void_p, c_size_t, c_void_p, c_void_p]),
    "szs_rocm_tuning_set": (c_int, [c_char_p, c_char_p]),
    "szs_rocm_team_shape": (ctypes.c_uint32, [c_size_t]),
    "szs_rocm_node_init": (c_int, [c_void_p, c_size_t, ENGINE_OUT, ERR]),
    "szs_rocm_node_size": (c_size_t, [c_void_p]), "szs_rocm_node_free": (None, [c_void_p]),
    "szs_rocm_node_levenshtein_distances_init": (c_int, [c_void_p, c_int8, c_int8, c_int8, c_int8, ENGINE_OUT, ERR]),
    "szs_rocm_node_levenshtein_distances_utf8_init": (c_int, [c_void_p, c_int8, c_int8, c_int8, c_int8, ENGINE_OUT, ERR]),
    "szs_rocm_node_needleman_wunsch_scores_init": (c_int, [c_void_p, c_void_p, c_void_p, c_int8, c_int8, ENGINE_OUT, ERR]),
    "szs_rocm_node_smith_waterman_scores_init": (c_int, [c_void_p, c_void_p, c_void_p, c_int8, c_int8, ENGINE_OUT, ERR]),
    "szs_rocm_node_engine_free": (None, [c_void_p]),
    "szs_rocm_node_scores_u32tape": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_size_t, ctypes.POINTER(NodeStats), ERR]),
    "szs_rocm_node_scores_u64tape": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_size_t, ctypes.POINTER(NodeStats), ERR]),
    "szs_rocm_top_k": _TOP_K, "szs_rocm_top_k_u32tape": _TOP_K, "szs_rocm_top_k_u64tape": _TOP_K,
    "szs_rocm_within": _WITHIN, "szs_rocm_within_u32tape": _WITHIN, "szs_rocm_within_u64tape": _WITHIN,
    "szs_rocm_within_probe": (c_int, [c_size_t, c_size_t, c_size_t, ctypes.POINTER(c_size_t), ctypes.POINTER(c_size_t),
                                      ctypes.POINTER(c_size_t), ctypes.POINTER(c_size_t)]),
    "szs_rocm_clusters": _CLUSTERS, "szs_rocm_clusters_u32tape": _CLUSTERS, "szs_rocm_clusters_u64tape": _CLUSTERS,
    "szs_rocm_fingerprint_clusters": (c_int, [c_void_p, c_void_p, c_void_p, c_size_t, c_size_t, c_size_t, c_void_p, c_void_p, ERR]),
    "szs_rocm_clusters_probe": (c_int, [c_size_t, c_int, ctypes.POINTER(c_size_t), ctypes.POINTER(c_size_t), ctypes.POINTER(c_size_t),
                                        ctypes.POINTER(c_size_t)]),
    "szs_rocm_fuzzy_search_within": _FUZZY_SEARCH_WITHIN, "szs_rocm_fuzzy_search_within_u32tape": _FUZZY_SEARCH_WITHIN,
    "szs_rocm_fuzzy_search_within_u64tape": _FUZZY_SEARCH_WITHIN,
    "szs_rocm_rerank": _RERANK, "szs_rocm_rerank_u32tape": _RERANK, "szs_rocm_rerank_u64tape": _RERANK,
    "szs_rocm_fuzzy_find": _FUZZY_FIND, "szs_rocm_fuzzy_find_u32tape": _FUZZY_FIND, "szs_rocm_fuzzy_find_u64tape": _FUZZY_FIND,
    "szs_rocm_fuzzy_find_spans": _FUZZY_FIND_SPANS, "szs_rocm_fuzzy_find_spans_u32tape": _FUZZY_FIND_SPANS,
    "szs_rocm_fuzzy_find_spans_u64tape": _FUZZY_FIND_SPANS,
    "szs_rocm_alignments": _ALIGNMENTS, "szs_rocm_alignments_u32tape": _ALIGNMENTS, "szs_rocm_alignments_u64tape": _ALIGNMENTS,
    "szs_rocm_fuzzy_search": _FUZZY_SEARCH, "szs_rocm_fuzzy_search_u32tape": _FUZZY_SEARCH, "szs_rocm_fuzzy_search_u64tape": _FUZZY_SEARCH,
    "szs_rocm_fuzzy_search_probe": (c_int, [c_size_t, c_size_t, c_size_t, c_size_t, ctypes.POINTER(c_size_t), ctypes.POINTER(c_size_t),
                                            ctypes.POINTER(c_size_t), ctypes.POINTER(c_size_t)]),
    "szs_rocm_fuzzy_scan": _FUZZY_SCAN, "szs_rocm_fuzzy_scan_u32tape": _FUZZY_SCAN, "szs_rocm_fuzzy_scan_u64tape": _FUZZY_SCAN,
    "szs_rocm_fuzzy_scan_spans": _FUZZY_SCAN_SPANS, "szs_rocm_fuzzy_scan_spans_u32tape": _FUZZY_SCAN_SPANS,
    "szs_rocm_fuzzy_scan_spans_u64tape": _FUZZY_SCAN_SPANS,
    "szs_rocm_fuzzy_scan_matches": _FUZZY_SCAN_MATCHES, "szs_rocm_fuzzy_scan_matches_u32tape": _FUZZY_SCAN_MATCHES,
    "szs_rocm_fuzzy_scan_matches_u64tape": _FUZZY_SCAN_MATCHES,
    "szs_rocm_fuzzy_scan_occurrences": _FUZZY_SCAN_OCCURRENCES, "szs_rocm_fuzzy_scan_occurrences_u32tape": _FUZZY_SCAN_OCCURRENCES,
    "szs_rocm_fuzzy_scan_occurrences_u64tape": _FUZZY_SCAN_OCCURRENCES,
    "szs_rocm_fuzzy_scan_probe": (c_int, [c_size_t, c_size_t, c_size_t, ctypes.POINTER(c_size_t), ctypes.POINTER(c_size_t),
                                          ctypes.POINTER(c_size_t), ctypes.POINTER(c_size_t)]),
    "szs_rocm_rerank_probe": (c_int, [c_int, c_int, c_void_p, c_size_t, c_size_t, c_size_t, c_void_p, c_void_p, c_void_p, c_void_p]),
    "szs_rocm_fingerprint_matches": (c_int, [c_void_p, c_void_p, c_void_p, c_size_t, c_size_t, c_void_p, c_size_t, c_size_t,
                                             c_void_p, c_size_t, ERR]),
    "szs_rocm_fingerprint_top_k": (c_int, [c_void_p, c_void_p, c_void_p, c_size_t, c_size_t, c_void_p, c_size_t, c_size_t, c_size_t,
                                           c_void_p, c_void_p, c_size_t, ERR]),
}

REFERENCE_SYMBOLS = [name for name in SIGNATURES if not name.startswith("szs_rocm_")]  # the reference's 41

if not os.path.exists(LIBRARY_PATH):
    raise ImportError(
        f"{LIBRARY_PATH} is missing: build it with `make -C stringzilla_amd/csrc` (or `python -c 'import "
        "__graft_entry__ as g; g.build()'`). stringzilla_amd has no CPU fallback."
    )

# ONE HIP runtime per process.  PyTorch wheels bundle their own libamdhip64.so (SONAME libamdhip64.so.7, the SONAME this
# library NEEDs).  If torch is imported first, the dynamic linker binds this library to the runtime torch already loaded,
# so pointers, streams and device state are shared; if this library were loaded first, /opt/rocm's runtime would come in
# and torch would later load a SECOND one beside it, and then sees no GPU.  Hence: torch first, whenever it is installed.
try:
    import torch as _torch  # noqa: F401
except ImportError:  # C-only deployments: the RUNPATH'd /opt/rocm runtime is used
    _torch = None

lib = ctypes.CDLL(LIBRARY_PATH)
for _name, (_restype, _argtypes) in SIGNATURES.items():
    _fn = getattr(lib, _name)  # AttributeError here = the library does not export what the header declares
    _fn.restype = _restype
    _fn.argtypes = _argtypes


class StringZillasError(RuntimeError):
    def __init__(self, status: int, message: str | None):
        self.status = status
        self.status_name = STATUS_NAMES.get(status, str(status))
        super().__init__(f"sz_status_t {self.status_name} ({status}): {message or 'no message'}")


_KNOBS = {"tier": "SZS_ROCM_TIER", "swap": "SZS_ROCM_SWAP", "packed": "SZS_ROCM_PACKED", "rune_ids": "SZS_ROCM_RUNE_IDS",
          "chain_waves": "SZS_ROCM_CHAIN_WAVES", "trace": "SZS_ROCM_TRACE", "cells": "SZS_ROCM_CELLS",
          "planner": "SZS_ROCM_PLANNER", "speculate": "SZS_ROCM_SPECULATE", "cpu_requests": "SZS_ROCM_CPU_REQUESTS",
          "streams": "SZS_ROCM_STREAMS", "reuse": "SZS_ROCM_REUSE",
          "split": "SZS_ROCM_SPLIT", "alphabet": "SZS_ROCM_ALPHABET", "merge": "SZS_ROCM_MERGE",
          "team": "SZS_ROCM_TEAM", "queues": "SZS_ROCM_QUEUES", "roctx": "SZS_ROCM_ROCTX",
          "queue": "SZS_ROCM_QUEUE", "queue_words": "SZS_ROCM_QUEUE_WORDS", "queue_rounds": "SZS_ROCM_QUEUE_ROUNDS",
          "queue_priority": "SZS_ROCM_QUEUE_PRIORITY", "fused": "SZS_ROCM_FUSED", "tiny": "SZS_ROCM_TINY",
          "top_k_tile": "SZS_ROCM_TOP_K_TILE", "rerank": "SZS_ROCM_RERANK",
          "fuzzy_search_segment": "SZS_ROCM_FUZZY_SEARCH_SEGMENT", "fuzzy_scan_piece": "SZS_ROCM_FUZZY_SCAN_PIECE",
          "align_trace_kib": "SZS_ROCM_ALIGN_TRACE_KIB"}
_knob_values = {name: os.environ.get(variable) for name, variable in _KNOBS.items()}  # what the library read when it was loaded


def tuning_set(knob: str, value=None):
    """`szs_rocm_tuning_set`: pins one of the library's tuning / testing knobs ("tier", "swap", "packed", "rune_ids",
    "chain_waves", "trace", "cells", "planner", "speculate" or the `SZS_ROCM_*` spelling); None restores the automatic
    choice.  The environment is only read once, when the library is loaded.  Returns the previous setting."""
    name = next((short for short, variable in _KNOBS.items() if knob in (short, variable)), None)
    if name is None or lib.szs_rocm_tuning_set(name.encode(), None if value is None else str(value).encode()) != 0:
        raise ValueError(f"unknown tuning knob {knob!r}")
    previous, _knob_values[name] = _knob_values[name], None if value is None else str(value)
    return previous


def rerank_probe(query_lengths, k, longest_candidate, unit_cost=True, runes=False):
    """`szs_rocm_rerank_probe`: how a rerank call would route queries of these byte lengths - no GPU involved.  Returns
    (routes, strips, strip_words, scratch_bytes): per query 0 (an engine call of its own), 1 (hip/myers_rerank.hip) or
    2 (hip/myers_rerank_strips.hip), the strips it is walked in and their width in 32-bit words, and the bytes of parked deltas
    the strips launch would allocate.  The `rerank` knob applies as it does to the call."""
    import numpy as np

    lengths = np.ascontiguousarray(query_lengths, dtype=np.uint32)
    routes, strips = np.zeros(len(lengths), np.uint8), np.zeros(len(lengths), np.uint32)
    strip_words, scratch = np.zeros(len(lengths), np.uint32), c_size_t(0)
    status = lib.szs_rocm_rerank_probe(int(unit_cost), int(runes), lengths.ctypes.data, len(lengths), k, longest_candidate, routes.ctypes.data,
                                       strips.ctypes.data, strip_words.ctypes.data, ctypes.addressof(scratch))
    if status != 0:
        raise StringZillasError(status, None)
    return routes, strips, strip_words, int(scratch.value)


def fuzzy_search_probe(queries_count, candidates_count, k, longest_query=0):
    """`szs_rocm_fuzzy_search_probe`: how a fuzzy search of these counts would be cut - no GPU involved.  Returns (block, tile, segment,
    workgroups): the queries of a block, the candidates of a tile, the candidates one workgroup of the tile kernel scores for its row
    and the workgroups of the first tile's launch.  The `top_k_tile` and `fuzzy_search_segment` knobs apply as they do to the call."""
    block, tile, segment, workgroups = c_size_t(0), c_size_t(0), c_size_t(0), c_size_t(0)
    status = lib.szs_rocm_fuzzy_search_probe(queries_count, candidates_count, k, longest_query, ctypes.byref(block), ctypes.byref(tile),
                                             ctypes.byref(segment), ctypes.byref(workgroups))
    if status != 0:
        raise StringZillasError(status, None)
    return int(block.value), int(tile.value), int(segment.value), int(workgroups.value)


def within_probe(queries_count, candidates_count, limit):
    """`szs_rocm_within_probe`: how `within` and `fuzzy_search_within` would cut a call of these counts - no GPU involved.  Returns
    (block, tile, segments, segment_columns): the queries of a block, the candidates of a tile, the workgroups that share a row of the
    fold and the columns of each.  The `top_k_tile` knob applies as it does to the calls."""
    block, tile, segments, segment_columns = c_size_t(0), c_size_t(0), c_size_t(0), c_size_t(0)
    status = lib.szs_rocm_within_probe(queries_count, candidates_count, limit, ctypes.byref(block), ctypes.byref(tile),
                                       ctypes.byref(segments), ctypes.byref(segment_columns))
    if status != 0:
        raise StringZillasError(status, None)
    return int(block.value), int(tile.value), int(segments.value), int(segment_columns.value)


def clusters_probe(count, symmetric):
    """`szs_rocm_clusters_probe`: what `clusters` would score over `count` strings - no GPU involved.  Returns (block, tile,
    tiles_scored, pairs_scored): the rows of a block, the columns of a tile, and the tiles and pairs of the triangle (`symmetric`) or of
    the whole square.  The `top_k_tile` knob applies as it does to the call."""
    block, tile, tiles, pairs = c_size_t(0), c_size_t(0), c_size_t(0), c_size_t(0)
    status = lib.szs_rocm_clusters_probe(count, 1 if symmetric else 0, ctypes.byref(block), ctypes.byref(tile), ctypes.byref(tiles),
                                         ctypes.byref(pairs))
    if status != 0:
        raise StringZillasError(status, None)
    return int(block.value), int(tile.value), int(tiles.value), int(pairs.value)


def fuzzy_scan_probe(queries_count, longest_query, text_length):
    """`szs_rocm_fuzzy_scan_probe`: how a fuzzy scan would cut a text of `text_length` bytes for `queries_count` queries - no GPU
    involved.  Returns (piece, pieces, workgroups, walked_bytes_per_query): the bytes of a piece, the pieces, the workgroups of the
    first block's scan and the bytes a query of `longest_query` bytes walks, warm-ups included.  The `fuzzy_scan_piece` knob applies
    as it does to the call."""
    piece, pieces, workgroups, walked = c_size_t(0), c_size_t(0), c_size_t(0), c_size_t(0)
    status = lib.szs_rocm_fuzzy_scan_probe(queries_count, longest_query, text_length, ctypes.byref(piece), ctypes.byref(pieces),
                                           ctypes.byref(workgroups), ctypes.byref(walked))
    if status != 0:
        raise StringZillasError(status, None)
    return int(piece.value), int(pieces.value), int(workgroups.value), int(walked.value)


PAIR_RULE_CHOOSE = 0xFFFFFFFF


def pair_rule_probe(lengths, rule=PAIR_RULE_CHOOSE):
    """`szs_rocm_pair_rule_probe`: which two queries of these byte lengths share a workgroup of the short launch that plans itself -
    no GPU involved.  `rule`: PAIR_RULE_CHOOSE for the sorter's own choice, or a rule to evaluate.  Returns (rule, total_words,
    slot_pairs): slot_pairs[s] holds the descending ranks of slot s's two queries, -1 where it has no second one."""
    import numpy as np

    lengths = np.ascontiguousarray(lengths, dtype=np.uint32)
    slot_pairs = np.zeros(((len(lengths) + 1) // 2, 2), np.uint32)
    chosen, total = ctypes.c_uint32(rule), ctypes.c_uint64(0)
    status = lib.szs_rocm_pair_rule_probe(lengths.ctypes.data, len(lengths), ctypes.byref(chosen), ctypes.byref(total), slot_pairs.ctypes.data)
    if status != 0:
        raise StringZillasError(status, None)
    return int(chosen.value), int(total.value), slot_pairs.astype(np.int64) - (slot_pairs == 0xFFFFFFFF) * (1 << 32)


CORNER_CUT_NEVER = 0xFFFFFFFF


def corner_cut_probe(first_length, second_length, words, n_short, n_long):
    """`szs_rocm_corner_cut_probe`: the text columns (counted from 0) in which the short Myers bodies leave an end word of a
    `words`-word bit-vector untouched - no GPU involved.  `second_length`: None for a single query.  Returns (head_until, late_from):
    columns below head_until skip the top word, columns from late_from on the bottom word (CORNER_CUT_NEVER: none does)."""
    head, late = ctypes.c_uint32(0), ctypes.c_uint32(0)
    status = lib.szs_rocm_corner_cut_probe(first_length, 0xFFFFFFFF if second_length is None else second_length, words, n_short, n_long,
                                           ctypes.byref(head), ctypes.byref(late))
    if status != 0:
        raise StringZillasError(status, None)
    return int(head.value), int(late.value)


def team_shapes():
    """The compiled instances of the team tier: values for the `team` knob (lanes * 10000 + registers * 100 + waves)."""
    shapes, index = [], 0
    while lib.szs_rocm_team_shape(index):
        shapes.append(int(lib.szs_rocm_team_shape(index)))
        index += 1
    return shapes


def check(status: int, error: c_char_p) -> None:
    if status != 0:
        raise StringZillasError(status, error.value.decode() if error.value else None)
