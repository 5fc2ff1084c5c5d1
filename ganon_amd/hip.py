"""ctypes mirror of include/ganon_hip.h (the C ABI of libganon_hip.so).  No torch types, no CPU fallback."""
from __future__ import annotations

import ctypes as C
import os
from typing import Optional, Sequence, Tuple

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_LIB_PATH = os.environ.get("GANON_HIP_LIB") or os.path.join(_HERE, "csrc", "libganon_hip.so")  # override: A/B builds

READ_OK, READ_SMALL, READ_BIG = 0, 1, 2
FILL_3_OF_8 = 0x38  # gn_filter_fill_random: density 3/8 (GN_FILL_3_OF_8)
FILL_3_OF_16 = 0x3F  # density 3/16: m0 & m1 & (m2 | m3) (GN_FILL_3_OF_16)
MATCH_DTYPE = np.dtype([("read", "<u4"), ("target", "<u4"), ("count", "<u4")])
PACKED_BLOCK_DTYPE = np.dtype([("first", "<u8"), ("word_at", "<u8"), ("cnt", "<u4"), ("width", "<u4")])  # gn_packed_block

# every symbol include/ganon_hip.h declares (tests check the library exports all of them)
ABI_SYMBOLS = ["gn_device_count", "gn_last_error", "gn_filter_upload_ibf", "gn_filter_upload_hibf", "gn_filter_emplace",
               "gn_filter_emplace_ibf", "gn_filter_download_rows", "gn_filter_download_row_list", "gn_pinned_alloc",
               "gn_pinned_free", "gn_filter_write_rows", "gn_filter_write_sync", "gn_filter_finalize",
               "gn_filter_fill_random", "gn_filter_info", "gn_filter_free", "gn_stream_create", "gn_stream_destroy",
               "gn_stream_upload_reads", "gn_stream_minimisers", "gn_stream_classify", "gn_submit_batch", "gn_stream_sync", "gn_fetch_batch", "gn_stream_set_postfilter",
               "gn_fetch_postfilter", "gn_streams_postfilter_joint", "gn_stream_set_long_reads", "gn_stream_device_matches",
               "gn_stream_distinct_hashes", "gn_filter_emplace_split", "gn_stream_fetch_hashes", "gn_stream_dense_counts",
               "gn_stream_timings", "gn_stream_screen_deferred", "gn_filter_set_stream_rows_min_bytes", "gn_stream_rows_streamed", "gn_gather_create", "gn_gather_create_merged", "gn_gather_run", "gn_gather_fetch", "gn_gather_device_matches",
               "gn_gather_destroy", "gn_device_memory", "gn_hibf_row_stride_words", "gn_gather_run_buffers", "gn_stream_device_offsets", "gn_stream_hibf_levels", "gn_stream_hibf_level_lines", "gn_stream_classify_shared",
               "gn_stream_upload_fastq", "gn_stream_fastq_index", "gn_stream_fastq_keep", "gn_stream_fastq_records",
               "gn_peer_stats", "gn_stream_upload_text", "gn_stream_upload_text_pair", "gn_stream_text_pair_index", "gn_stream_text_pair_records2",
               "gn_ablate", "gn_filter_probe", "gn_reassign_create", "gn_reassign_run", "gn_reassign_diffs", "gn_reassign_fetch", "gn_reassign_info", "gn_reassign_free",
               "gn_inflate_create", "gn_inflate_destroy", "gn_inflate_feed", "gn_inflate_step", "gn_inflate_text", "gn_inflate_text_device",
               "gn_inflate_get_stats", "gn_inflate_cuts", "gn_inflate_set_carry", "gn_stream_upload_text_device", "gn_stream_fastq_headers",
               "gn_inflate_cuts_lines", "gn_inflate_cut_at_lines", "gn_stream_upload_text_pair_device", "gn_stream_fetch_letters",
               "gn_ibf_hash_constants", "gn_inflate_set_turns", "gn_inflate_handoff",
               "gn_stream_upload_text_pair_devices", "gn_hashes_union", "gn_filter_emplace_path", "gn_filter_probe_path", "gn_filter_probe_paths_shared",
               "gn_filter_bin_popcounts", "gn_filter_copy_ibf", "gn_filter_copy_ibf_spans", "gn_filter_fold_ibf", "gn_filter_extend_path",
               "gn_sketches_create", "gn_sketches_free", "gn_sketches_download", "gn_sketches_union_table", "gn_sketches_pair_table",
               "gn_filter_emplace_runs_window", "gn_filter_create_hibf_storage", "gn_filter_emplace_path_window",
               "gn_stream_distinct_hashes_packed", "gn_filter_emplace_packed_window",
               "gn_packed_union", "gn_sketches_create_packed", "gn_filter_emplace_path_packed_window",
               "gn_filter_probe_path_window", "gn_filter_probe_paths_shared_window",
               "gn_stream_upload_genome_text", "gn_stream_genome_index", "gn_stream_genome_records"]


GENOME_CONTINUES, GENOME_OPEN_END = 1, 2  # flags of gn_stream_upload_genome_text
GENOME_BAD_LETTER, GENOME_NO_HEADER = 1, 2  # status of gn_stream_genome_index


class PostFilter(C.Structure):  # gn_postfilter
    _fields_ = [("rel_filter", C.c_double), ("fpr_query", C.c_double), ("target_fpr", C.c_void_p), ("joint", C.c_int),
                ("target_gid", C.c_void_p)]


class GanonHipError(RuntimeError):
    def __init__(self, code: int, msg: str):
        super().__init__(f"libganon_hip error {code}: {msg}")
        self.code = code


class IbfDesc(C.Structure):
    _fields_ = [("rows", C.c_void_p), ("bin_size", C.c_uint64), ("bin_words", C.c_uint64), ("bins", C.c_uint64),
                ("hash_funs", C.c_uint32), ("hash_shift", C.c_uint32)]


class Timings(C.Structure):
    _fields_ = [("ms_minimiser", C.c_float), ("ms_count", C.c_float), ("ms_total", C.c_float),
                ("n_hashes", C.c_uint64), ("algo_bytes", C.c_uint64), ("n_matches", C.c_uint64),
                ("n_count_launches", C.c_uint32), ("fetched_bytes", C.c_uint64), ("ms_compact", C.c_float)]


class InflateStats(C.Structure):  # gn_inflate_stats
    _fields_ = [("steps", C.c_uint64), ("chunks", C.c_uint64), ("fixups", C.c_uint64), ("markers", C.c_uint64), ("members", C.c_uint64),
                ("text_bytes", C.c_uint64), ("ms_decode", C.c_double), ("ms_chain", C.c_double), ("ms_resolve", C.c_double),
                ("ms_step_wall", C.c_double), ("prof_ms", C.c_double * 8)]


_lib = None


_ablated: Tuple[str, ...] = tuple(x.strip() for x in os.environ.get("GANON_HIP_ABLATE", "").split(",") if x.strip())


def set_ablation(names) -> None:
    """gn_ablate(): replace the library's switch list (include/ganon_hip.h); "" = the product path"""
    global _ablated
    if isinstance(names, str):
        names = [x.strip() for x in names.split(",") if x.strip()]
    names = tuple(names)
    L = load_library()
    rc = L.gn_ablate(",".join(names).encode())
    if rc:
        raise GanonHipError(rc, L.gn_last_error().decode())
    _ablated = names


def ablation() -> Tuple[str, ...]:
    return _ablated


class ablate:
    """context manager: the named switches on top of the current list, the previous list back on exit
    (`with ganon_amd.ablate("early_exit"): ...`; an empty name list changes nothing)"""

    def __init__(self, *names: str):
        self.names = [x.strip() for n in names for x in n.split(",") if x.strip()]

    def __enter__(self):
        self.prev = _ablated
        key = lambda s: s.split("=")[0]
        set_ablation([p for p in self.prev if key(p) not in {key(n) for n in self.names}] + self.names)
        return self

    def __exit__(self, *exc):
        set_ablation(self.prev)
        return False


def library_path() -> str:
    return _LIB_PATH


def load_library():
    """dlopen the in-tree libganon_hip.so; raises (loudly) when it has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(_LIB_PATH):
        raise GanonHipError(-19, f"{_LIB_PATH} is missing: run `python -m ganon_amd.build` (hipcc, gfx950). "
                                 "There is no CPU fallback.")
    L = C.CDLL(_LIB_PATH)
    vp, u32, u64, i32 = C.c_void_p, C.c_uint32, C.c_uint64, C.c_int
    L.gn_last_error.restype = C.c_char_p
    L.gn_device_count.argtypes = [C.POINTER(i32)]
    L.gn_filter_upload_ibf.argtypes = [i32, C.POINTER(IbfDesc), vp, u32, C.POINTER(vp)]
    L.gn_filter_upload_hibf.argtypes = [i32, u32, C.POINTER(IbfDesc), C.POINTER(vp), C.POINTER(vp), u64, C.POINTER(vp)]
    L.gn_filter_emplace.argtypes = [vp, vp, vp, u64]
    L.gn_filter_emplace_ibf.argtypes = [vp, u32, vp, vp, u64]
    L.gn_filter_download_rows.argtypes = [vp, u32, u64, u64, vp]
    L.gn_filter_download_row_list.argtypes = [vp, u32, vp, u64, vp]
    L.gn_pinned_alloc.argtypes = [C.c_size_t, C.POINTER(vp)]
    L.gn_pinned_free.argtypes = [vp]
    L.gn_filter_write_rows.argtypes = [vp, u32, u64, u64, vp, u64, u64]
    L.gn_filter_write_sync.argtypes = [vp]
    L.gn_filter_finalize.argtypes = [vp]
    L.gn_filter_fill_random.argtypes = [vp, u32, u64, u32, u64, u64]
    L.gn_filter_info.argtypes = [vp, C.POINTER(i32), C.POINTER(u32), C.POINTER(u64), C.POINTER(u64)]
    L.gn_filter_free.argtypes = [vp]
    L.gn_stream_create.argtypes = [vp, u32, u64, u64, C.POINTER(vp)]
    L.gn_stream_destroy.argtypes = [vp]
    L.gn_stream_upload_reads.argtypes = [vp, vp, u64, vp, vp, u32]
    L.gn_stream_minimisers.argtypes = [vp, u32, u32]
    L.gn_stream_classify.argtypes = [vp, u32, u32, C.c_double]
    L.gn_submit_batch.argtypes = [vp, vp, u64, vp, vp, u32, u32, u32, C.c_double]
    L.gn_stream_sync.argtypes = [vp]
    L.gn_stream_classify_shared.argtypes = [vp, vp, C.c_double]
    L.gn_stream_upload_fastq.argtypes = [vp, vp, u64]
    L.gn_stream_upload_text.argtypes = [vp, vp, u64, i32]
    L.gn_stream_upload_text_pair.argtypes = [vp, vp, u64, vp, u64, i32]
    L.gn_stream_text_pair_index.argtypes = [vp, C.POINTER(u32), C.POINTER(u64), C.POINTER(u64)]
    L.gn_stream_text_pair_records2.argtypes = [vp, vp, vp, vp]
    L.gn_stream_fastq_index.argtypes = [vp, C.POINTER(u32), C.POINTER(u64), C.POINTER(u64)]
    L.gn_stream_fastq_keep.argtypes = [vp, u32]
    L.gn_stream_fastq_records.argtypes = [vp, vp, vp, vp]
    L.gn_fetch_batch.argtypes = [vp, vp, vp, vp, vp, u64, C.POINTER(u64)]
    L.gn_stream_device_matches.argtypes = [vp, C.POINTER(vp), C.POINTER(u64)]
    L.gn_stream_set_postfilter.argtypes = [vp, vp]
    L.gn_fetch_postfilter.argtypes = [vp, vp, C.POINTER(u64), C.POINTER(u64)]
    L.gn_stream_set_long_reads.argtypes = [vp, i32]
    L.gn_streams_postfilter_joint.argtypes = [vp, u32]
    L.gn_stream_fetch_hashes.argtypes = [vp, vp, vp, u64, C.POINTER(u64)]
    L.gn_stream_distinct_hashes.argtypes = [vp, vp, u64, C.POINTER(u64)]
    L.gn_filter_emplace_split.argtypes = [vp, vp, u64, u32, u64]
    L.gn_filter_emplace_runs_window.argtypes = [vp, vp, vp, vp, vp, u32, u64, u64, u64]
    L.gn_stream_distinct_hashes_packed.argtypes = [vp, vp, u64, vp, u64, C.POINTER(u64), C.POINTER(u64), C.POINTER(u64)]
    L.gn_filter_emplace_packed_window.argtypes = [vp, vp, vp, vp, vp, vp, u32, u64, u64, u64]
    L.gn_hashes_union.argtypes = [C.c_int, vp, vp, u32, vp, u64, C.POINTER(u64)]
    L.gn_filter_emplace_path.argtypes = [vp, vp, vp, u32, vp, u32]
    L.gn_filter_create_hibf_storage.argtypes = [i32, u32, C.POINTER(IbfDesc), C.POINTER(vp)]
    L.gn_filter_emplace_path_window.argtypes = [vp, vp, vp, u32, vp, u32, vp, vp, u64]
    L.gn_filter_emplace_path_packed_window.argtypes = [vp, vp, vp, vp, u32, vp, u32, vp, vp, u64]
    L.gn_packed_union.argtypes = [C.c_int, vp, vp, vp, u32, vp, u64, vp, u64, C.POINTER(u64), C.POINTER(u64), C.POINTER(u64)]
    L.gn_filter_probe_path.argtypes =[vp, vp, vp, u32, vp, u32, vp, vp, vp]
    L.gn_filter_probe_paths_shared.argtypes = [vp, vp, u64, vp, u32, u32, vp]
    L.gn_filter_probe_path_window.argtypes = [vp, vp, vp, u32, vp, u32, vp, vp, vp, vp, vp, u64]
    L.gn_filter_probe_paths_shared_window.argtypes = [vp, vp, u64, vp, u32, u32, vp, vp, vp, vp]
    L.gn_filter_bin_popcounts.argtypes = [vp, u32, vp]
    L.gn_filter_copy_ibf.argtypes = [vp, u32, vp, u32]
    L.gn_filter_copy_ibf_spans.argtypes = [vp, u32, vp, u32, vp, u32]
    L.gn_filter_fold_ibf.argtypes = [vp, u32, u32, u32, vp, u32, vp, u32]
    L.gn_filter_extend_path.argtypes = [vp, vp, vp, u32, vp, u32, vp, vp]
    L.gn_sketches_create.argtypes = [C.c_int, vp, vp, u32, C.POINTER(vp)]
    L.gn_sketches_create_packed.argtypes = [C.c_int, vp, vp, vp, u32, C.POINTER(vp)]
    L.gn_sketches_free.argtypes = [vp]
    L.gn_sketches_download.argtypes = [vp, u32, u32, vp]
    L.gn_sketches_union_table.argtypes = [vp, vp, u32, u32, u32, u32, vp]
    L.gn_sketches_pair_table.argtypes = [vp, vp, u32, vp]
    L.gn_stream_dense_counts.argtypes = [vp, u32, u32, vp]
    L.gn_stream_timings.argtypes = [vp, C.POINTER(Timings)]
    L.gn_stream_screen_deferred.argtypes = [vp, C.POINTER(C.c_uint64)]
    L.gn_filter_set_stream_rows_min_bytes.argtypes = [vp, u64]
    L.gn_stream_rows_streamed.argtypes = [vp, C.POINTER(C.c_int)]
    L.gn_gather_create.argtypes = [i32, u32, C.POINTER(vp), vp, C.POINTER(vp)]
    L.gn_gather_create_merged.argtypes = [i32, u32, C.POINTER(vp), vp, C.POINTER(vp)]
    L.gn_gather_run.argtypes = [vp, C.POINTER(vp), u32]
    L.gn_gather_fetch.argtypes = [vp, vp, vp, u64, C.POINTER(u64)]
    L.gn_gather_device_matches.argtypes = [vp, C.POINTER(vp), C.POINTER(vp), C.POINTER(u64), C.POINTER(u64)]
    L.gn_gather_destroy.argtypes = [vp]
    L.gn_gather_run_buffers.argtypes = [vp, C.POINTER(vp), C.POINTER(vp), vp, u32, u32]
    L.gn_stream_device_offsets.argtypes = [vp, C.POINTER(vp)]
    L.gn_ablate.argtypes = [C.c_char_p]
    L.gn_filter_probe.argtypes = [vp, vp, u64, vp, u32, C.POINTER(u64), C.POINTER(u64), C.POINTER(u64)]
    L.gn_stream_hibf_levels.argtypes = [vp, C.POINTER(u32), vp, vp, vp, vp, u32]
    L.gn_stream_hibf_level_lines.argtypes = [vp, vp, u32]
    L.gn_device_memory.argtypes = [i32, C.POINTER(u64), C.POINTER(u64)]
    L.gn_ibf_hash_constants.argtypes = [vp, C.POINTER(u64)]
    L.gn_inflate_set_turns.argtypes = [vp, u32, u32]
    L.gn_inflate_handoff.argtypes = [vp, vp]
    L.gn_stream_upload_text_pair_devices.argtypes = [vp, vp, u64, i32, vp, u64, i32, i32]
    L.gn_hibf_row_stride_words.argtypes = [u64]
    L.gn_hibf_row_stride_words.restype = u64
    L.gn_peer_stats.argtypes = [i32, i32, C.POINTER(i32), C.POINTER(u64)]
    L.gn_reassign_create.argtypes = [i32, u64, u64, u32, vp, vp, C.POINTER(vp)]
    L.gn_reassign_run.argtypes = [vp, u32, C.c_double, C.POINTER(u32)]
    L.gn_reassign_diffs.argtypes = [vp, vp, u32]
    L.gn_reassign_fetch.argtypes = [vp, vp, vp, vp, vp]
    L.gn_reassign_info.argtypes = [vp, C.POINTER(u64), C.POINTER(u64), C.POINTER(u64), C.POINTER(C.c_float), C.POINTER(u64)]
    L.gn_reassign_free.argtypes = [vp]
    L.gn_inflate_create.argtypes = [i32, u64, u32, u64, C.POINTER(vp)]
    L.gn_inflate_destroy.argtypes = [vp]
    L.gn_inflate_feed.argtypes = [vp, vp, u64]
    L.gn_inflate_step.argtypes = [vp, C.POINTER(u64), C.POINTER(i32)]
    L.gn_inflate_text.argtypes = [vp, vp, u64, u64]
    L.gn_inflate_text_device.argtypes = [vp, C.POINTER(vp), C.POINTER(u64)]
    L.gn_inflate_get_stats.argtypes = [vp, C.POINTER(InflateStats)]
    L.gn_inflate_cuts.argtypes = [vp, u32, u64, vp, u32, C.POINTER(u32)]
    L.gn_inflate_set_carry.argtypes = [vp, u64]
    L.gn_inflate_cuts_lines.argtypes = [vp, u32, u64, vp, vp, u32, C.POINTER(u32)]
    L.gn_inflate_cut_at_lines.argtypes = [vp, vp, u32, vp, C.POINTER(u64)]
    L.gn_stream_upload_text_pair_device.argtypes = [vp, vp, u64, vp, u64, i32, i32]
    L.gn_stream_fetch_letters.argtypes = [vp, vp, u64, vp, vp, C.POINTER(u64)]
    L.gn_stream_upload_text_device.argtypes = [vp, vp, u64, i32, i32]
    L.gn_stream_fastq_headers.argtypes = [vp, vp, u64, vp, C.POINTER(u64)]
    L.gn_stream_upload_genome_text.argtypes = [vp, vp, u64, u32, u32, u64, u32]
    L.gn_stream_genome_index.argtypes = [vp, C.POINTER(u32), C.POINTER(u32), C.POINTER(u64), C.POINTER(u64), C.POINTER(i32), C.POINTER(u64), C.POINTER(u64)]
    L.gn_stream_genome_records.argtypes = [vp, vp, vp, vp]
    for name in ABI_SYMBOLS:
        if name not in ("gn_last_error", "gn_hibf_row_stride_words"):   # (const char* and uint64_t returns, set above)
            getattr(L, name).restype = i32
    _lib = L
    return L


def _check(rc: int) -> None:
    if rc != 0:
        raise GanonHipError(rc, load_library().gn_last_error().decode(errors="replace"))


def _p(a: Optional[np.ndarray]):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def device_count() -> int:
    n = C.c_int(0)
    _check(load_library().gn_device_count(C.byref(n)))
    return n.value


def _desc(rows: Optional[np.ndarray], bins: int, bin_size: int, hash_funs: int) -> IbfDesc:
    W = (bins + 63) >> 6
    shift = 64 - int(bin_size).bit_length()
    if rows is not None:
        assert rows.dtype == np.uint64 and rows.size == bin_size * W and rows.flags["C_CONTIGUOUS"]
    return IbfDesc(rows.ctypes.data if rows is not None else None, bin_size, W, bins, hash_funs, shift)


def _mix64(z: np.ndarray) -> np.ndarray:
    with np.errstate(over="ignore"):
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        return z ^ (z >> np.uint64(31))


def fill_random_words(seed: int, rows: np.ndarray, n_words: int, and_words: int = 1, word_lo: int = 0,
                      row_words_total: int = 0, bins: int = 0) -> np.ndarray:
    """numpy statement of gn_filter_fill_random (include/ganon_hip.h): words [word_lo, word_lo+n_words) of the given
    rows -> uint64 [len(rows), n_words].  `bins` (of this column slice) clears the padding bins of its last word."""
    rows = np.asarray(rows, dtype=np.uint64).reshape(-1, 1)
    total = np.uint64(row_words_total or n_words)
    with np.errstate(over="ignore"):
        g = (rows * total + np.uint64(word_lo) + np.arange(n_words, dtype=np.uint64)[None, :]) * np.uint64(0x9E3779B97F4A7C15)
        v = np.full(g.shape, np.uint64(0xFFFFFFFFFFFFFFFF))
        key = [_mix64(np.array([(seed + a) & 0xFFFFFFFFFFFFFFFF], dtype=np.uint64))[0] for a in range(3 if and_words == FILL_3_OF_8 else 4 if and_words == FILL_3_OF_16 else and_words)]
        if and_words == FILL_3_OF_8:
            v = _mix64(key[0] + g) & (_mix64(key[1] + g) | _mix64(key[2] + g))
        elif and_words == FILL_3_OF_16:
            v = _mix64(key[0] + g) & _mix64(key[1] + g) & (_mix64(key[2] + g) | _mix64(key[3] + g))
        else:
            for a in range(and_words):
                v &= _mix64(key[a] + g)
    if bins & 63:
        v[:, -1] &= np.uint64((1 << (bins & 63)) - 1)
    return v


def ibf_hash_constants() -> Tuple[list, int]:
    """(five seeds, multiplier) of hash_and_fit as libganon_hip.so was built (gn_ibf_hash_constants; no device needed)"""
    seeds = np.zeros(5, dtype=np.uint64)
    mul = C.c_uint64(0)
    _check(load_library().gn_ibf_hash_constants(_p(seeds), C.byref(mul)))
    return [int(x) for x in seeds], int(mul.value)


def device_memory(device: int = 0) -> Tuple[int, int]:
    """(free, total) bytes of a device (gn_device_memory)"""
    f, t = C.c_uint64(0), C.c_uint64(0)
    _check(load_library().gn_device_memory(device, C.byref(f), C.byref(t)))
    return int(f.value), int(t.value)


class HipInflate:
    """gn_inflate_*: a gzip file inflated on the device (include/ganon_hip.h).  `inflate(data)` = the whole file at once."""

    def __init__(self, compressed_bytes: int, device: int = 0, chunk_bytes: int = 0, step_bytes: int = 0):
        self._L = load_library()
        self._h = C.c_void_p()
        _check(self._L.gn_inflate_create(device, compressed_bytes, chunk_bytes, step_bytes, C.byref(self._h)))

    def close(self) -> None:
        if self._h:
            self._L.gn_inflate_destroy(self._h)
            self._h = C.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def feed(self, data: np.ndarray) -> None:
        data = np.ascontiguousarray(data, dtype=np.uint8)
        _check(self._L.gn_inflate_feed(self._h, _p(data), data.size))

    def step(self) -> Tuple[int, bool]:
        n, done = C.c_uint64(0), C.c_int(0)
        _check(self._L.gn_inflate_step(self._h, C.byref(n), C.byref(done)))
        return int(n.value), bool(done.value)

    def text(self, n: int, off: int = 0) -> np.ndarray:
        out = np.empty(n, dtype=np.uint8)
        _check(self._L.gn_inflate_text(self._h, _p(out), off, n))
        return out

    def text_device(self) -> Tuple[int, int]:
        """(device pointer, bytes) of the last step's text"""
        ptr, n = C.c_void_p(), C.c_uint64()
        _check(self._L.gn_inflate_text_device(self._h, C.byref(ptr), C.byref(n)))
        return int(ptr.value or 0), int(n.value)

    def cuts(self, lines_per_record: int, piece_bytes: int) -> np.ndarray:
        """gn_inflate_cuts: record boundaries of the last step's text, one at or behind every multiple of piece_bytes + the last one"""
        _, n = self.text_device()
        out = np.empty(n // max(1, piece_bytes) + 2, dtype=np.uint64)
        k = C.c_uint32()
        _check(self._L.gn_inflate_cuts(self._h, lines_per_record, piece_bytes, _p(out), out.size, C.byref(k)))
        return out[:k.value].copy()

    def set_carry(self, n_tail: int) -> None:
        _check(self._L.gn_inflate_set_carry(self._h, n_tail))

    def set_turns(self, n_turns: int, my_turn: int) -> None:
        """gn_inflate_set_turns: this inflater runs steps my_turn, my_turn + n_turns, ... of a file that n_turns inflaters share"""
        _check(self._L.gn_inflate_set_turns(self._h, n_turns, my_turn))

    def handoff(self, to: "HipInflate") -> None:
        """gn_inflate_handoff: what the next step needs of the one this inflater just ran goes to `to` (device to device)"""
        _check(self._L.gn_inflate_handoff(self._h, to._h))

    def stats(self) -> dict:
        st = InflateStats()
        _check(self._L.gn_inflate_get_stats(self._h, C.byref(st)))
        return {k: (list(getattr(st, k)) if k == "prof_ms" else getattr(st, k)) for k, _ in InflateStats._fields_}

    def inflate_all(self, data: np.ndarray, feed_bytes: int = 0, fetch: bool = True):
        """feeds `data` (the whole file) in pieces of feed_bytes (0: at once), steps until the stream ends; returns the text
        (fetch=False: only its length -- timing runs)"""
        data = np.ascontiguousarray(data, dtype=np.uint8)
        parts, total, fed = [], 0, 0
        fb = feed_bytes or data.size
        done = False
        while not done:
            if fed < data.size:
                self.feed(data[fed:fed + fb])
                fed = min(data.size, fed + fb)
                if fed < data.size and fed < 2 * fb + (4 << 20):
                    continue
            n, done = self.step()
            if fetch and n:
                parts.append(self.text(n))
            total += n
        if not fetch:
            return total
        return np.concatenate(parts) if parts else np.empty(0, dtype=np.uint8)


class HipReassign:
    """gn_reassign_*: the EM of `ganon reassign` over a CSR table of (read -> entries naming targets), on the device"""

    def __init__(self, off: np.ndarray, target: np.ndarray, n_targets: int, device: int = 0):
        self._off = np.ascontiguousarray(off, dtype=np.uint64)
        self._target = np.ascontiguousarray(target, dtype=np.uint32)
        self.n_reads, self.n_targets = self._off.size - 1, int(n_targets)
        self._h = C.c_void_p()
        _check(load_library().gn_reassign_create(device, self.n_reads, self._target.size, self.n_targets, _p(self._off), _p(self._target),
                                                 C.byref(self._h)))

    def run(self, max_iter: int = 10, threshold: float = 0.0):
        """-> (diffs float64[iterations], counts uint64[n_targets], unique uint64[n_targets], prob float64[n_targets],
        choice uint64[n_reads] = entry index per read)"""
        L = load_library()
        it = C.c_uint32(0)
        _check(L.gn_reassign_run(self._h, max_iter, float(threshold), C.byref(it)))
        diffs = np.zeros(it.value, dtype=np.float64)
        _check(L.gn_reassign_diffs(self._h, _p(diffs), it.value))
        counts = np.zeros(self.n_targets, dtype=np.uint64)
        unique = np.zeros(self.n_targets, dtype=np.uint64)
        prob = np.zeros(self.n_targets, dtype=np.float64)
        choice = np.zeros(self.n_reads, dtype=np.uint64)
        _check(L.gn_reassign_fetch(self._h, _p(counts), _p(unique), _p(prob), _p(choice)))
        return diffs, counts, unique, prob, choice

    def info(self) -> dict:
        nu, nm, nw, by = C.c_uint64(0), C.c_uint64(0), C.c_uint64(0), C.c_uint64(0)
        ms = C.c_float(0)
        _check(load_library().gn_reassign_info(self._h, C.byref(nu), C.byref(nm), C.byref(nw), C.byref(ms), C.byref(by)))
        return dict(unique_reads=nu.value, multi_reads=nm.value, wave_reads=nw.value, ms=ms.value, bytes_per_iteration=by.value)

    def free(self):
        if self._h:
            load_library().gn_reassign_free(self._h)
            self._h = C.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.free()
        return False

    def __del__(self):
        try:
            self.free()
        except Exception:  # noqa: BLE001 -- interpreter shutdown
            pass


class HipGather:
    """gn_gather: the column parts of a bin-range partitioned flat IBF put back together on the batch's owner device;
    merged=True: the subtree parts of an HIBF, a read's segments merged by translated id (gn_gather_create_merged)."""

    def __init__(self, device: int, target_maps: Sequence[Optional[np.ndarray]], merged: bool = False):
        self._maps = [None if m is None else np.ascontiguousarray(m, dtype=np.uint32) for m in target_maps]
        n = len(self._maps)
        ptrs = (C.c_void_p * n)(*[None if m is None else m.ctypes.data for m in self._maps])
        sizes = np.array([0 if m is None else len(m) for m in self._maps], dtype=np.uint32)
        self._h = C.c_void_p()
        self.n_reads = 0
        L = load_library()
        _check((L.gn_gather_create_merged if merged else L.gn_gather_create)(device, n, ptrs, _p(sizes), C.byref(self._h)))

    def run(self, streams: Sequence["HipStream"]) -> None:
        arr = (C.c_void_p * len(streams))(*[st._h for st in streams])
        self.n_reads = streams[0].n_reads
        _check(load_library().gn_gather_run(self._h, arr, len(streams)))

    def run_buffers(self, off_ptrs: Sequence[int], match_ptrs: Sequence[int], n_matches: Sequence[int], n_reads: int) -> None:
        """gn_gather_run_buffers: parts given as raw device pointers (offsets, records) on the gather's device"""
        k = len(off_ptrs)
        a = (C.c_void_p * k)(*[int(x) for x in off_ptrs])
        b = (C.c_void_p * k)(*[int(x) if x else None for x in match_ptrs])
        nm = np.asarray(n_matches, dtype=np.uint64)
        self.n_reads = int(n_reads)
        _check(load_library().gn_gather_run_buffers(self._h, a, b, _p(nm), k, int(n_reads)))

    def fetch(self):
        """-> (match_off u64[n+1], matches MATCH_DTYPE[m]) grouped by read, ascending target"""
        L = load_library()
        mo = np.zeros(self.n_reads + 1, dtype=np.uint64)
        need = C.c_uint64(0)
        _check(L.gn_gather_fetch(self._h, _p(mo), None, 0, C.byref(need)))
        m = np.zeros(max(int(need.value), 1), dtype=MATCH_DTYPE)
        _check(L.gn_gather_fetch(self._h, None, _p(m), len(m), C.byref(need)))
        return mo, m[: int(need.value)]

    def peer_bytes(self) -> int:
        """bytes the last run() copied between devices"""
        b = C.c_uint64(0)
        _check(load_library().gn_gather_device_matches(self._h, None, None, None, C.byref(b)))
        return int(b.value)

    def destroy(self) -> None:
        if self._h:
            load_library().gn_gather_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.destroy()
        except Exception:
            pass


PATH_DTYPE = np.dtype([("ibf", "<u4"), ("first_bin", "<u4"), ("n_bins", "<u4"), ("reserved", "<u4"), ("hashes_per_bin", "<u8")])  # gn_path_entry


def hashes_union(sets: Sequence[np.ndarray], device: int = 0, size_only: bool = False):
    """gn_hashes_union: the ascending union of ascending uint64 sets (or, size_only, its size alone)"""
    sets = [np.ascontiguousarray(a, dtype=np.uint64) for a in sets]
    n = len(sets)
    ptrs = (C.c_void_p * max(n, 1))(*[a.ctypes.data for a in sets])
    sizes = np.array([len(a) for a in sets], dtype=np.uint64)
    nu = C.c_uint64(0)
    L = load_library()
    if size_only:
        _check(L.gn_hashes_union(device, ptrs, _p(sizes), n, None, 0, C.byref(nu)))
        return nu.value
    out = np.empty(int(sizes.sum()), dtype=np.uint64)
    _check(L.gn_hashes_union(device, ptrs, _p(sizes), n, _p(out), len(out), C.byref(nu)))
    return out[: nu.value].copy()


def _packed_runs(runs):
    """runs[r] = (blocks, payload) as the calls for packed runs take them -> (kept arrays, block pointers, n_blocks, payload pointers);
    a payload of None goes in as a null pointer"""
    blocks = [np.ascontiguousarray(b, dtype=PACKED_BLOCK_DTYPE) for b, _ in runs]
    words = [None if w is None else np.ascontiguousarray(w, dtype=np.uint64) for _, w in runs]
    bptr = (C.c_void_p * max(len(runs), 1))(*[a.ctypes.data for a in blocks])
    wptr = (C.c_void_p * max(len(runs), 1))(*[None if a is None else a.ctypes.data for a in words])
    n_blocks = np.array([len(a) for a in blocks], dtype=np.uint64)
    return (blocks, words), bptr, n_blocks, wptr


def packed_union(runs, device: int = 0, size_only: bool = False, cap_blocks: Optional[int] = None, cap_words: Optional[int] = None):
    """gn_packed_union: the ascending union of the hashes of packed runs (runs[r] = (blocks, payload), PACKED_BLOCK_DTYPE records whose
    word_at count from payload[0]) packed as one set -> (hashes, blocks, payload words); size_only -> (hashes, blocks, words) as counts.
    cap_blocks / cap_words: the buffers' sizes when the bounds of the format are not wanted; a GanonHipError of GN_EOVERFLOW carries the
    three sizes as .sizes"""
    keep, bptr, n_blocks, wptr = _packed_runs(runs)
    n, nb, nw = C.c_uint64(0), C.c_uint64(0), C.c_uint64(0)
    L = load_library()
    if size_only:
        _check(L.gn_packed_union(device, bptr, _p(n_blocks), wptr, len(runs), None, 0, None, 0, C.byref(n), C.byref(nb), C.byref(nw)))
        return int(n.value), int(nb.value), int(nw.value)
    total = int(sum(int(b["cnt"].sum()) for b in keep[0]))
    most = (total + 511) // 512  # gn_packed_max_blocks, gn_packed_max_words
    cap_blocks = most if cap_blocks is None else cap_blocks
    cap_words = total - most if cap_words is None else cap_words
    blocks = np.zeros(max(cap_blocks, 1), dtype=PACKED_BLOCK_DTYPE)
    words = np.zeros(max(cap_words, 1), dtype=np.uint64)
    try:
        _check(L.gn_packed_union(device, bptr, _p(n_blocks), wptr, len(runs), blocks.ctypes.data_as(C.c_void_p), cap_blocks, _p(words), cap_words, C.byref(n),
                                 C.byref(nb), C.byref(nw)))
    except GanonHipError as e:
        e.sizes = (int(n.value), int(nb.value), int(nw.value))
        e.written = bool(blocks.view(np.uint8).any() or words.any())
        raise
    return int(n.value), blocks[: int(nb.value)], words[: int(nw.value)]


SKETCH_M = 4096                # GN_SKETCH_M
SKETCH_TABLE_MAX = 1 << 24     # GN_SKETCH_TABLE_MAX


class HipSketches:
    """gn_sketches: one HyperLogLog sketch (SKETCH_M one-byte registers) per hash set, resident on the device"""

    def __init__(self, sets: Sequence[np.ndarray], device: int = 0):
        sets = [np.ascontiguousarray(a, dtype=np.uint64) for a in sets]
        self.n = len(sets)
        ptrs = (C.c_void_p * max(self.n, 1))(*[a.ctypes.data for a in sets])
        sizes = np.array([len(a) for a in sets], dtype=np.uint64)
        self._h = C.c_void_p()
        _check(load_library().gn_sketches_create(device, ptrs, _p(sizes), self.n, C.byref(self._h)))

    @classmethod
    def from_packed(cls, runs, device: int = 0) -> "HipSketches":
        """gn_sketches_create_packed: one sketch per packed run (runs[r] = (blocks, payload), as packed_union takes them)"""
        keep, bptr, n_blocks, wptr = _packed_runs(runs)
        self = cls.__new__(cls)
        self.n = len(runs)
        self._h = C.c_void_p()
        _check(load_library().gn_sketches_create_packed(device, bptr, _p(n_blocks), wptr, self.n, C.byref(self._h)))
        return self

    def download(self, first: int = 0, n: Optional[int] = None) -> np.ndarray:
        """registers of sketches first .. first + n - 1, uint8 [n, SKETCH_M]"""
        n = self.n - first if n is None else n
        out = np.empty((n, SKETCH_M), dtype=np.uint8)
        _check(load_library().gn_sketches_download(self._h, first, n, _p(out)))
        return out

    def union_table(self, order, width: int, j0: int = 0, j1: Optional[int] = None) -> np.ndarray:
        """gn_sketches_union_table -> uint64 [j1 - j0, width]"""
        order = np.ascontiguousarray(order, dtype=np.uint32)
        j1 = len(order) if j1 is None else j1
        out = np.empty((max(j1 - j0, 0), width), dtype=np.uint64)
        _check(load_library().gn_sketches_union_table(self._h, _p(order), len(order), j0, j1, width, _p(out)))
        return out

    def pair_table(self, idx) -> np.ndarray:
        """gn_sketches_pair_table -> uint64 [m, m]: the estimated union of sketches idx[a] and idx[b]"""
        idx = np.ascontiguousarray(idx, dtype=np.uint32)
        out = np.empty((len(idx), len(idx)), dtype=np.uint64)
        _check(load_library().gn_sketches_pair_table(self._h, _p(idx), len(idx), _p(out)))
        return out

    def free(self) -> None:
        if self._h:
            load_library().gn_sketches_free(self._h)
            self._h = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


class HipFilter:
    """Device-resident, immutable IBF / HIBF (gn_filter)."""

    def __init__(self, handle, keep=None, bins=None):
        self._h = handle
        self._keep = keep
        self._bins = list(bins) if bins is not None else None  # technical bins per IBF (one entry for a flat filter), when known

    @classmethod
    def ibf(cls, rows: Optional[np.ndarray], bins: int, bin_size: int, hash_funs: int,
            bin2target: Optional[np.ndarray] = None, n_targets: Optional[int] = None, device: int = 0) -> "HipFilter":
        if bin2target is None:
            bin2target = np.arange(bins, dtype=np.uint32)
            n_targets = bins
        bin2target = np.ascontiguousarray(bin2target, dtype=np.uint32)
        if n_targets is None:
            n_targets = int(bin2target[bin2target != 0xFFFFFFFF].max()) + 1
        d = _desc(rows, bins, bin_size, hash_funs)
        h = C.c_void_p()
        _check(load_library().gn_filter_upload_ibf(device, C.byref(d), _p(bin2target), n_targets, C.byref(h)))
        return cls(h, bins=[bins])

    @classmethod
    def hibf(cls, ibfs: Sequence[Tuple[np.ndarray, int, int, int]], next_ibf_id: Sequence[np.ndarray],
             bin2user: Sequence[np.ndarray], n_user_bins: int, device: int = 0) -> "HipFilter":
        """ibfs: sequence of (rows, bins, bin_size, hash_funs)."""
        n = len(ibfs)
        descs = (IbfDesc * n)(*[_desc(r, b, s, hf) for r, b, s, hf in ibfs])
        nx = [np.ascontiguousarray(a, dtype=np.int64) for a in next_ibf_id]
        bu = [np.ascontiguousarray(a, dtype=np.int64) for a in bin2user]
        nxp = (C.c_void_p * n)(*[a.ctypes.data for a in nx])
        bup = (C.c_void_p * n)(*[a.ctypes.data for a in bu])
        h = C.c_void_p()
        _check(load_library().gn_filter_upload_hibf(device, n, descs, nxp, bup, n_user_bins, C.byref(h)))
        return cls(h, keep=(nx, bu), bins=[b for _, b, _, _ in ibfs])

    def emplace(self, hashes: np.ndarray, bins: np.ndarray, ibf_idx: int = 0) -> None:
        hashes = np.ascontiguousarray(hashes, dtype=np.uint64)
        bins = np.ascontiguousarray(bins, dtype=np.uint32)
        assert len(hashes) == len(bins)
        _check(load_library().gn_filter_emplace_ibf(self._h, ibf_idx, _p(hashes), _p(bins), len(hashes)))

    @classmethod
    def ibf_storage(cls, bins: int, bin_size: int, hash_funs: int, device: int = 0) -> "HipFilter":
        """an empty storage-only flat filter (no bin map, as `ganon-build` creates it): bits can be inserted and read back"""
        d = _desc(None, bins, bin_size, hash_funs)
        h = C.c_void_p()
        _check(load_library().gn_filter_upload_ibf(device, C.byref(d), None, 0, C.byref(h)))
        return cls(h, bins=[bins])

    def emplace_split(self, hashes: np.ndarray, first_bin: int, hashes_per_bin: int) -> None:
        """gn_filter_emplace_split: hash i into bin first_bin + i // hashes_per_bin"""
        hashes = np.ascontiguousarray(hashes, dtype=np.uint64)
        _check(load_library().gn_filter_emplace_split(self._h, _p(hashes), len(hashes), first_bin, hashes_per_bin))

    def emplace_runs_window(self, runs: Sequence[np.ndarray], first_bins, hashes_per_bin, total_rows: int, row_begin: int,
                            chunk_hashes: int = 0) -> None:
        """gn_filter_emplace_runs_window: this filter stands for rows [row_begin, row_begin + its rows) of a filter of total_rows rows;
        hash i of runs[r] belongs to bin first_bins[r] + i // hashes_per_bin[r] and sets the bits of its rows inside that window"""
        runs = [np.ascontiguousarray(a, dtype=np.uint64) for a in runs]
        ptrs = (C.c_void_p * max(len(runs), 1))(*[a.ctypes.data for a in runs])
        sizes = np.array([len(a) for a in runs], dtype=np.uint64)
        first = np.ascontiguousarray(first_bins, dtype=np.uint32)
        per = np.ascontiguousarray(hashes_per_bin, dtype=np.uint64)
        assert len(first) == len(per) == len(runs)
        _check(load_library().gn_filter_emplace_runs_window(self._h, ptrs, _p(sizes), _p(first), _p(per), len(runs), total_rows, row_begin, chunk_hashes))

    def emplace_packed_window(self, runs, first_bins, hashes_per_bin, total_rows: int, row_begin: int, chunk_words: int = 0) -> None:
        """gn_filter_emplace_packed_window: emplace_runs_window for packed runs.  runs[r] = (blocks, payload): PACKED_BLOCK_DTYPE records
        whose word_at count from payload[0], and the uint64 payload words"""
        blocks = [np.ascontiguousarray(b, dtype=PACKED_BLOCK_DTYPE) for b, _ in runs]
        words = [np.ascontiguousarray(w, dtype=np.uint64) for _, w in runs]
        bptr = (C.c_void_p * max(len(runs), 1))(*[a.ctypes.data for a in blocks])
        wptr = (C.c_void_p * max(len(runs), 1))(*[a.ctypes.data for a in words])
        n_blocks = np.array([len(a) for a in blocks], dtype=np.uint64)
        first = np.ascontiguousarray(first_bins, dtype=np.uint32)
        per = np.ascontiguousarray(hashes_per_bin, dtype=np.uint64)
        assert len(first) == len(per) == len(runs)
        _check(load_library().gn_filter_emplace_packed_window(self._h, bptr, _p(n_blocks), wptr, _p(first), _p(per), len(runs), total_rows, row_begin, chunk_words))

    def emplace_path(self, sets: Sequence[np.ndarray], paths: np.ndarray) -> None:
        """gn_filter_emplace_path: sets[s] (ascending uint64) along paths[s] (PATH_DTYPE, shape [len(sets), depth]) of an HIBF"""
        paths = np.ascontiguousarray(paths, dtype=PATH_DTYPE)
        assert paths.ndim == 2 and paths.shape[0] == len(sets)
        off = np.zeros(len(sets) + 1, dtype=np.uint64)
        off[1:] = np.cumsum([len(a) for a in sets])
        hashes = np.concatenate([np.asarray(a, dtype=np.uint64) for a in sets]) if len(sets) else np.zeros(0, np.uint64)
        hashes = np.ascontiguousarray(hashes, dtype=np.uint64)
        _check(load_library().gn_filter_emplace_path(self._h, _p(hashes), _p(off), len(sets), paths.ctypes.data_as(C.c_void_p), paths.shape[1]))

    @classmethod
    def hibf_storage(cls, shapes: Sequence[Tuple[int, int, int]], device: int = 0) -> "HipFilter":
        """gn_filter_create_hibf_storage: an empty storage-only HIBF without tables, as `ganon-build --hibf` creates one per part of a
        tree built in parts.  shapes: (bins, rows, hash_funs) per IBF; the 4-tuples of `hibf` with rows None are taken too"""
        assert all(len(s) == 3 or (len(s) == 4 and s[0] is None) for s in shapes), "a storage filter starts zero-filled"
        shapes = [tuple(s[-3:]) for s in shapes]
        n = len(shapes)
        descs = (IbfDesc * max(n, 1))(*[_desc(None, b, r, hf) for b, r, hf in shapes])
        h = C.c_void_p()
        _check(load_library().gn_filter_create_hibf_storage(device, n, descs, C.byref(h)))
        return cls(h, bins=[b for b, _, _ in shapes])

    def emplace_path_window(self, sets: Sequence[np.ndarray], paths: np.ndarray, total_rows, row_begin, chunk_hashes: int = 0) -> None:
        """gn_filter_emplace_path_window: IBF j of this filter stands for rows [row_begin[j], row_begin[j] + its rows) of an IBF of
        total_rows[j] rows; sets[s] (ascending uint64) goes along paths[s] (PATH_DTYPE, [len(sets), depth], `ibf` numbering this filter's
        IBFs) and sets the bits of its rows inside those pieces"""
        paths = np.ascontiguousarray(paths, dtype=PATH_DTYPE)
        assert paths.ndim == 2 and paths.shape[0] == len(sets)
        sets = [np.ascontiguousarray(a, dtype=np.uint64) for a in sets]
        ptrs = (C.c_void_p * max(len(sets), 1))(*[a.ctypes.data for a in sets])
        sizes = np.array([len(a) for a in sets], dtype=np.uint64)
        total = np.ascontiguousarray(total_rows, dtype=np.uint64)
        begin = np.ascontiguousarray(row_begin, dtype=np.uint64)
        assert len(total) == len(begin) == len(self._bins)
        _check(load_library().gn_filter_emplace_path_window(self._h, ptrs, _p(sizes), len(sets), paths.ctypes.data_as(C.c_void_p), paths.shape[1],
                                                            _p(total), _p(begin), chunk_hashes))

    def emplace_path_packed_window(self, runs, paths: np.ndarray, total_rows, row_begin, chunk_words: int = 0) -> None:
        """gn_filter_emplace_path_packed_window: emplace_path_window for packed sets.  runs[s] = (blocks, payload): PACKED_BLOCK_DTYPE records
        whose word_at count from payload[0], and the uint64 payload words (None: a null pointer)"""
        paths = np.ascontiguousarray(paths, dtype=PATH_DTYPE)
        assert paths.ndim == 2 and paths.shape[0] == len(runs)
        keep, bptr, n_blocks, wptr = _packed_runs(runs)
        total = np.ascontiguousarray(total_rows, dtype=np.uint64)
        begin = np.ascontiguousarray(row_begin, dtype=np.uint64)
        assert len(total) == len(begin) == len(self._bins)
        _check(load_library().gn_filter_emplace_path_packed_window(self._h, bptr, _p(n_blocks), wptr, len(runs), paths.ctypes.data_as(C.c_void_p), paths.shape[1],
                                                                   _p(total), _p(begin), chunk_words))

    def extend_path(self, sets: Sequence[np.ndarray], paths: np.ndarray, quotas: Sequence[np.ndarray]) -> None:
        """gn_filter_extend_path: sets[s] (strictly ascending uint64) along paths[s] (PATH_DTYPE, [len(sets), depth]) of an HIBF that holds
        part of them already; quotas[s][j] = how many of the set's absent hashes bin first_bin + j of its leaf run takes"""
        paths = np.ascontiguousarray(paths, dtype=PATH_DTYPE)
        assert paths.ndim == 2 and paths.shape[0] == len(sets) == len(quotas)
        off = np.zeros(len(sets) + 1, dtype=np.uint64)
        off[1:] = np.cumsum([len(a) for a in sets])
        hashes = np.concatenate([np.asarray(a, dtype=np.uint64) for a in sets]) if len(sets) else np.zeros(0, np.uint64)
        hashes = np.ascontiguousarray(hashes, dtype=np.uint64)
        deal_off = np.zeros(len(sets) + 1, dtype=np.uint64)
        deal_off[1:] = np.cumsum([len(q) for q in quotas])
        deal = np.concatenate([np.asarray(q, dtype=np.uint64) for q in quotas]) if len(sets) else np.zeros(0, np.uint64)
        deal = np.ascontiguousarray(deal, dtype=np.uint64)
        _check(load_library().gn_filter_extend_path(self._h, _p(hashes), _p(off), len(sets), paths.ctypes.data_as(C.c_void_p), paths.shape[1],
                                                    _p(deal_off), _p(deal)))

    def probe_path(self, sets: Sequence[np.ndarray], paths: np.ndarray, with_lost_at: bool = True):
        """gn_filter_probe_path: sets[s] along paths[s] (PATH_DTYPE, [len(sets), depth]) -> (found uint64 [n], lost_at uint64 [n, depth] or
        None, first_lost uint64 [n], all ones = none)"""
        paths = np.ascontiguousarray(paths, dtype=PATH_DTYPE)
        assert paths.ndim == 2 and paths.shape[0] == len(sets)
        off = np.zeros(len(sets) + 1, dtype=np.uint64)
        off[1:] = np.cumsum([len(a) for a in sets])
        hashes = np.concatenate([np.asarray(a, dtype=np.uint64) for a in sets]) if len(sets) else np.zeros(0, np.uint64)
        hashes = np.ascontiguousarray(hashes, dtype=np.uint64)
        found = np.zeros(len(sets), dtype=np.uint64)
        first = np.full(len(sets), 0xFFFFFFFFFFFFFFFF, dtype=np.uint64)
        lost = np.zeros((len(sets), paths.shape[1]), dtype=np.uint64) if with_lost_at else None
        _check(load_library().gn_filter_probe_path(self._h, _p(hashes), _p(off), len(sets), paths.ctypes.data_as(C.c_void_p), paths.shape[1],
                                                   _p(found), _p(lost) if with_lost_at else None, _p(first)))
        return found, lost, first

    def probe_paths_shared(self, probes: np.ndarray, paths: np.ndarray) -> np.ndarray:
        """gn_filter_probe_paths_shared: the same probes against every path (PATH_DTYPE, [n_paths, depth]) -> found uint64 [n_paths]"""
        paths = np.ascontiguousarray(paths, dtype=PATH_DTYPE)
        assert paths.ndim == 2
        probes = np.ascontiguousarray(probes, dtype=np.uint64)
        found = np.zeros(paths.shape[0], dtype=np.uint64)
        _check(load_library().gn_filter_probe_paths_shared(self._h, _p(probes), len(probes), paths.ctypes.data_as(C.c_void_p), paths.shape[0],
                                                           paths.shape[1], _p(found)))
        return found

    def _plane_pointers(self, planes, n: int, depth: int):
        """planes: None, or {(path, entry): C-contiguous uint64 [n_bins, words]} -> the array of n * depth pointers the library takes"""
        if not planes:
            return None
        ptrs = (C.c_void_p * (n * depth))()
        for (s, d), a in planes.items():
            assert a.dtype == np.uint64 and a.flags.c_contiguous and a.flags.writeable and 0 <= s < n and 0 <= d < depth
            ptrs[s * depth + d] = a.ctypes.data
        return ptrs

    def probe_path_window(self, sets: Sequence[np.ndarray], paths: np.ndarray, total_rows, row_begin, alive: Sequence[np.ndarray],
                          lost_at: np.ndarray, planes=None, chunk_hashes: int = 0) -> None:
        """gn_filter_probe_path_window on a storage filter of pieces (see emplace_path_window for total_rows / row_begin).  In/out, only ever
        ANDed into (lost_at: added to): alive[s] uint64 [ceil(len(sets[s]) / 64)], lost_at uint64 [len(sets), depth], planes
        {(s, d): uint64 [n_bins, ceil(len(sets[s]) / 64)]} for the entries whose piece is a slab of its IBF"""
        paths = np.ascontiguousarray(paths, dtype=PATH_DTYPE)
        assert paths.ndim == 2 and paths.shape[0] == len(sets) == len(alive)
        sets = [np.ascontiguousarray(a, dtype=np.uint64) for a in sets]
        assert all(a.dtype == np.uint64 and a.flags.c_contiguous and len(a) == (len(x) + 63) // 64 for a, x in zip(alive, sets))
        assert lost_at.dtype == np.uint64 and lost_at.flags.c_contiguous and lost_at.shape == paths.shape
        ptrs = (C.c_void_p * max(len(sets), 1))(*[a.ctypes.data for a in sets])
        aptrs = (C.c_void_p * max(len(sets), 1))(*[a.ctypes.data for a in alive])
        sizes = np.array([len(a) for a in sets], dtype=np.uint64)
        total = np.ascontiguousarray(total_rows, dtype=np.uint64)
        begin = np.ascontiguousarray(row_begin, dtype=np.uint64)
        assert len(total) == len(begin) == len(self._bins)
        _check(load_library().gn_filter_probe_path_window(self._h, ptrs, _p(sizes), len(sets), paths.ctypes.data_as(C.c_void_p), paths.shape[1], _p(total),
                                                          _p(begin), aptrs, self._plane_pointers(planes, len(sets), paths.shape[1]), _p(lost_at),
                                                          chunk_hashes))

    def probe_paths_shared_window(self, probes: np.ndarray, paths: np.ndarray, total_rows, row_begin, alive: np.ndarray, planes=None) -> None:
        """gn_filter_probe_paths_shared_window: alive uint64 [n_paths, ceil(len(probes) / 64)] in/out; planes {(p, d): uint64 [n_bins,
        ceil(len(probes) / 64)]} for the entries whose piece is a slab of its IBF"""
        paths = np.ascontiguousarray(paths, dtype=PATH_DTYPE)
        assert paths.ndim == 2
        probes = np.ascontiguousarray(probes, dtype=np.uint64)
        assert alive.dtype == np.uint64 and alive.flags.c_contiguous and alive.shape == (paths.shape[0], (len(probes) + 63) // 64)
        total = np.ascontiguousarray(total_rows, dtype=np.uint64)
        begin = np.ascontiguousarray(row_begin, dtype=np.uint64)
        assert len(total) == len(begin) == len(self._bins)
        _check(load_library().gn_filter_probe_paths_shared_window(self._h, _p(probes), len(probes), paths.ctypes.data_as(C.c_void_p), paths.shape[0],
                                                                  paths.shape[1], _p(total), _p(begin), _p(alive),
                                                                  self._plane_pointers(planes, paths.shape[0], paths.shape[1])))

    def bin_popcounts(self, bins: Optional[int] = None, ibf_idx: int = 0) -> np.ndarray:
        """gn_filter_bin_popcounts: set bits per technical bin of IBF ibf_idx -> uint64 [bins of that IBF].  The library writes as many
        counts as the IBF has bins, so the buffer is sized from the shapes the filter was created with; `bins`, when given, has to agree
        (a filter wrapped around a bare handle knows no shapes: `bins` is then required and trusted)."""
        if self._bins is not None:
            if not 0 <= ibf_idx < len(self._bins):
                raise GanonHipError(-22, f"gn_filter_bin_popcounts: ibf {ibf_idx} of {len(self._bins)}")
            if bins is not None and bins != self._bins[ibf_idx]:
                raise ValueError(f"IBF {ibf_idx} has {self._bins[ibf_idx]} bins, not {bins}")
            bins = self._bins[ibf_idx]
        elif bins is None:
            raise ValueError("bins is required for a filter whose shapes are not known")
        out = np.zeros(bins, dtype=np.uint64)
        _check(load_library().gn_filter_bin_popcounts(self._h, ibf_idx, _p(out)))
        return out

    def copy_ibf(self, dst_ibf: int, src: "HipFilter", src_ibf: int) -> None:
        """gn_filter_copy_ibf: IBF src_ibf of the HIBF `src` into this HIBF's IBF dst_ibf (same rows, at least as many bins)"""
        _check(load_library().gn_filter_copy_ibf(self._h, dst_ibf, src._h, src_ibf))

    def copy_ibf_spans(self, dst_ibf: int, src: "HipFilter", src_ibf: int, spans) -> None:
        """gn_filter_copy_ibf_spans: bins [src_first, src_first + n_bins) of IBF src_ibf of the HIBF `src` become bins [dst_first, dst_first +
        n_bins) of this HIBF's IBF dst_ibf, for every span (src_first, dst_first, n_bins); every other bit of the destination is cleared"""
        spans = np.asarray(spans, dtype=np.int64).reshape(-1, 3)
        if ((spans < 0) | (spans > 0xFFFFFFFF)).any():
            raise ValueError("a span does not fit 32 bits")
        table = np.zeros((len(spans), 4), dtype=np.uint32)  # gn_bin_span: src_first, dst_first, n_bins, reserved
        table[:, :3] = spans
        _check(load_library().gn_filter_copy_ibf_spans(self._h, dst_ibf, src._h, src_ibf, _p(table) if len(table) else None, len(table)))

    def fold_ibf(self, dst_ibf: int, dst_first: int, n_groups: int, src: "HipFilter", src_ibf: int, members) -> None:
        """gn_filter_fold_ibf: bin dst_first + g of this HIBF's IBF dst_ibf is ORed, row by row, with the OR of bins [src_first, src_first +
        n_bins) of IBF src_ibf of the HIBF `src` over the members (src_first, n_bins, group) of group g; nothing else changes"""
        members = np.asarray(members, dtype=np.int64).reshape(-1, 3)
        if ((members < 0) | (members > 0xFFFFFFFF)).any():
            raise ValueError("a member does not fit 32 bits")
        table = np.zeros((len(members), 4), dtype=np.uint32)  # gn_fold_member: src_first, n_bins, group, reserved
        table[:, :3] = members
        _check(load_library().gn_filter_fold_ibf(self._h, dst_ibf, dst_first, n_groups, src._h, src_ibf, _p(table) if len(table) else None, len(table)))

    def probe(self, hashes: np.ndarray, bins: np.ndarray) -> Tuple[int, int, int]:
        """gn_filter_probe -> (hits summed over the bins, hashes in none of the bins, index of the first such hash or -1)"""
        hashes = np.ascontiguousarray(hashes, dtype=np.uint64)
        bins = np.ascontiguousarray(bins, dtype=np.uint32)
        hits, missing, first = C.c_uint64(0), C.c_uint64(0), C.c_uint64(0)
        _check(load_library().gn_filter_probe(self._h, _p(hashes), len(hashes), _p(bins), len(bins), C.byref(hits), C.byref(missing), C.byref(first)))
        return hits.value, missing.value, -1 if first.value == 0xFFFFFFFFFFFFFFFF else first.value

    def fill_random(self, seed: int, and_words: int = 1, word_lo: int = 0, row_words_total: int = 0, ibf_idx: int = 0) -> None:
        """device-side seeded Bernoulli(2**-and_words) fill (gn_filter_fill_random); fill_random_words() is its numpy twin"""
        _check(load_library().gn_filter_fill_random(self._h, ibf_idx, seed & 0xFFFFFFFFFFFFFFFF, and_words, word_lo,
                                                    row_words_total))

    def write_rows(self, row_begin: int, src: np.ndarray, word_lo: int = 0, ibf_idx: int = 0) -> None:
        """streaming upload of rows [row_begin, row_begin+len(src)) from a host chunk [n_rows, src_row_words]"""
        src = np.ascontiguousarray(src, dtype=np.uint64)
        assert src.ndim == 2
        L = load_library()
        _check(L.gn_filter_write_rows(self._h, ibf_idx, row_begin, src.shape[0], _p(src), src.shape[1], word_lo))
        _check(L.gn_filter_write_sync(self._h))

    def finalize(self) -> None:
        _check(load_library().gn_filter_finalize(self._h))

    def download_row_list(self, row_idx: np.ndarray, words: int, ibf_idx: int = 0) -> np.ndarray:
        row_idx = np.ascontiguousarray(row_idx, dtype=np.uint64)
        out = np.empty((len(row_idx), words), dtype=np.uint64)
        _check(load_library().gn_filter_download_row_list(self._h, ibf_idx, _p(row_idx), len(row_idx), _p(out)))
        return out

    def download_rows(self, row_begin: int, n_rows: int, words: int, ibf_idx: int = 0) -> np.ndarray:
        out = np.empty((n_rows, words), dtype=np.uint64)
        _check(load_library().gn_filter_download_rows(self._h, ibf_idx, row_begin, n_rows, _p(out)))
        return out

    def info(self) -> dict:
        a, b, c, d = C.c_int(), C.c_uint32(), C.c_uint64(), C.c_uint64()
        _check(load_library().gn_filter_info(self._h, C.byref(a), C.byref(b), C.byref(c), C.byref(d)))
        return dict(is_hibf=bool(a.value), n_ibf=b.value, n_targets=c.value, device_bytes=d.value)

    def set_stream_rows_min_bytes(self, n_bytes: int) -> None:
        """row storage from which this filter's fast count launches take the stream kernels, non-temporal row loads
        (gn_filter_set_stream_rows_min_bytes; default 2 GiB or $GANON_HIP_STREAM_ROWS_MIN_BYTES, 0 = whenever an instance exists)"""
        _check(load_library().gn_filter_set_stream_rows_min_bytes(self._h, int(n_bytes)))

    def free(self) -> None:
        if self._h:
            load_library().gn_filter_free(self._h)
            self._h = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


class HipStream:
    """Batch context (gn_stream): upload reads, classify, fetch sparse matches."""

    def __init__(self, flt: HipFilter, max_reads: int, max_bases: int, max_matches: int = 0):
        self._f = flt
        self._h = C.c_void_p()
        _check(load_library().gn_stream_create(flt._h, max_reads, max_bases, max_matches, C.byref(self._h)))
        self.n_reads = 0

    def upload(self, bases: np.ndarray, off1: np.ndarray, off2: Optional[np.ndarray] = None) -> None:
        bases = np.ascontiguousarray(bases, dtype=np.uint8)
        off1 = np.ascontiguousarray(off1, dtype=np.uint64)
        if off2 is not None:
            off2 = np.ascontiguousarray(off2, dtype=np.uint64)
        self.n_reads = len(off1) - 1
        self._keep = (bases, off1, off2)
        _check(load_library().gn_stream_upload_reads(self._h, _p(bases), bases.size, _p(off1), _p(off2), self.n_reads))

    def minimisers(self, k: int, w: int) -> None:
        """hash only (no filter lookup); results via fetch_hashes()"""
        _check(load_library().gn_stream_minimisers(self._h, k, w))

    def classify(self, k: int, w: int, rel_cutoff: float) -> None:
        _check(load_library().gn_stream_classify(self._h, k, w, float(rel_cutoff)))

    def classify_shared(self, source: "HipStream", rel_cutoff: float) -> None:
        """count the batch resident (and hashed) in `source` against this stream's filter too (gn_stream_classify_shared)"""
        self.n_reads = source.n_reads
        _check(load_library().gn_stream_classify_shared(self._h, source._h, float(rel_cutoff)))

    def submit(self, bases, off1, off2, k: int, w: int, rel_cutoff: float) -> None:
        self.upload(bases, off1, off2)
        self.classify(k, w, rel_cutoff)

    def upload_fastq(self, text, fasta=False) -> Tuple[int, int, int]:
        """four-line FASTQ text (or two-line FASTA text), tokenised on the device (gn_stream_upload_text + gn_stream_fastq_index):
        -> (reads, bases, parsed_bytes); the stream then holds the reads like after upload()"""
        text = np.ascontiguousarray(np.frombuffer(text, dtype=np.uint8) if isinstance(text, (bytes, bytearray)) else text, dtype=np.uint8)
        self._keep = (text,)
        L = load_library()
        _check(L.gn_stream_upload_text(self._h, _p(text), text.size, int(fasta)))
        n, nb, pb = C.c_uint32(), C.c_uint64(), C.c_uint64()
        _check(L.gn_stream_fastq_index(self._h, C.byref(n), C.byref(nb), C.byref(pb)))
        self.n_reads = n.value
        return n.value, nb.value, pb.value

    def upload_text_device(self, d_text: int, n_bytes: int, fasta=False, src_device: int = 0) -> Tuple[int, int, int]:
        """the same for a text that lies in device memory (gn_stream_upload_text_device): -> (reads, bases, parsed_bytes)"""
        L = load_library()
        _check(L.gn_stream_upload_text_device(self._h, C.c_void_p(d_text), n_bytes, int(fasta), src_device))
        n, nb, pb = C.c_uint32(), C.c_uint64(), C.c_uint64()
        _check(L.gn_stream_fastq_index(self._h, C.byref(n), C.byref(nb), C.byref(pb)))
        self.n_reads = n.value
        return n.value, nb.value, pb.value

    def fastq_headers(self) -> Tuple[bytes, np.ndarray]:
        """gn_stream_fastq_headers: the batch's header lines back to back, and record i's offset (n_reads + 1 entries)"""
        L = load_library()
        off = np.empty(self.n_reads + 1, dtype=np.uint32)
        cap = max(4096, 64 * self.n_reads)
        for _ in range(2):
            dst = np.empty(cap, dtype=np.uint8)
            nb = C.c_uint64()
            rc = L.gn_stream_fastq_headers(self._h, _p(dst), cap, _p(off), C.byref(nb))
            if rc == -75:
                cap = int(nb.value) + 64
                continue
            _check(rc)
            return dst[:nb.value].tobytes(), off
        raise GanonHipError(-75, "gn_stream_fastq_headers: the header lines did not fit twice")

    def upload_text_pair(self, text1, text2, fasta=False) -> Tuple[int, int, int]:
        """the two mate files' pieces as text -> (pairs, parsed_bytes1, parsed_bytes2); the stream then holds the pairs like after upload()"""
        t1, t2 = (np.ascontiguousarray(np.frombuffer(t, dtype=np.uint8) if isinstance(t, (bytes, bytearray)) else t, dtype=np.uint8) for t in (text1, text2))
        self._keep = (t1, t2)
        L = load_library()
        _check(L.gn_stream_upload_text_pair(self._h, _p(t1), t1.size, _p(t2), t2.size, int(fasta)))
        n, p1, p2 = C.c_uint32(), C.c_uint64(), C.c_uint64()
        _check(L.gn_stream_text_pair_index(self._h, C.byref(n), C.byref(p1), C.byref(p2)))
        self.n_reads = n.value
        return n.value, p1.value, p2.value

    def text_pair_records2(self):
        out = [np.empty(self.n_reads, dtype=np.uint32) for _ in range(3)]
        _check(load_library().gn_stream_text_pair_records2(self._h, _p(out[0]), _p(out[1]), _p(out[2])))
        return tuple(out)

    def fastq_keep(self, n_reads: int) -> None:
        _check(load_library().gn_stream_fastq_keep(self._h, n_reads))
        self.n_reads = n_reads

    def fastq_records(self):
        """(rec_at, seq_at, seq_len): uint32 per read, offsets into the uploaded text"""
        out = [np.empty(self.n_reads, dtype=np.uint32) for _ in range(3)]
        _check(load_library().gn_stream_fastq_records(self._h, _p(out[0]), _p(out[1]), _p(out[2])))
        return tuple(out)

    def upload_genome_text(self, text, w: int, stride: int, min_length: int = 0, continues: bool = False, open_end: bool = False) -> None:
        """wrapped multi-record FASTA text, tokenised and cut into pieces on the device (gn_stream_upload_genome_text; asynchronous).
        continues: text[0] goes on with the record the previous text left open; open_end: the text ends inside its last record"""
        text = np.ascontiguousarray(np.frombuffer(text, dtype=np.uint8) if isinstance(text, (bytes, bytearray)) else text, dtype=np.uint8)
        self._keep = (text,)
        flags = (GENOME_CONTINUES if continues else 0) | (GENOME_OPEN_END if open_end else 0)
        _check(load_library().gn_stream_upload_genome_text(self._h, _p(text), text.size, w, stride, min_length, flags))

    def genome_index(self) -> dict:
        """waits for the tokeniser (gn_stream_genome_index): n_records, n_pieces, n_bases, parsed_bytes, status (0, GENOME_BAD_LETTER,
        GENOME_NO_HEADER), bad_at, open_letters.  The stream then holds the pieces like reads after upload()"""
        nr, npc, st = C.c_uint32(), C.c_uint32(), C.c_int()
        nb, pb, bad, op = C.c_uint64(), C.c_uint64(), C.c_uint64(), C.c_uint64()
        _check(load_library().gn_stream_genome_index(self._h, C.byref(nr), C.byref(npc), C.byref(nb), C.byref(pb), C.byref(st), C.byref(bad), C.byref(op)))
        self.n_reads = npc.value
        self._genome_records = nr.value
        return dict(n_records=nr.value, n_pieces=npc.value, n_bases=nb.value, parsed_bytes=pb.value, status=st.value, bad_at=bad.value,
                    open_letters=op.value)

    def genome_records(self):
        """(rec_at u64, rec_letters u64, rec_state u8) per record of the tokenised genome text (gn_stream_genome_records)"""
        n = self._genome_records
        out = (np.empty(n, dtype=np.uint64), np.empty(n, dtype=np.uint64), np.empty(n, dtype=np.uint8))
        _check(load_library().gn_stream_genome_records(self._h, _p(out[0]), _p(out[1]), _p(out[2])))
        return out

    def sync(self) -> None:
        _check(load_library().gn_stream_sync(self._h))

    def fetch(self):
        """-> (n_hashes u32[n], status u8[n], match_off u64[n+1], matches MATCH_DTYPE[m])"""
        L = load_library()
        n = self.n_reads
        nh = np.zeros(n, dtype=np.uint32)
        st = np.zeros(n, dtype=np.uint8)
        mo = np.zeros(n + 1, dtype=np.uint64)
        need = C.c_uint64(0)
        _check(L.gn_fetch_batch(self._h, _p(nh), _p(st), _p(mo), None, 0, C.byref(need)))
        m = np.zeros(max(int(need.value), 1), dtype=MATCH_DTYPE)
        _check(L.gn_fetch_batch(self._h, None, None, None, _p(m), len(m), C.byref(need)))
        return nh, st, mo, m[: int(need.value)]

    def set_postfilter(self, rel_filter: Optional[float] = None, fpr_query: float = 1.0, target_fpr=None, joint=False, target_gid=None) -> None:
        """device-side pre-pass of filter_matches on the following batches (gn_stream_set_postfilter); rel_filter=None: off"""
        L = load_library()
        if rel_filter is None:
            _check(L.gn_stream_set_postfilter(self._h, None))
            return
        tf = None if target_fpr is None else np.ascontiguousarray(target_fpr, dtype=np.float64)
        tg = None if target_gid is None else np.ascontiguousarray(target_gid, dtype=np.uint32)
        pf = PostFilter(float(rel_filter), float(fpr_query), None if tf is None else tf.ctypes.data_as(C.c_void_p),
                        2 if tg is not None else (1 if joint else 0), None if tg is None else tg.ctypes.data_as(C.c_void_p))
        _check(L.gn_stream_set_postfilter(self._h, C.byref(pf)))

    def set_long_reads(self, on: bool = True) -> None:
        """classify reads with more than 65535 minimisers too (the reference's -DLONGREADS build); flat IBF only"""
        _check(load_library().gn_stream_set_long_reads(self._h, 1 if on else 0))

    @staticmethod
    def postfilter_joint(streams) -> None:
        """gn_streams_postfilter_joint: the pre-pass over the streams of one hierarchy level (same batch, disjoint targets)"""
        arr = (C.c_void_p * len(streams))(*[st._h for st in streams])
        _check(load_library().gn_streams_postfilter_joint(arr, len(streams)))

    def fetch_postfilter(self):
        """-> (max_count u32[n] before filtering, dropped by --rel-filter, dropped by --fpr-query) of the last batch"""
        mx = np.zeros(self.n_reads, dtype=np.uint32)
        a, b = C.c_uint64(0), C.c_uint64(0)
        _check(load_library().gn_fetch_postfilter(self._h, _p(mx), C.byref(a), C.byref(b)))
        return mx, int(a.value), int(b.value)

    def distinct_hashes(self) -> np.ndarray:
        """sorted distinct minimiser hashes of the resident sequences (gn_stream_distinct_hashes)"""
        L = load_library()
        n = C.c_uint64(0)
        _check(L.gn_stream_distinct_hashes(self._h, None, 0, C.byref(n)))
        out = np.zeros(max(int(n.value), 1), dtype=np.uint64)
        _check(L.gn_stream_distinct_hashes(self._h, _p(out), len(out), C.byref(n)))
        return out[: int(n.value)]

    def distinct_hashes_packed(self):
        """that set packed on the device (gn_stream_distinct_hashes_packed) -> (hashes, blocks as PACKED_BLOCK_DTYPE, payload words)"""
        L = load_library()
        n, nb, nw = C.c_uint64(0), C.c_uint64(0), C.c_uint64(0)
        _check(L.gn_stream_distinct_hashes_packed(self._h, None, 0, None, 0, C.byref(n), C.byref(nb), C.byref(nw)))
        blocks = np.zeros(max(int(nb.value), 1), dtype=PACKED_BLOCK_DTYPE)
        words = np.zeros(max(int(nw.value), 1), dtype=np.uint64)
        _check(L.gn_stream_distinct_hashes_packed(self._h, blocks.ctypes.data_as(C.c_void_p), int(nb.value), _p(words), int(nw.value), C.byref(n), C.byref(nb),
                                                  C.byref(nw)))
        return int(n.value), blocks[: int(nb.value)], words[: int(nw.value)]

    def fetch_read_info(self):
        """-> (n_hashes u32[n], status u8[n]) only"""
        n = self.n_reads
        nh = np.zeros(n, dtype=np.uint32)
        st = np.zeros(n, dtype=np.uint8)
        need = C.c_uint64(0)
        _check(load_library().gn_fetch_batch(self._h, _p(nh), _p(st), None, None, 0, C.byref(need)))
        return nh, st

    def device_records(self, device_index: int = 0):
        """the batch's matches as an int32 torch tensor [m, 3] (read, target, count) that ALIASES the library's device
        buffer (gn_stream_device_matches); valid until the next submit on this stream"""
        import torch
        ptr, n = C.c_void_p(), C.c_uint64(0)
        _check(load_library().gn_stream_device_matches(self._h, C.byref(ptr), C.byref(n)))
        if n.value == 0:
            return torch.empty((0, 3), dtype=torch.int32, device=f"cuda:{device_index}")

        class _Dev:  # __cuda_array_interface__ v2: torch wraps the pointer without copying
            __cuda_array_interface__ = {"data": (int(ptr.value), False), "shape": (int(n.value), 3), "typestr": "<i4",
                                        "version": 2}
        return torch.as_tensor(_Dev(), device=f"cuda:{device_index}")

    def device_offsets(self, device_index: int = 0):
        """the n_reads+1 per-read offsets that go with device_records(), as an int64 torch tensor ALIASING the library's buffer"""
        import torch
        ptr = C.c_void_p()
        _check(load_library().gn_stream_device_offsets(self._h, C.byref(ptr)))

        class _Dev:
            __cuda_array_interface__ = {"data": (int(ptr.value), False), "shape": (self.n_reads + 1,), "typestr": "<i8", "version": 2}
        return torch.as_tensor(_Dev(), device=f"cuda:{device_index}")

    def fetch_hashes(self):
        """-> (hash_off u64[n+1], hashes u64[total]) in emission order (parity tap)."""
        L = load_library()
        n = self.n_reads
        ho = np.zeros(n + 1, dtype=np.uint64)
        tot = C.c_uint64(0)
        _check(L.gn_stream_fetch_hashes(self._h, _p(ho), None, 0, C.byref(tot)))
        hs = np.zeros(max(int(tot.value), 1), dtype=np.uint64)
        _check(L.gn_stream_fetch_hashes(self._h, _p(ho), _p(hs), len(hs), C.byref(tot)))
        return ho, hs[: int(tot.value)]

    def dense_counts(self, read_begin: int, read_end: int, width: int) -> np.ndarray:
        out = np.zeros((read_end - read_begin, width), dtype=np.uint16)
        _check(load_library().gn_stream_dense_counts(self._h, read_begin, read_end, _p(out)))
        return out

    def timings(self) -> dict:
        t = Timings()
        _check(load_library().gn_stream_timings(self._h, C.byref(t)))
        return dict(ms_minimiser=t.ms_minimiser, ms_count=t.ms_count, ms_total=t.ms_total, n_hashes=t.n_hashes,
                    algo_bytes=t.algo_bytes, n_matches=t.n_matches, n_count_launches=t.n_count_launches,
                    fetched_bytes=t.fetched_bytes, ms_compact=t.ms_compact)

    def screen_deferred(self) -> int:
        """units of the last batch the fast count kernel's screen-only launch left to the launch after it (gn_stream_screen_deferred)"""
        n = C.c_uint64(0)
        _check(load_library().gn_stream_screen_deferred(self._h, C.byref(n)))
        return int(n.value)

    def rows_streamed(self) -> bool:
        """whether the fast count launches of the last classify took the stream kernels: non-temporal row loads (gn_stream_rows_streamed)"""
        v = C.c_int(0)
        _check(load_library().gn_stream_rows_streamed(self._h, C.byref(v)))
        return bool(v.value)

    def hibf_levels(self):
        """per tree level of the last HIBF batch: [dict(ms, algo_bytes, table_bytes, row_bytes, line_bytes)] (gn_stream_hibf_levels / _level_lines)"""
        cap = 8
        n = C.c_uint32(0)
        ms = np.zeros(cap, dtype=np.float32)
        ab = np.zeros(cap, dtype=np.uint64)
        tb = np.zeros(cap, dtype=np.uint64)
        rb = np.zeros(cap, dtype=np.uint32)
        _check(load_library().gn_stream_hibf_levels(self._h, C.byref(n), _p(ms), _p(ab), _p(tb), _p(rb), cap))
        lb = np.zeros(cap, dtype=np.uint64)
        _check(load_library().gn_stream_hibf_level_lines(self._h, _p(lb), cap))
        return [dict(ms=float(ms[i]), algo_bytes=int(ab[i]), table_bytes=int(tb[i]), row_bytes=int(rb[i]), line_bytes=int(lb[i])) for i in range(min(cap, n.value))]

    def destroy(self) -> None:
        if self._h:
            load_library().gn_stream_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.destroy()
        except Exception:
            pass
