"""ctypes binding of libffq_hip.so -- the C ABI declared in include/ffq.h.

This module is plumbing only: it loads the in-tree shared library, declares the
argument types and turns error codes into exceptions.  There is no CPU
fallback: if the library is missing or no gfx950 device is usable, everything
here raises.
"""
import ctypes
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
# FFQ_HIP_LIB: another build of the same library (same-box A/B measurements, tools/ab_run.sh)
LIB_PATH = os.environ.get("FFQ_HIP_LIB") or os.path.join(_HERE, "csrc", "libffq_hip.so")

# status codes (include/ffq.h; reference: _fastqandfurious.c:7-15)
INVALID = -1
POS_HEAD_BEG = 0
POS_HEAD_END = 1
POS_SEQ_BEG = 2
POS_SEQ_END = 3
POS_QUAL_BEG = 4
POS_QUAL_END = 5
COMPLETE = 6
MISSING_QUALHEADER_END = 7

END_OK, END_REFILL, END_ERR_FINAL_QUAL, END_ERR_INCOMPLETE, END_ERR_INVALID = range(5)
END_ERR_PAIR_COUNT, END_ERR_PAIR_NAMES = 5, 6      # a pair of streams only (PairStream)
_END_ERRORS = {END_ERR_FINAL_QUAL: 'Incomplete final quality string at byte',
               END_ERR_INCOMPLETE: 'Incomplete entry at byte %i',
               END_ERR_INVALID: 'Entry is invalid at byte %i'}


def raise_for_end(end_state, where):
    """The reference iterator's ValueError (fastqandfurious.py:262, :269, :272) for an END_ERR_* state met at stream byte `where`."""
    text = _END_ERRORS.get(end_state)
    if text is None:
        raise RuntimeError('unknown end state %r' % (end_state,))
    raise ValueError(text % where if '%' in text else text)


def length_bounds(min_len, max_len, open_low=-(1 << 62)):
    """(lo, hi) as the length filter's entry points take them: None is an open bound."""
    return open_low if min_len is None else int(min_len), (1 << 62) if max_len is None else int(max_len)


def _add(add, sentinel):
    """The default of every `add` argument: positions count the stream's bytes, not the sentinel in front of them."""
    return (-1 if sentinel else 0) if add is None else add


ABI_VERSION = 12
OK = 0
E_NODEVICE, E_HIP, E_ARG, E_NOMEM, E_TABLE_FULL, E_INTERNAL, E_TIMEOUT = -1, -2, -3, -4, -5, -6, -7
STAGE_NONE, STAGE_HANDOFF, STAGE_SCAN, STAGE_GATHER = 0, 1, 2, 3      # FFQ_SHARD_STAGE_*
STAGE_NAMES = ("none", "hand-off", "scan", "gather")

# statistics (include/ffq.h: FFQ_STATS_*)
STATS_QBINS, STATS_GCBINS, STATS_HEAD, STATS_MAX_CYCLES = 96, 101, 8, 4096
STATS_IN, STATS_OUT = 1, 2


def stats_words(max_cycles):
    """uint64 words of a block of statistics for max_cycles cycles (FFQ_STATS_WORDS)."""
    return 8 + max_cycles * 101 + (max_cycles + 1) + STATS_QBINS + STATS_GCBINS


F_DECODE_QUAL = 1
F_FORCE_SERIAL = 2
F_FORCE_RANKED = 4
F_POLL_RESULT = 8
F_SINGLE_PASS = 16
SEG_STRIDE = 8704            # FFQ_F_SINGLE_PASS: bytes of the quality buffer every 16 KiB tile of the input owns (include/ffq.h)
INPLACE_STRIDE = 16384       # ... and what admits the in-place layout as well (lines of any length)
PATH_IN_PLACE = 8            # ScanResult.path bit (FFQ_PATH_IN_PLACE): the general path's index pass decoded every byte in place
F_NO_TIMING = 32
F_FORCE_GENERAL = 64        # tests: skip the four-line fast path

# every symbol include/ffq.h declares (tests check the library exports them all)
SYMBOLS = (
    "ffq_abi_version", "ffq_build_id", "ffq_last_error", "ffq_device_count", "ffq_ctx_create", "ffq_ctx_create_shared",
    "ffq_ctx_destroy", "ffq_ctx_reserve", "ffq_ctx_forget", "ffq_ctx_stream", "ffq_dev_alloc", "ffq_dev_free",
    "ffq_pinned_alloc", "ffq_pinned_free", "ffq_copy_h2d", "ffq_copy_d2h", "ffq_sync",
    "ffq_scan_device", "ffq_scan_submit", "ffq_scan_wait", "ffq_scan_host", "ffq_entrypos", "ffq_arrayadd_b_device",
    "ffq_arrayadd_b", "ffq_arrayadd_q_device", "ffq_arrayadd_q", "ffq_table_lower_bound",
    "ffq_table_select_seqlen", "ffq_table_cut", "ffq_table_gather_column", "ffq_stream_open", "ffq_stream_next", "ffq_stream_close",
    "ffq_stream_open2", "ffq_stream_quals", "ffq_stream_tell", "ffq_stream_path",
    "ffq_shard_unique_id", "ffq_shard_create", "ffq_shard_create_lane", "ffq_shard_world_create", "ffq_shard_world_abort",
    "ffq_shard_world_destroy", "ffq_shard_create_local", "ffq_shard_destroy", "ffq_shard_halo", "ffq_shard_exchange_halo",
    "ffq_shard_step_submit", "ffq_shard_step_wait", "ffq_shard_transport", "ffq_shard_self_exchange", "ffq_stream_open_gzip", "ffq_gunzip_fd", "ffq_gunzip_stats", "ffq_bgzf_range", "ffq_stream_open_push",
    "ffq_stream_push_buffer", "ffq_stream_push", "ffq_scan_fasta_device", "ffq_scan_fasta_host",
    "ffq_synth_single",
    "ffq_synth_wrapped_size", "ffq_synth_wrapped", "ffq_selftest", "ffq_shard_load_fd", "ffq_load_fd",
    "ffq_shard_host_step", "ffq_shard_host_free", "ffq_stream_set_filter", "ffq_stream_selected",
    "ffq_shard_create_hosted",
    "ffq_shard_create2", "ffq_shard_scan_fd_slabs", "ffq_table_select_seqlen_idx", "ffq_shard_get_info", "ffq_shard_set_timeout", "ffq_shard_set_serial", "ffq_shard_abort", "ffq_shard_inject_stall",
    "ffq_table_trim_quality", "ffq_stream_set_trim", "ffq_stream_trimmed",
    "ffq_table_render_fastq", "ffq_stream_set_render", "ffq_stream_rendered",
    "ffq_table_trim_adapter", "ffq_stream_set_adapter", "ffq_stream_adapter_trimmed",
    "ffq_table_stats", "ffq_stream_set_stats", "ffq_stream_stats",
    "ffq_table_select_reads", "ffq_ee_micro_table", "ffq_stream_set_content", "ffq_stream_filter_counts",
    "ffq_table_select_pairs", "ffq_table_pair_names",
    "ffq_pair_open", "ffq_pair_wants", "ffq_pair_next", "ffq_pair_rows", "ffq_pair_selected", "ffq_pair_close",
    "ffq_table_pair_overlap", "ffq_pair_set_overlap", "ffq_pair_overlap",
    "ffq_table_pair_merge", "ffq_pair_set_merge", "ffq_pair_merged",
    "ffq_table_pair_correct", "ffq_pair_set_correct", "ffq_pair_corrected",
    "ffq_table_seq_keys", "ffq_seq_key_host", "ffq_pair_key_host", "ffq_dedup_create", "ffq_dedup_destroy", "ffq_dedup_select",
    "ffq_stream_set_dedup", "ffq_stream_dedup_counts", "ffq_pair_set_dedup", "ffq_pair_dedup_counts",
    "ffq_table_trim_poly", "ffq_stream_set_poly", "ffq_stream_poly_trimmed",
    "ffq_table_trim_ends", "ffq_stream_set_ends", "ffq_stream_ends_trimmed",
    "ffq_deflate_bgzf_bound", "ffq_deflate_bgzf", "ffq_bgzf_eof_block",
    "ffq_stream_set_compress", "ffq_stream_compressed", "ffq_pair_set_compress", "ffq_pair_merged_bgzf",
    "ffq_table_take_umi", "ffq_table_render_fastq_umi", "ffq_stream_set_umi", "ffq_stream_umi_counts", "ffq_pair_set_umi",
    "ffq_pair_umi_counts",
)


FILTER_COUNTS = 8            # FFQ_FILTER_COUNTS: rows kept, dropped by rule 1..6, not judged by content
POLY_ANY = -1                # FFQ_POLY_ANY: ffq_table_trim_poly's `base` for poly-X (any of the four bases)
POLY_BASES = {b"A": 0, b"C": 1, b"G": 2, b"T": 3, None: POLY_ANY}
POLY_MIN_LEN = (2, 65535)    # the range of a poly pass's min_len
KEY_NONE = 0                 # FFQ_KEY_NONE: a row without a key (ffq_table_seq_keys)
BGZF_BLOCK_BYTES = 65280     # FFQ_BGZF_BLOCK_BYTES: the bytes ffq_deflate_bgzf puts into a member (what bgzip does)
DEFLATE_SEG_BYTES = 256      # FFQ_DEFLATE_SEG_BYTES: a match does not cross a multiple of this inside its block
DEFLATE_ROUND_POSITIONS = 1024   # FFQ_DEFLATE_ROUND_POSITIONS: a position finds candidates of earlier rounds only
DEFLATE_GRID_BLOCKS = 256    # FFQ_DEFLATE_GRID_BLOCKS: blocks deflated at a time; a workgroup takes every 256th block
COMPRESS_NONE, COMPRESS_BGZF = 0, 1      # FFQ_COMPRESS_*: ffq_stream_set_compress, ffq_pair_set_compress
COMPRESS_MODES = {None: COMPRESS_NONE, "bgzf": COMPRESS_BGZF}
BGZF_EOF = bytes([0x1f, 0x8b, 8, 4, 0, 0, 0, 0, 0, 0xff, 6, 0, 0x42, 0x43, 2, 0, 0x1b, 0, 3, 0, 0, 0, 0, 0, 0, 0, 0, 0])    # ffq_bgzf_eof_block
DEFLATE_COUNTS = 4           # FFQ_DEFLATE_COUNTS: bytes in, bytes out, members, members stored
DEDUP_COUNTS = 6             # FFQ_DEDUP_COUNTS: rows kept, duplicates, rows without a key, distinct keys, slots, rehashes


class ContentRulesStruct(ctypes.Structure):
    """struct ffq_content_rules (include/ffq.h)."""
    _fields_ = [("qual_base", ctypes.c_int32), ("max_n", ctypes.c_int32), ("min_mean_qual", ctypes.c_int32),
                ("qualified_qual", ctypes.c_int32), ("max_unqualified_pct", ctypes.c_int32),
                ("min_complexity_pct", ctypes.c_int32), ("max_ee_micro", ctypes.c_int64)]


def content_rules_struct(rules):
    """What the library takes for `rules`: None, a ContentRulesStruct, or anything with its seven fields as attributes
    (fastqandfurious.ContentRules)."""
    if rules is None or isinstance(rules, ContentRulesStruct):
        return rules
    return ContentRulesStruct(*(int(getattr(rules, name)) for name, _ in ContentRulesStruct._fields_))


ENDS_WINDOW_MAX = 64         # the widest window of ffq_table_trim_ends
ENDS_QUALITY = (1, 93)       # the range of a window's quality


class EndsRulesStruct(ctypes.Structure):
    """struct ffq_ends_rules (include/ffq.h)."""
    _fields_ = [(name, ctypes.c_int32) for name in ("trim_front", "trim_tail", "keep_len", "qual_base", "front_window", "front_quality",
                                                    "right_window", "right_quality", "tail_window", "tail_quality")]


def ends_rules_struct(rules, qual_base=33):
    """What the library takes for `rules`: None or an EndsRulesStruct as it is, or anything with trim_front, trim_tail, keep_len
    (None: no limit) and front, right, tail -- each (window, quality) or None -- as attributes (fastqandfurious.EndRules) and
    `qual_base` beside it."""
    if rules is None or isinstance(rules, EndsRulesStruct):
        return rules
    w = [tuple(int(x) for x in st) if st is not None else (0, 0) for st in (rules.front, rules.right, rules.tail)]
    return EndsRulesStruct(int(rules.trim_front), int(rules.trim_tail), int(rules.keep_len or 0), int(qual_base),
                           w[0][0], w[0][1], w[1][0], w[1][1], w[2][0], w[2][1])


PAIR_FILTERS = {"any": 0, "both": 1, "first": 2}       # FFQ_PAIR_ANY / _BOTH / _FIRST
PAIR_COUNTS = 5              # pairs kept, dropped, only mate 1 failed, only mate 2 failed, both failed


UMI_READ1, UMI_READ2, UMI_PER_READ = 1, 2, 3          # FFQ_UMI_*: where the UMI is
UMI_LOCS = {"read1": UMI_READ1, "read2": UMI_READ2, "per_read": UMI_PER_READ}
UMI_LEN_MAX, UMI_SKIP_MAX, UMI_PREFIX_MAX = 64, 64, 16


class UmiRulesStruct(ctypes.Structure):
    """struct ffq_umi_rules (include/ffq.h)."""
    _fields_ = [("loc", ctypes.c_int32), ("len", ctypes.c_int32), ("skip", ctypes.c_int32), ("delim", ctypes.c_uint8),
                ("prefix_len", ctypes.c_uint8), ("prefix", ctypes.c_uint8 * 16)]


def umi_rules_struct(rules):
    """A UmiRulesStruct of a fastqandfurious.UmiRules (anything with loc, length, skip, prefix and delim; loc a name of
    UMI_LOCS or the C ABI's own number), or the struct itself.  Nothing is checked here: the library answers E_ARG."""
    if rules is None or isinstance(rules, UmiRulesStruct):
        return rules
    prefix, delim = bytes(rules.prefix), bytes(rules.delim)
    loc = UMI_LOCS.get(rules.loc, rules.loc if isinstance(rules.loc, int) else 0)
    r = UmiRulesStruct(int(loc), int(rules.length), int(rules.skip), delim[0] if len(delim) == 1 else 0,
                       min(len(prefix), 255))
    for j, b in enumerate(prefix[:16]):
        r.prefix[j] = b
    return r


class TableView(ctypes.Structure):
    """struct ffq_table_view (include/ffq.h): a mate's buffer and table as the pair passes take them."""
    _fields_ = [("d_buf", ctypes.c_void_p), ("n_bytes", ctypes.c_int64), ("sentinel", ctypes.c_int32), ("add", ctypes.c_int64),
                ("d_table", ctypes.c_void_p)]


def table_view(d_buf, n_bytes, d_table, sentinel=True, add=None):
    """A TableView of raw device pointers; d_buf / n_bytes / sentinel / add as for Context.table_gather_column."""
    return TableView(int(d_buf) if d_buf else None, int(n_bytes), int(bool(sentinel)), int(_add(add, sentinel)),
                     int(d_table) if d_table else None)


OVERLAP_MAX_LEN = 512                            # FFQ_OVERLAP_MAX_LEN: mates above it are not analysed
OVERLAP_HIST_WORDS = 2 * OVERLAP_MAX_LEN + 1     # insert sizes 0..1024
OVERLAP_COUNTS = 6           # pairs analysed, with an overlap, changed, bases removed from mate 1, from mate 2, pairs not analysed
MERGE_COUNTS = 6             # FFQ_MERGE_COUNTS: pairs merged, not merged, bytes of text, bases of the merged reads, positions inside overlaps, of those taken from mate 2


CORRECT_COUNTS = 6           # FFQ_CORRECT_COUNTS: pairs looked at, with a correction, bases corrected in mate 1, in mate 2, mismatch positions, pairs not looked at
CORRECT_MATRIX_WORDS = 20    # FFQ_CORRECT_MATRIX_WORDS: corrections by (class before 0..4, class after 0..3)


class CorrectRulesStruct(ctypes.Structure):
    """struct ffq_correct_rules (include/ffq.h)."""
    _fields_ = [("good_quality", ctypes.c_int32), ("bad_quality", ctypes.c_int32), ("qual_base", ctypes.c_int32)]


def correct_rules_struct(rules, qual_base=33):
    """What the library takes for `rules`: None or a CorrectRulesStruct as it is, or anything with good_quality and bad_quality as
    attributes (fastqandfurious.CorrectionRules) and `qual_base` beside it."""
    if rules is None or isinstance(rules, CorrectRulesStruct):
        return rules
    return CorrectRulesStruct(int(rules.good_quality), int(rules.bad_quality), int(qual_base))


class OverlapRulesStruct(ctypes.Structure):
    """struct ffq_overlap_rules (include/ffq.h)."""
    _fields_ = [("min_overlap", ctypes.c_int32), ("max_diff", ctypes.c_int32), ("diff_permille", ctypes.c_int32), ("trim", ctypes.c_int32)]


def overlap_rules_struct(rules, trim=True):
    """What the library takes for `rules`: an OverlapRulesStruct as it is, or anything with min_overlap, max_diff and
    diff_permille as attributes (fastqandfurious.OverlapRules) and `trim` beside it."""
    if rules is None or isinstance(rules, OverlapRulesStruct):
        return rules
    return OverlapRulesStruct(int(rules.min_overlap), int(rules.max_diff), int(rules.diff_permille), 1 if trim else 0)


def _pair_filter(mode):
    if mode in PAIR_FILTERS:
        return PAIR_FILTERS[mode]
    if isinstance(mode, int):
        return mode                                     # (the library checks the number)
    raise ValueError('pair_filter is "any", "both" or "first"')


class ScanResult(ctypes.Structure):
    _fields_ = [
        ("n_records", ctypes.c_int64),
        ("n_qual_bytes", ctypes.c_int64),
        ("end_offset", ctypes.c_int64),
        ("last_pos", ctypes.c_int64 * 6),
        ("last_status", ctypes.c_int32),
        ("end_state", ctypes.c_int32),
        ("path", ctypes.c_int32),
        ("retries", ctypes.c_int32),
        ("n_lines", ctypes.c_int64),
        ("ms_index", ctypes.c_float),
        ("ms_chain", ctypes.c_float),
        ("ms_decode", ctypes.c_float),
        ("ms_total", ctypes.c_float),
    ]


class ShardResult(ctypes.Structure):
    """ffq_shard_result (include/ffq.h)."""
    _fields_ = [
        ("scan", ScanResult),
        ("n_rows", ctypes.c_int64), ("row_lo", ctypes.c_int64), ("row_hi", ctypes.c_int64),
        ("exit_pos", ctypes.c_int64), ("first_pos", ctypes.c_int64),
        ("n_own_records", ctypes.c_int64), ("record_base", ctypes.c_int64), ("total_records", ctypes.c_int64),
        ("err_byte", ctypes.c_int64),
        ("err_state", ctypes.c_int32), ("rounds", ctypes.c_int32), ("regathers", ctypes.c_int32), ("halo_source", ctypes.c_int32),
        ("handoff_bytes", ctypes.c_int64),
        ("handoff_ms", ctypes.c_float), ("allgather_ms", ctypes.c_float),
        ("d_ext", ctypes.c_void_p), ("tail", ctypes.c_int64), ("head", ctypes.c_int64),
        ("nranks", ctypes.c_int32), ("serial", ctypes.c_int32),
        ("n_slabs", ctypes.c_int64), ("bytes_read", ctypes.c_int64),
    ]


class ShardInfo(ctypes.Structure):
    """ffq_shard_info (include/ffq.h): who is there -- the communicators' rank counts, every rank's PCI bus id --, the
    mode, the watchdog's deadline and where its last trip found the step."""
    _fields_ = [
        ("rank", ctypes.c_int32), ("world", ctypes.c_int32),
        ("nranks_handoff", ctypes.c_int32), ("nranks_gather", ctypes.c_int32),
        ("serial", ctypes.c_int32), ("last_stage", ctypes.c_int32), ("poisoned", ctypes.c_int32), ("n_bus", ctypes.c_int32),
        ("timeout_s", ctypes.c_double),
        ("bus_id", ctypes.c_int64 * 64),
    ]


class ShardPiece(ctypes.Structure):
    """ffq_shard_piece: stream bytes [a, b) go from rank src to rank dst; ptr: where this rank reads / writes them."""
    _fields_ = [("src", ctypes.c_int32), ("dst", ctypes.c_int32), ("a", ctypes.c_int64), ("b", ctypes.c_int64), ("ptr", ctypes.c_void_p)]


_SCAN_CB = ctypes.CFUNCTYPE(ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, ctypes.c_int, ctypes.c_int64, ctypes.c_int,
                            ctypes.c_int64, ctypes.c_void_p, ctypes.c_int64, ctypes.POINTER(ScanResult))
_EXCHANGE_CB = ctypes.CFUNCTYPE(ctypes.c_int, ctypes.c_void_p, ctypes.POINTER(ShardPiece), ctypes.c_int)
_GATHER_CB = ctypes.CFUNCTYPE(ctypes.c_int, ctypes.c_void_p, ctypes.POINTER(ctypes.c_int64), ctypes.POINTER(ctypes.c_int64))


class ShardHostOps(ctypes.Structure):
    """ffq_shard_host_ops (include/ffq.h)."""
    _fields_ = [("user", ctypes.c_void_p), ("scan", _SCAN_CB), ("exchange", _EXCHANGE_CB), ("allgather", _GATHER_CB)]


class FFQError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__("libffq_hip error %d: %s" % (code, msg))
        self.code = code


class FFQTimeout(FFQError, TimeoutError):
    """A shard step's watchdog (E_TIMEOUT): the message names the stage (hand-off / scan / gather), the transport, the mode
    and the ranks whose words are missing.  The shard is poisoned: abort() + close(), then build a new one."""


class FFQGzipError(FFQError, OSError):
    """Corrupt gzip input met by the stream front end's reader: also an OSError, as gzip.BadGzipFile is."""


class FFQGzipTruncated(FFQError, EOFError):
    """A gzip file that ends before its end-of-stream marker: also an EOFError, as Python's gzip raises."""


_lib = None
_probe = False      # use_probe_build(): tools load the instrumented build instead of the product library


def _share_torch_hip_runtime():
    """One process, one HIP runtime.  PyTorch-ROCm bundles its own libamdhip64; if this
    library's (the system ROCm one) initialises first, torch later finds "No HIP GPUs".  When
    torch is installed, load ITS runtime before libffq_hip.so so that both resolve to it --
    the order that `import torch` first gives anyway.  Without torch nothing happens."""
    try:
        import importlib.util
        spec = importlib.util.find_spec("torch")
        if spec is None or not spec.submodule_search_locations:
            return
        path = os.path.join(list(spec.submodule_search_locations)[0], "lib", "libamdhip64.so")
        if os.path.exists(path):
            ctypes.CDLL(path, mode=ctypes.RTLD_GLOBAL)
    except Exception:
        pass


def use_probe_build():
    """tools/ only: load libffq_probe.so (the same sources compiled with -DFFQ_PROBES: the file
    loader's ablation switch FFQ_LOAD_ABLATE, the streaming-read probe of include/ffq_probe.h) in
    place of the product library.  Must be called before the first use of lib()."""
    global _probe, LIB_PATH
    assert _lib is None, "use_probe_build() must come before the library is loaded"
    from . import build as _build
    _probe = True
    LIB_PATH = _build.build_probe()


def _checked_build():
    """The in-tree library must be the build of the sources in the tree: compare the id baked
    into it (ffq_build_id) with the hash of csrc/ + include/ and rebuild on a mismatch; if that
    is not possible, refuse.  (FFQ_HIP_LIB names another build on purpose: not checked.)"""
    if os.environ.get("FFQ_HIP_LIB") or _probe:
        return
    from . import build as _build
    want = _build.source_id()
    if os.path.exists(LIB_PATH) and _build.built_id(LIB_PATH) == want:
        return
    if os.environ.get("FFQ_TRUST_BUILD") == "1" and os.path.exists(LIB_PATH):
        # a read-only install / a box without hipcc: the caller takes responsibility (the ABI version is still checked)
        import warnings
        warnings.warn("%s carries build id %s, the sources in this tree hash to %s: loaded as it is (FFQ_TRUST_BUILD=1)"
                      % (LIB_PATH, _build.built_id(LIB_PATH), want))
        return
    try:
        _build.build()
    except Exception as e:      # noqa: BLE001
        raise FFQError(E_NODEVICE,
                       "%s is missing or was not built from the sources in this tree (build id %s, "
                       "sources %s) and cannot be rebuilt here: %s.  Build it with `python "
                       "fastq-and-furious_amd/build.py` (there is no CPU fallback for the scan path)"
                       % (LIB_PATH, _build.built_id(LIB_PATH), want, e))
    if _build.built_id(LIB_PATH) != want:
        raise FFQError(E_INTERNAL, "%s does not carry the build id of its sources after a rebuild" % LIB_PATH)


class _MissingExport:
    """An export the library named by FFQ_HIP_LIB does not have: an error when CALLED, not when bound."""

    def __init__(self, name):
        self._name = name
        self.argtypes = self.restype = None

    def __call__(self, *a):
        raise FFQError(E_INTERNAL, "%s: the library named by FFQ_HIP_LIB (%s) does not export it" % (self._name, LIB_PATH))


class _OtherBuild:
    """FFQ_HIP_LIB names another build on purpose (tools/ab_*.sh: an OLDER commit's library under this tree's Python for a
    same-box A/B): what it lacks is bound to _MissingExport.  The in-tree library never goes through this."""

    def __init__(self, cdll):
        self.__dict__["_cdll"] = cdll

    def __getattr__(self, name):
        try:
            f = getattr(self._cdll, name)
        except AttributeError:
            f = _MissingExport(name)
        self.__dict__[name] = f
        return f


def build_id():
    """The source hash baked into the loaded library (== build.source_id() of this tree)."""
    return lib().ffq_build_id().decode("ascii")


def lib():
    """The loaded library.  Raises if it has not been built and cannot be."""
    global _lib
    if _lib is None:
        if os.environ.get("FFQ_USE_PROBE_BUILD") == "1" and not _probe:
            use_probe_build()            # (tools: FFQ_LOAD_ABLATE lives in the instrumented build)
        _share_torch_hip_runtime()
        _checked_build()
        if not os.path.exists(LIB_PATH):
            raise FFQError(E_NODEVICE,
                           "%s is missing: build it with `python fastq-and-furious_amd/build.py` "
                           "(there is no CPU fallback for the scan path)" % LIB_PATH)
        L = ctypes.CDLL(LIB_PATH)
        if os.environ.get("FFQ_HIP_LIB"):
            L = _OtherBuild(L)
        vp, i64, i32, u32, u64 = (ctypes.c_void_p, ctypes.c_int64, ctypes.c_int, ctypes.c_uint32,
                                  ctypes.c_uint64)
        P = ctypes.POINTER
        L.ffq_abi_version.restype = i32
        L.ffq_build_id.restype = ctypes.c_char_p
        L.ffq_last_error.restype = ctypes.c_char_p
        L.ffq_device_count.restype = i32
        L.ffq_ctx_create.argtypes = [i32, P(vp)]
        L.ffq_ctx_create_shared.argtypes = [vp, P(vp)]
        L.ffq_ctx_destroy.argtypes = [vp]
        L.ffq_ctx_destroy.restype = None
        L.ffq_ctx_reserve.argtypes = [vp, i64]
        L.ffq_ctx_forget.argtypes = [vp]
        L.ffq_ctx_forget.restype = None
        L.ffq_ctx_stream.argtypes = [vp]
        L.ffq_ctx_stream.restype = vp
        L.ffq_dev_alloc.argtypes = [vp, i64, P(vp)]
        L.ffq_dev_free.argtypes = [vp, vp]
        L.ffq_pinned_alloc.argtypes = [i64, P(vp)]
        L.ffq_pinned_free.argtypes = [vp]
        L.ffq_copy_h2d.argtypes = [vp, vp, vp, i64, i32]
        L.ffq_copy_d2h.argtypes = [vp, vp, vp, i64, i32]
        L.ffq_sync.argtypes = [vp]
        L.ffq_scan_device.argtypes = [vp, vp, i64, i32, i64, i32, i64, u32, i32, vp, i64, vp, i64, vp,
                                      P(ScanResult)]
        L.ffq_scan_submit.argtypes = [vp, vp, i64, i32, i64, i32, i64, u32, i32, vp, i64, vp, i64, vp]
        L.ffq_scan_wait.argtypes = [vp, P(ScanResult)]
        L.ffq_scan_host.argtypes = [vp, vp, i64, i32, i64, i32, i64, u32, i32, vp, i64, vp, i64, vp,
                                    P(ScanResult)]
        L.ffq_entrypos.argtypes = [vp, vp, i64, i64, vp, P(i32)]
        L.ffq_arrayadd_b_device.argtypes = [vp, vp, i64, i32]
        L.ffq_arrayadd_b.argtypes = [vp, vp, i64, i32]
        L.ffq_arrayadd_q_device.argtypes = [vp, vp, i64, i64]
        L.ffq_arrayadd_q.argtypes = [vp, vp, i64, i64]
        L.ffq_table_lower_bound.argtypes = [vp, vp, i64, i32, i64, P(i64)]
        L.ffq_table_select_seqlen.argtypes = [vp, vp, i64, i64, i64, vp, P(i64)]
        L.ffq_table_select_seqlen_idx.argtypes = [vp, vp, i64, i64, i64, vp, vp, P(i64)]
        L.ffq_table_cut.argtypes = [vp, vp, i64, i64, i64, P(i64)]
        L.ffq_table_trim_quality.argtypes = [vp, vp, i64, i32, i64, vp, i64, i32, i32, i32, vp, P(i64)]
        L.ffq_table_trim_adapter.argtypes = [vp, vp, i64, i32, i64, vp, i64, ctypes.c_char_p, i32, i32, i32, vp, P(i64)]
        L.ffq_table_trim_poly.argtypes = [vp, vp, i64, i32, i64, vp, i64, i32, i32, vp, P(i64)]
        L.ffq_table_trim_ends.argtypes = [vp, vp, i64, i32, i64, vp, i64, P(EndsRulesStruct), vp, P(i64)]
        L.ffq_table_stats.argtypes = [vp, vp, i64, i32, i64, vp, i64, i32, i32, i32, vp, P(i64)]
        L.ffq_table_select_reads.argtypes = [vp, vp, i64, i32, i64, vp, i64, i64, i64, P(ContentRulesStruct), vp, vp, P(i64), P(i64)]
        L.ffq_ee_micro_table.argtypes = []
        L.ffq_ee_micro_table.restype = P(u32)
        L.ffq_table_select_pairs.argtypes = [vp, P(TableView), P(TableView), i64, P(i64), P(ContentRulesStruct), P(ContentRulesStruct),
                                             i32, vp, vp, vp, P(i64), P(i64), P(i64), P(i64)]
        L.ffq_table_pair_names.argtypes = [vp, P(TableView), P(TableView), i64, P(i64)]
        L.ffq_pair_open.argtypes = [vp, vp, i32, i32, P(vp)]
        L.ffq_pair_wants.argtypes = [vp]
        L.ffq_pair_next.argtypes = [vp, P(i64), P(i64), P(i32), P(i32), P(i64)]
        L.ffq_pair_rows.argtypes = [vp, i32, P(vp), P(vp), P(i64), P(i64)]
        L.ffq_pair_selected.argtypes = [vp, P(vp), P(i64)]
        L.ffq_pair_close.argtypes = [vp]
        L.ffq_table_pair_overlap.argtypes = [vp, P(TableView), P(TableView), i64, P(OverlapRulesStruct), vp, vp, vp, vp, i32, P(i64)]
        L.ffq_pair_set_overlap.argtypes = [vp, P(OverlapRulesStruct)]
        L.ffq_pair_overlap.argtypes = [vp, P(i64), vp, i64]
        L.ffq_table_pair_merge.argtypes = [vp, P(TableView), P(TableView), i64, vp, vp, vp, i64, vp, vp, vp, vp, P(i64), P(i64)]
        L.ffq_pair_set_merge.argtypes = [vp, i32]
        L.ffq_table_pair_correct.argtypes = [vp, P(TableView), P(TableView), i64, vp, P(CorrectRulesStruct), P(i64), P(i64)]
        L.ffq_pair_set_correct.argtypes = [vp, P(CorrectRulesStruct)]
        L.ffq_pair_corrected.argtypes = [vp, P(i64), P(i64)]
        L.ffq_pair_merged.argtypes = [vp, P(vp), P(i64), P(i64)]
        L.ffq_pair_close.restype = None
        L.ffq_table_seq_keys.argtypes = [vp, vp, i64, i32, i64, vp, i64, vp, P(i64)]
        L.ffq_seq_key_host.argtypes = [ctypes.c_char_p, i64]
        L.ffq_seq_key_host.restype = u64
        L.ffq_pair_key_host.argtypes = [u64, u64]
        L.ffq_pair_key_host.restype = u64
        L.ffq_dedup_create.argtypes = [vp, i64, i64, P(vp)]
        L.ffq_dedup_destroy.argtypes = [vp]
        L.ffq_dedup_destroy.restype = None
        L.ffq_dedup_select.argtypes = [vp, vp, vp, vp, i64, vp, vp, vp, vp, vp, P(i64), i32, P(i64)]
        L.ffq_stream_set_dedup.argtypes = [vp, i32, i64, i64]
        L.ffq_stream_dedup_counts.argtypes = [vp, P(i64)]
        L.ffq_pair_set_dedup.argtypes = [vp, i32, i64, i64]
        L.ffq_pair_dedup_counts.argtypes = [vp, P(i64)]
        L.ffq_stream_set_content.argtypes = [vp, P(ContentRulesStruct)]
        L.ffq_stream_filter_counts.argtypes = [vp, P(i64)]
        L.ffq_table_render_fastq.argtypes = [vp, vp, i64, i32, i64, vp, i64, vp, i64, vp, P(i64)]
        L.ffq_table_take_umi.argtypes = [vp, vp, i64, i32, i64, vp, i64, i32, i32, vp, P(i64)]
        L.ffq_table_render_fastq_umi.argtypes = [vp, P(TableView), i64, P(TableView), P(TableView), P(UmiRulesStruct), vp, i64, vp, P(i64)]
        L.ffq_deflate_bgzf_bound.argtypes = [i64]
        L.ffq_deflate_bgzf_bound.restype = i64
        L.ffq_deflate_bgzf.argtypes = [vp, vp, i64, vp, i64, vp, P(i64)]
        L.ffq_bgzf_eof_block.argtypes = [vp]
        L.ffq_bgzf_eof_block.restype = None
        L.ffq_table_gather_column.argtypes = [vp, vp, i64, i32, i64, vp, i64, i32, i32, i32, i32, vp, i64, vp, P(i64)]
        L.ffq_stream_open.argtypes = [vp, i32, i64, P(vp)]
        L.ffq_stream_next.argtypes = [vp, P(vp), P(i64), P(i32), P(i64), P(vp), P(i64), P(i64)]
        L.ffq_stream_close.argtypes = [vp]
        L.ffq_scan_fasta_device.argtypes = [vp, vp, i64, i32, i64, i64, vp, i64, P(ScanResult)]
        L.ffq_scan_fasta_host.argtypes = [vp, vp, i64, i32, i64, i64, vp, i64, P(ScanResult)]
        L.ffq_stream_open2.argtypes = [vp, i32, i64, u32, i32, i64, P(vp)]
        L.ffq_stream_open_gzip.argtypes = [vp, i32, i64, u32, i32, i64, P(vp)]
        L.ffq_gunzip_fd.argtypes = [i32, vp, i64, i64, i32, P(i64)]
        L.ffq_gunzip_fd.restype = i64
        L.ffq_gunzip_stats.argtypes = [P(i64)]
        L.ffq_gunzip_stats.restype = None
        L.ffq_bgzf_range.argtypes = [i32, i64, i64, vp, i64, i32, P(i64), P(i64), P(i64), P(i64)]
        L.ffq_stream_open_push.argtypes = [vp, i64, u32, i32, P(vp)]
        L.ffq_stream_push_buffer.argtypes = [vp, P(vp), P(i64)]
        L.ffq_stream_push.argtypes = [vp, i64, i32]
        L.ffq_stream_tell.argtypes = [vp]
        L.ffq_stream_tell.restype = i64
        L.ffq_stream_path.argtypes = [vp]
        L.ffq_stream_path.restype = i32
        L.ffq_shard_unique_id.argtypes = [vp]
        L.ffq_shard_create.argtypes = [vp, vp, i32, i32, P(i64), i64, i64, P(vp)]
        L.ffq_shard_create2.argtypes = [vp, vp, i32, i32, P(i64), i64, i64, u32, P(vp)]
        L.ffq_shard_create_lane.argtypes = [vp, vp, P(vp)]
        L.ffq_shard_world_create.argtypes = [i32, P(vp)]
        L.ffq_shard_world_abort.argtypes = [vp]
        L.ffq_shard_world_abort.restype = None
        L.ffq_shard_world_destroy.argtypes = [vp]
        L.ffq_shard_world_destroy.restype = None
        L.ffq_shard_create_local.argtypes = [vp, vp, i32, P(i64), i64, i64, P(vp)]
        L.ffq_shard_destroy.argtypes = [vp]
        L.ffq_shard_destroy.restype = None
        L.ffq_shard_halo.argtypes = [vp, P(i64), P(i64)]
        L.ffq_shard_exchange_halo.argtypes = [vp, vp, i32]
        L.ffq_shard_step_submit.argtypes = [vp, vp, i32, u32, i32, vp, i64, vp, i64, vp]
        L.ffq_shard_step_wait.argtypes = [vp, P(ShardResult)]
        L.ffq_shard_self_exchange.argtypes = [vp, vp, vp, i64]
        L.ffq_shard_transport.argtypes = [vp]
        L.ffq_shard_transport.restype = ctypes.c_char_p
        L.ffq_shard_get_info.argtypes = [vp, P(ShardInfo)]
        L.ffq_shard_set_timeout.argtypes = [vp, ctypes.c_double]
        L.ffq_shard_set_serial.argtypes = [vp, i32]
        L.ffq_shard_abort.argtypes = [vp]
        L.ffq_shard_inject_stall.argtypes = [vp, i32, ctypes.c_double]
        L.ffq_shard_load_fd.argtypes = [vp, i32, vp, P(i64)]
        L.ffq_shard_scan_fd_slabs.argtypes = [vp, i32, i64, u32, vp, i64, P(ShardResult)]
        L.ffq_load_fd.argtypes = [vp, i32, i64, i64, vp, P(i64)]
        L.ffq_shard_host_step.argtypes = [P(ShardHostOps), vp, i32, i32, P(i64), i64, i64, vp, vp, i64, P(ShardResult)]
        L.ffq_shard_create_hosted.argtypes = [vp, P(ShardHostOps), i32, i32, P(i64), i64, i64, P(vp)]
        L.ffq_shard_host_free.argtypes = [vp]
        L.ffq_shard_host_free.restype = None
        L.ffq_stream_set_filter.argtypes = [vp, i64, i64, i32, i32]
        L.ffq_stream_set_trim.argtypes = [vp, i32, i32, i32]
        L.ffq_stream_trimmed.argtypes = [vp, P(i64)]
        L.ffq_stream_set_adapter.argtypes = [vp, ctypes.c_char_p, i32, i32, i32]
        L.ffq_stream_adapter_trimmed.argtypes = [vp, P(i64)]
        L.ffq_stream_set_poly.argtypes = [vp, i32, i32]
        L.ffq_stream_set_ends.argtypes = [vp, P(EndsRulesStruct)]
        L.ffq_stream_ends_trimmed.argtypes = [vp, P(i64)]
        L.ffq_stream_poly_trimmed.argtypes = [vp, P(i64), P(i64)]
        L.ffq_stream_set_umi.argtypes = [vp, P(UmiRulesStruct)]
        L.ffq_stream_umi_counts.argtypes = [vp, P(i64)]
        L.ffq_pair_set_umi.argtypes = [vp, P(UmiRulesStruct)]
        L.ffq_pair_umi_counts.argtypes = [vp, P(i64), P(i64)]
        L.ffq_stream_set_stats.argtypes = [vp, i32, i32, i32]
        L.ffq_stream_stats.argtypes = [vp, i32, vp, i64]
        L.ffq_stream_set_render.argtypes = [vp]
        L.ffq_stream_rendered.argtypes = [vp, P(vp), P(i64), P(i64)]
        L.ffq_stream_set_compress.argtypes = [vp, i32]
        L.ffq_stream_compressed.argtypes = [vp, P(vp), P(i64), P(i64)]
        L.ffq_pair_set_compress.argtypes = [vp, i32]
        L.ffq_pair_merged_bgzf.argtypes = [vp, P(vp), P(i64), P(i64)]
        L.ffq_stream_selected.argtypes = [vp, P(vp), P(i64), P(vp), P(vp), P(i64)]
        L.ffq_stream_quals.argtypes = [vp, P(vp), P(vp), P(i64)]
        L.ffq_stream_close.restype = None
        L.ffq_synth_single.argtypes = [vp, vp, i64, i64, u64]
        L.ffq_synth_wrapped_size.argtypes = [i64, u64]
        L.ffq_synth_wrapped_size.restype = i64
        L.ffq_synth_wrapped.argtypes = [vp, vp, vp, i64, i64, u64]
        L.ffq_selftest.argtypes = [vp]
        _lib = L
    return _lib


def last_error():
    """the calling thread's last error text (ffq_last_error)"""
    return lib().ffq_last_error().decode("utf-8", "replace")


def check(rc, allow=()):
    if rc != OK and rc not in allow:
        msg = lib().ffq_last_error().decode("utf-8", "replace")
        if "gzip: " in msg:
            # what a drop-in caller of gzip.open() catches: EOFError for a file cut short, BadGzipFile (an OSError) otherwise
            raise (FFQGzipTruncated if "ended before the end-of-stream marker" in msg else FFQGzipError)(rc, msg)
        raise (FFQTimeout if rc == E_TIMEOUT else FFQError)(rc, msg)
    return rc


class Context:
    """One GPU context (stream + scratch).  Not thread-safe; one per thread."""

    def __init__(self, device=0, share=None):
        """share: another Context whose HIP streams this one uses (own scratch); scans of
        the two then execute in submission order (see scan_submit / scan_wait)."""
        self._h = ctypes.c_void_p()
        self._parent = share
        self._children = []          # contexts on this one's streams: they are closed first
        if share is not None:
            self.device = share.device
            check(lib().ffq_ctx_create_shared(share.handle, ctypes.byref(self._h)))
            import weakref
            share._children.append(weakref.ref(self))
        else:
            self.device = device
            check(lib().ffq_ctx_create(int(device), ctypes.byref(self._h)))

    def close(self):
        if self._h:
            for ref in self._children:
                child = ref()
                if child is not None:
                    child.close()
            self._children = []
            lib().ffq_ctx_destroy(self._h)
            self._h = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def handle(self):
        if not self._h:
            raise FFQError(E_ARG, "context is closed")
        return self._h

    def reserve(self, max_bytes):
        check(lib().ffq_ctx_reserve(self.handle, int(max_bytes)))

    def stream(self):
        """The HIP stream (hipStream_t as an integer) every scan of this context runs on."""
        return int(lib().ffq_ctx_stream(self.handle) or 0)

    def forget(self):
        """Drop the context's memory of what its recent input looked like."""
        lib().ffq_ctx_forget(self.handle)

    def selftest(self):
        check(lib().ffq_selftest(self.handle))

    # ---- raw device memory (for hosts without torch) -------------------
    def dev_alloc(self, nbytes):
        p = ctypes.c_void_p()
        check(lib().ffq_dev_alloc(self.handle, int(nbytes), ctypes.byref(p)))
        return p.value

    def dev_free(self, ptr):
        check(lib().ffq_dev_free(self.handle, ctypes.c_void_p(ptr)))

    def h2d(self, dptr, arr):
        a = np.ascontiguousarray(arr)
        check(lib().ffq_copy_h2d(self.handle, ctypes.c_void_p(dptr), a.ctypes.data, a.nbytes, 0))

    def d2h(self, arr, dptr):
        assert arr.flags.c_contiguous
        check(lib().ffq_copy_d2h(self.handle, arr.ctypes.data, ctypes.c_void_p(dptr), arr.nbytes, 0))

    def load_fd(self, fd, pos, n_bytes, d_dst):
        """Bytes [pos, pos + n_bytes) of the file behind fd into device memory (ffq_load_fd); returns the bytes loaded
        (less than n_bytes: the file ended)."""
        n = ctypes.c_int64()
        check(lib().ffq_load_fd(self.handle, int(fd), int(pos), int(n_bytes), ctypes.c_void_p(d_dst), ctypes.byref(n)))
        return n.value

    def sync(self):
        check(lib().ffq_sync(self.handle))

    # ---- hot path --------------------------------------------------------
    def scan_device(self, d_buf, n_bytes, d_table, table_cap, sentinel=True, offset=0, eof=True,
                    add=None, flags=0, qual_add=-33, d_qual=None, qual_cap=0, d_qoff=None):
        """Record chain over a device-resident buffer (raw device pointers).

        Returns (rc, ScanResult); rc is OK or E_TABLE_FULL."""
        add = _add(add, sentinel)
        res = ScanResult()
        rc = lib().ffq_scan_device(self.handle, ctypes.c_void_p(d_buf), int(n_bytes), int(bool(sentinel)),
                                   int(offset), int(bool(eof)), int(add), int(flags), int(qual_add),
                                   ctypes.c_void_p(d_table), int(table_cap),
                                   ctypes.c_void_p(d_qual) if d_qual else None, int(qual_cap),
                                   ctypes.c_void_p(d_qoff) if d_qoff else None, ctypes.byref(res))
        check(rc, allow=(E_TABLE_FULL,))
        return rc, res

    def scan_submit(self, d_buf, n_bytes, d_table, table_cap, sentinel=True, offset=0, eof=True,
                    add=None, flags=0, qual_add=-33, d_qual=None, qual_cap=0, d_qoff=None):
        """Enqueue a scan and return at once; scan_wait() completes it."""
        add = _add(add, sentinel)
        check(lib().ffq_scan_submit(self.handle, ctypes.c_void_p(d_buf), int(n_bytes), int(bool(sentinel)),
                                    int(offset), int(bool(eof)), int(add), int(flags), int(qual_add),
                                    ctypes.c_void_p(d_table), int(table_cap),
                                    ctypes.c_void_p(d_qual) if d_qual else None, int(qual_cap),
                                    ctypes.c_void_p(d_qoff) if d_qoff else None))

    def scan_wait(self):
        res = ScanResult()
        rc = lib().ffq_scan_wait(self.handle, ctypes.byref(res))
        check(rc, allow=(E_TABLE_FULL,))
        return rc, res

    @staticmethod
    def _sized(run, n_bytes, table_cap):
        """run(cap) -> (rc, ScanResult, result) with a table of table_cap rows; table_cap None: a row per 64 bytes of input, and
        a table that was too small (E_TABLE_FULL) is sized from the records the scan counted and the scan run again."""
        cap = int(table_cap) if table_cap is not None else max(n_bytes // 64 + 16, 16)
        while True:
            rc, res, result = run(cap)
            if rc == E_TABLE_FULL and table_cap is None:
                cap = int(res.n_records) + 1
                continue
            return result

    def scan_host(self, buf, sentinel=True, offset=0, eof=True, add=None, flags=0, qual_add=-33,
                  table_cap=None, qual_room=None):
        """Record chain over a host bytes-like object.

        qual_room: with F_SINGLE_PASS, bytes of the quality buffer per 16 KiB tile of input (SEG_STRIDE; INPLACE_STRIDE
        admits the in-place layout, i.e. long lines, as well).
        Returns (table int64[n,6], ScanResult[, qual int8[], qoff int64[n+1]])."""
        a = np.frombuffer(buf, dtype=np.uint8) if not isinstance(buf, np.ndarray) else buf
        add = _add(add, sentinel)
        decode = bool(flags & F_DECODE_QUAL)

        def run(cap):
            table = np.empty((cap, 6), dtype=np.int64)
            nq = a.size if decode else 0
            if decode and (flags & F_SINGLE_PASS):
                nq = max(nq, ((a.size + 16383) >> 14) * int(qual_room or SEG_STRIDE))     # room for every tile's segment
            qual = np.empty(nq, dtype=np.int8)
            qoff = np.empty(cap + 1 if decode else 0, dtype=np.int64)
            res = ScanResult()
            rc = lib().ffq_scan_host(self.handle, a.ctypes.data if a.size else None, a.size,
                                     int(bool(sentinel)), int(offset), int(bool(eof)), int(add),
                                     int(flags), int(qual_add), table.ctypes.data, cap,
                                     qual.ctypes.data if decode else None, qual.size,
                                     qoff.ctypes.data if decode else None, ctypes.byref(res))
            check(rc, allow=(E_TABLE_FULL,))
            n = min(int(res.n_records), cap)
            return rc, res, (table[:n], res, qual[:int(res.n_qual_bytes)], qoff[:n + 1]) if decode else (table[:n], res)
        return self._sized(run, a.size, table_cap)

    def scan_fasta_host(self, buf, sentinel=False, offset=0, add=0, table_cap=None):
        """Every COMPLETE FASTA entry of a host buffer (the repeated entrypos_fasta call,
        reference fastqandfurious.py:103-143): (table int64[n,6] with pos4 = pos5 = -1,
        ScanResult with the last call's status / posbuffer / offset)."""
        a = np.frombuffer(buf, dtype=np.uint8) if not isinstance(buf, np.ndarray) else buf

        def run(cap):
            table = np.empty((cap, 6), dtype=np.int64)
            res = ScanResult()
            rc = lib().ffq_scan_fasta_host(self.handle, a.ctypes.data if a.size else None, a.size, int(bool(sentinel)),
                                           int(offset), int(add), table.ctypes.data, cap, ctypes.byref(res))
            check(rc, allow=(E_TABLE_FULL,))
            return rc, res, (table[:min(int(res.n_records), cap)], res)
        return self._sized(run, a.size, table_cap)

    def scan_fasta_device(self, d_buf, n_bytes, d_table, table_cap, sentinel=False, offset=0, add=0):
        res = ScanResult()
        rc = lib().ffq_scan_fasta_device(self.handle, ctypes.c_void_p(d_buf), int(n_bytes), int(bool(sentinel)),
                                         int(offset), int(add), ctypes.c_void_p(d_table), int(table_cap),
                                         ctypes.byref(res))
        check(rc, allow=(E_TABLE_FULL,))
        return rc, res

    def entrypos(self, buf, offset, pos):
        """One scanner call on the GPU: fills pos (6 x int64), returns status."""
        a = np.frombuffer(buf, dtype=np.uint8)
        st = ctypes.c_int(0)
        p = np.empty(6, dtype=np.int64)
        check(lib().ffq_entrypos(self.handle, a.ctypes.data if a.size else None, a.size, int(offset),
                                 p.ctypes.data, ctypes.byref(st)))
        for i in range(6):
            pos[i] = int(p[i])
        return st.value

    def arrayadd_b(self, arr, value):
        a = np.frombuffer(arr, dtype=np.int8) if not isinstance(arr, np.ndarray) else arr
        check(lib().ffq_arrayadd_b(self.handle, a.ctypes.data, a.size, int(value)))

    def arrayadd_q(self, arr, value):
        a = np.frombuffer(arr, dtype=np.int64) if not isinstance(arr, np.ndarray) else arr
        v = (int(value) + 2**63) % 2**64 - 2**63
        check(lib().ffq_arrayadd_q(self.handle, a.ctypes.data, a.size, v))

    def arrayadd_b_device(self, dptr, n, value):
        check(lib().ffq_arrayadd_b_device(self.handle, ctypes.c_void_p(dptr), int(n), int(value)))

    def arrayadd_q_device(self, dptr, n, value):
        v = (int(value) + 2**63) % 2**64 - 2**63
        check(lib().ffq_arrayadd_q_device(self.handle, ctypes.c_void_p(dptr), int(n), v))

    def table_lower_bound(self, d_table, n_rows, col, value):
        idx = ctypes.c_int64(0)
        check(lib().ffq_table_lower_bound(self.handle, ctypes.c_void_p(d_table), int(n_rows), int(col),
                                          int(value), ctypes.byref(idx)))
        return idx.value

    def table_cut(self, d_table, n_rows, lo, hi):
        """(i0, i1, pos0[i0], pos0[i1], pos5[i0 - 1], pos5[i1 - 1]): first rows with pos0 >= lo / >= hi,
        their pos0, and pos5 of the rows in front of them (-1: none)."""
        out = (ctypes.c_int64 * 6)()
        check(lib().ffq_table_cut(self.handle, ctypes.c_void_p(d_table), int(n_rows), int(lo), int(hi), out))
        return [int(x) for x in out]

    def table_select_seqlen(self, d_table, n_rows, min_len, max_len, d_out):
        """Rows with min_len <= pos3 - pos2 <= max_len of a device table, in order, into
        d_out (raw device pointers); returns the number kept."""
        k = ctypes.c_int64(0)
        check(lib().ffq_table_select_seqlen(self.handle, ctypes.c_void_p(d_table), int(n_rows), int(min_len),
                                            int(max_len), ctypes.c_void_p(d_out), ctypes.byref(k)))
        return k.value

    def table_select_seqlen_idx(self, d_table, n_rows, min_len, max_len, d_out, d_idx):
        """... and d_idx[i] = the ordinal in the table of kept row i (ffq_table_select_seqlen_idx)."""
        k = ctypes.c_int64(0)
        check(lib().ffq_table_select_seqlen_idx(self.handle, ctypes.c_void_p(d_table), int(n_rows), int(min_len), int(max_len),
                                                ctypes.c_void_p(d_out), ctypes.c_void_p(d_idx), ctypes.byref(k)))
        return k.value

    def table_select_reads(self, d_buf, n_bytes, d_table, n_rows, d_out, rules=None, min_len=None, max_len=None, d_idx=None,
                           sentinel=True, add=None):
        """Rows of a device table kept by their length and by what is in the read (ffq_table_select_reads; include/ffq.h
        states the rule), in order, into d_out, with d_idx[i] = the ordinal of kept row i (None: not wanted).  rules: a
        fastqandfurious.ContentRules, a ContentRulesStruct, or None (the length alone: d_buf may then be 0).  Raw device
        pointers; d_buf / n_bytes / sentinel / add as for table_gather_column.  Returns (rows kept, the eight counts: kept,
        dropped by rule 1..6, not judged by content)."""
        add = _add(add, sentinel)
        lo, hi = length_bounds(min_len, max_len)
        r = content_rules_struct(rules)
        k = ctypes.c_int64(0)
        counts = (ctypes.c_int64 * FILTER_COUNTS)()
        check(lib().ffq_table_select_reads(self.handle, ctypes.c_void_p(d_buf) if d_buf else None, int(n_bytes), int(bool(sentinel)),
                                           int(add), ctypes.c_void_p(d_table), int(n_rows), lo, hi,
                                           None if r is None else ctypes.byref(r), ctypes.c_void_p(d_out),
                                           ctypes.c_void_p(d_idx) if d_idx else None, ctypes.byref(k), counts))
        return k.value, [int(x) for x in counts]

    def table_select_pairs(self, mate1, mate2, n_pairs, d_out1, d_out2, rules1=None, rules2=None, min_len=None, max_len=None,
                           pair_filter="any", d_idx=None):
        """Pairs of rows of two device tables kept or dropped together (ffq_table_select_pairs; include/ffq.h states the
        rule).  mate1 / mate2: TableViews (table_view()); rules1 / rules2 as `rules` of table_select_reads; min_len / max_len:
        an int (or None) for both mates or a (mate 1, mate 2) pair; pair_filter: "any", "both" or "first".  Kept pairs go to
        d_out1 / d_out2, their ordinals to d_idx (None: not wanted).  Returns (pairs kept, hist1, hist2, pairs): the eight
        counts of either mate judged alone, and [kept, dropped, only mate 1 failed, only mate 2 failed, both failed]."""
        def per_mate(x):
            return tuple(x) if isinstance(x, (tuple, list)) else (x, x)
        (lo1, lo2), (hi1, hi2) = per_mate(min_len), per_mate(max_len)
        bounds = (ctypes.c_int64 * 4)(*(length_bounds(lo1, hi1) + length_bounds(lo2, hi2)))
        r1, r2 = content_rules_struct(rules1), content_rules_struct(rules2)
        k = ctypes.c_int64(0)
        h1, h2 = (ctypes.c_int64 * FILTER_COUNTS)(), (ctypes.c_int64 * FILTER_COUNTS)()
        pairs = (ctypes.c_int64 * PAIR_COUNTS)()
        check(lib().ffq_table_select_pairs(self.handle, ctypes.byref(mate1), ctypes.byref(mate2), int(n_pairs), bounds,
                                           None if r1 is None else ctypes.byref(r1), None if r2 is None else ctypes.byref(r2),
                                           _pair_filter(pair_filter), ctypes.c_void_p(d_out1), ctypes.c_void_p(d_out2),
                                           ctypes.c_void_p(d_idx) if d_idx else None, ctypes.byref(k), h1, h2, pairs))
        return k.value, [int(x) for x in h1], [int(x) for x in h2], [int(x) for x in pairs]

    def table_pair_names(self, mate1, mate2, n_pairs):
        """Are rows i of the two tables mates by their names (ffq_table_pair_names; include/ffq.h states the rule,
        fastqandfurious.pair_id is its host statement)?  Returns (equal, different, not compared, ordinal of the first
        different pair or -1)."""
        out = (ctypes.c_int64 * 4)()
        check(lib().ffq_table_pair_names(self.handle, ctypes.byref(mate1), ctypes.byref(mate2), int(n_pairs), out))
        return tuple(int(x) for x in out)

    def table_pair_overlap(self, mate1, mate2, n_pairs, rules, d_out1, d_out2, d_insert=None, d_hist=None, accumulate=False,
                           trim=True):
        """The overlap of the mates of every pair of two device tables (ffq_table_pair_overlap; include/ffq.h states the rule,
        fastqandfurious.pair_overlap is its host statement): insert sizes, and with `trim` both rows cut to the fragment
        where it is shorter than the reads.  mate1 / mate2: TableViews; rules: an OverlapRulesStruct, or anything with
        min_overlap, max_diff and diff_permille (then `trim` says whether rows are cut).  d_out1 / d_out2 may be the tables
        themselves.  d_insert: int32 per pair (None: not wanted); d_hist: OVERLAP_HIST_WORDS uint64, overwritten or -- accumulate
        -- added to (None: not wanted).  Returns the six counts: [pairs analysed, with an overlap, changed, bases removed from
        mate 1, from mate 2, pairs not analysed]."""
        r = overlap_rules_struct(rules, trim)
        counts = (ctypes.c_int64 * OVERLAP_COUNTS)()
        check(lib().ffq_table_pair_overlap(self.handle, ctypes.byref(mate1), ctypes.byref(mate2), int(n_pairs),
                                           None if r is None else ctypes.byref(r), ctypes.c_void_p(d_out1), ctypes.c_void_p(d_out2),
                                           ctypes.c_void_p(d_insert) if d_insert else None, ctypes.c_void_p(d_hist) if d_hist else None,
                                           1 if accumulate else 0, counts))
        return [int(x) for x in counts]

    def table_pair_merge(self, mate1, mate2, n_pairs, d_insert, d_text, text_cap, d_rest1, d_rest2, d_ord=None, d_off=None,
                         d_rest_ord=None):
        """The mates of every pair of two device tables merged into one read where their insert size allows it, rendered as
        FASTQ text (ffq_table_pair_merge; include/ffq.h states the rule, fastqandfurious.merge_mates is its host statement).
        mate1 / mate2: TableViews; d_insert: int32 insert sizes (table_pair_overlap's), pair k's at d_insert[d_ord[k]] (d_ord
        None: at d_insert[k]); d_text: text_cap bytes; d_off: n_pairs + 1 offsets or None; d_rest1 / d_rest2: n_pairs rows of
        room each for the pairs that are not merged, not the input tables; d_rest_ord: their ordinals or None.  Raw device
        pointers.  Returns (rc, pairs not merged, counts): rc is OK or E_TABLE_FULL (text_cap too small: counts[2] is the need,
        d_text is not touched); counts = [pairs merged, not merged, bytes of text, bases of the merged reads, positions inside
        overlaps, of those taken from mate 2]."""
        n_rest = ctypes.c_int64(0)
        counts = (ctypes.c_int64 * MERGE_COUNTS)()
        rc = lib().ffq_table_pair_merge(self.handle, ctypes.byref(mate1), ctypes.byref(mate2), int(n_pairs),
                                        ctypes.c_void_p(d_insert) if d_insert else None, ctypes.c_void_p(d_ord) if d_ord else None,
                                        ctypes.c_void_p(d_text) if d_text else None, int(text_cap),
                                        ctypes.c_void_p(d_off) if d_off else None, ctypes.c_void_p(d_rest1) if d_rest1 else None,
                                        ctypes.c_void_p(d_rest2) if d_rest2 else None,
                                        ctypes.c_void_p(d_rest_ord) if d_rest_ord else None, ctypes.byref(n_rest), counts)
        check(rc, allow=(E_TABLE_FULL,))
        return rc, n_rest.value, [int(x) for x in counts]

    def table_pair_correct(self, mate1, mate2, n_pairs, d_insert, rules, qual_base=33, matrix=True):
        """Mismatched bases inside the overlap of the mates of every pair of two device tables corrected IN THE BUFFERS
        (ffq_table_pair_correct; include/ffq.h states the rule, fastqandfurious.correct_mates is its host statement).  mate1 /
        mate2: TableViews whose d_buf is written through; the rows of different pairs must not share bytes.  d_insert: int32
        insert sizes (table_pair_overlap's), a raw device pointer; rules: a CorrectRulesStruct, or anything with good_quality
        and bad_quality (then `qual_base` beside it).  Returns (counts, matrix): counts = [pairs looked at, with a correction,
        bases corrected in mate 1, in mate 2, mismatch positions, pairs not looked at]; matrix int64[5][4] by (class before,
        class after), None without `matrix`."""
        r = correct_rules_struct(rules, qual_base)
        counts = (ctypes.c_int64 * CORRECT_COUNTS)()
        mat = (ctypes.c_int64 * CORRECT_MATRIX_WORDS)() if matrix else None
        check(lib().ffq_table_pair_correct(self.handle, ctypes.byref(mate1), ctypes.byref(mate2), int(n_pairs),
                                           ctypes.c_void_p(d_insert) if d_insert else None, None if r is None else ctypes.byref(r),
                                           counts, mat))
        return [int(x) for x in counts], (np.array(mat, dtype=np.int64).reshape(5, 4) if matrix else None)

    def table_seq_keys(self, d_buf, n_bytes, d_table, n_rows, d_keys, sentinel=True, add=None):
        """The 64-bit sequence key of every row of a device table (ffq_table_seq_keys; include/ffq.h states the rule,
        fastqandfurious.seq_key is its host statement) into d_keys (uint64 per row; KEY_NONE for a row the rule does not
        apply to).  Raw device pointers; d_buf / n_bytes / sentinel / add as for table_gather_column.  Returns (rows keyed,
        rows not keyed)."""
        add = _add(add, sentinel)
        counts = (ctypes.c_int64 * 2)()
        check(lib().ffq_table_seq_keys(self.handle, ctypes.c_void_p(d_buf) if d_buf else None, int(n_bytes), int(bool(sentinel)),
                                       int(add), ctypes.c_void_p(d_table) if d_table else None, int(n_rows),
                                       ctypes.c_void_p(d_keys) if d_keys else None, counts))
        return int(counts[0]), int(counts[1])

    COLUMNS = {"header": (0, 1, 1), "sequence": (2, 0, 3), "quality": (4, 0, 5)}

    def table_gather_column(self, d_buf, n_bytes, d_table, n_rows, which, d_out, out_cap, d_off, sentinel=True,
                            add=None, value_add=0):
        """Packed component `which` ("header" = buf[pos0 + 1:pos1], "sequence", "quality", or a
        (begin column, shift, end column) triple) of every row of a device table, + value_add per
        byte, into d_out with CSR offsets d_off (n_rows + 1); raw device pointers.  Returns
        (rc, bytes of the stream); rc is OK or E_TABLE_FULL (out_cap too small)."""
        ca, sh, cb = self.COLUMNS[which] if isinstance(which, str) else which
        add = _add(add, sentinel)
        nb = ctypes.c_int64(0)
        rc = lib().ffq_table_gather_column(self.handle, ctypes.c_void_p(d_buf), int(n_bytes), int(bool(sentinel)),
                                           int(add), ctypes.c_void_p(d_table), int(n_rows), int(ca), int(sh), int(cb),
                                           int(value_add), ctypes.c_void_p(d_out) if d_out else None, int(out_cap),
                                           ctypes.c_void_p(d_off), ctypes.byref(nb))
        check(rc, allow=(E_TABLE_FULL,))
        return rc, nb.value

    def table_trim_quality(self, d_buf, n_bytes, d_table, n_rows, cutoff_back, cutoff_front=0, qual_base=33, d_out=None,
                           sentinel=True, add=None):
        """Quality-trim the rows of a device table (ffq_table_trim_quality: the running-sum rule of BWA / cutadapt -q,
        either end with its own cutoff): pos2..pos5 of every eligible row move inwards, every other row is copied
        unchanged.  d_out: n_rows rows of room (None: in place); raw device pointers; d_buf / n_bytes / sentinel / add as
        for table_gather_column.  Returns (rows changed, bases removed, rows skipped)."""
        add = _add(add, sentinel)
        stats = (ctypes.c_int64 * 3)()
        check(lib().ffq_table_trim_quality(self.handle, ctypes.c_void_p(d_buf), int(n_bytes), int(bool(sentinel)), int(add),
                                           ctypes.c_void_p(d_table), int(n_rows), int(qual_base), int(cutoff_front),
                                           int(cutoff_back), ctypes.c_void_p(d_table if d_out is None else d_out), stats))
        return int(stats[0]), int(stats[1]), int(stats[2])

    def table_trim_adapter(self, d_buf, n_bytes, d_table, n_rows, adapter, err_permille=100, min_overlap=3, d_out=None,
                           sentinel=True, add=None):
        """Cut the rows of a device table at a 3' adapter (ffq_table_trim_adapter: the leftmost position at which `adapter`
        -- bytes, 1..64 of them, 'N' a wildcard -- or a prefix of it that runs into the read's end matches with at most
        overlap * err_permille // 1000 mismatches; no indels): pos3 and pos5 of every eligible row move inwards, every other
        row is copied unchanged.  d_out: n_rows rows of room (None: in place); raw device pointers; d_buf / n_bytes /
        sentinel / add as for table_gather_column.  Returns (rows changed, bases removed, rows skipped)."""
        add = _add(add, sentinel)
        adapter = bytes(adapter)
        stats = (ctypes.c_int64 * 3)()
        check(lib().ffq_table_trim_adapter(self.handle, ctypes.c_void_p(d_buf), int(n_bytes), int(bool(sentinel)), int(add),
                                           ctypes.c_void_p(d_table), int(n_rows), adapter, len(adapter), int(err_permille),
                                           int(min_overlap), ctypes.c_void_p(d_table if d_out is None else d_out), stats))
        return int(stats[0]), int(stats[1]), int(stats[2])

    def table_trim_poly(self, d_buf, n_bytes, d_table, n_rows, base=b"G", min_len=10, d_out=None, sentinel=True, add=None):
        """Cut poly tails off the rows of a device table (ffq_table_trim_poly: the walk from the 3' end that include/ffq.h
        states; base: b"A", b"C", b"G" or b"T" -- poly-G is b"G" --, None for any of the four (poly-X), or the C ABI's own 0..3
        / POLY_ANY): pos3 and pos5 of every eligible row move inwards, every other row is copied unchanged.  d_out: n_rows rows
        of room (None: in place); raw device pointers; d_buf / n_bytes / sentinel / add as for table_gather_column.  Returns
        (rows changed, bases removed, rows skipped)."""
        add = _add(add, sentinel)
        base = POLY_BASES.get(base, base)
        stats = (ctypes.c_int64 * 3)()
        check(lib().ffq_table_trim_poly(self.handle, ctypes.c_void_p(d_buf), int(n_bytes), int(bool(sentinel)), int(add),
                                        ctypes.c_void_p(d_table), int(n_rows), int(base), int(min_len),
                                        ctypes.c_void_p(d_table if d_out is None else d_out), stats))
        return int(stats[0]), int(stats[1]), int(stats[2])

    def table_trim_ends(self, d_buf, n_bytes, d_table, n_rows, rules, qual_base=33, d_out=None, sentinel=True, add=None):
        """Fixed trims and sliding-window quality cutting of the rows of a device table (ffq_table_trim_ends: the rule that
        include/ffq.h states; rules: a fastqandfurious.EndRules with `qual_base` beside it, or an EndsRulesStruct): pos2..pos5
        of every eligible row move inwards, every other row is copied unchanged.  Run it in front of the other trims.  d_out:
        n_rows rows of room (None: in place); raw device pointers; d_buf / n_bytes / sentinel / add as for
        table_gather_column.  Returns (rows changed, bases removed, rows skipped)."""
        add = _add(add, sentinel)
        r = ends_rules_struct(rules, qual_base)
        stats = (ctypes.c_int64 * 3)()
        check(lib().ffq_table_trim_ends(self.handle, ctypes.c_void_p(d_buf), int(n_bytes), int(bool(sentinel)), int(add),
                                        ctypes.c_void_p(d_table), int(n_rows), ctypes.byref(r) if r is not None else None,
                                        ctypes.c_void_p(d_table if d_out is None else d_out), stats))
        return int(stats[0]), int(stats[1]), int(stats[2])

    def table_stats(self, d_buf, n_bytes, d_table, n_rows, d_stats, qual_base=33, max_cycles=512, accumulate=False, sentinel=True,
                    add=None, wait=True):
        """Per-cycle base and quality statistics of the rows of a device table (ffq_table_stats), counted into the
        stats_words(max_cycles) uint64 words at d_stats (device memory, 16-byte aligned; include/ffq.h has the layout):
        overwritten, or added to with accumulate.  Raw device pointers; d_buf / n_bytes / sentinel / add as for
        table_gather_column.  Returns the eight head words (rows counted, rows skipped, bases, ...) as they stand after the
        call -- one host wait --, or None with wait=False: the call is only enqueued on the context's stream."""
        add = _add(add, sentinel)
        head = (ctypes.c_int64 * STATS_HEAD)() if wait else None
        check(lib().ffq_table_stats(self.handle, ctypes.c_void_p(d_buf), int(n_bytes), int(bool(sentinel)), int(add),
                                    ctypes.c_void_p(d_table), int(n_rows), int(qual_base), int(max_cycles), int(bool(accumulate)),
                                    ctypes.c_void_p(d_stats), head))
        return [int(x) for x in head] if wait else None

    def table_render_fastq(self, d_buf, n_bytes, d_table, n_rows, d_out, out_cap, d_off=None, sentinel=True, add=None):
        """FASTQ text of the rows of a device table (ffq_table_render_fastq): row p renders as "@" + buf[p0 + 1:p1] + "\\n"
        + buf[p2:p3] + "\\n+\\n" + buf[p4:p5] + "\\n", a row that is not renderable as nothing.  d_out: out_cap bytes, any
        alignment; d_off: n_rows + 1 offsets or None; raw device pointers; d_buf / n_bytes / sentinel / add as for
        table_gather_column.  Returns (rc, (bytes rendered, rows rendered, rows skipped)); rc is OK or E_TABLE_FULL
        (out_cap too small: stats[0] is the need, d_out is not touched)."""
        add = _add(add, sentinel)
        stats = (ctypes.c_int64 * 3)()
        rc = lib().ffq_table_render_fastq(self.handle, ctypes.c_void_p(d_buf), int(n_bytes), int(bool(sentinel)), int(add),
                                          ctypes.c_void_p(d_table), int(n_rows), ctypes.c_void_p(d_out) if d_out else None,
                                          int(out_cap), ctypes.c_void_p(d_off) if d_off else None, stats)
        check(rc, allow=(E_TABLE_FULL,))
        return rc, (int(stats[0]), int(stats[1]), int(stats[2]))

    def table_take_umi(self, d_buf, n_bytes, d_table, n_rows, umi_len, umi_skip=0, d_out=None, sentinel=True, add=None):
        """Take the UMI off the rows of a device table (ffq_table_take_umi; include/ffq.h states the rule): pos2 and pos4 of
        every eligible row of at least umi_len bases move inwards by min(umi_len + umi_skip, length), every other row is copied
        unchanged.  pos1 stays, so the tag is found again at buf[pos1 + 1:pos1 + 1 + umi_len] (table_render_fastq_umi).  d_out:
        n_rows rows of room (None: in place); raw device pointers; d_buf / n_bytes / sentinel / add as for
        table_gather_column.  Returns (rows changed, bases removed, rows skipped)."""
        add = _add(add, sentinel)
        stats = (ctypes.c_int64 * 3)()
        check(lib().ffq_table_take_umi(self.handle, ctypes.c_void_p(d_buf), int(n_bytes), int(bool(sentinel)), int(add),
                                       ctypes.c_void_p(d_table), int(n_rows), int(umi_len), int(umi_skip),
                                       ctypes.c_void_p(d_table if d_out is None else d_out), stats))
        return int(stats[0]), int(stats[1]), int(stats[2])

    def table_render_fastq_umi(self, rows, n_rows, rules, d_out, out_cap, d_off=None, src1=None, src2=None):
        """FASTQ text of the rows of a device table with the UMI in the names (ffq_table_render_fastq_umi; include/ffq.h
        states the rule).  rows: a TableView (table_view()); src1 / src2: the TableViews whose row i may carry the tag of read 1
        / read 2 -- `rows` itself, or a table over another buffer; rules: a fastqandfurious.UmiRules or a UmiRulesStruct.  A
        row whose sources do not all carry a tag renders as table_render_fastq renders it.  Returns (rc, (bytes rendered, rows
        rendered, rows skipped, rows tagged)); rc is OK or E_TABLE_FULL (out_cap too small: stats[0] is the need, d_out is
        not touched)."""
        r = umi_rules_struct(rules)
        stats = (ctypes.c_int64 * 4)()
        rc = lib().ffq_table_render_fastq_umi(self.handle, ctypes.byref(rows), int(n_rows),
                                              ctypes.byref(src1) if src1 is not None else None,
                                              ctypes.byref(src2) if src2 is not None else None,
                                              ctypes.byref(r) if r is not None else None, ctypes.c_void_p(d_out) if d_out else None,
                                              int(out_cap), ctypes.c_void_p(d_off) if d_off else None, stats)
        check(rc, allow=(E_TABLE_FULL,))
        return rc, tuple(int(x) for x in stats)

    def deflate_bgzf(self, d_src, n_bytes, d_out, out_cap, d_member_off=None):
        """n_bytes of device memory written as BGZF members, deflated on the device (ffq_deflate_bgzf; include/ffq.h has the
        container, the bound and the match rule): a member per BGZF_BLOCK_BYTES, back to back in d_out, the same bytes for
        the same input on every call.  d_out: out_cap bytes -- deflate_bgzf_bound(n_bytes) always suffices --, any alignment;
        d_member_off: members + 1 offsets or None; raw device pointers.  The empty member that ends a BGZF file is not
        written (bgzf_eof_block()).  Returns (rc, (bytes in, bytes out, members, members stored)); rc is OK or E_TABLE_FULL
        (out_cap too small: stats[1] is the need, d_out is not touched)."""
        stats = (ctypes.c_int64 * DEFLATE_COUNTS)()
        rc = lib().ffq_deflate_bgzf(self.handle, ctypes.c_void_p(d_src) if d_src else None, int(n_bytes),
                                    ctypes.c_void_p(d_out) if d_out else None, int(out_cap),
                                    ctypes.c_void_p(d_member_off) if d_member_off else None, stats)
        check(rc, allow=(E_TABLE_FULL,))
        return rc, tuple(int(x) for x in stats)

    def synth_single(self, dptr, first, count, seed=42):
        check(lib().ffq_synth_single(self.handle, ctypes.c_void_p(dptr), int(first), int(count), int(seed)))

    def synth_wrapped(self, dptr, d_start, first, count, seed=43):
        check(lib().ffq_synth_wrapped(self.handle, ctypes.c_void_p(dptr), ctypes.c_void_p(d_start),
                                      int(first), int(count), int(seed)))


def deflate_bgzf_bound(n_bytes):
    """ffq_deflate_bgzf_bound: bytes that hold the BGZF members of n_bytes whatever they are, n + 31 per block."""
    return int(lib().ffq_deflate_bgzf_bound(int(n_bytes)))


def bgzf_eof_block():
    """ffq_bgzf_eof_block: the 28 bytes of the empty member that ends a BGZF file."""
    out = (ctypes.c_uint8 * 28)()
    lib().ffq_bgzf_eof_block(out)
    return bytes(out)


def seq_key_host(sequence):
    """ffq_seq_key_host: the key rule by the library's own host code (fastqandfurious.seq_key is the same in Python)."""
    b = bytes(sequence)
    return int(lib().ffq_seq_key_host(b, len(b)))


def pair_key_host(k1, k2):
    """ffq_pair_key_host"""
    return int(lib().ffq_pair_key_host(int(k1), int(k2)))


class Dedup:
    """A device-resident set of sequence keys that outlives the calls on it (ffq_dedup; include/ffq.h states the rule): the
    first copy of a key, in the order rows are submitted, is kept.  expected_keys: keys the table takes without growing (0:
    the minimum); max_bytes: cap of the table (0: none; a call that would grow beyond it raises FFQError E_NOMEM and leaves
    the set usable)."""

    def __init__(self, ctx, expected_keys=0, max_bytes=0):
        self._h = ctypes.c_void_p()
        self._ctx = ctx
        check(lib().ffq_dedup_create(ctx.handle, int(expected_keys), int(max_bytes), ctypes.byref(self._h)))

    def select(self, d_keys1, n, d_keys2=None, d_ord=None, d_table1=None, d_table2=None, d_out1=None, d_out2=None, d_idx=None,
               drop=True):
        """Rows 0..n of a call entered and judged (ffq_dedup_select): row i has the key d_keys1[j] -- with d_keys2 the pair key
        of d_keys1[j], d_keys2[j] --, j = d_ord[i] (None: i); the kept rows of d_table1 / d_table2 (None: nothing is copied)
        go to d_out1 / d_out2, their j to d_idx (None: not wanted).  drop False: count only, every row is kept.  Raw device
        pointers.  Returns (rows kept, counts): [kept, duplicates, rows without a key, distinct keys in the set, slots,
        rehashes so far]."""
        def ptr(x):
            return ctypes.c_void_p(x) if x else None
        k = ctypes.c_int64(0)
        counts = (ctypes.c_int64 * DEDUP_COUNTS)()
        check(lib().ffq_dedup_select(self._h, ptr(d_keys1), ptr(d_keys2), ptr(d_ord), int(n), ptr(d_table1), ptr(d_table2),
                                     ptr(d_out1), ptr(d_out2), ptr(d_idx), ctypes.byref(k), 1 if drop else 0, counts))
        return k.value, [int(x) for x in counts]

    def close(self):
        if self._h:
            lib().ffq_dedup_destroy(self._h)
            self._h = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def shard_unique_id():
    """128 bytes of communicator id (ncclGetUniqueId): rank 0 draws it, every rank gets it from rank 0."""
    buf = (ctypes.c_uint8 * 128)()
    check(lib().ffq_shard_unique_id(buf))
    return bytes(buf)


def _host_ops(world, exchange, allgather, scan=None):
    """(ShardHostOps, errors): the ctypes adapters of a host transport -- exchange(pieces), allgather(words) and, optionally,
    scan(...) as shard_host_step documents them.  An exception raised inside one must not propagate through the C frames: it
    is appended to `errors` (the caller re-raises it once the library has returned) and the library is told E_INTERNAL.  The
    structure holds the callbacks: they live as long as it does."""
    err = []

    def guard(fn):
        def run(*a):
            try:
                return int(fn(*a) or 0)
            except BaseException as e:      # noqa: BLE001
                err.append(e)
                return E_INTERNAL
        return run

    def c_exchange(_user, pieces, n):
        exchange([(pieces[i].src, pieces[i].dst, pieces[i].a, pieces[i].b, pieces[i].ptr) for i in range(n)])

    def c_gather(_user, mine, out):
        allv = allgather([mine[i] for i in range(8)])
        for r in range(world):
            for k in range(8):
                out[r * 8 + k] = int(allv[r][k])

    def c_scan(_user, buf, n, sentinel, offset, eof, add, table, cap, res):
        return scan(buf, n, sentinel, offset, eof, add, table, cap, res.contents)

    return ShardHostOps(None, _SCAN_CB(guard(c_scan)) if scan is not None else _SCAN_CB(), _EXCHANGE_CB(guard(c_exchange)),
                        _GATHER_CB(guard(c_gather))), err


def shard_host_step(rank, world, bounds, tail_bytes, head_bytes, ext_ptr, table_ptr, table_cap, exchange, allgather, scan=None, ctx=None):
    """One step of the byte-range shards over HOST memory (ffq_shard_host_step): the protocol is the library's
    (csrc/ffq_shard_proto.h), the transport the caller's --
        exchange(pieces)   pieces = [(src, dst, a, b, ptr)]: the same list on every rank; ptr is this rank's end (or None)
        allgather(words)   eight ints in, [world][8] out
        scan(buf_ptr, n, sentinel, offset, eof, add, table_ptr, cap, res) -> FFQ code, res (a ScanResult) filled;
                           None: ffq_scan_host on `ctx` (the GPU)
    An exception raised inside a callback is re-raised here.  Returns (rc, ShardResult); rc is OK or E_TABLE_FULL."""
    ops, err = _host_ops(world, exchange, allgather, scan)
    b = (ctypes.c_int64 * (world + 1))(*[int(x) for x in bounds])
    res = ShardResult()
    rc = lib().ffq_shard_host_step(ctypes.byref(ops), ctx.handle if ctx is not None else None, int(rank), int(world), b,
                                   int(tail_bytes), int(head_bytes), ctypes.c_void_p(ext_ptr), ctypes.c_void_p(table_ptr),
                                   int(table_cap), ctypes.byref(res))
    if err:
        raise err[0]
    check(rc, allow=(E_TABLE_FULL,))
    return rc, res


class ShardWorld:
    """k logical ranks as threads of one process (ffq_shard_world_*): the in-process transport of the native step."""

    def __init__(self, world):
        self.world = int(world)
        self._h = ctypes.c_void_p()
        check(lib().ffq_shard_world_create(self.world, ctypes.byref(self._h)))

    def abort(self):
        if self._h:
            lib().ffq_shard_world_abort(self._h)

    def close(self):
        if self._h:
            lib().ffq_shard_world_destroy(self._h)
            self._h = ctypes.c_void_p()


class Shard:
    """One rank's byte-range shard of a stream, the whole step behind the C ABI (ffq_shard_*, include/ffq.h): halo
    hand-off over RCCL (or the in-process transport), scan, cut, one gather of the hand-off words."""

    def __init__(self, ctx, bounds, rank, world, tail_bytes, head_bytes, unique_id=None, local_world=None, parent=None, hosted=None,
                 serial=None):
        """serial: True -- the serial step (ONE communicator, ONE stream) from the start; None: as FFQ_SHARD_SERIAL says.
        unique_id: RCCL between processes; local_world: a ShardWorld (threads of this process); hosted: a transport object
        with exchange(pieces) / allgather(words) as shard_host_step takes them -- the device step over the caller's own
        transport (ffq_shard_create_hosted: several processes on one GPU, a group over gloo)."""
        self._ctx = ctx
        self._h = ctypes.c_void_p()
        self._keep = (local_world, parent)
        self._err = []
        b = (ctypes.c_int64 * (world + 1))(*[int(x) for x in bounds])
        if hosted is not None:
            ops, self._err = _host_ops(world, hosted.exchange, hosted.allgather)
            self._keep = (ops, hosted)                     # (the callbacks live as long as the shard)
            check(lib().ffq_shard_create_hosted(ctx.handle, ctypes.byref(ops), int(rank), int(world), b, int(tail_bytes), int(head_bytes),
                                                ctypes.byref(self._h)))
        elif parent is not None:
            check(lib().ffq_shard_create_lane(parent._h, ctx.handle, ctypes.byref(self._h)))
        elif local_world is not None:
            check(lib().ffq_shard_create_local(ctx.handle, local_world._h, int(rank), b, int(tail_bytes), int(head_bytes),
                                               ctypes.byref(self._h)))
        else:
            idb = (ctypes.c_uint8 * 128).from_buffer_copy(unique_id)
            if serial is None:
                check(lib().ffq_shard_create(ctx.handle, idb, int(rank), int(world), b, int(tail_bytes), int(head_bytes),
                                             ctypes.byref(self._h)))
            else:
                check(lib().ffq_shard_create2(ctx.handle, idb, int(rank), int(world), b, int(tail_bytes), int(head_bytes),
                                              1 if serial else 0, ctypes.byref(self._h)))
                serial = None
        if serial is not None and parent is None:
            check(lib().ffq_shard_set_serial(self._h, 1 if serial else 0))
        import weakref
        ctx._children.append(weakref.ref(self))      # (a shard lives on its context: closed with it, before it)

    def lane(self, ctx):
        """A second shard of the same rank on another context (same scan stream): steps queued one ahead."""
        return Shard(ctx, [], 0, 0, 0, 0, parent=self)

    def halo(self):
        t, h = ctypes.c_int64(), ctypes.c_int64()
        check(lib().ffq_shard_halo(self._h, ctypes.byref(t), ctypes.byref(h)))
        return t.value, h.value

    def transport(self):
        return lib().ffq_shard_transport(self._h).decode()

    def info(self):
        """Who is there and how the steps run (ffq_shard_get_info): dict with nranks_handoff / nranks_gather
        (ncclCommCount), bus_ids (every rank's GPU as "dddd:bb:dd.f", None: unknown), serial, timeout_s, last_stage
        (where the last watchdog trip found the step), poisoned."""
        i = ShardInfo()
        check(lib().ffq_shard_get_info(self._h, ctypes.byref(i)))

        def bdf(v):
            return None if v < 0 else "%04x:%02x:%02x.%d" % (v >> 16, (v >> 8) & 0xFF, (v >> 3) & 0x1F, v & 7)
        return {"rank": i.rank, "world": i.world, "nranks_handoff": i.nranks_handoff, "nranks_gather": i.nranks_gather,
                "serial": bool(i.serial), "mode": "serial" if i.serial else "pipelined", "timeout_s": float(i.timeout_s),
                "last_stage": STAGE_NAMES[i.last_stage], "poisoned": bool(i.poisoned),
                "bus_ids": [bdf(int(i.bus_id[r])) for r in range(i.n_bus)]}

    def set_timeout(self, seconds):
        """The step watchdog's deadline (0: none; default FFQ_SHARD_TIMEOUT_S or 30 s): every lane of the rank."""
        check(lib().ffq_shard_set_timeout(self._h, float(seconds)))

    def set_serial(self, on=True):
        """Between steps (no lane pending), every rank alike: the serial step -- ONE communicator, ONE stream."""
        check(lib().ffq_shard_set_serial(self._h, 1 if on else 0))

    def abort(self):
        """After E_TIMEOUT: ncclCommAbort on the communicators, the streams drained.  True: drained; only close() is left."""
        return lib().ffq_shard_abort(self._h) == OK

    def inject_stall(self, stage, seconds):
        """diagnostics: the next step hangs at STAGE_* for up to `seconds` (released by abort / close)."""
        check(lib().ffq_shard_inject_stall(self._h, int(stage), float(seconds)))

    def self_exchange(self, d_src, d_dst, n):
        check(lib().ffq_shard_self_exchange(self._h, ctypes.c_void_p(d_src), ctypes.c_void_p(d_dst), int(n)))

    def exchange_halo(self, d_ext, overlap=False):
        check(lib().ffq_shard_exchange_halo(self._h, ctypes.c_void_p(d_ext), 1 if overlap else 0))

    def load_fd(self, fd, d_ext):
        """This rank's bytes [lo - tail, hi + head) of the file behind fd (bounds are file offsets) into d_ext; steps over
        that buffer then hand off nothing (ffq_shard_load_fd).  Returns the bytes loaded.  fd < 0: detach."""
        n = ctypes.c_int64()
        check(lib().ffq_shard_load_fd(self._h, int(fd), ctypes.c_void_p(d_ext), ctypes.byref(n)))
        return n.value

    def scan_fd_slabs(self, fd, slab_bytes, d_table, table_cap, flags=0):
        """This rank's range of the file behind fd through ONE device buffer of slab_bytes, slab after slab
        (ffq_shard_scan_fd_slabs: a range that does not fit the GPU); collective like a step.  (rc, ShardResult)."""
        res = ShardResult()
        rc = lib().ffq_shard_scan_fd_slabs(self._h, int(fd), int(slab_bytes), int(flags), ctypes.c_void_p(d_table), int(table_cap), ctypes.byref(res))
        if self._err:
            raise self._err.pop(0)
        check(rc, allow=(E_TABLE_FULL,))
        return rc, res

    def step_submit(self, d_ext, d_table, table_cap, flags=0, qual_add=-33, d_qual=None, qual_cap=0, d_qoff=None, overlap=False):
        rc = lib().ffq_shard_step_submit(self._h, ctypes.c_void_p(d_ext), 1 if overlap else 0, int(flags), int(qual_add),
                                         ctypes.c_void_p(d_table), int(table_cap), ctypes.c_void_p(d_qual), int(qual_cap),
                                         ctypes.c_void_p(d_qoff))
        if self._err:                                   # (an exception inside a hosted transport's callback: the hand-off)
            raise self._err.pop(0)
        check(rc)

    def step_wait(self):
        res = ShardResult()
        rc = lib().ffq_shard_step_wait(self._h, ctypes.byref(res))
        if self._err:                                   # (an exception inside a hosted transport's callback)
            raise self._err.pop(0)
        check(rc, allow=(E_TABLE_FULL,))
        return rc, res

    def close(self):
        if self._h:
            lib().ffq_shard_destroy(self._h)
            self._h = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def _compress_mode(mode):
    if mode not in COMPRESS_MODES:
        raise ValueError("compress: %r is not one of %s" % (mode, sorted(COMPRESS_MODES, key=str)))
    return COMPRESS_MODES[mode]


def _counts(call, handle, n, *more):
    """What a getter of the library counts: call(handle, n int64 it fills, *more), checked, as a list of ints."""
    counts = (ctypes.c_int64 * n)()
    check(call(handle, counts, *more))
    return [int(x) for x in counts]


def _pinned_view(ptr, n, ctype, shape=None):
    """numpy view of the n `ctype` elements at address `ptr` -- memory the library owns: valid as long as that says --, as
    `shape` if given; n 0: an empty array of the same type.  Elements without an address are the library's error."""
    if n and not ptr:
        raise FFQError(E_INTERNAL, "the library handed out %d elements and no address" % n)
    a = np.ctypeslib.as_array((ctype * n).from_address(ptr)) if n else np.zeros(0, dtype=ctype)
    return a if shape is None else a.reshape(shape)


def _members_of(call, handle):
    bp, nb = ctypes.c_void_p(), ctypes.c_int64()
    stats = (ctypes.c_int64 * DEFLATE_COUNTS)()
    check(call(handle, ctypes.byref(bp), ctypes.byref(nb), stats))
    return _pinned_view(bp.value, nb.value, ctypes.c_uint8), tuple(int(x) for x in stats)


class _Stream:
    """What the native stream front ends (ffq_stream_*) have in common.  Iterating yields
    (rows, fill, fill_offset, end_state, err_offset): `rows` int64[n][6] absolute offsets and
    `fill` (uint8 array, fill[i] = stream byte fill_offset + i) are views of memory the stream
    owns -- valid until the next iteration step."""
    _h = None
    decode = False
    on_close = None        # called once, before the native stream goes away
    consumed = 0
    at_end = False
    filtered = False

    def tell(self):
        """File position behind the last chunk handed out (-1: the source has none)."""
        return int(lib().ffq_stream_tell(self._h)) if self._h else -1

    def path(self):
        """ScanResult.path of the fill the iteration has just yielded (6: index and decoded qualities in one pass)."""
        return int(lib().ffq_stream_path(self._h)) if self._h else -1

    def quals(self):
        """(qual int8[], qoff int64[n + 1]) of the fill the iteration has just yielded (streams
        opened with decode=True); views, valid until the next iteration step.  Record i's decoded
        bytes are qual[qoff[i] : qoff[i] + pos5 - pos4] (row i's columns): packed back to back, or --
        single_pass streams, where the input allows it -- with gaps between the index tiles' segments
        (include/ffq.h, FFQ_F_SINGLE_PASS); qoff[n] is where the last record's bytes end."""
        qp, op, nq = ctypes.c_void_p(), ctypes.c_void_p(), ctypes.c_int64()
        check(lib().ffq_stream_quals(self._h, ctypes.byref(qp), ctypes.byref(op), ctypes.byref(nq)))
        return _pinned_view(qp.value, nq.value, ctypes.c_int8), _pinned_view(op.value, self._last_rows + 1, ctypes.c_int64)

    COLUMNS = {None: 0, "entry": 0, "header": 1, "sequence": 2, "quality": 3}

    def set_filter(self, min_seq_len=None, max_seq_len=None, column=None, value_add=0):
        """Push-down (ffq_stream_set_filter; doc/user-guide.rst:153-180): from the next fill on the iteration yields only the
        rows with min_seq_len <= pos3 - pos2 <= max_seq_len; column = "header" | "sequence" | "quality": that component
        of the kept rows is gathered on the device (selected())."""
        lo, hi = length_bounds(min_seq_len, max_seq_len)
        check(lib().ffq_stream_set_filter(self._h, lo, hi, self.COLUMNS[column], int(value_add)))
        self.filtered = True

    def set_content(self, rules):
        """Content rules in the stream (ffq_stream_set_content; before the first fill): every fill's rows are judged on the
        device by ffq_table_select_reads, as the trims left them; a stream without a filter gets one with open bounds and no
        column (set_filter may come before or after and keeps the rules).  rules: as for Context.table_select_reads."""
        r = content_rules_struct(rules)
        check(lib().ffq_stream_set_content(self._h, None if r is None else ctypes.byref(r)))
        self.filtered = True

    def filter_counts(self):
        """The eight counts (rows kept, dropped by rule 1..6, not judged by content) of the fill the iteration has just
        yielded; any filtered stream."""
        return _counts(lib().ffq_stream_filter_counts, self._h, FILTER_COUNTS)

    def set_dedup(self, drop=True, expected_keys=0, max_bytes=0):
        """Duplicate removal in the stream (ffq_stream_set_dedup; before the first fill): the stream owns a set of sequence
        keys; every fill's rows are keyed as scanned, in front of the trims, and the rows the filter kept are entered right
        behind it -- the first copy in file order stays, what follows sees the rows that remain.  drop False: counted only."""
        check(lib().ffq_stream_set_dedup(self._h, 1 if drop else 0, int(expected_keys), int(max_bytes)))
        self.filtered = True

    def dedup_counts(self):
        """[rows kept, duplicates, rows without a key] summed over every fill so far, [distinct keys, slots, rehashes] of the
        set as it stands (ffq_stream_dedup_counts)."""
        return _counts(lib().ffq_stream_dedup_counts, self._h, DEDUP_COUNTS)

    def set_trim(self, cutoff_back, cutoff_front=0, qual_base=33):
        """Quality trimming in the stream (ffq_stream_set_trim; before the first fill): every fill's rows are trimmed on
        the device right behind the scan, in front of the filter and the column gather (set_filter)."""
        check(lib().ffq_stream_set_trim(self._h, int(qual_base), int(cutoff_front), int(cutoff_back)))

    def trimmed(self):
        """(rows changed, bases removed, rows skipped) of the fill the iteration has just yielded (set_trim)."""
        return tuple(_counts(lib().ffq_stream_trimmed, self._h, 3))

    def set_adapter(self, adapter, err_permille=100, min_overlap=3):
        """3' adapter trimming in the stream (ffq_stream_set_adapter; before the first fill): every fill's rows are cut at
        the adapter on the device right behind the quality trim (set_trim), in front of the filter, the column gather and
        the render."""
        adapter = bytes(adapter)
        check(lib().ffq_stream_set_adapter(self._h, adapter, len(adapter), int(err_permille), int(min_overlap)))

    def adapter_trimmed(self):
        """(rows changed, bases removed, rows skipped) by the adapter step of the fill the iteration has just yielded."""
        return tuple(_counts(lib().ffq_stream_adapter_trimmed, self._h, 3))

    def set_ends(self, rules, qual_base=33):
        """Fixed trims and sliding-window cutting in the stream (ffq_stream_set_ends; before the first fill): every fill's rows
        go through ffq_table_trim_ends on the device in front of the quality trim and every other trim.  rules: as for
        Context.table_trim_ends."""
        r = ends_rules_struct(rules, qual_base)
        check(lib().ffq_stream_set_ends(self._h, ctypes.byref(r) if r is not None else None))

    def ends_trimmed(self):
        """(rows changed, bases removed, rows skipped) by the ends step of the fill the iteration has just yielded."""
        return tuple(_counts(lib().ffq_stream_ends_trimmed, self._h, 3))

    def set_poly(self, poly_g=None, poly_x=None):
        """Poly-tail trimming in the stream (ffq_stream_set_poly; before the first fill): poly_g / poly_x are the min_len of
        that step, None: off (one of them is on).  Poly-G runs behind the quality trim and in front of the adapter trim,
        poly-X behind the adapter trim."""
        check(lib().ffq_stream_set_poly(self._h, int(poly_g or 0), int(poly_x or 0)))

    def poly_trimmed(self):
        """((rows changed, bases removed, rows skipped) by poly-G, the same by poly-X) of the fill the iteration has just
        yielded; zeros for a step that is off."""
        x = (ctypes.c_int64 * 3)()
        return tuple(_counts(lib().ffq_stream_poly_trimmed, self._h, 3, x)), tuple(int(v) for v in x)

    def set_umi(self, rules):
        """UMIs in the stream (ffq_stream_set_umi; before the first fill): every fill's rows lose their UMI on the device in
        front of every trim, and a stream that renders puts it into the names.  rules: a fastqandfurious.UmiRules with loc
        "read1", or a UmiRulesStruct."""
        r = umi_rules_struct(rules)
        check(lib().ffq_stream_set_umi(self._h, ctypes.byref(r) if r is not None else None))

    def umi_counts(self):
        """(rows taken, bases removed, rows skipped, rows tagged in the output) of the fill the iteration has just yielded."""
        return tuple(_counts(lib().ffq_stream_umi_counts, self._h, 4))

    def set_stats(self, which, qual_base=33, max_cycles=512):
        """Statistics in the stream (ffq_stream_set_stats; before the first fill): which = STATS_IN (the rows as scanned),
        STATS_OUT (the rows as handed out, behind trim, adapter and filter) or both; counted on the device over all fills,
        with no host wait per fill."""
        check(lib().ffq_stream_set_stats(self._h, int(which), int(qual_base), int(max_cycles)))
        self._stats_cycles = int(max_cycles)

    def stats(self, which):
        """The running totals (numpy uint64[stats_words(max_cycles)]) of STATS_IN or STATS_OUT over every fill up to and
        including the one the iteration has just yielded (ffq_stream_stats; one host wait)."""
        out = np.zeros(stats_words(getattr(self, "_stats_cycles", 1)), dtype=np.uint64)
        check(lib().ffq_stream_stats(self._h, int(which), ctypes.c_void_p(out.ctypes.data), int(out.size)))
        return out

    def set_render(self):
        """FASTQ text in the stream (ffq_stream_set_render; before the first fill, behind set_trim / set_filter): the rows
        of every fill -- trimmed and filtered first, if the stream does that -- are rendered on the device (rendered())."""
        check(lib().ffq_stream_set_render(self._h))

    def rendered(self):
        """(text, (bytes rendered, rows rendered, rows skipped)) of the fill the iteration has just yielded (set_render):
        `text` is a uint8 view of the stream's pinned memory, valid until the next iteration step."""
        tp, nb, stats = ctypes.c_void_p(), ctypes.c_int64(), (ctypes.c_int64 * 3)()
        check(lib().ffq_stream_rendered(self._h, ctypes.byref(tp), ctypes.byref(nb), stats))
        # (set_compress: the text never leaves the device -- None; compressed() has the members)
        text = None if nb.value and not tp.value else _pinned_view(tp.value, nb.value, ctypes.c_uint8)
        return text, (int(stats[0]), int(stats[1]), int(stats[2]))

    def set_compress(self, mode="bgzf"):
        """The text compressed in the stream (ffq_stream_set_compress; behind set_render, before the first fill): every fill's
        text is written as BGZF members on the device and only those are copied back (compressed()); rendered() then has
        None for the text and its three counts as before.  mode: "bgzf" or None."""
        check(lib().ffq_stream_set_compress(self._h, _compress_mode(mode)))

    def compressed(self):
        """(members, (bytes in, bytes out, members, members stored)) of the fill the iteration has just yielded
        (set_compress): `members` is a uint8 view of the stream's pinned memory, whole BGZF members, valid until the next
        iteration step.  The fills' members one behind another and bgzf_eof_block() at the end are a BGZF file."""
        return _members_of(lib().ffq_stream_compressed, self._h)

    def selected(self):
        """(index int64[kept], n_scanned, col int8[] or None, coloff int64[kept + 1] or None) of the fill the iteration has
        just yielded: index[i] = ordinal of kept row i among the fill's n_scanned records; bytes of kept row i =
        col[coloff[i] : coloff[i + 1]].  Views, valid until the next iteration step."""
        ip, cp, op = ctypes.c_void_p(), ctypes.c_void_p(), ctypes.c_void_p()
        ns, nb = ctypes.c_int64(), ctypes.c_int64()
        check(lib().ffq_stream_selected(self._h, ctypes.byref(ip), ctypes.byref(ns), ctypes.byref(cp), ctypes.byref(op), ctypes.byref(nb)))
        k = self._last_rows
        col = off = None
        if op.value:
            off, col = _pinned_view(op.value, k + 1, ctypes.c_int64), _pinned_view(cp.value, nb.value, ctypes.c_int8)
        return _pinned_view(ip.value, k, ctypes.c_int64), int(ns.value), col, off

    def close(self):
        if self._h:
            if self.on_close is not None:
                cb, self.on_close = self.on_close, None
                cb()
            lib().ffq_stream_close(self._h)
            self._h = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _next(self):
        """One fill: (rows, fill, fill_offset, end_state, err_offset)."""
        rows_p, fill_p = ctypes.c_void_p(), ctypes.c_void_p()
        n, nb, off, err = ctypes.c_int64(), ctypes.c_int64(), ctypes.c_int64(), ctypes.c_int64()
        end = ctypes.c_int32()
        check(lib().ffq_stream_next(self._h, ctypes.byref(rows_p), ctypes.byref(n), ctypes.byref(end),
                                    ctypes.byref(err), ctypes.byref(fill_p), ctypes.byref(nb), ctypes.byref(off)))
        self._last_rows = n.value
        self.consumed = off.value + nb.value     # stream bytes handed out so far (byte i of the fill is stream offset off + i)
        self.at_end = end.value != END_REFILL    # the stream is through (cleanly or with its error): nothing follows
        rows = _pinned_view(rows_p.value, n.value * 6, ctypes.c_int64, (-1, 6))
        return rows, _pinned_view(fill_p.value, nb.value, ctypes.c_uint8), off.value, end.value, err.value


def _decode_flags(decode, single_pass):
    return (F_DECODE_QUAL | (F_SINGLE_PASS if single_pass else 0)) if decode else 0


class FileStream(_Stream):
    """The stream front end over a file descriptor: buffer fills read ahead into pinned memory (reader
    threads; a gzip file is inflated by them) while the previous fill is scanned."""

    def __init__(self, ctx, fd, fbufsize=1 << 24, decode=False, qual_add=-33, start=None, gzip=False, single_pass=True):
        """start: byte of the file the stream begins at (None: the descriptor's current position).
        A descriptor that can seek is read with pread: its own position does not move.
        gzip: the descriptor is a gzip file; the stream's reader thread inflates it into the pinned
        chunk buffers (fbufsize and every offset count DECOMPRESSED bytes).
        single_pass (with decode): the qualities of a fill of four-line records are decoded by the pass
        that builds the line index (one read of the bytes) and come segmented: see quals()."""
        self._ctx = ctx
        self._h = ctypes.c_void_p()
        self.decode = bool(decode)
        opener = lib().ffq_stream_open_gzip if gzip else lib().ffq_stream_open2
        check(opener(ctx.handle, int(fd), int(fbufsize), _decode_flags(decode, single_pass),
                     int(qual_add), -1 if start is None else int(start), ctypes.byref(self._h)))

    def __iter__(self):
        while True:
            t = self._next()
            yield t
            if t[3] != END_REFILL:
                return


class PushStream(_Stream):
    """The stream front end over any object with readinto() / read() -- BytesIO, bz2 / lzma / gzip
    file objects, sockets: no reader thread; every chunk is read by THIS thread straight into the
    stream's pinned chunk buffer (ffq_stream_push_buffer / ffq_stream_push; no bytes object, no
    copy), then scanned.  Iterates like FileStream."""

    def __init__(self, ctx, fh, fbufsize=1 << 23, decode=False, qual_add=-33, single_pass=True, min_fill=None):
        """min_fill: a chunk is handed over SHORT (which is not the end of the stream) as soon as it holds this many
        bytes and a read comes back with less than was asked for -- a live source (a socket, stdin, a decompressor
        over a pipe) has nothing more for now, and the reference's loop yields after every read of fbufsize bytes
        (fastqandfurious.py:222-232 advises small buffers for latency).  None: fbufsize (a chunk is always filled)."""
        self._ctx = ctx
        self._h = ctypes.c_void_p()
        self.decode = bool(decode)
        self._fh = fh
        self._min_fill = int(fbufsize if min_fill is None else max(1, min(int(min_fill), int(fbufsize))))
        self._readinto = getattr(fh, "readinto", None)
        check(lib().ffq_stream_open_push(ctx.handle, int(fbufsize), _decode_flags(decode, single_pass), int(qual_add),
                                         ctypes.byref(self._h)))

    def _pump(self):
        """One chunk of the source into the next slot (reference read(), fastqandfurious.py:30-36: the
        source is exhausted when it returns less than was asked for -- here after asking again until
        the chunk is full or nothing comes)."""
        dst, cap = ctypes.c_void_p(), ctypes.c_int64()
        check(lib().ffq_stream_push_buffer(self._h, ctypes.byref(dst), ctypes.byref(cap)))
        mv = memoryview((ctypes.c_uint8 * cap.value).from_address(dst.value)).cast("B")
        got, eof = 0, False
        while got < cap.value:
            want = cap.value - got
            if self._readinto is not None:
                n = self._readinto(mv[got:]) or 0
            else:
                data = self._fh.read(want)
                n = len(data)
                mv[got:got + n] = data
            if n <= 0:
                eof = True
                break
            got += n
            if n < want and got >= self._min_fill:
                break                       # a short read with enough in hand: hand the chunk over, the rest comes with the next
        check(lib().ffq_stream_push(self._h, got, 1 if eof else 0))

    def __iter__(self):
        self._pump()
        while True:
            t = self._next()
            yield t
            if t[3] != END_REFILL:
                return
            self._pump()


class PairStream:
    """Two streams whose i-th records are mates, walked in lockstep (ffq_pair; include/ffq.h): mate1 / mate2 are fresh
    FileStreams or PushStreams of one context, configured beforehand (set_trim, set_adapter, set_filter without a column,
    set_content, set_stats, set_render); set_overlap(), set_correct() and set_merge() here, before the first step.  Iterating yields (n_in, n_out,
    end_state, err_mate, err_offset) per ROUND; after each step the streams' own accessors (rendered(), trimmed(), adapter_trimmed(), filter_counts(), stats()) report that
    mate's share of the round.  PushStream mates are pumped here whenever the walk takes a new chunk of theirs.  The
    iteration ends behind the first end_state that is not END_REFILL (END_OK, a mate's END_ERR_*, END_ERR_PAIR_COUNT,
    END_ERR_PAIR_NAMES).  close() does not close the two streams."""

    def __init__(self, mate1, mate2, pair_filter="any", check_names=True):
        self._h = ctypes.c_void_p()
        self.mates = (mate1, mate2)
        self._ctx = mate1._ctx
        self.rounds = 0
        self._last_out = 0
        check(lib().ffq_pair_open(mate1._h, mate2._h, _pair_filter(pair_filter), 1 if check_names else 0, ctypes.byref(self._h)))

    def _next(self):
        wants = lib().ffq_pair_wants(self._h)
        for k, st in enumerate(self.mates):
            if wants & (1 << k) and isinstance(st, PushStream):
                st._pump()
        n_in, n_out, err = ctypes.c_int64(), ctypes.c_int64(), ctypes.c_int64()
        end, mate = ctypes.c_int32(), ctypes.c_int32()
        check(lib().ffq_pair_next(self._h, ctypes.byref(n_in), ctypes.byref(n_out), ctypes.byref(end), ctypes.byref(mate), ctypes.byref(err)))
        self.rounds += 1
        self._last_out = n_out.value
        for st in self.mates:
            st._last_rows = n_out.value
        return n_in.value, n_out.value, end.value, mate.value, err.value

    def __iter__(self):
        while True:
            t = self._next()
            yield t
            if t[2] != END_REFILL:
                return

    def _rows(self, mate, n_rows):
        """ffq_pair_rows of one mate: (its first n_rows rows, the fill, the fill's offset)"""
        rp, fp = ctypes.c_void_p(), ctypes.c_void_p()
        nb, off = ctypes.c_int64(), ctypes.c_int64()
        check(lib().ffq_pair_rows(self._h, int(mate), ctypes.byref(rp), ctypes.byref(fp), ctypes.byref(nb), ctypes.byref(off)))
        fill = _pinned_view(fp.value, nb.value if fp.value else 0, ctypes.c_uint8)
        return _pinned_view(rp.value, n_rows * 6, ctypes.c_int64, (-1, 6)), fill, off.value

    def rows(self, mate):
        """(rows int64[n_out][6], fill uint8[], fill_offset) of mate 1 or 2 for the round just yielded: the kept rows and
        the fill they point into (fill[i] = stream byte fill_offset + i).  Views, valid until the next step."""
        return self._rows(mate, self._last_out)

    def mismatch(self):
        """Behind END_ERR_PAIR_NAMES: the two headers (bytes, as entryfunc cuts them) of the pair that is not one."""
        out = []
        for mate in (1, 2):
            (row,), fill, off = self._rows(mate, 1)
            out.append(bytes(fill[row[0] + 1 - off:row[1] - off]))
        return tuple(out)

    def selected(self):
        """(index int64[n_out], pairs) of the round just yielded: index[k] = the ordinal, among the round's n_in pairs, of
        kept pair k; pairs = [kept, dropped, only mate 1 failed, only mate 2 failed, both failed]."""
        ip = ctypes.c_void_p()
        pairs = (ctypes.c_int64 * PAIR_COUNTS)()
        check(lib().ffq_pair_selected(self._h, ctypes.byref(ip), pairs))
        return _pinned_view(ip.value, self._last_out, ctypes.c_int64), [int(x) for x in pairs]

    def set_overlap(self, rules, trim=True):
        """Every round analyses the overlap of the mates behind the per-mate trims and in front of the filter, and with
        `trim` cuts both mates by it (ffq_pair_set_overlap; rules as Context.table_pair_overlap takes them, None: off).
        Before the first step only."""
        r = overlap_rules_struct(rules, trim)
        check(lib().ffq_pair_set_overlap(self._h, None if r is None else ctypes.byref(r)))

    def overlap(self, hist=True):
        """(counts, insert_hist): the six counts of the round just yielded (Context.table_pair_overlap's), and the insert sizes
        of every round so far as uint64[OVERLAP_HIST_WORDS] (None without `hist`: no host wait)."""
        h = np.zeros(OVERLAP_HIST_WORDS, dtype=np.uint64) if hist else None
        return _counts(lib().ffq_pair_overlap, self._h, OVERLAP_COUNTS, ctypes.c_void_p(h.ctypes.data) if hist else None, OVERLAP_HIST_WORDS), h

    def set_umi(self, rules):
        """UMIs of the pair (ffq_pair_set_umi; before the first step, not with set_merge): the mate or mates rules.loc names
        lose their UMI in front of every trim, and both mates' rendered() names get the same insert.  rules: a
        fastqandfurious.UmiRules or a UmiRulesStruct."""
        r = umi_rules_struct(rules)
        check(lib().ffq_pair_set_umi(self._h, ctypes.byref(r) if r is not None else None))

    def umi_counts(self):
        """((rows taken, bases removed, rows skipped, rows tagged in the output) of mate 1, the same of mate 2) for the round
        just yielded."""
        x = (ctypes.c_int64 * 4)()
        return tuple(_counts(lib().ffq_pair_umi_counts, self._h, 4, x)), tuple(int(v) for v in x)

    def set_merge(self, on=True):
        """Behind the filter every round merges the kept pairs whose insert size allows it (ffq_pair_set_merge; needs
        set_overlap).  Those pairs leave the two ordinary outputs: rows(), selected()'s index and the mates' rendered() are
        then the kept pairs that were not merged, n_out their number; merged() has the others.  Before the first step only."""
        check(lib().ffq_pair_set_merge(self._h, 1 if on else 0))

    def set_correct(self, rules, qual_base=33):
        """Every round corrects mismatched bases inside the mates' overlap in both fills' device bytes, between the overlap and
        the filter (ffq_pair_set_correct; needs set_overlap; rules as Context.table_pair_correct takes them, None: off).  The
        filter, statistics OUT, rendered() and merged() see the corrected bytes; rows()' fill stays as read.  Before the first
        step only."""
        r = correct_rules_struct(rules, qual_base)
        check(lib().ffq_pair_set_correct(self._h, None if r is None else ctypes.byref(r)))

    def corrected(self):
        """(counts, matrix): the six counts of the round just yielded (Context.table_pair_correct's) and the corrections of
        every round so far as int64[5][4] by (class before, class after) (ffq_pair_corrected)."""
        mat = (ctypes.c_int64 * CORRECT_MATRIX_WORDS)()
        return _counts(lib().ffq_pair_corrected, self._h, CORRECT_COUNTS, mat), np.array(mat, dtype=np.int64).reshape(5, 4)

    def set_dedup(self, drop=True, expected_keys=0, max_bytes=0):
        """Duplicate PAIRS dropped behind the filter and in front of the merge (ffq_pair_set_dedup; before the first step;
        neither stream may have a dedup of its own): a pair's key is made of both mates' sequence keys, as scanned."""
        check(lib().ffq_pair_set_dedup(self._h, 1 if drop else 0, int(expected_keys), int(max_bytes)))

    def dedup_counts(self):
        """_Stream.dedup_counts, in pairs, over every round so far (ffq_pair_dedup_counts)."""
        return _counts(lib().ffq_pair_dedup_counts, self._h, DEDUP_COUNTS)

    def merged(self):
        """(text uint8[], counts) of the round just yielded: the FASTQ text of the merged pairs (a view, valid until the next
        step) and the six counts of Context.table_pair_merge."""
        tp, nb, counts = ctypes.c_void_p(), ctypes.c_int64(), (ctypes.c_int64 * MERGE_COUNTS)()
        check(lib().ffq_pair_merged(self._h, ctypes.byref(tp), ctypes.byref(nb), counts))
        return _pinned_view(tp.value, nb.value if tp.value else 0, ctypes.c_uint8), [int(x) for x in counts]

    def set_compress(self, mode="bgzf"):
        """The round's merged text as BGZF members (ffq_pair_set_compress; behind set_merge, before the first step):
        merged_bgzf() has them, merged() then has an empty text and its counts.  The mates' own text is their streams'."""
        check(lib().ffq_pair_set_compress(self._h, _compress_mode(mode)))

    def merged_bgzf(self):
        """_Stream.compressed() for the merged reads of the round just yielded (ffq_pair_merged_bgzf)."""
        return _members_of(lib().ffq_pair_merged_bgzf, self._h)

    def close(self):
        if self._h:
            lib().ffq_pair_close(self._h)
            self._h = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


_default_ctx = {}


def gunzip_fd(fd, cap, chunk=16 << 20, threads=0):
    """The stream front end's gzip reader on its own (ffq_gunzip_fd; host only, no device): the file behind
    `fd` inflated into a new uint8 array of at most `cap` bytes, `chunk` bytes per call of the reader.
    Returns (array, members inflated side by side)."""
    import numpy as np
    out = np.empty(max(int(cap), 1), dtype=np.uint8)
    npar = ctypes.c_int64(0)
    n = lib().ffq_gunzip_fd(int(fd), out.ctypes.data, int(cap), int(chunk), int(threads), ctypes.byref(npar))
    if n < 0:
        check(int(n))
    return out[:n], int(npar.value)


def bgzf_range(fd, c_lo, c_hi, out=None, threads=0):
    """ffq_bgzf_range (host only): the BGZF members whose first byte lies in [c_lo, c_hi) of the file behind fd.
    out=None: nothing is inflated -> (c_first, c_end, n_bytes, n_members), n_bytes = what the members' trailers promise;
    out = a writable uint8 array of at least that many bytes: inflated into it, the same tuple.  FFQGzipError (an OSError)
    for what is not BGZF or does not inflate to its trailer, FFQGzipTruncated (an EOFError) for a file cut short."""
    cf, ce, no, nm = ctypes.c_int64(), ctypes.c_int64(), ctypes.c_int64(), ctypes.c_int64()
    check(lib().ffq_bgzf_range(int(fd), int(c_lo), int(c_hi), ctypes.c_void_p(out.ctypes.data) if out is not None else None,
                               int(out.size) if out is not None else 0, int(threads), ctypes.byref(cf), ctypes.byref(ce),
                               ctypes.byref(no), ctypes.byref(nm)))
    return int(cf.value), int(ce.value), int(no.value), int(nm.value)


def gunzip_stats():
    """Counters of the several-thread inflate of plain gzip members (ffq_gunzip_stats; csrc/ffq_pgz.h)."""
    a = (ctypes.c_int64 * 5)()
    lib().ffq_gunzip_stats(a)
    return dict(zip(("batches", "chunks", "rejected", "giveups", "members"), (int(x) for x in a)))


def default_context(device=None):
    """Process-wide context for `device` (default: LOCAL_RANK or 0)."""
    if device is None:
        device = int(os.environ.get("LOCAL_RANK", "0"))
    ctx = _default_ctx.get(device)
    if ctx is None:
        ctx = Context(device)
        _default_ctx[device] = ctx
    return ctx


class ReadProbe:
    """bench.py's `hbm_read_probe`: what this box's memory system gives a pure streaming read, measured
    by the INSTRUMENTED build (libffq_probe.so, include/ffq_probe.h) loaded beside the product library
    -- its own handle, its own context; the product library has no such entry point."""

    def __init__(self, device=0):
        from . import build as _build
        _share_torch_hip_runtime()
        self._L = ctypes.CDLL(_build.build_probe())
        L = self._L
        vp, i64, i32 = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int
        L.ffq_last_error.restype = ctypes.c_char_p
        L.ffq_ctx_create.argtypes = [i32, ctypes.POINTER(vp)]
        L.ffq_ctx_destroy.argtypes = [vp]
        L.ffq_ctx_destroy.restype = None
        L.ffq_read_probe.argtypes = [vp, vp, i64, i32, i32, ctypes.POINTER(ctypes.c_float)]
        self._h = vp()
        rc = L.ffq_ctx_create(int(device), ctypes.byref(self._h))
        if rc != OK:
            raise FFQError(rc, L.ffq_last_error().decode("utf-8", "replace"))

    def read_ms(self, dptr, n_bytes, mode=6, reps=10):
        ms = ctypes.c_float(0)
        rc = self._L.ffq_read_probe(self._h, ctypes.c_void_p(dptr), int(n_bytes), int(mode), int(reps), ctypes.byref(ms))
        if rc != OK:
            raise FFQError(rc, self._L.ffq_last_error().decode("utf-8", "replace"))
        return ms.value

    def close(self):
        if self._h:
            self._L.ffq_ctx_destroy(self._h)
            self._h = ctypes.c_void_p()
