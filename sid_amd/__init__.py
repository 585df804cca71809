"""sid_amd — Python bindings of libsid.so, the MI355X-native sid hot path.

The product is the C ABI in ``include/sid.h`` (``build/libsid.so``) and the
``build/sid`` command line that mirrors the reference's ``sid`` binary
(sid.cpp:1-110).  This module is a thin ctypes layer over that ABI for the
tests and ``bench.py``; it adds no computation of its own.

Device memory and streams come from PyTorch (plumbing only): when torch is
importable it is imported *before* libsid.so is loaded, so the process holds a
single HIP runtime.  There is no CPU fallback: if ``build/libsid.so`` is
missing, :func:`lib` raises.
"""
from __future__ import annotations

import ctypes as C
import os
from dataclasses import dataclass

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# SID_LIB_PATH: another build of the same sources (A/B measurements only)
LIB_PATH = os.environ.get("SID_LIB_PATH") or os.path.join(ROOT, "build", "libsid.so")
CLI_PATH = os.path.join(ROOT, "build", "sid")

METHOD_LOCAL, METHOD_LIKELIHOOD_RATIO, METHOD_BAYES, METHOD_QUALITY = 0, 1, 2, 3
METHODS = {"local": METHOD_LOCAL, "likelihood_ratio": METHOD_LIKELIHOOD_RATIO,
           "bayes": METHOD_BAYES, "quality": METHOD_QUALITY}

SID_OK = 0
STATUS = {0: "SID_OK", 1: "SID_EINVAL", 2: "SID_EHIP", 3: "SID_ENOMEM", 4: "SID_EMALFORMED",
          5: "SID_EMISSING_MQ", 6: "SID_ENULLCHROM", 7: "SID_ESTATE", 8: "SID_EBADFUNC",
          9: "SID_EEMPTY", 10: "SID_EIO", 11: "SID_ERANGE", 12: "SID_ENOBQ", 13: "SID_ELINE", 14: "SID_EBGZF"}

CODE_HET = 0x80
CODE_DROPPED = 0x40


class SidError(RuntimeError):
    def __init__(self, status: int, what: str = ""):
        self.status = status
        msg = f"{what}: {STATUS.get(status, status)}" if what else STATUS.get(status, str(status))
        if status == 2 and _LIB is not None:
            msg += f" (hip error {_LIB.sid_last_hip_error()})"
        super().__init__(msg)


class Opts(C.Structure):
    """sid_opts = GlobalOptions (sid.cpp:11-17)."""
    _fields_ = [("method", C.c_int), ("estimate_prior", C.c_int), ("snp_prior", C.c_double),
                ("significance_level", C.c_double), ("site_error_threshold", C.c_double), ("select", C.c_int),
                ("variants", C.c_int), ("regions", C.c_void_p), ("context", C.c_int)]
    # sid_opts.window, the int behind `context`: the structure's last four bytes (its size is a multiple
    # of the 8-byte alignment of its doubles and pointer, so they belong to it).  The field list above
    # ends at `context`, as its users have it; `window` reads and writes those bytes
    WINDOW_OFFSET = 52

    @property
    def window(self) -> int:
        return C.c_int.from_address(C.addressof(self) + self.WINDOW_OFFSET).value

    @window.setter
    def window(self, v: int):
        C.c_int.from_address(C.addressof(self) + self.WINDOW_OFFSET).value = int(v)


assert Opts.WINDOW_OFFSET == Opts.context.offset + 4 and C.sizeof(Opts) == Opts.WINDOW_OFFSET + 4


class Estimate(C.Structure):
    _fields_ = [("heterozygosity", C.c_double), ("error_rate", C.c_double), ("fval", C.c_double),
                ("dist", C.c_double * 4), ("iterations", C.c_int), ("converged", C.c_int),
                ("evaluations", C.c_uint64), ("n_unique", C.c_uint64)]


class EngineCfg(C.Structure):
    """sid_engine_cfg (include/sid.h, streaming engine)."""
    _fields_ = [("devices", C.c_int), ("first_device", C.c_int), ("chunk_bytes", C.c_uint64),
                ("slots", C.c_int), ("hold_bytes", C.c_uint64), ("retain_bytes", C.c_uint64),
                ("host_threads", C.c_int), ("verbose", C.c_int), ("device_sink", C.c_int), ("lanes", C.c_int),
                ("host_hold_bytes", C.c_uint64), ("strip", C.c_int)]


class RunStats(C.Structure):
    _fields_ = [("sites", C.c_uint64), ("chunks", C.c_uint64), ("bytes_in", C.c_uint64),
                ("bytes_out", C.c_uint64), ("chunks_held", C.c_uint64), ("chunks_retained", C.c_uint64),
                ("chunks_reloaded", C.c_uint64), ("devices", C.c_int), ("status_kind", C.c_int),
                ("err_offset", C.c_uint64), ("ingest_s", C.c_double), ("estimate_s", C.c_double),
                ("emit_s", C.c_double), ("estimate", Estimate), ("chunks_registered", C.c_uint64),
                ("register_s", C.c_double), ("h2d_s", C.c_double), ("h2d_bytes", C.c_uint64),
                ("chunks_tiled", C.c_uint64), ("tile_overflows", C.c_uint64),
                ("tile_overflows_queued", C.c_uint64), ("bgzf_bytes", C.c_uint64), ("bgzf_blocks", C.c_uint64),
                ("window_rows", C.c_uint64)]
    # the rows of the depth histogram (Engine(depth_hist=True)): no field of sid_run_stats, whose layout
    # stands -- Engine.emit sets it on the instance from sid_engine_depth_hist's count
    depth_rows = 0
    # what the strip crews did (Engine(strip=...)): likewise no fields -- Engine.ingest sets them on the
    # instance from sid_engine_strip_stats
    chunks_stripped = 0
    strip_bytes = 0


class Window(C.Structure):
    """sid_window: one row of the windowed summary (chrom is not NUL-terminated)."""
    _fields_ = [("chrom", C.c_void_p), ("chrom_len", C.c_uint32), ("start", C.c_int64), ("end", C.c_int64),
                ("sites", C.c_uint64), ("records", C.c_uint64), ("het", C.c_uint64), ("hom", C.c_uint64)]


class DepthRow(C.Structure):
    """sid_depth_row: one row of the depth histogram."""
    _fields_ = [("sites", C.c_uint64), ("records", C.c_uint64), ("het", C.c_uint64), ("hom", C.c_uint64),
                ("depth", C.c_uint32), ("pad", C.c_uint32)]


class RegionRow(C.Structure):
    """sid_region_row: one row of the region rows (chrom is not NUL-terminated)."""
    _fields_ = [("chrom", C.c_void_p), ("chrom_len", C.c_uint32), ("start", C.c_int64), ("end", C.c_int64),
                ("sites", C.c_uint64), ("depth", C.c_uint64), ("records", C.c_uint64), ("het", C.c_uint64),
                ("hom", C.c_uint64)]


REGION_STATS_MAX = 1 << 20   # SID_REGION_STATS_MAX


class CallableRow(C.Structure):
    """sid_callable_row: one callable run (BED start and end)."""
    _fields_ = [("chrom", C.c_void_p), ("chrom_len", C.c_uint32), ("pad", C.c_uint32),
                ("start", C.c_int64), ("end", C.c_int64), ("het", C.c_uint64)]


class Placement(C.Structure):
    """sid_placement (include/sid.h): a pipeline's host placement."""
    _fields_ = [("device", C.c_int), ("gpu_numa_node", C.c_int), ("cpus", C.c_int), ("first_cpu", C.c_int),
                ("arena_numa_node", C.c_int), ("ring_numa_node", C.c_int), ("pci", C.c_char * 16)]


class EngineProf(C.Structure):
    _fields_ = [("chunks", C.c_uint64), ("index_ms", C.c_double), ("parse_ms", C.c_double), ("call_ms", C.c_double),
                ("hist_ms", C.c_double), ("fmt_len_ms", C.c_double), ("fmt_write_ms", C.c_double)]


_LIB = None

# (name, restype, argtypes) for every entry point of include/sid.h
_P, _SZ, _U64, _I, _D = C.c_void_p, C.c_size_t, C.c_uint64, C.c_int, C.c_double
WRITE_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.POINTER(C.c_char), C.c_size_t)   # sid_write_fn
SIGNATURES = [
    ("sid_strerror", C.c_char_p, [_I]),
    ("sid_last_hip_error", _I, []),
    ("sid_version", C.c_char_p, []),
    ("sid_opts_default", None, [C.POINTER(Opts)]),
    ("sid_select_mark", _I, [_P, _SZ, _I]),
    ("sid_strip_lines", _SZ, [_P, _SZ, _P, _SZ, C.POINTER(_U64)]),
    ("sid_strip_lines_impl", _SZ, [_I, _P, _SZ, _P, _SZ, C.POINTER(_U64)]),
    ("sid_strip_impl", _I, []),
    ("sid_engine_strip_stats", _I, [_P, C.POINTER(_U64), C.POINTER(_U64)]),
    ("sid_strip_map", _SZ, [_P, _SZ, _SZ]),
    ("sid_context_mark", _I, [_P, _P, _SZ, _I]),
    ("sid_windows_host", _I, [_P, _SZ, _SZ, _P, _I, C.POINTER(C.POINTER(Window)), C.POINTER(C.c_size_t)]),
    ("sid_windows_free", None, [C.POINTER(Window)]),
    ("sid_windows_format", _I, [C.POINTER(Window), _SZ, _I, _P, _SZ, C.POINTER(C.c_size_t)]),
    ("sid_dtext_windows", _I, [_P, _P, _SZ, _SZ, _P, C.POINTER(C.POINTER(Window)), C.POINTER(C.c_size_t), _P]),
    ("sid_engine_windows", _I, [_P, C.POINTER(C.POINTER(Window)), C.POINTER(C.c_size_t)]),
    ("sid_depth_hist_host", _I, [_P, _SZ, _SZ, _P, C.POINTER(C.POINTER(DepthRow)), C.POINTER(C.c_size_t)]),
    ("sid_depth_hist_free", None, [C.POINTER(DepthRow)]),
    ("sid_depth_hist_format", _I, [C.POINTER(DepthRow), _SZ, _I, _P, _SZ, C.POINTER(C.c_size_t)]),
    ("sid_depth_hist_merge", _I, [C.POINTER(DepthRow), _SZ, C.POINTER(DepthRow), _SZ,
                                  C.POINTER(C.POINTER(DepthRow)), C.POINTER(C.c_size_t)]),
    ("sid_dtext_depth_hist", _I, [_P, _P, _SZ, _SZ, _P, C.POINTER(C.POINTER(DepthRow)), C.POINTER(C.c_size_t), _P]),
    ("sid_engine_set_depth_hist", _I, [_P, _I]),
    ("sid_engine_depth_hist", _I, [_P, C.POINTER(C.POINTER(DepthRow)), C.POINTER(C.c_size_t)]),
    ("sid_regions_interval", _I, [_P, _SZ, C.POINTER(_P), C.POINTER(C.c_uint32), C.POINTER(C.c_int64),
                                  C.POINTER(C.c_int64)]),
    ("sid_region_stats_valid", _I, [_P]),
    ("sid_region_stats_host", _I, [_P, _P, _SZ, _SZ, _P, C.POINTER(C.POINTER(RegionRow)), C.POINTER(C.c_size_t)]),
    ("sid_region_stats_free", None, [C.POINTER(RegionRow)]),
    ("sid_region_stats_format", _I, [C.POINTER(RegionRow), _SZ, _I, _P, _SZ, C.POINTER(C.c_size_t)]),
    ("sid_region_stats_merge", _I, [C.POINTER(RegionRow), C.POINTER(RegionRow), _SZ, C.POINTER(C.POINTER(RegionRow))]),
    ("sid_dtext_region_stats", _I, [_P, _P, _SZ, _SZ, _P, C.POINTER(C.POINTER(RegionRow)), C.POINTER(C.c_size_t), _P]),
    ("sid_engine_set_region_stats", _I, [_P, _I]),
    ("sid_engine_region_stats", _I, [_P, C.POINTER(C.POINTER(RegionRow)), C.POINTER(C.c_size_t)]),
    ("sid_callable_host", _I, [_P, _SZ, _SZ, _P, _I, _I, C.POINTER(C.POINTER(CallableRow)), C.POINTER(C.c_size_t)]),
    ("sid_callable_free", None, [C.POINTER(CallableRow)]),
    ("sid_callable_format", _I, [C.POINTER(CallableRow), _SZ, _P, _SZ, C.POINTER(C.c_size_t)]),
    ("sid_callable_join", _I, [C.POINTER(CallableRow), _SZ, _I, C.POINTER(CallableRow), _SZ, _I,
                               C.POINTER(C.POINTER(CallableRow)), C.POINTER(C.c_size_t)]),
    ("sid_callable_stitch_chunks", _I, [_P, _P, _P, _P, _P, _SZ, C.POINTER(C.POINTER(CallableRow)),
                                        C.POINTER(C.c_size_t)]),
    ("sid_dtext_callable", _I, [_P, _P, _SZ, _SZ, _P, C.POINTER(C.POINTER(CallableRow)), C.POINTER(C.c_size_t), _P]),
    ("sid_regions_from_bed", _I, [C.c_char_p, _SZ, C.POINTER(_P), C.POINTER(C.c_uint64)]),
    ("sid_regions_from_intervals", _I, [C.POINTER(C.c_char_p), _P, _P, _SZ, C.POINTER(_P)]),
    ("sid_regions_intervals", _SZ, [_P]),
    ("sid_regions_chroms", _SZ, [_P]),
    ("sid_regions_contains", _I, [_P, C.c_char_p, _SZ, C.c_int32]),
    ("sid_regions_free", None, [_P]),
    ("sid_regions_mark", _I, [_P, _P, _SZ, _SZ, _P]),
    ("sid_variants_mark", _I, [_P, _SZ, _SZ, _P]),
    ("sid_depth_mark", _I, [_P, _SZ, _SZ, _I, _I, _P]),
    ("sid_set_depth", _I, [_P, _I, _I]),
    ("sid_engine_set_depth", _I, [_P, _I, _I]),
    ("sid_set_format", _I, [_P, _I]),
    ("sid_engine_set_format", _I, [_P, _I]),
    ("sid_format_vcf", _I, [_P, _SZ, _SZ, _P, _P, _P, _P, _SZ, C.POINTER(C.c_size_t)]),
    ("sid_vcf_header", _I, [C.POINTER(Opts), _P, _SZ, C.POINTER(C.c_size_t)]),
    ("sid_device_count", _I, [C.POINTER(C.c_int)]),
    ("sid_create", _I, [_I, C.POINTER(Opts), C.POINTER(_P)]),
    ("sid_destroy", _I, [_P]),
    ("sid_set_prior", _I, [_P, _D]),
    ("sid_call_local", _I, [_P, _P, _SZ, _P, _P, _P, _P]),
    ("sid_timing_enable", _I, [_P, _I]),
    ("sid_timing_read", _I, [_P, C.POINTER(C.c_uint64), C.POINTER(C.c_double), C.POINTER(C.c_double)]),
    ("sid_profile_reset", _I, [_P, _P]),
    ("sid_profile_accumulate", _I, [_P, _P, _SZ, _P]),
    ("sid_profile_table", _I, [_P, _P, _P, _SZ, C.POINTER(C.c_size_t)]),
    ("sid_profile_load", _I, [_P, _P, _P, _SZ]),
    ("sid_lynch_setup", _I, [_P, C.POINTER(Estimate)]),
    ("sid_lynch_objective", _I, [_P, _D, _D, C.POINTER(C.c_double)]),
    ("sid_lynch_prepare", _I, [_P, _I, C.POINTER(Estimate)]),
    ("sid_lynch_prepare_given", _I, [_P, _I, C.POINTER(Estimate), C.POINTER(Estimate)]),
    ("sid_lookup_sites", _I, [_P, _P, _SZ, _P, _P, _P, _P]),
    ("sid_synth_counts", _I, [_P, _U64, _D, _U64, _SZ, _P, _P]),
    ("sid_synth_text", _I, [_U64, _D, _U64, _SZ, _U64, _P, _SZ, C.POINTER(C.c_size_t)]),
    ("sid_synth_counts_host", _I, [_U64, _D, _U64, _SZ, _P]),
    ("sid_synth_text_device", _I, [_P, _U64, _D, _U64, _SZ, _U64, _P, _SZ, C.POINTER(C.c_size_t), _P]),
    ("sid_synth_text_mq", _I, [_U64, _D, _U64, _SZ, _U64, _P, _SZ, C.POINTER(C.c_size_t)]),
    ("sid_parse_text", _I, [C.c_char_p, _SZ, _I, C.POINTER(_P), C.POINTER(C.c_uint64)]),
    ("sid_sites_free", None, [_P]),
    ("sid_sites_count", _SZ, [_P]),
    ("sid_sites_counts", _P, [_P]),
    ("sid_sites_positions", _P, [_P]),
    ("sid_sites_refs", _P, [_P]),
    ("sid_sites_chrom_segments", _SZ, [_P]),
    ("sid_sites_chrom_name", C.c_char_p, [_P, _SZ, C.POINTER(C.c_uint64)]),
    ("sid_format_csv", _I, [_P, _SZ, _SZ, _P, _P, _P, C.c_char_p, _P, _SZ, C.POINTER(C.c_size_t)]),
    ("sid_format_double", _I, [_D, C.c_char_p, _SZ]),
    ("sid_dtext_parse", _I, [_P, _P, _SZ, _SZ, C.POINTER(_P), C.POINTER(C.c_uint64), _P]),
    ("sid_dtext_parse_fd", _I, [_P, _I, _U64, _U64, _I, C.POINTER(_P), C.POINTER(C.c_uint64), _P]),
    ("sid_dtext_count", _SZ, [_P]),
    ("sid_dtext_counts", _P, [_P]),
    ("sid_dtext_format", _I, [_P, _P, _SZ, _SZ, _P, _P, _P, C.c_char_p, WRITE_FN, _P, _P]),
    ("sid_dtext_free", _I, [_P]),
    ("sid_call_quality", _I, [_P, _P, _P, _P, _P, _P]),
    ("sid_format_g6", _I, [_D, C.c_char_p, _SZ]),
    ("sid_format_g6_device", _I, [_P, _P, _SZ, _P, _P]),
    ("sid_bgzf_index", _I, [_P, _SZ, C.POINTER(_P), C.POINTER(C.c_uint64)]),
    ("sid_bgzf_blocks", _SZ, [_P]),
    ("sid_bgzf_text_len", _U64, [_P]),
    ("sid_bgzf_block", _I, [_P, _SZ, C.POINTER(C.c_uint64), C.POINTER(C.c_uint32), C.POINTER(C.c_uint64),
                            C.POINTER(C.c_uint32)]),
    ("sid_bgzf_free", None, [_P]),
    ("sid_bgzf_inflate_host", _I, [_P, _SZ, _P, _SZ, C.POINTER(C.c_size_t), C.POINTER(C.c_uint64)]),
    ("sid_bgzf_inflate_device", _I, [_P, _P, _P, _SZ, _SZ, _P, _SZ, C.POINTER(C.c_uint64), _P]),
    ("sid_crc32", C.c_uint32, [C.c_uint32, _P, _SZ]),
    ("sid_engine_cfg_default", None, [C.POINTER(EngineCfg)]),
    ("sid_engine_create", _I, [C.POINTER(Opts), C.POINTER(EngineCfg), C.POINTER(_P)]),
    ("sid_engine_destroy", _I, [_P]),
    ("sid_engine_devices", _I, [_P]),
    ("sid_engine_context", _P, [_P, _I]),
    ("sid_engine_placement", _I, [_P, _I, C.POINTER(Placement)]),
    ("sid_engine_source_text", _I, [_P, _P, _U64]),
    ("sid_engine_source_file", _I, [_P, _I, _U64, _U64]),
    ("sid_engine_source_bgzf", _I, [_P, _P, _U64, C.POINTER(C.c_uint64)]),
    ("sid_engine_source_bgzf_file", _I, [_P, _I, _U64, _U64, C.POINTER(C.c_uint64)]),
    ("sid_engine_source_device_text", _I, [_P, _P, _U64]),
    ("sid_engine_source_synth", _I, [_P, _U64, _D, _U64, _U64, _U64, _U64, _I]),
    ("sid_engine_ingest", _I, [_P, C.POINTER(RunStats)]),
    ("sid_engine_estimate", _I, [_P, C.POINTER(Estimate), C.POINTER(Estimate)]),
    ("sid_engine_emit", _I, [_P, C.c_char_p, WRITE_FN, _P, C.POINTER(RunStats)]),
    ("sid_engine_run", _I, [_P, C.c_char_p, WRITE_FN, _P, C.POINTER(RunStats)]),
    ("sid_engine_profile_table", _I, [_P, _P, _P, _SZ, C.POINTER(C.c_size_t)]),
    ("sid_engine_profile_load", _I, [_P, _P, _P, _SZ]),
    ("sid_engine_records", _I, [_P, _U64, C.POINTER(C.c_void_p), C.POINTER(C.c_uint64)]),
    ("sid_engine_profile", _I, [_P, _I]),
    ("sid_engine_profile_read", _I, [_P, C.POINTER(EngineProf)]),
]


def lib():
    """Load build/libsid.so (torch first, if importable: one HIP runtime)."""
    global _LIB
    if _LIB is not None:
        return _LIB
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(f"{LIB_PATH} is missing: run `make` (or __graft_entry__.build()); "
                           "sid_amd has no CPU fallback")
    try:  # plumbing: device memory / streams / distributed come from torch
        import torch  # noqa: F401
    except Exception:
        pass
    L = C.CDLL(LIB_PATH, mode=C.RTLD_GLOBAL)
    for name, res, args in SIGNATURES:
        f = getattr(L, name)
        f.restype = res
        f.argtypes = args
    _LIB = L
    return L


def check(status: int, what: str = ""):
    if status != SID_OK:
        raise SidError(status, what)


def _ptr(a: np.ndarray):
    return a.ctypes.data_as(C.c_void_p)


SELECT = {"all": 0, "het": 1, "hom": 2}   # SID_SELECT_*: the records emitted, by label (--only)
FORMATS = {"csv": 0, "vcf": 1}            # SID_FORMAT_*: what a record is (--vcf)


def _format(fmt) -> int:
    if isinstance(fmt, str):
        if fmt not in FORMATS:
            raise SidError(1, f"format: expected one of {sorted(FORMATS)}, got {fmt!r}")
        return FORMATS[fmt]
    return int(fmt)   # (another value: SID_EINVAL from the setter)


class Regions:
    """A region set (sid_regions, --regions): BED intervals, 0-based and
    half-open, merged per chrom; a site is inside when start < pos <= end.
    Built from BED bytes, a path to a BED file, or a list of (chrom, start,
    end).  A malformed BED line raises SidError naming its 1-based line.
    Context and Engine copy what they need when they are created, so the object
    may be closed right after."""

    def __init__(self, source):
        self.h = None
        L = lib()
        h = C.c_void_p()
        if isinstance(source, (str, os.PathLike)):
            with open(source, "rb") as f:
                source = f.read()
        if isinstance(source, (bytes, bytearray, memoryview)):
            text = bytes(source)
            line = C.c_uint64(0)
            st = L.sid_regions_from_bed(text, len(text), C.byref(h), C.byref(line))
            if st != SID_OK:
                raise SidError(st, f"sid_regions_from_bed: line {line.value}: malformed region")
        else:
            iv = list(source)
            names = (C.c_char_p * max(len(iv), 1))(*[c if isinstance(c, bytes) else str(c).encode() for c, _, _ in iv])
            for _, s, e in iv:
                if not (-2**31 <= int(s) < 2**31 and -2**31 <= int(e) < 2**31):
                    raise SidError(1, f"regions: interval ({s}, {e}) outside int32")
            start = np.array([s for _, s, _ in iv], np.int32)
            end = np.array([e for _, _, e in iv], np.int32)
            check(L.sid_regions_from_intervals(names, _ptr(start), _ptr(end), len(iv), C.byref(h)),
                  "sid_regions_from_intervals")
        self.h = h

    def _handle(self):
        if not self.h:
            raise SidError(1, "regions: the object is closed")
        return self.h

    def contains(self, chrom, pos: int) -> bool:
        c = chrom if isinstance(chrom, bytes) else str(chrom).encode()
        if not -2**31 <= int(pos) < 2**31:
            return False
        return bool(lib().sid_regions_contains(self._handle(), c, len(c), int(pos)))

    def __len__(self):
        """The intervals after the merge."""
        return int(lib().sid_regions_intervals(self._handle()))

    @property
    def chroms(self) -> int:
        return int(lib().sid_regions_chroms(self._handle()))

    def interval(self, j: int) -> tuple:
        """sid_regions_interval: (chrom bytes, start, end) of merged interval j
        in row order -- the chroms by their first non-empty interval in the
        source, a chrom's intervals ascending."""
        chrom, clen, start, end = C.c_void_p(), C.c_uint32(0), C.c_int64(0), C.c_int64(0)
        check(lib().sid_regions_interval(self._handle(), int(j), C.byref(chrom), C.byref(clen), C.byref(start),
                                         C.byref(end)), "sid_regions_interval")
        return (C.string_at(chrom.value, clen.value) if clen.value else b"", start.value, end.value)

    def region_stats_valid(self) -> bool:
        """sid_region_stats_valid: the region rows can be switched on for the set."""
        return lib().sid_region_stats_valid(self._handle()) == SID_OK

    def close(self):
        if getattr(self, "h", None) and _LIB is not None:
            _LIB.sid_regions_free(self.h)
        self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def make_opts(method="local", estimate_prior=False, snp_prior=-1.0, significance_level=0.05,
              site_error_threshold=0.1, select="all", regions=None, context=0, window=0, variants=0) -> Opts:
    o = Opts()
    lib().sid_opts_default(C.byref(o))
    o.method = METHODS[method] if isinstance(method, str) else int(method)
    o.estimate_prior = int(bool(estimate_prior))
    o.snp_prior = float(snp_prior)
    o.significance_level = float(significance_level)
    o.site_error_threshold = float(site_error_threshold)
    if isinstance(select, str) and select not in SELECT:
        raise SidError(1, f"select: expected one of {sorted(SELECT)}, got {select!r}")
    o.select = SELECT[select] if isinstance(select, str) else int(select)
    if regions is not None and not isinstance(regions, Regions):
        raise SidError(1, f"regions: expected a Regions object or None, got {type(regions).__name__}")
    # (the pointer alone: sid_create / sid_engine_create copy the set, and the
    # caller keeps the Regions object until then)
    o.regions = regions._handle() if regions is not None else None
    # (0 .. 64: sid_create / sid_engine_create return SID_EINVAL for another value)
    o.context = int(context)
    # (0 = off, 1 .. 2^31-1: a negative value is SID_EINVAL there too)
    o.window = int(window)
    # (0 or 1, True / False: another value is SID_EINVAL there too)
    o.variants = int(variants)
    return o


def _window_rows(rows, n: int) -> list:
    """sid_window rows as tuples (chrom, start, end, sites, records, het, hom)."""
    out = []
    for k in range(n):
        r = rows[k]
        chrom = C.string_at(r.chrom, r.chrom_len) if r.chrom_len else b""
        out.append((chrom, r.start, r.end, r.sites, r.records, r.het, r.hom))
    return out


def windows_host(sites: "Sites", code_all: np.ndarray, window: int, begin: int = 0, end: int = None) -> list:
    """sid_windows_host: the rows of the windowed summary of sites [begin, end)
    from their codes before any selection marked them."""
    code_all = np.ascontiguousarray(code_all, np.uint8)
    if end is None:
        end = len(sites)
    if code_all.size != len(sites):
        raise SidError(1, "windows_host: one code per site")
    rows, n = C.POINTER(Window)(), C.c_size_t(0)
    check(lib().sid_windows_host(sites.handle, begin, end, _ptr(code_all), int(window), C.byref(rows), C.byref(n)),
          "sid_windows_host")
    try:
        return _window_rows(rows, n.value)
    finally:
        lib().sid_windows_free(rows)


def windows_format(rows, header: bool = True) -> bytes:
    """sid_windows_format over rows as windows_host / Engine.windows return them."""
    rows = list(rows)
    arr = (Window * max(len(rows), 1))()
    keep = []
    for k, (chrom, start, end, sites, records, het, hom) in enumerate(rows):
        b = C.create_string_buffer(bytes(chrom), len(chrom))
        keep.append(b)
        arr[k] = Window(C.cast(b, C.c_void_p).value if len(chrom) else None, len(chrom), start, end, sites, records,
                        het, hom)
    n = C.c_size_t(0)
    st = lib().sid_windows_format(arr, len(rows), int(bool(header)), None, 0, C.byref(n))
    if st not in (SID_OK, 3):
        check(st, "sid_windows_format")
    buf = C.create_string_buffer(max(n.value, 1))
    check(lib().sid_windows_format(arr, len(rows), int(bool(header)), buf, n.value, C.byref(n)),
          "sid_windows_format")
    return buf.raw[:n.value]


def dtext_windows(ctx: "Context", dtext: "DText", code_ptr, begin: int = 0, end: int = None, stream=None) -> list:
    """sid_dtext_windows: the window stage over sites [begin, end) of a
    resident shard with the given device codes (the context's `window`)."""
    if end is None:
        end = len(dtext)
    rows, n = C.POINTER(Window)(), C.c_size_t(0)
    check(lib().sid_dtext_windows(ctx.h, dtext.h, begin, end, code_ptr, C.byref(rows), C.byref(n), stream),
          "sid_dtext_windows")
    try:
        return _window_rows(rows, n.value)
    finally:
        lib().sid_windows_free(rows)


def _depth_rows(rows, n: int) -> list:
    """sid_depth_row rows as tuples (depth, sites, records, het, hom)."""
    return [(rows[k].depth, rows[k].sites, rows[k].records, rows[k].het, rows[k].hom) for k in range(n)]


def _depth_array(rows):
    rows = list(rows)
    arr = (DepthRow * max(len(rows), 1))()
    for k, (depth, sites, records, het, hom) in enumerate(rows):
        arr[k] = DepthRow(sites, records, het, hom, depth, 0)
    return arr, len(rows)


def depth_hist_host(sites: "Sites", code_all: np.ndarray, begin: int = 0, end: int = None) -> list:
    """sid_depth_hist_host: the rows of the depth histogram of sites [begin, end)
    from their codes before any selection marked them."""
    code_all = np.ascontiguousarray(code_all, np.uint8)
    if end is None:
        end = len(sites)
    if code_all.size != len(sites):
        raise SidError(1, "depth_hist_host: one code per site")
    rows, n = C.POINTER(DepthRow)(), C.c_size_t(0)
    check(lib().sid_depth_hist_host(sites.handle, begin, end, _ptr(code_all), C.byref(rows), C.byref(n)),
          "sid_depth_hist_host")
    try:
        return _depth_rows(rows, n.value)
    finally:
        lib().sid_depth_hist_free(rows)


def depth_hist_format(rows, header: bool = True) -> bytes:
    """sid_depth_hist_format over rows as depth_hist_host / Engine.depth_hist return them."""
    arr, m = _depth_array(rows)
    n = C.c_size_t(0)
    st = lib().sid_depth_hist_format(arr, m, int(bool(header)), None, 0, C.byref(n))
    if st not in (SID_OK, 3):
        check(st, "sid_depth_hist_format")
    buf = C.create_string_buffer(max(n.value, 1))
    check(lib().sid_depth_hist_format(arr, m, int(bool(header)), buf, n.value, C.byref(n)), "sid_depth_hist_format")
    return buf.raw[:n.value]


def depth_hist_merge(a, b) -> list:
    """sid_depth_hist_merge: the sum of two row sets (ranks that took site
    ranges add their rows with it); both strictly ascending in depth."""
    aa, na = _depth_array(a)
    ab, nb = _depth_array(b)
    rows, n = C.POINTER(DepthRow)(), C.c_size_t(0)
    check(lib().sid_depth_hist_merge(aa, na, ab, nb, C.byref(rows), C.byref(n)), "sid_depth_hist_merge")
    try:
        return _depth_rows(rows, n.value)
    finally:
        lib().sid_depth_hist_free(rows)


def dtext_depth_hist(ctx: "Context", dtext: "DText", code_ptr, begin: int = 0, end: int = None, stream=None) -> list:
    """sid_dtext_depth_hist: the histogram's stage over sites [begin, end) of a
    resident shard with the given device codes."""
    if end is None:
        end = len(dtext)
    rows, n = C.POINTER(DepthRow)(), C.c_size_t(0)
    check(lib().sid_dtext_depth_hist(ctx.h, dtext.h, begin, end, code_ptr, C.byref(rows), C.byref(n), stream),
          "sid_dtext_depth_hist")
    try:
        return _depth_rows(rows, n.value)
    finally:
        lib().sid_depth_hist_free(rows)


def _region_rows(rows, n: int) -> list:
    """sid_region_row rows as tuples (chrom, start, end, sites, depth, records, het, hom)."""
    out = []
    for k in range(n):
        r = rows[k]
        chrom = C.string_at(r.chrom, r.chrom_len) if r.chrom_len else b""
        out.append((chrom, r.start, r.end, r.sites, r.depth, r.records, r.het, r.hom))
    return out


def _region_array(rows):
    """(array, n, keep-alive list of the chrom buffers)"""
    rows = list(rows)
    arr = (RegionRow * max(len(rows), 1))()
    keep = []
    for k, (chrom, start, end, sites, depth, records, het, hom) in enumerate(rows):
        c = chrom if isinstance(chrom, bytes) else str(chrom).encode()
        b = C.create_string_buffer(c, max(len(c), 1))
        keep.append(b)
        arr[k] = RegionRow(C.cast(b, C.c_void_p), len(c), start, end, sites, depth, records, het, hom)
    return arr, len(rows), keep


def region_stats_host(regions: "Regions", sites: "Sites", code_all: np.ndarray, begin: int = 0, end: int = None) -> list:
    """sid_region_stats_host: the region rows of sites [begin, end) from their
    codes before any selection marked them, one per interval of the set."""
    code_all = np.ascontiguousarray(code_all, np.uint8)
    if end is None:
        end = len(sites)
    if code_all.size != len(sites):
        raise SidError(1, "region_stats_host: one code per site")
    rows, n = C.POINTER(RegionRow)(), C.c_size_t(0)
    check(lib().sid_region_stats_host(regions._handle(), sites.handle, begin, end, _ptr(code_all), C.byref(rows),
                                      C.byref(n)), "sid_region_stats_host")
    try:
        return _region_rows(rows, n.value)
    finally:
        lib().sid_region_stats_free(rows)


def region_stats_format(rows, header: bool = True) -> bytes:
    """sid_region_stats_format over rows as region_stats_host / Engine.region_stats return them."""
    arr, m, _keep = _region_array(rows)
    n = C.c_size_t(0)
    st = lib().sid_region_stats_format(arr, m, int(bool(header)), None, 0, C.byref(n))
    if st not in (SID_OK, 3):
        check(st, "sid_region_stats_format")
    buf = C.create_string_buffer(max(n.value, 1))
    check(lib().sid_region_stats_format(arr, m, int(bool(header)), buf, n.value, C.byref(n)), "sid_region_stats_format")
    return buf.raw[:n.value]


def region_stats_merge(a, b) -> list:
    """sid_region_stats_merge: the elementwise sum of two row lists over the same
    set (ranks that took site ranges add their rows with it); SidError when the
    lists' lengths or keys differ."""
    aa, na, _ka = _region_array(a)
    ab, nb, _kb = _region_array(b)
    if na != nb:
        raise SidError(1, "region_stats_merge: the lists differ in length")
    rows = C.POINTER(RegionRow)()
    check(lib().sid_region_stats_merge(aa, ab, na, C.byref(rows)), "sid_region_stats_merge")
    try:
        return _region_rows(rows, na)
    finally:
        lib().sid_region_stats_free(rows)


def dtext_region_stats(ctx: "Context", dtext: "DText", code_ptr, begin: int = 0, end: int = None, stream=None) -> list:
    """sid_dtext_region_stats: the region rows' stage over sites [begin, end) of
    a resident shard with the given device codes, for the context's region set."""
    if end is None:
        end = len(dtext)
    rows, n = C.POINTER(RegionRow)(), C.c_size_t(0)
    check(lib().sid_dtext_region_stats(ctx.h, dtext.h, begin, end, code_ptr, C.byref(rows), C.byref(n), stream),
          "sid_dtext_region_stats")
    try:
        return _region_rows(rows, n.value)
    finally:
        lib().sid_region_stats_free(rows)


def _callable_rows(rows, n: int) -> list:
    """sid_callable_row rows as tuples (chrom bytes, start, end, het)."""
    return [(C.string_at(rows[k].chrom, rows[k].chrom_len) if rows[k].chrom_len else b"",
             rows[k].start, rows[k].end, rows[k].het) for k in range(n)]


def _callable_array(rows):
    """(array, count, the chroms' buffers kept alive) of tuples (chrom, start, end, het)."""
    rows = list(rows)
    arr = (CallableRow * max(len(rows), 1))()
    keep = []
    for k, (chrom, start, end, het) in enumerate(rows):
        buf = C.create_string_buffer(bytes(chrom), max(len(chrom), 1))
        keep.append(buf)
        arr[k] = CallableRow(C.cast(buf, C.c_void_p).value, len(chrom), 0, start, end, het)
    return arr, len(rows), keep


def callable_host(sites: "Sites", code_all: np.ndarray, min_depth: int = 0, max_depth: int = 0,
                  begin: int = 0, end: int = None) -> list:
    """sid_callable_host: the callable runs of sites [begin, end) from their
    codes before any selection marked them, under the depth bounds."""
    code_all = np.ascontiguousarray(code_all, np.uint8)
    if end is None:
        end = len(sites)
    if code_all.size != len(sites):
        raise SidError(1, "callable_host: one code per site")
    rows, n = C.POINTER(CallableRow)(), C.c_size_t(0)
    check(lib().sid_callable_host(sites.handle, begin, end, _ptr(code_all), min_depth, max_depth, C.byref(rows),
                                  C.byref(n)), "sid_callable_host")
    try:
        return _callable_rows(rows, n.value)
    finally:
        lib().sid_callable_free(rows)


def callable_format(rows) -> bytes:
    """sid_callable_format over rows as callable_host / dtext_callable return them."""
    arr, m, keep = _callable_array(rows)
    n = C.c_size_t(0)
    st = lib().sid_callable_format(arr, m, None, 0, C.byref(n))
    if st not in (SID_OK, 3):
        check(st, "sid_callable_format")
    buf = C.create_string_buffer(max(n.value, 1))
    check(lib().sid_callable_format(arr, m, buf, n.value, C.byref(n)), "sid_callable_format")
    del keep
    return buf.raw[:n.value]


def callable_join(a, b, a_open_end: bool, b_open_start: bool) -> list:
    """sid_callable_join: two row lists that are neighbours in file order (ranks
    that took site ranges); the boundary rows merge only when both flags are
    set, the chroms are equal and b's start is a's end."""
    aa, na, ka = _callable_array(a)
    ab, nb, kb = _callable_array(b)
    rows, n = C.POINTER(CallableRow)(), C.c_size_t(0)
    check(lib().sid_callable_join(aa, na, int(bool(a_open_end)), ab, nb, int(bool(b_open_start)), C.byref(rows),
                                  C.byref(n)), "sid_callable_join")
    del ka, kb
    try:
        return _callable_rows(rows, n.value)
    finally:
        lib().sid_callable_free(rows)


def dtext_callable(ctx: "Context", dtext: "DText", code_ptr, begin: int = 0, end: int = None, stream=None) -> list:
    """sid_dtext_callable: the callable stage over sites [begin, end) of a
    resident shard with the given device codes, under the context's depth bounds."""
    if end is None:
        end = len(dtext)
    rows, n = C.POINTER(CallableRow)(), C.c_size_t(0)
    check(lib().sid_dtext_callable(ctx.h, dtext.h, begin, end, code_ptr, C.byref(rows), C.byref(n), stream),
          "sid_dtext_callable")
    try:
        return _callable_rows(rows, n.value)
    finally:
        lib().sid_callable_free(rows)


def device_count() -> int:
    n = C.c_int(0)
    st = lib().sid_device_count(C.byref(n))
    return n.value if st == SID_OK else 0


# --------------------------------------------------------------- host side --
@dataclass
class Sites:
    counts: np.ndarray          # (n, 4) uint16, A C G T
    positions: np.ndarray       # (n,) int32
    chroms: list                # [(start_site, name)]
    handle: object = None       # sid_sites* kept for format_csv
    refs: np.ndarray = None     # (n,) uint8: the reference base of every site, the byte of its third column

    def __len__(self):
        return len(self.positions)

    def __del__(self):
        if self.handle is not None and _LIB is not None:
            _LIB.sid_sites_free(self.handle)
            self.handle = None


def parse_text(text: bytes, threads: int = 0) -> Sites:
    """sid_parse_text: pileup text -> SoA (pileup.cpp:13-153 semantics)."""
    L = lib()
    h = C.c_void_p()
    bad = C.c_uint64(0)
    st = L.sid_parse_text(text, len(text), threads, C.byref(h), C.byref(bad))
    if st != SID_OK:
        err = SidError(st, "parse")
        err.line = bad.value
        raise err
    n = L.sid_sites_count(h)
    counts = np.ctypeslib.as_array(C.cast(L.sid_sites_counts(h), C.POINTER(C.c_uint16)),
                                   shape=(n * 4,)).reshape(n, 4).copy() if n else np.zeros((0, 4), np.uint16)
    pos = np.ctypeslib.as_array(C.cast(L.sid_sites_positions(h), C.POINTER(C.c_int32)),
                                shape=(n,)).copy() if n else np.zeros(0, np.int32)
    chroms = []
    for k in range(L.sid_sites_chrom_segments(h)):
        start = C.c_uint64(0)
        name = L.sid_sites_chrom_name(h, k, C.byref(start))
        chroms.append((start.value, name))
    refs = np.ctypeslib.as_array(C.cast(L.sid_sites_refs(h), C.POINTER(C.c_uint8)),
                                 shape=(n,)).copy() if n else np.zeros(0, np.uint8)
    return Sites(counts, pos, chroms, h, refs)


def format_csv(sites: Sites, code: np.ndarray, hom: np.ndarray, het: np.ndarray,
               conf_type: str = "p_value", begin: int = 0, end: int = None) -> bytes:
    L = lib()
    code = np.ascontiguousarray(code, np.uint8)
    hom = np.ascontiguousarray(hom, np.float64)
    het = np.ascontiguousarray(het, np.float64)
    need = C.c_size_t(0)
    n = len(sites) if end is None else end
    L.sid_format_csv(sites.handle, begin, n, _ptr(code), _ptr(hom), _ptr(het), conf_type.encode(),
                     None, 0, C.byref(need))
    buf = C.create_string_buffer(max(need.value, 1))
    ln = C.c_size_t(0)
    check(L.sid_format_csv(sites.handle, begin, n, _ptr(code), _ptr(hom), _ptr(het), conf_type.encode(),
                           buf, need.value, C.byref(ln)), "format")
    return buf.raw[: ln.value]


def format_vcf(sites: Sites, code: np.ndarray, hom: np.ndarray, het: np.ndarray, begin: int = 0,
               end: int = None) -> bytes:
    """sid_format_vcf: the records format_csv prints, as VCF lines (REF from the
    sites' reference bytes, DP from their counts), without the header."""
    L = lib()
    code = np.ascontiguousarray(code, np.uint8)
    hom = np.ascontiguousarray(hom, np.float64)
    het = np.ascontiguousarray(het, np.float64)
    need = C.c_size_t(0)
    n = len(sites) if end is None else end
    st = L.sid_format_vcf(sites.handle, begin, n, _ptr(code), _ptr(hom), _ptr(het), None, 0, C.byref(need))
    if st not in (SID_OK, 3):
        check(st, "sid_format_vcf")
    buf = C.create_string_buffer(max(need.value, 1))
    ln = C.c_size_t(0)
    check(L.sid_format_vcf(sites.handle, begin, n, _ptr(code), _ptr(hom), _ptr(het), buf, need.value,
                           C.byref(ln)), "sid_format_vcf")
    return buf.raw[: ln.value]


def vcf_header(method="local", **opts) -> bytes:
    """sid_vcf_header: the VCF header of a run with these options."""
    o = make_opts(method=method, **opts)
    need = C.c_size_t(0)
    st = lib().sid_vcf_header(C.byref(o), None, 0, C.byref(need))
    if st not in (SID_OK, 3):
        check(st, "sid_vcf_header")
    buf = C.create_string_buffer(max(need.value, 1))
    check(lib().sid_vcf_header(C.byref(o), buf, need.value, C.byref(need)), "sid_vcf_header")
    return buf.raw[: need.value]


def select_mark(code: np.ndarray, select="all") -> np.ndarray:
    """sid_select_mark on a copy of the codes: the sites whose label is not
    `select` get SID_CODE_DROPPED, so format_csv skips them."""
    out = np.array(code, np.uint8, copy=True)
    if isinstance(select, str) and select not in SELECT:
        raise SidError(1, f"select: expected one of {sorted(SELECT)}, got {select!r}")
    check(lib().sid_select_mark(_ptr(out), out.size, SELECT[select] if isinstance(select, str) else int(select)),
          "sid_select_mark")
    return out


def context_mark(code_all: np.ndarray, code: np.ndarray, context: int) -> np.ndarray:
    """sid_context_mark on a copy of `code` (the codes after select_mark /
    regions_mark; code_all: the codes before them): every record within
    `context` records of a selected one gets its record back."""
    src = np.ascontiguousarray(code_all, dtype=np.uint8)
    out = np.ascontiguousarray(code, dtype=np.uint8).copy()
    if src.size != out.size:
        raise SidError(1, "context_mark: one code of each array per site")
    check(lib().sid_context_mark(_ptr(src), _ptr(out), out.size, int(context)), "sid_context_mark")
    return out


def regions_mark(sites: Sites, code: np.ndarray, regions) -> np.ndarray:
    """sid_regions_mark on a copy of the codes: the sites outside `regions`
    get SID_CODE_DROPPED, so format_csv skips them (None: every site stays)."""
    out = np.array(code, np.uint8, copy=True)
    if regions is not None and not isinstance(regions, Regions):
        raise SidError(1, f"regions: expected a Regions object or None, got {type(regions).__name__}")
    if out.size != len(sites):
        raise SidError(1, "regions_mark: one code per site")
    check(lib().sid_regions_mark(regions._handle() if regions is not None else None, sites.handle, 0, out.size,
                                 _ptr(out)), "sid_regions_mark")
    return out


def variants_mark(sites: Sites, code: np.ndarray, begin: int = 0, end: int = None) -> np.ndarray:
    """sid_variants_mark on a copy of the codes: the sites of [begin, end) whose
    record is no variant -- a reference base that is none of A, C, G, T, no
    counted base, or a genotype that is the reference's twice -- get
    SID_CODE_DROPPED, so format_csv skips them.  After select_mark /
    regions_mark or before them (they commute), before context_mark."""
    out = np.array(code, np.uint8, copy=True)
    if out.size != len(sites):
        raise SidError(1, "variants_mark: one code per site")
    check(lib().sid_variants_mark(sites.handle, int(begin), out.size if end is None else int(end), _ptr(out)),
          "sid_variants_mark")
    return out


def depth_mark(sites: Sites, code: np.ndarray, min_depth: int, max_depth: int, begin: int = 0,
               end: int = None) -> np.ndarray:
    """sid_depth_mark on a copy of the codes: the sites of [begin, end) whose
    depth -- the sum of their four counts -- is below min_depth or, with
    max_depth != 0, above max_depth get SID_CODE_DROPPED, so format_csv skips
    them.  After select_mark / regions_mark / variants_mark, before
    context_mark."""
    out = np.array(code, np.uint8, copy=True)
    if out.size != len(sites):
        raise SidError(1, "depth_mark: one code per site")
    check(lib().sid_depth_mark(sites.handle, int(begin), out.size if end is None else int(end), int(min_depth),
                               int(max_depth), _ptr(out)), "sid_depth_mark")
    return out


def format_double(v: float) -> str:
    buf = C.create_string_buffer(48)
    k = lib().sid_format_double(float(v), buf, 48)
    return buf.value.decode()


def format_g6(v: float) -> str:
    """The device formatter's %g (fmt.h), host build."""
    buf = C.create_string_buffer(48)
    k = lib().sid_format_g6(float(v), buf, 48)
    if k < 0:
        raise SidError(-k, "format_g6")
    return buf.value.decode()


class DText:
    """One shard of pileup text parsed on the device (sid_dtext_*)."""

    def __init__(self, ctx: "Context", text: bytes = None, chunk: int = 0, stream=None, fd: int = None,
                 offset: int = 0, length: int = None, threads: int = 0):
        self.ctx = ctx
        h = C.c_void_p()
        off = C.c_uint64(0)
        if fd is not None:   # bytes [offset, offset+length) of an open file
            rc = lib().sid_dtext_parse_fd(ctx.h, fd, offset, length, threads, C.byref(h), C.byref(off), stream)
        else:
            buf = C.c_char_p(text)
            rc = lib().sid_dtext_parse(ctx.h, C.cast(buf, C.c_void_p), len(text), chunk, C.byref(h), C.byref(off),
                                       stream)
        if rc != 0:
            err = SidError(rc, "sid_dtext_parse")
            err.offset = off.value   # byte offset of the first malformed line
            raise err
        self.h = h

    def __len__(self):
        return lib().sid_dtext_count(self.h)

    @property
    def counts_ptr(self):
        return lib().sid_dtext_counts(self.h)

    def format(self, code_ptr, hom_ptr, het_ptr, conf_type="p_value", begin=0, end=None, stream=None) -> bytes:
        end = len(self) if end is None else end
        parts = []

        def w(_user, data, n):
            parts.append(C.string_at(data, n))
            return 0
        cb = WRITE_FN(w)
        check(lib().sid_dtext_format(self.ctx.h, self.h, begin, end, code_ptr, hom_ptr, het_ptr,
                                     conf_type.encode(), cb, None, stream), "sid_dtext_format")
        return b"".join(parts)

    def close(self):
        if getattr(self, "h", None):
            lib().sid_dtext_free(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def synth_text(seed: int, n: int, depth: float = 30.0, first: int = 0,
               sites_per_chrom: int = 0, mapq: bool = False) -> bytes:
    """Synthetic pileup text; mapq=True adds the 7th (mapping quality) column."""
    L = lib()
    fn = L.sid_synth_text_mq if mapq else L.sid_synth_text
    ln = C.c_size_t(0)
    check(fn(seed, depth, first, n, sites_per_chrom, None, 0, C.byref(ln)), "synth")
    buf = C.create_string_buffer(max(ln.value, 1))
    check(fn(seed, depth, first, n, sites_per_chrom, buf, ln.value, C.byref(ln)), "synth")
    return buf.raw[: ln.value]


def synth_counts_host(seed: int, n: int, depth: float = 30.0, first: int = 0) -> np.ndarray:
    out = np.zeros((n, 4), np.uint16)
    check(lib().sid_synth_counts_host(seed, depth, first, n, _ptr(out)), "synth")
    return out


# -------------------------------------------------------------- BGZF input --
def _bgzf_error(st: int, what: str, off: int):
    err = SidError(st, what)
    err.offset = off   # SID_EBGZF: the bad member's compressed offset
    return err


class BgzfIndex:
    """The block index of a BGZF byte range (sid_bgzf_index)."""

    def __init__(self, data: bytes):
        self.h = None
        self.data = bytes(data)
        h, off = C.c_void_p(), C.c_uint64(0)
        st = lib().sid_bgzf_index(self.data, len(self.data), C.byref(h), C.byref(off))
        if st != SID_OK:
            raise _bgzf_error(st, "sid_bgzf_index", off.value)
        self.h = h

    def __len__(self):
        return int(lib().sid_bgzf_blocks(self.h))

    @property
    def text_len(self) -> int:
        return int(lib().sid_bgzf_text_len(self.h))

    def block(self, k: int):
        """(compressed offset, compressed size, text offset, text size) of member k."""
        coff, csize, toff, isize = C.c_uint64(0), C.c_uint32(0), C.c_uint64(0), C.c_uint32(0)
        check(lib().sid_bgzf_block(self.h, k, C.byref(coff), C.byref(csize), C.byref(toff), C.byref(isize)),
              "sid_bgzf_block")
        return coff.value, csize.value, toff.value, isize.value

    def blocks(self):
        return [self.block(k) for k in range(len(self))]

    def close(self):
        if getattr(self, "h", None) and _LIB is not None:
            _LIB.sid_bgzf_free(self.h)
        self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def bgzf_index(data: bytes):
    """The members of a BGZF byte range as (compressed offset, compressed
    size, text offset, text size) tuples; SidError (SID_EBGZF, .offset) when
    the bytes are not BGZF."""
    z = BgzfIndex(data)
    try:
        return z.blocks()
    finally:
        z.close()


def bgzf_inflate_host(data: bytes) -> bytes:
    """sid_bgzf_inflate_host: every member inflated and CRC-checked on the host."""
    data = bytes(data)
    L = lib()
    n, off = C.c_size_t(0), C.c_uint64(0)
    st = L.sid_bgzf_inflate_host(data, len(data), None, 0, C.byref(n), C.byref(off))
    if st != SID_OK:
        raise _bgzf_error(st, "sid_bgzf_inflate_host", off.value)
    buf = C.create_string_buffer(max(n.value, 1))
    st = L.sid_bgzf_inflate_host(data, len(data), buf, n.value, C.byref(n), C.byref(off))
    if st != SID_OK:
        raise _bgzf_error(st, "sid_bgzf_inflate_host", off.value)
    return buf.raw[: n.value]


def bgzf_inflate_device(ctx: "Context", d_bytes, index: BgzfIndex, d_out, cap: int = None, first_block: int = 0,
                        nblocks: int = None, stream=None):
    """sid_bgzf_inflate_device: members [first_block, first_block + nblocks)
    of the indexed range in device memory (a torch uint8 tensor or a raw
    device pointer) inflated into d_out (likewise; cap bytes, a tensor's size
    by default).  SidError (SID_EBGZF) carries .block, the lowest bad member."""
    def ptr(t):
        return t if isinstance(t, int) or t is None else t.data_ptr()
    if nblocks is None:
        nblocks = len(index) - first_block
    if cap is None:
        cap = d_out.numel() * d_out.element_size()
    bad = C.c_uint64(0)
    st = lib().sid_bgzf_inflate_device(ctx.h, ptr(d_bytes), index.h, first_block, nblocks, ptr(d_out), cap,
                                       C.byref(bad), stream)
    if st != SID_OK:
        err = SidError(st, "sid_bgzf_inflate_device")
        err.block = bad.value
        raise err


def crc32(data: bytes, crc: int = 0) -> int:
    """sid_crc32: zlib.crc32 by the host build of the device routine."""
    data = bytes(data)
    return int(lib().sid_crc32(crc, data, len(data)))


# ------------------------------------------------------------- device side --
class Context:
    """One sid_ctx (one device, one host thread)."""

    def __init__(self, device: int = 0, min_depth: int = 0, max_depth: int = 0, format="csv", **opts):
        fmt = _format(format)
        self.opts = make_opts(**opts)
        self.device = device
        h = C.c_void_p()
        check(lib().sid_create(device, C.byref(self.opts), C.byref(h)), "sid_create")
        self.opts.regions = None   # (the context holds its own copy of the set)
        self.h = h
        if min_depth or max_depth:   # (the depth bounds are no field of sid_opts)
            self.set_depth(min_depth, max_depth)
        if fmt:                      # (nor is the record format)
            self.set_format(fmt)

    @classmethod
    def wrap(cls, handle, device: int = 0):
        """A non-owning view of a context another object owns (e.g. an engine's)."""
        c = cls.__new__(cls)
        c.opts, c.device, c.h, c._borrowed = None, device, C.c_void_p(handle), True
        return c

    def close(self):
        if getattr(self, "h", None) and not getattr(self, "_borrowed", False):
            lib().sid_destroy(self.h)
        self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_prior(self, prior: float):
        check(lib().sid_set_prior(self.h, float(prior)), "sid_set_prior")

    def set_depth(self, min_depth: int, max_depth: int):
        """The depth bounds of every formatter call from now on (0, 0: none)."""
        check(lib().sid_set_depth(self.h, int(min_depth), int(max_depth)), "sid_set_depth")

    def set_format(self, format):
        """The record format ("csv" / "vcf", or SID_FORMAT_*) of every formatter call from now on."""
        check(lib().sid_set_format(self.h, _format(format)), "sid_set_format")

    # raw device-pointer entry points -------------------------------------
    def call_local(self, counts_ptr, n, code_ptr, hom_ptr, het_ptr, stream=None):
        check(lib().sid_call_local(self.h, counts_ptr, n, code_ptr, hom_ptr, het_ptr, stream),
              "sid_call_local")

    def timing_enable(self, on=True):
        check(lib().sid_timing_enable(self.h, int(bool(on))), "sid_timing_enable")

    def timing_read(self):
        """(calls, main kernel ms, fix-up kernel ms) averaged since the last read."""
        k, m, f = C.c_uint64(0), C.c_double(0), C.c_double(0)
        check(lib().sid_timing_read(self.h, C.byref(k), C.byref(m), C.byref(f)), "sid_timing_read")
        return k.value, m.value, f.value

    def lookup_sites(self, counts_ptr, n, code_ptr, hom_ptr, het_ptr, stream=None):
        check(lib().sid_lookup_sites(self.h, counts_ptr, n, code_ptr, hom_ptr, het_ptr, stream),
              "sid_lookup_sites")

    def profile_reset(self, stream=None):
        check(lib().sid_profile_reset(self.h, stream), "sid_profile_reset")

    def profile_accumulate(self, counts_ptr, n, stream=None):
        check(lib().sid_profile_accumulate(self.h, counts_ptr, n, stream), "sid_profile_accumulate")

    def profile_table(self):
        u = C.c_size_t(0)
        check(lib().sid_profile_table(self.h, None, None, 0, C.byref(u)), "sid_profile_table")
        keys = np.zeros(u.value, np.uint64)
        cnts = np.zeros(u.value, np.uint64)
        if u.value:
            check(lib().sid_profile_table(self.h, _ptr(keys), _ptr(cnts), u.value, C.byref(u)),
                  "sid_profile_table")
        return keys, cnts

    def profile_load(self, keys: np.ndarray, cnts: np.ndarray):
        keys = np.ascontiguousarray(keys, np.uint64)
        cnts = np.ascontiguousarray(cnts, np.uint64)
        check(lib().sid_profile_load(self.h, _ptr(keys), _ptr(cnts), len(keys)), "sid_profile_load")

    def lynch_setup(self) -> Estimate:
        e = Estimate()
        check(lib().sid_lynch_setup(self.h, C.byref(e)), "sid_lynch_setup")
        return e

    def lynch_objective(self, pi: float, eps: float) -> float:
        out = C.c_double(0)
        check(lib().sid_lynch_objective(self.h, pi, eps, C.byref(out)), "sid_lynch_objective")
        return out.value

    def lynch_prepare(self, verbose: bool = False) -> Estimate:
        e = Estimate()
        check(lib().sid_lynch_prepare(self.h, int(verbose), C.byref(e)), "sid_lynch_prepare")
        return e

    def synth_counts(self, seed, depth, first, n, counts_ptr, stream=None):
        check(lib().sid_synth_counts(self.h, seed, depth, first, n, counts_ptr, stream),
              "sid_synth_counts")

    def synth_text_device(self, seed, depth, first, n, out_ptr, cap, sites_per_chrom=0, stream=None) -> int:
        """The generator's text written on the device (sid_synth_text_device); returns its bytes."""
        ln = C.c_size_t(0)
        check(lib().sid_synth_text_device(self.h, seed, depth, first, n, sites_per_chrom, out_ptr, cap,
                                          C.byref(ln), stream), "sid_synth_text_device")
        return ln.value


HEADER = b"chrom,pos,label,gt,hom_conf,het_conf,conf_type\n"

STRIP_AUTO, STRIP_SCALAR, STRIP_AVX2, STRIP_AVX512 = 0, 1, 2, 3


def strip_lines(text: bytes, impl: int = STRIP_AUTO, align: int = 0):
    """sid_strip_lines_impl: (the text without its quality columns, its lines),
    or None when this CPU does not run the variant.  align: the input's first
    byte sits that many bytes past a 64-B boundary."""
    n = len(text)
    raw = C.create_string_buffer(n + 128)
    base = C.addressof(raw)
    src = (base + 63) // 64 * 64 + align % 64
    C.memmove(src, text, n)
    out = C.create_string_buffer(max(n, 1))
    lines = C.c_uint64(0)
    m = lib().sid_strip_lines_impl(impl, src, n, out, n, C.byref(lines))
    if m == C.c_size_t(-1).value:
        return None
    return out.raw[:m], lines.value


def strip_impl() -> int:
    """The variant STRIP_AUTO stands for on this CPU."""
    return lib().sid_strip_impl()


def strip_map(text: bytes, out_off: int) -> int:
    """sid_strip_map: the input offset of the stripped text's byte out_off."""
    return lib().sid_strip_map(text, len(text), out_off)


class Engine:
    """The streaming engine (sid_engine_*): pileup text in, CSV out, in
    line-aligned chunks over one or more devices."""

    def __init__(self, method="local", devices=1, first_device=0, chunk_bytes=0, slots=0, hold_bytes=0,
                 retain_bytes=0, host_threads=0, verbose=False, device_sink=False, lanes=0, host_hold_bytes=0,
                 min_depth=0, max_depth=0, format="csv", depth_hist=False, region_stats=False, strip=0, **opts):
        fmt = _format(format)
        self.opts = make_opts(method=method, **opts)
        cfg = EngineCfg()
        lib().sid_engine_cfg_default(C.byref(cfg))
        cfg.devices, cfg.first_device, cfg.chunk_bytes, cfg.slots = devices, first_device, chunk_bytes, slots
        cfg.hold_bytes, cfg.retain_bytes, cfg.host_threads = hold_bytes, retain_bytes, host_threads
        cfg.verbose, cfg.device_sink, cfg.lanes = int(bool(verbose)), int(device_sink), lanes
        cfg.host_hold_bytes = host_hold_bytes
        cfg.strip = int(strip)
        self.cfg = cfg
        h = C.c_void_p()
        check(lib().sid_engine_create(C.byref(self.opts), C.byref(cfg), C.byref(h)), "sid_engine_create")
        self.opts.regions = None   # (every pipeline's context holds its own copy of the set)
        self.h = h
        self._keep = None
        if min_depth or max_depth:   # (the depth bounds are no field of sid_opts)
            self.set_depth(min_depth, max_depth)
        if fmt:                      # (nor is the record format)
            self.set_format(fmt)
        if depth_hist:               # (nor the depth histogram's switch)
            self.set_depth_hist(True)
        if region_stats:             # (nor the region rows')
            try:
                self.set_region_stats(True)
            except Exception:
                self.close()
                raise

    def close(self):
        if getattr(self, "h", None):
            lib().sid_engine_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def context(self, i=0):
        return lib().sid_engine_context(self.h, i)

    def set_depth(self, min_depth: int, max_depth: int):
        """The depth bounds of every run from now on (0, 0: none); SID_ESTATE
        between an ingest and its emit."""
        check(lib().sid_engine_set_depth(self.h, int(min_depth), int(max_depth)), "sid_engine_set_depth")

    def set_format(self, format):
        """The record format ("csv" / "vcf", or SID_FORMAT_*) of every run from
        now on; SID_ESTATE between an ingest and its emit.  The header stays the
        caller's: emit(header=vcf_header(...))."""
        check(lib().sid_engine_set_format(self.h, _format(format)), "sid_engine_set_format")

    def set_depth_hist(self, on: bool):
        """The depth histogram of every run from now on (Engine.depth_hist);
        SID_ESTATE between an ingest and its emit."""
        check(lib().sid_engine_set_depth_hist(self.h, int(on)), "sid_engine_set_depth_hist")

    def set_region_stats(self, on: bool):
        """The region rows of every run from now on (Engine.region_stats);
        SID_EINVAL without a region set or past SID_REGION_STATS_MAX intervals,
        SID_ESTATE between an ingest and its emit."""
        check(lib().sid_engine_set_region_stats(self.h, int(on)), "sid_engine_set_region_stats")

    def placement(self, i=0) -> dict:
        """Pipeline i's host placement: its GPU's NUMA node, the CPUs its
        threads are bound to, the NUMA nodes of its pinned host buffers."""
        p = Placement()
        check(lib().sid_engine_placement(self.h, i, C.byref(p)), "sid_engine_placement")
        return {"device": p.device, "pci": p.pci.decode(), "gpu_numa_node": p.gpu_numa_node, "cpus": p.cpus,
                "first_cpu": p.first_cpu, "arena_numa_node": p.arena_numa_node, "ring_numa_node": p.ring_numa_node}

    def source_text(self, text: bytes):
        self._keep = C.create_string_buffer(text, len(text)) if text else None
        check(lib().sid_engine_source_text(self.h, C.cast(self._keep, C.c_void_p) if text else None, len(text)),
              "source_text")

    def source_host_ptr(self, ptr: int, n: int, keep=None):
        self._keep = keep
        check(lib().sid_engine_source_text(self.h, ptr, n), "source_text")

    def source_file(self, fd: int, offset: int = 0, length: int = None):
        if length is None:
            length = os.fstat(fd).st_size - offset
        check(lib().sid_engine_source_file(self.h, fd, offset, length), "source_file")

    def source_bgzf(self, data: bytes):
        """BGZF-compressed pileup text in host memory, inflated on the device."""
        self._keep = C.create_string_buffer(data, len(data)) if data else None
        off = C.c_uint64(0)
        st = lib().sid_engine_source_bgzf(self.h, C.cast(self._keep, C.c_void_p) if data else None, len(data),
                                          C.byref(off))
        if st != SID_OK:
            raise _bgzf_error(st, "source_bgzf", off.value)

    def source_bgzf_host_ptr(self, ptr: int, n: int, keep=None):
        """The same from host memory the caller owns (pinned, for measurements)."""
        self._keep = keep
        off = C.c_uint64(0)
        st = lib().sid_engine_source_bgzf(self.h, ptr, n, C.byref(off))
        if st != SID_OK:
            raise _bgzf_error(st, "source_bgzf", off.value)

    def source_bgzf_file(self, fd: int, offset: int = 0, length: int = None):
        if length is None:
            length = os.fstat(fd).st_size - offset
        off = C.c_uint64(0)
        st = lib().sid_engine_source_bgzf_file(self.h, fd, offset, length, C.byref(off))
        if st != SID_OK:
            raise _bgzf_error(st, "source_bgzf_file", off.value)

    def source_device_text(self, ptr: int, n: int, keep=None):
        self._keep = keep
        check(lib().sid_engine_source_device_text(self.h, ptr, n), "source_device_text")

    def source_synth(self, seed, n, depth=30.0, first=0, sites_per_chrom=0, sites_per_chunk=0, on_device=True):
        check(lib().sid_engine_source_synth(self.h, seed, depth, first, n, sites_per_chrom, sites_per_chunk,
                                            int(bool(on_device))), "source_synth")

    def ingest(self) -> RunStats:
        st = RunStats()
        rc = lib().sid_engine_ingest(self.h, C.byref(st))
        chunks, nbytes = C.c_uint64(0), C.c_uint64(0)
        check(lib().sid_engine_strip_stats(self.h, C.byref(chunks), C.byref(nbytes)), "sid_engine_strip_stats")
        st.chunks_stripped, st.strip_bytes = chunks.value, nbytes.value
        if rc != 0:
            err = SidError(rc, "sid_engine_ingest")
            err.offset = st.err_offset
            err.stats = st
            raise err
        return st

    def estimate(self, given: Estimate = None) -> Estimate:
        out = Estimate()
        check(lib().sid_engine_estimate(self.h, C.byref(given) if given is not None else None, C.byref(out)),
              "sid_engine_estimate")
        return out

    def emit(self, header=HEADER, sink=None, stats: RunStats = None):
        """Records in file order: returned as bytes (sink None), written to a
        file descriptor (sink int), or dropped (the device-sink engine)."""
        parts = []

        def w(_user, data, n):
            try:
                if isinstance(sink, int):   # every byte, across partial writes
                    mv = memoryview(C.string_at(data, n))
                    while len(mv):
                        mv = mv[os.write(sink, mv):]
                else:
                    parts.append(C.string_at(data, n))
                return 0
            except Exception:   # the engine reports SID_EIO
                return -1
        cb = WRITE_FN(w)
        st = stats if stats is not None else RunStats()
        check(lib().sid_engine_emit(self.h, header, cb, None, C.byref(st)), "sid_engine_emit")
        rows, n = C.POINTER(DepthRow)(), C.c_size_t(0)   # (SID_ESTATE with the option off: no rows)
        st.depth_rows = n.value if lib().sid_engine_depth_hist(self.h, C.byref(rows), C.byref(n)) == SID_OK else 0
        return b"".join(parts), st

    def profile_table(self):
        """The merged unique-profile table of all pipelines (after ingest)."""
        u = C.c_size_t(0)
        check(lib().sid_engine_profile_table(self.h, None, None, 0, C.byref(u)), "sid_engine_profile_table")
        keys = np.zeros(u.value, np.uint64)
        cnts = np.zeros(u.value, np.uint64)
        if u.value:
            check(lib().sid_engine_profile_table(self.h, _ptr(keys), _ptr(cnts), u.value, C.byref(u)),
                  "sid_engine_profile_table")
        return keys, cnts

    def profile_load(self, keys: np.ndarray, cnts: np.ndarray):
        keys = np.ascontiguousarray(keys, np.uint64)
        cnts = np.ascontiguousarray(cnts, np.uint64)
        check(lib().sid_engine_profile_load(self.h, _ptr(keys), _ptr(cnts), len(keys)), "sid_engine_profile_load")

    def records(self, chunk: int):
        """(address, length) of a chunk's records in the host arena."""
        p, n = C.c_void_p(), C.c_uint64(0)
        check(lib().sid_engine_records(self.h, chunk, C.byref(p), C.byref(n)), "sid_engine_records")
        return p.value or 0, n.value

    def records_bytes(self, nchunks: int) -> bytes:
        """Every chunk's records from the host arena, in file order."""
        out = []
        for j in range(nchunks):
            p, n = self.records(j)
            out.append(C.string_at(p, n) if n else b"")
        return b"".join(out)

    def windows(self) -> list:
        """The windowed summary of the last run (window != 0), after emit:
        tuples (chrom, start, end, sites, records, het, hom) in file order."""
        rows, n = C.POINTER(Window)(), C.c_size_t(0)
        check(lib().sid_engine_windows(self.h, C.byref(rows), C.byref(n)), "sid_engine_windows")
        return _window_rows(rows, n.value)

    def depth_hist(self) -> list:
        """The depth histogram of the last run (depth_hist=True), after emit:
        tuples (depth, sites, records, het, hom) in ascending depth order."""
        rows, n = C.POINTER(DepthRow)(), C.c_size_t(0)
        check(lib().sid_engine_depth_hist(self.h, C.byref(rows), C.byref(n)), "sid_engine_depth_hist")
        return _depth_rows(rows, n.value)

    def region_stats(self) -> list:
        """The region rows of the last run (region_stats=True), after emit: tuples
        (chrom, start, end, sites, depth, records, het, hom), one per interval of
        the region set in row order."""
        rows, n = C.POINTER(RegionRow)(), C.c_size_t(0)
        check(lib().sid_engine_region_stats(self.h, C.byref(rows), C.byref(n)), "sid_engine_region_stats")
        return _region_rows(rows, n.value)

    def profile(self, enable=True):
        check(lib().sid_engine_profile(self.h, int(bool(enable))), "sid_engine_profile")

    def profile_read(self) -> dict:
        p = EngineProf()
        check(lib().sid_engine_profile_read(self.h, C.byref(p)), "sid_engine_profile_read")
        return {f: getattr(p, f) for f, _ in EngineProf._fields_}

    def run(self, header=HEADER, sink=None):
        st = self.ingest()
        est = self.estimate()
        out, st2 = self.emit(header, sink)
        st.bytes_out, st.emit_s, st.chunks_reloaded = st2.bytes_out, st2.emit_s, st2.chunks_reloaded
        st.window_rows = st2.window_rows
        st.depth_rows = st2.depth_rows
        st.estimate = est
        return out, st


def profile_key(counts: np.ndarray) -> np.ndarray:
    c = counts.astype(np.uint64)
    return (c[:, 0] << np.uint64(48)) | (c[:, 1] << np.uint64(32)) | (c[:, 2] << np.uint64(16)) | c[:, 3]
