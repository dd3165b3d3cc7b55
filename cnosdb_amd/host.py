"""ctypes host bindings for libcnosdb_gs.so (see include/cnosdb_gs.h).

The binding mirrors the seam the reference's thin Rust shim would call
(SURVEY.md §8b): page upload standing where `ColumnGroupReader::read`
stands, `Engine.decode` standing where `decode_pages` stands
(tskv/src/tsm/reader.rs:494-560), `Engine.scan` standing where the
pure-time-range `DataFilter` + downsampling aggregate stand.
"""
import contextlib
import ctypes
import os

import numpy as np

CT_TIME, CT_I64, CT_F64, CT_BOOL, CT_U64, CT_STR = 0, 1, 2, 3, 4, 5

_DIR = os.path.dirname(os.path.abspath(__file__))


def lib_path():
    return os.path.join(_DIR, "libcnosdb_gs.so")


class GsTimeRange(ctypes.Structure):
    _fields_ = [("min_ts", ctypes.c_int64), ("max_ts", ctypes.c_int64)]


class GsPageSpec(ctypes.Structure):
    _fields_ = [
        ("bytes", ctypes.c_void_p),
        ("len", ctypes.c_uint64),
        ("num_values", ctypes.c_uint32),
        ("ctype", ctypes.c_uint8),
        ("column_id", ctypes.c_uint32),
    ]


class GsColumnGroupDesc(ctypes.Structure):
    _fields_ = [
        ("pages", ctypes.POINTER(GsPageSpec)),
        ("npages", ctypes.c_uint32),
        ("series_id", ctypes.c_uint32),
    ]


PRED_OPS = {"gt": 1, "ge": 2, "lt": 3, "le": 4, "eq": 5, "ne": 6,
            "between": 7}


class GsValuePred(ctypes.Structure):
    _fields_ = [("op", ctypes.c_int32), ("a", ctypes.c_double),
                ("b", ctypes.c_double)]


class GsScanSpec(ctypes.Structure):
    _fields_ = [
        ("range", GsTimeRange),
        ("field_col", ctypes.c_int32),
        ("tombstones", ctypes.POINTER(GsTimeRange)),
        ("n_tombstones", ctypes.c_size_t),
        ("bucket_ns", ctypes.c_int64),
        ("t0", ctypes.c_int64),
        ("n_buckets", ctypes.c_int32),
        ("d_agg_max", ctypes.c_void_p),
        ("d_agg_sum", ctypes.c_void_p),
        ("d_agg_count", ctypes.c_void_p),
        ("d_out_ts", ctypes.c_void_p),
        ("d_out_val", ctypes.c_void_p),
        ("d_ts", ctypes.c_void_p),
        ("d_val", ctypes.c_void_p),
        ("value_pred", GsValuePred),
    ]


class GsArrowArray(ctypes.Structure):
    pass


GsArrowArray._fields_ = [
    ("length", ctypes.c_int64), ("null_count", ctypes.c_int64),
    ("offset", ctypes.c_int64), ("n_buffers", ctypes.c_int64),
    ("n_children", ctypes.c_int64),
    ("buffers", ctypes.POINTER(ctypes.c_void_p)),
    ("children", ctypes.POINTER(ctypes.POINTER(GsArrowArray))),
    ("dictionary", ctypes.POINTER(GsArrowArray)),
    ("release", ctypes.c_void_p), ("private_data", ctypes.c_void_p),
]


class GsScanResult(ctypes.Structure):
    _fields_ = [
        ("out_rows", ctypes.c_int64),
        ("decoded_rows", ctypes.c_int64),
        ("ms_decode_ts", ctypes.c_double),
        ("ms_decode_val", ctypes.c_double),
        ("ms_filter", ctypes.c_double),
        ("ms_compact", ctypes.c_double),
        ("ms_agg", ctypes.c_double),
    ]


class GsStrColumn(ctypes.Structure):
    _fields_ = [("d_offsets", ctypes.c_void_p), ("d_bytes", ctypes.c_void_p),
                ("d_valid", ctypes.c_void_p)]


class GsStrColumnOut(ctypes.Structure):
    _fields_ = [("d_offsets", ctypes.c_void_p), ("d_bytes", ctypes.c_void_p),
                ("bytes_cap", ctypes.c_int64), ("d_valid", ctypes.c_void_p),
                ("total_bytes", ctypes.c_int64)]


class GsColPred(ctypes.Structure):
    _fields_ = [("col", ctypes.c_int32), ("op", ctypes.c_int32),
                ("a_bits", ctypes.c_uint64), ("b_bits", ctypes.c_uint64)]


class GsFilterCol(ctypes.Structure):
    _fields_ = [("ctype", ctypes.c_uint8), ("d_val", ctypes.c_void_p),
                ("d_valid", ctypes.c_void_p),
                ("tombstones", ctypes.POINTER(GsTimeRange)),
                ("n_tombstones", ctypes.c_size_t),
                ("d_out_val", ctypes.c_void_p),
                ("d_out_valid", ctypes.c_void_p)]


class GsFilterStrCol(ctypes.Structure):
    _fields_ = [("in_", GsStrColumn),
                ("tombstones", ctypes.POINTER(GsTimeRange)),
                ("n_tombstones", ctypes.c_size_t),
                ("out", ctypes.POINTER(GsStrColumnOut))]


class GsFilterSpec(ctypes.Structure):
    _fields_ = [("range", GsTimeRange),
                ("row_tombstones", ctypes.POINTER(GsTimeRange)),
                ("n_row_tombstones", ctypes.c_size_t),
                ("preds", ctypes.POINTER(GsColPred)),
                ("npreds", ctypes.c_int32)]


class GsAggSpec(ctypes.Structure):
    _fields_ = [("t0", ctypes.c_int64), ("bucket_ns", ctypes.c_int64),
                ("n_buckets", ctypes.c_int32), ("per_series", ctypes.c_int32)]


class GsAggOut(ctypes.Structure):
    _fields_ = [("col", ctypes.c_int32), ("d_count", ctypes.c_void_p),
                ("d_sum", ctypes.c_void_p), ("d_min", ctypes.c_void_p),
                ("d_max", ctypes.c_void_p), ("d_first", ctypes.c_void_p),
                ("d_last", ctypes.c_void_p), ("d_first_ts", ctypes.c_void_p),
                ("d_last_ts", ctypes.c_void_p)]


# gs_filter_group's ops: gs_scan's seven plus the two null tests
FILTER_OPS = dict(PRED_OPS, is_null=8, is_not_null=9)


def pred_bits(ctype, value):
    """A predicate constant as raw bits in the column's own type (GsColPred
    a_bits / b_bits).  Nothing is cast silently: a float on an integer
    column, a negative constant on u64, an integer outside the type's range
    or one a double cannot hold exactly are errors."""
    is_bool = isinstance(value, (bool, np.bool_))
    is_int = isinstance(value, (int, np.integer)) and not is_bool
    is_float = isinstance(value, (float, np.floating))
    if not (is_bool or is_int or is_float):
        raise TypeError(f"predicate constant {value!r} is no int, float or "
                        "bool")
    if ctype == CT_F64:
        if is_bool:
            raise TypeError("bool constant on an f64 column")
        if is_int and int(float(value)) != int(value):
            raise ValueError(f"{value} is not exact in f64")
        return int(np.array([value], dtype=np.float64).view(np.uint64)[0])
    if is_float:
        raise TypeError(f"float constant {value!r} on an integer or bool "
                        "column: compare in the column's own type")
    if ctype == CT_BOOL:
        if int(value) not in (0, 1):
            raise ValueError(f"bool constant must be 0 or 1, not {value}")
        return int(value)
    if is_bool:
        raise TypeError("bool constant on an integer column")
    value = int(value)
    if ctype == CT_I64:
        if not -2**63 <= value < 2**63:
            raise OverflowError(f"{value} is outside i64")
        return value & (2**64 - 1)
    if ctype == CT_U64:
        if value < 0:
            raise ValueError(f"negative constant {value} on a u64 column")
        if value >= 2**64:
            raise OverflowError(f"{value} is outside u64")
        return value
    raise ValueError(f"no predicate constants for ctype {ctype}")


# GsPageInfo as numpy sees it; min/max are re-viewed per column type
_PAGE_INFO_DT = np.dtype([("len", "<i8"), ("null_count", "<i8"),
                          ("min", "<u8"), ("max", "<u8")])


def _page_info_dtype(ctype):
    t = {CT_TIME: "<i8", CT_I64: "<i8", CT_F64: "<f8"}.get(int(ctype), "<u8")
    return np.dtype([("len", "<i8"), ("null_count", "<i8"),
                     ("min", t), ("max", t)])


class PageLib:
    """Loads libcnosdb_gs.so and declares signatures. Singleton per process."""

    _inst = None

    def __new__(cls):
        if cls._inst is None:
            cls._inst = super().__new__(cls)
            cls._inst._load()
        return cls._inst

    def _load(self):
        path = lib_path()
        if not os.path.exists(path):
            raise RuntimeError(
                f"cnosdb_gs HIP extension not built: {path} missing. "
                "Run __graft_entry__.build() — the product path has no "
                "CPU fallback.")
        lib = ctypes.CDLL(path)
        self.lib = lib
        for nm in ("gs_encode_ts", "gs_encode_i64", "gs_encode_f64",
                   "gs_encode_bool", "gs_encode_str", "gs_build_page"):
            getattr(lib, nm).restype = ctypes.c_int64
        lib.gs_decode_str.restype = ctypes.c_int32
        lib.gs_decode_str.argtypes = [
            ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint32,
            ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64,
            ctypes.c_void_p, ctypes.POINTER(ctypes.c_int64)]
        lib.gs_crc32.restype = ctypes.c_uint32
        lib.gs_version.restype = ctypes.c_char_p
        lib.gs_last_error.restype = ctypes.c_char_p
        lib.gs_device_count.restype = ctypes.c_int32
        lib.gs_ctx_create.restype = ctypes.c_void_p
        lib.gs_ctx_create.argtypes = [ctypes.c_int32]
        lib.gs_ctx_destroy.argtypes = [ctypes.c_void_p]
        lib.gs_groups_upload.restype = ctypes.c_void_p
        lib.gs_groups_upload.argtypes = [
            ctypes.c_void_p, ctypes.POINTER(GsColumnGroupDesc),
            ctypes.c_size_t, ctypes.c_int32]
        lib.gs_groups_free.argtypes = [ctypes.c_void_p]
        lib.gs_set_rows.restype = ctypes.c_int64
        lib.gs_set_rows.argtypes = [ctypes.c_void_p]
        lib.gs_set_groups.restype = ctypes.c_int64
        lib.gs_set_groups.argtypes = [ctypes.c_void_p]
        lib.gs_set_series.restype = ctypes.c_int64
        lib.gs_set_series.argtypes = [ctypes.c_void_p]
        lib.gs_count_pushdown.restype = ctypes.c_int64
        lib.gs_count_pushdown.argtypes = [ctypes.c_void_p, ctypes.c_uint32]
        lib.gs_set_row_offsets.restype = ctypes.c_int32
        lib.gs_set_row_offsets.argtypes = [ctypes.c_void_p, ctypes.c_void_p]
        lib.gs_decode.restype = ctypes.c_int32
        lib.gs_decode.argtypes = [ctypes.c_void_p, ctypes.c_void_p,
                                  ctypes.c_uint32, ctypes.c_void_p,
                                  ctypes.c_void_p]
        lib.gs_apply_tombstone.restype = ctypes.c_int32
        lib.gs_apply_tombstone.argtypes = [
            ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
            ctypes.c_void_p, ctypes.POINTER(GsTimeRange), ctypes.c_size_t]
        lib.gs_scan.restype = ctypes.c_int32
        lib.gs_scan.argtypes = [ctypes.c_void_p, ctypes.c_void_p,
                                ctypes.POINTER(GsScanSpec),
                                ctypes.POINTER(GsScanResult)]
        lib.gs_scan_async.restype = ctypes.c_int32
        lib.gs_scan_async.argtypes = [ctypes.c_void_p, ctypes.c_void_p,
                                      ctypes.POINTER(GsScanSpec)]
        lib.gs_scan_wait.restype = ctypes.c_int32
        lib.gs_scan_wait.argtypes = [ctypes.c_void_p, ctypes.c_void_p,
                                     ctypes.POINTER(GsScanResult)]
        lib.gs_encode_pages_dev.restype = ctypes.c_int32
        lib.gs_encode_pages_dev.argtypes = [
            ctypes.c_void_p, ctypes.c_int32, ctypes.c_void_p, ctypes.c_void_p,
            ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int32, ctypes.c_void_p,
            ctypes.c_int64, ctypes.c_void_p]
        lib.gs_encode_group_pages_dev.restype = ctypes.c_int32
        lib.gs_encode_group_pages_dev.argtypes = [
            ctypes.c_void_p, ctypes.c_int32, ctypes.c_void_p,
            ctypes.POINTER(ctypes.c_void_p), ctypes.POINTER(ctypes.c_void_p),
            ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int32,
            ctypes.POINTER(ctypes.c_void_p), ctypes.c_void_p, ctypes.c_void_p]
        lib.gs_encode_str_pages_dev.restype = ctypes.c_int32
        lib.gs_encode_str_pages_dev.argtypes = [
            ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
            ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int32, ctypes.c_void_p,
            ctypes.c_int64, ctypes.c_void_p]
        lib.gs_export_group_column.restype = ctypes.c_int32
        lib.gs_export_group_column.argtypes = [
            ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p,
            ctypes.c_int32, ctypes.c_void_p, ctypes.POINTER(GsArrowArray)]
        lib.gs_compact_merge.restype = ctypes.c_int32
        lib.gs_compact_merge.argtypes = [
            ctypes.c_void_p, ctypes.POINTER(ctypes.c_void_p), ctypes.c_int32,
            ctypes.POINTER(ctypes.c_void_p), ctypes.POINTER(ctypes.c_void_p),
            ctypes.POINTER(ctypes.c_void_p), ctypes.c_void_p, ctypes.c_void_p,
            ctypes.c_void_p, ctypes.c_void_p, ctypes.POINTER(ctypes.c_int64)]
        lib.gs_compact_merge_fields.restype = ctypes.c_int32
        lib.gs_compact_merge_fields.argtypes = [
            ctypes.c_void_p, ctypes.POINTER(ctypes.c_void_p), ctypes.c_int32,
            ctypes.c_int32, ctypes.POINTER(ctypes.c_int32),
            ctypes.POINTER(ctypes.c_void_p), ctypes.POINTER(ctypes.c_void_p),
            ctypes.POINTER(ctypes.c_void_p), ctypes.c_void_p,
            ctypes.POINTER(ctypes.c_void_p), ctypes.POINTER(ctypes.c_void_p),
            ctypes.c_void_p, ctypes.POINTER(ctypes.c_int64)]
        lib.gs_compact_merge_group.restype = ctypes.c_int32
        lib.gs_compact_merge_group.argtypes = [
            ctypes.c_void_p, ctypes.POINTER(ctypes.c_void_p), ctypes.c_int32,
            ctypes.c_int32, ctypes.POINTER(ctypes.c_int32),
            ctypes.POINTER(ctypes.c_void_p), ctypes.POINTER(ctypes.c_void_p),
            ctypes.POINTER(ctypes.c_void_p), ctypes.c_int32,
            ctypes.POINTER(GsStrColumn), ctypes.c_void_p,
            ctypes.POINTER(ctypes.c_void_p), ctypes.POINTER(ctypes.c_void_p),
            ctypes.POINTER(GsStrColumnOut), ctypes.c_void_p,
            ctypes.POINTER(ctypes.c_int64)]
        lib.gs_filter_group.restype = ctypes.c_int32
        lib.gs_filter_group.argtypes = [
            ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
            ctypes.POINTER(GsFilterSpec), ctypes.c_int32,
            ctypes.POINTER(GsFilterCol), ctypes.c_int32,
            ctypes.POINTER(GsFilterStrCol), ctypes.c_void_p, ctypes.c_void_p,
            ctypes.POINTER(ctypes.c_int64)]
        lib.gs_agg_group.restype = ctypes.c_int32
        lib.gs_agg_group.argtypes = [
            ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
            ctypes.POINTER(GsFilterSpec), ctypes.c_int32,
            ctypes.POINTER(GsFilterCol), ctypes.c_int32,
            ctypes.POINTER(GsFilterStrCol), ctypes.POINTER(GsAggSpec),
            ctypes.c_int32, ctypes.POINTER(GsAggOut), ctypes.c_void_p]
        lib.gs_debug_agg_ms.restype = ctypes.c_float
        lib.gs_debug_filter_tile.restype = ctypes.c_int32
        lib.gs_debug_filter_ms.restype = ctypes.c_float
        lib.gs_debug_set_grid_cap.restype = ctypes.c_int32
        lib.gs_debug_set_grid_cap.argtypes = [ctypes.c_int32]
        lib.gs_debug_grid_rounds.restype = ctypes.c_int32
        lib.gs_debug_grid_rounds.argtypes = [ctypes.c_int]

    def err(self):
        return self.lib.gs_last_error().decode()


def _np_ptr(arr):
    return arr.ctypes.data_as(ctypes.c_void_p)


# ---- host-side encoders (product write path; CPU like the reference's) ----

def encode_ts(values):
    values = np.ascontiguousarray(values, dtype=np.int64)
    lib = PageLib().lib
    buf = np.zeros(values.size * 9 + 64, dtype=np.uint8)
    n = lib.gs_encode_ts(_np_ptr(values), values.size, _np_ptr(buf), buf.size)
    if n < 0:
        raise RuntimeError(f"gs_encode_ts failed: {n}")
    return buf[:n].tobytes()


def encode_i64(values):
    values = np.ascontiguousarray(values, dtype=np.int64)
    lib = PageLib().lib
    buf = np.zeros(values.size * 9 + 64, dtype=np.uint8)
    n = lib.gs_encode_i64(_np_ptr(values), values.size, _np_ptr(buf), buf.size)
    if n < 0:
        raise RuntimeError(f"gs_encode_i64 failed: {n}")
    return buf[:n].tobytes()


def encode_f64(values):
    values = np.ascontiguousarray(values, dtype=np.float64)
    lib = PageLib().lib
    buf = np.zeros(values.size * 12 + 64, dtype=np.uint8)
    n = lib.gs_encode_f64(_np_ptr(values), values.size, _np_ptr(buf), buf.size)
    if n < 0:
        raise RuntimeError(f"gs_encode_f64 failed: {n}")
    return buf[:n].tobytes()


def encode_bool(values):
    values = np.ascontiguousarray(values, dtype=np.uint8)
    lib = PageLib().lib
    buf = np.zeros(values.size + 64, dtype=np.uint8)
    n = lib.gs_encode_bool(_np_ptr(values), values.size, _np_ptr(buf), buf.size)
    if n < 0:
        raise RuntimeError(f"gs_encode_bool failed: {n}")
    return buf[:n].tobytes()


def encode_str(strings):
    """Snappy string block (codec/string.rs:32-88): strings = list of
    bytes (non-null values only)."""
    lib = PageLib().lib
    concat = b"".join(strings)
    lens = np.array([len(s) for s in strings], dtype=np.uint64)
    src = np.frombuffer(concat, dtype=np.uint8) if concat else np.zeros(1, np.uint8)
    cap = 2 + 32 + len(concat) + len(concat) // 6 + len(strings) * 10 + 64
    buf = np.zeros(cap, dtype=np.uint8)
    n = lib.gs_encode_str(_np_ptr(src), _np_ptr(lens), len(strings),
                          _np_ptr(buf), buf.size)
    if n < 0:
        raise RuntimeError(f"gs_encode_str failed: {n}")
    return buf[:n].tobytes()


def str_page_of(strings, valid=None):
    """Build a string column page. strings = list of bytes per row;
    valid = bool array or None; null rows' strings are not encoded
    (page.rs/A.2 semantics)."""
    nrows = len(strings)
    if valid is None:
        present = strings
        bitset = None
    else:
        valid = np.asarray(valid, dtype=bool)
        present = [s for s, v in zip(strings, valid) if v]
        bitset = np.packbits(valid, bitorder="little")
    return build_page(encode_str(present), nrows, bitset)


def crc32(data):
    """CRC-32/ISO-HDLC of a page's data region (tsm/page.rs:58-76)."""
    d = np.frombuffer(bytes(data), dtype=np.uint8)
    return int(PageLib().lib.gs_crc32(_np_ptr(d), ctypes.c_size_t(d.size)))


def build_page(data, nrows, bitset=None):
    """Assemble full page bytes (tsm/page.rs layout). bitset: packed
    LSB-first validity bytes; None -> all valid."""
    lib = PageLib().lib
    if bitset is None:
        nb = (nrows + 7) // 8
        bitset = np.full(nb, 0xFF, dtype=np.uint8)
        if nrows % 8:
            bitset[-1] = (1 << (nrows % 8)) - 1
    else:
        bitset = np.ascontiguousarray(bitset, dtype=np.uint8)
    data = np.frombuffer(data, dtype=np.uint8) if isinstance(data, (bytes, bytearray)) else np.ascontiguousarray(data, dtype=np.uint8)
    out = np.zeros(16 + bitset.size + data.size, dtype=np.uint8)
    n = lib.gs_build_page(_np_ptr(bitset), nrows, _np_ptr(data), data.size,
                          _np_ptr(out), out.size)
    if n < 0:
        raise RuntimeError(f"gs_build_page failed: {n}")
    return out[:n].tobytes()


def page_of(values, ctype, valid=None):
    """Encode a column + assemble its page. valid: bool array or None.
    The encoded stream holds only non-null values (page.rs/A.2)."""
    values = np.asarray(values)
    nrows = values.size
    if valid is None:
        present = values
        bitset = None
    else:
        valid = np.asarray(valid, dtype=bool)
        present = values[valid]
        bitset = np.packbits(valid, bitorder="little")
    if ctype == CT_TIME:
        data = encode_ts(present.astype(np.int64))
    elif ctype == CT_I64:
        data = encode_i64(present.astype(np.int64))
    elif ctype == CT_F64:
        data = encode_f64(present.astype(np.float64))
    elif ctype == CT_BOOL:
        data = encode_bool(present.astype(np.uint8))
    elif ctype == CT_U64:
        # u64 is the i64 codec over the bit-cast values (unsigned.rs:15-18)
        data = encode_i64(
            np.ascontiguousarray(present).astype(np.uint64).view(np.int64))
    else:
        raise ValueError(ctype)
    return build_page(data, nrows, bitset)


# ------------------------------ device engine ------------------------------

class GroupSet:
    def __init__(self, engine, handle, nrows, ngroups, keepalive):
        self._engine = engine
        self._h = handle
        self.rows = nrows
        self.ngroups = ngroups
        self._keepalive = keepalive  # page byte buffers must outlive upload

    def count_pushdown(self, col=0):
        """pushed-down COUNT from page metadata (no decode)."""
        return PageLib().lib.gs_count_pushdown(self._h, col)

    def row_offsets(self):
        out = np.zeros(self.ngroups, dtype=np.int64)
        st = PageLib().lib.gs_set_row_offsets(self._h, _np_ptr(out))
        if st != 0:
            raise RuntimeError(PageLib().err())
        return out

    def free(self):
        if self._h:
            PageLib().lib.gs_groups_free(self._h)
            self._h = None
            self._keepalive = None


class Engine:
    """One GPU device context. Raises at construction if no HIP device —
    the product path fails loudly rather than falling back to CPU."""

    def __init__(self, device=0):
        self._pl = PageLib()
        self.lib = self._pl.lib
        ctx = self.lib.gs_ctx_create(device)
        if not ctx:
            raise RuntimeError(f"gs_ctx_create failed: {self._pl.err()}")
        self._ctx = ctypes.c_void_p(ctx)
        self.device = device

    def close(self):
        if self._ctx:
            self.lib.gs_ctx_destroy(self._ctx)
            self._ctx = None

    def upload_packed(self, buf, page_off, page_len, num_values, ctypes_arr,
                      series_ids, pages_per_group, validate_crc=True):
        """Vectorized upload: all pages live in one contiguous host buffer.
        page_off/page_len/num_values/ctypes_arr are per-page numpy arrays in
        group-major order (group g's pages at [g*ppg, (g+1)*ppg), pages[0]
        of each group = time page); series_ids is per-group."""
        buf = np.frombuffer(buf, dtype=np.uint8) if isinstance(buf, (bytes, bytearray)) else buf
        npages = page_off.size
        ngroups = npages // pages_per_group
        spec_dt = np.dtype({
            "names": ["ptr", "len", "nv", "ct", "cid"],
            "formats": ["<u8", "<u8", "<u4", "u1", "<u4"],
            "offsets": [0, 8, 16, 20, 24],
            "itemsize": ctypes.sizeof(GsPageSpec),
        })
        specs = np.zeros(npages, dtype=spec_dt)
        specs["ptr"] = buf.ctypes.data + page_off.astype(np.uint64)
        specs["len"] = page_len.astype(np.uint64)
        specs["nv"] = num_values.astype(np.uint32)
        specs["ct"] = ctypes_arr.astype(np.uint8)
        specs["cid"] = np.tile(np.arange(pages_per_group, dtype=np.uint32), ngroups)
        gdesc_dt = np.dtype({
            "names": ["pages", "npages", "sid"],
            "formats": ["<u8", "<u4", "<u4"],
            "offsets": [0, 8, 12],
            "itemsize": ctypes.sizeof(GsColumnGroupDesc),
        })
        gdescs = np.zeros(ngroups, dtype=gdesc_dt)
        gdescs["pages"] = specs.ctypes.data + \
            (np.arange(ngroups, dtype=np.uint64) * pages_per_group *
             ctypes.sizeof(GsPageSpec))
        gdescs["npages"] = pages_per_group
        gdescs["sid"] = series_ids.astype(np.uint32)
        h = self.lib.gs_groups_upload(
            self._ctx,
            ctypes.cast(gdescs.ctypes.data, ctypes.POINTER(GsColumnGroupDesc)),
            ngroups, 1 if validate_crc else 0)
        if not h:
            raise RuntimeError(f"gs_groups_upload failed: {self._pl.err()}")
        h = ctypes.c_void_p(h)
        rows = self.lib.gs_set_rows(h)
        # gs_groups_upload synchronizes after staging all page bytes, so the
        # host buffer need not be retained (matters at 8 ranks x ~17 GB)
        return GroupSet(self, h, rows, ngroups, None)

    def upload(self, groups, validate_crc=True):
        """groups: list of (series_id, [(page_bytes, ctype), ...]);
        pages[0] must be the time page."""
        keep = []
        gdescs = (GsColumnGroupDesc * len(groups))()
        for gi, (sid, pages) in enumerate(groups):
            specs = (GsPageSpec * len(pages))()
            keep.append(specs)
            for pi, (pb, ctype) in enumerate(pages):
                if isinstance(pb, (bytes, bytearray)):
                    pb = np.frombuffer(pb, dtype=np.uint8)
                keep.append(pb)
                nrows = int.from_bytes(pb[4:12].tobytes(), "big")
                specs[pi].bytes = pb.ctypes.data
                specs[pi].len = pb.size
                specs[pi].num_values = nrows
                specs[pi].ctype = ctype
                specs[pi].column_id = pi
            gdescs[gi].pages = specs
            gdescs[gi].npages = len(pages)
            gdescs[gi].series_id = sid
        h = self.lib.gs_groups_upload(self._ctx, gdescs, len(groups),
                                      1 if validate_crc else 0)
        if not h:
            raise RuntimeError(f"gs_groups_upload failed: {self._pl.err()}")
        h = ctypes.c_void_p(h)
        rows = self.lib.gs_set_rows(h)
        return GroupSet(self, h, rows, len(groups), keep)

    def decode(self, gset, col, d_out, d_valid=None):
        """d_out/d_valid: torch CUDA tensors (int64/float64/uint8)."""
        st = self.lib.gs_decode(self._ctx, gset._h, col,
                                ctypes.c_void_p(d_out.data_ptr()),
                                ctypes.c_void_p(d_valid.data_ptr()) if d_valid is not None else None)
        if st != 0:
            raise RuntimeError(f"gs_decode failed ({st}): {self._pl.err()}")

    def raw_set(self, counts):
        """Series structure over caller-resident device arrays (memcache
        rows, MemCacheReader): counts[i] = rows of series i.  The
        returned set is scanned with Engine.scan where d_ts/d_val hold
        the rows themselves, and composes with compact_merge."""
        counts = np.ascontiguousarray(counts, dtype=np.int64)
        self.lib.gs_raw_set.restype = ctypes.c_void_p
        h = self.lib.gs_raw_set(self._ctx, _np_ptr(counts), counts.size)
        if not h:
            raise RuntimeError(f"gs_raw_set failed: {self._pl.err()}")
        return GroupSet(self, ctypes.c_void_p(h), int(counts.sum()),
                        counts.size, None)

    def decode_str(self, gset, col, d_offsets, d_bytes, d_valid=None):
        """String column decode to Arrow varbinary layout
        (str_snappy_decode_to_array, string.rs:226-276): d_offsets int64
        CUDA tensor of rows+1, d_bytes uint8 CUDA tensor (capacity);
        returns total payload bytes written."""
        total = ctypes.c_int64(0)
        st = self.lib.gs_decode_str(
            self._ctx, gset._h, col,
            ctypes.c_void_p(d_offsets.data_ptr()),
            ctypes.c_void_p(d_bytes.data_ptr()), d_bytes.numel(),
            ctypes.c_void_p(d_valid.data_ptr()) if d_valid is not None else None,
            ctypes.byref(total))
        if st != 0:
            raise RuntimeError(f"gs_decode_str failed ({st}): {self._pl.err()}")
        return total.value

    def apply_tombstone(self, gset, d_ts, d_valid, ranges):
        arr = (GsTimeRange * len(ranges))(*[GsTimeRange(a, b) for a, b in ranges])
        st = self.lib.gs_apply_tombstone(self._ctx, gset._h,
                                         ctypes.c_void_p(d_ts.data_ptr()),
                                         ctypes.c_void_p(d_valid.data_ptr()),
                                         arr, len(ranges))
        if st != 0:
            raise RuntimeError(f"gs_apply_tombstone failed: {self._pl.err()}")

    def export_group_column(self, gset, group, d_col, elem_size=8,
                            d_valid=None):
        """Export one group's rows as an Arrow-C-data-interface array
        (host copy).  Returns (GsArrowArray, np data view, np bitmap or
        None); call arr-release via free_arrow when done."""
        arr = GsArrowArray()
        st = self.lib.gs_export_group_column(
            self._ctx, gset._h, group, ctypes.c_void_p(d_col.data_ptr()),
            elem_size,
            ctypes.c_void_p(d_valid.data_ptr()) if d_valid is not None else None,
            ctypes.byref(arr))
        if st != 0:
            raise RuntimeError(f"gs_export_group_column failed: {self._pl.err()}")
        n = arr.length
        data = np.ctypeslib.as_array(
            ctypes.cast(arr.buffers[1], ctypes.POINTER(ctypes.c_uint8)),
            shape=(n * elem_size,)).copy()
        bitmap = None
        if arr.buffers[0]:
            bitmap = np.ctypeslib.as_array(
                ctypes.cast(arr.buffers[0], ctypes.POINTER(ctypes.c_uint8)),
                shape=((n + 7) // 8,)).copy()
        rel = ctypes.CFUNCTYPE(None, ctypes.POINTER(GsArrowArray))(arr.release)
        rel(ctypes.byref(arr))
        return arr, data, bitmap

    def compact_merge(self, gsets, d_ts_list, d_val_list, d_valid_list,
                      d_out_ts, d_out_val, d_out_valid=None):
        """k-way merge+dedup (BASELINE config #5). gsets oldest->newest;
        d_*_list: per-stream decoded torch tensors (valid entries may be
        None). Returns (out_rows, per-series offsets np.array)."""
        k = len(gsets)
        sets = (ctypes.c_void_p * k)(*[g._h for g in gsets])
        ts_p = (ctypes.c_void_p * k)(*[t.data_ptr() for t in d_ts_list])
        val_p = (ctypes.c_void_p * k)(*[t.data_ptr() for t in d_val_list])
        vd_p = (ctypes.c_void_p * k)(
            *[(t.data_ptr() if t is not None else None) for t in d_valid_list])
        nseries = self.lib.gs_set_series(gsets[0]._h)
        offs = np.zeros(nseries + 1, dtype=np.int64)
        rows = ctypes.c_int64(0)
        st = self.lib.gs_compact_merge(
            self._ctx, sets, k, ts_p, val_p, vd_p,
            ctypes.c_void_p(d_out_ts.data_ptr()),
            ctypes.c_void_p(d_out_val.data_ptr()),
            ctypes.c_void_p(d_out_valid.data_ptr()) if d_out_valid is not None else None,
            _np_ptr(offs), ctypes.byref(rows))
        if st != 0:
            raise RuntimeError(f"gs_compact_merge failed ({st}): {self._pl.err()}")
        return rows.value, offs

    def compact_merge_fields(self, gsets, d_ts_list, cols, d_out_ts,
                             d_out_cols):
        """k-way merge+dedup over every field column of a column group
        (take_last_and_merge, batch_builder.rs:132-155): per column the
        newest non-null value wins.  gsets oldest->newest; cols[f][c] =
        (values_tensor_or_None, valid_tensor_or_None), a None values
        tensor meaning column c is absent from stream f; d_out_cols[c] =
        (values_tensor, valid_tensor_or_None).  Element sizes come from
        the output tensors' dtypes (float64/int64 -> 8, uint8 -> 1; u64
        travels as int64 bits).  Returns (out_rows, per-series offsets
        np.array)."""
        k = len(gsets)
        ncols = len(d_out_cols)
        for f in range(k):
            if len(cols[f]) != ncols:
                raise ValueError(f"stream {f}: {len(cols[f])} columns, "
                                 f"outputs have {ncols}")

        def ptr(t):
            return t.data_ptr() if t is not None else None

        sets = (ctypes.c_void_p * k)(*[g._h for g in gsets])
        ts_p = (ctypes.c_void_p * k)(*[t.data_ptr() for t in d_ts_list])
        val_p = (ctypes.c_void_p * (k * ncols))(
            *[ptr(cols[f][c][0]) for f in range(k) for c in range(ncols)])
        vds = [cols[f][c][1] for f in range(k) for c in range(ncols)]
        vd_p = None  # whole array NULL: every present column all-valid
        if any(v is not None for v in vds):
            vd_p = (ctypes.c_void_p * (k * ncols))(*[ptr(v) for v in vds])
        esz = (ctypes.c_int32 * ncols)(
            *[v.element_size() for v, _ in d_out_cols])
        oval_p = (ctypes.c_void_p * ncols)(
            *[v.data_ptr() for v, _ in d_out_cols])
        ovd_p = (ctypes.c_void_p * ncols)(*[ptr(v) for _, v in d_out_cols])
        nseries = self.lib.gs_set_series(gsets[0]._h)
        offs = np.zeros(nseries + 1, dtype=np.int64)
        rows = ctypes.c_int64(0)
        st = self.lib.gs_compact_merge_fields(
            self._ctx, sets, k, ncols, esz, ts_p, val_p, vd_p,
            ctypes.c_void_p(d_out_ts.data_ptr()), oval_p, ovd_p,
            _np_ptr(offs), ctypes.byref(rows))
        if st != 0:
            raise RuntimeError(
                f"gs_compact_merge_fields failed ({st}): {self._pl.err()}")
        return rows.value, offs

    def compact_merge_group(self, gsets, d_ts_list, cols, str_cols, d_out_ts,
                            d_out_cols, str_outs):
        """compact_merge_fields plus string columns
        (gs_compact_merge_group).  cols / d_out_cols as in
        compact_merge_fields (both may be empty lists per stream / empty);
        str_cols[f][c] = (d_offsets, d_bytes, d_valid_or_None), decode_str's
        layout, or None where column c is absent from stream f;
        str_outs[c] = (d_offsets, d_bytes, d_valid_or_None).  Returns
        (out_rows, per-series offsets np.array, [total_bytes per string
        column]).  The exception of a failed call carries .status (GsStatus)
        and .total_bytes (filled when the status is GS_ERR_CAP)."""
        k = len(gsets)
        ncols, nstr = len(d_out_cols), len(str_outs)
        for f in range(k):
            if len(cols[f]) != ncols or len(str_cols[f]) != nstr:
                raise ValueError(f"stream {f}: column counts differ from "
                                 "the outputs'")

        def ptr(t):
            return t.data_ptr() if t is not None else None

        sets = (ctypes.c_void_p * k)(*[g._h for g in gsets])
        ts_p = (ctypes.c_void_p * k)(*[t.data_ptr() for t in d_ts_list])
        ncell = max(k * ncols, 1)
        val_p = (ctypes.c_void_p * ncell)(
            *[ptr(cols[f][c][0]) for f in range(k) for c in range(ncols)])
        vd_p = (ctypes.c_void_p * ncell)(
            *[ptr(cols[f][c][1]) for f in range(k) for c in range(ncols)])
        esz = (ctypes.c_int32 * max(ncols, 1))(
            *[v.element_size() for v, _ in d_out_cols])
        oval_p = (ctypes.c_void_p * max(ncols, 1))(
            *[v.data_ptr() for v, _ in d_out_cols])
        ovd_p = (ctypes.c_void_p * max(ncols, 1))(
            *[ptr(v) for _, v in d_out_cols])
        sin = (GsStrColumn * max(k * nstr, 1))()
        for f in range(k):
            for c in range(nstr):
                col = str_cols[f][c]
                if col is not None:
                    sin[f * nstr + c] = GsStrColumn(
                        col[0].data_ptr(), col[1].data_ptr(), ptr(col[2]))
        sout = (GsStrColumnOut * max(nstr, 1))()
        for c, (d_off, d_bytes, d_vd) in enumerate(str_outs):
            sout[c] = GsStrColumnOut(d_off.data_ptr(), d_bytes.data_ptr(),
                                     d_bytes.numel(), ptr(d_vd), -1)
        nseries = self.lib.gs_set_series(gsets[0]._h)
        offs = np.zeros(nseries + 1, dtype=np.int64)
        rows = ctypes.c_int64(0)
        st = self.lib.gs_compact_merge_group(
            self._ctx, sets, k, ncols, esz, ts_p, val_p, vd_p, nstr, sin,
            ctypes.c_void_p(d_out_ts.data_ptr()), oval_p, ovd_p, sout,
            _np_ptr(offs), ctypes.byref(rows))
        totals = [int(sout[c].total_bytes) for c in range(nstr)]
        if st != 0:
            e = RuntimeError(
                f"gs_compact_merge_group failed ({st}): {self._pl.err()}")
            e.status, e.total_bytes = st, totals
            raise e
        return rows.value, offs, totals

    @staticmethod
    def _filter_args(cols, preds, str_cols, time_range, row_tombstones):
        """cols / preds / str_cols / time_range / row_tombstones of
        filter_group and agg_group as the C structs.  Returns (fcols, fstrs,
        spec, souts, keep): souts the GsStrColumnOut of every string column
        (None without output), keep whatever the structs point into."""
        ncols = len(cols)
        keep = []

        def ptr(t):
            return t.data_ptr() if t is not None else None

        def ranges(lst):
            lst = list(lst) if lst is not None else []
            if not lst:
                return None, 0
            arr = (GsTimeRange * len(lst))(*[GsTimeRange(a, b) for a, b in lst])
            keep.append(arr)
            return arr, len(lst)

        fcols = (GsFilterCol * max(ncols, 1))()
        ctypes_of = []
        for c, col in enumerate(cols):
            col = tuple(col) + (None,) * (6 - len(col))
            ct, d_val, d_valid, tombs, d_out_val, d_out_valid = col
            ctypes_of.append(int(ct))
            fcols[c].ctype = int(ct)
            fcols[c].d_val = ptr(d_val)
            fcols[c].d_valid = ptr(d_valid)
            tarr, tn = ranges(tombs)
            if tn:
                fcols[c].tombstones = tarr
            fcols[c].n_tombstones = tn
            fcols[c].d_out_val = ptr(d_out_val)
            fcols[c].d_out_valid = ptr(d_out_valid)
        fstrs = (GsFilterStrCol * max(len(str_cols), 1))()
        souts = []
        for s, col in enumerate(str_cols):
            col = tuple(col) + (None,) * (3 - len(col))
            (d_off, d_bytes, d_valid), tombs, out = col
            fstrs[s].in_ = GsStrColumn(ptr(d_off), ptr(d_bytes), ptr(d_valid))
            tarr, tn = ranges(tombs)
            if tn:
                fstrs[s].tombstones = tarr
            fstrs[s].n_tombstones = tn
            if out is None:
                souts.append(None)
                continue
            o = GsStrColumnOut(ptr(out[0]), ptr(out[1]),
                               out[1].numel() if out[1] is not None else 0,
                               ptr(out[2]) if len(out) > 2 else None, -1)
            souts.append(o)
            fstrs[s].out = ctypes.pointer(o)
        parr = (GsColPred * max(len(preds), 1))()
        keep.append(parr)
        for p, pred in enumerate(preds):
            col, op = int(pred[0]), pred[1]
            parr[p].col = col
            parr[p].op = FILTER_OPS[op] if isinstance(op, str) else int(op)
            # constants of a column the library will refuse stay 0
            if 0 <= col < ncols and ctypes_of[col] in (CT_I64, CT_F64,
                                                       CT_BOOL, CT_U64):
                if len(pred) > 2:
                    parr[p].a_bits = pred_bits(ctypes_of[col], pred[2])
                if len(pred) > 3:
                    parr[p].b_bits = pred_bits(ctypes_of[col], pred[3])
        spec = GsFilterSpec()
        lo, hi = time_range if time_range else (-(2**63), 2**63 - 1)
        spec.range = GsTimeRange(lo, hi)
        tarr, tn = ranges(row_tombstones)
        if tn:
            spec.row_tombstones = tarr
        spec.n_row_tombstones = tn
        if preds:
            spec.preds = parr
        spec.npreds = len(preds)
        return fcols, fstrs, spec, souts, keep

    def filter_group(self, gset, d_ts, cols, preds, str_cols=(),
                     time_range=None, row_tombstones=(), d_out_ts=None):
        """DataFilter over a column group (gs_filter_group): one mask from
        the time range, the row tombstones and a conjunction of typed
        predicates, and every projected column compacted by it.

        cols[c] = (ctype, d_val, d_valid, tombstones, d_out_val,
        d_out_valid); everything after d_val may be left out or None
        (d_out_val None = the column only serves predicates).
        str_cols[s] = ((d_offsets, d_bytes, d_valid), tombstones, out) in
        decode_str's layout, out = (d_offsets, d_bytes, d_valid) or None.
        preds = [(col, op, a[, b])], op one of FILTER_OPS ("gt" ... "between",
        "is_null", "is_not_null"), col >= len(cols) naming a string column;
        the constants are Python ints, floats or bools, converted to raw
        bits in the column's own type by pred_bits, which refuses what does
        not fit.  Tombstones are lists of closed (min_ts, max_ts).

        Returns (out_rows, offsets ndarray of ngroups + 1); the byte totals
        of the projected string columns are left in self.filter_str_totals
        (None for a column without output).  The exception of a failed call
        carries .status (GsStatus), and for GS_ERR_CAP .total_bytes,
        .out_rows and .offsets: size the byte buffers and call again."""
        ncols, nstr = len(cols), len(str_cols)
        fcols, fstrs, spec, souts, _keep = self._filter_args(
            cols, preds, str_cols, time_range, row_tombstones)

        def ptr(t):
            return t.data_ptr() if t is not None else None

        offs = np.zeros(gset.ngroups + 1, dtype=np.int64)
        rows = ctypes.c_int64(0)
        st = self.lib.gs_filter_group(
            self._ctx, gset._h, ptr(d_ts), ctypes.byref(spec), ncols,
            fcols if ncols else None, nstr, fstrs if nstr else None,
            ptr(d_out_ts), _np_ptr(offs), ctypes.byref(rows))
        self.filter_str_totals = [
            int(o.total_bytes) if o is not None else None for o in souts]
        if st != 0:
            e = RuntimeError(
                f"gs_filter_group failed ({st}): {self._pl.err()}")
            e.status = st
            e.total_bytes = self.filter_str_totals
            e.out_rows, e.offsets = rows.value, offs
            raise e
        return rows.value, offs

    AGG_NAMES = ("count", "sum", "min", "max", "first", "last", "first_ts",
                 "last_ts")

    def agg_group(self, gset, d_ts, cols, preds, aggs, t0, bucket_ns,
                  n_buckets, per_series=True, str_cols=(), time_range=None,
                  row_tombstones=(), d_rows=None):
        """Typed bucket aggregates over a filtered column group
        (gs_agg_group): the keep rule of filter_group, and the kept,
        effectively valid cells of the aggregated columns reduced into
        (series, bucket) cells without any row output.

        cols / preds / str_cols / time_range / row_tombstones exactly as
        filter_group takes them (output tensors in cols are ignored).
        aggs = [(col, {"count": tensor, "sum": tensor, "min": ..., "max":
        ..., "first": ..., "last": ..., "first_ts": ..., "last_ts": ...})]:
        col an index into cols, every tensor a CUDA tensor of 8 bytes per
        cell (gset series * n_buckets cells with per_series, else
        n_buckets), names left out are not computed.  Values come back as
        raw bits in the column's type: view the tensor as the column's
        dtype.  d_rows (int64, one per cell) receives the kept rows per
        cell.  Every cell of every tensor is written by the call.  The
        exception of a failed call carries .status (GsStatus)."""
        ncols, nstr = len(cols), len(str_cols)
        fcols, fstrs, spec, _souts, _keep = self._filter_args(
            cols, preds, str_cols, time_range, row_tombstones)

        def ptr(t):
            return t.data_ptr() if t is not None else None

        aspec = GsAggSpec(int(t0), int(bucket_ns), int(n_buckets),
                          1 if per_series else 0)
        outs = (GsAggOut * max(len(aggs), 1))()
        for i, (col, want) in enumerate(aggs):
            unknown = set(want) - set(self.AGG_NAMES)
            if unknown:
                raise ValueError(f"unknown aggregates {sorted(unknown)}")
            outs[i].col = int(col)
            for name in self.AGG_NAMES:
                setattr(outs[i], "d_" + name, ptr(want.get(name)))
        st = self.lib.gs_agg_group(
            self._ctx, gset._h, ptr(d_ts), ctypes.byref(spec), ncols,
            fcols if ncols else None, nstr, fstrs if nstr else None,
            ctypes.byref(aspec), len(aggs), outs if aggs else None,
            ptr(d_rows))
        if st != 0:
            e = RuntimeError(f"gs_agg_group failed ({st}): {self._pl.err()}")
            e.status = st
            raise e

    def encode_pages_dev(self, kind, d_vals, row_off, rows, d_out,
                         cap_per_page, d_valid=None):
        """GPU page re-encode. kind: 0=ts 1=i64 2=f64. row_off/rows: host
        numpy arrays; d_out capacity npages*cap_per_page. Returns lens.
        The exception of a failed call carries .status (GsStatus) and
        .lens (negative where a page failed, see cnosdb_gs.h)."""
        row_off = np.ascontiguousarray(row_off, dtype=np.int64)
        rows = np.ascontiguousarray(rows, dtype=np.int32)
        npages = row_off.size
        lens = np.zeros(npages, dtype=np.int64)
        st = self.lib.gs_encode_pages_dev(
            self._ctx, kind, ctypes.c_void_p(d_vals.data_ptr()),
            ctypes.c_void_p(d_valid.data_ptr()) if d_valid is not None else None,
            _np_ptr(row_off), _np_ptr(rows), npages,
            ctypes.c_void_p(d_out.data_ptr()), cap_per_page, _np_ptr(lens))
        if st != 0:
            e = RuntimeError(
                f"gs_encode_pages_dev failed ({st}): {self._pl.err()}")
            e.status, e.lens = st, lens
            raise e
        return lens

    def encode_group_pages_dev(self, cols, row_off, rows, outs):
        """GPU re-encode of a whole column group (gs_encode_group_pages_dev),
        taking compact_merge_fields' outputs as they are.  cols =
        [(ctype, d_vals, d_valid_or_None), ...] with the time column among
        them; row_off/rows: the page split shared by all columns; outs =
        [(d_out, cap_per_page), ...], page p of column c at
        d_out[p*cap:].  Returns one structured array per column with
        fields len, null_count, min, max ([npages]; min/max in the
        column's dtype, 0 for bool).  The exception of a failed call
        carries .status (GsStatus) and .info (the same list; len < 0
        exactly where a page failed, see cnosdb_gs.h)."""
        if len(cols) != len(outs):
            raise ValueError(f"{len(cols)} columns, {len(outs)} outputs")
        row_off = np.ascontiguousarray(row_off, dtype=np.int64)
        rows = np.ascontiguousarray(rows, dtype=np.int32)
        npages, ncols = row_off.size, len(cols)
        if rows.size != npages:
            raise ValueError("row_off and rows differ in length")

        def ptr(t):
            return t.data_ptr() if t is not None else None

        ct = np.array([c[0] for c in cols], dtype=np.uint8)
        val_p = (ctypes.c_void_p * max(ncols, 1))(*[ptr(c[1]) for c in cols])
        vd_p = None  # whole array NULL: every column all-valid
        if any(c[2] is not None for c in cols):
            vd_p = (ctypes.c_void_p * ncols)(*[ptr(c[2]) for c in cols])
        out_p = (ctypes.c_void_p * max(ncols, 1))(*[ptr(o[0]) for o in outs])
        caps = np.array([o[1] for o in outs], dtype=np.int64)
        raw = np.zeros(max(ncols, 1) * max(npages, 1), dtype=_PAGE_INFO_DT)
        st = self.lib.gs_encode_group_pages_dev(
            self._ctx, ncols, _np_ptr(ct), val_p, vd_p, _np_ptr(row_off),
            _np_ptr(rows), npages, out_p, _np_ptr(caps), _np_ptr(raw))
        info = [raw[c * npages:(c + 1) * npages].view(_page_info_dtype(ct[c]))
                for c in range(ncols)]
        if st != 0:
            e = RuntimeError(
                f"gs_encode_group_pages_dev failed ({st}): {self._pl.err()}")
            e.status, e.info = st, info
            raise e
        return info

    def encode_str_pages_dev(self, d_offsets, d_bytes, row_off, rows, d_out,
                             cap_per_page, d_valid=None):
        """GPU re-encode of a string column's pages
        (gs_encode_str_pages_dev).  d_offsets (int64, rows+1) and d_bytes
        (uint8): the column in Arrow varbinary layout, as decode_str leaves
        it; d_valid: uint8 per row or None.  Page p is written at
        d_out[p*cap_per_page:] and equals str_page_of byte for byte.
        Returns a structured array with fields len, null_count, min, max
        ([npages]); min/max are the absolute ROW INDEX of the page's
        smallest / largest value (bytewise order, smallest row among
        equals), 2**64-1 for a page without a non-null value.  The
        exception of a failed call carries .status (GsStatus)."""
        row_off = np.ascontiguousarray(row_off, dtype=np.int64)
        rows = np.ascontiguousarray(rows, dtype=np.int32)
        npages = row_off.size
        if rows.size != npages:
            raise ValueError("row_off and rows differ in length")
        info = np.zeros(max(npages, 1), dtype=_PAGE_INFO_DT)
        st = self.lib.gs_encode_str_pages_dev(
            self._ctx, ctypes.c_void_p(d_offsets.data_ptr()),
            ctypes.c_void_p(d_bytes.data_ptr()),
            ctypes.c_void_p(d_valid.data_ptr()) if d_valid is not None else None,
            _np_ptr(row_off), _np_ptr(rows), npages,
            ctypes.c_void_p(d_out.data_ptr()), cap_per_page, _np_ptr(info))
        if st != 0:
            e = RuntimeError(
                f"gs_encode_str_pages_dev failed ({st}): {self._pl.err()}")
            e.status = st
            raise e
        return info[:npages]

    def _mk_spec(self, d_ts, d_val, time_range, tombstones, d_out_ts,
                 d_out_val, agg, field_col=0):
        spec = GsScanSpec()
        lo, hi = time_range if time_range else (-(2**63), 2**63 - 1)
        spec.range = GsTimeRange(lo, hi)
        spec.field_col = field_col
        if tombstones:
            tarr = (GsTimeRange * len(tombstones))(*[GsTimeRange(a, b) for a, b in tombstones])
            spec.tombstones = tarr
            spec.n_tombstones = len(tombstones)
            spec._keep = tarr
        if d_ts is not None:
            spec.d_ts = d_ts.data_ptr()
            spec.d_val = d_val.data_ptr()
        if d_out_ts is not None:
            spec.d_out_ts = d_out_ts.data_ptr()
            spec.d_out_val = d_out_val.data_ptr()
        if agg:
            spec.bucket_ns = agg["bucket_ns"]
            spec.t0 = agg["t0"]
            spec.n_buckets = agg["n_buckets"]
            spec.d_agg_max = agg["d_max"].data_ptr()
            spec.d_agg_sum = agg["d_sum"].data_ptr()
            spec.d_agg_count = agg["d_count"].data_ptr()
        return spec

    def scan_async(self, gset, d_out_ts, d_out_val, time_range=None, agg=None,
                   field_col=0):
        """Enqueue the fused scan without synchronizing (fused-capable
        shapes only); pair with scan_wait."""
        spec = self._mk_spec(None, None, time_range, None, d_out_ts,
                             d_out_val, agg, field_col)
        st = self.lib.gs_scan_async(self._ctx, gset._h, ctypes.byref(spec))
        if st != 0:
            raise RuntimeError(f"gs_scan_async failed ({st}): {self._pl.err()}")

    def scan_wait(self, gset):
        res = GsScanResult()
        st = self.lib.gs_scan_wait(self._ctx, gset._h, ctypes.byref(res))
        if st != 0:
            raise RuntimeError(f"gs_scan_wait failed ({st}): {self._pl.err()}")
        return res

    def scan(self, gset, d_ts, d_val, time_range=None, tombstones=None,
             d_out_ts=None, d_out_val=None, agg=None, field_col=0,
             value_pred=None):
        """Fused scan. agg: dict(bucket_ns, t0, n_buckets, d_max, d_sum,
        d_count).  value_pred: (op, a) or ("between", a, b) evaluated like
        DataFilter's pushed expr.  Returns GsScanResult."""
        spec = GsScanSpec()
        spec.field_col = field_col
        if value_pred:
            spec.value_pred.op = PRED_OPS[value_pred[0]]
            spec.value_pred.a = float(value_pred[1])
            spec.value_pred.b = float(value_pred[2]) if len(value_pred) > 2 else 0.0
        lo, hi = time_range if time_range else (-(2**63), 2**63 - 1)
        spec.range = GsTimeRange(lo, hi)
        if tombstones:
            tarr = (GsTimeRange * len(tombstones))(*[GsTimeRange(a, b) for a, b in tombstones])
            spec.tombstones = tarr
            spec.n_tombstones = len(tombstones)
        spec.d_ts = d_ts.data_ptr()
        spec.d_val = d_val.data_ptr()
        if d_out_ts is not None:
            spec.d_out_ts = d_out_ts.data_ptr()
            spec.d_out_val = d_out_val.data_ptr()
        if agg:
            spec.bucket_ns = agg["bucket_ns"]
            spec.t0 = agg["t0"]
            spec.n_buckets = agg["n_buckets"]
            spec.d_agg_max = agg["d_max"].data_ptr()
            spec.d_agg_sum = agg["d_sum"].data_ptr()
            spec.d_agg_count = agg["d_count"].data_ptr()
        res = GsScanResult()
        st = self.lib.gs_scan(self._ctx, gset._h, ctypes.byref(spec),
                              ctypes.byref(res))
        if st != 0:
            raise RuntimeError(f"gs_scan failed ({st}): {self._pl.err()}")
        return res


def prune_column_groups(stats, time_range=None, value_pred=None):
    """Host-side mirror of `filter_column_groups` (tskv/src/reader/
    chunk.rs:12-49): the reference evaluates a DataFusion PruningPredicate
    over per-column-group min/max statistics (PageMeta ValueStatistics,
    tsm/page.rs:599-639) and drops groups no row of which can match.  The
    shim runs this BEFORE gs_groups_upload, so pruned pages are never
    read, uploaded, or decoded (a pruned page's corruption is therefore
    never observed — same as the reference never reading it).

    stats: iterable of (min_ts, max_ts, min_val, max_val); min_val/max_val
    may be None when the field column has no stats (never prunable then).
    time_range: closed interval (lo, hi) (TimeRange semantics,
    common/models/src/predicate/domain.rs:36-39).
    value_pred: ("gt"|"ge"|"lt"|"le"|"eq"|"ne"|"between", a[, b]) with
    PruningPredicate keep-if-maybe semantics (nulls fail predicates but
    other rows may pass, so stats ranges decide only certain misses).

    Returns a list of bools (True = keep), like the reference's indices.
    """
    keep = []
    for st in stats:
        min_ts, max_ts, min_v, max_v = st
        k = True
        if time_range is not None:
            lo, hi = time_range
            if max_ts < lo or min_ts > hi:
                k = False
        if k and value_pred is not None and min_v is not None \
                and max_v is not None:
            op, a = value_pred[0], value_pred[1]
            if op == "gt":
                k = max_v > a
            elif op == "ge":
                k = max_v >= a
            elif op == "lt":
                k = min_v < a
            elif op == "le":
                k = min_v <= a
            elif op == "eq":
                k = min_v <= a <= max_v
            elif op == "ne":
                k = not (min_v == max_v == a)
            elif op == "between":
                b = value_pred[2]
                k = max_v >= a and min_v <= b
        keep.append(bool(k))
    return keep


def fold_page_stats(ts_info, val_info=None, page_ranges=None):
    """Fold the page statistics Engine.encode_group_pages_dev returns into
    the (min_ts, max_ts, min_val, max_val) tuples prune_column_groups
    takes.  ts_info / val_info: one series' per-page records of the time
    column and of one field column (val_info None -> no value stats).
    page_ranges: [(p0, p1), ...] half-open page ranges to fold into one
    tuple each; None -> one tuple per page (a page is one column group).

    A page without a non-null value reports the starting values of the
    reference's loop (min > max), and so does an f64 page that holds only
    NaNs; such a page contributes nothing, and a range without any
    contributing page gets min_val = max_val = None (never prunable)."""
    npages = len(ts_info)
    if page_ranges is None:
        page_ranges = [(p, p + 1) for p in range(npages)]
    out = []
    for p0, p1 in page_ranges:
        t = ts_info[p0:p1]
        min_ts = t["min"].min() if len(t) else np.iinfo(np.int64).max
        max_ts = t["max"].max() if len(t) else np.iinfo(np.int64).min
        min_v = max_v = None
        if val_info is not None:
            v = val_info[p0:p1]
            v = v[v["min"] <= v["max"]]
            if len(v):
                min_v, max_v = v["min"].min().item(), v["max"].max().item()
        out.append((int(min_ts), int(max_ts), min_v, max_v))
    return out


def _bind_groupby(lib):
    import ctypes
    if getattr(lib, "_gb_bound", False):
        return
    lib.gs_groupby_tag.restype = ctypes.c_int
    lib.gs_groupby_tag.argtypes = [
        ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_int,
        ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
        ctypes.c_int, ctypes.POINTER(ctypes.c_int)]
    lib._gb_bound = True


def groupby_tag(engine, gset, n_buckets, d_max, d_sum, d_count,
                cap_gids, tag_col=0):
    """GROUP BY tag over a completed aggregate scan + decoded tag column
    (gs_groupby_tag).  Returns (ngids, tag_rep_rows ndarray)."""
    import ctypes
    _bind_groupby(engine.lib)
    rep = np.zeros(cap_gids, dtype=np.int64)
    ng = ctypes.c_int(0)
    st = engine.lib.gs_groupby_tag(
        engine._ctx, gset._h, tag_col, n_buckets,
        d_max.data_ptr(), d_sum.data_ptr(), d_count.data_ptr(),
        rep.ctypes.data_as(ctypes.c_void_p), cap_gids, ctypes.byref(ng))
    if st != 0:
        raise RuntimeError(f"gs_groupby_tag failed ({st}): {engine._pl.err()}")
    return ng.value, rep[:ng.value]


def _bind_scan_fields(lib):
    import ctypes
    if getattr(lib, "_sf_bound", False):
        return
    lib.gs_scan_fields.restype = ctypes.c_int
    lib.gs_scan_fields.argtypes = [ctypes.c_void_p, ctypes.c_void_p,
                                   ctypes.c_void_p, ctypes.c_void_p,
                                   ctypes.c_int, ctypes.c_void_p]
    lib._sf_bound = True


def scan_fields(engine, gset, fields, d_ts, d_val, time_range,
                d_out_ts, d_out_val, agg=None):
    """Fused multi-field scan (gs_scan_fields): one span/ts pass, then
    decode+aggregate per field.  d_out_val must hold len(fields)*rows
    doubles (field i at offset i*rows); agg buffers len(fields)*n_buckets."""
    import ctypes
    _bind_scan_fields(engine.lib)
    spec = GsScanSpec()
    spec.field_col = fields[0]
    lo, hi = time_range
    spec.range = GsTimeRange(lo, hi)
    spec.d_ts = d_ts.data_ptr()
    spec.d_val = d_val.data_ptr()
    spec.d_out_ts = d_out_ts.data_ptr()
    spec.d_out_val = d_out_val.data_ptr()
    if agg:
        spec.bucket_ns = agg["bucket_ns"]
        spec.t0 = agg["t0"]
        spec.n_buckets = agg["n_buckets"]
        spec.d_agg_max = agg["d_max"].data_ptr()
        spec.d_agg_sum = agg["d_sum"].data_ptr()
        spec.d_agg_count = agg["d_count"].data_ptr()
    fc = (ctypes.c_int32 * len(fields))(*fields)
    res = GsScanResult()
    st = engine.lib.gs_scan_fields(engine._ctx, gset._h, ctypes.byref(spec),
                                   fc, len(fields), ctypes.byref(res))
    if st != 0:
        raise RuntimeError(
            f"gs_scan_fields failed ({st}): {engine._pl.err()}")
    return res


def scan_fields_async(engine, gset, fields, d_ts, d_val, time_range,
                      d_out_ts, d_out_val, agg=None):
    """Async gs_scan_fields; pair with engine.scan_wait(gset)."""
    import ctypes
    _bind_scan_fields(engine.lib)
    if not getattr(engine.lib, "_sfa_bound", False):
        engine.lib.gs_scan_fields_async.restype = ctypes.c_int
        engine.lib.gs_scan_fields_async.argtypes = [
            ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
            ctypes.c_void_p, ctypes.c_int]
        engine.lib._sfa_bound = True
    spec = GsScanSpec()
    spec.field_col = fields[0]
    lo, hi = time_range
    spec.range = GsTimeRange(lo, hi)
    spec.d_ts = d_ts.data_ptr()
    spec.d_val = d_val.data_ptr()
    spec.d_out_ts = d_out_ts.data_ptr()
    spec.d_out_val = d_out_val.data_ptr()
    if agg:
        spec.bucket_ns = agg["bucket_ns"]
        spec.t0 = agg["t0"]
        spec.n_buckets = agg["n_buckets"]
        spec.d_agg_max = agg["d_max"].data_ptr()
        spec.d_agg_sum = agg["d_sum"].data_ptr()
        spec.d_agg_count = agg["d_count"].data_ptr()
    fc = (ctypes.c_int32 * len(fields))(*fields)
    st = engine.lib.gs_scan_fields_async(engine._ctx, gset._h,
                                         ctypes.byref(spec), fc, len(fields))
    if st != 0:
        raise RuntimeError(
            f"gs_scan_fields_async failed ({st}): {engine._pl.err()}")


def filter_tile():
    """FLT_TILE: rows per block of gs_filter_group's kernels (four waves of
    FLT_TILE / 4 rows each), for the tests' edge sizes."""
    return int(PageLib().lib.gs_debug_filter_tile())


def filter_ms():
    """Device time of the last filter_group call, first to last kernel,
    from HIP events on the engine stream (gs_debug_filter_ms)."""
    return float(PageLib().lib.gs_debug_filter_ms())


def agg_ms():
    """Device time of the last agg_group call, first to last kernel, from
    HIP events on the engine stream (gs_debug_agg_ms)."""
    return float(PageLib().lib.gs_debug_agg_ms())


def grid_rounds(reset=False):
    """Largest ceil(uncapped blocks / granted blocks) of any capped launch
    since the last reset (gs_debug_grid_rounds)."""
    return int(PageLib().lib.gs_debug_grid_rounds(1 if reset else 0))


@contextlib.contextmanager
def grid_cap(max_blocks):
    """Test seam: cap every capped kernel launch at max_blocks blocks
    (gs_debug_set_grid_cap), so a small set drives the kernels through
    several trips of their grid-stride loops.  Resets the round counter on
    entry and restores the previous cap on exit, whatever happens inside."""
    lib = PageLib().lib
    prev = lib.gs_debug_set_grid_cap(int(max_blocks))
    lib.gs_debug_grid_rounds(1)
    try:
        yield
    finally:
        lib.gs_debug_set_grid_cap(prev)
