"""gs_compact_merge_fields without a device: the entry is exported, bound,
and rejects bad arguments before any device work."""
import ctypes

import cnosdb_amd as gs


def test_library_exports_entry():
    lib = ctypes.CDLL(gs.lib_path())
    assert hasattr(lib, "gs_compact_merge_fields")


def test_null_context_is_gs_err():
    pl = gs.PageLib()
    fn = pl.lib.gs_compact_merge_fields
    assert fn.restype is ctypes.c_int32 and len(fn.argtypes) == 13
    rows = ctypes.c_int64(-7)
    st = fn(None, None, 1, 1, None, None, None, None, None, None, None, None,
            ctypes.byref(rows))
    assert st == -1  # GS_ERR
    assert "gs_compact_merge_fields" in pl.err()
    assert rows.value == -7


def test_engine_method_exists():
    assert callable(getattr(gs.Engine, "compact_merge_fields"))
