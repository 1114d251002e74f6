"""CPU test: the sparse pair layer entry points (cozk_sparse_layer_*, cozk_toggle_sparse_output, cozk_sparse_*_stats) are exported by
the built library, declared in include/cozk.h with the argument lists the python layer binds, and wrapped by lookups.SparseLayer (no
compute calls -- there is no GPU here)."""
import ctypes
import importlib
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# name -> (return type, number of parameters) as include/cozk.h declares them
SYMBOLS = {"cozk_sparse_layer_create": ("int", 8), "cozk_toggle_sparse_output": ("int", 4), "cozk_sparse_layer_free": ("int", 1),
           "cozk_sparse_layer_len": ("size_t", 1), "cozk_sparse_layer_count": ("size_t", 1), "cozk_sparse_layer_bytes": ("size_t", 1),
           "cozk_sparse_layer_next_count": ("int", 3), "cozk_sparse_layer_output_local": ("int", 7), "cozk_sparse_layer_from_output": ("int", 6),
           "cozk_sparse_layer_bind": ("int", 3), "cozk_sparse_layer_round": ("int", 6), "cozk_sparse_layer_to_dense": ("int", 4),
           "cozk_sparse_layer_download": ("int", 5), "cozk_sparse_get_stats": ("int", 2), "cozk_sparse_reset_stats": ("int", 1)}
STATS_FIELDS = ["layers_sparse", "layers_scattered", "sparse_rounds", "handovers", "bytes_sparse", "bytes_dense_equivalent"]


def _header():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "cozk.h")).read(), flags=re.S)


def test_sparse_layer_symbols_exported_declared_and_bound(cozk):
    lib = cozk._lib.lib()
    src = _header()
    for name, (ret, nargs) in SYMBOLS.items():
        assert hasattr(lib, name), name
        m = re.search(r"\b%s\s+%s\s*\(([^;]*?)\)\s*;" % (ret, name), src, flags=re.S)
        assert m, name
        assert len(m.group(1).split(",")) == nargs, name
        res, args = cozk._lib.SIGNATURES[name]
        assert len(args) == nargs, name
        assert res is (ctypes.c_int if ret == "int" else ctypes.c_size_t), name
    assert re.search(r"typedef\s+struct\s+cozk_sparse_layer\s+cozk_sparse_layer\s*;", src)
    stats = re.search(r"typedef\s+struct\s+cozk_sparse_stats\s*\{(.*?)\}\s*cozk_sparse_stats\s*;", src, flags=re.S)
    assert stats and re.sub(r"\s+", " ", stats.group(1)).strip() == "uint64_t " + ", ".join(STATS_FIELDS) + ";"
    assert [f[0] for f in cozk.SparseStats._fields_] == STATS_FIELDS
    assert ctypes.sizeof(cozk.SparseStats) == 8 * len(STATS_FIELDS)


def test_python_layer_has_the_sparse_layer(cozk):
    lookups = importlib.import_module("co-zkvms_amd.lookups")
    assert cozk.SparseLayer is lookups.SparseLayer
    for name in ("from_toggle", "from_lists", "from_vecs", "next_count", "output_local", "from_output", "bind", "round", "to_dense", "download", "free"):
        assert callable(getattr(lookups.SparseLayer, name)), name
    for name in ("count", "nbytes"):
        assert isinstance(getattr(lookups.SparseLayer, name), property), name
    assert callable(cozk.sparse_stats) and callable(cozk.sparse_reset_stats)


def test_null_handles_are_refused_on_the_host(cozk):
    l = cozk._lib.lib()
    bad = -1  # COZK_ERR_INVALID_ARG
    h = ctypes.c_void_p(0x5A5A)
    assert l.cozk_sparse_layer_create(None, 1, 4, None, None, None, 0, ctypes.byref(h)) == bad and h.value is None
    h = ctypes.c_void_p(0x5A5A)
    assert l.cozk_toggle_sparse_output(None, None, 0, ctypes.byref(h)) == bad and h.value is None
    h = ctypes.c_void_p(0x5A5A)
    assert l.cozk_sparse_layer_output_local(None, None, 0, None, None, 0, ctypes.byref(h)) == bad and h.value is None
    h = ctypes.c_void_p(0x5A5A)
    assert l.cozk_sparse_layer_from_output(None, None, None, None, 0, ctypes.byref(h)) == bad and h.value is None
    h = ctypes.c_void_p(0x5A5A)
    assert l.cozk_sparse_layer_to_dense(None, None, 0, ctypes.byref(h)) == bad and h.value is None
    n = ctypes.c_size_t(7)
    assert l.cozk_sparse_layer_next_count(None, None, ctypes.byref(n)) == bad and n.value == 0
    assert l.cozk_sparse_layer_bind(None, None, None) == bad
    assert l.cozk_sparse_layer_round(None, None, None, None, 0, None) == bad
    assert l.cozk_sparse_layer_download(None, None, None, None, None) == bad
    assert l.cozk_sparse_get_stats(None, None) == bad
    assert l.cozk_sparse_reset_stats(None) == bad
    assert l.cozk_sparse_layer_free(None) == 0
    assert l.cozk_sparse_layer_len(None) == 0 and l.cozk_sparse_layer_count(None) == 0 and l.cozk_sparse_layer_bytes(None) == 0
