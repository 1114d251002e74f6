"""CPU test of the read-write memory witness surface: the python binding's symbols are declared in include/cozk.h and exported by
the library, and the package exports the call (no GPU needed)."""
import importlib
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_rw_memory_symbols_declared_and_exported(cozk):
    RW = importlib.import_module("co-zkvms_amd.rw_memory")
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "cozk.h")).read(), flags=re.S)
    lib = cozk._lib.lib()
    assert RW.RW_MEMORY_SYMBOLS and cozk.RW_MEMORY_SYMBOLS == RW.RW_MEMORY_SYMBOLS and cozk.rw_memory_witness is RW.rw_memory_witness
    for n in RW.RW_MEMORY_SYMBOLS:
        assert re.search(r"\b%s\s*\(" % n, header), n
        assert hasattr(lib, n), n
    assert RW.RW_MEMORY_MAX_SLOTS == int(re.search(r"#define COZK_RW_MEMORY_MAX_SLOTS (\d+)", header).group(1))
