"""CPU test of the time-counter / timestamp range-check witness surface: the python binding's symbols are declared in include/cozk.h
and exported by the library, and the package exports both calls (no GPU needed)."""
import importlib
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_ts_range_symbols_declared_and_exported(cozk):
    TS = importlib.import_module("co-zkvms_amd.ts_range")
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "cozk.h")).read(), flags=re.S)
    lib = cozk._lib.lib()
    assert TS.TS_RANGE_SYMBOLS == ["cozk_time_counters", "cozk_timestamp_range_witness"] and cozk.TS_RANGE_SYMBOLS == TS.TS_RANGE_SYMBOLS
    assert cozk.time_counters is TS.time_counters and cozk.timestamp_range_witness is TS.timestamp_range_witness
    for n in TS.TS_RANGE_SYMBOLS:
        assert re.search(r"\b%s\s*\(" % n, header), n
        assert hasattr(lib, n), n
    assert TS.TIME_COUNTERS_MAX_COLS == int(re.search(r"#define COZK_TIME_COUNTERS_MAX_COLS (\d+)", header).group(1))
    assert TS.TIME_COUNTERS_MAX_COLS >= 2 * cozk.rw_memory.RW_MEMORY_MAX_SLOTS  # the witness is two columns per slot
