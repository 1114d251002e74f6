"""CPU test: the layer-group entry points and the Shamir provers' stats getter are exported by the built library, declared in
include/cozk.h and bound by the python layer; COZK_LAYER_GROUP_MAX is 32 (no compute calls -- there is no GPU here)."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ["cozk_layer_group_create", "cozk_layer_group_round", "cozk_layer_group_final", "cozk_layer_group_free", "cozk_shamir_gp_get_stats"]


def _header():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "cozk.h")).read(), flags=re.S)


def test_layer_group_symbols_exported_and_declared(cozk):
    lib = cozk._lib.lib()
    src = _header()
    for name in NEW_SYMBOLS:
        assert hasattr(lib, name), name
        assert re.search(r"\bint\s+%s\s*\(" % name, src), name
        assert name in cozk._lib.SIGNATURES, name
    assert re.search(r"typedef\s+struct\s+cozk_layer_group\s+cozk_layer_group\s*;", src)
    stats = re.search(r"typedef\s+struct\s+cozk_shamir_gp_stats\s*\{(.*?)\}\s*cozk_shamir_gp_stats\s*;", src, flags=re.S)
    assert stats and re.sub(r"\s+", " ", stats.group(1)).strip() == "uint64_t group_rounds, single_rounds, group_finals, single_finals;"
    assert [f[0] for f in cozk.ShamirGpStats._fields_] == ["group_rounds", "single_rounds", "group_finals", "single_finals"]


def test_layer_group_max_is_32(cozk):
    src = _header()
    m = re.search(r"#define\s+COZK_LAYER_GROUP_MAX\s+(\d+)", src)
    assert m and int(m.group(1)) == 32
    m = re.search(r"#define\s+COZK_SHAMIR_MAX_PARTIES\s+(\d+)", src)
    assert m and int(m.group(1)) == 32  # a group holds every sender of the largest Shamir prover
    assert cozk._lib.LAYER_GROUP_MAX == 32
