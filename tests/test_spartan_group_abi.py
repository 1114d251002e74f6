"""CPU test: the Spartan-group entry points and the Shamir Spartan prover are exported by the built library, declared in
include/cozk.h and bound by the python layer (no compute calls -- there is no GPU here)."""
import ctypes
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GROUP_SYMBOLS = ["cozk_spartan_group_create", "cozk_spartan_group_round", "cozk_spartan_group_final", "cozk_spartan_group_len",
                 "cozk_spartan_group_pub_download", "cozk_spartan_group_free"]


def _header():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "cozk.h")).read(), flags=re.S)


def test_spartan_group_symbols_exported_declared_and_bound(cozk):
    lib = cozk._lib.lib()
    src = _header()
    for name in GROUP_SYMBOLS:
        assert hasattr(lib, name), name
        assert re.search(r"\b(int|size_t)\s+%s\s*\(" % name, src), name
        assert name in cozk._lib.SIGNATURES, name
    assert re.search(r"typedef\s+struct\s+cozk_spartan_group\s+cozk_spartan_group\s*;", src)
    for macro, val in (("COZK_SPARTAN_GROUP_FIRST", 1), ("COZK_SPARTAN_GROUP_SECOND", 2)):
        m = re.search(r"#define\s+%s\s+(\d+)" % macro, src)
        assert m and int(m.group(1)) == val
    assert (cozk._lib.SPARTAN_GROUP_FIRST, cozk._lib.SPARTAN_GROUP_SECOND) == (1, 2)
    assert cozk.SpartanGroup is not None


def test_shamir_spartan_symbols_exported_declared_and_bound(cozk):
    lib = cozk._lib.lib()
    src = _header()
    mod = cozk.shamir_spartan
    for name in mod.SHAMIR_SPARTAN_SYMBOLS:
        assert hasattr(lib, name), name
        assert re.search(r"\b%s\s*\(" % name, src), name
    bound = {mod.ShamirSpartanHarness.PREFIX + s for s in ("_create", "_error", "_destroy", "_prove", "_proof_bytes")} | set(mod.ShamirSpartanHarness.EXTRA)
    assert bound == set(mod.SHAMIR_SPARTAN_SYMBOLS)
    mod.ShamirSpartanHarness._decl()  # every symbol resolves


def _struct_fields(src, name):
    m = re.search(r"typedef\s+struct\s+%s\s*\{(.*?)\}\s*%s\s*;" % (name, name), src, flags=re.S)
    assert m, name
    out = []
    for decl in m.group(1).split(";"):
        decl = decl.strip()
        if not decl:
            continue
        ty = re.match(r"(uint64_t|uint8_t|int|double)", decl).group(1)
        for nm in decl[len(ty):].split(","):
            out.append((ty, re.sub(r"\[.*\]", "", nm).strip()))
    return out


def test_config_and_result_layouts_match_the_header(cozk):
    src = _header()
    mod = cozk.shamir_spartan
    ctype = {"uint64_t": ctypes.c_uint64, "int": ctypes.c_int, "double": ctypes.c_double, "uint8_t": ctypes.c_uint8}
    for cname, cls in (("cozk_shamir_spartan_config", mod.ShamirSpartanConfig), ("cozk_shamir_spartan_result", mod.ShamirSpartanResult)):
        want = _struct_fields(src, cname)
        got = [(f[0], f[1]) for f in cls._fields_]
        assert [n for _, n in want] == [n for n, _ in got], cname
        for (ty, n), (_, ct) in zip(want, got):
            base = ct._type_ if hasattr(ct, "_length_") else ct
            assert base is ctype[ty], (cname, n)
    assert mod.ShamirSpartanConfig.devices.size == 4 * 32 and mod.ShamirSpartanResult.proof_digest.size == 32
