"""CPU test: the outer-group and shift-group entry points and the Shamir Jolt-Spartan prover are exported by the built library,
declared in include/cozk.h and bound by the python layer (no compute calls -- there is no GPU here)."""
import ctypes
import re

import pytest

import test_spartan_group_abi as A  # the header reader and the struct-layout parser


def test_group_symbols_exported_declared_and_bound(cozk):
    lib = cozk._lib.lib()
    src = A._header()
    mod = cozk.shamir_jolt_spartan
    assert len(mod.OUTER_GROUP_SYMBOLS) == 5 and len(mod.SHIFT_GROUP_SYMBOLS) == 6
    for name in mod.OUTER_GROUP_SYMBOLS + mod.SHIFT_GROUP_SYMBOLS:
        assert hasattr(lib, name), name
        assert re.search(r"\b(int|size_t)\s+%s\s*\(" % name, src), name
        assert name in cozk._lib.SIGNATURES, name
    for ty in ("cozk_outer_group", "cozk_shift_group"):
        assert re.search(r"typedef\s+struct\s+%s\s+%s\s*;" % (ty, ty), src)
    assert cozk.OuterGroup is mod.OuterGroup and cozk.ShiftGroup is mod.ShiftGroup
    m = re.search(r"#define\s+COZK_LAYER_GROUP_MAX\s+(\d+)", src)
    assert m and int(m.group(1)) == mod.MAX_PARTIES == 32


def test_group_signatures_match_the_header(cozk):
    """argument counts and return types of the bound signatures against the declarations"""
    src = A._header()
    mod = cozk.shamir_jolt_spartan
    for name in mod.OUTER_GROUP_SYMBOLS + mod.SHIFT_GROUP_SYMBOLS:
        m = re.search(r"\b(int|size_t)\s+%s\s*\(([^)]*)\)" % name, src)
        res, args = cozk._lib.SIGNATURES[name]
        assert res is (ctypes.c_int if m.group(1) == "int" else ctypes.c_size_t), name
        decl = [a.strip() for a in m.group(2).split(",")]
        assert len(decl) == len(args), name
        for d, a in zip(decl, args):
            if "*" in d or "[" in d:
                assert a in (ctypes.c_void_p, ctypes.POINTER(ctypes.c_void_p)), (name, d)
            else:
                assert d.startswith("int ") and a is ctypes.c_int, (name, d)


def test_shamir_jolt_spartan_symbols_exported_declared_and_bound(cozk):
    lib = cozk._lib.lib()
    src = A._header()
    mod = cozk.shamir_jolt_spartan
    for name in mod.SHAMIR_JOLT_SPARTAN_SYMBOLS:
        assert hasattr(lib, name), name
        assert re.search(r"\b%s\s*\(" % name, src), name
    bound = {mod.ShamirJoltSpartanHarness.PREFIX + s for s in ("_create", "_error", "_destroy", "_prove", "_proof_bytes")} | set(mod.ShamirJoltSpartanHarness.EXTRA)
    assert bound == set(mod.SHAMIR_JOLT_SPARTAN_SYMBOLS)
    mod.ShamirJoltSpartanHarness._decl()  # every symbol resolves


def test_config_and_result_layouts_match_the_header(cozk):
    src = A._header()
    mod = cozk.shamir_jolt_spartan
    ctype = {"uint64_t": ctypes.c_uint64, "int": ctypes.c_int, "double": ctypes.c_double, "uint8_t": ctypes.c_uint8}
    for cname, cls in (("cozk_shamir_jolt_spartan_config", mod.ShamirJoltSpartanConfig), ("cozk_shamir_jolt_spartan_result", mod.ShamirJoltSpartanResult)):
        want = A._struct_fields(src, cname)
        got = [(f[0], f[1]) for f in cls._fields_]
        assert [n for _, n in want] == [n for n, _ in got], cname
        for (ty, n), (_, ct) in zip(want, got):
            base = ct._type_ if hasattr(ct, "_length_") else ct
            assert base is ctype[ty], (cname, n)
    assert mod.ShamirJoltSpartanConfig.devices.size == 4 * 32 and mod.ShamirJoltSpartanResult.proof_digest.size == 32
    assert ctypes.sizeof(mod.ShamirJoltSpartanConfig) == 4 * 4 + 4 * 32 + 3 * 8
    assert ctypes.sizeof(mod.ShamirJoltSpartanResult) == 8 + 8 + 32 + 8 + 7 * 8


_BAD = [
    (dict(degree=0), "1 <= degree and 2 * degree <= COZK_SHAMIR_MAX_DEGREE"),
    (dict(degree=8, parties=17), "1 <= degree and 2 * degree <= COZK_SHAMIR_MAX_DEGREE"),
    (dict(degree=2, parties=4), "2 * degree + 1 <= num_parties <= COZK_SHAMIR_MAX_PARTIES"),
    (dict(degree=1, parties=33), "2 * degree + 1 <= num_parties <= COZK_SHAMIR_MAX_PARTIES"),
    (dict(log_steps=-1), "log_steps out of range (0..24)"),
    (dict(log_steps=25), "log_steps out of range (0..24)"),
    (dict(system=2), "system is 0 (toy) or 1 (the Jolt constraint set)"),
]


@pytest.mark.parametrize("kw,text", _BAD, ids=[t[:24] + str(i) for i, (_, t) in enumerate(_BAD)])
def test_create_refuses_bad_configs_before_any_context(cozk, kw, text):
    with pytest.raises(cozk.CozkError) as e:
        cozk.ShamirJoltSpartanHarness(**kw)
    assert e.value.code == -1 and "shamir_jolt_spartan: " in str(e.value) and text in str(e.value)
