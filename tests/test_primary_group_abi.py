"""CPU test: the primary level-group entry points and the Shamir primary prover are exported by the built library, declared in
include/cozk.h and bound by the python layer; every refusal that needs no device (no compute calls -- there is no GPU here)."""
import ctypes
import re

import pytest

import test_spartan_group_abi as A  # the header reader and the struct-layout parser

INVALID = -1


def test_group_symbols_exported_declared_and_bound(cozk):
    lib = cozk._lib.lib()
    src = A._header()
    mod = cozk.shamir_primary
    assert len(mod.PRIMARY_GROUP_SYMBOLS) == 6
    for name in mod.PRIMARY_GROUP_SYMBOLS:
        assert hasattr(lib, name), name
        assert re.search(r"\b(int|size_t)\s+%s\s*\(" % name, src), name
        assert name in cozk._lib.SIGNATURES, name
    assert re.search(r"typedef\s+struct\s+cozk_primary_group\s+cozk_primary_group\s*;", src)
    LK = __import__("importlib").import_module("co-zkvms_amd.lookups")
    assert cozk.PrimaryGroup is LK.PrimaryGroup is mod.PrimaryGroup
    m = re.search(r"#define\s+COZK_PRIMARY_GROUP_MAX\s+(\d+)", src)
    d = re.search(r"#define\s+COZK_SHAMIR_MAX_DEGREE\s+(\d+)", src)
    assert m and d and int(m.group(1)) == LK.PRIMARY_GROUP_MAX == 15
    assert int(m.group(1)) % 2 == 1 and int(m.group(1)) - 1 <= int(d.group(1))  # k = 2t + 1 with 2t <= COZK_SHAMIR_MAX_DEGREE


def test_group_signatures_match_the_header(cozk):
    """argument counts and return types of the bound signatures against the declarations"""
    src = A._header()
    for name in cozk.shamir_primary.PRIMARY_GROUP_SYMBOLS:
        m = re.search(r"\b(int|size_t)\s+%s\s*\(([^)]*)\)" % name, src)
        res, args = cozk._lib.SIGNATURES[name]
        assert res is (ctypes.c_int if m.group(1) == "int" else ctypes.c_size_t), name
        decl = [a.strip() for a in m.group(2).split(",")]
        assert len(decl) == len(args), name
        for d, a in zip(decl, args):
            if "*" in d or "[" in d:
                assert a in (ctypes.c_void_p, ctypes.POINTER(ctypes.c_void_p), ctypes.c_char_p, ctypes.POINTER(ctypes.c_size_t)), (name, d)
            elif d.startswith("uint64_t "):
                assert a is ctypes.c_uint64, (name, d)
            else:
                assert d.startswith("int ") and a is ctypes.c_int, (name, d)


def test_shamir_primary_symbols_exported_declared_and_bound(cozk):
    lib = cozk._lib.lib()
    src = A._header()
    mod = cozk.shamir_primary
    assert len(mod.SHAMIR_PRIMARY_SYMBOLS) == 10
    for name in mod.SHAMIR_PRIMARY_SYMBOLS:
        assert hasattr(lib, name), name
        assert re.search(r"\b%s\s*\(" % name, src), name
    bound = {mod.ShamirPrimary.PREFIX + s for s in ("_create", "_error", "_destroy", "_prove", "_proof_bytes")} | set(mod.ShamirPrimary.EXTRA)
    assert bound == set(mod.SHAMIR_PRIMARY_SYMBOLS)
    mod.ShamirPrimary._decl()  # every symbol resolves
    assert cozk.ShamirPrimary is mod.ShamirPrimary


def test_config_and_result_layouts_match_the_header(cozk):
    src = A._header()
    mod = cozk.shamir_primary
    ctype = {"uint64_t": ctypes.c_uint64, "int": ctypes.c_int, "double": ctypes.c_double, "uint8_t": ctypes.c_uint8}
    for cname, cls in (("cozk_shamir_primary_config", mod.ShamirPrimaryConfig), ("cozk_shamir_primary_result", mod.ShamirPrimaryResult)):
        want = A._struct_fields(src, cname)
        got = [(f[0], f[1]) for f in cls._fields_]
        assert [n for _, n in want] == [n for n, _ in got], cname
        for (ty, n), (_, ct) in zip(want, got):
            base = ct._type_ if hasattr(ct, "_length_") else ct
            assert base is ctype[ty], (cname, n)
    assert mod.ShamirPrimaryConfig.devices.size == 4 * 32 and mod.ShamirPrimaryResult.proof_digest.size == 32
    assert ctypes.sizeof(mod.ShamirPrimaryConfig) == 5 * 4 + 4 * 32 + 4 + 4 * 8 + 8  # 4 bytes of padding before seed, 4 after tamper_final
    assert ctypes.sizeof(mod.ShamirPrimaryResult) == 16 + 8 + 32 + 3 * 8 + 5 * 8


def test_group_calls_refuse_null_handles_without_a_device(cozk):
    lib = cozk._lib.lib()
    out = ctypes.c_void_p(1234)
    members = (ctypes.c_void_p * 3)()
    keys = bytes(3 * 32)
    assert lib.cozk_primary_group_create(None, members, 3, keys, ctypes.byref(out)) == INVALID  # no driver
    assert out.value is None  # *out is NULL after a refusal
    assert lib.cozk_primary_group_create(None, members, 3, keys, None) == INVALID
    n = ctypes.c_size_t(77)
    assert lib.cozk_primary_group_level(None, 1, 0, ctypes.byref(n)) == INVALID and n.value == 77
    buf = (ctypes.c_uint64 * 4)()
    assert lib.cozk_primary_group_round_finish(None, buf) == INVALID and list(buf) == [0] * 4
    ptr = ctypes.c_void_p(5)
    assert lib.cozk_primary_group_level_buffer(None, 0, 1, ctypes.byref(ptr), ctypes.byref(n)) == INVALID and ptr.value == 5
    assert lib.cozk_primary_group_len(None) == 0
    assert lib.cozk_primary_group_free(None) == 0


def test_prover_calls_refuse_null_handles(cozk):
    mod = cozk.shamir_primary
    lib = mod.ShamirPrimary._decl()
    res = mod.ShamirPrimaryResult()
    assert lib.cozk_shamir_primary_create(None, None) == INVALID
    assert lib.cozk_shamir_primary_prove(None, 1, ctypes.byref(res)) == INVALID
    assert lib.cozk_shamir_primary_msgs_len(None) == 0 and lib.cozk_shamir_primary_finals_len(None) == 0
    assert lib.cozk_shamir_primary_msgs(None, None, 0) == INVALID and lib.cozk_shamir_primary_finals(None, None, 0) == INVALID
    assert lib.cozk_shamir_primary_get_stats(None, None) == INVALID
    assert lib.cozk_shamir_primary_destroy(None) == 0


_BAD = [
    (dict(degree=0), "1 <= degree and 2 * degree <= COZK_SHAMIR_MAX_DEGREE"),
    (dict(degree=8, parties=17), "1 <= degree and 2 * degree <= COZK_SHAMIR_MAX_DEGREE"),
    (dict(degree=2, parties=4), "2 * degree + 1 <= num_parties <= COZK_SHAMIR_MAX_PARTIES"),
    (dict(degree=1, parties=33), "2 * degree + 1 <= num_parties <= COZK_SHAMIR_MAX_PARTIES"),
    (dict(log_n=0), "log_n out of range (1..24)"),
    (dict(log_n=25), "log_n out of range (1..24)"),
    (dict(n_mem=0), "n_mem out of range (1..128)"),
    (dict(n_mem=129), "n_mem out of range (1..128)"),
    (dict(mix=2), "mix is 0 (uniform) or 1 (sha2-shaped)"),
]


@pytest.mark.parametrize("kw,text", _BAD, ids=[t[:24] + str(i) for i, (_, t) in enumerate(_BAD)])
def test_create_refuses_bad_configs_before_any_context(cozk, kw, text):
    with pytest.raises(cozk.CozkError) as e:
        cozk.ShamirPrimary(**kw)
    assert e.value.code == INVALID and "shamir_primary: " in str(e.value) and text in str(e.value)
