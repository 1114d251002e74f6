"""CPU test: libcozk.so loads and exports every symbol include/cozk.h declares (no compute calls --
there is no GPU here), and the product refuses to run without a device (no CPU fallback)."""
import ctypes
import importlib
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _declared_symbols():
    src = open(os.path.join(ROOT, "include", "cozk.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(cozk_[a-z0-9_]+)\s*\(", src)))


def test_header_symbols_exported(cozk):
    lib = cozk._lib.lib()
    names = _declared_symbols()
    assert len(names) > 60
    missing = [n for n in names if not hasattr(lib, n)]
    assert not missing, missing
    # every symbol the python layer binds is declared in the header
    from importlib import import_module
    hp = import_module("co-zkvms_amd.harness")
    wk = import_module("co-zkvms_amd.workers")
    for n in list(cozk._lib.SIGNATURES) + hp.HARNESS_SYMBOLS + wk.WORKER_SYMBOLS + importlib.import_module("co-zkvms_amd.party_dist").PARTY_SYMBOLS + importlib.import_module("co-zkvms_amd.spartan").SPARTAN_SYMBOLS + importlib.import_module("co-zkvms_amd.lookups").LOOKUPS_SYMBOLS + importlib.import_module("co-zkvms_amd.outer").OUTER_SYMBOLS + importlib.import_module("co-zkvms_amd.flow").FLOW_SYMBOLS + importlib.import_module("co-zkvms_amd.logup").LOGUP_SYMBOLS:
        assert n in names, n


def test_no_cpu_fallback(cozk):
    n = ctypes.c_int(-1)
    rc = cozk._lib.lib().cozk_device_count(ctypes.byref(n))
    if rc == 0 and n.value > 0:
        pytest.skip("a GPU is visible here")
    with pytest.raises(cozk.CozkError):
        cozk.Context(0)
    with pytest.raises(cozk.CozkError):
        cozk.Harness(mode="plain", log_n=4, n_fr=1, n_u16=0, n_u32=0, n_flags=0, gp_batch=1)


def test_product_never_imports_oracle():
    pkg = os.path.join(ROOT, "co-zkvms_amd")
    for dp, _, files in os.walk(pkg):
        for f in files:
            if f.endswith((".py", ".hip", ".hpp", ".inc")):
                txt = open(os.path.join(dp, f), errors="ignore").read()
                assert "pyref" not in txt.replace("oracle/pyref.py", "") or f.endswith((".hip", ".hpp")), f
                assert "import pyharness" not in txt and "coracle" not in txt and "liboracle" not in txt, f


# one out-of-range config per harness: create rejects it before any context exists (no GPU needed), reports the check's
# text through *_error and destroys the half-built harness
_BAD_CONFIGS = [
    ("harness", "Harness", dict(log_n=30), "harness: log_n out of range"),
    ("spartan", "SpartanHarness", dict(log_n=4, log_pub_workers=4), "spartan: log_pub_workers out of range (0..3)"),
    ("lookups", "LookupsHarness", dict(density_pct=101), "lookups: log_n in 1..24, n_pairs in 1..128, density_pct in 0..100"),
    ("outer", "OuterHarness", dict(log_steps=23), "outer harness: log_steps in 0..22"),
    ("flow", "FlowHarness", dict(log_n=23), "flow: log_n in 1..22"),
    ("party_dist", "DistributedParty", dict(party=3), "harness_create_participant: bad (party, worker)"),
]


@pytest.mark.parametrize("module,cls,kw,text", _BAD_CONFIGS, ids=[c[1] for c in _BAD_CONFIGS])
def test_harness_rejects_bad_config(cozk, module, cls, kw, text):
    harness_cls = getattr(importlib.import_module("co-zkvms_amd." + module), cls)
    with pytest.raises(cozk.CozkError) as e:
        harness_cls(**kw)
    assert e.value.code == -1  # COZK_ERR_INVALID_ARG
    assert text in str(e.value)
