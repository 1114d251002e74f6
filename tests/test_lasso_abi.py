"""CPU test of the Lasso-witness surface: the python binding's symbols are declared in include/cozk.h and exported, and the flow
refuses its consistent-lookups mode at any table but Jolt's 2^16 before a context exists (no GPU needed)."""
import importlib
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_lasso_symbols_declared_and_exported(cozk):
    LS = importlib.import_module("co-zkvms_amd.lasso")
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "cozk.h")).read(), flags=re.S)
    lib = cozk._lib.lib()
    for n in LS.LASSO_SYMBOLS:
        assert re.search(r"\b%s\s*\(" % n, header), n
        assert hasattr(lib, n), n
    tile = int(re.search(r"#define COZK_LASSO_TILE (\d+)", header).group(1))
    assert LS.LASSO_TILE == tile and 64 <= tile <= 32768  # in-tile counts fit the 16-bit counters of the rank kernel


@pytest.mark.parametrize("kw,text", [(dict(lookups_witness=1, log_m=12), "flow: lookups_witness needs log_m == 16"),
                                     (dict(lookups_tamper=1, log_m=16), "flow: lookups_tamper in 0..2^log_m, with lookups_witness"),
                                     (dict(lookups_witness=1, log_n=23, log_m=16), "flow: log_n in 1..22")])
def test_flow_refuses_bad_consistent_lookups_config(cozk, kw, text):
    FL = importlib.import_module("co-zkvms_amd.flow")
    with pytest.raises(cozk.CozkError) as e:
        FL.FlowHarness(**dict(dict(mode="plain", log_n=16, log_b=8, log_mem=8), **kw))
    assert e.value.code == -1 and text in str(e.value)
