"""GPU: the toggled grand product with its low-density layers stored as sparse pair layers (COZK_TOGGLE_SPARSE=1, csrc/host/prover.hpp)
gives, byte for byte, the proof of the dense path and of the oracle (oracle/pylookups.py); the per-context counters show the sparse
layers, their rounds and exactly one hand-over per sparse layer, and stay zero with the switch off."""
import functools
import hashlib
import importlib

import pytest

import pylookups

pytestmark = pytest.mark.gpu
SHAPES = [dict(log_n=8, n_pairs=3, density_pct=10), dict(log_n=6, n_pairs=5, density_pct=5), dict(log_n=3, n_pairs=5, density_pct=0)]
SEED = 1
ZERO = dict(layers_sparse=0, layers_scattered=0, sparse_rounds=0, handovers=0, bytes_sparse=0, bytes_dense_equivalent=0)


@functools.lru_cache(maxsize=None)
def _oracle(log_n, n_pairs, density_pct, mode):
    ref = pylookups.run(dict(log_n=log_n, n_pairs=n_pairs, density_pct=density_pct, seed=SEED, mode=mode))
    assert ref["verified"]
    return ref["proof_bytes"]


def _stored_pairs_layer0(cfg):
    """from the oracle's flag columns: the pairs of the toggle layer's output with a set flag (both circuits of a memory share them)"""
    n = 1 << cfg["log_n"]
    cols = [pylookups.flag_column(SEED, q, n, cfg["density_pct"]) for q in range(cfg["n_pairs"])]
    return sum(2 for c in cols for i in range(0, n, 2) if c[i] | c[i + 1])


def _prove(h, monkeypatch, switch, verify=True):
    if switch is None:
        monkeypatch.delenv("COZK_TOGGLE_SPARSE", raising=False)
    else:
        monkeypatch.setenv("COZK_TOGGLE_SPARSE", switch)
    res = h.prove(verify=verify)
    if verify:
        assert res.verified == 1, h.last_error()
    return res


@pytest.mark.parametrize("mode", ["plain", "rep3"])
@pytest.mark.parametrize("cfg", SHAPES, ids=lambda c: "2p%d-%dpairs-%dpct" % (c["log_n"], c["n_pairs"], c["density_pct"]))
def test_sparse_switch_gives_the_dense_paths_and_the_oracles_proof(cozk, monkeypatch, mode, cfg):
    LK = importlib.import_module("co-zkvms_amd.lookups")
    n_dense = 2 * cfg["n_pairs"] << cfg["log_n"]
    cnt0 = _stored_pairs_layer0(cfg)
    assert 2 * cnt0 <= n_dense // 2, "the rule does not store layer 0 sparse for this seed: pick another seed"
    h = LK.LookupsHarness(mode=mode, seed=SEED, **cfg)
    nparties = 3 if mode == "rep3" else 1
    # the switch off (unset, then "0"): today's path, every counter zero
    dense = h.proof_bytes(_prove(h, monkeypatch, None))
    assert h.proof_bytes(_prove(h, monkeypatch, "0")) == dense
    for p in range(nparties):
        assert h.sparse_stats(p).as_dict() == ZERO
    # the switch on
    res = _prove(h, monkeypatch, "1")
    got = h.proof_bytes(res)
    assert hashlib.sha256(got).hexdigest() == bytes(res.proof_digest).hex()
    assert got == dense
    assert got == _oracle(cfg["log_n"], cfg["n_pairs"], cfg["density_pct"], mode)
    nc = 2 if mode == "rep3" else 1
    stats = [h.sparse_stats(p).as_dict() for p in range(nparties)]
    for st in stats:
        assert st["layers_sparse"] >= 1 and st["sparse_rounds"] >= st["layers_sparse"]
        assert st["handovers"] == st["layers_sparse"]
        assert st["layers_scattered"] == 1
        assert st["bytes_sparse"] >= cnt0 * (64 * nc + 4) and st["bytes_dense_equivalent"] >= n_dense * 32 * nc
        assert st["bytes_sparse"] < st["bytes_dense_equivalent"]
        assert st == stats[0]  # the pattern is public: every party stores and hands over alike
    # and off again: the counters do not move
    assert h.proof_bytes(_prove(h, monkeypatch, "0", verify=False)) == dense
    assert [h.sparse_stats(p).as_dict() for p in range(nparties)] == stats
    h.reset_sparse_stats()
    assert h.sparse_stats(0).as_dict() == ZERO
    h.close()


def test_2p14_54_memories_sparse_verifies_rep3_equals_plain_equals_dense(cozk, monkeypatch):
    LK = importlib.import_module("co-zkvms_amd.lookups")
    digs = {}
    for mode in ("plain", "rep3"):
        h = LK.LookupsHarness(mode=mode, log_n=14, n_pairs=54, density_pct=10, seed=2026)
        digs[mode] = bytes(_prove(h, monkeypatch, "1").proof_digest)
        st = h.sparse_stats(0).as_dict()
        assert st["layers_sparse"] >= 1 and st["handovers"] == st["layers_sparse"] and 2 * st["bytes_sparse"] < st["bytes_dense_equivalent"]
        if mode == "plain":
            digs["dense"] = bytes(_prove(h, monkeypatch, "0", verify=False).proof_digest)
        h.close()
    assert digs["plain"] == digs["rep3"] == digs["dense"]


@pytest.mark.parametrize("mode", ["plain", "rep3"])
def test_chained_flow_digest_is_the_same_with_the_switch_on_and_off(cozk, monkeypatch, mode):
    FL = importlib.import_module("co-zkvms_amd.flow")
    h = FL.FlowHarness(mode=mode, log_n=5, log_m=3, log_b=4, log_mem=4, n_mem=9, n_subtables=4, seed=7)
    off = _prove(h, monkeypatch, "0")
    on = _prove(h, monkeypatch, "1")
    assert bytes(on.proof_digest) == bytes(off.proof_digest) and h.proof_bytes(on) == h.proof_bytes(off)
    h.close()
