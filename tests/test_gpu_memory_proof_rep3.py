"""GPU tests of the memory check and the output check by three Rep3 parties (cozk_memory_proof_rep3_*, csrc/host/memory_proof_rep3.hpp) at
(log_n, log_mem, n_slots) = (3, 5, 1), (6, 5, 4), (5, 7, 2), each with an io window inside one W' block, one across a W' boundary and the
whole memory: the proof verifies; its bytes equal MemoryProof's PLAIN bytes at with_ts = 0 and the plain-Python restatement
tests/memory_proof_ref.py; windowed 0 and 1 and leaves_fused 0 and 1 give the same bytes; the first prefix_len bytes are RwProofRep3's
proof prefix; tampers 1 and 2 reject with the reasons they have in RwProofRep3, tamper 4 with "output check: final claim" and nothing
else; the refusals of bad configs."""
import pytest

import memory_proof_ref as MP
import rw_proof_ref as P

pytestmark = pytest.mark.gpu
INVALID_ARG = -1
SIZES = [(3, 5, 1), (6, 5, 4), (5, 7, 2)]
# per log_mem: inside one W'-aligned block, across a multiple of W', the whole memory (no sparse round)
WINDOWS = {5: [(3, 5), (13, 9), (0, 32)], 7: [(65, 6), (61, 6), (0, 128)]}
_WANT = {}  # per config: the restatement's proof and the plain harness's bytes, made once for every variant


def _cases():
    return [(n, m, ns, lo, W) for n, m, ns in SIZES for lo, W in WINDOWS[m]]


def _want(cozk, cfg):
    key = tuple(sorted(cfg.items()))
    if key not in _WANT:
        ref = MP.prove(dict(cfg, with_ts=0))
        p = cozk.MemoryProof(with_ts=False, **cfg)
        pres = p.prove(verify=True)
        assert pres.verified == 1, p.last_error()
        _WANT[key] = (ref, p.proof_bytes(pres), bytes(pres.proof_digest), int(pres.prefix_len))
        p.close()
    return _WANT[key]


@pytest.mark.parametrize("windowed", [True, False])
@pytest.mark.parametrize("log_n,log_mem,ns,lo,W", _cases())
def test_proof_verifies_and_its_bytes_are_the_plain_proofs(cozk, log_n, log_mem, ns, lo, W, windowed):
    cfg = dict(log_n=log_n, log_mem=log_mem, n_slots=ns, seed=61 + log_n, io_start=lo, io_len=W)
    ref, plain_bytes, plain_digest, plain_prefix = _want(cozk, cfg)
    h = cozk.MemoryProofRep3(windowed=windowed, **cfg)
    res = h.prove(verify=True)
    assert res.verified == 1, h.last_error()
    got = h.proof_bytes(res)
    assert len(got) == res.proof_len == len(plain_bytes) and res.prefix_len == plain_prefix == ref["prefix_len"]
    assert got == plain_bytes and bytes(res.proof_digest) == plain_digest
    assert got == ref["proof_bytes"]
    assert res.ring_bytes > 0 and res.out_peak_bytes > 0
    for t in (res.wall_ms, res.t_witness_ms, res.t_share_ms, res.t_commit_ms, res.t_leaves_ms, res.t_gp_ms, res.t_out_ms, res.t_open_ms):
        assert t > 0
    h.close()


@pytest.mark.parametrize("windowed", [True, False])
@pytest.mark.parametrize("log_n,log_mem,ns", SIZES)
def test_the_composed_leaves_give_the_same_bytes(cozk, log_n, log_mem, ns, windowed):
    lo, W = WINDOWS[log_mem][1]
    cfg = dict(log_n=log_n, log_mem=log_mem, n_slots=ns, seed=61 + log_n, io_start=lo, io_len=W)
    _, plain_bytes, plain_digest, _ = _want(cozk, cfg)
    h = cozk.MemoryProofRep3(windowed=windowed, leaves_fused=False, **cfg)
    res = h.prove(verify=True)
    assert res.verified == 1, h.last_error()
    assert h.proof_bytes(res) == plain_bytes and bytes(res.proof_digest) == plain_digest
    h.close()


@pytest.mark.parametrize("log_n,log_mem,ns", SIZES)
def test_the_prefix_is_the_rep3_rw_proofs(cozk, log_n, log_mem, ns):
    lo, W = WINDOWS[log_mem][0]
    cfg = dict(log_n=log_n, log_mem=log_mem, n_slots=ns, seed=61 + log_n)
    m = cozk.MemoryProofRep3(io_start=lo, io_len=W, **cfg)
    mr = m.prove(verify=True)
    r = cozk.RwProofRep3(**cfg)
    rr = r.prove(verify=True)
    assert mr.verified == 1 and rr.verified == 1, (m.last_error(), r.last_error())
    mb, rb = m.proof_bytes(mr), r.proof_bytes(rr)
    n = int(mr.prefix_len)
    assert 0 < n < len(rb) and mb[:n] == rb[:n] and mb[n:n + 8] == (log_mem).to_bytes(8, "little")  # the output sumcheck: log_mem rounds
    m.close()
    r.close()


@pytest.mark.parametrize("windowed", [True, False])
@pytest.mark.parametrize("tamper,reason", [(1, P.REASON_MULTISET), (2, P.REASON_LEAF), (4, MP.REASON_OUT_FINAL)])
def test_tampered_proofs_are_rejected_with_their_reason(cozk, tamper, reason, windowed):
    h = cozk.MemoryProofRep3(log_n=6, log_mem=7, seed=81, tamper=tamper, io_start=61, io_len=6, windowed=windowed)
    res = h.prove(verify=True)
    assert res.verified == 0
    if tamper == 4:
        assert h.last_error() == "verification failed: output check: final claim", h.last_error()
    else:
        r = cozk.RwProofRep3(log_n=6, log_mem=7, seed=81, tamper=tamper)
        assert r.prove(verify=True).verified == 0
        assert h.last_error() == r.last_error() and h.last_error().startswith("verification failed: " + reason), (h.last_error(), r.last_error())
        r.close()
    h.close()


def test_two_proves_of_one_handle_give_equal_bytes(cozk):
    h = cozk.MemoryProofRep3(log_n=5, log_mem=7, n_slots=2, seed=91, io_start=61, io_len=6)
    a = h.prove(verify=True)
    b = h.prove(verify=False)
    assert a.verified == 1 and b.verified == -1
    assert h.proof_bytes(b) and bytes(a.proof_digest) == bytes(b.proof_digest) and a.proof_len == b.proof_len and a.prefix_len == b.prefix_len
    h.close()


@pytest.mark.parametrize("kw,text", [(dict(log_n=0), "log_n in 1..22"), (dict(log_mem=25), "log_mem in 5..24"), (dict(n_slots=5), "n_slots in 1..4"),
                                     (dict(leaves_fused=2), "leaves_fused are 0 or 1"), (dict(tamper=5), "tamper in 0..4"), (dict(tamper=3), "3 only with with_ts"),
                                     (dict(io_len=0), "io_len is at least 1 word"), (dict(io_start=60, io_len=5), "io_start + io_len > MEM"),
                                     (dict(windowed=2), "windowed is 0 or 1")])
def test_bad_configs_are_refused(cozk, kw, text):
    with pytest.raises(cozk.CozkError) as e:
        cozk.MemoryProofRep3(**dict(dict(log_n=4, log_mem=6, io_start=3, io_len=5), **kw))
    assert e.value.code == INVALID_ARG and "memory_proof_rep3: " in str(e.value) and text in str(e.value), str(e.value)
