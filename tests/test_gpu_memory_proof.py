"""GPU tests of the whole read-write memory proof (cozk_memory_proof_*, csrc/host/memory_proof.hpp): proof bytes equal to the plain-Python
restatement tests/memory_proof_ref.py byte for byte at (log_n, log_mem, n_slots, with_ts) = (1, 5, 4, 1), (3, 7, 3, 0) and (6, 5, 4, 1),
each with an unaligned io window; verified proofs at (10, 10) and (16, 14) with the windowed and the dense output check and equal
digests; tampers 1-4 rejected with their reasons; proof[:prefix_len] equal to the same prefix of RwProof's bytes; two proves of one
handle; and the refusals of bad configs."""
import pytest

import memory_proof_ref as MP
import rw_proof_ref as P

pytestmark = pytest.mark.gpu
INVALID_ARG = -1
_WANT = {}  # the restatement's proof per config, made once for both output-check paths


@pytest.mark.parametrize("windowed", [True, False])
@pytest.mark.parametrize("log_n,log_mem,ns,with_ts,lo,W", [(1, 5, 4, 1, 3, 5), (3, 7, 3, 0, 61, 6), (6, 5, 4, 1, 13, 9)])
def test_proof_bytes_equal_the_python_restatement(cozk, log_n, log_mem, ns, with_ts, lo, W, windowed):
    cfg = dict(log_n=log_n, log_mem=log_mem, n_slots=ns, with_ts=with_ts, seed=61 + log_n, io_start=lo, io_len=W)
    key = tuple(sorted(cfg.items()))
    if key not in _WANT:
        _WANT[key] = MP.prove(cfg)
    want = _WANT[key]
    h = cozk.MemoryProof(windowed=windowed, **cfg)
    res = h.prove(verify=True)
    assert res.verified == 1, h.last_error()
    got = h.proof_bytes(res)
    assert len(got) == res.proof_len == len(want["proof_bytes"]) and res.prefix_len == want["prefix_len"]
    assert got == want["proof_bytes"]
    assert MP.verify(want, cfg)[0]
    h.close()


@pytest.mark.parametrize("log_n,log_mem,lo,W", [(10, 10, 64, 130), (16, 14, 8192 - 2500, 5000)])
def test_windowed_and_dense_output_checks_verify_with_equal_digests(cozk, log_n, log_mem, lo, W):
    digests = []
    for windowed in (True, False):
        h = cozk.MemoryProof(log_n=log_n, log_mem=log_mem, seed=71, io_start=lo, io_len=W, windowed=windowed)
        res = h.prove(verify=True)
        assert res.verified == 1, h.last_error()
        assert res.proof_len > res.prefix_len > 0 and res.wall_ms > 0 and res.t_witness_ms > 0 and res.t_commit_ms > 0 and res.t_leaves_ms > 0 and res.t_gp_ms > 0
        assert res.t_out_ms > 0 and res.t_ts_ms > 0 and res.t_open_ms > 0 and res.out_peak_bytes > 0
        digests.append(bytes(res.proof_digest))
        h.close()
    assert digests[0] == digests[1]


@pytest.mark.parametrize("log_n", [6, 14])
@pytest.mark.parametrize("tamper,reason", [(1, P.REASON_MULTISET), (2, P.REASON_LEAF), (3, "timestamp: multiset equality"), (4, MP.REASON_OUT_FINAL)])
def test_tampered_proofs_are_rejected_with_their_reason(cozk, log_n, tamper, reason):
    h = cozk.MemoryProof(log_n=log_n, log_mem=8, seed=81, tamper=tamper, io_start=61, io_len=70)
    res = h.prove(verify=True)
    assert res.verified == 0
    assert h.last_error().startswith("verification failed: " + reason), h.last_error()
    h.close()


def test_tamper_4_is_rejected_with_the_dense_output_check_too(cozk):
    h = cozk.MemoryProof(log_n=6, log_mem=8, seed=81, tamper=4, io_start=61, io_len=70, windowed=False)
    res = h.prove(verify=True)
    assert res.verified == 0 and h.last_error().startswith("verification failed: output check: final claim"), h.last_error()
    h.close()


@pytest.mark.parametrize("with_ts", [True, False])
def test_the_prefix_is_the_rw_proofs(cozk, with_ts):
    cfg = dict(log_n=8, log_mem=9, n_slots=4, seed=83, with_ts=with_ts)
    m = cozk.MemoryProof(io_start=250, io_len=33, **cfg)
    mr = m.prove(verify=True)
    r = cozk.RwProof(**cfg)
    rr = r.prove(verify=True)
    assert mr.verified == 1 and rr.verified == 1, (m.last_error(), r.last_error())
    mb, rb = m.proof_bytes(mr), r.proof_bytes(rr)
    n = int(mr.prefix_len)
    assert 0 < n < len(rb) and mb[:n] == rb[:n] and mb[n:n + 8] == (9).to_bytes(8, "little")  # the output sumcheck: log_mem rounds
    m.close()
    r.close()


def test_two_proves_of_one_handle_give_equal_bytes(cozk):
    h = cozk.MemoryProof(log_n=8, log_mem=9, seed=91, io_start=100, io_len=21)
    a = h.prove(verify=True)
    b = h.prove(verify=False)
    assert a.verified == 1 and b.verified == -1
    assert h.proof_bytes(b) and bytes(a.proof_digest) == bytes(b.proof_digest) and a.proof_len == b.proof_len and a.prefix_len == b.prefix_len
    h.close()


@pytest.mark.parametrize("kw,text", [(dict(mode="rep3"), "mode is COZK_MODE_PLAIN"), (dict(log_n=0), "log_n in 1..22"), (dict(log_mem=25), "log_mem in 5..24"),
                                     (dict(n_slots=5), "n_slots in 1..4"), (dict(tamper=5), "tamper in 0..4"), (dict(tamper=3, with_ts=False), "3 only with with_ts"),
                                     (dict(io_len=0), "io_len is at least 1 word"), (dict(io_start=60, io_len=5), "io_start + io_len > MEM"),
                                     (dict(windowed=2), "windowed is 0 or 1")])
def test_bad_configs_are_refused(cozk, kw, text):
    with pytest.raises(cozk.CozkError) as e:
        cozk.MemoryProof(**dict(dict(log_n=4, log_mem=6, io_start=3, io_len=5), **kw))
    assert e.value.code == INVALID_ARG and text in str(e.value), str(e.value)
