"""GPU tests of the read-write memory proof by three Rep3 parties (cozk_rw_proof_rep3_*, csrc/host/rw_memory_proof_rep3.hpp): the proof
is byte for byte the plain proof of the same instance.  Against the plain-Python restatement tests/rw_proof_ref.py with with_ts = 0 at
(log_n, log_mem, n_slots) = (1, 5, 4), (3, 5, 4), (6, 5, 4), (3, 7, 3) -- memory longer than the trace, a batch of 6 padded to 8 -- and
(6, 5, 1) -- no slot writes; against the plain harness RwProof(with_ts=False) of the same seed with either leaves path at (9, 5, 4) --
a read / write layer above 2048 elements -- (10, 10, 4) and (5, 12, 4); tampers 1 and 2 rejected with their reasons at log_n = 6 and
10; two proves of one handle; ring traffic and positive phase times; the refusals of bad configs."""
import pytest

import rw_proof_ref as P

pytestmark = pytest.mark.gpu
INVALID_ARG = -1


@pytest.mark.parametrize("log_n,log_mem,ns", [(1, 5, 4), (3, 5, 4), (6, 5, 4), (3, 7, 3), (6, 5, 1)])
def test_proof_bytes_equal_the_python_restatement(cozk, log_n, log_mem, ns):
    cfg = dict(log_n=log_n, log_mem=log_mem, n_slots=ns, seed=61 + log_n)
    want = P.prove(dict(cfg, with_ts=0))
    h = cozk.RwProofRep3(**cfg)
    res = h.prove(verify=True)
    assert res.verified == 1, h.last_error()
    got = h.proof_bytes(res)
    assert len(got) == res.proof_len == len(want["proof_bytes"])
    assert got == want["proof_bytes"]
    h.close()


@pytest.mark.parametrize("log_n,log_mem", [(9, 5), (10, 10), (5, 12)])
def test_bytes_and_digest_equal_the_plain_harness_with_either_leaves_path(cozk, log_n, log_mem):
    p = cozk.RwProof(log_n=log_n, log_mem=log_mem, n_slots=4, seed=71, with_ts=False, mode="plain")
    pres = p.prove(verify=True)
    assert pres.verified == 1, p.last_error()
    want, digest = p.proof_bytes(pres), bytes(pres.proof_digest)
    p.close()
    for fused in (False, True):
        h = cozk.RwProofRep3(log_n=log_n, log_mem=log_mem, n_slots=4, seed=71, leaves_fused=fused)
        res = h.prove(verify=True)
        assert res.verified == 1, h.last_error()
        assert h.proof_bytes(res) == want and bytes(res.proof_digest) == digest
        assert res.ring_bytes > 0
        for t in (res.wall_ms, res.t_witness_ms, res.t_share_ms, res.t_commit_ms, res.t_leaves_ms, res.t_gp_ms, res.t_open_ms):
            assert t > 0
        h.close()


@pytest.mark.parametrize("log_n", [6, 10])
@pytest.mark.parametrize("tamper,reason", [(1, P.REASON_MULTISET), (2, P.REASON_LEAF)])
def test_tampered_proofs_are_rejected_with_their_reason(cozk, log_n, tamper, reason):
    h = cozk.RwProofRep3(log_n=log_n, log_mem=8, seed=81, tamper=tamper)
    res = h.prove(verify=True)
    assert res.verified == 0
    assert h.last_error().startswith("verification failed: " + reason), h.last_error()
    h.close()


def test_two_proves_of_one_handle_give_equal_bytes(cozk):
    h = cozk.RwProofRep3(log_n=8, log_mem=9, seed=91)
    a = h.prove(verify=True)
    b = h.prove(verify=False)
    assert a.verified == 1 and b.verified == -1
    assert h.proof_bytes(b) and bytes(a.proof_digest) == bytes(b.proof_digest) and a.proof_len == b.proof_len
    h.close()


@pytest.mark.parametrize("kw,text", [(dict(log_n=0), "log_n in 1..22"), (dict(log_n=23), "log_n in 1..22"), (dict(n_slots=0), "n_slots in 1..4"),
                                     (dict(n_slots=5), "n_slots in 1..4"), (dict(log_mem=4), "log_mem in 5..24"), (dict(log_mem=25), "log_mem in 5..24"),
                                     (dict(leaves_fused=2), "leaves_fused are 0 or 1"), (dict(tamper=3), "tamper in 0..2")])
def test_bad_configs_are_refused(cozk, kw, text):
    with pytest.raises(cozk.CozkError) as e:
        cozk.RwProofRep3(**dict(dict(log_n=4, log_mem=6), **kw))
    assert e.value.code == INVALID_ARG and "rw_proof_rep3: " in str(e.value) and text in str(e.value), str(e.value)
