"""GPU tests of the read-write memory proof (cozk_rw_proof_*, csrc/host/rw_memory_proof.hpp): proof bytes equal to the plain-Python
restatement tests/rw_proof_ref.py byte for byte at (log_n, log_mem, n_slots, with_ts) = (1, 5, 4, 1), (3, 5, 4, 1), (6, 5, 4, 1),
(3, 7, 3, 0), (6, 5, 1, 1) -- one workgroup; the resident tail; a layer above 2048 elements; log_mem > log_n with a batch of 6 padded to
8; a trace with no write -- verified proofs at (10, 10) and (16, 14) with either leaves path and equal digests, tampers 1, 2 and 3
rejected with their reasons at log_n = 6 and 16, two proves of one handle, and the refusals of bad configs."""
import pytest

import rw_proof_ref as P

pytestmark = pytest.mark.gpu
INVALID_ARG = -1


@pytest.mark.parametrize("log_n,log_mem,ns,with_ts", [(1, 5, 4, 1), (3, 5, 4, 1), (6, 5, 4, 1), (3, 7, 3, 0), (6, 5, 1, 1)])
def test_proof_bytes_equal_the_python_restatement(cozk, log_n, log_mem, ns, with_ts):
    cfg = dict(log_n=log_n, log_mem=log_mem, n_slots=ns, with_ts=with_ts, seed=61 + log_n)
    want = P.prove(cfg)
    h = cozk.RwProof(**cfg)
    res = h.prove(verify=True)
    assert res.verified == 1, h.last_error()
    got = h.proof_bytes(res)
    assert len(got) == res.proof_len == len(want["proof_bytes"])
    assert got == want["proof_bytes"]
    assert P.verify(want, cfg)[0]
    h.close()


@pytest.mark.parametrize("log_n,log_mem", [(10, 10), (16, 14)])
def test_verified_with_either_leaves_path_and_equal_digests(cozk, log_n, log_mem):
    digests = []
    for fused in (True, False):
        h = cozk.RwProof(log_n=log_n, log_mem=log_mem, seed=71, leaves_fused=fused)
        res = h.prove(verify=True)
        assert res.verified == 1, h.last_error()
        assert res.proof_len > 0 and res.wall_ms > 0 and res.t_witness_ms > 0 and res.t_commit_ms > 0 and res.t_leaves_ms > 0 and res.t_gp_ms > 0
        assert res.t_ts_ms > 0 and res.t_open_ms > 0
        digests.append(bytes(res.proof_digest))
        h.close()
    assert digests[0] == digests[1]


@pytest.mark.parametrize("log_n", [6, 16])
@pytest.mark.parametrize("tamper,reason", [(1, P.REASON_MULTISET), (2, P.REASON_LEAF), (3, "timestamp: multiset equality")])
def test_tampered_proofs_are_rejected_with_their_reason(cozk, log_n, tamper, reason):
    h = cozk.RwProof(log_n=log_n, log_mem=8, seed=81, tamper=tamper)
    res = h.prove(verify=True)
    assert res.verified == 0
    assert h.last_error().startswith("verification failed: " + reason), h.last_error()
    h.close()


def test_two_proves_of_one_handle_give_equal_bytes(cozk):
    h = cozk.RwProof(log_n=8, log_mem=9, seed=91)
    a = h.prove(verify=True)
    b = h.prove(verify=False)
    assert a.verified == 1 and b.verified == -1
    assert h.proof_bytes(b) and bytes(a.proof_digest) == bytes(b.proof_digest) and a.proof_len == b.proof_len
    h.close()


@pytest.mark.parametrize("kw,text", [(dict(mode="rep3"), "mode is COZK_MODE_PLAIN"), (dict(log_n=0), "log_n in 1..22"), (dict(log_n=23), "log_n in 1..22"),
                                     (dict(n_slots=0), "n_slots in 1..4"), (dict(n_slots=5), "n_slots in 1..4"), (dict(log_mem=4), "log_mem in 5..24"),
                                     (dict(log_mem=25), "log_mem in 5..24"), (dict(tamper=4), "tamper in 0..3"),
                                     (dict(tamper=3, with_ts=False), "3 only with with_ts")])
def test_bad_configs_are_refused(cozk, kw, text):
    with pytest.raises(cozk.CozkError) as e:
        cozk.RwProof(**dict(dict(log_n=4, log_mem=6), **kw))
    assert e.value.code == INVALID_ARG and text in str(e.value), str(e.value)
