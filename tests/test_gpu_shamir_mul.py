"""GPU tests of the Shamir multiplication with degree reduction (cozk_shamir_mul_deal / _inproc / _vec, cozk_ring_all_to_all)
against the big-int restatement tests/shamir_mul_ref.py.  Bar: bit-exact; calls go through the C ABI (ctypes).
No test provokes a device fault: every bad argument is rejected on the host before any launch."""
import ctypes
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch  # noqa: F401 - a torch host maps its own librccl first; libcozk then reuses that copy (one RCCL per process)

import pyref as O
import shamir_mul_ref as M
import shamir_ref as S
from test_gpu_shamir import EDGE, EDGE_MONT

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
R = O.R
NMAX = 1000


def _secrets(seed, n):
    e = [0, 1, R - 1, R - 2] + EDGE_MONT
    return (O.synthetic_fr(seed, max(n - len(e), 1)) + e)[:n]


def _ints(vecs):
    return [v.to_ints() for v in vecs]


@functools.lru_cache(maxsize=None)
def _coefs(degree, counter):
    """the dealer's PRF coefficient vectors at the longest length, computed once: a shorter deal uses their prefixes"""
    return S.prf_coeffs(S.keys_for(40 + degree, degree), degree, counter, NMAX)


# ------------------------------------------------------------------------------------------------ (a) deal parity
@pytest.mark.parametrize("counter", [0, (1 << 33) + 7])
@pytest.mark.parametrize("n", [0, 1, 257, 1000])
@pytest.mark.parametrize("parties,degree", [(3, 1), (5, 2), (8, 2), (15, 7), (17, 8), (32, 15)])
def test_mul_deal_matches_share_of_the_product(cozk, ctx, parties, degree, n, counter):
    a, b = _secrets(300 + parties, n), list(reversed(_secrets(400 + degree, n)))
    keys = S.keys_for(40 + degree, degree)
    got = cozk.Vec.from_ints(ctx, a).shamir_mul_deal(cozk.Vec.from_ints(ctx, b), keys, degree, parties, counter=counter)
    assert len(got) == parties and all(len(g) == n for g in got)
    prod = [x * y % R for x, y in zip(a, b)]
    want = S.eval_vec([prod] + [c[:n] for c in _coefs(degree, counter)], parties)  # = S.share_vec(prod, keys, ...)
    assert _ints(got) == want  # every party's vector
    if n == 257 and counter == 0:
        assert want == S.share_vec(prod, keys, degree, parties, counter=counter)


# ------------------------------------------------------------------------------------------------ (b) edge operands
@pytest.mark.parametrize("degree", [1, 7, 8, 15])
def test_mul_deal_edge_operands_through_the_product(cozk, ctx, degree):
    """all pairs of the edge operands of test_gpu_shamir.py (EDGE + EDGE_MONT: 12 values, 144 pairs) through the Montgomery product
    in front of the Horner chains, at 32 parties, through the templated (1, 7) and the rolled (8, 15) variant"""
    edge = EDGE + EDGE_MONT
    a = [x for x in edge for _ in edge]
    b = [y for _ in edge for y in edge]
    assert len(a) == len(edge) ** 2 == 144  # every operand against every operand
    keys = S.keys_for(40 + degree, degree)
    got = cozk.Vec.from_ints(ctx, a).shamir_mul_deal(cozk.Vec.from_ints(ctx, b), keys, degree, 32, counter=0)
    prod = [x * y % R for x, y in zip(a, b)]
    want = S.eval_vec([prod] + [c[:len(a)] for c in _coefs(degree, 0)], 32)
    for p in range(32):
        assert got[p].to_ints() == want[p], "party %d" % p
    raw = np.concatenate([g.to_numpy() for g in got])  # canonical limbs: below r as 256-bit integers
    top = raw[:, 3]
    assert (top <= np.uint64(R >> 192)).all()
    for row in raw[top == np.uint64(R >> 192)]:
        assert O.from_limbs64(row) < R


# ------------------------------------------------------------------------------------------------ (c) fused vs composed
def test_mul_deal_equals_binop_then_share(cozk, ctx):
    parties, degree, n = 8, 2, 1000
    A, B = cozk.Vec.random(ctx, n, seed=51), cozk.Vec.random(ctx, n, seed=52)
    keys = S.keys_for(53, degree)
    fused = A.shamir_mul_deal(B, keys, degree, parties, counter=9)
    composed = A.binop(cozk.OP_MUL, B).shamir_share(keys, degree, parties, counter=9)
    for f, c in zip(fused, composed):
        assert np.array_equal(f.to_numpy(), c.to_numpy())  # raw Montgomery limbs: canonical outputs are unique


# ------------------------------------------------------------------------------------------------ (d) in-process
@pytest.fixture(scope="module")
def party_ctxs(cozk):
    cs = [cozk.Context(0) for _ in range(8)]
    yield cs
    for c in cs:
        c.close()


def _high_end(parties, k):
    return list(range(parties, parties - k, -1))


@pytest.mark.parametrize("n", [1, 257])
@pytest.mark.parametrize("parties,degree", [(3, 1), (5, 2), (8, 2), (7, 3)])
def test_mul_inproc(cozk, ctx, party_ctxs, parties, degree, n):
    pcs = party_ctxs[:parties]
    a, b, c = _secrets(61, n), list(reversed(_secrets(62, n))), _secrets(63, n)
    deal = lambda v, seed, ctr: cozk.Vec.from_ints(ctx, v).shamir_scatter(S.keys_for(seed, degree), degree, pcs, counter=ctr)
    sa, sb, sc = deal(a, 71, 0), deal(b, 72, n), deal(c, 73, 2 * n)
    keys = M.party_keys(7, parties, degree)
    got = cozk.shamir_mul(pcs, sa, sb, keys, degree, counter=3 * n)
    got_ints = _ints(got)  # (the downloads also drain every party's stream before another context reads the vectors below)
    for q in range(parties):
        assert got[q].ctx is pcs[q] and len(got[q]) == n
    assert got_ints == M.mul(_ints(sa), _ints(sb), keys, degree, counter=3 * n)  # every party's output
    ab = [x * y % R for x, y in zip(a, b)]
    pts = _high_end(parties, degree + 1)
    assert cozk.shamir_combine([got[p - 1] for p in pts], pts, degree).to_ints() == ab
    # negative control: t parties' worth of degree does not open it
    low = cozk.shamir_combine([got[p - 1] for p in pts], pts, degree - 1).to_ints()
    assert sum(x != y for x, y in zip(low, ab)) >= (n + 1) // 2
    # the product is a degree-t sharing: it multiplies again
    again = cozk.shamir_mul(pcs, got, sc, keys, degree, counter=4 * n)
    again_ints = _ints(again)
    assert again_ints == M.mul(got_ints, _ints(sc), keys, degree, counter=4 * n)
    assert cozk.shamir_combine([again[p - 1] for p in pts], pts, degree).to_ints() == [x * y % R for x, y in zip(ab, c)]
    # parties above 2t deal nothing: garbage or no vectors and keys there change no output
    k = M.dealers(degree)
    if parties > k:
        junk = [cozk.Vec.random(pcs[p], n + 3, seed=p) for p in range(k, parties)]
        for rest_a, rest_b in ((junk, junk), ([None] * (parties - k), [None] * (parties - k))):
            same = cozk.shamir_mul(pcs, sa[:k] + rest_a, sb[:k] + rest_b, keys[:k] + [None] * (parties - k), degree, counter=3 * n)
            assert _ints(same) == got_ints


def test_mul_inproc_empty(cozk, ctx, party_ctxs):
    pcs = party_ctxs[:5]
    empty = [cozk.Vec.alloc(c, 0) for c in pcs]
    got = cozk.shamir_mul(pcs, empty, empty, M.party_keys(1, 5, 2), 2)
    assert [len(g) for g in got] == [0] * 5 and all(g.to_ints() == [] for g in got)
    assert [len(g) for g in empty[0].shamir_mul_deal(empty[0], S.keys_for(1, 2), 2, 5)] == [0] * 5


# ------------------------------------------------------------------------------------------------ (e) refusals
def _expect_invalid(cozk, ctx, rc, text):
    assert rc == -1  # COZK_ERR_INVALID_ARG
    msg = cozk._lib.lib().cozk_last_error(ctx.h).decode()
    assert text in msg, msg


def test_refusals_leave_no_handle(cozk, ctx, party_ctxs):
    l = cozk._lib.lib()
    V = cozk.Vec.from_ints(ctx, [1, 2, 3])
    W = cozk.Vec.from_ints(ctx, [1, 2])
    U = cozk.Vec.from_ints(ctx, [1, 2, 3], kind=cozk.SCALAR_U32)
    keys = b"".join(S.keys_for(1, 15))
    SENT = 0x5A5A

    def outs():
        return (ctypes.c_void_p * 40)(*([SENT] * 40))

    def cleared(o, k):
        return all(o[i] is None for i in range(k)) and all(o[i] == SENT for i in range(k, 40))

    def deal(a, b, ks, deg, parties, text, k=None):
        o = outs()
        _expect_invalid(cozk, ctx, l.cozk_shamir_mul_deal(ctx.h, a.h if a else None, b.h if b else None, ks, deg, parties, 0, o), "shamir_mul_deal: " + text)
        assert cleared(o, parties if k is None else k)

    deal(V, V, keys, 6, 10, "2 * degree + 1 <= num_parties")  # the reference's test_shamir_10_6 shape shares but cannot multiply
    deal(V, V, keys, 1, 2, "2 * degree + 1 <= num_parties")
    deal(V, W, keys, 1, 3, "the factors must have one length")
    deal(V, U, keys, 1, 3, "the factors must be FR vectors")
    deal(U, V, keys, 1, 3, "the factors must be FR vectors")
    deal(V, V, None, 1, 3, "null argument")  # no key block
    deal(V, None, keys, 1, 3, "null argument")
    deal(V, V, keys, 0, 3, "1 <= degree <= COZK_SHAMIR_MAX_DEGREE")
    deal(V, V, keys, 16, 32, "1 <= degree <= COZK_SHAMIR_MAX_DEGREE")
    deal(V, V, keys, 1, 33, "degree < num_parties <= COZK_SHAMIR_MAX_PARTIES", k=0)  # out[] untouched: its length is unknown
    _expect_invalid(cozk, ctx, l.cozk_shamir_mul_deal(ctx.h, V.h, V.h, keys, 1, 3, 0, None), "null output")
    for bad, deg, parties in ((W, 1, 3), (U, 1, 3), (V, 6, 10)):
        with pytest.raises(cozk.CozkError) as e:
            V.shamir_mul_deal(bad, S.keys_for(1, deg), deg, parties)
        assert e.value.code == -1

    # in process: the same rules for every dealer; the text is left with party 0
    p0 = party_ctxs[0]
    mk = lambda c, vals, kind=cozk.SCALAR_FR: cozk.Vec.from_ints(c, vals, kind=kind)
    arr = lambda hs: (ctypes.c_void_p * 40)(*(list(hs) + [None] * (40 - len(hs))))
    kb = ctypes.create_string_buffer(keys, len(keys))

    def inproc(parties, deg, a, b, key_ptrs, text, ctxs=None, k=None):
        o = outs()
        cs = arr([c.h.value for c in party_ctxs[:parties]] + [party_ctxs[0].h.value] * max(parties - 8, 0)) if ctxs is None else ctxs
        rc = l.cozk_shamir_mul_inproc(cs, arr([v.h.value if v else None for v in a]), arr([v.h.value if v else None for v in b]), arr(key_ptrs), deg, parties, 0, o)
        _expect_invalid(cozk, p0, rc, "shamir_mul_inproc: " + text)
        assert cleared(o, parties if k is None else k)

    good = [mk(c, [1, 2, 3]) for c in party_ctxs[:3]]
    kp = [ctypes.addressof(kb)] * 3
    inproc(3, 1, good, [good[0], mk(party_ctxs[1], [1, 2]), good[2]], kp, "the factors must have one length")
    inproc(3, 1, good, [good[0], good[1], mk(party_ctxs[2], [1, 2, 3], cozk.SCALAR_U32)], kp, "the factors must be FR vectors")
    inproc(3, 1, [good[0], mk(party_ctxs[1], [1, 2]), good[2]], [good[0], mk(party_ctxs[1], [1, 2]), good[2]], kp, "the factors must have one length")
    inproc(3, 1, good, good, [kp[0], None, kp[2]], "parties 0..2 * degree need their key block")
    inproc(3, 1, good, [good[0], None, good[2]], kp, "parties 0..2 * degree need both factors")
    inproc(3, 1, good, [good[0], good[0], good[2]], kp, "party p's factors must be vectors of party_ctxs[p]")
    inproc(3, 1, good, good, kp, "null party context", ctxs=arr([party_ctxs[0].h.value, None, party_ctxs[2].h.value]))
    inproc(10, 6, good * 4, good * 4, kp * 4, "2 * degree + 1 <= num_parties")
    inproc(33, 1, good, good, kp, "degree < num_parties <= COZK_SHAMIR_MAX_PARTIES", k=0)
    for kw in (dict(b=[good[0], mk(party_ctxs[1], [1, 2]), good[2]]), dict(keys=[S.keys_for(1, 1), None, S.keys_for(2, 1)])):
        with pytest.raises(cozk.CozkError) as e:
            cozk.shamir_mul(party_ctxs[:3], good, kw.get("b", good), kw.get("keys", M.party_keys(1, 3, 1)), 1)
        assert e.value.code == -1
    assert V.to_ints() == [1, 2, 3] and _ints(good) == [[1, 2, 3]] * 3  # nothing ran


# ------------------------------------------------------------------------------------------------ (f) all-to-all, one rank
def test_all_to_all_single_rank_self_loop(cozk):
    c = cozk.Context(0)
    try:
        c.ring_init(cozk.Context.ring_unique_id(), 0, 1)
        vals = O.synthetic_fr(77, 1000)
        (got,) = c.all_to_all([cozk.Vec.from_ints(c, vals)])
        assert got.to_ints() == vals  # the only peer is the rank itself, through ncclSend / ncclRecv
        big = cozk.Vec.random(c, 1 << 21, seed=13)
        (back,) = c.all_to_all([big])
        assert back.binop(cozk.OP_SUB, big).to_numpy().any() == False  # noqa: E712 - numpy bool
        assert c.ring_info() == (0, 1, (1000 + (1 << 21)) * 32)
        (e,) = c.all_to_all([cozk.Vec.alloc(c, 0)])
        assert len(e) == 0
        assert c.all_to_all([None]) == [None]
        assert c.ring_info()[2] == (1000 + (1 << 21)) * 32
        with pytest.raises(cozk.CozkError) as err:  # one length on the own rank, and FR entries
            c.all_to_all([big], recv_lens=[5])
        assert err.value.code == -1 and "own rank" in str(err.value)
        with pytest.raises(cozk.CozkError) as err:
            c.all_to_all([cozk.Vec.from_ints(c, [1, 2], kind=cozk.SCALAR_U32)])
        assert err.value.code == -1 and "FR vectors" in str(err.value)
        # one party cannot multiply: 2t + 1 = 3 > 1 rank
        with pytest.raises(cozk.CozkError) as err:
            c.shamir_mul_vec(big, big, S.keys_for(1, 1), 1)
        assert err.value.code == -1 and "shamir_mul_vec" in str(err.value) and "num_parties" in str(err.value)
        c.ring_destroy()
        with pytest.raises(cozk.CozkError) as err:
            c.all_to_all([big])  # no ring any more
        assert "cozk_ring_init has not been called" in str(err.value)
        with pytest.raises(cozk.CozkError) as err:
            c.shamir_mul_vec(big, big, S.keys_for(1, 1), 1)
        assert "cozk_ring_init has not been called" in str(err.value)
    finally:
        c.close()


# ------------------------------------------------------------------------------------------------ (g) one party per process
def test_mul_vec_three_processes_one_gpu_each(cozk, tmp_path):
    if torch.cuda.device_count() < 3:
        pytest.skip("needs 3 GPUs: RCCL refuses two ranks of one communicator on the same device")
    parties, degree, n = 3, 1, 257
    a, b = _secrets(81, n), list(reversed(_secrets(82, n)))
    sa = S.share_vec(a, S.keys_for(83, degree), degree, parties)
    sb = S.share_vec(b, S.keys_for(84, degree), degree, parties, counter=n)
    keys = M.party_keys(9, parties, degree)
    script = os.path.join(ROOT, "tools", "shamir_mul_party.py")
    procs = []
    try:
        ring_id = None
        for rank in range(parties):  # three FRESH interpreters; rank 0 draws the ring id and prints it before it joins
            job = tmp_path / ("party%d.json" % rank)
            job.write_text(json.dumps({"a": [hex(x) for x in sa[rank]], "b": [hex(x) for x in sb[rank]], "keys": [k.hex() for k in keys[rank]],
                                       "degree": degree, "counter": 2 * n, "out": str(tmp_path / ("out%d.json" % rank))}))
            cmd = [sys.executable, script, "--rank", str(rank), "--ranks", str(parties), "--job", str(job)]
            if rank:
                cmd += ["--ring-id", ring_id]
            p = subprocess.Popen(cmd, cwd=ROOT, stdout=subprocess.PIPE, stderr=open(tmp_path / ("err%d.txt" % rank), "w"), text=True)
            procs.append(p)
            if rank == 0:
                for line in p.stdout:  # ends with the pipe if the child dies first
                    if line.startswith("ring-id "):
                        ring_id = line.split()[1]
                        break
                assert ring_id and len(ring_id) == 256, (tmp_path / "err0.txt").read_text()[-2000:]
        for rank, p in enumerate(procs):
            out, _ = p.communicate(timeout=300)
            assert p.returncode == 0, out[-2000:] + (tmp_path / ("err%d.txt" % rank)).read_text()[-2000:]
    finally:
        for p in procs:
            if p.poll() is None:
                p.kill()
    got = [[int(x, 16) for x in json.loads((tmp_path / ("out%d.json" % r)).read_text())] for r in range(parties)]
    assert got == M.mul(sa, sb, keys, degree, counter=2 * n)
    assert S.combine_vec(got[1:], [2, 3], degree) == [x * y % R for x, y in zip(a, b)]


# ------------------------------------------------------------------------------------------------ (h) two devices
def test_mul_inproc_peer_copy_two_gpus(cozk, ctx):
    """the hipMemcpyPeer leg of cozk_shamir_mul_inproc: odd parties on GPU 1, dealers on both devices"""
    if torch.cuda.device_count() < 2:
        pytest.skip("needs 2 GPUs")
    parties, degree, n = 5, 2, 257
    other = [cozk.Context(1) for _ in range(2)]
    mine = [cozk.Context(0) for _ in range(3)]
    pcs = [other[p // 2] if p % 2 else mine[p // 2] for p in range(parties)]
    a, b = _secrets(91, n), list(reversed(_secrets(92, n)))
    sa = cozk.Vec.from_ints(ctx, a).shamir_scatter(S.keys_for(93, degree), degree, pcs)
    sb = cozk.Vec.from_ints(ctx, b).shamir_scatter(S.keys_for(94, degree), degree, pcs, counter=n)
    keys = M.party_keys(11, parties, degree)
    got = cozk.shamir_mul(pcs, sa, sb, keys, degree, counter=2 * n)
    assert _ints(got) == M.mul(_ints(sa), _ints(sb), keys, degree, counter=2 * n)
    for q in range(parties):
        assert got[q].ctx is pcs[q]
    for v in got + sa + sb:
        v.free()
    for c in other + mine:
        c.close()
