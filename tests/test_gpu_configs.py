"""Every BASELINE.json configuration, at its own shape and size, through the C ABI on the one GPU of the box
(SURVEY 8d's synthetic restatements; `tools/run_config.py` runs the same shapes for timing):
  * configs[0] -- 2^14-cycle trace, 3-party Rep3, 64 Fr + 32 u16 + 16 u32 + 16 flag polynomials, 8 circuits;
  * configs[2] -- 2^22-cycle trace, 3-party Rep3, 137 shared polynomials per party, the three parties time-sliced on the
    one GPU (~215 GiB of HBM): the verifier accepts and every party moved exactly the ring traffic the construct phase
    implies (sum over the 22 multiplication layers of 8 * 2^22 / 2^l field elements);
  * configs[3] -- co-noir-spartan, 2^18 constraints, 3-party Rep3 == the plain proof bit for bit;
  * configs[1] (2^20, plain) is tests/test_gpu_fullsize.py::test_bench_workload_verifies_and_is_deterministic;
  * configs[4] (8-party Shamir) has no reference prover: its substitute, the 8-worker split of one proof,
    is exercised at 2^17 here (2^23 by tools/run_config.py --config 5).
The oracle cannot finish these sizes in seconds, so the checks are the domain's own: the built-in verifier (every
sumcheck round, final GKR claim == direct leaf evaluation, opening reduction, PST13 opening against the trapdoor) and
Rep3 proof == plain proof (shares and masks cancel in the coordinator's sums)."""
import pytest

pytestmark = pytest.mark.gpu


def _digest(res):
    return bytes(res.proof_digest).hex()


def test_config0_2p14_rep3_equals_plain(cozk):
    cfg = dict(log_n=14, n_fr=64, n_u16=32, n_u32=16, n_flags=16, n_small=0, gp_batch=8, gp_log_leaves=15, seed=2026)
    digs = {}
    for mode in ("plain", "rep3"):
        h = cozk.Harness(mode=mode, **cfg)
        r = h.prove(verify=True)
        assert r.verified == 1, h.last_error()
        if mode == "rep3":
            assert r.bytes_ring > 0 and r.star_messages > 0
        digs[mode] = _digest(r)
        h.close()
    assert digs["plain"] == digs["rep3"]


def test_config2_2p22_rep3_137_polys_time_sliced(cozk):
    h = cozk.Harness(mode="rep3", log_n=22, n_fr=137, n_u16=0, n_u32=0, n_flags=0, n_small=0, gp_batch=8, gp_log_leaves=23, seed=2026)
    try:
        r = h.prove(verify=True)
        assert r.verified == 1, h.last_error()
        # construct: layer l+1 = mul_vec(L, R) of layer l, l = 0..21: 8 * 2^23 / 2^(l+1) elements of 32 B to the next
        # party, for each of the three parties (bytes_ring is the sum over the in-process parties)
        assert r.bytes_ring == 3 * sum(8 * (1 << 23) // (1 << (l + 1)) * 32 for l in range(22)) == 6442449408
        assert r.proof_len > 0
    finally:
        h.close()


def test_config3_spartan_2p18_rep3_equals_plain(cozk):
    digs = {}
    for mode in ("plain", "rep3"):
        h = cozk.SpartanHarness(mode=mode, log_n=18, seed=2026)
        r = h.prove(verify=True)
        assert r.verified == 1, h.last_error()
        digs[mode] = _digest(r)
        h.close()
    assert digs["plain"] == digs["rep3"]


@pytest.mark.parametrize("log_n", [17, 21])
def test_config4_substitute_8_worker_split(cozk, log_n):
    """one proof of a 2^17- / 2^21-cycle trace as 8 worker sub-nets time-sliced on the one GPU (the substitute for the Shamir
    configuration, whose 2^24 trace is 2^21 cycles per GPU on the 8-GPU node): verifies, and its commitments + GKR part are the
    single-worker proof's (tests/test_gpu_split.py checks the byte prefix)"""
    h = cozk.Harness(mode="plain", log_n=log_n, n_fr=8, n_u16=4, n_u32=2, n_flags=2, n_small=0, gp_batch=8, gp_log_leaves=log_n + 1, seed=2026,
                     log_workers=3)
    r = h.prove(verify=True)
    assert r.verified == 1, h.last_error()
    assert bytes(h.prove(verify=False).proof_digest) == bytes(r.proof_digest)
    h.close()


def test_bench_four_ranks_share_the_gpu(tmp_path):
    """`bench.py --gpus 4 --log-n 14` starts its own four ranks (4 processes on the card: within the box's guard of 6; the 8-rank
    run is the driver's, on an 8-GPU node -- tests/test_dist_cpu.py rehearses its launch and hub on the CPU): ONE proof of a
    2^16-cycle trace as 4 worker sub-nets, one JSON line, every rank assembled the same proof, per-rank phases and hub waits;
    `--dump-outputs` writes rank 0's copy of that proof, whose SHA-256 is the line's proof_sha256"""
    import hashlib
    import json
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_PORT")}
    p = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "4", "--log-n", "14", "--steps", "2", "--warmup", "1",
                        "--dump-outputs", str(tmp_path)], env=env,
                       capture_output=True, timeout=600)
    assert p.returncode == 0, p.stderr.decode()[-3000:]
    lines = [ln for ln in p.stdout.decode().splitlines() if ln.startswith("{")]
    assert len(lines) == 1
    out = json.loads(lines[0])
    assert out["n_gpus"] == 4 and out["scaling"] == "weak" and len(set(out["proof_sha256"])) == 1 and len(out["proof_sha256"]) == 4
    assert [r["rank"] for r in out["per_rank"]] == [0, 1, 2, 3]
    assert all(r["hub_exchanges_per_step"] > 0 and r["hub_wait_ms_per_step"] >= 0 for r in out["per_rank"])
    import numpy as np
    proof = np.load(tmp_path / "proof.npy")
    assert proof.dtype == np.float32 and proof.size == out["proof_bytes"]
    assert hashlib.sha256(proof.astype(np.uint8).tobytes()).hexdigest()[:16] == out["proof_sha256"][0]


def test_bench_plain_run_dumps_the_last_proof(tmp_path):
    """a plain `bench.py --gpus 1` run prints the headline line without the `--full` legs, and `--dump-outputs` writes the
    last timed step's proof (one float32 per byte) whose SHA-256 is the line's proof_sha256"""
    import hashlib
    import json
    import os
    import subprocess
    import sys
    import numpy as np
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_PORT")}
    p = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "1", "--log-n", "14", "--steps", "2", "--warmup", "1",
                        "--dump-outputs", str(tmp_path)], env=env, capture_output=True, timeout=600)
    assert p.returncode == 0, p.stderr.decode()[-3000:]
    lines = [ln for ln in p.stdout.decode().splitlines() if ln.startswith("{")]
    assert len(lines) == 1
    out = json.loads(lines[0])
    assert all(k in out for k in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"))
    assert out["steps"] == 2 and out["ms_per_step"] > 0
    assert not any(k in out for k in ("roofline", "cpu_baseline", "full_step"))
    proof = np.load(tmp_path / "proof.npy")
    assert proof.dtype == np.float32 and proof.size == out["proof_bytes"]
    assert hashlib.sha256(proof.astype(np.uint8).tobytes()).hexdigest()[:16] == out["proof_sha256"][0]


def test_bench_steps_sets_the_number_of_timed_steps():
    """`--steps N` times N proofs: the MSM gather launches counted by the `--full` HIP events inside the timed region of a
    3-step run are exactly three times those of a 1-step run (the count per proof is fixed), and the warm-up is not counted"""
    import json
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_PORT")}
    launches = {}
    for steps in (1, 3):
        p = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "1", "--log-n", "14", "--steps", str(steps), "--warmup", "2",
                            "--full", "--no-full-step", "--no-cpu-baseline"], env=env, capture_output=True, timeout=600)
        assert p.returncode == 0, p.stderr.decode()[-3000:]
        lines = [ln for ln in p.stdout.decode().splitlines() if ln.startswith("{")]
        assert len(lines) == 1
        out = json.loads(lines[0])
        assert out["steps"] == steps
        launches[steps] = out["roofline"]["launches"]
    assert launches[1] > 0 and launches[3] == 3 * launches[1]
