"""GPU parity at production sizes: the HIP output against an oracle of the same operation, past the size thresholds where the
kernels switch to their multi-workgroup and throughput paths (the byte-exact checks elsewhere in the suite run at toy sizes).
  * whole proofs: byte for byte against the plain-C oracle (oracle/c/oracle.c) or the Python restatements live, and against
    the C oracle's committed digests at 2^18 / 2^20 (tests/golden/scale_pipelines.json, written by tests/golden/make_golden.py);
  * MSM: every point against the C Pippenger (coracle.msm) -- an exact check, which linearity is not: an error that is itself
    linear in the scalars (a dropped scalar, a shifted base, a lost slice) keeps MSM(a) + MSM(b) == MSM(a + b);
  * the reducing kernels past their grid caps against big-int sums.
Each docstring names the thresholds its sizes cross, with the dispatch line that decides them; the kernel names were checked against
a rocprofv3 kernel trace of one prove per pipeline shape."""
import ctypes
import functools
import hashlib
import importlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import coracle
import pyref as O

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SCALE_GOLD = json.load(open(os.path.join(HERE, "golden", "scale_pipelines.json")))
SCALE = SCALE_GOLD["pipelines"]

# the bench workload's column mix (bench.py, one GPU; 2^20 cycles there)
BENCH_MIX = dict(n_fr=64, n_u16=32, n_u32=16, n_flags=16, n_small=0, gp_batch=8, seed=2026)
RINV = pow(1 << 256, -1, O.R)
EDGE = [0, 1, 2, O.R - 1, O.R - 2, O.R_MONT_ONE, (1 << 253) + 12345, (1 << 253) - 1, O.TWO_INV, 65535, 65536, 1 << 16 * 15]


def _digest(res):
    return bytes(res.proof_digest).hex()


@functools.lru_cache(maxsize=None)
def _c_oracle_proof(key):
    """the C oracle's plain proof of a grand-product harness config (plain == rep3 in the oracle: tests/test_oracle.py)"""
    _, proof = coracle.pipeline(dict(key, mode="plain"))
    return proof


def _prove(h):
    res = h.prove(verify=True)
    assert res.verified == 1, h.last_error()
    got = h.proof_bytes(res)
    assert hashlib.sha256(got).hexdigest() == _digest(res)
    return res, got


# ---------------------------------------------------------------- (a) grand-product harness == the C oracle, live
GP_SHAPES = {
    # the bench mix; at 2^14 it is also config 0 of tests/test_gpu_configs.py
    "bench_2p12": dict(BENCH_MIX, log_n=12, gp_log_leaves=13),
    "bench_2p14": dict(BENCH_MIX, log_n=14, gp_log_leaves=15),
    "bench_2p16": dict(BENCH_MIX, log_n=16, gp_log_leaves=17),
    # small-value columns and a leaf count that is not log_n + 1
    "small_cols_2p14": dict(log_n=14, n_fr=6, n_u16=3, n_u32=2, n_flags=3, n_small=5, gp_batch=4, gp_log_leaves=14, seed=2024),
}


@pytest.mark.parametrize("mode", ["plain", "rep3"])
@pytest.mark.parametrize("shape", sorted(GP_SHAPES))
def test_grand_product_harness_equals_c_oracle(cozk, shape, mode):
    """commit -> dense grand product -> batch_evaluate -> reduce_and_prove -> PST open, byte for byte == orc_pipeline.
    Thresholds crossed (bench mix, n = 2^log_n, gp leaves 2^(log_n + 1) in 8 circuits):
      * MSM commit of 2^12..2^16 scalars per column: k_msm_hist_lds / k_msm_scatter_lds on ceil(n / 4096) > 1 workgroups
        (host/msm_schedule.hpp: msm_sort_wgs); 64 FR + 64 small-value columns = 128 polynomials, so two launch sets of 64 pipelined on the
        second stream (host/msm_schedule.hpp: MsmTailBlock::pipelined); fold levels k_msm_accumN once a bucket holds more than L0 = 8 references
        (host/msm_schedule.hpp: msm_set_counts);
      * GKR layers of len / 4 >= 1024 run the 9 x 29 kernels k_layer_cubic9 (LAYER_F9_MIN_CHUNKS); the plain prover's grouped
        split-eq variant k_layer_cubic9<1, 2> once E1_len / 2 >= 512 (layer_variant) -- reached by the 2^16 shape's
        first round (8 x 2^17 leaves; one dispatch in a kernel trace); tests/test_gpu_layer_grouped.py holds that variant and
        k_layer_bind_cubic9<1, 2> to the Python oracle at ragged lengths and pinned grids;
      * the resident round kernel below ROUND_PERSIST_MAX = 2048 elements (cozk_layer_prove_rounds);
      * batch_evaluate over 2^14 / 2^16-element columns: k_poly_eval_chi capped at 192 workgroups (EVAL_GRID_MAX), so
        lanes hold several elements above 49 152."""
    cfg = GP_SHAPES[shape]
    h = cozk.Harness(mode=mode, **cfg)
    _, got = _prove(h)
    h.close()
    assert got == _c_oracle_proof(frozenset(cfg.items()))


def test_grand_product_harness_without_window_table_equals_c_oracle(cozk):
    """precompute=False: the 16-window-group MSM (k_msm_hist / k_msm_scatter / k_msm_accum0, G = 16 bucket groups; at most 4
    polynomials per launch set and 16 per tail chunk, host/msm_schedule.hpp: msm_schedule), so the 128 commit polynomials of the bench mix run
    as tail chunks of at most 16 and launch sets of at most 4 polynomials, the cheapest set of a chunk rotated to the
    front (host/msm_schedule.hpp: msm_schedule).  Same bytes as with the table."""
    cfg = GP_SHAPES["bench_2p14"]
    for mode in ("plain", "rep3"):
        h = cozk.Harness(mode=mode, precompute=False, **cfg)
        _, got = _prove(h)
        h.close()
        assert got == _c_oracle_proof(frozenset(cfg.items())), mode


# ---------------------------------------------------------------- (b) 2^18 / 2^20 against the C oracle's committed digests
def _scale_row(log_n):
    rows = [r for r in SCALE if r["cfg"]["log_n"] == log_n]
    assert len(rows) == 1
    return rows[0]


@pytest.mark.parametrize("log_n,mode", [(18, "plain"), (18, "rep3"), (20, "plain")])
def test_production_sizes_equal_committed_c_oracle_digests(cozk, log_n, mode):
    """the bench workload itself (2^20 cycles, bench.py) and the same mix at 2^18: digest and length == the C oracle's
    (tests/golden/scale_pipelines.json).  Beyond (a): the level-0 MSM segment length L0 = M >> 18 grows past 8 once a launch set
    holds more than 2^21 references (host/msm_schedule.hpp: msm_set_counts) -- 64 FR columns x 2^18 scalars x 16 windows -- and the reducing
    kernels stride their grid past MAXBLK = 2048 workgroups x 256 lanes = 2^19 elements (grid_capped)."""
    row = _scale_row(log_n)
    cfg = dict(row["cfg"])
    cfg.pop("mode")
    h = cozk.Harness(mode=mode, **cfg)
    res, got = _prove(h)
    h.close()
    assert _digest(res) == row["digest"] and len(got) == row["proof_len"]


# ---------------------------------------------------------------- (c) Python-oracle pipelines past their thresholds
def test_spartan_2p10_equals_python_oracle(cozk):
    """co-noir Spartan at log_n = 10 (oracle/pyspartan.py, live), plain and Rep3 == the oracle's bytes.  Over the log_n = 6
    check this size adds multi-workgroup grids: round 0 of both sumchecks (k_spartan_first / k_spartan_second, BATCH_GRID_MAX)
    on 2 workgroups and the transposed sparse mat-vec (k_sparse_matvec3_rows / _items) on about 50; the commit of z sorts its
    1024 scalars on one workgroup (host/msm_schedule.hpp: msm_sort_wgs).  No 9 x 29 kernel runs at this size (kernel trace of one prove)."""
    import pyspartan
    ref = pyspartan.run(dict(log_n=10, seed=2026))
    assert ref["verified"]
    for mode in ("plain", "rep3"):
        h = cozk.SpartanHarness(mode=mode, log_n=10, seed=2026)
        _, got = _prove(h)
        h.close()
        assert got == ref["proof_bytes"], mode


def test_spartan_2p10_lookup_round_equals_committed_oracle_digest(cozk):
    """the same with the public lookup round (pyspartan lookup_round=1): the oracle takes over a minute at this size, so its
    digest is committed (tests/golden/scale_pipelines.json, "spartan").  Plain and Rep3 == that digest and length."""
    rows = SCALE_GOLD["spartan"]
    assert len(rows) == 1
    row = rows[0]
    cfg = row["cfg"]
    for mode in ("plain", "rep3"):
        h = cozk.SpartanHarness(mode=mode, log_n=cfg["log_n"], seed=cfg["seed"], lookup_round=bool(cfg["lookup_round"]))
        res, got = _prove(h)
        h.close()
        assert _digest(res) == row["digest"] and len(got) == row["proof_len"], mode


def test_lookups_primary_2p12_equals_python_oracle(cozk):
    """instruction lookups with the primary sumcheck, 54 memory pairs at 2^12 (oracle/pylookups.py), plain and Rep3 == the
    oracle's plain bytes (Rep3 == plain: tests/test_gpu_lookups.py).  The toggle layer holds 54 circuits x 2^12 leaves under a
    nested split-eq, so its first rounds have 54 x 2^11 >= 4096 pairs and run k_toggle_cubic9 (TOGGLE_F9_MIN_PAIRS; six rounds in a
    kernel trace, the first on the packed 0/1 bytes)."""
    import pylookups
    LK = importlib.import_module("co-zkvms_amd.lookups")
    cfg = dict(log_n=12, n_pairs=54, density_pct=10, seed=2026)
    ref = pylookups.run(dict(cfg, mode="plain", primary=1, mix=0))
    assert ref["verified"]
    for mode in ("plain", "rep3"):
        h = LK.LookupsHarness(mode=mode, primary=True, **cfg)
        _, got = _prove(h)
        h.close()
        assert got == ref["proof_bytes"], mode


@pytest.mark.parametrize("log_steps", [10, 12])
def test_jolt_spartan_worker_equals_python_oracle(cozk, log_steps):
    """the whole co-jolt Spartan worker (outer + inner + shift sumchecks) on the reference's constraint set at 2^10 / 2^12
    steps (oracle/pyspartan_outer.py run_full), plain and Rep3 == the oracle's plain bytes (Rep3 == plain:
    tests/test_gpu_outer.py).  The outer rounds over the active rows run k_outer_round_act9 once
    num_steps * act_rows / 2 >= 1024 (OUTER_F9_MIN_PAIRS): its first rounds at both sizes (seven at 2^10 in a kernel
    trace)."""
    import pyspartan_outer
    OU = importlib.import_module("co-zkvms_amd.outer")
    ref = pyspartan_outer.run_full(dict(mode="plain", log_steps=log_steps, seed=2026, system="jolt"))
    assert ref["verified"]
    for mode in ("plain", "rep3"):
        h = OU.OuterHarness(mode=mode, log_steps=log_steps, seed=2026, system="jolt", full=True)
        _, got = _prove(h)
        h.close()
        assert got == ref["proof_bytes"], mode


def test_flow_2p8_jolt_memories_equals_committed_oracle_digest(cozk):
    """the chained worker flow at 2^8 cycles with Jolt's 54 memories and 26 subtables: oracle/pyflow.py takes over a minute
    here, so its digest is committed (tests/golden/scale_pipelines.json, "flow").  Plain and Rep3 == that digest and length
    (Rep3 == plain: tests/test_gpu_flow.py).  The lookup toggle layer has 54 x 2^7 >= 4096 pairs under a nested split-eq
    (k_toggle_cubic9, TOGGLE_F9_MIN_PAIRS), its Spartan outer rounds run k_outer_round_act9 (OUTER_F9_MIN_PAIRS),
    and its MSMs run the fold levels k_msm_accumN (host/msm_schedule.hpp: msm_set_counts) -- all seen in a kernel trace of one prove."""
    FL = importlib.import_module("co-zkvms_amd.flow")
    rows = SCALE_GOLD["flow"]
    assert len(rows) == 1
    row = rows[0]
    cfg = dict(row["cfg"])
    cfg.pop("mode")
    for mode in ("plain", "rep3"):
        h = FL.FlowHarness(mode=mode, **cfg)
        res, got = _prove(h)
        h.close()
        assert _digest(res) == row["digest"] and len(got) == row["proof_len"], mode


# ---------------------------------------------------------------- (d) MSM == the C Pippenger
SRS_N = (1 << 18) + 64


def _bases_raw(B, offset, n):
    xy = np.zeros((n, 8), dtype=np.uint64)
    inf = np.zeros(n, dtype=np.uint8)
    B.ctx.check(B.ctx._l.cozk_bases_download(B.ctx.h, B.h, offset, n, xy.ctypes.data, inf.ctypes.data))
    return xy, inf


@pytest.fixture(scope="module")
def srs(cozk, ctx):
    """one SRS of 2^18 + 64 points made on the device (bases[i] = s_i G), with and without the window table, plus its
    affine coordinates on the host for the oracle"""
    s = cozk.Vec.random(ctx, SRS_N, seed=8080)
    out = {pre: cozk.Bases.from_scalars(ctx, s, precompute=pre) for pre in (True, False)}
    xy, inf = _bases_raw(out[True], 0, SRS_N)
    assert not inf.any()
    yield out, xy, inf
    for B in out.values():
        B.free()
    s.free()


def _fr_mont_of(v):
    """a device scalar vector as Fr Montgomery limbs (what coracle.msm takes)"""
    if v.kind == importlib.import_module("co-zkvms_amd").SCALAR_FR:
        return v.to_numpy()
    return fr_mont([x % O.R for x in v.to_ints()])


def fr_mont(vals):
    cozk = importlib.import_module("co-zkvms_amd")
    return cozk.fr_to_mont_limbs(vals)


def _oracle_point(xy, inf, sc_mont):
    out, oinf = coracle.msm(xy, inf, sc_mont)
    return None if oinf else (tuple(int(x) for x in out[:4]), tuple(int(x) for x in out[4:]))


def _raw_point(xy8, inf):
    return None if inf else (tuple(int(x) for x in xy8[:4]), tuple(int(x) for x in xy8[4:]))


def _edge_scalars(sc_mont, n):
    """edge values at the first and last index of every 4096-scalar range (the LDS sort's unit of work per workgroup)"""
    idx = sorted({i for b in range(0, n, 4096) for i in (b, min(b + 4095, n - 1))})
    vals = [EDGE[j % len(EDGE)] for j in range(len(idx))]
    sc_mont[idx] = fr_mont(vals)
    return sc_mont


@pytest.mark.parametrize("precompute", [True, False])
@pytest.mark.parametrize("n,offset", [(4097, 5), ((1 << 16) + 3, 61), (1 << 18, 0)])
def test_msm_equals_c_pippenger(cozk, ctx, srs, n, offset, precompute):
    """one MSM over bases[offset .. offset + n), random scalars with edge values at both ends of every 4096-scalar range.
    With the table: k_msm_hist_lds / k_msm_scatter_lds on ceil(n / 4096) = 2, 17, 64 workgroups (host/msm_schedule.hpp: msm_sort_wgs, capped at
    64); k_msm_accumN fold levels once a bucket holds more than L0 references (host/msm_schedule.hpp: msm_set_counts: 16 n / 2^15 per bucket on
    average); L0 = M >> 18 = 16 at 2^18 (host/msm_schedule.hpp: msm_set_counts).  Without it: the 16-window-group kernels (k_msm_hist /
    k_msm_scatter / k_msm_accum0) on cdiv(n, 256) workgroups."""
    Bs, xy, inf = srs
    s = _edge_scalars(cozk.Vec.random(ctx, n, seed=n + 7 * offset).to_numpy(), n)
    v = cozk.Vec.from_numpy(ctx, s)
    got = Bs[precompute].msm(v, offset=offset)
    want = _oracle_point(xy[offset:offset + n], inf[offset:offset + n], s)
    assert cozk.point_to_abi(got)[0].tolist() == (list(want[0]) + list(want[1]) if want else [0] * 8)
    v.free()


@pytest.mark.parametrize("precompute", [True, False])
def test_msm_bases_with_infinity_2p16(cozk, ctx, precompute):
    """2^16 bases of which every 97th (and the first and last) is the point at infinity (a zero SRS scalar): the window table
    marks has_inf and the gather runs k_msm_accum0_f9<true> with the k_msm_accum0_fix fix-up pass (csrc/msm.hip: msm_accumulate);
    without the table k_msm_accum0 skips them.  Exact == the C Pippenger."""
    n = 1 << 16
    s = cozk.Vec.random(ctx, n, seed=4141).to_numpy()
    zero_at = list(range(0, n, 97)) + [n - 1]
    s[zero_at] = 0
    B = cozk.Bases.from_scalars(ctx, cozk.Vec.from_numpy(ctx, s), precompute=precompute)
    xy, inf = _bases_raw(B, 0, n)
    assert inf.sum() == len(set(zero_at))
    sc = _edge_scalars(cozk.Vec.random(ctx, n, seed=4242).to_numpy(), n)
    got = B.msm(cozk.Vec.from_numpy(ctx, sc))
    want = _oracle_point(xy, inf, sc)
    assert cozk.point_to_abi(got)[0].tolist() == (list(want[0]) + list(want[1]) if want else [0] * 8)
    B.free()


KINDS = ("FR", "U8", "U16", "I64")


def _batch_vecs(cozk, ctx, k, seed, max_len):
    """k scalar vectors of mixed kinds and lengths, each on its own base slice; polynomial 3 has length zero"""
    vecs, offs, lens = [], [], []
    rng = O.SplitMix64(seed)
    for p in range(k):
        kind = KINDS[p % 4]
        n = 1 + rng.next() % max_len
        kw = dict(kind=getattr(cozk, "SCALAR_" + kind))
        if kind == "U8":
            kw["max_bits"] = 1
        vecs.append(cozk.Vec.random(ctx, n, seed=seed * 1000 + p, **kw))
        lens.append(0 if p == 3 else n)
        offs.append(1 + rng.next() % (SRS_N - n - 1))
    return vecs, offs, lens


def batch_points(cozk, ctx, B, vecs, offs, lens):
    """cozk_batch_msm_slices -> raw points (Montgomery limbs, or None)"""
    k = len(vecs)
    arr = (ctypes.c_void_p * k)(*[v.h for v in vecs])
    o = np.asarray(offs, dtype=np.uint64)
    ln = np.asarray(lens, dtype=np.uint64)
    out = np.zeros((k, 8), dtype=np.uint64)
    inf = np.zeros(k, dtype=np.int32)
    ctx.check(ctx._l.cozk_batch_msm_slices(ctx.h, B.h, o.ctypes.data, arr, ln.ctypes.data, k, out.ctypes.data, inf.ctypes.data))
    return [_raw_point(out[i], inf[i]) for i in range(k)]


# (k, precompute, longest polynomial): 70 with the table = launch sets of 64 + 6 on two streams, polynomials of up to 9000
# scalars sorted by up to 3 workgroups each (host/msm_schedule.hpp: msm_sort_wgs); 20 without = tail chunks of
# 16 + 4 (tail_cap = 256 / 16), the first cut into 4 launch sets of 4 and rotated; 300 with the table = tail chunks of 256 + 44,
# the first cut into 4 launch sets of 64 and rotated (host/msm_schedule.hpp: msm_schedule)
BATCHES = {"k70_table": (70, True, 9000), "k20_groups": (20, False, 5000), "k300_table": (300, True, 600)}


def _batch_case(cozk, ctx, Bs, name):
    k, pre, max_len = BATCHES[name]
    vecs, offs, lens = _batch_vecs(cozk, ctx, k, 31 + k, max_len)
    return vecs, offs, lens, batch_points(cozk, ctx, Bs[pre], vecs, offs, lens)


@pytest.mark.parametrize("name", sorted(BATCHES))
def test_batch_msm_mixed_kinds_and_slices_equal_c_pippenger(cozk, ctx, srs, name):
    """batched MSM with per-polynomial base slices at nonzero offsets, mixed scalar kinds (FR, 0/1 U8, U16, I64) and one
    zero-length polynomial: every point == the C Pippenger over its slice.  Launch-set and tail-chunk cuts: see BATCHES."""
    Bs, xy, inf = srs
    vecs, offs, lens, got = _batch_case(cozk, ctx, Bs, name)
    for p, (v, o, n) in enumerate(zip(vecs, offs, lens)):
        sc = _fr_mont_of(v)[:n]
        want = _oracle_point(xy[o:o + n], inf[o:o + n], sc) if n else None
        assert got[p] == want, (name, p, KINDS[p % 4], n)
    for v in vecs:
        v.free()


# 12 FR polynomials of up to 2^18 scalars (2^22 references each): one launch set by default; 3 sets of 4 under a 2^24-reference
# cap (COZK_MSM_SET_REFS_LOG2=24, host/msm_schedule.hpp: MsmOptions::set_refs_log2), the cheapest set rotated to the front
BIG_LENS = [(1 << 18) - 17 * i for i in range(11)] + [(1 << 16) + 5]


def big_batch_points(cozk, ctx, B):
    vecs = [cozk.Vec.random(ctx, n, seed=700 + i) for i, n in enumerate(BIG_LENS)]
    offs = [3 * i + 1 for i in range(len(BIG_LENS))]
    got = batch_points(cozk, ctx, B, vecs, offs, list(BIG_LENS))
    return vecs, offs, got


_CHILD = r"""
import importlib, json, sys
sys.path[:0] = [{root!r}, {oracle!r}, {tests!r}]
import test_gpu_scale_parity as T
cozk = importlib.import_module("co-zkvms_amd")
ctx = cozk.Context(0)
s = cozk.Vec.random(ctx, T.SRS_N, seed=8080)
Bs = {{pre: cozk.Bases.from_scalars(ctx, s, precompute=pre) for pre in (True, False)}}
out = {{name: T._batch_case(cozk, ctx, Bs, name)[3] for name in sorted(T.BATCHES)}}
out["big"] = T.big_batch_points(cozk, ctx, Bs[True])[2]
print("POINTS " + json.dumps(out))
ctx.close()
"""


def test_batch_msm_serial_and_small_launch_sets_in_a_fresh_process(cozk, ctx, srs):
    """COZK_MSM_SERIAL=1 (no second stream, host/msm_schedule.hpp: MsmOptions::serial) and COZK_MSM_SET_REFS_LOG2=24 (launch sets cut at 2^24
    references, host/msm_schedule.hpp: MsmOptions::set_refs_log2) are read once per process, so this leg runs in a child: its points of every batch above and
    of a 12 x 2^18 batch (one launch set by default, 3 rotated sets under the cap) == the default run's; the default run of the
    big batch == the C Pippenger."""
    Bs, xy, inf = srs
    want = {}
    for name in sorted(BATCHES):
        vecs, _, _, want[name] = _batch_case(cozk, ctx, Bs, name)
        for v in vecs:
            v.free()
    vecs, offs, want["big"] = big_batch_points(cozk, ctx, Bs[True])
    for p, (v, o, n) in enumerate(zip(vecs, offs, BIG_LENS)):
        assert want["big"][p] == _oracle_point(xy[o:o + n], inf[o:o + n], v.to_numpy()), p
        v.free()
    env = dict(os.environ, COZK_MSM_SERIAL="1", COZK_MSM_SET_REFS_LOG2="24")
    code = _CHILD.format(root=ROOT, oracle=os.path.join(ROOT, "oracle"), tests=HERE)
    r = subprocess.run(["timeout", "-k", "10", "300", sys.executable, "-c", code], env=env, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("POINTS ")][-1]
    got = json.loads(line[len("POINTS "):])
    for name, pts in want.items():
        assert [None if p is None else [list(p[0]), list(p[1])] for p in pts] == got[name], name


# ---------------------------------------------------------------- (e) reductions past their grid caps == big-int sums
def _ints(limbs):
    """(n, 4) uint64 Montgomery limbs -> the Montgomery integers (not reduced out of Montgomery form)"""
    b = np.ascontiguousarray(limbs, dtype=np.uint64).tobytes()
    return [int.from_bytes(b[32 * i:32 * i + 32], "little") for i in range(len(b) // 32)]


def _poly_raw(p):
    n = len(p)
    a = np.empty((n, 4), dtype=np.uint64)
    b = np.empty((n, 4), dtype=np.uint64)
    p.ctx.check(p.ctx._l.cozk_poly_download(p.ctx.h, p.h, a.ctypes.data, b.ctypes.data))
    return a, b


@pytest.mark.parametrize("mode", ["plain", "rep3"])
@pytest.mark.parametrize("base_len", [3 * (1 << 15) + 5, (1 << 19) + 7])
def test_reductions_past_grid_caps_equal_big_int_sums(cozk, ctx, mode, base_len):
    """batch_evaluate_at_chi, dot_product_with_public and linear_combination on ragged lengths around 3 * 2^15 + 5 and
    2^19 + 7, with chi longer than every polynomial.  k_poly_eval_chi caps its grid at 192 workgroups (EVAL_GRID_MAX), so
    above 192 x 256 = 49 152 elements a lane holds several; the grid-capped reducing kernels (dot product, linear combination)
    stop at MAXBLK = 2048 workgroups (grid_capped) and stride past 2^19 elements."""
    L = importlib.import_module("co-zkvms_amd._lib")
    md = L.MODE_PLAIN if mode == "plain" else L.MODE_REP3
    lens = [base_len, base_len - 6, base_len - 4097]
    polys = [cozk.Rep3DensePolynomial.random(ctx, n, seed=90 + i + base_len, mode=md) for i, n in enumerate(lens)]
    chi = cozk.Vec.random(ctx, base_len + 9, seed=base_len)
    raw = [_poly_raw(p) for p in polys]
    A = [_ints(a) for a, _ in raw]
    B = [_ints(b) for _, b in raw] if mode == "rep3" else None
    C = _ints(chi.to_numpy())
    r2 = RINV * RINV % O.R

    def dot(x, y):
        return sum(u * w for u, w in zip(x, y)) * r2 % O.R

    got = cozk.Rep3DensePolynomial.batch_evaluate_at_chi(polys, chi)
    if mode == "plain":
        want = [dot(a, C) for a in A]
    else:
        want = [(dot(a, C) + dot(b, C)) * O.TWO_INV % O.R for a, b in zip(A, B)]
    assert got == want
    pub = cozk.Vec.random(ctx, lens[1], seed=77)
    P = _ints(pub.to_numpy())
    d = polys[1].dot_product_with_public(pub)
    assert d == (dot(A[1], P) if mode == "plain" else (dot(A[1], P), dot(B[1], P)))
    cf = [O.R - 3, (1 << 200) + 9, 5]
    lc = cozk.Rep3DensePolynomial.linear_combination(polys, cf)
    la, lb = _poly_raw(lc)
    for comp, got_limbs in ((A, la),) + (((B, lb),) if mode == "rep3" else ()):
        acc = [0] * base_len
        for c, col in zip(cf, comp):
            for i, v in enumerate(col):
                acc[i] += c * v
        assert _ints(got_limbs) == [x % O.R for x in acc]
    for p in polys + [lc]:
        p.free()
    chi.free()
    pub.free()
