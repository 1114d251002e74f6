"""CPU: the launch schedule of the batched MSM (csrc/host/msm_schedule.hpp: msm_schedule), restated in a few lines of Python.

Two rules decide how a launch set is sorted:
  shape       a set's sort takes the wide shape (1024 threads) when the set launched before it places fewer than an eighth
              of the references the set itself places (its gather cannot hide the sort), or when there is no such set; otherwise
              the 256-thread shape that slips under the running gather;
  workgroups  per run of columns of one kind: FR columns one workgroup per 4096 scalars, every other kind one per 2^16
              digits (n x windows of the kind), at least 1, at most 64.
plan() restates what a set needs beyond that (segment length, segment count, fold levels), blocks() the cut into tail blocks, and
batch() puts all of it together.  test_msm_schedule_host.py holds the library's own schedule function to batch() on the CPU, at the
benchmark's sizes too; the GPU tests (test_gpu_msm_schedule.py) compare the COZK_TRACE_MSM lines of the library with what these
functions say.  Nothing here is derived from the C++, so the numbers expected there do not come from the code under test."""
NWIN = {"FR": 16, "U8": 1, "U16": 2, "U32": 3, "U64": 5, "I64": 5}
KIND_ORDER = ["FR", "U8", "U16", "U32", "U64", "I64"]  # the order in which the kind runs of a set are launched
MAX_POLYS = 64         # per launch set on a window table
MAX_POLYS_GROUPS = 4   # ... and without one, where every column is 16 bucket groups
TAIL_GROUPS = 256      # bucket groups per tail block
BUCKETS = 1 << 15
WGS_MAX = 64
WG_DIGITS_LOG2 = 16
WIDE, NARROW = "wide", "narrow"


def refs(col):
    kind, n = col
    return n * NWIN[kind]


def cut_sets(cols, cap, max_polys=MAX_POLYS):
    """cols: [(kind, n)] in the caller's order; a set takes columns while it stays within `cap` references (one column always fits)"""
    sets, cur, m = [], [], 0
    for c in cols:
        if cur and (m + refs(c) > cap or len(cur) == max_polys):
            sets.append(cur)
            cur, m = [], 0
        cur.append(c)
        m += refs(c)
    if cur:
        sets.append(cur)
    return sets


def default_cap(cols):
    return min(max(sum(refs(c) for c in cols) // 4, 1 << 28), 1 << 30)


def launch_order(sets):
    """more than two sets: the cheapest one (the first of them on a tie) moves to the front, the others keep their order"""
    if len(sets) <= 2:
        return list(sets)
    m = [sum(refs(c) for c in s) for s in sets]
    best = m.index(min(m))
    return [sets[best]] + sets[:best] + sets[best + 1:]


def shapes(ordered):
    out, pred = [], 0
    for s in ordered:
        own = sum(refs(c) for c in s)
        out.append(WIDE if 8 * pred < own else NARROW)
        pred = own
    return out


def workgroups(s, digits_log2=WG_DIGITS_LOG2, wgs_max=WGS_MAX):
    """[(kind, columns, workgroups per column)] of a set, in launch order"""
    out = []
    for kind in KIND_ORDER:
        ns = [n for k, n in s if k == kind and n]
        if not ns:
            continue
        if kind == "FR" or digits_log2 == 0:
            w = -(-max(ns) // 4096)
        else:
            w = -(-max(ns) * NWIN[kind] // (1 << digits_log2))
        out.append((kind, len(ns), min(max(w, 1), wgs_max)))
    return out


def schedule(cols, cap=None, digits_log2=WG_DIGITS_LOG2):
    """[(columns, references, shape, workgroups)] per launch set, in launch order"""
    ordered = launch_order(cut_sets(cols, default_cap(cols) if cap is None else cap))
    return [(len(s), sum(refs(c) for c in s), sh, workgroups(s, digits_log2)) for s, sh in zip(ordered, shapes(ordered))]


def blocks(cols, table=True):
    """the bucket-reduction tail runs once per block of 256 bucket groups: 256 columns on a window table, 16 without"""
    cap = TAIL_GROUPS if table else TAIL_GROUPS // 16
    return [cols[i:i + cap] for i in range(0, len(cols), cap)]


def plan(s, table=True):
    """what one launch set needs.  L0: level-0 segments are refs / 2^18 long, within [8, 127].  Fold levels: the fullest ordinary
    bucket holds the references of the longest column spread over 2^15 buckets (all its windows on a table, one window without),
    a quarter more for the spread, in segments of L0, plus one; every level folds 8 into 1 and there is at least one level."""
    groups = 1 if table else 16
    nb = len(s) * groups * BUCKETS
    m = sum(refs(c) for c in s)
    L0 = min(max(m >> 18, 8), 127)
    per = max(-(-(n * (NWIN[kind] if table else 1)) // BUCKETS) for kind, n in s)
    segs = -(-(per * 5) // (4 * L0)) + 1
    levels = 1
    while -(-segs // 8) > 1:
        segs = -(-segs // 8)
        levels += 1
    maxseg0 = m // L0 + nb
    part = max(maxseg0, 2 * nb)
    return dict(G=groups, nb=nb, refs=m, bound=max(refs(c) for c in s), L0=L0, maxseg0=maxseg0, fold_levels=levels, part=part, exc=maxseg0 + 2,
                blk=-(-part // 256) + 2)


def batch(cols, table=True, cap=None, digits_log2=WG_DIGITS_LOG2, shape_rule=True, serial=False, offset_forms=True):
    """[[set, ...] per tail block], sets in launch order: plan() of the set plus its first column in the caller's order, its index,
    its sort workspace, shape, kind runs and the columns that may take the offset digit form (bit p: column p of the set).  A block
    of more than one set pipelines unless the batch is serial; only then does a sort run beside the set in front.  shape_rule=False
    is the rule before: wide for the first set of the batch and wherever nothing is pipelined."""
    out, start = [], 0
    for b, bc in enumerate(blocks(cols, table)):
        cut = cut_sets(bc, default_cap(bc) if cap is None else cap, MAX_POLYS if table else MAX_POLYS_GROUPS)
        first = {}
        for s in cut:
            first[id(s)] = start
            start += len(s)
        ordered = launch_order(cut)
        pipelined = len(ordered) > 1 and not serial
        sets, pred = [], 0
        for i, s in enumerate(ordered):
            p = plan(s, table)
            wide = 8 * pred < p["refs"] if shape_rule else (b == 0 and i == 0) or not pipelined
            pred = p["refs"] if pipelined else 0
            elig = sum(1 << j for j, (kind, n) in enumerate(s) if table and offset_forms and n and kind in ("U16", "U32", "U64"))
            sets.append(dict(p, first=first[id(s)], polys=len(s), index=i, ws=i % 2, shape=WIDE if wide else NARROW, pipelined=pipelined,
                             groups=len(bc) * p["G"], kinds=workgroups(s, digits_log2) if table and p["refs"] else [], elig=elig))
        out.append(sets)
    return out


def bench_mix(n):
    return [("FR", n)] * 64 + [("U16", n)] * 32 + [("U32", n)] * 16 + [("U8", n)] * 16


def test_bench_commit_at_2p20():
    """128 columns: three sets of 18 field-element columns, the mixed set, ten flag columns; the flags go first, the first
    field-element set is then sorted wide (10 M references in front of 302 M), everything after it narrow"""
    n = 1 << 20
    got = schedule(bench_mix(n))
    assert [(p, m >> 20) for p, m, _, _ in got] == [(10, 10), (18, 288), (18, 288), (18, 288), (64, 278)]
    assert [sh for _, _, sh, _ in got] == [WIDE, WIDE, NARROW, NARROW, NARROW]
    assert got[0][3] == [("U8", 10, 16)]
    assert got[1][3] == [("FR", 18, 64)]
    assert got[4][3] == [("FR", 10, 64), ("U8", 6, 16), ("U16", 32, 32), ("U32", 16, 48)]
    # the rule before: every kind 64 workgroups
    assert workgroups(cut_sets(bench_mix(n), default_cap(bench_mix(n)))[3], 0) == [("FR", 10, 64), ("U8", 6, 64), ("U16", 32, 64), ("U32", 16, 64)]


MANY = [("FR", 1024)] * 12 + [("U16", 1024)] * 6 + [("U32", 1024)] * 3 + [("U8", 1024)] * 3


def test_many_small_sets():
    """the 24-column batch of the GPU test under a 2^12 cap: 19 sets, the two trailing flags in front"""
    got = schedule(MANY, cap=1 << 12)
    assert len(got) == 19
    assert got[0][:2] == (2, 2048) and got[0][2] == WIDE
    assert got[1][:3] == (1, 16384, NARROW)        # 2048 references in front of 16384: an eighth, not fewer
    assert all(g[2] == NARROW for g in got[1:])    # equal or shrinking sets hide behind their predecessor
    assert got[-1][3] == [("U8", 1, 1), ("U32", 1, 1)]


def small_large(flag_first):
    flag, fr = [("U8", 4096)], [("FR", 4096)] * 8
    return flag + fr if flag_first else fr + flag


def test_small_set_in_front_of_a_large_one_and_the_reverse():
    # one column per set: flag, then eight field-element sets; the first of those has 4096 references in front of 65536
    a = schedule(small_large(True), cap=1 << 16)
    assert [g[2] for g in a] == [WIDE, WIDE] + [NARROW] * 7
    # the reverse order cut the same way: the flag set is the cheapest and moves to the front, same schedule
    assert schedule(small_large(False), cap=1 << 16) == a
    # two sets keep their order: eight field-element columns (wide, nothing in front), then the flag behind 2^19 references
    b = schedule(small_large(False), cap=1 << 19)
    assert [(g[0], g[2]) for g in b] == [(8, WIDE), (1, NARROW)]
    # flag and seven field-element columns share the first set; the eighth follows 462848 references: narrow
    c = schedule(small_large(True), cap=1 << 19)
    assert [(g[0], g[1], g[2]) for g in c] == [(8, 4096 + 7 * 65536, WIDE), (1, 65536, NARROW)]
    assert c[0][3] == [("FR", 7, 1), ("U8", 1, 1)]
    assert schedule(small_large(True), cap=1 << 19, digits_log2=11)[0][3] == [("FR", 7, 1), ("U8", 1, 2)]


def test_workgroup_edges():
    for kind, nwin in NWIN.items():
        if kind == "FR":
            continue
        one = (1 << 12) // nwin          # the longest column with one workgroup at 2^12 digits per workgroup
        assert workgroups([(kind, one)], 12) == [(kind, 1, 1)]
        assert workgroups([(kind, one + 1)], 12) == [(kind, 1, 2)]
    assert workgroups([("FR", 4096)]) == [("FR", 1, 1)] and workgroups([("FR", 4097)]) == [("FR", 1, 2)]
    assert workgroups([("U16", 1 << 26)]) == [("U16", 1, 64)]
