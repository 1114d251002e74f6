"""Lasso counters over an identity table, and the dealer's timestamp range-check witness made of them, as plain Python (jolt-core's
TimestampRangeCheckPolynomials::generate_witness, whose four families jolt/witness.rs:384-409 shares as public vectors; jolt-core is
not in the reference tree, so the loop is restated from upstream knowledge and pinned by the multiset identity below).  For one
column of keys over a table of M entries, with a table of counters c = 0:

  read_cts[j] = c[key[j]];  c[key[j]] += 1          and at the end   final_cts = c

`time_counters` is that loop per column; `ts_range` applies it to key = t_read[s][j] and key = j - t_read[s][j] of every slot;
`hashes` gives the four products of the offline memory checking of one column over Fr, with tuples (key, key, count) and
h(a, v, t) = t g^2 + v g + a - tau (as tests/rw_witness_ref.py):

  init = prod_a h(a, a, 0)   writes = prod_j h(k_j, k_j, read_cts_j + 1)   reads = prod_j h(k_j, k_j, read_cts_j)   final = prod_a h(a, a, final_cts[a])"""
import pyref as O

R = O.R


def counters(keys, M):
    c, read_cts = [0] * M, [0] * len(keys)
    for j, k in enumerate(keys):
        if k >= M:
            raise ValueError("step %d: key %d >= M = %d" % (j, k, M))
        read_cts[j] = c[k]
        c[k] += 1
    return read_cts, c


def time_counters(keys, M):
    """keys: one list per column.  Returns (read_cts, final_cts), one list per column each."""
    out = [counters(col, M) for col in keys]
    return [o[0] for o in out], [o[1] for o in out]


def ts_range(t_read, M):
    """t_read: one list of n read timestamps per slot, M >= n.  Returns (read_cts_read_timestamp, read_cts_global_minus_read,
    final_cts_read_timestamp, final_cts_global_minus_read), one list per slot each."""
    n = len(t_read[0])
    assert M >= n and all(len(col) == n for col in t_read)
    for j in range(n):
        for s, col in enumerate(t_read):
            if col[j] > j:
                raise ValueError("step %d, slot %d: t_read %d > the step" % (j, s, col[j]))
    rc_rt, fc_rt = time_counters(t_read, M)
    rc_gmr, fc_gmr = time_counters([[j - t for j, t in enumerate(col)] for col in t_read], M)
    return rc_rt, rc_gmr, fc_rt, fc_gmr


def fingerprint(a, v, t, g, tau):
    return (t * g % R * g + v * g + a - tau) % R


def hashes(keys, read_cts, final_cts, g, tau):
    """(init, writes, reads, finals) of one column"""
    init = wr = rd = fin = 1
    for a, c in enumerate(final_cts):
        init = init * fingerprint(a, a, 0, g, tau) % R
        fin = fin * fingerprint(a, a, c, g, tau) % R
    for k, c in zip(keys, read_cts):
        rd = rd * fingerprint(k, k, c, g, tau) % R
        wr = wr * fingerprint(k, k, c + 1, g, tau) % R
    return init, wr, rd, fin
