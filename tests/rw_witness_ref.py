"""The dealer's read-write memory witness as plain Python (jolt-core's ReadWriteMemoryPolynomials::generate_witness, shared by
read_write_memory/witness.rs:34-93).  n_slots address columns of n steps over ONE memory of MEM words; the operations are ordered by
(step j, slot s).  From v = v_init, t = 0, per operation with a = addr[s][j]:

  v_read[s][j] = v[a];  t_read[s][j] = t[a];  w = v_write[s][j] if slot s writes at step j else v[a];  v[a] = w;  t[a] = j

and v_final = v, t_final = t at the end.  `replay` is that loop, `sort_and_sweep` the formulation the device uses (stable sort by
address, then one sweep per address), `hashes` the four products of the offline memory checking over Fr with
h(a, v, t) = t g^2 + v g + a - tau (as tests/lasso_witness_ref.py)."""
import pyref as O

R = O.R


def writes(v_write, is_write, s, j):
    return v_write[s] is not None and (is_write[s] is None or bool(is_write[s][j]))


def _check(addr, v_write, is_write, v_init):
    n, MEM = len(addr[0]), len(v_init)
    for s in range(len(addr)):
        assert len(addr[s]) == n and (v_write[s] is None or len(v_write[s]) == n) and (is_write[s] is None or len(is_write[s]) == n)
        assert is_write[s] is None or v_write[s] is not None
    for j in range(n):
        for s in range(len(addr)):
            if addr[s][j] >= MEM:
                raise ValueError("step %d, slot %d: address %d >= MEM = %d" % (j, s, addr[s][j], MEM))
    return n, MEM


def replay(addr, v_write, is_write, v_init):
    """Returns (v_read, t_read, v_written, v_final, t_final): per-slot lists (v_written None for a slot without flags) and two
    lists of MEM entries."""
    n, MEM = _check(addr, v_write, is_write, v_init)
    ns = len(addr)
    v, t = list(v_init), [0] * MEM
    v_read, t_read, w_all = [[0] * n for _ in range(ns)], [[0] * n for _ in range(ns)], [[0] * n for _ in range(ns)]
    for j in range(n):
        for s in range(ns):
            a = addr[s][j]
            v_read[s][j], t_read[s][j] = v[a], t[a]
            w = v_write[s][j] if writes(v_write, is_write, s, j) else v[a]
            v[a], t[a] = w, j
            w_all[s][j] = w
    return v_read, t_read, [w_all[s] if is_write[s] is not None else None for s in range(ns)], v, t


def sort_and_sweep(addr, v_write, is_write, v_init):
    n, MEM = _check(addr, v_write, is_write, v_init)
    ns = len(addr)
    ops = sorted(range(n * ns), key=lambda i: addr[i % ns][i // ns])  # Python's sort is stable: equal addresses stay in (j, s) order
    v_read, t_read, w_all = [[0] * n for _ in range(ns)], [[0] * n for _ in range(ns)], [[0] * n for _ in range(ns)]
    v_final, t_final = list(v_init), [0] * MEM
    last_write = None  # position of the last write so far, over all addresses
    for q, i in enumerate(ops):
        j, s = divmod(i, ns)
        a = addr[s][j]
        vr = v_init[a]
        if last_write is not None:
            jp, sp = divmod(ops[last_write], ns)
            if addr[sp][jp] == a:
                vr = v_write[sp][jp]
        tr = 0
        if q > 0:
            jn, sn = divmod(ops[q - 1], ns)
            if addr[sn][jn] == a:
                tr = jn
        w = v_write[s][j] if writes(v_write, is_write, s, j) else vr
        if writes(v_write, is_write, s, j):
            last_write = q
        v_read[s][j], t_read[s][j], w_all[s][j] = vr, tr, w
        v_final[a], t_final[a] = w, j  # the last operation of the address wins
    return v_read, t_read, [w_all[s] if is_write[s] is not None else None for s in range(ns)], v_final, t_final


def written(v_write, is_write, v_read):
    """the word every operation leaves behind: v_write where it writes, what it read otherwise"""
    ns, n = len(v_read), len(v_read[0])
    return [[v_write[s][j] if writes(v_write, is_write, s, j) else v_read[s][j] for j in range(n)] for s in range(ns)]


def fingerprint(a, v, t, g, tau):
    return (t * g % R * g + v * g + a - tau) % R


def hashes(addr, v_init, v_read, t_read, w, v_final, t_final, g, tau):
    """(init, writes, reads, finals); the write fingerprint of every operation of step j carries j, the init fingerprint no time"""
    init = wr = rd = fin = 1
    for a in range(len(v_init)):
        init = init * fingerprint(a, v_init[a], 0, g, tau) % R
        fin = fin * fingerprint(a, v_final[a], t_final[a], g, tau) % R
    for s in range(len(addr)):
        for j in range(len(addr[s])):
            rd = rd * fingerprint(addr[s][j], v_read[s][j], t_read[s][j], g, tau) % R
            wr = wr * fingerprint(addr[s][j], w[s][j], j, g, tau) % R
    return init, wr, rd, fin


def multiset_equal(addr, v_write, is_write, v_init, v_read, t_read, v_final, t_final, g, tau):
    init, wr, rd, fin = hashes(addr, v_init, v_read, t_read, written(v_write, is_write, v_read), v_final, t_final, g, tau)
    return init * wr % R == rd * fin % R


def jolt_instance(seed, n, MEM, store_pct=30, n_regs=None):
    """a Jolt-shaped instance: slots rs1, rs2 (read), rd (writes every step), ram (writes where the store flag is set); the register
    indices below n_regs (default: all of the memory), the ram address anywhere in it -- so the slots alias freely"""
    rng = O.SplitMix64(seed)
    n_regs = min(MEM, n_regs or MEM)
    addr = [[rng.next() % n_regs for _ in range(n)] for _ in range(3)] + [[rng.next() % MEM for _ in range(n)]]
    v_write = [None, None, [rng.next() & 0xFFFFFFFF for _ in range(n)], [rng.next() & 0xFFFFFFFF for _ in range(n)]]
    is_write = [None, None, None, [1 if rng.next() % 100 < store_pct else 0 for _ in range(n)]]
    v_init = [rng.next() & 0xFFFFFFFF for _ in range(MEM)]
    return addr, v_write, is_write, v_init


def aliasing_instances():
    """the aliasing cases inside and across steps, as (name, addr, v_write, is_write, v_init)"""
    n, MEM = 40, 64
    out = []
    a, vw, iw, vi = jolt_instance(71, n, MEM)
    a[1], a[2] = list(a[0]), list(a[0])  # rs1 == rs2 == rd at every step
    out.append(("rs1_rs2_rd_equal", a, vw, iw, vi))
    a, vw, iw, vi = jolt_instance(72, n, MEM, store_pct=50)
    a[3] = [a[j % 3][j] for j in range(n)]  # the ram address is the index of rs1, rs2 or rd of the same step
    out.append(("ram_equals_a_register", a, vw, iw, vi))
    a, vw, iw, vi = jolt_instance(73, n, MEM)
    a[0] = [a[0][0]] + a[2][:-1]  # rd of step j is read back by rs1 of step j + 1
    out.append(("rd_read_back_next_step", a, vw, iw, vi))
    return out
