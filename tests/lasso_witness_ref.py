"""The dealer's Lasso lookup witness as plain sequential Python (co-jolt/src/jolt/vm/instruction_lookups/witness.rs:85-150):
for one memory with addresses addr[0..n), 0/1 flags and a subtable of M entries

  read_cts[j]  = #{ j' < j : flag[j'] = 1 and addr[j'] = addr[j] }  if flag[j] = 1, else 0
  final_cts[a] = #{ j : flag[j] = 1 and addr[j] = a }
  E[j]         = subtable[addr[j]]                                   if flag[j] = 1, else 0

and the offline-memory-checking hashes over Fr that make those counters a witness: h(a, v, t) = t g^2 + v g + a - tau."""
import pyref as O

R = O.R


def witness(addr, flag, subtable):
    """flag None: used at every step.  Returns (read_cts, E, final_cts) as lists of ints."""
    n, M = len(addr), len(subtable)
    final = [0] * M
    read, E = [0] * n, [0] * n
    for j in range(n):
        if flag is not None and not flag[j]:
            continue
        a = addr[j]
        if a >= M:
            raise ValueError("memory step %d: flagged address %d >= M = %d" % (j, a, M))
        read[j] = final[a]
        final[a] += 1
        E[j] = subtable[a]
    return read, E, final


def witness_batch(dims, subtables, flags, mem_dim, mem_subtable):
    out = [witness(dims[d], f, subtables[s]) for d, s, f in zip(mem_dim, mem_subtable, flags)]
    return [o[0] for o in out], [o[1] for o in out], [o[2] for o in out]


def fingerprint(a, v, t, g, tau):
    return (t * g % R * g + v * g + a - tau) % R


def hashes(addr, flag, subtable, read, E, final, g, tau):
    """(init, writes, reads, finals): the four products of the memory checking of one memory; reads / writes over the flagged
    steps only (the toggled grand product), init / final over every address"""
    init = writes = reads = finals = 1
    for a in range(len(subtable)):
        init = init * fingerprint(a, subtable[a], 0, g, tau) % R
        finals = finals * fingerprint(a, subtable[a], final[a], g, tau) % R
    for j in range(len(addr)):
        if flag is not None and not flag[j]:
            continue
        reads = reads * fingerprint(addr[j], E[j], read[j], g, tau) % R
        writes = writes * fingerprint(addr[j], E[j], read[j] + 1, g, tau) % R
    return init, writes, reads, finals


def multiset_equal(addr, flag, subtable, read, E, final, g, tau):
    init, writes, reads, finals = hashes(addr, flag, subtable, read, E, final, g, tau)
    return init * writes % R == reads * finals % R
