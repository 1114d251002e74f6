"""Big-int expected values of cozk_rw_memory_shared_leaves and cozk_rw_memory_shared_init_final_leaves (csrc/rw_memory_leaves.hip): the
leaves of the read-write memory check with the values as polynomials, after Rep3ReadWriteMemoryProver::compute_leaves -- every leaf is
add_public(mul_public(v_share, gamma), t gamma^2 + a - tau, party_id).

A value column is a list of ints (a PLAIN polynomial: the value itself in a plain call, a public polynomial in a rep3 call) or a list of
(a, b) pairs (this party's Rep3 share components).  With pub = a + t gamma^2 - tau, plus gamma v for a public polynomial:
    plain:  out_a = h(a, v, t)
    rep3:   out_a = gamma v_a + [party == 0] pub,   out_b = gamma v_b + [party == 1] pub
as `_expect_shares` of tests/test_gpu_bytecode_leaves.py has it for the bytecode.  The fingerprint h is rw_proof_ref's."""
import rw_proof_ref as P

R = P.R


def is_shared(col):
    return len(col) > 0 and isinstance(col[0], tuple)


def split(col):
    """-> (the public values, the a components, the b components), zeros where the column has none"""
    n = len(col)
    if is_shared(col):
        return [0] * n, [x[0] for x in col], [x[1] for x in col]
    return list(col), [0] * n, [0] * n


def expect_shares(pub, va, vb, g, party):
    """add_public on gamma times the share components: party 0's a and party 1's b carry the public part"""
    a = [(g * x + (p if party == 0 else 0)) % R for x, p in zip(va, pub)]
    b = [(g * x + (p if party == 1 else 0)) % R for x, p in zip(vb, pub)]
    return a, b


def _leaf(addr, v, t, g, tau, mode, party):
    """one circuit: addr and t int lists (t None: the step number), v a value column -> (out_a, out_b | None)"""
    n = len(addr)
    t = list(range(n)) if t is None else t
    if mode == "plain":
        assert not is_shared(v)
        return [P.h(addr[j], v[j], t[j], g, tau) for j in range(n)], None
    vp, va, vb = split(v[:n])
    pub = [P.h(addr[j], vp[j], t[j], g, tau) for j in range(n)]
    return expect_shares(pub, va, vb, g, party)


def _flat(circuits, mode):
    a = [x for c in circuits for x in c[0]]
    return a, (None if mode == "plain" else [x for c in circuits for x in c[1]])


def rw_shared_leaves(addr, v_read, t_read, v_written, g, tau, mode="plain", party=0):
    """the 2 n_slots circuits, circuit-major and flattened: (out_a, out_b | None); v_written[s] None: the slot only reads"""
    circuits = []
    for s in range(len(addr)):
        w = v_written[s] if v_written is not None and v_written[s] is not None else v_read[s]
        circuits.append(_leaf(addr[s], v_read[s], t_read[s], g, tau, mode, party))
        circuits.append(_leaf(addr[s], w, None, g, tau, mode, party))
    return _flat(circuits, mode)


def if_shared_leaves(v_init, v_final, t_final, g, tau, mode="plain", party=0):
    """init = h(a, v_init, 0), final = h(a, v_final, t_final) over MEM = len(t_final) addresses, flattened: (out_a, out_b | None)"""
    MEM = len(t_final)
    iota = list(range(MEM))
    return _flat([_leaf(iota, v_init, [0] * MEM, g, tau, mode, party), _leaf(iota, v_final, t_final, g, tau, mode, party)], mode)
