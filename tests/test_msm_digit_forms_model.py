"""The two digit forms of the MSM's small-scalar columns (csrc/msm.hip, for_each_digit), restated in Python integers.

plain:   16-bit signed digits with a carry: limb + carry > 32768 -> digit limb + carry - 65536, carry 1; NWIN = limbs + 1
         windows (the last one holds only the carry).
offset:  digit k = limb_k - 32768 for every limb; no carry window.  v = sum_k digit_k 2^(16k) + c with
         c = 32768 sum_k 2^(16k) over the limbs of the kind.
A column takes the offset form where it places strictly fewer references (non-zero digits) than the plain form."""
import random

import pytest

LIMBS = {"U16": 1, "U32": 2, "U64": 4}


def plain_digits(v, limbs):
    out, carry = [], 0
    for k in range(limbs + 1):
        d = ((v >> (16 * k)) & 0xFFFF) + carry
        carry = 1 if d > 32768 else 0
        out.append(d - 65536 if carry else d)
    assert carry == 0
    return out


def offset_digits(v, limbs):
    return [((v >> (16 * k)) & 0xFFFF) - 32768 for k in range(limbs)]


def offset_constant(limbs):
    return 32768 * sum(1 << (16 * k) for k in range(limbs))


def _values(kind):
    limbs = LIMBS[kind]
    bits = 16 * limbs
    rng = random.Random(1000 + limbs)
    edge = [0, 1, 32767, 32768, 32769, 65535, (1 << bits) - 1, 1 << (bits - 1)]
    # the same edge limb in every limb of the scalar
    edge += [sum(e << (16 * k) for k in range(limbs)) for e in (32767, 32768, 32769)]
    return [e & ((1 << bits) - 1) for e in edge] + [rng.getrandbits(bits) for _ in range(1000)]


def _brute_force_refs(v, limbs):
    """references of both forms from their definitions, not from the digit lists: plain = non-zero digits of the unique
    expansion v = sum d_k 65536^k with d_k in (-32768, 32768]; offset = limbs other than 32768"""
    plain, x = 0, v
    while x:
        d = x % 65536
        if d > 32768:
            d -= 65536
        plain += d != 0
        x = (x - d) // 65536
    offset = sum(((v >> (16 * k)) & 0xFFFF) != 32768 for k in range(limbs))
    return plain, offset


@pytest.mark.parametrize("kind", sorted(LIMBS))
def test_offset_digits_are_one_signed_window_each_and_rebuild_the_value(kind):
    limbs = LIMBS[kind]
    c = offset_constant(limbs)
    assert c == {1: 0x8000, 2: 0x80008000, 4: 0x8000800080008000}[limbs]
    for v in _values(kind):
        d = offset_digits(v, limbs)
        assert len(d) == limbs and all(-32768 <= x <= 32767 for x in d)
        assert sum(x << (16 * k) for k, x in enumerate(d)) + c == v
        p = plain_digits(v, limbs)
        assert all(-32767 <= x <= 32768 for x in p)
        assert sum(x << (16 * k) for k, x in enumerate(p)) == v


@pytest.mark.parametrize("kind", sorted(LIMBS))
def test_reference_counts_of_both_forms_match_brute_force(kind):
    limbs = LIMBS[kind]
    for v in _values(kind):
        got = (sum(x != 0 for x in plain_digits(v, limbs)), sum(x != 0 for x in offset_digits(v, limbs)))
        assert got == _brute_force_refs(v, limbs), hex(v)


@pytest.mark.parametrize("kind", sorted(LIMBS))
def test_choice_rule_on_whole_columns(kind):
    """offset only where strictly fewer references: zeros and small values stay plain, uniform values go offset"""
    limbs = LIMBS[kind]
    bits = 16 * limbs
    rng = random.Random(7)

    def choice(col):
        plain = sum(_brute_force_refs(v, limbs)[0] for v in col)
        offset = sum(_brute_force_refs(v, limbs)[1] for v in col)
        return "offset" if offset < plain else "plain"

    assert choice([0] * 100) == "plain"
    assert choice([rng.randrange(32768) for _ in range(1000)]) == "plain"
    assert choice([rng.getrandbits(bits) for _ in range(1000)]) == "offset"
    assert choice([offset_constant(limbs)] * 10) == "offset"  # every offset digit is zero
    assert choice([]) == "plain"  # a tie is plain
