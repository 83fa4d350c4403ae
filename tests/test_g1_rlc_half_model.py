"""CPU: the integer model of the G1 batch's level 0 on one 63-bit scalar half (msm_geom half0).

* the signed window digits of a 63-bit a (k_msm.hip signed_digit on half_scalar(s, 0, g)) give back a exactly and the
  top window never exceeds 2^(c-1), at the benchmark's geometry (c = 16, 4 windows) and at a small one (c = 5, 13
  windows): a = 0, 2^63 - 1, values whose windows all carry, values that put exactly 2^(c-1) in the top window;
* the digits of a alone are rows 0 .. nwin - 1 of the split form of tests/test_g1_iso_late_model.py (each half recoded
  on its own), whatever b is: the one-half level 0 keys the same rows the batched subgroup test reads;
* on a toy group of prime order q > 2^8 with 8-bit halves, the level-0 sum taken through the recoding's buckets and the
  window Horner is sum a_i P_i; the one-half check accepts a valid set, and with one wrong element j it rejects for
  every value of a_j but at most one (all 2^8 enumerated, for every position of j and several wrong elements)."""
import random

import pytest

import test_g1_iso_late_model as SPLIT

SBITS = 63
GEOMS = ((16, 4), (5, 13))  # (c, nwin): the batch-sized geometry, and a small one with enough windows for 63 bits


def nwin_for(sbits, c):
    """drandhip.cpp geom_for: windows for scalars of sbits bits, one spare bit for the top window."""
    return (sbits + 1 + c - 1) // c


def signed_digits(k, c, nwin):
    """k_msm.hip signed_digit over nwin windows of c bits: the top window is not mapped."""
    out, carry = [], 0
    for w in range(nwin):
        v = ((k >> (w * c)) & ((1 << c) - 1)) + carry
        if w + 1 < nwin and v >= 1 << (c - 1):
            carry, d = 1, v - (1 << c)
        else:
            carry, d = 0, v
        out.append(d)
    return out


def value(digits, c):
    return sum(d << (c * w) for w, d in enumerate(digits))


def edge_values(c, nwin):
    half, full = 1 << (c - 1), (1 << c) - 1
    tbits = SBITS - c * (nwin - 1)  # bits of a in the top window
    top = ((1 << tbits) - 1) << (c * (nwin - 1))
    every = lambda d: sum(d << (c * w) for w in range(nwin - 1))  # noqa: E731
    return [0, 1, (1 << SBITS) - 1,
            every(half), every(full), top | every(half), top | every(full),  # every window below the top carries
            top | (half << (c * (nwin - 2))), top | ((1 << (c * (nwin - 1))) - 1),  # the top window reaches 2^tbits
            every(half - 1), every(half) - 1, 1 << (SBITS - 1)]


@pytest.mark.parametrize("c,nwin", GEOMS)
def test_digits_of_a_63_bit_half_give_it_back(c, nwin):
    assert nwin == nwin_for(SBITS, c) and nwin * c >= SBITS + 1
    half = 1 << (c - 1)
    rng = random.Random(2401 + c)
    vals = edge_values(c, nwin) + [rng.randrange(1 << SBITS) for _ in range(300)]
    tops = set()
    for a in vals:
        assert 0 <= a < 1 << SBITS
        d = signed_digits(a, c, nwin)
        assert value(d, c) == a
        assert all(-half <= x < half for x in d[:-1])
        assert 0 <= d[-1] <= half  # the top window keeps its carry: at most 2^(c-1), bucket indices reach nbuck - 1
        tops.add(d[-1])
    tbits = SBITS - c * (nwin - 1)
    assert 1 << tbits in tops and 0 in tops  # the carry into a full top window was met
    if tbits == c - 1:
        assert half in tops
    all_carry = signed_digits((1 << SBITS) - 1, c, nwin)
    assert all_carry[0] == -1 and all(x == 0 for x in all_carry[1:-1]) and all_carry[-1] == 1 << tbits


@pytest.mark.parametrize("c,nwin", GEOMS)
def test_a_only_digits_are_the_first_rows_of_the_split_form(monkeypatch, c, nwin):
    monkeypatch.setattr(SPLIT, "C", c)  # the split form's window width (its own tests run at 16)
    rng = random.Random(2402 + c)
    vals = edge_values(c, nwin) + [rng.randrange(1 << SBITS) for _ in range(100)]
    for a in vals:
        for b in (0, (1 << SBITS) - 1, rng.randrange(1 << SBITS)):
            rows = SPLIT.signed_digits(a, nwin) + SPLIT.signed_digits(b, nwin)  # rows 0..nwin-1: a, nwin..2nwin-1: b
            assert len(rows) == 2 * nwin
            assert signed_digits(a, c, nwin) == rows[:nwin]
            assert SPLIT.value(rows[:nwin]) == a and SPLIT.value(rows[nwin:]) == b


# ---------------------------------------------------------------- the one-half check on a toy prime-order group
Q = 257  # the group Z_q, prime order q > 2^8: the stand-in for G1 of order r > 2^63 under 8-bit halves
HB, TC = 8, 3
TNWIN = nwin_for(HB, TC)


def msm_level0(points, scalars):
    """The level-0 sum as the kernels take it: buckets by |digit| with the sign on the point, row sums, Horner."""
    nbuck = (1 << (TC - 1)) + 1
    rows = []
    for w in range(TNWIN):
        bucket = [0] * nbuck
        for p, a in zip(points, scalars):
            d = signed_digits(a, TC, TNWIN)[w]
            if d:
                bucket[abs(d)] = (bucket[abs(d)] + (p if d > 0 else -p)) % Q
        rows.append(sum(k * bucket[k] for k in range(1, nbuck)) % Q)
    acc = rows[-1]
    for w in range(TNWIN - 2, -1, -1):
        acc = (acc * (1 << TC) + rows[w]) % Q
    return acc


def accepts(sk, hashes, sigs, a):
    """sum a_i sigma_i == [sk] sum a_i H_i: the pairing equation of the level-0 check, in Z_q."""
    return msm_level0(sigs, a) == sk * msm_level0(hashes, a) % Q


def test_toy_group_one_half_check():
    assert TNWIN * TC >= HB + 1 and Q > 1 << HB
    rng = random.Random(2403)
    n, sk = 6, 101
    hashes = [rng.randrange(1, Q) for _ in range(n)]
    hashes[4] = hashes[1]  # one message twice
    sigs = [sk * h % Q for h in hashes]
    for _ in range(50):
        a = [rng.randrange(1 << HB) for _ in range(n)]
        assert msm_level0(sigs, a) == sum(x * s for x, s in zip(a, sigs)) % Q
        assert accepts(sk, hashes, sigs, a)
    for j in range(n):
        for delta in (1, 2, 128, Q - 1, rng.randrange(1, Q)):  # D_j = sigma_j - [sk] H_j != 0
            bad = list(sigs)
            bad[j] = (sigs[j] + delta) % Q
            for _ in range(4):
                a = [rng.randrange(1 << HB) for _ in range(n)]
                passing = []
                for aj in range(1 << HB):
                    a[j] = aj
                    if accepts(sk, hashes, bad, a):
                        passing.append(aj)
                # sum a_i D_i = a_j D_j with D_j of order q > 2^8: zero for a_j = 0 alone
                assert passing == [0]
    # two wrong elements: fix every scalar but a_j, at most one a_j passes (it need not be 0)
    bad = list(sigs)
    bad[0], bad[3] = (sigs[0] + 5) % Q, (sigs[3] + 77) % Q
    most = 0
    for _ in range(20):
        a = [rng.randrange(1 << HB) for _ in range(n)]
        cnt = 0
        for aj in range(1 << HB):
            a[3] = aj
            cnt += accepts(sk, hashes, bad, a)
        assert cnt <= 1
        most = max(most, cnt)
    assert most == 1
