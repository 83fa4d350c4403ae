"""Soundness model of the batched G1 subgroup test, on the torsion alone.

E(Fp) = G1 + E(Fp)[h]; a decoded signature outside G1 has a nonzero component t in E(Fp)[h], and the batched test
passes only when every bit-subset sum T[w][b] of the level-0 sigma buckets has a zero component there. The model
restates the kernel's signed window digits (k_msm.hip signed_digit) and the two halves' sharing of the window rows
(half 0 adds +-sigma, half 1 +-phi(sigma) to bucket |digit| of row w), shrinks the halves to 8 bits with c = 4, and
replaces the curve by the torsion groups the cofactor h = 3 * 11^2 * 10177^2 * ... offers:
  order 3:      Z_3 with phi = 1 (the only component phi fixes: the bound there is one k1 per k2);
  order 11:     Z_11^2 with phi = [[0, -1], [1, -1]] (11 = 2 mod 3: no eigenvalue, phi^2 + phi + 1 = 0);
  order 10177:  Z_10177 with phi = lambda, a root of lambda^2 + lambda + 1.
All 65,536 (k1, k2) of one bad round are enumerated, the other rounds' scalars fixed.
"""
import numpy as np
import pytest

SBITS, C = 8, 4
NWIN = (SBITS + 1 + C - 1) // C  # geom_for: one spare bit above the scalar


def signed_digits(k):
    """k_msm.hip signed_digit over the windows of one half: digits in [-2^(c-1), 2^(c-1)), the top one unmapped."""
    out, carry = [], 0
    for w in range(NWIN):
        v = ((k >> (w * C)) & ((1 << C) - 1)) + carry
        if w + 1 < NWIN and v >= 1 << (C - 1):
            carry, d = 1, v - (1 << C)
        else:
            carry, d = 0, v
        out.append(d)
    return out


def coeffs():
    """A[k, w, b] = sign(d_w) * bit_b(|d_w|): what half value k adds to T[w][b], in units of its point."""
    a = np.zeros((1 << SBITS, NWIN, C), np.int64)
    for k in range(1 << SBITS):
        for w, d in enumerate(signed_digits(k)):
            for b in range(C):
                if (abs(d) >> b) & 1:
                    a[k, w, b] = 1 if d > 0 else -1
    return a


A = coeffs()


def test_recoding_is_injective_and_exact():
    seen = set()
    for k in range(1 << SBITS):
        d = signed_digits(k)
        assert sum(x << (C * w) for w, x in enumerate(d)) == k
        assert all(-(1 << (C - 1)) <= x <= (1 << (C - 1)) for x in d)
        seen.add(tuple(d))
    assert len(seen) == 1 << SBITS


def lam_root(q):
    return next(x for x in range(2, q) if (x * x + x + 1) % q == 0)


# (order, t, phi(t)) as integer vectors mod q
def torsion_cases():
    lam = lam_root(10177)
    phi11 = np.array([[0, -1], [1, -1]])
    t11 = np.array([1, 0])
    return {3: (3, np.array([1]), np.array([1])),
            11: (11, t11, phi11 @ t11 % 11),
            10177: (10177, np.array([1]), np.array([lam]))}


def passing_pairs(q, t, pt, fixed):
    """Number of (k1, k2) of the bad round (torsion t, phi(t) = pt) for which every T[w][b] vanishes mod q, given the
    other rounds' total contribution fixed[w, b, component]."""
    # T[k1, k2, w, b, comp] = A[k1] t + A[k2] phi(t) + fixed
    T = (A[:, None, :, :, None] * t + A[None, :, :, :, None] * pt + fixed[None, None]) % q
    ok = (T == 0).all(axis=(2, 3, 4))
    return int(ok.sum()), ok


def other_rounds(q, t, pt, scal):
    """Contribution of rounds with fixed scalars (k1, k2) carrying m x the torsion (m = 0: an honest round)."""
    f = np.zeros((NWIN, C, len(t)), np.int64)
    for k1, k2, m in scal:
        f += m * (A[k1][:, :, None] * t + A[k2][:, :, None] * pt)
    return f % q


HONEST = [(0x5a, 0xc3, 0), (0x17, 0xee, 0), (0xff, 0x01, 0)]


@pytest.mark.parametrize("order", [3, 11, 10177])
def test_one_bad_round(order):
    q, t, pt = torsion_cases()[order]
    n_pass, ok = passing_pairs(q, t, pt, other_rounds(q, t, pt, HONEST))
    if order == 3:
        assert n_pass <= 1 << SBITS
        assert ok.sum(axis=0).max() <= 1  # at most one k1 per k2
    else:
        assert n_pass <= 1


@pytest.mark.parametrize("order", [3, 11, 10177])
def test_opposite_torsion_in_two_rounds(order):
    """Round A carries -t with fixed scalars, round B carries +t: only B's scalars equal to A's can cancel it."""
    q, t, pt = torsion_cases()[order]
    n_pass, ok = passing_pairs(q, t, pt, other_rounds(q, t, pt, HONEST + [(0x9d, 0x36, -1)]))
    if order == 3:
        assert n_pass <= 1 << SBITS
        assert ok.sum(axis=0).max() <= 1
    else:
        assert n_pass <= 1
        assert ok[0x9d, 0x36]  # the one pair: B's scalars equal A's, the two rounds cancel in every bucket


def test_bare_sum_would_be_unsound_on_3_torsion():
    """Why subset bits and not the one sum of r_i sigma_i: against order 3 (phi = 1) the bare test k1 + k2 = 0 mod 3
    passes for a third of the scalars."""
    k = np.arange(1 << SBITS)
    frac = ((k[:, None] + k[None, :]) % 3 == 0).mean()
    assert 0.3 < frac < 0.36
