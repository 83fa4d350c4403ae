"""Soundness model of the batched G2 subgroup test, on the torsion alone.

E'(Fp2) = G2 + E'(Fp2)[h2] with h2 = 13^2 * 23^2 * 2713 * 11953 * 262069 * (a 448-bit prime). An eligible G2 batch
draws two 63-bit halves k1, k2 per round (the scalar k1 + k2 u, psi = [u] on G2); half 0 adds +-sigma and half 1
+-psi(sigma) to bucket |digit| of window row w, and the test passes only when every bit-subset sum T[w][b] has a zero
component in E'(Fp2)[h2]. The digit model (signed digits, 8-bit halves, c = 4) is test_subgroup_batch_model's; the
curve is replaced by the torsion groups h2 offers, with psi acting as it does there (a root of X^2 - (u + 1) X + p,
or the companion matrix where there is no root):
  Z_13 with psi = 11 (= -2) and with psi = 7 (= 1/2): exactly the small ratios the G1 proof's second half excludes;
  Z_13^2 with t = (1, 1), psi = diag(11, 7);
  Z_23^2 with the companion matrix (no eigenvalue mod 23);
  Z_2713 with psi = 119.
All 65,536 (k1, k2) of one bad round are enumerated with the other rounds fixed: at most one k1 passes per k2, the
2^-63 bound of the claim. The last tests state why the four 31-bit psi parts were not kept.
"""
import itertools

import numpy as np
import pytest

from test_subgroup_batch_model import HONEST, SBITS, other_rounds, passing_pairs

P = 0x1a0111ea397fe69a4b1ba7b6434bacd764774b84f38512bf6730d2a0f6b0f6241eabfffeb153ffffb9feffffffffaaab
U = -0xd201000000010000
R = U ** 4 - U ** 2 + 1
H2 = (U ** 8 - 4 * U ** 7 + 5 * U ** 6 - 4 * U ** 4 + 6 * U ** 3 - 4 * U ** 2 - 4 * U + 13) // 9
TRACE = U + 1  # psi^2 - TRACE psi + p = 0 on E'(Fp2)


def eigenvalues(q):
    return sorted(x for x in range(q) if (x * x - TRACE * x + P) % q == 0)


def companion(q):
    """psi on Z_q^2 in the basis (t, psi t): psi^2 = TRACE psi - p"""
    return np.array([[0, -P % q], [1, TRACE % q]], dtype=np.int64)


def torsion_cases():
    c23 = companion(23)
    t23 = np.array([1, 0])
    return {"13_psi11": (13, np.array([1]), np.array([11])),
            "13_psi7": (13, np.array([1]), np.array([7])),
            "13x13": (13, np.array([1, 1]), np.array([11, 7])),
            "23x23": (23, t23, c23 @ t23 % 23),
            "2713": (2713, np.array([1]), np.array([119]))}


CASES = sorted(torsion_cases())


def test_cofactor_and_eigenvalue_table():
    small = 13 ** 2 * 23 ** 2 * 2713 * 11953 * 262069
    assert H2 % small == 0 and H2 % 2 == 1
    big = H2 // small
    assert big.bit_length() == 448 and pow(2, big - 1, big) == 1
    assert all(big % q for q in (13, 23, 2713, 11953, 262069))
    assert P % R == U % R  # psi = [u] on G2
    assert eigenvalues(13) == [7, 11] and eigenvalues(23) == []
    assert (11 + 2) % 13 == 0 and (2 * 7 - 1) % 13 == 0  # psi = -2 and psi = 1/2 on the two order-13 eigenvectors
    assert 119 in eigenvalues(2713)
    # no other prime factor of h2 has an eigenvalue in {+-1, +-2, +-1/2}
    for q in (2713, 11953, 262069, big):
        for lam in (1, -1, 2, -2):
            assert (lam * lam - TRACE * lam + P) % q != 0
            assert (1 - TRACE * lam + P * lam * lam) % q != 0  # 1 / lam


@pytest.mark.parametrize("case", CASES)
def test_one_bad_round(case):
    q, t, pt = torsion_cases()[case]
    n_pass, ok = passing_pairs(q, t, pt, other_rounds(q, t, pt, HONEST))
    assert ok.sum(axis=0).max() <= 1  # at most one k1 per k2
    assert n_pass <= 1 << SBITS


@pytest.mark.parametrize("case", CASES)
def test_opposite_torsion_in_two_rounds(case):
    """Round A carries -t with fixed scalars, round B carries +t: B's scalars equal to A's cancel it in every bucket,
    and no second k1 does for any k2."""
    q, t, pt = torsion_cases()[case]
    n_pass, ok = passing_pairs(q, t, pt, other_rounds(q, t, pt, HONEST + [(0x9d, 0x36, -1)]))
    assert ok.sum(axis=0).max() <= 1
    assert n_pass <= 1 << SBITS
    assert ok[0x9d, 0x36]


def test_four_parts_do_not_pin_the_scalars():
    """Why four 31-bit parts were not kept. On an order-13 eigenvector with psi t = -2 t one test sees
    (a1 + a2 psi + a3 psi^2 + a4 psi^3) t = (a1 - 2 a2 + 4 a3 - 8 a4) t with each a in {-1, 0, 1} (a part's bit x
    sign): every residue mod 13 has several preimages, so the tests do not read the four parts off jointly; fixing
    three of them pins the fourth only, a 2^-31 bound."""
    counts = np.zeros(13, np.int64)
    for a in itertools.product((-1, 0, 1), repeat=4):
        counts[(a[0] - 2 * a[1] + 4 * a[2] - 8 * a[3]) % 13] += 1
    assert counts.sum() == 81
    assert counts.min() >= 5 and counts.max() <= 7
    assert (counts > 1).all()
