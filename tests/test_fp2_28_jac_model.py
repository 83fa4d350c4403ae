"""CPU: the bound-checked integer model of the Jacobian-input G2 subgroup test (tests/fp2_28_jac_model.py, mirroring
drand_amd/csrc/fp2_28.hpp g2_jac_in_subgroup28) against the oracle's affine arithmetic: [r] T == O.

Every point enters in Jacobian form with a random Z and with its coordinates pushed to the top of the bounds a stored
bucket sum may have (X in [p, 2p), Y in [2p, 3p), Z in [11p, 12p) per component), so the formulas' product and sum bounds are
exercised where they are tightest. psi in Python is (conj(x) cx, conj(y) cy) with cx = (1 + i)^-((p-1)/3) and
cy = (1 + i)^-((p-1)/2); the first test checks that it satisfies X^2 - (u + 1) X + p on the curve and equals [u] on G2.
"""
import random

import pytest

import bls_py as B
import fp28_model as M1
import fp2_28_model as M
import fp2_28_jac_model as J

P, R = M.p, M1.r
U = -M1.U  # the BLS parameter (negative)
H2 = (U ** 8 - 4 * U ** 7 + 5 * U ** 6 - 4 * U ** 4 + 6 * U ** 3 - 4 * U ** 2 - 4 * U + 13) // 9


def psi(pt):
    if pt is None:
        return None
    cx, cy = M._psi_consts()
    return (B.f2mul(B.f2conj(pt[0]), cx), B.f2mul(B.f2conj(pt[1]), cy))


def curve_point(rng):
    while True:
        x = (rng.randrange(P), rng.randrange(P))
        y = B.f2sqrt(B.f2add(B.f2mul(B.f2mul(x, x), x), B.B2))
        if y is not None:
            return (x, y)


def g2_point(rng):
    return B.ec_mul(B.FP2, B.G2_GEN, rng.randrange(1, R))


def top(v, k):
    """v + m p inside [(k - 1) p, k p): the same residue at the top of the bound k p"""
    v %= P
    return v + (k - 1) * P


def jac_top(pt, rng):
    """pt as (X, Y, Z) with a random Z, every component at the top of the stored sums' bounds (2, 3, 12)"""
    z = (rng.randrange(1, P), rng.randrange(1, P))
    z2 = B.f2mul(z, z)
    X, Y, Z = M.from_f2(B.f2mul(pt[0], z2)), M.from_f2(B.f2mul(pt[1], B.f2mul(z2, z))), M.from_f2(z)
    return (tuple(top(c, 2) for c in X), tuple(top(c, 3) for c in Y), tuple(top(c, 12) for c in Z), False)


@pytest.fixture(scope="module")
def torsion13():
    """S of order 13 in E'(Fp2)[13] = Z_13^2 and the two psi eigenvectors (psi - 7) S (psi = 11 = -2 on it) and
    (psi - 11) S (psi = 7 = 1/2)."""
    assert H2 % 169 == 0 and (H2 // 169) % 13 != 0
    rng = random.Random(41)
    while True:
        S = B.ec_mul(B.FP2, curve_point(rng), R * H2 // 169)
        if S is None:
            continue
        if B.ec_mul(B.FP2, S, 13) is not None:
            S = B.ec_mul(B.FP2, S, 13)
        a = B.ec_add(B.FP2, psi(S), B.ec_neg(B.FP2, B.ec_mul(B.FP2, S, 7)))
        b = B.ec_add(B.FP2, psi(S), B.ec_neg(B.FP2, B.ec_mul(B.FP2, S, 11)))
        if a is not None and b is not None:
            return S, a, b


def test_python_psi_is_the_endomorphism(torsion13):
    rng = random.Random(2)
    q = curve_point(rng)
    assert B.g2_on_curve(psi(q))
    # psi^2 - (u + 1) psi + p = 0 on all of E'(Fp2)
    lhs = B.ec_add(B.FP2, psi(psi(q)), B.ec_mul(B.FP2, q, P))
    assert lhs == B.ec_mul(B.FP2, psi(q), (U + 1) % (R * H2))
    g = g2_point(rng)
    assert psi(g) == B.ec_mul(B.FP2, g, U % R)
    _, a, b = torsion13
    assert B.ec_mul(B.FP2, a, 13) is None and psi(a) == B.ec_mul(B.FP2, a, 11)
    assert B.ec_mul(B.FP2, b, 13) is None and psi(b) == B.ec_mul(B.FP2, b, 7)


def test_jacobian_subgroup_test_model(torsion13):
    rng = random.Random(13)
    _, t13a, t13b = torsion13
    sub = [g2_point(rng) for _ in range(3)]
    tors = B.ec_mul(B.FP2, curve_point(rng), R)  # a point of E'(Fp2)[h2]
    cases = [(pt, True) for pt in sub]
    cases += [(curve_point(rng), False) for _ in range(2)]
    cases += [(B.ec_add(B.FP2, sub[0], tors), False), (B.ec_add(B.FP2, sub[1], t13a), False),
              (B.ec_add(B.FP2, sub[2], t13b), False), (tors, False)]
    stats = {}
    for pt, want in cases:
        assert (B.ec_mul(B.FP2, pt, R) is None) == want
        for _ in range(2):  # two random Z each
            assert J.jac_in_subgroup(jac_top(pt, rng), stats) == want
    assert stats == {}  # no exceptional case on points of large order


def test_identity_passes():
    assert J.jac_in_subgroup(M.inf()) is True


@pytest.mark.parametrize("which", ["a", "b"])
def test_order_13_eigenvector(torsion13, which):
    """The chain of [|u|] T runs through multiples of T mod 13, and some prefix of |u| is 0 or +-1 mod 13 right before
    an addition of T: the fast additions poison Z and the exact chain decides. T is outside G2."""
    rng = random.Random(17)
    t = torsion13[1] if which == "a" else torsion13[2]
    stats = {}
    for k in (1, 5):
        assert J.jac_in_subgroup(jac_top(B.ec_mul(B.FP2, t, k), rng), stats) is False
    assert stats.get("exact", 0) >= 1
