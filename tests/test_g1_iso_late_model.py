"""CPU: the integer model of the G1 batch that leaves the hash's 11-isogeny to the MSM.

* the identity the deferral rests on: for SSWU sums S_i on E1' and 63-bit halves a_i, b_i,
  iso(sum a_i S_i) + phi(iso(sum b_i S_i)) and sum (a_i + mu b_i) iso(S_i) agree once the cofactor is cleared (phi is
  [mu] on G1 only; the batch check clears the cofactor of the hash sum), with phi(x, y) = (beta x, y) for the beta the
  MSM multiplies by (k_msm.hip BETA28) and mu = -z^2 (k_prep.hip k_scalars): this pins beta against mu;
* doubling on E1' with the curve's own A' agrees with the group law (a point added to itself through a third point),
  for the Jacobian formula of fp28.hpp j28_dbl_a and for the affine one of h2c.hpp e1p_dbl_aff, and E1's a = 0
  doubling does not;
* the two halves of a scalar recoded separately (k_msm.hip half_scalar / signed_digit, msm_geom split) reproduce a and
  b when a's top window is exactly 2^(c-1); the signed recoding of the 128-bit concatenation carries a unit from a
  into b instead;
* the per-round product counts of the new form: 6 + 6 + 6 around and after the chain, no isogeny, and 4 conversions
  (sigma and the hash point into the 28-bit form), 22 against 54."""
import os
import random
import re

import bls_py as B
import g1_ride_model as M

p = M.p
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MU = (-B.U_ABS * B.U_ABS) % B.R  # phi = [mu] on G1: mu = -z^2
C, SBITS = 16, 63
NWIN = (SBITS + 1 + C - 1) // C


def beta_of_the_msm():
    src = open(os.path.join(ROOT, "drand_amd", "csrc", "k_msm.hip")).read()
    body = re.search(r"BETA28\[14\] = \{([^}]*)\}", src).group(1)
    limbs = [int(t.strip().rstrip("u"), 16) for t in body.split(",")]
    assert len(limbs) == 14 and all(v < 1 << 28 for v in limbs)
    return sum(v << (28 * i) for i, v in enumerate(limbs)) * pow(1 << 392, -1, p) % p


def e1p_a_of_the_msm():
    src = open(os.path.join(ROOT, "drand_amd", "csrc", "fp28.hpp")).read()
    body = re.search(r"f28_e1p_a\(\) \{\s*const uint32_t k\[14\] = \{([^}]*)\}", src).group(1)
    limbs = [int(t.strip().rstrip("u"), 16) for t in body.split(",")]
    return sum(v << (28 * i) for i, v in enumerate(limbs)) * pow(1 << 392, -1, p) % p


def on_e1p(pt):
    x, y = pt
    return (y * y - (x * x * x + B.A1P * x + B.B1P)) % p == 0


def sswu_sum(u0, u1):
    return B.ec_add(B.FP, B.sswu_g1(u0), B.sswu_g1(u1), B.A1P)


def clear(pt):
    return B.ec_mul(B.FP, pt, B.H_EFF_G1)


def test_isogeny_once_per_half_sum_equals_the_per_round_isogenies():
    beta = beta_of_the_msm()
    assert beta != 1 and pow(beta, 3, p) == 1
    phi = lambda pt: None if pt is None else (beta * pt[0] % p, pt[1])  # noqa: E731
    rng = random.Random(2101)
    S = [sswu_sum(rng.randrange(p), rng.randrange(p)) for _ in range(24)]
    S[5] = S[4]  # two rounds with one message
    assert all(on_e1p(s) for s in S)
    a = [rng.randrange(1 << 63) for _ in S]
    b = [rng.randrange(1 << 63) for _ in S]
    sum_a = sum_b = want = None
    for s, ai, bi in zip(S, a, b):
        sum_a = B.ec_add(B.FP, sum_a, B.ec_mul(B.FP, s, ai, B.A1P), B.A1P)
        sum_b = B.ec_add(B.FP, sum_b, B.ec_mul(B.FP, s, bi, B.A1P), B.A1P)
        want = B.ec_add(B.FP, want, B.ec_mul(B.FP, clear(B.iso_map_g1(s)), (ai + MU * bi) % B.R))
    got = clear(B.ec_add(B.FP, B.iso_map_g1(sum_a), phi(B.iso_map_g1(sum_b))))
    assert got is not None and got == want
    # the other cube root of unity is the other eigenvalue: the test tells them apart
    phi2 = lambda pt: (beta * beta % p * pt[0] % p, pt[1])  # noqa: E731
    assert clear(B.ec_add(B.FP, B.iso_map_g1(sum_a), phi2(B.iso_map_g1(sum_b)))) != want


def j28_dbl_a(P3, a):
    """fp28.hpp j28_dbl_a on integers: dbl-2009-l with E = 3 X^2 + a Z^4."""
    X, Y, Z = P3
    A_, B_ = X * X % p, Y * Y % p
    C_ = B_ * B_ % p
    D = 2 * ((X + B_) ** 2 - A_ - C_) % p
    E = (3 * A_ + a * pow(Z, 4, p)) % p
    X3 = (E * E - 2 * D) % p
    return X3, (E * (D - X3) - 8 * C_) % p, 2 * Y * Z % p


def e1p_dbl_aff(xn, xd, y, a):
    """h2c.hpp e1p_dbl_aff on integers."""
    xd2, y2 = xd * xd % p, 2 * y % p
    ic = pow(y2 * xd2 % p, -1, p)
    lam = (3 * xn * xn + a * xd2) % p * ic % p
    x = xn * (y2 * xd % p * ic % p) % p
    x3 = (lam * lam - 2 * x) % p
    return x3, (lam * (x - x3) - y) % p


def test_doubling_on_e1p_agrees_with_the_group_law():
    a = e1p_a_of_the_msm()
    assert a == B.A1P
    rng = random.Random(2102)
    for _ in range(16):
        P_ = sswu_sum(rng.randrange(p), rng.randrange(p))
        T = sswu_sum(rng.randrange(p), rng.randrange(p))
        # 2P without a doubling: (P + T) + (P - T), additions of distinct points only
        want = B.ec_add(B.FP, B.ec_add(B.FP, P_, T), B.ec_add(B.FP, P_, B.ec_neg(B.FP, T)))
        assert on_e1p(want)
        z = rng.randrange(1, p)
        jac = (P_[0] * z * z % p, P_[1] * pow(z, 3, p) % p, z)
        assert M.jac_affine(j28_dbl_a(jac, a)) == want
        assert M.jac_affine(j28_dbl_a(jac, 0)) != want  # E1's doubling is another curve's
        xd = rng.randrange(1, p)
        assert e1p_dbl_aff(P_[0] * xd % p, xd, P_[1], a) == want
        assert B.ec_dbl(B.FP, P_, B.A1P) == want


def signed_digits(k, nwin):
    """k_msm.hip signed_digit over nwin windows of c bits: the top window is not mapped."""
    out, carry = [], 0
    for w in range(nwin):
        v = ((k >> (w * C)) & ((1 << C) - 1)) + carry
        if w + 1 < nwin and v >= 1 << (C - 1):
            carry, d = 1, v - (1 << C)
        else:
            carry, d = 0, v
        out.append(d)
    return out


def value(digits):
    return sum(d << (C * w) for w, d in enumerate(digits))


def test_halves_are_recoded_separately():
    rng = random.Random(2103)
    half = 1 << (C - 1)
    # a < 2^63: its top window holds at most 2^(c-1) - 1, and reaches 2^(c-1) exactly by the carry of the window below
    top = (half - 1) << (C * (NWIN - 1))
    cases = [(top | (half << (C * (NWIN - 2))), 1), (top | ((1 << (C * (NWIN - 1))) - 1), (1 << 63) - 1),
             (top | (0xC000 << (C * (NWIN - 2))) | 0x1234, rng.randrange(1 << 63))]
    cases += [(rng.randrange(1 << 63), rng.randrange(1 << 63)) for _ in range(50)]
    carried = 0
    for a, b in cases:
        assert a < 1 << 63 and b < 1 << 63
        da, db = signed_digits(a, NWIN), signed_digits(b, NWIN)
        assert value(da) == a and value(db) == b
        assert all(-half <= d <= half for d in da + db)
        assert da[-1] >= 0 and db[-1] >= 0  # the top window keeps 2^(c-1): no carry leaves a half
        # rows 0 .. nwin-1 stand for a, rows nwin .. 2 nwin - 1 for b (times mu, not times 2^64)
        whole = signed_digits(a | (b << 64), 2 * NWIN)
        assert value(whole) == a | (b << 64)
        if da[-1] == half:
            assert (value(whole[:NWIN]), value(whole[NWIN:])) == (a - (1 << 64), b + 1)
            carried += 1
        else:
            assert (value(whole[:NWIN]), value(whole[NWIN:])) == (a, b)
    assert carried >= 3


def test_product_counts_of_the_late_form():
    rng = random.Random(2104)
    sig = B.g1_compress(B.ec_mul(B.FP, B.G1_GEN, 0x7654321))
    for _ in range(20):
        u0, u1 = rng.randrange(p), rng.randrange(p)
        K = M.Counter()
        distinct, mid, c = M.g1_sum_pre(K, M.sswu_parts(u0, rng.randrange(1, p)), M.sswu_parts(u1, rng.randrange(1, p)))
        assert distinct and K.n == 6
        st, pt, inv_c = M.decode_ride(K, sig, c)
        assert st == 1 and K.n == 6 + 2 + 6  # x^3 of the signature, then the ride's six
        q = M.g1_sum_post(K, mid, inv_c)
        assert K.n == 6 + 2 + 6 + 6
        assert q == sswu_sum(u0, u1) and on_e1p(q)
        assert B.iso_map_g1(q) == B.ec_add(B.FP, B.iso_map_g1(B.sswu_g1(u0)), B.iso_map_g1(B.sswu_g1(u1)))
    # the hash side of a round: 6 + 6 + 6 and the 4 conversions into the MSM's form (sigma x, y; the hash point's x, y)
    # against 6 + 6 + 6 + 31 and 5 conversions, then k_msm_prep28's 4 conversions, 7 products and 2 images
    late, before = 6 + 6 + 6 + 4, 6 + 6 + 6 + 31 + 5
    assert (late, before) == (22, 54)
