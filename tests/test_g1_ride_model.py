"""CPU: the integer model of the G1 round's ride (tests/g1_ride_model.py: h2c.hpp fp_sqrt_ride, g1_sum_pre,
g1_sum_post, iso11_aff and codec.hpp g1_decompress_ride restated product by product) against the oracle.

* -4 is not a cube mod p, so a curve's right-hand side x^3 + 4 is never 0 and the chain always carries an inverse;
* root and inverse for residue and non-residue a and for the stand-in a = 1, with random c;
* the image equal to bls_py's map_to_curve sum (iso_map_g1(sswu(u0)) + iso_map_g1(sswu(u1)) on E1) for 200 random
  (u0, u1), the SSWU x's spread over random denominators as the device's are, and for the two inputs no hash reaches:
  u1 = u0 (the doubling) and u1 = -u0 (the identity), which take the exceptional order;
* the count of products: 6 around the chain (five and the root's check), 6 + 6 for the sum, 31 for the isogeny and
  5 conversions, 54 in all against the 108 of swu_jac x 2, add-2007-bl and iso11_jac;
* the decode's statuses for every class of rejected encoding, each still yielding the inverse."""
import random

import bls_py as B
import g1_ride_model as M
import iso11_h_model as H

p = M.p
HPOLY = H.monic_sqrt(B.ISO11_XDEN)
XNUM = [c % p for c in B.ISO11_XNUM]
YNUM = [c % p for c in B.ISO11_YNUM]


def test_minus_four_is_not_a_cube():
    assert p % 3 == 1 and p % 4 == 3
    assert pow(p - 4, (p - 1) // 3, p) != 1


def test_ride_gives_root_and_inverse():
    rng = random.Random(2001)
    seen = set()
    for k in range(200):
        a = 1 if k % 10 == 0 else rng.randrange(1, p)
        c = rng.randrange(1, p)
        K = M.Counter()
        qr, y, inv_c = M.fp_sqrt_ride(K, a, c)
        assert K.n == 6
        assert inv_c * c % p == 1
        assert qr == (pow(a, (p - 1) // 2, p) == 1)
        seen.add(qr)
        if qr:
            assert y * y % p == a and y in (B.fsqrt(a), p - B.fsqrt(a))
        else:
            assert B.fsqrt(a) is None and y * y % p == p - a
        if a == 1:
            assert qr
    assert seen == {True, False}
    # c = 0 (callers never pass it): no root, no inverse, no fault
    assert M.fp_sqrt_ride(M.Counter(), 5, 0) == (False, 0, 0)


def _want(u0, u1):
    return B.ec_add(B.FP, B.iso_map_g1(B.sswu_g1(u0)), B.iso_map_g1(B.sswu_g1(u1)))


def test_image_matches_oracle_and_product_count():
    rng = random.Random(2002)
    for _ in range(200):
        u0, u1 = rng.randrange(p), rng.randrange(p)
        K, conv = M.Counter(), M.Counter()
        st, pt, q = M.hash_point(u0, u1, XNUM, YNUM, HPOLY, None, rng.randrange(1, p), rng.randrange(1, p), K, conv)
        assert (st, pt) == (0, None)
        assert q is not None and q == _want(u0, u1)
        assert K.n == 6 + 6 + 6 + 31 and conv.n == 5 and K.n + conv.n == 54
    # the parts, as DESIGN §20 tables them
    K = M.Counter()
    distinct, mid, c = M.g1_sum_pre(K, M.sswu_parts(3, 7), M.sswu_parts(5, 9))
    assert distinct and K.n == 6
    K = M.Counter()
    pt = M.g1_sum_post(K, mid, pow(c, -1, p))
    assert K.n == 6
    assert pt == B.ec_add(B.FP, B.sswu_g1(3), B.sswu_g1(5))  # the addition law does not involve the curve's a
    K = M.Counter()
    M.iso11_aff(K, pt, XNUM, YNUM, HPOLY)
    assert K.n == 11 + 15 + 4 + 1


def test_exceptional_inputs_take_the_textbook_order():
    rng = random.Random(2003)
    u = rng.randrange(1, p)
    st, pt, q = M.hash_point(u, u, XNUM, YNUM, HPOLY)
    assert q == B.ec_dbl(B.FP, B.iso_map_g1(B.sswu_g1(u))) and q is not None
    st, pt, q = M.hash_point(u, p - u, XNUM, YNUM, HPOLY)
    assert q is None
    assert M.hash_point(0, 0, XNUM, YNUM, HPOLY)[2] == _want(0, 0)


def rejected_encodings(sig):
    """One valid compressed signature -> {class: encoding} for every class rejected before the root."""
    raw = bytearray(sig)
    clear = bytearray(raw)
    clear[0] &= 0x7F
    inf = bytes([0xC0]) + bytes(47)
    stray = bytearray(inf)
    stray[31] = 1
    big = bytearray((p + 5).to_bytes(48, "big"))
    big[0] |= 0x80
    return {"compression bit clear": bytes(clear), "infinity": inf, "infinity with a stray bit": bytes(stray),
            "x >= p": bytes(big)}


def non_residue(sig):
    x = int.from_bytes(bytes([sig[0] & 0x1F]) + bytes(sig[1:]), "big")
    while B.fsqrt((x * x * x + B.B1) % p) is not None:
        x += 1
    out = bytearray(x.to_bytes(48, "big"))
    out[0] |= sig[0] & 0xE0
    return bytes(out)


def test_decode_statuses_and_inverse_for_every_encoding_class():
    rng = random.Random(2004)
    pt = B.ec_mul(B.FP, B.G1_GEN, 0x1234567)
    for sign in (0, 1):
        want = pt if sign == 0 else B.ec_neg(B.FP, pt)
        sig = B.g1_compress(want)
        c = rng.randrange(1, p)
        st, got, inv_c = M.decode_ride(M.Counter(), sig, c)
        assert (st, got) == (1, want) and inv_c * c % p == 1
        assert got == B.g1_decompress(sig, subgroup_check=False)
    for name, enc in rejected_encodings(sig).items():
        c = rng.randrange(1, p)
        st, got, inv_c = M.decode_ride(M.Counter(), enc, c)
        assert got is None and inv_c * c % p == 1, name
        assert st == (2 if name == "infinity" else 0), name
    c = rng.randrange(1, p)
    st, got, inv_c = M.decode_ride(M.Counter(), non_residue(sig), c)
    assert (st, got) == (0, None) and inv_c * c % p == 1
    # the hash point does not depend on what the signature was
    u0, u1 = rng.randrange(p), rng.randrange(p)
    for enc in list(rejected_encodings(sig).values()) + [non_residue(sig), sig]:
        assert M.hash_point(u0, u1, XNUM, YNUM, HPOLY, enc)[2] == _want(u0, u1)
