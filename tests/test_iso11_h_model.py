"""CPU: the integer model of the G1 hash's 11-isogeny in its kernel-polynomial form (tests/iso11_h_model.py, a line by
line restatement of h2c.hpp iso11_jac and of fp_mul28.hpp's Montgomery body on limbs) against the oracle.

* the identities the map rests on, recomputed from the oracle's printed tables (bls_py.ISO11_*): x_den has a monic
  square root h, h^2 == x_den and h^3 == y_den coefficient for coefficient, and the header's ISO11_H_28 is that h;
  the same for the G2 3-isogeny (degree 1 over Fp2) and ISO3_H;
* 200 random points of E1' as Jacobian triples with a random Z, held to bls_py.iso_map_g1 as affine values;
* the identity (Z = 0), a point of the isogeny's kernel if h has a root in Fp (gcd(h, x^p - x)), the inputs at the top
  of the stated bounds (stored words p - 1, 28-bit values 2p - 1);
* the Montgomery body on limbs: the 64-bit column bounds with every limb at 2^28 - 1, and the result and its bounds
  at the edge of the value bound X Y < 2^392 p.
The model asserts every bound the device code relies on, so a violated bound fails here."""
import os
import random
import re

import bls_py as B
import iso11_h_model as H

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
p = H.p
RM = (1 << 384) % p


def _header():
    with open(os.path.join(ROOT, "drand_amd", "csrc", "consts.hpp")) as f:
        return f.read()


def _kernel_poly():
    h = H.monic_sqrt(B.ISO11_XDEN)
    return h


def test_kernel_polynomial_identities_and_header_table():
    h = _kernel_poly()
    assert len(h) == 6 and h[-1] == 1
    h2 = H.poly_mul(h, h)
    assert h2 == [c % p for c in B.ISO11_XDEN]
    assert H.poly_mul(h2, h) == [c % p for c in B.ISO11_YDEN]
    txt = _header()
    m = re.search(r"uint32_t ISO11_H_28\[6\]\[14\] = \{(.*?)\};", txt)
    words = [int(v, 16) for v in re.findall(r"0x([0-9a-f]+)u", m.group(1))]
    assert len(words) == 6 * 14
    for i, c in enumerate(h):
        assert H.value(words[14 * i:14 * i + 14]) == c * H.RP % p
    assert "ISO11_XDEN" not in txt and "ISO11_YDEN" not in txt and "ISO3_XDEN" not in txt and "ISO3_YDEN" not in txt


def test_g2_kernel_polynomial_identities_and_header_table():
    (c0, c1, lead) = B.ISO3_XDEN
    assert lead == (1, 0)
    half = (p + 1) // 2
    k = (c1[0] * half % p, c1[1] * half % p)  # h = x + k
    red = lambda a: (a[0] % p, a[1] % p)  # noqa: E731
    k2 = B.f2mul(k, k)
    assert red(k2) == red(c0)
    three = lambda a: (3 * a[0] % p, 3 * a[1] % p)  # noqa: E731
    assert [red(c) for c in B.ISO3_YDEN] == [red(B.f2mul(k2, k)), three(k2), three(k), (1, 0)]
    m = re.search(r"uint32_t ISO3_H\[2\]\[2\]\[12\] = \{(.*?)\};", _header())
    words = [int(v, 16) for v in re.findall(r"0x([0-9a-f]+)u", m.group(1))]
    vals = [sum(w << (32 * j) for j, w in enumerate(words[12 * i:12 * i + 12])) for i in range(4)]
    assert vals == [k[0] * RM % p, k[1] * RM % p, RM, 0]


def _e1p_point(rng):
    while True:
        x = rng.randrange(p)
        y = B.fsqrt((x * x * x + B.A1P * x + B.B1P) % p)
        if y is not None:
            return (x, y if rng.random() < 0.5 else (-y) % p)


def _affine(Xo, Yo, Zo):
    norm = lambda v: v * pow(RM, -1, p) % p  # noqa: E731
    zi = pow(norm(Zo), -1, p)
    return (norm(Xo) * zi * zi % p, norm(Yo) * zi ** 3 % p)


def _jac(x, y, z):
    m = lambda v: v % p * RM % p  # noqa: E731
    return m(x * z * z), m(y * z ** 3), m(z)


def test_isogeny_model_matches_oracle_on_random_jacobian_points():
    rng = random.Random(1111)
    h = _kernel_poly()
    for _ in range(200):
        x, y = _e1p_point(rng)
        z = rng.randrange(1, p)
        got = H.iso11_h(*_jac(x, y, z), B.ISO11_XNUM, B.ISO11_YNUM, h)
        assert got[2] != 0
        assert _affine(*got) == B.iso_map_g1((x, y))


def test_isogeny_model_identity_kernel_and_extreme_inputs():
    rng = random.Random(1112)
    h = _kernel_poly()
    x, y = _e1p_point(rng)
    # the identity: Z = 0, whatever X and Y hold
    assert H.iso11_h(x * RM % p, y * RM % p, 0, B.ISO11_XNUM, B.ISO11_YNUM, h)[2] == 0
    # stored words at their top value p - 1 (as normal values: some x, y, z; the oracle's map of them)
    inv = pow(RM, -1, p)
    z = (p - 1) * inv % p
    zi = pow(z, -1, p)
    want = B.iso_map_g1(((p - 1) * inv * zi * zi % p, (p - 1) * inv * zi ** 3 % p))
    got = H.iso11_h(p - 1, p - 1, p - 1, B.ISO11_XNUM, B.ISO11_YNUM, h)
    assert want is not None and _affine(*got) == want
    # 28-bit-form values at the top of the stated bound (< 2p), against the same map on their residues
    top = 2 * p - 1
    xo, yo, zo = H.iso11_h_core(top, top, top, B.ISO11_XNUM, B.ISO11_YNUM, h)
    f = lambda v: v * pow(H.RP, -1, p) % p  # noqa: E731
    z = f(top)
    zi = pow(z, -1, p)
    want = B.iso_map_g1((f(top) * zi * zi % p, f(top) * zi ** 3 % p))
    zoi = pow(f(zo), -1, p)
    assert want is not None and (f(xo) * zoi * zoi % p, f(yo) * zoi ** 3 % p) == want
    # a point of the kernel: a root of h in Fp, if there is one
    g = H.roots_in_fp(h)
    if len(g) == 1:
        assert g == [1]  # h has no root in Fp: no Fp-rational x reaches the kernel, and the case does not exist
        return
    r = H.a_root(g, rng)
    assert sum(c * pow(r, i, p) for i, c in enumerate(h)) % p == 0
    assert B.iso_map_g1((r, 1)) is None
    zz = rng.randrange(1, p)
    assert H.iso11_h(*_jac(r, 1, zz), B.ISO11_XNUM, B.ISO11_YNUM, h)[2] == 0


def test_montgomery_body_column_bounds_and_value_edge():
    full = [H.MASK] * 14
    # every limb at 2^28 - 1: 14 limb products and 14 quotient products a column, all inside 64 bits (the value bound
    # does not hold here, so only the columns are looked at)
    H.mont_mul_limbs(full, full, normalised=False)
    # the edge of the value bound X Y < 2^392 p, which every product of the map stays far below (4p x 2p)
    edge = H.RP * p - 1
    for x in (1 << 391, H.RP - 1, 50 * p, 4 * p - 1):
        y = min(edge // x, H.RP - 1)
        r = H.mul(x, y)
        assert r < 2 * p and (r * H.RP - x * y) % p == 0
