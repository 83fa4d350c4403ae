"""Integer model of the Jacobian-input G2 subgroup test (drand_amd/csrc/fp2_28.hpp g2_jac_in_subgroup28), for
tests/test_fp2_28_jac_model.py. Test infrastructure only.

Built on fp2_28_model: every product operand and every sum is bound-checked there, so a step of the device formula
whose bounds do not hold for a stored bucket sum fails in the model. The input is a Jacobian point as the batched
subgroup test's reduction stores it: X < 2p, Y < 3p and Z < 12p per component (every point formula ends
with X3, Y3 reduced below 2p; Z is (8, 12) after a doubling, (6, 12) after a mixed and (4, 6) after a Jacobian
addition; a sum of one entry is that entry, and a bucket holding one negated point keeps Y = 3p - y < 3p).
The steps follow the device function line by line: the six doubling runs of [|u|] with the Jacobian addition of T
after the first five, the fast additions first and the exact ones when the result is poisoned, and the projective
comparison of psi(T) = (conj(X) PSI_X, conj(Y) PSI_Y, conj(Z)) with -[|u|] T.
"""
import fp2_28_model as M

lin = M.lin
UABS_RUNS = (1, 2, 3, 9, 32, 16)  # fp2_28.hpp uabs_run: the doublings between |u|'s set bits
BOUNDS = (2, 3, 12)               # units of p, per component: the largest a stored sum's X, Y, Z may be


def check_bounds(T):
    X, Y, Z, _ = T
    for v, k in zip((X, Y, Z), BOUNDS):
        assert 0 <= v[0] < k * M.p and 0 <= v[1] < k * M.p


def mul_uabs(T, exact):
    """g2_jac_mul_uabs_ld<EXACT>: [|u|] T for finite T; the fast form leaves Z = 0 mod p after an exceptional case"""
    acc = T
    for r, k in enumerate(UABS_RUNS):
        for _ in range(k):
            acc = M.dbl(acc)
        if r < 5:
            acc = M.add_core(acc, T, exact)
    return acc


def jac_in_subgroup(T, stats=None):
    """g2_jac_in_subgroup28 on T = (X, Y, Z, inf). stats (optional dict) counts the exact retries."""
    if T[3]:
        return True
    check_bounds(T)
    acc = mul_uabs(T, False)
    if M.poisoned(acc):
        if stats is not None:
            stats["exact"] = stats.get("exact", 0) + 1
        acc = mul_uabs(T, True)
    Xa, Ya, Za, fl = acc
    if fl:
        return False
    X, Y, Z, _ = T
    cx, cy = M._psi_consts()
    cz = (Z[0], lin(12, Z[1], -1, Z[1], 0))            # conj(Z_T) < (12, 12)
    za2 = M.s2(Za, 12)
    zt2 = M.s2(cz, 12)
    px = M.m2(M.conj2(X), M.from_f2(cx))               # (4, 6)
    if not M.zero2(M.lin2(4, 6, M.m2(px, za2), 1, M.m2(Xa, zt2), -1)):
        return False
    py = M.m2(M.conj2(Y, 3), M.from_f2(cy))         # Y_T < 3
    ly = M.m2(py, M.m2(za2, Za))
    ry = M.m2(Ya, M.m2(zt2, cz))
    return M.zero2(M.add2(ly, ry))
