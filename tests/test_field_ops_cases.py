"""CPU: the case generator of the field-layer op kernel (tests/field_ops_cases.py), and fp_mul28.hpp compiled for the host.

* the generator: its op table equals the enum of drand_amd/csrc/k_fieldops.hip; every case has a complete record;
  every contract case's check accepts the integer models' result (so the contract can be met, and the models have
  asserted the header's entry bounds on the lazy inputs while producing it) and refuses a result off by one in a limb
  (and a reduced value moved by 2p); every raw-limb product keeps each column of fp_mul28.hpp's body inside 64 bits and the body, restated on
  integers, gives the exact Montgomery quotient the cases expect; both lane arrangements hold every case.
* fp_mul28.hpp for the host, as a stand-alone program fed on stdin, built with ROCm's clang (g++ 11 lacks
  __builtin_subc) plainly and with -fsanitize=shift,signed-integer-overflow: mont_mul / mont_sqr on the raw-limb cases,
  mul / sqr on the 12-word cases (the unreduced sums included), split / join / final_sub against shifts and masks.
* the debug entry is the kernel's only caller.
"""
import os
import re
import subprocess

import pytest

import field_ops_cases as C

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "drand_amd", "csrc")
CLANG = "/opt/rocm/lib/llvm/bin/clang++"


def test_op_table_matches_the_kernel():
    with open(os.path.join(CSRC, "k_fieldops.hip")) as f:
        txt = f.read()
    enum = txt[txt.index("enum field_op"):txt.index("};", txt.index("enum field_op"))]
    table = {m.group(1): int(m.group(2)) for m in re.finditer(r"FO_(\w+) = (\d+),", enum)}
    assert table == C.OPS
    with open(os.path.join(CSRC, "kernels.hpp")) as f:
        k = f.read()
    for name, v in (("FO_SCALARS", C.SCALARS), ("FO_IN_WORDS", C.IN_WORDS), ("FO_OUT_FLAGS", C.OUT_FLAGS), ("FO_OUT_WORDS", C.OUT_WORDS)):
        assert int(re.search(r"constexpr size_t %s = (\d+);" % name, k).group(1)) == v
    kp = re.findall(r"DH_KP\((\d+),", open(os.path.join(CSRC, "fp28.hpp")).read())
    assert sorted(int(x) for x in kp) == list(C.KS)


def test_debug_entry_is_the_only_caller():
    n = 0
    for name in os.listdir(CSRC):
        if name.endswith((".cpp", ".hip", ".hpp")) and name != "k_fieldops.hip":
            with open(os.path.join(CSRC, name)) as f:
                txt = f.read()
            assert "k_field_ops" not in txt, name
            n += len(re.findall(r"launch_field_ops\(", txt))
    assert n == 2  # the declaration (kernels.hpp) and dh_field_ops_debug's call (drandhip.cpp)
    with open(os.path.join(CSRC, "drandhip.cpp")) as f:
        txt = f.read()
    body = txt[txt.index("int dh_field_ops_debug("):txt.index("int dh_msm_level0_shape_debug(")]
    assert "launch_field_ops(" in body


@pytest.mark.parametrize("fam", list(C.FAMILIES))
def test_generator(fam):
    cases = C.family(fam)
    assert len(set(c.name for c in cases)) == len(cases), "case names are unique"
    for c in cases:
        assert c.op in C.OPS.values() or any(b <= c.op < b + 15 for b in (32, 48, 64)) or 104 <= c.op < 112 or 132 <= c.op < 136
        if c.check is None:
            continue
        assert c.model is not None, c.name
        c.check(list(c.model))
        # the contract bites: a reduced result moved by 2p is congruent but no longer below 2p ...
        moved = list(c.model)
        v = C.val(moved[:14]) + 2 * C.P
        if c.op in (C.OPS["F28_RED"], C.OPS["F2_RED"]):
            moved[:14] = C.limbs(v)
            with pytest.raises(AssertionError):
                c.check(moved)
        # ... or by one in the lowest limb
        off = list(c.model)
        if not off[C.OUT_FLAGS] and not off[C.OUT_FLAGS + 1]:
            off[0] ^= 1
            with pytest.raises(AssertionError):
                c.check(off)
    uniform, inter = C.arrangements(cases)
    assert len(uniform) % 64 != 0 and set(uniform) == set(inter) == set(range(len(cases)))
    if len(set(c.op for c in cases)) > 1:
        # every wave of the interleaved batch mixes opcodes, so each operation is entered with part of the wave masked
        # off; the commonest opcode (f28_red's 10,085 inputs) has more lanes than all the others can separate
        ops = [cases[i].op for i in inter]
        assert all(len(set(ops[k:k + 64])) > 1 for k in range(0, len(ops), 64))
        differ = sum(a != b for a, b in zip(ops, ops[1:]))
        assert differ >= len(ops) - max(ops.count(o) for o in set(ops))


def test_raw_products_stay_in_64_bits():
    """fp_mul28.hpp's body restated on integers, column by column: no column leaves uint64 on any raw-limb case, and
    the result is the exact quotient (X Y + m p) / 2^392, m = -X Y / p mod 2^392"""
    n = 0
    for name, X, Y, _ in C.raw_product_inputs():
        assert C.m28_emul(X, Y) == C.qlimbs(C.montq(C.val(X), C.val(X if Y is None else Y))), name
        n += 1
    assert n > 300
    x = 48 * C.P - 1  # the pair the bare product's bound is stated on: inside the model's bound, result at 1.977 p
    assert abs(C.M.mont(x, C.RP * C.P // x) / C.P - 1.977) < 1e-3


HARNESS = r"""
#include <cstdint>
#include <cstdio>
#include <cstring>
#define __device__
#define __forceinline__ inline
#include "fp_mul28.hpp"
using namespace dh::m28;
static bool rd(uint32_t* w, int n) {
  for (int i = 0; i < n; i++)
    if (scanf("%x", &w[i]) != 1) return false;
  return true;
}
static void pr(const uint32_t* w, int n) {
  for (int i = 0; i < n; i++) printf("%x ", w[i]);
  printf("\n");
}
int main() {
  char t[8];
  while (scanf("%7s", t) == 1) {
    uint32_t a[14] = {0}, b[14] = {0}, r[14] = {0};
    int n = 14;
    if (!strcmp(t, "M")) {
      if (!rd(a, 14) || !rd(b, 14)) return 2;
      mont_mul(r, a, b);
    } else if (!strcmp(t, "S")) {
      if (!rd(a, 14)) return 2;
      mont_sqr(r, a);
    } else if (!strcmp(t, "m")) {
      if (!rd(a, 12) || !rd(b, 12)) return 2;
      mul(r, a, b);
      n = 12;
    } else if (!strcmp(t, "s")) {
      if (!rd(a, 12)) return 2;
      sqr(r, a);
      n = 12;
    } else if (t[0] == 'p') {
      if (!rd(a, 12)) return 2;
      if (t[1] == '0') split<0>(r, a);
      else if (t[1] == '4') split<4>(r, a);
      else split<8>(r, a);
    } else if (!strcmp(t, "j")) {
      if (!rd(a, 14)) return 2;
      join(r, a);
      n = 12;
    } else if (!strcmp(t, "f")) {
      if (!rd(r, 12)) return 2;
      final_sub(r);
      n = 12;
    } else {
      return 3;
    }
    pr(r, n);
  }
  return 0;
}
"""


def _hex(ws):
    return " ".join("%x" % w for w in ws)


@pytest.fixture(scope="module")
def feed():
    lines, want = [], []
    for c in C.family("f28"):
        if c.op in (C.OPS["F28_MUL"], C.OPS["F28_SQR"]):
            sq = c.op == C.OPS["F28_SQR"]
            lines.append(("S " + _hex(c.rec[:14])) if sq else ("M %s %s" % (_hex(c.rec[:14]), _hex(c.rec[14:28]))))
            want.append((c.name, c.exp[:14]))
    w32 = lambda ws: sum(w << (32 * i) for i, w in enumerate(ws))  # noqa: E731
    for c in C.family("fp"):
        if c.op == C.OPS["FP_MUL"]:
            lines.append("m %s %s" % (_hex(c.rec[:12]), _hex(c.rec[12:24])))
        elif c.op == C.OPS["FP_SQR"]:
            lines.append("s " + _hex(c.rec[:12]))
        elif c.op == C.OPS["FP_MUL_NR"]:  # the sums as fp_add_nr hands them over
            a, b = w32(c.rec[:12]) + w32(c.rec[12:24]), w32(c.rec[24:36]) + w32(c.rec[36:48])
            lines.append("m %s %s" % (_hex(C.words(a, 12)), _hex(C.words(b, 12))))
        else:
            continue
        want.append((c.name, c.exp[:12]))
    for x in C.field_values() + [(1 << 384) - 1, 2 * C.P - 1]:
        for s in (0, 4, 8):
            lines.append("p%d %s" % (s, _hex(C.words(x, 12))))
            want.append(("split<%d> %x" % (s, x), C.limbs((x << s) & (C.RP - 1))))
        lines.append("j " + _hex(C.limbs(x)))
        want.append(("join %x" % x, C.words(x, 12)))
        if x < 2 * C.P:
            lines.append("f " + _hex(C.words(x, 12)))
            want.append(("final_sub %x" % x, C.words(x - C.P if x >= C.P else x, 12)))
    return "\n".join(lines) + "\n", want


def _build_and_run(tmp_path, feed, name, flags):
    text, want = feed
    src = tmp_path / (name + ".cpp")
    src.write_text(HARNESS)
    exe = tmp_path / name
    subprocess.check_call([CLANG, "-O2", "-std=c++17", *flags, "-I", CSRC, str(src), "-o", str(exe)])
    run = subprocess.run([str(exe)], input=text, capture_output=True, text=True)
    assert run.returncode == 0, run.stderr[-2000:]
    rows = run.stdout.strip().split("\n")
    assert len(rows) == len(want)
    for row, (nm, w) in zip(rows, want):
        assert [int(v, 16) for v in row.split()] == list(w), nm


@pytest.mark.skipif(not os.path.exists(CLANG), reason="ROCm's clang++ missing (g++ 11 has no __builtin_subc)")
def test_fp_mul28_host_build(tmp_path, feed):
    _build_and_run(tmp_path, feed, "fp_mul28_check", [])


@pytest.mark.skipif(not os.path.exists(CLANG), reason="ROCm's clang++ missing (g++ 11 has no __builtin_subc)")
def test_fp_mul28_host_build_sanitized(tmp_path, feed):
    _build_and_run(tmp_path, feed, "fp_mul28_check_ubsan",
                   ["-fsanitize=shift,signed-integer-overflow", "-fno-sanitize-recover=all"])
