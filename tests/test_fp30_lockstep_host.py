"""drand_amd/csrc/fp_mul30.hpp compiled for the host from the same source: the lockstep forms of the body
(m30::mont_sqr2 / mont_mul2, two operations side by side in one pass over the columns) against the single forms and
against Python. For every pair of values (x0, x1) and multipliers (y0, y1) the program runs 30 dependent steps, a
squaring each and a product every fifth, once through the lockstep body and once through the single body, compares all
26 digits after every step, and prints both results through the library's exit; the test compares them with the same
steps on Python integers mod p. 2,000 random pairs and the edge values 0, 1, 2, p - 1, p - 2, (p +- 1) / 2. Built
twice with g++ -O2: plainly, and with -fsanitize=signed-integer-overflow,shift -fno-sanitize-recover=all, so that an
accumulator leaving 64 bits under the rounding bias or an undefined shift ends the run. A stand-alone program fed on
stdin. The chains themselves (m30::pow_sched on the dependent body, all four committed schedules, against
pow(x, e, p)) are tests/test_fp30_host.py's. CPU only."""
import os
import random
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "drand_amd", "csrc")
P = 0x1a0111ea397fe69a4b1ba7b6434bacd764774b84f38512bf6730d2a0f6b0f6241eabfffeb153ffffb9feffffffffaaab
R = (1 << 384) % P
STEPS = 30

# stdin: lines of four hex values x0 x1 y0 y1 (12-word Montgomery forms); stdout: the two results, same form
HARNESS = r"""
#include <cstdio>
#include <cstring>
#define DH_HD static inline
#include "fp_mul30.hpp"
using namespace dh::m30;
static bool rd(uint32_t a[12]) {
  char hex[128];
  if (scanf("%127s", hex) != 1) return false;
  memset(a, 0, 48);
  size_t n = strlen(hex);
  for (size_t k = 0; k < n; k++) {  // hex digit k from the right end
    char ch = hex[n - 1 - k];
    uint32_t d = ch <= '9' ? ch - '0' : (ch | 32) - 'a' + 10;
    a[k / 8] |= d << (4 * (k % 8));
  }
  return true;
}
static void pr(const el& a) {
  uint32_t r[12];
  to(r, a);
  for (int i = 11; i >= 0; i--) printf("%08x", r[i]);
}
int main() {
  uint32_t w[4][12];
  while (rd(w[0])) {
    for (int j = 1; j < 4; j++)
      if (!rd(w[j])) return 2;
    el a0 = from(w[0]), a1 = from(w[1]);
    const el y0 = from(w[2]), y1 = from(w[3]);
    el s0 = a0, s1 = a1;
    for (int step = 1; step <= STEPS; step++) {
      if (step % 5 == 0) {
        mont_mul2(a0.l, a1.l, a0.l, a1.l, y0.l, y1.l);  // in place, as the chains run it
        s0 = mul(s0, y0);
        s1 = mul(s1, y1);
      } else {
        mont_sqr2(a0.l, a1.l, a0.l, a1.l);
        s0 = sqr(s0);
        s1 = sqr(s1);
      }
      if (memcmp(a0.l, s0.l, sizeof(a0.l)) || memcmp(a1.l, s1.l, sizeof(a1.l))) return 3;
    }
    pr(a0);
    printf(" ");
    pr(a1);
    printf("\n");
  }
  return 0;
}
"""


def _expected(x, y):
    """the steps on plain residues: x, y are the Montgomery forms X R, Y R"""
    rinv = pow(R, -1, P)
    a, m = x * rinv % P, y * rinv % P
    for step in range(1, STEPS + 1):
        a = a * m % P if step % 5 == 0 else a * a % P
    return a * R % P


@pytest.fixture(scope="module")
def feed():
    """the program's input and the expected output, shared by both builds"""
    rng = random.Random(3902)
    edge = [0, 1, 2, P - 1, P - 2, (P - 1) // 2, (P + 1) // 2]
    quads = [(a, edge[(i + 3) % 7], edge[(i + 5) % 7], b) for i, a in enumerate(edge) for b in edge[:3]]
    quads += [tuple(rng.randrange(P) for _ in range(4)) for _ in range(2000)]
    text = "".join("%x %x %x %x\n" % q for q in quads)
    want = [(_expected(x0, y0), _expected(x1, y1)) for x0, x1, y0, y1 in quads]
    return text, want


def _build_and_run(tmp_path, feed, name, flags):
    text, want = feed
    src = tmp_path / (name + ".cpp")
    src.write_text(HARNESS)
    exe = tmp_path / name
    subprocess.check_call(["g++", "-O2", "-std=c++17", *flags, "-DSTEPS=%d" % STEPS, "-I", CSRC, str(src), "-o", str(exe)])
    run = subprocess.run([str(exe)], input=text, capture_output=True, text=True)
    assert run.returncode == 0, (run.returncode, run.stderr[-2000:])
    out = [tuple(int(v, 16) for v in line.split()) for line in run.stdout.splitlines()]
    assert len(out) == len(want)
    for i, (o, w) in enumerate(zip(out, want)):
        assert o == w, i


@pytest.mark.skipif(shutil.which("g++") is None, reason="no host C++ compiler")
def test_lockstep_bodies_host_build(tmp_path, feed):
    _build_and_run(tmp_path, feed, "fp30_lockstep", [])


@pytest.mark.skipif(shutil.which("g++") is None, reason="no host C++ compiler")
def test_lockstep_bodies_host_build_sanitized(tmp_path, feed):
    _build_and_run(tmp_path, feed, "fp30_lockstep_ubsan",
                   ["-fsanitize=signed-integer-overflow,shift", "-fno-sanitize-recover=all"])
