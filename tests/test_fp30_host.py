"""drand_amd/csrc/fp_mul30.hpp (the fixed-exponent Fp chains on 13 signed 30-bit digits) compiled for the host from
the same source: entry from 12 words, the chain exactly as the device loop runs it (m30::pow_sched with the schedules
parsed here from consts.hpp), exit to canonical words, for all four exponents, against Python's pow(x, e, p). Built
twice with g++ -O2: plainly, and with -fsanitize=signed-integer-overflow,shift -fno-sanitize-recover=all, so that an
accumulator leaving 64 bits or an undefined shift ends the run. A stand-alone program fed on stdin. CPU only."""
import os
import random
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "drand_amd", "csrc")
P = 0x1a0111ea397fe69a4b1ba7b6434bacd764774b84f38512bf6730d2a0f6b0f6241eabfffeb153ffffb9feffffffffaaab
R = (1 << 384) % P
EXPONENTS = {"SCHED_SQRT": (P + 1) // 4, "SCHED_SR1_C1": (P - 3) // 4, "SCHED_INV": P - 2, "SCHED_LEGENDRE": (P - 1) // 2}

# stdin: "S <len> <n> <n hex entries>" sets the schedule, "X <hex>" runs one value (the 12-word Montgomery form in,
# the 12-word Montgomery form of the power out)
HARNESS = r"""
#include <cstdio>
#include <cstring>
#include <vector>
#define DH_HD static inline
#include "fp_mul30.hpp"
int main() {
  std::vector<uint32_t> sched;
  int len = 0;
  char tag[4], hex[128];
  while (scanf("%3s", tag) == 1) {
    if (tag[0] == 'S') {
      int n;
      if (scanf("%d %d", &len, &n) != 2) return 2;
      sched.assign(n, 0);
      for (int i = 0; i < n; i++)
        if (scanf("%x", &sched[i]) != 1) return 2;
      continue;
    }
    if (scanf("%127s", hex) != 1) return 2;
    uint32_t a[12] = {0}, r[12];
    size_t n = strlen(hex);
    for (size_t k = 0; k < n; k++) {  // hex digit k from the right end
      char ch = hex[n - 1 - k];
      uint32_t d = ch <= '9' ? ch - '0' : (ch | 32) - 'a' + 10;
      a[k / 8] |= d << (4 * (k % 8));
    }
    const dh::m30::el x = dh::m30::from(a);
    const dh::m30::el y = dh::m30::pow_sched<SCHED_W, SCHED_ODD, SCHED_RUNS>(x, sched.data(), len);
    dh::m30::to(r, y);
    for (int i = 11; i >= 0; i--) printf("%08x", r[i]);
    printf("\n");
  }
  return 0;
}
"""


def _consts():
    with open(os.path.join(CSRC, "consts.hpp")) as f:
        return f.read()


def _int(txt, name):
    return int(re.search(r"constexpr int %s = (\d+);" % name, txt).group(1))


def _sched(txt, name):
    m = re.search(r"uint32_t %s\[(\d+)\] = \{([^}]*)\};" % name, txt)
    arr = [int(v, 16) for v in m.group(2).split(",")]
    assert len(arr) == int(m.group(1))
    return arr, _int(txt, name + "_LEN")


def _inputs():
    rng = random.Random(390)
    return [0, 1, 2, P - 1, P - 2, (P - 1) // 2, (P + 1) // 2] + [rng.randrange(P) for _ in range(2000)]


@pytest.fixture(scope="module")
def feed():
    """the program's input and the expected output lines, shared by both builds"""
    txt = _consts()
    xs = _inputs()
    rinv = pow(R, -1, P)
    lines, want = [], []
    for name, e in EXPONENTS.items():
        arr, length = _sched(txt, name)
        lines.append("S %d %d %s" % (length, len(arr), " ".join("%x" % v for v in arr)))
        for x in xs:
            lines.append("X %x" % x)  # x = y R: the result is y^e R
            want.append(pow(x * rinv % P, e, P) * R % P)
    defs = ["-DSCHED_%s=%d" % (n, _int(txt, "SCHED_" + n)) for n in ("W", "ODD", "RUNS")]
    return "\n".join(lines) + "\n", want, defs


def _build_and_run(tmp_path, feed, name, flags):
    text, want, defs = feed
    src = tmp_path / (name + ".cpp")
    src.write_text(HARNESS)
    exe = tmp_path / name
    subprocess.check_call(["g++", "-O2", "-std=c++17", *flags, *defs, "-I", CSRC, str(src), "-o", str(exe)])
    run = subprocess.run([str(exe)], input=text, capture_output=True, text=True)
    assert run.returncode == 0, run.stderr[-2000:]
    out = run.stdout.split()
    assert len(out) == len(want)
    for i, (o, w) in enumerate(zip(out, want)):
        assert int(o, 16) == w, i


@pytest.mark.skipif(shutil.which("g++") is None, reason="no host C++ compiler")
def test_chains_host_build(tmp_path, feed):
    _build_and_run(tmp_path, feed, "fp30_check", [])


@pytest.mark.skipif(shutil.which("g++") is None, reason="no host C++ compiler")
def test_chains_host_build_sanitized(tmp_path, feed):
    _build_and_run(tmp_path, feed, "fp30_check_ubsan",
                   ["-fsanitize=signed-integer-overflow,shift", "-fno-sanitize-recover=all"])
