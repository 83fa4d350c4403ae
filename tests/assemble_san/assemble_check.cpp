// Stand-alone check of drand_amd/csrc/assemble.hpp under ASan + UBSan (tests/test_assemble_host.py builds and runs it):
// the serial assemble of one pile of candidates, step for step as dh_assemble_device takes them, with the verifier's
// verdict per candidate handed in. The columns are heap blocks of exactly n x stride bytes, and every compare inside a
// round's run is repeated by value_equal on heap copies of exactly min(length, stride) bytes, where a read behind a
// value is a report. Input (little endian): u32 n, stride, chained, want_sig_len, dedupe, has_anchor, has_up_to,
// anchor_sig_len; u64 anchor_round, up_to; the anchor's signature; per candidate u64 round, u32 skip, verdict, sig_len,
// prev_len, then the signature and the previous_signature in full. Output: "S" and the status bytes, then one
// "O round src flags" line per output row.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../drand_amd/csrc/assemble.hpp"

using namespace dh::assemble;

static FILE* in;
static uint32_t u32() {
  uint32_t v = 0;
  if (fread(&v, 4, 1, in) != 1) exit(3);
  return v;
}
static uint64_t u64() {
  uint64_t v = 0;
  if (fread(&v, 8, 1, in) != 1) exit(3);
  return v;
}
static uint8_t* exact(size_t n) {  // n bytes from the file in a block of exactly n bytes
  uint8_t* p = (uint8_t*)malloc(n ? n : 1);
  if (!n) {  // no byte of it may be read: a one-byte block would hide that
    free(p);
    return nullptr;
  }
  if (fread(p, 1, n, in) != n) exit(3);
  return p;
}

int main(int argc, char** argv) {
  if (argc != 2 || !(in = fopen(argv[1], "rb"))) return 3;
  const uint32_t n = u32(), stride = u32(), chained = u32(), want = u32(), dedupe = u32(), has_anchor = u32(), has_up_to = u32(),
                 anchor_len = u32();
  const bounds b{u64(), u64(), has_anchor, has_up_to};
  uint8_t* anchor_sig = exact(anchor_len);
  std::vector<uint64_t> rounds(n);
  std::vector<uint32_t> sig_lens(n), prev_lens(n), verdict(n);
  std::vector<uint8_t> skip(n);
  std::vector<uint8_t*> sig_val(n), prev_val(n);  // exact-size copies of what the rows hold
  uint8_t* sigs = (uint8_t*)calloc((size_t)n * stride + !n, 1);
  uint8_t* prevs = chained ? (uint8_t*)calloc((size_t)n * stride + !n, 1) : nullptr;
  for (uint32_t i = 0; i < n; i++) {
    rounds[i] = u64();
    skip[i] = (uint8_t)u32();
    verdict[i] = u32();
    sig_lens[i] = u32();
    prev_lens[i] = u32();
    uint8_t* s = exact(sig_lens[i]);
    uint8_t* p = exact(prev_lens[i]);
    if (sig_lens[i] <= stride && s) memcpy(sigs + (size_t)i * stride, s, sig_lens[i]);  // longer: a zero row, the true length
    if (chained && prev_lens[i] <= stride && p) memcpy(prevs + (size_t)i * stride, p, prev_lens[i]);
    auto held = [&](const uint8_t* v, uint32_t len) -> uint8_t* {  // what the row holds: min(len, stride) bytes, exactly
      const uint32_t k = len < stride ? len : stride;
      if (!k) return nullptr;
      uint8_t* out = (uint8_t*)calloc(k, 1);
      if (len <= stride) memcpy(out, v, k);  // a longer value: zeros
      return out;
    };
    sig_val[i] = held(s, sig_lens[i]);
    prev_val[i] = chained ? held(p, prev_lens[i]) : nullptr;
    free(s);
    free(p);
  }
  const cols c{rounds.data(), sigs, sig_lens.data(), prevs, chained ? prev_lens.data() : nullptr, skip.data(), stride, stride};
  std::vector<uint32_t> status(n), idx;
  for (uint32_t i = 0; i < n; i++) {
    status[i] = pre_status(rounds[i], skip[i] != 0, b);
    if (!status[i]) idx.push_back(i);
  }
  std::stable_sort(idx.begin(), idx.end(), [&](uint32_t x, uint32_t y) { return rounds[x] < rounds[y]; });
  const size_t m = idx.size();
  std::vector<size_t> run_of(m), run_start, rep(m);
  for (size_t j = 0; j < m; j++) {
    if (j == 0 || rounds[idx[j]] != rounds[idx[j - 1]]) run_start.push_back(j);
    run_of[j] = run_start.size() - 1;
  }
  for (size_t j = 0; j < m; j++) {
    rep[j] = dedupe ? class_of(c, idx.data(), run_start[run_of[j]], j) : j;
    for (size_t e = run_start[run_of[j]]; e < j; e++) {  // the compare over the columns against the exact-size values
      const uint32_t x = idx[e], y = idx[j];
      bool same = value_equal(sig_val[x], sig_lens[x], sig_val[y], sig_lens[y], stride);
      if (chained) same = same && value_equal(prev_val[x], prev_lens[x], prev_val[y], prev_lens[y], stride);
      if (same != rows_equal(c, x, y)) return 2;
    }
  }
  auto valid = [&](size_t j) { return verdict[idx[j]] && row_verifiable(c, idx[j], want); };
  std::vector<size_t> chosen(run_start.size(), (size_t)-1);
  for (size_t j = 0; j < m; j++)
    if (rep[j] == j && valid(j) && chosen[run_of[j]] == (size_t)-1) chosen[run_of[j]] = j;
  for (size_t j = 0; j < m; j++) {
    const size_t pick = chosen[run_of[j]];
    if (rep[j] != j) status[idx[j]] = dup_status(valid(rep[j]));
    else status[idx[j]] = rep_status(valid(j), pick == j, valid(j) && pick != j && repeats_earlier(c, idx.data(), run_start[run_of[j]], j));
  }
  printf("S");
  for (uint32_t i = 0; i < n; i++) printf(" %u", status[i]);
  printf("\n");
  bool have = has_anchor != 0;
  uint64_t before = b.anchor_round;
  const uint8_t* before_sig = anchor_sig;
  uint32_t before_len = anchor_len;
  for (size_t r = 0; r < chosen.size(); r++) {
    if (chosen[r] == (size_t)-1) continue;
    const uint32_t i = idx[chosen[r]];
    bool differs = false;
    if (chained && have && rounds[i] == before + 1)
      differs = prev_lens[i] != before_len || prev_lens[i] > stride || !value_equal(prevs + (size_t)i * stride, before_len, before_sig, before_len, before_len);
    printf("O %llu %u %u\n", (unsigned long long)rounds[i], i, row_flags(rounds[i], have, before, chained != 0, differs));
    have = true;
    before = rounds[i];
    before_sig = sigs + (size_t)i * stride;
    before_len = sig_lens[i];
  }
  for (uint32_t i = 0; i < n; i++) {
    free(sig_val[i]);
    free(prev_val[i]);
  }
  free(sigs);
  free(prevs);
  free(anchor_sig);
  fclose(in);
  return 0;
}
