// Assembling one chain from unordered candidate records: the row compare, the class of a sorted
// candidate, the status bits and the output-row flags, shared by k_assemble.hip and the host (tests/assemble_san runs
// it unchanged under sanitizers). Host- and device-compilable, no heap, no state. A value is read over
// min(length, stride) bytes of its row and never behind them.
#pragma once
#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define DH_AS_HD __host__ __device__
#else
#define DH_AS_HD
#endif

namespace dh {
namespace assemble {

enum : uint32_t { AS_CHOSEN = 1, AS_DUPLICATE = 2, AS_INVALID = 4, AS_STALE = 8, AS_SKIPPED = 16, AS_CONFLICT = 32 };
enum : uint32_t { AS_GAP = 1, AS_LINK = 2 };
// a candidate is compared with the first LOOKBACK entries of its round's run
constexpr uint32_t ASSEMBLE_LOOKBACK = 16;

struct cols {  // the candidates' columns; prevs / prev_lens NULL together (the unchained schemes), skip nullable
  const uint64_t* rounds;
  const uint8_t* sigs;
  const uint32_t* sig_lens;
  const uint8_t* prevs;
  const uint32_t* prev_lens;
  const uint8_t* skip;
  uint32_t sig_stride, prev_stride;
};

struct bounds {  // the anchor's round and up_to, each with its "given" flag
  uint64_t anchor_round, up_to;
  uint32_t has_anchor, has_up_to;
};

// rules 1 and 2: AS_SKIPPED, AS_STALE or 0 (the candidate goes on to the sort)
DH_AS_HD inline uint32_t pre_status(uint64_t round, bool skip, const bounds& b) {
  if (skip) return AS_SKIPPED;
  if (round == 0 || (b.has_anchor && round <= b.anchor_round) || (b.has_up_to && round > b.up_to)) return AS_STALE;
  return 0;
}

// two values: the same length and the same bytes (a value longer than its stride has no bytes in its row: the lengths decide)
DH_AS_HD inline bool value_equal(const uint8_t* a, uint32_t la, const uint8_t* b, uint32_t lb, uint32_t stride) {
  if (la != lb) return false;
  const uint32_t k = la < stride ? la : stride;
  uint32_t diff = 0;
  for (uint32_t i = 0; i < k; i++) diff |= (uint32_t)(a[i] ^ b[i]);
  return diff == 0;
}

// rule 3's compare of candidates i and k of one round: whole signature rows and, chained, whole prev rows
DH_AS_HD inline bool rows_equal(const cols& c, size_t i, size_t k) {
  if (!value_equal(c.sigs + i * (size_t)c.sig_stride, c.sig_lens[i], c.sigs + k * (size_t)c.sig_stride, c.sig_lens[k], c.sig_stride))
    return false;
  if (!c.prevs) return true;
  return value_equal(c.prevs + i * (size_t)c.prev_stride, c.prev_lens[i], c.prevs + k * (size_t)c.prev_stride, c.prev_lens[k],
                     c.prev_stride);
}

// The class of sorted entry j, whose round's run starts at sorted entry run_start (idx: sorted entry -> candidate): the
// lowest of the run's first ASSEMBLE_LOOKBACK entries before j that equals it, or j itself (a representative). The
// entry returned is always a representative: had it matched an earlier entry of the window, so would j.
DH_AS_HD inline size_t class_of(const cols& c, const uint32_t* idx, size_t run_start, size_t j) {
  size_t end = run_start + ASSEMBLE_LOOKBACK;
  if (end > j) end = j;
  for (size_t e = run_start; e < end; e++)
    if (rows_equal(c, idx[e], idx[j])) return e;
  return j;
}

// A valid representative j that is not the chosen one of its run: does an earlier entry of the run hold the same rows?
// Then it is a copy the lookback (or DRANDHIP_ASSEMBLE_DEDUPE=0) left un-collapsed, else a second valid signature of
// the round. The chosen entry lies before j, so honest copies end the walk there.
DH_AS_HD inline bool repeats_earlier(const cols& c, const uint32_t* idx, size_t run_start, size_t j) {
  for (size_t e = run_start; e < j; e++)
    if (rows_equal(c, idx[e], idx[j])) return true;
  return false;
}

// rule 4's checks in front of the verifier: the verdict of a row that fails them is not read
DH_AS_HD inline bool row_verifiable(const cols& c, size_t i, uint32_t want_sig_len) {
  if (c.sig_lens[i] != want_sig_len || want_sig_len > c.sig_stride) return false;
  return !c.prevs || c.prev_lens[i] <= c.prev_stride;
}

// rules 3 to 5: a representative's bits (repeats: repeats_earlier, read only when it is valid and not the chosen
// one), and a duplicate's
DH_AS_HD inline uint32_t rep_status(bool valid, bool is_chosen, bool repeats) {
  if (!valid) return AS_INVALID;
  if (is_chosen) return AS_CHOSEN;
  return repeats ? AS_DUPLICATE : AS_CONFLICT;
}
DH_AS_HD inline uint32_t dup_status(bool rep_valid) { return AS_DUPLICATE | (rep_valid ? 0u : (uint32_t)AS_INVALID); }

// rule 6: the flags of an output row of round `round` behind a row of round `before` (have_before: there is such a
// row or an anchor); link_differs: chained, its own prev against that row's signature
DH_AS_HD inline uint32_t row_flags(uint64_t round, bool have_before, uint64_t before, bool chained, bool link_differs) {
  if (!have_before) return 0;
  if (round != before + 1) return AS_GAP;  // before < round, so before + 1 does not wrap
  return chained && link_differs ? (uint32_t)AS_LINK : 0u;
}

}  // namespace assemble
}  // namespace dh
