// The image of a trimmed bbolt beacon store (chain/boltdb/trimmed.go:87-107: bucket "beacons", key = round as 8 bytes
// big-endian, value = the raw signature, leaves packed full as bucket.FillPercent = 1.0 intends), laid out from the
// verifier's columns {rounds u64[n], rows u8[n, stride], lens u32[n]}. Shared by the host (plain g++)
// and the device like bolt.hpp, whose page format comment applies; no heap, no state. What decides where a byte goes
// is here and nowhere else: the leaf plan, leaf_dword (dword w of a leaf's extent), and the branch / root-leaf /
// freelist / meta page writers with their checksum.
//
// Page plan: 0, 1 meta (txid 3 and 2), 2 an empty freelist, 3 the root bucket's leaf {"beacons" -> bucket root}, the
// bucket's leaves from page 4 in key order, then branch levels of (P - 16) / 24 children up to one root (a single leaf
// is the root). A record needs 16 + 8 + vsize bytes; a leaf is closed when 16 + the sum would pass P; a record that
// alone passes P gets a leaf of its own with overflow pages.
#pragma once
#include <stdint.h>

#ifndef BOLT_HD
#if defined(__HIPCC__)
#define BOLT_HD __host__ __device__ inline
#else
#define BOLT_HD inline
#endif
#endif

namespace dh {
namespace boltw {

constexpr uint32_t MAGIC = 0xED0CDAEDu;
constexpr uint32_t MIXED = 0xFFFFFFFFu;      // leaf_desc.vlen: the leaf's values differ in length
constexpr uint32_t MAX_LEAF_RECS = 2730;     // (65536 - 16) / 24: the records of a leaf of more than one record
constexpr uint64_t FIRST_LEAF_PAGE = 4;

BOLT_HD bool page_size_ok(uint32_t P) { return P >= 256 && P <= 65536 && !(P & (P - 1)); }
BOLT_HD uint32_t branch_fan(uint32_t P) { return (P - 16) / 24; }

BOLT_HD uint64_t fnv64a(const uint8_t* p, uint32_t n) {
  uint64_t h = 0xcbf29ce484222325ull;
  for (uint32_t i = 0; i < n; i++) h = (h ^ p[i]) * 0x100000001b3ull;
  return h;
}

BOLT_HD void wr16(uint8_t* p, uint32_t v) {
  p[0] = (uint8_t)v;
  p[1] = (uint8_t)(v >> 8);
}
BOLT_HD void wr32(uint8_t* p, uint32_t v) {
  wr16(p, v);
  wr16(p + 2, v >> 16);
}
BOLT_HD void wr64(uint8_t* p, uint64_t v) {
  wr32(p, (uint32_t)v);
  wr32(p + 4, (uint32_t)(v >> 32));
}
BOLT_HD void wr64be(uint8_t* p, uint64_t v) {
  for (int i = 0; i < 8; i++) p[i] = (uint8_t)(v >> (8 * (7 - i)));
}
BOLT_HD void zero(uint8_t* p, uint32_t n) {
  for (uint32_t i = 0; i < n; i++) p[i] = 0;
}
BOLT_HD void page_head(uint8_t* pg, uint64_t pgid, uint32_t flags, uint32_t count, uint32_t overflow) {
  wr64(pg, pgid);
  wr16(pg + 8, flags);
  wr16(pg + 10, count);
  wr32(pg + 12, overflow);
}

// ---- the leaf plan

// One leaf of the bucket (24 bytes): rows [row0, row0 + n) on pages [page, page + span).
struct leaf_desc {
  uint64_t page;
  uint32_t row0, n, span;
  uint32_t vlen;  // the common value length, MIXED when the values differ
};
static_assert(sizeof(leaf_desc) == 24, "leaf plan record");

// The greedy leaf that starts at row s < n. `sums` is the exclusive sum of the record sizes 24 + lens[i] (n + 1 words,
// modulo 2^32: only differences of neighbours are used, and a record size is below 2^32). Returns the rows taken.
BOLT_HD uint32_t plan_leaf(const uint32_t* sums, uint64_t n, uint64_t s, uint32_t P, uint64_t page, leaf_desc* out) {
  const uint32_t need0 = sums[s + 1] - sums[s];
  uint64_t size = 16 + (uint64_t)need0;
  uint32_t k = 1, vlen = need0 - 24;
  while (s + k < n) {
    const uint32_t need = sums[s + k + 1] - sums[s + k];
    if (size + need > P) break;
    size += need;
    if (need != need0) vlen = MIXED;
    k++;
  }
  out->page = page;
  out->row0 = (uint32_t)s;
  out->n = k;
  out->span = (uint32_t)((size + P - 1) / P);
  out->vlen = vlen;
  return k;
}

// The same leaf when rows [0, m) are a window of a longer list: the rows taken when the leaf is
// certainly closed, 0 while it is open. Closed means a following record is known not to fit: one follows in the window
// and did not fit, or no record of at least 24 bytes fits any more (a record with 16 + need > P is such a leaf of its
// own, as is a leaf filled to the last 23 bytes), or `final`: nothing follows. An open leaf therefore holds at most
// P - 24 bytes, i.e. fewer than MAX_LEAF_RECS rows: the bound of what a writer carries to its next window.
BOLT_HD uint32_t plan_leaf_window(const uint32_t* sums, uint64_t m, uint64_t s, uint32_t P, uint64_t page, bool final, leaf_desc* out) {
  const uint32_t k = plan_leaf(sums, m, s, P, page, out);
  if (final || s + k < m) return k;
  const uint64_t size = 16 + (uint64_t)(uint32_t)(sums[s + k] - sums[s]);  // exact: k > 1 keeps it within P, k = 1 below 2^32
  return size + 24 > P ? k : 0;
}

struct window_plan {
  uint64_t leaves;     // leaves closed by this window
  uint64_t open_row;   // first row of the open leaf (m when none is open): rows [open_row, m) are carried
  uint64_t next_page;  // the page of the next leaf
};
// The windowed leaf plan over rows [0, m) = (carried rows || new rows), the next leaf going to `page`. The closed
// leaves are written to out[0, cap) in order; those beyond cap are counted only, so a call with cap 0 sizes.
BOLT_HD window_plan plan_window(const uint32_t* sums, uint64_t m, uint32_t P, uint64_t page, bool final, leaf_desc* out, uint64_t cap) {
  window_plan w{0, 0, page};
  while (w.open_row < m) {
    leaf_desc L;
    const uint32_t k = plan_leaf_window(sums, m, w.open_row, P, w.next_page, final, &L);
    if (!k) break;
    if (w.leaves < cap) out[w.leaves] = L;
    w.leaves++;
    w.open_row += k;
    w.next_page += L.span;
  }
  return w;
}

// ---- a leaf's bytes

// the columns the records come from
struct cols {
  const uint64_t* rounds;
  const uint8_t* rows;
  uint64_t stride;
  const uint32_t* lens;
  BOLT_HD uint64_t round(uint64_t i) const { return rounds[i]; }
  BOLT_HD uint32_t len(uint64_t i) const { return lens[i]; }
  BOLT_HD uint8_t byte(uint64_t i, uint32_t o) const { return rows[i * stride + o]; }
};

// Two row segments read as one list: rows below n_carry are the writer's carried rows, row i from
// n_carry on is row i - n_carry of the caller's columns; each segment has its own stride.
struct cols2 {
  cols carry, fresh;
  uint64_t n_carry;
  BOLT_HD uint64_t round(uint64_t i) const { return i < n_carry ? carry.rounds[i] : fresh.rounds[i - n_carry]; }
  BOLT_HD uint32_t len(uint64_t i) const { return i < n_carry ? carry.lens[i] : fresh.lens[i - n_carry]; }
  BOLT_HD uint8_t byte(uint64_t i, uint32_t o) const {
    return i < n_carry ? carry.rows[i * carry.stride + o] : fresh.rows[(i - n_carry) * fresh.stride + o];
  }
};

// Data offsets of a MIXED leaf's records behind its element array: offs[i] for record i, offs[n] the end (n + 1 words).
template <class C>
BOLT_HD void leaf_offsets(const leaf_desc& L, const C& c, uint32_t* offs) {
  uint32_t o = 0;
  for (uint32_t i = 0; i < L.n; i++) {
    offs[i] = o;
    o += 8 + c.len((uint64_t)L.row0 + i);
  }
  offs[L.n] = o;
}

// record i's data offset (i <= n); offs is read for a MIXED leaf only
BOLT_HD uint32_t data_off(const leaf_desc& L, const uint32_t* offs, uint32_t i) {
  return L.vlen == MIXED ? offs[i] : i * (8 + L.vlen);
}

// Dword w (little-endian) of the leaf's extent of span * P bytes: the page header {id, flags 0x02, count, overflow},
// element i {flags 0, pos relative to the element, ksize 8, vsize}, then per record key and value, then zeros. The
// element array ends on a dword boundary, so a dword lies in one region; inside the data it may cross records.
template <class C>
BOLT_HD uint32_t leaf_dword(const leaf_desc& L, const C& c, const uint32_t* offs, uint32_t w) {
  if (w < 4) {
    if (w == 0) return (uint32_t)L.page;
    if (w == 1) return (uint32_t)(L.page >> 32);
    if (w == 2) return 0x02u | (L.n << 16);
    return L.span - 1;
  }
  if (w < 4 + 4 * L.n) {
    const uint32_t i = (w - 4) >> 2, f = w & 3;
    if (f == 0) return 0;
    if (f == 1) return 16 * (L.n - i) + data_off(L, offs, i);
    if (f == 2) return 8;
    return data_off(L, offs, i + 1) - data_off(L, offs, i) - 8;
  }
  const uint32_t d = 4 * (w - 4 - 4 * L.n), end = data_off(L, offs, L.n);
  if (d >= end) return 0;
  uint32_t r;  // the record holding byte d
  if (L.vlen != MIXED) {
    r = d / (8 + L.vlen);
  } else {
    uint32_t lo = 0, hi = L.n;  // offs[lo] <= d < offs[hi]
    while (hi - lo > 1) {
      const uint32_t mid = (lo + hi) / 2;
      if (offs[mid] <= d) lo = mid; else hi = mid;
    }
    r = lo;
  }
  uint32_t word = 0, next = data_off(L, offs, r + 1);
  for (uint32_t j = 0; j < 4 && d + j < end; j++) {
    while (d + j >= next) next = data_off(L, offs, ++r + 1);  // a record is at least its 8-byte key
    const uint32_t o = d + j - data_off(L, offs, r);
    const uint64_t row = (uint64_t)L.row0 + r;
    const uint32_t b = o < 8 ? (uint32_t)(c.round(row) >> (8 * (7 - o))) & 0xff : c.byte(row, o - 8);
    word |= b << (8 * j);
  }
  return word;
}

// ---- the other pages; each writes all P bytes of `pg`

// a branch page over n <= branch_fan(P) children: element i {pos, ksize 8, child pgid}, then the keys
BOLT_HD void branch_page(uint8_t* pg, uint32_t P, uint64_t pgid, const uint64_t* keys, const uint64_t* children, uint32_t n) {
  zero(pg, P);
  page_head(pg, pgid, 0x01, n, 0);
  for (uint32_t i = 0; i < n; i++) {
    uint8_t* e = pg + 16 + 16 * i;
    wr32(e, 16 * (n - i) + 8 * i);
    wr32(e + 4, 8);
    wr64(e + 8, children[i]);
    wr64be(pg + 16 + 16 * n + 8 * i, keys[i]);
  }
}

// page 3: the root bucket's leaf, one element {flags 0x01 (bucket), key "beacons", value {root pgid, sequence 0}}
BOLT_HD void root_leaf_page(uint8_t* pg, uint32_t P, uint64_t bucket_root) {
  const char* name = "beacons";
  zero(pg, P);
  page_head(pg, 3, 0x02, 1, 0);
  wr32(pg + 16, 0x01);
  wr32(pg + 20, 16);
  wr32(pg + 24, 7);
  wr32(pg + 28, 16);
  for (int i = 0; i < 7; i++) pg[32 + i] = (uint8_t)name[i];
  wr64(pg + 39, bucket_root);
  wr64(pg + 47, 0);
}

BOLT_HD void freelist_page(uint8_t* pg, uint32_t P) {
  zero(pg, P);
  page_head(pg, 2, 0x10, 0, 0);
}

// meta page `pgid` (0 or 1): root bucket {pgid 3, sequence 0}, freelist 2, high-water mark `pages`
BOLT_HD void meta_page(uint8_t* pg, uint32_t P, uint64_t pgid, uint64_t pages, uint64_t txid) {
  zero(pg, P);
  page_head(pg, pgid, 0x04, 0, 0);
  wr32(pg + 16, MAGIC);
  wr32(pg + 20, 2);
  wr32(pg + 24, P);
  wr32(pg + 28, 0);
  wr64(pg + 32, 3);
  wr64(pg + 40, 0);
  wr64(pg + 48, 2);
  wr64(pg + 56, pages);
  wr64(pg + 64, txid);
  wr64(pg + 72, fnv64a(pg + 16, 56));
}

// Pages of the branch levels over `leaves` leaves (0 for one leaf).
BOLT_HD uint64_t branch_pages(uint64_t leaves, uint32_t P) {
  uint64_t total = 0, level = leaves;
  while (level > 1) {
    level = (level + branch_fan(P) - 1) / branch_fan(P);
    total += level;
  }
  return total;
}

// The branch levels, pages 0, 1, 2 and 3 of a file whose leaf pages are not in memory. keys / pgids hold the first key
// and the page of every leaf on entry (`leaves` >= 1 entries) and are overwritten level by level. leaf_end is the page
// after the last leaf page; `tail` starts there and takes the branch_pages(leaves, P) branch pages, whose page ids stay
// absolute; `head` takes pages 0-3 (4 * P bytes). Returns the bucket's root page.
BOLT_HD uint64_t finish_tail(uint8_t* tail, uint8_t* head, uint32_t P, uint64_t pages, uint64_t leaf_end, uint64_t* keys,
                             uint64_t* pgids, uint64_t leaves) {
  uint64_t nxt = leaf_end, level = leaves;
  const uint32_t fan = branch_fan(P);
  while (level > 1) {
    uint64_t up = 0;
    for (uint64_t i = 0; i < level; i += fan, up++) {
      const uint32_t k = (uint32_t)(level - i < fan ? level - i : fan);
      branch_page(tail + (nxt - leaf_end) * P, P, nxt, keys + i, pgids + i, k);
      keys[up] = keys[i];  // up <= i: the entries read later lie further on
      pgids[up] = nxt++;
    }
    level = up;
  }
  meta_page(head, P, 0, pages, 3);
  meta_page(head + P, P, 1, pages, 2);
  freelist_page(head + 2 * (uint64_t)P, P);
  root_leaf_page(head + 3 * (uint64_t)P, P, pgids[0]);
  return pgids[0];
}

// The same for a whole image (pages * P bytes) whose leaf pages are in place.
BOLT_HD uint64_t finish_image(uint8_t* img, uint32_t P, uint64_t pages, uint64_t leaf_end, uint64_t* keys, uint64_t* pgids,
                              uint64_t leaves) {
  return finish_tail(img + leaf_end * P, img, P, pages, leaf_end, keys, pgids, leaves);
}

}  // namespace boltw
}  // namespace dh
