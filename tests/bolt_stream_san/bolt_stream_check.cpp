// Stand-alone driver of the windowed writer's layout code in drand_amd/csrc/bolt_write.hpp for the
// sanitizer build: a record list and a window size in; head, runs and tail of the trimmed store out, concatenated. The
// rows are taken `window` at a time through the shared functions alone (plan_window, leaf_offsets, leaf_dword over
// cols2, finish_tail); every run, the tail, the head, a window's columns and the two carry sets are exact-size heap
// allocations, so a read or write one byte outside is a report.
//   bolt_stream_check <records> <image out> <window>
// records: u32 page size, u32 n, then n x {u64 round, u32 length, value bytes}, little-endian, ascending rounds.
// Prints "OK <rows> <leaves> <pages> <appends that closed no leaf>" or "ERR <why>".
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <vector>

#include "../../drand_amd/csrc/bolt_write.hpp"

using namespace dh::boltw;

static bool read_all(const char* path, std::vector<uint8_t>* out) {
  FILE* f = fopen(path, "rb");
  if (!f) return false;
  uint8_t buf[65536];
  size_t k;
  while ((k = fread(buf, 1, sizeof buf, f)) > 0) out->insert(out->end(), buf, buf + k);
  fclose(f);
  return true;
}

struct rowset {  // exact-size columns; stride = roundup4 of the longest value for a carry, the longest value for a window
  std::unique_ptr<uint64_t[]> rounds;
  std::unique_ptr<uint32_t[]> lens;
  std::unique_ptr<uint8_t[]> rows;
  size_t n = 0, stride = 0;
  void alloc(size_t rows_n, size_t s) {
    n = rows_n;
    stride = s;
    rounds.reset(new uint64_t[n]);
    lens.reset(new uint32_t[n]);
    rows.reset(new uint8_t[n * stride]);
  }
  cols view() const { return cols{rounds.get(), rows.get(), stride, lens.get()}; }
};

struct writer {
  uint32_t P;
  rowset carry[2];
  int cur = 0;
  uint64_t next_page = FIRST_LEAF_PAGE, rows = 0, idle = 0;
  std::vector<uint64_t> keys, pgids;
  std::vector<uint8_t> file;  // the runs, then the tail: file offset 4 * P onwards

  // rows [0, w.n) appended (final: nothing follows); the run goes to the end of `file`
  bool append(const rowset& w, bool final) {
    const rowset& old = carry[cur];
    const cols2 c{old.view(), w.view(), old.n};
    const uint64_t m = old.n + w.n;
    std::unique_ptr<uint32_t[]> sums(new uint32_t[m + 1]);
    sums[0] = 0;
    for (uint64_t i = 0; i < m; i++) sums[i + 1] = sums[i] + 24 + c.len(i);
    const window_plan sized = plan_window(sums.get(), m, P, next_page, final, nullptr, 0);
    std::unique_ptr<leaf_desc[]> leaves(new leaf_desc[sized.leaves]);
    const window_plan pl = plan_window(sums.get(), m, P, next_page, final, leaves.get(), sized.leaves);
    if (pl.leaves != sized.leaves || pl.open_row != sized.open_row || pl.next_page != sized.next_page) return false;
    if (final && pl.open_row != m) return false;
    if (m - pl.open_row > MAX_LEAF_RECS) return false;
    const size_t bytes = (size_t)(pl.next_page - next_page) * P;
    std::unique_ptr<uint8_t[]> run(new uint8_t[bytes]);
    memset(run.get(), 0xA5, bytes);  // every byte is written below
    for (uint64_t k = 0; k < pl.leaves; k++) {
      const leaf_desc& L = leaves[k];
      std::unique_ptr<uint32_t[]> offs;
      if (L.vlen == MIXED) {
        if (L.n > MAX_LEAF_RECS) return false;
        offs.reset(new uint32_t[L.n + 1]);
        leaf_offsets(L, c, offs.get());
      }
      uint8_t* out = run.get() + (L.page - next_page) * P;
      const uint32_t ndw = L.span * (P / 4);
      for (uint32_t d = 0; d < ndw; d++) wr32(out + 4 * (size_t)d, leaf_dword(L, c, offs.get(), d));
      keys.push_back(c.round(L.row0));
      pgids.push_back(L.page);
    }
    // the open leaf's rows, into the other carry set at stride roundup4 of the longest of them
    uint32_t longest = 0;
    for (uint64_t i = pl.open_row; i < m; i++) longest = c.len(i) > longest ? c.len(i) : longest;
    if (16 + (uint64_t)(uint32_t)(sums[m] - sums[pl.open_row]) > P && pl.open_row < m) return false;
    rowset& nxt = carry[cur ^ 1];
    nxt.alloc(m - pl.open_row, (longest + 3) & ~3u);
    for (uint64_t i = pl.open_row; i < m; i++) {
      const size_t j = i - pl.open_row;
      nxt.rounds[j] = c.round(i);
      nxt.lens[j] = c.len(i);
      for (uint32_t o = 0; o < nxt.stride; o++) nxt.rows[j * nxt.stride + o] = o < c.len(i) ? c.byte(i, o) : 0;
    }
    carry[cur].alloc(0, 0);
    cur ^= 1;
    file.insert(file.end(), run.get(), run.get() + bytes);
    next_page = pl.next_page;
    rows += w.n;
    idle += !final && !pl.leaves;
    return true;
  }
};

int main(int argc, char** argv) {
  if (argc != 4) return 2;
  std::vector<uint8_t> in;
  if (!read_all(argv[1], &in) || in.size() < 8) return 2;
  const unsigned long long window = strtoull(argv[3], nullptr, 10);
  uint32_t P, n;
  memcpy(&P, in.data(), 4);
  memcpy(&n, in.data() + 4, 4);
  if (!page_size_ok(P) || !n || !window) {
    printf("ERR arguments\n");
    return 0;
  }
  std::vector<uint64_t> rounds(n);
  std::vector<uint32_t> lens(n);
  std::vector<size_t> at(n);
  size_t o = 8;
  for (uint32_t i = 0; i < n; i++) {
    if (o + 12 > in.size()) return 2;
    memcpy(&rounds[i], in.data() + o, 8);
    memcpy(&lens[i], in.data() + o + 8, 4);
    o += 12;
    at[i] = o;
    if (lens[i] > in.size() - o) return 2;
    o += lens[i];
    if (i && rounds[i - 1] >= rounds[i]) {
      printf("ERR order\n");
      return 0;
    }
  }
  writer w;
  w.P = P;
  w.carry[0].alloc(0, 0);
  w.carry[1].alloc(0, 0);
  for (size_t i0 = 0; i0 < n; i0 += window) {
    const size_t k = n - i0 < window ? n - i0 : (size_t)window;
    uint32_t longest = 0;
    for (size_t i = 0; i < k; i++) longest = lens[i0 + i] > longest ? lens[i0 + i] : longest;
    rowset cut;  // no padding: a read past a value's length leaves the buffer at the last row
    cut.alloc(k, longest);
    for (size_t i = 0; i < k; i++) {
      cut.rounds[i] = rounds[i0 + i];
      cut.lens[i] = lens[i0 + i];
      memcpy(cut.rows.get() + i * cut.stride, in.data() + at[i0 + i], lens[i0 + i]);
    }
    if (!w.append(cut, false)) {
      printf("ERR append at row %zu\n", i0);
      return 0;
    }
  }
  rowset none;
  none.alloc(0, 0);
  if (!w.append(none, true)) {  // finish: the open leaf is closed
    printf("ERR finish\n");
    return 0;
  }
  const size_t nl = w.keys.size();
  const uint64_t leaf_end = w.next_page, pages = leaf_end + branch_pages(nl, P);
  const size_t tail_bytes = (size_t)(pages - leaf_end) * P;
  std::unique_ptr<uint8_t[]> tail(new uint8_t[tail_bytes]), head(new uint8_t[4 * (size_t)P]);
  memset(tail.get(), 0xA5, tail_bytes);
  memset(head.get(), 0xA5, 4 * (size_t)P);
  std::unique_ptr<uint64_t[]> keys(new uint64_t[nl]), pgids(new uint64_t[nl]);
  memcpy(keys.get(), w.keys.data(), nl * 8);
  memcpy(pgids.get(), w.pgids.data(), nl * 8);
  finish_tail(tail.get(), head.get(), P, pages, leaf_end, keys.get(), pgids.get(), nl);
  FILE* f = fopen(argv[2], "wb");
  if (!f || fwrite(head.get(), 1, 4 * (size_t)P, f) != 4 * (size_t)P || fwrite(w.file.data(), 1, w.file.size(), f) != w.file.size() ||
      fwrite(tail.get(), 1, tail_bytes, f) != tail_bytes)
    return 2;
  fclose(f);
  printf("OK %llu %zu %llu %llu\n", (unsigned long long)w.rows, nl, (unsigned long long)pages, (unsigned long long)w.idle);
  return 0;
}
