// Stand-alone driver of drand_amd/csrc/bolt_write.hpp for the sanitizer build: a record list in, the whole image of
// the trimmed store out, built through the shared functions alone (plan_leaf, leaf_offsets, leaf_dword, finish_image)
// with every buffer an exact-size heap allocation, so a read or write one byte outside is a report.
//   bolt_write_check <records> <image out>
// records: u32 page size, u32 n, then n x {u64 round, u32 length, value bytes}, little-endian, ascending rounds.
// Prints "OK <rows> <leaves> <pages>" or "ERR <why>".
#include <cstdio>
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

int main(int argc, char** argv) {
  if (argc != 3) return 2;
  std::vector<uint8_t> in;
  if (!read_all(argv[1], &in) || in.size() < 8) return 2;
  uint32_t P, n;
  memcpy(&P, in.data(), 4);
  memcpy(&n, in.data() + 4, 4);
  if (!page_size_ok(P) || !n) {
    printf("ERR arguments\n");
    return 0;
  }
  // the columns, exact size
  std::unique_ptr<uint64_t[]> rounds(new uint64_t[n]);
  std::unique_ptr<uint32_t[]> lens(new uint32_t[n]);
  std::vector<size_t> at(n);
  size_t o = 8;
  uint32_t longest = 0;
  for (uint32_t i = 0; i < n; i++) {
    if (o + 12 > in.size()) return 2;
    memcpy(&rounds[i], in.data() + o, 8);
    memcpy(&lens[i], in.data() + o + 8, 4);
    o += 12;
    at[i] = o;
    if (lens[i] > in.size() - o) return 2;
    o += lens[i];
    if (lens[i] > longest) longest = lens[i];
    if (i && rounds[i - 1] >= rounds[i]) {
      printf("ERR order\n");
      return 0;
    }
  }
  const size_t stride = longest;  // no padding: a read past a value's length leaves the buffer at the last row
  std::unique_ptr<uint8_t[]> rows(new uint8_t[(size_t)n * stride + 1]);
  for (uint32_t i = 0; i < n; i++) memcpy(rows.get() + i * stride, in.data() + at[i], lens[i]);
  const cols c{rounds.get(), rows.get(), stride, lens.get()};
  // the exclusive sum of the record sizes, modulo 2^32 as the device scan leaves it
  std::unique_ptr<uint32_t[]> sums(new uint32_t[(size_t)n + 1]);
  sums[0] = 0;
  for (uint32_t i = 0; i < n; i++) sums[i + 1] = sums[i] + 24 + lens[i];
  std::vector<leaf_desc> leaves;
  uint64_t page = FIRST_LEAF_PAGE;
  for (uint64_t s = 0; s < n;) {
    leaf_desc L;
    s += plan_leaf(sums.get(), n, s, P, page, &L);
    page += L.span;
    leaves.push_back(L);
  }
  const uint64_t pages = page + branch_pages(leaves.size(), P);
  const size_t bytes = (size_t)pages * P;
  std::unique_ptr<uint8_t[]> img(new uint8_t[bytes]);
  memset(img.get(), 0xA5, bytes);  // every byte is written below
  std::unique_ptr<uint64_t[]> keys(new uint64_t[leaves.size()]), pgids(new uint64_t[leaves.size()]);
  for (size_t k = 0; k < leaves.size(); k++) {
    const leaf_desc& L = leaves[k];
    std::unique_ptr<uint32_t[]> offs;
    if (L.vlen == MIXED) {
      if (L.n > MAX_LEAF_RECS) return 3;
      offs.reset(new uint32_t[L.n + 1]);
      leaf_offsets(L, c, offs.get());
    }
    uint8_t* out = img.get() + L.page * P;
    const uint32_t ndw = L.span * (P / 4);
    for (uint32_t w = 0; w < ndw; w++) wr32(out + 4 * (size_t)w, leaf_dword(L, c, offs.get(), w));
    keys[k] = rounds[L.row0];
    pgids[k] = L.page;
  }
  finish_image(img.get(), P, pages, page, keys.get(), pgids.get(), leaves.size());
  FILE* f = fopen(argv[2], "wb");
  if (!f || fwrite(img.get(), 1, bytes, f) != bytes) return 2;
  fclose(f);
  printf("OK %u %zu %llu\n", n, leaves.size(), (unsigned long long)pages);
  return 0;
}
