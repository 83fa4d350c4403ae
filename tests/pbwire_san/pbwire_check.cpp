// Stand-alone host driver of the protobuf record parser in drand_amd/csrc/pbwire.hpp for the sanitizer build
// (tests/pbwire_san/Makefile, run by tests/test_packet_host.py): pbwire_parse, the call the packet kernels make, over
// records in exact-size heap buffers, so that any read outside the record is an AddressSanitizer report.
//   pbwire_check CORPUS      CORPUS = records {kind u8, length u32 LE, record bytes}; one output line per record:
//                            "C <round> <signature hex or -> <previous_signature hex or -> <randomness hex or -> <metadata
//                            present 0|1> <beaconID hex or ->" (canonical) or "D" (deferred)
//   pbwire_check -f FILE     the varint-delimited walk over a whole buffer: "<offset> <length>" per record, then
//                            "consumed <n>"; run twice, with room for every record and with room for none
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

#include "../../drand_amd/csrc/pbwire.hpp"

using namespace dh::bolt;

static std::string hex(const view& v, uint32_t off, uint32_t len) {
  static const char* d = "0123456789abcdef";
  std::string s;
  for (uint32_t k = 0; k < len; k++) {
    s += d[v.p[off + k] >> 4];
    s += d[v.p[off + k] & 15];
  }
  return s.empty() ? "-" : s;
}

static int framing(const char* path) {
  FILE* fp = fopen(path, "rb");
  if (!fp) {
    perror(path);
    return 2;
  }
  fseek(fp, 0, SEEK_END);
  const long len = ftell(fp);
  fseek(fp, 0, SEEK_SET);
  uint8_t* buf = (uint8_t*)malloc(len ? len : 1);
  if (len && fread(buf, 1, len, fp) != (size_t)len) return 2;
  fclose(fp);
  const view f{buf, (uint64_t)len};
  uint64_t consumed = 0, consumed0 = 0;
  const uint64_t n = pb_frame_delimited(f, nullptr, nullptr, 0, &consumed0);  // the counting call writes nothing
  std::vector<uint64_t> off(n ? n : 1);
  std::vector<uint32_t> ln(n ? n : 1);
  if (pb_frame_delimited(f, off.data(), ln.data(), n, &consumed) != n || consumed != consumed0) {
    fprintf(stderr, "the two walks disagree\n");
    return 3;
  }
  for (uint64_t i = 0; i < n; i++) printf("%llu %u\n", (unsigned long long)off[i], ln[i]);
  printf("consumed %llu\n", (unsigned long long)consumed);
  free(buf);
  return 0;
}

int main(int argc, char** argv) {
  if (argc == 3 && !strcmp(argv[1], "-f")) return framing(argv[2]);
  if (argc != 2) return 2;
  FILE* fp = fopen(argv[1], "rb");
  if (!fp) {
    perror(argv[1]);
    return 2;
  }
  for (;;) {
    uint8_t hdr[5];
    if (fread(hdr, 1, 5, fp) != 5) break;
    uint32_t len = 0;
    for (int i = 4; i >= 1; i--) len = (len << 8) | hdr[i];
    // an exact-size heap buffer: one byte past the end is a sanitizer report
    uint8_t* buf = (uint8_t*)malloc(len ? len : 1);
    if (len && fread(buf, 1, len, fp) != len) return 2;
    const view v{buf, len};
    pbrec r;
    if (pbwire_parse(hdr[0], v, &r)) {
      printf("C %llu %s %s %s %u %s\n", (unsigned long long)r.round, hex(v, r.sig_off, r.sig_len).c_str(), hex(v, r.prev_off, r.prev_len).c_str(),
             hex(v, r.rand_off, r.rand_len).c_str(), r.has_meta, hex(v, r.id_off, r.id_len).c_str());
    } else {
      if (r.round | r.sig_off | r.sig_len | r.prev_off | r.prev_len | r.rand_off | r.rand_len | r.id_off | r.id_len | r.has_meta) {
        fprintf(stderr, "a deferred record left fields behind\n");
        return 3;
      }
      printf("D\n");
    }
    free(buf);
  }
  fclose(fp);
  return 0;
}
