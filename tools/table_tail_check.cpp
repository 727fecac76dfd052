// table_tail_check.cpp -- stand-alone check of lcdb_amd/csrc/lgs_table_tail.cpp
// (the host-assembled metaindex block and footer of lgs_table_build_host),
// meant to be built with the host sanitizers; no GPU, not a pytest:
//
//   g++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all
//       tools/table_tail_check.cpp lcdb_amd/csrc/lgs_table_tail.cpp -o table_tail_check
//   ./table_tail_check
//
// Expected bytes are written out by hand from the formats (block_builder.c:
// 91-151, format.c:45-63, 92-106); output buffers are heap blocks of the
// exact size, so a byte written past the stated length is reported.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../lcdb_amd/csrc/lgs_table_tail.h"

static int failures = 0;

static void expect(bool ok, const char* what) {
  if (!ok) {
    fprintf(stderr, "FAIL: %s\n", what);
    ++failures;
  }
}

static std::vector<uint8_t> varint(uint64_t v) {
  std::vector<uint8_t> o;
  while (v >= 128) {
    o.push_back((uint8_t)(v | 128));
    v >>= 7;
  }
  o.push_back((uint8_t)v);
  return o;
}

int main() {
  const char name[] = "filter.leveldb.BuiltinBloomFilter2";
  // No filter: the empty block, restart array {0} and its count.
  {
    std::vector<uint8_t> buf(8);
    const uint8_t want[8] = {0, 0, 0, 0, 1, 0, 0, 0};
    expect(lgs::tail_metaindex(buf.data(), buf.size(), nullptr, 0, 0) == 8, "empty length");
    expect(memcmp(buf.data(), want, 8) == 0, "empty bytes");
    std::vector<uint8_t> small(7);
    expect(lgs::tail_metaindex(small.data(), small.size(), nullptr, 0, 0) == 0, "empty, no room");
  }
  // One entry, handles from one-byte to ten-byte varints.
  const uint64_t vals[] = {0, 1, 127, 128, 300, 0x1234, 1ull << 32, (1ull << 63) + 5, ~0ull - 1};
  for (uint64_t off : vals)
    for (uint64_t size : vals) {
      std::vector<uint8_t> want = {0, (uint8_t)strlen(name), 0};
      const std::vector<uint8_t> a = varint(off), b = varint(size);
      want[2] = (uint8_t)(a.size() + b.size());
      want.insert(want.end(), name, name + strlen(name));
      want.insert(want.end(), a.begin(), a.end());
      want.insert(want.end(), b.begin(), b.end());
      const uint8_t tail[8] = {0, 0, 0, 0, 1, 0, 0, 0};
      want.insert(want.end(), tail, tail + 8);
      std::vector<uint8_t> buf(lgs::kMetaindexMax);
      const size_t n = lgs::tail_metaindex(buf.data(), buf.size(), name, off, size);
      expect(n == want.size() && memcmp(buf.data(), want.data(), n) == 0, "metaindex entry");
      // The footer: four varints, zeros to 40 bytes, the magic.
      std::vector<uint8_t> foot(lgs::kFooterSize);
      lgs::tail_footer(foot.data(), off, size, size, off);
      std::vector<uint8_t> f;
      for (uint64_t v : {off, size, size, off}) {
        const std::vector<uint8_t> e = varint(v);
        f.insert(f.end(), e.begin(), e.end());
      }
      f.resize(40, 0);
      const uint8_t magic[8] = {0x57, 0xfb, 0x80, 0x8b, 0x24, 0x75, 0x47, 0xdb};
      f.insert(f.end(), magic, magic + 8);
      expect(memcmp(foot.data(), f.data(), 48) == 0, "footer");
    }
  // A name that cannot be a one-byte length, and a buffer one byte short.
  {
    std::vector<char> longname(200, 'x');
    longname.back() = 0;
    std::vector<uint8_t> buf(512);
    expect(lgs::tail_metaindex(buf.data(), buf.size(), longname.data(), 1, 1) == 0, "long name");
    std::vector<uint8_t> tight(3 + strlen(name) + 20 + 8 - 1);
    expect(lgs::tail_metaindex(tight.data(), tight.size(), name, 1, 1) == 0, "tight buffer");
  }
  printf("table_tail_check: %s\n", failures ? "FAILED" : "ok");
  return failures ? 1 : 0;
}
