// lgs_table_tail.cpp -- metaindex block and footer of an SSTable
// (table_builder.c:301-365), host only.  Both are under 200 bytes whatever
// the table's size; everything that scales with the table is built on the
// device (lgs_block.hip, lgs_table.hip, lgs_bloom.hip).
#include "lgs_table_tail.h"

#include <string.h>

namespace lgs {
namespace {

uint8_t* put_varint64(uint8_t* p, uint64_t v) {   // coding.h:137-148
  while (v >= 128) {
    *p++ = (uint8_t)(v | 128);
    v >>= 7;
  }
  *p++ = (uint8_t)v;
  return p;
}

uint8_t* put_fixed32(uint8_t* p, uint32_t v) {
  for (int i = 0; i < 4; ++i) *p++ = (uint8_t)(v >> (8 * i));
  return p;
}

}  // namespace

size_t tail_metaindex(uint8_t* out, size_t cap, const char* filter_name, uint64_t filter_off,
                      uint64_t filter_size) {
  uint8_t* p = out;
  if (filter_name) {
    const size_t k = strlen(filter_name);
    // shared | non_shared | value_size, one byte each under 128.
    if (k >= 128 || cap < 3 + k + 20 + 8) return 0;
    uint8_t handle[20];
    const size_t h = (size_t)(put_varint64(put_varint64(handle, filter_off), filter_size) - handle);
    *p++ = 0;                                      // block_builder.c:123-125
    *p++ = (uint8_t)k;
    *p++ = (uint8_t)h;
    memcpy(p, filter_name, k);                     // :128-129
    p += k;
    memcpy(p, handle, h);
    p += h;
  } else if (cap < 8) {
    return 0;
  }
  p = put_fixed32(p, 0);                           // the one restart, :68, :143-146
  p = put_fixed32(p, 1);
  return (size_t)(p - out);
}

void tail_footer(uint8_t out[kFooterSize], uint64_t meta_off, uint64_t meta_size,
                 uint64_t index_off, uint64_t index_size) {
  memset(out, 0, kFooterSize);                     // format.c:100-102
  uint8_t* p = put_varint64(put_varint64(out, meta_off), meta_size);
  put_varint64(put_varint64(p, index_off), index_size);
  const uint64_t magic = 0xdb4775248b80fb57ull;    // LDB_TABLE_MAGIC
  for (int i = 0; i < 8; ++i) out[40 + i] = (uint8_t)(magic >> (8 * i));
}

}  // namespace lgs
