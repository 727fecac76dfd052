// lgs_table_tail.h -- the two small blocks that end an SSTable, assembled on
// the host (lgs_table_tail.cpp; plain C++, no HIP).
#pragma once

#include <stddef.h>
#include <stdint.h>

namespace lgs {

constexpr size_t kMetaindexMax = 160;   // one "filter.<name>" entry + restarts
constexpr size_t kFooterSize = 48;      // LDB_FOOTER_SIZE (format.h:31)

// The raw metaindex block (table_builder.c:301-328; block_builder.c:91-151):
// no entry, or (filter_name != null) filter_name -> the filter block's handle
// (ldb_handle_export, format.c:45-63).  Returns its length, 0 when cap is too
// small.
size_t tail_metaindex(uint8_t* out, size_t cap, const char* filter_name, uint64_t filter_off,
                      uint64_t filter_size);

// The footer (format.c:92-106): both handles, zero padding to 40 bytes, the
// table magic (format.h:26).
void tail_footer(uint8_t out[kFooterSize], uint64_t meta_off, uint64_t meta_size,
                 uint64_t index_off, uint64_t index_size);

}  // namespace lgs
