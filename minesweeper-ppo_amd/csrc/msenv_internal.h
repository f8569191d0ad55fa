// Library-internal view of a handle for the other translation units of libmsenv.so
// (csrc/mssolve.hip, csrc/msposterior.hip). Not part of the C ABI; ms_handle itself stays private to msenv.hip.
#ifndef MSENV_INTERNAL_H
#define MSENV_INTERNAL_H

#include <stdint.h>

#include "../../include/msenv.h"

struct ms_board_view {
  int64_t n;
  int32_t H, W, NW;            // NW packed u64 words per board plane (floor(64/W) rows per word)
  int32_t device;
  const uint64_t* mine_words;  // [n, NW]
  const uint64_t* rev_words;   // [n, NW]
  const uint8_t* meta;         // per-env records, meta_stride bytes apart; the u32 at flags_offset
  int32_t meta_stride;         // has bit 0 = first_click_done
  int32_t flags_offset;
  int32_t* avoid_budget;       // the handle's node budget for ms_avoid (0 = default)
  int32_t mine_count;          // the handle's mines per board
  int32_t* posterior_budget;   // the handle's node budget for ms_posterior (0 = default)
};

int ms_internal_board_view(ms_handle* h, ms_board_view* out);  // h non-null
// records the thread-local ms_last_error() message and returns code
int ms_internal_fail(int code, const char* msg);

#endif  // MSENV_INTERNAL_H
