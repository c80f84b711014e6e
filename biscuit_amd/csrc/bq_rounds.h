// bq_rounds.h -- rounds: what the tile codecs' entry points share (kernels_jpeg / j2k / jpeg_encode / png_encode.hip, through
// bq_ctx.h).  Plain C++, so that a host program can check it (tests/png_encode_selfcheck.cpp).
// A call over n items whose scratch holds fewer works in rounds.  Items a round: as many as scratch_bytes holds at per_item
// bytes each, 32768 at most (a grid counts a round's items in y), rounded down to a multiple of `align` (1 or a power of two:
// a kernel that takes a workgroup's items together) once there are that many.  0: the scratch is smaller than one item's.
#pragma once
#include <stddef.h>

inline size_t round_items(size_t scratch_bytes, size_t per_item, size_t align) {
    size_t m = scratch_bytes / per_item;
    if (m > 32768) m = 32768;
    if (m >= align) m &= ~(align - 1);
    return m;
}
// the items of the round that a *_scratch_bytes function sizes scratch for: the whole call, or the tool's ROUND
inline size_t round_cap(int n, int round) { return (size_t)(n < round ? n : round); }
