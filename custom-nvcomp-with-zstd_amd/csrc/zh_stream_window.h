// zh_stream_window.h — the index arithmetic of a stream window's advance (zh_window_update_kernel,
// zh_stream.hip): what to keep of the old window, what to take of the chunk, and how a copy splits
// into ragged ends and an aligned middle.  Plain C++, no HIP types: tests/cpp/prefix_plan_check.cpp
// checks it on the host against a byte loop.
#pragma once
#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define ZH_SW_HD __host__ __device__ inline
#else
#define ZH_SW_HD inline
#endif

#define ZH_STREAM_WINDOW 65536u  // bytes of stream a window holds: what the matchers can stage (ZH_BLOCK_MAX, ZH_DEEP_PRE)

// The next window = old[keep_from, keep_from + keep) ++ chunk[take_from, take_from + take): the
// last <= W bytes of (old window of len bytes) ++ (chunk of n bytes).  len <= W.
struct ZhWindowMove {
  uint64_t keep_from, keep, take_from, take;
};
ZH_SW_HD ZhWindowMove zh_window_move(uint64_t len, uint64_t n, uint64_t W) {
  ZhWindowMove m;
  m.take = n < W ? n : W;
  m.keep = len < W - m.take ? len : W - m.take;
  m.keep_from = len - m.keep;
  m.take_from = n - m.take;
  return m;
}

// A copy of n bytes to address dst: head single bytes up to dst's next 16-byte boundary, then vec
// 16-byte pieces (stores aligned), then tail single bytes.  head + 16 * vec + tail == n.
struct ZhCopySplit {
  uint64_t head, vec, tail;
};
ZH_SW_HD ZhCopySplit zh_copy_split(uintptr_t dst, uint64_t n) {
  ZhCopySplit s;
  uint64_t const to_boundary = (uint64_t)((16u - (dst & 15u)) & 15u);
  s.head = to_boundary < n ? to_boundary : n;
  s.vec = (n - s.head) / 16u;
  s.tail = n - s.head - 16u * s.vec;
  return s;
}
