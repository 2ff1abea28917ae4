// zh_litpack.h — K1's literal compaction of one input dword (host + device, so a CPU test can
// check it: tests/cpp/litpack_check.cpp).  K1's literal extractor (zh_lz.hip lit_rounds) gives a
// lane one aligned dword of the window and its four literal bits; the lane's 0-4 literal bytes
// go, in order, into the low bytes of one register with one v_perm_b32.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define ZH_LP_HD __host__ __device__ inline
#else
#define ZH_LP_HD inline
#endif

// v_perm_b32 selector for the literal bits m4 (bit i = byte i of the dword is a literal), the
// dword being the instruction's second source and zero its first: selector byte k is the index of
// the k-th set bit of m4 (bytes 0-3 of the second source), and past m4's last bit an index 4-7
// (a byte of the first source: zero).  The sentinel bits 4-7 make every lowest-set-bit step
// defined; 14 VALU on the device, no table to load.
ZH_LP_HD constexpr uint32_t zh_litpack_sel(uint32_t m4) {
  uint32_t const a = (m4 & 15u) | 0xF0u, b = a & (a - 1u), c = b & (b - 1u), d = c & (c - 1u);
  return (uint32_t)__builtin_ctz(a) | (uint32_t)__builtin_ctz(b) << 8 | (uint32_t)__builtin_ctz(c) << 16 | (uint32_t)__builtin_ctz(d) << 24;
}

// v_perm_b32 as the hardware computes it, for the selector bytes zh_litpack_sel produces (0-3: a
// byte of s1, 4-7: a byte of s0) and the constants 0x0c (0x00) and >= 0x0d (0xff).
ZH_LP_HD constexpr uint32_t zh_perm_b32_model(uint32_t s0, uint32_t s1, uint32_t sel) {
  uint64_t const src = (uint64_t)s0 << 32 | s1;
  uint32_t r = 0;
  for (uint32_t k = 0; k < 4; k++) {
    uint32_t const s = (sel >> (8 * k)) & 255u;
    uint32_t const byte = s < 8 ? (uint32_t)(src >> (8 * s)) & 255u : s >= 13 ? 255u : 0u;
    r |= byte << (8 * k);
  }
  return r;
}

// The literal bytes of dword w (literal bits m4) in order in the low bytes, zero above them.
ZH_LP_HD uint32_t zh_litpack(uint32_t w, uint32_t m4) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __builtin_amdgcn_perm(0u, w, zh_litpack_sel(m4));
#else
  return zh_perm_b32_model(0u, w, zh_litpack_sel(m4));
#endif
}
