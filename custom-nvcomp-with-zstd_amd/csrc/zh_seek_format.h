// zh_seek_format.h — the Zstandard seekable format's seek table: sizes, limits, encode and
// validate, shared by the device kernels (zh_seek.hip) and the host (zh_host_seek.cpp's info call on
// a host buffer).  Plain integer code, no HIP calls.
//
//   u32 0x184D2A5E | u32 Frame_Size = N*E + 9 | N x { u32 csize; u32 dsize; [u32 checksum] }
//   | u32 N | u8 descriptor (bit 7 checksums, bits 6..2 reserved 0) | u32 0x8F92EAB1
//
// All little-endian; E = 8 without checksums, 12 with.
#pragma once
#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define ZH_SEEK_HD __host__ __device__ inline
#else
#define ZH_SEEK_HD inline
#endif

#define ZH_SEEK_SKIP_MAGIC 0x184D2A5Eu
#define ZH_SEEK_MAGIC 0x8F92EAB1u
#define ZH_SEEK_MAX_FRAMES 0x8000000ull
#define ZH_SEEK_MAX_FIELD 0x40000000ull
#define ZH_SEEK_FOOTER 9u    // Number_Of_Frames, descriptor, magic
#define ZH_SEEK_OVERHEAD 17u  // skippable header + footer

// nvcomp-style codes used by the seekable calls
enum : uint32_t { ZH_SEEK_OK = 0, ZH_SEEK_INVALID = 2, ZH_SEEK_CORRUPT = 6, ZH_SEEK_TOO_SMALL = 7, ZH_SEEK_CHECKSUM = 10 };

ZH_SEEK_HD uint32_t zh_seek_entry_bytes(int with_checksums) { return with_checksums ? 12u : 8u; }
ZH_SEEK_HD uint64_t zh_seek_table_bytes(uint64_t n, int with_checksums) { return n * zh_seek_entry_bytes(with_checksums) + ZH_SEEK_OVERHEAD; }

ZH_SEEK_HD uint32_t zh_seek_ld32(const uint8_t *p) {
  return (uint32_t)p[0] | (uint32_t)p[1] << 8 | (uint32_t)p[2] << 16 | (uint32_t)p[3] << 24;
}
ZH_SEEK_HD void zh_seek_st32(uint8_t *p, uint32_t v) {
  p[0] = (uint8_t)v;
  p[1] = (uint8_t)(v >> 8);
  p[2] = (uint8_t)(v >> 16);
  p[3] = (uint8_t)(v >> 24);
}

// Header (8 bytes at the table's start) and footer (9 bytes at its end)
ZH_SEEK_HD void zh_seek_write_header(uint8_t *table, uint64_t n, int with_checksums) {
  zh_seek_st32(table, ZH_SEEK_SKIP_MAGIC);
  zh_seek_st32(table + 4, (uint32_t)(n * zh_seek_entry_bytes(with_checksums) + ZH_SEEK_FOOTER));
}
ZH_SEEK_HD void zh_seek_write_footer(uint8_t *footer, uint64_t n, int with_checksums) {
  zh_seek_st32(footer, (uint32_t)n);
  footer[4] = with_checksums ? 0x80u : 0u;
  zh_seek_st32(footer + 5, ZH_SEEK_MAGIC);
}
ZH_SEEK_HD void zh_seek_write_entry(uint8_t *entry, uint32_t csize, uint32_t dsize, int with_checksums, uint32_t checksum) {
  zh_seek_st32(entry, csize);
  zh_seek_st32(entry + 4, dsize);
  if (with_checksums) zh_seek_st32(entry + 8, checksum);
}

struct ZhSeekFooter {
  uint64_t n;          // Number_Of_Frames
  uint32_t entry;      // bytes per entry
  uint32_t checksums;  // Checksum_Flag
  uint64_t table;      // bytes of the whole skippable frame
};

// Parse the last 9 bytes of a stream of `size` bytes: the magic, the reserved bits, N's limit,
// and that the table fits the stream.  `footer` points at those 9 bytes.
ZH_SEEK_HD uint32_t zh_seek_parse_footer(const uint8_t *footer, uint64_t size, ZhSeekFooter *f) {
  if (size < ZH_SEEK_OVERHEAD) return ZH_SEEK_CORRUPT;
  if (zh_seek_ld32(footer + 5) != ZH_SEEK_MAGIC) return ZH_SEEK_CORRUPT;
  uint8_t const d = footer[4];
  if (d & 0x7Cu) return ZH_SEEK_CORRUPT;
  f->n = zh_seek_ld32(footer);
  f->checksums = d >> 7;
  f->entry = zh_seek_entry_bytes((int)f->checksums);
  if (f->n > ZH_SEEK_MAX_FRAMES) return ZH_SEEK_CORRUPT;
  f->table = f->n * f->entry + ZH_SEEK_OVERHEAD;  // n <= 2^27, entry <= 12: no overflow
  if (f->table > size) return ZH_SEEK_CORRUPT;
  return ZH_SEEK_OK;
}

// The skippable header in front of the entries (`table` = stream + size - f.table)
ZH_SEEK_HD uint32_t zh_seek_check_header(const uint8_t *table, const ZhSeekFooter *f) {
  if (zh_seek_ld32(table) != ZH_SEEK_SKIP_MAGIC) return ZH_SEEK_CORRUPT;
  if ((uint64_t)zh_seek_ld32(table + 4) != f->n * f->entry + ZH_SEEK_FOOTER) return ZH_SEEK_CORRUPT;
  return ZH_SEEK_OK;
}

ZH_SEEK_HD bool zh_seek_field_ok(uint64_t v) { return v <= ZH_SEEK_MAX_FIELD; }
