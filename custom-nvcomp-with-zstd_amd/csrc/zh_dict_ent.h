// zh_dict_ent.h — the encoder's view of a formatted dictionary's entropy section (RFC 8878 §5):
// one blob per dictionary, built on the host at load (zh_dict_entropy.h) and read by
// zh_entropy_kernel for the first block of a frame when CompressionConfig::dict_entropy is set.
// Plain integers only: shared by host code, the stand-alone parser check and the kernels.
#pragma once
#include <stdint.h>

#define ZH_DENT_FSE_BYTES 3528u        // = ZH_FSE_TAB_BYTES (zh_common.h), the layout of ws.fse(b)
#define ZH_DENT_IMPOSSIBLE 0x00100000u // cost of a symbol the table gives no probability (> any real block's total)
#define ZH_DENT_COST_SHIFT 8u          // costs are bits << 8

struct ZhDictEnt {
  // stLL u16[512] | stOF u16[256] | stML u16[512] | symLL[36] | symOF[32] | symML[53] ({u32 dNb, s32 dFS}):
  // the FSE encoding tables as zh_fse_chain_kernel / zh_seq_pack_kernel read them
  uint8_t fse[ZH_DENT_FSE_BYTES];
  uint16_t hval[256];   // Huffman code of each byte value
  uint8_t hnb[256];     // its length, 0 = no code
  uint32_t hmask[8];    // bit v set: byte value v has a code (all zero: the table is not usable)
  uint32_t cost[3][64]; // LL, OF, ML: bits << 8 to code the symbol with the dictionary's table
  uint32_t logs[3];     // table logs, LL, OF, ML
  uint32_t reps[3];     // the three repcodes
  uint32_t huf_log;     // longest Huffman code (<= 11 when usable)
};
