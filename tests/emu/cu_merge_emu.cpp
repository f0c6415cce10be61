/*
 * cu_merge_emu.cpp -- TEST-ONLY build of the wave emulator (fcu_emu.cpp) with the cross-check of the merged CU bits:
 * under FCU_EMU_CHECK_CU_MERGE check_rd_cost_intra also walks every CU whose bits it merged from the search's coders and
 * FCU_CHECKs bits, bins, the Q15 count and every context byte against the walk.  tests/test_cu_bits_merge.py builds it as
 * libfcu_emu_cu_merge.so and reads the path counters.
 */
#define FCU_EMU_CHECK_CU_MERGE 1
#include "fcu_emu.cpp"

extern "C" {
/* intra candidate CUs since the last reset: [0] merged with the chroma search's coder, [1] merged with a chroma-only walk, [2] walked */
void fcu_emu_cu_paths(unsigned long long *out3, int reset)
{
  for (int i = 0; i < 3; i++) { out3[i] = g_emu_cu_paths[i]; if (reset) g_emu_cu_paths[i] = 0; }
}
}
