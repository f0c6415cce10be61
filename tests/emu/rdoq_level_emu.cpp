/*
 * rdoq_level_emu.cpp -- TEST-ONLY build of the wave emulator (fcu_emu.cpp) with the cross-check of the level choice: under
 * FCU_EMU_CHECK_RDOQ_LEVELS every coefficient with uiMaxAbsLevel > 0 of every rdoq() / rdoq_wave() call is priced twice, by
 * level_choice() and by coded_level() + ic_rate() (the definition), and the emulator aborts unless the level, pdCostCoeff,
 * pdCostCoeff0 and pdCostSig (bit patterns), rateIncUp, rateIncDown and deltaU agree; fcu_emu_level_cnt counts the cases met.
 * tests/test_rdoq_level_emu.py builds it as libfcu_emu_rdoq_level.so.
 */
#define FCU_EMU_CHECK_RDOQ_LEVELS 1
#include "fcu_emu.cpp"
