/*
 * rdoq_tail_emu.cpp -- TEST-ONLY build of the wave emulator (fcu_emu.cpp) with the cross-check of rdoq_wave's passes after the
 * walk: under FCU_EMU_CHECK_RDOQ_TAIL every rdoq_wave call also stores records and levels to the pools as the pool form does,
 * runs rdoq_finish() (last position, signs, sign hiding on one lane) on a copy and aborts unless the levels of every position
 * the caller reads, uiAbsSum and the last position agree.  tests/test_rdoq_tail_emu.py builds it as libfcu_emu_rdoq_tail.so.
 */
#define FCU_EMU_CHECK_RDOQ_TAIL 1
#include "fcu_emu.cpp"
