/* the wave emulator without the register path of the 4x4 / 8x8 trials: every size through the candidate pools (tests/test_small_tu_emu.py) */
#define FCU_SMALL_TU_POOLS 1
#include "fcu_emu.cpp"
