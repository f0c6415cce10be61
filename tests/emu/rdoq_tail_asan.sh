#!/bin/bash
# Host-side check of rdoq_wave's passes after the walk (lane registers, sign hiding on the wave): the emulator's engine
# translation unit with -DFCU_EMU_CHECK_RDOQ_TAIL plus rdoq_tail_asan_driver.cpp under the address and undefined-behaviour
# sanitizers, run directly (no Python, no GPU).
# -fno-sanitize=shift: the dequantiser shifts negative products left as the reference does (two's complement).
set -e
cd "$(dirname "$0")"
g++ -std=c++17 -O1 -g -ffp-contract=off -fsanitize=address,undefined -fno-sanitize=shift -fno-sanitize-recover=undefined -o rdoq_tail_asan_driver rdoq_tail_asan_driver.cpp
./rdoq_tail_asan_driver
