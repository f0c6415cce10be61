#!/bin/bash
# Host-side check of the register path of the 4x4 / 8x8 trials: the emulator's engine translation unit plus
# small_tu_asan_driver.cpp under the address and undefined-behaviour sanitizers, run directly (no Python, no GPU).
# -fno-sanitize=shift: the dequantiser shifts negative products left as the reference does (two's complement).
set -e
cd "$(dirname "$0")"
g++ -std=c++17 -O1 -g -ffp-contract=off -fsanitize=address,undefined -fno-sanitize=shift -fno-sanitize-recover=undefined -o small_tu_asan_driver small_tu_asan_driver.cpp
./small_tu_asan_driver
