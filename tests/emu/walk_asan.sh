#!/bin/bash
# Host-side out-of-bounds check of the group-ahead loads in the lane-private walks: the emulator's engine translation unit
# plus walk_asan_driver.cpp under the address and undefined-behaviour sanitizers, run directly (no Python, no GPU).
# -fno-sanitize=shift: the dequantiser shifts negative products left as the reference does (two's complement).
set -e
cd "$(dirname "$0")"
g++ -std=c++17 -O1 -g -ffp-contract=off -fsanitize=address,undefined -fno-sanitize=shift -fno-sanitize-recover=undefined -o walk_asan_driver walk_asan_driver.cpp
./walk_asan_driver
