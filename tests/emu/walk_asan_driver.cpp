/*
 * walk_asan_driver.cpp -- TEST-ONLY stand-alone program: the engine source as the CPU wave emulator (-DFCU_EMU) under the
 * address and undefined-behaviour sanitizers, on the frames of tests/walk_prefetch_cases.py (flat, impulse, checker, stripes;
 * "textured" is a generated texture here, the numpy one is not available to a C++ program), 64x64 and 128x64, QP 22 and 37.
 * It exists for the group-ahead loads of rdoq<0>: planes, the output array and the scratch block are
 * heap blocks of exactly the size the library gives them (sizeof(Scratch) per chain, as fcu_create does), so a load one
 * group too far at either end of a block is a sanitizer error; the pools are members of the scratch block, so there the
 * engine itself checks every address a group load of rdoq<0> forms against the bounds of Scratch::p_lscan (FCU_CHECK_LSCAN).
 * The program fails unless every edge case the pytest asserts was reached here too.  Build and run (tests/emu/walk_asan.sh):
 *   g++ -std=c++17 -O1 -g -ffp-contract=off -fsanitize=address,undefined -fno-sanitize=shift -fno-sanitize-recover=undefined \
 *       -o walk_asan_driver walk_asan_driver.cpp && ./walk_asan_driver
 */
#define FCU_EMU 1
#include "../../fast-cu-decision-hevc_amd/csrc/fcu_host.h"
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

using namespace fcu;

static void fill(int source, int w, int h, uint8_t *Y)
{
  memset(Y, 128, (size_t)w * h);
  uint32_t r = 12345u;
  for (int x0 = 0; x0 < w; x0 += 64) {
    if (source == 1) Y[21 * w + x0 + 37] = 250;
    else if (source == 2) {
      for (int y = 0; y < 32; y++) for (int x = 0; x < 32; x++) Y[y * w + x0 + x] = (uint8_t)(128 + 6 * (((x + y) & 1) * 2 - 1));
      for (int y = 0; y < 8; y++) for (int x = 0; x < 8; x++) {
        const int s = ((x + y) & 1) * 2 - 1;
        Y[(40 + y) * w + x0 + 40 + x] = (uint8_t)(128 + 9 * s);
        Y[(48 + y) * w + x0 + 8 + x] = (uint8_t)(128 + 1 * s);
        Y[(48 + y) * w + x0 + 24 + x] = (uint8_t)(128 + 5 * s);
      }
    } else if (source == 3) {
      for (int y = 0; y < 32; y++) for (int x = 0; x < 32; x++) {
        int v = 128 + 20 * ((y & 1) * 2 - 1) + (x - 16);
        Y[(32 + y) * w + x0 + x] = (uint8_t)(v < 0 ? 0 : v > 255 ? 255 : v);
      }
    } else if (source == 4) {
      for (int y = 0; y < h; y++) for (int x = 0; x < 64; x++) {
        r = r * 1664525u + 1013904223u;
        int v = 128 + (int)(40.0 * ((x * 3 + y * 5) % 17 - 8) / 8.0) + (int)((r >> 24) & 31) - 16;
        Y[y * w + x0 + x] = (uint8_t)(v < 0 ? 0 : v > 255 ? 255 : v);
      }
    }
  }
}

int main()
{
  static const char *names[5] = { "flat", "impulse", "checker", "stripes", "texture" };
  static const int sizes[2][2] = { { 64, 64 }, { 128, 64 } }, qps[2] = { 22, 37 };
  load_hot_tables();
  for (int source = 0; source < 5; source++) for (int si = 0; si < 2; si++) for (int qi = 0; qi < 2; qi++) {
    const int w = sizes[si][0], h = sizes[si][1], qp = qps[qi], nctu = ((w + 63) / 64) * ((h + 63) / 64);
    uint8_t *org[3], *rec[3];
    for (int k = 0; k < 3; k++) {
      const size_t n = k ? (size_t)(w / 2) * (h / 2) : (size_t)w * h;
      org[k] = (uint8_t *)malloc(n); rec[k] = (uint8_t *)malloc(n);
      memset(org[k], 128, n); memset(rec[k], 0, n);
    }
    fill(source, w, h, org[0]);
    fcu_ctu_out *out = (fcu_ctu_out *)calloc((size_t)nctu, sizeof(fcu_ctu_out));
    Chain *c = new Chain();
    fcu_frame_params fp; default_frame_params(fp, qp);
    chain_bind(*c, w, h, fp, org[0], org[1], org[2], rec[0], rec[1], rec[2], out);
    Scratch *g = (Scratch *)calloc(1, sizeof(Scratch));
    for (int a = 0; a < nctu; a++) { compress_ctu(c, g, a); c->next_ctu = a + 1; }
    unsigned long long sum = 0;
    for (size_t i = 0; i < (size_t)w * h; i++) sum += rec[0][i];
    printf("%-8s %3dx%-3d qp %d: %d CTUs, luma reconstruction sum %llu\n", names[source], w, h, qp, nctu, sum);
    free(g); delete c; free(out);
    for (int k = 0; k < 3; k++) { free(org[k]); free(rec[k]); }
  }
  static const char *cn[WALK_N] = { "rdoq<0> calls", "rdoq<0> starting in group 0", "rdoq<0> groups loaded ahead", "only level in group 0",
                                    "only level in the last group", "all-zero TUs", "bit counter calls", "one empty 128-byte run between non-empty ones",
                                    "second bit-count rounds (17-20 variants)" };
  int missed = 0;
  for (int i = 0; i < WALK_N; i++) {
    printf("%-48s %llu\n", cn[i], fcu_emu_walk_cnt[i]);
    if (!fcu_emu_walk_cnt[i]) { printf("  ^ edge case not reached\n"); missed++; }
  }
  if (missed) return 1;
  return 0;
}
