/*
 * small_tu_asan_driver.cpp -- TEST-ONLY stand-alone program: the engine source as the CPU wave emulator (-DFCU_EMU) under the
 * address and undefined-behaviour sanitizers, on four frames like those of tests/small_tu_cases.py (a generated texture at
 * 64x64 QP 22 / QP 37 and at 72x80 QP 32, sparse noise on a flat 64x64 frame at QP 32; the numpy generators are not available
 * to a C++ program).  It exists for the register path of the 4x4 / 8x8 trials (pu_first_pass_batched).  Planes, the output array and the scratch block are heap blocks of
 * exactly the size the library gives them, and a LaneVar of the emulator is an array of 64 elements, so a source lane or a pool
 * index out of range is a sanitizer error.  The program fails unless the edge cases were reached (fcu_emu_small_cnt).
 * Build and run: tests/emu/small_tu_asan.sh
 */
#define FCU_EMU 1
#include "../../fast-cu-decision-hevc_amd/csrc/fcu_host.h"
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

using namespace fcu;

static void fill(int noise, int w, int h, uint8_t *Y)
{
  uint32_t r = 12345u;
  for (int y = 0; y < h; y++) for (int x = 0; x < w; x++) {
    r = r * 1664525u + 1013904223u;
    int v;
    if (noise) v = ((r >> 16) % 100u) < 6u ? (((r >> 8) & 1) ? 230 : 20) : 100;
    else v = 128 + (int)(40.0 * ((x * 3 + y * 5) % 17 - 8) / 8.0) + (int)((r >> 24) & 31) - 16;
    Y[y * w + x] = (uint8_t)(v < 0 ? 0 : v > 255 ? 255 : v);
  }
}

int main()
{
  static const int cases[4][4] = { { 0, 64, 64, 22 }, { 0, 64, 64, 37 }, { 0, 72, 80, 32 }, { 1, 64, 64, 32 } };
  load_hot_tables();
  for (int k = 0; k < 4; k++) {
    const int noise = cases[k][0], w = cases[k][1], h = cases[k][2], qp = cases[k][3], nctu = ((w + 63) / 64) * ((h + 63) / 64);
    uint8_t *org[3], *rec[3];
    for (int c = 0; c < 3; c++) {
      const size_t n = c ? (size_t)(w / 2) * (h / 2) : (size_t)w * h;
      org[c] = (uint8_t *)malloc(n); rec[c] = (uint8_t *)malloc(n);
      memset(org[c], 128, n); memset(rec[c], 0, n);
    }
    fill(noise, w, h, org[0]);
    fcu_ctu_out *out = (fcu_ctu_out *)calloc((size_t)nctu, sizeof(fcu_ctu_out));
    Chain *c = new Chain();
    fcu_frame_params fp; default_frame_params(fp, qp);
    chain_bind(*c, w, h, fp, org[0], org[1], org[2], rec[0], rec[1], rec[2], out);
    Scratch *g = (Scratch *)calloc(1, sizeof(Scratch));
    for (int a = 0; a < nctu; a++) { compress_ctu(c, g, a); c->next_ctu = a + 1; }
    unsigned long long sum = 0;
    for (size_t i = 0; i < (size_t)w * h; i++) sum += rec[0][i];
    printf("%-8s %3dx%-3d qp %d: %d CTUs, luma reconstruction sum %llu\n", noise ? "noise" : "texture", w, h, qp, nctu, sum);
    free(g); delete c; free(out);
    for (int i = 0; i < 3; i++) { free(org[i]); free(rec[i]); }
  }
  static const char *cn[SMALL_N] = { "transform-skip winners", "trials with all levels zero", "4x4 batches of more than 16 variants", "chroma 4x4 trials" };
  int missed = 0;
  for (int i = 0; i < SMALL_N; i++) {
    printf("%-40s %llu\n", cn[i], fcu_emu_small_cnt[i]);
    if (!fcu_emu_small_cnt[i]) { printf("  ^ edge case not reached\n"); missed++; }
  }
  return missed ? 1 : 0;
}
