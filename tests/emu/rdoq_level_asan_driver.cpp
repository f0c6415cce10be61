/*
 * rdoq_level_asan_driver.cpp -- TEST-ONLY stand-alone program: the engine source as the CPU wave emulator (-DFCU_EMU) with the
 * cross-check of the level choice (-DFCU_EMU_CHECK_RDOQ_LEVELS: level_choice() against coded_level() + ic_rate() on every
 * coefficient with uiMaxAbsLevel > 0) under the address and undefined-behaviour sanitizers, on the frames of
 * tests/rdoq_level_cases.py.  tests/emu/rdoq_level_asan.sh writes them as raw 4:2:0 files into a directory, with a manifest.txt
 * that carries their sizes and QPs (so the numbers live in rdoq_level_cases.py alone), and passes the directory's name:
 *   intra FILE WIDTH HEIGHT QP                           an intra frame
 *   ldp FILE0 FILE1 REF WIDTH HEIGHT BASE_QP SEARCH_RANGE  the two pictures of the lowdelay_P clip; REF: the deblocked
 *                                                        reconstruction of the first (the reference picture of the second)
 * Planes, padded reference planes, the output array and the scratch block are heap blocks of exactly the size the library gives
 * them.  The program fails unless every case tests/test_rdoq_level_emu.py asserts was reached here too, and no remainder of
 * 32768 or more was formed.
 */
#define FCU_EMU 1
#define FCU_EMU_CHECK_RDOQ_LEVELS 1
#include "../../fast-cu-decision-hevc_amd/csrc/fcu_host.h"
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <string>

using namespace fcu;

struct Picture { int w, h; uint8_t *org[3], *rec[3]; };
static size_t plane_size(int w, int h, int k) { return k ? (size_t)(w / 2) * (h / 2) : (size_t)w * h; }
static Picture load_picture(const std::string &path, int w, int h)
{
  Picture p; p.w = w; p.h = h;
  FILE *f = fopen(path.c_str(), "rb");
  if (!f) { fprintf(stderr, "cannot open %s\n", path.c_str()); exit(2); }
  for (int k = 0; k < 3; k++) {
    const size_t n = plane_size(w, h, k);
    p.org[k] = (uint8_t *)malloc(n); p.rec[k] = (uint8_t *)calloc(n, 1);
    if (fread(p.org[k], 1, n, f) != n) { fprintf(stderr, "%s is shorter than a %dx%d 4:2:0 picture\n", path.c_str(), w, h); exit(2); }
  }
  fclose(f);
  return p;
}
static void free_picture(Picture &p) { for (int k = 0; k < 3; k++) { free(p.org[k]); free(p.rec[k]); } }

/* TComPicYuv::extendPicBorder into a block of exactly the padded size: margin m on every side */
static uint8_t *pad(const uint8_t *src, int w, int h, int m)
{
  const int sw = w + 2 * m, sh = h + 2 * m;
  uint8_t *p = (uint8_t *)malloc((size_t)sw * sh);
  for (int y = 0; y < sh; y++) for (int x = 0; x < sw; x++) {
    const int sx = x - m < 0 ? 0 : (x - m >= w ? w - 1 : x - m), sy = y - m < 0 ? 0 : (y - m >= h ? h - 1 : y - m);
    p[(size_t)y * sw + x] = src[sy * w + sx];
  }
  return p;
}

/* one picture as one chain; ref: the planes (in org[]) of the picture a P picture refers to (nullptr: an I picture) */
static void run(const char *name, Picture &pic, const fcu_frame_params &fp, const Picture *ref)
{
  const int w = pic.w, h = pic.h, nctu = ((w + 63) / 64) * ((h + 63) / 64);
  fcu_ctu_out *out = (fcu_ctu_out *)calloc((size_t)nctu, sizeof(fcu_ctu_out));
  Chain *c = new Chain();
  chain_bind(*c, w, h, fp, pic.org[0], pic.org[1], pic.org[2], pic.rec[0], pic.rec[1], pic.rec[2], out);
  uint8_t *pp[3] = { nullptr, nullptr, nullptr };
  if (ref) {
    for (int k = 0; k < 3; k++) pp[k] = pad(ref->org[k], k ? w / 2 : w, k ? h / 2 : h, k ? FCU_REF_MARGIN / 2 : FCU_REF_MARGIN);
    const uint8_t *const planes[3] = { pp[0], pp[1], pp[2] };
    const int ref_poc = 0;
    chain_set_list0(*c, 1, planes, &ref_poc, 1);
  }
  Scratch *g = (Scratch *)calloc(1, sizeof(Scratch));
  unsigned long long before = 0, after = 0, sum = 0;
  for (int i = LEVEL_MAX1; i <= LEVEL_MAX3UP; i++) before += fcu_emu_level_cnt[i];
  for (int a = 0; a < nctu; a++) { compress_ctu(c, g, a); c->next_ctu = a + 1; }
  for (int i = LEVEL_MAX1; i <= LEVEL_MAX3UP; i++) after += fcu_emu_level_cnt[i];
  for (size_t i = 0; i < (size_t)w * h; i++) sum += pic.rec[0][i];
  printf("%-8s %3dx%-3d qp %d: %d CTUs, luma reconstruction sum %llu, level choices checked %llu\n", name, w, h, fp.qp, nctu, sum, after - before);
  free(g); delete c; free(out);
  for (int k = 0; k < 3; k++) free(pp[k]);
}

int main(int argc, char **argv)
{
  if (argc < 2) { fprintf(stderr, "usage: %s DIRECTORY-OF-FRAMES\n", argv[0]); return 2; }
  const std::string dir = std::string(argv[1]) + "/";
  load_hot_tables();
  fcu_frame_params fp;
  FILE *mf = fopen((dir + "manifest.txt").c_str(), "r");
  if (!mf) { fprintf(stderr, "no manifest.txt in %s\n", argv[1]); return 2; }
  char kind[16], f0[64], f1[64], f2[64];
  int pictures = 0;
  while (fscanf(mf, "%15s", kind) == 1) {
    int w, h, qp, sr;
    if (!strcmp(kind, "intra") && fscanf(mf, "%63s %d %d %d", f0, &w, &h, &qp) == 4) {
      Picture p = load_picture(dir + f0, w, h);
      default_frame_params(fp, qp);
      run(f0, p, fp, nullptr);
      free_picture(p);
      pictures++;
    } else if (!strcmp(kind, "ldp") && fscanf(mf, "%63s %63s %63s %d %d %d %d", f0, f1, f2, &w, &h, &qp, &sr) == 7) {   /* TZ search */
      Picture a = load_picture(dir + f0, w, h), b = load_picture(dir + f1, w, h), r = load_picture(dir + f2, w, h);
      ldp_slice(fp, qp, 0);
      run(f0, a, fp, nullptr);
      ldp_slice(fp, qp, 1); fp.search_range = sr; fp.fast_search = 1;
      run(f1, b, fp, &r);
      free_picture(a); free_picture(b); free_picture(r);
      pictures += 2;
    } else { fprintf(stderr, "manifest.txt: cannot read a line of kind %s\n", kind); return 2; }
  }
  fclose(mf);
  if (!pictures) { fprintf(stderr, "manifest.txt lists no picture\n"); return 2; }
  static const char *cn[LEVEL_N] = { "uiMaxAbsLevel 1", "uiMaxAbsLevel 2", "uiMaxAbsLevel 3 and more", "chose uiMaxAbsLevel - 1 (not 0)", "chose level 0",
                                     "the last position", "c1Idx >= 8", "c2Idx >= 1", "Rice parameter 0", "Rice parameter 4", "remainder equal to 3 << rice",
                                     "remainder above 3 << rice", "remainder of 32768 or more" };
  int missed = 0;
  for (int i = 0; i < LEVEL_N; i++) {
    printf("%-34s %llu\n", cn[i], fcu_emu_level_cnt[i]);
    if (i == LEVEL_SYMBOL_32768UP) { if (fcu_emu_level_cnt[i]) { printf("  ^ must stay 0\n"); missed++; } }
    else if (!fcu_emu_level_cnt[i]) { printf("  ^ case not reached\n"); missed++; }
  }
  return missed ? 1 : 0;
}
