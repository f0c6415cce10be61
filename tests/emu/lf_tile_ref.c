/*
 * lf_tile_ref.c -- TEST-ONLY reference: sample adaptive offset of one picture cut into uniform tiles, for either value of
 * LFCrossTileBoundaryFlag.  It is oracle/hmo_sao.c's hmo_sao_picture said again with two rules added; every function it calls
 * (statistics of a block, offsets, the two RDO modes, the coder, the offset pass of a block) is the oracle's own, reached by
 * including that file, so that nothing but the rules below is new:
 *   1. merge candidates (TComPic::getSAOMergeAvailability, TComPic.cpp:138-143), both values of the flag: left iff the CTU is
 *      not in the first column of the picture or of its tile, above iff not in the first row of either.  The walk stays raster
 *      order over the picture, the coder is carried across tile boundaries (TEncSampleAdaptiveOffset.cpp:802-873);
 *   2. sample availability with the flag 0 (TComPicSym::deriveLoopFilterBoundaryAvailibility, TComPicSym.cpp:378,449-459):
 *      L / R / A / B are false towards a CTU of another tile, the diagonals are the conjunction of their sides (a rectangular
 *      grid), for the statistics -- the skipped right / bottom margins follow R / B -- and for the offset pass.  With the flag 1
 *      availability is the picture border.
 * Not pinned by a run of HM with tiles: tests/lf_tile_oracle.py says what pins it instead.
 * Built by __graft_entry__.build() together with oracle/hmo_tables.c (the coder's tables) into tests/emu/liblf_tile_ref.so.
 */
#define hmo_sao_stats lf_ref_untiled_stats_
#define hmo_sao_picture lf_ref_untiled_picture_
#include "../../oracle/hmo_sao.c"
#undef hmo_sao_stats
#undef hmo_sao_picture

/* col_start[cx] / row_start[cy]: CTU column / row is the first of a tile (index 0 always is) */
static void tile_avail(int cx, int cy, int wc, int hc, const uint8_t *col_start, const uint8_t *row_start, int cross, int *L, int *R, int *A, int *B)
{
  *L = cx > 0; *R = cx + 1 < wc; *A = cy > 0; *B = cy + 1 < hc;
  if (cross) return;
  *L = *L && !col_start[cx]; *R = *R && !col_start[cx + 1];
  *A = *A && !row_start[cy]; *B = *B && !row_start[cy + 1];
}

void lf_ref_sao_tiles(int width, int height, int qp, int slice_type, const double lambda[3], const int enabled[3],
                      const uint8_t *col_start, const uint8_t *row_start, int cross,
                      const uint8_t *const org[3], uint8_t *const rec[3], HmoSaoBlk *coded, HmoSaoStat *stats_out, int off_count[3])
{
  hmo_init_tables();
  const int wc = (width + 63) / 64, hc = (height + 63) / 64, n = wc * hc;
  uint8_t *src[3];
  for (int comp = 0; comp < 3; comp++) {
    const size_t sz = (size_t)(width >> (comp ? 1 : 0)) * (size_t)(height >> (comp ? 1 : 0));
    src[comp] = (uint8_t *)malloc(sz); memcpy(src[comp], rec[comp], sz);
  }
  HmoSaoStat *stats = stats_out ? stats_out : (HmoSaoStat *)malloc(sizeof(HmoSaoStat) * (size_t)n * 3);
  for (int a = 0; a < n; a++) {                                /* hmo_sao_stats with rule 2 */
    const int cx = a % wc, cy = a / wc, x0 = cx * 64, y0 = cy * 64;
    const int bw = x0 + 64 > width ? width - x0 : 64, bh = y0 + 64 > height ? height - y0 : 64;
    int L, R, A, B;
    tile_avail(cx, cy, wc, hc, col_start, row_start, cross, &L, &R, &A, &B);
    for (int comp = 0; comp < 3; comp++) {
      const int sh = comp ? 1 : 0, stride = width >> sh;
      const size_t o = (size_t)(y0 >> sh) * stride + (x0 >> sh);
      blk_stats(&stats[a * 3 + comp], src[comp] + o, org[comp] + o, stride, bw >> sh, bh >> sh, comp, L, R, A, B);
    }
  }
  HmoSaoBlk *recon = (HmoSaoBlk *)calloc((size_t)n, sizeof(HmoSaoBlk));
  SaoCab goon;
  static const int init_type[3] = { 160, 185, 200 };
  goon.ctx[0] = ctx_from_init(153, qp);
  goon.ctx[1] = ctx_from_init(init_type[slice_type == HMO_SLICE_I ? 2 : 1], qp);
  goon.frac = 0;
  const int allOff = !enabled[0] && !enabled[1] && !enabled[2];
  for (int a = 0; a < n; a++) {                                /* raster order over the picture */
    if (allOff) { memset(&coded[a], 0, sizeof(coded[a])); continue; }
    const SaoCab cur = goon;
    SaoCab next = goon;
    const int cx = a % wc, cy = a / wc;
    const HmoSaoBlk *merge[2] = { NULL, NULL };
    if (cy > 0 && !row_start[cy]) merge[1] = &recon[a - wc];   /* rule 1 */
    if (cx > 0 && !col_start[cx]) merge[0] = &recon[a - 1];
    double minCost = 1.7e+308;
    HmoSaoBlk mode;
    double cost = derive_mode_new(&stats[a * 3], lambda, enabled, merge[0] != NULL, merge[1] != NULL, &cur, &goon, &mode);
    if (cost < minCost) { minCost = cost; coded[a] = mode; next = goon; }
    cost = derive_mode_merge(&stats[a * 3], lambda, enabled, merge, &cur, &goon, &mode);
    if (cost < minCost) { minCost = cost; coded[a] = mode; next = goon; }
    goon = next;
    recon[a] = coded[a];
    for (int comp = 0; comp < 3; comp++) {
      HmoSaoOffset *p = &recon[a].c[comp];
      if (p->mode == SAO_NEW) invert_quant(p->type, p->aux, p->offset, p->offset);
      else if (p->mode == SAO_MERGE) *p = merge[p->type]->c[comp];
    }
    const int x0 = cx * 64, y0 = cy * 64;
    const int bw = x0 + 64 > width ? width - x0 : 64, bh = y0 + 64 > height ? height - y0 : 64;
    int L, R, A, B;
    tile_avail(cx, cy, wc, hc, col_start, row_start, cross, &L, &R, &A, &B);
    for (int comp = 0; comp < 3; comp++) {
      const HmoSaoOffset *p = &recon[a].c[comp];
      if (p->mode == SAO_OFF) continue;
      const int sh = comp ? 1 : 0, stride = width >> sh;
      const size_t o = (size_t)(y0 >> sh) * stride + (x0 >> sh);
      offset_block(p->type, p->offset, src[comp] + o, rec[comp] + o, stride, bw >> sh, bh >> sh, L, R, A, B);
    }
  }
  if (off_count) for (int comp = 0; comp < 3; comp++) { off_count[comp] = 0; for (int a = 0; a < n; a++) off_count[comp] += recon[a].c[comp].mode == SAO_OFF; }
  free(recon);
  if (!stats_out) free(stats);
  for (int comp = 0; comp < 3; comp++) free(src[comp]);
}
