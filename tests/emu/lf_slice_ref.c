/*
 * lf_slice_ref.c -- TEST-ONLY reference: the loop filters of one picture of SliceMode 1 slices for either value of
 * LFCrossSliceBoundaryFlag.  A slice is slice_ctus consecutive CTUs in raster order (the last one what is left) and may start
 * mid-row; all slices carry the same flag (TEncGOP.cpp:763).  It is oracle/hmo_deblock.c's hmo_deblock_pic and oracle/hmo_sao.c's
 * hmo_sao_picture said again with the slice rules added; every function below the rules (boundary strength, the sample filters,
 * offsets, the two RDO modes, the coder) is the oracle's own, reached by including those files, so that nothing but this is new:
 *   1. deblocking with the flag 0 (TComLoopFilter.cpp:369-411 with TComDataCU::getPULeft / getPUAbove, TComDataCU.cpp:1095,1134;
 *      :430-434,609-613,754-758): a partition on the left / top edge of its CTU gets no edge flag when the CTU to the left / above
 *      lies in another slice, luma and chroma, as on the picture border (edge_flag_slices);
 *   2. the offset pass with the flag 0 (TComSampleAdaptiveOffset.cpp:577; deriveLoopFilterBoundaryAvailibility, TComPicSym.cpp:
 *      357-447): a neighbour CTU is available iff it is inside the picture and in the CTU's slice, in eight directions of their
 *      own (slice_avail8), and offsetBlock (:317-556) said with eight flags (offset_block8): once a slice starts or ends mid-row a
 *      diagonal is not the conjunction of its sides;
 *   3. the statistics with the flag 0 (TEncSampleAdaptiveOffset.cpp:327-336): the same derivation, then right, below, below-right,
 *      below-left and above-right from the picture border only ("For simplicity, here only picture boundaries are considered"), so
 *      L, A and AL are the slice's and R and B -- with the skipped margins -- the picture's (blk_stats8; AL matters for sample
 *      (0, 0) of EO_135 only, :1150-1154);
 *   4. the decision is hmo_sao_picture's for either flag: merge candidates inside the slice, the walk and the coder across slices.
 * With the flag 1 every availability is the picture border: the oracle's.
 * lf_ref_blk_stats4 / 8 and lf_ref_offset_block4 / 8 hand single blocks to the tests: with the diagonals set to the conjunctions
 * of their sides the eight-flag functions must reproduce the oracle's four-flag ones.
 * Not pinned by a run of HM with slices and the flag 0: tests/lf_slice_oracle.py says what pins it instead.
 * Built by __graft_entry__.build() together with oracle/hmo_tables.c into tests/emu/liblf_slice_ref.so.
 */
#define hmo_sao_stats lf_sref_plain_stats_
#define hmo_sao_picture lf_sref_plain_picture_
#include "../../oracle/hmo_sao.c"
#undef hmo_sao_stats
#undef hmo_sao_picture
#define hmo_deblock_pic lf_sref_plain_deblock_pic_
#define hmo_deblock lf_sref_plain_deblock_
#include "../../oracle/hmo_deblock.c"
#undef hmo_deblock_pic
#undef hmo_deblock

/* S CTUs per slice (0, or the picture and more: one slice) */
static int slice_len(int n, int slice_ctus) { return slice_ctus <= 0 || slice_ctus > n ? n : slice_ctus; }
static int same_slice(int S, int n, int a, int b) { return b >= 0 && b < n && a / S == b / S; }

/* ---- rule 1 */
static int edge_flag_slices(const Dbk *d, int dir, int x4, int y4, int S, int n)
{
  const int pos = (dir == 0 ? x4 : y4) * 4;
  if (pos % 64 == 0 && pos > 0) {
    const int a = (y4 >> 4) * d->w_ctu + (x4 >> 4);
    if (!same_slice(S, n, a, dir == 0 ? a - 1 : a - d->w_ctu)) return 0;
  }
  return edge_flag(d, dir, x4, y4);
}
/* hmo_deblock_pic's loop with edge_flag_slices in the place of edge_flag */
void lf_ref_deblock_slices(const HmoCtu *pic, int width, int height, uint8_t *recY, uint8_t *recU, uint8_t *recV,
                           int betaOffsetDiv2, int tcOffsetDiv2, int slice_ctus, int cross)
{
  Dbk d; d.pic = pic; d.w = width; d.h = height; d.w_ctu = (width + 63) / 64;
  const int n = d.w_ctu * ((height + 63) / 64), S = cross ? n : slice_len(n, slice_ctus);
  const uint8_t *z2r = hmo_zscan_to_raster();
  for (int z = 0; z < 256; z++) d.r2z[z2r[z]] = (uint8_t)z;
  const int w4 = width / 4, h4 = height / 4, cw = width / 2;
  uint8_t *chroma[2] = { recU, recV };
  for (int dir = 0; dir < 2; dir++) {
    for (int y4 = 0; y4 < h4; y4++)
      for (int x4 = 0; x4 < w4; x4++) {
        const int pos4 = dir == 0 ? x4 : y4;
        int flag;
        if ((pos4 & 1) || !(flag = edge_flag_slices(&d, dir, x4, y4, S, n))) continue;
        const int bs = boundary_strength(&d, flag, x4, y4, dir == 0 ? x4 - 1 : x4, dir == 0 ? y4 : y4 - 1);
        if (bs == 0) continue;
        const int qpQ = qp_at(&d, x4, y4), qpP = dir == 0 ? qp_at(&d, x4 - 1, y4) : qp_at(&d, x4, y4 - 1);
        const int qp = (qpP + qpQ + 1) >> 1;
        uint8_t *p = recY + (y4 * 4) * width + x4 * 4;
        if (dir == 0) luma_segment(p, 1, width, qp, betaOffsetDiv2, tcOffsetDiv2, bs);
        else luma_segment(p, width, 1, qp, betaOffsetDiv2, tcOffsetDiv2, bs);
        if ((pos4 & 3) == 0 && bs == 2) {
          int qc = qp;
          if (qc >= 58) qc -= 6; else if (qc >= 0) qc = k_chroma_scale[qc];
          const int tc = k_tc[clip3(0, 53, qc + 2 * (2 - 1) + tcOffsetDiv2 * 2)];
          for (int c = 0; c < 2; c++) {
            uint8_t *q = chroma[c] + (y4 * 2) * cw + x4 * 2;
            for (int i = 0; i < 2; i++) {
              if (dir == 0) pel_filter_chroma(q + i * cw, 1, tc);
              else pel_filter_chroma(q + i, cw, tc);
            }
          }
        }
      }
  }
}

/* ---- rules 2 and 3: v[8] = L, R, A, B, AL, AR, BL, BR of CTU a (TComPicSym.cpp:369-447 with one flag for all slices: the
 * diagonal neighbour is picked by the picture border, then its own slice is tested) */
enum { AV_L, AV_R, AV_A, AV_B, AV_AL, AV_AR, AV_BL, AV_BR };
static void slice_avail8(int a, int wc, int hc, int S, int v[8])
{
  const int n = wc * hc, cx = a % wc, cy = a / wc;
  const int L = cx > 0, R = cx + 1 < wc, A = cy > 0, B = cy + 1 < hc;
  v[AV_L] = L && same_slice(S, n, a, a - 1);       v[AV_R] = R && same_slice(S, n, a, a + 1);
  v[AV_A] = A && same_slice(S, n, a, a - wc);      v[AV_B] = B && same_slice(S, n, a, a + wc);
  v[AV_AL] = A && L && same_slice(S, n, a, a - wc - 1); v[AV_AR] = A && R && same_slice(S, n, a, a - wc + 1);
  v[AV_BL] = B && L && same_slice(S, n, a, a + wc - 1); v[AV_BR] = B && R && same_slice(S, n, a, a + wc + 1);
}
void lf_ref_slice_avail8(int a, int wc, int hc, int slice_ctus, int v[8]) { slice_avail8(a, wc, hc, slice_len(wc * hc, slice_ctus), v); }

/* getBlkStats as the oracle's blk_stats says it, with AL a flag of its own (firstLineStartX of EO_135, :1153) */
static void blk_stats8(HmoSaoStat *st, const uint8_t *src, const uint8_t *org, int stride, int w, int h, int comp, int L, int R, int A, int B, int AL)
{
  memset(st, 0, sizeof(*st));
  const int skipR = comp ? 3 : 5, skipB = comp ? 2 : 4;
  const int sx = L ? 0 : 1, ex = R ? w - skipR : w - 1, exFull = R ? w - skipR : w;
  const int eyFull = B ? h - skipB : h, ey = B ? h - skipB : h - 1;
  for (int y = 0; y < h; y++) for (int x = 0; x < w; x++) {
    const uint8_t *s = src + y * stride + x;
    const int c = s[0], d = org[y * stride + x] - c;
    if (x < exFull && y < eyFull) { st->diff[SAO_BO][c >> 3] += d; st->count[SAO_BO][c >> 3]++; }
    if (x >= sx && x < ex && y < eyFull) { const int k = 2 + sgn(c - s[-1]) + sgn(c - s[1]); st->diff[0][k] += d; st->count[0][k]++; }
    if (x < exFull && y >= (A ? 0 : 1) && y < ey) { const int k = 2 + sgn(c - s[-stride]) + sgn(c - s[stride]); st->diff[1][k] += d; st->count[1][k]++; }
    if (y == 0 ? (x >= (AL ? 0 : 1) && x < (A ? ex : 1)) : (y < ey && x >= sx && x < ex)) {                 /* :1153-1156 */
      const int k = 2 + sgn(c - s[-stride - 1]) + sgn(c - s[stride + 1]); st->diff[2][k] += d; st->count[2][k]++;
    }
    if (y == 0 ? (A && x >= sx && x < ex) : (y < ey && x >= sx && x < ex)) {                                /* :1256-1259, AR = the picture's */
      const int k = 2 + sgn(c - s[-stride + 1]) + sgn(c - s[stride - 1]); st->diff[3][k] += d; st->count[3][k]++;
    }
  }
}
/* offsetBlock (TComSampleAdaptiveOffset.cpp:317-556), sample by sample, the first and last lines of the diagonal classes with the
 * bounds as HM writes them (:431-432, 468-469, 496-497, 525-526) */
static void offset_block8(int type, const int *offset, const uint8_t *src, uint8_t *res, int stride, int w, int h, const int v[8])
{
  const int L = v[AV_L], R = v[AV_R], A = v[AV_A], B = v[AV_B], AL = v[AV_AL], AR = v[AV_AR], BL = v[AV_BL], BR = v[AV_BR];
  const int sx = L ? 0 : 1, ex = R ? w : w - 1;
  for (int y = 0; y < h; y++) for (int x = 0; x < w; x++) {
    const uint8_t *s = src + y * stride + x;
    const int c = s[0];
    int k = -1;
    switch (type) {
    case 0: if (x >= sx && x < ex) k = 2 + sgn(c - s[-1]) + sgn(c - s[1]); break;
    case 1: if (y >= (A ? 0 : 1) && y < (B ? h : h - 1)) k = 2 + sgn(c - s[-stride]) + sgn(c - s[stride]); break;
    case 2: {
      int ok;
      if (y == 0) ok = x >= (AL ? 0 : 1) && x < (A ? ex : 1);
      else if (y == h - 1) ok = x >= (B ? sx : w - 1) && x < (BR ? w : w - 1);
      else ok = x >= sx && x < ex;
      if (ok) k = 2 + sgn(c - s[-stride - 1]) + sgn(c - s[stride + 1]);
      break; }
    case 3: {
      int ok;
      if (y == 0) ok = x >= (A ? sx : w - 1) && x < (AR ? w : w - 1);
      else if (y == h - 1) ok = x >= (BL ? 0 : 1) && x < (B ? ex : 1);
      else ok = x >= sx && x < ex;
      if (ok) k = 2 + sgn(c - s[-stride + 1]) + sgn(c - s[stride - 1]);
      break; }
    default: k = c >> 3; break;
    }
    if (k >= 0) { const int val = c + offset[k]; res[y * stride + x] = (uint8_t)(val < 0 ? 0 : (val > 255 ? 255 : val)); }
  }
}
/* single blocks for the tests: the oracle's four-flag functions and the eight-flag ones above */
void lf_ref_blk_stats4(HmoSaoStat *st, const uint8_t *src, const uint8_t *org, int stride, int w, int h, int comp, int L, int R, int A, int B)
{ blk_stats(st, src, org, stride, w, h, comp, L, R, A, B); }
void lf_ref_blk_stats8(HmoSaoStat *st, const uint8_t *src, const uint8_t *org, int stride, int w, int h, int comp, int L, int R, int A, int B, int AL)
{ blk_stats8(st, src, org, stride, w, h, comp, L, R, A, B, AL); }
void lf_ref_offset_block4(int type, const int *offset, const uint8_t *src, uint8_t *res, int stride, int w, int h, int L, int R, int A, int B)
{ offset_block(type, offset, src, res, stride, w, h, L, R, A, B); }
void lf_ref_offset_block8(int type, const int *offset, const uint8_t *src, uint8_t *res, int stride, int w, int h, const int v[8])
{ offset_block8(type, offset, src, res, stride, w, h, v); }

/* the statistics of the picture (rule 3; cross: the picture border alone) */
static void stats_slices(int width, int height, int S, const uint8_t *const org[3], uint8_t *const src[3], HmoSaoStat *stats)
{
  const int wc = (width + 63) / 64, hc = (height + 63) / 64;
  for (int a = 0; a < wc * hc; a++) {
    const int cx = a % wc, cy = a / wc, x0 = cx * 64, y0 = cy * 64;
    const int bw = x0 + 64 > width ? width - x0 : 64, bh = y0 + 64 > height ? height - y0 : 64;
    int v[8];
    slice_avail8(a, wc, hc, S, v);
    for (int comp = 0; comp < 3; comp++) {
      const int sh = comp ? 1 : 0, stride = width >> sh;
      const size_t o = (size_t)(y0 >> sh) * stride + (x0 >> sh);
      blk_stats8(&stats[a * 3 + comp], src[comp] + o, org[comp] + o, stride, bw >> sh, bh >> sh, comp, v[AV_L], cx + 1 < wc, v[AV_A], cy + 1 < hc, v[AV_AL]);
    }
  }
}
/* the offset pass of the picture with given reconstructed parameters (rule 2): src -> rec */
static void apply_slices(int width, int height, int S, const HmoSaoBlk *recon, uint8_t *const src[3], uint8_t *const rec[3])
{
  const int wc = (width + 63) / 64, hc = (height + 63) / 64;
  for (int a = 0; a < wc * hc; a++) {
    const int cx = a % wc, cy = a / wc, x0 = cx * 64, y0 = cy * 64;
    const int bw = x0 + 64 > width ? width - x0 : 64, bh = y0 + 64 > height ? height - y0 : 64;
    int v[8];
    slice_avail8(a, wc, hc, S, v);
    for (int comp = 0; comp < 3; comp++) {
      const HmoSaoOffset *p = &recon[a].c[comp];
      if (p->mode == SAO_OFF) continue;
      const int sh = comp ? 1 : 0, stride = width >> sh;
      const size_t o = (size_t)(y0 >> sh) * stride + (x0 >> sh);
      offset_block8(p->type, p->offset, src[comp] + o, rec[comp] + o, stride, bw >> sh, bh >> sh, v);
    }
  }
}
/* the offset pass alone: recon = reconstructed parameters (mode off / new with de-quantised offsets), in place on rec */
void lf_ref_sao_apply_slices(int width, int height, int slice_ctus, int cross, const HmoSaoBlk *recon, uint8_t *const rec[3])
{
  const int n = ((width + 63) / 64) * ((height + 63) / 64), S = cross ? n : slice_len(n, slice_ctus);
  uint8_t *src[3];
  for (int comp = 0; comp < 3; comp++) {
    const size_t sz = (size_t)(width >> (comp ? 1 : 0)) * (size_t)(height >> (comp ? 1 : 0));
    src[comp] = (uint8_t *)malloc(sz); memcpy(src[comp], rec[comp], sz);
  }
  apply_slices(width, height, S, recon, src, rec);
  for (int comp = 0; comp < 3; comp++) free(src[comp]);
}

/* hmo_sao_picture with rules 2 and 3; recon_out (may be NULL): the reconstructed parameters */
void lf_ref_sao_slices(int width, int height, int slice_ctus, int cross, int qp, int slice_type, const double lambda[3], const int enabled[3],
                       const uint8_t *const org[3], uint8_t *const rec[3], HmoSaoBlk *coded, HmoSaoStat *stats_out, int off_count[3], HmoSaoBlk *recon_out)
{
  hmo_init_tables();
  const int wc = (width + 63) / 64, hc = (height + 63) / 64, n = wc * hc, S = cross ? n : slice_len(n, slice_ctus);
  uint8_t *src[3];
  for (int comp = 0; comp < 3; comp++) {
    const size_t sz = (size_t)(width >> (comp ? 1 : 0)) * (size_t)(height >> (comp ? 1 : 0));
    src[comp] = (uint8_t *)malloc(sz); memcpy(src[comp], rec[comp], sz);
  }
  HmoSaoStat *stats = stats_out ? stats_out : (HmoSaoStat *)malloc(sizeof(HmoSaoStat) * (size_t)n * 3);
  stats_slices(width, height, S, org, src, stats);
  HmoSaoBlk *recon = (HmoSaoBlk *)calloc((size_t)n, sizeof(HmoSaoBlk));
  SaoCab goon;
  static const int init_type[3] = { 160, 185, 200 };
  goon.ctx[0] = ctx_from_init(153, qp);
  goon.ctx[1] = ctx_from_init(init_type[slice_type == HMO_SLICE_I ? 2 : 1], qp);
  goon.frac = 0;
  const int allOff = !enabled[0] && !enabled[1] && !enabled[2];
  for (int a = 0; a < n; a++) {                                /* rule 4: the oracle's walk */
    if (allOff) { memset(&coded[a], 0, sizeof(coded[a])); continue; }
    const SaoCab cur = goon;
    SaoCab next = goon;
    const int cx = a % wc, cy = a / wc;
    const int sliceStart = slice_ctus > 0 ? (a / slice_ctus) * slice_ctus : 0;
    const HmoSaoBlk *merge[2] = { NULL, NULL };
    if (cy > 0 && a - wc >= sliceStart) merge[1] = &recon[a - wc];
    if (cx > 0 && a - 1 >= sliceStart) merge[0] = &recon[a - 1];
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
  }
  apply_slices(width, height, S, recon, src, rec);
  if (off_count) for (int comp = 0; comp < 3; comp++) { off_count[comp] = 0; for (int a = 0; a < n; a++) off_count[comp] += recon[a].c[comp].mode == SAO_OFF; }
  if (recon_out) memcpy(recon_out, recon, sizeof(HmoSaoBlk) * (size_t)n);
  free(recon);
  if (!stats_out) free(stats);
  for (int comp = 0; comp < 3; comp++) free(src[comp]);
}
