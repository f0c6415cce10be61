/*
 * fcu_host.h -- host-side derivation of the per-chain parameters that HM computes once per
 * slice with libm (lambda, sqrt(lambda), chroma distortion weight, RDOQ lambdas, RDOQ error
 * scales, sign-hiding rdFactor).  They are handed to the kernels as f64/i64 bit patterns so
 * that no transcendental is ever evaluated on the device.
 * Also the host-side fills of the chain descriptor (chain_bind ... wpp_bind_row, tile_bind), the one copy
 * libfcu.so and the test-only emulators bind a chain with.
 */
#pragma once
#include <math.h>
#include "fcu_engine.h"

namespace fcu {

inline void fill_params(Params &p, int width, int height, const fcu_frame_params &fp)
{
  p.width = width; p.height = height; p.qp = fp.qp; p.slice_ctus = fp.slice_ctus;
  p.slice_type = fp.slice_type; p.search_range = fp.search_range; p.fast_enc = fp.fast_enc; p.had_me = fp.hadamard_me;
  p.fast_search = fp.fast_search; p.rdoq = fp.rdoq; p.rdoq_ts = fp.rdoq_ts; p.tmvp = fp.tmvp; p.amp = fp.amp != 0;
  p.cabac_b_table = fp.slice_type == FCU_SLICE_P && fp.cabac_b_table != 0;
  p.fdm = fp.fast_merge_decision; p.max_merge_cand = fp.max_merge_cand > 0 ? (fp.max_merge_cand > 5 ? 5 : fp.max_merge_cand) : 5;
  p.transform_skip = fp.transform_skip; p.ts_fast = fp.transform_skip_fast;
  p.sign_hiding = fp.sign_hiding; p.strong_smoothing = fp.strong_intra_smoothing;
  /* chroma QP: g_aucChromaScale[CHROMA_420] (TLibCommon/TComRom.cpp:507), offsets 0 */
  static const unsigned char chroma_scale[58] = {
    0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16, 17, 18, 19, 20, 21, 22, 23, 24, 25, 26, 27, 28, 29,
    29, 30, 31, 32, 33, 33, 34, 34, 35, 35, 36, 36, 37, 37, 38, 39, 40, 41, 42, 43, 44, 45, 46, 47, 48, 49, 50, 51 };
  p.qp_c = fp.qp < 0 ? fp.qp : chroma_scale[fp.qp > 57 ? 57 : fp.qp];
  if (fp.lambda > 0.0) {
    const double w = fp.chroma_weight > 0.0 ? fp.chroma_weight : pow(2.0, (fp.qp - p.qp_c) / 3.0);     /* setUpLambda, TEncSlice.cpp:496-524 */
    p.lambda = fp.lambda; p.sqrt_lambda = fp.sqrt_lambda > 0.0 ? fp.sqrt_lambda : sqrt(fp.lambda); p.chroma_weight = w;
    p.rdoq_lambda[0] = fp.rdoq_lambda[0] > 0.0 ? fp.rdoq_lambda[0] : fp.lambda;
    p.rdoq_lambda[1] = fp.rdoq_lambda[1] > 0.0 ? fp.rdoq_lambda[1] : fp.lambda / w;
    p.rdoq_lambda[2] = fp.rdoq_lambda[2] > 0.0 ? fp.rdoq_lambda[2] : fp.lambda / w;
  } else {
    /* TEncSlice::initEncSlice, I slice: lambda = 0.57 * 2^((QP-12)/3)  (TEncSlice.cpp:686-706) */
    const double lambda = 0.57 * pow(2.0, ((double)fp.qp - 12) / 3.0);
    const double w = pow(2.0, (fp.qp - p.qp_c) / 3.0);             /* setUpLambda, TEncSlice.cpp:496-524 */
    p.lambda = lambda; p.sqrt_lambda = sqrt(lambda); p.chroma_weight = w;
    p.rdoq_lambda[0] = lambda; p.rdoq_lambda[1] = lambda / w; p.rdoq_lambda[2] = lambda / w;
  }
  p.lambda_motion_sad = (uint32_t)floor(65536.0 * sqrt(p.lambda));      /* TComRdCost::setLambda, TComRdCost.cpp:194-219 */
  for (int ch = 0; ch < 2; ch++) {
    const int qp = ch ? p.qp_c : p.qp, per = qp / 6, rem = qp % 6;
    static const int quant_scales[6] = { 26214, 23302, 20560, 18396, 16384, 14564 };
    static const int inv_quant_scales[6] = { 40, 45, 51, 57, 64, 72 };
    for (int l = 0; l < 4; l++) {
      /* setErrScaleCoeff, TComTrQuant.cpp:3018-3040: 2^15 * 2^(-2*transformShift) / q / q */
      const int tshift = 15 - 8 - (l + 2);
      double e = (double)(1 << 15);
      e = e * ldexp(1.0, -2 * tshift);
      e = e / quant_scales[rem] / quant_scales[rem] / 1;
      p.err_scale[ch][l] = e;
    }
    /* rdFactor of sign-bit hiding, TComTrQuant.cpp:2444-2447 (lambda = m_dLambda of the component) */
    const double invQ = (double)inv_quant_scales[rem];
    const double lam = p.rdoq_lambda[ch ? 1 : 0];
    p.rd_factor[ch] = (long long)(invQ * invQ * (double)(1 << (2 * per)) / lam / 16 / 1 + 0.5);
  }
}

inline void default_frame_params(fcu_frame_params &fp, int qp)
{
  memset(&fp, 0, sizeof(fp));
  fp.qp = qp; fp.slice_ctus = 0; fp.transform_skip = 1; fp.transform_skip_fast = 1; fp.sign_hiding = 1; fp.strong_intra_smoothing = 1;
  fp.slice_type = FCU_SLICE_I; fp.search_range = 64; fp.fast_enc = 1; fp.hadamard_me = 1; fp.fast_merge_decision = 1; fp.max_merge_cand = 5; fp.fast_search = 0; fp.tmvp = 0; fp.rdoq = 1; fp.rdoq_ts = 1; fp.amp = 0;
}
/* TEncSlice::initEncSlice for HM's lowdelay_P GOP table (GOPSize 4): slice type, QP = base + offset, lambda =
 * QPFactor * 2^((QP-12)/3), x Clip3(2, 4, (QP-12)/6) at temporal depth > 0 (POC % 4 != 0); the I picture's factor is
 * 0.57 * (1 - 0.05 * (GOPSize - 1)) (TEncSlice.cpp:560-740) */
inline void ldp_slice(fcu_frame_params &fp, int base_qp, int poc)
{
  static const int qp_off[4] = { 3, 2, 3, 1 };
  static const double qp_fac[4] = { 0.4624, 0.4624, 0.4624, 0.578 };
  default_frame_params(fp, base_qp);
  if (poc == 0) { fp.lambda = 0.57 * (1.0 - 0.05 * 3) * pow(2.0, ((double)base_qp - 12) / 3.0); return; }
  const int g = (poc - 1) % 4, qp = base_qp + qp_off[g];
  double lambda = qp_fac[g] * pow(2.0, ((double)qp - 12) / 3.0);
  if (poc % 4 != 0) { double f = ((double)qp - 12) / 6.0; f = f < 2.0 ? 2.0 : (f > 4.0 ? 4.0 : f); lambda *= f; }
  fp.slice_type = FCU_SLICE_P; fp.qp = qp; fp.lambda = lambda;
}

/* ---- The host-side fills of the chain descriptor.  Plain pointers in, fields out, no HIP call: the entry points of libfcu.so
 * (fcu_kernels.hip: the checks, the error texts, the copies to the device) and the test-only emulator drivers (tests/emu, built
 * with -DFCU_EMU) bind a chain through these functions and through nothing else. */

/* fcu_chain_begin: a zeroed descriptor, the slice's parameters, the planes of a width x height picture and its output array;
 * the chain's range is the whole picture */
inline void chain_bind(Chain &h, int width, int height, const fcu_frame_params &fp,
                       const uint8_t *oy, const uint8_t *ou, const uint8_t *ov, uint8_t *ry, uint8_t *ru, uint8_t *rv, fcu_ctu_out *out)
{
  memset(&h, 0, sizeof(h));
  fill_params(h.p, width, height, fp);
  h.org[0] = oy; h.org[1] = ou; h.org[2] = ov; h.rec[0] = ry; h.rec[1] = ru; h.rec[2] = rv;
  h.stride[0] = width; h.stride[1] = h.stride[2] = width / 2;
  h.out = out;
  h.w_ctu = (width + 63) / 64; h.h_ctu = (height + 63) / 64; h.n_ctu = h.w_ctu * h.h_ctu;
  h.next_ctu = 0; h.end_ctu = h.n_ctu;
  h.tile_x0 = 0; h.tile_y0 = 0; h.tile_w = h.w_ctu; h.tile_h = h.h_ctu;     /* no tiles: the tile is the picture */
}

/* list 0 of a bound P chain: pad_planes[3r .. 3r+2] = first byte of the padded Y, U, V planes of RefPicList0[r] (luma border
 * FCU_REF_MARGIN), ref_pocs[r] their POCs, cur_poc the picture's.  Writes ref / ref_stride, refs[r] and ref_poc[r] for r < n_ref,
 * n_ref, poc, and the collocated picture = RefPicList0[0] with col_ref_poc[0] = its POC - 1; the slots of col_ref_poc past 0
 * stay as they are (chain_set_collocated_pocs names them).  fcu_chain_set_reference is the one-picture form: POC 0 seen from
 * POC 1, so no vector is ever scaled. */
inline void chain_set_list0(Chain &h, int n_ref, const uint8_t *const *pad_planes, const int *ref_pocs, int cur_poc)
{
  const int m = FCU_REF_MARGIN, sy = h.p.width + 2 * m, sc = h.p.width / 2 + m;
  h.ref_stride[0] = sy; h.ref_stride[1] = h.ref_stride[2] = sc;
  for (int r = 0; r < n_ref; r++) {
    h.refs[r][0] = pad_planes[3 * r] + (size_t)m * sy + m;
    h.refs[r][1] = pad_planes[3 * r + 1] + (size_t)(m / 2) * sc + m / 2; h.refs[r][2] = pad_planes[3 * r + 2] + (size_t)(m / 2) * sc + m / 2;
    h.ref_poc[r] = ref_pocs[r];
  }
  for (int k = 0; k < 3; k++) h.ref[k] = h.refs[0][k];
  h.n_ref = n_ref; h.poc = cur_poc; h.col_poc = ref_pocs[0]; h.col_ref_poc[0] = ref_pocs[0] - 1;
}

/* fcu_chain_set_collocated_pocs: the POCs the collocated picture's own list 0 named (slots past n: col_poc - 1).  false = a slot
 * holds the collocated picture's own POC (the slots before it are written) */
inline bool chain_set_collocated_pocs(Chain &h, int col_poc, const int *col_ref_pocs, int n)
{
  h.col_poc = col_poc;
  for (int k = 0; k < FCU_MAX_REF; k++) { h.col_ref_poc[k] = k < n ? col_ref_pocs[k] : col_poc - 1; if (h.col_ref_poc[k] == col_poc) return false; }
  return true;
}

/* fcu_chain_set_decision: the fork's decision block; the verification counters start from zero */
inline void chain_set_decision(Chain &h, int state, int depth_exception, const int16_t *obf, const uint8_t *sw_skip, const uint8_t *sw_term)
{
  h.dec_state = state; h.depth_exception = depth_exception != 0; h.obf = obf; h.obf_stride = h.p.width / 4;
  for (int d = 0; d < 4; d++) { h.sw_skip[d] = sw_skip[d] != 0; h.sw_term[d] = sw_term[d] != 0; }
  memset(h.ver, 0, sizeof(h.ver));
}

/* ---- WaveFrontSynchro on pictures cut into slices of whole CTU rows (fcu_wpp_begin_slices): the rules of the binding,
 * shared by libfcu.so and the test-only emulator driver.
 * wpp_slice_ctus: SliceArgument of a picture W CTUs wide whose slices hold slice_rows rows; fp_slice_ctus, what the caller's
 * frame parameters name, must be 0 or exactly that (a slice that starts mid-row is not supported).  -1 = invalid. */
inline int wpp_slice_ctus(int W, int slice_rows, int fp_slice_ctus)
{
  if (W < 1 || slice_rows < 1 || (long long)slice_rows * W > 0x7fffffffll) return -1;
  const int sl = slice_rows * W;
  return (fp_slice_ctus == 0 || fp_slice_ctus == sl) ? sl : -1;
}
/* row (of the picture) that row r waits for and loads its contexts from: r - 1, or -1 for a row that starts a slice -- row 0,
 * and with slice_rows >= 1 every slice_rows-th row.  slice_rows 0 = one slice. */
inline int wpp_row_above(int r, int slice_rows) { return (r == 0 || (slice_rows > 0 && r % slice_rows == 0)) ? -1 : r - 1; }
/* the WPP part of the descriptor of row r of a picture W CTUs wide whose rows are chains [first_chain, ...): its CTU range, the
 * chain it waits on and the sync slots (`sync` = slot 0 of the context's slot array, one slot of WPP_SYNC_BYTES per chain).
 * The one place that fills these fields, for libfcu.so's binder and for the emulator driver (tests/emu/wpp_emu.cpp) alike. */
inline void wpp_bind_row(Chain &h, int r, int W, int slice_rows, int first_chain, uint8_t *sync)
{
  const int ra = wpp_row_above(r, slice_rows);
  h.next_ctu = r * W; h.end_ctu = (r + 1) * W;
  h.wpp = 1; h.wpp_above = ra >= 0 ? first_chain + ra : -1;
  h.wpp_sync_in = ra >= 0 ? sync + (size_t)WPP_SYNC_BYTES * (first_chain + ra) : nullptr;
  h.wpp_sync_out = sync + (size_t)WPP_SYNC_BYTES * (first_chain + r);
}

/* ---- Tiles of a one-slice picture (fcu_tiles_begin / fcu_wpp_begin_tiles): the rules of the binding, shared by libfcu.so and
 * the test-only emulator driver.
 * tile_grid: TComPicSym::initTiles with TileUniformSpacing -- column i spans the CTU columns [i * W / C, (i + 1) * W / C), rows
 * likewise.  col_bd receives n_cols + 1 boundaries, row_bd n_rows + 1 (either may be null).  false = no grid: a count below 1,
 * or more columns / rows than the picture has CTU columns / rows (a tile would be empty). */
inline bool tile_grid(int W, int H, int n_cols, int n_rows, int *col_bd, int *row_bd)
{
  if (W < 1 || H < 1 || n_cols < 1 || n_rows < 1 || n_cols > W || n_rows > H) return false;
  if (col_bd) for (int i = 0; i <= n_cols; i++) col_bd[i] = (int)((long long)i * W / n_cols);
  if (row_bd) for (int i = 0; i <= n_rows; i++) row_bd[i] = (int)((long long)i * H / n_rows);
  return true;
}
/* chains a picture of W x H CTUs needs as n_cols x n_rows tiles: one per tile, or with WaveFrontSynchro inside the tiles one per
 * CTU row of every tile (= n_cols x H).  -1 = no such grid. */
inline int tile_chains(int W, int H, int n_cols, int n_rows, int wpp)
{
  if (!tile_grid(W, H, n_cols, n_rows, nullptr, nullptr)) return -1;
  return wpp ? n_cols * H : n_cols * n_rows;
}
/* what the tile binders refuse in the frame parameters: SliceMode 1 together with tiles, and TMVP across tile columns (HM's
 * collocated bottom-right candidate reads across the tile edge) */
inline bool tile_params_ok(const fcu_frame_params &fp, int n_cols) { return fp.slice_ctus == 0 && !(fp.tmvp && n_cols > 1); }
/* the tile part of a descriptor chain_bind has filled: the rectangle, and the chain's range = the whole tile, counted inside it */
inline void tile_bind(Chain &h, int x0, int y0, int w, int hh)
{
  h.tile_x0 = x0; h.tile_y0 = y0; h.tile_w = w; h.tile_h = hh;
  h.next_ctu = 0; h.end_ctu = w * hh;
}
/* WaveFrontSynchro inside a tile: row r of the tile tile_bind gave the descriptor, as chain `chain`; the rows of a tile are
 * consecutive chains top to bottom, so the row above is chain - 1.  Row 0 of a tile is bound as a row that starts a slice is:
 * nothing above, no slot to read (wpp_bind_row). */
inline void wpp_bind_tile_row(Chain &h, int r, int chain, uint8_t *sync)
{
  h.next_ctu = r * h.tile_w; h.end_ctu = (r + 1) * h.tile_w;
  h.wpp = 1; h.wpp_above = r > 0 ? chain - 1 : -1;
  h.wpp_sync_in = r > 0 ? sync + (size_t)WPP_SYNC_BYTES * (chain - 1) : nullptr;
  h.wpp_sync_out = sync + (size_t)WPP_SYNC_BYTES * chain;
}
/* picture address of position `pos` of the chain's tile (what compress_ctu derives on the device) */
inline int tile_ctu_addr(const Chain &h, int pos) { return (h.tile_y0 + pos / h.tile_w) * h.w_ctu + h.tile_x0 + pos % h.tile_w; }
inline bool tile_is_picture(const Chain &h) { return h.tile_x0 == 0 && h.tile_y0 == 0 && h.tile_w == h.w_ctu && h.tile_h == h.h_ctu; }
inline bool tile_is_last(const Chain &h) { return h.tile_x0 + h.tile_w == h.w_ctu && h.tile_y0 + h.tile_h == h.h_ctu; }

/* ---- the tile grid as the loop-filter kernels take it (fcu_deblock_tiles / fcu_sao_tiles), by value in the kernel arguments:
 * bit i of col / row = CTU column / row i is the first of a tile (bit 0 always), cross = LFCrossTileBoundaryFlag.  Two bitmasks
 * and no pointer: the kernels ask "does this CTU column / row start a tile" and nothing else, so another spacing rule is a change
 * of lf_tiles_fill alone.  256 bits each: pictures up to 256 x 256 CTUs (sao_decide's ring already ends at 255 columns). */
enum { LF_TILE_WORDS = 4, LF_TILE_MAX_CTUS = 64 * LF_TILE_WORDS };
struct LfTiles { uint64_t col[LF_TILE_WORDS], row[LF_TILE_WORDS]; int32_t cross, pad; };
/* false = no such grid (tile_grid), a picture beyond 256 CTUs in either direction, or a flag outside {0, 1} */
inline bool lf_tiles_fill(LfTiles &T, int W, int H, int n_cols, int n_rows, int cross)
{
  if (!tile_grid(W, H, n_cols, n_rows, nullptr, nullptr) || W > LF_TILE_MAX_CTUS || H > LF_TILE_MAX_CTUS || (cross != 0 && cross != 1)) return false;
  for (int k = 0; k < LF_TILE_WORDS; k++) { T.col[k] = 0; T.row[k] = 0; }
  for (int i = 0; i < n_cols; i++) { const int b = (int)((long long)i * W / n_cols); T.col[b >> 6] |= (uint64_t)1 << (b & 63); }
  for (int i = 0; i < n_rows; i++) { const int b = (int)((long long)i * H / n_rows); T.row[b >> 6] |= (uint64_t)1 << (b & 63); }
  T.cross = cross; T.pad = 0;
  return true;
}
/* does CTU column / row i start a tile?  The word is picked by selects, not by an address: the masks stay in registers. */
FCU_DEV int lf_tile_start(const uint64_t *m, int i)
{
  const uint64_t w = i < 64 ? m[0] : (i < 128 ? m[1] : (i < 192 ? m[2] : m[3]));
  return (int)((w >> (i & 63)) & 1u);
}

/* PSNR of a plane of n 8-bit samples from its sum of squared differences, as TEncGOP::xCalculateAddPSNR prints it
 * (TEncGOP.cpp:2254-2256): the reference value 255 * 255 * n in double precision, 999.99 for an exact reconstruction */
inline double report_psnr(uint64_t ssd, uint64_t n)
{
  const double ref = 255.0 * 255.0 * (double)n;
  return ssd ? 10.0 * log10(ref / (double)ssd) : 999.99;
}

} // namespace fcu
