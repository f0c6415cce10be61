/*
 * fcu_host.h -- host-side derivation of the per-chain parameters that HM computes once per
 * slice with libm (lambda, sqrt(lambda), chroma distortion weight, RDOQ lambdas, RDOQ error
 * scales, sign-hiding rdFactor).  They are handed to the kernels as f64/i64 bit patterns so
 * that no transcendental is ever evaluated on the device.
 * Also the host-side fills of the chain descriptor (chain_bind ... wpp_bind_row, tile_bind) and, at the end, HostState: the
 * host state machine of libfcu.so -- every argument and state rule of the chain entry points, the one picture binder and the
 * two launch guards, on the host descriptors alone.  No HIP header, no HIP call: libfcu.so (fcu_kernels.hip adds the device
 * copies and the launches), the test-only emulators and tests/emu/host_emu.cpp share this one copy, and the CPU suite runs the
 * rules (tests/test_host_rules.py).
 */
#pragma once
#include <math.h>
#include <stddef.h>
#include <string>
#include <vector>
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
 * (HostState below: the checks and the error texts; fcu_kernels.hip: the copies to the device) and the test-only emulator drivers (tests/emu, built
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

/* ---- what cuts the picture for a loop-filter kernel: the compile-time variant (the template argument CUT of fcu_deblock.h and
 * fcu_sao.h).  LF_CUT_TILES is 1: the variants with tiles used to be `true` of a bool. */
enum { LF_CUT_NONE = 0, LF_CUT_TILES = 1, LF_CUT_SLICES = 2 };
/* ---- the slices as the loop-filter kernels take them (fcu_deblock_slices / fcu_sao_slices) with LFCrossSliceBoundaryFlag 0.
 * A slice is slice_ctus consecutive CTUs in raster order, the last one what is left, so the length is the whole description: no
 * table and no limit on the picture.  CTU a lies in [a - a % S, min(a - a % S + S, n_ctu)). */
struct LfSlices { int32_t slice_ctus; };
/* CTUs per slice as the filters count them: 0, or the picture's CTU count and more, is one slice */
inline int lf_slice_len(int n_ctu, int slice_ctus) { return slice_ctus <= 0 || slice_ctus > n_ctu ? n_ctu : slice_ctus; }
/* true = the slice variants run (S filled in); false = LFCrossSliceBoundaryFlag 1 or one slice: the picture filters as
 * fcu_deblock / fcu_sao filter it, by their kernels */
inline bool lf_slices_fill(LfSlices &S, int n_ctu, int slice_ctus, int cross)
{
  S.slice_ctus = lf_slice_len(n_ctu, slice_ctus);
  return cross == 0 && S.slice_ctus < n_ctu;
}

/* PSNR of a plane of n 8-bit samples from its sum of squared differences, as TEncGOP::xCalculateAddPSNR prints it
 * (TEncGOP.cpp:2254-2256): the reference value 255 * 255 * n in double precision, 999.99 for an exact reconstruction */
inline double report_psnr(uint64_t ssd, uint64_t n)
{
  const double ref = 255.0 * 255.0 * (double)n;
  return ssd ? 10.0 * log10(ref / (double)ssd) : 999.99;
}

/* ---- The picture hash (fcu_hash.h, fcu_picture_hash): the arithmetic of HM's picture CRC (compCRC, TComPicYuvMD5.cpp:89-127) in
 * GF(2)[x] mod P, P = x^16 + x^12 + x^5 + 1.  compCRC shifts the message bits in at the low end, so a state is a polynomial of
 * degree < 16 and one message bit b takes s to s x + b: a message M of n bits takes s to s x^n + M(x), and the digest is that
 * state times x^16 (the sixteen flushed zero bits).  Hence for a message AB: state(AB, s) = state(A, s) x^|B| + state(B, 0) -- the
 * fold the kernels use; the initial state contributes 0xffff x^n, which is host arithmetic (crc_adv).  All constexpr: the kernels
 * take their multipliers x^n as compile-time constants, and the byte table is computed from the polynomial. */
enum { CRC_POLY = 0x1021, CRC_INIT = 0xffff };
/* a b mod P */
constexpr uint32_t crc_mul(uint32_t a, uint32_t b)
{
  uint32_t r = 0;
  for (int i = 0; i < 16; i++) {
    if ((b >> i) & 1u) r ^= a;
    a = ((a << 1) & 0xffffu) ^ ((a & 0x8000u) ? (uint32_t)CRC_POLY : 0u);
  }
  return r;
}
/* x^n mod P */
constexpr uint32_t crc_xpow(uint64_t n)
{
  uint32_t r = 1, sq = 2;
  for (; n; n >>= 1) { if (n & 1u) r = crc_mul(r, sq); sq = crc_mul(sq, sq); }
  return r;
}
/* state s after n_bits zero bits */
constexpr uint32_t crc_adv(uint32_t s, uint64_t n_bits) { return crc_mul(s, crc_xpow(n_bits)); }
/* entry h of the byte table: h x^16 mod P, the part of a state that leaves the register when a byte is shifted in */
constexpr uint16_t crc_tab_entry(uint32_t h) { return (uint16_t)crc_mul(h, crc_xpow(16)); }
struct CrcTab { uint16_t t[256]; };
constexpr CrcTab crc_make_tab() { CrcTab T = {}; for (uint32_t h = 0; h < 256; h++) T.t[h] = crc_tab_entry(h); return T; }
/* state s after the byte v: s x^8 + v */
constexpr uint32_t crc_byte(const CrcTab &T, uint32_t s, uint32_t v) { return ((s << 8) & 0xffffu) ^ v ^ T.t[s >> 8]; }
/* the serial definition on the host: the state after n bytes, and the digest of a whole message */
inline uint32_t crc_bytes(uint32_t s, const uint8_t *p, size_t n)
{
  static constexpr CrcTab T = crc_make_tab();
  for (size_t i = 0; i < n; i++) s = crc_byte(T, s, p[i]);
  return s;
}
inline uint32_t crc_digest(const uint8_t *p, size_t n) { return crc_adv(crc_bytes(CRC_INIT, p, n), 16); }

/* fcu_hash_string: digestToString (TComPicYuvMD5.cpp:209-225) of one kind of a record -- the three planes' digests in hex, joined
 * by ','.  Returns the length, FCU_ERR_ARG for a kind that is not exactly one of the three bits or a buffer too short for the
 * string and its terminator. */
inline int hash_string(const fcu_pic_hash *h, int kind, char *buf, int buf_len)
{
  if (!h || !buf) return FCU_ERR_ARG;
  const uint8_t *d; int n;
  if (kind == FCU_HASH_MD5) { d = &h->md5[0][0]; n = 16; }
  else if (kind == FCU_HASH_CRC) { d = &h->crc[0][0]; n = 2; }
  else if (kind == FCU_HASH_CHECKSUM) { d = &h->checksum[0][0]; n = 4; }
  else return FCU_ERR_ARG;
  const int len = 3 * 2 * n + 2;
  if (buf_len < len + 1) return FCU_ERR_ARG;
  static const char hex[] = "0123456789abcdef";
  char *o = buf;
  for (int pos = 0; pos < 3 * n; pos++) {
    if (pos % n == 0 && pos != 0) *o++ = ',';
    *o++ = hex[d[pos] >> 4]; *o++ = hex[d[pos] & 15];
  }
  *o = 0;
  return len;
}
/* fcu_picture_hash: what it refuses, with the argument named; FCU_OK otherwise */
inline int hash_args_check(int n_pics, int kinds, const uint8_t *const *dev_planes, const fcu_pic_hash *host_hashes, std::string &err)
{
  const char *bad = nullptr;
  if (n_pics < 1) bad = "n_pics must be at least 1";
  else if (kinds == 0 || (kinds & ~(FCU_HASH_MD5 | FCU_HASH_CRC | FCU_HASH_CHECKSUM))) bad = "kinds is a non-empty mask of FCU_HASH_MD5 | FCU_HASH_CRC | FCU_HASH_CHECKSUM";
  else if (!dev_planes) bad = "dev_planes is null";
  else if (!host_hashes) bad = "host_hashes is null";
  if (bad) { err = std::string("fcu_picture_hash: ") + bad; return FCU_ERR_ARG; }
  for (int i = 0; i < 3 * n_pics; i++) if (!dev_planes[i]) { err = "fcu_picture_hash: dev_planes[" + std::to_string(i) + "] is null"; return FCU_ERR_ARG; }
  return FCU_OK;
}

/* ---- Decision maps and split match (fcu_maps.h, fcu_decision_maps, fcu_split_match): geometry and argument rules.
 * maps_field_offset: byte offset of the 256-byte array of FCU_MAP_* id inside fcu_ctu_out, -1 for an unknown id */
inline int maps_field_offset(int id)
{
  switch (id) {
  case FCU_MAP_DEPTH: return (int)offsetof(fcu_ctu_out, depth);
  case FCU_MAP_PART_SIZE: return (int)offsetof(fcu_ctu_out, part_size);
  case FCU_MAP_PRED_MODE: return (int)offsetof(fcu_ctu_out, pred_mode);
  case FCU_MAP_SKIP: return (int)offsetof(fcu_ctu_out, skip);
  case FCU_MAP_MERGE_FLAG: return (int)offsetof(fcu_ctu_out, merge_flag);
  case FCU_MAP_MERGE_IDX: return (int)offsetof(fcu_ctu_out, merge_idx);
  case FCU_MAP_TR_IDX: return (int)offsetof(fcu_ctu_out, tr_idx);
  case FCU_MAP_CBF_Y: case FCU_MAP_CBF_CB: case FCU_MAP_CBF_CR: return (int)offsetof(fcu_ctu_out, cbf) + FCU_NPART * (id - FCU_MAP_CBF_Y);
  case FCU_MAP_TSKIP_Y: case FCU_MAP_TSKIP_CB: case FCU_MAP_TSKIP_CR: return (int)offsetof(fcu_ctu_out, tskip) + FCU_NPART * (id - FCU_MAP_TSKIP_Y);
  case FCU_MAP_INTRA_DIR_LUMA: case FCU_MAP_INTRA_DIR_CHROMA: return (int)offsetof(fcu_ctu_out, intra_dir) + FCU_NPART * (id - FCU_MAP_INTRA_DIR_LUMA);
  case FCU_MAP_QP: return (int)offsetof(fcu_ctu_out, qp);
  case FCU_MAP_INTER_DIR: return (int)offsetof(fcu_ctu_out, inter_dir);
  case FCU_MAP_MVP_IDX: return (int)offsetof(fcu_ctu_out, mvp_idx);
  case FCU_MAP_REF_IDX: return (int)offsetof(fcu_ctu_out, ref_idx);
  default: return -1;
  }
}
/* what the kernels need to know of a batch: the picture, the arrays to read, and where level d of a picture's label / N_OBF
 * maps starts (lvl_off[4] = their elements per picture) */
struct MapsGeom {
  int width, height, w_ctu, n_ctu, n_fields;
  int lvl_w[4], lvl_off[5];
  uint16_t field_off[FCU_MAP_FIELDS];
};
inline MapsGeom maps_geom(int width, int height, int n_fields, const int *field_ids)
{
  MapsGeom G = {};
  G.width = width; G.height = height; G.w_ctu = (width + 63) / 64; G.n_ctu = G.w_ctu * ((height + 63) / 64); G.n_fields = n_fields;
  for (int d = 0; d < 4; d++) {
    const int s = 64 >> d;
    G.lvl_w[d] = (width + s - 1) / s;
    G.lvl_off[d + 1] = G.lvl_off[d] + G.lvl_w[d] * ((height + s - 1) / s);
  }
  for (int k = 0; k < n_fields; k++) G.field_off[k] = (uint16_t)maps_field_offset(field_ids[k]);
  return G;
}
/* fcu_chain_set_labels: the picture's label array (null: none) and the offsets and row lengths of its four levels -- the geometry
 * of the label maps of fcu_decision_maps, from the one function that knows it */
inline void chain_set_labels(Chain &h, const int8_t *labels)
{
  const MapsGeom G = maps_geom(h.p.width, h.p.height, 0, nullptr);
  h.labels = labels;
  for (int d = 0; d < 4; d++) { h.lbl_off[d] = G.lvl_off[d]; h.lbl_w[d] = G.lvl_w[d]; }
}
/* fcu_labels_from_rasters: what it refuses */
inline int labels_args_check(int n_pics, const void *dev_depth, const void *dev_labels, std::string &err)
{
  const char *bad = n_pics < 1 ? "n_pics must be at least 1" : (!dev_depth ? "dev_depth is null" : (!dev_labels ? "dev_labels is null" : nullptr));
  if (bad) { err = std::string("fcu_labels_from_rasters: ") + bad; return FCU_ERR_ARG; }
  return FCU_OK;
}
/* fcu_label_score / fcu_trace_maps: what they refuse, with the argument named; FCU_OK otherwise */
inline int score_args_check(int n_pics, const fcu_cu_trace *const *dev_trace, const int8_t *const *dev_labels, const fcu_pic_score *host_scores, std::string &err)
{
  const std::string who = "fcu_label_score: ";
  const char *bad = nullptr;
  if (n_pics < 1) bad = "n_pics must be at least 1";
  else if (!dev_trace) bad = "dev_trace is null";
  else if (!dev_labels) bad = "dev_labels is null";
  else if (!host_scores) bad = "host_scores is null";
  if (bad) { err = who + bad; return FCU_ERR_ARG; }
  for (int i = 0; i < n_pics; i++) {
    if (!dev_trace[i]) { err = who + "dev_trace[" + std::to_string(i) + "] is null"; return FCU_ERR_ARG; }
    if (!dev_labels[i]) { err = who + "dev_labels[" + std::to_string(i) + "] is null"; return FCU_ERR_ARG; }
  }
  return FCU_OK;
}
inline int trace_maps_args_check(int n_pics, const fcu_cu_trace *const *dev_trace, const void *dev_labels, const void *dev_j0, const void *dev_j1, std::string &err)
{
  const std::string who = "fcu_trace_maps: ";
  const char *bad = nullptr;
  if (n_pics < 1) bad = "n_pics must be at least 1";
  else if (!dev_trace) bad = "dev_trace is null";
  else if (!dev_labels && !dev_j0 && !dev_j1) bad = "no output is wanted (dev_labels, dev_j0 and dev_j1 null)";
  else if (((uintptr_t)dev_j0 | (uintptr_t)dev_j1) & 7) bad = "dev_j0 and dev_j1 start at multiples of 8 bytes";
  if (bad) { err = who + bad; return FCU_ERR_ARG; }
  for (int i = 0; i < n_pics; i++) if (!dev_trace[i]) { err = who + "dev_trace[" + std::to_string(i) + "] is null"; return FCU_ERR_ARG; }
  return FCU_OK;
}
/* fcu_cu_index: the record of the CU of `depth` whose first 4x4 partition is zidx (z-order) inside its CTU's FCU_CUS_PER_CTU */
inline int cu_index(int depth, int zidx) { return depth <= 0 ? 0 : depth == 1 ? 1 + (zidx >> 6) : depth == 2 ? 5 + (zidx >> 4) : 21 + (zidx >> 2); }
/* the unit the rows of the byte maps (and of the motion map) go out in: 16 bytes when every row of every map starts on 16 bytes
 * -- W4 a multiple of 16 (whole CTU columns, every map a multiple of 16 bytes) and aligned bases --, else 2-byte units, which
 * W4 even always allows; their alignment is the base's: 2, or 1 for a byte map at an odd address */
inline int maps_row_align(int width, const void *dev_bytes, const void *dev_mv)
{
  const uintptr_t a = (uintptr_t)dev_bytes | (uintptr_t)dev_mv;
  if ((width & 63) == 0 && (a & 15) == 0) return 16;
  return (a & 1) ? 1 : 2;
}
/* fcu_decision_maps: what it refuses, with the argument named; FCU_OK otherwise */
inline int maps_args_check(int n_pics, const fcu_ctu_out *const *dev_out, int n_fields, const int *field_ids, const void *dev_bytes, const void *dev_mv,
                           const void *dev_labels, const int16_t *const *dev_obf, const void *dev_nobf, std::string &err)
{
  const std::string who = "fcu_decision_maps: ";
  const char *bad = nullptr;
  if (n_pics < 1) bad = "n_pics must be at least 1";
  else if (!dev_out) bad = "dev_out is null";
  else if (n_fields < 0 || n_fields > FCU_MAP_FIELDS) bad = "n_fields is 0 .. FCU_MAP_FIELDS";
  else if (n_fields > 0 && !field_ids) bad = "field_ids is null";
  else if (n_fields > 0 && !dev_bytes) bad = "dev_bytes is null although n_fields > 0";
  else if (n_fields == 0 && dev_bytes) bad = "dev_bytes is given although n_fields is 0";
  else if (dev_nobf && !dev_obf) bad = "dev_obf is null although dev_nobf is given";
  else if (dev_obf && !dev_nobf) bad = "dev_nobf is null although dev_obf is given";
  else if (((uintptr_t)dev_mv | (uintptr_t)dev_nobf) & 1) bad = "dev_mv and dev_nobf start at even bytes";
  else if (n_fields == 0 && !dev_mv && !dev_labels && !dev_nobf) bad = "no output is wanted (n_fields 0, dev_mv, dev_labels and dev_nobf null)";
  if (bad) { err = who + bad; return FCU_ERR_ARG; }
  for (int i = 0; i < n_pics; i++) if (!dev_out[i]) { err = who + "dev_out[" + std::to_string(i) + "] is null"; return FCU_ERR_ARG; }
  for (int i = 0; dev_obf && i < n_pics; i++) if (!dev_obf[i]) { err = who + "dev_obf[" + std::to_string(i) + "] is null"; return FCU_ERR_ARG; }
  for (int k = 0; k < n_fields; k++) {
    if (maps_field_offset(field_ids[k]) < 0) { err = who + "field_ids[" + std::to_string(k) + "] = " + std::to_string(field_ids[k]) + " is no FCU_MAP_* id"; return FCU_ERR_ARG; }
    for (int j = 0; j < k; j++) if (field_ids[j] == field_ids[k]) { err = who + "field_ids[" + std::to_string(k) + "] repeats field_ids[" + std::to_string(j) + "]"; return FCU_ERR_ARG; }
  }
  return FCU_OK;
}
/* fcu_feature_count / fcu_feature_maps: F of a set mask (FCU_ERR_ARG for a mask that is empty or has other bits), and what the
 * call refuses, with the argument named; FCU_OK otherwise */
inline int feature_count(int sets)
{
  if (sets == 0 || (sets & ~(FCU_FEATSET_TMV | FCU_FEATSET_SOC))) return FCU_ERR_ARG;
  return ((sets & FCU_FEATSET_TMV) ? FCU_FEAT_TMV : 0) + ((sets & FCU_FEATSET_SOC) ? FCU_FEAT_SOC : 0);
}
inline int features_args_check(int n_pics, int sets, const uint8_t *const *dev_y, const double *host_yc, const void *dev_features, std::string &err)
{
  const std::string who = "fcu_feature_maps: ";
  const char *bad = nullptr;
  if (n_pics < 1) bad = "n_pics must be at least 1";
  else if (feature_count(sets) < 0) bad = "sets is a non-empty mask of FCU_FEATSET_TMV | FCU_FEATSET_SOC";
  else if (!dev_y) bad = "dev_y is null";
  else if ((sets & FCU_FEATSET_SOC) && !host_yc) bad = "host_yc is null although FCU_FEATSET_SOC is asked for";
  else if (!(sets & FCU_FEATSET_SOC) && host_yc) bad = "host_yc is given although FCU_FEATSET_SOC is not asked for";
  else if (!dev_features) bad = "dev_features is null";
  else if ((uintptr_t)dev_features & 3) bad = "dev_features starts at a multiple of 4 bytes";
  if (bad) { err = who + bad; return FCU_ERR_ARG; }
  for (int i = 0; i < n_pics; i++) if (!dev_y[i]) { err = who + "dev_y[" + std::to_string(i) + "] is null"; return FCU_ERR_ARG; }
  for (int i = 0; host_yc && i < n_pics * 16; i++)           /* (a Yc beyond any coefficient is a threshold nothing reaches; obf_thr must not overflow) */
    if (!(host_yc[i] >= 0.0 && host_yc[i] <= 1.0e6)) { err = who + "host_yc[" + std::to_string(i / 16) + "][" + std::to_string(i % 16) + "] is negative or not finite"; return FCU_ERR_ARG; }
  return FCU_OK;
}
/* ---- the risk-table model (include/fcu.h).  risk_q and risk_rule are the one definition of the quantised loss and of the decision
 * rule: the kernels of fcu_risk.h call them on the device, fcu_risk_table below on the host */
#if defined(__HIPCC__) && !defined(FCU_EMU)
#define FCU_HOST_DEV __host__ __device__
#else
#define FCU_HOST_DEV
#endif
/* (int64) floor(fabs(j0 - j1) * 256), clamped to 2^40 - 1; whatever is not < 2^40 -- NaN, infinity -- gives 2^40 - 1 */
FCU_HOST_DEV inline int64_t risk_q(double j0, double j1)
{
  const double s = fabs(j0 - j1) * 256.0;                    /* (exact: a power of two) */
  return s < 1099511627776.0 ? (int64_t)floor(s) : FCU_RISK_Q_MAX;
}
/* the sample test and the quantised loss of a trace record as the key tree (fcu_tree.h) takes them: true for a record with valid,
 * split_tried and whole_tried all set; *q (q may be null: the test alone) receives risk_q.  risk_train (fcu_risk.h) keeps its own
 * spelling of the same test next to the same risk_q: calling this function there changed its compiled code (register allocation
 * of the whole kernel) in every form tried, and that kernel must stay what it was.  tests/test_tree.py holds the two sample sets
 * against each other: the histograms summed over bins equal the model risk_train gives on the node array */
FCU_HOST_DEV inline bool risk_sample(uint32_t valid, uint32_t split_tried, uint32_t whole_tried, double j0, double j1, int64_t *q)
{
  if (q) *q = risk_q(j0, j1);
  return valid != 0 && split_tried != 0 && whole_tried != 0;
}
/* the fork's R0 < R1 -> TerminateCU, else Skip2Nx2N: r0 = risk[..][0] (the loss of predicting SPLIT), r1 = risk[..][1] */
FCU_HOST_DEV inline int risk_rule(int64_t r0, int64_t r1, uint32_t c0, uint32_t c1, int min_count)
{
  if ((uint64_t)c0 + c1 < (uint64_t)min_count) return FCU_LABEL_ABSENT;
  return r1 < r0 ? FCU_LABEL_NOT_SPLIT : FCU_LABEL_SPLIT;
}
/* fcu_risk_table */
inline void risk_table(const fcu_risk_model *m, int min_count, int8_t table[4][FCU_RISK_BINS])
{
  for (int d = 0; d < 4; d++) for (int x = 0; x < FCU_RISK_BINS; x++)
    table[d][x] = (int8_t)risk_rule(m->risk[d][x][0], m->risk[d][x][1], m->count[d][x][0], m->count[d][x][1], min_count);
}
/* what the three calls refuse, with the argument named; FCU_OK otherwise.  n_blocks = NL of the context's picture size */
inline int risk_null_entry(const std::string &who, const char *name, const void *const *a, int n_pics, std::string &err)
{
  for (int i = 0; i < n_pics; i++) if (!a[i]) { err = who + name + "[" + std::to_string(i) + "] is null"; return FCU_ERR_ARG; }
  return FCU_OK;
}
inline int risk_train_args_check(int n_pics, const fcu_cu_trace *const *dev_trace, const uint16_t *const *dev_keys, const void *dev_model, int accumulate, int n_blocks, std::string &err)
{
  const std::string who = "fcu_risk_train: ";
  const char *bad = nullptr;
  if (n_pics < 1) bad = "n_pics must be at least 1";
  else if (!dev_trace) bad = "dev_trace is null";
  else if (!dev_keys) bad = "dev_keys is null";
  else if (!dev_model) bad = "dev_model is null";
  else if ((uintptr_t)dev_model & 7) bad = "dev_model starts at a multiple of 8 bytes";
  else if (accumulate != 0 && accumulate != 1) bad = "accumulate is 0 or 1";
  else if ((int64_t)n_pics * n_blocks > FCU_RISK_MAX_BLOCKS) bad = "n_pics * NL is at most 2^22 in one call";
  if (bad) { err = who + bad; return FCU_ERR_ARG; }
  if (risk_null_entry(who, "dev_trace", (const void *const *)dev_trace, n_pics, err) != FCU_OK) return FCU_ERR_ARG;
  if (risk_null_entry(who, "dev_keys", (const void *const *)dev_keys, n_pics, err) != FCU_OK) return FCU_ERR_ARG;
  for (int i = 0; i < n_pics; i++) if ((uintptr_t)dev_keys[i] & 1) { err = who + "dev_keys[" + std::to_string(i) + "] starts at an even byte"; return FCU_ERR_ARG; }
  return FCU_OK;
}
inline int risk_predict_args_check(int n_pics, const uint16_t *const *dev_keys, const void *dev_model, int min_count, const void *dev_labels, std::string &err)
{
  const std::string who = "fcu_risk_predict: ";
  const char *bad = nullptr;
  if (n_pics < 1) bad = "n_pics must be at least 1";
  else if (!dev_keys) bad = "dev_keys is null";
  else if (!dev_model) bad = "dev_model is null";
  else if ((uintptr_t)dev_model & 7) bad = "dev_model starts at a multiple of 8 bytes";
  else if (min_count < 0) bad = "min_count must not be negative";
  else if (!dev_labels) bad = "dev_labels is null";
  if (bad) { err = who + bad; return FCU_ERR_ARG; }
  if (risk_null_entry(who, "dev_keys", (const void *const *)dev_keys, n_pics, err) != FCU_OK) return FCU_ERR_ARG;
  for (int i = 0; i < n_pics; i++) if ((uintptr_t)dev_keys[i] & 1) { err = who + "dev_keys[" + std::to_string(i) + "] starts at an even byte"; return FCU_ERR_ARG; }
  return FCU_OK;
}
inline int nobf_args_check(int n_pics, const int16_t *const *dev_obf, const void *dev_nobf, std::string &err)
{
  const std::string who = "fcu_nobf_maps: ";
  const char *bad = nullptr;
  if (n_pics < 1) bad = "n_pics must be at least 1";
  else if (!dev_obf) bad = "dev_obf is null";
  else if (!dev_nobf) bad = "dev_nobf is null";
  else if ((uintptr_t)dev_nobf & 1) bad = "dev_nobf starts at an even byte";
  if (bad) { err = who + bad; return FCU_ERR_ARG; }
  return risk_null_entry(who, "dev_obf", (const void *const *)dev_obf, n_pics, err);
}
/* ---- the key tree (include/fcu.h): what its calls refuse, with the argument named, and the split choice (fcu_tree_split) */
static_assert(sizeof(fcu_key_tree) == 376 && sizeof(fcu_key_tree) % 8 == 0 && offsetof(fcu_key_tree, feature) == 4 && offsetof(fcu_key_tree, thr) == 252,
              "fcu_key_tree has no implicit padding and is a multiple of 8 bytes");
/* fcu_feature_edges_check: every row of 31 edges finite and non-decreasing */
inline int tree_edges_check(const float *edges, int sets, std::string &err)
{
  const std::string who = "fcu_feature_edges_check: ";
  const int F = feature_count(sets);
  if (F < 0) { err = who + "sets is a non-empty mask of FCU_FEATSET_TMV | FCU_FEATSET_SOC"; return FCU_ERR_ARG; }
  if (!edges) { err = who + "host_edges is null"; return FCU_ERR_ARG; }
  for (int r = 0; r < 4 * F; r++) {
    const float *e = edges + (size_t)r * (FCU_TREE_BINS - 1);
    for (int k = 0; k < FCU_TREE_BINS - 1; k++)
      if (!(e[k] - e[k] == 0.0f) || (k > 0 && e[k] < e[k - 1])) {      /* (x - x is 0 for a finite x only) */
        err = who + "host_edges[" + std::to_string(r / F) + "][" + std::to_string(r % F) + "] is not finite and non-decreasing at " + std::to_string(k);
        return FCU_ERR_ARG;
      }
  }
  return FCU_OK;
}
/* a tree the kernels may walk: levels 0..5, every column -1..F-1, every threshold 0..30 */
inline const char *tree_bad(const fcu_key_tree *t, int F)
{
  if (!t) return "host_tree is null";
  if (t->levels < 0 || t->levels > FCU_TREE_MAX_LEVELS) return "host_tree->levels is 0 .. FCU_TREE_MAX_LEVELS";
  for (int d = 0; d < 4; d++) for (int i = 0; i < FCU_TREE_NODES; i++) {
    if (t->feature[d][i] < -1 || t->feature[d][i] >= F) return "host_tree->feature holds -1 or a column of the feature sets";
    if (t->thr[d][i] > FCU_TREE_BINS - 2) return "host_tree->thr is 0 .. 30";
  }
  return nullptr;
}
inline int feature_bins_args_check(int n_pics, int sets, const void *dev_features, const void *dev_edges, const void *dev_bins, int n_blocks, std::string &err)
{
  const char *bad = nullptr;
  if (n_pics < 1) bad = "n_pics must be at least 1";
  else if (feature_count(sets) < 0) bad = "sets is a non-empty mask of FCU_FEATSET_TMV | FCU_FEATSET_SOC";
  else if (!dev_features) bad = "dev_features is null";
  else if ((uintptr_t)dev_features & 3) bad = "dev_features starts at a multiple of 4 bytes";
  else if (!dev_edges) bad = "dev_edges is null";
  else if ((uintptr_t)dev_edges & 3) bad = "dev_edges starts at a multiple of 4 bytes";
  else if (!dev_bins) bad = "dev_bins is null";
  else if ((int64_t)n_pics * n_blocks > FCU_RISK_MAX_BLOCKS) bad = "n_pics * NL is at most 2^22 in one call";
  if (bad) { err = std::string("fcu_feature_bins: ") + bad; return FCU_ERR_ARG; }
  return FCU_OK;
}
inline int tree_keys_args_check(int n_pics, int sets, const void *dev_bins, const fcu_key_tree *tree, int levels, const void *dev_keys, int n_blocks, std::string &err)
{
  const char *bad = nullptr;
  if (n_pics < 1) bad = "n_pics must be at least 1";
  else if (feature_count(sets) < 0) bad = "sets is a non-empty mask of FCU_FEATSET_TMV | FCU_FEATSET_SOC";
  else if (!dev_bins) bad = "dev_bins is null";
  else if (tree_bad(tree, feature_count(sets))) bad = tree_bad(tree, feature_count(sets));
  else if (levels < 0 || levels > tree->levels) bad = "levels is 0 .. host_tree->levels";
  else if (!dev_keys) bad = "dev_keys is null";
  else if ((uintptr_t)dev_keys & 1) bad = "dev_keys starts at an even byte";
  else if ((int64_t)n_pics * n_blocks > FCU_RISK_MAX_BLOCKS) bad = "n_pics * NL is at most 2^22 in one call";
  if (bad) { err = std::string("fcu_tree_keys: ") + bad; return FCU_ERR_ARG; }
  return FCU_OK;
}
inline int tree_hist_args_check(int n_pics, int sets, int level, const fcu_cu_trace *const *dev_trace, const uint8_t *const *dev_bins, const uint16_t *const *dev_nodes,
                                const void *dev_risk, const void *dev_count, int accumulate, int n_blocks, std::string &err)
{
  const std::string who = "fcu_tree_hist: ";
  const char *bad = nullptr;
  if (n_pics < 1) bad = "n_pics must be at least 1";
  else if (feature_count(sets) < 0) bad = "sets is a non-empty mask of FCU_FEATSET_TMV | FCU_FEATSET_SOC";
  else if (level < 0 || level >= FCU_TREE_MAX_LEVELS) bad = "level is 0 .. FCU_TREE_MAX_LEVELS - 1";
  else if (!dev_trace) bad = "dev_trace is null";
  else if (!dev_bins) bad = "dev_bins is null";
  else if (!dev_nodes && level > 0) bad = "dev_nodes is null although level > 0";
  else if (!dev_risk) bad = "dev_risk is null";
  else if ((uintptr_t)dev_risk & 7) bad = "dev_risk starts at a multiple of 8 bytes";
  else if (!dev_count) bad = "dev_count is null";
  else if ((uintptr_t)dev_count & 3) bad = "dev_count starts at a multiple of 4 bytes";
  else if (accumulate != 0 && accumulate != 1) bad = "accumulate is 0 or 1";
  else if ((int64_t)n_pics * n_blocks > FCU_RISK_MAX_BLOCKS) bad = "n_pics * NL is at most 2^22 in one call";
  if (bad) { err = who + bad; return FCU_ERR_ARG; }
  if (risk_null_entry(who, "dev_trace", (const void *const *)dev_trace, n_pics, err) != FCU_OK) return FCU_ERR_ARG;
  if (risk_null_entry(who, "dev_bins", (const void *const *)dev_bins, n_pics, err) != FCU_OK) return FCU_ERR_ARG;
  if (dev_nodes && risk_null_entry(who, "dev_nodes", (const void *const *)dev_nodes, n_pics, err) != FCU_OK) return FCU_ERR_ARG;
  for (int i = 0; dev_nodes && i < n_pics; i++) if ((uintptr_t)dev_nodes[i] & 1) { err = who + "dev_nodes[" + std::to_string(i) + "] starts at an even byte"; return FCU_ERR_ARG; }
  return FCU_OK;
}
inline int tree_train_args_check(int n_pics, int sets, int levels, int min_count, const fcu_cu_trace *const *dev_trace, const uint8_t *const *dev_bins, const fcu_key_tree *tree,
                                 int n_blocks, std::string &err)
{
  const std::string who = "fcu_tree_train: ";
  const char *bad = nullptr;
  if (n_pics < 1) bad = "n_pics must be at least 1";
  else if (feature_count(sets) < 0) bad = "sets is a non-empty mask of FCU_FEATSET_TMV | FCU_FEATSET_SOC";
  else if (levels < 0 || levels > FCU_TREE_MAX_LEVELS) bad = "levels is 0 .. FCU_TREE_MAX_LEVELS";
  else if (min_count < 0) bad = "min_count must not be negative";
  else if (!dev_trace) bad = "dev_trace is null";
  else if (!dev_bins) bad = "dev_bins is null";
  else if (!tree) bad = "host_tree is null";
  else if ((int64_t)n_pics * n_blocks > FCU_RISK_MAX_BLOCKS) bad = "n_pics * NL is at most 2^22 in one call";
  if (bad) { err = who + bad; return FCU_ERR_ARG; }
  if (risk_null_entry(who, "dev_trace", (const void *const *)dev_trace, n_pics, err) != FCU_OK) return FCU_ERR_ARG;
  return risk_null_entry(who, "dev_bins", (const void *const *)dev_bins, n_pics, err);
}
/* fcu_tree_train's first step: a tree of `levels` levels with no node split */
inline void tree_clear(fcu_key_tree &t, int levels)
{
  t.levels = levels;
  for (int d = 0; d < 4; d++) for (int i = 0; i < FCU_TREE_NODES; i++) { t.feature[d][i] = -1; t.thr[d][i] = 0; }
}
/* fcu_tree_split: the nodes of `level` from that level's histograms, [4][2^level][F][32][2] each */
inline int tree_split(const int64_t *risk, const uint32_t *count, int F, int level, int min_count, fcu_key_tree *tree, std::string &err)
{
  const std::string who = "fcu_tree_split: ";
  const char *bad = nullptr;
  if (!risk) bad = "host_risk is null";
  else if (!count) bad = "host_count is null";
  else if (F < 1 || F > FCU_FEAT_TMV + FCU_FEAT_SOC) bad = "F is 1 .. 146";
  else if (level < 0 || level >= FCU_TREE_MAX_LEVELS) bad = "level is 0 .. FCU_TREE_MAX_LEVELS - 1";
  else if (min_count < 0) bad = "min_count must not be negative";
  else if (!tree) bad = "tree is null";
  if (bad) { err = who + bad; return FCU_ERR_ARG; }
  const int B = FCU_TREE_BINS, n_nodes = 1 << level;
  const int64_t need = min_count > 1 ? min_count : 1;
  /* the totals of every node, summed over every column, must agree before anything is written */
  for (int d = 0; d < 4; d++) for (int n = 0; n < n_nodes; n++) {
    int64_t R0[2] = { 0, 0 }, N0[2] = { 0, 0 };
    for (int f = 0; f < F; f++) {
      const size_t o = (((size_t)d * n_nodes + n) * F + f) * B * 2;
      int64_t R[2] = { 0, 0 }, N[2] = { 0, 0 };
      for (int b = 0; b < B; b++) for (int t = 0; t < 2; t++) {
        if (risk[o + b * 2 + t] < 0) { err = who + "host_risk holds a negative sum"; return FCU_ERR_ARG; }
        R[t] += risk[o + b * 2 + t]; N[t] += count[o + b * 2 + t];
      }
      if (f == 0) { R0[0] = R[0]; R0[1] = R[1]; N0[0] = N[0]; N0[1] = N[1]; }
      else if (R[0] != R0[0] || R[1] != R0[1] || N[0] != N0[0] || N[1] != N0[1]) {
        err = who + "the totals of depth " + std::to_string(d) + " node " + std::to_string(n) + " differ between column 0 and column " + std::to_string(f) + " (a histogram of another shape?)";
        return FCU_ERR_ARG;
      }
    }
  }
  for (int d = 0; d < 4; d++) for (int n = 0; n < n_nodes; n++) {
    int64_t R[2] = { 0, 0 }, NT = 0;
    const size_t o0 = ((size_t)d * n_nodes + n) * F * B * 2;
    for (int b = 0; b < B; b++) for (int t = 0; t < 2; t++) { R[t] += risk[o0 + b * 2 + t]; NT += count[o0 + b * 2 + t]; }
    const int64_t whole = R[0] < R[1] ? R[0] : R[1];
    int64_t best = whole; int bf = -1, bb = 0;
    for (int f = 0; f < F; f++) {
      const size_t o = o0 + (size_t)f * B * 2;
      int64_t L[2] = { 0, 0 }, NL = 0;
      for (int b = 0; b < B - 1; b++) {
        L[0] += risk[o + b * 2]; L[1] += risk[o + b * 2 + 1]; NL += (int64_t)count[o + b * 2] + count[o + b * 2 + 1];
        if (NL < need || NT - NL < need) continue;
        const int64_t a = L[0] < L[1] ? L[0] : L[1], r0 = R[0] - L[0], r1 = R[1] - L[1], loss = a + (r0 < r1 ? r0 : r1);
        if (loss < best) { best = loss; bf = f; bb = b; }      /* strictly: ties stay with the smaller f, then the smaller b */
      }
    }
    const int i = n_nodes - 1 + n;
    tree->feature[d][i] = (int16_t)bf; tree->thr[d][i] = (uint8_t)bb;
  }
  return FCU_OK;
}
/* fcu_split_match: likewise */
inline int match_args_check(int n_pics, const fcu_ctu_out *const *dev_out_a, const fcu_ctu_out *const *dev_out_b, const fcu_pic_match *host_matches, std::string &err)
{
  const std::string who = "fcu_split_match: ";
  const char *bad = nullptr;
  if (n_pics < 1) bad = "n_pics must be at least 1";
  else if (!dev_out_a) bad = "dev_out_a is null";
  else if (!dev_out_b) bad = "dev_out_b is null";
  else if (!host_matches) bad = "host_matches is null";
  if (bad) { err = who + bad; return FCU_ERR_ARG; }
  for (int i = 0; i < n_pics; i++) {
    if (!dev_out_a[i]) { err = who + "dev_out_a[" + std::to_string(i) + "] is null"; return FCU_ERR_ARG; }
    if (!dev_out_b[i]) { err = who + "dev_out_b[" + std::to_string(i) + "] is null"; return FCU_ERR_ARG; }
  }
  return FCU_OK;
}

/* ---- The byte ranges { offset, length } of the descriptor libfcu.so copies to the device on their own, named once: a setter
 * uploads the range it has written and nothing else, so a chain's position, coder state and counters on the device stay. */
struct ChainRange { size_t off, len; };
constexpr ChainRange CR_ALL = { 0, sizeof(Chain) };
constexpr ChainRange CR_REF = { offsetof(Chain, ref), 3 * sizeof(void *) + 3 * sizeof(int) };      /* ref, ref_stride */
static_assert(offsetof(Chain, ref_stride) == offsetof(Chain, ref) + 3 * sizeof(void *) && offsetof(Chain, out) >= offsetof(Chain, ref_stride) + 3 * sizeof(int), "ref / ref_stride are adjacent, out follows");
constexpr ChainRange CR_LIST0 = { offsetof(Chain, refs), offsetof(Chain, int_mv_r) - offsetof(Chain, refs) };      /* refs .. col_ref_poc: list 0 and the collocated POCs, not the search state */
static_assert(offsetof(Chain, refs) < offsetof(Chain, n_ref) && offsetof(Chain, col_ref_poc) + sizeof(int) * FCU_MAX_REF == offsetof(Chain, int_mv_r), "refs .. col_ref_poc end where int_mv_r starts");
constexpr ChainRange CR_RANGE = { offsetof(Chain, next_ctu), 2 * sizeof(int) };      /* next_ctu, end_ctu */
static_assert(offsetof(Chain, end_ctu) == offsetof(Chain, next_ctu) + sizeof(int), "next_ctu / end_ctu are adjacent");
constexpr ChainRange CR_DECISION = { offsetof(Chain, dec_state), sizeof(Chain) - offsetof(Chain, dec_state) };      /* dec_state .. the end */
static_assert(offsetof(Chain, dec_state) > offsetof(Chain, prof) && offsetof(Chain, dec_state) > offsetof(Chain, state), "the decision block lies behind the coder state and the counters");
/* the label fields alone: binding labels touches neither the decision block in front of them nor the search state inside it */
constexpr ChainRange CR_LABELS = { offsetof(Chain, labels), sizeof(void *) + 8 * sizeof(int) };      /* labels, lbl_off, lbl_w */
static_assert(offsetof(Chain, lbl_off) == offsetof(Chain, labels) + sizeof(void *) && offsetof(Chain, lbl_w) == offsetof(Chain, lbl_off) + 4 * sizeof(int)
              && offsetof(Chain, labels) >= offsetof(Chain, tile_h) + sizeof(int), "labels / lbl_off / lbl_w are adjacent, behind the tile rectangle");
constexpr ChainRange CR_COL = { offsetof(Chain, col), sizeof(void *) };
static_assert(sizeof(((Chain *)0)->col) == sizeof(void *), "col is one pointer");
constexpr ChainRange CR_PU_TRACE = { offsetof(Chain, pu_trace), sizeof(void *) };
static_assert(sizeof(((Chain *)0)->pu_trace) == sizeof(void *), "pu_trace is one pointer");
/* the CU trace: the last pointer of the GPU layout, behind every range above -- binding it copies that pointer alone */
constexpr ChainRange CR_CU_TRACE = { offsetof(Chain, cu_trace), sizeof(void *) };
static_assert(sizeof(((Chain *)0)->cu_trace) == sizeof(void *) && offsetof(Chain, cu_trace) == CR_LABELS.off + CR_LABELS.len
              && offsetof(Chain, cu_trace) >= offsetof(Chain, int_mv_r) + sizeof(((Chain *)0)->int_mv_r) && CR_DECISION.off + CR_DECISION.len >= CR_CU_TRACE.off + CR_CU_TRACE.len,
              "cu_trace is one pointer directly behind the label fields; the decision copy, which runs to the end, carries the host's copy of it");
constexpr ChainRange CR_INT_MV = { offsetof(Chain, int_mv_r), 2 * FCU_MAX_REF * sizeof(int32_t) };
static_assert(sizeof(((Chain *)0)->int_mv_r) == 2 * FCU_MAX_REF * sizeof(int32_t), "search state layout");

/* the rows of a P picture decide one picture: every row must name row 0's reference pictures and collocated field */
inline bool wpp_same_refs(const Chain &a, const Chain &b)
{
  if (a.n_ref != b.n_ref || a.poc != b.poc || a.col != b.col || a.col_poc != b.col_poc || a.ref_stride[0] != b.ref_stride[0]) return false;
  for (int k = 0; k < 3; k++) if (a.ref[k] != b.ref[k]) return false;
  for (int r = 0; r < FCU_MAX_REF; r++) {
    if (a.col_ref_poc[r] != b.col_ref_poc[r]) return false;
    if (r >= a.n_ref) continue;
    if (a.ref_poc[r] != b.ref_poc[r]) return false;
    for (int k = 0; k < 3; k++) if (a.refs[r][k] != b.refs[r][k]) return false;
  }
  return true;
}

/* ---- The host state machine.  planes of a picture as the binders take them */
struct Planes { const uint8_t *oy, *ou, *ov; uint8_t *ry, *ru, *rv; fcu_ctu_out *out; };

/* how a binder cuts a picture into chains, and the entry point it speaks for in the messages: the rows of a one-slice picture
 * (fcu_wpp_begin: I slices only, fcu_wpp_begin_p: P slices only), rows of slices of slice_rows whole CTU rows
 * (fcu_wpp_begin_slices), one chain per tile (fcu_tiles_begin), rows inside tiles (fcu_wpp_begin_tiles) */
struct PictureCut {
  const char *name; int only_type; bool sliced; int slice_rows; bool tiled; int n_cols, n_rows, wpp;
  static PictureCut rows(int slice_type) { return { slice_type == FCU_SLICE_P ? "fcu_wpp_begin_p" : "fcu_wpp_begin", slice_type, false, 0, false, 0, 0, 1 }; }
  static PictureCut row_slices(int slice_rows) { return { "fcu_wpp_begin_slices", -1, true, slice_rows, false, 0, 0, 1 }; }
  static PictureCut tiles(int n_cols, int n_rows, int wpp) { return { wpp ? "fcu_wpp_begin_tiles" : "fcu_tiles_begin", -1, false, 0, true, n_cols, n_rows, wpp }; }
};

/* The sequence parameters, the host copy of every chain's descriptor and every chain's position (where the launches so far
 * have left it).  A method that can refuse returns the FCU_* code and leaves the text, which names the entry point, in `err`. */
struct HostState {
  fcu_seq_params sp = {};
  int w_ctu = 0, h_ctu = 0, n_ctu = 0;           /* the picture in CTUs: computed here and nowhere else */
  std::vector<Chain> chains;
  std::vector<int> pos;
  struct Picture { int first, n; };               /* per chain: the chains [first, first + n) picture_bind last filled together with it */
  std::vector<Picture> pic;
  std::string err;

  int refuse(int code, const std::string &msg) { err = msg; return code; }
  static bool seq_ok(const fcu_seq_params *s) { return s && s->width > 0 && s->height > 0 && !(s->width & 7) && !(s->height & 7) && s->max_chains > 0; }
  void init(const fcu_seq_params &s)
  {
    sp = s; w_ctu = (s.width + 63) / 64; h_ctu = (s.height + 63) / 64; n_ctu = w_ctu * h_ctu;
    chains.resize((size_t)s.max_chains);
    memset(chains.data(), 0, sizeof(Chain) * chains.size());
    pos.assign((size_t)s.max_chains, 0);
    pic.assign((size_t)s.max_chains, Picture{ 0, 0 });
  }
  bool has(int chain) const { return chain >= 0 && chain < sp.max_chains; }
  int position(int chain) const { return has(chain) ? pos[(size_t)chain] : -1; }
  /* what every setter of a bound chain's state asks first */
  int bound(const char *name, int chain)
  {
    if (!has(chain)) return refuse(FCU_ERR_ARG, std::string(name) + ": bad argument");
    if (chains[(size_t)chain].out == nullptr) return refuse(FCU_ERR_STATE, std::string(name) + ": chain not bound (fcu_chain_begin)");
    return FCU_OK;
  }

  /* fcu_chain_begin: the argument checks, then the descriptor of a chain that decides the whole picture from CTU 0 */
  int chain_begin_check(int chain, const fcu_frame_params *fp, const Planes &pl)
  {
    if (!fp || !has(chain) || !pl.oy || !pl.ou || !pl.ov || !pl.ry || !pl.ru || !pl.rv || !pl.out) return refuse(FCU_ERR_ARG, "fcu_chain_begin: bad argument");
    if (fp->qp < 0 || fp->qp > 51 || fp->slice_ctus < 0) return refuse(FCU_ERR_ARG, "fcu_chain_begin: QP / slice_ctus out of range");
    if (fp->slice_type != FCU_SLICE_I && fp->slice_type != FCU_SLICE_P) return refuse(FCU_ERR_ARG, "fcu_chain_begin: unknown slice type");
    if (fp->slice_type == FCU_SLICE_P && (!(fp->lambda > 0.0) || fp->search_range < 1 || fp->search_range > 64)) return refuse(FCU_ERR_ARG, "fcu_chain_begin: a P slice needs its lambda (fcu_ldp_slice) and 1 <= search_range <= 64");
    return FCU_OK;
  }
  int chain_begin(int chain, const fcu_frame_params *fp, const Planes &pl)
  {
    if (const int rc = chain_begin_check(chain, fp, pl)) return rc;
    chain_bind(chains[(size_t)chain], sp.width, sp.height, *fp, pl.oy, pl.ou, pl.ov, pl.ry, pl.ru, pl.rv, pl.out);
    pos[(size_t)chain] = 0;
    return FCU_OK;
  }

  /* ---- the picture binder.  picture_check: everything the five picture entry points refuse, in their order (libfcu.so allocates
   * the WaveFrontSynchro blocks between the two steps); picture_bind: the descriptors and positions of the picture's chains
   * [first, first + n), returns n.  A row that starts a slice, and row 0 of a tile, is bound as row 0 of a picture is: no row
   * above (wpp_above -1), no sync slot to read -- run_wpp_chain waits for and inherits nothing, compress_ctu resets the coder. */
  int picture_chains(const PictureCut &cut) const { return cut.tiled ? tile_chains(w_ctu, h_ctu, cut.n_cols, cut.n_rows, cut.wpp) : h_ctu; }
  int picture_check(const PictureCut &cut, int first, const fcu_frame_params *fp, const Planes &pl)
  {
    const std::string name(cut.name);
    if (!fp) return refuse(FCU_ERR_ARG, name + ": bad argument");
    if (cut.only_type == FCU_SLICE_I && fp->slice_type != FCU_SLICE_I) return refuse(FCU_ERR_ARG, name + ": binds I slices only (P slices: fcu_wpp_begin_p)");
    if (cut.only_type == FCU_SLICE_P && fp->slice_type != FCU_SLICE_P) return refuse(FCU_ERR_ARG, name + ": binds P slices only (I slices: fcu_wpp_begin)");
    fcu_frame_params f = *fp;
    if (cut.tiled) {
      if (!tile_grid(w_ctu, h_ctu, cut.n_cols, cut.n_rows, nullptr, nullptr)) return refuse(FCU_ERR_ARG, name + ": a grid needs 1 <= n_cols <= width and 1 <= n_rows <= height in CTUs (no empty tile)");
      if (fp->slice_ctus != 0) return refuse(FCU_ERR_ARG, name + ": tiles need one slice per picture (slice_ctus 0)");
      if (!tile_params_ok(*fp, cut.n_cols)) return refuse(FCU_ERR_ARG, name + ": TMVP across tile columns is not supported (tmvp 1 needs n_cols 1)");
      if (first < 0 || first + picture_chains(cut) > sp.max_chains) return refuse(FCU_ERR_ARG, name + ": too few chains (fcu_tile_chains)");
    } else {
      if (cut.sliced && cut.slice_rows < 1) return refuse(FCU_ERR_ARG, name + ": slice_rows must be at least 1");
      if (!cut.sliced && fp->slice_ctus != 0) return refuse(FCU_ERR_ARG, name + ": WaveFrontSynchro needs one slice per picture (slice_ctus 0); slices of whole CTU rows are bound by fcu_wpp_begin_slices");
      if (cut.sliced && (f.slice_ctus = wpp_slice_ctus(w_ctu, cut.slice_rows, fp->slice_ctus)) < 0) return refuse(FCU_ERR_ARG, name + ": slice_rows must be >= 1 and slice_ctus 0 or slice_rows x the picture width in CTUs (a slice starts at a row start)");
      if (first < 0 || first + h_ctu > sp.max_chains) return refuse(FCU_ERR_ARG, name + ": too few chains for one chain per CTU row (fcu_wpp_rows)");
    }
    return chain_begin_check(first, &f, pl);
  }
  /* (arguments picture_check has accepted; sync = slot 0 of the sync slot array, used with cut.wpp only) */
  int picture_bind(const PictureCut &cut, int first, const fcu_frame_params &fp, const Planes &pl, uint8_t *sync)
  {
    fcu_frame_params f = fp;
    if (cut.sliced) f.slice_ctus = wpp_slice_ctus(w_ctu, cut.slice_rows, fp.slice_ctus);
    Chain base;
    chain_bind(base, sp.width, sp.height, f, pl.oy, pl.ou, pl.ov, pl.ry, pl.ru, pl.rv, pl.out);
    const int n_cols = cut.tiled ? cut.n_cols : 1, n_rows = cut.tiled ? cut.n_rows : 1;      /* no tiles: one tile, the picture */
    std::vector<int> cb((size_t)n_cols + 1), rb((size_t)n_rows + 1);
    tile_grid(w_ctu, h_ctu, n_cols, n_rows, cb.data(), rb.data());
    int i = first;
    for (int ty = 0; ty < n_rows; ty++) for (int tx = 0; tx < n_cols; tx++) {      /* tile-scan order */
      const int x0 = cb[(size_t)tx], y0 = rb[(size_t)ty], tw = cb[(size_t)tx + 1] - x0, th = rb[(size_t)ty + 1] - y0;
      for (int r = 0; r < (cut.wpp ? th : 1); r++, i++) {
        Chain &h = chains[(size_t)i];
        h = base;
        if (cut.tiled) tile_bind(h, x0, y0, tw, th);
        if (cut.wpp && cut.tiled) wpp_bind_tile_row(h, r, i, sync);
        else if (cut.wpp) wpp_bind_row(h, r, w_ctu, cut.sliced ? cut.slice_rows : 0, first, sync);
        pos[(size_t)i] = h.next_ctu;
      }
    }
    for (int k = first; k < i; k++) pic[(size_t)k] = Picture{ first, i - first };
    return i - first;
  }

  /* ---- the fork's decision block and the caller's labels.  NL: elements of one picture's label array */
  int label_count() const { return maps_geom(sp.width, sp.height, 0, nullptr).lvl_off[4]; }
  /* fcu_chain_set_decision: Verifying / Testing predict from the OBF map or from labels bound before; the binding stays */
  int set_decision(int chain, const fcu_decision_params *dp)
  {
    if (!dp || !has(chain)) return refuse(FCU_ERR_ARG, "fcu_chain_set_decision: bad argument");
    if (dp->state < FCU_TRAINING || dp->state > FCU_TESTING) return refuse(FCU_ERR_ARG, "fcu_chain_set_decision: unknown state");
    Chain &h = chains[(size_t)chain];
    if (dp->state != FCU_TRAINING && !dp->dev_obf && !h.labels) return refuse(FCU_ERR_ARG, "fcu_chain_set_decision: Verifying / Testing need the frame's OBF map (fcu_obf_prepass) or labels bound before (fcu_chain_set_labels)");
    if (const int rc = bound("fcu_chain_set_decision", chain)) return rc;
    chain_set_decision(h, dp->state, dp->depth_exception, dp->dev_obf, dp->sw_skip2nx2n, dp->sw_terminate);
    return FCU_OK;
  }
  /* fcu_chain_set_labels: null unbinds -- but not from a chain that would then predict from nothing */
  int set_labels(int chain, const int8_t *labels)
  {
    if (const int rc = bound("fcu_chain_set_labels", chain)) return rc;
    Chain &h = chains[(size_t)chain];
    if (!labels && h.dec_state != DEC_TRAINING && !h.obf) return refuse(FCU_ERR_STATE, "fcu_chain_set_labels: a chain in the Verifying / Testing state without an OBF map cannot lose its labels (set the state to Training first)");
    chain_set_labels(h, labels);
    return FCU_OK;
  }

  /* fcu_chain_set_pu_trace / fcu_chain_set_cu_trace: a bound chain; null stops recording.  The CU trace is cleared and written in
   * 4- and 8-byte units */
  int set_pu_trace(int chain, fcu_pu_trace *trace)
  {
    if (const int rc = bound("fcu_chain_set_pu_trace", chain)) return rc;
    chains[(size_t)chain].pu_trace = trace;
    return FCU_OK;
  }
  int set_cu_trace(int chain, fcu_cu_trace *trace)
  {
    if (const int rc = bound("fcu_chain_set_cu_trace", chain)) return rc;
    if ((uintptr_t)trace & 7) return refuse(FCU_ERR_ARG, "fcu_chain_set_cu_trace: dev_trace must start at a multiple of 8 bytes");
    chains[(size_t)chain].cu_trace = trace;
    return FCU_OK;
  }

  /* fcu_chain_set_range: the state checks before the range checks */
  int set_range(int chain, int first_ctu, int n_ctus)
  {
    if (!has(chain)) return refuse(FCU_ERR_ARG, "fcu_chain_set_range: bad argument");
    Chain &h = chains[(size_t)chain];
    if (h.out == nullptr) return refuse(FCU_ERR_STATE, "fcu_chain_set_range: chain not bound (fcu_chain_begin)");
    if (h.wpp) return refuse(FCU_ERR_STATE, "fcu_chain_set_range: a WaveFrontSynchro row chain keeps the row fcu_wpp_begin gave it");
    if (!tile_is_picture(h)) return refuse(FCU_ERR_STATE, "fcu_chain_set_range: a tile chain keeps the tile fcu_tiles_begin gave it");
    const int sl = h.p.slice_ctus;
    if (first_ctu < 0 || n_ctus <= 0 || first_ctu + n_ctus > h.n_ctu) return refuse(FCU_ERR_ARG, "fcu_chain_set_range: range outside the frame");
    /* a chain may only start where the reference resets its entropy coder and cuts the neighbourhood: at a slice start */
    if (first_ctu != 0 && (sl <= 0 || first_ctu % sl != 0)) return refuse(FCU_ERR_ARG, "fcu_chain_set_range: a chain must start at a slice boundary");
    if (first_ctu + n_ctus != h.n_ctu && (sl <= 0 || (first_ctu + n_ctus) % sl != 0)) return refuse(FCU_ERR_ARG, "fcu_chain_set_range: a chain must end at a slice boundary");
    h.next_ctu = first_ctu; h.end_ctu = first_ctu + n_ctus;
    pos[(size_t)chain] = first_ctu;
    return FCU_OK;
  }

  /* fcu_compress_ctu's own rule (a tile chain's position counts CTUs inside its tile; the CTU is named by its picture address) */
  int ctu_check(int chain, uint32_t ctuRsAddr)
  {
    if (!has(chain)) return refuse(FCU_ERR_ARG, "fcu_compress_ctu: bad argument");
    const Chain &h = chains[(size_t)chain];
    if (pos[(size_t)chain] >= h.end_ctu || h.out == nullptr || (int)ctuRsAddr != tile_ctu_addr(h, pos[(size_t)chain])) return refuse(FCU_ERR_STATE, "fcu_compress_ctu: CTUs of a chain must be decided in raster order");
    return FCU_OK;
  }

  /* fcu_compress_chains: the guard of the launch, and the positions after it */
  int chains_check(int first, int n, int ctus)
  {
    if (first < 0 || n <= 0 || first + n > sp.max_chains || ctus <= 0) return refuse(FCU_ERR_ARG, "fcu_compress_chains: bad range");
    for (int i = first; i < first + n; i++) {
      const Chain &h = chains[(size_t)i];
      if (h.out == nullptr) return refuse(FCU_ERR_STATE, "fcu_compress_chains: chain not bound (fcu_chain_begin)");
      if (h.wpp) return refuse(FCU_ERR_STATE, "fcu_compress_chains: a WaveFrontSynchro row chain is decided by fcu_compress_wpp");
      if (h.p.slice_type == SLICE_P && h.ref[0] == nullptr) return refuse(FCU_ERR_STATE, "fcu_compress_chains: P chain without reference picture (fcu_chain_set_reference)");
    }
    return FCU_OK;
  }
  void chains_launched(int first, int n, int ctus) { for (int i = first; i < first + n; i++) { int &p = pos[(size_t)i]; p += ctus; if (p > chains[(size_t)i].end_ctu) p = chains[(size_t)i].end_ctu; } }

  /* fcu_compress_wpp: the guard of the WaveFrontSynchro launch.  A row waits for the chain its descriptor names, and for ever if
   * that chain is not in the launch: the range must hold whole pictures, each as picture_bind made it (`pic`) and not yet decided.
   * A chain bound again since -- by fcu_chain_begin (no row chain any more) or as part of another picture (another record) --
   * breaks its old picture until that is bound again as a whole. */
  int wpp_check(int first, int n)
  {
    if (first < 0 || n <= 0 || first + n > sp.max_chains) return refuse(FCU_ERR_ARG, "fcu_compress_wpp: bad range");
    for (int i = first, start = first, end = first; i < first + n; i++) {
      const Chain &h = chains[(size_t)i];
      const Picture &p = pic[(size_t)i];
      if (h.out == nullptr || !h.wpp) return refuse(FCU_ERR_STATE, "fcu_compress_wpp: chain not bound by fcu_wpp_begin(_p) / fcu_wpp_begin_slices / fcu_wpp_begin_tiles");
      if (i == end) { start = i; end = i + p.n; }             /* a picture must start here: chain i is its first, the rest carry its record */
      if (p.first != start || p.n != end - start) return refuse(FCU_ERR_STATE, "fcu_compress_wpp: the range must hold whole pictures bound by fcu_wpp_begin(_p) / fcu_wpp_begin_slices / fcu_wpp_begin_tiles, their rows at consecutive chains (tiles: in tile-scan order, the rows of a tile top to bottom)");
      if (end > first + n) return refuse(FCU_ERR_STATE, "fcu_compress_wpp: the range must end with the last row of a picture (tiles: of its last tile)");
      if (pos[(size_t)i] != h.next_ctu) return refuse(FCU_ERR_STATE, "fcu_compress_wpp: picture already decided (bind it again with fcu_wpp_begin(_p) / fcu_wpp_begin_slices / fcu_wpp_begin_tiles)");
      if (h.p.slice_type == SLICE_P) {
        if (h.ref[0] == nullptr) return refuse(FCU_ERR_STATE, "fcu_compress_wpp: P row without reference picture (fcu_chain_set_reference(s) on every row)");
        if (!wpp_same_refs(h, chains[(size_t)p.first])) return refuse(FCU_ERR_STATE, "fcu_compress_wpp: the rows of a P picture name different reference pictures or collocated fields");
      }
    }
    return FCU_OK;
  }
  void wpp_launched(int first, int n) { for (int i = first; i < first + n; i++) pos[(size_t)i] = chains[(size_t)i].end_ctu; }
};

} // namespace fcu
