/*
 * wpp_p_emu.cpp -- TEST-ONLY build of the engine source (-DFCU_EMU) for WaveFrontSynchro on P slices: the row chains of one P
 * picture, bound as fcu_wpp_begin_p + the per-row reference setters bind them, run through run_wpp_chain one after the other
 * in chain order (the row above first).  Every wait of a row is then a check that the row above has progressed far enough,
 * and the emulator-only bookkeeping of the search state (Chain::wpp_mv_known) counts every TZ search that reads a start
 * vector before the row wrote or inherited it.  Compiled by tests/test_wpp_p_emu.py.
 * It is NOT part of libfcu.so and nothing in the product path can reach it.
 */
#define FCU_EMU 1
#include "../../fast-cu-decision-hevc_amd/csrc/fcu_host.h"
#include <stdlib.h>
#include <vector>

using namespace fcu;

struct EmuWppP {
  int rows;
  std::vector<Chain> c;
  std::vector<Scratch *> g;
  std::vector<uint8_t> sync;
  std::vector<unsigned> ctl;
};

extern "C" {
/* One P picture.  pad_planes[3r .. 3r+2] = padded Y, U, V of RefPicList0[r] (luma margin FCU_REF_MARGIN), ref_pocs[r] their
 * POCs, poc the picture's, col_ref_pocs the POCs the collocated picture's list 0 named (n_col of them); col = that picture's
 * fcu_ctu_out array (TMVP) or null.  int_mv = the search state row 0 starts from (FCU_MAX_REF x, y pairs); row0_known = 0 makes
 * the read-before-write bookkeeping treat row 0's start state as unknown (to show the count can fire). */
void *wpp_p_emu_create(int width, int height, int qp, double lambda, int search_range, int fast_search, int amp, int cabac_b_table,
                       const uint8_t *oy, const uint8_t *ou, const uint8_t *ov, uint8_t *ry, uint8_t *ru, uint8_t *rv, fcu_ctu_out *out,
                       int n_ref, const uint8_t *const *pad_planes, const int *ref_pocs, int poc, const int *col_ref_pocs, int n_col,
                       const fcu_ctu_out *col, const int32_t *int_mv, int row0_known)
{
  EmuWppP *e = new EmuWppP();
  const int W = (width + 63) / 64, H = (height + 63) / 64;
  e->rows = H;
  e->c.resize((size_t)H);
  e->sync.assign((size_t)H * WPP_SYNC_BYTES, 0);
  e->ctl.assign((size_t)(WPP_CTL_WORDS + H), 0u);
  fcu_frame_params fp; default_frame_params(fp, qp);
  fp.slice_type = FCU_SLICE_P; fp.lambda = lambda; fp.search_range = search_range; fp.fast_search = fast_search;
  const int m = FCU_REF_MARGIN, sy = width + 2 * m, sc = width / 2 + m;
  for (int r = 0; r < H; r++) {
    Chain &h = e->c[(size_t)r];
    memset(&h, 0, sizeof(h));
    fill_params(h.p, width, height, fp);
    h.p.amp = amp != 0; h.p.tmvp = col != nullptr; h.p.cabac_b_table = cabac_b_table != 0;
    h.org[0] = oy; h.org[1] = ou; h.org[2] = ov; h.rec[0] = ry; h.rec[1] = ru; h.rec[2] = rv;
    h.stride[0] = width; h.stride[1] = h.stride[2] = width / 2;
    h.out = out; h.col = col;
    h.w_ctu = W; h.h_ctu = H; h.n_ctu = W * H;
    h.next_ctu = r * W; h.end_ctu = (r + 1) * W;
    h.wpp = 1; h.wpp_above = r - 1;
    h.wpp_sync_in = r ? &e->sync[(size_t)(r - 1) * WPP_SYNC_BYTES] : nullptr;
    h.wpp_sync_out = &e->sync[(size_t)r * WPP_SYNC_BYTES];
    h.ref_stride[0] = sy; h.ref_stride[1] = h.ref_stride[2] = sc;
    for (int k = 0; k < n_ref; k++) {
      h.refs[k][0] = pad_planes[3 * k] + (size_t)m * sy + m;
      h.refs[k][1] = pad_planes[3 * k + 1] + (size_t)(m / 2) * sc + m / 2; h.refs[k][2] = pad_planes[3 * k + 2] + (size_t)(m / 2) * sc + m / 2;
      h.ref_poc[k] = ref_pocs[k];
    }
    for (int k = 0; k < 3; k++) h.ref[k] = h.refs[0][k];
    h.n_ref = n_ref; h.poc = poc; h.col_poc = ref_pocs[0];
    for (int k = 0; k < FCU_MAX_REF; k++) h.col_ref_poc[k] = k < n_col ? col_ref_pocs[k] : ref_pocs[0] - 1;
    if (r == 0) {                                            /* fcu_chain_set_search_state on row 0 */
      for (int k = 0; k < FCU_MAX_REF; k++) { h.int_mv_r[k][0] = int_mv[2 * k]; h.int_mv_r[k][1] = int_mv[2 * k + 1]; }
      h.wpp_mv_known = row0_known ? (1 << FCU_MAX_REF) - 1 : 0;
    }
    e->g.push_back((Scratch *)calloc(1, sizeof(Scratch)));
  }
  return e;
}
void wpp_p_emu_destroy(void *p) { EmuWppP *e = (EmuWppP *)p; for (Scratch *g : e->g) free(g); delete e; }
int wpp_p_emu_rows(void *p) { return ((EmuWppP *)p)->rows; }
void wpp_p_emu_set_decision(void *p, int state, const uint8_t *sw_skip, const uint8_t *sw_term, int depth_exception, const int16_t *obf)
{
  for (Chain &c : ((EmuWppP *)p)->c) {
    c.dec_state = state; c.depth_exception = depth_exception; c.obf = obf; c.obf_stride = c.p.width / 4;
    for (int d = 0; d < 4; d++) { c.sw_skip[d] = sw_skip[d]; c.sw_term[d] = sw_term[d]; }
    memset(c.ver, 0, sizeof(c.ver));
  }
}
/* every row in chain order; returns the rows that ran to their end */
int wpp_p_emu_run(void *p)
{
  EmuWppP *e = (EmuWppP *)p;
  int done = 0;
  for (int r = 0; r < e->rows; r++) done += run_wpp_chain(&e->c[(size_t)r], e->g[(size_t)r], e->ctl.data(), r);
  return done;
}
void wpp_p_emu_get_state_full(void *p, int row, uint8_t *ctx, uint64_t *frac)
{
  const Chain &c = ((EmuWppP *)p)->c[(size_t)row];
  memcpy(ctx, c.state.ctx, NCTX); *frac = c.state.frac;
}
/* the search state a row chain ends with (fcu_chain_get_search_state) */
void wpp_p_emu_get_search_state(void *p, int row, int32_t *xy)
{
  const Chain &c = ((EmuWppP *)p)->c[(size_t)row];
  for (int k = 0; k < FCU_MAX_REF; k++) { xy[2 * k] = c.int_mv_r[k][0]; xy[2 * k + 1] = c.int_mv_r[k][1]; }
}
/* TZ searches, summed over the rows, that read a start vector the row had neither written nor inherited */
int wpp_p_emu_read_before_write(void *p)
{
  int n = 0;
  for (const Chain &c : ((EmuWppP *)p)->c) n += c.wpp_mv_rbw;
  return n;
}
}
