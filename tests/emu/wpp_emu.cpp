/*
 * wpp_emu.cpp -- TEST-ONLY build of the engine source (-DFCU_EMU) for WaveFrontSynchro: the row chains of one I or P picture,
 * one slice or slices of whole CTU rows, bound as fcu_wpp_begin / fcu_wpp_begin_p / fcu_wpp_begin_slices (+ the per-row
 * reference setters) bind them and run through run_wpp_chain one after the other in chain order, the row above first
 * (picture_emu.h).  Every wait of a row is then a check that the row above has progressed far enough (a row bound without a row
 * above never waits), and the emulator-only bookkeeping of the search state (Chain::wpp_mv_known) counts every TZ search that
 * reads a start vector the row neither wrote nor inherited.
 * Built by __graft_entry__.build().  It is NOT part of libfcu.so and nothing in the product path can reach it.
 */
#include "picture_emu.h"

extern "C" {
/* the rule fcu_wpp_begin_slices refuses its slice arguments by (-1) */
int wpp_emu_slice_rule(int W, int slice_rows, int fp_slice_ctus) { return wpp_slice_ctus(W, slice_rows, fp_slice_ctus); }

/* One picture.  slice_rows 0 = one slice, as fcu_wpp_begin(_p) binds it (fp_slice_ctus, what the frame parameters name, must be
 * 0); slice_rows R != 0 = the arguments of fcu_wpp_begin_slices (fp_slice_ctus 0 or R x width in CTUs).  Returns null where the
 * entry point returns FCU_ERR_ARG for them.  tools, and the arguments from n_ref to col: picture_emu.h.
 * int_mv = the search state row 0 of a one-slice picture starts from (FCU_MAX_REF x, y pairs; fcu_chain_set_search_state on row
 * 0), or null: zero, which every slice of a sliced picture starts from.  start_known 0 makes the read-before-write bookkeeping
 * treat the start state of every row without a row above as unknown (to show the count can fire). */
void *wpp_emu_create(int width, int height, int qp, int slice_rows, int fp_slice_ctus, int tools,
                     const uint8_t *oy, const uint8_t *ou, const uint8_t *ov, uint8_t *ry, uint8_t *ru, uint8_t *rv, fcu_ctu_out *out,
                     int n_ref, double lambda, int search_range, int fast_search, int amp, int cabac_b_table,
                     const uint8_t *const *pad_planes, const int *ref_pocs, int poc, const int *col_ref_pocs, int n_col, const fcu_ctu_out *col,
                     const int32_t *int_mv, int start_known)
{
  const fcu_frame_params fp = emu_frame_params(qp, fp_slice_ctus, tools, n_ref, lambda, search_range, fast_search, amp, cabac_b_table, col != nullptr);
  const PictureCut cut = slice_rows == 0 ? PictureCut::rows(fp.slice_type) : PictureCut::row_slices(slice_rows);
  EmuPicture *e = emu_picture(width, height, cut, fp, Planes{ oy, ou, ov, ry, ru, rv, out }, EmuList0{ n_ref, pad_planes, ref_pocs, poc, col_ref_pocs, n_col, col },
                              start_known ? (1 << FCU_MAX_REF) - 1 : 0);     /* a start state is the value the row is meant to read */
  if (e && n_ref > 0 && slice_rows == 0 && int_mv) memcpy(e->c[0].int_mv_r, int_mv, sizeof(e->c[0].int_mv_r));
  return e;
}
void wpp_emu_destroy(void *p) { delete (EmuPicture *)p; }
int wpp_emu_rows(void *p) { return (int)((EmuPicture *)p)->c.size(); }
/* what the binder gave a row: the row it waits on (-1: none), and the slice length of the descriptor */
int wpp_emu_above(void *p, int row) { return ((EmuPicture *)p)->c[(size_t)row].wpp_above; }
int wpp_emu_slice_ctus(void *p) { return ((EmuPicture *)p)->c[0].p.slice_ctus; }
void wpp_emu_set_decision(void *p, int state, const uint8_t *sw_skip, const uint8_t *sw_term, int depth_exception, const int16_t *obf) { emu_set_decision((EmuPicture *)p, state, sw_skip, sw_term, depth_exception, obf); }
int wpp_emu_run(void *p) { return emu_run((EmuPicture *)p); }
void wpp_emu_get_state_full(void *p, int row, uint8_t *ctx, uint64_t *frac) { emu_get_state_full((EmuPicture *)p, row, ctx, frac); }
void wpp_emu_get_verify(void *p, double *out24) { emu_get_verify((EmuPicture *)p, out24); }
void wpp_emu_get_search_state(void *p, int row, int32_t *xy) { emu_get_search_state((EmuPicture *)p, row, xy); }
int wpp_emu_read_before_write(void *p) { return emu_read_before_write((EmuPicture *)p); }
}
