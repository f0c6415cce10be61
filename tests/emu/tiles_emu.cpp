/*
 * tiles_emu.cpp -- TEST-ONLY build of the engine source (-DFCU_EMU) for tiles: the chains of one I or P picture cut into uniform
 * tiles, bound as fcu_tiles_begin (one chain per tile, run raster-in-tile as fcu_compress_chains runs them) or
 * fcu_wpp_begin_tiles (one chain per CTU row of every tile, run through run_wpp_chain) bind them, and run one after the other in
 * chain order (tile-scan order, the row above first; picture_emu.h).  Every wait of a row is then a check that the row above in
 * its tile has progressed far enough.
 * Built by __graft_entry__.build().  It is NOT part of libfcu.so and nothing in the product path can reach it.
 */
#include "picture_emu.h"

extern "C" {
/* fcu_tile_grid: 1 = a grid (col_bd / row_bd filled), 0 = refused */
int tiles_emu_grid(int W, int H, int n_cols, int n_rows, int *col_bd, int *row_bd) { return tile_grid(W, H, n_cols, n_rows, col_bd, row_bd) ? 1 : 0; }
/* fcu_tile_chains of a picture of W x H CTUs */
int tiles_emu_chains(int W, int H, int n_cols, int n_rows, int wpp) { return tile_chains(W, H, n_cols, n_rows, wpp); }

/* One picture as n_cols x n_rows uniform tiles; wpp 0 = fcu_tiles_begin, 1 = fcu_wpp_begin_tiles.  Returns null where the entry
 * points return FCU_ERR_ARG: fp_slice_ctus != 0, a grid with an empty tile, tmvp with n_cols > 1.
 * tools, and the arguments from n_ref to col: picture_emu.h; tmvp = frame_params.tmvp (col may be null: every temporal candidate
 * unavailable).  Every tile starts from a zero search state. */
void *tiles_emu_create(int width, int height, int qp, int n_cols, int n_rows, int wpp, int fp_slice_ctus, int tools,
                       const uint8_t *oy, const uint8_t *ou, const uint8_t *ov, uint8_t *ry, uint8_t *ru, uint8_t *rv, fcu_ctu_out *out,
                       int n_ref, double lambda, int search_range, int fast_search, int amp, int cabac_b_table,
                       const uint8_t *const *pad_planes, const int *ref_pocs, int poc, const int *col_ref_pocs, int n_col, const fcu_ctu_out *col, int tmvp)
{
  const fcu_frame_params fp = emu_frame_params(qp, fp_slice_ctus, tools, n_ref, lambda, search_range, fast_search, amp, cabac_b_table, tmvp);
  return emu_picture(width, height, PictureCut::tiles(n_cols, n_rows, wpp), fp, Planes{ oy, ou, ov, ry, ru, rv, out },
                     EmuList0{ n_ref, pad_planes, ref_pocs, poc, col_ref_pocs, n_col, col }, (1 << FCU_MAX_REF) - 1);      /* the zero start state is the value the tile is meant to read */
}
void tiles_emu_destroy(void *p) { delete (EmuPicture *)p; }
int tiles_emu_n(void *p) { return (int)((EmuPicture *)p)->c.size(); }
/* what the binder gave chain i: out6 = tile_x0, tile_y0, tile_w, tile_h, next_ctu, end_ctu; returns wpp_above */
int tiles_emu_chain(void *p, int i, int *out6)
{
  const Chain &c = ((EmuPicture *)p)->c[(size_t)i];
  out6[0] = c.tile_x0; out6[1] = c.tile_y0; out6[2] = c.tile_w; out6[3] = c.tile_h; out6[4] = c.next_ctu; out6[5] = c.end_ctu;
  return c.wpp_above;
}
void tiles_emu_set_decision(void *p, int state, const uint8_t *sw_skip, const uint8_t *sw_term, int depth_exception, const int16_t *obf) { emu_set_decision((EmuPicture *)p, state, sw_skip, sw_term, depth_exception, obf); }
int tiles_emu_run(void *p) { return emu_run((EmuPicture *)p); }
void tiles_emu_get_state_full(void *p, int i, uint8_t *ctx, uint64_t *frac) { emu_get_state_full((EmuPicture *)p, i, ctx, frac); }
void tiles_emu_get_verify(void *p, double *out24) { emu_get_verify((EmuPicture *)p, out24); }
void tiles_emu_get_search_state(void *p, int i, int32_t *xy) { emu_get_search_state((EmuPicture *)p, i, xy); }
int tiles_emu_read_before_write(void *p) { return emu_read_before_write((EmuPicture *)p); }
}
