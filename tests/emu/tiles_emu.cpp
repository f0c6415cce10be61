/*
 * tiles_emu.cpp -- TEST-ONLY build of the engine source (-DFCU_EMU) for tiles: the chains of one I or P picture cut into uniform
 * tiles, bound as fcu_tiles_begin (one chain per tile, run raster-in-tile as fcu_compress_chains runs them) or
 * fcu_wpp_begin_tiles (one chain per CTU row of every tile, run through run_wpp_chain) bind them -- through the functions of
 * fcu_host.h the library's entry points use: tile_grid, tile_chains, tile_params_ok, chain_bind, tile_bind, wpp_bind_tile_row,
 * chain_set_list0, chain_set_collocated_pocs, chain_set_decision -- and run one after the other in chain order (tile-scan order,
 * the row above first).  Every wait of a row is then a check that the row above in its tile has progressed far enough.
 * Built by __graft_entry__.build().  It is NOT part of libfcu.so and nothing in the product path can reach it.
 */
#define FCU_EMU 1
#include "../../fast-cu-decision-hevc_amd/csrc/fcu_host.h"
#include <stdlib.h>
#include <vector>

using namespace fcu;

struct EmuTiles {
  std::vector<Chain> c;
  std::vector<Scratch *> g;
  std::vector<uint8_t> sync;
  std::vector<unsigned> ctl;
};

extern "C" {
/* fcu_tile_grid: 1 = a grid (col_bd / row_bd filled), 0 = refused */
int tiles_emu_grid(int W, int H, int n_cols, int n_rows, int *col_bd, int *row_bd) { return tile_grid(W, H, n_cols, n_rows, col_bd, row_bd) ? 1 : 0; }
/* fcu_tile_chains of a picture of W x H CTUs */
int tiles_emu_chains(int W, int H, int n_cols, int n_rows, int wpp) { return tile_chains(W, H, n_cols, n_rows, wpp); }

/* One picture as n_cols x n_rows uniform tiles; wpp 0 = fcu_tiles_begin, 1 = fcu_wpp_begin_tiles.  Returns null where the entry
 * points return FCU_ERR_ARG: fp_slice_ctus != 0, a grid with an empty tile, tmvp with n_cols > 1.
 * tools, and the arguments from n_ref on: as wpp_emu_create (tests/emu/wpp_emu.cpp); tmvp = frame_params.tmvp (col may be null:
 * every temporal candidate unavailable).  Every tile starts from a zero search state. */
void *tiles_emu_create(int width, int height, int qp, int n_cols, int n_rows, int wpp, int fp_slice_ctus, int tools,
                       const uint8_t *oy, const uint8_t *ou, const uint8_t *ov, uint8_t *ry, uint8_t *ru, uint8_t *rv, fcu_ctu_out *out,
                       int n_ref, double lambda, int search_range, int fast_search, int amp, int cabac_b_table,
                       const uint8_t *const *pad_planes, const int *ref_pocs, int poc, const int *col_ref_pocs, int n_col, const fcu_ctu_out *col, int tmvp)
{
  const int W = (width + 63) / 64, H = (height + 63) / 64;
  fcu_frame_params fp; default_frame_params(fp, qp);
  if (tools >= 0) { fp.transform_skip = tools & 1; fp.transform_skip_fast = (tools >> 1) & 1; fp.sign_hiding = (tools >> 2) & 1; fp.strong_intra_smoothing = (tools >> 3) & 1; }
  fp.slice_ctus = fp_slice_ctus;
  if (n_ref > 0) {
    fp.slice_type = FCU_SLICE_P; fp.lambda = lambda; fp.search_range = search_range; fp.fast_search = fast_search;
    fp.amp = amp; fp.cabac_b_table = cabac_b_table; fp.tmvp = tmvp;
  }
  std::vector<int> cb((size_t)(n_cols > 0 ? n_cols : 0) + 1), rb((size_t)(n_rows > 0 ? n_rows : 0) + 1);
  if (!tile_grid(W, H, n_cols, n_rows, cb.data(), rb.data()) || !tile_params_ok(fp, n_cols)) return nullptr;
  const int n = tile_chains(W, H, n_cols, n_rows, wpp);
  EmuTiles *e = new EmuTiles();
  e->c.resize((size_t)n);
  e->sync.assign((size_t)n * WPP_SYNC_BYTES, 0);
  e->ctl.assign((size_t)(WPP_CTL_WORDS + n), 0u);
  int i = 0;
  for (int ty = 0; ty < n_rows; ty++) for (int tx = 0; tx < n_cols; tx++) {
    const int x0 = cb[(size_t)tx], y0 = rb[(size_t)ty], tw = cb[(size_t)tx + 1] - x0, th = rb[(size_t)ty + 1] - y0;
    for (int r = 0; r < (wpp ? th : 1); r++, i++) {
      Chain &h = e->c[(size_t)i];
      chain_bind(h, width, height, fp, oy, ou, ov, ry, ru, rv, out);
      tile_bind(h, x0, y0, tw, th);
      if (wpp) wpp_bind_tile_row(h, r, i, e->sync.data());
      if (n_ref > 0) {
        chain_set_list0(h, n_ref, pad_planes, ref_pocs, poc);
        if (n_col > 0) chain_set_collocated_pocs(h, ref_pocs[0], col_ref_pocs, n_col);
        h.col = col;
      }
      if (h.wpp_above < 0) h.wpp_mv_known = (1 << FCU_MAX_REF) - 1;     /* the zero start state is the value the tile is meant to read */
      e->g.push_back((Scratch *)calloc(1, sizeof(Scratch)));
    }
  }
  return e;
}
void tiles_emu_destroy(void *p) { EmuTiles *e = (EmuTiles *)p; for (Scratch *g : e->g) free(g); delete e; }
int tiles_emu_n(void *p) { return (int)((EmuTiles *)p)->c.size(); }
/* what the binder gave chain i: out6 = tile_x0, tile_y0, tile_w, tile_h, next_ctu, end_ctu; returns wpp_above */
int tiles_emu_chain(void *p, int i, int *out6)
{
  const Chain &c = ((EmuTiles *)p)->c[(size_t)i];
  out6[0] = c.tile_x0; out6[1] = c.tile_y0; out6[2] = c.tile_w; out6[3] = c.tile_h; out6[4] = c.next_ctu; out6[5] = c.end_ctu;
  return c.wpp_above;
}
void tiles_emu_set_decision(void *p, int state, const uint8_t *sw_skip, const uint8_t *sw_term, int depth_exception, const int16_t *obf)
{
  for (Chain &c : ((EmuTiles *)p)->c) chain_set_decision(c, state, depth_exception, obf, sw_skip, sw_term);
}
/* every chain in chain order; returns the chains that ran to their end */
int tiles_emu_run(void *p)
{
  EmuTiles *e = (EmuTiles *)p;
  int done = 0;
  for (size_t i = 0; i < e->c.size(); i++) {
    Chain &c = e->c[i];
    if (c.wpp) { done += run_wpp_chain(&c, e->g[i], e->ctl.data(), (int)i); continue; }
    load_hot_tables();
    for (int k = c.next_ctu; k < c.end_ctu; k++) { compress_ctu(&c, e->g[i], k); c.next_ctu = k + 1; }    /* run_chain of fcu_kernels.hip */
    done++;
  }
  return done;
}
void tiles_emu_get_state_full(void *p, int i, uint8_t *ctx, uint64_t *frac)
{
  const Chain &c = ((EmuTiles *)p)->c[(size_t)i];
  memcpy(ctx, c.state.ctx, NCTX); *frac = c.state.frac;
}
void tiles_emu_get_verify(void *p, double *out24)
{
  memset(out24, 0, sizeof(double) * 24);
  for (const Chain &c : ((EmuTiles *)p)->c) for (int d = 0; d < 4; d++) for (int k = 0; k < 6; k++) out24[d * 6 + k] += c.ver[d][k];
}
void tiles_emu_get_search_state(void *p, int i, int32_t *xy) { memcpy(xy, ((EmuTiles *)p)->c[(size_t)i].int_mv_r, sizeof(((Chain *)0)->int_mv_r)); }
/* TZ searches, summed over the chains, that read a start vector the row had neither written nor inherited */
int tiles_emu_read_before_write(void *p)
{
  int n = 0;
  for (const Chain &c : ((EmuTiles *)p)->c) n += c.wpp_mv_rbw;
  return n;
}
}
