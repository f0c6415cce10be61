/*
 * wpp_emu.cpp -- TEST-ONLY build of the engine source (-DFCU_EMU) for WaveFrontSynchro: the row chains of one picture,
 * bound as fcu_wpp_begin binds them, run through run_wpp_chain one after the other in chain order (the row above first),
 * so every wait of a row is a check that the row above has progressed far enough.  Compiled by tests/test_wpp_emu.py.
 * It is NOT part of libfcu.so and nothing in the product path can reach it.
 */
#define FCU_EMU 1
#include "../../fast-cu-decision-hevc_amd/csrc/fcu_host.h"
#include <stdlib.h>
#include <vector>

using namespace fcu;

struct EmuWpp {
  int rows;
  std::vector<Chain> c;
  std::vector<Scratch *> g;
  std::vector<uint8_t> sync;
  std::vector<unsigned> ctl;
};

extern "C" {
/* tools: bit 0 transform_skip, 1 transform_skip_fast, 2 sign_hiding, 3 strong_intra_smoothing; -1 = defaults */
void *wpp_emu_create(int width, int height, int qp, int tools, const uint8_t *oy, const uint8_t *ou, const uint8_t *ov,
                     uint8_t *ry, uint8_t *ru, uint8_t *rv, fcu_ctu_out *out)
{
  EmuWpp *e = new EmuWpp();
  const int W = (width + 63) / 64, H = (height + 63) / 64;
  e->rows = H;
  e->c.resize((size_t)H);
  e->sync.assign((size_t)H * WPP_SYNC_BYTES, 0);
  e->ctl.assign((size_t)(WPP_CTL_WORDS + H), 0u);
  fcu_frame_params fp; default_frame_params(fp, qp);
  if (tools >= 0) { fp.transform_skip = tools & 1; fp.transform_skip_fast = (tools >> 1) & 1; fp.sign_hiding = (tools >> 2) & 1; fp.strong_intra_smoothing = (tools >> 3) & 1; }
  for (int r = 0; r < H; r++) {
    Chain &h = e->c[(size_t)r];
    memset(&h, 0, sizeof(h));
    fill_params(h.p, width, height, fp);
    h.org[0] = oy; h.org[1] = ou; h.org[2] = ov; h.rec[0] = ry; h.rec[1] = ru; h.rec[2] = rv;
    h.stride[0] = width; h.stride[1] = h.stride[2] = width / 2;
    h.out = out;
    h.w_ctu = W; h.h_ctu = H; h.n_ctu = W * H;
    h.next_ctu = r * W; h.end_ctu = (r + 1) * W;
    h.wpp = 1; h.wpp_above = r - 1;
    h.wpp_sync_in = r ? &e->sync[(size_t)(r - 1) * WPP_SYNC_BYTES] : nullptr;
    h.wpp_sync_out = &e->sync[(size_t)r * WPP_SYNC_BYTES];
    e->g.push_back((Scratch *)calloc(1, sizeof(Scratch)));
  }
  return e;
}
void wpp_emu_destroy(void *p) { EmuWpp *e = (EmuWpp *)p; for (Scratch *g : e->g) free(g); delete e; }
int wpp_emu_rows(void *p) { return ((EmuWpp *)p)->rows; }
void wpp_emu_set_decision(void *p, int state, const uint8_t *sw_skip, const uint8_t *sw_term, int depth_exception, const int16_t *obf)
{
  for (Chain &c : ((EmuWpp *)p)->c) {
    c.dec_state = state; c.depth_exception = depth_exception; c.obf = obf; c.obf_stride = c.p.width / 4;
    for (int d = 0; d < 4; d++) { c.sw_skip[d] = sw_skip[d]; c.sw_term[d] = sw_term[d]; }
    memset(c.ver, 0, sizeof(c.ver));
  }
}
/* every row in chain order; returns the rows that ran to their end */
int wpp_emu_run(void *p)
{
  EmuWpp *e = (EmuWpp *)p;
  int done = 0;
  for (int r = 0; r < e->rows; r++) done += run_wpp_chain(&e->c[(size_t)r], e->g[(size_t)r], e->ctl.data(), r);
  return done;
}
void wpp_emu_get_state_full(void *p, int row, uint8_t *ctx, uint64_t *frac)
{
  const Chain &c = ((EmuWpp *)p)->c[(size_t)row];
  memcpy(ctx, c.state.ctx, NCTX); *frac = c.state.frac;
}
/* verification counters of the rows added up in chain order (fcu_get_verify_counts) */
void wpp_emu_get_verify(void *p, double *out24)
{
  memset(out24, 0, sizeof(double) * 24);
  for (const Chain &c : ((EmuWpp *)p)->c) for (int d = 0; d < 4; d++) for (int k = 0; k < 6; k++) out24[d * 6 + k] += c.ver[d][k];
}
}
