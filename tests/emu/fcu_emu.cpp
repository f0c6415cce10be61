/*
 * fcu_emu.cpp -- TEST-ONLY build of the engine source as a plain C++ wave emulator
 * (-DFCU_EMU: the 64 lanes of each phase run as a loop).  It exists so that the engine's
 * decision logic can be compared with the oracle in `-m "not gpu"` tests where no GPU is
 * present.  It is NOT part of libfcu.so and nothing in the product path can reach it.
 */
#define FCU_EMU 1
#include "../../fast-cu-decision-hevc_amd/csrc/fcu_host.h"
#include <stdlib.h>
#include <new>

using namespace fcu;

struct EmuChain { Chain c; Scratch *g; };

extern "C" {
/* tools: bit 0 transform_skip, 1 transform_skip_fast, 2 sign_hiding, 3 strong_intra_smoothing; -1 = defaults */
void *fcu_emu_create(int width, int height, int qp, int slice_ctus, int tools, const uint8_t *oy, const uint8_t *ou, const uint8_t *ov,
                     uint8_t *ry, uint8_t *ru, uint8_t *rv, fcu_ctu_out *out)
{
  EmuChain *e = new EmuChain();
  fcu_frame_params fp; default_frame_params(fp, qp); fp.slice_ctus = slice_ctus;
  if (tools >= 0) { fp.transform_skip = tools & 1; fp.transform_skip_fast = (tools >> 1) & 1; fp.sign_hiding = (tools >> 2) & 1; fp.strong_intra_smoothing = (tools >> 3) & 1; }
  chain_bind(e->c, width, height, fp, oy, ou, ov, ry, ru, rv, out);      /* the fill of fcu_chain_begin */
  load_hot_tables();
  e->g = (Scratch *)calloc(1, sizeof(Scratch));
  return e;
}
/* P picture: lambda of the slice (fcu_ldp_slice on the host), search range, and the padded reference planes
 * (luma margin FCU_REF_MARGIN, pointers to the first byte of each padded plane) */
void fcu_emu_set_p(void *h, int qp, double lambda, int search_range, int fast_search, const uint8_t *py, const uint8_t *pu, const uint8_t *pv)
{
  EmuChain *e = (EmuChain *)h;
  const int width = e->c.p.width, height = e->c.p.height;
  fcu_frame_params fp; default_frame_params(fp, qp);
  fp.slice_ctus = e->c.p.slice_ctus; fp.slice_type = FCU_SLICE_P; fp.lambda = lambda; fp.search_range = search_range; fp.fast_search = fast_search;
  fill_params(e->c.p, width, height, fp);
  const uint8_t *const planes[3] = { py, pu, pv };
  const int ref_poc = 0;
  chain_set_list0(e->c, 1, planes, &ref_poc, 1);            /* fcu_chain_set_reference */
}
/* several reference pictures: planes[3r .. 3r+2] = padded Y, U, V of RefPicList0[r] (after fcu_emu_set_p with planes[0..2]) */
void fcu_emu_set_refs(void *h, int n, const uint8_t *const *planes, const int *pocs, int poc, const int *col_ref_pocs, int n_col)
{
  EmuChain *e = (EmuChain *)h;
  chain_set_list0(e->c, n, planes, pocs, poc);              /* fcu_chain_set_references, then fcu_chain_set_collocated_pocs */
  if (n_col > 0) chain_set_collocated_pocs(e->c, pocs[0], col_ref_pocs, n_col);
}
/* lambda of an I picture that is not the intra_main default (lowdelay_P: 0.57 * 0.85) */
void fcu_emu_set_lambda(void *h, int qp, double lambda)
{
  EmuChain *e = (EmuChain *)h;
  fcu_frame_params fp; default_frame_params(fp, qp); fp.slice_ctus = e->c.p.slice_ctus; fp.lambda = lambda;
  fill_params(e->c.p, e->c.p.width, e->c.p.height, fp);
}
void fcu_emu_get_state_full(void *h, uint8_t *ctx, uint64_t *frac) { EmuChain *e = (EmuChain *)h; memcpy(ctx, e->c.state.ctx, NCTX); *frac = e->c.state.frac; }
void fcu_emu_destroy(void *h) { EmuChain *e = (EmuChain *)h; free(e->g); delete e; }
void fcu_emu_compress_ctu(void *h, int a) { EmuChain *e = (EmuChain *)h; compress_ctu(&e->c, e->g, a); e->c.next_ctu = a + 1; }
void fcu_emu_get_state(void *h, uint8_t *ctx, uint64_t *frac) { EmuChain *e = (EmuChain *)h; memcpy(ctx, e->c.state.ctx, NCTX_INTRA); *frac = e->c.state.frac; }
void fcu_emu_set_decision(void *h, int state, const uint8_t *sw_skip, const uint8_t *sw_term, int depth_exception, const int16_t *obf)
{
  chain_set_decision(((EmuChain *)h)->c, state, depth_exception, obf, sw_skip, sw_term);
}
void fcu_emu_set_col(void *h, const fcu_ctu_out *col) { ((EmuChain *)h)->c.col = col; ((EmuChain *)h)->c.p.tmvp = col != nullptr; }
void fcu_emu_set_amp(void *h, int amp) { ((EmuChain *)h)->c.p.amp = amp != 0; }
void fcu_emu_set_cabac_b(void *h, int on) { ((EmuChain *)h)->c.p.cabac_b_table = on != 0; }
void fcu_emu_set_rdoq(void *h, int rdoq, int rdoq_ts) { ((EmuChain *)h)->c.p.rdoq = rdoq; ((EmuChain *)h)->c.p.rdoq_ts = rdoq_ts; }
void fcu_emu_set_pu_trace(void *h, fcu_pu_trace *buf) { ((EmuChain *)h)->c.pu_trace = buf; }
void fcu_emu_get_verify(void *h, double *out24) { memcpy(out24, ((EmuChain *)h)->c.ver, sizeof(double) * 24); }
unsigned long long fcu_emu_tu_trials(void *h) { return ((EmuChain *)h)->c.n_tu_trials; }
int fcu_emu_sizes(int which) { return which == 0 ? (int)sizeof(Scratch) : which == 1 ? (int)sizeof(Shared) : (int)sizeof(Chain); }
}
