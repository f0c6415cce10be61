/*
 * cu_trace_emu.cpp -- TEST-ONLY build of the engine source (-DFCU_EMU) with a CU trace bound: one I or P picture as the chains the
 * library binds for it -- slice chains (fcu_chain_begin + fcu_chain_set_range), WaveFrontSynchro rows, tiles -- with the decision
 * block, the labels and the trace set through the rules of HostState (set_decision, set_labels, set_cu_trace: what the entry points
 * of libfcu.so apply), run in chain order (picture_emu.h); and the kernel bodies of fcu_label_score and fcu_trace_maps (fcu_trace.h)
 * with the HIP keywords defined away and every grid run as a loop (workgroup phases in order, threads inside a phase in order).
 * Built by __graft_entry__.build().  It is NOT part of libfcu.so and nothing in the product path can reach it.
 */
#include "picture_emu.h"
#define __device__
struct Dim3 { unsigned x, y, z; };
static thread_local Dim3 blockIdx, threadIdx;
#include "../../fast-cu-decision-hevc_amd/csrc/fcu_trace.h"

static thread_local std::string g_err;

extern "C" {
const char *cu_trace_emu_last_error(void) { return g_err.c_str(); }

/* One picture.  kind 0: slice chains, a = CTUs per slice (0: one chain over the picture); kind 1: WaveFrontSynchro rows, a =
 * slice_rows (0: one slice); kind 2 / 3: a x b uniform tiles without / with WaveFrontSynchro inside.  The arguments from n_ref on:
 * picture_emu.h.  Null where the library's entry points refuse the arguments. */
void *cu_trace_emu_create(int kind, int width, int height, int qp, int a, int b,
                          const uint8_t *oy, const uint8_t *ou, const uint8_t *ov, uint8_t *ry, uint8_t *ru, uint8_t *rv, fcu_ctu_out *out,
                          int n_ref, double lambda, int search_range, int fast_search, const uint8_t *const *pad_planes, const int *ref_pocs, int poc)
{
  const Planes pl{ oy, ou, ov, ry, ru, rv, out };
  const EmuList0 l0{ n_ref, pad_planes, ref_pocs, poc, nullptr, 0, nullptr };
  const int known = (1 << FCU_MAX_REF) - 1;
  if (kind != 0) {
    const fcu_frame_params fp = emu_frame_params(qp, 0, -1, n_ref, lambda, search_range, fast_search, 0, 0, 0);
    const PictureCut cut = kind == 1 ? (a == 0 ? PictureCut::rows(fp.slice_type) : PictureCut::row_slices(a)) : PictureCut::tiles(a, b, kind == 3);
    return emu_picture(width, height, cut, fp, pl, l0, known);
  }
  const fcu_frame_params fp = emu_frame_params(qp, a, -1, n_ref, lambda, search_range, fast_search, 0, 0, 0);
  const int n_ctu = ((width + 63) / 64) * ((height + 63) / 64), n = a > 0 ? (n_ctu + a - 1) / a : 1;
  EmuPicture *e = new EmuPicture();
  e->hs.init(fcu_seq_params{ width, height, n, 0 });
  for (int k = 0; k < n; k++) {                                /* CuEngine.init_picture with a slice layout */
    int rc = e->hs.chain_begin(k, &fp, pl);
    if (rc == FCU_OK && a > 0) rc = e->hs.set_range(k, k * a, n_ctu - k * a < a ? n_ctu - k * a : a);
    if (rc != FCU_OK) { g_err = e->hs.err; delete e; return nullptr; }
    if (n_ref > 0) chain_set_list0(e->c[(size_t)k], n_ref, pad_planes, ref_pocs, poc);
    e->c[(size_t)k].wpp_mv_known = known;
    e->g.push_back((Scratch *)calloc(1, sizeof(Scratch)));
  }
  return e;
}
void cu_trace_emu_destroy(void *p) { delete (EmuPicture *)p; }
int cu_trace_emu_n(void *p) { return (int)((EmuPicture *)p)->c.size(); }
/* fcu_chain_set_decision / fcu_chain_set_labels / fcu_chain_set_cu_trace on every chain of the picture, in chain order: FCU_OK or
 * the first refusal */
int cu_trace_emu_set_decision(void *p, int state, const uint8_t *sw_skip, const uint8_t *sw_term, int depth_exception, const int16_t *obf)
{
  EmuPicture *e = (EmuPicture *)p;
  fcu_decision_params dp = {};
  dp.state = state; dp.depth_exception = depth_exception; dp.dev_obf = obf;
  for (int d = 0; d < 4; d++) { dp.sw_skip2nx2n[d] = sw_skip ? sw_skip[d] : 0; dp.sw_terminate[d] = sw_term ? sw_term[d] : 0; }
  for (int i = 0; i < (int)e->c.size(); i++) { const int rc = e->hs.set_decision(i, &dp); if (rc != FCU_OK) { g_err = e->hs.err; return rc; } }
  return FCU_OK;
}
int cu_trace_emu_set_labels(void *p, const int8_t *labels)
{
  EmuPicture *e = (EmuPicture *)p;
  for (int i = 0; i < (int)e->c.size(); i++) { const int rc = e->hs.set_labels(i, labels); if (rc != FCU_OK) { g_err = e->hs.err; return rc; } }
  return FCU_OK;
}
int cu_trace_emu_set_trace(void *p, fcu_cu_trace *trace)
{
  EmuPicture *e = (EmuPicture *)p;
  for (int i = 0; i < (int)e->c.size(); i++) { const int rc = e->hs.set_cu_trace(i, trace); if (rc != FCU_OK) { g_err = e->hs.err; return rc; } }
  return FCU_OK;
}
/* the setter on one chain index, which may be out of range or not bound; returns the code, *bound_out = the pointer the chain holds after */
int cu_trace_emu_set_trace_one(void *p, int chain, fcu_cu_trace *trace, void **bound_out)
{
  EmuPicture *e = (EmuPicture *)p;
  const int rc = e->hs.set_cu_trace(chain, trace); g_err = e->hs.err;
  if (bound_out) *bound_out = e->hs.has(chain) ? (void *)e->c[(size_t)chain].cu_trace : nullptr;
  return rc;
}
int cu_trace_emu_run(void *p) { return emu_run((EmuPicture *)p); }
void cu_trace_emu_get_state_full(void *p, int i, uint8_t *ctx, uint64_t *frac) { emu_get_state_full((EmuPicture *)p, i, ctx, frac); }
void cu_trace_emu_get_verify(void *p, double *out24) { emu_get_verify((EmuPicture *)p, out24); }
/* a context without a bound chain: HostState alone */
void *cu_trace_emu_host(int width, int height, int max_chains) { EmuPicture *e = new EmuPicture(); e->hs.init(fcu_seq_params{ width, height, max_chains, 0 }); return e; }
/* the byte ranges of the descriptor the setters copy to the device: out = { off, len } of CR_CU_TRACE, CR_LABELS, CR_DECISION, CR_PU_TRACE,
 * CR_COL, CR_INT_MV, CR_LIST0, CR_RANGE, CR_REF, then offsetof(ver), sizeof(ver), offsetof(state), sizeof(state), offsetof(next_ctu),
 * and the size of the descriptor on the GPU (the end of cu_trace) */
void cu_trace_emu_ranges(size_t *out24)
{
  const ChainRange r[9] = { CR_CU_TRACE, CR_LABELS, CR_DECISION, CR_PU_TRACE, CR_COL, CR_INT_MV, CR_LIST0, CR_RANGE, CR_REF };
  for (int i = 0; i < 9; i++) { out24[2 * i] = r[i].off; out24[2 * i + 1] = r[i].len; }
  out24[18] = offsetof(Chain, ver); out24[19] = sizeof(((Chain *)0)->ver);
  out24[20] = offsetof(Chain, state); out24[21] = sizeof(((Chain *)0)->state);
  out24[22] = offsetof(Chain, next_ctu); out24[23] = offsetof(Chain, cu_trace) + sizeof(void *);
}
int cu_trace_emu_index(int depth, int zidx) { return cu_index(depth, zidx); }
int cu_trace_emu_sizeof(int which) { return which == 0 ? (int)sizeof(fcu_cu_trace) : which == 1 ? (int)sizeof(fcu_ctu_score) : which == 2 ? (int)sizeof(fcu_pic_score) : -1; }

/* mirrors fcu_label_score for w x h pictures */
int cu_trace_emu_score(int w, int h, int n_pics, const fcu_cu_trace *const *trace, const int8_t *const *labels, fcu_pic_score *scores, fcu_ctu_score *ctu)
{
  const int rc = score_args_check(n_pics, trace, labels, scores, g_err);
  if (rc != FCU_OK) return rc;
  const MapsGeom G = maps_geom(w, h, 0, nullptr);
  std::vector<ScorePic> P((size_t)n_pics);
  for (int i = 0; i < n_pics; i++) { P[i].trace = trace[i]; P[i].labels = labels[i]; }
  static ScoreLds L;                                         /* the workgroup's LDS */
  for (unsigned pic = 0; pic < (unsigned)n_pics; pic++) for (unsigned g = 0; g < (unsigned)((G.n_ctu + SCORE_CTUS - 1) / SCORE_CTUS); g++) {
    blockIdx.x = g; blockIdx.y = pic;
    memset(&L, 0xee, sizeof(L));                             /* (nothing may be read that this workgroup did not write) */
    memset(L.cnt, 0, sizeof(L.cnt));                         /* the CPU form of the wave count adds into its word */
    for (unsigned t = 0; t < SCORE_THREADS; t++) { threadIdx.x = t; score_ctu_phase<1>(L, P.data(), ctu, G); }
    for (unsigned t = 0; t < SCORE_THREADS; t++) { threadIdx.x = t; score_ctu_phase<2>(L, P.data(), ctu, G); }
  }
  blockIdx.y = 0;
  for (unsigned pic = 0; pic < (unsigned)n_pics; pic++) {
    blockIdx.x = pic;
    for (unsigned t = 0; t < SCORE_PIC_THREADS; t++) { threadIdx.x = t; score_pic_body(ctu, scores, G.n_ctu); }
  }
  return FCU_OK;
}

/* mirrors fcu_trace_maps */
int cu_trace_emu_maps(int w, int h, int n_pics, const fcu_cu_trace *const *trace, int8_t *labels, double *j0, double *j1)
{
  const int rc = trace_maps_args_check(n_pics, trace, labels, j0, j1, g_err);
  if (rc != FCU_OK) return rc;
  const MapsGeom G = maps_geom(w, h, 0, nullptr);
  const TraceOut Q = { labels, j0, j1 };
  for (unsigned pic = 0; pic < (unsigned)n_pics; pic++) for (unsigned g = 0; g < (unsigned)((G.n_ctu + SCORE_CTUS - 1) / SCORE_CTUS); g++) {
    blockIdx.x = g; blockIdx.y = pic;
    for (unsigned t = 0; t < SCORE_THREADS; t++) { threadIdx.x = t; trace_ctu_body(trace, Q, G); }
  }
  return FCU_OK;
}
}
