/*
 * fcu_kernels.hip -- gfx950 kernel entry + the C ABI of libfcu.so (include/fcu.h).
 *
 * Launch geometry: one 64-thread workgroup (= one wavefront) per chain, grid = number of
 * chains advanced by the call.  Chains are dealt round-robin over the 8 XCDs by the
 * dispatcher; a chain's scratch (fcu::Scratch, ~0.7 MB) is touched only by its own wave,
 * so it stays in that XCD's L2 / the Infinity Cache with no cross-XCD traffic.  The hot CABAC
 * coders, reference samples and per-PU mailboxes live in LDS (fcu::Shared + fcu::HotTables, ~10 KB per chain).
 *
 * There is no CPU fallback: every entry point returns FCU_ERR_NO_DEVICE without a GPU.
 */
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <string>
#include <vector>
#include "fcu_host.h"
#include "fcu_obf.h"
#include "fcu_deblock.h"
#include "fcu_sao.h"
#include "fcu_report.h"
#include "fcu_hash.h"
#include "fcu_maps.h"
#include "fcu_trace.h"
#include "fcu_features.h"
#include "fcu_risk.h"
#include "fcu_tree.h"

using namespace fcu;

/* the chain loop lives in a callable so that the kernel body itself keeps no state across the call
 * (its SGPR spills would otherwise cost two extra VGPRs and the fourth wave per SIMD) */
__device__ __noinline__ static void run_chain(Chain *C, Scratch *G, int ctus)
{
  load_hot_tables();
  for (int k = 0; k < ctus; k++) {
    const int a = C->next_ctu;
    if (a >= C->end_ctu || C->out == nullptr) break;        /* every wave reaches this exit */
    compress_ctu(C, G, a);
    FCU_SERIAL { C->next_ctu = a + 1; }
  }
}

__global__ void __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(FCU_WAVES_PER_EU, FCU_WAVES_PER_EU)))
fcu_ctu_engine(Chain *chains, Scratch *scratch, int first, int ctus)
{
  run_chain(&chains[first + blockIdx.x], &scratch[first + blockIdx.x], ctus);
}

/* WaveFrontSynchro: the row chains [first, first + gridDim.x) of whole pictures, one launch.  A wave takes a ticket and decides
 * chain first + ticket: the rows of a picture are bound top to bottom at increasing chain indices, so the chain a wave waits on
 * holds an earlier ticket and is already running (or done) -- no deadlock whatever the dispatch order, and the launch may hold
 * more chains than are resident.  ctl: fcu_ctx::wpp_ctl, zeroed before every launch. */
__global__ void __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(FCU_WAVES_PER_EU, FCU_WAVES_PER_EU)))
fcu_ctu_engine_wpp(Chain *chains, Scratch *scratch, unsigned *ctl, int first)
{
  unsigned t = 0;
  if (threadIdx.x == 0) t = __hip_atomic_fetch_add((FCU_HBM unsigned *)ctl, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  const int i = first + __builtin_amdgcn_readfirstlane((int)t);
  run_wpp_chain(&chains[i], &scratch[i], ctl, i);
}

/* Reference picture padding (TComPicYuv::extendPicBorder): every thread writes 16 consecutive bytes of one row of a
 * padded plane; the source coordinate is clamped into the picture.  HBM-bound: reads W*H*1.5, writes (W+160)*(H+160)*1.5/.. */
__global__ void __launch_bounds__(256) fcu_pad_plane(const uint8_t *src, int w, int h, uint8_t *dst, int margin)
{
  const int pw = w + 2 * margin, ph = h + 2 * margin, chunks = (pw + 15) >> 4;
  const int t = blockIdx.x * 256 + threadIdx.x;
  if (t >= chunks * ph) return;
  const int y = t / chunks, x0 = (t - y * chunks) << 4;
  int sy = y - margin; sy = sy < 0 ? 0 : (sy >= h ? h - 1 : sy);
  const uint8_t *row = src + (size_t)sy * w;
  uint8_t v[16];
  const int sx0 = x0 - margin;
  if (sx0 >= 0 && sx0 + 16 <= w) __builtin_memcpy(v, row + sx0, 16);
  else for (int k = 0; k < 16; k++) { int sx = sx0 + k; sx = sx < 0 ? 0 : (sx >= w ? w - 1 : sx); v[k] = row[sx]; }
  uint8_t *o = dst + (size_t)y * pw + x0;
  if (x0 + 16 <= pw) __builtin_memcpy(o, v, 16); else for (int k = 0; x0 + k < pw; k++) o[k] = v[k];
}

/* ---------------------------------------------------------------------------------------- */
/* one buffer per host thread: a failure text never races with another thread's call */
static thread_local char g_err[256] = "";
static int fail(int code, const char *msg) { snprintf(g_err, sizeof(g_err), "%s", msg); return code; }
static int fail(int code, const std::string &msg) { return fail(code, msg.c_str()); }
#define HIPCHK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { snprintf(g_err, sizeof(g_err), "%s: %s", #x, hipGetErrorString(e_)); return FCU_ERR_HIP; } } while (0)
#define CHK(x) do { const int rc_ = (x); if (rc_ != FCU_OK) return rc_; } while (0)
/* the first step of an entry point: the rule of fcu_host.h on the host state, its code and text on a refusal */
#define HOST(null_msg, call) do { if (!c) return fail(FCU_ERR_ARG, null_msg); const int rc_ = c->hs.call; if (rc_ != FCU_OK) return fail(rc_, c->hs.err); } while (0)

/* a device block of the context that only grows: no allocation in the steady state.  The old block may still be read by work
 * queued on the stream, so the stream is drained before it is freed. */
struct DevBuf {
  void *p = nullptr; size_t cap = 0;
  hipError_t reserve(size_t bytes, hipStream_t st)
  {
    if (bytes <= cap) return hipSuccess;
    if (p) { const hipError_t e = hipStreamSynchronize(st); if (e != hipSuccess) return e; hipFree(p); p = nullptr; cap = 0; }
    const hipError_t e = hipMalloc(&p, bytes);
    if (e == hipSuccess) cap = bytes;
    return e;
  }
};

/* the events a call times its kernels with: created and recorded only when `on` (the caller asked for times), destroyed on
 * every return */
struct Events {
  hipStream_t st; bool on; hipEvent_t e[5] = {};
  Events(hipStream_t st_, bool on_) : st(st_), on(on_) {}
  ~Events() { for (hipEvent_t x : e) if (x) hipEventDestroy(x); }
  hipError_t create(int n) { for (int i = 0; on && i < n; i++) { const hipError_t r = hipEventCreate(&e[i]); if (r != hipSuccess) return r; } return hipSuccess; }
  hipError_t record(int i) { return on ? hipEventRecord(e[i], st) : hipSuccess; }
  void ms(float *out, int i, int j) { if (on) hipEventElapsedTime(out, e[i], e[j]); }
};

struct fcu_ctx {
  HostState hs;                    /* sequence parameters, host descriptors, positions -- and every rule on them (fcu_host.h) */
  Chain *d_chains = nullptr; Scratch *d_scratch = nullptr;
  std::vector<hipEvent_t> ev;      /* start/stop pairs of launches not yet harvested (bounded, see harvest_events) */
  double ms_acc = 0; int launches = 0;
  DevBuf hist, thr;                /* fcu_obf_prepass: histograms, thresholds */
  DevBuf sao;                      /* fcu_sao: picture descriptors, copy of the deblocked planes, statistics, candidates, reconstructed parameters, off counters */
  DevBuf rep;                      /* fcu_picture_report: picture descriptors, picture records, per-CTU records (when the caller gives none) */
  DevBuf hash;                     /* fcu_picture_hash: plane pointers, hash records, per-chunk partials */
  DevBuf score;                    /* fcu_label_score / fcu_trace_maps: picture descriptors, picture records, per-CTU records (when the caller gives none) */
  DevBuf risk;                     /* fcu_risk_train / fcu_risk_predict / fcu_nobf_maps: pointer arrays, the dropped counter, one table slot per workgroup */
  DevBuf tree;                     /* fcu_tree_keys / fcu_tree_hist / fcu_tree_train: pointer arrays, the tree, the dropped counter, table slots; training: node indices, a level's histograms */
  DevBuf maps;                     /* fcu_decision_maps / fcu_split_match: picture descriptors, picture records, per-CTU records (when the caller gives none) */
  /* WaveFrontSynchro (allocated by the first binder that makes rows chains): wpp_ctl = the words a launch polls (ticket, abort,
   * one progress word per chain), a multiple of 16 bytes, zeroed before every launch; wpp_sync = one slot of WPP_SYNC_BYTES per chain */
  DevBuf wpp_ctl, wpp_sync;
};

/* Launch timing keeps two events per launch until they are read.  A long-running caller that never asks for
 * fcu_kernel_ms must not grow that list without bound: past FCU_MAX_PENDING_EVENTS pairs the oldest are folded
 * into the accumulator (they have long completed; hipEventSynchronize on them returns at once) and destroyed. */
enum { FCU_MAX_PENDING_EVENTS = 64 };
static void harvest_events(fcu_ctx *c, size_t keep_pairs)
{
  while (c->ev.size() > 2 * keep_pairs) {
    float ms = 0.f;
    hipEventSynchronize(c->ev[1]);
    if (hipEventElapsedTime(&ms, c->ev[0], c->ev[1]) == hipSuccess) { c->ms_acc += ms; c->launches++; }
    hipEventDestroy(c->ev[0]); hipEventDestroy(c->ev[1]);
    c->ev.erase(c->ev.begin(), c->ev.begin() + 2);
  }
}
/* an engine launch between its two events */
template <class Launch> static int timed_launch(fcu_ctx *c, hipStream_t st, Launch launch)
{
  hipEvent_t e0, e1;
  HIPCHK(hipEventCreate(&e0)); HIPCHK(hipEventCreate(&e1));
  HIPCHK(hipEventRecord(e0, st));
  launch();
  HIPCHK(hipGetLastError());
  HIPCHK(hipEventRecord(e1, st));
  c->ev.push_back(e0); c->ev.push_back(e1);
  harvest_events(c, FCU_MAX_PENDING_EVENTS);
  return FCU_OK;
}

/* every copy into d_chains: the byte range r (fcu_host.h) of the host descriptors of chains [first, first + n) -- or, with
 * src, the caller's bytes for that range.  sync_first: the chains may be running, the device is drained before the copy. */
static int upload(fcu_ctx *c, int first, int n, ChainRange r, bool sync_first, const void *src = nullptr)
{
  if (sync_first) HIPCHK(hipDeviceSynchronize());
  if (r.len == sizeof(Chain)) { HIPCHK(hipMemcpy(&c->d_chains[first], &c->hs.chains[(size_t)first], sizeof(Chain) * (size_t)n, hipMemcpyHostToDevice)); return FCU_OK; }
  for (int i = first; i < first + n; i++)
    HIPCHK(hipMemcpy((char *)&c->d_chains[i] + r.off, src ? src : (const char *)&c->hs.chains[(size_t)i] + r.off, r.len, hipMemcpyHostToDevice));
  return FCU_OK;
}
/* ... and every whole descriptor back, after the device has finished */
static int read_back(fcu_ctx *c, int first, int n, std::vector<Chain> &h)
{
  HIPCHK(hipSetDevice(c->hs.sp.device));
  HIPCHK(hipDeviceSynchronize());
  h.resize((size_t)n);
  HIPCHK(hipMemcpy(h.data(), &c->d_chains[first], sizeof(Chain) * (size_t)n, hipMemcpyDeviceToHost));
  return FCU_OK;
}

extern "C" {

const char *fcu_last_error(void) { return g_err; }

/* compiler + flags this library was built with (recorded by the build recipe in __graft_entry__.py).  The engine's
 * correctness depends on `-mllvm -amdgpu-remove-redundant-endcf=false`; tests/test_cabi.py asserts it. */
#ifndef FCU_BUILD_FLAGS
#define FCU_BUILD_FLAGS "unrecorded"
#endif
#define FCU_STR2(x) #x
#define FCU_STR(x) FCU_STR2(x)
int fcu_abi_sizeof(int which)
{
  switch (which) {
  case FCU_ABI_CTU_OUT: return (int)sizeof(fcu_ctu_out);
  case FCU_ABI_SEQ_PARAMS: return (int)sizeof(fcu_seq_params);
  case FCU_ABI_FRAME_PARAMS: return (int)sizeof(fcu_frame_params);
  case FCU_ABI_DECISION_PARAMS: return (int)sizeof(fcu_decision_params);
  case FCU_ABI_VERIFY_COUNTS: return (int)sizeof(fcu_verify_counts);
  case FCU_ABI_SAO_CTU: return (int)sizeof(fcu_sao_ctu);
  case FCU_ABI_SAO_PARAMS: return (int)sizeof(fcu_sao_params);
  case FCU_ABI_PU_TRACE: return (int)sizeof(fcu_pu_trace);
  case FCU_ABI_PIC_REPORT: return (int)sizeof(fcu_pic_report);
  case FCU_ABI_CTU_REPORT: return (int)sizeof(fcu_ctu_report);
  case FCU_ABI_PIC_HASH: return (int)sizeof(fcu_pic_hash);
  case FCU_ABI_CTU_MATCH: return (int)sizeof(fcu_ctu_match);
  case FCU_ABI_PIC_MATCH: return (int)sizeof(fcu_pic_match);
  case FCU_ABI_CU_TRACE: return (int)sizeof(fcu_cu_trace);
  case FCU_ABI_CTU_SCORE: return (int)sizeof(fcu_ctu_score);
  case FCU_ABI_PIC_SCORE: return (int)sizeof(fcu_pic_score);
  case FCU_ABI_RISK_MODEL: return (int)sizeof(fcu_risk_model);
  case FCU_ABI_KEY_TREE: return (int)sizeof(fcu_key_tree);
  default: return -1;
  }
}
const char *fcu_build_info(void)
{
  return "hipcc clang " __clang_version__ " HIP " FCU_STR(HIP_VERSION_MAJOR) "." FCU_STR(HIP_VERSION_MINOR) "." FCU_STR(HIP_VERSION_PATCH)
         " waves_per_eu=" FCU_STR(FCU_WAVES_PER_EU) " flags: " FCU_BUILD_FLAGS;
}

void fcu_default_frame_params(fcu_frame_params *fp, int qp) { default_frame_params(*fp, qp); }

int fcu_create(const fcu_seq_params *sp, fcu_ctx **out)
{
  if (!out || !HostState::seq_ok(sp)) return fail(FCU_ERR_ARG, "bad sequence parameters");
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0 || sp->device >= ndev) return fail(FCU_ERR_NO_DEVICE, "no HIP device: libfcu has no CPU fallback");
  HIPCHK(hipSetDevice(sp->device));
  fcu_ctx *c = new fcu_ctx();
  struct Guard { fcu_ctx *c; ~Guard() { if (c) { hipFree(c->d_chains); hipFree(c->d_scratch); delete c; } } } guard{ c };   /* frees on every early return */
  HIPCHK(hipMalloc((void **)&c->d_chains, sizeof(Chain) * (size_t)sp->max_chains));
  HIPCHK(hipMalloc((void **)&c->d_scratch, sizeof(Scratch) * (size_t)sp->max_chains));
  HIPCHK(hipMemset(c->d_chains, 0, sizeof(Chain) * (size_t)sp->max_chains));
  guard.c = nullptr;
  c->hs.init(*sp);
  *out = c;
  return FCU_OK;
}

void fcu_destroy(fcu_ctx *c)
{
  if (!c) return;
  hipSetDevice(c->hs.sp.device);
  hipDeviceSynchronize();
  for (hipEvent_t e : c->ev) hipEventDestroy(e);
  hipFree(c->d_chains); hipFree(c->d_scratch); hipFree(c->hist.p); hipFree(c->thr.p); hipFree(c->sao.p); hipFree(c->rep.p); hipFree(c->hash.p); hipFree(c->maps.p); hipFree(c->score.p); hipFree(c->risk.p); hipFree(c->tree.p);
  hipFree(c->wpp_ctl.p); hipFree(c->wpp_sync.p);
  delete c;
}

int fcu_num_ctus(const fcu_ctx *c) { return c ? c->hs.n_ctu : 0; }

int fcu_chain_begin(fcu_ctx *c, int chain, const fcu_frame_params *fp,
                    const uint8_t *oy, const uint8_t *ou, const uint8_t *ov, uint8_t *ry, uint8_t *ru, uint8_t *rv, fcu_ctu_out *dev_out)
{
  HOST("fcu_chain_begin: bad argument", chain_begin(chain, fp, Planes{ oy, ou, ov, ry, ru, rv, dev_out }));
  HIPCHK(hipSetDevice(c->hs.sp.device));
  return upload(c, chain, 1, CR_ALL, false);
}

void fcu_ldp_slice(fcu_frame_params *fp, int base_qp, int poc) { if (fp) ldp_slice(*fp, base_qp, poc); }

void fcu_pad_sizes(const fcu_ctx *c, size_t *out3)
{
  if (!c || !out3) return;
  out3[0] = (size_t)(c->hs.sp.width + 2 * FCU_REF_MARGIN) * (size_t)(c->hs.sp.height + 2 * FCU_REF_MARGIN);
  out3[1] = out3[2] = (size_t)(c->hs.sp.width / 2 + FCU_REF_MARGIN) * (size_t)(c->hs.sp.height / 2 + FCU_REF_MARGIN);
}
int fcu_ldp_layer(int poc) { static const int layer[4] = { 0, 2, 1, 2 }; return poc < 0 ? 0 : layer[poc & 3]; }

int fcu_pad_reference(fcu_ctx *c, const uint8_t *dy, const uint8_t *du, const uint8_t *dv, uint8_t *py, uint8_t *pu, uint8_t *pv, void *hip_stream)
{
  if (!c || !dy || !du || !dv || !py || !pu || !pv) return fail(FCU_ERR_ARG, "fcu_pad_reference: bad argument");
  HIPCHK(hipSetDevice(c->hs.sp.device));
  hipStream_t st = (hipStream_t)hip_stream;
  const uint8_t *src[3] = { dy, du, dv }; uint8_t *dst[3] = { py, pu, pv };
  for (int k = 0; k < 3; k++) {
    const int w = k ? c->hs.sp.width / 2 : c->hs.sp.width, h = k ? c->hs.sp.height / 2 : c->hs.sp.height, m = k ? FCU_REF_MARGIN / 2 : FCU_REF_MARGIN;
    const int n = ((w + 2 * m + 15) >> 4) * (h + 2 * m);
    hipLaunchKernelGGL(fcu_pad_plane, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, src[k], w, h, dst[k], m);
    HIPCHK(hipGetLastError());
  }
  return FCU_OK;
}

int fcu_chain_set_reference(fcu_ctx *c, int chain, const uint8_t *py, const uint8_t *pu, const uint8_t *pv)
{
  if (!c || !py || !pu || !pv) return fail(FCU_ERR_ARG, "fcu_chain_set_reference: bad argument");
  HOST("", bound("fcu_chain_set_reference", chain));
  HIPCHK(hipSetDevice(c->hs.sp.device));
  /* this entry point: one reference picture at POC distance 1 (no vector is ever scaled), list 0 = { this picture } */
  const uint8_t *const planes[3] = { py, pu, pv };
  const int ref_poc = 0;
  chain_set_list0(c->hs.chains[(size_t)chain], 1, planes, &ref_poc, 1);
  CHK(upload(c, chain, 1, CR_REF, true));
  return upload(c, chain, 1, CR_LIST0, false);
}

int fcu_chain_set_references(fcu_ctx *c, int chain, int n_ref, const uint8_t *const *dev_pad_planes, const int *ref_pocs, int cur_poc)
{
  if (!c || !c->hs.has(chain) || n_ref < 1 || n_ref > FCU_MAX_REF || !dev_pad_planes || !ref_pocs) return fail(FCU_ERR_ARG, "fcu_chain_set_references: bad argument");
  for (int k = 0; k < 3 * n_ref; k++) if (!dev_pad_planes[k]) return fail(FCU_ERR_ARG, "fcu_chain_set_references: null plane");
  for (int a = 0; a < n_ref; a++) { if (ref_pocs[a] == cur_poc) return fail(FCU_ERR_ARG, "fcu_chain_set_references: a reference picture cannot have the current POC");
    for (int b = 0; b < a; b++) if (ref_pocs[a] == ref_pocs[b]) return fail(FCU_ERR_ARG, "fcu_chain_set_references: the same picture twice in the list"); }
  CHK(fcu_chain_set_reference(c, chain, dev_pad_planes[0], dev_pad_planes[1], dev_pad_planes[2]));
  chain_set_list0(c->hs.chains[(size_t)chain], n_ref, dev_pad_planes, ref_pocs, cur_poc);       /* (ref / ref_stride: the values the call above has copied) */
  return upload(c, chain, 1, CR_LIST0, false);
}

int fcu_chain_get_search_state(fcu_ctx *c, int chain, int32_t *xy)
{
  if (!c || !c->hs.has(chain) || !xy) return fail(FCU_ERR_ARG, "fcu_chain_get_search_state: bad argument");
  HIPCHK(hipSetDevice(c->hs.sp.device));
  HIPCHK(hipDeviceSynchronize());
  HIPCHK(hipMemcpy(xy, (const char *)&c->d_chains[chain] + CR_INT_MV.off, CR_INT_MV.len, hipMemcpyDeviceToHost));
  return FCU_OK;
}
int fcu_chain_set_search_state(fcu_ctx *c, int chain, const int32_t *xy)
{
  if (!c || !xy) return fail(FCU_ERR_ARG, "fcu_chain_set_search_state: bad argument");
  HOST("", bound("fcu_chain_set_search_state", chain));
  HIPCHK(hipSetDevice(c->hs.sp.device));
  return upload(c, chain, 1, CR_INT_MV, true, xy);          /* the device copy alone: the host descriptor keeps its own */
}

int fcu_chain_set_collocated_pocs(fcu_ctx *c, int chain, int col_poc, const int *col_ref_pocs, int n)
{
  if (!c || !col_ref_pocs || n < 1 || n > FCU_MAX_REF) return fail(FCU_ERR_ARG, "fcu_chain_set_collocated_pocs: bad argument");
  HOST("", bound("fcu_chain_set_collocated_pocs", chain));
  HIPCHK(hipSetDevice(c->hs.sp.device));
  if (!chain_set_collocated_pocs(c->hs.chains[(size_t)chain], col_poc, col_ref_pocs, n)) return fail(FCU_ERR_ARG, "fcu_chain_set_collocated_pocs: a reference of the collocated picture has its own POC");
  return upload(c, chain, 1, CR_LIST0, true);
}

int fcu_chain_set_range(fcu_ctx *c, int chain, int first_ctu, int n_ctus)
{
  HOST("fcu_chain_set_range: bad argument", set_range(chain, first_ctu, n_ctus));
  HIPCHK(hipSetDevice(c->hs.sp.device));
  /* only the range: the chain's coder state, verification counters and trial count on the device stay as they are */
  return upload(c, chain, 1, CR_RANGE, true);
}

int fcu_compress_chains(fcu_ctx *c, int first, int n, int ctus, void *hip_stream)
{
  HOST("fcu_compress_chains: bad range", chains_check(first, n, ctus));
  HIPCHK(hipSetDevice(c->hs.sp.device));
  hipStream_t st = (hipStream_t)hip_stream;
  CHK(timed_launch(c, st, [&] { hipLaunchKernelGGL(fcu_ctu_engine, dim3((unsigned)n), dim3(64), 0, st, c->d_chains, c->d_scratch, first, ctus); }));
  c->hs.chains_launched(first, n, ctus);
  return FCU_OK;
}

int fcu_wpp_rows(const fcu_ctx *c) { return c ? c->hs.h_ctu : 0; }

/* the five picture entry points: the binder's checks (HostState::picture_check), the WaveFrontSynchro blocks where rows are
 * chains, the descriptors of the picture's chains (HostState::picture_bind), one copy to the device */
static int picture_begin(fcu_ctx *c, const PictureCut &cut, int first_chain, const fcu_frame_params *fp, const Planes &pl)
{
  if (!c) return fail(FCU_ERR_ARG, std::string(cut.name) + ": bad argument");
  { const int rc = c->hs.picture_check(cut, first_chain, fp, pl); if (rc != FCU_OK) return fail(rc, c->hs.err); }
  HIPCHK(hipSetDevice(c->hs.sp.device));
  if (cut.wpp) {                                             /* the control words and sync slots: sized once, so allocated once */
    HIPCHK(c->wpp_ctl.reserve(((size_t)(WPP_CTL_WORDS + c->hs.sp.max_chains) * sizeof(unsigned) + 15) & ~(size_t)15, nullptr));
    HIPCHK(c->wpp_sync.reserve((size_t)WPP_SYNC_BYTES * c->hs.sp.max_chains, nullptr));
  }
  const int n = c->hs.picture_bind(cut, first_chain, *fp, pl, (uint8_t *)c->wpp_sync.p);
  return upload(c, first_chain, n, CR_ALL, false);
}

int fcu_wpp_begin(fcu_ctx *c, int first_chain, const fcu_frame_params *fp,
                  const uint8_t *oy, const uint8_t *ou, const uint8_t *ov, uint8_t *ry, uint8_t *ru, uint8_t *rv, fcu_ctu_out *dev_out)
{
  return picture_begin(c, PictureCut::rows(FCU_SLICE_I), first_chain, fp, Planes{ oy, ou, ov, ry, ru, rv, dev_out });
}

int fcu_wpp_begin_p(fcu_ctx *c, int first_chain, const fcu_frame_params *fp,
                    const uint8_t *oy, const uint8_t *ou, const uint8_t *ov, uint8_t *ry, uint8_t *ru, uint8_t *rv, fcu_ctu_out *dev_out)
{
  return picture_begin(c, PictureCut::rows(FCU_SLICE_P), first_chain, fp, Planes{ oy, ou, ov, ry, ru, rv, dev_out });
}

int fcu_wpp_begin_slices(fcu_ctx *c, int first_chain, const fcu_frame_params *fp, int slice_rows,
                         const uint8_t *oy, const uint8_t *ou, const uint8_t *ov, uint8_t *ry, uint8_t *ru, uint8_t *rv, fcu_ctu_out *dev_out)
{
  return picture_begin(c, PictureCut::row_slices(slice_rows), first_chain, fp, Planes{ oy, ou, ov, ry, ru, rv, dev_out });     /* the slice type: fcu_chain_begin's check */
}

/* ---- tiles of a one-slice picture */
int fcu_tile_grid(int width_in_ctus, int height_in_ctus, int n_cols, int n_rows, int *col_bd, int *row_bd)
{
  if (!tile_grid(width_in_ctus, height_in_ctus, n_cols, n_rows, col_bd, row_bd)) return fail(FCU_ERR_ARG, "fcu_tile_grid: a grid needs 1 <= n_cols <= width and 1 <= n_rows <= height in CTUs (no empty tile)");
  return FCU_OK;
}

int fcu_tile_chains(const fcu_ctx *c, int n_cols, int n_rows, int wpp) { return c ? c->hs.picture_chains(PictureCut::tiles(n_cols, n_rows, wpp)) : -1; }

int fcu_tiles_begin(fcu_ctx *c, int first_chain, const fcu_frame_params *fp, int n_cols, int n_rows,
                    const uint8_t *oy, const uint8_t *ou, const uint8_t *ov, uint8_t *ry, uint8_t *ru, uint8_t *rv, fcu_ctu_out *dev_out)
{
  return picture_begin(c, PictureCut::tiles(n_cols, n_rows, 0), first_chain, fp, Planes{ oy, ou, ov, ry, ru, rv, dev_out });
}

int fcu_wpp_begin_tiles(fcu_ctx *c, int first_chain, const fcu_frame_params *fp, int n_cols, int n_rows,
                        const uint8_t *oy, const uint8_t *ou, const uint8_t *ov, uint8_t *ry, uint8_t *ru, uint8_t *rv, fcu_ctu_out *dev_out)
{
  return picture_begin(c, PictureCut::tiles(n_cols, n_rows, 1), first_chain, fp, Planes{ oy, ou, ov, ry, ru, rv, dev_out });
}

int fcu_compress_wpp(fcu_ctx *c, int first, int n, void *hip_stream)
{
  HOST("fcu_compress_wpp: bad range", wpp_check(first, n));
  HIPCHK(hipSetDevice(c->hs.sp.device));
  hipStream_t st = (hipStream_t)hip_stream;
  unsigned *ctl = (unsigned *)c->wpp_ctl.p;
  HIPCHK(hipMemsetAsync(ctl, 0, c->wpp_ctl.cap, st));          /* ticket, abort and progress words: every launch */
  CHK(timed_launch(c, st, [&] { hipLaunchKernelGGL(fcu_ctu_engine_wpp, dim3((unsigned)n), dim3(64), 0, st, c->d_chains, c->d_scratch, ctl, first); }));
  unsigned abort_word = 0;
  HIPCHK(hipStreamSynchronize(st));
  HIPCHK(hipMemcpy(&abort_word, ctl + 1, sizeof(unsigned), hipMemcpyDeviceToHost));
  if (abort_word) return fail(FCU_ERR_STATE, "fcu_compress_wpp: a row waited for the row above beyond the give-up time; the launch was abandoned");
  c->hs.wpp_launched(first, n);
  return FCU_OK;
}

int fcu_sync(fcu_ctx *c)
{
  if (!c) return fail(FCU_ERR_ARG, "null ctx");
  HIPCHK(hipSetDevice(c->hs.sp.device));
  HIPCHK(hipDeviceSynchronize());
  return FCU_OK;
}

double fcu_kernel_ms(fcu_ctx *c, int *launches)
{
  if (!c) return 0.0;
  hipSetDevice(c->hs.sp.device);
  hipDeviceSynchronize();
  harvest_events(c, 0);
  const int n = c->launches; const double avg = n ? c->ms_acc / n : 0.0;
  if (launches) *launches = n;
  c->ms_acc = 0; c->launches = 0;
  return avg;
}

int fcu_chain_position(fcu_ctx *c, int chain) { return c ? c->hs.position(chain) : -1; }

int fcu_compress_ctu(fcu_ctx *c, int chain, uint32_t ctuRsAddr, fcu_ctu_out *host_out)
{
  if (!c || !host_out) return fail(FCU_ERR_ARG, "fcu_compress_ctu: bad argument");
  HOST("", ctu_check(chain, ctuRsAddr));
  CHK(fcu_compress_chains(c, chain, 1, 1, nullptr));
  HIPCHK(hipDeviceSynchronize());
  HIPCHK(hipMemcpy(host_out, c->hs.chains[(size_t)chain].out + ctuRsAddr, sizeof(fcu_ctu_out), hipMemcpyDeviceToHost));
  return FCU_OK;
}

/* diagnostic: per-chain section timers (only meaningful in a -DFCU_PROFILE build) and TU-trial count */
int fcu_debug_counters(fcu_ctx *c, int chain, unsigned long long *out17)
{
  if (!c || !c->hs.has(chain) || !out17) return fail(FCU_ERR_ARG, "fcu_debug_counters: bad argument");
  std::vector<Chain> h;
  CHK(read_back(c, chain, 1, h));
  for (int i = 0; i < 16; i++) out17[i] = h[0].prof[i];
  out17[16] = h[0].n_tu_trials;
  return FCU_OK;
}

/* the coder state a chain stands at: n_ctx = NCTX_INTRA (fcu_get_ctx_state) or NCTX (fcu_get_ctx_state_full) context bytes */
static int get_ctx_state(fcu_ctx *c, int chain, uint8_t *ctx, int n_ctx, uint64_t *frac_bits, const char *name)
{
  if (!c || !c->hs.has(chain) || !ctx || !frac_bits) return fail(FCU_ERR_ARG, std::string(name) + ": bad argument");
  std::vector<Chain> h;
  CHK(read_back(c, chain, 1, h));
  memcpy(ctx, h[0].state.ctx, (size_t)n_ctx);
  *frac_bits = h[0].state.frac;
  return FCU_OK;
}
int fcu_get_ctx_state(fcu_ctx *c, int chain, uint8_t *ctx160, uint64_t *frac_bits) { return get_ctx_state(c, chain, ctx160, NCTX_INTRA, frac_bits, "fcu_get_ctx_state"); }
int fcu_get_ctx_state_full(fcu_ctx *c, int chain, uint8_t *ctx176, uint64_t *frac_bits) { return get_ctx_state(c, chain, ctx176, NCTX, frac_bits, "fcu_get_ctx_state_full"); }

int fcu_chain_set_decision(fcu_ctx *c, int chain, const fcu_decision_params *dp)
{
  HOST("fcu_chain_set_decision: bad argument", set_decision(chain, dp));
  HIPCHK(hipSetDevice(c->hs.sp.device));
  /* only the decision block of the descriptor: the chain's position and context state on the device stay as they are */
  return upload(c, chain, 1, CR_DECISION, true);
}

int fcu_chain_set_labels(fcu_ctx *c, int chain, const int8_t *dev_labels)
{
  HOST("fcu_chain_set_labels: bad argument", set_labels(chain, dev_labels));
  HIPCHK(hipSetDevice(c->hs.sp.device));
  /* only the label fields: the decision block, the search state and everything in front of them on the device stay as they are */
  return upload(c, chain, 1, CR_LABELS, true);
}
int fcu_label_count(const fcu_ctx *c) { return c ? c->hs.label_count() : 0; }

int fcu_chain_set_collocated(fcu_ctx *c, int chain, const fcu_ctu_out *dev_col_out)
{
  HOST("fcu_chain_set_collocated: bad argument", bound("fcu_chain_set_collocated", chain));
  Chain &h = c->hs.chains[(size_t)chain];
  if (dev_col_out == h.out) return fail(FCU_ERR_ARG, "fcu_chain_set_collocated: the collocated picture's array is the chain's own output array");
  HIPCHK(hipSetDevice(c->hs.sp.device));
  h.col = dev_col_out;
  return upload(c, chain, 1, CR_COL, true);
}
int fcu_pu_index(int depth, int nxn, int zidx) { return nxn ? 85 + zidx : (depth <= 0 ? 0 : depth == 1 ? 1 + (zidx >> 6) : depth == 2 ? 5 + (zidx >> 4) : 21 + (zidx >> 2)); }
int fcu_chain_set_pu_trace(fcu_ctx *c, int chain, fcu_pu_trace *dev_trace)
{
  HOST("fcu_chain_set_pu_trace: bad argument", set_pu_trace(chain, dev_trace));
  HIPCHK(hipSetDevice(c->hs.sp.device));
  return upload(c, chain, 1, CR_PU_TRACE, true);
}
int fcu_cu_index(int depth, int zidx) { return cu_index(depth, zidx); }
int fcu_chain_set_cu_trace(fcu_ctx *c, int chain, fcu_cu_trace *dev_trace)
{
  HOST("fcu_chain_set_cu_trace: bad argument", set_cu_trace(chain, dev_trace));
  HIPCHK(hipSetDevice(c->hs.sp.device));
  /* only the pointer: position, coder state, counters, search state and labels on the device stay as they are */
  return upload(c, chain, 1, CR_CU_TRACE, true);
}

int fcu_get_verify_counts(fcu_ctx *c, int first, int n, fcu_verify_counts *host_sum)
{
  if (!c || !host_sum || first < 0 || n <= 0 || first + n > c->hs.sp.max_chains) return fail(FCU_ERR_ARG, "fcu_get_verify_counts: bad argument");
  std::vector<Chain> h;
  CHK(read_back(c, first, n, h));
  memset(host_sum, 0, sizeof(*host_sum));
  for (int i = 0; i < n; i++) for (int d = 0; d < 4; d++) for (int k = 0; k < 6; k++) host_sum->n[d][k] += h[(size_t)i].ver[d][k];
  return FCU_OK;
}

void fcu_decision_switch(const fcu_verify_counts *v, const double th_skip[4], const double th_term[4], uint8_t sw_skip[4], uint8_t sw_term[4])
{
  for (int d = 0; d < 4; d++) {
    const double tp = v->n[d][0], fp = v->n[d][1], tn = v->n[d][2], fn = v->n[d][3];
    const double ths = (th_skip && th_skip[d] != 0) ? th_skip[d] : 0.8, tht = (th_term && th_term[d] != 0) ? th_term[d] : 0.8;
    const double ps = (tp + fp == 0) ? 0.0 : tp / (tp + fp);            /* getSkipPrecision, tools_YS.cpp:1251-1258 */
    const double pt = (tn + fn == 0) ? 0.0 : tn / (tn + fn);            /* getTermPrecision, :1259-1266 */
    sw_skip[d] = ps > ths; sw_term[d] = pt > tht;
  }
}

int fcu_frame_state(int poc, int period, int n_training, int n_verifying)
{
  if (period <= 0) return FCU_TRAINING;
  const int r = poc % period;
  return r < n_training ? FCU_TRAINING : (r < n_training + n_verifying ? FCU_VERIFYING : FCU_TESTING);
}

/* diagnostic: resident workgroups (= chains) per CU the runtime grants the engine kernel */
int fcu_chains_per_cu(void)
{
  int n = 0;
  if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, fcu_ctu_engine, 64, 0) != hipSuccess) return -1;
  return n;
}

/* the host step of the pre-pass on its own: Yc of one frequency from its amplitude histogram (pure host arithmetic, no GPU) */
double fcu_tcm_threshold(const unsigned *hist, int hist_len, int n_samples)
{
  if (!hist || hist_len <= 0 || n_samples <= 0) return 0.0;
  std::vector<unsigned> h((size_t)OBF_HB, 0u);
  for (int i = 0; i < hist_len && i < OBF_HB; i++) h[(size_t)i] = hist[i];
  return tcm_threshold(h.data(), n_samples);
}

/* ---- fork pre-pass: OBF maps of n luma planes ------------------------------------------------------------ */
int fcu_obf_prepass(fcu_ctx *c, int n_frames, const uint8_t *dev_y, int16_t *dev_obf, double *host_yc, float *kernel_ms2, void *hip_stream)
{
  if (!c || n_frames <= 0 || !dev_y || !dev_obf) return fail(FCU_ERR_ARG, "fcu_obf_prepass: bad argument");
  HIPCHK(hipSetDevice(c->hs.sp.device));
  hipStream_t st = (hipStream_t)hip_stream;
  const int w = c->hs.sp.width, h = c->hs.sp.height, nblk = (w / 4) * (h / 4);
  const size_t frame_bytes = (size_t)w * h, hist_n = (size_t)n_frames * 15 * OBF_HB;
  /* histogram / threshold buffers belong to the context and only grow: no allocation in the steady state */
  HIPCHK(c->hist.reserve(hist_n * sizeof(unsigned), st));
  HIPCHK(c->thr.reserve((size_t)n_frames * 16 * sizeof(int), st));
  unsigned *d_hist = (unsigned *)c->hist.p; int *d_thr = (int *)c->thr.p;
  HIPCHK(hipMemsetAsync(d_hist, 0, hist_n * sizeof(unsigned), st));
  Events ev(st, true);                                         /* (this call syncs with the host anyway: always timed) */
  HIPCHK(ev.create(4));
  const int ngrp = (((w / 4) + 3) / 4) * (h / 4);               /* groups of four blocks along a row */
  const dim3 grid((unsigned)((ngrp + OBF_THREADS * OBF_GROUPS_PER_THREAD - 1) / (OBF_THREADS * OBF_GROUPS_PER_THREAD)), (unsigned)n_frames);
  HIPCHK(ev.record(0));
  hipLaunchKernelGGL(obf_hist, grid, dim3(OBF_THREADS), 0, st, dev_y, w, h, frame_bytes, d_hist);
  HIPCHK(hipGetLastError());
  HIPCHK(ev.record(1));
  std::vector<unsigned> hist(hist_n);
  HIPCHK(hipMemcpyAsync(hist.data(), d_hist, hist_n * sizeof(unsigned), hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  /* threshold fit on the host (doubles + libm exp/log, as the reference), frames spread over a few threads */
  std::vector<double> yc((size_t)n_frames * 16, 0.0);
  std::vector<int> thr((size_t)n_frames * 16, 0);
  {
    const int nt = n_frames < 8 ? n_frames : 8;
    std::vector<std::thread> pool;
    for (int t = 0; t < nt; t++)
      pool.emplace_back([&, t]() {
        for (int f = t; f < n_frames; f += nt)
          for (int x = 1; x < 16; x++) {
            const double v = tcm_threshold(&hist[((size_t)f * 15 + (x - 1)) * OBF_HB], nblk);
            yc[(size_t)f * 16 + x] = v; thr[(size_t)f * 16 + x] = obf_thr(v);
          }
      });
    for (auto &th : pool) th.join();
  }
  for (size_t k = 0; k < (size_t)n_frames * 15; k++)           /* the clamp bin is unreachable for 8-bit sources (|coef/8| <= 4080) */
    if (hist[k * OBF_HB + OBF_HB - 1]) { return fail(FCU_ERR_ARG, "fcu_obf_prepass: amplitude beyond the histogram (not an 8-bit plane?)"); }
  HIPCHK(hipMemcpyAsync(d_thr, thr.data(), thr.size() * sizeof(int), hipMemcpyHostToDevice, st));
  HIPCHK(ev.record(2));
  hipLaunchKernelGGL(obf_count, grid, dim3(OBF_THREADS), 0, st, dev_y, w, h, frame_bytes, d_thr, dev_obf);
  HIPCHK(hipGetLastError());
  HIPCHK(ev.record(3));
  HIPCHK(hipStreamSynchronize(st));
  if (kernel_ms2) { ev.ms(&kernel_ms2[0], 0, 1); ev.ms(&kernel_ms2[1], 2, 3); }
  if (host_yc) memcpy(host_yc, yc.data(), yc.size() * sizeof(double));
  return FCU_OK;
}

} /* extern "C" */

/* the grid of fcu_deblock_tiles / fcu_sao_tiles as the kernels take it; FCU_ERR_ARG with the entry point's name */
static int lf_tiles_arg(const fcu_ctx *c, int n_cols, int n_rows, int lf_cross_tiles, const char *name, LfTiles &T)
{
  if (lf_cross_tiles != 0 && lf_cross_tiles != 1) return fail(FCU_ERR_ARG, std::string(name) + ": lf_cross_tiles (LFCrossTileBoundaryFlag) is 0 or 1");
  const int W = c->hs.w_ctu, H = c->hs.h_ctu;
  if (!tile_grid(W, H, n_cols, n_rows, nullptr, nullptr)) return fail(FCU_ERR_ARG, std::string(name) + ": a grid needs 1 <= n_cols <= width and 1 <= n_rows <= height in CTUs (no empty tile)");
  if (!lf_tiles_fill(T, W, H, n_cols, n_rows, lf_cross_tiles)) return fail(FCU_ERR_ARG, std::string(name) + ": pictures beyond 256 CTUs in width or height are not supported with tiles");
  return FCU_OK;
}

/* the slices of fcu_deblock_slices / fcu_sao_slices; FCU_ERR_ARG with the entry point's name */
static int lf_slices_arg(int slice_ctus, int lf_cross_slices, const char *name)
{
  if (lf_cross_slices != 0 && lf_cross_slices != 1) return fail(FCU_ERR_ARG, std::string(name) + ": lf_cross_slices (LFCrossSliceBoundaryFlag) is 0 or 1");
  if (slice_ctus < 0) return fail(FCU_ERR_ARG, std::string(name) + ": slice_ctus must not be negative (0 = one slice per picture)");
  return FCU_OK;
}

/* fcu_deblock (T and S null: the kernels without a grid), fcu_deblock_tiles (T) and fcu_deblock_slices (S, where the slices cut) */
static int deblock_run(fcu_ctx *c, const char *name, const LfTiles *T, const LfSlices *S, const fcu_ctu_out *dev_out, uint8_t *dev_rec_y, uint8_t *dev_rec_u, uint8_t *dev_rec_v,
                       int beta_offset_div2, int tc_offset_div2, float *kernel_ms2, void *hip_stream)
{
  if (!dev_out || !dev_rec_y || !dev_rec_u || !dev_rec_v) return fail(FCU_ERR_ARG, std::string(name) + ": bad argument");
  if (beta_offset_div2 < -6 || beta_offset_div2 > 6 || tc_offset_div2 < -6 || tc_offset_div2 > 6) return fail(FCU_ERR_ARG, std::string(name) + ": offsets are limited to [-6, 6]");
  HIPCHK(hipSetDevice(c->hs.sp.device));
  hipStream_t st = (hipStream_t)hip_stream;
  const int w = c->hs.sp.width, h = c->hs.sp.height, w_ctu = c->hs.w_ctu;
  const unsigned n0 = (unsigned)((w >> 3) * (h >> 2)), n1 = (unsigned)((w >> 2) * (h >> 3));
  Events ev(st, kernel_ms2 != nullptr);
  HIPCHK(ev.create(3)); HIPCHK(ev.record(0));
  /* all vertical edges of the picture before the first horizontal one (TComLoopFilter.cpp:133-154): stream order */
  const dim3 g0((n0 + DBK_THREADS - 1) / DBK_THREADS), g1((n1 + DBK_THREADS - 1) / DBK_THREADS);
  if (T) hipLaunchKernelGGL((dbk_pass<0, LF_CUT_TILES>), g0, dim3(DBK_THREADS), 0, st, dev_out, dev_rec_y, dev_rec_u, dev_rec_v, w, h, w_ctu, beta_offset_div2, tc_offset_div2, DbkGrid<LF_CUT_TILES>{ *T });
  else if (S) hipLaunchKernelGGL((dbk_pass<0, LF_CUT_SLICES>), g0, dim3(DBK_THREADS), 0, st, dev_out, dev_rec_y, dev_rec_u, dev_rec_v, w, h, w_ctu, beta_offset_div2, tc_offset_div2, DbkGrid<LF_CUT_SLICES>{ *S });
  else hipLaunchKernelGGL((dbk_pass<0, LF_CUT_NONE>), g0, dim3(DBK_THREADS), 0, st, dev_out, dev_rec_y, dev_rec_u, dev_rec_v, w, h, w_ctu, beta_offset_div2, tc_offset_div2, DbkGrid<LF_CUT_NONE>());
  HIPCHK(hipGetLastError());
  HIPCHK(ev.record(1));
  if (T) hipLaunchKernelGGL((dbk_pass<1, LF_CUT_TILES>), g1, dim3(DBK_THREADS), 0, st, dev_out, dev_rec_y, dev_rec_u, dev_rec_v, w, h, w_ctu, beta_offset_div2, tc_offset_div2, DbkGrid<LF_CUT_TILES>{ *T });
  else if (S) hipLaunchKernelGGL((dbk_pass<1, LF_CUT_SLICES>), g1, dim3(DBK_THREADS), 0, st, dev_out, dev_rec_y, dev_rec_u, dev_rec_v, w, h, w_ctu, beta_offset_div2, tc_offset_div2, DbkGrid<LF_CUT_SLICES>{ *S });
  else hipLaunchKernelGGL((dbk_pass<1, LF_CUT_NONE>), g1, dim3(DBK_THREADS), 0, st, dev_out, dev_rec_y, dev_rec_u, dev_rec_v, w, h, w_ctu, beta_offset_div2, tc_offset_div2, DbkGrid<LF_CUT_NONE>());
  HIPCHK(hipGetLastError());
  HIPCHK(ev.record(2));
  if (kernel_ms2) { HIPCHK(hipStreamSynchronize(st)); ev.ms(&kernel_ms2[0], 0, 1); ev.ms(&kernel_ms2[1], 1, 2); }
  return FCU_OK;
}

static size_t up(size_t v) { return (v + 255) & ~(size_t)255; }      /* sub-blocks of a DevBuf start at multiples of 256 bytes */
/* fcu_sao (T null, no_cross_slices false: the kernels without a grid), fcu_sao_tiles (T) and fcu_sao_slices (no_cross_slices =
 * LFCrossSliceBoundaryFlag 0: the slice variants of the statistics and the offset pass, where a picture of the batch has slices) */
static int sao_run(fcu_ctx *c, const char *name_, const LfTiles *T, bool no_cross_slices, int n_pics, const fcu_sao_params *params, const uint8_t *const *dev_org, uint8_t *const *dev_rec,
                   fcu_sao_ctu *dev_coded, int32_t *off_count, float *kernel_ms4, void *hip_stream)
{
  const std::string name(name_);
  if (n_pics <= 0 || !params || !dev_org || !dev_rec || !dev_coded) return fail(FCU_ERR_ARG, name + ": bad argument");
  for (int i = 0; i < 3 * n_pics; i++) if (!dev_org[i] || !dev_rec[i]) return fail(FCU_ERR_ARG, name + ": null plane");
  for (int i = 0; i < n_pics; i++) {
    if (params[i].slice_type != FCU_SLICE_I && params[i].slice_type != FCU_SLICE_P) return fail(FCU_ERR_ARG, name + ": slice type");
    if (params[i].qp < 0 || params[i].qp > 51 || params[i].slice_ctus < 0) return fail(FCU_ERR_ARG, name + ": qp / slice_ctus");
    if (T && params[i].slice_ctus != 0) return fail(FCU_ERR_ARG, name + ": tiles need one slice per picture (slice_ctus 0)");
    if (!(params[i].lambda[0] > 0) || params[i].lambda[1] < 0 || params[i].lambda[2] < 0) return fail(FCU_ERR_ARG, name + ": lambda[0] must be positive");
  }
  HIPCHK(hipSetDevice(c->hs.sp.device));
  hipStream_t st = (hipStream_t)hip_stream;
  const int w = c->hs.sp.width, h = c->hs.sp.height, w_ctu = c->hs.w_ctu, n_ctu = c->hs.n_ctu;
  bool SL = false;                                           /* one slice in every picture: nothing to cut, the plain kernels */
  for (int i = 0; i < n_pics && no_cross_slices; i++) { LfSlices S; SL = SL || lf_slices_fill(S, n_ctu, params[i].slice_ctus, 0); }
  if (w_ctu + 1 > SAO_RING) return fail(FCU_ERR_ARG, name + ": pictures wider than 255 CTUs are not supported (sao_decide's neighbour ring)");
  const size_t plane[3] = { (size_t)w * h, (size_t)(w / 2) * (h / 2), (size_t)(w / 2) * (h / 2) }, pic_bytes = plane[0] + 2 * plane[1];
  const size_t o_pics = 0, o_src = up(o_pics + sizeof(SaoPic) * n_pics), o_stats = up(o_src + pic_bytes * n_pics),
               o_cand = up(o_stats + sizeof(int32_t) * SAO_STAT_INTS * 3 * (size_t)n_ctu * n_pics),
               o_recon = up(o_cand + sizeof(SaoCand) * 15 * (size_t)n_ctu * n_pics),
               o_off = up(o_recon + sizeof(fcu_sao_ctu) * (size_t)n_ctu * n_pics), total = up(o_off + sizeof(int32_t) * 3 * n_pics);
  HIPCHK(c->sao.reserve(total, st));
  uint8_t *base = (uint8_t *)c->sao.p;
  SaoPic *d_pics = (SaoPic *)(base + o_pics); int32_t *d_stats = (int32_t *)(base + o_stats); SaoCand *d_cand = (SaoCand *)(base + o_cand);
  fcu_sao_ctu *d_recon = (fcu_sao_ctu *)(base + o_recon); int32_t *d_off = (int32_t *)(base + o_off);
  std::vector<SaoPic> hp((size_t)n_pics);
  for (int i = 0; i < n_pics; i++) {
    uint8_t *s = base + o_src + pic_bytes * (size_t)i;
    for (int k = 0; k < 3; k++) {
      hp[i].org[k] = dev_org[3 * i + k]; hp[i].rec[k] = dev_rec[3 * i + k]; hp[i].src[k] = s;
      HIPCHK(hipMemcpyAsync(s, dev_rec[3 * i + k], plane[k], hipMemcpyDeviceToDevice, st));      /* resYuv->copyToPic(srcYuv), :265 */
      s += plane[k];
      hp[i].enabled[k] = params[i].enabled[k] ? 1 : 0;
    }
    fcu_frame_params fp; default_frame_params(fp, params[i].qp); fp.lambda = params[i].lambda[0];
    Params pp; fill_params(pp, w, h, fp);                      /* chroma lambdas = lambda / chroma weight (setUpLambda) unless given */
    for (int k = 0; k < 3; k++) hp[i].lambda[k] = params[i].lambda[k] > 0 ? params[i].lambda[k] : pp.rdoq_lambda[k];
    hp[i].slice_type = params[i].slice_type; hp[i].qp = params[i].qp; hp[i].slice_ctus = params[i].slice_ctus;
  }
  HIPCHK(hipMemcpyAsync(d_pics, hp.data(), sizeof(SaoPic) * n_pics, hipMemcpyHostToDevice, st));
  Events ev(st, kernel_ms4 != nullptr);
  HIPCHK(ev.create(5)); HIPCHK(ev.record(0));
  if (T) hipLaunchKernelGGL(sao_stats_tiles, dim3(n_ctu, 3, n_pics), dim3(SAO_THREADS), 0, st, d_pics, d_stats, w, h, w_ctu, n_ctu, *T);
  else if (SL) hipLaunchKernelGGL(sao_stats_slices, dim3(n_ctu, 3, n_pics), dim3(SAO_THREADS), 0, st, d_pics, d_stats, w, h, w_ctu, n_ctu);
  else hipLaunchKernelGGL(sao_stats, dim3(n_ctu, 3, n_pics), dim3(SAO_THREADS), 0, st, d_pics, d_stats, w, h, w_ctu, n_ctu);
  HIPCHK(hipGetLastError());
  HIPCHK(ev.record(1));
  const long long n_cand = (long long)n_pics * n_ctu * 15;
  hipLaunchKernelGGL(sao_cands, dim3((unsigned)((n_cand + SAO_THREADS - 1) / SAO_THREADS)), dim3(SAO_THREADS), 0, st, d_pics, d_stats, d_cand, n_ctu, n_pics);
  HIPCHK(hipGetLastError());
  HIPCHK(ev.record(2));
  if (T) hipLaunchKernelGGL(sao_decide_tiles, dim3(n_pics), dim3(64), 0, st, d_pics, d_stats, d_cand, dev_coded, d_recon, d_off, w_ctu, n_ctu, n_pics, *T);
  else hipLaunchKernelGGL(sao_decide, dim3(n_pics), dim3(64), 0, st, d_pics, d_stats, d_cand, dev_coded, d_recon, d_off, w_ctu, n_ctu, n_pics);
  HIPCHK(hipGetLastError());
  HIPCHK(ev.record(3));
  if (T) hipLaunchKernelGGL(sao_apply_tiles, dim3(n_ctu, 3, n_pics), dim3(SAO_THREADS), 0, st, d_pics, d_recon, w, h, w_ctu, n_ctu, *T);
  else if (SL) hipLaunchKernelGGL(sao_apply_slices, dim3(n_ctu, 3, n_pics), dim3(SAO_THREADS), 0, st, d_pics, d_recon, w, h, w_ctu, n_ctu);
  else hipLaunchKernelGGL(sao_apply, dim3(n_ctu, 3, n_pics), dim3(SAO_THREADS), 0, st, d_pics, d_recon, w, h, w_ctu, n_ctu);
  HIPCHK(hipGetLastError());
  HIPCHK(ev.record(4));
  if (off_count) HIPCHK(hipMemcpyAsync(off_count, d_off, sizeof(int32_t) * 3 * n_pics, hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));                          /* hp (the host descriptors) and off_count are done with */
  if (kernel_ms4) for (int i = 0; i < 4; i++) ev.ms(&kernel_ms4[i], i, i + 1);
  return FCU_OK;
}

extern "C" {

int fcu_deblock(fcu_ctx *c, const fcu_ctu_out *dev_out, uint8_t *dev_rec_y, uint8_t *dev_rec_u, uint8_t *dev_rec_v,
                int beta_offset_div2, int tc_offset_div2, float *kernel_ms2, void *hip_stream)
{
  if (!c) return fail(FCU_ERR_ARG, "fcu_deblock: bad argument");
  return deblock_run(c, "fcu_deblock", nullptr, nullptr, dev_out, dev_rec_y, dev_rec_u, dev_rec_v, beta_offset_div2, tc_offset_div2, kernel_ms2, hip_stream);
}

int fcu_deblock_tiles(fcu_ctx *c, const fcu_ctu_out *dev_out, uint8_t *dev_rec_y, uint8_t *dev_rec_u, uint8_t *dev_rec_v,
                      int beta_offset_div2, int tc_offset_div2, int n_cols, int n_rows, int lf_cross_tiles, float *kernel_ms2, void *hip_stream)
{
  if (!c) return fail(FCU_ERR_ARG, "fcu_deblock_tiles: bad argument");
  LfTiles T;
  const int rc = lf_tiles_arg(c, n_cols, n_rows, lf_cross_tiles, "fcu_deblock_tiles", T);
  if (rc != FCU_OK) return rc;
  return deblock_run(c, "fcu_deblock_tiles", &T, nullptr, dev_out, dev_rec_y, dev_rec_u, dev_rec_v, beta_offset_div2, tc_offset_div2, kernel_ms2, hip_stream);
}

int fcu_sao(fcu_ctx *c, int n_pics, const fcu_sao_params *params, const uint8_t *const *dev_org, uint8_t *const *dev_rec,
            fcu_sao_ctu *dev_coded, int32_t *off_count, float *kernel_ms4, void *hip_stream)
{
  if (!c) return fail(FCU_ERR_ARG, "fcu_sao: bad argument");
  return sao_run(c, "fcu_sao", nullptr, false, n_pics, params, dev_org, dev_rec, dev_coded, off_count, kernel_ms4, hip_stream);
}

int fcu_sao_tiles(fcu_ctx *c, int n_pics, const fcu_sao_params *params, int n_cols, int n_rows, int lf_cross_tiles,
                  const uint8_t *const *dev_org, uint8_t *const *dev_rec, fcu_sao_ctu *dev_coded, int32_t *off_count, float *kernel_ms4, void *hip_stream)
{
  if (!c) return fail(FCU_ERR_ARG, "fcu_sao_tiles: bad argument");
  LfTiles T;
  const int rc = lf_tiles_arg(c, n_cols, n_rows, lf_cross_tiles, "fcu_sao_tiles", T);
  if (rc != FCU_OK) return rc;
  return sao_run(c, "fcu_sao_tiles", &T, false, n_pics, params, dev_org, dev_rec, dev_coded, off_count, kernel_ms4, hip_stream);
}

int fcu_deblock_slices(fcu_ctx *c, const fcu_ctu_out *dev_out, uint8_t *dev_rec_y, uint8_t *dev_rec_u, uint8_t *dev_rec_v,
                       int beta_offset_div2, int tc_offset_div2, int slice_ctus, int lf_cross_slices, float *kernel_ms2, void *hip_stream)
{
  if (!c) return fail(FCU_ERR_ARG, "fcu_deblock_slices: bad argument");
  const int rc = lf_slices_arg(slice_ctus, lf_cross_slices, "fcu_deblock_slices");
  if (rc != FCU_OK) return rc;
  LfSlices S;
  const bool cut = lf_slices_fill(S, c->hs.n_ctu, slice_ctus, lf_cross_slices);      /* false: fcu_deblock's kernels */
  return deblock_run(c, "fcu_deblock_slices", nullptr, cut ? &S : nullptr, dev_out, dev_rec_y, dev_rec_u, dev_rec_v, beta_offset_div2, tc_offset_div2, kernel_ms2, hip_stream);
}

int fcu_sao_slices(fcu_ctx *c, int n_pics, const fcu_sao_params *params, int lf_cross_slices,
                   const uint8_t *const *dev_org, uint8_t *const *dev_rec, fcu_sao_ctu *dev_coded, int32_t *off_count, float *kernel_ms4, void *hip_stream)
{
  if (!c) return fail(FCU_ERR_ARG, "fcu_sao_slices: bad argument");
  const int rc = lf_slices_arg(0, lf_cross_slices, "fcu_sao_slices");       /* (each picture's slice_ctus: sao_run) */
  if (rc != FCU_OK) return rc;
  return sao_run(c, "fcu_sao_slices", nullptr, lf_cross_slices == 0, n_pics, params, dev_org, dev_rec, dev_coded, off_count, kernel_ms4, hip_stream);
}

void fcu_sao_enabled(const double rate[3][8], int layer, int32_t enabled[3])
{
  static const double thr[3] = { 0.75, 0.5, 0.5 };           /* SAO_ENCODING_RATE / SAO_ENCODING_RATE_CHROMA, TypeDef.h:201-204 */
  for (int k = 0; k < 3; k++) enabled[k] = (layer > 0 && layer <= 8 && rate[k][layer - 1] > thr[k]) ? 0 : 1;
}
void fcu_sao_update_rate(double rate[3][8], int layer, const int32_t off_count[3], int num_ctus)
{
  if (layer < 0 || layer >= 8 || num_ctus <= 0) return;
  for (int k = 0; k < 3; k++) rate[k][layer] = (double)off_count[k] / (double)num_ctus;
}

/* TEncGOP::xCalculateAddPSNR of n_pics pictures: report_ctu + report_pic (fcu_report.h), the records back, PSNR on the host */
int fcu_picture_report(fcu_ctx *c, int n_pics, const uint8_t *const *dev_org, const uint8_t *const *dev_rec, const fcu_ctu_out *const *dev_out,
                       fcu_pic_report *host_reports, fcu_ctu_report *dev_ctu, float *kernel_ms2, void *hip_stream)
{
  if (!c) return fail(FCU_ERR_ARG, "fcu_picture_report: null context");
  if (n_pics < 1) return fail(FCU_ERR_ARG, "fcu_picture_report: n_pics must be at least 1");
  if (!dev_org) return fail(FCU_ERR_ARG, "fcu_picture_report: dev_org is null");
  if (!dev_rec) return fail(FCU_ERR_ARG, "fcu_picture_report: dev_rec is null");
  if (!dev_out) return fail(FCU_ERR_ARG, "fcu_picture_report: dev_out is null");
  if (!host_reports) return fail(FCU_ERR_ARG, "fcu_picture_report: host_reports is null");
  for (int i = 0; i < 3 * n_pics; i++) {
    if (!dev_org[i]) return fail(FCU_ERR_ARG, "fcu_picture_report: dev_org[" + std::to_string(i) + "] is null");
    if (!dev_rec[i]) return fail(FCU_ERR_ARG, "fcu_picture_report: dev_rec[" + std::to_string(i) + "] is null");
  }
  for (int i = 0; i < n_pics; i++) if (!dev_out[i]) return fail(FCU_ERR_ARG, "fcu_picture_report: dev_out[" + std::to_string(i) + "] is null");
  HIPCHK(hipSetDevice(c->hs.sp.device));
  hipStream_t st = (hipStream_t)hip_stream;
  const int w = c->hs.sp.width, h = c->hs.sp.height, w_ctu = c->hs.w_ctu, n_ctu = c->hs.n_ctu;
  const size_t o_pics = 0, o_rep = up(o_pics + sizeof(ReportPic) * n_pics), o_ctu = up(o_rep + sizeof(fcu_pic_report) * n_pics),
               total = dev_ctu ? o_ctu : up(o_ctu + sizeof(fcu_ctu_report) * (size_t)n_ctu * n_pics);
  HIPCHK(c->rep.reserve(total, st));
  uint8_t *base = (uint8_t *)c->rep.p;
  ReportPic *d_pics = (ReportPic *)(base + o_pics); fcu_pic_report *d_rep = (fcu_pic_report *)(base + o_rep);
  fcu_ctu_report *d_ctu = dev_ctu ? dev_ctu : (fcu_ctu_report *)(base + o_ctu);
  std::vector<ReportPic> hp((size_t)n_pics);
  for (int i = 0; i < n_pics; i++) {
    for (int k = 0; k < 3; k++) { hp[i].org[k] = dev_org[3 * i + k]; hp[i].rec[k] = dev_rec[3 * i + k]; }
    hp[i].out = dev_out[i];
  }
  const bool wide = report_wide_ok(w, hp.data(), n_pics);
  HIPCHK(hipMemcpyAsync(d_pics, hp.data(), sizeof(ReportPic) * n_pics, hipMemcpyHostToDevice, st));
  Events ev(st, kernel_ms2 != nullptr);
  HIPCHK(ev.create(3)); HIPCHK(ev.record(0));
  if (wide) hipLaunchKernelGGL(report_ctu<true>, dim3(n_ctu, n_pics), dim3(REP_THREADS), 0, st, d_pics, d_ctu, w, h, w_ctu, n_ctu);
  else hipLaunchKernelGGL(report_ctu<false>, dim3(n_ctu, n_pics), dim3(REP_THREADS), 0, st, d_pics, d_ctu, w, h, w_ctu, n_ctu);
  HIPCHK(hipGetLastError());
  HIPCHK(ev.record(1));
  hipLaunchKernelGGL(report_pic, dim3(n_pics), dim3(REP_THREADS), 0, st, d_ctu, d_rep, w, h, n_ctu);
  HIPCHK(hipGetLastError());
  HIPCHK(ev.record(2));
  HIPCHK(hipMemcpyAsync(host_reports, d_rep, sizeof(fcu_pic_report) * n_pics, hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));                          /* hp (the host descriptors) and host_reports are done with */
  if (kernel_ms2) { ev.ms(&kernel_ms2[0], 0, 1); ev.ms(&kernel_ms2[1], 1, 2); }
  for (int i = 0; i < n_pics; i++) for (int k = 0; k < 3; k++) host_reports[i].psnr[k] = report_psnr(host_reports[i].ssd[k], host_reports[i].n_samples[k]);
  return FCU_OK;
}

/* calcMD5 / calcCRC / calcChecksum of n_pics pictures: hash_chunk + hash_fold and / or hash_md5 (fcu_hash.h), the records back */
int fcu_picture_hash(fcu_ctx *c, int n_pics, int kinds, const uint8_t *const *dev_planes, fcu_pic_hash *host_hashes, float *kernel_ms3, void *hip_stream)
{
  if (!c) return fail(FCU_ERR_ARG, "fcu_picture_hash: null context");
  { std::string err; const int rc = hash_args_check(n_pics, kinds, dev_planes, host_hashes, err); if (rc != FCU_OK) return fail(rc, err); }
  HIPCHK(hipSetDevice(c->hs.sp.device));
  hipStream_t st = (hipStream_t)hip_stream;
  const uint32_t w[3] = { (uint32_t)c->hs.sp.width, (uint32_t)c->hs.sp.width / 2, (uint32_t)c->hs.sp.width / 2 },
                 h[3] = { (uint32_t)c->hs.sp.height, (uint32_t)c->hs.sp.height / 2, (uint32_t)c->hs.sp.height / 2 };
  const HashGeom G = hash_geom(3, w, h, kinds);
  const size_t o_planes = 0, o_hash = up(o_planes + sizeof(void *) * 3 * n_pics), o_part = up(o_hash + sizeof(fcu_pic_hash) * n_pics),
               total = up(o_part + sizeof(HashPartial) * (size_t)G.per_pic * n_pics);
  HIPCHK(c->hash.reserve(total, st));
  uint8_t *base = (uint8_t *)c->hash.p;
  const uint8_t **d_planes = (const uint8_t **)(base + o_planes); fcu_pic_hash *d_hash = (fcu_pic_hash *)(base + o_hash); HashPartial *d_part = (HashPartial *)(base + o_part);
  const bool wide = hash_wide_ok(dev_planes, 3 * n_pics), sums = (kinds & (FCU_HASH_CRC | FCU_HASH_CHECKSUM)) != 0, md5 = (kinds & FCU_HASH_MD5) != 0;
  HIPCHK(hipMemcpyAsync(d_planes, dev_planes, sizeof(void *) * 3 * n_pics, hipMemcpyHostToDevice, st));
  Events ev(st, kernel_ms3 != nullptr);
  HIPCHK(ev.create(4)); HIPCHK(ev.record(0));
  if (sums) {
    if (wide) hipLaunchKernelGGL(hash_chunk<16>, dim3(G.per_pic, n_pics), dim3(HASH_THREADS), 0, st, d_planes, d_part, G);
    else hipLaunchKernelGGL(hash_chunk<1>, dim3(G.per_pic, n_pics), dim3(HASH_THREADS), 0, st, d_planes, d_part, G);
    HIPCHK(hipGetLastError());
  }
  HIPCHK(ev.record(1));
  if (sums) { hipLaunchKernelGGL(hash_fold, dim3(3, n_pics), dim3(HASH_THREADS), 0, st, d_part, d_hash, G); HIPCHK(hipGetLastError()); }
  HIPCHK(ev.record(2));
  if (md5) {
    const int n_streams = 3 * n_pics; const dim3 grid((unsigned)((n_streams + HASH_MD5_THREADS - 1) / HASH_MD5_THREADS));
    if (wide) hipLaunchKernelGGL(hash_md5<16>, grid, dim3(HASH_MD5_THREADS), 0, st, d_planes, d_hash, G, n_streams);
    else hipLaunchKernelGGL(hash_md5<1>, grid, dim3(HASH_MD5_THREADS), 0, st, d_planes, d_hash, G, n_streams);
    HIPCHK(hipGetLastError());
  }
  HIPCHK(ev.record(3));
  HIPCHK(hipMemcpyAsync(host_hashes, d_hash, sizeof(fcu_pic_hash) * n_pics, hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));                          /* dev_planes (the caller's array) and host_hashes are done with */
  for (int i = 0; i < n_pics; i++) hash_clear_unasked(host_hashes[i], kinds);
  if (kernel_ms3) {
    kernel_ms3[0] = kernel_ms3[1] = kernel_ms3[2] = 0.f;
    if (sums) { ev.ms(&kernel_ms3[0], 0, 1); ev.ms(&kernel_ms3[1], 1, 2); }
    if (md5) ev.ms(&kernel_ms3[2], 2, 3);
  }
  return FCU_OK;
}

int fcu_hash_string(const fcu_pic_hash *h, int kind, char *buf, int buf_len)
{
  const int rc = hash_string(h, kind, buf, buf_len);
  return rc < 0 ? fail(rc, "fcu_hash_string: kind is exactly one of FCU_HASH_MD5 / FCU_HASH_CRC / FCU_HASH_CHECKSUM and the buffer holds the string (MD5: 99 bytes)") : rc;
}

/* the decision as rasters: maps_ctu (fcu_maps.h), one launch for the batch */
int fcu_decision_maps(fcu_ctx *c, int n_pics, const fcu_ctu_out *const *dev_out, int n_fields, const int *field_ids, uint8_t *dev_bytes, int16_t *dev_mv,
                      int8_t *dev_labels, const int16_t *const *dev_obf, uint16_t *dev_nobf, float *kernel_ms, void *hip_stream)
{
  if (!c) return fail(FCU_ERR_ARG, "fcu_decision_maps: null context");
  { std::string err; const int rc = maps_args_check(n_pics, dev_out, n_fields, field_ids, dev_bytes, dev_mv, dev_labels, dev_obf, dev_nobf, err); if (rc != FCU_OK) return fail(rc, err); }
  HIPCHK(hipSetDevice(c->hs.sp.device));
  hipStream_t st = (hipStream_t)hip_stream;
  const MapsGeom G = maps_geom(c->hs.sp.width, c->hs.sp.height, n_fields, field_ids);
  HIPCHK(c->maps.reserve(up(sizeof(MapsPic) * n_pics), st));
  MapsPic *d_pics = (MapsPic *)c->maps.p;
  std::vector<MapsPic> hp((size_t)n_pics);
  for (int i = 0; i < n_pics; i++) { hp[i].out = dev_out[i]; hp[i].obf = dev_obf ? dev_obf[i] : nullptr; }
  HIPCHK(hipMemcpyAsync(d_pics, hp.data(), sizeof(MapsPic) * n_pics, hipMemcpyHostToDevice, st));
  const MapsOut Q = { dev_bytes, dev_mv, dev_labels, dev_nobf };
  const int align = maps_row_align(G.width, dev_bytes, dev_mv);
  const dim3 grid(G.n_ctu, n_pics), block(MAPS_THREADS);
  Events ev(st, kernel_ms != nullptr);
  HIPCHK(ev.create(2)); HIPCHK(ev.record(0));
  if (align == 16) hipLaunchKernelGGL((maps_ctu<16, 16>), grid, block, 0, st, d_pics, Q, G);
  else if (align == 2) hipLaunchKernelGGL((maps_ctu<2, 2>), grid, block, 0, st, d_pics, Q, G);
  else hipLaunchKernelGGL((maps_ctu<2, 1>), grid, block, 0, st, d_pics, Q, G);
  HIPCHK(hipGetLastError());
  HIPCHK(ev.record(1));
  HIPCHK(hipStreamSynchronize(st));                          /* hp (the host descriptors) is done with */
  if (kernel_ms) ev.ms(kernel_ms, 0, 1);
  return FCU_OK;
}

/* label arrays from depth / part_size rasters: labels_ctu (fcu_maps.h), one launch for the batch */
int fcu_labels_from_rasters(fcu_ctx *c, int n_pics, const uint8_t *dev_depth, const int8_t *dev_part_size, int8_t *dev_labels, void *hip_stream)
{
  if (!c) return fail(FCU_ERR_ARG, "fcu_labels_from_rasters: null context");
  { std::string err; const int rc = labels_args_check(n_pics, dev_depth, dev_labels, err); if (rc != FCU_OK) return fail(rc, err); }
  HIPCHK(hipSetDevice(c->hs.sp.device));
  const MapsGeom G = maps_geom(c->hs.sp.width, c->hs.sp.height, 0, nullptr);
  hipLaunchKernelGGL(labels_ctu, dim3((unsigned)((G.n_ctu + LABELS_CTUS - 1) / LABELS_CTUS), (unsigned)n_pics), dim3(LABELS_THREADS), 0, (hipStream_t)hip_stream,
                     dev_depth, dev_part_size, dev_labels, G);
  HIPCHK(hipGetLastError());
  return FCU_OK;
}

/* the agreement of two decisions: match_ctu + match_pic (fcu_maps.h), the records back */
int fcu_split_match(fcu_ctx *c, int n_pics, const fcu_ctu_out *const *dev_out_a, const fcu_ctu_out *const *dev_out_b, fcu_pic_match *host_matches,
                    fcu_ctu_match *dev_ctu, float *kernel_ms2, void *hip_stream)
{
  if (!c) return fail(FCU_ERR_ARG, "fcu_split_match: null context");
  { std::string err; const int rc = match_args_check(n_pics, dev_out_a, dev_out_b, host_matches, err); if (rc != FCU_OK) return fail(rc, err); }
  HIPCHK(hipSetDevice(c->hs.sp.device));
  hipStream_t st = (hipStream_t)hip_stream;
  const MapsGeom G = maps_geom(c->hs.sp.width, c->hs.sp.height, 0, nullptr);
  const size_t o_pics = 0, o_rec = up(o_pics + sizeof(MatchPic) * n_pics), o_ctu = up(o_rec + sizeof(fcu_pic_match) * n_pics),
               total = dev_ctu ? o_ctu : up(o_ctu + sizeof(fcu_ctu_match) * (size_t)G.n_ctu * n_pics);
  HIPCHK(c->maps.reserve(total, st));
  uint8_t *base = (uint8_t *)c->maps.p;
  MatchPic *d_pics = (MatchPic *)(base + o_pics); fcu_pic_match *d_rec = (fcu_pic_match *)(base + o_rec);
  fcu_ctu_match *d_ctu = dev_ctu ? dev_ctu : (fcu_ctu_match *)(base + o_ctu);
  std::vector<MatchPic> hp((size_t)n_pics);
  for (int i = 0; i < n_pics; i++) { hp[i].a = dev_out_a[i]; hp[i].b = dev_out_b[i]; }
  HIPCHK(hipMemcpyAsync(d_pics, hp.data(), sizeof(MatchPic) * n_pics, hipMemcpyHostToDevice, st));
  Events ev(st, kernel_ms2 != nullptr);
  HIPCHK(ev.create(3)); HIPCHK(ev.record(0));
  hipLaunchKernelGGL(match_ctu, dim3(G.n_ctu, n_pics), dim3(MAPS_THREADS), 0, st, d_pics, d_ctu, G);
  HIPCHK(hipGetLastError());
  HIPCHK(ev.record(1));
  hipLaunchKernelGGL(match_pic, dim3(n_pics), dim3(MAPS_THREADS), 0, st, d_ctu, d_rec, G.n_ctu);
  HIPCHK(hipGetLastError());
  HIPCHK(ev.record(2));
  HIPCHK(hipMemcpyAsync(host_matches, d_rec, sizeof(fcu_pic_match) * n_pics, hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));                          /* hp (the host descriptors) and host_matches are done with */
  if (kernel_ms2) { ev.ms(&kernel_ms2[0], 0, 1); ev.ms(&kernel_ms2[1], 1, 2); }
  return FCU_OK;
}

/* the Verifying counters of label arrays against CU traces: score_ctu + score_pic (fcu_trace.h), the records back */
int fcu_label_score(fcu_ctx *c, int n_pics, const fcu_cu_trace *const *dev_trace, const int8_t *const *dev_labels, fcu_pic_score *host_scores,
                    fcu_ctu_score *dev_ctu, float *kernel_ms2, void *hip_stream)
{
  if (!c) return fail(FCU_ERR_ARG, "fcu_label_score: null context");
  { std::string err; const int rc = score_args_check(n_pics, dev_trace, dev_labels, host_scores, err); if (rc != FCU_OK) return fail(rc, err); }
  HIPCHK(hipSetDevice(c->hs.sp.device));
  hipStream_t st = (hipStream_t)hip_stream;
  const MapsGeom G = maps_geom(c->hs.sp.width, c->hs.sp.height, 0, nullptr);
  const size_t o_pics = 0, o_rec = up(o_pics + sizeof(ScorePic) * n_pics), o_ctu = up(o_rec + sizeof(fcu_pic_score) * n_pics),
               total = dev_ctu ? o_ctu : up(o_ctu + sizeof(fcu_ctu_score) * (size_t)G.n_ctu * n_pics);
  HIPCHK(c->score.reserve(total, st));
  uint8_t *base = (uint8_t *)c->score.p;
  ScorePic *d_pics = (ScorePic *)(base + o_pics); fcu_pic_score *d_rec = (fcu_pic_score *)(base + o_rec);
  fcu_ctu_score *d_ctu = dev_ctu ? dev_ctu : (fcu_ctu_score *)(base + o_ctu);
  std::vector<ScorePic> hp((size_t)n_pics);
  for (int i = 0; i < n_pics; i++) { hp[i].trace = dev_trace[i]; hp[i].labels = dev_labels[i]; }
  HIPCHK(hipMemcpyAsync(d_pics, hp.data(), sizeof(ScorePic) * n_pics, hipMemcpyHostToDevice, st));
  Events ev(st, kernel_ms2 != nullptr);
  HIPCHK(ev.create(3)); HIPCHK(ev.record(0));
  hipLaunchKernelGGL(score_ctu, dim3((unsigned)((G.n_ctu + SCORE_CTUS - 1) / SCORE_CTUS), (unsigned)n_pics), dim3(SCORE_THREADS), 0, st, d_pics, d_ctu, G);
  HIPCHK(hipGetLastError());
  HIPCHK(ev.record(1));
  hipLaunchKernelGGL(score_pic, dim3((unsigned)n_pics), dim3(SCORE_PIC_THREADS), 0, st, d_ctu, d_rec, G.n_ctu);
  HIPCHK(hipGetLastError());
  HIPCHK(ev.record(2));
  HIPCHK(hipMemcpyAsync(host_scores, d_rec, sizeof(fcu_pic_score) * n_pics, hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));                          /* hp (the host descriptors) and host_scores are done with */
  if (kernel_ms2) { ev.ms(&kernel_ms2[0], 0, 1); ev.ms(&kernel_ms2[1], 1, 2); }
  return FCU_OK;
}

/* CU traces as label / J0 / J1 maps: trace_ctu (fcu_trace.h), one launch for the batch */
int fcu_trace_maps(fcu_ctx *c, int n_pics, const fcu_cu_trace *const *dev_trace, int8_t *dev_labels, double *dev_j0, double *dev_j1, float *kernel_ms, void *hip_stream)
{
  if (!c) return fail(FCU_ERR_ARG, "fcu_trace_maps: null context");
  { std::string err; const int rc = trace_maps_args_check(n_pics, dev_trace, dev_labels, dev_j0, dev_j1, err); if (rc != FCU_OK) return fail(rc, err); }
  HIPCHK(hipSetDevice(c->hs.sp.device));
  hipStream_t st = (hipStream_t)hip_stream;
  const MapsGeom G = maps_geom(c->hs.sp.width, c->hs.sp.height, 0, nullptr);
  HIPCHK(c->score.reserve(up(sizeof(void *) * n_pics), st));
  const fcu_cu_trace **d_tr = (const fcu_cu_trace **)c->score.p;
  HIPCHK(hipMemcpyAsync(d_tr, dev_trace, sizeof(void *) * n_pics, hipMemcpyHostToDevice, st));
  const TraceOut Q = { dev_labels, dev_j0, dev_j1 };
  Events ev(st, kernel_ms != nullptr);
  HIPCHK(ev.create(2)); HIPCHK(ev.record(0));
  hipLaunchKernelGGL(trace_ctu, dim3((unsigned)((G.n_ctu + SCORE_CTUS - 1) / SCORE_CTUS), (unsigned)n_pics), dim3(SCORE_THREADS), 0, st, d_tr, Q, G);
  HIPCHK(hipGetLastError());
  HIPCHK(ev.record(1));
  HIPCHK(hipStreamSynchronize(st));                          /* dev_trace (the caller's array) is done with */
  if (kernel_ms) ev.ms(kernel_ms, 0, 1);
  return FCU_OK;
}

/* the fork's TMV / SOC features per block of the label maps: feat_ctu (fcu_features.h), one launch for the batch */
int fcu_feature_count(int sets)
{
  const int f = feature_count(sets);
  return f < 0 ? fail(FCU_ERR_ARG, "fcu_feature_count: sets is a non-empty mask of FCU_FEATSET_TMV | FCU_FEATSET_SOC") : f;
}
int fcu_feature_maps(fcu_ctx *c, int n_pics, int sets, const uint8_t *const *dev_y, const double *host_yc, float *dev_features, float *kernel_ms, void *hip_stream)
{
  if (!c) return fail(FCU_ERR_ARG, "fcu_feature_maps: null context");
  { std::string err; const int rc = features_args_check(n_pics, sets, dev_y, host_yc, dev_features, err); if (rc != FCU_OK) return fail(rc, err); }
  HIPCHK(hipSetDevice(c->hs.sp.device));
  hipStream_t st = (hipStream_t)hip_stream;
  const MapsGeom G = maps_geom(c->hs.sp.width, c->hs.sp.height, 0, nullptr);
  HIPCHK(c->maps.reserve(up(sizeof(FeatPic) * n_pics), st));
  FeatPic *d_pics = (FeatPic *)c->maps.p;
  std::vector<FeatPic> hp((size_t)n_pics);
  for (int i = 0; i < n_pics; i++) {
    hp[i].y = dev_y[i];
    for (int k = 0; k < 16; k++) hp[i].thr[k] = host_yc ? obf_thr(host_yc[(size_t)i * 16 + k]) : 0;
  }
  HIPCHK(hipMemcpyAsync(d_pics, hp.data(), sizeof(FeatPic) * n_pics, hipMemcpyHostToDevice, st));
  const dim3 grid(G.n_ctu, n_pics), block(FEAT_THREADS);
  Events ev(st, kernel_ms != nullptr);
  HIPCHK(ev.create(2)); HIPCHK(ev.record(0));
  if (sets == FCU_FEATSET_TMV) hipLaunchKernelGGL((feat_ctu<FCU_FEATSET_TMV>), grid, block, 0, st, d_pics, dev_features, G);
  else if (sets == FCU_FEATSET_SOC) hipLaunchKernelGGL((feat_ctu<FCU_FEATSET_SOC>), grid, block, 0, st, d_pics, dev_features, G);
  else hipLaunchKernelGGL((feat_ctu<FCU_FEATSET_TMV | FCU_FEATSET_SOC>), grid, block, 0, st, d_pics, dev_features, G);
  HIPCHK(hipGetLastError());
  HIPCHK(ev.record(1));
  HIPCHK(hipStreamSynchronize(st));                          /* hp (the host descriptors) is done with */
  if (kernel_ms) ev.ms(kernel_ms, 0, 1);
  return FCU_OK;
}

/* the risk-table model: risk_train + risk_add, risk_predict, nobf_blocks (fcu_risk.h) */
int fcu_risk_train(fcu_ctx *c, int n_pics, const fcu_cu_trace *const *dev_trace, const uint16_t *const *dev_keys, fcu_risk_model *dev_model, int accumulate,
                   uint32_t *host_dropped, float *kernel_ms2, void *hip_stream)
{
  if (!c) return fail(FCU_ERR_ARG, "fcu_risk_train: null context");
  { std::string err; const int rc = risk_train_args_check(n_pics, dev_trace, dev_keys, dev_model, accumulate, c->hs.label_count(), err); if (rc != FCU_OK) return fail(rc, err); }
  HIPCHK(hipSetDevice(c->hs.sp.device));
  hipStream_t st = (hipStream_t)hip_stream;
  const MapsGeom G = maps_geom(c->hs.sp.width, c->hs.sp.height, 0, nullptr);
  const int n_units = G.n_ctu * n_pics, n_groups = risk_train_groups(n_units);
  const size_t o_tr = 0, o_key = up(o_tr + sizeof(void *) * n_pics), o_drop = up(o_key + sizeof(void *) * n_pics), o_slots = up(o_drop + sizeof(uint32_t)),
               total = o_slots + sizeof(RiskSlot) * (size_t)n_groups;
  HIPCHK(c->risk.reserve(total, st));
  uint8_t *base = (uint8_t *)c->risk.p;
  const fcu_cu_trace **d_tr = (const fcu_cu_trace **)(base + o_tr); const uint16_t **d_key = (const uint16_t **)(base + o_key);
  uint32_t *d_drop = (uint32_t *)(base + o_drop); RiskSlot *d_slots = (RiskSlot *)(base + o_slots);
  HIPCHK(hipMemcpyAsync(d_tr, dev_trace, sizeof(void *) * n_pics, hipMemcpyHostToDevice, st));
  HIPCHK(hipMemcpyAsync(d_key, dev_keys, sizeof(void *) * n_pics, hipMemcpyHostToDevice, st));
  Events ev(st, kernel_ms2 != nullptr);
  HIPCHK(ev.create(3)); HIPCHK(ev.record(0));
  hipLaunchKernelGGL(risk_train, dim3((unsigned)n_groups), dim3(RISK_THREADS), 0, st, d_tr, d_key, d_slots, G, n_units, n_groups);
  HIPCHK(hipGetLastError());
  HIPCHK(ev.record(1));
  hipLaunchKernelGGL(risk_add, dim3(RISK_ADD_GROUPS), dim3(RISK_ADD_THREADS), 0, st, d_slots, n_groups, dev_model, d_drop, accumulate);
  HIPCHK(hipGetLastError());
  HIPCHK(ev.record(2));
  uint32_t dropped = 0;
  HIPCHK(hipMemcpyAsync(&dropped, d_drop, sizeof(dropped), hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));                          /* dev_trace, dev_keys (the caller's arrays) and `dropped` are done with */
  if (host_dropped) *host_dropped = dropped;
  if (kernel_ms2) { ev.ms(&kernel_ms2[0], 0, 1); ev.ms(&kernel_ms2[1], 1, 2); }
  return FCU_OK;
}

int fcu_risk_predict(fcu_ctx *c, int n_pics, const uint16_t *const *dev_keys, const fcu_risk_model *dev_model, int min_count, int8_t *dev_labels, float *kernel_ms, void *hip_stream)
{
  if (!c) return fail(FCU_ERR_ARG, "fcu_risk_predict: null context");
  { std::string err; const int rc = risk_predict_args_check(n_pics, dev_keys, dev_model, min_count, dev_labels, err); if (rc != FCU_OK) return fail(rc, err); }
  HIPCHK(hipSetDevice(c->hs.sp.device));
  hipStream_t st = (hipStream_t)hip_stream;
  const MapsGeom G = maps_geom(c->hs.sp.width, c->hs.sp.height, 0, nullptr);
  const RiskPlan P = risk_plan(G);
  HIPCHK(c->risk.reserve(up(sizeof(void *) * n_pics), st));
  const uint16_t **d_key = (const uint16_t **)c->risk.p;
  HIPCHK(hipMemcpyAsync(d_key, dev_keys, sizeof(void *) * n_pics, hipMemcpyHostToDevice, st));
  Events ev(st, kernel_ms != nullptr);
  HIPCHK(ev.create(2)); HIPCHK(ev.record(0));
  hipLaunchKernelGGL(risk_predict, dim3((unsigned)P.wg_off[4], (unsigned)n_pics), dim3(RISK_PRED_THREADS), 0, st, d_key, dev_model, min_count, dev_labels, G, P);
  HIPCHK(hipGetLastError());
  HIPCHK(ev.record(1));
  HIPCHK(hipStreamSynchronize(st));                          /* dev_keys (the caller's array) is done with */
  if (kernel_ms) ev.ms(kernel_ms, 0, 1);
  return FCU_OK;
}

int fcu_nobf_maps(fcu_ctx *c, int n_pics, const int16_t *const *dev_obf, uint16_t *dev_nobf, void *hip_stream)
{
  if (!c) return fail(FCU_ERR_ARG, "fcu_nobf_maps: null context");
  { std::string err; const int rc = nobf_args_check(n_pics, dev_obf, dev_nobf, err); if (rc != FCU_OK) return fail(rc, err); }
  HIPCHK(hipSetDevice(c->hs.sp.device));
  hipStream_t st = (hipStream_t)hip_stream;
  const MapsGeom G = maps_geom(c->hs.sp.width, c->hs.sp.height, 0, nullptr);
  const RiskPlan P = risk_plan(G);
  HIPCHK(c->risk.reserve(up(sizeof(void *) * n_pics), st));
  const int16_t **d_obf = (const int16_t **)c->risk.p;
  HIPCHK(hipMemcpyAsync(d_obf, dev_obf, sizeof(void *) * n_pics, hipMemcpyHostToDevice, st));
  hipLaunchKernelGGL(nobf_blocks, dim3((unsigned)P.wg_off[4], (unsigned)n_pics), dim3(RISK_PRED_THREADS), 0, st, d_obf, dev_nobf, G, P);
  HIPCHK(hipGetLastError());
  HIPCHK(hipStreamSynchronize(st));                          /* dev_obf (the caller's array) is done with */
  return FCU_OK;
}

void fcu_risk_table(const fcu_risk_model *host_model, int min_count, int8_t table[4][FCU_RISK_BINS]) { risk_table(host_model, min_count, table); }

/* the key tree: feat_bins, tree_keys, tree_hist + tree_fold (fcu_tree.h); the split choice is host arithmetic (fcu_host.h) */
int fcu_feature_edges_check(const float *host_edges, int sets)
{
  std::string err;
  const int rc = tree_edges_check(host_edges, sets, err);
  return rc == FCU_OK ? FCU_OK : fail(rc, err);
}
int fcu_tree_split(const int64_t *host_risk, const uint32_t *host_count, int F, int level, int min_count, fcu_key_tree *tree)
{
  std::string err;
  const int rc = tree_split(host_risk, host_count, F, level, min_count, tree, err);
  return rc == FCU_OK ? FCU_OK : fail(rc, err);
}

int fcu_feature_bins(fcu_ctx *c, int n_pics, int sets, const float *dev_features, const float *dev_edges, uint8_t *dev_bins, float *kernel_ms, void *hip_stream)
{
  if (!c) return fail(FCU_ERR_ARG, "fcu_feature_bins: null context");
  { std::string err; const int rc = feature_bins_args_check(n_pics, sets, dev_features, dev_edges, dev_bins, c->hs.label_count(), err); if (rc != FCU_OK) return fail(rc, err); }
  HIPCHK(hipSetDevice(c->hs.sp.device));
  hipStream_t st = (hipStream_t)hip_stream;
  const MapsGeom G = maps_geom(c->hs.sp.width, c->hs.sp.height, 0, nullptr);
  const TreePlan P = tree_plan(G, TREE_BIN_ROWS);
  Events ev(st, kernel_ms != nullptr);
  HIPCHK(ev.create(2)); HIPCHK(ev.record(0));
  hipLaunchKernelGGL(feat_bins, dim3((unsigned)P.wg_off[4], (unsigned)n_pics), dim3(TREE_THREADS), 0, st, dev_features, dev_edges, dev_bins, G, P, feature_count(sets));
  HIPCHK(hipGetLastError());
  HIPCHK(ev.record(1));
  HIPCHK(hipStreamSynchronize(st));
  if (kernel_ms) ev.ms(kernel_ms, 0, 1);
  return FCU_OK;
}

/* where the sub-blocks of fcu_ctx::tree lie for a call on n_pics pictures whose deepest histogram level is max_level (-1: none);
 * train: also the node indices and a level's histograms */
struct TreeBufs { size_t tr, bins, nodes, tree, drop, slots, keys, risk, count, total; };
static TreeBufs tree_bufs(const MapsGeom &G, int n_pics, int F, int max_level, bool train)
{
  TreeBufs B = {};
  size_t o = 0;
  auto take = [&o](size_t bytes) { const size_t at = o; o = up(o + bytes); return at; };
  B.tr = take(sizeof(void *) * n_pics); B.bins = take(sizeof(void *) * n_pics); B.nodes = take(sizeof(void *) * n_pics);
  B.tree = take(sizeof(fcu_key_tree)); B.drop = take(sizeof(uint32_t));
  B.slots = take(max_level < 0 ? 0 : sizeof(TreeSlot) * (size_t)tree_hist_groups(tree_hist_plan(G, n_pics, F, max_level)));
  B.keys = take(train ? sizeof(uint16_t) * (size_t)n_pics * (size_t)G.lvl_off[4] : 0);
  B.risk = take(train && max_level >= 0 ? sizeof(int64_t) * (size_t)tree_hist_cells(F, max_level) : 0);
  B.count = take(train && max_level >= 0 ? sizeof(uint32_t) * (size_t)tree_hist_cells(F, max_level) : 0);
  B.total = o;
  return B;
}
/* tree_keys for `levels` steps of *host_tree on the device array d_bins of picture pointers (queued; host_tree is copied before
 * the return of the caller's synchronisation) */
static int tree_keys_launch(fcu_ctx *c, hipStream_t st, const MapsGeom &G, int n_pics, int F, const TreeBufs &B, const fcu_key_tree *host_tree, int levels, uint16_t *dev_keys)
{
  uint8_t *base = (uint8_t *)c->tree.p;
  HIPCHK(hipMemcpyAsync(base + B.tree, host_tree, sizeof(fcu_key_tree), hipMemcpyHostToDevice, st));
  const TreePlan P = tree_plan(G, TREE_THREADS);
  hipLaunchKernelGGL(tree_keys, dim3((unsigned)P.wg_off[4], (unsigned)n_pics), dim3(TREE_THREADS), 0, st, (const uint8_t *const *)(base + B.bins), (const fcu_key_tree *)(base + B.tree), levels, dev_keys, G, P, F);
  HIPCHK(hipGetLastError());
  return FCU_OK;
}
/* tree_hist + tree_fold of `level` on the device arrays of picture pointers (queued) */
static int tree_hist_launch(fcu_ctx *c, hipStream_t st, const MapsGeom &G, int n_pics, int F, const TreeBufs &B, int level, bool with_nodes, int64_t *dev_risk, uint32_t *dev_count, int accumulate, Events *ev)
{
  uint8_t *base = (uint8_t *)c->tree.p;
  const TreeHistPlan P = tree_hist_plan(G, n_pics, F, level);
  TreeSlot *d_slots = (TreeSlot *)(base + B.slots);
  hipLaunchKernelGGL(tree_hist, dim3((unsigned)tree_hist_groups(P)), dim3(TREE_THREADS), 0, st, (const fcu_cu_trace *const *)(base + B.tr), (const uint8_t *const *)(base + B.bins),
                     with_nodes ? (const uint16_t *const *)(base + B.nodes) : nullptr, d_slots, G, P);
  HIPCHK(hipGetLastError());
  if (ev) HIPCHK(ev->record(1));
  hipLaunchKernelGGL(tree_fold, dim3((unsigned)((tree_hist_cells(F, level) + 1 + TREE_FOLD_THREADS - 1) / TREE_FOLD_THREADS)), dim3(TREE_FOLD_THREADS), 0, st, d_slots, P, dev_risk, dev_count,
                     (uint32_t *)(base + B.drop), accumulate);
  HIPCHK(hipGetLastError());
  return FCU_OK;
}

int fcu_tree_keys(fcu_ctx *c, int n_pics, int sets, const uint8_t *dev_bins, const fcu_key_tree *host_tree, int levels, uint16_t *dev_keys, float *kernel_ms, void *hip_stream)
{
  if (!c) return fail(FCU_ERR_ARG, "fcu_tree_keys: null context");
  { std::string err; const int rc = tree_keys_args_check(n_pics, sets, dev_bins, host_tree, levels, dev_keys, c->hs.label_count(), err); if (rc != FCU_OK) return fail(rc, err); }
  HIPCHK(hipSetDevice(c->hs.sp.device));
  hipStream_t st = (hipStream_t)hip_stream;
  const MapsGeom G = maps_geom(c->hs.sp.width, c->hs.sp.height, 0, nullptr);
  const int F = feature_count(sets);
  const TreeBufs B = tree_bufs(G, n_pics, F, -1, false);
  HIPCHK(c->tree.reserve(B.total, st));
  std::vector<const uint8_t *> hp((size_t)n_pics);
  for (int i = 0; i < n_pics; i++) hp[i] = dev_bins + (size_t)i * (size_t)G.lvl_off[4] * (size_t)F;
  HIPCHK(hipMemcpyAsync((uint8_t *)c->tree.p + B.bins, hp.data(), sizeof(void *) * n_pics, hipMemcpyHostToDevice, st));
  Events ev(st, kernel_ms != nullptr);
  HIPCHK(ev.create(2)); HIPCHK(ev.record(0));
  CHK(tree_keys_launch(c, st, G, n_pics, F, B, host_tree, levels, dev_keys));
  HIPCHK(ev.record(1));
  HIPCHK(hipStreamSynchronize(st));                          /* hp and host_tree are done with */
  if (kernel_ms) ev.ms(kernel_ms, 0, 1);
  return FCU_OK;
}

int fcu_tree_hist(fcu_ctx *c, int n_pics, int sets, int level, const fcu_cu_trace *const *dev_trace, const uint8_t *const *dev_bins, const uint16_t *const *dev_nodes,
                  int64_t *dev_risk, uint32_t *dev_count, int accumulate, uint32_t *host_dropped, float *kernel_ms2, void *hip_stream)
{
  if (!c) return fail(FCU_ERR_ARG, "fcu_tree_hist: null context");
  { std::string err; const int rc = tree_hist_args_check(n_pics, sets, level, dev_trace, dev_bins, dev_nodes, dev_risk, dev_count, accumulate, c->hs.label_count(), err); if (rc != FCU_OK) return fail(rc, err); }
  HIPCHK(hipSetDevice(c->hs.sp.device));
  hipStream_t st = (hipStream_t)hip_stream;
  const MapsGeom G = maps_geom(c->hs.sp.width, c->hs.sp.height, 0, nullptr);
  const int F = feature_count(sets);
  const TreeBufs B = tree_bufs(G, n_pics, F, level, false);
  HIPCHK(c->tree.reserve(B.total, st));
  uint8_t *base = (uint8_t *)c->tree.p;
  HIPCHK(hipMemcpyAsync(base + B.tr, dev_trace, sizeof(void *) * n_pics, hipMemcpyHostToDevice, st));
  HIPCHK(hipMemcpyAsync(base + B.bins, dev_bins, sizeof(void *) * n_pics, hipMemcpyHostToDevice, st));
  if (dev_nodes) HIPCHK(hipMemcpyAsync(base + B.nodes, dev_nodes, sizeof(void *) * n_pics, hipMemcpyHostToDevice, st));
  Events ev(st, kernel_ms2 != nullptr);
  HIPCHK(ev.create(3)); HIPCHK(ev.record(0));
  CHK(tree_hist_launch(c, st, G, n_pics, F, B, level, dev_nodes != nullptr, dev_risk, dev_count, accumulate, &ev));
  HIPCHK(ev.record(2));
  uint32_t dropped = 0;
  HIPCHK(hipMemcpyAsync(&dropped, base + B.drop, sizeof(dropped), hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));                          /* the caller's arrays and `dropped` are done with */
  if (host_dropped) *host_dropped = dropped;
  if (kernel_ms2) { ev.ms(&kernel_ms2[0], 0, 1); ev.ms(&kernel_ms2[1], 1, 2); }
  return FCU_OK;
}

int fcu_tree_train(fcu_ctx *c, int n_pics, int sets, int levels, int min_count, const fcu_cu_trace *const *dev_trace, const uint8_t *const *dev_bins, fcu_key_tree *host_tree,
                   float *kernel_ms, void *hip_stream)
{
  if (!c) return fail(FCU_ERR_ARG, "fcu_tree_train: null context");
  { std::string err; const int rc = tree_train_args_check(n_pics, sets, levels, min_count, dev_trace, dev_bins, host_tree, c->hs.label_count(), err); if (rc != FCU_OK) return fail(rc, err); }
  HIPCHK(hipSetDevice(c->hs.sp.device));
  hipStream_t st = (hipStream_t)hip_stream;
  const MapsGeom G = maps_geom(c->hs.sp.width, c->hs.sp.height, 0, nullptr);
  const int F = feature_count(sets);
  const TreeBufs B = tree_bufs(G, n_pics, F, levels - 1, true);
  HIPCHK(c->tree.reserve(B.total, st));
  uint8_t *base = (uint8_t *)c->tree.p;
  uint16_t *d_keys = (uint16_t *)(base + B.keys);
  std::vector<const uint16_t *> nodes((size_t)n_pics);
  for (int i = 0; i < n_pics; i++) nodes[i] = d_keys + (size_t)i * (size_t)G.lvl_off[4];
  HIPCHK(hipMemcpyAsync(base + B.tr, dev_trace, sizeof(void *) * n_pics, hipMemcpyHostToDevice, st));
  HIPCHK(hipMemcpyAsync(base + B.bins, dev_bins, sizeof(void *) * n_pics, hipMemcpyHostToDevice, st));
  HIPCHK(hipMemcpyAsync(base + B.nodes, nodes.data(), sizeof(void *) * n_pics, hipMemcpyHostToDevice, st));
  tree_clear(*host_tree, levels);
  std::vector<int64_t> h_risk; std::vector<uint32_t> h_count;
  Events ev(st, kernel_ms != nullptr);
  HIPCHK(ev.create(2));
  float total = 0.f;
  for (int l = 0; l < levels; l++) {
    const size_t cells = (size_t)tree_hist_cells(F, l);
    h_risk.resize(cells); h_count.resize(cells);
    HIPCHK(ev.record(0));
    if (l > 0) CHK(tree_keys_launch(c, st, G, n_pics, F, B, host_tree, l, d_keys));
    CHK(tree_hist_launch(c, st, G, n_pics, F, B, l, l > 0, (int64_t *)(base + B.risk), (uint32_t *)(base + B.count), 0, nullptr));
    HIPCHK(ev.record(1));
    HIPCHK(hipMemcpyAsync(h_risk.data(), base + B.risk, sizeof(int64_t) * cells, hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(h_count.data(), base + B.count, sizeof(uint32_t) * cells, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    if (kernel_ms) { float ms = 0.f; ev.ms(&ms, 0, 1); total += ms; }
    std::string err;
    const int rc = tree_split(h_risk.data(), h_count.data(), F, l, min_count, host_tree, err);
    if (rc != FCU_OK) return fail(rc, err);
  }
  HIPCHK(hipStreamSynchronize(st));                          /* (levels 0: the pointer arrays are done with) */
  if (kernel_ms) *kernel_ms = total;
  return FCU_OK;
}

} /* extern "C" */
