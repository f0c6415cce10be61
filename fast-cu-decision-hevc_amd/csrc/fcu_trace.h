/*
 * fcu_trace.h -- what is made of a CU trace (fcu_chain_set_cu_trace: J0, J1 and the outcome of every CU the search visited) on the
 * device: the Verifying counters of any label array (fcu_label_score) and the fork's whole Training set as maps (fcu_trace_maps).
 * Records, label codes and the sum order: include/fcu.h.  Included by fcu_kernels.hip only (and by the test-only CPU build
 * tests/emu/cu_trace_emu.cpp).
 *
 *   score_ctu    one wave per (CTU, picture), four CTUs per 256-thread workgroup.  Lane l owns node 21 + l of the CTU's quadtree
 *                (the 64 CUs of depth 3) and, l < 21, node l (depths 0..2) as well: the numbering of fcu_cu_index.  A node loads its
 *                24-byte record as three 8-byte words, all loads of a lane before the first use, and -- when the record is a sample
 *                (valid and split_tried) -- the one label byte of its block (maps_place: picture coordinates).  Every counter is
 *                one wave ballot + popcount.  The losses go through LDS: every node leaves |J0 - J1| and which sum it belongs to
 *                (none / FPLoss / FNLoss), and after a barrier lane 16 + 2 d + k walks the nodes of depth d in z-order and adds
 *                the terms of sum k one after the other from 0.0 -- at most 64 dependent additions, the order the engine's own
 *                Verifying counters take inside a CTU.  Lanes 0..15 store one dword of the record's integer half each.
 *   score_pic    one 64-thread workgroup per picture; lane (d, k) < 32 walks the picture's CTU records in raster order and adds
 *                its counter from 0.0 (the six of fcu_verify_counts as doubles, then open and scored as integers), SCORE_AHEAD
 *                loads in flight.  The additions of a lane are dependent on purpose: the order is the interface.
 *   trace_ctu    fcu_trace_maps: one wave per (CTU, picture), nodes dealt as in score_ctu; a node whose block starts inside the
 *                picture stores its label byte and its two costs at the block's element of the label-map layout.
 * No atomics; every output byte is written by exactly one thread; nothing must be cleared beforehand: a repeated call gives
 * identical bytes.  Algorithmic bytes per picture: score 85 x 24 B + up to 85 label bytes read and 128 B written per CTU, then
 * 128 B per CTU read again; maps 85 x 24 B read and up to 85 x 17 B written per CTU.
 */
#pragma once
#include "fcu_maps.h"

namespace fcu {

enum { SCORE_THREADS = 256, SCORE_CTUS = SCORE_THREADS / 64, SCORE_SLOTS = 20, SCORE_PIC_THREADS = 64, SCORE_PIC_LANES = 32, SCORE_AHEAD = 8,
       SCORE_NONE = 0, SCORE_FP = 1, SCORE_FN = 2 };
static_assert(sizeof(fcu_cu_trace) == 24 && sizeof(fcu_ctu_score) == 128 && sizeof(fcu_pic_score) == 224 && offsetof(fcu_ctu_score, loss) == 64
              && offsetof(fcu_pic_score, open) == 192 && FCU_CUS_PER_CTU == MAPS_NODES, "record layouts the word-wise accesses rely on");

struct ScorePic { const fcu_cu_trace *trace; const int8_t *labels; };      /* one picture of a batch (device copy) */
struct TraceOut { int8_t *labels; double *j0, *j1; };

/* the workgroup's LDS: per wave (= CTU) the counters n[4][4], open[4] and what every node adds to the loss sums */
struct ScoreLds { uint32_t cnt[SCORE_CTUS][SCORE_SLOTS]; double loss[SCORE_CTUS][MAPS_NODES]; uint8_t kind[SCORE_CTUS][MAPS_NODES + 3]; };

/* one record as a lane holds it */
struct TraceRec { double j0, j1; uint32_t valid, split_won, whole_tried, split_tried; };
__device__ static inline TraceRec trace_load(const fcu_cu_trace *p)
{
  const FCU_HBM uint64_t *q = (const FCU_HBM uint64_t *)p;
  const uint64_t a = q[0], b = q[1], f = q[2];
  TraceRec R;
  __builtin_memcpy(&R.j0, &a, 8); __builtin_memcpy(&R.j1, &b, 8);
  R.valid = (uint32_t)(f & 255u); R.split_won = (uint32_t)((f >> 8) & 255u); R.whole_tried = (uint32_t)((f >> 16) & 255u); R.split_tried = (uint32_t)((f >> 24) & 255u);
  return R;
}
/* (the CPU build runs the lanes one after the other into a word its driver cleared) */
__device__ static inline void score_wave_count(uint32_t *slot, bool flag)
{
#ifdef FCU_EMU
  *slot += flag ? 1u : 0u;
#else
  const uint32_t n = (uint32_t)__popcll(__ballot(flag));
  if ((threadIdx.x & 63) == 0) *slot = n;
#endif
}

/* ---- score_ctu: phase 1 counts and leaves the loss terms, phase 2 stores the record */
template <int PHASE>
__device__ static inline void score_ctu_phase(ScoreLds &L, const ScorePic *pics, fcu_ctu_score *ctu, const MapsGeom &G)
{
  const int l = (int)threadIdx.x & 63, wv = (int)threadIdx.x >> 6, a = (int)blockIdx.x * SCORE_CTUS + wv, pic = (int)blockIdx.y;
  if (a >= G.n_ctu) return;                                  /* (a whole wave) */
  if (PHASE == 1) {
    const int cx = a % G.w_ctu, cy = a / G.w_ctu;
    const ScorePic &P = pics[pic];
    const fcu_cu_trace *rec = P.trace + (size_t)a * FCU_CUS_PER_CTU;
    const FCU_HBM int8_t *lab = (const FCU_HBM int8_t *)P.labels;
    /* node 0: depth 3 (every lane), node 1: depths 0..2 (lanes 0..20) */
    const int t[2] = { 21 + l, l < 21 ? l : 0 };
    const bool own[2] = { true, l < 21 };
    MapsNode N[2] = { maps_node(t[0]), maps_node(t[1]) };
    MapsPlace C[2] = { maps_place(G, N[0], cx, cy), maps_place(G, N[1], cx, cy) };
    TraceRec R[2];
#pragma unroll
    for (int k = 0; k < 2; k++) R[k] = trace_load(rec + t[k]);
    bool sample[2]; int v[2] = { 0, 0 };
#pragma unroll
    for (int k = 0; k < 2; k++) {                            /* a block that is not wholly inside the picture has no label to read */
      sample[k] = own[k] && C[k].whole && R[k].valid != 0 && R[k].split_tried != 0;
      if (sample[k]) v[k] = lab[C[k].idx];
    }
    int cls[2];                                              /* 0..3 = TP, FP, TN, FN; 4 = open; -1 = no sample */
#pragma unroll
    for (int k = 0; k < 2; k++) {
      const bool truth = R[k].split_won != 0;
      cls[k] = !sample[k] ? -1 : (v[k] == FCU_LABEL_SPLIT ? (truth ? 0 : 1) : (v[k] == FCU_LABEL_NOT_SPLIT ? (truth ? 3 : 2) : 4));
      if (own[k]) {
        L.loss[wv][t[k]] = fabs(R[k].j0 - R[k].j1);
        L.kind[wv][t[k]] = (uint8_t)(cls[k] == 1 ? SCORE_FP : (cls[k] == 3 ? SCORE_FN : SCORE_NONE));
      }
    }
    uint32_t *W = L.cnt[wv];
#pragma unroll
    for (int d = 0; d < 4; d++) {
      const int k = d == 3 ? 0 : 1;                          /* depth 3 is node 0 of every lane, depths 0..2 are node 1 */
#pragma unroll
      for (int c = 0; c < 4; c++) score_wave_count(&W[4 * d + c], cls[k] == c && N[k].d == d);
      score_wave_count(&W[16 + d], cls[k] == 4 && N[k].d == d);
    }
  } else {
    uint32_t *W = L.cnt[wv];
    fcu_ctu_score *out = ctu + (size_t)pic * G.n_ctu + a;
    if (l < 16) {                                            /* dword l: n[4][4] in pairs, open[4] in pairs, then `pad` */
      uint32_t w = 0;
      if (l < 10) w = W[2 * l] | (W[2 * l + 1] << 16);
      ((FCU_HBM uint32_t *)out)[l] = w;
    } else if (l < 24) {                                     /* loss[d][k]: the nodes of depth d in z-order, one term after the other */
      const int d = (l - 16) >> 1, k = (l - 16) & 1;
      const int first = d == 0 ? 0 : (d == 1 ? 1 : (d == 2 ? 5 : 21)), n = 1 << (2 * d);
      double s = 0.0;
      for (int j = 0; j < n; j++) if (L.kind[wv][first + j] == (k ? SCORE_FN : SCORE_FP)) s += L.loss[wv][first + j];
      ((FCU_HBM double *)out)[8 + 2 * d + k] = s;
    }
  }
}

/* ---- score_pic: lane i < 24: v.n[d][k], i = 6 d + k (k < 4: the count n[d][k], k = 4, 5: loss[d][k - 4]); 24..27: open[d];
 * 28..31: scored[d] = the four counts of depth d */
__device__ static inline void score_pic_body(const fcu_ctu_score *ctu, fcu_pic_score *rec, int n_ctu)
{
  const int i = (int)threadIdx.x, pic = (int)blockIdx.x;
  if (i >= SCORE_PIC_LANES) return;
  const FCU_HBM fcu_ctu_score *c = (const FCU_HBM fcu_ctu_score *)(ctu + (size_t)pic * n_ctu);
  FCU_HBM fcu_pic_score *out = (FCU_HBM fcu_pic_score *)(rec + pic);
  if (i < 24 && i % 6 >= 4) {
    const int d = i / 6, k = i % 6 - 4;
    double s = 0.0;
    for (int r0 = 0; r0 < n_ctu; r0 += SCORE_AHEAD) {
      double v[SCORE_AHEAD];
#pragma unroll
      for (int j = 0; j < SCORE_AHEAD; j++) v[j] = r0 + j < n_ctu ? c[r0 + j].loss[d][k] : 0.0;
#pragma unroll
      for (int j = 0; j < SCORE_AHEAD; j++) if (r0 + j < n_ctu) s += v[j];      /* raster order, one after the other */
    }
    out->v.n[d][4 + k] = s;
  } else {
    const int d = i < 24 ? i / 6 : (i - 24) & 3, k = i < 24 ? i % 6 : (i < 28 ? 4 : 5);      /* 4: open, 5: scored */
    uint64_t s = 0;
    for (int r0 = 0; r0 < n_ctu; r0 += SCORE_AHEAD) {
      uint32_t v[SCORE_AHEAD];
#pragma unroll
      for (int j = 0; j < SCORE_AHEAD; j++) {
        v[j] = 0;
        if (r0 + j < n_ctu) {
          const FCU_HBM fcu_ctu_score &q = c[r0 + j];
          v[j] = k < 4 ? q.n[d][k] : (k == 4 ? q.open[d] : (uint32_t)q.n[d][0] + q.n[d][1] + q.n[d][2] + q.n[d][3]);
        }
      }
#pragma unroll
      for (int j = 0; j < SCORE_AHEAD; j++) s += v[j];
    }
    if (i < 24) out->v.n[d][k] = (double)s;                  /* (exact: far below 2^53) */
    else if (i < 28) out->open[d] = (uint32_t)s;
    else out->scored[d] = (uint32_t)s;
  }
}

/* ---- trace_ctu: the whole kernel body (no LDS, no barrier) */
__device__ static inline void trace_ctu_body(const fcu_cu_trace *const *traces, const TraceOut Q, const MapsGeom &G)
{
  const int l = (int)threadIdx.x & 63, a = (int)blockIdx.x * SCORE_CTUS + ((int)threadIdx.x >> 6), pic = (int)blockIdx.y;
  if (a >= G.n_ctu) return;                                  /* (a whole wave) */
  const int cx = a % G.w_ctu, cy = a / G.w_ctu;
  const fcu_cu_trace *rec = traces[pic] + (size_t)a * FCU_CUS_PER_CTU;
  const size_t base = (size_t)pic * (size_t)G.lvl_off[4];
  const int t[2] = { 21 + l, l < 21 ? l : 0 };
  MapsNode N[2] = { maps_node(t[0]), maps_node(t[1]) };
  MapsPlace C[2] = { maps_place(G, N[0], cx, cy), maps_place(G, N[1], cx, cy) };
  C[1].exists = C[1].exists && l < 21;
  TraceRec R[2];
#pragma unroll
  for (int k = 0; k < 2; k++) R[k] = trace_load(rec + t[k]);  /* (inside the CTU's 85 records whether or not the block exists) */
#pragma unroll
  for (int k = 0; k < 2; k++) {
    if (!C[k].exists) continue;                              /* idx < lvl_off[4] for every block that starts inside the picture */
    const bool forced = !C[k].whole, kept = !forced && R[k].valid != 0 && R[k].split_tried != 0;      /* (a level-3 block is always whole) */
    const size_t o = base + (size_t)C[k].idx;
    if (Q.labels) ((FCU_HBM int8_t *)Q.labels)[o] = (int8_t)(forced ? FCU_LABEL_FORCED : (kept ? (R[k].split_won != 0 ? FCU_LABEL_SPLIT : FCU_LABEL_NOT_SPLIT) : FCU_LABEL_ABSENT));
    if (Q.j0) ((FCU_HBM double *)Q.j0)[o] = kept ? R[k].j0 : 0.0;
    if (Q.j1) ((FCU_HBM double *)Q.j1)[o] = kept ? R[k].j1 : 0.0;
  }
}

#ifndef FCU_EMU
__global__ void __launch_bounds__(SCORE_THREADS) score_ctu(const ScorePic *pics, fcu_ctu_score *ctu, const MapsGeom G)
{
  __shared__ ScoreLds L;
  score_ctu_phase<1>(L, pics, ctu, G);
  __syncthreads();
  score_ctu_phase<2>(L, pics, ctu, G);
}
__global__ void __launch_bounds__(SCORE_PIC_THREADS) score_pic(const fcu_ctu_score *ctu, fcu_pic_score *rec, int n_ctu)
{
  score_pic_body(ctu, rec, n_ctu);
}
__global__ void __launch_bounds__(SCORE_THREADS) trace_ctu(const fcu_cu_trace *const *traces, const TraceOut Q, const MapsGeom G)
{
  trace_ctu_body(traces, Q, G);
}
#endif

} /* namespace fcu */
