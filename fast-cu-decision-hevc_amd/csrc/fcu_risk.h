/*
 * fcu_risk.h -- the risk-table model on the device: trained on CU traces (fcu_risk_train), run as a table lookup (fcu_risk_predict),
 * and the N_OBF map of a picture that has not been decided (fcu_nobf_maps).  Definition, sample set, quantised loss and rule:
 * include/fcu.h; risk_q and risk_rule: fcu_host.h.  Included by fcu_kernels.hip only (and by the test-only CPU build
 * tests/emu/risk_emu.cpp).
 *
 *   risk_train   RISK_THREADS threads = RISK_WAVES waves per workgroup, the whole model as one table in LDS (RiskSlot, 24 680 B:
 *                a key may name any of the 257 bins at every depth).  A wave takes a (CTU, picture) unit at a time, units
 *                u = workgroup * RISK_WAVES + wave, then in steps of the grid; nodes dealt to lanes as in trace_ctu: lane l owns
 *                node 21 + l (depth 3) and, l < 21, node l (depths 0..2).  A lane loads its 24-byte records as three 8-byte words
 *                and, for a sample, the 2-byte key at the block's element of the key array, all loads before the first use;
 *                a sample is one 64-bit and one 32-bit integer add into LDS.  Integer adds commute, so the table does not
 *                depend on the order the lanes and waves arrive in.  After a barrier the table leaves as 8-byte words to the
 *                workgroup's slot of a context buffer: every word of the slot is written, nothing is cleared beforehand.
 *   risk_add     one workgroup per RISK_ADD_CELLS cells (a cell = one (depth, key, truth) entry: its sum and its count; cell
 *                RISK_CELLS is the dropped counter).  Wave w adds the slots w, w + 4, ... of its 64 cells, four loads in flight;
 *                the four partial sums meet in LDS and lanes 0..63 of wave 0 write -- or add to -- the model.  Every word of
 *                the model is written by exactly one thread.
 *   risk_predict one thread per block of the label layout; a workgroup stays inside one level (RiskPlan), so the 257 labels of
 *                that level's table are formed once per workgroup from the model in HBM (risk_rule) and staged in LDS; a
 *                thread loads its key and stores its one label byte.
 *   nobf_blocks  fcu_nobf_maps: the same grid; a thread counts maps_obf_flag (fcu_maps.h, the flag maps_ctu counts) over the
 *                4x4 partitions of its block and stores one uint16.  No LDS.
 * No global atomics; nothing must be cleared beforehand: a repeated call gives identical bytes.  Algorithmic bytes: train 85 x 24 B
 * + up to 85 x 2 B per CTU read, 24 680 B per workgroup written and read again; predict 2 B read and 1 B written per block + the
 * level's table per workgroup; N_OBF 2 B per partition and level read, 2 B per block written.
 */
#pragma once
#include "fcu_trace.h"

namespace fcu {

enum { RISK_THREADS = 512, RISK_WAVES = RISK_THREADS / 64, RISK_CELLS = 4 * FCU_RISK_BINS * 2, RISK_MAX_SLOTS = 128, RISK_UNITS_PER_WAVE = 2,
       RISK_ADD_THREADS = 256, RISK_ADD_CELLS = 64, RISK_ADD_GROUPS = (RISK_CELLS + 1 + RISK_ADD_CELLS - 1) / RISK_ADD_CELLS,
       RISK_PRED_THREADS = 256 };

/* a workgroup's table, in LDS and as its slot in HBM: the model's two arrays flat, then the samples dropped */
struct RiskSlot { int64_t risk[RISK_CELLS]; uint32_t count[RISK_CELLS]; uint32_t dropped, pad; };
static_assert(sizeof(fcu_risk_model) == 24672 && offsetof(fcu_risk_model, count) == 8 * RISK_CELLS && sizeof(RiskSlot) == sizeof(fcu_risk_model) + 8
              && offsetof(RiskSlot, count) == offsetof(fcu_risk_model, count) && sizeof(RiskSlot) % 8 == 0, "the flat cell layout of model and slot");

/* workgroups of risk_predict / nobf_blocks: those of level d are [wg_off[d], wg_off[d + 1]) */
struct RiskPlan { int wg_off[5]; };
inline RiskPlan risk_plan(const MapsGeom &G)
{
  RiskPlan P = {};
  for (int d = 0; d < 4; d++) P.wg_off[d + 1] = P.wg_off[d] + (G.lvl_off[d + 1] - G.lvl_off[d] + RISK_PRED_THREADS - 1) / RISK_PRED_THREADS;
  return P;
}
/* workgroups (= slots) of risk_train for a batch of n_units (CTU, picture) units */
inline int risk_train_groups(int n_units)
{
  const int per = RISK_WAVES * RISK_UNITS_PER_WAVE, n = (n_units + per - 1) / per;
  return n < 1 ? 1 : (n > RISK_MAX_SLOTS ? RISK_MAX_SLOTS : n);
}

/* integer adds into the workgroup's LDS table (the CPU build runs the threads one after the other) */
__device__ static inline void risk_lds_add(int64_t *p, int64_t v)
{
#ifdef FCU_EMU
  *p += v;
#else
  atomicAdd((unsigned long long *)p, (unsigned long long)v);
#endif
}
__device__ static inline void risk_lds_add(uint32_t *p, uint32_t v)
{
#ifdef FCU_EMU
  *p += v;
#else
  atomicAdd(p, v);
#endif
}

/* ---- risk_train: phase 0 clears the table, phase 1 adds the samples, phase 2 stores the slot */
template <int PHASE>
__device__ static inline void risk_train_phase(RiskSlot &L, const fcu_cu_trace *const *traces, const uint16_t *const *keys, RiskSlot *slots, const MapsGeom &G, int n_units, int n_groups)
{
  const int t = (int)threadIdx.x;
  if (PHASE == 0) {
    uint64_t *w = (uint64_t *)&L;
    for (int i = t; i < (int)(sizeof(RiskSlot) / 8); i += RISK_THREADS) w[i] = 0;
  } else if (PHASE == 1) {
    const int l = t & 63, wv = t >> 6;
    const int tn[2] = { 21 + l, l < 21 ? l : 0 };
    const bool own[2] = { true, l < 21 };
    const MapsNode N[2] = { maps_node(tn[0]), maps_node(tn[1]) };
    for (int u = (int)blockIdx.x * RISK_WAVES + wv; u < n_units; u += n_groups * RISK_WAVES) {      /* (a whole wave) */
      const int pic = u / G.n_ctu, a = u - pic * G.n_ctu, cx = a % G.w_ctu, cy = a / G.w_ctu;
      const fcu_cu_trace *rec = traces[pic] + (size_t)a * FCU_CUS_PER_CTU;
      const FCU_HBM uint16_t *key = (const FCU_HBM uint16_t *)keys[pic];
      const MapsPlace C[2] = { maps_place(G, N[0], cx, cy), maps_place(G, N[1], cx, cy) };
      TraceRec R[2];
#pragma unroll
      for (int k = 0; k < 2; k++) R[k] = trace_load(rec + tn[k]);   /* (inside the CTU's 85 records whether or not the block exists) */
      bool sample[2]; uint32_t x[2] = { 0, 0 };
#pragma unroll
      for (int k = 0; k < 2; k++) {                            /* a whole block exists: idx < lvl_off[4], inside the key array */
        sample[k] = own[k] && C[k].whole && R[k].valid != 0 && R[k].split_tried != 0 && R[k].whole_tried != 0;
        if (sample[k]) x[k] = key[C[k].idx];
      }
#pragma unroll
      for (int k = 0; k < 2; k++) {
        if (!sample[k]) continue;
        if (x[k] >= FCU_RISK_BINS) { risk_lds_add(&L.dropped, 1u); continue; }
        const int cell = (N[k].d * FCU_RISK_BINS + (int)x[k]) * 2 + (R[k].split_won != 0 ? 1 : 0);      /* < RISK_CELLS */
        risk_lds_add(&L.risk[cell], risk_q(R[k].j0, R[k].j1));
        risk_lds_add(&L.count[cell], 1u);
      }
    }
  } else {
    const uint64_t *w = (const uint64_t *)&L;
    FCU_HBM uint64_t *out = (FCU_HBM uint64_t *)(slots + blockIdx.x);
    for (int i = t; i < (int)(sizeof(RiskSlot) / 8); i += RISK_THREADS) out[i] = w[i];
  }
}

/* ---- risk_add: phase 1 leaves every wave's partial sums in LDS, phase 2 writes the model (and the dropped counter) */
struct RiskAddLds { int64_t risk[RISK_ADD_THREADS]; uint32_t count[RISK_ADD_THREADS]; };
template <int PHASE>
__device__ static inline void risk_add_phase(RiskAddLds &L, const RiskSlot *slots, int n_slots, fcu_risk_model *model, uint32_t *dropped, int accumulate)
{
  const int t = (int)threadIdx.x, l = t & 63, e = (int)blockIdx.x * RISK_ADD_CELLS + l;      /* e == RISK_CELLS: the dropped counter */
  if (PHASE == 1) {
    int64_t r = 0; uint32_t n = 0;
    if (e <= RISK_CELLS) {
      const int part = t >> 6, step = RISK_ADD_THREADS / 64;
      for (int s0 = part; s0 < n_slots; s0 += 4 * step) {      /* four slots in flight */
        int64_t rv[4]; uint32_t nv[4];
#pragma unroll
        for (int j = 0; j < 4; j++) {
          const int s = s0 + j * step;
          rv[j] = 0; nv[j] = 0;
          if (s < n_slots) {
            const FCU_HBM RiskSlot &S = *(const FCU_HBM RiskSlot *)(slots + s);
            if (e < RISK_CELLS) { rv[j] = S.risk[e]; nv[j] = S.count[e]; } else nv[j] = S.dropped;
          }
        }
#pragma unroll
        for (int j = 0; j < 4; j++) { r += rv[j]; n += nv[j]; }
      }
    }
    L.risk[t] = r; L.count[t] = n;
  } else if (t < 64 && e <= RISK_CELLS) {
    int64_t r = 0; uint32_t n = 0;
    for (int j = 0; j < RISK_ADD_THREADS / 64; j++) { r += L.risk[j * 64 + l]; n += L.count[j * 64 + l]; }
    if (e < RISK_CELLS) {
      FCU_HBM int64_t *mr = (FCU_HBM int64_t *)model + e;
      FCU_HBM uint32_t *mc = (FCU_HBM uint32_t *)((char *)model + offsetof(fcu_risk_model, count)) + e;
      if (accumulate) { r += *mr; n += *mc; }
      *mr = r; *mc = n;
    } else *(FCU_HBM uint32_t *)dropped = n;
  }
}

/* the level a workgroup of risk_predict / nobf_blocks works on */
__device__ static inline int risk_plan_level(const RiskPlan &P, int wg) { return wg < P.wg_off[1] ? 0 : (wg < P.wg_off[2] ? 1 : (wg < P.wg_off[3] ? 2 : 3)); }

/* ---- risk_predict: phase 1 stages the level's labels, phase 2 stores one label per thread */
struct RiskPredLds { int8_t tab[FCU_RISK_BINS + 3]; };
template <int PHASE>
__device__ static inline void risk_predict_phase(RiskPredLds &L, const uint16_t *const *keys, const fcu_risk_model *model, int min_count, int8_t *labels, const MapsGeom &G, const RiskPlan &P)
{
  const int t = (int)threadIdx.x, pic = (int)blockIdx.y, d = risk_plan_level(P, (int)blockIdx.x);
  if (PHASE == 1) {
    const FCU_HBM fcu_risk_model &M = *(const FCU_HBM fcu_risk_model *)model;
    for (int x = t; x < FCU_RISK_BINS; x += RISK_PRED_THREADS)
      L.tab[x] = (int8_t)risk_rule(M.risk[d][x][0], M.risk[d][x][1], M.count[d][x][0], M.count[d][x][1], min_count);
  } else {
    const int e = ((int)blockIdx.x - P.wg_off[d]) * RISK_PRED_THREADS + t, n = G.lvl_off[d + 1] - G.lvl_off[d];
    if (e >= n) return;                                      /* lvl_off[d] + e < lvl_off[4] from here on */
    const int s = 64 >> d, bx = e % G.lvl_w[d], by = e / G.lvl_w[d];
    const bool whole = (bx + 1) * s <= G.width && (by + 1) * s <= G.height;
    const uint32_t x = ((const FCU_HBM uint16_t *)keys[pic])[G.lvl_off[d] + e];
    const int v = d < 3 && !whole ? FCU_LABEL_FORCED : (x >= FCU_RISK_BINS ? FCU_LABEL_ABSENT : L.tab[x]);
    ((FCU_HBM int8_t *)labels)[(size_t)pic * (size_t)G.lvl_off[4] + (size_t)(G.lvl_off[d] + e)] = (int8_t)v;
  }
}

/* ---- nobf_blocks: the whole kernel body (no LDS, no barrier) */
template <int D>
__device__ static inline uint16_t nobf_block(const int16_t *obf, int W4, int H4, int bx, int by)
{
  const int s4 = 16 >> D;
  uint32_t n = 0;
  for (int yy = 0; yy < s4; yy++) {
#pragma unroll
    for (int xx = 0; xx < s4; xx++) n += maps_obf_flag(obf, W4, H4, bx * s4 + xx, by * s4 + yy);
  }
  return (uint16_t)n;
}
__device__ static inline void nobf_blocks_body(const int16_t *const *obfs, uint16_t *nobf, const MapsGeom &G, const RiskPlan &P)
{
  const int t = (int)threadIdx.x, pic = (int)blockIdx.y, d = risk_plan_level(P, (int)blockIdx.x);
  const int e = ((int)blockIdx.x - P.wg_off[d]) * RISK_PRED_THREADS + t, n = G.lvl_off[d + 1] - G.lvl_off[d];
  if (e >= n) return;                                        /* lvl_off[d] + e < lvl_off[4] from here on */
  const int bx = e % G.lvl_w[d], by = e / G.lvl_w[d], W4 = G.width >> 2, H4 = G.height >> 2;
  const int16_t *obf = obfs[pic];
  const uint16_t v = d == 0 ? nobf_block<0>(obf, W4, H4, bx, by) : (d == 1 ? nobf_block<1>(obf, W4, H4, bx, by) : (d == 2 ? nobf_block<2>(obf, W4, H4, bx, by) : nobf_block<3>(obf, W4, H4, bx, by)));
  ((FCU_HBM uint16_t *)nobf)[(size_t)pic * (size_t)G.lvl_off[4] + (size_t)(G.lvl_off[d] + e)] = v;
}

#ifndef FCU_EMU
__global__ void __launch_bounds__(RISK_THREADS) risk_train(const fcu_cu_trace *const *traces, const uint16_t *const *keys, RiskSlot *slots, const MapsGeom G, int n_units, int n_groups)
{
  __shared__ RiskSlot L;
  risk_train_phase<0>(L, traces, keys, slots, G, n_units, n_groups);
  __syncthreads();
  risk_train_phase<1>(L, traces, keys, slots, G, n_units, n_groups);
  __syncthreads();
  risk_train_phase<2>(L, traces, keys, slots, G, n_units, n_groups);
}
__global__ void __launch_bounds__(RISK_ADD_THREADS) risk_add(const RiskSlot *slots, int n_slots, fcu_risk_model *model, uint32_t *dropped, int accumulate)
{
  __shared__ RiskAddLds L;
  risk_add_phase<1>(L, slots, n_slots, model, dropped, accumulate);
  __syncthreads();
  risk_add_phase<2>(L, slots, n_slots, model, dropped, accumulate);
}
__global__ void __launch_bounds__(RISK_PRED_THREADS) risk_predict(const uint16_t *const *keys, const fcu_risk_model *model, int min_count, int8_t *labels, const MapsGeom G, const RiskPlan P)
{
  __shared__ RiskPredLds L;
  risk_predict_phase<1>(L, keys, model, min_count, labels, G, P);
  __syncthreads();
  risk_predict_phase<2>(L, keys, model, min_count, labels, G, P);
}
__global__ void __launch_bounds__(RISK_PRED_THREADS) nobf_blocks(const int16_t *const *obfs, uint16_t *nobf, const MapsGeom G, const RiskPlan P)
{
  nobf_blocks_body(obfs, nobf, G, P);
}
#endif

} /* namespace fcu */
