/*
 * fcu_tree.h -- the key tree on the device: feature maps to 32 bins per column (fcu_feature_bins), a tree walk per block to the
 * key of the risk table (fcu_tree_keys), and the histograms a level of the tree is chosen from (fcu_tree_hist).  Definitions:
 * include/fcu.h; the argument rules and the split choice: fcu_host.h.  Included by fcu_kernels.hip only (and by the test-only CPU
 * build tests/emu/tree_emu.cpp).
 *
 *   feat_bins  TREE_THREADS threads, a workgroup takes TREE_BIN_ROWS rows of one level (TreePlan) of one picture: the level's edges,
 *              F x 31 floats (18 104 B for F = 146), go to LDS once, then thread t takes the elements t, t + TREE_THREADS, ... of the
 *              rows' F values as one flat run: consecutive lanes load consecutive floats and store consecutive bytes.  A value's bin
 *              is the upper bound of a 5-step search over its column's 31 edges (stride 31 words: no bank conflict between
 *              columns); every comparison is `e <= x`, false for NaN.
 *   tree_keys  one thread per block, TREE_THREADS per workgroup inside one level; the level's 31 nodes in LDS; a thread walks
 *              `levels` steps, one byte load of its row of bins per split node, and stores one uint16.
 *   tree_hist  a workgroup owns one depth d, one tile of TREE_LDS_COLS >> level columns and the chunks c, c + chunks(d), ... of
 *              TREE_CHUNK blocks of that depth over the whole batch (TreeHistPlan: at most TREE_MAX_CHUNKS workgroups per depth and
 *              tile).  Its LDS table (TreeSlot, 49 160 B) holds [2^level nodes][tile columns][32 bins][2] cells, 4096 whatever the
 *              level.  A thread takes a block: the trace record of that block (three 8-byte loads, the loads of risk_train), the
 *              sample test and q of risk_sample, the block's node, then per column of the tile one byte of bins and one 64-bit and
 *              one 32-bit integer LDS add; lane l starts at column l of the tile and wraps, so that the lanes of a wave do not all
 *              add to one column at a time.  After a barrier the table leaves as 8-byte words to the workgroup's slot: every word
 *              is written, nothing is cleared beforehand.  The workgroups of tile 0 count the dropped samples.
 *   tree_fold  one thread per cell of the histograms (and one for the dropped counter): it adds the slots of the cell's depth and
 *              tile, TREE_FOLD_AHEAD loads in flight, and writes -- or adds to -- risk and count.  Every word is written by
 *              exactly one thread.
 * No global atomics, nothing to clear: a repeated call gives identical bytes.  Algorithmic bytes: feat_bins 4 B read + 1 B written
 * per element; tree_keys <= 5 B read + 2 B written per block; tree_hist per block and column tile 24 B of trace + 2 B of node +
 * one byte per column, 49 160 B per workgroup written and read again; tree_fold 12 B per cell written.
 */
#pragma once
#include "fcu_trace.h"
#include "fcu_risk.h"

namespace fcu {

enum { TREE_THREADS = 256, TREE_BIN_ROWS = 128, TREE_EDGES = FCU_TREE_BINS - 1, TREE_MAX_F = FCU_FEAT_TMV + FCU_FEAT_SOC,
       TREE_LDS_COLS = 64,                                   /* (node, column) pairs of a tree_hist table: the tile is 64 >> level columns */
       TREE_CELLS = TREE_LDS_COLS * FCU_TREE_BINS * 2,       /* cells of a table */
       TREE_CHUNK = 1024, TREE_CHUNK_TRIPS = TREE_CHUNK / TREE_THREADS, TREE_MAX_CHUNKS = 8,
       TREE_FOLD_THREADS = 256, TREE_FOLD_AHEAD = 4 };
static_assert((TREE_LDS_COLS >> (FCU_TREE_MAX_LEVELS - 1)) >= 1 && TREE_CHUNK % TREE_THREADS == 0, "a tile holds a column at the last level; whole trips");

/* a workgroup's table, in LDS and as its slot in HBM */
struct TreeSlot { int64_t risk[TREE_CELLS]; uint32_t count[TREE_CELLS]; uint32_t dropped, pad; };
static_assert(sizeof(TreeSlot) == 12 * TREE_CELLS + 8 && sizeof(TreeSlot) % 8 == 0 && sizeof(TreeSlot) <= 65536, "the slot goes out as 8-byte words and fits LDS");

/* workgroups of feat_bins (per = TREE_BIN_ROWS) / tree_keys (per = TREE_THREADS): those of level d are [wg_off[d], wg_off[d + 1]) */
struct TreePlan { int wg_off[5]; };
inline TreePlan tree_plan(const MapsGeom &G, int per)
{
  TreePlan P = {};
  for (int d = 0; d < 4; d++) P.wg_off[d + 1] = P.wg_off[d] + (G.lvl_off[d + 1] - G.lvl_off[d] + per - 1) / per;
  return P;
}
__device__ static inline int tree_plan_level(const TreePlan &P, int wg) { return wg < P.wg_off[1] ? 0 : (wg < P.wg_off[2] ? 1 : (wg < P.wg_off[3] ? 2 : 3)); }

/* the grid of tree_hist: per depth d the blocks of the batch (rows of level d x pictures) in chunks, chunk workgroups
 * [chunk_off[d], chunk_off[d + 1]) of every tile; workgroup = chunk workgroup * n_tiles + tile, and that is its slot as well */
struct TreeHistPlan { int level, F, tile, n_tiles, n_pics, blocks[4], chunk_off[5]; };
inline TreeHistPlan tree_hist_plan(const MapsGeom &G, int n_pics, int F, int level)
{
  TreeHistPlan P = {};
  P.level = level; P.F = F; P.tile = TREE_LDS_COLS >> level; P.n_tiles = (F + P.tile - 1) / P.tile; P.n_pics = n_pics;
  for (int d = 0; d < 4; d++) {
    P.blocks[d] = (G.lvl_off[d + 1] - G.lvl_off[d]) * n_pics;      /* <= 2^22 (the argument rules) */
    const int n = (P.blocks[d] + TREE_CHUNK - 1) / TREE_CHUNK;
    P.chunk_off[d + 1] = P.chunk_off[d] + (n > TREE_MAX_CHUNKS ? TREE_MAX_CHUNKS : n);
  }
  return P;
}
inline int tree_hist_groups(const TreeHistPlan &P) { return P.chunk_off[4] * P.n_tiles; }
FCU_HOST_DEV inline int tree_hist_cells(int F, int level) { return 4 * (1 << level) * F * FCU_TREE_BINS * 2; }

/* ---- feat_bins: phase 1 stages the level's edges, phase 2 bins the workgroup's rows */
struct TreeBinLds { float edge[TREE_MAX_F * TREE_EDGES + 1]; };
template <int PHASE>
__device__ static inline void feat_bins_phase(TreeBinLds &L, const float *features, const float *edges, uint8_t *bins, const MapsGeom &G, const TreePlan &P, int F)
{
  const int t = (int)threadIdx.x, pic = (int)blockIdx.y, d = tree_plan_level(P, (int)blockIdx.x);
  if (PHASE == 1) {
    const FCU_HBM float *e = (const FCU_HBM float *)edges + (size_t)d * (size_t)(F * TREE_EDGES);
    for (int i = t; i < F * TREE_EDGES; i += TREE_THREADS) L.edge[i] = e[i];
  } else {
    const int r0 = ((int)blockIdx.x - P.wg_off[d]) * TREE_BIN_ROWS, n = G.lvl_off[d + 1] - G.lvl_off[d];
    const int rows = n - r0 < TREE_BIN_ROWS ? n - r0 : TREE_BIN_ROWS, count = rows * F;      /* rows >= 1 by the plan */
    const size_t base = ((size_t)pic * (size_t)G.lvl_off[4] + (size_t)(G.lvl_off[d] + r0)) * (size_t)F;
    const FCU_HBM float *in = (const FCU_HBM float *)features + base;
    FCU_HBM uint8_t *out = (FCU_HBM uint8_t *)bins + base;
    for (int i = t; i < count; i += TREE_THREADS) {          /* base + i < n_pics * NL * F */
      const float x = in[i];
      const float *e = L.edge + (i % F) * TREE_EDGES;
      int lo = 0;                                            /* edges e[0 .. lo) are <= x */
#pragma unroll
      for (int step = 16; step >= 1; step >>= 1) if (e[lo + step - 1] <= x) lo += step;      /* lo + step - 1 <= 30 */
      out[i] = (uint8_t)lo;
    }
  }
}

/* ---- tree_keys: phase 1 stages the level's nodes, phase 2 walks one block per thread */
struct TreeKeyLds { int16_t feature[FCU_TREE_NODES + 1]; uint8_t thr[FCU_TREE_NODES + 1]; };
template <int PHASE>
__device__ static inline void tree_keys_phase(TreeKeyLds &L, const uint8_t *const *bins, const fcu_key_tree *tree, int levels, uint16_t *keys, const MapsGeom &G, const TreePlan &P, int F)
{
  const int t = (int)threadIdx.x, pic = (int)blockIdx.y, d = tree_plan_level(P, (int)blockIdx.x);
  if (PHASE == 1) {
    const FCU_HBM fcu_key_tree &T = *(const FCU_HBM fcu_key_tree *)tree;
    if (t < FCU_TREE_NODES) { L.feature[t] = T.feature[d][t]; L.thr[t] = T.thr[d][t]; }
  } else {
    const int e = ((int)blockIdx.x - P.wg_off[d]) * TREE_THREADS + t, n = G.lvl_off[d + 1] - G.lvl_off[d];
    if (e >= n) return;                                      /* lvl_off[d] + e < lvl_off[4] from here on */
    const FCU_HBM uint8_t *row = (const FCU_HBM uint8_t *)bins[pic] + (size_t)(G.lvl_off[d] + e) * (size_t)F;
    int i = 0;
    for (int s = 0; s < levels; s++) {                       /* i <= 2^(s + 1) - 2 <= 30 < FCU_TREE_NODES: levels <= 5 */
      const int f = L.feature[i];                            /* -1 or < F (the argument rules) */
      const bool right = f >= 0 && row[f] > L.thr[i];
      i = 2 * i + 1 + (right ? 1 : 0);
    }
    ((FCU_HBM uint16_t *)keys)[(size_t)pic * (size_t)G.lvl_off[4] + (size_t)(G.lvl_off[d] + e)] = (uint16_t)(i - ((1 << levels) - 1));
  }
}

/* block e of level d (raster inside the level): its CTU, its record inside the CTU's 85 (z-order inside the depth) and whether it
 * lies wholly inside the picture -- maps_place the other way round */
struct TreeBlock { int ctu, rec; bool whole; };
__device__ static inline TreeBlock tree_block(const MapsGeom &G, int d, int e)
{
  const int bx = e % G.lvl_w[d], by = e / G.lvl_w[d], s = 64 >> d, m = (1 << d) - 1, x = bx & m, y = by & m;
  int j = 0;
#pragma unroll
  for (int b = 0; b < 3; b++) j |= (((x >> b) & 1) << (2 * b)) | (((y >> b) & 1) << (2 * b + 1));
  TreeBlock B;
  B.ctu = (by >> d) * G.w_ctu + (bx >> d);
  B.rec = (d == 0 ? 0 : (d == 1 ? 1 : (d == 2 ? 5 : 21))) + j;
  B.whole = (bx + 1) * s <= G.width && (by + 1) * s <= G.height;
  return B;
}

/* ---- tree_hist: phase 0 clears the table, phase 1 adds the samples, phase 2 stores the slot */
template <int PHASE>
__device__ static inline void tree_hist_phase(TreeSlot &L, const fcu_cu_trace *const *traces, const uint8_t *const *bins, const uint16_t *const *nodes, TreeSlot *slots,
                                              const MapsGeom &G, const TreeHistPlan &P)
{
  const int t = (int)threadIdx.x, wg = (int)blockIdx.x, cw = wg / P.n_tiles, tile = wg - cw * P.n_tiles;
  if (PHASE == 0) {
    uint64_t *w = (uint64_t *)&L;
    for (int i = t; i < (int)(sizeof(TreeSlot) / 8); i += TREE_THREADS) w[i] = 0;
  } else if (PHASE == 1) {
    const int d = cw < P.chunk_off[1] ? 0 : (cw < P.chunk_off[2] ? 1 : (cw < P.chunk_off[3] ? 2 : 3));
    const int c = cw - P.chunk_off[d], chunks = P.chunk_off[d + 1] - P.chunk_off[d], n = G.lvl_off[d + 1] - G.lvl_off[d];
    const int f0 = tile * P.tile, cols = P.F - f0 < P.tile ? P.F - f0 : P.tile, n_nodes = 1 << P.level;
    for (int k = c; k * TREE_CHUNK < P.blocks[d]; k += chunks) {
      for (int trip = 0; trip < TREE_CHUNK_TRIPS; trip++) {
        const int g = k * TREE_CHUNK + trip * TREE_THREADS + t;
        if (g >= P.blocks[d]) continue;
        const int pic = g / n, e = g - pic * n;              /* pic < n_pics */
        const TreeBlock B = tree_block(G, d, e);
        if (!B.whole) continue;                              /* a whole block: its CTU and its record exist */
        const TraceRec R = trace_load(traces[pic] + (size_t)B.ctu * FCU_CUS_PER_CTU + B.rec);
        int64_t q;
        if (!risk_sample(R.valid, R.split_tried, R.whole_tried, R.j0, R.j1, &q)) continue;
        const int row = G.lvl_off[d] + e;                    /* < NL */
        const int node = nodes ? (int)((const FCU_HBM uint16_t *)nodes[pic])[row] : 0;
        if (node >= n_nodes) { if (tile == 0) risk_lds_add(&L.dropped, 1u); continue; }
        const FCU_HBM uint8_t *b = (const FCU_HBM uint8_t *)bins[pic] + (size_t)row * (size_t)P.F + f0;
        const int truth = R.split_won != 0 ? 1 : 0;
        for (int i = 0; i < P.tile; i++) {
          const int fi = (i + t) & (P.tile - 1);             /* the tile is a power of two */
          if (fi >= cols) continue;                          /* f0 + fi < F */
          const int bin = b[fi] & (FCU_TREE_BINS - 1);       /* (bins are 0..31; the mask keeps a foreign byte inside the table) */
          const int cell = (((node * P.tile + fi) * FCU_TREE_BINS) + bin) * 2 + truth;      /* < TREE_CELLS: node * tile + fi < 64 */
          risk_lds_add(&L.risk[cell], q);
          risk_lds_add(&L.count[cell], 1u);
        }
      }
    }
  } else {
    const uint64_t *w = (const uint64_t *)&L;
    FCU_HBM uint64_t *out = (FCU_HBM uint64_t *)(slots + wg);
    for (int i = t; i < (int)(sizeof(TreeSlot) / 8); i += TREE_THREADS) out[i] = w[i];
  }
}

/* ---- tree_fold: the whole kernel body (no LDS, no barrier) */
__device__ static inline void tree_fold_body(const TreeSlot *slots, const TreeHistPlan &P, int64_t *risk, uint32_t *count, uint32_t *dropped, int accumulate)
{
  const int g = (int)blockIdx.x * TREE_FOLD_THREADS + (int)threadIdx.x, n_cells = tree_hist_cells(P.F, P.level);
  if (g > n_cells) return;
  if (g == n_cells) {                                        /* the dropped samples: the workgroups of tile 0, every depth */
    uint32_t n = 0;
    for (int cw = 0; cw < P.chunk_off[4]; cw++) n += ((const FCU_HBM TreeSlot *)(slots + (size_t)cw * P.n_tiles))->dropped;
    *(FCU_HBM uint32_t *)dropped = n;
    return;
  }
  /* g = (((d * 2^level + node) * F + f) * 32 + bin) * 2 + truth */
  const int bt = g & (FCU_TREE_BINS * 2 - 1), r = g >> 6, f = r % P.F, dn = r / P.F, node = dn & ((1 << P.level) - 1), d = dn >> P.level;
  const int tile = f / P.tile, fi = f - tile * P.tile, cell = (node * P.tile + fi) * (FCU_TREE_BINS * 2) + bt;
  const int c0 = P.chunk_off[d], c1 = P.chunk_off[d + 1];
  int64_t rs = 0; uint32_t ns = 0;
  for (int cw = c0; cw < c1; cw += TREE_FOLD_AHEAD) {
    int64_t rv[TREE_FOLD_AHEAD]; uint32_t nv[TREE_FOLD_AHEAD];
#pragma unroll
    for (int j = 0; j < TREE_FOLD_AHEAD; j++) {
      rv[j] = 0; nv[j] = 0;
      if (cw + j < c1) {
        const FCU_HBM TreeSlot &S = *(const FCU_HBM TreeSlot *)(slots + ((size_t)(cw + j) * P.n_tiles + tile));
        rv[j] = S.risk[cell]; nv[j] = S.count[cell];
      }
    }
#pragma unroll
    for (int j = 0; j < TREE_FOLD_AHEAD; j++) { rs += rv[j]; ns += nv[j]; }
  }
  FCU_HBM int64_t *pr = (FCU_HBM int64_t *)risk + g;
  FCU_HBM uint32_t *pc = (FCU_HBM uint32_t *)count + g;
  if (accumulate) { rs += *pr; ns += *pc; }
  *pr = rs; *pc = ns;
}

#ifndef FCU_EMU
__global__ void __launch_bounds__(TREE_THREADS) feat_bins(const float *features, const float *edges, uint8_t *bins, const MapsGeom G, const TreePlan P, int F)
{
  __shared__ TreeBinLds L;
  feat_bins_phase<1>(L, features, edges, bins, G, P, F);
  __syncthreads();
  feat_bins_phase<2>(L, features, edges, bins, G, P, F);
}
__global__ void __launch_bounds__(TREE_THREADS) tree_keys(const uint8_t *const *bins, const fcu_key_tree *tree, int levels, uint16_t *keys, const MapsGeom G, const TreePlan P, int F)
{
  __shared__ TreeKeyLds L;
  tree_keys_phase<1>(L, bins, tree, levels, keys, G, P, F);
  __syncthreads();
  tree_keys_phase<2>(L, bins, tree, levels, keys, G, P, F);
}
__global__ void __launch_bounds__(TREE_THREADS) tree_hist(const fcu_cu_trace *const *traces, const uint8_t *const *bins, const uint16_t *const *nodes, TreeSlot *slots, const MapsGeom G, const TreeHistPlan P)
{
  __shared__ TreeSlot L;
  tree_hist_phase<0>(L, traces, bins, nodes, slots, G, P);
  __syncthreads();
  tree_hist_phase<1>(L, traces, bins, nodes, slots, G, P);
  __syncthreads();
  tree_hist_phase<2>(L, traces, bins, nodes, slots, G, P);
}
__global__ void __launch_bounds__(TREE_FOLD_THREADS) tree_fold(const TreeSlot *slots, const TreeHistPlan P, int64_t *risk, uint32_t *count, uint32_t *dropped, int accumulate)
{
  tree_fold_body(slots, P, risk, count, dropped, accumulate);
}
#endif

} /* namespace fcu */
