/*
 * tree_emu.cpp -- TEST-ONLY: the kernel source of the key tree (csrc/fcu_tree.h, with the record loads of csrc/fcu_trace.h and the
 * LDS adds of csrc/fcu_risk.h) compiled for the CPU with the HIP keywords defined away and every grid run as loops (workgroup phases
 * in order, threads inside a phase in order, the workgroup's LDS poisoned before its first phase), behind the argument rules of
 * fcu_host.h the library applies, so that the bin search, the walk, the block addressing, the tiling of the histograms and the fold
 * can be checked against tests/tree_ref.py without a GPU.  It also exports the kernels' tiling enums and plans, so that the cases
 * of tests/tree_cases.py can assert that they cross them.  Not part of libfcu.so.
 */
#define FCU_EMU 1
#include <vector>
#include <cstring>
#include "../../fast-cu-decision-hevc_amd/csrc/fcu_host.h"
#define __device__
struct Dim3 { unsigned x, y, z; };
static thread_local Dim3 blockIdx, threadIdx;
#include "../../fast-cu-decision-hevc_amd/csrc/fcu_tree.h"

using namespace fcu;

static thread_local std::string g_err;

static void run_keys(const MapsGeom &G, int n_pics, int F, const uint8_t *const *bins, const fcu_key_tree *tree, int levels, uint16_t *keys)
{
  const TreePlan P = tree_plan(G, TREE_THREADS);
  static TreeKeyLds L;
  for (unsigned pic = 0; pic < (unsigned)n_pics; pic++) for (unsigned g = 0; g < (unsigned)P.wg_off[4]; g++) {
    blockIdx.x = g; blockIdx.y = pic;
    memset((void *)&L, 0xee, sizeof(L));                     /* (nothing may be read that this workgroup did not write) */
    for (unsigned t = 0; t < TREE_THREADS; t++) { threadIdx.x = t; tree_keys_phase<1>(L, bins, tree, levels, keys, G, P, F); }
    for (unsigned t = 0; t < TREE_THREADS; t++) { threadIdx.x = t; tree_keys_phase<2>(L, bins, tree, levels, keys, G, P, F); }
  }
}

static void run_hist(const MapsGeom &G, int n_pics, int F, int level, const fcu_cu_trace *const *trace, const uint8_t *const *bins, const uint16_t *const *nodes,
                     int64_t *risk, uint32_t *count, int accumulate, uint32_t *dropped)
{
  const TreeHistPlan P = tree_hist_plan(G, n_pics, F, level);
  const int groups = tree_hist_groups(P);
  std::vector<TreeSlot> slots((size_t)groups);
  memset((void *)slots.data(), 0x77, sizeof(TreeSlot) * slots.size());      /* stale bytes: every word of a slot is written */
  static TreeSlot L;                                         /* the workgroup's LDS */
  blockIdx.y = 0;
  for (unsigned g = 0; g < (unsigned)groups; g++) {
    blockIdx.x = g;
    memset((void *)&L, 0xee, sizeof(L));
    for (unsigned t = 0; t < TREE_THREADS; t++) { threadIdx.x = t; tree_hist_phase<0>(L, trace, bins, nodes, slots.data(), G, P); }
    for (unsigned t = 0; t < TREE_THREADS; t++) { threadIdx.x = t; tree_hist_phase<1>(L, trace, bins, nodes, slots.data(), G, P); }
    for (unsigned t = 0; t < TREE_THREADS; t++) { threadIdx.x = t; tree_hist_phase<2>(L, trace, bins, nodes, slots.data(), G, P); }
  }
  uint32_t drop = 0x77777777u;
  const unsigned fold = (unsigned)((tree_hist_cells(F, level) + 1 + TREE_FOLD_THREADS - 1) / TREE_FOLD_THREADS);
  for (unsigned g = 0; g < fold; g++) {
    blockIdx.x = g;
    for (unsigned t = 0; t < TREE_FOLD_THREADS; t++) { threadIdx.x = t; tree_fold_body(slots.data(), P, risk, count, &drop, accumulate); }
  }
  if (dropped) *dropped = drop;
}

extern "C" {
const char *tree_emu_last_error(void) { return g_err.c_str(); }
int tree_emu_sizeof(void) { return (int)sizeof(fcu_key_tree); }
int tree_emu_label_count(int w, int h) { return maps_geom(w, h, 0, nullptr).lvl_off[4]; }

/* the tiling enums of the kernels and the plan of tree_hist: out = tile, n_tiles, blocks[4], chunk_off[5], workgroups */
int tree_emu_threads(void) { return TREE_THREADS; }
int tree_emu_bin_rows(void) { return TREE_BIN_ROWS; }
int tree_emu_lds_cols(void) { return TREE_LDS_COLS; }
int tree_emu_chunk(void) { return TREE_CHUNK; }
int tree_emu_max_chunks(void) { return TREE_MAX_CHUNKS; }
int tree_emu_fold_ahead(void) { return TREE_FOLD_AHEAD; }
int tree_emu_fold_threads(void) { return TREE_FOLD_THREADS; }
void tree_emu_hist_plan(int w, int h, int n_pics, int F, int level, int *out)
{
  const TreeHistPlan P = tree_hist_plan(maps_geom(w, h, 0, nullptr), n_pics, F, level);
  out[0] = P.tile; out[1] = P.n_tiles;
  for (int d = 0; d < 4; d++) out[2 + d] = P.blocks[d];
  for (int d = 0; d < 5; d++) out[6 + d] = P.chunk_off[d];
  out[11] = tree_hist_groups(P);
}

int tree_emu_edges_check(const float *edges, int sets) { return tree_edges_check(edges, sets, g_err); }

/* mirrors fcu_feature_bins for w x h pictures */
int tree_emu_bins(int w, int h, int n_pics, int sets, const float *features, const float *edges, uint8_t *bins)
{
  const MapsGeom G = maps_geom(w, h, 0, nullptr);
  const int rc = feature_bins_args_check(n_pics, sets, features, edges, bins, G.lvl_off[4], g_err);
  if (rc != FCU_OK) return rc;
  const TreePlan P = tree_plan(G, TREE_BIN_ROWS);
  static TreeBinLds L;
  for (unsigned pic = 0; pic < (unsigned)n_pics; pic++) for (unsigned g = 0; g < (unsigned)P.wg_off[4]; g++) {
    blockIdx.x = g; blockIdx.y = pic;
    memset((void *)&L, 0xee, sizeof(L));
    for (unsigned t = 0; t < TREE_THREADS; t++) { threadIdx.x = t; feat_bins_phase<1>(L, features, edges, bins, G, P, feature_count(sets)); }
    for (unsigned t = 0; t < TREE_THREADS; t++) { threadIdx.x = t; feat_bins_phase<2>(L, features, edges, bins, G, P, feature_count(sets)); }
  }
  return FCU_OK;
}

/* mirrors fcu_tree_keys */
int tree_emu_keys(int w, int h, int n_pics, int sets, const uint8_t *bins, const fcu_key_tree *tree, int levels, uint16_t *keys)
{
  const MapsGeom G = maps_geom(w, h, 0, nullptr);
  const int rc = tree_keys_args_check(n_pics, sets, bins, tree, levels, keys, G.lvl_off[4], g_err);
  if (rc != FCU_OK) return rc;
  const int F = feature_count(sets);
  std::vector<const uint8_t *> p((size_t)n_pics);
  for (int i = 0; i < n_pics; i++) p[i] = bins + (size_t)i * (size_t)G.lvl_off[4] * (size_t)F;
  run_keys(G, n_pics, F, p.data(), tree, levels, keys);
  return FCU_OK;
}

/* mirrors fcu_tree_hist */
int tree_emu_hist(int w, int h, int n_pics, int sets, int level, const fcu_cu_trace *const *trace, const uint8_t *const *bins, const uint16_t *const *nodes,
                  int64_t *risk, uint32_t *count, int accumulate, uint32_t *dropped)
{
  const MapsGeom G = maps_geom(w, h, 0, nullptr);
  const int rc = tree_hist_args_check(n_pics, sets, level, trace, bins, nodes, risk, count, accumulate, G.lvl_off[4], g_err);
  if (rc != FCU_OK) return rc;
  run_hist(G, n_pics, feature_count(sets), level, trace, bins, nodes, risk, count, accumulate, dropped);
  return FCU_OK;
}

/* fcu_tree_split */
int tree_emu_split(const int64_t *risk, const uint32_t *count, int F, int level, int min_count, fcu_key_tree *tree) { return tree_split(risk, count, F, level, min_count, tree, g_err); }

/* mirrors fcu_tree_train: per level keys, histograms, split */
int tree_emu_train(int w, int h, int n_pics, int sets, int levels, int min_count, const fcu_cu_trace *const *trace, const uint8_t *const *bins, fcu_key_tree *tree)
{
  const MapsGeom G = maps_geom(w, h, 0, nullptr);
  int rc = tree_train_args_check(n_pics, sets, levels, min_count, trace, bins, tree, G.lvl_off[4], g_err);
  if (rc != FCU_OK) return rc;
  const int F = feature_count(sets);
  std::vector<uint16_t> keys((size_t)n_pics * (size_t)G.lvl_off[4], (uint16_t)0x7777);
  std::vector<const uint16_t *> nodes((size_t)n_pics);
  for (int i = 0; i < n_pics; i++) nodes[i] = keys.data() + (size_t)i * (size_t)G.lvl_off[4];
  tree_clear(*tree, levels);
  for (int l = 0; l < levels; l++) {
    const size_t cells = (size_t)tree_hist_cells(F, l);
    std::vector<int64_t> risk(cells, (int64_t)0x7777777777777777ll); std::vector<uint32_t> count(cells, 0x77777777u);
    if (l > 0) run_keys(G, n_pics, F, bins, tree, l, keys.data());
    run_hist(G, n_pics, F, l, trace, bins, l > 0 ? nodes.data() : nullptr, risk.data(), count.data(), 0, nullptr);
    rc = tree_split(risk.data(), count.data(), F, l, min_count, tree, g_err);
    if (rc != FCU_OK) return rc;
  }
  return FCU_OK;
}
}
