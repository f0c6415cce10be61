/*
 * fcu_features.h -- the fork's per-CU model inputs formed on the device from the luma plane (fcu_feature_maps; definition, columns
 * and reference lines: include/fcu.h): the 5 x 26 TMV texture statistics of getTMVFeature (tools_YS.cpp:1682-1839) and the
 * outlier-coefficient sums SOC of FormFeatureVector (tools_YS.cpp:379-396) on the Outlier plane of getOutlierWithDCT
 * (TEncSlice.cpp:1057-1132), one row of F floats per block of the label / N_OBF maps (fcu_maps.h).
 * Included by fcu_kernels.hip only (and by the test-only CPU build tests/emu/features_emu.cpp).
 *
 *   feat_ctu    one 256-thread workgroup per (CTU, picture).  The CTU's 64 x 64 luma goes once from HBM into LDS (8-byte loads when
 *               the plane starts on 8 bytes, byte loads otherwise; samples outside the picture are zeros), with a one-sample halo
 *               so that no tile looks outside the array; rows are 72 bytes apart: the 32 lanes of a half wave read 32 banks.
 *   lanes       thread t owns the 4 x 4 samples of partition t in z-order (k_z2r) -- one DCT block -- and keeps them with their
 *               neighbours (6 x 6) in registers.  In z-order the tiles of a CU are consecutive threads at every level: 4 threads are a
 *               depth-3 CU (each thread one quadrant of it), 16 a depth-2 CU, 64 -- one wave -- a depth-1 CU and a quadrant of the
 *               depth-0 CU.  No level serialises: every level is the same three steps over all 256 threads,
 *                 sums   per filter the tile's sum and its share of the four triangles, the level's one-sample ring zeroed, added up
 *                        over the lanes of one QUADRANT of the CU (1, 4, 16 or 64 lanes: DPP adds, no LDS) into one LDS word;
 *                 abs    the tile again against the sums of the CU's whole, its row half, column half and quadrant:
 *                        sum |q N - S| >> log2 N, added up the same way;
 *                 store  item i of the level = (CU i / F, column i % F): up to four LDS words added, one int -> float conversion, one
 *                        exact scale (ldexp), one dword store.  Consecutive threads store consecutive floats of a row.
 *               The depth-0 CU is thus reduced by the whole workgroup: four waves leave four quadrant words, the store step adds them.
 *   integers    every divisor is a power of two (N = W^2, W^2/2, W^2/4): trunc(q - S/N) = trunc((q N - S) / N), so
 *               |trunc(q - S/N)| = |q N - S| >> log2 N, and |q N| < 2^20.  No floating-point operation can round: a mean is an
 *               integer below 2^24 times a power of two, and so is every sum of absolute values.
 *   triangles   the fork assigns (not adds) in its triangle loops, whose last element lies on the zero ring: the "variance" is
 *               |trunc(0 - mean)| / (W^2/2) = (|S_T| >> log2(W^2/2)) / (W^2/2).
 *   SOC         the thread's tile is one 4x4 DCT block: obf_dct4 + obf_outlier (fcu_obf.h, the functions of obf_count), |coef| / 100
 *               of the outliers summed over the four lanes of a depth-3 CU into LDS; a CU of level d adds its 4^(3-d) words.
 * Every output element -- the zero rows of the blocks the picture cuts included -- is written by exactly one thread; no atomics,
 * nothing to clear: the same input gives the same bytes.
 * Algorithmic bytes per picture: W H read, NL F 4 written (4K, both sets: 8.3 MB read, 101 MB written).
 */
#pragma once
#include "fcu_obf.h"
#include "fcu_maps.h"

namespace fcu {

enum { FEAT_THREADS = 256, FEAT_ROWS = 66, FEAT_STRIDE = 72, FEAT_FILTERS = 5, FEAT_K = 26,
       FEAT_SUM = 0, FEAT_TRI = 1 /* .. 4 */, FEAT_ABS_WHOLE = 5, FEAT_ABS_ROWS = 6, FEAT_ABS_COLS = 7, FEAT_ABS_QUAD = 8, FEAT_KINDS = 9 };
static_assert(FEAT_FILTERS * FEAT_K == FCU_FEAT_TMV, "columns of the TMV set");

struct FeatPic { const uint8_t *y; int thr[16]; };             /* one picture of a batch (device copy): luma, obf_thr(Yc) */

struct FeatLds {
  alignas(16) uint8_t y[FEAT_ROWS][FEAT_STRIDE];               /* sample (X, Y) of the CTU at y[Y + 1][X + 4] */
  int part[FEAT_FILTERS][FEAT_KINDS][FCU_NPART];               /* [filter][FEAT_*][quadrant = node of level d + 1] */
  int soc[16][64];                                             /* [coefficient][CU of level 3] */
};

/* column k of a filter = the sum of the words `mask` names (bit n: quadrant n = TL, TR, BL, BR) of kind `kind`, over
 * N >> dsh elements; tri: the triangle "variance".  k = 20 / 24 are the fork's, not a quadrant: its third "quadrant" runs over all
 * columns of the bottom rows (tools_YS.cpp:1823-1825), so they repeat k = 3 / 5. */
#define FEAT_RULE(kind, mask, dsh, tri) (uint16_t)((kind) | ((mask) << 4) | ((dsh) << 8) | ((tri) << 10))
FCU_TABLE uint16_t k_feat_rule[FEAT_K] = {
  FEAT_RULE(FEAT_SUM, 15, 0, 0), FEAT_RULE(FEAT_ABS_WHOLE, 15, 0, 0),
  FEAT_RULE(FEAT_SUM, 3, 1, 0), FEAT_RULE(FEAT_SUM, 12, 1, 0), FEAT_RULE(FEAT_ABS_ROWS, 3, 1, 0), FEAT_RULE(FEAT_ABS_ROWS, 12, 1, 0),
  FEAT_RULE(FEAT_SUM, 5, 1, 0), FEAT_RULE(FEAT_SUM, 10, 1, 0), FEAT_RULE(FEAT_ABS_COLS, 5, 1, 0), FEAT_RULE(FEAT_ABS_COLS, 10, 1, 0),
  FEAT_RULE(FEAT_TRI + 0, 15, 1, 0), FEAT_RULE(FEAT_TRI + 1, 15, 1, 0), FEAT_RULE(FEAT_TRI + 0, 15, 1, 1), FEAT_RULE(FEAT_TRI + 1, 15, 1, 1),
  FEAT_RULE(FEAT_TRI + 2, 15, 1, 0), FEAT_RULE(FEAT_TRI + 3, 15, 1, 0), FEAT_RULE(FEAT_TRI + 2, 15, 1, 1), FEAT_RULE(FEAT_TRI + 3, 15, 1, 1),
  FEAT_RULE(FEAT_SUM, 1, 2, 0), FEAT_RULE(FEAT_SUM, 2, 2, 0), FEAT_RULE(FEAT_SUM, 12, 1, 0), FEAT_RULE(FEAT_SUM, 8, 2, 0),
  FEAT_RULE(FEAT_ABS_QUAD, 1, 2, 0), FEAT_RULE(FEAT_ABS_QUAD, 2, 2, 0), FEAT_RULE(FEAT_ABS_ROWS, 12, 1, 0), FEAT_RULE(FEAT_ABS_QUAD, 8, 2, 0) };
#undef FEAT_RULE

__device__ static inline uint32_t feat_ldw(const uint8_t *p)
{
  uint32_t v;
  __builtin_memcpy(&v, __builtin_assume_aligned(p, 4), 4);
  return v;
}
__device__ static inline void feat_stw(uint8_t *p, uint32_t v) { __builtin_memcpy(__builtin_assume_aligned(p, 4), &v, 4); }

/* v added up over the G consecutive lanes t belongs to (G = 1, 4, 16, 64) into slot[t / G].  All lanes call it, outside divergent
 * code.  The CPU build runs the threads one after the other: the first of a group sets the word, the others add to it. */
template <int G>
__device__ static inline void feat_group_put(int *slot, int t, int v)
{
  static_assert(G == 1 || G == 4 || G == 16 || G == 64, "quadrants of a CU in z-order");
#ifdef FCU_EMU
  if ((t & (G - 1)) == 0) slot[t / G] = v; else slot[t / G] += v;
#else
  if constexpr (G == 64) v = (int)fcu_wave_sum((uint32_t)v);
  else if constexpr (G > 1) {
    v += __builtin_amdgcn_update_dpp(0, v, 0xb1, 0xf, 0xf, false);      /* quad_perm:[1,0,3,2] */
    v += __builtin_amdgcn_update_dpp(0, v, 0x4e, 0xf, 0xf, false);      /* quad_perm:[2,3,0,1]: every lane of a quad holds its sum */
    if constexpr (G == 16) {
      v += __builtin_amdgcn_update_dpp(0, v, 0x124, 0xf, 0xf, false);   /* row_ror:4 */
      v += __builtin_amdgcn_update_dpp(0, v, 0x128, 0xf, 0xf, false);   /* row_ror:8: every lane of a row holds the row's sum */
    }
  }
  if ((t & (G - 1)) == 0) slot[t / G] = v;
#endif
}

/* the thread's 4 x 4 samples with their neighbours: p[r + 1][c + 1] = sample (4 tx + c, 4 ty + r) of the CTU */
struct FeatTile { int p[6][6]; int tx, ty; };
__device__ static inline FeatTile feat_tile(const FeatLds &L, int t)
{
  FeatTile T;
  const int r = k_z2r[t];
  T.tx = r & 15; T.ty = r >> 4;
#pragma unroll
  for (int rr = 0; rr < 6; rr++) {
    const uint8_t *row = &L.y[4 * T.ty + rr][4 * T.tx];
    const uint32_t a = feat_ldw(row), b = feat_ldw(row + 4), c = feat_ldw(row + 8);
    T.p[rr][0] = (int)(a >> 24); T.p[rr][1] = (int)(b & 255u); T.p[rr][2] = (int)((b >> 8) & 255u);
    T.p[rr][3] = (int)((b >> 16) & 255u); T.p[rr][4] = (int)(b >> 24); T.p[rr][5] = (int)(c & 255u);
  }
  return T;
}
/* filter f at sample (r, c) of the tile: the masks of getTMVFeature (tools_YS.cpp:1693-1697) as T3x3Filter::filter applies them */
__device__ static inline int feat_q(const FeatTile &T, int f, int r, int c)
{
  switch (f) {
  case 0: return T.p[r + 1][c + 1];
  case 1: return T.p[r + 1][c] - T.p[r + 1][c + 2];
  case 2: return T.p[r][c + 1] - T.p[r + 2][c + 1];
  case 3: return T.p[r][c + 2] - T.p[r + 2][c];
  default: return T.p[r][c] - T.p[r + 2][c + 2];
  }
}
__device__ static inline int feat_abs(int v) { return v < 0 ? -v : v; }

/* step "sums" of level D */
template <int D>
__device__ static inline void feat_sum_pass(FeatLds &L, int t)
{
  constexpr int W = 64 >> D, GQ = 1 << (2 * (3 - D));
  const FeatTile T = feat_tile(L, t);
  const int i0 = (4 * T.ty) & (W - 1), j0 = (4 * T.tx) & (W - 1);
#pragma unroll
  for (int f = 0; f < FEAT_FILTERS; f++) {
    int s = 0, tri[4] = { 0, 0, 0, 0 };
#pragma unroll
    for (int r = 0; r < 4; r++) {
#pragma unroll
      for (int c = 0; c < 4; c++) {
        const int i = i0 + r, j = j0 + c;
        const bool ring = i == 0 || i == W - 1 || j == 0 || j == W - 1;   /* the ring of THIS CU, identity filter included (:1659-1672) */
        const int v = ring ? 0 : feat_q(T, f, r, c);
        s += v;
        tri[0] += i + j <= W - 1 ? v : 0;                      /* j < W - i       (:1749) */
        tri[1] += i + j >= W - 1 ? v : 0;                      /* j >= W - i - 1  (:1766) */
        tri[2] += j >= i ? v : 0;                              /* (:1784) */
        tri[3] += j <= i ? v : 0;                              /* j < i + 1       (:1801) */
      }
    }
    feat_group_put<GQ>(L.part[f][FEAT_SUM], t, s);
#pragma unroll
    for (int k = 0; k < 4; k++) feat_group_put<GQ>(L.part[f][FEAT_TRI + k], t, tri[k]);
  }
}

/* step "abs" of level D: getSubBlockVariance (tools_YS.h:116-126) of the four rectangles the tile lies in */
template <int D>
__device__ static inline void feat_abs_pass(FeatLds &L, int t)
{
  constexpr int W = 64 >> D, GQ = 1 << (2 * (3 - D)), LG = 2 * (6 - D);
  const FeatTile T = feat_tile(L, t);
  const int i0 = (4 * T.ty) & (W - 1), j0 = (4 * T.tx) & (W - 1);
  const int quad = t / GQ, mine = quad & 3, first = quad & ~3;
#pragma unroll
  for (int f = 0; f < FEAT_FILTERS; f++) {
    const int *Q = &L.part[f][FEAT_SUM][first];
    const int q0 = Q[0], q1 = Q[1], q2 = Q[2], q3 = Q[3];
    const int sw = q0 + q1 + q2 + q3, sr = mine < 2 ? q0 + q1 : q2 + q3, sc = (mine & 1) ? q1 + q3 : q0 + q2;
    const int sq = mine == 0 ? q0 : (mine == 1 ? q1 : (mine == 2 ? q2 : q3));
    int aw = 0, ar = 0, ac = 0, aq = 0;
#pragma unroll
    for (int r = 0; r < 4; r++) {
#pragma unroll
      for (int c = 0; c < 4; c++) {
        const int i = i0 + r, j = j0 + c;
        const bool ring = i == 0 || i == W - 1 || j == 0 || j == W - 1;
        const int v = ring ? 0 : feat_q(T, f, r, c);
        aw += feat_abs(v * (1 << LG) - sw) >> LG;
        ar += feat_abs(v * (1 << (LG - 1)) - sr) >> (LG - 1);
        ac += feat_abs(v * (1 << (LG - 1)) - sc) >> (LG - 1);
        aq += feat_abs(v * (1 << (LG - 2)) - sq) >> (LG - 2);
      }
    }
    feat_group_put<GQ>(L.part[f][FEAT_ABS_WHOLE], t, aw);
    feat_group_put<GQ>(L.part[f][FEAT_ABS_ROWS], t, ar);
    feat_group_put<GQ>(L.part[f][FEAT_ABS_COLS], t, ac);
    feat_group_put<GQ>(L.part[f][FEAT_ABS_QUAD], t, aq);
  }
}

/* the outlier coefficients of the thread's DCT block: |coef| / 100 where obf_count would count the coefficient */
__device__ static inline void feat_soc_pass(FeatLds &L, const FeatPic &P, int t)
{
  const int r = k_z2r[t], tx = r & 15, ty = r >> 4;
  uint32_t rows[4];
#pragma unroll
  for (int y = 0; y < 4; y++) rows[y] = feat_ldw(&L.y[4 * ty + 1 + y][4 * tx + 4]);
  int coef[16];
  obf_dct4(rows, coef);
  const FCU_HBM int *thr = (const FCU_HBM int *)P.thr;
#pragma unroll
  for (int k = 1; k < 16; k++) feat_group_put<4>(L.soc[k], t, obf_outlier(coef[k], thr[k]) ? feat_abs(coef[k]) / 100 : 0);
}

/* column col (f * 26 + k) of CU cu of level D from the words of the level */
template <int D>
__device__ static inline float feat_tmv_value(const FeatLds &L, int cu, int col)
{
  constexpr int LG = 2 * (6 - D);
  const int f = col / FEAT_K, rule = k_feat_rule[col - f * FEAT_K];
  const int *w = &L.part[f][rule & 15][4 * cu];
  int num = 0;
#pragma unroll
  for (int n = 0; n < 4; n++) if (rule & (16 << n)) num += w[n];
  const int sh = LG - ((rule >> 8) & 3);
  if (rule & (1 << 10)) num = feat_abs(num) >> sh;
  return __builtin_ldexpf((float)num, -sh);
}
template <int D>
__device__ static inline float feat_soc_value(const FeatLds &L, int cu, int k)
{
  constexpr int N = 1 << (2 * (3 - D));
  if (k == 0) return 0.0f;                                     /* DC is no outlier (StartFreq 1, TEncSlice.cpp:987) */
  int s = 0;
  for (int m = 0; m < N; m++) s += L.soc[k][cu * N + m];
  return (float)s;
}

/* step "store" of level D: the rows of the level's CUs; zeros for a block the picture cuts (!bBoundary, TEncCu.cpp:1525) */
template <int SETS, int D>
__device__ static inline void feat_store_level(const FeatLds &L, float *out, const MapsGeom &G, int cx, int cy, int t)
{
  constexpr int F = ((SETS & FCU_FEATSET_TMV) ? FCU_FEAT_TMV : 0) + ((SETS & FCU_FEATSET_SOC) ? FCU_FEAT_SOC : 0);
  constexpr int NCU = 1 << (2 * D), NODE0 = D == 0 ? 0 : (D == 1 ? 1 : (D == 2 ? 5 : 21));
  for (int i = t; i < NCU * F; i += FEAT_THREADS) {
    const int cu = i / F, col = i - cu * F;
    const MapsPlace P = maps_place(G, maps_node(NODE0 + cu), cx, cy);
    if (!P.exists) continue;
    float v = 0.0f;
    if (P.whole) {
      if ((SETS & FCU_FEATSET_TMV) && col < FCU_FEAT_TMV) v = feat_tmv_value<D>(L, cu, col);
      else v = feat_soc_value<D>(L, cu, col - ((SETS & FCU_FEATSET_TMV) ? FCU_FEAT_TMV : 0));
    }
    ((FCU_HBM float *)out)[(size_t)P.idx * F + col] = v;        /* idx < lvl_off[4]: inside the picture's NL rows */
  }
}

/* 8 bytes of the plane, which is known to be ALIGN-aligned (1: nothing is known) */
typedef uint32_t FeatVec2 __attribute__((vector_size(8)));
template <int ALIGN>
__device__ static inline void feat_load8(uint32_t *w, const uint8_t *p)
{
  if constexpr (ALIGN == 8) {
    const FeatVec2 v = *(const FCU_HBM FeatVec2 *)p;
    w[0] = v[0]; w[1] = v[1];
  } else {
    uint32_t b[8];
#pragma unroll
    for (int k = 0; k < 8; k++) b[k] = ((const FCU_HBM uint8_t *)p)[k];
    w[0] = b[0] | (b[1] << 8) | (b[2] << 16) | (b[3] << 24);
    w[1] = b[4] | (b[5] << 8) | (b[6] << 16) | (b[7] << 24);
  }
}

/* ---- feat_ctu: phase 0 fills the luma tile; level D = 0..3 is phases 1 + 3 D (sums; at D = 0 also the SOC words), 2 + 3 D (abs)
 * and 3 + 3 D (store).  A barrier lies between two phases; without the TMV set the sums and abs phases of D > 0 are empty. */
template <int SETS, int PHASE>
__device__ static inline void feat_ctu_phase(FeatLds &L, const FeatPic *pics, float *out, const MapsGeom &G)
{
  constexpr int F = ((SETS & FCU_FEATSET_TMV) ? FCU_FEAT_TMV : 0) + ((SETS & FCU_FEATSET_SOC) ? FCU_FEAT_SOC : 0);
  const int t = (int)threadIdx.x, a = (int)blockIdx.x, pic = (int)blockIdx.y;
  const int cx = a % G.w_ctu, cy = a / G.w_ctu;
  if constexpr (PHASE == 0) {
    const uint8_t *plane = pics[pic].y;
    const int row = t >> 2, seg = t & 3, gy = cy * 64 + row, gx = cx * 64 + 16 * seg;
    uint32_t w[4] = { 0u, 0u, 0u, 0u };
    if (gy < G.height) {
      const uint8_t *p = plane + (size_t)gy * G.width + gx;
      /* the width is a multiple of 8: a unit of 8 samples lies inside the picture or outside it */
      if (((uintptr_t)plane & 7) == 0) {
        if (gx < G.width) feat_load8<8>(&w[0], p);
        if (gx + 8 < G.width) feat_load8<8>(&w[2], p + 8);
      } else {
        if (gx < G.width) feat_load8<1>(&w[0], p);
        if (gx + 8 < G.width) feat_load8<1>(&w[2], p + 8);
      }
    }
    uint8_t *dst = &L.y[row + 1][4 + 16 * seg];
#pragma unroll
    for (int k = 0; k < 4; k++) feat_stw(dst + 4 * k, w[k]);
    if (seg == 0) feat_stw(&L.y[row + 1][0], 0u);              /* the halo: read by the tiles on the CTU's ring, whose filters are zeroed */
    if (seg == 3) feat_stw(&L.y[row + 1][FEAT_STRIDE - 4], 0u);
    if (t < 2 * (FEAT_STRIDE / 4)) feat_stw(&L.y[t < FEAT_STRIDE / 4 ? 0 : FEAT_ROWS - 1][4 * (t % (FEAT_STRIDE / 4))], 0u);
  } else {
    constexpr int D = (PHASE - 1) / 3, STEP = (PHASE - 1) % 3;
    if constexpr (STEP == 0) {
      if constexpr ((SETS & FCU_FEATSET_SOC) != 0 && D == 0) feat_soc_pass(L, pics[pic], t);
      if constexpr ((SETS & FCU_FEATSET_TMV) != 0) feat_sum_pass<D>(L, t);
    } else if constexpr (STEP == 1) {
      if constexpr ((SETS & FCU_FEATSET_TMV) != 0) feat_abs_pass<D>(L, t);
    } else feat_store_level<SETS, D>(L, out + (size_t)pic * (size_t)G.lvl_off[4] * F, G, cx, cy, t);
  }
}

#ifndef FCU_EMU
template <int SETS>
__global__ void __launch_bounds__(FEAT_THREADS) feat_ctu(const FeatPic *pics, float *out, const MapsGeom G)
{
  __shared__ FeatLds L;
  feat_ctu_phase<SETS, 0>(L, pics, out, G);
  __syncthreads();
  if constexpr ((SETS & FCU_FEATSET_TMV) != 0) {
    feat_ctu_phase<SETS, 1>(L, pics, out, G); __syncthreads();
    feat_ctu_phase<SETS, 2>(L, pics, out, G); __syncthreads();
    feat_ctu_phase<SETS, 3>(L, pics, out, G); __syncthreads();   /* (the next level's sums take the words this store read) */
    feat_ctu_phase<SETS, 4>(L, pics, out, G); __syncthreads();
    feat_ctu_phase<SETS, 5>(L, pics, out, G); __syncthreads();
    feat_ctu_phase<SETS, 6>(L, pics, out, G); __syncthreads();
    feat_ctu_phase<SETS, 7>(L, pics, out, G); __syncthreads();
    feat_ctu_phase<SETS, 8>(L, pics, out, G); __syncthreads();
    feat_ctu_phase<SETS, 9>(L, pics, out, G); __syncthreads();
    feat_ctu_phase<SETS, 10>(L, pics, out, G); __syncthreads();
    feat_ctu_phase<SETS, 11>(L, pics, out, G); __syncthreads();
    feat_ctu_phase<SETS, 12>(L, pics, out, G);
  } else {                                                     /* SOC alone: one pass, then every level stores from the same words */
    feat_ctu_phase<SETS, 1>(L, pics, out, G); __syncthreads();
    feat_ctu_phase<SETS, 3>(L, pics, out, G);
    feat_ctu_phase<SETS, 6>(L, pics, out, G);
    feat_ctu_phase<SETS, 9>(L, pics, out, G);
    feat_ctu_phase<SETS, 12>(L, pics, out, G);
  }
}
#endif

} /* namespace fcu */
