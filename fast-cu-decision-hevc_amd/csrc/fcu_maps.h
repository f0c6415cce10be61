/*
 * fcu_maps.h -- the decision of whole pictures as rasters, and the agreement of two decisions, formed on the device from the
 * fcu_ctu_out records (fcu_decision_maps, fcu_split_match; shapes, label codes and records: include/fcu.h).
 * Included by fcu_kernels.hip only (and by the test-only CPU build tests/emu/maps_emu.cpp).
 *
 *   maps_ctu    one 256-thread workgroup per (CTU, picture).  Thread z reads entry z of every requested 256-byte array of the
 *               record's head -- one coalesced 256-byte row per array, four loads in flight -- and writes it to raster position
 *               k_z2r[z] of the array's 16 x 16 tile in LDS; the vectors of `mv` go the same way.  After one barrier the tiles leave
 *               as rows of the picture-wide maps.  Two store paths, chosen by the host per batch (maps_row_align):
 *                 UNIT 16  a tile row of a byte map is one 16-byte store, a row of the motion tile four; needs W4 a multiple of 16
 *                          (then no CTU is cut in x) and 16-byte aligned bases;
 *                 UNIT 2   2-byte units of a byte map (W4 is even, so a cut CTU ends on a unit), one vector per store in the motion
 *                          map; right for any base address (an odd one makes the unit two byte stores).
 *               A cut CTU stores only its columns and rows inside the picture, so what the engine left in entries outside never
 *               reaches an output; inside / outside is geometry (k_z2r), never a value read.
 *               Labels and N_OBF: thread t < 85 owns node t of the CTU's quadtree (1 + 4 + 16 + 64 blocks of level 0..3, each level
 *               in z-order: node j of level d starts at partition j << (8 - 2d)).  Its label comes from depth / part_size of that
 *               partition, read directly.  N_OBF: thread z leaves "partition z lies inside the picture and its OBF count is > 0"
 *               in LDS; level 3 sums four flags, every level above four sums of the level below (a barrier between levels).
 *               The labels are those of the CUs ON THE CHOSEN TREE: the record holds one depth per partition, the result of the
 *               search.  The fork's Training dump also labels the CUs the search visited and discarded; those are not recorded.
 *   match_ctu   one 256-thread workgroup per (CTU, picture): depth of A and B as two coalesced rows, the node labels as above;
 *               every counter is one wave ballot + popcount, the four waves meet in LDS, threads 0..15 store one dword of the
 *               64-byte record each.
 *   match_pic   one 256-thread workgroup per picture folds the CTU records as report_pic does: 64-bit sums, no atomics.
 *   labels_ctu  the inverse of the label half of maps_ctu (fcu_labels_from_rasters): the picture-wide depth / part_size rasters in,
 *               the label array out.  One wave per CTU, four CTUs per 256-thread workgroup, no LDS and no barrier: lane l owns node
 *               21 + l of the CTU's quadtree (the 64 blocks of level 3) and, l < 21, node l (levels 0..2) as well.  A node reads
 *               the raster byte(s) at its top-left partition -- byte loads, right at any base address and any W4; the two or four
 *               loads of a lane are issued before the first is used -- and stores its one label byte.  The label rule is
 *               maps_label, shared with maps_ctu, so the maps of a decided picture give back the labels maps_ctu wrote.
 * Every output byte is written by exactly one thread; nothing must be cleared beforehand: a repeated call gives identical bytes.
 * Algorithmic bytes per picture: 256 B per CTU and requested array (1 024 B for mv; depth and part_size for the labels when they
 * are not among the arrays: two more rows, of which 85 + 64 bytes are used; 2 B per partition of the OBF map) + the map bytes
 * written.  Split match: 2 x 512 B per CTU + 64 B per CTU written and read back.  Labels from rasters: 85 B of the depth raster and
 * 64 B of the part_size raster read per whole CTU, 85 B written.
 */
#pragma once
#include "fcu_report.h"

namespace fcu {

enum { LABELS_THREADS = 256, LABELS_CTUS = LABELS_THREADS / 64 };      /* labels_ctu: one wave per CTU */
enum { MAPS_THREADS = 256, MAPS_NODES = 85, MATCH_COUNTERS = 26, MATCH_CTU_WORDS = 16, MATCH_PIC_AHEAD = 8, MAPS_SIZE_NXN = 3 };
static_assert(sizeof(fcu_ctu_match) == 4 * MATCH_CTU_WORDS && sizeof(fcu_pic_match) == 8 * MATCH_COUNTERS && MATCH_COUNTERS <= 2 * MATCH_CTU_WORDS,
              "record layouts the word-wise stores rely on");

struct MapsPic { const fcu_ctu_out *out; const int16_t *obf; };       /* one picture of a batch (device copy) */
struct MapsOut { uint8_t *bytes; int16_t *mv; int8_t *labels; uint16_t *nobf; };
struct MatchPic { const fcu_ctu_out *a, *b; };

struct MapsLds {
  alignas(16) uint8_t tile[FCU_MAP_FIELDS][FCU_NPART];     /* raster */
  alignas(16) int16_t mv[FCU_NPART][2];                    /* raster */
  uint16_t flag[FCU_NPART];                                /* z-order: inside the picture and OBF count > 0 */
  uint16_t sum[4][64];                                     /* N_OBF of level d, node j */
};

/* node t < MAPS_NODES of a CTU's quadtree: its level, its number inside the level (z-order), its first partition (z-order) and
 * that partition's position inside the CTU in units of 4 samples */
struct MapsNode { int d, j, z0, px, py; };
__device__ static inline MapsNode maps_node(int t)
{
  const int d = t == 0 ? 0 : (t < 5 ? 1 : (t < 21 ? 2 : 3));
  const int j = t - (d == 0 ? 0 : (d == 1 ? 1 : (d == 2 ? 5 : 21)));
  const int z0 = j << (8 - 2 * d), r = k_z2r[z0];
  return MapsNode{ d, j, z0, r & 15, r >> 4 };
}
/* where the node lies in the picture: `exists` = its top-left sample is inside, `whole` = all of it is; idx = its element in the
 * picture's label / N_OBF maps */
struct MapsPlace { bool exists, whole; int idx; };
__device__ static inline MapsPlace maps_place(const MapsGeom &G, const MapsNode &N, int cx, int cy)
{
  const int s = 64 >> N.d, x = cx * 64 + 4 * N.px, y = cy * 64 + 4 * N.py;
  MapsPlace P;
  P.exists = x < G.width && y < G.height;
  P.whole = x + s <= G.width && y + s <= G.height;
  P.idx = G.lvl_off[N.d] + ((cy << N.d) + (N.py >> (4 - N.d))) * G.lvl_w[N.d] + (cx << N.d) + (N.px >> (4 - N.d));
  return P;
}
/* FCU_LABEL_* of a node of level d whose first partition has this depth and part_size */
__device__ static inline int maps_label(int d, int depth, int part_size, bool whole)
{
  if (depth < d) return FCU_LABEL_ABSENT;
  if (d < 3 && !whole) return FCU_LABEL_FORCED;
  return (d < 3 ? depth > d : part_size == MAPS_SIZE_NXN) ? FCU_LABEL_SPLIT : FCU_LABEL_NOT_SPLIT;
}
__device__ static inline int maps_node_label(const FCU_HBM fcu_ctu_out &O, const MapsNode &N, bool whole)
{
  return maps_label(N.d, O.depth[N.z0], O.part_size[N.z0], whole);
}

/* N bytes from LDS to dst in HBM, which is known to be ALIGN-aligned (1: nothing is known): one 16-byte store, or 2-byte
 * stores, or byte stores */
typedef uint32_t MapsVec4 __attribute__((vector_size(16)));
template <int N, int ALIGN>
__device__ static inline void maps_put(void *dst, const void *src)
{
  static_assert((N == 16 && ALIGN == 16) || (N < 16 && N % 2 == 0 && ALIGN <= 2), "the units of the two store paths");
  if constexpr (N == 16) {
    MapsVec4 v;
    __builtin_memcpy(&v, src, 16);
    *(FCU_HBM MapsVec4 *)dst = v;
  } else if constexpr (ALIGN == 2) {
    uint16_t v[N / 2];
    __builtin_memcpy(v, src, N);
#pragma unroll
    for (int k = 0; k < N / 2; k++) ((FCU_HBM uint16_t *)dst)[k] = v[k];
  } else {
    uint8_t v[N];
    __builtin_memcpy(v, src, N);
#pragma unroll
    for (int k = 0; k < N; k++) ((FCU_HBM uint8_t *)dst)[k] = v[k];
  }
}

/* what N_OBF counts: "partition (x4, y4) lies inside the picture and its count in the OBF map is > 0".  One definition, shared by
 * maps_ctu and by the kernel of fcu_nobf_maps (fcu_risk.h) */
__device__ static inline uint16_t maps_obf_flag(const int16_t *obf, int W4, int H4, int x4, int y4)
{
  const bool in = x4 < W4 && y4 < H4;
  return (uint16_t)(in && ((const FCU_HBM int16_t *)obf)[(size_t)y4 * W4 + x4] > 0 ? 1 : 0);
}

/* N_OBF of level D: node sums four values of the level below */
template <int D>
__device__ static inline void maps_nobf_level(MapsLds &L, const MapsGeom &G, uint16_t *nobf, int cx, int cy, int t)
{
  if (t >= MAPS_NODES) return;
  const MapsNode N = maps_node(t);
  if (N.d != D) return;
  const uint16_t *c = D == 3 ? &L.flag[4 * N.j] : &L.sum[D == 3 ? 0 : D + 1][4 * N.j];
  const uint16_t s = (uint16_t)(c[0] + c[1] + c[2] + c[3]);
  L.sum[D][N.j] = s;
  const MapsPlace P = maps_place(G, N, cx, cy);
  if (P.exists) nobf[P.idx] = s;
}

/* ---- maps_ctu: phase 1 fills the tiles (and stores the labels), phase 2 stores the rows and level 3 of N_OBF, phases 3..5 the
 * levels 2..0 of N_OBF.  UNIT / ALIGN: the store path (header comment) */
template <int PHASE, int UNIT, int ALIGN>
__device__ static inline void maps_ctu_phase(MapsLds &L, const MapsPic *pics, const MapsOut Q, const MapsGeom &G)
{
  const int t = (int)threadIdx.x, a = (int)blockIdx.x, pic = (int)blockIdx.y;
  const int cx = a % G.w_ctu, cy = a / G.w_ctu, W4 = G.width >> 2, H4 = G.height >> 2;
  const MapsPic &P = pics[pic];
  const FCU_HBM fcu_ctu_out &O = *(const FCU_HBM fcu_ctu_out *)(P.out + a);
  const size_t lvl_all = (size_t)G.lvl_off[4];
  if (PHASE == 1) {
    const FCU_HBM uint8_t *head = (const FCU_HBM uint8_t *)&O;
    const int r = k_z2r[t];
    for (int f0 = 0; f0 < G.n_fields; f0 += 4) {             /* four rows in flight */
      uint8_t v[4];
#pragma unroll
      for (int k = 0; k < 4; k++) v[k] = f0 + k < G.n_fields ? head[G.field_off[f0 + k] + t] : (uint8_t)0;
#pragma unroll
      for (int k = 0; k < 4; k++) if (f0 + k < G.n_fields) L.tile[f0 + k][r] = v[k];
    }
    if (Q.mv) { const int16_t hor = O.mv[t][0], ver = O.mv[t][1]; L.mv[r][0] = hor; L.mv[r][1] = ver; }
    if (Q.nobf) {
      L.flag[t] = maps_obf_flag(P.obf, W4, H4, cx * 16 + (r & 15), cy * 16 + (r >> 4));
    }
    if (Q.labels && t < MAPS_NODES) {
      const MapsNode N = maps_node(t);
      const MapsPlace C = maps_place(G, N, cx, cy);
      if (C.exists) Q.labels[(size_t)pic * lvl_all + C.idx] = (int8_t)maps_node_label(O, N, C.whole);
    }
  } else if (PHASE == 2) {
    const int cw = W4 - cx * 16 < 16 ? W4 - cx * 16 : 16, ch = H4 - cy * 16 < 16 ? H4 - cy * 16 : 16;
    const size_t plane = (size_t)H4 * W4, org = (size_t)cy * 16 * W4 + (size_t)cx * 16;
    if (G.n_fields) {
      uint8_t *maps = Q.bytes + (size_t)pic * G.n_fields * plane + org;
      if constexpr (UNIT == 16) {                                /* unit = one row of one tile */
        for (int i = t; i < G.n_fields * 16; i += MAPS_THREADS) {
          const int f = i >> 4, row = i & 15;
          if (row < ch) maps_put<16, 16>(maps + (size_t)f * plane + (size_t)row * W4, &L.tile[f][row * 16]);
        }
      } else {                                               /* unit = two partitions of a row */
        for (int i = t; i < G.n_fields * 128; i += MAPS_THREADS) {
          const int f = i >> 7, row = (i >> 3) & 15, col = (i & 7) * 2;
          if (row < ch && col < cw) maps_put<2, ALIGN>(maps + (size_t)f * plane + (size_t)row * W4 + col, &L.tile[f][row * 16 + col]);
        }
      }
    }
    if (Q.mv) {
      int16_t *mv = Q.mv + 2 * ((size_t)pic * plane + org);
      if constexpr (UNIT == 16) {
        const int row = t >> 2, col = (t & 3) * 4;
        if (t < 64 && row < ch) maps_put<16, 16>(mv + 2 * ((size_t)row * W4 + col), &L.mv[row * 16 + col][0]);
      } else {
        const int row = t >> 4, col = t & 15;
        if (row < ch && col < cw) maps_put<4, 2>(mv + 2 * ((size_t)row * W4 + col), &L.mv[t][0]);
      }
    }
    if (Q.nobf) maps_nobf_level<3>(L, G, Q.nobf + (size_t)pic * lvl_all, cx, cy, t);
  } else if (PHASE == 3) maps_nobf_level<2>(L, G, Q.nobf + (size_t)pic * lvl_all, cx, cy, t);
  else if (PHASE == 4) maps_nobf_level<1>(L, G, Q.nobf + (size_t)pic * lvl_all, cx, cy, t);
  else maps_nobf_level<0>(L, G, Q.nobf + (size_t)pic * lvl_all, cx, cy, t);
}

/* ---- match_ctu: phase 1 fills the four waves' slots, phase 2 stores the record.  Slots: part_total, part_equal,
 * node[4][2][2], only_a[4], only_b[4] -- the order of both records */
template <int PHASE>
__device__ static inline void match_ctu_phase(uint32_t (*part)[MATCH_COUNTERS], const MatchPic *pics, fcu_ctu_match *ctu, const MapsGeom &G)
{
  const int t = (int)threadIdx.x, a = (int)blockIdx.x, pic = (int)blockIdx.y;
  if (PHASE == 1) {
    const int cx = a % G.w_ctu, cy = a / G.w_ctu;
    const FCU_HBM fcu_ctu_out &A = *(const FCU_HBM fcu_ctu_out *)(pics[pic].a + a), &B = *(const FCU_HBM fcu_ctu_out *)(pics[pic].b + a);
    uint32_t *W = part[t >> 6];
    const int r = k_z2r[t];
    const bool in = cx * 64 + 4 * (r & 15) < G.width && cy * 64 + 4 * (r >> 4) < G.height;
    const int da = A.depth[t], db = B.depth[t];
    report_wave_count(&W[0], in);
    report_wave_count(&W[1], in && da == db);
    const MapsNode N = maps_node(t < MAPS_NODES ? t : 0);
    const MapsPlace C = maps_place(G, N, cx, cy);
    const bool node = t < MAPS_NODES && C.exists;
    const int la = node ? maps_node_label(A, N, C.whole) : FCU_LABEL_FORCED, lb = node ? maps_node_label(B, N, C.whole) : FCU_LABEL_FORCED;
    const bool fa = la == FCU_LABEL_NOT_SPLIT || la == FCU_LABEL_SPLIT, fb = lb == FCU_LABEL_NOT_SPLIT || lb == FCU_LABEL_SPLIT;
#pragma unroll
    for (int d = 0; d < 4; d++) {
#pragma unroll
      for (int k = 0; k < 4; k++) report_wave_count(&W[2 + 4 * d + k], N.d == d && fa && fb && la == (k >> 1) && lb == (k & 1));
      report_wave_count(&W[18 + d], N.d == d && fa && lb == FCU_LABEL_ABSENT);
      report_wave_count(&W[22 + d], N.d == d && fb && la == FCU_LABEL_ABSENT);
    }
  } else if (t < MATCH_CTU_WORDS) {
    uint32_t w = 0;                                            /* dword t: counters 2t and 2t + 1; the last three dwords are `pad` */
    if (2 * t < MATCH_COUNTERS) {
      const int k = 2 * t;
      w = (part[0][k] + part[1][k] + part[2][k] + part[3][k]) | ((part[0][k + 1] + part[1][k + 1] + part[2][k + 1] + part[3][k + 1]) << 16);
    }
    ((uint32_t *)(ctu + (size_t)pic * G.n_ctu + a))[t] = w;
  }
}

/* ---- match_pic: phase 1 leaves every thread's partial sums in LDS, phase 2 stores the record */
struct MatchPicLds { uint64_t lo[MAPS_THREADS], hi[MAPS_THREADS]; };
template <int PHASE>
__device__ static inline void match_pic_phase(MatchPicLds &L, const fcu_ctu_match *ctu, fcu_pic_match *rec, int n_ctu)
{
  const int t = (int)threadIdx.x, pic = (int)blockIdx.x;
  if (PHASE == 1) {
    const uint32_t *w = (const uint32_t *)(ctu + (size_t)pic * n_ctu) + (t & 15);
    uint64_t lo = 0, hi = 0;
    /* MATCH_PIC_AHEAD loads in flight per thread: one workgroup walks the whole picture */
    for (int r0 = t >> 4; r0 < n_ctu; r0 += MATCH_PIC_AHEAD * (MAPS_THREADS / 16)) {
      uint32_t v[MATCH_PIC_AHEAD];
#pragma unroll
      for (int k = 0; k < MATCH_PIC_AHEAD; k++) { const int r = r0 + k * (MAPS_THREADS / 16); v[k] = r < n_ctu ? w[(size_t)r * MATCH_CTU_WORDS] : 0u; }
#pragma unroll
      for (int k = 0; k < MATCH_PIC_AHEAD; k++) { lo += v[k] & 0xffffu; hi += v[k] >> 16; }
    }
    L.lo[t] = lo; L.hi[t] = hi;
  } else if (2 * t < MATCH_COUNTERS) {
    uint64_t lo = 0, hi = 0;
    for (int j = 0; j < MAPS_THREADS / 16; j++) { lo += L.lo[j * 16 + t]; hi += L.hi[j * 16 + t]; }
    uint64_t *q = (uint64_t *)(rec + pic);
    q[2 * t] = lo; q[2 * t + 1] = hi;
  }
}

/* ---- labels_ctu: the whole kernel body (no LDS, no barrier: one phase) */
__device__ static inline void labels_ctu_body(const uint8_t *depth, const int8_t *part_size, int8_t *labels, const MapsGeom &G)
{
  const int l = (int)threadIdx.x & 63, a = (int)blockIdx.x * LABELS_CTUS + ((int)threadIdx.x >> 6), pic = (int)blockIdx.y;
  if (a >= G.n_ctu) return;                                  /* (a whole wave) */
  const int cx = a % G.w_ctu, cy = a / G.w_ctu, W4 = G.width >> 2, H4 = G.height >> 2;
  const size_t plane = (size_t)H4 * W4;
  const FCU_HBM uint8_t *dp = (const FCU_HBM uint8_t *)depth + (size_t)pic * plane;
  const FCU_HBM int8_t *pp = part_size ? (const FCU_HBM int8_t *)part_size + (size_t)pic * plane : nullptr;
  FCU_HBM int8_t *out = (FCU_HBM int8_t *)labels + (size_t)pic * (size_t)G.lvl_off[4];
  /* node 0: level 3 (every lane), node 1: levels 0..2 (lanes 0..20).  A node that exists has its top-left partition inside the
   * picture, so every load below is inside the rasters; every store is at idx < lvl_off[4] */
  MapsNode N[2] = { maps_node(21 + l), maps_node(l < 21 ? l : 0) };
  MapsPlace P[2] = { maps_place(G, N[0], cx, cy), maps_place(G, N[1], cx, cy) };
  P[1].exists = P[1].exists && l < 21;
  int dv[2] = { 0, 0 }, pv = 0;
#pragma unroll
  for (int k = 0; k < 2; k++) if (P[k].exists) dv[k] = dp[(size_t)(cy * 16 + N[k].py) * W4 + cx * 16 + N[k].px];
  if (pp && P[0].exists) pv = pp[(size_t)(cy * 16 + N[0].py) * W4 + cx * 16 + N[0].px];      /* (part_size matters at level 3 alone) */
#pragma unroll
  for (int k = 0; k < 2; k++) if (P[k].exists) out[P[k].idx] = (int8_t)maps_label(N[k].d, dv[k], pv, P[k].whole);
}

#ifndef FCU_EMU
__global__ void __launch_bounds__(LABELS_THREADS) labels_ctu(const uint8_t *depth, const int8_t *part_size, int8_t *labels, const MapsGeom G)
{
  labels_ctu_body(depth, part_size, labels, G);
}
template <int UNIT, int ALIGN>
__global__ void __launch_bounds__(MAPS_THREADS) maps_ctu(const MapsPic *pics, const MapsOut Q, const MapsGeom G)
{
  __shared__ MapsLds L;
  maps_ctu_phase<1, UNIT, ALIGN>(L, pics, Q, G);
  __syncthreads();
  maps_ctu_phase<2, UNIT, ALIGN>(L, pics, Q, G);
  if (Q.nobf) {                                              /* (the same in every thread) */
    __syncthreads();
    maps_ctu_phase<3, UNIT, ALIGN>(L, pics, Q, G);
    __syncthreads();
    maps_ctu_phase<4, UNIT, ALIGN>(L, pics, Q, G);
    __syncthreads();
    maps_ctu_phase<5, UNIT, ALIGN>(L, pics, Q, G);
  }
}
__global__ void __launch_bounds__(MAPS_THREADS) match_ctu(const MatchPic *pics, fcu_ctu_match *ctu, const MapsGeom G)
{
  __shared__ uint32_t part[4][MATCH_COUNTERS];
  match_ctu_phase<1>(part, pics, ctu, G);
  __syncthreads();
  match_ctu_phase<2>(part, pics, ctu, G);
}
__global__ void __launch_bounds__(MAPS_THREADS) match_pic(const fcu_ctu_match *ctu, fcu_pic_match *rec, int n_ctu)
{
  __shared__ MatchPicLds L;
  match_pic_phase<1>(L, ctu, rec, n_ctu);
  __syncthreads();
  match_pic_phase<2>(L, ctu, rec, n_ctu);
}
#endif

} /* namespace fcu */
