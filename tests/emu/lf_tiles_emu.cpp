/*
 * lf_tiles_emu.cpp -- TEST-ONLY: the tile variants of the loop-filter kernel source (csrc/fcu_deblock.h: dbk_pass<DIR, true>;
 * csrc/fcu_sao.h: the TILES = true bodies) compiled for the CPU with the HIP keywords defined away and every grid run as a loop,
 * as tests/emu/dbk_emu.cpp and tests/emu/sao_emu.cpp run the kernels without tiles.  The grid reaches the kernel bodies as
 * libfcu.so hands it over: an LfTiles made by lf_tiles_fill (fcu_host.h), by value.  Not part of libfcu.so.
 */
/* sao_decide writes a CTU's records a dword per lane and sao_apply reads them as bytes: two kernels on the device, one
 * translation unit here, where type-based alias analysis may move the byte loads across the dword stores */
#pragma GCC optimize("no-strict-aliasing")
#define FCU_EMU 1
#include <vector>
#include <cstring>
#include "../../fast-cu-decision-hevc_amd/csrc/fcu_host.h"
#define __device__
#define __global__
#define __launch_bounds__(x)
struct Dim3 { unsigned x, y, z; };
static thread_local Dim3 blockIdx, threadIdx;
static inline void atomicAdd(int32_t *p, int v) { *p += v; }
#include "../../fast-cu-decision-hevc_amd/csrc/fcu_deblock.h"
#include "../../fast-cu-decision-hevc_amd/csrc/fcu_sao.h"

using namespace fcu;

/* 0 = the grid is refused (what fcu_deblock_tiles / fcu_sao_tiles answer with FCU_ERR_ARG); masks8 (may be null) receives the
 * eight mask words, columns first */
extern "C" int lf_tiles_emu_grid(int w, int h, int n_cols, int n_rows, int cross, uint64_t *masks8)
{
  LfTiles T;
  if (!lf_tiles_fill(T, (w + 63) / 64, (h + 63) / 64, n_cols, n_rows, cross)) return 0;
  if (masks8) for (int k = 0; k < 4; k++) { masks8[k] = T.col[k]; masks8[4 + k] = T.row[k]; }
  return 1;
}

/* mirrors the launches of fcu_deblock_tiles */
extern "C" int lf_tiles_emu_deblock(const fcu_ctu_out *out, uint8_t *y, uint8_t *u, uint8_t *v, int w, int h, int boff, int toff, int n_cols, int n_rows, int cross)
{
  LfTiles T;
  if (!lf_tiles_fill(T, (w + 63) / 64, (h + 63) / 64, n_cols, n_rows, cross)) return 0;
  const DbkGrid<true> G{ T };
  const int w_ctu = (w + 63) / 64;
  const unsigned n0 = (unsigned)((w >> 3) * (h >> 2)), n1 = (unsigned)((w >> 2) * (h >> 3));
  for (unsigned b = 0; b < (n0 + DBK_THREADS - 1) / DBK_THREADS; b++)
    for (unsigned t = 0; t < DBK_THREADS; t++) { blockIdx.x = b; threadIdx.x = t; dbk_pass<0, true>(out, y, u, v, w, h, w_ctu, boff, toff, G); }
  for (unsigned b = 0; b < (n1 + DBK_THREADS - 1) / DBK_THREADS; b++)
    for (unsigned t = 0; t < DBK_THREADS; t++) { blockIdx.x = b; threadIdx.x = t; dbk_pass<1, true>(out, y, u, v, w, h, w_ctu, boff, toff, G); }
  return 1;
}

/* one picture; mirrors the launches of fcu_sao_tiles */
extern "C" int lf_tiles_emu_sao(int w, int h, int slice_type, int qp, const double *lambda, const int *enabled, int n_cols, int n_rows, int cross,
                                const uint8_t *oy, const uint8_t *ou, const uint8_t *ov, uint8_t *ry, uint8_t *ru, uint8_t *rv,
                                fcu_sao_ctu *coded, int32_t *off_count, int32_t *stats_out)
{
  LfTiles T;
  if (!lf_tiles_fill(T, (w + 63) / 64, (h + 63) / 64, n_cols, n_rows, cross)) return 0;
  const int w_ctu = (w + 63) / 64, n_ctu = w_ctu * ((h + 63) / 64);
  const size_t plane[3] = { (size_t)w * h, (size_t)(w / 2) * (h / 2), (size_t)(w / 2) * (h / 2) };
  std::vector<uint8_t> src[3];
  uint8_t *rec[3] = { ry, ru, rv }; const uint8_t *org[3] = { oy, ou, ov };
  SaoPic P;
  for (int k = 0; k < 3; k++) {
    src[k].assign(rec[k], rec[k] + plane[k]);
    P.org[k] = org[k]; P.rec[k] = rec[k]; P.src[k] = src[k].data(); P.lambda[k] = lambda[k]; P.enabled[k] = enabled[k];
  }
  P.slice_type = slice_type; P.qp = qp; P.slice_ctus = 0;
  std::vector<int32_t> stats((size_t)n_ctu * 3 * SAO_STAT_INTS);
  std::vector<SaoCand> cands((size_t)n_ctu * 15);
  std::vector<fcu_sao_ctu> recon((size_t)n_ctu);
  int32_t hist[SAO_STAT_INTS];
  blockIdx.z = 0;
  for (unsigned a = 0; a < (unsigned)n_ctu; a++) for (unsigned comp = 0; comp < 3; comp++) {
    blockIdx.x = a; blockIdx.y = comp;
    for (unsigned t = 0; t < SAO_THREADS; t++) { threadIdx.x = t; sao_stats_phase<0, true>(hist, &P, stats.data(), w, h, w_ctu, n_ctu, T); }
    for (unsigned t = 0; t < SAO_THREADS; t++) { threadIdx.x = t; sao_stats_phase<1, true>(hist, &P, stats.data(), w, h, w_ctu, n_ctu, T); }
    for (unsigned t = 0; t < SAO_THREADS; t++) { threadIdx.x = t; sao_stats_phase<2, true>(hist, &P, stats.data(), w, h, w_ctu, n_ctu, T); }
  }
  blockIdx.y = 0;
  for (unsigned b = 0; b < ((unsigned)n_ctu * 15 + SAO_THREADS - 1) / SAO_THREADS; b++)
    for (unsigned t = 0; t < SAO_THREADS; t++) { blockIdx.x = b; threadIdx.x = t; sao_cands_thread(&P, stats.data(), cands.data(), n_ctu, 1); }
  static SaoDecideLds lds;
  sao_decide_picture<true>(P, stats.data(), cands.data(), coded, recon.data(), off_count, w_ctu, n_ctu, lds, T);
  for (unsigned a = 0; a < (unsigned)n_ctu; a++) for (unsigned comp = 0; comp < 3; comp++)
    for (unsigned t = 0; t < SAO_THREADS; t++) { blockIdx.x = a; blockIdx.y = comp; threadIdx.x = t; sao_apply_block<true>(&P, recon.data(), w, h, w_ctu, n_ctu, T); }
  if (stats_out) memcpy(stats_out, stats.data(), stats.size() * sizeof(int32_t));
  return 1;
}
