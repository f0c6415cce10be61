/*
 * lf_slices_emu.cpp -- TEST-ONLY: the slice variants of the loop-filter kernel source (csrc/fcu_deblock.h: dbk_pass<DIR,
 * LF_CUT_SLICES>; csrc/fcu_sao.h: the CUT = LF_CUT_SLICES bodies of the statistics and the offset pass) compiled for the CPU with
 * the HIP keywords defined away and every grid run as a loop, as tests/emu/lf_tiles_emu.cpp runs the tile variants.  The slices
 * reach the kernel bodies as libfcu.so hands them over: lf_slices_fill (fcu_host.h) decides between the slice variants and the
 * kernels without a cut (LFCrossSliceBoundaryFlag 1, or one slice), deblocking takes an LfSlices by value, SAO the picture's
 * SaoPic::slice_ctus.  Not part of libfcu.so.
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

/* what fcu_deblock_slices / fcu_sao_slices refuse with FCU_ERR_ARG */
static bool args_ok(int slice_ctus, int cross) { return (cross == 0 || cross == 1) && slice_ctus >= 0; }

/* 1 = the slice variants run for this picture, 0 = the kernels without a cut, -1 = refused; len (may be null): CTUs per slice */
extern "C" int lf_slices_emu_variant(int w, int h, int slice_ctus, int cross, int *len)
{
  if (!args_ok(slice_ctus, cross)) return -1;
  LfSlices S;
  const bool cut = lf_slices_fill(S, ((w + 63) / 64) * ((h + 63) / 64), slice_ctus, cross);
  if (len) *len = S.slice_ctus;
  return cut ? 1 : 0;
}

template <int CUT>
static void run_deblock(const fcu_ctu_out *out, uint8_t *y, uint8_t *u, uint8_t *v, int w, int h, int boff, int toff, const DbkGrid<CUT> &G)
{
  const int w_ctu = (w + 63) / 64;
  const unsigned n0 = (unsigned)((w >> 3) * (h >> 2)), n1 = (unsigned)((w >> 2) * (h >> 3));
  for (unsigned b = 0; b < (n0 + DBK_THREADS - 1) / DBK_THREADS; b++)
    for (unsigned t = 0; t < DBK_THREADS; t++) { blockIdx.x = b; threadIdx.x = t; dbk_pass<0, CUT>(out, y, u, v, w, h, w_ctu, boff, toff, G); }
  for (unsigned b = 0; b < (n1 + DBK_THREADS - 1) / DBK_THREADS; b++)
    for (unsigned t = 0; t < DBK_THREADS; t++) { blockIdx.x = b; threadIdx.x = t; dbk_pass<1, CUT>(out, y, u, v, w, h, w_ctu, boff, toff, G); }
}
/* mirrors the launches of fcu_deblock_slices */
extern "C" int lf_slices_emu_deblock(const fcu_ctu_out *out, uint8_t *y, uint8_t *u, uint8_t *v, int w, int h, int boff, int toff, int slice_ctus, int cross)
{
  if (!args_ok(slice_ctus, cross)) return 0;
  LfSlices S;
  if (lf_slices_fill(S, ((w + 63) / 64) * ((h + 63) / 64), slice_ctus, cross)) run_deblock<LF_CUT_SLICES>(out, y, u, v, w, h, boff, toff, DbkGrid<LF_CUT_SLICES>{ S });
  else run_deblock<LF_CUT_NONE>(out, y, u, v, w, h, boff, toff, DbkGrid<LF_CUT_NONE>());
  return 1;
}

template <int CUT>
static void run_stats(const SaoPic &P, int32_t *stats, int w, int h, int w_ctu, int n_ctu)
{
  int32_t hist[SAO_STAT_INTS];
  blockIdx.z = 0;
  for (unsigned a = 0; a < (unsigned)n_ctu; a++) for (unsigned comp = 0; comp < 3; comp++) {
    blockIdx.x = a; blockIdx.y = comp;
    for (unsigned t = 0; t < SAO_THREADS; t++) { threadIdx.x = t; sao_stats_phase<0, CUT>(hist, &P, stats, w, h, w_ctu, n_ctu); }
    for (unsigned t = 0; t < SAO_THREADS; t++) { threadIdx.x = t; sao_stats_phase<1, CUT>(hist, &P, stats, w, h, w_ctu, n_ctu); }
    for (unsigned t = 0; t < SAO_THREADS; t++) { threadIdx.x = t; sao_stats_phase<2, CUT>(hist, &P, stats, w, h, w_ctu, n_ctu); }
  }
  blockIdx.y = 0;
}
template <int CUT>
static void run_apply(const SaoPic &P, const fcu_sao_ctu *recon, int w, int h, int w_ctu, int n_ctu)
{
  blockIdx.z = 0;
  for (unsigned a = 0; a < (unsigned)n_ctu; a++) for (unsigned comp = 0; comp < 3; comp++)
    for (unsigned t = 0; t < SAO_THREADS; t++) { blockIdx.x = a; blockIdx.y = comp; threadIdx.x = t; sao_apply_block<CUT>(&P, recon, w, h, w_ctu, n_ctu); }
  blockIdx.y = 0;
}
struct Pic { std::vector<uint8_t> src[3]; SaoPic P; };
static void bind(Pic &p, int w, int h, const uint8_t *const org[3], uint8_t *const rec[3])
{
  const size_t plane[3] = { (size_t)w * h, (size_t)(w / 2) * (h / 2), (size_t)(w / 2) * (h / 2) };
  for (int k = 0; k < 3; k++) {
    p.src[k].assign(rec[k], rec[k] + plane[k]);
    p.P.org[k] = org[k]; p.P.rec[k] = rec[k]; p.P.src[k] = p.src[k].data(); p.P.lambda[k] = 0; p.P.enabled[k] = 1;
  }
  p.P.slice_type = 0; p.P.qp = 0; p.P.slice_ctus = 0;
}

/* one picture; mirrors the launches of fcu_sao_slices.  recon_out (may be null): the reconstructed parameters */
extern "C" int lf_slices_emu_sao(int w, int h, int slice_type, int qp, const double *lambda, const int *enabled, int slice_ctus, int cross,
                                 const uint8_t *oy, const uint8_t *ou, const uint8_t *ov, uint8_t *ry, uint8_t *ru, uint8_t *rv,
                                 fcu_sao_ctu *coded, int32_t *off_count, int32_t *stats_out, fcu_sao_ctu *recon_out)
{
  if (!args_ok(slice_ctus, cross)) return 0;
  const int w_ctu = (w + 63) / 64, n_ctu = w_ctu * ((h + 63) / 64);
  const uint8_t *org[3] = { oy, ou, ov }; uint8_t *rec[3] = { ry, ru, rv };
  Pic p;
  bind(p, w, h, org, rec);
  SaoPic &P = p.P;
  for (int k = 0; k < 3; k++) { P.lambda[k] = lambda[k]; P.enabled[k] = enabled[k]; }
  P.slice_type = slice_type; P.qp = qp; P.slice_ctus = slice_ctus;
  LfSlices S;
  const bool SL = lf_slices_fill(S, n_ctu, slice_ctus, cross);
  std::vector<int32_t> stats((size_t)n_ctu * 3 * SAO_STAT_INTS);
  std::vector<SaoCand> cands((size_t)n_ctu * 15);
  std::vector<fcu_sao_ctu> recon((size_t)n_ctu);
  if (SL) run_stats<LF_CUT_SLICES>(P, stats.data(), w, h, w_ctu, n_ctu); else run_stats<LF_CUT_NONE>(P, stats.data(), w, h, w_ctu, n_ctu);
  for (unsigned b = 0; b < ((unsigned)n_ctu * 15 + SAO_THREADS - 1) / SAO_THREADS; b++)
    for (unsigned t = 0; t < SAO_THREADS; t++) { blockIdx.x = b; threadIdx.x = t; sao_cands_thread(&P, stats.data(), cands.data(), n_ctu, 1); }
  static SaoDecideLds lds;
  sao_decide_picture(P, stats.data(), cands.data(), coded, recon.data(), off_count, w_ctu, n_ctu, lds);
  if (SL) run_apply<LF_CUT_SLICES>(P, recon.data(), w, h, w_ctu, n_ctu); else run_apply<LF_CUT_NONE>(P, recon.data(), w, h, w_ctu, n_ctu);
  if (stats_out) memcpy(stats_out, stats.data(), stats.size() * sizeof(int32_t));
  if (recon_out) memcpy(recon_out, recon.data(), recon.size() * sizeof(fcu_sao_ctu));
  return 1;
}

/* the offset pass alone, with given reconstructed parameters, in place on the planes (sao_apply_slices / sao_apply) */
extern "C" int lf_slices_emu_apply(int w, int h, int slice_ctus, int cross, const fcu_sao_ctu *recon, uint8_t *ry, uint8_t *ru, uint8_t *rv)
{
  if (!args_ok(slice_ctus, cross)) return 0;
  const int w_ctu = (w + 63) / 64, n_ctu = w_ctu * ((h + 63) / 64);
  uint8_t *rec[3] = { ry, ru, rv }; const uint8_t *org[3] = { ry, ru, rv };
  Pic p;
  bind(p, w, h, org, rec);
  p.P.slice_ctus = slice_ctus;
  LfSlices S;
  if (lf_slices_fill(S, n_ctu, slice_ctus, cross)) run_apply<LF_CUT_SLICES>(p.P, recon, w, h, w_ctu, n_ctu); else run_apply<LF_CUT_NONE>(p.P, recon, w, h, w_ctu, n_ctu);
  return 1;
}
