/*
 * report_emu.cpp -- TEST-ONLY: the picture-report kernel source (csrc/fcu_report.h) compiled for the CPU with the HIP keywords
 * defined away and both grids run as loops (workgroup phases in order, threads inside a phase in order), so that indexing,
 * the load paths and the sums can be checked against tests/report_ref.py without a GPU.  Not part of libfcu.so.
 */
#define FCU_EMU 1
#include <vector>
#include <cstring>
#include "../../fast-cu-decision-hevc_amd/csrc/fcu_host.h"
#define __device__
struct Dim3 { unsigned x, y, z; };
static thread_local Dim3 blockIdx, threadIdx;
#include "../../fast-cu-decision-hevc_amd/csrc/fcu_report.h"

using namespace fcu;

template <bool WIDE>
static void run_report_ctu(const ReportPic *pics, fcu_ctu_report *ctu, int w, int h, int w_ctu, int n_ctu, int n_pics)
{
  for (unsigned pic = 0; pic < (unsigned)n_pics; pic++) for (unsigned a = 0; a < (unsigned)n_ctu; a++) {
    uint32_t part[4][REP_SLOTS];                             /* the workgroup's LDS; the CPU forms of the wave sums add into it */
    memset(part, 0, sizeof(part));
    blockIdx.x = a; blockIdx.y = pic;
    for (unsigned t = 0; t < REP_THREADS; t++) { threadIdx.x = t; report_ctu_phase<1, WIDE>(part, pics, ctu, w, h, w_ctu, n_ctu); }
    for (unsigned t = 0; t < REP_THREADS; t++) { threadIdx.x = t; report_ctu_phase<2, WIDE>(part, pics, ctu, w, h, w_ctu, n_ctu); }
  }
}

/* mirrors the launches of fcu_picture_report (fcu_kernels.hip).  org / rec: 3 * n_pics plane pointers, out: n_pics record arrays;
 * wide 0: the byte-exact load path whatever the pointers allow, 1: the path the library's host code would choose.
 * Returns the path taken (1 = wide). */
extern "C" int report_emu(int w, int h, int n_pics, int wide, const uint8_t *const *org, const uint8_t *const *rec, const fcu_ctu_out *const *out,
                          fcu_pic_report *reports, fcu_ctu_report *ctu)
{
  const int w_ctu = (w + 63) / 64, n_ctu = w_ctu * ((h + 63) / 64);
  std::vector<ReportPic> P((size_t)n_pics);
  for (int i = 0; i < n_pics; i++) {
    for (int k = 0; k < 3; k++) { P[i].org[k] = org[3 * i + k]; P[i].rec[k] = rec[3 * i + k]; }
    P[i].out = out[i];
  }
  const bool use_wide = wide && report_wide_ok(w, P.data(), n_pics);
  if (use_wide) run_report_ctu<true>(P.data(), ctu, w, h, w_ctu, n_ctu, n_pics);
  else run_report_ctu<false>(P.data(), ctu, w, h, w_ctu, n_ctu, n_pics);
  blockIdx.y = 0;
  static ReportPicLds lds;
  for (unsigned pic = 0; pic < (unsigned)n_pics; pic++) {
    blockIdx.x = pic;
    for (unsigned t = 0; t < REP_THREADS; t++) { threadIdx.x = t; report_pic_phase<1>(lds, ctu, reports, w, h, n_ctu); }
    for (unsigned t = 0; t < REP_THREADS; t++) { threadIdx.x = t; report_pic_phase<2>(lds, ctu, reports, w, h, n_ctu); }
  }
  for (int i = 0; i < n_pics; i++) for (int k = 0; k < 3; k++) reports[i].psnr[k] = report_psnr(reports[i].ssd[k], reports[i].n_samples[k]);
  return use_wide ? 1 : 0;
}
