/*
 * features_emu.cpp -- TEST-ONLY: the feature-map kernel source (csrc/fcu_features.h, with the DCT and the outlier test of
 * csrc/fcu_obf.h) compiled for the CPU with the HIP keywords defined away and the grid run as a loop (workgroup phases in order,
 * threads inside a phase in order), behind the argument rules of fcu_host.h the library applies, so that indexing, the lane
 * layout and the integer arithmetic can be checked against tests/features_ref.py without a GPU.  Not part of libfcu.so.
 */
#define FCU_EMU 1
#include <vector>
#include <cstring>
#include "../../fast-cu-decision-hevc_amd/csrc/fcu_host.h"
#define __device__
struct Dim3 { unsigned x, y, z; };
static thread_local Dim3 blockIdx, threadIdx;
#include "../../fast-cu-decision-hevc_amd/csrc/fcu_features.h"

using namespace fcu;

static thread_local std::string g_err;
extern "C" const char *features_emu_last_error(void) { return g_err.c_str(); }

template <int SETS, int PHASE>
static void run_phases(FeatLds &L, const FeatPic *pics, float *out, const MapsGeom &G)
{
  for (unsigned t = 0; t < FEAT_THREADS; t++) { threadIdx.x = t; feat_ctu_phase<SETS, PHASE>(L, pics, out, G); }
  if constexpr (PHASE < 12) run_phases<SETS, PHASE + 1>(L, pics, out, G);
}
template <int SETS>
static void run_feat_ctu(const FeatPic *pics, float *out, const MapsGeom &G, int n_pics)
{
  static FeatLds L;                                          /* the workgroup's LDS */
  for (unsigned pic = 0; pic < (unsigned)n_pics; pic++) for (unsigned a = 0; a < (unsigned)G.n_ctu; a++) {
    blockIdx.x = a; blockIdx.y = pic;
    memset(&L, 0xee, sizeof(L));                             /* (nothing may be read that this workgroup did not write) */
    run_phases<SETS, 0>(L, pics, out, G);
  }
}

/* mirrors fcu_feature_maps (fcu_kernels.hip) for w x h pictures.  FCU_OK, or FCU_ERR_ARG (text: features_emu_last_error) */
extern "C" int features_emu(int w, int h, int n_pics, int sets, const uint8_t *const *y, const double *yc, float *features)
{
  const int rc = features_args_check(n_pics, sets, y, yc, features, g_err);
  if (rc != FCU_OK) return rc;
  const MapsGeom G = maps_geom(w, h, 0, nullptr);
  std::vector<FeatPic> P((size_t)n_pics);
  for (int i = 0; i < n_pics; i++) {
    P[i].y = y[i];
    for (int k = 0; k < 16; k++) P[i].thr[k] = yc ? obf_thr(yc[(size_t)i * 16 + k]) : 0;
  }
  if (sets == FCU_FEATSET_TMV) run_feat_ctu<FCU_FEATSET_TMV>(P.data(), features, G, n_pics);
  else if (sets == FCU_FEATSET_SOC) run_feat_ctu<FCU_FEATSET_SOC>(P.data(), features, G, n_pics);
  else run_feat_ctu<FCU_FEATSET_TMV | FCU_FEATSET_SOC>(P.data(), features, G, n_pics);
  return FCU_OK;
}

extern "C" int features_emu_count(int sets) { return feature_count(sets); }
