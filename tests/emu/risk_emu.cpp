/*
 * risk_emu.cpp -- TEST-ONLY: the kernel source of the risk-table model (csrc/fcu_risk.h, with the node geometry of csrc/fcu_maps.h
 * and the record loads of csrc/fcu_trace.h) compiled for the CPU with the HIP keywords defined away and every grid run as loops
 * (workgroup phases in order, threads inside a phase in order, the workgroup's LDS poisoned before its first phase), behind the
 * argument rules of fcu_host.h the library applies, so that sample selection, key addressing, the integer sums and the rule can be
 * checked against tests/risk_ref.py without a GPU.  Not part of libfcu.so.
 */
#define FCU_EMU 1
#include <vector>
#include <cstring>
#include "../../fast-cu-decision-hevc_amd/csrc/fcu_host.h"
#define __device__
struct Dim3 { unsigned x, y, z; };
static thread_local Dim3 blockIdx, threadIdx;
#include "../../fast-cu-decision-hevc_amd/csrc/fcu_risk.h"

using namespace fcu;

static thread_local std::string g_err;

extern "C" {
const char *risk_emu_last_error(void) { return g_err.c_str(); }
int risk_emu_sizeof(void) { return (int)sizeof(fcu_risk_model); }
int risk_emu_label_count(int w, int h) { return maps_geom(w, h, 0, nullptr).lvl_off[4]; }

/* mirrors fcu_risk_train for w x h pictures; groups > 0 overrides the number of workgroups (= slots) the batch is dealt to */
int risk_emu_train(int w, int h, int n_pics, const fcu_cu_trace *const *trace, const uint16_t *const *keys, fcu_risk_model *model, int accumulate, uint32_t *dropped, int groups)
{
  const MapsGeom G = maps_geom(w, h, 0, nullptr);
  const int rc = risk_train_args_check(n_pics, trace, keys, model, accumulate, G.lvl_off[4], g_err);
  if (rc != FCU_OK) return rc;
  const int n_units = G.n_ctu * n_pics, n_groups = groups > 0 ? groups : risk_train_groups(n_units);
  std::vector<RiskSlot> slots((size_t)n_groups);
  memset((void *)slots.data(), 0x77, sizeof(RiskSlot) * slots.size());      /* stale bytes: every word of a slot is written */
  static RiskSlot L;                                         /* the workgroup's LDS */
  blockIdx.y = 0;
  for (unsigned g = 0; g < (unsigned)n_groups; g++) {
    blockIdx.x = g;
    memset((void *)&L, 0xee, sizeof(L));                     /* (nothing may be read that this workgroup did not write) */
    for (unsigned t = 0; t < RISK_THREADS; t++) { threadIdx.x = t; risk_train_phase<0>(L, trace, keys, slots.data(), G, n_units, n_groups); }
    for (unsigned t = 0; t < RISK_THREADS; t++) { threadIdx.x = t; risk_train_phase<1>(L, trace, keys, slots.data(), G, n_units, n_groups); }
    for (unsigned t = 0; t < RISK_THREADS; t++) { threadIdx.x = t; risk_train_phase<2>(L, trace, keys, slots.data(), G, n_units, n_groups); }
  }
  uint32_t drop = 0x77777777u;
  static RiskAddLds A;
  for (unsigned g = 0; g < RISK_ADD_GROUPS; g++) {
    blockIdx.x = g;
    memset((void *)&A, 0xee, sizeof(A));
    for (unsigned t = 0; t < RISK_ADD_THREADS; t++) { threadIdx.x = t; risk_add_phase<1>(A, slots.data(), n_groups, model, &drop, accumulate); }
    for (unsigned t = 0; t < RISK_ADD_THREADS; t++) { threadIdx.x = t; risk_add_phase<2>(A, slots.data(), n_groups, model, &drop, accumulate); }
  }
  if (dropped) *dropped = drop;
  return FCU_OK;
}

/* mirrors fcu_risk_predict */
int risk_emu_predict(int w, int h, int n_pics, const uint16_t *const *keys, const fcu_risk_model *model, int min_count, int8_t *labels)
{
  const int rc = risk_predict_args_check(n_pics, keys, model, min_count, labels, g_err);
  if (rc != FCU_OK) return rc;
  const MapsGeom G = maps_geom(w, h, 0, nullptr);
  const RiskPlan P = risk_plan(G);
  static RiskPredLds L;
  for (unsigned pic = 0; pic < (unsigned)n_pics; pic++) for (unsigned g = 0; g < (unsigned)P.wg_off[4]; g++) {
    blockIdx.x = g; blockIdx.y = pic;
    memset((void *)&L, 0xee, sizeof(L));
    for (unsigned t = 0; t < RISK_PRED_THREADS; t++) { threadIdx.x = t; risk_predict_phase<1>(L, keys, model, min_count, labels, G, P); }
    for (unsigned t = 0; t < RISK_PRED_THREADS; t++) { threadIdx.x = t; risk_predict_phase<2>(L, keys, model, min_count, labels, G, P); }
  }
  return FCU_OK;
}

/* mirrors fcu_nobf_maps */
int risk_emu_nobf(int w, int h, int n_pics, const int16_t *const *obf, uint16_t *nobf)
{
  const int rc = nobf_args_check(n_pics, obf, nobf, g_err);
  if (rc != FCU_OK) return rc;
  const MapsGeom G = maps_geom(w, h, 0, nullptr);
  const RiskPlan P = risk_plan(G);
  for (unsigned pic = 0; pic < (unsigned)n_pics; pic++) for (unsigned g = 0; g < (unsigned)P.wg_off[4]; g++) {
    blockIdx.x = g; blockIdx.y = pic;
    for (unsigned t = 0; t < RISK_PRED_THREADS; t++) { threadIdx.x = t; nobf_blocks_body(obf, nobf, G, P); }
  }
  return FCU_OK;
}

/* fcu_risk_table */
void risk_emu_table(const fcu_risk_model *model, int min_count, int8_t *table) { risk_table(model, min_count, (int8_t (*)[FCU_RISK_BINS])table); }
}
