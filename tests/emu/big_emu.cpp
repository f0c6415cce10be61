/*
 * big_emu.cpp -- TEST-ONLY: the loop and grid constants of the picture-level kernels (csrc/fcu_report.h, fcu_maps.h, fcu_trace.h,
 * fcu_risk.h), read from the kernel source itself, so that the cases of tests/big_cases.py can assert that they cross them: a
 * retuned constant then fails the case instead of quietly shrinking what it covers.  No kernel body is run here (the drivers are
 * report_emu.cpp, maps_emu.cpp, cu_trace_emu.cpp and risk_emu.cpp).  Not part of libfcu.so.
 */
#define FCU_EMU 1
#include "../../fast-cu-decision-hevc_amd/csrc/fcu_host.h"
#define __device__
struct Dim3 { unsigned x, y, z; };
static thread_local Dim3 blockIdx, threadIdx;
#include "../../fast-cu-decision-hevc_amd/csrc/fcu_risk.h"

using namespace fcu;

extern "C" {
/* CTU records one trip of the walks of report_pic and match_pic covers */
int big_emu_report_pic_trip(void) { return REP_PIC_AHEAD * (REP_THREADS / 16); }
int big_emu_match_pic_trip(void) { return MATCH_PIC_AHEAD * (MAPS_THREADS / 16); }
/* CTU records one trip of score_pic's walk loads, and the CTUs a workgroup of score_ctu / trace_ctu takes */
int big_emu_score_ahead(void) { return SCORE_AHEAD; }
int big_emu_score_ctus(void) { return SCORE_CTUS; }
/* the plan of risk_train: the cap on workgroups (= slots), the units a workgroup takes before the grid grows no further, its
 * waves, the workgroups of a batch; and the blocks a workgroup of risk_predict / nobf_blocks takes */
int big_emu_risk_max_slots(void) { return RISK_MAX_SLOTS; }
int big_emu_risk_group_units(void) { return RISK_WAVES * RISK_UNITS_PER_WAVE; }
int big_emu_risk_waves(void) { return RISK_WAVES; }
int big_emu_risk_train_groups(int n_units) { return risk_train_groups(n_units); }
int big_emu_risk_pred_threads(void) { return RISK_PRED_THREADS; }
}
