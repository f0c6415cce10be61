/*
 * maps_emu.cpp -- TEST-ONLY: the decision-map and split-match kernel source (csrc/fcu_maps.h) compiled for the CPU with the HIP
 * keywords defined away and every grid run as a loop (workgroup phases in order, threads inside a phase in order), behind the
 * argument rules of fcu_host.h the library applies, so that indexing, both store paths and the counts can be checked against
 * tests/maps_ref.py without a GPU.  Not part of libfcu.so.
 */
#define FCU_EMU 1
#include <vector>
#include <cstring>
#include "../../fast-cu-decision-hevc_amd/csrc/fcu_host.h"
#define __device__
struct Dim3 { unsigned x, y, z; };
static thread_local Dim3 blockIdx, threadIdx;
#include "../../fast-cu-decision-hevc_amd/csrc/fcu_maps.h"

using namespace fcu;

static thread_local std::string g_err;
extern "C" const char *maps_emu_last_error(void) { return g_err.c_str(); }

template <int UNIT, int ALIGN>
static void run_maps_ctu(const MapsPic *pics, const MapsOut &Q, const MapsGeom &G, int n_pics)
{
  static MapsLds L;                                          /* the workgroup's LDS */
  for (unsigned pic = 0; pic < (unsigned)n_pics; pic++) for (unsigned a = 0; a < (unsigned)G.n_ctu; a++) {
    blockIdx.x = a; blockIdx.y = pic;
    memset(&L, 0xee, sizeof(L));                             /* (nothing may be read that this workgroup did not write) */
    for (unsigned t = 0; t < MAPS_THREADS; t++) { threadIdx.x = t; maps_ctu_phase<1, UNIT, ALIGN>(L, pics, Q, G); }
    for (unsigned t = 0; t < MAPS_THREADS; t++) { threadIdx.x = t; maps_ctu_phase<2, UNIT, ALIGN>(L, pics, Q, G); }
    if (!Q.nobf) continue;
    for (unsigned t = 0; t < MAPS_THREADS; t++) { threadIdx.x = t; maps_ctu_phase<3, UNIT, ALIGN>(L, pics, Q, G); }
    for (unsigned t = 0; t < MAPS_THREADS; t++) { threadIdx.x = t; maps_ctu_phase<4, UNIT, ALIGN>(L, pics, Q, G); }
    for (unsigned t = 0; t < MAPS_THREADS; t++) { threadIdx.x = t; maps_ctu_phase<5, UNIT, ALIGN>(L, pics, Q, G); }
  }
}

/* mirrors fcu_decision_maps (fcu_kernels.hip) for a w x h picture; wide 0: the 2-byte store path whatever the pointers allow, 1:
 * the path the library's host code would choose.  Returns FCU_ERR_ARG (text: maps_emu_last_error) or the alignment of the path
 * taken: 16, 2 or 1. */
extern "C" int maps_emu(int w, int h, int n_pics, int wide, const fcu_ctu_out *const *out, int n_fields, const int *field_ids, uint8_t *bytes, int16_t *mv,
                        int8_t *labels, const int16_t *const *obf, uint16_t *nobf)
{
  const int rc = maps_args_check(n_pics, out, n_fields, field_ids, bytes, mv, labels, obf, nobf, g_err);
  if (rc != FCU_OK) return rc;
  const MapsGeom G = maps_geom(w, h, n_fields, field_ids);
  std::vector<MapsPic> P((size_t)n_pics);
  for (int i = 0; i < n_pics; i++) { P[i].out = out[i]; P[i].obf = obf ? obf[i] : nullptr; }
  const MapsOut Q = { bytes, mv, labels, nobf };
  int align = maps_row_align(w, bytes, mv);
  if (!wide && align == 16) align = 2;
  if (align == 16) run_maps_ctu<16, 16>(P.data(), Q, G, n_pics);
  else if (align == 2) run_maps_ctu<2, 2>(P.data(), Q, G, n_pics);
  else run_maps_ctu<2, 1>(P.data(), Q, G, n_pics);
  return align;
}

/* mirrors fcu_split_match */
extern "C" int match_emu(int w, int h, int n_pics, const fcu_ctu_out *const *out_a, const fcu_ctu_out *const *out_b, fcu_pic_match *matches, fcu_ctu_match *ctu)
{
  const int rc = match_args_check(n_pics, out_a, out_b, matches, g_err);
  if (rc != FCU_OK) return rc;
  const MapsGeom G = maps_geom(w, h, 0, nullptr);
  std::vector<MatchPic> P((size_t)n_pics);
  for (int i = 0; i < n_pics; i++) { P[i].a = out_a[i]; P[i].b = out_b[i]; }
  for (unsigned pic = 0; pic < (unsigned)n_pics; pic++) for (unsigned a = 0; a < (unsigned)G.n_ctu; a++) {
    uint32_t part[4][MATCH_COUNTERS];                        /* the workgroup's LDS; the CPU form of the wave count adds into it */
    memset(part, 0, sizeof(part));
    blockIdx.x = a; blockIdx.y = pic;
    for (unsigned t = 0; t < MAPS_THREADS; t++) { threadIdx.x = t; match_ctu_phase<1>(part, P.data(), ctu, G); }
    for (unsigned t = 0; t < MAPS_THREADS; t++) { threadIdx.x = t; match_ctu_phase<2>(part, P.data(), ctu, G); }
  }
  blockIdx.y = 0;
  static MatchPicLds lds;
  for (unsigned pic = 0; pic < (unsigned)n_pics; pic++) {
    blockIdx.x = pic;
    for (unsigned t = 0; t < MAPS_THREADS; t++) { threadIdx.x = t; match_pic_phase<1>(lds, ctu, matches, G.n_ctu); }
    for (unsigned t = 0; t < MAPS_THREADS; t++) { threadIdx.x = t; match_pic_phase<2>(lds, ctu, matches, G.n_ctu); }
  }
  return FCU_OK;
}

/* the field table of fcu_host.h, for the layout test */
extern "C" int maps_emu_field_offset(int id) { return maps_field_offset(id); }
