/*
 * fcu_engine.h -- the CTU decision engine: one 64-lane wavefront per chain.
 *
 * A chain is the unit that HM processes strictly sequentially (a slice of an I picture:
 * reconstructed neighbours, CABAC contexts and neighbour decisions all flow CTU to CTU,
 * SURVEY.md 7.1).  Chains are independent, so the GPU runs thousands of them side by
 * side, one wavefront each; inside a chain the wave
 *   - spreads pixel work (35-mode prediction, Hadamard SATD, DCT/DST, dequant, recon, SSE)
 *     across its 64 lanes,
 *   - evaluates the independent RDO candidates of a PU (each restarts from the same CABAC
 *     snapshot, TEncSearch.cpp:2457) on different lanes: RDOQ and bit counting are
 *     lane-private serial code,
 *   - keeps CABAC snapshots, reference samples and the SATD staging buffer in LDS.
 *
 * Code style: "phases".  FCU_FOR_LANES { ... } is per-lane code followed by a workgroup
 * barrier; everything outside such a block is wave-uniform, reads memory only, and never
 * stores.  All cross-lane communication goes through memory (LDS / the chain's global
 * scratch).  The same source therefore also builds as a plain C++ wave emulator
 * (-DFCU_EMU, tests only) used to check the engine's logic where no GPU is present.
 *
 * Every routine cites the reference code it replaces (paths relative to the reference tree).
 */
#pragma once
#include <stdint.h>
#include <string.h>
#include <type_traits>
#include "../../include/fcu.h"

#ifdef FCU_EMU
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#define FCU_DEV static inline
#define FCU_MEMBER inline
#define FCU_NOINLINE
#define FCU_INLINE
#define FCU_TABLE static const
/* The emulator runs the 64 lanes of a phase one after the other.  FCU_UNI(x) claims "x is the same in every lane":
 * on the device it is a readfirstlane that silently takes lane 0's value, so a false claim corrupts the other lanes.
 * The emulator checks the claim: inside a phase every lane that reaches the same FCU_UNI site must bring the value the
 * first lane brought (tests/emu; the device build cannot check this). */
static int g_emu_phase = 0, g_emu_in_phase = 0, g_emu_lane = 0, g_emu_relax = 0;
/* a lane-private serial walk whose calls are data dependent per lane (the lanes that do call are in lockstep on the
 * device, but the emulator cannot line their calls up): the check is suspended inside */
#define FCU_EMU_RELAX(on) (g_emu_relax = (on))
static inline int fcu_emu_phase_begin() { g_emu_phase++; g_emu_in_phase = 1; g_emu_lane = 0; return 0; }
static inline int fcu_emu_phase_next(int lane) { if (lane + 1 >= 64) g_emu_in_phase = 0; g_emu_lane = lane + 1; return lane + 1; }
/* the k-th visit of a site by a lane must bring what the k-th visit by the first visiting lane brought (lanes run in
 * lockstep on the device; a lane may visit a site more often than the first one did: different trip counts) */
template <class T> static inline T fcu_emu_uni(T v, int site, int line)
{
  enum { SITES = 2048, K = 32, B = 16 };
  struct Seen { int phase, first, cur, idx, n; unsigned char vals[K][B]; };
  static Seen seen[SITES];
  if (g_emu_in_phase && !g_emu_relax && sizeof(T) <= B && site < SITES) {
    Seen &s = seen[site];
    if (s.phase != g_emu_phase) { s.phase = g_emu_phase; s.first = s.cur = g_emu_lane; s.idx = 0; s.n = 0; }
    if (s.cur != g_emu_lane) { s.cur = g_emu_lane; s.idx = 0; }
    if (g_emu_lane == s.first) { if (s.n < K) memcpy(s.vals[s.n++], &v, sizeof(T)); }
    else if (s.idx < s.n && memcmp(s.vals[s.idx], &v, sizeof(T)) != 0) { fprintf(stderr, "FCU_UNI at line %d: value differs between lanes of one phase\n", line); abort(); }
    s.idx++;
  }
  return v;
}
#define FCU_FOR_LANES for (int lane = fcu_emu_phase_begin(); lane < 64; lane = fcu_emu_phase_next(lane))
/* a phase whose results stay in the lanes' registers (LaneVar) or go to memory nothing reads before the next FCU_FOR_LANES
 * phase has ended: the same lane loop here, no barrier on the device */
#define FCU_FOR_LANES_REG FCU_FOR_LANES
#define FCU_ATOMIC_ADD(p, v) (*(p) += (v))
#define FCU_ATOMIC_MAX(p, v) do { if (*(p) < (v)) *(p) = (v); } while (0)
#define FCU_ATOMIC_OR(p, v) (*(p) |= (v))
/* wave reductions of per-lane partial results into one LDS word (all 64 lanes call them, outside divergent code) */
#define FCU_WAVE_ADD(p, v) (*(p) += (v))
#define FCU_WAVE_MIN64(p, v) do { if ((v) < *(p)) *(p) = (v); } while (0)
#define FCU_IN_LDS(p) do { } while (0)
#define FCU_UNI(x) fcu_emu_uni((x), __COUNTER__, __LINE__)
#define FCU_HBM
#define FCU_FLOOR(x) floor(x)
#define FCU_CHECK(c) do { if (!(c)) { fprintf(stderr, "FCU_CHECK failed: %s (line %d)\n", #c, __LINE__); abort(); } } while (0)
/* intra candidate CUs by the way their bits were found (check_rd_cost_intra): merged from the search's coders with the chroma
 * search's own coder, merged with a chroma-only walk, walked in full */
static unsigned long long g_emu_cu_paths[3] = { 0, 0, 0 };
#else
#define FCU_DEV __device__ static
#define FCU_MEMBER __device__ inline
#define FCU_NOINLINE __noinline__
#define FCU_INLINE __attribute__((always_inline))
#define FCU_TABLE __device__ static const
#define FCU_FOR_LANES for (int lane = (int)threadIdx.x, fcu_once_ = 1; fcu_once_; fcu_once_ = 0, __syncthreads())
#define FCU_FOR_LANES_REG for (int lane = (int)threadIdx.x, fcu_once_ = 1; fcu_once_; fcu_once_ = 0)
#define FCU_ATOMIC_ADD(p, v) atomicAdd((p), (v))
#define FCU_ATOMIC_MAX(p, v) atomicMax((p), (v))
#define FCU_ATOMIC_OR(p, v) atomicOr((p), (v))
/* wave reductions in registers, then ONE lane touches LDS -- the SAD / SSE / Hadamard partial sums (north star: "wavefront
 * reductions for per-PU costs").  The sum runs on the DPP path of the VALU (six v_add_u32_dpp: two quad permutes, two row
 * rotations, row_bcast:15 into rows 1 and 3, row_bcast:31 into rows 2 and 3; lane 63 then holds the total) instead of
 * six ds_bpermute round trips through the LDS crossbar (__shfl_xor).  All 64 lanes must be active. */
__device__ inline uint32_t fcu_wave_sum(uint32_t v)
{
  v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0xb1, 0xf, 0xf, false);    /* quad_perm:[1,0,3,2] */
  v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x4e, 0xf, 0xf, false);    /* quad_perm:[2,3,0,1] */
  v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x124, 0xf, 0xf, false);   /* row_ror:4 */
  v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x128, 0xf, 0xf, false);   /* row_ror:8: every lane of a row holds the row's sum */
  v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x142, 0xa, 0xf, false);   /* row_bcast:15 -> rows 1, 3 */
  v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x143, 0xc, 0xf, false);   /* row_bcast:31 -> rows 2, 3 */
  return (uint32_t)__builtin_amdgcn_readlane((int)v, 63);
}
__device__ inline unsigned long long fcu_wave_min64(unsigned long long v)
{
  for (int o = 32; o > 0; o >>= 1) {
    const unsigned lo = (unsigned)__shfl_xor((int)(unsigned)v, o), hi = (unsigned)__shfl_xor((int)(unsigned)(v >> 32), o);
    const unsigned long long w = ((unsigned long long)hi << 32) | lo;
    v = w < v ? w : v;
  }
  return v;
}
#define FCU_WAVE_ADD(p, v) do { const uint32_t s_ = fcu_wave_sum(v); if (threadIdx.x == 0) *(p) += s_; } while (0)
#define FCU_WAVE_MIN64(p, v) do { const unsigned long long s_ = fcu_wave_min64(v); if (threadIdx.x == 0 && s_ < *(p)) *(p) = s_; } while (0)
/* address-space fact for a pointer that crossed a call boundary (lets the compiler emit ds_ instead of flat_ accesses) */
/* wave-uniform value -> scalar registers.  Everything the orchestration code passes around (chain/scratch/CU
 * pointers, TU descriptors, depths) is the same in all lanes; saying so keeps it in SGPRs, turns the control
 * flow into scalar branches and keeps such values out of VGPR spill code around calls. */
template <class T> __device__ inline T fcu_uni(T v)
{
  static_assert(sizeof(T) % 4 == 0, "dword-sized objects only");
  int w[sizeof(T) / 4];
  __builtin_memcpy(w, &v, sizeof(T));
  for (unsigned i = 0; i < sizeof(T) / 4; i++) w[i] = __builtin_amdgcn_readfirstlane(w[i]);
  __builtin_memcpy(&v, w, sizeof(T));
  return v;
}
#define FCU_UNI(x) fcu_uni(x)
#define FCU_EMU_RELAX(on) do { } while (0)
/* pointer-to-HBM type qualifier: accesses become global_ instead of flat_ instructions, which (unlike flat) may stay
 * in flight across a partial s_waitcnt -- needed for the one-ahead loads of the serial coefficient loops */
#if defined(__HIP_DEVICE_COMPILE__)
#define FCU_HBM __attribute__((address_space(1)))
#else
#define FCU_HBM
#endif
#define FCU_GENERIC_(p) ((const __attribute__((address_space(0))) void *)(p))
#define FCU_IN_LDS(p) __builtin_assume(__builtin_amdgcn_is_shared(FCU_GENERIC_(p)))
#define FCU_FLOOR(x) floor(x)
#define FCU_CHECK(c) do { } while (0)
#endif
/* Squared error of one sample into the distortion word of its candidate `v` (samples i of candidates of n2 samples each, dealt
 * 64 per iteration).  Blocks of 64 samples or more: the 64 lanes of an iteration share the candidate, so each lane sums in a
 * register and the wave reduces once per candidate; 4x4 blocks (four candidates per iteration) keep the LDS atomic. */
#define FCU_DIST_ADD(acc, v, e, i, n2) do { \
    if ((n2) >= 64) { (acc) += (uint32_t)((e) * (e)); if (((((i) - lane) + 64) & ((n2) - 1)) == 0) { FCU_WAVE_ADD(&g_S.vc_dist[v], acc); (acc) = 0; } } \
    else FCU_ATOMIC_ADD(&g_S.vc_dist[v], (uint32_t)((e) * (e))); } while (0)
#define FCU_SERIAL FCU_FOR_LANES if (lane == 0)
/* section timers (diagnostic build only: -DFCU_PROFILE; shader-clock ticks summed per chain by lane 0) */
#if defined(FCU_PROFILE_RDOQ) && ((FCU_PROFILE_RDOQ + 0) < 2 || (FCU_PROFILE_RDOQ + 0) > 4)
#error "-DFCU_PROFILE_RDOQ takes a value: 2 (rdoq() on lane 0), 3 (the passes of rdoq_wave) or 4 (the level choice of rdoq())"
#endif
#if defined(FCU_PROFILE) && !defined(FCU_EMU)
#define FCU_TIC(v) const long long v = clock64()
#ifdef FCU_PROFILE_RQT   /* inter residual quadtree variant: slots 0..8 belong to the stages of inter_tu_trials / est_inter_residual_qt (FCU_QTOC); 10 stays the CTU total */
#define FCU_QTIC(v) long long v = clock64()
#define FCU_QTOC(E_, v, idx) do { if (threadIdx.x == 0) (E_).C->prof[idx] += (unsigned long long)(clock64() - v); v = clock64(); } while (0)
#define FCU_TOC(E_, v, idx) do { if ((idx) == 10 && threadIdx.x == 0) (E_).C->prof[idx] += (unsigned long long)(clock64() - v); } while (0)
#define FCU_COUNT(E_, idx, n) do { } while (0)
#elif defined(FCU_PROFILE_INTER)  /* P-path variant: slots 0..9 and 11..14 belong to the sections of compress_cu's P branch / pred_inter_search (FCU_ITOC); 10 stays the CTU total */
#define FCU_ITOC(E_, v, idx) do { if (threadIdx.x == 0) (E_).C->prof[idx] += (unsigned long long)(clock64() - v); } while (0)
#define FCU_TOC(E_, v, idx) do { if ((idx) == 10 && threadIdx.x == 0) (E_).C->prof[idx] += (unsigned long long)(clock64() - v); } while (0)
#define FCU_COUNT(E_, idx, n) do { } while (0)
#elif defined(FCU_PROFILE_RDOQ) && (FCU_PROFILE_RDOQ + 0) == 3   /* rdoq_wave variant: every slot but 10 (the CTU total) belongs to the sub-timers of rdoq_wave (FCU_WTOC) */
#define FCU_TOC(E_, v, idx) do { if ((idx) == 10 && threadIdx.x == 0) (E_).C->prof[idx] += (unsigned long long)(clock64() - v); } while (0)
#define FCU_COUNT(E_, idx, n) do { } while (0)
#elif defined(FCU_PROFILE_RDOQ) && (FCU_PROFILE_RDOQ + 0) == 4   /* level-choice variant: slots 2, 8 and 10 keep their sections and 13 (chroma_rdoq) moves to 3; the others belong to the coefficient loop of rdoq() (FCU_LV_*) */
#define FCU_TOC(E_, v, idx) do { if (((idx) == 2 || (idx) == 8 || (idx) == 10 || (idx) == 13) && threadIdx.x == 0) (E_).C->prof[(idx) == 13 ? 3 : (idx)] += (unsigned long long)(clock64() - v); } while (0)
#define FCU_COUNT(E_, idx, n) do { } while (0)
#elif defined(FCU_PROFILE_RDOQ) || defined(FCU_PROFILE_DEPTH)   /* slots 11..15 belong to the sub-timers of rdoq() on lane 0, -DFCU_PROFILE_RDOQ=2 (FCU_PROFILE_DEPTH: 11..14 to the time spent at CU depth 0..3 without its sub-CUs) in these variants */
#define FCU_TOC(E_, v, idx) do { if ((idx) < 11 && threadIdx.x == 0) (E_).C->prof[idx] += (unsigned long long)(clock64() - v); } while (0)
#define FCU_COUNT(E_, idx, n) do { } while (0)
#elif defined(FCU_PROFILE_RMD)   /* RMD variant: slots 11..14 belong to the sub-timers of rmd() and to the reference build of the first pass (FCU_MTOC) */
#define FCU_MTOC(E_, v, idx) do { if (threadIdx.x == 0) (E_).C->prof[idx] += (unsigned long long)(clock64() - v); } while (0)
#define FCU_TOC(E_, v, idx) do { if ((idx) < 11 && threadIdx.x == 0) (E_).C->prof[idx] += (unsigned long long)(clock64() - v); } while (0)
#define FCU_COUNT(E_, idx, n) do { } while (0)
#elif defined(FCU_PROFILE_CUSYN)   /* CU-syntax variant: slots 11..14 split section 7 (FCU_STOC: 11 / 12 = its 2Nx2N / NxN calls, 13 / 14 = code_coeff_nxn of luma / chroma levels inside the 2Nx2N calls); 15 counts the CUs per path, 21 bits each (FCU_SPATH) */
#define FCU_STOC(E_, v, idx) do { if (threadIdx.x == 0) (E_).C->prof[idx] += (unsigned long long)(clock64() - v); } while (0)
#define FCU_SPATH(E_, path) do { if (threadIdx.x == 0) (E_).C->prof[15] += 1ull << (21 * (path)); } while (0)
#define FCU_S7_COEFF(E_, v, comp) do { if (g_S.prof_s7 == 1) FCU_STOC(E_, v, (comp) ? 14 : 13); } while (0)   /* inside a 2Nx2N call of section 7 only */
#define FCU_TOC(E_, v, idx) do { if ((idx) < 11 && threadIdx.x == 0) (E_).C->prof[idx] += (unsigned long long)(clock64() - v); } while (0)
#define FCU_COUNT(E_, idx, n) do { } while (0)
#elif defined(FCU_PROFILE_PIX)   /* pixel-stage variant: slots 1, 2, 8 and 10 keep their sections; the other twelve belong to the pixel stages before / after the quantiser of pu_first_pass_batched and tu_trial, split by block size (FCU_PTOC, slot = FCU_PIX_SLOT(part, log2)) */
#define FCU_PTIC(v) long long v = clock64()
#define FCU_PRST(v) (v = clock64())
#define FCU_PIX_SLOT(part, log2) ((int)((0x0fedcb976543ull >> (4 * ((part) * 3 + ((log2) >= 4 ? 2 : (log2) - 2)))) & 15))   /* part 0 / 1 = first pass before / after, 2 / 3 = tu_trial before / after: 3 4 5, 6 7 9, 11 12 13, 14 15 0 */
#define FCU_PTOC(E_, v, idx) do { if (threadIdx.x == 0) (E_).C->prof[idx] += (unsigned long long)(clock64() - v); v = clock64(); } while (0)
#define FCU_TOC(E_, v, idx) do { if (((idx) == 1 || (idx) == 2 || (idx) == 8 || (idx) == 10) && threadIdx.x == 0) (E_).C->prof[idx] += (unsigned long long)(clock64() - v); } while (0)
#define FCU_COUNT(E_, idx, n) do { } while (0)
#else
#define FCU_TOC(E_, v, idx) do { if (threadIdx.x == 0) (E_).C->prof[idx] += (unsigned long long)(clock64() - v); } while (0)
#define FCU_COUNT(E_, idx, n) do { (E_).C->prof[idx] += (unsigned long long)(n); } while (0)
#endif
#else
#define FCU_TIC(v) do { } while (0)
#define FCU_TOC(E_, v, idx) do { } while (0)
#define FCU_COUNT(E_, idx, n) do { } while (0)
#endif
#ifndef FCU_QTOC
#define FCU_QTIC(v) do { } while (0)
#define FCU_QTOC(E_, v, idx) do { } while (0)
#endif
#ifndef FCU_ITOC
#define FCU_ITOC(E_, v, idx) do { } while (0)
#endif
#ifndef FCU_MTOC
#define FCU_MTOC(E_, v, idx) do { } while (0)
#endif
#ifndef FCU_PTOC
#define FCU_PTIC(v) do { } while (0)
#define FCU_PRST(v) do { } while (0)
#define FCU_PTOC(E_, v, idx) do { } while (0)
#endif
#ifndef FCU_STOC
#define FCU_STOC(E_, v, idx) do { } while (0)
#define FCU_SPATH(E_, path) do { } while (0)
#define FCU_S7_COEFF(E_, v, comp) do { } while (0)
#endif

#include "fcu_tables.h"

/* hot tables mirrored in LDS (the per-bin cost/transition table is read once per context-coded bin and several
 * times per RDOQ coefficient; on-chip reads keep the vector-memory pipeline for the scratch traffic) */
struct HotTables { uint32_t bin[256]; uint16_t scan[3][16]; uint8_t scan_cg8[3][4]; uint8_t ctx_ind_map4x4[16]; uint8_t group_idx[32];
                   uint64_t scan4_nib[3], map4_nib; uint32_t cnt_bits[4]; };   /* 4x4 scans / 4x4 sig-ctx map as nibbles, sig-ctx counts per pattern as 2-bit fields */
#ifdef FCU_EMU
static HotTables g_hot;
#else
__shared__ HotTables g_hot;
#endif

#if defined(FCU_PROFILE_RQT) && !defined(FCU_EMU)     /* lane 0 of the lane-private RDOQ (the luma variant of an inter TU): slots 11..15 */
#define FCU_RTIC(v) long long v = clock64()
#define FCU_RTOC(P_, v, idx) do { if (threadIdx.x == 0) { ((Chain *)((char *)&(P_) - __builtin_offsetof(Chain, p)))->prof[idx] += (unsigned long long)(clock64() - v); v = clock64(); } } while (0)
#elif defined(FCU_PROFILE_RDOQ) && (FCU_PROFILE_RDOQ + 0) == 2 && !defined(FCU_EMU)      /* -DFCU_PROFILE_RDOQ=2: lane 0 of the lane-private RDOQ, rdoq() */
#define FCU_RTIC(v) long long v = clock64()
#define FCU_RTOC(P_, v, idx) do { if (threadIdx.x == 0) { ((Chain *)((char *)&(P_) - __builtin_offsetof(Chain, p)))->prof[idx] += (unsigned long long)(clock64() - v); v = clock64(); } } while (0)
#else
#define FCU_RTIC(v) do { } while (0)
#define FCU_RTOC(P_, v, idx) do { } while (0)
#endif
/* -DFCU_PROFILE -DFCU_PROFILE_RDOQ=3: the passes of rdoq_wave, five timers (0 set-up + uncoded tail, 1 main walk with its record
 * stores, 2 last-position search, 3 sign pass, 4 sign hiding + last level) by block size (4x4, 8x8, larger): timer t of size
 * class s in slot 3 t + s, moved up by one from 10 on (slot 10 stays the CTU total).  tests/prof_run_rdoq_tail.py prints them. */
#if defined(FCU_PROFILE_RDOQ) && (FCU_PROFILE_RDOQ + 0) == 3 && !defined(FCU_EMU)
#define FCU_WTIC(v) long long v = clock64()
#define FCU_WTOC(P_, v, t, log2) do { if (threadIdx.x == 0) { const int s_ = (t) * 3 + ((log2) >= 4 ? 2 : (log2) - 2); \
    ((Chain *)((char *)&(P_) - __builtin_offsetof(Chain, p)))->prof[s_ + (s_ >= 10)] += (unsigned long long)(clock64() - v); } v = clock64(); } while (0)
#else
#define FCU_WTIC(v) do { } while (0)
#define FCU_WTOC(P_, v, t, log2) do { } while (0)
#endif
/* -DFCU_PROFILE -DFCU_PROFILE_RDOQ=4: the coefficient loop of rdoq() on lane 0, by kind of iteration.  The ticks between two
 * iteration tops go to the kind of the iteration they follow: 1 = no lane of the batch has a candidate level (uiMaxAbsLevel 0
 * on every active lane), 2 = at least one lane takes the level choice; 0 = the head and tail of a coefficient group.  Inside the
 * level choice, when lane 0 itself takes it: the level choice (xGetCodedLevel), the rates of rateIncUp / rateIncDown, and the
 * record store with the c1 / c2 / Rice update.  Sums stay in registers and reach the chain once per call: slots 0, 11, 12 =
 * group / short / long iterations and 13 = level choice, each ticks + (count << 40); 14, 15 = rates, store + update; 1 = the
 * call up to the end of the walk + (calls << 40).  tests/prof_run_rdoq_level.py prints them.  Slot 14 stays 0: level_choice() forms
 * the rates in the pass of the level choice, and with -DFCU_RDOQ_LEVELS_REF rdoq() calls level_choice_ref() as rdoq_wave() does,
 * so level choice and rates are one section (13) in that build too. */
#if defined(FCU_PROFILE_RDOQ) && (FCU_PROFILE_RDOQ + 0) == 4 && !defined(FCU_EMU)
struct LvProf { long long t0, t, ts; unsigned long long grp, sht, lng, s0, s1, s2; unsigned n_grp, n_sht, n_lng, n_own; int kind; };
#define FCU_LV_BEGIN(L_) LvProf L_ = { }; L_.t0 = L_.t = clock64()
#define FCU_LV_TOP(L_, next) do { const long long n_ = clock64(); const unsigned long long d_ = (unsigned long long)(n_ - L_.t); \
    if (L_.kind == 0) { L_.grp += d_; L_.n_grp++; } else if (L_.kind == 1) { L_.sht += d_; L_.n_sht++; } else { L_.lng += d_; L_.n_lng++; } \
    L_.t = n_; L_.kind = (next); } while (0)
#if defined(__HIP_DEVICE_COMPILE__)
#define FCU_LV_LONG(L_, cand) do { if (__builtin_amdgcn_ballot_w64(cand)) L_.kind = 2; } while (0)
#else                                                         /* host pass over the device code: parsed, never run */
#define FCU_LV_LONG(L_, cand) do { if (cand) L_.kind = 2; } while (0)
#endif
#define FCU_LV_OWN(L_) do { L_.ts = clock64(); L_.n_own++; } while (0)
#define FCU_LV_SEC(L_, acc) do { const long long n_ = clock64(); L_.acc += (unsigned long long)(n_ - L_.ts); L_.ts = n_; } while (0)
#define FCU_LV_END(P_, L_) do { if (threadIdx.x == 0) { unsigned long long *f_ = ((Chain *)((char *)&(P_) - __builtin_offsetof(Chain, p)))->prof; \
    f_[0] += L_.grp + ((unsigned long long)L_.n_grp << 40); f_[11] += L_.sht + ((unsigned long long)L_.n_sht << 40); f_[12] += L_.lng + ((unsigned long long)L_.n_lng << 40); \
    f_[13] += L_.s0 + ((unsigned long long)L_.n_own << 40); f_[14] += L_.s1; f_[15] += L_.s2; f_[1] += (unsigned long long)(clock64() - L_.t0) + (1ull << 40); } } while (0)
#else
#define FCU_LV_BEGIN(p) do { } while (0)
#define FCU_LV_TOP(p, next) do { } while (0)
#define FCU_LV_LONG(p, cand) do { } while (0)
#define FCU_LV_OWN(p) do { } while (0)
#define FCU_LV_SEC(p, acc) do { } while (0)
#define FCU_LV_END(P_, p) do { } while (0)
#endif
namespace fcu {

/* ---- constants ------------------------------------------------------------------------ */
enum { CTU = 64, MAXDEPTH = 3, NPART = 256, LOG2_MAXTU = 5, LOG2_MINTU = 2, TU_MAXDEPTH_INTRA = 3 };
enum { SIZE_2Nx2N = 0, SIZE_2NxN = 1, SIZE_Nx2N = 2, SIZE_NxN = 3, SIZE_2NxnU = 4, SIZE_2NxnD = 5, SIZE_nLx2N = 6, SIZE_nRx2N = 7, SIZE_NONE = 8, MODE_INTER = 0, MODE_INTRA = 1, MODE_NONE = 2 };
enum { SLICE_I = 0, SLICE_P = 1 };
enum { PLANAR = 0, DC = 1, HOR = 10, VER = 26, DM_CHROMA = 36 };
/* context layout (counts: TLibCommon/ContextTables.h:49-161) */
enum { CTX_SPLIT = 0, CTX_PARTSIZE = 3, CTX_INTRA_LUMA = 4, CTX_CHROMA_PRED = 5, CTX_CBF_LUMA = 6, CTX_CBF_CHROMA = 11,
       CTX_SUBDIV = 16, CTX_SIGCG = 19, CTX_SIG = 23, CTX_LASTX = 67, CTX_LASTY = 97, CTX_ONE = 127, CTX_ABS = 151,
       CTX_TSKIP = 157, NCTX_INTRA = 160,
       /* inter syntax of P slices, appended: skip flag (3), merge flag, merge index, pred mode, part-size contexts 1..3,
        * mvd (2), ref idx (2), mvp idx, rqt root cbf, pad */
       CTX_SKIP = 160, CTX_MERGE_FLAG = 163, CTX_MERGE_IDX = 164, CTX_PRED_MODE = 165, CTX_PARTSIZE1 = 166, CTX_MVD = 169,
       CTX_REF = 171, CTX_MVP_IDX = 173, CTX_ROOT_CBF = 174, NCTX = 176 };
enum { CI_CURR_BEST = 0, CI_NEXT_BEST, CI_TEMP_BEST, CI_CHROMA_INTRA, CI_QT_TRAFO_TEST, CI_QT_TRAFO_ROOT, CI_NUM };
enum { MEMO_K = 6, MEMO_POOL = 6144 + 1536 + 384 + 96 };    /* slots per depth; levels (or residual samples) of one slot of every depth: 1.5 * (64 >> d)^2 */
enum { MAXVC = 20, MAXLC = 16, POOL = 5120 };   /* MAXVC candidate variants of a batch, MAXLC lane-private coders (the bit count runs in rounds) */
/* <= 8 RMD survivors + 2 MPMs (iMode, TEncSearch.cpp:2407-2428), x2 transform-skip variants; 5 x 32x32 */
#define FCU_MAX_DOUBLE 1.7e+308

/* coder state copied by TEncSbac::load/store (TEncSbac.cpp:397-426) */
struct Cabac { uint8_t ctx[NCTX]; uint64_t frac; uint32_t bins; uint32_t pad_; };

struct Params {
  int width, height, qp, qp_c, slice_ctus, slice_type;
  int transform_skip, ts_fast, sign_hiding, strong_smoothing;
  double lambda, sqrt_lambda, chroma_weight, rdoq_lambda[3];
  double err_scale[2][4];     /* [luma/chroma][log2-2]   setErrScaleCoeff, TComTrQuant.cpp:3018-3040 */
  long long rd_factor[2];     /* sign-hiding rdFactor,   TComTrQuant.cpp:2444-2447 */
  /* P slices (BASELINE configs[4]) */
  int search_range, fast_enc, had_me, fdm, max_merge_cand, fast_search;
  int tmvp;                    /* TMVPMode: temporal merge / AMVP candidate from Chain::col */
  int amp;                     /* asymmetric motion partitions (AMP with AMP_ENC_SPEEDUP + AMP_MRG, TEncCu.cpp:381-450,836-943) */
  int rdoq, rdoq_ts;           /* RDOQ / RDOQTS: 0 = the plain quantiser of xQuant (quant_plain) for blocks without / with transform skip */
  uint32_t lambda_motion_sad;  /* m_uiLambdaMotionSAD = floor(65536 * sqrt(lambda)), TComRdCost.cpp:194-219 */
  int cabac_b_table;           /* P slice initialised from the B-slice context tables (encCABACTableIdx == B_SLICE, TEncSbac.cpp:111-115) */
};

/* per-chain descriptor in HBM */
struct Chain {
  const uint8_t *org[3];
  uint8_t *rec[3];
  int stride[3];
  /* P slice: reference picture (list 0, index 0), padded planes: ref[c] points at sample (0,0), the border is
   * replicated FCU_REF_MARGIN (>> 1 for chroma) samples to every side (TComPicYuv::extendPicBorder) */
  const uint8_t *ref[3];
  int ref_stride[3];
  fcu_ctu_out *out;
  Params p;
  int w_ctu, h_ctu, n_ctu;
  int next_ctu, end_ctu;       /* the chain decides CTUs [next_ctu, end_ctu): the whole frame, or whole slices of it */
  Cabac state;                 /* m_pppcRDSbacCoder[0][CI_CURR_BEST] between CTUs */
  unsigned long long n_tu_trials;
  unsigned long long prof[16];
  /* fork decision state (tools_YS.cpp): frame state, per-depth switches of the Naive model, OBF count map, g_iVerResult */
  int dec_state, depth_exception, obf_stride;
  uint8_t sw_skip[4], sw_term[4];
  const int16_t *obf;
  double ver[4][6];
  const fcu_ctu_out *col;      /* TMVP: the reference picture's fcu_ctu_out array (its motion field), or null */
  int int_mv[2];               /* (kept for layout; the TZ start vectors live in int_mv_r below) */
  fcu_pu_trace *pu_trace;      /* optional [n_ctu][FCU_PUS_PER_CTU] record of the luma search (fcu_chain_set_pu_trace) */
  /* reference picture list 0 of a P slice: refs[r] = padded planes of RefPicList0[r] (refs[0] == ref; all share ref_stride),
   * ref_poc[r] its POC, poc the current picture's, n_ref = num_ref_idx_l0_active (1..FCU_MAX_REF).  col_poc / col_ref_poc: the
   * collocated picture (= RefPicList0[0]) and the POCs its own list 0 named, for the TMVP scaling (xGetColMVP).
   * int_mv_r[r] = m_integerMv2Nx2N[list 0][r]: integer vector of the chain's last 2Nx2N motion search on that reference. */
  const uint8_t *refs[FCU_MAX_REF][3];
  int n_ref, poc, ref_poc[FCU_MAX_REF], col_poc, col_ref_poc[FCU_MAX_REF];
  int int_mv_r[FCU_MAX_REF][2];
  /* WaveFrontSynchro row chain (fcu_wpp_begin / fcu_wpp_begin_p / fcu_wpp_begin_slices), written by the host only: wpp = 1 binds
   * the chain to one CTU row of a picture, wpp_above = chain index of the row above, or -1 for a row that starts a slice (row 0;
   * with slices of whole rows, p.slice_ctus = R * w_ctu, every R-th row): such a row waits for nothing, loads no contexts and
   * inherits no search state.  wpp_sync_in / wpp_sync_out = the sync slots (NCTX context bytes,
   * m_entropyCodingSyncContextState) of the row above (null with wpp_above -1, never read then) / of this row.  The slots themselves are device
   * memory of the context (fcu_kernels.hip), not part of the descriptor: no host copy of the descriptor ever overwrites them. */
  int wpp, wpp_above;
  const uint8_t *wpp_sync_in;
  uint8_t *wpp_sync_out;
  /* Tile of a one-slice picture (fcu_tiles_begin / fcu_wpp_begin_tiles), written by the host only: the CTU rectangle
   * [tile_x0, tile_x0 + tile_w) x [tile_y0, tile_y0 + tile_h) the chain decides raster-in-tile.  next_ctu / end_ctu of the chain
   * then count CTUs INSIDE the tile (position k = CTU (tile_x0 + k % tile_w, tile_y0 + k / tile_w)); a CTU outside the rectangle
   * is no neighbour (TComDataCU::getPULeft ... CUIsFromSameSliceAndTile).  chain_bind sets the whole picture: position and
   * picture address are then the same number and nothing is masked.  The fields sit in the tail fcu_chain_set_decision copies
   * from the host descriptor, which therefore holds them too (ADVICE.md finding 4). */
  int tile_x0, tile_y0, tile_w, tile_h;
  /* Caller-supplied split labels (fcu_chain_set_labels), written by the host only: labels = the PICTURE's label array, int8 [NL]
   * in the layout fcu_decision_maps writes (level d = 0..3 one after the other, [ceil(height / s)][ceil(width / s)], s = 64 >> d),
   * or null: the Naive model on N_OBF decides.  lbl_off[d] / lbl_w[d] = element offset and row length of level d.  A CU reads
   * the label at its picture coordinates, so the slice, row and tile chains of a picture share one array.  The fields sit at the
   * end of the tail fcu_chain_set_decision copies from the host descriptor, which holds them too; fcu_chain_set_labels copies
   * them alone (CR_LABELS, fcu_host.h). */
  const int8_t *labels;
  int lbl_off[4], lbl_w[4];
  /* Optional [n_ctu][FCU_CUS_PER_CTU] record of both RD costs of every CU the search visits (fcu_chain_set_cu_trace), written by
   * the host only; the chains of a picture share one array and write disjoint CTUs.  The last field of the GPU layout, behind
   * everything the CR_* ranges of fcu_host.h name: binding it copies this pointer alone (CR_CU_TRACE). */
  fcu_cu_trace *cu_trace;
#ifdef FCU_EMU
  /* emulator only (the GPU layout has neither): bit r of wpp_mv_known = int_mv_r[r] holds HM's value (written by this row's
   * search, or taken from the caller / the row above); wpp_mv_rbw counts TZ searches that read a slot before it was known */
  int wpp_mv_known, wpp_mv_rbw;
#endif
};
enum { DEC_TRAINING = 0, DEC_VERIFYING = 1, DEC_TESTING = 2 };

/* per-depth working CU (TComDataCU best/temp objects, TEncCu.cpp:163-198) */
struct CuObj {
  double cost; uint32_t dist, bits, bins;
  int depth_cu, x, y, zidx, nparts;
  uint8_t depth[NPART]; int8_t part_size[NPART], pred_mode[NPART]; uint8_t tr_idx[NPART];
  uint8_t tskip[3][NPART], cbf[3][NPART], intra_dir[2][NPART];
  uint8_t skip[NPART], merge_flag[NPART], merge_idx[NPART], inter_dir[NPART]; int8_t mvp_idx[NPART], ref_idx[NPART];
  int16_t mv[NPART][2], mvd[NPART][2];
  alignas(16) int16_t coef[3][CTU * CTU];
};
struct Yuv16 { int16_t y[64 * 64], u[32 * 32], v[32 * 32]; };
struct Yuv { uint8_t y[64 * 64], u[32 * 32], v[32 * 32]; };
enum { FCU_REF_MARGIN = 80 };                     /* luma border of a reference picture: g_uiMaxCUWidth + 16 (TComPic::create) */
/* state of one chroma-mode trial: the mode's own reconstruction (overlay of PicYuvRec inside the CU), levels, flags */
struct ChromaModeBuf { uint8_t u[32 * 32], v[32 * 32]; alignas(16) int16_t coef[2][1024]; uint8_t cbf[2][NPART], tskip[2][NPART]; };

/* RDOQ's per-coefficient locals as one record (TComTrQuant.cpp:2082-2095) */
struct RdoqRec { double cc, cs, c0; int32_t up, dn, sd, du; };   /* pdCostCoeff, pdCostSig, pdCostCoeff0, rateIncUp/Down, sigRateDelta, deltaU */

/* per-chain scratch in HBM (L2 resident working set) */
struct alignas(16) Scratch {
  CuObj cu[4][2];
  Yuv org[4], predt[4], reco[4][2];
  Yuv qt_rec[4];                                   /* m_pcQTTempTComYuv[layer] */
  alignas(16) int16_t qt_coef[3][4][CTU * CTU];                /* m_ppcQTTempCoeff[comp][layer] */
  int16_t ts_coef[3][1024]; Yuv ts_rec; uint8_t shared_pred[3][1024];
  uint8_t tmp_tr_idx[NPART], tmp_cbf[NPART], tmp_tskip[NPART];
  ChromaModeBuf cm[5];
  Cabac slots[MAXDEPTH + 2][CI_NUM];               /* the colder snapshots (NEXT/TEMP_BEST, QT_TRAFO_*) live in L2 */
  /* candidate pools: slot v occupies [v*N*N, (v+1)*N*N) */
  uint8_t p_pred[POOL]; int16_t p_resi[POOL]; int32_t p_tmp[POOL]; int32_t p_tcoef[POOL]; uint8_t p_rec[POOL];
  /* scan-order domain of a batch: element (scan position sp, slot v) at [sp * nslots + v] */
  int32_t p_lscan[POOL]; int16_t p_qscan[POOL];
  /* RDOQ locals (TComTrQuant.cpp:2082-2095), same interleaving */
  RdoqRec r_rec[POOL]; double r_cg[MAXVC * 64];
  /* 64x64 first pass: per-candidate reconstruction and levels of the whole PU (candidates advance side by side) */
  uint8_t c64_rec[5][CTU * CTU]; alignas(16) int16_t c64_coef[5][CTU * CTU];
  Cabac c64_state[5][4]; uint32_t c64_distk[5][4];   /* ... and its coder / distortion after each of the four TUs */
  /* inter: residual of the CU, chosen residual, residual per RQT layer (m_pcQTTempTComYuv holds residuals here), m_tmpYuvPred,
   * the nine interpolated blocks of a fractional refinement round */
  Yuv16 resi_cu, resi_best, qt_resi[4];
  Yuv tmp_pred;
  uint8_t me_pred[9][CTU * CTU];
  int16_t me_h[3][72 * 64];                        /* sub-sample refinement: the three horizontally filtered planes of a round (14-bit intermediates, xExtDIFUpSamplingH/Q) */
  int par_ps[4];                                   /* eParentPartSize of the CU being compressed at each depth (SIZE_NONE: intra / none); read only with AMP on */
  /* Residual-coding memo of the inter candidates of ONE CU (encode_res_and_calc_rd_inter_cu): the inter RQT is a function of
   * the CU's prediction (= its per-partition motion field), the source block and the coder snapshot [depth][CI_CURR_BEST],
   * none of which change between the candidates of a CU except the motion.  Candidates whose motion field equals an earlier
   * one's (merge candidates with equal vectors, Nx2N / 2NxN / AMP shapes that found the 2Nx2N vector twice) reuse its transform
   * tree, levels and residual instead of searching them again.  Slots are per depth, FIFO, cleared when a CU starts. */
  int memo_valid[4][MEMO_K], memo_next[4], memo_zero[4][MEMO_K];
  int16_t memo_mv[4][MEMO_K][NPART][2]; int8_t memo_ref[4][MEMO_K][NPART];
  uint8_t memo_tr_idx[4][MEMO_K][NPART], memo_cbf[4][MEMO_K][3][NPART], memo_tskip[4][MEMO_K][3][NPART];
  alignas(16) int16_t memo_coef[MEMO_K * MEMO_POOL], memo_resi[MEMO_K * MEMO_POOL];
};

/* tx0 .. ty1: the chain's tile in CTUs, [tx0, tx1) x [ty0, ty1) (pictures are at most a few hundred CTUs wide) */
struct Env { Chain *C; Scratch *G; int cur_ctu, slice_start; int16_t tx0, ty0, tx1, ty1; };
/* CTU (cx, cy) lies in the tile of the chain (CUIsFromSameTile of a CTU of the picture) */
FCU_DEV int in_tile(const Env E, int cx, int cy) { return cx >= E.tx0 && cx < E.tx1 && cy >= E.ty0 && cy < E.ty1; }
/* transform unit descriptor (TComTU / TComTURecurse, TLibCommon/TComTU.cpp:47-207) */
struct TU { int log2, tr_depth, part, nparts, x, y, off_y, cw, cwo, cx, cy, c_tr_depth, c_code_all, off_c, cu_depth, plast; };

/* per-chain LDS */
struct Shared {
  /* hot coders, one LDS array so that coder ids index it directly:
   * [CAB_GOON] go-on coder, [CAB_CUR0+d] = [depth][CI_CURR_BEST], [CAB_LANE0+k] lane-private trial coders,
   * [CAB_LUMA] the coder after the walk of the luma encoding est_intra_pred_luma chose for a 2Nx2N CU */
  Cabac cab[1 + (MAXDEPTH + 1) + MAXLC + 1];
  uint8_t ref5[5][68]; int dc5[5]; uint32_t cm_dist[5];     /* chroma: per-mode reference samples (N <= 16) */
  /* Three tenants that are never live together (the union is 1 280 B, the size of rq_grp;
   * 8 688 B of LDS per chain in all = 16 chains per CU, four waves per SIMD):
   *  - reference samples of the block being predicted (+ the availability flags that build them): dead once the
   *    predictions of the batch are in the candidate pools, i.e. before any quantisation;
   *  - per lane the level_double values of the coefficient group a lane-private RDOQ is walking;
   *  - the |level| lists of the lane-private bit counters. */
  union {
    int16_t lane_abs[MAXLC][32];                    /* per lane: |level| list of the coefficient group being coded [0..15], the group's levels [16..31] */
    int32_t rq_grp[16][MAXVC];                      /* lane-private RDOQ: the group being walked, position-major (a read by all lanes is conflict-free) */
    struct {
      int32_t colsum[128];                          /* availability flags of build_ref / chroma_leaf_refs5 */
      union {                                       /* luma reference samples / scratch copy of the chroma sets */
        struct { uint8_t ref[264], reff[264]; };
        uint8_t ref5b[5][68];
      };
    };
  };
  uint32_t sad[36];                                 /* RMD SATD per mode; [35] SSE accumulator of a TU trial */
  int dc;
  /* hand-over of ref / reff / dc from rmd() to the first pass of the same PU: ref_key(x, y, log2) of the luma block whose
   * samples they hold, or -1.  Set by rmd() only; build_ref and chroma_leaf_refs5 (which overwrite the arrays) clear it, the
   * first pass consumes it.  Anyone who finds -1, or another block's key, builds the samples himself. */
  int ref_tag;
  int best_idx[4], reco_best_idx[4];               /* which of cu[d][0/1] / reco[d][0/1] is "best" */
  /* PU / TU mailbox written by serial blocks */
  union {
    struct { int rd_mode[12]; int n_rd; int preds[3]; int n_mpm; };   /* luma PU */
    int uni[8];                                                       /* chroma leaf: transform-skip choice per mode */
  };
/* est: the estBit table of the coder RDOQ prices against, bits[ctx][bin] (TEncSbac.cpp:1722-1956), lives in the upper
   * lane coders (FCU_EST below): it is built and read before the bit count that loads them; [159] (the pad context) carries rqt_root_cbf for inter luma */
  union {                                           /* intra candidate batch / inter mailboxes: never live at the same time */
    struct {
      uint8_t vc_slot[MAXVC];                       /* lane coder that holds a variant's state after the bit count */
      int vc_abs[MAXVC], vc_lsp[MAXVC], vc_last[MAXVC]; uint32_t vc_dist[MAXVC]; uint32_t vc_bits[MAXVC]; double vc_cost[MAXVC];   /* chroma uses [10..14] of vc_dist */
    };
    struct {
      uint32_t acc[16];                             /* wave-reduced sums (SAD / SSE / Hadamard per candidate or variant) */
      unsigned long long me_best;                   /* (cost << 32) | raster index of the best integer position */
      int mrg_mv[5][2], mrg_ref[5], amvp[2][2];     /* merge candidates, AMVP candidates of the PU being searched */
      int iv_abs[6], iv_lsp[6], iv_top[6]; uint32_t iv_dist[6], iv_bits[6];   /* inter TU variants: Y, Y-ts, Cb, Cb-ts, Cr, Cr-ts */
      int it_abs[3], it_ts[3]; uint32_t it_dist[3]; /* chosen variant per component */
      double iq_cost[5]; uint32_t iq_bits[5], iq_dist[5], iq_zero;   /* xEstimateInterResidualQT accumulators per recursion level */
      int16_t tz_x[16], tz_y[16]; uint8_t tz_pt[16], tz_d[16]; int tz_n;          /* TZ search: the positions of the round in flight (test order) */
      uint32_t tz_best; int tz_bx, tz_by, tz_dist, tz_round, tz_point;               /* IntTZSearchStruct */
      int mrg_buf[5], best_is_skip, me_out[4];      /* xCheckRDCostMerge2Nx2N bookkeeping; motion_estimation results (mvx, mvy) */
    };
  };
  int pu_best_vc, pu_best_mode, pu_nvc; uint32_t pu_best_dist; double pu_best_cost;
  /* sequential TU trial mailbox */
  int t_abs, t_lsp, t_last; uint32_t t_dist;
  int rw_abs, rw_lsp;                               /* rdoq_wave's result */
  /* RQT recursion results */
  double q_cost[4]; uint32_t q_dist[4];
  /* chroma search */
  int c_best_mode; uint32_t c_best_dist; double c_best_cost; int c_modes[5];
  uint32_t c_dist;
  Env env;
  /* explicit stacks of the serial tree walkers (a private array indexed by the stack pointer would live in scratch memory) */
  TU wk_st[4]; int wk_ci[4]; int wk_part[4], wk_child[4];
  double cand_cost[12];                             /* RMD candidate costs (CandCostList, TEncSearch.cpp:2289) */
  uint32_t c64_dist[5]; uint8_t c64_cbf[5][4]; int c64_valid;      /* 64x64 first pass: per-candidate distortion / cbf of its four TUs */
  uint64_t q_frac[5], t_frac;                       /* exact (Q15) bit counts of the chosen RQT subtrees per recursion level / of the last walk */
  uint32_t q_bins[5], t_bins;                       /* ... and their bin counts */
  /* luma-final state of a 2Nx2N intra CU, from est_intra_pred_luma to check_rd_cost_intra: cab[CAB_LUMA] holds the contexts,
   * lf_frac the Q15 count (with the remainder the search started from), lf_bins the bins; lf_valid = 0: none, walk the CU */
  uint64_t lf_frac; uint32_t lf_bins; int lf_valid;
  double dec_j0, dec_j1; int dec_cnt, dec_flip;     /* fork hooks: J0 / J1 / Num_OBF / bPartition_True of the CU being closed */
#ifdef FCU_PROFILE_CUSYN
  int prof_s7;                                      /* section 7 in flight: 1 = of a 2Nx2N CU, 2 = of an NxN CU, 0 = none (the CTU replay walks the same code) */
#endif
};

enum { CAB_GOON = 0, CAB_CUR0 = 1, CAB_LANE0 = 1 + (MAXDEPTH + 1), CAB_LUMA = CAB_LANE0 + MAXLC };
/* RDOQ's rate table (NCTX_INTRA x 2 words) borrows lane coders [MAXLC-7, MAXLC): est_build() fills it before the RDOQ of a
 * batch, the bit count that follows is the first to load those coders, and nothing reads the table afterwards. */
enum { EST_CODERS = 7 };
static_assert(EST_CODERS * sizeof(Cabac) >= NCTX_INTRA * 2 * sizeof(uint32_t) && EST_CODERS <= MAXLC, "est table does not fit its lane coders");
#define FCU_EST ((uint32_t *)&g_S.cab[CAB_LANE0 + MAXLC - EST_CODERS])
/* The RMD borrows the lane coders too (none is live between the PUs of a CU: a PU's winner is re-coded before the next PU's
 * RMD starts): the row-transformed lines of the (mode, line) items of one wave iteration, 64 x 8 int16, and the 35 mode costs
 * the candidate ranking reads. */
enum { RMD_STAGE_BYTES = 64 * 8 * 2, RMD_COST_BYTES = 35 * 8 };
static_assert(RMD_STAGE_BYTES + RMD_COST_BYTES <= MAXLC * sizeof(Cabac) && (CAB_LANE0 * sizeof(Cabac)) % 8 == 0, "RMD staging does not fit the lane coders");
#define FCU_RMD_STAGE ((int16_t *)&g_S.cab[CAB_LANE0])
#define FCU_RMD_COST ((double *)((char *)&g_S.cab[CAB_LANE0] + RMD_STAGE_BYTES))
FCU_DEV int ref_key(int px, int py, int log2) { return px | (py << 13) | (log2 << 26); }
#ifdef FCU_EMU
static Shared g_S;
#else
__shared__ Shared g_S;
#endif
/* the wave's environment lives in LDS (g_S.env): non-inlined functions fetch it (to scalar registers) instead of
 * receiving it as six vector-register arguments that would be spilled around every call */
FCU_DEV Env env_get() { return FCU_UNI(g_S.env); }
FCU_DEV Cabac *slot_ptr(const Env E, int d, int ci) { return ci == CI_CURR_BEST ? &g_S.cab[CAB_CUR0 + d] : &E.G->slots[d][ci]; }


/* ======================================================================================== */
/* small helpers                                                                            */
/* ======================================================================================== */
FCU_DEV int part_x(int z) { return (k_z2r[z] & 15) << 2; }
FCU_DEV int part_y(int z) { return (k_z2r[z] >> 4) << 2; }
FCU_DEV int zidx_of(int lx, int ly) { return k_r2z[((ly & 63) >> 2) * 16 + ((lx & 63) >> 2)]; }
FCU_DEV int ilog2(int n) { int l = 0; while ((1 << l) < n) l++; return l; }
FCU_DEV int iabs(int v) { return v < 0 ? -v : v; }
FCU_DEV int clip8(int v) { return v < 0 ? 0 : (v > 255 ? 255 : v); }
FCU_DEV int clip3i(int lo, int hi, int v) { return v < lo ? lo : (v > hi ? hi : v); }
FCU_DEV uint8_t *yuv_plane(Yuv *b, int comp) { return comp == 0 ? b->y : (comp == 1 ? b->u : b->v); }
FCU_DEV double rd_cost(const Params &p, uint32_t bits, uint32_t dist)          /* TComRdCost::calcRdCost, TComRdCost.cpp:56-123 */
{ return FCU_FLOOR((double)dist + ((double)bits * p.lambda) + 0.5); }

FCU_DEV void tu_root(TU &t, int depth)
{
  t.log2 = 6 - depth; t.tr_depth = 0; t.part = 0; t.nparts = NPART >> (2 * depth); t.x = t.y = 0; t.off_y = 0;
  t.cw = t.cwo = (CTU >> depth) >> 1; t.cx = t.cy = 0; t.c_tr_depth = 0; t.c_code_all = 1; t.off_c = 0;
  t.cu_depth = depth; t.plast = 0;
}
FCU_DEV void tu_child(TU &c, const TU &p, int i, int processLast)
{
  const int s = 1 << (p.log2 - 1);
  c.log2 = p.log2 - 1; c.tr_depth = p.tr_depth + 1; c.cu_depth = p.cu_depth; c.plast = processLast;
  c.nparts = p.nparts >> 2; if (c.nparts < 1) c.nparts = 1;
  c.part = p.part + i * c.nparts;
  c.x = p.x + (i & 1) * s; c.y = p.y + (i >> 1) * s; c.off_y = p.off_y + i * s * s;
  const int pw = p.cwo;
  if ((pw >> 1) >= 4) {
    const int cs = pw >> 1;
    c.cw = c.cwo = cs; c.c_code_all = 1; c.c_tr_depth = p.c_tr_depth + 1;
    c.cx = p.cx + (i & 1) * cs; c.cy = p.cy + (i >> 1) * cs; c.off_c = p.off_c + i * cs * cs;
  } else {
    c.cwo = pw; c.c_code_all = 0; c.c_tr_depth = p.c_tr_depth; c.cx = p.cx; c.cy = p.cy; c.off_c = p.off_c;
    c.cw = (processLast ? (i == 3) : (i == 0)) ? pw : 0;
  }
}
/* A TU is a function of (CU depth, transform depth, first partition, processLast of the last split): non-inlined
 * functions receive this 13-bit key in one register and rebuild the descriptor with scalar arithmetic, instead of a
 * 64-byte struct passed through the stack (a scratch-memory round trip per call and lane). */
FCU_DEV uint32_t tu_key(const TU &t) { return (uint32_t)(t.cu_depth | (t.tr_depth << 2) | (t.part << 4) | (t.plast << 12)); }
FCU_DEV TU tu_of_key(uint32_t k)
{
  TU t; tu_root(t, (int)(k & 3));
  const int trd = (int)((k >> 2) & 3), part = (int)((k >> 4) & 255), pl = (int)((k >> 12) & 1);
  for (int l = 0; l < trd; l++) {
    TU c; int np = t.nparts >> 2; if (np < 1) np = 1;
    tu_child(c, t, ((part - t.part) / np) & 3, pl);
    t = c;
  }
  return t;
}
FCU_DEV int tu_part_c(const TU &t) { return t.c_code_all ? t.part : (t.part & ~3); }
FCU_DEV int tu_nparts_c(const TU &t) { return t.c_code_all ? t.nparts : t.nparts * 4; }

/* ======================================================================================== */
/* CABAC bit counter -- per-lane callable (TEncBinCoderCABACCounter.cpp:59-136)              */
/* ======================================================================================== */
FCU_DEV void cab_init(Cabac *c, int qp, int sliceType, int bTable)   /* ContextModel::init, ContextModel.cpp:56-65; TEncSbac::resetEntropy :106-156 */
{
  if (qp < 0) qp = 0; if (qp > 51) qp = 51;
  for (int i = 0; i < NCTX; i++) {
    int iv = sliceType == SLICE_P ? (bTable ? k_ctx_init_B[i] : k_ctx_init_P[i]) : k_ctx_init_I[i], slope = (iv >> 4) * 5 - 45, offset = ((iv & 15) << 3) - 16;
    int st = ((slope * qp) >> 4) + offset; st = st < 1 ? 1 : (st > 126 ? 126 : st);
    int mps = st >= 64;
    c->ctx[i] = (uint8_t)(((mps ? (st - 64) : (63 - st)) << 1) + mps);
  }
  c->frac = 0; c->bins = 0; c->pad_ = 0;
}
FCU_DEV void cab_copy(Cabac *d, const Cabac *s, int lane)     /* cooperative copy: 44 dwords */
{ const uint32_t *a = (const uint32_t *)s; uint32_t *b = (uint32_t *)d; if (lane < (int)(sizeof(Cabac) / 4)) b[lane] = a[lane]; }
FCU_DEV void cab_copy1(Cabac *d, const Cabac *s)              /* single-lane copy */
{ const uint32_t *a = (const uint32_t *)s; uint32_t *b = (uint32_t *)d; for (int i = 0; i < (int)(sizeof(Cabac) / 4); i++) b[i] = a[i]; }
/* the hot primitives take the coder id (index into g_S.cab) so that every access is a plain LDS access */
#define FCU_CB g_S.cab[cid]
FCU_DEV void cab_bin(int cid, int bin, int ctx)
{
  const uint32_t e = g_hot.bin[FCU_CB.ctx[ctx] * 2 + bin];      /* (bits << 8) | next state */
  FCU_CB.bins++;
  FCU_CB.frac += (uint64_t)(e >> 8);
  FCU_CB.ctx[ctx] = (uint8_t)e;
}
FCU_DEV void cab_ep(int cid, int n) { FCU_CB.bins += (uint32_t)n; FCU_CB.frac += (uint64_t)32768 * (uint64_t)n; }
FCU_DEV void cab_trm(int cid, int bin) { FCU_CB.bins++; FCU_CB.frac += (uint64_t)k_entropy_bits[126 ^ bin]; }
FCU_DEV void cab_reset_bits(int cid) { FCU_CB.frac &= 32767; FCU_CB.bins = 0; }
FCU_DEV uint32_t cab_bits(int cid) { return (uint32_t)(FCU_CB.frac >> 15); }
FCU_DEV int ctx_bits(int cid, int ctx, int bin) { return (int)(g_hot.bin[FCU_CB.ctx[ctx] * 2 + bin] >> 8); }
/* TEncSbac::estBit: the costs of both bins of every context of coder `cid`, one LDS word each; called by all lanes
 * in the phase before RDOQ (the contexts are frozen while RDOQ runs) */
enum { EST_ROOT_CBF = NCTX_INTRA - 1 };
FCU_DEV void est_build(int cid, int lane) { for (int i = lane; i < NCTX_INTRA * 2; i += 64) { const int cx = (i >> 1) == EST_ROOT_CBF ? CTX_ROOT_CBF : (i >> 1); FCU_EST[i] = g_hot.bin[FCU_CB.ctx[cx] * 2 + (i & 1)] >> 8; } }

/* TComDataCU::getCoefScanIdx, TComDataCU.cpp:3356-3411 */
FCU_DEV int coef_scan_idx(int dir, int log2, int comp)
{
  if (log2 > (comp ? 2 : 3)) return 0;
  if (iabs(dir - VER) <= 4) return 1;
  if (iabs(dir - HOR) <= 4) return 2;
  return 0;
}
/* coefficient-group flags: bit (cgy*wg+cgx) of a 64-bit mask (<= 8x8 groups) */
FCU_DEV int pattern_sig_ctx(uint64_t cg, int cgx, int cgy, int wg)             /* TComTrQuant.cpp:2584-2609 */
{
  if (wg <= 1) return 0;
  int r = 0, l = 0;
  if (cgx < wg - 1) r = (int)((cg >> (cgy * wg + cgx + 1)) & 1);
  if (cgy < wg - 1) l = (int)((cg >> ((cgy + 1) * wg + cgx)) & 1);
  return r + (l << 1);
}
FCU_DEV int sig_cg_ctx(uint64_t cg, int cgx, int cgy, int wg)                  /* TComTrQuant.cpp:2949-2969 */
{
  int r = 0, l = 0;
  if (cgx < wg - 1) r = (int)((cg >> (cgy * wg + cgx + 1)) & 1);
  if (cgy < wg - 1) l = (int)((cg >> ((cgy + 1) * wg + cgx)) & 1);
  return (r + l) != 0;
}
FCU_DEV int first_sig_ctx(int log2, int scan, int ch)                          /* TComChromaFormat.cpp:129-155 */
{ if (log2 == 2) return 0; if (log2 == 3) return 9 + ((scan != 0 && !ch) ? 6 : 0); return ch ? 12 : 21; }
FCU_DEV int sig_ctx_inc(int pattern, int first, int pos, int log2, int ch)     /* TComTrQuant.cpp:2619-2718 */
{
  const int py = pos >> log2, px = pos - (py << log2);
  if (px + py == 0) return 0;
  int offset;
  if (log2 == 2) offset = g_hot.ctx_ind_map4x4[4 * py + px];
  else {
    int cnt; const int xs = px & 3, ys = py & 3;
    if (pattern == 0) { int t = xs + ys; cnt = (t >= 3) ? 0 : ((t >= 1) ? 1 : 2); }
    else if (pattern == 1) cnt = (ys >= 2) ? 0 : ((ys >= 1) ? 1 : 2);
    else if (pattern == 2) cnt = (xs >= 2) ? 0 : ((xs >= 1) ? 1 : 2);
    else cnt = 2;
    offset = ((((px >> 2) + (py >> 2)) > 0) ? (ch ? 0 : 3) : 0) + cnt;
  }
  return first + offset;
}
FCU_DEV int coef_remain_bins(uint32_t symbol, uint32_t rparam)             /* bypass bins of xWriteCoefRemainExGolomb, TEncSbac.cpp:338-391 */
{
  int code = (int)symbol;
  if (code < (3 << rparam)) return (int)(((uint32_t)code >> rparam) + 1) + (int)rparam;
  uint32_t length = rparam;
  code -= 3 << rparam;
  while (code >= (1 << length)) code -= 1 << (length++);
  return (int)(3 + length + 1 - rparam) + (int)length;
}
#ifdef FCU_EMU
/* test bookkeeping of the emulator (tests/test_walk_prefetch_emu.py, tests/emu/walk_asan_driver.cpp; SMALL_*:
 * tests/test_small_tu_emu.py, the edge cases of the 4x4 / 8x8 trials): how often the lane-private
 * walks met their edge cases, and the bounds of the pool rdoq() loads from (set by compress_ctu): every address its group loads
 * form is checked against them, because the pools are members of one Scratch block and no sanitizer sees one run into the next */
enum { WALK_RDOQ_CALLS, WALK_RDOQ_TOP_IS_GROUP0, WALK_RDOQ_AHEAD_GROUPS, WALK_RDOQ_ONLY_GROUP0, WALK_RDOQ_ONLY_LAST_GROUP, WALK_RDOQ_ALL_ZERO,
       WALK_BITS_CALLS, WALK_BITS_ONE_EMPTY_RUN_BETWEEN, WALK_BITS_SECOND_ROUND, WALK_N };
enum { SMALL_TS_WINNER, SMALL_ALL_ZERO, SMALL_BATCH_OVER_16, SMALL_CHROMA_4X4, SMALL_N };
/* TAIL_*: tests/test_rdoq_tail_emu.py, the passes of rdoq_wave after its walk.  Sign hiding changed a level in a 4x4 block / in a
 * group below the top one of an 8x8 block / in a block of 16x16 or more; two positions tied for the smallest cost; sign hiding
 * cleared the last level; the last-position search zeroed the block; costZeroCG zeroed a group of an 8x8 block; an 8x8 block whose
 * top candidate level is in group 0; a chroma block; a call from the inter RQT; no position of a group had a finite cost */
enum { TAIL_SH_4X4, TAIL_SH_8X8_LOW, TAIL_SH_BIG, TAIL_SH_TIE, TAIL_SH_CLEARED_LAST, TAIL_LAST_ZERO, TAIL_CG_ZEROED_8X8, TAIL_TOP_IN_GROUP0_8X8,
       TAIL_CHROMA, TAIL_INTER, TAIL_SH_NO_FINITE, TAIL_N };
extern "C" { __attribute__((weak)) unsigned long long fcu_emu_walk_cnt[WALK_N]; __attribute__((weak)) unsigned long long fcu_emu_small_cnt[SMALL_N];
             __attribute__((weak)) unsigned long long fcu_emu_tail_cnt[TAIL_N]; }
#define FCU_SMALL_COUNT(i, n) (fcu_emu_small_cnt[i] += (unsigned long long)(n))
#define FCU_TAIL_COUNT(i, n) (fcu_emu_tail_cnt[i] += (unsigned long long)(n))
static const int32_t *g_emu_lscan_lo = nullptr, *g_emu_lscan_hi = nullptr;
#define FCU_WALK_COUNT(i, n) (fcu_emu_walk_cnt[i] += (unsigned long long)(n))
#define FCU_CHECK_LSCAN(p) FCU_CHECK((const int32_t *)(p) >= g_emu_lscan_lo && (const int32_t *)(p) < g_emu_lscan_hi)
#else
#define FCU_WALK_COUNT(i, n) do { } while (0)
#define FCU_SMALL_COUNT(i, n) do { } while (0)
#define FCU_TAIL_COUNT(i, n) do { } while (0)
#define FCU_CHECK_LSCAN(p) do { } while (0)
#endif
/* TEncSbac::codeCoeffNxN (+codeTransformSkipFlags, codeLastSignificantXY), TEncSbac.cpp:997-1535.
 * Inside the engine the levels of a TU are kept in SCAN ORDER (coef[sp * st] = level at scan position sp;
 * st = 1 in CU objects, st = number of slots in an interleaved candidate batch), so the coder walks memory
 * linearly.  `last` = scan position of the last non-zero level, or -1: find it here (returns at once on an
 * all-zero TU).  The significant-group flags the reference gathers in its first loop (:1255-1275) are
 * derived group by group on the way down (a group's right/below neighbours come earlier in reverse scan). */
/* ONE_LANE = 1: called by one lane (serial sections): every argument is wave-uniform */
template <int ONE_LANE>
FCU_DEV FCU_INLINE void code_coeff_body(int c, const int16_t *coef, int st, int last, int log2, int comp, int scanType, int tsFlag, const Params &P_, int16_t *absCoeff)
{
  if (ONE_LANE) { c = FCU_UNI(c); coef = FCU_UNI(coef); last = FCU_UNI(last); scanType = FCU_UNI(scanType); tsFlag = FCU_UNI(tsFlag); absCoeff = FCU_UNI(absCoeff); }
  const Params &P = *FCU_UNI(&P_);
  st = FCU_UNI(st); log2 = FCU_UNI(log2); comp = FCU_UNI(comp);
  FCU_IN_LDS(absCoeff);
  const FCU_HBM int16_t *coefg = (const FCU_HBM int16_t *)coef;
  const int ch = comp ? 1 : 0, N = 1 << log2; int n2 = N * N;
  if (last < 0 && st == 1 && n2 >= 64) {                       /* contiguous levels: skip empty runs of four groups (128 bytes) with wide loads */
    int q = (n2 >> 6) - 1;
    for (; q >= 0; q--) {
      uint32_t w[32];
      __builtin_memcpy(w, __builtin_assume_aligned((const void *)(coef + q * 64), 16), 128);   /* TU-contiguous levels start on 32-byte boundaries */
      uint32_t any = 0;
#pragma unroll
      for (int k = 0; k < 32; k++) any |= w[k];
      if (any) break;
    }
    if (q < 0) return;
    n2 = (q + 1) * 64;                                         /* the group-wise search below starts in the first non-empty run */
  }
  if (last < 0) {                                             /* find the last non-zero level, a group's sixteen loads at a time */
    for (int cg = (n2 >> 4) - 1; cg >= 0 && last < 0; cg--) {
      uint32_t nz = 0;
#pragma unroll
      for (int k = 0; k < 16; k++) nz |= (uint32_t)(coefg[(cg * 16 + k) * st] != 0) << k;
      if (nz) last = cg * 16 + 31 - __builtin_clz(nz);
    }
    if (last < 0) return;
  }
  FCU_WALK_COUNT(WALK_BITS_CALLS, 1);
#ifdef FCU_EMU
  if (log2 == 5) {                                            /* test bookkeeping: one empty 128-byte run (four groups) between two non-empty ones */
    int e[16];
    for (int q = 0; q < 16; q++) { e[q] = 1; for (int k = 0; k < 64; k++) if (q * 64 + k <= last && coef[(q * 64 + k) * st]) e[q] = 0; }
    for (int q = 1; q < (last >> 6); q++) FCU_WALK_COUNT(WALK_BITS_ONE_EMPTY_RUN_BETWEEN, e[q] && !e[q - 1] && !e[q + 1]);
  }
#endif
  /* bit/bin totals are kept in registers and added to the coder once at the end (sums commute) */
  uint64_t fr = 0; uint32_t nb = 0;
#define FCU_BIN(bin_, ctx_) do { const int cx_ = (ctx_); const uint32_t e_ = g_hot.bin[g_S.cab[c].ctx[cx_] * 2 + (bin_)]; nb++; fr += (uint64_t)(e_ >> 8); g_S.cab[c].ctx[cx_] = (uint8_t)e_; } while (0)
#define FCU_EP(n_) do { const uint32_t n__ = (uint32_t)(n_); nb += n__; fr += (uint64_t)32768 * (uint64_t)n__; } while (0)
  if (P.transform_skip && log2 == 2) FCU_BIN(tsFlag, CTX_TSKIP + ch);
  const uint16_t *scan = log2 == 2 ? &g_hot.scan[scanType][0] : k_scan + k_scan_off[scanType * 4 + log2 - 2];
  const uint8_t *scanCG = log2 <= 3 ? g_hot.scan_cg8[log2 == 2 ? 0 : scanType] : k_scan_cg + k_scan_cg_off[scanType * 4 + log2 - 2];
  const int wg = N >> 2, firstSig = first_sig_ctx(log2, scanType, ch);
  uint64_t cgflag = 0;
  const uint64_t scan4 = g_hot.scan4_nib[scanType], map4 = g_hot.map4_nib;
  const int scanPosLast = last, posLast = scan[last], lastVal = coefg[last * st];
  {
    int py = posLast >> log2, px = posLast - (py << log2);
    if (scanType == 2) { int t = px; px = py; py = t; }
    const int gx = g_hot.group_idx[px], gy = g_hot.group_idx[py], cc = log2 - 2;
    const int off = ch ? 0 : (cc * 3 + ((cc + 1) >> 2)), sh = ch ? cc : ((cc + 3) >> 2);
    const int bx = CTX_LASTX + (ch ? 15 : 0) + off, by = CTX_LASTY + (ch ? 15 : 0) + off, gmax = g_hot.group_idx[N - 1];
    int k;
    for (k = 0; k < gx; k++) FCU_BIN(1, bx + (k >> sh));
    if (gx < gmax) FCU_BIN(0, bx + (k >> sh));
    for (k = 0; k < gy; k++) FCU_BIN(1, by + (k >> sh));
    if (gy < gmax) FCU_BIN(0, by + (k >> sh));
    if (gx > 3) FCU_EP((gx - 2) >> 1);
    if (gy > 3) FCU_EP((gy - 2) >> 1);
  }
  const int baseCG = CTX_SIGCG + (ch ? 2 : 0), baseSig = CTX_SIG + (ch ? 28 : 0), lastSet = scanPosLast >> 4;
  uint32_t c1 = 1, goRice;
  int scanPosSig = scanPosLast;
  for (int sub = lastSet; sub >= 0; sub--) {
    int numNonZero = 0; const int subPos = sub << 4;
    goRice = 0;
    int lastNZ = -1, firstNZ = 16, escape = 0;
    if (scanPosSig == scanPosLast) { absCoeff[0] = (int16_t)iabs(lastVal); numNonZero = 1; lastNZ = scanPosSig; firstNZ = scanPosSig; scanPosSig--; }
    const int cgpos = scanCG[sub], cgy = cgpos / wg, cgx = cgpos - cgy * wg;
    /* the group's sixteen levels: one round of loads, parked in LDS for the serial walk below */
    int16_t *stage = absCoeff + 16;
    int any = 0;
    {
      int lv[16];
#pragma unroll
      for (int k = 0; k < 16; k++) lv[k] = coefg[(subPos + k) * st];
#pragma unroll
      for (int k = 0; k < 16; k++) { any |= lv[k]; stage[k] = (int16_t)lv[k]; }
    }
    if (sub == lastSet || sub == 0) cgflag |= 1ull << cgpos;
    else {
      if (any) cgflag |= 1ull << cgpos;
      FCU_BIN(any != 0, baseCG + sig_cg_ctx(cgflag, cgx, cgy, wg));
    }
    if ((cgflag >> cgpos) & 1) {
      const int pattern = pattern_sig_ctx(cgflag, cgx, cgy, wg);
      const uint32_t cntBits = g_hot.cnt_bits[pattern];
      const int sigBase = baseSig + firstSig + ((!ch && (cgx + cgy) > 0) ? 3 : 0);
      /* a group of a TU > 4x4 uses three significance contexts (+ DC): their states stay in registers for the group */
      uint32_t s0 = 0, s1 = 0, s2 = 0;
      if (log2 > 2) { s0 = g_S.cab[c].ctx[sigBase]; s1 = g_S.cab[c].ctx[sigBase + 1]; s2 = g_S.cab[c].ctx[sigBase + 2]; }
      for (; scanPosSig >= subPos; scanPosSig--) {
        const int v = stage[scanPosSig - subPos], sig = v != 0;
        const int p4 = (int)((scan4 >> (4 * (scanPosSig - subPos))) & 15);     /* getSigCtxInc on the packed 4x4 scan (see rdoq) */
        if (scanPosSig > subPos || sub == 0 || numNonZero) {
          if (log2 == 2) FCU_BIN(sig, baseSig + (p4 ? (int)((map4 >> (4 * p4)) & 15) : 0));
          else if (scanPosSig == 0) FCU_BIN(sig, baseSig);
          else {
            const int cnt = (int)((cntBits >> (2 * p4)) & 3);
            const uint32_t e = g_hot.bin[(cnt == 0 ? s0 : (cnt == 1 ? s1 : s2)) * 2 + sig], ns = e & 255;
            nb++; fr += (uint64_t)(e >> 8);
            if (cnt == 0) s0 = ns; else if (cnt == 1) s1 = ns; else s2 = ns;
          }
        }
        if (sig) { absCoeff[numNonZero++] = (int16_t)iabs(v); if (lastNZ == -1) lastNZ = scanPosSig; firstNZ = scanPosSig; }
      }
      if (log2 > 2) { g_S.cab[c].ctx[sigBase] = (uint8_t)s0; g_S.cab[c].ctx[sigBase + 1] = (uint8_t)s1; g_S.cab[c].ctx[sigBase + 2] = (uint8_t)s2; }
    } else scanPosSig = subPos - 1;
    if (numNonZero > 0) {
      const int signHidden = (lastNZ - firstNZ >= 4);
      const int ctxSet = (ch ? 4 : 0) + ((!ch && sub > 0) ? 2 : 0) + (c1 == 0);
      c1 = 1;
      const int baseOne = CTX_ONE + 4 * ctxSet, numC1 = numNonZero < 8 ? numNonZero : 8;
      int firstC2 = -1;
      for (int idx = 0; idx < numC1; idx++) {
        const int sym = absCoeff[idx] > 1;
        FCU_BIN(sym, baseOne + (int)c1);
        if (sym) { c1 = 0; if (firstC2 == -1) firstC2 = idx; else escape = 1; }
        else if (c1 < 3 && c1 > 0) c1++;
      }
      if (c1 == 0 && firstC2 != -1) { const int sym = absCoeff[firstC2] > 2; FCU_BIN(sym, CTX_ABS + ctxSet); if (sym) escape = 1; }
      escape = escape || (numNonZero > 8);
      FCU_EP((P.sign_hiding && signHidden) ? numNonZero - 1 : numNonZero);
      int firstCoeff2 = 1;
      if (escape)
        for (int idx = 0; idx < numNonZero; idx++) {
          const int base = (idx < 8) ? (2 + firstCoeff2) : 1;
          if (absCoeff[idx] >= base) {
            FCU_EP(coef_remain_bins((uint32_t)(absCoeff[idx] - base), goRice));
            if (absCoeff[idx] > (3 << goRice)) goRice = goRice + 1 < 4 ? goRice + 1 : 4;
          }
          if (absCoeff[idx] >= 2) firstCoeff2 = 0;
        }
    }
  }
  g_S.cab[c].frac += fr; g_S.cab[c].bins += nb;
#undef FCU_BIN
#undef FCU_EP
}

template <int ONE_LANE>
FCU_DEV FCU_NOINLINE void code_coeff_nxn(int c, const int16_t *coef, int st, int last, int log2, int comp, int scanType, int tsFlag, const Params &P, int16_t *absCoeff)
{ code_coeff_body<ONE_LANE>(c, coef, st, last, log2, comp, scanType, tsFlag, P, absCoeff); }

/* ======================================================================================== */
/* RDOQ -- per-lane callable (TComTrQuant::xRateDistOptQuant, TComTrQuant.cpp:2033-2573)     */
/* Works in the scan-order domain: the producer (forward transform phase) hands over          */
/* sign * lLevelDouble per scan position, the levels come back per scan position; element     */
/* stride `st` interleaves the candidates of a batch so that one lane-private iteration of    */
/* all lanes touches consecutive bytes.  The seven per-coefficient arrays of the reference     */
/* (:2082-2095) are one record per scan position.                                              */
/* ======================================================================================== */

/* sign(coef) * min(|coef| * quantScale, MAX_INT - (1 << (qbits-1)))   (TComTrQuant.cpp:2117-2128) */
FCU_DEV int32_t level_double(int32_t coef, int qcoef, int qbits)
{
  const long long t = (long long)iabs(coef) * qcoef, lim = 2147483647LL - (1LL << (qbits - 1));
  const int32_t l = (int32_t)(t < lim ? t : lim);
  return coef < 0 ? -l : l;
}
FCU_DEV int rdoq_qbits(int log2, int qp) { return 14 + qp / 6 + (15 - 8 - log2); }
/* uiMaxAbsLevel > 0 for this level_double() value (:2130) */
FCU_DEV int level_nonzero(int32_t ld, int qbits) { return iabs(ld) >= ((int32_t)1 << (qbits - 1)); }

struct LevelBits { int g10, g11, g20, g21; };              /* greater1 / greater2 flag costs of the current contexts */
/* The level choice of one coefficient with uiMaxAbsLevel > 0 and the rates its record needs, in one pass: xGetCodedLevel
 * (TComTrQuant.cpp:2738-2794) and the xGetICRate calls of rateIncUp / rateIncDown (:2263-2270).  Under one (goRice, c1Idx,
 * c2Idx) state xGetICRate (:2807-2881) of neighbouring levels shares everything but the level: the prefix / escape threshold
 * baseLevel, the flag bits and the Rice threshold are formed once (LevelRate), and the bypass bins of coeff_abs_level_remaining
 * come in closed form: below 3 << rice (symbol >> rice) + 1 + rice; from there on the reference's loop leaves `length` as the
 * position of the top bit of symbol - (3 << rice) + (1 << rice), one clz, and the bins are 4 + 2 length - rice.  Three rates are
 * formed, of uiMaxAbsLevel, uiMaxAbsLevel - 1 and the one outer neighbour of the chosen level; every expression that yields a
 * double has the operands and the order of the reference.  -DFCU_RDOQ_LEVELS_REF builds rdoq() and rdoq_wave() on coded_level()
 * and ic_rate() below instead, which follow the reference call by call and are the definition; -DFCU_EMU_CHECK_RDOQ_LEVELS
 * (emulator only, tests/emu/rdoq_level_emu.cpp) runs them next to level_choice() on every such coefficient and aborts unless
 * level, costs (bit patterns), rateIncUp / rateIncDown and deltaU agree. */
struct LevelRate { uint32_t base, rice, thr; int esc, one, two; };
FCU_DEV LevelRate level_rate_state(const LevelBits &b, uint32_t goRice, uint32_t c1Idx, uint32_t c2Idx)
{
  LevelRate s;
  s.base = (c1Idx < 8) ? (2 + (c2Idx < 1)) : 1; s.rice = goRice; s.thr = 3u << goRice;
  s.esc = 32768 + ((c1Idx < 8) ? b.g11 + ((c2Idx < 1) ? b.g21 : 0) : 0);   /* a level coded with a remainder: its flags are all 1 */
  s.one = 32768 + b.g10; s.two = 32768 + b.g11 + b.g20;                   /* levels 1 and 2 below baseLevel */
  return s;
}
FCU_DEV int level_rate(const LevelRate &s, uint32_t absLevel)
{
  if (absLevel >= s.base) {
    const uint32_t symbol = absLevel - s.base; uint32_t bins;
    if (symbol < s.thr) bins = (symbol >> s.rice) + 1 + s.rice;
    else { const uint32_t length = 31u - (uint32_t)__builtin_clz(symbol - s.thr + (1u << s.rice)); bins = 4 + 2 * length - s.rice; }
    return s.esc + (int)(bins << 15);
  }
  return absLevel == 0 ? 0 : (absLevel == 1 ? s.one : s.two);
}
struct LevelChoice { uint32_t level; int rup, rdn; };        /* the chosen level, rateIncUp, rateIncDown */
/* maxAbsLevel > 0; sbit0 / sbit1: the bits of the significance flag in this coefficient's context; *codedCost, *codedCostSig
 * as the caller initialised them (the reference leaves pdCostSig alone where no level beats MAX_DOUBLE) */
FCU_DEV LevelChoice level_choice(double lambda, double *codedCost, const double *codedCost0, double *codedCostSig, int32_t levelDouble, uint32_t maxAbsLevel,
                                 int sbit0, int sbit1, const LevelBits &lb, uint32_t goRice, uint32_t c1Idx, uint32_t c2Idx, int qbits, double errScale, int last)
{
  const LevelRate rs = level_rate_state(lb, goRice, c1Idx, c2Idx);
  const int rateHi = level_rate(rs, maxAbsLevel), rateLo = level_rate(rs, maxAbsLevel - 1);
  double currCostSig = 0; uint32_t bestAbs = 0;
  if (!last && maxAbsLevel < 3) {
    *codedCostSig = lambda * (double)sbit0;
    *codedCost = *codedCost0 + *codedCostSig;
  } else *codedCost = FCU_MAX_DOUBLE;
  if (!last) currCostSig = lambda * (double)sbit1;
  {
    const double err = (double)(levelDouble - ((int32_t)maxAbsLevel << qbits));
    double cost = err * err * errScale + lambda * (double)rateHi;
    cost += currCostSig;
    if (cost < *codedCost) { bestAbs = maxAbsLevel; *codedCost = cost; *codedCostSig = currCostSig; }
  }
  if (maxAbsLevel > 1) {
    const double err = (double)(levelDouble - ((int32_t)(maxAbsLevel - 1) << qbits));
    double cost = err * err * errScale + lambda * (double)rateLo;
    cost += currCostSig;
    if (cost < *codedCost) { bestAbs = maxAbsLevel - 1; *codedCost = cost; *codedCostSig = currCostSig; }
  }
  /* the chosen level is maxAbsLevel, maxAbsLevel - 1 or 0: two of the three rates of its record are rateHi and rateLo (the rate
   * of level 0 is 0), the third is the rate of the neighbour on the far side.  It is formed at one place, from a selected level
   * and ahead of the branches (unused where level 0 wins): lanes of a batch that chose differently then share one evaluation
   * where a call in each branch would run one after the other */
  LevelChoice o; o.level = bestAbs;
  const int isHi = bestAbs == maxAbsLevel;
  const int rateOut = level_rate(rs, isHi ? maxAbsLevel + 1 : (maxAbsLevel >= 2 ? maxAbsLevel - 2 : 0));
  if (bestAbs == 0) { o.rup = lb.g10; o.rdn = 0; }
  else if (isHi) { o.rup = rateOut - rateHi; o.rdn = rateLo - rateHi; }
  else { o.rup = rateHi - rateLo; o.rdn = rateOut - rateLo; }
  return o;
}
#if defined(FCU_RDOQ_LEVELS_REF) || defined(FCU_EMU_CHECK_RDOQ_LEVELS)
FCU_DEV int ic_rate(const LevelBits &b, uint32_t absLevel, uint32_t goRice, uint32_t c1Idx, uint32_t c2Idx)
{                                                          /* xGetICRate, TComTrQuant.cpp:2807-2881 */
  int rate = 32768;
  const uint32_t baseLevel = (c1Idx < 8) ? (2 + (c2Idx < 1)) : 1;
  if (absLevel >= baseLevel) {
    uint32_t symbol = absLevel - baseLevel, length;
    if (symbol < (3u << goRice)) { length = symbol >> goRice; rate += (int)((length + 1 + goRice) << 15); }
    else {
      length = goRice; symbol = symbol - (3u << goRice);
      while (symbol >= (1u << length)) symbol -= (1u << (length++));
      rate += (int)((3 + length + 1 - goRice + length) << 15);
    }
    if (c1Idx < 8) { rate += b.g11; if (c2Idx < 1) rate += b.g21; }
  } else if (absLevel == 1) rate += b.g10;
  else if (absLevel == 2) { rate += b.g11; rate += b.g20; }
  else rate = 0;
  return rate;
}
/* rateHi / rateLo: xGetICRate of the two levels tried, maxAbsLevel and maxAbsLevel - 1 (rateLo only when that level is >= 1).
 * The caller needs the rates of the chosen level and of its two neighbours afterwards (rateIncUp / rateIncDown,
 * TComTrQuant.cpp:2263-2270): two of those three are among the values computed here. */
template <class CB>
FCU_DEV uint32_t coded_level(CB cb, double lambda, double *codedCost, double *codedCost0, double *codedCostSig,
                             int32_t levelDouble, uint32_t maxAbsLevel, int ctxSig, const LevelBits &lb,
                             uint32_t goRice, uint32_t c1Idx, uint32_t c2Idx, int qbits, double errScale, int last, int *rateHi, int *rateLo)
{                                                          /* xGetCodedLevel, TComTrQuant.cpp:2738-2794 */
  double currCostSig = 0; uint32_t bestAbs = 0;
  if (!last && maxAbsLevel < 3) {
    *codedCostSig = lambda * (double)cb(ctxSig, 0);
    *codedCost = *codedCost0 + *codedCostSig;
    if (maxAbsLevel == 0) return bestAbs;
  } else *codedCost = FCU_MAX_DOUBLE;
  if (!last) currCostSig = lambda * (double)cb(ctxSig, 1);
  const uint32_t minAbs = maxAbsLevel > 1 ? maxAbsLevel - 1 : 1;
  for (int a = (int)maxAbsLevel; a >= (int)minAbs; a--) {
    double err = (double)(levelDouble - ((int32_t)a << qbits));
    const int rate = ic_rate(lb, (uint32_t)a, goRice, c1Idx, c2Idx);
    if (a == (int)maxAbsLevel) *rateHi = rate; else *rateLo = rate;
    double cost = err * err * errScale + lambda * (double)rate;
    cost += currCostSig;
    if (cost < *codedCost) { bestAbs = (uint32_t)a; *codedCost = cost; *codedCostSig = currCostSig; }
  }
  return bestAbs;
}
/* The record of one coefficient as rdoq() formed it before level_choice(): the level choice, then the rates of the chosen level's
 * neighbours (two of them are among those of the level choice). */
template <class CB>
FCU_DEV LevelChoice level_choice_ref(CB cb, double lambda, double *codedCost, double *codedCost0, double *codedCostSig, int32_t levelDouble, uint32_t maxAbsLevel,
                                     int ctxSig, const LevelBits &lb, uint32_t goRice, uint32_t c1Idx, uint32_t c2Idx, int qbits, double errScale, int last)
{
  int rateHi = 0, rateLo = 0;                                  /* xGetICRate(maxAbsLevel), (maxAbsLevel - 1) from the level choice */
  LevelChoice o; o.rdn = 0;
  o.level = coded_level(cb, lambda, codedCost, codedCost0, codedCostSig, levelDouble, maxAbsLevel, ctxSig, lb, goRice, c1Idx, c2Idx, qbits, errScale, last, &rateHi, &rateLo);
  if (o.level > 0) {                                           /* the chosen level is maxAbsLevel or maxAbsLevel - 1: one new rate, not three */
    if (o.level == maxAbsLevel) {
      o.rup = ic_rate(lb, o.level + 1, goRice, c1Idx, c2Idx) - rateHi;
      o.rdn = (maxAbsLevel > 1 ? rateLo : ic_rate(lb, 0, goRice, c1Idx, c2Idx)) - rateHi;
    } else {
      o.rup = rateHi - rateLo;
      o.rdn = ic_rate(lb, o.level - 1, goRice, c1Idx, c2Idx) - rateLo;
    }
  } else o.rup = lb.g10;
  return o;
}
#endif
#ifdef FCU_EMU_CHECK_RDOQ_LEVELS
/* test bookkeeping (tests/test_rdoq_level_emu.py, tests/emu/rdoq_level_asan_driver.cpp): the cases the level choices of a run met.
 * uiMaxAbsLevel 1 / 2 / 3 and more; the level below uiMaxAbsLevel chosen (not 0); level 0 chosen; the last position; c1Idx >= 8
 * (baseLevel 1); c2Idx >= 1; Rice parameter 0 / 4; a rate of a symbol equal to / above 3 << rice (the escape branch); a symbol
 * of 32768 or more, which the clipped levels cannot form (must stay 0) */
enum { LEVEL_MAX1, LEVEL_MAX2, LEVEL_MAX3UP, LEVEL_CHOSE_LOWER, LEVEL_CHOSE_ZERO, LEVEL_LAST, LEVEL_C1IDX_8UP, LEVEL_C2IDX_1UP, LEVEL_RICE0, LEVEL_RICE4,
       LEVEL_ESCAPE_AT, LEVEL_ESCAPE_ABOVE, LEVEL_SYMBOL_32768UP, LEVEL_N };
extern "C" { __attribute__((weak)) unsigned long long fcu_emu_level_cnt[LEVEL_N]; }
/* got / cc / cs: what level_choice() returned and left in the caller's costs (both 0 before the call, as in every caller) */
template <class CB>
static void level_choice_check(CB cb, int ctxSig, const LevelChoice &got, double cc, double c0, double cs, double lambda, int32_t levelDouble, uint32_t maxAbsLevel,
                               const LevelBits &lb, uint32_t goRice, uint32_t c1Idx, uint32_t c2Idx, int qbits, double errScale, int last)
{
  double rcc = 0, rc0 = c0, rcs = 0;
  const LevelChoice ref = level_choice_ref(cb, lambda, &rcc, &rc0, &rcs, levelDouble, maxAbsLevel, ctxSig, lb, goRice, c1Idx, c2Idx, qbits, errScale, last);
  const int32_t du = (int32_t)((levelDouble - ((int32_t)got.level << qbits)) >> (qbits - 8)), rdu = (int32_t)((levelDouble - ((int32_t)ref.level << qbits)) >> (qbits - 8));
  if (got.level != ref.level || memcmp(&cc, &rcc, 8) || memcmp(&c0, &rc0, 8) || memcmp(&cs, &rcs, 8) || got.rup != ref.rup || got.rdn != ref.rdn || du != rdu) {
    fprintf(stderr, "FCU_EMU_CHECK_RDOQ_LEVELS: level_choice differs from coded_level + ic_rate (levelDouble %d max %u rice %u c1Idx %u c2Idx %u last %d: level %u / %u, "
            "cc %a / %a, c0 %a / %a, cs %a / %a, up %d / %d, dn %d / %d, du %d / %d)\n", levelDouble, maxAbsLevel, goRice, c1Idx, c2Idx, last, got.level, ref.level,
            cc, rcc, c0, rc0, cs, rcs, got.rup, ref.rup, got.rdn, ref.rdn, du, rdu);
    abort();
  }
  unsigned long long *n = fcu_emu_level_cnt;
  n[maxAbsLevel == 1 ? LEVEL_MAX1 : (maxAbsLevel == 2 ? LEVEL_MAX2 : LEVEL_MAX3UP)]++;
  n[LEVEL_CHOSE_LOWER] += got.level > 0 && got.level == maxAbsLevel - 1; n[LEVEL_CHOSE_ZERO] += got.level == 0; n[LEVEL_LAST] += last != 0;
  n[LEVEL_C1IDX_8UP] += c1Idx >= 8; n[LEVEL_C2IDX_1UP] += c2Idx >= 1; n[LEVEL_RICE0] += goRice == 0; n[LEVEL_RICE4] += goRice == 4;
  const uint32_t base = (c1Idx < 8) ? (2 + (c2Idx < 1)) : 1;
  const uint32_t lv[3] = { maxAbsLevel, maxAbsLevel - 1, got.level == maxAbsLevel ? maxAbsLevel + 1 : (maxAbsLevel >= 2 ? maxAbsLevel - 2 : 0) };   /* the rates level_choice() formed */
  for (int k = 0; k < 3; k++) if (lv[k] >= base) {
    const uint32_t symbol = lv[k] - base;
    n[LEVEL_ESCAPE_AT] += symbol == (3u << goRice); n[LEVEL_ESCAPE_ABOVE] += symbol > (3u << goRice); n[LEVEL_SYMBOL_32768UP] += symbol >= 32768u;
  }
}
#define FCU_CHECK_LEVELS(...) level_choice_check(__VA_ARGS__)
#else
#define FCU_CHECK_LEVELS(...) do { } while (0)
#endif
/* The rules of xRateDistOptQuant that both walks apply, rdoq() inside a lane loop and rdoq_wave() from wave-uniform code or a
 * lane loop: each is defined here once.  They take and return values and touch neither the pools nor the lanes; what differs
 * between the walks (where a group is staged, where records go, the order of the running sums) stays in the walks. */
/* the loop-invariant numbers and tables of one call (:2033-2110) */
struct RdoqSetup {
  int ch, N, n2, qbits; double lambda, errScale;
  const uint16_t *scan; const uint8_t *scanCG;                 /* scan position -> block position, of coefficients / of coefficient groups */
  int wg, firstSig, sigOff, cgBase;                            /* groups per row; first significance context of the size, contexts of sig_coeff / coded_sub_block */
  uint64_t scan4, map4;                                        /* the 4x4 scan and the 4x4 significance-context map as nibbles */
};
FCU_DEV FCU_INLINE RdoqSetup rdoq_setup(const Params &P, int log2, int comp, int scanType)
{
  RdoqSetup S;
  S.ch = comp ? 1 : 0; S.N = 1 << log2; S.n2 = S.N * S.N;
  S.qbits = rdoq_qbits(log2, comp ? P.qp_c : P.qp);
  S.lambda = P.rdoq_lambda[comp];
  S.errScale = P.err_scale[S.ch][log2 - 2];
  S.scan = log2 == 2 ? &g_hot.scan[scanType][0] : k_scan + k_scan_off[scanType * 4 + log2 - 2];
  S.scanCG = log2 <= 3 ? g_hot.scan_cg8[log2 == 2 ? 0 : scanType] : k_scan_cg + k_scan_cg_off[scanType * 4 + log2 - 2];
  S.wg = S.N >> 2; S.firstSig = first_sig_ctx(log2, scanType, S.ch);
  S.sigOff = CTX_SIG + (S.ch ? 28 : 0); S.cgBase = CTX_SIGCG + (S.ch ? 2 : 0);
  S.scan4 = g_hot.scan4_nib[scanType]; S.map4 = g_hot.map4_nib;
  return S;
}
/* The significance context of the coefficient at posInCG of a group (getSigCtxInc, TComTrQuant.cpp:2619-2718).  In a TU above
 * 4x4 only DC and the three contexts sigBase + 0..2 occur: sigBase = sig_base_of() of the group, cntBits = g_hot.cnt_bits[] of
 * its neighbour pattern. */
FCU_DEV FCU_INLINE int sig_base_of(const RdoqSetup &S, int cgx, int cgy) { return S.sigOff + S.firstSig + ((!S.ch && (cgx + cgy) > 0) ? 3 : 0); }
FCU_DEV FCU_INLINE int sig_ctx_of(const RdoqSetup &S, int log2, int scanPos, int posInCG, int sigBase, uint32_t cntBits)
{
  const int p4 = (int)((S.scan4 >> (4 * posInCG)) & 15);       /* position inside the 4x4 group (raster) from the packed 4x4 scan */
  if (log2 == 2) return S.sigOff + (p4 ? (int)((S.map4 >> (4 * p4)) & 15) : 0);
  if (scanPos == 0) return S.sigOff;
  return sigBase + (int)((cntBits >> (2 * p4)) & 3);
}
/* the greater1 / greater2 / Rice state of the walk (:2190-2316): which contexts and which Rice parameter price the next level */
struct LevelState { uint32_t ctxSet = 0, c1Idx = 0, c2Idx = 0, goRice = 0; int c1 = 1, c2 = 0; };
/* the context set at the first candidate level, the block's last significant position (:2190-2196) */
FCU_DEV FCU_INLINE void level_state_first(LevelState &s, int ch, int scanPos) { s.ctxSet = (uint32_t)((ch ? 4 : 0) + ((!ch && (scanPos >> 4) > 0) ? 2 : 0)); }
/* after a coefficient whose level was chosen (:2272-2294) */
FCU_DEV FCU_INLINE void level_state_advance(LevelState &s, uint32_t level)
{
  const uint32_t baseLevel = (s.c1Idx < 8) ? (2 + (s.c2Idx < 1)) : 1;
  if (level >= baseLevel) { if (level > 3u * (1u << s.goRice)) s.goRice = s.goRice + 1 < 4 ? s.goRice + 1 : 4; }
  if (level >= 1) s.c1Idx++;
  if (level > 1) { s.c1 = 0; s.c2 += (s.c2 < 2); s.c2Idx++; }
  else if (s.c1 < 3 && s.c1 > 0 && level) s.c1++;
}
/* at the end of group cgScanPos > 0, once the last position is known: the context set of the next group (:2306-2316) */
FCU_DEV FCU_INLINE void level_state_next_group(LevelState &s, int ch, int cgScanPos)
{
  s.ctxSet = (uint32_t)((ch ? 4 : 0) + ((!ch && (cgScanPos - 1) > 0) ? 2 : 0) + (s.c1 == 0));
  s.c1 = 1; s.c2 = 0; s.c1Idx = 0; s.c2Idx = 0; s.goRice = 0;
}
/* The decision of a coefficient group at the end of its walk (:2318-2358): the cost of its coded_sub_block_flag goes into
 * baseCost, and a group whose levels cost more than leaving it empty is zeroed.  rdSigCost, rdSigCost0, rdCodedLevelandDist,
 * rdUncodedDist, nnzBeforePos0: the group's sums as the walk left them.  Returns costCGSig of the group and whether it was
 * zeroed; the caller then clears the group's levels and sets cc = c0, cs = 0 in the records of those that were not 0. */
struct CgDecision { double cgSig; int zeroed; };
template <class CB>
FCU_DEV FCU_INLINE CgDecision cg_decide(CB cb, const RdoqSetup &S, int cgScanPos, int cgLastScanPos, int cgBlk, int cgx, int cgy, uint64_t &cgflag, double &baseCost,
                                        double rdSigCost, double rdSigCost0, double rdCodedLevelandDist, double rdUncodedDist, int nnzBeforePos0)
{
  CgDecision d = { 0, 0 };
  if (cgLastScanPos >= 0) {
    if (cgScanPos) {
      if (((cgflag >> cgBlk) & 1) == 0) {
        const int ctxSig = S.cgBase + sig_cg_ctx(cgflag, cgx, cgy, S.wg);
        baseCost += S.lambda * (double)cb(ctxSig, 0) - rdSigCost;
        d.cgSig = S.lambda * (double)cb(ctxSig, 0);
      } else if (cgScanPos < cgLastScanPos) {
        if (nnzBeforePos0 == 0) { baseCost -= rdSigCost0; rdSigCost -= rdSigCost0; }
        double costZeroCG = baseCost;
        const int ctxSig = S.cgBase + sig_cg_ctx(cgflag, cgx, cgy, S.wg);
        baseCost += S.lambda * (double)cb(ctxSig, 1);
        costZeroCG += S.lambda * (double)cb(ctxSig, 0);
        d.cgSig = S.lambda * (double)cb(ctxSig, 1);
        costZeroCG += rdUncodedDist; costZeroCG -= rdCodedLevelandDist; costZeroCG -= rdSigCost;
        if (costZeroCG < baseCost) {
          cgflag &= ~(1ull << cgBlk); baseCost = costZeroCG;
          d.cgSig = S.lambda * (double)cb(ctxSig, 0);
          d.zeroed = 1;
        }
      }
    } else cgflag |= 1ull << cgBlk;
  }
  return d;
}
/* lambda * xGetRateLast (TComTrQuant.cpp:2898-2916) of scan position scanPos, with estLastSignificantPositionBit
 * (TEncSbac.cpp:1863-1923) evaluated on demand; LastCtx: what that estimate needs of the block, formed once per call */
struct LastCtx { int lsh, lbx, lby, lgmax; };
FCU_DEV FCU_INLINE LastCtx last_ctx_of(const RdoqSetup &S, int log2)
{
  const int lcc = log2 - 2, loff = S.ch ? 0 : (lcc * 3 + ((lcc + 1) >> 2));
  LastCtx L; L.lsh = S.ch ? lcc : ((lcc + 3) >> 2);
  L.lbx = CTX_LASTX + (S.ch ? 15 : 0) + loff; L.lby = CTX_LASTY + (S.ch ? 15 : 0) + loff; L.lgmax = g_hot.group_idx[S.N - 1];
  return L;
}
template <class CB>
FCU_DEV FCU_INLINE double rate_last(CB cb, const RdoqSetup &S, const LastCtx &L, int log2, int scanType, int scanPos)
{
  const int blk = S.scan[scanPos];
  const int py = blk >> log2, px = blk - (py << log2);
  const int ax = scanType == 2 ? py : px, ay = scanType == 2 ? px : py;
  const int gx = g_hot.group_idx[ax], gy = g_hot.group_idx[ay];
  int bxs = 0, bys = 0;
  for (int k = 0; k < gx; k++) bxs += cb(L.lbx + (k >> L.lsh), 1);
  if (gx < L.lgmax) bxs += cb(L.lbx + (gx >> L.lsh), 0);
  for (int k = 0; k < gy; k++) bys += cb(L.lby + (k >> L.lsh), 1);
  if (gy < L.lgmax) bys += cb(L.lby + (gy >> L.lsh), 0);
  double r = (double)(bxs + bys);
  if (gx > 3) r += 32768.0 * (double)((gx - 2) >> 1);
  if (gy > 3) r += 32768.0 * (double)((gy - 2) >> 1);
  return S.lambda * r;
}
/* Sign bit hiding (TComTrQuant.cpp:2478-2544): the price of changing the level at position n of a group by one, and in *change
 * the direction that price is for.  lv and du, up, dn, sd: the level and its record; srcNeg: the source value is negative
 * (looked at only where lv is 0 and n < firstNZ); firstNZ, lastNZ: the group's first and last non-zero positions, signbit: the
 * sign of the level at firstNZ; lastCG == 1: the group holds the block's last level. */
FCU_DEV FCU_INLINE long long sh_cost(int lv, int32_t du, int32_t up, int32_t dn, int32_t sd, int srcNeg, int n, int firstNZ, int lastNZ, int lastCG, uint32_t signbit,
                                     long long rdFactor, int *change)
{
  const long long kInf = 0x7fffffffffffffffLL;
  long long curCost;
  if (lv != 0) {
    const long long costUp = rdFactor * (-du) + up;
    long long costDown = rdFactor * (du) + dn - ((iabs(lv) == 1) ? sd : 0);
    if (lastCG == 1 && lastNZ == n && iabs(lv) == 1) costDown -= (4 << 15);
    if (costUp < costDown) { curCost = costUp; *change = 1; }
    else { *change = -1; if (n == firstNZ && iabs(lv) == 1) curCost = kInf; else curCost = costDown; }
  } else {
    curCost = rdFactor * (-(long long)(iabs(du))) + (1 << 15) + up + sd;
    *change = 1;
    if (n < firstNZ) { const uint32_t thissign = srcNeg ? 1 : 0; if (thissign != signbit) curCost = kInf; }
  }
  return curCost;
}
/* `c` is the coder whose contexts estBit() would snapshot (TEncSbac.cpp:1722-1956); cbfCtx
 * is the QT-CBF context of this TU (getCtxQtCbf + getCBFContextOffset).
 * src[sp*st] = level_double() of the coefficient at scan position sp; dst[sp*st] receives its level.
 * topNZ = highest scan position whose uiMaxAbsLevel is > 0 (found by the producer phase; -1: none).
 * Levels are written for the scan positions of coefficient groups <= topNZ/16 only; everything above is
 * zero by construction and the consumers know topNZ.  Returns uiAbsSum and the scan position of the last
 * non-zero level (-1: none). */
struct RdoqOut { int abs_sum, last; };
/* EST = 1: the caller has built g_S.est for coder `c` (est_build); EST = 0: costs are looked up in the coder itself */
/* The quantiser without RDOQ: xQuant's plain branch (TComTrQuant.cpp:1160-1240) + signBitHidingHDQ (:991-1124) in the
 * engine's scan-order domain.  src = sign * |coefficient| * quantiser scale per scan position (stride st), dst = levels;
 * positions above the coefficient group of topNZ can only quantise to 0 and are not touched (callers treat them as 0).
 * abs_sum is the sum before sign hiding, as the reference returns it; last = highest non-zero scan position afterwards. */
FCU_DEV FCU_NOINLINE RdoqOut quant_plain(const int32_t *src, int16_t *dst, int st, int topNZ, int log2, int comp, const Params &P)
{
  RdoqOut o = { 0, -1 };
  if (topNZ < 0) return o;
  const FCU_HBM int32_t *srcg = (const FCU_HBM int32_t *)src; FCU_HBM int16_t *dstg = (FCU_HBM int16_t *)dst;
  const int qp = comp ? P.qp_c : P.qp, qbits = rdoq_qbits(log2, qp), qbits8 = qbits - 8;
  const long long add = (long long)(P.slice_type == SLICE_I ? 171 : 85) << (qbits - 9);
  const int cgTop = topNZ >> 4;
  int absSum = 0;
  for (int sp = cgTop * 16 + 15; sp >= 0; sp--) {
    const int32_t ld = srcg[sp * st];
    const int q = (int)(((long long)iabs(ld) + add) >> qbits);
    absSum += q;
    dstg[sp * st] = (int16_t)clip3i(-32768, 32767, ld < 0 ? -q : q);
  }
  o.abs_sum = absSum;
  if (P.sign_hiding && absSum >= 2) {
    int lastCG = -1;
    for (int cg = cgTop; cg >= 0; cg--) {
      const int sub = cg << 4;
      int lv[16], du[16];
      int first = 16, last = -1, sum = 0;
      for (int n = 0; n < 16; n++) {
        const int32_t ld = srcg[(sub + n) * st]; lv[n] = dstg[(sub + n) * st];
        du[n] = (int)(((long long)iabs(ld) - ((long long)iabs(lv[n]) << qbits)) >> qbits8);
        if (lv[n]) { if (first == 16) first = n; last = n; }
      }
      for (int n = first; n <= last; n++) sum += lv[n];
      if (last >= 0 && lastCG == -1) lastCG = 1;
      if (last - first >= 4) {
        const unsigned signbit = lv[first] > 0 ? 0 : 1;
        if (signbit != (unsigned)(sum & 1)) {
          int curCost = 0x7fffffff, minCostInc = 0x7fffffff, minPos = -1, finalChange = 0, curChange = 0;
          for (int n = (lastCG == 1 ? last : 15); n >= 0; --n) {
            if (lv[n] != 0) {
              if (du[n] > 0) { curCost = -du[n]; curChange = 1; }
              else if (n == first && iabs(lv[n]) == 1) curCost = 0x7fffffff;
              else { curCost = du[n]; curChange = -1; }
            } else if (n < first) {
              const unsigned thisSign = srcg[(sub + n) * st] >= 0 ? 0 : 1;
              if (thisSign != signbit) curCost = 0x7fffffff; else { curCost = -du[n]; curChange = 1; }
            } else { curCost = -du[n]; curChange = 1; }
            if (curCost < minCostInc) { minCostInc = curCost; finalChange = curChange; minPos = n; }
          }
          if (lv[minPos] == 32767 || lv[minPos] == -32768) finalChange = -1;
          const int nv = srcg[(sub + minPos) * st] >= 0 ? lv[minPos] + finalChange : lv[minPos] - finalChange;
          dstg[(sub + minPos) * st] = (int16_t)nv;
        }
      }
      if (lastCG == 1) lastCG = 0;
    }
  }
  for (int sp = cgTop * 16 + 15; sp >= 0; sp--) if (dstg[sp * st]) { o.last = sp; break; }
  return o;
}

/* The passes of xRateDistOptQuant after its first loop, shared by rdoq() and rdoq_wave(): the last significant position
 * (:2360-2436), the signs, sign bit hiding (:2442-2572). */
template <class CB>
FCU_DEV FCU_INLINE int rdoq_last_pos(CB cb, const RdoqSetup &S, const FCU_HBM int16_t *dstg, const FCU_HBM RdoqRec *recg, const FCU_HBM double *cgg,
                                     int st, int log2, int scanType, int cbfCtx,
                                     uint64_t cgflag, int cgLastScanPos, int lastScanPos, double baseCost, double blockUncodedCost)
{
  const double lambda = S.lambda;
  double bestCost; int bestLastIdxP1 = 0;
  bestCost = blockUncodedCost + lambda * (double)cb(cbfCtx, 0);
  baseCost += lambda * (double)cb(cbfCtx, 1);
  const LastCtx L = last_ctx_of(S, log2);
  int foundLast = 0;
  for (int cgScanPos = cgLastScanPos; cgScanPos >= 0; cgScanPos--) {
    const int cgBlk = S.scanCG[cgScanPos];
    baseCost -= cgg[cgScanPos * st];
    if ((cgflag >> cgBlk) & 1) {
      const int top = (cgScanPos * 16 + 15 > lastScanPos) ? lastScanPos - cgScanPos * 16 : 15;   /* positions above the last one are skipped */
      int aLv = dstg[(cgScanPos * 16 + top) * st]; double aCs = recg[(cgScanPos * 16 + top) * st].cs;    /* one ahead */
      for (int posInCG = top; posInCG >= 0; posInCG--) {
        const int scanPos = cgScanPos * 16 + posInCG;
        const int lv = aLv; const double curCs = aCs;
        if (posInCG > 0) { aLv = dstg[(scanPos - 1) * st]; aCs = recg[(scanPos - 1) * st].cs; }
        if (lv) {
          const double costLast = rate_last(cb, S, L, log2, scanType, scanPos);
          const double totalCost = baseCost + costLast - curCs;
          if (totalCost < bestCost) { bestLastIdxP1 = scanPos + 1; bestCost = totalCost; }
          if (lv > 1) { foundLast = 1; break; }
          baseCost -= recg[scanPos * st].cc; baseCost += recg[scanPos * st].c0;
        } else baseCost -= curCs;
      }
      if (foundLast) break;
    }
  }
  return bestLastIdxP1;
}
/* signs back on the kept levels, zeros above the chosen last position; returns uiAbsSum */
FCU_DEV FCU_INLINE int rdoq_signs(const FCU_HBM int32_t *srcg, FCU_HBM int16_t *dstg, int st, int bestLastIdxP1, int lastScanPos)
{
  int absSum = 0;
  for (int sp0 = 0; sp0 < bestLastIdxP1; sp0 += 16) {           /* signs back on the kept levels, sixteen positions per round of loads */
    int lv[16]; int32_t sv[16];
#pragma unroll
    for (int k = 0; k < 16; k++) { const int ok = sp0 + k < bestLastIdxP1; lv[k] = ok ? dstg[(sp0 + k) * st] : 0; sv[k] = ok ? srcg[(sp0 + k) * st] : 0; }
#pragma unroll
    for (int k = 0; k < 16; k++) if (sp0 + k < bestLastIdxP1) { absSum += lv[k]; dstg[(sp0 + k) * st] = (int16_t)((sv[k] < 0) ? -lv[k] : lv[k]); }
  }
  for (int sp = bestLastIdxP1; sp <= lastScanPos; sp++) dstg[sp * st] = 0;

  return absSum;
}
FCU_DEV FCU_INLINE void rdoq_sign_hiding(const Params &P, const FCU_HBM int32_t *srcg, FCU_HBM int16_t *dstg, const FCU_HBM RdoqRec *recg, int st, int ch, int bestLastIdxP1, int absSum)
{
  if (P.sign_hiding && absSum >= 2) {                        /* TComTrQuant.cpp:2442-2572 */
    const long long rdFactor = P.rd_factor[ch];
    int lastCG = -1;
    for (int subSet = (bestLastIdxP1 - 1) >> 4; subSet >= 0; subSet--) {   /* groups above hold no level any more */
      const int subPos = subSet << 4; int firstNZ = 16, lastNZ = -1, sum = 0, n;
      uint32_t nzMask = 0, negMask = 0;                          /* the group's sixteen levels in one go */
      {
        int lv16[16];
#pragma unroll
        for (int k = 0; k < 16; k++) lv16[k] = dstg[(subPos + k) * st];
#pragma unroll
        for (int k = 0; k < 16; k++) { sum += lv16[k]; nzMask |= (uint32_t)(lv16[k] != 0) << k; negMask |= (uint32_t)(lv16[k] < 0) << k; }
      }
      if (nzMask) { lastNZ = 31 - __builtin_clz(nzMask); firstNZ = __builtin_ctz(nzMask); }
      if (lastNZ >= 0 && lastCG == -1) lastCG = 1;
      if (lastNZ - firstNZ >= 4) {
        const uint32_t signbit = (negMask >> firstNZ) & 1;
        if (signbit != (uint32_t)(sum & 1)) {
          long long minCostInc = 0x7fffffffffffffffLL;
          int minPos = -1, finalChange = 0, curChange = 0;
          for (n = (lastCG == 1 ? lastNZ : 15); n >= 0; --n) {
            const int sp = n + subPos; const int lv = dstg[sp * st]; const RdoqRec q = recg[sp * st];
            const int srcNeg = (lv == 0 && n < firstNZ) ? srcg[sp * st] < 0 : 0;   /* loaded only where sh_cost() looks at it */
            const long long curCost = sh_cost(lv, q.du, q.up, q.dn, q.sd, srcNeg, n, firstNZ, lastNZ, lastCG, signbit, rdFactor, &curChange);
            if (curCost < minCostInc) { minCostInc = curCost; finalChange = curChange; minPos = sp; }
          }
          const int old = dstg[minPos * st];
          if (old == 32767 || old == -32768) finalChange = -1;
          const int nv = srcg[minPos * st] >= 0 ? old + finalChange : old - finalChange;
          dstg[minPos * st] = (int16_t)nv;
        }
      }
      if (lastCG == 1) lastCG = 0;
    }
  }
}
/* the tail of rdoq(), and the reference -DFCU_EMU_CHECK_RDOQ_TAIL runs next to the passes of rdoq_wave() */
template <class CB>
FCU_DEV FCU_INLINE RdoqOut rdoq_finish(CB cb, const Params &P, const RdoqSetup &S, const FCU_HBM int32_t *srcg, FCU_HBM int16_t *dstg, FCU_HBM RdoqRec *recg, FCU_HBM double *cgg,
                                       int st, int log2, int scanType, int cbfCtx,
                                       uint64_t cgflag, int cgLastScanPos, int lastScanPos, double baseCost, double blockUncodedCost)
{
  FCU_RTIC(rt_);
  const int bestLastIdxP1 = rdoq_last_pos(cb, S, dstg, recg, cgg, st, log2, scanType, cbfCtx, cgflag, cgLastScanPos, lastScanPos, baseCost, blockUncodedCost);
  FCU_RTOC(P, rt_, 13);                                       /* last-position search */
  const int absSum = rdoq_signs(srcg, dstg, st, bestLastIdxP1, lastScanPos);
  FCU_RTOC(P, rt_, 14);                                       /* signs */
  rdoq_sign_hiding(P, srcg, dstg, recg, st, S.ch, bestLastIdxP1, absSum);
  FCU_RTOC(P, rt_, 15);                                       /* sign hiding */
  int last = bestLastIdxP1 - 1;                              /* sign hiding may have cleared the last level */
  while (last >= 0 && dstg[last * st] == 0) last--;
  RdoqOut o = { absSum, last };
  return o;
}


template <int EST>
/* called inside a lane loop, a candidate per lane.  slot: the caller's lane, < MAXVC: the column of g_S.rq_grp this walk stages
 * its coefficient group in */
FCU_DEV FCU_NOINLINE RdoqOut rdoq(int c, const int32_t *src, int16_t *dst, int st, int topNZ, int log2, int comp, int scanType, int cbfCtx, const Params &P_, RdoqRec *rec, double *costCGSig, int slot = 0)
{
  const Params &P = *FCU_UNI(&P_);
  st = FCU_UNI(st); log2 = FCU_UNI(log2); comp = FCU_UNI(comp); cbfCtx = FCU_UNI(cbfCtx);
  FCU_RTIC(rt_);
  if (topNZ < 0) { FCU_WALK_COUNT(WALK_RDOQ_ALL_ZERO, 1); RdoqOut z = { 0, -1 }; return z; }            /* every level is 0: the reference leaves with uiAbsSum 0 (:2330) */
  const FCU_HBM int32_t *srcg = (const FCU_HBM int32_t *)src; FCU_HBM int16_t *dstg = (FCU_HBM int16_t *)dst;
  FCU_HBM RdoqRec *recg = (FCU_HBM RdoqRec *)rec; FCU_HBM double *cgg = (FCU_HBM double *)costCGSig;
  auto cb = [&](int ctx, int bin) -> int { return EST ? (int)FCU_EST[ctx * 2 + bin] : ctx_bits(c, ctx, bin); };
  /* the reference clears all seven arrays; only entries at scan positions <= the last significant one are
   * ever read back (last-position search, group zero-out, sign hiding), and each of those is written below */
  const RdoqSetup S = rdoq_setup(P, log2, comp, scanType);
  const int ch = S.ch, n2 = S.n2, qbits = S.qbits, wg = S.wg, sigOff = S.sigOff; const double lambda = S.lambda, errScale = S.errScale;
  uint64_t cgflag = 0;
  int cgLastScanPos = -1; LevelState ls;
  double baseCost = 0, blockUncodedCost = 0;
  int lastScanPos = -1;

  int g10 = 0, g10Ctx = -1;
  /* coefficient groups above the last candidate level: only the uncoded cost accumulates (in scan order) */
  const int cgTop = topNZ >> 4;
  for (int cg = (n2 >> 4) - 1; cg > cgTop; cg--) {            /* a group's sixteen loads first, then the adds in scan order */
    int32_t v[16];
#pragma unroll
    for (int k = 0; k < 16; k++) v[k] = srcg[(cg * 16 + k) * st];
#pragma unroll
    for (int k = 15; k >= 0; k--) { const double err = (double)iabs(v[k]); blockUncodedCost += err * err * errScale; }
  }
  baseCost = blockUncodedCost;
  FCU_RTOC(P, rt_, 11);                                       /* set-up + uncoded tail */
  /* A group is fetched as a group: sixteen loads issued together, one round trip per group where a load one coefficient
   * ahead pays a partly exposed round trip on every short iteration.  The loads of group cg - 1 are written at the
   * top of the walk of group cg, but that is NOT an overlap with the walk in the compiled kernel: the flat load of
   * scanCG[cgScanPos] follows them, loads retire in order, and its s_waitcnt vmcnt(0) waits for all sixteen.  (Reading scanCG
   * one group ahead through typed pointers does remove that wait, but a table read still stalls at the group top for TUs above
   * 8x8 and the private segment grows by 250 B: not shipped)  The values are parked in the lane's column of
   * g_S.rq_grp, which the coefficient loop indexes (a register array indexed by the position would live in scratch memory). */
  int32_t nxt[16];
  FCU_CHECK(slot >= 0 && slot < MAXVC);
#pragma unroll
  for (int k = 0; k < 16; k++) { FCU_CHECK_LSCAN(&srcg[(cgTop * 16 + k) * st]); nxt[k] = srcg[(cgTop * 16 + k) * st]; }
  FCU_WALK_COUNT(WALK_RDOQ_CALLS, 1); FCU_WALK_COUNT(WALK_RDOQ_TOP_IS_GROUP0, cgTop == 0);
  FCU_LV_BEGIN(lv_);
  for (int cgScanPos = cgTop; cgScanPos >= 0; cgScanPos--) {
#pragma unroll
    for (int k = 0; k < 16; k++) g_S.rq_grp[k][slot] = nxt[k];
    if (cgScanPos > 0) {                                      /* group 0 has no successor: no address below scan position 0 is formed */
      FCU_WALK_COUNT(WALK_RDOQ_AHEAD_GROUPS, 1);
#pragma unroll
      for (int k = 0; k < 16; k++) { FCU_CHECK_LSCAN(&srcg[((cgScanPos - 1) * 16 + k) * st]); nxt[k] = srcg[((cgScanPos - 1) * 16 + k) * st]; }
    }
    const int cgBlk = S.scanCG[cgScanPos], cgy = cgBlk / wg, cgx = cgBlk - cgy * wg;
    double rdSigCost = 0, rdSigCost0 = 0, rdCodedLevelandDist = 0, rdUncodedDist = 0; int nnzBeforePos0 = 0;
    const int pattern = pattern_sig_ctx(cgflag, cgx, cgy, wg);
    /* The contexts are frozen during RDOQ (estBit snapshot, TEncSbac.cpp:1722-1956), so the significance costs of a
     * group are loop invariants: in a TU > 4x4 only the three contexts sigBase + cnt occur besides DC (sig_ctx_of). */
    const int sigBase = sig_base_of(S, cgx, cgy);
    int b00 = 0, b01 = 0, b02 = 0, b10 = 0, b11 = 0, b12 = 0;
    if (log2 > 2) {
      b00 = cb(sigBase, 0); b01 = cb(sigBase + 1, 0); b02 = cb(sigBase + 2, 0);
      b10 = cb(sigBase, 1); b11 = cb(sigBase + 1, 1); b12 = cb(sigBase + 2, 1);
    }
    const uint32_t cntBits = g_hot.cnt_bits[pattern];
    for (int posInCG = 15; posInCG >= 0; posInCG--) {
      const int scanPos = cgScanPos * 16 + posInCG;
      FCU_LV_TOP(lv_, 1);
      const int32_t levelDouble = iabs(g_S.rq_grp[posInCG][slot]);
      uint32_t maxAbsLevel = (uint32_t)((levelDouble + ((int32_t)1 << (qbits - 1))) >> qbits);
      if (maxAbsLevel > 32767u) maxAbsLevel = 32767u;
      FCU_LV_LONG(lv_, maxAbsLevel > 0);
      const double err = (double)levelDouble;
      double c0 = err * err * errScale, cc = 0, cs = 0;
      blockUncodedCost += c0;
      uint32_t level = maxAbsLevel;
      if (maxAbsLevel > 0 && lastScanPos < 0) {
        lastScanPos = scanPos;
        level_state_first(ls, ch, scanPos);
        cgLastScanPos = cgScanPos;
      }
      if (lastScanPos >= 0) {
        const int oneCtx = CTX_ONE + 4 * (int)ls.ctxSet + ls.c1;
        if (oneCtx != g10Ctx) { g10 = cb(oneCtx, 0); g10Ctx = oneCtx; }
        const int ctxSig = sig_ctx_of(S, log2, scanPos, posInCG, sigBase, cntBits);
        int sbit0, sbit1;
        if (log2 == 2 || scanPos == 0) { sbit0 = cb(ctxSig, 0); sbit1 = cb(ctxSig, 1); }
        else { const int cnt = ctxSig - sigBase; sbit0 = cnt == 0 ? b00 : (cnt == 1 ? b01 : b02); sbit1 = cnt == 0 ? b10 : (cnt == 1 ? b11 : b12); }   /* one of the group's three: costs in registers */
        int sdel = 0, rup, rdn = 0;
        if (maxAbsLevel == 0) {                              /* xGetCodedLevel's early exit (:2752-2760); never the last position */
          /* short path: level 0 leaves c1/c2/Rice state alone; everything the long path does for it, and on to the next */
          cs = lambda * (double)sbit0; cc = c0 + cs;
          RdoqRec r; r.cc = cc; r.cs = cs; r.c0 = c0; r.up = g10; r.dn = 0; r.sd = sbit1 - sbit0;
          r.du = (int32_t)(levelDouble >> (qbits - 8));
          recg[scanPos * st] = r;
          baseCost += cc;
          dstg[scanPos * st] = 0;
          rdSigCost += cs;
          if (posInCG == 0) rdSigCost0 = cs;
          continue;
        } else {
          const int absCtx = CTX_ABS + (int)ls.ctxSet + ls.c2;
          LevelBits lb; lb.g10 = g10; lb.g11 = cb(oneCtx, 1); lb.g20 = cb(absCtx, 0); lb.g21 = cb(absCtx, 1);
          const int isLast = scanPos == lastScanPos;
          FCU_LV_OWN(lv_);
#ifdef FCU_RDOQ_LEVELS_REF
          const LevelChoice lc = level_choice_ref(cb, lambda, &cc, &c0, &cs, levelDouble, maxAbsLevel, isLast ? sigOff : ctxSig, lb, ls.goRice, ls.c1Idx, ls.c2Idx, qbits, errScale, isLast);
#else
          const LevelChoice lc = level_choice(lambda, &cc, &c0, &cs, levelDouble, maxAbsLevel, sbit0, sbit1, lb, ls.goRice, ls.c1Idx, ls.c2Idx, qbits, errScale, isLast);
          FCU_CHECK_LEVELS(cb, isLast ? sigOff : ctxSig, lc, cc, c0, cs, lambda, levelDouble, maxAbsLevel, lb, ls.goRice, ls.c1Idx, ls.c2Idx, qbits, errScale, isLast);
#endif
          FCU_LV_SEC(lv_, s0);
          level = lc.level; rup = lc.rup; rdn = lc.rdn;
          if (!isLast) sdel = sbit1 - sbit0;
        }
        RdoqRec r; r.cc = cc; r.cs = cs; r.c0 = c0; r.up = rup; r.dn = rdn; r.sd = sdel;
        r.du = (int32_t)((levelDouble - ((int32_t)level << qbits)) >> (qbits - 8));
        recg[scanPos * st] = r;
        baseCost += cc;
        level_state_advance(ls, level);
        FCU_LV_SEC(lv_, s2);
      } else baseCost += c0;
      dstg[scanPos * st] = (int16_t)level;
      rdSigCost += cs;
      if (posInCG == 0) rdSigCost0 = cs;
      if (level) {
        cgflag |= 1ull << cgBlk;
        rdCodedLevelandDist += cc - cs;
        rdUncodedDist += c0;
        if (posInCG != 0) nnzBeforePos0++;
      }
    }
    FCU_LV_TOP(lv_, 0);
    if (lastScanPos >= 0 && cgScanPos > 0) level_state_next_group(ls, ch, cgScanPos);
    const CgDecision cgd = cg_decide(cb, S, cgScanPos, cgLastScanPos, cgBlk, cgx, cgy, cgflag, baseCost, rdSigCost, rdSigCost0, rdCodedLevelandDist, rdUncodedDist, nnzBeforePos0);
    cgg[cgScanPos * st] = cgd.cgSig;
    if (cgd.zeroed) {
      for (int posInCG = 15; posInCG >= 0; posInCG--) {
        const int scanPos = cgScanPos * 16 + posInCG;
        if (dstg[scanPos * st]) { dstg[scanPos * st] = 0; recg[scanPos * st].cc = recg[scanPos * st].c0; recg[scanPos * st].cs = 0; }
      }
    }
  }
  FCU_RTOC(P, rt_, 12);                                       /* main loop */
  FCU_LV_TOP(lv_, 0); FCU_LV_END(P, lv_);
  if (lastScanPos < 0) { RdoqOut z = { 0, -1 }; return z; }
#ifdef FCU_EMU
  FCU_WALK_COUNT(WALK_RDOQ_ONLY_GROUP0, lastScanPos < 16);
  if (n2 > 16 && lastScanPos >= n2 - 16) {                    /* test bookkeeping: every level below the last group is 0 */
    int other = 0;
    for (int sp = 0; sp < n2 - 16; sp++) other |= dstg[sp * st];
    FCU_WALK_COUNT(WALK_RDOQ_ONLY_LAST_GROUP, !other);
  }
#endif
  return rdoq_finish(cb, P, S, srcg, dstg, recg, cgg, st, log2, scanType, cbfCtx, cgflag, cgLastScanPos, lastScanPos, baseCost, blockUncodedCost);
}

/* A value every lane holds one element of, readable and writable by element from wave-uniform code: a register plus
 * v_readlane / v_writelane on the GPU, an array on the CPU emulator (whose lanes run one after the other).  from(src), inside a
 * lane loop, reads the element of another lane, a source index per lane (ds_bpermute on the GPU): the element must have been
 * set in an earlier lane loop, and on the GPU all 64 lanes must be active at the read. */
#ifdef FCU_EMU
template <class T> struct LaneVar {
  T v[64];
  LaneVar() { for (int i = 0; i < 64; i++) v[i] = T(); }
  void set(int lane, T x) { v[lane] = x; }                   /* inside a lane loop: this lane's element */
  T own(int lane) const { return v[lane]; }
  T get(int k) const { return v[k]; }                        /* wave-uniform code: element k */
  void put(int k, T x) { v[k] = x; }
  T from(int src) const { return v[src & 63]; }              /* inside a lane loop: the element of lane `src`, set in an EARLIER lane loop (a source index per lane) */
};
/* wave-uniform summaries of a lane value: which of the sixteen lanes lb .. lb + 15 hold a non-zero / an odd element, and the
 * sum of all 64 (modulo 2^32).  On the GPU all 64 lanes must be active at the call. */
FCU_DEV uint32_t lane_nz16(const LaneVar<int> &f, int lb) { uint32_t m = 0; for (int k = 0; k < 16; k++) m |= (uint32_t)(f.v[lb + k] != 0) << k; return m; }
FCU_DEV uint32_t lane_odd16(const LaneVar<int> &f, int lb) { uint32_t m = 0; for (int k = 0; k < 16; k++) m |= (uint32_t)(f.v[lb + k] & 1) << k; return m; }
FCU_DEV int lane_sum(const LaneVar<int> &f) { uint32_t s = 0; for (int k = 0; k < 64; k++) s += (uint32_t)f.v[k]; return (int)s; }
#else
#if defined(__HIP_DEVICE_COMPILE__)
#define FCU_READLANE(v, k) __builtin_amdgcn_readlane((v), (k))
#define FCU_WRITELANE(val_, k_, old_) (((int)threadIdx.x == (k_)) ? (val_) : (old_))     /* (this compiler has no v_writelane builtin: compare + select) */
#define FCU_BALLOT(p) __builtin_amdgcn_ballot_w64(p)
#define FCU_PERMUTE(v, src) __builtin_amdgcn_ds_bpermute((src) << 2, (v))     /* all 64 lanes active: an inactive source lane reads as 0 */
#else                                                         /* host pass over the device code: parsed, never run */
#define FCU_READLANE(v, k) (v)
#define FCU_WRITELANE(val_, k_, old_) (val_)
#define FCU_BALLOT(p) ((unsigned long long)(p))
#define FCU_PERMUTE(v, src) (v)
#endif
template <class T> struct LaneVar;
template <> struct LaneVar<int> {
  int r = 0;
  __device__ void set(int, int x) { r = x; }
  __device__ int own(int) const { return r; }
  __device__ int get(int k) const { return FCU_READLANE(r, k); }
  __device__ void put(int k, int x) { r = FCU_WRITELANE(x, k, r); }
  __device__ int from(int src) const { return FCU_PERMUTE(r, src); }
};
template <> struct LaneVar<double> {
  double r = 0;
  __device__ void set(int, double x) { r = x; }
  __device__ double own(int) const { return r; }
  __device__ double get(int k) const
  { union { double d; int i[2]; } u; u.d = r; u.i[0] = FCU_READLANE(u.i[0], k); u.i[1] = FCU_READLANE(u.i[1], k); return u.d; }
  __device__ void put(int k, double x)
  { union { double d; int i[2]; } u, w; u.d = r; w.d = x; u.i[0] = FCU_WRITELANE(w.i[0], k, u.i[0]); u.i[1] = FCU_WRITELANE(w.i[1], k, u.i[1]); r = u.d; }
};
__device__ inline uint32_t lane_nz16(const LaneVar<int> &f, int lb) { return (uint32_t)(FCU_BALLOT(f.r != 0) >> lb) & 0xffffu; }
__device__ inline uint32_t lane_odd16(const LaneVar<int> &f, int lb) { return (uint32_t)(FCU_BALLOT((f.r & 1) != 0) >> lb) & 0xffffu; }
__device__ inline int lane_sum(const LaneVar<int> &f) { return (int)fcu_wave_sum((uint32_t)f.r); }
#endif

/* The same quantiser for ONE block with the whole wave (called from wave-uniform code, not from inside a lane loop): the
 * un-split trial of a transform unit has a single candidate, and then a lane-private rdoq() leaves 63 lanes idle while one
 * lane walks every coefficient.  What is serial in xRateDistOptQuant's first loop is the order of the floating-point sums and
 * the greater1 / greater2 / Rice state, which only a non-zero level moves; everything else about a coefficient -- |level_double|,
 * uiMaxAbsLevel, its uncoded cost, its significance context and rates, and for a coefficient that can only quantise to 0 the
 * whole record -- depends on its position and on the group flags of the groups already walked.  So per coefficient group:
 *   sixteen lanes one coefficient each, results kept in the lane's registers (LaneVar);
 *   the wave      the walk in scan order as wave-uniform code: a coefficient's prepared numbers come over v_readlane (no memory
 *                 access), three additions for one whose uiMaxAbsLevel is 0, the level choice (coded_level) for the others,
 *                 results back into the owning lane (v_writelane); then the group decisions.
 * A 4x4 or 8x8 block (log2 <= 3, at most 64 coefficients) gives group g the lanes 16 g .. 16 g + 15, so after the walk lane sp
 * holds level, record, source value of scan position sp, and every pass after the walk runs on those registers: each lane
 * prices its own position as the last one, applies its sign, prices its own sign-hiding change; the block's levels are stored
 * once, at the end, and its records never.  A larger block walks every group on lanes 0..15 and stores its records and
 * levels to the pools per group; its passes fetch a group per round trip (sixteen lanes, a position each) and run the same
 * lane code.  Every floating-point expression and every comparison is the one rdoq() and rdoq_finish() evaluate, in the same
 * order (the running sums stay wave-uniform walks in scan order); sign hiding is the argmin of rdoq_sign_hiding() with its order
 * of preference (the highest position among equal costs).  st = 1, EST = 1 (the caller has built g_S.est for coder c).
 * Emulator: a LaneVar is an array and a lane loop runs its lanes one after the other, so a lane reads elements of OTHER lanes
 * only in wave-uniform code (get) or through from(), never through own() of a value another lane sets in the same loop.
 * -DFCU_EMU_CHECK_RDOQ_TAIL (emulator only): every call also stores what the pool form stores, runs rdoq_finish() on a copy
 * and aborts unless levels, uiAbsSum and last position agree.
 * Result: g_S.rw_abs / g_S.rw_lsp, levels of scan positions < 16 (topNZ / 16 + 1) in dst. */
FCU_DEV FCU_NOINLINE void rdoq_wave(int c, const int32_t *src, int16_t *dst, int topNZ, int log2, int comp, int scanType, int cbfCtx, const Params &P_, RdoqRec *rec, double *costCGSig)
{
  const Params &P = *FCU_UNI(&P_);
  c = FCU_UNI(c); src = FCU_UNI(src); dst = FCU_UNI(dst); topNZ = FCU_UNI(topNZ); log2 = FCU_UNI(log2); comp = FCU_UNI(comp);
  scanType = FCU_UNI(scanType); cbfCtx = FCU_UNI(cbfCtx); rec = FCU_UNI(rec); costCGSig = FCU_UNI(costCGSig);
  if (topNZ < 0) { FCU_SERIAL { g_S.rw_abs = 0; g_S.rw_lsp = -1; } return; }   /* every level is 0: the reference leaves with uiAbsSum 0 (:2330) */
  const FCU_HBM int32_t *srcg = (const FCU_HBM int32_t *)src; FCU_HBM int16_t *dstg = (FCU_HBM int16_t *)dst;
  FCU_HBM RdoqRec *recg = (FCU_HBM RdoqRec *)rec; FCU_HBM double *cgg = (FCU_HBM double *)costCGSig;
  auto cb = [&](int ctx, int bin) -> int { return (int)FCU_EST[ctx * 2 + bin]; };
  const RdoqSetup S = rdoq_setup(P, log2, comp, scanType);
  const int ch = S.ch, n2 = S.n2, qbits = S.qbits, wg = S.wg; const double lambda = S.lambda, errScale = S.errScale;
  const int cgTop = topNZ >> 4;
  const int inRegs = log2 <= 3;                                /* the block's records stay in the lanes: scan position sp in lane sp */
  const int nStore = (cgTop + 1) << 4;                         /* the caller reads the levels of scan positions below this */
#ifdef FCU_EMU_CHECK_RDOQ_TAIL
  const int toPools = 1;
#else
  const int toPools = !inRegs;
#endif
  FCU_TAIL_COUNT(TAIL_CHROMA, ch); FCU_TAIL_COUNT(TAIL_TOP_IN_GROUP0_8X8, log2 == 3 && cgTop == 0);
  /* the walk's state: wave-uniform values (the same in every lane) */
  uint64_t cgflag = 0;
  int cgLastScanPos = -1; LevelState ls;
  double baseCost = 0, blockUncodedCost = 0;
  int lastScanPos = -1;
  int g10 = 0, g10Ctx = -1;
  FCU_WTIC(wt_);
  /* coefficient groups above the last candidate level: only the uncoded cost accumulates (in scan order); lanes 0..15 load and
   * square, the wave adds in order */
  for (int cg = (n2 >> 4) - 1; cg > cgTop; cg -= 4) {           /* four groups per round of loads: lanes 16 j .. 16 j + 15 take group cg - j */
    LaneVar<double> t0;
    FCU_FOR_LANES { const int g = cg - (lane >> 4); if (g > cgTop) { const double err = (double)iabs(srcg[g * 16 + (lane & 15)]); t0.set(lane, err * err * errScale); } }
    for (int j = 0; j < 4 && cg - j > cgTop; j++)
      for (int k = 15; k >= 0; k--) blockUncodedCost += t0.get(j * 16 + k);
  }
  baseCost = blockUncodedCost;
  /* memory latency off the walk: lane k holds the block position of group k for the whole call; the coefficients of a block in
   * registers are all fetched here (lane sp keeps the source value, whose sign the later passes need), those of a larger block
   * group by group, while the group before is walked */
  LaneVar<int> vCgBlk, vNext;
  LaneVar<double> vCgSig;                                      /* costCGSig of group k in lane k */
  FCU_FOR_LANES_REG {
    if (lane <= cgTop) vCgBlk.set(lane, S.scanCG[lane]);
    if (inRegs) { if (lane < nStore) vNext.set(lane, srcg[lane]); }
    else if (lane < 16) vNext.set(lane, srcg[cgTop * 16 + lane]);
  }
  FCU_WTOC(P, wt_, 0, log2);
  /* a coefficient's numbers, in the lane that owns it (declared here: in a block in registers they outlive the walk) */
  LaneVar<int> vLd, vMax, vSb0, vSb1, vUp, vDn, vSd, vDu, vLv, vCand;
  LaneVar<double> vC0, vCs, vCc;
  for (int cgScanPos = cgTop; cgScanPos >= 0; cgScanPos--) {
    const int lb = inRegs ? cgScanPos << 4 : 0;                /* the group's sixteen lanes: lb .. lb + 15 */
    const int cgBlk = vCgBlk.get(cgScanPos), cgy = cgBlk / wg, cgx = cgBlk - cgy * wg;
    const int sigBase = sig_base_of(S, cgx, cgy);
    const uint32_t cntBits = g_hot.cnt_bits[pattern_sig_ctx(cgflag, cgx, cgy, wg)];
    FCU_FOR_LANES_REG {
      if ((unsigned)(lane - lb) < 16u) {                       /* one coefficient of this group per lane */
        const int posInCG = lane - lb, scanPos = cgScanPos * 16 + posInCG;
        const int32_t levelDouble = iabs(vNext.own(lane));
        if (!inRegs && cgScanPos > 0) vNext.set(lane, srcg[scanPos - 16]);
        uint32_t maxAbsLevel = (uint32_t)((levelDouble + ((int32_t)1 << (qbits - 1))) >> qbits);
        if (maxAbsLevel > 32767u) maxAbsLevel = 32767u;
        const double err = (double)levelDouble;
        const double c0 = err * err * errScale;
        const int ctxSig = sig_ctx_of(S, log2, scanPos, posInCG, sigBase, cntBits);
        const int sbit0 = cb(ctxSig, 0), sbit1 = cb(ctxSig, 1);
        vLd.set(lane, levelDouble); vMax.set(lane, (int)maxAbsLevel); vSb0.set(lane, sbit0); vSb1.set(lane, sbit1);
        vC0.set(lane, c0); vCand.set(lane, maxAbsLevel != 0);
        /* xGetCodedLevel's early exit (:2752-2760) for uiMaxAbsLevel 0: the whole record but rateIncUp, which follows the greater1 state */
        const double cs = lambda * (double)sbit0;
        vCs.set(lane, cs); vCc.set(lane, c0 + cs); vSd.set(lane, sbit1 - sbit0); vDu.set(lane, (int32_t)(levelDouble >> (qbits - 8)));
        vUp.set(lane, 0); vDn.set(lane, 0); vLv.set(lane, 0);
      }
    }
    const uint32_t cand = lane_nz16(vCand, lb);
    double rdSigCost = 0, rdSigCost0 = 0, rdCodedLevelandDist = 0, rdUncodedDist = 0; int nnzBeforePos0 = 0;
    for (int posInCG = 15; posInCG >= 0; posInCG--) {
      const int scanPos = cgScanPos * 16 + posInCG, ln = lb + posInCG;
      const int isCand = (int)((cand >> posInCG) & 1);
      double c0 = vC0.get(ln), cc = 0, cs = 0;
      blockUncodedCost += c0;
      uint32_t level = 0;
      if (isCand && lastScanPos < 0) {
        lastScanPos = scanPos;
        level_state_first(ls, ch, scanPos);
        cgLastScanPos = cgScanPos;
      }
      if (lastScanPos >= 0) {
        const int oneCtx = CTX_ONE + 4 * (int)ls.ctxSet + ls.c1;
        if (oneCtx != g10Ctx) { g10 = cb(oneCtx, 0); g10Ctx = oneCtx; }
        if (!isCand) {                                         /* level 0 leaves c1/c2/Rice state alone */
          cs = vCs.get(ln); cc = vCc.get(ln);
          vUp.put(ln, g10);
          baseCost += cc;
          rdSigCost += cs;
          if (posInCG == 0) rdSigCost0 = cs;
          continue;
        }
        const int32_t levelDouble = vLd.get(ln); const uint32_t maxAbsLevel = (uint32_t)vMax.get(ln);
        const int sbit0 = vSb0.get(ln), sbit1 = vSb1.get(ln);
        auto cbs = [&](int, int bin) -> int { return bin ? sbit1 : sbit0; };   /* the significance rates of this coefficient, looked up by its lane */
        int sdel = 0, rup, rdn = 0;
        const int absCtx = CTX_ABS + (int)ls.ctxSet + ls.c2;
        LevelBits lb4; lb4.g10 = g10; lb4.g11 = cb(oneCtx, 1); lb4.g20 = cb(absCtx, 0); lb4.g21 = cb(absCtx, 1);
        const int isLast = scanPos == lastScanPos;
#ifdef FCU_RDOQ_LEVELS_REF
        const LevelChoice lc = level_choice_ref(cbs, lambda, &cc, &c0, &cs, levelDouble, maxAbsLevel, 0, lb4, ls.goRice, ls.c1Idx, ls.c2Idx, qbits, errScale, isLast);
#else
        const LevelChoice lc = level_choice(lambda, &cc, &c0, &cs, levelDouble, maxAbsLevel, sbit0, sbit1, lb4, ls.goRice, ls.c1Idx, ls.c2Idx, qbits, errScale, isLast);
        FCU_CHECK_LEVELS(cbs, 0, lc, cc, c0, cs, lambda, levelDouble, maxAbsLevel, lb4, ls.goRice, ls.c1Idx, ls.c2Idx, qbits, errScale, isLast);
#endif
        level = lc.level; rup = lc.rup; rdn = lc.rdn;
        if (!isLast) sdel = sbit1 - sbit0;
        vCc.put(ln, cc); vCs.put(ln, cs); vC0.put(ln, c0); vUp.put(ln, rup); vDn.put(ln, rdn); vSd.put(ln, sdel);
        vDu.put(ln, (int32_t)((levelDouble - ((int32_t)level << qbits)) >> (qbits - 8)));
        baseCost += cc;
        level_state_advance(ls, level);
      } else baseCost += c0;
      vLv.put(ln, (int)level);
      rdSigCost += cs;
      if (posInCG == 0) rdSigCost0 = cs;
      if (level) {
        cgflag |= 1ull << cgBlk;
        rdCodedLevelandDist += cc - cs;
        rdUncodedDist += c0;
        if (posInCG != 0) nnzBeforePos0++;
      }
    }
    if (lastScanPos >= 0 && cgScanPos > 0) level_state_next_group(ls, ch, cgScanPos);
    const CgDecision cgd = cg_decide(cb, S, cgScanPos, cgLastScanPos, cgBlk, cgx, cgy, cgflag, baseCost, rdSigCost, rdSigCost0, rdCodedLevelandDist, rdUncodedDist, nnzBeforePos0);
    const double cgSig = cgd.cgSig;                            /* costCGSig of this group */
    FCU_TAIL_COUNT(TAIL_CG_ZEROED_8X8, cgd.zeroed && log2 == 3);
    if (cgd.zeroed) FCU_FOR_LANES_REG { if ((unsigned)(lane - lb) < 16u) vLv.set(lane, 0); }   /* the group's levels go to 0, each in its lane */
    /* a larger block: records and levels of the group to the pools.  The passes that follow read the records of groups that
     * kept a level only (last position: flagged groups; sign hiding: the same): a group without one stores its sixteen zero
     * levels and nothing else.  A block in registers stores nothing here, and nothing outside this function reads its records
     * or costCGSig (tu_trial and the inter RQT read the levels alone) */
    if (toPools) {
      const int keepsLevel = (int)((cgflag >> cgBlk) & 1);
      FCU_FOR_LANES {
        if ((unsigned)(lane - lb) < 16u) {
          const int sp = cgScanPos * 16 + lane - lb;
          if (keepsLevel) {
            RdoqRec r; r.cc = vCc.own(lane); r.cs = vCs.own(lane); r.c0 = vC0.own(lane); r.up = vUp.own(lane); r.dn = vDn.own(lane); r.sd = vSd.own(lane); r.du = vDu.own(lane);
            recg[sp] = r;
          }
          dstg[sp] = (int16_t)vLv.own(lane);
        }
        if (lane == 0) cgg[cgScanPos] = cgSig;
      }
    }
    vCgSig.put(cgScanPos, cgSig);
  }
  FCU_WTOC(P, wt_, 1, log2);
  if (lastScanPos < 0) {
    FCU_FOR_LANES { if (inRegs && lane < nStore) dstg[lane] = 0; if (lane == 0) { g_S.rw_abs = 0; g_S.rw_lsp = -1; } }
    return;
  }
#ifdef FCU_EMU_CHECK_RDOQ_TAIL
  int16_t chkLv[1024]; const double chkBase = baseCost; int chkSkip = 0;
  for (int sp = 0; sp < nStore; sp++) chkLv[sp] = dstg[sp];
#endif
  /* rdoq_last_pos as a wave: every lane prices its position as the last one (xGetRateLast) -- a block in registers all at once
   * from the lane's own level, a larger block per group that kept a level, after sixteen lanes fetched level and record of a
   * position each; the walk over the positions -- the running cost without the coefficients above -- is wave-uniform code on
   * those numbers, same expressions in the same order */
  int bestLastIdxP1 = 0;
  {
    double bestCost = blockUncodedCost + lambda * (double)cb(cbfCtx, 0);
    baseCost += lambda * (double)cb(cbfCtx, 1);
    const LastCtx L = last_ctx_of(S, log2);
    LaneVar<double> wCl;
    if (inRegs) FCU_FOR_LANES_REG { if (lane <= lastScanPos) wCl.set(lane, vLv.own(lane) ? rate_last(cb, S, L, log2, scanType, lane) : 0.0); }
    int foundLast = 0;
    for (int cgScanPos = cgLastScanPos; cgScanPos >= 0 && !foundLast; cgScanPos--) {
      const int lb = inRegs ? cgScanPos << 4 : 0;
      const int cgBlk = vCgBlk.get(cgScanPos);
      baseCost -= vCgSig.get(cgScanPos);
      if (!((cgflag >> cgBlk) & 1)) continue;
      const int top = (cgScanPos * 16 + 15 > lastScanPos) ? lastScanPos - cgScanPos * 16 : 15;   /* positions above the last one are skipped */
      if (!inRegs) FCU_FOR_LANES_REG {
        if (lane <= top) {
          const int scanPos = cgScanPos * 16 + lane;
          const int lv = dstg[scanPos];
          const RdoqRec q = recg[scanPos];
          vLv.set(lane, lv); vCs.set(lane, q.cs); vCc.set(lane, q.cc); vC0.set(lane, q.c0);
          wCl.set(lane, lv ? rate_last(cb, S, L, log2, scanType, scanPos) : 0.0);
        }
      }
      for (int posInCG = top; posInCG >= 0; posInCG--) {
        const int ln = lb + posInCG;
        const int lv = vLv.get(ln); const double curCs = vCs.get(ln);
        if (lv) {
          const double totalCost = baseCost + wCl.get(ln) - curCs;
          if (totalCost < bestCost) { bestLastIdxP1 = cgScanPos * 16 + posInCG + 1; bestCost = totalCost; }
          if (lv > 1) { foundLast = 1; break; }
          baseCost -= vCc.get(ln); baseCost += vC0.get(ln);
        } else baseCost -= curCs;
      }
    }
  }
  FCU_TAIL_COUNT(TAIL_LAST_ZERO, bestLastIdxP1 == 0);
  FCU_WTOC(P, wt_, 2, log2);
  /* rdoq_signs with a position per lane: the sign of the source value on the kept levels, 0 above the chosen last position;
   * uiAbsSum is one wave sum.  Invariant the passes below rely on: a LaneVar starts as 0 in every lane (on the device as in the
   * emulator), this pass sets vAcc in all 64 lanes, and for a block in registers vLv too; lanes of groups that were never
   * walked (>= nStore) hold level 0 and source 0, and every ballot, get and put below stays inside the walked groups. */
  LaneVar<int> vAcc;
  if (inRegs) FCU_FOR_LANES_REG {
    const int lv = lane < bestLastIdxP1 ? vLv.own(lane) : 0;
    vAcc.set(lane, lv); vLv.set(lane, vNext.own(lane) < 0 ? -lv : lv);
  }
  else FCU_FOR_LANES {
    uint32_t acc = 0;
    for (int sp = lane; sp <= lastScanPos; sp += 64) {
      if (sp < bestLastIdxP1) { const int lv = dstg[sp]; acc += (uint32_t)lv; dstg[sp] = (int16_t)((srcg[sp] < 0) ? -lv : lv); }
      else dstg[sp] = 0;
    }
    vAcc.set(lane, (int)acc);
  }
  const int absSum = lane_sum(vAcc);
  FCU_WTOC(P, wt_, 3, log2);
  /* sign bit hiding (TComTrQuant.cpp:2442-2572) per group from the top, as rdoq_sign_hiding() walks them: the group's masks
   * come from ballots; in a group whose parity is wrong every lane prices the change of its own position exactly as the serial
   * loop body does (positions above the loop's start keep an infinite cost), and the position with the smallest cost takes it.
   * Among equal costs the serial loop, which descends with a strict <, keeps the highest position: so does the scan here.  A
   * larger block fetches level, record and source value of the group's sixteen positions in one round trip first. */
  int last = bestLastIdxP1 - 1;                                /* the level there is non-zero; sign hiding may clear it */
  if (P.sign_hiding && absSum >= 2) {
    const long long rdFactor = P.rd_factor[ch], kInf = 0x7fffffffffffffffLL;
    int lastCG = -1;
    for (int subSet = (bestLastIdxP1 - 1) >> 4; subSet >= 0; subSet--) {   /* groups above hold no level any more */
      if (!((cgflag >> vCgBlk.get(subSet)) & 1)) continue;     /* every level of the group is 0 (and a larger block has stored no records for it) */
      const int lb = inRegs ? subSet << 4 : 0, subPos = subSet << 4;
      if (!inRegs) FCU_FOR_LANES_REG {
        if (lane < 16) {
          const RdoqRec q = recg[subPos + lane];
          vLv.set(lane, dstg[subPos + lane]); vNext.set(lane, srcg[subPos + lane]);
          vUp.set(lane, q.up); vDn.set(lane, q.dn); vSd.set(lane, q.sd); vDu.set(lane, q.du);
        }
      }
      const uint32_t nzMask = lane_nz16(vLv, lb);
      if (!nzMask) continue;
      const int lastNZ = 31 - __builtin_clz(nzMask), firstNZ = __builtin_ctz(nzMask);
      if (lastCG == -1) lastCG = 1;
      if (lastNZ - firstNZ >= 4) {
        const uint32_t signbit = vLv.get(lb + firstNZ) < 0 ? 1 : 0;
        if (signbit != (uint32_t)(__builtin_popcount(lane_odd16(vLv, lb)) & 1)) {    /* the parity of the sum of the levels */
          const int nTop = lastCG == 1 ? lastNZ : 15;          /* where the serial loop starts */
          LaneVar<int> vCostLo, vCostHi, vChg;
          FCU_FOR_LANES_REG {
            const int n = lane - lb;
            long long curCost = kInf; int curChange = 0;
            if (n >= 0 && n <= nTop)
              curCost = sh_cost(vLv.own(lane), vDu.own(lane), vUp.own(lane), vDn.own(lane), vSd.own(lane), vNext.own(lane) < 0, n, firstNZ, lastNZ, lastCG, signbit, rdFactor, &curChange);
            vCostLo.set(lane, (int)(uint32_t)(unsigned long long)curCost); vCostHi.set(lane, (int)(curCost >> 32)); vChg.set(lane, curChange);
          }
          long long minCostInc = kInf; int minN = -1;
          for (int n = nTop; n >= 0; --n) {
            const long long curCost = (long long)(((unsigned long long)(uint32_t)vCostHi.get(lb + n) << 32) | (uint32_t)vCostLo.get(lb + n));
            if (curCost < minCostInc) { minCostInc = curCost; minN = n; }
          }
          if (minN >= 0) {
#ifdef FCU_EMU
            { int same = 0;
              for (int n = nTop; n >= 0; --n) same += vCostHi.get(lb + n) == vCostHi.get(lb + minN) && vCostLo.get(lb + n) == vCostLo.get(lb + minN);
              FCU_TAIL_COUNT(TAIL_SH_TIE, same > 1); }
#endif
            const int old = vLv.get(lb + minN); int finalChange = vChg.get(lb + minN);
            if (old == 32767 || old == -32768) finalChange = -1;
            const int nv = (int)(int16_t)(vNext.get(lb + minN) >= 0 ? old + finalChange : old - finalChange);
            vLv.put(lb + minN, nv);
            if (!inRegs) FCU_FOR_LANES_REG { if (lane == 0) dstg[subPos + minN] = (int16_t)nv; }
            FCU_TAIL_COUNT(TAIL_SH_4X4, log2 == 2); FCU_TAIL_COUNT(TAIL_SH_8X8_LOW, log2 == 3 && lastCG == 0); FCU_TAIL_COUNT(TAIL_SH_BIG, log2 >= 4);
          } else {
            /* No position with a finite cost: the reference (and rdoq_sign_hiding) would index position -1 here.  That case is
             * given no meaning: nothing changes, the emulator counts it and the tests require the count to stay 0. */
            FCU_TAIL_COUNT(TAIL_SH_NO_FINITE, 1);
#ifdef FCU_EMU_CHECK_RDOQ_TAIL
            chkSkip = 1;
#endif
          }
        }
      }
      if (lastCG == 1) {                                       /* the top group with a level: the block's last level is here */
        const uint32_t nzNow = lane_nz16(vLv, lb);
        last = subPos + 31 - __builtin_clz(nzNow);             /* (two levels four apart, or none changed: never empty) */
        FCU_TAIL_COUNT(TAIL_SH_CLEARED_LAST, last != bestLastIdxP1 - 1);
        lastCG = 0;
      }
    }
  }
  if (inRegs) {                                                /* the only store of a block in registers: a level per lane */
    FCU_FOR_LANES { if (lane < nStore) dstg[lane] = (int16_t)vLv.own(lane); if (lane == 0) { g_S.rw_abs = absSum; g_S.rw_lsp = last; } }
  } else {
    FCU_SERIAL { g_S.rw_abs = absSum; g_S.rw_lsp = last; }
  }
  FCU_WTOC(P, wt_, 4, log2);
#ifdef FCU_EMU_CHECK_RDOQ_TAIL
  if (!chkSkip) {                                              /* the serial passes on what the pool form stored */
    const RdoqOut o = rdoq_finish(cb, P, S, srcg, chkLv, recg, cgg, 1, log2, scanType, cbfCtx, cgflag, cgLastScanPos, lastScanPos, chkBase, blockUncodedCost);
    int bad = o.abs_sum != g_S.rw_abs || o.last != g_S.rw_lsp;
    for (int sp = 0; sp < nStore; sp++) bad |= chkLv[sp] != dstg[sp];
    if (bad) {
      fprintf(stderr, "FCU_EMU_CHECK_RDOQ_TAIL: rdoq_wave differs from rdoq_finish (log2 %d comp %d scan %d topNZ %d: abs %d / %d, last %d / %d)\n",
              log2, comp, scanType, topNZ, g_S.rw_abs, o.abs_sum, g_S.rw_lsp, o.last);
      abort();
    }
  }
#endif
}

/* ======================================================================================== */
/* intra prediction: closed form per pixel (TComPrediction.cpp:183-496,755-841)              */
/* ======================================================================================== */
FCU_DEV int use_filtered_ref(int mode, int log2, int isLuma)               /* TComPattern.cpp:523-548 */
{
  if (!isLuma || mode == DC) return 0;
  const int d1 = iabs(mode - HOR), d2 = iabs(mode - VER);
  return (d1 < d2 ? d1 : d2) > k_filter_thr[log2 - 2];
}
/* ref[0..4N]: bottom-left ... corner(2N) ... top-right.  corner[+i] = top(i-1), corner[-i] = left(i-1) */
FCU_DEV int pred_pixel(const uint8_t *ref, int log2, int mode, int isLuma, int dc, int x, int y)
{
  const int N = 1 << log2;
  const uint8_t *corner = ref + 2 * N;
  if (mode == PLANAR)
    return ((N - 1 - x) * corner[-1 - y] + (x + 1) * corner[1 + N] + (N - 1 - y) * corner[1 + x] + (y + 1) * corner[-1 - N] + N) >> (log2 + 1);
  if (mode == DC) {
    int v = dc;
    if (isLuma && N <= 16) {
      if (x == 0 && y == 0) v = (corner[1] + corner[-1] + 2 * dc + 2) >> 2;
      else if (y == 0) v = (corner[1 + x] + 3 * dc + 2) >> 2;
      else if (x == 0) v = (corner[-1 - y] + 3 * dc + 2) >> 2;
    }
    return v;
  }
  const int isVer = mode >= 18;
  const int angMode = isVer ? mode - VER : -(mode - HOR);
  /* intraPredAngle / invAngle (TComPrediction.cpp:287-288) packed into constants: 9 x 6 bits, 8 x 13 bits (no table loads per pixel) */
  const int absAng = iabs(angMode);
  const int angAbs = (int)((0x2069544d245080ull >> (6 * absAng)) & 63);
  const int invAngle = absAng == 0 ? 0 : (int)(((absAng <= 4 ? 0x13b0e38ccd000ull : 0x8004ec30c1e2ull) >> (13 * ((absAng - 1) & 3))) & 8191);
  const int angle = angMode < 0 ? -angAbs : angAbs;
  const int px = isVer ? x : y, py = isVer ? y : x, ms = isVer ? 1 : -1;   /* main array direction from the corner */
  if (angle == 0) {
    int v = corner[ms * (px + 1)];
    if (isLuma && N <= 16 && px == 0) v = clip8(v + ((corner[-ms * (py + 1)] - corner[0]) >> 1));
    return v;
  }
  const int deltaPos = (py + 1) * angle, di = deltaPos >> 5, df = deltaPos & 31;
  const int i0 = px + di + 1;
  int r0, r1;
  { int i = i0; r0 = (i >= 0) ? corner[ms * i] : corner[-ms * ((128 + (-i) * invAngle) >> 8)]; }
  if (!df) return r0;
  { int i = i0 + 1; r1 = (i >= 0) ? corner[ms * i] : corner[-ms * ((128 + (-i) * invAngle) >> 8)]; }
  return ((32 - df) * r0 + df * r1 + 16) >> 5;
}

/* z-scan availability (H.265 6.4.1 == getPULeft/Above/.../BelowLeftAdi, TComDataCU.cpp:1071-1390) */
FCU_DEV int unit_available(const Env E, int lx, int ly, int cx, int cy)
{
  const Params &P = E.C->p;
  if (lx < 0 || ly < 0 || lx >= P.width || ly >= P.height) return 0;
  const int ctuN = (ly >> 6) * E.C->w_ctu + (lx >> 6), ctuC = (cy >> 6) * E.C->w_ctu + (cx >> 6);
  if (ctuN < E.slice_start || !in_tile(E, lx >> 6, ly >> 6)) return 0;
  if (ctuN < ctuC) return 1;
  if (ctuN > ctuC) return 0;
  return zidx_of(lx, ly) < zidx_of(cx, cy);
}

/* Reference samples of a block (initAdiPatternChType + fillReferenceSamples + smoothing,
 * TComPattern.cpp:104-521) -> g_S.ref (unfiltered), g_S.reff (filtered, luma only), g_S.dc. */
FCU_DEV FCU_NOINLINE void build_ref(int comp, int px, int py, int log2, int wantFilt)
{
  const Env E = env_get(); comp = FCU_UNI(comp); px = FCU_UNI(px); py = FCU_UNI(py); log2 = FCU_UNI(log2); wantFilt = FCU_UNI(wantFilt);
  const int N = 1 << log2, sh = comp ? 1 : 0, unit = 4 >> sh, total = 4 * N + 1;
  const int lx0 = px << sh, ly0 = py << sh;
  const uint8_t *rec = E.C->rec[comp]; const int stride = E.C->stride[comp];
  uint8_t *ref = g_S.ref, *avail = (uint8_t *)g_S.colsum;    /* availability flags staged in colsum (>= 257 bytes) */
  FCU_FOR_LANES {
    if (lane == 0) g_S.ref_tag = -1;
    for (int i = lane; i < total; i += 64) {
      int a, v = 0;
      if (i < 2 * N) { const int y = 2 * N - 1 - i; a = unit_available(E, lx0 - 4, ((py + y) / unit * unit) << sh, lx0, ly0); if (a) v = rec[(py + y) * stride + px - 1]; }
      else if (i == 2 * N) { a = unit_available(E, lx0 - 4, ly0 - 4, lx0, ly0); if (a) v = rec[(py - 1) * stride + px - 1]; }
      else { const int x = i - 2 * N - 1; a = unit_available(E, ((px + x) / unit * unit) << sh, ly0 - 4, lx0, ly0); if (a) v = rec[(py - 1) * stride + px + x]; }
      avail[i] = (uint8_t)a; ref[i] = (uint8_t)v;
    }
  }
  /* substitution: every unavailable sample takes the nearest available one below it in walk
   * order, or (for the leading run) the first available one */
  FCU_FOR_LANES {
    for (int i = lane; i < total; i += 64) {
      if (!avail[i]) {
        int j = i - 1;
        while (j >= 0 && !avail[j]) j--;
        if (j < 0) { j = i + 1; while (j < total && !avail[j]) j++; }
        g_S.reff[i] = (j < total) ? ref[j] : 128;            /* staged in reff, merged below */
      }
    }
  }
  FCU_FOR_LANES { for (int i = lane; i < total; i += 64) if (!avail[i]) ref[i] = g_S.reff[i]; }
  FCU_FOR_LANES {
    if (lane == 0) { int sum = 0; for (int i = 0; i < N; i++) sum += ref[2 * N + 1 + i] + ref[2 * N - 1 - i]; g_S.dc = (sum + N) >> (log2 + 1); }
    if (wantFilt) {
      int strong = 0;
      if (comp == 0 && E.C->p.strong_smoothing && N >= 32) {
        const int bl = ref[0], tl = ref[2 * N], tr = ref[4 * N];
        strong = (iabs(bl + tl - 2 * ref[N]) < 8) && (iabs(tl + tr - 2 * ref[3 * N]) < 8);
      }
      for (int i = lane; i < total; i += 64) {
        int v;
        if (i == 0 || i == 4 * N) v = ref[i];
        else if (strong) {
          const int bl = ref[0], tl = ref[2 * N], tr = ref[4 * N];
          if (i < 2 * N) v = ((2 * N - i) * bl + i * tl + N) >> (log2 + 1);
          else if (i == 2 * N) v = tl;
          else { const int k = i - 2 * N; v = ((2 * N - k) * tl + k * tr + N) >> (log2 + 1); }
        } else v = (ref[i - 1] + 2 * ref[i] + ref[i + 1] + 2) >> 2;
        g_S.reff[i] = (uint8_t)v;
      }
    }
  }
}

/* ======================================================================================== */
/* transforms: one output coefficient per call (xTrMxN / xITrMxN, TComTrQuant.cpp:860-987;    */
/* the partial butterflies are exact factorizations of these products)                       */
/* ======================================================================================== */
/* Every stage is a dot product of one basis row with one CONTIGUOUS data row, unrolled per size so that the loads
 * of a row are issued together (wide loads) instead of one dependent load per multiply-add:
 *   fwd1: tmp[k*N + y]   = sum_n T[k][n]  * resi[y*N + n]          fwd2: coef[k2*N + k1] = sum_y T[k2][y] * tmp[k1*N + y]
 *   inv1: tmp2[y*N + kh] = sum_kv Tt[y][kv] * deqT[kh*N + kv]      inv2: resi[y*N + x]   = sum_kh Tt[x][kh] * tmp2[y*N + kh]
 * (Tt = transposed basis; deqT = de-quantised coefficients stored transposed by the caller, see tr_index). */
template <int N, class T>
FCU_DEV int32_t dot_row(const int8_t *m, const T *a)
{
  m = (const int8_t *)__builtin_assume_aligned(m, N >= 16 ? 16 : N);
  a = (const T *)__builtin_assume_aligned(a, sizeof(T) * N >= 16 ? 16 : 8);
  uint32_t mw[N / 4];                                         /* four basis values per word: N/4 (wide) loads */
  __builtin_memcpy(mw, m, N);
  int32_t s = 0;
#pragma unroll
  for (int n = 0; n < N; n++) s += (int32_t)(int8_t)(mw[n >> 2] >> (8 * (n & 3))) * (int32_t)a[n];
  return s;
}
/* The input line of a lane's dot products, held in registers across the iterations of an element loop.  Every caller walks
 * its outputs with a stride of 64 lanes, and 64 is a multiple of N: inside one block a lane keeps meeting the same input
 * line (N of them per block, every one feeding N outputs).  Re-reading the line per output made each pass stream its whole
 * N x N tile N * N / 64 times through L1 / L2 -- 16 x for 32x32 -- and with thousands of resident chains that stream lands
 * in HBM.  A lane (re)loads its line only when the line's address changes (next candidate block).  The input arrays are
 * never written during the phase that reads them, so the copy cannot go stale; a cache lives for one phase only. */
template <int N, class T> struct RowCache {
  T v[N]; const T *src;
  FCU_MEMBER RowCache() : src(nullptr) {}
  FCU_MEMBER const T *get(const T *p)
  {
    if (p != src) { src = p; __builtin_memcpy(v, (const T *)__builtin_assume_aligned(p, sizeof(T) * N >= 16 ? 16 : 8), sizeof(v)); }
    return v;
  }
};
template <int N, class T>
FCU_DEV int32_t dot_regs(const int8_t *m, const T *a)         /* a: a RowCache line (registers) */
{
  m = (const int8_t *)__builtin_assume_aligned(m, N >= 16 ? 16 : N);
  uint32_t mw[N / 4];
  __builtin_memcpy(mw, m, N);
  int32_t s = 0;
#pragma unroll
  for (int n = 0; n < N; n++) s += (int32_t)(int8_t)(mw[n >> 2] >> (8 * (n & 3))) * (int32_t)a[n];
  return s;
}
/* size dispatch OUTSIDE the element loops: f(std::integral_constant<int, log2>) */
template <class F>
FCU_DEV void by_log2(int log2, F f)
{
  switch (log2) {
    case 2: f(std::integral_constant<int, 2>()); break;
    case 3: f(std::integral_constant<int, 3>()); break;
    case 4: f(std::integral_constant<int, 4>()); break;
    default: f(std::integral_constant<int, 5>()); break;
  }
}
template <int LOG2> FCU_DEV const int8_t *basis_row(int useDst, int k) { return (useDst && LOG2 == 2) ? k_dst4 + k * 4 : k_dct + k_dct_off[LOG2 - 2] + (k << LOG2); }
template <int LOG2> FCU_DEV const int8_t *basis_col(int useDst, int n) { return (useDst && LOG2 == 2) ? k_dst4_t + n * 4 : k_dct_t + k_dct_off[LOG2 - 2] + (n << LOG2); }
FCU_DEV int tr_index(int i, int log2) { const int N = 1 << log2; return ((i & (N - 1)) << log2) + (i >> log2); }   /* raster index of the transposed block */
template <int LOG2> FCU_DEV int32_t fwd1(const int16_t *resi, int useDst, int idx)
{ constexpr int N = 1 << LOG2, s1 = LOG2 - 1; const int k = idx >> LOG2, y = idx & (N - 1); return (dot_row<N>(basis_row<LOG2>(useDst, k), resi + (y << LOG2)) + (1 << (s1 - 1))) >> s1; }
template <int LOG2> FCU_DEV int32_t fwd2(const int32_t *tmp, int useDst, int idx)
{ constexpr int N = 1 << LOG2, s2 = LOG2 + 6; const int k2 = idx >> LOG2, k1 = idx & (N - 1); return (dot_row<N>(basis_row<LOG2>(useDst, k2), tmp + (k1 << LOG2)) + (1 << (s2 - 1))) >> s2; }
template <int LOG2> FCU_DEV int32_t inv1(const int32_t *deqT, int useDst, int idx)
{ constexpr int N = 1 << LOG2; const int y = idx >> LOG2, kh = idx & (N - 1); return clip3i(-32768, 32767, (dot_row<N>(basis_col<LOG2>(useDst, y), deqT + (kh << LOG2)) + 64) >> 7); }
template <int LOG2> FCU_DEV int32_t inv2(const int32_t *tmp2, int useDst, int idx)
{ constexpr int N = 1 << LOG2; const int y = idx >> LOG2, x = idx & (N - 1); return clip3i(-32768, 32767, (dot_row<N>(basis_col<LOG2>(useDst, x), tmp2 + (y << LOG2)) + 2048) >> 12); }
/* three of the four passes with the lane's input line cached (declare one RowCache per element loop) */
template <int LOG2> FCU_DEV int32_t fwd1(RowCache<(1 << LOG2), int16_t> &rc, const int16_t *resi, int useDst, int idx)
{ constexpr int N = 1 << LOG2, s1 = LOG2 - 1; const int k = idx >> LOG2, y = idx & (N - 1); return (dot_regs<N>(basis_row<LOG2>(useDst, k), rc.get(resi + (y << LOG2))) + (1 << (s1 - 1))) >> s1; }
template <int LOG2> FCU_DEV int32_t fwd2(RowCache<(1 << LOG2), int32_t> &rc, const int32_t *tmp, int useDst, int idx)
{ constexpr int N = 1 << LOG2, s2 = LOG2 + 6; const int k2 = idx >> LOG2, k1 = idx & (N - 1); return (dot_regs<N>(basis_row<LOG2>(useDst, k2), rc.get(tmp + (k1 << LOG2))) + (1 << (s2 - 1))) >> s2; }
template <int LOG2> FCU_DEV int32_t inv1(RowCache<(1 << LOG2), int32_t> &rc, const int32_t *deqT, int useDst, int idx)
{ constexpr int N = 1 << LOG2; const int y = idx >> LOG2, kh = idx & (N - 1); return clip3i(-32768, 32767, (dot_regs<N>(basis_col<LOG2>(useDst, y), rc.get(deqT + (kh << LOG2))) + 64) >> 7); }
/* (inv2's input line follows the high index bits: neighbouring lanes share it, one broadcast read per iteration) */
/* The four passes for a 4x4 or 8x8 block whose samples sit one per lane (lane blk + p holds element p of the block; a wave
 * holds four 4x4 blocks or one 8x8 block): the input line of a dot product is fetched from the N lanes that hold it instead of
 * from a pool in scratch.  The same products as above, summed in int32 (the order of the terms cannot matter), so the results
 * are the pool path's bit for bit.  Called with all 64 lanes active; -DFCU_SMALL_TU_POOLS builds the engine without them. */
template <int N>
FCU_DEV int32_t dot_lanes(const int8_t *m, const LaneVar<int> &a, int src0, int step)
{
  m = (const int8_t *)__builtin_assume_aligned(m, N);
  uint32_t mw[N / 4];
  __builtin_memcpy(mw, m, N);
  int32_t s = 0;
#pragma unroll
  for (int n = 0; n < N; n++) s += (int32_t)(int8_t)(mw[n >> 2] >> (8 * (n & 3))) * a.from(src0 + n * step);
  return s;
}
template <int LOG2> FCU_DEV int32_t fwd1_lanes(const LaneVar<int> &resi, int useDst, int blk, int idx)
{ constexpr int N = 1 << LOG2, s1 = LOG2 - 1; const int k = idx >> LOG2, y = idx & (N - 1); return (dot_lanes<N>(basis_row<LOG2>(useDst, k), resi, blk + (y << LOG2), 1) + (1 << (s1 - 1))) >> s1; }
template <int LOG2> FCU_DEV int32_t fwd2_lanes(const LaneVar<int> &tmp, int useDst, int blk, int idx)
{ constexpr int N = 1 << LOG2, s2 = LOG2 + 6; const int k2 = idx >> LOG2, k1 = idx & (N - 1); return (dot_lanes<N>(basis_row<LOG2>(useDst, k2), tmp, blk + (k1 << LOG2), 1) + (1 << (s2 - 1))) >> s2; }
/* deq: the de-quantised coefficients in raster order (lane blk + kv * N + kh), not transposed: the step does what tr_index does */
template <int LOG2> FCU_DEV int32_t inv1_lanes(const LaneVar<int> &deq, int useDst, int blk, int idx)
{ constexpr int N = 1 << LOG2; const int y = idx >> LOG2, kh = idx & (N - 1); return clip3i(-32768, 32767, (dot_lanes<N>(basis_col<LOG2>(useDst, y), deq, blk + kh, N) + 64) >> 7); }
template <int LOG2> FCU_DEV int32_t inv2_lanes(const LaneVar<int> &tmp2, int useDst, int blk, int idx)
{ constexpr int N = 1 << LOG2; const int y = idx >> LOG2, x = idx & (N - 1); return clip3i(-32768, 32767, (dot_lanes<N>(basis_col<LOG2>(useDst, x), tmp2, blk + (y << LOG2), 1) + 2048) >> 12); }
/* -DFCU_SMALL_TU_POOLS: the engine without the register path, every size through the candidate pools (tests/test_small_tu_emu.py).
 * tu_trial keeps the pool path for every size: its register path was built and measured, gave nothing on top of the first
 * pass's and grew the kernels' private segment by 240 B per lane (profiles/small_tu_resources.txt). */
#ifdef FCU_SMALL_TU_POOLS
#define FCU_SMALL_TU_REGS(log2) 0
#else
#define FCU_SMALL_TU_REGS(log2) ((log2) <= 3)
#endif
struct DeqParams { int scale, rs, lo, hi; };                /* xDeQuant flat, TComTrQuant.cpp:1242-1352: loop invariants of one TU */
FCU_DEV DeqParams deq_params(int log2, int qp)
{
  DeqParams d;
  const int per = qp / 6, rem = qp % 6;
  d.rs = 6 - ((15 - 8 - log2) + per); d.scale = k_inv_quant_scales[rem];
  int tbd = 32 + d.rs - 7; if (tbd > 16) tbd = 16;
  d.lo = -(1 << (tbd - 1)); d.hi = (1 << (tbd - 1)) - 1;
  return d;
}
FCU_DEV int32_t dequant1(int q, const DeqParams &d)
{
  const int c = clip3i(d.lo, d.hi, q);
  if (d.rs > 0) return clip3i(-32768, 32767, (c * d.scale + (1 << (d.rs - 1))) >> d.rs);
  return clip3i(-32768, 32767, (c * d.scale) << (-d.rs));
}

/* ======================================================================================== */
/* neighbour decisions (MPM, split context)                                                  */
/* ======================================================================================== */
FCU_DEV int inside_cu(const CuObj *cu, int lx, int ly) { const int s = CTU >> cu->depth_cu; return lx >= cu->x && lx < cu->x + s && ly >= cu->y && ly < cu->y + s; }
FCU_DEV int nb_depth(const Env E, const CuObj *cu, int lx, int ly)
{ return inside_cu(cu, lx, ly) ? cu->depth[zidx_of(lx, ly) - cu->zidx] : E.C->out[(ly >> 6) * E.C->w_ctu + (lx >> 6)].depth[zidx_of(lx, ly)]; }
FCU_DEV int nb_luma_dir(const Env E, const CuObj *cu, int lx, int ly)
{
  if (inside_cu(cu, lx, ly)) { const int p = zidx_of(lx, ly) - cu->zidx; return cu->pred_mode[p] == MODE_INTRA ? cu->intra_dir[0][p] : DC; }
  const fcu_ctu_out *c = &E.C->out[(ly >> 6) * E.C->w_ctu + (lx >> 6)]; const int p = zidx_of(lx, ly);
  return c->pred_mode[p] == MODE_INTRA ? c->intra_dir[0][p] : DC;
}
FCU_DEV int left_ctu_ok(const Env E, int lx, int ly) { if (lx == 0) return 0; if (lx & 63) return 1; return (ly >> 6) * E.C->w_ctu + (lx >> 6) - 1 >= E.slice_start && (lx >> 6) > E.tx0; }
FCU_DEV int above_ctu_ok(const Env E, int lx, int ly) { if (ly == 0) return 0; if (ly & 63) return 1; return (ly >> 6) * E.C->w_ctu + (lx >> 6) - E.C->w_ctu >= E.slice_start && (ly >> 6) > E.ty0; }
/* getIntraDirPredictor, TComDataCU.cpp:1542-1624 */
FCU_DEV int intra_dir_predictor(const Env E, const CuObj *cu, int part, int *preds)
{
  const int z = cu->zidx + part, lx = (cu->x & ~63) + part_x(z), ly = (cu->y & ~63) + part_y(z);
  const int left = left_ctu_ok(E, lx, ly) ? nb_luma_dir(E, cu, lx - 1, ly) : DC;
  const int above = ((ly & 63) != 0) ? nb_luma_dir(E, cu, lx, ly - 1) : DC;
  if (left == above) {
    if (left > 1) { preds[0] = left; preds[1] = ((left + 29) % 32) + 2; preds[2] = ((left - 1) % 32) + 2; }
    else { preds[0] = PLANAR; preds[1] = DC; preds[2] = VER; }
    return 1;
  }
  preds[0] = left; preds[1] = above;
  preds[2] = (left && above) ? PLANAR : ((left + above) < 2 ? VER : DC);
  return 2;
}
FCU_DEV int min_tu_log2_in_cu(int depth, int partSize)      /* getQuadtreeTULog2MinSizeInCU, TComDataCU.cpp:1658-1686 */
{
  const int log2Cb = 6 - depth, split = partSize == SIZE_NxN;
  if (log2Cb < LOG2_MINTU + TU_MAXDEPTH_INTRA - 1 + split) return LOG2_MINTU;
  const int m = log2Cb - (TU_MAXDEPTH_INTRA - 1 + split);
  return m > LOG2_MAXTU ? LOG2_MAXTU : m;
}

#include "fcu_inter.h"

/* ---- syntax element coders (serial, any Cabac) ------------------------------------------ */
FCU_DEV void code_split_flag(const Env E, int c, const CuObj *cu, int part, int depth)   /* TEncSbac.cpp:613-628 */
{
  if (depth == MAXDEPTH) return;
  const int z = cu->zidx + part, lx = (cu->x & ~63) + part_x(z), ly = (cu->y & ~63) + part_y(z);
  int ctx = 0;
  if (left_ctu_ok(E, lx, ly)) ctx += nb_depth(E, cu, lx - 1, ly) > depth;
  if (above_ctu_ok(E, lx, ly)) ctx += nb_depth(E, cu, lx, ly - 1) > depth;
  cab_bin(c, cu->depth[part] > depth, CTX_SPLIT + ctx);
}
/* codeIntraDirLumaAng for one PU with known MPM list (TEncSbac.cpp:643-696) */
FCU_DEV void code_luma_dir_bits(int c, int dir, const int *preds)
{
  int predIdx = -1;
  for (int i = 0; i < 3; i++) if (dir == preds[i]) predIdx = i;
  cab_bin(c, predIdx != -1, CTX_INTRA_LUMA);
  cab_ep(c, predIdx != -1 ? (predIdx ? 2 : 1) : 5);
}
FCU_DEV FCU_NOINLINE void code_intra_dir_luma(int c, const CuObj *cu, int part, int multiple)
{
  const Env E = env_get(); c = FCU_UNI(c); cu = FCU_UNI(cu); part = FCU_UNI(part); multiple = FCU_UNI(multiple);
  int preds[4][3], predIdx[4];
  const int partNum = multiple ? (cu->part_size[part] == SIZE_NxN ? 4 : 1) : 1;
  const int partOffset = (NPART >> (cu->depth[part] << 1)) >> 2;
  for (int j = 0; j < partNum; j++) {
    const int dir = cu->intra_dir[0][part + partOffset * j];
    intra_dir_predictor(E, cu, part + partOffset * j, preds[j]);
    predIdx[j] = -1;
    for (int i = 0; i < 3; i++) if (dir == preds[j][i]) predIdx[j] = i;
    cab_bin(c, predIdx[j] != -1, CTX_INTRA_LUMA);
  }
  for (int j = 0; j < partNum; j++) cab_ep(c, predIdx[j] != -1 ? (predIdx[j] ? 2 : 1) : 5);
}
FCU_DEV void code_intra_dir_chroma(int c, int dir)       /* TEncSbac.cpp:698-725 */
{ if (dir == DM_CHROMA) cab_bin(c, 0, CTX_CHROMA_PRED); else { cab_bin(c, 1, CTX_CHROMA_PRED); cab_ep(c, 2); } }
FCU_DEV int chroma_final_mode(const CuObj *cu, int part) { int m = cu->intra_dir[1][part]; return m == DM_CHROMA ? cu->intra_dir[0][part & ~3] : m; }

/* search-time tree walkers: xEncSubdivCbfQT / xEncCoeffQT / xGetIntraBitsQT, TEncSearch.cpp:866-1090 */
FCU_DEV FCU_NOINLINE void enc_subdiv_cbf_qt(int c, const CuObj *cu, uint32_t root_k, int bLuma, int bChroma)
{
  const Env E = env_get(); c = FCU_UNI(c); cu = FCU_UNI(cu); const TU root = tu_of_key(FCU_UNI(root_k)); bLuma = FCU_UNI(bLuma); bChroma = FCU_UNI(bChroma);
  TU *st = g_S.wk_st; int *ci = g_S.wk_ci; int sp = 0;
  st[0] = root; ci[0] = -1;
  while (sp >= 0) {
    const TU tu = st[sp];
    if (ci[sp] < 0) {
      const int subdiv = cu->tr_idx[tu.part] > tu.tr_depth;
      if (cu->part_size[0] == SIZE_NxN && tu.tr_depth == 0) { }
      else if (tu.log2 > LOG2_MAXTU) { }
      else if (tu.log2 == LOG2_MINTU) { }
      else if (tu.log2 == min_tu_log2_in_cu(cu->depth[tu.part], cu->part_size[tu.part])) { }
      else if (bLuma) cab_bin(c, subdiv, CTX_SUBDIV + 5 - tu.log2);
      if (bChroma)
        for (int comp = 1; comp < 3; comp++)
          if (tu.c_code_all && (tu.tr_depth == 0 || ((cu->cbf[comp][tu.part] >> (tu.tr_depth - 1)) & 1))) {
            const int lowest = tu.tr_depth + ((subdiv && !(tu.cw >= 8)) ? 1 : 0);
            cab_bin(c, (cu->cbf[comp][tu_part_c(tu)] >> lowest) & 1, CTX_CBF_CHROMA + tu.tr_depth);
          }
      if (!subdiv) { if (bLuma) cab_bin(c, (cu->cbf[0][tu.part] >> tu.tr_depth) & 1, CTX_CBF_LUMA + (tu.tr_depth == 0 ? 1 : 0)); sp--; continue; }
      ci[sp] = 0;
    }
    if (ci[sp] >= 4) { sp--; continue; }
    { TU ch; tu_child(ch, st[sp], ci[sp], 0); ci[sp]++; sp++; st[sp] = ch; ci[sp] = -1; }
  }
  (void)E;
}
FCU_DEV FCU_NOINLINE void enc_coeff_qt(int c, const CuObj *cu, uint32_t root_k, int comp, int realCoeff)
{
  const Env E = env_get(); c = FCU_UNI(c); cu = FCU_UNI(cu); const TU root = tu_of_key(FCU_UNI(root_k)); comp = FCU_UNI(comp); realCoeff = FCU_UNI(realCoeff);
  TU *st = g_S.wk_st; int *ci = g_S.wk_ci; int sp = 0;
  st[0] = root; ci[0] = -1;
  while (sp >= 0) {
    const TU tu = st[sp];
    if (ci[sp] < 0) {
      if (!(cu->tr_idx[tu.part] > tu.tr_depth)) {
        if (!(comp && tu.cw == 0) && ((cu->cbf[comp][tu.part] >> tu.tr_depth) & 1)) {
          const int layer = LOG2_MAXTU - tu.log2;
          const int16_t *buf = realCoeff ? cu->coef[comp] : E.G->qt_coef[comp][layer];
          const int log2 = comp ? ilog2(tu.cw) : tu.log2, pc = comp ? tu_part_c(tu) : tu.part;
          const int dir = comp ? chroma_final_mode(cu, pc) : cu->intra_dir[0][pc];
          code_coeff_nxn<1>(c, buf + (comp ? tu.off_c : tu.off_y), 1, -1, log2, comp, coef_scan_idx(dir, log2, comp), cu->tskip[comp][pc], E.C->p, g_S.lane_abs[0]);
        }
        sp--; continue;
      }
      ci[sp] = 0;
    }
    if (ci[sp] >= 4) { sp--; continue; }
    { TU ch; tu_child(ch, st[sp], ci[sp], 0); ci[sp]++; sp++; st[sp] = ch; ci[sp] = -1; }
  }
}
FCU_DEV void enc_intra_header(const Env E, int c, const CuObj *cu, int trDepth, int part, int bLuma, int bChroma)
{
  if (bLuma) {
    if (part == 0 && E.C->p.slice_type != SLICE_I) { code_skip_flag(E, c, cu, 0); code_pred_mode(c, cu, 0); }   /* TEncSearch.cpp:990-1000 */
    if (part == 0 && cu->depth[0] == MAXDEPTH) cab_bin(c, cu->part_size[0] == SIZE_2Nx2N, CTX_PARTSIZE);
    if (cu->part_size[0] == SIZE_2Nx2N) { if (part == 0) code_intra_dir_luma(c, cu, 0, 0); }
    else { const int q = cu->nparts >> 2; if (trDepth > 0 && (part & (q - 1)) == 0) code_intra_dir_luma(c, cu, part, 0); }
  }
  if (bChroma && part == 0) code_intra_dir_chroma(c, cu->intra_dir[1][part]);
}
FCU_DEV FCU_NOINLINE uint32_t intra_bits_qt(int c, const CuObj *cu, uint32_t tu_k, int bLuma, int bChroma)
{
  const Env E = env_get(); c = FCU_UNI(c); cu = FCU_UNI(cu); const TU tu = tu_of_key(FCU_UNI(tu_k)); bLuma = FCU_UNI(bLuma); bChroma = FCU_UNI(bChroma);
  cab_reset_bits(c);
  enc_intra_header(E, c, cu, tu.tr_depth, tu.part, bLuma, bChroma);
  enc_subdiv_cbf_qt(c, cu, tu_key(tu), bLuma, bChroma);
  if (bLuma) enc_coeff_qt(c, cu, tu_key(tu), 0, 0);
  if (bChroma) { enc_coeff_qt(c, cu, tu_key(tu), 1, 0); enc_coeff_qt(c, cu, tu_key(tu), 2, 0); }
  return cab_bits(c);
}

/* xGetIntraBitsQT (luma only) for the un-split TU that tu_trial() has just coded: the same bins as
 * intra_bits_qt() on a leaf, with the PU's MPM list from the RMD (g_S.preds, same intra_dir_predictor call)
 * and the levels still in scan order in the trial buffers */
FCU_DEV FCU_NOINLINE uint32_t leaf_luma_bits(int c, const CuObj *cu, uint32_t tu_k)
{
  const Env E = env_get(); c = FCU_UNI(c); cu = FCU_UNI(cu); const TU tu = tu_of_key(FCU_UNI(tu_k));
  const int part = tu.part, partSize = cu->part_size[0], log2 = tu.log2;
  cab_reset_bits(c);
  if (part == 0 && E.C->p.slice_type != SLICE_I) { code_skip_flag(E, c, cu, 0); code_pred_mode(c, cu, 0); }
  if (part == 0 && cu->depth[0] == MAXDEPTH) cab_bin(c, partSize == SIZE_2Nx2N, CTX_PARTSIZE);
  if (partSize == SIZE_2Nx2N ? (part == 0) : (tu.tr_depth > 0 && (part & ((cu->nparts >> 2) - 1)) == 0))
    code_luma_dir_bits(c, cu->intra_dir[0][part], g_S.preds);
  if (!(partSize == SIZE_NxN && tu.tr_depth == 0) && log2 != LOG2_MINTU && log2 != min_tu_log2_in_cu(cu->depth[part], cu->part_size[part]))
    cab_bin(c, 0, CTX_SUBDIV + 5 - log2);
  const int cbf = g_S.t_abs > 0;
  cab_bin(c, cbf, CTX_CBF_LUMA + (tu.tr_depth == 0 ? 1 : 0));
  if (cbf) code_coeff_body<1>(c, E.G->p_qscan, 1, g_S.t_lsp, log2, 0, coef_scan_idx(cu->intra_dir[0][part], log2, 0), cu->tskip[0][part], E.C->p, g_S.lane_abs[0]);
  return cab_bits(c);
}

/* final-order CU syntax: encodeCoeff / xEncodeTransform, TEncEntropy.cpp:201-400.  withLuma = 0 leaves out everything the
 * luma search's walk has coded (subdivision flags, luma cbf, luma levels): the chroma cbf bins and the Cb / Cr levels
 * leaf by leaf, in the order of the full walk (check_rd_cost_intra merges the two) */
FCU_DEV FCU_NOINLINE void encode_transform(int c, const CuObj *cu, int cuPart, uint32_t root_k, int withLuma)
{
  const Env E = env_get(); c = FCU_UNI(c); cu = FCU_UNI(cu); cuPart = FCU_UNI(cuPart); const TU root = tu_of_key(FCU_UNI(root_k)); withLuma = FCU_UNI(withLuma);
  TU *st = g_S.wk_st; int *ci = g_S.wk_ci; int sp = 0;
  st[0] = root; ci[0] = -1;
  while (sp >= 0) {
    const TU tu = st[sp];
    if (ci[sp] < 0) {
      const int part = cuPart + tu.part, trIdx = tu.tr_depth, subdiv = cu->tr_idx[part] > trIdx;
      if (cu->part_size[part] == SIZE_NxN && trIdx == 0) { }
      else if (tu.log2 > LOG2_MAXTU) { }
      else if (tu.log2 == LOG2_MINTU) { }
      else if (tu.log2 == min_tu_log2_in_cu(cu->depth[part], cu->part_size[part])) { }
      else if (withLuma) cab_bin(c, subdiv, CTX_SUBDIV + 5 - tu.log2);
      const int first = trIdx == 0;
      for (int comp = 1; comp < 3; comp++)
        if (first || tu.c_code_all)
          if (first || ((cu->cbf[comp][part] >> (trIdx - 1)) & 1)) {
            const int lowest = trIdx + ((subdiv && !(tu.cwo >= 8)) ? 1 : 0);
            cab_bin(c, (cu->cbf[comp][cuPart + tu_part_c(tu)] >> lowest) & 1, CTX_CBF_CHROMA + trIdx);
          }
      if (!subdiv) {
        if (withLuma) cab_bin(c, (cu->cbf[0][part] >> trIdx) & 1, CTX_CBF_LUMA + (trIdx == 0 ? 1 : 0));
        for (int comp = withLuma ? 0 : 1; comp < 3; comp++) {
          if (comp && tu.cw == 0) continue;
          if (!((cu->cbf[comp][part] >> trIdx) & 1)) continue;
          const int log2 = comp ? ilog2(tu.cw) : tu.log2, pc = cuPart + (comp ? tu_part_c(tu) : tu.part);
          const int dir = comp ? chroma_final_mode(cu, pc) : cu->intra_dir[0][pc];
          const int16_t *coef = cu->coef[comp] + (comp ? (cuPart * 4 + tu.off_c) : (cuPart * 16 + tu.off_y));
          { FCU_TIC(ts_); code_coeff_nxn<1>(c, coef, 1, -1, log2, comp, coef_scan_idx(dir, log2, comp), cu->tskip[comp][pc], E.C->p, g_S.lane_abs[0]); FCU_S7_COEFF(E, ts_, comp); }
        }
        sp--; continue;
      }
      ci[sp] = 0;
    }
    if (ci[sp] >= 4) { sp--; continue; }
    { TU ch; tu_child(ch, st[sp], ci[sp], 1); ci[sp]++; sp++; st[sp] = ch; ci[sp] = -1; }
  }
}
FCU_DEV void encode_cu_syntax(const Env E, int c, const CuObj *cu, int cuPart, int depth)   /* TEncCu.cpp:2117-2141 / 1753-1778 */
{
  if (E.C->p.slice_type != SLICE_I) {                        /* encodeSkipFlag / encodePredMode are no-ops in I slices */
    if (cu->pred_mode[cuPart] == MODE_INTER) { encode_cu_syntax_inter(E, c, cu, cuPart, depth); return; }
    code_skip_flag(E, c, cu, cuPart); code_pred_mode(c, cu, cuPart);
  }
  if (depth == MAXDEPTH) cab_bin(c, cu->part_size[cuPart] == SIZE_2Nx2N, CTX_PARTSIZE);
  code_intra_dir_luma(c, cu, cuPart, 1);
  code_intra_dir_chroma(c, cu->intra_dir[1][cuPart]);
  TU root; tu_root(root, depth);
  encode_transform(c, cu, cuPart, tu_key(root), 1);
}

/* ======================================================================================== */
/* CU object helpers (cooperative)                                                           */
/* ======================================================================================== */
FCU_DEV FCU_NOINLINE void cu_init(CuObj *cu, int depth, int x, int y, int zidx)       /* initEstData / initSubCU */
{
  const Env E = env_get(); cu = FCU_UNI(cu); depth = FCU_UNI(depth); x = FCU_UNI(x); y = FCU_UNI(y); zidx = FCU_UNI(zidx);
  const int n = NPART >> (2 * depth), s = CTU >> depth;
  FCU_FOR_LANES {
    if (lane == 0) { cu->cost = FCU_MAX_DOUBLE; cu->dist = 0; cu->bits = 0; cu->bins = 0; cu->depth_cu = depth; cu->x = x; cu->y = y; cu->zidx = zidx; cu->nparts = n; }
    for (int i = lane; i < n; i += 64) {
      cu->depth[i] = (uint8_t)depth; cu->part_size[i] = SIZE_NONE; cu->pred_mode[i] = MODE_NONE; cu->tr_idx[i] = 0;
      cu->tskip[0][i] = cu->tskip[1][i] = cu->tskip[2][i] = 0; cu->cbf[0][i] = cu->cbf[1][i] = cu->cbf[2][i] = 0;
      cu->intra_dir[0][i] = DC; cu->intra_dir[1][i] = 0;
      cu->skip[i] = 0; cu->merge_flag[i] = 0; cu->merge_idx[i] = 0; cu->inter_dir[i] = 0; cu->mvp_idx[i] = -1; cu->ref_idx[i] = -1;
      cu->mv[i][0] = cu->mv[i][1] = 0; cu->mvd[i][0] = cu->mvd[i][1] = 0;
    }
    for (int i = lane; i < s * s; i += 64) cu->coef[0][i] = 0;
    for (int i = lane; i < s * s / 4; i += 64) { cu->coef[1][i] = 0; cu->coef[2][i] = 0; }
  }
  (void)E;
}
FCU_DEV FCU_NOINLINE void cu_copy_part_from(CuObj *dst, const CuObj *src, int partUnitIdx)   /* copyPartFrom */
{
  const Env E = env_get(); dst = FCU_UNI(dst); src = FCU_UNI(src); partUnitIdx = FCU_UNI(partUnitIdx);
  const int n = src->nparts, off = partUnitIdx * n;
  FCU_FOR_LANES {
    if (lane == 0) { dst->dist += src->dist; dst->bits += src->bits; dst->bins += src->bins; }
    for (int i = lane; i < n; i += 64) {
      dst->depth[off + i] = src->depth[i]; dst->part_size[off + i] = src->part_size[i]; dst->pred_mode[off + i] = src->pred_mode[i];
      dst->tr_idx[off + i] = src->tr_idx[i];
      for (int c = 0; c < 3; c++) { dst->tskip[c][off + i] = src->tskip[c][i]; dst->cbf[c][off + i] = src->cbf[c][i]; }
      dst->intra_dir[0][off + i] = src->intra_dir[0][i]; dst->intra_dir[1][off + i] = src->intra_dir[1][i];
      dst->skip[off + i] = src->skip[i]; dst->merge_flag[off + i] = src->merge_flag[i]; dst->merge_idx[off + i] = src->merge_idx[i];
      dst->inter_dir[off + i] = src->inter_dir[i]; dst->mvp_idx[off + i] = src->mvp_idx[i]; dst->ref_idx[off + i] = src->ref_idx[i];
      dst->mv[off + i][0] = src->mv[i][0]; dst->mv[off + i][1] = src->mv[i][1]; dst->mvd[off + i][0] = src->mvd[i][0]; dst->mvd[off + i][1] = src->mvd[i][1];
    }
    for (int i = lane; i < n * 16; i += 64) dst->coef[0][off * 16 + i] = src->coef[0][i];
    for (int i = lane; i < n * 4; i += 64) { dst->coef[1][off * 4 + i] = src->coef[1][i]; dst->coef[2][off * 4 + i] = src->coef[2][i]; }
  }
  (void)E;
}
FCU_DEV FCU_NOINLINE void cu_copy_to_pic(const CuObj *cu)                             /* copyToPic */
{
  const Env E = env_get(); cu = FCU_UNI(cu);
  fcu_ctu_out *p = &E.C->out[E.cur_ctu];
  const int n = cu->nparts, off = cu->zidx, qp = E.C->p.qp;
  FCU_FOR_LANES {
    if (lane == 0) { p->total_cost = cu->cost; p->total_dist = cu->dist; p->total_bits = cu->bits; p->total_bins = cu->bins; }
    for (int i = lane; i < n; i += 64) {
      p->depth[off + i] = cu->depth[i]; p->width[off + i] = p->height[off + i] = (uint8_t)(CTU >> cu->depth[i]);   /* the sub-CUs' own sizes */ p->skip[off + i] = cu->skip[i];
      p->merge_flag[off + i] = cu->merge_flag[i]; p->merge_idx[off + i] = cu->merge_idx[i]; p->inter_dir[off + i] = cu->inter_dir[i];
      p->mvp_idx[off + i] = cu->mvp_idx[i]; p->ref_idx[off + i] = cu->ref_idx[i];
      p->mv[off + i][0] = cu->mv[i][0]; p->mv[off + i][1] = cu->mv[i][1]; p->mvd[off + i][0] = cu->mvd[i][0]; p->mvd[off + i][1] = cu->mvd[i][1];
      p->part_size[off + i] = cu->part_size[i]; p->pred_mode[off + i] = cu->pred_mode[i]; p->qp[off + i] = (int8_t)qp;
      p->tr_idx[off + i] = cu->tr_idx[i];
      for (int c = 0; c < 3; c++) { p->tskip[c][off + i] = cu->tskip[c][i]; p->cbf[c][off + i] = cu->cbf[c][i]; }
      p->intra_dir[0][off + i] = cu->intra_dir[0][i]; p->intra_dir[1][off + i] = cu->intra_dir[1][i];
    }
    /* m_pcTrCoeff is raster order inside each TU; the engine keeps scan order, converted here.  Only the
     * depth-0 call matters for the coefficients (it rewrites the whole CTU and nothing reads them before). */
    if (cu->depth_cu == 0) {
      for (int i = lane; i < 4096; i += 64) {
        const int part = i >> 4; int v = 0;
        if (cu->pred_mode[part] != MODE_NONE) {
          const int log2 = 6 - cu->depth[part] - cu->tr_idx[part], np = 1 << (2 * (log2 - 2)), tp = part & ~(np - 1);
          const int st = cu->pred_mode[part] == MODE_INTRA ? coef_scan_idx(cu->intra_dir[0][tp], log2, 0) : 0;   /* inter: SCAN_DIAG */
          v = cu->coef[0][tp * 16 + k_iscan[k_scan_off[st * 4 + log2 - 2] + (i - tp * 16)]];
          if (cu->pred_mode[part] == MODE_INTER && !cu->cbf[0][part]) v = 0;   /* dropped residual: the levels of an earlier candidate are still there */
        }
        p->coeff_y[i] = v;
      }
      for (int i = lane; i < 1024; i += 64) {
        const int part = i >> 2; int vb = 0, vr = 0;
        if (cu->pred_mode[part] != MODE_NONE) {
          const int ll = 6 - cu->depth[part] - cu->tr_idx[part];            /* luma TU; chroma is half of it, 4x4 covers four luma 4x4 */
          const int log2 = ll > 2 ? ll - 1 : 2, np = ll > 2 ? 1 << (2 * (ll - 2)) : 4, tp = part & ~(np - 1);
          const int mode = chroma_final_mode(cu, tp), o = k_scan_off[(cu->pred_mode[part] == MODE_INTRA ? coef_scan_idx(mode, log2, 1) : 0) * 4 + log2 - 2];
          const int sp = k_iscan[o + (i - tp * 4)];
          vb = cu->coef[1][tp * 4 + sp]; vr = cu->coef[2][tp * 4 + sp];
          if (cu->pred_mode[part] == MODE_INTER) { if (!cu->cbf[1][part]) vb = 0; if (!cu->cbf[2][part]) vr = 0; }
        }
        p->coeff_cb[i] = vb; p->coeff_cr[i] = vr;
      }
    }
  }
}
FCU_DEV FCU_NOINLINE void copy_reco_to_pic(const Yuv *r, int x, int y, int s)
{
  const Env E = env_get(); r = FCU_UNI(r); x = FCU_UNI(x); y = FCU_UNI(y); s = FCU_UNI(s);
  FCU_FOR_LANES {
    for (int c = 0; c < 3; c++) {
      const int sh = c ? 1 : 0, bs = c ? 32 : 64, w = E.C->p.width >> sh, h = E.C->p.height >> sh;
      const uint8_t *src = c == 0 ? r->y : (c == 1 ? r->u : r->v);
      const int px = x >> sh, py = y >> sh, n = s >> sh;
      for (int i = lane; i < n * n; i += 64) { const int yy = i / n, xx = i % n; if (py + yy < h && px + xx < w) E.C->rec[c][(py + yy) * E.C->stride[c] + px + xx] = src[yy * bs + xx]; }
    }
  }
}

/* ======================================================================================== */
/* generic (sequential-candidate) TU trial: xIntraCodingTUBlock, TEncSearch.cpp:1092-1387    */
/* pixel phases use all lanes, RDOQ runs on lane 0 against coder `*cab`                       */
/* ======================================================================================== */
FCU_DEV FCU_NOINLINE void tu_trial(CuObj *cu, uint32_t tu_k, int comp, int cab, int save1load2)
{
  const Env E = env_get(); cu = FCU_UNI(cu); const TU tu = tu_of_key(FCU_UNI(tu_k)); comp = FCU_UNI(comp); cab = FCU_UNI(cab); save1load2 = FCU_UNI(save1load2);
  Scratch *G = E.G; const Params &P = E.C->p;
  if (comp && tu.cw == 0) { FCU_SERIAL { g_S.t_dist = 0; g_S.t_abs = 0; g_S.t_lsp = -1; } return; }
  FCU_TIC(t11_);
  const int d = cu->depth_cu, N = comp ? tu.cw : (1 << tu.log2), log2 = ilog2(N), n2 = N * N;
  const int bx = comp ? tu.cx : tu.x, by = comp ? tu.cy : tu.y, bs = comp ? 32 : 64, sh = comp ? 1 : 0;
  const int part = tu.part, layer = LOG2_MAXTU - tu.log2;
  uint8_t *org = yuv_plane(&G->org[d], comp) + by * bs + bx;
  uint8_t *pred = yuv_plane(&G->predt[d], comp) + by * bs + bx;
  uint8_t *recqt = yuv_plane(&G->qt_rec[layer], comp) + by * bs + bx;
  const int px = (cu->x >> sh) + bx, py = (cu->y >> sh) + by;
  uint8_t *recpic = E.C->rec[comp] + py * E.C->stride[comp] + px; const int rs = E.C->stride[comp];
  int16_t *coef = G->qt_coef[comp][layer] + (comp ? tu.off_c : tu.off_y);
  const int useTS = cu->tskip[comp][part];
  const int mode = comp ? chroma_final_mode(cu, part) : cu->intra_dir[0][part];
  const int useDst = comp == 0 && log2 == 2;
  const int qp = comp ? P.qp_c : P.qp;

  const int filt = use_filtered_ref(mode, log2, comp == 0);
  if (save1load2 != 2) build_ref(comp, px, py, log2, filt);
  FCU_PTIC(tp_);
  const int scanType = coef_scan_idx(mode, log2, comp), qbits = rdoq_qbits(log2, qp), qscale = k_quant_scales[qp % 6];
  const uint16_t *iscan = k_iscan + k_scan_off[scanType * 4 + log2 - 2];
  if (save1load2 != 2) {
    FCU_FOR_LANES {
      const uint8_t *r = filt ? g_S.reff : g_S.ref; const int dc = g_S.dc;
      if (lane == 0) g_S.t_last = -1;
      for (int i = lane; i < n2; i += 64) {
        const int y = i >> log2, x = i & (N - 1);
        const int v = pred_pixel(r, log2, mode, comp == 0, dc, x, y);
        pred[y * bs + x] = (uint8_t)v;
        if (save1load2 == 1) G->shared_pred[comp][i] = (uint8_t)v;
        G->p_resi[i] = (int16_t)(org[y * bs + x] - v);
      }
    }
  } else {
    FCU_FOR_LANES {
      if (lane == 0) g_S.t_last = -1;
      for (int i = lane; i < n2; i += 64) {
        const int y = i >> log2, x = i & (N - 1); const int v = G->shared_pred[comp][i];
        pred[y * bs + x] = (uint8_t)v; G->p_resi[i] = (int16_t)(org[y * bs + x] - v);
      }
    }
  }
  /* forward transform; the coefficients go to RDOQ as sign * lLevelDouble in scan order */
  if (useTS) { FCU_FOR_LANES { est_build(cab, lane); for (int i = lane; i < n2; i += 64) { const int sp = iscan[i]; const int32_t ld = level_double((int32_t)G->p_resi[i] << (15 - 8 - log2), qscale, qbits); G->p_lscan[sp] = ld; if (level_nonzero(ld, qbits)) FCU_ATOMIC_MAX(&g_S.t_last, sp); } } }
  else {
    FCU_FOR_LANES { by_log2(log2, [&](auto L) { constexpr int LG = decltype(L)::value; RowCache<(1 << LG), int16_t> rc; for (int i = lane; i < n2; i += 64) G->p_tmp[i] = fwd1<LG>(rc, G->p_resi, useDst, i); }); }
    FCU_FOR_LANES { est_build(cab, lane); by_log2(log2, [&](auto L) { constexpr int LG = decltype(L)::value; RowCache<(1 << LG), int32_t> rc; for (int i = lane; i < n2; i += 64) { const int sp = iscan[i]; const int32_t ld = level_double(fwd2<LG>(rc, G->p_tmp, useDst, i), qscale, qbits); G->p_lscan[sp] = ld; if (level_nonzero(ld, qbits)) FCU_ATOMIC_MAX(&g_S.t_last, sp); } }); }
  }
  FCU_PTOC(E, tp_, FCU_PIX_SLOT(2, log2));
  {
    FCU_TIC(t8_);
    const int cbfCtx = comp ? (CTX_CBF_CHROMA + tu.tr_depth) : (CTX_CBF_LUMA + (tu.tr_depth == 0 ? 1 : 0));
    const int useRdoq = FCU_UNI((int)(useTS ? P.rdoq_ts : P.rdoq));
    if (useRdoq) rdoq_wave(cab, G->p_lscan, G->p_qscan, FCU_UNI(g_S.t_last), log2, comp, scanType, cbfCtx, P, G->r_rec, G->r_cg);
    FCU_FOR_LANES {
      if (comp == 0) for (int i = lane; i < tu.nparts; i += 64) cu->tr_idx[part + i] = (uint8_t)tu.tr_depth;   /* setTrIdxSubParts */
      if (lane == 0) {
        if (useRdoq) { g_S.t_abs = g_S.rw_abs; g_S.t_lsp = g_S.rw_lsp; }
        else { const RdoqOut o = quant_plain(G->p_lscan, G->p_qscan, 1, g_S.t_last, log2, comp, P); g_S.t_abs = o.abs_sum; g_S.t_lsp = o.last; }
        E.C->n_tu_trials++;
        FCU_COUNT(E, 15, (1ull << 40) + (unsigned long long)(g_S.t_last >= 0 ? ((g_S.t_last >> 4) + 1) * 16 : 0));   /* calls : coefficient iterations */
      }
    }
    FCU_TOC(E, t8_, 8);
  }
  FCU_PRST(tp_);                                             /* (the quantiser has its own section) */
  const int absSum = g_S.t_abs;
  FCU_SMALL_COUNT(SMALL_ALL_ZERO, log2 <= 3 && absSum == 0); FCU_SMALL_COUNT(SMALL_CHROMA_4X4, comp != 0 && log2 == 2);
  FCU_FOR_LANES {                                            /* setCbfPartRange + coefficient store */
    const int np = comp ? tu_nparts_c(tu) : tu.nparts;
    for (int i = lane; i < np; i += 64) cu->cbf[comp][part + i] = (uint8_t)((absSum > 0 ? 1 : 0) << tu.tr_depth);
    const int cgEnd = ((g_S.t_last >> 4) + 1) << 4;                /* RDOQ wrote the levels of scan positions < cgEnd */
    const DeqParams dq = deq_params(log2, qp);
    for (int i = lane; i < n2; i += 64) { const int sp = iscan[i]; const int q = (absSum > 0 && sp < cgEnd) ? G->p_qscan[sp] : 0; coef[sp] = (int16_t)q; G->p_tmp[useTS ? i : tr_index(i, log2)] = dequant1(q, dq); }
  }
  if (absSum > 0) {
    if (useTS) { FCU_FOR_LANES { const int s = 15 - 8 - log2; for (int i = lane; i < n2; i += 64) G->p_resi[i] = (int16_t)((G->p_tmp[i] + (1 << (s - 1))) >> s); } }
    else {
      FCU_FOR_LANES { by_log2(log2, [&](auto L) { constexpr int LG = decltype(L)::value; RowCache<(1 << LG), int32_t> rc; for (int i = lane; i < n2; i += 64) G->p_tcoef[i] = inv1<LG>(rc, G->p_tmp, useDst, i); }); }
      FCU_FOR_LANES { by_log2(log2, [&](auto L) { for (int i = lane; i < n2; i += 64) G->p_resi[i] = (int16_t)inv2<decltype(L)::value>(G->p_tcoef, useDst, i); }); }
    }
  }
  FCU_FOR_LANES {
    if (lane == 0) g_S.sad[35] = 0;
  }
  FCU_FOR_LANES {
    uint32_t sse = 0;
    for (int i = lane; i < n2; i += 64) {
      const int y = i >> log2, x = i & (N - 1);
      const int r = clip8(pred[y * bs + x] + (absSum > 0 ? G->p_resi[i] : 0));
      pred[y * bs + x] = (uint8_t)r; recqt[y * bs + x] = (uint8_t)r; recpic[y * rs + x] = (uint8_t)r;
      const int e = org[y * bs + x] - r; sse += (uint32_t)(e * e);
    }
    FCU_WAVE_ADD(&g_S.sad[35], sse);
  }
  FCU_SERIAL { const uint32_t sse = g_S.sad[35]; g_S.t_dist = comp ? (uint32_t)(P.chroma_weight * (double)sse) : sse; }
  FCU_PTOC(E, tp_, FCU_PIX_SLOT(3, log2));
  FCU_TOC(E, t11_, 11);
}

/* xStoreIntraResultQT / xLoadIntraResultQT, TEncSearch.cpp:1760-1850 */
FCU_DEV FCU_NOINLINE void store_intra_result_qt(uint32_t tu_k, int comp)
{
  const Env E = env_get(); const TU tu = tu_of_key(FCU_UNI(tu_k)); comp = FCU_UNI(comp);
  Scratch *G = E.G;
  if (comp && tu.cw == 0) return;
  const int N = comp ? tu.cw : (1 << tu.log2), layer = LOG2_MAXTU - tu.log2, bs = comp ? 32 : 64, bx = comp ? tu.cx : tu.x, by = comp ? tu.cy : tu.y;
  const int16_t *src = G->qt_coef[comp][layer] + (comp ? tu.off_c : tu.off_y);
  const uint8_t *s = yuv_plane(&G->qt_rec[layer], comp) + by * bs + bx; uint8_t *t = yuv_plane(&G->ts_rec, comp) + by * bs + bx;
  FCU_FOR_LANES { for (int i = lane; i < N * N; i += 64) { G->ts_coef[comp][i] = src[i]; t[(i / N) * bs + (i % N)] = s[(i / N) * bs + (i % N)]; } }
}
FCU_DEV FCU_NOINLINE void load_intra_result_qt(const CuObj *cu, uint32_t tu_k, int comp)
{
  const Env E = env_get(); cu = FCU_UNI(cu); const TU tu = tu_of_key(FCU_UNI(tu_k)); comp = FCU_UNI(comp);
  Scratch *G = E.G;
  if (comp && tu.cw == 0) return;
  const int N = comp ? tu.cw : (1 << tu.log2), layer = LOG2_MAXTU - tu.log2, bs = comp ? 32 : 64, sh = comp ? 1 : 0, bx = comp ? tu.cx : tu.x, by = comp ? tu.cy : tu.y;
  int16_t *dst = G->qt_coef[comp][layer] + (comp ? tu.off_c : tu.off_y);
  uint8_t *t = yuv_plane(&G->qt_rec[layer], comp) + by * bs + bx; const uint8_t *s = yuv_plane(&G->ts_rec, comp) + by * bs + bx;
  uint8_t *pic = E.C->rec[comp] + ((cu->y >> sh) + by) * E.C->stride[comp] + (cu->x >> sh) + bx; const int rs = E.C->stride[comp];
  FCU_FOR_LANES { for (int i = lane; i < N * N; i += 64) { dst[i] = G->ts_coef[comp][i]; const uint8_t v = s[(i / N) * bs + (i % N)]; t[(i / N) * bs + (i % N)] = v; pic[(i / N) * rs + (i % N)] = v; } }
}

/* ======================================================================================== */
/* xRecurIntraCodingLumaQT (sequential path), TEncSearch.cpp:1393-1713                        */
/* LEVEL = recursion level (compile-time unrolled, <= 3).  Adds to g_S.q_dist/q_cost[LEVEL].   */
/* ======================================================================================== */
template <int LEVEL>
FCU_DEV FCU_NOINLINE void recur_luma_qt(CuObj *cu, uint32_t tu_k, int checkFirst, int reuseVc = -1)
{
  const Env E = env_get(); cu = FCU_UNI(cu); const TU tu = tu_of_key(FCU_UNI(tu_k)); checkFirst = FCU_UNI(checkFirst); reuseVc = FCU_UNI(reuseVc);
  Scratch *G = E.G; const Params &P = E.C->p;
  const int d = FCU_UNI((int)cu->depth_cu), part = tu.part, trDepth = tu.tr_depth, fullDepth = d + trDepth, log2 = tu.log2;
  const int partSize = FCU_UNI((int)cu->part_size[part]);
  const int checkFull = log2 <= LOG2_MAXTU;
  int checkSplit = log2 > min_tu_log2_in_cu(d, partSize);
  if (checkFirst && checkFull) checkSplit = 0;
  int checkTS = P.transform_skip && log2 == 2;
  if (P.ts_fast) checkTS = checkTS && (partSize == SIZE_NxN);
  double singleCost = FCU_MAX_DOUBLE; uint32_t singleDist = 0, singleCbf = 0, singleBins = 0; int bestModeId = 0; uint64_t singleFrac = 0;

  if (checkFull) {
    if (checkTS) {
      FCU_FOR_LANES cab_copy(slot_ptr(E, fullDepth, CI_QT_TRAFO_ROOT), &g_S.cab[CAB_GOON], lane);
      for (int modeId = 0; modeId < 2; modeId++) {
        FCU_FOR_LANES { for (int i = lane; i < tu.nparts; i += 64) cu->tskip[0][part + i] = (uint8_t)modeId; }
        tu_trial(cu, tu_key(tu), 0, (CAB_GOON), modeId == 0 ? 1 : 2);
        const uint32_t tmpDist = FCU_UNI(g_S.t_dist), tmpCbf = FCU_UNI((uint32_t)((cu->cbf[0][part] >> trDepth) & 1));
        double tmpCost;
        if (modeId == 1 && tmpCbf == 0) tmpCost = FCU_MAX_DOUBLE;
        else {
          { FCU_TIC(t12_); FCU_SERIAL { const uint64_t f0 = g_S.cab[CAB_GOON].frac & 32767; g_S.vc_bits[0] = leaf_luma_bits(CAB_GOON, cu, tu_key(tu)); g_S.t_frac = g_S.cab[CAB_GOON].frac - f0; g_S.t_bins = g_S.cab[CAB_GOON].bins; } FCU_TOC(E, t12_, 12); }
          tmpCost = FCU_UNI(rd_cost(P, g_S.vc_bits[0], tmpDist));
        }
        if (tmpCost < singleCost) {
          singleCost = tmpCost; singleDist = tmpDist; singleCbf = tmpCbf; bestModeId = modeId; singleFrac = FCU_UNI(g_S.t_frac); singleBins = FCU_UNI(g_S.t_bins);
          if (bestModeId == 0) { store_intra_result_qt(tu_key(tu), 0); FCU_FOR_LANES cab_copy(slot_ptr(E, fullDepth, CI_TEMP_BEST), &g_S.cab[CAB_GOON], lane); }
        }
        if (modeId == 0) FCU_FOR_LANES cab_copy(&g_S.cab[CAB_GOON], slot_ptr(E, fullDepth, CI_QT_TRAFO_ROOT), lane);
      }
      FCU_SMALL_COUNT(SMALL_TS_WINNER, bestModeId == 1);
      FCU_FOR_LANES { for (int i = lane; i < tu.nparts; i += 64) cu->tskip[0][part + i] = (uint8_t)bestModeId; }
      if (bestModeId == 0) {
        load_intra_result_qt(cu, tu_key(tu), 0);
        FCU_FOR_LANES { for (int i = lane; i < tu.nparts; i += 64) cu->cbf[0][part + i] = (uint8_t)(singleCbf << trDepth); cab_copy(&g_S.cab[CAB_GOON], slot_ptr(E, fullDepth, CI_TEMP_BEST), lane); }
      }
    } else {
      if (checkSplit) FCU_FOR_LANES cab_copy(slot_ptr(E, fullDepth, CI_QT_TRAFO_ROOT), &g_S.cab[CAB_GOON], lane);
      FCU_FOR_LANES { for (int i = lane; i < tu.nparts; i += 64) cu->tskip[0][part + i] = 0; }
      if (reuseVc >= 0) {
        /* the un-split trial of the re-run (TEncSearch.cpp:2518-2586) repeats the first-pass trial of the same mode
         * from the same snapshot: take its levels, reconstruction, distortion, bits and coder state instead of
         * recomputing them (the candidate pools still hold them) */
        const int bv = reuseVc, N = 1 << log2, n2 = N * N, layer = LOG2_MAXTU - log2, cbf = FCU_UNI((int)(g_S.vc_abs[bv] > 0));
        FCU_SERIAL { const Cabac *w = &g_S.cab[CAB_LANE0 + g_S.vc_slot[bv]]; g_S.t_frac = w->frac - (g_S.cab[CAB_GOON].frac & 32767); g_S.t_bins = w->bins; }   /* the lane coder started from this snapshot */
        singleFrac = FCU_UNI(g_S.t_frac); singleBins = FCU_UNI(g_S.t_bins);
        FCU_FOR_LANES {
          for (int i = lane; i < n2; i += 64) {
            G->qt_coef[0][layer][tu.off_y + i] = (cbf && (i >> 4) <= (g_S.vc_last[bv] >> 4)) ? G->p_qscan[i * g_S.pu_nvc + bv] : (int16_t)0;
            G->qt_rec[layer].y[(tu.y + (i >> log2)) * 64 + tu.x + (i & (N - 1))] = G->p_rec[bv * n2 + i];
          }
          for (int i = lane; i < tu.nparts; i += 64) { cu->tr_idx[part + i] = (uint8_t)trDepth; cu->cbf[0][part + i] = (uint8_t)(cbf << trDepth); }
          cab_copy(&g_S.cab[CAB_GOON], &g_S.cab[CAB_LANE0 + g_S.vc_slot[bv]], lane);
        }
        singleDist = FCU_UNI(g_S.vc_dist[bv]); singleCbf = (uint32_t)cbf; singleCost = FCU_UNI(g_S.vc_cost[bv]);
      } else if (reuseVc <= -2) {
        /* 32x32 TU k of a 64x64 PU whose earlier TUs all kept the first pass's un-split result: coder and neighbourhood
         * are what they were in the first pass (pu_first_pass_64), so this trial would reproduce that pass's TU k of the
         * winning candidate -- levels, reconstruction, distortion, bits and coder state are taken from there */
        const int k = -2 - reuseVc, bv = FCU_UNI(g_S.pu_best_vc), N = 1 << log2, n2 = N * N, layer = LOG2_MAXTU - log2, cbf = FCU_UNI((int)g_S.c64_cbf[bv][k]);
        FCU_SERIAL {
          const uint64_t fprev = k ? G->c64_state[bv][k - 1].frac : (slot_ptr(E, d, CI_CURR_BEST)->frac & 32767);
          g_S.t_frac = G->c64_state[bv][k].frac - fprev;
          g_S.t_bins = G->c64_state[bv][k].bins - (k ? G->c64_state[bv][k - 1].bins : 0u);
          g_S.vc_bits[0] = (uint32_t)(((fprev & 32767) + g_S.t_frac) >> 15);
          g_S.t_dist = G->c64_distk[bv][k];
        }
        singleFrac = FCU_UNI(g_S.t_frac); singleBins = FCU_UNI(g_S.t_bins);
        FCU_FOR_LANES {
          for (int i = lane; i < n2; i += 64) {
            G->qt_coef[0][layer][tu.off_y + i] = G->c64_coef[bv][tu.off_y + i];
            const int o = (tu.y + (i >> log2)) * 64 + tu.x + (i & (N - 1));
            G->qt_rec[layer].y[o] = G->c64_rec[bv][o];
          }
          for (int i = lane; i < tu.nparts; i += 64) { cu->tr_idx[part + i] = (uint8_t)trDepth; cu->cbf[0][part + i] = (uint8_t)(cbf << trDepth); }
          cab_copy(&g_S.cab[CAB_GOON], &G->c64_state[bv][k], lane);
        }
        FCU_SERIAL { g_S.cab[CAB_GOON].frac = (g_S.cab[CAB_GOON].frac & 32767) + ((uint64_t)g_S.vc_bits[0] << 15); }
        singleDist = FCU_UNI(g_S.t_dist); singleCbf = (uint32_t)cbf;
        singleCost = FCU_UNI(rd_cost(P, g_S.vc_bits[0], singleDist));
      } else {
        tu_trial(cu, tu_key(tu), 0, (CAB_GOON), 0);
        singleDist = FCU_UNI(g_S.t_dist);
        if (checkSplit) singleCbf = FCU_UNI((uint32_t)((cu->cbf[0][part] >> trDepth) & 1));
        { FCU_TIC(t12_); FCU_SERIAL { const uint64_t f0 = g_S.cab[CAB_GOON].frac & 32767; g_S.vc_bits[0] = leaf_luma_bits(CAB_GOON, cu, tu_key(tu)); g_S.t_frac = g_S.cab[CAB_GOON].frac - f0; g_S.t_bins = g_S.cab[CAB_GOON].bins; } FCU_TOC(E, t12_, 12); }
        singleFrac = FCU_UNI(g_S.t_frac); singleBins = FCU_UNI(g_S.t_bins);
        singleCost = FCU_UNI(rd_cost(P, g_S.vc_bits[0], singleDist));
      }
    }
  }
  if (checkSplit) {
    if constexpr (LEVEL < 3) {
      if (checkFull) { FCU_FOR_LANES { cab_copy(slot_ptr(E, fullDepth, CI_QT_TRAFO_TEST), &g_S.cab[CAB_GOON], lane); } FCU_FOR_LANES { cab_copy(&g_S.cab[CAB_GOON], slot_ptr(E, fullDepth, CI_QT_TRAFO_ROOT), lane); } }
      else FCU_FOR_LANES cab_copy(slot_ptr(E, fullDepth, CI_QT_TRAFO_ROOT), &g_S.cab[CAB_GOON], lane);
      FCU_SERIAL { g_S.q_dist[LEVEL + 1] = 0; g_S.q_cost[LEVEL + 1] = 0; g_S.q_frac[LEVEL + 1] = 0; g_S.q_bins[LEVEL + 1] = 0; }
      uint32_t splitCbf = 0;
      int chainOk = LEVEL == 0 && log2 == 6 && !checkFirst && FCU_UNI(g_S.c64_valid);   /* see the reuse branch above */
      for (int i = 0; i < 4; i++) {
        TU c; tu_child(c, tu, i, 0);
        recur_luma_qt<LEVEL + 1>(cu, tu_key(c), checkFirst, chainOk ? -2 - i : -1);
        splitCbf |= FCU_UNI((uint32_t)((cu->cbf[0][c.part] >> c.tr_depth) & 1));
        chainOk = chainOk && FCU_UNI((int)cu->tr_idx[c.part]) == c.tr_depth;
      }
      const uint32_t splitDist = FCU_UNI(g_S.q_dist[LEVEL + 1]);
      /* uiSplitBits = xGetIntraBitsQT of the whole split subtree from QT_TRAFO_ROOT (TEncSearch.cpp:1600-1606).  Every bin
       * of that walk has already been counted, from the same state of its context, by the walks of the children's chosen
       * encodings (child 0 starts from this node's root state and, when this node begins the CU, also carries the
       * part-size / luma-mode bins; the subdivision and cbf contexts are indexed by TU size / depth), so the exact Q15
       * count is this node's own subdivision flag plus the children's counts, and the coder after the last child is
       * the coder after the walk.  The bins add up the same way.  Not for the NxN root, whose walk leaves out the luma
       * modes its children count. */
      const int sumBits = !(partSize == SIZE_NxN && trDepth == 0);
      FCU_FOR_LANES {
        if (splitCbf) for (int o = lane; o < tu.nparts; o += 64) cu->cbf[0][part + o] |= (uint8_t)(1 << trDepth);
        if (!sumBits) cab_copy(&g_S.cab[CAB_GOON], slot_ptr(E, fullDepth, CI_QT_TRAFO_ROOT), lane);
      }
      {
        FCU_TIC(t12_);
        FCU_SERIAL {
          const uint64_t f0 = slot_ptr(E, fullDepth, CI_QT_TRAFO_ROOT)->frac & 32767;
          if (sumBits) {
            g_S.cab[CAB_GOON].frac = f0; g_S.cab[CAB_GOON].bins = 0;
            if (log2 <= LOG2_MAXTU) cab_bin((CAB_GOON), 1, CTX_SUBDIV + 5 - log2);
            g_S.cab[CAB_GOON].frac += g_S.q_frac[LEVEL + 1]; g_S.cab[CAB_GOON].bins += g_S.q_bins[LEVEL + 1];
            g_S.vc_bits[0] = (uint32_t)(g_S.cab[CAB_GOON].frac >> 15);
          } else g_S.vc_bits[0] = intra_bits_qt((CAB_GOON), cu, tu_key(tu), 1, 0);
          g_S.t_frac = g_S.cab[CAB_GOON].frac - f0; g_S.t_bins = g_S.cab[CAB_GOON].bins;
        }
        FCU_TOC(E, t12_, 12);
      }
      const double splitCost = FCU_UNI(rd_cost(P, g_S.vc_bits[0], splitDist));
      if (splitCost < singleCost) { FCU_SERIAL { g_S.q_dist[LEVEL] += splitDist; g_S.q_cost[LEVEL] += splitCost; g_S.q_frac[LEVEL] += g_S.t_frac; g_S.q_bins[LEVEL] += g_S.t_bins; } return; }
      FCU_FOR_LANES {
        cab_copy(&g_S.cab[CAB_GOON], slot_ptr(E, fullDepth, CI_QT_TRAFO_TEST), lane);
        for (int i = lane; i < tu.nparts; i += 64) { cu->tr_idx[part + i] = (uint8_t)trDepth; cu->cbf[0][part + i] = (uint8_t)(singleCbf << trDepth); cu->tskip[0][part + i] = (uint8_t)bestModeId; }
        const int N = 1 << log2, layer = LOG2_MAXTU - log2;
        const uint8_t *s = G->qt_rec[layer].y + tu.y * 64 + tu.x;
        uint8_t *p = E.C->rec[0] + (cu->y + tu.y) * E.C->stride[0] + cu->x + tu.x; const int rs = E.C->stride[0];
        for (int i = lane; i < N * N; i += 64) p[(i >> log2) * rs + (i & (N - 1))] = s[(i >> log2) * 64 + (i & (N - 1))];
      }
    }
  }
  FCU_SERIAL { g_S.q_dist[LEVEL] += singleDist; g_S.q_cost[LEVEL] += singleCost; g_S.q_frac[LEVEL] += singleFrac; g_S.q_bins[LEVEL] += singleBins; }
}

/* xSetIntraResultLumaQT, TEncSearch.cpp:1717-1757 (iterative) */
FCU_DEV FCU_NOINLINE void set_intra_result_luma_qt(CuObj *cu, uint32_t root_k, Yuv *reco)
{
  const Env E = env_get(); cu = FCU_UNI(cu); const TU root = tu_of_key(FCU_UNI(root_k)); reco = FCU_UNI(reco);
  Scratch *G = E.G;
  TU *st = g_S.wk_st; int *ci = g_S.wk_ci; int sp = 0;
  st[0] = root; ci[0] = -1;
  while (sp >= 0) {
    const TU tu = st[sp];
    if (ci[sp] < 0) {
      if (cu->tr_idx[tu.part] == tu.tr_depth) {
        const int N = 1 << tu.log2, layer = LOG2_MAXTU - tu.log2;
        FCU_FOR_LANES {
          for (int i = lane; i < N * N; i += 64) {
            cu->coef[0][tu.off_y + i] = G->qt_coef[0][layer][tu.off_y + i];
            const int yy = tu.y + (i >> tu.log2), xx = tu.x + (i & (N - 1));
            reco->y[yy * 64 + xx] = G->qt_rec[layer].y[yy * 64 + xx];
          }
        }
        sp--; continue;
      }
      ci[sp] = 0;
    }
    if (ci[sp] >= 4) { sp--; continue; }
    { TU ch; tu_child(ch, st[sp], ci[sp], 0); ci[sp]++; sp++; st[sp] = ch; ci[sp] = -1; }
  }
}

/* ======================================================================================== */
/* RMD: 35 predictions + Hadamard SATD staged through LDS (TEncSearch.cpp:2300-2361,          */
/* TComRdCost.cpp:1343-1604) and the sorted candidate list (xUpdateCandList :5345-5370)       */
/* ======================================================================================== */
/* SATD of one USZ x USZ block of (source - prediction) for one mode (xCalcHADs8x8 / xCalcHADs4x4, TComRdCost.cpp:1343-1534).
 * Row by row: predict, row butterfly, then add the row into the USZ*USZ column-transform accumulators with the sign of the
 * Sylvester matrix (-1)^popcount(k & y); the sum of magnitudes does not depend on the order of the Hadamard outputs. */
template <int USZ>
FCU_DEV uint32_t satd_unit(const uint8_t *org, int log2, int mode, int dc, int bx, int by)
{
  const uint8_t *r = use_filtered_ref(mode, log2, 1) ? g_S.reff : g_S.ref;
  int acc[USZ * USZ];
#pragma unroll
  for (int i = 0; i < USZ * USZ; i++) acc[i] = 0;
  for (int y = 0; y < USZ; y++) {
    uint8_t o[USZ]; int row[USZ];
    __builtin_memcpy(o, org + (by + y) * 64 + bx, USZ);
#pragma unroll
    for (int x = 0; x < USZ; x++) row[x] = (int)o[x] - pred_pixel(r, log2, mode, 1, dc, bx + x, by + y);
#pragma unroll
    for (int len = 1; len < USZ; len <<= 1)
#pragma unroll
      for (int i = 0; i < USZ; i += 2 * len)
#pragma unroll
        for (int j = i; j < i + len; j++) { const int a = row[j], b = row[j + len]; row[j] = a + b; row[j + len] = a - b; }
#pragma unroll
    for (int k = 0; k < USZ; k++) {
      const int neg = -(__builtin_popcount((unsigned)(k & y)) & 1);          /* 0 or -1 */
#pragma unroll
      for (int j = 0; j < USZ; j++) acc[k * USZ + j] += (row[j] ^ neg) - neg;
    }
  }
  int s = 0;
#pragma unroll
  for (int i = 0; i < USZ * USZ; i++) s += iabs(acc[i]);
  return (uint32_t)(USZ == 8 ? ((s + 2) >> 2) : ((s + 1) >> 1));
}

/* Order in which the RMD deals the modes to the lanes: planar, DC and the two pure directions first, so that the wave
 * iterations after the first hold general angular modes only and pred_pixel's other branches are skipped by the whole wave. */
FCU_DEV int rmd_mode_of(int j) { return j < 2 ? j : j == 2 ? HOR : j == 3 ? VER : j < 12 ? j - 2 : j < 27 ? j - 1 : j; }

/* One line of the prediction of an N x N luma block, N <= 8: out[k] = pred_pixel(ref, LOG2, mode, 1, dc, X, Y) with
 * (X, Y) = (k, line) for planar, DC and the vertical modes 18..34 (a row), (line, k) for the horizontal modes 2..17 (a column).
 * Along such a line deltaPos, and with it the sample offset and the interpolation weight, are constants, and neighbouring
 * samples share a reference sample.  Same arithmetic as pred_pixel, which stays the definition (checked in the emulator). */
template <int LOG2>
FCU_DEV void pred_line(const uint8_t *ref, int mode, int dc, int line, int *out)
{
  constexpr int N = 1 << LOG2;
  static_assert(N <= 8, "edge filters of DC / pure directions assumed on (N <= 16)");
  const uint8_t *corner = ref + 2 * N;
  if (mode < 2) {
#pragma unroll
    for (int k = 0; k < N; k++) out[k] = pred_pixel(ref, LOG2, mode, 1, dc, k, line);
    return;
  }
  const int isVer = mode >= 18, ms = isVer ? 1 : -1;
  const int angMode = isVer ? mode - VER : -(mode - HOR), absAng = iabs(angMode);
  if (absAng == 0) {
#pragma unroll
    for (int k = 0; k < N; k++) out[k] = corner[ms * (k + 1)];
    out[0] = clip8(out[0] + ((corner[-ms * (line + 1)] - corner[0]) >> 1));
  } else {
    const int angAbs = (int)((0x2069544d245080ull >> (6 * absAng)) & 63);
    const int invAngle = (int)(((absAng <= 4 ? 0x13b0e38ccd000ull : 0x8004ec30c1e2ull) >> (13 * ((absAng - 1) & 3))) & 8191);
    const int angle = angMode < 0 ? -angAbs : angAbs;
    const int deltaPos = (line + 1) * angle, di = deltaPos >> 5, df = deltaPos & 31;
    int r[N + 1];
#pragma unroll
    for (int k = 0; k <= N; k++) {
      const int i = k + di + 1;
      r[k] = (k == N && !df) ? 0 : (i >= 0) ? corner[ms * i] : corner[-ms * ((128 + (-i) * invAngle) >> 8)];
    }
#pragma unroll
    for (int k = 0; k < N; k++) out[k] = df ? (((32 - df) * r[k] + df * r[k + 1] + 16) >> 5) : r[k];
  }
#ifdef FCU_EMU
  for (int k = 0; k < N; k++) FCU_CHECK(out[k] == pred_pixel(ref, LOG2, mode, 1, dc, isVer ? k : line, isVer ? line : k));
#endif
}

template <int N> FCU_DEV void hadamard_line(int *v)
{
#pragma unroll
  for (int len = 1; len < N; len <<= 1)
#pragma unroll
    for (int i = 0; i < N; i += 2 * len)
#pragma unroll
      for (int j = i; j < i + len; j++) { const int a = v[j], b = v[j + len]; v[j] = a + b; v[j + len] = a - b; }
}

/* RMD of an 8x8 or 4x4 PU (one Hadamard block per mode): the work item is (mode, line), 35 * N of them, 64 per wave iteration
 * (280 of 320 lane slots for 8x8, 140 of 192 for 4x4, against 35 of 64 with a whole block per lane).  A lane predicts its line
 * (pred_line), subtracts it from the source and transforms it; the lines of a block meet in the staging area, where lane
 * (block, k) transforms sample k of its N lines and adds the magnitudes into g_S.sad[mode] (the raw sum: the caller rounds).
 * Horizontal modes are dealt by columns: the transform is separable, so which direction runs first does not matter. */
template <int LOG2>
FCU_DEV void rmd_satd_small(const uint8_t *org)
{
  constexpr int N = 1 << LOG2, ITEMS = 35 * N;
  int16_t *stage = FCU_RMD_STAGE;
  for (int base = 0; base < ITEMS; base += 64) {
    FCU_FOR_LANES {
      const int it = base + lane;
      if (it < ITEMS) {
        const int mode = rmd_mode_of(it >> LOG2), line = it & (N - 1);
        int v[N];
        pred_line<LOG2>(use_filtered_ref(mode, LOG2, 1) ? g_S.reff : g_S.ref, mode, g_S.dc, line, v);
        if (mode >= 2 && mode < 18) {
#pragma unroll
          for (int k = 0; k < N; k++) v[k] = (int)org[k * 64 + line] - v[k];
        } else {
          uint8_t o[N];
          __builtin_memcpy(o, org + line * 64, N);
#pragma unroll
          for (int k = 0; k < N; k++) v[k] = (int)o[k] - v[k];
        }
        hadamard_line<N>(v);
#pragma unroll
        for (int k = 0; k < N; k++) stage[lane * N + k] = (int16_t)v[k];     /* |v| <= 8 * 255 */
      }
    }
    FCU_FOR_LANES {
      const int blk = lane >> LOG2, k = lane & (N - 1), it = base + blk * N;
      if (it < ITEMS) {
        int v[N];
#pragma unroll
        for (int l = 0; l < N; l++) v[l] = stage[(blk * N + l) * N + k];
        hadamard_line<N>(v);
        int sum = 0;
#pragma unroll
        for (int l = 0; l < N; l++) sum += iabs(v[l]);
        FCU_ATOMIC_ADD(&g_S.sad[rmd_mode_of(it >> LOG2)], (uint32_t)sum);
      }
    }
  }
}

FCU_DEV FCU_NOINLINE void rmd(CuObj *cu, uint32_t tu_k)
{
  const Env E = env_get(); cu = FCU_UNI(cu); const TU tu = tu_of_key(FCU_UNI(tu_k));
  Scratch *G = E.G; const Params &P = E.C->p;
  const int d = cu->depth_cu, N = 1 << tu.log2, log2 = tu.log2;
  { FCU_TIC(tm_); build_ref(0, cu->x + tu.x, cu->y + tu.y, log2, 1); FCU_MTOC(E, tm_, 11); }
  const uint8_t *org = G->org[d].y + tu.y * 64 + tu.x;
  FCU_TIC(tm1_);
  FCU_FOR_LANES {
    if (lane < 36) g_S.sad[lane] = 0;
    if (lane == 0) {                                       /* the most probable modes: neighbour CU data only */
      int preds[3];
      g_S.n_mpm = intra_dir_predictor(E, cu, tu.part, preds);
      g_S.preds[0] = preds[0]; g_S.preds[1] = preds[1]; g_S.preds[2] = preds[2];
      g_S.ref_tag = ref_key(cu->x + tu.x, cu->y + tu.y, log2);   /* the first pass of this PU takes the samples over */
    }
  }
  if (N >= 16) {
    /* one (mode, Hadamard block) unit per lane, entirely in registers; block index fastest, so that the lanes of an iteration
     * share the mode (64x64) or hold 4 / 16 modes of one class */
    FCU_FOR_LANES {
      const int dc = g_S.dc;
      const int bpr = N >> 3, nblk = bpr * bpr;
      for (int u = lane; u < 35 * nblk; u += 64) { const int j = u / nblk, blk = u - j * nblk, mode = rmd_mode_of(j); FCU_ATOMIC_ADD(&g_S.sad[mode], satd_unit<8>(org, log2, mode, dc, (blk % bpr) * 8, (blk / bpr) * 8)); }
    }
  } else if (N == 8) rmd_satd_small<3>(org);
  else rmd_satd_small<2>(org);
  FCU_MTOC(E, tm1_, 12);
  FCU_TIC(tm2_);
  /* Candidate list (xUpdateCandList): the insertion with a strict '<' is a stable sort by cost, so mode m ends up at position
   * #{m' : cost[m'] < cost[m]} + #{m' < m : cost[m'] == cost[m]}.  One lane per mode prices its mode, then ranks it against the
   * 35 costs; the first numRmd positions are the list. */
  const int numRmd = k_rd_mode_num[log2 - 2];
  double *cost35 = FCU_RMD_COST;
  FCU_FOR_LANES {
    if (lane < 35) {
      const int mode = lane;
      int predIdx = -1;
      for (int i = 0; i < 3; i++) if (mode == g_S.preds[i]) predIdx = i;
      const uint64_t carry = slot_ptr(E, d, CI_CURR_BEST)->frac & 32767;   /* loadIntraDirMode + resetBits, TEncSearch.cpp:5313-5340 */
      const uint64_t fr = carry + (uint64_t)ctx_bits(CAB_CUR0 + d, CTX_INTRA_LUMA, predIdx != -1) + (uint64_t)32768 * (uint64_t)(predIdx != -1 ? (predIdx ? 2 : 1) : 5);
      const uint32_t modeBits = (uint32_t)(fr >> 15);
      uint32_t sad = g_S.sad[mode];
      if (N == 8) sad = (sad + 2) >> 2; else if (N == 4) sad = (sad + 1) >> 1;   /* xCalcHADs8x8 / xCalcHADs4x4 round the block's sum */
      cost35[mode] = (double)sad + (double)modeBits * P.sqrt_lambda;
    }
  }
  FCU_FOR_LANES {
    if (lane < 35) {
      const double c = cost35[lane];
      int rank = 0;
      for (int m = 0; m < 35; m++) { const double o = cost35[m]; rank += (o < c || (o == c && m < lane)) ? 1 : 0; }
      if (rank < numRmd) { g_S.rd_mode[rank] = lane; g_S.cand_cost[rank] = c; }
    }
  }
  FCU_SERIAL {
    int numFull = numRmd;
    const int nm = g_S.n_mpm;
    for (int j = 0; j < nm; j++) {
      int inc = 0;
      for (int i = 0; i < numFull; i++) inc |= (g_S.preds[j] == g_S.rd_mode[i]);
      if (!inc) g_S.rd_mode[numFull++] = g_S.preds[j];
    }
    g_S.n_rd = numFull;
  }
  FCU_MTOC(E, tm2_, 13);
}

/* ======================================================================================== */
/* first-pass RDO of one PU whose TU is not split: all candidates (x transform-skip variants) */
/* side by side -- pixel phases on all lanes, RDOQ + bit counting one candidate per lane.     */
/* Restates the loop TEncSearch.cpp:2447-2516 for the bCheckFirst case (:1428-1444).          */
/* ======================================================================================== */
FCU_DEV FCU_NOINLINE void pu_first_pass_batched(CuObj *cu, uint32_t tu_k)
{
  const Env E = env_get(); cu = FCU_UNI(cu); const TU tu = tu_of_key(FCU_UNI(tu_k));
  Scratch *G = E.G; const Params &P = E.C->p;
  const int d = cu->depth_cu, N = 1 << tu.log2, log2 = tu.log2, n2 = N * N, part = tu.part;
  const int partSize = cu->part_size[part];
  int checkTS = P.transform_skip && log2 == 2;
  if (P.ts_fast) checkTS = checkTS && (partSize == SIZE_NxN);
  const int nc = g_S.n_rd, tsv = checkTS ? 2 : 1, tss = tsv - 1, nvc = nc * tsv;   /* v / tsv == v >> tss, v % tsv == v & tss */
  FCU_CHECK(nvc <= MAXVC && nvc * n2 <= POOL && (MAXLC % 2) == 0);
  FCU_SMALL_COUNT(SMALL_BATCH_OVER_16, log2 == 2 && nvc > 16);
  const int qbits = rdoq_qbits(log2, P.qp), qscale = k_quant_scales[P.qp % 6];
  const int useDst = log2 == 2;
  const uint8_t *org = G->org[d].y + tu.y * 64 + tu.x;
  /* reference samples are shared by all candidates: the TU is the whole PU */
  /* ... and rmd() has just built them for this very block, unless the caller came another way (the tag says) */
  const int haveRefs = FCU_UNI(g_S.ref_tag) == ref_key(cu->x + tu.x, cu->y + tu.y, log2);
  if (!haveRefs) { FCU_TIC(tm_); build_ref(0, cu->x + tu.x, cu->y + tu.y, log2, 1); FCU_MTOC(E, tm_, 14); }
  FCU_PTIC(tp_);
  /* 4x4 / 8x8: a sample per lane and the stages in registers, four candidates or one per pass of the wave.  Only what a later
   * stage or another function reads goes to memory: the prediction (the reference samples die in the quantiser), the
   * level_double values in scan order, the reconstruction. */
  const int regs = FCU_SMALL_TU_REGS(log2), blk_mask = ~(n2 - 1), l2n2 = 2 * log2;
  if (regs) {
    FCU_FOR_LANES_REG { if (lane == 0) g_S.ref_tag = -1; if (lane < nvc) g_S.vc_last[lane] = -1; }   /* (LDS accesses of one wave stay in program order) */
    for (int base = 0; base < nc * n2; base += 64) {
      LaneVar<int> vResi, vT1;
      FCU_FOR_LANES_REG {                                    /* prediction + residual */
        const int i = base + lane, act = i < nc * n2, cnd = act ? (i >> l2n2) : 0, p = i & (n2 - 1), y = p >> log2, x = p & (N - 1), mode = g_S.rd_mode[cnd];
        const uint8_t *r = use_filtered_ref(mode, log2, 1) ? g_S.reff : g_S.ref;
        const int v = pred_pixel(r, log2, mode, 1, g_S.dc, x, y);
        int res = 0;
        if (act) { G->p_pred[i] = (uint8_t)v; res = (int16_t)(org[y * 64 + x] - v); }
        vResi.set(lane, res);
      }
      FCU_FOR_LANES_REG { vT1.set(lane, log2 == 2 ? fwd1_lanes<2>(vResi, useDst, lane & blk_mask, lane & (n2 - 1)) : fwd1_lanes<3>(vResi, 0, lane & blk_mask, lane & (n2 - 1))); }
      FCU_FOR_LANES_REG {                                    /* second pass + level_double of the candidate's variants: slot v = cand*tsv + ts */
        const int i = base + lane, act = i < nc * n2, cnd = act ? (i >> l2n2) : 0, p = i & (n2 - 1);
        const int32_t t = log2 == 2 ? fwd2_lanes<2>(vT1, useDst, lane & blk_mask, p) : fwd2_lanes<3>(vT1, 0, lane & blk_mask, p);
        if (act) {
          const uint16_t *iscan = k_iscan + k_scan_off[coef_scan_idx(g_S.rd_mode[cnd], log2, 0) * 4 + log2 - 2];
          const int sp = iscan[p];
          for (int ts = 0; ts < tsv; ts++) {
            const int v = cnd * tsv + ts;
            const int32_t ld = level_double(ts ? ((int32_t)vResi.own(lane) << (15 - 8 - log2)) : t, qscale, qbits);
            G->p_lscan[sp * nvc + v] = ld;
            if (level_nonzero(ld, qbits)) FCU_ATOMIC_MAX(&g_S.vc_last[v], sp);
          }
        }
      }
    }
    FCU_FOR_LANES { est_build(CAB_CUR0 + d, lane); }
  } else {
  FCU_FOR_LANES {                                            /* prediction + residual per candidate */
    if (lane == 0) g_S.ref_tag = -1;                         /* consumed: the quantisation below reuses the arrays */
    const int dc = g_S.dc;
    for (int i = lane; i < nc * n2; i += 64) {
      const int cnd = i / n2, p = i - cnd * n2, y = p >> log2, x = p & (N - 1), mode = g_S.rd_mode[cnd];
      const uint8_t *r = use_filtered_ref(mode, log2, 1) ? g_S.reff : g_S.ref;
      const int v = pred_pixel(r, log2, mode, 1, dc, x, y);
      G->p_pred[i] = (uint8_t)v; G->p_resi[i] = (int16_t)(org[y * 64 + x] - v);
    }
  }
  FCU_FOR_LANES { if (lane < nvc) g_S.vc_last[lane] = -1; by_log2(log2, [&](auto L) { constexpr int LG = decltype(L)::value; RowCache<(1 << LG), int16_t> rc; for (int i = lane; i < nc * n2; i += 64) { const int cnd = i / n2; G->p_tmp[i] = fwd1<LG>(rc, G->p_resi + cnd * n2, useDst, i - cnd * n2); } }); }
  FCU_FOR_LANES {                                            /* slot v = cand*tsv + ts */
    est_build(CAB_CUR0 + d, lane);
    by_log2(log2, [&](auto L) { constexpr int LG = decltype(L)::value; RowCache<(1 << LG), int32_t> rc;
      for (int i = lane; i < nvc * n2; i += 64) {
        const int v = i / n2, p = i - v * n2, cnd = (v >> tss), ts = (v & tss);
        const uint16_t *iscan = k_iscan + k_scan_off[coef_scan_idx(g_S.rd_mode[cnd], log2, 0) * 4 + log2 - 2];
        const int32_t t = ts ? ((int32_t)G->p_resi[cnd * n2 + p] << (15 - 8 - log2)) : fwd2<LG>(rc, G->p_tmp + cnd * n2, useDst, p);
        const int sp = iscan[p]; const int32_t ld = level_double(t, qscale, qbits);
        G->p_lscan[sp * nvc + v] = ld;
        if (level_nonzero(ld, qbits)) FCU_ATOMIC_MAX(&g_S.vc_last[v], sp);
      }
    });
  }
  }
  FCU_PTOC(E, tp_, FCU_PIX_SLOT(0, log2));
  FCU_TIC(t2_);
  FCU_FOR_LANES {                                            /* RDOQ: one virtual candidate per lane */
    if (lane < nvc) {
      const int mode = g_S.rd_mode[(lane >> tss)];
      RdoqRec *rrec = G->r_rec + lane; double *rcg = G->r_cg + lane;
      const int cbfCtx = CTX_CBF_LUMA + (tu.tr_depth == 0 ? 1 : 0);
      const RdoqOut o = ((lane & tss) ? P.rdoq_ts : P.rdoq) ? rdoq<1>(CAB_CUR0 + d, G->p_lscan + lane, G->p_qscan + lane, nvc, g_S.vc_last[lane], log2, 0, coef_scan_idx(mode, log2, 0), cbfCtx, P, rrec, rcg, lane)
                                                            : quant_plain(G->p_lscan + lane, G->p_qscan + lane, nvc, g_S.vc_last[lane], log2, 0, P);
      g_S.vc_abs[lane] = o.abs_sum; g_S.vc_lsp[lane] = o.last;
      g_S.vc_dist[lane] = 0;
    }
    if (lane == 0) E.C->n_tu_trials += (unsigned long long)nvc;
  }
  FCU_TOC(E, t2_, 2);
  FCU_PRST(tp_);
  if (regs) {
    const DeqParams dq = deq_params(log2, P.qp);
    for (int base = 0; base < nvc * n2; base += 64) {        /* four 4x4 variants or one 8x8 variant per pass */
      const int skip = n2 == 64 && FCU_UNI(g_S.vc_abs[base >> 6]) == 0;   /* an 8x8 variant without levels: its residual is 0 */
      LaneVar<int> vDeq, vT2, vPO;
      FCU_FOR_LANES_REG {                                    /* level in raster order + dequantisation; prediction and source sample in the same trip */
        const int i = base + lane, act = i < nvc * n2, v = act ? (i >> l2n2) : 0, p = i & (n2 - 1), cnd = (v >> tss);
        int dv = 0, po = 0;
        if (act) {
          const uint16_t *iscan = k_iscan + k_scan_off[coef_scan_idx(g_S.rd_mode[cnd], log2, 0) * 4 + log2 - 2];
          const int sp = iscan[p];
          const int q = (g_S.vc_abs[v] > 0 && (sp >> 4) <= (g_S.vc_last[v] >> 4)) ? G->p_qscan[sp * nvc + v] : 0;
          dv = dequant1(q, dq);
          po = G->p_pred[cnd * n2 + p] | (org[(p >> log2) * 64 + (p & (N - 1))] << 8);
        }
        vDeq.set(lane, dv); vPO.set(lane, po);
      }
      if (!skip) FCU_FOR_LANES_REG { vT2.set(lane, log2 == 2 ? inv1_lanes<2>(vDeq, useDst, lane & blk_mask, lane & (n2 - 1)) : inv1_lanes<3>(vDeq, 0, lane & blk_mask, lane & (n2 - 1))); }
      FCU_FOR_LANES_REG {                                    /* second inverse pass + reconstruction + SSE */
        const int i = base + lane, act = i < nvc * n2, v = act ? (i >> l2n2) : 0, p = i & (n2 - 1), ts = (v & tss);
        const int t = skip ? 0 : (log2 == 2 ? inv2_lanes<2>(vT2, useDst, lane & blk_mask, p) : inv2_lanes<3>(vT2, 0, lane & blk_mask, p));
        int e = 0;
        if (act) {
          int res = 0;
          if (g_S.vc_abs[v] > 0) { const int s = 15 - 8 - log2; res = ts ? (int16_t)((vDeq.own(lane) + (1 << (s - 1))) >> s) : t; }
          const int po = vPO.own(lane), r = clip8((po & 255) + res);
          G->p_rec[i] = (uint8_t)r;
          e = (po >> 8) - r;
        }
        if (n2 == 64) FCU_WAVE_ADD(&g_S.vc_dist[base >> 6], (uint32_t)(e * e));
        else if (act) FCU_ATOMIC_ADD(&g_S.vc_dist[v], (uint32_t)(e * e));
      }
    }
    FCU_FOR_LANES { }                                        /* p_rec and vc_dist are complete before the bit count reads them */
  } else {
  FCU_FOR_LANES {                                            /* levels back to raster order + dequantisation */
    const DeqParams dq = deq_params(log2, P.qp);
    for (int i = lane; i < nvc * n2; i += 64) {
      const int v = i / n2, p = i - v * n2;
      const uint16_t *iscan = k_iscan + k_scan_off[coef_scan_idx(g_S.rd_mode[(v >> tss)], log2, 0) * 4 + log2 - 2];
      const int sp = iscan[p];
      const int q = (g_S.vc_abs[v] > 0 && (sp >> 4) <= (g_S.vc_last[v] >> 4)) ? G->p_qscan[sp * nvc + v] : 0;
      G->p_tmp[((v & tss)) ? i : v * n2 + tr_index(p, log2)] = dequant1(q, dq);
    }
  }
  FCU_FOR_LANES {
    by_log2(log2, [&](auto L) { constexpr int LG = decltype(L)::value; RowCache<(1 << LG), int32_t> rc;
      for (int i = lane; i < nvc * n2; i += 64) {
        const int v = i / n2, p = i - v * n2, ts = (v & tss);
        if (ts) { const int s = 15 - 8 - log2; G->p_tcoef[i] = (G->p_tmp[i] + (1 << (s - 1))) >> s; }
        else G->p_tcoef[i] = inv1<LG>(rc, G->p_tmp + v * n2, useDst, p);
      }
    });
  }
  FCU_FOR_LANES {
    by_log2(log2, [&](auto L) {
      uint32_t acc = 0;
      for (int i = lane; i < nvc * n2; i += 64) {
        const int v = i / n2, p = i - v * n2, cnd = (v >> tss), ts = (v & tss), y = p >> log2, x = p & (N - 1);
        int res = 0;
        if (g_S.vc_abs[v] > 0) res = ts ? (int16_t)G->p_tcoef[i] : inv2<decltype(L)::value>(G->p_tcoef + v * n2, useDst, p);
        const int r = clip8(G->p_pred[cnd * n2 + p] + res);
        G->p_rec[i] = (uint8_t)r;
        const int e = org[y * 64 + x] - r;
        FCU_DIST_ADD(acc, v, e, i, n2);
      }
    });
  }
  }
  FCU_PTOC(E, tp_, FCU_PIX_SLOT(1, log2));
  FCU_TIC(t3_);
  /* Bits of (header, subdiv, cbf, coefficients): xGetIntraBitsQT, one variant per lane on MAXLC lane-private coders.
   * More than MAXLC variants (a 4x4 PU with 9-10 candidates x 2) take a second round; it reuses coder slots, but
   * never the one of the best variant so far: the re-run of the winner (recur_luma_qt) takes its coder state from there. */
  for (int vbase = 0; vbase < nvc; vbase += MAXLC) {
    const int slotBase = vbase ? (g_S.vc_slot[g_S.pu_best_vc] + 1) % MAXLC : 0;
#if defined(FCU_EMU) && defined(FCU_EMU_TRACE_ROUNDS)
    if (vbase) fprintf(stderr, "second bit-count round: %d variants\n", nvc);
#endif
    FCU_WALK_COUNT(WALK_BITS_SECOND_ROUND, vbase != 0);
    FCU_FOR_LANES {
      const int vc = vbase + lane;
      if (lane < MAXLC && vc < nvc) {
        const int cnd = (vc >> tss), ts = (vc & tss), mode = g_S.rd_mode[cnd], cbf = g_S.vc_abs[vc] > 0;
        const int slot = (slotBase + lane) % MAXLC;
        double cost;
        g_S.vc_slot[vc] = (uint8_t)slot;
        if (ts && !cbf) cost = FCU_MAX_DOUBLE;               /* TS with CBF 0 is forbidden, TEncSearch.cpp:1503-1507 */
        else {
          const int c = CAB_LANE0 + slot;
          cab_copy1(&g_S.cab[c], slot_ptr(E, d, CI_CURR_BEST));
          cab_reset_bits(c);
          if (part == 0 && P.slice_type != SLICE_I) { code_skip_flag(E, c, cu, 0); code_pred_mode(c, cu, 0); }
          if (part == 0 && d == MAXDEPTH) cab_bin(c, partSize == SIZE_2Nx2N, CTX_PARTSIZE);
          code_luma_dir_bits(c, mode, g_S.preds);
          if (!(partSize == SIZE_NxN && tu.tr_depth == 0) && log2 <= LOG2_MAXTU && log2 != LOG2_MINTU && log2 != min_tu_log2_in_cu(d, partSize))
            cab_bin(c, 0, CTX_SUBDIV + 5 - log2);
          cab_bin(c, cbf, CTX_CBF_LUMA + (tu.tr_depth == 0 ? 1 : 0));
          if (cbf) code_coeff_nxn<0>(c, G->p_qscan + vc, nvc, g_S.vc_lsp[vc], log2, 0, coef_scan_idx(mode, log2, 0), ts, P, g_S.lane_abs[slot]);
          g_S.vc_bits[vc] = cab_bits(c);
          cost = rd_cost(P, g_S.vc_bits[vc], g_S.vc_dist[vc]);
        }
        g_S.vc_cost[vc] = cost;
      }
    }
    FCU_SERIAL {                                             /* strict '<', earlier candidate wins ties; candidates coded so far */
      const int ncDone = ((vbase + MAXLC < nvc) ? vbase + MAXLC : nvc) / tsv;
      double best = FCU_MAX_DOUBLE; int bv = 0;
      for (int cnd = 0; cnd < ncDone; cnd++) {
        int v = cnd * tsv; double c = g_S.vc_cost[v];
        if (tsv == 2 && g_S.vc_cost[v + 1] < c) { v = v + 1; c = g_S.vc_cost[v]; }
        if (c < best) { best = c; bv = v; }
      }
      g_S.pu_nvc = nvc; g_S.pu_best_vc = bv; g_S.pu_best_cost = best; g_S.pu_best_dist = g_S.vc_dist[bv]; g_S.pu_best_mode = g_S.rd_mode[(bv >> tss)];
    }
  }
  FCU_TOC(E, t3_, 3);
  {                                                          /* xSetIntraResultLumaQT + decision snapshot */
    const int bv = g_S.pu_best_vc, ts = (bv & tss), cbf = g_S.vc_abs[bv] > 0;
    FCU_SMALL_COUNT(SMALL_TS_WINNER, ts); FCU_SMALL_COUNT(SMALL_ALL_ZERO, log2 <= 3 && !cbf);
    Yuv *reco = &G->reco[d][1 - g_S.reco_best_idx[d]];
    FCU_FOR_LANES {
      for (int i = lane; i < n2; i += 64) {
        cu->coef[0][tu.off_y + i] = (cbf && (i >> 4) <= (g_S.vc_last[bv] >> 4)) ? G->p_qscan[i * nvc + bv] : (int16_t)0;
        reco->y[(tu.y + (i >> log2)) * 64 + tu.x + (i & (N - 1))] = G->p_rec[bv * n2 + i];
      }
      for (int i = lane; i < tu.nparts; i += 64) { G->tmp_tr_idx[i] = (uint8_t)tu.tr_depth; G->tmp_cbf[i] = (uint8_t)(cbf << tu.tr_depth); G->tmp_tskip[i] = (uint8_t)ts; }
    }
  }
}

/* First pass of a 64x64 PU (TEncSearch.cpp:2440-2516, where xRecurIntraCodingLumaQT can only code it as four 32x32 TUs).
 * The candidates share the snapshot they start from and nothing else, so they advance side by side: for each of the four
 * TUs in turn, the prediction of every candidate from that candidate's own reconstruction of the earlier TUs (swapped
 * into the picture plane for build_ref), then one batched transform, RDOQ with one candidate per lane on its own running
 * coder, reconstruction and bit count.  A candidate's bits are the Q15 sum of its four TU walks (see recur_luma_qt). */
FCU_DEV FCU_NOINLINE void pu_first_pass_64(CuObj *cu, uint32_t root_k)
{
  const Env E = env_get(); cu = FCU_UNI(cu); const TU root = tu_of_key(FCU_UNI(root_k));
  Scratch *G = E.G; const Params &P = E.C->p;
  const int d = cu->depth_cu, nc = g_S.n_rd, log2 = 5, N = 32, n2 = N * N, partSize = cu->part_size[root.part];
  FCU_CHECK(nc <= 5 && nc * n2 <= POOL && root.log2 == 6);
  const int qbits = rdoq_qbits(log2, P.qp), qscale = k_quant_scales[P.qp % 6];
  uint8_t *recpic = E.C->rec[0] + cu->y * E.C->stride[0] + cu->x; const int rs = E.C->stride[0];
  FCU_FOR_LANES {
    if (lane < nc) { const int c = CAB_LANE0 + lane; cab_copy1(&g_S.cab[c], slot_ptr(E, d, CI_CURR_BEST)); cab_reset_bits(c); g_S.c64_dist[lane] = 0; }
  }
  for (int k = 0; k < 4; k++) {
    TU tu; tu_child(tu, root, k, 0);
    const uint8_t *org = G->org[d].y + tu.y * 64 + tu.x;
    for (int cand = 0; cand < nc; cand++) {
      const int mode = g_S.rd_mode[cand], filt = use_filtered_ref(mode, log2, 1);
      if (k) {
        FCU_FOR_LANES {                                      /* this candidate's earlier TUs become the neighbourhood */
          for (int i = lane; i < k * n2; i += 64) {
            const int j = i >> 10, q = i & (n2 - 1), yy = (j >> 1) * N + (q >> log2), xx = (j & 1) * N + (q & (N - 1));
            recpic[yy * rs + xx] = G->c64_rec[cand][yy * 64 + xx];
          }
        }
      }
      build_ref(0, cu->x + tu.x, cu->y + tu.y, log2, filt);
      FCU_FOR_LANES {
        const uint8_t *r = filt ? g_S.reff : g_S.ref; const int dc = g_S.dc;
        for (int i = lane; i < n2; i += 64) {
          const int y = i >> log2, x = i & (N - 1);
          const int v = pred_pixel(r, log2, mode, 1, dc, x, y);
          G->p_pred[cand * n2 + i] = (uint8_t)v; G->p_resi[cand * n2 + i] = (int16_t)(org[y * 64 + x] - v);
        }
      }
    }
    FCU_FOR_LANES { if (lane < nc) g_S.vc_last[lane] = -1; by_log2(log2, [&](auto L) { constexpr int LG = decltype(L)::value; RowCache<(1 << LG), int16_t> rc; for (int i = lane; i < nc * n2; i += 64) { const int cnd = i / n2; G->p_tmp[i] = fwd1<LG>(rc, G->p_resi + cnd * n2, 0, i - cnd * n2); } }); }
    FCU_FOR_LANES {
      by_log2(log2, [&](auto L) { constexpr int LG = decltype(L)::value; RowCache<(1 << LG), int32_t> rc;
        for (int i = lane; i < nc * n2; i += 64) {
          const int v = i / n2, p = i - v * n2;
          const uint16_t *iscan = k_iscan + k_scan_off[coef_scan_idx(g_S.rd_mode[v], log2, 0) * 4 + log2 - 2];
          const int32_t t = fwd2<LG>(rc, G->p_tmp + v * n2, 0, p);
          const int sp = iscan[p]; const int32_t ld = level_double(t, qscale, qbits);
          G->p_lscan[sp * nc + v] = ld;
          if (level_nonzero(ld, qbits)) FCU_ATOMIC_MAX(&g_S.vc_last[v], sp);
        }
      });
    }
    FCU_FOR_LANES {                                          /* RDOQ: one candidate per lane, priced against its own coder */
      if (lane < nc) {
        RdoqRec *rrec = G->r_rec + lane; double *rcg = G->r_cg + lane;
        const RdoqOut o = P.rdoq ? rdoq<0>(CAB_LANE0 + lane, G->p_lscan + lane, G->p_qscan + lane, nc, g_S.vc_last[lane], log2, 0,
                                              coef_scan_idx(g_S.rd_mode[lane], log2, 0), CTX_CBF_LUMA + (tu.tr_depth == 0 ? 1 : 0), P, rrec, rcg, lane)
                                 : quant_plain(G->p_lscan + lane, G->p_qscan + lane, nc, g_S.vc_last[lane], log2, 0, P);
        g_S.vc_abs[lane] = o.abs_sum; g_S.vc_lsp[lane] = o.last; g_S.vc_dist[lane] = 0;
      }
      if (lane == 0) E.C->n_tu_trials += (unsigned long long)nc;
    }
    FCU_FOR_LANES {                                          /* levels kept per candidate (scan order) + dequantisation */
      const DeqParams dq = deq_params(log2, P.qp);
      for (int i = lane; i < nc * n2; i += 64) {
        const int v = i / n2, p = i - v * n2;
        const uint16_t *iscan = k_iscan + k_scan_off[coef_scan_idx(g_S.rd_mode[v], log2, 0) * 4 + log2 - 2];
        const int sp = iscan[p];
        const int q = (g_S.vc_abs[v] > 0 && (sp >> 4) <= (g_S.vc_last[v] >> 4)) ? G->p_qscan[sp * nc + v] : 0;
        G->c64_coef[v][tu.off_y + sp] = (int16_t)q;
        G->p_tmp[v * n2 + tr_index(p, log2)] = dequant1(q, dq);
      }
    }
    FCU_FOR_LANES { by_log2(log2, [&](auto L) { constexpr int LG = decltype(L)::value; RowCache<(1 << LG), int32_t> rc; for (int i = lane; i < nc * n2; i += 64) { const int v = i / n2; G->p_tcoef[i] = inv1<LG>(rc, G->p_tmp + v * n2, 0, i - v * n2); } }); }
    FCU_FOR_LANES {
      by_log2(log2, [&](auto L) {
        uint32_t acc = 0;
        for (int i = lane; i < nc * n2; i += 64) {
          const int v = i / n2, p = i - v * n2, y = p >> log2, x = p & (N - 1);
          const int res = g_S.vc_abs[v] > 0 ? inv2<decltype(L)::value>(G->p_tcoef + v * n2, 0, p) : 0;
          const int r = clip8(G->p_pred[i] + res);
          G->c64_rec[v][(tu.y + y) * 64 + tu.x + x] = (uint8_t)r;
          const int e = org[y * 64 + x] - r;
          FCU_DIST_ADD(acc, v, e, i, n2);
        }
      });
    }
    FCU_FOR_LANES {                                          /* the TU's walk (leaf_luma_bits) on the candidate's running coder */
      if (lane < nc) {
        const int c = CAB_LANE0 + lane, mode = g_S.rd_mode[lane], cbf = g_S.vc_abs[lane] > 0;
        if (tu.part == 0 && P.slice_type != SLICE_I) { code_skip_flag(E, c, cu, 0); code_pred_mode(c, cu, 0); }
        if (tu.part == 0 && d == MAXDEPTH) cab_bin(c, partSize == SIZE_2Nx2N, CTX_PARTSIZE);
        if (tu.part == 0) code_luma_dir_bits(c, mode, g_S.preds);
        if (log2 != LOG2_MINTU && log2 != min_tu_log2_in_cu(d, partSize)) cab_bin(c, 0, CTX_SUBDIV + 5 - log2);
        cab_bin(c, cbf, CTX_CBF_LUMA + (tu.tr_depth == 0 ? 1 : 0));
        if (cbf) code_coeff_nxn<0>(c, G->p_qscan + lane, nc, g_S.vc_lsp[lane], log2, 0, coef_scan_idx(mode, log2, 0), 0, P, g_S.lane_abs[lane]);
        g_S.c64_dist[lane] += g_S.vc_dist[lane]; g_S.c64_cbf[lane][k] = (uint8_t)cbf;
        G->c64_distk[lane][k] = g_S.vc_dist[lane]; cab_copy1(&G->c64_state[lane][k], &g_S.cab[c]);
      }
    }
  }
  FCU_SERIAL {                                               /* strict '<' in candidate order (TEncSearch.cpp:2488-2510) */
    double best = FCU_MAX_DOUBLE; int bv = 0;
    for (int cand = 0; cand < nc; cand++) {
      const double c = rd_cost(P, (uint32_t)(g_S.cab[CAB_LANE0 + cand].frac >> 15), g_S.c64_dist[cand]);
      if (c < best) { best = c; bv = cand; }
    }
    g_S.pu_best_vc = bv; g_S.pu_best_cost = best; g_S.pu_best_dist = g_S.c64_dist[bv]; g_S.pu_best_mode = g_S.rd_mode[bv];
    g_S.c64_valid = 1;
  }
  {                                                          /* xSetIntraResultLumaQT + decision snapshot of the winner */
    const int bv = g_S.pu_best_vc;
    Yuv *reco = &G->reco[d][1 - g_S.reco_best_idx[d]];
    const int any = g_S.c64_cbf[bv][0] | g_S.c64_cbf[bv][1] | g_S.c64_cbf[bv][2] | g_S.c64_cbf[bv][3];
    FCU_FOR_LANES {
      for (int i = lane; i < CTU * CTU; i += 64) { cu->coef[0][i] = G->c64_coef[bv][i]; reco->y[i] = G->c64_rec[bv][i]; }
      for (int i = lane; i < root.nparts; i += 64) {
        G->tmp_tr_idx[i] = 1; G->tmp_cbf[i] = (uint8_t)((g_S.c64_cbf[bv][i / (root.nparts >> 2)] << 1) | any); G->tmp_tskip[i] = 0;
      }
    }
  }
}

/* ======================================================================================== */
/* estIntraPredLumaQT, TEncSearch.cpp:2178-2655                                               */
/* ======================================================================================== */
FCU_DEV int pu_trace_index(int depth, int nxn, int zidx) { return nxn ? 85 + zidx : (depth == 0 ? 0 : depth == 1 ? 1 + (zidx >> 6) : depth == 2 ? 5 + (zidx >> 4) : 21 + (zidx >> 2)); }   /* = fcu_pu_index (include/fcu.h) */
FCU_DEV FCU_NOINLINE void est_intra_pred_luma(CuObj *cu)
{
  const Env E = env_get(); cu = FCU_UNI(cu);
  Scratch *G = E.G;
  const int d = cu->depth_cu, partSize = cu->part_size[0];
  const int initTrDepth = partSize == SIZE_2Nx2N ? 0 : 1, numPU = 1 << (2 * initTrDepth), qNumParts = cu->nparts >> 2;
  uint32_t overallDistY = 0;
  TU root; tu_root(root, d);
  Yuv *recoT = &G->reco[d][1 - g_S.reco_best_idx[d]];
  const int keepLuma = initTrDepth == 0;                     /* 2Nx2N: the CU's bits come from the search's coders (check_rd_cost_intra) */
  for (int pu = 0; pu < numPU; pu++) {
    TU tu; if (initTrDepth == 0) tu = root; else tu_child(tu, root, pu, 0);
    const int partOffset = tu.part, N = 1 << tu.log2, log2 = tu.log2;
    FCU_SERIAL { g_S.c64_valid = 0; g_S.lf_valid = 0; }
    { FCU_TIC(t_); rmd(cu, tu_key(tu)); FCU_TOC(E, t_, 0); }
    fcu_pu_trace *ptr = FCU_UNI(E.C->pu_trace ? E.C->pu_trace + (size_t)E.cur_ctu * FCU_PUS_PER_CTU + pu_trace_index(d, initTrDepth, cu->zidx + partOffset) : (fcu_pu_trace *)nullptr);
    if (ptr) FCU_SERIAL {                                    /* candidate list and CandCostList as the RMD leaves them */
      const int nRmd = k_rd_mode_num[log2 - 2];
      ptr->n_rmd = (uint8_t)nRmd; ptr->n_rd = (uint8_t)g_S.n_rd; ptr->pad = 0;
      for (int i = 0; i < 12; i++) ptr->rd_mode[i] = (uint8_t)(i < g_S.n_rd ? g_S.rd_mode[i] : 0);
      for (int i = 0; i < 8; i++) ptr->rmd_cost[i] = i < nRmd ? g_S.cand_cost[i] : 0.0;
    }
    const int singleTU = log2 <= LOG2_MAXTU;                /* first pass never splits such a PU */
    if (singleTU) { FCU_TIC(t_); pu_first_pass_batched(cu, tu_key(tu)); FCU_TOC(E, t_, 1); }
    else if (g_S.n_rd <= 5) { FCU_TIC(t_); pu_first_pass_64(cu, tu_key(tu)); FCU_TOC(E, t_, 1); }   /* 64x64: four 32x32 TUs, candidates side by side */
    else {                                                   /* more candidates than the pools hold: one after the other */
      FCU_SERIAL { g_S.pu_best_cost = FCU_MAX_DOUBLE; g_S.pu_best_mode = 0; g_S.pu_best_dist = 0; }
      const int nc = g_S.n_rd;
      for (int m = 0; m < nc; m++) {
        const int orgMode = g_S.rd_mode[m];
        FCU_FOR_LANES { for (int i = lane; i < tu.nparts; i += 64) cu->intra_dir[0][partOffset + i] = (uint8_t)orgMode; cab_copy(&g_S.cab[CAB_GOON], slot_ptr(E, d, CI_CURR_BEST), lane); if (lane == 0) { g_S.q_dist[0] = 0; g_S.q_cost[0] = 0; g_S.q_frac[0] = 0; g_S.q_bins[0] = 0; } }
        recur_luma_qt<0>(cu, tu_key(tu), 1);
        if (g_S.q_cost[0] < g_S.pu_best_cost) {
          FCU_SERIAL { g_S.pu_best_mode = orgMode; g_S.pu_best_dist = g_S.q_dist[0]; g_S.pu_best_cost = g_S.q_cost[0]; g_S.lf_frac = (slot_ptr(E, d, CI_CURR_BEST)->frac & 32767) + g_S.q_frac[0]; g_S.lf_bins = g_S.q_bins[0]; g_S.lf_valid = keepLuma; }
          set_intra_result_luma_qt(cu, tu_key(tu), recoT);
          FCU_FOR_LANES { for (int i = lane; i < tu.nparts; i += 64) { G->tmp_tr_idx[i] = cu->tr_idx[partOffset + i]; G->tmp_cbf[i] = cu->cbf[0][partOffset + i]; G->tmp_tskip[i] = cu->tskip[0][partOffset + i]; } if (keepLuma) cab_copy(&g_S.cab[CAB_LUMA], &g_S.cab[CAB_GOON], lane); }
        }
      }
    }
    if (keepLuma && (singleTU || g_S.n_rd <= 5)) {
      /* The winner's lane coder is the coder after the walk of the CU's luma encoding, unless the re-run below finds a
       * cheaper tree: kept for check_rd_cost_intra, out of reach of the tenants of the lane coders (est table, RMD
       * staging, chroma search). */
      const int w = CAB_LANE0 + (singleTU ? FCU_UNI((int)g_S.vc_slot[g_S.pu_best_vc]) : FCU_UNI(g_S.pu_best_vc));
      FCU_FOR_LANES { cab_copy(&g_S.cab[CAB_LUMA], &g_S.cab[w], lane); if (lane == 0) { g_S.lf_frac = g_S.cab[w].frac; g_S.lf_bins = g_S.cab[w].bins; g_S.lf_valid = 1; } }
    }
    /* best mode again with the full RQT (TEncSearch.cpp:2518-2586).  When the TU cannot split the
     * re-run reproduces the first-pass trial exactly (same snapshot, same inputs) and `<` keeps the
     * earlier result, so it is skipped. */
    if (log2 > min_tu_log2_in_cu(d, partSize)) {
      const int orgMode = g_S.pu_best_mode;
      FCU_FOR_LANES { for (int i = lane; i < tu.nparts; i += 64) cu->intra_dir[0][partOffset + i] = (uint8_t)orgMode; cab_copy(&g_S.cab[CAB_GOON], slot_ptr(E, d, CI_CURR_BEST), lane); if (lane == 0) { g_S.q_dist[0] = 0; g_S.q_cost[0] = 0; g_S.q_frac[0] = 0; g_S.q_bins[0] = 0; } }
      { FCU_TIC(t_); recur_luma_qt<0>(cu, tu_key(tu), 0, singleTU ? g_S.pu_best_vc : -1); FCU_TOC(E, t_, 4); }
      if (g_S.q_cost[0] < g_S.pu_best_cost) {                /* the go-on coder is the coder after the walk of the chosen tree, q_frac / q_bins[0] its counts */
        FCU_SERIAL { g_S.pu_best_dist = g_S.q_dist[0]; g_S.pu_best_cost = g_S.q_cost[0]; g_S.lf_frac = (slot_ptr(E, d, CI_CURR_BEST)->frac & 32767) + g_S.q_frac[0]; g_S.lf_bins = g_S.q_bins[0]; g_S.lf_valid = keepLuma; }
        set_intra_result_luma_qt(cu, tu_key(tu), recoT);
        FCU_FOR_LANES { for (int i = lane; i < tu.nparts; i += 64) { G->tmp_tr_idx[i] = cu->tr_idx[partOffset + i]; G->tmp_cbf[i] = cu->cbf[0][partOffset + i]; G->tmp_tskip[i] = cu->tskip[0][partOffset + i]; } if (keepLuma) cab_copy(&g_S.cab[CAB_LUMA], &g_S.cab[CAB_GOON], lane); }
      }
    }
    overallDistY += g_S.pu_best_dist;
    const int bestMode = g_S.pu_best_mode;
    if (ptr) FCU_SERIAL { ptr->best_mode = (uint8_t)g_S.pu_best_mode; ptr->best_dist = g_S.pu_best_dist; ptr->best_cost = g_S.pu_best_cost; ptr->valid = 1; }
    FCU_FOR_LANES {
      for (int i = lane; i < tu.nparts; i += 64) {
        cu->tr_idx[partOffset + i] = G->tmp_tr_idx[i]; cu->cbf[0][partOffset + i] = G->tmp_cbf[i]; cu->tskip[0][partOffset + i] = G->tmp_tskip[i];
        cu->intra_dir[0][partOffset + i] = (uint8_t)bestMode;
      }
      if (pu != numPU - 1) {
        uint8_t *p = E.C->rec[0] + (cu->y + tu.y) * E.C->stride[0] + cu->x + tu.x; const int rs = E.C->stride[0];
        for (int i = lane; i < N * N; i += 64) p[(i >> log2) * rs + (i & (N - 1))] = recoT->y[(tu.y + (i >> log2)) * 64 + tu.x + (i & (N - 1))];
      }
    }
  }
  if (numPU > 1) {
    FCU_SERIAL {
      uint8_t cy = 0, cu1 = 0, cv = 0;
      for (int p = 0, idx = 0; p < 4; p++, idx += qNumParts) { cy |= (cu->cbf[0][idx] >> 1) & 1; cu1 |= (cu->cbf[1][idx] >> 1) & 1; cv |= (cu->cbf[2][idx] >> 1) & 1; }
      for (int o = 0; o < 4 * qNumParts; o++) { cu->cbf[0][o] |= cy; cu->cbf[1][o] |= cu1; cu->cbf[2][o] |= cv; }
    }
  }
  FCU_FOR_LANES { cab_copy(&g_S.cab[CAB_GOON], slot_ptr(E, d, CI_CURR_BEST), lane); if (lane == 0) cu->dist = overallDistY; }
}

/* ======================================================================================== */
/* chroma search, the five modes side by side (estIntraPredChromaQT + xRecurIntraChroma-      */
/* CodingQT, TEncSearch.cpp:1916-2120,2661-2810).  Every mode restarts from [d][CURR_BEST]    */
/* (:2713) and only reads its OWN reconstruction inside the CU, so the modes are independent:  */
/* the luma TU tree is walked once, and at every chroma leaf the wave runs prediction /         */
/* transform / reconstruction for all modes, RDOQ and bit counting one mode (x transform-skip   */
/* variant) per lane on lane-private coders.                                                   */
/* ======================================================================================== */
FCU_DEV void chroma_leaf_refs5(const Env E, const CuObj *cu, int comp, int px, int py, int log2)
{
  /* reference samples of one chroma block for the five modes: outside the CU from the picture, inside from
   * the mode's own overlay (what PicYuvRec would hold during that mode's trial, TEncSearch.cpp:1374) */
  Scratch *G = E.G;
  const int N = 1 << log2, total = 4 * N + 1, lx0 = px << 1, ly0 = py << 1;
  const uint8_t *rec = E.C->rec[comp]; const int stride = E.C->stride[comp];
  const int cx0 = cu->x >> 1, cy0 = cu->y >> 1, cs = (CTU >> cu->depth_cu) >> 1;
  uint8_t *avail = (uint8_t *)g_S.colsum;
  FCU_FOR_LANES {
    if (lane == 0) g_S.ref_tag = -1;                         /* ref5b overlays ref / reff */
    for (int i = lane; i < total; i += 64) {
      int a, x, y;
      if (i < 2 * N) { y = py + 2 * N - 1 - i; x = px - 1; a = unit_available(E, lx0 - 4, (y / 2 * 2) << 1, lx0, ly0); }
      else if (i == 2 * N) { y = py - 1; x = px - 1; a = unit_available(E, lx0 - 4, ly0 - 4, lx0, ly0); }
      else { x = px + i - 2 * N - 1; y = py - 1; a = unit_available(E, (x / 2 * 2) << 1, ly0 - 4, lx0, ly0); }
      avail[i] = (uint8_t)a;
      if (a) {
        const int inside = x >= cx0 && x < cx0 + cs && y >= cy0 && y < cy0 + cs;
        for (int m = 0; m < 5; m++) {
          const uint8_t *ov = comp == 1 ? G->cm[m].u : G->cm[m].v;
          g_S.ref5[m][i] = inside ? ov[(y - cy0) * 32 + (x - cx0)] : rec[y * stride + x];
        }
      }
    }
  }
  FCU_FOR_LANES {
    for (int i = lane; i < total; i += 64) {
      if (!avail[i]) {
        int j = i - 1;
        while (j >= 0 && !avail[j]) j--;
        if (j < 0) { j = i + 1; while (j < total && !avail[j]) j++; }
        for (int m = 0; m < 5; m++) g_S.ref5b[m][i] = (j < total) ? g_S.ref5[m][j] : 128;
      }
    }
  }
  FCU_FOR_LANES { for (int i = lane; i < total; i += 64) if (!avail[i]) for (int m = 0; m < 5; m++) g_S.ref5[m][i] = g_S.ref5b[m][i]; }
  FCU_FOR_LANES { if (lane < 5) { int sum = 0; for (int i = 0; i < N; i++) sum += g_S.ref5[lane][2 * N + 1 + i] + g_S.ref5[lane][2 * N - 1 - i]; g_S.dc5[lane] = (sum + N) >> (log2 + 1); } }
}

/* xGetIntraBitsQT(rTu, false, true) for mode slot m from the lane-private coder c (serial, one lane) */
FCU_DEV FCU_NOINLINE uint32_t chroma_tree_bits(int c, const CuObj *cu, int m, int mode, int16_t *absbuf)
{
  const Env E = env_get(); cu = FCU_UNI(cu);
  FCU_IN_LDS(absbuf);
  const ChromaModeBuf *B = &E.G->cm[m];
  FCU_EMU_RELAX(1);
  cab_reset_bits(c);
  code_intra_dir_chroma(c, mode);
  /* the five lanes (modes) walk the same luma TU tree in lockstep: they share the LDS walker stack (same values) */
  TU *st = g_S.wk_st; int *ci = g_S.wk_ci;
  for (int pass = 0; pass < 3; pass++) {                      /* 0: subdiv/cbf walk, 1: Cb coefficients, 2: Cr coefficients */
    int sp = 0; tu_root(st[0], cu->depth_cu); ci[0] = -1;
    while (sp >= 0) {
      const TU tu = st[sp];
      if (ci[sp] < 0) {
        const int subdiv = cu->tr_idx[tu.part] > tu.tr_depth;
        if (pass == 0) {
          for (int k = 0; k < 2; k++)
            if (tu.c_code_all && (tu.tr_depth == 0 || ((B->cbf[k][tu.part] >> (tu.tr_depth - 1)) & 1))) {
              const int lowest = tu.tr_depth + ((subdiv && !(tu.cw >= 8)) ? 1 : 0);
              cab_bin(c, (B->cbf[k][tu_part_c(tu)] >> lowest) & 1, CTX_CBF_CHROMA + tu.tr_depth);
            }
        } else if (!subdiv) {
          const int k = pass - 1;
          if (tu.cw != 0 && ((B->cbf[k][tu.part] >> tu.tr_depth) & 1)) {
            const int log2 = ilog2(tu.cw), pc = tu_part_c(tu);
            const int fmode = mode == DM_CHROMA ? cu->intra_dir[0][pc & ~3] : mode;
            code_coeff_nxn<0>(c, B->coef[k] + tu.off_c, 1, -1, log2, 1 + k, coef_scan_idx(fmode, log2, 1 + k), B->tskip[k][pc], E.C->p, absbuf);
          }
        }
        if (!subdiv) { sp--; continue; }
        ci[sp] = 0;
      }
      if (ci[sp] >= 4) { sp--; continue; }
      { TU ch; tu_child(ch, st[sp], ci[sp], 0); ci[sp]++; sp++; st[sp] = ch; ci[sp] = -1; }
    }
  }
  FCU_EMU_RELAX(0);
  return cab_bits(c);
}

/* one chroma leaf of the TU tree: both components, the five modes (x transform-skip variant) side by side */
FCU_DEV FCU_NOINLINE void chroma_leaf_trials(CuObj *cu, uint32_t tu_k)
{
  const Env E = env_get(); cu = FCU_UNI(cu); const TU tu = tu_of_key(FCU_UNI(tu_k));
  Scratch *G = E.G; const Params &P = E.C->p;
  const int d = cu->depth_cu;
  const int N = tu.cw, log2 = ilog2(N), n2 = N * N, trDepth = tu.tr_depth;
  int checkTS = P.transform_skip && N <= 4;
  if (P.ts_fast) {
    checkTS = checkTS && (tu.log2 == 2);
    if (checkTS) { int nb = 0; const int maxp = tu.part + (tu.c_code_all ? 1 : 4); for (int p = tu.part; p < maxp; p++) nb += cu->tskip[0][p]; checkTS = checkTS && (nb > 0); }
  }
  const int tsv = checkTS ? 2 : 1, tss = tsv - 1;                /* v / tsv == v >> tss, v % tsv == v & tss */
  FCU_SMALL_COUNT(SMALL_CHROMA_4X4, log2 == 2);                 /* (the chroma trials all run here: nobody calls tu_trial with comp != 0) */
  /* Without a transform-skip trial nothing is coded between the two components (the bits are counted on the whole tree
   * afterwards), so Cb and Cr of a mode are priced against the same coder state and are independent of each other: both
   * go through one round, ten variants side by side.  With the trial the coder moves on after Cb's winner
   * (TEncSearch.cpp:1985-2058) and the components stay in sequence; so do 32x32 blocks, which would not fit the pools. */
  const int perRound = (tsv == 1 && 10 * n2 <= POOL) ? 2 : 1;
  const int nm = 5 * perRound, nvc = nm * tsv;                  /* prediction blocks / variants of a round */
  const int qbits = rdoq_qbits(log2, P.qp_c), qscale = k_quant_scales[P.qp_c % 6];
  const int subPart = tu_part_c(tu), nPartsC = tu_nparts_c(tu);
  const int lumaDir = cu->intra_dir[0][tu.part & ~3];
  for (int comp0 = 1; comp0 < 3; comp0 += perRound) {
    const int px = (cu->x >> 1) + tu.cx, py = (cu->y >> 1) + tu.cy;
    for (int cc = 0; cc < perRound; cc++) {
      const int comp = comp0 + cc;
      const uint8_t *org = yuv_plane(&G->org[d], comp) + tu.cy * 32 + tu.cx;
      chroma_leaf_refs5(E, cu, comp, px, py, log2);
      FCU_FOR_LANES {
        for (int i = lane; i < 5 * n2; i += 64) {
          const int m = i / n2, p = i - m * n2, y = p >> log2, x = p & (N - 1);
          const int mode = g_S.c_modes[m] == DM_CHROMA ? lumaDir : g_S.c_modes[m];
          const int pr = pred_pixel(g_S.ref5[m], log2, mode, 0, g_S.dc5[m], x, y);
          G->p_pred[cc * 5 * n2 + i] = (uint8_t)pr; G->p_resi[cc * 5 * n2 + i] = (int16_t)(org[y * 32 + x] - pr);
        }
      }
    }
    FCU_FOR_LANES { if (lane < nvc) g_S.vc_last[lane] = -1; by_log2(log2, [&](auto L) { constexpr int LG = decltype(L)::value; RowCache<(1 << LG), int16_t> rc; for (int i = lane; i < nm * n2; i += 64) { const int b = i / n2; G->p_tmp[i] = fwd1<LG>(rc, G->p_resi + b * n2, 0, i - b * n2); } }); }
    FCU_FOR_LANES {
      by_log2(log2, [&](auto L) { constexpr int LG = decltype(L)::value; RowCache<(1 << LG), int32_t> rc;
        for (int i = lane; i < nvc * n2; i += 64) {
          const int v = i / n2, p = i - v * n2, b = (v >> tss), ts = (v & tss), m = b % 5, comp = comp0 + b / 5;
          const int mode = g_S.c_modes[m] == DM_CHROMA ? lumaDir : g_S.c_modes[m];
          const uint16_t *iscan = k_iscan + k_scan_off[coef_scan_idx(mode, log2, comp) * 4 + log2 - 2];
          const int32_t t = ts ? ((int32_t)G->p_resi[b * n2 + p] << (15 - 8 - log2)) : fwd2<LG>(rc, G->p_tmp + b * n2, 0, p);
          const int sp = iscan[p]; const int32_t ld = level_double(t, qscale, qbits);
          G->p_lscan[sp * nvc + v] = ld;
          if (level_nonzero(ld, qbits)) FCU_ATOMIC_MAX(&g_S.vc_last[v], sp);
        }
      });
    }
    FCU_TIC(t13_);
    FCU_FOR_LANES {                                      /* RDOQ from the mode's coder state (its QT_TRAFO_ROOT) */
      if (lane < nvc) {
        const int b = (lane >> tss), m = b % 5, comp = comp0 + b / 5;
        const int mode = g_S.c_modes[m] == DM_CHROMA ? lumaDir : g_S.c_modes[m];
        RdoqRec *rrec = G->r_rec + lane; double *rcg = G->r_cg + lane;
        const RdoqOut o = ((lane & tss) ? P.rdoq_ts : P.rdoq)
          ? rdoq<0>(CAB_LANE0 + m, G->p_lscan + lane, G->p_qscan + lane, nvc, g_S.vc_last[lane], log2, 1 /* Cb and Cr share every parameter the call reads; the argument is wave-uniform */, coef_scan_idx(mode, log2, comp), CTX_CBF_CHROMA + trDepth, P, rrec, rcg, lane)
          : quant_plain(G->p_lscan + lane, G->p_qscan + lane, nvc, g_S.vc_last[lane], log2, 1, P);
        g_S.vc_abs[lane] = o.abs_sum; g_S.vc_lsp[lane] = o.last;
        g_S.vc_dist[lane] = 0;
      }
      if (lane == 0) E.C->n_tu_trials += (unsigned long long)nvc;
    }
    FCU_TOC(E, t13_, 13);
    FCU_FOR_LANES {                                      /* levels back to raster order + dequantisation */
      const DeqParams dq = deq_params(log2, P.qp_c);
      for (int i = lane; i < nvc * n2; i += 64) {
        const int v = i / n2, p = i - v * n2, b = (v >> tss), m = b % 5, comp = comp0 + b / 5;
        const int mode = g_S.c_modes[m] == DM_CHROMA ? lumaDir : g_S.c_modes[m];
        const uint16_t *iscan = k_iscan + k_scan_off[coef_scan_idx(mode, log2, comp) * 4 + log2 - 2];
        const int sp = iscan[p];
        const int q = (g_S.vc_abs[v] > 0 && (sp >> 4) <= (g_S.vc_last[v] >> 4)) ? G->p_qscan[sp * nvc + v] : 0;
        G->p_tmp[((v & tss)) ? i : v * n2 + tr_index(p, log2)] = dequant1(q, dq);
      }
    }
    FCU_FOR_LANES {
      by_log2(log2, [&](auto L) { constexpr int LG = decltype(L)::value; RowCache<(1 << LG), int32_t> rc;
        for (int i = lane; i < nvc * n2; i += 64) {
          const int v = i / n2, p = i - v * n2, ts = (v & tss);
          if (ts) { const int sft = 15 - 8 - log2; G->p_tcoef[i] = (G->p_tmp[i] + (1 << (sft - 1))) >> sft; }
          else G->p_tcoef[i] = inv1<LG>(rc, G->p_tmp + v * n2, 0, p);
        }
      });
    }
    FCU_FOR_LANES {
      by_log2(log2, [&](auto L) {
        uint32_t acc = 0;
        for (int i = lane; i < nvc * n2; i += 64) {
          const int v = i / n2, p = i - v * n2, b = (v >> tss), ts = (v & tss), y = p >> log2, x = p & (N - 1);
          const uint8_t *org = yuv_plane(&G->org[d], comp0 + b / 5) + tu.cy * 32 + tu.cx;
          int res = 0;
          if (g_S.vc_abs[v] > 0) res = ts ? (int16_t)G->p_tcoef[i] : inv2<decltype(L)::value>(G->p_tcoef + v * n2, 0, p);
          const int r = clip8(G->p_pred[b * n2 + p] + res);
          G->p_rec[i] = (uint8_t)r;
          const int e = org[y * 32 + x] - r;
          FCU_DIST_ADD(acc, v, e, i, n2);
        }
      });
    }
    FCU_FOR_LANES {                                      /* per mode: transform-skip decision (TEncSearch.cpp:1985-2058) */
      if (lane < 5) {
        const int m = lane; int bestTs = 0;
        const int mode = g_S.c_modes[m] == DM_CHROMA ? lumaDir : g_S.c_modes[m];
        if (tsv == 2) {                                      /* one component per round: variants 2m (coded) and 2m+1 (skipped) */
          const int comp = comp0;
          uint32_t dsel = (uint32_t)(P.chroma_weight * (double)g_S.vc_dist[m * 2]);
          const uint32_t d0 = dsel, d1 = (uint32_t)(P.chroma_weight * (double)g_S.vc_dist[m * 2 + 1]);
          const int c0 = CAB_LANE0 + 5 + m, c1 = CAB_LANE0 + 10 + m;
          cab_copy1(&g_S.cab[c0], &g_S.cab[CAB_LANE0 + m]); cab_reset_bits(c0);
          if (g_S.vc_abs[m * 2] > 0) code_coeff_nxn<0>(c0, G->p_qscan + m * 2, nvc, g_S.vc_lsp[m * 2], log2, comp, coef_scan_idx(mode, log2, comp), 0, P, g_S.lane_abs[lane]);
          const double cost0 = rd_cost(P, cab_bits(c0), d0);
          double cost1 = FCU_MAX_DOUBLE;
          if (g_S.vc_abs[m * 2 + 1] > 0) {
            cab_copy1(&g_S.cab[c1], &g_S.cab[CAB_LANE0 + m]); cab_reset_bits(c1);
            code_coeff_nxn<0>(c1, G->p_qscan + m * 2 + 1, nvc, g_S.vc_lsp[m * 2 + 1], log2, comp, coef_scan_idx(mode, log2, comp), 1, P, g_S.lane_abs[lane]);
            cost1 = rd_cost(P, cab_bits(c1), d1);
          }
          if (cost1 < cost0) { bestTs = 1; dsel = d1; cab_copy1(&g_S.cab[CAB_LANE0 + m], &g_S.cab[c1]); } else cab_copy1(&g_S.cab[CAB_LANE0 + m], &g_S.cab[c0]);
          g_S.cm_dist[m] += dsel;
        } else {
          for (int cc = 0; cc < perRound; cc++) g_S.cm_dist[m] += (uint32_t)(P.chroma_weight * (double)g_S.vc_dist[cc * 5 + m]);
        }
        g_S.uni[m] = bestTs;
      }
    }
    FCU_FOR_LANES {                                      /* publish the chosen variant into the mode's buffers */
      for (int i = lane; i < nm * n2; i += 64) {
        const int b = i / n2, p = i - b * n2, m = b % 5, comp = comp0 + b / 5, v = b * tsv + g_S.uni[m], cbf = g_S.vc_abs[v] > 0;
        G->cm[m].coef[comp - 1][tu.off_c + p] = (cbf && (p >> 4) <= (g_S.vc_last[v] >> 4)) ? G->p_qscan[p * nvc + v] : (int16_t)0;
        uint8_t *ov = comp == 1 ? G->cm[m].u : G->cm[m].v;
        ov[(tu.cy + (p >> log2)) * 32 + tu.cx + (p & (N - 1))] = G->p_rec[v * n2 + p];
      }
      for (int i = lane; i < nm * nPartsC; i += 64) {
        const int b = i / nPartsC, p = i - b * nPartsC, m = b % 5, comp = comp0 + b / 5, v = b * tsv + g_S.uni[m];
        G->cm[m].cbf[comp - 1][subPart + p] = (uint8_t)((g_S.vc_abs[v] > 0 ? 1 : 0) << trDepth);
        G->cm[m].tskip[comp - 1][subPart + p] = (uint8_t)g_S.uni[m];
      }
    }
  }
}

FCU_DEV FCU_NOINLINE void est_intra_pred_chroma(CuObj *cu)
{
  const Env E = env_get(); cu = FCU_UNI(cu);
  Scratch *G = E.G; const Params &P = E.C->p;
  const int d = cu->depth_cu, n = cu->nparts, cs = (CTU >> d) >> 1;
  /* getAllowedChromaDir, TComDataCU.cpp:1509-1533; the list lives in LDS (it is indexed per element below) */
  FCU_FOR_LANES {
    if (lane == 0) {
      int ml[5] = { PLANAR, VER, HOR, DC, DM_CHROMA };
      const int luma = cu->intra_dir[0][0]; for (int i = 0; i < 4; i++) if (luma == ml[i]) { ml[i] = 34; break; }
      for (int i = 0; i < 5; i++) g_S.c_modes[i] = ml[i];
    }
    if (lane < 5) { cab_copy1(&g_S.cab[CAB_LANE0 + lane], slot_ptr(E, d, CI_CURR_BEST)); g_S.cm_dist[lane] = 0; }
    for (int i = lane; i < 5 * n; i += 64) { const int m = i / n, p = i - m * n; G->cm[m].cbf[0][p] = G->cm[m].cbf[1][p] = 0; G->cm[m].tskip[0][p] = G->cm[m].tskip[1][p] = 0; }
  }
  /* ---- walk the luma TU tree; chroma leaves in z-order ---- */
  TU *st = g_S.wk_st; int *ci = g_S.wk_ci; int sp = 0;
  tu_root(st[0], d); ci[0] = -1;
  while (sp >= 0) {
    if (ci[sp] < 0) {
      const TU tu = st[sp];
      const int subdiv = cu->tr_idx[tu.part] > tu.tr_depth;
      if (!subdiv) {
        if (tu.cw != 0) chroma_leaf_trials(cu, tu_key(tu));
        sp--; continue;
      }
      ci[sp] = 0;
    }
    if (ci[sp] >= 4) { sp--; continue; }
    { TU ch; tu_child(ch, st[sp], ci[sp], 0); ci[sp]++; sp++; st[sp] = ch; ci[sp] = -1; }
  }
  /* ---- per mode: CBF propagation up the tree, bits, cost ---- */
  FCU_TIC(t14_);
  FCU_FOR_LANES {
    if (lane < 5) {
      const int m = lane; ChromaModeBuf *B = &G->cm[m];
      for (int t = 2; t >= 0; t--) {                            /* nodes of relative depth t, deepest first */
        const int np = n >> (2 * t);
        if (np < 4) continue;
        for (int part = 0; part < n; part += np) {
          if (!(cu->tr_idx[part] > t)) continue;
          for (int k = 0; k < 2; k++) {
            int any = 0;
            for (int q = 0; q < 4; q++) any |= (B->cbf[k][part + q * (np >> 2)] >> (t + 1)) & 1;
            if (any) for (int o = 0; o < np; o++) B->cbf[k][part + o] |= (uint8_t)(1 << t);
          }
        }
      }
      const int c = CAB_LANE0 + 5 + m;
      cab_copy1(&g_S.cab[c], slot_ptr(E, d, CI_CURR_BEST));
      g_S.vc_bits[m] = chroma_tree_bits(c, cu, m, g_S.c_modes[m], g_S.lane_abs[lane]);
      g_S.vc_cost[m] = rd_cost(P, g_S.vc_bits[m], g_S.cm_dist[m]);
    }
  }
  FCU_TOC(E, t14_, 14);
  FCU_SERIAL {
    double best = FCU_MAX_DOUBLE; int bm = 0;
    for (int m = 0; m < 5; m++) if (g_S.vc_cost[m] < best) { best = g_S.vc_cost[m]; bm = m; }
    g_S.c_best_mode = bm;
  }
  {
    const int bm = g_S.c_best_mode; const ChromaModeBuf *B = &G->cm[bm];
    Yuv *recoT = &G->reco[d][1 - g_S.reco_best_idx[d]];
    FCU_FOR_LANES {
      for (int i = lane; i < cs * cs; i += 64) {
        cu->coef[1][i] = B->coef[0][i]; cu->coef[2][i] = B->coef[1][i];
        const int o = (i / cs) * 32 + (i % cs); recoT->u[o] = B->u[o]; recoT->v[o] = B->v[o];
      }
      for (int i = lane; i < n; i += 64) {
        cu->cbf[1][i] = B->cbf[0][i]; cu->cbf[2][i] = B->cbf[1][i]; cu->tskip[1][i] = B->tskip[0][i]; cu->tskip[2][i] = B->tskip[1][i];
        cu->intra_dir[1][i] = (uint8_t)g_S.c_modes[bm];
      }
      if (lane == 0) cu->dist += g_S.cm_dist[bm];
      cab_copy(&g_S.cab[CAB_GOON], slot_ptr(E, d, CI_CURR_BEST), lane);
    }
  }
}

/* ======================================================================================== */
/* CU level: xCheckRDCostIntra / xCheckBestMode / xCompressCU (TEncCu.cpp:460-1616,2064-2255)  */
/* ======================================================================================== */
FCU_DEV CuObj *cu_best(const Env E, int d) { return &E.G->cu[d][g_S.best_idx[d]]; }
FCU_DEV CuObj *cu_temp(const Env E, int d) { return &E.G->cu[d][1 - g_S.best_idx[d]]; }

FCU_DEV FCU_NOINLINE void check_best_mode(int d)
{
  const Env E = env_get(); d = FCU_UNI(d);
  const int change = cu_temp(E, d)->cost < cu_best(E, d)->cost;
  FCU_FOR_LANES {
    if (change) { cab_copy(slot_ptr(E, d, CI_NEXT_BEST), slot_ptr(E, d, CI_TEMP_BEST), lane); if (lane == 0) { g_S.best_idx[d] = 1 - g_S.best_idx[d]; g_S.reco_best_idx[d] = 1 - g_S.reco_best_idx[d]; } }
  }
}
FCU_DEV FCU_NOINLINE void check_rd_cost_intra(int d, int partSize)
{
  const Env E = env_get(); d = FCU_UNI(d); partSize = FCU_UNI(partSize);
  Scratch *G = E.G; const Params &P = E.C->p;
  CuObj *cu = cu_temp(E, d);
  const int n = cu->nparts, s = CTU >> d;
  FCU_FOR_LANES { for (int i = lane; i < n; i += 64) { cu->part_size[i] = (int8_t)partSize; cu->pred_mode[i] = MODE_INTRA; } }
  est_intra_pred_luma(cu);
  {
    const Yuv *recoT = &G->reco[d][1 - g_S.reco_best_idx[d]];
    FCU_FOR_LANES { uint8_t *p = E.C->rec[0] + cu->y * E.C->stride[0] + cu->x; const int rs = E.C->stride[0]; for (int i = lane; i < s * s; i += 64) p[(i / s) * rs + (i % s)] = recoT->y[(i / s) * 64 + (i % s)]; }
  }
  { FCU_TIC(t_); est_intra_pred_chroma(cu); FCU_TOC(E, t_, 6); }
  FCU_TIC(t7_);
#ifdef FCU_PROFILE_CUSYN
  if (threadIdx.x == 0) g_S.prof_s7 = partSize == SIZE_2Nx2N ? 1 : 2;
#endif
  /* The CU's bits (encodeCoeff from [d][CI_CURR_BEST], TEncCu.cpp:1753-1778).  A 2Nx2N CU is not walked again: the luma
   * search's chosen walk (cab[CAB_LUMA]) and the chroma search's (lane coder 5 + best mode) started from that snapshot too and
   * have between them pushed every bin of the CU through its context in the order of the final walk -- the two touch
   * disjoint contexts, a bin's cost depends on its own context only and the Q15 count is additive.  Cb and Cr
   * share their level contexts and the search codes all Cb leaves before the Cr leaves, so with more than one chroma leaf
   * the chroma part is walked again, leaf by leaf.  NxN (every PU searched from the snapshot, not from its predecessor's
   * state) and a CU without a kept luma coder take the full walk. */
  const int merge = partSize == SIZE_2Nx2N && FCU_UNI(g_S.lf_valid);
  const int oneLeaf = merge && (FCU_UNI((int)cu->tr_idx[0]) == 0 || d == MAXDEPTH);   /* un-split tree, or four 4x4 luma TUs over one 4x4 chroma block */
  if (!merge) {
    FCU_FOR_LANES {
      if (lane == 0) {
        cab_reset_bits((CAB_GOON));
        encode_cu_syntax(E, (CAB_GOON), cu, 0, d);
        cu->bits = cab_bits((CAB_GOON)); cu->bins = g_S.cab[CAB_GOON].bins;
        cu->cost = rd_cost(P, cu->bits, cu->dist);
      }
    }
    FCU_FOR_LANES cab_copy(slot_ptr(E, d, CI_TEMP_BEST), &g_S.cab[CAB_GOON], lane);
    FCU_SPATH(E, 2);
  } else {
    if (!oneLeaf) {
      FCU_FOR_LANES {
        if (lane == 0) {                                     /* the go-on coder is a copy of [d][CI_CURR_BEST] here */
          cab_reset_bits((CAB_GOON));
          code_intra_dir_chroma((CAB_GOON), cu->intra_dir[1][0]);
          TU root; tu_root(root, d);
          encode_transform((CAB_GOON), cu, 0, tu_key(root), 0);
        }
      }
    }
    const int cc = oneLeaf ? CAB_LANE0 + 5 + FCU_UNI(g_S.c_best_mode) : (int)CAB_GOON;
    FCU_FOR_LANES {
      const Cabac *cur = slot_ptr(E, d, CI_CURR_BEST), *lum = &g_S.cab[CAB_LUMA], *chr = &g_S.cab[cc];
      Cabac *tmp = slot_ptr(E, d, CI_TEMP_BEST), *go = &g_S.cab[CAB_GOON];
      if (lane < NCTX / 4) {                                 /* four contexts per lane: luma's byte where luma moved it, chroma's otherwise */
        const uint32_t k = ((const uint32_t *)cur->ctx)[lane], l = ((const uint32_t *)lum->ctx)[lane], c = ((const uint32_t *)chr->ctx)[lane];
        uint32_t m = 0;
        for (int b = 0; b < 32; b += 8) {
          const uint32_t kb = (k >> b) & 255, lb = (l >> b) & 255, cb = (c >> b) & 255;
          FCU_CHECK(lb == kb || cb == kb);                   /* no context is moved by both searches */
          m |= (lb != kb ? lb : cb) << b;
        }
        ((uint32_t *)tmp->ctx)[lane] = m; ((uint32_t *)go->ctx)[lane] = m;
      } else if (lane == NCTX / 4) {
        const uint64_t f = g_S.lf_frac + chr->frac - (cur->frac & 32767);
        const uint32_t nb = g_S.lf_bins + chr->bins;
        tmp->frac = f; tmp->bins = nb; tmp->pad_ = 0; go->frac = f; go->bins = nb; go->pad_ = 0;
        cu->bits = (uint32_t)(f >> 15); cu->bins = nb;
        cu->cost = rd_cost(P, cu->bits, cu->dist);
      }
    }
    FCU_SPATH(E, oneLeaf ? 0 : 1);
#ifdef FCU_EMU
    g_emu_cu_paths[oneLeaf ? 0 : 1]++;
#ifdef FCU_EMU_CHECK_CU_MERGE
    FCU_FOR_LANES {                                          /* the full walk on a spare lane coder must give the merged state */
      if (lane == 0) {
        const int w = CAB_LANE0 + MAXLC - 1;
        cab_copy1(&g_S.cab[w], slot_ptr(E, d, CI_CURR_BEST)); cab_reset_bits(w);
        encode_cu_syntax(E, w, cu, 0, d);
        const Cabac *tmp = slot_ptr(E, d, CI_TEMP_BEST);
        FCU_CHECK(memcmp(g_S.cab[w].ctx, tmp->ctx, NCTX) == 0);
        FCU_CHECK(g_S.cab[w].frac == tmp->frac); FCU_CHECK(g_S.cab[w].bins == tmp->bins);
        FCU_CHECK(cab_bits(w) == cu->bits); FCU_CHECK(g_S.cab[w].bins == cu->bins);
        FCU_CHECK(memcmp(&g_S.cab[CAB_GOON], tmp, sizeof(Cabac)) == 0);
      }
    }
#endif
#endif
  }
#ifdef FCU_EMU
  if (!merge) g_emu_cu_paths[2]++;
#endif
#ifdef FCU_PROFILE_CUSYN
  if (threadIdx.x == 0) g_S.prof_s7 = 0;
#endif
  FCU_TOC(E, t7_, 7);
  FCU_STOC(E, t7_, partSize == SIZE_2Nx2N ? 11 : 12);
  check_best_mode(d);
}

/* xCheckRDCostInter, TEncCu.cpp:2025-2062 */
FCU_DEV FCU_NOINLINE void check_rd_cost_inter(int d, int partSize, int useMrg)
{
  const Env E = env_get(); d = FCU_UNI(d); partSize = FCU_UNI(partSize); useMrg = FCU_UNI(useMrg);
  CuObj *cu = cu_temp(E, d);
  const int n = cu->nparts;
  FCU_FOR_LANES { for (int i = lane; i < n; i += 64) { cu->part_size[i] = (int8_t)partSize; cu->pred_mode[i] = MODE_INTER; } }
  pred_inter_search(cu, partSize, useMrg);
  { FCU_TIC(p_); encode_res_and_calc_rd_inter_cu(cu, 0); FCU_ITOC(E, p_, 9); }
  check_best_mode(d);
}
/* xCheckRDCostMerge2Nx2N, TEncCu.cpp:1900-2018 (early skip detection off) */
FCU_DEV FCU_NOINLINE void check_rd_cost_merge_2nx2n(int d)
{
  const Env E = env_get(); d = FCU_UNI(d);
  Scratch *G = E.G; const Params &P = E.C->p;
  const CuObj *t0 = cu_temp(E, d);
  const int x = t0->x, y = t0->y, zidx = t0->zidx, n = t0->nparts;
  FCU_FOR_LANES { CuObj *cu = cu_temp(E, d); for (int i = lane; i < n; i += 64) cu->part_size[i] = SIZE_2Nx2N; if (lane < 5) g_S.mrg_buf[lane] = 0; if (lane == 0) g_S.best_is_skip = 0; }
  FCU_SERIAL merge_candidates(cu_temp(E, d), SIZE_2Nx2N, 0);
  int cmv[5][2], cref[5];
  for (int c = 0; c < 5; c++) { cmv[c][0] = FCU_UNI(g_S.mrg_mv[c][0]); cmv[c][1] = FCU_UNI(g_S.mrg_mv[c][1]); cref[c] = FCU_UNI(g_S.mrg_ref[c]); }
  const int nc = P.max_merge_cand;
  for (int noRes = 0; noRes < 2; noRes++)
    for (int c = 0; c < nc; c++) {
      if (noRes == 1 && FCU_UNI(g_S.mrg_buf[c]) == 1) continue;
      if (FCU_UNI(g_S.best_is_skip) && noRes == 0) continue;
      CuObj *cu = cu_temp(E, d);
      FCU_FOR_LANES {
        for (int i = lane; i < n; i += 64) { cu->pred_mode[i] = MODE_INTER; cu->part_size[i] = SIZE_2Nx2N; }
        pu_set_motion(cu, SIZE_2Nx2N, 0, lane, cmv[c][0], cmv[c][1], cref[c]); pu_set_info(cu, SIZE_2Nx2N, 0, lane, 1, c, 0, 0, -1);
      }
      { FCU_TIC(p_); mc_pu(cu, SIZE_2Nx2N, 0, &G->predt[d], 0); FCU_ITOC(E, p_, 8); }
      { FCU_TIC(p_); encode_res_and_calc_rd_inter_cu(cu, noRes); FCU_ITOC(E, p_, noRes ? 12 : 11); }
      FCU_SERIAL { if (noRes == 0 && !qt_root_cbf(cu, 0)) g_S.mrg_buf[c] = 1; }
      check_best_mode(d);
      cu_init(cu_temp(E, d), d, x, y, zidx);
      FCU_SERIAL { if (P.fdm && !g_S.best_is_skip) g_S.best_is_skip = !qt_root_cbf(cu_best(E, d), 0); }
    }
}

/* fork hooks of xCompressCU for its default control (YSGlobalControl, tools_YS.cpp:4-58: Naive model on N_OBF).
 * Num_OBF = 4x4 blocks of the CU with a positive OBF count (TEncCu.cpp:585-600); the Naive label is Skip2Nx2N when
 * there is one, TerminateCU when there is none (tools_YS.cpp:686-695, TEncCu.cpp:670-678). */
FCU_DEV FCU_NOINLINE int cu_num_obf(int x, int y, int s)
{
  const Env E = env_get(); x = FCU_UNI(x); y = FCU_UNI(y); s = FCU_UNI(s);
  FCU_SERIAL g_S.dec_cnt = 0;
  FCU_FOR_LANES {
    const int q = s >> 2; int n = 0;
    for (int i = lane; i < q * q; i += 64) n += E.C->obf[((y >> 2) + i / q) * E.C->obf_stride + (x >> 2) + i % q] > 0;
    FCU_WAVE_ADD((uint32_t *)&g_S.dec_cnt, (uint32_t)n);
  }
  return FCU_UNI(g_S.dec_cnt);
}
/* The label a caller bound for the CU of depth D at picture position (x, y) (Chain::labels): one wave-uniform read.
 * 1 = Skip2Nx2N ("will be divided"), 0 = TerminateCU, -1 = no prediction (any other code: FCU_LABEL_ABSENT, FCU_LABEL_FORCED ...) */
template <int D>
FCU_DEV int cu_label(const Chain *C, int x, int y)
{
  x = FCU_UNI(x); y = FCU_UNI(y);
  const int v = ((const FCU_HBM int8_t *)C->labels)[C->lbl_off[D] + (y >> (6 - D)) * C->lbl_w[D] + (x >> (6 - D))];
  return FCU_UNI(v == FCU_LABEL_SPLIT ? 1 : (v == FCU_LABEL_NOT_SPLIT ? 0 : -1));
}
/* countTFPN + countRDLoss (tools_YS.cpp:968-986; ResultType order TP,FP,TN,FN,FPLoss,FNLoss, globals_YS.h:81-89) */
FCU_DEV void count_verify(Chain *C, int d, int predictSkip, int partitionTrue, double j0, double j1)
{
  const double loss = fabs(j0 - j1);
  if (predictSkip) { C->ver[d][partitionTrue ? 0 : 1] += 1.0; if (!partitionTrue) C->ver[d][4] += loss; }
  else { C->ver[d][partitionTrue ? 3 : 2] += 1.0; if (partitionTrue) C->ver[d][5] += loss; }
}

/* -DFCU_PROFILE -DFCU_PROFILE_DEPTH: prof[11 + D] = ticks spent at CU depth D without its sub-CUs (what a wave-per-depth
 * frontier could overlap; measured on MI355X: 13 / 17 / 21 / 48 % for depths 0..3) */
#if defined(FCU_PROFILE) && defined(FCU_PROFILE_DEPTH) && !defined(FCU_EMU)
#define FCU_DTIC(v) long long v = clock64()
#define FCU_DADD(E_, v, idx, sign) do { if (threadIdx.x == 0) (E_).C->prof[idx] += (unsigned long long)((sign) * (clock64() - v)); } while (0)
#else
#define FCU_DTIC(v) do { } while (0)
#define FCU_DADD(E_, v, idx, sign) do { } while (0)
#endif
template <int D>
FCU_DEV FCU_NOINLINE void compress_cu()
{
  const Env E = env_get();
  FCU_DTIC(dt_);
  Scratch *G = E.G; const Params &P = E.C->p;
  const CuObj *b0 = cu_best(E, D);
  const int x = b0->x, y = b0->y, zidx = b0->zidx, s = CTU >> D;
  const int boundary = !((x + s - 1 < P.width) && (y + s - 1 < P.height));
  const int state = E.C->dec_state;
  /* predictSkip: 1 = the label Skip2Nx2N, 0 = TerminateCU, -1 = no prediction (a caller's label array may leave a CU open: it is
   * searched exhaustively and not counted).  The Naive model always predicts. */
  int skip2Nx2N = 0, earlyTerminate = 0, predictSkip = -1;
  int nxnTried = 0;                                          /* (D == MAXDEPTH only) */
  if (!boundary && state != DEC_TRAINING) {
    predictSkip = E.C->labels ? cu_label<D>(E.C, x, y) : (cu_num_obf(x, y, s) > 0);
    if (state == DEC_TESTING && predictSkip >= 0) {          /* TEncCu.cpp:951-996 */
      if (E.C->sw_term[D]) earlyTerminate = !predictSkip;
      if (E.C->sw_skip[D]) skip2Nx2N = predictSkip;
      if (D == 3 && predictSkip && E.C->depth_exception) skip2Nx2N = earlyTerminate = 0;
    }
  }
  if (!boundary) {
    FCU_FOR_LANES {                                          /* source block -> L2-resident CU buffer */
      for (int i = lane; i < s * s; i += 64) G->org[D].y[(i / s) * 64 + (i % s)] = E.C->org[0][(y + i / s) * E.C->stride[0] + x + (i % s)];
      const int h = s / 2;
      for (int i = lane; i < h * h; i += 64) {
        G->org[D].u[(i / h) * 32 + (i % h)] = E.C->org[1][(y / 2 + i / h) * E.C->stride[1] + x / 2 + (i % h)];
        G->org[D].v[(i / h) * 32 + (i % h)] = E.C->org[2][(y / 2 + i / h) * E.C->stride[2] + x / 2 + (i % h)];
      }
    }
    cu_init(cu_temp(E, D), D, x, y, zidx);
    int tryIntra = 1;
    if (P.slice_type == SLICE_P) {                           /* inter candidates first (TEncCu.cpp:753-943; ESD / CFM off) */
      FCU_FOR_LANES { if (lane < MEMO_K) G->memo_valid[D][lane] = 0; if (lane == MEMO_K) G->memo_next[D] = 0; }
      { FCU_TIC(p_); check_rd_cost_merge_2nx2n(D); FCU_ITOC(E, p_, 0); }
      cu_init(cu_temp(E, D), D, x, y, zidx);
      { FCU_TIC(p_); check_rd_cost_inter(D, SIZE_2Nx2N, 0); FCU_ITOC(E, p_, 1); } cu_init(cu_temp(E, D), D, x, y, zidx);
      { FCU_TIC(p_); check_rd_cost_inter(D, SIZE_Nx2N, 0); FCU_ITOC(E, p_, 2); } cu_init(cu_temp(E, D), D, x, y, zidx);
      { FCU_TIC(p_); check_rd_cost_inter(D, SIZE_2NxN, 0); FCU_ITOC(E, p_, 3); } cu_init(cu_temp(E, D), D, x, y, zidx);
      if (P.amp && D < MAXDEPTH) {                             /* AMP with AMP_ENC_SPEEDUP + AMP_MRG (:836-943); deriveTestModeAMP (:381-430) */
        const CuObj *bb = cu_best(E, D);
        const int bps = FCU_UNI((int)bb->part_size[0]), bmrg = FCU_UNI((int)bb->merge_flag[0]), bskip = FCU_UNI((int)bb->skip[0]), par = FCU_UNI(G->par_ps[D]);
        int hor = 0, ver = 0, mhor = 0, mver = 0;
        if (bps == SIZE_2NxN) hor = 1;
        else if (bps == SIZE_Nx2N) ver = 1;
        else if (bps == SIZE_2Nx2N && !bmrg && !bskip) hor = ver = 1;
        if (par >= SIZE_2NxnU && par <= SIZE_nRx2N) mhor = mver = 1;
        if (par == SIZE_NONE) { if (bps == SIZE_2NxN) mhor = 1; else if (bps == SIZE_Nx2N) mver = 1; }
        if (bps == SIZE_2Nx2N && !bskip) mhor = mver = 1;
        if (s == 64) hor = ver = 0;
        if (hor || mhor) {
          check_rd_cost_inter(D, SIZE_2NxnU, !hor); cu_init(cu_temp(E, D), D, x, y, zidx);
          check_rd_cost_inter(D, SIZE_2NxnD, !hor); cu_init(cu_temp(E, D), D, x, y, zidx);
        }
        if (ver || mver) {
          check_rd_cost_inter(D, SIZE_nLx2N, !ver); cu_init(cu_temp(E, D), D, x, y, zidx);
          check_rd_cost_inter(D, SIZE_nRx2N, !ver); cu_init(cu_temp(E, D), D, x, y, zidx);
        }
      }
      const CuObj *b = cu_best(E, D);                          /* intra only when the best inter candidate has a residual (:1033-1036) */
      tryIntra = FCU_UNI((int)(b->cbf[0][0] | b->cbf[1][0] | b->cbf[2][0])) != 0;
    }
    { FCU_TIC(p_); if (!skip2Nx2N && tryIntra) check_rd_cost_intra(D, SIZE_2Nx2N);      /* :1040; skipped => the best cost stays MAX_DOUBLE (:1077) */
      FCU_ITOC(E, p_, 4); }
    cu_init(cu_temp(E, D), D, x, y, zidx);
    if (D == MAXDEPTH && !earlyTerminate && tryIntra) {      /* :1141-1143 */
      FCU_SERIAL { g_S.dec_j0 = cu_best(E, D)->cost; g_S.dec_flip = g_S.best_idx[D]; }
      check_rd_cost_intra(D, SIZE_NxN);
      FCU_SERIAL { g_S.dec_flip ^= g_S.best_idx[D]; g_S.dec_j1 = g_S.dec_flip ? cu_best(E, D)->cost : cu_temp(E, D)->cost; }   /* :1175-1183 */
      cu_init(cu_temp(E, D), D, x, y, zidx);
      nxnTried = 1;
    } else if (D == MAXDEPTH && (state == DEC_VERIFYING || FCU_UNI(E.C->cu_trace) != nullptr)) {    /* NxN not tried (a P CU whose best inter candidate has no residual; Testing: TerminateCU): */
      FCU_SERIAL { g_S.dec_j0 = cu_best(E, D)->cost; g_S.dec_j1 = 0; g_S.dec_flip = 0; }      /* J1 0, bPartition_True false, not what the CU before left */
    }
    FCU_SERIAL {
      CuObj *best = cu_best(E, D);
      if (best->cost != FCU_MAX_DOUBLE) {                   /* fork: TEncCu.cpp:1224 */
        cab_reset_bits((CAB_GOON));
        code_split_flag(E, (CAB_GOON), best, 0, D);
        best->bits += cab_bits((CAB_GOON)); best->bins += g_S.cab[CAB_GOON].bins;
        best->cost = rd_cost(P, best->bits, best->dist);
      }
    }
  }
  cu_init(cu_temp(E, D), D, x, y, zidx);
  if constexpr (D < MAXDEPTH) {
   if (!earlyTerminate) {                                    /* bSubBranch = false, TEncCu.cpp:1257-1260 */
    const int nd = D + 1, hs = s >> 1, qn = NPART >> (2 * nd);
    if (P.amp) FCU_SERIAL { const CuObj *b = cu_best(E, D); G->par_ps[nd] = (boundary || b->pred_mode[0] != MODE_INTER) ? SIZE_NONE : b->part_size[0]; }   /* eParentPartSize, :1355-1363 */
    for (int i = 0; i < 4; i++) {
      const int sx = x + (i & 1) * hs, sy = y + (i >> 1) * hs;
      cu_init(&G->cu[nd][0], nd, sx, sy, zidx + i * qn);
      cu_init(&G->cu[nd][1], nd, sx, sy, zidx + i * qn);
      if (sx < P.width && sy < P.height) {
        FCU_FOR_LANES cab_copy(slot_ptr(E, nd, CI_CURR_BEST), i == 0 ? slot_ptr(E, D, CI_CURR_BEST) : slot_ptr(E, nd, CI_NEXT_BEST), lane);
        { FCU_DTIC(dc_); compress_cu<D + 1>(); FCU_DADD(E, dc_, 11 + D, -1); }   /* the child's time is not this depth's */
        cu_copy_part_from(cu_temp(E, D), cu_best(E, nd), i);
        {                                                    /* xCopyYuv2Tmp */
          const Yuv *src = &G->reco[nd][g_S.reco_best_idx[nd]]; Yuv *dst = &G->reco[D][1 - g_S.reco_best_idx[D]];
          FCU_FOR_LANES {
            for (int k = lane; k < hs * hs; k += 64) dst->y[((i >> 1) * hs + k / hs) * 64 + (i & 1) * hs + k % hs] = src->y[(k / hs) * 64 + k % hs];
            const int h = hs / 2;
            for (int k = lane; k < h * h; k += 64) { const int o = ((i >> 1) * h + k / h) * 32 + (i & 1) * h + k % h; dst->u[o] = src->u[(k / h) * 32 + k % h]; dst->v[o] = src->v[(k / h) * 32 + k % h]; }
          }
        }
      } else {
        cu_copy_to_pic(cu_best(E, nd));
        cu_copy_part_from(cu_temp(E, D), cu_best(E, nd), i);
      }
    }
    FCU_SERIAL {
      CuObj *t = cu_temp(E, D);
      if (!boundary) { cab_reset_bits((CAB_GOON)); code_split_flag(E, (CAB_GOON), t, 0, D); t->bits += cab_bits((CAB_GOON)); t->bins += g_S.cab[CAB_GOON].bins; }
      t->cost = rd_cost(P, t->bits, t->dist);
      if (skip2Nx2N) cu_best(E, D)->cost = FCU_MAX_DOUBLE;   /* :1446-1449 */
      g_S.dec_j0 = cu_best(E, D)->cost; g_S.dec_j1 = t->cost; g_S.dec_flip = g_S.best_idx[D];   /* J0, J1 :1450-1451 */
    }
    FCU_FOR_LANES cab_copy(slot_ptr(E, D, CI_TEMP_BEST), slot_ptr(E, nd, CI_NEXT_BEST), lane);
    check_best_mode(D);
    FCU_SERIAL g_S.dec_flip ^= g_S.best_idx[D];              /* bPartition_True = xCheckBestMode(...) */
   }
  }
  if (!boundary && state == DEC_VERIFYING && predictSkip >= 0) {      /* TEncCu.cpp:1489-1497 */
    FCU_SERIAL count_verify(E.C, D, predictSkip, g_S.dec_flip, g_S.dec_j0, g_S.dec_j1);
  }
  /* fcu_cu_trace of this CU: the numbers count_verify takes, in every state (the pointer is read here, not kept across the
   * sub-CUs: with no trace bound the cost is this wave-uniform branch) */
  fcu_cu_trace *const trace = boundary ? (fcu_cu_trace *)nullptr : FCU_UNI(E.C->cu_trace);
  if (trace) {
    const int splitTried = D < MAXDEPTH ? !earlyTerminate : nxnTried;      /* the four sub-CUs were searched / SIZE_NxN was tried */
    FCU_SERIAL {
      FCU_HBM fcu_cu_trace *r = (FCU_HBM fcu_cu_trace *)trace + (size_t)E.cur_ctu * FCU_CUS_PER_CTU + pu_trace_index(D, 0, zidx);
      /* a CU that was not divided (D < 3, Testing: TerminateCU) never set dec_j0: its whole-CU cost with the split flag is the best cost */
      const double j0 = (splitTried || D == MAXDEPTH) ? g_S.dec_j0 : cu_best(E, D)->cost;
      r->j0 = j0; r->j1 = splitTried ? g_S.dec_j1 : 0.0;
      r->valid = 1; r->split_won = (uint8_t)(splitTried && g_S.dec_flip); r->whole_tried = (uint8_t)(j0 != FCU_MAX_DOUBLE); r->split_tried = (uint8_t)splitTried;
    }
  }
  cu_copy_to_pic(cu_best(E, D));
  copy_reco_to_pic(&G->reco[D][g_S.reco_best_idx[D]], x, y, s);
  FCU_DADD(E, dt_, 11 + D, 1);
}

/* ---- encodeCtu replay: xEncodeCU, TEncCu.cpp:1679-1778 (serial, iterative) --------------- */
FCU_DEV FCU_NOINLINE void encode_ctu(int c, const CuObj *ctu, int lastCtuOfSlice)
{
  const Env E = env_get(); c = FCU_UNI(c); ctu = FCU_UNI(ctu); lastCtuOfSlice = FCU_UNI(lastCtuOfSlice);
  const Params &P = E.C->p;
  int *stPart = g_S.wk_part, *stChild = g_S.wk_child; int sp = 0;
  stPart[0] = 0; stChild[0] = -1;
  while (sp >= 0) {
    const int depth = sp, part = stPart[sp];
    if (stChild[sp] < 0) {
      const int cx = ctu->x + part_x(part), cy = ctu->y + part_y(part), s = CTU >> depth;
      int boundary = 0;
      if (cx + s - 1 < P.width && cy + s - 1 < P.height) code_split_flag(E, c, ctu, part, depth); else boundary = 1;
      if (!((depth < ctu->depth[part] && depth < MAXDEPTH) || boundary)) {
        encode_cu_syntax(E, c, ctu, part, depth);
        const int rx = cx + s, ry = cy + s;                  /* finishCU / isLastSubCUOfCtu, TEncCu.cpp:1629-1645 */
        if (((rx % CTU) == 0 || rx == P.width) && ((ry % CTU) == 0 || ry == P.height) && !lastCtuOfSlice) cab_trm(c, 0);
        sp--; continue;
      }
      stChild[sp] = 0;
    }
    if (stChild[sp] >= 4) { sp--; continue; }
    {
      const int qn = (NPART >> (2 * depth)) >> 2, p = part + stChild[sp] * qn;
      stChild[sp]++;
      if (ctu->x + part_x(p) < P.width && ctu->y + part_y(p) < P.height) { sp++; stPart[sp] = p; stChild[sp] = -1; }
    }
  }
}

/* cooperative fill of the LDS table mirror; called once per kernel launch */
FCU_DEV void load_hot_tables()
{
  FCU_FOR_LANES {
    for (int i = lane; i < 256; i += 64) g_hot.bin[i] = k_bin[i];
    for (int i = lane; i < 3 * 16; i += 64) { const int t = i / 16, j = i % 16; g_hot.scan[t][j] = k_scan[k_scan_off[t * 4 + 0] + j]; }
    if (lane < 12) g_hot.scan_cg8[lane / 4][lane % 4] = k_scan_cg[k_scan_cg_off[(lane / 4) * 4 + 1] + lane % 4];
    if (lane < 16) g_hot.ctx_ind_map4x4[lane] = k_ctx_ind_map4x4[lane];
    if (lane < 32) g_hot.group_idx[lane] = k_group_idx[lane];
    if (lane < 3) { uint64_t v = 0; for (int j = 0; j < 16; j++) v |= (uint64_t)k_scan[k_scan_off[lane * 4 + 0] + j] << (4 * j); g_hot.scan4_nib[lane] = v; }
    if (lane == 3) { uint64_t v = 0; for (int j = 0; j < 16; j++) v |= (uint64_t)k_ctx_ind_map4x4[j] << (4 * j); g_hot.map4_nib = v; }
    if (lane >= 4 && lane < 8) {                               /* getSigCtxInc's cnt per pattern and 4x4 raster position (TComTrQuant.cpp:2650-2690) */
      const int pattern = lane - 4; uint32_t v = 0;
      for (int j = 0; j < 16; j++) {
        const int xs = j & 3, ys = j >> 2; int cnt;
        if (pattern == 0) { const int t = xs + ys; cnt = (t >= 3) ? 0 : ((t >= 1) ? 1 : 2); }
        else if (pattern == 1) cnt = (ys >= 2) ? 0 : ((ys >= 1) ? 1 : 2);
        else if (pattern == 2) cnt = (xs >= 2) ? 0 : ((xs >= 1) ? 1 : 2);
        else cnt = 2;
        v |= (uint32_t)cnt << (2 * j);
      }
      g_hot.cnt_bits[pattern] = v;
    }
  }
}

/* ---- one CTU of one chain: the loop body of TEncSlice::compressSlice, TEncSlice.cpp:1380-1551.
 * WPP = a WaveFrontSynchro row chain (Chain::wpp): the first CTU of a row that does not start a slice restarts the coder (resetEntropy) and,
 * when the picture is at least two CTUs wide, takes the contexts saved after the second CTU of the row above (loadContexts of
 * m_entropyCodingSyncContextState, TEncSlice.cpp:1396-1411: contexts only, the Q15 counter stays as the reset leaves it); after
 * the second CTU of its own row it saves its contexts for the row below (:1514-1517).  A row that starts a slice (slices of whole
 * rows, fcu_wpp_begin_slices) is the first CTU of its slice: the slice's reset alone, row_start false, wpp_sync_in never read
 * (CUIsFromSameSliceAndTile(pCtuTR) fails at :1400, nothing is loaded); its above neighbours are masked by E.slice_start.  Every
 * row saves after its second CTU, whether or not a row of its slice follows.  WPP = false is the plain chain.
 * Tiles (fcu_tiles_begin / fcu_wpp_begin_tiles; one slice per picture): `pos` counts CTUs inside the chain's tile, raster-in-tile,
 * and the CTU's picture address follows from it; without tiles the tile is the picture and both are the same number.  The first
 * CTU of a tile resets the coder as the first CTU of a slice does (:1392-1395); "first column" and "second column" of the
 * WaveFrontSynchro rules are those of the tile (tileXPosInCtus, :1396 and :1514), and a one-CTU-wide tile loads nothing (its
 * above-right CTU is in another tile: CUIsFromSameSliceAndTile fails).  end_of_slice_segment_flag is 1 at the picture's last CTU
 * in tile-scan order only -- the last CTU of the last tile, which is the CTU at the picture's last address; the last CTU of any
 * other tile codes a 0 there (its substream ends with it, :1718-1727, which touches no context). */
template <bool WPP = false>
FCU_DEV FCU_NOINLINE void compress_ctu(Chain *C, Scratch *G, int pos)
{
  C = FCU_UNI(C); G = FCU_UNI(G); pos = FCU_UNI(pos);
  Env E; E.C = C; E.G = G;
#ifdef FCU_EMU
  g_emu_lscan_lo = G->p_lscan; g_emu_lscan_hi = G->p_lscan + POOL;
#endif
  FCU_TIC(t10_);
  const Params &P = C->p;
  const int tileW = FCU_UNI(C->tile_w), tileX0 = FCU_UNI(C->tile_x0), tileY0 = FCU_UNI(C->tile_y0);
  const int col = pos % tileW;                                /* column inside the tile */
  const int ctuRsAddr = FCU_UNI((tileY0 + pos / tileW) * C->w_ctu + tileX0 + col);
  E.tx0 = (int16_t)tileX0; E.ty0 = (int16_t)tileY0; E.tx1 = (int16_t)(tileX0 + tileW); E.ty1 = (int16_t)(tileY0 + FCU_UNI(C->tile_h));
  const int sliceLen = P.slice_ctus > 0 ? P.slice_ctus : C->n_ctu;
  const int sliceStart = (ctuRsAddr / sliceLen) * sliceLen;
  int sliceEnd = sliceStart + sliceLen; if (sliceEnd > C->n_ctu) sliceEnd = C->n_ctu;
  E.cur_ctu = ctuRsAddr; E.slice_start = sliceStart;
  fcu_ctu_out *out = &C->out[ctuRsAddr];
  const int x = (ctuRsAddr % C->w_ctu) * CTU, y = (ctuRsAddr / C->w_ctu) * CTU;
  const bool unit_start = ctuRsAddr == sliceStart || pos == 0;      /* first CTU of a slice or of a tile */
  const bool row_start = WPP && col == 0 && !unit_start;
  FCU_SERIAL { g_S.env = E; g_S.ref_tag = -1; if (unit_start || row_start) cab_init(slot_ptr(E, 0, CI_CURR_BEST), P.qp, P.slice_type, P.cabac_b_table); else cab_copy1(slot_ptr(E, 0, CI_CURR_BEST), &C->state); }
  if (row_start && tileW >= 2) {
    const uint8_t *src = C->wpp_sync_in;
    FCU_FOR_LANES { Cabac *d = slot_ptr(E, 0, CI_CURR_BEST); for (int i = lane; i < NCTX; i += 64) d->ctx[i] = src[i]; }   /* lane-indexed: vector loads */
  }
  FCU_FOR_LANES {                                            /* TComDataCU::initCtu defaults, TComDataCU.cpp:474-560 */
    for (int i = lane; i < NPART; i += 64) {
      out->depth[i] = 0; out->width[i] = CTU; out->height[i] = CTU; out->skip[i] = 0; out->part_size[i] = SIZE_NONE; out->pred_mode[i] = MODE_NONE;
      out->tq_bypass[i] = 0; out->qp[i] = (int8_t)P.qp; out->chroma_qp_adj[i] = 0; out->tr_idx[i] = 0; out->ipcm[i] = 0;
      out->merge_flag[i] = 0; out->merge_idx[i] = 0; out->inter_dir[i] = 0; out->mvp_idx[i] = -1; out->ref_idx[i] = -1;   /* clearMvField: NOT_VALID */
      out->mv[i][0] = out->mv[i][1] = 0; out->mvd[i][0] = out->mvd[i][1] = 0;
      for (int c = 0; c < 3; c++) { out->tskip[c][i] = 0; out->cbf[c][i] = 0; }
      out->intra_dir[0][i] = DC; out->intra_dir[1][i] = 0;
    }
    for (int i = lane; i < 4096; i += 64) out->coeff_y[i] = 0;
    for (int i = lane; i < 1024; i += 64) { out->coeff_cb[i] = 0; out->coeff_cr[i] = 0; }
    cab_copy(&g_S.cab[CAB_GOON], slot_ptr(E, 0, CI_CURR_BEST), lane);
    if (lane == 0) { for (int d = 0; d < 4; d++) { g_S.best_idx[d] = 0; g_S.reco_best_idx[d] = 0; } G->par_ps[0] = SIZE_NONE; out->total_cost = FCU_MAX_DOUBLE; out->total_dist = out->total_bits = out->total_bins = 0; }
  }
  if (FCU_UNI(C->cu_trace) != nullptr) {                     /* the CTU's 85 records start as "not visited": 2040 bytes, lanes striding */
    FCU_HBM uint32_t *w = (FCU_HBM uint32_t *)(C->cu_trace + (size_t)ctuRsAddr * FCU_CUS_PER_CTU);
    FCU_FOR_LANES { for (int i = lane; i < (int)(FCU_CUS_PER_CTU * sizeof(fcu_cu_trace) / 4); i += 64) w[i] = 0u; }
  }
  cu_init(&G->cu[0][0], 0, x, y, 0);
  cu_init(&G->cu[0][1], 0, x, y, 0);
  compress_cu<0>();
  /* encodeCtu on [0][CI_CURR_BEST] (TEncSlice.cpp:1474-1487): replay the winner to advance the contexts */
  {
    const CuObj *view = cu_best(E, 0);                     /* what copyToPic has just published (whole CTU) */
    FCU_FOR_LANES {
      cab_copy(&g_S.cab[CAB_GOON], slot_ptr(E, 0, CI_CURR_BEST), lane);
    }
    FCU_TIC(t9_);
    FCU_SERIAL {
      cab_reset_bits((CAB_GOON));
      encode_ctu((CAB_GOON), view, ctuRsAddr == sliceEnd - 1);
      cab_copy1(&C->state, &g_S.cab[CAB_GOON]);
    }
    FCU_TOC(E, t9_, 9);
    if (WPP && col == 1) {
      uint8_t *dst = C->wpp_sync_out;
      FCU_FOR_LANES { for (int i = lane; i < NCTX; i += 64) dst[i] = g_S.cab[CAB_GOON].ctx[i]; }
    }
  }
  FCU_TOC(E, t10_, 10);
}

/* ---- WaveFrontSynchro: one CTU row of a picture as a chain (TEncSlice.cpp:1386-1411,1514-1517) --------------------------
 * "The row above" below = the row above IN THE SAME SLICE.  A one-slice picture has one for every row but row 0; a picture cut
 * into slices of R whole rows (SliceMode 1 with WaveFrontSynchro, fcu_wpp_begin_slices) has none for rows 0, R, 2R, ...: those
 * are bound with wpp_above -1 and run like a row 0, so no chain ever waits on a chain of another slice, and the critical path of
 * W x H CTUs falls from W + 2(H - 1) to W + 2(R - 1) CTUs.
 * Row r may decide CTU x once row r-1 has finished CTU min(x + 1, W - 1): that completes every neighbour CTU x reads (left,
 * above-left, above, above-right) and, for x == 0, the sync slot written after CTU 1 of the row above.  The rows of a picture
 * hand these bytes (fcu_ctu_out entries, reconstruction rows, the sync slot) over through per-chain progress words:
 * ctl[WPP_CTL_WORDS + chain] = CTUs the chain has finished in this launch; ctl[0] = ticket counter, ctl[1] = abort word. */
enum { WPP_CTL_WORDS = 4, WPP_SYNC_BYTES = 192 };          /* sync slot: NCTX context bytes, padded */
#ifdef FCU_EMU
/* the emulator runs the chains one after the other in index order (row above first): a wait is a claim that holds already */
FCU_DEV bool wpp_wait(unsigned *ctl, int above, unsigned need) { FCU_CHECK(ctl[WPP_CTL_WORDS + above] >= need); return true; }
FCU_DEV void wpp_publish(unsigned *ctl, int chain, unsigned done) { ctl[WPP_CTL_WORDS + chain] = done; }
#else
/* 120 s of s_memrealtime (100 MHz): far beyond the longest wait of a healthy launch (a row waits at most for the rows above it to
 * advance two CTUs each) */
#define FCU_WPP_GIVE_UP_TICKS (120ull * 100000000ull)
/* consumer (cdna_hip_programming.md 6, Guideline 16): lane 0 polls the producer's word relaxed at agent scope, the value is made
 * wave-uniform, s_sleep between polls; ONE agent-scope acquire after the match, then plain (vector) loads.  Gives up -- and
 * raises the abort word that stops every other waiter -- after FCU_WPP_GIVE_UP_TICKS or when another wave has aborted. */
FCU_DEV bool wpp_wait(unsigned *ctl_, int above, unsigned need)
{
  FCU_HBM unsigned *ctl = (FCU_HBM unsigned *)ctl_;
  const unsigned long long t0 = __builtin_amdgcn_s_memrealtime();
  for (;;) {
    unsigned v = 0, ab = 0;
    if (threadIdx.x == 0) {
      v = __hip_atomic_load(ctl + WPP_CTL_WORDS + above, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      ab = __hip_atomic_load(ctl + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    v = (unsigned)__builtin_amdgcn_readfirstlane((int)v); ab = (unsigned)__builtin_amdgcn_readfirstlane((int)ab);
    if (ab != 0) return false;
    if (v >= need) break;
    if (__builtin_amdgcn_s_memrealtime() - t0 > FCU_WPP_GIVE_UP_TICKS) {
      if (threadIdx.x == 0) __hip_atomic_store(ctl + 1, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      return false;
    }
    __builtin_amdgcn_s_sleep(8);
  }
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
  return true;
}
/* producer: drain this wave's stores of the CTU (its fcu_ctu_out entry, reconstruction, sync slot), agent-scope release, drain
 * again (the fence's own wait may be dropped: Guideline 16 Pitfall 12), then lane 0 stores the progress word atomically */
FCU_DEV void wpp_publish(unsigned *ctl_, int chain, unsigned done)
{
  FCU_HBM unsigned *ctl = (FCU_HBM unsigned *)ctl_;
  asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  if (threadIdx.x == 0) __hip_atomic_store(ctl + WPP_CTL_WORDS + chain, done, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
#endif
/* ---- P slices: m_integerMv2Nx2N across rows.  HM walks the CTUs of a WPP picture in raster order, so the TZ start vectors
 * (int_mv_r, TEncSearch.cpp:3833-3842) a row begins with are the ones the row above ended with.  They are read only by a TZ
 * search that is not the depth-0 2Nx2N one (:3833-3837) and written after every 2Nx2N TZ search (:3839-3842).  A CTU that holds
 * a 64x64 CU always runs that depth-0 2Nx2N search on every reference index in order first (merge 2Nx2N, then inter 2Nx2N:
 * TEncCu.cpp:774-780, oracle/hmo_search.c:851-864), so a row whose first CTU is full writes slots [0, n_ref) before it reads
 * any, and only a row that begins on a boundary CTU (the partial bottom row, a picture narrower than 64) reads what the row
 * above left.  Hence, under TZ search (slots >= n_ref, and all of them under full search, are never written):
 *   - a row below the first whose first CTU is a boundary CTU waits for the whole row above and takes all its slots first;
 *   - every row below the first, at its end, takes from the row above the slots it did not write (rule: the row wrote
 *     [0, n_ref) iff TZ search and a full first CTU; a boundary-first row already holds every slot), so each row chain ends
 *     with HM's state after its row, the last one with HM's state after the picture.
 * The row above is finished when either copy happens (progress W, waited for before the first / the last CTU); its own end copy
 * precedes its last publish.  Lane-indexed loads (vector memory, never the scalar cache: Guideline 16 Pitfall 6).
 * Slices of whole rows: "the first row" reads "the first row of the slice" throughout.  A row that starts a slice takes nothing
 * from the chain before it, at its start or at its end: it begins from its own descriptor (zero after binding: the convention
 * for slices decided side by side), so the last row chain of a slice ends with the state after that slice.
 * Tiles: the same with "tile" for "slice" -- the first row of every tile starts from its own descriptor (zero after binding; HM's
 * tile-scan walk would carry the state from the tile before), and the last row chain of a tile ends with the state after it. */
FCU_DEV void wpp_take_search_state(Chain *C, const Chain *A, int first, int end)
{
  FCU_FOR_LANES {
    if (lane >= 2 * first && lane < 2 * end) {
      const int v = ((const FCU_HBM int *)&A->int_mv_r[0][0])[lane];
      ((FCU_HBM int *)&C->int_mv_r[0][0])[lane] = v;
    }
  }
#ifdef FCU_EMU
  C->wpp_mv_known |= ((1 << end) - 1) & ~((1 << first) - 1);
#endif
}
/* one WPP row chain (`chain` = its index, the one its progress word is kept under) decided to the end of its row; 0 = gave up */
FCU_DEV FCU_NOINLINE int run_wpp_chain(Chain *C, Scratch *G, unsigned *ctl, int chain)
{
  C = FCU_UNI(C); G = FCU_UNI(G); ctl = FCU_UNI(ctl); chain = FCU_UNI(chain);
  load_hot_tables();
  /* W, and x below: the width of the chain's tile and the column inside it (the picture's without tiles); first / end count CTUs
   * inside the tile.  A row waits for min(x + 2, W) CTUs of the row above IN ITS TILE and for nothing of another tile. */
  const int above = FCU_UNI(C->wpp_above), W = FCU_UNI(C->tile_w), end = FCU_UNI(C->end_ctu);
  const int first = FCU_UNI(C->next_ctu);
  /* P row below the first of its slice: the row above's descriptor (rows of a picture are consecutive chains) and the hand-off rule above */
  const bool inherit = above >= 0 && C->p.slice_type == SLICE_P;
  const Chain *A = C + (above - chain);
  const bool tz = C->p.fast_search != 0, full_first = (FCU_UNI(C->tile_x0) + 1) * CTU <= C->p.width && (FCU_UNI(C->tile_y0) + first / W + 1) * CTU <= C->p.height;
#ifdef FCU_EMU
  if (above >= 0) C->wpp_mv_known = 0;                       /* (a row that starts a slice keeps what its binder declared known) */
#endif
  if (inherit && tz && !full_first && first < end) {
    if (!wpp_wait(ctl, above, (unsigned)W)) return 0;
    wpp_take_search_state(C, A, 0, FCU_MAX_REF);
  }
  for (int a = first; a < end; a++) {
    const int x = a % W;
    if (above >= 0 && !wpp_wait(ctl, above, (unsigned)(x + 2 < W ? x + 2 : W))) return 0;
    compress_ctu<true>(C, G, a);
    FCU_SERIAL { C->next_ctu = a + 1; }
    if (inherit && a + 1 == end && (!tz || full_first)) wpp_take_search_state(C, A, tz ? FCU_UNI(C->n_ref) : 0, FCU_MAX_REF);
    wpp_publish(ctl, chain, (unsigned)(x + 1));
  }
  return 1;
}

} // namespace fcu
