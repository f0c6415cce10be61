/*
 * fcu_report.h -- the per-picture report line of the encoder on the device: SSD per plane (-> PSNR), bits / bins / distortion
 * and CU statistics of decided (and filtered) pictures (TEncGOP::xCalculateAddPSNR, Lib/TLibEncoder/TEncGOP.cpp:2195-2290;
 * the PSNR expression itself, :2254-2256, is evaluated on the host from the sums -- no libm on the device).
 * Included by fcu_kernels.hip only (and by the test-only CPU build tests/emu/report_emu.cpp).
 *
 * Two launches per batch of pictures, no atomics, no memory that must be zero beforehand; every byte of both records is
 * written by exactly one thread, so a repeated call gives identical bytes:
 *   report_ctu   one 256-thread workgroup per (CTU, picture) -> one fcu_ctu_report (64 B).
 *                Samples: every thread reads a few units of a row of org and rec.  Two load paths, chosen by the host per batch
 *                (report_wide_ok): WIDE = 16 B of a luma row, 8 B of a chroma row, when every plane pointer is 16-byte aligned
 *                and the width a multiple of 16; otherwise 4 B units through byte-exact copies, right for any base address and
 *                any width fcu_create accepts (partial CTUs end on multiples of 8 luma / 4 chroma samples).  All loads of a
 *                thread are issued before the first use.  Squared differences sum in 32 bits per thread and per CTU:
 *                4096 * 255^2 = 266 342 400 < 2^32.
 *                Partitions: thread z looks at 4x4 partition z (z-order) of the CTU's fcu_ctu_out head -- eight 256-byte arrays,
 *                each read as one coalesced 256-byte row.  Inside / outside the picture is geometry (k_z2r), never what the
 *                engine left in unused entries.  Every counter is one wave ballot + popcount (scalar).
 *                The four waves meet in 4 x 22 words of LDS; threads 0..15 then store one dword of the record each.
 *   report_pic   one 256-thread workgroup per picture: sums the picture's CTU records into one fcu_pic_report.  Thread t reads
 *                dword (t & 15) of records (t >> 4), (t >> 4) + 16, ... (coalesced: 16 consecutive records per instruction,
 *                REP_PIC_AHEAD loads in flight) and keeps the dword's 64-bit sum and the 32-bit sums of its two halves; 16 partial sums per dword meet in LDS.
 *                64-bit: the luma SSD of a picture passes 2^32 from 66 050 samples of error 255 on, the bit sum may as well.
 * Algorithmic bytes per picture: 2 x 1.5 W H (org + rec) + 2 060 B of every fcu_ctu_out head and tail + 64 B per CTU record
 * written and read back.
 */
#pragma once

namespace fcu {

enum { REP_THREADS = 256, REP_COUNTERS = 19,               /* n_part, depth[4], part_size[8], intra, skip, merge, cbf[3] */
       REP_SLOTS = 3 + REP_COUNTERS,                       /* per wave: SSD Y, U, V, then the counters */
       REP_CTU_WORDS = 16, REP_PIC_CNT_WORD = 18, REP_PIC_PSNR_QWORD = 19, REP_PIC_AHEAD = 8 };
static_assert(sizeof(fcu_ctu_report) == 4 * REP_CTU_WORDS && sizeof(fcu_pic_report) == 8 * (REP_PIC_PSNR_QWORD + 3), "record layouts the word-wise stores rely on");

struct ReportPic { const uint8_t *org[3], *rec[3]; const fcu_ctu_out *out; };     /* one picture of a batch (device copy) */

/* host: may the batch take the wider loads?  They need every row of every plane on the unit's alignment: planes that start on
 * 16 bytes and a width that is a multiple of 16 (luma rows and units of 16 B, chroma rows and units of 8 B; a partial CTU then
 * ends on a unit) */
inline bool report_wide_ok(int width, const ReportPic *pics, int n_pics)
{
  bool ok = (width & 15) == 0;
  for (int i = 0; i < n_pics; i++) for (int k = 0; k < 3; k++) ok = ok && (((uintptr_t)pics[i].org[k] | (uintptr_t)pics[i].rec[k]) & 15) == 0;
  return ok;
}

/* sum of squared differences of N bytes at o and r, each known to be ALIGN-aligned (1: nothing is known) */
template <int N>
struct ReportUnit { uint32_t o[N / 4], r[N / 4]; };
template <int N, int ALIGN>
__device__ static inline void report_load(ReportUnit<N> &u, const uint8_t *o, const uint8_t *r)
{
  /* (planes are HBM: global_ instead of flat_ loads) */
  __builtin_memcpy(u.o, (const FCU_HBM uint8_t *)__builtin_assume_aligned(o, ALIGN), N);
  __builtin_memcpy(u.r, (const FCU_HBM uint8_t *)__builtin_assume_aligned(r, ALIGN), N);
}
template <int N>
__device__ static inline uint32_t report_ssd(const ReportUnit<N> &u)
{
  uint32_t s = 0;
#pragma unroll
  for (int k = 0; k < N; k++) {
    const int d = (int)((u.o[k >> 2] >> (8 * (k & 3))) & 255u) - (int)((u.r[k >> 2] >> (8 * (k & 3))) & 255u);
    s += (uint32_t)(d * d);
  }
  return s;
}
/* SSD of this thread's units of one plane of the CTU: the plane's CTU block is SIDE x SIDE samples (64 luma, 32 chroma) of which
 * bw x bh lie inside the picture (bw a multiple of N), dealt as units of N bytes of a row to NT threads (t < NT).  The trip
 * count is a constant: the loads of all units are issued first, the arithmetic follows. */
template <int N, int ALIGN, int SIDE, int NT>
__device__ static inline uint32_t report_plane_ssd(const uint8_t *org, const uint8_t *rec, int stride, int bw, int bh, int t)
{
  enum { UPR = SIDE / N, ITERS = UPR * SIDE / NT };
  static_assert(ITERS >= 1 && UPR * SIDE % NT == 0, "whole rounds");
  ReportUnit<N> u[ITERS];
  bool in[ITERS];
#pragma unroll
  for (int k = 0; k < ITERS; k++) {
    const int i = t + k * NT, y = i / UPR, x = (i % UPR) * N;
    in[k] = x < bw && y < bh;
    const size_t o = (size_t)y * stride + x;
    if (in[k]) report_load<N, ALIGN>(u[k], org + o, rec + o);
  }
  uint32_t s = 0;
#pragma unroll
  for (int k = 0; k < ITERS; k++) if (in[k]) s += report_ssd<N>(u[k]);
  return s;
}

/* a per-lane value summed / a per-lane flag counted over the wave into the wave's LDS word.  All 64 lanes call them, outside
 * divergent code.  The CPU build runs the lanes one after the other into a word its driver cleared. */
__device__ static inline void report_wave_add(uint32_t *slot, uint32_t v)
{
#ifdef FCU_EMU
  *slot += v;
#else
  const uint32_t s = fcu_wave_sum(v);
  if ((threadIdx.x & 63) == 0) *slot = s;
#endif
}
__device__ static inline void report_wave_count(uint32_t *slot, bool flag)
{
#ifdef FCU_EMU
  *slot += flag ? 1u : 0u;
#else
  const uint32_t n = (uint32_t)__popcll(__ballot(flag));    /* s_bcnt1_i32_b64 of the compare mask */
  if ((threadIdx.x & 63) == 0) *slot = n;
#endif
}

/* ---- report_ctu: phase 1 fills the four waves' slots, phase 2 stores the record ---------------------------------------- */
template <int PHASE, bool WIDE>
__device__ static inline void report_ctu_phase(uint32_t (*part)[REP_SLOTS], const ReportPic *pics, fcu_ctu_report *ctu, int width, int height, int w_ctu, int n_ctu)
{
  const int t = (int)threadIdx.x, a = (int)blockIdx.x, pic = (int)blockIdx.y;
  const ReportPic &P = pics[pic];
  const FCU_HBM fcu_ctu_out &O = *(const FCU_HBM fcu_ctu_out *)(P.out + a);
  if (PHASE == 1) {
    uint32_t *W = part[t >> 6];
    const int cx = a % w_ctu, cy = a / w_ctu, x0 = cx * 64, y0 = cy * 64;
    const int bw = x0 + 64 > width ? width - x0 : 64, bh = y0 + 64 > height ? height - y0 : 64, sc = width >> 1;
    const size_t oy = (size_t)y0 * width + x0, oc = (size_t)(y0 >> 1) * sc + (x0 >> 1);
    uint32_t sy, su, sv;
    if (WIDE) {                                               /* waves 0, 1: Cb; waves 2, 3: Cr (wave-uniform) */
      sy = report_plane_ssd<16, 16, 64, REP_THREADS>(P.org[0] + oy, P.rec[0] + oy, width, bw, bh, t);
      const int c = 1 + (t >> 7);
      const uint32_t s = report_plane_ssd<8, 8, 32, REP_THREADS / 2>(P.org[c] + oc, P.rec[c] + oc, sc, bw >> 1, bh >> 1, t & 127);
      su = c == 1 ? s : 0u; sv = c == 2 ? s : 0u;
    } else {
      sy = report_plane_ssd<4, 1, 64, REP_THREADS>(P.org[0] + oy, P.rec[0] + oy, width, bw, bh, t);
      su = report_plane_ssd<4, 1, 32, REP_THREADS>(P.org[1] + oc, P.rec[1] + oc, sc, bw >> 1, bh >> 1, t);
      sv = report_plane_ssd<4, 1, 32, REP_THREADS>(P.org[2] + oc, P.rec[2] + oc, sc, bw >> 1, bh >> 1, t);
    }
    report_wave_add(&W[0], sy); report_wave_add(&W[1], su); report_wave_add(&W[2], sv);
    /* 4x4 partition t (z-order) of the CTU */
    const int r = k_z2r[t];
    const bool in = x0 + 4 * (r & 15) < width && y0 + 4 * (r >> 4) < height;
    const int depth = O.depth[t], ps = O.part_size[t], pm = O.pred_mode[t];
    const int skip = O.skip[t], mrg = O.merge_flag[t], c0 = O.cbf[0][t], c1 = O.cbf[1][t], c2 = O.cbf[2][t];
    uint32_t *K = W + 3;
    report_wave_count(&K[0], in);
#pragma unroll
    for (int d = 0; d < 4; d++) report_wave_count(&K[1 + d], in && depth == d);
#pragma unroll
    for (int s = 0; s < 8; s++) report_wave_count(&K[5 + s], in && ps == s);
    report_wave_count(&K[13], in && pm == 1);
    report_wave_count(&K[14], in && skip != 0);
    report_wave_count(&K[15], in && mrg != 0);
    report_wave_count(&K[16], in && (c0 & 1));
    report_wave_count(&K[17], in && (c1 & 1));
    report_wave_count(&K[18], in && (c2 & 1));
  } else if (t < REP_CTU_WORDS) {
    /* dword t of the record: 0..2 ssd[3]; 3..5 bits, bins, dist; 6..15 the counters in pairs (the last half-word is `pad`) */
    uint32_t w;
    if (t >= 3 && t < 6) w = t == 3 ? O.total_bits : (t == 4 ? O.total_bins : O.total_dist);
    else {
      const int k0 = t < 3 ? t : 3 + 2 * (t - 6), k1 = k0 + 1;
      w = part[0][k0] + part[1][k0] + part[2][k0] + part[3][k0];
      if (t >= 6 && k1 < REP_SLOTS) w |= (part[0][k1] + part[1][k1] + part[2][k1] + part[3][k1]) << 16;
    }
    ((uint32_t *)(ctu + (size_t)pic * n_ctu + a))[t] = w;
  }
}

/* ---- report_pic: phase 1 leaves every thread's partial sums in LDS, phase 2 stores the record -------------------------- */
struct ReportPicLds { uint64_t full[REP_THREADS]; uint32_t lo[REP_THREADS], hi[REP_THREADS]; };
template <int PHASE>
__device__ static inline void report_pic_phase(ReportPicLds &L, const fcu_ctu_report *ctu, fcu_pic_report *rep, int width, int height, int n_ctu)
{
  const int t = (int)threadIdx.x, pic = (int)blockIdx.x;
  if (PHASE == 1) {
    const uint32_t *w = (const uint32_t *)(ctu + (size_t)pic * n_ctu) + (t & 15);
    uint64_t full = 0; uint32_t lo = 0, hi = 0;              /* halves: <= 256 per record, 2^24 records before 32 bits fill */
    /* REP_PIC_AHEAD loads in flight per thread: one workgroup walks the whole picture, so the latency of a load must not be paid per record */
    for (int r0 = t >> 4; r0 < n_ctu; r0 += REP_PIC_AHEAD * (REP_THREADS / 16)) {
      uint32_t v[REP_PIC_AHEAD];
#pragma unroll
      for (int k = 0; k < REP_PIC_AHEAD; k++) { const int r = r0 + k * (REP_THREADS / 16); v[k] = r < n_ctu ? w[(size_t)r * REP_CTU_WORDS] : 0u; }
#pragma unroll
      for (int k = 0; k < REP_PIC_AHEAD; k++) { full += v[k]; lo += v[k] & 0xffffu; hi += v[k] >> 16; }
    }
    L.full[t] = full; L.lo[t] = lo; L.hi[t] = hi;
  } else {
    uint64_t *q = (uint64_t *)(rep + pic);
    if (t < REP_CTU_WORDS) {
      uint64_t full = 0; uint32_t lo = 0, hi = 0;
      for (int j = 0; j < REP_THREADS / 16; j++) { full += L.full[j * 16 + t]; lo += L.lo[j * 16 + t]; hi += L.hi[j * 16 + t]; }
      if (t < 6) q[t] = full;                                 /* ssd[3], bits, bins, dist */
      else { uint32_t *c = (uint32_t *)q + REP_PIC_CNT_WORD + 2 * (t - 6); c[0] = lo; c[1] = hi; }      /* the counters; the last one is `pad` = 0 */
    } else if (t < 19) q[6 + (t - 16)] = t == 16 ? (uint64_t)width * (uint64_t)height : (uint64_t)(width >> 1) * (uint64_t)(height >> 1);   /* n_samples[3] */
    else if (t < 22) q[REP_PIC_PSNR_QWORD + (t - 19)] = 0;   /* psnr[3]: the host fills it from ssd and n_samples */
  }
}

#ifndef FCU_EMU
template <bool WIDE>
__global__ void __launch_bounds__(REP_THREADS) report_ctu(const ReportPic *pics, fcu_ctu_report *ctu, int width, int height, int w_ctu, int n_ctu)
{
  __shared__ uint32_t part[4][REP_SLOTS];
  report_ctu_phase<1, WIDE>(part, pics, ctu, width, height, w_ctu, n_ctu);
  __syncthreads();
  report_ctu_phase<2, WIDE>(part, pics, ctu, width, height, w_ctu, n_ctu);
}
__global__ void __launch_bounds__(REP_THREADS) report_pic(const fcu_ctu_report *ctu, fcu_pic_report *rep, int width, int height, int n_ctu)
{
  __shared__ ReportPicLds L;
  report_pic_phase<1>(L, ctu, rep, width, height, n_ctu);
  __syncthreads();
  report_pic_phase<2>(L, ctu, rep, width, height, n_ctu);
}
#endif

} /* namespace fcu */
