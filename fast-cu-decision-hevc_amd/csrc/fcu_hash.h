/*
 * fcu_hash.h -- the decoded-picture hash of the encoder on the device: MD5, CRC and checksum of reconstructed planes as HM computes
 * and prints them (calcMD5 / calcCRC / calcChecksum, Lib/TLibCommon/TComPicYuvMD5.cpp:44-207; printed by TEncGOP.cpp:1742-1756).
 * Included by fcu_kernels.hip only (and by the test-only CPU build tests/emu/hash_emu.cpp).
 *
 * Planes are 8-bit and dense (stride = width); every plane is hashed on its own.  A plane of n bytes (a multiple of 16) is cut
 * into units of 16 bytes and chunks of HASH_CHUNK = 16 KiB, counted from the END of the plane: the chunks are full except the
 * first, which holds what is left.  No atomics, no memory that must be zero beforehand; every output byte is written by exactly one
 * thread, so a repeated call gives identical bytes.
 *   hash_chunk   one 256-thread workgroup per (chunk, picture) -> one HashPartial (CRC state from 0 and checksum of the chunk).
 *                A thread loads unit t, t + 256, t + 512, t + 768 of the chunk (coalesced; all four loads are issued before the
 *                first use): 16-byte loads when every plane pointer of the batch is 16-byte aligned (hash_wide_ok), byte-exact
 *                copies otherwise.  CRC: the state is a polynomial over GF(2) mod P and the update is linear (fcu_host.h), so a
 *                unit's state from 0 comes from the byte table (in LDS, copied from the constexpr table) and units fold as
 *                v = v x^n ^ next, with n the distance in bits -- a compile-time constant at every level: x^(128 * 256) between a
 *                thread's four units, x^128 between neighbouring threads (sixteen threads fold sixteen values each, one thread
 *                folds those with x^(128 * 16)).  State 0 stays 0 under zero input: the units the short first chunk lacks sit at
 *                the FRONT of its workgroup and hold 0, the rest is right-aligned and folds through the same tree (zeros in
 *                front are neutral; appended zeros would not be).  Checksum: a thread derives x and y of its unit's first byte
 *                from the byte index (one division per unit) and walks the 16 bytes; 32-bit adds wrap as the definition does.
 *   hash_fold    one 256-thread workgroup per (plane, picture): the same tree over the plane's partials, with x^(8 * HASH_CHUNK)
 *                between neighbouring chunks; then the initial state's term 0xffff x^(8 n) (host arithmetic, in HashGeom) and
 *                the sixteen flushed zero bits.  Thread 0 stores crc[plane] and checksum[plane] of the record (0 for a kind
 *                that was not asked for), high byte first.
 *   hash_md5     RFC 1321 is one dependent chain of 64-byte blocks per plane, so the unit of parallelism is the stream
 *                (picture, plane): one stream per lane, 64 streams per workgroup.  A lane loads block b + 1 before the 64 steps
 *                of block b.  Any byte length (the padding blocks are built byte by byte).  Launched only when MD5 is asked for.
 * Algorithmic bytes per picture: 1.5 W H read once for CRC + checksum, once more for MD5; 8 B per chunk written and read back.
 * Planes stay below 4 GiB (byte indices are 32 bits wide inside a plane).
 */
#pragma once

namespace fcu {

enum { HASH_THREADS = 256, HASH_UNIT = 16, HASH_UPT = 4, HASH_CHUNK = HASH_THREADS * HASH_UPT * HASH_UNIT, HASH_FOLD_AHEAD = 4, HASH_MD5_THREADS = 64 };
static_assert(sizeof(fcu_pic_hash) == 68 && offsetof(fcu_pic_hash, crc) == 48 && offsetof(fcu_pic_hash, checksum) == 54 && offsetof(fcu_pic_hash, pad) == 66, "record layout the byte stores rely on");

/* the multipliers of the two trees: x^n for the distance n in bits between the values a level folds */
constexpr uint32_t HASH_X_UNIT = crc_xpow(8 * HASH_UNIT), HASH_X_UNIT16 = crc_xpow(8 * HASH_UNIT * 16), HASH_X_ROUND = crc_xpow(8 * HASH_UNIT * HASH_THREADS),
                   HASH_X_CHUNK = crc_xpow(8 * HASH_CHUNK), HASH_X_CHUNK16 = crc_xpow(8 * (uint64_t)HASH_CHUNK * 16), HASH_X_CHUNK_ROUND = crc_xpow(8 * (uint64_t)HASH_CHUNK * HASH_THREADS),
                   HASH_X_FLUSH = crc_xpow(16);
FCU_TABLE CrcTab k_crc_tab = crc_make_tab();

struct HashPartial { uint32_t crc, sum; };                 /* of one chunk: CRC state from state 0, checksum */
/* the planes of a batch as the kernels see them (by value): n_planes per picture (3; 1 for the plane-level entry of the CPU build),
 * per plane its width, bytes, chunks, the index of its first chunk among the picture's per_pic chunks, and 0xffff x^(8 bytes) */
struct HashGeom { uint32_t w[3], n[3], chunks[3], first[3], crc_init[3]; int32_t n_planes, per_pic, kinds; };
inline HashGeom hash_geom(int n_planes, const uint32_t *w, const uint32_t *h, int kinds)
{
  HashGeom G = {};
  G.n_planes = n_planes; G.kinds = kinds;
  uint32_t first = 0;
  for (int k = 0; k < 3; k++) {
    G.first[k] = first;
    if (k >= n_planes) continue;
    G.w[k] = w[k]; G.n[k] = w[k] * h[k]; G.chunks[k] = (G.n[k] + HASH_CHUNK - 1) / HASH_CHUNK;
    G.crc_init[k] = crc_adv(CRC_INIT, 8 * (uint64_t)G.n[k]);
    first += G.chunks[k];
  }
  G.per_pic = (int32_t)first;
  return G;
}
/* host: may the batch take the 16-byte loads?  Every plane pointer on 16 bytes (plane lengths are multiples of 16) */
inline bool hash_wide_ok(const uint8_t *const *planes, int n)
{
  bool ok = true;
  for (int i = 0; i < n; i++) ok = ok && ((uintptr_t)planes[i] & 15) == 0;
  return ok;
}
/* host: the record as the caller gets it -- the fields of a kind that was not asked for (its kernel has not written them) are zero */
inline void hash_clear_unasked(fcu_pic_hash &r, int kinds)
{
  if (!(kinds & FCU_HASH_MD5)) memset(r.md5, 0, sizeof(r.md5));
  if (!(kinds & (FCU_HASH_CRC | FCU_HASH_CHECKSUM))) { memset(r.crc, 0, sizeof(r.crc)); memset(r.checksum, 0, sizeof(r.checksum)); memset(r.pad, 0, sizeof(r.pad)); }
}

/* N bytes at p, known to be ALIGN-aligned (1: nothing is known), as little-endian words */
template <int N> struct HashBytes { uint32_t v[N / 4]; };
typedef HashBytes<HASH_UNIT> HashUnit;
template <int N, int ALIGN>
__device__ static inline void hash_load(HashBytes<N> &u, const uint8_t *p)
{
  /* (planes are HBM: global_ instead of flat_ loads) */
  __builtin_memcpy(u.v, (const FCU_HBM uint8_t *)__builtin_assume_aligned(p, ALIGN), N);
}
/* CRC state after the unit's 16 bytes from state 0 */
__device__ static inline uint32_t hash_unit_crc(const uint16_t *tab, const HashUnit &u)
{
  uint32_t s = 0;
#pragma unroll
  for (int k = 0; k < HASH_UNIT; k++) s = ((s << 8) & 0xffffu) ^ ((u.v[k >> 2] >> (8 * (k & 3))) & 255u) ^ tab[s >> 8];
  return s;
}
/* checksum of the unit whose first byte is byte i of a plane w samples wide */
__device__ static inline uint32_t hash_unit_sum(const HashUnit &u, uint32_t i, uint32_t w)
{
  uint32_t y = i / w, x = i - y * w, s = 0;
#pragma unroll
  for (int k = 0; k < HASH_UNIT; k++) {
    s += ((u.v[k >> 2] >> (8 * (k & 3))) ^ x ^ y ^ (x >> 8) ^ (y >> 8)) & 255u;
    if (++x == w) { x = 0; y++; }
  }
  return s;
}

/* the workgroup's LDS of hash_chunk and hash_fold: the byte table, one value per thread, one per group of sixteen threads */
struct HashLds { uint16_t tab[256]; uint32_t crc[HASH_THREADS], sum[HASH_THREADS], crc16[HASH_THREADS / 16], sum16[HASH_THREADS / 16]; };

/* phases 2 and 3 of both kernels: 256 values in thread order -> one.  XN: x^n for the distance n between neighbours, XN16 = XN^16.
 * Phase 2 leaves sixteen values in LDS; phase 3 returns true in thread 0 with the result */
template <int PHASE>
__device__ static inline bool hash_tree(HashLds &L, uint32_t xn, uint32_t xn16, uint32_t &crc, uint32_t &sum)
{
  const int t = (int)threadIdx.x;
  if (PHASE == 2) {
    if (t < HASH_THREADS / 16) {
      uint32_t v = 0, s = 0;
      for (int j = 0; j < 16; j++) { v = crc_mul(v, xn) ^ L.crc[t * 16 + j]; s += L.sum[t * 16 + j]; }
      L.crc16[t] = v; L.sum16[t] = s;
    }
    return false;
  }
  if (t != 0) return false;
  uint32_t v = 0, s = 0;
  for (int j = 0; j < HASH_THREADS / 16; j++) { v = crc_mul(v, xn16) ^ L.crc16[j]; s += L.sum16[j]; }
  crc = v; sum = s;
  return true;
}

/* ---- hash_chunk: phase 0 copies the byte table, 1 leaves every thread's value in LDS, 2 and 3 fold and store the partial ---- */
template <int PHASE, int ALIGN>
__device__ static inline void hash_chunk_phase(HashLds &L, const uint8_t *const *planes, HashPartial *part, const HashGeom &G)
{
  const int t = (int)threadIdx.x, c = (int)blockIdx.x, pic = (int)blockIdx.y;
  if (PHASE == 0) { L.tab[t] = k_crc_tab.t[t]; return; }
  if (PHASE == 1) {
    const int k = (G.n_planes > 2 && (uint32_t)c >= G.first[2]) ? 2 : ((G.n_planes > 1 && (uint32_t)c >= G.first[1]) ? 1 : 0);
    const uint8_t *p = planes[(size_t)pic * G.n_planes + k];
    /* byte of the plane at which this chunk's window of HASH_CHUNK bytes starts: below 0 in the short first chunk only */
    const long long base = (long long)G.n[k] - (long long)(G.chunks[k] - ((uint32_t)c - G.first[k])) * HASH_CHUNK;
    HashUnit u[HASH_UPT];
    bool in[HASH_UPT];
#pragma unroll
    for (int r = 0; r < HASH_UPT; r++) {
      const long long o = base + (long long)(r * HASH_THREADS + t) * HASH_UNIT;
      in[r] = o >= 0;                                         /* (o + 16 <= n always: the window ends with the plane or before) */
      if (in[r]) hash_load<HASH_UNIT, ALIGN>(u[r], p + o);
    }
    uint32_t v = 0, s = 0;
#pragma unroll
    for (int r = 0; r < HASH_UPT; r++) {
      v = crc_mul(v, HASH_X_ROUND);
      if (!in[r]) continue;
      if (G.kinds & FCU_HASH_CRC) v ^= hash_unit_crc(L.tab, u[r]);
      if (G.kinds & FCU_HASH_CHECKSUM) s += hash_unit_sum(u[r], (uint32_t)(base + (long long)(r * HASH_THREADS + t) * HASH_UNIT), G.w[k]);
    }
    L.crc[t] = v; L.sum[t] = s;
    return;
  }
  uint32_t v = 0, s = 0;
  if (hash_tree<PHASE>(L, HASH_X_UNIT, HASH_X_UNIT16, v, s)) { HashPartial &o = part[(size_t)pic * G.per_pic + c]; o.crc = v; o.sum = s; }
}

/* ---- hash_fold: phase 1 leaves every thread's value in LDS, 2 and 3 fold, finish and store the record's fields ------------- */
template <int PHASE>
__device__ static inline void hash_fold_phase(HashLds &L, const HashPartial *part, fcu_pic_hash *hashes, const HashGeom &G)
{
  const int t = (int)threadIdx.x, k = (int)blockIdx.x, pic = (int)blockIdx.y;
  if (PHASE == 1) {
    const FCU_HBM HashPartial *P = (const FCU_HBM HashPartial *)(part + (size_t)pic * G.per_pic + G.first[k]);
    const int n = (int)G.chunks[k], rounds = (n + HASH_THREADS - 1) / HASH_THREADS, lead = rounds * HASH_THREADS - n;      /* right-aligned as the units of a chunk are */
    uint32_t v = 0, s = 0;
    for (int r0 = 0; r0 < rounds; r0 += HASH_FOLD_AHEAD) {
      HashPartial q[HASH_FOLD_AHEAD];
#pragma unroll
      for (int j = 0; j < HASH_FOLD_AHEAD; j++) {
        const int i = (r0 + j) * HASH_THREADS + t - lead;
        q[j].crc = 0; q[j].sum = 0;
        if (r0 + j < rounds && i >= 0) { q[j].crc = P[i].crc; q[j].sum = P[i].sum; }
      }
#pragma unroll
      for (int j = 0; j < HASH_FOLD_AHEAD; j++) if (r0 + j < rounds) { v = crc_mul(v, HASH_X_CHUNK_ROUND) ^ q[j].crc; s += q[j].sum; }
    }
    L.crc[t] = v; L.sum[t] = s;
    return;
  }
  uint32_t v = 0, s = 0;
  if (hash_tree<PHASE>(L, HASH_X_CHUNK, HASH_X_CHUNK16, v, s)) {
    const uint32_t crc = (G.kinds & FCU_HASH_CRC) ? crc_mul(v ^ G.crc_init[k], HASH_X_FLUSH) : 0u, sum = (G.kinds & FCU_HASH_CHECKSUM) ? s : 0u;
    uint8_t *o = (uint8_t *)(hashes + pic);
    o[48 + 2 * k] = (uint8_t)(crc >> 8); o[49 + 2 * k] = (uint8_t)crc;
    for (int j = 0; j < 4; j++) o[54 + 4 * k + j] = (uint8_t)(sum >> (24 - 8 * j));
    if (k == 0) { o[66] = 0; o[67] = 0; }
  }
}

/* ---- MD5 (RFC 1321).  T[i] = floor(2^32 |sin(i + 1)|), the per-round shift amounts --------------------------------------- */
FCU_TABLE uint32_t k_md5_t[64] = {
  0xd76aa478u, 0xe8c7b756u, 0x242070dbu, 0xc1bdceeeu, 0xf57c0fafu, 0x4787c62au, 0xa8304613u, 0xfd469501u, 0x698098d8u, 0x8b44f7afu, 0xffff5bb1u, 0x895cd7beu,
  0x6b901122u, 0xfd987193u, 0xa679438eu, 0x49b40821u, 0xf61e2562u, 0xc040b340u, 0x265e5a51u, 0xe9b6c7aau, 0xd62f105du, 0x02441453u, 0xd8a1e681u, 0xe7d3fbc8u,
  0x21e1cde6u, 0xc33707d6u, 0xf4d50d87u, 0x455a14edu, 0xa9e3e905u, 0xfcefa3f8u, 0x676f02d9u, 0x8d2a4c8au, 0xfffa3942u, 0x8771f681u, 0x6d9d6122u, 0xfde5380cu,
  0xa4beea44u, 0x4bdecfa9u, 0xf6bb4b60u, 0xbebfbc70u, 0x289b7ec6u, 0xeaa127fau, 0xd4ef3085u, 0x04881d05u, 0xd9d4d039u, 0xe6db99e5u, 0x1fa27cf8u, 0xc4ac5665u,
  0xf4292244u, 0x432aff97u, 0xab9423a7u, 0xfc93a039u, 0x655b59c3u, 0x8f0ccc92u, 0xffeff47du, 0x85845dd1u, 0x6fa87e4fu, 0xfe2ce6e0u, 0xa3014314u, 0x4e0811a1u,
  0xf7537e82u, 0xbd3af235u, 0x2ad7d2bbu, 0xeb86d391u };
FCU_TABLE uint8_t k_md5_s[16] = { 7, 12, 17, 22, 5, 9, 14, 20, 4, 11, 16, 23, 6, 10, 15, 21 };

/* the 64 steps on one block (sixteen little-endian words); fully unrolled: every table entry and word index is a constant */
__device__ static inline void md5_block(uint32_t st[4], const HashBytes<64> &blk)
{
  const uint32_t *w = blk.v;
  uint32_t a = st[0], b = st[1], c = st[2], d = st[3];
#pragma unroll
  for (int i = 0; i < 64; i++) {
    const uint32_t f = i < 16 ? ((b & c) | (~b & d)) : (i < 32 ? ((d & b) | (~d & c)) : (i < 48 ? (b ^ c ^ d) : (c ^ (b | ~d))));
    const int g = i < 16 ? i : (i < 32 ? (5 * i + 1) & 15 : (i < 48 ? (3 * i + 5) & 15 : (7 * i) & 15)), sh = k_md5_s[(i >> 4) * 4 + (i & 3)];
    const uint32_t x = a + f + k_md5_t[i] + w[g];
    a = d; d = c; c = b; b = b + ((x << sh) | (x >> (32 - sh)));
  }
  st[0] += a; st[1] += b; st[2] += c; st[3] += d;
}
/* block b of the padded message of len bytes at p (n_blocks in all): a full block is one 64-byte copy, the last one or two
 * blocks -- the message's tail, 0x80, zeros and the length in bits -- are built byte by byte */
template <int ALIGN>
__device__ static inline void md5_fetch(HashBytes<64> &blk, const uint8_t *p, uint64_t len, uint64_t b, uint64_t n_blocks)
{
  if (b < (len >> 6)) { hash_load<64, ALIGN>(blk, p + (b << 6)); return; }
  uint32_t *w = blk.v;
  const FCU_HBM uint8_t *q = (const FCU_HBM uint8_t *)p;
#pragma unroll
  for (int j = 0; j < 16; j++) w[j] = 0;
#pragma unroll
  for (int j = 0; j < 64; j++) {
    const uint64_t pos = (b << 6) + (uint64_t)j;
    const uint32_t v = pos < len ? q[pos] : (pos == len ? 0x80u : 0u);
    w[j >> 2] |= v << (8 * (j & 3));
  }
  if (b + 1 == n_blocks) { w[14] = (uint32_t)(len << 3); w[15] = (uint32_t)(len >> 29); }
}
/* MD5 of len bytes at p (known to be ALIGN-aligned; 1: nothing is known) -> 16 digest bytes */
template <int ALIGN>
__device__ static inline void md5_stream(const uint8_t *p, uint64_t len, uint8_t *digest)
{
  const uint64_t n_blocks = ((len + 8) >> 6) + 1;
  uint32_t st[4] = { 0x67452301u, 0xefcdab89u, 0x98badcfeu, 0x10325476u };
  HashBytes<64> cur, nxt;
  md5_fetch<ALIGN>(nxt, p, len, 0, n_blocks);
  for (uint64_t b = 0; b < n_blocks; b++) {
    cur = nxt;
    if (b + 1 < n_blocks) md5_fetch<ALIGN>(nxt, p, len, b + 1, n_blocks);      /* in flight during the 64 steps below */
    md5_block(st, cur);
  }
#pragma unroll
  for (int j = 0; j < 16; j++) digest[j] = (uint8_t)(st[j >> 2] >> (8 * (j & 3)));
}
/* stream i of the batch = plane i % n_planes of picture i / n_planes */
template <int ALIGN>
__device__ static inline void hash_md5_thread(const uint8_t *const *planes, fcu_pic_hash *hashes, const HashGeom &G, int n_streams)
{
  const int i = (int)(blockIdx.x * HASH_MD5_THREADS + threadIdx.x);
  if (i >= n_streams) return;
  const int pic = i / G.n_planes, k = i - pic * G.n_planes;
  md5_stream<ALIGN>(planes[i], G.n[k], hashes[pic].md5[k]);
}

#ifndef FCU_EMU
template <int ALIGN>
__global__ void __launch_bounds__(HASH_THREADS) hash_chunk(const uint8_t *const *planes, HashPartial *part, const HashGeom G)
{
  __shared__ HashLds L;
  hash_chunk_phase<0, ALIGN>(L, planes, part, G);
  __syncthreads();
  hash_chunk_phase<1, ALIGN>(L, planes, part, G);
  __syncthreads();
  hash_chunk_phase<2, ALIGN>(L, planes, part, G);
  __syncthreads();
  hash_chunk_phase<3, ALIGN>(L, planes, part, G);
}
__global__ void __launch_bounds__(HASH_THREADS) hash_fold(const HashPartial *part, fcu_pic_hash *hashes, const HashGeom G)
{
  __shared__ HashLds L;
  hash_fold_phase<1>(L, part, hashes, G);
  __syncthreads();
  hash_fold_phase<2>(L, part, hashes, G);
  __syncthreads();
  hash_fold_phase<3>(L, part, hashes, G);
}
template <int ALIGN>
__global__ void __launch_bounds__(HASH_MD5_THREADS) hash_md5(const uint8_t *const *planes, fcu_pic_hash *hashes, const HashGeom G, int n_streams)
{
  hash_md5_thread<ALIGN>(planes, hashes, G, n_streams);
}
#endif

} /* namespace fcu */
