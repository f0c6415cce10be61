/*
 * hash_emu.cpp -- TEST-ONLY: the picture-hash kernel source (csrc/fcu_hash.h) compiled for the CPU with the HIP keywords defined
 * away and the three grids run as loops (workgroup phases in order, threads inside a phase in order), so that the fold, the load
 * paths, the chunking and MD5's padding can be checked against tests/hash_ref.py without a GPU; and the host arithmetic of the
 * CRC (fcu_host.h) on its own.  Not part of libfcu.so.
 */
#define FCU_EMU 1
#include <vector>
#include <cstring>
#include "../../fast-cu-decision-hevc_amd/csrc/fcu_host.h"
#define __device__
struct Dim3 { unsigned x, y, z; };
static thread_local Dim3 blockIdx, threadIdx;
#include "../../fast-cu-decision-hevc_amd/csrc/fcu_hash.h"

using namespace fcu;

template <int ALIGN>
static void run_chunks(const uint8_t *const *planes, HashPartial *part, const HashGeom &G, int n_pics)
{
  static HashLds L;
  for (unsigned pic = 0; pic < (unsigned)n_pics; pic++) for (unsigned c = 0; c < (unsigned)G.per_pic; c++) {
    memset(&L, 0x55, sizeof(L));                             /* the workgroup's LDS starts with whatever the last one left */
    blockIdx.x = c; blockIdx.y = pic;
    for (unsigned t = 0; t < HASH_THREADS; t++) { threadIdx.x = t; hash_chunk_phase<0, ALIGN>(L, planes, part, G); }
    for (unsigned t = 0; t < HASH_THREADS; t++) { threadIdx.x = t; hash_chunk_phase<1, ALIGN>(L, planes, part, G); }
    for (unsigned t = 0; t < HASH_THREADS; t++) { threadIdx.x = t; hash_chunk_phase<2, ALIGN>(L, planes, part, G); }
    for (unsigned t = 0; t < HASH_THREADS; t++) { threadIdx.x = t; hash_chunk_phase<3, ALIGN>(L, planes, part, G); }
  }
}
/* mirrors the launches of fcu_picture_hash (fcu_kernels.hip) for planes of the given geometry; returns the path taken (1 = wide) */
static int run_hash(const HashGeom &G, int n_pics, int wide, const uint8_t *const *planes, fcu_pic_hash *hashes)
{
  const int kinds = G.kinds, n_streams = G.n_planes * n_pics;
  const bool use_wide = wide && hash_wide_ok(planes, n_streams);
  std::vector<HashPartial> part((size_t)G.per_pic * n_pics, HashPartial{ 0xaaaaaaaau, 0xaaaaaaaau });      /* never cleared in the library either */
  if (kinds & (FCU_HASH_CRC | FCU_HASH_CHECKSUM)) {
    if (use_wide) run_chunks<16>(planes, part.data(), G, n_pics); else run_chunks<1>(planes, part.data(), G, n_pics);
    static HashLds L;
    for (unsigned pic = 0; pic < (unsigned)n_pics; pic++) for (unsigned k = 0; k < (unsigned)G.n_planes; k++) {
      memset(&L, 0x55, sizeof(L));
      blockIdx.x = k; blockIdx.y = pic;
      for (unsigned t = 0; t < HASH_THREADS; t++) { threadIdx.x = t; hash_fold_phase<1>(L, part.data(), hashes, G); }
      for (unsigned t = 0; t < HASH_THREADS; t++) { threadIdx.x = t; hash_fold_phase<2>(L, part.data(), hashes, G); }
      for (unsigned t = 0; t < HASH_THREADS; t++) { threadIdx.x = t; hash_fold_phase<3>(L, part.data(), hashes, G); }
    }
  }
  blockIdx.y = 0;
  if (kinds & FCU_HASH_MD5)
    for (unsigned b = 0; b < (unsigned)((n_streams + HASH_MD5_THREADS - 1) / HASH_MD5_THREADS); b++) for (unsigned t = 0; t < HASH_MD5_THREADS; t++) {
      blockIdx.x = b; threadIdx.x = t;
      if (use_wide) hash_md5_thread<16>(planes, hashes, G, n_streams); else hash_md5_thread<1>(planes, hashes, G, n_streams);
    }
  for (int i = 0; i < n_pics; i++) hash_clear_unasked(hashes[i], kinds);
  return use_wide ? 1 : 0;
}

extern "C" {
int hash_emu_chunk(void) { return HASH_CHUNK; }
/* fcu_picture_hash of n_pics pictures of w x h; planes: 3 * n_pics pointers; wide 0: the byte-exact load path whatever the pointers
 * allow, 1: the path the library's host code would choose.  Returns the path taken, or the FCU_ERR_* of the argument check */
int hash_emu(int w, int h, int n_pics, int kinds, int wide, const uint8_t *const *planes, fcu_pic_hash *hashes, char *err, int err_len)
{
  std::string e;
  const int rc = hash_args_check(n_pics, kinds, planes, hashes, e);
  if (rc != FCU_OK) { if (err && err_len > 0) snprintf(err, (size_t)err_len, "%s", e.c_str()); return rc; }
  const uint32_t pw[3] = { (uint32_t)w, (uint32_t)w / 2, (uint32_t)w / 2 }, ph[3] = { (uint32_t)h, (uint32_t)h / 2, (uint32_t)h / 2 };
  return run_hash(hash_geom(3, pw, ph, kinds), n_pics, wide, planes, hashes);
}
/* one plane of w x h samples on its own: its digests land in the fields of plane 0 */
int hash_emu_plane(int w, int h, int kinds, int wide, const uint8_t *plane, fcu_pic_hash *hash)
{
  const uint32_t pw[3] = { (uint32_t)w, 0, 0 }, ph[3] = { (uint32_t)h, 0, 0 };
  memset(hash, 0, sizeof(*hash));
  return run_hash(hash_geom(1, pw, ph, kinds), 1, wide, &plane, hash);
}
/* the kernels' MD5 of a byte buffer of any length */
void hash_emu_md5(const uint8_t *buf, unsigned long long len, uint8_t *digest16) { md5_stream<1>(buf, len, digest16); }
int hash_emu_string(const fcu_pic_hash *h, int kind, char *buf, int buf_len) { return hash_string(h, kind, buf, buf_len); }

/* the host arithmetic of the CRC (fcu_host.h) */
unsigned hash_emu_crc_mul(unsigned a, unsigned b) { return crc_mul(a, b); }
unsigned hash_emu_crc_xpow(unsigned long long n_bits) { return crc_xpow(n_bits); }
unsigned hash_emu_crc_adv(unsigned s, unsigned long long n_bits) { return crc_adv(s, n_bits); }
unsigned hash_emu_crc_bytes(unsigned s, const uint8_t *p, unsigned long long n) { return crc_bytes(s, p, (size_t)n); }
unsigned hash_emu_crc_digest(const uint8_t *p, unsigned long long n) { return crc_digest(p, (size_t)n); }
void hash_emu_crc_tab(uint16_t *out256) { static constexpr CrcTab T = crc_make_tab(); memcpy(out256, T.t, sizeof(T.t)); }
}
