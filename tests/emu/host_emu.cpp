/*
 * host_emu.cpp -- TEST-ONLY driver of the host state machine of libfcu.so (HostState, fcu_host.h) without a device: the argument
 * and state rules of the chain entry points, the picture binder and the two launch guards, called in the order the entry points
 * of fcu_kernels.hip call them, with plane pointers that are not null and never read.  No engine code runs; "launched" stands
 * for the kernel.  Every function returns the FCU_* code the entry point of the same name returns (0 = accepted).
 * Built by __graft_entry__.build().  It is NOT part of libfcu.so and nothing in the product path can reach it.
 */
#define FCU_EMU 1
#include "../../fast-cu-decision-hevc_amd/csrc/fcu_host.h"

using namespace fcu;

struct EmuHost {
  HostState hs;
  std::vector<uint8_t> sync;
  int bound_chains = 0;            /* chains the last accepted binder filled */
};
/* never read: addresses that tell the planes, output arrays and reference pictures of the test apart by `tag` */
static uint8_t g_arena[4096];
static uint8_t *fake(int tag, int k) { return g_arena + 16 * (tag & 255) + k; }

extern "C" {
void *host_emu_create(int width, int height, int max_chains)
{
  const fcu_seq_params sp = { width, height, max_chains, 0 };
  if (!HostState::seq_ok(&sp)) return nullptr;
  EmuHost *e = new EmuHost();
  e->hs.init(sp);
  e->sync.assign((size_t)max_chains * WPP_SYNC_BYTES, 0);
  return e;
}
void host_emu_destroy(void *p) { delete (EmuHost *)p; }
const char *host_emu_error(void *p) { return ((EmuHost *)p)->hs.err.c_str(); }
int host_emu_position(void *p, int chain) { return ((EmuHost *)p)->hs.position(chain); }
int host_emu_bound_chains(void *p) { return ((EmuHost *)p)->bound_chains; }

/* the binders.  kind 0 fcu_chain_begin (first = the chain), 1 fcu_wpp_begin, 2 fcu_wpp_begin_p, 3 fcu_wpp_begin_slices (a =
 * slice_rows), 4 fcu_tiles_begin, 5 fcu_wpp_begin_tiles (a x b tiles); pic: the picture's planes and output array */
int host_emu_begin(void *p, int kind, int first, const fcu_frame_params *fp, int a, int b, int pic)
{
  EmuHost *e = (EmuHost *)p;
  const Planes pl = { fake(pic, 0), fake(pic, 1), fake(pic, 2), fake(pic, 3), fake(pic, 4), fake(pic, 5), (fcu_ctu_out *)fake(pic, 8) };
  if (kind == 0) return e->hs.chain_begin(first, fp, pl);
  const PictureCut cut = kind == 1 ? PictureCut::rows(FCU_SLICE_I) : kind == 2 ? PictureCut::rows(FCU_SLICE_P) : kind == 3 ? PictureCut::row_slices(a) : PictureCut::tiles(a, b, kind == 5);
  const int rc = e->hs.picture_check(cut, first, fp, pl);
  if (rc == FCU_OK) e->bound_chains = e->hs.picture_bind(cut, first, *fp, pl, e->sync.data());
  return rc;
}
int host_emu_set_range(void *p, int chain, int first_ctu, int n_ctus) { return ((EmuHost *)p)->hs.set_range(chain, first_ctu, n_ctus); }
/* fcu_chain_set_references with the padded planes of picture `tag + r` as RefPicList0[r] */
int host_emu_set_references(void *p, int chain, int n_ref, int tag, const int *ref_pocs, int cur_poc)
{
  HostState &hs = ((EmuHost *)p)->hs;
  const int rc = hs.bound("fcu_chain_set_references", chain);
  if (rc != FCU_OK) return rc;
  const uint8_t *planes[3 * FCU_MAX_REF];
  for (int k = 0; k < 3 * n_ref; k++) planes[k] = fake(tag + k / 3, k % 3);
  chain_set_list0(hs.chains[(size_t)chain], n_ref, planes, ref_pocs, cur_poc);
  return FCU_OK;
}
int host_emu_set_collocated_pocs(void *p, int chain, int col_poc, const int *col_ref_pocs, int n)
{
  HostState &hs = ((EmuHost *)p)->hs;
  const int rc = hs.bound("fcu_chain_set_collocated_pocs", chain);
  if (rc != FCU_OK) return rc;
  return chain_set_collocated_pocs(hs.chains[(size_t)chain], col_poc, col_ref_pocs, n) ? FCU_OK : FCU_ERR_ARG;
}
int host_emu_set_collocated(void *p, int chain, int tag)
{
  HostState &hs = ((EmuHost *)p)->hs;
  const int rc = hs.bound("fcu_chain_set_collocated", chain);
  if (rc == FCU_OK) hs.chains[(size_t)chain].col = tag < 0 ? nullptr : (const fcu_ctu_out *)fake(tag, 8);
  return rc;
}

/* the guards of fcu_compress_chains / fcu_compress_wpp alone, and the bookkeeping after a launch ("mark as launched") */
int host_emu_chains_check(void *p, int first, int n, int ctus) { return ((EmuHost *)p)->hs.chains_check(first, n, ctus); }
int host_emu_wpp_check(void *p, int first, int n) { return ((EmuHost *)p)->hs.wpp_check(first, n); }
void host_emu_chains_launched(void *p, int first, int n, int ctus) { ((EmuHost *)p)->hs.chains_launched(first, n, ctus); }
void host_emu_wpp_launched(void *p, int first, int n) { ((EmuHost *)p)->hs.wpp_launched(first, n); }
/* fcu_compress_ctu: its own rule, then the launch of one CTU as fcu_compress_chains(chain, 1, 1) */
int host_emu_compress_ctu(void *p, int chain, unsigned addr)
{
  HostState &hs = ((EmuHost *)p)->hs;
  int rc = hs.ctu_check(chain, addr);
  if (rc == FCU_OK) rc = hs.chains_check(chain, 1, 1);
  if (rc == FCU_OK) hs.chains_launched(chain, 1, 1);
  return rc;
}
}
