/*
 * fcu.h -- C ABI of the MI355X CU-decision engine (libfcu.so).
 *
 * Drop-in boundary for HM's `TEncCu` (reference: Lib/TLibEncoder/TEncCu.h:104-118):
 *
 *   reference entry point                         replacement
 *   -------------------------------------------   ------------------------------------------
 *   TEncCu::create  (TEncCu.cpp:163)              fcu_create
 *   TEncCu::destroy (TEncCu.cpp:214)              fcu_destroy
 *   TEncCu::init + TEncSlice::setUpLambda         fcu_chain_begin   (per slice-chain parameters,
 *     (TEncCu.cpp:306, TEncSlice.cpp:496-524)                        lambda as f64 bit patterns)
 *   slice loop of TEncGOP::compressGOP             fcu_chain_set_range (one chain per slice of a frame)
 *     (TEncGOP.cpp:1102-1138, SliceMode 1)
 *   TEncCu::compressCtu (TEncCu.cpp:329)          fcu_compress_ctu  (one CTU of one chain) /
 *     + TEncCu::encodeCtu context replay          fcu_compress_chains (batched, many chains)
 *     (TEncCu.cpp:359, TEncSlice.cpp:1468-1487)
 *   TEncSlice::getOutlierWithDCT (fork pre-pass)   fcu_obf_prepass
 *     (TEncSlice.cpp:878-1173, TEncGOP.cpp:1096)
 *   fork decision hooks of TEncCu::xCompressCU     fcu_chain_set_decision (frame state + Naive switches + OBF map),
 *     (TEncCu.cpp:504-507,585-603,951-996,           fcu_get_verify_counts (g_iVerResult of the Verifying frame),
 *      1040,1143,1257,1446,1489-1497;                fcu_decision_switch (SetDecisionSwitch), fcu_frame_state
 *      tools_YS.cpp:686-695,968-986,1123-1154,1237)   (getCurrentState)
 *   TEncSearch::estIntraPredLumaQT per-PU results  fcu_chain_set_pu_trace (BASELINE configs[1]: luma RDO artefact)
 *     (TEncSearch.cpp:2178-2655)
 *   TComLoopFilter::loopFilterPic                  fcu_deblock (in-loop deblocking of the decided picture);
 *     (TComLoopFilter.cpp:130, TEncGOP.cpp:1160)     a picture with tiles: fcu_deblock_tiles (LFCrossTileBoundaryFlag 0 or 1);
 *                                                    slices: fcu_deblock_slices (LFCrossSliceBoundaryFlag 0 or 1, :369-411)
 *   TEncSampleAdaptiveOffset::SAOProcess           fcu_sao (statistics, per-CTU parameter decision, offset pass) +
 *     (TEncSampleAdaptiveOffset.cpp:257,              fcu_sao_enabled / fcu_sao_update_rate (decidePicParams and the
 *      TEncGOP.cpp:1427-1441)                         m_saoDisabledRate bookkeeping across pictures, :363-395,895-917);
 *                                                    a picture with tiles: fcu_sao_tiles (merge candidates inside the tile,
 *                                                    TComPic.cpp:138-143; LFCrossTileBoundaryFlag 0 or 1, TComPicSym.cpp:378,449-459);
 *                                                    slices: fcu_sao_slices (LFCrossSliceBoundaryFlag 0 or 1, TComPicSym.cpp:357-447)
 *   WaveFrontSynchro=1 row loop of                 fcu_wpp_begin / fcu_wpp_begin_p (one chain per CTU row of a
 *     TEncSlice::compressSlice                       one-slice I / P picture), fcu_compress_wpp (every row of whole
 *     (TEncSlice.cpp:1386-1411,1514-1517)            pictures in one launch, a row waiting for the row above), fcu_wpp_rows
 *     + m_integerMv2Nx2N across rows              (P: the row above's TZ start vectors, taken in the launch)
 *     (TEncSearch.cpp:3833-3842)
 *   tiles of a one-slice picture                    fcu_tile_grid (TileUniformSpacing), fcu_tiles_begin (one chain per tile,
 *     (TComPicSym::initTiles; TEncSlice.cpp            tile-scan order), fcu_wpp_begin_tiles (WaveFrontSynchro inside every
 *      1386-1411,1514-1517,1718-1727;                  tile: one chain per CTU row of every tile), fcu_tile_chains
 *      TComDataCU.cpp:422-440,1071-1390)
 *   TEncGOP::xCalculateAddPSNR                     fcu_picture_report (SSD per plane -> PSNR, bits, bins, distortion and CU
 *     (TEncGOP.cpp:2195-2290)                        statistics of decided, filtered pictures; per CTU and per picture)
 *   calcMD5 / calcCRC / calcChecksum,               fcu_picture_hash (the decoded-picture hash of reconstructed pictures, per
 *     digestToString (TComPicYuvMD5.cpp:44-225,       plane, as the encoder prints it at the end of the picture line),
 *      TEncGOP.cpp:1619-1640,1742-1756)               fcu_hash_string (the printed form)
 *   the fork's other model types (SVM, forest,      fcu_chain_set_labels (split labels of a model of the caller's, per picture, in
 *     CNN ... behind the same hooks,                  the place of the Naive label), fcu_label_count, fcu_labels_from_rasters
 *     tools_YS.cpp:686-695, TEncCu.cpp:670-678)       (depth / part_size rasters -> label array)
 *   the published decision as pictures;             fcu_decision_maps (raster maps of the per-partition arrays of fcu_ctu_out, the
 *     the fork's Training dump of split labels         motion map, per-CU split labels and N_OBF features of the chosen tree),
 *     next to N_OBF (tools_YS.cpp:304-318,             fcu_split_match (agreement of two decisions of a picture, per partition
 *      TEncCu.cpp:585-600,1489-1497)                   and per quadtree node)
 *   the fork's Training set of ALL visited CUs:      fcu_chain_set_cu_trace (J0, J1 and the outcome of every CU the search visits, kept
 *     label, J0, J1 per CU (tools_YS.cpp:304-318,     per CTU), fcu_trace_maps (the trace as label / J0 / J1 maps aligned with N_OBF),
 *      968-986; TEncCu.cpp:1450-1451,1489-1497)       fcu_label_score (countTFPN + countRDLoss of any label array against a trace,
 *                                                    without deciding the picture again), fcu_cu_index
 *   the fork's tree model type RTS_OpenCV           fcu_feature_bins (feature maps -> 32 bins per column), fcu_tree_train / fcu_tree_hist /
 *     (CvRTrees_model, globals_YS.h:124: OpenCV's     fcu_tree_split (a small tree per depth over the binned columns, from integer
 *      random trees, external)                        histograms of the trace's quantised loss), fcu_tree_keys (its leaf index as
 *                                                    the key of the risk table): this library's definition, not OpenCV's
 *   m_pppcRDSbacCoder[0][CI_CURR_BEST] state      fcu_get_ctx_state
 *     (TEncSlice.cpp:1417,1477)
 *
 * Plain pointers and sizes only; no torch / HIP types.  All `dev_*` pointers are device
 * (HBM) addresses owned by the caller; planes are 8-bit 4:2:0 (HM's int16 `Pel` planes are
 * narrowed by the adapter).  The library FAILS (returns FCU_ERR_NO_DEVICE)
 * when no HIP device is present: there is no CPU fallback.
 */
#ifndef FCU_H
#define FCU_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

#define FCU_NPART 256            /* 4x4 partitions per 64x64 CTU, z-order (TComDataCU) */

enum { FCU_OK = 0, FCU_ERR_NO_DEVICE = -1, FCU_ERR_ARG = -2, FCU_ERR_HIP = -3, FCU_ERR_STATE = -4 };

/* Per-CTU result: the TComDataCU arrays that copyToPic publishes (TComDataCU.h:72-164,
 * TComDataCU.cpp:992-1065).  One entry per 4x4 luma partition, z-order.  Coefficients are
 * TU-contiguous at offset absPartIdx*16 (luma) / absPartIdx*4 (chroma) like m_pcTrCoeff. */
typedef struct fcu_ctu_out {
  uint8_t  depth[FCU_NPART], width[FCU_NPART], height[FCU_NPART];   /* m_puhDepth/Width/Height */
  uint8_t  skip[FCU_NPART];                                         /* m_skipFlag              */
  int8_t   part_size[FCU_NPART], pred_mode[FCU_NPART];              /* m_pePartSize/PredMode   */
  uint8_t  tq_bypass[FCU_NPART];                                    /* m_CUTransquantBypass    */
  int8_t   qp[FCU_NPART];                                           /* m_phQP                  */
  uint8_t  chroma_qp_adj[FCU_NPART];                                /* m_ChromaQpAdj           */
  uint8_t  tr_idx[FCU_NPART];                                       /* m_puhTrIdx              */
  uint8_t  tskip[3][FCU_NPART];                                     /* m_puhTransformSkip      */
  uint8_t  cbf[3][FCU_NPART];                                       /* m_puhCbf (bit t = depth t) */
  uint8_t  intra_dir[2][FCU_NPART];                                 /* m_puhIntraDir           */
  uint8_t  ipcm[FCU_NPART];                                         /* m_pbIPCMFlag            */
  /* inter prediction data, reference picture list 0 (P slices; list 1 does not exist in the configurations built) */
  uint8_t  merge_flag[FCU_NPART], merge_idx[FCU_NPART];             /* m_pbMergeFlag, m_puhMergeIndex */
  uint8_t  inter_dir[FCU_NPART];                                    /* m_puhInterDir (1 = list 0) */
  int8_t   mvp_idx[FCU_NPART], ref_idx[FCU_NPART];                  /* m_apiMVPIdx[0], m_acCUMvField[0] refIdx (-1 = none) */
  int16_t  mv[FCU_NPART][2], mvd[FCU_NPART][2];                     /* m_acCUMvField[0] mv / mvd, quarter samples, [hor, ver] */
  int32_t  coeff_y[4096], coeff_cb[1024], coeff_cr[1024];           /* m_pcTrCoeff             */
  double   total_cost;                                              /* m_dTotalCost            */
  uint32_t total_dist, total_bits, total_bins;                      /* m_uiTotal*              */
} fcu_ctu_out;

typedef struct fcu_seq_params {
  int width, height;             /* luma samples, multiples of 8 (SPS)                       */
  int max_chains;                /* chains (frame/slice sequences) decided concurrently      */
  int device;                    /* HIP device ordinal                                       */
} fcu_seq_params;

typedef struct fcu_frame_params {
  int qp;                        /* slice QP                                                 */
  int slice_ctus;                /* SliceMode 1 / SliceArgument (CTUs per slice); 0 = 1 slice */
  int transform_skip, transform_skip_fast, sign_hiding, strong_intra_smoothing;
  /* 0.0 => derive as HM does for an I slice (TEncSlice.cpp:686-706, 496-524); a P slice must give lambda (its GOP
   * entry's QP factor, fcu_ldp_slice), sqrt_lambda / chroma_weight / rdoq_lambda are then derived from it when left 0 */
  double lambda, sqrt_lambda, chroma_weight, rdoq_lambda[3];
  /* P slices (lowdelay_P, BASELINE configs[4]); all 0 in an I slice */
  int slice_type;                /* FCU_SLICE_I / FCU_SLICE_P: a P chain needs fcu_chain_set_reference                   */
  int search_range;              /* SearchRange in integer samples (64)                                                 */
  int fast_enc;                  /* FEN: every other row in the integer-search SAD of blocks taller than 8              */
  int hadamard_me;               /* HadamardME: SATD in the sub-sample refinement and the merge estimation              */
  int fast_merge_decision;       /* FDM                                                                                  */
  int max_merge_cand;            /* MaxNumMergeCand (5)                                                                  */
  int fast_search;               /* FastSearch: 0 = full search (xPatternSearch), 1 = TZ search (xTZSearch, HM's cfg default) */
  int tmvp;                      /* TMVPMode: temporal merge / AMVP candidate from the collocated picture = the reference picture
                                    (collocated_from_l0, collocated_ref_idx 0); needs fcu_chain_set_collocated                */
  int rdoq, rdoq_ts;             /* RDOQ / RDOQTS (fcu_default_frame_params: 1, 1): 0 = TComTrQuant::xQuant's plain quantiser with
                                    signBitHidingHDQ for blocks without / with transform skip */
  int amp;                       /* AMP: asymmetric motion partitions 2NxnU / 2NxnD / nLx2N / nRx2N at CU sizes 64..16, selected as
                                    HM does with AMP_ENC_SPEEDUP + AMP_MRG (TEncCu.cpp:381-450,836-943); part_size 4..7 in fcu_ctu_out */
  int cabac_b_table;             /* P slice: 1 = its contexts start from the B-slice tables (TComSlice::getEncCABACTableIdx() == B_SLICE
                                    with cabac_init_present_flag: TEncSbac::resetEntropy, TEncSbac.cpp:111-115 -- the choice
                                    TEncSbac::determineCabacInitIdx made after the previous slice, TEncSlice.cpp:1750-1753); 0 = the
                                    slice type's own tables */
} fcu_frame_params;
enum { FCU_SLICE_I = 0, FCU_SLICE_P = 1 };
#define FCU_REF_MARGIN_LUMA 80   /* border of a padded reference plane: g_uiMaxCUWidth + 16 (TComPic::create); chroma: 40 */

typedef struct fcu_ctx fcu_ctx;

void fcu_default_frame_params(fcu_frame_params *fp, int qp);
int  fcu_create(const fcu_seq_params *sp, fcu_ctx **out);
void fcu_destroy(fcu_ctx *c);
int  fcu_num_ctus(const fcu_ctx *c);
/* Bind a chain to its planes/output and reset it to CTU 0.  dev_out holds fcu_num_ctus() entries. */
int  fcu_chain_begin(fcu_ctx *c, int chain, const fcu_frame_params *fp,
                     const uint8_t *dev_org_y, const uint8_t *dev_org_u, const uint8_t *dev_org_v,
                     uint8_t *dev_rec_y, uint8_t *dev_rec_u, uint8_t *dev_rec_v,
                     fcu_ctu_out *dev_out);
/* P slice: the reference picture of the chain (list 0, index 0) = the previous picture after the loop filters, as padded
 * planes made by fcu_pad_reference (pointers to the first byte of each padded plane; luma stride = width + 2 * 80).
 * Slice QP and lambda of picture `poc` under HM's lowdelay_P GOP table come from fcu_ldp_slice. */
int  fcu_chain_set_reference(fcu_ctx *c, int chain, const uint8_t *dev_pad_y, const uint8_t *dev_pad_u, const uint8_t *dev_pad_v);
/* Several reference pictures (HM's lowdelay_P cfg lists four): RefPicList0[r] = dev_pad_planes[3r .. 3r+2] (padded Y, U, V of
 * fcu_pad_reference) at POC ref_pocs[r], r < n_ref <= FCU_MAX_REF; cur_poc = the picture being decided.  The search then loops
 * over the reference indices (TEncSearch::predInterSearch, TEncSearch.cpp:3110-3190), codes ref_idx, and scales neighbouring /
 * collocated vectors that point at another picture by the POC distances (TComDataCU::xGetDistScaleFactor, TComDataCU.cpp:3312).
 * The collocated picture of TMVP is RefPicList0[0]; name the POCs ITS list 0 referenced with fcu_chain_set_collocated_pocs
 * (default: one reference at its POC - 1). */
#define FCU_MAX_REF 4
int  fcu_chain_set_references(fcu_ctx *c, int chain, int n_ref, const uint8_t *const *dev_pad_planes, const int *ref_pocs, int cur_poc);
int  fcu_chain_set_collocated_pocs(fcu_ctx *c, int chain, int col_poc, const int *col_ref_pocs, int n);
/* TEncSearch::m_integerMv2Nx2N[REF_PIC_LIST_0][r] (TEncSearch.h:123; read and written at TEncSearch.cpp:3833-3842): the integer
 * vector of the last 2Nx2N TZ search on reference index r, an extra start point of the next search.  In HM it is a member of the
 * encoder that is never reset: it crosses CTUs, slices and pictures.  A chain carries it from CTU to CTU and, when one chain walks
 * several slices, from slice to slice; fcu_chain_begin starts it from zero.  A caller that runs slices or pictures one after the
 * other as HM does (the adapter) reads it with _get after a chain's last CTU and puts it back with _set after the next
 * fcu_chain_begin; slices decided side by side as independent chains cannot know the state the slice before them ends with and
 * start from zero -- which differs from HM only for a slice whose first CTU is too small for a 64x64 CU (otherwise the slice's
 * first search overwrites the state before anything reads it).  xy = { x0, y0, x1, y1, ... } for FCU_MAX_REF indices. */
int  fcu_chain_get_search_state(fcu_ctx *c, int chain, int32_t *xy);
int  fcu_chain_set_search_state(fcu_ctx *c, int chain, const int32_t *xy);
/* TMVP: the motion field of the chain's reference picture = the fcu_ctu_out array that picture was decided into (device
 * pointer, fcu_num_ctus() entries, kept alive by the caller).  What TComPic::compressMotion keeps (the top-left 4x4 partition
 * of every 16x16 block) is read in place; frame_params.tmvp switches the temporal candidates on (TComDataCU.cpp:2528-2563,
 * 2863-2900, xGetColMVP :3175-3242).  NULL: no collocated picture (every temporal candidate unavailable). */
int  fcu_chain_set_collocated(fcu_ctx *c, int chain, const fcu_ctu_out *dev_col_out);
/* Reference picture padding (TComPicYuv::extendPicBorder): copies the width x height planes into planes of
 * (width + 160) x (height + 160) luma / (width/2 + 80) x (height/2 + 80) chroma samples with the border replicated.
 * One kernel on `hip_stream`, asynchronous. */
int  fcu_pad_reference(fcu_ctx *c, const uint8_t *dev_y, const uint8_t *dev_u, const uint8_t *dev_v,
                       uint8_t *dev_pad_y, uint8_t *dev_pad_u, uint8_t *dev_pad_v, void *hip_stream);
/* bytes of the three padded planes of this sequence: out3[0] luma, out3[1] = out3[2] chroma */
void fcu_pad_sizes(const fcu_ctx *c, size_t *out3);
/* Slice type, QP and lambda of picture `poc` under HM's encoder_lowdelay_P_main GOP table (QP offsets 3,2,3,1; QP factors
 * 0.4624 x3, 0.578) as TEncSlice::initEncSlice derives them (TEncSlice.cpp:560-740): fills fp->qp / lambda / slice_type and the
 * configuration defaults (SearchRange 64, FEN, HadamardME, FDM, MaxNumMergeCand 5).  Pure host arithmetic. */
void fcu_ldp_slice(fcu_frame_params *fp, int base_qp, int poc);
/* pic->getSlice(0)->getDepth() of picture `poc` under that table (GOPSize 4; TEncSlice.cpp:236-262): 0, 2, 1, 2 for
 * poc % 4 = 0..3 -- the temporal layer fcu_sao_enabled / fcu_sao_update_rate key on */
int  fcu_ldp_layer(int poc);
/* Restrict a bound chain to the CTUs [first_ctu, first_ctu + n_ctus) of its frame.  Both ends must be slice
 * boundaries (frame_params.slice_ctus), where HM resets the entropy coder (TEncSlice.cpp:1392-1395) and masks the
 * neighbourhood (TComDataCU::getPULeft/Above): the slices of ONE frame then run as independent chains that share
 * the frame's planes and fcu_ctu_out array (disjoint writes) -- the way a single frame is spread over chains / GPUs. */
int  fcu_chain_set_range(fcu_ctx *c, int chain, int first_ctu, int n_ctus);
/* Advance chains [first, first+n) by up to `ctus` CTUs each (raster order; compressCtu +
 * encodeCtu replay per CTU).  Asynchronous on `hip_stream` (hipStream_t or NULL). */
int  fcu_compress_chains(fcu_ctx *c, int first, int n, int ctus, void *hip_stream);
/* ---- WaveFrontSynchro (WPP, entropy_coding_sync_enabled_flag; TEncSlice.cpp:1386-1411,1514-1517): the picture stays ONE
 * slice, so every earlier CTU stays available as a neighbour, and each CTU row restarts its contexts (resetEntropy) from the
 * state saved after the second CTU of the row above (contexts only; a one-CTU-wide picture keeps the plain reset).  Row r may
 * decide CTU x once row r-1 has finished CTU x+1: a picture of W x H CTUs is H chains with a critical path of W + 2(H-1) CTUs.
 * fcu_wpp_begin binds chains [first_chain, first_chain + fcu_wpp_rows(c)) to the CTU rows of ONE I picture, top to bottom (the
 * arguments of fcu_chain_begin; the rows share the planes and dev_out); fp->slice_type must be FCU_SLICE_I.  fcu_wpp_begin_p
 * takes the same arguments for ONE P picture; fp->slice_type must be FCU_SLICE_P.  Both need fp->slice_ctus 0 (WPP with
 * SliceMode 1 goes through fcu_wpp_begin_slices below; writing substreams / entry points is not supported); otherwise, or with
 * too few chains, FCU_ERR_ARG.
 * P pictures: after fcu_wpp_begin_p, set the reference pictures (fcu_chain_set_reference or _set_references, and
 * _set_collocated_pocs) and the collocated field (fcu_chain_set_collocated) on EVERY row chain, the same on each; set the search
 * state (fcu_chain_set_search_state: what the previous picture left) on ROW 0 only.  Call order per row: fcu_chain_set_decision
 * first (it rewrites the descriptor tail from the host copy, which resets the search state), the search state last.
 * HM's m_integerMv2Nx2N crosses the rows of the picture (it walks them in raster order); the launch reproduces that exactly:
 * a row whose first CTU is too small for a 64x64 CU waits for the whole row above and starts from its final search state, and
 * every row ends with the slots it did not write taken from the row above, so fcu_chain_get_search_state on the LAST row chain
 * returns HM's state after the picture (the next picture's row-0 state).  A row that begins on a full CTU writes every slot it
 * reads first (its depth-0 2Nx2N searches), so only the partial bottom row, or a picture narrower than 64, waits longer.
 * fcu_chain_set_decision, fcu_chain_set_pu_trace, fcu_get_verify_counts (rows added up in chain order), fcu_chain_position and
 * fcu_get_ctx_state (the state after the chain's row) work on row chains as on slice chains; fcu_compress_chains /
 * fcu_compress_ctu / fcu_chain_set_range on a row chain return FCU_ERR_STATE.
 * WaveFrontSynchro with SliceMode 1: fcu_wpp_begin_slices binds the same fcu_wpp_rows(c) chains to the CTU rows of ONE picture
 * cut into independent slices of slice_rows whole CTU rows (the last slice holds the rows that are left); fp->slice_type selects
 * I or P.  slice_rows >= 1; fp->slice_ctus 0 or exactly slice_rows x the picture width in CTUs, which is what the picture is
 * decided with; anything else (a slice that starts mid-row), or too few chains, FCU_ERR_ARG.  Every slice starts at a row start:
 *   - the first row of a slice is the first CTU of a slice AND a row start: the slice's reset, nothing loaded (the above-right CTU
 *     is in another slice), above neighbours unavailable.  It waits for nothing: it depends on nothing the slice above produced;
 *   - every other row of the slice follows the rules above with "row 0" read as "the first row of my slice";
 *   - every row saves its contexts after its second CTU.
 * A picture of W x H CTUs is H chains with a critical path of W + 2(slice_rows - 1) CTUs; slice_rows >= H decides what
 * fcu_wpp_begin(_p) decides.  P pictures: the setters as for fcu_wpp_begin_p, on every row.  The search state does not cross a
 * slice boundary: the first row of EVERY slice starts from its own descriptor (zero after binding -- this library's convention
 * for slices decided side by side -- unless fcu_chain_set_search_state put a state there), and fcu_chain_get_search_state on the
 * last row chain of a slice returns the state after that slice.  HM's raster walk would carry the state into the next slice;
 * that differs only for a slice whose first CTU is too small for a 64x64 CU. */
int  fcu_wpp_rows(const fcu_ctx *c);
int  fcu_wpp_begin(fcu_ctx *c, int first_chain, const fcu_frame_params *fp,
                   const uint8_t *dev_org_y, const uint8_t *dev_org_u, const uint8_t *dev_org_v,
                   uint8_t *dev_rec_y, uint8_t *dev_rec_u, uint8_t *dev_rec_v, fcu_ctu_out *dev_out);
int  fcu_wpp_begin_p(fcu_ctx *c, int first_chain, const fcu_frame_params *fp,
                     const uint8_t *dev_org_y, const uint8_t *dev_org_u, const uint8_t *dev_org_v,
                     uint8_t *dev_rec_y, uint8_t *dev_rec_u, uint8_t *dev_rec_v, fcu_ctu_out *dev_out);
int  fcu_wpp_begin_slices(fcu_ctx *c, int first_chain, const fcu_frame_params *fp, int slice_rows,
                          const uint8_t *dev_org_y, const uint8_t *dev_org_u, const uint8_t *dev_org_v,
                          uint8_t *dev_rec_y, uint8_t *dev_rec_u, uint8_t *dev_rec_v, fcu_ctu_out *dev_out);
/* Decide every row chain in [first, first + n) to the end, in one launch on `hip_stream`.  The range must hold whole pictures
 * bound by fcu_wpp_begin(_p), fcu_wpp_begin_slices or fcu_wpp_begin_tiles and not yet decided (else FCU_ERR_STATE, as for a chain not bound by fcu_wpp_begin; also for a P
 * row without a reference picture, or whose references or collocated field differ from its row 0's).  It may hold more
 * chains than the GPU keeps resident.  Returns when the launch has finished; FCU_ERR_STATE if a row gave up waiting for the
 * row above (a bounded wait of 120 s; the pictures of the launch are then undefined). */
int  fcu_compress_wpp(fcu_ctx *c, int first, int n, void *hip_stream);
/* ---- Tiles (NumTileColumnsMinus1 / NumTileRowsMinus1 with TileUniformSpacing 1; one slice per picture holding all tiles).
 * fcu_tile_grid: TComPicSym::initTiles -- tile column i spans the CTU columns [i * W / C, (i + 1) * W / C), rows likewise; col_bd
 * receives n_cols + 1 boundaries, row_bd n_rows + 1 (either may be NULL).  FCU_ERR_ARG for a grid with an empty tile (more columns
 * / rows than CTU columns / rows) or a count below 1.  Pure host arithmetic.
 * HM codes the CTUs in tile-scan order (tiles in raster order, CTUs raster inside a tile); the first CTU of every tile resets the
 * coder; a CTU of another tile is no neighbour (intra reference samples, MPMs, split / skip contexts, spatial merge and AMVP
 * candidates: TComDataCU::getPULeft ... getPUBelowLeft); motion vectors, the search window and motion compensation are NOT
 * restricted to the tile; end_of_slice_segment_flag is 1 at the last CTU of the picture only.  The tiles of a picture are
 * therefore independent chains, as slices are, and cut the picture in both directions.
 * fcu_tiles_begin binds chains [first_chain, first_chain + n_cols * n_rows) to the tiles of ONE I or P picture (fp->slice_type),
 * in tile-scan order; they share the planes and dev_out, and fcu_compress_chains advances them, each raster-in-tile.
 * fcu_wpp_begin_tiles binds one chain per (tile, CTU row of the tile), tiles in tile-scan order and the rows of a tile top to
 * bottom -- fcu_tile_chains(c, n_cols, n_rows, 1) = n_cols x the picture height in CTUs of them -- for fcu_compress_wpp: the
 * WaveFrontSynchro rules with "first / second CTU of the row" read inside the tile (tileXPosInCtus), a one-CTU-wide tile keeps the
 * plain reset, and a row only ever waits on the chain before it, inside its own tile.  4 x 2 uniform tiles of a 60 x 34 CTU
 * picture: critical path 15 + 2 * 16 = 47 CTU-times instead of 60 + 2 * 33 = 126.
 * fcu_tile_chains(c, n_cols, n_rows, wpp): chains either binding needs (-1: no such grid).
 * FCU_ERR_ARG: fp->slice_ctus != 0 (tiles together with SliceMode 1), a grid with an empty tile, too few chains, and fp->tmvp with
 * n_cols > 1 (HM's collocated bottom-right candidate reads across the tile edge).  Non-uniform spacing, tiles together with
 * SliceMode 1, B slices, substreams and entry points are not supported.  The loop filters of a tile picture are fcu_deblock_tiles
 * and fcu_sao_tiles below (fcu_deblock is the deblocking of LFCrossTileBoundaryFlag 1; fcu_sao's merge candidates would cross
 * tiles).
 * fcu_chain_set_decision, _set_pu_trace, fcu_get_ctx_state(_full), the reference / collocated / search-state setters (P: on EVERY
 * chain of the picture, the same on each) work on tile chains as on slice chains.  A tile chain's position (fcu_chain_position)
 * counts the CTUs decided INSIDE its tile; fcu_compress_ctu on a tile chain names the CTU by its picture address, in raster-in-tile
 * order; fcu_chain_set_range on a tile chain returns FCU_ERR_STATE.
 * The search state (m_integerMv2Nx2N) starts from zero in every tile -- this library's convention for units decided side by
 * side; HM's tile-scan walk would carry it from the tile before, which differs only for a tile whose first CTU is too small for
 * a 64x64 CU.  With WaveFrontSynchro it crosses the rows of a tile as it crosses the rows of a picture. */
int  fcu_tile_grid(int width_in_ctus, int height_in_ctus, int n_cols, int n_rows, int *col_bd, int *row_bd);
int  fcu_tile_chains(const fcu_ctx *c, int n_cols, int n_rows, int wpp);
int  fcu_tiles_begin(fcu_ctx *c, int first_chain, const fcu_frame_params *fp, int n_cols, int n_rows,
                     const uint8_t *dev_org_y, const uint8_t *dev_org_u, const uint8_t *dev_org_v,
                     uint8_t *dev_rec_y, uint8_t *dev_rec_u, uint8_t *dev_rec_v, fcu_ctu_out *dev_out);
int  fcu_wpp_begin_tiles(fcu_ctx *c, int first_chain, const fcu_frame_params *fp, int n_cols, int n_rows,
                         const uint8_t *dev_org_y, const uint8_t *dev_org_u, const uint8_t *dev_org_v,
                         uint8_t *dev_rec_y, uint8_t *dev_rec_u, uint8_t *dev_rec_v, fcu_ctu_out *dev_out);
/* HM-shaped call: decide CTU `ctuRsAddr` (must be the chain's next CTU) and copy its
 * TComDataCU arrays to host memory.  Synchronous. */
int  fcu_compress_ctu(fcu_ctx *c, int chain, uint32_t ctuRsAddr, fcu_ctu_out *host_out);
/* context state of m_pppcRDSbacCoder[0][CI_CURR_BEST] after the chain's last CTU:
 * 160 context bytes (engine order, see fcu_engine.h) + the Q15 fractional bit counter */
int  fcu_get_ctx_state(fcu_ctx *c, int chain, uint8_t *ctx160, uint64_t *frac_bits);
/* all 176 context states (160 residual / intra contexts + the inter syntax, engine order) + the Q15 counter */
int  fcu_get_ctx_state_full(fcu_ctx *c, int chain, uint8_t *ctx176, uint64_t *frac_bits);
int  fcu_chain_position(fcu_ctx *c, int chain);          /* next CTU to be decided */
int  fcu_sync(fcu_ctx *c);
/* average duration (ms) of the engine kernel launches recorded with HIP events on the launch
 * stream since the last call; resets the accumulator */
double fcu_kernel_ms(fcu_ctx *c, int *launches);
/* diagnostic counters of a chain: out17[0..15] section timers (shader clocks, -DFCU_PROFILE builds only),
 * out17[16] = TU trials so far */
int  fcu_debug_counters(fcu_ctx *c, int chain, unsigned long long *out17);
/* Fork pre-pass TEncSlice::getOutlierWithDCT (TEncSlice.cpp:878-1173, called per picture at TEncGOP.cpp:1096):
 * outlier-block-flag maps of n_frames luma planes (each width*height bytes, contiguous).  dev_obf receives
 * n_frames * (width/4)*(height/4) int16 counts (what xCompressCU reads at TEncCu.cpp:585-603); host_yc (may be
 * NULL) receives the 16 per-frequency TCM thresholds of every frame; kernel_ms2 (may be NULL) the durations of
 * the histogram and the counting kernel.  Synchronous (the threshold fit runs on the host between the kernels). */
int  fcu_obf_prepass(fcu_ctx *c, int n_frames, const uint8_t *dev_y, int16_t *dev_obf, double *host_yc,
                     float *kernel_ms2, void *hip_stream);
/* The host step of fcu_obf_prepass on its own: TCMprocessOneSequence (TEncSlice.cpp:343-392) on the histogram of
 * |coefficient / 8| of one frequency (hist[a] = samples of amplitude a, n_samples in total); returns the threshold Yc.
 * Pure host arithmetic (doubles + libm, as the reference); needs no GPU. */
double fcu_tcm_threshold(const unsigned *hist, int hist_len, int n_samples);
/* ---- the fork's fast CU-size decision (its default control: Naive model on the N_OBF feature, YSGlobalControl,
 * tools_YS.cpp:4-58).  A chain starts in FCU_TRAINING (exhaustive RDO).  FCU_VERIFYING is exhaustive too and counts,
 * per depth, how the Naive label ("split" when the CU holds an outlier block, "do not split" when it holds none)
 * compares with the RDO outcome.  FCU_TESTING prunes: at a depth whose sw_skip2nx2n is on, a CU labelled "split" skips
 * its 2Nx2N check; at a depth whose sw_terminate is on, a CU labelled "do not split" is not divided further (at depth 3:
 * NxN is not tried).  dev_obf is the frame's map from fcu_obf_prepass ((height/4) x (width/4) int16). */
enum { FCU_TRAINING = 0, FCU_VERIFYING = 1, FCU_TESTING = 2 };      /* CurrentState, getCurrentState tools_YS.cpp:1237 */
typedef struct fcu_decision_params {
  int state;
  int depth_exception;           /* g_bDepthException (tools_YS.cpp:25): no pruning of depth-3 CUs that hold outliers */
  uint8_t sw_skip2nx2n[4];       /* g_bDecisionSwitch[depth][Naive][Skip2Nx2N]   */
  uint8_t sw_terminate[4];       /* g_bDecisionSwitch[depth][Naive][TerminateCU] */
  const int16_t *dev_obf;
} fcu_decision_params;
/* g_iVerResult[depth][Naive][TP, FP, TN, FN, FPLoss, FNLoss] (globals_YS.h:81-89) */
typedef struct fcu_verify_counts { double n[4][6]; } fcu_verify_counts;
/* Set the decision state of a bound chain (any time between launches) and clear its verification counters. */
int  fcu_chain_set_decision(fcu_ctx *c, int chain, const fcu_decision_params *dp);
/* Sum of the verification counters of chains [first, first+n), added up in chain order.  Synchronous. */
int  fcu_get_verify_counts(fcu_ctx *c, int first, int n, fcu_verify_counts *host_sum);
/* SetDecisionSwitch (tools_YS.cpp:1123-1154): a switch turns on when the precision of its label on the Verifying frame
 * exceeds the threshold (0 => the reference's default 0.8).  Pure host arithmetic. */
void fcu_decision_switch(const fcu_verify_counts *v, const double th_skip[4], const double th_term[4],
                         uint8_t sw_skip2nx2n[4], uint8_t sw_terminate[4]);
/* getCurrentState (tools_YS.cpp:1237-1242) for picture `poc` with g_iP = period, g_iT = n_training, g_iV = n_verifying
 * (reference defaults 60 / 2 / 1, tools_YS.cpp:41-43) */
int  fcu_frame_state(int poc, int period, int n_training, int n_verifying);
/* In-loop deblocking of a completely decided I or P picture, in place on its reconstruction planes:
 * TComLoopFilter::loopFilterPic (TComLoopFilter.cpp:130-155) as TEncGOP::compressGOP runs it after the last slice of the
 * picture (TEncGOP.cpp:1155-1160), with the encoder's default control -- filter enabled, LFCrossSliceBoundaryFlag 1
 * (TAppEncCfg.cpp:813-818,848-849; either value of that flag: fcu_deblock_slices) -- and the slice's beta / tc offsets (div 2,
 * -6..6).  It knows no tiles: for a tile picture
 * it is the filter of LFCrossTileBoundaryFlag 1 (HM's default); either value of that flag: fcu_deblock_tiles.
 * dev_out is the picture's fcu_ctu_out array (depth, part_size, tr_idx and qp are read).  Two kernels on `hip_stream`;
 * asynchronous unless kernel_ms2 is given, which then receives the durations of the vertical- and horizontal-edge pass. */
int  fcu_deblock(fcu_ctx *c, const fcu_ctu_out *dev_out, uint8_t *dev_rec_y, uint8_t *dev_rec_u, uint8_t *dev_rec_v,
                 int beta_offset_div2, int tc_offset_div2, float *kernel_ms2, void *hip_stream);
/* fcu_deblock of a picture cut into n_cols x n_rows uniform tiles (fcu_tile_grid) with LFCrossTileBoundaryFlag = lf_cross_tiles:
 * 1 filters the tile boundaries like any other CTU boundary (what fcu_deblock does); 0 leaves every edge that lies on a tile
 * boundary unfiltered, luma and chroma, as the picture border is (TComLoopFilter.cpp:379,401,430-434,609-613,754-758) -- the tiles
 * can then be filtered independently.  A 1 x 1 grid is fcu_deblock byte for byte.  FCU_ERR_ARG: a grid fcu_tile_grid refuses,
 * lf_cross_tiles outside {0, 1}, a picture beyond 256 CTUs in either direction, and what fcu_deblock refuses. */
int  fcu_deblock_tiles(fcu_ctx *c, const fcu_ctu_out *dev_out, uint8_t *dev_rec_y, uint8_t *dev_rec_u, uint8_t *dev_rec_v,
                       int beta_offset_div2, int tc_offset_div2, int n_cols, int n_rows, int lf_cross_tiles,
                       float *kernel_ms2, void *hip_stream);
/* fcu_deblock of a picture of SliceMode 1 slices -- slice_ctus consecutive CTUs in raster order each, the last one what is
 * left; a slice may start mid-row; 0, or the picture's CTU count and more, is one slice -- with LFCrossSliceBoundaryFlag =
 * lf_cross_slices for all of them (TEncGOP.cpp:763).  1 filters a slice boundary like any other CTU boundary (what fcu_deblock
 * does); with 0 a partition on the left / top edge of its CTU gets no edge flag when the CTU to the left / above lies in another
 * slice, luma and chroma, as on the picture border (TComLoopFilter.cpp:369-411,430-434,609-613,754-758; TComDataCU::getPULeft /
 * getPUAbove) -- the slices can then be filtered independently.  lf_cross_slices 1, or one slice, is fcu_deblock byte for byte
 * (and runs its kernels).  The slice length is the whole description: no limit on the picture beyond fcu_deblock's.
 * FCU_ERR_ARG: lf_cross_slices outside {0, 1}, a negative slice_ctus, and what fcu_deblock refuses. */
int  fcu_deblock_slices(fcu_ctx *c, const fcu_ctu_out *dev_out, uint8_t *dev_rec_y, uint8_t *dev_rec_u, uint8_t *dev_rec_v,
                        int beta_offset_div2, int tc_offset_div2, int slice_ctus, int lf_cross_slices,
                        float *kernel_ms2, void *hip_stream);
/* ---- sample adaptive offset --------------------------------------------------------------------------------------
 * SAOOffset / SAOBlkParam of the reference (TypeDef.h:760-800) narrowed to bytes: mode 0 off / 1 new / 2 merge;
 * type: edge class 0..3 or 4 = band offset for a new mode, 0 = left / 1 = above for a merge; band = band position;
 * offset[class]: EO offsets at [0,1,3,4] (class 2 is always 0), BO offsets at [band .. band+3] (mod 32). */
typedef struct { int8_t mode, type, band, pad; int8_t offset[32]; } fcu_sao_offset;
typedef struct { fcu_sao_offset c[3]; } fcu_sao_ctu;                    /* Y, Cb, Cr */
typedef struct {
  int32_t slice_type;        /* FCU_SLICE_I / FCU_SLICE_P: context initialisation of the SAO syntax */
  int32_t qp;                /* slice QP */
  int32_t slice_ctus;        /* SliceArgument (0 = one slice): merge candidates do not cross slices; fcu_sao_slices: nor do samples */
  int32_t enabled[3];        /* slice-level switches (fcu_sao_enabled) */
  double  lambda[3];         /* TComSlice::getLambdas(): lambda, lambda / chroma weight (x2); [1], [2] = 0: derived from [0] and the QP (chroma QP offsets 0) */
} fcu_sao_params;
/* TEncSampleAdaptiveOffset::SAOProcess (TEncSampleAdaptiveOffset.cpp:257-287; TEncGOP.cpp:1427-1441, SaoCtuBoundary 0) of
 * n_pics completely decided and deblocked pictures of this context's size, in place on their reconstruction planes.
 * dev_org / dev_rec: host arrays of 3 * n_pics device pointers (Y, U, V of picture 0, then picture 1 ...);
 * dev_coded: device array [n_pics][num_ctus] receiving the parameters as signalled (what the adapter stores into
 * TComPicSym::getSAOBlkParam()); off_count (host, 3 * n_pics, may be NULL): CTUs whose reconstructed mode is off, per
 * component -- the input of fcu_sao_update_rate.  Four kernels on `hip_stream`; the call returns after they have finished
 * (off_count and kernel_ms4 -- statistics, candidates, decision, offset pass -- are read back).  No CPU fallback. */
int  fcu_sao(fcu_ctx *c, int n_pics, const fcu_sao_params *params, const uint8_t *const *dev_org, uint8_t *const *dev_rec,
             fcu_sao_ctu *dev_coded, int32_t *off_count, float *kernel_ms4, void *hip_stream);
/* fcu_sao of pictures cut into n_cols x n_rows uniform tiles (one grid for the batch: a context has one picture size) with
 * LFCrossTileBoundaryFlag = lf_cross_tiles.  For either value a merge candidate exists only inside the CTU's tile: left iff the
 * CTU is not in the first column of its tile, above iff not in its first row (TComPic::getSAOMergeAvailability, TComPic.cpp:
 * 138-143); decideBlkParams still walks the CTUs in raster order over the picture and carries its contexts across the tile
 * boundaries.  With lf_cross_tiles 0 a CTU of another tile is also unavailable to the statistics and to the offset pass in all
 * eight directions (TComPicSym::deriveLoopFilterBoundaryAvailibility, TComPicSym.cpp:378,449-459); with 1 sample availability is
 * the picture border as in fcu_sao.  A 1 x 1 grid is fcu_sao byte for byte.  FCU_ERR_ARG: a grid fcu_tile_grid refuses,
 * lf_cross_tiles outside {0, 1}, any params[i].slice_ctus != 0 (tiles with SliceMode 1), a picture beyond 256 CTUs in either
 * direction, and what fcu_sao refuses. */
int  fcu_sao_tiles(fcu_ctx *c, int n_pics, const fcu_sao_params *params, int n_cols, int n_rows, int lf_cross_tiles,
                   const uint8_t *const *dev_org, uint8_t *const *dev_rec, fcu_sao_ctu *dev_coded, int32_t *off_count,
                   float *kernel_ms4, void *hip_stream);
/* fcu_sao with LFCrossSliceBoundaryFlag = lf_cross_slices; each picture's slices are its params[i].slice_ctus (as for
 * fcu_deblock_slices; pictures of one batch may differ).  The decision is fcu_sao's for either value: merge candidates stay
 * inside the slice, the walk and the coder cross slices.  With lf_cross_slices 0 a neighbour CTU is available to the offset pass
 * iff it is inside the picture and in the CTU's slice, each of the eight directions on its own -- once a slice starts or ends
 * mid-row a diagonal is not the conjunction of its sides (TComPicSym::deriveLoopFilterBoundaryAvailibility, TComPicSym.cpp:
 * 357-447) --, and the statistics take left, above and above-left that way and keep right and below, with the margins they skip,
 * at the picture border (TEncSampleAdaptiveOffset.cpp:327-336).  lf_cross_slices 1, or one slice in every picture, is fcu_sao
 * byte for byte (and runs its kernels).  FCU_ERR_ARG: lf_cross_slices outside {0, 1} and what fcu_sao refuses (a negative
 * slice_ctus among it). */
int  fcu_sao_slices(fcu_ctx *c, int n_pics, const fcu_sao_params *params, int lf_cross_slices,
                    const uint8_t *const *dev_org, uint8_t *const *dev_rec, fcu_sao_ctu *dev_coded, int32_t *off_count,
                    float *kernel_ms4, void *hip_stream);
/* decidePicParams (:363-395): enabled[comp] = 0 when the picture's temporal layer is > 0 and the share of SAO-off CTUs in
 * layer - 1 exceeded 0.75 (luma) / 0.5 (chroma).  rate = m_saoDisabledRate[3][8], zero-initialised by the caller per sequence. */
void fcu_sao_enabled(const double rate[3][8], int layer, int32_t enabled[3]);
/* the bookkeeping at the end of decideBlkParams (:895-917) */
void fcu_sao_update_rate(double rate[3][8], int layer, const int32_t off_count[3], int num_ctus);

/* ---- the picture report: what the encoder prints per picture (TEncGOP::xCalculateAddPSNR, TEncGOP.cpp:2195-2290) and what a user
 * of the fast decision looks at -- quality, rate, and how the picture was partitioned -- taken where the picture is, in HBM.
 * The counters are in units of 4x4 luma partitions and count only partitions inside the picture (a partial CTU's entries
 * outside it are ignored whatever they hold): n_part = partitions inside; depth_part[d] = partitions of CU depth d (a depth above
 * 3 is counted nowhere); part_size_part[s] = partitions of PartSize s = 2Nx2N, 2NxN, Nx2N, NxN, 2NxnU, 2NxnD, nLx2N, nRx2N (another
 * value is counted nowhere); intra_part = pred_mode 1; skip_part / merge_part = skip / merge_flag non-zero; cbf_part[c] = bit 0
 * (the CU level) of cbf of Y, Cb, Cr.  ssd[c] = sum over the plane's samples inside the picture of (org - rec)^2; bits / bins /
 * dist = total_bits / total_bins / total_dist of the CTU's record, per picture their sums.  Neither structure has implicit padding. */
typedef struct fcu_ctu_report {
  uint32_t ssd[3], bits, bins, dist;                       /* ssd <= 4096 * 255^2 per CTU */
  uint16_t n_part, depth_part[4], part_size_part[8], intra_part, skip_part, merge_part, cbf_part[3], pad;
} fcu_ctu_report;
typedef struct fcu_pic_report {
  uint64_t ssd[3], bits, bins, dist, n_samples[3];         /* n_samples: width x height, and a quarter of it for Cb and Cr */
  uint32_t n_part, depth_part[4], part_size_part[8], intra_part, skip_part, merge_part, cbf_part[3], pad;
  double   psnr[3];                                        /* ssd ? 10 log10(255 * 255 * n_samples / ssd) : 999.99 (TEncGOP.cpp:2254-2256), in double precision on the host */
} fcu_pic_report;
/* Report of n_pics pictures of this context's size.  dev_org / dev_rec: host arrays of 3 * n_pics device pointers (Y, U, V of
 * picture 0, then picture 1 ...), as for fcu_sao; any byte alignment (16-byte aligned planes of a width that is a multiple of
 * 16 take wider loads); dev_out: host array of n_pics device pointers, each picture's fcu_ctu_out array (only the per-partition
 * arrays in front of the coefficients and the totals at the end are read).  host_reports receives n_pics records.  dev_ctu
 * (device, [n_pics][fcu_num_ctus], or NULL: a buffer of the context) receives the per-CTU records.  Nothing is modified but the
 * outputs; no atomics and no buffer that must be cleared: the same input gives the same bytes.  Two kernels on `hip_stream`; the
 * call returns after they have finished and the reports are on the host; kernel_ms2 (may be NULL) receives their durations.
 * FCU_ERR_ARG: n_pics < 1, a NULL array, a NULL entry of one, NULL host_reports.  No CPU fallback. */
int  fcu_picture_report(fcu_ctx *c, int n_pics, const uint8_t *const *dev_org, const uint8_t *const *dev_rec,
                        const fcu_ctu_out *const *dev_out, fcu_pic_report *host_reports, fcu_ctu_report *dev_ctu,
                        float *kernel_ms2, void *hip_stream);

/* ---- the picture hash: the decoded-picture hash of HM (SEIDecodedPictureHash 1 / 2 / 3; calcMD5, calcCRC, calcChecksum of
 * TComPicYuvMD5.cpp:44-207) of reconstructed pictures, taken where they are, in HBM -- what the encoder prints as ` [MD5:...]`,
 * ` [CRC:...]` or ` [Checksum:...]` at the end of a picture line (TEncGOP.cpp:1742-1756).  Every plane is hashed on its own, in
 * the order Y, Cb, Cr:
 *   MD5       RFC 1321 over the plane's width x height bytes in raster order
 *   CRC       16 bits, polynomial 0x1021, initial state 0xffff, the bits of every sample shifted in at the low end MSB first,
 *             sixteen zero bits flushed at the end
 *   checksum  the sum mod 2^32 over the samples of sample ^ (uint8)((x & 255) ^ (y & 255) ^ (x >> 8) ^ (y >> 8))
 * The record holds the bytes in HM's digest order (crc and checksum high byte first): the hex of the bytes is HM's string. */
enum { FCU_HASH_MD5 = 1, FCU_HASH_CRC = 2, FCU_HASH_CHECKSUM = 4 };   /* bit mask; HM's SEIDecodedPictureHash 1 / 2 / 3 */
typedef struct fcu_pic_hash { uint8_t md5[3][16], crc[3][2], checksum[3][4], pad[2]; } fcu_pic_hash;      /* 68 B, no implicit padding */
/* Hashes of n_pics pictures of this context's size.  dev_planes: host array of 3 * n_pics device pointers (Y, U, V of picture
 * 0, then picture 1 ...); planes are dense (stride = width) and may start at any byte (16-byte aligned planes take 16-byte
 * loads).  kinds: the mask of the hashes wanted; only those are computed, the fields of the others are zero.  host_hashes
 * receives n_pics records.  Nothing is modified but the outputs; no atomics and no buffer that must be cleared: the same input
 * gives the same bytes.  CRC and checksum share one pass over the samples (one kernel that leaves a partial result per 16 KiB of
 * a plane, one that folds them); MD5 is a third kernel (one lane per plane: a serial chain of 64-byte blocks), launched only
 * when asked for.  The call returns after they have finished and the records are on the host; kernel_ms3 (may be NULL)
 * receives the durations of the three kernels, 0 for one that was not launched.
 * FCU_ERR_ARG, with the argument named in fcu_last_error(): n_pics < 1, kinds 0 or with other bits, a NULL dev_planes, a NULL
 * entry of it, a NULL host_hashes.  No CPU fallback. */
int  fcu_picture_hash(fcu_ctx *c, int n_pics, int kinds, const uint8_t *const *dev_planes, fcu_pic_hash *host_hashes,
                      float *kernel_ms3, void *hip_stream);
/* digestToString (TComPicYuvMD5.cpp:209-225) of one kind of a record: the three planes' digests in hex, joined by ','.  Pure
 * host.  Returns the length of the string; FCU_ERR_ARG for a kind that is not exactly one of the three bits or a buffer too
 * short for the string and its terminator (MD5 needs 99 bytes). */
int  fcu_hash_string(const fcu_pic_hash *h, int kind, char *buf, int buf_len);

/* ---- decision maps: the decision of whole pictures as rasters aligned with the pixels, formed where the records lie, in HBM.
 * With W4 = width / 4, H4 = height / 4 and, for level d = 0..3 of the quadtree, s = 64 >> d, BW(d) = ceil(width / s),
 * BH(d) = ceil(height / s), NL = sum over d of BW(d) * BH(d):
 *   byte maps     uint8 [n_pics][n_fields][H4][W4]: entry (y4, x4) of map k is the byte fcu_ctu_out.<field_ids[k]> holds for the
 *                 4x4 partition at luma (4 x4, 4 y4) -- z-order undone; signed fields (part_size, pred_mode, qp, mvp_idx, ref_idx)
 *                 keep their byte.  Only the arrays named are read.
 *   motion map    int16 [n_pics][H4][W4][2] from fcu_ctu_out.mv ([hor, ver], quarter samples)
 *   label maps    int8 [n_pics][NL]: per picture the four levels one after the other, level d as [BH(d)][BW(d)] at element offset
 *                 sum over e < d of BW(e) * BH(e).  Entry (by, bx) of level d describes the s x s block at luma (bx s, by s), from
 *                 depth (and, at d = 3, part_size) of the block's top-left partition -- an FCU_LABEL_* code.  These are the split
 *                 flags of the CUs ON THE CHOSEN TREE (what TEncCu::xEncodeCU codes, TEncCu.cpp:1679-1699; at d = 3 the choice
 *                 SIZE_NxN of the 8x8 CU).  The fork's Training dump (tools_YS.cpp:304-318, written at TEncCu.cpp:1489-1497) also
 *                 labels the CUs its exhaustive search visited and discarded; those are not in fcu_ctu_out and get no label.
 *   N_OBF maps    uint16 [n_pics][NL], the layout of the label maps: the fork's feature of that block (TEncCu.cpp:585-600) -- the
 *                 number of 4x4 blocks of the block's area inside the picture whose count in the OBF map of fcu_obf_prepass is > 0.
 * Entries of a record that belong to partitions outside the picture reach no output. */
enum { FCU_MAP_DEPTH = 0, FCU_MAP_PART_SIZE, FCU_MAP_PRED_MODE, FCU_MAP_SKIP, FCU_MAP_MERGE_FLAG, FCU_MAP_MERGE_IDX, FCU_MAP_TR_IDX,
       FCU_MAP_CBF_Y, FCU_MAP_CBF_CB, FCU_MAP_CBF_CR, FCU_MAP_TSKIP_Y, FCU_MAP_TSKIP_CB, FCU_MAP_TSKIP_CR, FCU_MAP_INTRA_DIR_LUMA,
       FCU_MAP_INTRA_DIR_CHROMA, FCU_MAP_QP, FCU_MAP_INTER_DIR, FCU_MAP_MVP_IDX, FCU_MAP_REF_IDX, FCU_MAP_FIELDS };
enum { FCU_LABEL_ABSENT = -1,      /* depth < d: the parent was not split, there is no CU of this size here                       */
       FCU_LABEL_NOT_SPLIT = 0,    /* a CU of depth d that was not split (split_cu_flag 0); at d = 3: part_size is not NxN        */
       FCU_LABEL_SPLIT = 1,        /* depth > d (split_cu_flag 1); at d = 3: part_size NxN                                       */
       FCU_LABEL_FORCED = 2 };     /* d < 3 and the block does not lie wholly inside the picture: split without a coded flag
                                      (bBoundary, TEncCu.cpp:486-488,1694-1699); the fork never labels these CUs                             */
/* Maps of n_pics decided pictures of this context's size.  dev_out: host array of n_pics device pointers, each picture's fcu_ctu_out
 * array.  field_ids: n_fields distinct FCU_MAP_* ids, in the order of the maps (n_fields 0: no byte maps).  dev_bytes, dev_mv,
 * dev_labels, dev_nobf: device outputs of the shapes above, NULL = not wanted; dev_bytes may start at any byte (rows go out as 16-byte
 * units when W4 is a multiple of 16 and the base is 16-byte aligned, else as 2-byte units), dev_mv and dev_nobf at any even byte.
 * dev_obf: host array of n_pics device pointers, each picture's OBF map (int16 [H4][W4] of fcu_obf_prepass); given exactly when dev_nobf
 * is.  Nothing is modified but the outputs; every output byte is written by exactly one thread, no atomics and no buffer that must be
 * cleared: the same input gives the same bytes.  One kernel on `hip_stream`; the call returns after it has finished; kernel_ms (may be
 * NULL) receives its duration.
 * FCU_ERR_ARG, with the argument named in fcu_last_error(): n_pics < 1; a NULL dev_out or entry of it; n_fields outside
 * 0..FCU_MAP_FIELDS; n_fields > 0 with a NULL field_ids or a NULL dev_bytes, and dev_bytes with n_fields 0; an unknown or repeated
 * field id; dev_nobf without dev_obf and the reverse, a NULL entry of dev_obf; no output wanted at all.  No CPU fallback. */
int  fcu_decision_maps(fcu_ctx *c, int n_pics, const fcu_ctu_out *const *dev_out, int n_fields, const int *field_ids,
                       uint8_t *dev_bytes, int16_t *dev_mv, int8_t *dev_labels, const int16_t *const *dev_obf, uint16_t *dev_nobf,
                       float *kernel_ms, void *hip_stream);
/* ---- split match: how far two decisions A and B of the same picture agree (a Testing-state picture against its exhaustive
 * decision).  part_total = 4x4 partitions inside the picture; part_equal = those whose depth is equal
 * in A and B; node[d][a][b] = blocks of level d that are a CU with a coded flag in both (label a in A, b in B; 0 = not split,
 * 1 = split: the diagonal agrees); only_a[d] / only_b[d] = blocks that are such a CU in one decision and absent in the other.
 * Forced blocks (FCU_LABEL_FORCED) are counted nowhere.  Neither structure has implicit padding. */
typedef struct fcu_ctu_match { uint16_t part_total, part_equal, node[4][2][2], only_a[4], only_b[4], pad[6]; } fcu_ctu_match;   /* 64 B */
typedef struct fcu_pic_match { uint64_t part_total, part_equal, node[4][2][2], only_a[4], only_b[4]; } fcu_pic_match;           /* 208 B */
/* dev_out_a / dev_out_b: host arrays of n_pics device pointers to fcu_ctu_out arrays (only depth and part_size are read);
 * host_matches receives n_pics records; dev_ctu (device, [n_pics][fcu_num_ctus], or NULL: a buffer of the context) the per-CTU
 * records.  Two kernels on `hip_stream` (one record per CTU, then 64-bit sums per picture); no atomics, nothing to clear; the call
 * returns after they have finished; kernel_ms2 (may be NULL) receives their durations.  FCU_ERR_ARG: n_pics < 1, a NULL array, a NULL
 * entry of one, NULL host_matches. */
int  fcu_split_match(fcu_ctx *c, int n_pics, const fcu_ctu_out *const *dev_out_a, const fcu_ctu_out *const *dev_out_b,
                     fcu_pic_match *host_matches, fcu_ctu_match *dev_ctu, float *kernel_ms2, void *hip_stream);

/* ---- caller-supplied split labels: a model of the caller's in the place of the Naive model on N_OBF.  The engine's only predictor is
 * "N_OBF > 0" on the OBF map; a caller that trained another model on the label maps of fcu_decision_maps runs it wherever it likes
 * and hands its prediction back as ONE label array per picture, int8 [NL] in the layout of the label maps above, in HBM:
 *   FCU_LABEL_SPLIT      the fork's Skip2Nx2N label ("will be divided")
 *   FCU_LABEL_NOT_SPLIT  its TerminateCU label
 *   any other value (FCU_LABEL_ABSENT and FCU_LABEL_FORCED among them): no prediction -- the CU is searched exhaustively and is
 *                        not counted in the Verifying state.
 * A CU of depth d at luma (x, y) reads element off(d) + (y / s) * BW(d) + x / s, s = 64 >> d: picture coordinates, so the slice
 * chains, WaveFrontSynchro rows and tile chains of a picture all take the picture's one array.  A CU the picture edge cuts reads no
 * label (it is split without a decision, as before).  Everything else of the decision block stays as fcu_chain_set_decision set
 * it: the state, sw_skip2nx2n / sw_terminate per depth, and depth_exception, which with labels bound reads "no pruning of depth-3
 * CUs labelled FCU_LABEL_SPLIT".  The label array an OBF map would give (N_OBF > 0 -> SPLIT, else NOT_SPLIT) decides bit for bit
 * what that OBF map decides.
 * fcu_chain_set_labels binds dev_labels (fcu_label_count() bytes, kept alive and unchanged by the caller while the chain runs) to a
 * bound chain, NULL unbinds; fcu_chain_begin and the picture binders start a chain without labels, fcu_chain_set_decision leaves
 * the binding as it is.  With labels bound the OBF map is never read, and fcu_chain_set_decision accepts FCU_VERIFYING / FCU_TESTING
 * with a NULL dev_obf.  Call order: after fcu_chain_set_decision when that call names an OBF map (the labels then take its place);
 * without an OBF map bind the labels while the chain is in FCU_TRAINING -- the state fcu_chain_begin leaves -- and set the state
 * after.  Only the label fields of the descriptor are copied: position, coder state, counters and search state on the device stay.
 * FCU_ERR_ARG: a bad chain index; FCU_ERR_STATE: a chain that is not bound, and unbinding (NULL) from a chain in FCU_VERIFYING /
 * FCU_TESTING that has no OBF map (it would have nothing to predict from). */
int  fcu_chain_set_labels(fcu_ctx *c, int chain, const int8_t *dev_labels);
/* NL of this context's picture size: elements of one picture's label array (and of its N_OBF maps) */
int  fcu_label_count(const fcu_ctx *c);
/* Label arrays from rasters: the inverse of the label half of fcu_decision_maps.  dev_depth: uint8 [n_pics][H4][W4], the CU depth per
 * 4x4 partition (the byte map FCU_MAP_DEPTH; the form partition models predict); dev_part_size: int8 [n_pics][H4][W4] (FCU_MAP_PART_SIZE)
 * or NULL; dev_labels: int8 [n_pics][NL].  Block (by, bx) of level d looks at the partition at its top-left corner: depth < d ->
 * FCU_LABEL_ABSENT; else, d < 3 and the block not wholly inside the picture -> FCU_LABEL_FORCED; else d < 3: depth > d -> FCU_LABEL_SPLIT,
 * depth == d -> FCU_LABEL_NOT_SPLIT; d = 3: part_size NxN (3) -> FCU_LABEL_SPLIT, else (and always with a NULL dev_part_size)
 * FCU_LABEL_NOT_SPLIT.  On the maps of a decided picture this gives the bytes fcu_decision_maps gives.  All three arrays may start at
 * any byte.  Every output byte is written by exactly one thread, no atomics, nothing to clear: the same input gives the same bytes.
 * One kernel on `hip_stream`, asynchronous.  FCU_ERR_ARG: n_pics < 1, a NULL dev_depth or dev_labels. */
int  fcu_labels_from_rasters(fcu_ctx *c, int n_pics, const uint8_t *dev_depth, const int8_t *dev_part_size, int8_t *dev_labels, void *hip_stream);

/* ---- CU trace: both RD costs of every CU the search visits.  The label maps of fcu_decision_maps cover the CUs on the chosen tree;
 * the fork's Training dump (tools_YS.cpp:304-318) also holds the CUs its search visited and discarded, and the two costs its
 * FPLoss / FNLoss are made of: J0, the best cost of the CU coded whole, and J1, the cost of the CU split (TEncCu.cpp:1450-1451; at
 * depth 3 the cost of SIZE_NxN, :1175-1183).  Optional side output of the ordinary decision, like fcu_pu_trace: bind a device array of
 * fcu_num_ctus() * FCU_CUS_PER_CTU records to a chain and every CU closed from then on is recorded at [ctu][fcu_cu_index], in every
 * decision state.  The decisions themselves do not change.
 *   valid        1 for a CU that lies wholly inside the picture and was visited.  A CU the picture edge cuts is never recorded, nor
 *                is a CU below a parent that was not divided (Testing state: TerminateCU).
 *   whole_tried  1 when the whole-CU best cost is a real cost (0: Skip2Nx2N pruned the check; j0 is then FCU_MAX_DOUBLE)
 *   j0           that cost including the split flag (FCU_MAX_DOUBLE when whole_tried is 0)
 *   split_tried  depth < 3: the four sub-CUs were searched; depth 3: SIZE_NxN was tried
 *   j1           the cost of the split / of NxN; 0.0 when split_tried is 0
 *   split_won    the split (NxN) won: the fork's bPartition_True; 0 when split_tried is 0
 * A chain with a trace bound clears the 85 records of a CTU when it starts that CTU: the caller clears nothing, and a picture
 * decided twice into the same array gives the same bytes.  The slice, row and tile chains of a picture are given the same array
 * and write disjoint CTUs.  fcu_chain_begin and the picture binders start a chain without a trace; NULL stops recording; only the
 * pointer is copied to the device: position, coder state, counters, search state and labels stay.  FCU_ERR_ARG: a bad chain
 * index; FCU_ERR_STATE: a chain that is not bound. */
#define FCU_CUS_PER_CTU 85            /* 1 + 4 + 16 + 64 CUs of depth 0..3 */
#define FCU_MAX_DOUBLE 1.7e+308       /* HM's MAX_DOUBLE (TypeDef.h): the cost of a CU that was not evaluated */
typedef struct fcu_cu_trace {         /* 24 B, no implicit padding */
  double  j0, j1;
  uint8_t valid, split_won, whole_tried, split_tried, pad[4];
} fcu_cu_trace;
/* = fcu_pu_index(depth, 0, zidx): layer offsets 0 / 1 / 5 / 21, inside a layer the CUs in z-order */
int  fcu_cu_index(int depth, int zidx);
int  fcu_chain_set_cu_trace(fcu_ctx *c, int chain, fcu_cu_trace *dev_trace);

/* ---- label score: the Verifying counters (g_iVerResult) of ANY label array against the trace of an exhaustively decided picture,
 * without deciding the picture again.  Every record with valid and split_tried set is a sample: its label is read from the picture's
 * label array (int8 [NL], the layout of the label maps, the addressing of fcu_chain_set_labels: off(d) + (y / s) * BW(d) + x / s at
 * picture coordinates) and counted as countTFPN + countRDLoss count it (tools_YS.cpp:968-986): FCU_LABEL_SPLIT predicts 1,
 * FCU_LABEL_NOT_SPLIT 0, the truth is split_won, fabs(j0 - j1) is added to FPLoss / FNLoss of a wrong prediction.  Any other label
 * value is no prediction: counted in open[d] and nowhere else.  scored[d] = samples of depth d that had a prediction.
 * v holds the six counters per depth in the order of fcu_verify_counts: &score.v goes straight into fcu_decision_switch.
 * Two kernels, no atomics, nothing to clear.  One wave per CTU forms the fcu_ctu_score: counts from ballots, n[d] = TP, FP, TN, FN;
 * loss[d] = FPLoss, FNLoss, each the sum over the CUs of depth d IN Z-ORDER, one term after the other from 0.0 (a CU that adds
 * nothing to a sum adds nothing, not 0.0).  One lane per (picture, depth, counter) then adds the CTU records IN RASTER ORDER from
 * 0.0.  The order is part of the interface (double sums do not commute).  Against the engine's own Verifying counters of the same
 * labels: the counts are equal; the losses are bit for bit equal when every chain is one CTU, else equal to 1e-9 relative.
 * (A P picture has depth-3 CUs whose SIZE_NxN is never tried; the Verifying state counts them with J1 = 0 as the fork does, the
 * score does not -- split_tried is 0 -- so there it is short of the Verifying counters at depth 3 by exactly those CUs.)
 * dev_trace / dev_labels: host arrays of n_pics device pointers; host_scores receives n_pics records; dev_ctu (device,
 * [n_pics][fcu_num_ctus], or NULL: a buffer of the context) the per-CTU records.  The call returns after the kernels have finished;
 * kernel_ms2 (may be NULL) receives their durations.  FCU_ERR_ARG, with the argument named in fcu_last_error(): n_pics < 1, a NULL
 * array, a NULL entry of one, NULL host_scores.  Neither structure has implicit padding.  No CPU fallback. */
typedef struct fcu_ctu_score { uint16_t n[4][4], open[4], pad[12]; double loss[4][2]; } fcu_ctu_score;   /* 128 B */
typedef struct fcu_pic_score { fcu_verify_counts v; uint32_t open[4], scored[4]; } fcu_pic_score;       /* 224 B */
int  fcu_label_score(fcu_ctx *c, int n_pics, const fcu_cu_trace *const *dev_trace, const int8_t *const *dev_labels,
                     fcu_pic_score *host_scores, fcu_ctu_score *dev_ctu, float *kernel_ms2, void *hip_stream);

/* ---- trace maps: the trace as the fork's whole Training set, in the layout of the label and N_OBF maps of fcu_decision_maps.
 * dev_labels int8 [n_pics][NL], dev_j0 / dev_j1 double [n_pics][NL]; each may be NULL, at least one is wanted.  Block (by, bx) of
 * level d: FCU_LABEL_FORCED for d < 3 and a block not wholly inside the picture; FCU_LABEL_ABSENT for a block whose record has valid 0
 * or split_tried 0; else split_won.  j0 / j1: the record's costs, 0.0 where the label is ABSENT or FORCED.  Element for element
 * aligned with the N_OBF map: (feature, label, J0, J1) of every visited CU, with no host pass.  One kernel; every output element is
 * written by exactly one thread, nothing to clear.  dev_labels may start at any byte, dev_j0 / dev_j1 at multiples of 8.  The call
 * returns after the kernel has finished; kernel_ms (may be NULL) receives its duration.  FCU_ERR_ARG, argument named: n_pics < 1, a
 * NULL dev_trace or entry of it, no output wanted, a misaligned cost array. */
int  fcu_trace_maps(fcu_ctx *c, int n_pics, const fcu_cu_trace *const *dev_trace,
                    int8_t *dev_labels, double *dev_j0, double *dev_j1, float *kernel_ms, void *hip_stream);

/* ---- feature maps: the inputs of a partition model, per block of the label / N_OBF maps above and row for row aligned with them:
 * (X, label, J0, J1) of a Training picture are device arrays with no host pass.  The fork dumps these next to every Training label
 * (TEncCu.cpp:1558-1579).  dev_features is float32 [n_pics][NL][F]: block (by, bx) of level d (s = 64 >> d, luma (bx s, by s)) is row
 * off(d) + by BW(d) + bx; a block that does not lie wholly inside the picture gets a row of zeros (the fork forms features only
 * under !bBoundary, TEncCu.cpp:1525).  The columns of FCU_FEATSET_TMV come first, then those of FCU_FEATSET_SOC.
 *
 * TMV, column f * 26 + k: getTMVFeature (tools_YS.cpp:1682-1839).  For the W x W samples p[i][j] of the block (W = s, i = row,
 * j = column) filter f gives a W x W plane q that is ZERO on its one-sample border ring -- the ring of this CU, not of the picture,
 * and the identity filter has it too (T3x3Filter::filter, :1659-1672) -- and, for 1 <= i, j <= W - 2,
 *   f = 0  p[i][j]                    f = 1  p[i][j-1] - p[i][j+1]          f = 2  p[i-1][j] - p[i+1][j]
 *   f = 3  p[i-1][j+1] - p[i+1][j-1]  f = 4  p[i-1][j-1] - p[i+1][j+1]      (masks :1693-1697)
 * so a block's features depend on its own samples only.  A rectangle R of N elements with sum S has mean = S / N and "variance" =
 * (sum over R of |trunc(q - mean)|) / N, truncation toward zero (getSubBlockMean / getSubBlockVariance, tools_YS.h:106-126).  The
 * four triangles hold W (W + 1) / 2 elements each but divide by W W / 2, and their "variance" loop ASSIGNS instead of adding
 * (`iVariance =`, :1749-1811): it is |trunc(q_last - mean)| / (W W / 2) for the last element of the loop, which always lies on the
 * zero ring, i.e. floor(|mean|) / (W W / 2).
 *   k = 0 / 1           mean / variance of the whole block
 *   k = 2, 3 / 4, 5     means / variances of rows [0, W/2) and rows [W/2, W)
 *   k = 6, 7 / 8, 9     ... of columns [0, W/2) and columns [W/2, W)
 *   k = 10, 11 / 12, 13 ... of the triangles j < W - i and j >= W - i - 1
 *   k = 14, 15 / 16, 17 ... of the triangles j >= i and j <= i
 *   k = 18, 19, 20, 21 / 22, 23, 24, 25   ... of the top-left quadrant, the top-right quadrant, THE BOTTOM HALF (rows [W/2, W), all
 *                       columns: the fork passes (0, uiCuWidth) as the column range of its third "quadrant", :1823-1825, so k = 20 /
 *                       24 repeat k = 3 / 5) and the bottom-right quadrant.
 * Every divisor is a power of two and |S| <= 4096 * 255, so every value is an integer below 2^24 times a power of two: float32
 * holds the fork's doubles exactly, and the kernel is integer-only, |trunc(q - S/N)| = |q N - S| >> log2 N.  No floating-point
 * ordering enters the interface.
 *
 * SOC, column k = y * 4 + x (after the TMV columns when both sets are asked for): FormFeatureVector, Type SOC
 * (tools_YS.cpp:379-396), on the Outlier plane of getOutlierWithDCT (TEncSlice.cpp:1057-1132) with REVERSETRANSFORM_OUTLIER 0 and
 * BINARIZE_OUTLIER 0 (TypeDef.h:126-127): the plane holds |coef| / 100 (integer division) at the coefficient's position in its 4x4
 * block, for the coefficients the pre-pass keeps as outliers and 0 for the others.  SOC[k] = sum over the 4x4 blocks of the CU of
 * |coef[k]| / 100 where coefficient k (frequency k of fcu_obf_prepass, k = 1..15) is an outlier: coef != 0 and |coef| >= (int)(Yc[k] * 8),
 * the test and the threshold of fcu_obf_prepass, one function for both.  SOC[0] (DC) is 0.  host_yc: double [n_pics][16], the Yc
 * fcu_obf_prepass returned for each picture (entry 0 is not read).  Sums stay below 2^24: exact in float32.
 * The fork's SUBSOC of a depth-d CU (:397-444) is the SOC of its four sub-blocks: the rows of the blocks
 * (2 by, 2 bx), (2 by, 2 bx + 1), (2 by + 1, 2 bx), (2 by + 1, 2 bx + 1) of level d + 1, in that order; it is not emitted a second
 * time (and SOC of level d is the sum of those four rows).
 * Out of scope: the OBF / EOBF patches and Outlier / BOutlier are crops of maps the caller can already form (fcu_obf_prepass, the
 * luma plane); OBF_SATD* carries only the patch -- its SATD / RDCost lines are commented out in the fork; the models themselves.
 *
 * dev_y: host array of n_pics device pointers to dense width x height luma planes, each may start at any byte (a plane on an
 * 8-byte boundary is read with 8-byte loads).  dev_features: 4-byte aligned.  One kernel on `hip_stream`, one workgroup per CTU; every
 * output element, the zero rows included, is written by exactly one thread, no atomics, nothing to clear: the same input gives
 * the same bytes.  The call returns after the kernel has finished; kernel_ms (may be NULL) receives its duration.
 * FCU_ERR_ARG, with the argument named in fcu_last_error(): n_pics < 1; sets 0 or with other bits; a NULL dev_y or entry of it;
 * FCU_FEATSET_SOC without host_yc and host_yc without it; a negative or non-finite Yc; a NULL or misaligned dev_features.
 * No CPU fallback. */
enum { FCU_FEATSET_TMV = 1, FCU_FEATSET_SOC = 2 };
#define FCU_FEAT_TMV 130
#define FCU_FEAT_SOC 16
/* F of a set mask: 130, 16 or 146; FCU_ERR_ARG for any other mask */
int  fcu_feature_count(int sets);
int  fcu_feature_maps(fcu_ctx *c, int n_pics, int sets, const uint8_t *const *dev_y, const double *host_yc,
                      float *dev_features, float *kernel_ms, void *hip_stream);

/* ---- risk-table model: a model between fcu_trace_maps and fcu_chain_set_labels that is trained and run on the device.
 * The fork's BayesDecision (tools_YS.cpp:709-725) looks up two risks by the CU's N_OBF, R0 = g_dJdx01[depth][x] and
 * R1 = g_dJdx10[depth][x], and predicts TerminateCU when R0 < R1, Skip2Nx2N otherwise; BayesNew sizes the tables {257, 65, 17, 5}
 * per depth (:906).  The decision rule and the table sizes are the fork's.  The fork never fills the tables (g_dJdx01 has no
 * definition in its tree): the training rule below is this library's.
 *   sample   a trace record with valid, split_tried and whole_tried all set (the samples of fcu_label_score whose j0 is a real
 *            cost, never FCU_MAX_DOUBLE).  A CU the picture edge cuts has no record and is no sample.
 *   key      the record of CTU a, depth d, z-index z is the block at off(d) + (y / s) * BW(d) + x / s of the label-map layout (the
 *            addressing of fcu_trace_maps and fcu_chain_set_labels); its key is the uint16 at that element of the picture's key
 *            array, uint16 [NL] -- the N_OBF map (fcu_decision_maps, fcu_nobf_maps) or any feature of the caller's quantised to
 *            0..256.  A sample whose key is >= FCU_RISK_BINS is dropped and counted in `dropped`.
 *   q        the quantised loss (int64) floor(fabs(j0 - j1) * 256.0), clamped to 2^40 - 1; a value that is not < 2^40, NaN
 *            included, gives 2^40 - 1.  The multiplication is exact and fabs is countRDLoss' (tools_YS.cpp:980-986).
 *   model    risk[d][x][t] = sum of q, count[d][x][t] = number, over the samples of depth d and key x with split_won == t.
 *            risk[d][x][0] is what predicting SPLIT on bin x loses (its not-split samples become false positives: FPLoss),
 *            risk[d][x][1] what predicting NOT_SPLIT loses (FNLoss).
 *   rule     FCU_LABEL_NOT_SPLIT iff risk[d][x][1] < risk[d][x][0], else FCU_LABEL_SPLIT (a tie gives SPLIT: the fork's
 *            R0 < R1 -> -1, else +1); a bin with count[d][x][0] + count[d][x][1] < min_count gives FCU_LABEL_ABSENT, no
 *            prediction.  min_count 0 is the fork's rule on every bin: an empty bin predicts SPLIT.
 * Every accumulated quantity is an integer: sums commute, so the model is the same bytes whatever order the kernels visit the
 * records in, and no tolerance, iteration count or summation order enters the interface.  Capacity: q < 2^40, so 2^23 samples per
 * bin before a sum could wrap -- the caller's to respect across accumulating calls; one call takes at most 2^22 blocks
 * (n_pics * NL).  The structure has no implicit padding and lives in HBM at a multiple of 8 bytes.
 *
 * fcu_risk_train: dev_trace / dev_keys are host arrays of n_pics device pointers (a picture's fcu_cu_trace array and its key array).
 * accumulate 0: dev_model is overwritten -- the caller clears nothing; accumulate 1: the batch is added to what dev_model holds:
 * pictures A then B with accumulate 1 give the bytes of [A, B] in one call.  host_dropped (may be NULL) receives the samples this
 * call dropped.  Two kernels: one pass over the records, every workgroup adding its samples into a table of its own in LDS (integer
 * LDS adds) and storing it to its slot of a context buffer; then one thread per table entry adds the slots and writes, or adds to,
 * dev_model.  No global atomics, nothing to clear: a repeated call gives identical bytes.  The call returns after the kernels have
 * finished; kernel_ms2 (may be NULL) receives their durations.
 * fcu_risk_predict: dev_labels int8 [n_pics][NL], ready for fcu_chain_set_labels: a block the picture edge cuts (d < 3) gets
 * FCU_LABEL_FORCED whatever its key (the rule of fcu_trace_maps), a key >= FCU_RISK_BINS gets FCU_LABEL_ABSENT, everything else the
 * rule above.  dev_model is read on the device; one kernel, one thread per block, every output byte written by exactly one
 * thread; the call returns after it has finished, kernel_ms (may be NULL) receives its duration.
 * fcu_nobf_maps: the N_OBF map uint16 [n_pics][NL] of pictures that have not been decided (a Testing picture's keys are needed
 * before its fcu_ctu_out exists): the bytes fcu_decision_maps(..., dev_obf, dev_nobf) gives.  One kernel on `hip_stream`, one thread per block;
 * the call returns after it has finished.
 * fcu_risk_table: the rule on a host copy of a model (host arithmetic, needs no GPU).
 * FCU_ERR_ARG, with the argument named in fcu_last_error(): n_pics < 1; a NULL array or a NULL entry of one; a NULL or misaligned
 * dev_model; dev_keys / dev_nobf at an odd byte; a negative min_count; n_pics * NL > 2^22 (fcu_risk_train).  No CPU fallback. */
#define FCU_RISK_BINS 257            /* N_OBF of a 64x64 CU is 0..256 */
#define FCU_RISK_Q_MAX ((int64_t)1099511627775)      /* 2^40 - 1 */
#define FCU_RISK_MAX_BLOCKS (1 << 22)                /* n_pics * NL of one fcu_risk_train call */
typedef struct fcu_risk_model {      /* 24 672 B, no implicit padding; lives in HBM, 8-byte aligned */
  int64_t  risk [4][FCU_RISK_BINS][2];   /* [depth][key][truth]: sum of q over the samples of that bin whose split_won == truth */
  uint32_t count[4][FCU_RISK_BINS][2];   /* samples of that bin with split_won == truth */
} fcu_risk_model;
int  fcu_risk_train(fcu_ctx *c, int n_pics, const fcu_cu_trace *const *dev_trace, const uint16_t *const *dev_keys,
                    fcu_risk_model *dev_model, int accumulate, uint32_t *host_dropped, float *kernel_ms2, void *hip_stream);
int  fcu_risk_predict(fcu_ctx *c, int n_pics, const uint16_t *const *dev_keys, const fcu_risk_model *dev_model, int min_count,
                      int8_t *dev_labels, float *kernel_ms, void *hip_stream);
int  fcu_nobf_maps(fcu_ctx *c, int n_pics, const int16_t *const *dev_obf, uint16_t *dev_nobf, void *hip_stream);
void fcu_risk_table(const fcu_risk_model *host_model, int min_count, int8_t table[4][FCU_RISK_BINS]);

/* ---- key tree: risk-table keys learnt from the feature maps.  One small decision tree per CU depth over the quantised columns
 * of fcu_feature_maps; its leaf index is the uint16 key of fcu_risk_train / fcu_risk_predict.  The fork's tree model type is
 * RTS_OpenCV (CvRTrees_model, globals_YS.h:124): OpenCV's random trees, an external library.  Nothing below is the fork's: bins,
 * tree, histograms and the split rule are this library's, as the training rule of the risk table is.  Every quantity is an
 * integer, every result is the same bytes in any order of evaluation.
 * F = fcu_feature_count(sets); rows, NL, off(d), BW(d) and the block addressing are those of the label maps.
 *   bins     edges is float32 [4][F][FCU_TREE_BINS - 1]: per (level d of the NL layout, column) 31 finite, non-decreasing values.
 *            The bin of x is the number of edges e with e <= x, 0..31; NaN compares false and gives bin 0.  Equal edges are
 *            allowed and leave bins unreachable.  A row of level d uses edges[d].
 *   tree     fcu_key_tree: per depth d a complete binary tree in heap order (node i has children 2 i + 1 and 2 i + 2), `levels`
 *            (0..5) deep, so at most 32 leaves.  feature[d][i] is the column node i splits on, or -1 for a node that is not
 *            split; thr[d][i] is 0..30.  The walk of a row of level d starts at node 0 and takes exactly `levels` steps: at a
 *            split node it goes right iff bin[feature] > thr, at an unsplit node left.  key = the heap index reached -
 *            (2^levels - 1), in [0, 2^levels).  levels 0: key 0 everywhere.
 *   hist     sample and quantised loss q are exactly those of fcu_risk_train (valid, split_tried and whole_tried all set;
 *            q = floor(|j0 - j1| * 256) clamped to 2^40 - 1), one function for both; the record of CTU a, depth d, z-index z is the
 *            row fcu_risk_train reads its key from.  risk is int64 [4][2^level][F][32][2], count uint32 of the same shape: cell
 *            [d][n][f][b][t] = the sum of q, respectively the number, over the samples of depth d in node n whose bin of column f
 *            is b and whose split_won is t.  Capacity as for the risk model: 2^23 samples per cell, 2^22 blocks per call.
 *   split    for depth d and node n with total risks R[t]: L[t](f, b) = the cell risks of column f summed over bins <= b;
 *            loss(f, b) = min(L[0], L[1]) + min(R[0] - L[0], R[1] - L[1]) -- what the best label per child loses, the quantity
 *            the risk table's rule minimises.  Candidates: b in 0..30 with at least max(1, min_count) samples in both children.
 *            The smallest loss wins, ties go to the smallest f, then the smallest b; the node is split only if that loss is
 *            strictly below min(R[0], R[1]), else feature = -1 (and thr = 0).
 *
 * fcu_feature_edges_check: FCU_OK for a host copy of edges ([4][F][31]) whose rows are finite and non-decreasing, else FCU_ERR_ARG
 * with the row named.  Edges formed on the device are the caller's to get right; fcu_feature_bins reads them as they are.
 * fcu_feature_bins: dev_features float32 [n_pics][NL][F] (4-byte aligned) -> dev_bins uint8 [n_pics][NL][F], which may start at any
 * byte.  One kernel, a workgroup inside one level with that level's edges in LDS; every output byte is written by exactly one
 * thread.  The bin is found by a 5-step search over the row of edges, which equals the count above for non-decreasing edges.
 * fcu_tree_keys: dev_bins as fcu_feature_bins wrote it -> dev_keys uint16 [n_pics][NL] at any even byte.  levels <= tree->levels:
 * a smaller value walks only that many steps and gives the node-in-level index that training needs.  One kernel, one thread per
 * block; a block the picture edge cuts walks its zero row like any other.
 * fcu_tree_hist: the histograms of `level` (0..4).  dev_trace / dev_bins: host arrays of n_pics device pointers (a picture's trace
 * and its uint8 [NL][F] bins); dev_nodes: host array of n_pics device pointers to uint16 [NL], the output of
 * fcu_tree_keys(levels = level), may be NULL at level 0 (node 0 everywhere).  accumulate 0 overwrites every cell -- the caller
 * clears nothing --, accumulate 1 adds: A then B equals [A, B].  A sample whose node index is >= 2^level is dropped and counted
 * (once, not per column) in host_dropped[0] (may be NULL).  Two kernels as fcu_risk_train: workgroups add into LDS tables of their
 * own (integer LDS adds) and store them to slots of a context buffer, a second kernel folds the slots, one thread per cell.  No
 * global atomics: a repeated call gives identical bytes.  kernel_ms2 (may be NULL) receives the two durations.
 * fcu_tree_split: pure host integer arithmetic, needs no GPU: fills the nodes of `level` from a host copy of that level's
 * histograms and leaves the rest of the tree alone (the caller sets tree->levels).  The totals of a node are the same whichever
 * column they are summed over: FCU_ERR_ARG when they are not (a histogram of another shape, F or level).
 * fcu_tree_train: for each level l < levels: keys of l levels, histograms, copy to the host (at most 7.2 MB), split.  Uses
 * buffers of the context, synchronous as fcu_obf_prepass; pictures, features and traces stay on the device.  host_tree is
 * overwritten: levels, every node (-1 / 0 below the trained levels).  kernel_ms (may be NULL): the kernels' durations added up.
 * FCU_ERR_ARG, with the argument named in fcu_last_error(): n_pics < 1; a bad sets, level or levels; NULL arrays or entries;
 * misaligned dev_features / dev_keys / dev_nodes / dev_risk / dev_count; a tree whose levels, features or thresholds are out of
 * range; n_pics * NL > 2^22.  No CPU fallback. */
#define FCU_TREE_BINS 32
#define FCU_TREE_MAX_LEVELS 5
#define FCU_TREE_NODES 31            /* internal nodes of a depth's tree, heap order */
typedef struct fcu_key_tree {        /* 376 B, no implicit padding (already a multiple of 8) */
  int32_t levels;                        /* 0..FCU_TREE_MAX_LEVELS */
  int16_t feature[4][FCU_TREE_NODES];    /* [depth][node]: column, or -1 for a node that is not split */
  uint8_t thr[4][FCU_TREE_NODES];        /* right iff bin[feature] > thr; 0..30 */
} fcu_key_tree;
int  fcu_feature_edges_check(const float *host_edges, int sets);
int  fcu_feature_bins(fcu_ctx *c, int n_pics, int sets, const float *dev_features, const float *dev_edges, uint8_t *dev_bins,
                      float *kernel_ms, void *hip_stream);
int  fcu_tree_keys(fcu_ctx *c, int n_pics, int sets, const uint8_t *dev_bins, const fcu_key_tree *host_tree, int levels,
                   uint16_t *dev_keys, float *kernel_ms, void *hip_stream);
int  fcu_tree_hist(fcu_ctx *c, int n_pics, int sets, int level, const fcu_cu_trace *const *dev_trace, const uint8_t *const *dev_bins,
                   const uint16_t *const *dev_nodes, int64_t *dev_risk, uint32_t *dev_count, int accumulate, uint32_t *host_dropped,
                   float *kernel_ms2, void *hip_stream);
int  fcu_tree_split(const int64_t *host_risk, const uint32_t *host_count, int F, int level, int min_count, fcu_key_tree *tree);
int  fcu_tree_train(fcu_ctx *c, int n_pics, int sets, int levels, int min_count, const fcu_cu_trace *const *dev_trace,
                    const uint8_t *const *dev_bins, fcu_key_tree *host_tree, float *kernel_ms, void *hip_stream);

/* ---- per-PU record of the luma search (BASELINE configs[1]: intra-luma RDO, TEncSearch::estIntraPredLumaQT over the 35
 * modes at all depths).  Exhaustive RDO visits every PU of the five layers of a CTU -- 1 + 4 + 16 + 64 PUs of 2Nx2N CUs at
 * depth 0..3 and 256 PUs of NxN CUs at depth 3 = 341 -- and estIntraPredLumaQT (TEncSearch.cpp:2178-2655) leaves per PU: the
 * RMD survivors with their SATD costs (CandCostList, :2289-2336), the candidate list after the MPM additions (:2407-2428),
 * the winning mode, its luma distortion and RD cost after the full-RQT re-run (:2518-2586).  Optional side output of the
 * ordinary decision: bind a device array of fcu_num_ctus() * FCU_PUS_PER_CTU records to a chain and every PU searched
 * from then on is recorded at [ctu][fcu_pu_index]; PUs outside the picture or pruned by the fork's Testing state stay
 * valid = 0.  The decisions themselves do not change. */
#define FCU_PUS_PER_CTU 341
typedef struct fcu_pu_trace {
  uint8_t  valid;            /* 1 once the PU has been searched                                    */
  uint8_t  best_mode;        /* luma intra direction of the PU                                     */
  uint8_t  n_rmd;            /* RMD survivors (g_aucIntraModeNumFast: 8, 8, 3, 3, 3 for 4..64)     */
  uint8_t  n_rd;             /* full-RD candidates after the MPM additions                         */
  uint8_t  rd_mode[12];      /* the candidates in test order                                       */
  uint32_t best_dist;        /* luma SSE of the winner                                             */
  uint32_t pad;
  double   best_cost;        /* its RD cost                                                        */
  double   rmd_cost[8];      /* CandCostList of the survivors: SATD + sqrt(lambda) * mode bits     */
} fcu_pu_trace;
/* layer offsets 0 / 1 / 5 / 21 (2Nx2N CUs at depth 0..3) and 85 (NxN PUs); zidx = z-order index of the PU's first 4x4 partition */
int  fcu_pu_index(int depth, int nxn, int zidx);
int  fcu_chain_set_pu_trace(fcu_ctx *c, int chain, fcu_pu_trace *dev_trace);

/* diagnostic: chains (one-wave workgroups of the engine kernel) the runtime keeps resident per compute unit */
int  fcu_chains_per_cu(void);
/* text of the calling thread's last failure (one buffer per host thread) */
const char *fcu_last_error(void);
/* compiler version and the exact flags libfcu.so was built with.  The engine relies on
 * `-mllvm -amdgpu-remove-redundant-endcf=false`: a build without it is refused by tests/test_cabi.py. */
const char *fcu_build_info(void);
/* sizeof() of the ABI's structures as this library was compiled, by FCU_ABI_* index (-1 for an unknown index): a binding
 * in another language (ctypes, cgo, JNI) checks its own layouts against them before the first call; tests/test_cabi.py does. */
enum { FCU_ABI_CTU_OUT = 0, FCU_ABI_SEQ_PARAMS = 1, FCU_ABI_FRAME_PARAMS = 2, FCU_ABI_DECISION_PARAMS = 3, FCU_ABI_VERIFY_COUNTS = 4,
       FCU_ABI_SAO_CTU = 5, FCU_ABI_SAO_PARAMS = 6, FCU_ABI_PU_TRACE = 7, FCU_ABI_PIC_REPORT = 8, FCU_ABI_CTU_REPORT = 9,
       FCU_ABI_PIC_HASH = 10, FCU_ABI_CTU_MATCH = 11, FCU_ABI_PIC_MATCH = 12, FCU_ABI_CU_TRACE = 13, FCU_ABI_CTU_SCORE = 14,
       FCU_ABI_PIC_SCORE = 15, /* 16 is not assigned and stays unknown */ FCU_ABI_RISK_MODEL = 17, FCU_ABI_KEY_TREE = 18 };
int  fcu_abi_sizeof(int which);

#ifdef __cplusplus
}
#endif
#endif
