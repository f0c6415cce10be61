"""Host side of the engine: ctypes binding of libfcu.so and a `TEncCu`-shaped class.

The reference boundary is the C++ class `TEncCu` (Lib/TLibEncoder/TEncCu.h:104-118):
create / init / compressCtu / encodeCtu / destroy, called once per CTU by
`TEncSlice::compressSlice` (TEncSlice.cpp:1380-1551).  `CuEngine` keeps those names and
their meaning; the batched form (`compress_chains`) is what a throughput-oriented caller uses.

torch is plumbing only (device buffers, streams); the arithmetic is in the HIP kernels.
The module raises if libfcu.so is missing or no GPU is present: there is no CPU fallback.
"""
import ctypes as C
import os

import numpy as np

from .layout import PictureLayout

_HERE = os.path.dirname(os.path.abspath(__file__))
NPART = 256


class FcuError(RuntimeError):
    pass


class FrameParams(C.Structure):
    """fcu_frame_params (include/fcu.h)."""
    _fields_ = [("qp", C.c_int), ("slice_ctus", C.c_int), ("transform_skip", C.c_int),
                ("transform_skip_fast", C.c_int), ("sign_hiding", C.c_int), ("strong_intra_smoothing", C.c_int),
                ("lambda_", C.c_double), ("sqrt_lambda", C.c_double), ("chroma_weight", C.c_double),
                ("rdoq_lambda", C.c_double * 3),
                ("slice_type", C.c_int), ("search_range", C.c_int), ("fast_enc", C.c_int), ("hadamard_me", C.c_int),
                ("fast_merge_decision", C.c_int), ("max_merge_cand", C.c_int), ("fast_search", C.c_int), ("tmvp", C.c_int), ("rdoq", C.c_int), ("rdoq_ts", C.c_int), ("amp", C.c_int), ("cabac_b_table", C.c_int)]


class SeqParams(C.Structure):
    _fields_ = [("width", C.c_int), ("height", C.c_int), ("max_chains", C.c_int), ("device", C.c_int)]


class CtuOut(C.Structure):
    """fcu_ctu_out: the TComDataCU arrays published by copyToPic (TComDataCU.h:72-164)."""
    _fields_ = [("depth", C.c_uint8 * NPART), ("width", C.c_uint8 * NPART), ("height", C.c_uint8 * NPART),
                ("skip", C.c_uint8 * NPART), ("part_size", C.c_int8 * NPART), ("pred_mode", C.c_int8 * NPART),
                ("tq_bypass", C.c_uint8 * NPART), ("qp", C.c_int8 * NPART), ("chroma_qp_adj", C.c_uint8 * NPART),
                ("tr_idx", C.c_uint8 * NPART), ("tskip", (C.c_uint8 * NPART) * 3), ("cbf", (C.c_uint8 * NPART) * 3),
                ("intra_dir", (C.c_uint8 * NPART) * 2), ("ipcm", C.c_uint8 * NPART),
                ("merge_flag", C.c_uint8 * NPART), ("merge_idx", C.c_uint8 * NPART), ("inter_dir", C.c_uint8 * NPART),
                ("mvp_idx", C.c_int8 * NPART), ("ref_idx", C.c_int8 * NPART),
                ("mv", (C.c_int16 * 2) * NPART), ("mvd", (C.c_int16 * 2) * NPART),
                ("coeff_y", C.c_int32 * 4096), ("coeff_cb", C.c_int32 * 1024), ("coeff_cr", C.c_int32 * 1024),
                ("total_cost", C.c_double), ("total_dist", C.c_uint32), ("total_bits", C.c_uint32),
                ("total_bins", C.c_uint32)]


CTU_OUT_BYTES = C.sizeof(CtuOut)

TRAINING, VERIFYING, TESTING = 0, 1, 2          # CurrentState (getCurrentState, tools_YS.cpp:1237-1242)


class SaoOffset(C.Structure):
    _fields_ = [("mode", C.c_int8), ("type", C.c_int8), ("band", C.c_int8), ("pad", C.c_int8), ("offset", C.c_int8 * 32)]


class SaoCtu(C.Structure):
    _fields_ = [("c", SaoOffset * 3)]


class SaoParams(C.Structure):
    _fields_ = [("slice_type", C.c_int32), ("qp", C.c_int32), ("slice_ctus", C.c_int32), ("enabled", C.c_int32 * 3), ("lambda_", C.c_double * 3)]


SAO_CTU_BYTES = C.sizeof(SaoCtu)


class DecisionParams(C.Structure):
    """fcu_decision_params (include/fcu.h): frame state, Naive switches per depth, the frame's OBF map."""
    _fields_ = [("state", C.c_int), ("depth_exception", C.c_int), ("sw_skip2nx2n", C.c_uint8 * 4),
                ("sw_terminate", C.c_uint8 * 4), ("dev_obf", C.c_void_p)]


class CtuReport(C.Structure):
    """fcu_ctu_report: SSD per plane, bits / bins / distortion and the partition counters of one CTU."""
    _fields_ = [("ssd", C.c_uint32 * 3), ("bits", C.c_uint32), ("bins", C.c_uint32), ("dist", C.c_uint32),
                ("n_part", C.c_uint16), ("depth_part", C.c_uint16 * 4), ("part_size_part", C.c_uint16 * 8), ("intra_part", C.c_uint16),
                ("skip_part", C.c_uint16), ("merge_part", C.c_uint16), ("cbf_part", C.c_uint16 * 3), ("pad", C.c_uint16)]


class PicReport(C.Structure):
    """fcu_pic_report: the sums over a picture's CTUs, the sample counts and the PSNR per plane."""
    _fields_ = [("ssd", C.c_uint64 * 3), ("bits", C.c_uint64), ("bins", C.c_uint64), ("dist", C.c_uint64), ("n_samples", C.c_uint64 * 3),
                ("n_part", C.c_uint32), ("depth_part", C.c_uint32 * 4), ("part_size_part", C.c_uint32 * 8), ("intra_part", C.c_uint32),
                ("skip_part", C.c_uint32), ("merge_part", C.c_uint32), ("cbf_part", C.c_uint32 * 3), ("pad", C.c_uint32),
                ("psnr", C.c_double * 3)]


CTU_REPORT_DTYPE = np.dtype([("ssd", np.uint32, (3,)), ("bits", np.uint32), ("bins", np.uint32), ("dist", np.uint32),
                             ("n_part", np.uint16), ("depth_part", np.uint16, (4,)), ("part_size_part", np.uint16, (8,)), ("intra_part", np.uint16),
                             ("skip_part", np.uint16), ("merge_part", np.uint16), ("cbf_part", np.uint16, (3,)), ("pad", np.uint16)])   # fcu_ctu_report
PIC_REPORT_DTYPE = np.dtype([("ssd", np.uint64, (3,)), ("bits", np.uint64), ("bins", np.uint64), ("dist", np.uint64), ("n_samples", np.uint64, (3,)),
                             ("n_part", np.uint32), ("depth_part", np.uint32, (4,)), ("part_size_part", np.uint32, (8,)), ("intra_part", np.uint32),
                             ("skip_part", np.uint32), ("merge_part", np.uint32), ("cbf_part", np.uint32, (3,)), ("pad", np.uint32),
                             ("psnr", np.float64, (3,))])                                                                   # fcu_pic_report


def pic_report_to_dict(rec):
    """one element of a PIC_REPORT_DTYPE array -> dict of numpy scalars and arrays (`pad` dropped)"""
    return {n: (rec[n].copy() if rec[n].ndim else rec[n]) for n in PIC_REPORT_DTYPE.names if n != "pad"}


class PicHash(C.Structure):
    """fcu_pic_hash: MD5, CRC and checksum per plane, the bytes in HM's digest order."""
    _fields_ = [("md5", (C.c_uint8 * 16) * 3), ("crc", (C.c_uint8 * 2) * 3), ("checksum", (C.c_uint8 * 4) * 3), ("pad", C.c_uint8 * 2)]


PIC_HASH_DTYPE = np.dtype([("md5", np.uint8, (3, 16)), ("crc", np.uint8, (3, 2)), ("checksum", np.uint8, (3, 4)), ("pad", np.uint8, (2,))])   # fcu_pic_hash
HASH_KINDS = {"md5": 1, "crc": 2, "checksum": 4}             # FCU_HASH_*: HM's SEIDecodedPictureHash 1 / 2 / 3
HASH_LABELS = {"md5": "MD5", "crc": "CRC", "checksum": "Checksum"}      # as TEncGOP.cpp:1746-1754 prints them


def hash_string(rec, kind):
    """fcu_hash_string: HM's digestToString of one kind ("md5", "crc" or "checksum") of one element of a PIC_HASH_DTYPE array"""
    buf = C.create_string_buffer(128)
    a = np.ascontiguousarray(rec).view(np.uint8).reshape(-1)
    n = load_lib().fcu_hash_string(a.ctypes.data, HASH_KINDS[kind], buf, 128)
    if n < 0:
        raise FcuError("fcu_hash_string: %d" % n)
    return buf.value.decode()


def hash_line(kind, string):
    """what the encoder appends to the picture line (TEncGOP.cpp:1742-1756)"""
    return " [%s:%s]" % (HASH_LABELS[kind], string)


class CtuMatch(C.Structure):
    """fcu_ctu_match: the split match of one CTU."""
    _fields_ = [("part_total", C.c_uint16), ("part_equal", C.c_uint16), ("node", ((C.c_uint16 * 2) * 2) * 4), ("only_a", C.c_uint16 * 4),
                ("only_b", C.c_uint16 * 4), ("pad", C.c_uint16 * 6)]


class PicMatch(C.Structure):
    """fcu_pic_match: the sums over a picture's CTUs."""
    _fields_ = [("part_total", C.c_uint64), ("part_equal", C.c_uint64), ("node", ((C.c_uint64 * 2) * 2) * 4), ("only_a", C.c_uint64 * 4),
                ("only_b", C.c_uint64 * 4)]


CTU_MATCH_DTYPE = np.dtype([("part_total", np.uint16), ("part_equal", np.uint16), ("node", np.uint16, (4, 2, 2)), ("only_a", np.uint16, (4,)),
                            ("only_b", np.uint16, (4,)), ("pad", np.uint16, (6,))])                                                # fcu_ctu_match
PIC_MATCH_DTYPE = np.dtype([("part_total", np.uint64), ("part_equal", np.uint64), ("node", np.uint64, (4, 2, 2)), ("only_a", np.uint64, (4,)),
                            ("only_b", np.uint64, (4,))])                                                                          # fcu_pic_match
# FCU_MAP_*: the byte-per-partition arrays of fcu_ctu_out a byte map can be taken from
MAP_FIELDS = {n: i for i, n in enumerate(("depth", "part_size", "pred_mode", "skip", "merge_flag", "merge_idx", "tr_idx", "cbf_y", "cbf_cb", "cbf_cr",
                                          "tskip_y", "tskip_cb", "tskip_cr", "intra_dir_luma", "intra_dir_chroma", "qp", "inter_dir", "mvp_idx", "ref_idx"))}
MAP_SIGNED = ("part_size", "pred_mode", "qp", "mvp_idx", "ref_idx")      # int8 in the record: their maps come back as int8 views
LABEL_ABSENT, LABEL_NOT_SPLIT, LABEL_SPLIT, LABEL_FORCED = -1, 0, 1, 2    # FCU_LABEL_*


def pic_match_to_dict(rec):
    """one element of a PIC_MATCH_DTYPE array -> dict: part_total, part_equal (int), node [4, 2, 2], only_a [4], only_b [4] (int64) and
    split_match = part_equal / part_total, the share of the picture's 4x4 partitions decided to the same CU depth (bench.py's
    figure of that name is stricter: it also asks for equal part_size and pred_mode, and walks all 256 entries of a cut CTU)"""
    d = {n: (rec[n].astype(np.int64) if rec[n].ndim else int(rec[n])) for n in PIC_MATCH_DTYPE.names}
    d["split_match"] = d["part_equal"] / d["part_total"] if d["part_total"] else 1.0
    return d


def map_level_shapes(width, height):
    """[(BH(d), BW(d))] of the label / N_OBF maps of level d = 0..3 (blocks of 64 >> d samples)"""
    return [((height + (64 >> d) - 1) // (64 >> d), (width + (64 >> d) - 1) // (64 >> d)) for d in range(4)]


class VerifyCounts(C.Structure):
    """fcu_verify_counts: g_iVerResult[depth][TP, FP, TN, FN, FPLoss, FNLoss]."""
    _fields_ = [("n", (C.c_double * 6) * 4)]

EXPORTS = ["fcu_default_frame_params", "fcu_create", "fcu_destroy", "fcu_num_ctus", "fcu_chain_begin",
           "fcu_compress_chains", "fcu_compress_ctu", "fcu_get_ctx_state", "fcu_chain_position", "fcu_sync",
           "fcu_kernel_ms", "fcu_last_error", "fcu_debug_counters", "fcu_chain_set_range", "fcu_obf_prepass", "fcu_chains_per_cu",
           "fcu_chain_set_decision", "fcu_get_verify_counts", "fcu_decision_switch", "fcu_frame_state", "fcu_deblock",
           "fcu_build_info", "fcu_abi_sizeof", "fcu_tcm_threshold", "fcu_chain_set_reference", "fcu_pad_reference", "fcu_pad_sizes", "fcu_ldp_slice", "fcu_get_ctx_state_full",
           "fcu_sao", "fcu_sao_enabled", "fcu_sao_update_rate", "fcu_ldp_layer", "fcu_chain_set_pu_trace", "fcu_pu_index", "fcu_chain_set_collocated",
           "fcu_chain_set_references", "fcu_chain_set_collocated_pocs", "fcu_chain_get_search_state", "fcu_chain_set_search_state",
           "fcu_wpp_begin", "fcu_wpp_rows", "fcu_compress_wpp", "fcu_wpp_begin_p", "fcu_wpp_begin_slices",
           "fcu_tile_grid", "fcu_tile_chains", "fcu_tiles_begin", "fcu_wpp_begin_tiles", "fcu_deblock_tiles", "fcu_sao_tiles", "fcu_picture_report",
           "fcu_picture_hash", "fcu_hash_string", "fcu_decision_maps", "fcu_split_match", "fcu_deblock_slices", "fcu_sao_slices",
           "fcu_chain_set_labels", "fcu_label_count", "fcu_labels_from_rasters",
           "fcu_cu_index", "fcu_chain_set_cu_trace", "fcu_label_score", "fcu_trace_maps", "fcu_feature_count", "fcu_feature_maps",
           "fcu_risk_train", "fcu_risk_predict", "fcu_nobf_maps", "fcu_risk_table",
           "fcu_feature_edges_check", "fcu_feature_bins", "fcu_tree_keys", "fcu_tree_hist", "fcu_tree_split", "fcu_tree_train"]
MAX_REF = 4                                                # FCU_MAX_REF: reference pictures in list 0

SLICE_I, SLICE_P = 0, 1
PUS_PER_CTU = 341
PU_TRACE_DTYPE = np.dtype([("valid", np.uint8), ("best_mode", np.uint8), ("n_rmd", np.uint8), ("n_rd", np.uint8), ("rd_mode", np.uint8, (12,)),
                           ("best_dist", np.uint32), ("pad", np.uint32), ("best_cost", np.float64), ("rmd_cost", np.float64, (8,))])   # fcu_pu_trace


CUS_PER_CTU = 85                                           # FCU_CUS_PER_CTU: 1 + 4 + 16 + 64 CUs of depth 0..3
MAX_DOUBLE = 1.7e+308                                      # FCU_MAX_DOUBLE: j0 of a CU whose whole-CU check was pruned
CU_TRACE_DTYPE = np.dtype([("j0", np.float64), ("j1", np.float64), ("valid", np.uint8), ("split_won", np.uint8), ("whole_tried", np.uint8),
                           ("split_tried", np.uint8), ("pad", np.uint8, (4,))])                                                    # fcu_cu_trace
CTU_SCORE_DTYPE = np.dtype([("n", np.uint16, (4, 4)), ("open", np.uint16, (4,)), ("pad", np.uint16, (12,)), ("loss", np.float64, (4, 2))])   # fcu_ctu_score
PIC_SCORE_DTYPE = np.dtype([("v", np.float64, (4, 6)), ("open", np.uint32, (4,)), ("scored", np.uint32, (4,))])                    # fcu_pic_score

RISK_BINS = 257                                            # FCU_RISK_BINS: N_OBF of a 64x64 CU is 0..256
RISK_MODEL_DTYPE = np.dtype([("risk", np.int64, (4, RISK_BINS, 2)), ("count", np.uint32, (4, RISK_BINS, 2))])                      # fcu_risk_model


def risk_table(model, min_count=1):
    """fcu_risk_table: the rule of the risk-table model on a host copy of one (a RISK_MODEL_DTYPE array, or the uint8 bytes of one)
    -> int8 [4, 257]: LABEL_NOT_SPLIT where risk[d][x][1] < risk[d][x][0], else LABEL_SPLIT; LABEL_ABSENT for a bin with fewer than
    min_count samples.  Host arithmetic of libfcu.so; needs no GPU."""
    m = np.ascontiguousarray(model).view(np.uint8).reshape(-1)
    assert m.size == RISK_MODEL_DTYPE.itemsize and min_count >= 0, "risk_table: one fcu_risk_model and a non-negative min_count"
    out = np.zeros((4, RISK_BINS), np.int8)
    load_lib().fcu_risk_table(m.ctypes.data, int(min_count), out.ctypes.data)
    return out


TREE_BINS, TREE_MAX_LEVELS, TREE_NODES = 32, 5, 31           # FCU_TREE_BINS, FCU_TREE_MAX_LEVELS, FCU_TREE_NODES


class KeyTree(C.Structure):
    """fcu_key_tree: per depth a complete binary tree in heap order over the binned feature columns (include/fcu.h)"""
    _fields_ = [("levels", C.c_int32), ("feature", (C.c_int16 * TREE_NODES) * 4), ("thr", (C.c_uint8 * TREE_NODES) * 4)]

    def __init__(self, levels=0):
        super().__init__()
        self.levels = levels
        for d in range(4):
            for i in range(TREE_NODES):
                self.feature[d][i] = -1

    def arrays(self):
        """(levels, feature int16 [4, 31], thr uint8 [4, 31]) as numpy copies"""
        return int(self.levels), np.array([list(r) for r in self.feature], np.int16), np.array([list(r) for r in self.thr], np.uint8)


def tree_hist_shape(n_features, level):
    """the shape of both histograms of fcu_tree_hist: [depth, node, column, bin, split_won]"""
    return (4, 1 << level, n_features, TREE_BINS, 2)


def tree_split(risk, count, level, tree, min_count=1):
    """fcu_tree_split: fills the nodes of `level` of `tree` (a KeyTree, changed in place) from host copies of that level's
    histograms, int64 / uint32 [4, 2^level, F, 32, 2].  Host integer arithmetic of libfcu.so; needs no GPU.  The caller sets
    tree.levels."""
    risk, count = np.ascontiguousarray(risk, np.int64), np.ascontiguousarray(count, np.uint32)
    if risk.ndim != 5 or risk.shape != count.shape or risk.shape != tree_hist_shape(risk.shape[2], level):
        raise ValueError("tree_split: histograms are [4, 2^level, F, 32, 2]")
    lib = load_lib()
    if lib.fcu_tree_split(risk.ctypes.data, count.ctypes.data, risk.shape[2], int(level), int(min_count), C.byref(tree)) != 0:
        raise FcuError("fcu_tree_split: " + lib.fcu_last_error().decode())
    return tree


def feature_edges(X, width, height):
    """The driver's default edges for feature_bins: X = the float32 tensor [n, NL, F] of feature_maps for pictures of
    width x height.  Per (level, column) the rows of that level -- of all n pictures -- are sorted with torch on X's device and
    the values at ranks round(k * rows / 32), k = 1..31, are taken: float32 [4, F, 31] on that device.  A constant column gives
    equal edges.  Not part of the ABI: any finite, non-decreasing edges do."""
    import torch
    shapes = map_level_shapes(width, height)
    assert X.dim() == 3 and X.shape[1] == sum(a * b for a, b in shapes), "feature_edges: [n, NL, F] of feature_maps"
    out, o = [], 0
    for bh, bw in shapes:
        rows = X[:, o:o + bh * bw, :].reshape(-1, X.shape[2])
        o += bh * bw
        s = torch.sort(rows, dim=0).values
        n = s.shape[0]
        rank = torch.tensor([min(n - 1, int(round(k * n / TREE_BINS))) for k in range(1, TREE_BINS)], device=X.device)
        out.append(s.index_select(0, rank).t())
    return torch.stack(out).contiguous().to(torch.float32)


# FCU_FEATSET_*: the feature sets of fcu_feature_maps, in column order, and the names of their columns (include/fcu.h):
# tmv_<filter>_<mean | var>_<region>, column f * 26 + k, and soc_<k>, k = y * 4 + x of the 4x4 DCT
FEATURE_SETS = {"tmv": 1, "soc": 2}
FEATURE_COUNTS = {"tmv": 130, "soc": 16}                  # FCU_FEAT_TMV, FCU_FEAT_SOC
TMV_FILTERS = ("org", "hor", "ver", "diag", "antd")
# k = 20 / 24 ("q_bottom") are the fork's third "quadrant": all columns of the bottom rows, equal to k = 3 / 5
TMV_STATS = ("mean_all", "var_all", "mean_top", "mean_bottom", "var_top", "var_bottom", "mean_left", "mean_right", "var_left", "var_right",
             "mean_tri_tl", "mean_tri_br", "var_tri_tl", "var_tri_br", "mean_tri_tr", "mean_tri_bl", "var_tri_tr", "var_tri_bl",
             "mean_q_tl", "mean_q_tr", "mean_q_bottom", "mean_q_br", "var_q_tl", "var_q_tr", "var_q_bottom", "var_q_br")
FEATURE_NAMES = tuple("tmv_%s_%s" % (f, k) for f in TMV_FILTERS for k in TMV_STATS) + tuple("soc_%d" % k for k in range(16))


def feature_sets(sets):
    """the names of `sets` (one name or several, any order) as (mask, names in column order)"""
    sets = (sets,) if isinstance(sets, str) else tuple(sets)
    for n in sets:
        if n not in FEATURE_SETS:
            raise ValueError("feature sets are among %s, not %r" % (sorted(FEATURE_SETS), n))
    names = tuple(n for n in FEATURE_SETS if n in sets)
    return sum(FEATURE_SETS[n] for n in names), names


def feature_columns(sets):
    """the column names of feature_maps(..., sets=sets), in column order"""
    _, names = feature_sets(sets)
    return tuple(c for c in FEATURE_NAMES if c.split("_")[0] in names)


def cu_index(depth, zidx):
    """fcu_cu_index: position of a CU inside its CTU's 85 records (zidx = z-order index of its first 4x4 partition)"""
    return load_lib().fcu_cu_index(depth, zidx)


def pu_index(depth, nxn, zidx):
    """fcu_pu_index: position of a PU inside its CTU's 341 records"""
    return load_lib().fcu_pu_index(depth, nxn, zidx)

REF_MARGIN = 80


def lib_path():
    # FCU_LIB: another build of the same library next to it (diagnostic variants: profiling timers, register budgets)
    return os.path.join(_HERE, os.environ.get("FCU_LIB", "libfcu.so"))


_lib = None


def load_lib():
    """Loads libfcu.so (the HIP extension).  Fails loudly if it has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    p = lib_path()
    if not os.path.exists(p):
        raise FcuError(f"{p} not found: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                       "(hipcc --offload-arch=gfx950); there is no CPU fallback")
    lib = C.CDLL(p)
    lib.fcu_create.argtypes = [C.POINTER(SeqParams), C.POINTER(C.c_void_p)]
    lib.fcu_destroy.argtypes = [C.c_void_p]
    lib.fcu_num_ctus.argtypes = [C.c_void_p]
    lib.fcu_default_frame_params.argtypes = [C.POINTER(FrameParams), C.c_int]
    lib.fcu_chain_begin.argtypes = [C.c_void_p, C.c_int, C.POINTER(FrameParams)] + [C.c_void_p] * 7
    lib.fcu_compress_chains.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p]
    lib.fcu_chain_set_range.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int]
    lib.fcu_obf_prepass.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_float), C.c_void_p]
    lib.fcu_compress_ctu.argtypes = [C.c_void_p, C.c_int, C.c_uint32, C.POINTER(CtuOut)]
    lib.fcu_get_ctx_state.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.POINTER(C.c_uint64)]
    lib.fcu_get_ctx_state_full.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.POINTER(C.c_uint64)]
    lib.fcu_chain_position.argtypes = [C.c_void_p, C.c_int]
    lib.fcu_sync.argtypes = [C.c_void_p]
    lib.fcu_kernel_ms.restype = C.c_double
    lib.fcu_kernel_ms.argtypes = [C.c_void_p, C.POINTER(C.c_int)]
    lib.fcu_debug_counters.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_ulonglong)]
    lib.fcu_last_error.restype = C.c_char_p
    lib.fcu_build_info.restype = C.c_char_p
    lib.fcu_tcm_threshold.restype = C.c_double
    lib.fcu_tcm_threshold.argtypes = [C.c_void_p, C.c_int, C.c_int]
    lib.fcu_chain_set_reference.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.fcu_pad_reference.argtypes = [C.c_void_p] * 8
    lib.fcu_pad_sizes.restype = None
    lib.fcu_pad_sizes.argtypes = [C.c_void_p, C.POINTER(C.c_size_t)]
    lib.fcu_ldp_slice.restype = None
    lib.fcu_ldp_slice.argtypes = [C.POINTER(FrameParams), C.c_int, C.c_int]
    lib.fcu_chain_set_decision.argtypes = [C.c_void_p, C.c_int, C.POINTER(DecisionParams)]
    lib.fcu_get_verify_counts.argtypes = [C.c_void_p, C.c_int, C.c_int, C.POINTER(VerifyCounts)]
    lib.fcu_decision_switch.restype = None
    lib.fcu_decision_switch.argtypes = [C.POINTER(VerifyCounts), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.fcu_frame_state.argtypes = [C.c_int] * 4
    lib.fcu_deblock.argtypes = [C.c_void_p] * 5 + [C.c_int, C.c_int, C.POINTER(C.c_float), C.c_void_p]
    lib.fcu_sao.argtypes = [C.c_void_p, C.c_int, C.POINTER(SaoParams), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_float), C.c_void_p]
    lib.fcu_deblock_tiles.argtypes = [C.c_void_p] * 5 + [C.c_int] * 5 + [C.POINTER(C.c_float), C.c_void_p]
    lib.fcu_sao_tiles.argtypes = [C.c_void_p, C.c_int, C.POINTER(SaoParams), C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_float), C.c_void_p]
    lib.fcu_deblock_slices.argtypes = [C.c_void_p] * 5 + [C.c_int] * 4 + [C.POINTER(C.c_float), C.c_void_p]
    lib.fcu_sao_slices.argtypes = [C.c_void_p, C.c_int, C.POINTER(SaoParams), C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_float), C.c_void_p]
    lib.fcu_sao_enabled.restype = None
    lib.fcu_sao_enabled.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
    lib.fcu_sao_update_rate.restype = None
    lib.fcu_sao_update_rate.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int]
    lib.fcu_ldp_layer.argtypes = [C.c_int]
    lib.fcu_chain_set_pu_trace.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
    lib.fcu_chain_set_collocated.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
    lib.fcu_chain_set_references.argtypes = [C.c_void_p, C.c_int, C.c_int, C.POINTER(C.c_void_p), C.POINTER(C.c_int), C.c_int]
    lib.fcu_chain_set_collocated_pocs.argtypes = [C.c_void_p, C.c_int, C.c_int, C.POINTER(C.c_int), C.c_int]
    lib.fcu_chain_get_search_state.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_int32)]
    lib.fcu_chain_set_search_state.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_int32)]
    lib.fcu_wpp_rows.argtypes = [C.c_void_p]
    lib.fcu_wpp_begin.argtypes = [C.c_void_p, C.c_int, C.POINTER(FrameParams)] + [C.c_void_p] * 7
    lib.fcu_wpp_begin_p.argtypes = [C.c_void_p, C.c_int, C.POINTER(FrameParams)] + [C.c_void_p] * 7
    lib.fcu_wpp_begin_slices.argtypes = [C.c_void_p, C.c_int, C.POINTER(FrameParams), C.c_int] + [C.c_void_p] * 7
    lib.fcu_compress_wpp.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p]
    lib.fcu_tile_grid.argtypes = [C.c_int] * 4 + [C.POINTER(C.c_int)] * 2
    lib.fcu_tile_chains.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int]
    lib.fcu_tiles_begin.argtypes = [C.c_void_p, C.c_int, C.POINTER(FrameParams), C.c_int, C.c_int] + [C.c_void_p] * 7
    lib.fcu_wpp_begin_tiles.argtypes = [C.c_void_p, C.c_int, C.POINTER(FrameParams), C.c_int, C.c_int] + [C.c_void_p] * 7
    lib.fcu_picture_report.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_float), C.c_void_p]
    lib.fcu_picture_hash.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.POINTER(C.c_float), C.c_void_p]
    lib.fcu_hash_string.argtypes = [C.c_void_p, C.c_int, C.c_char_p, C.c_int]
    lib.fcu_decision_maps.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int] + [C.c_void_p] * 6 + [C.POINTER(C.c_float), C.c_void_p]
    lib.fcu_split_match.argtypes = [C.c_void_p, C.c_int] + [C.c_void_p] * 4 + [C.POINTER(C.c_float), C.c_void_p]
    lib.fcu_chain_set_labels.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
    lib.fcu_label_count.argtypes = [C.c_void_p]
    lib.fcu_labels_from_rasters.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.fcu_cu_index.argtypes = [C.c_int, C.c_int]
    lib.fcu_chain_set_cu_trace.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
    lib.fcu_label_score.argtypes = [C.c_void_p, C.c_int] + [C.c_void_p] * 4 + [C.POINTER(C.c_float), C.c_void_p]
    lib.fcu_trace_maps.argtypes = [C.c_void_p, C.c_int] + [C.c_void_p] * 4 + [C.POINTER(C.c_float), C.c_void_p]
    lib.fcu_feature_count.argtypes = [C.c_int]
    lib.fcu_feature_maps.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_float), C.c_void_p]
    lib.fcu_risk_train.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.POINTER(C.c_uint32), C.POINTER(C.c_float), C.c_void_p]
    lib.fcu_risk_predict.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.POINTER(C.c_float), C.c_void_p]
    lib.fcu_nobf_maps.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.fcu_feature_edges_check.argtypes = [C.c_void_p, C.c_int]
    lib.fcu_feature_bins.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_float), C.c_void_p]
    lib.fcu_tree_keys.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.POINTER(C.c_float), C.c_void_p]
    lib.fcu_tree_hist.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int] + [C.c_void_p] * 5 + [C.c_int, C.POINTER(C.c_uint32), C.POINTER(C.c_float), C.c_void_p]
    lib.fcu_tree_split.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p]
    lib.fcu_tree_train.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_float), C.c_void_p]
    lib.fcu_risk_table.restype = None
    lib.fcu_risk_table.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
    _lib = lib
    return lib


def decision_switch(ver, th_skip=(0, 0, 0, 0), th_term=(0, 0, 0, 0)):
    """SetDecisionSwitch (tools_YS.cpp:1123-1154) on summed verification counters [4, 6]: (sw_skip[4], sw_term[4]).
    Host arithmetic of libfcu.so; needs no GPU."""
    lib = load_lib()
    v = VerifyCounts()
    a = np.ascontiguousarray(ver, np.float64).reshape(4, 6)
    for d in range(4):
        for k in range(6):
            v.n[d][k] = a[d, k]
    ts, tt = np.ascontiguousarray(th_skip, np.float64), np.ascontiguousarray(th_term, np.float64)
    sk, te = np.zeros(4, np.uint8), np.zeros(4, np.uint8)
    lib.fcu_decision_switch(C.byref(v), ts.ctypes.data, tt.ctypes.data, sk.ctypes.data, te.ctypes.data)
    return sk, te


def sao_coded_to_array(coded):
    """uint8 [.., n_ctu, SAO_CTU_BYTES] (device tensor or array) -> int32 [.., n_ctu, 3, 35]: mode, type, band, offset[32]"""
    a = coded.cpu().numpy() if hasattr(coded, "cpu") else np.asarray(coded)
    a = a.view(np.int8).reshape(a.shape[:-1] + (3, 36)).astype(np.int32)
    return np.concatenate([a[..., :3], a[..., 4:]], axis=-1)


class SaoRate:
    """m_saoDisabledRate across the pictures of one sequence (fcu_sao_enabled / fcu_sao_update_rate)"""

    def __init__(self):
        self.rate = np.zeros((3, 8), np.float64)

    def enabled(self, layer):
        e = np.zeros(3, np.int32)
        load_lib().fcu_sao_enabled(self.rate.ctypes.data, layer, e.ctypes.data)
        return [int(v) for v in e]

    def update(self, layer, off_count, n_ctu):
        oc = np.ascontiguousarray(off_count, np.int32)
        load_lib().fcu_sao_update_rate(self.rate.ctypes.data, layer, oc.ctypes.data, n_ctu)


def ldp_layer(poc):
    return load_lib().fcu_ldp_layer(poc)


def ldp_slice(base_qp, poc):
    """FrameParams of picture `poc` under HM's lowdelay_P GOP table (fcu_ldp_slice): slice type, QP, lambda, inter defaults."""
    fp = FrameParams()
    load_lib().fcu_ldp_slice(C.byref(fp), base_qp, poc)
    return fp


def tile_grid(width_in_ctus, height_in_ctus, n_cols, n_rows):
    """fcu_tile_grid: HM's uniform tile spacing -> (column boundaries [n_cols + 1], row boundaries [n_rows + 1]) in CTUs.
    Raises ValueError for a grid with an empty tile.  Host arithmetic of libfcu.so; needs no GPU."""
    cb, rb = (C.c_int * (max(n_cols, 0) + 1))(), (C.c_int * (max(n_rows, 0) + 1))()
    if load_lib().fcu_tile_grid(width_in_ctus, height_in_ctus, n_cols, n_rows, cb, rb) != 0:
        raise ValueError(f"no {n_cols} x {n_rows} tile grid on a picture of {width_in_ctus} x {height_in_ctus} CTUs (a tile would be empty)")
    return list(cb), list(rb)


def frame_state(poc, period=60, n_training=2, n_verifying=1):
    """getCurrentState (tools_YS.cpp:1237-1242) with the reference's defaults g_iP / g_iT / g_iV (tools_YS.cpp:41-43)."""
    return load_lib().fcu_frame_state(poc, period, n_training, n_verifying)


def ctu_to_dict(c):
    out = {}
    for name, _ in CtuOut._fields_:
        v = getattr(c, name)
        out[name] = np.ctypeslib.as_array(v).copy() if hasattr(v, "_length_") else v
    return out


class CuEngine:
    """`TEncCu` stand-in for a set of independent chains (frames / slices) on one GPU.

    create()        <- TEncCu::create  : allocates the per-chain device scratch
    init_chain()    <- TEncCu::init + TEncSlice::setUpLambda : binds planes, QP, lambda
    compress_ctu()  <- TEncCu::compressCtu + encodeCtu : one CTU of one chain, result to host
    compress_chains(): the batched form, many chains x k CTUs per launch
    init_picture() / compress_pictures(): one picture as the chains of a PictureLayout (slices, WPP rows, tiles)
    destroy()       <- TEncCu::destroy
    """

    def __init__(self, width, height, max_chains=1, device=0):
        import torch
        if not torch.cuda.is_available():
            raise FcuError("no GPU visible: the CU engine has no CPU fallback")
        self.torch = torch
        self.lib = load_lib()
        self.width, self.height, self.max_chains, self.device = width, height, max_chains, device
        self.h = C.c_void_p()
        self._keep = {}
        self._keep_obf = {}
        self._keep_ref = {}
        self.create()

    # -- TEncCu::create
    def create(self):
        sp = SeqParams(self.width, self.height, self.max_chains, self.device)
        r = self.lib.fcu_create(C.byref(sp), C.byref(self.h))
        if r != 0:
            raise FcuError(f"fcu_create failed ({r}): {self.lib.fcu_last_error().decode()}")
        self.n_ctu = self.lib.fcu_num_ctus(self.h)

    def _chk(self, r, what):
        if r != 0:
            raise FcuError(f"{what} failed ({r}): {self.lib.fcu_last_error().decode()}")

    # -- TEncCu::init + slice parameters
    def _open(self, org, qp, rec, out, params, flags, who):
        """what every binder starts with: the planes on the device, rec / out allocated when None, the frame parameters from
        `params` or the I-slice defaults for `qp`, with `flags` applied.  Returns planes, rec, out, fp."""
        torch = self.torch
        dev = torch.device("cuda", self.device)
        planes = [(torch.as_tensor(a) if not torch.is_tensor(a) else a).to(device=dev, dtype=torch.uint8).contiguous() for a in org]
        if rec is None:
            rec = [torch.zeros_like(p) for p in planes]
        if out is None:
            out = torch.zeros(self.n_ctu * CTU_OUT_BYTES, dtype=torch.uint8, device=dev)
        fp = FrameParams()
        if params is not None:
            C.memmove(C.byref(fp), C.byref(params), C.sizeof(FrameParams))
        else:
            self.lib.fcu_default_frame_params(C.byref(fp), qp)
        known = {n for n, _ in FrameParams._fields_}
        for k, v in flags.items():
            if k not in known:                                  # a misspelt tool flag must not be dropped silently
                raise TypeError(f"{who}: unknown frame parameter {k!r} (fcu_frame_params has {sorted(known)})")
            setattr(fp, k, v)
        return planes, rec, out, fp

    def init_chain(self, chain, org, qp, slice_ctus=0, rec=None, out=None, ref=None, params=None, col=None,
                   refs=None, ref_pocs=None, poc=None, col_ref_pocs=None, **flags):
        """org: (Y,U,V) uint8 torch tensors on this device (or numpy arrays, uploaded once).
        params: a FrameParams to start from (e.g. ldp_slice(base_qp, poc)) instead of the I-slice defaults for `qp`;
        ref: padded reference planes from pad_reference() -- required for a P slice;
        col: the reference picture's fcu_ctu_out array (TMVP, with params.tmvp = 1);
        refs / ref_pocs / poc: several reference pictures instead of `ref` -- RefPicList0 as a list of pad_reference() triplets
        with their POCs and this picture's POC; col_ref_pocs: the POCs the list 0 of refs[0] (the collocated picture) named."""
        if refs is not None:
            assert ref is None and 1 <= len(refs) <= MAX_REF and len(ref_pocs) == len(refs) and poc is not None
        planes, rec, out, fp = self._open(org, qp, rec, out, params, flags, "init_chain")
        fp.slice_ctus = slice_ctus
        self._chk(self.lib.fcu_chain_begin(self.h, chain, C.byref(fp), *[p.data_ptr() for p in planes],
                                           *[p.data_ptr() for p in rec], out.data_ptr()), "fcu_chain_begin")
        self._keep[chain] = (planes, rec, out)
        self._bind_refs(chain, ref, refs, ref_pocs, poc, col_ref_pocs, col)
        return rec, out

    def init_picture(self, first_chain, org, qp, layout, rec=None, out=None, params=None, ref=None, refs=None, ref_pocs=None, poc=None,
                     col_ref_pocs=None, col=None, search_state=None, **flags):
        """One picture as the chains [first_chain, first_chain + layout.chains) of a PictureLayout; they share the picture's
        planes and fcu_ctu_out array.  org / rec / out / params / flags as init_chain takes them (I or P by params.slice_type).
          slices         one chain per slice, in order (fcu_chain_begin + fcu_chain_set_range; one slice: a single chain bound
                         with slice_ctus 0); compress_chains advances them;
          wpp            one chain per CTU row, top to bottom (fcu_wpp_begin, fcu_wpp_begin_p for a P slice; with slice_rows
                         fcu_wpp_begin_slices: the first row of every slice waits for nothing and starts from a zero search
                         state); decided by compress_wpp;
          tiles          one chain per tile in tile-scan order, each raster-in-tile (fcu_tiles_begin); with wpp one chain per CTU
                         row of every tile, rows top to bottom (fcu_wpp_begin_tiles).  Every tile starts from a zero search state.
        A P picture takes ref or refs / ref_pocs / poc / col_ref_pocs and col (init_chain) on every chain, and search_state
        (set_search_state: what the previous picture left; zero when None) on the first chain.  set_decision rewrites the search
        state: a caller that sets decision states passes search_state=None and calls set_search_state(first_chain, ...) after its
        set_decision calls.  compress_pictures launches what was bound.  Returns (n_chains, rec, out)."""
        if refs is not None:
            assert ref is None and 1 <= len(refs) <= MAX_REF and len(ref_pocs) == len(refs) and poc is not None
        assert layout.n_ctu == self.n_ctu
        planes, rec, out, fp = self._open(org, qp, rec, out, params, flags, "init_picture")
        p_slice = fp.slice_type == SLICE_P
        ptrs = [p.data_ptr() for p in planes] + [p.data_ptr() for p in rec] + [out.data_ptr()]
        if layout.tiles is not None:
            name, args = "fcu_wpp_begin_tiles" if layout.wpp else "fcu_tiles_begin", [int(v) for v in layout.tiles]
        elif layout.slice_rows is not None:
            name, args = "fcu_wpp_begin_slices", [int(layout.slice_rows)]
        elif layout.wpp:
            name, args = "fcu_wpp_begin_p" if p_slice else "fcu_wpp_begin", []
        else:
            name, sl = None, layout.bind_slice_ctus
            fp.slice_ctus = sl
            for k in range(layout.chains):
                self._chk(self.lib.fcu_chain_begin(self.h, first_chain + k, C.byref(fp), *ptrs), "fcu_chain_begin")
                if sl:
                    self.set_range(first_chain + k, k * sl, min(sl, self.n_ctu - k * sl))
        if name:
            self._chk(getattr(self.lib, name)(self.h, first_chain, C.byref(fp), *args, *ptrs), name)
        for k in range(layout.chains):
            self._keep[first_chain + k] = (planes, rec, out)
            if p_slice:
                self._bind_refs(first_chain + k, ref, refs, ref_pocs, poc, col_ref_pocs, col)
        if p_slice and search_state is not None:
            self.set_search_state(first_chain, search_state)
        return layout.chains, rec, out

    def compress_pictures(self, first, n_pictures, layout, stream=None):
        """decides n_pictures pictures bound by init_picture with this layout at consecutive chains from `first`, to their end"""
        if layout.uses_wpp_launch:
            self.compress_wpp(first, n_pictures * layout.chains, stream)
        else:
            self.compress_chains(first, n_pictures * layout.chains, layout.launch_ctus, stream)

    def _bind_refs(self, chain, ref=None, refs=None, ref_pocs=None, poc=None, col_ref_pocs=None, col=None):
        """reference pictures and collocated field of a bound chain (init_chain's arguments of the same names)"""
        if ref is not None:
            self._chk(self.lib.fcu_chain_set_reference(self.h, chain, *[p.data_ptr() for p in ref]), "fcu_chain_set_reference")
            self._keep_ref[chain] = ref
        if refs is not None:
            ptrs = (C.c_void_p * (3 * len(refs)))(*[p.data_ptr() for r in refs for p in r])
            pocs = (C.c_int * len(refs))(*[int(v) for v in ref_pocs])
            self._chk(self.lib.fcu_chain_set_references(self.h, chain, len(refs), ptrs, pocs, int(poc)), "fcu_chain_set_references")
            self._keep_ref[chain] = refs
            if col_ref_pocs:
                crp = (C.c_int * len(col_ref_pocs))(*[int(v) for v in col_ref_pocs])
                self._chk(self.lib.fcu_chain_set_collocated_pocs(self.h, chain, int(ref_pocs[0]), crp, len(col_ref_pocs)), "fcu_chain_set_collocated_pocs")
        if col is not None:                                   # TMVP: the reference picture's fcu_ctu_out array (uint8 device tensor)
            assert col.is_cuda and col.numel() >= self.n_ctu * CTU_OUT_BYTES
            self._chk(self.lib.fcu_chain_set_collocated(self.h, chain, col.data_ptr()), "fcu_chain_set_collocated")
            self._keep_ref[("col", chain)] = col

    def search_state(self, chain):
        """m_integerMv2Nx2N of the chain: [(x, y)] per reference index (fcu_chain_get_search_state)"""
        xy = (C.c_int32 * (2 * MAX_REF))()
        self._chk(self.lib.fcu_chain_get_search_state(self.h, chain, xy), "fcu_chain_get_search_state")
        return [(int(xy[2 * r]), int(xy[2 * r + 1])) for r in range(MAX_REF)]

    def set_search_state(self, chain, state):
        """after init_chain: the state the encoder's previous searches left (fcu_chain_set_search_state)"""
        xy = (C.c_int32 * (2 * MAX_REF))(*[int(v) for p in (list(state) + [(0, 0)] * MAX_REF)[:MAX_REF] for v in p])
        self._chk(self.lib.fcu_chain_set_search_state(self.h, chain, xy), "fcu_chain_set_search_state")

    def pad_reference(self, planes, stream=None):
        """(Y, U, V) device planes of a reconstructed (loop-filtered) picture -> padded planes for P chains
        (TComPicYuv::extendPicBorder).  Returns three uint8 tensors."""
        torch = self.torch
        sz = (C.c_size_t * 3)()
        self.lib.fcu_pad_sizes(self.h, sz)
        dev = torch.device("cuda", self.device)
        src = [torch.as_tensor(p).to(device=dev, dtype=torch.uint8).contiguous() for p in planes]
        out = [torch.empty(int(sz[k]), dtype=torch.uint8, device=dev) for k in range(3)]
        s = C.c_void_p(stream.cuda_stream) if stream is not None else None
        self._chk(self.lib.fcu_pad_reference(self.h, *[p.data_ptr() for p in src], *[p.data_ptr() for p in out], s), "fcu_pad_reference")
        return out

    def init_slice_chains(self, first_chain, org, qp, slice_ctus, **flags):
        """One frame as ceil(n_ctu / slice_ctus) chains, one per slice (SliceMode 1): init_picture with that layout;
        flags may name its other arguments.  Returns (n_slices, rec, out)."""
        return self.init_picture(first_chain, org, qp, PictureLayout(self.width, self.height, slice_ctus=slice_ctus, who="init_slice_chains"), **flags)

    def init_wpp_picture(self, first_chain, org, qp, rec=None, out=None, params=None, ref=None, refs=None, ref_pocs=None, poc=None,
                         col_ref_pocs=None, col=None, search_state=None, slice_rows=None, **flags):
        """One picture with WaveFrontSynchro on, its CTU rows as chains: init_picture with the layout wpp=True, slice_rows
        (None: one slice; N: independent slices of N whole CTU rows).  Returns (n_rows, rec, out)."""
        lo = PictureLayout(self.width, self.height, wpp=True, slice_rows=slice_rows, who="init_wpp_picture")
        return self.init_picture(first_chain, org, qp, lo, rec=rec, out=out, params=params, ref=ref, refs=refs, ref_pocs=ref_pocs, poc=poc,
                                 col_ref_pocs=col_ref_pocs, col=col, search_state=search_state, **flags)

    def tile_chains(self, n_cols, n_rows, wpp=False):
        """chains init_tile_picture binds for this grid (fcu_tile_chains); -1: no such grid"""
        return self.lib.fcu_tile_chains(self.h, n_cols, n_rows, int(bool(wpp)))

    def init_tile_picture(self, first_chain, org, qp, n_cols, n_rows, wpp=False, rec=None, out=None, params=None, ref=None, refs=None,
                          ref_pocs=None, poc=None, col_ref_pocs=None, col=None, **flags):
        """One picture, one slice, cut into n_cols x n_rows uniform tiles (HM's TileUniformSpacing), with wpp WaveFrontSynchro
        inside every tile: init_picture with the layout tiles=(n_cols, n_rows), wpp.  Returns (n_chains, rec, out)."""
        lo = PictureLayout(self.width, self.height, wpp=wpp, tiles=(n_cols, n_rows), who="init_tile_picture")
        return self.init_picture(first_chain, org, qp, lo, rec=rec, out=out, params=params, ref=ref, refs=refs, ref_pocs=ref_pocs, poc=poc,
                                 col_ref_pocs=col_ref_pocs, col=col, **flags)

    def compress_wpp(self, first, n, stream=None):
        """decides the WPP row chains [first, first + n) (whole pictures) to the end in one launch; returns once it has finished"""
        s = C.c_void_p(stream.cuda_stream) if stream is not None else None
        self._chk(self.lib.fcu_compress_wpp(self.h, first, n, s), "fcu_compress_wpp")

    def set_range(self, chain, first_ctu, n_ctus):
        self._chk(self.lib.fcu_chain_set_range(self.h, chain, first_ctu, n_ctus), "fcu_chain_set_range")

    # -- TEncCu::compressCtu (+ encodeCtu replay)
    def compress_ctu(self, chain, ctu_rs_addr):
        c = CtuOut()
        self._chk(self.lib.fcu_compress_ctu(self.h, chain, ctu_rs_addr, C.byref(c)), "fcu_compress_ctu")
        return ctu_to_dict(c)

    def compress_chains(self, first, n, ctus, stream=None):
        s = C.c_void_p(stream.cuda_stream) if stream is not None else None
        self._chk(self.lib.fcu_compress_chains(self.h, first, n, ctus, s), "fcu_compress_chains")

    def sync(self):
        self._chk(self.lib.fcu_sync(self.h), "fcu_sync")

    def kernel_ms(self):
        n = C.c_int(0)
        ms = self.lib.fcu_kernel_ms(self.h, C.byref(n))
        return ms, n.value

    def debug_counters(self, chain):
        buf = (C.c_ulonglong * 17)()
        self._chk(self.lib.fcu_debug_counters(self.h, chain, buf), "fcu_debug_counters")
        return list(buf)

    def position(self, chain):
        return self.lib.fcu_chain_position(self.h, chain)

    def ctx_state(self, chain, full=False):
        """context states after the chain's last CTU: the 160 of an I slice, or all 176 (full=True), + the Q15 counter"""
        ctx = np.zeros(176 if full else 160, np.uint8)
        frac = C.c_uint64(0)
        if full:
            self._chk(self.lib.fcu_get_ctx_state_full(self.h, chain, ctx.ctypes.data, C.byref(frac)), "fcu_get_ctx_state_full")
        else:
            self._chk(self.lib.fcu_get_ctx_state(self.h, chain, ctx.ctypes.data, C.byref(frac)), "fcu_get_ctx_state")
        return ctx, int(frac.value)

    def rec_planes(self, chain):
        return [p.cpu().numpy() for p in self._keep[chain][1]]

    def org_planes(self, chain):
        """the source planes the chain was bound with, as uploaded: (Y, U, V) uint8 device tensors"""
        return self._keep[chain][0]

    def ctu_out(self, chain, ctu_rs_addr):
        buf = self._keep[chain][2][ctu_rs_addr * CTU_OUT_BYTES:(ctu_rs_addr + 1) * CTU_OUT_BYTES].cpu().numpy()
        return ctu_to_dict(CtuOut.from_buffer_copy(buf.tobytes()))

    # -- fork pre-pass (TEncSlice::getOutlierWithDCT)
    def obf_prepass(self, luma):
        """luma: uint8 tensor [n, height, width] on this device (or a numpy array).  Returns (obf int16 tensor
        [n, height/4, width/4], yc float64 array [n, 16], (hist_ms, count_ms))."""
        torch = self.torch
        dev = torch.device("cuda", self.device)
        t = torch.as_tensor(luma) if not torch.is_tensor(luma) else luma
        t = t.to(device=dev, dtype=torch.uint8).contiguous()
        if t.dim() == 2:
            t = t[None]
        n = t.shape[0]
        assert tuple(t.shape[1:]) == (self.height, self.width)
        obf = torch.zeros((n, self.height // 4, self.width // 4), dtype=torch.int16, device=dev)
        yc = np.zeros((n, 16), np.float64)
        ms = (C.c_float * 2)()
        self._chk(self.lib.fcu_obf_prepass(self.h, n, t.data_ptr(), obf.data_ptr(), yc.ctypes.data, ms, None), "fcu_obf_prepass")
        return obf, yc, (ms[0], ms[1])

    # -- fork decision hooks of xCompressCU
    def set_decision(self, chain, state, obf=None, sw_skip=(0, 0, 0, 0), sw_term=(0, 0, 0, 0), depth_exception=0):
        """obf: this frame's map from obf_prepass (int16 tensor [height/4, width/4] on this device); None in the Verifying /
        Testing state: the chain predicts from the labels set_labels bound before."""
        dp = DecisionParams()
        dp.state, dp.depth_exception = state, depth_exception
        for d in range(4):
            dp.sw_skip2nx2n[d], dp.sw_terminate[d] = int(sw_skip[d]), int(sw_term[d])
        if obf is not None:
            assert obf.is_contiguous() and obf.dtype == self.torch.int16 and tuple(obf.shape) == (self.height // 4, self.width // 4)
            dp.dev_obf = obf.data_ptr()
            self._keep_obf[chain] = obf
        self._chk(self.lib.fcu_chain_set_decision(self.h, chain, C.byref(dp)), "fcu_chain_set_decision")

    # -- split labels of a model of the caller's in the place of the Naive label
    def label_count(self):
        """NL: elements of one picture's label array (fcu_label_count)"""
        return self.lib.fcu_label_count(self.h)

    def set_labels(self, chains, labels):
        """Binds one picture's label array -- an int8 device tensor of label_count() elements in the layout decision_maps writes
        (the four levels one after the other; LABEL_SPLIT = Skip2Nx2N, LABEL_NOT_SPLIT = TerminateCU, anything else = no
        prediction) -- to a chain or to every chain of `chains` (the slice, row or tile chains of the picture share the array),
        in the place of the Naive label on the OBF map; None unbinds (fcu_chain_set_labels).  After set_decision when that
        names an OBF map; a chain without one takes its labels first and its Verifying / Testing state after."""
        chains = [chains] if isinstance(chains, int) else list(chains)
        if labels is not None:
            assert labels.is_cuda and labels.dtype == self.torch.int8 and labels.is_contiguous() and labels.numel() == self.label_count(), "set_labels: int8 [NL] on the device"
        for k in chains:
            self._chk(self.lib.fcu_chain_set_labels(self.h, k, labels.data_ptr() if labels is not None else None), "fcu_chain_set_labels")
            self._keep_obf[("labels", k)] = labels

    def labels_from_rasters(self, depth, part_size=None, out=None, stream=None):
        """Label arrays from depth (uint8) and part_size (int8, or None: no NxN) rasters [n, height / 4, width / 4] on the device --
        the form partition models predict and decision_maps(fields=("depth", "part_size")) writes -- formed on the device
        (fcu_labels_from_rasters).  Returns the int8 tensor [n, NL] (`out` when given); row i is what set_labels takes."""
        torch = self.torch
        H4, W4 = self.height // 4, self.width // 4
        depth = depth[None] if depth.dim() == 2 else depth
        n = depth.shape[0]
        assert depth.is_cuda and depth.dtype == torch.uint8 and depth.is_contiguous() and tuple(depth.shape[1:]) == (H4, W4)
        if part_size is not None:
            part_size = part_size[None] if part_size.dim() == 2 else part_size
            assert part_size.is_cuda and part_size.dtype in (torch.int8, torch.uint8) and part_size.is_contiguous() and tuple(part_size.shape) == (n, H4, W4)
        if out is None:
            out = torch.empty((n, self.label_count()), dtype=torch.int8, device=depth.device)
        assert out.is_cuda and out.dtype == torch.int8 and out.is_contiguous() and out.numel() == n * self.label_count()
        s = C.c_void_p(stream.cuda_stream) if stream is not None else None
        self._chk(self.lib.fcu_labels_from_rasters(self.h, n, depth.data_ptr(), part_size.data_ptr() if part_size is not None else None, out.data_ptr(), s),
                  "fcu_labels_from_rasters")
        return out

    def verify_counts(self, first, n=1):
        v = VerifyCounts()
        self._chk(self.lib.fcu_get_verify_counts(self.h, first, n, C.byref(v)), "fcu_get_verify_counts")
        return np.array([[v.n[d][k] for k in range(6)] for d in range(4)], np.float64)

    # -- per-PU record of the luma search (BASELINE configs[1])
    def enable_pu_trace(self, chain, trace=None):
        """Binds a device array of n_ctu x 341 fcu_pu_trace records to the chain (several slice chains of a picture may share
        one).  Returns the uint8 tensor; pu_trace_array() turns it into a structured numpy array."""
        torch = self.torch
        if trace is None:
            trace = torch.zeros(self.n_ctu * PUS_PER_CTU * PU_TRACE_DTYPE.itemsize, dtype=torch.uint8, device=torch.device("cuda", self.device))
        self._chk(self.lib.fcu_chain_set_pu_trace(self.h, chain, trace.data_ptr()), "fcu_chain_set_pu_trace")
        self._keep_obf[("pu_trace", chain)] = trace
        return trace

    def pu_trace_array(self, trace):
        return trace.cpu().numpy().view(PU_TRACE_DTYPE).reshape(self.n_ctu, PUS_PER_CTU)

    # -- both RD costs of every CU the search visits (the fork's Training set), and what is made of them on the device
    def enable_cu_trace(self, chain, trace=None):
        """Binds a device array of n_ctu x 85 fcu_cu_trace records to the chain (the slice, row or tile chains of a picture share
        one: pass the tensor the first call returned).  The engine clears a CTU's records when it starts the CTU.  Returns the uint8
        tensor; cu_trace_array() turns it into a structured numpy array."""
        torch = self.torch
        if trace is None:
            trace = torch.zeros(self.n_ctu * CUS_PER_CTU * CU_TRACE_DTYPE.itemsize, dtype=torch.uint8, device=torch.device("cuda", self.device))
        assert trace.is_cuda and trace.dtype == torch.uint8 and trace.is_contiguous() and trace.numel() >= self.n_ctu * CUS_PER_CTU * CU_TRACE_DTYPE.itemsize
        self._chk(self.lib.fcu_chain_set_cu_trace(self.h, chain, trace.data_ptr()), "fcu_chain_set_cu_trace")
        self._keep_obf[("cu_trace", chain)] = trace
        return trace

    def disable_cu_trace(self, chain):
        self._chk(self.lib.fcu_chain_set_cu_trace(self.h, chain, None), "fcu_chain_set_cu_trace")
        self._keep_obf.pop(("cu_trace", chain), None)

    def cu_trace_array(self, trace):
        return trace.cpu().numpy()[:self.n_ctu * CUS_PER_CTU * CU_TRACE_DTYPE.itemsize].view(CU_TRACE_DTYPE).reshape(self.n_ctu, CUS_PER_CTU)

    def _trace_ptrs(self, traces, who):
        ptrs = (C.c_void_p * max(len(traces), 1))()
        for i, t in enumerate(traces):
            t = t["cu_trace"] if isinstance(t, dict) else t
            assert t.is_cuda and t.dtype == self.torch.uint8 and t.is_contiguous() and t.numel() >= self.n_ctu * CUS_PER_CTU * CU_TRACE_DTYPE.itemsize, who
            ptrs[i] = t.data_ptr()
        return ptrs

    def label_score(self, traces, labels, ctu=False, timed=False, stream=None):
        """The Verifying counters of label arrays against the CU traces of exhaustively decided pictures, without deciding them
        again (fcu_label_score).  traces: list of trace tensors (enable_cu_trace; result dicts with "cu_trace" qualify); labels:
        an int8 device tensor [n, NL] or a list of [NL] tensors, picture i against trace i (the layout set_labels takes).
        Returns a structured array [n] of PIC_SCORE_DTYPE: v [4, 6] = TP, FP, TN, FN, FPLoss, FNLoss per depth (what
        decision_switch takes), open [4] (samples whose label is no prediction), scored [4].  ctu=True: also the per-CTU records
        [n, n_ctu] of CTU_SCORE_DTYPE; timed=True: also the durations (ms) of the two kernels.  The extras follow in that order."""
        torch = self.torch
        n = len(traces)
        labs = [labels[i] for i in range(n)]
        assert len(labels) == n
        for t in labs:
            assert t.is_cuda and t.dtype == torch.int8 and t.is_contiguous() and t.numel() == self.label_count(), "label_score: int8 [NL] on the device"
        tp = self._trace_ptrs(traces, "label_score")
        lp = (C.c_void_p * max(n, 1))(*[t.data_ptr() for t in labs])
        rec = np.zeros(max(n, 1), PIC_SCORE_DTYPE)
        d_ctu = torch.empty((n, self.n_ctu, CTU_SCORE_DTYPE.itemsize), dtype=torch.uint8, device=torch.device("cuda", self.device)) if ctu else None
        ms = (C.c_float * 2)() if timed else None
        s = C.c_void_p(stream.cuda_stream) if stream is not None else None
        self._chk(self.lib.fcu_label_score(self.h, n, tp, lp, rec.ctypes.data, d_ctu.data_ptr() if ctu else None, ms, s), "fcu_label_score")
        rec = rec[:n]
        if not ctu and not timed:
            return rec
        extra = ([d_ctu.cpu().numpy().view(CTU_SCORE_DTYPE).reshape(n, self.n_ctu)] if ctu else []) + ([(ms[0], ms[1])] if timed else [])
        return (rec, *extra)

    def trace_maps(self, traces, labels=True, costs=False, timed=False, stream=None):
        """CU traces as the fork's whole Training set, in the layout of the label / N_OBF maps of decision_maps, formed on the
        device (fcu_trace_maps).  Returns a dict of device tensors over the batch: "labels" (labels=True) int8 [n, NL] --
        LABEL_SPLIT / LABEL_NOT_SPLIT for every CU the search visited and tried to split, LABEL_ABSENT for the others, LABEL_FORCED
        where the picture edge cuts the block --, "j0" / "j1" (costs=True) float64 [n, NL], 0.0 where there is no label.  Element
        for element aligned with decision_maps(...)["n_obf"] flattened.  timed=True: (dict, kernel ms)."""
        torch = self.torch
        n, NL = len(traces), self.label_count()
        dev = torch.device("cuda", self.device)
        tp = self._trace_ptrs(traces, "trace_maps")
        d_lab = torch.empty((n, NL), dtype=torch.int8, device=dev) if labels else None
        d_j0 = torch.empty((n, NL), dtype=torch.float64, device=dev) if costs else None
        d_j1 = torch.empty((n, NL), dtype=torch.float64, device=dev) if costs else None
        ptr = lambda t: t.data_ptr() if t is not None else None
        ms = C.c_float(0)
        s = C.c_void_p(stream.cuda_stream) if stream is not None else None
        self._chk(self.lib.fcu_trace_maps(self.h, n, tp, ptr(d_lab), ptr(d_j0), ptr(d_j1), C.byref(ms) if timed else None, s), "fcu_trace_maps")
        res = {k: v for k, v in (("labels", d_lab), ("j0", d_j0), ("j1", d_j1)) if v is not None}
        return (res, float(ms.value)) if timed else res

    # -- the risk-table model: trained on CU traces and run on the device
    def _key_ptrs(self, keys, who):
        n = len(keys)
        rows = [keys[i] for i in range(n)]
        for t in rows:
            assert t.is_cuda and t.dtype in (self.torch.uint16, self.torch.int16) and t.is_contiguous() and t.numel() == self.label_count(), who + ": uint16 [NL] keys on the device"
        return (C.c_void_p * max(n, 1))(*[t.data_ptr() for t in rows]), rows

    def risk_train(self, traces, keys, model=None, accumulate=False, timed=False, stream=None):
        """Trains the risk-table model on the CU traces of exhaustively decided pictures (fcu_risk_train; definition: include/fcu.h).
        traces: list of trace tensors (enable_cu_trace; result dicts with "cu_trace" qualify); keys: a uint16 device tensor [n, NL]
        or a list of [NL] tensors -- nobf_maps(obf), or any feature quantised to 0..256 -- block for block aligned with trace_maps.
        model: the uint8 device tensor of one fcu_risk_model to write (accumulate=False: overwritten, nothing to clear) or to add
        the batch to (accumulate=True); None: a new one.  Returns (model, dropped): dropped = samples whose key was >= 257.
        timed=True: also the durations (ms) of the two kernels."""
        torch = self.torch
        n = len(traces)
        assert len(keys) == n
        tp = self._trace_ptrs(traces, "risk_train")
        kp, keep = self._key_ptrs(keys, "risk_train")
        if model is None:
            assert not accumulate, "risk_train: accumulate=True adds to a model"
            model = torch.empty(RISK_MODEL_DTYPE.itemsize, dtype=torch.uint8, device=torch.device("cuda", self.device))
        assert model.is_cuda and model.dtype == torch.uint8 and model.is_contiguous() and model.numel() == RISK_MODEL_DTYPE.itemsize, "risk_train: one fcu_risk_model as uint8 on the device"
        dropped = C.c_uint32(0)
        ms = (C.c_float * 2)() if timed else None
        s = C.c_void_p(stream.cuda_stream) if stream is not None else None
        self._chk(self.lib.fcu_risk_train(self.h, n, tp, kp, model.data_ptr(), 1 if accumulate else 0, C.byref(dropped), ms, s), "fcu_risk_train")
        return (model, int(dropped.value), (ms[0], ms[1])) if timed else (model, int(dropped.value))

    def risk_predict(self, keys, model, min_count=1, timed=False, stream=None):
        """The model's labels for pictures that need not be decided yet (fcu_risk_predict): keys as in risk_train, model the tensor
        risk_train returned.  Returns the int8 device tensor [n, NL]; row i is what set_labels takes: LABEL_FORCED where the picture
        edge cuts the block, LABEL_ABSENT for a key >= 257 or a bin with fewer than min_count samples, else the rule.  timed=True:
        (tensor, kernel ms)."""
        torch = self.torch
        kp, keep = self._key_ptrs(keys, "risk_predict")
        n = len(keep)
        assert model.is_cuda and model.dtype == torch.uint8 and model.is_contiguous() and model.numel() == RISK_MODEL_DTYPE.itemsize, "risk_predict: one fcu_risk_model as uint8 on the device"
        out = torch.empty((n, self.label_count()), dtype=torch.int8, device=model.device)
        ms = C.c_float(0)
        s = C.c_void_p(stream.cuda_stream) if stream is not None else None
        self._chk(self.lib.fcu_risk_predict(self.h, n, kp, model.data_ptr(), int(min_count), out.data_ptr(), C.byref(ms) if timed else None, s), "fcu_risk_predict")
        return (out, float(ms.value)) if timed else out

    def nobf_maps(self, obf, stream=None):
        """The N_OBF maps of pictures that have not been decided (fcu_nobf_maps): obf = an int16 device tensor [n, height / 4,
        width / 4] (or one map, or a list of maps) of obf_prepass.  Returns the uint16 device tensor [n, NL]: the bytes
        decision_maps(..., obf=...)["n_obf"] flattened."""
        torch = self.torch
        maps = [obf] if torch.is_tensor(obf) and obf.dim() == 2 else [obf[i] for i in range(len(obf))]
        for t in maps:
            assert t.is_cuda and t.dtype == torch.int16 and t.is_contiguous() and tuple(t.shape) == (self.height // 4, self.width // 4), "nobf_maps: int16 [height / 4, width / 4] on the device"
        n = len(maps)
        out = torch.empty((n, self.label_count()), dtype=torch.uint16, device=torch.device("cuda", self.device))
        ptrs = (C.c_void_p * max(n, 1))(*[t.data_ptr() for t in maps])
        s = C.c_void_p(stream.cuda_stream) if stream is not None else None
        self._chk(self.lib.fcu_nobf_maps(self.h, n, ptrs, out.data_ptr(), s), "fcu_nobf_maps")
        return out

    # -- the key tree: risk-table keys learnt from the feature maps (include/fcu.h)
    def _bins_ptrs(self, bins, F, who):
        n = len(bins)
        rows = [bins[i] for i in range(n)]
        for t in rows:
            assert t.is_cuda and t.dtype == self.torch.uint8 and t.is_contiguous() and t.numel() == self.label_count() * F, who + ": uint8 [NL, F] bins on the device"
        return (C.c_void_p * max(n, 1))(*[t.data_ptr() for t in rows]), rows

    def feature_bins(self, features, edges, sets=("tmv", "soc"), out=None, timed=False, stream=None):
        """The columns of feature_maps quantised to 32 bins (fcu_feature_bins): features float32 [n, NL, F] on the device; edges
        float32 [4, F, 31] -- a device tensor (feature_edges; read as it is) or a host array, which is checked to be finite and
        non-decreasing (fcu_feature_edges_check) and copied.  Returns the uint8 device tensor [n, NL, F] (out: a contiguous uint8
        tensor of that many bytes to write instead, at any byte offset).  timed=True: (tensor, kernel ms)."""
        torch = self.torch
        mask, names = feature_sets(sets)
        F, NL = sum(FEATURE_COUNTS[k] for k in names), self.label_count()
        assert features.is_cuda and features.dtype == torch.float32 and features.is_contiguous() and features.dim() == 3 and tuple(features.shape[1:]) == (NL, F), "feature_bins: float32 [n, NL, F] on the device"
        n = features.shape[0]
        if not torch.is_tensor(edges):
            e = np.ascontiguousarray(edges, np.float32)
            assert e.shape == (4, F, TREE_BINS - 1), "feature_bins: edges are [4, F, 31]"
            self._chk(self.lib.fcu_feature_edges_check(e.ctypes.data, mask), "fcu_feature_edges_check")
            edges = torch.tensor(e, device=features.device)
        assert edges.is_cuda and edges.dtype == torch.float32 and edges.is_contiguous() and tuple(edges.shape) == (4, F, TREE_BINS - 1), "feature_bins: edges are float32 [4, F, 31]"
        if out is None:
            out = torch.empty((n, NL, F), dtype=torch.uint8, device=features.device)
        assert out.is_cuda and out.dtype == torch.uint8 and out.is_contiguous() and out.numel() == n * NL * F, "feature_bins: out is uint8 [n, NL, F]"
        ms = C.c_float(0)
        s = C.c_void_p(stream.cuda_stream) if stream is not None else None
        self._chk(self.lib.fcu_feature_bins(self.h, n, mask, features.data_ptr(), edges.data_ptr(), out.data_ptr(), C.byref(ms) if timed else None, s), "fcu_feature_bins")
        return (out, float(ms.value)) if timed else out

    def tree_keys(self, bins, tree, levels=None, sets=("tmv", "soc"), timed=False, stream=None):
        """The key of every block (fcu_tree_keys): bins the uint8 device tensor [n, NL, F] of feature_bins, tree a KeyTree; levels
        (default tree.levels) below tree.levels gives the node-in-level index training needs.  Returns the uint16 device tensor
        [n, NL] that risk_train / risk_predict take as keys.  timed=True: (tensor, kernel ms)."""
        torch = self.torch
        mask, names = feature_sets(sets)
        F, NL = sum(FEATURE_COUNTS[k] for k in names), self.label_count()
        assert bins.is_cuda and bins.dtype == torch.uint8 and bins.is_contiguous() and bins.numel() % (NL * F) == 0 and bins.numel() > 0, "tree_keys: uint8 [n, NL, F] on the device"
        n = bins.numel() // (NL * F)
        out = torch.empty((n, NL), dtype=torch.uint16, device=bins.device)
        ms = C.c_float(0)
        s = C.c_void_p(stream.cuda_stream) if stream is not None else None
        self._chk(self.lib.fcu_tree_keys(self.h, n, mask, bins.data_ptr(), C.byref(tree), int(tree.levels if levels is None else levels), out.data_ptr(), C.byref(ms) if timed else None, s), "fcu_tree_keys")
        return (out, float(ms.value)) if timed else out

    def tree_hist(self, traces, bins, level, nodes=None, sets=("tmv", "soc"), hist=None, accumulate=False, timed=False, stream=None):
        """The histograms a level of the tree is chosen from (fcu_tree_hist).  traces: as risk_train; bins: a uint8 tensor
        [n, NL, F] or a list of [NL, F] tensors; nodes: uint16 [n, NL] (or a list) from tree_keys(levels=level), None at level 0.
        hist: (risk int64, count uint32) device tensors [4, 2^level, F, 32, 2] to write (accumulate=False: overwritten, nothing to
        clear) or to add to; None: new ones.  Returns (risk, count, dropped) -- dropped = samples whose node was >= 2^level.
        timed=True: also the durations (ms) of the two kernels."""
        torch = self.torch
        mask, names = feature_sets(sets)
        F = sum(FEATURE_COUNTS[k] for k in names)
        n = len(traces)
        assert len(bins) == n and (nodes is None or len(nodes) == n)
        tp = self._trace_ptrs(traces, "tree_hist")
        bp, keep_b = self._bins_ptrs(bins, F, "tree_hist")
        np_, keep_n = self._key_ptrs(nodes, "tree_hist") if nodes is not None else (None, None)
        shape = tree_hist_shape(F, level)
        if hist is None:
            assert not accumulate, "tree_hist: accumulate=True adds to histograms"
            dev = torch.device("cuda", self.device)
            hist = (torch.empty(shape, dtype=torch.int64, device=dev), torch.empty(shape, dtype=torch.uint32, device=dev))
        risk, count = hist
        assert risk.is_cuda and risk.dtype == torch.int64 and risk.is_contiguous() and tuple(risk.shape) == shape and count.is_cuda and count.dtype == torch.uint32 and count.is_contiguous() and tuple(count.shape) == shape, "tree_hist: int64 / uint32 [4, 2^level, F, 32, 2] on the device"
        dropped = C.c_uint32(0)
        ms = (C.c_float * 2)() if timed else None
        s = C.c_void_p(stream.cuda_stream) if stream is not None else None
        self._chk(self.lib.fcu_tree_hist(self.h, n, mask, int(level), tp, bp, np_, risk.data_ptr(), count.data_ptr(), 1 if accumulate else 0, C.byref(dropped), ms, s), "fcu_tree_hist")
        return (risk, count, int(dropped.value), (ms[0], ms[1])) if timed else (risk, count, int(dropped.value))

    def tree_train(self, traces, bins, levels, min_count=1, sets=("tmv", "soc"), timed=False, stream=None):
        """Trains a KeyTree of `levels` levels level by level (fcu_tree_train): keys, histograms, the copy of a level's histograms
        to the host, the split choice.  traces / bins as tree_hist.  Synchronous.  Returns the KeyTree; timed=True: (tree, the
        kernels' durations added up in ms)."""
        mask, names = feature_sets(sets)
        F = sum(FEATURE_COUNTS[k] for k in names)
        n = len(traces)
        assert len(bins) == n
        tp = self._trace_ptrs(traces, "tree_train")
        bp, keep_b = self._bins_ptrs(bins, F, "tree_train")
        tree = KeyTree()
        ms = C.c_float(0)
        s = C.c_void_p(stream.cuda_stream) if stream is not None else None
        self._chk(self.lib.fcu_tree_train(self.h, n, mask, int(levels), int(min_count), tp, bp, C.byref(tree), C.byref(ms) if timed else None, s), "fcu_tree_train")
        return (tree, float(ms.value)) if timed else tree

    # -- getTMVFeature / FormFeatureVector(SOC)
    def feature_maps(self, lumas, sets=("tmv", "soc"), yc=None, timed=False, stream=None):
        """The fork's per-CU model inputs, formed on the device from the luma planes (fcu_feature_maps): the 5 x 26 TMV texture
        statistics of getTMVFeature ("tmv", 130 columns) and the outlier-coefficient sums of FormFeatureVector ("soc", 16
        columns); definition and quirks: include/fcu.h.  lumas: list of uint8 device tensors [height, width] (dense; views at
        any byte offset allowed), or of dicts with `org` or of (Y, U, V) triples, of which the luma plane is read.  yc: float64
        [n, 16], the thresholds obf_prepass returned for these pictures -- given exactly when "soc" is asked for.
        Returns a float32 device tensor [n, NL, F] (F = len(feature_columns(sets)), "tmv" columns first): row r of picture i
        belongs to the block of row r of decision_maps(...)["labels"] / ["n_obf"] flattened and of trace_maps(...); a block
        the picture edge cuts (LABEL_FORCED) has a row of zeros.  timed=True: (tensor, kernel ms)."""
        torch = self.torch
        mask, names = feature_sets(sets)
        n, NL, F = len(lumas), self.label_count(), sum(FEATURE_COUNTS[k] for k in names)
        dev = torch.device("cuda", self.device)
        ptrs, keep = (C.c_void_p * max(n, 1))(), []
        for i, p in enumerate(lumas):
            t = p["org"][0] if isinstance(p, dict) else (p if torch.is_tensor(p) else p[0])
            assert t.is_cuda and t.dtype == torch.uint8 and tuple(t.shape) == (self.height, self.width) and t.is_contiguous(), "feature_maps: dense uint8 luma planes on the device"
            keep.append(t)
            ptrs[i] = t.data_ptr()
        ycp = None
        if yc is not None:
            yc = np.ascontiguousarray(np.asarray(yc, np.float64).reshape(-1, 16))
            assert yc.shape[0] == n, "feature_maps: one row of 16 thresholds per picture"
            ycp = yc.ctypes.data
        out = torch.empty((n, NL, F), dtype=torch.float32, device=dev)
        ms = C.c_float(0)
        s = C.c_void_p(stream.cuda_stream) if stream is not None else None
        self._chk(self.lib.fcu_feature_maps(self.h, n, mask, ptrs, ycp, out.data_ptr(), C.byref(ms) if timed else None, s), "fcu_feature_maps")
        return (out, float(ms.value)) if timed else out

    # -- TComLoopFilter::loopFilterPic
    def deblock(self, chain=None, beta_offset_div2=0, tc_offset_div2=0, timed=False, stream=None, out=None, rec=None, tiles=None, lf_cross_tiles=1, slice_ctus=None, lf_cross_slices=1, layout=None):
        """Deblocks, in place, the reconstruction planes bound to `chain` (all slice chains of a picture share them)
        once every CTU of the picture has been decided -- or explicit device tensors: `out` = the picture's
        fcu_ctu_out array as uint8, `rec` = (Y, U, V).  tiles=(C, R): the picture's uniform tile grid, filtered with
        LFCrossTileBoundaryFlag = lf_cross_tiles (fcu_deblock_tiles; 0 leaves the tile boundaries unfiltered); without tiles
        lf_cross_tiles is not looked at.  slice_ctus: CTUs per slice of a picture of SliceMode 1 slices, filtered with
        LFCrossSliceBoundaryFlag = lf_cross_slices (fcu_deblock_slices; 0 leaves the slice boundaries unfiltered); None: fcu_deblock,
        the flag 1.  layout: a PictureLayout to take all four from.  Returns (ms vertical pass, ms horizontal pass) if timed."""
        if layout is not None:
            tiles, lf_cross_tiles = layout.tiles, layout.lf_cross_tiles
            slice_ctus, lf_cross_slices = (layout.sao_slice_ctus, layout.lf_cross_slices) if layout.lf_cross_slices != 1 else (None, 1)
        if tiles is not None and slice_ctus:
            raise ValueError("CuEngine.deblock: tiles need one slice per picture (no slice_ctus)")
        if chain is not None:
            _, rec, out = self._keep[chain]
        assert out.numel() >= self.n_ctu * CTU_OUT_BYTES and rec[0].numel() == self.width * self.height
        ms = (C.c_float * 2)() if timed else None
        s = C.c_void_p(stream.cuda_stream) if stream is not None else None
        if tiles is not None:
            self._chk(self.lib.fcu_deblock_tiles(self.h, out.data_ptr(), rec[0].data_ptr(), rec[1].data_ptr(), rec[2].data_ptr(),
                                                 beta_offset_div2, tc_offset_div2, int(tiles[0]), int(tiles[1]), int(lf_cross_tiles), ms, s), "fcu_deblock_tiles")
        elif slice_ctus is not None:
            self._chk(self.lib.fcu_deblock_slices(self.h, out.data_ptr(), rec[0].data_ptr(), rec[1].data_ptr(), rec[2].data_ptr(),
                                                  beta_offset_div2, tc_offset_div2, int(slice_ctus), int(lf_cross_slices), ms, s), "fcu_deblock_slices")
        else:
            self._chk(self.lib.fcu_deblock(self.h, out.data_ptr(), rec[0].data_ptr(), rec[1].data_ptr(), rec[2].data_ptr(),
                                           beta_offset_div2, tc_offset_div2, ms, s), "fcu_deblock")
        return (ms[0], ms[1]) if timed else None

    # -- TEncSampleAdaptiveOffset::SAOProcess
    def sao(self, pictures, timed=False, stream=None, tiles=None, lf_cross_tiles=1, lf_cross_slices=1, layout=None):
        """SAO of completely decided, deblocked pictures, in place on their reconstruction planes.  pictures: list of dicts
        {org: (Y,U,V) device tensors, rec: (Y,U,V) device tensors, qp, lambda_ (the slice's luma lambda), slice_type,
        slice_ctus, enabled (3 ints, default all on), chroma_weight (default: from the QP, chroma QP offset 0)}.
        tiles=(C, R): every picture of the batch is cut into C x R uniform tiles (fcu_sao_tiles): merge candidates stay inside
        the CTU's tile, and with lf_cross_tiles=0 (LFCrossTileBoundaryFlag) so do the samples the statistics and the offset pass
        read; slice_ctus must then be 0.  lf_cross_slices: LFCrossSliceBoundaryFlag of the pictures' slices (each picture's
        slice_ctus); 0 (fcu_sao_slices) keeps the samples the statistics and the offset pass read inside the CTU's slice.
        layout: a PictureLayout to take all three from.  Returns (coded uint8 tensor
        [n, n_ctu, SAO_CTU_BYTES] on the device, off_count int32 array [n, 3], kernel ms x4 or None)."""
        if layout is not None:
            tiles, lf_cross_tiles, lf_cross_slices = layout.tiles, layout.lf_cross_tiles, layout.lf_cross_slices
        torch = self.torch
        n = len(pictures)
        dev = torch.device("cuda", self.device)
        prm = (SaoParams * n)()
        org, rec = (C.c_void_p * (3 * n))(), (C.c_void_p * (3 * n))()
        for i, p in enumerate(pictures):
            w = p.get("chroma_weight")
            prm[i].slice_type, prm[i].qp, prm[i].slice_ctus = p.get("slice_type", SLICE_I), p["qp"], p.get("slice_ctus", 0)
            lam = p["lambda_"]
            for k in range(3):
                prm[i].enabled[k] = int(p.get("enabled", (1, 1, 1))[k])
                prm[i].lambda_[k] = lam if k == 0 else (lam / w if w else 0.0)
                for t in (p["org"][k], p["rec"][k]):
                    assert t.is_cuda and t.dtype == torch.uint8 and t.is_contiguous() and t.numel() == (self.width >> (1 if k else 0)) * (self.height >> (1 if k else 0))
                org[3 * i + k], rec[3 * i + k] = p["org"][k].data_ptr(), p["rec"][k].data_ptr()
        coded = torch.zeros((n, self.n_ctu, SAO_CTU_BYTES), dtype=torch.uint8, device=dev)
        off = np.zeros((n, 3), np.int32)
        ms = (C.c_float * 4)() if timed else None
        s = C.c_void_p(stream.cuda_stream) if stream is not None else None
        if tiles is not None:
            self._chk(self.lib.fcu_sao_tiles(self.h, n, prm, int(tiles[0]), int(tiles[1]), int(lf_cross_tiles), org, rec, coded.data_ptr(), off.ctypes.data, ms, s), "fcu_sao_tiles")
        elif lf_cross_slices != 1:
            self._chk(self.lib.fcu_sao_slices(self.h, n, prm, int(lf_cross_slices), org, rec, coded.data_ptr(), off.ctypes.data, ms, s), "fcu_sao_slices")
        else:
            self._chk(self.lib.fcu_sao(self.h, n, prm, org, rec, coded.data_ptr(), off.ctypes.data, ms, s), "fcu_sao")
        return coded, off, (list(ms) if timed else None)

    # -- TEncGOP::xCalculateAddPSNR
    def report(self, pictures, ctu=False, timed=False, stream=None):
        """The picture report of decided (and filtered) pictures, taken on the device (fcu_picture_report).  pictures: list of
        dicts {org: (Y,U,V) uint8 device tensors, rec: (Y,U,V) uint8 device tensors, out: the picture's fcu_ctu_out array as a
        uint8 device tensor}; the planes may be views at any byte offset as long as their rows are dense.  Returns one dict
        per picture: ssd[3], bits, bins, dist, n_samples[3], n_part, depth_part[4], part_size_part[8], intra_part, skip_part,
        merge_part, cbf_part[3] (integers, counters in 4x4 luma partitions inside the picture) and psnr[3] (float64, HM's
        expression).  ctu=True: also the per-CTU records, a structured array [n, n_ctu] of CTU_REPORT_DTYPE; timed=True: also
        the durations (ms) of the two kernels.  The extras follow the list in that order."""
        torch = self.torch
        n = len(pictures)
        org, rec, out = (C.c_void_p * (3 * n))(), (C.c_void_p * (3 * n))(), (C.c_void_p * n)()
        for i, p in enumerate(pictures):
            for k in range(3):
                w, h = self.width >> (1 if k else 0), self.height >> (1 if k else 0)
                for t in (p["org"][k], p["rec"][k]):
                    assert t.is_cuda and t.dtype == torch.uint8 and tuple(t.shape) == (h, w) and t.is_contiguous()
                org[3 * i + k], rec[3 * i + k] = p["org"][k].data_ptr(), p["rec"][k].data_ptr()
            o = p["out"]
            assert o.is_cuda and o.dtype == torch.uint8 and o.is_contiguous() and o.numel() >= self.n_ctu * CTU_OUT_BYTES
            out[i] = o.data_ptr()
        reports = np.zeros(max(n, 1), PIC_REPORT_DTYPE)
        d_ctu = torch.empty((n, self.n_ctu, CTU_REPORT_DTYPE.itemsize), dtype=torch.uint8, device=torch.device("cuda", self.device)) if ctu else None
        ms = (C.c_float * 2)() if timed else None
        s = C.c_void_p(stream.cuda_stream) if stream is not None else None
        self._chk(self.lib.fcu_picture_report(self.h, n, org, rec, out, reports.ctypes.data, d_ctu.data_ptr() if ctu else None, ms, s), "fcu_picture_report")
        res = [pic_report_to_dict(reports[i]) for i in range(n)]
        if not ctu and not timed:
            return res
        extra = ([d_ctu.cpu().numpy().view(CTU_REPORT_DTYPE).reshape(n, self.n_ctu)] if ctu else []) + ([(ms[0], ms[1])] if timed else [])
        return (res, *extra)

    # -- calcMD5 / calcCRC / calcChecksum
    def picture_hash(self, pictures, kinds=("md5",), timed=False, stream=None):
        """The decoded-picture hash of reconstructed pictures as HM computes and prints it, taken on the device
        (fcu_picture_hash): per plane the MD5, the CRC or the checksum of TComPicYuvMD5.cpp.  pictures: list of dicts with `rec`
        (the result dicts of the drivers qualify) or of (Y, U, V) triples -- uint8 device tensors, dense, views at any byte
        offset allowed (16-byte aligned planes take 16-byte loads).  kinds: any of "md5", "crc", "checksum"; only those are
        computed.  Returns one dict per picture: per kind the three planes' digests in hex, and under "line" per kind HM's
        string (the three joined by ','), e.g. {"md5": [hex, hex, hex], "line": {"md5": "...,...,..."}}.  timed=True: also the
        durations (ms) of the three kernels (partials, fold, MD5; 0 for one that was not launched).
        16 to 48 bytes per picture come back instead of the planes.  Measured on one MI355X at 4K (tests/hash_bench.py,
        profiles/hash_bench.json): CRC or checksum 0.05 ms per call for one picture, 0.20-0.22 ms for sixteen (the copy of the
        planes alone: 0.26-0.41 ms per picture).  MD5 is one serial chain per plane, one plane per lane: 129 ms for one picture
        and 126 ms for sixteen, against 12.7 ms per picture for copy + hashlib.md5 -- slower than the host below about ten
        pictures per call."""
        torch = self.torch
        kinds = (kinds,) if isinstance(kinds, str) else tuple(kinds)
        mask = 0
        for k in kinds:
            if k not in HASH_KINDS:
                raise ValueError("picture_hash: kinds are among %s, not %r" % (sorted(HASH_KINDS), k))
            mask |= HASH_KINDS[k]
        n = len(pictures)
        planes = (C.c_void_p * (3 * n))()
        for i, p in enumerate(pictures):
            rec = p["rec"] if isinstance(p, dict) else p
            for k in range(3):
                w, h = self.width >> (1 if k else 0), self.height >> (1 if k else 0)
                t = rec[k]
                assert t.is_cuda and t.dtype == torch.uint8 and tuple(t.shape) == (h, w) and t.is_contiguous()
                planes[3 * i + k] = t.data_ptr()
        hashes = np.zeros(max(n, 1), PIC_HASH_DTYPE)
        ms = (C.c_float * 3)() if timed else None
        s = C.c_void_p(stream.cuda_stream) if stream is not None else None
        self._chk(self.lib.fcu_picture_hash(self.h, n, mask, planes, hashes.ctypes.data, ms, s), "fcu_picture_hash")
        res = []
        for i in range(n):
            d = {k: [bytes(hashes[i][k][c]).hex() for c in range(3)] for k in kinds}
            d["line"] = {k: hash_string(hashes[i], k) for k in kinds}
            res.append(d)
        return (res, (ms[0], ms[1], ms[2])) if timed else res

    # -- the decision as pictures
    def _out_ptrs(self, pics, who):
        ptrs = (C.c_void_p * max(len(pics), 1))()
        for i, p in enumerate(pics):
            o = p["out"] if isinstance(p, dict) else p
            assert o.is_cuda and o.dtype == self.torch.uint8 and o.is_contiguous() and o.numel() >= self.n_ctu * CTU_OUT_BYTES, who
            ptrs[i] = o.data_ptr()
        return ptrs

    def decision_maps(self, pics, fields=("depth",), mv=False, labels=False, obf=None, timed=False, stream=None):
        """The decision of decided pictures as rasters aligned with the pixels, formed on the device (fcu_decision_maps).
        pics: list of dicts with `out` (the result dicts of the drivers qualify) or of the fcu_ctu_out arrays themselves, uint8
        device tensors.  fields: names among MAP_FIELDS, in the order wanted.  Returns a dict of device tensors over the batch
        (n = len(pics), H4 = height / 4, W4 = width / 4):
          one entry per field name   [n, H4, W4], uint8 or (MAP_SIGNED) int8: the array's bytes with z-order undone
          "mv"      (mv=True)        int16 [n, H4, W4, 2], quarter samples [hor, ver]
          "labels"  (labels=True)    four int8 tensors [n, ceil(height / s), ceil(width / s)], s = 64, 32, 16, 8: LABEL_* per block --
                                     the split flags of the CUs on the chosen tree (at s = 8: NxN or not); LABEL_ABSENT where the
                                     parent was not split, LABEL_FORCED where the picture edge forced the split
          "n_obf"   (obf given)      four int16 tensors of those shapes: the fork's N_OBF feature of the block (values 0..256)
        obf: the pictures' OBF maps from obf_prepass, an int16 tensor [n, H4, W4] or a list of [H4, W4] tensors.
        timed=True: (dict, kernel ms).  The level tensors are views into one allocation per kind (rows of a picture are dense)."""
        torch = self.torch
        fields = (fields,) if isinstance(fields, str) else tuple(fields)
        for f in fields:
            if f not in MAP_FIELDS:
                raise ValueError("decision_maps: fields are among %s, not %r" % (sorted(MAP_FIELDS), f))
        n, H4, W4 = len(pics), self.height // 4, self.width // 4
        dev = torch.device("cuda", self.device)
        outs = self._out_ptrs(pics, "decision_maps")
        shapes = map_level_shapes(self.width, self.height)
        NL = sum(a * b for a, b in shapes)
        ids = (C.c_int * max(len(fields), 1))(*[MAP_FIELDS[f] for f in fields])
        d_bytes = torch.empty((n, len(fields), H4, W4), dtype=torch.uint8, device=dev) if fields else None
        d_mv = torch.empty((n, H4, W4, 2), dtype=torch.int16, device=dev) if mv else None
        d_lab = torch.empty((n, NL), dtype=torch.int8, device=dev) if labels else None
        d_nobf, obf_ptrs, keep = None, None, None
        if obf is not None:
            keep = [obf[i] for i in range(n)]
            assert len(obf) == n
            for o in keep:
                assert o.is_cuda and o.dtype == torch.int16 and o.is_contiguous() and tuple(o.shape) == (H4, W4)
            obf_ptrs = (C.c_void_p * n)(*[o.data_ptr() for o in keep])
            d_nobf = torch.empty((n, NL), dtype=torch.int16, device=dev)
        ptr = lambda t: t.data_ptr() if t is not None else None
        ms = C.c_float(0)
        s = C.c_void_p(stream.cuda_stream) if stream is not None else None
        self._chk(self.lib.fcu_decision_maps(self.h, n, outs, len(fields), ids, ptr(d_bytes), ptr(d_mv), ptr(d_lab), obf_ptrs, ptr(d_nobf),
                                             C.byref(ms) if timed else None, s), "fcu_decision_maps")
        res = {}
        for k, f in enumerate(fields):
            res[f] = d_bytes[:, k].view(torch.int8) if f in MAP_SIGNED else d_bytes[:, k]
        if mv:
            res["mv"] = d_mv
        for name, t in (("labels", d_lab), ("n_obf", d_nobf)):
            if t is not None:
                res[name], o = [], 0
                for bh, bw in shapes:
                    res[name].append(t[:, o:o + bh * bw].unflatten(1, (bh, bw)))
                    o += bh * bw
        return (res, float(ms.value)) if timed else res

    def split_match(self, pics_a, pics_b, ctu=False, timed=False, stream=None):
        """How far two decisions of the same pictures agree, counted on the device (fcu_split_match): pics_a / pics_b as
        decision_maps takes them, picture i of one against picture i of the other.  Returns one dict per picture
        (pic_match_to_dict): part_total, part_equal (partitions of equal depth), split_match = their quotient, node[4][2][2]
        (blocks that carry a coded split flag in both: by level, flag in A, flag in B), only_a[4], only_b[4] (a CU in one, absent
        in the other).  ctu=True: also the per-CTU records, a structured array [n, n_ctu] of CTU_MATCH_DTYPE; timed=True: also the
        durations (ms) of the two kernels.  The extras follow the list in that order."""
        torch = self.torch
        n = len(pics_a)
        assert len(pics_b) == n
        a, b = self._out_ptrs(pics_a, "split_match"), self._out_ptrs(pics_b, "split_match")
        rec = np.zeros(max(n, 1), PIC_MATCH_DTYPE)
        d_ctu = torch.empty((n, self.n_ctu, CTU_MATCH_DTYPE.itemsize), dtype=torch.uint8, device=torch.device("cuda", self.device)) if ctu else None
        ms = (C.c_float * 2)() if timed else None
        s = C.c_void_p(stream.cuda_stream) if stream is not None else None
        self._chk(self.lib.fcu_split_match(self.h, n, a, b, rec.ctypes.data, d_ctu.data_ptr() if ctu else None, ms, s), "fcu_split_match")
        res = [pic_match_to_dict(rec[i]) for i in range(n)]
        if not ctu and not timed:
            return res
        extra = ([d_ctu.cpu().numpy().view(CTU_MATCH_DTYPE).reshape(n, self.n_ctu)] if ctu else []) + ([(ms[0], ms[1])] if timed else [])
        return (res, *extra)

    # -- TEncCu::destroy
    def destroy(self):
        if self.h:
            self.lib.fcu_destroy(self.h)
            self.h = C.c_void_p()
        self._keep = {}
        self._keep_obf = {}
        self._keep_ref = {}

    def __del__(self):
        try:
            self.destroy()
        except Exception:
            pass
