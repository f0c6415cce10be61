"""Picture-level host driver around the engine: what TEncTop / TEncGOP / TEncSlice do around `TEncCu` for an
all-intra sequence, reduced to the calls of include/fcu.h.

  FastDecisionSchedule   the fork's per-picture control of its fast CU decision: state of the picture
                         (getCurrentState, tools_YS.cpp:1237-1242), reset at the start of a period
                         (TEncTop.cpp:393-398 -> resetYSGlobal, tools_YS.cpp:89-110), switches from the Verifying
                         pictures' counters after the last of them (TEncTop.cpp:548-552 -> ReportPerformance ->
                         SetDecisionSwitch, tools_YS.cpp:1123-1154).  Pure host logic, engine-agnostic.
  SequenceDecider        per picture: OBF pre-pass (TEncGOP.cpp:1096), one chain per slice (TEncGOP.cpp:1102-1138,
                         SliceMode 1), the decisions, the in-loop deblocking (TEncGOP.cpp:1155-1160).
  read_yuv420 / write_yuv420   planar 8-bit 4:2:0 files as TVideoIOYuv reads / writes them for fileBitDepth 8
                         (TLibVideoIO/TVideoIOYuv.cpp:247-400 readPlane, :402-560 writePlane, :680, :767).

torch is plumbing (device buffers); there is no CPU fallback for the decisions.
"""
import numpy as np

from . import engine as _engine
from .layout import PictureLayout

TRAINING, VERIFYING, TESTING = _engine.TRAINING, _engine.VERIFYING, _engine.TESTING


class FastDecisionSchedule:
    """The reference keeps this state in globals (g_iPOC, g_iP/g_iT/g_iV, g_iVerResult, g_bDecisionSwitch); here the
    caller owns it.  `decision_switch` / `frame_state` default to the host functions of libfcu.so."""

    def __init__(self, period=60, n_training=2, n_verifying=1, th_skip=(0, 0, 0, 0), th_term=(0, 0, 0, 0),
                 decision_switch=None, frame_state=None):
        self.period, self.n_training, self.n_verifying = period, n_training, n_verifying
        self.th_skip, self.th_term = th_skip, th_term
        self._switch = decision_switch or _engine.decision_switch
        self._state = frame_state or _engine.frame_state
        self.sw_skip = np.zeros(4, np.uint8)
        self.sw_term = np.zeros(4, np.uint8)
        self.ver = np.zeros((4, 6), np.float64)

    def begin_picture(self, poc):
        """State and switches picture `poc` is decided with."""
        if poc % self.period == 0:                        # resetYSGlobal: counters and switches start again
            self.sw_skip[:] = 0
            self.sw_term[:] = 0
            self.ver[:] = 0
        return self._state(poc, self.period, self.n_training, self.n_verifying), self.sw_skip.copy(), self.sw_term.copy()

    def end_picture(self, poc, verify_counts=None):
        """After the picture is decided: Verifying pictures add their counters; the last one sets the switches."""
        r = poc % self.period
        if self.n_training <= r < self.n_training + self.n_verifying:
            if verify_counts is None:
                raise ValueError("a Verifying picture must report its counters")
            self.ver += np.asarray(verify_counts, np.float64).reshape(4, 6)
        if r == self.n_training + self.n_verifying - 1:
            sk, te = self._switch(self.ver, self.th_skip, self.th_term)
            self.sw_skip[:] = sk
            self.sw_term[:] = te


def read_yuv420(path, width, height, frame):
    """Frame `frame` of a planar 8-bit 4:2:0 file -> (Y, U, V) uint8 arrays; None past the end of the file."""
    ysz, csz = width * height, (width // 2) * (height // 2)
    with open(path, "rb") as f:
        f.seek(frame * (ysz + 2 * csz))
        buf = f.read(ysz + 2 * csz)
    if len(buf) < ysz + 2 * csz:
        return None
    a = np.frombuffer(buf, np.uint8)
    return (a[:ysz].reshape(height, width).copy(), a[ysz:ysz + csz].reshape(height // 2, width // 2).copy(),
            a[ysz + csz:].reshape(height // 2, width // 2).copy())


def write_yuv420(f, planes):
    """Appends one frame (Y, U, V uint8 arrays) to the binary file object `f`."""
    for p in planes:
        f.write(np.ascontiguousarray(p, np.uint8).tobytes())


def engine_maps_options(maps, default_fields, who, mv=False):
    """the maps= option of the drivers -> keyword arguments of CuEngine.decision_maps, or None"""
    if maps is None or maps is False:
        return None
    opt = {"fields": default_fields, "mv": mv, "labels": True}
    if maps is not True:
        if not isinstance(maps, dict) or set(maps) - {"fields", "mv", "labels"}:
            raise ValueError(who + ": maps is None, True or a dict with fields / mv / labels")
        opt.update(maps)
    return opt


def split_batch_maps(res, n):
    """the batch tensors of CuEngine.decision_maps -> one dict per picture (views)"""
    return [{k: ([t[i] for t in v] if isinstance(v, list) else v[i]) for k, v in res.items()} for i in range(n)]


class SequenceDecider:
    """All-intra sequence, picture by picture, on one GPU.  `fast=False` keeps every picture in the Training state
    (plain HM RDO); `fast=True` runs the fork's Training / Verifying / Testing cycle with its default (Naive) control."""

    def __init__(self, width, height, qp, slice_ctus=None, fast=True, deblock=True, device=0, schedule=None, in_flight=1, wpp=False, slice_rows=None, tiles=None, lf_cross_tiles=None, report=False, pic_hash=None, maps=None, lf_cross_slices=None, labels=None, cu_trace=False, features=None, risk=None, **flags):
        """cu_trace=True: every Training picture (all of them with fast=False) is decided with a CU trace bound to its chains
        (CuEngine.enable_cu_trace): its result dict gains `cu_trace`, the device tensor of n_ctu x 85 fcu_cu_trace records -- J0, J1 and
        the outcome of every CU the exhaustive search visited; CuEngine.trace_maps and CuEngine.label_score take it as it is.
        labels (with fast=True): a callable labels(poc, planes, obf) -> int8 device tensor [NL] or None -- a partition model of the
        caller's in the place of the Naive label.  It is asked for every Verifying and Testing picture with the picture's index, its
        source planes (Y, U, V device tensors) and its OBF map (device tensor); the label array it returns (the layout
        CuEngine.decision_maps writes; CuEngine.labels_from_rasters makes one from depth / part_size rasters) is bound to every
        chain of the picture (CuEngine.set_labels): counted on Verifying pictures -- the switches come from fcu_decision_switch on
        those counts exactly as for the Naive label --, pruning on Testing pictures.  None: the picture uses N_OBF as before.  The
        result dict of a picture that ran on labels carries them as `labels`.
        slice_ctus: CTUs per slice (HM's SliceMode 1 / SliceArgument).  None = one slice per picture, which is the
        reference's default (SliceMode 0, TAppEncCfg.cpp:838) and what `encoder_intra_main.cfg` encodes; a smaller value
        (e.g. the picture width in CTUs for one slice per CTU row) is a DIFFERENT encoder configuration -- the slices then
        run as concurrent chains, but every slice start cuts the intra neighbourhood and resets CABAC.
        wpp: WaveFrontSynchro=1 -- one slice per picture whose CTU rows run as chains, each row waiting for the row above
        (fcu_wpp_begin / fcu_compress_wpp); the pictures in flight go in one launch.
        slice_rows (with wpp only): WaveFrontSynchro together with SliceMode 1, SliceArgument = slice_rows x the picture width in
        CTUs -- independent slices of slice_rows whole CTU rows whose rows run as chains (fcu_wpp_begin_slices): the first row of
        a slice waits for nothing.
        lf_cross_slices (with slice_ctus or slice_rows only): LFCrossSliceBoundaryFlag of the deblocking, 0 or 1; None means 1,
        HM's default -- deblocking crosses the slice boundaries; 0 leaves them unfiltered (fcu_deblock_slices).
        tiles=(C, R): one slice per picture cut into C x R uniform tiles (HM's TileUniformSpacing) decided as chains
        (fcu_tiles_begin), with wpp=True WaveFrontSynchro inside every tile (fcu_wpp_begin_tiles).  lf_cross_tiles (with tiles
        only): LFCrossTileBoundaryFlag of the deblocking, 0 or 1 (fcu_deblock_tiles); None means 1, HM's default -- deblocking
        crosses the tile boundaries.  PictureLayout holds the rules of these combinations.  This driver runs no SAO: sao=True
        together with tiles is refused whatever lf_cross_tiles says.
        report=True: every result dict gains `report`, the picture report (CuEngine.report: SSD / PSNR per plane, bits, CU
        statistics) of the final planes, taken on the device in one batched call for the pictures of a group.
        pic_hash="md5", "crc" or "checksum": every result dict gains `hash`, HM's decoded-picture hash string of the final planes
        (CuEngine.picture_hash; what the encoder prints as [MD5:...] / [CRC:...] / [Checksum:...]), one batched call per group.
        maps=True, or a dict of CuEngine.decision_maps' keyword arguments (fields, mv, labels): every result dict gains `maps`, the
        picture's raster maps as device tensors -- by default the depth, part-size, prediction-mode and luma-mode maps and the four
        split-label maps; a picture that was decided with an OBF map (fast=True, outside Training) also gets `n_obf`.  They are
        formed after the launch, one batched call per group.
        features=True, or a tuple of feature-set names ("tmv", "soc"; True means both): every result dict gains `features`, the
        float32 device tensor [NL, F] of CuEngine.feature_maps -- the fork's TMV / SOC model inputs of every block, row for row
        aligned with the label / N_OBF maps and with CuEngine.trace_maps of `cu_trace` -- formed in one batched call per group from
        the source planes the chains were bound with.  With "soc" the OBF pre-pass runs for Training pictures too (it already runs
        for the others) to get the picture's thresholds; a Training chain is not given the map, so no decision changes.
        risk=True, or a dict with min_count (default 1) and / or key (with fast=True, not together with labels): the fork's schedule
        on the risk-table model (include/fcu.h), nothing leaving the device.  Every Training picture is decided with a CU trace
        bound (as cu_trace=True does) and gets its OBF pre-pass; after the launch of a Training group CuEngine.risk_train adds the
        group's traces to the model -- overwriting it at the first Training group of a period.  The keys are
        CuEngine.nobf_maps(obf), or key(poc, planes, obf, n_obf) -> uint16 device tensor [NL].  Every Verifying and Testing
        picture gets CuEngine.risk_predict on its own keys and the labels bound to all its chains: the Verifying counters,
        fcu_decision_switch and the per-depth switches work on them unchanged.  The result dicts of such pictures carry `labels`;
        `risk_model` is the model's device tensor (None before the first Training group).
        risk={"tree": {"levels": T, "sets": ("tmv", "soc"), "min_count": 1}} (not together with key): the keys are the leaves of a
        key tree over the binned feature maps (include/fcu.h).  The driver keeps the traces and features of the period's Training
        pictures; when the schedule leaves Training it forms the default edges (engine.feature_edges), the bins, the tree
        (CuEngine.tree_train), its keys and one CuEngine.risk_train over all of them; every Verifying / Testing picture gets
        feature_maps, feature_bins, tree_keys and risk_predict.  `key_tree` and `tree_edges` hold the tree and the edges."""
        if risk is None or risk is False:
            self.risk = None
        else:
            if risk is not True and (not isinstance(risk, dict) or set(risk) - {"min_count", "key", "tree"}):
                raise ValueError("SequenceDecider: risk is None, True or a dict with min_count / key / tree")
            self.risk = {"min_count": 1, "key": None, "tree": None}
            self.risk.update({} if risk is True else risk)
            if self.risk["tree"] is not None:
                tr = self.risk["tree"]
                if not isinstance(tr, dict) or "levels" not in tr or set(tr) - {"levels", "sets", "min_count"}:
                    raise ValueError("SequenceDecider: risk tree is a dict with levels and, optionally, sets / min_count")
                if self.risk["key"] is not None:
                    raise ValueError("SequenceDecider: risk tree and risk key both name the keys of the risk table; give one")
                tr = dict({"sets": ("tmv", "soc"), "min_count": 1}, **tr)
                for k in ("levels", "min_count"):
                    if not isinstance(tr[k], (int, np.integer)) or isinstance(tr[k], bool) or tr[k] < 0 or (k == "levels" and tr[k] > _engine.TREE_MAX_LEVELS):
                        raise ValueError("SequenceDecider: risk tree levels is 0 .. 5 and min_count a non-negative integer")
                try:
                    tr["sets"] = _engine.feature_sets(tr["sets"])[1]
                    if not tr["sets"]:
                        raise ValueError("no feature set")
                except ValueError as e:
                    raise ValueError("SequenceDecider: risk tree sets: %s" % e)
                self.risk["tree"] = tr
            mc = self.risk["min_count"]
            if not isinstance(mc, (int, np.integer)) or isinstance(mc, bool) or mc < 0:
                raise ValueError("SequenceDecider: risk min_count is a non-negative integer")
            if self.risk["key"] is not None and not callable(self.risk["key"]):
                raise ValueError("SequenceDecider: risk key is a callable key(poc, planes, obf, n_obf) -> uint16 device tensor [NL]")
            if not fast:
                raise ValueError("SequenceDecider: risk needs fast=True (the model is trained on the Training pictures of the schedule)")
            if labels is not None:
                raise ValueError("SequenceDecider: risk and labels both name the model of the Verifying / Testing pictures; give one")
        self.risk_model = None
        self.key_tree, self.tree_edges, self._tree_train = None, None, []      # risk tree: the tree, its edges, (trace, features) of the period's Training pictures
        self.do_report = report
        self.features = None if features is None or features is False else _engine.feature_sets(("tmv", "soc") if features is True else features)[1]
        if labels is not None and not callable(labels):
            raise ValueError("SequenceDecider: labels is a callable labels(poc, planes, obf) -> int8 device tensor [NL] or None")
        self.labels = labels
        self.cu_trace = bool(cu_trace) or self.risk is not None
        self.maps = engine_maps_options(maps, ("depth", "part_size", "pred_mode", "intra_dir_luma"), "SequenceDecider")
        if pic_hash is not None and pic_hash not in _engine.HASH_KINDS:
            raise ValueError("SequenceDecider: pic_hash is None, 'md5', 'crc' or 'checksum'")
        self.pic_hash = pic_hash
        sao = flags.get("sao")
        self.layout = lo = PictureLayout(width, height, slice_ctus, wpp, slice_rows, tiles, lf_cross_tiles, sao=sao, who="SequenceDecider", lf_cross_slices=lf_cross_slices)
        if sao and tiles is not None:
            raise ValueError("SequenceDecider: sao=True is not supported: this driver runs no SAO (LowDelayPDecider(tiles=..., sao=True, lf_cross_tiles=...) does)")
        self.tiles, self.lf_cross_tiles, self.wpp, self.slice_rows, self.slice_ctus = tiles, lo.lf_cross_tiles, wpp, slice_rows, lo.slice_ctus
        self.lf_cross_slices = lo.lf_cross_slices
        self.slice_mode, self.n_slices = lo.describe(), lo.chains      # n_slices: chains per picture (slices, rows or tile chains)
        self.width, self.height, self.qp, self.fast, self.do_deblock, self.flags = width, height, qp, fast, deblock, flags
        self.in_flight = max(1, in_flight)
        self.eng = _engine.CuEngine(width, height, max_chains=self.n_slices * self.in_flight, device=device)
        self.schedule = schedule or FastDecisionSchedule()
        self.poc = 0

    def decide(self, yuv):
        """Decides one picture.  Returns a dict: poc, state, switches, `out` (the fcu_ctu_out array as a uint8 device
        tensor), `rec` (device planes, deblocked when enabled), `depth` ([n_ctu, 256] numpy, z-order), verify counters."""
        return self.decide_group([yuv])[0]

    def group_size(self):
        """How many of the next pictures may be decided side by side: they share their state, and no switch that one
        of them reads is set by another (the switches change only after the last Verifying picture of a period)."""
        if not self.fast:
            return self.in_flight
        sc, r = self.schedule, self.poc % self.schedule.period
        end = sc.n_training if r < sc.n_training else (sc.n_training + sc.n_verifying if r < sc.n_training + sc.n_verifying else sc.period)
        return max(1, min(self.in_flight, end - r))

    def decide_group(self, yuvs):
        """Decides len(yuvs) <= group_size() consecutive pictures in one launch: picture i owns the chains
        [i * n_slices, (i + 1) * n_slices).  Returns one dict per picture (see decide)."""
        eng = self.eng
        assert 1 <= len(yuvs) <= self.group_size()
        pics = []
        for i, yuv in enumerate(yuvs):
            poc = self.poc + i
            state, sk, te = self.schedule.begin_picture(poc) if self.fast else (TRAINING, np.zeros(4, np.uint8), np.zeros(4, np.uint8))
            first = i * self.n_slices
            n_sl, rec, out = eng.init_picture(first, yuv, self.qp, self.layout, **self.flags)
            yc = None
            if state != TRAINING:
                obf, yc, _ = eng.obf_prepass(eng.org_planes(first)[0])
                obf = obf[0].contiguous()
                for k in range(n_sl):
                    eng.set_decision(first + k, state, obf, sk, te)
                lab = self.labels(poc, eng.org_planes(first), obf) if self.labels is not None else None
                if self.risk is not None:
                    if self._tree_train:                       # the schedule has left Training: edges, tree, keys, one risk_train
                        self._tree_fit()
                    if self.risk_model is None:
                        raise ValueError("SequenceDecider: risk has no model yet: the schedule needs at least one Training picture per period")
                    lab = eng.risk_predict(self._risk_keys(poc, first, obf, yc)[None], self.risk_model, self.risk["min_count"])[0]
                if lab is not None:                            # labels are per picture: every chain of it takes the one array
                    eng.set_labels(range(first, first + n_sl), lab)
            pics.append({"poc": poc, "state": state, "sw_skip": sk, "sw_term": te, "out": out, "rec": rec, "first": first})
            if self.cu_trace and state == TRAINING:            # one array per picture, shared by its chains; the result owns it
                tr = eng.enable_cu_trace(first)
                for k in range(1, n_sl):
                    eng.enable_cu_trace(first + k, tr)
                pics[-1]["cu_trace"] = tr
                if self.risk is not None and self.risk["tree"] is None:      # the keys of a Training picture: its own pre-pass; the chains are not given the map
                    pics[-1]["risk_keys"] = self._risk_keys(poc, first, eng.obf_prepass(eng.org_planes(first)[0])[0][0].contiguous())
            if state != TRAINING and lab is not None:
                pics[-1]["labels"] = lab
            if self.maps and state != TRAINING:
                pics[-1]["obf"] = obf
            if self.features and "soc" in self.features:       # the thresholds of the picture's own pre-pass; the map is not bound in Training
                pics[-1]["yc"] = yc[0] if yc is not None else eng.obf_prepass(eng.org_planes(first)[0])[1][0]
        eng.compress_pictures(0, len(yuvs), self.layout)
        nb = _engine.CTU_OUT_BYTES
        if self.risk is not None and self.risk["tree"] is not None and pics[0]["state"] == TRAINING:
            if pics[0]["poc"] % self.schedule.period == 0:     # a new period: its own tree and model
                self._tree_train = []
            for p in pics:                                     # kept until the schedule leaves Training (_tree_fit)
                self._tree_train.append((p["cu_trace"], self._tree_features(p["first"])[0].clone()))
        elif self.risk is not None and pics[0]["state"] == TRAINING:      # the pictures of a group share their state
            first_group = pics[0]["poc"] % self.schedule.period == 0
            self.risk_model, _ = eng.risk_train(pics, [p.pop("risk_keys") for p in pics], model=None if first_group else self.risk_model, accumulate=not first_group)
        for p in pics:
            p["verify"] = eng.verify_counts(p["first"], self.n_slices) if p["state"] == VERIFYING else None
            if self.fast:
                self.schedule.end_picture(p["poc"], p["verify"])
            if self.do_deblock:
                eng.deblock(p["first"], layout=self.layout)
        if self.do_report:                                   # on the final planes: after the deblocking when it is enabled
            for p, rep in zip(pics, eng.report([{"org": eng.org_planes(p["first"]), "rec": p["rec"], "out": p["out"]} for p in pics])):
                p["report"] = rep
        if self.pic_hash:                                    # on the final planes as well, nothing but the digests comes back
            for p, d in zip(pics, eng.picture_hash(pics, kinds=(self.pic_hash,))):
                p["hash"] = d["line"][self.pic_hash]
        if self.maps:                                        # the pictures of a group share their state: all of them have an OBF map or none
            obf = [p.pop("obf") for p in pics] if "obf" in pics[0] else None
            for p, m in zip(pics, split_batch_maps(eng.decision_maps(pics, obf=obf, **self.maps), len(pics))):
                p["maps"] = m
        if self.features:
            yc = np.stack([p.pop("yc") for p in pics]) if "soc" in self.features else None
            feat = eng.feature_maps([eng.org_planes(p["first"])[0] for p in pics], sets=self.features, yc=yc)
            for i, p in enumerate(pics):
                p["features"] = feat[i]
        eng.sync()
        for p in pics:
            p["depth"] = p["out"].view(eng.n_ctu, nb)[:, :256].cpu().numpy().copy()      # fcu_ctu_out.depth leads the struct
            p["tu_trials"] = sum(eng.debug_counters(p["first"] + k)[16] for k in range(self.n_slices))
        self.poc += len(yuvs)
        return pics

    def _tree_features(self, first, yc=None):
        """float32 [1, NL, F] of the picture bound to chain `first`, in the tree's feature sets (yc: its pre-pass thresholds, formed here when None)"""
        sets = self.risk["tree"]["sets"]
        if "soc" in sets and yc is None:
            yc = self.eng.obf_prepass(self.eng.org_planes(first)[0])[1]
        return self.eng.feature_maps([self.eng.org_planes(first)[0]], sets=sets, yc=yc[:1] if "soc" in sets else None)

    def _tree_fit(self):
        """what leaving Training does with risk tree: default edges from the Training pictures' features, their bins, the tree, its
        keys, and one risk_train over all of them"""
        eng, opt = self.eng, self.risk["tree"]
        traces = [t for t, _ in self._tree_train]
        X = self.eng.torch.stack([x for _, x in self._tree_train])
        self._tree_train = []
        self.tree_edges = _engine.feature_edges(X, self.width, self.height)
        bins = eng.feature_bins(X, self.tree_edges, sets=opt["sets"])
        self.key_tree = eng.tree_train(traces, bins, opt["levels"], opt["min_count"], sets=opt["sets"])
        self.risk_model, _ = eng.risk_train(traces, eng.tree_keys(bins, self.key_tree, sets=opt["sets"]))

    def _risk_keys(self, poc, first, obf, yc=None):
        """the uint16 [NL] key array of a picture: its N_OBF map, what the caller's key function makes of it, or the tree's keys"""
        if self.risk["tree"] is not None:
            sets = self.risk["tree"]["sets"]
            return self.eng.tree_keys(self.eng.feature_bins(self._tree_features(first, yc), self.tree_edges, sets=sets), self.key_tree, sets=sets)[0]
        n_obf = self.eng.nobf_maps(obf)[0]
        if self.risk["key"] is None:
            return n_obf
        k = self.risk["key"](poc, self.eng.org_planes(first), obf, n_obf)
        if not (k.is_cuda and k.dtype == n_obf.dtype and k.is_contiguous() and k.numel() == n_obf.numel()):
            raise ValueError("SequenceDecider: risk key returns a contiguous uint16 device tensor [NL]")
        return k

    def close(self):
        self.eng.destroy()
