"""Host-side driver of the RAU hot path: a thin object over the C ABI.

``RAU`` owns one ``rau_ctx`` (one GPU) and exposes the step the reference's
``feval`` performs (experiments/Ours_SS/LstmAttCtrlGradNoiseDontSelect.lua:428-596):
``set_batch`` (next_batch_feat + H2D, SS:434-439), ``forward`` (SS:443-520),
``backward(hop_w)`` (SS:561-596), ``update`` (SS:597-630 + adam, SS:770-772).
All arithmetic happens in librau.so; this file only moves pointers.
"""
from __future__ import annotations

import contextlib
import ctypes as C
import fnmatch
from dataclasses import dataclass

import numpy as np

from . import _lib as L
from . import feat16


@dataclass
class Config:
    """Network sizes; defaults are the reference's hard-coded locals (SS:202-229)."""
    B: int = 100            # the context's CAPACITY: RAU.set_batch_size(n <= B) runs smaller batches on it
    T: int = 26
    V: int = 14000
    E: int = 200
    Rq: int = 512
    D: int = 512
    S: int = 196
    M: int = 512
    A: int = 256
    R: int = 512
    K: int = 1000
    H: int = 8
    p_we: float = 0.5
    p_rnn: float = 0.5
    p_q: float = 0.5
    p_x: float = 0.5
    p_mf: float = 0.5
    device_id: int = 0
    dtype: str = "f32"      # "f32" | "bf16" (bf16-rounded operands in every conv and Linear GEMM) | "f32s" (convs: 3 x bf16 split)

    @property
    def Q(self) -> int:
        return 4 * self.Rq

    def mask_shapes(self, n=None, tied_x=False):
        """Shapes of the five mask sites at batch size n (default: the capacity B).  tied_x: the feature-map
        site of a context with RAU.tie_feature_dropout() on: one mask [B, D, S] shared by all hops."""
        B = self.B if n is None else int(n)
        return {"we": (self.T, B, self.E), "rnn": (self.T, B, self.Rq),
                "q": (self.H, B, self.Q),
                "x": (B, self.D, self.S) if tied_x else (self.H, B, self.D, self.S),
                "mf": (self.H, B, self.M)}


def regions_of(n_image, image_of):
    """Per-sample region counts of a batch that names its images by row: n_image [N] counts of the table's (or
    the bank rows') maps, image_of [B] 0-based rows -> int32 [B] = n_image[image_of], what set_regions takes."""
    n_image = np.ascontiguousarray(n_image, np.int32)
    image_of = np.ascontiguousarray(image_of, np.int64)
    if n_image.ndim != 1 or image_of.ndim != 1:
        raise ValueError("regions_of: n_image [N] and image_of [B] must be 1-d")
    if image_of.size and (image_of.min() < 0 or image_of.max() >= n_image.size):
        raise ValueError(f"regions_of: image_of out of [0, {n_image.size})")
    return np.ascontiguousarray(n_image[image_of], np.int32)


def check_att_bias(bias, n, S, regions=None):
    """The host-side check of an attention bias handed over as numpy (RAU.set_att_bias): bias [n,S] of float32,
    float16 or float64 with finite values and -inf only, and in every row at least one finite entry among the positions
    the sample attends to -- all S, or the first regions[b] (a softmax over nothing has no value).  Returns the bias as
    contiguous float32; raises ValueError, touching no device, otherwise."""
    b = np.asarray(bias)
    if b.dtype.kind != "f":
        raise ValueError(f"attention bias must be a floating-point array, got {b.dtype}")
    if b.shape != (int(n), int(S)):
        raise ValueError(f"attention bias has shape {b.shape}, expected {(int(n), int(S))}")
    if np.isnan(b).any():
        raise ValueError("attention bias holds NaN")
    if np.isposinf(b).any():
        raise ValueError("attention bias holds +inf (only finite values and -inf are allowed)")
    finite = np.isfinite(b)
    if regions is not None:
        r = np.asarray(regions)
        if r.shape != (int(n),) or r.min() < 1 or r.max() > int(S):
            raise ValueError(f"regions must be [{int(n)}] counts in [1, {int(S)}]")
        finite = finite & (np.arange(int(S))[None, :] < r[:, None])
    empty = np.flatnonzero(~finite.any(axis=1))
    if empty.size:
        where = "below their region count" if regions is not None else "at all"
        raise ValueError(f"attention bias rows {empty.tolist()} have no finite entry {where}: a softmax over nothing")
    return np.ascontiguousarray(b, np.float32)


def hop_weights(variant: str, H: int, epoch: int = 0):
    """Per-hop scale of the criterion gradient for the four training scripts.

    SS: x nHop (Ours_SS:569); MS: x1 (Ours_MS:568-570); Full / ResNet: x1 until
    ``epoch >= tab_multhop_stop_timing[h]``, then x0 (Ours_Full:414-426,587-589;
    Ours_ResNet:418-427).
    """
    if variant == "SS":
        return np.full(H, float(H), np.float32)
    if variant == "MS":
        return np.ones(H, np.float32)
    sched = {"Full": [1000, 35, 25, 20, 18, 16, 16, 16, 16, 1000],
             "ResNet": [1000, 30, 24, 20, 18, 16, 16, 15, 1000, 1000]}[variant]
    w = np.ones(H, np.float32)
    for h in range(H):
        stop = sched[h] if h < len(sched) else 1000
        if epoch >= stop:
            w[h] = 0.0
    return w


LAYER_DEFAULTS = (1.0, 1.0, 0.0)      # lr_scale, decay, bias_decay of rau_set_layer_opts


def layer_units(layouts):
    """{group: [(entry name, ...)]} as RAU.layout gives it -> [(layer name, group, index)]: unit i of a group is its
    entries 2i ("<name>.weight") and 2i + 1 ("<name>.bias"); word_embed has the weight only."""
    out = []
    for g in L.GROUPS:
        names = [e[0] for e in layouts[g]]
        for i in range(0, len(names), 2):
            pair = names[i:i + 2]
            base = pair[0][:-len(".weight")]
            if pair != [base + ".weight", base + ".bias"][:len(pair)]:
                raise ValueError(f"layout of {g}: {pair} is not a weight and its bias")
            out.append((base, g, i // 2))
    return out


def match_layers(name_or_glob, units):
    """The units a name or an fnmatch pattern addresses: an exact name first (also with the .weight / .bias of one
    of its entries), else every unit the pattern matches.  Nothing matched: KeyError."""
    key = str(name_or_glob)
    exact = {key} | {key[:-len(s)] for s in (".weight", ".bias") if key.endswith(s)}
    hit = [u for u in units if u[0] in exact] or [u for u in units if fnmatch.fnmatchcase(u[0], key)]
    if not hit:
        raise KeyError(f"no layer matches {key!r}; layers: {[u[0] for u in units]}")
    return hit


class RAU:
    def __init__(self, cfg: Config):
        self.cfg = cfg
        self._lib = L.lib()
        c = L.RauConfig(B=cfg.B, T=cfg.T, V=cfg.V, E=cfg.E, Rq=cfg.Rq, D=cfg.D, S=cfg.S,
                        M=cfg.M, A=cfg.A, R=cfg.R, K=cfg.K, H=cfg.H, p_we=cfg.p_we,
                        p_rnn=cfg.p_rnn, p_q=cfg.p_q, p_x=cfg.p_x, p_mf=cfg.p_mf,
                        dtype={"f32": 0, "bf16": 1, "f32s": 2}[cfg.dtype],
                        device_id=cfg.device_id)
        h = C.c_void_p()
        L.check(self._lib.rau_create(C.byref(c), C.byref(h)))
        self._h = h
        self._n = int(cfg.B)       # current batch size (rau_set_batch_size); cfg.B stays the capacity

    # ---- batch size: one context runs batches of up to cfg.B rows (rau_set_batch_size)
    @property
    def capacity(self) -> int:
        return int(self.cfg.B)

    @property
    def batch_size(self) -> int:
        """Rows of every batch and result tensor from now on (what set_batch_size last set)."""
        return self._n

    def set_batch_size(self, n: int):
        """The context now behaves, bit for bit, like one created with B = n holding the same parameters,
        gradients, optimizer state, dropout seed, mode and bank.  The resident batch, both upload slots,
        explicit masks and the last results do not outlive the call (n == batch_size: a no-op).  It drains
        the streams and clears the activation storage: per epoch, not per step."""
        n = int(n)
        if not 1 <= n <= self.capacity:
            raise ValueError(f"batch size {n} out of [1, {self.capacity}] (the B the context was created with)")
        L.check(self._lib.rau_set_batch_size(self._h, n))
        self._n = n

    def _rows(self, lens, what):
        """The batch size a batch's lens [n] asks for, checked against the capacity (no library call)."""
        if lens.ndim != 1 or lens.shape[0] < 1:
            raise ValueError(f"{what}: lens must be [n]")
        n = int(lens.shape[0])
        if n > self.capacity:
            raise ValueError(f"{what}: {n} rows exceed the context's capacity of {self.capacity}")
        return n

    def close(self):
        if getattr(self, "_h", None):
            self._lib.rau_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- parameters (m:getParameters(), SS:322-324)
    def group_size(self, group: str) -> int:
        n = C.c_size_t()
        L.check(self._lib.rau_params(self._h, L.GROUPS[group], None, None, C.byref(n)))
        return n.value

    def group_sizes(self):
        return {g: self.group_size(g) for g in L.GROUPS}

    def device_pointers(self, group: str):
        """(weights_ptr, grads_ptr, n): raw device addresses of the flat buffers."""
        w, g, n = C.c_void_p(), C.c_void_p(), C.c_size_t()
        L.check(self._lib.rau_params(self._h, L.GROUPS[group], C.byref(w), C.byref(g), C.byref(n)))
        return w.value, g.value, n.value

    def layout(self, group: str):
        out = []
        for i in range(self._lib.rau_layout_count(self._h, L.GROUPS[group])):
            name, off, r, c = C.c_char_p(), C.c_size_t(), C.c_int32(), C.c_int32()
            L.check(self._lib.rau_layout_entry(self._h, L.GROUPS[group], i, C.byref(name),
                                               C.byref(off), C.byref(r), C.byref(c)))
            out.append((name.value.decode(), off.value, r.value, c.value))
        return out

    def set_params(self, params):
        for g, a in params.items():
            a = np.ascontiguousarray(a, np.float32)
            L.check(self._lib.rau_set_params(self._h, L.GROUPS[g], a.ctypes.data, a.size))

    def _get(self, fn, group):
        a = np.empty(self.group_size(group), np.float32)
        L.check(fn(self._h, L.GROUPS[group], a.ctypes.data, a.size))
        return a

    def get_params(self):
        return {g: self._get(self._lib.rau_get_params, g) for g in L.GROUPS}

    def get_grads(self):
        return {g: self._get(self._lib.rau_get_grads, g) for g in L.GROUPS}

    def set_grads(self, grads):
        for g, a in grads.items():
            a = np.ascontiguousarray(a, np.float32)
            L.check(self._lib.rau_set_grads(self._h, L.GROUPS[g], a.ctypes.data, a.size))

    # ---- snapshots (torch.save / torch.load of SS:1188-1197, Eval.lua:113-114,344-347)
    def save_snapshot(self, path, it, epoch, opt, cuda=True, optim=False, ema=False):
        """optim=True adds the optimizer state (opt_state) as one more field, so a run resumed from the file goes
        on with its moments and step counts; ema=True adds the weight average (ema) as another, next to it.  A
        Torch7 reader of the reference ignores both fields.  While the weights are swapped with their average
        (ema_swap, averaged) `params` holds the averaged weights and `ema` the trained ones."""
        from . import t7
        self.sync()
        t7.save_snapshot(path, self.get_params(), it, epoch, opt, cuda=cuda,
                         optim=self.opt_state() if optim else None, ema=self.ema() if ema else None)

    def load_snapshot(self, path):
        """embed_param:copy(snap.params[1]) ...; returns (it, epoch, opt).  A snapshot that carries the optimizer
        state restores it as well, and so with the weight average; one without leaves the context's as it is."""
        from . import t7
        it, epoch, opt, params = t7.load_snapshot(path)
        ema = t7.load_ema(path)
        for g, a in params.items():
            if a.size != self.group_size(g):
                raise ValueError(f"snapshot group {g} has {a.size} floats, model has "
                                 f"{self.group_size(g)}")
        optim = t7.load_optim(path)
        self.set_params(params)
        if optim is not None:
            self.set_opt_state(*optim)
        if ema is not None:
            self.set_ema(ema)
        return it, epoch, opt

    def init_uniform(self, seed=123, lo=-0.08, hi=0.08):
        L.check(self._lib.rau_init_uniform(self._h, seed, lo, hi))

    def zero_grads(self):
        L.check(self._lib.rau_zero_grads(self._h))

    # ---- mode / dropout
    def training(self):
        L.check(self._lib.rau_set_mode(self._h, L.MODE_TRAIN))

    def evaluate(self):
        L.check(self._lib.rau_set_mode(self._h, L.MODE_EVAL))

    def set_dropout_seed(self, seed: int, step: int = 0):
        L.check(self._lib.rau_set_dropout_seed(self._h, seed, step))

    def tie_feature_dropout(self, on=True):
        """One feature-map dropout mask shared by all hops (rau_set_feat_dropout, RAU_XDROP_TIED) instead of
        the reference's mask per hop clone: a train-mode step then runs the two 1x1 convolutions and their three
        gradients once, not once per hop.  The "x" mask site becomes [B, D, S]; a seeded tied mask is hop 0's
        slice of the per-hop one.  Between steps, in either mode; a change drops an explicit "x" mask and the
        last forward."""
        L.check(self._lib.rau_set_feat_dropout(self._h, L.XDROP_TIED if on else L.XDROP_PER_HOP))

    @property
    def feature_dropout_tied(self) -> bool:
        k = C.c_int()
        L.check(self._lib.rau_feat_dropout(self._h, C.byref(k)))
        return k.value == L.XDROP_TIED

    def set_answer_loss(self, kind: str):
        """The answer criterion of forward() / graph_step() (rau_set_answer_loss): "ce", the reference's softmax
        cross-entropy (soft-target with an answer set), or "bce": one sigmoid per answer, binary cross-entropy
        against the labels' one-hot rows or the answer set's soft targets min(1, sum of the weights on an answer)
        -- predict.soft_bce / soft_bce_grad state it.  Losses are summed over the K answers.  Between steps, in
        either mode; a change drops the last forward.  A non-zero merge_w is refused under "bce"."""
        if kind not in L.LOSSES:
            raise ValueError(f"answer loss {kind!r}: 'ce' or 'bce'")
        L.check(self._lib.rau_set_answer_loss(self._h, L.LOSSES[kind]))

    @property
    def answer_loss(self) -> str:
        k = C.c_int()
        L.check(self._lib.rau_answer_loss(self._h, C.byref(k)))
        return "bce" if k.value == L.LOSS_BCE else "ce"

    def set_masks(self, masks):
        """masks: site name -> keep flags in Config.mask_shapes' shape for the current batch size (the library
        checks the element count).  With tie_feature_dropout() on, "x" is [B, D, S] or [1, B, D, S]: any other
        shape, the per-hop [H, B, D, S] of H > 1 among them, is refused."""
        for k, m in masks.items():
            m = np.ascontiguousarray(m, np.uint8)
            if k == "x" and self.feature_dropout_tied:
                want = self.cfg.mask_shapes(self._n, tied_x=True)["x"]
                if m.shape != want and m.shape != (1,) + want:
                    raise ValueError(f"mask site x is tied across the hops: {want}, got {m.shape}")
            L.check(self._lib.rau_set_mask(self._h, L.MASK_SITES[k], m.ctypes.data, m.size))

    def get_mask(self, site: str):
        shape = self.cfg.mask_shapes(self._n, tied_x=site == "x" and self.feature_dropout_tied)[site]
        m = np.empty(int(np.prod(shape)), np.uint8)
        L.check(self._lib.rau_get_mask(self._h, L.MASK_SITES[site], m.ctypes.data, m.size))
        return m.reshape(shape)

    # ---- batch + the hot path
    def _image_index(self, feats, image_of, rows):
        """(n_images, index array) of a batch of `rows` samples whose feats [N, D, ...] is an image table."""
        c = self.cfg
        image_of = np.ascontiguousarray(image_of, np.int32)
        n = int(feats.shape[0]) if feats.ndim >= 2 else 0
        if image_of.shape != (rows,) or n < 1 or feats.size != n * c.D * c.S:
            raise ValueError("image table shapes do not match the config")
        return n, image_of

    # ---- feature bank (rau_bank_*): every image's map once in device memory
    def bank_create(self, capacity, feat_type="f32"):
        """One bank of `capacity` maps [D, S] of feat_type per context."""
        L.check(self._lib.rau_bank_create(self._h, int(capacity), feat16.FEAT_TYPES[feat16.check_name(feat_type)]))

    def bank_destroy(self):
        L.check(self._lib.rau_bank_destroy(self._h))

    def bank_info(self):
        """{"capacity", "feat_type", "rows_filled"} of the context's bank."""
        cap, ft, n = C.c_int32(), C.c_int(), C.c_int32()
        L.check(self._lib.rau_bank_info(self._h, C.byref(cap), C.byref(ft), C.byref(n)))
        return {"capacity": cap.value, "feat_type": feat16.FEAT_NAMES[ft.value], "rows_filled": n.value}

    def bank_put(self, first, feats, feat_type=None):
        """feats [n, D, S] into rows first .. first+n-1.  Maps of the bank's type are copied; f32 maps
        into a 16-bit or fp8 bank are narrowed on the device (the bits feat16.store gives on the host; fp8:
        feat16.fp8_bits, round to nearest even, saturating at the largest finite value).  fp8 codes are
        uint8 arrays and need feat_type="e4m3" | "e5m2"."""
        c = self.cfg
        feats, ft = feat16.as_feats(feats, feat_type)
        n = feats.size // (c.D * c.S)
        if n < 1 or feats.size != n * c.D * c.S:
            raise ValueError("bank_put: feats is not [n, D, S]")
        L.check(self._lib.rau_bank_put(self._h, int(first), n, feats.ctypes.data, feat16.FEAT_TYPES[ft]))

    def bank_put_packed(self, first, rows, counts, feat_type=None):
        """Packed region rows [sum(counts), D] into bank rows first .. first+len(counts)-1: map i gets its
        counts[i] rows transposed and zero bits behind them (feat16.unpack_regions), on the device.  The type
        pairs of bank_put: rows of the bank's type are moved, f32 rows into a narrower bank are narrowed on the
        way with bank_put's bits.  The bank keeps dense maps and no counts: keep them (QuestionSet.img_regions)
        and pass regions= with the bank batch."""
        c = self.cfg
        counts = feat16.check_counts(counts, c.S)
        rows, ft = feat16.as_feats(rows, feat_type)
        if rows.ndim != 2 or rows.shape != (int(counts.sum()), c.D):
            raise ValueError(f"bank_put_packed: rows {rows.shape} is not [sum(counts)={int(counts.sum())}, D={c.D}]")
        L.check(self._lib.rau_bank_put_packed(self._h, int(first), int(counts.size), rows.ctypes.data,
                                              feat16.FEAT_TYPES[ft], counts.ctypes.data))

    def bank_get(self, first, count):
        """Rows first .. first+count-1 as [count, D, S] in the bank's element type (bf16: uint16 bits; fp8: uint8 codes)."""
        c = self.cfg
        out = np.empty((int(count), c.D, c.S), feat16.dtype_of(self.bank_info()["feat_type"]))
        L.check(self._lib.rau_bank_get(self._h, int(first), int(count), out.ctypes.data))
        return out

    def _bank_index(self, bank_rows, image_of, B):
        """(n_images, rows, image_of) of a bank batch of B samples; image_of None with B rows is the identity."""
        rows = np.ascontiguousarray(bank_rows, np.int32)
        if rows.ndim != 1 or rows.size < 1:
            raise ValueError("bank_rows must be a 1-d array of bank rows")
        if image_of is None:
            if rows.size != B:
                raise ValueError("bank_rows without image_of needs one row per sample")
            image_of = np.arange(B, dtype=np.int32)
        image_of = np.ascontiguousarray(image_of, np.int32)
        if image_of.shape != (B,):
            raise ValueError("image_of must have one entry per sample")
        return int(rows.size), rows, image_of

    # ---- answer sets: multi-answer ground truth (rau_set_answers)
    MAX_ANSWERS = 16

    def set_answers(self, ids, w, score=None, slot=None):
        """Give the batch in `slot` (None: the resident batch; 0 | 1: after set_batch_async(slot), before
        use_batch(slot)) an answer set in place of its labels: ids [n, G] int (1..K, 0 = empty entry), w [n, G]
        loss weights, score [n, G] metric scores (None: w), G <= 16.  The criterion head then computes
        sum_g w (lse - logit[y_g]) and its gradient, step_stats counts an answer as correct when it carries a
        positive score, and step_scores / predict_scores return the scores.  predict.soft_ce / answer_score /
        set_correct state the contract in numpy.  The set lasts until the next batch goes into that slot."""
        ids = np.ascontiguousarray(ids, np.int32)
        w = np.ascontiguousarray(w, np.float32)
        if ids.ndim != 2 or ids.shape[0] != self._n or w.shape != ids.shape:
            raise ValueError(f"answer set: ids and w must be [{self._n}, G]")
        if not 1 <= ids.shape[1] <= self.MAX_ANSWERS:
            raise ValueError(f"answer set: G={ids.shape[1]} out of [1, {self.MAX_ANSWERS}]")
        sp = None
        if score is not None:
            score = np.ascontiguousarray(score, np.float32)
            if score.shape != ids.shape:
                raise ValueError("answer set: score must have the shape of ids")
            sp = score.ctypes.data
        L.check(self._lib.rau_set_answers(self._h, -1 if slot is None else int(slot), int(ids.shape[1]),
                                          ids.ctypes.data, w.ctypes.data, sp))

    @property
    def batch_answers(self) -> int:
        """G of the resident batch's answer set, 0 when it has none."""
        g = C.c_int32()
        L.check(self._lib.rau_batch_answers(self._h, C.byref(g)))
        return int(g.value)

    # ---- region counts: attention over a sample's valid positions only (rau_set_regions)
    def set_regions(self, n, slot=None):
        """Give the batch in `slot` (None: the resident batch; 0 | 1: after set_batch_async(slot), before
        use_batch(slot)) per-sample region counts n [batch] int, 1 <= n[b] <= S: sample b attends to its first
        n[b] positions only, the others get attention and gradient exactly 0 in every hop (prefix-packed region
        features padded to S, padded grids).  Features at masked positions must be finite; zero is recommended.
        Always per sample: for an image table gather first (regions_of).  The counts last until the next batch
        goes into that slot."""
        n = np.ascontiguousarray(n, np.int32)
        if n.shape != (self._n,):
            raise ValueError(f"region counts must be [{self._n}], one per sample")
        L.check(self._lib.rau_set_regions(self._h, -1 if slot is None else int(slot), n.ctypes.data))

    def batch_regions(self) -> bool:
        """Whether the resident batch carries region counts."""
        v = C.c_int()
        L.check(self._lib.rau_batch_regions(self._h, C.byref(v)))
        return bool(v.value)

    @staticmethod
    def _sample_regions(regions, image_of, B):
        """regions= of set_batch / set_batch_async as per-sample counts: [B] as given, or, for a batch with an
        image table or bank rows, per-image [N] gathered through image_of (None: one image per sample)."""
        if image_of is not None:
            return regions_of(regions, image_of)
        regions = np.ascontiguousarray(regions, np.int32)
        if regions.shape != (B,):
            raise ValueError(f"region counts must be [{B}], one per sample")
        return regions

    # ---- per-sample loss weights: every training term of the step path (rau_set_sample_weights)
    @staticmethod
    def _sample_weights(s, B, normalize=False):
        """s as float32 [B], checked on the host: shape, finite, >= 0.  normalize: rescaled in float64 so that the
        weights sum to B (all-zero weights cannot be)."""
        s = np.asarray(s)
        if s.shape != (B,):
            raise ValueError(f"sample weights must be [{B}], one per sample")
        s64 = s.astype(np.float64)
        if not np.isfinite(s64).all() or (s64 < 0).any():
            raise ValueError("sample weights must be finite and >= 0")
        if normalize:
            tot = float(s64.sum())
            if not tot > 0.0:
                raise ValueError("sample weights that are all zero cannot be normalised")
            s64 = s64 * (B / tot)
        return np.ascontiguousarray(s64, np.float32)

    def set_sample_weights(self, s, slot=-1, normalize=False):
        """Give the batch in `slot` (-1 or None: the resident batch; 0 | 1: after set_batch_async(slot), before
        use_batch(slot)) per-sample loss weights s [batch] >= 0: every built-in mean (1/n) sum_b row_b of the step
        path -- the answer criterion, the selection BCE, the attention supervision, the merged rows -- becomes
        (1/n) sum_b s_b row_b (joint.weighted_mean), and losses(), loss_rows(), step_stats()' and att_stats()' losses
        follow; counts, metric scores and predictions stay unweighted.  The library never renormalises;
        normalize=True rescales here, in float64, so that the weights sum to n.  A forward that already ran must be
        run again.  The weights last until the next batch goes into that slot."""
        s = self._sample_weights(s, self._n, normalize)
        L.check(self._lib.rau_set_sample_weights(self._h, -1 if slot is None else int(slot), s.ctypes.data))

    def clear_sample_weights(self, slot=-1):
        """Detach the weights of the batch in `slot`: the next step is the unweighted one, bit for bit."""
        L.check(self._lib.rau_set_sample_weights(self._h, -1 if slot is None else int(slot), None))

    @property
    def batch_sample_weights(self) -> bool:
        """Whether the resident batch carries per-sample loss weights."""
        v = C.c_int()
        L.check(self._lib.rau_batch_sample_weights(self._h, C.byref(v)))
        return bool(v.value)

    # ---- multiple-choice candidates: the criterion restricted to them (rau_set_candidates)
    MAX_CANDIDATES = 32

    def _candidates(self, cand, B):
        """cand as int32 [B, C], checked on the host: shape, 1 <= C <= 32, ids in 0..K."""
        cand = np.ascontiguousarray(cand, np.int32)
        if cand.ndim != 2 or cand.shape[0] != B:
            raise ValueError(f"candidates must be [{B}, C], one list per sample")
        if not 1 <= cand.shape[1] <= self.MAX_CANDIDATES:
            raise ValueError(f"candidates: C={cand.shape[1]} out of [1, {self.MAX_CANDIDATES}]")
        if cand.min() < 0 or cand.max() > self.cfg.K:
            raise ValueError(f"candidates: an id outside [0, {self.cfg.K}] (0 = empty entry)")
        return cand

    def set_candidates(self, cand, slot=None):
        """Give the batch in `slot` (None: the resident batch; 0 | 1: after set_batch_async(slot), before
        use_batch(slot)) multiple-choice candidates cand [batch, C] int (1..K, 0 = empty entry; a duplicate counts
        once), C <= 32 -- VQA v1's 18 choices, Visual7W's four.  The criterion head is then normalised over a
        sample's candidates only (predict.cand_ce / cand_bce state it in numpy), losses() and loss_rows() are the
        restricted rows, cand_stats() and top_candidates() read the MC statistics and ranked MC answers; argmax(),
        step_stats()' counts, predict() and topk() stay open-ended.  A forward that already ran must be run again.
        The list lasts until the next batch goes into that slot."""
        cand = self._candidates(cand, self._n)
        L.check(self._lib.rau_set_candidates(self._h, -1 if slot is None else int(slot), int(cand.shape[1]),
                                             cand.ctypes.data))

    def clear_candidates(self, slot=None):
        """Detach the candidates of the batch in `slot`: the next step is the full-vocabulary one, bit for bit."""
        L.check(self._lib.rau_set_candidates(self._h, -1 if slot is None else int(slot), 0, None))

    @property
    def batch_candidates(self) -> int:
        """C of the resident batch's candidates, 0 when it has none."""
        v = C.c_int32()
        L.check(self._lib.rau_batch_candidates(self._h, C.byref(v)))
        return int(v.value)

    def cand_stats(self):
        """MC statistics of the last forward on a batch with candidates (feval rule, as step_stats), per row of
        {hops, uni, select}: ``loss`` [H+2] the restricted criterion (loss[:H] bitwise losses()), ``correct`` [H+2]
        the labelled rows whose best candidate is the label or carries a positive score, ``score`` [H+2] that
        candidate's summed metric score, and ``n_lab`` the labelled rows.  predict.cand_stats is the numpy
        restatement."""
        R = self.cfg.H + 2
        loss, score = np.empty(R, np.float32), np.empty(R, np.float32)
        correct, n = np.empty(R, np.int32), C.c_int32()
        L.check(self._lib.rau_cand_stats(self._h, loss.ctypes.data, correct.ctypes.data, score.ctypes.data, C.byref(n)))
        return {"loss": loss, "correct": correct, "score": score, "n_lab": int(n.value)}

    def top_candidates(self, k):
        """The k best candidates of every predict_result row of the last forward (hops, uni, select; last hop
        forced, as predict()): (ids int32, score f32, conf f32), each [H+2, B, k], best first; conf is the softmax
        over the row's live candidates; ranks behind their number are id 0, score -inf, conf 0.  Rank 0 is
        predict()'s ``mc`` whenever the best candidate's logit is positive.  predict.top_candidates is the numpy
        restatement."""
        shape = (self.cfg.H + 2, self._n, int(k))
        ids = np.empty(shape, np.int32)
        score = np.empty(shape, np.float32)
        conf = np.empty(shape, np.float32)
        L.check(self._lib.rau_topk_cand(self._h, int(k), ids.ctypes.data, score.ctypes.data, conf.ctypes.data))
        return ids, score, conf

    # ---- attention targets: supervise attprob on per-sample maps (rau_set_att_targets)
    def _att_targets(self, t, B):
        """t as float32 [B, S], checked on the host: shape, finite, >= 0."""
        t = np.ascontiguousarray(t, np.float32)
        if t.ndim < 2 or t.shape[0] != B or t.size != B * self.cfg.S:
            raise ValueError(f"attention targets must be [{B}, {self.cfg.S}], one map per sample")
        if not np.isfinite(t).all() or (t < 0).any():
            raise ValueError("attention targets must be finite and >= 0")
        return t.reshape(B, self.cfg.S)

    def set_att_targets(self, t, slot=None):
        """Give the batch in `slot` (None: the resident batch; 0 | 1: after set_batch_async(slot), before
        use_batch(slot)) per-sample attention targets t [batch, S] >= 0: backward(att_w=) / graph_step(att_w=) then
        add att_w[h] * ATT_h, ATT_h = mean_b sum_s t (-log(attprob_h + 1e-12)), to the objective (joint.att_ce).  Rows
        are not normalised here; a row of zeros is an unsupervised sample; with region counts, positions behind a
        count are ignored.  Always per sample, also for image-table and bank batches.  The forward does not read
        them: they may be set after it.  They last until the next batch goes into that slot."""
        t = self._att_targets(t, self._n)
        L.check(self._lib.rau_set_att_targets(self._h, -1 if slot is None else int(slot), t.ctypes.data))

    def batch_att_targets(self) -> bool:
        """Whether the resident batch carries attention targets."""
        v = C.c_int()
        L.check(self._lib.rau_batch_att_targets(self._h, C.byref(v)))
        return bool(v.value)

    def att_stats(self):
        """Of the last forward against its batch's attention targets: ``loss`` [H] (ATT_h), ``mass`` [H] (mean
        attention on the positions with t > 0, over the supervised rows), ``hits`` [H] (supervised rows whose
        first-max attention position has t > 0) and ``n_sup`` (supervised rows).  joint.att_stats is the numpy
        restatement."""
        H = self.cfg.H
        loss, mass = np.empty(H, np.float32), np.empty(H, np.float32)
        hits, n = np.empty(H, np.int32), C.c_int32()
        L.check(self._lib.rau_att_stats(self._h, loss.ctypes.data, mass.ctypes.data, hits.ctypes.data, C.byref(n)))
        return {"loss": loss, "mass": mass, "hits": hits, "n_sup": int(n.value)}

    def step_scores(self):
        """Metric score of every row's answer of the last forward (feval rule, as step_stats) against its
        batch's answer set: (per_sample [H+2, n], total [H+2]); rows = hops, uni, select."""
        H = self.cfg.H
        per = np.empty((H + 2, self._n), np.float32)
        tot = np.empty(H + 2, np.float32)
        L.check(self._lib.rau_step_scores(self._h, per.ctypes.data, tot.ctypes.data))
        return per, tot

    def predict_scores(self, mc=False):
        """Metric scores of the last predict()'s answers (last hop forced): (oe [H+2, n], mc [H+2, n] or None,
        totals [2, H+2]); mc=True asks for the MC rows (that predict() must have had an MC list: without one
        they and totals[1] are not written and come back as zeros)."""
        H = self.cfg.H
        oe = np.empty((H + 2, self._n), np.float32)
        mcs = np.zeros((H + 2, self._n), np.float32) if mc else None
        tot = np.zeros((2, H + 2), np.float32)
        L.check(self._lib.rau_predict_scores(self._h, oe.ctypes.data, None if mcs is None else mcs.ctypes.data,
                                             tot.ctypes.data))
        return oe, mcs, tot

    def set_batch(self, feats, tokens, lens, labels=None, feat_type=None, image_of=None, bank_rows=None,
                  answers=None, regions=None, att_targets=None, sample_w=None, candidates=None):
        """feat_type "f32" | "f16" | "bf16" | "e4m3" | "e5m2" (default: from the dtype, see feat16.infer;
        bf16 is uint16 bits, fp8 is uint8 codes, both must be named): a 16-bit or fp8 map gives the same
        results, bit for bit, as the f32 map of its widened values.
        image_of [B] (0-based rows): feats is an image TABLE [N, D, S] that the questions of one image
        share; the same results, bit for bit, as the plain batch feats[image_of].
        bank_rows [N] (feats None): the table is bank[bank_rows], gathered inside device memory.
        The batch size is lens.shape[0]: a batch of n <= capacity rows switches the context to n first
        (set_batch_size); every array must agree on n, checked before anything reaches the library.
        answers = (ids, w[, score]): set_answers on the batch once it is up.
        regions: set_regions on the batch once it is up; per sample [B], or with image_of / bank_rows per image
        [N] (gathered here: regions_of).
        att_targets [B, S]: set_att_targets on the batch once it is up; always per sample.
        sample_w [B]: set_sample_weights on the batch once it is up; always per sample.
        candidates [B, C]: set_candidates on the batch once it is up; always per sample."""
        if candidates is not None:   # checked before anything reaches the library
            candidates = self._candidates(candidates, int(np.asarray(lens).shape[0]))
        if regions is not None:
            regions = self._sample_regions(regions, image_of, int(np.asarray(lens).shape[0]))
        if att_targets is not None:
            att_targets = self._att_targets(att_targets, int(np.asarray(lens).shape[0]))
        if sample_w is not None:
            sample_w = self._sample_weights(sample_w, int(np.asarray(lens).shape[0]))
        self._set_batch(feats, tokens, lens, labels, feat_type, image_of, bank_rows)
        if answers is not None:
            self.set_answers(*answers)
        if regions is not None:
            self.set_regions(regions)
        if att_targets is not None:
            self.set_att_targets(att_targets)
        if sample_w is not None:
            self.set_sample_weights(sample_w)
        if candidates is not None:
            self.set_candidates(candidates)

    def _packed(self, rows, counts, image_of, B, feat_type):
        """(rows or None, feat type, n_maps, counts, image_of or None) of a packed batch of B samples, checked on
        the host: counts [n_maps] in 1..S, rows [sum(counts), D] (None: already in the slot's staging), n_maps == B
        unless image_of [B] names the maps."""
        c = self.cfg
        counts = feat16.check_counts(counts, c.S)
        if image_of is not None:
            image_of = np.ascontiguousarray(image_of, np.int32)
            if image_of.shape != (B,):
                raise ValueError("image_of must have one entry per sample")
        elif counts.size != B:
            raise ValueError(f"a packed batch without image_of needs one count per sample: {counts.size} != {B}")
        if rows is None:
            return None, feat16.check_name(feat_type or "f32"), int(counts.size), counts, image_of
        rows, ft = feat16.as_feats(rows, feat_type)
        if rows.ndim != 2 or rows.shape != (int(counts.sum()), c.D):
            raise ValueError(f"packed rows {rows.shape} are not [sum(counts)={int(counts.sum())}, D={c.D}]")
        return rows, ft, int(counts.size), counts, image_of

    def set_batch_packed(self, rows, counts, tokens, lens, labels=None, feat_type=None, image_of=None,
                         candidates=None):
        """A batch of region features as the files store them: rows [sum(counts), D], one row per box, map i
        owning counts[i] consecutive rows (1..S).  Only the rows cross the link; the device transposes and
        zero-pads them and the counts become the batch's region counts.  The same results, bit for bit, as
        set_batch(feat16.unpack_regions(rows, counts, S), ..., regions=counts).  image_of [B]: the maps are an
        image table of len(counts) maps (counts per IMAGE).  feat_type as in set_batch.  candidates [B, C]:
        set_candidates on the batch once it is up."""
        c = self.cfg
        lens = np.ascontiguousarray(lens, np.int32)
        B = self._rows(lens, "set_batch_packed")
        if candidates is not None:
            candidates = self._candidates(candidates, B)
        rows, ft, n_maps, counts, image_of = self._packed(rows, counts, image_of, B, feat_type)
        if rows is None:
            raise ValueError("set_batch_packed needs rows")
        tokens = np.ascontiguousarray(tokens, np.int32)
        if tokens.shape != (c.T, B):
            raise ValueError("batch shapes do not match the config")
        lp = None
        if labels is not None:
            labels = np.ascontiguousarray(labels, np.int32)
            if labels.shape != (B,):
                raise ValueError("labels shape")
            lp = labels.ctypes.data
        if B != self._n:
            self.set_batch_size(B)
        L.check(self._lib.rau_set_batch_packed(self._h, rows.ctypes.data, feat16.FEAT_TYPES[ft], n_maps,
                                               counts.ctypes.data, None if image_of is None else image_of.ctypes.data,
                                               tokens.ctypes.data, lens.ctypes.data, lp))
        if candidates is not None:
            self.set_candidates(candidates)

    def _set_batch(self, feats, tokens, lens, labels, feat_type, image_of, bank_rows):
        c = self.cfg
        lens = np.ascontiguousarray(lens, np.int32)
        B = self._rows(lens, "set_batch")
        if bank_rows is not None:
            if feats is not None:
                raise ValueError("a bank batch takes bank_rows, not feats")
            n_images, rows, image_of = self._bank_index(bank_rows, image_of, B)
            tokens = np.ascontiguousarray(tokens, np.int32)
            if tokens.shape != (c.T, B):
                raise ValueError("batch shapes do not match the config")
            lp = None
            if labels is not None:
                labels = np.ascontiguousarray(labels, np.int32)
                if labels.shape != (B,):
                    raise ValueError("labels shape")
                lp = labels.ctypes.data
            if B != self._n:
                self.set_batch_size(B)
            L.check(self._lib.rau_set_batch_bank(self._h, n_images, rows.ctypes.data, image_of.ctypes.data,
                                                 tokens.ctypes.data, lens.ctypes.data, lp))
            return
        feats, ft = feat16.as_feats(feats, feat_type)
        tokens = np.ascontiguousarray(tokens, np.int32)
        n_images = 0
        if image_of is not None:
            n_images, image_of = self._image_index(feats, image_of, B)
        elif feats.size != B * c.D * c.S:
            raise ValueError("batch shapes do not match the config")
        if tokens.shape != (c.T, B):
            raise ValueError("batch shapes do not match the config")
        lp = None
        if labels is not None:
            labels = np.ascontiguousarray(labels, np.int32)
            if labels.shape != (B,):
                raise ValueError("labels shape")
            lp = labels.ctypes.data
        if B != self._n:
            self.set_batch_size(B)
        if image_of is not None:
            L.check(self._lib.rau_set_batch_images(self._h, feats.ctypes.data, feat16.FEAT_TYPES[ft], n_images,
                                                   image_of.ctypes.data, tokens.ctypes.data, lens.ctypes.data,
                                                   lp))
            return
        L.check(self._lib.rau_set_batch_typed(self._h, feats.ctypes.data, feat16.FEAT_TYPES[ft],
                                              tokens.ctypes.data, lens.ctypes.data, lp))

    def batch_images(self) -> int:
        """0 for a plain resident batch, else the number of maps in its image table."""
        v = C.c_int()
        L.check(self._lib.rau_batch_images(self._h, C.byref(v)))
        return v.value

    def batch_feat_type(self) -> str:
        """Element type of the resident batch's feature map."""
        v = C.c_int()
        L.check(self._lib.rau_batch_feat_type(self._h, C.byref(v)))
        return feat16.FEAT_NAMES[v.value]

    # asynchronous, double-buffered upload (rau_batch_slot / rau_set_batch_async / rau_use_batch)
    def batch_slot(self, slot, feat_type="f32"):
        """numpy views of slot's PINNED staging: {feats [n,D,S], tokens [T,n], lens [n], labels [n]},
        n = the current batch_size (each array starts where the capacity puts it and is dense in n).
        A loader fills them in place; set_batch_async(slot) then uploads without a host copy.
        feats is a view of the staging's start in feat_type's dtype (bf16: uint16 bit patterns; fp8: uint8
        codes, the first quarter of the staging);
        upload it with set_batch_async(slot, feat_type=<the same>)."""
        c, B = self.cfg, self._n
        fdt = feat16.dtype_of(feat_type)
        p = [C.c_void_p() for _ in range(4)]
        L.check(self._lib.rau_batch_slot(self._h, slot, *[C.byref(x) for x in p]))

        def view(ptr, n, ct, dt, shape):
            return np.frombuffer((ct * n).from_address(ptr.value), dtype=dt).reshape(shape)
        return {"feats": view(p[0], B * c.D * c.S, C.c_uint8 * fdt.itemsize, fdt, (B, c.D, c.S)),
                "tokens": view(p[1], c.T * B, C.c_int32, np.int32, (c.T, B)),
                "lens": view(p[2], B, C.c_int32, np.int32, (B,)),
                "labels": view(p[3], B, C.c_int32, np.int32, (B,))}

    def set_batch_async(self, slot, feats=None, tokens=None, lens=None, labels=None, has_labels=True,
                        feat_type=None, image_of=None, n_images=None, bank_rows=None, answers=None,
                        regions=None, att_targets=None, packed_counts=None, sample_w=None, candidates=None):
        """Enqueue the upload of a batch into `slot` on the copy stream and return.  Arrays left None
        are taken from the slot's staging (filled in place through batch_slot).  feat_type: as in
        set_batch; with feats None it names what the staging holds (default "f32").
        image_of [B]: the batch carries an image table (see set_batch) of feats.shape[0] maps, or, with
        feats None, of the n_images maps at the start of the slot's staging; only those are uploaded.
        bank_rows [N] (feats None): the table is bank[bank_rows]; the slot's feature staging is not read.
        The batch size is lens.shape[0] when lens is given (the context is switched to it first, which
        drops both slots' earlier uploads), else the current batch_size.
        answers = (ids, w[, score]): set_answers(slot=slot) behind the upload, on the copy stream.
        regions: set_regions(slot=slot) behind the upload; per sample, or per image as in set_batch.
        att_targets [B, S]: set_att_targets(slot=slot) behind the upload.
        packed_counts [N]: feats is packed region rows [sum(packed_counts), D] (see set_batch_packed), or, with
        feats None, the slot's staging holds them at its start (batch_slot(...)["feats"] viewed flat); N is the
        batch size, or with image_of the number of maps.  The counts become the batch's region counts.
        sample_w [B]: set_sample_weights(slot=slot) behind the upload.
        candidates [B, C]: set_candidates(slot=slot) behind the upload."""
        if candidates is not None:
            candidates = self._candidates(candidates, self._n if lens is None else int(np.asarray(lens).shape[0]))
        if packed_counts is not None and (regions is not None or bank_rows is not None):
            raise ValueError("a packed batch brings its own region counts and its own rows")
        if regions is not None:
            B = self._n if lens is None else int(np.asarray(lens).shape[0])
            regions = self._sample_regions(regions, image_of, B)
        if att_targets is not None:
            att_targets = self._att_targets(att_targets, self._n if lens is None else int(np.asarray(lens).shape[0]))
        if sample_w is not None:
            sample_w = self._sample_weights(sample_w, self._n if lens is None else int(np.asarray(lens).shape[0]))
        self._set_batch_async(slot, feats, tokens, lens, labels, has_labels, feat_type, image_of, n_images,
                              bank_rows, packed_counts)
        if answers is not None:
            self.set_answers(*answers, slot=slot)
        if regions is not None:
            self.set_regions(regions, slot=slot)
        if att_targets is not None:
            self.set_att_targets(att_targets, slot=slot)
        if sample_w is not None:
            self.set_sample_weights(sample_w, slot=slot)
        if candidates is not None:
            self.set_candidates(candidates, slot=slot)

    def _set_batch_async(self, slot, feats, tokens, lens, labels, has_labels, feat_type, image_of, n_images,
                         bank_rows, packed_counts=None):
        c = self.cfg
        B = self._n
        if lens is not None:
            lens = np.ascontiguousarray(lens, np.int32)
            B = self._rows(lens, "set_batch_async")
        if packed_counts is not None:
            rows, ft, nmaps, counts, image_of = self._packed(feats, packed_counts, image_of, B, feat_type)
            keep = [None if a is None else np.ascontiguousarray(a, np.int32) for a in (tokens, lens, labels)]
            for a, n in zip(keep, (c.T * B, B, B)):
                if a is not None and a.size != n:
                    raise ValueError("batch shapes do not match the config")
            if B != self._n:
                self.set_batch_size(B)
            tp, lp, yp = [None if a is None else a.ctypes.data for a in keep]
            L.check(self._lib.rau_set_batch_async_packed(
                self._h, slot, None if rows is None else rows.ctypes.data, feat16.FEAT_TYPES[ft], nmaps,
                counts.ctypes.data, None if image_of is None else image_of.ctypes.data, tp, lp, yp,
                int(bool(has_labels))))
            return
        if bank_rows is not None:
            if feats is not None:
                raise ValueError("a bank batch takes bank_rows, not feats")
            nmaps, rows, image_of = self._bank_index(bank_rows, image_of, B)
            keep = [None if a is None else np.ascontiguousarray(a, np.int32) for a in (tokens, lens, labels)]
            for a, n in zip(keep, (c.T * B, B, B)):
                if a is not None and a.size != n:
                    raise ValueError("batch shapes do not match the config")
            if B != self._n:
                self.set_batch_size(B)
            tp, lp, yp = [None if a is None else a.ctypes.data for a in keep]
            L.check(self._lib.rau_set_batch_async_bank(self._h, slot, nmaps, rows.ctypes.data,
                                                       image_of.ctypes.data, tp, lp, yp, int(bool(has_labels))))
            return
        nmaps = B
        if image_of is not None:
            if feats is None:
                image_of = np.ascontiguousarray(image_of, np.int32)
                if image_of.shape != (B,) or n_images is None:
                    raise ValueError("an in-place image table needs image_of [B] and n_images")
                nmaps = int(n_images)
            else:
                nmaps, image_of = self._image_index(np.asarray(feats), image_of, B)
        if feats is None:
            ft = feat16.check_name(feat_type or "f32")
        else:
            feats, ft = feat16.as_feats(feats, feat_type)

        def ptr(a, dt, n):
            if a is None:
                return None, None
            a = np.ascontiguousarray(a, dt)
            if a.size != n:
                raise ValueError("batch shapes do not match the config")
            return a.ctypes.data, a
        fp, fk = ptr(feats, feat16.dtype_of(ft), nmaps * c.D * c.S)
        tp, tk = ptr(tokens, np.int32, c.T * B)
        lp, lk = ptr(lens, np.int32, B)
        yp, yk = ptr(labels, np.int32, B)
        if B != self._n:
            self.set_batch_size(B)
        if image_of is not None:
            L.check(self._lib.rau_set_batch_async_images(self._h, slot, fp, feat16.FEAT_TYPES[ft], nmaps,
                                                         image_of.ctypes.data, tp, lp, yp,
                                                         int(bool(has_labels))))
            return
        L.check(self._lib.rau_set_batch_async_typed(self._h, slot, fp, feat16.FEAT_TYPES[ft], tp, lp, yp,
                                                    int(bool(has_labels))))

    def use_batch(self, slot):
        L.check(self._lib.rau_use_batch(self._h, slot))

    def forward(self):
        L.check(self._lib.rau_forward(self._h))

    def _hop_array(self, w, what):
        w = np.ascontiguousarray(w, np.float32)
        if w.shape != (self.cfg.H,):
            raise ValueError(f"{what} must have H entries")
        return w

    def _merge_array(self, w):
        w = np.ascontiguousarray(w, np.float32)
        if w.shape != (2,):
            raise ValueError("merge_w must have 2 entries: uni, select")
        return w

    def _loss_args(self, hop_w, select_w, att_w, merge_w):
        """The entry-point family that takes these loss terms ("", "_select", "_att" or "_merged": the last term
        given decides) and its weight arguments: pointers that keep their arrays alive, None for a term left out."""
        arrs = [self._hop_array(hop_w, "hop_w"),
                None if select_w is None else self._hop_array(select_w, "select_w"),
                None if att_w is None else self._hop_array(att_w, "att_w"),
                None if merge_w is None else self._merge_array(merge_w)]
        n = max(i for i, a in enumerate(arrs) if a is not None)
        return (("", "_select", "_att", "_merged")[n],
                [None if a is None else a.ctypes.data_as(C.c_void_p) for a in arrs[:n + 1]])

    def _out_grad(self, out_grads, key, shape, what="out_grads"):
        """Device address of out_grads[key] (a contiguous float32 CUDA torch tensor of `shape`), None when absent."""
        t = out_grads.get(key)
        if t is None:
            return None
        import torch
        if not (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.float32 and t.is_contiguous()):
            raise ValueError(f"{what}[{key!r}] must be a contiguous float32 CUDA torch tensor")
        if t.device.index != self.cfg.device_id:
            raise ValueError(f"{what}[{key!r}] is on {t.device}, the context on cuda:{self.cfg.device_id}")
        if tuple(t.shape) != shape:
            raise ValueError(f"{what}[{key!r}] has shape {tuple(t.shape)}, expected {shape}")
        return t.data_ptr()

    def backward(self, hop_w=None, select_w=None, att_w=None, merge_w=None, out_grads=None, state_grads=None):
        """select_w [H]: per-hop weight of the step-selection head's BCE gradient, the multiplier the
        reference fixes at 0 (SS:566); None is that zero (rau_backward).
        att_w [H]: per-hop weight of the attention supervision against the batch's targets (set_att_targets), where
        the reference passes gradattprob = zeros (SS:361, 573); None is those zeros.
        merge_w [2]: weights of the cross-entropies of the merged "uni" and "select" rows (step_stats' loss[H] and
        loss[H+1], which the reference only logs); None is no such term.
        out_grads: a dict with any of "logits" [H,n,K], "dopred" [H,n], "attprob" [H,n,S] -- the gradients of a
        term of the caller's own at those outputs (output_tensors), contiguous float32 CUDA torch tensors that the
        ctx's stream may read (order it behind the stream that wrote them).  The call then goes through
        rau_backward_ext, where hop_w may be None (zeros); without out_grads it is exactly what it was.
        state_grads: a dict with any of "h" [H,n,R] (the gradient at h' of every hop, state_tensors()) and "c_last"
        [n,R] (at c' of the last hop), tensors like those of out_grads.  The call then goes through
        rau_backward_state; hop_w may be None again."""
        if state_grads is not None:
            unknown = set(state_grads) - {"h", "c_last"}
            if unknown:
                raise ValueError(f"state_grads has unknown keys {sorted(unknown)}")
            if state_grads.get("h") is None and state_grads.get("c_last") is None:
                state_grads = None
        if state_grads is not None and out_grads is None:
            out_grads = {}
        if out_grads is None:
            if hop_w is None:
                raise ValueError("hop_w is required without out_grads")
            family, ws = self._loss_args(hop_w, select_w, att_w, merge_w)
            L.check(getattr(self._lib, "rau_backward" + family)(self._h, *ws))
            return
        unknown = set(out_grads) - {"logits", "dopred", "attprob"}
        if unknown:
            raise ValueError(f"out_grads has unknown keys {sorted(unknown)}")
        H, n = self.cfg.H, self._n
        g = L.RauOutGrads(self._out_grad(out_grads, "logits", (H, n, self.cfg.K)),
                          self._out_grad(out_grads, "dopred", (H, n)),
                          self._out_grad(out_grads, "attprob", (H, n, self.cfg.S)))
        arrs = [None if hop_w is None else self._hop_array(hop_w, "hop_w"),
                None if select_w is None else self._hop_array(select_w, "select_w"),
                None if att_w is None else self._hop_array(att_w, "att_w"),
                None if merge_w is None else self._merge_array(merge_w)]
        ws = [None if a is None else a.ctypes.data_as(C.c_void_p) for a in arrs]
        if state_grads is None:
            L.check(self._lib.rau_backward_ext(self._h, *ws, C.byref(g)))
            return
        R = self.cfg.R
        sg = L.RauStateGrads(self._out_grad(state_grads, "h", (H, n, R), "state_grads"),
                             self._out_grad(state_grads, "c_last", (n, R), "state_grads"))
        L.check(self._lib.rau_backward_state(self._h, *ws, C.byref(g), C.byref(sg)))

    def output_tensors(self):
        """Zero-copy torch views of the last step-level forward's outputs in device memory (rau_outputs_dev):
        logits [H,n,K], dopred [H,n], attprob [H,n,S] -- the last a strided view of the pitched buffer, and so are the
        logits where K % 4 != 0 (logits_pitch).  Valid until the next forward or set_batch_size, ordered on the ctx's
        stream (stream()), read-only."""
        from .dist import device_view
        lg, dp, at = C.c_void_p(), C.c_void_p(), C.c_void_p()
        pitch = C.c_int32()
        L.check(self._lib.rau_outputs_dev(self._h, C.byref(lg), C.byref(dp), C.byref(at), C.byref(pitch)))
        H, n, K, S, dev = self.cfg.H, self._n, self.cfg.K, self.cfg.S, self.cfg.device_id
        kp = self.logits_pitch
        return (device_view(lg.value, H * n * kp, dev).view(H, n, kp)[:, :, :K],
                device_view(dp.value, H * n, dev).view(H, n),
                device_view(at.value, H * n * pitch.value, dev).view(H, n, pitch.value)[:, :, :S])

    @property
    def logits_pitch(self) -> int:
        """Row pitch of the logits in device memory (rau_logits_pitch): K where K % 4 == 0, else K rounded up to a
        multiple of 4 with +0 in columns K..pitch-1.  output_tensors() hides it; out_grads stay dense [H,n,K]."""
        pitch = C.c_int32()
        L.check(self._lib.rau_logits_pitch(self._h, C.byref(pitch)))
        return int(pitch.value)

    def want_feature_grad(self, on=True, per_image=False):
        """Every step-level backward (backward, graph_step) also leaves the gradient at the feature map behind
        (rau_set_feat_grad): feature_grad() / feature_grad_tensor().  Off (the default) the step is what it was.
        per_image=False (RAU_FEAT_GRAD_SAMPLES): batches with one map per sample only; the backward of an
        image-table or bank batch raises.  per_image=True (RAU_FEAT_GRAD_IMAGES): the backward of an image-table
        batch leaves the gradient at the TABLE, [N,D,S] -- each image's samples summed in ascending order, no
        atomics, an unnamed image exactly zero; every other batch as with per_image=False; bank batches still raise."""
        mode = L.FEAT_GRAD_OFF if not on else L.FEAT_GRAD_IMAGES if per_image else L.FEAT_GRAD_SAMPLES
        L.check(self._lib.rau_set_feat_grad(self._h, mode))

    @property
    def feature_grad_wanted(self) -> bool:
        return self.feature_grad_mode != L.FEAT_GRAD_OFF

    @property
    def feature_grad_mode(self) -> int:
        """0 = off, 1 = per sample, 2 = per image where the batch has an image table (rau_feat_grad)."""
        on = C.c_int(0)
        L.check(self._lib.rau_feat_grad(self._h, C.byref(on)))
        return int(on.value)

    def feature_grad_rows(self) -> int:
        """The map count of the last backward's feature-map gradient (rau_feat_grad_rows): the batch size n, or the
        table's N where it was formed per image."""
        rows = C.c_int32(0)
        L.check(self._lib.rau_feat_grad_rows(self._h, C.byref(rows)))
        return int(rows.value)

    def feature_grad(self):
        """The last backward's feature-map gradient [rows,D,S] (numpy; synchronises); rows = feature_grad_rows()."""
        out = np.empty((self.feature_grad_rows(), self.cfg.D, self.cfg.S), np.float32)
        L.check(self._lib.rau_get_feat_grad(self._h, out.ctypes.data))
        return out

    def feature_grad_tensor(self):
        """Zero-copy torch view [rows,D,S] of the last backward's feature-map gradient in device memory
        (rau_feat_grad_dev) -- strided where the maps are pitched (S % 4 != 0).  Valid until the next forward or
        set_batch_size, ordered on the ctx's stream (stream()), read-only."""
        from .dist import device_view
        p, pitch = C.c_void_p(), C.c_int32()
        L.check(self._lib.rau_feat_grad_dev(self._h, C.byref(p), C.byref(pitch)))
        n, D, S, dev = self.feature_grad_rows(), self.cfg.D, self.cfg.S, self.cfg.device_id
        return device_view(p.value, n * D * pitch.value, dev).view(n, D, pitch.value)[:, :, :S]

    # ---- per-position L2 normalisation of the batch's maps (rau_set_feat_norm)
    def normalize_features(self, on=True, eps=1e-12):
        """Every step-level forward first L2-normalises each position's channel vector of the batch's maps on the
        device, x / max(||x||_2, eps) over D in float32 (torch.nn.functional.normalize(x, dim=1, eps=eps) on
        [n,D,S]) -- whatever type the maps are stored in -- and runs on the result as on a float32 batch; with
        want_feature_grad the gradient goes back through the normalisation to the raw maps.  Off (the default) the
        step is what it was.  A change drops the last forward."""
        L.check(self._lib.rau_set_feat_norm(self._h, L.XNORM_L2 if on else L.XNORM_NONE, float(eps)))

    @property
    def features_normalized(self):
        """(kind, eps) of rau_feat_norm: kind 0 = off, 1 = L2."""
        kind, eps = C.c_int(0), C.c_float(0.0)
        L.check(self._lib.rau_feat_norm(self._h, C.byref(kind), C.byref(eps)))
        return int(kind.value), float(eps.value)

    def _norm_feats_dev(self):
        xn, nrm, pitch, rows = C.c_void_p(), C.c_void_p(), C.c_int32(), C.c_int32()
        L.check(self._lib.rau_norm_feats_dev(self._h, C.byref(xn), C.byref(nrm), C.byref(pitch), C.byref(rows)))
        return xn.value, nrm.value, int(pitch.value), int(rows.value)

    def norm_feats(self):
        """The last forward's normalised maps and their norms, (xn [rows,D,S], nrm [rows,S]) (numpy; synchronises):
        rows = N after the evaluate-mode forward of an image-table or bank batch, else n."""
        rows = self._norm_feats_dev()[3]
        xn = np.empty((rows, self.cfg.D, self.cfg.S), np.float32)
        nrm = np.empty((rows, self.cfg.S), np.float32)
        L.check(self._lib.rau_get_norm_feats(self._h, xn.ctypes.data, nrm.ctypes.data))
        return xn, nrm

    def norm_feats_tensors(self):
        """Zero-copy torch views (xn [rows,D,S], nrm [rows,S]) of the same in device memory (rau_norm_feats_dev) --
        strided where the maps are pitched (S % 4 != 0).  Valid until the next forward or set_batch_size, ordered on
        the ctx's stream (stream()), read-only."""
        from .dist import device_view
        xn, nrm, pitch, rows = self._norm_feats_dev()
        D, S, dev = self.cfg.D, self.cfg.S, self.cfg.device_id
        return (device_view(xn, rows * D * pitch, dev).view(rows, D, pitch)[:, :, :S],
                device_view(nrm, rows * pitch, dev).view(rows, pitch)[:, :S])

    def _dev_maps(self, t, what, shape=None):
        import torch
        if not (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.float32 and t.is_contiguous()):
            raise ValueError(f"{what} must be a contiguous float32 CUDA torch tensor")
        if t.device.index != self.cfg.device_id:
            raise ValueError(f"{what} is on {t.device}, the context on cuda:{self.cfg.device_id}")
        want = shape if shape is not None else (int(t.shape[0]) if t.dim() else 0, self.cfg.D, self.cfg.S)
        if tuple(t.shape) != tuple(want):
            raise ValueError(f"{what} has shape {tuple(t.shape)}, expected {tuple(want)}")
        return t

    def l2norm(self, x, eps=1e-12, out=None):
        """rau_dev_l2norm on a contiguous float32 CUDA tensor x [n,D,S] (any n): returns (y, nrm), new tensors, or
        y written into `out` (which may be x).  On the ctx's stream, no synchronisation: order it behind the stream
        that wrote x, as for set_batch_dev."""
        import torch
        x = self._dev_maps(x, "x")
        y = torch.empty_like(x) if out is None else self._dev_maps(out, "out", x.shape)
        nrm = torch.empty((x.shape[0], self.cfg.S), dtype=torch.float32, device=x.device)
        L.check(self._lib.rau_dev_l2norm(self._h, x.data_ptr(), int(x.shape[0]), float(eps), y.data_ptr(),
                                         nrm.data_ptr()))
        return y, nrm

    def l2norm_backward(self, y, nrm, g, eps=1e-12, out=None):
        """rau_dev_l2norm_backward: the gradient at x for the gradient g [n,D,S] at y = l2norm(x), from that call's
        y and nrm; a new tensor, or written into `out` (which may be g).  Same stream rule as l2norm."""
        import torch
        y = self._dev_maps(y, "y")
        g = self._dev_maps(g, "g", y.shape)
        nrm = self._dev_maps(nrm, "nrm", (y.shape[0], self.cfg.S))
        dx = torch.empty_like(g) if out is None else self._dev_maps(out, "out", y.shape)
        L.check(self._lib.rau_dev_l2norm_backward(self._h, y.data_ptr(), nrm.data_ptr(), float(eps), g.data_ptr(),
                                                  int(y.shape[0]), dx.data_ptr()))
        return dx

    # ---- question state from the caller (rau_set_question_dev): another question encoder in front of the step path
    def set_question(self, q_cuda):
        """Attach the question state q [n,Q] (Q = 4 Rq) to the resident batch: a contiguous CUDA torch tensor of
        float32, float16 or bfloat16 on the ctx's device -- the type is taken from the dtype, 16-bit values are
        widened exactly.  One copy on the ctx's stream, no host synchronisation: order the ctx's stream behind the
        stream that wrote the tensor and keep it unchanged until the copy has run (set_batch_dev's rule).  While it
        is attached forward / graph_step read it in place of the built-in encoder's output and launch nothing of the
        encoder; the backward leaves question_grad() behind and does not touch the embed and rnn gradients.  The
        next set_batch* / use_batch / set_batch_size detaches it; attaching again replaces the contents."""
        import torch
        t = q_cuda
        types = {torch.float32: "f32", torch.float16: "f16", torch.bfloat16: "bf16"}
        if not (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype in types and t.is_contiguous()):
            raise ValueError("q_cuda must be a contiguous float32, float16 or bfloat16 CUDA torch tensor")
        if t.device.index != self.cfg.device_id:
            raise ValueError(f"q_cuda is on {t.device}, the context on cuda:{self.cfg.device_id}")
        if tuple(t.shape) != (self._n, self.cfg.Q):
            raise ValueError(f"q_cuda has shape {tuple(t.shape)}, expected {(self._n, self.cfg.Q)}")
        L.check(self._lib.rau_set_question_dev(self._h, t.data_ptr(), feat16.FEAT_TYPES[types[t.dtype]]))

    def clear_question(self):
        """Detach the question: the resident batch is the built-in encoder's again."""
        L.check(self._lib.rau_set_question_dev(self._h, None, 0))

    @property
    def batch_question(self) -> bool:
        """The resident batch has a question attached (rau_batch_question)."""
        has = C.c_int(0)
        L.check(self._lib.rau_batch_question(self._h, C.byref(has)))
        return bool(has.value)

    def question_grad(self):
        """The last backward's gradient at the attached question [n,Q] (numpy; synchronises)."""
        out = np.empty((self._n, self.cfg.Q), np.float32)
        L.check(self._lib.rau_get_question_grad(self._h, out.ctypes.data))
        return out

    def question_grad_tensor(self):
        """Zero-copy torch view [n,Q] of the last backward's gradient at the attached question in device memory
        (rau_question_grad_dev).  Valid until the next forward or set_batch_size, ordered on the ctx's stream
        (stream()), read-only."""
        from .dist import device_view
        p = C.c_void_p()
        L.check(self._lib.rau_question_grad_dev(self._h, C.byref(p)))
        n, Q = self._n, self.cfg.Q
        return device_view(p.value, n * Q, self.cfg.device_id).view(n, Q)

    # ---- the hop recurrence's ends (rau_set_state_dev, rau_backward_state): initial state in, state gradients out
    def set_state(self, c0, h0):
        """Attach the initial state (c0, h0), each [n,R], of the hop chain to the resident batch: contiguous CUDA torch
        tensors of one dtype, float32, float16 or bfloat16, on the ctx's device (16-bit values are widened exactly).
        One launch on the ctx's stream, no host synchronisation: set_question's ordering rule.  While it is attached
        forward / graph_step start hop 0 from it, and every backward leaves state_grad() behind.  The next
        set_batch* / use_batch / set_batch_size detaches it; attaching again replaces the contents."""
        import torch
        types = {torch.float32: "f32", torch.float16: "f16", torch.bfloat16: "bf16"}
        for name, t in (("c0", c0), ("h0", h0)):
            if not (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype in types and t.is_contiguous()):
                raise ValueError(f"{name} must be a contiguous float32, float16 or bfloat16 CUDA torch tensor")
            if t.device.index != self.cfg.device_id:
                raise ValueError(f"{name} is on {t.device}, the context on cuda:{self.cfg.device_id}")
            if tuple(t.shape) != (self._n, self.cfg.R):
                raise ValueError(f"{name} has shape {tuple(t.shape)}, expected {(self._n, self.cfg.R)}")
        if c0.dtype != h0.dtype:
            raise ValueError("c0 and h0 must have the same dtype")
        L.check(self._lib.rau_set_state_dev(self._h, c0.data_ptr(), h0.data_ptr(), feat16.FEAT_TYPES[types[c0.dtype]]))

    def clear_state(self):
        """Detach the initial state: the next forward starts from zeros."""
        L.check(self._lib.rau_set_state_dev(self._h, None, None, 0))

    def carry_state(self):
        """Attach the last forward's final state (c', h' of hop H-1) as the next forward's initial state: one launch,
        the values never leave the device."""
        c, h = C.c_void_p(), C.c_void_p()
        L.check(self._lib.rau_state_dev(self._h, C.byref(c), C.byref(h)))
        off = (self.cfg.H - 1) * self._n * self.cfg.R * 4
        L.check(self._lib.rau_set_state_dev(self._h, c.value + off, h.value + off, feat16.FEAT_TYPES["f32"]))

    @property
    def batch_state(self) -> bool:
        """The resident batch has an initial state attached (rau_batch_state)."""
        has = C.c_int(0)
        L.check(self._lib.rau_batch_state(self._h, C.byref(has)))
        return bool(has.value)

    def state_tensors(self):
        """Zero-copy torch views (c, h), each [H,n,R], of the hop states the last step-level forward left in device
        memory (rau_state_dev); row H-1 is the final state.  Valid until the next forward or set_batch_size, ordered
        on the ctx's stream (stream()), read-only."""
        from .dist import device_view
        c, h = C.c_void_p(), C.c_void_p()
        L.check(self._lib.rau_state_dev(self._h, C.byref(c), C.byref(h)))
        H, n, R, dev = self.cfg.H, self._n, self.cfg.R, self.cfg.device_id
        return (device_view(c.value, H * n * R, dev).view(H, n, R), device_view(h.value, H * n * R, dev).view(H, n, R))

    def state_grad(self):
        """The last backward's gradient (d_c0, d_h0), each [n,R], at the attached initial state (numpy; synchronises)."""
        dc = np.empty((self._n, self.cfg.R), np.float32)
        dh = np.empty((self._n, self.cfg.R), np.float32)
        L.check(self._lib.rau_get_state_grad(self._h, dc.ctypes.data, dh.ctypes.data))
        return dc, dh

    def state_grad_tensors(self):
        """Zero-copy torch views (d_c0, d_h0), each [n,R], of that gradient in device memory (rau_state_grad_dev).
        Valid until the next forward or set_batch_size, ordered on the ctx's stream (stream()), read-only."""
        from .dist import device_view
        dc, dh = C.c_void_p(), C.c_void_p()
        L.check(self._lib.rau_state_grad_dev(self._h, C.byref(dc), C.byref(dh)))
        n, R, dev = self._n, self.cfg.R, self.cfg.device_id
        return device_view(dc.value, n * R, dev).view(n, R), device_view(dh.value, n * R, dev).view(n, R)

    # ---- attention bias from the caller (rau_set_att_bias_dev): masks and priors in, the gradient at them out
    def set_att_bias(self, bias, regions=None):
        """Attach an additive attention bias [n,S] to the resident batch: bias[b,s] joins sample b's attention score at
        position s in every hop; -inf gives attention (and gradient) exactly 0 there.  One bias per batch, always per
        sample.  Three kinds of input:
          * a contiguous CUDA torch tensor of float32, float16 or bfloat16 on the ctx's device: zero-copy, one launch
            on the ctx's stream, no host synchronisation -- set_question's ordering rule.  Its values are not checked:
            +inf and NaN are the caller's error, a row without a finite entry in its attended range gives NaN;
          * a numpy array: checked first (check_att_bias: NaN, +inf, or a row with no finite entry among its attended
            positions raise ValueError before anything is uploaded), then uploaded into a context-owned staging
            buffer.  regions: the per-sample counts the batch carries, which the check needs (required when it has any);
          * None: detaches (clear_att_bias).
        While it is attached every backward leaves att_bias_grad() behind.  The next set_batch* / use_batch /
        set_batch_size detaches it; attaching again replaces the contents."""
        if bias is None:
            return self.clear_att_bias()
        n, S = self._n, self.cfg.S
        if isinstance(bias, np.ndarray):
            if regions is None and self._h and self.batch_regions():
                raise ValueError("the resident batch carries region counts: pass them as regions= for the check")
            b = check_att_bias(bias, n, S, regions)
            if getattr(self, "_att_bias_stage", None) is None:   # [capacity,S] floats, the ctx's until it is destroyed
                p = C.c_void_p()
                L.check(self._lib.rau_dev_alloc(self._h, self.capacity * S, C.byref(p)))
                self._att_bias_stage = p.value
            L.check(self._lib.rau_dev_upload(self._h, self._att_bias_stage, b.ctypes.data, b.nbytes))
            L.check(self._lib.rau_set_att_bias_dev(self._h, self._att_bias_stage, feat16.FEAT_TYPES["f32"]))
            return
        import torch
        t = bias
        types = {torch.float32: "f32", torch.float16: "f16", torch.bfloat16: "bf16"}
        if not (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype in types and t.is_contiguous()):
            raise ValueError("bias must be a numpy array or a contiguous float32, float16 or bfloat16 CUDA torch tensor")
        if t.device.index != self.cfg.device_id:
            raise ValueError(f"bias is on {t.device}, the context on cuda:{self.cfg.device_id}")
        if tuple(t.shape) != (n, S):
            raise ValueError(f"bias has shape {tuple(t.shape)}, expected {(n, S)}")
        L.check(self._lib.rau_set_att_bias_dev(self._h, t.data_ptr(), feat16.FEAT_TYPES[types[t.dtype]]))

    def set_att_mask(self, allowed, regions=None):
        """set_att_bias(where(allowed, 0, -inf)): allowed [n,S] of bool, a numpy array or a CUDA torch tensor."""
        if isinstance(allowed, np.ndarray):
            if allowed.dtype != np.bool_:
                raise ValueError("allowed must be a bool array")
            return self.set_att_bias(np.where(allowed, np.float32(0), np.float32(-np.inf)), regions=regions)
        import torch
        if not (isinstance(allowed, torch.Tensor) and allowed.dtype == torch.bool):
            raise ValueError("allowed must be a bool numpy array or a bool CUDA torch tensor")
        zero = torch.zeros((), dtype=torch.float32, device=allowed.device)
        b = torch.where(allowed, zero, zero - float("inf")).contiguous()
        own = torch.cuda.ExternalStream(self.stream(), device=allowed.device)
        own.wait_stream(torch.cuda.current_stream(allowed.device))   # the bias was written on torch's stream
        b.record_stream(own)                    # ... and is read by the ctx's: not handed out again before that
        self.set_att_bias(b)

    def clear_att_bias(self):
        """Detach the attention bias: the resident batch's scores are the model's own again."""
        L.check(self._lib.rau_set_att_bias_dev(self._h, None, 0))

    @property
    def batch_att_bias(self) -> bool:
        """The resident batch has an attention bias attached (rau_batch_att_bias)."""
        has = C.c_int(0)
        L.check(self._lib.rau_batch_att_bias(self._h, C.byref(has)))
        return bool(has.value)

    def att_bias_grad(self):
        """The last backward's gradient at the attached attention bias [n,S] (numpy; synchronises)."""
        out = np.empty((self._n, self.cfg.S), np.float32)
        L.check(self._lib.rau_get_att_bias_grad(self._h, out.ctypes.data))
        return out

    def att_bias_grad_tensor(self):
        """Zero-copy torch view [n,S] (rows at the device pitch) of that gradient in device memory
        (rau_att_bias_grad_dev).  Valid until the next forward or set_batch_size, ordered on the ctx's stream
        (stream()), read-only; no synchronisation."""
        from .dist import device_view
        p, pitch = C.c_void_p(), C.c_int32()
        L.check(self._lib.rau_att_bias_grad_dev(self._h, C.byref(p), C.byref(pitch)))
        n, S, P = self._n, self.cfg.S, int(pitch.value)
        return device_view(p.value, n * P, self.cfg.device_id).view(n, P)[:, :S]

    def set_batch_dev(self, feats_cuda, tokens, lens, labels=None, answers=None, regions=None, att_targets=None,
                      image_of=None, question=None, sample_w=None, candidates=None, state=None, att_bias=None):
        """set_batch with the maps already on the device: feats_cuda a contiguous float32 CUDA torch tensor
        [n,D,S] on the ctx's device (rau_set_batch_dev: one copy on the ctx's stream, no host synchronisation).
        The ctx's stream must be ordered behind the stream that wrote the tensor (autograd.step's docstring shows
        the two lines); the tensor must stay unchanged until that copy has run.  answers, regions, att_targets as
        in set_batch.  image_of [n] (0-based rows): feats_cuda is an image TABLE [N,D,S] (rau_set_batch_dev_images);
        regions may then be per image [N].  question: a CUDA tensor [n,Q] attached behind the upload (set_question);
        tokens / lens may then be None -- the step does not read them, and id 1 with length 1 is uploaded.
        sample_w [n]: set_sample_weights behind the upload.
        candidates [n, C]: set_candidates behind the upload.
        state: (c0, h0), CUDA tensors [n,R] attached behind the upload (set_state).
        att_bias: [n,S] attached behind the upload (set_att_bias; a numpy bias is checked against `regions`)."""
        import torch
        c = self.cfg
        if question is not None and (tokens is None or lens is None):
            if not (isinstance(question, torch.Tensor) and question.dim() == 2):
                raise ValueError("question must be a CUDA torch tensor [n,Q]")
            tokens = np.ones((c.T, int(question.shape[0])), np.int32)
            lens = np.ones((int(question.shape[0]),), np.int32)
        lens = np.ascontiguousarray(lens, np.int32)
        B = self._rows(lens, "set_batch_dev")
        t = feats_cuda
        if not (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.float32 and t.is_contiguous()):
            raise ValueError("feats_cuda must be a contiguous float32 CUDA torch tensor")
        if t.device.index != c.device_id:
            raise ValueError(f"feats_cuda is on {t.device}, the context on cuda:{c.device_id}")
        if image_of is not None:
            image_of = np.ascontiguousarray(image_of, np.int32)
            if image_of.shape != (B,) or t.dim() != 3 or tuple(t.shape[1:]) != (c.D, c.S) or t.shape[0] < 1:
                raise ValueError(f"an image table needs image_of [{B}] and feats_cuda [N, {c.D}, {c.S}]")
        elif tuple(t.shape) != (B, c.D, c.S):
            raise ValueError(f"feats_cuda has shape {tuple(t.shape)}, expected {(B, c.D, c.S)}")
        tokens = np.ascontiguousarray(tokens, np.int32)
        if tokens.shape != (c.T, B):
            raise ValueError("batch shapes do not match the config")
        lp = None
        if labels is not None:
            labels = np.ascontiguousarray(labels, np.int32)
            if labels.shape != (B,):
                raise ValueError("labels shape")
            lp = labels.ctypes.data
        if regions is not None:
            regions = self._sample_regions(regions, image_of, B)
        if att_targets is not None:
            att_targets = self._att_targets(att_targets, B)
        if sample_w is not None:
            sample_w = self._sample_weights(sample_w, B)
        if candidates is not None:
            candidates = self._candidates(candidates, B)
        if B != self._n:
            self.set_batch_size(B)
        if image_of is not None:
            L.check(self._lib.rau_set_batch_dev_images(self._h, t.data_ptr(), int(t.shape[0]), image_of.ctypes.data,
                                                       tokens.ctypes.data, lens.ctypes.data, lp))
        else:
            L.check(self._lib.rau_set_batch_dev(self._h, t.data_ptr(), tokens.ctypes.data, lens.ctypes.data, lp))
        if answers is not None:
            self.set_answers(*answers)
        if regions is not None:
            self.set_regions(regions)
        if att_targets is not None:
            self.set_att_targets(att_targets)
        if sample_w is not None:
            self.set_sample_weights(sample_w)
        if candidates is not None:
            self.set_candidates(candidates)
        if question is not None:
            self.set_question(question)
        if state is not None:
            self.set_state(*state)
        if att_bias is not None:
            self.set_att_bias(att_bias, regions=regions if isinstance(att_bias, np.ndarray) else None)

    def graph_step(self, hop_w, zero_grads=True, select_w=None, att_w=None, merge_w=None):
        """zero_grads + forward + backward as one hipGraph launch (captured on first use); select_w, att_w and
        merge_w as in backward (read from device memory: they may change between replays)."""
        family, ws = self._loss_args(hop_w, select_w, att_w, merge_w)
        L.check(getattr(self._lib, "rau_graph_step" + family)(self._h, *ws, int(zero_grads)))

    def sync(self):
        L.check(self._lib.rau_sync(self._h))

    def update(self, step_t, lr=3e-3, mult_lr=3e-4, beta1=0.9, beta2=0.999, eps=1e-8,
               eta=0.01, gamma=0.55, clip=0.1, noise_seed=0, rule="adam", clip_scope="group",
               weight_decay=0.0, ema_decay=0.0):
        """Noise, clip and the optimizer step.  With rule and clip_scope at their defaults this is the reference's
        update (rau_noise_clip_adam) and returns the three groups' pre-clip norms.  rule="adamax" and / or
        clip_scope="global" (neither is in the reference) go through rau_update and return four norms: the groups'
        and the global one.  A non-zero weight_decay (decoupled, AdamW's order, under either rule) or ema_decay (the
        weight average: ema_reset first), or any layer option off its default (set_layer_opts, freeze), goes through
        rau_update_ex and returns four norms as well; frozen layers are in none of them.  With guard_updates() on, a
        call that finds a non-finite gradient element is skipped and returns NaN norms (update_guard tells)."""
        if rule not in L.OPT_RULES:
            raise ValueError(f"update: rule {rule!r} is not one of {sorted(L.OPT_RULES)}")
        if clip_scope not in L.CLIP_SCOPES:
            raise ValueError(f"update: clip_scope {clip_scope!r} is not one of {sorted(L.CLIP_SCOPES)}")
        extras = weight_decay != 0 or ema_decay != 0 or bool(getattr(self, "_layer_custom", None))
        if rule == "adam" and clip_scope == "group" and not extras:
            norms = np.zeros(3, np.float32)
            L.check(self._lib.rau_noise_clip_adam(self._h, step_t, lr, mult_lr, beta1, beta2, eps,
                                                  eta, gamma, clip, noise_seed, norms.ctypes.data))
            return norms
        o = L.RauUpdateOpts(rule=L.OPT_RULES[rule], clip_scope=L.CLIP_SCOPES[clip_scope], lr=lr, mult_lr=mult_lr,
                            beta1=beta1, beta2=beta2, eps=eps, eta=eta, gamma=gamma, clip=clip,
                            noise_seed=noise_seed)
        norms = np.zeros(4, np.float32)
        if extras:
            x = L.RauUpdateExtras(weight_decay=weight_decay, ema_decay=ema_decay)
            L.check(self._lib.rau_update_ex(self._h, step_t, C.byref(o), C.byref(x), norms.ctypes.data))
            return norms
        L.check(self._lib.rau_update(self._h, step_t, C.byref(o), norms.ctypes.data))
        return norms

    # ---- per-layer statistics on the device (rau_layer_stats) and the non-finite guard (rau_set_update_guard)
    def _stat_names(self):
        """[(entry name, group)] in the records' order: rau_layout_entry's, EMBED then RNN then MULT."""
        if getattr(self, "_stat_entries", None) is None:
            self._stat_entries = [(e[0], g) for g in L.GROUPS for e in self.layout(g)]
        return self._stat_entries

    @staticmethod
    def _stat_what(grads, params, direction):
        what = (L.STAT_GRAD if grads else 0) | (L.STAT_PARAM if params else 0) | (L.STAT_DIR if direction else 0)
        if not what:
            raise ValueError("layer_stats: ask for at least one of grads, params, direction")
        return what

    def layer_stats(self, grads=True, params=False, direction=False, eps=1e-8):
        """Statistics of every layout entry, computed on the device (two launches, one download of 35 records in
        place of the flat vectors): a list of dicts in layout order with name, group, n and, per requested source
        under "grad", "param", "dir", a dict of norm (sqrt of the f32 sum of squares of the FINITE elements, taken
        in float64 here), sumsq, absmax (largest finite magnitude) and nonfinite (NaN and +-Inf elements).
        direction: the rule's direction from the moments as they stand, m / (sqrt(v) + eps) or Adamax's m / u; it
        needs an update to have run.  Frozen layers are reported like any other.  Synchronises."""
        what = self._stat_what(grads, params, direction)
        names = self._stat_names()
        rec = (L.RauLayerStat * len(names))()
        L.check(self._lib.rau_layer_stats(self._h, what, eps, rec))
        out = []
        for (name, g), r in zip(names, rec):
            row = {"name": name, "group": g, "n": int(r.n)}
            for k, (key, bit) in enumerate((("grad", L.STAT_GRAD), ("param", L.STAT_PARAM), ("dir", L.STAT_DIR))):
                if what & bit:
                    row[key] = {"norm": float(np.sqrt(np.float64(r.sumsq[k]))), "sumsq": np.float32(r.sumsq[k]),
                                "absmax": np.float32(r.absmax[k]), "nonfinite": int(r.nonfinite[k])}
            out.append(row)
        return out

    def layer_stats_tensor(self, grads=True, params=False, direction=False, eps=1e-8):
        """The same records as zero-copy torch views of the device array (rau_layer_stats_dev), no synchronisation:
        {"sumsq": [count, 3] float32, "absmax": [count, 3] float32, "nonfinite": [count, 3] int64, "n": [count]
        int64}, the columns being grad, param, dir (0 where not requested).  Ordered on the ctx's stream (stream()),
        valid until the next layer_stats / layer_stats_tensor call, read-only."""
        import torch
        from .dist import device_view
        what = self._stat_what(grads, params, direction)
        dev = C.c_void_p()
        L.check(self._lib.rau_layer_stats_dev(self._h, what, eps, C.byref(dev)))
        count, words = len(self._stat_names()), C.sizeof(L.RauLayerStat) // 4
        raw = device_view(dev.value, count * words, self.cfg.device_id).view(count, words)
        ints = raw[:, 6:].view(torch.int64)
        return {"sumsq": raw[:, 0:3], "absmax": raw[:, 3:6], "nonfinite": ints[:, 0:3], "n": ints[:, 3]}

    def update_ratios(self, lr=3e-3, mult_lr=3e-4, beta1=0.9, beta2=0.999, eps=1e-8, rule="adam"):
        """{layer name: step * ||dir|| / ||x||}: the size of the step the last update took in every unit (weight and
        bias together) relative to its weights, from one layer_stats call.  The step size is formed as rau_update_ex
        forms it, in double on the host, from the groups' update count t, the unit's lr_scale and the rule:
        group_lr * lr_scale * sqrt(1 - beta2^t) / (1 - beta1^t) for "adam", group_lr * lr_scale / (1 - beta1^t) for
        "adamax".  A unit whose weights are all zero gives inf; a frozen unit gives 0."""
        if rule not in L.OPT_RULES:
            raise ValueError(f"update_ratios: rule {rule!r} is not one of {sorted(L.OPT_RULES)}")
        st = self.layer_stats(grads=False, params=True, direction=True, eps=eps)
        sums = {}
        for row in st:
            base = row["name"].rsplit(".", 1)[0]
            d, x = sums.get((base, row["group"]), (0.0, 0.0))
            sums[(base, row["group"])] = (d + float(row["dir"]["sumsq"]), x + float(row["param"]["sumsq"]))
        ts = {}
        for g in L.GROUPS:
            t = C.c_int64()
            L.check(self._lib.rau_get_opt_state(self._h, L.GROUPS[g], None, None, C.byref(t), None))
            ts[g] = int(t.value)
        out = {}
        for name, g, i in self.layers():
            group_lr = mult_lr if g == "mult" else lr
            bc1, bc2 = 1.0 - float(beta1) ** ts[g], 1.0 - float(beta2) ** ts[g]
            scale = self._layer_get(g, i)[0]
            step = group_lr * scale * np.sqrt(bc2) / bc1 if rule == "adam" else group_lr * scale / bc1
            d, x = sums[(name, g)]
            out[name] = float(np.float32(step) * np.sqrt(d) / np.sqrt(x)) if x > 0 else float("inf")
        return out

    def guard_updates(self, on=True):
        """With the guard on, every update first counts the non-finite elements of the gradients on the device (one
        more read of them and a stream synchronisation per update; frozen layers are left out where layer options
        are in force).  A clean step runs exactly as without the guard.  A poisoned one is skipped: weights,
        gradients, moments, the average and the update count keep their bits, update() returns NaN norms, and
        update_guard counts it.  Gradients accumulated over several backward calls keep a NaN until zero_grads():
        every update is skipped until then."""
        L.check(self._lib.rau_set_update_guard(self._h, L.GUARD_SKIP if on else L.GUARD_OFF))

    @property
    def update_guard(self):
        """{"mode": 0 | 1, "skipped": updates skipped so far, "last_skipped": whether the last update was,
        "last_nonfinite": {group: non-finite gradient elements the last skipped update found}}."""
        mode, skipped, last = C.c_int(), C.c_int64(), C.c_int32()
        nf = (C.c_int64 * 3)()
        L.check(self._lib.rau_update_guard(self._h, C.byref(mode), C.byref(skipped), C.byref(last), nf))
        return {"mode": int(mode.value), "skipped": int(skipped.value), "last_skipped": bool(last.value),
                "last_nonfinite": {g: int(nf[i]) for g, i in L.GROUPS.items()}}

    # ---- per-layer options (rau_set_layer_opts): a layer is a named unit, weight and bias, of the layout
    def layers(self):
        """[(name, group, index)]: the units rau_set_layer_opts addresses, in layout order."""
        if getattr(self, "_layers", None) is None:
            self._layers = layer_units({g: self.layout(g) for g in L.GROUPS})
        return self._layers

    def set_layer_opts(self, name_or_glob, lr_scale=None, decay=None, bias_decay=None):
        """Step-size scale, weight-decay multiplier of the weight and of the bias (defaults 1, 1, 0) of the layer
        named, or of every layer an fnmatch pattern such as "classifier.*" matches; what is None keeps its value.
        lr_scale = 0 freezes.  Returns the names changed; a name or pattern that matches nothing is a KeyError.
        Only updates with these options in force (RAU.update routes them to rau_update_ex) look at them."""
        hit = match_layers(name_or_glob, self.layers())
        for name, g, i in hit:
            cur = self._layer_get(g, i)
            new = tuple(float(c if v is None else v) for c, v in zip(cur, (lr_scale, decay, bias_decay)))
            L.check(self._lib.rau_set_layer_opts(self._h, L.GROUPS[g], i, *new))
            if getattr(self, "_layer_custom", None) is None:
                self._layer_custom = set()
            (self._layer_custom.discard if new == LAYER_DEFAULTS else self._layer_custom.add)(name)
        return [name for name, _, _ in hit]

    def _layer_get(self, group, index):
        v = [C.c_float(), C.c_float(), C.c_float()]
        L.check(self._lib.rau_get_layer_opts(self._h, L.GROUPS[group], index, *(C.byref(x) for x in v)))
        return tuple(float(x.value) for x in v)

    def layer_opts(self):
        """{name: (lr_scale, decay, bias_decay)} of every layer."""
        return {name: self._layer_get(g, i) for name, g, i in self.layers()}

    def freeze(self, *names):
        """lr_scale = 0: the layers' weights, moments, average and gradients keep their bits, and they are in no
        norm.  The backward still forms their gradients."""
        return [n for p in names for n in self.set_layer_opts(p, lr_scale=0.0)]

    def unfreeze(self, *names):
        """lr_scale back to 1 (for another scale use set_layer_opts)."""
        return [n for p in names for n in self.set_layer_opts(p, lr_scale=1.0)]

    # ---- the weight average (rau_ema_*): updated by update(ema_decay=...), swapped in for evaluation
    def ema_reset(self):
        """average := current weights (allocated at the first use)."""
        L.check(self._lib.rau_ema_reset(self._h))

    def ema_swap(self):
        """Exchange weights and average in place, one launch.  While swapped every reader of the weights sees the
        average and every update is refused; a second swap restores every bit."""
        L.check(self._lib.rau_ema_swap(self._h))

    def _ema_state(self):
        has, sw = C.c_int(), C.c_int()
        L.check(self._lib.rau_ema_state(self._h, C.byref(has), C.byref(sw)))
        return bool(has.value), bool(sw.value)

    @property
    def has_ema(self) -> bool:
        return self._ema_state()[0]

    @property
    def ema_swapped(self) -> bool:
        return self._ema_state()[1]

    def ema(self):
        """{group: float32 vector}: the average (while swapped: the trained weights)."""
        return {g: self._get(self._lib.rau_get_ema, g) for g in L.GROUPS}

    def set_ema(self, ema):
        for g, a in ema.items():
            a = np.ascontiguousarray(a, np.float32)
            L.check(self._lib.rau_set_ema(self._h, L.GROUPS[g], a.ctypes.data, a.size))

    @contextlib.contextmanager
    def averaged(self):
        """with m.averaged(): ... runs its body on the averaged weights and swaps back on the way out."""
        self.ema_swap()
        try:
            yield self
        finally:
            self.ema_swap()

    # ---- optimizer state (rau_get_opt_state / rau_set_opt_state): what a resumed run needs besides the parameters
    def opt_state(self):
        """-> ({group: (m, v, t)}, rule): the moments as float32 vectors (v holds Adamax's u), the update count
        and the rule that owns the state ("adam" before the first update)."""
        names = {v: k for k, v in L.OPT_RULES.items()}
        out, rule = {}, None
        for g in L.GROUPS:
            n = self.group_size(g)
            m, v = np.empty(n, np.float32), np.empty(n, np.float32)
            t, r = C.c_int64(), C.c_int32()
            L.check(self._lib.rau_get_opt_state(self._h, L.GROUPS[g], m.ctypes.data, v.ctypes.data,
                                                C.byref(t), C.byref(r)))
            out[g] = (m, v, int(t.value))
            if rule is None:            # every update writes all three groups, so they agree
                rule = r.value
        return out, names[rule]

    def set_opt_state(self, state, rule="adam"):
        """state: {group: (m, v, t)} as opt_state returns it; groups not named keep theirs."""
        if rule not in L.OPT_RULES:
            raise ValueError(f"set_opt_state: rule {rule!r} is not one of {sorted(L.OPT_RULES)}")
        for g, (m, v, t) in state.items():
            m, v = np.ascontiguousarray(m, np.float32).ravel(), np.ascontiguousarray(v, np.float32).ravel()
            n = self.group_size(g)
            if m.size != n or v.size != n:
                raise ValueError(f"set_opt_state: group {g} has {n} floats, got {m.size} and {v.size}")
            L.check(self._lib.rau_set_opt_state(self._h, L.GROUPS[g], m.ctypes.data, v.ctypes.data, int(t),
                                                L.OPT_RULES[rule]))

    def reset_opt_state(self, rule="adam"):
        """Zero moments and t = 0 in every group, owned by `rule` from now on: the way to change rule."""
        if rule not in L.OPT_RULES:
            raise ValueError(f"reset_opt_state: rule {rule!r} is not one of {sorted(L.OPT_RULES)}")
        for g in L.GROUPS:
            L.check(self._lib.rau_set_opt_state(self._h, L.GROUPS[g], None, None, 0, L.OPT_RULES[rule]))

    # ---- results
    def _out(self, fn, shape, dtype=np.float32):
        a = np.empty(shape, dtype)
        L.check(fn(self._h, a.ctypes.data))
        return a

    def losses(self):
        return self._out(self._lib.rau_get_losses, (self.cfg.H,))

    def loss_rows(self):
        """The per-sample loss rows [H, n] of the last forward: losses() is their mean over n.  With sample weights
        these are the weighted rows s_b * row."""
        return self._out(self._lib.rau_get_loss_rows, (self.cfg.H, self._n))

    def argmax(self):
        return self._out(self._lib.rau_get_argmax, (self.cfg.H, self._n), np.int32)

    def logits(self):
        return self._out(self._lib.rau_get_logits, (self.cfg.H, self._n, self.cfg.K))

    def dopred(self):
        return self._out(self._lib.rau_get_dopred, (self.cfg.H, self._n))

    def attention(self):
        return self._out(self._lib.rau_get_attention, (self.cfg.H, self._n, self.cfg.S))

    def question_state(self):
        return self._out(self._lib.rau_get_question_state, (self._n, self.cfg.Q))

    def att_state(self):
        c = np.empty((self.cfg.H, self._n, self.cfg.R), np.float32)
        h = np.empty_like(c)
        L.check(self._lib.rau_get_att_state(self._h, c.ctypes.data, h.ctypes.data))
        return c, h

    # ---- merged hops on the device (valid from a forward through its backward, include/rau.h)
    def step_stats(self):
        """feval's bookkeeping of the last forward (SS:476-556, last hop not forced): ``loss`` [H+2]
        (per-hop CE, uni CE, select CE), ``loss_do_pred`` [H] (BCE of do_pred vs argmax_h == y) and
        the counts: ``correct`` [H+2], ``do_pred_correct`` [H] (masked by did_correct),
        ``did_correct``, ``fired`` [H] (do_pred > 0.5), ``selected`` [H] (select row = hop h)."""
        H = self.cfg.H
        loss = np.empty(H + 2, np.float32)
        ldp = np.empty(H, np.float32)
        cnt = np.empty(4 * H + 3, np.int32)
        L.check(self._lib.rau_step_stats(self._h, loss.ctypes.data, ldp.ctypes.data, cnt.ctypes.data))
        return {"loss": loss, "loss_do_pred": ldp, "correct": cnt[:H + 2],
                "do_pred_correct": cnt[H + 2:2 * H + 2], "did_correct": int(cnt[2 * H + 2]),
                "fired": cnt[2 * H + 3:3 * H + 3], "selected": cnt[3 * H + 3:]}

    def predict(self, mc_ans=None):
        """predict_result's answers of the last forward (SS:633-705, 877-900, last hop forced):
        (oe [H+2, B], mc [H+2, B] or None), 1-based, rows = hops, uni, select.  mc_ans: int
        [B, n] candidate ids, 0 = empty slot."""
        H, B = self.cfg.H, self._n
        oe = np.empty((H + 2, B), np.int32)
        if mc_ans is None:
            L.check(self._lib.rau_predict(self._h, None, 0, oe.ctypes.data, None))
            return oe, None
        m = np.ascontiguousarray(mc_ans, np.int32)
        if m.ndim != 2 or m.shape[0] != B:
            raise ValueError("mc_ans must be [B, n]")
        mc = np.empty((H + 2, B), np.int32)
        L.check(self._lib.rau_predict(self._h, m.ctypes.data, m.shape[1], oe.ctypes.data, mc.ctypes.data))
        return oe, mc

    def merged(self):
        """Merged rows of the last predict(): pred [2, B, K], att [2, B, S] (uni, select; select
        without the reference's carried test_select_att)."""
        pred = np.empty((2, self._n, self.cfg.K), np.float32)
        att = np.empty((2, self._n, self.cfg.S), np.float32)
        L.check(self._lib.rau_get_merged(self._h, pred.ctypes.data, att.ctypes.data))
        return pred, att

    def topk(self, k):
        """The k best open-ended answers of every predict_result row of the last forward (hops, uni,
        select; last hop forced, as predict()): (ids int32, score f32, conf f32), each [H+2, B, k],
        best first.  Larger logit first, equal logits by the lower id, so ``ids[..., 0]`` is
        predict()'s ``oe``; ``score`` is the row's logit at that id bit for bit, ``conf`` its softmax
        probability.  predict.top_answers is the numpy restatement."""
        shape = (self.cfg.H + 2, self._n, int(k))
        ids = np.empty(shape, np.int32)
        score = np.empty(shape, np.float32)
        conf = np.empty(shape, np.float32)
        L.check(self._lib.rau_topk(self._h, int(k), ids.ctypes.data, score.ctypes.data, conf.ctypes.data))
        return ids, score, conf

    def outputs(self):
        c, h = self.att_state()
        return {"losses": self.losses(), "argmax": self.argmax(), "logits": self.logits(),
                "dopred": self.dopred(), "att": self.attention(), "q": self.question_state(),
                "att_c": c, "att_h": h}

    # ---- timing
    def stream(self) -> int:
        s = C.c_void_p()
        L.check(self._lib.rau_stream(self._h, C.byref(s)))
        return s.value or 0

    # ---- native data-parallel exchange (RCCL inside librau, no torch.distributed needed)
    @staticmethod
    def comm_unique_id() -> bytes:
        buf = C.create_string_buffer(128)
        L.check(L.lib().rau_comm_unique_id(buf, 128))
        return buf.raw

    def comm_init(self, nranks: int, rank: int, uid: bytes):
        L.check(self._lib.rau_comm_init(self._h, nranks, rank, uid, len(uid)))

    def allreduce_grads(self):
        """Average the three flat gradient buffers over all ranks, in place, ordered on the
        ctx stream (mult bucket overlapped with the encoder BPTT)."""
        L.check(self._lib.rau_allreduce_grads(self._h))

    def comm_destroy(self):
        L.check(self._lib.rau_comm_destroy(self._h))

    def wait_grads(self, group: str, hip_stream: int):
        """Order `hip_stream` after the last backward's gradients of `group` (no host sync)."""
        L.check(self._lib.rau_wait_grads(self._h, L.GROUPS[group], C.c_void_p(hip_stream)))

    def timer_begin(self):
        L.check(self._lib.rau_timer_begin(self._h))

    def timer_end(self) -> float:
        ms = C.c_float()
        L.check(self._lib.rau_timer_end(self._h, C.byref(ms)))
        return ms.value

    def prof_enable(self, on=True):
        L.check(self._lib.rau_prof_enable(self._h, int(on)))

    def prof_reset(self):
        L.check(self._lib.rau_prof_reset(self._h))

    def prof(self):
        out = {}
        n = self._lib.rau_prof_count(self._h)
        for i in range(n):
            name, cnt = C.c_char_p(), C.c_int64()
            ms, fl, by = C.c_double(), C.c_double(), C.c_double()
            L.check(self._lib.rau_prof_entry(self._h, i, C.byref(name), C.byref(cnt),
                                             C.byref(ms), C.byref(fl), C.byref(by)))
            out[name.value.decode()] = {"launches": cnt.value, "ms": ms.value,
                                        "flops": fl.value, "bytes": by.value}
        return out
