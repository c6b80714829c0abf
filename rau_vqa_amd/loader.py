"""Host-side batch producer with the reference loader's contract.

Restates utils/vqa_prepro_loader.lua of the reference:
  * ``load_data`` (lines 1294-1473): question tensors + vocabulary from ``data_prepro.h5`` /
    ``data_prepro.json``; word ids are shifted by one so that id 1 is ZEROPAD (1335, 1393);
  * batch order options 1-4 (1219-1291): shuffle / inorder / sort by length / randsort;
  * ``next_batch_feat`` (837-1010): returns ``feats [B,D,W,H]``, ``x [T,B]`` (transposed),
    ``x_len [B]``, answers ``[B]`` (train) or multiple-choice ids ``[B,nMC]`` (test) and
    ``qids [B]``; per-image features are ``torch.save``d FloatTensors named after the image
    (``COCO_*.t7``), looked up in ``tab_featpaths[datatype]``; the order is re-drawn when fewer
    than one batch is left; with prefetch the NEXT batch's feature files are read by one
    background worker while the current batch is being used (the reference's ``threads`` pool).

What differs, and why: the HDF5 question file needs ``h5py``, which is not installed in the build
image -- ``load_data`` reads it when h5py is importable and otherwise an ``.npz`` with the same
dataset names; Torch's ``randperm`` / unstable ``sort`` streams cannot be reproduced, numpy's
seeded generator and a stable sort are used instead (same distribution, different draws).
"""
from __future__ import annotations

import json
import os
import threading
from dataclasses import dataclass

import numpy as np

from . import feat16, t7


@dataclass
class QuestionSet:
    question: np.ndarray      # [N, T] int32, ids already +1 (1 = ZEROPAD)
    lengths_q: np.ndarray     # [N]
    img_list: np.ndarray      # [N] 1-based index into the image-name list
    question_id: np.ndarray   # [N]
    answers: np.ndarray = None    # [N] 1-based answer id (train)
    mc_ans: np.ndarray = None     # [N, nMC] (test)
    datatype: np.ndarray = None   # [N] 1-based index into tab_featpaths
    # multi-answer ground truth (rau_set_answers), all optional: [N, G] answer ids (1-based, 0 = empty entry),
    # loss weights, metric scores (None: the weights), e.g. vqa_scores(counts)
    ans_ids: np.ndarray = None
    ans_w: np.ndarray = None
    ans_score: np.ndarray = None
    # region counts (rau_set_regions), optional: [number of images] valid positions of every image of the name
    # list (prefix-packed region features padded to S), indexed like img_list
    img_regions: np.ndarray = None


def vqa_scores(counts):
    """The VQA accuracy of an answer that `counts` of the ten annotators gave: min(counts / 3, 1), float32."""
    return np.minimum(np.asarray(counts, np.float32) / np.float32(3), np.float32(1)).astype(np.float32)


def feature_name(img_path: str) -> str:
    """'train2014/COCO_train2014_000000357413.jpg' -> 'COCO_train2014_000000357413.t7'."""
    base = os.path.basename(img_path)
    stem, ext = os.path.splitext(base)
    return stem + ".t7" if ext else base + ".t7"


class DataClass:
    """One split's batch iterator (the reference's ``dataclass``)."""

    def __init__(self, qs: QuestionSet, img_names, batch_size, split="train", prefetch=False,
                 seed=123, feat_type="f32"):
        self.qs, self.img_names, self.batch_size, self.split = qs, list(img_names), batch_size, split
        # element type of the feats next_batch_feat returns: "f32" | "f16" | "bf16" (uint16 bits) | "e4m3" | "e5m2"
        # (uint8 codes: the files' f32 / f16 values narrowed on the host by feat16.fp8_bits)
        self.feat_type = feat16.check_name(feat_type)
        self.n = int(qs.question.shape[0])
        if self.n < batch_size:
            raise ValueError(f"{self.n} examples < batch_size {batch_size}")
        self.seq_len = int(qs.question.shape[1])
        self.opt_prefetch = prefetch
        self.opt_batch_order = 2
        self.rng = np.random.default_rng(seed)
        self.batch_index = 0
        self.batch_order = np.arange(self.n)
        self._job = None          # (key, thread, result holder)
        self._next_dest = None    # SlotFeeder: where the prefetch worker assembles the next batch
        self._unique = False      # the last next_batch_feat asked for an image table: so will the prefetched one
        self._packed = False      # ... for packed region rows: so will the prefetched one
        self._bank = None         # (key, files, row of every question): bank_rows' answer for one tab_featpaths
        self.last_answers = None  # (ids, w[, score]) rows of the batch last taken, when qs carries answer sets
        self.last_regions = None  # [B] per-sample region counts of the batch last taken, when qs carries img_regions

    # ---- batch order options, loader.lua:1219-1291
    def set_batch_order_option(self, opt):
        if opt not in (1, 2, 3, 4):
            raise ValueError("batch order option must be 1 (shuffle), 2 (inorder), 3 (sort), 4 (randsort)")
        self.opt_batch_order = opt

    def reorder(self):
        self.batch_index = 0
        self._job = None
        lens = np.asarray(self.qs.lengths_q)
        if self.opt_batch_order == 1:
            self.batch_order = self.rng.permutation(self.n)
        elif self.opt_batch_order == 2:
            self.batch_order = np.arange(self.n)
        elif self.opt_batch_order == 3:
            self.batch_order = np.argsort(lens, kind="stable")
        else:   # sorted by length, ties shuffled
            order = np.argsort(lens, kind="stable")
            s = lens[order]
            i = 0
            while i < self.n:
                j = i
                while j < self.n and s[j] == s[i]:
                    j += 1
                order[i:j] = order[i:j][self.rng.permutation(j - i)]
                i = j
            self.batch_order = order

    def reset_batch_pointer(self):
        self.batch_index = 0

    # ---- features
    def _paths(self, start, tab_featpaths):
        idx = self.batch_order[start:start + self.batch_size]
        dt = self.qs.datatype[idx] if self.qs.datatype is not None else np.ones(len(idx), int)
        return [os.path.join(tab_featpaths[int(d) - 1],
                             feature_name(self.img_names[int(self.qs.img_list[i]) - 1]))
                for i, d in zip(idx, dt)]

    @staticmethod
    def _image_table(paths):
        """The batch's distinct feature paths in order of first appearance, and image_of [B] int32: the
        0-based row of that list each sample looks at.  Duplicates are found by path, so the questions of
        one image need not be adjacent."""
        row, uniq = {}, []
        image_of = np.empty(len(paths), np.int32)
        for b, p in enumerate(paths):
            if p not in row:
                row[p] = len(uniq)
                uniq.append(p)
            image_of[b] = row[p]
        return uniq, image_of

    @staticmethod
    def _load_feats(paths, D, W, H, out=None, feat_type="f32"):
        """Per-image feature files into one [B,D,W,H] array of feat_type; `out` = a caller-owned
        destination (the pinned staging of an upload slot: the batch is assembled where the H2D copy
        reads it), whose dtype then decides; fewer paths than it has room for (an image table) fill its
        first len(paths) maps.  f32 files are rounded into a 16-bit destination on
        assignment; HalfTensor files are copied as they are into an fp16 one.  An fp8 destination (uint8:
        `feat_type` says which format) takes feat16.fp8_bits of the files' values."""
        if out is None:
            out = np.zeros((len(paths), D, W, H), feat16.dtype_of(feat_type))
        else:
            out = out.reshape(-1)[:len(paths) * D * W * H].reshape(len(paths), D, W, H)
        keep_half = out.dtype != np.float32
        for i, p in enumerate(paths):   # load_feature asserts the three sizes
            feat16.store(out[i], t7.load_feature(p, D, W, H, keep_half).reshape(D, W, H), feat_type)
        return out

    @staticmethod
    def _load_rows(paths, D, S, out=None, feat_type="f32"):
        """Per-image region files [n, D] (t7.load_regions) -> (rows [sum(n), D] of feat_type, counts [len(paths)]
        int32): every file read once, the rows concatenated without padding or transposing.  `out` = a caller-owned
        destination (the pinned staging of an upload slot) whose start takes the rows and whose dtype decides.
        n above S (the context's position count) is an error."""
        dt = feat16.dtype_of(feat_type) if out is None else out.dtype
        keep_half = dt != np.float32
        maps = [t7.load_regions(p, D, keep_half) for p in paths]
        counts = np.array([m.shape[0] for m in maps], np.int32)
        if counts.max() > S:
            raise ValueError(f"a region file holds {int(counts.max())} boxes, above S={S}")
        total = int(counts.sum())
        if out is None:
            rows = np.empty((total, D), dt)
        else:
            if out.size < total * D:
                raise ValueError("the packed rows do not fit the destination")
            rows = out.reshape(-1)[:total * D].reshape(total, D)
        off = 0
        for m in maps:
            feat16.store(rows[off:off + m.shape[0]], m, feat_type)
            off += m.shape[0]
        return rows, counts

    def _start_prefetch(self, tab_featpaths, D, W, H):
        paths = self._paths(self.batch_index, tab_featpaths)
        holder = {}
        dest = self._next_dest() if self._next_dest is not None else None
        unique, packed = self._unique, self._packed
        files = self._image_table(paths)[0] if unique else paths

        def work():
            try:
                if packed:
                    holder["feats"] = self._load_rows(files, D, W * H, dest, self.feat_type)
                else:
                    holder["feats"] = self._load_feats(files, D, W, H, dest, self.feat_type)
            except Exception as e:   # surfaced on the consumer side
                holder["error"] = e
        th = threading.Thread(target=work, daemon=True)
        th.start()
        self._job = ((self.batch_index, tuple(paths), unique, packed), th, holder)

    def next_batch_feat(self, tab_featpaths, feat_dim, feat_w=1, feat_h=1, unique=False, packed=False):
        """-> feats [B,D,W,H] (f32, or the 16-bit / fp8 feat_type), x [T,B] i32, x_len [B] i32, a [B] | [B,nMC] i32, qids [B].
        unique=True: every distinct feature file of the batch is read once, in order of first appearance;
        feats is that image table [N,D,W,H] and image_of [B] i32 (0-based table rows) is appended to the
        tuple: feats[image_of] is what unique=False returns.
        packed=True: the files are region files [n_boxes, D] (t7.load_regions), n_boxes <= feat_w * feat_h; every
        file is read once and the rows are concatenated without padding: -> rows [sum(counts), D], counts [B] (with
        unique=True: [N], per image), x, x_len, a, qids (and image_of).  feat16.unpack_regions(rows, counts, S) is
        the feats of the dense files of the same boxes; RAU.set_batch_packed / loader.feed take the tuple."""
        if isinstance(tab_featpaths, (str, os.PathLike)):
            tab_featpaths = [tab_featpaths]
        B = self.batch_size
        idx = self.batch_order[self.batch_index:self.batch_index + B]
        paths = self._paths(self.batch_index, tab_featpaths)
        files, image_of = self._image_table(paths) if unique else (paths, None)
        self._unique, self._packed = bool(unique), bool(packed)
        feats = None
        if self.opt_prefetch and self._job is not None:
            key, th, holder = self._job
            th.join()                                    # pool:synchronize()
            if "error" in holder:
                raise holder["error"]
            if key == (self.batch_index, tuple(paths), bool(unique), bool(packed)):
                feats = holder["feats"]
        if feats is None and packed:
            feats = self._load_rows(files, feat_dim, feat_w * feat_h, feat_type=self.feat_type)
        elif feats is None:
            feats = self._load_feats(files, feat_dim, feat_w, feat_h, feat_type=self.feat_type)
        x, x_len, a, qids = self._take(idx)
        if self.opt_prefetch:
            self._start_prefetch(tab_featpaths, feat_dim, feat_w, feat_h)
        head = feats if packed else (feats,)              # packed: (rows, counts)
        if unique:
            return (*head, x, x_len, a, qids, image_of)
        return (*head, x, x_len, a, qids)

    def _take(self, idx):
        """The question side of the batch `idx` (x, x_len, a, qids), and the step to the next batch."""
        B = self.batch_size
        x = np.ascontiguousarray(self.qs.question[idx].T, np.int32)          # transpose(1,2)
        x_len = np.ascontiguousarray(self.qs.lengths_q[idx], np.int32)
        qids = np.ascontiguousarray(self.qs.question_id[idx])
        src = self.qs.answers if self.split == "train" else self.qs.mc_ans
        a = np.ascontiguousarray(src[idx], np.int32)
        self.last_answers = None
        if self.qs.ans_ids is not None and self.qs.ans_w is not None:
            self.last_answers = (np.ascontiguousarray(self.qs.ans_ids[idx], np.int32),
                                 np.ascontiguousarray(self.qs.ans_w[idx], np.float32))
            if self.qs.ans_score is not None:
                self.last_answers += (np.ascontiguousarray(self.qs.ans_score[idx], np.float32),)
        self.last_regions = None
        if self.qs.img_regions is not None:              # per sample, whatever form the feats take
            self.last_regions = np.ascontiguousarray(
                np.asarray(self.qs.img_regions)[np.asarray(self.qs.img_list)[idx] - 1], np.int32)
        self.batch_index += B
        if self.batch_index + B > self.n:                # loader.lua:911-913
            self.reorder()
        return x, x_len, a, qids

    # ---- feature bank: every distinct image of the split lives in device memory, batches name rows
    def bank_rows(self, tab_featpaths):
        """-> (files, row_of): the split's distinct feature files in the order of their first question in
        the data set (independent of the batch order), and {file: bank row}."""
        if isinstance(tab_featpaths, (str, os.PathLike)):
            tab_featpaths = [tab_featpaths]
        key = tuple(str(p) for p in tab_featpaths)
        if self._bank is None or self._bank[0] != key:
            dt = self.qs.datatype if self.qs.datatype is not None else np.ones(self.n, int)
            row_of, files, qrow = {}, [], np.empty(self.n, np.int32)
            for i in range(self.n):
                p = os.path.join(key[int(dt[i]) - 1], feature_name(self.img_names[int(self.qs.img_list[i]) - 1]))
                if p not in row_of:
                    row_of[p] = len(files)
                    files.append(p)
                qrow[i] = row_of[p]
            self._bank = (key, files, row_of, qrow)
        return list(self._bank[1]), dict(self._bank[2])

    def fill_bank(self, rau, tab_featpaths, feat_dim, feat_w=1, feat_h=1, chunk=64, packed=False):
        """Reads every distinct feature file of the split ONCE and puts it into rau's bank at its
        bank_rows row, `chunk` files per rau.bank_put.  f32 files go up as f32 whatever the bank's type
        (a 16-bit or fp8 bank narrows them on the device: for fp8, round to nearest even, saturating at the
        largest finite value); HalfTensor files go into an fp16 bank as they are.
        -> number of rows written.
        packed=True: the files are region files [n_boxes, D]; they go up as packed rows (rau.bank_put_packed: no
        host transpose, no padding on the link) and the bank keeps the dense maps.  The bank stores no counts, so
        this also fills the QuestionSet's img_regions (one count per image of the name list, 1 where the split
        never asks about the image) and -> that array: next_batch_rows then leaves per-sample counts in
        last_regions, as for any QuestionSet with img_regions."""
        files, _ = self.bank_rows(tab_featpaths)
        info = rau.bank_info()
        if info["capacity"] < len(files):
            raise ValueError(f"bank of {info['capacity']} maps < {len(files)} distinct images")
        keep_half = info["feat_type"] == "f16"
        if packed:
            per_row = np.empty(len(files), np.int32)
            for r0 in range(0, len(files), max(int(chunk), 1)):
                maps = [t7.load_regions(p, feat_dim, keep_half) for p in files[r0:r0 + max(int(chunk), 1)]]
                half = all(m.dtype == np.float16 for m in maps)
                counts = np.array([m.shape[0] for m in maps], np.int32)
                rau.bank_put_packed(r0, np.concatenate([m if half else m.astype(np.float32) for m in maps]), counts)
                per_row[r0:r0 + len(maps)] = counts
            regions = np.ones(len(self.img_names), np.int32)
            regions[np.asarray(self.qs.img_list) - 1] = per_row[self._bank[3]]
            self.qs.img_regions = regions
            return regions
        for r0 in range(0, len(files), max(int(chunk), 1)):
            maps = [t7.load_feature(p, feat_dim, feat_w, feat_h, keep_half) for p in files[r0:r0 + max(int(chunk), 1)]]
            half = all(m.dtype == np.float16 for m in maps)
            rau.bank_put(r0, np.stack([m if half else m.astype(np.float32) for m in maps]))
        return len(files)

    def next_batch_rows(self, tab_featpaths):
        """-> rows [N] i32 (bank rows of the batch's distinct images, in order of first appearance),
        image_of [B] i32, x, x_len, a, qids: next_batch_feat(unique=True) with bank rows in place of the
        maps -- the same batches in the same order, epoch wrap included -- and no file access."""
        self.bank_rows(tab_featpaths)
        B = self.batch_size
        idx = self.batch_order[self.batch_index:self.batch_index + B]
        rows, first, image_of = np.unique(self._bank[3][idx], return_index=True, return_inverse=True)
        order = np.argsort(first, kind="stable")          # np.unique sorts by value: back to first appearance
        rank = np.empty_like(order)
        rank[order] = np.arange(len(order))
        x, x_len, a, qids = self._take(idx)
        return (np.ascontiguousarray(rows[order], np.int32), np.ascontiguousarray(rank[image_of.reshape(-1)], np.int32),
                x, x_len, a, qids)


class VqaData:
    """What ``vqa_prepro_loader.load_data`` returns: vocabulary + train / test iterators."""


def _read_questions(vqa_dir):
    h5 = os.path.join(vqa_dir, "data_prepro.h5")
    npz = os.path.join(vqa_dir, "data_prepro.npz")
    if os.path.exists(h5):
        try:
            import h5py   # not in the build image; used when present
        except ImportError as e:
            raise RuntimeError("data_prepro.h5 needs h5py, which is not installed; convert it to "
                               "data_prepro.npz with the same dataset names") from e
        with h5py.File(h5, "r") as f:
            return {k: np.asarray(f[k]) for k in f.keys()}
    with np.load(npz, allow_pickle=False) as f:
        return {k: f[k] for k in f.files}


def load_data(vqa_dir, batch_size, prefetch=False, test_batch_size=None, seed=123, feat_type="f32"):
    """loader.lua:1294-1473 (without the valid_ratio split); feat_type: element type of the
    feature maps the iterators return ("f32" | "f16" | "bf16" | "e4m3" | "e5m2"; fp8 maps are the files'
    values narrowed on the host, feat16.fp8_bits)."""
    with open(os.path.join(vqa_dir, "data_prepro.json")) as f:
        info = json.load(f)
    d = _read_questions(vqa_dir)
    one = lambda n: np.ones(n, np.int64)
    train = QuestionSet(question=d["ques_train"].astype(np.int32) + 1,     # zero padding -> 1
                        lengths_q=d["ques_length_train"], img_list=d["img_pos_train"],
                        question_id=d["question_id_train"], answers=d["answers"],
                        datatype=d.get("datatype_train", one(len(d["answers"]))))
    test = QuestionSet(question=d["ques_test"].astype(np.int32) + 1,
                       lengths_q=d["ques_length_test"], img_list=d["img_pos_test"],
                       question_id=d["question_id_test"], mc_ans=d["MC_ans_test"],
                       datatype=one(len(d["question_id_test"])))
    v = VqaData()
    as_list = lambda m: [m[k] for k in sorted(m, key=int)] if isinstance(m, dict) else list(m)
    v.img_train, v.img_test = as_list(info["unique_img_train"]), as_list(info["unique_img_test"])
    v.vocab_dict = {1: "ZEROPAD", **{int(i) + 1: w for i, w in info["ix_to_word"].items()}}
    v.vocab_map = {w: i for i, w in v.vocab_dict.items()}
    v.answer_dict = {int(i): w for i, w in info["ix_to_ans"].items()}
    v.answer_map = {w: i for i, w in v.answer_dict.items()}
    v.vocab_size = len(info["ix_to_word"]) + 1            # including ZEROPAD
    v.answer_size = len(info["ix_to_ans"])
    v.seq_len = v.max_sentence_len = int(train.question.shape[1])
    v.train_data = DataClass(train, v.img_train, batch_size, "train", prefetch, seed, feat_type)
    v.test_data = DataClass(test, v.img_test, test_batch_size or batch_size, "test", prefetch, seed,
                            feat_type)
    return v


def feed(rau, batch, feat_type=None, answers=None, regions=None, att_targets=None, sample_w=None, candidates=None):
    """next_batch_feat's tuple -> rau_set_batch (the H2D of SS:434-439); returns qids.
    feat_type: that of the feats (needed for bf16 and fp8, which arrive as uint16 / uint8 bits).  A tuple of
    next_batch_feat(unique=True) goes up as an image table, one of next_batch_rows as a bank batch, one of
    next_batch_feat(packed=True) as packed region rows (set_batch_packed: its counts are the batch's regions).
    The batch may be smaller than the context's capacity (a test split at test_batch_size): set_batch
    takes the size from x_len and switches the context to it.
    answers = (ids, w[, score]) rows of the batch (DataClass.last_answers, when its QuestionSet has ans_ids /
    ans_w): attached with rau.set_answers once the batch is up; None changes nothing.
    regions = per-sample region counts [B] of the batch (DataClass.last_regions, when its QuestionSet has
    img_regions): attached with rau.set_regions once the batch is up; None changes nothing.
    A batch given as a dict (the keyword arguments of RAU.set_batch: feats, tokens, lens, labels and optionally
    image_of, bank_rows, answers, regions, qids) goes to set_batch as it is: its "regions" key is per sample, or
    per image beside image_of / bank_rows; the regions= argument, when given, replaces it.
    att_targets = per-sample attention target maps [B, S] of the batch (human attention maps, boxes rendered onto
    the positions): attached with rau.set_att_targets once the batch is up; None changes nothing.  For a dict it
    replaces the dict's own "att_targets" key.
    sample_w = per-sample loss weights [B] of the batch (class- or question-type balancing, importance weights):
    attached with rau.set_sample_weights once the batch is up; None changes nothing.  For a dict it replaces the
    dict's own "sample_w" key.
    candidates = per-sample multiple-choice candidates [B, C] of the batch (VQA v1's 18 choices): attached with
    rau.set_candidates once the batch is up; None changes nothing.  For a dict it replaces the dict's own
    "candidates" key."""
    if isinstance(batch, dict):
        kw = {k: v for k, v in batch.items() if k != "qids"}
        if feat_type is not None:
            kw["feat_type"] = feat_type
        if answers is not None:
            kw["answers"] = answers
        if regions is not None:
            kw.pop("regions", None)
        if att_targets is not None:
            kw.pop("att_targets", None)
        if sample_w is not None:
            kw.pop("sample_w", None)
        if candidates is not None:
            kw.pop("candidates", None)
        rau.set_batch(**kw)
        qids = batch.get("qids")
    else:
        qids = _feed_batch(rau, batch, feat_type)
        if answers is not None:
            rau.set_answers(*answers)
    if regions is not None:
        rau.set_regions(regions)
    if att_targets is not None:
        rau.set_att_targets(att_targets)
    if sample_w is not None:
        rau.set_sample_weights(sample_w)
    if candidates is not None:
        rau.set_candidates(candidates)
    return qids


def _feed_batch(rau, batch, feat_type):
    if batch[0].ndim == 1:                                # next_batch_rows: rows, image_of, x, x_len, a, qids
        rows, image_of, x, x_len, a, qids = batch
        rau.set_batch(None, x, x_len, a if a.ndim == 1 else None, bank_rows=rows, image_of=image_of)
        return qids
    if batch[0].ndim == 2:                                # next_batch_feat(packed=True): rows, counts, x, x_len, a, qids
        rows, counts, x, x_len, a, qids = batch[:6]
        rau.set_batch_packed(rows, counts, x, x_len, a if a.ndim == 1 else None, feat_type=feat_type,
                             image_of=batch[6] if len(batch) > 6 else None)
        return qids
    feats, x, x_len, a, qids = batch[:5]
    image_of = batch[5] if len(batch) > 5 else None
    B, D = feats.shape[0], feats.shape[1]                 # (image table: B is its number of maps)
    labels = a if a.ndim == 1 else None                   # test batches carry MC ids, no labels
    rau.set_batch(feats.reshape(B, D, -1), x, x_len, labels, feat_type=feat_type, image_of=image_of)
    return qids


class SlotFeeder:
    """The loader's prefetch joined to the ctx's two upload slots (rau_batch_slot /
    rau_set_batch_async / rau_use_batch): what SS:434-439 + vqa_prepro_loader.lua:931-958 do every
    iteration, without a host copy or a host wait on the step's path.

    The prefetch worker reads the NEXT batch's feature files straight into the pinned staging of
    the slot the device is not using; ``next()`` (called right after the current step has been
    enqueued) hands that slot to the copy stream -- the 100 MB transfer runs under the step still
    executing -- makes it the resident batch for the following step, and points the worker at the
    slot just left.  Usage::

        feeder = SlotFeeder(rau, data, featdir, D, W, H)      # batch 0 resident on return
        for it in range(n):
            rau.forward(); rau.backward(w); ...              # enqueue step `it`
            qids = feeder.next()                              # batch it+1 resident for the next step

    sample_w: a callable qids -> per-sample loss weights [B] (None: no weights); the weights go up behind every
    batch's upload, on the copy stream (rau.set_sample_weights(slot=)).
    candidates: a callable qids -> multiple-choice candidates [B, C] (None: none); they go up the same way
    (rau.set_candidates(slot=)).

    A feeder is BOUND to one batch size, the DataClass's: if the context runs another size when the
    feeder is made (a test split at test_batch_size below the capacity) it is switched first
    (rau.set_batch_size), and a feeder whose context has been switched since refuses to go on -- the
    switch dropped the slots it had filled.  Make a new feeder after every set_batch_size.
    """

    def __init__(self, rau, data: DataClass, tab_featpaths, feat_dim, feat_w=1, feat_h=1,
                 feat_type=None, share_images=False, bank=False, packed=False, sample_w=None,
                 candidates=None):
        self.rau, self.data = rau, data
        self.sample_w = sample_w
        self.candidates = candidates
        self.n = int(data.batch_size)
        if getattr(rau, "batch_size", self.n) != self.n:
            rau.set_batch_size(self.n)     # raises above the capacity
        # bank=True: the maps are in rau's feature bank (DataClass.fill_bank); a batch is next_batch_rows' tuple,
        # there is no prefetch worker and nothing is written to the slots' feature staging
        self.bank = bool(bank)
        # every distinct image of a batch is read, staged and uploaded once (next_batch_feat(unique=True));
        # the worker fills the first N maps of the slot's staging
        self.share_images = bool(share_images)
        # packed=True: the files are region files [n_boxes, D]; the worker concatenates their rows at the start of
        # the slot's staging (no transpose, no padding) and the device unpacks them (rau_set_batch_async_packed)
        self.packed = bool(packed)
        if self.packed and self.bank:
            raise ValueError("a bank feeder has no feature staging to pack (fill_bank(packed=True) fills the bank)")
        self.args = (tab_featpaths, feat_dim, feat_w, feat_h)
        self.slot = 0                  # the slot the NEXT batch is assembled in
        # element type of the maps in the staging and on the wire (default: the DataClass's)
        self.feat_type = data.feat_type = feat16.check_name(feat_type or data.feat_type)
        self._ft = {} if self.feat_type == "f32" else {"feat_type": self.feat_type}   # f32: the plain calls
        data.opt_prefetch = not self.bank
        data._job = None               # any batch prefetched before now went to ordinary memory
        data._next_dest = lambda: self.rau.batch_slot(self.slot, **self._ft)["feats"]
        self.qids = self._advance()    # batch 0: read synchronously (nothing to overlap with yet)

    def _advance(self):
        d, rau, s = self.data, self.rau, self.slot
        if getattr(rau, "batch_size", self.n) != self.n:
            raise RuntimeError(f"this SlotFeeder feeds batches of {self.n}; the context now runs "
                               f"{rau.batch_size}: make a new feeder after set_batch_size")
        view = rau.batch_slot(s, **self._ft)          # (host-waits until the slot's last upload has left)
        self.slot = s ^ 1                             # the worker started by next_batch_feat fills the other
        if self.bank:
            rows, image_of, x, x_len, a, qids = d.next_batch_rows(self.args[0])
            view["tokens"][...] = x
            view["lens"][...] = x_len
            labels = a.ndim == 1
            if labels:
                view["labels"][...] = a
            rau.set_batch_async(s, has_labels=labels, bank_rows=rows, image_of=image_of)
            if d.last_answers is not None:
                rau.set_answers(*d.last_answers, slot=s)
            if d.last_regions is not None:
                rau.set_regions(d.last_regions, slot=s)
            if self.sample_w is not None:
                rau.set_sample_weights(self.sample_w(qids), slot=s)
            if self.candidates is not None:
                rau.set_candidates(self.candidates(qids), slot=s)
            rau.use_batch(s)
            return qids
        batch = d.next_batch_feat(*self.args, unique=self.share_images, packed=self.packed)
        if self.packed:
            feats, counts, x, x_len, a, qids = batch[:6]
            table = {"packed_counts": counts}
            if self.share_images:
                table["image_of"] = batch[6]
        else:
            feats, x, x_len, a, qids = batch[:5]
            table = {"image_of": batch[5], "n_images": feats.shape[0]} if self.share_images else {}
        if not np.shares_memory(feats, view["feats"]):   # first batch / a re-drawn order: not prefetched in place
            stage = view["feats"].reshape(-1)[:feats.size]
            feat16.store(stage, feats.reshape(stage.shape), self.feat_type)
        view["tokens"][...] = x
        view["lens"][...] = x_len
        labels = a.ndim == 1                          # test batches carry MC ids, no labels
        if labels:
            view["labels"][...] = a
        rau.set_batch_async(s, has_labels=labels, **table, **self._ft)   # staging filled in place: no host copy
        if d.last_answers is not None:                # the QuestionSet carries answer sets: behind the upload
            rau.set_answers(*d.last_answers, slot=s)
        if d.last_regions is not None and not self.packed:   # ... and region counts: per sample, also for an image
            rau.set_regions(d.last_regions, slot=s)          # table (a packed batch brought its own)
        if self.sample_w is not None:                 # ... and per-sample loss weights, looked up by question id
            rau.set_sample_weights(self.sample_w(qids), slot=s)
        if self.candidates is not None:               # ... and multiple-choice candidates, the same way
            rau.set_candidates(self.candidates(qids), slot=s)
        rau.use_batch(s)
        return qids

    def next(self):
        """Upload the prefetched batch and make it resident; returns its question ids."""
        self.qids = self._advance()
        return self.qids
