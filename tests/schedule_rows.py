"""The step path's launch sequences, one row per arm of its image, encoder, head-gradient and weight-gradient
units.  Run as its own process by tests/test_gpu_schedule.py (librau reads several A/B variables once per process)
with RAU_PROF_TIMELINE set: prof_collect then appends one `class,stream,start,end` line per launch in host enqueue
order.  Prints the sequences as one JSON line (encode() below); `python tests/schedule_rows.py record [path]` writes
it to tests/golden/step_schedule.json (or path) instead: to be run on a build of the commit BEFORE a change of the
step path, never on the code under test."""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import util  # noqa: E402

FIXTURE = os.path.join(ROOT, "tests", "golden", "step_schedule.json")
CFG_KEYS = ("B", "T", "V", "E", "Rq", "D", "S", "M", "A", "R", "K", "H")
# the dims of tests/knob_check.py: "" generic, "bf16" (wgrad16.hip / dgrad16.hip widths; 72 samples here, because up
# to 64 take the split attention kernels, which leave dS in f32), "ws" (enc_ws.hip's Rq)
GENERIC = dict(T=7, V=120, E=200, Rq=64, D=64, S=196, M=128, A=64, R=64, K=1000, H=4)
BF16 = dict(B=72, T=5, V=60, E=64, Rq=64, D=256, S=196, M=256, A=64, R=64, K=200, H=3)
WS = dict(B=32, T=6, V=120, E=200, Rq=512, D=64, S=196, M=128, A=64, R=64, K=200, H=2)


def f32(a):
    return np.asarray(a, np.float32)


def model(dims, dtype="f32", mode="train", tied=False, **batch_kw):
    """A context at `dims` with seeded parameters and masks and its batch resident."""
    from rau_vqa_amd.model import RAU, Config
    sh = util.shapes(dims)
    batch, params, _ = util.make_problem(sh, scale=0.3)
    m = RAU(Config(**{k: getattr(sh, k) for k in CFG_KEYS}, dtype=dtype))
    m.set_params(params)
    m.training() if mode == "train" else m.evaluate()
    if tied:
        m.tie_feature_dropout()
    m.set_dropout_seed(11, 2)
    m.set_batch(**dict(batch, **batch_kw))
    return m, sh, batch


def traced(m, fn):
    """The (class, stream) pairs of the launches fn() enqueues."""
    path = os.environ["RAU_PROF_TIMELINE"]
    open(path, "w").close()
    m.prof_enable(True)
    fn()
    m.prof()            # collects: the timeline is written here
    m.prof_enable(False)
    with open(path) as f:
        rows = [ln.split(",") for ln in f.read().split("\n") if ln and ln != "#"]
    return [[r[0], int(r[1])] for r in rows]


def step(m, hop_w, backward=True, **loss):
    def fn():
        m.zero_grads()
        m.forward()
        if backward:
            m.backward(f32(hop_w), **loss)
    return fn


def run_step(dims, hop_w=None, backward=True, loss=None, **kw):
    m, sh, _ = model(dims, **kw)
    seq = traced(m, step(m, hop_w if hop_w is not None else [sh.H] * sh.H, backward, **(loss or {})))
    m.close()
    return seq


def captured():
    """rau_graph_step refuses to run with the profile on, so a captured step has no timeline.  The row runs one, then
    the same step eagerly on the same context with the profile on: the sequence is that eager step's (the first
    behind a graph launch), and the captured step's results must equal it bit for bit."""
    m, sh, _ = model(util.SMALL)
    hop_w = f32([sh.H] * sh.H)

    def results():
        g = m.get_grads()
        return [m.losses(), m.logits(), g["embed"], g["rnn"], g["mult"]]
    m.graph_step(hop_w)
    graph = results()
    m.set_dropout_seed(11, 2)
    seq = traced(m, step(m, hop_w))
    for a, b in zip(graph, results()):
        assert np.array_equal(a, b) and np.any(a), "captured step differs from the eager step"
    m.close()
    return seq


def external():
    import torch
    m, sh, _ = model(util.SMALL)
    rng = np.random.default_rng(9)
    og = {k: torch.as_tensor(rng.standard_normal(s).astype(np.float32) * 0.1).cuda()
          for k, s in (("logits", (sh.H, sh.B, sh.K)), ("dopred", (sh.H, sh.B)), ("attprob", (sh.H, sh.B, sh.S)))}
    torch.cuda.synchronize()
    seq = traced(m, step(m, [1.0] * sh.H, out_grads=og))
    m.close()
    return seq


def multimodal():
    import torch
    from rau_vqa_amd import modules
    m, sh, batch = model(util.SMALL)
    rng = np.random.default_rng(5)
    cu = lambda *s: torch.as_tensor(rng.standard_normal(s).astype(np.float32) * 0.3).cuda()  # noqa: E731
    args = [cu(sh.B, sh.Q), torch.as_tensor(batch["feats"]).cuda(), cu(sh.B, sh.R), cu(sh.B, sh.R)]
    d_logits = cu(sh.B, sh.K)
    torch.cuda.synchronize()
    clone = modules.MultimodalClone(m, 1)

    def fn():
        m.zero_grads()
        clone.forward(*args)
        clone.backward(*args, d_logits)
    seq = traced(m, fn)
    m.close()
    return seq


def table_batch():
    sh = util.shapes(util.SMALL)
    batch, _, _ = util.make_problem(sh, scale=0.3)
    image_of = np.array([0, 1, 1, 2, 0, 3, 3, 3], np.int32)
    return dict(feats=np.ascontiguousarray(batch["feats"][:4]), image_of=image_of)


def att_targets():
    sh = util.shapes(util.SMALL)
    return np.random.default_rng(4).random((sh.B, sh.S)).astype(np.float32)


ROWS = {
    "f32-train": lambda: run_step(util.SMALL),
    "tied-train": lambda: run_step(util.SMALL, tied=True),
    "eval-forward": lambda: run_step(util.SMALL, backward=False, mode="eval"),
    "eval-forward-backward": lambda: run_step(util.SMALL, mode="eval"),
    "eval-table-forward": lambda: run_step(util.SMALL, backward=False, mode="eval", **table_batch()),
    "captured": captured,
    "select_w": lambda: run_step(util.SMALL, loss=dict(select_w=f32([0.5, 1.0, 0.25]))),
    "att_w": lambda: run_step(util.SMALL, loss=dict(att_w=f32([0.3, 0.0, 0.7])), att_targets=att_targets()),
    "ext": external,
    "generic-B72": lambda: run_step(dict(GENERIC, B=72)),
    "generic-B24": lambda: run_step(dict(GENERIC, B=24)),
    "bf16-tiles": lambda: run_step(BF16, dtype="bf16"),
    "ws-train": lambda: run_step(WS),
    "ws-eval-forward": lambda: run_step(WS, backward=False, mode="eval"),
    "multimodal": multimodal,
}


def encode(seqs):
    """{"classes": [names], "rows": {row: "c.s c.s ..."}}: launch = index into classes, dot, stream."""
    classes = sorted({c for seq in seqs.values() for c, _ in seq})
    at = {c: i for i, c in enumerate(classes)}
    return {"classes": classes, "rows": {k: " ".join(f"{at[c]}.{s}" for c, s in seq) for k, seq in seqs.items()}}


def decode(doc):
    names = doc["classes"]
    return {k: [(names[int(c)], int(s)) for c, s in (tok.split(".") for tok in row.split())]
            for k, row in doc["rows"].items()}


if __name__ == "__main__":
    text = json.dumps(encode({name: row() for name, row in ROWS.items()}), separators=(",", ":"))
    if sys.argv[1:2] == ["record"]:
        with open(sys.argv[2] if len(sys.argv) > 2 else FIXTURE, "w") as f:
            f.write(text + "\n")
        print("recorded", len(text), "bytes")
    else:
        print(text)
