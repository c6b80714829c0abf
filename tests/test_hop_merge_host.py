"""joint.feval_stats: the host restatement of feval's joint-loss bookkeeping (SS:476-556) on
hand-built cases, and tied to the oracle through the committed fixtures."""
import glob
import os

import numpy as np
import pytest

from rau_vqa_amd import joint

HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURES = sorted(glob.glob(os.path.join(HERE, "golden", "*.npz")))


def ce_rows(pred, y):
    p = np.asarray(pred, np.float64)
    mx = p.max(1)
    return mx + np.log(np.exp(p - mx[:, None]).sum(1)) - p[np.arange(len(y)), y - 1]


def case(H=3, B=6, K=5, seed=0):
    rng = np.random.default_rng(seed)
    logits = rng.standard_normal((H, B, K)).astype(np.float32)
    dopred = rng.random((H, B)).astype(np.float32)
    labels = rng.integers(1, K + 1, size=B).astype(np.int32)
    return logits, dopred, labels


def test_first_max_ties_decide_answers_and_correct_counts():
    logits, dopred, labels = case()
    logits[0, 0] = [1, 3, 3, 0, 3]            # tie: index 2 (1-based) wins
    labels[0] = 2
    logits[0, 1] = [3, 3, 0, 0, 0]
    labels[1] = 2                              # the tie goes to answer 1: not correct
    s = joint.feval_stats(logits, dopred, labels)
    ans0 = np.argmax(logits[0], 1) + 1
    assert s["correct"][0] == int((ans0 == labels).sum())
    assert ans0[0] == 2 and ans0[1] == 1
    uni = logits.sum(0) / np.float32(3)
    assert np.array_equal(s["uni_ans"], np.argmax(uni, 1) + 1)
    assert s["correct"][3] == int((s["uni_ans"] == labels).sum())


def test_no_hop_fires_select_row_is_zero():
    logits, dopred, labels = case(K=7)
    dopred[:] = 0.5                            # strict > 0.5: nothing fires
    s = joint.feval_stats(logits, dopred, labels)
    H = 3
    assert np.all(s["fired"] == 0) and np.all(s["selected"] == 0)
    assert np.all(s["select_ans"] == 1)        # all-zero row: first max = answer 1
    assert s["loss"][H + 1] == pytest.approx(np.log(7), rel=1e-6)
    assert s["correct"][H + 1] == int((labels == 1).sum())


def test_every_hop_fires_select_is_hop_one():
    logits, dopred, labels = case(B=9, seed=4)
    dopred[:] = 0.75
    s = joint.feval_stats(logits, dopred, labels)
    assert list(s["selected"]) == [9, 0, 0] and list(s["fired"]) == [9, 9, 9]
    assert np.array_equal(s["select_ans"], np.argmax(logits[0], 1) + 1)
    assert s["loss"][4] == s["loss"][0]        # the select row IS hop 1's logits
    assert s["loss"][0] == pytest.approx(ce_rows(logits[0], labels).mean(), rel=1e-6)


def test_last_hop_is_not_forced_and_first_firing_hop_is_selected():
    logits, dopred, labels = case(B=4, seed=2)
    dopred[:] = 0.1
    dopred[1, 0] = dopred[2, 0] = 0.9          # sample 0: hop 2 first
    dopred[2, 1] = 0.9                         # sample 1: hop 3
    s = joint.feval_stats(logits, dopred, labels)
    assert list(s["selected"]) == [0, 1, 1]
    sel = np.zeros((4, logits.shape[2]), np.float32)
    sel[0], sel[1] = logits[1, 0], logits[2, 1]
    assert s["loss"][4] == pytest.approx(ce_rows(sel, labels).mean(), rel=1e-6)


def test_bce_eps_term_at_exactly_zero_and_one():
    H, B, K = 2, 4, 3
    logits = np.zeros((H, B, K), np.float32)
    logits[:, :, 0] = 1.0                      # every hop answers 1
    labels = np.array([1, 1, 2, 2], np.int32)  # gt = 1, 1, 0, 0
    dopred = np.array([[1.0, 0.0, 1.0, 0.0], [0.25, 0.75, 0.5, 1.0]], np.float32)
    s = joint.feval_stats(logits, dopred, labels)
    big = -np.log(np.float32(1e-12))           # log(0 + eps)
    want0 = (0.0 + big + big + 0.0) / 4        # x=1,t=1 | x=0,t=1 | x=1,t=0 | x=0,t=0
    assert s["loss_do_pred"][0] == pytest.approx(want0, rel=1e-6)
    want1 = (-np.log(0.25) - np.log(0.75) - np.log(0.5) + big) / 4
    assert s["loss_do_pred"][1] == pytest.approx(want1, rel=1e-6)
    assert np.all(np.isfinite(s["loss_do_pred"]))


def test_do_pred_accuracy_is_masked_by_did_correct():
    H, B, K = 2, 4, 3
    logits = np.zeros((H, B, K), np.float32)
    logits[0, :, 0] = 1.0                      # hop 1 answers 1
    logits[1, :, 1] = 1.0                      # hop 2 answers 2
    labels = np.array([1, 2, 3, 3], np.int32)  # did_correct = 1, 1, 0, 0
    dopred = np.array([[0.9, 0.9, 0.1, 0.9], [0.1, 0.9, 0.9, 0.1]], np.float32)
    s = joint.feval_stats(logits, dopred, labels)
    assert s["did_correct"] == 2
    # hop 1 gt = 1,0,0,0: agree on sample 0 only (among the did_correct ones); hop 2 gt = 0,1,0,0: both
    assert list(s["do_pred_correct"]) == [1, 2]
    assert list(s["correct"][:2]) == [1, 1]


def test_single_hop():
    logits, dopred, labels = case(H=1, B=5, K=4, seed=7)
    dopred[0] = [0.9, 0.2, 0.9, 0.2, 0.9]
    s = joint.feval_stats(logits, dopred, labels)
    assert s["loss"].shape == (3,) and s["loss_do_pred"].shape == (1,)
    assert s["loss"][1] == s["loss"][0]        # uni of one hop = l / 1
    assert list(s["selected"]) == [3]
    for k in ("correct", "do_pred_correct", "fired", "selected"):
        assert s[k].dtype == np.int32


@pytest.mark.parametrize("path", FIXTURES, ids=[os.path.basename(p) for p in FIXTURES])
def test_per_hop_losses_match_the_oracle_fixtures(path):
    z = np.load(path, allow_pickle=False)
    H = z["o_logits"].shape[0]
    s = joint.feval_stats(z["o_logits"], z["o_dopred"], z["in_labels"])
    rel = np.max(np.abs(s["loss"][:H] - z["o_losses"])) / np.max(np.abs(z["o_losses"]))
    assert rel < 1e-6
    assert s["loss"].shape == (H + 2,) and s["loss_do_pred"].shape == (H,)
