"""The step path enqueues what it enqueued before its image, encoder, head-gradient and weight-gradient passes became
named units: per row, the (kernel class, stream) sequence of one step in host enqueue order equals
tests/golden/step_schedule.json, which tests/schedule_rows.py recorded on a build of the commit before that change.
One child process runs every row (several A/B variables are read once per process; none is set here but the
timeline path).  The arm of the moved code each row reaches:

  f32-train              util.SMALL, train: feature_maps with the generating dropout pass, image_forward and the
                         per-hop-group conv_grads (8 samples: one group per direction; S = 12: the plain dgrad,
                         dzf = 0), forward_heads with head_dgrad on the side stream, scale_hops3, mult_wgrads /
                         enc_wgrads on the side stream
  tied-train             ... under tie_feature_dropout: one masked copy, one conv group, hop_sum + conv_grads with
                         outer_sum between the dgrad and the weight gradients
  eval-forward           evaluate mode: no mask, the convs read the batch itself, one group, no head_dgrad
  eval-forward-backward  ... and the backward's loop over hops on the shared I (conv_grads once per hop), head_dgrad
                         on the chain stream
  eval-table-forward     evaluate-mode forward of an image-table batch: the image side runs on 4 maps for 8 samples
  captured               the eager step behind a captured one on the same context (rau_graph_step refuses to run with
                         the profile on, so a captured step has no timeline; the child asserts the captured step's
                         losses, logits and gradients equal the eager step's bit for bit)
  select_w, att_w, ext   loss_gradients' arms: select_signal / att_sup_grad / ext_dl + ext_signal + ext_da, head_dgrad
                         with the addend in the backward, select_wgrad in mult_wgrads
  generic-B72            knob_check.py's generic dims above the 64-sample switch: three launch groups per direction, no
                         side split, wg_bulk = 1 (mult_wgrads at the end of the bulk stream), S = 196: the fused dZ
                         dgrad (dzf = 1) and the last group's colsum
  generic-B24            ... below it: one group, side split (encoder input projection in chunks and q_proj rows of
                         hops 1.. on the side stream), wg_bulk = 0
  bf16-tiles             knob_check.py's "bf16" dims in bf16 mode at 72 samples (up to 64 take the split attention
                         kernels, which leave dS in f32): bf16 hop copies (x16), bf16 dS, bf16 dZ, dzf = 1, three
                         groups with the side split: q_proj_dgrad of the finished groups on the side stream
  ws-train, ws-eval-forward   knob_check.py's "ws" dims: encoder_forward's persistent-encoder arm where the shape selects it
  multimodal             one rau_multimodal_forward / rau_multimodal_backward pair: image_forward and conv_grads on the
                         chain stream
"""
import json
import os
import subprocess
import sys

import pytest

from tests import schedule_rows

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def sequences(tmp_path_factory):
    env = {k: v for k, v in os.environ.items() if not k.startswith("RAU_")}
    env["RAU_PROF_TIMELINE"] = str(tmp_path_factory.mktemp("schedule") / "timeline.csv")
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "schedule_rows.py")], env=env, cwd=ROOT,
                         capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-3000:]
    return schedule_rows.decode(json.loads(out.stdout.strip().splitlines()[-1]))


@pytest.fixture(scope="module")
def recorded():
    with open(schedule_rows.FIXTURE) as f:
        return schedule_rows.decode(json.load(f))


def test_fixture_has_every_row(recorded):
    assert sorted(recorded) == sorted(schedule_rows.ROWS)
    assert os.path.getsize(schedule_rows.FIXTURE) < 64 * 1024


@pytest.mark.parametrize("row", list(schedule_rows.ROWS))
def test_step_enqueues_the_recorded_sequence(row, sequences, recorded):
    got, want = sequences[row], recorded[row]
    assert len(want) > 0
    first = next((i for i, (a, b) in enumerate(zip(got, want)) if a != b), min(len(got), len(want)))
    assert got == want, (f"{row}: {len(got)} launches against {len(want)} recorded; first difference at launch {first}: "
                         f"{got[first:first + 3]} against {want[first:first + 3]}")
