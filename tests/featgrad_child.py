"""One step with the feature-map gradient on, run as its own process by tests/test_gpu_featgrad.py: one setting of
RAU_XGRAD_FUSED the way a user sets an A/B variable, before the process creates its context.  The named problem under its
explicit masks, dX saved to the given .npy file."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

from tests.test_gpu_featgrad import HOP_W, dev_step, make_model, problem, put

name, out = sys.argv[1], sys.argv[2]
sh, batch, params, masks = problem(name)
m = make_model(sh, params, masks)
m.want_feature_grad()
put(m, batch)
m.prof_enable()
dX, _ = dev_step(m, HOP_W)
launches = {n: v["launches"] for n, v in m.prof().items() if v["launches"]}
m.close()
np.save(out, dX)
print("launches", launches.get("conv_embed_dgrad", 0), launches.get("xgrad_accum", 0))
print("OK")
