"""The update of rau_update stated in fp64 numpy: gradient noise (given as an array of normals), the
norm clip in both scopes, and both rules.  What tests/test_update_rules_host.py pins to torch's Adamax and to
tests/test_update.py's adam_ref, and what tests/test_gpu_update_rules.py holds the device to."""
import numpy as np

GROUPS = ("embed", "rnn", "mult")


def clip_scale(norm, clip):
    """The project's form: norm > clip ? clip / norm : 1 (not torch's clip / (norm + 1e-6))."""
    return clip / norm if norm > clip else 1.0


def adam_elem(x, g, m, v, t, lr, b1, b2, eps):
    m = m * b1 + (1 - b1) * g
    v = v * b2 + (1 - b2) * g * g
    step = lr * np.sqrt(1 - b2 ** t) / (1 - b1 ** t)
    return x - step * m / (np.sqrt(v) + eps), m, v            # eps OUTSIDE the sqrt


def adamax_elem(x, g, m, u, t, lr, b1, b2, eps):
    """torch.optim.Adamax: u is the exponentially weighted infinity norm, u0 = 0."""
    m = m * b1 + (1 - b1) * g
    u = np.maximum(b2 * u, np.abs(g) + eps)
    return x - (lr / (1 - b1 ** t)) * m / u, m, u


def update(x, g, m, v, t, step_t, noise=None, rule="adam", clip_scope="group", lr=3e-3, mult_lr=3e-4,
           b1=0.9, b2=0.999, eps=1e-8, eta=0.01, gamma=0.55, clip=0.1):
    """One update of the three groups.  x, g, m, v, noise: {group: fp64 vector} (noise: standard normals, or None
    for eta = 0); t: {group: update count AFTER this update}.  Returns (x, g_clipped, m, v, norms[4]): the group
    norms and the global norm sqrt(s_embed + s_rnn + s_mult), all pre-clip."""
    elem = {"adam": adam_elem, "adamax": adamax_elem}[rule]
    gn = {}
    for k in GROUPS:
        gk = np.asarray(g[k], np.float64)
        if noise is not None and eta > 0:
            gk = gk + noise[k] * np.sqrt(eta / ((step_t + 1) * gamma))   # gamma multiplies (SS:598)
        gn[k] = gk
    sq = [float(np.sum(gn[k] * gn[k])) for k in GROUPS]
    norms = [np.sqrt(s) for s in sq] + [np.sqrt(sq[0] + sq[1] + sq[2])]
    xo, go, mo, vo = {}, {}, {}, {}
    for i, k in enumerate(GROUPS):
        sc = clip_scale(norms[3] if clip_scope == "global" else norms[i], clip)
        go[k] = gn[k] * sc
        xo[k], mo[k], vo[k] = elem(np.asarray(x[k], np.float64), go[k], np.asarray(m[k], np.float64),
                                   np.asarray(v[k], np.float64), t[k], mult_lr if k == "mult" else lr,
                                   b1, b2, eps)
    return xo, go, mo, vo, np.array(norms)
