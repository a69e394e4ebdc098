"""The kernel cases of the object layers (tests/test_layers_kernel.py) and their generator (no GPU import: tests/test_layers_ref.py
holds the same inputs against the cap on near-threshold decisions).

A lane's particles are jittered copies of a base scene (sigma 0.02 / 0.15 / 0.5 in logit units: all agree / the threshold cuts
through them / few agree) with random presence -- lanes without an object and lanes with all N among them -- and the weight patterns
of tests/test_estimate_kernel.py (random, equal, dominant, spread, neg_inf), then a NaN lane, a +inf lane and an all -inf lane.  The
scale logits lie around -1 on the 50 x 50 and 70 x 70 frames (boxes of about a quarter of the frame) and around 3 on the small ones
(boxes larger than the frame); glimpses are 0.3 N(0, 1), the magnitude tests/test_hip_kernels.py::test_st_insert_loglik gates the
decoder's canvas at."""
from collections import namedtuple

import numpy as np

PATTERNS = ("random", "equal", "dominant", "spread", "neg_inf")
SIGMAS = (0.02, 0.15, 0.5)
CELLS = [(PATTERNS[i % 5], SIGMAS[i % 3]) for i in range(15)]   # every (pattern, sigma) once, mixed from the first lane on
IOU_MIN = 0.5
COVER_MIN = 0.5
TOL = 2e-5      # absolute, on layer and cover: the decoder's own gate in test_st_insert_loglik at the same glimpse magnitude

Case = namedtuple("Case", "K T N wide hw G lanes seed")
# (K, T, N, library, H x W, G) as the issue lists them; `lanes` finite lanes (+ 3 non-finite ones: 11 to 48 in all), `seed` chosen
# in tests/test_layers_ref.py's count of near-threshold decisions
CASES = [
    Case(1, 1, 4, False, (50, 50), 20, 45, 1),      # a single particle
    Case(2, 3, 4, False, (50, 50), 20, 30, 2),      # prefix weights over frames
    Case(5, 1, 4, False, (50, 50), 20, 45, 3),
    Case(64, 1, 4, False, (12, 9), 20, 15, 4),      # boxes larger than the frame
    Case(65, 1, 4, False, (12, 9), 5, 15, 5),       # a wave boundary
    Case(256, 1, 4, False, (12, 9), 5, 8, 6),
    Case(3, 1, 4, False, (10, 130), 20, 45, 7),     # wider than a wavefront
    Case(5, 1, 4, False, (70, 70), 20, 30, 8),      # several pixel tiles, H * W a multiple of nothing
    Case(5, 1, 14, True, (20, 16), 8, 30, 9),       # the wide build's N = 14
]


def case_id(c):
    return "K{}_T{}_N{}_{}x{}_G{}{}".format(c.K, c.T, c.N, c.hw[0], c.hw[1], c.G, "_wide" if c.wide else "")


def make(c):
    """glimpse [T, R, N, G, G], where [T, R, N, 4], presence [T, R, N], lw0 [R], lw [T, R] (float32) and the lanes' pattern names;
    the last three lanes are the non-finite ones."""
    K, T, N, G = c.K, c.T, c.N, c.G
    rng = np.random.default_rng(c.seed)
    B = c.lanes + 3
    cells = [CELLS[i % len(CELLS)] for i in range(c.lanes)]
    sig = np.array([s for _, s in cells] + [0.15] * 3)
    names = [p for p, _ in cells] + ["nan", "pos_inf", "all_neg_inf"]
    base = rng.standard_normal((T, B, 1, N, 4))
    base[..., :2] = base[..., :2] * 0.7 + (-1.0 if min(c.hw) >= 50 else 3.0)
    where = (base + sig[None, :, None, None, None] * rng.standard_normal((T, B, K, N, 4))).astype(np.float32)
    n_obj = rng.integers(0, N + 1, size=(T, B))
    n_obj[:, 0::7] = 0          # lanes with no object in the base scene ...
    n_obj[:, 1::7] = N          # ... and with all N
    base_p = np.arange(N)[None, None, :] < n_obj[..., None]
    flip = rng.uniform(size=(T, B, K, N)) < 0.15                          # particles disagree on the count, holes included
    flip[:, 0::7] = False
    flip[:, 1::7] = False
    pres = (base_p[:, :, None, :] ^ flip).astype(np.float32)
    glimpse = (0.3 * rng.standard_normal((T, B, K, N, G, G))).astype(np.float32)
    lw0 = np.zeros((B, K), np.float32)
    lw = np.zeros((T, B, K), np.float32)
    for b, name in enumerate(names):
        if name == "random":
            lw0[b] = rng.standard_normal(K) * 2
            lw[:, b] = rng.standard_normal((T, K)) * 3
        elif name == "equal":
            lw0[b] = rng.standard_normal() * 5
            lw[:, b] = rng.standard_normal((T, 1))
        elif name == "dominant":
            lw0[b] = -np.inf if b % 2 == 0 else -200.0
            lw0[b, rng.integers(0, K)] = 0.0
        elif name == "spread":
            lw0[b] = -rng.uniform(size=K) * rng.uniform(80, 110)
        elif name == "neg_inf":
            lw0[b] = rng.standard_normal(K)
            dead = rng.uniform(size=K) < 0.4
            dead[rng.integers(0, K)] = False
            lw0[b] = np.where(dead, -np.inf, lw0[b])
            lw[:, b] = rng.standard_normal((T, K))
    lw0[-3, K // 2] = np.nan
    lw0[-2, K - 1] = np.inf
    lw0[-1, :] = -np.inf
    R = B * K
    return dict(B=B, glimpse=glimpse.reshape(T, R, N, G, G), where=where.reshape(T, R, N, 4), presence=pres.reshape(T, R, N),
                lw0=lw0.reshape(R), lw=lw.reshape(T, R), names=names)
