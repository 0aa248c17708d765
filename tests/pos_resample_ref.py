"""The fp64 definition of the position-table resample (plain helper module, no tests of its own; include/xpretrain_hip.h:
xp_pos_resample_fwd / xp_pos_resample_bwd; transformers' ``CLIPVisionEmbeddings.interpolate_pos_encoding``).

Per axis of target length g over a source axis of length g0: destination d reads the source coordinate (d + 0.5) g0 / g - 0.5, taken
as the exact rational ((2 d + 1) g0 - g) / (2 g): its floor i and fraction t come from integer division, the four taps i-1 .. i+2 are
clamped to [0, g0-1], and the weights are the Keys cubic-convolution weights with A = -0.75.  ``axis_matrix`` is the dense [g, g0]
matrix of that map (clamped taps that coincide add up); the 2-D map is Wy (x) Wx on the g0 x g0 grid of rows 1.., row 0 is copied.
tests/test_pos_resample_cpu.py holds this against torch's float64 ``F.interpolate`` and its autograd."""
import math

import numpy as np

KEYS_A = -0.75

# (g0, gh, gw): the grids of tests/test_pos_resample_cpu.py
GRIDS = [(7, 3, 5), (7, 10, 13), (7, 14, 14), (14, 28, 28), (14, 7, 7), (4, 6, 5), (2, 5, 3), (1, 3, 3), (7, 1, 1)]
# (g0, gh, gw, D): the kernel cases of tests/test_pos_resample_gpu.py
KERNEL_CASES = [(7, 3, 5, 64), (7, 10, 13, 192), (7, 14, 14, 768), (14, 28, 28, 768), (14, 7, 7, 128), (2, 5, 3, 64), (1, 3, 3, 64),
                (7, 1, 1, 64)]


def grid_of(rows: int) -> int:
    g0 = math.isqrt(rows - 1)
    if g0 * g0 != rows - 1:
        raise ValueError(f"{rows} rows: not 1 + a square")
    return g0


def keys_weights(t: float):
    """weights of taps i-1, i, i+1, i+2 at fraction t (cubic convolution, A = -0.75)"""
    A = KEYS_A

    def near(x):            # |x| <= 1
        return ((A + 2.0) * x - (A + 3.0)) * x * x + 1.0

    def far(x):             # 1 < |x| < 2
        return ((A * x - 5.0 * A) * x + 8.0 * A) * x - 4.0 * A
    return far(t + 1.0), near(t), near(1.0 - t), far(2.0 - t)


def axis_matrix(g0: int, g: int) -> np.ndarray:
    W = np.zeros((g, g0), np.float64)
    for d in range(g):
        num, den = (2 * d + 1) * g0 - g, 2 * g
        i = num // den                       # Python's // floors
        w = keys_weights((num - i * den) / den)
        for k in range(4):
            W[d, min(max(i - 1 + k, 0), g0 - 1)] += w[k]
    return W


def forward(pos: np.ndarray, gh: int, gw: int) -> np.ndarray:
    """pos [1 + g0*g0, D] -> [1 + gh*gw, D], float64"""
    pos = np.asarray(pos, np.float64)
    g0, D = grid_of(pos.shape[0]), pos.shape[1]
    grid = np.einsum("ys,xt,std->yxd", axis_matrix(g0, gh), axis_matrix(g0, gw), pos[1:].reshape(g0, g0, D))
    return np.concatenate([pos[:1], grid.reshape(gh * gw, D)])


def transpose(d_out: np.ndarray, g0: int, gh: int, gw: int) -> np.ndarray:
    """d_out [1 + gh*gw, D] -> d_pos [1 + g0*g0, D], float64: the transposed map"""
    d_out = np.asarray(d_out, np.float64)
    D = d_out.shape[1]
    assert d_out.shape[0] == 1 + gh * gw
    grid = np.einsum("ys,xt,yxd->std", axis_matrix(g0, gh), axis_matrix(g0, gw), d_out[1:].reshape(gh, gw, D))
    return np.concatenate([d_out[:1], grid.reshape(g0 * g0, D)])
