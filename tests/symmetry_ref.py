"""The board symmetries of include/mssym.h restated in numpy: the three-line transform, its
inverse, the cell map it implies, and the pairwise mean. Shared by tests/test_symmetry_host.py
and tests/test_symmetry_gpu.py."""
from __future__ import annotations

import numpy as np

# (H, W): degenerate, odd, rectangular both ways, the production board, and A = 512
SHAPES = ((1, 1), (1, 7), (7, 1), (2, 2), (4, 4), (5, 7), (9, 9), (16, 16), (16, 30), (30, 16), (16, 32))


def group_size(H: int, W: int) -> int:
    return 8 if H == W else 4


def transform(X: np.ndarray, g: int) -> np.ndarray:
    """T_g on the last two axes of X."""
    if g & 4:
        X = np.swapaxes(X, -1, -2)
    if g & 1:
        X = X[..., ::-1, :]
    if g & 2:
        X = X[..., :, ::-1]
    return X


def inverse(g: int) -> int:
    return g if g < 4 else 4 | ((g & 1) << 1) | ((g >> 1) & 1)


def cell_map(H: int, W: int, g: int) -> np.ndarray:
    """map with T_g(X).flat[i] == X.flat[map[i]]: the transform of the planes of cell indices."""
    return np.ascontiguousarray(transform(np.arange(H * W, dtype=np.int32).reshape(H, W), g)).reshape(-1)


def rows_transform(plane: np.ndarray, g: np.ndarray, H: int, W: int) -> np.ndarray:
    """[n, H*W] -> [n, H*W], row i under T_{g[i]}."""
    out = np.empty_like(plane)
    for i in range(plane.shape[0]):
        out[i] = np.ascontiguousarray(transform(plane[i].reshape(H, W), int(g[i]))).reshape(-1)
    return out


def expand(codes: np.ndarray, G: int) -> np.ndarray:
    """[n, H, W] -> [G, n, H, W]."""
    return np.stack([np.ascontiguousarray(transform(codes, g)) for g in range(G)])


def mean(x: np.ndarray, H: int, W: int) -> np.ndarray:
    """f32 [G, n, H*W] -> f32 [n, H*W]: every image moved back (T_g undone) and summed in the
    fixed pairwise tree, then one multiply by 1/G; f32 throughout."""
    G, n, A = x.shape
    y = [np.ascontiguousarray(transform(x[g].reshape(n, H, W), inverse(g))).reshape(n, A).astype(np.float32)
         for g in range(G)]
    if G == 1:
        s = y[0]
    elif G == 4:
        s = (y[0] + y[1]) + (y[2] + y[3])
    else:
        assert G == 8
        s = ((y[0] + y[1]) + (y[2] + y[3])) + ((y[4] + y[5]) + (y[6] + y[7]))
    return (s * np.float32(1.0 / G)).astype(np.float32)
