"""Layout predicates for the tensor arguments of the engines' device entry points: pure functions of a tensor and a
device, no engine in them.  They answer; the caller raises, with a message that names its method, its argument and the
dtype, shape and device it needs."""
from __future__ import annotations

import torch


def is_exact(t, device, dtype, shape, contiguous: bool = True) -> bool:
    """``t`` is a contiguous ``dtype`` tensor of exactly ``shape`` on ``device``.  ``shape``: a tuple, None standing for
    any size -- or an int: that many elements, whatever the shape.  ``contiguous=False``: any strides."""
    if not isinstance(t, torch.Tensor) or t.dtype != dtype or t.device != device or (contiguous and not t.is_contiguous()):
        return False
    if isinstance(shape, int):
        return t.numel() == shape
    return t.dim() == len(shape) and all(w is None or s == w for s, w in zip(t.shape, shape))


def is_rows(t, device, dtypes, T: int, N: int, P: int, tail: tuple = (), at_least: bool = False) -> bool:
    """``t`` is ``[T, N] + tail`` rows of pitch ``P`` lanes on ``device``, of one of ``dtypes``, everything inside a row
    dense.  ``at_least``: ``shape[0] >= T``.  A stride is compared only where the size is above 1."""
    if (not isinstance(t, torch.Tensor) or t.dtype not in dtypes or t.device != device or t.dim() != 2 + len(tail)
            or (t.shape[0] < T if at_least else t.shape[0] != T) or tuple(t.shape[1:]) != (N,) + tuple(tail)):
        return False
    per_lane = 1  # elements
    for d in range(t.dim() - 1, 1, -1):
        if t.shape[d] > 1 and t.stride(d) != per_lane:
            return False
        per_lane *= t.shape[d]
    return (N <= 1 or t.stride(1) == per_lane) and (t.shape[0] <= 1 or t.stride(0) == P * per_lane)


def row_layout(t) -> tuple[int, int, int]:
    """``(T, N, P)`` of a ``[T, N]`` tensor that leads a group of rows: ``P``, the lanes per row, is ``stride(0)``, and
    ``N`` where one row leaves it open.  (ValueError from the unpacking unless ``t`` has two dimensions.)"""
    T, N = (int(v) for v in t.shape)
    return T, N, (int(t.stride(0)) if T > 1 else N)
