"""Cost-minimising speaker permutation between two activation sequences (utils/permutation.py:38-196):
`permutate(y1, y2)` maps the speakers of `y2` onto those of `y1` by Hungarian assignment on the mean
squared (or absolute) frame difference.  Used by `OracleClustering`; pinned by the reference's own
tests/utils/test_permutation.py (tests/test_permutation_cpu.py)."""
from __future__ import annotations

from typing import Callable, List, Optional, Tuple, Union

import numpy as np
import torch
from scipy.optimize import linear_sum_assignment

Array = Union[np.ndarray, torch.Tensor]


def _pair_costs(a: np.ndarray, b: np.ndarray, cost_func) -> np.ndarray:
    """(frames, C1), (frames, C2) -> (C1, C2) cost of pairing class i of `a` with class j of `b`"""
    if cost_func in (None, "mse", "mae"):
        diff = a[:, :, None] - b[:, None, :]
        return np.mean(diff * diff if cost_func != "mae" else np.abs(diff), axis=0)
    # callable: cost_func(Y, y) -> (num_classes,) with y one class of `a` repeated (permutation.py:143-148)
    ta, tb = torch.from_numpy(np.array(a)), torch.from_numpy(np.array(b))     # (writable copies)
    rows = [cost_func(tb, ta[:, i:i + 1].expand(-1, tb.shape[1])) for i in range(ta.shape[1])]
    return torch.stack(rows).numpy()


def permutate(y1: Array, y2: Array, cost_func: Union[Callable, str, None] = "mse", return_cost: bool = False):
    """y1: (batch, frames, C1); y2: (frames, C2) or (batch, frames, C2).
    -> (y2 re-ordered like y1 (batch, frames, C1), permutations[, costs (batch, C1, C2)]) where
    `permutations[b][i] = j` says class j of y2 plays the part of class i of y1 (None: nobody does)."""
    as_torch = isinstance(y1, torch.Tensor)
    a = y1.detach().cpu().numpy() if as_torch else np.asarray(y1)
    b = y2.detach().cpu().numpy() if isinstance(y2, torch.Tensor) else np.asarray(y2)
    if b.ndim == 2:
        b = np.broadcast_to(b, (a.shape[0],) + b.shape)
    if b.ndim != 3:
        raise ValueError("Incorrect shape: should be (batch_size, num_frames, num_classes).")
    if a.shape[:2] != b.shape[:2]:
        raise ValueError(f"Shape mismatch: {tuple(a.shape)} vs. {tuple(b.shape)}.")
    batch, _, c1 = a.shape
    c2 = b.shape[2]
    out = np.zeros(a.shape, dtype=b.dtype)
    permutations: List[Tuple[Optional[int], ...]] = []
    costs = []
    for k in range(batch):
        cost = _pair_costs(a[k], b[k], cost_func)
        costs.append(cost)
        padded = cost
        if c2 > c1:   # every class of y2 must be matched to something: dummy classes of y1 take the rest
            padded = np.concatenate([cost, np.full((c2 - c1, c2), cost.max() + 1, dtype=cost.dtype)], axis=0)
        chosen: List[Optional[int]] = [None] * c1
        for i, j in zip(*linear_sum_assignment(padded)):
            if i < c1:
                chosen[i] = int(j)
                out[k, :, i] = b[k, :, j]
        permutations.append(tuple(chosen))
    result = torch.from_numpy(out) if as_torch else out
    if return_cost:
        stacked = np.stack(costs) if costs else np.zeros((0, c1, c2))
        return result, permutations, (torch.from_numpy(stacked) if as_torch else stacked)
    return result, permutations


def _device_route(y1, y2, cost_func) -> bool:
    return (isinstance(y1, torch.Tensor) and isinstance(y2, torch.Tensor) and y1.is_cuda and y2.is_cuda
            and cost_func in (None, "mse", "mae") and y1.dtype == y2.dtype
            and y1.dtype in (torch.float32, torch.float64) and y1.ndim == 3 and y2.ndim in (2, 3)
            and y1.shape[2] * y2.shape[-1] != 1 and 0 < y1.shape[2] <= 64 and 0 < y2.shape[-1] <= 64
            and y1.shape[0] > 0 and y1.shape[1] > 0)


def permutate_batch(y1: torch.Tensor, y2: torch.Tensor, cost_func: Union[Callable, str, None] = "mse",
                    return_cost: bool = False):
    """`permutate` for device tensors, without leaving the device: the cost matrices (`pa_pair_costs`, numpy's bits),
    SciPy's assignment of every one of them (`pa_lsap_batch`) and the re-ordering (`pa_permute_classes`), three
    launches for the batch (csrc/lsap.hip).  y1: (batch, frames, C1) and y2: (frames, C2) or
    (batch, frames, C2) of one dtype, float32 or float64, of any strides.
    -> (y2 re-ordered like y1 (batch, frames, C1), permutations (batch, C1) int32 with -1 where `permutate` says None
    [, costs (batch, C1, C2) in the input dtype]), all on the device and equal to what `permutate` returns for the
    same values.  An assignment SciPy would refuse (a NaN among the costs) raises its `ValueError`.
    What has no device route goes through `permutate` and comes back on y1's device: a callable `cost_func`, C1 * C2
    == 1 (numpy adds that one column pairwise), other or mixed dtypes, more than 64 classes, an empty batch."""
    if not _device_route(y1, y2, cost_func):
        out = permutate(y1, y2, cost_func=cost_func, return_cost=return_cost)
        dev = y1.device if isinstance(y1, torch.Tensor) else None
        found = torch.tensor([[-1 if j is None else j for j in row] for row in out[1]],
                             dtype=torch.int32).reshape(len(out[1]), -1)
        moved = [torch.as_tensor(x).to(dev) if dev is not None else torch.as_tensor(x) for x in (out[0], found) + out[2:]]
        return tuple(moved)
    from . import ffi
    from .distance import linear_sum_assignment_batch
    if y2.ndim == 3 and y1.shape[:2] != y2.shape[:2] or y2.ndim == 2 and y1.shape[1] != y2.shape[0]:
        raise ValueError(f"Shape mismatch: {tuple(y1.shape)} vs. {tuple(y2.shape)}.")
    y1, y2 = y1.detach(), y2.detach()
    batch, frames, c1 = y1.shape
    c2 = y2.shape[-1]
    rows = max(c1, c2)
    strides2 = (0,) + tuple(y2.stride()) if y2.ndim == 2 else tuple(y2.stride())
    is_f64 = int(y1.dtype == torch.float64)
    lib = ffi.load()
    void = ffi.C.c_void_p
    with torch.cuda.device(y1.device):
        cost = torch.empty((batch, rows, c2), dtype=torch.float64, device=y1.device)
        ffi.check(lib.pa_pair_costs(void(y1.data_ptr()), *y1.stride(), void(y2.data_ptr()), *strides2, is_f64, batch,
                                    frames, c1, c2, int(cost_func == "mae"), ffi.ptr(cost), ffi.stream()),
                  "pa_pair_costs")
        permutations = linear_sum_assignment_batch(cost)[:, :c1]
        out = torch.empty((batch, frames, c1), dtype=y2.dtype, device=y1.device)
        ffi.check(lib.pa_permute_classes(void(y2.data_ptr()), *strides2, is_f64, void(permutations.data_ptr()), rows,
                                         batch, frames, c1, c2, ffi.ptr(out), ffi.stream()), "pa_permute_classes")
    permutations = permutations.contiguous()
    if return_cost:
        return out, permutations, cost[:, :c1].to(y1.dtype)
    return out, permutations
