"""Device plumbing shared by the wrappers of the C ABI: the stream handle a
call runs on, host <-> device copies of the unsigned columns, the cached
workspace and the statistics dict."""
from __future__ import annotations

from typing import Dict, Optional, Sequence

import numpy as np
import torch

# torch has no unsigned 16/32/64-bit tensors: device storage uses the signed
# dtype of the same width, the same bytes.
_SIGNED = {np.uint8: np.uint8, np.uint32: np.int32, np.uint64: np.int64, np.uint16: np.int16}


def stream_handle(device, stream=None) -> int:
    """The raw HIP stream for a call on ``device``: the current stream when
    ``stream`` is None, else a torch stream's handle or a raw handle as is."""
    if stream is None:
        return torch.cuda.current_stream(device).cuda_stream
    return getattr(stream, "cuda_stream", stream)


def to_dev(a: np.ndarray, dt, device) -> torch.Tensor:
    a = np.ascontiguousarray(np.asarray(a, dtype=dt))
    if a.size == 0:
        a = np.zeros(1, dtype=dt)  # keep a valid device pointer
    return torch.from_numpy(a.view(_SIGNED[dt]).copy()).to(device)


def to_np(t: torch.Tensor, dt, n: Optional[int] = None) -> np.ndarray:
    a = t.detach().cpu().numpy().view(dt)
    return a if n is None else a[:n]


def grow_workspace(cached: Optional[torch.Tensor], need: int, device) -> torch.Tensor:
    """``cached`` if it holds ``need`` bytes, else a new uint8 workspace (never
    empty, so its pointer is valid)."""
    if cached is not None and cached.numel() >= need:
        return cached
    return torch.empty(max(need, 256), dtype=torch.uint8, device=device)


def stats_dict(names: Sequence[str], tensor: torch.Tensor) -> Dict[str, int]:
    v = tensor.cpu().tolist()
    return {k: int(v[i]) for i, k in enumerate(names)}
