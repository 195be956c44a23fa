"""What every operator module needs of the device: the current stream, the argument checks, output buffers and the
shared workspace.  A leaf: it imports torch and ``_lib`` only (``ops`` and ``scans`` both import from here).
"""
from __future__ import annotations

import os

import torch

from . import _lib


_raw_stream = getattr(torch._C, "_cuda_getCurrentRawStream", None)


def _stream() -> int:
    """Handle of torch's current stream on the current device (the raw getter where torch has it: a fifth of the host
    time of building a Stream object, ~25 times per training epoch)."""
    if _raw_stream is not None:
        return _raw_stream(torch.cuda.current_device())
    return torch.cuda.current_stream().cuda_stream


def _need_cuda(*tensors: torch.Tensor) -> None:
    for t in tensors:
        if not t.is_cuda:
            raise _lib.DisenlinkHipError(
                "disenlink_amd operators run only on the GPU through libdisenlink_hip.so "
                "(there is no CPU fallback); got a tensor on " + str(t.device))


def _f32c(t: torch.Tensor) -> torch.Tensor:
    if t.dtype != torch.float32:
        raise TypeError(f"expected float32, got {t.dtype}")
    return t.contiguous()


def table_code(dtype) -> int:
    """The dl_dtype code of a node table's storage type: the ONE rule (fp32 or bf16, nothing else)."""
    if dtype == torch.float32:
        return _lib.DL_F32
    if dtype == torch.bfloat16:
        return _lib.DL_BF16
    raise TypeError(f"node tables must be float32 or bfloat16, got {dtype}")


def _tab(t: torch.Tensor):
    """A node table (Z or H): fp32 or bf16 storage -> (contiguous tensor, dl_dtype code)."""
    code = table_code(t.dtype)
    return t.contiguous(), code


def _nkd(Z: torch.Tensor):
    if Z.dim() != 3:
        raise ValueError("Z/H must be [N, K, d]")
    return Z.shape[0], Z.shape[1], Z.shape[2]


# DL_POISON=1 (tests): every buffer the kernels are expected to fill — outputs and the workspace — starts as
# NaN bit patterns instead of whatever the allocator hands out, so a read of anything nobody wrote shows up as
# a NaN in the result instead of depending on what happened to be in that memory.
_POISON = os.environ.get("DL_POISON", "0") == "1"


def _empty(shape, dtype, device):
    t = torch.empty(shape, dtype=dtype, device=device)
    if _POISON:
        t.view(torch.uint8).fill_(0xFF) if t.numel() else None
    return t


def _empty_like(x):
    return _empty(x.shape, x.dtype, x.device)


class _Workspace:
    """Grow-only scratch per device; the C ABI never allocates.  ONE buffer per device, whatever the stream: launches on one
    stream use it one after the other — two streams of one process computing side by side would share it (INTEGRATION.md:
    one compute stream per device, or order the streams).  (Per-stream buffers were tried at the end of round 6 and taken
    back: every graph-replayed run warms up on a fresh side stream and captures on another, so the buffers — and the
    captured graphs' memory pools they were allocated from — accumulated run after run.)"""

    def __init__(self):
        self.buf: dict = {}

    def get(self, nbytes: int, device) -> torch.Tensor:
        cur = self.buf.get(device)
        if cur is None or cur.numel() < nbytes:
            cur = torch.empty(max(nbytes, 1024), dtype=torch.uint8, device=device)
            self.buf[device] = cur
        if _POISON:
            cur.fill_(0xFF)
        return cur


_ws = _Workspace()
