"""Device JPEG 4:2:2 base layer: the encode -> decode round trip of
models/utils/turbo_jpeg_compression.py as HIP kernels (csrc/jpeg.hip), bit-exact with libjpeg-turbo.

    roundtrip(x, quality) -> (decoded [N,3,H,W] fp32, sizes [N] int32)       both on x's device, no host sync
    encode(x, quality)    -> (decoded, [bytes per image])                    the files; one device-to-host copy
    bpp(sizes, x)         -> 0-dim fp32 device tensor = sum(sizes) * 8 / (N*H*W)
    supported(x)          -> the device path takes it (else the caller keeps the host path)

``roundtrip_host`` / ``encode_host`` run the same arithmetic (csrc/jpeg_core.h) on CPU tensors through the pure-host
C-ABI; they exist to pin the codec against Pillow's libjpeg-turbo where no GPU is present.
"""
from __future__ import annotations

import ctypes
from typing import List, Tuple

import numpy as np
import torch

from . import _lib as L


def supported_shape(x: torch.Tensor) -> bool:
    """3-channel fp32 NCHW with whole 16x8 MCUs (no edge replication, no dummy blocks)."""
    return (isinstance(x, torch.Tensor) and x.dtype == torch.float32 and x.dim() == 4
            and x.size(0) >= 1 and x.size(1) == 3 and x.size(2) >= 8 and x.size(3) >= 16
            and x.size(2) % 8 == 0 and x.size(3) % 16 == 0)


def supported(x: torch.Tensor) -> bool:
    """The device path takes ``x``: a supported shape, on the GPU."""
    return supported_shape(x) and x.is_cuda


def quant_tables(quality: int) -> Tuple[np.ndarray, np.ndarray]:
    """The luminance / chrominance DQT payloads (zigzag order) libjpeg writes for ``quality``."""
    lum, chr_ = np.zeros(64, np.uint8), np.zeros(64, np.uint8)
    L.call("hyres_jpeg_quant_tables", int(quality), lum.ctypes.data, chr_.ctypes.data)
    return lum, chr_


def stream_bytes(H: int, W: int) -> int:
    n = L.load().hyres_jpeg_stream_bytes(int(H), int(W))
    if n < 0:
        L.check(1, "hyres_jpeg_stream_bytes")
    return int(n)


def _run(x: torch.Tensor, quality: int, files: bool):
    if not supported(x):
        raise ValueError(f"jpeg_device: unsupported input {tuple(x.shape)} {x.dtype} on {x.device} "
                         "(3-channel fp32 NCHW on the GPU, H % 8 == 0, W % 16 == 0)")
    from .ops import Workspace
    x = x.detach().contiguous()
    N, _, H, W = x.shape
    lib = L.load()
    nws = lib.hyres_jpeg_workspace_bytes(N, H, W)
    if nws < 0:
        L.check(1, "hyres_jpeg_workspace_bytes")
    ws = Workspace.get(int(nws), x.device, "jpeg")
    decoded = torch.empty_like(x)
    sizes = torch.empty(N, dtype=torch.int32, device=x.device)
    stride = stream_bytes(H, W) if files else 0
    buf = torch.empty((N, stride), dtype=torch.uint8, device=x.device) if files else None
    L.call("hyres_jpeg_roundtrip", x.data_ptr(), N, H, W, int(quality), decoded.data_ptr(), sizes.data_ptr(),
           L.ptr(buf), stride, ws.data_ptr(), ws.numel(), L.stream())
    return decoded, sizes, buf


def roundtrip(x: torch.Tensor, quality: int) -> Tuple[torch.Tensor, torch.Tensor]:
    decoded, sizes, _ = _run(x, quality, False)
    return decoded, sizes


def bpp(sizes: torch.Tensor, x: torch.Tensor) -> torch.Tensor:
    """total bytes * 8 / (N*H*W), rounded to fp32 once as the host stage's Python float is."""
    N, _, H, W = x.shape
    return (sizes.sum(dtype=torch.int64) * 8).to(torch.float64).div(N * H * W).to(torch.float32)


def _split(buf: torch.Tensor, sizes) -> List[bytes]:
    return [buf[i, :int(n)].numpy().tobytes() for i, n in enumerate(sizes)]


def encode(x: torch.Tensor, quality: int) -> Tuple[torch.Tensor, List[bytes]]:
    decoded, sizes, buf = _run(x, quality, True)
    sizes_h = sizes.cpu().tolist()
    # one device-to-host copy of the used prefix of every file
    return decoded, _split(buf[:, :max(sizes_h)].cpu(), sizes_h)


# ---------------------------------------------------------------------------------------------- host (CPU tensors)
def _run_host(x: torch.Tensor, quality: int, files: bool):
    if x.is_cuda or x.dtype != torch.float32 or x.dim() != 4 or x.size(1) != 3:
        raise ValueError("jpeg_device.roundtrip_host: 3-channel fp32 NCHW CPU tensor")
    x = x.detach().contiguous()
    N, _, H, W = x.shape
    decoded = torch.empty_like(x)
    sizes = torch.empty(N, dtype=torch.int32)
    stride = stream_bytes(H, W) if files else 0
    buf = torch.empty((N, stride), dtype=torch.uint8) if files else None
    L.call("hyres_jpeg_roundtrip_host", x.data_ptr(), N, H, W, int(quality), decoded.data_ptr(), sizes.data_ptr(),
           L.ptr(buf), stride, None, 0, ctypes.c_void_p(None))
    return decoded, sizes, buf


def roundtrip_host(x: torch.Tensor, quality: int) -> Tuple[torch.Tensor, torch.Tensor]:
    decoded, sizes, _ = _run_host(x, quality, False)
    return decoded, sizes


def encode_host(x: torch.Tensor, quality: int) -> Tuple[torch.Tensor, List[bytes]]:
    decoded, sizes, buf = _run_host(x, quality, True)
    return decoded, _split(buf, sizes.tolist())
