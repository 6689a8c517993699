"""Device JPEG 4:2:2 base layer: the encode -> decode round trip of
models/utils/turbo_jpeg_compression.py as HIP kernels (csrc/jpeg.hip), bit-exact with libjpeg-turbo.

    roundtrip(x, quality) -> (decoded [N,3,H,W] fp32, sizes [N] int32)       both on x's device, no host sync
    encode(x, quality)    -> (decoded, [bytes per image])                    the files; one device-to-host copy
    bpp(sizes, x)         -> 0-dim fp32 device tensor = sum(sizes) * 8 / (N*H*W)
    supported(x)          -> the device path takes it (else the caller keeps the host path)

    supported_file(data)  -> the device decoder takes this JPEG file (unsupported_reason(data) says why not)
    decode(files, device) -> [N,3,H,W] fp32 on the GPU, bit-exact with libjpeg-turbo's decode: the host reads the
                             marker segments only; the entropy segments go up in one pinned copy and a
                             self-synchronising parallel Huffman decoder, DC scan and IDCT run as HIP kernels
    stage / decode_tensors   the two halves of ``decode``: capture ``decode_tensors`` into a graph over a static
                             ``Staged`` buffer and refill the buffer between replays

``roundtrip_host`` / ``encode_host`` / ``decode_host`` run the same arithmetic (csrc/jpeg_core.h) on CPU tensors through
the pure-host C-ABI; they exist to pin the codec against Pillow's libjpeg-turbo where no GPU is present.
``decode_host`` runs the decoder's very schedule (rounds over subsequences), a loop where the kernel has threads.

``any_size=True`` on any of these takes every H x W >= 1 x 1 through the ``*_any`` entry points (partial MCUs coded as
libjpeg codes them: edge replication, dummy blocks, the true size in SOF0); the default keeps whole MCUs
(H % 8 == 0, W % 16 == 0) as the contract, and everything else stays with the caller's host path.
"""
from __future__ import annotations

import ctypes
from typing import List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib as L


def supported_shape(x: torch.Tensor, any_size: bool = False) -> bool:
    """3-channel fp32 NCHW with whole 16x8 MCUs; any_size: any H, W in 1 .. 65535."""
    if not (isinstance(x, torch.Tensor) and x.dtype == torch.float32 and x.dim() == 4
            and x.size(0) >= 1 and x.size(1) == 3):
        return False
    if any_size:
        return 1 <= x.size(2) <= 65535 and 1 <= x.size(3) <= 65535
    return x.size(2) >= 8 and x.size(3) >= 16 and x.size(2) % 8 == 0 and x.size(3) % 16 == 0


def supported(x: torch.Tensor, any_size: bool = False) -> bool:
    """The device path takes ``x``: a supported shape, on the GPU."""
    return supported_shape(x, any_size) and x.is_cuda


_ANY = {
    "hyres_jpeg_workspace_bytes": "hyres_jpeg_workspace_bytes_any",
    "hyres_jpeg_stream_bytes": "hyres_jpeg_stream_bytes_any",
    "hyres_jpeg_roundtrip": "hyres_jpeg_roundtrip_any",
    "hyres_jpeg_roundtrip_host": "hyres_jpeg_roundtrip_any_host",
    "hyres_jpeg_parse": "hyres_jpeg_parse_any",
    "hyres_jpeg_decode_workspace_bytes": "hyres_jpeg_decode_any_workspace_bytes",
    "hyres_jpeg_decode": "hyres_jpeg_decode_any",
    "hyres_jpeg_decode_host": "hyres_jpeg_decode_any_host",
}


def _any(name: str, any_size: bool) -> str:
    """The C-ABI name of an entry point or of its any-size twin."""
    return _ANY[name] if any_size else name


def quant_tables(quality: int) -> Tuple[np.ndarray, np.ndarray]:
    """The luminance / chrominance DQT payloads (zigzag order) libjpeg writes for ``quality``."""
    lum, chr_ = np.zeros(64, np.uint8), np.zeros(64, np.uint8)
    L.call("hyres_jpeg_quant_tables", int(quality), lum.ctypes.data, chr_.ctypes.data)
    return lum, chr_


def stream_bytes(H: int, W: int, any_size: bool = False) -> int:
    name = _any("hyres_jpeg_stream_bytes", any_size)
    n = getattr(L.load(), name)(int(H), int(W))
    if n < 0:
        L.check(1, name)
    return int(n)


def _run(x: torch.Tensor, quality: int, files: bool, any_size: bool = False):
    if not supported(x, any_size):
        raise ValueError(f"jpeg_device: unsupported input {tuple(x.shape)} {x.dtype} on {x.device} "
                         "(3-channel fp32 NCHW on the GPU" + ("" if any_size else ", H % 8 == 0, W % 16 == 0") + ")")
    from .ops import Workspace
    x = x.detach().contiguous()
    N, _, H, W = x.shape
    name = _any("hyres_jpeg_workspace_bytes", any_size)
    nws = getattr(L.load(), name)(N, H, W)
    if nws < 0:
        L.check(1, name)
    ws = Workspace.get(int(nws), x.device, "jpeg")
    decoded = torch.empty_like(x)
    sizes = torch.empty(N, dtype=torch.int32, device=x.device)
    stride = stream_bytes(H, W, any_size) if files else 0
    buf = torch.empty((N, stride), dtype=torch.uint8, device=x.device) if files else None
    L.call(_any("hyres_jpeg_roundtrip", any_size), x.data_ptr(), N, H, W, int(quality), decoded.data_ptr(), sizes.data_ptr(),
           L.ptr(buf), stride, ws.data_ptr(), ws.numel(), L.stream())
    return decoded, sizes, buf


def roundtrip(x: torch.Tensor, quality: int, any_size: bool = False) -> Tuple[torch.Tensor, torch.Tensor]:
    decoded, sizes, _ = _run(x, quality, False, any_size)
    return decoded, sizes


def bpp(sizes: torch.Tensor, x: torch.Tensor) -> torch.Tensor:
    """total bytes * 8 / (N*H*W), rounded to fp32 once as the host stage's Python float is."""
    N, _, H, W = x.shape
    return (sizes.sum(dtype=torch.int64) * 8).to(torch.float64).div(N * H * W).to(torch.float32)


def _split(buf: torch.Tensor, sizes) -> List[bytes]:
    return [buf[i, :int(n)].numpy().tobytes() for i, n in enumerate(sizes)]


def encode(x: torch.Tensor, quality: int, any_size: bool = False) -> Tuple[torch.Tensor, List[bytes]]:
    decoded, sizes, buf = _run(x, quality, True, any_size)
    sizes_h = sizes.cpu().tolist()
    # one device-to-host copy of the used prefix of every file
    return decoded, _split(buf[:, :max(sizes_h)].cpu(), sizes_h)


# ---------------------------------------------------------------------------------------------- host (CPU tensors)
def _run_host(x: torch.Tensor, quality: int, files: bool, any_size: bool = False):
    if x.is_cuda or x.dtype != torch.float32 or x.dim() != 4 or x.size(1) != 3:
        raise ValueError("jpeg_device.roundtrip_host: 3-channel fp32 NCHW CPU tensor")
    x = x.detach().contiguous()
    N, _, H, W = x.shape
    decoded = torch.empty_like(x)
    sizes = torch.empty(N, dtype=torch.int32)
    stride = stream_bytes(H, W, any_size) if files else 0
    buf = torch.empty((N, stride), dtype=torch.uint8) if files else None
    L.call(_any("hyres_jpeg_roundtrip_host", any_size), x.data_ptr(), N, H, W, int(quality), decoded.data_ptr(), sizes.data_ptr(),
           L.ptr(buf), stride, None, 0, ctypes.c_void_p(None))
    return decoded, sizes, buf


def roundtrip_host(x: torch.Tensor, quality: int, any_size: bool = False) -> Tuple[torch.Tensor, torch.Tensor]:
    decoded, sizes, _ = _run_host(x, quality, False, any_size)
    return decoded, sizes


def encode_host(x: torch.Tensor, quality: int, any_size: bool = False) -> Tuple[torch.Tensor, List[bytes]]:
    decoded, sizes, buf = _run_host(x, quality, True, any_size)
    return decoded, _split(buf, sizes.tolist())


# ---------------------------------------------------------------------------------------------- decoding files
def _parse(data, any_size: bool = False) -> Tuple[Optional[L.JpegInfo], Optional[str]]:
    data = bytes(data)
    info = L.JpegInfo()
    L.call(_any("hyres_jpeg_parse", any_size), data, len(data), ctypes.byref(info))
    if info.supported:
        return info, None
    return None, L.load().hyres_last_error_string().decode()


def unsupported_reason(data, any_size: bool = False) -> Optional[str]:
    """None when the device decoder takes the file, else why it does not (the file keeps the host decoder)."""
    return _parse(data, any_size)[1]


def supported_file(data, any_size: bool = False) -> bool:
    """Baseline 8-bit 4:2:2 with the Annex K Huffman tables, one interleaved scan, no restart interval; whole MCUs
    unless ``any_size``."""
    return _parse(data, any_size)[0] is not None


class Staged:
    """N files of one size ready for ``decode_tensors``: one uint8 buffer holding the scan offsets (int64), lengths
    (int32), quantisers [N,2,64] and the raw entropy segments; ``capacity`` bounds every segment's length."""

    def __init__(self, buf: torch.Tensor, N: int, H: int, W: int, capacity: int, room: int, any_size: bool = False):
        self.buf, self.N, self.H, self.W, self.capacity, self.room = buf, N, H, W, capacity, room
        self.any_size = any_size
        self.o_len, self.o_q, self.o_scans = self.layout(N)[:3]

    @staticmethod
    def layout(N: int, room: int = 0):
        o_len = 8 * N
        o_q = (o_len + 4 * N + 7) & ~7
        o_scans = (o_q + 128 * N + 15) & ~15
        return o_len, o_q, o_scans, o_scans + room

    scan_off = property(lambda s: s.buf[:s.o_len].view(torch.int64))
    scan_len = property(lambda s: s.buf[s.o_len:s.o_len + 4 * s.N].view(torch.int32))
    qtabs = property(lambda s: s.buf[s.o_q:s.o_q + 128 * s.N])
    scans = property(lambda s: s.buf[s.o_scans:])


_pinned = {}  # stream -> (pinned staging buffer, event of its last upload)


def _pinned_for(nbytes: int, device: torch.device) -> torch.Tensor:
    key = (device.index, torch.cuda.current_stream(device).cuda_stream)
    ent = _pinned.get(key)
    if ent is not None:
        ent[1].synchronize()  # the previous upload has read the buffer
    if ent is None or ent[0].numel() < nbytes:
        n = max(int(nbytes), 1 << 16)
        if ent is not None:
            n = max(n, int(ent[0].numel() * 1.5))
        ent = (torch.empty(n, dtype=torch.uint8, pin_memory=True), torch.cuda.Event())
        _pinned[key] = ent
    return ent[0]


def stage(files: Sequence, device=None, capacity: Optional[int] = None, room: Optional[int] = None,
          any_size: bool = False) -> Staged:
    """Parse ``files`` (bytes each) and lay their entropy segments out for the decoder; on a GPU ``device`` with one
    pinned upload, else (None / CPU) as a host buffer.  ``capacity`` / ``room`` fix the longest segment / the bytes of
    all segments the buffer can take (for a static buffer refilled between graph replays)."""
    datas = [bytes(f) for f in files]
    if not datas:
        raise ValueError("jpeg_device.stage: no files")
    infos = []
    for i, d in enumerate(datas):
        info, why = _parse(d, any_size)
        if info is None:
            raise ValueError(f"jpeg_device: file {i} is not supported by the device decoder: {why}")
        infos.append(info)
    H, W = infos[0].H, infos[0].W
    if any((f.H, f.W) != (H, W) for f in infos):
        raise ValueError("jpeg_device: the files differ in H x W")
    N = len(datas)
    lens = [int(f.scan_len) for f in infos]
    need = sum((n + 15) & ~15 for n in lens) + 16
    capacity = max(max(lens), 1) if capacity is None else int(capacity)
    room = need if room is None else int(room)
    if max(lens) > capacity or need > room:
        raise ValueError(f"jpeg_device.stage: segments of {max(lens)} / {need} bytes exceed capacity {capacity} / "
                         f"room {room}")
    o_len, o_q, o_scans, total = Staged.layout(N, room)
    on_gpu = device is not None and torch.device(device).type == "cuda"
    host = _pinned_for(total, torch.device(device))[:total] if on_gpu else torch.empty(total, dtype=torch.uint8)
    h = host.numpy()
    offs, o = [], 0
    for d, f, n in zip(datas, infos, lens):
        h[o_scans + o:o_scans + o + n] = np.frombuffer(d, np.uint8, n, int(f.scan_off))
        offs.append(o)
        o += (n + 15) & ~15
    h[:o_len].view(np.int64)[:] = offs
    h[o_len:o_len + 4 * N].view(np.int32)[:] = lens
    h[o_q:o_q + 128 * N] = np.concatenate([np.frombuffer(bytes(f.qtab), np.uint8) for f in infos])
    if not on_gpu:
        return Staged(host, N, H, W, capacity, room, any_size)
    device = torch.device(device)
    buf = torch.empty(total, dtype=torch.uint8, device=device)
    buf.copy_(host, non_blocking=True)  # the one upload
    _pinned[(device.index, torch.cuda.current_stream(device).cuda_stream)][1].record()
    return Staged(buf, N, H, W, capacity, room, any_size)


def decode_tensors(st: Staged, sub_bits: int = 0, block_threads: int = 0):
    """The kernels of ``decode`` on a staged batch: (decoded [N,3,H,W] fp32, status [N] int32, rounds [N] int32) on
    the device, no host sync — capture-legal once the stream's workspace exists (after one warm-up call)."""
    from .ops import Workspace
    dev = st.buf.device
    if dev.type != "cuda":
        raise ValueError("jpeg_device.decode_tensors: the staged batch is not on the GPU (decode_host decodes there)")
    name = _any("hyres_jpeg_decode_workspace_bytes", st.any_size)
    nws = getattr(L.load(), name)(st.N, st.H, st.W, st.capacity)
    if nws < 0:
        L.check(1, name)
    ws = Workspace.get(int(nws), dev, "jpeg_decode")
    decoded = torch.empty((st.N, 3, st.H, st.W), dtype=torch.float32, device=dev)
    status = torch.empty(st.N, dtype=torch.int32, device=dev)
    rounds = torch.empty(st.N, dtype=torch.int32, device=dev)
    L.call(_any("hyres_jpeg_decode", st.any_size), st.scans.data_ptr(), st.scan_off.data_ptr(), st.scan_len.data_ptr(),
           st.qtabs.data_ptr(), st.N, st.H, st.W, st.capacity, int(sub_bits), int(block_threads), decoded.data_ptr(),
           status.data_ptr(), rounds.data_ptr(), ws.data_ptr(), ws.numel(), L.stream())
    return decoded, status, rounds


def _raise_on_status(status: List[int]) -> None:
    bad = [(i, s) for i, s in enumerate(status) if s]
    if bad:
        raise ValueError("jpeg_device: corrupt entropy-coded segment in image(s) "
                         + ", ".join(f"{i} (status {s})" for i, s in bad))


def decode(files: Sequence, device, sub_bits: int = 0, check: bool = True, any_size: bool = False):
    """JPEG files (bytes) of one size -> [N,3,H,W] fp32 on ``device``.  check: read the N status words back and
    raise ValueError naming the corrupt images; check=False returns (decoded, status), both on the device."""
    decoded, status, _ = decode_tensors(stage(files, device, any_size=any_size), sub_bits)
    if not check:
        return decoded, status
    _raise_on_status(status.cpu().tolist())
    return decoded


def decode_host(files: Sequence, sub_bits: int = 0, check: bool = True, return_rounds: bool = False,
                any_size: bool = False):
    """``decode`` on the host twin (CPU tensors): the same rounds, write pass, DC scan and IDCT, no GPU call."""
    st = stage(files, None, any_size=any_size)
    decoded = torch.empty((st.N, 3, st.H, st.W), dtype=torch.float32)
    status = torch.empty(st.N, dtype=torch.int32)
    rounds = torch.empty(st.N, dtype=torch.int32)
    L.call(_any("hyres_jpeg_decode_host", any_size), st.scans.data_ptr(), st.scan_off.data_ptr(), st.scan_len.data_ptr(),
           st.qtabs.data_ptr(), st.N, st.H, st.W, st.capacity, int(sub_bits), 0, decoded.data_ptr(),
           status.data_ptr(), rounds.data_ptr(), None, 0, ctypes.c_void_p(None))
    if check:
        _raise_on_status(status.tolist())
    out = (decoded,) + (() if check else (status,)) + ((rounds,) if return_rounds else ())
    return out[0] if len(out) == 1 else out
