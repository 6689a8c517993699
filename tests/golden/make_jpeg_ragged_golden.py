"""Writes tests/golden/jpeg_ragged_cases.npz: what Pillow's bundled libjpeg-turbo makes of small images whose sides
are not whole 16x8 MCUs, with the settings of the host JPEG stage (models/utils/turbo_jpeg_compression.py
``_PillowTurbo``: the array's channels reversed in and out, ``subsampling=1`` = 4:2:2, standard Huffman tables).
numpy and Pillow only.

    python tests/golden/make_jpeg_ragged_golden.py

The layout is that of jpeg_device_cases.npz.  Per case i (``meta`` is a JSON list: name, input key, quality):
    in_<key>   uint8 [H, W, 3]   the image in the model's channel order (channel 0 is read as B)
    file_<i>   uint8 [n]         Pillow's JPEG file
    dec_<i>    uint8 [H, W, 3]   Pillow's decode of that file, same channel order
Sizes, each the smallest at which one rule of libjpeg's partial-MCU handling can go wrong:
    8x24     ceil(W/8) odd: a dummy luminance block, nothing else
    9x16     bottom replication only
    16x17    one column into a new MCU
    13x21, 15x31   both edges, odd W (the last chroma sample averages a replicated pixel; the last output is dropped)
    33x47    several MCU rows with a dummy block on each
    60x72, 64x72   the shapes the strict entry points refuse
    3x5      less than one block either way
    2x2      one chroma sample a row: libjpeg replicates it instead of interpolating
Recorded with Pillow 12.2.0.
"""
import io
import json
import os

import numpy as np
from PIL import Image

HERE = os.path.dirname(os.path.abspath(__file__))
SIZES = [(8, 24), (9, 16), (16, 17), (13, 21), (15, 31), (33, 47), (60, 72), (64, 72), (3, 5), (2, 2)]
QUALITIES = [1, 25, 50, 95]


def roundtrip(u8, quality):
    im = Image.fromarray(np.ascontiguousarray(u8[..., ::-1]), "RGB")
    buf = io.BytesIO()
    im.save(buf, format="JPEG", quality=int(quality), subsampling=1)
    data = buf.getvalue()
    dec = np.asarray(Image.open(io.BytesIO(data)).convert("RGB"))[..., ::-1]
    return np.frombuffer(data, np.uint8), np.ascontiguousarray(dec)


def images():
    rng = np.random.default_rng(20240611)
    for H, W in SIZES:
        tag = f"{H}x{W}"
        big = H * W > 2048  # the two largest sizes at two qualities only (bytes)
        yield f"noise_{tag}", rng.integers(0, 256, (H, W, 3), dtype=np.uint8), ([1, 50] if big else QUALITIES)
        ramp = np.add.outer(np.arange(H) * 2, np.arange(W)) % 256
        yield f"ramp_{tag}", np.stack([ramp, ramp // 2, 255 - ramp], -1).astype(np.uint8), QUALITIES
        prim = np.zeros((H, W, 3), np.uint8)  # saturated primaries and their complements: range limiting
        for c in range(3):
            prim[:, c * W // 3:(c + 1) * W // 3, c] = 255
        prim[H // 2:] = 255 - prim[H // 2:]
        yield f"primaries_{tag}", prim, QUALITIES
        # the last real column and row differ sharply from the rest: replication against zero fill shows in the file
        edge = np.full((H, W, 3), (40, 90, 200), np.uint8)
        edge[:, -1] = (255, 0, 30)
        edge[-1, :] = (0, 255, 250)
        yield f"edge_{tag}", edge, QUALITIES


def main():
    arrays, meta = {}, []
    for key, u8, qualities in images():
        arrays[f"in_{key}"] = u8
        for q in qualities:
            i = len(meta)
            arrays[f"file_{i}"], arrays[f"dec_{i}"] = roundtrip(u8, q)
            meta.append({"name": f"{key}_q{q}", "input": key, "quality": q})
    arrays["meta"] = np.frombuffer(json.dumps(meta).encode(), np.uint8)
    out = os.path.join(HERE, "jpeg_ragged_cases.npz")
    np.savez_compressed(out, **arrays)
    print(f"{out}: {len(meta)} cases, {os.path.getsize(out)} bytes")


if __name__ == "__main__":
    main()
