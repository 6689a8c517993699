"""Writes tests/golden/jpeg_device_cases.npz: what Pillow's bundled libjpeg-turbo makes of small images with the
settings of the host JPEG stage (models/utils/turbo_jpeg_compression.py ``_PillowTurbo``: the array's channels
reversed in and out, ``subsampling=1`` = 4:2:2, standard Huffman tables).  numpy and Pillow only.

    python tests/golden/make_jpeg_device_golden.py

Per case i (``meta`` is a JSON list, one entry per case: name, input key, quality):
    in_<key>   uint8 [H, W, 3]   the image in the model's channel order (channel 0 is read as B)
    file_<i>   uint8 [n]         Pillow's JPEG file
    dec_<i>    uint8 [H, W, 3]   Pillow's decode of that file, same channel order
Inputs are shared between the qualities of one image.  Recorded with Pillow 12.2.0.
"""
import io
import json
import os

import numpy as np
from PIL import Image

HERE = os.path.dirname(os.path.abspath(__file__))
SIZES = [(8, 16), (16, 32), (24, 48), (64, 64), (64, 128)]
QUALITIES = [1, 25, 50, 95]


def roundtrip(u8, quality):
    im = Image.fromarray(np.ascontiguousarray(u8[..., ::-1]), "RGB")
    buf = io.BytesIO()
    im.save(buf, format="JPEG", quality=int(quality), subsampling=1)
    data = buf.getvalue()
    dec = np.asarray(Image.open(io.BytesIO(data)).convert("RGB"))[..., ::-1]
    return np.frombuffer(data, np.uint8), np.ascontiguousarray(dec)


def images():
    rng = np.random.default_rng(20240607)
    for H, W in SIZES:
        tag = f"{H}x{W}"
        # uniform noise: long codes, ZRL runs, stuffed 0xFF bytes; the largest size at two qualities only (bytes)
        yield f"noise_{tag}", rng.integers(0, 256, (H, W, 3), dtype=np.uint8), (QUALITIES if W < 128 else [1, 50])
        ramp = np.add.outer(np.arange(H) * 2, np.arange(W)) % 256  # smooth: DC / EOB only at low quality
        yield f"ramp_{tag}", np.stack([ramp, ramp // 2, 255 - ramp], -1).astype(np.uint8), QUALITIES
        yield f"zeros_{tag}", np.zeros((H, W, 3), np.uint8), QUALITIES
        yield f"full_{tag}", np.full((H, W, 3), 255, np.uint8), QUALITIES
        prim = np.zeros((H, W, 3), np.uint8)  # saturated primaries and their complements: range limiting
        for c in range(3):
            prim[:, c * W // 3:(c + 1) * W // 3, c] = 255
        prim[H // 2:] = 255 - prim[H // 2:]
        yield f"primaries_{tag}", prim, QUALITIES
    with np.load(os.path.join(HERE, "kodim01_crop64_eval.npz")) as z:
        x = z["x"]
    for i in range(x.shape[0]):
        u8 = (np.clip(x[i], 0, 1) * np.float32(255)).astype(np.uint8).transpose(1, 2, 0)
        yield f"kodim01_{i}", np.ascontiguousarray(u8), [1, 50]


def main():
    arrays, meta = {}, []
    for key, u8, qualities in images():
        arrays[f"in_{key}"] = u8
        for q in qualities:
            i = len(meta)
            arrays[f"file_{i}"], arrays[f"dec_{i}"] = roundtrip(u8, q)
            meta.append({"name": f"{key}_q{q}", "input": key, "quality": q})
    arrays["meta"] = np.frombuffer(json.dumps(meta).encode(), np.uint8)
    out = os.path.join(HERE, "jpeg_device_cases.npz")
    np.savez_compressed(out, **arrays)
    print(f"{out}: {len(meta)} cases, {os.path.getsize(out)} bytes")


if __name__ == "__main__":
    main()
