"""TEST INFRASTRUCTURE ONLY: pure-Python restatement of the device coder's string format HRW1, written from its
specification (DESIGN.md "Device rANS coder"), not from the C++.

One string per image and pass, little endian:
    "HRW1" | uint32 n | uint32 n_esc | uint32 n_words | 64 x uint64 lane states | n_esc x int32 | n_words x uint32
* coded symbols: the positions of the [C, H, W] latent in (c, h, w) order that the checkerboard parity owns
  ((h + w) % 2 == parity; parity -1 owns all); coded symbol k has row k // 64 and lane k % 64;
* slot: v = sym - offset[ci], max_value = cdf_size[ci] - 2; 0 <= v < max_value codes slot v, anything else codes slot
  max_value and appends the raw sym to the escape list (coded-symbol order);
* lanes: rans64 (64-bit state from 1 << 31, 32-bit words, precision 16); the encoder walks rows last to first, the
  decoder first to last; the words of the lanes that renormalise at a row lie in ascending lane order, rows ascending.
"""
from __future__ import annotations

import math
import struct
from typing import List, Sequence, Tuple

LANES = 64
L = 1 << 31
PRECISION = 16
MAGIC = b"HRW1"
FIXED = 16 + 8 * LANES


def owned(C: int, H: int, W: int, parity: int) -> List[int]:
    """Flat (c, h, w) indexes of the coded positions, in coded-symbol order."""
    return [(c * H + h) * W + w for c in range(C) for h in range(H) for w in range(W)
            if parity < 0 or (h + w) % 2 == parity]


def _slots(sym: Sequence[int], idx: Sequence[int], cdfs, sizes, offsets) -> Tuple[list, list]:
    steps, esc = [], []
    for s, ci in zip(sym, idx):
        max_value = int(sizes[ci]) - 2
        v = int(s) - int(offsets[ci])
        if not 0 <= v < max_value:
            v = max_value
            esc.append(int(s))
        start = int(cdfs[ci][v])
        steps.append((start, int(cdfs[ci][v + 1]) - start))
    return steps, esc


def encode(sym: Sequence[int], idx: Sequence[int], cdfs, sizes, offsets) -> bytes:
    """``sym`` / ``idx``: the coded symbols and their CDF rows, in coded-symbol order."""
    n = len(sym)
    steps, esc = _slots(sym, idx, cdfs, sizes, offsets)
    x = [L] * LANES
    rows = (n + LANES - 1) // LANES
    row_words: List[List[int]] = [[] for _ in range(rows)]
    for r in range(rows - 1, -1, -1):
        for lane in range(LANES):
            k = r * LANES + lane
            if k >= n:
                break
            start, freq = steps[k]
            if x[lane] >= ((L >> PRECISION) << 32) * freq:
                row_words[r].append(x[lane] & 0xFFFFFFFF)
                x[lane] >>= 32
            x[lane] = ((x[lane] // freq) << PRECISION) + (x[lane] % freq) + start
    words = [w for row in row_words for w in row]
    return (MAGIC + struct.pack("<3I", n, len(esc), len(words)) + struct.pack("<64Q", *x)
            + struct.pack(f"<{len(esc)}i", *esc) + struct.pack(f"<{len(words)}I", *words))


def parse(data: bytes):
    """(n, states, escapes, words) of a well-formed string."""
    assert data[:4] == MAGIC and len(data) >= FIXED
    n, n_esc, n_words = struct.unpack_from("<3I", data, 4)
    assert len(data) == FIXED + 4 * (n_esc + n_words)
    states = list(struct.unpack_from("<64Q", data, 16))
    esc = list(struct.unpack_from(f"<{n_esc}i", data, FIXED))
    words = list(struct.unpack_from(f"<{n_words}I", data, FIXED + 4 * n_esc))
    return n, states, esc, words


def decode(data: bytes, idx: Sequence[int], cdfs, sizes, offsets) -> List[int]:
    n, x, esc, words = parse(data)
    assert n == len(idx)
    out, wpos, epos = [], 0, 0
    for k in range(n):
        lane, ci = k % LANES, idx[k]
        max_value = int(sizes[ci]) - 2
        cum = x[lane] & ((1 << PRECISION) - 1)
        s = 0
        while s < max_value and int(cdfs[ci][s + 1]) <= cum:
            s += 1
        start = int(cdfs[ci][s])
        freq = int(cdfs[ci][s + 1]) - start
        x[lane] = freq * (x[lane] >> PRECISION) + cum - start
        if x[lane] < L:
            x[lane] = (x[lane] << 32) | words[wpos]
            wpos += 1
        if s == max_value:
            out.append(esc[epos])
            epos += 1
        else:
            out.append(s + int(offsets[ci]))
    assert wpos == len(words) and epos == len(esc) and all(v == L for v in x)
    return out


def ideal_bits(sym: Sequence[int], idx: Sequence[int], cdfs, sizes, offsets) -> float:
    """sum over the coded slots of log2(65536 / freq)."""
    steps, _ = _slots(sym, idx, cdfs, sizes, offsets)
    return sum(math.log2(65536.0 / freq) for _, freq in steps)
