"""TEST INFRASTRUCTURE ONLY: pure-Python restatement of the segmented device-coder format HRW2, written from its
specification (DESIGN.md "Device rANS coder", HRW2) on top of tests/wrans_ref.py, not from the C++.

One string per image and pass, little endian:
    "HRW2" | uint32 n | uint32 R | uint32 S | S x {uint32 esc_end, uint32 words_end} | S x 64 x uint64 lane states
    | esc_end[S-1] x int32 | words_end[S-1] x uint32
* S = max(1, ceil(n / (64 R))); segment s owns the coded symbols [64 R s, min(n, 64 R (s + 1)));
* a segment is coded exactly as HRW1 codes a whole string of its symbols: its states, escapes and payload words are
  those parts of ``wrans_ref.encode`` on the sub-lists; the directory holds the cumulative counts through segment s.
"""
from __future__ import annotations

import struct
from typing import List, Sequence

import wrans_ref

MAGIC = b"HRW2"
LANES = wrans_ref.LANES


def segments(n: int, R: int) -> int:
    return max(1, -(-n // (LANES * R)))


def seg_range(n: int, R: int, s: int) -> range:
    return range(min(n, LANES * R * s), min(n, LANES * R * (s + 1)))


def encode(sym: Sequence[int], idx: Sequence[int], cdfs, sizes, offsets, R: int) -> bytes:
    """``sym`` / ``idx``: the coded symbols and their CDF rows, in coded-symbol order; ``R`` rows per segment."""
    n = len(sym)
    assert R >= 1
    S = segments(n, R)
    directory, states, esc, words = [], [], [], []
    for s in range(S):
        k = seg_range(n, R, s)
        _, st, e, w = wrans_ref.parse(wrans_ref.encode(sym[k.start:k.stop], idx[k.start:k.stop], cdfs, sizes, offsets))
        states += st
        esc += e
        words += w
        directory += [len(esc), len(words)]
    return (MAGIC + struct.pack("<3I", n, R, S) + struct.pack(f"<{2 * S}I", *directory)
            + struct.pack(f"<{LANES * S}Q", *states) + struct.pack(f"<{len(esc)}i", *esc)
            + struct.pack(f"<{len(words)}I", *words))


def parse2(data: bytes):
    """(n, R, S, directory, segs) of a well-formed string: ``directory`` the S (esc_end, words_end) pairs, ``segs`` the
    S (states, escapes, words) triples."""
    assert data[:4] == MAGIC and len(data) >= 16
    n, R, S = struct.unpack_from("<3I", data, 4)
    assert R >= 1 and S == segments(n, R)
    flat = struct.unpack_from(f"<{2 * S}I", data, 16)
    directory = [(flat[2 * s], flat[2 * s + 1]) for s in range(S)]
    n_esc, n_words = directory[-1]
    body = 16 + 8 * S + 8 * LANES * S
    assert len(data) == body + 4 * (n_esc + n_words)
    states = struct.unpack_from(f"<{LANES * S}Q", data, 16 + 8 * S)
    esc = struct.unpack_from(f"<{n_esc}i", data, body)
    words = struct.unpack_from(f"<{n_words}I", data, body + 4 * n_esc)
    segs, e0, w0 = [], 0, 0
    for s, (e1, w1) in enumerate(directory):
        assert e0 <= e1 and w0 <= w1
        segs.append((list(states[LANES * s:LANES * (s + 1)]), list(esc[e0:e1]), list(words[w0:w1])))
        e0, w0 = e1, w1
    return n, R, S, directory, segs


def hrw1_of_segment(n_s: int, seg) -> bytes:
    """The HRW1 string that holds one parsed segment of ``n_s`` coded symbols."""
    states, esc, words = seg
    return (wrans_ref.MAGIC + struct.pack("<3I", n_s, len(esc), len(words)) + struct.pack("<64Q", *states)
            + struct.pack(f"<{len(esc)}i", *esc) + struct.pack(f"<{len(words)}I", *words))


def decode(data: bytes, idx: Sequence[int], cdfs, sizes, offsets) -> List[int]:
    n, R, S, _, segs = parse2(data)
    assert n == len(idx)
    out: List[int] = []
    for s in range(S):
        k = seg_range(n, R, s)
        out += wrans_ref.decode(hrw1_of_segment(len(k), segs[s]), idx[k.start:k.stop], cdfs, sizes, offsets)
    return out
