"""Code-block bytes that no Grok encoder writes (oracle/make_golden_foreign.py,
tests/cpp/test_t1_foreign.cpp, tests/test_gpu_t1_foreign.py): a marker inside
a segment, a segment shorter than the decoder consumes, a segment ending in
0xFF, FF 80..8F pairs at any density.  Every byte comes from the xorshift64
below, so nothing here depends on a library's random generator.

  Gen(seed)                         the byte source
  FAMILIES[name](seed, length)      uniform / ffdense / carrymax / stuffed
  trim / marker_at / end_ff         edits of a valid segment
  block / valid_segment             a `_blocks`-like block and its oracle encode
  scan(seg)                         what the decoder's input side makes of a segment
  host_cases(oracle, n)             the CPU leg's case list (test_t1_foreign.cpp)
  overwrite_bodies(cs, pattern, seed)   packet bodies of an SOP + EPH stream
"""
import numpy as np

M64 = (1 << 64) - 1


class Gen:
    """xorshift64 (13, 7, 17); eight bytes per step, least significant first."""

    def __init__(self, seed):
        self.s = ((seed + 1) * 0x9E3779B97F4A7C15) & M64 or 88172645463325252
        self.buf = b""
        self.pos = 0

    def raw(self, n):
        """the next n bytes"""
        have = len(self.buf) - self.pos
        if have < n:
            s, out = self.s, []
            for _ in range((n - have + 7) // 8):
                s ^= (s << 13) & M64
                s ^= s >> 7
                s ^= (s << 17) & M64
                out.append(s.to_bytes(8, "little"))
            self.s = s
            self.buf = self.buf[self.pos:] + b"".join(out)
            self.pos = 0
        r = self.buf[self.pos:self.pos + n]
        self.pos += n
        return r


def uniform(seed, length):
    return Gen(seed).raw(length)


def ffdense(seed, length):
    """1/4 FF, 1/4 80..8F, the rest uniform (two draws a byte)"""
    r = Gen(seed).raw(2 * length)
    return bytes(0xFF if r[2 * i] & 3 == 0 else 0x80 | (r[2 * i + 1] & 15) if r[2 * i] & 3 == 1 else r[2 * i + 1]
                 for i in range(length))


def carrymax(seed, length):
    """FF 8x FF 8x ...: length // 2 carry events, the most a segment can hold"""
    r = Gen(seed).raw(length)
    return bytes(0xFF if i % 2 == 0 else 0x80 | (r[i] & 15) for i in range(length))


def stuffed(seed, length):
    """00..7F with 1/16 FF (never two in a row): no marker, no carry event"""
    r = Gen(seed).raw(2 * length)
    out = bytearray(length)
    for i in range(length):
        ff = r[2 * i] & 15 == 0 and not (i and out[i - 1] == 0xFF)
        out[i] = 0xFF if ff else r[2 * i + 1] & 0x7F
    return bytes(out)


FAMILIES = {"uniform": uniform, "ffdense": ffdense, "carrymax": carrymax, "stuffed": stuffed}
EDITS = ("trim", "marker_at", "end_ff")
KINDS = tuple(FAMILIES) + EDITS  # the kind numbers of test_t1_foreign.cpp


def trim(seg, t):
    """the last t bytes dropped (the pass count stays)"""
    assert 0 < t < len(seg)
    return seg[:len(seg) - t]


def marker_at(seg, p):
    """FF 90 at offsets p, p + 1"""
    assert 0 <= p and p + 2 <= len(seg)
    return seg[:p] + b"\xff\x90" + seg[p + 2:]


def end_ff(seg):
    assert seg
    return seg[:-1] + b"\xff"


def block(seed, h, w, nb):
    """A `_blocks`-like (h, w) int32 block of nb magnitude bit-planes: a
    triangle-wave structure plus noise that thins towards the top planes."""
    r = np.frombuffer(Gen(seed).raw(3 * h * w), np.uint8).reshape(h, w, 3).astype(np.int64)
    top = (1 << nb) - 1
    yy, xx = np.mgrid[0:h, 0:w]
    tri = np.abs((xx * 5 + yy * 3 + seed) % 32 - 16) * top // 16
    depth = r[..., 1] % nb  # bit-planes taken off this sample's noise
    mag = (tri >> 1) + (((r[..., 0] << 8 | r[..., 2]) * (top + 1) >> 16) >> depth)
    mag = np.minimum(mag, top)
    mag[(seed * 7) % h, (seed * 3) % w] = top  # the top plane is in use
    return (mag * (1 - 2 * (r[..., 1] >> 7))).astype(np.int32)


def valid_segment(oracle, seed, h, w, nb):
    """(bytes, numpasses, numbps, orient) of the oracle's 5/3 encode of block(seed, h, w, nb)"""
    orient = seed % 4
    data, passes, nbps = oracle.t1_encode_cblk(block(seed, h, w, nb), orient, 1, 0)
    assert nbps == nb and len(passes) == 3 * nb - 2 and len(data) == passes[-1][0]
    return data, len(passes), nbps, orient


def scan(seg):
    """(marker, carries): the offset of the first marker's FF (a FF followed
    by a byte above 8F; None: none) and the carry events before it (a FF
    followed by 80..8F), as t1_flat.h Unstuff reads the segment."""
    carries = 0
    for i in range(1, len(seg)):
        if seg[i - 1] == 0xFF:
            if seg[i] > 0x8F:
                return i - 1, carries
            carries += seg[i] >> 7
    return None, carries


# ------------------------------------------------------------ the CPU leg
NUMBPS = (1, 2, 16, 30)
LENGTHS = (1, 2, 3, 15, 16, 17, 63, 64, 65, 127, 128, 129, 16448)
SHAPES = ((1, 1), (4, 4), (7, 3), (1, 64), (64, 1), (64, 16), (47, 33), (64, 64))  # (h, w)
_BASES = ((47, 33, 1), (16, 16, 2), (47, 33, 16), (64, 64, 16), (64, 16, 9), (7, 3, 5))  # (h, w, nb) of the valid segments


def passes_of(nb, which):
    """pass count 1, middle, all of a block of nb bit-planes"""
    full = 3 * nb - 2
    return (1, max(1, full // 2), full)[which]


def host_cases(oracle, n):
    """n cases (kind, seed, param, base, seg, numbps, numpasses, w, h, orient,
    align): the four families at NUMBPS x pass counts x LENGTHS x alignments
    x SHAPES (each value list cycles at its own period) and the three edits
    of valid segments."""
    out = []
    for i in range(n):
        kind, align = KINDS[i % 7], i % 16
        if kind in FAMILIES:
            length = LENGTHS[i % 13]
            nb = NUMBPS[(i // 7) % 4]
            h, w = SHAPES[(i // 3) % 8]
            seg = FAMILIES[kind](i, length)
            out.append((kind, i, 0, b"", seg, nb, passes_of(nb, (i // 5) % 3), w, h, i % 4, align))
            continue
        h, w, nb = _BASES[(i // 7) % len(_BASES)]
        base, npass, nbps, orient = valid_segment(oracle, i, h, w, nb)
        assert len(base) >= 4
        if kind == "trim":
            ts = [t for t in (1, 2, 3, len(base) // 2, len(base) - 1) if 0 < t < len(base)]
            param = ts[(i // 49) % len(ts)]
            seg = trim(base, param)
        elif kind == "marker_at":
            param = (i * 37) % (len(base) - 1)
            seg = marker_at(base, param)
        else:
            param, seg = 0, end_ff(base)
        out.append((kind, i, param, base, seg, nbps, npass, w, h, orient, align))
    return out


def write_host_cases(path, cases):
    """u32 count, then per case eleven u32 (kind, seed, param, base length,
    length, numbps, numpasses, w, h, orient, align), the base and the bytes"""
    with open(path, "wb") as f:
        f.write(np.uint32(len(cases)).tobytes())
        for kind, seed, param, base, seg, nb, npass, w, h, orient, align in cases:
            f.write(np.array([KINDS.index(kind), seed, param, len(base), len(seg), nb, npass, w, h, orient, align],
                             "<u4").tobytes())
            f.write(base)
            f.write(seg)


# ------------------------------------------------------------ whole streams
def _rd16(b, o):
    return b[o] << 8 | b[o + 1]


def _rd32(b, o):
    return _rd16(b, o) << 16 | _rd16(b, o + 2)


def packet_bodies(cs):
    """[(start, end)] of every packet body of a stream written with SOP and
    EPH: the bytes after a packet's FF 92 up to the next FF 91, SOT or EOC
    (oracle/make_golden_markers.py split_packets: a Grok body holds no FF 91,
    a packet header no FF above 8F)."""
    pos = 2
    while _rd16(cs, pos) != 0xFF90:
        pos += 2 + _rd16(cs, pos + 2)
    out = []
    while _rd16(cs, pos) == 0xFF90:
        psot = _rd32(cs, pos + 6)
        end = pos + psot if psot else len(cs) - 2
        q = pos + 12
        while _rd16(cs, q) != 0xFF93:
            q += 2 + _rd16(cs, q + 2)
        i, sops = q + 2, []
        while i + 1 < end:
            if cs[i] == 0xFF and cs[i + 1] == 0x91:
                sops.append(i)
                i += 6
            else:
                i += 1
        assert not sops or sops[0] == q + 2, "every packet starts with SOP"
        for k, s in enumerate(sops):
            e = sops[k + 1] if k + 1 < len(sops) else end
            j = cs.index(b"\xff\x92", s + 6, e) + 2
            out.append((j, e))
        pos = end
    assert _rd16(cs, pos) == 0xFFD9 and pos + 2 == len(cs)
    return out


PATTERNS = ("noise", "sparse", "tailff")
_SPARSE = np.array([0xFF, 0x90, 0x8F, 0x80, 0x00, 0x00], np.uint8)


def overwrite_bodies(cs, pattern, seed):
    """The stream with its packet bodies overwritten in place -- every length
    and every header stays.  noise: every body byte uniform; sparse: a byte is
    replaced with probability 1/64 by FF, 90, 8F, 80, 00 or a uniform byte
    (three draws a byte); tailff: the last byte of every non-empty body
    becomes FF."""
    bodies = [(s, e) for s, e in packet_bodies(cs) if e > s]  # located before anything changes
    a = np.frombuffer(cs, np.uint8).copy()
    if pattern == "tailff":
        a[[e - 1 for _, e in bodies]] = 0xFF
        return a.tobytes()
    idx = np.concatenate([np.arange(s, e) for s, e in bodies])
    g = Gen(seed)
    if pattern == "noise":
        a[idx] = np.frombuffer(g.raw(len(idx)), np.uint8)
    elif pattern == "sparse":
        r = np.frombuffer(g.raw(3 * len(idx)), np.uint8).reshape(-1, 3)
        new = np.where(r[:, 1] % 6 == 5, r[:, 2], _SPARSE[r[:, 1] % 6])
        a[idx] = np.where(r[:, 0] < 4, new, a[idx])
    else:
        raise ValueError(pattern)
    return a.tobytes()
