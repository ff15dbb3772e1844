"""CPU restatement of the BC6H granule-sorted field split, layout version 1 (docs/BC6H_FORMAT.md), for the tests and tools
(numpy, no library).

It holds the format's field table, the record packing (`record_fields`, `decorrelated`), the granule sort, the streams and the
main / tail split, and a small BC6H decoder built from the same field table.  The decoder exists only to pin the table
against an independent one (tests/test_bc6h.py); it is no library feature.

`kernel_tables()` prints the record permutation as the (source bit, destination bit, length) runs that
csrc/bc6h_fields.h carries; tests/test_bc6h.py checks that the header holds exactly these runs.
"""
from __future__ import annotations

import numpy as np

GRANULE = 1024
CLASSES = 15                      # 14 modes + the reserved encodings (moved unchanged)
RESERVED = 14
STREAM_OFF = (0, 8, 10, 11, 12, 13, 14, 15)
STREAM_WIDTH = (8, 2, 1, 1, 1, 1, 1, 1)
LAYOUT_VERSION = 1
HEADER_WORD = 0x4 | (((0xD175 << 12) | LAYOUT_VERSION) << 4)   # TransformFormat::Bc6H = 4, vendor tag, layout version

# ---- the field table (D3D11 BC6H) ------------------------------------------------------------------------------------
# Class k's block layout, LSB first.  "m2"/"m5": mode bits, "d5": partition, "r0:9-0": bits 9..0 of red endpoint 0 (w),
# lowest bit stored first; "r0:R10-15": bits 10..15 stored in reversed order (bit 15 first).  Endpoints 0..3 = w, x, y, z.
# The index bits fill the rest of the block.
MODE_BITS = (0b00, 0b01, 2, 6, 10, 14, 18, 22, 26, 30, 3, 7, 11, 15)   # byte0 & 0x3 (classes 0, 1) or byte0 & 0x1F
LAYOUTS = (
    "m2 g2:4 b2:4 b3:4 r0:9-0 g0:9-0 b0:9-0 r1:4-0 g3:4 g2:3-0 g1:4-0 b3:0 g3:3-0 b1:4-0 b3:1 b2:3-0 r2:4-0 b3:2 r3:4-0 b3:3 d5",
    "m2 g2:5 g3:4 g3:5 r0:6-0 b3:0 b3:1 b2:4 g0:6-0 b2:5 b3:2 g2:4 b0:6-0 b3:3 b3:5 b3:4 r1:5-0 g2:3-0 g1:5-0 g3:3-0 "
    "b1:5-0 b2:3-0 r2:5-0 r3:5-0 d5",
    "m5 r0:9-0 g0:9-0 b0:9-0 r1:4-0 r0:10 g2:3-0 g1:3-0 g0:10 b3:0 g3:3-0 b1:3-0 b0:10 b3:1 b2:3-0 r2:4-0 b3:2 r3:4-0 b3:3 d5",
    "m5 r0:9-0 g0:9-0 b0:9-0 r1:3-0 r0:10 g3:4 g2:3-0 g1:4-0 g0:10 g3:3-0 b1:3-0 b0:10 b3:1 b2:3-0 r2:3-0 b3:0 b3:2 r3:3-0 "
    "g2:4 b3:3 d5",
    "m5 r0:9-0 g0:9-0 b0:9-0 r1:3-0 r0:10 b2:4 g2:3-0 g1:3-0 g0:10 b3:0 g3:3-0 b1:4-0 b0:10 b2:3-0 r2:3-0 b3:1 b3:2 r3:3-0 "
    "b3:4 b3:3 d5",
    "m5 r0:8-0 b2:4 g0:8-0 g2:4 b0:8-0 b3:4 r1:4-0 g3:4 g2:3-0 g1:4-0 b3:0 g3:3-0 b1:4-0 b3:1 b2:3-0 r2:4-0 b3:2 r3:4-0 b3:3 d5",
    "m5 r0:7-0 g3:4 b2:4 g0:7-0 b3:2 g2:4 b0:7-0 b3:3 b3:4 r1:5-0 g2:3-0 g1:4-0 b3:0 g3:3-0 b1:4-0 b3:1 b2:3-0 r2:5-0 r3:5-0 d5",
    "m5 r0:7-0 b3:0 b2:4 g0:7-0 g2:5 g2:4 b0:7-0 g3:5 b3:4 r1:4-0 g3:4 g2:3-0 g1:5-0 g3:3-0 b1:4-0 b3:1 b2:3-0 r2:4-0 b3:2 "
    "r3:4-0 b3:3 d5",
    "m5 r0:7-0 b3:1 b2:4 g0:7-0 b2:5 g2:4 b0:7-0 b3:5 b3:4 r1:4-0 g3:4 g2:3-0 g1:4-0 b3:0 g3:3-0 b1:5-0 b2:3-0 r2:4-0 b3:2 "
    "r3:4-0 b3:3 d5",
    "m5 r0:5-0 g3:4 b3:0 b3:1 b2:4 g0:5-0 g2:5 b2:5 b3:2 g2:4 b0:5-0 g3:5 b3:3 b3:5 b3:4 r1:5-0 g2:3-0 g1:5-0 g3:3-0 b1:5-0 "
    "b2:3-0 r2:5-0 r3:5-0 d5",
    "m5 r0:9-0 g0:9-0 b0:9-0 r1:9-0 g1:9-0 b1:9-0",
    "m5 r0:9-0 g0:9-0 b0:9-0 r1:8-0 r0:10 g1:8-0 g0:10 b1:8-0 b0:10",
    "m5 r0:9-0 g0:9-0 b0:9-0 r1:7-0 r0:R10-11 g1:7-0 g0:R10-11 b1:7-0 b0:R10-11",
    "m5 r0:9-0 g0:9-0 b0:9-0 r1:3-0 r0:R10-15 g1:3-0 g0:R10-15 b1:3-0 b0:R10-15",
)
# endpoint precision and the widths of the red / green / blue delta (or, untransformed, second-endpoint) fields
WIDTHS = ((10, 5, 5, 5), (7, 6, 6, 6), (11, 5, 4, 4), (11, 4, 5, 4), (11, 4, 4, 5), (9, 5, 5, 5), (8, 6, 5, 5), (8, 5, 6, 5),
          (8, 5, 5, 6), (6, 6, 6, 6), (10, 10, 10, 10), (11, 9, 9, 9), (12, 8, 8, 8), (16, 4, 4, 4))
TRANSFORMED = tuple(k not in (9, 10) for k in range(14))   # x, y, z stored as deltas to w


def two_region(k: int) -> bool:
    return k <= 9


def mode_bit_count(k: int) -> int:
    return 2 if k <= 1 else 5


def field_width(k: int, ch: int, e: int) -> int:
    return WIDTHS[k][0] if e == 0 else WIDTHS[k][1 + ch]


def n_endpoints(k: int) -> int:
    return 4 if two_region(k) else 2


def _parse(k: int):
    """{(ch, e): [block bit of value bit 0, 1, ...]}, partition bit positions, first index bit"""
    fields: dict[tuple[int, int], dict[int, int]] = {}
    part: list[int] = []
    pos = 0
    for tok in LAYOUTS[k].split():
        if tok[0] == "m":
            pos += int(tok[1:])
            continue
        if tok[0] == "d":
            part = list(range(pos, pos + 5))
            pos += 5
            continue
        name, bits = tok.split(":")
        ch, e = "rgb".index(name[0]), int(name[1])
        if bits.startswith("R"):
            lo, hi = (int(x) for x in bits[1:].split("-"))
            order = list(range(hi, lo - 1, -1))
        elif "-" in bits:
            hi, lo = (int(x) for x in bits.split("-"))
            order = list(range(lo, hi + 1))
        else:
            order = [int(bits)]
        d = fields.setdefault((ch, e), {})
        for b in order:
            assert b not in d, (k, tok)
            d[b] = pos
            pos += 1
    out = {}
    for key, d in fields.items():
        w = field_width(k, *key)
        assert sorted(d) == list(range(w)), (k, key, sorted(d))
        out[key] = [d[b] for b in range(w)]
    assert len(out) == 3 * n_endpoints(k), k
    return out, part, pos


FIELDS, PARTITION, INDEX_START = [], [], []
for _k in range(14):
    _f, _p, _i = _parse(_k)
    FIELDS.append(_f)
    PARTITION.append(_p)
    INDEX_START.append(_i)
    assert _i == (82 if two_region(_k) else 65), _k
    assert sum(len(v) for v in _f.values()) == (75 if _k <= 1 else 72 if two_region(_k) else 60), _k


def block_class(byte0):
    """class 0..14 of a block (or of a record: byte 0 keeps the mode bits), from byte 0; vectorised"""
    b = np.asarray(byte0, dtype=np.int64) & 0x1F
    two = b & 3
    k = np.where(two == 2, 2 + (b >> 2), np.where(b >> 2 < 4, 10 + (b >> 2), RESERVED))
    return np.where(two < 2, two, k).astype(np.int64)


# ---- the record -------------------------------------------------------------------------------------------------------
# Layout candidates (docs/BC6H_FORMAT.md section 4): "a" = no record (bytes in block order), "b" = fields split, endpoints
# whole, "c" = b + the high byte of every base endpoint of 8 bits or more at the top of the record, "d" = c + red and blue
# as differences to green.  Version 1 ships "d".
SHIPPED = "d"


def high_byte_fields(k: int) -> list[tuple[int, int]]:
    """(ch, e) of the base endpoints whose top 8 bits move to the top of the record: w, and in the untransformed one-region
    mode x too, when the field has 8 bits or more; order R0 (R1) G0 (G1) B0 (B1)"""
    es = [0, 1] if k == 10 else [0]
    return [(ch, e) for ch in range(3) for e in es if field_width(k, ch, e) >= 8]


def decorrelated(k: int) -> list[int]:
    """endpoints whose red and blue are stored as differences to green (modulo the field width)"""
    if k >= 14:
        return []
    return list(range(n_endpoints(k))) if not TRANSFORMED[k] else [0]


def record_fields(k: int, variant: str = SHIPPED):
    """{(ch, e): [record bit of value bit 0, 1, ...]} and the record's full permutation: perm[record bit] = block bit"""
    mb = mode_bit_count(k)
    order: list[int] = list(range(mb)) + PARTITION[k] + list(range(INDEX_START[k], 128))
    rec_of: dict[tuple[int, int], list[int]] = {}
    hb = high_byte_fields(k) if variant in ("c", "d") else []
    for ch in range(3):
        for e in range(n_endpoints(k)):
            src = FIELDS[k][(ch, e)]
            low = src[:-8] if (ch, e) in hb else src
            rec_of[(ch, e)] = list(range(len(order), len(order) + len(low)))
            order += low
    for key in hb:
        src = FIELDS[k][key]
        rec_of[key] = rec_of[key] + list(range(len(order), len(order) + 8))
        order += src[-8:]
    assert sorted(order) == list(range(128)), k
    return rec_of, np.array(order, dtype=np.int64)


def _bits(blocks: np.ndarray) -> np.ndarray:
    return np.unpackbits(blocks.reshape(-1, 16), axis=1, bitorder="little")


def _bytes(bits: np.ndarray) -> np.ndarray:
    return np.packbits(bits, axis=1, bitorder="little")


def _value(bits: np.ndarray, pos) -> np.ndarray:
    v = np.zeros(bits.shape[0], dtype=np.int64)
    for i, p in enumerate(pos):
        v |= bits[:, p].astype(np.int64) << i
    return v


def _store(bits: np.ndarray, pos, v: np.ndarray) -> None:
    for i, p in enumerate(pos):
        bits[:, p] = (v >> i) & 1


def records(blocks: np.ndarray, variant: str = SHIPPED) -> np.ndarray:
    """(n, 16) blocks -> (n, 16) records"""
    blocks = np.asarray(blocks, dtype=np.uint8).reshape(-1, 16)
    out = blocks.copy()
    if variant == "a" or blocks.shape[0] == 0:
        return out
    cls = block_class(blocks[:, 0])
    for k in range(14):
        sel = np.nonzero(cls == k)[0]
        if sel.size == 0:
            continue
        rec_of, perm = record_fields(k, variant)
        rb = _bits(blocks[sel])[:, perm]
        if variant == "d":
            for e in decorrelated(k):
                w = field_width(k, 1, e)
                g = _value(rb, rec_of[(1, e)])
                for ch in (0, 2):
                    _store(rb, rec_of[(ch, e)], (_value(rb, rec_of[(ch, e)]) - g) & ((1 << w) - 1))
        out[sel] = _bytes(rb)
    return out


def blocks_of_records(recs: np.ndarray, variant: str = SHIPPED) -> np.ndarray:
    recs = np.asarray(recs, dtype=np.uint8).reshape(-1, 16)
    out = recs.copy()
    if variant == "a" or recs.shape[0] == 0:
        return out
    cls = block_class(recs[:, 0])
    for k in range(14):
        sel = np.nonzero(cls == k)[0]
        if sel.size == 0:
            continue
        rec_of, perm = record_fields(k, variant)
        rb = _bits(recs[sel])
        if variant == "d":
            for e in decorrelated(k):
                w = field_width(k, 1, e)
                g = _value(rb, rec_of[(1, e)])
                for ch in (0, 2):
                    _store(rb, rec_of[(ch, e)], (_value(rb, rec_of[(ch, e)]) + g) & ((1 << w) - 1))
        bb = np.empty_like(rb)
        bb[:, perm] = rb
        out[sel] = _bytes(bb)
    return out


# ---- granules and streams ---------------------------------------------------------------------------------------------
def _part_forward(blocks: np.ndarray, variant: str) -> np.ndarray:
    n = blocks.shape[0]
    out = np.empty(16 * n, dtype=np.uint8)
    if n == 0:
        return out
    rec = records(blocks, variant)
    order = np.concatenate([g0 + np.argsort(block_class(blocks[g0:g0 + GRANULE, 0]), kind="stable")
                            for g0 in range(0, n, GRANULE)])
    srt = rec[order]
    out[0:8 * n] = srt[:, 1:9].reshape(-1)
    out[8 * n:10 * n] = srt[:, 9:11].reshape(-1)
    for s in range(5):
        out[(10 + s) * n:(11 + s) * n] = srt[:, 11 + s]
    out[15 * n:] = rec[:, 0]
    return out


def _part_inverse(soa: np.ndarray) -> tuple[np.ndarray, np.ndarray]:
    """records in block order"""
    n = soa.size // 16
    rec = np.empty((n, 16), dtype=np.uint8)
    if n == 0:
        return rec
    f = soa[15 * n:]
    order = np.concatenate([g0 + np.argsort(block_class(f[g0:g0 + GRANULE]), kind="stable") for g0 in range(0, n, GRANULE)])
    srt = np.empty((n, 16), dtype=np.uint8)
    srt[:, 1:9] = soa[0:8 * n].reshape(n, 8)
    srt[:, 9:11] = soa[8 * n:10 * n].reshape(n, 2)
    for s in range(5):
        srt[:, 11 + s] = soa[(10 + s) * n:(11 + s) * n]
    rec[order] = srt
    rec[:, 0] = f
    return rec


def transform(aos: np.ndarray, variant: str = SHIPPED) -> np.ndarray:
    a = np.asarray(aos, dtype=np.uint8).reshape(-1)
    assert a.size % 16 == 0
    n = a.size // 16
    main = n - n % GRANULE
    blocks = a.reshape(n, 16)
    return np.concatenate([_part_forward(blocks[:main], variant), _part_forward(blocks[main:], variant)])


def untransform(soa: np.ndarray, variant: str = SHIPPED) -> np.ndarray:
    s = np.asarray(soa, dtype=np.uint8).reshape(-1)
    assert s.size % 16 == 0
    n = s.size // 16
    main = n - n % GRANULE
    rec = np.concatenate([_part_inverse(s[:16 * main]), _part_inverse(s[16 * main:])])
    return blocks_of_records(rec, variant).reshape(-1)


def stream_offsets(n: int) -> list[tuple[int, int]]:
    """[(byte offset, bytes)] of the main part's eight streams and of the tail part, for n blocks"""
    main = n - n % GRANULE
    return [(o * main, w * main) for o, w in zip(STREAM_OFF, STREAM_WIDTH)] + [(16 * main, 16 * (n - main))]


def shard_pieces(total: int, first: int, num: int):
    """what dxtlt_bc6h_shard_pieces answers: (global offsets, local offsets, bytes), nine entries each"""
    main_total = total - total % GRANULE
    end = first + num
    main_count = 0 if first >= main_total else min(end, main_total) - first
    g = [o * main_total + w * first for o, w in zip(STREAM_OFF, STREAM_WIDTH)] + [16 * main_total]
    lo = [o * main_count for o in STREAM_OFF] + [16 * main_count]
    nb = [w * main_count for w in STREAM_WIDTH] + [16 * (num - main_count)]
    return g, lo, nb


# ---- the kernels' tables ----------------------------------------------------------------------------------------------
def runs(k: int, variant: str = SHIPPED) -> list[tuple[int, int, int]]:
    """the record permutation of class k as (block bit, record bit, length) runs, none crossing a dword on either side"""
    _, perm = record_fields(k, variant)
    out: list[list[int]] = []
    for dst, src in enumerate(perm.tolist()):
        if out and out[-1][0] + out[-1][2] == src and out[-1][1] + out[-1][2] == dst and src % 32 != 0 and dst % 32 != 0:
            out[-1][2] += 1
        else:
            out.append([src, dst, 1])
    return [tuple(r) for r in out]


def record_pieces(k: int, ch: int, e: int) -> tuple[int, int, int, int]:
    """(low run's first record bit, its length, high byte's first record bit, its length) of a field of the record"""
    rec_of, _ = record_fields(k)
    pos = rec_of[(ch, e)]
    hb = (ch, e) in high_byte_fields(k)
    low = pos[:-8] if hb else pos
    assert low == list(range(low[0], low[0] + len(low))) if low else hb
    return (low[0] if low else 0, len(low), pos[-8] if hb else 0, 8 if hb else 0)


def kernel_tables() -> str:
    """the generated part of csrc/bc6h_fields.h"""
    lines = []
    for k in range(14):
        rs = ", ".join("{%d, %d, %d}" % r for r in runs(k))
        ds = ", ".join("{%d, {%s}}" % (field_width(k, 1, e), ", ".join("{%d, %d, %d, %d}" % record_pieces(k, ch, e) for ch in range(3)))
                       for e in decorrelated(k))
        lines.append(f"template <> struct Tab<{k}> {{")
        lines.append(f"    static constexpr Run runs[] = {{{rs}}};")
        lines.append(f"    static constexpr Dec dec[] = {{{ds}}};")
        lines.append("};")
    return "\n".join(lines) + "\n"


# ---- a BC6H decoder from the same field table (pins the table; not a library feature) -------------------------------
PARTITIONS = (0xCCCC, 0x8888, 0xEEEE, 0xECC8, 0xC880, 0xFEEC, 0xFEC8, 0xEC80, 0xC800, 0xFFEC, 0xFE80, 0xE800, 0xFFE8,
              0xFF00, 0xFFF0, 0xF000, 0xF710, 0x008E, 0x7100, 0x08CE, 0x008C, 0x7310, 0x3100, 0x8CCE, 0x088C, 0x3110,
              0x6666, 0x366C, 0x17E8, 0x0FF0, 0x718E, 0x399C)   # bit i: subset of pixel i
ANCHOR2 = (15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 2, 8, 2, 2, 8, 8, 15, 2, 8, 2, 2, 8, 8, 2, 2)
WEIGHTS3 = (0, 9, 18, 27, 37, 46, 55, 64)
WEIGHTS4 = (0, 4, 9, 13, 17, 21, 26, 30, 34, 38, 43, 47, 51, 55, 60, 64)


def _sext(v: np.ndarray, w: int) -> np.ndarray:
    return np.where(v >= 1 << (w - 1), v - (1 << w), v)


def _unquantize(c: np.ndarray, bits: int, signed: bool) -> np.ndarray:
    if not signed:
        if bits >= 15:
            return c
        return np.where(c == 0, 0, np.where(c == (1 << bits) - 1, 0xFFFF, ((c << 16) + 0x8000) >> bits))
    if bits >= 16:
        return c
    neg = c < 0
    a = np.abs(c)
    u = np.where(a == 0, 0, np.where(a >= (1 << (bits - 1)) - 1, 0x7FFF, ((a << 15) + 0x4000) >> (bits - 1)))
    return np.where(neg, -u, u)


def _finish(c: np.ndarray, signed: bool) -> np.ndarray:
    if not signed:
        return (c * 31) >> 6
    return np.where(c < 0, -(((-c) * 31) >> 5), (c * 31) >> 5)


def decode(blocks: np.ndarray, signed: bool = False) -> np.ndarray:
    """(n, 16) BC6H blocks -> (n, 16 pixels, 3) half-float bit patterns (uint16); reserved modes decode to zero"""
    blocks = np.asarray(blocks, dtype=np.uint8).reshape(-1, 16)
    n = blocks.shape[0]
    out = np.zeros((n, 16, 3), dtype=np.uint16)
    cls = block_class(blocks[:, 0])
    for k in range(14):
        sel = np.nonzero(cls == k)[0]
        if sel.size == 0:
            continue
        bits = _bits(blocks[sel])
        m = sel.size
        epb = WIDTHS[k][0]
        ne = n_endpoints(k)
        ep = np.zeros((m, ne, 3), dtype=np.int64)
        for ch in range(3):
            w0 = _value(bits, FIELDS[k][(ch, 0)])
            ep[:, 0, ch] = w0
            for e in range(1, ne):
                v = _value(bits, FIELDS[k][(ch, e)])
                if TRANSFORMED[k]:
                    v = (w0 + _sext(v, field_width(k, ch, e))) & ((1 << epb) - 1)
                ep[:, e, ch] = v
        if signed:
            ep = _sext(ep, epb)
        ep = _unquantize(ep, epb, signed)
        rows = np.arange(m)
        if two_region(k):
            part = _value(bits, PARTITION[k])
            mask = np.array(PARTITIONS, dtype=np.int64)[part]
            anchor2 = np.array(ANCHOR2, dtype=np.int64)[part]
        ib = 3 if two_region(k) else 4
        weights = np.array(WEIGHTS3 if ib == 3 else WEIGHTS4, dtype=np.int64)
        cursor = np.full(m, INDEX_START[k], dtype=np.int64)   # anchors store one bit fewer: a cursor per block
        for px in range(16):
            if two_region(k):
                subset = (mask >> px) & 1
                anchor = (anchor2 == px) | (px == 0)
            else:
                subset = np.zeros(m, dtype=np.int64)
                anchor = np.full(m, px == 0)
            nb = np.where(anchor, ib - 1, ib)
            idx = np.zeros(m, dtype=np.int64)
            for b in range(ib):
                bit = bits[rows, np.minimum(cursor + b, 127)].astype(np.int64)
                idx |= np.where(b < nb, bit << b, 0)
            cursor += nb
            wgt = weights[idx][:, None]
            e0 = ep[rows, 2 * subset]
            e1 = ep[rows, 2 * subset + 1]
            val = (e0 * (64 - wgt) + e1 * wgt + 32) >> 6
            out[sel, px] = (_finish(val, signed) & 0xFFFF).astype(np.uint16)
    return out


def pack_block(k: int, ep: dict, partition: int = 0, index_bits: int = 0) -> np.ndarray:
    """one block of class k from field values ep[(ch, e)] (x, y, z as stored: deltas in the transformed modes), the
    partition and the index bits (an integer, bit 0 = the first index bit); 16 bytes"""
    bits = np.zeros(128, dtype=np.uint8)
    mb = mode_bit_count(k)
    for i in range(mb):
        bits[i] = (MODE_BITS[k] >> i) & 1
    for i, p in enumerate(PARTITION[k]):
        bits[p] = (partition >> i) & 1
    for i in range(128 - INDEX_START[k]):
        bits[INDEX_START[k] + i] = (index_bits >> i) & 1
    for key, pos in FIELDS[k].items():
        for i, p in enumerate(pos):
            bits[p] = (ep[key] >> i) & 1
    return np.packbits(bits, bitorder="little")


def dds_dx10(payload: bytes, width: int, height: int, dxgi: int, mips: int = 1) -> bytes:
    """a minimal DX10 DDS file around a BCn payload of 16-byte blocks"""
    import struct

    linear = max(1, (width + 3) // 4) * max(1, (height + 3) // 4) * 16
    flags = 0x1 | 0x2 | 0x4 | 0x1000 | 0x80000 | (0x20000 if mips > 1 else 0)
    caps = 0x1000 | (0x400008 if mips > 1 else 0)
    hdr = struct.pack("<7I44x", 124, flags, height, width, linear, 0, mips)
    pf = struct.pack("<II4s20x", 32, 0x4, b"DX10")
    hdr += pf + struct.pack("<5I", caps, 0, 0, 0, 0)
    dx10 = struct.pack("<5I", dxgi, 3, 0, 1, 0)
    return b"DDS " + hdr + dx10 + payload
