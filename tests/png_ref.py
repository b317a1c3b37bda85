"""A scalar restatement of the PNG files mujoco_manip_amd/csrc/mmx_png.hip writes, and the case images of
tests/test_png_stream.py.

The encoder is deterministic (greedy parse with two match candidates, one final fixed-Huffman block, IDAT chunks
of 512 bytes), so the whole file is a function of the pixels and this module predicts every byte of it.  It is
written the way the format documents state it, one scanline and one token after the other: no row streams, no
scan, no dword assembly, no chunk-position arithmetic.  The length and distance tables are RFC 1951 section
3.2.5's, typed in; Adler-32 and CRC-32 are zlib's.

    parse_row(line, above) -> tokens         the greedy parse of one scanline (filter byte included)
    deflate(tokens) -> (block bytes, bits)   one final fixed-Huffman block
    encode(image) -> (file, tokens, zlib_len, nbits)
    tokens_of(zlib_bytes) -> tokens          a fixed-Huffman inflater that keeps the tokens
    first_difference(...)                    names the first differing token of two streams by row and position
    chunks(png), round_trip(png, image)      the decoder-side checks of tests/test_png.py

Tokens are ('L', byte) and ('M', length, distance).  Everything is seeded; nothing is read from disk."""
import functools
import io
import struct
import zlib

import numpy as np

MAX_MATCH = 258
CHUNK = 512         # IDAT data bytes per chunk
MAX_HEIGHT = 1024   # mmx_png_bound refuses more rows
MAX_WIDTH = 10922   # 3 W + 1 <= 32768, deflate's largest distance

# RFC 1951 section 3.2.5: symbols 257..285 (lengths) and 0..29 (distances), base value and extra bits
LEN_BASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195,
            227, 258]
LEN_EXTRA = [0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0]
DIST_BASE = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073,
             4097, 6145, 8193, 12289, 16385, 24577]
DIST_EXTRA = [0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13]


def _last_at_most(bases, v):
    return max(k for k, b in enumerate(bases) if b <= v)


def length_symbol(n):
    """Match length 3..258 -> (symbol 257..285, extra bits, extra value): the last row of the table whose base is
    <= n (258 has a row of its own, symbol 285)."""
    k = _last_at_most(LEN_BASE, n)
    return 257 + k, LEN_EXTRA[k], n - LEN_BASE[k]


def distance_code(d):
    """Distance 1..32768 -> (code 0..29, extra bits, extra value)."""
    k = _last_at_most(DIST_BASE, d)
    return k, DIST_EXTRA[k], d - DIST_BASE[k]


def _rev(v, n):
    return int(format(v, f"0{n}b")[::-1], 2)


def literal_code(sym):
    """Fixed Huffman code of literal / length symbol 0..287 (RFC 1951 section 3.2.6) -> (code as it enters an
    LSB-first stream, i.e. bit-reversed, bits)."""
    if sym < 144:
        return _rev(0b00110000 + sym, 8), 8
    if sym < 256:
        return _rev(0b110010000 + sym - 144, 9), 9
    if sym < 280:
        return _rev(sym - 256, 7), 7
    return _rev(0b11000000 + sym - 280, 8), 8


_LIT = [literal_code(s) for s in range(288)]
_LEN = {n: length_symbol(n) for n in range(3, MAX_MATCH + 1)}


def token_bits(tok):
    """Bits of one token in the block."""
    if tok[0] == "L":
        return _LIT[tok[1]][1]
    sym, eb, _ = _LEN[tok[1]]
    return _LIT[sym][1] + eb + 5 + distance_code(tok[2])[1]


# ---------------------------------------------------------------------------------------------------- the parse
def parse_row_plain(line, above):
    """The greedy parse as the comment at the top of mmx_png.hip states it, byte by byte.  `line` and `above` are
    scanlines with their filter byte (above: None in row 0).  At scanline position t two candidates are measured,
    both at most min(258, len - t) long: the bytes 3 back (the same channel of the pixel before; only inside the
    row, t >= 3) and the bytes one scanline back (distance len(line)).  The longer wins, ties go to distance 3; a
    match is taken from length 3, otherwise one literal."""
    line = bytes(line)
    above = None if above is None else bytes(above)
    n, t, out = len(line), 0, []
    while t < n:
        lim = min(MAX_MATCH, n - t)
        m1 = m2 = 0
        if t >= 3:
            while m1 < lim and line[t + m1] == line[t + m1 - 3]:
                m1 += 1
        if above is not None:
            while m2 < lim and line[t + m2] == above[t + m2]:
                m2 += 1
        if max(m1, m2) >= 3:
            out.append(("M", m1, 3) if m1 >= m2 else ("M", m2, n))
            t += max(m1, m2)
        else:
            out.append(("L", line[t]))
            t += 1
    return out


def _run_from(eq):
    """eq: bool [n] -> the number of consecutive True values starting at each index."""
    n = len(eq)
    idx = np.arange(n)
    stop = np.minimum.accumulate(np.where(eq, n, idx)[::-1])[::-1]  # the next False at or after each index
    return stop - idx


def parse_row(line, above):
    """parse_row_plain with the two common-prefix searches done by numpy for the whole row at once (the choice at
    position t depends on nothing but t, so the greedy walk only visits the positions it reaches)."""
    line = np.asarray(line, np.uint8)
    n = len(line)
    near = np.zeros(n, bool)
    near[3:] = line[3:] == line[:-3]
    m1 = np.minimum(_run_from(near), MAX_MATCH)
    m2 = np.zeros(n, np.int64) if above is None else np.minimum(_run_from(line == np.asarray(above, np.uint8)), MAX_MATCH)
    m = np.maximum(m1, m2)
    starts = np.flatnonzero(m >= 3).tolist()
    is_near, m, raw = (m1 >= m2).tolist(), m.tolist(), line.tolist()
    out, t, k = [], 0, 0
    while t < n:
        while k < len(starts) and starts[k] < t:
            k += 1
        s = starts[k] if k < len(starts) else n
        out.extend(("L", b) for b in raw[t:s])
        if s < n:
            out.append(("M", m[s], 3 if is_near[s] else n))
            s += m[s]
        t = s
    return out


def scanlines(image):
    """[H, W, 3] uint8 -> [H, 3 W + 1]: filter byte 0, then the row's bytes."""
    image = np.asarray(image, np.uint8)
    h, w, _ = image.shape
    lines = np.zeros((h, 3 * w + 1), np.uint8)
    lines[:, 1:] = image.reshape(h, 3 * w)
    return lines


def parse_image(image, parse=parse_row):
    lines = scanlines(image)
    out = []
    for r in range(len(lines)):
        out.extend(parse(lines[r], lines[r - 1] if r else None))
    return out


# ---------------------------------------------------------------------------------------------------- the block
class _Bits:
    """LSB-first bit writer: bits go into a Python integer, whole bytes leave it."""

    def __init__(self):
        self.acc, self.n, self.total, self.out = 0, 0, 0, bytearray()

    def put(self, v, nb):
        self.acc |= v << self.n
        self.n += nb
        self.total += nb
        if self.n >= 64:
            self.out += (self.acc & 0xFFFFFFFFFFFFFFFF).to_bytes(8, "little")
            self.acc >>= 64
            self.n -= 64

    def done(self):
        return bytes(self.out) + self.acc.to_bytes((self.n + 7) // 8, "little")


def deflate(tokens, length_rule=None):
    """One final fixed-Huffman block of the tokens -> (bytes, bit count).  BFINAL = 1, BTYPE = 01, the tokens, end
    of block (symbol 256).  length_rule: another length -> (symbol, extra bits, extra value) rule, for the
    mutants of the tests."""
    lens = _LEN if length_rule is None else {n: length_rule(n) for n in range(3, MAX_MATCH + 1)}
    dist = {}
    w = _Bits()
    w.put(1, 1)
    w.put(1, 2)
    for tok in tokens:
        if tok[0] == "L":
            w.put(*_LIT[tok[1]])
            continue
        sym, eb, ev = lens[tok[1]]
        w.put(*_LIT[sym])
        if eb:
            w.put(ev, eb)
        if tok[2] not in dist:
            dist[tok[2]] = distance_code(tok[2])
        code, deb, dev = dist[tok[2]]
        w.put(_rev(code, 5), 5)
        if deb:
            w.put(dev, deb)
    w.put(*_LIT[256])
    return w.done(), w.total


def _chunk(typ, data):
    return struct.pack(">I", len(data)) + typ + data + struct.pack(">I", zlib.crc32(typ + data) & 0xFFFFFFFF)


def encode(image, parse=parse_row, length_rule=None):
    """The file of one [H, W, 3] uint8 image -> (file bytes, tokens, zlib stream length, bits of the block)."""
    image = np.asarray(image, np.uint8)
    h, w, _ = image.shape
    tokens = parse_image(image, parse)
    block, nbits = deflate(tokens, length_rule)
    z = b"\x78\x01" + block + struct.pack(">I", zlib.adler32(scanlines(image).tobytes()) & 0xFFFFFFFF)
    png = b"\x89PNG\r\n\x1a\n" + _chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, 8, 2, 0, 0, 0))
    for k in range(0, len(z), CHUNK):
        png += _chunk(b"IDAT", z[k:k + CHUNK])
    return png + _chunk(b"IEND", b""), tokens, len(z), nbits


# ---------------------------------------------------------------------------------------------------- reading back
_PEEK = {}
for _s in range(288):
    _c, _nb = _LIT[_s]
    for _hi in range(1 << (9 - _nb)):
        _PEEK[_c | (_hi << _nb)] = (_s, _nb)
_LEN_OF_SYM = {257 + k: (LEN_BASE[k], LEN_EXTRA[k]) for k in range(29)}


def tokens_of(data, raw=False):
    """The tokens of a zlib stream (raw: of a bare deflate stream) that holds one final fixed-Huffman block.
    Raises ValueError for anything else."""
    if not raw:
        if data[:2] != b"\x78\x01":
            raise ValueError(f"zlib header {data[:2].hex()}")
        data = data[2:]
    acc, n, pos = 0, 0, 0

    def take(nb):
        nonlocal acc, n, pos
        if n < nb:
            more = data[pos:pos + 8]
            if len(more) * 8 + n < nb:
                raise ValueError("stream ends inside a token")
            acc |= int.from_bytes(more, "little") << n
            n += 8 * len(more)
            pos += len(more)
        v = acc & ((1 << nb) - 1)
        acc >>= nb
        n -= nb
        return v

    if take(3) != 0b011:
        raise ValueError("not one final fixed-Huffman block")
    out = []
    while True:
        if n < 9:  # (the end-of-block code is 7 bits and at most 4 Adler bytes follow: pad with what is there)
            more = data[pos:pos + 8]
            acc |= int.from_bytes(more, "little") << n
            n += 8 * len(more)
            pos += len(more)
        if (acc & 511) not in _PEEK:
            raise ValueError("bad literal / length code")
        sym, nb = _PEEK[acc & 511]
        if n < nb:
            raise ValueError("stream ends inside a token")
        acc >>= nb
        n -= nb
        if sym < 256:
            out.append(("L", sym))
        elif sym == 256:
            return out
        elif sym > 285:
            raise ValueError(f"length symbol {sym}")
        else:
            base, eb = _LEN_OF_SYM[sym]
            length = base + (take(eb) if eb else 0)
            code = _rev(take(5), 5)
            if code > 29:
                raise ValueError(f"distance code {code}")
            out.append(("M", length, DIST_BASE[code] + (take(DIST_EXTRA[code]) if DIST_EXTRA[code] else 0)))


def chunks(png):
    """[(type, data)] of a PNG file; checks the signature, every chunk's CRC-32 and that nothing follows."""
    assert png[:8] == b"\x89PNG\r\n\x1a\n"
    k, out = 8, []
    while k < len(png):
        n = struct.unpack(">I", png[k:k + 4])[0]
        typ, data = png[k + 4:k + 8], png[k + 8:k + 8 + n]
        crc = struct.unpack(">I", png[k + 8 + n:k + 12 + n])[0]
        assert zlib.crc32(typ + data) & 0xFFFFFFFF == crc, typ
        out.append((typ, data))
        k += 12 + n
    assert k == len(png)
    return out


def idat(png):
    return b"".join(d for t, d in chunks(png) if t == b"IDAT")


def round_trip(png, im):
    """What any decoder sees: the chunk layout walked by hand, zlib inflating the IDAT stream (it verifies the
    Adler-32) to the filter-0 scanlines, and PIL decoding the file (it verifies each CRC-32) to the pixels."""
    from PIL import Image

    ch = chunks(png)
    assert ch[0][0] == b"IHDR" and ch[-1][0] == b"IEND"
    w, h = struct.unpack(">II", ch[0][1][:8])
    assert (h, w) == im.shape[:2] and ch[0][1][8:] == b"\x08\x02\x00\x00\x00"
    raw = zlib.decompress(b"".join(d for t, d in ch if t == b"IDAT"))
    lines = np.frombuffer(raw, np.uint8).reshape(h, 3 * w + 1)
    assert (lines[:, 0] == 0).all()
    np.testing.assert_array_equal(lines[:, 1:].reshape(im.shape), im)
    np.testing.assert_array_equal(np.asarray(Image.open(io.BytesIO(png)).convert("RGB")), im)
    return len(png)


def first_difference(want_tokens, got_tokens, width):
    """(row, scanline position, expected token, got token) of the first token two parses of one image differ in,
    or None."""
    n1, pos = 3 * width + 1, 0
    for k in range(max(len(want_tokens), len(got_tokens))):
        a = want_tokens[k] if k < len(want_tokens) else None
        b = got_tokens[k] if k < len(got_tokens) else None
        if a != b:
            return pos // n1, pos % n1, a, b
        pos += 1 if a[0] == "L" else a[1]
    return None


def explain(want_png, got_png, width):
    """Why two files differ, for an assertion message: the first differing token where the streams can be read,
    otherwise the first differing byte."""
    if want_png == got_png:
        return "equal"
    k = next((i for i, (a, b) in enumerate(zip(want_png, got_png)) if a != b), min(len(want_png), len(got_png)))
    where = f"{len(want_png)} / {len(got_png)} bytes, first differing byte {k}"
    try:
        d = first_difference(tokens_of(idat(want_png)), tokens_of(idat(got_png)), width)
    except (ValueError, AssertionError, struct.error) as e:
        return f"{where}; the stream cannot be read ({e})"
    if d is None:
        return f"{where}; the tokens are equal (the coding of a token, the framing, the padding or a checksum differs)"
    return f"{where}; first differing token in row {d[0]} at scanline position {d[1]}: expected {d[2]}, got {d[3]}"


def row_offsets(image, tokens):
    """Bit offset of every row's first token in the block, and the block's end-of-block code, [H + 1]."""
    n1 = 3 * image.shape[1] + 1
    offs, pos, bit = [3], 0, 3
    for tok in tokens:
        bit += token_bits(tok)
        pos += 1 if tok[0] == "L" else tok[1]
        if pos % n1 == 0:
            offs.append(bit)
    assert len(offs) == image.shape[0] + 1
    return offs


# ---------------------------------------------------------------------------------------------------- the cases
def _noise(rng, *shape):
    return rng.integers(0, 256, shape, dtype=np.uint8)


def _other(rng, b):
    """A byte that differs from every byte of `b`."""
    taken = set(np.atleast_1d(b).tolist())
    return int(rng.choice([v for v in range(256) if v not in taken]))


def _image_of(lines):
    """Scanlines [H, 3 W + 1] (filter bytes are dropped) -> image [H, W, 3]."""
    lines = np.asarray(lines, np.uint8)
    return np.ascontiguousarray(lines[:, 1:]).reshape(len(lines), -1, 3)


def ladder_far():
    """Every length 3..258 at the row-above distance: W = 120 (scanlines of 361 bytes), 256 pairs of rows.  The
    first of a pair is noise, the second its copy with every byte outside the planted run inverted, so it matches
    the row above in the run and nowhere else.  512 rows: a lane parses two."""
    rng = np.random.default_rng(101)
    n1 = 361
    lines = _noise(rng, 512, n1)
    plan = []
    for k in range(256):
        length = 3 + k
        p = int(rng.integers(2, n1 - length + 1))  # scanline positions [p, p + length), apart from the filter byte
        lines[2 * k + 1] = lines[2 * k] ^ 0xFF
        lines[2 * k + 1, p:p + length] = lines[2 * k, p:p + length]
        plan.append((2 * k + 1, p, length))
    return _image_of(lines), plan


def ladder_near():
    """Every length 3..258 at distance 3: row k of 256 noise rows (W = 120) holds a run of period 3 whose match is
    exactly 3 + k long, broken on both sides; the rows above are unrelated noise."""
    rng = np.random.default_rng(102)
    n1 = 361
    lines = _noise(rng, 256, n1)
    plan = []
    for k in range(256):
        length = 3 + k
        p = int(rng.integers(5, n1 - length))  # the match covers [p, p + length); p + length < n1
        row = lines[k]
        row[p - 1] = _other(rng, row[p - 4])  # no match that starts before p
        for i in range(p, p + length):
            row[i] = row[i - 3]
        row[p + length] = _other(rng, row[p + length - 3])
        plan.append((k, p, length))
    return _image_of(lines), plan


def _two_rows(rng, n1):
    """Two noise scanlines of n1 bytes that match nowhere: not each other, and no byte its neighbour 3 back."""
    lines = np.zeros((2, n1), np.uint8)
    for r in range(2):
        for i in range(1, n1):
            lines[r, i] = _other(rng, [lines[r, i - 3] if i >= 3 else 0, lines[0, i] if r else 0])
    return lines


def _plant(rng, lines, p, near, far):
    """In row 1 of two unmatched scanlines: from position p a match of exactly `near` bytes at distance 3 and of
    exactly `far` bytes with the row above (0: none)."""
    n = max(near, far)
    for i in range(p, p + near):
        lines[1, i] = lines[1, i - 3]
    for i in range(p + near, p + n + 1):  # behind the near match: not periodic, and unlike the row above
        lines[1, i] = _other(rng, [lines[1, i - 3], lines[0, i]])
    lines[0, p:p + far] = lines[1, p:p + far]
    lines[0, p + far] = _other(rng, lines[1, p + far])


def choice_cases():
    """Images of 2 rows x 20 pixels (scanlines of 61 bytes) for the choice between the two candidates; one batch.
    -> (images [n, 2, 20, 3], names)."""
    rng = np.random.default_rng(103)
    n1 = 61
    out, names = [], []

    def add(name, lines):
        names.append(name)
        out.append(_image_of(lines))

    for name, near, far in (("tie_3", 3, 3), ("tie_9", 9, 9), ("tie_40", 40, 40), ("near_longer_by_1", 8, 7),
                            ("far_longer_by_1", 7, 8), ("near_3_far_4", 3, 4), ("near_4_far_3", 4, 3),
                            ("near_2_far_3", 2, 3), ("near_3_far_2", 3, 2), ("near_2_far_11", 2, 11),
                            ("near_11_far_2", 11, 2), ("near_2_far_2", 2, 2)):
        lines = _two_rows(rng, n1)
        _plant(rng, lines, 17, near, far)
        add(name, lines)
    # the near match at t = 3 compares its first byte with the filter byte: row[2] == 0 makes it a match from 3
    # on (rows 0 and 1, row 1 also with a shorter row-above match), row[2] != 0 delays it to t = 4
    for name, third, m in (("t3_zero", 0, 12), ("t3_zero_short", 0, 2), ("t3_nonzero", 77, 12)):
        lines = _two_rows(rng, n1)
        for r in range(2):
            lines[r, 3] = third
            for i in range(4, 3 + m):
                lines[r, i] = lines[r, i - 3]
            lines[r, 3 + m] = _other(rng, [lines[r, m], lines[0, 3 + m] if r else 0])
        add(name, lines)
    lines = _two_rows(rng, n1)  # ... and with a row-above match of the same length from t = 3: distance 3 wins
    lines[1, 3] = 0
    for i in range(4, 12):
        lines[1, i] = lines[1, i - 3]
    lines[0, 3:12] = lines[1, 3:12]
    lines[1, 12] = _other(rng, [lines[1, 9], lines[0, 12]])
    add("t3_zero_tie", lines)
    lines = _two_rows(rng, n1)  # a whole row equal to the one above: one match from t = 0, the filter byte in it
    lines[1] = lines[0]
    add("whole_row", lines)
    # row 0 has no row above: here it equals the last row of the image before it in the batch, which is where a
    # "row -1" would lie if the batch were one tall image
    lines = _two_rows(rng, n1)
    lines[0, 1:] = out[-1][1].reshape(-1)
    add("row0_equals_previous_image", lines)
    return np.stack(out), names


def tail_cases():
    """Row ends.  -> {name: image}: 2 x 20 images whose second row matches the first (or itself, 3 back) up to the
    row end, 1 byte and 2 bytes before it; tails whose last 1 or 2 bytes match although no match of 3 fits; and
    rows of maximal matches with 1, 2 and 3 bytes left over (W = 86, 87, 88)."""
    rng = np.random.default_rng(104)
    n1 = 61
    out = {}
    for short in (0, 1, 2):
        lines = _two_rows(rng, n1)
        lines[1, 30:n1 - short] = lines[0, 30:n1 - short]
        out[f"far_ends_{short}_before"] = _image_of(lines)
        lines = _two_rows(rng, n1)
        for i in range(30, n1 - short):
            lines[1, i] = lines[1, i - 3]
        for i in range(n1 - short, n1):
            lines[1, i] = _other(rng, [lines[1, i - 3], lines[0, i]])
        out[f"near_ends_{short}_before"] = _image_of(lines)
    for k in (1, 2):  # the last k bytes match (both candidates), the byte before does not: lim < 3, literals
        lines = _two_rows(rng, n1)
        lines[1, n1 - k:] = lines[0, n1 - k:] = lines[1, n1 - k - 3:n1 - 3]
        out[f"last_{k}_match"] = _image_of(lines)
    for w, broken in ((86, 0), (87, 1), (88, 3)):  # 259 = 258 + 1; 262 - 2 = 258 + 2; 265 - 4 = 258 + 3
        lines = _two_rows(rng, 3 * w + 1)
        lines[1] = lines[0]
        for i in range(1, 1 + broken):
            lines[1, i] = _other(rng, [lines[0, i], lines[1, i - 3] if i >= 3 else 0])
        out[f"left_over_w{w}"] = _image_of(lines)
    return out


def distance_widths():
    """{distance code: (smallest W, largest W)} with 3 W + 1 in the code's range, W <= MAX_WIDTH.  Code 4
    (distances 5 and 6) holds no 3 W + 1 and is absent."""
    out = {}
    for code in range(3, 30):
        lo, hi = DIST_BASE[code], DIST_BASE[code] + (1 << DIST_EXTRA[code]) - 1
        ws = [w for w in range(1, MAX_WIDTH + 1) if lo <= 3 * w + 1 <= hi]
        if ws:
            out[code] = (ws[0], ws[-1])
    return out


def distance_cases():
    """{W: image [3, W, 3]} for every W of distance_widths(): row 1 repeats row 0 except for its first third and
    a byte near the end, row 2 repeats row 1 except for one byte in the middle (W <= 2: whole copies)."""
    rng = np.random.default_rng(105)
    out = {}
    for w in sorted({w for pair in distance_widths().values() for w in pair}):
        n1 = 3 * w + 1
        lines = np.zeros((3, n1), np.uint8)
        lines[0, 1:] = _noise(rng, n1 - 1)
        lines[1] = lines[0]
        lines[2] = lines[0]
        if w > 2:
            lines[1, 1:n1 // 3] = _noise(rng, n1 // 3 - 1)
            lines[1, n1 - 2] ^= 0x55
            lines[2] = lines[1]
            lines[2, n1 // 2] ^= 0xAA
        out[w] = _image_of(lines)
    return out


HEIGHTS = (1, 2, 127, 128, 129, 255, 256, 257, 513, 1023, 1024)


def height_cases():
    """{H: images [2, H, 5, 3]}: noise rows, about half of them repeating the row above in whole or from some
    byte on, the last row from its fourth byte on."""
    out = {}
    for h in HEIGHTS:
        rng = np.random.default_rng(1060000 + h)
        lines = np.zeros((2, h, 16), np.uint8)
        lines[:, :, 1:] = _noise(rng, 2, h, 15)
        for i in range(2):
            for r in range(1, h):
                u = rng.random()
                if u < 0.3:
                    lines[i, r] = lines[i, r - 1]
                elif u < 0.5:
                    p = int(rng.integers(1, 13))
                    lines[i, r, p:] = lines[i, r - 1, p:]
            if h > 1:  # the last row: three bytes unlike the row above, then its copy
                lines[i, -1] = lines[i, -2]
                lines[i, -1, 1:4] ^= 0xFF
        out[h] = np.stack([_image_of(lines[0]), _image_of(lines[1])])
    return out


def short_row_cases():
    """{W: images [2, 1024, W, 3]} for W = 1 and 2: image 0 repeats one pixel row 1024 times (a row is one match
    of 12 or 13 bits, so several rows share an output dword), image 1 has distinct noise rows."""
    rng = np.random.default_rng(107)
    out = {}
    for w in (1, 2):
        same = np.broadcast_to(np.array([200, 10, 20] * w, np.uint8).reshape(1, w, 3), (MAX_HEIGHT, w, 3))
        out[w] = np.stack([same, _noise(rng, MAX_HEIGHT, w, 3)])
    return out


# (name, zlib stream length or None, (modulus, residue) of the block's bit count)
STREAM_TARGETS = (("z1024_b1", 1024, (8, 1)), ("z1025_b2", 1025, (8, 2)), ("z1026_b3", 1026, (8, 3)),
                  ("z1027_b4", 1027, (8, 4)), ("z1028_b5", 1028, (8, 5)), ("z1029_b6", 1029, (8, 6)),
                  ("z1023_b7", 1023, (8, 7)), ("z512_b0", 512, (8, 0)), ("z302_b31of32", 302, (32, 31)),
                  ("z702_b0of32", 702, (32, 0)), ("z513_b0", 513, (8, 0)), ("z516_b3", 516, (8, 3)))


def stream_cases():
    """{name: image [1, W, 3]} of STREAM_TARGETS.  One row of literals: the block has 3 + 8 + 24 W + h + 7 bits
    when h of the 3 W bytes are >= 144 (9-bit codes).  W and h follow from the target; a seeded search places the
    bytes and asks the reference whether the stream has the wanted length and bit count (an accidental match
    would change them), until it does."""
    out = {}
    for name, zlen, (mod, res) in STREAM_TARGETS:
        nd = zlen - 6  # deflate bytes: the bit count lies in (8 nd - 8, 8 nd]
        nbits = next(b for b in range(8 * nd, 8 * nd - 8, -1) if b % mod == res)
        w = next(w for w in range(1, MAX_WIDTH) if 18 + 26 * w >= nbits)
        h = nbits - 18 - 24 * w
        assert 0 <= h <= 3 * w
        for seed in range(100):
            rng = np.random.default_rng(1080000 + 1000 * zlen + seed)
            row = np.concatenate([rng.integers(144, 256, h), rng.integers(0, 144, 3 * w - h)]).astype(np.uint8)
            image = rng.permutation(row).reshape(1, w, 3)
            _, _, z, b = encode(image)
            if z == zlen and b == nbits:
                out[name] = image
                break
        else:
            raise AssertionError(name)
    return out


def adler_cases():
    """All-0 and all-255 images of 1024 rows x 64 pixels, [2, 1024, 64, 3]."""
    return np.stack([np.zeros((1024, 64, 3), np.uint8), np.full((1024, 64, 3), 255, np.uint8)])


def alignment_cases():
    """[4, 2, 3, 5, 3]: four pairs of 3 x 5 images (45 bytes each).  Packed, images [:, 0] lie 45 bytes apart, on
    all four residues mod 4; as one camera of the pair they lie 90 bytes apart, from offset 0 or 45.  Rows repeat
    in part."""
    rng = np.random.default_rng(109)
    im = _noise(rng, 4, 2, 3, 5, 3)
    flat = im.reshape(4, 2, 3, 15)
    flat[:, :, 1, 4:] = flat[:, :, 0, 4:]
    flat[:, :, 2, :11] = flat[:, :, 1, :11]
    return im


@functools.lru_cache(maxsize=None)
def case_groups():
    """{group: [(name, images [n, H, W, 3])]}: every batch the GPU tests launch, built once per process."""
    ch, ch_names = choice_cases()
    al = alignment_cases()
    return {
        "ladder_far": [("ladder_far", ladder_far()[0][None])],
        "ladder_near": [("ladder_near", ladder_near()[0][None])],
        "choice": [("choice", ch)],
        "tails": [(k, v[None]) for k, v in tail_cases().items()],
        "distances": [(f"w{w}", v[None]) for w, v in distance_cases().items()],
        "heights": [(f"h{h}", v) for h, v in height_cases().items()],
        "short_rows": [(f"w{w}", v) for w, v in short_row_cases().items()],
        "stream": [(k, v[None]) for k, v in stream_cases().items()],
        "adler": [("adler", adler_cases())],
        "alignment": [("alignment", np.ascontiguousarray(al[:, 0])), ("alignment_cam1", np.ascontiguousarray(al[:, 1]))],
    }


@functools.lru_cache(maxsize=None)
def reference(group):
    """[(name, images, [encode(image) for each image])] of a group, computed once per process."""
    return [(name, ims, [encode(im) for im in ims]) for name, ims in case_groups()[group]]
