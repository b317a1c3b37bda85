"""The batched PNG encoder (mujoco_manip_amd/csrc/mmx_png.hip) byte for byte against tests/png_ref.py.

tests/test_png.py shows that every file decodes to its pixels.  This module pins which file it is: the encoder is
deterministic, png_ref restates it token by token from the format documents, and the GPU tests demand equal bytes
at the symbol, row, size and alignment edges listed in the case builders of png_ref.  Three parts:

* reference validity (CPU): the reference's own files decode (zlib, PIL, its own inflater) for every case image;
* census (CPU): each case set reaches the edge it is named after, asserted on the reference's tokens and lengths,
  so an edit to a builder cannot empty a GPU test without a CPU test failing;
* the GPU comparisons, one small launch (or a few) per case, and mmx_image_stats at the size limit it states.

test_what_byte_equality_adds is the argument for the module: see its docstring."""
import zlib

import numpy as np
import pytest

import png_ref as R

GROUPS = ("ladder_far", "ladder_near", "choice", "tails", "distances", "heights", "short_rows", "stream", "adler",
          "alignment")


def rows_of(tokens, width):
    """Tokens of an image -> per row [(scanline position, token)]."""
    n1, pos, out = 3 * width + 1, 0, []
    for tok in tokens:
        if pos % n1 == 0:
            out.append([])
        out[-1].append((pos % n1, tok))
        pos += 1 if tok[0] == "L" else tok[1]
    return out


def candidates(line, above, t):
    """(length at distance 3, length at the row-above distance) at scanline position t, by the definition."""
    lim = min(R.MAX_MATCH, len(line) - t)
    m1 = m2 = 0
    while t >= 3 and m1 < lim and line[t + m1] == line[t + m1 - 3]:
        m1 += 1
    while above is not None and m2 < lim and line[t + m2] == above[t + m2]:
        m2 += 1
    return m1, m2


def decisions(image, tokens):
    """[(row, t, m1, m2, token)] at every position the greedy parse of `image` stopped at."""
    lines = R.scanlines(image)
    return [(r, t, *candidates(lines[r].tolist(), lines[r - 1].tolist() if r else None, t), tok)
            for r, row in enumerate(rows_of(tokens, image.shape[1])) for t, tok in row]


def matches(tokens, distance=None):
    return [t for t in tokens if t[0] == "M" and (distance is None or t[2] == distance)]


def one(group):
    """(images, references) of a group that is a single batch."""
    (_, ims, refs), = R.reference(group)
    return ims, refs


# ------------------------------------------------------------------------------------------- reference validity
def test_length_and_distance_tables_are_complete():
    """The typed-in RFC 1951 tables: 29 length rows covering 3..258 and 30 distance rows covering 1..32768 without
    gap or overlap (258 is also the last value of row 284: it has its own row, 285)."""
    assert len(R.LEN_BASE) == len(R.LEN_EXTRA) == 29 and len(R.DIST_BASE) == len(R.DIST_EXTRA) == 30
    for k in range(27):
        assert R.LEN_BASE[k] + (1 << R.LEN_EXTRA[k]) == R.LEN_BASE[k + 1]
    assert R.LEN_BASE[27] + (1 << R.LEN_EXTRA[27]) - 1 == 258 == R.LEN_BASE[28] and R.LEN_BASE[0] == 3
    for k in range(29):
        assert R.DIST_BASE[k] + (1 << R.DIST_EXTRA[k]) == R.DIST_BASE[k + 1]
    assert R.DIST_BASE[0] == 1 and R.DIST_BASE[29] + (1 << R.DIST_EXTRA[29]) - 1 == 32768
    assert R.length_symbol(258) == (285, 0, 0) and R.length_symbol(257) == (284, 5, 30)
    assert R.distance_code(32768) == (29, 13, 8191) and R.distance_code(4) == (3, 0, 0)


@pytest.mark.parametrize("group", GROUPS)
def test_reference_files_decode(group):
    """For every case image: zlib inflates the reference's IDAT stream to the filter-0 scanlines, PIL decodes the
    file to the pixels, the chunk walk passes, the reference's inflater returns the tokens that were written
    (from the bare block and from the file), and the byte-by-byte parse agrees with the numpy one (all images but
    the widest)."""
    for name, ims, refs in R.reference(group):
        for im, (png, tokens, zlen, nbits) in zip(ims, refs):
            z = R.idat(png)
            assert len(z) == zlen and zlen == 2 + (nbits + 7) // 8 + 4, name
            assert zlib.decompress(z) == R.scanlines(im).tobytes(), name
            R.round_trip(png, im)
            block, bits = R.deflate(tokens)
            assert bits == nbits == 3 + sum(map(R.token_bits, tokens)) + 7, name
            assert R.tokens_of(block, raw=True) == tokens, name
            assert R.tokens_of(z) == tokens, name
            if im.shape[1] <= 1024:
                assert R.parse_image(im, R.parse_row_plain) == tokens, name


def test_first_difference_names_row_and_position():
    im = R.tail_cases()["far_ends_1_before"]
    _, tokens, _, _ = R.encode(im)
    other = tokens[:-2] + [("M", 31, 61)]
    assert R.first_difference(tokens, other, 20) == (1, 30, ("M", 30, 61), ("M", 31, 61))
    assert R.first_difference(tokens, list(tokens), 20) is None


# ------------------------------------------------------------------------------------------------------- census
BOUNDARIES = ((10, 11), (18, 19), (34, 35), (66, 67), (130, 131), (226, 227), (257, 258))


@pytest.mark.parametrize("group,distance", [("ladder_far", 361), ("ladder_near", 3)])
def test_census_length_ladders(group, distance):
    """Each ladder holds every length 3..258 at its distance, one planted match per row at the planned position
    and nothing but literals around it; the pairs of lengths on both sides of every change of extra-bit count
    are there with different symbols.  The row-above ladder has 512 rows (two per lane of a 256-lane workgroup)
    and the noise row before each planted row has no match at all."""
    ims, refs = one(group)
    image, plan = R.ladder_far() if group == "ladder_far" else R.ladder_near()
    assert np.array_equal(ims[0], image) and image.shape == ((512 if group == "ladder_far" else 256), 120, 3)
    rows = rows_of(refs[0][1], 120)
    assert len(rows) == image.shape[0]
    planted = {r for r, _, _ in plan}
    for r, p, length in plan:
        ms = [(t, tok) for t, tok in rows[r] if tok[0] == "M"]
        assert ms == [(p, ("M", length, distance))], (r, ms)
    for r in set(range(len(rows))) - planted:
        assert not matches(tok for _, tok in rows[r])
    assert sorted(length for _, _, length in plan) == list(range(3, 259))
    seen = {tok[1] for tok in matches(refs[0][1], distance)}
    for a, b in BOUNDARIES:
        assert {a, b} <= seen and R.length_symbol(a)[0] + 1 == R.length_symbol(b)[0]
    assert {R.length_symbol(n)[0] for n in seen} == set(range(257, 286))
    assert R.distance_code(distance)[0] == (16 if distance == 361 else 2)


def test_census_candidate_choice():
    """The choice cases reach: equal candidates (distance 3 taken), either longer by one, one of length 2 beside
    one of at least 3 (both ways) and both of length 2 (a literal); the near match at t = 3 against the filter
    byte with row[2] == 0 (taken at 3; also tied with the row above; also too short) and with row[2] != 0
    (a literal at 3, the match from 4); a whole row as one match from t = 0; no row 0 with a row-above match
    although its bytes equal the last row of the image before it."""
    ims, refs = one("choice")
    _, names = R.choice_cases()
    assert ims.shape == (len(names), 2, 20, 3)
    dec = {name: decisions(im, ref[1]) for name, im, ref in zip(names, ims, refs)}
    every = [d for ds in dec.values() for d in ds]
    for r, t, m1, m2, tok in every:  # the reference follows the rule at every position it visits
        if max(m1, m2) >= 3:
            assert tok == (("M", m1, 3) if m1 >= m2 else ("M", m2, 61)), (r, t, m1, m2, tok)
        else:
            assert tok[0] == "L", (r, t, m1, m2, tok)

    def reached(cond):
        return [d for d in every if cond(*d)]

    assert len(reached(lambda r, t, m1, m2, tok: m1 == m2 >= 3 and tok == ("M", m1, 3))) >= 4
    assert {m1 for r, t, m1, m2, tok in reached(lambda r, t, m1, m2, tok: m1 == m2 >= 3)} >= {3, 9, 40}
    assert reached(lambda r, t, m1, m2, tok: m1 == m2 + 1 and m2 >= 3 and tok == ("M", m1, 3))
    assert reached(lambda r, t, m1, m2, tok: m2 == m1 + 1 and m1 >= 3 and tok == ("M", m2, 61))
    assert reached(lambda r, t, m1, m2, tok: (m1, m2) == (3, 4) and tok == ("M", 4, 61))
    assert reached(lambda r, t, m1, m2, tok: (m1, m2) == (4, 3) and tok == ("M", 4, 3))
    assert reached(lambda r, t, m1, m2, tok: m1 == 2 and m2 == 3 and tok == ("M", 3, 61))
    assert reached(lambda r, t, m1, m2, tok: m1 == 3 and m2 == 2 and tok == ("M", 3, 3))
    assert reached(lambda r, t, m1, m2, tok: m1 == 2 and m2 == 11 and tok == ("M", 11, 61))
    assert reached(lambda r, t, m1, m2, tok: m1 == 11 and m2 == 2 and tok == ("M", 11, 3))
    assert reached(lambda r, t, m1, m2, tok: m1 == 2 and m2 == 2 and tok[0] == "L")
    lines = {name: R.scanlines(im) for name, im in zip(names, ims)}
    for r in (0, 1):  # t = 3, row[2] == 0: in row 0 and below an unrelated row
        assert lines["t3_zero"][r, 3] == 0 and (r, 3, 12, 1 if r else 0, ("M", 12, 3)) in dec["t3_zero"]
        assert lines["t3_nonzero"][r, 3] != 0
        assert (r, 3, 0, 1 if r else 0, ("L", 77)) in dec["t3_nonzero"] and (r, 4, 11, 0, ("M", 11, 3)) in dec["t3_nonzero"]
        assert (r, 3, 2, 1 if r else 0, ("L", 0)) in dec["t3_zero_short"]
    assert (1, 3, 9, 9, ("M", 9, 3)) in dec["t3_zero_tie"]
    assert dec["whole_row"][-1] == (1, 0, 0, 61, ("M", 61, 61))
    k = names.index("row0_equals_previous_image")
    assert np.array_equal(ims[k][0], ims[k - 1][1])
    assert all(tok[0] == "L" or tok[2] == 3 for name in names for r, t, m1, m2, tok in dec[name] if r == 0)


def test_census_row_tails():
    """Matches at both distances that end at the row end, 1 byte and 2 bytes before it (the rest: literals parsed
    with a limit below 3); last bytes that match although no match fits; maximal matches with 1, 2 and 3 bytes
    left over."""
    cases = R.tail_cases()
    ref = {name: (im, r[0]) for name, im, r in ((n, ims[0], refs) for n, ims, refs in R.reference("tails"))}
    assert set(ref) == set(cases)
    last_row = {name: [tok for _, tok in rows_of(r[1], im.shape[1])[1]] for name, (im, r) in ref.items()}
    for short in (0, 1, 2):
        for kind, d in (("far", 61), ("near", 3)):
            row = last_row[f"{kind}_ends_{short}_before"]
            assert row[30] == ("M", 31 - short, d) and len(row) == 31 + short
            assert all(tok[0] == "L" for tok in row[:30] + row[31:])
    for k in (1, 2):
        im, r = ref[f"last_{k}_match"]
        dec = [d for d in decisions(im, r[1]) if d[0] == 1]
        assert [(t, m1, m2, tok[0]) for _, t, m1, m2, tok in dec[-k:]] == [(61 - k + j, k - j, k - j, "L") for j in range(k)]
        assert all(tok[0] == "L" for tok in last_row[f"last_{k}_match"])
    assert ref["left_over_w86"][0].shape[1] == 86 and last_row["left_over_w86"][0] == ("M", 258, 259)
    assert [t[0] for t in last_row["left_over_w86"]] == ["M", "L"]
    assert [t[0] for t in last_row["left_over_w87"]] == ["L", "L", "M", "L", "L"] and last_row["left_over_w87"][2] == ("M", 258, 262)
    assert last_row["left_over_w88"][-2:] == [("M", 258, 265), ("M", 3, 265)]
    assert [t[0] for t in last_row["left_over_w88"]] == ["L"] * 4 + ["M", "M"]


def test_census_distance_codes():
    """Every distance code a row-above match can have (3 and 5..29; code 4 holds distances 5 and 6, no 3 W + 1),
    at the smallest and the largest width of the code; every image has a match with that code; the set holds
    first and last values of codes, the distance 4 of W = 1 and 32767 of the widest image."""
    widths = R.distance_widths()
    assert set(widths) == set(range(3, 30)) - {4}
    imgs = {im.shape[2]: ref for _, im, ref in R.reference("distances")}
    firsts, lasts = set(), set()
    for code, (lo, hi) in widths.items():
        first, last = R.DIST_BASE[code], R.DIST_BASE[code] + (1 << R.DIST_EXTRA[code]) - 1
        assert first <= 3 * lo + 1 <= 3 * hi + 1 <= last
        assert 3 * (lo - 1) + 1 < first and (3 * (hi + 1) + 1 > last or hi == R.MAX_WIDTH)
        for w in (lo, hi):
            tokens = imgs[w][0][1]
            assert matches(tokens, 3 * w + 1) and R.distance_code(3 * w + 1)[0] == code
            assert imgs[w][0][0][16:24] == w.to_bytes(4, "big") + (3).to_bytes(4, "big")
        firsts |= {code} if 3 * lo + 1 == first else set()
        lasts |= {code} if 3 * hi + 1 == last else set()
    assert widths[3] == (1, 1) and widths[29] == (8192, R.MAX_WIDTH) and 3 * R.MAX_WIDTH + 1 == 32767
    # a code's first value is 3 * 2^e + 1 (odd codes: always a 3 W + 1) or 2^(e+1) + 1 (even codes: never); its
    # last is 2^(e+2) (odd codes: a 3 W + 1 for even e) or 3 * 2^e (even codes: never)
    assert firsts == {3} | set(range(5, 30, 2)) and lasts == set(range(3, 30, 4)), (firsts, lasts)
    extra_values = {R.distance_code(3 * w + 1)[2] for pair in widths.values() for w in pair}
    assert 0 in extra_values and max(extra_values) >= 8190


def test_census_heights():
    """Heights 1, 2, both sides of the 128- and 256-row steps (the 128-lane kernel up to 128 rows; from 257 a lane
    parses several rows), 513, 1023 and the limit 1024, at W = 5; from 2 rows on every image mixes row-above
    matches with literals, and the limit + 1 is what the GPU test expects to be refused."""
    got = {ims.shape[1]: (ims, refs) for _, ims, refs in R.reference("heights")}
    assert tuple(got) == R.HEIGHTS == (1, 2, 127, 128, 129, 255, 256, 257, 513, 1023, 1024)
    assert R.MAX_HEIGHT == 1024
    for h, (ims, refs) in got.items():
        assert ims.shape == (2, h, 5, 3)
        for im, ref in zip(ims, refs):
            rows = rows_of(ref[1], 5)
            assert len(rows) == h
            if h >= 127:
                far_rows = {r for r, row in enumerate(rows) if matches((tok for _, tok in row), 16)}
                lit_rows = {r for r, row in enumerate(rows) if any(tok[0] == "L" for _, tok in row)}
                whole = {r for r, row in enumerate(rows) if row == [(0, ("M", 16, 16))]}
                assert len(far_rows) > h // 4 and len(lit_rows) > h // 4 and len(whole) > h // 8
            if h >= 2:  # the last row (beyond row 255 from 257 rows on): literals, then a row-above match
                assert [tok for _, tok in rows[-1]][-2:] == [("L", int(im[-1, 0, 2])), ("M", 12, 16)]
                assert all(tok[0] == "L" for _, tok in rows[-1][:-1])


def test_census_short_rows():
    """W = 1 and 2 at 1024 rows: rows of 12 or 13 bits (one match), so some output dword holds bits of three rows
    or more, and some row ends exactly on a dword boundary; the second image of each batch has distinct rows."""
    got = {ims.shape[2]: (ims, refs) for _, ims, refs in R.reference("short_rows")}
    assert set(got) == {1, 2}
    for w, (ims, refs) in got.items():
        assert ims.shape == (2, 1024, w, 3)
        rows = rows_of(refs[0][1], w)
        assert all(row == [(0, ("M", 3 * w + 1, 3 * w + 1))] for row in rows[1:])
        assert R.token_bits(rows[1][0][1]) == (12 if w == 1 else 13)
        assert len({bytes(r) for r in ims[1].reshape(1024, -1)}) > 1000
        for k, (im, ref) in enumerate(zip(ims, refs)):
            offs = np.array(R.row_offsets(im, ref[1]))
            assert offs[-1] + 7 == ref[3]
            assert (offs[1:] % 32 == 0).any(), (w, k)  # a row that ends where a dword ends
            dwords = np.arange(0, ref[3], 32)  # rows with bits in each dword
            per_dword = np.searchsorted(offs[:-1], dwords + 32, "left") - np.searchsorted(offs[1:], dwords, "right")
            assert per_dword.min() >= 1 and (per_dword.max() >= 3 or k == 1), (w, k)


def test_census_stream_lengths():
    """One-row images of literals whose zlib stream is 0, 1 .. 5 and 511 bytes mod 512 long (a full last chunk; the
    Adler-32 across a chunk header, byte by byte; one byte short of full), shorter than a chunk and exactly one
    chunk; bit counts on all eight residues mod 8, and 0 and 31 mod 32."""
    got = {name: refs[0] for name, _, refs in R.reference("stream")}
    assert set(got) == {name for name, _, _ in R.STREAM_TARGETS}
    for name, zlen, (mod, res) in R.STREAM_TARGETS:
        _, tokens, z, nbits = got[name]
        assert z == zlen and nbits % mod == res and all(t[0] == "L" for t in tokens), name
        assert len([1 for typ, _ in R.chunks(got[name][0]) if typ == b"IDAT"]) == -(-zlen // 512)
    zl = [r[2] for r in got.values()]
    assert {z % 512 for z in zl} >= {0, 1, 2, 3, 4, 5, 511}
    assert {z % 512 for z in zl if z > 512} >= {0, 1, 2, 3, 4, 5, 511}
    assert min(zl) < 512 and 512 in zl
    assert {r[3] % 8 for r in got.values()} == set(range(8))
    assert {0, 31} <= {r[3] % 32 for r in got.values()}


def test_census_adler_extremes():
    """All-0 and all-255 at 1024 x 64: the Adler-32 from its definition (two running sums) equals zlib's and the
    last four bytes of the reference's stream; for all-255 the second sum passes 2^42 before its reduction."""
    ims, refs = one("adler")
    assert ims.shape == (2, 1024, 64, 3) and not ims[0].any() and (ims[1] == 255).all()
    for im, ref in zip(ims, refs):
        data = R.scanlines(im).ravel().astype(object)
        n = len(data)
        s1 = 1 + int(data.sum())
        s2 = n + int((data * np.arange(n, 0, -1).astype(object)).sum())
        want = ((s2 % 65521) << 16) | (s1 % 65521)
        assert want == zlib.adler32(R.scanlines(im).tobytes()) == int.from_bytes(R.idat(ref[0])[-4:], "big")
        assert s2 > (1 << 42) or not im.any()
    assert int.from_bytes(R.idat(refs[0][0])[-4:], "big") == (((1024 * 193) % 65521) << 16) | 1


def test_census_alignment():
    """Four 3 x 5 images of 45 bytes: packed they start on all four residues mod 4, as one camera of a pair 90
    bytes apart from offset 0 or 45; every image has row-above matches."""
    al = R.alignment_cases()
    assert al.shape == (4, 2, 3, 5, 3) and al[0, 0].nbytes == 45
    assert {(45 * i) % 4 for i in range(4)} == {0, 1, 2, 3}
    assert {(90 * i + 45 * cam) % 4 for i in range(4) for cam in (0, 1)} == {0, 1, 2, 3}
    for _, ims, refs in R.reference("alignment"):
        assert ims.shape == (4, 3, 5, 3)
        assert all(len(matches(ref[1], 16)) >= 2 for ref in refs)


def test_census_image_stats_limit():
    """mmx_image_stats' fast path adds 4 squares per step into 32 bits per lane: at 4096 x 4096 a lane of 256
    takes 16384 steps and all-255 gives 4,261,478,400 < 2^32 with 0.8 % to spare: the sizes of the GPU test are
    that limit, the byte path next to it (an odd pixel count), and 4097, which is refused."""
    steps = 4096 * 4096 // 4 // 256
    assert steps == 16384 and steps * 4 * 255 * 255 == 4261478400 < 1 << 32
    assert (1 << 32) - 4261478400 < 0.008 * (1 << 32)
    assert (4095 * 4095) % 4 != 0 and (1024 * 1024) % 4 == 0


# ------------------------------------------------------------------------------------- what byte equality adds
def mutant(tie_far=False, near_from=3, keep_tail=0, min_match=3):
    """A parse_row with one rule changed."""
    def parse(line, above):
        line = bytes(line)
        above = None if above is None else bytes(above)
        n, t, out = len(line), 0, []
        while t < n:
            lim = min(R.MAX_MATCH, n - keep_tail - t)
            m1 = m2 = 0
            while t >= near_from and m1 < lim and line[t + m1] == line[t + m1 - 3]:
                m1 += 1
            while above is not None and m2 < lim and line[t + m2] == above[t + m2]:
                m2 += 1
            if max(m1, m2) >= min_match:
                out.append(("M", m1, 3) if (m1 > m2 if tie_far else m1 >= m2) else ("M", m2, n))
                t += max(m1, m2)
            else:
                out.append(("L", line[t]))
                t += 1
        return out
    return parse


def length_258_as_284(n):
    return (284, 5, 31) if n == 258 else R.length_symbol(n)


MUTANTS = {  # name: (encode arguments, does the round trip notice, do the bytes differ)
    "ties go to the far distance": (dict(parse=mutant(tie_far=True)), False, True),
    "no near match at t == 3": (dict(parse=mutant(near_from=4)), False, True),
    "length 258 as symbol 284, extra 31": (dict(length_rule=length_258_as_284), False, True),
    "literals only": (dict(parse=mutant(min_match=1 << 30)), False, True),
    "no match into the last 2 bytes of a row": (dict(parse=mutant(keep_tail=2)), False, True),
}


def test_what_byte_equality_adds():
    """Five encoders that are wrong by this project's definition, applied to the candidate-choice and row-tail
    images, and what notices them:

        mutation                                   zlib + PIL + chunk walk   bytes against the reference
        ties go to the far distance                passes                    differs
        no near match at t == 3                    passes                    differs
        length 258 as symbol 284, extra 31         passes                    differs
        literals only                              passes                    differs
        no match into the last 2 bytes of a row    passes                    differs

    Every one of them writes a valid PNG of the right pixels (zlib accepts 284 + 31 for 258), so the round trip of
    tests/test_png.py passes all five; only the size bounds of that file would catch the fourth, and only on its
    flat and rendered images.  Comparing bytes catches each.  The unchanged mutant equals the reference."""
    images = [im for g in ("choice", "tails") for _, ims, _ in R.reference(g) for im in ims]
    want = [ref[0] for g in ("choice", "tails") for _, _, refs in R.reference(g) for ref in refs]
    assert [R.encode(im, parse=mutant())[0] for im in images] == want
    for name, (kw, round_trip_notices, bytes_differ) in MUTANTS.items():
        files = [R.encode(im, **kw)[0] for im in images]
        noticed = False
        for png, im in zip(files, images):
            try:
                R.round_trip(png, im)
            except (AssertionError, zlib.error, OSError, SyntaxError, ValueError):
                noticed = True
        assert noticed == round_trip_notices, name
        assert (files != want) == bytes_differ and bytes_differ, name
        k = next(i for i, (a, b) in enumerate(zip(files, want)) if a != b)
        said = R.explain(want[k], files[k], images[k].shape[1])  # a changed parse is named by its first token
        assert ("first differing token in row" if "parse" in kw else "the tokens are equal") in said, (name, said)


# ---------------------------------------------------------------------------------------------------- on the GPU
@pytest.fixture(scope="module")
def sim():
    torch = pytest.importorskip("torch")
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    from mujoco_manip_amd import _lib

    s = _lib.Sim(1, action_mode="abs_pos", image_size=0)
    yield s
    s.close()


def assert_files(files, ims, refs, name):
    """Device files against the reference's, byte for byte, and through the round trip of test_png.py."""
    assert len(files) == len(ims)
    for i, (png, im, ref) in enumerate(zip(files, ims, refs)):
        assert png == ref[0], f"{name}[{i}] {im.shape}: {R.explain(ref[0], png, im.shape[1])}"
        R.round_trip(png, im)


@pytest.mark.gpu
@pytest.mark.parametrize("group", GROUPS)
def test_device_files_equal_reference(sim, group):
    """sim.png_encode of every batch of the group equals png_ref.encode of each image byte for byte."""
    import torch

    for name, ims, refs in R.reference(group):
        packed, offs = sim.png_encode(torch.as_tensor(ims).cuda())
        data = packed.cpu().numpy().tobytes()
        assert len(offs) == len(ims) + 1 and offs[-1] == len(data)
        assert_files([data[offs[i]:offs[i + 1]] for i in range(len(ims))], ims, refs, f"{group}/{name}")


@pytest.mark.gpu
def test_device_files_equal_reference_strided(sim):
    """The alignment images as the two cameras of a [n, 2, H, W, 3] batch through png_encode_device (image bases
    90 bytes apart, from offset 0 and 45): the same files."""
    import torch

    dev = torch.as_tensor(R.alignment_cases()).cuda()
    assert dev.data_ptr() % 4 == 0
    for cam, (name, ims, refs) in enumerate(R.reference("alignment")):
        view = dev[:, cam]
        assert view.stride(0) == 90 and not view.is_contiguous()
        packed, ends = sim.png_encode_device(view)
        ends = [0] + ends.cpu().numpy().tolist()
        data = packed.cpu().numpy().tobytes()
        assert_files([data[ends[i]:ends[i + 1]] for i in range(4)], ims, refs, name)


@pytest.mark.gpu
def test_height_limit_is_refused(sim):
    """1025 rows: mmx_png_bound returns -1 and both entry points raise ValueError; 1024 rows is a case above."""
    import torch

    assert sim.L.mmx_png_bound(5, R.MAX_HEIGHT) > 0
    assert sim.L.mmx_png_bound(5, R.MAX_HEIGHT + 1) == -1 and sim.L.mmx_png_scratch(5, R.MAX_HEIGHT + 1) == -1
    tall = torch.zeros((1, R.MAX_HEIGHT + 1, 5, 3), dtype=torch.uint8, device="cuda")
    with pytest.raises(ValueError, match="unsupported image size"):
        sim.png_encode(tall)
    with pytest.raises(ValueError, match="unsupported image size"):
        sim.png_encode_device(tall)


def _stats_by_histogram(im):
    """[4, 3] (min, max, sum, sum of squares) per channel of [H, W, 3] uint8 in Python integers."""
    out = np.zeros((4, 3), np.int64)
    v = np.arange(256, dtype=np.int64)
    for c in range(3):
        cnt = np.bincount(im[..., c].ravel(), minlength=256).astype(np.int64)
        out[:, c] = (v[cnt > 0].min(), v[cnt > 0].max(), int((v * cnt).sum()), int((v * v * cnt).sum()))
    return out


@pytest.mark.gpu
def test_image_stats_at_its_size_limit(sim):
    """mmx_image_stats at the largest image it accepts: all-255 at 4096 x 4096 (the 32-bit per-lane sums of squares
    reach 4,261,478,400) gives exactly (255, 255, 255 npx, 255^2 npx) per channel; random 1024 x 1024 (fast path)
    and 4095 x 4095 (an odd pixel count: the byte path) equal an int64 histogram count; 4097 either way is
    refused with MMX_EINVAL."""
    import ctypes as C

    import torch

    npx = 4096 * 4096
    got = sim.image_stats(torch.full((1, 4096, 4096, 3), 255, dtype=torch.uint8, device="cuda")).cpu().numpy()
    np.testing.assert_array_equal(got[0], np.array([[255] * 3, [255] * 3, [255 * npx] * 3, [255 * 255 * npx] * 3]))
    rng = np.random.default_rng(110)
    for s in (1024, 4095):
        im = rng.integers(0, 256, (s, s, 3), dtype=np.uint8)
        got = sim.image_stats(torch.as_tensor(im).cuda().unsqueeze(0)).cpu().numpy()  # (stride 3 s s, not numpy's 0)
        np.testing.assert_array_equal(got[0], _stats_by_histogram(im))
    out = torch.zeros((1, 4, 3), dtype=torch.int64, device="cuda")
    for h, w in ((4097, 1), (1, 4097)):
        t = torch.zeros((1, h, w, 3), dtype=torch.uint8, device="cuda")
        rc = sim.L.mmx_image_stats(sim.ptr, C.c_void_p(t.data_ptr()), t.stride(0), 1, w, h, C.c_void_p(out.data_ptr()))
        assert rc == -1  # MMX_EINVAL (include/mmx_api.h)
        with pytest.raises(RuntimeError, match="mmx_image_stats"):
            sim.image_stats(t)
    assert not out.any().item()
