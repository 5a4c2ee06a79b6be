"""The reference of mtgs_amd.jpeg (tests/test_jpeg_host.py, tests/test_gpu_jpeg.py): a baseline sequential JPEG encoder in plain
NumPy, stage by stage as include/mtgs_jpeg.h states the arithmetic -- libjpeg's integer path, which Pillow with libjpeg-turbo
writes byte for byte.  Written for reading, not for speed: whole-image arrays for the pixel stages, a Python loop over the
blocks for the entropy coder.

    encode(image, quality=75, subsampling="4:2:0")   the whole file, bytes
    header(h, w, quality, subsampling)               SOI .. SOS header, bytes
    scan(image, quality, subsampling)                the entropy-coded segment, stuffed and padded, without EOI
    segments(data)                                   [(marker, payload)] of a file's header, and the offset of the scan
    to_u8(x, conversion)                             float32 -> uint8 by the presented frame's two conversions
    images(kind, h, w, seed)                         the five kinds of test image, uint8 [h, w, 3]
"""
import numpy as np

ZIGZAG = np.array([0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21,
                   28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61,
                   54, 47, 55, 62, 63])
# ITU-T T.81 Annex K.1: the base tables, row by row
LUMA_Q = np.array([16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51, 87,
                   80, 62, 18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101, 72,
                   92, 95, 98, 112, 100, 103, 99])
CHROMA_Q = np.array([17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99,
                     99, 99, 99] + [99] * 32)
# Annex K.3: (BITS, HUFFVAL) of the four tables
DC_LUMA = ([0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0], list(range(12)))
DC_CHROMA = ([0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0], list(range(12)))
AC_LUMA = ([0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7d], [
    0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71, 0x14, 0x32, 0x81, 0x91,
    0xa1, 0x08, 0x23, 0x42, 0xb1, 0xc1, 0x15, 0x52, 0xd1, 0xf0, 0x24, 0x33, 0x62, 0x72, 0x82, 0x09, 0x0a, 0x16, 0x17, 0x18, 0x19, 0x1a,
    0x25, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x34, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53,
    0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79,
    0x7a, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5,
    0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9,
    0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe1, 0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf1, 0xf2,
    0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa])
AC_CHROMA = ([0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77], [
    0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71, 0x13, 0x22, 0x32, 0x81, 0x08, 0x14,
    0x42, 0x91, 0xa1, 0xb1, 0xc1, 0x09, 0x23, 0x33, 0x52, 0xf0, 0x15, 0x62, 0x72, 0xd1, 0x0a, 0x16, 0x24, 0x34, 0xe1, 0x25, 0xf1, 0x17,
    0x18, 0x19, 0x1a, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a,
    0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78,
    0x79, 0x7a, 0x82, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3,
    0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7,
    0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf2,
    0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa])
SUBSAMPLINGS = ("4:2:0", "4:4:4")
BLOCK_BITS = 22 + 63 * 26        # the longest block: see capacity()
HEADER_BYTES = 623


def quant_table(base, quality):
    """libjpeg's jpeg_quality_scaling and jpeg_add_quant_table (force_baseline), in natural order"""
    scale = 5000 // quality if quality < 50 else 200 - 2 * quality
    return np.clip((base * scale + 50) // 100, 1, 255)


def huffman_codes(table):
    """{symbol: (code, length)} of a (BITS, HUFFVAL) pair: Annex C's canonical assignment"""
    bits, vals = table
    codes, code, k = {}, 0, 0
    for length in range(1, 17):
        for _ in range(bits[length - 1]):
            codes[vals[k]] = (code, length)
            code, k = code + 1, k + 1
        code <<= 1
    return codes


# ---- the header -------------------------------------------------------------------------------------------------------------------
def _segment(marker, payload):
    return bytes([0xFF, marker]) + (len(payload) + 2).to_bytes(2, "big") + bytes(payload)


def header(h, w, quality, subsampling):
    """SOI, JFIF 1.01 APP0 (no units, density 1:1, no thumbnail), DQT 0 and DQT 1, SOF0, the four DHT, the SOS header"""
    out = b"\xff\xd8" + _segment(0xE0, b"JFIF\x00" + bytes([1, 1, 0, 0, 1, 0, 1, 0, 0]))
    for index, base in enumerate((LUMA_Q, CHROMA_Q)):
        out += _segment(0xDB, bytes([index]) + bytes(int(v) for v in quant_table(base, quality)[ZIGZAG]))
    luma_sampling = 0x22 if subsampling == "4:2:0" else 0x11
    out += _segment(0xC0, bytes([8]) + h.to_bytes(2, "big") + w.to_bytes(2, "big") + bytes([3, 1, luma_sampling, 0, 2, 0x11, 1, 3, 0x11, 1]))
    for tc_th, (bits, vals) in ((0x00, DC_LUMA), (0x10, AC_LUMA), (0x01, DC_CHROMA), (0x11, AC_CHROMA)):
        out += _segment(0xC4, bytes([tc_th]) + bytes(bits) + bytes(vals))
    return out + _segment(0xDA, bytes([3, 1, 0x00, 2, 0x11, 3, 0x11, 0, 63, 0]))


def segments(data):
    """([(marker, payload)] up to and including SOS, offset of the first scan byte) of a JPEG file"""
    assert data[:2] == b"\xff\xd8"
    at, out = 2, []
    while True:
        assert data[at] == 0xFF
        marker, length = data[at + 1], int.from_bytes(data[at + 2:at + 4], "big")
        out.append((marker, bytes(data[at + 4:at + 2 + length])))
        at += 2 + length
        if marker == 0xDA:
            return out, at


# ---- pixels to quantised blocks ---------------------------------------------------------------------------------------------------
def _fix(x):
    return int(x * 65536 + 0.5)


def ycbcr(rgb):
    """jccolor.c: 16-bit fixed point, uint8 [h, w, 3] -> three int arrays"""
    r, g, b = (rgb[..., c].astype(np.int64) for c in range(3))
    y = (_fix(0.299) * r + _fix(0.587) * g + _fix(0.114) * b + 32768) >> 16
    cb = (-_fix(0.16874) * r - _fix(0.33126) * g + _fix(0.5) * b + (128 << 16) + 32767) >> 16
    cr = (_fix(0.5) * r - _fix(0.41869) * g - _fix(0.08131) * b + (128 << 16) + 32767) >> 16
    return y, cb, cr


def _extend(plane, rows, cols):
    """replicates the last row and the last column out to [rows, cols]"""
    return np.pad(plane, ((0, rows - plane.shape[0]), (0, cols - plane.shape[1])), mode="edge")


def h2v2(plane):
    """jcsample.c h2v2_downsample: an even-sized plane -> half size, the bias alternating 1, 2 along a row"""
    a, b, c, d = plane[0::2, 0::2], plane[0::2, 1::2], plane[1::2, 0::2], plane[1::2, 1::2]
    bias = np.where(np.arange(a.shape[1]) % 2 == 0, 1, 2)[None, :]
    return (a + b + c + d + bias) >> 2


def _descale(x, n):
    return (x + (1 << (n - 1))) >> n


def _dct_1d(d, first):
    """jfdctint.c, one pass along the LAST axis of d [..., 8]: CONST_BITS = 13, PASS1_BITS = 2"""
    d = [d[..., i] for i in range(8)]
    t0, t7, t1, t6 = d[0] + d[7], d[0] - d[7], d[1] + d[6], d[1] - d[6]
    t2, t5, t3, t4 = d[2] + d[5], d[2] - d[5], d[3] + d[4], d[3] - d[4]
    t10, t13, t11, t12 = t0 + t3, t0 - t3, t1 + t2, t1 - t2
    low = 13 - 2 if first else 13 + 2
    out = [None] * 8
    out[0] = (t10 + t11) << 2 if first else _descale(t10 + t11, 2)
    out[4] = (t10 - t11) << 2 if first else _descale(t10 - t11, 2)
    z1 = (t12 + t13) * 4433
    out[2] = _descale(z1 + t13 * 6270, low)
    out[6] = _descale(z1 - t12 * 15137, low)
    z1, z2, z3, z4 = t4 + t7, t5 + t6, t4 + t6, t5 + t7
    z5 = (z3 + z4) * 9633
    t4, t5, t6, t7 = t4 * 2446, t5 * 16819, t6 * 25172, t7 * 12299
    z1, z2, z3, z4 = z1 * -7373, z2 * -20995, z3 * -16069 + z5, z4 * -3196 + z5
    out[7] = _descale(t4 + z1 + z3, low)
    out[5] = _descale(t5 + z2 + z4, low)
    out[3] = _descale(t6 + z2 + z3, low)
    out[1] = _descale(t7 + z1 + z4, low)
    return np.stack(out, axis=-1)


def blocks_of(plane, table):
    """[rows of blocks, columns of blocks, 64] quantised coefficients in NATURAL order of a plane whose sides are multiples of 8"""
    bh, bw = plane.shape[0] // 8, plane.shape[1] // 8
    b = plane.reshape(bh, 8, bw, 8).transpose(0, 2, 1, 3) - 128                   # [bh, bw, row, column]
    b = _dct_1d(b, True)                                                          # rows first
    b = _dct_1d(b.transpose(0, 1, 3, 2), False).transpose(0, 1, 3, 2)             # then columns
    d = (table.reshape(8, 8) << 3)[None, None]
    return (np.sign(b) * ((np.abs(b) + (d >> 1)) // d)).reshape(bh, bw, 64)


def component_blocks(image, quality, subsampling):
    """[(quantised blocks [bh, bw, 64] in zigzag order, h sampling, v sampling)] of Y, Cb, Cr: the REAL blocks only"""
    h, w = image.shape[:2]
    y, cb, cr = ycbcr(image)
    tables = quant_table(LUMA_Q, quality), quant_table(CHROMA_Q, quality)
    up8 = lambda n: -(-n // 8) * 8
    out = [(blocks_of(_extend(y, up8(h), up8(w)), tables[0])[..., ZIGZAG], 2 if subsampling == "4:2:0" else 1)]
    for plane in (cb, cr):
        if subsampling == "4:2:0":
            ch, cw = -(-h // 2), -(-w // 2)
            # columns out to 16 per chroma block at full resolution, rows only to an even height; the rest below is the LAST
            # DOWNSAMPLED row again
            plane = _extend(h2v2(_extend(plane, 2 * ch, 2 * up8(cw))), up8(ch), up8(cw))
        else:
            plane = _extend(plane, up8(h), up8(w))
        out.append((blocks_of(plane, tables[1])[..., ZIGZAG], 1))
    return out


# ---- entropy coding ---------------------------------------------------------------------------------------------------------------
class _Bits:
    def __init__(self):
        self.acc, self.n, self.out = 0, 0, bytearray()

    def put(self, code, length):
        self.acc, self.n = (self.acc << length) | code, self.n + length
        while self.n >= 8:
            byte = (self.acc >> (self.n - 8)) & 0xFF
            self.out.append(byte)
            if byte == 0xFF:
                self.out.append(0)
            self.n -= 8
        self.acc &= (1 << self.n) - 1

    def flush(self):
        if self.n:
            self.put((1 << (8 - self.n)) - 1, 8 - self.n)
        return bytes(self.out)


def _magnitude(v):
    """(category, the low bits that follow the code)"""
    n = int(abs(v)).bit_length()
    return n, (v if v >= 0 else v - 1) & ((1 << n) - 1)


def _code_block(bits, block, pred, dc, ac):
    n, low = _magnitude(int(block[0]) - pred)
    bits.put(*dc[n])
    bits.put(low, n)
    run = 0
    for v in block[1:]:
        v = int(v)
        if v == 0:
            run += 1
            continue
        while run > 15:
            bits.put(*ac[0xF0])
            run -= 16
        n, low = _magnitude(v)
        bits.put(*ac[(run << 4) | n])
        bits.put(low, n)
        run = 0
    if run:
        bits.put(*ac[0x00])


def scan(image, quality=75, subsampling="4:2:0", stats=None):
    """The entropy-coded segment: one interleaved scan, MCU by MCU; `stats` (a dict) receives the counts of blocks, ZRL and EOB"""
    comps = component_blocks(image, quality, subsampling)
    dc = [huffman_codes(DC_LUMA), huffman_codes(DC_CHROMA), huffman_codes(DC_CHROMA)]
    ac = [huffman_codes(AC_LUMA), huffman_codes(AC_CHROMA), huffman_codes(AC_CHROMA)]
    h, w = image.shape[:2]
    side = 16 if subsampling == "4:2:0" else 8
    bits, pred, n_blocks = _Bits(), [0, 0, 0], 0
    for my in range(-(-h // side)):
        for mx in range(-(-w // side)):
            for c, (blocks, s) in enumerate(comps):
                last = None
                for by in range(s):
                    for bx in range(s):
                        y, x = my * s + by, mx * s + bx
                        if y < blocks.shape[0] and x < blocks.shape[1]:
                            block = blocks[y, x]
                        else:                       # a dummy block: the DC of the block before it in this MCU, no AC
                            block = np.zeros(64, dtype=np.int64)
                            block[0] = last[0]
                        _code_block(bits, block, pred[c], dc[c], ac[c])
                        pred[c], last, n_blocks = int(block[0]), block, n_blocks + 1
                        if stats is not None:
                            nz = np.flatnonzero(block[1:])
                            stats["eob"] = stats.get("eob", 0) + int(len(nz) == 0 or nz[-1] < 62)
                            stats["zrl"] = stats.get("zrl", 0) + int(sum((b - a - 1) // 16 for a, b in zip(np.r_[-1, nz[:-1]], nz)))
    if stats is not None:
        stats["blocks"] = n_blocks
    return bits.flush()


def encode(image, quality=75, subsampling="4:2:0"):
    """the whole file for uint8 [h, w, 3]"""
    image = np.asarray(image)
    assert image.dtype == np.uint8 and image.ndim == 3 and image.shape[2] == 3 and subsampling in SUBSAMPLINGS
    return header(image.shape[0], image.shape[1], quality, subsampling) + scan(image, quality, subsampling) + b"\xff\xd9"


def n_blocks(h, w, subsampling):
    side, per_mcu = (16, 6) if subsampling == "4:2:0" else (8, 3)
    return -(-h // side) * -(-w // side) * per_mcu


def capacity(h, w, subsampling):
    """The bound of include/mtgs_jpeg.h: the header, every block at its longest (a DC code of 11 bits with 11 more, 63 AC codes of
    16 bits with 10 more each), every byte of that stuffed, EOI."""
    return HEADER_BYTES + 2 * -(-n_blocks(h, w, subsampling) * BLOCK_BITS // 8) + 2


# ---- inputs -----------------------------------------------------------------------------------------------------------------------
def to_u8(x, conversion):
    """float32 -> uint8 as the presented frame's conversions: clamp to [0, 1] with NaN -> 0, times 255, (+ 0.5), truncated"""
    x = np.asarray(x, dtype=np.float32)
    x = np.where(x != x, np.float32(0), np.clip(x, np.float32(0), np.float32(1))).astype(np.float32)
    x = x * np.float32(255)
    if conversion == "round":
        x = x + np.float32(0.5)
    return x.astype(np.uint8)


KINDS = ("noise", "ramp", "checker", "blocks", "constant")


def images(kind, h, w, seed=0):
    """uint8 [h, w, 3]: uniform noise | a smooth ramp | a one-pixel checkerboard of 0 / 255 | alternating 8 x 8 blocks of 0 / 255
    (DC differences of the largest category) | a constant"""
    yy, xx = np.mgrid[0:h, 0:w]
    if kind == "noise":
        return np.random.default_rng(seed).integers(0, 256, (h, w, 3), dtype=np.uint8)
    if kind == "ramp":
        return np.stack([(255 * xx) // max(w - 1, 1), (255 * yy) // max(h - 1, 1), (255 * (xx + yy)) // max(h + w - 2, 1)], -1).astype(np.uint8)
    if kind == "checker":
        return np.repeat((((yy + xx) & 1) * 255)[..., None], 3, -1).astype(np.uint8)
    if kind == "blocks":
        return np.repeat(((((yy >> 3) + (xx >> 3)) & 1) * 255)[..., None], 3, -1).astype(np.uint8)
    if kind == "constant":
        return np.full((h, w, 3), (200, 30, 90), dtype=np.uint8)
    raise ValueError(kind)


# ---- the cases of the tests, and one encode of each for all of them ------------------------------------------------------------------
SIZES = [(1, 1), (2, 2), (7, 5), (8, 8), (12, 12), (16, 16), (17, 33), (24, 8), (31, 9), (9, 31), (40, 48), (64, 50)]
QUALITIES = (1, 40, 75, 95, 100)
_ENCODED = {}


def image_of(kind, h, w):
    return images(kind, h, w, seed=1000 * h + w)


def encoded(kind, h, w, quality, subsampling):
    """encode(image_of(kind, h, w), quality, subsampling), computed once per session"""
    key = (kind, h, w, quality, subsampling)
    if key not in _ENCODED:
        _ENCODED[key] = encode(image_of(kind, h, w), quality, subsampling)
    return _ENCODED[key]


def golden():
    """{(kind, h, w, quality, subsampling): (uint8 [h, w, 3], Pillow's bytes)} of tests/golden/jpeg_pillow.npz, and its default save"""
    from pathlib import Path
    out, default = {}, None
    with np.load(Path(__file__).resolve().parent / "golden" / "jpeg_pillow.npz") as z:
        for name in z.files:
            part = name.split("/")
            if part[0] == "jpg":
                kind, (h, w), q, s = part[1], map(int, part[2].split("x")), int(part[3]), {"420": "4:2:0", "444": "4:4:4"}[part[4]]
                out[(kind, h, w, q, s)] = (z[f"img/{kind}/{h}x{w}"], z[name].tobytes())
            elif part[0] == "default":
                default = (z["img/" + "/".join(part[1:])], z[name].tobytes())
    return out, default
