"""The reference of mtgs_amd.jpegdec (tests/test_jpegdec_host.py, tests/test_gpu_jpegdec.py): a baseline JPEG decoder in plain NumPy,
stage by stage as include/mtgs_jpegdec.h states the arithmetic -- libjpeg's integer islow IDCT, fancy upsampling and 16-bit
fixed-point colour, which is what np.array(Image.open(...)) gives with Pillow 12.2.0 -- and a model of the synchronisation of the
parallel entropy decode.  Written for reading: a Python loop over the symbols, whole-image arrays for the pixel stages.  It reads the
file with a parser of its own, not mtgs_amd.jpegdec.parse_jpeg.

    decode(data)             uint8 [H, W, 3], by the SERIAL decoder
    read(data)               the header as a File (sizes, sampling, tables, the clean stream, the interval starts)
    serial_states(f, bits)   the serial decoder's state at the first bit of every subsequence
    entries(f, bits)         the entry states after the fixed-point iteration has converged
    steps(f, bits)           the whole-stream steps it took, the confirming one included
    golden()                 the cases of tests/golden/jpegdec_pillow.npz
"""
from pathlib import Path
from types import SimpleNamespace

import numpy as np

from tests import jpeg_refs

ZIGZAG = jpeg_refs.ZIGZAG
SUBSAMPLINGS = {(1, 1): "4:4:4", (2, 1): "4:2:2", (2, 2): "4:2:0"}


# ---- the file ---------------------------------------------------------------------------------------------------------------------
def _lut(bits, vals):
    """[65536] (length, symbol) by the next 16 bits; length 0 where no code starts"""
    lut = [(0, 0)] * 65536
    for symbol, (code, length) in jpeg_refs.huffman_codes((bits, vals)).items():
        lo = code << (16 - length)
        lut[lo:lo + (1 << (16 - length))] = [(length, symbol)] * (1 << (16 - length))
    return lut


def read(data):
    """The header's fields, the clean stream (stuffed zeros and restart markers removed) and the clean byte each interval starts at"""
    assert data[:2] == b"\xff\xd8"
    f = SimpleNamespace(quant={}, huff={}, restart=0)
    at = 2
    while True:
        while data[at + 1] == 0xFF:
            at += 1
        marker, length = data[at + 1], int.from_bytes(data[at + 2:at + 4], "big")
        body = data[at + 4:at + 2 + length]
        at += 2 + length
        if marker == 0xDB:
            for k in range(0, len(body), 65):
                table = np.zeros(64, dtype=np.int64)
                table[ZIGZAG] = list(body[k + 1:k + 65])
                f.quant[body[k]] = table
        elif marker == 0xC4:
            k = 0
            while k < len(body):
                n = sum(body[k + 1:k + 17])
                f.huff[(body[k] >> 4, body[k] & 15)] = (list(body[k + 1:k + 17]), list(body[k + 17:k + 17 + n]))
                k += 17 + n
        elif marker == 0xDD:
            f.restart = int.from_bytes(body, "big")
        elif marker == 0xC0:
            f.h, f.w = int.from_bytes(body[1:3], "big"), int.from_bytes(body[3:5], "big")
            f.sampling = [(body[7 + 3 * c] >> 4, body[7 + 3 * c] & 15) for c in range(3)]
            f.tq = [body[8 + 3 * c] for c in range(3)]
        elif marker == 0xDA:
            f.selectors = [(body[2 + 2 * c] >> 4, body[2 + 2 * c] & 15) for c in range(3)]
            break
    f.hs, f.vs = f.sampling[0]
    f.subsampling = SUBSAMPLINGS[f.sampling[0]]
    f.nb = f.hs * f.vs + 2
    f.mcus_x, f.mcus_y = -(-f.w // (8 * f.hs)), -(-f.h // (8 * f.vs))
    n_mcu = f.mcus_x * f.mcus_y
    f.ri = f.restart if 0 < f.restart < n_mcu else n_mcu
    f.n_int = -(-n_mcu // f.ri)
    f.n_blocks = n_mcu * f.nb
    f.interval_blocks = [min(f.ri * f.nb, f.n_blocks - k * f.ri * f.nb) for k in range(f.n_int)]
    f.scan_offset = at
    end = data.rindex(b"\xff\xd9")
    f.scan = data[at:end]
    clean, starts, k = bytearray(), [0], 0
    while k < len(f.scan):
        b = f.scan[k]
        if b == 0xFF and k + 1 < len(f.scan) and f.scan[k + 1] == 0x00:
            clean.append(0xFF)
            k += 2
        elif b == 0xFF and k + 1 < len(f.scan) and 0xD0 <= f.scan[k + 1] <= 0xD7:
            starts.append(len(clean))
            k += 2
        else:
            clean.append(b)
            k += 1
    assert len(starts) == f.n_int
    f.clean, f.starts = bytes(clean), starts + [len(clean)]
    padded = np.frombuffer(f.clean + b"\xff" * 16, dtype=np.uint8).astype(np.uint64)
    window = np.zeros(len(f.clean) + 8, dtype=np.uint64)
    for j in range(6):                                      # 48 bits from every byte
        window = (window << np.uint64(8)) | padded[j:j + len(window)]
    f.window = window.tolist()
    f.dc = [_lut(*f.huff[(0, td)]) for td, _ in f.selectors]
    f.ac = [_lut(*f.huff[(1, ta)]) for _, ta in f.selectors]
    f.comp = [0] * (f.nb - 2) + [1, 2]
    return f


# ---- the decoder's step --------------------------------------------------------------------------------------------------------------
def _bits(f, p, n):
    """the n <= 32 bits at bit p of the clean stream (ones beyond its end)"""
    at = min(p >> 3, len(f.window) - 1)
    return (f.window[at] >> (48 - (p & 7) - n)) & ((1 << n) - 1)


def _extend(v, cat):
    return v - (1 << cat) + 1 if cat and v < (1 << (cat - 1)) else v


def run(f, state, end, sink=None):
    """Decodes from state = (bit, block within the MCU, zigzag index) until the bit reaches `end`; returns (the state there, the
    blocks completed).  A prefix that is no code skips one bit.  sink(blocks completed so far, zigzag index, value) per coefficient."""
    p, blk, zz = state
    done = 0
    while p < end:
        comp = f.comp[blk]
        length, symbol = (f.dc if zz == 0 else f.ac)[comp][_bits(f, p, 16)]
        if length == 0:
            p += 1
            continue
        run_, cat = symbol >> 4, symbol & 15
        value = _extend(_bits(f, p + length, cat), cat) if cat else 0
        p += length + cat
        if zz == 0:
            if sink:
                sink(done, 0, value)
            zz = 1
        elif cat:
            k = zz + run_
            if sink and k <= 63:
                sink(done, k, value)
            zz = k + 1
        else:
            zz = zz + 16 if run_ == 15 else 64
        if zz > 63:
            zz, blk, done = 0, (blk + 1) % f.nb, done + 1
    return (p, blk, zz), done


def coefficients(f):
    """int64 [n_blocks, 64] in NATURAL order, the DC predicted: the serial decoder, interval by interval, block by block"""
    coef = np.zeros((f.n_blocks, 64), dtype=np.int64)
    for k in range(f.n_int):
        first, state, pred = k * f.ri * f.nb, (8 * f.starts[k], 0, 0), [0, 0, 0]
        for i in range(first, first + f.interval_blocks[k]):
            def sink(_, z, v, i=i):
                coef[i, ZIGZAG[z]] = v
            p = state[0]
            while True:                                     # one block: until a block completes
                state, done = run(f, state, state[0] + 1, sink)
                if done:
                    break
                assert state[0] <= 8 * f.starts[k + 1] + 64, "ran off the interval"
            comp = f.comp[i % f.nb]
            pred[comp] += coef[i, 0]
            coef[i, 0] = pred[comp]
            assert state[0] > p
    return coef


# ---- the pixel stages ----------------------------------------------------------------------------------------------------------------
def _idct_1d(d):
    """jidctint.c's islow butterfly along the LAST axis, before the descale"""
    d = [d[..., i] for i in range(8)]
    z1 = (d[2] + d[6]) * 4433
    e2, e3 = z1 - d[6] * 15137, z1 + d[2] * 6270
    e0, e1 = (d[0] + d[4]) << 13, (d[0] - d[4]) << 13
    t10, t13, t11, t12 = e0 + e3, e0 - e3, e1 + e2, e1 - e2
    t0, t1, t2, t3 = d[7], d[5], d[3], d[1]
    z1, z2, z3, z4 = t0 + t3, t1 + t2, t0 + t2, t1 + t3
    z5 = (z3 + z4) * 9633
    t0, t1, t2, t3 = t0 * 2446, t1 * 16819, t2 * 25172, t3 * 12299
    z1, z2, z3, z4 = z1 * -7373, z2 * -20995, z3 * -16069 + z5, z4 * -3196 + z5
    t0, t1, t2, t3 = t0 + z1 + z3, t1 + z2 + z4, t2 + z2 + z3, t3 + z1 + z4
    return np.stack([t10 + t3, t11 + t2, t12 + t1, t13 + t0, t13 - t0, t12 - t1, t11 - t2, t10 - t3], axis=-1)


def _descale(x, n):
    return (x + (1 << (n - 1))) >> n


def planes(f, coef):
    """[Y, Cb, Cr] at component resolution, padded to whole MCUs"""
    out = [np.zeros((f.mcus_y * 8 * (f.vs if c == 0 else 1), f.mcus_x * 8 * (f.hs if c == 0 else 1)), dtype=np.int64) for c in range(3)]
    comp = np.array(f.comp)[np.arange(f.n_blocks) % f.nb]
    quant = np.stack([f.quant[t] for t in f.tq])[comp]
    b = (coef * quant).reshape(-1, 8, 8)                                    # [block, row, column]
    b = _descale(_idct_1d(b.transpose(0, 2, 1)), 11).transpose(0, 2, 1)     # columns
    b = np.clip(_descale(_idct_1d(b), 18) + 128, 0, 255)                    # rows
    for i in range(f.n_blocks):
        mcu, j = divmod(i, f.nb)
        my, mx = divmod(mcu, f.mcus_x)
        c = comp[i]
        by, bx = (my * f.vs + j // f.hs, mx * f.hs + j % f.hs) if c == 0 else (my, mx)
        out[c][8 * by:8 * by + 8, 8 * bx:8 * bx + 8] = b[i]
    return out


def _h2v1(c):
    """jdsample.c h2v1_fancy_upsample on the TRUE width of the component"""
    left, right = np.roll(c, 1, axis=1), np.roll(c, -1, axis=1)
    even, odd = (3 * c + left + 1) >> 2, (3 * c + right + 2) >> 2
    even[:, 0], odd[:, -1] = c[:, 0], c[:, -1]
    return np.stack([even, odd], axis=-1).reshape(c.shape[0], -1)


def _h2v2(c):
    """jdsample.c h2v2_fancy_upsample on the TRUE size of the component"""
    above, below = np.vstack([c[:1], c[:-1]]), np.vstack([c[1:], c[-1:]])
    s = np.stack([3 * c + above, 3 * c + below], axis=1).reshape(-1, c.shape[1])
    left, right = np.roll(s, 1, axis=1), np.roll(s, -1, axis=1)
    even, odd = (3 * s + left + 8) >> 4, (3 * s + right + 7) >> 4
    even[:, 0], odd[:, -1] = (4 * s[:, 0] + 8) >> 4, (4 * s[:, -1] + 7) >> 4
    return np.stack([even, odd], axis=-1).reshape(s.shape[0], -1)


def pixels(f, coef, replicate_narrow=True):
    """uint8 [H, W, 3]; replicate_narrow=False applies the fancy rule to every width, which libjpeg does not (for the tests)"""
    y, cb, cr = planes(f, coef)
    ch, cw = -(-f.h // f.vs), -(-f.w // f.hs)
    if f.hs == 2 and (cw > 2 or not replicate_narrow):
        up = _h2v2 if f.vs == 2 else _h2v1
        cb, cr = up(cb[:ch, :cw]), up(cr[:ch, :cw])
    elif f.hs == 2:                        # jdsample.c takes the fancy path only for components wider than two samples: replication
        cb, cr = (np.repeat(np.repeat(c[:ch, :cw], f.vs, axis=0), 2, axis=1) for c in (cb, cr))
    y, cb, cr = y[:f.h, :f.w], cb[:f.h, :f.w] - 128, cr[:f.h, :f.w] - 128
    r = y + ((91881 * cr + 32768) >> 16)
    g = y + ((-22554 * cb - 46802 * cr + 32768) >> 16)
    b = y + ((116130 * cb + 32768) >> 16)
    return np.clip(np.stack([r, g, b], axis=-1), 0, 255).astype(np.uint8)


_DECODED = {}


def decode(data):
    """uint8 [H, W, 3]; computed once per file and session (do not write into it)"""
    if data not in _DECODED:
        f = read(data)
        _DECODED[data] = pixels(f, coefficients(f))
        _DECODED[data].setflags(write=False)
    return _DECODED[data]


# ---- the synchronisation model -------------------------------------------------------------------------------------------------------
def subsequences(f, bits):
    """[(first bit, last bit, starts an interval)]: every interval cut into pieces of `bits` bits"""
    out = []
    for k in range(f.n_int):
        begin, stop = 8 * f.starts[k], 8 * f.starts[k + 1]
        n = max(1, -(-(stop - begin) // bits))
        out += [(min(begin + j * bits, stop), min(begin + (j + 1) * bits, stop), j == 0) for j in range(n)]
    return out


def serial_states(f, bits):
    """the serial decoder's state at the first bit it reads at or behind the start of every subsequence"""
    out = []
    for begin, end, first in subsequences(f, bits):
        state = (begin, 0, 0) if first else run(f, out[-1], begin)[0]
        out.append(state)
    return out


def _iterate(f, bits):
    subs = subsequences(f, bits)
    entry = [(b, 0, 0) for b, _, _ in subs]
    dirty, n_steps = [True] * len(subs), 0
    while True:
        n_steps += 1
        exits = {i: run(f, entry[i], subs[i][1])[0] for i in range(len(subs)) if dirty[i]}
        dirty = [False] * len(subs)
        for i, x in exits.items():
            if i + 1 < len(subs) and not subs[i + 1][2] and entry[i + 1] != x:
                entry[i + 1], dirty[i + 1] = x, True
        if not any(dirty):
            return entry, n_steps


def entries(f, bits):
    return _iterate(f, bits)[0]


def steps(f, bits):
    return _iterate(f, bits)[1]


# ---- the cases ---------------------------------------------------------------------------------------------------------------------
SIZES = [(1, 1), (8, 8), (7, 9), (16, 16), (17, 17), (9, 33), (31, 50), (48, 65)]
NARROW = [(3, 2), (2, 3), (6, 4), (5, 3), (4, 4)]      # chroma one or two samples wide at 4:2:2 / 4:2:0: libjpeg replicates it
KINDS = jpeg_refs.KINDS
QUALITIES = (1, 75, 100)
WORST = dict(seed=48065, shape=(48, 65, 3), quality=95, subsampling=2, optimize=True)


def image_of(kind, h, w):
    return jpeg_refs.images(kind, h, w, seed=1000 * h + w)


def worst_image():
    return np.random.default_rng(WORST["seed"]).integers(0, 256, WORST["shape"], dtype=np.uint8)


def golden():
    """{name: (the file's bytes, Pillow's uint8 [H, W, 3])} of tests/golden/jpegdec_pillow.npz"""
    out = {}
    with np.load(Path(__file__).resolve().parent / "golden" / "jpegdec_pillow.npz") as z:
        jpg, pix = z["jpg"].tobytes(), z["pix"]
        at = p = 0
        for name, n, (h, w) in zip(z["names"].tolist(), z["jpg_bytes"].tolist(), z["shapes"].tolist()):
            out[name] = (jpg[at:at + n], pix[p:p + h * w * 3].reshape(h, w, 3))
            at, p = at + n, p + h * w * 3
    return out
