"""The indexed PNG codec of include/mtgs_png.h restated in NumPy and plain Python: the writer, the parser and the reader, and the
two depth rules.  Checked against zlib.decompress, zlib.adler32 and Pillow by tests/test_png_host.py; the kernels have one job: equal
it bit for bit (tests/test_gpu_png.py)."""
import struct
import zlib

import numpy as np

INDEX_VERSION = 1
LENGTH_BASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258]
LENGTH_EXTRA = [0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0]
CLC_ORDER = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]
SIGNATURE = b"\x89PNG\r\n\x1a\n"


def length_symbol(length):
    """(symbol - 257, extra bits, their value) of a match length 3..258"""
    if length == 258:
        return 28, 0, 0
    s = max(k for k in range(28) if LENGTH_BASE[k] <= length)
    return s, LENGTH_EXTRA[s], length - LENGTH_BASE[s]


# ---- the row stream ------------------------------------------------------------------------------------------------------------------
def file_pixels(image, order="rgb"):
    """uint8 [H, W, C] in the FILE's channel order from [H, W] or [H, W, 3] in `order`"""
    a = np.asarray(image)
    if a.ndim == 2:
        a = a[:, :, None]
    return np.ascontiguousarray(a[:, :, ::-1] if order == "bgr" else a)


def row_stream(pixels, filter):
    """uint8 [H, 1 + W * C]: the filter byte and the filtered bytes of every row"""
    h, w, c = pixels.shape
    p = pixels.astype(np.int32)
    pred = np.zeros_like(p)
    if filter == 1:
        pred[:, 1:] = p[:, :-1]
    elif filter == 2:
        pred[1:] = p[:-1]
    elif filter != 0:
        raise ValueError(filter)
    rows = np.empty((h, 1 + w * c), dtype=np.uint8)
    rows[:, 0] = filter
    rows[:, 1:] = ((p - pred) & 255).reshape(h, w * c)
    return rows


def unfilter(rows, h, w, c, filter):
    """uint8 [H, W, C] from the row stream"""
    d = rows.reshape(h, 1 + w * c)[:, 1:].reshape(h, w, c).astype(np.int64)
    if filter == 1:
        d = np.cumsum(d, axis=1)
    elif filter == 2:
        d = np.cumsum(d, axis=0)
    return (d & 255).astype(np.uint8)


def segments(h, row_bytes, segment_bytes):
    """[(start, length)] of every segment in the row stream"""
    out = []
    for y in range(h):
        for k in range(0, row_bytes, segment_bytes):
            out.append((y * row_bytes + k, min(segment_bytes, row_bytes - k)))
    return out


def tokens_of(segment):
    """[(literal,) or (length,)] as ('L', byte) / ('M', length): the tokens of one segment, by the per-position rule"""
    n = len(segment)
    out = []
    i = 0
    while i < n:
        j = i
        while j + 1 < n and segment[j + 1] == segment[i]:
            j += 1
        r = j - i
        for p in range(r + 1):
            if p == 0:
                out.append(("L", int(segment[i])))
                continue
            q = (p - 1) // 258
            rem = r - 258 * q
            if rem >= 3:
                if (p - 1) % 258 == 0:
                    out.append(("M", min(rem, 258)))
            else:
                out.append(("L", int(segment[i])))
        i = j + 1
    return out


# ---- the code builder ----------------------------------------------------------------------------------------------------------------
def build_lengths(counts, limit):
    """code lengths of the symbols with a count: two-queue Huffman, Annex K.2's limit, lengths by (count descending, symbol)"""
    used = sorted((c, s) for s, c in enumerate(counts) if c > 0)
    m = len(used)
    lengths = [0] * len(counts)
    if m == 0:
        return lengths
    bits = [0] * (max(len(counts), limit) + 34)
    if m == 1:
        bits[1] = 1
    else:
        w_leaf = [c for c, _ in used]
        w_int, par_leaf, par_int = [], [0] * m, [0] * m
        li = ii = 0
        for _ in range(m - 1):
            total = 0
            for _ in range(2):
                if li < m and (ii >= len(w_int) or w_leaf[li] <= w_int[ii]):
                    total += w_leaf[li]
                    par_leaf[li] = len(w_int)
                    li += 1
                else:
                    total += w_int[ii]
                    par_int[ii] = len(w_int)
                    ii += 1
            w_int.append(total)
        for leaf in range(m):
            d, node = 1, par_leaf[leaf]
            while node != m - 2:
                node = par_int[node]
                d += 1
            bits[d] += 1
        for i in range(m - 1, limit, -1):
            while bits[i] > 0:
                j = i - 2
                while bits[j] == 0:
                    j -= 1
                bits[i] -= 2
                bits[i - 1] += 1
                bits[j + 1] += 2
                bits[j] -= 1
    order = sorted(((-c, s) for c, s in used))
    k = 0
    for length in range(1, limit + 1):
        for _ in range(bits[length]):
            lengths[order[k][1]] = length
            k += 1
    assert k == m
    return lengths


def canonical_codes(lengths):
    """RFC 1951 3.2.2: code of every symbol (MSB first, as an integer)"""
    top = max(lengths) if lengths else 0
    bl = [0] * (top + 2)
    for n in lengths:
        if n:
            bl[n] += 1
    code, nxt = 0, [0] * (top + 2)
    for n in range(1, top + 1):
        code = (code + bl[n - 1]) << 1
        nxt[n] = code
    codes = [0] * len(lengths)
    for s, n in enumerate(lengths):
        if n:
            codes[s] = nxt[n]
            nxt[n] += 1
    return codes


def reverse_bits(value, n):
    return int(format(value, "0%db" % n)[::-1], 2) if n else 0


class BitWriter:
    def __init__(self):
        self.acc, self.n = 0, 0

    def put(self, value, n):
        """n bits of value, LSB first"""
        self.acc |= value << self.n
        self.n += n

    def put_code(self, code, n):
        self.put(reverse_bits(code, n), n)

    def tobytes(self):
        return self.acc.to_bytes((self.n + 7) // 8, "little")


def length_sequence(lit_lengths):
    """(hlit, [(symbol, extra bits, value)]) of the code-length sequence: the lit/len lengths, then the distance length"""
    hlit = 257
    for s in range(285, 256, -1):
        if lit_lengths[s]:
            hlit = s + 1
            break
    seq = list(lit_lengths[:hlit]) + [1 if hlit > 257 else 0]
    out, i = [], 0
    while i < len(seq):
        if seq[i]:
            out.append((seq[i], 0, 0))
            i += 1
            continue
        z = 0
        while i + z < len(seq) and seq[i + z] == 0:
            z += 1
        i += z
        while z >= 11:
            k = min(z, 138)
            out.append((18, 7, k - 11))
            z -= k
        if z >= 3:
            out.append((17, 3, z - 3))
            z = 0
        out.extend([(0, 0, 0)] * z)
    return hlit, out


# ---- the writer ----------------------------------------------------------------------------------------------------------------------
def chunk(name, body):
    return struct.pack(">I", len(body)) + name + body + struct.pack(">I", zlib.crc32(name + body))


def encode(image, filter=1, segment_bytes=512, order="rgb", details=None):
    """The file of uint8 `image` [H, W] or [H, W, 3].  `details` (a dict) receives the row stream, the payload and the index."""
    pixels = file_pixels(image, order)
    h, w, c = pixels.shape
    rows = row_stream(pixels, filter)
    stream = rows.reshape(-1)
    segs = segments(h, rows.shape[1], segment_bytes)
    toks = [tokens_of(stream[a:a + n]) for a, n in segs]
    counts = [0] * 286
    counts[256] = 1
    for seg in toks:
        for kind, v in seg:
            counts[v if kind == "L" else 257 + length_symbol(v)[0]] += 1
    lit_len = build_lengths(counts, 15)
    lit_code = canonical_codes(lit_len)
    hlit, seq = length_sequence(lit_len)
    clc_counts = [0] * 19
    for s, _, _ in seq:
        clc_counts[s] += 1
    clc_len = build_lengths(clc_counts, 7)
    clc_code = canonical_codes(clc_len)
    hclen = 19
    while hclen > 4 and clc_len[CLC_ORDER[hclen - 1]] == 0:
        hclen -= 1
    out = BitWriter()
    out.put(0x78, 8)
    out.put(0x01, 8)
    out.put(1, 1)
    out.put(2, 2)
    out.put(hlit - 257, 5)
    out.put(0, 5)
    out.put(hclen - 4, 4)
    for k in range(hclen):
        out.put(clc_len[CLC_ORDER[k]], 3)
    for s, n, v in seq:
        out.put_code(clc_code[s], clc_len[s])
        out.put(v, n)
    offsets = []
    for seg in toks:
        offsets.append(out.n)
        for kind, v in seg:
            if kind == "L":
                out.put_code(lit_code[v], lit_len[v])
            else:
                s, n, extra = length_symbol(v)
                out.put_code(lit_code[257 + s], lit_len[257 + s])
                out.put(extra, n)
                out.put(0, 1)
    eob = out.n
    out.put_code(lit_code[256], lit_len[256])
    if out.n >= 1 << 32:
        raise ValueError("the stream exceeds 2^32 bits")
    payload = out.tobytes() + struct.pack(">I", zlib.adler32(stream.tobytes()))
    index = struct.pack("<%dI" % (5 + len(segs)), INDEX_VERSION, filter, segment_bytes, len(segs), *offsets, eob)
    if details is not None:
        details.update(stream=stream, payload=payload, offsets=offsets, eob=eob, lit_lengths=lit_len, clc_lengths=clc_len, tokens=toks)
    ihdr = struct.pack(">IIBBBBB", w, h, 8, 2 if c == 3 else 0, 0, 0, 0)
    return SIGNATURE + chunk(b"IHDR", ihdr) + chunk(b"mtIX", index) + chunk(b"IDAT", payload) + chunk(b"IEND", b"")


# ---- the parser and the reader -------------------------------------------------------------------------------------------------------
class BitReader:
    def __init__(self, data, at=0):
        self.value, self.at, self.limit = int.from_bytes(data, "little"), at, 8 * len(data)

    def take(self, n):
        v = (self.value >> self.at) & ((1 << n) - 1)
        self.at += n
        return v


def decode_table(lengths):
    """{(length, code MSB first): symbol}"""
    codes = canonical_codes(lengths)
    return {(n, codes[s]): s for s, n in enumerate(lengths) if n}


def read_symbol(bits, table, longest):
    code = 0
    for n in range(1, longest + 1):
        code = (code << 1) | bits.take(1)
        if (n, code) in table:
            return table[(n, code)]
    return None


def parse(data):
    """dict: height, width, channels, filter, segment_bytes, offsets, eob, payload, lit_lengths, dist_length, first_token_bit"""
    assert data[:8] == SIGNATURE
    at, chunks = 8, []
    while at < len(data):
        n, name = struct.unpack(">I4s", data[at:at + 8])
        chunks.append((name, data[at + 8:at + 8 + n]))
        at += 12 + n
    assert [c[0] for c in chunks] == [b"IHDR", b"mtIX", b"IDAT", b"IEND"]
    w, h, depth, colour, _, _, interlace = struct.unpack(">IIBBBBB", chunks[0][1])
    assert depth == 8 and colour in (0, 2) and interlace == 0
    index = chunks[1][1]
    version, filter, segment_bytes, n = struct.unpack("<4I", index[:16])
    assert version == INDEX_VERSION
    words = struct.unpack("<%dI" % (n + 1), index[16:])
    payload = chunks[2][1]
    bits = BitReader(payload, 16)
    assert payload[:2] == b"\x78\x01" and bits.take(1) == 1 and bits.take(2) == 2
    hlit, hdist, hclen = bits.take(5) + 257, bits.take(5) + 1, bits.take(4) + 4
    clc = [0] * 19
    for k in range(hclen):
        clc[CLC_ORDER[k]] = bits.take(3)
    table = decode_table(clc)
    lengths = []
    while len(lengths) < hlit + hdist:
        s = read_symbol(bits, table, 7)
        if s < 16:
            lengths.append(s)
        elif s == 17:
            lengths.extend([0] * (3 + bits.take(3)))
        elif s == 18:
            lengths.extend([0] * (11 + bits.take(7)))
        else:
            raise ValueError("symbol 16")
    assert len(lengths) == hlit + hdist and hdist == 1
    return dict(height=h, width=w, channels=3 if colour == 2 else 1, filter=filter, segment_bytes=segment_bytes, offsets=list(words[:n]),
                eob=words[n], payload=payload, lit_lengths=lengths[:hlit] + [0] * (286 - hlit), dist_length=lengths[hlit],
                first_token_bit=bits.at)


def inflate_segments(info, payload=None):
    """(the row stream, segments decoded, every segment stayed inside its own bytes and the payload) by the indexed reader: every
    segment from its bit offset, alone.  `payload` replaces the file's (a corrupted copy)."""
    payload = info["payload"] if payload is None else payload
    h, row_bytes = info["height"], 1 + info["width"] * info["channels"]
    table = decode_table(info["lit_lengths"])
    stream = np.zeros(h * row_bytes, dtype=np.uint8)
    ends = info["offsets"][1:] + [info["eob"]]
    good, inside = 0, True
    for (start, n), offset, end in zip(segments(h, row_bytes, info["segment_bytes"]), info["offsets"], ends):
        bits = BitReader(payload, offset)
        produced, prev, bad = 0, 0, False
        while produced < n:
            s = read_symbol(bits, table, 15)
            if s is None or s == 256 or s > 285:
                bad = True
                break
            if s < 256:
                prev, m = s, 1
            else:
                m = LENGTH_BASE[s - 257] + bits.take(LENGTH_EXTRA[s - 257])
                if produced == 0 or not info["dist_length"] or bits.take(1) != 0 or m > n - produced:
                    bad = True
                    break
            stream[start + produced:start + produced + m] = prev
            produced += m
        inside = inside and bits.at <= bits.limit
        good += not bad and bits.at == end
    return stream, good, inside


def decode(data, order="rgb"):
    """uint8 [H, W] or [H, W, 3] in `order` from a file of this writer, by the indexed reader"""
    info = parse(data)
    stream, good, _ = inflate_segments(info)
    assert good == len(info["offsets"])
    assert zlib.adler32(stream.tobytes()) == struct.unpack(">I", info["payload"][-4:])[0]
    px = unfilter(stream, info["height"], info["width"], info["channels"], info["filter"])
    if info["channels"] == 1:
        return px[:, :, 0]
    return px[:, :, ::-1] if order == "bgr" else px


def fibonacci_image():
    """uint8 [233, 321], about 75 000 bytes, whose token histogram under filter 0 is Fibonacci-weighted, so that the unlimited Huffman
    code is 22 bits deep: end-of-block counts 1, the filter byte 0 counts 233 (one per row), pixel value 7 k + 1 counts the k-th other
    Fibonacci number up to 28657 (the last takes the 3 bytes that fill the rectangle).  No two neighbours are equal (always the most
    frequent value left that differs from the one before), so no match takes a literal away."""
    import heapq
    fib = [1, 2]
    while fib[-1] < 28657:
        fib.append(fib[-1] + fib[-2])
    fib.remove(233)
    fib[-1] += 233 * 321 - sum(fib)
    heap = [(-c, 7 * k + 1) for k, c in enumerate(fib)]
    heapq.heapify(heap)
    out, prev = [], None
    while heap:
        first = heapq.heappop(heap)
        if first[1] == prev:
            second = heapq.heappop(heap)
            heapq.heappush(heap, first)
            first = second
        out.append(first[1])
        prev = first[1]
        if first[0] + 1:
            heapq.heappush(heap, (first[0] + 1, first[1]))
    return np.array(out, dtype=np.uint8).reshape(233, 321)


# ---- the reference's two depth rules -------------------------------------------------------------------------------------------------
def depth_image(depth, raw_size, roi, max_range=80, min_depth=0.1):
    """nuplan_scripts/generate_dense_depth.py:236-247: the [H, W, 3] uint8 array handed to cv2.imwrite (OpenCV's channel order)"""
    depth = np.array(depth, dtype=np.float32)
    x, y, w, h = roi
    with np.errstate(invalid="ignore"):
        depth[depth > max_range] = 0
        depth[depth < np.float32(min_depth)] = 0
        depth[np.isnan(depth)] = 0              # the cast of a NaN is no defined byte; the project's rule is 0
        image = np.zeros((raw_size[0], raw_size[1], 3), dtype=np.uint8)
        image[y:y + h, x:x + w, 0] = ((depth * 100) % 256).astype(np.uint8)
        image[y:y + h, x:x + w, 1] = ((depth * 100) // 256).astype(np.uint8)
    return image


def depth_from_image(image):
    """mtgs/dataset/custom_dataset.py:166-168 on the array cv2.imread returns (OpenCV's channel order): float32 [H, W, 1]"""
    depth_img = np.asarray(image).astype(np.float32)
    depth = depth_img[:, :, 0] + (depth_img[:, :, 1] * 256.0)
    depth = depth * 0.01
    return depth[:, :, None]
