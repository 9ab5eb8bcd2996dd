"""A float64 restatement of the baseline JPEG of DESIGN.md section 6m: colour transform, padding, chroma mean, DCT and
quantisation in numpy, a plain sequential bit writer, and a decoder (dequantise, float IDCT, colour) that limits each
component to 0..255 after the IDCT as libjpeg does.  Nothing here is shared with csrc/jpeg_math.h: the tables are
written out a second time (tests/test_jpeg_cpu.py compares them with the DHT and DQT segments libjpeg writes)."""
import numpy as np

ZIGZAG = np.array(sorted(range(64), key=lambda i: (i // 8 + i % 8,
                                                   i // 8 if (i // 8 + i % 8) % 2 else i % 8)), np.int64)  # zigzag k -> v*8+u
LUMA_Q = np.array([16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56,
                   14, 17, 22, 29, 51, 87, 80, 62, 18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92,
                   49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99], np.int64)
CHROMA_Q = np.array([17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99,
                     47, 66, 99, 99, 99, 99, 99, 99] + [99] * 32, np.int64)
DC_LUMA = ([0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0], list(range(12)))
DC_CHROMA = ([0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0], list(range(12)))
AC_LUMA = ([0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7d], list(bytes.fromhex(
    "01020300041105122131410613516107227114328191a1082342b1c11552d1f02433627282090a161718191a25262728292a3435363738"
    "393a434445464748494a535455565758595a636465666768696a737475767778797a838485868788898a92939495969798999aa2a3a4a5"
    "a6a7a8a9aab2b3b4b5b6b7b8b9bac2c3c4c5c6c7c8c9cad2d3d4d5d6d7d8d9dae1e2e3e4e5e6e7e8e9eaf1f2f3f4f5f6f7f8f9fa")))
AC_CHROMA = ([0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77], list(bytes.fromhex(
    "000102031104052131061241510761711322328108144291a1b1c109233352f0156272d10a162434e125f11718191a262728292a353637"
    "38393a434445464748494a535455565758595a636465666768696a737475767778797a82838485868788898a92939495969798999aa2a3"
    "a4a5a6a7a8a9aab2b3b4b5b6b7b8b9bac2c3c4c5c6c7c8c9cad2d3d4d5d6d7d8d9dae2e3e4e5e6e7e8e9eaf2f3f4f5f6f7f8f9fa")))


def dct_matrix():
    u, x = np.arange(8)[:, None], np.arange(8)[None, :]
    c = 0.5 * np.cos((2 * x + 1) * u * np.pi / 16)
    c[0] = np.sqrt(1 / 8)
    return c                                                    # C[u][x]


def scaled_tables(quality):
    s = 5000 // quality if quality < 50 else 200 - 2 * quality
    return tuple(np.clip((t * s + 50) // 100, 1, 255) for t in (LUMA_Q, CHROMA_Q))


def huffman_codes(table):
    """symbol -> (code, length), T.81 Annex C."""
    bits, vals = table
    codes, code, k = {}, 0, 0
    for length in range(1, 17):
        for _ in range(bits[length - 1]):
            codes[vals[k]] = (code, length)
            code, k = code + 1, k + 1
        code <<= 1
    return codes


def geometry(width, height, subsampling):
    m = 16 if subsampling == "420" else 8
    return m, -(-width // m), -(-height // m)                    # MCU side, MCUs across, MCUs down


def default_restart(width, subsampling):
    return geometry(width, 1, subsampling)[1]


def planes(img, subsampling):
    """uint8 [H, W, 3] -> (Y, Cb, Cr) float64 planes, padded to whole MCUs by edge repetition, chroma averaged 2x2."""
    h, w, _ = img.shape
    m, mx, my = geometry(w, h, subsampling)
    p = np.pad(img.astype(np.float64), ((0, my * m - h), (0, mx * m - w), (0, 0)), mode="edge")
    r, g, b = p[..., 0], p[..., 1], p[..., 2]
    y = 0.299 * r + 0.587 * g + 0.114 * b - 128
    cb = -0.168735892 * r - 0.331264108 * g + 0.5 * b
    cr = 0.5 * r - 0.418687589 * g - 0.081312411 * b
    if subsampling == "420":
        cb, cr = (c.reshape(c.shape[0] // 2, 2, c.shape[1] // 2, 2).mean(axis=(1, 3)) for c in (cb, cr))
    return y, cb, cr


def _blocks(plane):
    h, w = plane.shape
    return plane.reshape(h // 8, 8, w // 8, 8).transpose(0, 2, 1, 3)      # [rows, cols, y, x]


def transform(img, quality, subsampling):
    """-> ([Y, Cb, Cr] int64 [rows, cols, 64] in zigzag order, the unrounded quotients c / q, the divisors q)."""
    c = dct_matrix()
    lq, cq = scaled_tables(quality)
    out, quot, div = [], [], []
    for plane, q in zip(planes(img, subsampling), (lq, cq, cq)):
        b = _blocks(plane)
        f = np.einsum("vy,rcyx,ux->rcvu", c, b, c).reshape(b.shape[0], b.shape[1], 64)[..., ZIGZAG]
        qz = q[ZIGZAG].astype(np.float64)
        quot.append(f / qz)
        div.append(np.broadcast_to(qz, f.shape))
        out.append(np.rint(f / qz).astype(np.int64))
    return out, quot, div


def scan_order(coefs, subsampling):
    """[Y, Cb, Cr] -> (int64 [blocks, 64] in scan order, component index per block, blocks per MCU)."""
    y, cb, cr = coefs
    my, mx = cb.shape[:2]
    if subsampling == "420":
        yy = y.reshape(my, 2, mx, 2, 64).transpose(0, 2, 1, 3, 4).reshape(my, mx, 4, 64)
        comp = [0, 0, 0, 0, 1, 2]
    else:
        yy = y.reshape(my, mx, 1, 64)
        comp = [0, 1, 2]
    mcus = np.concatenate([yy, cb[:, :, None], cr[:, :, None]], axis=2)
    return mcus.reshape(-1, 64), np.tile(comp, my * mx), len(comp)


def header(width, height, quality, subsampling, restart_interval):
    lq, cq = scaled_tables(quality)
    out = bytearray(b"\xff\xd8\xff\xe0\x00\x10JFIF\x00\x01\x01\x00\x00\x01\x00\x01\x00\x00")
    for i, q in enumerate((lq, cq)):
        out += b"\xff\xdb\x00\x43" + bytes([i]) + bytes(int(v) for v in q[ZIGZAG])
    s = 0x22 if subsampling == "420" else 0x11
    out += b"\xff\xc0\x00\x11\x08" + height.to_bytes(2, "big") + width.to_bytes(2, "big") + bytes([3, 1, s, 0, 2, 0x11, 1, 3, 0x11, 1])
    for tc, (bits, vals) in ((0x00, DC_LUMA), (0x10, AC_LUMA), (0x01, DC_CHROMA), (0x11, AC_CHROMA)):
        out += b"\xff\xc4" + (19 + len(vals)).to_bytes(2, "big") + bytes([tc]) + bytes(bits) + bytes(vals)
    out += b"\xff\xdd\x00\x04" + restart_interval.to_bytes(2, "big")
    out += b"\xff\xda\x00\x0c\x03\x01\x00\x02\x11\x03\x11\x00\x3f\x00"
    return bytes(out)


class _Bits:
    def __init__(self):
        self.out, self.acc, self.n = bytearray(), 0, 0
        self.stuffed = 0

    def put(self, value, length):
        self.acc, self.n = (self.acc << length) | value, self.n + length
        while self.n >= 8:
            byte = (self.acc >> (self.n - 8)) & 0xFF
            self.out.append(byte)
            if byte == 0xFF:
                self.out.append(0)
                self.stuffed += 1
            self.n -= 8
        self.acc &= (1 << self.n) - 1

    def flush(self):
        if self.n:
            self.put((1 << (8 - self.n)) - 1, 8 - self.n)


def _amplitude(v):
    size = int(abs(v)).bit_length()
    return size, (v if v >= 0 else v + (1 << size) - 1)


def write(coefs, width, height, quality, subsampling, restart_interval=None):
    """The file of the given quantised coefficients ([Y, Cb, Cr] as transform returns them) -> (bytes, statistics)."""
    if restart_interval is None:
        restart_interval = default_restart(width, subsampling)
    blocks, comp, per_mcu = scan_order(coefs, subsampling)
    dc = [huffman_codes(DC_LUMA), huffman_codes(DC_CHROMA), huffman_codes(DC_CHROMA)]
    ac = [huffman_codes(AC_LUMA), huffman_codes(AC_CHROMA), huffman_codes(AC_CHROMA)]
    mcus = len(blocks) // per_mcu
    segments = -(-mcus // restart_interval)
    st = {"zrl": 0, "eob": 0, "dc_cat": 0, "ac_cat": 0, "zero_dc_diff": 0, "segments": segments, "stuffed": 0}
    out = bytearray(header(width, height, quality, subsampling, restart_interval))
    for s in range(segments):
        w, pred = _Bits(), [0, 0, 0]
        for b in range(s * restart_interval * per_mcu, min(mcus, (s + 1) * restart_interval) * per_mcu):
            c, z = comp[b], [int(v) for v in blocks[b]]
            size, amp = _amplitude(z[0] - pred[c])
            st["zero_dc_diff"] += z[0] == pred[c] and b >= per_mcu + s * restart_interval * per_mcu
            pred[c] = z[0]
            st["dc_cat"] = max(st["dc_cat"], size)
            w.put(*dc[c][size])
            w.put(amp, size)
            run = 0
            for k in range(1, 64):
                if z[k] == 0:
                    run += 1
                    continue
                while run >= 16:
                    w.put(*ac[c][0xF0])
                    st["zrl"] += 1
                    run -= 16
                size, amp = _amplitude(z[k])
                st["ac_cat"] = max(st["ac_cat"], size)
                w.put(*ac[c][(run << 4) | size])
                w.put(amp, size)
                run = 0
            if run:
                w.put(*ac[c][0])
                st["eob"] += 1
        w.flush()
        st["stuffed"] += w.stuffed
        out += w.out
        out += bytes([0xFF, 0xD0 + s % 8]) if s < segments - 1 else b"\xff\xd9"
    return bytes(out), st


def encode(img, quality=90, subsampling="420", restart_interval=None):
    coefs, _, _ = transform(img, quality, subsampling)
    return write(coefs, img.shape[1], img.shape[0], quality, subsampling, restart_interval)


def decode(coefs, width, height, quality, subsampling):
    """Quantised coefficients -> uint8 [H, W, 3]: dequantise, float IDCT, each component limited to 0..255, the
    chroma samples repeated 2x2, colour."""
    c = dct_matrix()
    lq, cq = scaled_tables(quality)
    comps = []
    for z, q in zip(coefs, (lq, cq, cq)):
        f = np.zeros(z.shape, np.float64)
        f[..., ZIGZAG] = z * q[ZIGZAG]
        f = f.reshape(z.shape[0], z.shape[1], 8, 8)
        p = np.einsum("vy,rcvu,ux->rcyx", c, f, c) + 128
        p = np.clip(np.rint(p), 0, 255)
        comps.append(p.transpose(0, 2, 1, 3).reshape(z.shape[0] * 8, z.shape[1] * 8))
    y, cb, cr = comps
    if subsampling == "420":
        cb, cr = (np.repeat(np.repeat(v, 2, 0), 2, 1) for v in (cb, cr))
    cb, cr = cb - 128, cr - 128
    rgb = np.stack([y + 1.402 * cr, y - 0.344136286 * cb - 0.714136286 * cr, y + 1.772 * cb], -1)
    return np.clip(np.rint(rgb), 0, 255).astype(np.uint8)[:height, :width]


def psnr(a, b):
    mse = np.mean((a.astype(np.float64) - b.astype(np.float64)) ** 2)
    return float("inf") if mse == 0 else 10 * np.log10(255.0 ** 2 / mse)
