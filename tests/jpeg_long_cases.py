"""Files for the long-scan tests (melf_ctx_set_jpeg_long_scans): Pillow-encoded baseline files, what the host and the chapter kernel see
of their scans, and files whose clean scan length is steered into a window of a few bytes.  The plan's arithmetic is restated here from
meterelf_amd/csrc/melf_jpeg_long.h; tests/jpeg_long_main.cpp sweeps the header itself."""
import functools
import io

import numpy as np

T = 1024                          # segments of a chapter
MIN_DWORDS = 9
MAX_DWORDS = 999
PRODUCTION = T * 4 * MAX_DWORDS   # 4 091 904 bytes
MIN_CHAPTER = T * 4 * MIN_DWORDS  # 36 864 bytes
MAX_PAR_SCAN = 4000000            # what k_jpeg_huff addresses: longer restart-less scans are long with the switch in production


def seg_dwords(want):
    d = max(8, -(-want * 8 // (32 * T))) | 1
    return min(d, MAX_DWORDS)


def chapter_bytes(want):
    return T * 4 * seg_dwords(want)


def encode(img, **kw):
    from PIL import Image
    buf = io.BytesIO()
    Image.fromarray(img).save(buf, 'JPEG', **kw)
    return buf.getvalue()


def pillow_bgr(data, truncated=False):
    from PIL import Image, ImageFile
    old = ImageFile.LOAD_TRUNCATED_IMAGES
    ImageFile.LOAD_TRUNCATED_IMAGES = bool(truncated)
    try:
        with Image.open(io.BytesIO(data)) as im:
            rgb = np.asarray(im.convert('RGB'), dtype=np.uint8)
    finally:
        ImageFile.LOAD_TRUNCATED_IMAGES = old
    return np.ascontiguousarray(rgb[:, :, ::-1])


def scan_begin(data):
    """Offset of the first entropy-coded byte of a single-scan file (behind the SOS header)."""
    i = 2
    while True:
        assert data[i] == 0xFF, i
        (m, n) = (data[i + 1], (data[i + 2] << 8) | data[i + 3])
        if m == 0xDA:
            return i + 2 + n
        i += 2 + n


def scan_lengths(data):
    """(raw, clean) of a restart-less single-scan file that ends with EOI: the bytes from the scan's first to the file's last -- what the
    host compares with the chapter length -- and the entropy-coded bytes without stuffing, which the chapters count."""
    b = scan_begin(data)
    assert data[-2:] == b'\xff\xd9'
    body = data[b:-2]
    clean = body.replace(b'\xff\x00', b'\xff')
    assert b'\xff' not in body.replace(b'\xff\x00', b'')       # no marker, no fill byte inside
    return (len(data) - b, len(clean))


def chapters(data, k):
    """Chapters the kernel takes a file's scan in, with chapters of k bytes (k: what melf_ctx_get_jpeg_long_scans reports)."""
    return -(-scan_lengths(data)[1] // k)


def natural(rng, H, W):
    (yy, xx) = np.mgrid[0:H, 0:W]
    img = np.zeros((H, W, 3), np.float64)
    for c in range(3):
        img[..., c] = 128 + 100 * np.sin(xx / (7.0 + 5 * c) + rng.uniform(0, 6)) * np.cos(yy / (11.0 + 3 * c))
    for _ in range(6):
        (cy, cx, r) = (rng.integers(0, H), rng.integers(0, W), rng.integers(3, max(4, min(H, W) // 3)))
        img[(yy - cy) ** 2 + (xx - cx) ** 2 < r * r] = rng.integers(0, 256, 3)
    img += rng.normal(0, 6, img.shape)
    return np.clip(img, 0, 255).astype(np.uint8)


SHAPES = ((251, 333), (480, 640), (33, 1024))
SAMPLINGS = ('4:4:4', '4:2:2', '4:2:0', 'grey')


@functools.lru_cache(None)
def pool(shape):
    """[(name, bytes)]: noise and natural images of one shape in every sampling, qualities 75 to 100, Huffman-optimised and not."""
    (H, W) = shape
    rng = np.random.default_rng(H * 1000 + W)
    noise = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
    nat = natural(rng, H, W)
    out = []
    for s in SAMPLINGS:
        for (kind, img, q, opt) in (('noise', noise, 100, False), ('noise', noise, 90, False), ('natural', nat, 75, True),
                                    ('natural', nat, 95, False), ('natural', nat, 100, True)):
            kw = dict(quality=q, optimize=opt)
            if s == 'grey':
                data = encode(img[..., 1], **kw)
            else:
                data = encode(img, subsampling=s, **kw)
            out.append(('%s-%s-q%d%s' % (kind, s, q, '-opt' if opt else ''), data))
    return out


@functools.lru_cache(None)
def _steer_material(H, W):
    rng = np.random.default_rng(H * 7 + W)
    big = rng.integers(0, 256, (H, W), dtype=np.uint8)
    small = np.full((H, W), 128, np.uint8)
    small[:, 4::8] = 131          # a step inside every block: a few bytes a block
    small[:, 5::8] = 131
    small[:, 6::8] = 131
    small[:, 7::8] = 131
    return (big, small)


def _steered(H, W, nbig, nsmall):
    """A greyscale H x W file (multiples of 8) at quality 100: the first nbig blocks in raster order noise, the next nsmall a faint step,
    the rest flat."""
    (big, small) = _steer_material(H, W)
    bx = W // 8
    kind = np.zeros((H // 8) * bx, np.uint8)
    kind[:nbig] = 2
    kind[nbig:nbig + nsmall] = 1
    k = np.kron(kind.reshape(H // 8, bx), np.ones((8, 8), np.uint8))
    img = np.where(k == 2, big, np.where(k == 1, small, np.uint8(128))).astype(np.uint8)
    return encode(img, quality=100)


@functools.lru_cache(None)
def steered_file(lo, hi, W=1024):
    """A restart-less greyscale file whose CLEAN scan length lies in (lo, hi] (hi - lo >= 16): noise blocks up to just below the window, then
    faint blocks, a few bytes each, into it.  Returns (bytes, (H, W))."""
    H = (-(-hi // (70 * (W // 8))) + 2) * 8        # a noise block takes more than 70 bytes at quality 100
    total = (H // 8) * (W // 8)
    (a, b) = (0, total)                            # most noise blocks that stay at or below lo
    while a < b:
        m = (a + b + 1) // 2
        if scan_lengths(_steered(H, W, m, 0))[1] <= lo:
            a = m
        else:
            b = m - 1
    nbig = a
    assert nbig < total - 64, (lo, hi, H, W)
    (a, b) = (0, total - nbig)                     # fewest faint blocks that get above lo
    while a < b:
        m = (a + b) // 2
        if scan_lengths(_steered(H, W, nbig, m))[1] > lo:
            b = m
        else:
            a = m + 1
    data = _steered(H, W, nbig, a)
    n = scan_lengths(data)[1]
    assert lo < n <= hi, (lo, hi, n, nbig, a)
    return (data, (H, W))
