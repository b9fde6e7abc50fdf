"""What tests/test_jpeg_samplings.py and tools/jpeg_sampling_rate.py share: YCbCr 4:4:0 and 4:1:1 JPEG files (melf_ctx_set_jpeg_samplings)
written by tests/jpeg_writer.py, and the reference for them.  The reference never comes from the GPU: a frame is Pillow's
(libjpeg-turbo's) decode of the same bytes; `upsampled_frame` is the numpy restatement of include/meterelf_hip.h's two formulas on
libjpeg's own component planes, which a CPU test holds against Pillow."""
import glob
import io
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))   # the tool imports this module from tools/, without the package
import jpeg_writer as jw  # noqa: E402

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
LAYOUTS = ('440', '411')
# the sizes the formulas were checked on: whole and partial MCUs of both layouts, one pixel, one block, narrow and flat images
SIZES13 = [(48, 64), (37, 53), (16, 32), (9, 5), (1, 1), (17, 3), (2, 8), (38, 40), (22, 33), (10, 7), (6, 70), (4, 4), (30, 34)]
FLAT_Q = (4, 6)   # flat quantisation tables for re-encoded camera frames: every golden frame stays inside the writer's check_in_range


def q_ramp(step, base=2):
    (i, j) = np.mgrid[0:8, 0:8]
    return np.minimum(base + step * (i + j), 255).reshape(64).tolist()


QT = {0: (q_ramp(2), False), 1: (q_ramp(3, 3), False)}


def std_tables():
    std = jw.standard_tables()
    return ({0: std['dc'][0], 1: std['dc'][1]}, {0: std['ac'][0], 1: std['ac'][1]})


def pillow_bgr(data):
    from PIL import Image
    with Image.open(io.BytesIO(data)) as im:
        rgb = np.asarray(im.convert('RGB'), dtype=np.uint8)
    return np.ascontiguousarray(rgb[:, :, ::-1])


def natural(rng, H, W):
    """Smooth gradients, blobs and noise, RGB."""
    (yy, xx) = np.mgrid[0:H, 0:W]
    img = np.zeros((H, W, 3), np.float64)
    for c in range(3):
        img[..., c] = 128 + 100 * np.sin(xx / (7.0 + 5 * c) + rng.uniform(0, 6)) * np.cos(yy / (11.0 + 3 * c))
    for _ in range(6):
        (cy, cx, r) = (rng.integers(0, H), rng.integers(0, W), rng.integers(3, max(4, min(H, W) // 3)))
        img[(yy - cy) ** 2 + (xx - cx) ** 2 < r * r] = rng.integers(0, 256, 3)
    img += rng.normal(0, 6, img.shape)
    return np.clip(img, 0, 255).astype(np.uint8)


def image_coefs(img, sampling, qt=QT):
    nc = jw.SAMPLING[sampling][0]
    return jw.coefficients_from_image(img[..., 1] if nc == 1 else img, sampling, [qt[0][0], qt[1][0], qt[1][0]][:nc])


def write(coefs, size, sampling, qt=QT, **kw):
    """A baseline file of the grids with the Annex K tables, luma on tables 0 and chroma on tables 1 unless kw says otherwise."""
    (dc, ac) = std_tables()
    nc = len(coefs)
    dc = kw.pop('dc', {t: dc[t] for t in range(min(nc, 2))})
    ac = kw.pop('ac', {t: ac[t] for t in range(min(nc, 2))})
    return jw.write_jpeg(coefs, size, sampling, qt, dc, ac, **kw)


def natural_file(rng, size, sampling, **kw):
    return write(image_coefs(natural(rng, *size), sampling), size, sampling, **kw)


def component_planes(coefs, size, sampling, qt=QT):
    """libjpeg's own sample planes of a colour file's components: each component's REAL block grid written as a greyscale file of the
    component's size and decoded by Pillow (a greyscale decode is the IDCT and nothing else)."""
    from PIL import Image
    (H, W) = size
    (_nc, hs, vs) = jw.SAMPLING[sampling]
    planes = []
    for (c, grid) in enumerate(coefs):
        (h, w) = (H, W) if c == 0 else (-(-H // vs), -(-W // hs))
        (by, bx) = (-(-h // 8), -(-w // 8))
        t = 0 if c == 0 else 1
        data = write([np.ascontiguousarray(grid[:by, :bx])], (h, w), 'grey', {0: qt[t]})
        with Image.open(io.BytesIO(data)) as im:
            assert im.mode == 'L' and im.size == (w, h)
            planes.append(np.asarray(im, dtype=np.uint8).astype(np.int64))
    return planes


def upsample(P, size, sampling):
    """A chroma plane at the frame's size, by include/meterelf_hip.h's formulas."""
    (H, W) = size
    if sampling == '411':
        return P[:, np.arange(W) >> 2]
    assert sampling == '440'
    ch = P.shape[0]
    y = np.arange(H)
    cy = y >> 1
    far = np.where(y & 1, np.minimum(cy + 1, ch - 1), np.maximum(cy - 1, 0))
    return (3 * P[cy] + P[far] + (1 + (y & 1))[:, None]) >> 2


def ycc_to_bgr(Y, Cb, Cr):
    """libjpeg's 16-bit fixed-point colour tables, as k_jpeg.hip's ycc_to_bgr states them."""
    (cb, cr) = (Cb - 128, Cr - 128)
    r = Y + ((91881 * cr + 32768) >> 16)
    g = Y + ((-22554 * cb + 32768 - 46802 * cr) >> 16)
    b = Y + ((116130 * cb + 32768) >> 16)
    return np.clip(np.dstack([b, g, r]), 0, 255).astype(np.uint8)


def upsampled_frame(coefs, size, sampling, qt=QT):
    (Y, Cb, Cr) = component_planes(coefs, size, sampling, qt)
    return ycc_to_bgr(Y, upsample(Cb, size, sampling), upsample(Cr, size, sampling))


def golden_files(sd='sample-images1'):
    return sorted(glob.glob(os.path.join(GOLDEN, sd, '*.jpg')))


def fixture_frames(n, sd='sample-images1'):
    """(files, RGB frames) of n golden files of the set's commonest size, from the third on (sample-images1 begins with two frames
    whose dials are not found)."""
    from PIL import Image
    sizes = {}
    for f in golden_files(sd):
        with Image.open(f) as im:
            sizes[f] = im.size
    common = max(set(sizes.values()), key=list(sizes.values()).count)
    files = [f for f in golden_files(sd) if sizes[f] == common][2:2 + n]
    frames = []
    for f in files:
        with Image.open(f) as im:
            frames.append(np.asarray(im.convert('RGB'), dtype=np.uint8))
    return (files, frames)


def reencode(rgb, sampling):
    """A camera frame as a writer file of `sampling` with the flat tables FLAT_Q and the Annex K Huffman tables."""
    qt = {0: ([FLAT_Q[0]] * 64, False), 1: ([FLAT_Q[1]] * 64, False)}
    return write(image_coefs(rgb, sampling, qt), rgb.shape[:2], sampling, qt)


def dense_file(size, sampling, seed=1024):
    """A file whose scan is as long as its block count allows while every block stays inside the writer's range condition: DC 0
    and all 63 AC coefficients of magnitude 16..31 in every block (79 bytes a block with the Annex K tables), the grids tiled from
    8 x 8 random blocks per component.  Every field of such a scan has a fixed width -- the DC code of difference 0, then 63 times
    the code of run 0 / size 5 and five value bits -- so the scan is packed in numpy here, behind the header jpeg_writer writes for
    the same size (its entropy coder is a Python loop per symbol: two million symbols).  Returns (bytes, scan length)."""
    (nc, hs, vs) = jw.SAMPLING[sampling]
    assert nc == 3
    ((my, mx), shapes) = jw.grid_shape(size, sampling)
    rng = np.random.default_rng(seed)
    qt = {0: ([1] * 64, False), 1: ([1] * 64, False)}
    (dc, ac) = std_tables()
    tiles = []
    for _c in range(3):
        t = np.zeros((8, 8, 64), np.int16)
        t[..., jw.ZIGZAG[1:]] = rng.integers(16, 32, (8, 8, 63)) * rng.choice([-1, 1], (8, 8, 63))
        tiles.append(t)
    jw.check_in_range(tiles, qt, [(0, 0, 0), (1, 1, 1), (1, 1, 1)])
    grids = [np.tile(t, (-(-by // 8), -(-bx // 8), 1))[:by, :bx] for (t, (by, bx)) in zip(tiles, shapes)]
    head = write([np.zeros((by, bx, 64), np.int16) for (by, bx) in shapes], size, sampling, qt)
    sos = head.index(b'\xff\xda')
    head = head[:sos + 2 + ((head[sos + 2] << 8) | head[sos + 3])]

    def block_bits(grid, t):
        (dcode, dlen, _p) = jw.code_paths(dc[t], True)[0]
        (acode, alen, _p) = jw.code_paths(ac[t], False)[0x05]
        zz = grid.reshape(-1, 64)[:, jw.ZIGZAG[1:]].astype(np.int64)
        vb = np.where(zz >= 0, zz, zz + 31)
        field = np.empty((zz.shape[0], 63, alen + 5), np.uint8)
        field[:, :, :alen] = [(acode >> (alen - 1 - k)) & 1 for k in range(alen)]
        field[:, :, alen:] = (vb[:, :, None] >> np.arange(4, -1, -1)) & 1
        first = np.empty((zz.shape[0], dlen), np.uint8)
        first[:] = [(dcode >> (dlen - 1 - k)) & 1 for k in range(dlen)]
        return np.concatenate([first, field.reshape(zz.shape[0], -1)], axis=1)
    luma = block_bits(grids[0], 0).reshape(my, vs, mx, hs, -1).transpose(0, 2, 1, 3, 4).reshape(my * mx, -1)
    bits = np.concatenate([luma, block_bits(grids[1], 1), block_bits(grids[2], 1)], axis=1).reshape(-1)
    bits = np.concatenate([bits, np.ones(-len(bits) % 8, np.uint8)])
    body = np.packbits(bits)
    body = np.insert(body, np.flatnonzero(body == 255) + 1, 0)
    return (head + body.tobytes() + b'\xff\xd9', len(body))
