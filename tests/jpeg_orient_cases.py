"""What tests/test_jpeg_orient.py and tools/jpeg_orient_rate.py share: JPEG files that carry an EXIF orientation, and the reference
for them.  The reference never comes from the GPU: a frame is Pillow's (libjpeg-turbo's) decode of the same bytes, permuted in numpy
by the orientation table of include/meterelf_hip.h; a record is the reader's on the frame the host decoder (imread_bgr) returns."""
import glob
import io
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))   # the tool imports this module from tools/, without the package
from oriented_cases import CODES, inverse, orient  # noqa: E402,F401  (the header's table, as tests/test_oriented.py checks it against Pillow)

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')


def unorient(O, code):
    """The stored frame whose oriented frame under `code` is O."""
    return orient(O, inverse(code))


def pillow_bgr(data):
    """Pillow's decode of the bytes AS STORED (Image.open applies no tag), BGR."""
    from PIL import Image
    with Image.open(io.BytesIO(data)) as im:
        rgb = np.asarray(im.convert('RGB'), dtype=np.uint8)
    return np.ascontiguousarray(rgb[:, :, ::-1])


def reference_frame(data, code):
    return np.ascontiguousarray(orient(pillow_bgr(data), code))


def encode(img, code=None, **kw):
    """img (H x W x 3 RGB, or H x W grey) as a JPEG file with the orientation tag `code` (None: no EXIF block at all)."""
    from PIL import Image
    buf = io.BytesIO()
    if code is not None:
        exif = Image.Exif()
        exif[0x0112] = code
        kw = dict(kw, exif=exif)
    Image.fromarray(img).save(buf, 'JPEG', **kw)
    return buf.getvalue()


def tiff_block(value, big_endian):
    """An EXIF TIFF block whose IFD0 holds the orientation tag alone, SHORT, count 1."""
    e = 'big' if big_endian else 'little'
    b = lambda v, n: int(v).to_bytes(n, e)   # noqa: E731
    return ((b'MM' if big_endian else b'II') + b(42, 2) + b(8, 4) + b(1, 2) + b(0x0112, 2) + b(3, 2) + b(1, 4) + b(value, 2) + b(0, 2)
            + b(0, 4))


def with_app1(data, tiff):
    """data (a JPEG file without APP1) with an Exif APP1 segment holding `tiff` right behind SOI."""
    app1 = b'\xff\xe1' + (len(tiff) + 8).to_bytes(2, 'big') + b'Exif\x00\x00' + tiff
    return data[:2] + app1 + data[2:]


def golden_files(sd='sample-images1'):
    return sorted(glob.glob(os.path.join(GOLDEN, sd, '*.jpg')))


_natural = {}


def natural(H, W):
    """Natural-looking content of any size: a crop of a golden camera frame (the meter's face, dials and print), resized.  RGB."""
    if (H, W) not in _natural:
        from PIL import Image
        with Image.open(golden_files()[3]) as im:
            im = im.convert('RGB')
            (w, h) = im.size
            crop = im.crop((w // 4, h // 4, w // 4 + w // 2, h // 4 + h // 2))
            _natural[(H, W)] = np.asarray(crop.resize((W, H), Image.BILINEAR), dtype=np.uint8).copy()
    return _natural[(H, W)]


def stored_under(path_or_frame, code, quality=95, **kw):
    """A file whose UPRIGHT frame is (up to the re-encoding) the given golden file's: the frame un-oriented in numpy and encoded with
    the tag.  Returns the bytes."""
    from PIL import Image
    if isinstance(path_or_frame, str):
        with Image.open(path_or_frame) as im:
            frame = np.asarray(im.convert('RGB'), dtype=np.uint8)
    else:
        frame = path_or_frame
    return encode(np.ascontiguousarray(unorient(frame, code or 1)), code, quality=quality, **kw)   # code None: upright, no EXIF block
