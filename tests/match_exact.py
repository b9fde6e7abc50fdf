"""An exact reference of cv2.matchTemplate(L, T, TM_CCOEFF) + cv2.minMaxLoc, written out as the definition, and the batches
that drive the match kernels through cc in [2^31, 2^32).

numpy only; no code shared with oracle/melf_oracle.c or with the library.  The cross-correlation and the window sums are int64,
so they are exact for any u8 template, however large; the post-pass is OpenCV's own (two float64 operations, then float32).

Every template whose product sum th * tw * 255^2 fits 32 UNSIGNED bits is admitted by the match kernels, and the VALU kernel's
64 KiB LDS tile lets a context have templates of up to about 40 000 pixels -- 209 x 190, 159 x 256, 291 x 128 (th x tw) -- whose
cc reaches 2.6e9 on bright frames.  limit_cases builds bright batches for such templates; what each frame is for is returned with
the batch, and tests/test_match_limits.py shows by this reference alone that the frames hold what they claim.
"""
import numpy as np

TWO31 = 1 << 31
TWO32 = 1 << 32

# (th, tw, rows, cols): the largest templates a context accepts, in crops whose maps exercise ...
LIMIT_SHAPES = {
    't209x190_i231x250': (209, 190, 231, 250),   # ... the tuned kernel's two column blocks (map 23 x 61),
    't209x190_i231x215': (209, 190, 231, 215),   # its single column block (map 23 x 26),
    't159x256_i175x288': (159, 256, 175, 288),   # the general kernel's column block + one V-form column, K slices (map 17 x 33),
    't291x128_i300x161': (291, 128, 300, 161),   # and five Toeplitz blocks per template row with two V-form columns (map 10 x 34)
}
VARIANTS = ('bright', 'extreme')
N_LIMIT = 40          # two 32-frame groups
ROLE_NAMES = ('a', 'b', 'c', 'd', 'e', 'f')
PASTE_XY = (3, 5)     # frame (d): where the template occurs, (x, y)


def exact_match(imgs, tpl):
    """imgs (n, rows, cols) u8, tpl (th, tw) u8 -> (cc int64 (n, rh, rw), ws int64, map float32, [(max value, x, y)] per frame:
    the first maximum in raster order)."""
    imgs = np.asarray(imgs)
    tpl = np.asarray(tpl)
    assert imgs.dtype == np.uint8 and tpl.dtype == np.uint8 and imgs.ndim == 3 and tpl.ndim == 2
    (n, rows, cols) = imgs.shape
    (th, tw) = tpl.shape
    (rh, rw) = (rows - th + 1, cols - tw + 1)
    assert rh >= 1 and rw >= 1
    I = imgs.astype(np.int64)
    T = tpl.astype(np.int64)
    # cc[y, x] = sum_ij T[i, j] * I[y + i, x + j]
    cc = np.zeros((n, rh, rw), np.int64)
    tmp = np.empty_like(cc)
    for i in range(th):
        for j in range(tw):
            np.multiply(I[:, i:i + rh, j:j + rw], T[i, j], out=tmp)
            cc += tmp
    # ws[y, x] = sum_ij I[y + i, x + j], from an integral image
    S = np.zeros((n, rows + 1, cols + 1), np.int64)
    S[:, 1:, 1:] = I.cumsum(axis=1).cumsum(axis=2)
    ws = S[:, th:, tw:] - S[:, :rh, tw:] - S[:, th:, :rw] + S[:, :rh, :rw]
    # OpenCV's post-pass: mean(T) in cv::mean's reciprocal form, then num = double(cc) - double(ws) * mean as two operations
    tmean = np.float64(T.sum()) * (np.float64(1.0) / (np.float64(th) * np.float64(tw)))
    prod = ws.astype(np.float64) * tmean
    num = cc.astype(np.float64) - prod
    rmap = num.astype(np.float32)
    firsts = []
    for k in range(n):
        idx = int(np.argmax(rmap[k].ravel()))     # the first of equal maxima
        firsts.append((float(rmap[k].ravel()[idx]), idx % rw, idx // rw))
    return cc, ws, rmap, firsts


def limit_template(th, tw, seed, variant='bright'):
    """'bright': random 236..255.  'extreme': 0 or 255 (4 % / 96 %): the extremes of the matrix-core kernels' T - 128 in int8."""
    rng = np.random.default_rng([seed, th, tw, VARIANTS.index(variant)])
    if variant == 'bright':
        return rng.integers(236, 256, size=(th, tw), dtype=np.uint8)
    return rng.choice(np.array([0, 255], np.uint8), size=(th, tw), p=[0.04, 0.96])


def limit_cases(th, tw, rows, cols, n, seed, variant='bright'):
    """-> (tpl, imgs (n, rows, cols) u8, roles): roles[name] = the batch indices of frame `name`, one in each 32-frame group
    (frames are the N dimension of the matrix instructions and the lanes of a group).
      a  bright random 236..255: every cc >= 2^31
      b  all 255: the largest window sums and the largest cc; every map value ties
      c  a brightness ramp along the columns (+-8 noise), centred so that cc crosses 2^31 in the middle of the map
      d  random (0..255, darker for small maps) with an exact occurrence of the template at PASTE_XY: the first maximum is known,
         cc on both sides of 2^31
      e  a 5 x 7 block of random 225..255 tiled over the frame: the map repeats, so the maximum occurs many times with equal value
      f  random 0..255: every cc < 2^31, in the same frame group as the others
    Every other frame is bright random like (a)."""
    assert n >= 38 and rows >= th + PASTE_XY[1] and cols >= tw + PASTE_XY[0]
    tpl = limit_template(th, tw, seed, variant)
    rng = np.random.default_rng([seed, th, tw, rows, cols, VARIANTS.index(variant)])
    imgs = rng.integers(236, 256, size=(n, rows, cols), dtype=np.uint8)
    special = {}
    special['a'] = rng.integers(236, 256, size=(rows, cols), dtype=np.uint8)
    special['b'] = np.full((rows, cols), 255, np.uint8)
    # (c): a window's mean brightness at which cc = 2^31 is 2^31 / sum T; the ramp passes through it at the middle map column
    # (window centre x = (rw - 1) / 2 + (tw - 1) / 2) and rises by 40 over the frame, as 200 + 40 x / (cols - 1) does at 209 x 190 in
    # 231 x 250
    rw = cols - tw + 1
    level = TWO31 / float(tpl.astype(np.int64).sum())
    xc = (rw - 1) / 2.0 + (tw - 1) / 2.0
    ramp = level + 40.0 * (np.arange(cols) - xc) / (cols - 1)
    noisy = np.rint(ramp)[None, :].astype(np.int64) + rng.integers(-8, 9, size=(rows, cols))
    special['c'] = np.clip(noisy, 0, 255).astype(np.uint8)
    # (d): where the map is small against the template, every window lies mostly on the pasted (bright) occurrence and a 0..255
    # background leaves every cc above 2^31: the background is then darkened (0..127, 0..63, ...) until the window farthest from the
    # occurrence, the last map position, has cc clearly below 2^31
    noise = rng.integers(0, 256, size=(rows, cols), dtype=np.uint8)
    (px, py) = PASTE_XY
    (fy, fx) = (rows - th, cols - tw)
    for shift in range(9):
        d = noise >> shift
        d[py:py + th, px:px + tw] = tpl
        if int((tpl.astype(np.int64) * d[fy:fy + th, fx:fx + tw]).sum()) < 0.98 * TWO31:
            break
    special['d'] = d
    block = rng.integers(225, 256, size=(5, 7), dtype=np.uint8)
    special['e'] = np.tile(block, ((rows + 4) // 5, (cols + 6) // 7))[:rows, :cols]
    special['f'] = rng.integers(0, 256, size=(rows, cols), dtype=np.uint8)
    roles = {}
    for (k, name) in enumerate(ROLE_NAMES):
        roles[name] = (k, 32 + k)
        imgs[k] = special[name]
        imgs[32 + k] = special[name]
    return tpl, imgs, roles


_cache = {}


def limit_reference(shape_id, variant):
    """The batch of LIMIT_SHAPES[shape_id] and its exact reference, computed once per process and never modified:
    dict(tpl, imgs, roles, cc, ws, map, firsts)."""
    key = (shape_id, variant)
    if key not in _cache:
        (th, tw, rows, cols) = LIMIT_SHAPES[shape_id]
        (tpl, imgs, roles) = limit_cases(th, tw, rows, cols, N_LIMIT, 2031, variant)
        (cc, ws, rmap, firsts) = exact_match(imgs, tpl)
        for a in (tpl, imgs, cc, ws, rmap):
            a.setflags(write=False)
        _cache[key] = dict(tpl=tpl, imgs=imgs, roles=roles, cc=cc, ws=ws, map=rmap, firsts=firsts)
    return _cache[key]
