"""Inputs of the colour Lucas-Kanade tests (tests/test_lk_bgr_cpu.py, tests/test_lk_bgr_gpu.py): 8UC3 images (H, W, 3), B, G, R
interleaved.  Colour textures are three smooth canvases of tests/lk_cases.py with different seeds - uncorrelated channels -
moved by one planted shift.  The positions of the oscillation, the 30-iteration and the gray-against-colour points were found
by running the restatement (tests/lk_ref.py) on the CPU over candidate points, then fixed here."""
import struct
import zlib

import numpy as np

import lk_cases


def gray_of(bgr):
    """cv::cvtColor(COLOR_BGR2GRAY) for 8U: (1868 B + 9617 G + 4899 R + 8192) >> 14."""
    a = np.asarray(bgr).astype(np.int64)
    return ((a[..., 0] * 1868 + a[..., 1] * 9617 + a[..., 2] * 4899 + 8192) >> 14).astype(np.uint8)


def replicate(gray):
    """B = G = R."""
    return np.ascontiguousarray(np.repeat(np.asarray(gray, np.uint8)[..., None], 3, axis=-1))


def colour_pair(seeds, W, H, shift):
    """(prev, next): one smooth canvas per channel, all moved by `shift`."""
    cs = [lk_cases.smooth_canvas(s, W, H) for s in seeds]
    prev = np.stack([lk_cases.resample(c, W, H, 0.0, 0.0) for c in cs], axis=2)
    nxt = np.stack([lk_cases.resample(c, W, H, shift[0], shift[1]) for c in cs], axis=2)
    return np.ascontiguousarray(prev), np.ascontiguousarray(nxt)


def colour_noise(seed, W, H):
    return np.random.default_rng(seed).integers(0, 256, (H, W, 3), dtype=np.uint8)


def padded(img, pad):
    """(buffer, stride): the image with `pad` bytes of 0xA5 after every row."""
    H, W = img.shape[:2]
    buf = np.full((H, 3 * W + pad), 0xA5, np.uint8)
    buf[:, :3 * W] = img.reshape(H, 3 * W)
    return buf, 3 * W + pad


# ---- the isoluminant pair -------------------------------------------------------------------------------------------------------
ISO_SIZE = (200, 180)
ISO_SHIFT = (1.5, 2.25)


def _green_for_gray(b, r, target=128):
    """Per pixel the smallest G in 0..255 that makes the fixed-point gray of (B, G, R) equal `target` (one unit of G moves the
    gray by 0 or 1, so while B and R stay moderate one exists); asserted."""
    b = b.astype(np.int64)[..., None]; r = r.astype(np.int64)[..., None]
    g = np.arange(256, dtype=np.int64)
    hit = ((1868 * b + 9617 * g + 4899 * r + 8192) >> 14) == target
    assert hit.any(axis=-1).all(), "no G gives the target gray: B and R are not moderate"
    return hit.argmax(axis=-1).astype(np.uint8)


def isoluminant_pair():
    """200 x 180, shift (1.5, 2.25): B and R are smooth canvases of 40% amplitude around mid-range, G makes COLOR_BGR2GRAY 128
    at every pixel of both images.  To a gray tracker both images are constant; the colour one sees B, G and R move."""
    W, H = ISO_SIZE
    out = []
    cb = (lk_cases.smooth_canvas(51, W, H) - 127.5) * 0.4 + 128.0
    cr = (lk_cases.smooth_canvas(52, W, H) - 127.5) * 0.4 + 128.0
    for dx, dy in ((0.0, 0.0), ISO_SHIFT):
        b, r = lk_cases.resample(cb, W, H, dx, dy), lk_cases.resample(cr, W, H, dx, dy)
        img = np.ascontiguousarray(np.stack([b, _green_for_gray(b, r), r], axis=2))
        assert np.all(gray_of(img) == 128)
        out.append(img)
    return out[0], out[1]


# ---- the exits ------------------------------------------------------------------------------------------------------------------
def exits_pair():
    """lk_cases.exits_pair() in colour, 185 x 177: three textures moved 12 px to the right, the 60 x 60 patch at (60, 50)
    constant in every channel of both images, the 50 x 50 block at (10, 120) unrelated colour noise in the two images."""
    W, H = lk_cases.EXITS_SIZE
    p, n = colour_pair((11, 12, 13), W, H, (12.0, 0.0))
    p[50:110, 60:120] = (90, 140, 60); n[50:110, 60:120] = (90, 140, 60)
    p[120:170, 10:60] = colour_noise(100, 50, 50); n[120:170, 10:60] = colour_noise(101, 50, 50)
    return p, n


EXITS_N = 150                      # lk_cases.exits_points(150): the three special points, 40 integer, 40 with ties, 67 others


def exits_points():
    return lk_cases.exits_points(EXITS_N)


def low_contrast_pair():
    """120 x 100, 16 levels of smooth texture per channel moved by (0.4, 0.3)."""
    cs = [lk_cases.smooth_canvas(s, 120, 100) * (16.0 / 255.0) + 100 for s in (30, 31, 32)]
    prev = np.stack([lk_cases.resample(c, 120, 100, 0.0, 0.0) for c in cs], axis=2)
    nxt = np.stack([lk_cases.resample(c, 120, 100, 0.4, 0.3) for c in cs], axis=2)
    return np.ascontiguousarray(prev), np.ascontiguousarray(nxt)


OSCILLATION_POINT = (36.0, 36.0)   # in low_contrast_pair(): ends by the oscillation rule at level 0 after 3 iterations


def wander_pair():
    """Two unrelated 40 x 40 colour noise images: one level, no correspondence."""
    return colour_noise(100, 40, 40), colour_noise(101, 40, 40)


MAX_COUNT_POINT = (8.0, 4.0)           # in wander_pair(): all 30 iterations at level 0, status stays 1


# ---- one point, two statuses -----------------------------------------------------------------------------------------------------
def faint_pair():
    """64 x 64, a few gray levels of smooth texture moved by (0.3, 0.2), levels 0 and 1.  Tracked as gray and as B = G = R colour:
    the colour sums are three times the gray ones against the same divisor 882."""
    c = lk_cases.smooth_canvas(60, 64, 64) * (FAINT_LEVELS / 255.0) + 100
    return lk_cases.resample(c, 64, 64, 0.0, 0.0), lk_cases.resample(c, 64, 64, 0.3, 0.2)


FAINT_LEVELS = 6.0
SPLIT_POINT = (16.0, 12.0)         # in faint_pair(): minEig below 1e-4 as gray (status 0), above it as B = G = R (status 1)


# ---- files ----------------------------------------------------------------------------------------------------------------------
def write_ppm(path, bgr):
    """Binary P6: the file holds R, G, B."""
    with open(path, "wb") as f:
        f.write(b"P6\n%d %d\n255\n" % (bgr.shape[1], bgr.shape[0]))
        f.write(np.ascontiguousarray(bgr[..., ::-1], np.uint8).tobytes())


def write_png(path, bgr):
    """8-bit RGB PNG, filter 0 on every row, standard library only."""
    rgb = np.ascontiguousarray(bgr[..., ::-1], np.uint8)
    H, W = rgb.shape[:2]
    raw = b"".join(b"\x00" + rgb[y].tobytes() for y in range(H))

    def chunk(tag, data):
        return struct.pack(">I", len(data)) + tag + data + struct.pack(">I", zlib.crc32(tag + data) & 0xffffffff)
    with open(path, "wb") as f:
        f.write(b"\x89PNG\r\n\x1a\n" + chunk(b"IHDR", struct.pack(">IIBBBBB", W, H, 8, 2, 0, 0, 0)) +
                chunk(b"IDAT", zlib.compress(raw, 1)) + chunk(b"IEND", b""))
