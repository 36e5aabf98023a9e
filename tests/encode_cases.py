"""Shared cases of the encoders from pixels (bu_rgba_encode_blocks): formats, shapes, images, and the expected blocks.

Expected bytes are the numpy models' (tests/colour_model.py, tests/channel_model.py -- written from the rules of DESIGN.md sections 4.4 / 4.5, pinned
by spec decoders elsewhere in the suite) applied to the image after replication padding to multiples of four and cut into blocks; nothing here
borrows the product's gather or its encoders."""
import functools

import numpy as np

import channel_model as cm
import colour_model as col

FORMATS = {"bc4": (6, 8), "bc5": (7, 16), "r11": (8, 8), "rg11": (9, 16), "bc1": (11, 8), "bc3": (12, 16)}  # name -> (bu_target, bytes per block)
OTHER_FORMATS = (0, 1, 2, 3, 4, 5, 10, 13, -1, 1 << 20)  # ASTC, BC7, ETC1, ETC2, RGBA32, the non-targets, outside the enumeration
# width x height -> what it exercises in the kernel
SHAPES = {
    (1, 1): "the smallest image: one block, fifteen replicated texels",
    (4, 4): "one whole block",
    (5, 3): "partial last column and row",
    (3, 5): "partial only column, partial last row",
    (255, 9): "lane 63 is the partial block, last block row partial",
    (257, 8): "65 blocks per row: waves straddle block rows",
    (12, 203): "three blocks per row: a wave spans 21 rows",
    (1024, 4): "one full block row of four waves",
}
KINDS = ("random", "gradient", "solid", "checker")


def blocks_of(w, h):
    return (w + 3) // 4, (h + 3) // 4


@functools.lru_cache(maxsize=None)
def image(kind, w, h, seed=0):
    """[h, w, 4] uint8, read-only.  random: seeded bytes; gradient: smooth R, G, B ramps with a random alpha; solid: one colour per 8 x 8 tile
    (every block solid, the colours seeded, 0 and 255 among them); checker: two colours per image in a 1-pixel checker, the pair changing every 16
    columns (BC1's degenerate paths: equal endpoints after quantisation, two-point covariance)"""
    rng = np.random.default_rng(1000 * seed + 7 * w + h + 31 * KINDS.index(kind))
    y, x = np.mgrid[0:h, 0:w]
    if kind == "random":
        img = rng.integers(0, 256, size=(h, w, 4), dtype=np.uint8)
    elif kind == "gradient":
        img = np.stack([(3 * x + y) % 256, (255 - x - 2 * y) % 256, (x * y // 7 + 5) % 256, rng.integers(0, 256, size=(h, w))], -1).astype(np.uint8)
    elif kind == "solid":
        pal = rng.integers(0, 256, size=(64, 4), dtype=np.uint8)
        pal[0], pal[1] = 0, 255
        img = pal[((y // 8) * 5 + x // 8) % 64]
    else:
        pal = rng.integers(0, 256, size=(16, 2, 4), dtype=np.uint8)
        pal[1] = [[16, 32, 16, 200], [17, 33, 17, 100]]  # a pair that quantises to equal 5/6/5 endpoints (2, 8, 2)
        img = pal[(x // 16) % 16, (x + y) % 2]
    img = np.ascontiguousarray(img, dtype=np.uint8)
    img.setflags(write=False)
    return img


def to_blocks(img):
    """[h, w, 4] -> [nby * nbx, 64]: the RGBA32 bytes of every block in raster order, the last column and row replicated into partial blocks"""
    h, w, _ = img.shape
    nbx, nby = blocks_of(w, h)
    p = np.pad(img, ((0, 4 * nby - h), (0, 4 * nbx - w), (0, 0)), mode="edge")
    return np.ascontiguousarray(p.reshape(nby, 4, nbx, 4, 4).transpose(0, 2, 1, 3, 4)).reshape(-1, 64)


def model(name, rgba_blocks):
    """[n, 64] texel bytes -> [n, block bytes] by the numpy models"""
    return (cm if name in cm.CHANNEL_TARGETS else col).encode(name, rgba_blocks)


@functools.lru_cache(maxsize=None)
def expected(name, kind, w, h, seed=0):
    """[nby, nbx, block bytes] uint8, read-only"""
    nbx, nby = blocks_of(w, h)
    out = np.ascontiguousarray(model(name, to_blocks(image(kind, w, h, seed)))).reshape(nby, nbx, FORMATS[name][1])
    out.setflags(write=False)
    return out


def image_bytes(w, h, pitch):
    """bytes of an image whose last row ends at its last pixel"""
    return (h - 1) * pitch + 4 * w


def pitched(img, pitch, pad_fill):
    """the image as the flat bytes the entry points read: rows `pitch` apart, the padding between them taken from pad_fill (uint8, at least
    image_bytes long)"""
    h, w, _ = img.shape
    n = image_bytes(w, h, pitch)
    buf = np.array(pad_fill[:n], dtype=np.uint8)
    rows = np.lib.stride_tricks.as_strided(buf, shape=(h, 4 * w), strides=(pitch, 1))
    rows[:] = img.reshape(h, 4 * w)
    return buf


def formula_image(w, h):
    """the image of tests/host_emul/bu_emul_encode_main.cpp: byte c of pixel (px, py) = (131 py + 31 px + 89 c + 7 (py ^ px)) & 255"""
    y, x, c = np.mgrid[0:h, 0:w, 0:4]
    return ((131 * y + 31 * x + 89 * c + 7 * (y ^ x)) & 255).astype(np.uint8)


def weighted_sum(values):
    """sum of (k + 1) * values[k] mod 2^64 (the checksum of bu_emul_encode_main.cpp)"""
    v = np.ascontiguousarray(values).reshape(-1).astype(np.uint64)
    return int((v * np.arange(1, v.size + 1, dtype=np.uint64)).sum(dtype=np.uint64))
