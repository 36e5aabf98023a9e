"""Shared cases of the encoder from pixels to UASTC (bu_rgba_encode_uastc): images, shapes and the model's answer for each,
computed once per process and shared by the CPU and the GPU tests.

An image is a variant of an encode_cases.image kind:
  plain    the kind as it is (random alpha, mostly: the RGBA modes 14, 12, 10; solid tiles: mode 8)
  opaque   A := 255 (modes 5, 0, 18)
  grey     G := R, B := R (mode 15)
  ag       A := G (alpha correlated with colour)
Every shape of the list carries at least one image; the whole list is about 2800 blocks.

Beside the images: EDGE_FAMILIES, 64 blocks each that are built to sit on one arithmetic edge of the rule (edge_sorted, as a strip four pixels high),
the same blocks in an order that puts all four block classes into every wave (edge_mixed), and a 64 x 64 pattern that mixes the classes
(mixed_pattern)."""
import functools

import numpy as np

import encode_cases as ec
import uastc_encode_model as um
from basisu_rs_amd import synth

SHAPES = ((1, 1), (5, 3), (255, 9), (257, 8), (12, 203), (64, 64))
VARIANTS = ("plain", "opaque", "grey", "ag")
CASES = ([("plain", k, w, h) for k in ec.KINDS for (w, h) in ((1, 1), (5, 3), (255, 9))]
         + [("opaque", k, w, h) for k in ("random", "gradient", "checker") for (w, h) in ((257, 8), (64, 64))]
         + [("opaque", "solid", 5, 3)]
         + [("grey", k, 12, 203) for k in ec.KINDS]
         + [("ag", "gradient", 64, 64)])
assert {(w, h) for _, _, w, h in CASES} == set(SHAPES)


def case_id(c):
    return "%s-%s-%dx%d" % c


@functools.lru_cache(maxsize=None)
def image(variant, kind, w, h):
    """[h, w, 4] uint8, read-only"""
    img = np.array(ec.image(kind, w, h))
    if variant == "opaque":
        img[..., 3] = 255
    elif variant == "grey":
        img[..., 1] = img[..., 0]
        img[..., 2] = img[..., 0]
    elif variant == "ag":
        img[..., 3] = img[..., 1]
    else:
        assert variant == "plain"
    img.setflags(write=False)
    return img


@functools.lru_cache(maxsize=None)
def fields(variant, kind, w, h):
    """uastc_encode_model.encode_fields of the image's blocks (raster order), every array read-only"""
    f = um.encode_fields(ec.to_blocks(image(variant, kind, w, h)))
    for v in f.values():
        v.setflags(write=False)
    return f


def expected(variant, kind, w, h):
    """[nby, nbx, 16] uint8"""
    nbx, nby = ec.blocks_of(w, h)
    return fields(variant, kind, w, h)["blocks"].reshape(nby, nbx, 16)


def formula_image(w, h):
    """the image of tests/host_emul/bu_emul_uastc_encode_main.cpp: encode_cases.formula_image with its alpha forced to 255 in the 8 x 8 tiles whose
    (px / 8 + py / 8) is odd and a single colour in the tiles where it is a multiple of five, so that opaque, alpha and solid blocks all occur"""
    img = np.array(ec.formula_image(w, h))
    y, x = np.mgrid[0:h, 0:w]
    t = x // 8 + y // 8
    img[..., 3] = np.where(t % 2 == 1, 255, img[..., 3])
    flat = (t % 5 == 0)
    img[flat] = np.stack([(t * 37) & 255, (t * 11) & 255, (t * 73) & 255, (t * 5) & 255], -1).astype(np.uint8)[flat]
    return img


# ---- blocks on the edges of the rule -------------------------------------------------------------------------------------------------------------
def _rand(rng, lo, hi, *shape):
    return rng.integers(lo, hi + 1, size=shape).astype(np.int64)


def _opaque(b):
    b = b.copy()
    b[:, :, 3] = 255
    return b


def _two_level(rng):
    return 255 * _rand(rng, 0, 1, 64, 16, 4)


def _tiny(rng):
    return _rand(rng, 0, 254, 64, 1, 4) + _rand(rng, 0, 1, 64, 16, 4)


def _one_channel(c):
    def gen(rng):
        b = np.repeat(_rand(rng, 0, 255, 64, 1, 4), 16, 1)
        b[:, :, c] = _rand(rng, 0, 255, 64, 16)
        if c < 3:
            b[0::2, :, 3] = 255
        return b
    return gen


def _anti(rng):
    r = _rand(rng, 0, 255, 64, 16)
    return np.stack([r, 255 - r, r // 2, 255 - r], -1)


def _outlier(rng):
    base, mask, at = _rand(rng, 1, 254, 64, 4), _rand(rng, 0, 1, 64, 4) == 1, _rand(rng, 0, 15, 64)
    mask[~mask.any(1), 1] = True
    base[0::3, 3], mask[0::3, 3] = 255, False  # every third block opaque: its outlier differs in R, G, B only
    mask[0::3, 1] |= ~mask[0::3, :3].any(1)
    kind = np.arange(64) % 4  # + 1, - 1, + 255, - 255
    base = np.where(mask & (kind == 2)[:, None], 0, np.where(mask & (kind == 3)[:, None], 255, base))
    b = np.repeat(base[:, None, :], 16, 1)
    b[np.arange(64), at] += mask * np.array([1, -1, 255, -255])[kind][:, None]
    return b


def _near_opaque(rng):
    b = _opaque(_rand(rng, 0, 255, 64, 16, 4))
    b[np.arange(64), _rand(rng, 0, 15, 64), 3] = np.where(np.arange(64) % 2 == 0, 254, 0)
    return b


def _near_grey(rng):
    g = _rand(rng, 0, 255, 64, 16)
    b = np.stack([g, g, g, _rand(rng, 0, 255, 64, 16)], -1)
    b[np.arange(64), _rand(rng, 0, 15, 64), 1] ^= 1
    return b


def _grey_a(anti):
    def gen(rng):
        g = _rand(rng, 0, 255, 64, 16)
        return np.stack([g, g, g, 255 - g if anti else g], -1)
    return gen


def _ramp_sat(rng):
    start, step, down = _rand(rng, 128, 255, 64, 1, 4), _rand(rng, 8, 40, 64, 1, 4), _rand(rng, 0, 1, 64, 1, 4) == 1
    v = np.minimum(255, start + step * np.arange(16)[None, :, None])
    b = np.where(down, 255 - v, v)
    b[0::2, :, 3] = 255
    return b


def _three_colour(rng):
    return np.array([[255, 0, 0, 255], [0, 255, 0, 255], [0, 0, 255, 255]])[_rand(rng, 0, 2, 64, 16)]


def _four_sym(rng):
    return 255 * np.eye(4, dtype=np.int64)[_rand(rng, 0, 3, 64, 16)]


def _halves(rng):
    c0, far, step = _rand(rng, 0, 255, 64, 3), _rand(rng, 0, 255, 64, 3), _rand(rng, -48, 48, 64, 3)
    kind = np.arange(64) % 4  # left / right, top / bottom, and the same two with a small step between the halves
    c1 = np.where((kind >= 2)[:, None], np.clip(c0 + step, 0, 255), far)
    i = np.arange(16)
    second = np.where((kind % 2 == 0)[:, None], (i % 4 >= 2)[None], (i >= 8)[None])  # [64, 16]
    b = np.full((64, 16, 4), 255, dtype=np.int64)
    b[:, :, :3] = np.where(second[:, :, None], c1[:, None, :], c0[:, None, :])
    return b


def _solid_extremes(rng):
    v = np.array([0, 7, 8, 247, 248, 255])
    rgb = [(0, 0, 0), (255, 255, 255), (255, 0, 0), (0, 255, 0), (0, 0, 255), (7, 7, 7), (8, 8, 8), (247, 247, 247), (248, 248, 248)]
    rgb = np.concatenate([np.array(rgb), v[_rand(rng, 0, 5, 64 - len(rgb), 3)]])
    c = np.concatenate([rgb, np.array([0, 1, 254, 255])[np.arange(64) % 4][:, None]], 1)
    return np.repeat(c[:, None, :], 16, 1)


def _two_colour(rng):
    pair = _rand(rng, 0, 255, 64, 2, 4)
    pair[0::2, :, 3] = 255
    pick = _rand(rng, 0, 1, 64, 16)
    pick[:, 0], pick[:, 15] = 0, 1  # (both colours occur)
    return pair[np.arange(64)[:, None], pick]


def _level_tripod(rng):
    base = um.LEVELS[11][_rand(rng, 1, 30, 64, 3)]
    b = np.repeat(np.concatenate([base, np.full((64, 1), 255)], 1)[:, None, :], 16, 1)
    at = np.argsort(rng.random((64, 16)), 1)[:, :3]  # three different texels
    b[np.arange(64)[:, None], at, :3] += np.array([[1, 1, 1], [1, -1, -1], [-1, 1, -1]])[None] * (2 * _rand(rng, 0, 1, 64, 1, 3) - 1)
    return b


# name -> (generator of [64, 16, 4] blocks from a seeded rng, what the family is there for)
EDGE_FAMILIES = {
    "two_level": (_two_level, "every channel 0 or 255: the largest covariance, csh > 0, least-squares numerators clamped at 0 and results saturated at 255"),
    "two_level_opaque": (lambda rng: _opaque(_two_level(rng)), "the same with A := 255, through modes 5 / 0 / 18"),
    "tiny": (_tiny, "a base colour + {0, 1} per channel: csh == 0, equal quantised endpoints and det >> t == 0, ties between modes"),
    "tiny_opaque": (lambda rng: _opaque(_tiny(rng)), "the same with A := 255"),
    "one_channel_0": (_one_channel(0), "a constant colour but for R (every other block opaque): a rank-one covariance on that axis, constant decoded alpha"),
    "one_channel_1": (_one_channel(1), "the same for G"),
    "one_channel_2": (_one_channel(2), "the same for B"),
    "one_channel_3": (_one_channel(3), "the same for A: the whole fit runs along alpha"),
    "anti": (_anti, "(r, 255 - r, r / 2, 255 - r): negative covariances through the arithmetic shifts"),
    "anti_opaque": (lambda rng: _opaque(_anti(rng)), "the same with A := 255"),
    "outlier": (_outlier, "15 equal texels and one that differs by +-1 or +-255 in some channels: two-colour blocks, which must be exact"),
    "near_opaque": (_near_opaque, "A = 255 but for one texel (254 or 0): the class boundary, must not take modes 5 / 0 / 18"),
    "near_grey": (_near_grey, "R = G = B but for one texel with G ^= 1: the class boundary, must not take mode 15"),
    "grey_a_eq": (_grey_a(False), "(g, g, g, g): mode 15 with fully correlated channels"),
    "grey_a_anti": (_grey_a(True), "(g, g, g, 255 - g): mode 15 with fully anti-correlated channels"),
    "ramp_sat": (_ramp_sat, "ramps that run into 255 or 0 (every other block opaque): min(255, ...) of the least-squares step"),
    "three_colour": (_three_colour, "pure red, green and blue texels: a symmetric covariance, ties for the largest diagonal entry"),
    "four_sym": (_four_sym, "the four unit axes of RGBA: the same with four channels"),
    "dark": (lambda rng: _rand(rng, 0, 3, 64, 16, 4), "values 0..3: ETC1 / EAC modifiers clamped at 0, searches that end on all-zero hints"),
    "bright": (lambda rng: _rand(rng, 252, 255, 64, 16, 4), "values 252..255: the modifiers clamped at 255"),
    "bright_opaque": (lambda rng: _opaque(_rand(rng, 252, 255, 64, 16, 4)), "the same with A := 255"),
    "halves": (_halves, "opaque left / right and top / bottom halves, far apart and a small step apart: the differential clamp (-4..3) of the ETC1 bases, both flips"),
    "solid_extremes": (_solid_extremes, "solid blocks of 0, 255, pure axes and 5-bit boundaries (7, 8, 247, 248), A in {0, 1, 254, 255}: mode 8's ETC1 fields at the clamps"),
    "level_tripod": (_level_tripod, "opaque, a colour on the levels of range 11 and three texels one step off it in directions that span RGB: where mode 18 "
                                    "wins, both its endpoints are the same level and det >> t == 0"),
    "two_colour": (_two_colour, "two arbitrary colours in a random assignment (every other block opaque): must be exact"),
}


@functools.lru_cache(maxsize=None)
def edge_blocks(name):
    """[64, 16, 4] uint8, read-only"""
    b = EDGE_FAMILIES[name][0](np.random.default_rng(4110 + list(EDGE_FAMILIES).index(name)))
    assert b.shape == (64, 16, 4) and b.min() >= 0 and b.max() <= 255
    b = b.astype(np.uint8)
    b.setflags(write=False)
    return b


@functools.lru_cache(maxsize=None)
def edge_fields(name):
    """uastc_encode_model.encode_fields of the family's blocks, every array read-only"""
    f = um.encode_fields(edge_blocks(name).reshape(64, 64))
    for v in f.values():
        v.setflags(write=False)
    return f


def strip(blocks):
    """[n, 16, 4] -> the image [4, 4 n, 4] whose block i is blocks[i]: the block order is the kernel's linear order, 64 consecutive blocks are one wave"""
    n = blocks.shape[0]
    return np.ascontiguousarray(blocks.reshape(n, 4, 4, 4).transpose(1, 0, 2, 3)).reshape(4, 4 * n, 4)


def block_class(blocks):
    """[n, 16, 4] -> [n]: 0 solid, 1 opaque, 2 grey with alpha, 3 RGBA -- from the texels alone"""
    b = np.asarray(blocks).reshape(-1, 16, 4)
    solid = (b == b[:, :1]).all((1, 2))
    opaque = (b[:, :, 3] == 255).all(1)
    grey = ((b[:, :, 0] == b[:, :, 1]) & (b[:, :, 0] == b[:, :, 2])).all(1)
    return np.where(solid, 0, np.where(opaque, 1, np.where(grey, 2, 3)))


CLASS_MODES = ((8,), (5, 0, 18), (15,), (14, 12, 10))  # by block_class


def class_rule_violations(src, blocks):
    """the indices of the blocks [n, 16] whose mode -- read out of their bytes, no model involved -- is none of the modes of the class that their
    texels src [n, 16, 4] are in"""
    modes, cls = synth.block_modes(np.asarray(blocks).reshape(-1, 16)), block_class(src)
    return np.nonzero(~np.array([int(m) in CLASS_MODES[c] for m, c in zip(modes, cls)], dtype=bool))[0]


@functools.lru_cache(maxsize=None)
def edge_sorted():
    """(blocks [n, 16, 4], expected [n, 16]): all families one after another, read-only"""
    b = np.concatenate([edge_blocks(name) for name in EDGE_FAMILIES])
    e = np.concatenate([edge_fields(name)["blocks"] for name in EDGE_FAMILIES])
    b.setflags(write=False)
    e.setflags(write=False)
    return b, e


def edge_field(key):
    """one array of edge_fields over edge_sorted's blocks"""
    return np.concatenate([edge_fields(name)[key] for name in EDGE_FAMILIES])


@functools.lru_cache(maxsize=None)
def edge_mixed():
    """(blocks, expected, order): block i = edge_sorted's block order[i], of class i % 4 (solid, opaque, grey with alpha, RGBA); each class cycles through
    its own blocks and the strip is four times the largest class long (RGBA, 771 of the 1600 blocks: 3084 blocks), so every block occurs and every aligned
    run of 64 holds all four classes"""
    b, e = edge_sorted()
    cls = block_class(b)
    pools = [np.nonzero(cls == c)[0] for c in range(4)]
    assert all(p.size for p in pools)
    i = np.arange(4 * max(p.size for p in pools))
    order = np.zeros(i.size, dtype=np.int64)
    for c, p in enumerate(pools):
        order[c::4] = p[(i[c::4] // 4) % p.size]
    out = (b[order], e[order], order)
    for v in out:
        v.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def mixed_pattern():
    """formula_image(64, 64) with every third of its 8 x 8 tiles that are neither flat nor opaque turned grey (G := R, B := R): solid, opaque, grey with
    alpha and RGBA blocks next to each other in every block row.  Read-only"""
    img = formula_image(64, 64)
    t = np.add.outer(np.arange(8), np.arange(8))  # [ty, tx]
    free = np.nonzero(((t % 2 == 0) & (t % 5 != 0)).reshape(-1))[0][0::3]
    for ty, tx in zip(*np.unravel_index(free, (8, 8))):
        tile = img[8 * ty:8 * ty + 8, 8 * tx:8 * tx + 8]
        tile[..., 1] = tile[..., 2] = tile[..., 0]
    img.setflags(write=False)
    return img


@functools.lru_cache(maxsize=None)
def mixed_pattern_expected():
    """[16, 16, 16]"""
    e = um.encode(ec.to_blocks(mixed_pattern())).reshape(16, 16, 16)
    e.setflags(write=False)
    return e
