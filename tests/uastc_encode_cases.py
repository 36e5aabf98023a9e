"""Shared cases of the encoder from pixels to UASTC (bu_rgba_encode_uastc): images, shapes and the model's answer for each,
computed once per process and shared by the CPU and the GPU tests.

An image is a variant of an encode_cases.image kind:
  plain    the kind as it is (random alpha, mostly: the RGBA modes 14, 12, 10; solid tiles: mode 8)
  opaque   A := 255 (modes 5, 0, 18)
  grey     G := R, B := R (mode 15)
  ag       A := G (alpha correlated with colour)
Every shape of the list carries at least one image; the whole list is about 2800 blocks."""
import functools

import numpy as np

import encode_cases as ec
import uastc_encode_model as um

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
