"""The shapes real `.basis` files have, as ETC1S files for the whole-file calls (bu_read_to, bu_read_file_to; csrc/bu_capi_file.hpp): a cube map with mips, images
whose block counts sit either side of a 64-block unit, a texture array of many small images, a mip chain down to 1 x 1 blocks.  Shared by
tests/test_file_shape_cases.py (CPU: oracle, layout and unit search) and tests/test_gpu_file_shapes.py (the kernels behind both front doors).

All dims are (nbx, nby) in blocks.  Every file is basis_builder.etc1s_file(default_rng(seed), dims, n_codebook=1024, alpha=...), with and without alpha pairs.
Which front door a shape takes is decided by the file's TOTAL block count, whether its payload CRC is deferred by the file's size; both are asserted per shape
(check_door) against the constants restated here, which tests/test_file_shape_cases.py pins to the source.

Expected values: the oracle's images byte for byte (oracle_images), and for the six block targets the numpy models applied to the blocks of the oracle's
RGBA32 read (want_blocks, model_blocks, check_model)."""
import functools

import numpy as np

import basis_builder as bb
import test_etc1s_targets as tet
from basisu_rs_amd import read_header, read_slice_descs

STREAM_MIN_BLOCKS = 32768   # BU_ETC1S_STREAM_MIN_BLOCKS: the streamed front door from this many blocks in the whole file
BAND_BLOCKS = 16384         # BU_ETC1S_BAND_BLOCKS: the feeder launches an unfinished image in bands of at least this many blocks
CRC_DEFER_BYTES = 64 << 10  # ETC1S files from this size on have their payload CRC checked beside the decode, not up front
UNIT = 64

# name -> (dims, seed, streamed, CRC deferred without alpha, CRC deferred with alpha)
SHAPES = {
    # one launch; a 37-entry table with the sentinel; per face 32 x 32 ... 1 x 1: 18 images smaller than one unit
    "cube_mips": ([(s, s) for _ in range(6) for s in (32, 16, 8, 4, 2, 1)], 4101, False, False, False),
    # one launch; block counts 63, 64, 65, 127, 128, 129, 1, 4095, 4096, 4097; images of one column and of one row
    "unit_edges": ([(63, 1), (1, 64), (5, 13), (127, 1), (2, 64), (3, 43), (1, 1), (65, 63), (64, 64), (17, 241)], 4102, False, False, False),
    # streamed although every image is far below a band: 144 images that end in a unit with 48 of 64 lanes live; a 145-entry table
    "array_240": ([(16, 15)] * 144, 4103, True, False, True),
    # streamed; the first slice is decoded on two threads and fed in bands, then a tail of small images down to one block
    "mip_chain_192": ([(192, 192), (96, 96), (48, 48), (24, 24), (12, 12), (6, 6), (3, 3), (2, 2), (1, 1)], 4104, True, False, True),
}
TOTALS = {"cube_mips": (36, 8190), "unit_edges": (10, 12865), "array_240": (144, 34560), "mip_chain_192": (9, 49154)}  # images, blocks
NAMES = tuple(SHAPES)
STREAMED = tuple(n for n in NAMES if SHAPES[n][2])


def dims_of(name):
    return SHAPES[name][0]


def total_blocks(name):
    return sum(x * y for x, y in dims_of(name))


@functools.lru_cache(maxsize=None)
def etc1s_file(name, alpha):
    dims, seed = SHAPES[name][:2]
    return bb.etc1s_file(np.random.default_rng(seed), dims, n_codebook=1024, alpha=alpha)[0]


def check_door(name, alpha):
    """the shape is what its row says: image and block counts, the front door by the total block count, the CRC mode by the file's size"""
    dims, _, streamed, deferred_opaque, deferred_alpha = SHAPES[name]
    assert (len(dims), total_blocks(name)) == TOTALS[name], name
    assert (total_blocks(name) >= STREAM_MIN_BLOCKS) == streamed, name
    assert (len(etc1s_file(name, alpha)) >= CRC_DEFER_BYTES) == (deferred_alpha if alpha else deferred_opaque), (name, alpha, len(etc1s_file(name, alpha)))
    if name == "array_240":  # every image below a band, three quarters of its last unit live
        assert all(x * y < BAND_BLOCKS and x * y % UNIT == 48 for x, y in dims)
    if name == "mip_chain_192":  # the first slice is split over two threads and is more than two bands long
        assert dims[0][0] * dims[0][1] >= STREAM_MIN_BLOCKS and dims[0][0] * dims[0][1] > 2 * BAND_BLOCKS


def colour_slice(f, image, alpha):
    """the slice descriptor of an image's colour slice"""
    return read_slice_descs(f, read_header(f))[(2 if alpha else 1) * image]


def damaged(f, images, alpha):
    """the file with the first min(64, file_size) bytes of the colour slices of `images` inverted, behind recomputed CRCs"""
    g = bytearray(f)
    for image in images:
        d = colour_slice(f, image, alpha)
        for k in range(d.file_ofs, d.file_ofs + min(64, d.file_size)):
            g[k] ^= 0xFF
    return bb.reseal(bytes(g))


# ---- expected values ------------------------------------------------------------------------------------------------------------------
def tuples(imgs):
    return [(g.w, g.h, g.stride, g.data.tobytes()) for g in imgs]


def oracle_images(oracle, which, f):
    """(header as a list, [(w, h, stride, bytes)]) of the oracle's whole-file read"""
    st, hdr, imgs = oracle.read_to(which, f)
    assert st == 0
    return hdr, [(w, h, s, d.tobytes()) for (w, h, s, d) in imgs]


def want_blocks(oracle, f, alpha):
    """per image: (w, h, nbx, blocks [n, 64] of the oracle's RGBA32 read)"""
    st, _, imgs = oracle.read_to("rgba", f)
    assert st == 0
    descs = read_slice_descs(f, read_header(f))
    step = 2 if alpha else 1
    assert len(imgs) * step == len(descs)
    out = []
    for k, (_, _, _, data) in enumerate(imgs):
        d = descs[step * k]
        nbx, nby = d.num_blocks_x, d.num_blocks_y
        assert data.size == nbx * nby * 64
        out.append((d.orig_width, d.orig_height, nbx, data.reshape(nby, 4, nbx, 4, 4).transpose(0, 2, 1, 3, 4).reshape(-1, 64)))  # image -> blocks
    return out


def model_blocks(want, name):
    """per image the target's blocks [n, bytes per block]: the colour or the channel model over all images of want_blocks at once"""
    sizes = [rgba.shape[0] for _, _, _, rgba in want]
    model = tet.model(name, np.concatenate([rgba for _, _, _, rgba in want]))
    return np.split(model, np.cumsum(sizes)[:-1])


def check_model(got, want, name, models=None):
    """the images of a read to one of the six block targets against the model of want_blocks (models: model_blocks(want, name), computed before)"""
    bytes_per_block = tet.TARGETS[name][1]
    assert len(got) == len(want)
    if models is None:
        models = model_blocks(want, name)
    for k, (g, (w, h, nbx, _), model) in enumerate(zip(got, want, models)):
        assert (g.w, g.h, g.stride) == (w, h, bytes_per_block * nbx), (name, k)
        blocks = np.frombuffer(g.data.tobytes(), dtype=np.uint8).reshape(-1, bytes_per_block)
        assert blocks.shape == model.shape, (name, k)
        bad = np.nonzero((blocks != model).any(1))[0]
        assert bad.size == 0, "%s image %d: %d blocks differ, first %d: %s vs %s" % (name, k, bad.size, bad[0], blocks[bad[0]], model[bad[0]])
