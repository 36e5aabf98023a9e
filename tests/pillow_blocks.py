"""BC blocks decoded by a third party: Pillow's DDS reader, through PIL.Image.open of a DDS file built in memory.  Needs Pillow; the callers decide
what to do without it (tests/golden/make_bc7_third_party.py is run by hand; the live tests of tests/test_decode_fields.py skip).

decode(fmt, blocks) -> [n, 16, 4] uint8: the texels of each block, texel i = 4y + x, channels R, G, B, A (BC4: the value in R, G and B, A = 255;
BC5: R, G, B = 0 as Pillow gives it, A = 255)."""
import io
import struct

import numpy as np

DXGI = {"bc1": (71, 8, "RGBA"), "bc3": (77, 16, "RGBA"), "bc4": (80, 8, "L"), "bc5": (83, 16, "RGB"), "bc7": (98, 16, "RGBA")}  # format, block bytes, mode


def dds(fmt, blocks, bw):
    """the DDS file of `blocks` (a whole number of rows of bw blocks, row-major): magic, the 124-byte header, the DX10 header, the blocks"""
    dxgi, bb, _ = DXGI[fmt]
    blocks = np.ascontiguousarray(blocks, dtype=np.uint8).reshape(-1, bb)
    n = blocks.shape[0]
    assert n % bw == 0
    flags = 0x1 | 0x2 | 0x4 | 0x1000 | 0x80000  # caps, height, width, pixel format, linear size
    pixel_format = struct.pack("<II4s5I", 32, 0x4, b"DX10", 0, 0, 0, 0, 0)
    header = struct.pack("<7I44x", 124, flags, 4 * (n // bw), 4 * bw, n * bb, 0, 1) + pixel_format + struct.pack("<5I", 0x1000, 0, 0, 0, 0)
    assert len(header) == 124
    return b"DDS " + header + struct.pack("<5I", dxgi, 3, 0, 1, 0) + blocks.tobytes()


def decode(fmt, blocks, bw=None):
    from PIL import Image

    _, bb, mode = DXGI[fmt]
    blocks = np.ascontiguousarray(blocks, dtype=np.uint8).reshape(-1, bb)
    n = blocks.shape[0]
    if bw is None:
        bw = next(w for w in (256, 128, 64, 32, 16, 8, 4, 2, 1) if n % w == 0)
    im = Image.open(io.BytesIO(dds(fmt, blocks, bw)))
    assert im.mode == mode and im.size == (4 * bw, 4 * (n // bw)), (im.mode, im.size)
    a = np.asarray(im.convert("RGBA"), dtype=np.uint8)
    return np.ascontiguousarray(a.reshape(n // bw, 4, bw, 4, 4).transpose(0, 2, 1, 3, 4)).reshape(n, 16, 4)
