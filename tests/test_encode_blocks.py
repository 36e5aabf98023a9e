"""The encoders from pixels of DESIGN.md section 4.10 on the CPU: bu_encode_blocks.hpp -- the header the gfx950 encode kernels include, holding the
gather of a block's texels with edge replication and the call of the per-block encoders -- compiled for the host and compared with the numpy models
(tests/encode_cases.py); the same header in a stand-alone program under AddressSanitizer and UBSan, run as a child process over heap images that
end at their last pixel (nothing built with a sanitizer is loaded into this process); and the argument rules of the two entry points that are
decided before a device is needed."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import encode_cases as ec
from basisu_rs_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST_EMUL = os.path.join(ROOT, "tests", "host_emul")
CSRC = os.path.join(ROOT, "basisu_rs_amd", "csrc")
PADS = (0, 4, 64)  # pitch - 4 * width


@pytest.fixture(scope="module")
def emul_encode(tmp_path_factory):
    """(name, flat image bytes, w, h, pitch) -> blocks [nby, nbx, block bytes] through the plain host build of bu_encode_blocks.hpp"""
    so = str(tmp_path_factory.mktemp("emul_encode") / "libbu_emul_encode.so")
    r = subprocess.run(["g++", "-std=c++17", "-O2", "-shared", "-fPIC", "-Wall", "-Wno-unknown-pragmas", "-I" + CSRC, "-o", so,
                        os.path.join(HOST_EMUL, "bu_emul_encode.cpp")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    lib = ctypes.CDLL(so)
    lib.bu_emul_encode_image.argtypes = [ctypes.c_int, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_size_t, ctypes.c_size_t, ctypes.c_void_p]
    lib.bu_emul_encode_image.restype = ctypes.c_int

    def run(name, buf, w, h, pitch):
        t, bb = ec.FORMATS[name]
        nbx, nby = ec.blocks_of(w, h)
        assert buf.size == ec.image_bytes(w, h, pitch)
        out = np.zeros((nby, nbx, bb), dtype=np.uint8)
        assert lib.bu_emul_encode_image(t, buf.ctypes.data, w, h, pitch, out.ctypes.data) == 0
        return out

    run.lib = lib
    return run


@pytest.mark.parametrize("shape", list(ec.SHAPES), ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("name", list(ec.FORMATS))
def test_host_build_against_the_models(emul_encode, name, shape):
    """all six formats, every shape, every kind of image, tight and padded pitches; the padding bytes differ from call to call"""
    w, h = shape
    for k, kind in enumerate(ec.KINDS):
        want = ec.expected(name, kind, w, h)
        for pad in PADS:
            pitch = 4 * w + pad
            fill = np.random.default_rng(100 * k + pad).integers(0, 256, size=ec.image_bytes(w, h, pitch), dtype=np.uint8)
            got = emul_encode(name, ec.pitched(ec.image(kind, w, h), pitch, fill), w, h, pitch)
            bad = np.argwhere((got != want).any(-1))
            assert bad.size == 0, "%s %s %dx%d pad %d: blocks (by, bx) %s differ" % (name, kind, w, h, pad, bad[:5].tolist())


def test_host_build_refuses_other_formats(emul_encode):
    buf = np.zeros(64, dtype=np.uint8)
    for t in ec.OTHER_FORMATS:
        assert emul_encode.lib.bu_emul_encode_image(t, buf.ctypes.data, 4, 4, 16, buf.ctypes.data) == -1


def test_cases_are_what_they_claim_to_be():
    """the images reach the paths they are there for"""
    import colour_model as col

    f = col.fields(ec.to_blocks(ec.image("solid", 257, 8)))
    assert f["solid"].all()
    f = col.fields(ec.to_blocks(ec.image("checker", 257, 8)))
    assert not f["solid"].any() and f["eq"].any() and f["det0"].any()  # two colours everywhere; one pair quantises to equal endpoints
    assert f["rejected"].any() and f["swap"].any()
    f = col.fields(ec.to_blocks(ec.image("gradient", 257, 8)))
    assert f["kept"].any() and f["rejected"].any() and f["swap"].any() and f["tie_sel"].any()
    assert col.fields(ec.to_blocks(ec.image("random", 257, 8)))["kept"].any()
    for w, h in ec.SHAPES:
        nbx, nby = ec.blocks_of(w, h)
        assert ec.to_blocks(ec.image("random", w, h)).shape == (nbx * nby, 64)
    # replication: the partial block of a 5 x 3 image repeats column 4 and row 2
    b = ec.to_blocks(ec.image("random", 5, 3)).reshape(2, 4, 4, 4)
    img = ec.image("random", 5, 3)
    assert (b[1, :3, :] == img[:, 4:5]).all() and (b[1, 3] == img[2, 4]).all() and (b[0, 3] == img[2, :4]).all()


def test_stand_alone_build_under_asan_and_ubsan(tmp_path):
    """every block of every shape, gathered from a heap image of exactly (h - 1) * pitch + 4 w bytes (one byte past the last pixel is a heap
    overflow) and encoded to all six formats under -fsanitize=address,undefined; the checksums of the gathered texels and of the blocks are numpy's"""
    exe = str(tmp_path / "bu_emul_encode_main")
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-Wall", "-Wno-unknown-pragmas",
                        "-I" + CSRC, "-o", exe, os.path.join(HOST_EMUL, "bu_emul_encode_main.cpp")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    cases = [(w, h, pad) for (w, h) in ec.SHAPES for pad in PADS]
    r = subprocess.run([exe] + [str(v) for c in cases for v in c], capture_output=True, text=True)
    assert r.returncode == 0, (r.returncode, r.stderr[-3000:])
    lines = r.stdout.split("\n")[:-1]
    assert len(lines) == len(cases)
    for (w, h, pad), line in zip(cases, lines):
        got = [int(v) for v in line.split()]
        blocks = ec.to_blocks(ec.formula_image(w, h))
        want = [w, h, pad, ec.weighted_sum(blocks.view("<u4"))] + [ec.weighted_sum(ec.model(name, blocks)) for name in ec.FORMATS]
        assert got == want, (w, h, pad)


# ---- argument rules decided before a device is needed ---------------------------------------------------------------------------------------
# Every refusal below is returned before the context is looked at, so a block of zeroed memory stands in for one; a null context is refused whatever
# else is passed.  The calls that would reach the device (valid arguments and a non-empty image) are the GPU tests'.
@pytest.fixture(scope="module")
def lib():
    return _lib.load()


def _device_rows(lib, ctx):
    buf = ctypes.create_string_buffer(1 << 16)
    p = (ctypes.addressof(buf) + 255) & ~255

    def call(c=ctx, fmt=_lib.BC3_RGBA, src=p, w=32, h=8, in_pitch=0, dst=p + 4096, out_pitch=0):
        return lib.bu_rgba_encode_blocks_device(c, fmt, src, w, h, in_pitch, dst, out_pitch, None)

    rows = [dict(fmt=t) for t in ec.OTHER_FORMATS] + [dict(fmt=t, w=0) for t in ec.OTHER_FORMATS]
    rows += [dict(src=None), dict(dst=None)]
    rows += [dict(src=p + 2), dict(src=p + 1), dict(dst=p + 4096 + 8), dict(fmt=_lib.BC1_RGB, dst=p + 4096 + 4), dict(fmt=_lib.EAC_R11, dst=p + 4096 + 4)]
    rows += [dict(in_pitch=4 * 32 - 4), dict(in_pitch=4 * 32 + 2), dict(in_pitch=4), dict(in_pitch=4 * 32 + 2, h=0)]
    rows += [dict(out_pitch=16 * 8 - 16), dict(out_pitch=16 * 8 + 8), dict(fmt=_lib.BC4_R, out_pitch=8 * 8 + 4), dict(out_pitch=16, h=0)]
    rows += [dict(w=(1 << 30) + 1), dict(w=1 << 40), dict(w=(1 << 64) - 1)]  # nbx above 2^28
    return call, rows


def test_device_form_argument_rules(lib):
    fake = ctypes.create_string_buffer(1 << 16)
    call, rows = _device_rows(lib, ctypes.addressof(fake))
    A = _lib.ERR_ARGUMENT
    for row in rows:
        assert call(**row) == A, row
        assert call(c=None, **row) == A, row  # a null context with every bad-argument row
    assert call(c=None) == A and call(c=None, w=0) == A
    # an empty image is not an error: no launch, the context is not touched, null buffers are allowed
    for row in (dict(w=0), dict(h=0), dict(w=0, h=0), dict(w=0, src=None, dst=None), dict(h=0, in_pitch=4 * 32 + 64, out_pitch=16 * 8 + 48)):
        assert call(**row) == _lib.OK, row
    assert call(fmt=_lib.BC1_RGB, dst=4096 + 8, src=4, w=0) == _lib.OK  # the smallest alignments
    assert call(w=1 << 30, h=0) == _lib.OK  # nbx = 2^28 is the widest image


def test_host_form_argument_rules(lib):
    fake = ctypes.create_string_buffer(1 << 16)
    ctx = ctypes.addressof(fake)
    src, dst = ctypes.create_string_buffer(4096), ctypes.create_string_buffer(4096)

    def call(c=ctx, fmt=_lib.BC3_RGBA, data=src, w=32, h=8, in_pitch=0, out=dst, out_bytes=4096):
        return lib.bu_rgba_encode_blocks(c, fmt, data, w, h, in_pitch, out, out_bytes)

    A = _lib.ERR_ARGUMENT
    rows = [dict(fmt=t) for t in ec.OTHER_FORMATS] + [dict(data=None), dict(out=None), dict(in_pitch=4 * 32 - 4), dict(in_pitch=4 * 32 + 2), dict(w=(1 << 30) + 1)]
    for row in rows:
        assert call(**row) == A, row
        assert call(c=None, **row) == A, row
    assert call(c=None) == A
    assert call(out_bytes=16 * 8 * 2 - 1) == _lib.ERR_OUTPUT_SIZE and call(fmt=_lib.BC4_R, w=5, h=5, out_bytes=31) == _lib.ERR_OUTPUT_SIZE
    assert call(w=0) == _lib.OK and call(h=0, data=None, out=None, out_bytes=0) == _lib.OK


def test_binding_rust_facade_and_header_spell_the_two_calls_alike():
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "basisu_hip.h")).read(), flags=re.S)
    rs = re.sub(r"//.*", "", open(os.path.join(ROOT, "rust", "src", "ffi.rs")).read())
    lib_rs = open(os.path.join(ROOT, "rust", "src", "lib.rs")).read()
    for name, n_params in (("bu_rgba_encode_blocks_device", 9), ("bu_rgba_encode_blocks", 8)):
        m = re.search(r"bu_status\s+%s\s*\(([^;]*?)\)\s*;" % name, hdr, flags=re.S)
        assert m and m.group(1).count(",") + 1 == n_params
        assert name in _lib.SYMBOLS
        m = re.search(r"fn %s\s*\((.*?)\)\s*->\s*c_int;" % name, rs, flags=re.S)
        assert m and m.group(1).count(":") == n_params and ("ffi::%s(" % name) in lib_rs
    assert re.search(r"pub fn encode_blocks\(", lib_rs) and re.search(r"pub unsafe fn encode_blocks_device\(", lib_rs)
