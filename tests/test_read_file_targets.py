"""bu_read_file_query / bu_read_file_to on the CPU: the whole-file call keyed by block format (include/basisu_hip.h, DESIGN.md section
4.6).  Image geometry of an ETC1S file for BC1, BC3, BC4, BC5, EAC R11 and EAC RG11, delegation of everything bu_read_to already
serves, the refusals and their order, and the slice lookup of the whole-file kernels (bu_etc1s_unit_slice) through a host build."""
import ctypes
import itertools
import os
import subprocess

import numpy as np
import pytest

import basis_builder as bb
from basisu_rs_amd import BasisuError, _lib, read_file_query, read_query, write_uastc_file

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST_EMUL = os.path.join(ROOT, "tests", "host_emul")
CSRC = os.path.join(ROOT, "basisu_rs_amd", "csrc")
SIX = {"bc1": (11, 8), "bc3": (12, 16), "bc4": (6, 8), "bc5": (7, 16), "r11": (8, 8), "rg11": (9, 16)}  # name -> (bu_target, bytes per block)
# bu_target -> the read target whose block target it is
READ_OF = {_lib.ASTC: _lib.READ_ASTC, _lib.BC7: _lib.READ_BC7, _lib.ETC1: _lib.READ_ETC1, _lib.ETC2: _lib.READ_ETC2, _lib.RGBA32: _lib.READ_RGBA,
           _lib.BC4_R: _lib.READ_BC4, _lib.BC5_RG: _lib.READ_BC5, _lib.EAC_R11: _lib.READ_EAC_R11, _lib.EAC_RG11: _lib.READ_EAC_RG11,
           _lib.BC1_RGB: _lib.READ_BC1, _lib.BC3_RGBA: _lib.READ_BC3}
DIMS = [(64, 64), (33, 17), (1, 1)]


def status_of(fn, *args):
    try:
        fn(*args)
        return _lib.OK
    except BasisuError as e:
        return e.status


@pytest.fixture(scope="module")
def files():
    return {alpha: bb.etc1s_file(np.random.default_rng(61), DIMS, n_codebook=1024, alpha=alpha)[0] for alpha in (True, False)}


@pytest.mark.parametrize("alpha", [True, False], ids=["alpha", "opaque"])
def test_query_geometry_of_an_etc1s_file(files, alpha):
    """one image per colour / alpha pair (or per slice), sum of nbx * nby * block bytes; ETC1 and RGBA32 are bu_read_query's"""
    f = files[alpha]
    blocks = sum(x * y for x, y in DIMS)
    for name, (t, bytes_per_block) in SIX.items():
        assert read_file_query(t, f) == (3, blocks * bytes_per_block), name
    assert read_file_query(_lib.ETC1, f) == read_query(_lib.READ_ETC1, f) == (6 if alpha else 3, blocks * 8 * (2 if alpha else 1))
    assert read_file_query(_lib.RGBA32, f) == read_query(_lib.READ_RGBA, f) == (3, blocks * 64)


def test_uastc_file_is_read_query(golden):
    blocks = golden["uastc"][:48]
    f = write_uastc_file([dict(data=blocks[:32].tobytes(), orig_w=32, orig_h=16, nbx=8, nby=4),
                          dict(data=blocks[32:].tobytes(), orig_w=16, orig_h=16, nbx=4, nby=4, image_index=1)])
    assert len(READ_OF) == 11
    for t, rt in READ_OF.items():
        assert read_file_query(t, f) == read_query(rt, f) == (2, 48 * _lib.BLOCK_BYTES[t]), t


def test_refusals(files):
    lib = _lib.load()
    n, nb = ctypes.c_size_t(0), ctypes.c_size_t(0)
    f = files[True]
    for buf in (np.frombuffer(f, dtype=np.uint8), np.zeros(0, dtype=np.uint8)):
        for t in (5, 10, 13, -1):  # no bu_target: refused before the file is looked at
            assert lib.bu_read_file_query(t, buf.ctypes.data, buf.size, ctypes.byref(n), ctypes.byref(nb)) == _lib.ERR_ARGUMENT, (t, buf.size)
    for alpha in (True, False):
        for t in (_lib.ASTC, _lib.BC7, _lib.ETC2):  # no rule for them yet
            assert status_of(read_file_query, t, files[alpha]) == _lib.ERR_UNSUPPORTED, t
    # flagged alpha, odd slice count: the last slice dropped from the header's count
    g = bytearray(f)
    g[14:17] = (5).to_bytes(3, "little")
    g = bb.reseal(bytes(g))
    assert status_of(read_query, _lib.READ_RGBA, g) == _lib.ERR_ALPHA_SLICES
    for name, (t, _) in SIX.items():
        assert status_of(read_file_query, t, g) == _lib.ERR_ALPHA_SLICES, name
    # second slice of a pair without the alpha flag; unequal block grids
    for field, value in ((4, 0), (9, 63)):
        g = bytearray(f)
        g[77 + 23 + field] = value
        g = bb.reseal(bytes(g))
        assert status_of(read_query, _lib.READ_RGBA, g) == _lib.ERR_ALPHA_SLICES
        assert status_of(read_file_query, _lib.BC3_RGBA, g) == _lib.ERR_ALPHA_SLICES


def test_error_order_is_that_of_read_query_rgba(files):
    f = files[True]
    flipped = bytearray(f)
    flipped[-1] ^= 0x10  # payload damage, CRCs left alone
    past_eof = bytearray(f)
    past_eof[77 + 2 * 23 + 17:77 + 2 * 23 + 21] = len(f).to_bytes(4, "little")  # slice 2: file_size past the end
    damaged = {"data crc": bytes(flipped), "truncated header": f[:50], "slice past EOF": bb.reseal(bytes(past_eof))}
    seen = set()
    for what, g in damaged.items():
        want = status_of(read_query, _lib.READ_RGBA, g)
        assert want != _lib.OK, what
        assert status_of(read_file_query, _lib.BC1_RGB, g) == want, what
        seen.add(want)
    assert status_of(read_query, _lib.READ_RGBA, damaged["data crc"]) == _lib.ERR_DATA_CRC
    assert len(seen) == 3
    # an unknown tex_format is reported before the kind / target combination
    g = bytearray(f)
    g[20] = 2
    g = bb.reseal(bytes(g))
    assert status_of(read_file_query, _lib.ASTC, g) == status_of(read_query, _lib.READ_RGBA, g) != _lib.ERR_UNSUPPORTED


def test_read_query_still_refuses_the_etc1s_file(files):
    assert status_of(read_query, _lib.READ_BC1, files[True]) == _lib.ERR_ARGUMENT
    assert status_of(read_query, _lib.READ_BC1, files[False]) == _lib.ERR_ARGUMENT


# ---- bu_etc1s_unit_slice through a host build -------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def slices_lib(tmp_path_factory):
    so = tmp_path_factory.mktemp("etc1s_slices") / "libbu_emul_etc1s_slices_ubsan.so"
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=undefined", "-fno-sanitize-recover=undefined", "-fPIC", "-shared", "-Wall",
                    "-Wno-unknown-pragmas", "-I" + CSRC, "-o", str(so), os.path.join(HOST_EMUL, "bu_emul_etc1s_slices.cpp")], check=True)
    lib = ctypes.CDLL(str(so))
    lib.bu_emul_etc1s_slice_bytes.restype = ctypes.c_size_t
    lib.bu_emul_etc1s_unit_slices.argtypes = [ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_void_p]
    lib.bu_emul_etc1s_unit_slices.restype = None
    return lib


SLICE = np.dtype([("unit0", "<u4"), ("n_blocks", "<u4"), ("nbx", "<u4"), ("idx_ofs", "<u4"), ("aidx_ofs", "<u4"), ("image", "<u4"), ("out_ofs", "<u8")])


def table_of(block_counts):
    """the descriptor table as the host builds it: images without blocks are skipped, the sentinel holds the total"""
    rows, units = [], 0
    for image, n in enumerate(block_counts):
        if n == 0:
            continue
        rows.append((units, n, 1, 0, 0xFFFFFFFF, image, 0))
        units += (n + 63) // 64
    rows.append((units, 0, 0, 0, 0, 0, 0))
    return np.array(rows, dtype=SLICE), units


def orders():
    sizes = [1, 63, 64, 65, 561, 4096]
    out = [sizes, sizes[::-1], [4096, 1, 561, 63, 65, 64], [64, 64, 1, 1, 4096, 65, 63, 561], [1], [4096], [65]]
    out += [list(p) for p in itertools.islice(itertools.permutations(sizes), 5, 720, 97)]
    gaps = [[0] + sizes, sizes + [0], [0, 0, 1, 0, 63, 64, 0, 0, 65, 561, 0, 4096, 0], [0, 65, 0]]  # empty images between the others
    return out + gaps


def test_unit_slice_equals_a_linear_scan_and_covers_every_block_once(slices_lib):
    assert slices_lib.bu_emul_etc1s_slice_bytes() == SLICE.itemsize == 32
    lanes = np.arange(64, dtype=np.int64)
    for counts in orders():
        table, n_units = table_of(counts)
        n_slices = table.size - 1
        unit0 = table["unit0"].astype(np.int64)
        assert (np.diff(unit0[:n_slices]) > 0).all() and unit0[0] == 0  # consecutive entries never share a unit0
        got = np.full(n_units, 0xFFFFFFFF, dtype=np.uint32)
        slices_lib.bu_emul_etc1s_unit_slices(table.ctypes.data, n_slices, n_units, got.ctypes.data)
        scan = np.array([max(s for s in range(n_slices) if unit0[s] <= u) for u in range(n_units)], dtype=np.uint32)
        assert (got == scan).all(), counts
        hits = [np.zeros(int(n), dtype=np.int64) for n in table["n_blocks"][:n_slices]]
        for u in range(n_units):
            s = int(got[u])
            i = (u - unit0[s]) * 64 + lanes
            assert (i >= 0).all()
            ok = i < int(table["n_blocks"][s])  # the kernel's test: nothing at or past n_blocks is accepted
            np.add.at(hits[s], i[ok], 1)
        for s in range(n_slices):
            assert (hits[s] == 1).all(), (counts, s)
        assert [table["image"][s] for s in range(n_slices)] == [k for k, n in enumerate(counts) if n]
