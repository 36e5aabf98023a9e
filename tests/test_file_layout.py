"""The whole-file layout (csrc/bu_file_layout.hpp) on the CPU, through the stand-alone host build tests/host_emul/bu_emul_file_layout.cpp compiled with and
without -fsanitize=undefined (a report aborts it): the ETC1S index buffer and slice table against a model written here, the UASTC runs, the piece sizes
and the carve-up of the aux buffer against literals, the fold of the CRC piece registers against the plain CRC."""
import json
import os
import subprocess

import numpy as np
import pytest

import basis_builder as bb
from basisu_rs_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "basisu_rs_amd", "csrc")
SRC = os.path.join(ROOT, "tests", "host_emul", "bu_emul_file_layout.cpp")
MIB = 1 << 20
PIECE = 65536  # BU_CRC_PIECE


@pytest.fixture(scope="module", params=["plain", "ubsan"])
def layout(request, tmp_path_factory):
    """run(command, *args) -> the JSON the stand-alone build prints"""
    d = tmp_path_factory.mktemp("file_layout_" + request.param)
    exe = d / "bu_emul_file_layout"
    flags = ["-O1", "-g", "-fsanitize=undefined", "-fno-sanitize-recover=undefined"] if request.param == "ubsan" else ["-O2"]
    subprocess.run(["g++", "-std=c++17"] + flags + ["-Wall", "-Wno-unknown-pragmas", "-pthread", "-I" + CSRC, "-o", str(exe), SRC], check=True)
    count = [0]

    def run(*args, file=None):
        args = [str(a) for a in args]
        if file is not None:
            count[0] += 1
            path = d / ("f%d.basis" % count[0])
            path.write_bytes(file)
            args.insert(1 if args[0] == "fold" else len(args), str(path))
        r = subprocess.run([str(exe)] + args, capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, (args, r.returncode, r.stderr[-2000:])
        return json.loads(r.stdout)

    return run


def test_header_builds_alone():
    """the header includes what it needs and nothing of HIP: g++ -Wall alone, without a warning"""
    r = subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-fsyntax-only", "-I" + CSRC, "-include", "bu_file_layout.hpp", "-x", "c++", os.devnull],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]


# ---- ETC1S --------------------------------------------------------------------------------------------------------------------------
DIMS = [(64, 64), (33, 17), (0, 0), (1, 1)]


def etc1s_model(dims, alpha_pairs, block_bytes, rgba):
    """pad to 64, colour then alpha, skip empty images, sentinel"""
    words = units = out_ofs = 0
    idx, aidx, unit0, units_of, descs = [], [], [], [], []
    for image, (x, y) in enumerate(dims):
        n = x * y
        padded = (n + 63) // 64 * 64
        idx.append(words)
        words += padded
        aidx.append(words if alpha_pairs else 0)
        words += padded if alpha_pairs else 0
        unit0.append(units)
        units_of.append(padded // 64)
        if n:
            descs.append([units, n, x, idx[-1], aidx[-1] if alpha_pairs else 0xFFFFFFFF, image, out_ofs])
        units += padded // 64
        out_ofs += n * (64 if rgba else block_bytes)
    descs.append([units, 0, 0, 0, 0, 0, 0])
    return dict(status=0, words=words, n_units=units, idx_ofs=idx, aidx_ofs=aidx, unit0=unit0, units_of=units_of, descs=descs)


@pytest.fixture(scope="module")
def etc1s_files():
    # (the (0,0) slice is built as (1,1) and emptied in the slice table: the layout reads the table alone)
    out = {}
    for alpha in (True, False):
        f = bytearray(bb.etc1s_file(np.random.default_rng(61), [d if d != (0, 0) else (1, 1) for d in DIMS], n_codebook=1024, alpha=alpha)[0])
        for i in range(len(DIMS) * (2 if alpha else 1)):
            if DIMS[i // (2 if alpha else 1)] == (0, 0):
                f[77 + 23 * i + 9:77 + 23 * i + 13] = bytes(4)  # num_blocks_x, num_blocks_y
        out[alpha] = bb.reseal(bytes(f))
    return out


ETC1S_TARGETS = {"etc1": (_lib.READ_ETC1, 0, 8), "rgba": (_lib.READ_RGBA, 0, 16), "bc3": (_lib.READ_BC3, 1, 16)}  # name -> (read target, six, block bytes)


def check_etc1s_layout(layout, f, file_dims, alpha, target):
    """the layout of the ETC1S file f (images of file_dims blocks, alpha: colour / alpha slice pairs) for `target` is the model's, and the kernel's
    lookup over the produced table finds every unit's image -> (the layout, unit_slice: the table entry of every unit)"""
    read_target, six, block_bytes = ETC1S_TARGETS[target]
    pairs = alpha and target != "etc1"  # ETC1 of a file with alpha: every slice is an image of its own
    dims = file_dims if pairs or not alpha else [d for d in file_dims for _ in range(2)]
    got = layout("etc1s", read_target, six, file=f)
    want = etc1s_model(dims, pairs, block_bytes, target == "rgba")
    unit_slice = got.pop("unit_slice")
    assert got == want
    # the kernel's lookup over the produced table finds, for every unit, the entry of the image whose [unit0, unit0 + units_of) holds it
    assert len(unit_slice) == got["n_units"] > 0
    for u, s in enumerate(unit_slice):
        image = got["descs"][s][5]
        assert got["unit0"][image] <= u < got["unit0"][image] + got["units_of"][image], u
    spans = 2 if pairs else 1
    for d in got["descs"][:-1]:
        assert d[3] + d[1] <= got["words"] and (spans == 1 or d[4] + d[1] <= got["words"])
    return got, unit_slice


@pytest.mark.parametrize("alpha", [True, False], ids=["alpha", "opaque"])
@pytest.mark.parametrize("target", list(ETC1S_TARGETS))
def test_etc1s_layout_is_the_model(layout, etc1s_files, alpha, target):
    check_etc1s_layout(layout, etc1s_files[alpha], DIMS, alpha, target)


def test_etc1s_layout_that_does_not_fit_32_bits_is_out_of_bounds(layout):
    """two slices of 65 535 x 65 535 blocks: each block count fits, the second one's end does not"""
    assert layout("etc1s-huge")["status"] == _lib.ERR_BOUNDS


# ---- UASTC runs -----------------------------------------------------------------------------------------------------------------------
def uastc_file(dims, pads, sizes=None):
    blocks = [np.zeros((x * y, 16), dtype=np.uint8) for x, y in dims]
    if sizes:
        blocks = [np.zeros(n, dtype=np.uint8) for n in sizes]
    return bb.uastc_file(blocks, dims, pads=pads)


def align256(v):
    return (v + 255) // 256 * 256


def test_runs_of_the_mixed_file(layout):
    """the file of test_gpu_parity.py: runs {0,1,2}, {3,4} behind a 7-byte gap, {5} behind a 16-byte gap, an empty slice, a 40-slice array"""
    dims = [(40, 30), (20, 15), (10, 8), (64, 64), (32, 32), (5, 3), (0, 0)] + [(32, 32)] * 40
    pads = [0, 0, 0, 7, 0, 16, 0] + [0] * 40
    got = layout("runs", _lib.READ_BC7, file=uastc_file(dims, pads))
    data0 = 77 + 23 * 47
    b = [16 * x * y for x, y in dims]
    r0, r1, r2, r4 = sum(b[:3]), sum(b[3:5]), b[5], sum(b[7:])
    assert (r0, r1, r2, r4) == (25280, 81920, 240, 655360)
    at1, at2, at3 = align256(r0), align256(r0) + r1, align256(r0) + r1 + 256
    assert got["runs"] == [[0, 2, 0, data0, r0], [3, 4, at1, data0 + r0 + 7, r1], [5, 5, at2, data0 + r0 + 7 + r1 + 16, r2],
                           [6, 6, at3, data0 + r0 + r1 + r2 + 23, 0], [7, 46, at3, data0 + r0 + r1 + r2 + 23, r4]]
    assert got["total_in"] == at3 + r4
    # inside a run the slices are staged back to back
    want_off = [0, b[0], b[0] + b[1], at1, at1 + b[3], at2, at3] + [at3 + i * 16384 for i in range(40)]
    assert got["in_off"] == want_off


def test_a_zero_size_slice_breaks_a_run(layout):
    """three slices back to back in the file, the middle one empty: three runs, although every file offset continues the last"""
    got = layout("runs", _lib.READ_ETC1, file=uastc_file([(4, 4), (0, 0), (4, 4)], None))
    data0 = 77 + 23 * 3
    assert got["runs"] == [[0, 0, 0, data0, 256], [1, 1, 256, data0 + 256, 0], [2, 2, 256, data0 + 256, 256]]
    assert got["total_in"] == 512


def test_a_slice_of_no_whole_blocks_breaks_a_run(layout):
    """a slice of 250 bytes between two of 256, back to back: no run takes it or follows it.  Only BU_READ_UASTC plans such a file (every
    other target refuses it, uastc.rs:54-59), so that is the plan the layout is asked about."""
    f = uastc_file([(4, 4), (4, 4), (4, 4), (4, 4)], None, sizes=[256, 250, 256, 256])
    data0 = 77 + 23 * 4
    got = layout("runs", _lib.READ_UASTC, file=f)
    assert got["runs"] == [[0, 0, 0, data0, 256], [1, 1, 256, data0 + 256, 250], [2, 3, 512, data0 + 506, 512]]
    assert got["in_off"] == [0, 256, 512, 768] and got["total_in"] == 1024


# ---- pieces ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("run_mib, piece_mib, pieced", [(7, 4, False), (8, 4, True), (16, 4, True), (63, 15, True), (64, 16, True), (65, 16, True)])
def test_piece_size_at_the_edges(layout, run_mib, piece_mib, pieced):
    """a quarter of the run in whole MiB, between 4 and 16 MiB; pieced from two pieces on"""
    assert layout("piece", run_mib * MIB, _lib.READ_BC7, 1) == dict(piece=piece_mib * MIB, pieced=int(pieced))
    assert layout("piece", run_mib * MIB - 16, _lib.READ_BC7, 1) == dict(piece=max(4, min(16, (run_mib * MIB - 16) // 4 // MIB)) * MIB,
                                                                        pieced=int(pieced and run_mib != 8))
    # never for RGBA32 (one launch per image) and never without a mapped output
    assert layout("piece", run_mib * MIB, _lib.READ_RGBA, 1)["pieced"] == 0
    assert layout("piece", run_mib * MIB, _lib.READ_BC7, 0)["pieced"] == 0


def test_fixed_piece_size(layout):
    """BU_RUN_PIECE_MIB: 0 switches the pieces off, 1 cuts every run of 2 MiB and more"""
    for run in (MIB, 2 * MIB - 16, 2 * MIB, 65 * MIB):
        assert layout("piece", run, _lib.READ_ETC2, 1, 0) == dict(piece=0, pieced=0)
        assert layout("piece", run, _lib.READ_ETC2, 1, 1) == dict(piece=MIB, pieced=int(run >= 2 * MIB))
        assert layout("piece", run, _lib.READ_RGBA, 1, 1)["pieced"] == 0 and layout("piece", run, _lib.READ_ETC2, 0, 1)["pieced"] == 0


# ---- the aux buffer ---------------------------------------------------------------------------------------------------------------------
AUX_SLACK = 512


@pytest.mark.parametrize("align", [16, 256])
@pytest.mark.parametrize("sizes", [[1], [255, 256, 257], [4000, 8000, 24, 128], [0, 0, 0, 0], [7, 0, 9], [0, 100], [100, 0], [1 << 33, 3, 1 << 20, 17], []],
                         ids=lambda s: "-".join(map(str, s)) or "none")
def test_aux_regions_are_aligned_ordered_and_disjoint(layout, sizes, align):
    got = layout("aux", align, *sizes)
    off = got["off"]
    assert got["slack"] == AUX_SLACK and len(off) == len(sizes)
    assert all(o % align == 0 for o in off) and (not off or off[0] == 0)
    rounded = [(s + align - 1) // align * align for s in sizes]
    for i in range(1, len(off)):
        # ordered, and a region ends where the next begins or before: strictly ordered wherever the region in front holds a byte
        assert off[i] >= off[i - 1] + sizes[i - 1] and (off[i] > off[i - 1] or sizes[i - 1] == 0)
        assert off[i] == off[i - 1] + rounded[i - 1]
    assert got["total"] == sum(rounded) + AUX_SLACK
    assert not off or off[-1] + sizes[-1] <= got["total"] - AUX_SLACK


# what the four drivers ask for, against the sums they used to write out inline (a + b: bu_align256(a) + bu_align256(b), as plain numbers)
AUX_SHAPES = {
    # 1000 codebook entries, 3 images, 4 descriptors of 32 bytes: 4 n, 8 n, 8 per image, the table
    "streamed ETC1S": (256, [4000, 8000, 24, 128], [0, 4096, 4096 + 8192, 4096 + 8192 + 256], 4096 + 8192 + 256 + 256),
    # 300 endpoints of 4 bytes, 300 selectors of 8, 40 images, 41 descriptors
    "one-launch ETC1S": (256, [1200, 2400, 320, 1312], [0, 1280, 1280 + 2560, 1280 + 2560 + 512], 1280 + 2560 + 512 + 1536),
    # 47 images, 257 CRC registers of 2 bytes
    "UASTC runs": (256, [376, 514], [0, 512], 512 + 768),
    # the slice-level ETC1S calls round to 16: 37 endpoints, 21 selectors, 65 alpha indices -- or none
    "ETC1S slice with alpha": (16, [148, 168, 260], [0, 160, 160 + 176], 160 + 176 + 272),
    "ETC1S slice": (16, [148, 168, 0], [0, 160, 160 + 176], 160 + 176),
}


@pytest.mark.parametrize("name", list(AUX_SHAPES))
def test_aux_offsets_of_the_drivers_are_the_inline_sums(layout, name):
    align, sizes, off, regions = AUX_SHAPES[name]
    assert layout("aux", align, *sizes) == dict(slack=AUX_SLACK, off=off, total=regions + AUX_SLACK)


# ---- the CRC fold -----------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def crc_file():
    """a UASTC file of one slice of 4 x 64 KiB + 4000 bytes of noise; its payload starts at 77, its slice data at 100"""
    data = np.random.default_rng(5).integers(0, 256, 4 * PIECE + 4000, dtype=np.uint8)
    f = bb.uastc_file([data], [(1, 1)])
    assert len(f) == 100 + data.size and bb.crc16(f[77:]) == int.from_bytes(f[12:14], "little")
    return f


FOLDS = {  # name -> (segments, byte positions of every class: in a piece, in a tail, between / around the segments)
    "whole pieces": ([(100, 3 * PIECE)], [100, 100 + PIECE - 1, 100 + PIECE, 100 + 3 * PIECE - 1, 77, 99, 100 + 3 * PIECE, -1]),
    "pieces and a tail": ([(100, 2 * PIECE + 777)], [100, 100 + 2 * PIECE - 1, 100 + 2 * PIECE, 100 + 2 * PIECE + 776, 100 + 2 * PIECE + 777, 78, -1]),
    "two segments with a gap": ([(1000 + 2 * PIECE, PIECE + 5), (200, PIECE)], [200, 199, 200 + PIECE - 1, 200 + PIECE, 999 + 2 * PIECE, 1000 + 2 * PIECE,
                                                                                  1000 + 3 * PIECE, 1004 + 3 * PIECE, 1005 + 3 * PIECE, -1]),
    "shorter than a piece": ([(5000, PIECE - 1)], [4999, 5000, 5000 + PIECE - 2, 5000 + PIECE - 1, 77, -1]),
    "whole payload": ([(77, 4 * PIECE + 4023)], [77, 77 + 4 * PIECE - 1, 77 + 4 * PIECE, -1]),
    "nothing uploaded": ([], [77, 30000, -1]),
}


@pytest.mark.parametrize("name", list(FOLDS))
def test_crc_fold_is_the_plain_crc(layout, crc_file, name):
    segs, positions = FOLDS[name]
    args = ["%d:%d" % s for s in segs]
    assert layout("fold", *args, file=crc_file) == dict(ok=1, folded=1, host=1)
    for pos in positions:
        g = bytearray(crc_file)
        g[pos] ^= 0x20
        assert layout("fold", *args, file=bytes(g)) == dict(ok=0, folded=1, host=0), pos


@pytest.mark.parametrize("segs", [[(100, 2 * PIECE), (100 + PIECE, 2 * PIECE)], [(100, PIECE), (100, PIECE)], [(60, PIECE)], [(100, 5 * PIECE)],
                                  [(100 + 4 * PIECE, 4001)], [(1 << 40, PIECE)]],
                         ids=["overlap", "twice", "into the header", "past the end", "one byte past the end", "far away"])
def test_segments_that_cannot_be_folded_take_the_host_crc(layout, crc_file, segs):
    args = ["%d:%d" % s for s in segs]
    assert layout("fold", *args, file=crc_file) == dict(ok=1, folded=0, host=1)
    g = bytearray(crc_file)
    g[100 + PIECE + 3] ^= 1
    assert layout("fold", *args, file=bytes(g)) == dict(ok=0, folded=0, host=0)
