"""The addresses of the multi-run kernels (csrc/bu_multi_addr.hpp), checked on the CPU through the test-only host build of that header
(tests/host_emul/bu_emul_multi_addr.cpp): every access of a tile is a wave-uniform 64-bit base -- the tile's corner block -- plus a 32-bit byte offset that
hangs on the lane and the run's width alone.  Against the formula the kernel used before, evaluated here in Python's integers:
    address of block l of tile d = run.in + 16 * run_idx(d, l),  run_idx = first + (l // 64) * width + l % 64  (strips: first + l)
and the descriptor the same-run fast path derives against the one the table look-up gives.

The second half reads the built library the way tests/test_multi_kernel_address_space.py does: in every bu_uastc_multi_kernel instantiation each streaming
block load and each write-through result store names an SGPR-pair base and a 32-bit VGPR offset."""
import ctypes
import importlib.util
import os
import random
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "basisu_rs_amd", "csrc")
SRC = os.path.join(ROOT, "tests", "host_emul", "bu_emul_multi_addr.cpp")
STRIPS = 0xFFFFFFFF
U64 = ctypes.POINTER(ctypes.c_uint64)
U32 = ctypes.POINTER(ctypes.c_uint32)


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    so = tmp_path_factory.mktemp("multi_addr") / "libbu_emul_multi_addr.so"
    subprocess.run(["g++", "-std=c++17", "-O2", "-fPIC", "-shared", "-Wall", "-Wno-unknown-pragmas", "-I" + CSRC, "-o", str(so), SRC], check=True)
    L = ctypes.CDLL(str(so))
    for f in ("bu_emul_multi_max_width", "bu_emul_multi_rgba_max_bpr", "bu_emul_multi_runs", "bu_emul_multi_strips"):
        getattr(L, f).restype = ctypes.c_uint32
    L.bu_emul_multi_lane_offs.argtypes = [ctypes.c_int, ctypes.c_uint32, ctypes.c_uint32, U64]
    L.bu_emul_multi_walk.argtypes = [ctypes.c_uint32] * 4 + [U64, U32, ctypes.c_uint32, U32, U64, U64]
    L.bu_emul_multi_rgba_offs.argtypes = [ctypes.c_uint32] * 4 + [U64]
    assert L.bu_emul_multi_strips() == STRIPS and L.bu_emul_multi_runs() == 96 and L.bu_emul_multi_max_width() == 1 << 20
    return L


def lane_offs(lib, whole, width, tile):
    o = np.zeros(tile, dtype=np.uint64)
    lib.bu_emul_multi_lane_offs(int(whole), width, tile, o.ctypes.data_as(U64))
    return [int(x) for x in o]


FIELDS = ("fast", "in", "out", "base", "first", "n", "width", "bx0", "run")


def walk(lib, runs, first_tile, tiles, tile=1024, out_bytes=16, rgba_bpr=0):
    """runs: [(in, out, base, n, vshift)]; -> (walked, fresh): per tile a dict of FIELDS, the cursor kept / thrown away"""
    k = len(runs)
    rw = np.array([w for r in runs for w in r], dtype=np.uint64)
    ft = np.full(k + 32, 0xFFFFFFFF, dtype=np.uint32)
    ft[:k] = first_tile
    ts = np.array(tiles, dtype=np.uint32)
    a, b = np.zeros(9 * len(tiles), dtype=np.uint64), np.zeros(9 * len(tiles), dtype=np.uint64)
    lib.bu_emul_multi_walk(tile, out_bytes, rgba_bpr, k, rw.ctypes.data_as(U64), ft.ctypes.data_as(U32), len(tiles), ts.ctypes.data_as(U32), a.ctypes.data_as(U64),
                           b.ctypes.data_as(U64))
    rows = lambda x: [dict(zip(FIELDS, (int(v) for v in x[9 * i:9 * i + 9]))) for i in range(len(tiles))]
    return rows(a), rows(b)


def old_tile(run, lt, tile):
    """(first, n, width) of tile lt of a run, as the kernel's descriptor look-up computed them before"""
    _, _, _, n, vshift = run
    if vshift != STRIPS:
        width = 64 << vshift
        ty, tx = lt >> vshift, lt & ((1 << vshift) - 1)
        return (tile // 64) * ty * width + 64 * tx, tile, width
    first = lt * tile
    return first, min(tile, n - first), 0


def old_idx(first, width, l):
    return first + ((l // 64) * width + l % 64 if width else l)


def check_tile(lib, run, lt, d, tile=1024, out_bytes=16, offs_cache={}):
    first, n, width = old_tile(run, lt, tile)
    assert (d["first"], d["n"], d["width"], d["base"]) == (first, n, width, run[2])
    key = (width, tile)
    if key not in offs_cache:
        offs_cache[key] = lane_offs(lib, False, width, tile)
    offs = offs_cache[key]
    for l in range(n):
        assert offs[l] < 1 << 32
        idx = old_idx(first, width, l)
        assert idx < run[3]
        assert d["in"] + offs[l] == run[0] + 16 * idx, (run, lt, l)
        assert d["out"] + offs[l] * out_bytes // 16 == run[1] + out_bytes * idx, (run, lt, l)
        assert d["first"] + (offs[l] >> 4) == idx  # the status word's block number, less the run's base


def test_lane_offsets_of_every_width_fit_32_bits(lib):
    for tile in (1024, 2048):
        for k in range(15):  # widths 64 * 2^k up to 2^20
            width = 64 << k
            offs = lane_offs(lib, True, width, tile)
            assert offs == [((l // 64) * width + l % 64) * 16 for l in range(tile)]
            assert max(offs) < 1 << 32
            assert lane_offs(lib, False, width, tile) == offs
        assert lane_offs(lib, False, 0, tile) == [16 * l for l in range(tile)]
    assert 64 << 14 == lib.bu_emul_multi_max_width()


def test_rectangle_runs_of_every_width_up_to_2_32_blocks(lib):
    """start, middle and end of the largest run of each width that 32 bits hold; the runs sit high in the address space and on 16-byte alignment only"""
    for k in range(15):
        width = 64 << k
        n = ((1 << 32) - 1) // (16 * width) * (16 * width)
        for n_run in (n, 16 * width):
            run = (0x7F0000000010 + (k << 33), 0x7E0000000030 + (k << 33), (1 << 40) + k, n_run, k)
            nt = n_run // 1024
            tiles = sorted({0, 1, nt // 2, nt - 2, nt - 1} & set(range(nt)))
            walked, fresh = walk(lib, [run], [0], tiles)
            assert walked == [dict(f, fast=int(i > 0)) for i, f in enumerate(fresh)]
            for t, d in zip(tiles, walked):
                check_tile(lib, run, t, d)


@pytest.mark.parametrize("tile,out_bytes", [(1024, 16), (1024, 8), (2048, 8)])
def test_strip_runs_up_to_2_32_blocks(lib, tile, out_bytes):
    for n in ((1 << 32) - 1, (1 << 32) - tile, 5000, 1025, 1, tile):
        run = (0x7F1234567890, 0x7E0000000008, 77 << 32, n, STRIPS)
        nt = (n + tile - 1) // tile
        tiles = sorted({0, 1, nt // 2, nt - 2, nt - 1} & set(range(nt)))
        walked, fresh = walk(lib, [run], [0], tiles, tile, out_bytes)
        assert [w["fast"] for w in walked] == [0] + [1] * (len(tiles) - 1)
        for t, d, f in zip(tiles, walked, fresh):
            assert {**d, "fast": 0} == f
            check_tile(lib, run, t, d, tile, out_bytes)
        assert walked[-1]["n"] == n - (nt - 1) * tile  # the ragged last tile


def table_of_96():
    rnd = random.Random(96)
    runs, first, tiles = [], [], 0
    for i in range(96):
        if i % 4 == 3:
            vshift, n = STRIPS, rnd.choice((1, 700, 1024, 1025, 5000, 70001, 262143))
        else:
            vshift = rnd.choice((2, 3, 4, 4, 5, 14)) if i % 8 else 0
            n = 16 * (64 << vshift) * rnd.randint(1, 3)
        runs.append((0x7F0000000000 + (i << 34) + 16 * rnd.randrange(1 << 20), 0x7A0000000000 + (i << 34) + 16 * rnd.randrange(1 << 20), (i + 1) << 36, n, vshift))
        first.append(tiles)
        tiles += (n + 1023) // 1024
    return runs, first, tiles


def test_fast_path_equals_the_look_up_over_a_table_of_96_runs(lib):
    runs, first, n_tiles = table_of_96()
    assert len({r[4] for r in runs}) >= 6 and any(r[4] == STRIPS for r in runs)
    # every run's boundary in walking order -- the last tile of one run, then the first of the next --, a seeded random walk, and a fixed stride as a
    # persistent workgroup walks without tickets
    boundary = [t for f in first[1:] for t in (f - 1, f)]
    rnd = random.Random(7)
    for tiles in (boundary, [rnd.randrange(n_tiles) for _ in range(3000)], list(range(5, n_tiles, 1280)), list(range(n_tiles - 40, n_tiles))):
        walked, fresh = walk(lib, runs, first, tiles)
        prev = None
        for t, d, f in zip(tiles, walked, fresh):
            assert {**d, "fast": 0} == f, t
            r = max(i for i in range(96) if first[i] <= t)
            assert d["run"] == r
            assert d["fast"] == int(prev == r), (t, prev, r)  # the look-up runs exactly when the run changes
            prev = r
    walked, _ = walk(lib, runs, first, boundary)
    for t, d in zip(boundary, walked):
        check_tile(lib, runs[d["run"]], t - first[d["run"]], d)
    assert all(walked[i]["fast"] == 0 for i in range(1, len(boundary), 2))  # the first tile of a run, behind the last tile of the run before it


def test_rgba32_rows_from_the_corner(lib):
    """RGBA32: block idx of a run goes to pixel rows 4 * (idx // bpr) .. + 3 at column idx % bpr, 16 bytes per row"""
    tile = 1024
    for bpr, vshift, n in ((128, 1, 16 * 128 * 5), (1024, 4, 16 * 1024 * 3), (1000, STRIPS, 1000 * 37), (128, STRIPS, 128 * 7), (7, STRIPS, 7 * 1000), (1 << 24, STRIPS, 5000)):
        run = (0x7F0000000000, 0x7E0000000100, 0, n, vshift)
        nt = (n + tile - 1) // tile
        tiles = list(range(min(nt, 40)))
        walked, _ = walk(lib, [run], [0], tiles, tile, 16, bpr)
        for t, d in zip(tiles, walked):
            first, cnt, width = old_tile(run, t, tile)
            assert (d["first"], d["n"], d["width"]) == (first, cnt, width)
            off = np.zeros(tile, dtype=np.uint64)
            lib.bu_emul_multi_rgba_offs(width, d["bx0"], bpr, tile, off.ctypes.data_as(U64))
            for l in range(cnt):
                idx = old_idx(first, width, l)
                by, bx = divmod(idx, bpr)
                for r in (0, 3):
                    o = int(off[l]) + r * bpr * 16
                    assert o < 1 << 32
                    assert d["out"] + o == run[1] + ((4 * by + r) * bpr + bx) * 16, (bpr, t, l, r)
    assert lib.bu_emul_multi_rgba_max_bpr() == 1 << 24


def test_walk_under_ubsan(tmp_path):
    exe = tmp_path / "bu_emul_multi_addr"
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=undefined", "-fno-sanitize-recover=undefined", "-Wall", "-Wno-unknown-pragmas", "-DBU_EMUL_MULTI_ADDR_MAIN",
                    "-I" + CSRC, "-o", str(exe), SRC], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.startswith("clean 96 runs"), r.stdout + r.stderr


# ---- the built library ---------------------------------------------------------------------------------------------------------------
def _kernel_diff():
    spec = importlib.util.spec_from_file_location("kernel_diff", os.path.join(ROOT, "tools", "kernel_diff.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def multi_kernels():
    kd = _kernel_diff()
    if not kd.tools_present():
        pytest.skip("the LLVM tools that unbundle and read a gfx950 code object are not installed")
    from basisu_rs_amd import build

    ks = kd.kernels(build.LIB if os.path.exists(build.LIB) else build.build_hip())
    multi = {name: k for name, k in ks.items() if "bu_uastc_multi_kernel" in name}
    assert len(multi) >= 30, "the code object holds %d multi-run kernels" % len(multi)
    return multi


SCALAR_BASE = re.compile(r"^global_(load|store)_dwordx4 (v\[\d+:\d+\], v\d+|v\d+, v\[\d+:\d+\]), s\[\d+:\d+\]( offset:\d+)?( \w+)*$")


def test_every_streaming_access_names_a_scalar_base(multi_kernels):
    """each `global_load_dwordx4 ... nt` and each `global_store_dwordx4 ... sc1` of every multi-run kernel: an SGPR pair as the base, one VGPR as the offset, never `off`"""
    seen = 0
    for name, k in multi_kernels.items():
        loads = [ln for ln in k["code"] if ln.startswith("global_load_dwordx4") and ln.endswith(" nt")]
        stores = [ln for ln in k["code"] if ln.startswith("global_store_dwordx4") and " sc1" in ln]
        assert loads, name
        for ln in loads + stores:
            assert SCALAR_BASE.match(ln) and " off" not in ln.replace("offset", ""), (name, ln)
        seen += len(loads) + len(stores)
    assert seen >= 4 * len(multi_kernels)


WHOLE = ("bu_uastc_multi_kernelILi1ELi256ELi4ELb1ELb1EE", "bu_uastc_multi_kernelILi0ELi256ELi4ELb1ELb1EE")


def test_whole_tile_kernels_build_no_address_with_64_bit_multiply_adds(multi_kernels):
    """The headline (BC7) holds no v_mad_u64_u32 at all.  ASTC's block code itself holds four -- its trit packing, `x * 3 + y` with no 24-bit bound, which the
    one-slice ASTC kernels hold as well and which no address is made of --: there every v_mad_u64_u32 must be that one (multiplier 3, result read as an LDS index),
    and with every streaming access in the scalar-base form (the test above) none can feed an address."""
    for tid in WHOLE:
        (name,) = [n for n in multi_kernels if tid in n]
        code = multi_kernels[name]["code"]
        mads = [(i, ln) for i, ln in enumerate(code) if ln.startswith("v_mad_u64_u32")]
        if "ILi1E" in tid:
            assert not mads, (tid, mads[:4])
            continue
        assert len(mads) <= 4, (tid, len(mads))
        for i, ln in mads:
            m = re.match(r"v_mad_u64_u32 v\[(\d+):\d+\], s\[\d+:\d+\], v\d+, 3, v\[\d+:\d+\]$", ln)
            assert m, (tid, ln)
            assert re.match(r"ds_read_u8 v\d+, v%s offset:\d+$" % m.group(1), code[i + 1]), (tid, ln, code[i + 1])
