"""UASTC -> BC1 / BC3 on the CPU: the numpy model of tests/colour_model.py against a spec decoder and properties that do not lean on the
model's own steps, the host build of the device headers against the model, the launch plan of the colour targets, and the ABI values.

The model is written from the rule of DESIGN.md section 4.5; its input is the block's RGBA32 decode by the oracle (oracle/bu_oracle.c),
so neither side of the comparison borrows the kernel's own unpack."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import channel_model as cm
import colour_model as col
import test_channel_targets as tct
from basisu_rs_amd import _lib, synth
from test_channel_targets import plan_lib  # noqa: F401  (the fixture)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST_EMUL = os.path.join(ROOT, "tests", "host_emul")
CSRC = os.path.join(ROOT, "basisu_rs_amd", "csrc")
NAMES = ("bc1", "bc3")
MINE_K = 48  # blocks per mined edge class
CLASSES = ("det0", "kept", "rejected", "swap", "eq", "tie_hl", "tie_sel", "sh", "anti")


# ---- input sets --------------------------------------------------------------------------------------------------------------
def mined_set(oracle, n_pool=60000, seed=21):
    """blocks of the random and high-contrast pools that reach each edge class of the rule, MINE_K per class"""
    pool = np.concatenate([synth.atlas_rand(n_pool, seed=seed), synth.atlas_contrast(n_pool, seed=seed + 1)])
    f = col.fields(tct.rgba_of(oracle, pool))
    pick = set()
    for name in CLASSES:
        idx = np.nonzero(f[name])[0]
        assert idx.size > 0, "no block of the pool reaches edge class %s" % name
        pick.update(idx[:MINE_K].tolist())
    return pool[sorted(pick)]


def cpu_sets(golden, oracle):
    return {
        "reference": golden["uastc"],
        "rand": synth.atlas_rand(8192, seed=13),
        "contrast": synth.atlas_contrast(8192, seed=14),
        "dense": tct.dense_modes(golden),
        "solid": tct.solid_blocks(),
        "mined": mined_set(oracle),
    }


@pytest.fixture(scope="module")
def sets(golden, oracle):
    return {k: (np.ascontiguousarray(b), tct.rgba_of(oracle, b)) for k, b in cpu_sets(golden, oracle).items()}


def _decode_thirds(blk):
    """BC1 blocks -> colours x 3 [n, 16, 3] (float: exact for the four-colour mode, halves for the three-colour mode), opaque mask"""
    num, den, opaque = col.bc1_decode(blk)
    return 3.0 * num / den[:, None, None], opaque


def _bbox_error(x):
    """squared error in thirds of bounding-box corners (q(max), q(min) per channel) with the same nearest-point selectors"""
    c0, c1 = col.quant(x.max(1)), col.quant(x.min(1))
    _, E, _ = col.selectors(x, col.expand(c0), col.expand(c1))
    return E


# ---- the spec decoder and properties -------------------------------------------------------------------------------------------
def test_spec_decoder_reads_hand_made_blocks():
    # four-colour mode: c0 = (31, 63, 31) white, c1 = 0 black; texel 0 index 0, 1 index 1, 2 index 2, 3 index 3
    blk = np.array([[0xFF, 0xFF, 0x00, 0x00, 0b11100100, 0, 0, 0]], dtype=np.uint8)
    num, den, opaque = col.bc1_decode(blk)
    assert den[0] == 3 and opaque.all()
    assert num[0, 0].tolist() == [765] * 3 and num[0, 1].tolist() == [0] * 3 and num[0, 2].tolist() == [510] * 3 and num[0, 3].tolist() == [255] * 3
    # bit replication: r5 = 16 -> 132, g6 = 32 -> 130, b5 = 1 -> 8
    w = (16 << 11) | (32 << 5) | 1
    blk = np.array([[w & 0xFF, w >> 8, 0, 0, 0, 0, 0, 0]], dtype=np.uint8)
    num, den, _ = col.bc1_decode(blk)
    assert (num[0, 0] // 3).tolist() == [132, 130, 8]
    # three-colour mode (color0 <= color1): index 2 is the midpoint, index 3 transparent black
    w0, w1 = (4 << 11), (8 << 11) | (2 << 5)
    blk = np.array([[w0 & 0xFF, w0 >> 8, w1 & 0xFF, w1 >> 8, 0b11100100, 0, 0, 0]], dtype=np.uint8)
    num, den, opaque = col.bc1_decode(blk)
    assert den[0] == 2 and opaque[0].tolist() == [True, True, True, False] + [True] * 12
    assert num[0, 0].tolist() == [2 * 33, 0, 0] and num[0, 1].tolist() == [2 * 66, 2 * 8, 0]
    assert num[0, 2].tolist() == [33 + 66, 8, 0] and num[0, 3].tolist() == [0, 0, 0]
    # equal words are the three-colour mode too
    blk = np.array([[0x34, 0x12, 0x34, 0x12, 0, 0, 0, 0]], dtype=np.uint8)
    assert col.bc1_decode(blk)[1][0] == 2


def test_solid_tables_are_the_generated_ones():
    """tools/gen_tables.py's BU_BC1_OM5 / OM6 (in the generated header the kernels read) equal the model's own exhaustive search"""
    hdr = open(os.path.join(CSRC, "bu_tables.h")).read()
    for name, om in (("BU_BC1_OM5", col.OM5), ("BU_BC1_OM6", col.OM6)):
        body = re.search(name + r"\[256\] = \{(.*?)\};", hdr, re.S).group(1)
        vals = [int(t, 16) for t in re.findall(r"0x[0-9A-F]+", body)]
        assert vals == [int(a) | (int(b) << 8) for a, b in om], name


def _palette(blk):
    """the four palette points of each block in thirds [n, 4, 3] (the block's words with every index set to k)"""
    out = []
    for k, byte in enumerate((0x00, 0x55, 0xAA, 0xFF)):
        b = blk.copy()
        b[:, 4:] = byte
        out.append(_decode_thirds(b)[0][:, 0, :])
    return np.stack(out, 1)


def test_indices_are_nearest_palette_points(sets):
    """every texel takes a nearest opaque point of the spec palette (three-colour mode, w0 == w1: index 3 is transparent, not a candidate)"""
    for name, (_, rgba) in sets.items():
        x = col.rgb_of(rgba)
        blk = col.bc1_encode(rgba)
        dec, opaque = _decode_thirds(blk)
        assert opaque.all(), name
        four = col.bc1_decode(blk)[1] == 3
        dist = ((3 * x[:, :, None, :] - _palette(blk)[:, None, :, :]) ** 2).sum(-1)  # [n, 16, 4]
        dist = np.where(four[:, None, None] | (np.arange(4) < 3)[None, None, :], dist, np.inf)
        assert (((3 * x - dec) ** 2).sum(-1) <= dist.min(-1)).all(), name


def test_endpoint_order(sets):
    for name, (_, rgba) in sets.items():
        blk = col.bc1_encode(rgba).astype(np.int64)
        w0, w1 = blk[:, 0] | blk[:, 1] << 8, blk[:, 2] | blk[:, 3] << 8
        idx = blk[:, 4] | blk[:, 5] << 8 | blk[:, 6] << 16 | blk[:, 7] << 24
        assert ((w0 > w1) | ((w0 == w1) & (idx == 0))).all(), name


def test_solid_error_is_optimal():
    """every solid value 0..255 in every channel: the decoded error equals the best thirds point over all 5- or 6-bit pairs"""
    v = np.arange(256)
    rgba = np.zeros((256, 16, 4), dtype=np.uint8)
    rgba[:, :, 0], rgba[:, :, 1], rgba[:, :, 2], rgba[:, :, 3] = v[:, None], v[:, None], (255 - v)[:, None], 255
    dec, opaque = _decode_thirds(col.bc1_encode(rgba.reshape(-1, 64)))
    assert opaque.all()
    x = rgba[:, 0, :3].astype(np.int64)
    for c, bits in ((0, 5), (1, 6), (2, 5)):
        n = 1 << bits
        e = np.array([(a << (8 - bits)) | (a >> (2 * bits - 8)) for a in range(n)])
        pts = np.concatenate([(2 * e[:, None] + e[None, :]).ravel(), 3 * e])  # every point the block could decode to, in thirds
        best = np.abs(pts[None, :] - 3 * x[:, c:c + 1]).min(1)
        assert (np.abs(dec[:, 0, c] - 3 * x[:, c]) == best).all(), c
        assert (dec[:, :, c] == dec[:, :1, c]).all()


def test_psnr_at_least_bounding_box(sets):
    _, rgba = sets["dense"]
    x = col.rgb_of(rgba)
    dec, _ = _decode_thirds(col.bc1_encode(rgba))
    ours = ((3 * x - dec) ** 2).sum()
    bbox = _bbox_error(x).sum()
    psnr = lambda e: 10 * np.log10(255.0 ** 2 / (e / 9.0 / x.size))
    assert psnr(ours) >= psnr(bbox), (psnr(ours), psnr(bbox))


def test_bc3_is_bc4_of_alpha_then_bc1(sets):
    for _, rgba in sets.values():
        want = np.concatenate([cm.bc4_encode(cm.channel(rgba, 3)), col.bc1_encode(rgba)], 1)
        assert (col.encode("bc3", rgba) == want).all()
        assert (col.encode("bc1", rgba) == want[:, 8:]).all()


def test_mined_set_reaches_every_edge_class(oracle):
    f = col.fields(tct.rgba_of(oracle, mined_set(oracle)))
    for name in CLASSES:
        assert f[name].sum() >= 1, name


# ---- the host build of the device headers against the model ------------------------------------------------------------------
def test_host_build_equals_the_model(sets, tmp_path):
    """tests/host_emul/bu_emul_colour.cpp, built with the flags of tests/host_emul/Makefile's UBSan target and run once over every set in
    a child process (an UBSan report aborts it: a test failure), then compared with the model bit for bit"""
    so = tmp_path / "libbu_emul_colour_ubsan.so"
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fPIC", "-shared", "-fsanitize=undefined", "-fno-sanitize-recover=undefined", "-Wall",
                    "-Wno-unknown-pragmas", "-I" + CSRC, "-o", str(so), os.path.join(HOST_EMUL, "bu_emul_colour.cpp")], check=True)
    inp = tmp_path / "in.npz"
    np.savez(inp, **{k: b for k, (b, _) in sets.items()})
    outp = tmp_path / "out.npz"
    code = r"""
import ctypes, numpy as np
lib = ctypes.CDLL(%r)
lib.bu_emul_colour_batch.argtypes = [ctypes.c_int, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_void_p]
lib.bu_emul_colour_batch.restype = ctypes.c_int
sets = np.load(%r)
res = {}
for k in sets.files:
    b = np.ascontiguousarray(sets[k])
    for name, (t, bb) in %r.items():
        out = np.zeros((b.shape[0], bb), dtype=np.uint8)
        st = np.zeros(b.shape[0], dtype=np.uint8)
        assert lib.bu_emul_colour_batch(t, b.ctypes.data, b.shape[0], out.ctypes.data, st.ctypes.data) == 0
        res[k + "/" + name], res[k + "/" + name + "/st"] = out, st
o = np.zeros((1, 16), dtype=np.uint8)
s = np.zeros(1, dtype=np.uint8)
for t in (4, 9, 10, 13):
    assert lib.bu_emul_colour_batch(t, b.ctypes.data, 1, o.ctypes.data, s.ctypes.data) == -1
np.savez(%r, **res)
print("clean")
""" % (str(so), str(inp), col.COLOUR_TARGETS, str(outp))
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0 and "clean" in r.stdout, r.stderr[-2000:]
    res = np.load(outp)
    for k, (_, rgba) in sets.items():
        for name in NAMES:
            assert (res[k + "/" + name + "/st"] == 0).all()
            got, want = res[k + "/" + name], col.encode(name, rgba)
            bad = np.nonzero((got != want).any(1))[0]
            assert bad.size == 0, "%s / %s: %d blocks differ, first %d: %s vs %s" % (k, name, bad.size, bad[0], got[bad[0]], want[bad[0]])


def test_host_build_reports_invalid_blocks(golden, tmp_path):
    so = tmp_path / "libbu_emul_colour.so"
    subprocess.run(["g++", "-std=c++17", "-O2", "-fPIC", "-shared", "-Wall", "-Wno-unknown-pragmas", "-I" + CSRC, "-o", str(so),
                    os.path.join(HOST_EMUL, "bu_emul_colour.cpp")], check=True)
    lib = ctypes.CDLL(str(so))
    lib.bu_emul_colour_batch.argtypes = [ctypes.c_int, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_void_p]
    b = np.ascontiguousarray(synth.atlas_err(golden["uastc"], 64, [3, 40]))
    for name, (t, bb) in col.COLOUR_TARGETS.items():
        out = np.full((64, bb), 0xAB, dtype=np.uint8)
        st = np.zeros(64, dtype=np.uint8)
        lib.bu_emul_colour_batch(t, b.ctypes.data, 64, out.ctypes.data, st.ctypes.data)
        assert st[3] != 0 and st[40] != 0 and (np.delete(st, [3, 40]) == 0).all(), name
        assert (out[[3, 40]] == 0).all(), name


# ---- launch plan --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("target", [11, 12])
def test_slice_plan_covers_every_block_once(plan_lib, target):  # noqa: F811
    etc = 2 if target == 11 else 3  # the ETC target whose shapes it takes
    for cu in (256, 80):
        for n in tct.SIZES:
            for bpr in (0, 1, 1024, 4096):
                for grid_cap in (0, 64):
                    for policy, auto in ((0, 0), (1, 1), (2, 0), (2, 1), (2, 3)):
                        plan = tct._slice_plan(plan_lib, target, n, bpr, grid_cap, policy, auto, cu)
                        ref = tct._slice_plan(plan_lib, etc, n, bpr, grid_cap, policy, auto, cu)
                        covered = 0
                        for r in plan:
                            assert r[0] == covered and r[1] > 0
                            covered += r[1]
                            assert r[14] == 0, "no tile tickets for the colour targets"
                        assert covered == n
                        assert len(plan) == len(ref)
                        for a, b in zip(plan, ref):
                            assert a[:2] == b[:2] and a[3:] == b[3:]
                            assert (a[2] < 0) == (b[2] < 0)
                            assert a[2] < 0 or a[2] >= 62  # (the existing 62 sorted kernels keep their numbers)


@pytest.mark.parametrize("target", [11, 12])
def test_runs_plan_covers_every_block_once(plan_lib, target):  # noqa: F811
    tct.test_runs_plan_covers_every_block_once(plan_lib, target)  # (the channel targets' check: ETC-family runs tables, every block once)


# ---- ABI ----------------------------------------------------------------------------------------------------------------------
def test_abi_values():
    lib = _lib.load()
    # (5 and 10 name no target; 13 is past the end)
    assert [lib.bu_target_block_bytes(t) for t in range(14)] == [16, 16, 8, 16, 64, 0, 8, 16, 8, 16, 0, 8, 16, 0]
    assert (_lib.BC1_RGB, _lib.BC3_RGBA) == (11, 12)
    assert all(_lib.BLOCK_BYTES[t] == lib.bu_target_block_bytes(t) for t in _lib.BLOCK_BYTES) and 10 not in _lib.BLOCK_BYTES
    assert (_lib.READ_BC1, _lib.READ_BC3) == (11, 12)
    from basisu_rs_amd import TargetTextureFormat as F

    assert (int(F.Bc1Rgb), int(F.Bc3Rgba)) == (11, 12)
    hdr = open(os.path.join(ROOT, "include", "basisu_hip.h")).read()
    for name, v in (("BU_TARGET_BC1_RGB", 11), ("BU_TARGET_BC3_RGBA", 12), ("BU_READ_BC1", 11), ("BU_READ_BC3", 12)):
        assert "%s = %d" % (name, v) in hdr
    ffi = open(os.path.join(ROOT, "rust", "src", "ffi.rs")).read()
    for name, v in (("BU_TARGET_BC1_RGB", 11), ("BU_TARGET_BC3_RGBA", 12), ("BU_READ_BC1", 11), ("BU_READ_BC3", 12)):
        assert "pub const %s: c_int = %d;" % (name, v) in ffi


def test_read_query_of_the_colour_targets(golden):
    """host-only: image sizes of a UASTC file, BU_ERR_ARGUMENT for targets 10 and 13 and for an ETC1S file"""
    from basisu_rs_amd import read_query, write_uastc_file

    blocks = golden["uastc"][:48]
    f = write_uastc_file([dict(data=blocks[:32].tobytes(), orig_w=32, orig_h=16, nbx=8, nby=4),
                          dict(data=blocks[32:].tobytes(), orig_w=16, orig_h=16, nbx=4, nby=4, image_index=1)])
    for t, bb in ((_lib.READ_BC1, 8), (_lib.READ_BC3, 16)):
        assert read_query(t, f) == (2, 48 * bb)
    lib = _lib.load()
    a = np.frombuffer(f, dtype=np.uint8)
    n, nb = ctypes.c_size_t(0), ctypes.c_size_t(0)
    for t in (10, 13):
        assert lib.bu_read_query(t, a.ctypes.data, a.size, ctypes.byref(n), ctypes.byref(nb)) == _lib.ERR_ARGUMENT
    import basis_builder as bb

    e, _, _ = bb.etc1s_file(np.random.default_rng(1), [(4, 4)], n_codebook=32)
    d = np.frombuffer(e, dtype=np.uint8)
    assert lib.bu_read_query(_lib.READ_ETC1, d.ctypes.data, d.size, ctypes.byref(n), ctypes.byref(nb)) == 0
    for t in (_lib.READ_BC1, _lib.READ_BC3):
        assert lib.bu_read_query(t, d.ctypes.data, d.size, ctypes.byref(n), ctypes.byref(nb)) == _lib.ERR_ARGUMENT
