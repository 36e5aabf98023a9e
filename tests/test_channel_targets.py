"""UASTC -> BC4 / BC5 / EAC R11 / EAC RG11 on the CPU: the numpy model of tests/channel_model.py against spec decoders, the host build of
the device headers against the model, the launch plan of the new targets, and the ABI values.

The model is written from the rules of DESIGN.md section 4.4; its input is the block's RGBA32 decode by the oracle (oracle/bu_oracle.c),
so neither side of the comparison borrows the kernel's own unpack."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

import channel_model as cm
from basisu_rs_amd import _lib, synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST_EMUL = os.path.join(ROOT, "tests", "host_emul")
CSRC = os.path.join(ROOT, "basisu_rs_amd", "csrc")
NAMES = ("bc4", "bc5", "r11", "rg11")
MINE_K = 48  # blocks per mined edge class


# ---- input sets --------------------------------------------------------------------------------------------------------------
def _mode8_code():
    codes = [c for c in range(128) if synth._mode_lut()[c] == 8]
    return codes[0]


def solid_blocks():
    """mode-8 (solid colour) blocks: R = 0..255 with A = 255 - R, and R = A = v"""
    code = _mode8_code()
    out = []
    for v in range(256):
        for r, g, b, a in ((v, 17, 200, 255 - v), (v, v, v, v)):
            w = code | (r << 5) | (g << 13) | (b << 21) | (a << 29)
            out.append(np.frombuffer(int(w).to_bytes(16, "little"), dtype=np.uint8))
    return np.stack(out)


def dense_modes(golden, per_mode=256, seed=5):
    """every mode densely: a reference vector's mode byte, random bits behind it, pattern fields brought into range"""
    rng = np.random.default_rng(seed)
    modes = synth.block_modes(golden["uastc"])
    rows = []
    for m in range(19):
        src = golden["uastc"][modes == m]
        pick = src[rng.integers(0, src.shape[0], size=per_mode)]
        noise = rng.integers(0, 256, size=pick.shape, dtype=np.uint8)
        noise[:, 0] = (pick[:, 0] & 0x7F) | (noise[:, 0] & 0x80)
        rows.append(noise)
    return synth._fix_pattern_fields(np.concatenate(rows))


def rgba_of(oracle, blocks):
    st, _, rgba = oracle.decode_to_rgba(np.ascontiguousarray(blocks).tobytes(), 1)
    assert st == 0
    return rgba.reshape(-1, 64)


def edge_classes(rgba):
    """per block, the edge classes of both channels: BC4 spans d = 1, 2, 13, 14, 15, 255; R11 targets at 0 / 2047, a multiplier clamped at 15,
    two tables tied for the smallest error"""
    cls = {}
    for c in (0, 3):
        v = cm.channel(rgba, c)
        d = v.max(1) - v.min(1)
        for dv in (1, 2, 13, 14, 15, 255):
            cls["d%d_c%d" % (dv, c)] = d == dv
        t = cm.r11_targets(v)
        cls["t0_c%d" % c] = (t.min(1) == 0) & (d > 0)
        cls["t2047_c%d" % c] = (t.max(1) == 2047) & (d > 0)
        span = (t.max(1) - t.min(1))[:, None]
        cls["mult15_c%d" % c] = (-(-span // (8 * cm.EAC_RANGE[None, :])) > 15).any(1)
        _, _, _, _, _, err, solid = cm.r11_fields(v)
        best = err.min(1, keepdims=True)
        cls["tie_c%d" % c] = ((err == best).sum(1) >= 2) & ~solid
    return cls


def mined_set(oracle, n_pool=60000, seed=11):
    """blocks of the random and high-contrast pools that reach each edge class, MINE_K per class"""
    pool = np.concatenate([synth.atlas_rand(n_pool, seed=seed), synth.atlas_contrast(n_pool, seed=seed + 1)])
    cls = edge_classes(rgba_of(oracle, pool))
    pick = set()
    for name, hit in cls.items():
        idx = np.nonzero(hit)[0]
        assert idx.size > 0, "no block of the pool reaches edge class %s" % name
        pick.update(idx[:MINE_K].tolist())
    return pool[sorted(pick)], cls


def cpu_sets(golden, oracle):
    mined, _ = mined_set(oracle)
    return {
        "reference": golden["uastc"],
        "rand": synth.atlas_rand(8192, seed=3),
        "contrast": synth.atlas_contrast(8192, seed=4),
        "dense": dense_modes(golden),
        "solid": solid_blocks(),
        "mined": mined,
    }


@pytest.fixture(scope="module")
def sets(golden, oracle):
    return {k: (np.ascontiguousarray(b), rgba_of(oracle, b)) for k, b in cpu_sets(golden, oracle).items()}


# ---- the model against spec decoders -------------------------------------------------------------------------------------------
def test_spec_decoders_read_hand_made_blocks():
    # BC4, 8-value mode: r0 = 200, r1 = 100; texel 0 code 0, texel 1 code 1, texel 2 code 2 (= (6*200 + 100)/7), texel 15 code 7
    bits = 0 | (1 << 3) | (2 << 6) | (7 << 45)
    blk = np.array([[200, 100] + list(bits.to_bytes(6, "little"))], dtype=np.uint8)
    num, den = cm.bc4_decode(blk)
    assert den[0] == 7 and num[0, 0] == 1400 and num[0, 1] == 700 and num[0, 2] == 1300 and num[0, 15] == 200 + 6 * 100
    # 6-value mode (r0 <= r1): codes 6 and 7 are 0 and 255
    bits = (6 << 0) | (7 << 3)
    num, den = cm.bc4_decode(np.array([[10, 20] + list(bits.to_bytes(6, "little"))], dtype=np.uint8))
    assert den[0] == 5 and num[0, 0] == 0 and num[0, 1] == 5 * 255
    # R11: base 100, mult 2, table 0 (-3 -6 -9 -15 2 5 8 14); pixel id 0 = (0, 0) j = 3, id 1 = (0, 1) j = 7, id 4 = (1, 0) j = 4
    sel = (3 << 45) | (7 << 42) | (4 << 33)
    blk = np.array([[100, (2 << 4) | 0] + list(sel.to_bytes(6, "big"))], dtype=np.uint8)
    v = cm.r11_decode(blk)[0]
    assert v[0] == 804 - 16 * 15 and v[4] == 804 + 16 * 14 and v[1] == 804 + 16 * 2 and v[5] == 804 - 16 * 3
    # multiplier 0: the modifier counts once; values clamp to 0..2047
    blk = np.array([[255, (0 << 4) | 13] + list((7 << 45).to_bytes(6, "big"))], dtype=np.uint8)
    v = cm.r11_decode(blk)[0]
    assert v[0] == 2047 and v[1] == 2044 - 1  # (texel 1 = pixel id 4: j = 0, modifier -1)
    blk = np.array([[0, (15 << 4) | 0] + list((3 << 45).to_bytes(6, "big"))], dtype=np.uint8)
    assert cm.r11_decode(blk)[0, 0] == 0


@pytest.mark.parametrize("c", [0, 3])
def test_bc4_model_within_d_over_14(sets, c):
    for name, (_, rgba) in sets.items():
        v = cm.channel(rgba, c)
        blk = cm.bc4_encode(v)
        num, den = cm.bc4_decode(blk)
        d = (v.max(1) - v.min(1))[:, None]
        assert (np.abs(14 * num - 14 * v * den[:, None]) <= d * den[:, None]).all(), name
        solid = d[:, 0] == 0
        assert (num[solid] == v[solid] * den[solid, None]).all(), name
        assert (blk[:, 0] >= blk[:, 1]).all()


@pytest.mark.parametrize("c", [0, 3])
def test_r11_model_against_the_spec_decoder(sets, c):
    seen_tie = 0
    for name, (_, rgba) in sets.items():
        v = cm.channel(rgba, c)
        t = cm.r11_targets(v)
        base, mult, table, _, chosen, _, solid = cm.r11_fields(v)
        blk = cm.r11_encode(v)
        dec = cm.r11_decode(blk)
        assert (dec == chosen).all(), name
        assert (np.abs(dec[solid] - t[solid]) <= 1).all(), name
        ns = np.nonzero(~solid)[0]
        if ns.size == 0:
            continue
        tn = t[ns]
        sse = ((dec[ns] - tn) ** 2).sum(1)
        mn, mx = tn.min(1), tn.max(1)
        for k in range(16):  # every other table rebuilt by the rule and decoded: none beats the chosen one, ties go to the lower k
            mk = np.minimum(15, -(-(mx - mn) // (8 * cm.EAC_RANGE[k])))
            bk = np.minimum(255, (mn + mx + 8 * mk) // 16)
            sk = ((cm.r11_decode(cm.r11_block(bk, mk, np.full(ns.size, k), tn)) - tn) ** 2).sum(1)
            assert (sk >= sse).all(), (name, k)
            assert (sk[table[ns] > k] > sse[table[ns] > k]).all(), (name, k)
            seen_tie += int(((sk == sse) & (table[ns] < k)).sum())
    assert seen_tie > 0, "no block with two tables of equal error"


def test_two_channel_blocks_are_the_concatenation(sets):
    for _, rgba in sets.values():
        assert (cm.encode("bc5", rgba) == np.concatenate([cm.bc4_encode(cm.channel(rgba, 0)), cm.bc4_encode(cm.channel(rgba, 3))], 1)).all()
        assert (cm.encode("rg11", rgba) == np.concatenate([cm.r11_encode(cm.channel(rgba, 0)), cm.r11_encode(cm.channel(rgba, 3))], 1)).all()


def test_mined_set_reaches_every_edge_class(oracle):
    blocks, _ = mined_set(oracle)
    cls = edge_classes(rgba_of(oracle, blocks))
    for name, hit in cls.items():
        assert hit.sum() >= 1, name
    # a block without alpha: Y is a solid 255 (2047) block
    rgb = solid_blocks()[0:1].copy()
    rgba = rgba_of(oracle, rgb)
    rgba[:, 3::4] = 255
    assert cm.encode("bc5", rgba)[0, 8:].tolist() == [255, 255, 0, 0, 0, 0, 0, 0]
    assert cm.r11_decode(cm.encode("rg11", rgba)[:, 8:]).tolist() == [[2047] * 16]


# ---- the host build of the device headers against the model ------------------------------------------------------------------
def test_host_build_equals_the_model(sets, tmp_path):
    """tests/host_emul/bu_emul_channels.cpp, built with the flags of tests/host_emul/Makefile's UBSan target and run once over every set
    in a child process (an UBSan report aborts it: a test failure), then compared with the model bit for bit"""
    so = tmp_path / "libbu_emul_channels_ubsan.so"
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fPIC", "-shared", "-fsanitize=undefined", "-fno-sanitize-recover=undefined", "-Wall",
                    "-Wno-unknown-pragmas", "-I" + CSRC, "-o", str(so), os.path.join(HOST_EMUL, "bu_emul_channels.cpp")], check=True)
    inp = tmp_path / "in.npz"
    np.savez(inp, **{k: b for k, (b, _) in sets.items()})
    outp = tmp_path / "out.npz"
    code = r"""
import ctypes, numpy as np
lib = ctypes.CDLL(%r)
lib.bu_emul_channels_batch.argtypes = [ctypes.c_int, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_void_p]
lib.bu_emul_channels_batch.restype = ctypes.c_int
sets = np.load(%r)
res = {}
for k in sets.files:
    b = np.ascontiguousarray(sets[k])
    for name, (t, bb) in %r.items():
        out = np.zeros((b.shape[0], bb), dtype=np.uint8)
        st = np.zeros(b.shape[0], dtype=np.uint8)
        assert lib.bu_emul_channels_batch(t, b.ctypes.data, b.shape[0], out.ctypes.data, st.ctypes.data) == 0
        res[k + "/" + name], res[k + "/" + name + "/st"] = out, st
o = np.zeros((1, 8), dtype=np.uint8)
s = np.zeros(1, dtype=np.uint8)
assert lib.bu_emul_channels_batch(4, b.ctypes.data, 1, o.ctypes.data, s.ctypes.data) == -1
np.savez(%r, **res)
print("clean")
""" % (str(so), str(inp), cm.CHANNEL_TARGETS, str(outp))
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0 and "clean" in r.stdout, r.stderr[-2000:]
    res = np.load(outp)
    for k, (_, rgba) in sets.items():
        for name in NAMES:
            assert (res[k + "/" + name + "/st"] == 0).all()
            got, want = res[k + "/" + name], cm.encode(name, rgba)
            bad = np.nonzero((got != want).any(1))[0]
            assert bad.size == 0, "%s / %s: %d blocks differ, first %d: %s vs %s" % (k, name, bad.size, bad[0], got[bad[0]], want[bad[0]])


def test_host_build_reports_invalid_blocks(golden, tmp_path):
    so = tmp_path / "libbu_emul_channels.so"
    subprocess.run(["g++", "-std=c++17", "-O2", "-fPIC", "-shared", "-Wall", "-Wno-unknown-pragmas", "-I" + CSRC, "-o", str(so),
                    os.path.join(HOST_EMUL, "bu_emul_channels.cpp")], check=True)
    lib = ctypes.CDLL(str(so))
    lib.bu_emul_channels_batch.argtypes = [ctypes.c_int, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_void_p]
    b = np.ascontiguousarray(synth.atlas_err(golden["uastc"], 64, [3, 40]))
    for name, (t, bb) in cm.CHANNEL_TARGETS.items():
        out = np.full((64, bb), 0xAB, dtype=np.uint8)
        st = np.zeros(64, dtype=np.uint8)
        lib.bu_emul_channels_batch(t, b.ctypes.data, 64, out.ctypes.data, st.ctypes.data)
        assert st[3] != 0 and st[40] != 0 and (np.delete(st, [3, 40]) == 0).all(), name
        assert (out[[3, 40]] == 0).all(), name


# ---- launch plan --------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def plan_lib():
    subprocess.run(["make", "-C", HOST_EMUL, "libbu_emul.so"], check=True, capture_output=True)
    lib = ctypes.CDLL(os.path.join(HOST_EMUL, "libbu_emul.so"))
    I64P = ctypes.POINTER(ctypes.c_int64)
    U64P = ctypes.POINTER(ctypes.c_uint64)
    lib.bu_emul_launch_plan.argtypes = [ctypes.c_int, ctypes.c_size_t, ctypes.c_size_t, ctypes.c_uint, ctypes.c_int, ctypes.c_int, ctypes.c_uint, I64P,
                                        ctypes.c_size_t, ctypes.POINTER(ctypes.c_int)]
    lib.bu_emul_launch_plan.restype = ctypes.c_size_t
    lib.bu_emul_runs_plan.argtypes = [ctypes.c_int, ctypes.c_size_t, U64P, U64P, ctypes.POINTER(ctypes.c_size_t), U64P, ctypes.c_size_t, ctypes.c_int,
                                      ctypes.c_int, ctypes.c_uint, I64P, ctypes.c_size_t, I64P, ctypes.c_size_t]
    lib.bu_emul_runs_plan.restype = ctypes.c_size_t
    return lib


def _slice_plan(lib, t, n, bpr, grid_cap, policy, auto, cu):
    cap = 256
    rows = (ctypes.c_int64 * (15 * cap))()
    needs = ctypes.c_int(0)
    k = lib.bu_emul_launch_plan(t, n, bpr, grid_cap, policy, auto, cu, rows, cap, ctypes.byref(needs))
    assert k <= cap
    return [rows[15 * i:15 * i + 15] for i in range(k)]


SIZES = [1, 7, 8, 1000, 1024 * 256, 1024 * 256 + 1, 3 * 1024 * 256, 3 * 1024 * 256 + 1, (1 << 20) - 1, 1 << 20, (1 << 20) + 4321, 5 << 20, (1 << 26) + 3]


@pytest.mark.parametrize("target", [6, 7, 8, 9])
def test_slice_plan_covers_every_block_once(plan_lib, target):
    etc = 2 if target in (6, 8) else 3  # the ETC target whose shapes it takes
    for cu in (256, 80):
        for n in SIZES:
            for bpr in (0, 1, 1024, 4096):
                for grid_cap in (0, 64):
                    for policy, auto in ((0, 0), (1, 1), (2, 0), (2, 1), (2, 3)):
                        plan = _slice_plan(plan_lib, target, n, bpr, grid_cap, policy, auto, cu)
                        ref = _slice_plan(plan_lib, etc, n, bpr, grid_cap, policy, auto, cu)
                        covered = 0
                        for r in plan:
                            assert r[0] == covered and r[1] > 0
                            covered += r[1]
                            assert r[14] == 0, "no tile tickets for the channel targets"
                        assert covered == n
                        # the same shape, grid and arguments as the ETC target, in the channel target's own kernel
                        assert len(plan) == len(ref)
                        for a, b in zip(plan, ref):
                            assert a[:2] == b[:2] and a[3:] == b[3:]
                            assert (a[2] < 0) == (b[2] < 0)
                            assert a[2] < 0 or a[2] >= 34  # (the existing 34 sorted kernels keep their numbers)


@pytest.mark.parametrize("target", [6, 7, 8, 9])
def test_runs_plan_covers_every_block_once(plan_lib, target):
    I64P = ctypes.POINTER(ctypes.c_int64)
    rng = np.random.default_rng(target)
    for trial in range(40):
        n_runs = int(rng.integers(2, 200))
        sizes = rng.choice([1, 9, 1000, 2047, 4096, 70001, 1 << 19, (1 << 20) + 7], size=n_runs)
        in_addr = (ctypes.c_uint64 * n_runs)(*[(1 << 40) + (i << 32) for i in range(n_runs)])
        out_addr = (ctypes.c_uint64 * n_runs)(*[(2 << 40) + (i << 32) for i in range(n_runs)])
        nb = (ctypes.c_size_t * n_runs)(*[int(s) for s in sizes])
        base = (ctypes.c_uint64 * n_runs)(*[0] * n_runs)
        cap, ecap = 64, 4096
        rows = (ctypes.c_int64 * (10 * cap))()
        ents = (ctypes.c_int64 * (5 * ecap))()
        policy = int(rng.integers(0, 3))
        k = plan_lib.bu_emul_runs_plan(target, n_runs, in_addr, out_addr, nb, base, 0, policy, int(rng.integers(0, 2)), 256,
                                       ctypes.cast(rows, I64P), cap, ctypes.cast(ents, I64P), ecap)
        assert k > 0
        seen = np.zeros(n_runs, dtype=np.int64)
        for j in range(k):
            r = rows[10 * j:10 * j + 10]
            if r[0] >= 0:
                seen[r[0]] += sizes[r[0]]
                continue
            assert r[8] in (0, 1) and r[5] in (0, 1, 3)  # (no whole-rectangle kernel for these targets)
            tiles = 0
            for e in range(r[9], r[9] + r[1]):
                run, off, n, _, first = ents[5 * e:5 * e + 5]
                assert off == seen[run] and first == tiles
                seen[run] += n
                tiles += -(-n // r[3])
            assert tiles == r[2]
        assert (seen == sizes).all()


# ---- ABI ----------------------------------------------------------------------------------------------------------------------
def test_abi_values():
    lib = _lib.load()
    # (5 names no target, as before the channel targets existed; 10 is past the end)
    assert [lib.bu_target_block_bytes(t) for t in range(11)] == [16, 16, 8, 16, 64, 0, 8, 16, 8, 16, 0]
    assert (_lib.BC4_R, _lib.BC5_RG, _lib.EAC_R11, _lib.EAC_RG11) == (6, 7, 8, 9)
    assert all(_lib.BLOCK_BYTES[t] == lib.bu_target_block_bytes(t) for t in _lib.BLOCK_BYTES) and 5 not in _lib.BLOCK_BYTES
    assert (_lib.READ_BC4, _lib.READ_BC5, _lib.READ_EAC_R11, _lib.READ_EAC_RG11) == (6, 7, 8, 9)
    from basisu_rs_amd import TargetTextureFormat as F

    assert (int(F.Bc4R), int(F.Bc5Rg), int(F.EacR11), int(F.EacRg11)) == (6, 7, 8, 9)
    hdr = open(os.path.join(ROOT, "include", "basisu_hip.h")).read()
    for name, v in (("BU_TARGET_BC4_R", 6), ("BU_TARGET_BC5_RG", 7), ("BU_TARGET_EAC_R11", 8), ("BU_TARGET_EAC_RG11", 9), ("BU_READ_BC4", 6),
                    ("BU_READ_BC5", 7), ("BU_READ_EAC_R11", 8), ("BU_READ_EAC_RG11", 9)):
        assert "%s = %d" % (name, v) in hdr
    ffi = open(os.path.join(ROOT, "rust", "src", "ffi.rs")).read()
    for name, v in (("BU_TARGET_BC4_R", 6), ("BU_TARGET_EAC_RG11", 9), ("BU_READ_BC4", 6), ("BU_READ_EAC_RG11", 9)):
        assert "pub const %s: c_int = %d;" % (name, v) in ffi


def test_read_query_of_the_new_targets(golden):
    """host-only: image sizes of a UASTC file, BU_ERR_ARGUMENT for target 10 and for an ETC1S file"""
    from basisu_rs_amd import read_query, write_uastc_file

    blocks = golden["uastc"][:48]
    f = write_uastc_file([dict(data=blocks[:32].tobytes(), orig_w=32, orig_h=16, nbx=8, nby=4),
                          dict(data=blocks[32:].tobytes(), orig_w=16, orig_h=16, nbx=4, nby=4, image_index=1)])
    for t, bb in ((_lib.READ_BC4, 8), (_lib.READ_BC5, 16), (_lib.READ_EAC_R11, 8), (_lib.READ_EAC_RG11, 16)):
        assert read_query(t, f) == (2, 48 * bb)
    lib = _lib.load()
    a = np.frombuffer(f, dtype=np.uint8)
    n, nb = ctypes.c_size_t(0), ctypes.c_size_t(0)
    assert lib.bu_read_query(10, a.ctypes.data, a.size, ctypes.byref(n), ctypes.byref(nb)) == _lib.ERR_ARGUMENT
    import basis_builder as bb

    e, _, _ = bb.etc1s_file(np.random.default_rng(1), [(4, 4)], n_codebook=32)
    d = np.frombuffer(e, dtype=np.uint8)
    assert lib.bu_read_query(_lib.READ_ETC1, d.ctypes.data, d.size, ctypes.byref(n), ctypes.byref(nb)) == 0
    for t in (_lib.READ_BC4, _lib.READ_BC5, _lib.READ_EAC_R11, _lib.READ_EAC_RG11):
        assert lib.bu_read_query(t, d.ctypes.data, d.size, ctypes.byref(n), ctypes.byref(nb)) == _lib.ERR_ARGUMENT

