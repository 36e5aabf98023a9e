"""ETC1S -> BC1, BC3, BC4, BC5, EAC R11 and EAC RG11 on the CPU: the host build of the palette-form encoders (bu_etc1s_targets.hpp,
DESIGN.md section 4.6) against the numpy models of tests/colour_model.py and tests/channel_model.py, applied to the oracle's RGBA32
decode of the same blocks (oracle/bu_oracle.c), so neither side of the comparison borrows the kernel's own palette or masks.  The ETC1
and RGBA32 blocks and the index check of the same header, which every ETC1S kernel shares, are compared with the oracle directly.

Three sets: every palette word of one channel under every non-empty set of used selectors (BC4, R11), random blocks for every target,
and a mined set that reaches every edge class of the BC1 rule a palette can take."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

import channel_model as cm
import colour_model as col

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST_EMUL = os.path.join(ROOT, "tests", "host_emul")
CSRC = os.path.join(ROOT, "basisu_rs_amd", "csrc")
# name -> (bu_target, bytes per block)
TARGETS = {"bc1": (11, 8), "bc3": (12, 16), "bc4": (6, 8), "bc5": (7, 16), "r11": (8, 8), "rg11": (9, 16)}
BASE = {"etc1": (2, 8), "rgba": (4, 64)}  # the two targets of the ETC1S back end that the oracle itself writes
N_RANDOM = 200_000
CHUNK = 32768  # blocks per oracle call: a codebook entry per block and per slice, indices below 2^16
MINE_K = 64
BC1_CLASSES = ("solid_one", "solid_dup", "eq", "swap", "det0", "kept", "rejected")


def model(name, rgba):
    """the target's blocks from the RGBA32 decode (the colour or the channel model)"""
    return col.encode(name, rgba) if name in ("bc1", "bc3") else cm.encode(name, rgba)


def endpoint(r5, g5, b5, inten):
    return (np.asarray(r5, np.uint32) | np.asarray(g5, np.uint32) << 8 | np.asarray(b5, np.uint32) << 16
            | np.asarray(inten, np.uint32) << 24).astype(np.uint32)


def rgba_of(oracle, ep, rows, aep=None, arows=None):
    """the oracle's RGBA32 decode [n, 64] of blocks given as one endpoint word and one rows word each (a codebook entry per block)"""
    n = ep.size
    sel = np.zeros((2 * n, 8), dtype=np.uint8)
    sel[:n, :4] = rows.astype("<u4").view(np.uint8).reshape(n, 4)
    idx = (np.arange(n, dtype=np.uint32) | (np.arange(n, dtype=np.uint32) << 16)).astype(np.uint32)
    aidx = None
    endpoints = np.concatenate([ep, np.zeros(n, np.uint32)])
    if aep is not None:
        endpoints[n:] = aep
        sel[n:, :4] = arows.astype("<u4").view(np.uint8).reshape(n, 4)
        aidx = ((np.arange(n, dtype=np.uint32) + n) | ((np.arange(n, dtype=np.uint32) + n) << 16)).astype(np.uint32)
    return oracle.etc1s_to_rgba(idx, aidx, 1, n, endpoints, sel).reshape(n, 64)


def rows_from(rng, n, subsets=True):
    """random rows; with `subsets`, each block draws its texels from a random non-empty set of selectors"""
    if not subsets:
        return rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)
    mask = rng.integers(1, 16, n)
    pick = rng.integers(0, 4, (n, 16))
    ok = (mask[:, None] >> pick) & 1
    for _ in range(8):  # redraw texels whose selector is outside the set
        pick = np.where(ok == 1, pick, rng.integers(0, 4, (n, 16)))
        ok = (mask[:, None] >> pick) & 1
    first = np.array([0] + [[s for s in range(4) if (m >> s) & 1][0] for m in range(1, 16)])[mask]
    pick = np.where(ok == 1, pick, first[:, None])
    return (pick.astype(np.uint64) << (2 * np.arange(16, dtype=np.uint64))).sum(1).astype(np.uint32)


def random_endpoints(rng, n, extreme=False):
    if extreme:  # 5-bit values at or near the ends, large intensities: clamped duplicate palette entries
        c = rng.choice(np.array([0, 1, 30, 31]), (n, 3))
        inten = rng.integers(4, 8, n)
    else:
        c = rng.integers(0, 32, (n, 3))
        inten = rng.integers(0, 8, n)
    return endpoint(c[:, 0], c[:, 1], c[:, 2], inten)


def random_set(n, seed):
    rng = np.random.default_rng(seed)
    h = n // 2
    ep = np.concatenate([random_endpoints(rng, h), random_endpoints(rng, n - h, extreme=True)])
    rows = np.concatenate([rows_from(rng, h, subsets=False), rows_from(rng, n - h)])
    aep = np.concatenate([random_endpoints(rng, n - h), random_endpoints(rng, h, extreme=True)])
    arows = np.concatenate([rows_from(rng, n - h), rows_from(rng, h, subsets=False)])
    return ep, rows, aep, arows


def exhaustive_set():
    """all 256 palette words (c5, inten: R = G = B) x all 15 non-empty sets of used selectors x four count patterns"""
    pats = []
    for m in range(1, 16):
        u = [s for s in range(4) if (m >> s) & 1]
        k = len(u)
        mine = [[u[i % k] for i in range(16)],                         # round robin
                [u[min(i, k - 1)] for i in range(16)],                 # one texel each, the rest the last
                [u[k - 1 - min(i, k - 1)] for i in range(16)][::-1],   # the same, reversed
                [u[(i * k) // 16] for i in range(16)][::-1]]           # runs of 16 / k
        for p in mine:  # every pattern uses exactly its set
            assert sorted(set(p)) == u
        pats += mine
    pats = np.array(pats, dtype=np.uint64)
    rows = (pats << (2 * np.arange(16, dtype=np.uint64))).sum(1).astype(np.uint32)
    c5, inten = np.meshgrid(np.arange(32), np.arange(8), indexing="ij")
    eps = endpoint(c5.ravel(), c5.ravel(), c5.ravel(), inten.ravel())
    ep = np.repeat(eps, rows.size)
    rr = np.tile(rows, eps.size)
    return ep, rr


def used_count(rows):
    r = rows.astype(np.int64)
    sel = (r[:, None] >> (2 * np.arange(16))) & 3
    return np.stack([(sel == s).any(1) for s in range(4)], -1).sum(1)


def bc1_classes(rgba, rows):
    """the edge classes of the BC1 rule an ETC1S block can reach.  Every channel of an ETC1S palette is non-decreasing in the selector,
    so H >= L channel by channel and a block that is not solid never swaps its endpoints: the swap comes from the solid tables"""
    f = col.fields(rgba)
    k = used_count(rows)
    v = col.rgb_of(rgba)[:, 0, :]
    sa = np.stack([col.OM5[v[:, 0], 0], col.OM6[v[:, 1], 0], col.OM5[v[:, 2], 0]], -1)
    sb = np.stack([col.OM5[v[:, 0], 1], col.OM6[v[:, 1], 1], col.OM5[v[:, 2], 1]], -1)
    swap = f["swap"] | (f["solid"] & (col.word(sa) < col.word(sb)))
    return {"solid_one": f["solid"] & (k == 1), "solid_dup": f["solid"] & (k > 1), "eq": f["eq"], "swap": swap,
            "det0": f["det0"], "kept": f["kept"], "rejected": f["rejected"]}


def mined_set(oracle, n_pool=60000, seed=31):
    """blocks of a pool with few used selectors and extreme endpoints that reach each edge class of the BC1 rule, MINE_K per class"""
    rng = np.random.default_rng(seed)
    third = n_pool // 3
    c = rng.integers(0, 32, (third, 3))  # the smallest intensities: neighbouring entries that quantise alike (w0 == w1, det = 0)
    small = endpoint(c[:, 0], c[:, 1], c[:, 2], rng.integers(0, 2, third))
    ep = np.concatenate([random_endpoints(rng, third, extreme=True), small, random_endpoints(rng, n_pool - 2 * third)])
    rows = rows_from(rng, n_pool)
    f = bc1_classes(rgba_of(oracle, ep, rows), rows)
    pick = set()
    for name in BC1_CLASSES:
        idx = np.nonzero(f[name])[0]
        assert idx.size > 0, "no block of the pool reaches edge class %s" % name
        pick.update(idx[:MINE_K].tolist())
    pick = np.array(sorted(pick))
    return ep[pick], rows[pick]


# ---- the host build -----------------------------------------------------------------------------------------------------------
def _build(tmp_path, ubsan):
    so = tmp_path / ("libbu_emul_etc1s%s.so" % ("_ubsan" if ubsan else ""))
    flags = ["-O1", "-g", "-fsanitize=undefined", "-fno-sanitize-recover=undefined"] if ubsan else ["-O2"]
    subprocess.run(["g++", "-std=c++17"] + flags + ["-fPIC", "-shared", "-Wall", "-Wno-unknown-pragmas", "-I" + CSRC, "-o", str(so),
                    os.path.join(HOST_EMUL, "bu_emul_etc1s.cpp")], check=True)
    return so


_CHILD = r"""
import ctypes, numpy as np
lib = ctypes.CDLL(%r)
lib.bu_emul_etc1s_batch.argtypes = [ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p]
lib.bu_emul_etc1s_batch.restype = ctypes.c_int
sets = np.load(%r)
res = {}
for k in sorted({f.split("/")[0] for f in sets.files}):
    ep, rows = sets[k + "/ep"], sets[k + "/rows"]
    alpha = (k + "/aep") in sets.files
    aep, arows = (sets[k + "/aep"], sets[k + "/arows"]) if alpha else (None, None)
    for name, (t, bb) in %r.items():
        out = np.zeros((ep.size, bb), dtype=np.uint8)
        sel = sets[k + "/sely"] if name == "etc1" else rows  # the word of the selector entry the target reads
        assert lib.bu_emul_etc1s_batch(t, ep.ctypes.data, sel.ctypes.data, None if aep is None else aep.ctypes.data,
                                       None if arows is None else arows.ctypes.data, ep.size, out.ctypes.data) == 0
        res[k + "/" + name] = out
o = np.zeros((1, 16), dtype=np.uint8)
for t in (0, 1, 3, 5, 10, 13):
    assert lib.bu_emul_etc1s_batch(t, ep.ctypes.data, rows.ctypes.data, None, None, 1, o.ctypes.data) == -1
np.savez(%r, **res)
print("clean")
"""


def run_host_build(so, tmp_path, sets, targets=TARGETS, sely=None):
    """sets: name -> (ep, rows, aep, arows) with aep / arows None for no alpha slice; run in a child process (an UBSan report aborts it).
    sely: name -> the second word of each block's selector entry, for the ETC1 target"""
    inp, outp = tmp_path / "in.npz", tmp_path / "out.npz"
    arrays = {}
    for k, (ep, rows, aep, arows) in sets.items():
        arrays[k + "/ep"], arrays[k + "/rows"] = ep, rows
        if aep is not None:
            arrays[k + "/aep"], arrays[k + "/arows"] = aep, arows
        if sely is not None:
            arrays[k + "/sely"] = sely[k]
    np.savez(inp, **arrays)
    r = subprocess.run([sys.executable, "-c", _CHILD % (str(so), str(inp), targets, str(outp))], capture_output=True, text=True, timeout=1200)
    assert r.returncode == 0 and "clean" in r.stdout, r.stderr[-2000:]
    return np.load(outp)


def check(res, oracle, sets, names):
    for k, (ep, rows, aep, arows) in sets.items():
        for name in names:
            got = res[k + "/" + name]
            for c0 in range(0, ep.size, CHUNK):
                sl = slice(c0, c0 + CHUNK)
                rgba = rgba_of(oracle, ep[sl], rows[sl], None if aep is None else aep[sl], None if arows is None else arows[sl])
                want = model(name, rgba)
                bad = np.nonzero((got[sl] != want).any(1))[0]
                assert bad.size == 0, "%s / %s: %d blocks differ, first %d: %s vs %s (ep %08x rows %08x)" % (
                    k, name, bad.size, c0 + bad[0], got[sl][bad[0]], want[bad[0]], ep[sl][bad[0]], rows[sl][bad[0]])


@pytest.fixture(scope="module")
def ubsan_so(tmp_path_factory):
    return _build(tmp_path_factory.mktemp("etc1s_emul"), ubsan=True)


@pytest.fixture(scope="module")
def plain_so(tmp_path_factory):
    return _build(tmp_path_factory.mktemp("etc1s_emul_plain"), ubsan=False)


@pytest.fixture(params=["plain", "ubsan"])
def either_so(request, plain_so, ubsan_so):
    return plain_so if request.param == "plain" else ubsan_so


def check_base(so, tmp_path, oracle, sets):
    """ETC1 and RGBA32 of the host build against the oracle's own, byte for byte.  A codebook entry per block: the selector entries are
    the oracle's (selectors_from_rows: rows, then the ETC1 selector bytes), so ETC1 reads a real second word"""
    entries = {k: oracle.selectors_from_rows(v[1].astype("<u4").view(np.uint8).reshape(-1, 4)) for k, v in sets.items()}
    sely = {k: np.ascontiguousarray(e[:, 4:]).view("<u4").reshape(-1).astype(np.uint32) for k, e in entries.items()}
    res = run_host_build(so, tmp_path, sets, targets=BASE, sely=sely)
    for k, (ep, rows, aep, arows) in sets.items():
        for c0 in range(0, ep.size, CHUNK):
            sl = slice(c0, c0 + CHUNK)
            n = ep[sl].size
            idx = (np.arange(n, dtype=np.uint32) | (np.arange(n, dtype=np.uint32) << 16)).astype(np.uint32)
            assert (entries[k][sl][:, :4] == rows[sl].astype("<u4").view(np.uint8).reshape(n, 4)).all()
            want = {"etc1": oracle.etc1s_to_etc1(idx, ep[sl], entries[k][sl]).reshape(n, 8),
                    "rgba": rgba_of(oracle, ep[sl], rows[sl], None if aep is None else aep[sl], None if arows is None else arows[sl])}
            for name in BASE:
                got = res[k + "/" + name][sl]
                bad = np.nonzero((got != want[name]).any(1))[0]
                assert bad.size == 0, "%s / %s: %d blocks differ, first %d: %s vs %s (ep %08x rows %08x)" % (
                    k, name, bad.size, c0 + bad[0], got[bad[0]], want[name][bad[0]], ep[sl][bad[0]], rows[sl][bad[0]])


def test_exhaustive_palettes_etc1_rgba32(oracle, either_so, tmp_path):
    ep, rows = exhaustive_set()
    check_base(either_so, tmp_path, oracle, {"exhaustive": (ep, rows, None, None)})


def test_random_blocks_etc1_rgba32(oracle, either_so, tmp_path):
    ep, rows, aep, arows = random_set(N_RANDOM, seed=41)
    check_base(either_so, tmp_path, oracle, {"alpha": (ep, rows, aep, arows), "opaque": (ep[:CHUNK], rows[:CHUNK], None, None)})


def test_index_split_and_check(either_so):
    """bu_etc1s_index: the halves of both index words, and bad <=> some index the block reads lies outside its codebook"""
    lib = ctypes.CDLL(str(either_so))
    lib.bu_emul_etc1s_index.argtypes = [ctypes.c_uint32, ctypes.c_int, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_void_p]
    lib.bu_emul_etc1s_index.restype = None
    out = np.zeros(5, dtype=np.uint32)
    edge = (0, 1, 6, 7, 8, 0xFFFF)
    for n_ep, n_sel in ((7, 9), (1, 1), (0, 0), (65536, 65536)):
        for e in edge:
            for s in edge:
                for has_a, ae, as_ in [(0, 0xFFFF, 0xFFFF)] + [(1, x, y) for x in edge for y in edge]:
                    lib.bu_emul_etc1s_index(e | s << 16, has_a, ae | as_ << 16, n_ep, n_sel, out.ctypes.data)
                    bad = e >= n_ep or s >= n_sel or (has_a == 1 and (ae >= n_ep or as_ >= n_sel))
                    assert out.tolist() == [e, s, ae if has_a else 0, as_ if has_a else 0, int(bad)], (n_ep, n_sel, e, s, has_a, ae, as_)


def test_exhaustive_palettes_bc4_r11(oracle, ubsan_so, tmp_path):
    ep, rows = exhaustive_set()
    assert ep.size == 256 * 15 * 4
    assert set(used_count(rows).tolist()) == {1, 2, 3, 4}
    sets = {"exhaustive": (ep, rows, None, None)}
    check(run_host_build(ubsan_so, tmp_path, sets), oracle, sets, ("bc4", "r11"))


def test_random_blocks_every_target(oracle, ubsan_so, tmp_path):
    ep, rows, aep, arows = random_set(N_RANDOM, seed=41)
    sets = {"alpha": (ep, rows, aep, arows), "opaque": (ep[:CHUNK], rows[:CHUNK], None, None)}
    check(run_host_build(ubsan_so, tmp_path, sets), oracle, sets, tuple(TARGETS))


def test_mined_set_reaches_every_bc1_class(oracle):
    ep, rows = mined_set(oracle)
    f = bc1_classes(rgba_of(oracle, ep, rows), rows)
    for name in BC1_CLASSES:
        assert f[name].sum() >= 1, name


def test_mined_blocks_every_target(oracle, ubsan_so, tmp_path):
    ep, rows = mined_set(oracle)
    rng = np.random.default_rng(5)
    aep, arows = random_endpoints(rng, ep.size, extreme=True), rows_from(rng, ep.size)
    sets = {"mined": (ep, rows, None, None), "mined_a": (ep, rows, aep, arows), "mined_swap": (aep, arows, ep, rows)}
    check(run_host_build(ubsan_so, tmp_path, sets), oracle, sets, tuple(TARGETS))


def test_solid_alpha_constants(oracle, tmp_path):
    """a block without an alpha slice reads A = 255: the constant A halves equal the model of a solid 255 channel"""
    v = np.full((1, 16), 255, dtype=np.int64)
    so = _build(tmp_path, ubsan=False)
    lib = ctypes.CDLL(str(so))
    lib.bu_emul_etc1s_batch.argtypes = [ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t,
                                        ctypes.c_void_p]
    ep, rows = endpoint([3], [9], [27], [2]), np.array([0x1B1B1B1B], dtype=np.uint32)
    for name, enc in (("bc5", cm.bc4_encode), ("rg11", cm.r11_encode), ("bc3", cm.bc4_encode)):
        t, bb = TARGETS[name]
        out = np.zeros((1, bb), dtype=np.uint8)
        assert lib.bu_emul_etc1s_batch(t, ep.ctypes.data, rows.ctypes.data, None, None, 1, out.ctypes.data) == 0
        half = out[:, 8:] if name != "bc3" else out[:, :8]
        assert (half == enc(v)).all(), name
        assert (out == model(name, rgba_of(oracle, ep, rows))).all(), name
