"""The files of tests/lz_shape_cases.py through both host decoders (no GPU).  Every expected index word is the ENCODER's record
(basis_builder.SliceSymbols.indices, written from basis_lz/mod.rs without calling a decoder); the oracle's decode and the product's are what is judged.
Which of the product's slice loops produced a result -- the fast loop, the exact loop behind a refusal, the two-thread form -- is read from the stand-alone
ASan / UBSan build of tests/host_emul/bu_hostlogic_asan.cpp, which also runs every case file under 300 rounds of bit flips."""
import os
import re
import subprocess

import numpy as np
import pytest

import basis_builder as bb
import basisu_rs_amd as bu
import lz_shape_cases as lz
from basisu_rs_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST_EMUL = os.path.join(ROOT, "tests", "host_emul")
DECODING = tuple(n for n in lz.NAMES if not lz.CASES[n].rejected)
REJECTED = tuple(n for n in lz.NAMES if lz.CASES[n].rejected)
ERR_BASISLZ = 18  # BU_ERR_BASISLZ (include/basisu_hip.h): any Err of basis_lz


def sections(f):
    h = bu.read_header(f)
    return (h, f[h.endpoint_cb_file_ofs:h.endpoint_cb_file_ofs + h.endpoint_cb_file_size], f[h.selector_cb_file_ofs:h.selector_cb_file_ofs + h.selector_cb_file_size],
            f[h.tables_file_ofs:h.tables_file_ofs + h.tables_file_size])


def oracle_slice(oracle, f, si):
    """-> (status, endpoints, selectors, index words) of the oracle's decode of slice si"""
    h, ecb, scb, tables = sections(f)
    s = bu.read_slice_descs(f, h)[si]
    st, oep, osel, oidx = oracle.lz_decode(ecb, scb, tables, h.total_selectors, h.total_selectors, h.tex_type == 3, f[s.file_ofs:s.file_ofs + s.file_size],
                                           s.num_blocks_x, s.num_blocks_y)
    return st, oep, osel, oidx[:, 0].astype(np.uint32) | (oidx[:, 1].astype(np.uint32) << 16)


def product_status(f, si):
    a = np.frombuffer(f, dtype=np.uint8)
    s = bu.read_slice_descs(f)[si]
    idx = np.zeros(max(s.num_blocks_x * s.num_blocks_y, 1), dtype=np.uint32)
    return _lib.load().bu_basislz_decode(a.ctypes.data, a.size, si, None, None, idx.ctypes.data)


def first_difference(got, want, stream, nbx):
    """for a failure message: the first block whose index word differs, and how many symbols and VLC fields the encoder had written before that block"""
    bad = int(np.nonzero(got != want)[0][0])
    return "block %d (x %d, y %d), behind %d symbols and VLC fields of the slice: got endpoint %d selector %d, the record has %d / %d; %d of %d blocks differ" % (
        bad, bad % nbx, bad // nbx, stream.op_start[bad], got[bad] & 0xFFFF, got[bad] >> 16, want[bad] & 0xFFFF, want[bad] >> 16, int((got != want).sum()),
        want.size)


# ---- a. both decoders give the record ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", DECODING)
def test_both_decoders_give_the_encoders_record(oracle, name):
    f, ep, rows, streams = lz.build(name)
    descs = bu.read_slice_descs(f)
    assert len(descs) == len(streams) and 2 <= len(descs) <= 4
    for si, (s, stream) in enumerate(zip(descs, streams)):
        assert s.num_blocks_x <= 40 and s.num_blocks_y <= 30
        want = bb.index_words(stream)
        st, oep, osel, oidx = oracle_slice(oracle, f, si)
        assert st == 0, (name, si, st)
        assert (oidx == want).all(), "oracle, %s slice %d: %s" % (name, si, first_difference(oidx, want, stream, s.num_blocks_x))
        pep, psel, pidx = bu.basislz_decode(f, si)
        assert (pidx == want).all(), "product, %s slice %d: %s" % (name, si, first_difference(pidx, want, stream, s.num_blocks_x))
        assert (pep == ep).all() and (oep == ep).all() and (psel[:, :4] == rows).all() and (osel[:, :4] == rows).all()


@pytest.mark.parametrize("name", REJECTED)
def test_over_subscribed_tables_are_refused_alike(oracle, name):
    """Kraft sum above 1: huffman.rs:176-178 refuses the table behind the symbol-order fill, whichever symbols still own entries"""
    f = lz.build(name)[0]
    for si in range(len(bu.read_slice_descs(f))):
        st = oracle_slice(oracle, f, si)[0]
        assert st == product_status(f, si) == ERR_BASISLZ, (name, si, st)


def test_run_state_does_not_cross_slices(oracle):
    """a selector run that ends on a slice's last block, and one with 40 blocks left over: the next slice starts with no run pending (mod.rs:223), so its
    first selector is the literal the script wrote, not history entry 0 -- in the record and in both decoders"""
    for name, pending in (("run_exact_end-opaque-hs32", 0), ("run_leftover-opaque-hs32", 40), ("run_exact_end-alpha-hs32", 0), ("run_leftover-alpha-hs32", 40)):
        f, _, _, streams = lz.build(name)
        for si, stream in enumerate(streams):
            assert stream.run_pending == pending
            first = int(stream.indices[0, 0, 1])
            assert first == lz.N_CODEBOOK - 1 != 0  # (history entry 0 holds 0 at this point: a pending run would give 0)
            assert oracle_slice(oracle, f, si)[3][0] >> 16 == first
            assert bu.basislz_decode(f, si)[2][0] >> 16 == first


def test_global_and_hybrid_selector_codebooks_are_refused_alike(oracle):
    """mod.rs:531-537: neither kind is implemented by the reference; the oracle and the product refuse both with one status"""
    f = lz.build("incomplete-pred")[0]
    h = bu.read_header(f)
    for bit in (0, 1):
        g = bytearray(f)
        g[h.selector_cb_file_ofs] |= 1 << bit
        g = bb.reseal(bytes(g))
        st = oracle_slice(oracle, g, 0)[0]
        assert st == product_status(g, 0) != 0, (bit, st)


# ---- b., c. which loop decoded the file; the same files under the sanitizers and bit flips ---------------------------------------------------
@pytest.fixture(scope="module")
def harness():
    subprocess.run(["make", "-C", HOST_EMUL, "bu_hostlogic_asan"], check=True, capture_output=True)
    return os.path.join(HOST_EMUL, "bu_hostlogic_asan")


@pytest.mark.parametrize("name", lz.NAMES)
def test_which_loop_decodes_the_file_and_bit_flips_under_asan(tmp_path, harness, name):
    case = lz.CASES[name]
    f, _, _, streams = lz.build(name)
    path = tmp_path / "t.basis"
    path.write_bytes(f)
    r = subprocess.run([harness, str(path), "300"], capture_output=True, text=True)
    if case.rejected:  # the pristine file does not parse: the harness says so and stops
        assert r.returncode == 3 and "codebooks and tables: status=%d" % ERR_BASISLZ in r.stdout, r.stdout + r.stderr[-3000:]
        return
    assert r.returncode == 0 and "fuzz done" in r.stdout, r.stdout + r.stderr[-3000:]
    loops = re.findall(r"^slice (\d+): decode_slice=(\w+) status=0$", r.stdout, re.M)
    split = re.findall(r"^slice (\d+): two-thread=([\w+-]+)$", r.stdout, re.M)
    assert [int(k) for k, _ in loops] == list(range(len(streams)))
    if case.refuse:  # an empty history_rle table: the fast loop refuses every slice, the two-thread form may not start
        assert {w for _, w in loops} == {"exact"} and "split_ok=0" in r.stdout and not split, r.stdout
    else:
        assert {w for _, w in loops} == {"fast"} and "split_ok=1" in r.stdout, r.stdout
        assert split == [(str(k), "lex+resolve") for k in range(len(streams))], r.stdout


# ---- e. every case is what its name says: a parser of the written table records, of this test's own -------------------------------------------
class Bits:
    def __init__(self, data):
        self.data, self.pos = data, 0

    def read(self, n):
        v = 0
        for k in range(n):
            byte = self.data[self.pos >> 3] if (self.pos >> 3) < len(self.data) else 0
            v |= ((byte >> (self.pos & 7)) & 1) << k
            self.pos += 1
        return v


def parse_table(r):
    """one Huffman table record (huffman.rs:43-118) -> dict(total_used, n_cl, cl_sizes[21], tokens [(symbol, extra)], sizes: every size the tokens give).
    The code-length codes are read bit by bit against the canonical code words, most significant bit first."""
    total_used, n_cl = r.read(14), r.read(5)
    order = [17, 18, 19, 20, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15, 16]
    cl = [0] * 21
    for k in range(n_cl):
        cl[order[k]] = r.read(3)
    words, code = {}, 0
    for ln in range(1, 8):
        for sym in range(21):
            if cl[sym] == ln:
                words[ln, code] = sym
                code += 1
        code <<= 1
    tokens, sizes = [], []
    while len(sizes) < total_used:
        ln, code = 0, 0
        while (ln, code) not in words:
            code = (code << 1) | r.read(1)
            ln += 1
            assert ln <= 7, "no code-length code matches"
        t = words[ln, code]
        extra = r.read({17: 3, 18: 7, 19: 2, 20: 7}.get(t, 0))
        tokens.append((t, extra))
        if t <= 16:
            sizes.append(t)
        elif t <= 18:
            sizes += [0] * (extra + (3 if t == 17 else 11))
        else:
            sizes += [sizes[-1]] * (extra + (3 if t == 19 else 7))
    return dict(total_used=total_used, n_cl=n_cl, cl_sizes=cl, tokens=tokens, sizes=sizes)


def parse_tables(f):
    """the four slice tables and the history size (mod.rs:77-83)"""
    r = Bits(sections(f)[3])
    return [parse_table(r) for _ in range(4)], r.read(13)


def kraft16(sizes):
    return sum(1 << (16 - s) for s in sizes if s)


def symbols_written(streams, table):
    return [op[1] for st in streams for op in st.ops if op[0] == table]


def vlc_chunks(v, bits):
    n = 1
    while v >> (bits * n):
        n += 1
    return n


@pytest.mark.parametrize("name", lz.NAMES)
def test_every_case_is_what_its_name_says(name):
    case = lz.CASES[name]
    f, _, _, streams = lz.build(name)
    tables, hs = parse_tables(f)
    assert hs == case.hs and bool(bu.read_header(f).flags & 4) == case.alpha
    for ti, t in enumerate(tables):  # every symbol the streams write has a code; every table but the one under test is a complete code
        used = set(symbols_written(streams, ti))
        assert all(s < len(t["sizes"]) and t["sizes"][s] for s in used), (name, ti)
        if bb.TABLE_NAMES[ti] != case.table and len(used) > 1:
            assert kraft16(t["sizes"]) == 65536 and len(t["sizes"]) == t["total_used"]
    if case.shape == "script":
        check_script(case, streams)
        return
    ti = bb.TABLE_NAMES.index(case.table)
    t = tables[ti]
    sizes, used = t["sizes"], set(symbols_written(streams, ti))
    coded = [s for s in sizes if s]
    if case.shape == "single":
        assert coded == [1] and len(used) == 1
    elif case.shape == "fixed16":
        assert len(used) >= 1 and set(coded) == {16} and max(sizes) == 16 and len(coded) == len(used) and kraft16(sizes) == len(used) < 65536
    elif case.shape == "incomplete":
        assert len(used) >= 2 and kraft16(sizes) == 32768
    elif case.shape in ("long_tail_zero", "long_tail_repeat"):
        assert len(used) >= 2 and t["tokens"][-1][0] in ((17, 18) if case.shape == "long_tail_zero" else (19, 20))
        assert len(sizes) - t["total_used"] >= 5 and kraft16(sizes) <= 65536
        if case.shape == "long_tail_repeat":  # the sizes past total_used are coded symbols no stream uses
            assert all(sizes[t["total_used"]:]) and max(used) < t["total_used"]
    elif case.shape == "cl_full":
        assert t["n_cl"] == 21 and all(t["cl_sizes"]) and len(used) >= 2
    elif case.shape == "cl_min":
        assert t["n_cl"] == 6 and set(coded) == {8} and len(used) >= 2
        assert {tok for tok, _ in t["tokens"]} <= {0, 8, 17, 18, 19, 20}
    elif case.shape == "collide":
        assert len(used) >= 2 and kraft16(sizes) > 65536 and max(sizes) < 16
    elif case.shape == "empty_rle":
        assert (t["total_used"], sizes) == ((0, []) if case.tables["rle"] == "empty" else (1, [0]))
        assert not used and all(not st.runs for st in streams)
        if case.tables["rle"] == "empty":
            assert t["n_cl"] == 0
    else:
        raise AssertionError(case.shape)


def check_script(case, streams):
    n_sel, hs = lz.N_CODEBOOK, case.hs
    assert [(st.indices.shape[1], st.indices.shape[0]) for st in streams] == [d for d in case.dims for _ in range(2 if case.alpha else 1)]
    assert {1} <= {d[0] for d in case.dims} and any(d[0] & 1 and d[1] & 1 and d[0] > 1 for d in case.dims)  # a one-column grid and an odd x odd one
    if not case.alpha:
        assert any(d[1] == 1 for d in case.dims) and (40, 30) in case.dims  # a one-row grid and the largest
    chunks = set()
    for st in streams:
        nby, nbx = st.indices.shape[:2]
        n_blocks, n_groups = nbx * nby, ((nbx + 1) // 2) * ((nby + 1) // 2)
        pred, sel, rle = ([op[1] for op in st.ops if op[0] == k] for k in (0, 2, 3))
        if case.script in ("pred_run", "one_run"):  # one literal group, one run over all the others
            assert pred == [bb.ONE_RUN_PRED_SYM, 256] and st.pred_runs == [(1, n_groups - 1)]
            chunks.add(vlc_chunks(n_groups - 1 - 3, 4))
        if case.script in ("sel_run", "one_run"):  # one literal, one run over all the other blocks, through the escape
            assert sel == [n_sel - 1, n_sel + hs] and rle == [63] and st.runs == [(1, n_blocks - 1)] and st.run_pending == 0
            chunks.add(-vlc_chunks(n_blocks - 1 - 3, 7))
        if case.script in ("run_exact_end", "run_leftover"):
            left = 40 if case.script == "run_leftover" else 0
            assert len(st.runs) == 1 and sum(st.runs[0]) == n_blocks + left and st.run_pending == left and sel.count(n_sel + hs) == 1
        if case.script == "hist_last":
            lits = max(1, hs // 2)
            assert len(sel) == n_blocks and all(s < n_sel for s in sel[:lits]) and set(sel[lits:]) == {n_sel + hs - 1}
            assert len(np.unique(st.indices[:, :, 1])) >= (1 if hs == 1 else 2)
        if case.script == "delta_wrap":
            assert pred == [255] * n_groups and len([op for op in st.ops if op[0] == 1]) == n_blocks
            # (the slice's first block cannot wrap: the previous index is 0, mod.rs:228)
            assert all(w >= 1 for y, w in enumerate(st.wraps) if not (y == 0 and nbx == 1)), st.wraps
    if case.script in ("pred_run", "one_run") and not case.alpha:
        assert {1, 2, 3} <= {c for c in chunks if c > 0}  # the repeat count in one, two and three VLC chunks (mod.rs:585-608)
    if case.script in ("sel_run", "one_run") and not case.alpha:
        assert {-1, -2} <= {c for c in chunks if c < 0}   # the 63-escape's count in one and two chunks


# ---- the files tests/test_gpu_lz_shapes.py reads on the device ---------------------------------------------------------------------------
@pytest.mark.parametrize("recipe,size", lz.GPU_FILES, ids=["%s-%s" % k for k in lz.GPU_FILES])
def test_device_files_take_the_doors_and_loops_their_rows_say(tmp_path, oracle, harness, recipe, size):
    """the front door and the CRC mode by the constants (check_gpu_door); both host decoders give the record; the empty history_rle table sends every slice
    to the exact loop and keeps the two-thread form from starting (may_split false), the run slices decode in the fast loop and on two threads"""
    lz.check_gpu_door(recipe, size)
    f, ep, rows, streams = lz.gpu_file(recipe, size)
    may_split = lz.GPU_RECIPES[recipe][1]
    for si, stream in enumerate(streams):
        want = bb.index_words(stream)
        st, oep, osel, oidx = oracle_slice(oracle, f, si)
        assert st == 0 and (oidx == want).all() and (oep == ep).all() and (osel[:, :4] == rows).all(), (recipe, size, si)
        assert (bu.basislz_decode(f, si)[2] == want).all(), (recipe, size, si)
    path = tmp_path / "t.basis"
    path.write_bytes(f)
    r = subprocess.run([harness, str(path), "0"], capture_output=True, text=True)
    assert r.returncode == 0 and "fuzz done" in r.stdout, r.stdout + r.stderr[-3000:]
    loops = re.findall(r"^slice \d+: decode_slice=(\w+) status=0$", r.stdout, re.M)
    assert loops == ["fast" if may_split else "exact"] * len(streams) and "split_ok=%d" % may_split in r.stdout, r.stdout
    assert len(re.findall(r"^slice \d+: two-thread=lex\+resolve$", r.stdout, re.M)) == (len(streams) if may_split else 0)


# ---- the builder writes the files it always wrote ----------------------------------------------------------------------------------------
PINNED = {  # SHA-256 of files built before the record, `tables=` and `script=` existed
    ("cube_mips", False): "6e754a1825b7d3db3ef7da8cd93f6f04d6ccda37d7aa7eb57f7c09fc98da676f",
    ("cube_mips", True): "5cee722f247f8aa41fa0f24adc1ad964371666b5ebad7e176d2f1b6d6674d9e5",
    ("unit_edges", False): "27962a75e4b24b743bc5a264a7d948010edc69a2ed87b0db49997d1af7749c19",
    ("unit_edges", True): "7beb9a18e0bacb645823ad590d495309986dd1b400150cef9ab9c84219654f82",
    ("array_240", False): "07052a2f5d551342517360cafac47bc45f6106c6dfb80f058b712680f0262c4f",
    ("array_240", True): "d85ca044550a7b307c2a8db5ea7c0243c2efa82d777ff56044b78b69496dc820",
    ("mip_chain_192", False): "3a6ac1213e09f457cfc240e8e99fc2d78e69ba6ddefb18eafc05e571deff9c40",
    ("mip_chain_192", True): "2cb7dfc34d23599ab057a8f3e767bdd288e8d17c1c9060fddab26a62d7b3f2c4",
}
PINNED_CONTAINER = (  # three etc1s_file calls of tests/test_container.py: (seed, dims, keywords, SHA-256)
    (1, [(4, 4)], dict(n_codebook=32), "bf5e8db44fc23bdba545986784fdb78be924db0436e01a0bcefdc8f62d8a5a14"),
    (3, [(7, 5), (4, 4)], dict(n_codebook=40, raw_selectors=False), "296c0d9bb2f556abc50544f9f5943f6516d4e46e6b110d9d4c4e1953a70a2d2d"),
    (4, [(9, 7), (4, 4), (13, 2), (6, 6), (5, 3), (8, 8)], dict(n_codebook=70, alpha=True), "5fb68e012500df50538993bd2303505711233dc144c8476d01cf6029e6aa6ad9"),
)


def test_existing_calls_of_the_builder_write_the_same_bytes():
    import hashlib

    import file_shape_cases as fsc

    for (name, alpha), want in PINNED.items():
        assert hashlib.sha256(fsc.etc1s_file(name, alpha)).hexdigest() == want, (name, alpha)
    for seed, dims, kw, want in PINNED_CONTAINER:
        assert hashlib.sha256(bb.etc1s_file(np.random.default_rng(seed), dims, **kw)[0]).hexdigest() == want, seed
        # asking for the record changes neither the bytes nor the draws
        assert hashlib.sha256(bb.etc1s_file(np.random.default_rng(seed), dims, want_indices=True, **kw)[0]).hexdigest() == want, seed
