"""Guard bands and poisoned tails at every device entry point.  The other GPU tests pin what the kernels write inside [0, n); here every buffer a
kernel is handed sits in an arena of tests/gpu_guard.py -- a guard band in front of it and behind it (and between the runs of a batch), inputs
followed and preceded by invalid blocks / indices no codebook holds -- and every case asserts four things: the data equals the expected bytes, every
band of every buffer is intact (the inputs' too, which nothing may write), the status word is clear, and with one invalid block planted at n - 1 and
one at 0 the lowest is reported, both outputs are zeros and the bands are still intact.

The cases are tests/guard_cases.py's (tests/test_guard_cases.py holds, without a GPU, that they reach every kernel the launch plan can choose).  Inputs
are gathered on the device from the 608 known-answer vectors by a seeded index; expected bytes are the same gather of the golden results (ASTC, BC7,
ETC1, ETC2, RGBA32 rearranged into image rows) and of the numpy models applied once to the oracle's RGBA32 decode of the 608 vectors (the six other
targets).  Run on the GPU box: pytest -m gpu."""
import ctypes
import os

import numpy as np
import pytest

import basis_builder as bb
import gpu_guard as gg
import guard_cases as gc
import test_etc1s_targets as tet
from basisu_rs_amd import BasisuError, _lib, read_file_query, read_file_to, read_query, read_to_bc1, read_to_bc7, read_to_etc1, read_to_rgba, synth

pytestmark = pytest.mark.gpu
CLEAR = 0xFFFFFFFFFFFFFFFF
BASE = 1000  # block_index_base of the blocking call


# ---- shared state -----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def env(golden, oracle, ctx):
    """the 608 vectors and every target's 608 expected blocks on the device (computed once, never written)"""
    import torch

    st, _, rgba = oracle.decode_to_rgba(golden["uastc"].tobytes(), 1)
    assert st == 0
    rgba = rgba.reshape(608, 64)
    assert (rgba == golden["rgba"]).all()
    want = {name: golden[name] for name in ("astc", "bc7", "etc1", "etc2", "rgba")}
    for name in tet.TARGETS:
        want[name] = tet.model(name, rgba)
    return dict(torch=torch, ctx=ctx, cus=torch.cuda.get_device_properties(0).multi_processor_count,
                gu=torch.from_numpy(golden["uastc"]).cuda(), want={k: torch.from_numpy(np.ascontiguousarray(v)).cuda() for k, v in want.items()},
                gu_host=golden["uastc"], want_host=want)


def _index(torch, n, seed):
    return torch.randint(0, 608, (n,), device="cuda", generator=torch.Generator(device="cuda").manual_seed(seed))


def _rows(blocks, bpr):
    """RGBA32 blocks [n, 64] (four rows of 16 bytes each) -> the row-major image of bpr blocks per row, flat"""
    n = blocks.shape[0]
    return blocks.reshape(n // bpr, bpr, 4, 16).permute(0, 2, 1, 3).reshape(-1)


def _expected(e, name, idx, bpr, zero=()):
    """the flat expected bytes of blocks gu[idx]; `zero`: blocks written as zeros (failing ones)"""
    w = e["want"][name][idx]
    for z in zero:
        w[z] = 0
    return _rows(w, bpr) if name == "rgba" else w.reshape(-1)


def _tile_blocks(name, n, cus):
    return 4096 if name in gc.ETC_FAMILY and n > 3 * gc.TILE * cus else 1024


def _status_tensor(e):
    st = e["torch"].empty(1, dtype=e["torch"].int64, device="cuda")
    e["ctx"].status_word_reset(st)
    return st


def _word(st):
    return int(st.item()) & CLEAR


def _first_bad(ctx, word):
    with pytest.raises(BasisuError) as err:
        ctx.status_word_check(word)
    return err.value.first_bad_block


def _arenas(e, name, sizes, in_offsets, out_offsets, tile, adjacent=False):
    """the input arena (invalid blocks around and between the runs) and the output arena of runs of `sizes` blocks"""
    bb_ = gc.TARGETS[name][1]
    if adjacent:
        sizes, in_offsets, out_offsets = [sum(sizes)], in_offsets[:1], out_offsets[:1]
    ain = gg.Arena(name + " input", [16 * n for n in sizes], gg.POISON_BLOCKS * 16, in_offsets, fill="uastc")
    aout = gg.Arena(name + " output", [bb_ * n for n in sizes], gg.guard_bytes(bb_, tile), out_offsets)
    return ain, aout


def _min_out_align(name):
    return 8 if gc.TARGETS[name][1] == 8 else 16


# ---- bu_uastc_transcode_device and bu_uastc_transcode_device_sync -----------------------------------------------------------------
def _one_slice(e, name, c):
    torch, ctx, cus = e["torch"], e["ctx"], e["cus"]
    t, bb_ = gc.TARGETS[name]
    n, bpr = gc.size_of(c, name, cus), gc.pitch_of(c, name, cus)
    ain, aout = _arenas(e, name, [n], [16 if c["min_align"] else 0], [_min_out_align(name) if c["min_align"] else 0], _tile_blocks(name, n, cus))
    idx = _index(torch, n, 5 + n % 1000)
    d_in = ain.data().view(n, 16)
    d_in[:] = e["gu"][idx]
    good = _expected(e, name, idx, bpr)
    planted = _expected(e, name, idx, bpr, zero=(0, n - 1))
    status = _status_tensor(e)
    for policy in c["policies"]:
        ctx.set_launch_policy({gc.EXCL: False, gc.SHARED: True, gc.AUTO: "auto"}[policy])
        for bad in (False, True):
            what = (name, c["id"], n, bpr, policy, "planted" if bad else "good")
            if bad:
                d_in[0, 0] = 69
                d_in[n - 1, 0] = 69
            aout.data().fill_(0xEE)
            torch.cuda.synchronize()
            if c["entry"] == "sync":
                word = ctx.transcode_device_sync(t, ain.ptr(), n, aout.ptr(), bpr, BASE)
            else:
                ctx.status_word_reset(status)
                ctx.transcode_device(t, ain.ptr(), n, aout.ptr(), bpr, 0, status)
                torch.cuda.synchronize()
                word = _word(status)
            if bad:
                assert _first_bad(ctx, word) == (BASE if c["entry"] == "sync" else 0), what
                d_in[0] = e["gu"][idx[0]]
                d_in[n - 1] = e["gu"][idx[n - 1]]
            else:
                assert word == CLEAR, what + (hex(word),)
            assert torch.equal(aout.data(), planted if bad else good), what
            ain.check()
            aout.check()
    ctx.set_launch_policy("auto")


@pytest.mark.parametrize("name", gc.ALL)
def test_device_call_over_the_one_slice_cases(env, name):
    cases = gc.cases_for(name, "device")
    assert sum(c["min_align"] for c in cases) >= 1
    try:
        for c in cases:
            _one_slice(env, name, c)
    finally:  # (the context is the session's)
        env["ctx"].set_launch_policy("auto")


@pytest.mark.parametrize("name", gc.ALL)
def test_blocking_device_call_on_a_ragged_range(env, name):
    cases = gc.cases_for(name, "sync")
    assert cases
    try:
        for c in cases:
            _one_slice(env, name, c)
    finally:  # (the context is the session's)
        env["ctx"].set_launch_policy("auto")


# ---- bu_uastc_transcode_batch_device and bu_uastc_transcode_batch_in_flight -------------------------------------------------------
def _batch(e, name, sizes, bpr, adjacent, calls):
    """runs of `sizes` blocks, every run a region of one input and one output arena (adjacent: one region cut into the runs); `calls`: which of
    "batch" (bu_uastc_transcode_batch_device on the current stream) and "in_flight" (four of the context's streams) to run"""
    torch, ctx, cus = e["torch"], e["ctx"], e["cus"]
    t, bb_ = gc.TARGETS[name]
    k = len(sizes)
    # every third run's output on the smallest alignment the entry point takes
    out_offsets = [(_min_out_align(name) if i % 3 == 1 else 0) for i in range(k)]
    in_offsets = [(16 if i % 3 == 2 else 0) for i in range(k)]
    ain, aout = _arenas(e, name, sizes, in_offsets, out_offsets, 2048 if name in gc.ETC_FAMILY else 1024, adjacent)
    starts = np.concatenate([[0], np.cumsum(sizes)])
    if adjacent:
        in_ptrs = [ain.ptr() + 16 * int(s) for s in starts[:-1]]
        out_ptrs = [aout.ptr() + bb_ * int(s) for s in starts[:-1]]
        ins = [ain.data().view(-1, 16)[int(a):int(b)] for a, b in zip(starts, starts[1:])]
        outs = [aout.data()[bb_ * int(a):bb_ * int(b)] for a, b in zip(starts, starts[1:])]
    else:
        in_ptrs, out_ptrs = [ain.ptr(i) for i in range(k)], [aout.ptr(i) for i in range(k)]
        ins, outs = [ain.data(i).view(-1, 16) for i in range(k)], [aout.data(i) for i in range(k)]
    idxs = [_index(torch, n, 31 + i) for i, n in enumerate(sizes)]
    for d, idx in zip(ins, idxs):
        d[:] = e["gu"][idx]
    good = [_expected(e, name, idx, bpr) for idx in idxs]
    planted = list(good)
    planted[0] = _expected(e, name, idxs[0], bpr, zero=(0,) if k > 1 else (0, sizes[0] - 1))
    if k > 1:
        planted[-1] = _expected(e, name, idxs[-1], bpr, zero=(sizes[-1] - 1,))
    status = _status_tensor(e)
    VP, SZ = ctypes.c_void_p * k, ctypes.c_size_t * k
    for call in calls:
        for bad in (False, True):
            what = (name, sizes, bpr, call, "planted" if bad else "good")
            if bad:
                ins[0][0, 0] = 69
                ins[-1][sizes[-1] - 1, 0] = 69
            for o in outs:
                o.fill_(0xEE)
            ctx.status_word_reset(status)
            torch.cuda.synchronize()
            if call == "batch":
                st = ctx._lib.bu_uastc_transcode_batch_device(ctx.handle, t, k, VP(*in_ptrs), SZ(*sizes), VP(*out_ptrs), bpr, None,
                                                              ctypes.c_void_p(status.data_ptr()), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
                assert st == 0, what
            else:
                ctx.transcode_batch_in_flight(t, in_ptrs, sizes, out_ptrs, bpr, None, status, 4)
                ctx.synchronize()
            torch.cuda.synchronize()
            word = _word(status)
            if bad:
                assert _first_bad(ctx, word) == 0, what  # (runs are numbered back to back from 0: the first block of the batch)
                ins[0][0] = e["gu"][idxs[0][0]]
                ins[-1][sizes[-1] - 1] = e["gu"][idxs[-1][sizes[-1] - 1]]
            else:
                assert word == CLEAR, what + (hex(word),)
            for i, o in enumerate(outs):
                assert torch.equal(o, (planted if bad else good)[i]), what + (i,)
            ain.check()
            aout.check()


@pytest.mark.parametrize("name", gc.ALL)
def test_batch_calls_with_a_guard_band_between_runs(env, name):
    batches = [b for b in gc.BATCHES if name in b["targets"]]
    assert batches
    for b in batches:
        _batch(env, name, b["sizes"](env["cus"]), b["bpr"], b["adjacent"], ("batch", "in_flight") if b["in_flight"] else ("batch",))


@pytest.mark.parametrize("name", gc.ALL)
def test_in_flight_call_cuts_one_array_into_pieces(env, name):
    arrays = [a for a in gc.IN_FLIGHT_ARRAYS if name in a["targets"]]
    assert arrays
    for a in arrays:
        _batch(env, name, [a["n"](env["cus"])], a["bpr"], False, ("in_flight",))


# ---- host pointers: transcode / decode_to_rgba ------------------------------------------------------------------------------------
def _host_call(ctx, name, t, data, bpr, out):
    return ctx.decode_to_rgba(data, bpr, out=out) if name == "rgba" else ctx.transcode(t, data, out=out)


@pytest.mark.parametrize("where", ["pinned", "pageable"])
@pytest.mark.parametrize("name", gc.ALL)
def test_host_pointer_calls_into_a_guarded_out(env, name, where):
    """page-locked out=: the kernels store into it over PCIe, on the zero-copy shape; pageable out=: the copy-back stays in range"""
    ctx, cus = env["ctx"], env["cus"]
    t, bb_ = gc.TARGETS[name]
    for c in gc.cases_for(name, where):
        n, bpr = gc.size_of(c, name, cus), gc.pitch_of(c, name, cus)
        idx = synth.gold_indices(n, seed=900 + n % 97)
        ain = gg.Arena(name + " host input", 16 * n, gg.POISON_BLOCKS * 16, 0, fill="uastc", where="pageable")
        aout = gg.Arena(name + " host output", bb_ * n, gg.guard_bytes(bb_), 0, where=where, ctx=ctx)
        try:
            ain.data().reshape(n, 16)[:] = env["gu_host"][idx]
            want = env["want_host"][name][idx]
            want = want.reshape(n // bpr, bpr, 4, 16).transpose(0, 2, 1, 3).reshape(-1) if name == "rgba" else want.reshape(-1)
            aout.data()[:] = 0xEE
            got = _host_call(ctx, name, t, ain.data(), bpr, aout.data())
            assert got.ctypes.data == aout.ptr() and (got == want).all(), (name, where, n)
            ain.check()
            aout.check()
            blocks = ain.data().reshape(n, 16)
            blocks[0, 0] = 69
            blocks[n - 1, 0] = 69
            with pytest.raises(BasisuError) as err:
                _host_call(ctx, name, t, ain.data(), bpr, aout.data())
            assert err.value.first_bad_block == 0, (name, where, n)
            ain.check()
            aout.check()  # (the contents of `out` are unspecified after an error; the bands around it are not)
        finally:
            aout.free()


@pytest.mark.parametrize("where", ["pinned", "pageable"])
def test_rgba32_ragged_last_row_writes_nothing_past_the_buffer(env, where):
    """decode_to_rgba stores whole image rows: n % blocks_per_row != 0 is refused (the reference would index past its image there) and nothing is
    written, neither past 64 * n bytes of the caller's buffer nor into it"""
    ctx = env["ctx"]
    n, bpr = 5003, 128
    ain = gg.Arena("rgba host input", 16 * n, gg.POISON_BLOCKS * 16, 0, fill="uastc", where="pageable")
    aout = gg.Arena("rgba host output", 64 * n, gg.guard_bytes(64), 0, where=where, ctx=ctx)
    try:
        ain.data().reshape(n, 16)[:] = env["gu_host"][synth.gold_indices(n, seed=77)]
        aout.data()[:] = 0xEE
        with pytest.raises(BasisuError) as err:
            ctx.decode_to_rgba(ain.data(), bpr, out=aout.data())
        assert err.value.status == _lib.ERR_ARGUMENT
        assert (aout.data() == 0xEE).all()
        ain.check()
        aout.check()
    finally:
        aout.free()


# ---- ETC1S slice entry points -----------------------------------------------------------------------------------------------------
M = 4096  # distinct blocks; the index arrays repeat them in a scrambled order
N_BASE = 6003
EP_PREFIXES, SEL_PREFIXES = (6000, 6001, 6002, 6003), (6000, 6001)
ETC1S_SIZES = (1, 255, 257, 1000, (1 << 19) + 77)  # the gather kernels; the staged ones from 2^19 blocks
ETC1S_ALL16 = ("etc1", "rgba", "bc1", "rg11")  # every prefix pair x both alignments; the four other targets take the two extreme combinations
ETC1S_TARGETS = dict(tet.TARGETS, etc1=(2, 8), rgba=(4, 64))


def _order(n):
    return (np.arange(n, dtype=np.int64) * 7919 + 13) % M


@pytest.fixture(scope="module")
def books(oracle):
    """one base codebook of 6003 + 6003 entries; M colour / alpha index pairs below 6000; per prefix pair, the two index pairs forced to endpoint 0 /
    selector 0 and to the last endpoint / selector of the prefix (the first two blocks of the scrambled order); expected blocks of all M from the
    oracle (ETC1, RGBA32) and the models applied to the oracle's RGBA32, once per codebook"""
    ep, rows = synth.etc1s_codebooks(N_BASE, N_BASE, seed=6003)
    rng = np.random.default_rng(6003)
    q = N_BASE // 4
    rows[:q] = tet.rows_from(rng, q).astype("<u4").view(np.uint8).reshape(q, 4)
    sel = oracle.selectors_from_rows(rows)
    idx = (rng.integers(0, 6000, M) | (rng.integers(0, 6000, M) << 16)).astype(np.uint32)
    aidx = (rng.integers(0, 6000, M) | (rng.integers(0, 6000, M) << 16)).astype(np.uint32)
    first, second = int(_order(2)[0]), int(_order(2)[1])
    idx[first] = aidx[first] = 0

    def expect(i, a, alpha, names):
        rgba = oracle.etc1s_to_rgba(i, a if alpha else None, 1, i.size, ep, sel).reshape(-1, 64)
        out = {"rgba": rgba}
        if not alpha:
            out["etc1"] = oracle.etc1s_to_etc1(i, ep, sel).reshape(-1, 8)
        for name in names:
            out[name] = tet.model(name, rgba)
        return out

    base = {alpha: expect(idx, aidx, alpha, tuple(tet.TARGETS)) for alpha in (False, True)}
    base[True]["etc1"] = base[False]["etc1"]
    forced = {}
    for n_ep in EP_PREFIXES:
        for n_sel in SEL_PREFIXES:
            w = np.array([(n_ep - 1) | ((n_sel - 1) << 16)], dtype=np.uint32)
            forced[n_ep, n_sel] = {alpha: expect(w, w, alpha, tuple(tet.TARGETS)) for alpha in (False, True)}
            forced[n_ep, n_sel][True]["etc1"] = forced[n_ep, n_sel][False]["etc1"]
    return dict(ep=ep, sel=sel, idx=idx, aidx=aidx, second=second, base=base, forced=forced)


def _etc1s_call(ctx, name, d_idx, d_aidx, n, nbx, d_ep, n_ep, d_sel, n_sel, d_out, d_st, stream):
    lib = ctx._lib
    if name == "etc1":
        return lib.bu_etc1s_transcode_etc1_device(ctx.handle, d_idx, n, d_ep, n_ep, d_sel, n_sel, d_out, d_st, stream)
    if name == "rgba":
        return lib.bu_etc1s_decode_rgba_device(ctx.handle, d_idx, d_aidx, nbx, n // nbx, d_ep, n_ep, d_sel, n_sel, d_out, d_st, stream)
    return lib.bu_etc1s_transcode_device(ctx.handle, ETC1S_TARGETS[name][0], d_idx, d_aidx, n, d_ep, n_ep, d_sel, n_sel, d_out, d_st, stream)


def _etc1s_combo(e, books, name, n_ep, n_sel, misaligned):
    torch, ctx = e["torch"], e["ctx"]
    t, bb_ = ETC1S_TARGETS[name]
    # codebooks: the prefix, then entries no good block decodes to; 0 / 4 and 0 / 8 bytes from 16-byte alignment
    a_ep = gg.Arena("endpoints", 4 * n_ep, gg.GUARD_MIN, 4 if misaligned else 0, fill="endpoint")
    a_sel = gg.Arena("selectors", 8 * n_sel, gg.GUARD_MIN, 8 if misaligned else 0, fill="selector")
    a_ep.data()[:] = torch.from_numpy(books["ep"][:n_ep].view(np.uint8)).cuda()
    a_sel.data()[:] = torch.from_numpy(books["sel"][:n_sel].reshape(-1)).cuda()
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    forced_word = (n_ep - 1) | ((n_sel - 1) << 16)
    for alpha in ((False,) if name == "etc1" else (False, True)):
        want_m = books["base"][alpha][name].copy()
        want_m[books["second"]] = books["forced"][n_ep, n_sel][alpha][name][0]
        d_want_m = torch.from_numpy(want_m).cuda()
        words = []
        for w in (books["idx"], books["aidx"]):
            w = w.copy()
            w[books["second"]] = forced_word
            words.append(torch.from_numpy(w.view(np.int32)).cuda())
        for n in ETC1S_SIZES:
            what = (name, n_ep, n_sel, misaligned, alpha, n)
            order = torch.from_numpy(_order(n)).cuda()
            nbx = gc.rgba_pitch(n) if name == "rgba" else 0
            ofs = 4 if misaligned else 0  # (index arrays: any 4-byte boundary; 8 bytes give the staged ETC1 kernel its four-blocks-per-lane path)
            a_idx = gg.Arena("indices", 4 * n, gg.POISON_BLOCKS * 4, ofs, fill="ones")
            a_aidx = gg.Arena("alpha indices", 4 * n, gg.POISON_BLOCKS * 4, ofs, fill="ones") if alpha else None
            a_out = gg.Arena(name + " output", bb_ * n, gg.guard_bytes(bb_), (8 if bb_ == 8 else 16) if misaligned else 0)
            a_idx.data().view(torch.int32)[:] = words[0][order]
            if alpha:
                a_aidx.data().view(torch.int32)[:] = words[1][order]
            good = d_want_m[order]
            planted = good.clone()
            planted[0] = 0
            planted[n - 1] = 0
            if name == "rgba":
                good, planted = _rows(good, nbx), _rows(planted, nbx)
            d_st = torch.empty(1, dtype=torch.int64, device="cuda")
            for bad in (False, True):
                if bad:  # an endpoint index one past the prefix in block 0, a selector index one past it in block n - 1 (the alpha slice's where there is one)
                    a_idx.data().view(torch.int32)[0] = n_ep
                    (a_aidx if alpha else a_idx).data().view(torch.int32)[n - 1] = n_sel << 16 if n > 1 else n_ep
                a_out.data().fill_(0xEE)
                d_st.fill_(-1)
                torch.cuda.synchronize()
                st = _etc1s_call(ctx, name, a_idx.ptr(), a_aidx.ptr() if alpha else None, n, nbx, a_ep.ptr(), n_ep, a_sel.ptr(), n_sel, a_out.ptr(),
                                 ctypes.c_void_p(d_st.data_ptr()), stream)
                assert st == 0, what
                torch.cuda.synchronize()
                word = _word(d_st)
                if bad:
                    with pytest.raises(BasisuError) as err:
                        ctx.status_word_check(word)
                    assert err.value.status == _lib.ERR_INDEX_RANGE and err.value.first_bad_block == 0, what
                else:
                    assert word == CLEAR, what + (hex(word),)
                assert torch.equal(a_out.data(), (planted if bad else good).reshape(-1)), what + (bad,)
                for a in (a_idx, a_aidx, a_out, a_ep, a_sel):
                    if a is not None:
                        a.check()


@pytest.mark.parametrize("name", tuple(ETC1S_TARGETS))
def test_etc1s_slice_entry_points(env, books, name):
    combos = [(n_ep, n_sel, mis) for n_ep in EP_PREFIXES for n_sel in SEL_PREFIXES for mis in (False, True)]
    assert len(combos) == 16
    if name not in ETC1S_ALL16:
        combos = [combos[0], combos[-1]]
    for n_ep, n_sel, mis in combos:
        _etc1s_combo(env, books, name, n_ep, n_sel, mis)


# ---- whole files ------------------------------------------------------------------------------------------------------------------
SMALL = [(64, 64), (33, 17), (1, 1)]  # blocks: whole 64-block units; ends mid-unit, units straddle rows; one block
STREAMED = [(192, 192), (33, 17), (1, 1)]  # the first image is above the streamed front door's threshold


def _tuples(imgs):
    return [(g.w, g.h, g.stride, g.data.tobytes()) for g in imgs]


def _read_file(name, f, ctx, out=None):
    if name == "etc1":
        return read_to_etc1(f, ctx, out=out)
    if name == "rgba":
        return read_to_rgba(f, ctx, out=out)[1]
    return read_file_to(ETC1S_TARGETS[name][0], f, ctx, out=out)


def _guarded_read(ctx, what, nbytes, bb_, read):
    """read(out) into a guarded page-locked and a guarded pageable buffer of exactly nbytes: [images of each]"""
    got = []
    for where in ("pinned", "pageable"):
        a = gg.Arena("%s %s out" % (what, where), nbytes, gg.guard_bytes(bb_), 0, where=where, ctx=ctx)
        try:
            a.data()[:] = 0xEE
            got.append(_tuples(read(a.data())))
            a.check()
        finally:
            a.free()
    return got


@pytest.fixture(scope="module")
def etc1s_files():
    out = {}
    for alpha in (True, False):
        out["small", alpha] = bb.etc1s_file(np.random.default_rng(61), SMALL, n_codebook=1024, alpha=alpha)[0]
        out["streamed", alpha] = bb.etc1s_file(np.random.default_rng(905), STREAMED, n_codebook=1024, alpha=alpha)[0]
    return out


@pytest.mark.parametrize("alpha", [True, False], ids=["alpha", "opaque"])
@pytest.mark.parametrize("name", tuple(ETC1S_TARGETS))
def test_etc1s_files_into_guarded_buffers(env, etc1s_files, name, alpha):
    """both front doors (everything decoded, then one launch over units padded to 64 blocks; the streamed door for a large first image): the
    images of the unguarded call (which the other GPU tests compare with the oracle and the models), and no byte outside them"""
    ctx = env["ctx"]
    t, bb_ = ETC1S_TARGETS[name]
    for door, f, var in (("one launch", etc1s_files["small", alpha], "BU_ETC1S_ONE_LAUNCH"), ("streamed", etc1s_files["streamed", alpha], None)):
        if var:
            os.environ[var] = "1"
        try:
            want = _tuples(_read_file(name, f, ctx))
            nbytes = (read_query(_lib.READ_ETC1 if name == "etc1" else _lib.READ_RGBA, f) if name in ("etc1", "rgba") else read_file_query(t, f))[1]
            assert nbytes == sum(len(w[3]) for w in want)
            for got in _guarded_read(ctx, "%s %s" % (name, door), nbytes, bb_, lambda out: _read_file(name, f, ctx, out)):
                assert got == want, (name, door, alpha)
        finally:
            if var:
                os.environ.pop(var, None)


def test_uastc_file_into_a_guarded_buffer(env):
    ctx = env["ctx"]
    dims = [(40, 30), (33, 17)]
    blocks = [env["gu_host"][synth.gold_indices(x * y, seed=70 + i)] for i, (x, y) in enumerate(dims)]
    f = bb.uastc_file(blocks, dims)
    for what, read, rt, bb_ in (("bc7", read_to_bc7, _lib.READ_BC7, 16), ("bc1", read_to_bc1, _lib.READ_BC1, 8),
                                ("rgba", lambda *a, **k: read_to_rgba(*a, **k)[1], _lib.READ_RGBA, 64)):
        want = _tuples(read(f, ctx))
        assert len(want) == 2
        for got in _guarded_read(ctx, "uastc file to " + what, read_query(rt, f)[1], bb_, lambda out: read(f, ctx, out=out)):
            assert got == want, what


# ---- the helper itself ------------------------------------------------------------------------------------------------------------
def test_checker_names_the_offset_of_a_dirtied_guard_byte(env):
    """one guard byte changed with a torch write (no kernel of the library takes part): the check names the arena, the band and the offset"""
    torch = env["torch"]
    a = gg.Arena("self-check", [4096, 8 * 7], 1024 * 16, [16, 8])
    assert [(a.addr + r.start) % 256 for r in a.regions] == [16, 8] and all(b - s >= gg.GUARD_MIN for s, b in a.bands)
    s0, b0 = a.bands[0]
    assert torch.equal(a.buf[s0:b0].cpu(), torch.from_numpy(gg.fill_bytes(np, s0, b0)))  # (the device's fill is the host's)
    a.data(0).zero_()
    a.data(1).zero_()
    a.check()
    at = a.regions[0].stop + 3
    a.buf[at] ^= 0x10
    assert a.violations() == [(1, at, 1)]
    with pytest.raises(AssertionError, match=r"self-check: guard band 1 changed at arena offset %d \(3 bytes past the end of region 0 " % at):
        a.check()
