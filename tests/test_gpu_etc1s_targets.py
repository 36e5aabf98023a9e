"""ETC1S -> BC1, BC3, BC4, BC5, EAC R11 and EAC RG11 on the device (bu_etc1s_transcode_device / bu_etc1s_transcode), bit for bit against
the numpy models of tests/colour_model.py and tests/channel_model.py applied to the oracle's RGBA32 decode of the same blocks.  Both kernel
paths (the L2 gather below 2^19 blocks or with codebooks too large for LDS, the LDS-staged kernel above), with and without an alpha slice,
index errors, refused arguments, graph capture, and a whole ETC1S file slice pair by slice pair.  Run on the GPU box: pytest -m gpu."""
import numpy as np
import pytest

import basis_builder as bb
import test_etc1s_targets as tet
from basisu_rs_amd import BasisuError, _lib, basislz_decode, read_header, read_slice_descs, synth

pytestmark = pytest.mark.gpu
NAMES = tuple(tet.TARGETS)
BIG = (1 << 19) + 77  # the staged kernel from 2^19 blocks
SIZES = (1, 1000, BIG)
M = 32768  # distinct blocks per codebook; the index arrays repeat them in a scrambled order
# (n_endpoints, n_selectors): (n_ep + n_sel + 256) * 4 bytes of LDS = about 48 KiB, 126 KiB, and 188 KiB (too large: the gather)
CODEBOOKS = {"48k": (6000, 6000), "126k": (16000, 16000), "big": (24000, 24000)}


def _selectors(rows):
    sel = np.zeros((rows.shape[0], 8), dtype=np.uint8)
    sel[:, :4] = rows
    return sel


@pytest.fixture(scope="module")
def books(oracle):
    """per codebook: endpoints, selector entries, M distinct colour / alpha index pairs, the scrambled order of BIG blocks, and the
    model's blocks of the M pairs for every target, with and without the alpha slice"""
    out = {}
    for k, (n_ep, n_sel) in CODEBOOKS.items():
        ep, rows = synth.etc1s_codebooks(n_ep, n_sel, seed=n_ep)
        rng = np.random.default_rng(n_ep)
        # a quarter of the entries draw their texels from a few selectors only (solid and two-colour blocks)
        q = n_sel // 4
        rows[:q] = tet.rows_from(rng, q).astype("<u4").view(np.uint8).reshape(q, 4)
        sel = _selectors(rows)
        idx = (rng.integers(0, n_ep, M) | (rng.integers(0, n_sel, M) << 16)).astype(np.uint32)
        aidx = (rng.integers(0, n_ep, M) | (rng.integers(0, n_sel, M) << 16)).astype(np.uint32)
        idx[:n_ep] = (np.arange(n_ep) | (rng.integers(0, n_sel, n_ep) << 16)).astype(np.uint32)  # every endpoint at least once
        order = (np.arange(BIG, dtype=np.int64) * 7919 + 13) % M
        want = {}
        for alpha in (False, True):
            rgba = np.concatenate([oracle.etc1s_to_rgba(idx[c:c + 8192], aidx[c:c + 8192] if alpha else None, 1, min(8192, M - c), ep, sel)
                                   for c in range(0, M, 8192)]).reshape(M, 64)
            for name in NAMES:
                want[name, alpha] = tet.model(name, rgba)
        out[k] = dict(ep=ep, sel=sel, idx=idx, aidx=aidx, order=order, want=want)
    return out


def _device(ctx, target, idx, aidx, ep, sel, n, bb_, offset=0):
    import torch

    d_idx = torch.from_numpy(idx.view(np.int32)).cuda()
    d_aidx = None if aidx is None else torch.from_numpy(aidx.view(np.int32)).cuda()
    d_ep = torch.from_numpy(ep.view(np.int32)).cuda()
    d_sel = torch.from_numpy(sel.reshape(-1)).cuda()
    d_out = torch.full((n * bb_ + 16,), 0xAB, dtype=torch.uint8, device="cuda")
    d_st = torch.full((1,), -1, dtype=torch.int64, device="cuda")
    ctx.etc1s_transcode_device(target, d_idx, d_aidx, n, d_ep, ep.size, d_sel, sel.shape[0], d_out.data_ptr() + offset, d_st)
    torch.cuda.synchronize()
    return d_out[offset:offset + n * bb_].cpu().numpy().reshape(n, bb_), int(d_st.cpu().numpy().view(np.uint64)[0])


def _first_bad(word):
    import ctypes

    bad = ctypes.c_uint64(0)
    st = _lib.load().bu_status_word_decode(word, ctypes.byref(bad))
    return st, bad.value


def _same(got, want, what):
    badb = np.nonzero((got != want).any(1))[0]
    assert badb.size == 0, "%s: %d blocks differ, first %d: %s vs %s" % (what, badb.size, badb[0], got[badb[0]], want[badb[0]])


@pytest.mark.parametrize("alpha", [False, True], ids=["opaque", "alpha"])
@pytest.mark.parametrize("name", NAMES)
def test_both_forms_equal_the_model(ctx, books, name, alpha):
    t, bb_ = tet.TARGETS[name]
    for k, b in books.items():
        for n in SIZES:
            o = b["order"][:n]
            idx, aidx = b["idx"][o], (b["aidx"][o] if alpha else None)
            want = b["want"][name, alpha][o]
            got, word = _device(ctx, t, idx, aidx, b["ep"], b["sel"], n, bb_)
            assert _first_bad(word)[0] == _lib.OK
            _same(got, want, "%s %s n=%d device" % (name, k, n))
            got = ctx.etc1s_transcode(t, idx, aidx, b["ep"], b["sel"]).reshape(n, bb_)
            _same(got, want, "%s %s n=%d host" % (name, k, n))


@pytest.mark.parametrize("name", NAMES)
def test_index_errors_report_the_lowest_block(ctx, books, name):
    t, bb_ = tet.TARGETS[name]
    b = books["48k"]
    n_ep, n_sel = CODEBOOKS["48k"]
    for n in (1000, BIG):
        o = b["order"][:n]
        for where, (i_bad, a_bad) in {"colour": (700, None), "alpha": (None, 600), "both": (900, 333)}.items():
            idx, aidx = b["idx"][o].copy(), b["aidx"][o].copy()
            if i_bad is not None:
                idx[i_bad] = n_ep  # endpoint index out of range
                idx[i_bad + 50] = (idx[i_bad + 50] & 0xFFFF) | (n_sel << 16)  # and a selector index further on
            if a_bad is not None:
                aidx[a_bad] = (aidx[a_bad] & 0xFFFF) | (n_sel << 16)
            lowest = min(x for x in (i_bad, a_bad) if x is not None)
            got, word = _device(ctx, t, idx, aidx, b["ep"], b["sel"], n, bb_)
            st, first = _first_bad(word)
            assert st == _lib.ERR_INDEX_RANGE and first == lowest, (where, n, st, first)
            assert (got[lowest] == 0).all()
            with pytest.raises(BasisuError) as e:
                ctx.etc1s_transcode(t, idx, aidx, b["ep"], b["sel"])
            assert e.value.status == _lib.ERR_INDEX_RANGE and e.value.first_bad_block == lowest, (where, n)


def test_other_targets_and_misaligned_output_are_refused(ctx, books):
    import torch

    b = books["48k"]
    idx = b["idx"][:64]
    for t in (0, 1, 2, 3, 4, 5, 10, 13):
        with pytest.raises(BasisuError) as e:
            ctx.etc1s_transcode(t, idx, None, b["ep"], b["sel"])
        assert e.value.status == _lib.ERR_ARGUMENT, t
        d_out = torch.zeros(64 * 64, dtype=torch.uint8, device="cuda")
        with pytest.raises(BasisuError) as e:
            ctx.etc1s_transcode_device(t, torch.from_numpy(idx.view(np.int32)).cuda(), None, 64, torch.from_numpy(b["ep"].view(np.int32)).cuda(),
                                       b["ep"].size, torch.from_numpy(b["sel"].reshape(-1)).cuda(), b["sel"].shape[0], d_out)
        assert e.value.status == _lib.ERR_ARGUMENT, t
    for name, (t, bb_) in tet.TARGETS.items():
        with pytest.raises(BasisuError) as e:
            _device(ctx, t, idx, None, b["ep"], b["sel"], 64, bb_, offset=bb_ // 2)
        assert e.value.status == _lib.ERR_ARGUMENT, name
        got, word = _device(ctx, t, idx, None, b["ep"], b["sel"], 0, bb_)  # n_blocks == 0: OK, nothing written
        assert word == 0xFFFFFFFFFFFFFFFF


@pytest.mark.parametrize("name", ["bc1", "rg11"])
def test_graph_capture_equals_the_direct_call(ctx, books, name):
    import torch

    t, bb_ = tet.TARGETS[name]
    b = books["126k"]
    o = b["order"]
    d_idx = torch.from_numpy(b["idx"][o].view(np.int32)).cuda()
    d_aidx = torch.from_numpy(b["aidx"][o].view(np.int32)).cuda()
    d_ep = torch.from_numpy(b["ep"].view(np.int32)).cuda()
    d_sel = torch.from_numpy(b["sel"].reshape(-1)).cuda()
    direct = torch.zeros(BIG * bb_, dtype=torch.uint8, device="cuda")
    ctx.etc1s_transcode_device(t, d_idx, d_aidx, BIG, d_ep, b["ep"].size, d_sel, b["sel"].shape[0], direct)
    torch.cuda.synchronize()
    replay = torch.zeros_like(direct)
    s = torch.cuda.Stream()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        ctx.etc1s_transcode_device(t, d_idx, d_aidx, BIG, d_ep, b["ep"].size, d_sel, b["sel"].shape[0], replay, stream=s)
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(direct, replay)
    _same(replay.cpu().numpy().reshape(BIG, bb_), b["want"][name, True][o], name + " graph")


@pytest.mark.parametrize("name", NAMES)
def test_etc1s_file_slice_pairs(ctx, oracle, name):
    t, bb_ = tet.TARGETS[name]
    f, _, _ = bb.etc1s_file(np.random.default_rng(61), [(64, 64), (33, 17), (1, 1)], n_codebook=1024, alpha=True)
    st, _, imgs = oracle.read_to("rgba", f)
    assert st == 0 and len(imgs) == 3
    descs = read_slice_descs(f, read_header(f))
    for k, (w, h, _, data) in enumerate(imgs):
        nbx, nby = descs[2 * k].num_blocks_x, descs[2 * k].num_blocks_y
        assert data.size == nbx * nby * 64
        rgba = data.reshape(nby, 4, nbx, 4, 4).transpose(0, 2, 1, 3, 4).reshape(-1, 64)  # row-major image -> blocks
        ep, sel, idx = basislz_decode(f, 2 * k)
        _, _, aidx = basislz_decode(f, 2 * k + 1)
        got = ctx.etc1s_transcode(t, idx, aidx, ep, sel).reshape(-1, bb_)
        _same(got, tet.model(name, rgba), "%s image %d" % (name, k))
