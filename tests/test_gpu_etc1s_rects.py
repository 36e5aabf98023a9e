"""bu_etc1s_transcode_rects_device on the GPU: rectangles of ETC1S slices into pitched surfaces, many per call.

The test slices are 200 x 40 blocks (and 64 x 40, 37 x 40 for the many-job call) of random colour and alpha indices into synth.etc1s_codebooks(6000, 6000).
Expected bytes come from outside the code under test: oracle.etc1s_to_etc1, oracle.etc1s_to_rgba, and the numpy models of the six targets
(test_etc1s_targets.model) applied to the oracle's decode of the whole slice, cut with numpy.  Every surface is pre-filled with 0xAB between two guard bands of
the same byte and every byte of it is compared afterwards: the positions of the rectangle against the expected bytes, all others still 0xAB.  The index arrays
sit between bands of out-of-range index words, so a lane that took a block outside its slice would report it."""
import os
import sys

import numpy as np
import pytest

from basisu_rs_amd import _lib

pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

TARGETS = {"etc1": _lib.ETC1, "rgba": _lib.RGBA32, "bc1": _lib.BC1_RGB, "bc3": _lib.BC3_RGBA, "bc4": _lib.BC4_R, "bc5": _lib.BC5_RG, "r11": _lib.EAC_R11,
           "rg11": _lib.EAC_RG11}
N_EP = N_SEL = 6000
NBX, NBY = 200, 40
WIDTHS = (200, 64, 37)  # the three slices, all NBY block rows high
RECTS = ((0, 0, 200, 40), (7, 3, 1, 1), (5, 1, 63, 15), (64, 16, 64, 16), (3, 2, 65, 17), (190, 0, 10, 40), (0, 39, 200, 1), (11, 5, 32, 32), (1, 0, 1, 40),
         (2, 1, 9, 9), (20, 3, 17, 5), (100, 7, 33, 3))
POISON = 0xAB
GUARD = 4096       # bytes of poison in front of and behind every surface
BAND = 1024        # out-of-range index words in front of and behind every index array
CLEAR = _lib.STATUS_WORD_CLEAR


def row_bytes(name):
    """bytes a block takes of one output row (RGBA32: one of its four pixel rows)"""
    return 16 if name == "rgba" else _lib.BLOCK_BYTES[TARGETS[name]]


def rows_per_block(name):
    return 4 if name == "rgba" else 1


class Books:
    """both codebooks on the host and on the device"""

    def __init__(self, oracle):
        import torch
        from basisu_rs_amd import synth

        self.ep, rows = synth.etc1s_codebooks(N_EP, N_SEL)
        self.sel = oracle.selectors_from_rows(rows)  # 8-byte entries: texel rows and ETC1 selector bytes
        self.d_ep = torch.from_numpy(self.ep.view(np.int32)).cuda()
        self.d_sel = torch.from_numpy(self.sel.reshape(-1)).cuda()


class Slice:
    """a slice pair (colour and alpha indices) in device memory between bands of out-of-range indices, and what every target makes of it with and without
    the alpha slice: want[name, alpha] of shape (blocks, block bytes), a block of RGBA32 as its four pixel rows"""

    def __init__(self, oracle, books, nbx, seed):
        import test_etc1s_targets as tet

        rng = np.random.default_rng(seed)
        self.nbx, self.n = nbx, nbx * NBY
        self.idx = (rng.integers(0, N_EP, self.n) | (rng.integers(0, N_SEL, self.n) << 16)).astype(np.uint32)
        self.aidx = (rng.integers(0, N_EP, self.n) | (rng.integers(0, N_SEL, self.n) << 16)).astype(np.uint32)
        self.want = {("etc1", False): oracle.etc1s_to_etc1(self.idx, books.ep, books.sel).reshape(self.n, 8)}
        for alpha in (False, True):
            # (one block per row of a 4-pixel-wide image: 64 consecutive bytes per block, pixel row by pixel row)
            rgba = oracle.etc1s_to_rgba(self.idx, self.aidx if alpha else None, 1, self.n, books.ep, books.sel).reshape(self.n, 64)
            self.want["rgba", alpha] = rgba
            for name in tet.TARGETS:
                self.want[name, alpha] = tet.model(name, rgba)
        self.upload(self.idx, self.aidx)

    def upload(self, idx, aidx):
        import torch

        def banded(a):
            t = torch.full((self.n + 2 * BAND,), -1, dtype=torch.int32, device="cuda")
            t[BAND:BAND + self.n] = torch.from_numpy(a.view(np.int32)).cuda()
            return t

        self._d_idx, self._d_aidx = banded(idx), banded(aidx)
        self.d_idx, self.d_aidx = self._d_idx.data_ptr() + 4 * BAND, self._d_aidx.data_ptr() + 4 * BAND

    def rect(self, name, alpha, x0, y0, w, h, zero=()):
        """the bytes of the rectangle's surface rows, tight: (h * rows per block, w * row bytes); zero: slice indices of blocks that must be all zeros"""
        y, x = np.meshgrid(np.arange(y0, y0 + h), np.arange(x0, x0 + w), indexing="ij")
        want = self.want[name, alpha]
        if len(zero):
            want = want.copy()
            want[list(zero)] = 0
        b = want[y * self.nbx + x]  # (h, w, block bytes)
        if name == "rgba":
            return b.reshape(h, w, 4, 16).transpose(0, 2, 1, 3).reshape(4 * h, 16 * w)
        return b.reshape(h, -1)


@pytest.fixture(scope="module")
def books(oracle):
    return Books(oracle)


@pytest.fixture(scope="module")
def slices(oracle, books):
    return [Slice(oracle, books, nbx, seed=1000 + nbx) for nbx in WIDTHS]


class Surfaces:
    """one poisoned surface per job, each between guard bands; jobs: (slice, alpha, x0, y0, w, h, pitch, index_base)"""

    def __init__(self, name, jobs, zero=()):
        import torch

        self.name, self.jobs, self.zero = name, jobs, zero
        rpb = rows_per_block(name)
        self.sizes = [rpb * h * pitch for (_, _, _, _, _, h, pitch, _) in jobs]
        self.mem = [torch.empty(n + 2 * GUARD, dtype=torch.uint8, device="cuda") for n in self.sizes]
        self.poison()

    def poison(self):
        for m in self.mem:
            m.fill_(POISON)

    def ptr(self, i):
        return self.mem[i].data_ptr() + GUARD

    def table(self):
        return [(s.d_idx, s.d_aidx if alpha else None, s.nbx, x0, y0, w, h, self.ptr(i), pitch, base)
                for i, (s, alpha, x0, y0, w, h, pitch, base) in enumerate(self.jobs)]

    def check(self, untouched=False):
        rb, rpb = row_bytes(self.name), rows_per_block(self.name)
        for i, (s, alpha, x0, y0, w, h, pitch, _) in enumerate(self.jobs):
            all_bytes = self.mem[i].cpu().numpy()
            assert (all_bytes[:GUARD] == POISON).all() and (all_bytes[GUARD + self.sizes[i]:] == POISON).all(), "job %d: a guard band was written" % i
            got = all_bytes[GUARD:GUARD + self.sizes[i]].reshape(rpb * h, pitch)
            if untouched:
                assert (got == POISON).all(), "job %d: something was written" % i
                continue
            want = s.rect(self.name, alpha, x0, y0, w, h, self.zero)
            assert np.array_equal(got[:, :w * rb], want), "job %d (%d, %d, %d, %d) pitch %d: the rectangle's bytes differ" % (i, x0, y0, w, h, pitch)
            assert (got[:, w * rb:] == POISON).all(), "job %d (%d, %d, %d, %d) pitch %d: padding was written" % (i, x0, y0, w, h, pitch)


def pitches(name, w):
    rb = row_bytes(name)
    return {"tight": w * rb, "padded": -(-(w * rb + rb + 48) // rb) * rb, "4096": max(4096, w * rb)}


def status_word():
    import torch

    return torch.zeros(1, dtype=torch.int64, device="cuda")


def word_of(st):
    return int(st.item()) & (2**64 - 1)


def run(ctx, books, name, surf, st=None, stream=None, table=None):
    ctx.etc1s_transcode_rects_device(TARGETS[name], surf.table() if table is None else table, books.d_ep, N_EP, books.d_sel, N_SEL, d_status=st, stream=stream)


# (ETC1 has no alpha: the call refuses an alpha slice, test_argument_rules_and_nothing_launched)
@pytest.mark.parametrize("pitch", ["tight", "padded", "4096"])
@pytest.mark.parametrize("name,alpha", [(n, a) for n in TARGETS for a in (False, True) if not (n == "etc1" and a)],
                         ids=lambda v: v if isinstance(v, str) else ("alpha" if v else "opaque"))
def test_twelve_rectangles_in_one_call(ctx, books, slices, name, alpha, pitch):
    import torch

    s = slices[0]
    surf = Surfaces(name, [(s, alpha, x0, y0, w, h, pitches(name, w)[pitch], 0) for (x0, y0, w, h) in RECTS])
    st = status_word()
    ctx.status_word_reset(st)
    run(ctx, books, name, surf, st)
    torch.cuda.synchronize()
    surf.check()
    assert word_of(st) == CLEAR  # (nothing of the out-of-range indices around the slice was taken)


@pytest.mark.parametrize("name", list(TARGETS))
def test_150_jobs_from_three_slices_in_one_call(ctx, books, slices, name):
    """more jobs than one launch's table holds at any table size the kernel arguments allow: several launches on the stream, in order"""
    import torch

    rng = np.random.default_rng(150)
    rb, jobs = row_bytes(name), []
    for i in range(150):
        s = slices[i % 3]
        w, h = int(rng.integers(1, min(40, s.nbx) + 1)), int(rng.integers(1, 41))
        x0, y0 = int(rng.integers(0, s.nbx - w + 1)), int(rng.integers(0, NBY - h + 1))
        jobs.append((s, name != "etc1" and (i // 3) % 2 == 1, x0, y0, w, h, w * rb + rb * int(rng.choice([0, 1, 5])), 1000 * i))
    surf = Surfaces(name, jobs)
    st = status_word()
    ctx.status_word_reset(st)
    run(ctx, books, name, surf, st)
    torch.cuda.synchronize()
    surf.check()
    assert word_of(st) == CLEAR


STATUS_RECTS = ((5, 1, 63, 15, 70000), (64, 16, 64, 16, 0), (11, 25, 32, 10, 1 << 40))


@pytest.mark.parametrize("name", ["bc1", "bc4", "etc1", "rgba", "rg11"])
def test_status_word(ctx, oracle, books, slices, name):
    """a bad endpoint index inside two jobs and a bad selector index further on: the word names the lowest index_base + slice index with BU_ERR_INDEX_RANGE and
    the failing blocks are zeros; a bad ALPHA index is reported by targets that do not read A; a bad index that lies in no rectangle is not reported"""
    import torch

    base = slices[0]
    in_a, in_b, further, outside = 9 * NBX + 30, 20 * NBX + 100, 22 * NBX + 110, 38 * NBX + 199  # (30, 9) in job 0; (100, 20), (110, 22) in job 1; (199, 38) in none
    cases = [("colour", (in_a, in_b), (further,), (outside,), (), (0 + in_b) << 8 | _lib.ERR_INDEX_RANGE),
             ("outside", (), (), (outside,), (), CLEAR),
             ("job0", (in_a,), (), (outside,), (), (70000 + in_a) << 8 | _lib.ERR_INDEX_RANGE)]
    if name != "etc1":
        cases.append(("alpha", (), (), (), (in_b,), (0 + in_b) << 8 | _lib.ERR_INDEX_RANGE))
    s = Slice.__new__(Slice)  # the same slice and expected bytes, with index arrays of its own
    s.nbx, s.n, s.want = base.nbx, base.n, base.want
    for what, bad_ep, bad_sel, bad_out, bad_alpha, want_word in cases:
        idx, aidx = base.idx.copy(), base.aidx.copy()
        for i in bad_ep + bad_out:
            idx[i] = (idx[i] & 0xFFFF0000) | N_EP           # endpoint index one past the codebook
        for i in bad_sel:
            idx[i] = (idx[i] & 0xFFFF) | (N_SEL << 16)      # selector index one past the codebook
        for i in bad_alpha:
            aidx[i] = (aidx[i] & 0xFFFF) | (N_SEL << 16)
        s.upload(idx, aidx)
        alpha = name != "etc1"
        zero = bad_ep + bad_sel + bad_alpha
        surf = Surfaces(name, [(s, alpha, x0, y0, w, h, pitches(name, w)["padded"], b) for (x0, y0, w, h, b) in STATUS_RECTS], zero=zero)
        st = status_word()
        ctx.status_word_reset(st)
        run(ctx, books, name, surf, st)
        torch.cuda.synchronize()
        assert word_of(st) == want_word, what
        surf.check()
        # without a status word the same call writes the same bytes
        surf.poison()
        run(ctx, books, name, surf)
        torch.cuda.synchronize()
        surf.check()


def test_argument_rules_and_nothing_launched(ctx, books, slices):
    import torch

    from basisu_rs_amd import BasisuError

    s = slices[0]
    lib = _lib.load()
    for name in ("bc1", "etc1", "rgba", "rg11"):
        rb, alpha = row_bytes(name), name != "etc1"
        surf = Surfaces(name, [(s, alpha, x0, y0, w, h, pitches(name, w)["padded"], 0) for (x0, y0, w, h) in RECTS[1:5]])
        good = surf.table()

        def refused(last, target=TARGETS[name], d_ep=books.d_ep, d_sel=books.d_sel):
            with pytest.raises(BasisuError) as e:
                ctx.etc1s_transcode_rects_device(target, good[:-1] + [tuple(last)], d_ep, N_EP, d_sel, N_SEL)
            assert e.value.status == _lib.ERR_ARGUMENT
            torch.cuda.synchronize()
            surf.check(untouched=True)  # a bad argument in the LAST job: the jobs in front of it were not launched either

        d_idx, d_aidx, bpr, x0, y0, w, h, d_out, pitch, base = good[-1]
        refused((0, d_aidx, bpr, x0, y0, w, h, d_out, pitch, base))
        refused((d_idx, d_aidx, bpr, x0, y0, w, h, 0, pitch, base))
        refused((d_idx, d_aidx, bpr, x0, y0, 0, h, d_out, pitch, base))
        refused((d_idx, d_aidx, bpr, x0, y0, w, 0, d_out, pitch, base))
        refused((d_idx, d_aidx, 0, 0, y0, w, h, d_out, pitch, base))
        refused((d_idx, d_aidx, bpr, bpr - w + 1, y0, w, h, d_out, pitch, base))           # x0 + w > in_blocks_per_row
        refused((d_idx, d_aidx, 1 << 21, 0, 2048 - h + 1, w, h, d_out, pitch, base))      # (y0 + h) * in_blocks_per_row one block row past 2^32
        refused((d_idx + 2, d_aidx, bpr, x0, y0, w, h, d_out, pitch, base))               # d_idx not 4-byte aligned
        if alpha:
            refused((d_idx, d_aidx + 2, bpr, x0, y0, w, h, d_out, pitch, base))           # nor d_alpha_idx
        else:
            refused((d_idx, s.d_aidx, bpr, x0, y0, w, h, d_out, pitch, base))             # ETC1 has no alpha
        refused((d_idx, d_aidx, bpr, x0, y0, w, h, d_out + rb // 2, pitch, base))         # d_out no multiple of the row bytes
        refused((d_idx, d_aidx, bpr, x0, y0, w, h, d_out, pitch + rb // 2, base))         # nor the pitch
        refused((d_idx, d_aidx, bpr, x0, y0, w, h, d_out, w * rb - rb, base))             # pitch below the row
        refused(good[-1], d_ep=None)
        refused(good[-1], d_sel=None)
        for t in (0, 1, 3, 5, 10, 13):
            refused(good[-1], target=t)
        args = (books.d_ep.data_ptr(), N_EP, books.d_sel.data_ptr(), N_SEL, None, None)
        assert lib.bu_etc1s_transcode_rects_device(ctx.handle, TARGETS[name], 2, None, *args) == _lib.ERR_ARGUMENT
        assert lib.bu_etc1s_transcode_rects_device(ctx.handle, TARGETS[name], 0, None, *args) == _lib.OK  # a no-op
        ctx.etc1s_transcode_rects_device(TARGETS[name], [], books.d_ep, N_EP, books.d_sel, N_SEL)
        torch.cuda.synchronize()
        surf.check(untouched=True)
        run(ctx, books, name, surf)  # and the same table, unharmed, works on the same context
        torch.cuda.synchronize()
        surf.check()


@pytest.mark.parametrize("name", ["bc3", "etc1", "rgba"])
def test_a_three_job_call_is_captured_into_a_graph_and_replayed(ctx, books, slices, name):
    """the call only enqueues: recorded by (linear) stream capture as tests/test_gpu_rects.py does it, replayed twice into re-poisoned surfaces"""
    import torch

    alpha = name != "etc1"
    surf = Surfaces(name, [(slices[0], alpha and k != 1, x0, y0, w, h, pitches(name, w)["padded"], 5000 * k) for k, (x0, y0, w, h) in enumerate(RECTS[2:5])])
    st = status_word()
    side = torch.cuda.Stream()
    table = surf.table()

    def record():
        ctx.status_word_reset(st, stream=side)
        run(ctx, books, name, surf, st, stream=side, table=table)

    with torch.cuda.stream(side):
        record()  # (first use outside the capture)
    torch.cuda.synchronize()
    surf.check()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        record()
    del table  # (the job array travelled in the kernel arguments: nothing of it is read at replay)
    first = None
    for _ in range(2):
        surf.poison()
        st.fill_(0)
        graph.replay()
        torch.cuda.synchronize()
        surf.check()
        assert word_of(st) == CLEAR
        got = [m.cpu().numpy().copy() for m in surf.mem]
        if first is None:
            first = got
        assert all(np.array_equal(a, b) for a, b in zip(first, got))


@pytest.mark.parametrize("name", list(TARGETS))
def test_one_job_over_a_whole_slice_equals_the_plain_call(ctx, books, slices, name):
    """one job over the whole slice at the tight pitch against the whole-slice device call, byte for byte, the status word included"""
    import torch

    base = slices[0]
    s = Slice.__new__(Slice)
    s.nbx, s.n, s.want = base.nbx, base.n, base.want
    idx = base.idx.copy()
    bad = 17 * NBX + 5
    idx[bad] = (idx[bad] & 0xFFFF) | (N_SEL << 16)
    s.upload(idx, base.aidx)
    t, rb, alpha = TARGETS[name], row_bytes(name), name != "etc1"
    n_out = s.n * _lib.BLOCK_BYTES[t]
    plain = torch.full((n_out,), POISON, dtype=torch.uint8, device="cuda")
    rects = torch.full((n_out,), POISON, dtype=torch.uint8, device="cuda")
    st_a, st_b = status_word(), status_word()
    ctx.status_word_reset(st_a)
    ctx.status_word_reset(st_b)
    lib, stream = _lib.load(), torch.cuda.current_stream().cuda_stream
    cb = (books.d_ep.data_ptr(), N_EP, books.d_sel.data_ptr(), N_SEL)
    if name == "etc1":
        assert lib.bu_etc1s_transcode_etc1_device(ctx.handle, s.d_idx, s.n, *cb, plain.data_ptr(), st_a.data_ptr(), stream) == _lib.OK
    elif name == "rgba":
        assert lib.bu_etc1s_decode_rgba_device(ctx.handle, s.d_idx, s.d_aidx, NBX, NBY, *cb, plain.data_ptr(), st_a.data_ptr(), stream) == _lib.OK
    else:
        ctx.etc1s_transcode_device(t, s.d_idx, s.d_aidx, s.n, books.d_ep, N_EP, books.d_sel, N_SEL, plain, st_a)
    ctx.etc1s_transcode_rects_device(t, [(s.d_idx, s.d_aidx if alpha else None, NBX, 0, 0, NBX, NBY, rects, NBX * rb, 0)], books.d_ep, N_EP, books.d_sel, N_SEL, d_status=st_b)
    torch.cuda.synchronize()
    assert torch.equal(plain, rects)
    assert word_of(st_a) == word_of(st_b) == bad << 8 | _lib.ERR_INDEX_RANGE
