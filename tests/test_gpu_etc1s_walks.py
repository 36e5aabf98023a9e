"""ETC1S launches whose waves take a second and a third step of their grid-stride loop (the cases of tests/etc1s_walk_cases.py; tests/test_etc1s_walk_cases.py
holds without a GPU that they walk, and every test here asserts the case's condition again for the CU count of the device it runs on):

1. bu_etc1s_transcode_rects_device, all eight targets: one launch over three ragged rounds whose wave slots step across jobs of different unit shape, source
   pitch and surface pitch; two walking launches in one call; the status word from a third-round unit; graph capture and replay.
2. bu_read_to / bu_read_file_to through the one-launch door: files of thousands of tiny images, more than two rounds of units, with and without alpha.
3. The slice kernels over several rounds: the staged ETC1 kernel's four-blocks-per-lane path (the carry of the prefetched index words into the next step), and
   the L2-gather kernels with codebooks of 24 000 + 24 000 entries -- (24 000 + 24 000 + 256) * 4 = 193 024 bytes, more than the 155 648 bytes of LDS the staged
   kernels may take (BU_ETC1S_LDS_MAX), so bu_etc1s_shape cannot stage them and the gather serves every size.

Expected bytes come from outside the code under test: oracle.etc1s_to_etc1, oracle.etc1s_to_rgba, oracle.read_to, and the numpy models of the six block targets
(test_etc1s_targets.model) applied to the oracle's RGBA32.  Large index arrays draw their words from a pool of 16 384 distinct colour / alpha pairs in a
scrambled order; the pool is modelled once and gathered.  Every output byte is compared: surfaces and flat outputs lie between the guard bands of
tests/gpu_guard.py and are pre-filled with a poison byte, index arrays lie between bands of out-of-range index words."""
import os

import numpy as np
import pytest

import basis_builder as bb
import etc1s_walk_cases as wc
import gpu_guard as gg
import test_etc1s_targets as tet
from basisu_rs_amd import _lib, read_file_query, read_file_to, read_header, read_query, read_slice_descs, read_to_etc1, read_to_rgba, synth

pytestmark = pytest.mark.gpu
NAMES = tuple(wc.TARGETS)
SIX = tuple(tet.TARGETS)
POISON = 0xAB
CLEAR = _lib.STATUS_WORD_CLEAR
M = wc.POOL


@pytest.fixture(scope="module")
def cu(ctx):
    """the CU count the context hands to bu_grid_for (bu_context_create: hipDeviceProp_t::multiProcessorCount)"""
    import torch

    return torch.cuda.get_device_properties(0).multi_processor_count


def _word(st):
    return int(st.item()) & CLEAR


def _status():
    import torch

    return torch.zeros(1, dtype=torch.int64, device="cuda")


def _i32(a):
    import torch

    return torch.from_numpy(np.ascontiguousarray(a).view(np.int32)).cuda()


def _differs(got, want):
    """None, or where two device byte tensors of the same shape differ first"""
    import torch

    if torch.equal(got, want):
        return None
    bad = torch.nonzero(got.reshape(-1) != want.reshape(-1))[:, 0]
    k = int(bad[0].item())
    return "%d bytes differ, first at %d: %d against %d" % (bad.numel(), k, int(got.reshape(-1)[k].item()), int(want.reshape(-1)[k].item()))


# ---- the pool ---------------------------------------------------------------------------------------------------------------------
class Pool:
    """codebooks of 24 000 + 24 000 entries, M colour / alpha index pairs, and what every target makes of the M pairs with and without the alpha slice: row M of
    every table is a block of zeros, what a failing block is written as.  Modelled on first use, kept on the device."""

    def __init__(self, oracle):
        import torch

        self.oracle = oracle
        self.ep, rows = synth.etc1s_codebooks(wc.N_EP, wc.N_SEL, seed=wc.N_EP + 1)
        rng = np.random.default_rng(24001)
        q = wc.N_SEL // 4   # a quarter of the entries draw their texels from a few selectors only (solid and two-colour blocks)
        rows[:q] = tet.rows_from(rng, q).astype("<u4").view(np.uint8).reshape(q, 4)
        self.sel = oracle.selectors_from_rows(rows)
        self.idx = (rng.integers(0, wc.N_EP, M) | (rng.integers(0, wc.N_SEL, M) << 16)).astype(np.uint32)
        self.aidx = (rng.integers(0, wc.N_EP, M) | (rng.integers(0, wc.N_SEL, M) << 16)).astype(np.uint32)
        self.idx[-1] = (wc.N_EP - 1) | ((wc.N_SEL - 1) << 16)   # the last entry of both codebooks
        self.aidx[-2] = (wc.N_EP - 1) | ((wc.N_SEL - 1) << 16)
        self.d_ep = torch.from_numpy(self.ep.view(np.int32)).cuda()
        self.d_sel = torch.from_numpy(self.sel.reshape(-1)).cuda()
        self._rgba, self._want = {}, {}

    def rgba(self, alpha):
        if alpha not in self._rgba:
            self._rgba[alpha] = self.oracle.etc1s_to_rgba(self.idx, self.aidx if alpha else None, 1, M, self.ep, self.sel).reshape(M, 64)
        return self._rgba[alpha]

    def want(self, name, alpha):
        """(M + 1, block bytes) on the device; RGBA32 blocks as their four pixel rows of 16 bytes"""
        import torch

        alpha = bool(alpha) and name != "etc1"
        if (name, alpha) not in self._want:
            w = self.oracle.etc1s_to_etc1(self.idx, self.ep, self.sel).reshape(M, 8) if name == "etc1" else self.rgba(alpha) if name == "rgba" else \
                tet.model(name, self.rgba(alpha))
            assert w.shape == (M, wc.BLOCK_BYTES[name])
            self._want[name, alpha] = torch.from_numpy(np.concatenate([w, np.zeros((1, w.shape[1]), np.uint8)])).cuda()
        return self._want[name, alpha]


@pytest.fixture(scope="module")
def pool(oracle):
    return Pool(oracle)


def _bad_endpoint(word):
    return (int(word) & 0xFFFF0000) | wc.N_EP           # endpoint index one past the codebook


def _bad_selector(word):
    return (int(word) & 0xFFFF) | (wc.N_SEL << 16)      # selector index one past the codebook


# ---- 1. rectangles ----------------------------------------------------------------------------------------------------------------
class Slices:
    """the slices of a job table in device memory between bands of out-of-range index words (0xFFFFFFFF: a lane that took a block outside its slice would
    report it); p[s]: the pool entry of every block, (rows, blocks per row); planted: status_blocks of the table, or None"""

    def __init__(self, pool, slices, planted=None):
        import torch

        self.p = [wc.pool_order(b * r, salt=s).reshape(r, b) for s, (b, r) in enumerate(slices)]
        self.planted = planted
        idx, aidx = [pool.idx[p.reshape(-1)] for p in self.p], [pool.aidx[p.reshape(-1)] for p in self.p]
        if planted:
            for key, words, bad in (("endpoint", idx, _bad_endpoint), ("selector", idx, _bad_selector), ("outside", idx, _bad_endpoint), ("alpha", aidx, _bad_selector)):
                s, sidx = planted[key]
                words[s][sidx] = bad(words[s][sidx])
        sizes = [4 * b * r for b, r in slices]
        self.a_idx = gg.Arena("indices", sizes, gg.POISON_BLOCKS * 4, 0, fill="ones")
        self.a_aidx = gg.Arena("alpha indices", sizes, gg.POISON_BLOCKS * 4, 0, fill="ones")
        for s in range(len(slices)):
            self.a_idx.data(s).view(torch.int32)[:] = _i32(idx[s])
            self.a_aidx.data(s).view(torch.int32)[:] = _i32(aidx[s])
        self.idx_ptrs = [self.a_idx.ptr(s) for s in range(len(slices))]
        self.aidx_ptrs = [self.a_aidx.ptr(s) for s in range(len(slices))]

    def region(self, name, j, slices):
        """the pool entries of a job's rectangle, (h, w); M where the job's block fails"""
        reg = self.p[j["slice"]][j["y0"]:j["y0"] + j["h"], j["x0"]:j["x0"] + j["w"]]
        if self.planted:
            reg = reg.copy()
            for key in ("endpoint", "selector", "outside") + (("alpha",) if j["alpha"] and name != "etc1" else ()):
                s, sidx = self.planted[key]
                y, x = divmod(sidx, slices[s][0])
                if s == j["slice"] and j["y0"] <= y < j["y0"] + j["h"] and j["x0"] <= x < j["x0"] + j["w"]:
                    reg[y - j["y0"], x - j["x0"]] = M
        return reg


class Surfaces:
    """one poisoned surface per job, a guard band in front of, between and behind them"""

    def __init__(self, name, jobs):
        self.name, self.jobs = name, jobs
        self.arena = gg.Arena(name + " surfaces", [wc.surface_bytes(name, j) for j in jobs], gg.guard_bytes(wc.BLOCK_BYTES[name], wc.UNIT), 0)
        self.ptrs = [self.arena.ptr(i) for i in range(len(jobs))]
        self.poison()

    def poison(self):
        for i in range(len(self.jobs)):
            self.arena.data(i).fill_(POISON)

    def check(self, pool, src, slices):
        """every byte of every surface: the rectangle's blocks at the job's pitch, the padding still poison; and the guard bands"""
        import torch

        name = self.name
        rb, rpb = wc.row_bytes(name), wc.rows_per_block(name)
        for i, j in enumerate(self.jobs):
            want = pool.want(name, j["alpha"])
            reg = torch.from_numpy(np.ascontiguousarray(src.region(name, j, slices))).cuda()
            b = want[reg]   # (h, w, block bytes)
            if name == "rgba":
                b = b.reshape(j["h"], j["w"], 4, 16).permute(0, 2, 1, 3)
            pitch = wc.pitch_of(name, j)
            exp = torch.full((rpb * j["h"], pitch), POISON, dtype=torch.uint8, device="cuda")
            exp[:, :j["w"] * rb] = b.reshape(rpb * j["h"], j["w"] * rb)
            miss = _differs(self.arena.data(i).reshape(rpb * j["h"], pitch), exp)
            assert miss is None, "job %d (%d x %d at %d, %d of slice %d, pitch %d): %s" % (i, j["w"], j["h"], j["x0"], j["y0"], j["slice"], pitch, miss)
        self.arena.check()

    def snapshot(self):
        return self.arena.buf.clone()


@pytest.fixture(scope="module")
def rect_inputs(pool, cu):
    """(jobs, slices, Slices) per case, built on first use; "status": three_rounds with the planted blocks"""
    made = {}

    def get(case):
        if case not in made:
            jobs, slices = wc.RECT_CASES["three_rounds" if case == "status" else case](cu)
            made[case] = (jobs, slices, Slices(pool, slices, wc.status_blocks(jobs, slices) if case == "status" else None))
        return made[case]

    return get


def _run_rects(ctx, pool, name, jobs, slices, src, surf, st=None, stream=None):
    table = wc.job_table(name, jobs, slices, src.idx_ptrs, src.aidx_ptrs, surf.ptrs)
    table = [row[:1] + (row[1] or None,) + row[2:] for row in table]
    ctx.etc1s_transcode_rects_device(wc.TARGETS[name], table, pool.d_ep, wc.N_EP, pool.d_sel, wc.N_SEL, d_status=st, stream=stream)


def _check_inputs(src):
    src.a_idx.check()
    src.a_aidx.check()


@pytest.mark.parametrize("case", ["three_rounds", "two_launches"])
@pytest.mark.parametrize("name", NAMES)
def test_rectangle_launches_that_walk(ctx, pool, cu, rect_inputs, name, case):
    """three_rounds: one launch of 64 jobs over two whole rounds and a ragged third; two_launches: three more jobs, a second launch over more than a round"""
    import torch

    assert wc.rect_condition(case, cu) is None
    jobs, slices, src = rect_inputs(case)
    surf = Surfaces(name, jobs)
    st = _status()
    ctx.status_word_reset(st)
    _run_rects(ctx, pool, name, jobs, slices, src, surf, st)
    torch.cuda.synchronize()
    surf.check(pool, src, slices)
    assert _word(st) == CLEAR   # (nothing of the out-of-range words around the slices was taken)
    _check_inputs(src)


@pytest.mark.parametrize("name", ["bc1", "bc4", "etc1", "rgba", "rg11"])
def test_status_word_from_a_third_round_unit(ctx, pool, cu, rect_inputs, name):
    """a bad endpoint index in a unit of the third round (a late job: the lowest index base), a bad selector index in a first-round unit of an early job, a bad
    alpha index in a second-round unit (reported by targets that do not read A; ETC1 takes no alpha slice), a bad index in a row no job takes (not reported):
    the word names the lowest index_base + slice index with BU_ERR_INDEX_RANGE, the failing blocks are zeros, and without a status word the same call writes
    the same bytes"""
    import torch

    assert wc.rect_condition("three_rounds", cu) is None and wc.status_condition(cu) is None
    jobs, slices, src = rect_inputs("status")
    surf = Surfaces(name, jobs)
    st = _status()
    ctx.status_word_reset(st)
    _run_rects(ctx, pool, name, jobs, slices, src, surf, st)
    torch.cuda.synchronize()
    assert _word(st) == (wc.lowest_status_index(name, jobs, slices, src.planted) << 8) | _lib.ERR_INDEX_RANGE
    surf.check(pool, src, slices)
    surf.poison()
    _run_rects(ctx, pool, name, jobs, slices, src, surf)
    torch.cuda.synchronize()
    surf.check(pool, src, slices)
    _check_inputs(src)


@pytest.mark.parametrize("name", ["bc3", "etc1", "rgba"])
def test_three_rounds_captured_into_a_graph_and_replayed(ctx, pool, cu, rect_inputs, name):
    """the call only enqueues: recorded by (linear) stream capture as tests/test_gpu_etc1s_rects.py does it, replayed twice into re-poisoned surfaces"""
    import torch

    assert wc.rect_condition("three_rounds", cu) is None
    jobs, slices, src = rect_inputs("three_rounds")
    surf = Surfaces(name, jobs)
    st = _status()
    side = torch.cuda.Stream()

    def record():
        ctx.status_word_reset(st, stream=side)
        _run_rects(ctx, pool, name, jobs, slices, src, surf, st, stream=side)

    with torch.cuda.stream(side):
        record()  # (first use outside the capture)
    torch.cuda.synchronize()
    surf.check(pool, src, slices)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        record()
    first = None
    for _ in range(2):
        surf.poison()
        st.fill_(0)
        graph.replay()
        torch.cuda.synchronize()
        surf.check(pool, src, slices)
        assert _word(st) == CLEAR
        got = surf.snapshot()
        if first is None:
            first = got
        assert torch.equal(first, got)


# ---- 2. whole files ---------------------------------------------------------------------------------------------------------------
class WalkFile:
    """a file of file_dims(cu) images and what the oracle reads from it: RGBA32 and ETC1 images, and the RGBA32 blocks of all images in one array"""

    def __init__(self, oracle, dims, alpha):
        self.dims, self.alpha = dims, alpha
        self.data = bb.etc1s_file(np.random.default_rng(7000 + alpha), dims, n_codebook=wc.FILE_CODEBOOK, alpha=alpha)[0]
        st, _, self.rgba = oracle.read_to("rgba", self.data)
        assert st == 0 and len(self.rgba) == len(dims)
        st, _, self.etc1 = oracle.read_to("etc1", self.data)
        assert st == 0
        descs = read_slice_descs(self.data, read_header(self.data))
        step = 2 if alpha else 1
        assert len(descs) == step * len(dims)
        blocks = []
        for k, ((nbx, nby), (_, _, _, data)) in enumerate(zip(dims, self.rgba)):
            d = descs[step * k]
            assert (d.num_blocks_x, d.num_blocks_y) == (nbx, nby) and data.size == nbx * nby * 64
            blocks.append(data.reshape(nby, 4, nbx, 4, 4).transpose(0, 2, 1, 3, 4).reshape(-1, 64))  # image -> blocks
        self.blocks = np.concatenate(blocks)
        self.sizes = [(d.orig_width, d.orig_height) for d in descs[::step]]
        self._model = {}

    def want(self, name):
        """[(w, h, stride, bytes)] of every image"""
        if name == "rgba":
            return [(w, h, s, d.tobytes()) for w, h, s, d in self.rgba]
        if name == "etc1":
            return [(w, h, s, d.tobytes()) for w, h, s, d in self.etc1]
        if name not in self._model:
            bb_ = wc.BLOCK_BYTES[name]
            m, out, at = tet.model(name, self.blocks), [], 0
            for (nbx, nby), (w, h) in zip(self.dims, self.sizes):
                out.append((w, h, bb_ * nbx, m[at:at + nbx * nby].tobytes()))
                at += nbx * nby
            assert at == m.shape[0]
            self._model[name] = out
        return self._model[name]


@pytest.fixture(scope="module")
def walk_files(oracle, cu):
    made = {}

    def get(alpha):
        if alpha not in made:
            made[alpha] = WalkFile(oracle, wc.file_dims(cu), alpha)
        return made[alpha]

    return get


def _read(name, f, ctx, out=None):
    """through the one-launch door (as tests/test_gpu_read_file_targets.py pins it)"""
    os.environ["BU_ETC1S_ONE_LAUNCH"] = "1"
    try:
        if name == "etc1":
            return read_to_etc1(f, ctx, out=out)
        if name == "rgba":
            return read_to_rgba(f, ctx, out=out)[1]
        return read_file_to(wc.TARGETS[name], f, ctx, out=out)
    finally:
        os.environ.pop("BU_ETC1S_ONE_LAUNCH", None)


def _tuples(imgs):
    return [(g.w, g.h, g.stride, g.data.tobytes()) for g in imgs]


@pytest.mark.parametrize("alpha", [True, False], ids=["alpha", "opaque"])
@pytest.mark.parametrize("name", NAMES)
def test_files_of_many_tiny_images_walk_the_one_launch_door(ctx, cu, walk_files, name, alpha):
    """bu_etc1s_file_kernel<false> (etc1), <true> (rgba) and bu_etc1s_file_target_kernel (the six): every image's (w, h, stride) and bytes, into a guarded
    buffer of exactly the queried size"""
    assert wc.file_condition(cu) is None
    wf = walk_files(alpha)
    n_units = sum((nbx * nby + 63) // 64 for nbx, nby in wf.dims if nbx * nby)   # the one-launch door: ceil(blocks / 64) per non-empty image
    assert n_units > 2 * wc.round_units(cu) and n_units % wc.round_units(cu) != 0
    want = wf.want(name)
    n_img, nbytes = read_query(_lib.READ_ETC1 if name == "etc1" else _lib.READ_RGBA, wf.data) if name in ("etc1", "rgba") else read_file_query(wc.TARGETS[name], wf.data)
    assert (n_img, nbytes) == (len(want), sum(len(w[3]) for w in want))
    for where in ("pageable",) + (("pinned",) if name == "bc1" else ()):   # (page-locked: the kernel stores into it directly)
        a = gg.Arena("%s file out (%s)" % (name, where), nbytes, gg.guard_bytes(wc.BLOCK_BYTES[name], wc.UNIT), 0, where=where, ctx=ctx)
        try:
            a.data()[:] = POISON
            got = _tuples(_read(name, wf.data, ctx, out=a.data()))
            a.check()
        finally:
            a.free()
        assert len(got) == len(want)
        bad = [k for k, (g, w) in enumerate(zip(got, want)) if g != w]
        assert not bad, "%s %s: %d images differ, first %d (%s blocks): %s against %s" % (name, where, len(bad), bad[0], wf.dims[bad[0]], got[bad[0]][:3], want[bad[0]][:3])


# ---- 3. slice kernels -------------------------------------------------------------------------------------------------------------
def _flat_call(ctx, name, d_idx, d_aidx, n, nbx, d_ep, n_ep, d_sel, n_sel, d_out, d_st):
    import torch

    lib, stream = ctx._lib, torch.cuda.current_stream().cuda_stream
    if name == "etc1":
        return lib.bu_etc1s_transcode_etc1_device(ctx.handle, d_idx, n, d_ep, n_ep, d_sel, n_sel, d_out, d_st, stream)
    if name == "rgba":
        return lib.bu_etc1s_decode_rgba_device(ctx.handle, d_idx, d_aidx, nbx, n // nbx, d_ep, n_ep, d_sel, n_sel, d_out, d_st, stream)
    return lib.bu_etc1s_transcode_device(ctx.handle, wc.TARGETS[name], d_idx, d_aidx, n, d_ep, n_ep, d_sel, n_sel, d_out, d_st, stream)


@pytest.fixture(scope="module")
def staged(oracle, cu):
    """codebooks of 4096 + 8192 entries, random index words of staged_case(cu) blocks, and the oracle's ETC1 of them"""
    c = wc.staged_case(cu)
    ep, rows = synth.etc1s_codebooks(wc.STAGED_EP, wc.STAGED_SEL, seed=4096)
    sel = oracle.selectors_from_rows(rows)
    rng = np.random.default_rng(8192)
    idx = (rng.integers(0, wc.STAGED_EP, c["n"]) | (rng.integers(0, wc.STAGED_SEL, c["n"]) << 16)).astype(np.uint32)
    idx[:wc.STAGED_EP] = (np.arange(wc.STAGED_EP) | (idx[:wc.STAGED_EP] & 0xFFFF0000)).astype(np.uint32)   # every endpoint, and the last selector
    idx[-1] = (wc.STAGED_EP - 1) | ((wc.STAGED_SEL - 1) << 16)
    return dict(c, ep=ep, sel=sel, idx=idx, want=oracle.etc1s_to_etc1(idx, ep, sel))


def test_staged_etc1_four_blocks_per_lane_over_three_steps(ctx, cu, staged):
    """bu_etc1s_staged_kernel<false> with the index array 8-byte and the output 16-byte aligned: 2 W + W / 2 + 3 chunks of 256 blocks on W = 16 cu waves and 77
    blocks more, so every wave carries prefetched index words into a second step and most into a third.  Then a bad selector index in a wave's third step (its
    lane 9's block + 129) and a bad endpoint index in a lower block of the same wave's second step: the word names the lower block, both are zeros, nothing
    else changes"""
    import torch

    assert wc.staged_condition(cu) is None
    n = staged["n"]
    a_idx = gg.Arena("indices", 4 * n, gg.POISON_BLOCKS * 4, 0, fill="ones")
    a_out = gg.Arena("etc1 output", 8 * n, gg.guard_bytes(8), 0)
    assert a_idx.ptr() % 8 == 0 and a_out.ptr() % 16 == 0   # what the four-blocks-per-lane path asks for
    d_ep, d_sel = _i32(staged["ep"]), torch.from_numpy(staged["sel"].reshape(-1)).cuda()
    want = torch.from_numpy(staged["want"]).cuda()
    lo, hi = staged["bad_endpoint"], staged["bad_selector"]
    idx = staged["idx"].copy()
    st = _status()
    for planted in (False, True):
        if planted:
            idx[hi] = (int(idx[hi]) & 0xFFFF) | (wc.STAGED_SEL << 16)
            idx[lo] = (int(idx[lo]) & 0xFFFF0000) | wc.STAGED_EP
            want = want.clone()
            want[8 * lo:8 * lo + 8] = 0
            want[8 * hi:8 * hi + 8] = 0
        a_idx.data().view(torch.int32)[:] = _i32(idx)
        a_out.data().fill_(POISON)
        ctx.status_word_reset(st)
        torch.cuda.synchronize()
        assert _flat_call(ctx, "etc1", a_idx.ptr(), None, n, 0, d_ep.data_ptr(), wc.STAGED_EP, d_sel.data_ptr(), wc.STAGED_SEL, a_out.ptr(), st.data_ptr()) == _lib.OK
        torch.cuda.synchronize()
        assert _word(st) == ((lo << 8) | _lib.ERR_INDEX_RANGE if planted else CLEAR)
        miss = _differs(a_out.data(), want)
        assert miss is None, "planted %s: %s" % (planted, miss)
        a_idx.check()
        a_out.check()


@pytest.mark.parametrize("name,alpha", [("etc1", False)] + [(n, a) for n in ("rgba",) + SIX for a in (False, True)],
                         ids=lambda v: v if isinstance(v, str) else ("alpha" if v else "opaque"))
def test_gather_kernels_over_three_rounds(ctx, pool, cu, name, alpha):
    """bu_etc1s_etc1_kernel, bu_etc1s_rgba_kernel (blocks per row no power of two: block rows straddle the rounds) and bu_etc1s_target_kernel<T, false> over
    2 B + B / 2 + 77 blocks, B = 8 cu x 256: clean; then with a bad selector index (the alpha slice's where there is one) in the last, partial round -- the
    word names it; then with a bad endpoint index in round one as well -- the word names that lower block.  Failing blocks are zeros, nothing else changes"""
    import torch

    assert wc.gather_condition(cu, name) is None
    c = wc.gather_case(cu, name)
    n, bb_ = c["n"], wc.BLOCK_BYTES[name]
    nbx = wc.RGBA_NBX if name == "rgba" else 0
    order = wc.pool_order(n, salt=5)
    idx, aidx = pool.idx[order], pool.aidx[order]
    a_idx = gg.Arena("indices", 4 * n, gg.POISON_BLOCKS * 4, 0, fill="ones")
    a_aidx = gg.Arena("alpha indices", 4 * n, gg.POISON_BLOCKS * 4, 0, fill="ones") if alpha else None
    a_out = gg.Arena(name + " output", bb_ * n, gg.guard_bytes(bb_), 0)
    d_order = torch.from_numpy(order).cuda()
    table = pool.want(name, alpha)
    st = _status()
    for planted in ((), ("late",), ("late", "early")):
        if "late" in planted:
            (aidx if alpha else idx)[c["late"]] = _bad_selector((aidx if alpha else idx)[c["late"]])
        if "early" in planted:
            idx[c["early"]] = _bad_endpoint(idx[c["early"]])
        for k in planted:
            d_order[c[k]] = M
        want = table[d_order]
        if name == "rgba":
            want = want.reshape(n // nbx, nbx, 4, 16).permute(0, 2, 1, 3)
        a_idx.data().view(torch.int32)[:] = _i32(idx)
        if alpha:
            a_aidx.data().view(torch.int32)[:] = _i32(aidx)
        a_out.data().fill_(POISON)
        ctx.status_word_reset(st)
        torch.cuda.synchronize()
        assert _flat_call(ctx, name, a_idx.ptr(), a_aidx.ptr() if alpha else None, n, nbx, pool.d_ep.data_ptr(), wc.N_EP, pool.d_sel.data_ptr(), wc.N_SEL,
                          a_out.ptr(), st.data_ptr()) == _lib.OK
        torch.cuda.synchronize()
        assert _word(st) == ((min(c[k] for k in planted) << 8) | _lib.ERR_INDEX_RANGE if planted else CLEAR), planted
        miss = _differs(a_out.data(), want.reshape(-1))
        assert miss is None, "%s planted %s: %s" % (name, planted, miss)
        for a in (a_idx, a_aidx, a_out):
            if a is not None:
                a.check()
