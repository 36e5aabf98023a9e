"""EXPERIMENT: bu_read_file_to of an ETC1S file to BC1 / BC3 / RG11 against the slice-by-slice route (bu_basislz_decode per slice, then
bu_etc1s_transcode per colour / alpha pair), same process, same warm-up, median of N runs.  Two files: 2048 x 2048 px with alpha (one
pair of 512 x 512 blocks) and 512 small slices (256 pairs of 16 x 16 blocks).  --trace prints the BU_TRACE laps of one call per target."""
import ctypes, os, statistics, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import basis_builder as bb
import basisu_rs_amd as bu
from basisu_rs_amd import _lib

N, WARM = 15, 3
TARGETS = (("bc1", _lib.BC1_RGB), ("bc3", _lib.BC3_RGBA), ("rg11", _lib.EAC_RG11))
lib = _lib.load()
ctx = bu.Context(0)


def median_ms(fn):
    for _ in range(WARM):
        fn()
    ts = []
    for _ in range(N):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ts), min(ts), max(ts)


def by_slices(f, t):
    """the route without the file call: every slice decoded on the calling thread, then one transcode per pair"""
    a = np.frombuffer(f, dtype=np.uint8)
    h = bu.read_header(f)
    descs = bu.read_slice_descs(f, h)
    n_cb = h.total_selectors
    ep, sel = np.zeros(n_cb, dtype=np.uint32), np.zeros((n_cb, 8), dtype=np.uint8)
    idx = [np.zeros(d.num_blocks_x * d.num_blocks_y, dtype=np.uint32) for d in descs]
    bytes_per_block = _lib.BLOCK_BYTES[t]
    out = np.empty(sum(i.size for i in idx[::2]) * bytes_per_block, dtype=np.uint8)
    bad = ctypes.c_uint64(0)

    def run():
        for k in range(len(descs)):
            assert lib.bu_basislz_decode(a.ctypes.data, a.size, k, ep.ctypes.data, sel.ctypes.data, idx[k].ctypes.data) == 0
        ofs = 0
        for k in range(0, len(descs), 2):
            n = idx[k].size
            assert lib.bu_etc1s_transcode(ctx.handle, t, idx[k].ctypes.data, idx[k + 1].ctypes.data, n, ep.ctypes.data, n_cb, sel.ctypes.data, n_cb,
                                          out.ctypes.data + ofs, out.size - ofs, ctypes.byref(bad)) == 0
            ofs += n * bytes_per_block
    return run, out


files = {"2048x2048 px, alpha (2 slices)": [(512, 512)], "512 slices of 16 x 16 blocks (256 pairs)": [(16, 16)] * 256}
for what, dims in files.items():
    f = bb.etc1s_file(np.random.default_rng(7), dims, n_codebook=4096, alpha=True)[0]
    print("%s: %d bytes" % (what, len(f)), flush=True)
    nb = bu.read_query(_lib.READ_RGBA, f)[1]
    out = np.empty(nb, dtype=np.uint8)
    print("  read_to_rgba  (pageable out)            %8.3f ms (min %.3f max %.3f)" % median_ms(lambda: bu.read_to_rgba(f, ctx, out=out)), flush=True)
    for name, t in TARGETS:
        nb = bu.read_file_query(t, f)[1]
        out = np.empty(nb, dtype=np.uint8)
        pin = ctx.host_alloc(nb)
        new = median_ms(lambda: bu.read_file_to(t, f, ctx, out=out))
        new_pin = median_ms(lambda: bu.read_file_to(t, f, ctx, out=pin))
        os.environ["BU_ETC1S_ONE_LAUNCH"] = "1"  # the front door of small files: everything decoded first, then ONE launch over all slices
        one = median_ms(lambda: bu.read_file_to(t, f, ctx, out=out))
        os.environ.pop("BU_ETC1S_ONE_LAUNCH")
        run, old_out = by_slices(f, t)
        old = median_ms(run)
        assert (old_out == out).all() and (np.asarray(pin) == out).all(), name
        ctx.host_free(pin)
        print("  %-4s read_file_to (pageable out)        %8.3f ms (min %.3f max %.3f)" % ((name,) + new))
        print("  %-4s read_file_to (page-locked out)     %8.3f ms (min %.3f max %.3f)" % ((name,) + new_pin))
        print("  %-4s read_file_to (BU_ETC1S_ONE_LAUNCH=1)  %8.3f ms (min %.3f max %.3f)" % ((name,) + one))
        print("  %-4s slice by slice                     %8.3f ms (min %.3f max %.3f)   ratio %.2f" % ((name,) + old + (old[0] / new[0],)), flush=True)
        if "--trace" in sys.argv:
            os.environ["BU_TRACE"] = "1"
            sys.stderr.write("---- %s / %s\n" % (what, name))
            bu.read_file_to(t, f, ctx, out=out)
            os.environ.pop("BU_TRACE")
ctx.close()
