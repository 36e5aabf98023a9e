"""ETC1S files a fitted Huffman code over a random symbol stream never is (tests/basis_builder.py: `tables=`, `script=`): the table shapes and stream
shapes other encoders may write and src/basis_lz/huffman.rs:43-184 / mod.rs:188-458 accept.  Shared by tests/test_lz_shape_cases.py (CPU: both host
decoders against the encoder's own record of what every block means, and which of the product's slice loops decoded the file) and
tests/test_gpu_lz_shapes.py (the kernels get the same bytes whichever host path decoded the file).

CPU cases are files of 2-4 slices of at most 40 x 30 blocks, n_codebook = 256.  Table shapes, each on each of the four slice tables in turn (the others
fitted; tables "delta" and "rle" in a file with alpha pairs):
  single            one used symbol of length 1 (the stream scripted so that the table sees one symbol)
  fixed16           every used symbol 16 bits: a 65 536-entry lookup, incomplete
  incomplete        the fitted lengths plus one: Kraft sum 1/2
  long_tail_zero    the record's last token a zero run that passes total_used by 11 sizes
  long_tail_repeat  the record's last token a repeat that passes total_used by 5 sizes (five phantom symbols with codes of their own)
  cl_full           the code-length alphabet written with n = 21, every one of its 21 symbols with a code.  (Every one of them also OCCURRING in one record is
                    not possible in a prefix code: sizes 1 .. 16 once each have the Kraft sum 1 - 2^-16, which leaves room for one more 16-bit symbol, and
                    the shortest repeat, symbol 19, brings three.)
  cl_min            every used symbol 8 bits: code sizes 0 and 8 and the four run symbols only, n = 6 -- the smallest n any table with a coded symbol can
                    have, 8 being the first code size in the alphabet's order (huffman.rs:52-56)
  collide           Kraft sum above 1.  NOT a file that decodes: huffman.rs:143-149 makes next_code[16] = 65 536 x the Kraft sum of the sizes below 16, every
                    16-bit symbol adds one, and huffman.rs:176-178 refuses the table when any next_code exceeds 65 536 -- exactly when the Kraft sum
                    exceeds 1.  So the symbol-order fill "later symbols overwrite" (huffman.rs:155-174; bu_huffman.hpp's over-subscribed branch) is only ever
                    the prelude of an error.  The case is written through that fill all the same (basis_builder.LookupCoder), and what is held is that the
                    oracle and the product refuse it with the same status.
  empty_rle         the history_rle table with total_used = 0 (and n = 0), and with total_used = 1 and the size 0, for history_size 0 and 32, in a stream
                    that never emits the run symbol.  Legal: read_huffman_table builds a one-entry lookup without a code (huffman.rs:151) and only
                    decode_symbol fails on it (huffman.rs:189-197), which mod.rs:380-383 reaches through the run symbol alone.  The product's fast loop and
                    its two-thread form refuse such tables (they index the lookup unconditionally) and the exact loop decodes the file.
  empty_pred_video  LEFT OUT: mod.rs:264 decodes a symbol from the endpoint-predictor table for the first 2 x 2 group of every slice, whatever the
                    texture type (texture video only changes what predictor 2 means, mod.rs:327-331), so a slice with a block always decodes from that table
                    and an empty one is never legal.
Stream scripts (basis_builder.SCRIPTS), each on grids 1 x N, N x 1, odd x odd and 40 x 30 and on a file with alpha pairs: pred_run, sel_run, one_run (both),
run_exact_end, run_leftover, hist_last with history_size 1 and 32, delta_wrap.

The files for the GPU (gpu_file) are the same recipes at two sizes: a few thousand blocks in three images (one launch), and one image of 192 x 176 blocks
with two small ones, 33 792 + 24 blocks: just past STREAM_MIN_BLOCKS, the streamed front door."""
import collections
import functools

import numpy as np

import basis_builder as bb

N_CODEBOOK = 256
TABLE_DIMS = {False: [(17, 11), (1, 30), (40, 1)], True: [(17, 11), (9, 5)]}           # by alpha: 3 slices, 2 x 2 slices
SCRIPT_DIMS = {False: [(1, 30), (40, 1), (13, 9), (40, 30)], True: [(1, 30), (13, 9)]}  # 4 slices, 2 x 2 slices
TABLE_SHAPES = ("single", "fixed16", "incomplete", "long_tail_zero", "long_tail_repeat", "cl_full", "cl_min", "collide")
SCRIPT_NAMES = ("pred_run", "sel_run", "one_run", "run_exact_end", "run_leftover", "hist_last", "delta_wrap")

# refuse: the fast loop and split_ok() must refuse, the exact loop decodes; rejected: no decoder may accept the file
Case = collections.namedtuple("Case", "name shape table script dims alpha hs tables seed refuse rejected")


def _cases():
    out = []
    for ti, table in enumerate(bb.TABLE_NAMES):
        alpha = bool(ti & 1)
        for shape in TABLE_SHAPES:
            spec = {"cl_full": dict(lengths="fitted", cl="full"), "cl_min": "fixed8"}.get(shape, shape)
            out.append(Case("%s-%s" % (shape, table), shape, table, "single_" + table if shape == "single" else None, TABLE_DIMS[alpha], alpha, 32,
                            {table: spec}, 100 + 10 * ti + len(out) % 10, False, shape == "collide"))
    for k, (rule, hs) in enumerate((("empty", 0), ("empty", 32), ("empty_one", 0), ("empty_one", 32))):
        alpha = bool(k & 1)
        out.append(Case("empty_rle-%s-hs%d" % (rule, hs), "empty_rle", "rle", "no_rle", TABLE_DIMS[alpha], alpha, hs, {"rle": rule}, 200 + k, True, False))
    for k, script in enumerate(SCRIPT_NAMES):
        for alpha in (False, True):
            for hs in ((1, 32) if script == "hist_last" else (32,)):
                out.append(Case("%s-%s-hs%d" % (script, "alpha" if alpha else "opaque", hs), "script", None, script, SCRIPT_DIMS[alpha], alpha, hs, None,
                                300 + 2 * k + alpha, False, False))
    return collections.OrderedDict((c.name, c) for c in out)


CASES = _cases()
NAMES = tuple(CASES)


@functools.lru_cache(maxsize=None)
def build(name):
    """-> (file, endpoints, selector rows, the SliceSymbols of every slice: .indices is the record)"""
    c = CASES[name]
    return bb.etc1s_file(np.random.default_rng(c.seed), c.dims, n_codebook=N_CODEBOOK, history_size=c.hs, alpha=c.alpha, tables=c.tables, script=c.script,
                         want_indices=True)


# ---- the files for the device ---------------------------------------------------------------------------------------------------------
STREAM_MIN_BLOCKS = 32768   # as in tests/file_shape_cases.py, which tests/test_file_shape_cases.py pins to the source
CRC_DEFER_BYTES = 64 << 10
GPU_DIMS = {"small": [(64, 40), (33, 17), (1, 1)], "large": [(192, 176), (5, 4), (2, 2)]}  # 3122 and 33 816 blocks
# recipe -> (keywords of etc1s_file, may_split: whether the streamed door may decode the large first slice on two threads)
GPU_RECIPES = {
    "empty_rle_fixed16": (dict(history_size=32, alpha=False, tables={"rle": "empty", "sel": "fixed16"}, script="no_rle"), False),
    "one_run_alpha": (dict(history_size=32, alpha=True, script="one_run"), True),
}
# (recipe, size) -> (streamed, payload CRC deferred): the door by the total block count, the CRC mode by the file's size
GPU_DOORS = {("empty_rle_fixed16", "small"): (False, False), ("empty_rle_fixed16", "large"): (True, True),
             ("one_run_alpha", "small"): (False, False), ("one_run_alpha", "large"): (True, False)}
GPU_FILES = tuple(GPU_DOORS)


@functools.lru_cache(maxsize=None)
def gpu_file(recipe, size):
    """-> (file, endpoints, selector rows, SliceSymbols per slice)"""
    kw = GPU_RECIPES[recipe][0]
    return bb.etc1s_file(np.random.default_rng(400 + len(recipe) + len(size)), GPU_DIMS[size], n_codebook=N_CODEBOOK, want_indices=True, **kw)


def check_gpu_door(recipe, size):
    """the file is what its row says: three images, the front door by the total block count, the CRC mode by the file's size"""
    streamed, deferred = GPU_DOORS[recipe, size]
    dims = GPU_DIMS[size]
    total = sum(x * y for x, y in dims)
    assert len(dims) == 3 and total == {"small": 3122, "large": 33816}[size]
    assert (total >= STREAM_MIN_BLOCKS) == streamed, (recipe, size)
    if size == "large":  # the first slice alone is long enough for the two-thread form, where the tables allow it
        assert dims[0][0] * dims[0][1] == 33792 >= STREAM_MIN_BLOCKS
    f = gpu_file(recipe, size)[0]
    assert (len(f) >= CRC_DEFER_BYTES) == deferred, (recipe, size, len(f))
