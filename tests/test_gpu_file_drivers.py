"""Every driver of the whole-file call (csrc/bu_capi_file.hpp) on its smallest file: the intact file equals the oracle; one flipped payload bit that
also breaks a block or the symbol stream gives the data CRC's status while the CRC is stale, whichever way the path checks it (up front, on the
device, on a pool thread, settled on the host afterwards), and the oracle's status once both CRCs are recomputed."""
import numpy as np
import pytest

import basis_builder as bb
import basisu_rs_amd as bu
import file_shape_cases as fsc
from basisu_rs_amd import _lib, synth

pytestmark = pytest.mark.gpu
MIB = 1 << 20
READ = {"bc7": (bu.read_to_bc7, _lib.READ_BC7), "rgba": (lambda f, ctx, out=None: bu.read_to_rgba(f, ctx, out=out)[1], _lib.READ_RGBA)}


def uastc(golden, dims, seed):
    idx = [synth.gold_indices(x * y, seed=seed + i) for i, (x, y) in enumerate(dims)]
    return bb.uastc_file([golden["uastc"][ix] for ix in idx], dims)


def data_ofs(f, slice_index):
    return int.from_bytes(f[77 + 23 * slice_index + 13:77 + 23 * slice_index + 17], "little")


def near_69(f, slice_index):
    """a block of the slice whose first byte is one bit away from 69, which is no UASTC mode"""
    lo = data_ofs(f, slice_index)
    return [next(pos for pos in range(lo, lo + 16 * 4000, 16) if bin(f[pos] ^ 69).count("1") == 1)]


def breaking_flip(oracle, target, f, positions):
    """the first (position, bit) of `positions` whose flip makes the oracle refuse the resealed file"""
    for pos in positions:
        for bit in range(8):
            g = bytearray(f)
            g[pos] ^= 1 << bit
            st = oracle.read_to(target, bb.reseal(bytes(g)))[0]
            if st != 0:
                return bytes(g), st
    raise AssertionError("no flip of these bytes breaks the file")


def make_cases(golden):
    """name -> (target, file, byte positions to damage (one damaged file per list), environment, page-locked output)"""
    cases = {}
    f = uastc(golden, [(64, 48), (40, 15)], 300)
    assert len(f) < MIB  # the plan checks the CRC on the host
    cases["uastc, host crc"] = ("bc7", f, [near_69(f, 1)], {}, False)
    f = uastc(golden, [(256, 128), (256, 129)], 310)
    assert len(f) >= MIB and data_ofs(f, 1) == data_ofs(f, 0) + 16 * 256 * 128  # the device registers the run's 64 KiB pieces
    cases["uastc, device crc"] = ("bc7", f, [near_69(f, 1)], {}, False)
    f = uastc(golden, [(256, 256), (256, 256), (128, 37)], 320)
    assert data_ofs(f, 2) - data_ofs(f, 0) == 2 * MIB  # one run: pieces of 1 MiB on the context stream, its own stream, and a ragged one
    cases["uastc, pieced"] = ("bc7", f, [near_69(f, 0), near_69(f, 1)], {"BU_RUN_PIECE_MIB": "1"}, True)
    f = bb.etc1s_file(np.random.default_rng(7), [(64, 64)], n_codebook=1024)[0]
    assert len(f) < 64 << 10  # CRC up front, one launch
    cases["etc1s one launch, crc up front"] = ("rgba", f, [range(len(f) - 2000, len(f) - 1990)], {}, False)
    f = bb.etc1s_file(np.random.default_rng(7), [(180, 180)], n_codebook=4096)[0]
    assert len(f) >= 64 << 10 and 180 * 180 < 32768  # CRC deferred, one launch: settled on the host behind it
    cases["etc1s one launch, crc deferred"] = ("rgba", f, [range(len(f) - 2000, len(f) - 1990)], {}, False)
    f = bb.etc1s_file(np.random.default_rng(7), [(181, 182)], n_codebook=1024)[0]
    assert len(f) < 64 << 10 and 181 * 182 >= 32768  # CRC up front, streamed
    cases["etc1s streamed, crc up front"] = ("rgba", f, [range(len(f) - 2000, len(f) - 1990)], {}, False)
    f = fsc.etc1s_file("array_240", True)
    assert len(f) >= 64 << 10 and fsc.total_blocks("array_240") >= 32768  # CRC deferred, streamed: on a pool thread beside 288 small slices
    cases["etc1s streamed, crc deferred"] = ("rgba", f, [range(len(f) - 2000, len(f) - 1990)], {}, False)
    return cases


@pytest.fixture(scope="module")
def cases(golden):
    return make_cases(golden)


def read(ctx, target, f, pinned):
    """pinned: bytes of a page-locked output to read into, 0 = an ordinary one"""
    fn = READ[target][0]
    out = ctx.host_alloc(pinned) if pinned else None
    try:
        try:
            imgs = fn(f, ctx, out=out)
        except bu.BasisuError as e:
            return e.status, None
        return 0, [(g.w, g.h, g.stride, np.asarray(g.data).tobytes()) for g in imgs]
    finally:
        if pinned:
            ctx.host_free(out)


@pytest.mark.parametrize("name", ["uastc, host crc", "uastc, device crc", "uastc, pieced", "etc1s one launch, crc up front", "etc1s one launch, crc deferred",
                                  "etc1s streamed, crc up front", "etc1s streamed, crc deferred"])
def test_driver_path(ctx, oracle, cases, monkeypatch, name):
    target, f, damage, env, pinned = cases[name]
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    st, _, want = oracle.read_to(target, f)
    assert st == 0
    pinned = bu.read_query(READ[target][1], f)[1] if pinned else 0
    assert read(ctx, target, f, pinned) == (0, [(w, h, s, d.tobytes()) for (w, h, s, d) in want])
    for positions in damage:
        g, broken = breaking_flip(oracle, target, f, positions)
        assert read(ctx, target, g, pinned) == (_lib.ERR_DATA_CRC, None)
        assert read(ctx, target, bb.reseal(g), pinned) == (broken, None)
