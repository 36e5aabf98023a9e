"""Guard bands around everything a kernel is handed: what the suite's comparisons do not see is a store outside [0, n) -- torch's caching
allocator rounds and pools allocations, so an overrun faults nothing -- and a lane that works on a block or an index outside its input.

Arena          one uint8 buffer (a torch tensor on the device, or a numpy array: page-locked from Context.host_alloc, or pageable) holding one or
               more data regions, a guard band in front of the first, between every two and behind the last.  A band is at least GUARD_MIN bytes
               and at least what the caller asks for (one tile of the buffer's data).  Each region starts at a chosen offset from 256-byte
               alignment, so a case can sit on the smallest alignment include/basisu_hip.h allows.
the fill       a fixed pseudo-random function of the byte's offset in the arena (never a constant: a failing block is written as zeros and a
               constant may coincide with result bytes), with no aligned run of eight zero bytes; regenerated for the check.  Input arenas use
               the poisoned fills instead: "uastc" -- every 16-byte block of the band has mode byte 69, an invalid block, so a lane that takes a
               block outside its slice reports it in the status word even where its store is masked; "ones" -- 0xFF bytes, an index no codebook
               holds; "endpoint" / "selector" -- codebook entries no good block decodes to.
check()        every band still holds its fill; the failure names the arena, the byte offset and the region it lies next to."""
import numpy as np

GUARD_MIN = 64 * 1024
BASE_ALIGN = 256
FILLS = ("random", "uastc", "ones", "endpoint", "selector")


def fill_bytes(xp, start, stop, fill="random", phase=0, device=None):
    """the fill of arena bytes [start, stop) as uint8; xp = torch or numpy.  `phase`: offset of a 16-byte boundary of the data (the poisoned
    fills are laid out in the data's blocks / entries)"""
    kw = {"device": device} if device is not None else {}
    o = xp.arange(start, stop, dtype=xp.int64, **kw)
    if fill == "ones" or fill == "endpoint":  # 0xFFFFFFFF: an index beyond every codebook / an endpoint with five-bit fields of 255
        return (o * 0 + 0xFF).to(xp.uint8) if hasattr(o, "to") else (o * 0 + 0xFF).astype(np.uint8)
    rel = (o - phase) % 16
    if fill == "selector":  # rows of all threes whose ETC1 bytes belong to other rows: no selector entry is built like that
        v = o * 0 + 0xFF
        v = xp.where(rel % 8 >= 4, o * 0 + 0x5A, v)
    else:
        h = o * 40503 + 12345  # (below 2^63 for any offset here)
        v = ((h >> 9) ^ (h >> 3) ^ (o >> 11) ^ o) & 0xFF
        v = xp.where(o % 8 == 0, v | 1, v)  # no aligned run of eight zero bytes
        if fill == "uastc":
            v = xp.where(rel == 0, o * 0 + 69, v)  # mode byte 69: "invalid mode index"
    return v.to(xp.uint8) if hasattr(v, "to") else v.astype(np.uint8)


class Region:
    def __init__(self, start, nbytes):
        self.start, self.nbytes = start, nbytes

    @property
    def stop(self):
        return self.start + self.nbytes


def _layout(base_addr, sizes, guard, offsets):
    """starts of the data regions in an arena at address base_addr: a band of >= guard bytes in front of each, the region at
    offsets[i] bytes past a 256-byte boundary; returns (regions, total bytes)"""
    guard = max(int(guard), GUARD_MIN)
    regions, pos = [], 0
    for nbytes, ofs in zip(sizes, offsets):
        pos += guard
        pos += (ofs - (base_addr + pos)) % BASE_ALIGN
        regions.append(Region(pos, int(nbytes)))
        pos += int(nbytes)
    return regions, pos + guard


class Arena:
    """`sizes`: bytes of each data region; `guard`: bytes a band must at least have (>= GUARD_MIN is enforced); `offsets`: per region (or one for
    all), the distance of its start from 256-byte alignment; `fill`: one of FILLS; `where`: "cuda", "pinned" (needs ctx), or "pageable"."""

    def __init__(self, name, sizes, guard, offsets=0, fill="random", where="cuda", ctx=None):
        assert fill in FILLS
        sizes = [int(s) for s in (sizes if isinstance(sizes, (list, tuple)) else [sizes])]
        offsets = list(offsets) if isinstance(offsets, (list, tuple)) else [offsets] * len(sizes)
        self.name, self.fill, self.where, self.ctx = name, fill, where, ctx
        slack = BASE_ALIGN * len(sizes)
        total = _layout(0, sizes, guard, [0] * len(sizes))[1] + slack
        if where == "cuda":
            import torch

            self.xp, self.device = torch, "cuda"
            self.buf = torch.empty(total, dtype=torch.uint8, device="cuda")
            self.addr = self.buf.data_ptr()
        else:
            self.xp, self.device = np, None
            self.buf = ctx.host_alloc(total) if where == "pinned" else np.empty(total, dtype=np.uint8)
            self.addr = self.buf.ctypes.data
        self.regions, used = _layout(self.addr, sizes, guard, offsets)
        assert used <= total
        self.phase = self.regions[0].start % 16
        assert all(r.start % 16 == self.phase for r in self.regions) or fill in ("random", "ones", "endpoint")
        self.bands = []  # (start, stop) of every guard band
        pos = 0
        for r in self.regions:
            self.bands.append((pos, r.start))
            pos = r.stop
        self.bands.append((pos, total))
        assert all(b - a >= max(int(guard), GUARD_MIN) for a, b in self.bands)
        for a, b in self.bands:
            self.buf[a:b] = self._fill(a, b)

    def _fill(self, a, b):
        return fill_bytes(self.xp, a, b, self.fill, self.phase, self.device)

    def data(self, i=0):
        """region i as a uint8 view of the arena"""
        r = self.regions[i]
        return self.buf[r.start:r.stop]

    def ptr(self, i=0):
        return self.addr + self.regions[i].start

    def violations(self):
        """[(band index, arena byte offset of the first changed byte, number of changed bytes)] over all bands"""
        out = []
        for k, (a, b) in enumerate(self.bands):
            want = self._fill(a, b)
            got = self.buf[a:b]
            if self.xp is np:
                if np.array_equal(got, want):
                    continue
                bad = np.nonzero(got != want)[0]
                out.append((k, a + int(bad[0]), int(bad.size)))
            else:
                if self.xp.equal(got, want):
                    continue
                bad = self.xp.nonzero(got != want)[:, 0]
                out.append((k, a + int(bad[0].item()), int(bad.numel())))
        return out

    def check(self):
        bad = self.violations()
        if not bad:
            return
        lines = []
        for k, ofs, count in bad:
            if k == 0:
                rel = "%d bytes in front of region 0" % (self.regions[0].start - ofs)
            else:
                r = self.regions[k - 1]
                rel = "%d bytes past the end of region %d (%d bytes)" % (ofs - r.stop, k - 1, r.nbytes)
                if k < len(self.regions):
                    rel += ", %d bytes in front of region %d" % (self.regions[k].start - ofs, k)
            lines.append("guard band %d changed at arena offset %d (%s), %d bytes in all" % (k, ofs, rel, count))
        raise AssertionError("%s: %s" % (self.name, "; ".join(lines)))

    def free(self):
        if self.where == "pinned":
            self.ctx.host_free(self.buf)
        self.buf = None


def guard_bytes(block_bytes, tile_blocks=1024):
    """the band of a buffer of block_bytes per block whose kernels work in tiles of tile_blocks: one tile, at least GUARD_MIN"""
    return max(GUARD_MIN, tile_blocks * block_bytes)


POISON_BLOCKS = 4096  # invalid blocks / 0xFFFFFFFF words in front of and behind an input, at least
