"""Writes tests/golden/bc7_third_party.bin: 1024 valid BC7 blocks, 128 per mode, each with the 64 bytes a THIRD PARTY decodes it to -- Pillow's DDS
reader (tests/pillow_blocks.py), which shares no code and no author with this project's decoders.  Generated with Pillow 12.2.0.

    python tests/golden/make_bc7_third_party.py          (run by hand, needs Pillow; the suite only reads the file)

The file: 1024 records of 80 bytes = the 16 block bytes, then the 16 texels as R, G, B, A bytes, texel i = 4y + x.  Record 128 m + k is of mode m.
Within a mode every bit but the fields below is random (seed 7); every bit pattern with a mode bit is a valid BC7 block.
  modes 0 (16 partitions), 1, 2, 3, 7 (64 partitions): partition index = k mod 16 / k mod 64, so each appears 8 / 2 times
  mode 4: (rotation, index selector) = (k mod 4, (k >> 2) mod 2), each pair 16 times          mode 5: rotation = k mod 4, each 32 times"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import pillow_blocks  # noqa: E402

PER_MODE, SEED = 128, 7
FIELD_BITS = {0: 4, 1: 6, 2: 6, 3: 6, 4: 3, 5: 2, 6: 0, 7: 6}  # the bits after the mode bit that are stratified: partition / rotation (+ selector)


def blocks():
    rng = np.random.default_rng(SEED)
    out = []
    for mode in range(8):
        raw = rng.integers(0, 256, size=(PER_MODE, 16), dtype=np.uint8)
        for k in range(PER_MODE):
            v = int.from_bytes(raw[k].tobytes(), "little")
            nb = FIELD_BITS[mode]
            v &= ~((1 << (mode + 1 + nb)) - 1)
            v |= 1 << mode | (k % (1 << nb)) << (mode + 1)
            out.append(np.frombuffer(v.to_bytes(16, "little"), dtype=np.uint8))
    return np.stack(out)


if __name__ == "__main__":
    import PIL

    b = blocks()
    px = pillow_blocks.decode("bc7", b, 32).reshape(-1, 64)
    path = os.path.join(HERE, "bc7_third_party.bin")
    np.concatenate([b, px], axis=1).tofile(path)
    print("Pillow %s: %d blocks -> %s (%d bytes)" % (PIL.__version__, b.shape[0], path, os.path.getsize(path)))
