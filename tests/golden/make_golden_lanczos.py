"""tests/golden/make_golden_lanczos.py -- writes tests/golden/lanczos_pillow.npz with Pillow alone: what `Image.resize(...,
LANCZOS)` makes of closed-form inputs (fill.hashed_uniform; the inputs are NOT stored, the tests rebuild them with the functions
below).

  img_<H>x<W>_<h>x<w>   (h, w, 3) uint8 = Image.fromarray(image_in(H, W)).resize((w, h), LANCZOS)      for every entry of CASES
  bin_<H>x<W>_<h>x<w>   the same of binary_in(H, W), an image of 0 and 255 only: the negative lobes overshoot at every edge, so
                        the clip to a byte after each pass is exercised                                 for BINARY
  chain                 image_in(*CHAIN[0]) resized to CHAIN[1], then to CHAIN[2]: two resizes, a uint8 image in between
  pillow                the version of Pillow that made the file

Run from the repository root:  python tests/golden/make_golden_lanczos.py"""
import os

import numpy as np
from fill import hashed_uniform

CASES = [(24, 40, 12, 20),          # plain down-scale
         (27, 43, 16, 25),          # ragged
         (9, 13, 16, 25),           # up-scaling: 7 taps
         (37, 64, 37, 21),          # one axis only (Pillow skips the other pass)
         (135, 240, 67, 120),       # two tiles in both axes
         (260, 70, 13, 66)]         # vertical scale 20, 121 taps: the tile shrinks to fit LDS; the width spans two column tiles
BINARY = (64, 96, 48, 72)
CHAIN = [(135, 240), (67, 120), (40, 72)]


def case_name(c):
    return "%dx%d_%dx%d" % tuple(c)


def image_in(H, W, key="lanczos/img"):
    """decoded image, (H, W, 3) uint8 channels last (what np.asarray(PIL image) gives)"""
    return (hashed_uniform((H, W, 3), f"{key}/{H}x{W}") * 256).astype(np.uint8)


def binary_in(H, W, key="lanczos/bin"):
    """0 / 255 in 4 x 4 blocks per channel: sharp edges everywhere"""
    coarse = hashed_uniform(((H + 3) // 4, (W + 3) // 4, 3), f"{key}/{H}x{W}") < 0.5
    return (np.repeat(np.repeat(coarse, 4, 0), 4, 1)[:H, :W] * 255).astype(np.uint8)


def main():
    import PIL
    from PIL import Image

    def lanczos(a, size):
        return np.asarray(Image.fromarray(a).resize((size[1], size[0]), Image.LANCZOS))

    out = {"pillow": np.array(PIL.__version__)}
    for c in CASES:
        out["img_" + case_name(c)] = lanczos(image_in(c[0], c[1]), c[2:])
    out["bin_" + case_name(BINARY)] = lanczos(binary_in(*BINARY[:2]), BINARY[2:])
    out["chain"] = lanczos(lanczos(image_in(*CHAIN[0]), CHAIN[1]), CHAIN[2])
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "lanczos_pillow.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
