"""tests/golden/make_golden_resample.py -- writes tests/golden/resample_pillow.npz with Pillow alone: what `Image.resize` makes of
closed-form inputs (fill.hashed_uniform; the inputs are NOT stored, the tests rebuild them with the functions below).

  img_<H>x<W>_<h>x<w>   (h, w, 3) uint8 = Image.fromarray(image_in(H, W)).resize((w, h), BILINEAR)
  lbl_<H>x<W>_<h>x<w>   (h, w) uint8    = Image.fromarray(label_in(H, W)).resize((w, h), NEAREST)         for every entry of CASES
  set_img<i> / set_ref<i> / set_lbl<i>  the samplers' data set (sampler_set: SET_N decoded 96 x 160 samples with big classes in
                        blocks and a few rare-class patches) resized to SET_DIMS, as the data set readers do at load time
  eval_img2 / eval_lbl2 EVAL's decoded image resized to EVAL_DIMS, then to EVAL_RESIZE: two resizes, a uint8 image in between
  eval_img1             the decoded image resized to EVAL_RESIZE at once (a `test:` section: Resize alone, img_only)
  pillow                the version of Pillow that made the file

Run from the repository root:  python tests/golden/make_golden_resample.py"""
import os

import numpy as np
from fill import hashed_uniform

CASES = [(24, 40, 12, 20), (27, 43, 16, 25), (9, 13, 16, 25), (37, 64, 37, 21), (100, 333, 31, 7), (54, 96, 27, 48),
         (135, 240, 67, 120)]
SET_N, SET_SIZE, SET_DIMS = 4, (96, 160), (48, 80)
EVAL, EVAL_DIMS, EVAL_RESIZE = (135, 240), (67, 120), (40, 72)


def case_name(c):
    return "%dx%d_%dx%d" % tuple(c)


def image_in(H, W, key="resample/img"):
    """decoded image, (H, W, 3) uint8 channels last (what np.asarray(PIL image) gives)"""
    return (hashed_uniform((H, W, 3), f"{key}/{H}x{W}") * 256).astype(np.uint8)


def label_in(H, W, key="resample/lbl"):
    return (hashed_uniform((H, W), f"{key}/{H}x{W}") * 256).astype(np.uint8)


def sampler_set():
    """-> (images, refs, labels): SET_N decoded samples; labels: classes 0..5 in 16 x 16 blocks (one of them dominant), patches of
    the rare classes 11..13, 3 % ignore pixels"""
    H, W = SET_SIZE
    imgs, refs, lbls = [], [], []
    for i in range(SET_N):
        coarse = (hashed_uniform((H // 16, W // 16), f"resample/set/lbl{i}") * 6).astype(np.uint8)
        coarse[hashed_uniform((H // 16, W // 16), f"resample/set/big{i}") < 0.5] = i % 3
        lbl = np.repeat(np.repeat(coarse, 16, 0), 16, 1)
        u = hashed_uniform((3, 2), f"resample/set/rare{i}")
        for k in range(3):
            y, x = int(u[k, 0] * (H - 30)), int(u[k, 1] * (W - 40))
            lbl[y:y + 14 + 6 * k, x:x + 34] = 11 + k
        lbl[hashed_uniform((H, W), f"resample/set/ign{i}") < 0.03] = 255
        imgs.append(image_in(H, W, f"resample/set/img{i}"))
        refs.append(image_in(H, W, f"resample/set/ref{i}"))
        lbls.append(lbl)
    return imgs, refs, lbls


def main():
    import PIL
    from PIL import Image

    def bilinear(a, size):
        return np.asarray(Image.fromarray(a).resize((size[1], size[0]), Image.BILINEAR))

    def nearest(a, size):
        return np.asarray(Image.fromarray(a).resize((size[1], size[0]), Image.NEAREST))

    out = {"pillow": np.array(PIL.__version__)}
    for c in CASES:
        H, W, h, w = c
        out["img_" + case_name(c)] = bilinear(image_in(H, W), (h, w))
        out["lbl_" + case_name(c)] = nearest(label_in(H, W), (h, w))
    imgs, refs, lbls = sampler_set()
    for i in range(SET_N):
        out[f"set_img{i}"], out[f"set_ref{i}"] = bilinear(imgs[i], SET_DIMS), bilinear(refs[i], SET_DIMS)
        out[f"set_lbl{i}"] = nearest(lbls[i], SET_DIMS)
    img, lbl = image_in(*EVAL), label_in(*EVAL)
    out["eval_img2"] = bilinear(bilinear(img, EVAL_DIMS), EVAL_RESIZE)
    out["eval_lbl2"] = nearest(nearest(lbl, EVAL_DIMS), EVAL_RESIZE)
    out["eval_img1"] = bilinear(img, EVAL_RESIZE)
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "resample_pillow.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
