"""tests/golden/make_golden_matcher_ingest.py -- the matcher's `test:` pipeline (configs/megadepth/uawarpc_evalonly.yaml) run by
the reference's own transform classes on closed-form decoded images and points: data_modules.transforms.Resize(size=SIZE,
img_interpolation='lanczos') -> ToTensor -> ConvertImageDtype -> Normalize -> PadBottomRight(same_shape_keys=[image,
image_ref]).  The inputs are NOT stored (image_in / points_in below rebuild them).

torchvision and cv2 are not installed here; they get make_golden_data's throw-away stubs, and the three torchvision functions
the called code reaches are stubbed with their documented arithmetic: pil_to_tensor (the decoded bytes, channels first),
ConvertImageDtype.forward (uint8 -> float: x / 255) and Normalize.forward ((x - mean) / std per channel).  The resize itself is
Pillow's, the size and point arithmetic and the padding are the reference's.

  image / image_ref      (3, 128, 160) fp32: the padded, normalised images      corr_pts / corr_pts_ref   (N, 2) fp32, scaled
  size / size_ref        the (h, w) each image had before the padding           pillow                    Pillow's version

    python tests/golden/make_golden_matcher_ingest.py"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from fill import hashed_uniform  # noqa: E402

SIZE = 128                                   # Resize(size=128): the short side
IMAGE, IMAGE_REF, N = (160, 200), (192, 210), 50     # decoded sizes (h, w): -> 128 x 160 (x 0.8) and 128 x 140 (x 2 / 3)


def image_in(H, W, key):
    return (hashed_uniform((H, W, 3), f"matcher_ingest/{key}/{H}x{W}") * 256).astype(np.uint8)


def points_in(H, W, key):
    """(N, 2) fp32 (x, y): spread over the image and a margin around it, so a few lie outside"""
    u = hashed_uniform((N, 2), f"matcher_ingest/{key}/pts")
    return np.stack([u[:, 0] * (W + 12) - 6, u[:, 1] * (H + 12) - 6], 1).astype(np.float32)


def main():
    import PIL
    from PIL import Image

    import _ref_import as R
    from make_golden_data import stubs
    R.setup()
    stubs()
    tt = sys.modules["torchvision.transforms"]

    class ConvertImageDtype(torch.nn.Module):          # torchvision's, uint8 -> float: image.to(dtype) / 255
        def __init__(self, dtype=torch.float):
            super().__init__()
            self.dtype = dtype

        def forward(self, image):
            assert image.dtype == torch.uint8
            return image.to(self.dtype) / 255

    class Normalize(torch.nn.Module):                  # torchvision's: (tensor - mean[:, None, None]) / std[:, None, None]
        def __init__(self, mean, std, inplace=False):
            super().__init__()
            self.mean, self.std = mean, std

        def forward(self, tensor):
            mean = torch.as_tensor(self.mean, dtype=tensor.dtype).view(-1, 1, 1)
            std = torch.as_tensor(self.std, dtype=tensor.dtype).view(-1, 1, 1)
            return tensor.clone().sub_(mean).div_(std)

    tt.ConvertImageDtype, tt.Normalize = ConvertImageDtype, Normalize
    tt.functional.pil_to_tensor = lambda pic: torch.as_tensor(np.array(pic, copy=True)).permute(2, 0, 1).contiguous()
    tr = R.ref_module("data_modules.transforms")

    sample = {"image": Image.fromarray(image_in(*IMAGE, "image")), "image_ref": Image.fromarray(image_in(*IMAGE_REF, "image_ref")),
              "corr_pts": torch.from_numpy(points_in(*IMAGE, "image")), "corr_pts_ref": torch.from_numpy(points_in(*IMAGE_REF, "image_ref"))}
    sample = tr.Resize(size=SIZE, img_interpolation="lanczos")(sample)
    sizes = [sample[k].size[::-1] for k in ("image", "image_ref")]
    for t in (tr.ToTensor(), tr.ConvertImageDtype(), tr.Normalize(), tr.PadBottomRight(same_shape_keys=["image", "image_ref"])):
        sample = t(sample)
    out = {k: sample[k].numpy() for k in ("image", "image_ref", "corr_pts", "corr_pts_ref")}
    out.update(size=np.array(sizes[0]), size_ref=np.array(sizes[1]), pillow=np.array(PIL.__version__))
    path = os.path.join(HERE, "matcher_ingest.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes", {k: (v.shape, v.dtype) for k, v in out.items()})


if __name__ == "__main__":
    main()
