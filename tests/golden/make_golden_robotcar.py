"""tests/golden/make_golden_robotcar.py -- what the reference's RobotCar, NighttimeDriving and BDD100kNight readers make of the
tiny tree of robotcar_tree.py, and what RobotCar.encode_semantic_map makes of an image holding all 256 codes (authoring container
only).  The classes are imported through _ref_import.py with make_golden_data.py's throw-away stubs.  Three things stand in:
  * `h5py` (absent here) is robotcar_tree.standin_h5py(), which reads the tree's stand-in correspondence files -- as
    make_golden_rotate.py stands in for torchvision;
  * the BDD reader opens its file list inside the reference's own source tree: its module's `open` is pointed at the tree's
    made-up list for that one call, so that no line of the real list is recorded;
  * the readers' `Image.open` is wrapped to record WHICH files a sample opens (the pair form keeps no path list).
Recorded: len, the path tuples and file names per stage (relative to the data set's root), orig_dims, the encoded codes, and the
recipe, so that the tests build the same tree again.
    python tests/golden/make_golden_robotcar.py      ->  robotcar_ref.json"""
import json
import os
import shutil
import sys
import tempfile

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "..", ".."))
import _ref_import as R  # noqa: E402
import make_golden_data  # noqa: E402
from robotcar_tree import RECIPE, build_tree, standin_h5py, write_bdd_list  # noqa: E402


class _Opened:
    """PIL.Image for a reader's module: open() records the path"""

    def __init__(self):
        from PIL import Image
        self.Image, self.paths = Image, []

    def open(self, path, *a, **k):
        self.paths.append(path)
        return self.Image.open(path, *a, **k)

    def __getattr__(self, name):
        return getattr(self.Image, name)


def samples(ds, mod, root):
    """every sample's file name and the files it opened, in load_keys order"""
    rec = mod.Image = _Opened()
    out = []
    for i in range(len(ds)):
        rec.paths.clear()
        s = ds[i]
        out.append({"filename": s["filename"], "opened": {k: os.path.relpath(p, root) for k, p in zip(ds.load_keys, rec.paths)}})
        assert len(rec.paths) == len(ds.load_keys)
    return out


if __name__ == "__main__":
    R.setup()
    make_golden_data.stubs()
    sys.modules["h5py"] = standin_h5py()
    tt = sys.modules["torchvision.transforms"]
    tt.Compose = lambda ts: ts
    tt.functional.pil_to_tensor = lambda pic: torch.from_numpy(np.asarray(pic).reshape(pic.size[1], pic.size[0], -1).transpose(2, 0, 1).copy())
    data_dir = tempfile.mkdtemp(prefix="rc_")
    build_tree(data_dir, RECIPE)
    bdd_list = write_bdd_list(data_dir, RECIPE)
    mods = {"RobotCar": R.ref_module("data_modules.datasets.robotcar"),
            "NighttimeDriving": R.ref_module("data_modules.datasets.nighttimedriving"),
            "BDD100kNight": R.ref_module("data_modules.datasets.bdd100knight")}
    mods["BDD100kNight"].open = lambda path, *a, **k: open(bdd_list, *a, **k)
    cases = {"RobotCar": [("train|labelled", "train", {"load_keys": ["image", "semantic"], "dims": RECIPE["RobotCar"]["size"]}),
                          ("train|pairs", "train", {"load_keys": ["image", "image_ref"], "dims": RECIPE["RobotCar"]["size"]}),
                          ("val", "val", {"load_keys": ["image", "semantic"], "dims": RECIPE["RobotCar"]["size"]}),
                          ("test", "test", {"load_keys": ["image", "semantic"], "dims": RECIPE["RobotCar"]["size"]}),
                          ("predict", "predict", {"load_keys": ["image"], "dims": RECIPE["RobotCar"]["size"]})],
             "NighttimeDriving": [("test", "test", {"dims": RECIPE["NighttimeDriving"]["size"]})],
             "BDD100kNight": [("test", "test", {"dims": RECIPE["BDD100kNight"]["size"]})]}
    out = {"recipe": RECIPE, "readers": {}}
    for name, cs in cases.items():
        cls, root = getattr(mods[name], name), os.path.join(data_dir, name)
        out["readers"][name] = {"orig_dims": list(cls.orig_dims), "default_dims": None, "stages": {}}
        import inspect
        out["readers"][name]["default_dims"] = list(inspect.signature(cls.__init__).parameters["dims"].default)
        for key, stage, kwargs in cs:
            ds = cls(root, stage=stage, **kwargs)
            out["readers"][name]["stages"][key] = {"split": ds.split, "len": len(ds), "load_keys": list(ds.load_keys),
                                                   "samples": samples(ds, mods[name], root)}
    # the pair form lists its correspondence files in the directory's order: the CSV's lines follow it
    ds = mods["RobotCar"].RobotCar(os.path.join(data_dir, "RobotCar"), stage="train", load_keys=["image", "image_ref"])
    out["readers"]["RobotCar"]["stages"]["train|pairs"]["corr_files"] = [os.path.basename(p) for p in ds.paths["corr_files"]]
    try:
        mods["RobotCar"].RobotCar(os.path.join(data_dir, "RobotCar"), stage="val", load_keys=["image", "image_ref"])
        raise SystemExit("the reference accepted image_ref in val")
    except AssertionError:
        out["readers"]["RobotCar"]["val_refuses_image_ref"] = True
    from PIL import Image
    codes = np.arange(256, dtype=np.uint8).reshape(16, 16)
    enc = np.asarray(mods["RobotCar"].RobotCar.encode_semantic_map(Image.fromarray(codes)))
    assert enc.dtype == np.uint8 and enc.shape == (16, 16)
    out["encode_semantic_map"] = {"input": "np.arange(256, dtype=uint8).reshape(16, 16)", "output": enc.ravel().tolist()}
    shutil.rmtree(data_dir)
    dst = os.path.join(HERE, "robotcar_ref.json")
    with open(dst, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
    print(f"  wrote robotcar_ref.json  ({os.path.getsize(dst) / 1024:.1f} kB)")
