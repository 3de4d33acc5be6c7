"""tests/golden/make_golden_matching.py -- what the reference's MegaDepth and RobotCarMatching readers make of the tiny tree of
matching_tree.py (authoring container only).  The two classes are imported through _ref_import.py with make_golden_data.py's
throw-away stubs.  The reference opens its scene lists inside its own source tree: the class's `cfg` entries are set to the
absolute paths of the tree's made-up lists (os.path.join returns an absolute second argument unchanged).
Recorded (no pixels: pixel parity is Pillow's, and the Lanczos tests carry it):
  recipe                       the tree
  megadepth/<case>             len, the items as [image_path1, image_path2, number of matches] in the list's order -- for the
                               in-memory and the on-demand form -- and per sampled index and exchange decision the two paths
                               below the root and the points without dims and with DIMS (both forms gave the same)
  megadepth/exchange           under random.seed(SEED), which of val's samples were exchanged, and random.random() afterwards
  megadepth/test, robotcar     len and per row the paths and the points without dims and with DIMS
    python tests/golden/make_golden_matching.py      ->  matching_ref.json"""
import json
import os
import random
import shutil
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "..", ".."))
import _ref_import as R  # noqa: E402
import make_golden_data  # noqa: E402
from matching_tree import LIST_FILES, RECIPE, build_tree  # noqa: E402

DIMS = (160, 160)
SEED = 77
CASES = {"train": ("train", False), "val": ("val", False), "debug": ("train", True)}
SAMPLED = 3


def pts(t):
    return [[float(v) for v in row] for row in np.asarray(t, dtype=np.float32)]


def bundle(ds, i):
    it = ds.items[i]
    return it if isinstance(it, dict) else ds._read_pair_info(*it[:3])


if __name__ == "__main__":
    R.setup()
    make_golden_data.stubs()
    MegaDepth = R.ref_module("data_modules.datasets.megadepth").MegaDepth
    RobotCarMatching = R.ref_module("data_modules.datasets.robotcarmatching").RobotCarMatching
    data_dir = tempfile.mkdtemp(prefix="match_")
    build_tree(data_dir, RECIPE)
    root = os.path.join(data_dir, "MegaDepth")
    MegaDepth.cfg = dict(MegaDepth.cfg, train_split=os.path.join(root, "lists", LIST_FILES["train"]),
                         train_debug_split=os.path.join(root, "lists", LIST_FILES["train_debug"]),
                         val_split=os.path.join(root, "lists", LIST_FILES["validation"]),
                         test_split=os.path.join(root, "lists", LIST_FILES["test"]))
    keys = ["image_ref", "image"]
    out = {"recipe": RECIPE, "dims": list(DIMS), "seed": SEED, "megadepth": {}}
    for case, (stage, debug) in CASES.items():
        rec = {}
        for mode, in_memory in (("in_memory", True), ("on_demand", False)):
            ds = MegaDepth(root, stage=stage, load_keys=keys, dims=None, store_scene_info_in_memory=in_memory, debug=debug)
            scaled = MegaDepth(root, stage=stage, load_keys=keys, dims=DIMS, store_scene_info_in_memory=in_memory, debug=debug)
            items = [[b["image_path1"], b["image_path2"], len(b["2d_matches_1"])] for b in (bundle(ds, i) for i in range(len(ds.items)))]
            samples = {}
            for i in range(0, len(ds.items), max(1, len(ds.items) // SAMPLED)):
                for exchange in (False, True):
                    b = bundle(ds, i)
                    _, _, p1, p2 = ds.recover_pair(b, exchange_images=exchange)
                    _, _, s1, s2 = scaled.recover_pair(bundle(scaled, i), exchange_images=exchange)
                    first, second = (b["image_path2"], b["image_path1"]) if exchange else (b["image_path1"], b["image_path2"])
                    samples[f"{i}|{int(exchange)}"] = {"image_ref": first, "image": second, "corr_pts_ref": pts(p1), "corr_pts": pts(p2),
                                                       "corr_pts_ref_dims": pts(s1), "corr_pts_dims": pts(s2)}
            rec[mode] = {"len": len(ds), "n_items": len(ds.items), "items": items, "samples": samples}
        assert rec["in_memory"] == rec["on_demand"], case
        del rec["on_demand"]["samples"]                      # (equal, as just checked: stored once)
        out["megadepth"][case] = rec
    # the exchange coin: the val split throws it too, and a probability of 0 consumes it as well
    ds = MegaDepth(root, stage="val", load_keys=keys, dims=None, store_scene_info_in_memory=True, exchange_images_with_proba=0.5)
    calls = []
    inner = ds.recover_pair
    ds.recover_pair = lambda meta, exchange_images=False: (calls.append(bool(exchange_images)), inner(meta, exchange_images))[1]
    random.seed(SEED)
    for i in range(len(ds)):
        ds[i]
    out["megadepth"]["exchange"] = {"proba": 0.5, "exchanged": calls, "next": random.random()}
    ds = MegaDepth(root, stage="val", load_keys=keys, dims=None, store_scene_info_in_memory=True)
    random.seed(SEED)
    for i in range(3):
        ds[i]
    out["megadepth"]["exchange"]["next_after_3_at_proba_0"] = random.random()

    def rows(cls, root):
        plain, scaled = cls(root, stage="test", load_keys=keys, dims=None), cls(root, stage="test", load_keys=keys, dims=DIMS)
        rec = {"len": len(plain), "rows": []}
        for i in range(len(plain)):
            a, b = plain[i], scaled[i]
            scene = "." if plain.df["scene"][i] == "/" else plain.df["scene"][i]
            rec["rows"].append({"image_ref": os.path.join(scene, plain.df["source_image"][i]),
                                "image": os.path.join(scene, plain.df["target_image"][i]),
                                "sizes": {k: [a[k].size[1], a[k].size[0]] for k in keys},
                                "corr_pts_ref": pts(a["corr_pts_ref"]), "corr_pts": pts(a["corr_pts"]),
                                "corr_pts_ref_dims": pts(b["corr_pts_ref"]), "corr_pts_dims": pts(b["corr_pts"])})
        return rec

    out["megadepth"]["test"] = rows(MegaDepth, root)
    rc = os.path.join(data_dir, "RobotCarMatching")
    out["robotcar"] = rows(RobotCarMatching, rc)
    try:
        RobotCarMatching(rc, stage="train")
        raise SystemExit("RobotCarMatching took stage='train'")
    except AssertionError:
        out["robotcar"]["train_stage"] = "AssertionError"
    shutil.rmtree(data_dir)
    dst = os.path.join(HERE, "matching_ref.json")
    with open(dst, "w") as f:
        json.dump(out, f, indent=None, sort_keys=True, separators=(",", ":"))
    print(f"  wrote matching_ref.json  ({os.path.getsize(dst) / 1024:.1f} kB)")
