"""tests/golden/make_golden_datamodule.py -- what the reference's readers and its CombinedDataModule make of a tiny tree and of
the reference's own ACDC / Dark Zurich configurations (authoring container only).  Cityscapes, ACDC, DarkZurich and
CombinedDataModule are imported through _ref_import.py with make_golden_data.py's throw-away stubs plus a numpy `pil_to_tensor`;
no file is decoded by them here: recorded are the path lists, orig_dims, the rare-class tables and the parsed sections.
The tree is datamodule_tree.build_tree(RECIPE); the recipe is stored with the results, so that the tests build the same tree
again.  The two rare-class JSON files the reference's Cityscapes reads are written by refign_amd.datasets.write_class_stats
(the reference's own writer starts from the polygon files and needs cityscapesscripts).
    python tests/golden/make_golden_datamodule.py      ->  datamodule_ref.json"""
import copy
import glob
import json
import os
import shutil
import sys
import tempfile

import numpy as np
import torch
import yaml

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "..", ".."))
import _ref_import as R  # noqa: E402
import make_golden_data  # noqa: E402
from datamodule_tree import RECIPE, build_tree  # noqa: E402

READER_CASES = {
    "Cityscapes": [("train", {"rcs_enabled": True, "rcs_min_pixels": 40}), ("val", {}), ("test", {}), ("predict", {})],
    "ACDC": [("train", {"load_keys": ["image", "image_ref"]}), ("val", {}), ("test", {}), ("predict", {}),
             ("predict", {"predict_on": "val"}), ("val", {"condition": "fog"})],
    "DarkZurich": [("train", {}), ("val", {"load_keys": ["image", "semantic"]}), ("test", {}), ("predict", {}),
                   ("predict", {"predict_on": "val"})],
}


def case_key(stage, kwargs):
    return stage + "".join(f"|{k}={v}" for k, v in sorted(kwargs.items()) if k in ("predict_on", "condition"))


def scratch_dir():
    """the reference pairs files by str.replace on whole paths: the root must not hold a split's or a condition's name"""
    while True:
        d = tempfile.mkdtemp(prefix="dm_")
        if not any(w in d for w in ("train", "val", "test", "night", "day", "fog")):
            return d
        shutil.rmtree(d)


if __name__ == "__main__":
    R.setup()
    make_golden_data.stubs()
    tt = sys.modules["torchvision.transforms"]
    tt.Compose = lambda ts: ts
    tt.functional.pil_to_tensor = lambda pic: torch.from_numpy(np.asarray(pic).reshape(pic.size[1], pic.size[0], -1).transpose(2, 0, 1).copy())
    cli = sys.modules["pytorch_lightning.utilities.cli"]
    cli.DATAMODULE_REGISTRY, cli.instantiate_class = (lambda cls: cls), (lambda args, init: init)
    data_dir = scratch_dir()
    os.environ["DATA_DIR"] = data_dir
    build_tree(data_dir, RECIPE)
    from refign_amd.datasets import write_class_stats
    write_class_stats(os.path.join(data_dir, "Cityscapes"))
    ref = {"Cityscapes": R.ref_module("data_modules.datasets.cityscapes").Cityscapes,
           "ACDC": R.ref_module("data_modules.datasets.acdc").ACDC,
           "DarkZurich": R.ref_module("data_modules.datasets.darkzurich").DarkZurich}
    out = {"recipe": RECIPE, "readers": {}, "configs": {}}
    if any("zurich_dn_pair_train" in p for p in RECIPE["DarkZurich"]["pairs"][0]):
        raise SystemExit("the pair list of the tree must be made up")
    for name, cases in READER_CASES.items():
        root = os.path.join(data_dir, name)
        out["readers"][name] = {"orig_dims": list(ref[name].orig_dims), "stages": {}}
        for stage, kwargs in cases:
            if name == "DarkZurich" and stage == "train":
                # the reference opens the list inside its own source tree: the made-up list cannot be handed to it.  Its pairing
                # rule (root/rgb_anon/<name>_rgb_anon.png for both columns) is applied to the tree's list by the test itself.
                continue
            ds = ref[name](root, stage=stage, **copy.deepcopy(kwargs))
            rel = lambda p: os.path.relpath(p, root)  # noqa: E731
            n = len(ds)
            rec = {"split": ds.split, "len": n,
                   "triples": [[rel(ds.paths[k][i]) if k in ds.paths and ds.paths[k] else None
                                for k in ("image", "image_ref", "semantic")] for i in range(n)]}
            if kwargs.get("rcs_enabled"):
                rec["rcs_classes"] = [int(c) for c in ds.rcs_classes]
                assert ds.rcs_classprob.dtype == np.float32
                rec["rcs_classprob"] = [float(p) for p in ds.rcs_classprob]
                rec["files_with_class"] = {str(c): sorted(rel(ds.paths["semantic"][i]) for i in idx)
                                           for c, idx in ds.indices_with_class.items()}
            out["readers"][name]["stages"][case_key(stage, kwargs)] = rec
    cdm = R.ref_module("data_modules.combined_data_module").CombinedDataModule
    cfg_root = os.path.join(R.REF, "configs")
    for path in sorted(glob.glob(os.path.join(cfg_root, "cityscapes_acdc", "**", "*.yaml"), recursive=True)
                       + glob.glob(os.path.join(cfg_root, "cityscapes_darkzurich", "**", "*.yaml"), recursive=True)):
        with open(path) as f:
            args = copy.deepcopy(yaml.safe_load(f)["data"]["init_args"])
        dm = cdm(**args)
        out["configs"][os.path.relpath(path, cfg_root)] = {
            "train_on": dm.train_on, "val_on": dm.val_on, "test_on": dm.test_on, "predict_on": dm.predict_on,
            "idx_to_name": {s: {str(i): n for i, n in d.items()} for s, d in dm.idx_to_name.items()},
            "batch_size": dm.batch_size, "val_batch_size": dm.val_batch_size, "test_batch_size": dm.test_batch_size}
    shutil.rmtree(data_dir)
    dst = os.path.join(HERE, "datamodule_ref.json")
    with open(dst, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
    print(f"  wrote datamodule_ref.json  ({os.path.getsize(dst) / 1024:.1f} kB)")
