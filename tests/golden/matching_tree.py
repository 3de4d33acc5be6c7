"""tests/golden/matching_tree.py -- a tiny MegaDepth / RobotCarMatching tree, built from a recipe (made-up scene names, sizes,
seeds, overlap matrices), and the `data:` sections the matching data module tests run over it.  make_golden_matching.py builds
it to run the reference's readers over it and stores the recipe next to what they found; the tests build the same tree again
from that recipe.

What the recipe pins: JPEG files of different sizes (40 x 56 ... 97 x 131); scene_info/<scene>.0.npz with object arrays as the
real files have them (an image without a path and one without a depth map, which the valid mask drops; their point tables are
None); overlap matrices with values on both sides of 0.3, exactly 0.3 (excluded) and exactly 1.0 (included), -1 on the diagonal;
a scene with more candidate pairs than val_num_per_scene (25) and train_debug_num_per_scene (10), so that the seeded choice
runs; a listed scene without an info file; the two CSV files with one row of scene `/`."""
import os

import numpy as np

_M = -1.0
RECIPE = {
    "seed": 20250,
    "n_points": 30,
    "scenes": {
        # 4 images, one without a path: 3 valid
        "9001": {"sizes": [[40, 56], [64, 48], [97, 131], [57, 83]], "no_path": [1], "no_depth": [],
                 "overlap": [[_M, 0.9, 0.5, 0.3],
                             [0.9, _M, 0.9, 0.9],
                             [1.0, 0.9, _M, 0.31],
                             [0.29, 0.9, 0.0, _M]]},
        # 5 images, one without a depth map: 4 valid
        "9005": {"sizes": [[48, 64], [75, 100], [60, 90], [97, 131], [41, 57]], "no_path": [], "no_depth": [3],
                 "overlap": [[_M, 0.45, 0.2, 0.8, 1.0],
                             [0.35, _M, 0.6, 0.8, 0.3],
                             [0.1, 0.7, _M, 0.8, 0.55],
                             [0.8, 0.8, 0.8, _M, 0.8],
                             [1.0, 0.30000001, 0.4, 0.8, _M]]},
        # 6 images, all valid: 27 candidate pairs of 30
        "9022": {"sizes": [[56, 40], [66, 88], [90, 120], [45, 61], [80, 96], [97, 131]], "no_path": [], "no_depth": [],
                 "overlap": [[_M, 0.5, 0.6, 0.7, 0.8, 0.9],
                             [0.5, _M, 0.3, 0.7, 0.8, 0.9],
                             [0.5, 0.6, _M, 0.1, 0.8, 0.9],
                             [0.5, 0.6, 0.7, _M, 0.0, 0.9],
                             [0.5, 0.6, 0.7, 0.8, _M, 1.0],
                             [0.5, 0.6, 0.7, 0.8, 0.9, _M]]},
    },
    # made-up lists in the format of the reference's (names separated by white space); 9099 has no info file
    "lists": {"train": ["9001", "9099", "9005"], "train_debug": ["9022"], "validation": ["9022", "9001"], "test": ["9005"]},
    # rows of the two pair files: scene, source image (size), target image (size), number of points
    "MegaDepthTest": [["0015", "a.jpg", [60, 80], "b.jpg", [75, 57], 7], ["/", "c.jpg", [48, 64], "d.jpg", [97, 131], 5],
                      ["0022", "e.jpg", [50, 70], "f.jpg", [50, 70], 9]],
    "RobotCarMatching": [["overcast", "1.jpg", [64, 64], "2.jpg", [64, 64], 6], ["/", "3.jpg", [40, 56], "4.jpg", [72, 96], 4],
                         ["night", "5.jpg", [80, 60], "6.jpg", [61, 85], 8]],
}
LIST_FILES = {"train": "train_scenes_MegaDepth.txt", "train_debug": "train_debug_scenes_MegaDepth.txt",
              "validation": "validation_scenes_MegaDepth.txt", "test": "test_scenes_MegaDepth.txt"}


def _image(rng, h, w):
    """smooth colour ramps plus noise, so that a resize has something to interpolate"""
    y, x = np.mgrid[0:h, 0:w]
    base = np.stack([(x * 255 // max(w - 1, 1)), (y * 255 // max(h - 1, 1)), ((x + y) * 255 // max(h + w - 2, 1))], -1)
    return np.clip(base + rng.integers(-40, 41, (h, w, 3)), 0, 255).astype(np.uint8)


def _save(arr, *path):
    from PIL import Image
    os.makedirs(os.path.dirname(os.path.join(*path)), exist_ok=True)
    Image.fromarray(arr).save(os.path.join(*path), quality=90)


def _objects(values):
    out = np.empty(len(values), dtype=object)
    for i, v in enumerate(values):
        out[i] = v
    return out


def _pairs_csv(rng, rows, images_dir, csv_path):
    lines = [",scene,source_image,target_image,XA,YA,XB,YB"]
    for n, (scene, src, src_size, trg, trg_size, count) in enumerate(rows):
        sub = "." if scene == "/" else scene
        _save(_image(rng, *src_size), images_dir, sub, src)
        _save(_image(rng, *trg_size), images_dir, sub, trg)
        cols = []
        for (h, w) in (src_size, trg_size):
            cols.append(";".join(repr(float(v)) for v in np.round(rng.uniform(0, w - 1, count), 3)))
            cols.append(";".join(repr(float(v)) for v in np.round(rng.uniform(0, h - 1, count), 3)))
        lines.append(",".join([str(n), scene, src, trg] + cols))
    os.makedirs(os.path.dirname(csv_path), exist_ok=True)
    with open(csv_path, "w") as f:
        f.write("\n".join(lines) + "\n")


def build_tree(data_dir, recipe=RECIPE):
    """writes <data_dir>/MegaDepth and <data_dir>/RobotCarMatching as the recipe says.  Everything is drawn in a fixed order
    from one seeded generator, so the same recipe gives the same tables."""
    rng = np.random.default_rng(int(recipe["seed"]))
    root = os.path.join(data_dir, "MegaDepth")
    os.makedirs(os.path.join(root, "scene_info"), exist_ok=True)
    for scene, spec in sorted(recipe["scenes"].items()):
        ids = rng.choice(10 ** 6, int(recipe["n_points"]), replace=False)
        paths, depths, points = [], [], []
        for k, (h, w) in enumerate(spec["sizes"]):
            rel = f"Undistorted_SfM/{scene}/images/{scene}_{k:02d}.jpg"
            _save(_image(rng, h, w), root, rel)
            seen = ids[rng.random(len(ids)) < 0.6]
            table = {int(i): np.array([rng.uniform(0, w - 1), rng.uniform(0, h - 1)]) for i in rng.permutation(seen)}
            bad = k in spec["no_path"] or k in spec["no_depth"]
            paths.append(None if k in spec["no_path"] else rel)
            depths.append(None if k in spec["no_depth"] else f"phoenix/S6/zl548/MegaDepth_v1/{scene}/dense0/depths/{scene}_{k:02d}.h5")
            points.append(None if bad else table)
        np.savez(os.path.join(root, "scene_info", f"{scene}.0.npz"), image_paths=_objects(paths), depth_paths=_objects(depths),
                 points3D_id_to_2D=_objects(points), overlap_matrix=np.asarray(spec["overlap"], dtype=np.float64))
    os.makedirs(os.path.join(root, "lists"), exist_ok=True)
    for split, scenes in recipe["lists"].items():
        with open(os.path.join(root, "lists", LIST_FILES[split]), "w") as f:
            f.write("\n".join(scenes) + "\n")
    _pairs_csv(rng, recipe["MegaDepthTest"], os.path.join(root, "Test", "test1600Pairs"), os.path.join(root, "Test", "test1600Pairs.csv"))
    rc = os.path.join(data_dir, "RobotCarMatching")
    _pairs_csv(rng, recipe["RobotCarMatching"], os.path.join(rc, "images"), os.path.join(rc, "test6511.csv"))
    return data_dir


_PIPE = "data_modules.transforms."


def train_transforms(crop, elastic=True, photometric=True):
    """the transforms of uawarpc_stage2.yaml's training section (stage 1: its three smaller ranges and no elastic field)"""
    keys = {"apply_keys": ["image_prime"]}
    photo = [{"class_path": _PIPE + "ColorJitter", "init_args": dict(keys, brightness=0.6, contrast=0.6, saturation=0.6, hue=0)},
             {"class_path": _PIPE + "ChannelShuffle", "init_args": dict(keys)},
             {"class_path": _PIPE + "RandomGaussianBlur", "init_args": dict(keys, p=0.2, kernel_size=7, sigma=[0.2, 2.0])}]
    flow = dict(keys, include_transforms=["hom", "tps", "afftps"], random_alpha=0.26, random_s=0.45, random_tx=0.25,
                random_ty=0.25, random_t_hom=0.4 if elastic else 0.333, random_t_tps=0.4 if elastic else 0.333,
                random_t_tps_for_afftps=0.26 if elastic else 0.08, parameterize_with_gaussian=False, add_elastic=elastic)
    return ([{"class_path": _PIPE + "ToTensor"}] + (photo if photometric else []) +
            [{"class_path": _PIPE + "ConvertImageDtype"}, {"class_path": _PIPE + "Normalize"},
             {"class_path": _PIPE + "CompositeFlow", "init_args": flow},
             {"class_path": _PIPE + "CenterCrop", "init_args": {"size": list(crop)}}])


def eval_transforms(resize=None):
    """val: ToTensor, ConvertImageDtype, Normalize; test (resize given): Resize(lanczos) in front, PadBottomRight behind"""
    plain = [{"class_path": _PIPE + "ToTensor"}, {"class_path": _PIPE + "ConvertImageDtype"}, {"class_path": _PIPE + "Normalize"}]
    if resize is None:
        return plain
    return ([{"class_path": _PIPE + "Resize", "init_args": {"size": resize, "img_interpolation": "lanczos"}}] + plain +
            [{"class_path": _PIPE + "PadBottomRight", "init_args": {"same_shape_keys": ["image", "image_ref"]}}])


def data_section(dims=(160, 160), crop=(128, 160), val_dims=(128, 160), test_resize=128, batch_size=2, num_workers=0,
                 exchange=0.5, in_memory=True, robotcar_dims=(96, 96), elastic=True):
    """a `data:` section in the layout of the reference's uawarpc_stage2.yaml (elastic=False: stage 1's), at the tree's scale.
    (The reference's RobotCarMatching section has no dims and reads at the reader's 1024 x 1024; the tree's files get a smaller
    size.  The elastic field draws bump centres 3 x 40 pixels from every border: a frame below 240 pixels takes stage 1's
    section.)"""
    pair = ["image", "image_ref"]
    return {"class_path": "data_modules.CombinedDataModule", "init_args": {
        "batch_size": batch_size, "num_workers": num_workers, "load_config": {
            "train": {"MegaDepth": {"store_scene_info_in_memory": in_memory, "exchange_images_with_proba": exchange,
                                    "dims": list(dims), "load_keys": pair + ["image_prime"],
                                    "transforms": train_transforms(crop, elastic)}},
            "val": {"MegaDepth": {"dims": list(val_dims), "load_keys": list(pair), "transforms": eval_transforms()}},
            "test": {"MegaDepth": {"load_keys": list(pair), "transforms": eval_transforms(test_resize)},
                     "RobotCarMatching": {"dims": list(robotcar_dims), "load_keys": list(pair),
                                          "transforms": eval_transforms(test_resize)}}}}}
