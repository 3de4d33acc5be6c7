"""N4: the DACS data step on the HIP kernels (csrc/dacs.hip, refign_amd/dacs.py) against the torch formulation of the same
operators in refign_amd/uda.py (strong_transform / one_mix / get_class_masks: helpers/dacs_transforms.py:14-24,43-112 as
called by models/segmentation_model.py:525-582), with identical random draws.  Labels and the mixed / unmixed choice are
exact; the image agrees to float rounding (1e-5: the contrast mean is a different summation order, the blur taps are
rounded from float64).

The second half of the file holds the same kernels to the fp64 reference of tests/dacs_ref.py, an independent statement of the
operators: all 24 jitter orders, per-sample switches mixed within a full batch of 8, the contrast mean at every position, the
label and bit-set edges of the mask, the blur against its whole window, and the refusals of the contract."""
import random
import types

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


def _inputs(dev, B, H, W, seed):
    g = torch.Generator(device="cpu").manual_seed(seed)
    src = torch.randn(B, 3, H, W, generator=g).to(dev)
    trg = torch.randn(B, 3, H, W, generator=g).to(dev)
    gt = torch.randint(0, 19, (B, H // 8, W // 8), generator=g).repeat_interleave(8, 1).repeat_interleave(8, 2)
    gt[torch.rand(B, H, W, generator=g) < 0.05] = 255
    probs = torch.softmax(4 * torch.randn(B, 19, H, W, generator=g), 1).to(dev)
    return src, trg, gt.to(dev), probs


@pytest.mark.parametrize("jitter", [False, True])
@pytest.mark.parametrize("blur", [False, True])
@pytest.mark.parametrize("B,H,W", [(2, 64, 96), (1, 40, 72)])
def test_dacs_mix_kernels_match_torch_formulation(monkeypatch, jitter, blur, B, H, W):
    from refign_amd.uda import DomainAdaptationSegmentationModel as M
    dev = torch.device("cuda:0")
    src, trg, gt, probs = _inputs(dev, B, H, W, 3)
    ns = types.SimpleNamespace(color_jitter_s=0.2, color_jitter_p=-1.0 if jitter else 2.0, blur=True,
                               pseudo_label_threshold=0.968, psweight_ignore_top=3, psweight_ignore_bottom=5)
    coins = iter([0.5, 0.9 if blur else 0.1] * 2)
    monkeypatch.setattr(random, "uniform", lambda a, b: next(coins))
    outs = []
    for kernel in ("0", "1"):
        monkeypatch.setenv("RFN_DACS_KERNEL", kernel)
        np.random.seed(5); torch.manual_seed(7)
        outs.append(M.get_dacs_mix(ns, trg, probs, src, gt))
    (img0, lbl0, w0), (img1, lbl1, w1) = outs
    assert img1.shape == img0.shape and lbl1.dtype == lbl0.dtype and w1.shape == w0.shape
    assert torch.equal(lbl0, lbl1)
    assert torch.equal(w0.float(), w1.float())
    assert float((img0.float() - img1).abs().max()) <= 1e-5 * max(1.0, float(img0.abs().max()))
    # the mix really took pixels of both images
    if not jitter and not blur:
        from_src = (img1 == src).all(1).float().mean()
        from_trg = (img1 == trg).all(1).float().mean()
        assert 0.2 < float(from_src) < 0.8 and abs(float(from_src + from_trg) - 1.0) < 1e-6


def test_dacs_draws_follow_the_reference_order(monkeypatch):
    """Same generator states after the call with and without the kernels: the step's later draws (HRDA crops, drop-path)
    do not depend on which implementation mixed the batch."""
    from refign_amd.uda import DomainAdaptationSegmentationModel as M
    dev = torch.device("cuda:0")
    src, trg, gt, probs = _inputs(dev, 2, 64, 96, 4)
    ns = types.SimpleNamespace(color_jitter_s=0.2, color_jitter_p=0.2, blur=True, pseudo_label_threshold=0.968,
                               psweight_ignore_top=0, psweight_ignore_bottom=0)
    states = []
    for kernel in ("0", "1"):
        monkeypatch.setenv("RFN_DACS_KERNEL", kernel)
        random.seed(1); np.random.seed(2); torch.manual_seed(3)
        M.get_dacs_mix(ns, trg, probs, src, gt)
        states.append((random.random(), float(np.random.rand()), float(torch.rand(()))))
    assert states[0] == states[1]


def test_class_set_prefetch_equals_torch_unique():
    """uda._prefetch_classes / _take_class_prefetch: the class set of the next batch from a fixed-size histogram + an
    asynchronous copy (no host synchronisation in the step) == torch.unique of the labels, ignore label included."""
    from refign_amd.uda import DomainAdaptationSegmentationModel as M
    dev = torch.device("cuda:0")
    g = torch.Generator(device="cpu").manual_seed(9)
    gt = torch.tensor([0, 3, 7, 18, 255, 11])[torch.randint(0, 6, (3, 40, 56), generator=g)].to(dev)
    ns = types.SimpleNamespace()
    M._prefetch_classes(ns, gt, 2)
    got = M._take_class_prefetch(ns, gt, 2)
    assert got is not None and torch.equal(got.cpu(), torch.unique(gt[:2]).cpu())
    assert M._take_class_prefetch(ns, gt, 2) is None                      # consumed
    M._prefetch_classes(ns, gt, 2)
    assert M._take_class_prefetch(ns, gt.clone(), 2) is None              # a different tensor: not this prefetch


@pytest.mark.parametrize("jitter", [False, True])
@pytest.mark.parametrize("blur", [False, True])
def test_dacs_mix_halves_equal_the_whole(jitter, blur):
    """Round 5: the mix in two launches -- the image half before the teacher's pseudo-labels exist (the student's forward on the
    mixed image starts next to the teacher branch), labels + weights afterwards -- is bit for bit the one-launch mix."""
    from refign_amd import dacs
    dev = torch.device("cuda:0")
    B, H, W = 2, 64, 96
    src, trg, gt, probs = _inputs(dev, B, H, W, 11)
    pp, pl = torch.max(probs, 1)
    pw = torch.full_like(pp, 0.37)
    np.random.seed(5); torch.manual_seed(7)
    bits = dacs.draw_class_bits(torch.unique(gt), B)
    jit = [dacs.draw_jitter(0.2) if jitter else None for _ in range(B)]
    sig = [0.8 if blur else None for _ in range(B)]
    img, lbl, wgt = dacs.mix(src, trg, gt, pl, pw, bits, jit, sig)
    img_a, none_l, none_w = dacs.mix(src, trg, gt, None, None, bits, jit, sig, part="image")
    none_i, lbl_b, wgt_b = dacs.mix(None, None, gt, pl, pw, bits, jit, sig, part="labels")
    assert none_l is None and none_w is None and none_i is None
    assert torch.equal(img, img_a) and torch.equal(lbl, lbl_b) and torch.equal(wgt, wgt_b)


# ---------------------------------------------------------------------------------------------------------------------
# The kernels against the fp64 reference of tests/dacs_ref.py, through dacs.mix with explicit jitter, blur_sigma, class_bits.
# Bound: min(M E + 2^-23, 1e-5) in max|got - want| / max(1, max|want|), E the fp32 model's error on the very input
# (test_dacs_ref_cpu.py shows what that bound catches); labels, weights and every sample that is neither jittered nor blurred
# are bit-equal.  Every test prints its figures before it asserts (`pytest -s`); profiles/dacs_reference.txt is such a run.
# ---------------------------------------------------------------------------------------------------------------------
def _held_to_reference(dev, name, det=False, part="all"):
    import dacs_ref as dr
    from refign_amd import determinism
    c, (want_img, want_lbl, want_wgt) = dr.case(name), dr.case_reference(name)
    with determinism.deterministic(det):
        img, lbl, wgt = dr.run_kernels(c, dev, part)
    if part != "image":
        assert lbl.dtype == torch.long and wgt.dtype == torch.float32
        assert np.array_equal(lbl.cpu().numpy(), want_lbl) and np.array_equal(wgt.cpu().numpy(), want_wgt)
    else:
        assert lbl is None and wgt is None
    if part == "labels":
        assert img is None
        return None
    E, got = dr.case_E(name), img.cpu().numpy()
    err = dr.rel_err(got, want_img)
    print(f"DACS_BOUND {name} {'det' if det else 'atomic'} {part} kernel {err:.3e} model {E:.3e} "
          f"ratio {err / E if E > 0 else float('nan'):.3f} bound {dr.bound(E):.3e}")
    assert got.dtype == np.float32 and got.shape == want_img.shape
    plain = dr.plain_mix(c)
    for n in range(c.shape[0]):
        if c.jitter[n] is None and c.sigma[n] is None:
            assert np.array_equal(got[n], plain[n]), (name, n)          # 1 * s + 0 * t is exact
    assert err <= dr.bound(E)
    return img


def _jitter_cases():
    import dacs_ref as dr
    return dr.JITTER_CASES + dr.EVEN_CASES


@pytest.mark.parametrize("det", [False, True], ids=["atomic", "det"])
@pytest.mark.parametrize("name", _jitter_cases())
def test_jitter_all_orders_within_model_bound(dev, name, det):
    """All 24 operator orders (three batches of 8 per shape), factors and hue angles on both ends of their range; `-even`: jitter
    on for the even samples only, the odd ones are the plain mix bit for bit.  det: rfn_dacs_mix_jitter_det, same bound, and
    bit-equal when launched again."""
    img = _held_to_reference(dev, name, det)
    if det:
        assert torch.equal(img, _held_to_reference(dev, name, det))


@pytest.mark.parametrize("det", [False, True], ids=["atomic", "det"])
def test_contrast_mean_is_of_the_image_in_front_of_the_operator(dev, det):
    """Contrast at each of its four positions behind a brightness step that saturates a third of the image."""
    _held_to_reference(dev, "contrast-40x72", det)


@pytest.mark.parametrize("part", ["all", "image", "labels"])
def test_mask_label_edges(dev, part):
    """Labels 0, 5, 18, 30, 31, 40, 254, 255, -1 under bit sets with and without bit 30 and bit 31, in both halves of the mix."""
    _held_to_reference(dev, "mask-40x72", part=part)


def _blur_cases():
    import dacs_ref as dr
    return dr.BLUR_CASES + ("both-40x72",)


@pytest.mark.parametrize("name", _blur_cases())
def test_blur_against_the_whole_window(dev, name):
    """Windows 1x1, 3x7, 35x3 (wider than the kernel's 33 taps) and 3x69 (11 column blocks, the last ragged); sigma 0.15, 0.5
    and 1.15 and unblurred samples in one batch; impulses on both borders, and a constant image (taps summing to 1).
    both-40x72: jitter and blur switched per sample in every combination."""
    import dacs_ref as dr
    img = _held_to_reference(dev, name)
    if name.startswith("blur-17x20"):                                  # a 1x1 window: the blur launches and changes nothing
        assert any(s is not None for s in dr.case(name).sigma)
        assert np.array_equal(img.cpu().numpy(), dr.plain_mix(dr.case(name)))


def test_contract_refusals_launch_nothing(dev):
    """sigma > 1.25, an extent of 16 and a batch of 9 are RFN_EINVAL from the host-side check: RuntimeError from _lib.call, and
    the output buffers keep their contents."""
    import ctypes
    import dacs_ref as dr
    from refign_amd import _lib, dacs
    c = dr.case("blur-17x20-random")
    B = c.shape[0]

    def refused(fn, entry):
        with pytest.raises(RuntimeError) as e:
            fn()
        last = _lib.load_library().rfn_last_error().decode()
        assert entry in str(e.value) and "code -1" in str(e.value) and last and last in str(e.value)

    # through dacs.mix
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)   # noqa: E731
    bits = torch.tensor(list(c.bits), dtype=torch.int64, device=dev)
    args = (t(c.src), t(c.trg), t(c.gt), t(c.pseudo), t(c.pweight), bits, [None] * B)
    refused(lambda: dacs.mix(*args, [1.26] + [None] * (B - 1)), "rfn_dacs_blur")
    cut = lambda x: x[..., :16, :].contiguous()                        # noqa: E731
    refused(lambda: dacs.mix(*(cut(a) for a in args[:5]), bits, [None] * B, [0.5] * B), "rfn_dacs_blur")
    nine = lambda x: torch.cat([x, x])[:9].contiguous()                # noqa: E731
    refused(lambda: dacs.mix(*(nine(a) for a in args[:6]), [None] * 9, [None] * 9), "rfn_dacs_mix_jitter")
    # straight through the ABI on buffers whose contents show a launch
    H, W = c.shape[1:]
    x = torch.full((9, 3, H, W), 3.0, device=dev)
    tmp, out = torch.full_like(x, 5.0), torch.full_like(x, 7.0)
    on = (ctypes.c_int * 9)(*[1] * 9)
    cast = lambda a: ctypes.cast(a, ctypes.c_void_p)                   # noqa: E731
    sig = lambda v: cast((ctypes.c_double * 9)(*[v] * 9))              # noqa: E731
    blur = lambda b, h, s: _lib.call("rfn_dacs_blur", dev, x.data_ptr(), tmp.data_ptr(), out.data_ptr(), b, 3, h, W, 1, 1,   # noqa: E731
                                     cast(on), sig(s), sig(s))
    refused(lambda: blur(2, H, 1.26), "rfn_dacs_blur")
    refused(lambda: blur(2, 16, 0.5), "rfn_dacs_blur")
    refused(lambda: blur(9, H, 0.5), "rfn_dacs_blur")
    gt9 = torch.zeros(9, H, W, dtype=torch.long, device=dev)
    lbl, wgt = torch.full_like(gt9, 77), torch.full((9, H, W), 5.0, device=dev)
    ws = torch.zeros(dacs.MAX_BATCH, dtype=torch.float64, device=dev)
    order = (ctypes.c_int * 36)(*[0, 1, 2, 3] * 9)
    factor, hue = (ctypes.c_float * 36)(*[1.0] * 36), (ctypes.c_float * 81)(*[0.0] * 81)
    mean3, std3 = (ctypes.c_float * 3)(*dacs.IMNET_MEAN), (ctypes.c_float * 3)(*dacs.IMNET_STD)
    bits9 = torch.zeros(9, dtype=torch.int64, device=dev)
    for entry in ("rfn_dacs_mix_jitter", "rfn_dacs_mix_jitter_det"):
        refused(lambda: _lib.call(entry, dev, x.data_ptr(), x.data_ptr(), gt9.data_ptr(), gt9.data_ptr(), wgt.data_ptr(),
                                  out.data_ptr(), lbl.data_ptr(), wgt.data_ptr(), ws.data_ptr(), 9, H, W, bits9.data_ptr(), cast(on),
                                  cast(order), cast(factor), cast(hue), cast(mean3), cast(std3)), entry)
    torch.cuda.synchronize(dev)
    assert bool((tmp == 5.0).all()) and bool((out == 7.0).all()) and bool((lbl == 77).all()) and bool((wgt == 5.0).all())
    assert float(ws.abs().max()) == 0
