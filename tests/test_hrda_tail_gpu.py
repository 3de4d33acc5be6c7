"""GPU: the fused HRDA logit merge (csrc/hrdatail.hip, refign_amd/hrdatail.py) against the element-wise chain of seg.hrda_head it
replaces (seg._HRDA_TAIL_FUSED = False: the comparison path) and against the same formulas in fp64 on the CPU.

Reference semantics: models/hrda.py:139-235.  ONE rule for every comparison: the fused path's maximum absolute error against fp64
must not exceed the chain's maximum absolute error against fp64, per output tensor.  The forward reproduces the chain's roundings
one by one, so there it is also asserted BIT-EQUAL to the chain.  (Measured with fp32 operands, which the kernels therefore do not
take: forward 1 fp32 ulp from the chain in either direction, 9.21e-07 against 9.05e-07 and 9.76e-07 against 8.88e-07 -- the blend's
fma choice; gradients 5e-08 ... 1.5e-07 against 1e-07 ... 1e-06.)  Each figure is printed before it is asserted
(profiles/hrda_tail_parity.txt is this file's `-s` output)."""
import os
import sys
from types import SimpleNamespace

import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from guardband import GuardArena  # noqa: E402

pytestmark = pytest.mark.gpu

K = 19
OS = 4                                   # head_os; crop offsets are multiples of 2 * OS
DTYPES = [torch.bfloat16]                # the kernels' domain: bf16 under autocast (test_other_precisions_stay_on_the_chain)
DT_IDS = ["bf16-autocast"]


def _autocast(dtype):
    return torch.autocast("cuda", dtype=dtype, enabled=dtype != torch.float32)


def _head(training, is_teacher, a, k=K):
    """seg.hrda_head around a stub decode head: scale attention = `a`, class logits = the features handed in."""
    from refign_amd import seg
    stub = SimpleNamespace(training=training, num_classes=k)
    return seg.hrda_head(stub, lambda feats: a, OS, is_teacher=is_teacher)(lambda feats: feats[0])


def _chain(fn):
    """fn() on the element-wise chain"""
    from refign_amd import seg
    saved = seg._HRDA_TAIL_FUSED
    seg._HRDA_TAIL_FUSED = False
    try:
        return fn()
    finally:
        seg._HRDA_TAIL_FUSED = saved


def _padded_cl(x, pad):
    """the same values as a channels-last view of a buffer with `pad` channels: how the decode head hands its logits over"""
    n, k, h, w = x.shape
    buf = torch.full((n, h, w, pad), 7.0, dtype=x.dtype, device=x.device)
    buf[..., :k] = x.permute(0, 2, 3, 1)
    return buf[..., :k].permute(0, 3, 1, 2)


def _cl(x):
    """dense channels-last: the memory format of the decode head's logits (the chain's result is then channels-last too)"""
    return x.contiguous(memory_format=torch.channels_last)


def _up64(x):
    return F.interpolate(x, scale_factor=2, mode="bilinear", align_corners=False)


def _err(x, ref):
    return float((x.detach().double().cpu() - ref).abs().max())


def _rule(name, fused, chain, ref, bit_equal=False):
    ef, ec = _err(fused, ref), _err(chain, ref)
    eq = torch.equal(fused, chain)
    print(f"hrda_tail {name}: max |err| vs fp64  fused {ef:.4e}  chain {ec:.4e}  bit-equal {eq}")
    assert fused.dtype == chain.dtype and fused.shape == chain.shape, (fused.dtype, chain.dtype)
    assert ef <= ec, (name, ef, ec)
    if bit_equal:
        assert eq, name


# ---- teacher -----------------------------------------------------------------------------------------------------------------------
def _slide_boxes(H, W):
    """the sliding crops of an (H, W) image as hrda_backbone cuts them, scaled to the (2h, 2w) logit grid"""
    from refign_amd import seg
    _, boxes = seg.extract_slide_crop(torch.zeros(1, 1, H, W), (H // 2, W // 2))
    return [list(seg.scale_box(b, OS)) for b in boxes]


def _teacher_inputs(dev, dtype, nl, h, w, hc, wc, nb, seed):
    g = torch.Generator().manual_seed(seed)
    a = (2.0 * torch.randn(nl, K, h, w, generator=g)).to(dtype)
    lr = (3.0 * torch.randn(nl, K, h, w, generator=g)).to(dtype)
    hr = (3.0 * torch.randn(nb * nl, K, hc, wc, generator=g)).to(dtype)
    return a, lr, hr


def _teacher_ref(a, lr, hr, boxes):
    a, lr, hr = a.double(), lr.double(), hr.double()
    nl, _, h, w = lr.shape
    att = torch.sigmoid(a)
    preds = torch.zeros(nl, K, 2 * h, 2 * w, dtype=torch.float64)
    count = torch.zeros(nl, 1, 2 * h, 2 * w, dtype=torch.float64)
    for i, (y1, y2, x1, x2) in enumerate(boxes):
        preds[:, :, y1:y2, x1:x2] += hr[i * nl:(i + 1) * nl]
        count[:, :, y1:y2, x1:x2] += 1
    return _up64(att) * (preds / count) + _up64((1 - att) * lr)


def _teacher_head(a, lr, hr, boxes_img, dtype):
    """the teacher branch of hrda_head on image-pixel boxes (it scales them in place)"""
    with torch.no_grad(), _autocast(dtype):
        return _head(False, True, a)(((lr,), (hr,), [list(b) for b in boxes_img]))


def _teacher_chain_ops(a, lr, hr, boxes, dtype):
    """The teacher branch's own operations, one by one, for the one case hrda_head cannot be handed: a single crop as large as the
    image has crop logits of (2h, 2w), and hrda_head splits ONE decode-head batch into lr_seg and hr_seg of equal size."""
    nl = lr.shape[0]
    with torch.no_grad(), _autocast(dtype):
        att = torch.sigmoid(a)
        up_lr = F.interpolate((1 - att) * lr, scale_factor=2, mode='bilinear', align_corners=False)
        Hh, Ww = max(b[1] for b in boxes), max(b[3] for b in boxes)
        preds = lr.new_zeros((nl, K, Hh, Ww))
        count = lr.new_zeros((nl, 1, Hh, Ww))
        for i, (y1, y2, x1, x2) in enumerate(boxes):
            preds[:, :, y1:y2, x1:x2] += hr[i * nl:(i + 1) * nl]
            count[:, :, y1:y2, x1:x2] += 1
        up_att = F.interpolate(att, scale_factor=2, mode='bilinear', align_corners=False)
        return up_att * (preds / count) + up_lr


TEACHER = {
    # name: (image H, W, boxes in image pixels or None = the sliding crops)
    "slide-72x104": (72, 104, None),                     # 9 crops of 9 x 13 on 18 x 26; stride 18 / 4 truncates; counts 1, 2, 4
    "single-crop": (72, 104, [[0, 72, 0, 104]]),         # crop == image
}


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("case", list(TEACHER))
def test_teacher_merge(dev, case, dtype):
    from refign_amd import hrdatail, seg
    H, W, boxes_img = TEACHER[case]
    if boxes_img is None:
        _, boxes_img = seg.extract_slide_crop(torch.zeros(1, 1, H, W), (H // 2, W // 2))
    boxes = [list(seg.scale_box(b, OS)) for b in boxes_img]
    nl, h, w = 2, H // (2 * OS), W // (2 * OS)
    hc, wc = boxes[0][1] - boxes[0][0], boxes[0][3] - boxes[0][2]
    a, lr, hr = _teacher_inputs(dev, dtype, nl, h, w, hc, wc, len(boxes), 11)
    if case == "slide-72x104":
        assert len(boxes) == 9 and (hc, wc) == (9, 13) and boxes[4] == [4, 13, 6, 19]
    ref = _teacher_ref(a, lr, hr, boxes)
    ad, lrd, hrd = (_cl(t.to(dev)) for t in (a, lr, hr))
    if case == "single-crop":
        chain = _teacher_chain_ops(ad, lrd, hrd, boxes, dtype)
    else:
        chain = _chain(lambda: _teacher_head(ad, lrd, hrd, boxes_img, dtype))
    with torch.no_grad(), _autocast(dtype):
        fused = hrdatail.merge_slide(ad, lrd, hrd, boxes)
        # the decode head's layout: channels-last views of padded buffers
        fused_cl = hrdatail.merge_slide(_padded_cl(ad, 24), _padded_cl(lrd, 24), _padded_cl(hrd, 24), boxes)
    assert fused is not None and fused_cl is not None
    assert fused.stride() == chain.stride()
    _rule(f"teacher {case} {DT_IDS[DTYPES.index(dtype)]}", fused, chain, ref, bit_equal=True)
    assert torch.equal(fused_cl, fused)
    if case != "single-crop":
        wired = _teacher_head(ad, lrd, hrd, boxes_img, dtype)         # through hrda_head with the constant on
        assert torch.equal(wired, fused)


def test_teacher_uncovered_pixel_falls_back(dev):
    """Boxes that reach the last row and column but leave pixels uncovered: the entry point declines, hrda_head takes the chain
    (0 / 0 in the uncovered pixels and all)."""
    from refign_amd import hrdatail
    boxes_img = [[0, 36, 0, 52], [36, 72, 52, 104]]
    boxes = [[0, 9, 0, 13], [9, 18, 13, 26]]
    a, lr, hr = (_cl(t.to(dev)) for t in _teacher_inputs(dev, torch.bfloat16, 2, 9, 13, 9, 13, 2, 12))
    with torch.no_grad(), _autocast(torch.bfloat16):
        assert hrdatail.merge_slide(a, lr, hr, boxes) is None
        # one pixel short of a cover, and more than 16 boxes
        assert hrdatail.merge_slide(a, lr, torch.cat((hr, hr)), boxes + [[0, 9, 13, 26], [9, 18, 0, 13]]) is not None
        assert hrdatail.merge_slide(a, lr, torch.cat((hr, hr)), boxes + [[0, 9, 13, 26], [8, 17, 0, 13]]) is None
        many = [[0, 9, 0, 13], [9, 18, 13, 26], [0, 9, 13, 26], [9, 18, 0, 13]] * 5
        assert hrdatail.merge_slide(a, lr, torch.cat([hr] * 10), many) is None
    today = _chain(lambda: _teacher_head(a, lr, hr, boxes_img, torch.bfloat16))
    got = _teacher_head(a, lr, hr, boxes_img, torch.bfloat16)
    assert torch.isnan(today).any()
    assert torch.equal(got.view(torch.int32), today.view(torch.int32))


def test_other_precisions_stay_on_the_chain(dev):
    """fp32 operands, and bf16 operands outside autocast (where the chain returns bf16): both wrappers decline, hrda_head returns
    the chain's result."""
    from refign_amd import hrdatail, seg
    boxes_img = seg.extract_slide_crop(torch.zeros(1, 1, 72, 104), (36, 52))[1]
    boxes = _slide_boxes(72, 104)
    box = seg.DeviceBox(torch.tensor((16, 24), dtype=torch.long, device=dev), 36, 52, 2 * OS)
    for dtype, cast in ((torch.float32, torch.float32), (torch.bfloat16, torch.float32)):      # cast float32: autocast off
        a, lr, hr = (_cl(t.to(dev)) for t in _teacher_inputs(dev, dtype, 2, 9, 13, 9, 13, 9, 15))
        with torch.no_grad(), _autocast(cast):
            assert hrdatail.merge_slide(a, lr, hr, boxes) is None
            assert hrdatail.fuse_crop(a, lr, hr[:2], box, float(OS)) is None
        today = _chain(lambda: _teacher_head(a, lr, hr, boxes_img, cast))
        got = _teacher_head(a, lr, hr, boxes_img, cast)
        assert got.dtype == dtype and torch.equal(got, today)
        with _autocast(cast):
            s_today = _chain(lambda: _head(True, False, a)(((lr,), (hr[:2],), [box])))[0]
            s_got = _head(True, False, a)(((lr,), (hr[:2],), [box]))[0]
        assert s_got.dtype == dtype and torch.equal(s_got, s_today)


@pytest.mark.parametrize("H,W", [(72, 104), (1080, 1920)])
def test_real_box_sets_cover_every_pixel(dev, H, W):
    """The sliding crops of the real workload, built on the CPU by extract_slide_crop and scale_box, cover the whole (2h, 2w) grid
    and reach its last row and column -- so the entry point never declines them."""
    from refign_amd import hrdatail
    boxes = _slide_boxes(H, W)
    h2, w2 = H // OS, W // OS
    count = torch.zeros(h2, w2, dtype=torch.int32)
    for y1, y2, x1, x2 in boxes:
        count[y1:y2, x1:x2] += 1
    assert len(boxes) == 9 and int(count.min()) >= 1 and sorted(count.unique().tolist()) == [1, 2, 4]
    assert (max(b[1] for b in boxes), max(b[3] for b in boxes)) == (h2, w2)
    hc, wc = boxes[0][1] - boxes[0][0], boxes[0][3] - boxes[0][2]
    a, lr, hr = (t.to(dev) for t in _teacher_inputs(dev, torch.bfloat16, 1, h2 // 2, w2 // 2, hc, wc, 9, 13))
    with torch.no_grad(), _autocast(torch.bfloat16):
        assert hrdatail.merge_slide(a, lr, hr, boxes) is not None


@pytest.mark.parametrize("fill", [0xFF, 0x7B])
def test_teacher_guard_band(dev, fill):
    from refign_amd import hrdatail
    boxes = _slide_boxes(72, 104)
    a, lr, hr = (t.to(dev) for t in _teacher_inputs(dev, torch.bfloat16, 2, 9, 13, 9, 13, 9, 14))
    with torch.no_grad(), _autocast(torch.bfloat16):
        clean = hrdatail.merge_slide(a, lr, hr, boxes)
        arena = GuardArena(dev, fill, 4 << 20)
        pa, pl, ph = arena.place(_padded_cl(a, 24)), arena.place(lr), arena.place(hr)
        with arena.allocations():
            got = hrdatail.merge_slide(pa, pl, ph, boxes)
    arena.check()
    assert torch.equal(got, clean)


# ---- student -----------------------------------------------------------------------------------------------------------------------
STUDENT = {
    # name: (n, K, logits h, w): image 8 h x 8 w, crop = its half, crop logits h x w
    "9x13": (2, K, 9, 13),
    "7x11-K5": (3, 5, 7, 11),        # 3 * 5 * 14 * 22 outputs: no multiple of a wave or a workgroup, K odd
}
_STUDENT_CACHE = {}


def _offsets(h, w):
    ymax, xmax = (8 * h - 4 * h) // 8 * 8, (8 * w - 4 * w) // 8 * 8
    return {"zero": (0, 0), "max": (ymax, xmax), "interior": (16, 24)}


def _student_ref(a, lr, hr, g, off, h, w):
    """fp64 on the CPU: the result and the three gradients for upstream gradient g"""
    a, lr, hr = (t.double().detach().requires_grad_() for t in (a, lr, hr))
    hs, ws = int(4 * h / 8.0), int(4 * w / 8.0)
    mask = torch.zeros(1, 1, h, w, dtype=torch.float64)
    mask[:, :, off[0] // 8:off[0] // 8 + hs, off[1] // 8:off[1] // 8 + ws] = 1
    att = torch.sigmoid(a) * mask
    iy, ix = off[0] // 4, off[1] // 4
    ins = F.pad(hr, (ix, 2 * w, iy, 2 * h))[:, :, :2 * h, :2 * w]          # hr written at (iy, ix) of zeros(2h, 2w)
    out = _up64(att) * ins + _up64((1 - att) * lr)
    grads = torch.autograd.grad(out, [a, lr, hr], g.double())
    return out.detach(), grads


def _border_g(g, off, h, w):
    """g kept only on the border rows and columns of the inserted box"""
    iy, ix = off[0] // 4, off[1] // 4
    keep = torch.zeros_like(g)
    ys, xs = [iy, min(iy + h, 2 * h) - 1], [ix, min(ix + w, 2 * w) - 1]
    keep[:, :, ys, ix:ix + w] = 1
    keep[:, :, iy:iy + h, xs] = 1
    return g * keep


def _student_run(dev, dtype, a, lr, hr, g, box, fused, layout="dense"):
    """(out, grad_a, grad_lr, grad_hr) on the device: the direct call of the fused Function or hrda_head on the chain"""
    from refign_amd import hrdatail
    prep = (lambda t: _padded_cl(t, 64)) if layout == "padded" else _cl
    a, lr, hr = (prep(t.to(dev)).detach().requires_grad_() for t in (a, lr, hr))
    with _autocast(dtype):
        if fused:
            out = hrdatail.fuse_crop(a, lr, hr, box, float(OS))
            assert out is not None
        else:
            out = _chain(lambda: _head(True, False, a, a.shape[1])(((lr,), (hr,), [box])))[0]
    grads = torch.autograd.grad(out, [a, lr, hr], g.to(dev))
    return (out.detach(),) + tuple(grads)


def _student_setup(dev, case, dtype, where, gkind):
    key = (case, dtype, where, gkind)
    if key not in _STUDENT_CACHE:
        from refign_amd import seg
        n, k, h, w = STUDENT[case]
        gen = torch.Generator().manual_seed(100 + h)
        a = (2.0 * torch.randn(n, k, h, w, generator=gen)).to(dtype)
        lr = (3.0 * torch.randn(n, k, h, w, generator=gen)).to(dtype)
        hr = (3.0 * torch.randn(n, k, h, w, generator=gen)).to(dtype)
        g = torch.randn(n, k, 2 * h, 2 * w, generator=gen)
        off = _offsets(h, w)[where]
        if gkind == "border":
            g = _border_g(g, off, h, w)
        box = seg.DeviceBox(torch.tensor(off, dtype=torch.long, device=dev), 4 * h, 4 * w, 2 * OS)
        ref = _student_ref(a, lr, hr, g, off, h, w)
        chain = _student_run(dev, dtype, a, lr, hr, g, box, fused=False)
        _STUDENT_CACHE[key] = (a, lr, hr, g, box, ref, chain)
    return _STUDENT_CACHE[key]


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("gkind", ["random", "border"])
@pytest.mark.parametrize("where", ["zero", "max", "interior"])
@pytest.mark.parametrize("case", list(STUDENT))
def test_student_fuse_crop(dev, case, where, gkind, dtype):
    a, lr, hr, g, box, (ref_out, ref_g), chain = _student_setup(dev, case, dtype, where, gkind)
    fused = _student_run(dev, dtype, a, lr, hr, g, box, fused=True)
    tag = f"student {case} {where} g={gkind} {DT_IDS[DTYPES.index(dtype)]}"
    assert fused[0].stride() == chain[0].stride()
    _rule(tag + " out", fused[0], chain[0], ref_out, bit_equal=True)
    for name, f, c, r in zip(("grad_a", "grad_lr", "grad_hr"), fused[1:], chain[1:], ref_g):
        _rule(f"{tag} {name}", f, c, r)
    # the decode head's layout (channels-last views of 64-channel buffers): the same bits
    padded = _student_run(dev, dtype, a, lr, hr, g, box, fused=True, layout="padded")
    for f, p in zip(fused, padded):
        assert torch.equal(f, p)
    # forward and backward once more: no atomics, the same bits
    again = _student_run(dev, dtype, a, lr, hr, g, box, fused=True)
    for f, p in zip(fused, again):
        assert torch.equal(f, p)


def test_student_wired_into_hrda_head(dev):
    """hrda_head with the constant on returns the fused result for a DeviceBox (and hands the crop logits and the box on)."""
    a, lr, hr, g, box, _, chain = _student_setup(dev, "9x13", torch.bfloat16, "interior", "random")
    ad, lrd, hrd = (t.to(dev).requires_grad_() for t in (a, lr, hr))
    with _autocast(torch.bfloat16):
        out, hr_logits, b = _head(True, False, ad)(((lrd,), (hrd,), [box]))
    assert b is box and tuple(hr_logits.shape[2:]) == (box.h, box.w)
    assert type(out.grad_fn).__name__.startswith("_FuseCrop")
    grads = torch.autograd.grad(out, [ad, lrd, hrd], g.to(dev))
    fused = _student_run(dev, torch.bfloat16, a, lr, hr, g, box, fused=True)
    for x, y in zip((out,) + tuple(grads), fused):
        assert torch.equal(x, y)


def test_student_offset_is_device_data(dev):
    """The offset tensor's CONTENTS change between two calls, nothing is rebuilt: the second result follows them."""
    a, lr, hr, g, _, _, _ = _student_setup(dev, "9x13", torch.bfloat16, "zero", "random")
    from refign_amd import seg
    offs = _offsets(9, 13)
    box = seg.DeviceBox(torch.tensor(offs["zero"], dtype=torch.long, device=dev), 36, 52, 2 * OS)
    first = _student_run(dev, torch.bfloat16, a, lr, hr, g, box, fused=True)
    box.off.copy_(torch.tensor(offs["max"], dtype=torch.long))
    second = _student_run(dev, torch.bfloat16, a, lr, hr, g, box, fused=True)
    want = _student_setup(dev, "9x13", torch.bfloat16, "max", "random")[6]
    assert not torch.equal(first[0], second[0])
    assert torch.equal(second[0], want[0])
    fresh = _student_run(dev, torch.bfloat16, a, lr, hr, g, _student_setup(dev, "9x13", torch.bfloat16, "max", "random")[4], fused=True)
    for x, y in zip(second, fresh):
        assert torch.equal(x, y)


@pytest.mark.parametrize("fill", [0xFF, 0x7B])
def test_student_guard_band(dev, fill):
    """Operands next to poison, every output carved from poisoned (stale) memory: nothing outside the outputs is written and the
    results are those of clean memory -- the backward overwrites, it does not accumulate."""
    from refign_amd import hrdatail, seg
    a, lr, hr, g, box, _, _ = _student_setup(dev, "7x11-K5", torch.bfloat16, "max", "random")
    clean = _student_run(dev, torch.bfloat16, a, lr, hr, g, box, fused=True)
    arena = GuardArena(dev, fill, 4 << 20)
    pa, pl, ph = (arena.place(_padded_cl(t.to(dev), 8)).requires_grad_() for t in (a, lr, hr))
    pbox = seg.DeviceBox(arena.place(box.off), box.h, box.w, box.divisible)
    pg = arena.place(g.to(dev))
    with _autocast(torch.bfloat16), arena.allocations():
        out = hrdatail.fuse_crop(pa, pl, ph, pbox, float(OS))
        grads = torch.autograd.grad(out, [pa, pl, ph], pg)
    arena.check()
    for x, y in zip((out.detach(),) + tuple(grads), clean):
        assert torch.equal(x, y)
