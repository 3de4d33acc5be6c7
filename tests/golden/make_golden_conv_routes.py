"""tests/golden/make_golden_conv_routes.py -- which kernels a convolution / ConvBNReLU call launches, as a fixture.

For every case in CASES this records, on the GPU, from freshly built modules each time:
  trace / library          the ordered (entry point, normalised arguments) list seen by a wrapper around _lib.call (a pointer is
                           "p", None is 0, ints and floats stay -- tools/abi_census.py::_short) and the keys the case adds to
                           mfma.LIBRARY_CALLS (with their counts), in the default mode
  det_trace / det_library  the same under determinism.deterministic(), which picks other kernel forms
  hashes                   sha256 of the bytes of the output, the input gradient(s) and every parameter gradient under
                           deterministic mode, plus dtype / shape / strides of the output
  raises                   [exception type, a short substring of its message] where the call raises instead (RAISES)
  aten_only                a case that is ATen's from end to end (ATEN_ONLY): nothing of this project is launched and no library
                           call is recorded, so its bits are the library's alone; held by its empty traces and by dtype, shape
                           and strides of the output, and no hash is stored for it
The generator runs every case twice in deterministic mode; a case whose two runs hash differently is marked "unstable" (held
by its traces alone), which is accepted only for a case that made a library call.  tests/test_conv_routes_gpu.py imports CASES
and record() from here and compares against conv_routes.json.  The fixture is a record of one commit's dispatch: it is
regenerated only by a change that means to move a route.

  python tests/golden/make_golden_conv_routes.py [--out tests/golden/conv_routes.json] [--only case,case]
(--only: record these cases and merge them into the existing file; the other entries stay as they were recorded)
"""
import argparse
import contextlib
import hashlib
import json
import os
import sys
from functools import partial

import torch
import torch.nn as nn

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

B, H, W = 2, 12, 20
BF, HF, F32 = torch.bfloat16, torch.float16, torch.float32
_leaky = partial(nn.LeakyReLU, negative_slope=0.1)


class Patch:
    """setattr / setenv with undo() (pytest's monkeypatch, for a run outside pytest)."""

    def __init__(self):
        self._undo = []

    def setattr(self, obj, name, value):
        self._undo.append(partial(setattr, obj, name, getattr(obj, name)))
        setattr(obj, name, value)

    def setenv(self, name, value):
        old = os.environ.get(name)
        self._undo.append((lambda: os.environ.pop(name, None)) if old is None else partial(os.environ.__setitem__, name, old))
        os.environ[name] = value

    def undo(self):
        while self._undo:
            self._undo.pop()()


def _short(a):
    if isinstance(a, float):
        return a
    if a is None:
        return 0
    if isinstance(a, int):
        return a if abs(a) < (1 << 31) else "p"
    return "p"


class Tracer:
    """The wrapper around _lib.call: install with patch.setattr(_lib, "call", tracer)."""

    def __init__(self, real):
        self.real, self.trace = real, []

    def __call__(self, name, device, *args):
        self.trace.append([name, [_short(a) for a in args]])
        return self.real(name, device, *args)


# ---------------------------------------------------------------------------------------------------------------------
# case builders: (dev, patch) -> dict(mods=[modules], x=tensor or list of tensors, call=f(x), grad=bool, autocast=dtype|None)
# Values are drawn on the CPU from the seeded default generator (record() seeds it), so they do not depend on the device.
# ---------------------------------------------------------------------------------------------------------------------
def _randomise(mods):
    for mod in mods:
        for m in mod.modules():
            if isinstance(m, nn.modules.batchnorm._BatchNorm):
                with torch.no_grad():
                    if m.weight is not None:
                        m.weight.uniform_(0.5, 1.5)
                        m.bias.normal_(0, 0.1)
                    m.running_mean.normal_(0, 0.1)
                    m.running_var.uniform_(0.5, 1.5)


def _x(c, dtype, h=H, w=W, b=B, dev=None):
    return torch.randn(b, c, h, w).to(dev).to(dtype).contiguous(memory_format=torch.channels_last)


def _spec(dev, mods, x, call, grad, autocast, train=True, frozen=False):
    """frozen: no parameter requires a gradient and neither does x, but the call runs with grad mode ON (no backward)."""
    _randomise(mods)
    for m in mods:
        m.to(dev).train(train)
        if frozen:
            m.requires_grad_(False)
    return dict(mods=mods, x=x, call=call, grad=grad and not frozen, grad_mode=grad or frozen, autocast=autocast)


def _block_case(args, kw, cin, dtype, grad, *, train=True, autocast="same", xdtype=None, shape=None, consts=(), env=(), out=False,
                drop=None, frozen=False):
    """One ConvBNReLU(*args, **kw) on a (B, cin, H, W) input."""
    def build(dev, patch):
        from refign_amd import layers
        from refign_amd.layers import ConvBNReLU
        for name, value in consts:
            patch.setattr(layers, name, value)
        for name, value in env:
            patch.setenv(name, value)
        m = ConvBNReLU(*args, **kw)
        b, h, w = shape or (B, H, W)
        x = _x(cin, xdtype or dtype, h, w, b, dev)
        kwargs = {}
        if drop is not None:
            kwargs["drop"] = ((torch.rand(b, drop, 1, 1) > 0.1).float() / 0.9).to(dev).to(dtype)
        if out:
            wide = torch.zeros(b, h, w, 2 * out, dtype=dtype, device=dev)
            kwargs["out"] = wide[..., out // 2:out // 2 + out].permute(0, 3, 1, 2)
        ac = dtype if autocast == "same" else autocast
        return _spec(dev, [m], x, lambda t: m(t, **kwargs), grad, ac if ac in (BF, HF) else None, train, frozen)
    return build


def _parts_case(dev, patch):
    from refign_amd.layers import ConvBNReLU
    m = ConvBNReLU(24, 16, 3, activation_layer=_leaky)
    x = [_x(16, F32, dev=dev), _x(8, F32, dev=dev)]
    return _spec(dev, [m], x, lambda t: m(t), False, None, train=False)


def _conv2d_case(args, kw, cin, dtype, grad, frozen=False):
    def build(dev, patch):
        from refign_amd.conv import Conv2d
        m = Conv2d(*args, **kw)
        return _spec(dev, [m], _x(cin, dtype, dev=dev), lambda t: m(t), grad, dtype if dtype in (BF, HF) else None, frozen=frozen)
    return build


def _logits_case(dtype, grad):
    def build(dev, patch):
        from refign_amd import seg
        conv = nn.Conv2d(64, 19, 1)
        return _spec(dev, [conv], _x(64, dtype, dev=dev), lambda t: seg._class_logits(conv, t), grad,
                     dtype if dtype in (BF, HF) else None)
    return build


def _bottleneck_case(dtype, grad, train):
    def build(dev, patch):
        from refign_amd import resnet
        m = resnet.Bottleneck(64, 16)
        return _spec(dev, [m], _x(64, dtype, dev=dev), lambda t: m(t), grad, dtype if dtype in (BF, HF) else None, train)
    return build


def _patch_statistics_case(train):
    def build(dev, patch):
        from refign_amd import align
        m = align.UncertaintyModule(1, search_size=9)
        x = torch.randn(B, 81, 6, 10).to(dev)
        return _spec(dev, [m], x, lambda t: m.patch_statistics(t), train, HF if train else None, train)
    return build


def _aspp_case(grad, consts=()):
    def build(dev, patch):
        from refign_amd import seg
        for name, value in consts:
            patch.setattr(seg, name, value)
        m = seg.ASPPWrapper(64, 64, sep=True, dilations=(1, 6, 12, 18), pool=False, norm_layer=nn.BatchNorm2d,
                            activation_layer=nn.ReLU)
        return _spec(dev, [m], _x(64, BF, dev=dev), lambda t: m(t), grad, BF)
    return build


CASES = {}
for _dt, _n in ((BF, "bf16"), (HF, "fp16")):
    CASES[f"pw64_grad_{_n}"] = _block_case((64, 64, 1), {}, 64, _dt, True)
    CASES[f"pw64_nograd_{_n}"] = _block_case((64, 64, 1), {}, 64, _dt, False)
    CASES[f"pw64_out_{_n}"] = _block_case((64, 64, 1), {}, 64, _dt, False, out=64)
    CASES[f"pw64to24_grad_{_n}"] = _block_case((64, 24, 1), {}, 64, _dt, True)
_DW = dict(dilation=6, padding=6, groups=64)
CASES.update({
    "pw64_grad_bf16_bn_kernel_off": _block_case((64, 64, 1), {}, 64, BF, True, env=(("RFN_BN_KERNEL", "0"),)),
    "dw64_nograd": _block_case((64, 64, 3), _DW, 64, BF, False),
    "dw64_grad": _block_case((64, 64, 3), _DW, 64, BF, True),
    "dw64_out": _block_case((64, 64, 3), _DW, 64, BF, False, out=64),
    "dw64_nograd_not_fused": _block_case((64, 64, 3), _DW, 64, BF, False, consts=(("_DW_BN_FUSED", False),)),
    "dw64_nograd_no_stats": _block_case((64, 64, 3), _DW, 64, BF, False, consts=(("_DW_BN_STATS", False),)),
    "dw64_grad_no_stats": _block_case((64, 64, 3), _DW, 64, BF, True, consts=(("_DW_BN_STATS", False),)),
    "dw12_nograd": _block_case((12, 12, 3), dict(dilation=6, padding=6, groups=12), 12, BF, False),
    "dw12_grad": _block_case((12, 12, 3), dict(dilation=6, padding=6, groups=12), 12, BF, True),
    "separable_nograd": _block_case((64, 64, 3), dict(dilation=6, padding=6, depthwise_separable=True), 64, BF, False),
    "separable_grad": _block_case((64, 64, 3), dict(dilation=6, padding=6, depthwise_separable=True), 64, BF, True),
    "separable_out": _block_case((64, 64, 3), dict(dilation=6, padding=6, depthwise_separable=True), 64, BF, False, out=64),
    "dense3x3_grad": _block_case((128, 64, 3), {}, 128, BF, True),
    "dense3x3_nograd": _block_case((128, 64, 3), {}, 128, BF, False),
    "dense3x3_grad_drop": _block_case((128, 64, 3), {}, 128, BF, True, drop=64),
    "dense3x3_drop_raises": _block_case((128, 12, 3), {}, 128, BF, True, drop=12),
    "eval_leaky_bf16": _block_case((64, 64, 3), dict(activation_layer=_leaky), 64, BF, False, train=False),
    "eval_leaky_fp32_split32": _block_case((64, 64, 3), dict(activation_layer=_leaky), 64, F32, False, train=False),
    "eval_parts_fp32_split32": _parts_case,
    "eval_slope02_bf16": _block_case((64, 64, 3), dict(activation_layer=partial(nn.LeakyReLU, 0.2)), 64, BF, False, train=False),
    "eval_slope02_fp32": _block_case((64, 64, 3), dict(activation_layer=partial(nn.LeakyReLU, 0.2)), 64, F32, False, train=False),
    "eval_bn_under_autograd_bf16": _block_case((64, 64, 3), {}, 64, BF, True, train=False),
    "nonorm_fp16_grad": _block_case((24, 16, 3), dict(norm_layer=None, activation_layer=_leaky), 24, HF, True),
    "nonorm_fp16_nograd": _block_case((24, 16, 3), dict(norm_layer=None, activation_layer=_leaky), 24, HF, False),
    "nonorm_fp32_input_fp16_autocast_grad": _block_case((24, 16, 3), dict(norm_layer=None, activation_layer=_leaky), 24, HF, True,
                                                        xdtype=F32),
    "nonorm_fp32_input_fp16_autocast_nograd": _block_case((24, 16, 3), dict(norm_layer=None, activation_layer=_leaky), 24, HF,
                                                          False, xdtype=F32),
    "nonorm_noact_fp16_grad": _block_case((24, 16, 3), dict(norm_layer=None, activation_layer=None), 24, HF, True),
    "nonorm_fp32_grad": _block_case((24, 16, 3), dict(norm_layer=None, activation_layer=_leaky), 24, F32, True),
    "conv1to32_k7_leaky_grad": _block_case((1, 32, 7), dict(padding=0, activation_layer=_leaky), 1, HF, True),
    "conv1to32_k7_leaky_nograd": _block_case((1, 32, 7), dict(padding=0, activation_layer=_leaky), 1, HF, False),
    "groups2_grad": _block_case((64, 64, 3), dict(groups=2), 64, BF, True),
    "groups2_nograd": _block_case((64, 64, 3), dict(groups=2), 64, BF, False),
    "one_value_per_channel": _block_case((64, 64, 3), dict(padding=0), 64, BF, False, shape=(1, 3, 3)),
    "conv2d_fp32_grad": _conv2d_case((24, 64, 3), dict(stride=2, padding=1), 24, F32, True),
    "conv2d_fp32_nograd": _conv2d_case((24, 64, 3), dict(stride=2, padding=1), 24, F32, False),
    "conv2d_bf16_grad": _conv2d_case((24, 64, 3), dict(stride=2, padding=1), 24, BF, True),
    "conv2d_bf16_nograd": _conv2d_case((24, 64, 3), dict(stride=2, padding=1), 24, BF, False),
    "conv2d_groups2_grad": _conv2d_case((64, 64, 3), dict(padding=1, groups=2), 64, BF, True),
    "conv2d_groups2_nograd": _conv2d_case((64, 64, 3), dict(padding=1, groups=2), 64, BF, False),
    # grad mode on, nothing requires a gradient (a frozen layer outside no_grad)
    "conv2d_bf16_frozen_grad_mode": _conv2d_case((24, 64, 3), dict(stride=2, padding=1), 24, BF, False, frozen=True),
    "nonorm_fp16_frozen_grad_mode": _block_case((24, 16, 3), dict(norm_layer=None, activation_layer=None), 24, HF, False,
                                                frozen=True),
    "pw64to24_bf16_frozen_grad_mode": _block_case((64, 24, 1), {}, 64, BF, False, frozen=True),
    "conv2d_reflect": _conv2d_case((24, 64, 3), dict(padding=1, padding_mode='reflect'), 24, BF, False),
    "class_logits_bf16_grad": _logits_case(BF, True),
    "class_logits_bf16_nograd": _logits_case(BF, False),
    "class_logits_fp32_grad": _logits_case(F32, True),
    "class_logits_fp32_nograd": _logits_case(F32, False),
    "bottleneck_eval_bf16": _bottleneck_case(BF, False, False),
    "bottleneck_train_bf16": _bottleneck_case(BF, True, True),
    "bottleneck_train_fp32": _bottleneck_case(F32, True, True),
    "patch_statistics_train": _patch_statistics_case(True),
    "patch_statistics_eval": _patch_statistics_case(False),
    "aspp_nograd": _aspp_case(False),
    "aspp_grad": _aspp_case(True),
    "aspp_grad_cat": _aspp_case(True, consts=(("_ASPP_NOCAT_GRAD", False),)),
})

# cases that raise: (exception type, a substring of the message that says which error it is)
RAISES = {
    "dense3x3_drop_raises": ("RuntimeError", "on the fused BatchNorm(train) pass only"),
    "one_value_per_channel": ("ValueError", "Expected more than 1 value per channel"),
    # the block's in-place activation on the (view) output of the convolution's autograd Function: torch refuses it
    "nonorm_fp16_grad": ("RuntimeError", "is a view and is being modified inplace"),
    "nonorm_fp32_input_fp16_autocast_grad": ("RuntimeError", "is a view and is being modified inplace"),
    "nonorm_fp32_grad": ("RuntimeError", "is a view and is being modified inplace"),
}
# cases that are ATen's from end to end: conv.Conv2d hands padding_mode != 'zeros' to nn.Conv2d.forward, which pads and calls
# the library convolution without a mfma.note_library record.  Their bits are the library's choice of algorithm.
ATEN_ONLY = {"conv2d_reflect": "nn.Conv2d.forward behind padding_mode='reflect': a library convolution that is not recorded"}


def _sha(t):
    return hashlib.sha256(t.detach().cpu().clone(memory_format=torch.contiguous_format).flatten().view(torch.uint8).numpy().tobytes()).hexdigest()


def record(name, dev, tracer, deterministic):
    """One run of case `name` from freshly built modules; `tracer` is installed around _lib.call by the caller.
    -> dict(trace, library[, raises][, hashes])."""
    from refign_amd import determinism, mfma
    patch = Patch()
    saved = dict(mfma.LIBRARY_CALLS)
    mfma.LIBRARY_CALLS.clear()
    out = {}
    try:
        torch.manual_seed(20240)
        spec = CASES[name](dev, patch)
        xs = spec["x"] if isinstance(spec["x"], list) else [spec["x"]]
        if spec["grad"]:
            xs = [t.requires_grad_(True) for t in xs]
        tracer.trace = []
        ac = torch.autocast("cuda", dtype=spec["autocast"]) if spec["autocast"] is not None else contextlib.nullcontext()
        with determinism.deterministic(deterministic), torch.set_grad_enabled(spec["grad_mode"]):
            y = None
            try:
                with ac:
                    y = spec["call"](xs if isinstance(spec["x"], list) else xs[0])
                if spec["grad"]:
                    g = torch.randn(y.shape).to(dev).to(y.dtype)
                    tracer.trace.append(["backward", []])
                    y.backward(g)
            except (RuntimeError, ValueError) as e:
                want = RAISES.get(name, (None, None))[1]
                out["raises"] = [type(e).__name__, want if want is not None and want in str(e) else str(e)]
        torch.cuda.synchronize(dev)
        if deterministic and "raises" not in out:
            hashes = {"out": _sha(y), "out_meta": [str(y.dtype), list(y.shape), list(y.stride())]}
            if spec["grad"]:
                for i, t in enumerate(xs):
                    hashes[f"grad_x{i}"] = _sha(t.grad)
                for j, mod in enumerate(spec["mods"]):
                    for k, p_ in mod.named_parameters():
                        hashes[f"grad_{j}.{k}"] = None if p_.grad is None else _sha(p_.grad)
            out["hashes"] = hashes
        out["trace"] = tracer.trace
        out["library"] = sorted([k[0], k[1], [list(s) for s in k[2]], n] for k, n in mfma.LIBRARY_CALLS.items())
    finally:
        tracer.trace = []
        patch.undo()
        mfma.LIBRARY_CALLS.clear()
        mfma.LIBRARY_CALLS.update(saved)
    return out


def record_case(name, dev, tracer):
    """The fixture entry of one case: default-mode run, two deterministic runs."""
    plain = record(name, dev, tracer, False)
    det = [record(name, dev, tracer, True) for _ in range(2)]
    if det[0]["trace"] != det[1]["trace"] or det[0]["library"] != det[1]["library"]:
        raise SystemExit(f"{name}: two runs launched different kernels")
    entry = {"trace": plain["trace"], "library": plain["library"], "det_trace": det[0]["trace"], "det_library": det[0]["library"]}
    if "raises" in plain or "raises" in det[0]:
        if plain.get("raises") != det[0].get("raises"):
            raise SystemExit(f"{name}: raises in one mode only")
        entry["raises"] = plain["raises"]
    else:
        entry["hashes"] = det[0]["hashes"]
        if det[0]["hashes"] != det[1]["hashes"]:
            if not det[0]["library"]:
                raise SystemExit(f"{name}: two deterministic runs differ and no library call is in the trace")
            entry["unstable"] = True
    if ("raises" in entry) != (name in RAISES) or ("raises" in entry and entry["raises"] != list(RAISES[name])):
        raise SystemExit(f"{name}: raises {entry.get('raises')}, RAISES says {RAISES.get(name)}")
    if name in ATEN_ONLY:
        if entry["trace"] or entry["library"] or entry["det_trace"] or entry["det_library"] or "raises" in entry:
            raise SystemExit(f"{name}: listed in ATEN_ONLY but launched or recorded something")
        entry["aten_only"] = ATEN_ONLY[name]
        entry["hashes"] = {"out_meta": entry["hashes"]["out_meta"]}
        entry.pop("unstable", None)
    return entry


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(HERE, "conv_routes.json"))
    ap.add_argument("--only", default=None, help="comma-separated cases: record these and merge them into --out")
    a = ap.parse_args()
    from refign_amd import _lib
    dev = torch.device("cuda:0")
    names = list(CASES) if a.only is None else a.only.split(",")
    cases = {}
    if a.only is not None:
        with open(a.out) as f:
            cases = json.load(f)["cases"]
    patch = Patch()
    tracer = Tracer(_lib.call)
    patch.setattr(_lib, "call", tracer)
    try:
        for name in names:
            cases[name] = record_case(name, dev, tracer)
    finally:
        patch.undo()
    # cases that launch the same thing as another one are kept on purpose; say so (an empty trace says nothing)
    by_route = {}
    for name, e in cases.items():
        e.pop("note", None)
        if e["trace"] or e["library"]:
            by_route.setdefault(json.dumps([e["trace"], e["library"], e["det_trace"], e["det_library"]]), []).append(name)
    for same in by_route.values():
        for n in same if len(same) > 1 else ():
            cases[n]["note"] = "same launches as " + ", ".join(m for m in same if m != n)
    with open(a.out, "w") as f:                              # one case per line
        rows = [f' {json.dumps(n)}: {json.dumps(cases[n], sort_keys=True)}' for n in sorted(cases)]
        f.write('{"cases": {\n' + ",\n".join(rows) + "\n}}\n")
    unstable = [n for n, e in cases.items() if e.get("unstable")]
    print(f"wrote {a.out}: {len(cases)} cases ({len(names)} recorded now), {len(unstable)} unstable {unstable}")


if __name__ == "__main__":
    main()
