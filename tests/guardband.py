"""Guard-band arena for the kernel tests (a plain helper module like bn_standin.py; tests/test_guardband_cpu.py is its self-test).

Every other test hands its kernels fresh tensors: freshly mapped device memory reads as zero and the neighbours of an operand are
other small finite tensors.  In a training run the caching allocator hands out blocks that held the inf / NaN of an overflowed
fp16 step.  `GuardArena` reproduces that in a test: ONE uint8 allocation filled with a poison byte, operands copied into it
(`place`), and -- inside `allocations()` -- every `torch.empty` / `empty_like` / `empty_strided` (and `zeros` / `zeros_like` / `full`,
which are then filled with their value) of the arena's device carved out of it as well.  So everything a wrapper reads beyond an
operand's logical extent, and everything it leaves unwritten in an output or a temporary, is poison; `check()` then proves that
nothing was written outside the ranges handed out.

Fills: 0x00 (what a fresh process sees), 0xFF (NaN in fp64 / fp32 / fp16 / bf16 / e4m3, 255 as u8, -1 as an integer) and 0x7B
(large and finite: 1.3058e36 fp32, 1.3033e36 bf16, 61280 fp16 -- fmaxf / fminf and comparisons swallow a NaN, a running maximum
fed with garbage does not propagate one).
"""
import contextlib

import torch

FILLS = (0x00, 0xFF, 0x7B)
GUARD = 64 << 10          # bytes of untouched fill on each side of everything handed out
ALIGN = 256

_EMPTY = torch.empty      # the real one: the arena's own bookkeeping must not go through its patch
_PATCHED = ("empty", "empty_like", "empty_strided", "zeros", "zeros_like", "full")


class GuardViolation(AssertionError):
    pass


class GuardArena:
    def __init__(self, device, fill, nbytes, skew=0):
        self.device = torch.device(device)
        if self.device.type == "cuda" and self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        self.fill = int(fill)
        self.skew = int(skew)                 # default skew of place()
        self.nbytes = int(nbytes)
        assert 0 <= self.fill <= 255 and self.nbytes > 2 * GUARD + ALIGN
        self.buf = torch.full((self.nbytes,), self.fill, dtype=torch.uint8, device=self.device)
        self.ranges = []                      # (first byte, one past the last byte, label) in address order
        self._cursor = 0
        self._base_misalign = self.buf.data_ptr() % ALIGN
        self.high_water = 0

    # ---- bump allocator ---------------------------------------------------------------------------------------------
    def _carve(self, shape, strides, dtype, skew, label):
        """A tensor of its own (own version counter: autograd saves such tensors) over the arena's storage."""
        item = _EMPTY((), dtype=dtype).element_size()
        assert skew % item == 0 and 0 <= skew < ALIGN, "skew must be a multiple of the element size"
        assert all(s >= 0 for s in strides), "negative strides are not placed"
        span = 0 if any(n == 0 for n in shape) else (1 + sum((n - 1) * s for n, s in zip(shape, strides))) * item
        start = self._cursor + GUARD
        # ALIGN-byte boundary of the ADDRESS (the arena's own base is at least that aligned on every allocator met so far)
        start += (-(start + self._base_misalign)) % ALIGN
        start += skew
        end = start + span
        if end + GUARD > self.nbytes:
            raise RuntimeError(f"guard arena of {self.nbytes} bytes exhausted by {label} ({span} bytes at {start})")
        self._cursor = end
        self.high_water = end + GUARD
        self.ranges.append((start, end, label))
        t = _EMPTY(0, dtype=dtype, device=self.device)
        t.set_(self.buf.untyped_storage(), (self.buf.storage_offset() + start) // item, tuple(shape), tuple(strides))
        return t

    def place(self, t, skew=None):
        """Copy of `t` in the arena: same shape, strides, dtype and values; starts `skew` bytes past a 256-byte boundary."""
        skew = self.skew if skew is None else skew
        p = self._carve(tuple(t.shape), tuple(t.stride()), t.dtype, skew, f"place{tuple(t.shape)}")
        with torch.no_grad():
            p.copy_(t.detach())
        return p

    # ---- the patched allocators -------------------------------------------------------------------------------------
    def _mine(self, dev):
        if dev is None:
            return self.device.type == "cpu"
        dev = torch.device(dev)
        if dev.type != self.device.type:
            return False
        return dev.index is None or self.device.index is None or dev.index == self.device.index

    def _make(self, name, orig, like):
        def patched(*args, **kw):
            try:
                if kw.get("pin_memory") or kw.get("names") is not None or kw.get("out") is not None or \
                        kw.get("layout", torch.strided) is not torch.strided:
                    return orig(*args, **kw)
                dev = kw.get("device", args[0].device if like else None)
                if not self._mine(dev):
                    return orig(*args, **kw)
                # the real function on the meta device tells shape, strides and dtype without this module parsing arguments
                meta = orig(*args, **{k: v for k, v in kw.items() if k not in ("device", "requires_grad", "pin_memory")},
                            device="meta")
            except Exception:
                return orig(*args, **kw)
            t = self._carve(tuple(meta.shape), tuple(meta.stride()), meta.dtype, 0, f"{name}{tuple(meta.shape)}")
            if name in ("zeros", "zeros_like"):
                t.zero_()
            elif name == "full":
                t.fill_(args[1] if len(args) > 1 else kw["fill_value"])
            if kw.get("requires_grad"):
                t.requires_grad_(True)
            return t
        patched.__name__ = name
        return patched

    @contextlib.contextmanager
    def allocations(self):
        """Inside: torch.empty & co. for the arena's device come out of the arena, poisoned, guarded and recorded."""
        saved = {n: getattr(torch, n) for n in _PATCHED}
        try:
            for n, orig in saved.items():
                setattr(torch, n, self._make(n, orig, n.endswith("_like")))
            yield self
        finally:
            for n, orig in saved.items():
                setattr(torch, n, orig)

    # ---- the check --------------------------------------------------------------------------------------------------
    def gaps(self):
        """Byte ranges never handed out, in order (the first and the last are at least GUARD long)."""
        out, at = [], 0
        for a, b, _ in self.ranges:
            out.append((at, a))
            at = b
        out.append((at, self.nbytes))
        return out

    def violations(self):
        """[(first byte, one past the last modified byte, label of the allocation before, label of the one after)]"""
        gaps = self.gaps()
        bad = torch.stack([(self.buf[a:b] != self.fill).any() for a, b in gaps]).cpu().tolist()
        labels = ["<arena start>"] + [r[2] for r in self.ranges] + ["<arena end>"]
        out = []
        for i, ((a, b), hit) in enumerate(zip(gaps, bad)):
            if hit:
                idx = (self.buf[a:b] != self.fill).nonzero().flatten()
                out.append((a + int(idx[0]), a + int(idx[-1]) + 1, labels[i], labels[i + 1]))
        return out

    def check(self):
        if self.device.type == "cuda":
            torch.cuda.synchronize(self.device)
        v = self.violations()
        if v:
            a, b, before, after = v[0]
            prev_end = max([r[1] for r in self.ranges if r[1] <= a], default=0)
            raise GuardViolation(
                f"fill 0x{self.fill:02X}: bytes [{a}, {b}) of the arena were written outside every allocation: between "
                f"{before} (ends at {prev_end}, {a - prev_end} bytes before) and {after}; {len(v)} gap(s) touched")
