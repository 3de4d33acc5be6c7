#!/usr/bin/env python3
"""tools/kvpath_bench.py [views] -- the key / value path of a MiT-B5 attention block at the EMA teacher's shapes (40 views per stage):
the fused launch (csrc/kvpath.hip) against today's launches (patchify, spatial-reduction GEMM, LayerNorm, kv GEMM, pack).
Run it under `rocprofv3 --kernel-trace` and hand the trace to `--parse`: times are taken from the trace, not from HIP events around
eager launches (profiles/r05_student_gemm_shapes.txt).

  tools/kvpath_bench.py --parse KERNEL_TRACE.csv    per stage: median time of the fused launch and of each launch of the chain

The run issues, per stage, WARM + REPS chains and then WARM + REPS fused launches; the parser cuts the trace at the fused kernels
(their names carry the stage's C and r) and drops each segment's first WARM repetitions."""
import csv
import os
import statistics
import sys

STAGES = [(135, 240, 64, 8), (68, 120, 128, 4), (34, 60, 320, 2), (17, 30, 512, 1)]      # H, W, C, r
WARM, REPS = 3, 20


def parse(path):
    rows = []
    with open(path) as f:
        for r in csv.DictReader(f):
            rows.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]) - int(r["Start_Timestamp"]), r["Kernel_Name"]))
    rows.sort()
    fused, order = {}, []                                       # fused kernels in order of first appearance = stage order
    for _, dur, name in rows:
        if "kvpath_kernel" in name:
            if name not in fused:
                order.append(name)
            fused.setdefault(name, []).append(dur)
    seg, chains = 0, [[] for _ in order]
    for _, dur, name in rows:
        if "kvpath_kernel" in name:
            seg = order.index(name) + 1
        elif seg < len(order):
            chains[seg].append((name, dur))
    for s, name in enumerate(order):
        H, W, C, r = STAGES[s]
        f_us = statistics.median(fused[name][WARM:]) / 1e3
        ch = [c for c in chains[s] if any(k in c[0] for k in ("patchify", "gemm_nt", "layernorm_fwd", "attn_pack"))]
        per = len(ch) // (WARM + REPS)
        ch = ch[WARM * per:]
        parts = []
        for i in range(per):
            parts.append((ch[i][0].split("(")[0][-70:], statistics.median(c[1] for c in ch[i::per]) / 1e3))
        total = sum(p[1] for p in parts)
        map_mb = 40 * H * W * C * 2 / 1e6
        print(f"stage {s + 1} ({H}x{W}, C {C}, r {r}; map {map_mb:6.1f} MB = {map_mb / 5e3 * 1e3:5.1f} us at 5 TB/s): fused {f_us:7.1f} us | "
              f"chain {total:7.1f} us in {per} launches")
        for n, t in parts:
            print(f"      {t:7.1f} us  {n}")


if len(sys.argv) > 2 and sys.argv[1] == "--parse":
    parse(sys.argv[2])
    sys.exit(0)

import torch  # noqa: E402

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from refign_amd import mfma  # noqa: E402
from refign_amd.conv import patch_conv_tokens  # noqa: E402
from refign_amd.seg import Attention  # noqa: E402

dev = torch.device("cuda:0")
views = int(sys.argv[1]) if len(sys.argv) > 1 else 40
for stage, (H, W, C, r) in enumerate(STAGES, 1):
    torch.manual_seed(stage)
    m = Attention(C, num_heads=C // 64, qkv_bias=True, sr_ratio=r).to(dev).eval()
    x = torch.randn(views, H * W, C, device=dev).to(torch.bfloat16)
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
        for _ in range(WARM + REPS):
            n = m.norm(patch_conv_tokens(x, H, W, m.sr)) if r > 1 else x
            kv = m.kv(n)
            Nkv = kv.shape[1]
            mfma._pack(kv, kv.stride(0), kv.stride(1), views, 2 * (C // 64), Nkv, mfma._nkblk(Nkv))
        torch.cuda.synchronize()
        for _ in range(WARM + REPS):
            out = mfma.kv_packs(x, H, W, m.sr if r > 1 else None, m.norm if r > 1 else None, m.kv)
        assert out is not None
        torch.cuda.synchronize()
    print(f"stage {stage}: {views} x {H}x{W}, C {C}, r {r}: {WARM + REPS} chains, {WARM + REPS} fused launches", flush=True)
