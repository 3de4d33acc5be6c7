"""SparseEPE.update in one launch (csrc/sparseepe.hip, rfn_sparse_epe_f32): from the matcher's full-resolution flow, its
confidence and the batch's sparse correspondences to one row of eight numbers per sample -- mean EPE, the four PCK counts, the
AUSE of the confidence, the number of valid correspondences, and whether the sample counts -- with no host synchronisation:
helpers/metrics.py:68-201 reads `int(ok.sum())` back per sample and calls torch.quantile a hundred times.

The semantics are metrics.SparseEPE.update's (the host-driven mirror of the reference, which stays: it is the fallback and the
operand this kernel is tested against); metrics.SparseEPE.add_rows takes the rows.  `MAX_POINTS` correspondences per sample."""
import ctypes

import torch

from . import _lib
from ._tensor import ptr

MAX_POINTS = 8192
MAX_BATCH = 64
ROW = ("AEPE", "PCK_1", "PCK_3", "PCK_5", "PCK_10", "AUSE_AEPE", "nbr_valid_corr", "nbr_samples")


def points_ok(pts, batch, device):
    """a batch's correspondences as the kernel takes them: a list of `batch` (n, 2) fp32 tensors on `device`, n <= MAX_POINTS"""
    return isinstance(pts, (list, tuple)) and len(pts) == batch and all(
        torch.is_tensor(p) and p.device == device and p.dtype == torch.float32 and p.dim() == 2 and p.shape[1] == 2 and
        p.shape[0] <= MAX_POINTS for p in pts)


def sparse_epe_rows(flow, corr_pts_s, corr_pts_t, uncertainty_est=None):
    """flow (B, 2, h, w) fp32, corr_pts_s / corr_pts_t: B x (n_b, 2) fp32 (x, y) in the source (reference) / target image,
    uncertainty_est (B, 1, h, w) fp32 or None -> rows (B, 8) fp64 on the device, columns ROW.  Nothing here waits for the
    device: the per-sample offsets come from the tensors' shapes."""
    if not (torch.is_tensor(flow) and flow.is_cuda and flow.dtype == torch.float32 and flow.dim() == 4 and flow.shape[1] == 2):
        raise RuntimeError("sparse_epe_rows: flow must be a (B, 2, h, w) float32 HIP (cuda:N) tensor: refign_amd has no CPU path")
    B, _, h, w = flow.shape
    dev = flow.device
    if B > MAX_BATCH:
        raise RuntimeError(f"sparse_epe_rows: {B} samples in a batch, the kernel takes {MAX_BATCH}")
    if not (points_ok(corr_pts_s, B, dev) and points_ok(corr_pts_t, B, dev)) or \
            any(s.shape[0] != t.shape[0] for s, t in zip(corr_pts_s, corr_pts_t)):
        raise RuntimeError(f"sparse_epe_rows: the points must be {B} pairs of (n, 2) float32 tensors on {dev}, n <= {MAX_POINTS}")
    conf = uncertainty_est
    if conf is not None:
        if not (conf.dtype == torch.float32 and tuple(conf.shape) == (B, 1, h, w) and conf.device == dev):
            raise RuntimeError(f"sparse_epe_rows: uncertainty_est ({B}, 1, {h}, {w}) float32 on {dev} expected")
        conf = conf.contiguous()
    flow = flow.contiguous()
    offsets = [0]
    for p in corr_pts_t:
        offsets.append(offsets[-1] + int(p.shape[0]))
    ps = (torch.cat(list(corr_pts_s)) if B > 1 else corr_pts_s[0]).contiguous()
    pt = (torch.cat(list(corr_pts_t)) if B > 1 else corr_pts_t[0]).contiguous()
    if offsets[-1] == 0:                                   # no point at all: nothing to read, every row is zero
        return torch.zeros((B, 8), dtype=torch.float64, device=dev)
    rows = torch.empty((B, 8), dtype=torch.float64, device=dev)
    _lib.call("rfn_sparse_epe_f32", dev, ptr(flow), ptr(conf), ptr(ps), ptr(pt), (ctypes.c_int * (B + 1))(*offsets), B, h, w,
              ptr(rows))
    return rows
