"""SparseEPE.update as one kernel (csrc/sparseepe.hip through refign_amd/sparse_epe.py): against the values the reference's own
class produced (tests/golden/metric_sparse_epe.npz) at the tolerance tests/test_metrics_cpu.py holds the host metric to, and
against metrics.SparseEPE.update -- which that golden pins to the reference -- on the same device tensors at the 1e-6 of
tests/test_fit_gpu.py, on the cases where the two could part: ties at the thresholds, one valid point, none, the capacity, integer
and non-integer quantile ranks."""
import numpy as np
import pytest
import torch
from conftest import golden

pytestmark = pytest.mark.gpu
KEYS = ("AEPE", "PCK_1", "PCK_3", "PCK_5", "PCK_10", "AUSE_AEPE")


def fused_metric(flow, ps, pt, unc, uncertainty=True):
    from refign_amd.metrics import SparseEPE
    from refign_amd.sparse_epe import sparse_epe_rows
    m = SparseEPE(uncertainty_estimation=uncertainty)
    rows = sparse_epe_rows(flow, ps, pt, unc)
    assert rows.dtype == torch.float64 and tuple(rows.shape) == (flow.shape[0], 8)
    m.add_rows(rows)
    return m, rows


def host_metric(flow, ps, pt, unc, uncertainty=True):
    from refign_amd.metrics import SparseEPE
    m = SparseEPE(uncertainty_estimation=uncertainty)
    m.update(flow, ps, pt, tuple(flow.shape[-2:]), unc)
    return m


def test_kernel_matches_the_reference(dev):
    z = golden("metric_sparse_epe")
    flow, unc = torch.from_numpy(z["flow"]).to(dev), torch.from_numpy(z["unc"]).to(dev)
    ps, pt = [torch.from_numpy(p).to(dev) for p in z["pts_s"]], [torch.from_numpy(p).to(dev) for p in z["pts_t"]]
    m, rows = fused_metric(flow, ps, pt, unc)
    assert int(m.nbr_valid_corr) == int(z["nbr_valid_corr"]) and int(m.nbr_samples) == 2
    assert int(z["nbr_valid_corr"]) < 2 * 400                         # (some points are outside the image)
    out = m.compute()
    for k in KEYS:
        print(k, float(out[k]), float(z[k]))
        assert abs(float(out[k]) - float(z[k])) <= 1e-5 * max(abs(float(z[k])), 1e-3), k
    m2, rows2 = fused_metric(flow[:1], ps[:1], pt[:1], None, uncertainty=False)      # without a confidence, the first sample
    out2 = m2.compute()
    assert "AUSE_AEPE" not in out2 and float(rows2[0, 5]) == 0.0
    for k in ("AEPE", "PCK_1", "PCK_10"):
        assert abs(float(out2[k]) - float(z[k + "_first"])) <= 1e-5 * max(abs(float(z[k + "_first"])), 1e-3), k
    assert torch.equal(rows2[0, [0, 1, 2, 3, 4, 6, 7]], rows[0, [0, 1, 2, 3, 4, 6, 7]])


def _case(dev, ns, H=48, W=64, seed=0, levels=None, valid=None):
    """B = len(ns) samples of ns[b] correspondences on an H x W flow; levels: the confidence quantised to that many values;
    valid[b]: how many points of sample b lie inside the image (the others far outside), None = a margin decides"""
    g = torch.Generator().manual_seed(seed)
    B = len(ns)
    flow = (torch.rand(B, 2, H, W, generator=g) - 0.5) * 10
    unc = torch.rand(B, 1, H, W, generator=g)
    if levels:
        unc = torch.floor(unc * levels) / levels
    ps, pt = [], []
    for b, n in enumerate(ns):
        t = torch.stack([torch.rand(n, generator=g) * (W + 6) - 3, torch.rand(n, generator=g) * (H + 6) - 3], 1)
        if valid is not None:
            t = torch.stack([torch.rand(n, generator=g) * (W - 1), torch.rand(n, generator=g) * (H - 1)], 1)
            t[valid[b]:] += 1000.0
        ix, iy = t[:, 0].round().clamp(0, W - 1).long(), t[:, 1].round().clamp(0, H - 1).long()
        err = (torch.rand(n, 2, generator=g) - 0.5) * 16 * (0.2 + unc[b, 0, iy, ix])[:, None]
        s = t + flow[b][:, iy, ix].T + err
        if valid is not None:
            s[:valid[b]] = s[:valid[b]].clamp(min=0.0).minimum(torch.tensor([W - 1.0, H - 1.0]))
        ps.append(s.to(dev))
        pt.append(t.to(dev))
    return flow.to(dev), ps, pt, unc.to(dev)


def _compare(dev, case, samples=None):
    flow, ps, pt, unc = case
    want = host_metric(flow, ps, pt, unc)
    got, rows = fused_metric(flow, ps, pt, unc)
    assert int(got.nbr_valid_corr) == int(want.nbr_valid_corr) and int(got.nbr_samples) == int(want.nbr_samples)
    if samples is not None:
        assert int(got.nbr_samples) == samples
    a, b = got.compute(), want.compute()
    for k in KEYS:
        print(k, float(a[k]), float(b[k]))
        assert abs(float(a[k]) - float(b[k])) <= 1e-6 * max(1.0, abs(float(b[k]))), k
    return rows


@pytest.mark.parametrize("n", [51, 300, 8192], ids=lambda n: f"n{n}")
def test_kernel_matches_the_host_metric(dev, n):
    """n = 51: q * (n - 1) is an integer for every q = t / 50 (up to fp32 rounding); 300: it is not; 8192: the capacity"""
    _compare(dev, _case(dev, [n, n], seed=n, valid=[n, n]))
    _compare(dev, _case(dev, [n], seed=n + 1))                        # a margin: some points outside the image


def test_ties_at_the_thresholds(dev):
    """a confidence of 4 levels: every threshold falls on a run of equal keys, which `>=` keeps whole"""
    rows = _compare(dev, _case(dev, [400, 257], seed=3, levels=4))
    assert float(rows[:, 5].min()) > 0.0


def test_one_valid_point_and_none(dev):
    rows = _compare(dev, _case(dev, [40, 40, 40], seed=5, valid=[1, 0, 40]), samples=2)
    assert int(rows[0, 6]) == 1 and float(rows[0, 7]) == 1.0 and float(rows[0, 5]) < 1e-6      # one point: both curves are one value
    assert not rows[1].any()                                          # no valid point: a zero row, the sample is not counted
    assert int(rows[2, 6]) == 40
    flow, ps, pt, unc = _case(dev, [0, 7], seed=6, valid=[0, 7])      # an EMPTY point list
    rows = _compare(dev, (flow, ps, pt, unc), samples=1)
    assert not rows[0].any()


def test_capacity_and_fallback(dev):
    """n = 8193 is past the kernel's capacity: the library refuses, and evaltail.eval_step returns False so that the model's own
    step runs"""
    from refign_amd import evaltail, sparse_epe
    from refign_amd.alignment_model import AlignmentModel
    from refign_amd.metrics import IoU, MyMetricCollection, SparseEPE
    flow, ps, pt, unc = _case(dev, [8193], seed=7)
    with pytest.raises(RuntimeError, match="n <= 8192"):
        sparse_epe.sparse_epe_rows(flow, ps, pt, unc)

    class Model(AlignmentModel):                                      # eval_step must decide BEFORE it runs the forward
        def __init__(self):
            torch.nn.Module.__init__(self)

        def forward(self, a, b):
            self.calls = getattr(self, "calls", 0) + 1
            return flow[:, :, :a.shape[-2], :a.shape[-1]], unc[:, :, :a.shape[-2], :a.shape[-1]]

    model = Model()
    img = torch.zeros(1, 3, *flow.shape[-2:], device=dev)
    metrics = MyMetricCollection({"val_MegaDepth_SparseEPE": SparseEPE(uncertainty_estimation=True)})
    batch = {"image": img, "image_ref": img, "corr_pts": pt, "corr_pts_ref": ps}
    assert evaltail.eval_step(model, metrics, batch, "MegaDepth") is False and not hasattr(model, "calls")
    ok = {**batch, "corr_pts": [pt[0][:8192]], "corr_pts_ref": [ps[0][:8192]]}
    assert evaltail.eval_step(model, metrics, ok, "MegaDepth") is True and model.calls == 1
    want = host_metric(flow, ok["corr_pts_ref"], ok["corr_pts"], unc).compute()
    got = metrics["val_MegaDepth_SparseEPE"].compute()
    for k in KEYS:
        assert abs(float(got[k]) - float(want[k])) <= 1e-6 * max(1.0, abs(float(want[k]))), k
    # the other conditions: points on the host, fp64 points, a metric of another class, no metric of this data set
    assert evaltail.eval_step(model, metrics, {**ok, "corr_pts": [ok["corr_pts"][0].cpu()]}, "MegaDepth") is False
    assert evaltail.eval_step(model, metrics, {**ok, "corr_pts": [ok["corr_pts"][0].double()]}, "MegaDepth") is False
    assert evaltail.eval_step(model, metrics, ok, "RobotCarMatching") is False

    class Sub(SparseEPE):
        pass

    assert evaltail.eval_step(model, MyMetricCollection({"val_MegaDepth_SparseEPE": Sub()}), ok, "MegaDepth") is False
    assert evaltail.eval_step(model, MyMetricCollection({"val_MegaDepth_IoU": IoU(3)}), ok, "MegaDepth") is False
    assert model.calls == 1


def test_deterministic_mode_and_equal_bits(dev):
    """no floating-point atomics: the kernel runs while the library's deterministic flag is set, and two runs give equal bits"""
    from refign_amd import determinism
    from refign_amd.sparse_epe import sparse_epe_rows
    flow, ps, pt, unc = _case(dev, [700, 333], seed=9, levels=8)
    plain = sparse_epe_rows(flow, ps, pt, unc)
    with determinism.deterministic():
        assert determinism.enabled()
        a = sparse_epe_rows(flow, ps, pt, unc)                        # (RFN_ENONDET would raise here)
        b = sparse_epe_rows(flow, ps, pt, unc)
    for t in (a, b):
        assert torch.equal(t.view(torch.int64), plain.view(torch.int64))
    with pytest.raises(RuntimeError, match="no CPU path"):
        sparse_epe_rows(flow.cpu(), ps, pt, unc)
