"""The matcher's `test:` section end to end on the device: decoded uint8 arrays and points -> resample.EvalIngest (Lanczos resize,
normalise, pad) -> Trainer.test -> AlignmentModel.forward -> one sparse-EPE kernel -> {"test_MegaDepth_SparseEPE_AEPE": ...},
against the same call with RFN_EVAL_FUSED=0 (the model's own test_step: metrics.SparseEPE.update on the host)."""
import pytest
import torch
from make_golden_matcher_ingest import IMAGE, IMAGE_REF, SIZE, image_in, points_in

pytestmark = pytest.mark.gpu


def test_matcher_test_section_runs_fused(dev, monkeypatch):
    from refign_amd.metrics import MyMetricCollection, SparseEPE
    from refign_amd.resample import EvalIngest
    from refign_amd.trainer import Trainer
    from test_matcher_gpu import build_matcher
    batch = EvalIngest(resize=SIZE, interpolation="lanczos", pad="same", device=dev)(
        image_in(*IMAGE, "image"), image_ref=image_in(*IMAGE_REF, "image_ref"), corr_pts=points_in(*IMAGE, "image"),
        corr_pts_ref=points_in(*IMAGE_REF, "image_ref"))
    assert tuple(batch["image"].shape) == tuple(batch["image_ref"].shape) == (1, 3, 128, 160)
    model = build_matcher(dev)
    model.test_metrics = MyMetricCollection({"test_MegaDepth_SparseEPE": SparseEPE(uncertainty_estimation=True)})
    calls = [0]
    inner = SparseEPE.update

    def counted(self, *a, **k):
        calls[0] += 1
        return inner(self, *a, **k)

    monkeypatch.setattr(SparseEPE, "update", counted)
    monkeypatch.setattr(SparseEPE, "__call__", counted)                # (the class binds __call__ to update's function)
    tr = Trainer(model)
    monkeypatch.delenv("RFN_EVAL_FUSED", raising=False)
    fused = tr.test({"MegaDepth": [batch]})
    assert calls[0] == 0                                               # the fused path ran: the host metric was never fed
    monkeypatch.setenv("RFN_EVAL_FUSED", "0")
    host = tr.test({"MegaDepth": [batch]})
    assert calls[0] >= 1
    tr.close()
    assert set(fused) == set(host) == {"test_MegaDepth_SparseEPE_" + k for k in ("AEPE", "PCK_1", "PCK_3", "PCK_5", "PCK_10", "AUSE_AEPE")}
    for k, v in host.items():
        print(k, fused[k], v)
        assert isinstance(fused[k], float) and abs(fused[k] - v) <= 1e-6 * max(1.0, abs(v)), k
    assert fused["test_MegaDepth_SparseEPE_AEPE"] > 0.0
