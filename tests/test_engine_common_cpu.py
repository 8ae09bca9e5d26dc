"""What the feature engines share (wise_amd/feature/_engine.py), as far as it runs without the library or a device: the
weight blobs' size check and the workspace's growth rule."""
import pytest
import torch

from wise_amd.feature._engine import device_blobs, fit_workspace


def test_blob_check_names_all_four_counts_when_either_is_off_by_one():
    wb, pf = torch.zeros(1201, dtype=torch.bfloat16), torch.zeros(77)
    dwb, dpf = device_blobs((1201, 77), (wb, pf), "cpu", "wise_some_layout")
    assert torch.equal(dwb, wb) and torch.equal(dpf, pf) and dwb.dtype == torch.bfloat16
    for nb, nf in ((1200, 77), (1202, 77), (1201, 76), (1201, 78)):
        with pytest.raises(RuntimeError, match="blob size mismatch") as e:
            device_blobs((nb, nf), (wb, pf), "cpu", "wise_some_layout")
        text = str(e.value)
        assert "packed 1201/77" in text and f"expects {nb}/{nf}" in text and "wise_some_layout" in text


def test_workspace_grows_only_past_what_is_held():
    grown = []
    hook = lambda: grown.append(1)
    bad = ValueError("shape unsupported")
    ws = fit_workspace(None, 100, "cpu", bad, hook)
    assert ws.numel() == 100 and ws.dtype == torch.uint8 and len(grown) == 1
    for n in (100, 1, 99):                                               # fits: the same object, no hook
        assert fit_workspace(ws, n, "cpu", bad, hook) is ws
    assert len(grown) == 1
    big = fit_workspace(ws, 101, "cpu", bad, hook)
    assert big is not ws and big.numel() == 101 and len(grown) == 2
    assert fit_workspace(big, 100, "cpu", bad, hook) is big and len(grown) == 2      # never shrinks
    assert fit_workspace(big, 500, "cpu", bad).numel() == 500            # the hook is optional


def test_zero_bytes_is_the_callers_error():
    grown = []
    ws = torch.empty(64, dtype=torch.uint8)
    for held in (None, ws):
        with pytest.raises(ValueError, match="Cnn14: batch 1 x 5 samples unsupported"):
            fit_workspace(held, 0, "cpu", ValueError("Cnn14: batch 1 x 5 samples unsupported"), lambda: grown.append(1))
        with pytest.raises(RuntimeError, match="bad config"):
            fit_workspace(held, 0, "cpu", RuntimeError("wise_vit_workspace_bytes: bad config"))
    assert not grown
