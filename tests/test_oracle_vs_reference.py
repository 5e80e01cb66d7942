"""Re-check of the oracle against the REFERENCE's own outputs on fresh seeded inputs (tests/golden/recheck.pt, written by
oracle/make_golden.py golden_recheck from the reference itself).  The other fixtures under tests/golden/ were produced by
the same comparison; this test repeats a slice of it on other inputs so that an edit of the oracle cannot drift away from
the reference unnoticed between fixture regenerations."""
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "oracle"))


def _recheck():
    from conftest import GOLDEN
    return torch.load(os.path.join(GOLDEN, "recheck.pt"), weights_only=True)


def _fusion_sd():
    from conftest import load_golden
    return load_golden("fusion_full.pt")["sd"]


def test_fusion_eval_forward_fresh_input():
    from ffsr_oracle import fusion
    from make_golden import recheck_inputs
    (lr, imgs, feats, _), _, _ = recheck_inputs()
    want = _recheck()["sr"]
    with torch.no_grad():
        got = fusion.fusion_forward(_fusion_sd(), lr, imgs, feats)
    assert (got - want).abs().max().item() < 2e-5


def test_fusion_train_forward_and_gradients_fresh_input():
    import torch.nn.functional as F
    from ffsr_oracle import fusion
    from make_golden import recheck_grad_index, recheck_inputs
    _, (lr, imgs, feats, hr), _ = recheck_inputs()
    want = _recheck()["grads"]
    sd = _fusion_sd()
    names = want["names"]
    sdo = {k: (v.clone().requires_grad_(True) if k in names else v.clone()) for k, v in sd.items()}
    F.l1_loss(fusion.fusion_forward(sdo, lr, imgs, feats, train=True).clamp(0, 1), hr).backward()
    assert len(names) > 0
    off = 0
    for k, gmax, gsum, gl2 in zip(names, want["max"].tolist(), want["sum"].tolist(), want["l2"].tolist()):
        # the fixture keeps max|g|, the sum and L2 norm of the whole gradient and its values at fixed positions (all of
        # them for small parameters).  An error of at most tol per element moves the sum by at most tol * n and the
        # L2 norm by at most tol * sqrt(n), so those two bounds follow from the per-element one.
        got = sdo[k].grad
        n = got.numel()
        idx = recheck_grad_index(n)
        g = want["values"][off:off + len(idx)]
        off += len(idx)
        tol = 2e-3 * gmax + 1e-12
        err = (got.reshape(-1)[idx] - g).abs().max().item()
        assert err <= tol, (k, err)
        assert abs(got.abs().max().item() - gmax) <= tol, (k, "max|grad|")
        assert abs(got.double().sum().item() - gsum) <= tol * n, (k, "sum")
        assert abs(got.double().norm().item() - gl2) <= tol * n ** 0.5, (k, "L2")
    assert off == want["values"].numel()


def test_metrics_fresh_pair():
    from ffsr_oracle import metrics as om
    from make_golden import recheck_inputs
    _, _, (a, b) = recheck_inputs()
    want = _recheck()["metrics"]
    for crop, y in ((0, False), (4, True)):
        psnr, ssim = want[(crop, y)]
        assert abs(om.psnr(a, b, crop, y) - psnr) < 1e-4
        assert abs(om.ssim(a, b, crop, y) - ssim) < 1e-6
