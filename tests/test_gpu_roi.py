"""GPU parity, RoI pooling: rpn_roi_pool bit for bit against the float32 restatement of tests/test_roi_host.py, its backward
against the float64 scatter restatement, the model-level pool against the float32 pool of the copied-out tap, and autograd.

Tile edges of the kernels as written (tf_rpn_amd/csrc/roi_kernels.hip):
  forward   a wave covers 256 channels per pass (kRoiChannelTile): C = 252 (63 lanes), 256 (exactly one pass), 260 (one lane in a second);
            a workgroup covers 16 samples (i, j) of one RoI, a wave 4 of them (kRoiSampleTile, kRoiSamplesPerWave): ph x pw = 4 x 4
            (exactly one workgroup), 3 x 5 (the last wave has 3), 1 x 17 (one sample in a second workgroup; also the ph == 1 formula)
  backward  the same channel tile; RoIs are tested 64 at a time: R = 64 (one batch), 65 (one RoI in a second); sample rows / columns
            are weighted 64 at a time: ph x pw = 65 x 66
"""
import numpy as np
import pytest
import torch

import test_roi_host as rh
from oracle import bbox_oracle as bo
from tf_rpn_amd.models._rpn_model import synthetic_weights
from tf_rpn_amd.predictor import Proposer
from tf_rpn_amd.utils import roi_utils

pytestmark = pytest.mark.gpu

# (B, H, W, C, R, ph, pw)
ISSUE_FORWARD = [(1, 2, 2, 4, 1, 1, 1), (2, 5, 9, 20, 3, 2, 3), (2, 7, 7, 16, 5, 7, 7), (1, 31, 31, 512, 9, 7, 7), (2, 6, 6, 8, 4, 14, 14)]
CHANNEL_EDGES = [(1, 3, 4, 252, 2, 3, 5), (1, 3, 4, 256, 2, 4, 4), (1, 4, 3, 260, 2, 1, 17)]      # + the three sample-tile edges
FORWARD_CASES = ISSUE_FORWARD + CHANNEL_EDGES
BACKWARD_CASES = ([c for c in ISSUE_FORWARD if c[3] != 512] + [(1, 31, 31, 64, 300, 7, 7)] + CHANNEL_EDGES
                  + [(1, 5, 5, 8, 64, 2, 2), (2, 5, 5, 8, 65, 2, 2), (1, 3, 3, 4, 2, 65, 66)])
# kinds of rh.BOX_KINDS whose samples fall on the same side of the border in float32 and float64 coordinates: everything but the
# boxes that TOUCH 0.0 / 1.0 (there the last sample can round just past H - 1 in float32, include/rpn_hip.h)
STABLE_KINDS = [0, 4, 5, 6, 7, 0, 0]   # interior (three times as often), wholly outside, zero area, flipped, NaN


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _valid_for(B, R):
    """valid smaller than R, including 0 (for the second image when there is one)."""
    return np.array([max(R - 2, 0)] + [0] * (B - 1), dtype=np.int32) if B > 1 or R > 2 else np.array([0], dtype=np.int32)


@pytest.mark.parametrize("case", FORWARD_CASES, ids=lambda c: "x".join(map(str, c)))
def test_forward_bit_exact_against_float32_restatement(case):
    B, H, W, C, R, ph, pw = case
    rng = np.random.RandomState(sum(case))
    x = rng.standard_normal((B, H, W, C)).astype(np.float32)
    # every kind of rh.BOX_KINDS over the cases: box (b, r) is kind (first + b R + r) mod 9; the 9-RoI case holds all nine
    rois = rh.nasty_boxes(rng, B, R, first=FORWARD_CASES.index(case))
    for valid in (None, _valid_for(B, R)):
        got = roi_utils.roi_pooling(x, rois, (ph, pw), valid=valid)
        ref = rh.roi_pool_ref(x, rois, ph, pw, valid=valid)
        assert got.dtype == np.float32 and got.shape == (B, R, ph, pw, C)
        assert np.array_equal(_bits(got), _bits(ref)), "max |diff| %g" % np.nanmax(np.abs(got - ref))


def test_forward_edge_touching_boxes_bit_exact():
    """Boxes clipped to exactly 0.0 / 1.0 (what clip_boxes produces) on the workload's 31 x 31 map: the last sample of some rounds
    just above H - 1 in float32 and is 0 (the contract); the kernel takes the same branch as the restatement on every sample."""
    rng = np.random.RandomState(5)
    x = rng.standard_normal((1, 31, 31, 8)).astype(np.float32)
    rois = rh.nasty_boxes(rng, 1, 80, kinds=[1, 2, 8])
    got = roi_utils.roi_pooling(x, rois, (7, 7))
    assert np.array_equal(_bits(got), _bits(rh.roi_pool_ref(x, rois, 7, 7)))


@pytest.mark.parametrize("case", FORWARD_CASES, ids=lambda c: "x".join(map(str, c)))
def test_forward_against_float64_on_interior_boxes(case):
    """|out - out64| <= 2e-5 max|x| on interior boxes, every sample taking part (the bound: tests/test_roi_host.py)."""
    B, H, W, C, R, ph, pw = case
    rng = np.random.RandomState(100 + sum(case))
    x = rng.standard_normal((B, H, W, C)).astype(np.float32)
    rois = rh.interior_boxes(rng, B, R)
    got = roi_utils.roi_pooling(torch.from_numpy(x), torch.from_numpy(rois), (ph, pw)).cpu().numpy()
    err = np.abs(got - rh.roi_pool_ref(x, rois, ph, pw, dtype=np.float64)).max()
    print("forward vs float64:", case, err, np.abs(x).max())
    assert err <= 2e-5 * np.abs(x).max()


@pytest.mark.parametrize("case", BACKWARD_CASES, ids=lambda c: "x".join(map(str, c)))
def test_backward_against_float64_scatter(case):
    """|dx - dx64| <= 3e-5 S, S = the float64 scatter of |dy| with all corner weights 1: a weight is off by <= 1.2e-5 per contribution
    (two fractions of a coordinate that is off by <= 5.7e-6), the float32 summation adds ~1e-7 per term.  Against the float64
    restatement on boxes whose samples are on the same side of the border in both precisions (STABLE_KINDS), and on every kind --
    the edge-touching boxes included -- against the scatter that takes its coordinates in float32, as the forward does.
    Also: two runs give the same bits."""
    B, H, W, C, R, ph, pw = case
    rng = np.random.RandomState(200 + sum(case))
    dy = rng.standard_normal((B, R, ph, pw, C)).astype(np.float32)
    for kinds, coord_dtype in ((STABLE_KINDS, np.float64), (None, np.float32)):
        rois = rh.nasty_boxes(rng, B, R, first=BACKWARD_CASES.index(case), kinds=kinds)
        for valid in (None, _valid_for(B, R)):
            dx = roi_utils.roi_pooling_backward(dy, rois, (B, H, W, C), valid=valid)
            again = roi_utils.roi_pooling_backward(dy, rois, (B, H, W, C), valid=valid)
            assert np.array_equal(_bits(dx), _bits(again))
            ref = rh.roi_pool_backward_ref(dy, rois, (B, H, W, C), valid=valid, coord_dtype=coord_dtype)
            S = rh.roi_pool_backward_ref(np.abs(dy), rois, (B, H, W, C), valid=valid, coord_dtype=coord_dtype, unit_weights=True)
            excess = np.abs(dx - ref) - 3e-5 * S
            print("backward:", case, np.dtype(coord_dtype).name, "max |diff|", np.abs(dx - ref).max(), "max S", S.max())
            assert excess.max() <= 0, (excess.max(), np.unravel_index(excess.argmax(), excess.shape))
            assert not dx[S == 0].any()                                   # pixels no sample touches: written as zeros


@pytest.mark.parametrize("case", BACKWARD_CASES, ids=lambda c: "x".join(map(str, c)))
def test_backward_is_the_adjoint_of_the_forward(case):
    """<roi_pool(x), dy> = <x, backward(dy)> to 1e-5 relative, both sides summed in float64 (positive data: no cancellation)."""
    B, H, W, C, R, ph, pw = case
    rng = np.random.RandomState(300 + sum(case))
    x = rng.uniform(0.5, 1.5, size=(B, H, W, C)).astype(np.float32)
    dy = rng.uniform(0.5, 1.5, size=(B, R, ph, pw, C)).astype(np.float32)
    rois = rh.nasty_boxes(rng, B, R, first=BACKWARD_CASES.index(case))
    valid = _valid_for(B, R) if B > 1 else None
    out = roi_utils.roi_pooling(x, rois, (ph, pw), valid=valid)
    dx = roi_utils.roi_pooling_backward(dy, rois, (B, H, W, C), valid=valid)
    lhs, rhs = (out.astype(np.float64) * dy).sum(), (x.astype(np.float64) * dx).sum()
    print("adjoint:", case, lhs, rhs)
    assert abs(lhs - rhs) <= 1e-5 * abs(lhs)


def test_backward_of_one_image_ignores_the_other_images_rois():
    rng = np.random.RandomState(7)
    B, H, W, C, R, ph, pw = 2, 7, 7, 16, 70, 3, 3
    dy = torch.from_numpy(rng.standard_normal((B, R, ph, pw, C)).astype(np.float32)).cuda()
    rois = torch.from_numpy(rh.nasty_boxes(rng, B, R)).cuda()
    valid = torch.tensor([R, R], dtype=torch.int32, device="cuda")
    dx = roi_utils.roi_pooling_backward(dy, rois, (B, H, W, C), valid=valid)
    rois2, valid2 = rois.clone(), valid.clone()
    rois2[1] = torch.from_numpy(rh.interior_boxes(rng, 1, R)[0]).cuda()
    valid2[1] = 3
    dx2 = roi_utils.roi_pooling_backward(dy, rois2, (B, H, W, C), valid=valid2)
    assert torch.equal(dx[0], dx2[0]) and not torch.equal(dx[1], dx2[1])
    alone = roi_utils.roi_pooling_backward(dy[:1], rois[:1], (1, H, W, C), valid=valid[:1])      # ... nor on the batch it is part of
    assert torch.equal(alone[0], dx[0])


def test_autograd_calls_the_backward_kernel():
    rng = np.random.RandomState(8)
    x = torch.from_numpy(rng.standard_normal((2, 5, 9, 20)).astype(np.float32)).cuda().requires_grad_()
    rois = torch.from_numpy(rh.nasty_boxes(rng, 2, 9)).cuda()
    valid = torch.tensor([9, 4], dtype=torch.int32, device="cuda")
    out = roi_utils.roi_pooling(x, rois, (2, 3), valid=valid)
    assert out.requires_grad and torch.equal(out.detach(), roi_utils.roi_pooling(x.detach(), rois, (2, 3), valid=valid))
    out.sum().backward()
    direct = roi_utils.roi_pooling_backward(torch.ones_like(out), rois, x.shape, valid=valid)
    assert x.grad is not None and torch.equal(x.grad, direct) and x.grad.abs().sum() > 0
    # a head written in torch trains through it: a weighted loss gives the weighted adjoint
    w = torch.from_numpy(rng.standard_normal(tuple(out.shape)).astype(np.float32)).cuda()
    x.grad = None
    (roi_utils.roi_pooling(x, rois, (2, 3), valid=valid) * w).sum().backward()
    assert torch.equal(x.grad, roi_utils.roi_pooling_backward(w, rois, x.shape, valid=valid))


_WEIGHTS = {}


def _proposer(backbone, precision):
    hp = dict(bo.get_hyper_params(backbone, img_size=96, feature_map_shape=6))
    if backbone not in _WEIGHTS:
        _WEIGHTS[backbone] = synthetic_weights(backbone, hp, seed=2)
    return Proposer(backbone, hyper_params=hp, weights=_WEIGHTS[backbone], precision=precision, max_batch=2, iou_threshold=0.7)


@pytest.mark.parametrize("precision", ["f32", "f16x3", "bf16x3"])
@pytest.mark.parametrize("backbone", ["vgg16", "mobilenet_v2"])
def test_model_level_pool_equals_pool_of_the_copied_tap(backbone, precision):
    """FeatureExtractor.roi_pool (straight from the arena: the split form under f16x3 / bf16x3) == roi_pooling of get_activation of
    the tap, bit for bit, at B = 1 and B = 2; propose_features returns propose's boxes and the pool of those boxes."""
    prop = _proposer(backbone, precision)
    fe = prop.feature_extractor
    rng = np.random.RandomState(11)
    imgs = torch.from_numpy(rng.uniform(0, 1, size=(2, 96, 96, 3)).astype(np.float32)).cuda()
    with pytest.raises(ValueError):
        fe.roi_pool(torch.zeros((1, 1, 4), device="cuda"))                # no forward has run on this handle
    for B in (1, 2):
        prop.forward(imgs[:B])
        rois = torch.from_numpy(rh.nasty_boxes(rng, B, 9)).cuda()
        valid = torch.tensor([8, 0][:B], dtype=torch.int32, device="cuda")
        tap = fe.output()[:B]
        assert tap.shape[1:3] == (6, 6) and tap.abs().max() > 0
        for v in (None, valid):
            got = fe.roi_pool(rois, (7, 7), valid=v)
            assert got.shape == (B, 9, 7, 7, tap.shape[3])
            assert torch.equal(got.view(torch.int32), roi_utils.roi_pooling(tap, rois, (7, 7), valid=v).view(torch.int32))
        if precision == "f32":       # ... and the float32 tap against the restatement, end to end
            assert np.array_equal(_bits(got.cpu().numpy()), _bits(rh.roi_pool_ref(tap.cpu().numpy(), rois.cpu().numpy(), 7, 7, valid=valid.cpu().numpy())))
        boxes, scores, nvalid, pooled = [t.clone() for t in prop.propose_features(imgs[:B], (3, 2))]
        b2, s2, v2, _idx = prop.propose(imgs[:B])
        assert torch.equal(boxes, b2) and torch.equal(scores, s2) and torch.equal(nvalid, v2) and int(nvalid.min()) > 0
        want = roi_utils.roi_pooling(fe.output()[:B], b2, (3, 2), valid=v2)
        assert pooled.shape == want.shape and torch.equal(pooled.view(torch.int32), want.view(torch.int32))
        assert pooled.abs().sum() > 0
        for b in range(B):
            assert not pooled[b, int(nvalid[b]):].any()
    with pytest.raises(ValueError):
        fe.roi_pool(torch.zeros((3, 1, 4), device="cuda"))                # beyond max_batch
