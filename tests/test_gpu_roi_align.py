"""GPU parity, RoI Align: rpn_roi_align bit for bit against the float32 restatement of tests/test_roi_align_host.py, its backward
against the float64 scatter restatement, the known answers on the device, the model-level entry against the float32 operator on
the copied-out tap, and autograd.

Tile edges of the kernels as written (tf_rpn_amd/csrc/roi_kernels.hip):
  forward   a wave covers 256 channels per pass (kRoiChannelTile): C = 252 (63 lanes), 256 (exactly one pass), 260 (one lane in a second);
            a workgroup covers 16 bins (i, j) of one RoI, a wave 4 of them (kRoiSampleTile, kRoiSamplesPerWave): ph x pw = 4 x 4
            (exactly one workgroup), 3 x 5 (the last wave has 3), 1 x 17 (one bin in a second workgroup);
            a bin's sample columns are kept in four unrolled slots (kRoiAlignMaxSamples): s = 1 .. 4 each take another guard path
  backward  the same channel tile; RoIs are tested 64 at a time: R = 64 (one batch), 65 (one RoI in a second); bin rows / columns
            are weighted 64 at a time, one bin per lane with its s samples in a loop: ph x pw = 65 x 66 (s = 1), and the issue's
            17 x 33 at s = 4 (68 x 132 samples)
"""
import numpy as np
import pytest
import torch

import test_roi_align_host as ah
import test_roi_host as rh
from oracle import bbox_oracle as bo
from tf_rpn_amd.models._rpn_model import synthetic_weights
from tf_rpn_amd.models.detection_head import DetectionHead
from tf_rpn_amd.predictor import Proposer
from tf_rpn_amd.utils import roi_utils

pytestmark = pytest.mark.gpu

# (B, H, W, C, R, ph, pw, s)
ISSUE_FORWARD = [(1, 2, 2, 4, 1, 1, 1, 1), (2, 5, 9, 20, 3, 2, 3, 3), (2, 7, 7, 16, 5, 7, 7, 2), (1, 31, 31, 512, 9, 7, 7, 2),
                 (2, 6, 6, 8, 4, 14, 14, 1), (1, 1, 1, 4, 2, 2, 2, 2), (1, 1, 5, 8, 3, 1, 3, 4)]
TILE_EDGES = [(1, 3, 4, 252, 2, 3, 5, 2), (1, 3, 4, 256, 2, 4, 4, 3), (1, 4, 3, 260, 2, 1, 17, 4)]       # channel and bin-tile edges
FORWARD_CASES = ISSUE_FORWARD + TILE_EDGES
BACKWARD_CASES = ([c for c in ISSUE_FORWARD if c[3] != 512] + [(1, 31, 31, 64, 300, 7, 7, 2)] + TILE_EDGES
                  + [(1, 5, 5, 8, 64, 2, 2, 2), (2, 5, 5, 8, 65, 2, 2, 2), (1, 3, 3, 4, 2, 17, 33, 4), (1, 3, 3, 4, 2, 65, 66, 1)])
INSIDE_KINDS = [0, 1, 2, 8, 5]          # clipped to [0, 1]: interior, full image, touching 1.0, touching 0.0, zero area
U = 2.0 ** -24


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _valid_for(B, R):
    """valid smaller than R, including 0 (for the second image when there is one)."""
    return np.array([max(R - 2, 0)] + [0] * (B - 1), dtype=np.int32) if B > 1 or R > 2 else np.array([0], dtype=np.int32)


def _ids(c):
    return "x".join(map(str, c))


@pytest.mark.parametrize("case", FORWARD_CASES, ids=_ids)
def test_forward_bit_exact_against_float32_restatement(case):
    B, H, W, C, R, ph, pw, s = case
    rng = np.random.RandomState(sum(case))
    x = rng.standard_normal((B, H, W, C)).astype(np.float32)
    # every kind of rh.BOX_KINDS over the cases: box (b, r) is kind (first + b R + r) mod 9; the 9-RoI case holds all nine
    rois = rh.nasty_boxes(rng, B, R, first=FORWARD_CASES.index(case))
    for valid in (None, _valid_for(B, R)):
        got = roi_utils.roi_align(x, rois, (ph, pw), sampling_ratio=s, valid=valid)
        ref = ah.roi_align_ref(x, rois, ph, pw, s, valid=valid)
        assert got.dtype == np.float32 and got.shape == (B, R, ph, pw, C)
        assert np.array_equal(_bits(got), _bits(ref)), "max |diff| %g" % np.nanmax(np.abs(got - ref))


@pytest.mark.parametrize("s", [1, 2, 3, 4])
def test_forward_all_box_kinds_and_stride_exact_extent_bit_exact(s):
    """The workload's 31 x 31 map under extent (31.25, 31.25) (500 / 16: the box [0, 1] reaches a quarter pixel past the last
    pixel centre's cell) and under the default, 4 x every kind of box, at every sampling ratio."""
    rng = np.random.RandomState(40 + s)
    x = rng.standard_normal((1, 31, 31, 8)).astype(np.float32)
    rois = rh.nasty_boxes(rng, 1, 36)
    for extent in ((31.25, 31.25), None, (31.0, 40.5)):
        got = roi_utils.roi_align(x, rois, (7, 7), sampling_ratio=s, extent=extent)
        assert np.array_equal(_bits(got), _bits(ah.roi_align_ref(x, rois, 7, 7, s, extent=extent)))


@pytest.mark.parametrize("case", FORWARD_CASES, ids=_ids)
def test_forward_against_float64(case):
    """|out - out64| <= f32_vs_f64_bound * max|x| on interior boxes and on boxes clipped to [0, 1] (the bound:
    tests/test_roi_align_host.py)."""
    B, H, W, C, R, ph, pw, s = case
    rng = np.random.RandomState(100 + sum(case))
    x = rng.standard_normal((B, H, W, C)).astype(np.float32)
    for rois in (rh.interior_boxes(rng, B, R), np.clip(rh.nasty_boxes(rng, B, R, kinds=INSIDE_KINDS), 0, 1)):
        got = roi_utils.roi_align(torch.from_numpy(x), torch.from_numpy(rois), (ph, pw), sampling_ratio=s).cpu().numpy()
        err = np.abs(got - ah.roi_align_ref(x, rois, ph, pw, s, dtype=np.float64)).max()
        print("forward vs float64:", case, err, np.abs(x).max())
        assert err <= ah.f32_vs_f64_bound(H, W) * np.abs(x).max()


@pytest.mark.parametrize("n", [4, 7, 31, 32])
def test_identity_known_answer_on_the_device(n):
    """Box [0,0,1,1], ph = pw = H = W, s = 1: every sample is a pixel centre, the output is x[0] bit for bit."""
    rng = np.random.RandomState(n)
    x = rng.standard_normal((1, n, n, 4)).astype(np.float32)
    out = roi_utils.roi_align(x, np.array([[[0, 0, 1, 1]]], np.float32), (n, n), sampling_ratio=1)
    assert np.array_equal(_bits(out[0, 0]), _bits(x[0]))


@pytest.mark.parametrize("s", [1, 2, 3, 4])
def test_affine_known_answer_on_the_device(s):
    """An affine map's RoI Align is its value at the bin centre (case and bound: tests/test_roi_align_host.py)."""
    x, rois, want, ab = ah.affine_case()
    err = np.abs(roi_utils.roi_align(x, rois, (7, 5), sampling_ratio=s) - want).max()
    print("affine known answer on the device: s", s, "err", err, "bound", ah.affine_bound(x, ab, s))
    assert err <= ah.affine_bound(x, ab, s)


def _backward_excess(dx, dy, rois, shape, s, valid, coord_dtype, extent=None):
    """-> (|dx - dx64| - c S per element of dx, S32), the bound of test_backward_against_float64_scatter.  S and N: the unit-weight
    scatter of |dy| and of ones (the number of terms), over the pixels the bins touch with float32 coordinates (the kernel's: S32)
    and with `coord_dtype` coordinates, the larger of the two -- a sample within COORD_EPS of a pixel centre reads another pixel
    pair in the two precisions, with a weight below COORD_EPS on the pixel the other does not read."""
    def unit(values, cd, sh):
        return ah.roi_align_backward_ref(values, rois, sh, s, extent=extent, valid=valid, coord_dtype=cd, unit_weights=True)

    ones, shape1 = np.ones_like(dy[..., :1]), tuple(shape[:3]) + (1,)
    S32, N = unit(np.abs(dy), np.float32, shape), unit(ones, np.float32, shape1)
    S = S32
    if coord_dtype != np.float32:
        S, N = np.maximum(S, unit(np.abs(dy), coord_dtype, shape)), np.maximum(N, unit(ones, coord_dtype, shape1))
    ref = ah.roi_align_backward_ref(dy, rois, shape, s, extent=extent, valid=valid, coord_dtype=coord_dtype)
    print("backward:", tuple(shape), "s", s, np.dtype(coord_dtype).name, "max |diff|", np.abs(dx - ref).max(), "max S", S.max(), "max N", N.max())
    return np.abs(dx - ref) - (2 * ah.coord_eps(shape[1], shape[2]) + (N + 8) * U) * S, S32


@pytest.mark.parametrize("case", BACKWARD_CASES, ids=_ids)
def test_backward_against_float64_scatter(case):
    """|dx - dx64| <= c S, S = the float64 scatter of |dy| with every non-zero axis weight 1, c = 2 COORD_EPS + (N + 8) u
    (u = 2^-24; twice the COORD_EPS on maps of 33 to 64): a term's weight is (Ay / s)(Ax / s), two averages of fractions of
    coordinates that are off by <= COORD_EPS each, so it is off by <= 2 COORD_EPS (+ COORD_EPS^2); the kernel's own arithmetic
    rounds each weight sum, product and the division (8 u covers them) and sums the N terms of a pixel sequentially in float32,
    (N - 1) u of the sum of their magnitudes, which S bounds.  Against the float64 restatement with float64 coordinates on boxes
    clipped to [0, 1] (no sample near an ok threshold), and on all nine kinds against the scatter that takes its coordinates in
    float32, as the kernel does.  Also: two runs give the same bits; pixels no sample touches are exactly 0."""
    B, H, W, C, R, ph, pw, s = case
    rng = np.random.RandomState(200 + sum(case))
    dy = rng.standard_normal((B, R, ph, pw, C)).astype(np.float32)
    shape = (B, H, W, C)
    for coord_dtype in (np.float64, np.float32):
        rois = rh.nasty_boxes(rng, B, R, first=BACKWARD_CASES.index(case), kinds=INSIDE_KINDS if coord_dtype == np.float64 else None)
        if coord_dtype == np.float64:
            rois = np.clip(rois, 0, 1)
        for valid in (None, _valid_for(B, R)):
            dx = roi_utils.roi_align_backward(dy, rois, shape, sampling_ratio=s, valid=valid)
            again = roi_utils.roi_align_backward(dy, rois, shape, sampling_ratio=s, valid=valid)
            assert dx.shape == shape and np.array_equal(_bits(dx), _bits(again))
            excess, S32 = _backward_excess(dx, dy, rois, shape, s, valid, coord_dtype)
            assert excess.max() <= 0, (excess.max(), np.unravel_index(excess.argmax(), excess.shape))
            assert not dx[S32 == 0].any()                                 # pixels no sample touches: written as zeros


@pytest.mark.parametrize("case", BACKWARD_CASES, ids=_ids)
def test_backward_is_the_adjoint_of_the_forward(case):
    """<roi_align(x), dy> = <x, backward(dy)> to 1e-5 relative, both sides summed in float64 (positive data: no cancellation)."""
    B, H, W, C, R, ph, pw, s = case
    rng = np.random.RandomState(300 + sum(case))
    x = rng.uniform(0.5, 1.5, size=(B, H, W, C)).astype(np.float32)
    dy = rng.uniform(0.5, 1.5, size=(B, R, ph, pw, C)).astype(np.float32)
    rois = rh.nasty_boxes(rng, B, R, first=BACKWARD_CASES.index(case))
    valid = _valid_for(B, R) if B > 1 else None
    out = roi_utils.roi_align(x, rois, (ph, pw), sampling_ratio=s, valid=valid)
    dx = roi_utils.roi_align_backward(dy, rois, (B, H, W, C), sampling_ratio=s, valid=valid)
    lhs, rhs = (out.astype(np.float64) * dy).sum(), (x.astype(np.float64) * dx).sum()
    print("adjoint:", case, lhs, rhs)
    assert abs(lhs - rhs) <= 1e-5 * abs(lhs)


def test_backward_extent_reaches_the_kernel():
    """The adjoint identity under a non-default extent (a backward that ignored it would pair with another forward)."""
    rng = np.random.RandomState(9)
    x = rng.uniform(0.5, 1.5, size=(1, 31, 31, 8)).astype(np.float32)
    dy = rng.uniform(0.5, 1.5, size=(1, 20, 7, 7, 8)).astype(np.float32)
    rois = rh.interior_boxes(rng, 1, 20)
    out = roi_utils.roi_align(x, rois, (7, 7), extent=(31.25, 29.0))
    dx = roi_utils.roi_align_backward(dy, rois, x.shape, extent=(31.25, 29.0))
    assert not np.array_equal(dx, roi_utils.roi_align_backward(dy, rois, x.shape))
    assert _backward_excess(dx, dy, rois, x.shape, 2, None, np.float32, extent=(31.25, 29.0))[0].max() <= 0
    lhs, rhs = (out.astype(np.float64) * dy).sum(), (x.astype(np.float64) * dx).sum()
    assert abs(lhs - rhs) <= 1e-5 * abs(lhs)


def test_backward_of_one_image_ignores_the_other_images_rois():
    rng = np.random.RandomState(7)
    B, H, W, C, R, ph, pw = 2, 7, 7, 16, 70, 3, 3
    dy = torch.from_numpy(rng.standard_normal((B, R, ph, pw, C)).astype(np.float32)).cuda()
    rois = torch.from_numpy(rh.nasty_boxes(rng, B, R)).cuda()
    valid = torch.tensor([R, R], dtype=torch.int32, device="cuda")
    dx = roi_utils.roi_align_backward(dy, rois, (B, H, W, C), valid=valid)
    rois2, valid2 = rois.clone(), valid.clone()
    rois2[1] = torch.from_numpy(rh.interior_boxes(rng, 1, R)[0]).cuda()
    valid2[1] = 3
    dx2 = roi_utils.roi_align_backward(dy, rois2, (B, H, W, C), valid=valid2)
    assert torch.equal(dx[0], dx2[0]) and not torch.equal(dx[1], dx2[1])
    alone = roi_utils.roi_align_backward(dy[:1], rois[:1], (1, H, W, C), valid=valid[:1])      # ... nor on the batch it is part of
    assert torch.equal(alone[0], dx[0])


def test_autograd_calls_the_backward_kernel():
    rng = np.random.RandomState(8)
    x = torch.from_numpy(rng.standard_normal((2, 5, 9, 20)).astype(np.float32)).cuda().requires_grad_()
    rois = torch.from_numpy(rh.nasty_boxes(rng, 2, 9)).cuda()
    valid = torch.tensor([9, 4], dtype=torch.int32, device="cuda")
    kw = dict(sampling_ratio=3, extent=(5.5, 9.25), valid=valid)
    out = roi_utils.roi_align(x, rois, (2, 3), **kw)
    assert out.requires_grad and torch.equal(out.detach(), roi_utils.roi_align(x.detach(), rois, (2, 3), **kw))
    out.sum().backward()
    direct = roi_utils.roi_align_backward(torch.ones_like(out), rois, x.shape, **kw)
    assert x.grad is not None and torch.equal(x.grad, direct) and x.grad.abs().sum() > 0
    # a head written in torch trains through it: a weighted loss gives the weighted adjoint
    w = torch.from_numpy(rng.standard_normal(tuple(out.shape)).astype(np.float32)).cuda()
    x.grad = None
    (roi_utils.roi_align(x, rois, (2, 3), **kw) * w).sum().backward()
    assert torch.equal(x.grad, roi_utils.roi_align_backward(w, rois, x.shape, **kw))


def test_detection_head_trains_through_roi_align():
    rng = np.random.RandomState(12)
    feat = torch.from_numpy(rng.standard_normal((2, 6, 6, 8)).astype(np.float32)).cuda().requires_grad_()
    rois = torch.from_numpy(rh.interior_boxes(rng, 2, 5)).cuda()
    valid = torch.tensor([5, 3], dtype=torch.int32, device="cuda")
    head = DetectionHead(3, pooling_size=(3, 3), channels=8, hidden=(16, 16), max_rois=10, seed=4)
    pooled = roi_utils.roi_align(feat, rois, (3, 3), valid=valid)
    pooled.retain_grad()
    logits, deltas = head(pooled)
    (logits.square().sum() + deltas.sum()).backward()
    assert feat.grad is not None and tuple(feat.grad.shape) == tuple(feat.shape) and float(feat.grad.abs().sum()) > 0
    assert torch.equal(feat.grad, roi_utils.roi_align_backward(pooled.grad, rois, tuple(feat.shape), valid=valid))


_WEIGHTS = {}


def _proposer(backbone, precision):
    hp = dict(bo.get_hyper_params(backbone, img_size=96, feature_map_shape=6))
    if backbone not in _WEIGHTS:
        _WEIGHTS[backbone] = synthetic_weights(backbone, hp, seed=2)
    return Proposer(backbone, hyper_params=hp, weights=_WEIGHTS[backbone], precision=precision, max_batch=2, iou_threshold=0.7)


@pytest.mark.parametrize("precision", ["f32", "f16x3", "bf16x3"])
@pytest.mark.parametrize("backbone", ["vgg16", "mobilenet_v2"])
def test_model_level_align_equals_align_of_the_copied_tap(backbone, precision):
    """FeatureExtractor.roi_align (straight from the arena: the split form under f16x3 / bf16x3) == roi_align of get_activation of
    the tap, bit for bit, at B = 1 and B = 2; propose_features(pooling="align") returns propose's boxes and the align of those
    boxes; the default arguments still run crop_and_resize."""
    prop = _proposer(backbone, precision)
    fe = prop.feature_extractor
    rng = np.random.RandomState(11)
    imgs = torch.from_numpy(rng.uniform(0, 1, size=(2, 96, 96, 3)).astype(np.float32)).cuda()
    with pytest.raises(ValueError):
        fe.roi_align(torch.zeros((1, 1, 4), device="cuda"))               # no forward has run on this handle
    for B in (1, 2):
        prop.forward(imgs[:B])
        rois = torch.from_numpy(rh.nasty_boxes(rng, B, 9)).cuda()
        valid = torch.tensor([8, 0][:B], dtype=torch.int32, device="cuda")
        tap = fe.output()[:B]
        assert tap.shape[1:3] == (6, 6) and tap.abs().max() > 0
        for v, s, extent in ((None, 2, None), (valid, 3, (6.0, 6.0)), (valid, 1, (6.25, 5.5))):
            got = fe.roi_align(rois, (7, 7), sampling_ratio=s, extent=extent, valid=v)
            assert got.shape == (B, 9, 7, 7, tap.shape[3])
            want = roi_utils.roi_align(tap, rois, (7, 7), sampling_ratio=s, extent=extent, valid=v)
            assert torch.equal(got.view(torch.int32), want.view(torch.int32))
        if precision == "f32":       # ... and the float32 tap against the restatement, end to end
            ref = ah.roi_align_ref(tap.cpu().numpy(), rois.cpu().numpy(), 7, 7, 1, extent=(6.25, 5.5), valid=valid.cpu().numpy())
            assert np.array_equal(_bits(got.cpu().numpy()), _bits(ref))
        boxes, scores, nvalid, pooled = [t.clone() for t in prop.propose_features(imgs[:B], (3, 2), pooling="align")]
        b2, s2, v2, _idx = prop.propose(imgs[:B])
        assert torch.equal(boxes, b2) and torch.equal(scores, s2) and torch.equal(nvalid, v2) and int(nvalid.min()) > 0
        want = roi_utils.roi_align(fe.output()[:B], b2, (3, 2), valid=v2)
        assert pooled.shape == want.shape and torch.equal(pooled.view(torch.int32), want.view(torch.int32))
        assert pooled.abs().sum() > 0
        for b in range(B):
            assert not pooled[b, int(nvalid[b]):].any()
        # the defaults are pooling="crop": the same bits as naming it, and as roi_pooling of the tap
        default = [t.clone() for t in prop.propose_features(imgs[:B], (3, 2))]
        named = prop.propose_features(imgs[:B], (3, 2), pooling="crop", sampling_ratio=4, extent=(3.0, 3.0))
        assert all(torch.equal(a.view(torch.int32), c.view(torch.int32)) for a, c in zip(default, named))
        crop = roi_utils.roi_pooling(fe.output()[:B], b2, (3, 2), valid=v2)
        assert torch.equal(default[3].view(torch.int32), crop.view(torch.int32)) and not torch.equal(default[3], pooled)
    with pytest.raises(ValueError):
        fe.roi_align(torch.zeros((3, 1, 4), device="cuda"))               # beyond max_batch
    with pytest.raises(ValueError):
        prop.propose_features(imgs, pooling="max")
    with pytest.raises(ValueError):
        fe.roi_align(rois, (7, 7), sampling_ratio=0)


def test_detect_default_is_crop_and_align_is_selectable():
    prop = _proposer("vgg16", "f32")
    C = prop.feature_extractor.output_shape[3]
    head = DetectionHead(5, pooling_size=(3, 3), channels=C, hidden=(16, 16), max_rois=2 * prop.topn, trainable=False, seed=2)
    imgs = torch.from_numpy(np.random.RandomState(0).uniform(0, 1, size=(2, 96, 96, 3)).astype(np.float32)).cuda()
    kw = dict(score_threshold=0.01, max_total_size=50)
    default = [t.clone() for t in prop.detect(imgs, head, **kw)]
    crop = [t.clone() for t in prop.detect(imgs, head, pooling="crop", **kw)]
    assert all(torch.equal(a, b) for a, b in zip(default, crop))
    rois, _s, valid, pooled = prop.propose_features(imgs, pooling_size=(3, 3), pooling="align", sampling_ratio=2)
    want = [t.clone() for t in head.detect(rois, pooled, prop.hyper_params["variances"], valid=valid, **kw)]
    got = prop.detect(imgs, head, pooling="align", sampling_ratio=2, **kw)
    assert all(torch.equal(a, b) for a, b in zip(got, want))
    with pytest.raises(ValueError):
        prop.detect(imgs, head, pooling="max")
