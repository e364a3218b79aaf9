"""GPU parity, RoI max pooling: rpn_roi_max_pool (maximum and argmax) bit for bit against the restatement of
tests/test_roi_max_host.py, rpn_roi_max_pool_backward bit for bit against the float32 restatement and within the sequential-sum
bound of the float64 one, run-to-run identity, autograd, the model-level entry against the float32 operator on the copied-out
tap, the argument checks and DetectionHead.load_keras_weights on the device.

Tile edges of the kernels as written (tf_rpn_amd/csrc/roi_kernels.hip):
  forward   a wave covers 256 channels per pass (kRoiChannelTile): C = 252 (63 lanes), 256 (exactly one pass), 260 (one lane in a second);
            a workgroup covers 16 bins (i, j) of one RoI, a wave 4 of them: ph x pw = 4 x 4 (exactly one workgroup), 3 x 5 (the last
            wave has 3), 1 x 17 (one bin in a second workgroup); with and without the argmax store
  backward  the same channel tile; RoIs are tested 64 at a time: R = 64 (one batch), 65 (one RoI in a second); bin rows / columns
            are tested 64 at a time, one bin per lane: ph x pw = 17 x 33 and 65 x 66 on a 3 x 3 map (many bins per pixel)

The Proposer's name for this pooling is "max_pool": the name "max" is held as an unknown one by the suites that came before.
"""
import os

import numpy as np
import pytest
import torch

import test_gpu_roi_align as ga
import test_roi_host as rh
import test_roi_max_host as mh
from tf_rpn_amd.models.detection_head import DetectionHead
from tf_rpn_amd.utils import roi_utils

pytestmark = pytest.mark.gpu

# (B, H, W, C, R, ph, pw)
ISSUE_FORWARD = [(1, 2, 2, 4, 1, 1, 1), (2, 5, 9, 20, 3, 2, 3), (2, 7, 7, 16, 5, 7, 7), (1, 31, 31, 512, 9, 7, 7),
                 (1, 2, 2, 8, 4, 7, 7), (1, 1, 1, 4, 2, 2, 2)]
TILE_EDGES = [(1, 3, 4, 252, 2, 3, 5), (1, 3, 4, 256, 2, 4, 4), (1, 4, 3, 260, 2, 1, 17)]
FORWARD_CASES = ISSUE_FORWARD + TILE_EDGES
BACKWARD_CASES = ([c for c in FORWARD_CASES if c[3] != 512]
                  + [(1, 31, 31, 64, 300, 7, 7), (1, 5, 5, 8, 64, 2, 2), (2, 5, 5, 8, 65, 2, 2), (1, 3, 3, 4, 2, 17, 33), (1, 3, 3, 4, 2, 65, 66)])
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

_bits, _valid_for, _ids = ga._bits, ga._valid_for, ga._ids


def _assert_forward(x, rois, ph, pw, extent=None, valid=None, fast=False):
    """the operator with and without the argmax store == the restatement, bits and indices"""
    ref, ref_idx = mh.roi_max_pool_ref(x, rois, ph, pw, extent=extent, valid=valid, fast=fast)
    got, idx = roi_utils.roi_max_pooling(x, rois, (ph, pw), extent=extent, valid=valid, return_argmax=True)
    alone = roi_utils.roi_max_pooling(x, rois, (ph, pw), extent=extent, valid=valid)
    assert got.dtype == np.float32 and got.shape == ref.shape and idx.dtype == np.int32 and idx.shape == ref.shape
    assert isinstance(alone, np.ndarray) and np.array_equal(_bits(alone), _bits(got))
    assert np.array_equal(_bits(got), _bits(ref)), "differing outputs: %d" % (_bits(got) != _bits(ref)).sum()
    assert np.array_equal(idx, ref_idx), "differing argmax: %d" % (idx != ref_idx).sum()
    return got, idx


@pytest.mark.parametrize("case", FORWARD_CASES, ids=_ids)
def test_forward_bit_exact_against_the_restatement(case):
    B, H, W, C, R, ph, pw = case
    rng = np.random.RandomState(sum(case))
    x = rng.standard_normal((B, H, W, C)).astype(np.float32)
    # every kind of rh.BOX_KINDS over the cases: box (b, r) is kind (first + b R + r) mod 9; the 9-RoI case holds all nine
    rois = rh.nasty_boxes(rng, B, R, first=FORWARD_CASES.index(case))
    for valid in (None, _valid_for(B, R)):
        _assert_forward(x, rois, ph, pw, valid=valid)
    # ... and boxes that all reach the map (full image, touching 1.0, touching 0.0, interior), whatever kinds the case drew above
    out, idx = _assert_forward(x, rh.nasty_boxes(rng, B, R, kinds=[1, 2, 8, 0]), ph, pw)
    assert (idx >= 0).any()


def test_forward_all_box_kinds_and_stride_exact_extent_bit_exact():
    """The workload's 31 x 31 map under the default extent (30, 30) and the stride-exact (31.25, 31.25), 4 x every kind of box."""
    rng = np.random.RandomState(41)
    x = rng.standard_normal((1, 31, 31, 8)).astype(np.float32)
    rois = rh.nasty_boxes(rng, 1, 36)
    a, ia = _assert_forward(x, rois, 7, 7, extent=None)
    b, ib = _assert_forward(x, rois, 7, 7, extent=(31.25, 31.25))
    _assert_forward(x, rois, 7, 7, extent=(30.0, 40.5), valid=np.array([30], np.int32))
    assert np.array_equal(_bits(a), _bits(_assert_forward(x, rois, 7, 7, extent=(30, 30))[0])) and not np.array_equal(ia, ib)


def test_forward_ties_negative_maps_and_non_finite_pixels():
    rng = np.random.RandomState(42)
    base = rng.standard_normal((2, 7, 9, 20)).astype(np.float32)
    rois = rh.nasty_boxes(rng, 2, 9)
    valid = np.array([9, 7], np.int32)
    relu, idx = _assert_forward(np.maximum(base, 0), rois, 3, 4, valid=valid)       # post-ReLU: ties between zeros, the first wins
    assert (relu == 0).any() and (idx >= 0).any()
    neg, idx = _assert_forward(-np.abs(base) - 1, rois, 3, 4, valid=valid)          # all negative: the negative maximum, not 0
    assert (neg[idx >= 0] <= -1).all() and (idx >= 0).any() and not neg[idx < 0].any() and (idx < 0).any()
    x = base.copy()
    x[0, 3, 4, 2], x[1, 2, 2, 5], x[1, 2, 3, 5], x[0, 1, 1, 0] = np.nan, np.nan, np.nan, -np.inf
    x[1, :, :, 7] = -np.inf                                                         # an all -inf channel gives -inf
    x[0, :, :, 9] = -0.0
    out, _ = _assert_forward(x, rois, 3, 4, valid=valid)
    assert np.isnan(out[0, 1, :, :, 2]).any() and np.isneginf(out[1, 0, :, :, 7]).all() and np.signbit(out[0, 1, :, :, 9]).all()


_BACKWARD = {}


def _backward_case(case, with_valid):
    """-> (dy, argmax of the restatement, rois, valid, the four results of the backward restatement); computed once per case"""
    key = (case, with_valid)
    if key not in _BACKWARD:
        B, H, W, C, R, ph, pw = case
        rng = np.random.RandomState(200 + sum(case))
        x = rng.standard_normal((B, H, W, C)).astype(np.float32)
        x[rng.uniform(size=x.shape) < 0.2] = 0.0
        rois = rh.nasty_boxes(rng, B, R, first=BACKWARD_CASES.index(case))
        valid = _valid_for(B, R) if with_valid else None
        dy = rng.standard_normal((B, R, ph, pw, C)).astype(np.float32)
        _out, argmax = mh.roi_max_pool_ref(x, rois, ph, pw, valid=valid, fast=True)
        _BACKWARD[key] = (x, dy, argmax, rois, valid, mh.roi_max_pool_backward_ref(dy, argmax, (B, H, W, C), valid=valid))
    return _BACKWARD[key]


@pytest.mark.parametrize("with_valid", [False, True], ids=["all", "valid"])
@pytest.mark.parametrize("case", BACKWARD_CASES, ids=_ids)
def test_backward_bit_exact_and_within_the_sequential_sum_bound(case, with_valid):
    """dx == the float32 restatement bit for bit (the same terms in the same order), and |dx - dx64| <= 1.01 (n - 1) 2^-24 S per
    element, n the number of terms and S the sum of their |dy|: the bound of a sequential float32 sum of n terms (each of the
    n - 1 additions rounds a partial sum of magnitude <= S by at most 2^-24 of it; 1.01 covers the second-order terms).  The
    argmax is the device's own, which must be the restatement's.  Two runs give the same bits."""
    B, H, W, C, R, ph, pw = case
    x, dy, ref_idx, rois, valid, (dx32, dx64, n, S) = _backward_case(case, with_valid)
    _out, idx = roi_utils.roi_max_pooling(x, rois, (ph, pw), valid=valid, return_argmax=True)
    assert np.array_equal(idx, ref_idx)
    dx = roi_utils.roi_max_pooling_backward(dy, idx, rois, (B, H, W, C), valid=valid)
    again = roi_utils.roi_max_pooling_backward(dy, idx, rois, (B, H, W, C), valid=valid)
    assert dx.dtype == np.float32 and dx.shape == (B, H, W, C) and np.array_equal(_bits(dx), _bits(again))
    excess = np.abs(dx.astype(np.float64) - dx64) - mh.backward_bound(n, S)
    print("backward:", case, "valid" if with_valid else "all", "max terms", n.max(), "max |dx - dx64|", np.abs(dx - dx64).max(),
          "max bound", mh.backward_bound(n, S).max(), "differing bits", (_bits(dx) != _bits(dx32)).sum())
    assert np.array_equal(_bits(dx), _bits(dx32))
    assert excess.max() <= 0, (excess.max(), np.unravel_index(excess.argmax(), excess.shape))
    assert not dx[n == 0].any()                                                   # pixels no bin chose: written as zeros


def test_backward_extent_reaches_the_kernel():
    rng = np.random.RandomState(9)
    x = rng.standard_normal((1, 31, 31, 8)).astype(np.float32)
    rois = rh.nasty_boxes(rng, 1, 18)
    dy = rng.standard_normal((1, 18, 7, 7, 8)).astype(np.float32)
    for extent in ((31.25, 29.0), (12.0, 44.0)):
        _out, idx = _assert_forward(x, rois, 7, 7, extent=extent)
        dx = roi_utils.roi_max_pooling_backward(dy, idx, rois, x.shape, extent=extent)
        assert np.array_equal(_bits(dx), _bits(mh.roi_max_pool_backward_ref(dy, idx, x.shape)[0]))


def test_backward_of_one_image_ignores_the_other_image():
    rng = np.random.RandomState(7)
    B, H, W, C, R, ph, pw = 2, 7, 7, 16, 70, 3, 3
    x = torch.from_numpy(rng.standard_normal((B, H, W, C)).astype(np.float32)).cuda()
    dy = torch.from_numpy(rng.standard_normal((B, R, ph, pw, C)).astype(np.float32)).cuda()
    rois = torch.from_numpy(rh.nasty_boxes(rng, B, R)).cuda()
    valid = torch.tensor([R, R], dtype=torch.int32, device="cuda")
    _o, idx = roi_utils.roi_max_pooling(x, rois, (ph, pw), valid=valid, return_argmax=True)
    dx = roi_utils.roi_max_pooling_backward(dy, idx, rois, (B, H, W, C), valid=valid)
    assert torch.equal(dx, roi_utils.roi_max_pooling_backward(dy, idx, rois, (B, H, W, C), valid=valid))
    rois2, valid2 = rois.clone(), valid.clone()
    rois2[1] = torch.from_numpy(rh.interior_boxes(rng, 1, R)[0]).cuda()
    valid2[1] = 3
    _o, idx2 = roi_utils.roi_max_pooling(x, rois2, (ph, pw), valid=valid2, return_argmax=True)
    dx2 = roi_utils.roi_max_pooling_backward(dy, idx2, rois2, (B, H, W, C), valid=valid2)
    assert torch.equal(dx[0], dx2[0]) and not torch.equal(dx[1], dx2[1])
    alone = roi_utils.roi_max_pooling_backward(dy[:1], idx[:1], rois[:1], (1, H, W, C), valid=valid[:1])
    assert torch.equal(alone[0], dx[0])


def test_autograd_calls_the_backward_kernel_and_no_argmax_is_kept_without_grad():
    rng = np.random.RandomState(8)
    x = torch.from_numpy(rng.standard_normal((2, 5, 9, 20)).astype(np.float32)).cuda().requires_grad_()
    rois = torch.from_numpy(rh.nasty_boxes(rng, 2, 9)).cuda()
    valid = torch.tensor([9, 4], dtype=torch.int32, device="cuda")
    kw = dict(extent=(5.5, 9.25), valid=valid)
    plain = roi_utils.roi_max_pooling(x.detach(), rois, (2, 3), **kw)
    assert isinstance(plain, torch.Tensor) and not plain.requires_grad             # one tensor: no argmax was allocated
    _o, idx = roi_utils.roi_max_pooling(x.detach(), rois, (2, 3), return_argmax=True, **kw)
    out = roi_utils.roi_max_pooling(x, rois, (2, 3), **kw)
    assert isinstance(out, torch.Tensor) and out.requires_grad and torch.equal(out.detach().view(torch.int32), plain.view(torch.int32))
    w = torch.from_numpy(rng.standard_normal(tuple(out.shape)).astype(np.float32)).cuda()
    (out * w).sum().backward()
    direct = roi_utils.roi_max_pooling_backward(w, idx, rois, x.shape, **kw)
    assert x.grad is not None and torch.equal(x.grad, direct) and x.grad.abs().sum() > 0
    x.grad = None
    out, idx2 = roi_utils.roi_max_pooling(x, rois, (2, 3), return_argmax=True, **kw)
    assert torch.equal(idx2, idx) and not idx2.requires_grad
    out.sum().backward()
    assert torch.equal(x.grad, roi_utils.roi_max_pooling_backward(torch.ones_like(out), idx, rois, x.shape, **kw))
    with torch.no_grad():
        assert not roi_utils.roi_max_pooling(x, rois, (2, 3), **kw).requires_grad


@pytest.mark.parametrize("precision", ["f32", "f16x3"])
def test_model_level_max_pool_equals_max_pool_of_the_copied_tap(precision):
    """FeatureExtractor.roi_max_pool (straight from the arena: the split form under f16x3) == roi_max_pooling of the copied tap,
    bit for bit; propose_features(pooling="max_pool") returns propose's boxes and the max pool of those boxes; "crop" gives the
    bits it gave before any max pooling ran on the handle."""
    prop = ga._proposer("vgg16", precision)
    fe = prop.feature_extractor
    rng = np.random.RandomState(11)
    imgs = torch.from_numpy(rng.uniform(0, 1, size=(2, 96, 96, 3)).astype(np.float32)).cuda()
    with pytest.raises(ValueError):
        fe.roi_max_pool(torch.zeros((1, 1, 4), device="cuda"))                      # no forward has run on this handle
    crop_before = [t.clone() for t in prop.propose_features(imgs, (3, 2), pooling="crop")]
    for B in (1, 2):
        prop.forward(imgs[:B])
        rois = torch.from_numpy(rh.nasty_boxes(rng, B, 9)).cuda()
        valid = torch.tensor([8, 0][:B], dtype=torch.int32, device="cuda")
        tap = fe.output()[:B]
        assert tap.shape[1:3] == (6, 6) and tap.abs().max() > 0
        for v, extent in ((None, None), (valid, (6.0, 6.0)), (valid, (6.25, 5.5))):
            got = fe.roi_max_pool(rois, (7, 7), extent=extent, valid=v)
            assert got.shape == (B, 9, 7, 7, tap.shape[3])
            want = roi_utils.roi_max_pooling(tap, rois, (7, 7), extent=extent, valid=v)
            assert torch.equal(got.view(torch.int32), want.view(torch.int32))
        if precision == "f32":       # ... and the float32 tap against the restatement, end to end
            ref, _ = mh.roi_max_pool_ref(tap.cpu().numpy(), rois.cpu().numpy(), 7, 7, extent=(6.25, 5.5), valid=valid.cpu().numpy(), fast=True)
            assert np.array_equal(_bits(got.cpu().numpy()), _bits(ref))
        boxes, scores, nvalid, pooled = [t.clone() for t in prop.propose_features(imgs[:B], (3, 2), pooling="max_pool", sampling_ratio=4)]
        b2, s2, v2, _idx = prop.propose(imgs[:B])
        assert torch.equal(boxes, b2) and torch.equal(scores, s2) and torch.equal(nvalid, v2) and int(nvalid.min()) > 0
        want = roi_utils.roi_max_pooling(fe.output()[:B], b2, (3, 2), valid=v2)
        assert pooled.shape == want.shape and torch.equal(pooled.view(torch.int32), want.view(torch.int32))
        assert pooled.abs().sum() > 0
        for b in range(B):
            assert not pooled[b, int(nvalid[b]):].any()
        stride_exact = prop.propose_features(imgs[:B], (3, 2), pooling="max_pool", extent=(6.5, 6.5))[3]
        want = roi_utils.roi_max_pooling(fe.output()[:B], b2, (3, 2), extent=(6.5, 6.5), valid=v2)
        assert torch.equal(stride_exact.view(torch.int32), want.view(torch.int32))
    crop_after = prop.propose_features(imgs, (3, 2), pooling="crop")
    assert all(torch.equal(a.view(torch.int32), c.view(torch.int32)) for a, c in zip(crop_before, crop_after))
    assert not torch.equal(crop_after[3], pooled)
    with pytest.raises(ValueError):
        fe.roi_max_pool(torch.zeros((3, 1, 4), device="cuda"))                      # beyond max_batch
    with pytest.raises(ValueError):
        prop.propose_features(imgs, pooling="maximum")


def test_detect_with_max_pooling():
    prop = ga._proposer("vgg16", "f32")
    C = prop.feature_extractor.output_shape[3]
    head = DetectionHead(5, pooling_size=(3, 3), channels=C, hidden=(16, 16), max_rois=2 * prop.topn, trainable=False, seed=2)
    imgs = torch.from_numpy(np.random.RandomState(0).uniform(0, 1, size=(2, 96, 96, 3)).astype(np.float32)).cuda()
    kw = dict(score_threshold=0.01, max_total_size=50)
    crop = [t.clone() for t in prop.detect(imgs, head, **kw)]
    rois, _s, valid, pooled = prop.propose_features(imgs, pooling_size=(3, 3), pooling="max_pool")
    want = [t.clone() for t in head.detect(rois, pooled, prop.hyper_params["variances"], valid=valid, **kw)]
    got = [t.clone() for t in prop.detect(imgs, head, pooling="max_pool", **kw)]
    assert all(torch.equal(a, b) for a, b in zip(got, want)) and int(got[3].sum()) > 0
    assert all(torch.equal(a, b) for a, b in zip(crop, prop.detect(imgs, head, pooling="crop", **kw)))


def test_argument_errors_are_raised_before_any_launch():
    x, rois = np.zeros((1, 3, 3, 8), np.float32), np.zeros((1, 2, 4), np.float32)
    g, idx = np.zeros((1, 2, 2, 2, 8), np.float32), np.zeros((1, 2, 2, 2, 8), np.int32)
    bad_forward = [dict(feature_map=np.zeros((1, 3, 3, 6), np.float32)), dict(feature_map=np.zeros((3, 3, 8), np.float32)),
                   dict(rois=np.zeros((1, 2, 3), np.float32)), dict(rois=np.zeros((2, 2, 4), np.float32)),
                   dict(valid=np.zeros((2,), np.int32)), dict(pooling_size=(0, 2))]
    bad_backward = [dict(argmax=idx.astype(np.int64)), dict(argmax=g), dict(argmax=idx[:, :1]), dict(rois=np.zeros((1, 3, 4), np.float32)),
                    dict(feature_shape=(1, 3, 3, 4)), dict(feature_shape=(2, 3, 3, 8)), dict(valid=np.zeros((2,), np.int32)),
                    dict(argmax=torch.zeros(idx.shape, dtype=torch.float32, device="cuda"))]
    for e in ((0, 3), (3, -1.0), (float("nan"), 3), (3, float("inf"))):
        bad_forward.append(dict(extent=e))
        bad_backward.append(dict(extent=e))
    for bad in bad_forward:
        with pytest.raises(ValueError):
            roi_utils.roi_max_pooling(**dict(dict(feature_map=x, rois=rois, pooling_size=(2, 2)), **bad))
    for bad in bad_backward:
        with pytest.raises(ValueError):
            roi_utils.roi_max_pooling_backward(**dict(dict(grad_out=g, argmax=idx, rois=rois, feature_shape=x.shape), **bad))
    assert roi_utils.roi_max_pooling_backward(g, idx, rois, x.shape).shape == x.shape


def test_load_keras_weights_on_the_device():
    """tests/golden/keras_vgg16_fc_tiny.h5 (tests/golden/make_keras_fc_fixture.py): fc1 / fc2 come back from the device as the file
    holds them, bit for bit; cls / reg keep their initial values."""
    from test_h5_weights import expected_array                                     # the fixture generators' formula
    head = DetectionHead(3, pooling_size=(2, 2), channels=4, hidden=(8, 8), max_rois=4, seed=3)
    before = head.get_weights()
    assert head.load_keras_weights(os.path.join(GOLDEN, "keras_vgg16_fc_tiny.h5")) == ["fc1", "fc2"]
    after = head.get_weights()
    for name, shape in (("fc1", (16, 8)), ("fc2", (8, 8))):
        for p, s in (("kernel", shape), ("bias", shape[1:])):
            want = expected_array("%s/%s/%s:0" % (name, name, p), s)
            assert np.array_equal(_bits(after[name][p]), _bits(want)) and not np.array_equal(after[name][p], before[name][p])
    for name in ("cls", "reg"):
        for p in ("kernel", "bias"):
            assert np.array_equal(_bits(after[name][p]), _bits(before[name][p]))
    big = DetectionHead(3, pooling_size=(3, 3), channels=4, hidden=(8, 8), max_rois=4, seed=3)
    with pytest.raises(ValueError) as e:
        big.load_keras_weights(os.path.join(GOLDEN, "keras_vgg16_fc_tiny.h5"))
    assert "fc1" in str(e.value) and "(16, 8)" in str(e.value) and "(36, 8)" in str(e.value)
    with pytest.raises(ValueError):
        head.load_keras_weights(os.path.join(GOLDEN, "keras_weights_vlen_strings.h5"))      # a file without fc1 / fc2
