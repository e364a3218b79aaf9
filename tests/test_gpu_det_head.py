"""The detection head on the GPU (rpn_fc_forward, rpn_det_head_*, models.DetectionHead, Proposer.detect) against the float64
restatements of tests/test_det_head_host.py.

Tolerances (none of them comes from what the kernels give):
  * forward, gradients, grad_pooled: elementwise inside `bounds` / `product_bound` of tests/test_det_head_host.py, the first-order
    float32 forward error analysis stated there; the cases assert on the CPU that the ReLU masks of float32 and float64 agree.
  * everything the contract calls bit-identical (a second run, another batch size, no_grad against grad mode, weights round trips,
    roi_pooling_backward of the head's grad_pooled) is compared byte for byte.
  * Adam: 1e-6 * max|w| after three steps at learning_rate 1e-3, the bar tests/test_train.py::test_adam_steps_and_test_on_batch holds
    the RPN head to.
  * end to end: the head's bound with the output gradients' own error (the loss kernel's 2e-6 * max|g| of tests/test_gpu_roi_head.py
    plus the softmax / Huber derivatives, at most 2 / n and 1 / n, times the bound on the logits / deltas they were computed from),
    pushed through the float64 adjoint of the pool, plus that adjoint's own rounding: at most R ph pw 4 terms per pixel, each with
    two roundings in its weight, on the scale of the unit-weight adjoint of |grad_pooled|.
"""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import test_det_head_host as dh  # noqa: E402
import test_roi_head_host as rh  # noqa: E402
import test_roi_host as rp  # noqa: E402
from oracle import bbox_oracle as bo  # noqa: E402
from test_det_head_host import lib  # noqa: E402,F401  (fixture)
from tf_rpn_amd import _lib as L  # noqa: E402
from tf_rpn_amd.models import DetectionHead  # noqa: E402
from tf_rpn_amd.utils import roi_utils  # noqa: E402

pytestmark = pytest.mark.gpu
LAYERS = dh.LAYERS


def bits(t):
    a = t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)
    return np.ascontiguousarray(a).view(np.uint32 if a.dtype.itemsize == 4 else np.uint8)


def same_bits(a, b):
    return np.array_equal(bits(a), bits(b))


# ---- 1. the GEMM on its own -----------------------------------------------------------------------------------------------------------------
def fc(lib, a, w_padded, bias, N, relu):
    M, K = (int(v) for v in a.shape)
    out = torch.full((M, N), float("nan"), dtype=torch.float32, device="cuda")
    st = lib.rpn_fc_forward(L.ptr(a), L.ptr(w_padded), L.ptr(bias), M, K, N, int(w_padded.shape[1]), int(relu), L.ptr(out), L.stream_ptr())
    L.check(st, "rpn_fc_forward")
    return out


@pytest.mark.parametrize("N", [3, 12, 68, 132])
@pytest.mark.parametrize("K", [32, 108, 516])
def test_fc_forward_against_float64(lib, K, N):
    rng = np.random.RandomState(1000 * K + N)
    A = rng.uniform(-1.0, 1.0, size=(130, K)).astype(np.float32)
    A[rng.uniform(size=A.shape) < 0.03] = 0.0
    A[1] = 0.0                                                   # the all-zero row (present for M > 1)
    W = rng.uniform(-1.0, 1.0, size=(K, N)).astype(np.float32)
    W[rng.uniform(size=W.shape) < 0.03] = 0.0
    bias = rng.uniform(-1.0, 1.0, size=(N,)).astype(np.float32)
    ldw = (N + 3) // 4 * 4
    Wp = np.full((K, ldw), 7.0, np.float32)                      # the padding columns are read and must be dropped
    Wp[:, :N] = W
    a_d, w_d, b_d = torch.from_numpy(A).cuda(), torch.from_numpy(Wp).cuda(), torch.from_numpy(bias).cuda()
    A64, W64 = A.astype(np.float64), W.astype(np.float64)
    full = {}
    for M in (1, 74, 130):
        for use_bias in (False, True):
            z = A64[:M] @ W64 + (bias.astype(np.float64) if use_bias else 0.0)
            bound = dh.product_bound(A64[:M], W64, bias if use_bias else None)
            for relu in (0, 1):
                ref = np.maximum(z, 0.0) if relu else z
                a_m = a_d[:M].contiguous()
                got_t = fc(lib, a_m, w_d, b_d if use_bias else None, N, relu)
                got = got_t.cpu().numpy()
                assert got.shape == (M, N) and not np.isnan(got).any()
                err = np.abs(got - ref)
                print("M %3d K %3d N %3d bias %d relu %d: max err %.3e, max err / bound %.3f" % (M, K, N, use_bias, relu, err.max(),
                                                                                             (err / np.maximum(bound, 1e-300)).max()))
                assert (err <= bound).all()
                assert same_bits(got_t, fc(lib, a_m, w_d, b_d if use_bias else None, N, relu))        # a second call: the same bytes
                if M > 1:
                    act_bias = np.maximum(bias, np.float32(0)) if relu else bias
                    assert same_bits(got[1], act_bias if use_bias else np.zeros((N,), np.float32))    # the zero row: act(bias)
                if M == 130:
                    full[(use_bias, relu)] = got
    # batch independence: row m of the M = 130 result is the M = 1 result of row m alone, byte for byte
    for m in (0, 1, 31, 32, 63, 64, 73, 127, 128, 129):
        for (use_bias, relu), got in full.items():
            one = fc(lib, a_d[m:m + 1].contiguous(), w_d, b_d if use_bias else None, N, relu)
            assert same_bits(one[0], got[m]), (m, use_bias, relu)


# ---- 2. / 3. the whole head -------------------------------------------------------------------------------------------------------------------
def make_head(c, trainable=True, **kw):
    ph, pw, Cf, H1, H2, C = c["dims"]
    head = DetectionHead(C, pooling_size=(ph, pw), channels=Cf, hidden=(H1, H2), max_rois=74, trainable=trainable, **kw)
    head.set_weights(c["weights"])
    return head


def inside(got, ref, bound, what):
    got = got.detach().cpu().numpy() if isinstance(got, torch.Tensor) else np.asarray(got)
    err = np.abs(got.astype(np.float64) - ref)
    print("%-18s max |ref| %.3e  max err %.3e  max err / bound %.3f" % (what, np.abs(ref).max(), err.max(),
                                                                     (err / np.maximum(bound, 1e-300)).max()))
    assert got.shape == ref.shape and (err <= bound).all(), what


@pytest.mark.parametrize("index", range(len(dh.HEAD_CONFIGS)))
def test_head_forward(lib, index):
    c = dh.head_case(index)
    C = c["dims"][5]
    head = make_head(c)
    pooled = torch.from_numpy(np.array(c["pooled"])).cuda()
    logits, deltas = head(pooled)
    assert tuple(logits.shape) == (2, 37, C) and tuple(deltas.shape) == (2, 37, 4 * C)
    assert logits.dtype == torch.float32 and deltas.dtype == torch.float32 and logits.is_contiguous() and deltas.is_contiguous()
    assert logits.requires_grad and deltas.requires_grad
    b = dh.bounds(c["weights"], c["pooled"])
    inside(logits, c["ref"]["logits"], b["logits"], "logits")
    inside(deltas, c["ref"]["deltas"], b["deltas"], "deltas")
    with torch.no_grad():
        l2, d2 = head(pooled)
    assert not l2.requires_grad and same_bits(l2, logits) and same_bits(d2, deltas)
    # the same RoIs in a batch of one image, and on the inference head: the same bits
    infer = make_head(c, trainable=False)
    l3, d3 = infer(pooled[1:2])
    assert same_bits(l3, logits[1:2]) and same_bits(d3, deltas[1:2])


def loss_gradients(logits, deltas, labels, roi_deltas):
    """what rpn_roi_losses hands the head for the loss reg + cls: (grad_logits, grad_deltas) as the device computed them"""
    l, d = logits.detach().clone().requires_grad_(), deltas.detach().clone().requires_grad_()
    reg_loss, cls_loss = roi_utils.roi_losses(l, d, torch.from_numpy(np.array(labels)).cuda(), torch.from_numpy(np.array(roi_deltas)).cuda())
    (reg_loss + cls_loss).backward()
    return l.grad, d.grad


def run_backward(head, c, pooled):
    logits, deltas = head(pooled)
    gl, gd = loss_gradients(logits, deltas, c["labels"], c["deltas"])
    torch.autograd.backward([logits, deltas], [gl, gd])
    return gl, gd


@pytest.mark.parametrize("index", range(len(dh.HEAD_CONFIGS)))
def test_head_backward(lib, index):
    c = dh.head_case(index)
    head = make_head(c)
    pooled = torch.from_numpy(np.array(c["pooled"])).cuda().requires_grad_()
    gl, gd = run_backward(head, c, pooled)
    ignored = torch.from_numpy(np.array(c["labels"]) < 0).cuda()
    assert int(ignored.sum()) > 0 and int((~ignored).sum()) > 0 and int((np.array(c["labels"]) > 0).sum()) > 0
    assert not bits(gl[ignored]).any() and not bits(gd[ignored]).any()              # ignored rows: exactly +0.0 rows of dZ
    assert float(gl.abs().max()) > 0 and float(gd.abs().max()) > 0
    gl64, gd64 = gl.cpu().numpy().astype(np.float64), gd.cpu().numpy().astype(np.float64)
    ref_g, ref_gp = dh.det_head_backward_ref(c["weights"], c["pooled"], gl64, gd64)
    b = dh.bounds(c["weights"], c["pooled"], gl64, gd64)
    got = head.get_gradients()
    for n in LAYERS:
        for k in ("kernel", "bias"):
            assert got[n][k].dtype == np.float32
            inside(got[n][k], ref_g[n][k], b[n][k], "%s/%s" % (n, k))
    inside(pooled.grad, ref_gp, b["grad_pooled"], "grad_pooled")
    # a second run: identical bytes
    first_gp = pooled.grad.clone()
    pooled.grad = None
    run_backward(head, c, pooled)
    again = head.get_gradients()
    assert same_bits(pooled.grad, first_gp)
    assert all(same_bits(again[n][k], got[n][k]) for n in LAYERS for k in ("kernel", "bias"))
    # pooled without a gradient (autograd passes NULL for grad_pooled): the parameter gradients are the same bytes
    run_backward(head, c, pooled.detach())
    third = head.get_gradients()
    assert all(same_bits(third[n][k], got[n][k]) for n in LAYERS for k in ("kernel", "bias"))
    # the ABI itself: d_grad_pooled non-NULL is written in full with the same bytes; NULL succeeds, writes no such tensor and leaves the
    # same parameter gradients
    x = pooled.detach()
    head._forward(x, keep=True)
    gp = torch.full_like(x, float("nan"))
    back = lambda out: lib.rpn_det_head_backward(head._h, L.ptr(x), 74, L.ptr(gl), L.ptr(gd), L.ptr(out), L.stream_ptr())
    assert back(gp) == L.RPN_OK and same_bits(gp, first_gp)
    with_gp = head.get_gradients()
    assert back(None) == L.RPN_OK
    without_gp = head.get_gradients()
    for n in LAYERS:
        for k in ("kernel", "bias"):
            assert same_bits(with_gp[n][k], got[n][k]) and same_bits(without_gp[n][k], got[n][k])
    # ... and it goes back through the kept forward's own input only
    other = x.clone()
    assert lib.rpn_det_head_backward(head._h, L.ptr(other), 74, L.ptr(gl), L.ptr(gd), None, L.stream_ptr()) == L.RPN_ERR_INVALID
    assert b"no kept forward" in lib.rpn_last_error()
    assert lib.rpn_det_head_backward(head._h, L.ptr(x), 37, L.ptr(gl), L.ptr(gd), None, L.stream_ptr()) == L.RPN_ERR_INVALID
    head._forward(x, keep=False)                                 # a forward that keeps nothing leaves nothing to go back through
    assert back(None) == L.RPN_ERR_INVALID and b"no kept forward" in lib.rpn_last_error()


def test_backward_of_a_stale_forward_raises(lib):
    """The head keeps ONE forward's activations.  The backward of a call that is no longer the head's most recent one -- after a kept
    forward of the same row count (two batches before one .backward()), a forward that keeps nothing, new weights or an Adam step --
    raises ValueError and leaves the stored gradients alone; it never computes from another call's activations."""
    c = dh.head_case(0)
    head = make_head(c)
    pooled_a = torch.from_numpy(np.array(c["pooled"])).cuda().requires_grad_()
    pooled_b = (torch.from_numpy(np.array(c["pooled"])).cuda().flip(1).contiguous() * 0.5).requires_grad_()
    gl, gd = run_backward(head, c, pooled_b)                     # the gradients of batch B, the reference for "left alone"
    grads_b = head.get_gradients()
    out_a = head(pooled_a)
    out_b = head(pooled_b)                                       # same M, kept: the row-count guard alone would let A's backward through
    with pytest.raises(ValueError, match="most recent call"):
        torch.autograd.backward(list(out_a), [gl, gd])
    assert pooled_a.grad is None
    after = head.get_gradients()
    assert all(same_bits(after[n][k], grads_b[n][k]) for n in LAYERS for k in ("kernel", "bias"))
    pooled_b.grad = None
    torch.autograd.backward(list(out_b), [gl, gd])               # the most recent call still goes back, with B's bytes
    again = head.get_gradients()
    assert all(same_bits(again[n][k], grads_b[n][k]) for n in LAYERS for k in ("kernel", "bias"))
    # (loss_a + loss_b).backward() in one graph fails the same way
    out_a, out_b = head(pooled_a), head(pooled_b)
    with pytest.raises(ValueError, match="most recent call"):
        (out_a[0].sum() + out_b[0].sum()).backward()
    for stale in (lambda: head(pooled_a.detach()), lambda: head.set_weights(c["weights"]), head.apply_gradients):
        out = head(pooled_a)
        with torch.no_grad():
            stale()
        with pytest.raises(ValueError, match="most recent call"):
            torch.autograd.backward(list(out), [gl, gd])


# ---- 4. Adam ------------------------------------------------------------------------------------------------------------------------------------
def test_adam_steps(lib):
    c = dh.head_case(0)
    head = make_head(c)
    lr = 1e-3
    head.compile(learning_rate=lr)
    pooled = torch.from_numpy(np.array(c["pooled"])).cuda()
    w64 = {n: {k: v.astype(np.float64) for k, v in d.items()} for n, d in head.get_weights().items()}
    mv = {n: {k: (np.zeros_like(v), np.zeros_like(v)) for k, v in d.items()} for n, d in w64.items()}
    assert head.train_steps() == 0
    for t in (1, 2, 3):
        run_backward(head, c, pooled)
        g = head.get_gradients()
        head.apply_gradients()
        for n in LAYERS:
            for k in ("kernel", "bias"):
                w64[n][k], m, v = dh.adam64(w64[n][k], g[n][k].astype(np.float64), *mv[n][k], t, lr)
                mv[n][k] = (m, v)
        got = head.get_weights()
        if t in (1, 3):
            for n in LAYERS:
                for k in ("kernel", "bias"):
                    ref = w64[n][k]
                    err = np.abs(got[n][k] - ref).max()
                    print("t %d %s/%s: max err %.3e, bar %.3e" % (t, n, k, err, 1e-6 * np.abs(ref).max()))
                    assert err <= 1e-6 * np.abs(ref).max(), (t, n, k)
                    assert not np.array_equal(got[n][k], c["weights"][n][k])
        assert head.train_steps() == t
        head(pooled)                                             # a forward between steps, kept ...
        with torch.no_grad():
            head(pooled)                                         # ... or not, changes no weight
        after = head.get_weights()
        assert all(same_bits(after[n][k], got[n][k]) for n in LAYERS for k in ("kernel", "bias"))
        assert head.train_steps() == t


# ---- 5. end to end through autograd -----------------------------------------------------------------------------------------------------------
def test_feature_map_gradient_end_to_end(lib):
    c = dh.e2e_case()
    ph, pw, Cf, H1, H2, C = c["dims"]
    head = make_head(c)
    feat = torch.from_numpy(c["feat"]).cuda().requires_grad_()
    rois, valid = torch.from_numpy(c["rois"]).cuda(), torch.from_numpy(np.array(c["valid"])).cuda()
    assert int(c["valid"].min()) < 37                            # some RoIs lie beyond valid
    pooled = roi_utils.roi_pooling(feat, rois, (ph, pw), valid=valid)
    pooled.retain_grad()
    assert same_bits(pooled, c["pooled"])                        # (the pool's own contract: the case's masks were checked on these bits)
    logits, deltas = head(pooled)
    labels, roi_deltas = torch.from_numpy(np.array(c["labels"])).cuda(), torch.from_numpy(np.array(c["deltas"])).cuda()
    reg_loss, cls_loss = roi_utils.roi_losses(logits, deltas, labels, roi_deltas)
    (reg_loss + cls_loss).backward()
    assert feat.grad is not None and tuple(feat.grad.shape) == tuple(feat.shape)
    through_pool = roi_utils.roi_pooling_backward(pooled.grad, rois, tuple(feat.shape), valid=valid)
    assert same_bits(feat.grad, through_pool)
    # the same chain in float64
    w = {n: {k: torch.tensor(np.asarray(v, np.float64)) for k, v in c["weights"][n].items()} for n in LAYERS}
    x = torch.tensor(c["pooled"].astype(np.float64), requires_grad=True)
    lin = lambda a, n: torch.nn.functional.linear(a, w[n]["kernel"].t(), w[n]["bias"])
    h2 = torch.relu(lin(torch.relu(lin(x.reshape(74, -1), "fc1")), "fc2"))
    l64, d64 = lin(h2, "cls"), lin(h2, "reg")
    l64.retain_grad(), d64.retain_grad()
    lab = torch.from_numpy(c["labels"].reshape(-1).astype(np.int64))
    kept, pos = lab >= 0, lab > 0
    n_kept, n_pos = max(1, int(kept.sum())), max(1, int(pos.sum()))
    cls64 = torch.nn.functional.cross_entropy(l64[kept], lab[kept], reduction="sum") / n_kept
    pred = d64.reshape(74, C, 4)[pos, lab[pos]]
    target = torch.tensor(np.asarray(c["deltas"], np.float64).reshape(74, 4))[pos]
    reg64 = torch.nn.functional.smooth_l1_loss(pred, target, reduction="sum", beta=1.0) / n_pos
    (reg64 + cls64).backward()
    print("losses: device %.7f %.7f, float64 %.7f %.7f" % (float(reg_loss.detach()), float(cls_loss.detach()), float(reg64.detach()), float(cls64.detach())))
    gl64, gd64, gp64 = l64.grad.numpy(), d64.grad.numpy(), x.grad.numpy()
    fwd = dh.bounds(c["weights"], c["pooled"])
    keptn, posn = kept.numpy()[:, None], pos.numpy()[:, None]
    e_gl = np.broadcast_to(keptn * (2.0 * fwd["logits"].reshape(74, C).max(axis=1, keepdims=True) / n_kept), (74, C)) + 2e-6 * np.abs(gl64).max()
    e_gd = posn * (fwd["deltas"].reshape(74, 4 * C) / n_pos) + 2e-6 * np.abs(gd64).max()
    b = dh.bounds(c["weights"], c["pooled"], gl64, gd64, e_grad_logits=e_gl, e_grad_deltas=e_gd)
    inside(pooled.grad, gp64, b["grad_pooled"], "grad_pooled")
    shape = tuple(c["feat"].shape)
    ref = rp.roi_pool_backward_ref(gp64, c["rois"], shape, valid=c["valid"], coord_dtype=np.float32)
    terms = 37 * ph * pw * 4
    bound = rp.roi_pool_backward_ref(b["grad_pooled"], c["rois"], shape, valid=c["valid"], coord_dtype=np.float32) + \
        2.0 * (terms + 4) * dh.U * rp.roi_pool_backward_ref(np.abs(gp64), c["rois"], shape, valid=c["valid"], coord_dtype=np.float32,
                                                           unit_weights=True)
    assert np.abs(ref).max() > 0
    inside(feat.grad, ref, bound, "feat.grad")


# ---- 6. weights round trip ----------------------------------------------------------------------------------------------------------------------
def test_weights_round_trip(lib, tmp_path):
    c = dh.head_case(1)
    head = make_head(c)
    pooled = torch.from_numpy(np.array(c["pooled"])).cuda()
    got = head.get_weights()
    assert all(same_bits(got[n][k], c["weights"][n][k]) for n in LAYERS for k in ("kernel", "bias"))
    head.set_weights(got)
    again = head.get_weights()
    assert all(same_bits(again[n][k], got[n][k]) for n in LAYERS for k in ("kernel", "bias"))
    with torch.no_grad():
        logits, deltas = head(pooled)
    path = str(tmp_path / "head.npz")
    head.save_weights(path)
    ph, pw, Cf, H1, H2, C = c["dims"]
    fresh = DetectionHead(C, pooling_size=(ph, pw), channels=Cf, hidden=(H1, H2), max_rois=74, seed=9)
    f0 = fresh.get_weights()
    limit = np.sqrt(6.0 / (ph * pw * Cf + H1))
    assert np.abs(f0["fc1"]["kernel"]).max() <= limit and np.abs(f0["fc1"]["kernel"]).max() > 0.9 * limit and not f0["fc1"]["bias"].any()
    assert sorted(fresh.load_weights(path)) == sorted(LAYERS)
    with torch.no_grad():
        l2, d2 = fresh(pooled)
    assert same_bits(l2, logits) and same_bits(d2, deltas)
    infer = DetectionHead(C, pooling_size=(ph, pw), channels=Cf, hidden=(H1, H2), max_rois=74, trainable=False)
    infer.set_weights(head.get_weights())
    l3, d3 = infer(pooled)
    assert not l3.requires_grad and same_bits(l3, logits) and same_bits(d3, deltas)
    assert infer.memory_bytes()[0] * 4 == head.memory_bytes()[0]


# ---- 7. detections -------------------------------------------------------------------------------------------------------------------------------
def test_detect_is_the_head_then_roi_detections(lib):
    c = dh.head_case(1)
    head = make_head(c)
    pooled = torch.from_numpy(np.array(c["pooled"])).cuda()
    t = rh.target_case(3)
    rois, valid = torch.from_numpy(np.array(t["rois"])).cuda(), torch.from_numpy(np.array(t["valid"])).cuda()
    kw = dict(valid=valid, score_threshold=0.02, max_total_size=50, max_output_size_per_class=10)
    got = head.detect(rois, pooled, rh.VARIANCES, **kw)
    with torch.no_grad():
        ref = roi_utils.roi_detections(rois, *reversed(head(pooled)), rh.VARIANCES, **kw)
    assert len(got) == len(ref) == 4 and int(got[3].sum()) > 0
    assert all(same_bits(a, b) for a, b in zip(got, ref))


def test_proposer_detect(lib):
    from tf_rpn_amd.models._rpn_model import synthetic_weights
    from tf_rpn_amd.predictor import Proposer
    hp = bo.get_hyper_params("vgg16", img_size=224, feature_map_shape=14)
    prop = Proposer("vgg16", hyper_params=dict(hp), weights=synthetic_weights("vgg16", hp, seed=1), precision="f32", max_batch=2)
    head = DetectionHead(21, pooling_size=(7, 7), channels=512, hidden=(64, 64), max_rois=2 * prop.topn, trainable=False, seed=2)
    imgs = torch.from_numpy(np.random.RandomState(0).uniform(0, 1, size=(2, 224, 224, 3)).astype(np.float32)).cuda()
    out = prop.detect(imgs, head, score_threshold=0.01, max_total_size=100)
    assert len(out) == 4
    boxes, scores, classes, valid = out
    assert tuple(boxes.shape) == (2, 100, 4) and tuple(scores.shape) == (2, 100) and tuple(classes.shape) == (2, 100)
    assert tuple(valid.shape) == (2,) and valid.dtype == torch.int32
    assert float(boxes.min()) >= 0.0 and float(boxes.max()) <= 1.0
    first = [t.clone() for t in out]
    again = prop.detect(imgs, head, score_threshold=0.01, max_total_size=100)
    assert all(same_bits(a, b) for a, b in zip(first, again))
