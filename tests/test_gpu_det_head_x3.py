"""The split-float16 inference head on the GPU (rpn_fc_forward_x3, rpn_det_head_create_ex / _status, models.DetectionHead
(precision="f16x3"), Proposer.detect) against the float64 restatements of tests/test_det_head_host.py, inside the a-priori bound
of tests/test_det_head_x3_host.py (`product_bound_x3`, `bounds_x3`: stated from the inputs alone, checked there on the CPU against
a numpy emulation of the contract).  Everything the contract calls bit-identical -- a second call, a row alone against the row in a
batch, the exact case against the emulation, weight round trips -- is compared byte for byte.
"""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import test_det_head_host as dh  # noqa: E402
import test_det_head_x3_host as hx  # noqa: E402
import test_roi_head_host as rh  # noqa: E402
from oracle import bbox_oracle as bo  # noqa: E402
from test_det_head_host import lib  # noqa: E402,F401  (fixture)
from test_gpu_det_head import fc, inside, same_bits  # noqa: E402
from tf_rpn_amd import _lib as L  # noqa: E402
from tf_rpn_amd.models import DetectionHead  # noqa: E402
from tf_rpn_amd.utils import roi_utils  # noqa: E402

pytestmark = pytest.mark.gpu
LAYERS = dh.LAYERS


def fc_x3(lib, a, w_padded, bias, N, relu, status=None):
    M, K = (int(v) for v in a.shape)
    out = torch.full((M, N), float("nan"), dtype=torch.float32, device="cuda")
    st = lib.rpn_fc_forward_x3(L.ptr(a), L.ptr(w_padded), L.ptr(bias), M, K, N, int(w_padded.shape[1]), int(relu), L.ptr(out),
                               L.ptr(status), L.stream_ptr())
    L.check(st, "rpn_fc_forward_x3")
    return out


def cuda(a):
    return torch.from_numpy(np.array(a)).cuda()


# ---- 1. / 3. the GEMM against float64, at the data's own scale and with the weights moved by powers of two ------------------------------------
@pytest.mark.parametrize("scale", (1.0,) + hx.SHIFT_SCALES)
@pytest.mark.parametrize("N", hx.GEMM_N)
@pytest.mark.parametrize("K", hx.GEMM_K)
def test_fc_forward_x3_against_float64(lib, K, N, scale):
    c = hx.gemm_case(K, N)
    A, bias = c["A"], c["bias"]
    W = (c["W"] * np.float32(scale)).astype(np.float32)
    a_d, w_d, b_d = cuda(A), cuda(hx.pad_columns(W)), cuda(bias)           # the padding columns (7.0) are read and must be dropped
    A64, W64 = A.astype(np.float64), W.astype(np.float64)
    full = {}
    for M in hx.GEMM_M:
        for use_bias in (False, True):
            z = A64[:M] @ W64 + (bias.astype(np.float64) if use_bias else 0.0)
            bound = hx.product_bound_x3(A64[:M], W64, bias if use_bias else None)
            for relu in (0, 1):
                ref = np.maximum(z, 0.0) if relu else z
                a_m = a_d[:M].contiguous()
                got_t = fc_x3(lib, a_m, w_d, b_d if use_bias else None, N, relu)
                got = got_t.cpu().numpy()
                assert got.shape == (M, N) and not np.isnan(got).any()
                err = np.abs(got - ref)
                print("M %3d K %3d N %3d scale %g bias %d relu %d: max err %.3e, max err / bound %.3f" % (
                    M, K, N, scale, use_bias, relu, err.max(), (err / np.maximum(bound, 1e-300)).max()))
                assert (err <= bound).all()
                assert same_bits(got_t, fc_x3(lib, a_m, w_d, b_d if use_bias else None, N, relu))      # a second call: the same bytes
                if M > 1:
                    act_bias = np.maximum(bias, np.float32(0)) if relu else bias
                    assert same_bits(got[1], act_bias if use_bias else np.zeros((N,), np.float32))    # the zero row: act(bias)
                if M == 130:
                    full[(use_bias, relu)] = got
    if scale != 1.0:
        return
    # batch independence: row m of the M = 130 result is the M = 1 result of row m alone, byte for byte
    for m in (0, 1, 15, 16, 31, 32, 63, 64, 127, 128, 129):
        for (use_bias, relu), got in full.items():
            one = fc_x3(lib, a_d[m:m + 1].contiguous(), w_d, b_d if use_bias else None, N, relu)
            assert same_bits(one[0], got[m]), (m, use_bias, relu)


# ---- 2. / 3. the exact case ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scale", (1.0, 2.0 ** 18))
@pytest.mark.parametrize("K", (32, 108))
def test_exact_case_equals_the_emulation_bit_for_bit(lib, K, scale):
    """every product is a multiple of 2^-12 and every partial sum fits float32 (asserted on the CPU): any order of summation gives
    the emulation's bits, and dropping one of the three products or misplacing a lo half does not"""
    c = hx.exact_case(K)
    W = (c["W"] * np.float32(scale)).astype(np.float32)
    z = hx.emulate_x3(c["A"], W)
    t = z / scale * 2.0 ** 14
    assert np.array_equal(t, np.round(t)) and np.abs(t).max() < 2.0 ** 21
    for parts in ((1, 0, 1), (1, 1, 0), (0, 1, 1)):
        assert not np.array_equal(hx.emulate_x3(c["A"], W, parts=parts), z)
    a_d, w_d = cuda(c["A"]), cuda(hx.pad_columns(W))
    got = fc_x3(lib, a_d, w_d, None, W.shape[1], 0)
    assert same_bits(got, z.astype(np.float32))
    # the float32 head's product keeps lo lo (about K 2^-23 here, against results of a few units): where that term survives the
    # rounding to float32 the two products differ
    f32 = fc(lib, a_d, w_d, None, W.shape[1], 0).cpu().numpy()
    full = c["A"].astype(np.float64) @ W.astype(np.float64)
    matters = full.astype(np.float32) != z.astype(np.float32)
    differs = got.cpu().numpy() != f32
    print("K %d scale %g: lo lo changes %d of %d float32 results; the float32 product differs at %d" % (K, scale, int(matters.sum()),
                                                                                                   matters.size, int(differs.sum())))
    assert matters.any() and differs.any()


# ---- 4. range ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("value,raised", [(70000.0, True), (-70000.0, True), (float("inf"), True), (float("nan"), True), (65504.0, False),
                                          (-65504.0, False)])
def test_range_flag_through_d_status(lib, value, raised):
    c = hx.gemm_case(108, 12)
    A = np.array(c["A"][:74])
    A[70, 101] = value                                           # in the K tail of the last step, in a row of the last row tile
    status = torch.zeros((1,), dtype=torch.int32, device="cuda")
    w_d = cuda(hx.pad_columns(c["W"]))
    fc_x3(lib, cuda(A), w_d, None, 12, 0, status=status)
    assert int(status.item()) == (L.STATUS_F16_RANGE if raised else 0)
    fc_x3(lib, cuda(c["A"][:74]), w_d, None, 12, 0, status=status)       # sticky: a clean product leaves it
    assert int(status.item()) == (L.STATUS_F16_RANGE if raised else 0)


def make_head_x3(c, **kw):
    ph, pw, Cf, H1, H2, C = c["dims"]
    head = DetectionHead(C, pooling_size=(ph, pw), channels=Cf, hidden=(H1, H2), max_rois=74, trainable=False, precision="f16x3", seed=None, **kw)
    head.set_weights(c["weights"])
    return head


def test_head_status_reads_and_clears_the_flag(lib):
    c = dh.head_case(1)
    head = make_head_x3(c)
    pooled = np.array(c["pooled"])
    assert head.status() == {"f16_range": False}
    head(cuda(pooled))
    assert head.status() == {"f16_range": False}
    bad = pooled.copy()
    bad[1, 5, 1, 0, 3] = 70000.0
    head(cuda(bad))
    head(cuda(pooled))                                           # sticky over a clean forward
    assert head.status() == {"f16_range": True}
    assert head.status(reset=True) == {"f16_range": True}
    assert head.status() == {"f16_range": False}
    # a hidden activation beyond the range: fc1's bias pushes h1 over 65504 while the pooled features stay small
    w = {n: {k: np.array(v) for k, v in d.items()} for n, d in c["weights"].items()}
    w["fc1"]["bias"][7] = 1.0e5
    head.set_weights(w)
    head(cuda(pooled))
    assert head.status(reset=True) == {"f16_range": True}
    f32 = DetectionHead(c["dims"][5], pooling_size=c["dims"][:2], channels=c["dims"][2], hidden=c["dims"][3:5], max_rois=74, trainable=False,
                        seed=None)
    f32.set_weights(w)
    f32(cuda(bad))
    assert f32.status(reset=True) == {"f16_range": False}        # a float32 head always reports 0


# ---- 5. long K -----------------------------------------------------------------------------------------------------------------------------------
def test_long_k(lib):
    """K1 = 25 088: 784 steps and packed offsets of 13 MB"""
    c = hx.long_k_case()
    M, K, N = hx.LONG_K
    got = fc_x3(lib, cuda(c["A"]), cuda(c["W"]), cuda(c["bias"]), N, 0)
    inside(got, c["ref"], c["bound"], "long K")
    f32 = fc(lib, cuda(c["A"]), cuda(c["W"]), cuda(c["bias"]), N, 0).cpu().numpy()
    print("long K: max |f16x3 - ref| %.3e, max |f32 - ref| %.3e" % (np.abs(got.cpu().numpy() - c["ref"]).max(), np.abs(f32 - c["ref"]).max()))


# ---- 6. the whole head ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("index", range(len(dh.HEAD_CONFIGS)))
def test_head_forward_x3(lib, index):
    c = dh.head_case(index)
    C = c["dims"][5]
    head = make_head_x3(c)
    assert head.precision == "f16x3"
    pooled = cuda(c["pooled"])
    logits, deltas = head(pooled)
    assert tuple(logits.shape) == (2, 37, C) and tuple(deltas.shape) == (2, 37, 4 * C)
    assert logits.dtype == torch.float32 and logits.is_contiguous() and deltas.is_contiguous() and not logits.requires_grad
    b = hx.bounds_x3(c["weights"], c["pooled"])
    inside(logits, c["ref"]["logits"], b["logits"], "logits")
    inside(deltas, c["ref"]["deltas"], b["deltas"], "deltas")
    l2, d2 = head(pooled)
    assert same_bits(l2, logits) and same_bits(d2, deltas)
    l3, d3 = head(pooled[1:2])
    assert same_bits(l3, logits[1:2]) and same_bits(d3, deltas[1:2])
    assert head.status() == {"f16_range": False}
    # the weights come back bit for bit, and a head given them computes the same bits
    got = head.get_weights()
    assert all(same_bits(got[n][k], c["weights"][n][k]) for n in LAYERS for k in ("kernel", "bias"))
    # the hidden layer on its own (the benchmark's hook) is the forward's first launch
    ph, pw, Cf, H1, H2, _ = c["dims"]
    x = pooled.reshape(74, -1).contiguous()
    h1 = torch.full((74, H1), float("nan"), device="cuda")
    L.check(lib.rpn_det_head_forward_layer(head._h, b"fc1", L.ptr(x), 74, L.ptr(h1), L.stream_ptr()), "forward_layer")
    s = hx.shift_of(c["weights"]["fc1"]["kernel"])
    ref_h1 = fc_x3(lib, x, cuda(c["weights"]["fc1"]["kernel"]), cuda(c["weights"]["fc1"]["bias"]), H1, 1)
    assert -100 <= s <= 24 and same_bits(h1, ref_h1)
    # training calls raise
    with pytest.raises(RuntimeError):
        with torch.enable_grad():
            head(pooled.clone().requires_grad_())
    with pytest.raises(ValueError):
        head.apply_gradients()
    with pytest.raises(ValueError):
        head.get_gradients()
    st = lib.rpn_det_head_backward(head._h, L.ptr(pooled), 74, L.ptr(logits), L.ptr(deltas), None, L.stream_ptr())
    assert st == L.RPN_ERR_INVALID and b"trainable = 0" in lib.rpn_last_error()


def test_inference_copy_of_a_trained_head(lib):
    c = dh.head_case(0)
    ph, pw, Cf, H1, H2, C = c["dims"]
    trained = DetectionHead(C, pooling_size=(ph, pw), channels=Cf, hidden=(H1, H2), max_rois=74, seed=None)
    trained.set_weights(c["weights"])
    trained.compile(learning_rate=1e-3)
    pooled = cuda(c["pooled"])
    logits, deltas = trained(pooled)
    torch.autograd.backward([logits, deltas], [torch.ones_like(logits) / 74, torch.ones_like(deltas) / 74])
    trained.apply_gradients()
    w = trained.get_weights()
    assert not np.array_equal(w["fc1"]["kernel"], c["weights"]["fc1"]["kernel"])
    copy = trained.inference_copy(precision="f16x3")
    assert copy.precision == "f16x3" and not copy.trainable and copy.max_rois == 74
    built = make_head_x3(dict(c, weights=w))
    out_copy, out_built = copy(pooled), built(pooled)
    assert same_bits(out_copy[0], out_built[0]) and same_bits(out_copy[1], out_built[1])
    got = copy.get_weights()
    assert all(same_bits(got[n][k], w[n][k]) for n in LAYERS for k in ("kernel", "bias"))
    # ... from an inference head too, and back to float32: the float32 head's own bits
    back = copy.inference_copy()
    assert back.precision == "f32"
    with torch.no_grad():
        ref = trained(pooled)
    out_back = back(pooled)
    assert same_bits(out_back[0], ref[0]) and same_bits(out_back[1], ref[1])
    b = hx.bounds_x3(w, c["pooled"])
    ref64 = dh.det_head_ref(w, c["pooled"])
    inside(out_copy[0], ref64["logits"], b["logits"], "logits of the copy")
    assert copy.memory_bytes()[1] == back.memory_bytes()[1] and copy.memory_bytes()[0] > back.memory_bytes()[0]


# ---- 7. detections -------------------------------------------------------------------------------------------------------------------------------
def test_detect_is_the_head_then_roi_detections(lib):
    c = dh.head_case(1)
    head = make_head_x3(c)
    pooled = cuda(c["pooled"])
    t = rh.target_case(3)
    rois, valid = cuda(t["rois"]), cuda(t["valid"])
    kw = dict(valid=valid, score_threshold=0.02, max_total_size=50, max_output_size_per_class=10)
    got = head.detect(rois, pooled, rh.VARIANCES, **kw)
    ref = roi_utils.roi_detections(rois, *reversed(head(pooled)), rh.VARIANCES, **kw)
    assert len(got) == len(ref) == 4 and int(got[3].sum()) > 0
    assert all(same_bits(a, b) for a, b in zip(got, ref))


def test_proposer_detect(lib):
    from tf_rpn_amd.models._rpn_model import synthetic_weights
    from tf_rpn_amd.predictor import Proposer
    hp = bo.get_hyper_params("vgg16", img_size=224, feature_map_shape=14)
    prop = Proposer("vgg16", hyper_params=dict(hp), weights=synthetic_weights("vgg16", hp, seed=1), precision="f16x3", max_batch=2)
    head = DetectionHead(21, pooling_size=(7, 7), channels=512, hidden=(64, 64), max_rois=2 * prop.topn, trainable=False, seed=2,
                         precision="f16x3")
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
    assert head.status() == {"f16_range": False}
