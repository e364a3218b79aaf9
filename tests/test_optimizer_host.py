"""CPU suite for the optimizers (include/rpn_hip.h, "Optimizers"; tf_rpn_amd/csrc/optim_kernels.hip): SGD momentum, L2 weight decay,
clipping by the global norm, the optimizer's state.  Here: the ABI checks that need no device, the register budgets, the decayed-range
tables against the documented layouts, and the restatements the GPU tests (tests/test_gpu_optimizer.py) compare with --

  sgd32: the contract in float32 numpy, every operation rounded on its own (numpy's float32 scalars and arrays round
      after every operation, as the kernel does): the SGD step must equal it byte for byte;
  sgd64, adam64_extras (adam64 of tests/test_train.py fed g2): the same rules in float64, the references of the 1e-6 bar test_adam_steps_and_test_on_batch holds.

sgd32 against sgd64.  One step rounds g1 = g c, wd w, g2, mu a, lr g2, a and w + a: relative U = 2^-24 each.  With |w| <= W, |a| <= A the
step's new error in w is at most U W (the final add) plus the error a carries, a few U A; A = O(lr |g|) << W here.  After 3 steps:
3 U W + O(U A) < 4 U W = 2 ulp-scale steps of W (one ulp-scale step = 2^-23 W).  That is the bound asserted below, from the formats alone.
"""
import ctypes
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import codeobj  # noqa: E402
import test_train as tt  # noqa: E402
from test_train import adam64, lib  # noqa: E402,F401  (fixture)
from oracle import bbox_oracle as bo  # noqa: E402
from tf_rpn_amd import _lib as L  # noqa: E402
from tf_rpn_amd.models._rpn_model import HEAD_LAYERS, RPNModel, synthetic_weights  # noqa: E402
from tf_rpn_amd.models.detection_head import DetectionHead  # noqa: E402

ROOT = tt.ROOT
F32 = np.float32
ADAM, SGD = 0, 1
NEW_SYMBOLS = ["rpn_head_trainer_set_optimizer", "rpn_det_head_set_optimizer", "rpn_head_trainer_grad_norm", "rpn_det_head_grad_norm",
               "rpn_head_trainer_decay_ranges", "rpn_det_head_decay_ranges", "rpn_head_trainer_get_slot", "rpn_head_trainer_set_slot",
               "rpn_head_trainer_get_bn_slot", "rpn_head_trainer_set_bn_slot", "rpn_det_head_get_slot", "rpn_det_head_set_slot",
               "rpn_head_trainer_set_steps", "rpn_det_head_set_steps", "rpn_grad_sq_norm_workspace_bytes", "rpn_grad_sq_norm",
               "rpn_optimizer_apply"]
NEW_KERNELS = ["grad_sq_norm_kernel", "grad_sq_norm_finish_kernel", "optim_apply_kernel<0>", "optim_apply_kernel<1>"]
# the norm kernel's grid: up to 2048 workgroups of 256 threads, one float4 per thread and sweep
SWEEP = 2048 * 256 * 4


# ---- restatements -----------------------------------------------------------------------------------------------------------------------
def decay_mask(n, ranges):
    mask = np.zeros(n, bool)
    for b, e in ranges:
        mask[b:e] = True
    return mask


def g2_of(w, g, scale, wd, mask, dtype):
    """g1 = g c (g itself without a scale); g2 = g1 + wd w on the decayed elements, g1 elsewhere -- in `dtype`, each operation rounded"""
    w, g = w.astype(dtype), g.astype(dtype)
    g1 = g * dtype(scale) if scale is not None else g
    return np.where(mask, g1 + dtype(wd) * w, g1) if wd else g1


def sgd_step(w, g, a, lr, mu, nesterov, wd, mask, scale, dtype):
    """ApplyKerasMomentum in `dtype`: a = mu a - lr g2; w += a (nesterov: w += mu a - lr g2 with the new a)"""
    g2 = g2_of(w, g, scale, wd, mask, dtype)
    step = dtype(lr) * g2
    a = dtype(mu) * a.astype(dtype) - step
    w = w.astype(dtype)
    return (w + (dtype(mu) * a - step) if nesterov else w + a), a


def sgd32(w, g, a, lr, mu=0.0, nesterov=False, wd=0.0, mask=None, scale=None):
    mask = np.zeros(w.shape, bool) if mask is None else mask
    out = sgd_step(w, g, a, F32(lr), F32(mu), nesterov, F32(wd), mask, None if scale is None else F32(scale), np.float32)
    assert out[0].dtype == np.float32 and out[1].dtype == np.float32
    return out


def sgd64(w, g, a, lr, mu=0.0, nesterov=False, wd=0.0, mask=None, scale=None):
    """the same rule in float64, fed the float32 hyper-parameters the kernel gets"""
    mask = np.zeros(w.shape, bool) if mask is None else mask
    return sgd_step(w, g, a, float(F32(lr)), float(F32(mu)), nesterov, float(F32(wd)), mask, None if scale is None else float(F32(scale)),
                    np.float64)


def adam64_extras(w, g, m, v, t, lr, wd=0.0, mask=None, scale=None, **kw):
    """adam64 fed g2"""
    mask = np.zeros(w.shape, bool) if mask is None else mask
    g2 = g2_of(w, g, None if scale is None else float(F32(scale)), float(F32(wd)), mask, np.float64)
    return adam64(w.astype(np.float64), g2, m, v, t, lr, **kw)


def clip_scale(S, C):
    """the finishing workgroup's c from the device's S"""
    r = np.sqrt(np.float64(S))
    return F32(1.0) if not C or r <= np.float64(F32(C)) else F32(np.float64(F32(C)) / r)


def test_sgd32_tracks_sgd64_within_two_ulp_steps():
    rng = np.random.RandomState(5)
    n = 4099
    mask = decay_mask(n, [(3, 1001), (2050, 4097)])
    for mu, nesterov, wd, scale in [(0.0, False, 0.0, None), (0.9, False, 5e-4, 0.37), (0.9, True, 5e-4, None), (0.5, True, 0.0, 0.9)]:
        w0 = rng.standard_normal(n).astype(np.float32)
        w32, a32, w64, a64 = w0.copy(), np.zeros(n, np.float32), w0.astype(np.float64), np.zeros(n)
        for _ in range(3):
            g = rng.standard_normal(n).astype(np.float32)
            w32, a32 = sgd32(w32, g, a32, 1e-2, mu, nesterov, wd, mask, scale)
            w64, a64 = sgd64(w64, g, a64, 1e-2, mu, nesterov, wd, mask, scale)
        assert np.abs(w32 - w64).max() <= 2 * 2.0 ** -23 * np.abs(w64).max()
        # an undecayed element does not see wd at all
        w32b, _ = sgd32(w0, g, np.zeros(n, np.float32), 1e-2, mu, nesterov, 0.0, mask, scale)
        w32c, _ = sgd32(w0, g, np.zeros(n, np.float32), 1e-2, mu, nesterov, wd, mask, scale)
        assert np.array_equal(w32b[~mask], w32c[~mask]) and (not wd or not np.array_equal(w32b[mask], w32c[mask]))


def test_clip_scale_restatement():
    assert clip_scale(4.0, 0.0) == 1.0 and clip_scale(4.0, 2.0) == 1.0 and clip_scale(4.0, 3.0) == 1.0
    assert clip_scale(16.0, 1.0) == F32(0.25) and clip_scale(16.0, 1.0).dtype == np.float32


# ---- the ABI ----------------------------------------------------------------------------------------------------------------------------
def test_new_symbols_are_declared_exported_and_bound(lib):
    code = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "rpn_hip.h")).read(), flags=re.S)
    raw = ctypes.CDLL(L.LIB_PATH)
    for name in NEW_SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, code), "%s is not declared" % name
        assert hasattr(raw, name) and name in L.exported_symbols()
    assert re.search(r"#define RPN_OPT_ADAM 0\b", code) and re.search(r"#define RPN_OPT_SGD 1\b", code)
    assert lib.rpn_abi_version() == 1


def _trainer(lib, backbone="vgg16", train_from=None, **hp_kw):
    hp = bo.get_hyper_params(backbone, **hp_kw)
    m = RPNModel(backbone, hp, max_batch=2)
    m.compile(train_backbone_from=train_from)
    return m, hp


def _head_handle(lib, C=3):
    h = L.vp(0)
    assert lib.rpn_det_head_create(2, 2, 8, 16, 12, C, 10, 1, ctypes.byref(h)) == L.RPN_OK
    return h


def test_set_optimizer_rejects_bad_values_without_a_device(lib):
    m, _ = _trainer(lib)
    h = _head_handle(lib)
    try:
        for fn, handle in ((lib.rpn_head_trainer_set_optimizer, m._t), (lib.rpn_det_head_set_optimizer, h)):
            for bad in ((SGD, 1.0, 0, 0.0, 0.0), (SGD, -0.1, 0, 0.0, 0.0), (SGD, float("nan"), 0, 0.0, 0.0), (ADAM, 0.0, 0, -1e-4, 0.0),
                        (ADAM, 0.0, 0, float("nan"), 0.0), (ADAM, 0.0, 0, float("inf"), 0.0), (SGD, 0.9, 0, 0.0, -1.0),
                        (SGD, 0.9, 0, 0.0, float("nan")), (2, 0.0, 0, 0.0, 0.0), (-1, 0.0, 0, 0.0, 0.0), (SGD, 0.9, 2, 0.0, 0.0)):
                assert fn(handle, *bad) == L.RPN_ERR_INVALID, bad
                assert lib.rpn_last_error(), bad
            assert fn(handle, SGD, 0.9, 1, 5e-4, 10.0) == L.RPN_OK
            assert fn(handle, ADAM, 0.0, 0, 0.0, 0.0) == L.RPN_OK
        norm, scale = ctypes.c_double(0), ctypes.c_float(0)
        # no clip norm configured / no step run: nothing to report
        assert lib.rpn_head_trainer_grad_norm(m._t, ctypes.byref(norm), ctypes.byref(scale), None) == L.RPN_ERR_INVALID
        assert lib.rpn_det_head_grad_norm(h, ctypes.byref(norm), ctypes.byref(scale), None) == L.RPN_ERR_INVALID
        assert lib.rpn_det_head_set_optimizer(h, SGD, 0.9, 0, 0.0, 5.0) == L.RPN_OK
        assert lib.rpn_det_head_grad_norm(h, ctypes.byref(norm), ctypes.byref(scale), None) == L.RPN_ERR_INVALID
        assert lib.rpn_head_trainer_set_steps(m._t, -1) == L.RPN_ERR_INVALID and lib.rpn_det_head_set_steps(h, -1) == L.RPN_ERR_INVALID
        assert lib.rpn_head_trainer_set_steps(m._t, 7) == L.RPN_OK and m.train_steps() == 7
        # switching the rule zeroes the step count; the same rule keeps it
        assert lib.rpn_head_trainer_set_optimizer(m._t, ADAM, 0.0, 0, 1e-4, 0.0) == L.RPN_OK and m.train_steps() == 7
        assert lib.rpn_head_trainer_set_optimizer(m._t, SGD, 0.0, 0, 0.0, 0.0) == L.RPN_OK and m.train_steps() == 0
        # a bad slot, an unknown or frozen layer
        buf = (ctypes.c_float * (9 * 512 * 512))()
        assert lib.rpn_head_trainer_get_slot(m._t, b"rpn_conv", 2, buf, buf, None) == L.RPN_ERR_INVALID
        assert lib.rpn_head_trainer_get_slot(m._t, b"block5_conv3", 0, buf, buf, None) == L.RPN_ERR_INVALID
        assert lib.rpn_det_head_get_slot(h, b"fc1", 2, buf, buf, None) == L.RPN_ERR_INVALID
        assert lib.rpn_det_head_get_slot(h, b"fc3", 0, buf, buf, None) == L.RPN_ERR_INVALID
        # the stand-alone entries validate before the device
        assert lib.rpn_grad_sq_norm_workspace_bytes(0) == 0 and lib.rpn_grad_sq_norm_workspace_bytes(1) >= 8
        assert lib.rpn_grad_sq_norm_workspace_bytes(10 * SWEEP) == lib.rpn_grad_sq_norm_workspace_bytes(SWEEP) == 2048 * 8
        a = L.vp(4096)
        assert lib.rpn_grad_sq_norm(a, 0, 0.0, a, a, a, 1 << 20, None) == L.RPN_ERR_INVALID
        assert lib.rpn_grad_sq_norm(a, 8, -1.0, a, a, a, 1 << 20, None) == L.RPN_ERR_INVALID
        assert lib.rpn_grad_sq_norm(L.vp(4100), 8, 0.0, a, a, a, 1 << 20, None) == L.RPN_ERR_INVALID
        assert lib.rpn_grad_sq_norm(a, 8, 0.0, a, a, a, 4, None) == L.RPN_ERR_WORKSPACE
        args = lambda kind=SGD, n=8, ranges=None, nr=0, t=1, mu=0.9: (kind, a, a, a, a, n, ranges, nr, t, 1e-3, 0.9, 0.999, 1e-7, mu, 0, 5e-4, None, None)
        assert lib.rpn_optimizer_apply(*args(kind=2)) == L.RPN_ERR_INVALID
        assert lib.rpn_optimizer_apply(*args(mu=1.0)) == L.RPN_ERR_INVALID
        assert lib.rpn_optimizer_apply(*args(t=0)) == L.RPN_ERR_INVALID
        assert lib.rpn_optimizer_apply(*args(ranges=None, nr=1)) == L.RPN_ERR_INVALID
        assert lib.rpn_optimizer_apply(*args(ranges=L.vp(4104), nr=1)) == L.RPN_ERR_INVALID           # not 16-byte aligned
    finally:
        lib.rpn_det_head_destroy(h)


def test_compile_arguments(lib):
    hp = bo.get_hyper_params("vgg16", img_size=224, feature_map_shape=14)
    model = RPNModel("vgg16", hp, max_batch=2)
    w = synthetic_weights("vgg16", hp, seed=1)
    for name in HEAD_LAYERS:                                 # (the Python side only: compiling again reads the trainer's weights back)
        model._head[name] = (w[name]["kernel"], w[name]["bias"])
    head = DetectionHead(3, pooling_size=(2, 2), channels=8, hidden=(16, 12), max_rois=10, seed=None)
    for obj in (model, head):
        for bad in (dict(optimizer="rmsprop"), dict(momentum=1.0), dict(global_clipnorm=-1), dict(weight_decay=-1e-4),
                    dict(weight_decay=float("nan")), dict(learning_rate=float("nan"))):
            with pytest.raises(ValueError):
                obj.compile(**bad)
        obj.compile()
        assert obj.optimizer == "adam" and obj.learning_rate == (1e-5 if obj is model else 1e-4)
        obj.compile(learning_rate=lambda t: 1e-3 if t < 2 else 1e-4, optimizer="sgd", momentum=0.9, nesterov=True, weight_decay=5e-4,
                    global_clipnorm=10.0)
        assert obj.optimizer == "sgd" and obj.learning_rate == 1e-3 and obj.train_steps() == 0
        obj.learning_rate = 0.5
        assert obj.learning_rate == 0.5
        with pytest.raises(ValueError):
            obj.learning_rate = -1.0
        with pytest.raises(ValueError):
            obj.set_optimizer_state({"optimizer": "adam", "steps": 0, "slots": {}})       # the other rule's
        with pytest.raises(ValueError):
            obj.set_optimizer_state({"optimizer": "sgd", "steps": 0, "slots": {"fc9": {}}})   # another layer set
    with pytest.raises(ValueError):
        DetectionHead(3, pooling_size=(2, 2), channels=8, hidden=(16, 12), max_rois=10, trainable=False, seed=None).compile(optimizer="sgd")


def test_new_kernels_register_budget(lib):
    tab = codeobj.table(L.LIB_PATH)
    for name in NEW_KERNELS:
        assert name in tab, name
        _v, _ss, vspill, scratch, _lds, wg = tab[name]
        assert vspill == 0 and scratch == 0 and wg == 256, (name, tab[name])
    assert "adam_kernel" in tab


# ---- the decayed ranges: host arithmetic against the documented layouts -------------------------------------------------------------------
VGG = [("block1_conv1", 3, 64), ("block1_conv2", 64, 64), ("block2_conv1", 64, 128), ("block2_conv2", 128, 128), ("block3_conv1", 128, 256),
       ("block3_conv2", 256, 256), ("block3_conv3", 256, 256), ("block4_conv1", 256, 512), ("block4_conv2", 512, 512), ("block4_conv3", 512, 512),
       ("block5_conv1", 512, 512), ("block5_conv2", 512, 512), ("block5_conv3", 512, 512)]


def expected_mask(segments):
    """segments: (floats, decayed, align) in layout order -> the boolean mask over the flat buffer"""
    parts = []
    n = 0
    for size, decayed, align in segments:
        pad = -n % align
        parts += [np.zeros(pad, bool), np.full(size, decayed)]
        n += pad + size
    return np.concatenate(parts)


def rpn_head_segments(cin, K):
    # rpn_conv kernel | bias | the fused head matrix (512, 5K) | its bias row (5K)
    return [(9 * cin * 512, True, 1), (512, False, 1), (512 * 5 * K, True, 1), (5 * K, False, 1)]


def check_ranges(ranges, mask, kernels):
    assert ranges.ndim == 2 and ranges.shape[1] == 2 and len(ranges) >= 1
    assert np.all(ranges[:, 0] < ranges[:, 1]) and np.all(ranges[1:, 0] >= ranges[:-1, 1]) and ranges[-1, 1] <= len(mask)
    got = decay_mask(len(mask), ranges)
    assert np.array_equal(got, mask)
    assert int(got.sum()) == kernels


def test_decay_ranges_vgg16_head_only(lib):
    m, hp = _trainer(lib)
    K = hp["anchor_count"]
    check_ranges(m.decay_ranges(), expected_mask(rpn_head_segments(512, K)), 9 * 512 * 512 + 512 * 5 * K)
    assert len(m.decay_ranges()) == 2                      # the fused head's bias row (the last 5K floats) is outside both


def test_decay_ranges_vgg16_from_block5_conv1(lib):
    m, hp = _trainer(lib, train_from="block5_conv1")
    K = hp["anchor_count"]
    seg = rpn_head_segments(512, K)
    for _name, cin, cout in VGG[10:]:
        seg += [(9 * cin * cout, True, 1), (cout, False, 1)]
    check_ranges(m.decay_ranges(), expected_mask(seg), 9 * 512 * 512 + 512 * 5 * K + 3 * 9 * 512 * 512)
    assert len(m.decay_ranges()) == 5


def test_decay_ranges_mobilenet_from_block_13_expand(lib):
    m, hp = _trainer(lib, backbone="mobilenet_v2", train_from="block_13_expand")
    K = hp["anchor_count"]
    # a trained MobileNetV2 conv: kernel at a multiple of 4 floats | gamma | beta
    seg = rpn_head_segments(576, K) + [(96 * 576, True, 4), (576, False, 1), (576, False, 1)]
    mask = expected_mask(seg)
    check_ranges(m.decay_ranges(), mask, 9 * 576 * 512 + 512 * 5 * K + 96 * 576)
    assert (9 * 576 * 512 + 512 + 513 * 5 * K) % 4 != 0 or K % 4 == 0      # (with K = 9 the kernel sits behind an alignment gap)


def test_decay_ranges_detection_head_padded_pair(lib):
    head = DetectionHead(21, pooling_size=(2, 2), channels=8, hidden=(16, 12), max_rois=10, seed=None)
    k1, h1, h2, C, npad = 32, 16, 12, 21, 108
    seg = [(k1 * h1, True, 1), (h1, False, 1), (h1 * h2, True, 1), (h2, False, 1)]
    for _ in range(h2):
        seg += [(5 * C, True, 1), (npad - 5 * C, False, 1)]            # 105 real columns, 3 of padding
    seg += [(npad, False, 1)]
    check_ranges(head.decay_ranges(), expected_mask(seg), k1 * h1 + h1 * h2 + h2 * 5 * C)
    # an unpadded pair (C = 4: 20 columns) is one range
    head4 = DetectionHead(4, pooling_size=(2, 2), channels=8, hidden=(16, 12), max_rois=10, seed=None)
    assert len(head4.decay_ranges()) == 3
