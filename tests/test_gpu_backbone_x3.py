"""The VGG16 backbone's backward in split float16 on the GPU: the two single-layer entries (rpn_conv3x3_dgrad_x3,
rpn_conv3x3_wgrad_wide_x3) against float64 inside the a-priori bounds of tests/test_backbone_x3_host.py, exact cases byte for byte,
the bit identities of the contract, the range flag, a block-boundary chain, and the trainer with backward_precision="f16x3" beside
the float32 one.  Every input, output and workspace sits inside the NaN guard bands of tests/test_gpu_backward.py; the workspace view
is exactly *_workspace_bytes long.
"""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import test_backbone_x3_host as bx  # noqa: E402
import test_det_head_x3_train_host as tr  # noqa: E402
import test_train_backbone as tb  # noqa: E402
from test_gpu_backward import Band, dy_like, he_like, relu_like, settle, workspace  # noqa: E402
from test_gpu_backward import lib  # noqa: E402,F401  (fixture)
from test_train_backbone import dgrad64, maxpool_backward64, wgrad64  # noqa: E402
from tf_rpn_amd import _lib as L  # noqa: E402
from tf_rpn_amd.models._rpn_model import HEAD_LAYERS, VGG16_CONVS, synthetic_weights  # noqa: E402

pytestmark = pytest.mark.gpu
F32, F16X3 = 0, 2


def status_band():
    b = Band(4)
    b.view.view(torch.int32).zero_()
    return b


def flag_of(band):
    return int(band.view.view(torch.int32)[0].item())


def run_dgrad(lib, dy, w, mask=None, add=None, in_place=False, runs=2):
    """-> (dx, status flags); in_place: the addend lives in dx's own buffer (add == dx)"""
    B, H, W, Cout = dy.shape
    Cin = w.shape[2]
    need = lib.rpn_conv3x3_dgrad_x3_workspace_bytes(Cin, Cout)
    bands = {"dy": Band(dy.size, dy), "w": Band(w.size, w)}
    if mask is not None:
        bands["mask"] = Band(mask.size, mask)
    if add is not None and not in_place:
        bands["add"] = Band(add.size, add)
    got = []
    for _ in range(runs):
        bands["ws"], bands["status"] = workspace(need), status_band()
        bands["dx"] = Band(B * H * W * Cin, add if in_place else None)
        addp = None if add is None else (bands["dx"].ptr if in_place else bands["add"].ptr)
        L.check(lib.rpn_conv3x3_dgrad_x3(bands["dy"].ptr, bands["w"].ptr, bands["mask"].ptr if mask is not None else None, addp, B, H, W,
                                         Cin, Cout, bands["dx"].ptr, bands["status"].ptr, bands["ws"].ptr, need, L.stream_ptr()),
                "rpn_conv3x3_dgrad_x3")
        torch.cuda.synchronize()
        for name, band in bands.items():
            assert band.intact(), "the canary around %s changed: a store outside a buffer" % name
        got.append((bands["dx"].numpy((B, H, W, Cin)), flag_of(bands["status"])))
    for later in got[1:]:
        assert later[0].tobytes() == got[0][0].tobytes() and later[1] == got[0][1], "two runs of the same call differ"
    return got[0]


def run_wgrad(lib, x, dy, runs=2):
    """-> (dw, db, status flags)"""
    B, H, W, Cin = x.shape
    Cout = dy.shape[3]
    need = lib.rpn_conv3x3_wgrad_wide_x3_workspace_bytes(B, H, W, Cin, Cout)
    bands = {"x": Band(x.size, x), "dy": Band(dy.size, dy)}
    got = []
    for _ in range(runs):
        bands["ws"], bands["status"] = workspace(need), status_band()
        bands["dw"], bands["db"] = Band(9 * Cin * Cout), Band(Cout)
        L.check(lib.rpn_conv3x3_wgrad_wide_x3(bands["x"].ptr, bands["dy"].ptr, B, H, W, Cin, Cout, bands["dw"].ptr, bands["db"].ptr,
                                              bands["status"].ptr, bands["ws"].ptr, need, L.stream_ptr()), "rpn_conv3x3_wgrad_wide_x3")
        torch.cuda.synchronize()
        for name, band in bands.items():
            assert band.intact(), "the canary around %s changed: a store outside a buffer" % name
        got.append((bands["dw"].numpy((3, 3, Cin, Cout)), bands["db"].numpy((Cout,)), flag_of(bands["status"])))
    for later in got[1:]:
        assert later[0].tobytes() == got[0][0].tobytes() and later[1].tobytes() == got[0][1].tobytes() and later[2] == got[0][2]
    return got[0]


def run_pool_backward(lib, y, dpool):
    B, H, W, C = y.shape
    bands = {"y": Band(y.size, y), "dpool": Band(dpool.size, dpool), "dy_out": Band(y.size)}
    L.check(lib.rpn_maxpool2x2_backward(bands["y"].ptr, bands["dpool"].ptr, B, H, W, C, bands["dy_out"].ptr, L.stream_ptr()),
            "rpn_maxpool2x2_backward")
    settle(bands, ("dy_out",))
    return bands["dy_out"].numpy((B, H, W, C))


def inside(what, got, ref, bound):
    assert not np.isnan(got).any(), "NaN in %s: an element nobody wrote, or a read outside a buffer" % what
    err = np.abs(got.astype(np.float64) - ref)
    worst = float((err / np.maximum(bound, 1e-300)).max())
    print("%-40s worst error / bound %.3f" % (what, worst))
    assert (err <= bound).all(), (what, worst)


# ---- against float64 inside the a-priori bounds ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", bx.DGRAD)
def test_dgrad_lies_inside_the_bound(lib, shape):
    c = bx.dgrad_case(shape)
    for scale in bx.GRAD_SCALES:
        for use_mask, use_add, in_place in ((False, False, False), (True, False, False), (False, True, False), (True, True, True)):
            dy, add, ref, bound = bx.dgrad_reference(c, scale, use_mask, use_add)
            got, flags = run_dgrad(lib, dy, c["w"], c["mask"] if use_mask else None, add, in_place, runs=1)
            inside("dgrad %s %g mask %d add %d" % (shape, scale, use_mask, use_add), got, ref, bound)
            assert flags == 0
            if use_mask:
                assert not got[~(c["mask"] > 0)].any() and not np.signbit(got[~(c["mask"] > 0)]).any()     # exactly +0


@pytest.mark.parametrize("shape", bx.WGRAD)
def test_wgrad_lies_inside_the_bound(lib, shape):
    c = bx.wgrad_case(shape)
    leaves = bx.x3_leaves(lib, *shape)
    for scale in bx.GRAD_SCALES:
        dy = tr.scaled(c["dy"], scale)
        ref_w, ref_b = wgrad64(c["x"].astype(np.float64), dy.astype(np.float64))
        bw, bb = bx.conv_wgrad_bound(c["x"], dy, leaves)
        dw, db, flags = run_wgrad(lib, c["x"], dy, runs=1)
        inside("wgrad dw %s %g (%d leaves)" % (shape, scale, leaves), dw, ref_w, bw)
        inside("wgrad db %s %g" % (shape, scale), db, ref_b, bb)
        assert flags == 0


# ---- exact cases, byte for byte ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", bx.DGRAD)
def test_dgrad_exact_cases_byte_for_byte(lib, shape):
    c = bx.exact_dgrad_case(shape)
    ref = dgrad64(c["dy"].astype(np.float64), c["w"].astype(np.float64))
    for use_mask, use_add, in_place in ((False, False, False), (True, False, False), (True, True, False), (False, True, True)):
        got, flags = run_dgrad(lib, c["dy"], c["w"], c["mask"] if use_mask else None, c["add"] if use_add else None, in_place)
        want = ref + c["add"].astype(np.float64) if use_add else ref          # integers times 2^-5: the float32 sum is exact
        want = np.where(c["mask"] > 0, want, 0.0) if use_mask else want
        assert (got + np.float32(0)).tobytes() == (want.astype(np.float32) + np.float32(0)).tobytes(), (use_mask, use_add, in_place)
        assert flags == 0


@pytest.mark.parametrize("shape", bx.WGRAD)
def test_wgrad_exact_cases_byte_for_byte(lib, shape):
    c = bx.exact_wgrad_case(shape)
    ref_w, ref_b = wgrad64(c["x"].astype(np.float64), c["dy"].astype(np.float64))
    dw, db, flags = run_wgrad(lib, c["x"], c["dy"])
    assert np.array_equal(dw, ref_w.astype(np.float32)) and np.array_equal(db, ref_b.astype(np.float32)) and flags == 0
    assert (dw + np.float32(0)).tobytes() == (ref_w.astype(np.float32) + np.float32(0)).tobytes()


# ---- bit identities ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(2, 7, 13, 20, 48), (3, 31, 17, 132, 80)])
def test_dgrad_of_one_image_equals_its_slice_of_the_batch(lib, shape):
    c = bx.dgrad_case(shape)                 # every image holds the tensor's maximum: the same t alone and in the batch
    full, _ = run_dgrad(lib, c["dy"], c["w"], c["mask"], c["add"], runs=1)
    for b in range(shape[0]):
        one, _ = run_dgrad(lib, c["dy"][b:b + 1], c["w"], c["mask"][b:b + 1], c["add"][b:b + 1], runs=1)
        assert one.tobytes() == full[b:b + 1].tobytes(), b


def test_dgrad_tile_widths_give_the_same_bytes(lib):
    """The library picks ONE tile width per shape, from the shape alone, so two widths of one shape cannot be run through the ABI.
    The closest substitute: a Cin = 128 call (the 128-wide tile) against a separate Cin = 64 call on the first 64 input channels (the
    64-wide tile), which hold max|w| so that both calls find the same s.  They walk the same reduction; the shared channels must
    come out byte for byte."""
    shape = (2, 128, 128, 128, 16)
    c = bx.dgrad_case(shape)
    w = c["w"].copy()
    w[0, 0, 0, 0] = np.abs(w).max() * np.float32(1.25)
    assert lib.rpn_conv3x3_dgrad_x3_tile_n(2, 128, 128, 128) == 128 and lib.rpn_conv3x3_dgrad_x3_tile_n(2, 128, 128, 64) == 64
    wide, _ = run_dgrad(lib, c["dy"], w, runs=1)
    narrow, _ = run_dgrad(lib, c["dy"], np.ascontiguousarray(w[:, :, :64]), runs=1)
    assert np.ascontiguousarray(wide[..., :64]).tobytes() == narrow.tobytes()


@pytest.mark.parametrize("offset", [1, 3])
def test_dgrad_of_an_unaligned_kernel_gives_the_same_bytes(lib, offset):
    """The trainer's master kernels are slices of one flat buffer behind the head's 5 K columns: 4-byte aligned only (offset 1 mod 4
    floats at K = 9).  Such a kernel is scanned and packed with scalar loads; the result is that of the aligned kernel, and the
    floats in front of it (NaN here) are not read."""
    shape = (2, 7, 13, 20, 48)
    c = bx.dgrad_case(shape)
    B, H, W, Cin, Cout = shape
    want, _ = run_dgrad(lib, c["dy"], c["w"], c["mask"], runs=1)
    need = lib.rpn_conv3x3_dgrad_x3_workspace_bytes(Cin, Cout)
    padded = np.concatenate([np.full(offset, np.nan, np.float32), c["w"].reshape(-1), np.full(4 - offset, np.nan, np.float32)])
    bands = {"dy": Band(c["dy"].size, c["dy"]), "w": Band(padded.size, padded), "mask": Band(c["mask"].size, c["mask"]),
             "ws": workspace(need), "status": status_band(), "dx": Band(B * H * W * Cin)}
    wp = L.vp(bands["w"].view.data_ptr() + 4 * offset)
    assert wp.value % 16 == 4 * offset
    L.check(lib.rpn_conv3x3_dgrad_x3(bands["dy"].ptr, wp, bands["mask"].ptr, None, B, H, W, Cin, Cout, bands["dx"].ptr,
                                     bands["status"].ptr, bands["ws"].ptr, need, L.stream_ptr()), "rpn_conv3x3_dgrad_x3")
    settle(bands, ("dx",))
    assert bands["dx"].numpy((B, H, W, Cin)).tobytes() == want.tobytes() and flag_of(bands["status"]) == 0


# ---- range ---------------------------------------------------------------------------------------------------------------------------------
def test_range_flag(lib):
    shape = (1, 3, 5, 4, 16)
    c = bx.dgrad_case(shape)
    rng = np.random.RandomState(5)
    x = relu_like(rng, (1, 3, 5, 4))
    for value, raised in ((65504.0, 0), (65520.0, 1), (np.inf, 1)):
        xv = x.copy()
        xv[0, 1, 2, 1] = value
        assert run_wgrad(lib, xv, c["dy"], runs=1)[2] == raised, value
    for value, raised in ((1e30, 0), (1e-30, 0), (-3e38, 0), (np.inf, 1), (np.nan, 1)):
        dy = c["dy"].copy()
        dy[0, 1, 2, 3] = value
        dw, db, flags = run_wgrad(lib, x, dy, runs=1)
        assert flags == raised, ("wgrad", value)
        dx, dflags = run_dgrad(lib, dy, c["w"], runs=1)
        assert dflags == raised, ("dgrad", value)
        if not raised and abs(value) <= 1e30:        # (3e38 times an activation above 1 leaves float32 in any arithmetic)
            assert np.isfinite(dx).all() and np.isfinite(dw).all()
        if not raised:
            ref = dgrad64(dy.astype(np.float64), c["w"].astype(np.float64))
            assert (np.abs(dx - ref) <= bx.conv_dgrad_bound(dy, c["w"])).all(), value


# ---- a block-boundary chain through the single-layer entries ---------------------------------------------------------------------------------
def test_block_boundary_chain_lies_inside_the_chained_bounds(lib):
    """conv3 -> pool2 -> conv2 as backbone_backward chains them: dgrad without mask, the pool backward (+ the ReLU mask of the pooled
    conv), then the weight gradient and the masked dgrad of conv2, on given activations (the float64 chain routes through the same
    float32 y, so no pool maximum flips); the bounds are chained with edz="""
    B, h, w, H, W, C1, C2, C3 = 1, 24, 32, 48, 64, 8, 16, 32
    rng = np.random.RandomState(3100)
    dy3, w3, w2 = dy_like(rng, (B, h, w, C3)), he_like(rng, C2, C3), he_like(rng, C1, C2)
    y2, x2 = relu_like(rng, (B, H, W, C2)), relu_like(rng, (B, H, W, C1))
    r1 = dgrad64(dy3.astype(np.float64), w3.astype(np.float64))
    e1 = bx.conv_dgrad_bound(dy3, w3, final=False)
    r2, e2 = maxpool_backward64(y2.astype(np.float64), r1), maxpool_backward64(y2.astype(np.float64), e1)
    r_w, r_b = wgrad64(x2.astype(np.float64), r2)
    leaves = bx.x3_leaves(lib, B, H, W, C1, C2)
    e_w, e_b = bx.conv_wgrad_bound(x2, r2, leaves, edy=e2)
    keep = x2 > 0
    r3 = dgrad64(r2, w2.astype(np.float64)) * keep
    e3 = bx.conv_dgrad_bound(r2, w2, edy=e2) * keep

    g1, _ = run_dgrad(lib, dy3, w3, runs=1)
    inside("chain dgrad", g1, r1, 2 * e1)
    g2 = run_pool_backward(lib, y2, g1)
    assert np.array_equal(g2, maxpool_backward64(y2, g1).astype(np.float32))          # the pool step alone is exact
    inside("chain pool", g2, r2, 2 * e2)
    dw, db, flags = run_wgrad(lib, x2, g2, runs=1)
    inside("chain dw", dw, r_w, e_w)
    inside("chain db", db, r_b, e_b)
    g3, dflags = run_dgrad(lib, g2, w2, mask=x2, runs=1)
    inside("chain dgrad 2", g3, r3, e3)
    assert flags == 0 and dflags == 0


# ---- the trainer -----------------------------------------------------------------------------------------------------------------------------
HP = dict(img_size=250, feature_map_shape=15)
B = 2


@pytest.fixture(scope="module")
def steps(lib):
    """one float32 and one f16x3 step of the same weights and batch, and what the later tests compare with"""
    from oracle import bbox_oracle as bo
    hp = bo.get_hyper_params("vgg16", **HP)
    w0 = synthetic_weights("vgg16", hp, seed=1)
    imgs, deltas, labels = tb.batch(hp, B, seed=67)
    out = {"hp": hp, "w0": w0, "batch": (imgs, deltas, labels)}
    for precision in ("f32", "f16x3"):
        model = tb.make_model(hp, B)
        model.compile(train_backbone_from="block1_conv1", backward_precision=precision)
        assert model.backward_precision == precision
        losses = model.train_on_batch(imgs, (deltas, labels))
        out[precision] = dict(model=model, losses=losses, grads=model.get_gradients())
    return out


def same_bytes(a, b, names):
    for n in names:
        for k in ("kernel", "bias"):
            assert a[n][k].tobytes() == b[n][k].tobytes(), (n, k)


def test_trainer_losses_and_head_gradients_are_those_of_the_float32_step(steps):
    f, x = steps["f32"], steps["f16x3"]
    assert np.asarray(f["losses"], np.float32).tobytes() == np.asarray(x["losses"], np.float32).tobytes()
    same_bytes(f["grads"], x["grads"], HEAD_LAYERS)
    assert x["model"].train_status() == {"f16_range": False} and f["model"].train_status() == {"f16_range": False}


def test_trainer_backbone_gradients_wiring(steps):
    """d = max|g_x3 - g_f32| / max|g_f32| <= 2^-10 per backbone layer: a wiring check (a wrong tap, mask, layer or a missing 2^-t /
    2^-s factor gives a d of order 1); the accuracy is held by the single-layer bounds above"""
    f, x = steps["f32"]["grads"], steps["f16x3"]["grads"]
    assert set(x) == set(VGG16_CONVS + HEAD_LAYERS)
    differs = False
    for n in VGG16_CONVS:
        for k in ("kernel", "bias"):
            assert np.isfinite(x[n][k]).all(), (n, k)
            d = np.abs(x[n][k].astype(np.float64) - f[n][k]).max() / np.abs(f[n][k]).max()
            print("backbone %-13s %-6s d = %.3e" % (n, k, d))
            assert d <= 2.0 ** -10, (n, k, d)
            differs = differs or x[n][k].tobytes() != f[n][k].tobytes()
    assert differs                                     # the f16x3 step did run other kernels


def test_trainer_two_f16x3_steps_give_the_same_bytes(steps):
    model, (imgs, deltas, labels) = steps["f16x3"]["model"], steps["batch"]
    model.set_weights(steps["w0"])
    assert model.train_on_batch(imgs, (deltas, labels)) == steps["f16x3"]["losses"]
    same_bytes(model.get_gradients(), steps["f16x3"]["grads"], VGG16_CONVS + HEAD_LAYERS)


def test_trainer_truncated_backward_gives_the_same_bytes(steps):
    imgs, deltas, labels = steps["batch"]
    model = tb.make_model(steps["hp"], B)
    model.compile(train_backbone_from="block4_conv1", backward_precision="f16x3")
    assert model.train_on_batch(imgs, (deltas, labels)) == steps["f16x3"]["losses"]
    g = model.get_gradients()
    assert set(g) == set(VGG16_CONVS[7:] + HEAD_LAYERS)
    same_bytes(g, steps["f16x3"]["grads"], VGG16_CONVS[7:] + HEAD_LAYERS)


def test_trainer_back_to_float32_reproduces_the_float32_step(lib, steps):
    model, (imgs, deltas, labels) = steps["f16x3"]["model"], steps["batch"]
    model.set_weights(steps["w0"])
    t = model.train_steps()
    L.check(lib.rpn_head_trainer_set_backward_precision(model._t, F32), "rpn_head_trainer_set_backward_precision")
    try:
        assert model.backward_precision == "f32" and model.train_steps() == t
        assert model.train_on_batch(imgs, (deltas, labels)) == steps["f32"]["losses"]
        same_bytes(model.get_gradients(), steps["f32"]["grads"], VGG16_CONVS + HEAD_LAYERS)
    finally:
        L.check(lib.rpn_head_trainer_set_backward_precision(model._t, F16X3), "rpn_head_trainer_set_backward_precision")
    assert model.train_status(reset=True) == {"f16_range": False}


def test_trainer_joint_step_differs_only_below_the_tap(steps):
    model, (imgs, deltas, labels) = steps["f16x3"]["model"], steps["batch"]
    model.set_weights(steps["w0"])
    losses, feat, _ = model.forward_for_training(imgs, (deltas, labels))
    rng = np.random.RandomState(9)
    fg = torch.from_numpy((rng.standard_normal(tuple(feat.shape)) * 1e-4).astype(np.float32)).cuda()
    model.apply_gradients(feature_grad=fg)
    torch.cuda.synchronize()
    assert np.asarray(losses.cpu().numpy(), np.float32).tobytes() == np.asarray(steps["f16x3"]["losses"], np.float32).tobytes()
    g = model.get_gradients()
    same_bytes(g, steps["f16x3"]["grads"], HEAD_LAYERS)
    for n in VGG16_CONVS:
        assert np.isfinite(g[n]["kernel"]).all() and g[n]["kernel"].tobytes() != steps["f16x3"]["grads"][n]["kernel"].tobytes(), n
    assert model.train_status() == {"f16_range": False}


def test_fit_in_f16x3_reduces_the_loss(steps):
    from oracle import bbox_oracle as bo
    hp = bo.get_hyper_params("vgg16", **HP)
    imgs, deltas, labels = tb.batch(hp, 2, seed=66)
    model = tb.make_model(hp, 2)
    model.compile(learning_rate=1e-4, train_backbone_from="block1_conv1", backward_precision="f16x3")
    before = model.test_on_batch(imgs, (deltas, labels))[0]
    hist = model.fit(iter([(imgs, (deltas, labels))] * 5), steps_per_epoch=5)
    after = model.test_on_batch(imgs, (deltas, labels))[0]
    assert np.isfinite(hist["loss"][0]) and after < before, (before, after)
    assert model.train_status() == {"f16_range": False}
