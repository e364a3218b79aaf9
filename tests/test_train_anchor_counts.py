"""Training of the RPN head at every anchor count the trainer accepts (5K <= 64: K = 1 .. 12), beside tests/test_train.py which
runs K = 9 only.  head_wgrad_kernel<NC> / head_dgrad_kernel<NC> are instantiated per NC = 5K, and the trainer's flat parameter buffer
places rpn_cls at column 4K of the fused (512, 5K) head matrix: the gradients of all three head layers against torch float64
autograd on the library's own feature tap (the rpn_conv kernel gradient is what covers head_dgrad), a five-step Adam replay whose
trained head then runs in inference, bit determinism, and the refusal of K = 13.

Targets are synthetic arrays of the shapes calculate_rpn_actual_outputs returns (deltas (B, F F K, 4), labels (B, F, F, K) in
{1, 0, -1}); the conditions on them and on the float64 reference are asserted in `case`, never on the library's output.
"""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

from oracle import bbox_oracle as bo  # noqa: E402
from oracle import conv_oracle as cv  # noqa: E402
from test_train import adam64, cls_loss64, head64, lib, make_model, reg_loss64  # noqa: E402,F401  (lib: fixture)
from tf_rpn_amd.models._rpn_model import HEAD_LAYERS, RPNModel  # noqa: E402

# anchor tables (ratios x scales) whose product is K = 1 .. 12
TABLES = {1: (1, 1), 2: (2, 1), 3: (3, 1), 4: (2, 2), 5: (5, 1), 6: (3, 2), 7: (7, 1), 8: (4, 2), 9: (3, 3), 10: (5, 2), 11: (11, 1),
          12: (4, 3)}
IMG, F = 80, 5


def hyper(backbone, K):
    nr, ns = TABLES[K]
    hp = bo.get_hyper_params(backbone, img_size=IMG, feature_map_shape=F, anchor_ratios=[0.5 + 0.25 * i for i in range(nr)],
                             anchor_scales=[16.0 * (i + 1) for i in range(ns)])
    assert hp["anchor_count"] == K
    return hp


def targets(K, B, seed):
    """Labels 1 / 0 / -1 with probabilities 0.25 / 0.35 / 0.4, one of each forced into every image; deltas N(0, 1) on the positives (a
    few beyond the Huber knee at 1), zero elsewhere."""
    rng = np.random.RandomState(seed)
    A = F * F * K
    labels = rng.choice(np.array([1.0, 0.0, -1.0], np.float32), size=(B, A), p=[0.25, 0.35, 0.4])
    for b in range(B):
        labels[b, rng.permutation(A)[:3]] = [1.0, 0.0, -1.0]
    deltas = (rng.standard_normal((B, A, 4)) * (labels == 1)[..., None]).astype(np.float32)
    for v in (1.0, 0.0, -1.0):
        assert ((labels == v).sum(1) >= 1).all()                # every image has at least one label of each kind
    assert ((deltas != 0).any(-1) == (labels == 1)).all()
    return deltas, labels.reshape(B, F, F, K)


def batch(K, B, seed):
    imgs = np.random.RandomState(seed).uniform(0, 1, size=(B, IMG, IMG, 3)).astype(np.float32)
    return (imgs,) + targets(K, B, seed + 1)


def reference(X, w, K, deltas, labels, float32_reaches=None):
    """float64 head + losses on the tap X -> (params with .grad filled, [total, reg, cls] losses), with the conditions on the
    reference asserted: 10 % .. 90 % of rpn_conv's outputs positive (the ReLU mask of head_dgrad is exercised both ways), and, where
    the losses are held to a relative bound, that float32 can reach it on these inputs: the same head evaluated by torch in float32
    (losses still in float64) lands within `float32_reaches` -- a sigmoid saturated to 1 - 1e-6 would put the rounding of p
    alone above 1e-6 of the loss."""
    params, reg, cls = head64(X, w, K)
    dt, lt = torch.tensor(deltas, dtype=torch.float64), torch.tensor(labels, dtype=torch.float64)
    with torch.no_grad():
        x = torch.tensor(np.asarray(X, np.float64)).permute(0, 3, 1, 2)
        s = torch.nn.functional.conv2d(x, params["rpn_conv"][0].permute(3, 2, 0, 1), params["rpn_conv"][1], padding=1)
        positive = (s > 0).to(torch.float64).mean().item()
    assert 0.1 <= positive <= 0.9, positive
    r, c = reg_loss64(dt, reg), cls_loss64(lt, cls)
    if float32_reaches is not None:
        with torch.no_grad():
            r32, c32 = cv._head(torch.from_numpy(np.asarray(X, np.float32)).permute(0, 3, 1, 2).contiguous(), w, torch.float32)
            r32 = reg_loss64(dt, r32.permute(0, 2, 3, 1).to(torch.float64))
            c32 = cls_loss64(lt, c32.permute(0, 2, 3, 1).to(torch.float64))
        for l32, l64 in ((r32, r), (c32, c), (r32 + c32, r + c)):
            assert abs(l32.item() - l64.item()) <= float32_reaches * abs(l64.item()), (l32.item(), l64.item())
    (r + c).backward()
    return params, [(r + c).item(), r.item(), c.item()]


# ---- CPU --------------------------------------------------------------------------------------------------------------------
def test_trainer_refuses_thirteen_anchors(lib):
    """5K = 65 > 64: no head_wgrad / head_dgrad instantiation.  compile() raises and names the head; the inference model at
    K = 13 is built all the same (it runs in tests/test_gpu_anchor_counts.py)."""
    m = RPNModel("vgg16", {"img_size": IMG, "anchor_count": 13}, max_batch=1)
    assert m.ops()[-1]["kernel"] == "rpn_head_splitk<5>"
    with pytest.raises(ValueError, match=r"unsupported head \(Cin 512, K 13\)"):
        m.compile()
    RPNModel("vgg16", {"img_size": IMG, "anchor_count": 12}, max_batch=1).compile()


def test_targets_hold_their_conditions():
    for K in TABLES:
        for B, seed in ((3, 300 + K), (4, 500 + K)):
            deltas, labels = targets(K, B, seed + 1)
            assert deltas.shape == (B, F * F * K, 4) and labels.shape == (B, F, F, K)


# ---- GPU --------------------------------------------------------------------------------------------------------------------
def _gradients(backbone, K):
    B = 3
    hp = hyper(backbone, K)
    model = make_model(backbone, hp, B)
    w0 = model.get_weights()
    if backbone == "mobilenet_v2":
        # the ReLU6 tap reaches 6: with He-normal rpn_cls the sigmoid saturates (1 - p below 1e-5), where float32 cannot hold p
        # to 1e-6 of the loss.  A quarter of the weights keeps every probability representable (asserted in `reference`)
        w0["rpn_cls"]["kernel"] = (w0["rpn_cls"]["kernel"] * np.float32(0.25)).astype(np.float32)
        model.set_weights(w0, partial=True)
    imgs, deltas, labels = batch(K, B, seed=300 + K)
    model.compile()
    losses = model.train_on_batch(imgs, (deltas, labels))
    grads = model.get_gradients()
    X = model.get_activation(model.tap_layer, batch=B).cpu().numpy()
    params, losses64 = reference(X, w0, K, deltas, labels, float32_reaches=2.5e-7)
    worst = 0.0
    for name in HEAD_LAYERS:
        for i, key in enumerate(("kernel", "bias")):
            g64 = params[name][i].grad.numpy()
            assert np.abs(g64).max() > 0, (name, key)
            assert grads[name][key].shape == g64.shape
            err = np.abs(grads[name][key] - g64).max()
            worst = max(worst, err / np.abs(g64).max())
            assert err <= 2e-5 * np.abs(g64).max(), (name, key, err, np.abs(g64).max())
    rel = [abs(a - b) / abs(b) for a, b in zip(losses, losses64)]
    print("train_anchor_counts %s NC=%d worst gradient error %.3g of max|g64| (bound 2e-5); losses rel %s (bound 1e-6)"
          % (backbone, 5 * K, worst, ["%.3g" % v for v in rel]))
    for got, ref in zip(losses, losses64):                          # the bound of test_train.test_losses_and_output_gradients
        assert abs(got - ref) <= 1e-6 * abs(ref), (losses, losses64)


@pytest.mark.gpu
@pytest.mark.parametrize("K", sorted(TABLES))
def test_head_gradients_at_every_anchor_count(lib, K):
    """VGG16 at img_size 80, three images: head_wgrad_kernel<5K> (one ragged chunk of 75 rows = 64 + 11) and
    head_dgrad_kernel<5K> (five workgroups, the last of 11 rows).  Measured on an MI355X over NC = 5 .. 60 and both backbones: the
    worst gradient entry 6.8e-7 .. 1.3e-6 of max|g64| (bound 2e-5), the losses within 1.2e-7 relative (bound 1e-6)."""
    _gradients("vgg16", K)


@pytest.mark.gpu
@pytest.mark.parametrize("K", [1, 12])
def test_head_gradients_mobilenet_v2(lib, K):
    _gradients("mobilenet_v2", K)


@pytest.mark.gpu
@pytest.mark.parametrize("K", [12, 1])
def test_five_steps_track_a_float64_replay_at_other_anchor_counts(lib, K):
    """test_train.test_five_steps_track_a_float64_replay_and_inference_sees_the_head at K = 12 and K = 1: rpn_cls sits at column 4K
    of the trainer's fused head matrix, Adam walks the flat buffer, and the trained head is copied into the inference handle
    (K = 12: rpn_head_splitk<4>).  Same bounds as there.

    Four images and lr = 1e-4 where that test has two at 1e-3.  With 25 pixels per image a step of 1e-3 on all 2.4 M rpn_conv
    weights overshoots (the float64 loss goes 2.2 -> 4.0 -> 5.4 at K = 1) and Adam's lr g / (|g| + eps) amplifies the gradient's
    rounding until ANY float32 evaluation leaves the bound: torch-CPU float32 running these five steps ends 2.6e-2 of max|w| from the
    float64 replay at K = 1 and 2e-4 at K = 12 (two images, 1e-3).  At 1e-4 on these inputs the float64 loss falls at every step and
    the torch float32 replay stays within 5e-6 of max|w| and 3e-7 of the losses, so the bounds measure the library (measured on an
    MI355X: 8e-6 of max|w| at most, on the rpn_reg kernel, bound 2e-4)."""
    hp = hyper("vgg16", K)
    B, lr = 4, 1e-4
    model = make_model("vgg16", hp, B)
    imgs, deltas, labels = batch(K, B, seed=500 + K)
    w = model.get_weights()
    model.compile(learning_rate=lr)
    losses = [model.train_on_batch(imgs, (deltas, labels)) for _ in range(5)]
    X = model.get_activation(model.tap_layer, batch=B).cpu().numpy()
    w64 = {n: {k: v.astype(np.float64) for k, v in d.items()} for n, d in w.items()}
    mv = {n: {k: (0.0, 0.0) for k in d} for n, d in w64.items()}
    losses64 = []
    for t in range(1, 6):
        params, l64 = reference(X, w64, K, deltas, labels)
        losses64.append(l64)
        for n in HEAD_LAYERS:
            for i, k in enumerate(("kernel", "bias")):
                w64[n][k], m, v = adam64(w64[n][k], params[n][i].grad.numpy(), *mv[n][k], t, lr)
                mv[n][k] = (m, v)
    assert np.allclose(losses, losses64, rtol=1e-4, atol=0), (losses, losses64)
    got = model.get_weights()
    for n in HEAD_LAYERS:
        for k in ("kernel", "bias"):
            assert got[n][k].shape == w64[n][k].shape
            err = np.abs(got[n][k] - w64[n][k]).max() / np.abs(w64[n][k]).max()
            print("train_anchor_counts replay K=%d %s %s: %.3g of max|w| (bound 2e-4)" % (K, n, k, err))
            assert err <= 2e-4, (n, k, err)
    dt, lt = torch.tensor(deltas, dtype=torch.float64), torch.tensor(labels, dtype=torch.float64)
    after, (reg, cls) = model.test_on_batch(imgs, (deltas, labels), return_outputs=True)
    _params, reg64, cls64 = head64(X, w64, K)
    ref_total = (reg_loss64(dt, reg64) + cls_loss64(lt, cls64)).item()
    assert np.isclose(after[0], ref_total, rtol=1e-4)
    assert after[0] < losses64[0][0]
    # inference sees the trained head: f32 within 1e-5, f16x3 within the 1e-4 contract
    assert model.head_launch_info(B)["route"] == "splitk" and model.ops()[-1]["kernel"] == "rpn_head_splitk<%d>" % ((5 * K + 15) // 16)
    pred_reg, pred_cls = model.predict_on_batch(torch.from_numpy(imgs).cuda())
    assert (pred_reg - reg).abs().max().item() <= 1e-5 and (pred_cls - cls).abs().max().item() <= 1e-5
    m16 = make_model("vgg16", hp, B, precision="f16x3")
    m16.compile(learning_rate=lr)
    for _ in range(2):
        m16.train_on_batch(imgs, (deltas, labels))
    _, (reg16, cls16) = m16.test_on_batch(imgs, (deltas, labels), return_outputs=True)
    p_reg, p_cls = m16.predict_on_batch(torch.from_numpy(imgs).cuda())
    assert (p_reg - reg16).abs().max().item() <= 1e-4 and (p_cls - cls16).abs().max().item() <= 1e-4


@pytest.mark.gpu
def test_train_step_is_deterministic_at_twelve_anchors(lib):
    hp = hyper("vgg16", 12)
    model = make_model("vgg16", hp, 3)
    w0 = model.get_weights()
    imgs, deltas, labels = batch(12, 3, seed=700)
    runs = []
    for _ in range(2):
        model.compile()
        model.set_weights(w0, partial=True)
        losses = model.train_on_batch(imgs, (deltas, labels))
        runs.append((losses, model.get_weights(), model.get_gradients()))
    assert runs[0][0] == runs[1][0]
    for n in HEAD_LAYERS:
        for k in ("kernel", "bias"):
            assert np.array_equal(runs[0][1][n][k], runs[1][1][n][k]), (n, k)
            assert np.array_equal(runs[0][2][n][k], runs[1][2][n][k]), (n, k)
