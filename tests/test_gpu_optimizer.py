"""GPU suite for the optimizers (include/rpn_hip.h, "Optimizers"): the norm and update kernels on caller buffers, then through both
handles -- RPNModel's trainer and DetectionHead -- with resume, a learning-rate schedule and the f16x3 head.  The restatements and
their bounds are in tests/test_optimizer_host.py.

Sizes: n in {1, 255, 256, 257, 1000, 65 537} (one thread, a partial float4, one full workgroup, one element into the second, a size
that is no multiple of anything, many workgroups below the grid cap) and SWEEP + 5 = 2 097 157: one full sweep of the capped grid
(2048 workgroups x 256 threads x 4 floats) plus a float4 and a partial one, so that the grid-stride loop's second trip, the cap and
the tail all run."""
import math
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import test_train as tt  # noqa: E402
from test_optimizer_host import ADAM, F32, SGD, SWEEP, adam64_extras, clip_scale, decay_mask, sgd32, sgd64  # noqa: E402
from test_train import lib  # noqa: E402,F401  (fixture)
from oracle import bbox_oracle as bo  # noqa: E402
from tf_rpn_amd import _lib as L  # noqa: E402
from tf_rpn_amd.models._rpn_model import HEAD_LAYERS, RPNModel, synthetic_weights  # noqa: E402
from tf_rpn_amd.models.detection_head import DetectionHead  # noqa: E402

pytestmark = pytest.mark.gpu
NS = [1, 255, 256, 257, 1000, 65537, SWEEP + 5]


def cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def ranges_for(n):
    """two decayed ranges whose four ends are all off a 4-element boundary (one range where n is too small for two)"""
    if n < 64:
        return [(0, n)]
    off = lambda v: v + (1 if v % 4 == 0 else 0)
    return [(3, off(n // 3)), (off(n // 2 + 1), off(n - 6))]


# ---- 1. the norm ------------------------------------------------------------------------------------------------------------------------
def grad_sq_norm(lib, g, C):
    n = g.numel()
    ws_bytes = lib.rpn_grad_sq_norm_workspace_bytes(n)
    ws = torch.empty((ws_bytes // 8,), dtype=torch.float64, device="cuda")
    S = torch.zeros((1,), dtype=torch.float64, device="cuda")
    c = torch.zeros((1,), dtype=torch.float32, device="cuda")
    L.check(lib.rpn_grad_sq_norm(L.ptr(g), n, float(C), L.ptr(S), L.ptr(c), L.ptr(ws), ws_bytes, L.stream_ptr()), "rpn_grad_sq_norm")
    return S.cpu().numpy()[0], c.cpu().numpy()[0]


@pytest.mark.parametrize("mag", [1e-4, 1.0, 1e4])
@pytest.mark.parametrize("n", NS)
def test_norm(lib, n, mag):
    rng = np.random.RandomState(n % 1000 + 7)
    g = (rng.standard_normal(n) * mag).astype(np.float32)
    ref = math.fsum((g.astype(np.float64) ** 2).tolist())           # the squares are exact in float64
    d = cuda(g)
    S, c = grad_sq_norm(lib, d, 0.0)
    print("n %d mag %g: S %r, fsum %r, rel %.3g (bound %.3g)" % (n, mag, S, ref, abs(S - ref) / ref, n * 2.0 ** -53))
    assert abs(S - ref) <= n * 2.0 ** -53 * ref
    assert c == 1.0
    for C in (0.5 * math.sqrt(ref), 2.0 * math.sqrt(ref)):
        S2, c2 = grad_sq_norm(lib, d, C)
        assert S2.tobytes() == S.tobytes()                          # two calls: identical bytes
        assert c2.tobytes() == clip_scale(S, C).tobytes(), (C, c2)
        assert (c2 == 1.0) == (np.sqrt(S) <= np.float64(F32(C)))
    bad = g.copy()
    bad[n // 2] = np.nan
    S3, c3 = grad_sq_norm(lib, cuda(bad), 1.0)
    assert np.isnan(S3) and np.isnan(c3)


# ---- 2. / 3. the update on caller buffers ---------------------------------------------------------------------------------------------
def apply(lib, kind, w, g, m, v, t, ranges=(), lr=1e-2, mu=0.0, nesterov=False, wd=0.0, scale=None, b1=0.9, b2=0.999, eps=1e-7):
    table = cuda(np.asarray(ranges, np.int64)) if len(ranges) else None
    L.check(lib.rpn_optimizer_apply(kind, L.ptr(w), L.ptr(g), L.ptr(m), L.ptr(v), w.numel(), L.ptr(table), len(ranges), t, lr, b1, b2, eps, mu,
                                    int(nesterov), wd, L.ptr(scale), L.stream_ptr()), "rpn_optimizer_apply")


SGD_CONFIGS = [(0.0, False, 0.0, None), (0.9, False, 5e-4, 0.37), (0.9, True, 5e-4, None), (0.0, True, 5e-4, 0.5), (0.9, False, 0.0, 0.25)]


@pytest.mark.parametrize("n", NS)
def test_sgd_is_bit_exact(lib, n):
    rng = np.random.RandomState(n % 1000 + 11)
    ranges = ranges_for(n)
    mask = decay_mask(n, ranges)
    w0 = rng.standard_normal(n).astype(np.float32)
    gs = [rng.standard_normal(n).astype(np.float32) for _ in range(3)]
    sentinel = rng.standard_normal(n).astype(np.float32)
    for mu, nesterov, wd, scale in SGD_CONFIGS:
        runs = {}
        for decay in ((wd, 0.0) if wd else (wd,)):
            w, a, v = cuda(w0), torch.zeros(n, device="cuda"), cuda(sentinel)
            sc = cuda(np.array([scale], np.float32)) if scale is not None else None
            wr, ar = w0.copy(), np.zeros(n, np.float32)
            for t in (1, 2, 3):
                apply(lib, SGD, w, cuda(gs[t - 1]), a, v, t, ranges if decay else (), mu=mu, nesterov=nesterov, wd=decay, scale=sc)
                wr, ar = sgd32(wr, gs[t - 1], ar, 1e-2, mu, nesterov, decay, mask, scale)
                assert w.cpu().numpy().tobytes() == wr.tobytes(), (n, mu, nesterov, decay, scale, t)
                assert a.cpu().numpy().tobytes() == ar.tobytes(), (n, mu, nesterov, decay, scale, t)
            assert v.cpu().numpy().tobytes() == sentinel.tobytes()                    # v is not touched
            runs[decay] = w.cpu().numpy()
        if wd:
            assert np.array_equal(runs[wd][~mask], runs[0.0][~mask])                  # outside the ranges: the no-decay bytes
            assert not np.array_equal(runs[wd][mask], runs[0.0][mask])


@pytest.mark.parametrize("n", NS)
def test_adam_with_decay_and_scale(lib, n):
    rng = np.random.RandomState(n % 1000 + 13)
    ranges = ranges_for(n)
    mask = decay_mask(n, ranges)
    w0 = rng.standard_normal(n).astype(np.float32)
    gs = [rng.standard_normal(n).astype(np.float32) for _ in range(3)]
    lr, wd, scale = 1e-3, 5e-4, 0.37
    w, m, v = cuda(w0), torch.zeros(n, device="cuda"), torch.zeros(n, device="cuda")
    sc = cuda(np.array([scale], np.float32))
    w64, m64, v64 = w0.astype(np.float64), np.zeros(n), np.zeros(n)
    for t in (1, 2, 3):
        apply(lib, ADAM, w, cuda(gs[t - 1]), m, v, t, ranges, lr=lr, wd=wd, scale=sc)
        w64, m64, v64 = adam64_extras(w64, gs[t - 1], m64, v64, t, float(F32(lr)), wd, mask, scale, eps=float(F32(1e-7)),
                                      b1=float(F32(0.9)), b2=float(F32(0.999)))
    err = np.abs(w.cpu().numpy() - w64).max()
    print("n %d: |w - w64| %.3g, bar %.3g" % (n, err, 1e-6 * np.abs(w64).max()))
    assert err <= 1e-6 * np.abs(w64).max()
    # no decay and a scale buffer holding 1.0 = today's launch, byte for byte (reached with no ranges and no scale)
    one = cuda(np.array([1.0], np.float32))
    state = {}
    for key, kw in (("new", dict(scale=one)), ("adam_kernel", dict())):
        w, m, v = cuda(w0), torch.zeros(n, device="cuda"), torch.zeros(n, device="cuda")
        for t in (1, 2, 3):
            apply(lib, ADAM, w, cuda(gs[t - 1]), m, v, t, lr=lr, **kw)
        state[key] = [x.cpu().numpy().tobytes() for x in (w, m, v)]
    assert state["new"] == state["adam_kernel"]


# ---- 4. .. 7. through the handles ---------------------------------------------------------------------------------------------------------
IMG_MN = 80


@pytest.fixture(scope="module")
def vgg(lib):
    hp = bo.get_hyper_params("vgg16", img_size=224, feature_map_shape=14)
    model = tt.make_model("vgg16", hp, 2)
    imgs, deltas, labels = tt.batch(hp, 2, seed=31)
    return dict(hp=hp, model=model, w0=synthetic_weights("vgg16", hp, seed=1), x=imgs, y=(deltas, labels))


@pytest.fixture(scope="module")
def mnv2(lib):
    hp = bo.get_hyper_params("mobilenet_v2", img_size=IMG_MN, feature_map_shape=(IMG_MN + 15) // 16)
    w0 = synthetic_weights("mobilenet_v2", hp, seed=3)
    model = RPNModel("mobilenet_v2", hp, precision="f32", max_batch=2)
    model.set_weights(w0)
    imgs, deltas, labels = tt.batch(hp, 2, seed=33)
    return dict(hp=hp, model=model, w0=w0, x=imgs, y=(deltas, labels))


def fresh(case, **compile_kw):
    m = case["model"]
    m.set_weights(case["w0"])
    m.compile(**compile_kw)
    return m


HEAD_KW = dict(pooling_size=(2, 2), channels=8, hidden=(16, 12), max_rois=10)


@pytest.fixture(scope="module")
def head_batch():
    rng = np.random.RandomState(41)
    return dict(pooled=cuda(rng.standard_normal((2, 5, 2, 2, 8)).astype(np.float32)), gl=cuda(rng.standard_normal((2, 5, 3)).astype(np.float32)),
                gd=cuda(rng.standard_normal((2, 5, 12)).astype(np.float32)))


def head_step(head, hb):
    logits, deltas = head(hb["pooled"])
    ((logits * hb["gl"]).sum() + (deltas * hb["gd"]).sum()).backward()
    head.apply_gradients()


def flat64(d):
    return {(n, k): np.asarray(v, np.float64) for n, e in d.items() for k, v in e.items() if k in ("kernel", "bias", "gamma", "beta")}


def norm64(grads):
    sq = []
    n = 0
    for v in flat64(grads).values():
        sq += (v.ravel() ** 2).tolist()
        n += v.size
    return math.sqrt(math.fsum(sq)), n


def replay_sgd64(step, get_weights, get_gradients, grad_norm, lr, mu, wd, steps=3):
    """the steps on the device, sgd64 beside them from get_gradients() and the reported scale -> the worst |w - w64| / max |w64|"""
    w64 = flat64(get_weights())
    a64 = {k: np.zeros_like(v) for k, v in w64.items()}
    worst = 0.0
    for _ in range(steps):
        step()
        g, scale = flat64(get_gradients()), grad_norm()["scale"]
        for k in w64:
            mask = np.full(w64[k].shape, k[1] == "kernel")             # kernels are decayed, biases are not
            w64[k], a64[k] = sgd64(w64[k], g[k], a64[k], lr, mu, False, wd, mask, scale)
        got = flat64(get_weights())
        for k in w64:
            worst = max(worst, np.abs(got[k] - w64[k]).max() / np.abs(w64[k]).max())
    return worst


def test_vgg_head_sgd_with_decay_and_clip_tracks_sgd64(lib, vgg):
    lr, mu, wd = 1e-3, 0.9, 5e-4
    m = fresh(vgg, learning_rate=lr, optimizer="sgd", momentum=mu, weight_decay=wd, global_clipnorm=0.05)
    worst = replay_sgd64(lambda: m.train_on_batch(vgg["x"], vgg["y"]), m.get_weights, m.get_gradients, m.grad_norm, lr, mu, wd)
    gn = m.grad_norm()
    print("vgg16 head, SGD + decay + clip: worst %.3g (bar 1e-6), norm %.6g, scale %.6g" % (worst, gn["norm"], gn["scale"]))
    assert worst <= 1e-6
    assert gn["scale"] == float(clip_scale(gn["norm"] ** 2, 0.05)) or abs(gn["scale"] - min(1.0, 0.05 / gn["norm"])) <= 1e-6 * gn["scale"]


def test_det_head_sgd_with_decay_and_clip_tracks_sgd64(lib, head_batch):
    lr, mu, wd = 1e-2, 0.9, 5e-4
    head = DetectionHead(3, seed=5, **HEAD_KW)
    head.compile(learning_rate=lr, optimizer="sgd", momentum=mu, weight_decay=wd, global_clipnorm=0.5)
    worst = replay_sgd64(lambda: head_step(head, head_batch), head.get_weights, head.get_gradients, head.grad_norm, lr, mu, wd)
    gn = head.grad_norm()
    print("detection head, SGD + decay + clip: worst %.3g (bar 1e-6), norm %.6g, scale %.6g" % (worst, gn["norm"], gn["scale"]))
    assert worst <= 1e-6
    assert abs(gn["scale"] - min(1.0, 0.5 / gn["norm"])) <= 1e-6 * gn["scale"]


@pytest.mark.parametrize("which", ["vgg16_head", "vgg16_block5_conv1", "mobilenet_block_13_expand"])
def test_grad_norm_is_the_norm_of_get_gradients(lib, vgg, mnv2, which):
    case, kw = {"vgg16_head": (vgg, {}), "vgg16_block5_conv1": (vgg, dict(train_backbone_from="block5_conv1")),
                "mobilenet_block_13_expand": (mnv2, dict(train_backbone_from="block_13_expand"))}[which]
    m = fresh(case, optimizer="sgd", global_clipnorm=1e30, learning_rate=1e-4, **kw)
    m.train_on_batch(case["x"], case["y"])
    ref, n = norm64(m.get_gradients())
    gn = m.grad_norm()
    print("%s: norm %r, float64 of get_gradients %r over %d elements" % (which, gn["norm"], ref, n))
    assert gn["scale"] == 1.0
    assert abs(gn["norm"] - ref) <= n * 2.0 ** -53 * ref             # the gaps and the padding contribute nothing


def weights_bytes(w):
    return {k: v.tobytes() for k, v in flat64(w).items()}


@pytest.mark.parametrize("optimizer", ["adam", "sgd"])
def test_huge_clipnorm_changes_no_bit(lib, vgg, head_batch, optimizer):
    kw = dict(optimizer=optimizer, momentum=0.9 if optimizer == "sgd" else 0.0, learning_rate=1e-3)
    got = []
    for clip in (None, 1e30):
        m = fresh(vgg, global_clipnorm=clip, **kw)
        for _ in range(2):
            m.train_on_batch(vgg["x"], vgg["y"])
        got.append(weights_bytes(m.get_weights()))
        head = DetectionHead(3, seed=5, **HEAD_KW)
        head.compile(global_clipnorm=clip, **kw)
        for _ in range(2):
            head_step(head, head_batch)
        got.append(weights_bytes(head.get_weights()))
    assert got[0] == got[2] and got[1] == got[3]


def test_adam_defaults_are_todays_step(lib, vgg):
    got = []
    for kw in ({}, dict(optimizer="adam", momentum=0.0, nesterov=False, weight_decay=0.0, global_clipnorm=None)):
        m = fresh(vgg, learning_rate=1e-3, **kw)
        for _ in range(2):
            m.train_on_batch(vgg["x"], vgg["y"])
        got.append((weights_bytes(m.get_weights()), {e: {p: {s: a.tobytes() for s, a in sl.items()} for p, sl in d.items()}
                                                      for e, d in m.get_optimizer_state()["slots"].items()}))
    assert got[0] == got[1]
    with pytest.raises(ValueError):
        m.grad_norm()                                                  # no clip norm configured


def test_clip_to_a_tenth_of_the_norm(lib, vgg):
    lr = 1e-3
    m = fresh(vgg, optimizer="sgd", global_clipnorm=1e30, learning_rate=0.0)
    m.train_on_batch(vgg["x"], vgg["y"])                              # lr 0: the weights stay, the norm is measured
    norm = m.grad_norm()["norm"]
    m.compile(optimizer="sgd", global_clipnorm=norm / 10, learning_rate=lr)
    before = m.get_weights()
    m.train_on_batch(vgg["x"], vgg["y"])
    gn, g, after, state = m.grad_norm(), m.get_gradients(), m.get_weights(), m.get_optimizer_state()
    print("norm %.6g, clip norm %.6g, scale %.9g" % (gn["norm"], norm / 10, gn["scale"]))
    assert gn["norm"] == norm and abs(gn["scale"] - 0.1) <= 1e-6
    for name in HEAD_LAYERS:
        for p in ("kernel", "bias"):
            update = -(F32(lr) * (g[name][p] * F32(gn["scale"])))
            # (value for value: the kernel's 0 * a - step and this -step differ in the sign of a zero, and in nothing else)
            assert np.array_equal(state["slots"][name][p]["m"], update), (name, p)
            assert np.array_equal(after[name][p], before[name][p] + update), (name, p)


def slots_bytes(state):
    return {(e, p, s): a.tobytes() for e, d in state["slots"].items() for p, sl in d.items() for s, a in sl.items()}


OPT_KW = {"adam": dict(optimizer="adam", learning_rate=1e-3), "sgd": dict(optimizer="sgd", momentum=0.9, learning_rate=1e-3)}


@pytest.mark.parametrize("optimizer", ["adam", "sgd"])
@pytest.mark.parametrize("which", ["vgg16_head", "mobilenet_block_13_expand"])
def test_resume_rpn_model(lib, vgg, mnv2, tmp_path, which, optimizer):
    case, kw = (vgg, {}) if which == "vgg16_head" else (mnv2, dict(train_backbone_from="block_13_expand"))
    kw = dict(kw, **OPT_KW[optimizer])
    step = lambda m: m.train_on_batch(case["x"], case["y"])
    a = fresh(case, **kw)
    for _ in range(4):
        step(a)
    final = (weights_bytes(a.get_weights()), slots_bytes(a.get_optimizer_state()), a.train_steps())
    b = fresh(case, **kw)
    for _ in range(2):
        step(b)
    wpath, opath = str(tmp_path / "w.npz"), str(tmp_path / "opt.npz")
    RPNModel.save_weights(b.get_weights(), wpath)
    b.save_optimizer_state(opath)
    results = []
    for load_state in (True, False):
        c = RPNModel(case["model"].backbone, case["hp"], precision="f32", max_batch=2)     # a fresh object
        c.set_weights(case["w0"])
        c.load_weights(wpath)
        c.compile(**kw)
        if load_state:
            c.load_optimizer_state(opath)
            assert c.train_steps() == 2
        for _ in range(2):
            step(c)
        results.append((weights_bytes(c.get_weights()), slots_bytes(c.get_optimizer_state()), c.train_steps()))
    assert results[0] == final
    assert results[1][0] != final[0] and results[1][2] == 2                # without the state the run is another one


@pytest.mark.parametrize("optimizer", ["adam", "sgd"])
def test_resume_detection_head(lib, head_batch, tmp_path, optimizer):
    kw = OPT_KW[optimizer]
    a = DetectionHead(3, seed=5, **HEAD_KW)
    a.compile(**kw)
    for _ in range(4):
        head_step(a, head_batch)
    final = (weights_bytes(a.get_weights()), slots_bytes(a.get_optimizer_state()), a.train_steps())
    b = DetectionHead(3, seed=5, **HEAD_KW)
    b.compile(**kw)
    for _ in range(2):
        head_step(b, head_batch)
    wpath, opath = str(tmp_path / "w.npz"), str(tmp_path / "opt.npz")
    b.save_weights(wpath)
    b.save_optimizer_state(opath)
    results = []
    for load_state in (True, False):
        c = DetectionHead(3, seed=None, **HEAD_KW)
        c.load_weights(wpath)
        c.compile(**kw)
        if load_state:
            c.load_optimizer_state(opath)
            assert c.train_steps() == 2
        for _ in range(2):
            head_step(c, head_batch)
        results.append((weights_bytes(c.get_weights()), slots_bytes(c.get_optimizer_state()), c.train_steps()))
    assert results[0] == final
    assert results[1][0] != final[0] and results[1][2] == 2
    with pytest.raises(ValueError):                                        # the other rule's state
        other = DetectionHead(3, seed=5, **HEAD_KW)
        other.compile(**OPT_KW["sgd" if optimizer == "adam" else "adam"])
        other.load_optimizer_state(opath)


def test_learning_rate_schedule(lib, vgg):
    sched = lambda t: 1e-3 if t < 2 else 1e-4
    m = fresh(vgg, optimizer="sgd", learning_rate=sched)
    for t in range(3):
        assert m.learning_rate == sched(t) and m.train_steps() == t
        before = m.get_weights()
        m.train_on_batch(vgg["x"], vgg["y"])
        g, after, state = m.get_gradients(), m.get_weights(), m.get_optimizer_state()
        for name in HEAD_LAYERS:
            for p in ("kernel", "bias"):
                update = -(F32(sched(t)) * g[name][p])
                assert np.array_equal(state["slots"][name][p]["m"], update), (t, name, p)        # (value for value, as above)
                assert np.array_equal(after[name][p], before[name][p] + update), (t, name, p)
    assert m.learning_rate == 1e-4
    m.learning_rate = 5e-4
    assert m.learning_rate == 5e-4


def test_f16x3_head_under_sgd_refreshes_its_image(lib, head_batch):
    head = DetectionHead(3, seed=5, **HEAD_KW)
    head.compile(precision="f16x3", optimizer="sgd", momentum=0.9, weight_decay=5e-4, global_clipnorm=0.5, learning_rate=1e-2)
    for _ in range(2):
        head_step(head, head_batch)
    with torch.no_grad():
        got = head(head_batch["pooled"])
    ref = head.inference_copy(precision="f16x3")(head_batch["pooled"])
    for x, y in zip(got, ref):
        assert x.cpu().numpy().tobytes() == y.cpu().numpy().tobytes()
    assert not head.status()["f16_range"]
