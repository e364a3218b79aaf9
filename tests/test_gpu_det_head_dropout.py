"""The detection head's seeded dropout on the GPU (rpn_dropout_forward, rpn_det_head_set_dropout / _dropout_state /
_set_dropout_calls / _get_activation, models.DetectionHead(dropout=...)) against the numpy restatement of
tests/test_det_head_dropout_host.py.

Tolerances (none of them comes from what the kernels give):
  * the mask is integer arithmetic: rpn_dropout_forward, and the zero pattern of the stored activations, are compared exactly;
  * stored activations, logits, deltas, the eight parameter gradients and grad_pooled: elementwise inside `bounds_dropout` of the
    host file -- the bounds of tests/test_det_head_host.py (float32) and tests/test_det_head_x3_host.py /
    tests/test_det_head_x3_train_host.py (f16x3) extended by the two roundings of the scale, derived there; the cases assert on
    the CPU that the ReLU masks of the device and of float64 agree;
  * everything the contract calls identical (a second run, a call number set back, another batch shape, rate 0 against a head
    without the argument, no_grad / detect against a rate-0 head) is compared byte for byte.
"""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import test_det_head_dropout_host as dd  # noqa: E402
import test_det_head_host as dh  # noqa: E402
from test_det_head_host import lib  # noqa: E402,F401  (fixture)
from test_gpu_det_head import inside, loss_gradients, make_head, same_bits  # noqa: E402
from tf_rpn_amd import _lib as L  # noqa: E402
from tf_rpn_amd.models import detection_head  # noqa: E402

pytestmark = pytest.mark.gpu
LAYERS = dh.LAYERS
RATE = dd.RATE
PRECISIONS = ("f32", "f16x3")


def cuda(a):
    return torch.from_numpy(np.array(a)).cuda()


# ---- 1. the stand-alone kernel ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(1, 4), (5, 68), (130, 132), (3, 7)])
def test_dropout_forward_byte_for_byte(lib, shape):
    rng = np.random.RandomState(100 * shape[0] + shape[1])
    x = rng.uniform(-2.0, 2.0, size=shape).astype(np.float32)
    x[rng.uniform(size=shape) < 0.05] = 0.0
    x_d = cuda(x)
    kept_rate, dropped_rate = dd.edge_rates()
    checked = 0
    for rate in (0.5, 0.1, kept_rate, dropped_rate):
        for seed in (3, 0x1234567812345697):
            for layer in (0, 1):
                for calls in (0, 2 ** 32 - 1):
                    got = detection_head.dropout(x_d, rate, seed, calls=calls, layer=layer)
                    ref = dd.dropout_ref(x, rate, seed, calls=calls, layer=layer)
                    assert tuple(got.shape) == shape and same_bits(got, ref), (rate, seed, layer, calls)
                    checked += 1
    assert checked == 32
    assert same_bits(x_d, x)                                     # out of place: the input is untouched
    assert same_bits(detection_head.dropout(x_d, 0.0, 3), x)     # rate 0 keeps every element, times 1
    if shape == (130, 132):
        # the edge of the compare on the device: element (5, 7) of seed 3 is kept at w / 2^32 and dropped at (w + 1) / 2^32
        ones = torch.ones(shape, device="cuda")
        assert float(detection_head.dropout(ones, kept_rate, 3)[5, 7]) == float(dd.scale_of(kept_rate))
        assert float(detection_head.dropout(ones, dropped_rate, 3)[5, 7]) == 0.0
        share = float((detection_head.dropout(ones, 0.5, 3) > 0).float().mean())
        assert 0.45 < share < 0.55


# ---- 2. the head --------------------------------------------------------------------------------------------------------------------------------
def make_drop_head(c, precision="f32", rate=RATE, **kw):
    head = make_head(c, seed=None, dropout=rate, dropout_seed=c["seed"], **kw)
    if precision != "f32":
        head.compile(precision=precision)
    return head


def kept_forward_and_backward(head, c, pooled, gl=None, gd=None):
    """one grad-mode call and its backward -> dict(logits, deltas, a1, a2, gl, gd, grads, grad_pooled)"""
    pooled = pooled.detach().clone().requires_grad_()
    logits, deltas = head(pooled)
    a1, a2 = head.kept_activation("fc1"), head.kept_activation("fc2")
    if gl is None:
        gl, gd = loss_gradients(logits, deltas, c["labels"], c["deltas"])
    torch.autograd.backward([logits, deltas], [gl.reshape(logits.shape), gd.reshape(deltas.shape)])
    return dict(logits=logits.detach(), deltas=deltas.detach(), a1=a1, a2=a2, gl=gl, gd=gd, grads=head.get_gradients(), grad_pooled=pooled.grad)


def same_run(a, b):
    return (same_bits(a["logits"], b["logits"]) and same_bits(a["deltas"], b["deltas"]) and same_bits(a["a1"], b["a1"]) and
            same_bits(a["a2"], b["a2"]) and same_bits(a["grad_pooled"], b["grad_pooled"]) and
            all(same_bits(a["grads"][n][k], b["grads"][n][k]) for n in LAYERS for k in ("kernel", "bias")))


_RUNS = {}


def first_run(index, precision):
    """the first dropped call (t = DROP_CALLS[index]) of a fresh head and its backward, computed once per (case, precision)"""
    if (index, precision) not in _RUNS:
        c = dd.drop_case(index)
        head = make_drop_head(c, precision)
        head.set_dropout(RATE, calls=c["calls"])
        _RUNS[(index, precision)] = kept_forward_and_backward(head, c, cuda(c["pooled"]))
        assert head.dropout_state() == {"rate": RATE, "seed": c["seed"], "calls": c["calls"] + 1}
        assert head.status() == {"f16_range": False}
    return _RUNS[(index, precision)]


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("index", range(len(dh.HEAD_CONFIGS)))
def test_kept_activations(lib, index, precision):
    c = dd.drop_case(index)
    run = first_run(index, precision)
    b = dd.bounds_dropout(c["weights"], c["pooled"], c["masks"], RATE, x3=precision == "f16x3")
    for name, z, keep in (("a1", "z1", c["masks"][0]), ("a2", "z2", c["masks"][1])):
        got = run[name].cpu().numpy()
        zero = ~keep | (c["ref"][z] <= 0)                        # numpy says dropped, or z <= 0
        assert got.dtype == np.float32 and got.shape == zero.shape
        assert not got[zero].view(np.uint32).any()               # exactly +0.0
        assert (got[~zero] > 0).all()
        assert zero.any() and (~zero).any()
        inside(got, c["ref"]["h" + name[1]], b["h" + name[1]], "%s %s" % (precision, name))
    # the zero patterns of the two precisions are identical
    other = first_run(index, PRECISIONS[1 - PRECISIONS.index(precision)])
    assert np.array_equal(run["a1"].cpu().numpy() == 0, other["a1"].cpu().numpy() == 0)
    assert np.array_equal(run["a2"].cpu().numpy() == 0, other["a2"].cpu().numpy() == 0)
    assert not same_bits(run["a1"], other["a1"])                 # ... while the values are each precision's own


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("index", range(len(dh.HEAD_CONFIGS)))
def test_outputs_and_gradients_inside_the_extended_bounds(lib, index, precision):
    c = dd.drop_case(index)
    run = first_run(index, precision)
    gl64, gd64 = run["gl"].cpu().numpy().astype(np.float64), run["gd"].cpu().numpy().astype(np.float64)
    assert np.abs(gl64).max() > 0 and np.abs(gd64).max() > 0
    b = dd.bounds_dropout(c["weights"], c["pooled"], c["masks"], RATE, gl64, gd64, x3=precision == "f16x3")
    ref_g, ref_gp = dd.det_head_backward_ref_dropout(c["weights"], c["pooled"], c["masks"], RATE, gl64, gd64)
    inside(run["logits"], c["ref"]["logits"], b["logits"], "logits")
    inside(run["deltas"], c["ref"]["deltas"], b["deltas"], "deltas")
    for n in LAYERS:
        for k in ("kernel", "bias"):
            assert run["grads"][n][k].dtype == np.float32
            inside(run["grads"][n][k], ref_g[n][k], b[n][k], "%s/%s" % (n, k))
    inside(run["grad_pooled"], ref_gp, b["grad_pooled"], "grad_pooled")
    # the plain (rate 0) restatement is NOT what the device computed: dropout really applied
    plain = dh.head_case(index)["ref"]["logits"]
    assert (np.abs(run["logits"].cpu().numpy() - plain) > b["logits"]).any()


@pytest.mark.parametrize("precision", PRECISIONS)
def test_calls_seeds_and_batch_shapes(lib, precision):
    c = dd.drop_case(0)
    pooled = cuda(c["pooled"])
    first = first_run(0, precision)
    head = make_drop_head(c, precision)
    t0 = c["calls"]
    # the same (seed, calls) twice: the same outputs, activations and gradients
    head.set_dropout(RATE, calls=t0)
    again = kept_forward_and_backward(head, c, pooled, first["gl"], first["gd"])
    assert same_run(again, first) and head.dropout_state()["calls"] == t0 + 1
    # consecutive kept forwards differ, and calls counts exactly them
    second = kept_forward_and_backward(head, c, pooled, first["gl"], first["gd"])
    assert head.dropout_state()["calls"] == t0 + 2
    assert not same_bits(second["a1"], first["a1"]) and not same_bits(second["logits"], first["logits"])
    ref2 = dd.head_masks(c["dims"], RATE, c["seed"], t0 + 1)
    if precision == "f32":                                       # (z1 does not depend on the mask; no z1 lies within its float32 bound of zero)
        assert np.array_equal(second["a1"].cpu().numpy() > 0, ref2[0] & (c["ref"]["z1"] > 0))
    # set_dropout_calls back to an earlier value reproduces that call
    head.set_dropout(RATE, calls=t0 + 1)
    assert same_run(kept_forward_and_backward(head, c, pooled, first["gl"], first["gd"]), second)
    head.set_dropout(RATE, calls=t0)
    assert same_run(kept_forward_and_backward(head, c, pooled, first["gl"], first["gd"]), first)
    # another seed: another mask
    head.set_dropout(RATE, seed=c["seed"] + 1, calls=t0)
    assert not same_bits(kept_forward_and_backward(head, c, pooled, first["gl"], first["gd"])["a1"], first["a1"])
    # rows of a (1, 74) call equal the rows of the (2, 37) call: the mask belongs to the flat row
    head.set_dropout(RATE, seed=c["seed"], calls=t0)
    flat = kept_forward_and_backward(head, c, pooled.reshape((1, 74) + tuple(pooled.shape[2:])), first["gl"].reshape(1, 74, -1),
                                     first["gd"].reshape(1, 74, -1))
    assert same_bits(flat["logits"].reshape(2, 37, -1), first["logits"]) and same_bits(flat["a1"], first["a1"]) and same_bits(flat["a2"], first["a2"])
    assert same_bits(flat["grad_pooled"].reshape(first["grad_pooled"].shape), first["grad_pooled"])
    assert all(same_bits(flat["grads"][n][k], first["grads"][n][k]) for n in LAYERS for k in ("kernel", "bias"))
    # the ABI: get_activation wants the kept forward's row count
    out = torch.empty((74, c["dims"][3]), device="cuda")
    assert lib.rpn_det_head_get_activation(head._h, b"fc1", L.ptr(out), 37, L.stream_ptr()) == L.RPN_ERR_INVALID
    assert lib.rpn_det_head_get_activation(head._h, b"fc1", L.ptr(out), 74, L.stream_ptr()) == L.RPN_OK and same_bits(out, first["a1"])


@pytest.mark.parametrize("precision", PRECISIONS)
def test_forwards_that_are_not_kept_are_a_rate_0_heads(lib, precision):
    c = dd.drop_case(1)
    pooled = cuda(c["pooled"])
    head = make_drop_head(c, precision)
    plain = make_head(c, seed=None)
    if precision != "f32":
        plain.compile(precision=precision)
    with torch.no_grad():
        ref = plain(pooled)
        out = head(pooled)
    assert same_bits(out[0], ref[0]) and same_bits(out[1], ref[1]) and head.dropout_state()["calls"] == 0
    copy = head.inference_copy(precision=precision)
    assert copy.dropout_state()["rate"] == 0.0                  # inference_copy never carries dropout
    inf = copy(pooled)
    assert same_bits(inf[0], ref[0]) and same_bits(inf[1], ref[1])
    # detect: the rate-0 head's detections, and no call counted
    rng = np.random.RandomState(2)
    lo = rng.uniform(0.0, 0.6, size=(2, 37, 2)).astype(np.float32)
    rois = cuda(np.concatenate([lo, lo + rng.uniform(0.1, 0.4, size=(2, 37, 2)).astype(np.float32)], axis=-1))
    variances = [0.1, 0.1, 0.2, 0.2]
    got, want = head.detect(rois, pooled, variances), plain.detect(rois, pooled, variances)
    assert all(same_bits(g, w) for g, w in zip(got, want)) and head.dropout_state()["calls"] == 0
    # a kept forward of the rate-0 head stores the plain activation (get_activation is useful on its own)
    kept = plain(pooled)
    assert same_bits(kept[0], ref[0])
    a1 = plain.kept_activation("fc1").cpu().numpy()
    assert a1.shape == (74, c["dims"][3]) and plain.dropout_state()["calls"] == 0
    if precision == "f32":                                       # (no z1 lies within its float32 bound of zero)
        assert np.array_equal(a1 > 0, dh.head_case(1)["ref"]["z1"] > 0)
    # the dropped head's kept forward differs from it, and counts
    dropped = head(pooled)
    assert not same_bits(dropped[0], ref[0]) and head.dropout_state()["calls"] == 1
    # ... and nothing is kept by a no_grad forward
    with torch.no_grad():
        head(pooled)
    with pytest.raises(ValueError):
        head.kept_activation("fc1")


def train_three_steps(head, c, pooled):
    for _ in range(3):
        run = kept_forward_and_backward(head, c, pooled)
        head.apply_gradients()
    return head.get_weights(), run


@pytest.mark.parametrize("precision", PRECISIONS)
def test_rate_0_is_the_head_without_the_argument_and_training_is_reproducible(lib, precision):
    c = dd.drop_case(0)
    pooled = cuda(c["pooled"])

    def fresh(**kw):
        head = make_head(c, seed=None, **kw)
        head.compile(learning_rate=1e-3, precision=precision)
        return head

    w_plain, run_plain = train_three_steps(fresh(), c, pooled)
    zero = fresh(dropout=0.0, dropout_seed=c["seed"])
    w_zero, run_zero = train_three_steps(zero, c, pooled)
    assert same_run(run_zero, run_plain) and zero.dropout_state()["calls"] == 0 and zero.train_steps() == 3
    assert all(same_bits(w_zero[n][k], w_plain[n][k]) for n in LAYERS for k in ("kernel", "bias"))
    # three steps at rate 0.5: other weights, and the same bytes on a second run from the same state
    first = fresh(dropout=RATE, dropout_seed=c["seed"])
    w_a, run_a = train_three_steps(first, c, pooled)
    assert first.dropout_state()["calls"] == 3
    assert any(not same_bits(w_a[n][k], w_plain[n][k]) for n in LAYERS for k in ("kernel", "bias"))
    w_b, run_b = train_three_steps(fresh(dropout=RATE, dropout_seed=c["seed"]), c, pooled)
    assert same_run(run_b, run_a) and all(same_bits(w_b[n][k], w_a[n][k]) for n in LAYERS for k in ("kernel", "bias"))
    assert all(np.isfinite(w_a[n][k]).all() for n in LAYERS for k in ("kernel", "bias"))


def test_backward_after_set_dropout_raises(lib):
    c = dd.drop_case(1)
    head = make_drop_head(c)
    pooled = cuda(c["pooled"]).requires_grad_()
    out = head(pooled)
    gl, gd = torch.ones_like(out[0]), torch.ones_like(out[1])
    head.set_dropout(0.25)
    with pytest.raises(ValueError, match="most recent call"):
        torch.autograd.backward(list(out), [gl, gd])
    assert pooled.grad is None
    # the ABI drops the kept forward too
    x = pooled.detach()
    head._forward(x, keep=True)
    assert lib.rpn_det_head_set_dropout(head._h, 0.5, 1) == L.RPN_OK
    assert lib.rpn_det_head_backward(head._h, L.ptr(x), 74, L.ptr(gl), L.ptr(gd), None, L.stream_ptr()) == L.RPN_ERR_INVALID
    assert b"no kept forward" in lib.rpn_last_error()
    out = head(pooled)                                           # the next call goes back as usual
    torch.autograd.backward(list(out), [gl, gd])
    assert pooled.grad is not None and bool(torch.isfinite(pooled.grad).all())
