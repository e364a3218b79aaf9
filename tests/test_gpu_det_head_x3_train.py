"""The detection head trained in split float16 on the GPU (rpn_fc_wgrad_x3, rpn_fc_dgrad_x3, rpn_det_head_set_train_precision,
models.DetectionHead.compile(precision="f16x3")) against the float64 restatements of tests/test_det_head_host.py, inside the
a-priori bounds of tests/test_det_head_x3_train_host.py (`wgrad_bound`, `dgrad_bound`, `bounds_train`: stated from the inputs
alone and checked there on the CPU against a numpy emulation of the contract).  Everything the contract calls bit-identical -- a
second call, appended zero rows, a row alone against the row in a batch, the exact cases against the emulation, the forward against
the f16x3 inference head, the way back to float32 -- is compared byte for byte.
"""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import test_det_head_host as dh  # noqa: E402
import test_det_head_x3_host as hx  # noqa: E402
import test_det_head_x3_train_host as tr  # noqa: E402
import test_roi_host as rp  # noqa: E402
from test_det_head_host import lib  # noqa: E402,F401  (fixture)
from test_gpu_det_head import inside, loss_gradients, make_head, same_bits  # noqa: E402
from tf_rpn_amd import _lib as L  # noqa: E402
from tf_rpn_amd.utils import roi_utils  # noqa: E402

pytestmark = pytest.mark.gpu
LAYERS = dh.LAYERS
FILL = 7.0                                                       # what padding columns hold: read and dropped, or never written


def cuda(a):
    return torch.from_numpy(np.array(a)).cuda()


def wgrad_x3(lib, a, dz_padded, N, status=None):
    """-> (K, N) of a (M, K)^T dz (M, N); asserts that the padding columns of the output were left alone"""
    M, K = (int(v) for v in a.shape)
    ldo = (N + 3) // 4 * 4
    out = torch.full((K, ldo), FILL, dtype=torch.float32, device="cuda")
    st = lib.rpn_fc_wgrad_x3(L.ptr(a), L.ptr(dz_padded), M, K, N, int(dz_padded.shape[1]), ldo, L.ptr(out), L.ptr(status), L.stream_ptr())
    L.check(st, "rpn_fc_wgrad_x3")
    assert bool((out[:, N:] == FILL).all())
    return out[:, :N].contiguous()


def dgrad_x3(lib, dz_padded, w_padded, N, h=None, status=None):
    M, K = int(dz_padded.shape[0]), int(w_padded.shape[0])
    out = torch.full((M, K), float("nan"), dtype=torch.float32, device="cuda")
    st = lib.rpn_fc_dgrad_x3(L.ptr(dz_padded), L.ptr(w_padded), M, K, N, int(dz_padded.shape[1]), int(w_padded.shape[1]), L.ptr(h), L.ptr(out),
                             L.ptr(status), L.stream_ptr())
    L.check(st, "rpn_fc_dgrad_x3")
    return out


# ---- the two products against float64 ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", tr.WGRAD_N)
@pytest.mark.parametrize("K", tr.WGRAD_K)
def test_fc_wgrad_x3_against_float64(lib, K, N):
    c = tr.wgrad_case(K, N)
    a_d = cuda(c["a"])
    for scale in tr.GRAD_SCALES:
        dz = tr.scaled(c["dz"], scale)
        dz_d = cuda(tr.pad_columns(dz, FILL))
        for M in tr.WGRAD_M:
            a64, z64 = c["a"][:M].astype(np.float64), dz[:M].astype(np.float64)
            ref, bound = a64.T @ z64, tr.wgrad_bound(a64, z64)
            a_m, dz_m = a_d[:M].contiguous(), dz_d[:M].contiguous()
            got_t = wgrad_x3(lib, a_m, dz_m, N)
            got = got_t.cpu().numpy()
            assert got.shape == (K, N) and np.isfinite(got).all()
            err = np.abs(got - ref)
            print("M %3d K %3d N %3d scale %g: max err %.3e, max err / bound %.3f" % (M, K, N, scale, err.max(),
                                                                                    (err / np.maximum(bound, 1e-300)).max()))
            assert (err <= bound).all()
            assert same_bits(got_t, wgrad_x3(lib, a_m, dz_m, N))                              # a second call: the same bytes
            # zero rows appended to both operands (a reduction tail that crosses into another step of 32): the same bytes
            a_z = torch.cat([a_m, torch.zeros((35, K), device="cuda")])
            dz_z = torch.cat([dz_m, torch.zeros((35, dz_m.shape[1]), device="cuda")])
            assert same_bits(got_t, wgrad_x3(lib, a_z, dz_z, N))


@pytest.mark.parametrize("N", tr.DGRAD_N)
@pytest.mark.parametrize("K", tr.DGRAD_K)
def test_fc_dgrad_x3_against_float64(lib, K, N):
    c = tr.dgrad_case(K, N)
    w64 = c["w"].astype(np.float64)
    w_d, h_d = cuda(tr.pad_columns(c["w"], FILL)), cuda(c["h"])
    full = {}
    for scale in tr.GRAD_SCALES:
        dz = tr.scaled(c["dz"], scale)
        dz_d = cuda(tr.pad_columns(dz, FILL))
        for M in tr.DGRAD_M:
            z64 = dz[:M].astype(np.float64)
            bound = tr.dgrad_bound(z64, w64)
            dz_m = dz_d[:M].contiguous()
            for masked in (False, True):
                h_m = h_d[:M].contiguous() if masked else None
                ref = z64 @ w64.T * ((c["h"][:M] > 0) if masked else 1.0)
                got_t = dgrad_x3(lib, dz_m, w_d, N, h=h_m)
                got = got_t.cpu().numpy()
                assert got.shape == (M, K) and np.isfinite(got).all()
                err = np.abs(got - ref)
                print("M %3d K %3d N %3d scale %g mask %d: max err %.3e, max err / bound %.3f" % (
                    M, K, N, scale, masked, err.max(), (err / np.maximum(bound, 1e-300)).max()))
                assert (err <= bound).all()
                assert same_bits(got_t, dgrad_x3(lib, dz_m, w_d, N, h=h_m))
                if masked:
                    assert not got[c["h"][:M] <= 0].any()                                    # exactly zero under the mask
                if M == 130 and scale == 1.0:
                    full[masked] = got
    # batch independence: row m of the M = 130 result is the M = 1 result of row m alone, byte for byte, at the tile edges (the rows
    # share the batch's t: tr.dgrad_case)
    dz_d = cuda(tr.pad_columns(c["dz"], FILL))
    for m in tr.EDGE_ROWS:
        for masked, got in full.items():
            one = dgrad_x3(lib, dz_d[m:m + 1].contiguous(), w_d, N, h=h_d[m:m + 1].contiguous() if masked else None)
            assert same_bits(one[0], got[m]), (m, masked)


@pytest.mark.parametrize("K", (32, 108))
def test_exact_cases_equal_the_emulation_bit_for_bit(lib, K):
    """every product is a multiple of a fixed power of two and every partial sum fits float32 (asserted on the CPU): any order of
    summation gives the emulation's bits; a dropped product, a misplaced lo half or a wrong shift does not"""
    c = tr.exact_operands(K)
    z = c["z"].astype(np.float32)
    got = wgrad_x3(lib, cuda(c["at"]), cuda(hx.pad_columns(c["W"])), c["W"].shape[1])
    assert same_bits(got[:c["rows"]], z) and not got[c["rows"]:].cpu().numpy().any()
    got = dgrad_x3(lib, cuda(c["A"]), cuda(c["wt"]), K)
    assert same_bits(got, z)


# ---- the whole head ------------------------------------------------------------------------------------------------------------------------
def make_head_x3t(c, **kw):
    head = make_head(c, seed=None)
    head.compile(precision="f16x3", **kw)
    return head


def run_backward(head, c, pooled, scale=1.0):
    logits, deltas = head(pooled)
    gl, gd = loss_gradients(logits, deltas, c["labels"], c["deltas"])
    gl, gd = gl * scale, gd * scale
    torch.autograd.backward([logits, deltas], [gl, gd])
    return gl, gd


@pytest.mark.parametrize("scale", tr.HEAD_GRAD_SCALES)
@pytest.mark.parametrize("index", range(len(dh.HEAD_CONFIGS)))
def test_head_backward_x3(lib, index, scale):
    c = dh.head_case(index)
    head = make_head_x3t(c)
    assert head.train_precision == "f16x3" and head.precision == "f32"
    pooled = cuda(c["pooled"]).requires_grad_()
    gl, gd = run_backward(head, c, pooled, scale)
    gl64, gd64 = gl.cpu().numpy().astype(np.float64), gd.cpu().numpy().astype(np.float64)
    ref_g, ref_gp = dh.det_head_backward_ref(c["weights"], c["pooled"], gl64, gd64)
    b = tr.bounds_train(c["weights"], c["pooled"], gl64, gd64)
    got = head.get_gradients()
    for n in LAYERS:
        for k in ("kernel", "bias"):
            assert got[n][k].dtype == np.float32
            inside(got[n][k], ref_g[n][k], b[n][k], "%s/%s" % (n, k))
    inside(pooled.grad, ref_gp, b["grad_pooled"], "grad_pooled")
    assert head.status() == {"f16_range": False}
    # the float32 head's gradients differ somewhere: the products really ran in split float16
    f32 = make_head(c, seed=None)
    x = cuda(c["pooled"])
    f32._forward(x, keep=True)
    L.check(lib.rpn_det_head_backward(f32._h, L.ptr(x), 74, L.ptr(gl), L.ptr(gd), None, L.stream_ptr()), "float32 backward")
    assert not same_bits(f32.get_gradients()["fc1"]["kernel"], got["fc1"]["kernel"])
    # a second forward + backward: the same bytes
    first_gp = pooled.grad.clone()
    pooled.grad = None
    run_backward(head, c, pooled, scale)
    again = head.get_gradients()
    assert same_bits(pooled.grad, first_gp)
    assert all(same_bits(again[n][k], got[n][k]) for n in LAYERS for k in ("kernel", "bias"))
    # pooled without requires_grad skips the last product: the parameter gradients are the same bytes
    run_backward(head, c, pooled.detach(), scale)
    third = head.get_gradients()
    assert all(same_bits(third[n][k], got[n][k]) for n in LAYERS for k in ("kernel", "bias"))
    # the ABI itself: NULL for d_grad_pooled writes no such tensor, a buffer is written in full with the same bytes
    head._forward(x, keep=True)
    gp = torch.full_like(x, float("nan"))
    assert lib.rpn_det_head_backward(head._h, L.ptr(x), 74, L.ptr(gl), L.ptr(gd), L.ptr(gp), L.stream_ptr()) == L.RPN_OK
    assert same_bits(gp, first_gp)
    # the kept forward is dropped by a change of precision
    head._forward(x, keep=True)
    assert lib.rpn_det_head_set_train_precision(head._h, L.PRECISIONS["f16x3"]) == L.RPN_OK
    assert lib.rpn_det_head_backward(head._h, L.ptr(x), 74, L.ptr(gl), L.ptr(gd), None, L.stream_ptr()) == L.RPN_ERR_INVALID
    assert b"no kept forward" in lib.rpn_last_error()


def test_forward_is_the_inference_heads_and_follows_the_weights(lib):
    """compile("f16x3"): every forward is the f16x3 inference head's on the same weights, bit for bit, before and after each Adam step
    (the image and the shifts are refreshed on the device)"""
    c = dh.head_case(0)
    lr = 1e-3
    head = make_head_x3t(c, learning_rate=lr)
    twin = make_head(c, seed=None)
    twin.compile(learning_rate=lr)
    pooled = cuda(c["pooled"])

    def check_forward():
        with torch.no_grad():
            out = head(pooled)
        copy = head.inference_copy(precision="f16x3")
        ref = copy(pooled)
        assert same_bits(out[0], ref[0]) and same_bits(out[1], ref[1])
        kept = head(pooled)                                      # a kept forward: the same bits
        assert kept[0].requires_grad and same_bits(kept[0], out[0]) and same_bits(kept[1], out[1])
        with torch.no_grad():
            f32 = head.inference_copy()(pooled)
        assert not same_bits(f32[0], out[0])                     # ... and not the float32 head's
        return out

    before = check_forward()
    for step in (1, 2, 3):
        for h in (head, twin):
            run_backward(h, c, pooled)
            h.apply_gradients()
        after = check_forward()
        assert not same_bits(after[0], before[0])
        before = after
    assert head.train_steps() == 3 and twin.train_steps() == 3
    # The float32 twin took the same three steps from gradients that differ inside the gradient bound.  Adam turns a gradient into a
    # move of at most lr (1 - beta_1) / sqrt(1 - beta_2) per step whatever its size (and one of about lr times the relative error
    # where the gradient is well above that error), so the two sets of weights agree within 3 steps x 2 such moves -- not by bytes.
    w, wt = head.get_weights(), twin.get_weights()
    move = lr * (1 - 0.9) / np.sqrt(1 - 0.999)
    differ = False
    for n in LAYERS:
        for k in ("kernel", "bias"):
            d = np.abs(w[n][k].astype(np.float64) - wt[n][k]).max()
            print("%s/%s: max |f16x3 - f32| after three steps %.3e (bar %.3e)" % (n, k, d, 6 * move))
            assert d <= 6 * move
            differ = differ or not same_bits(w[n][k], wt[n][k])
            assert not np.array_equal(w[n][k], c["weights"][n][k])
    assert differ
    # set_weights: the image follows too
    head.set_weights(c["weights"])
    with torch.no_grad():
        out = head(pooled)
    fresh = make_head(c, trainable=False, seed=None, precision="f16x3")(pooled)
    assert same_bits(out[0], fresh[0]) and same_bits(out[1], fresh[1])


def test_going_back_to_float32(lib):
    c = dh.head_case(1)
    head = make_head_x3t(c, learning_rate=1e-3)
    pooled = cuda(c["pooled"]).requires_grad_()
    run_backward(head, c, pooled)
    head.apply_gradients()
    head.compile(learning_rate=1e-3, precision="f32")
    assert head.train_precision == "f32" and head.train_steps() == 1
    never = make_head(dict(c, weights=head.get_weights()), seed=None)
    grads = []
    for h in (head, never):
        x = cuda(c["pooled"]).requires_grad_()
        logits, deltas = h(x)
        if not grads:
            gl, gd = loss_gradients(logits, deltas, c["labels"], c["deltas"])
        torch.autograd.backward([logits, deltas], [gl, gd])
        grads.append((logits.detach().clone(), h.get_gradients(), x.grad.clone()))
    assert same_bits(grads[0][0], grads[1][0]) and same_bits(grads[0][2], grads[1][2])
    assert all(same_bits(grads[0][1][n][k], grads[1][1][n][k]) for n in LAYERS for k in ("kernel", "bias"))
    assert head.status() == {"f16_range": False}
    head.apply_gradients()                                       # Adam's moments and the step count went along
    assert head.train_steps() == 2
    # ... and forth again: the image kept from before is stale after that float32 step and is refreshed before it is read
    head.compile(learning_rate=1e-3, precision="f16x3")
    with torch.no_grad():
        out = head(cuda(c["pooled"]))
    ref = head.inference_copy(precision="f16x3")(cuda(c["pooled"]))
    assert same_bits(out[0], ref[0]) and same_bits(out[1], ref[1]) and head.train_steps() == 2


def test_gradient_range(lib):
    """a non-finite gradient raises the flag; a finite one of any magnitude does not (the shift brings it into range)"""
    c = dh.head_case(1)
    head = make_head_x3t(c)
    pooled = cuda(c["pooled"]).requires_grad_()
    for value, raised in ((float("nan"), True), (float("inf"), True), (3e38, False)):
        pooled.grad = None
        logits, deltas = head(pooled)
        gl, gd = loss_gradients(logits, deltas, c["labels"], c["deltas"])
        gl[1, 5, 2] = value
        torch.autograd.backward([logits, deltas], [gl, gd])
        assert head.status(reset=True) == {"f16_range": raised}, value
        if not raised:
            g = head.get_gradients()
            assert all(np.isfinite(g[n][k]).all() for n in LAYERS for k in ("kernel", "bias"))
            assert bool(torch.isfinite(pooled.grad).all())
            assert np.abs(g["cls"]["kernel"]).max() > 1e36       # ... and the large entry is still there
    assert head.status() == {"f16_range": False}


# ---- end to end through autograd -------------------------------------------------------------------------------------------------------------
def test_feature_map_gradient_end_to_end_x3(lib):
    """tests/test_gpu_det_head.test_feature_map_gradient_end_to_end's route with the head compiled in f16x3"""
    c = dh.e2e_case()
    ph, pw, Cf, H1, H2, C = c["dims"]
    head = make_head_x3t(c)
    feat = cuda(c["feat"]).requires_grad_()
    rois, valid = cuda(c["rois"]), cuda(c["valid"])
    pooled = roi_utils.roi_pooling(feat, rois, (ph, pw), valid=valid)
    pooled.retain_grad()
    assert same_bits(pooled, c["pooled"])
    logits, deltas = head(pooled)
    reg_loss, cls_loss = roi_utils.roi_losses(logits, deltas, cuda(c["labels"]), cuda(c["deltas"]))
    (reg_loss + cls_loss).backward()
    assert feat.grad is not None and tuple(feat.grad.shape) == tuple(feat.shape)
    assert same_bits(feat.grad, roi_utils.roi_pooling_backward(pooled.grad, rois, tuple(feat.shape), valid=valid))
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
    gl64, gd64, gp64 = l64.grad.numpy(), d64.grad.numpy(), x.grad.numpy()
    # the output gradients' own error, as in the float32 test but from the split forward's bound on the logits / deltas
    fwd = hx.bounds_x3(c["weights"], c["pooled"])
    keptn, posn = kept.numpy()[:, None], pos.numpy()[:, None]
    e_gl = np.broadcast_to(keptn * (2.0 * fwd["logits"].reshape(74, C).max(axis=1, keepdims=True) / n_kept), (74, C)) + 2e-6 * np.abs(gl64).max()
    e_gd = posn * (fwd["deltas"].reshape(74, 4 * C) / n_pos) + 2e-6 * np.abs(gd64).max()
    b = tr.bounds_train(c["weights"], c["pooled"], gl64, gd64, e_grad_logits=e_gl, e_grad_deltas=e_gd)
    inside(pooled.grad, gp64, b["grad_pooled"], "grad_pooled")
    shape = tuple(c["feat"].shape)
    ref = rp.roi_pool_backward_ref(gp64, c["rois"], shape, valid=c["valid"], coord_dtype=np.float32)
    terms = 37 * ph * pw * 4
    bound = rp.roi_pool_backward_ref(b["grad_pooled"], c["rois"], shape, valid=c["valid"], coord_dtype=np.float32) + \
        2.0 * (terms + 4) * dh.U * rp.roi_pool_backward_ref(np.abs(gp64), c["rois"], shape, valid=c["valid"], coord_dtype=np.float32,
                                                           unit_weights=True)
    assert np.abs(ref).max() > 0
    inside(feat.grad, ref, bound, "feat.grad")
    assert head.status() == {"f16_range": False}
