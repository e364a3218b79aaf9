"""Helpers of tests/test_gpu_anchor_counts.py, shared with the child process that test starts under RPN_HEAD_SPLITK=0 (the knob is
read once per process): models at an arbitrary anchor count K, the float64 reference of rpn_conv + rpn_reg | rpn_cls on the
library's own feature tap, and the bounds.

Bounds (outputs against float64 on the same tap):
  f32              no further than 4 x the distance of torch-CPU float32 evaluating the same two layers on the same tap, + 1e-6 (the
                   rule of test_gpu_conv.test_model_forward_small), and within the project's 1e-4
  f16x3 / bf16x3   the project's 1e-4 on reg and cls
"""
import functools

import numpy as np
import torch

from oracle import conv_oracle as cv
from tf_rpn_amd.models._rpn_model import RPNModel, synthetic_weights

TOL = 1e-4


def hyper(img, K):
    return {"img_size": img, "anchor_count": K}


@functools.lru_cache(maxsize=2)
def weights_for(backbone, img, K, seed):
    """Every column of rpn_reg | rpn_cls has its own random weights: a column written to the wrong place is O(1) wrong."""
    return synthetic_weights(backbone, hyper(img, K), seed=seed)


def make(backbone, img, K, precision, max_batch, seed=None):
    weights = weights_for(backbone, img, K, 100 + K if seed is None else seed)
    model = RPNModel(backbone, hyper(img, K), precision=precision, max_batch=max_batch)
    model.set_weights(weights)
    return model, weights


@functools.lru_cache(maxsize=2)
def _images_cpu(B, img):
    return torch.rand((B, img, img, 3), generator=torch.Generator().manual_seed(B * 1000 + img))


def images(B, img):
    return _images_cpu(B, img).cuda()


def form(model, B):
    """(route, NB, pixels per workgroup, slabs) of a forward of B images, from rpn_model_head_launch_info."""
    info = model.head_launch_info(B)
    return info["route"], info["NB"], info["pixels_per_workgroup"], info["slabs"]


def head_kernel(model):
    return [op["kernel"] for op in model.ops() if op["name"] == "rpn_head"][0]


def head_on_tap(tap, weights, dtype):
    """rpn_conv (3x3 'same', ReLU) + rpn_reg | rpn_cls of oracle/conv_oracle.py on an NHWC tap -> NHWC float64 numpy (reg, cls)."""
    with torch.no_grad():
        x = torch.from_numpy(np.ascontiguousarray(tap)).to(dtype).permute(0, 3, 1, 2).contiguous()
        reg, cls = cv._head(x, weights, dtype)
    return tuple(t.permute(0, 2, 3, 1).to(torch.float64).numpy() for t in (reg, cls))


def forward(model, x):
    """Outputs of one forward, cloned (the next forward of the handle may reuse nothing of them, but the caller compares bits)."""
    reg, cls = model.predict_on_batch(x.contiguous())
    return reg.clone(), cls.clone()


def check_float64(model, weights, reg, cls, rows, label):
    """reg, cls: what the forward that JUST ran on `model` returned; rows: the images to check.  Asserts the bound of the model's
    precision on both outputs, no NaN, cls strictly inside (0, 1); prints and returns (err_reg, bound_reg, err_cls, bound_cls)."""
    B = int(reg.shape[0])
    assert not torch.isnan(reg).any().item() and not torch.isnan(cls).any().item(), label
    assert (cls > 0).all().item() and (cls < 1).all().item(), label
    tap = model.get_activation(model.tap_layer, batch=B)[list(rows)].cpu().numpy()
    r64, c64 = head_on_tap(tap, weights, torch.float64)
    # (a condition on the inputs: the reference itself stays where float32 holds a sigmoid strictly inside (0, 1) -- from a logit of
    # 16.7 on, 1 / (1 + exp(-v)) IS 1.0 in float32)
    assert c64.max() <= 1 - 2.0 ** -22 and c64.min() >= 2.0 ** -100, (label, c64.min(), 1 - c64.max())
    got_r = reg[list(rows)].cpu().numpy().astype(np.float64).reshape(r64.shape)
    got_c = cls[list(rows)].cpu().numpy().astype(np.float64).reshape(c64.shape)
    err_r, err_c = np.abs(got_r - r64).max(), np.abs(got_c - c64).max()
    bound_r = bound_c = TOL
    if model.precision == "f32":
        r32, c32 = head_on_tap(tap, weights, torch.float32)
        bound_r = min(TOL, 4 * np.abs(r32 - r64).max() + 1e-6)
        bound_c = min(TOL, 4 * np.abs(c32 - c64).max() + 1e-6)
    print("anchor_counts %s %s B=%d form=%s kernel=%s reg %.3g (bound %.3g) cls %.3g (bound %.3g)"
          % (label, model.precision, B, form(model, B), head_kernel(model), err_r, bound_r, err_c, bound_c))
    assert err_r <= bound_r and err_c <= bound_c, (label, err_r, bound_r, err_c, bound_c)
    return err_r, bound_r, err_c, bound_c


def same_bits(a, b):
    return torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


def row(out, i):
    return out[0][i], out[1][i]


def fallback_case(backbone, img, K, precision, max_batch, rows):
    """The head on the float32 implicit GEMM (K >= 20, or RPN_HEAD_SPLITK=0): float64 bound on `rows` of the full batch, image 0
    alone bit for bit."""
    model, weights = make(backbone, img, K, precision, max_batch)
    assert form(model, max_batch) == ("f32", 0, 0, 1) and form(model, 1) == ("f32", 0, 0, 1)
    assert "rpn_head_splitk" not in head_kernel(model) and head_kernel(model).startswith("conv_igemm_f32"), head_kernel(model)
    x = images(max_batch, img)
    full = forward(model, x)
    assert full[0].shape[-1] == 4 * K and full[1].shape[-1] == K
    errs = check_float64(model, weights, full[0], full[1], rows, "fallback %s img=%d K=%d" % (backbone, img, K))
    one = forward(model, x[:1])
    assert same_bits(row(one, 0), row(full, 0))
    return errs
