"""Cases, float64 reference, contract emulation and bounds of the VGG16 split-precision (f16x3 / bf16x3) forward, one op at a time.
Shared by tests/test_gpu_vgg16_ops.py (the kernels on an MI355X) and tests/test_vgg16_ops_host.py (the case table classified through
rpn_model_conv_launch_info, the bounds proved on the CPU).

Ops.  `graph(precision, keep)` lists the tensors the handle's graph really WRITES, in order, each with the conv layers and the pool
that produce it from the tensor before it.  Production f16x3: block1_pool (block1_conv1 + block1_conv2 + pool, one launch),
block2_conv1, block2_pool (block2_conv2 with the pool in its epilogue), block3_conv1, block3_conv2, block3_pool, block4_conv1,
block4_conv2, block4_pool, block5_conv1 .. 3, rpn_conv.  bf16x3: block1_conv1 (a float32 kernel writing SPLIT16) comes first and
block1_pool is block1_conv2 + pool.  `keep` (every activation kept): one op per layer, the pools on their own (maxpool_split).

Reference.  `op_ref(op, x, w)` is that op ALONE in float64 -- conv, bias, ReLU per layer (oracle/conv_oracle.py's `_conv`), the 2 x 2
'valid' max-pool where the op has one -- on the library's own output of the op before it, read with rpn_model_forward_to.  A SPLIT16
value is hi + lo of two 16-bit floats with |lo| <= ulp(hi) / 2: at most 11 + 11 + 1 (f16) or 8 + 8 + 1 (bf16) significant bits, so the
joined pair is EXACT in float32 and the float32 tensor forward_to returns is exactly what the next kernel reads (`join_is_exact`,
asserted once on the CPU).  The head pair (reg, cls) is rpn_conv + rpn_reg | rpn_cls in float64 on the library's block5_conv3.

Weights: synthetic_weights("vgg16", seed 11) with every bias redrawn uniform in (-0.1, 0.2): non-zero, both signs, most of them
positive -- a halo filled with relu(bias) instead of zeros, or a max-pool taken before the bias with 0 as its start value, shows.
Images: uniform [0, 1), one seeded sequence per image size.

Conditions on the inputs (`input_conditions`, asserted on the float64 reference, never on a kernel's output): every compared tensor
has between 5 % and 95 % non-zero elements and no value beyond half the float16 range (32752).

Bounds (U = 2^-24; u2 = 2^-22 for float16 halves, 2^-16 for bfloat16 halves), never from what the kernels give.
  `x3_bound`, elementwise, from the contract of include/rpn_hip.h and tf_rpn_amd/csrc/split_conv.h.  Per conv layer, with S = the
  same convolution of |x| with |w| in float64 and K = 9 Cin:
      (3 K + 2) U (S + |b|)   three float32-accumulated products per term, the 2^-s scale (exact) and the bias addition
    + conv(eX, |w|)           what the input already carries: the split residue u2 |x| (at least 2^-25 for a float16 lo half, whose
                              subnormal quantum is 2^-24) where the kernel splits float32 on the fly (the images), and inside
                              vgg_block1 the error of block1_conv1
    + u2 S + q K max|x|       the split of w 2^s (s = split_weight_shift: max|w| 2^s in [2^11, 2^12), so a float16 lo half's
                              quantum 2^-24 2^-s is at most 2^-35 max|w|; q = half of it, 2^-36 max|w|; bfloat16: s = 0, q = 0)
    + u2 S                    the dropped lo lo product
  ReLU is 1-Lipschitz; a pooled element takes the largest bound of its window (max is 1-Lipschitz in the sup norm); a tensor
  written as SPLIT16 adds u2 |y| + 2^-25 (float16: a lo half below 2^-14 is subnormal, spaced 2^-24 -- without this absolute term
  the bound is wrong for small activations); the total is doubled (second-order terms), as in tests/test_det_head_x3_host.py, whose
  product_bound_x3 this restates with convolutions in place of matrix products (an im2col of the full-resolution 64-channel tensors does not fit).
  `x3_f32_bound`, a scalar: 4 d + 1e-6 max(1, max|ref64|), d = the largest deviation from float64 of the contract evaluated on the CPU
  with float32 accumulation (`emulate_op`: three torch-CPU float32 convolutions of the 16-bit halves, lo hi + hi lo + hi hi, times
  2^-s, + bias, ReLU, pool, hi + lo) -- tests/mnv2_blocks.py's rule, its 4 and its 1e-6.
  Why both: x3_bound must allow one rounding per accumulated term against the whole S, (3 K + 2) U S = 2^-13 S at K = 576 and
  2^-10 S at K = 4608, while a dropped float16 cross product is 2^-12 per term with random signs.  x3_bound sees a wrong scale, a
  halo, a misplaced pooled value, a missing hi hi, and with bfloat16 halves (cross products of 2^-9) a dropped lo hi or lo half;
  the float16 cross product and lo half are seen by x3_f32_bound (tests/test_vgg16_ops_host.py proves which sees what).
  Float32 ops on these handles (bf16x3's block1_conv1): mnv2_blocks.f32_bound, with torch-CPU float32 evaluating the op AND
  writing it as hi + lo (the op's output format belongs to the op).
  Head pair: the scalar rule on reg and on cls (emulation: rpn_conv under the contract, the two 1 x 1 layers and the sigmoid in
  torch float32), and elementwise on reg: x3_bound of rpn_conv (float32 output: no hi + lo term, + 2 U S for the K tree's adds)
  carried through rpn_reg as test_det_head_host.product_bound does.
"""
import functools
import os
import sys

import numpy as np
import torch
import torch.nn.functional as Fnn

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import mnv2_blocks as mb  # noqa: E402
import test_det_head_x3_host as x3h  # noqa: E402
from oracle import conv_oracle as cv  # noqa: E402
from tf_rpn_amd.models._rpn_model import RPNModel, synthetic_weights  # noqa: E402

U = 2.0 ** -24
HALF_F16_RANGE = 32752.0
f32_bound = mb.f32_bound

CFG = ((2, 64), (2, 128), (3, 256), (3, 512), (3, 512))


def hyper(img):
    return {"img_size": img, "anchor_count": 9}


# ---- the graphs ------------------------------------------------------------------------------------------------------------------------
def _op(name, src, convs=(), pool=False, out_f32=False):
    return {"name": name, "src": src, "convs": tuple(convs), "pool": pool, "out_f32": out_f32}


@functools.lru_cache(maxsize=None)
def graph(precision, keep=False):
    """[op] in graph order (module docstring); op = {"name": tensor written, "src": tensor read ("input": the images), "convs": the
    conv layers run, "pool": a 2 x 2 max-pool behind them, "out_f32": written as float32 (rpn_conv) instead of SPLIT16}"""
    ops, t = [], "input"
    for b, (n, _c) in enumerate(CFG, start=1):
        names = ["block%d_conv%d" % (b, i + 1) for i in range(n)]
        pool = "block%d_pool" % b if b < 5 else None
        if keep:
            groups = [((c,), False, c) for c in names] + ([((), True, pool)] if pool else [])
        elif b == 1 and precision == "f16x3":
            groups = [(tuple(names), True, pool)]
        else:
            groups = [((c,), False, c) for c in names[:-1]] + [((names[-1],), bool(pool), pool or names[-1])]
        for convs, pooled, name in groups:
            ops.append(_op(name, t, convs, pooled))
            t = name
    ops.append(_op("rpn_conv", t, ("rpn_conv",), out_f32=True))
    return tuple(ops)


def op_named(precision, name, keep=False):
    return [o for o in graph(precision, keep) if o["name"] == name][0]


# ---- the case table --------------------------------------------------------------------------------------------------------------------
R64 = ("split16_reg", 64)
D64, D128 = ("split16_dma", 64), ("split16_dma", 128)


def _forms(b2, b3, b4, b5, rpn):
    """expected forms of one batch size: the (family, tile width) of block 2, 3, 4's layers WITHOUT the pool epilogue, of the same
    blocks' last layer WITH it (a pair each: (plain, pooled)), of block 5, and rpn_conv's (family, K form)"""
    return {"b2": b2, "b3": b3, "b4": b4, "b5": b5, "rpn": rpn}


# Each case: (precision, img, max_batch, keep) and per batch size the expected rpn_model_conv_launch_info of every op; `compare`: the ops
# compared with float64 (None: all of them; the others still run, they produce the inputs).  From the rules of
# conv3x3_split16_variant, at tiles = ceil(W / 32) ceil(H / 8) B: "dma,128" from tiles ceil(Cout / 128) >= 256 on; without a pool
# epilogue "reg,64" up to tiles ceil(Cout / 64) <= 128; "dma,64" between and under every pool below 256.  "reg,128" needs
# Cin % 64 != 0, which VGG16 never has (it stays covered by test_conv3x3_split_single_layer).  rpn_conv (F x F x 512 -> 512, a K
# tree): split 4 ways up to ceil(F / 32) ceil(F / 4) B 8 <= 128, 2 ways up to 256 on the register-staged kernel, 2 ways on the DMA
# kernel at 64 < ceil(F / 32) ceil(F / 8) B 8 <= 128, else the tree inside one workgroup of the 64-wide DMA kernel.
CASES = [
    # 136 -> 68, 34, 17, 8, many small images (the float64 reference of four of them is cheap): blocks 2 - 4 on dma,128 at B = 22
    # (block3_conv3 with 2, block4_conv3 with 4 channel tiles under the pool; 17 x 17 is ragged in x and y -- 3 tiles an image, 66 in
    # all -- and 17 -> 8 floors), blocks 3 and 4 on dma,64 at B = 12 and on reg,64 / dma,64 at B = 1: every layer of blocks 3 to 5
    # crosses a form boundary between two batch sizes of the one handle.  rpn_conv on its 8 x 8 map: 4 ways, 2 ways on the DMA
    # kernel, the unsplit tree.  (The 2-way split on the register-staged kernel cannot be reached at Cout = 512: it needs
    # ceil(F / 32) ceil(F / 4) B 8 in (128, 256] while the DMA form, asked first, takes every grid with ceil(F / 32) ceil(F / 8) B 8
    # in (64, 128] -- and ceil(F / 4) <= 2 ceil(F / 8).)
    dict(id="f16x3-136-b22", precision="f16x3", img=136, max_batch=22, keep=False, compare=None,
         forms={1: _forms((R64, D64), (R64, D64), (R64, D64), R64, ("split16_reg", 4)),
                12: _forms((D128, D128), (D64, D64), (D64, D64), R64, ("split16_dma", 2)),
                22: _forms((D128, D128), (D128, D128), (D128, D128), D64, ("split16_dma", 1))}),
    # the small-grid end: reg,64 everywhere, dma,64 under every pool
    dict(id="f16x3-96-b2", precision="f16x3", img=96, max_batch=2, keep=False, compare=None,
         forms={1: _forms((R64, D64), (R64, D64), (R64, D64), R64, ("split16_reg", 4)),
                2: _forms((R64, D64), (R64, D64), (R64, D64), R64, ("split16_reg", 4))}),
    # the reference's own size (31 x 31 features): rpn_conv 4 ways, 2 ways on the DMA kernel, unsplit; block 5 on reg,64 and dma,64
    dict(id="f16x3-500-b5", precision="f16x3", img=500, max_batch=5, keep=False,
         compare=("block5_conv1", "block5_conv2", "block5_conv3", "rpn_conv", "head"),
         forms={1: _forms((D128, D128), (D64, D64), (R64, D64), R64, ("split16_reg", 4)),
                3: _forms((D128, D128), (D128, D128), (D64, D64), R64, ("split16_dma", 2)),
                5: _forms((D128, D128), (D128, D128), (D128, D128), D64, ("split16_dma", 1))}),
    # bfloat16 halves: the float32 first layer writing SPLIT16, conv3x3_split with the pool epilogue; 150 -> 75, 37, 18, 9
    dict(id="bf16x3-150-b3", precision="bf16x3", img=150, max_batch=3, keep=False, compare=None,
         forms={1: _forms((R64, D64), (R64, D64), (R64, D64), R64, ("split16_reg", 4)),
                3: _forms((D64, D64), (R64, D64), (R64, D64), R64, ("split16_reg", 4))}),
    # every activation kept: convs without a pool epilogue, maxpool_split on its own, the f16x3 first layer on the 16-bit MFMA
    dict(id="f16x3-96-b2-keep", precision="f16x3", img=96, max_batch=2, keep=True, compare=None,
         forms={2: _forms((R64, R64), (R64, R64), (R64, R64), R64, ("split16_dma", 1))}),
    dict(id="bf16x3-96-b2-keep", precision="bf16x3", img=96, max_batch=2, keep=True, compare=None,
         forms={2: _forms((R64, R64), (R64, R64), (R64, R64), R64, ("split16_dma", 1))}),
]


def case_ids():
    return [c["id"] for c in CASES]


def expected_form(case, name, B):
    """(family, tile width, pool in the epilogue, K form) of the op writing tensor `name` at B images, from the case table"""
    f = case["forms"][B]
    op = op_named(case["precision"], name, case["keep"])
    if name == "rpn_conv":
        return (f["rpn"][0], 64, False, f["rpn"][1])
    if not op["convs"]:
        return ("maxpool_split", 0, False, 0)
    if len(op["convs"]) == 2:
        return ("vgg_block1", 64, True, 0)
    conv = op["convs"][0]
    if conv == "block1_conv1":
        return ("first_layer", 64, False, 0)
    if conv == "block1_conv2":
        return ("split", 64, op["pool"], 0)
    b = int(conv[5])
    fam, width = f["b5"] if b == 5 else f["b%d" % b][1 if op["pool"] else 0]
    return (fam, width, op["pool"], 0)


def form(model, name, B):
    info = model.conv_launch_info(name, B)
    return info["route"], info["width"], info["pool"], info["kform"]


def reached(case, model):
    """the set of forms a case reaches, as (precision, family, width, pool, K form, channel tiles under the pool), from the hook"""
    out = set()
    for B in case["forms"]:
        for op in graph(case["precision"], case["keep"]):
            fam, width, pool, kform = form(model, op["name"], B)
            cout = weights()[op["convs"][-1]]["kernel"].shape[3] if op["convs"] else 0
            out.add((case["precision"], fam, width, pool, kform, -(-cout // width) if pool and width else 0))
    return out


# ---- weights and images --------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=4)
def images(B, img):
    """(B, img, img, 3) float32 in [0, 1) on the CPU: the first B of one seeded sequence per image size"""
    return torch.rand((B, img, img, 3), generator=torch.Generator().manual_seed(9000 + img))


@functools.lru_cache(maxsize=1)
def weights():
    """module docstring, "Weights"; read-only"""
    w = synthetic_weights("vgg16", hyper(96), seed=11)
    rng = np.random.RandomState(12)
    for name in sorted(w):
        w[name] = dict(w[name], bias=rng.uniform(-0.1, 0.2, size=w[name]["bias"].shape).astype(np.float32))
        assert (w[name]["bias"] != 0).all() and (w[name]["bias"] > 0).sum() >= 4 and (w[name]["bias"] < 0).sum() >= 4
    return w


def scaled_layer(base, producer, consumer, k):
    """`base` with the producer's kernel and bias times 2^k and the consumer's kernel times 2^-k: ReLU is positively homogeneous, so
    only the producer's output changes (test_vgg16_block1_one_launch_flags_f16_overflow's trick)"""
    w = {n: dict(v) for n, v in base.items()}
    s = np.float32(2.0 ** k)
    w[producer]["kernel"] = base[producer]["kernel"] * s
    w[producer]["bias"] = base[producer]["bias"] * s
    w[consumer]["kernel"] = base[consumer]["kernel"] / s
    return w


def make(case, w=None):
    model = RPNModel("vgg16", hyper(case["img"]), precision=case["precision"], max_batch=case["max_batch"], keep_activations=case["keep"])
    model.set_weights(weights() if w is None else w)
    return model


# ---- the 16-bit halves ---------------------------------------------------------------------------------------------------------------------
def _bf16(x):
    """float32 -> the nearest bfloat16 (ties to even), as float32: split_format.hip's f32_to_bf16_rne"""
    u = np.ascontiguousarray(x, np.float32).view(np.uint32).astype(np.uint64)
    u = (u + 0x7fff + ((u >> 16) & 1)) & 0xffff0000
    return u.astype(np.uint32).view(np.float32)


def split(x, fmt):
    """float32 -> (hi, lo) float32 arrays: hi = h(x), lo = h(x - hi), h = float16 or bfloat16 rounding (split_piece)"""
    x = np.asarray(x, np.float32)
    if fmt == "f16x3":
        hi, lo = x3h.split16(x)
        return hi.astype(np.float32), lo.astype(np.float32)
    hi = _bf16(x)
    return hi, _bf16(x - hi)


def joined(x, fmt, drop_lo=False):
    """what a float32 tensor becomes when it is written as SPLIT16 and read back: hi + lo in float32 (exact, `join_is_exact`)"""
    hi, lo = split(x, fmt)
    return hi if drop_lo else hi + lo


def join_is_exact(x, fmt):
    hi, lo = split(x, fmt)
    return np.array_equal((hi + lo).astype(np.float64), hi.astype(np.float64) + lo.astype(np.float64))


def u2_of(fmt):
    return 2.0 ** -22 if fmt == "f16x3" else 2.0 ** -16


def shift_of(kernel, fmt):
    return x3h.shift_of(kernel) if fmt == "f16x3" else 0


# ---- float64 reference ---------------------------------------------------------------------------------------------------------------------
def _nchw(a, dtype):
    return cv._t(a, dtype).permute(0, 3, 1, 2).contiguous()


def _nhwc64(t):
    return t.permute(0, 2, 3, 1).contiguous().to(torch.float64).numpy()


def _conv3(x_nchw, kernel, bias, dtype):
    return cv._conv(x_nchw, kernel, bias, padding=1, dtype=dtype)


def _pool(t):
    return Fnn.max_pool2d(t, 2, 2)


def op_ref(op, x_nhwc, w, dtype=torch.float64):
    """op alone on its NHWC input in `dtype` -> {"layers": [float64 NHWC output of every conv layer, behind its ReLU], "out"}"""
    with torch.no_grad():
        h, layers = _nchw(x_nhwc, dtype), []
        for c in op["convs"]:
            h = torch.relu(_conv3(h, w[c]["kernel"], w[c]["bias"], dtype))
            layers.append(_nhwc64(h))
        if op["pool"]:
            h = _pool(h)
        return {"layers": layers, "out": _nhwc64(h)}


def op_ref32(op, x_nhwc, w, fmt):
    """a float32 op (bf16x3's block1_conv1) in torch-CPU float32, written as SPLIT16 as the op writes it"""
    return joined(op_ref(op, x_nhwc, w, torch.float32)["out"].astype(np.float32), fmt).astype(np.float64)


def head_ref(tap_nhwc, w, dtype=torch.float64):
    """rpn_conv + rpn_reg | rpn_cls on an NHWC tap -> float64 NHWC {"h": rpn_conv behind its ReLU, "reg", "cls"}"""
    with torch.no_grad():
        x = _nchw(tap_nhwc, dtype)
        h = torch.relu(_conv3(x, w["rpn_conv"]["kernel"], w["rpn_conv"]["bias"], dtype))
        reg, cls = cv._head(x, w, dtype)
        return {"h": _nhwc64(h), "reg": _nhwc64(reg), "cls": _nhwc64(cls)}


def input_conditions(out64, label=""):
    nz = float(np.mean(out64 != 0.0))
    assert 0.05 <= nz <= 0.95, (label, "non-zero share", nz)
    assert np.abs(out64).max() <= HALF_F16_RANGE, (label, np.abs(out64).max())
    return nz


# ---- the elementwise bound -----------------------------------------------------------------------------------------------------------------
def _conv_abs(t_nhwc, k_abs):
    """the same 3 x 3 'same' convolution of a non-negative float64 NHWC tensor with a non-negative HWIO kernel"""
    with torch.no_grad():
        return _nhwc64(_conv3(_nchw(t_nhwc, torch.float64), k_abs, None, torch.float64))


def _pool_max(e_nhwc):
    with torch.no_grad():
        return _nhwc64(_pool(_nchw(e_nhwc, torch.float64)))


def x3_bound(op, x_nhwc, ref, w, fmt, on_the_fly=None):
    """Elementwise bound on |split-precision op - ref["out"]| (module docstring).  on_the_fly: the kernel splits a float32 input
    itself (default: the op reads the images); an input read as SPLIT16 is exact."""
    u2 = u2_of(fmt)
    q_act = 2.0 ** -25 if fmt == "f16x3" else 0.0
    h = np.abs(np.asarray(x_nhwc, np.float64))
    on_the_fly = op["src"] == "input" if on_the_fly is None else on_the_fly
    e_in = np.where(h == 0, 0.0, np.maximum(u2 * h, q_act)) if on_the_fly else None
    e = None
    for c, y in zip(op["convs"], ref["layers"]):
        k_abs = np.abs(np.asarray(w[c]["kernel"], np.float64))
        K = 9 * k_abs.shape[2]
        S = _conv_abs(h, k_abs)
        q_w = max(2.0 ** -36 * k_abs.max(), 2.0 ** -49) if fmt == "f16x3" else 0.0
        e = (3 * K + 2) * U * (S + np.abs(np.asarray(w[c]["bias"], np.float64))) + 2.0 * u2 * S
        e = e + q_w * K * h.max()                      # q conv(|x|, 1) <= q K max|x|
        if e_in is not None:
            e = e + _conv_abs(e_in, k_abs)
        if op["out_f32"]:
            e = e + 2 * U * S                          # the K tree: (l0 + l1) + (l2 + l3), two more float32 additions
        else:
            e = e + u2 * np.abs(y) + q_act             # written as hi + lo (inside vgg_block1: into the second conv's halo tile)
        h, e_in = np.abs(y), e
    if op["pool"]:
        e = _pool_max(e) if e is not None else np.zeros_like(ref["out"])
    return 2.0 * e if e is not None else np.zeros_like(ref["out"])


def head_bounds(tap_nhwc, ref, w, fmt):
    """elementwise bound of reg (module docstring): x3_bound of rpn_conv carried through rpn_reg's float32 product"""
    import test_det_head_host as dh
    op = _op("rpn_conv", "block5_conv3", ("rpn_conv",), out_f32=True)
    e_h = x3_bound(op, tap_nhwc, {"layers": [ref["h"]], "out": ref["h"]}, w, fmt) / 2.0
    Wr = np.asarray(w["rpn_reg"]["kernel"], np.float64).reshape(512, -1)
    e = dh.product_bound(ref["h"].reshape(-1, 512), Wr, w["rpn_reg"]["bias"], eA=e_h.reshape(-1, 512), final=False)
    e = e + 4 * U * (np.abs(ref["h"].reshape(-1, 512)) @ np.abs(Wr))          # the head adds up to four slabs of rpn_conv first
    return (2.0 * e).reshape(ref["reg"].shape)


# ---- the contract's emulation --------------------------------------------------------------------------------------------------------------
def _conv32(t_nhwc, kernel):
    with torch.no_grad():
        y = _conv3(_nchw(np.asarray(t_nhwc, np.float32), torch.float32), np.asarray(kernel, np.float32), None, torch.float32)
        return y.permute(0, 2, 3, 1).contiguous().numpy()


def _pool32(t_nhwc):
    with torch.no_grad():
        return _pool(_nchw(t_nhwc, torch.float32)).permute(0, 2, 3, 1).contiguous().numpy()


def emulate_op(op, x_nhwc, w, fmt, parts=(1, 1, 1), drop_lo_out=False, shift_off=0, pool_first=False):
    """The contract of one op on a float32 NHWC input -> float32 NHWC: per conv layer the input as (hi, lo), the kernel times 2^s as
    (hi, lo), three float32-accumulated convolutions lo hi + hi lo + hi hi (`parts` switches hi hi, hi lo, lo hi), times 2^-s, + bias,
    ReLU, the pool, the result written as hi + lo unless the op writes float32.
    The mutations a kernel could have (tests/test_vgg16_ops_host.py): `drop_lo_out` writes the hi half alone; `shift_off` scales by
    2^-(s + shift_off); `pool_first` takes the pool of the raw accumulators with 0 as the start value of the maximum (right for
    values behind a ReLU, wrong before the bias) and applies bias and ReLU afterwards."""
    h = np.asarray(x_nhwc, np.float32)
    for i, c in enumerate(op["convs"]):
        kernel = np.asarray(w[c]["kernel"], np.float32)
        s = shift_of(kernel, fmt)
        (ah, al), (wh, wl) = split(h, fmt), split(kernel * np.float32(2.0 ** s), fmt)
        acc = np.float32(parts[2]) * _conv32(al, wh)
        acc = acc + np.float32(parts[1]) * _conv32(ah, wl)
        acc = acc + np.float32(parts[0]) * _conv32(ah, wh)
        z = acc * np.float32(2.0 ** -(s + shift_off))
        last = i == len(op["convs"]) - 1
        if pool_first and last and op["pool"]:
            z = _pool32(np.maximum(z, np.float32(0.0)))
        h = np.maximum(z + np.asarray(w[c]["bias"], np.float32), np.float32(0.0)).astype(np.float32)
        if not op["out_f32"]:
            h = joined(h, fmt, drop_lo=drop_lo_out and last)
    if op["pool"] and not (pool_first and op["convs"]):
        h = _pool32(h)
    return h


def emulate_head(tap_nhwc, w, fmt, **kw):
    """rpn_conv under the contract (float32 output), rpn_reg | rpn_cls and the sigmoid in torch-CPU float32 -> (reg, cls) float64"""
    h = emulate_op(_op("rpn_conv", "block5_conv3", ("rpn_conv",), out_f32=True), tap_nhwc, w, fmt, **kw)
    with torch.no_grad():
        x = _nchw(h, torch.float32)
        cls = torch.sigmoid(cv._conv(x, w["rpn_cls"]["kernel"], w["rpn_cls"]["bias"], dtype=torch.float32))
        reg = cv._conv(x, w["rpn_reg"]["kernel"], w["rpn_reg"]["bias"], dtype=torch.float32)
    return _nhwc64(reg), _nhwc64(cls)


def scalar_bound(emulated, ref64):
    """4 d + 1e-6 max(1, max|ref64|): mnv2_blocks.x3_f32_bound's rule"""
    return 4.0 * np.abs(np.asarray(emulated, np.float64) - ref64).max() + 1e-6 * max(1.0, np.abs(ref64).max())


def x3_f32_bound(op, x_nhwc, ref, w, fmt):
    return scalar_bound(emulate_op(op, x_nhwc, w, fmt), ref["out"])


def is_f32_op(model, op):
    """a conv op of a split-precision handle whose arithmetic is float32 (rpn_model_op_arith): bf16x3's first layer"""
    arith = {o["name"]: o["arith"] for o in model.ops()}
    return len(op["convs"]) == 1 and arith.get(op["convs"][0]) == "f32"


# ---- the inputs without a GPU ----------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=8)
def cpu_chain(precision, img, keep=False, B=1):
    """The ops' inputs without a GPU: B case images carried through the float64 ops, each op's input rounded to float32 (and to hi +
    lo where the library holds it as SPLIT16) as the library would hand it on -> {tensor name: float32 NHWC}, "input" included"""
    x = images(B, img).numpy()
    out = {"input": x}
    for op in graph(precision, keep):
        y = op_ref(op, out[op["src"]], weights())["out"].astype(np.float32)
        out[op["name"]] = y if op["out_f32"] else joined(y, precision)
    return out
