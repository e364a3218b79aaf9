"""CPU suite of the one-op-at-a-time VGG16 split-precision tests (tests/vgg_ops.py, tests/test_gpu_vgg16_ops.py): the launch-info hook
rpn_model_conv_launch_info where it needs no device, the case table classified through it, the conditions on the inputs, and the two
bounds proved against the emulation of the arithmetic contract -- inside them as specified, outside them with a term dropped, the
scale off by one, or the pool taken too early.

Which bound sees which mutation (printed by test_the_bounds_notice_a_wrong_kernel; f16x3 at img 96, fused and with every activation
kept, bf16x3 at img 150; ratios over the ops):
  x3_bound (elementwise) is left on at least one op by every mutation: by a scale off by one power of two on every op (33 - 38000
  times the bound), by a pool taken before the bias on every pooled op (1.98 - 84 times), by a dropped lo hi product on the K = 27
  first layer (19 times) and on bf16x3's block1_pool and block2_conv1 (2.2 times), by a dropped lo half of the output on the same
  and on bf16x3's block2_pool and block3_conv1.  With float16 halves a dropped lo hi or lo half stays at 0.015 - 0.73 of x3_bound
  on the K >= 576 layers (vgg_ops.py says why); x3_f32_bound sees both on every op (62 - 160 times), which is asserted too.
"""
import ctypes
import os
import re
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import vgg_ops as vo  # noqa: E402
from test_det_head_host import lib  # noqa: E402,F401  (fixture)
from tf_rpn_amd import _lib as L  # noqa: E402
from tf_rpn_amd.models._rpn_model import RPNModel  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ["rpn_model_conv_launch_info"]


def _handle(case):
    return RPNModel("vgg16", vo.hyper(case["img"]), precision=case["precision"], max_batch=case["max_batch"],
                    keep_activations=case["keep"])


def test_new_symbols_are_declared_exported_and_bound(lib):
    code = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "rpn_hip.h")).read(), flags=re.S)
    raw = ctypes.CDLL(L.LIB_PATH)
    for name in NEW_SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, code), "%s is not declared" % name
        assert hasattr(raw, name) and name in L.exported_symbols()
    for i, route in enumerate(RPNModel.CONV_ROUTES):
        assert re.search(r"#define RPN_CONV_ROUTE_%s %d\b" % (route.upper(), i), code), route
    assert lib.rpn_abi_version() == 1
    assert "max_batch" in RPNModel.ops.__doc__ and "conv_launch_info" in RPNModel.ops.__doc__


@pytest.mark.parametrize("case", vo.CASES, ids=vo.case_ids())
def test_conv_launch_info_matches_the_case_table(lib, case):
    """Host arithmetic only (a handle is created without a device): every op of every case at every batch size of the table has the
    form the table expects.  Printed: the forms the case reaches."""
    m = _handle(case)
    for B in case["forms"]:
        for op in vo.graph(case["precision"], case["keep"]):
            assert vo.form(m, op["name"], B) == vo.expected_form(case, op["name"], B), (case["id"], op["name"], B)
    print("vgg16 ops %s reaches: %s" % (case["id"], sorted(vo.reached(case, m))))
    # a pooled tensor is written by the conv in front of it; the conv's own tensor is then never written
    if not case["keep"]:
        assert vo.form(m, "block2_conv2", 1) == vo.form(m, "block2_pool", 1) and vo.form(m, "block2_pool", 1)[2]


def test_case_table_reaches_every_form(lib):
    """Every form of the list occurs in the table, classified through the hook: a changed threshold cannot silently empty a class."""
    seen = set()
    for case in vo.CASES:
        seen |= vo.reached(case, _handle(case))
    f16 = {s[1:] for s in seen if s[0] == "f16x3"}
    bf16 = {s[1:] for s in seen if s[0] == "bf16x3"}
    assert ("vgg_block1", 64, True, 0, 1) in f16
    assert ("split", 64, True, 0, 1) in bf16 and ("first_layer", 64, False, 0, 0) in bf16      # block1_conv2 + pool; SPLIT16 first layer
    assert ("first_layer", 64, False, 0, 0) in f16 and ("split", 64, False, 0, 0) in f16       # every activation kept
    assert ("maxpool_split", 0, False, 0, 0) in f16
    assert ("split16_reg", 64, False, 0, 0) in f16
    for width in (64, 128):
        assert ("split16_dma", width, False, 0, 0) in f16, width
        assert any(s[:4] == ("split16_dma", width, True, 0) for s in f16), width
    assert ("split16_dma", 128, True, 0, 2) in f16 and ("split16_dma", 128, True, 0, 4) in f16   # block3_conv3 / block4_conv3
    # rpn_conv: every value conv_ksplit_at returns, and the unsplit K tree
    assert {("split16_reg", 64, False, 4, 0), ("split16_dma", 64, False, 2, 0), ("split16_dma", 64, False, 1, 0)} <= f16
    assert not any(s[1] == 128 and s[0] == "split16_reg" for s in f16 | bf16)                    # reg,128: Cin % 64 != 0 only
    # one layer crosses from one form to another between two batch sizes of the same handle
    case = vo.CASES[0]
    m = _handle(case)
    assert case["id"] == "f16x3-136-b22"
    forms = {B: vo.form(m, "block4_conv1", B) for B in case["forms"]}
    assert len(set(forms.values())) == 3, forms
    # ... while ops() names the kernel of max_batch
    kernels = {o["name"]: o["kernel"] for o in m.ops()}
    assert kernels["block4_conv1"] == "conv3x3_split16_dma<f16x3,128>" and forms[1][0] == "split16_reg"
    # no op of the production graphs is left uncompared in every case
    for precision in ("f16x3", "bf16x3"):
        names = {op["name"] for op in vo.graph(precision)} | {"head"}
        covered = set()
        for c in vo.CASES:
            if c["precision"] == precision and not c["keep"]:
                covered |= names if c["compare"] is None else set(c["compare"])
        assert covered == names, (precision, names - covered)


def test_conv_launch_info_errors(lib):
    m = RPNModel("vgg16", vo.hyper(96), precision="f16x3", max_batch=4)
    info = (ctypes.c_int * 4)()
    assert lib.rpn_model_conv_launch_info(m._h, b"block2_pool", 4, info) == L.RPN_OK
    for bad in (0, -1, 5):
        assert lib.rpn_model_conv_launch_info(m._h, b"block2_pool", bad, info) == L.RPN_ERR_INVALID
        assert b"outside [1, 4]" in lib.rpn_last_error()
        with pytest.raises(ValueError):
            m.conv_launch_info("block2_pool", bad)
    for bad in ("block9_conv1", "input", "rpn_reg", "rpn_head", ""):
        assert lib.rpn_model_conv_launch_info(m._h, bad.encode(), 1, info) == L.RPN_ERR_INVALID, bad
        with pytest.raises(ValueError):
            m.conv_launch_info(bad, 1)
    assert lib.rpn_model_conv_launch_info(None, b"block2_pool", 1, info) == L.RPN_ERR_INVALID
    assert lib.rpn_model_conv_launch_info(m._h, None, 1, info) == L.RPN_ERR_INVALID
    assert lib.rpn_model_conv_launch_info(m._h, b"block2_pool", 1, None) == L.RPN_ERR_INVALID
    # ops that are not on a split route: the float32 graph, MobileNetV2's fused blocks
    f = RPNModel("vgg16", vo.hyper(96), precision="f32", max_batch=2)
    for name in (b"block1_conv1", b"block2_conv1", b"block2_pool", b"rpn_conv"):
        assert lib.rpn_model_conv_launch_info(f._h, name, 1, info) == L.RPN_ERR_INVALID, name
    assert b"not written on a split-precision route" in lib.rpn_last_error()
    mn = RPNModel("mobilenet_v2", vo.hyper(128), precision="f16x3", max_batch=2)
    assert lib.rpn_model_conv_launch_info(mn._h, b"block_3_project", 1, info) == L.RPN_ERR_INVALID
    assert mn.conv_launch_info("rpn_conv", 1)["route"].startswith("split16")


# ---- inputs, emulation, bounds ---------------------------------------------------------------------------------------------------------------
SIZES = sorted({(c["precision"], c["img"]) for c in vo.CASES})
CHAINS = [("f16x3", 96, False), ("f16x3", 96, True), ("bf16x3", 150, False)]


def test_a_joined_pair_is_exact_in_float32():
    rng = np.random.RandomState(4)
    x = np.concatenate([rng.standard_normal(4096).astype(np.float32) * s for s in (1.0, 1e-3, 1e-6, 3e4, 2.0 ** -14, 2.0 ** -20)]
                       + [np.float32([0.0, 65504.0, 2.0 ** -24, 2.0 ** -25, 1.0 + 2.0 ** -11, 1.0 + 2.0 ** -12])])
    x = x[np.abs(x) <= 65504.0]
    for fmt in ("f16x3", "bf16x3"):
        assert vo.join_is_exact(x, fmt), fmt
        assert np.abs(vo.joined(x, fmt).astype(np.float64) - x).max() <= (2.0 ** -25 if fmt == "f16x3" else 0) + vo.u2_of(fmt) * np.abs(x).max()
        y = vo.joined(x, fmt)
        assert np.array_equal(vo.joined(y, fmt), y)          # what the next kernel reads back is what forward_to returns
    chain = vo.cpu_chain("f16x3", 96)
    assert all(np.array_equal(vo.joined(chain[op["name"]], "f16x3"), chain[op["name"]]) for op in vo.graph("f16x3")[:-1])


@pytest.mark.parametrize("precision,img", SIZES, ids=["%s-%d" % s for s in SIZES])
def test_case_inputs_meet_the_conditions(precision, img):
    chain = vo.cpu_chain(precision, img)
    w = vo.weights()
    for op in vo.graph(precision):
        nz = vo.input_conditions(vo.op_ref(op, chain[op["src"]], w)["out"], "%s img %d %s" % (precision, img, op["name"]))
        print("vgg16 ops conditions %s img=%d %s: %.3f non-zero" % (precision, img, op["name"], nz))
    ref = vo.head_ref(chain["block5_conv3"], w)
    assert ref["cls"].max() <= 1 - 2.0 ** -22 and ref["cls"].min() >= 2.0 ** -100


@pytest.mark.parametrize("precision,img,keep", CHAINS, ids=["%s-%d%s" % (p, i, "-keep" if k else "") for p, i, k in CHAINS])
def test_the_contract_lies_inside_both_bounds(precision, img, keep):
    """emulate_op (the contract, float32 accumulation) lies inside x3_bound, elementwise, and (by construction) inside x3_f32_bound on
    every op; printed: the largest share used of x3_bound."""
    chain, w = vo.cpu_chain(precision, img, keep), vo.weights()
    for op in vo.graph(precision, keep):
        x = chain[op["src"]]
        ref = vo.op_ref(op, x, w)
        emu = vo.emulate_op(op, x, w, precision).astype(np.float64)
        err = np.abs(emu - ref["out"])
        if not op["convs"]:
            assert err.max() == 0.0, op["name"]
            continue
        if op["convs"] == ("block1_conv1",) and precision == "bf16x3":          # a float32 kernel on this handle
            assert np.abs(vo.op_ref32(op, x, w, precision) - ref["out"]).max() <= vo.f32_bound(ref["out"], vo.op_ref32(op, x, w, precision))
            continue
        bound, scalar = vo.x3_bound(op, x, ref, w, precision), vo.scalar_bound(emu, ref["out"])
        print("vgg16 ops bounds %s img=%d %s: contract err %.3g; x3_bound there %.3g (largest share %.3g); x3_f32_bound %.3g; |out| max %.3g"
              % (precision, img, op["name"], err.max(), bound.flat[err.argmax()], (err / bound).max(), scalar, np.abs(ref["out"]).max()))
        assert (bound > 0).all() and (err <= bound).all(), (op["name"], (err / bound).max())
        assert err.max() <= scalar
    tap = chain["block5_conv3"]
    ref = vo.head_ref(tap, w)
    reg, cls = vo.emulate_head(tap, w, precision)
    bound = vo.head_bounds(tap, ref, w, precision)
    assert (np.abs(reg - ref["reg"]) <= bound).all()
    print("vgg16 ops bounds %s img=%d head: reg err %.3g (largest share of the elementwise bound %.3g), cls err %.3g"
          % (precision, img, np.abs(reg - ref["reg"]).max(), (np.abs(reg - ref["reg"]) / bound).max(), np.abs(cls - ref["cls"]).max()))


MUTATIONS = [("lo*hi dropped", dict(parts=(1, 1, 0))), ("lo half of the output dropped", dict(drop_lo_out=True)),
             ("weight shift off by one", dict(shift_off=1)), ("pool before the bias", dict(pool_first=True))]


@pytest.mark.parametrize("what,kw", MUTATIONS, ids=[m[0].replace(" ", "-") for m in MUTATIONS])
def test_the_bounds_notice_a_wrong_kernel(what, kw):
    """Each wrong emulation leaves the ELEMENTWISE bound on at least one op of the case table's graphs, and the scalar bound on every
    split-precision op it applies to (module docstring)."""
    w = vo.weights()
    left_elementwise = []
    for precision, img, keep in CHAINS:
        chain = vo.cpu_chain(precision, img, keep)
        for op in vo.graph(precision, keep):
            if not op["convs"] or (op["convs"] == ("block1_conv1",) and precision == "bf16x3"):
                continue
            if ("pool_first" in kw and not op["pool"]) or ("drop_lo_out" in kw and op["out_f32"]):
                continue
            x = chain[op["src"]]
            ref = vo.op_ref(op, x, w)
            bound, scalar = vo.x3_bound(op, x, ref, w, precision), vo.x3_f32_bound(op, x, ref, w, precision)
            err = np.abs(vo.emulate_op(op, x, w, precision, **kw).astype(np.float64) - ref["out"])
            ratio = (err / bound).max()
            print("vgg16 ops mutation '%s' %s img=%d%s %s: err %.3g = %.3g x3_f32_bound, largest share of x3_bound %.3g"
                  % (what, precision, img, " keep" if keep else "", op["name"], err.max(), err.max() / scalar, ratio))
            assert err.max() > scalar, (what, precision, op["name"], err.max(), scalar)
            if ratio > 1.0:
                left_elementwise.append((precision, op["name"]))
    assert left_elementwise, what
    print("vgg16 ops mutation '%s' leaves x3_bound on: %s" % (what, left_elementwise))
