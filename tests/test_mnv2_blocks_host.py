"""CPU suite of the one-block-at-a-time MobileNetV2 tests (tests/mnv2_blocks.py, tests/test_gpu_mnv2_blocks.py): the two test hooks
of the C ABI where they need no device, the case table classified through rpn_model_ir_launch_info, and the f16x3 bound proved
against a numpy emulation of the arithmetic contract -- inside the bound as specified, outside it with any one product dropped."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import mnv2_blocks as mb  # noqa: E402
from test_det_head_host import lib  # noqa: E402,F401  (fixture)
from tf_rpn_amd import _lib as L  # noqa: E402
from tf_rpn_amd.models._rpn_model import RPNModel  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ["rpn_model_forward_to", "rpn_model_ir_launch_info"]


def _handle(case):
    return RPNModel("mobilenet_v2", mb.hyper(case["img"]), precision=case["precision"], max_batch=case["max_batch"])


def test_new_symbols_declared_exported_bound(lib):
    code = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "rpn_hip.h")).read(), flags=re.S)
    raw = ctypes.CDLL(L.LIB_PATH)
    for name in NEW_SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, code), "%s is not declared" % name
        assert hasattr(raw, name) and name in L.exported_symbols()
    for i, route in enumerate(RPNModel.IR_ROUTES):
        assert re.search(r"#define RPN_IR_ROUTE_%s %d\b" % (route.upper(), i), code), route
    assert lib.rpn_abi_version() == 1


@pytest.mark.parametrize("case", mb.CASES, ids=mb.case_ids())
def test_ir_launch_info_matches_the_case_table(lib, case):
    """Host arithmetic only (a handle is created without a device): every block of every case at every batch size of the table has
    the form the table expects; the tile count is the grid's."""
    m = _handle(case)
    for B in case["forms"]:
        for k in range(mb.NBLOCKS):
            assert mb.form(m, k, B) == mb.expected_form(case, k, B), (case["id"], k, B)
    if case["precision"] != "f16x3":
        assert all(mb.form(m, k, B)[0] in mb.F32_ROUTES for B in case["forms"] for k in range(mb.NBLOCKS))


def test_case_table_reaches_every_form(lib):
    """Every form the block launchers can take on a product build occurs in the table, classified through the query: a changed
    threshold cannot silently empty a class."""
    seen = set()
    for case in mb.CASES:
        m = _handle(case)
        for B in case["forms"]:
            for k in range(mb.NBLOCKS):
                seen.add((case["precision"] == "f16x3", k) + mb.form(m, k, B))
    x3 = {s[1:] for s in seen if s[0]}
    f32 = {s[1:] for s in seen if not s[0]}
    for chunk in (48, 16):
        for ks in (3, 1):
            assert (3, "ir_block_hrx3", chunk, ks) in x3, (chunk, ks)
    for ks in (4, 2, 1):
        assert (6, "ir_block_hrx3", 48, ks) in x3, ks
    for ks in (6, 3, 2, 1):
        assert any((k, "ir_block_x3", 32, ks) in x3 for k in (4, 5)), ks                 # 32 -> 192 -> 32
        assert any((k, "ir_block_x3", 32, ks) in x3 for k in (7, 8, 9)), ks              # 64 -> 384 -> 64
        assert (10, "ir_block_x3", 32, ks) in x3 and any((k, "ir_block_x3", 32, ks) in x3 for k in (11, 12)), ks   # -> 96
    assert {s[1] for s in x3 if s[0] in (4, 5)} == {"ir_block_x3", "ir_block_hrx3"}
    assert {s[1] for s in x3 if s[0] in (1, 2)} == {"ir_block_hrx3"} and {s[1] for s in x3 if s[0] == 0} == {"stem"}
    assert {s[1] for s in f32 if s[0] == 3} == {"ir_block", "ir_block_hr"}
    assert {s[1] for s in f32 if s[0] in (1, 2)} == {"ir_block_hr"} and {s[1] for s in f32 if s[0] >= 4} == {"ir_block"}


def test_ir_launch_info_errors(lib):
    m = RPNModel("mobilenet_v2", mb.hyper(128), precision="f16x3", max_batch=4)
    info = (ctypes.c_int * 4)()
    name = mb.tensor_name(3).encode()
    assert lib.rpn_model_ir_launch_info(m._h, name, 4, info) == L.RPN_OK
    for bad in (0, -1, 5):
        assert lib.rpn_model_ir_launch_info(m._h, name, bad, info) == L.RPN_ERR_INVALID
        assert b"outside [1, 4]" in lib.rpn_last_error()
        with pytest.raises(ValueError):
            m.ir_launch_info(mb.tensor_name(3), bad)
    # an unknown name; tensors that exist but are not written by a fused block (a plain conv, the caller's images); the parts of a block
    for bad in ("block_99_project", "block_13_expand", "input", "block_3_expand", "block_3_depthwise", "Conv1", ""):
        assert lib.rpn_model_ir_launch_info(m._h, bad.encode(), 1, info) == L.RPN_ERR_INVALID, bad
        with pytest.raises(ValueError):
            m.ir_launch_info(bad, 1)
    assert lib.rpn_model_ir_launch_info(None, name, 1, info) == L.RPN_ERR_INVALID
    assert lib.rpn_model_ir_launch_info(m._h, None, 1, info) == L.RPN_ERR_INVALID
    assert lib.rpn_model_ir_launch_info(m._h, name, 1, None) == L.RPN_ERR_INVALID
    # VGG16 has no fused block; the unfused MobileNetV2 graph (every activation kept) has the tensor, written by a plain conv
    v = RPNModel("vgg16", mb.hyper(96), precision="f16x3", max_batch=2)
    assert lib.rpn_model_ir_launch_info(v._h, b"block1_pool", 1, info) == L.RPN_ERR_INVALID
    u = RPNModel("mobilenet_v2", mb.hyper(128), precision="f32", max_batch=2, keep_activations=True)
    assert lib.rpn_model_ir_launch_info(u._h, name, 1, info) == L.RPN_ERR_INVALID
    assert b"not a fused MobileNetV2 block" in lib.rpn_last_error()


def test_forward_to_argument_checks(lib):
    """The checks that come before any device use."""
    m = RPNModel("mobilenet_v2", mb.hyper(128), precision="f32", max_batch=2)
    one = ctypes.c_void_p(16)                   # never dereferenced: every call below is refused first
    name = mb.tensor_name(3).encode()
    assert lib.rpn_model_forward_to(None, name, one, 1, one, None) == L.RPN_ERR_INVALID
    assert lib.rpn_model_forward_to(m._h, None, one, 1, one, None) == L.RPN_ERR_INVALID
    assert lib.rpn_model_forward_to(m._h, name, None, 1, one, None) == L.RPN_ERR_INVALID
    assert lib.rpn_model_forward_to(m._h, name, one, 1, None, None) == L.RPN_ERR_INVALID
    for bad in (0, 3):
        assert lib.rpn_model_forward_to(m._h, name, one, bad, one, None) == L.RPN_ERR_INVALID
    for bad in (b"input", b"block_99_project", b"block_3_expand", b"rpn_reg"):
        assert lib.rpn_model_forward_to(m._h, bad, one, 1, one, None) == L.RPN_ERR_INVALID, bad
    assert lib.rpn_model_forward_to(m._h, name, one, 1, one, None) == L.RPN_ERR_INVALID
    assert b"never set" in lib.rpn_last_error()


# ---- the bound against the contract's emulation -------------------------------------------------------------------------------------------
SIZES = (128, 150, 75)          # the image sizes of the f16x3 cases


@pytest.mark.parametrize("img", SIZES)
def test_case_inputs_meet_the_conditions(img):
    w = mb.weights()
    for k, x in enumerate(mb.cpu_chain(img)):
        mb.input_conditions(k, mb.cpu_block(img, k)[1] if k else mb.block_ref(k, x, w, torch.float64), w, "img %d" % img)


@pytest.mark.parametrize("img", SIZES)
def test_x3_bounds_hold_for_the_contract(img):
    """emulate_block (the contract, exact accumulation) lies inside x3_bound, elementwise, and inside x3_f32_bound on every block
    shape; printed: the largest share used of each."""
    w = mb.weights()
    for k in range(1, mb.NBLOCKS):
        x, ref, bound, scalar = mb.cpu_block(img, k)
        err = np.abs(mb.emulate_block(k, x, w).astype(np.float64) - ref["out"])
        print("mnv2 x3 bounds img=%d block %d: contract err %.3g; x3_bound there %.3g (largest share %.3g, bound max %.3g); "
              "x3_f32_bound %.3g; |out| max %.3g" % (img, k, err.max(), bound.flat[err.argmax()], (err / bound).max(), bound.max(),
                                                     scalar, np.abs(ref["out"]).max()))
        assert (bound > 0).all() and (err <= bound).all(), (img, k, (err / bound).max())
        assert err.max() <= scalar, (img, k, err.max(), scalar)


DROPS = [(g, p) for g in ("expand", "project") for p in range(3)]


@pytest.mark.parametrize("img", (75,))
@pytest.mark.parametrize("gemm,part", DROPS, ids=["%s-%s" % (g, ("hihi", "hilo", "lohi")[p]) for g, p in DROPS])
def test_x3_bounds_reject_a_dropped_product(gemm, part, img):
    """The same emulation with one of the three float16 products of one GEMM left out must leave x3_f32_bound on EVERY block, and
    x3_bound too when the product is hi hi (tests/mnv2_blocks.py says why x3_bound cannot see a cross product): the bounds are tight
    enough to see a kernel that drops a term."""
    w = mb.weights()
    parts = tuple(0 if i == part else 1 for i in range(3))
    kw = {"parts_e": parts} if gemm == "expand" else {"parts_p": parts}
    for k in range(1, mb.NBLOCKS):
        x, ref, bound, scalar = mb.cpu_block(img, k)
        err = np.abs(mb.emulate_block(k, x, w, **kw).astype(np.float64) - ref["out"])
        print("mnv2 x3 drop %s part %d img=%d block %d: err %.3g = %.3g x3_f32_bound, largest share of x3_bound %.3g"
              % (gemm, part, img, k, err.max(), err.max() / scalar, (err / bound).max()))
        assert err.max() > scalar, (img, k, gemm, part, err.max(), scalar)
        if part == 0:
            assert (err > bound).any(), (img, k, gemm)
