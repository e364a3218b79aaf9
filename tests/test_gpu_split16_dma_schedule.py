"""Where conv3x3_split16_dma_kernel issues its LDS-DMA pieces inside a tap's interval is timing only: a misplaced piece shows up
as a stale or an early LDS read, rarely and in single values.  So every path of the schedule is run ten times on small-integer
inputs, where the f16x3 / bf16x3 arithmetic is exact in any order, and compared with `==` against an integer convolution.  Every
case asserts the kernel it is routed to: at small grids the launcher prefers the register-staged kernel."""
import ctypes
import os
import subprocess
import sys
import textwrap

import numpy as np
import pytest
import torch

from oracle import bbox_oracle as bo
from oracle import conv_oracle as cv
from tf_rpn_amd import _lib as L
from tf_rpn_amd.models._rpn_model import RPNModel, synthetic_weights

pytestmark = pytest.mark.gpu

RUNS = 10
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _route(B, H, W, Cin, Cout, pool=False):
    """The launcher's own choice for a 3x3 split conv: rpn::conv3x3_split16_variant -> "dma,128" | "dma,64" | "reg,.." | None."""
    fn = getattr(ctypes.CDLL(L.LIB_PATH), "_ZN3rpn23conv3x3_split16_variantEiiiiiib")
    fn.restype = ctypes.c_char_p
    fn.argtypes = [ctypes.c_int] * 6 + [ctypes.c_bool]
    cout_pad = 64 if Cout <= 64 else (Cout + 127) // 128 * 128          # split_cout_pad
    v = fn(B, H, W, Cin, Cout, cout_pad, pool)
    return v.decode() if v else None


def _walked_batch():
    """Images of 32 x 32 (four 8-row tiles each) so that a layer with two N tiles has more than 2 x CUs tiles: every persistent
    workgroup walks at least two (72 at 256 CUs)."""
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    return 2 * cus // 8 + 8


# name -> (B or None: _walked_batch(), H, W, Cin, Cout, the route it must take or None); the path of the schedule it reaches.
# The 64-wide LDS-DMA tile runs grids of more than 128 tiles of 64 channels that are fewer than 256 tiles of 128.
LAYERS = {
    "one_pair_64": (12, 9, 40, 64, 192, "dma,64"),      # one slice pair per tile: the first interval's "no wait" and the last slice's look-ahead in one pair
    "pairs_64": (12, 16, 64, 192, 192, "dma,64"),       # several pairs
    "wide64": (8, 31, 31, 256, 320, "dma,64"),          # 64-wide tiles, ragged in both directions
    "wide64_two_tiles": (12, 31, 31, 256, 512, "dma,64"),   # 384 tiles of 64: workgroups walk two, the hand-over DMAs run under the last taps
    "two_tiles": (None, 32, 32, 64, 256, "dma,128"),    # 128 wide, one pair, every workgroup walks >= 2 tiles
    "n_tile_changes": (None, 32, 32, 128, 384, "dma,128"),  # ... with the N tile changing between a workgroup's tiles
    # the same shapes at the batch sizes of one or two images: the register-staged kernel takes these (kept: they must stay exact too)
    "one_pair_b1": (1, 9, 40, 64, 192, None),
    "pairs_b1": (1, 16, 64, 192, 128, None),
    "wide64_b2": (2, 31, 31, 256, 320, None),
}
_cache = {}


def _layer(name):
    """Inputs and the integer reference of a case: built once, shared by both precisions, never written to."""
    if name not in _cache:
        B, H, W, Cin, Cout, _ = LAYERS[name]
        B = B or _walked_batch()
        rng = np.random.RandomState(H * 1000 + Cin + Cout)
        x = torch.from_numpy(rng.randint(-3, 4, size=(B, H, W, Cin)).astype(np.float32))
        w = torch.from_numpy(rng.randint(-3, 4, size=(3, 3, Cin, Cout)).astype(np.float32))
        b = torch.from_numpy(rng.randint(-5, 6, size=(Cout,)).astype(np.float32))
        # inputs and weights are their own 16-bit `hi` halves (`lo` = 0), every partial sum is an integer below 2^24 (exact in
        # float32 in any order) and every output one below 2^16 (a bfloat16 pair holds it)
        assert 9 * Cin * 3 * 3 + 5 < 2 ** 16
        ref = torch.nn.functional.conv2d(x.double().permute(0, 3, 1, 2), w.double().permute(3, 2, 0, 1), b.double(), padding=1)
        ref = ref.clamp_(min=0).permute(0, 2, 3, 1).contiguous().float()
        _cache[name] = (x.cuda(), w.cuda(), b.cuda(), ref.cuda())
    return _cache[name]


def _same(got, ref, what):
    if not torch.equal(got, ref):
        wrong = (got != ref).nonzero()
        at = tuple(wrong[0].tolist())
        raise AssertionError("%s: %d wrong values, first at %s: got %r want %r" % (what, len(wrong), at, got[at].item(), ref[at].item()))


@pytest.mark.parametrize("precision", ["f16x3", "bf16x3"])
@pytest.mark.parametrize("name", list(LAYERS))
def test_layer_is_exact_on_integers_ten_times(name, precision):
    x, w, b, ref = _layer(name)
    B, H, W, Cin = x.shape
    Cout = w.shape[3]
    want = LAYERS[name][5]
    if want:
        assert _route(B, H, W, Cin, Cout) == want, "the case no longer reaches the kernel it is about"
    out = torch.empty((B, H, W, Cout), device="cuda")
    for run in range(RUNS):
        out.fill_(float("nan"))
        L.check(L.lib().rpn_conv2d(L.ptr(x), B, H, W, Cin, L.ptr(w), L.ptr(b), 3, 3, Cout, 1, 1, 1, H, W, L.ACTS["relu"],
                                   L.PRECISIONS[precision], L.ptr(out), L.stream_ptr()), "rpn_conv2d")
        _same(out, ref, "run %d" % run)


# ---- the POOL and K-tree instantiations: only a backbone's handle launches them -------------------------------------------------
# A VGG16 whose every activation is a small integer: images of 0 / 1, centre-tap identity kernels without bias everywhere except
#   the layer in front of the one under test: a centre tap of -1 / 0 / 1 (the three image channels fan out over all of its outputs;
#       values 0 .. 3 behind the ReLU),
#   the layer under test: all nine taps -2 .. 2 and a bias of -5 .. 5 (outputs below 9 * 512 * 3 * 2 + 5 < 2^15),
#   rpn_reg: output c sums the channels j = c (mod 36) of rpn_conv (below 2^24), so that `reg` sees every channel; rpn_cls: zeros.
# The feature map (block5_conv3) and `reg` must then equal the float64 oracle's.  Two different images, repeated to fill the batch.
_int_cache = {}


def _integer_vgg16(img, under_test, before):
    key = (img, under_test)
    if key not in _int_cache:
        hp = bo.get_hyper_params("vgg16", img_size=img) if img != 500 else bo.get_hyper_params("vgg16")
        weights = synthetic_weights("vgg16", hp, seed=1)               # (for the names and shapes)
        rng = np.random.RandomState(img + len(under_test))
        for name, e in weights.items():
            R, S, Cin, Cout = e["kernel"].shape
            k = np.zeros((R, S, Cin, Cout), dtype=np.float32)
            bias = np.zeros((Cout,), dtype=np.float32)
            if name == under_test:
                k[:] = rng.randint(-2, 3, size=k.shape)
                bias[:] = rng.randint(-5, 6, size=bias.shape)
            elif name == before:
                k[R // 2, S // 2] = rng.randint(-1, 2, size=(Cin, Cout))
            elif name == "rpn_reg":
                k[0, 0, np.arange(Cin), np.arange(Cin) % Cout] = 1
            elif name != "rpn_cls":
                n = min(Cin, Cout)
                k[R // 2, S // 2, np.arange(n), np.arange(n)] = 1
            e["kernel"], e["bias"] = k, bias
        two = np.random.RandomState(img).randint(0, 2, size=(2, img, img, 3)).astype(np.float32)
        reg, _cls, feat = cv.rpn_forward("vgg16", two, weights, dtype=torch.float64, return_features=True)
        assert feat.max() < 2 ** 15 and np.abs(reg).max() < 2 ** 24 and feat.max() > 0 and np.abs(reg).max() > 0
        _int_cache[key] = (hp, weights, torch.from_numpy(two).cuda(), torch.from_numpy(np.ascontiguousarray(reg)).cuda(),
                           torch.from_numpy(np.ascontiguousarray(feat)).cuda())
    return _int_cache[key]


def _handle_is_exact_ten_times(img, under_test, before, precision, max_batch, batches, kernel, pooled):
    hp, weights, two, reg_ref, feat_ref = _integer_vgg16(img, under_test, before)
    model = RPNModel("vgg16", hp, precision=precision, max_batch=max_batch)
    model.set_weights(weights)
    ops = model.ops()
    i = [op["name"] for op in ops].index(under_test)
    assert kernel in ops[i]["kernel"], ops[i]["kernel"]                 # (the handle's choice at max_batch images)
    assert ops[i + 1]["kernel"].startswith("fused:") == pooled, ops[i + 1]
    for B in batches:
        pick = torch.arange(B, device="cuda") % 2
        imgs = two[pick].contiguous()
        for run in range(RUNS):
            reg, _cls = model.predict_on_batch(imgs)
            _same(reg.reshape(reg_ref[pick].shape), reg_ref[pick], "%d images, run %d, reg" % (B, run))
            feat = model.get_activation(model.tap_layer, batch=B)
            _same(feat, feat_ref[pick], "%d images, run %d, feature map" % (B, run))
    assert not model.status()["f16_range"]


@pytest.mark.parametrize("precision", ["f16x3", "bf16x3"])
@pytest.mark.parametrize("B,width", [(2, 64), (7, 128)])
def test_pooled_tile_is_exact_on_integers_ten_times(B, width, precision):
    """block4_conv3 + its 2x2 pool at 37 x 37 (odd: the pool's 'valid' floor), 512 -> 512: 80 tiles of 128 channels at two images
    (the 64-wide pooled tile), 280 at seven (the 128-wide one).  Nothing pools behind it, so the feature map shows every value."""
    assert _route(B, 37, 37, 512, 512, pool=True) == "dma,%d" % width
    _handle_is_exact_ten_times(300, "block4_conv3", "block4_conv2", precision, B, [B], "split16_dma<%s,%d>" % (precision, width), True)


@pytest.mark.parametrize("precision", ["f16x3", "bf16x3"])
def test_rpn_conv_k_tree_is_exact_on_integers_ten_times(precision):
    """rpn_conv at full size, as test_rpn_conv_k_tree_same_bits_at_every_split_factor builds it: eight images (the persistent 64-wide
    kernel folds the four leaves inside its tile loop) and three (two workgroups per tile, half of K each, the head adds the slabs)."""
    _handle_is_exact_ten_times(500, "rpn_conv", "block5_conv3", precision, 8, [8, 3], "split16_dma<%s,64>" % precision, False)


def test_dynamic_tile_schedule_is_exact_on_integers_subprocess():
    """RPN_S16_DYN=1 is read once per process: the cases whose workgroups walk several tiles, at both tile widths, in a child process
    with the tile queue on -- the next tile is then known only from tap 6 on, in time for the last slice's look-ahead DMAs."""
    code = textwrap.dedent("""
        import sys
        sys.path.insert(0, %r)
        from tests.test_gpu_split16_dma_schedule import test_layer_is_exact_on_integers_ten_times as run
        for precision in ("f16x3", "bf16x3"):
            run("n_tile_changes", precision)
            run("wide64_two_tiles", precision)
        print("dynamic schedule exact")
    """ % ROOT)
    r = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, RPN_S16_DYN="1"), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "dynamic schedule exact" in r.stdout
