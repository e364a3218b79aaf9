"""The inference RPN head at every anchor count K and in every launch form.

K = len(anchor_ratios) * len(anchor_scales) selects rpn_head_kernel<NB, MB, PXV> with NB = ceil(5K / 16) = 1 .. 6 (K <= 19), per
launch one of three grids -- 32 pixels per workgroup (MB = 2, from 8161 pixels on), 16 (MB = 1), 4 (PXV = 4: at most 1024 pixels in
2 or 4 partial-sum slabs) -- and 1, 2 or 4 slabs of a split-K rpn_conv; from K = 20 on, and under RPN_HEAD_SPLITK=0, the float32
implicit GEMM with two outputs cut at column 4K.  Every case asks rpn_model_head_launch_info which form it ran and asserts it.

Reference: float64 rpn_conv + rpn_reg | rpn_cls (oracle/conv_oracle._head) on the library's OWN feature tap of that forward, so the
comparison isolates the two layers; bounds in tests/anchor_counts.py.  Across forms the library promises the same bits for the same
image at every batch size of one handle: torch.equal.

Forms run here, (NB, pixels per workgroup, slabs):
  test_head_widths            f32: (1..6, 16, 1); f16x3: (1..6, 4, 4)
  test_head_slabs_px4         (1 | 4 | 6, 4, 4), (.., 4, 2), (.., 16, 1)
  test_head_slabs_16px        (1 | 6, 16, 4), (.., 16, 2), (.., 16, 1)
  test_head_mb2               (1..6, 32, 1) and (1..6, 16, 1)
(32 pixels per workgroup with 2 or 4 slabs cannot be reached through a model: rpn_conv splits K only on grids of at most 256
workgroups of 4 x 32 pixels x 64 channels -- 32 pixel tiles for the 512 output channels, at most 4096 pixels -- and MB = 2 starts at
8161.  No instantiation is missed by that: the slab count is a run-time argument of the same 18 kernels.)

Measured on an MI355X, largest error against float64 over the cases of this file (every case prints its own):
  f32     reg 2.3e-6, cls 4.2e-6 (MobileNetV2 at 528; VGG16 at 80: 6.6e-7, 1.6e-6) against bounds of 1.4e-6 .. 7.2e-6: the error
          is a quarter to nine tenths of the bound, which is 4 x torch float32's own distance + 1e-6 (closest: K = 16 at 528, cls
          4.23e-6 under 4.79e-6)
  f16x3   reg 8.5e-7, cls 1.2e-6 (bound 1e-4)
  bf16x3  reg 2.0e-6, cls 4.2e-6 (bound 1e-4)
"""
import os
import subprocess
import sys
import textwrap

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import anchor_counts as ac  # noqa: E402

pytestmark = pytest.mark.gpu


def nb_of(K):
    return (5 * K + 15) // 16


# n_reg = 4K on a 16-column block boundary: K = 4, 8, 12, 16; inside a block: the others; 5K = 80 fills the last block (K = 16);
# K = 13 leaves ONE live column in the last block; K = 1: five columns in all.
WIDTHS = [(1, 1), (3, 1), (4, 2), (6, 2), (8, 3), (12, 4), (13, 5), (16, 5), (19, 6)]


def _widths(backbone, K, nb, precision):
    assert nb_of(K) == nb
    model, weights = ac.make(backbone, 80, K, precision, 3)
    # 25 pixels per image: a ragged last workgroup in every form.  f32: rpn_conv on the float32 GEMM, one slab, 16-pixel workgroups;
    # f16x3: rpn_conv split four ways along K at these grids, the head adds four slabs in 4-pixel workgroups
    want = ("splitk", nb, 16, 1) if precision == "f32" else ("splitk", nb, 4, 4)
    assert ac.form(model, 1) == want and ac.form(model, 3) == want
    assert ac.head_kernel(model) == "rpn_head_splitk<%d>" % nb
    x = ac.images(3, 80)
    full = ac.forward(model, x)
    assert tuple(full[0].shape) == (3, 5, 5, 4 * K) and tuple(full[1].shape) == (3, 5, 5, K)
    ac.check_float64(model, weights, full[0], full[1], (0, 1, 2), "widths %s K=%d" % (backbone, K))
    one = ac.forward(model, x[:1])
    assert ac.same_bits(ac.row(one, 0), ac.row(full, 0))


@pytest.mark.parametrize("precision", ["f32", "f16x3"])
@pytest.mark.parametrize("K,nb", WIDTHS)
def test_head_widths(K, nb, precision):
    """VGG16 at img_size 80 (F = 5), one and three images of a handle of three.  Measured: f32 reg <= 5.4e-7 (bounds 1.4e-6 ..
    1.8e-6), cls <= 1.1e-6 (bounds 1.7e-6 .. 2.6e-6); f16x3 reg <= 2.3e-7, cls <= 5.7e-7 (bound 1e-4)."""
    _widths("vgg16", K, nb, precision)


@pytest.mark.parametrize("precision", ["f32", "f16x3"])
@pytest.mark.parametrize("K,nb", [(4, 2), (19, 6)])
def test_head_widths_mobilenet_v2(K, nb, precision):
    """The 576-channel tap: rpn_conv has 18 slices of 32 channels instead of 16."""
    _widths("mobilenet_v2", K, nb, precision)


@pytest.mark.parametrize("precision", ["f16x3", "bf16x3"])
@pytest.mark.parametrize("K", [3, 12, 19])
def test_head_slabs_px4(K, precision):
    """VGG16 at img_size 80 on a handle of 20 images: the batch sizes at which the query reports 4, 2 and 1 slabs (conv3x3_split16_ksplit:
    B <= 8, 9 .. 16, 17 .. 20 -- taken from the query, not from this sentence).  4 and 2 slabs run 4-pixel workgroups (at most 500
    pixels), one slab 16-pixel ones.  The same image must give the same bits at all three."""
    nb = nb_of(K)
    model, weights = ac.make("vgg16", 80, K, precision, 20)
    by_slabs = {}
    for B in range(1, 21):
        by_slabs.setdefault(ac.form(model, B)[3], []).append(B)
    assert sorted(by_slabs) == [1, 2, 4], by_slabs
    b4, b2, b1 = min(by_slabs[4]), by_slabs[2][len(by_slabs[2]) // 2], max(by_slabs[1])
    assert ac.form(model, b4) == ("splitk", nb, 4, 4) and ac.form(model, b2) == ("splitk", nb, 4, 2)
    assert ac.form(model, b1) == ("splitk", nb, 16, 1)
    x = ac.images(20, 80)
    big = ac.forward(model, x[:b1])
    ac.check_float64(model, weights, big[0], big[1], (0, b1 - 1), "slabs/px4 K=%d" % K)
    for B in (b2, b4):
        out = ac.forward(model, x[:B])
        ac.check_float64(model, weights, out[0], out[1], (0, B - 1), "slabs/px4 K=%d" % K)
        assert ac.same_bits(ac.row(out, 0), ac.row(big, 0)) and ac.same_bits(ac.row(out, B - 1), ac.row(big, B - 1)), B


@pytest.mark.parametrize("K", [3, 19])
def test_head_slabs_16px(K):
    """VGG16 at img_size 384 (F = 24), f16x3, 2 / 4 / 8 images of a handle of 8: more than 1024 pixels in 4, 2 and 1 slabs --
    16-pixel workgroups that add slabs."""
    nb = nb_of(K)
    model, weights = ac.make("vgg16", 384, K, "f16x3", 8)
    for B, slabs in ((2, 4), (4, 2), (8, 1)):
        assert ac.form(model, B) == ("splitk", nb, 16, slabs), (B, ac.form(model, B))
    x = ac.images(8, 384)
    outs = {B: ac.forward(model, x[:B]) for B in (8, 4)}
    outs[2] = ac.forward(model, x[:2])
    ac.check_float64(model, weights, outs[2][0], outs[2][1], (0,), "slabs/16px K=%d" % K)
    for B in (4, 8):
        assert ac.same_bits(ac.row(outs[B], 0), ac.row(outs[2], 0)), B


@pytest.mark.parametrize("K,nb,seed", [(3, 1, 103), (6, 2, 206), (8, 3, 108), (12, 4, 112), (16, 5, 216), (19, 6, 119)])
def test_head_mb2(K, nb, seed):
    """MobileNetV2 at img_size 528 (F = 33), f32, 8 images: 8712 pixels, above 8160 and not a multiple of 32 -- 32-pixel workgroups
    (MB = 2) with a ragged last one.  Images 0 and 7 alone run the MB = 1 form and must equal the batch's rows bit for bit.
    Every NB, not only the issue's K = 3, 12, 19: each <NB, 2> is an instantiation of its own.

    The weight seeds are those of the other cases (100 + K) but for K = 6 and 16: there the ReLU6 tap times He-normal rpn_cls puts
    the largest of the 8712 K objectness logits at 17.96 and 16.82 (float64 reference on the CPU), and from 16.7 on a float32 sigmoid
    IS 1.0, so `cls < 1` would fail for any float32 evaluation; with the seeds used here the largest logit over all eight images
    is 4.2, 10.8, 11.5, 14.5, 13.6, 14.5."""
    assert nb_of(K) == nb
    model, weights = ac.make("mobilenet_v2", 528, K, "f32", 8, seed=seed)
    assert ac.form(model, 8) == ("splitk", nb, 32, 1) and ac.form(model, 1) == ("splitk", nb, 16, 1)
    x = ac.images(8, 528)
    full = ac.forward(model, x)
    ac.check_float64(model, weights, full[0], full[1], (7,), "MB=2 K=%d" % K)
    for i in (0, 7):
        one = ac.forward(model, x[i:i + 1])
        assert ac.same_bits(ac.row(one, 0), ac.row(full, i)), i


@pytest.mark.parametrize("precision", ["f32", "f16x3"])
@pytest.mark.parametrize("K", [20, 26])
def test_head_fallback(K, precision):
    """5K > 96: the head on the float32 implicit GEMM with two outputs; the reg | cls cut falls at columns 80 and 104, inside an N
    tile, and the 100 / 130 columns span several N tiles."""
    ac.fallback_case("vgg16", 80, K, precision, 3, (0, 1, 2))


def test_head_fallback_larger_grid():
    """MobileNetV2 at img_size 528, two images: 2178 pixels, many M tiles."""
    ac.fallback_case("mobilenet_v2", 528, 20, "f32", 2, (1,))


def test_head_splitk_knob_off_subprocess():
    """RPN_HEAD_SPLITK=0 (documented product knob, read once per process): every K goes through the float32 GEMM.  K = 9 and 12 in
    both precisions hold the same bounds, and model.ops() does not name rpn_head_splitk."""
    code = textwrap.dedent("""
        import sys
        sys.path.insert(0, %r); sys.path.insert(0, %r)
        import anchor_counts as ac
        for K in (9, 12):
            for precision in ("f32", "f16x3"):
                ac.fallback_case("vgg16", 80, K, precision, 3, (0, 1, 2))
        print("knob off ok")
    """ % (ROOT, os.path.join(ROOT, "tests")))
    r = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, RPN_HEAD_SPLITK="0"), capture_output=True, text=True,
                       timeout=600)
    print(r.stdout)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "knob off ok" in r.stdout
