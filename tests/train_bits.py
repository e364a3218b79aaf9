"""Cases, seeded inputs and runners shared by tests/golden/make_train_kernel_bits.py (the recorder) and tests/test_gpu_train_bits.py:
the backward kernels of the training path through their public single-layer entries, each output reduced to the SHA-256 of its bytes.

The digests pin the ORDER of every sum: the inputs are real-valued (the builders of tests/test_gpu_backward.py), so two correct
float32 summation orders give different bits (order_sensitive below holds the builders to that on the CPU), which neither the
integer bit-exact tests (order-blind) nor the float64 parity tests (16 x float32 rounding) nor the determinism tests (a build
against itself) would notice."""
import hashlib
import zlib

import numpy as np
import torch

from tf_rpn_amd import _lib as L


# ---- data shaped like what the trainer feeds (as tests/test_gpu_backward.py builds it) ---------------------------------------------------
def dy_like(rng, shape):
    """ReLU-masked gradients: about half the entries exactly zero, the others spread over three decades."""
    v = rng.standard_normal(shape) * 10.0 ** rng.uniform(-3.0, 0.0, size=shape)
    v[rng.uniform(size=shape) < 0.5] = 0.0
    return v.astype(np.float32)


def relu_like(rng, shape):
    return np.maximum(rng.standard_normal(shape), 0.0).astype(np.float32)


def taps_like(rng, shape):
    """Depthwise 3x3 taps (He-scaled, fan-in 9)."""
    return (rng.standard_normal(shape) * np.sqrt(2.0 / 9.0)).astype(np.float32)


def image_like(rng, shape):
    """A preprocessed image: MobileNetV2's [-1, 1]."""
    return rng.uniform(-1.0, 1.0, size=shape).astype(np.float32)


# every (a, b) pair of builders whose products a kernel below sums
BUILDER_PAIRS = {"relu_like x dy_like": (relu_like, dy_like), "dy_like x taps_like": (dy_like, taps_like),
                 "image_like x dy_like": (image_like, dy_like)}


def order_sensitive(build_a, build_b, seed=0, n=4096, c=64):
    """Whether the float32 sum of a slab's n x c products, taken first to last and last to first, differs in at least one of the c
    elements.  (np.add.accumulate adds strictly in sequence.)"""
    rng = np.random.RandomState(seed)
    prod = build_a(rng, (n, c)) * build_b(rng, (n, c))
    assert prod.dtype == np.float32
    fwd = np.add.accumulate(prod, axis=0, dtype=np.float32)[-1]
    bwd = np.add.accumulate(prod[::-1], axis=0, dtype=np.float32)[-1]
    return bool((fwd != bwd).any())


# ---- the cases: the smallest at which each path can still go wrong -----------------------------------------------------------------------
# conv entries (B, H, W, Cin, Cout); depthwise (B, H, W, C); the stem (B, H, W, Cout); 1x1 (P, Cin, Cout)
CASES = [
    ("rpn_conv3x3_wgrad", (1, 1, 2, 4, 4)),                # fewer pixels than leaves
    ("rpn_conv3x3_wgrad", (2, 7, 5, 20, 36)),
    ("rpn_conv3x3_wgrad", (1, 9, 33, 64, 132)),            # ragged tiles in both directions
    ("rpn_conv3x3_wgrad_wide", (1, 1, 1, 3, 4)),
    ("rpn_conv3x3_wgrad_wide", (1, 3, 5, 4, 20)),          # one leaf
    ("rpn_conv3x3_wgrad_wide", (1, 40, 27, 12, 132)),      # two leaves, the tree loop skipped
    ("rpn_conv3x3_wgrad_wide", (2, 62, 47, 128, 68)),      # 8 leaves, two tree levels
    ("rpn_conv3x3_wgrad_wide", (1, 9, 11, 3, 8)),          # Cin 3: the padded image
    ("rpn_dwconv3x3_dgrad", (1, 3, 3, 8)), ("rpn_dwconv3x3_dgrad", (3, 5, 5, 384)), ("rpn_dwconv3x3_dgrad", (2, 14, 14, 576)),
    ("rpn_dwconv3x3_wgrad", (1, 3, 3, 8)), ("rpn_dwconv3x3_wgrad", (3, 5, 5, 384)), ("rpn_dwconv3x3_wgrad", (2, 14, 14, 576)),
    ("rpn_dwconv3x3_s2_dgrad", (1, 1, 1, 4)), ("rpn_dwconv3x3_s2_dgrad", (1, 2, 2, 4)),
    ("rpn_dwconv3x3_s2_dgrad", (1, 7, 12, 8)),             # odd and even sides: pt != pl
    ("rpn_dwconv3x3_s2_dgrad", (2, 9, 9, 144)), ("rpn_dwconv3x3_s2_dgrad", (2, 10, 10, 96)),
    ("rpn_dwconv3x3_s2_wgrad", (1, 1, 1, 4)), ("rpn_dwconv3x3_s2_wgrad", (1, 2, 2, 4)), ("rpn_dwconv3x3_s2_wgrad", (1, 7, 12, 8)),
    ("rpn_dwconv3x3_s2_wgrad", (2, 9, 9, 144)), ("rpn_dwconv3x3_s2_wgrad", (2, 10, 10, 96)),
    ("rpn_conv3x3_s2_cin3_wgrad", (1, 6, 5, 40)), ("rpn_conv3x3_s2_cin3_wgrad", (1, 9, 13, 32)),
    ("rpn_conv3x3_s2_cin3_wgrad", (1, 128, 128, 32)),      # 4096 output pixels: 64 leaves, two groups of 32
    ("rpn_conv1x1_wgrad", (40, 96, 96)),                   # one leaf
    ("rpn_conv1x1_wgrad", (392, 96, 576)),                 # several leaves through the slab tree
]


def s2_out(n):
    """Output pixels of one side of n input pixels under ZeroPadding2D(correct_pad) + 3x3 stride-2 'valid'."""
    return (n + n % 2 + 1 - 3) // 2 + 1


def build_inputs(entry, shape, seed):
    """The named float32 inputs of a case, in the order the entry takes them."""
    rng = np.random.RandomState(seed)
    if entry in ("rpn_conv3x3_wgrad", "rpn_conv3x3_wgrad_wide"):
        B, H, W, Cin, Cout = shape
        return [relu_like(rng, (B, H, W, Cin)), dy_like(rng, (B, H, W, Cout))]
    if entry == "rpn_conv1x1_wgrad":
        P, Cin, Cout = shape
        return [relu_like(rng, (P, Cin)), dy_like(rng, (P, Cout))]
    B, H, W, C = shape
    s2 = "_s2_" in entry
    dy = dy_like(rng, (B, s2_out(H), s2_out(W), C) if s2 else (B, H, W, C))
    if entry.endswith("_dgrad"):
        return [dy, taps_like(rng, (3, 3, C))]
    if entry == "rpn_conv3x3_s2_cin3_wgrad":
        return [image_like(rng, (B, H, W, 3)), dy]
    return [relu_like(rng, (B, H, W, C)), dy]


def seed_of(entry, shape):
    """The case's seed: from its name and shape, stepped past draws that leave an input all zero (dy_like zeroes half its entries: a
    one-pixel case can draw nothing else)."""
    seed = zlib.crc32(("%s %s" % (entry, tuple(shape))).encode()) % (1 << 20)
    while not all(a.any() for a in build_inputs(entry, shape, seed)):
        seed += 1
    return seed


def run_case(lib, entry, shape, seed):
    """Runs the entry once on the current device; {output name: its bytes}.  The workspace is filled with NaN bit patterns, so a read
    of scratch nobody wrote shows in the digest."""
    a, b = [torch.from_numpy(v).cuda() for v in build_inputs(entry, shape, seed)]

    def scratch(nbytes):
        return torch.full((max(nbytes, 16),), 0xFF, dtype=torch.uint8, device="cuda")

    def out(*dims):
        return torch.full(dims, float("nan"), dtype=torch.float32, device="cuda")

    s = L.stream_ptr()
    outs = {}
    if entry in ("rpn_conv3x3_wgrad", "rpn_conv3x3_wgrad_wide"):
        B, H, W, Cin, Cout = shape
        need = getattr(lib, entry + "_workspace_bytes")(B, H, W, Cin, Cout)
        ws, outs["dw"], outs["db"] = scratch(need), out(3, 3, Cin, Cout), out(Cout)
        L.check(getattr(lib, entry)(L.ptr(a), L.ptr(b), B, H, W, Cin, Cout, L.ptr(outs["dw"]), L.ptr(outs["db"]), L.ptr(ws), need, s), entry)
    elif entry == "rpn_conv1x1_wgrad":
        P, Cin, Cout = shape
        need = lib.rpn_conv1x1_wgrad_workspace_bytes(P, Cin, Cout)
        ws, outs["dw"] = scratch(need), out(Cin, Cout)
        L.check(lib.rpn_conv1x1_wgrad(L.ptr(a), L.ptr(b), P, Cin, Cout, L.ptr(outs["dw"]), L.ptr(ws), need, s), entry)
    elif entry.endswith("_dgrad"):
        B, H, W, C = shape
        outs["dx"] = out(B, H, W, C)
        L.check(getattr(lib, entry)(L.ptr(a), L.ptr(b), B, H, W, C, L.ptr(outs["dx"]), s), entry)
    else:
        B, H, W, C = shape
        need = getattr(lib, entry + "_workspace_bytes")(B, H, W, C)
        assert need > 0, (entry, shape)
        ws, outs["dw"] = scratch(need), (out(3, 3, 3, C) if entry == "rpn_conv3x3_s2_cin3_wgrad" else out(3, 3, C))
        L.check(getattr(lib, entry)(L.ptr(a), L.ptr(b), B, H, W, C, L.ptr(outs["dw"]), L.ptr(ws), need, s), entry)
    torch.cuda.synchronize()
    return {name: t.cpu().numpy().tobytes() for name, t in outs.items()}


def digests(lib, entry, shape, seed):
    return {name: hashlib.sha256(raw).hexdigest() for name, raw in run_case(lib, entry, shape, seed).items()}
