"""Cases, seeded inputs and the runner shared by tests/golden/make_forward_bits.py (the recorder) and tests/test_gpu_forward_bits.py:
whole forwards of both inference graphs, each output reduced to the SHA-256 of its float32 bytes.

Every sum of the forward is a fixed tree, so a build gives the same bits on every run, and a change that only moves the
choice of each op's kernel leaves every digest as it is.  The shapes are those at which the choice differs: the small graphs the
suite already runs (pooled and un-pooled convs, the head, every MobileNetV2 block form, the layer-by-layer graph of
keep_activations) and the benchmarked 500 x 500 shapes (the 128- and 64-wide persistent tiles, the Winograd variants, the
high-resolution x3 blocks, the split-K factor of rpn_conv at batch 1 against batch 8)."""
import ctypes
import functools
import hashlib

import numpy as np
import torch

from tf_rpn_amd import _lib as L
from tf_rpn_amd.models._rpn_model import RPNModel, synthetic_weights

BACKBONES = ("vgg16", "mobilenet_v2")
PRECISIONS = ("f32", "bf16x3", "f16x3", "f32w")
K = 9
SEED = 5
MID_LAYER = {"vgg16": "block3_pool", "mobilenet_v2": "block_6_depthwise"}      # read on the keep_activations handles
TAP_LAYER = {"vgg16": "block5_conv3", "mobilenet_v2": "block_13_expand"}

# (backbone, precision, keep_activations, img_size, max_batch, batches forwarded in this order on the one handle)
CASES = ([(b, p, keep, 96, 2, (1, 2)) for b in BACKBONES for p in PRECISIONS for keep in (False, True)]
         + [(b, p, False, 500, 8, (8, 1)) for b in BACKBONES for p in PRECISIONS])


def key_of(case):
    backbone, precision, keep, img_size, max_batch, _batches = case
    return "%s %s %s %d b%d" % (backbone, precision, "keep" if keep else "plan", img_size, max_batch)


def activations_of(case):
    """The activations read back after the case's last forward: the tap layer of the f32 and f16x3 VGG16 handles at 96, and one
    mid-graph layer of every handle that keeps its activations."""
    backbone, precision, keep, img_size, _mb, _batches = case
    names = []
    if backbone == "vgg16" and precision in ("f32", "f16x3") and img_size == 96:
        names.append(TAP_LAYER[backbone])
    if keep:
        names.append(MID_LAYER[backbone])
    return names


def outputs_of(case):
    """The names of the digests a case yields."""
    return ["B%d" % b for b in case[5]] + ["act:" + n for n in activations_of(case)]


@functools.lru_cache(maxsize=None)
def weights_of(backbone):
    return synthetic_weights(backbone, {"img_size": 96, "anchor_count": K}, seed=SEED)      # (the shapes do not depend on img_size)


@functools.lru_cache(maxsize=None)
def images_of(img_size, batch):
    rng = np.random.RandomState(1000 * img_size + batch)
    return rng.uniform(0.0, 1.0, size=(batch, img_size, img_size, 3)).astype(np.float32)


def sha(*tensors):
    h = hashlib.sha256()
    for t in tensors:
        h.update(t.cpu().numpy().astype(np.float32, copy=False).tobytes())
    return h.hexdigest()


def run_case(case):
    """One handle, its forwards in the case's order -> ({output name: sha256}, the RPN_STATUS flags raised by all of them)."""
    backbone, precision, keep, img_size, max_batch, batches = case
    m = RPNModel(backbone, {"img_size": img_size, "anchor_count": K}, precision=precision, max_batch=max_batch,
                 keep_activations=keep)
    m.set_weights(weights_of(backbone))
    out = {}
    for b in batches:
        reg, cls = m.predict_on_batch(torch.from_numpy(images_of(img_size, b)).cuda())
        torch.cuda.synchronize()
        out["B%d" % b] = sha(reg, cls)
    assert batches[-1] == max_batch or not activations_of(case)        # get_activation returns max_batch images: all written
    for name in activations_of(case):
        out["act:" + name] = sha(m.get_activation(name))
    flags = ctypes.c_uint(0)
    L.check(L.lib().rpn_model_status(m._h, ctypes.byref(flags), 0, L.stream_ptr()), "rpn_model_status")
    return out, int(flags.value)
