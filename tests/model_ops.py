"""The handles and the record shared by tests/golden/make_model_ops.py (the recorder) and tests/test_model_ops.py: what
rpn_model_create decides for a handle -- the op list with the kernel each op runs on, the weight blob and arena sizes, the feature
map's side and the layer table -- all of it without touching a device.

Where no device is present the library's three CU-count queries fall back to 256, the MI355X's count, so the record made on a
CPU-only machine is the one an MI355X gives."""
import itertools

from tf_rpn_amd import _lib as L
from tf_rpn_amd.models._rpn_model import RPNModel

BACKBONES = ("vgg16", "mobilenet_v2")
PRECISIONS = ("f32", "bf16x3", "f16x3", "f32w")
MAX_BATCHES = (1, 8, 64)
SIZES = ((500, 9), (1024, 15), (96, 9))            # (img_size, anchor_count)

# (backbone, precision, max_batch, keep_activations, img_size, anchor_count)
HANDLES = [(b, p, mb, keep, size, k) for b, p, mb, keep, (size, k) in
           itertools.product(BACKBONES, PRECISIONS, MAX_BATCHES, (False, True), SIZES)]

CU_COUNT = 256                                     # the count the record holds for


def key_of(handle):
    backbone, precision, max_batch, keep, img_size, k = handle
    return "%s %s b%d %s %d k%d" % (backbone, precision, max_batch, "keep" if keep else "plan", img_size, k)


def record_of(handle):
    """The record of one handle: every op and every layer as one string."""
    backbone, precision, max_batch, keep, img_size, k = handle
    assert precision in L.PRECISIONS
    m = RPNModel(backbone, {"img_size": img_size, "anchor_count": k}, precision=precision, max_batch=max_batch,
                 keep_activations=keep)
    ops = ["%s|%s|%s|%r|%r|%d" % (o["name"], o["kernel"], o["arith"], o["flops_per_image"], o["bytes_per_image"], o["launches"])
           for o in m.ops()]
    layers = ["%s|%s|%s|%d" % (la["name"], la["bn_name"], "x".join(str(v) for v in la["shape"]), la["kind"]) for la in m.layers]
    return {"ops": ops, "memory_bytes": list(m.memory_bytes()), "feature_map_shape": m.feature_map_shape, "layers": layers}
