"""Python handle over the native ``rpn_model`` of librpn_hip.so -- the object that stands where
the reference's Keras ``rpn_model`` stands (models/rpn_vgg16.py:21, predictor.py:41-50).

The inference surface the proposal path touches is mirrored: ``predict_on_batch``, ``__call__`` and ``load_weights``
(Keras ``.h5`` checkpoints through ``utils/h5_weights.py`` -- no h5py needed -- or a flat ``.npz``).
Training mirrors trainer.py:54-69 (``compile`` with Adam, ``train_on_batch`` / ``test_on_batch`` / ``fit``).  By default the RPN
head (``rpn_conv``, ``rpn_reg``, ``rpn_cls``) is trained on a frozen backbone; ``compile(train_backbone_from="block1_conv1")``
trains the whole VGG16 model as the reference does (its Keras base model is trainable), a later conv name the convs from there up.
On MobileNetV2 ``train_backbone_from`` names the first layer of a stride-16 inverted-residual block (``"block_7_expand"`` ..
``"block_12_expand"``) or ``"block_13_expand"``: that layer and everything above it train with the head, BatchNorm in training mode;
the layers below stay frozen.  ``compile(train_backbone=True)`` trains every layer of either backbone, as the reference's trainer.py
does: on MobileNetV2 all 40 convs (``MOBILENET_V2_CONVS``: the stem, ``expanded_conv``, ``block_1`` .. ``block_12``,
``block_13_expand``), each with its BatchNorm, and the head.
"""
import ctypes

import numpy as np
import torch

from .. import _lib as L
from . import _optimizer as O


class FeatureExtractor(object):
    """Stand-in for the Keras layer handle ``get_model`` returns second (models/rpn_vgg16.py:17,22):
    names the tap layer and can fetch its activation after a forward pass."""

    def __init__(self, model, name):
        self._model = model
        self.name = name

    @property
    def output_shape(self):
        return self._model.activation_shape(self.name)

    def output(self):
        return self._model.get_activation(self.name)

    def roi_pool(self, rois, pooling_size=(7, 7), valid=None, out=None):
        """RoI pooling of this layer's output as the model's last forward left it, under ``rois`` (B, R, [y1, x1, y2, x2])
        normalised -> (B, R, ph, pw, C) float32 (``utils/roi_utils.py`` states the operator; ``valid`` (B,) int32: rows beyond it
        are zeros).  Read straight from the handle's arena on the current stream -- under "f16x3" / "bf16x3" in the split form the
        tap is kept in, without a float32 copy -- and bit-identical to ``roi_utils.roi_pooling(self.output()[:B], ...)``."""
        if self.name != self._model.tap_layer:
            raise ValueError("roi_pool reads the model's feature tap %r, not %r" % (self._model.tap_layer, self.name))
        return self._model.roi_pool(rois, pooling_size, valid, out)

    def roi_align(self, rois, pooling_size=(7, 7), sampling_ratio=2, extent=None, valid=None, out=None):
        """RoI Align of this layer's output as the model's last forward left it (``roi_utils.roi_align`` states the operator):
        read straight from the arena like ``roi_pool``, bit-identical to ``roi_utils.roi_align(self.output()[:B], ...)``."""
        if self.name != self._model.tap_layer:
            raise ValueError("roi_align reads the model's feature tap %r, not %r" % (self._model.tap_layer, self.name))
        return self._model.roi_align(rois, pooling_size, sampling_ratio, extent, valid, out)

    def roi_max_pool(self, rois, pooling_size=(7, 7), extent=None, valid=None, out=None):
        """RoI max pooling of this layer's output as the model's last forward left it (``roi_utils.roi_max_pooling`` states the
        operator): read straight from the arena like ``roi_pool``, bit-identical to
        ``roi_utils.roi_max_pooling(self.output()[:B], ...)``.  No argmax is written (inference)."""
        if self.name != self._model.tap_layer:
            raise ValueError("roi_max_pool reads the model's feature tap %r, not %r" % (self._model.tap_layer, self.name))
        return self._model.roi_max_pool(rois, pooling_size, extent, valid, out)


# the layers a training step updates (models/rpn_vgg16.py:18-20, models/rpn_mobilenet_v2.py:18-20)
HEAD_LAYERS = ("rpn_conv", "rpn_cls", "rpn_reg")
# the VGG16 convs in graph order (keras.applications.VGG16 up to block5_conv3): what train_backbone_from names
VGG16_CONVS = ("block1_conv1", "block1_conv2", "block2_conv1", "block2_conv2", "block3_conv1", "block3_conv2", "block3_conv3",
               "block4_conv1", "block4_conv2", "block4_conv3", "block5_conv1", "block5_conv2", "block5_conv3")
# MobileNetV2's convs at the feature map's own resolution (stride 16), in graph order: the span train_backbone_from can open.
# Conv X is followed by the BatchNormalization layer "X_BN"; none has a bias.
MOBILENET_V2_SPAN = tuple("block_%d_%s" % (b, part) for b in range(7, 13) for part in ("expand", "depthwise", "project")) + ("block_13_expand",)
# ... and the names it accepts: the first layer of a block, or block_13_expand alone
MOBILENET_V2_TRAIN_FROM = tuple("block_%d_expand" % b for b in range(7, 14))
# every conv of MobileNetV2 up to the feature map, in graph order: what compile(train_backbone=True) trains.  expanded_conv has no
# expand conv; Conv1's BatchNorm layer is "bn_Conv1" (its Keras name), every other conv X's is "X_BN".
MOBILENET_V2_CONVS = (("Conv1", "expanded_conv_depthwise", "expanded_conv_project")
                      + tuple("block_%d_%s" % (b, part) for b in range(1, 13) for part in ("expand", "depthwise", "project"))
                      + ("block_13_expand",))
BN_KEYS = ("gamma", "beta", "mean", "var")


class RPNModel(O.OptimizerMixin):
    _t = None
    _h = None

    def __init__(self, backbone, hyper_params, precision="f32", max_batch=8, keep_activations=False):
        if backbone not in L.BACKBONES:
            raise ValueError("unknown backbone %r" % (backbone,))
        if precision not in L.PRECISIONS:
            raise ValueError("unknown precision %r (choose from %s)" % (precision, sorted(L.PRECISIONS)))
        self.backbone = backbone
        self.precision = precision
        self.img_size = int(hyper_params["img_size"])
        self.anchor_count = int(hyper_params["anchor_count"])
        self.max_batch = int(max_batch)
        self._h = L.vp(0)
        lib = L.lib()
        st = lib.rpn_model_create(L.BACKBONES[backbone], self.img_size, self.anchor_count,
                                  L.PRECISIONS[precision], self.max_batch, ctypes.byref(self._h))
        L.check(st, "rpn_model_create")
        if keep_activations:
            L.check(lib.rpn_model_keep_activations(self._h, 1), "rpn_model_keep_activations")
        self.feature_map_shape = int(lib.rpn_model_feature_map_shape(self._h))
        self.flops_per_image = float(lib.rpn_model_flops_per_image(self._h))
        self.layers = self._enumerate_layers()
        self.tap_layer = "block5_conv3" if backbone == "vgg16" else "block_13_expand"
        self._head = {}                 # head weights last given to set_weights / load_weights: {name: (kernel, bias)}
        self._backbone = {}             # the same for the VGG16 convs (the handle keeps only packed / transformed copies)
        self._mn = {}                   # MobileNetV2's convs, UNFOLDED (the handle folds BatchNorm at load):
                                        # {conv: {"kernel", "gamma", "beta", "mean", "var"}}
        self._bn_of = {layer["name"]: layer["bn_name"] for layer in self.layers}
        self._t = L.vp(0)               # native trainer (compile)
        self._opt = None
        self._train_from = None         # first trained backbone layer, None: the head only
        self._head_dirty = False        # the trainer's head differs from the handle's: copied before the next inference
        self._pending = None            # (image batch, B) of a forward_for_training that apply_gradients has not consumed

    # ---- introspection ----------------------------------------------------------------
    def _enumerate_layers(self):
        lib = L.lib()
        out = []
        buf = ctypes.create_string_buffer(128)
        shape = (ctypes.c_int * 4)()
        kind = ctypes.c_int(0)
        for i in range(lib.rpn_model_num_layers(self._h)):
            L.check(lib.rpn_model_layer_info(self._h, i, buf, 128, shape, ctypes.byref(kind)), "rpn_model_layer_info")
            name = buf.value.decode()
            L.check(lib.rpn_model_layer_bn_name(self._h, i, buf, 128), "rpn_model_layer_bn_name")
            out.append({"name": name, "bn_name": buf.value.decode(), "shape": tuple(shape), "kind": int(kind.value)})
        return out

    def memory_bytes(self):
        w, a = ctypes.c_size_t(0), ctypes.c_size_t(0)
        L.check(L.lib().rpn_model_memory_bytes(self._h, ctypes.byref(w), ctypes.byref(a)), "rpn_model_memory_bytes")
        return int(w.value), int(a.value)

    # ---- weights ------------------------------------------------------------------------
    def set_weights(self, weights, partial=False):
        """weights: {layer_name: {"kernel": HWIO, "bias": (Cout,)}} and, for layers followed by
        BatchNorm, {bn_name: {"gamma", "beta", "mean", "var"}} -- Keras layer names.  ``partial``: layers absent
        from ``weights`` are left as they are (Keras ``by_name`` loading); forward still refuses to run until every
        layer has been set once.  Returns the names of the layers set."""
        lib = L.lib()
        fp = lambda a: (np.ascontiguousarray(a, dtype=np.float32))
        done = []
        for layer in self.layers:
            name, bn = layer["name"], layer["bn_name"]
            if name not in weights:
                if partial:
                    continue
                raise KeyError("weights for layer %r are missing" % name)
            kernel = fp(weights[name]["kernel"])
            if tuple(kernel.shape) != layer["shape"]:
                raise ValueError("layer %r: kernel shape %s, expected %s" % (name, kernel.shape, layer["shape"]))
            bias = weights[name].get("bias")
            bias = fp(bias) if bias is not None else None
            args = [kernel.ctypes.data_as(L.c_float_p), bias.ctypes.data_as(L.c_float_p) if bias is not None else None]
            keep = [kernel, bias]
            if bn:
                if bn not in weights:
                    raise KeyError("BatchNorm parameters %r (after %r) are missing" % (bn, name))
                for key in ("gamma", "beta", "mean", "var"):
                    arr = fp(weights[bn][key])
                    keep.append(arr)
                    args.append(arr.ctypes.data_as(L.c_float_p))
            else:
                args += [None, None, None, None]
            L.check(lib.rpn_model_set_layer(self._h, name.encode(), *args), "rpn_model_set_layer(%s)" % name)
            if self._is_mn(name):
                self._mn[name] = dict({"kernel": kernel.copy()}, **{k: a.copy() for k, a in zip(BN_KEYS, keep[2:])})
                if self._t and name in self.trained_layers():
                    self._trainer_set(name)
            elif name in HEAD_LAYERS or (self.backbone == "vgg16" and name in VGG16_CONVS):
                (self._head if name in HEAD_LAYERS else self._backbone)[name] = (kernel.copy(), bias.copy())
                if self._t and (name in HEAD_LAYERS or self._train_from is not None):
                    self._trainer_set(name)
            done.append(name)
        return done

    def load_weights(self, path, by_name=True):
        """``model.load_weights(path, by_name=True)`` of the reference (predictor.py:43-44).

        ``path``: a Keras ``.h5`` / ``.hdf5`` weights file (what the reference's trainer checkpoints, or the
        ``model_weights`` of a full-model file; read by ``utils/h5_weights.py``, no h5py needed), or a flat ``.npz``
        written by ``save_weights`` (keys ``<layer>/<param>``).  Layers are matched by their Keras names; BatchNorm is
        folded into the preceding conv at load time.  ``by_name=True``: layers of this model that the file does not
        contain are left untouched, layers of the file that this model lacks are ignored.  Returns the layers set."""
        with open(path, "rb") as f:
            is_h5 = f.read(8) == b"\x89HDF\r\n\x1a\n"
        if is_h5:
            from ..utils import h5_weights
            weights = h5_weights.to_layer_arrays(h5_weights.read_keras_weights(path)[0])
        else:
            data = np.load(path)
            weights = {}
            for key in data.files:
                layer, param = key.rsplit("/", 1)
                weights.setdefault(layer, {})[param] = data[key]
        return self.set_weights(weights, partial=bool(by_name))

    @staticmethod
    def save_weights(weights, path):
        np.savez(path, **{"%s/%s" % (layer, p): v for layer, d in weights.items() for p, v in d.items()})

    # ---- forward ------------------------------------------------------------------------
    def predict_on_batch(self, imgs):
        """imgs (B, img_size, img_size, 3) float32 in [0,1] -> [rpn_reg (B,F,F,4K), rpn_cls (B,F,F,K)]
        (the reference's output order, models/rpn_vgg16.py:21)."""
        x, was_np = L.to_device(imgs)
        if x.dim() != 4 or tuple(x.shape[1:]) != (self.img_size, self.img_size, 3):
            raise ValueError("imgs must be (B,%d,%d,3) NHWC, got %s" % (self.img_size, self.img_size, tuple(x.shape)))
        B = int(x.shape[0])
        F, K = self.feature_map_shape, self.anchor_count
        reg = torch.empty((B, F, F, 4 * K), dtype=torch.float32, device="cuda")
        cls = torch.empty((B, F, F, K), dtype=torch.float32, device="cuda")
        self.forward_into(x, reg, cls)
        if was_np and self.precision in ("f16x3", "fp16x3"):
            # numpy in / numpy out synchronises anyway: never hand back silently wrong outputs.  CUDA-tensor callers
            # (the hot path) poll ``status()`` themselves, a forward never reads the flag back.
            self.raise_on_range_error()
        return [L.from_device(reg, was_np), L.from_device(cls, was_np)]

    __call__ = predict_on_batch

    def forward_into(self, x, reg, cls):
        """Forward on preallocated CUDA tensors (no allocation: graph-capturable once the head is in sync).  The C side sees
        raw pointers, so dtype / device / layout / shape are checked here."""
        self._sync_head()
        B = int(x.shape[0]) if isinstance(x, torch.Tensor) and x.dim() == 4 else -1
        F, K = self.feature_map_shape, self.anchor_count
        for t, shape, what in ((x, (B, self.img_size, self.img_size, 3), "imgs"), (reg, (B, F, F, 4 * K), "reg"),
                               (cls, (B, F, F, K), "cls")):
            if not (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.float32 and t.is_contiguous()
                    and tuple(t.shape) == shape):
                raise ValueError("%s must be a contiguous CUDA float32 tensor of shape %s, got %s"
                                 % (what, shape, (tuple(t.shape), t.dtype, t.device) if isinstance(t, torch.Tensor) else type(t)))
        if not 1 <= B <= self.max_batch:
            raise ValueError("batch %d outside [1, %d]" % (B, self.max_batch))
        st = L.lib().rpn_model_forward(self._h, L.ptr(x), int(x.shape[0]), L.ptr(reg), L.ptr(cls), L.stream_ptr())
        L.check(st, "rpn_model_forward")

    # ---- float16 range status (precision "f16x3") ---------------------------------------------------
    def status(self, reset=False):
        """Sticky flags raised on the device by the forwards so far -> {"f16_range": bool}.  ``f16_range``: some
        activation did not fit float16 when it was written in split form (|x| > 65504 or non-finite), the outputs of
        that forward are invalid.  Synchronises the current stream (not part of the hot path)."""
        flags = ctypes.c_uint(0)
        L.check(L.lib().rpn_model_status(self._h, ctypes.byref(flags), 1 if reset else 0, L.stream_ptr()),
                "rpn_model_status")
        return {"f16_range": bool(flags.value & L.STATUS_F16_RANGE)}

    def raise_on_range_error(self):
        if self.status(reset=True)["f16_range"]:
            raise FloatingPointError("precision 'f16x3': an activation left the float16 range (|x| > 65504); the outputs "
                                     "are invalid -- use precision='bf16x3' (float32 range, same speed) or 'f32' for "
                                     "these weights")

    # ---- per-op timing (HIP events on the launch stream) ---------------------------------------
    def set_profiling(self, n_forwards=1):
        """Keep HIP-event timings of the last ``n_forwards`` forwards (0 switches profiling off)."""
        L.check(L.lib().rpn_model_set_profiling(self._h, int(n_forwards)), "rpn_model_set_profiling")

    def set_profiling_mask(self, mask=None):
        """Time only the ops with a true entry in ``mask`` (one per op; None: every op)."""
        if mask is None:
            L.check(L.lib().rpn_model_set_profiling_mask(self._h, None, 0), "rpn_model_set_profiling_mask")
            return
        buf = (ctypes.c_ubyte * len(mask))(*[1 if v else 0 for v in mask])
        L.check(L.lib().rpn_model_set_profiling_mask(self._h, buf, len(mask)), "rpn_model_set_profiling_mask")

    def set_profiling_rotate(self, on=True):
        """With a mask: time one marked op per forward, round robin (2 events per forward)."""
        L.check(L.lib().rpn_model_set_profiling_rotate(self._h, 1 if on else 0), "rpn_model_set_profiling_rotate")

    def ops(self):
        """[{name, kernel, flops_per_image, bytes_per_image, arith, launches}] in graph order.  `arith` is the arithmetic the
        op's matrix work runs in ("f32" | "bf16x3" | "f16x3"); `launches` is 0 for a max-pool that runs inside the previous
        conv's epilogue (kernel "fused:maxpool_split": no launch, no bytes of its own), else 1.  ``kernel`` is what a forward of
        ``max_batch`` images runs: a ``conv3x3_split16`` layer picks its form from the grid of each call, so a smaller batch may
        run another one (same bits) -- ``conv_launch_info(name, batch)`` reports the form at any batch size."""
        lib = L.lib()
        out = []
        nb, kb = ctypes.create_string_buffer(128), ctypes.create_string_buffer(128)
        fl, by = ctypes.c_double(0), ctypes.c_double(0)
        for i in range(lib.rpn_model_num_ops(self._h)):
            L.check(lib.rpn_model_op_info(self._h, i, nb, 128, kb, 128, ctypes.byref(fl), ctypes.byref(by)),
                    "rpn_model_op_info")
            kernel = kb.value.decode()
            out.append({"name": nb.value.decode(), "kernel": kernel, "flops_per_image": fl.value,
                        "bytes_per_image": by.value,
                        "arith": {0: "f32", 1: "bf16x3", 2: "f16x3", 3: "f32w"}[lib.rpn_model_op_arith(self._h, i)],
                        "launches": 0 if kernel.startswith("fused:") else 1})
        return out

    def head_launch_info(self, batch):
        """Which form of the head a forward of ``batch`` images runs (test hook; host arithmetic, nothing is launched) ->
        {"route": "splitk" | "f32", "NB", "pixels_per_workgroup": 32 | 16 | 4, "slabs": 1 | 2 | 4} (zeros / 1 on "f32")."""
        info = (ctypes.c_int * 4)()
        L.check(L.lib().rpn_model_head_launch_info(self._h, int(batch), info), "rpn_model_head_launch_info")
        return {"route": "splitk" if info[0] == 0 else "f32", "NB": int(info[1]), "pixels_per_workgroup": int(info[2]),
                "slabs": int(info[3])}

    IR_ROUTES = ("ir_block", "ir_block_hr", "ir_block_x3", "ir_block_hrx3", "stem")      # rpn_hip.h: RPN_IR_ROUTE_*

    def ir_launch_info(self, name, batch):
        """Which form of the fused MobileNetV2 block writing tensor ``name`` ("block_<k>_project", "expanded_conv_project") a forward
        of ``batch`` images runs (test hook; host arithmetic shared with the launchers, nothing is launched) ->
        {"route": one of ``IR_ROUTES``, "chunk": expanded channels per step, "ksplit": workgroups per tile, "tiles"}."""
        info = (ctypes.c_int * 4)()
        L.check(L.lib().rpn_model_ir_launch_info(self._h, name.encode(), int(batch), info), "rpn_model_ir_launch_info")
        return {"route": self.IR_ROUTES[info[0]], "chunk": int(info[1]), "ksplit": int(info[2]), "tiles": int(info[3])}

    CONV_ROUTES = ("vgg_block1", "first_layer", "split", "split16_reg", "split16_dma", "maxpool_split")   # rpn_hip.h: RPN_CONV_ROUTE_*

    def conv_launch_info(self, name, batch):
        """Which form of the split-precision op writing tensor ``name`` ("block2_conv1", "block2_pool", "rpn_conv", ...) a forward of
        ``batch`` images runs (test hook; host arithmetic shared with the launchers, nothing is launched) ->
        {"route": one of ``CONV_ROUTES``, "width": channels per tile, "pool": the 2 x 2 max-pool runs in the epilogue,
        "kform": 0 one chain | 1 K tree in one workgroup | 2 | 4 K tree over that many workgroups}."""
        info = (ctypes.c_int * 4)()
        L.check(L.lib().rpn_model_conv_launch_info(self._h, name.encode(), int(batch), info), "rpn_model_conv_launch_info")
        return {"route": self.CONV_ROUTES[info[0]], "width": int(info[1]), "pool": bool(info[2]), "kform": int(info[3])}

    def forward_to(self, name, imgs):
        """The handle's own graph up to the op that writes tensor ``name``, at the handle's precision (test hook: no kept
        activations needed) -> that tensor for the ``B`` images given, a fresh float32 CUDA tensor (B, H, W, C)."""
        self._sync_head()
        x, _ = L.to_device(imgs)
        if x.dim() != 4 or tuple(x.shape[1:]) != (self.img_size, self.img_size, 3):
            raise ValueError("imgs must be (B,%d,%d,3) NHWC, got %s" % (self.img_size, self.img_size, tuple(x.shape)))
        B = int(x.shape[0])
        if not 1 <= B <= self.max_batch:
            raise ValueError("batch %d outside [1, %d]" % (B, self.max_batch))
        shape = self.activation_shape(name)
        out = torch.empty((B,) + tuple(shape[1:]), dtype=torch.float32, device="cuda")
        L.check(L.lib().rpn_model_forward_to(self._h, name.encode(), L.ptr(x), B, L.ptr(out), L.stream_ptr()), "rpn_model_forward_to")
        return out

    def profile_ms(self):
        """Mean milliseconds per op over the kept forwards -> (list, n_forwards)."""
        n = L.lib().rpn_model_num_ops(self._h)
        buf = (ctypes.c_float * n)()
        kept = ctypes.c_int(0)
        L.check(L.lib().rpn_model_get_profile(self._h, buf, n, ctypes.byref(kept)), "rpn_model_get_profile")
        return [float(v) for v in buf], int(kept.value)

    def activation_shape(self, name):
        shape = (ctypes.c_int * 4)()
        L.check(L.lib().rpn_model_get_activation(self._h, name.encode(), None, 0, shape, None),
                "rpn_model_get_activation")
        return tuple(shape)

    def get_activation(self, name, batch=None):
        shape = self.activation_shape(name)
        out = torch.empty(shape, dtype=torch.float32, device="cuda")
        L.check(L.lib().rpn_model_get_activation(self._h, name.encode(), L.ptr(out), out.numel() * 4, None,
                                                 L.stream_ptr()), "rpn_model_get_activation")
        return out if batch is None else out[:batch]

    def roi_pool(self, rois, pooling_size=(7, 7), valid=None, out=None):
        """``FeatureExtractor.roi_pool``: rpn_model_roi_pool of the tap layer after a forward.  ``out``: a preallocated contiguous
        CUDA float32 (B, R, ph, pw, C) tensor to fill (no allocation, as ``forward_into``)."""
        rois, valid, out, (B, R, ph, pw) = self._roi_args(rois, pooling_size, valid, out)
        L.check(L.lib().rpn_model_roi_pool(self._h, L.ptr(rois), B, R, ph, pw, L.ptr(valid), L.ptr(out), L.stream_ptr()),
                "rpn_model_roi_pool")
        return out

    def roi_align(self, rois, pooling_size=(7, 7), sampling_ratio=2, extent=None, valid=None, out=None):
        """``FeatureExtractor.roi_align``: rpn_model_roi_align of the tap layer after a forward; ``extent`` defaults to the tap's
        (H, W).  ``out`` as in ``roi_pool``."""
        from ..utils import roi_utils
        s = roi_utils._sampling_ratio(sampling_ratio)
        sy, sx = roi_utils._extent(extent, *self.activation_shape(self.tap_layer)[1:3])
        rois, valid, out, (B, R, ph, pw) = self._roi_args(rois, pooling_size, valid, out)
        L.check(L.lib().rpn_model_roi_align(self._h, L.ptr(rois), B, R, ph, pw, s, sy, sx, L.ptr(valid), L.ptr(out), L.stream_ptr()),
                "rpn_model_roi_align")
        return out

    def roi_max_pool(self, rois, pooling_size=(7, 7), extent=None, valid=None, out=None):
        """``FeatureExtractor.roi_max_pool``: rpn_model_roi_max_pool of the tap layer after a forward, without an argmax; ``extent``
        defaults to the tap's (H - 1, W - 1).  ``out`` as in ``roi_pool``."""
        from ..utils import roi_utils
        sy, sx = roi_utils._max_extent(extent, *self.activation_shape(self.tap_layer)[1:3])
        rois, valid, out, (B, R, ph, pw) = self._roi_args(rois, pooling_size, valid, out)
        L.check(L.lib().rpn_model_roi_max_pool(self._h, L.ptr(rois), B, R, ph, pw, sy, sx, L.ptr(valid), L.ptr(out), None,
                                               L.stream_ptr()), "rpn_model_roi_max_pool")
        return out

    def _roi_args(self, rois, pooling_size, valid, out):
        """the argument checks ``roi_pool``, ``roi_align`` and ``roi_max_pool`` share -> (rois, valid, out (allocated when None), (B, R, ph, pw))"""
        ph, pw = (int(v) for v in pooling_size)
        C = self.activation_shape(self.tap_layer)[3]
        for t, dtype, what in ((rois, torch.float32, "rois"), (valid, torch.int32, "valid")):
            if t is not None and not (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == dtype and t.is_contiguous()):
                raise ValueError("%s must be a contiguous CUDA %s tensor" % (what, dtype))
        if rois.dim() != 3 or int(rois.shape[2]) != 4 or not 1 <= int(rois.shape[0]) <= self.max_batch:
            raise ValueError("rois must be (B<=%d, R, 4), got %s" % (self.max_batch, tuple(rois.shape)))
        B, R = int(rois.shape[0]), int(rois.shape[1])
        if valid is not None and tuple(valid.shape) != (B,):
            raise ValueError("valid must be (%d,), got %s" % (B, tuple(valid.shape)))
        shape = (B, R, ph, pw, C)
        if out is None:
            out = torch.empty(shape, dtype=torch.float32, device="cuda")
        elif not (isinstance(out, torch.Tensor) and out.is_cuda and out.dtype == torch.float32 and out.is_contiguous()
                  and tuple(out.shape) == shape):
            raise ValueError("out must be a contiguous CUDA float32 tensor of shape %s" % (shape,))
        return rois, valid, out, (B, R, ph, pw)

    # ---- training of the head (trainer.py:54-69) ----------------------------------------------------------------------------
    def compile(self, learning_rate=1e-5, beta_1=0.9, beta_2=0.999, epsilon=1e-7, trainable=HEAD_LAYERS, train_backbone_from=None,
                train_backbone=False, backward_precision="f32", optimizer="adam", momentum=0.0, nesterov=False, weight_decay=0.0,
                global_clipnorm=None):
        """``rpn_model.compile(optimizer=tf.optimizers.Adam(learning_rate), loss=[reg_loss, cls_loss])`` (trainer.py:54-56).

        ``train_backbone_from=None`` (default) trains the RPN head (``rpn_conv``, ``rpn_cls``, ``rpn_reg``) on a frozen backbone,
        the backbone running at the handle's precision.  A VGG16 conv name trains that conv and every conv above it (up to
        ``block5_conv3``) with the head; ``"block1_conv1"`` trains the whole model, as the reference does (its Keras base model is
        trainable).  Such a step runs the whole VGG16 forward in exact float32 from the trainer's own weights.

        On MobileNetV2 the name is one of ``MOBILENET_V2_TRAIN_FROM``: ``"block_7_expand"`` .. ``"block_12_expand"`` (the first
        layer of an inverted-residual block) or ``"block_13_expand"``; it and every layer above it -- the stride-1 blocks at the
        feature map's own resolution -- train with the head: per conv the kernel and its BatchNorm's gamma and beta.  The layers
        below stay frozen and run as in inference (BatchNorm folded, the handle's ops and precision).  In ``train_on_batch`` the
        trained layers run in exact float32 with BatchNorm in TRAINING mode -- batch mean and biased batch variance over (B, F, F),
        eps 1e-3, and the moving statistics updated in the same step with momentum 0.999 and Bessel's correction (TF 2.0's fused
        BatchNorm as recalled); ``test_on_batch`` normalises with the moving statistics and updates nothing (Keras ``evaluate``).
        With any other name the backbone trains its head only.

        ``train_backbone=True`` trains every layer of the model, as the reference's trainer.py does (it cannot be combined with
        ``train_backbone_from``).  On VGG16 it is ``train_backbone_from="block1_conv1"``.  On MobileNetV2 it trains all 40 convs of
        ``MOBILENET_V2_CONVS`` -- the stem ``Conv1``, ``expanded_conv``, the stride-2 blocks included -- each with its BatchNorm, and
        the head: there is no frozen prefix, every layer runs in exact float32 at its own resolution from the image batch up, with
        BatchNorm as described above.  The kept activations take about 2 GB at batch 8, 500 x 500 (README, "Training the head").

        ``trainable`` names the head layers only and must be exactly the three of them.

        ``backward_precision``: ``"f32"`` (default) or ``"f16x3"``.  ``"f16x3"`` runs the 3x3 products of a trained VGG16 span's
        backward -- every input gradient and every weight gradient but ``block1_conv1``'s -- in split float16 on the 16-bit MFMA
        (include/rpn_hip.h, "Training the backbone's backward in split float16"); the forward, the losses and the head's backward
        stay exact float32.  It needs a VGG16 backbone span (``train_backbone_from`` / ``train_backbone``).

        Adam is TF 2.0's ApplyAdam (as recalled from its sources): alpha = lr sqrt(1 - beta_2^t) / (1 - beta_1^t),
        m += (g - m)(1 - beta_1), v += (g^2 - v)(1 - beta_2), w -= alpha m / (sqrt(v) + epsilon), m = v = 0 at compile, t = the
        number of applied steps.  The trainer starts from the weights last given to ``set_weights`` / ``load_weights`` (or from
        the trained ones when compiled again).

        ``optimizer``: ``"adam"`` (default) or ``"sgd"`` with ``momentum`` in [0, 1) and ``nesterov``; ``weight_decay``: L2 decay of
        every trained kernel (never a bias, gamma or beta), added to the gradient after the clip; ``global_clipnorm``: clip the whole
        gradient by its global norm (None / 0: off; NOT Keras' per-tensor ``clipnorm``).  The defaults launch exactly the Adam step
        this method always compiled.  ``learning_rate``: a float or a callable ``f(applied_steps) -> float`` evaluated with
        ``train_steps()`` before every update; ``model.learning_rate`` reads and sets it.  Every ``compile`` builds a new trainer
        with zero optimizer state: ``set_optimizer_state`` / ``load_optimizer_state`` come AFTER it.  README, "Optimizers"."""
        if isinstance(trainable, str) or set(trainable) != set(HEAD_LAYERS):
            raise ValueError("trainable=%r: trainable names the RPN head, which trains on a frozen backbone -- it must be exactly %s; "
                             "to train backbone convs too use train_backbone_from=<first trained conv>" % (trainable, HEAD_LAYERS))
        if train_backbone and train_backbone_from is not None:
            raise ValueError("train_backbone=True trains every layer: it cannot be combined with train_backbone_from=%r"
                             % (train_backbone_from,))
        if train_backbone and self.backbone == "vgg16":
            train_backbone_from = VGG16_CONVS[0]
        if train_backbone_from is not None:
            if self.backbone != "vgg16":
                if train_backbone_from not in MOBILENET_V2_TRAIN_FROM:
                    raise ValueError("train_backbone_from=%r: on %s the accepted names are %s (that layer and every layer above it "
                                     "train with the head); otherwise the backbone trains its head only -- the named layer is a VGG16 "
                                     "conv, is not the first layer of a block, or lies below block_7_expand (train_backbone=True "
                                     "trains the whole model)"
                                     % (train_backbone_from, self.backbone, MOBILENET_V2_TRAIN_FROM))
            elif train_backbone_from not in VGG16_CONVS:
                raise ValueError("train_backbone_from=%r is not a VGG16 conv (one of %s)" % (train_backbone_from, VGG16_CONVS))
        if backward_precision in ("bf16x3", "f32w"):
            raise ValueError("backward_precision=%r: the backward has no %s kernels -- it runs in 'f32' or 'f16x3'"
                             % (backward_precision, backward_precision))
        if backward_precision not in ("f32", "f16x3"):
            raise ValueError("backward_precision=%r is not a backward precision: 'f32' or 'f16x3'" % (backward_precision,))
        if backward_precision == "f16x3" and (self.backbone != "vgg16" or train_backbone_from is None):
            raise ValueError("backward_precision='f16x3' runs the VGG16 backbone's backward products in split float16: "
                             + ("the %s backward has no such kernels" % self.backbone if self.backbone != "vgg16" else
                                "this compile trains the head only, so there is no backbone backward (give train_backbone_from or "
                                "train_backbone=True)"))
        cfg = O.check_config(optimizer, momentum, nesterov, weight_decay, global_clipnorm)
        lr = O.check_learning_rate(learning_rate)
        self._lr = lr
        self._opt = (0.0 if callable(lr) else lr, float(beta_1), float(beta_2), float(epsilon))
        if self._t:
            self._sync_head()       # layers the new trainer freezes run on the handle: they keep what the old one trained
            got = self.get_weights()
            for k, d in got.items():
                if self._is_mn(k):
                    self._mn[k] = dict({"kernel": d["kernel"]}, **got[self._bn_of[k]])
                elif "kernel" in d:
                    (self._head if k in HEAD_LAYERS else self._backbone)[k] = (d["kernel"], d["bias"])
            L.lib().rpn_head_trainer_destroy(self._t)
            self._t = L.vp(0)
        t = L.vp(0)
        if train_backbone and train_backbone_from is None:      # MobileNetV2 from the stem up
            L.check(L.lib().rpn_model_trainer_create_full(self._h, ctypes.byref(t)), "rpn_model_trainer_create_full")
            train_backbone_from = MOBILENET_V2_CONVS[0]
        elif train_backbone_from is None:
            L.check(L.lib().rpn_head_trainer_create(self._h, ctypes.byref(t)), "rpn_head_trainer_create")
        else:
            L.check(L.lib().rpn_model_trainer_create(self._h, train_backbone_from.encode(), ctypes.byref(t)),
                    "rpn_model_trainer_create")
        self._t = t
        self._pending = None
        self._train_from = train_backbone_from
        self._opt_cfg = cfg
        if cfg != O.OptimizerMixin._opt_cfg:
            self._apply_optimizer_config()
        L.check(L.lib().rpn_head_trainer_set_backward_precision(t, L.PRECISIONS[backward_precision]),
                "rpn_head_trainer_set_backward_precision")
        for name in self._head:
            self._trainer_set(name)
        if train_backbone_from is not None:
            for name in self._backbone:
                self._trainer_set(name)
            for name in self._mn:
                if name in self.trained_layers():
                    self._trainer_set(name)

    @property
    def backward_precision(self):
        """``"f32"`` or ``"f16x3"``: the arithmetic of the backbone's backward products (``compile(backward_precision=...)``)."""
        if not self._t:
            return "f32"
        return {0: "f32", 2: "f16x3"}[L.lib().rpn_head_trainer_backward_precision(self._t)]

    def train_status(self, reset=False):
        """``{"f16_range": bool}``: whether a value of the split-float16 backward left float16's range (an activation with
        |x| > 65504, a non-finite activation or gradient) since the last reset; synchronises the current stream."""
        if not self._t:
            raise RuntimeError("call compile() first")
        flags = ctypes.c_uint(0)
        L.check(L.lib().rpn_head_trainer_status(self._t, ctypes.byref(flags), 1 if reset else 0,
                                                L.stream_ptr() if torch.cuda.is_available() else None), "rpn_head_trainer_status")
        return {"f16_range": bool(flags.value & L.STATUS_F16_RANGE)}

    def trained_layers(self):
        """The layers a training step updates: the head, plus the backbone convs from ``train_backbone_from`` up, or all of them
        after ``compile(train_backbone=True)``, in graph order (each MobileNetV2 conv with its BatchNorm)."""
        if self._train_from is None:
            return HEAD_LAYERS
        order = VGG16_CONVS if self.backbone == "vgg16" else MOBILENET_V2_CONVS
        return tuple(order[order.index(self._train_from):]) + HEAD_LAYERS

    def _is_mn(self, name):
        return self.backbone == "mobilenet_v2" and name in MOBILENET_V2_CONVS

    def _trainer_set(self, name):
        if self._is_mn(name):
            d = self._mn[name]
            L.check(L.lib().rpn_head_trainer_set_layer(self._t, name.encode(), d["kernel"].ctypes.data_as(L.c_float_p), None),
                    "rpn_head_trainer_set_layer(%s)" % name)
            L.check(L.lib().rpn_head_trainer_set_bn(self._t, name.encode(), *[d[k].ctypes.data_as(L.c_float_p) for k in BN_KEYS]),
                    "rpn_head_trainer_set_bn(%s)" % name)
            return
        kernel, bias = self._head[name] if name in HEAD_LAYERS else self._backbone[name]
        L.check(L.lib().rpn_head_trainer_set_layer(self._t, name.encode(), kernel.ctypes.data_as(L.c_float_p),
                                                   bias.ctypes.data_as(L.c_float_p)), "rpn_head_trainer_set_layer(%s)" % name)

    # what OptimizerMixin asks for
    def _opt_target(self):
        return (self._t if self._t else None), "rpn_head_trainer"

    def _opt_entries(self):
        out = []
        trained = self.trained_layers()
        for layer in self.layers:
            name = layer["name"]
            if name not in trained:
                continue
            if self._is_mn(name):
                C = layer["shape"][2] if layer["kind"] == 2 else layer["shape"][3]
                out.append((name, name, False, {"kernel": tuple(layer["shape"])}))
                out.append((layer["bn_name"], name, True, {"gamma": (C,), "beta": (C,)}))
            else:
                out.append((name, name, False, {"kernel": tuple(layer["shape"]), "bias": (layer["shape"][3],)}))
        return out

    def _opt_touch(self):
        self._pending = None

    def get_gradients(self):
        """{layer: {"kernel", "bias"}}: the gradient of the total loss at the last ``train_on_batch`` (test hook).  A trained
        MobileNetV2 conv gives {conv: {"kernel"}} and {conv_BN: {"gamma", "beta"}}."""
        if not self._t:
            raise RuntimeError("call compile() first")
        out = {}
        trained = self.trained_layers()
        fpp = lambda a: a.ctypes.data_as(L.c_float_p)
        for layer in self.layers:
            if layer["name"] in trained and self._is_mn(layer["name"]):
                name, C = layer["name"], layer["shape"][2] if layer["kind"] == 2 else layer["shape"][3]
                kernel = np.empty(layer["shape"], dtype=np.float32)
                dg, db = np.empty((C,), np.float32), np.empty((C,), np.float32)
                L.check(L.lib().rpn_head_trainer_get_gradient(self._t, name.encode(), fpp(kernel), None, L.stream_ptr()),
                        "rpn_head_trainer_get_gradient")
                L.check(L.lib().rpn_head_trainer_get_bn_gradient(self._t, name.encode(), fpp(dg), fpp(db), L.stream_ptr()),
                        "rpn_head_trainer_get_bn_gradient")
                out[name] = {"kernel": kernel}
                out[layer["bn_name"]] = {"gamma": dg, "beta": db}
            elif layer["name"] in trained:
                kernel = np.empty(layer["shape"], dtype=np.float32)
                bias = np.empty((layer["shape"][3],), dtype=np.float32)
                L.check(L.lib().rpn_head_trainer_get_gradient(self._t, layer["name"].encode(), kernel.ctypes.data_as(L.c_float_p),
                                                              bias.ctypes.data_as(L.c_float_p), L.stream_ptr()),
                        "rpn_head_trainer_get_gradient")
                out[layer["name"]] = {"kernel": kernel, "bias": bias}
        return out

    def get_weights(self):
        """{layer: {"kernel": HWIO, "bias"}} of the trained layers -- the three head layers, plus the VGG16 convs from
        ``train_backbone_from`` up when compiled so (the trained values once a step has run): what ``save_weights`` writes and
        ``set_weights`` / ``load_weights`` read back.  A trained MobileNetV2 conv gives {conv: {"kernel"}} and {conv_BN: {"gamma",
        "beta", "mean", "var"}} (unfolded; mean / var are the moving statistics)."""
        out = {}
        trained = self.trained_layers()
        stream = L.stream_ptr() if torch.cuda.is_available() else None
        fpp = lambda a: a.ctypes.data_as(L.c_float_p)
        for layer in self.layers:
            name = layer["name"]
            if name not in trained:
                continue
            if self._is_mn(name):
                if self._t:
                    C = layer["shape"][2] if layer["kind"] == 2 else layer["shape"][3]
                    kernel = np.empty(layer["shape"], dtype=np.float32)
                    bn = {k: np.empty((C,), np.float32) for k in BN_KEYS}
                    L.check(L.lib().rpn_head_trainer_get_layer(self._t, name.encode(), fpp(kernel), None, stream),
                            "rpn_head_trainer_get_layer(%s)" % name)
                    L.check(L.lib().rpn_head_trainer_get_bn(self._t, name.encode(), *([fpp(bn[k]) for k in BN_KEYS] + [stream])),
                            "rpn_head_trainer_get_bn(%s)" % name)
                elif name in self._mn:
                    kernel = self._mn[name]["kernel"].copy()
                    bn = {k: self._mn[name][k].copy() for k in BN_KEYS}
                else:
                    continue
                out[name] = {"kernel": kernel}
                out[layer["bn_name"]] = bn
                continue
            if self._t:
                kernel = np.empty(layer["shape"], dtype=np.float32)
                bias = np.empty((layer["shape"][3],), dtype=np.float32)
                L.check(L.lib().rpn_head_trainer_get_layer(self._t, name.encode(), kernel.ctypes.data_as(L.c_float_p),
                                                           bias.ctypes.data_as(L.c_float_p),
                                                           L.stream_ptr() if torch.cuda.is_available() else None),
                        "rpn_head_trainer_get_layer(%s)" % name)
            elif name in self._head:
                kernel, bias = (a.copy() for a in self._head[name])
            elif name in self._backbone:
                kernel, bias = (a.copy() for a in self._backbone[name])
            else:
                continue
            out[name] = {"kernel": kernel, "bias": bias}
        return out

    def _sync_head(self):
        """After training: every trained layer into the inference handle (once, before the next forward), which repacks it at
        its own precision."""
        if not self._head_dirty:
            return
        lib = L.lib()
        got = self.get_weights()
        for name, d in got.items():
            if "kernel" not in d:           # a BatchNorm entry: goes with its conv
                continue
            if self._is_mn(name):           # refolded from kernel + gamma / beta / the updated moving statistics
                bn = [got[self._bn_of[name]][k].ctypes.data_as(L.c_float_p) for k in BN_KEYS]
                L.check(lib.rpn_model_set_layer(self._h, name.encode(), d["kernel"].ctypes.data_as(L.c_float_p), None, *bn),
                        "rpn_model_set_layer(%s)" % name)
                continue
            L.check(lib.rpn_model_set_layer(self._h, name.encode(), d["kernel"].ctypes.data_as(L.c_float_p),
                                            d["bias"].ctypes.data_as(L.c_float_p), None, None, None, None),
                    "rpn_model_set_layer(%s)" % name)
        self._head_dirty = False

    def _batch_args(self, x, y):
        if not self._t:
            raise RuntimeError("call compile() before training or evaluating the model")
        if not isinstance(y, (tuple, list)) or len(y) != 2:
            raise ValueError("y must be (bbox_deltas, bbox_labels), as rpn_generator yields it")
        imgs, _ = L.to_device(x)
        deltas, _ = L.to_device(y[0])
        labels, _ = L.to_device(y[1])
        B = int(imgs.shape[0]) if imgs.dim() == 4 else -1
        F, K = self.feature_map_shape, self.anchor_count
        if tuple(imgs.shape) != (B, self.img_size, self.img_size, 3):
            raise ValueError("imgs must be (B,%d,%d,3) NHWC, got %s" % (self.img_size, self.img_size, tuple(imgs.shape)))
        if deltas.numel() != B * F * F * K * 4 or labels.numel() != B * F * F * K:
            raise ValueError("bbox_deltas must be (B,%d,4) and bbox_labels (B,%d,%d,%d); got %s, %s"
                             % (F * F * K, F, F, K, tuple(deltas.shape), tuple(labels.shape)))
        if not 1 <= B <= self.max_batch:
            raise ValueError("batch %d outside [1, %d]" % (B, self.max_batch))
        return imgs, deltas, labels, B

    def _step(self, x, y, update):
        imgs, deltas, labels, B = self._batch_args(x, y)
        self._pending = None                    # the library's forward replaces a pending one
        losses = torch.empty((3,), dtype=torch.float32, device="cuda")
        lr, b1, b2, eps = self._step_opt() if update else self._opt
        L.check(L.lib().rpn_head_trainer_step(self._t, L.ptr(imgs), B, L.ptr(deltas), L.ptr(labels), 1 if update else 0, lr, b1,
                                              b2, eps, L.ptr(losses), L.stream_ptr()), "rpn_head_trainer_step")
        if update:
            self._head_dirty = True
        return losses, B

    def _trainer_outputs(self, B):
        F, K = self.feature_map_shape, self.anchor_count
        reg = torch.empty((B, F, F, 4 * K), dtype=torch.float32, device="cuda")
        cls = torch.empty((B, F, F, K), dtype=torch.float32, device="cuda")
        L.check(L.lib().rpn_head_trainer_outputs(self._t, L.ptr(reg), L.ptr(cls), B, L.stream_ptr()), "rpn_head_trainer_outputs")
        return [reg, cls]

    def forward_for_training(self, x, y):
        """The first half of a training step: forward pass and losses, nothing updated yet -> ``(losses, feat, [reg, cls])``.

        ``losses``: CUDA tensor [loss, rpn_reg_loss, rpn_cls_loss] (not read back: no host synchronisation).  ``feat``: a fresh
        float32 CUDA tensor (B,F,F,C), the trainer's own feature tap -- ``block5_conv3`` after its ReLU / ``block_13_expand`` after
        its ReLU6, computed in exact float32 from the master weights, BatchNorm with the batch statistics on MobileNetV2 -- that the
        caller may set ``requires_grad_()`` on and build a second-stage loss from.  ``[reg, cls]``: the float32 head outputs.
        ``apply_gradients`` runs the second half.  A later ``forward_for_training`` / ``train_on_batch`` / ``test_on_batch`` replaces
        the pending forward (on MobileNetV2 the moving BatchNorm statistics are updated by every training forward)."""
        imgs, deltas, labels, B = self._batch_args(x, y)
        self._pending = None
        losses = torch.empty((3,), dtype=torch.float32, device="cuda")
        L.check(L.lib().rpn_head_trainer_forward(self._t, L.ptr(imgs), B, L.ptr(deltas), L.ptr(labels), 1, L.ptr(losses),
                                                 L.stream_ptr()), "rpn_head_trainer_forward")
        self._pending = (imgs, B)               # the backward reads the same image batch: keep it alive
        if self._train_from is not None and self.backbone != "vgg16":
            self._head_dirty = True             # the moving statistics moved
        C = self.activation_shape(self.tap_layer)[3]
        feat = torch.empty((B, self.feature_map_shape, self.feature_map_shape, C), dtype=torch.float32, device="cuda")
        L.check(L.lib().rpn_head_trainer_feature(self._t, L.ptr(feat), B, L.stream_ptr()), "rpn_head_trainer_feature")
        return losses, feat, self._trainer_outputs(B)

    def apply_gradients(self, feature_grad=None):
        """The second half of the step ``forward_for_training`` began: head backward, backbone backward, one Adam step.

        ``feature_grad``: None, or a contiguous float32 CUDA tensor (B,F,F,C) -- the gradient of a second-stage loss with respect to
        ``feat``; the backbone then trains on the RPN's gradient plus this one (it enters before the tap's activation mask).  The
        head layers' gradients do not depend on it.  ValueError for a bad tensor, and for any ``feature_grad`` on a model compiled
        without a backbone span (nothing below the tap trains); RuntimeError without a pending ``forward_for_training``."""
        if not self._t:
            raise RuntimeError("call compile() before training or evaluating the model")
        if feature_grad is not None and self._train_from is None:
            # (rpn_head_trainer_backward refuses the same call with the same reason, for callers of the C ABI)
            raise ValueError("feature_grad given to a model compiled with a frozen backbone: nothing below the feature tap trains, so "
                             "the gradient would be dropped -- compile with train_backbone_from=<layer> or train_backbone=True")
        F = self.feature_map_shape
        C = self.activation_shape(self.tap_layer)[3]
        pend = self._pending
        if feature_grad is not None:
            g = feature_grad
            if not isinstance(g, torch.Tensor):
                raise ValueError("feature_grad must be a torch tensor, got %s" % type(g).__name__)
            ok_b = int(g.shape[0]) == pend[1] if (pend and g.dim() == 4) else (g.dim() == 4 and 1 <= int(g.shape[0]) <= self.max_batch)
            if g.dim() != 4 or tuple(g.shape[1:]) != (F, F, C) or not ok_b:
                raise ValueError("feature_grad must be (%s,%d,%d,%d), the shape of forward_for_training's feat; got %s"
                                 % (pend[1] if pend else "B", F, F, C, tuple(g.shape)))
            if g.dtype != torch.float32 or not g.is_contiguous() or not g.is_cuda:
                raise ValueError("feature_grad must be a contiguous float32 CUDA tensor, got %s on %s%s"
                                 % (g.dtype, g.device, "" if g.is_contiguous() else ", not contiguous"))
        if pend is None:
            raise RuntimeError("apply_gradients needs a pending forward_for_training (each one is applied once; train_on_batch and "
                               "test_on_batch replace it)")
        imgs, B = pend
        self._pending = None
        lr, b1, b2, eps = self._step_opt()
        L.check(L.lib().rpn_head_trainer_backward(self._t, L.ptr(imgs), B, L.ptr(feature_grad), lr, b1, b2, eps, L.stream_ptr()),
                "rpn_head_trainer_backward")
        self._head_dirty = True

    def train_on_batch(self, x, y, second_stage=None):
        """One Adam step on ``y = (bbox_deltas, bbox_labels)`` (what ``rpn_generator`` yields) -> [loss, rpn_reg_loss,
        rpn_cls_loss], computed with the weights before the update (Keras order; loss = reg_loss + cls_loss, unit weights).

        ``second_stage(feat, reg, cls)``: joint training.  It gets the trainer's float32 feature tap (requiring grad) and the head
        outputs of this step and returns a scalar torch loss built from ``feat`` with torch operations (``roi_utils.roi_pooling``
        first, typically).  The model calls ``.backward()`` on it and hands ``feat.grad`` to the backbone's backward (a loss that does
        not touch ``feat`` gives none: the plain step); the caller steps its own optimizer for the second stage's parameters.  Returns
        [loss + second, rpn_reg_loss, rpn_cls_loss, second].  Needs a trained backbone span (``train_backbone_from`` /
        ``train_backbone``).  Everything stays on the current stream; the one host synchronisation is the losses' readback."""
        if second_stage is None:
            losses, _ = self._step(x, y, True)
            return [float(v) for v in losses.cpu().numpy()]
        if not self._t:
            raise RuntimeError("call compile() before training or evaluating the model")
        if self._train_from is None:
            raise ValueError("second_stage needs a trained backbone span: this model was compiled with a frozen backbone, so nothing "
                             "below the feature tap trains and the second stage's gradient would be dropped -- compile with "
                             "train_backbone_from=<layer> or train_backbone=True")
        losses, feat, (reg, cls) = self.forward_for_training(x, y)
        feat.requires_grad_()
        with torch.enable_grad():
            second = second_stage(feat, reg, cls)
        if not isinstance(second, torch.Tensor) or second.numel() != 1 or not second.requires_grad:
            self._pending = None
            raise ValueError("second_stage must return a scalar torch loss that requires grad")
        second.backward()
        g = feat.grad
        self.apply_gradients(None if g is None else g.contiguous())
        vals = torch.cat([losses, second.detach().reshape(1).to(device="cuda", dtype=torch.float32)]).cpu().numpy()
        total = np.float32(np.float32(vals[1] + vals[2]) + vals[3])
        return [float(total), float(vals[1]), float(vals[2]), float(vals[3])]

    def test_on_batch(self, x, y, return_outputs=False):
        """[loss, rpn_reg_loss, rpn_cls_loss] without an update (Adam's t is not advanced).  ``return_outputs``: also the
        float32 head outputs [rpn_reg (B,F,F,4K), rpn_cls (B,F,F,K)] of this evaluation, as CUDA tensors."""
        losses, B = self._step(x, y, False)
        out = [float(v) for v in losses.cpu().numpy()]
        if not return_outputs:
            return out
        return out, self._trainer_outputs(B)

    def train_steps(self):
        """Adam's t: the number of applied steps since compile."""
        return int(L.lib().rpn_head_trainer_steps(self._t)) if self._t else 0

    def fit(self, generator, steps_per_epoch, epochs=1, validation_data=None, validation_steps=None, second_stage=None):
        """trainer.py:64-69 without the ModelCheckpoint callback: ``steps_per_epoch`` batches of ``generator`` per epoch, then
        ``validation_steps`` batches of ``validation_data`` evaluated.  Returns the history dict of the per-epoch means:
        {"loss", "rpn_reg_loss", "rpn_cls_loss"} (+ the same with a "val_" prefix).  ``second_stage``: passed to every
        ``train_on_batch`` (joint training); the history then has "second_stage_loss" too, and "loss" includes it."""
        keys = ("loss", "rpn_reg_loss", "rpn_cls_loss")
        tkeys = keys + (("second_stage_loss",) if second_stage is not None else ())
        history = {k: [] for k in tkeys}
        if validation_data is not None:
            history.update({"val_" + k: [] for k in keys})
        it = iter(generator)
        vit = iter(validation_data) if validation_data is not None else None
        for _epoch in range(int(epochs)):
            sums = np.zeros(len(tkeys))
            for _ in range(int(steps_per_epoch)):
                x, y = next(it)
                sums += self.train_on_batch(x, y) if second_stage is None else self.train_on_batch(x, y, second_stage=second_stage)
            for k, v in zip(tkeys, sums / max(1, int(steps_per_epoch))):
                history[k].append(float(v))
            if vit is not None:
                n = int(validation_steps) if validation_steps else 1
                vs = np.zeros(3)
                for _ in range(n):
                    x, y = next(vit)
                    vs += self.test_on_batch(x, y)
                for k, v in zip(keys, vs / n):
                    history["val_" + k].append(float(v))
        return history

    def __del__(self):
        try:
            if self._t:
                L.lib().rpn_head_trainer_destroy(self._t)
                self._t = L.vp(0)
        except Exception:
            pass
        try:
            if self._h:
                L.lib().rpn_model_destroy(self._h)
                self._h = L.vp(0)
        except Exception:
            pass


def synthetic_weights(backbone, hyper_params, seed=1):
    """Seeded random-init weights of the right architecture (there is no network access for
    ImageNet / trained checkpoints): He-normal kernels (std = sqrt(2 / fan_in)), small uniform
    biases, ``rpn_reg`` scaled by 0.1 so that |dh|,|dw| stay small after ``x variances``
    (SURVEY.md 8d, H6).  MobileNetV2 BatchNorm gets seeded non-trivial (gamma, beta, mean, var).
    Keys are Keras layer names.  The layer table comes from the native graph builder."""
    probe = RPNModel(backbone, hyper_params, max_batch=1)
    rng = np.random.RandomState(seed)
    weights = {}
    for layer in probe.layers:
        R, S, Cin, Cout = layer["shape"]
        fan_in = R * S * (1 if layer["kind"] == 2 else Cin)
        std = np.sqrt(2.0 / fan_in)
        kernel = (rng.standard_normal(layer["shape"]) * std).astype(np.float32)
        ch = Cin if layer["kind"] == 2 else Cout
        entry = {"kernel": kernel}
        if layer["kind"] == 0:
            entry["bias"] = rng.uniform(-0.05, 0.05, size=(ch,)).astype(np.float32)
        if layer["name"] == "rpn_reg":
            entry["kernel"] = (kernel * 0.1).astype(np.float32)
        weights[layer["name"]] = entry
        if layer["bn_name"]:
            weights[layer["bn_name"]] = {
                "gamma": rng.uniform(0.8, 1.2, size=(ch,)).astype(np.float32),
                "beta": rng.uniform(-0.1, 0.1, size=(ch,)).astype(np.float32),
                "mean": rng.uniform(-0.1, 0.1, size=(ch,)).astype(np.float32),
                "var": rng.uniform(0.8, 1.2, size=(ch,)).astype(np.float32),
            }
    del probe
    return weights
