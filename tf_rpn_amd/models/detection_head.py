"""The detection head of a Faster R-CNN second stage on MI355X: two fully-connected ReLU layers on the RoI features and the
cls | reg output pair, trained on the device (``rpn_det_head_*``; contract in ``include/rpn_hip.h``).

This module has NO counterpart in the reference, which stops at the proposals.  The architecture is this project's choice (the
Fast R-CNN head), as the thresholds of ``calculate_roi_targets`` are:

    pooled (B,R,ph,pw,Cf) --Flatten (NHWC: index (i*pw + j)*Cf + c)--> x (B*R, ph*pw*Cf)
    fc1: h1 = relu(x  W1 + b1)     fc2: h2 = relu(h1 W2 + b2)
    cls: logits = h2 Wc + bc  -> (B,R,C)  LOGITS         reg: deltas = h2 Wr + br  -> (B,R,4C)  class-specific

Kernels are Keras ``Dense`` kernels, (in, out).  Every training entry point of this library gives the same bits on every run,
and so does this one -- with dropout too (below).  Exact float32; a RoI's outputs do not depend on the batch it is part of.

``dropout=rate`` (trainable heads; default 0: nothing changes) drops the two hidden activations of every GRAD-MODE call the way
Keras' ``Dropout`` does, ``h * 1/(1 - rate) * mask``, with a seeded counter-based generator (Philox4x32-10; the contract is in
``include/rpn_hip.h``): an element is kept iff its 32-bit word, a function of ``(dropout_seed, call number, layer, row, column)``
alone, is ``>= min(llround(rate * 2^32), 2^32 - 1)``.  There is no generator state and no mask tensor: the same
``(weights, input, seed, call number)`` gives the same bits on every run, in float32 and in ``f16x3`` (which use the identical
mask), whatever the batch is shaped like.  Dropout is the identity under ``torch.no_grad()``, in ``detect`` and in every
inference head, and such calls do not advance the call number: VALIDATION THEREFORE RUNS UNDER ``torch.no_grad()``.

``precision="f16x3"`` (inference heads only) runs the three products on the float16 matrix cores with every float32 operand
carried as hi + lo float16 halves (``hi*hi + hi*lo + lo*hi``, float32 accumulation; the contract is in ``include/rpn_hip.h``):
the same batch independence and run-to-run bit identity, an error a little above float32's, and twice the weight memory (the
float32 weights are kept beside their packed image).  Features or activations beyond the float16 range raise a flag
(``status()``); the outputs of such a forward are invalid and the float32 head is the one to use.

A trainable head is created in float32 and may TRAIN in split float16: ``compile(..., precision="f16x3")`` runs every product
of the forward and of the backward in ``f16x3`` (the output gradients carried as the split of ``dZ * 2^t``, one power of two per
gradient tensor found on the device) while the master weights, the gradients, the bias sums and Adam stay float32.  Every forward
that is not kept (``torch.no_grad()``, ``detect``), and every grad-mode forward at dropout rate 0, is bit for bit the ``f16x3``
inference head's on the same weights; the packed image (a fifth copy of the weights: 2.4 GB in all
at 25 088 x 4096 x 4096) is refreshed on the device after every ``apply_gradients()``.
"""
import ctypes

import numpy as np
import torch

from .. import _lib as L
from ..utils import roi_utils
from . import _optimizer as O

LAYERS = ("fc1", "fc2", "cls", "reg")
PRECISIONS = ("f32", "f16x3")


def dropout(x, rate, seed, calls=0, layer=0):
    """The head's dropout on any 2-D float32 tensor (``rpn_dropout_forward``): ``keep ? x * 1/(1 - rate) : +0`` with the mask of
    hidden layer ``layer`` at call number ``calls`` -- element (m, n) is kept iff output word ``m & 3`` of Philox4x32-10 at counter
    ``(n, m >> 2, layer, calls mod 2^32)``, key ``(seed & 0xffffffff, seed >> 32)`` is ``>= min(llround(rate * 2^32), 2^32 - 1)``.
    No ReLU, out of place; returns a new CUDA tensor."""
    if not isinstance(x, torch.Tensor) or x.dim() != 2:
        raise ValueError("dropout takes a 2-D torch tensor (M, N)")
    x = L.to_device(x)[0]
    out = torch.empty_like(x)
    st = L.lib().rpn_dropout_forward(L.ptr(x), int(x.shape[0]), int(x.shape[1]), float(rate), int(seed) & (2 ** 64 - 1),
                                     int(calls) & 0xffffffff, int(layer), L.ptr(out), L.stream_ptr())
    L.check(st, "rpn_dropout_forward")
    return out


class _HeadFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, pooled, token, head):
        # token: the head's stand-in for its parameters in the torch graph (they live inside the object, not in torch), so that a
        # trainable head's outputs require grad even when `pooled` does not
        ctx.head = head
        ctx.save_for_backward(pooled)
        out = head._forward(pooled, keep=True)
        ctx.serial = head._serial                # the head keeps ONE forward's activations: this one's, until its next call
        return out

    @staticmethod
    def backward(ctx, grad_logits, grad_deltas):
        pooled, = ctx.saved_tensors
        head = ctx.head
        if ctx.serial != head._serial:
            raise ValueError("DetectionHead backward: the head has been called, given weights or stepped since this forward (call %d, now "
                             "%d); it keeps the activations of its most recent call only" % (ctx.serial, head._serial))
        B, R = int(pooled.shape[0]), int(pooled.shape[1])
        zeros = lambda n: torch.zeros((B, R, n), dtype=torch.float32, device="cuda")
        gl = grad_logits.contiguous() if grad_logits is not None else zeros(head.total_labels)
        gd = grad_deltas.contiguous() if grad_deltas is not None else zeros(4 * head.total_labels)
        want = ctx.needs_input_grad[0]
        gp = torch.empty_like(pooled) if want else None
        st = L.lib().rpn_det_head_backward(head._h, L.ptr(pooled), B * R, L.ptr(gl), L.ptr(gd), L.ptr(gp), L.stream_ptr())
        L.check(st, "DetectionHead backward")
        return gp, None, None


class DetectionHead(O.OptimizerMixin):
    """``head(pooled) -> (cls_logits (B,R,C), reg_pred (B,R,4C))`` on torch CUDA tensors; ``pooled`` (B,R,ph,pw,Cf) is what
    ``roi_utils.roi_pooling`` returns, B*R <= ``max_rois``.

    With grad mode on, a call on a trainable head -- or on a ``pooled`` that requires grad -- is a ``torch.autograd.Function``:
    its backward runs ``rpn_det_head_backward``, leaves the eight parameter gradients inside the object (``get_gradients()``;
    ``apply_gradients()`` is one Adam launch over all of them) and returns the gradient with respect to ``pooled``, which flows
    on through ``roi_pooling`` into the feature map.  The head keeps the activations of ONE forward, so a backward must belong
    to the head's most recent call: after any other call of the head (kept or not: a second batch, a ``detect``), a
    ``set_weights`` or an ``apply_gradients`` the backward of an earlier call raises ``ValueError`` instead of computing from
    another call's activations.  Each backward REPLACES the stored parameter gradients; they do not accumulate over calls, so
    it is one forward, one backward, one ``apply_gradients``.  Under ``torch.no_grad()`` nothing is kept.  ``trainable=False`` is the inference head: weights and the two hidden activations only.

    ``dropout``, ``dropout_seed``: the rate in [0, 1) and the 64-bit seed of the dropout after the two hidden layers (module
    docstring; ``set_dropout``, ``dropout_state``).  ``dropout_seed=None`` means ``seed``, or 0 when ``seed`` is None.
    ``dropout > 0`` needs ``trainable=True``.  It applies to grad-mode calls only: run validation under ``torch.no_grad()``.

    ``precision``: ``"f32"`` (exact float32, the default) or ``"f16x3"`` (split float16 on the 16-bit matrix cores; needs
    ``trainable=False``).  ``head.precision`` reports it.  A trainable head is always constructed in float32; the precision it
    TRAINS in is ``compile``'s ``precision`` (``head.train_precision``).

    Initial weights are Keras' ``Dense`` defaults, Glorot-uniform kernels and zero biases, drawn from ``seed``; ``seed=None`` sets
    none (every layer must then be given with ``set_weights`` before the first call)."""

    def __init__(self, total_labels, pooling_size=(7, 7), channels=512, hidden=(4096, 4096), max_rois=8 * 300, trainable=True,
                 seed=0, precision="f32", dropout=0.0, dropout_seed=None):
        if precision not in PRECISIONS:
            raise ValueError("precision must be one of %r, got %r" % (PRECISIONS, precision))
        if precision == "f16x3" and trainable:
            raise ValueError("precision 'f16x3' is the inference head's: pass trainable=False (training stays exact float32)")
        if not 0.0 <= float(dropout) < 1.0:                  # (a NaN fails both compares)
            raise ValueError("dropout must be in [0, 1), got %r" % (dropout,))
        if float(dropout) > 0.0 and not trainable:
            raise ValueError("dropout applies to the kept (grad-mode) forwards of a trainable head: pass trainable=True")
        self.precision = precision
        self.total_labels = int(total_labels)
        self.pooling_size = tuple(int(v) for v in pooling_size)
        self.channels, self.hidden = int(channels), tuple(int(v) for v in hidden)
        self.max_rois, self.trainable = int(max_rois), bool(trainable)
        if len(self.pooling_size) != 2 or len(self.hidden) != 2:
            raise ValueError("pooling_size and hidden must have two entries each, got %r and %r" % (pooling_size, hidden))
        ph, pw = self.pooling_size
        h = L.vp(0)
        L.check(L.lib().rpn_det_head_create_ex(ph, pw, self.channels, self.hidden[0], self.hidden[1], self.total_labels, self.max_rois,
                                               int(self.trainable), L.PRECISIONS[precision], ctypes.byref(h)), "rpn_det_head_create")
        self._h = h
        self.features = ph * pw * self.channels
        C = self.total_labels
        self.shapes = {"fc1": (self.features, self.hidden[0]), "fc2": self.hidden, "cls": (self.hidden[1], C),
                       "reg": (self.hidden[1], 4 * C)}
        self._opt = None
        self._token = None
        self._serial = 0                         # counts what invalidates a kept forward: calls, set_weights, apply_gradients, set_dropout
        self._kept_rows = 0                      # rows of the most recent call when it was kept
        self.compile()
        if self.trainable:
            self.set_dropout(dropout, seed=dropout_seed if dropout_seed is not None else (seed if seed is not None else 0))
        if torch.cuda.is_available() and seed is not None:   # (without a device the object still answers shape and memory questions;
            # seed=None: the caller sets every layer itself)
            self.set_weights(self.initial_weights(seed))

    def __del__(self):
        h, self._h = getattr(self, "_h", None), None
        if h:
            try:
                L.lib().rpn_det_head_destroy(h)
            except Exception:
                pass

    # ---- weights ------------------------------------------------------------------------
    def initial_weights(self, seed=0):
        """Keras ``Dense`` defaults: kernel ~ U(-l, l), l = sqrt(6 / (fan_in + fan_out)); bias 0."""
        rng = np.random.RandomState(seed)
        out = {}
        for name in LAYERS:
            fan_in, fan_out = self.shapes[name]
            limit = np.sqrt(6.0 / (fan_in + fan_out))
            out[name] = {"kernel": rng.uniform(-limit, limit, size=(fan_in, fan_out)).astype(np.float32),
                         "bias": np.zeros((fan_out,), np.float32)}
        return out

    def memory_bytes(self):
        """(weights -- with gradients and Adam's moments when trainable --, workspace) bytes of device memory the head holds"""
        w, ws = ctypes.c_size_t(0), ctypes.c_size_t(0)
        L.check(L.lib().rpn_det_head_memory_bytes(self._h, ctypes.byref(w), ctypes.byref(ws)), "rpn_det_head_memory_bytes")
        return int(w.value), int(ws.value)

    def set_weights(self, weights, partial=False):
        """weights: {layer: {"kernel": (in, out), "bias": (out,)}}, layers "fc1", "fc2", "cls", "reg".  ``partial``: layers absent
        from ``weights`` are left as they are.  Returns the names of the layers set."""
        done = []
        for name in LAYERS:
            if name not in weights:
                if partial:
                    continue
                raise KeyError("weights for layer %r are missing" % name)
            kernel = np.ascontiguousarray(weights[name]["kernel"], dtype=np.float32)
            bias = np.ascontiguousarray(weights[name]["bias"], dtype=np.float32)
            if tuple(kernel.shape) != tuple(self.shapes[name]) or tuple(bias.shape) != (self.shapes[name][1],):
                raise ValueError("layer %r: kernel %s / bias %s, expected %s / (%d,)" % (name, kernel.shape, bias.shape,
                                                                                         tuple(self.shapes[name]), self.shapes[name][1]))
            self._serial += 1
            L.check(L.lib().rpn_det_head_set_layer(self._h, name.encode(), kernel.ctypes.data_as(L.c_float_p),
                                                   bias.ctypes.data_as(L.c_float_p)), "rpn_det_head_set_layer(%s)" % name)
            done.append(name)
        return done

    def _get(self, fn, what):
        out = {}
        for name in LAYERS:
            kernel = np.empty(self.shapes[name], dtype=np.float32)
            bias = np.empty((self.shapes[name][1],), dtype=np.float32)
            L.check(fn(self._h, name.encode(), kernel.ctypes.data_as(L.c_float_p), bias.ctypes.data_as(L.c_float_p), L.stream_ptr()),
                    "%s(%s)" % (what, name))
            out[name] = {"kernel": kernel, "bias": bias}
        return out

    def get_weights(self):
        """{layer: {"kernel", "bias"}} as numpy arrays (synchronises the current stream)"""
        return self._get(L.lib().rpn_det_head_get_layer, "rpn_det_head_get_layer")

    def get_gradients(self):
        """{layer: {"kernel", "bias"}}: the parameter gradients the last backward left in the head"""
        return self._get(L.lib().rpn_det_head_get_gradient, "rpn_det_head_get_gradient")

    def inference_copy(self, precision="f32"):
        """a new inference head (``trainable=False``) of the same shape at ``precision`` holding this head's current weights"""
        if precision not in PRECISIONS:
            raise ValueError("precision must be one of %r, got %r" % (PRECISIONS, precision))
        weights = self.get_weights()
        head = DetectionHead(self.total_labels, pooling_size=self.pooling_size, channels=self.channels, hidden=self.hidden,
                             max_rois=self.max_rois, trainable=False, seed=None, precision=precision)
        head.set_weights(weights)
        return head

    # ---- dropout ------------------------------------------------------------------------
    def set_dropout(self, rate, seed=None, calls=None):
        """The dropout rate in [0, 1) of the grad-mode calls from here on; ``seed`` (None: unchanged) and ``calls``, the call number
        the next dropped call will use (None: unchanged; it starts at 0 and counts the calls that applied dropout), are what a resumed
        run restores from ``dropout_state()``.  A kept forward is dropped: its backward raises ``ValueError``."""
        if not self.trainable:
            raise ValueError("set_dropout needs a trainable head (dropout applies to kept forwards only)")
        state = self.dropout_state()
        self._serial += 1
        L.check(L.lib().rpn_det_head_set_dropout(self._h, float(rate), int(state["seed"] if seed is None else seed) & (2 ** 64 - 1)),
                "rpn_det_head_set_dropout")
        if calls is not None:
            L.check(L.lib().rpn_det_head_set_dropout_calls(self._h, int(calls)), "rpn_det_head_set_dropout_calls")

    def dropout_state(self):
        """{"rate", "seed", "calls"}: with the weights and the optimiser's state, what reproduces the next dropped call"""
        rate, seed, calls = ctypes.c_double(0.0), ctypes.c_ulonglong(0), ctypes.c_ulonglong(0)
        L.check(L.lib().rpn_det_head_dropout_state(self._h, ctypes.byref(rate), ctypes.byref(seed), ctypes.byref(calls)),
                "rpn_det_head_dropout_state")
        return {"rate": float(rate.value), "seed": int(seed.value), "calls": int(calls.value)}

    def kept_activation(self, name):
        """the hidden activation ``"fc1"`` (M, H1) or ``"fc2"`` (M, H2) the most recent grad-mode call stored for its backward (dropped
        and scaled when dropout applied), as a new torch tensor; ``ValueError`` when no forward is kept"""
        if name not in ("fc1", "fc2"):
            raise ValueError("kept_activation: %r is not a hidden layer (fc1, fc2)" % (name,))
        rows = self._kept_rows
        out = torch.empty((max(rows, 1), self.shapes[name][1]), dtype=torch.float32, device="cuda")
        L.check(L.lib().rpn_det_head_get_activation(self._h, name.encode(), L.ptr(out), rows, L.stream_ptr()), "rpn_det_head_get_activation")
        return out

    def status(self, reset=False):
        """Sticky flags raised on the device by the forwards so far -> {"f16_range": bool}.  ``f16_range`` (``precision="f16x3"``
        or a head compiled with it; a float32 head always reports False): a pooled feature or a hidden activation did not fit
        float16 (|x| > 65504 or non-finite), or an output gradient was non-finite; the outputs of that forward / backward are
        invalid -- use the float32 head.  Synchronises the current stream."""
        flags = ctypes.c_uint(0)
        stream = L.stream_ptr() if torch.cuda.is_available() else None     # (without a device there is no flag either)
        L.check(L.lib().rpn_det_head_status(self._h, ctypes.byref(flags), 1 if reset else 0, stream), "rpn_det_head_status")
        return {"f16_range": bool(flags.value & L.STATUS_F16_RANGE)}

    def save_weights(self, path):
        """a flat ``.npz`` with keys ``<layer>/<param>``, the form ``RPNModel.save_weights`` writes"""
        np.savez(path, **{"%s/%s" % (layer, p): v for layer, d in self.get_weights().items() for p, v in d.items()})

    def load_weights(self, path, by_name=True):
        data = np.load(path)
        weights = {}
        for key in data.files:
            layer, param = key.rsplit("/", 1)
            if layer in LAYERS:
                weights.setdefault(layer, {})[param] = data[key]
        return self.set_weights(weights, partial=bool(by_name))

    def load_keras_weights(self, path, layers=("fc1", "fc2")):
        """Start the hidden layers from a Keras VGG16 ``.h5`` (a weights file or a full model): reads the layer groups ``layers``
        with ``h5_weights.read_keras_weights`` and sets them (``set_weights(..., partial=True)``: ``cls`` / ``reg`` and the layers
        not named keep their values).  Returns the names set.  No transpose is needed: the head's flatten index
        ``(i * pw + j) * channels + c`` is Keras' ``Flatten`` of an NHWC tensor, so at the default shape ``fc1`` / ``fc2`` are
        exactly ``block5_pool -> flatten -> fc1 -> fc2`` -- layers trained on MAX-pooled ``block5_conv3`` features
        (``roi_utils.roi_max_pooling``).  ``ValueError``: a layer that is not ``fc1`` / ``fc2``, that the file does not hold, or
        whose kernel is not the head's ``(ph * pw * channels, H1)`` / ``(H1, H2)``."""
        from ..utils import h5_weights
        layers = tuple(layers)
        for name in layers:
            if name not in ("fc1", "fc2"):
                raise ValueError("load_keras_weights: %r is not a hidden layer of the head (fc1, fc2)" % (name,))
        weights, _info = h5_weights.read_keras_weights(path)
        chosen = {}
        for name in layers:
            layer = weights.get(name)
            if not layer or "kernel" not in layer or "bias" not in layer:
                raise ValueError("load_keras_weights: the file holds no layer %r with a kernel and a bias (its layers: %s)"
                                 % (name, ", ".join(weights)))
            kernel, bias = np.asarray(layer["kernel"]), np.asarray(layer["bias"])
            want = tuple(self.shapes[name])
            if tuple(kernel.shape) != want or tuple(bias.shape) != (want[1],):
                raise ValueError("load_keras_weights: layer %r has kernel %s / bias %s in the file, the head's is %s / (%d,)"
                                 % (name, tuple(kernel.shape), tuple(bias.shape), want, want[1]))
            chosen[name] = {"kernel": kernel, "bias": bias}
        return self.set_weights(chosen, partial=True)

    # ---- forward / backward -------------------------------------------------------------
    def _forward(self, pooled, keep):
        B, R = int(pooled.shape[0]), int(pooled.shape[1])
        C = self.total_labels
        logits = torch.empty((B, R, C), dtype=torch.float32, device="cuda")
        deltas = torch.empty((B, R, 4 * C), dtype=torch.float32, device="cuda")
        self._serial += 1
        st = L.lib().rpn_det_head_forward(self._h, L.ptr(pooled), B * R, int(keep), L.ptr(logits), L.ptr(deltas), L.stream_ptr())
        L.check(st, "DetectionHead forward")
        self._kept_rows = B * R if keep else 0
        return logits, deltas

    def __call__(self, pooled):
        if not isinstance(pooled, torch.Tensor):
            raise TypeError("pooled must be a torch tensor (B, R, ph, pw, C)")
        expect = self.pooling_size + (self.channels,)
        if pooled.dim() != 5 or tuple(int(v) for v in pooled.shape[2:]) != expect:
            raise ValueError("pooled must be (B, R, %d, %d, %d), got %s" % (expect + (tuple(pooled.shape),)))
        if int(pooled.shape[0]) * int(pooled.shape[1]) > self.max_rois:
            raise ValueError("%d x %d RoIs, the head was made for at most %d" % (int(pooled.shape[0]), int(pooled.shape[1]), self.max_rois))
        grad = torch.is_grad_enabled() and (self.trainable or pooled.requires_grad)
        if grad and not self.trainable:
            raise RuntimeError("a gradient through DetectionHead needs trainable=True (the inference head keeps no activations)")
        x = L.to_device(pooled)[0]
        if grad:
            if self._token is None:
                self._token = torch.zeros((), dtype=torch.float32, device="cuda", requires_grad=True)
            return _HeadFunction.apply(x, self._token, self)
        return self._forward(x.detach(), keep=False)

    # ---- optimiser ----------------------------------------------------------------------
    def compile(self, learning_rate=1e-4, beta_1=0.9, beta_2=0.999, epsilon=1e-7, precision="f32", optimizer="adam", momentum=0.0,
                nesterov=False, weight_decay=0.0, global_clipnorm=None):
        """Adam's parameters (Keras' defaults but for the learning rate); the moments live in the head from its creation.

        ``optimizer``: ``"adam"`` (default) or ``"sgd"`` with ``momentum`` in [0, 1) and ``nesterov``; ``weight_decay``: L2 decay of
        the four kernels (never the biases), added to the gradient after the clip; ``global_clipnorm``: clip the whole gradient by
        its global norm (None / 0: off; NOT Keras' per-tensor ``clipnorm``).  The defaults launch exactly the Adam step the head
        always ran.  ``learning_rate``: a float or a callable ``f(applied_steps) -> float`` evaluated with ``train_steps()`` before
        every ``apply_gradients()``; ``head.learning_rate`` reads and sets it.  Compiling again with the same ``optimizer`` keeps
        the state; the other one zeroes ``m``, ``v`` and the step count.  README, "Optimizers".

        ``precision``: what a trainable head computes in from here on -- ``"f32"`` (exact float32) or ``"f16x3"`` (every product of the
        forward and the backward in split float16; master weights, gradients, bias sums and Adam stay float32).  Compiling again
        switches back and forth; the weights, Adam's moments and the step count are kept, a kept forward is dropped."""
        if precision not in PRECISIONS:
            raise ValueError("precision must be one of %r, got %r" % (PRECISIONS, precision))
        if precision == "f16x3" and not self.trainable:
            raise ValueError("compile(precision='f16x3') needs a trainable head; an inference head takes its precision at construction")
        cfg = O.check_config(optimizer, momentum, nesterov, weight_decay, global_clipnorm)
        lr = O.check_learning_rate(learning_rate)
        if cfg != (0, cfg[1], cfg[2], 0.0, 0.0) and not self.trainable:
            raise ValueError("optimizer, weight_decay and global_clipnorm need a trainable head")
        if self.trainable:
            self._serial += 1
            L.check(L.lib().rpn_det_head_set_train_precision(self._h, L.PRECISIONS[precision]), "rpn_det_head_set_train_precision")
        self._lr = lr
        self._opt = (0.0 if callable(lr) else lr, float(beta_1), float(beta_2), float(epsilon))
        if self.trainable:
            self._opt_cfg = cfg
            self._apply_optimizer_config()

    # what OptimizerMixin asks for
    def _opt_target(self):
        return (self._h if self.trainable else None), "rpn_det_head"

    def _opt_entries(self):
        return [(name, name, False, {"kernel": tuple(self.shapes[name]), "bias": (self.shapes[name][1],)}) for name in LAYERS]

    def _opt_touch(self):
        self._serial += 1

    @property
    def train_precision(self):
        """the precision of a trainable head's products (``compile``); an inference head reports its construction precision"""
        if not self.trainable:
            return self.precision
        return "f16x3" if int(L.lib().rpn_det_head_train_precision(self._h)) == L.PRECISIONS["f16x3"] else "f32"

    def apply_gradients(self):
        """one step of the compiled optimizer (Adam by default: one launch) from the gradients the last backward left"""
        self._serial += 1
        L.check(L.lib().rpn_det_head_adam_step(self._h, *(self._step_opt() + (L.stream_ptr(),))), "rpn_det_head_adam_step")

    def train_steps(self):
        return int(L.lib().rpn_det_head_steps(self._h))

    # ---- inference ----------------------------------------------------------------------
    def detect(self, rois, pooled, variances, valid=None, **nms_kwargs):
        """``head(pooled)`` then ``roi_utils.roi_detections``: (boxes (B,M,4), scores (B,M), classes (B,M), valid_detections (B,)).
        ``nms_kwargs`` go to ``roi_detections`` unfiltered: the sizes and thresholds, and ``nms="linear"`` / ``"gaussian"`` with
        ``sigma`` for Soft-NMS in place of the hard NMS."""
        with torch.no_grad():
            logits, deltas = self(pooled)
        return roi_utils.roi_detections(rois, deltas, logits, variances, valid=valid, **nms_kwargs)
