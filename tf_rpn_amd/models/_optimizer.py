"""What ``RPNModel`` and ``DetectionHead`` share around their update step (contract: ``include/rpn_hip.h``, "Optimizers"): the
``compile`` arguments ``optimizer``, ``momentum``, ``nesterov``, ``weight_decay``, ``global_clipnorm``, a learning rate that may be
a callable of the applied steps, ``grad_norm()`` and the optimizer's state (``get`` / ``set`` / ``save`` / ``load``).

A class that mixes this in provides ``_opt_target()`` -> (handle or None, C prefix), ``_opt_entries()`` -> the trained entries
``[(name, C layer name, is_bn, {param: shape})]`` in ``get_weights`` order, ``_opt_touch()`` (a state change drops a kept forward) and
``train_steps()``; it keeps ``self._opt = (lr, beta_1, beta_2, epsilon)`` for the step call."""
import ctypes

import numpy as np

from .. import _lib as L

OPTIMIZERS = {"adam": 0, "sgd": 1}
SLOTS = ("m", "v")


def check_config(optimizer, momentum, nesterov, weight_decay, global_clipnorm):
    """-> (kind, momentum, nesterov, weight_decay, clipnorm) as the C ABI takes them; ``ValueError`` for a bad value"""
    if optimizer not in OPTIMIZERS:
        raise ValueError("optimizer=%r: 'adam' or 'sgd'" % (optimizer,))
    momentum, weight_decay = float(momentum), float(weight_decay)
    clip = 0.0 if global_clipnorm is None else float(global_clipnorm)
    if not 0.0 <= momentum < 1.0:                            # (a NaN fails both compares)
        raise ValueError("momentum=%r must lie in [0, 1)" % (momentum,))
    if not (np.isfinite(weight_decay) and weight_decay >= 0.0):
        raise ValueError("weight_decay=%r must be finite and >= 0" % (weight_decay,))
    if not (np.isfinite(clip) and clip >= 0.0):
        raise ValueError("global_clipnorm=%r must be None or finite and >= 0 (the global norm over everything the object trains; "
                         "0 / None: off)" % (global_clipnorm,))
    return OPTIMIZERS[optimizer], momentum, 1 if nesterov else 0, weight_decay, clip


def check_learning_rate(learning_rate):
    if callable(learning_rate):
        return learning_rate
    lr = float(learning_rate)
    if not (np.isfinite(lr) and lr >= 0.0):
        raise ValueError("learning_rate=%r must be finite and >= 0, or a callable f(applied_steps) -> float" % (learning_rate,))
    return lr


class OptimizerMixin(object):
    _lr = 0.0
    _opt_cfg = (0, 0.0, 0, 0.0, 0.0)

    # ---- learning rate ------------------------------------------------------------------
    @property
    def learning_rate(self):
        """the value the next update will use: the float given to ``compile`` (or assigned here), or the callable's value at
        ``train_steps()``"""
        lr = self._lr
        return float(lr(self.train_steps())) if callable(lr) else float(lr)

    @learning_rate.setter
    def learning_rate(self, value):
        self._lr = check_learning_rate(value)

    def _step_opt(self):
        """(lr, beta_1, beta_2, epsilon) of the update about to run"""
        return (self.learning_rate,) + tuple(self._opt[1:])

    @property
    def optimizer(self):
        return {v: k for k, v in OPTIMIZERS.items()}[self._opt_cfg[0]]

    def _apply_optimizer_config(self):
        h, prefix = self._opt_target()
        if h:
            fn = getattr(L.lib(), prefix + "_set_optimizer")
            L.check(fn(h, *self._opt_cfg), prefix + "_set_optimizer")

    # ---- the global norm ----------------------------------------------------------------
    def grad_norm(self):
        """``{"norm", "scale"}``: the global norm of the loss gradient (before the clip) and the clip scale of the last applied step;
        ``ValueError`` when no ``global_clipnorm`` is configured or no step has run.  Synchronises the current stream."""
        h, prefix = self._opt_target()
        if not h:
            raise RuntimeError("call compile() first")
        norm, scale = ctypes.c_double(0.0), ctypes.c_float(0.0)
        L.check(getattr(L.lib(), prefix + "_grad_norm")(h, ctypes.byref(norm), ctypes.byref(scale), L.stream_ptr()), prefix + "_grad_norm")
        return {"norm": float(norm.value), "scale": float(scale.value)}

    def decay_ranges(self):
        """the decayed elements of the flat parameter buffer as an (n, 2) int64 array of sorted [begin, end) ranges: the kernels
        and nothing else (host arithmetic)"""
        h, prefix = self._opt_target()
        if not h:
            raise RuntimeError("call compile() first")
        fn = getattr(L.lib(), prefix + "_decay_ranges")
        n = int(fn(h, None, 0))
        out = np.zeros((max(n, 0), 2), dtype=np.int64)
        fn(h, out.ctypes.data_as(ctypes.POINTER(ctypes.c_longlong)), n)
        return out

    # ---- state --------------------------------------------------------------------------
    def _slot_call(self, write, name, cname, is_bn, slot, arrays):
        h, prefix = self._opt_target()
        fn = getattr(L.lib(), "%s_%s_%sslot" % (prefix, "set" if write else "get", "bn_" if is_bn else ""))
        ptrs = [a.ctypes.data_as(L.c_float_p) if a is not None else None for a in arrays]
        args = [h, cname.encode(), slot] + ptrs + ([] if write else [L.stream_ptr()])
        L.check(fn(*args), "%s(%s)" % (fn.__name__, name))

    def get_optimizer_state(self):
        """``{"optimizer", "steps", "slots": {entry: {param: {"m", "v"}}}}`` with the entries and parameter names of ``get_weights``
        (``kernel`` / ``bias``; a trained MobileNetV2 conv gives ``{conv: {"kernel"}}`` and ``{conv_BN: {"gamma", "beta"}}``).  ``m`` is
        Adam's first moment or SGD's accumulator, ``v`` Adam's second moment (zeros under SGD)."""
        h, _ = self._opt_target()
        if not h:
            raise RuntimeError("call compile() first")
        slots = {}
        for name, cname, is_bn, shapes in self._opt_entries():
            keys = list(shapes)
            entry = {k: {} for k in keys}
            for si, sname in enumerate(SLOTS):
                arrays = [np.empty(shapes[k], dtype=np.float32) for k in keys]
                self._slot_call(False, name, cname, is_bn, si, arrays + [None] * (2 - len(arrays)))
                for k, a in zip(keys, arrays):
                    entry[k][sname] = a
            slots[name] = entry
        return {"optimizer": self.optimizer, "steps": self.train_steps(), "slots": slots}

    def set_optimizer_state(self, state):
        """Restores what ``get_optimizer_state`` returned.  Call it AFTER ``compile`` (which configures the optimizer and, on
        ``RPNModel``, builds a new trainer with zero state).  ``ValueError`` when the optimizer kind, the set of entries or a shape
        does not match the compiled object."""
        h, prefix = self._opt_target()
        if not h:
            raise RuntimeError("call compile() first")
        if state.get("optimizer") != self.optimizer:
            raise ValueError("the state is %r's, the object was compiled with optimizer=%r" % (state.get("optimizer"), self.optimizer))
        entries = self._opt_entries()
        slots = state["slots"]
        if set(slots) != set(e[0] for e in entries):
            raise ValueError("the state holds %s, the object trains %s" % (sorted(slots), sorted(e[0] for e in entries)))
        staged = []
        for name, cname, is_bn, shapes in entries:
            if set(slots[name]) != set(shapes):
                raise ValueError("entry %r: the state holds %s, expected %s" % (name, sorted(slots[name]), sorted(shapes)))
            for si, sname in enumerate(SLOTS):
                arrays = []
                for k in shapes:
                    a = np.ascontiguousarray(slots[name][k][sname], dtype=np.float32)
                    if tuple(a.shape) != tuple(shapes[k]):
                        raise ValueError("entry %r %s/%s: shape %s, expected %s" % (name, k, sname, a.shape, tuple(shapes[k])))
                    arrays.append(a)
                staged.append((name, cname, is_bn, si, arrays + [None] * (2 - len(arrays))))
        steps = int(state["steps"])
        if steps < 0:
            raise ValueError("steps=%d" % steps)
        self._opt_touch()
        for item in staged:
            self._slot_call(True, *item)
        L.check(getattr(L.lib(), prefix + "_set_steps")(h, steps), prefix + "_set_steps")

    def save_optimizer_state(self, path):
        """a flat ``.npz``: ``<entry>/<param>/<m|v>`` arrays plus ``optimizer`` and ``steps`` (the form ``save_weights`` uses)"""
        st = self.get_optimizer_state()
        flat = {"%s/%s/%s" % (e, p, s): a for e, d in st["slots"].items() for p, sl in d.items() for s, a in sl.items()}
        np.savez(path, optimizer=np.array(st["optimizer"]), steps=np.array(st["steps"], dtype=np.int64), **flat)

    def load_optimizer_state(self, path):
        data = np.load(path)
        state = {"optimizer": str(data["optimizer"]), "steps": int(data["steps"]), "slots": {}}
        for key in data.files:
            if key in ("optimizer", "steps"):
                continue
            entry, param, slot = key.rsplit("/", 2)
            state["slots"].setdefault(entry, {}).setdefault(param, {})[slot] = data[key]
        self.set_optimizer_state(state)
