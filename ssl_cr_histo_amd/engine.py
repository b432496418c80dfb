"""Python face of the native engine (libsslcr.so): binds the nn.Module parameter containers of net.py to a
``sslcr_net`` and runs whole steps with one C call.  PyTorch is only the owner of device memory, streams and the
torch.distributed bootstrap here -- there is no torch-op fallback for any compute.
"""
import ctypes as C
import os
import weakref

import torch

from . import _lib as L
from .kernels import LossOptions, switches
from .net import Classifier, FinetuneResNet, TripletNet, TripletNet_Finetune, unwrap

_DTYPES = {"fp32": 0, "f32": 0, "float32": 0, "bf16": 1, "bfloat16": 1, "fp8": 2}     # fp8: bf16 engine + e4m3 forward convs (config 5)

SslcrNetDesc = L._S("sslcr_net_desc", "SslcrNetDesc", [
    ("params", C.POINTER(C.c_void_p)), ("nparams", C.c_int), ("bn_running_mean", C.POINTER(C.c_void_p)),
    ("bn_running_var", C.POINTER(C.c_void_p)), ("bn_num_batches_tracked", C.POINTER(C.c_void_p)),
    ("requires_grad", C.POINTER(C.c_uint8)), ("head_kind", C.c_int), ("num_classes", C.c_int), ("triplet", C.c_int)])
SslCrDesc = L._S("sslcr_ssl_cr_desc", "SslCrDesc", [
    ("kind", C.c_int), ("x_student", C.c_void_p), ("x_teacher", C.c_void_p), ("in_f32", C.c_int), ("nx", C.c_int),
    ("nu", C.c_int), ("H", C.c_int), ("W", C.c_int), ("target_f", C.c_void_p), ("target_i", C.c_void_p),
    ("lambda_u", C.c_float), ("nx_global", C.c_int), ("nu_global", C.c_int), ("feats", C.c_void_p), ("logits", C.c_void_p),
    ("logits_t", C.c_void_p), ("losses", C.c_void_p), ("backward", C.c_int), ("x_student2", C.c_void_p)])
SupDesc = L._S("sslcr_sup_desc", "SupDesc", [
    ("kind", C.c_int), ("x1", C.c_void_p), ("x2", C.c_void_p), ("x3", C.c_void_p), ("in_f32", C.c_int), ("n", C.c_int),
    ("H", C.c_int), ("W", C.c_int), ("target_f", C.c_void_p), ("target_i", C.c_void_p), ("n_global", C.c_int),
    ("feats", C.c_void_p), ("logits", C.c_void_p), ("losses", C.c_void_p), ("train", C.c_int), ("backward", C.c_int)])

_ENGINE_SIGS = {
    "sslcr_create": (C.c_int, [C.POINTER(C.c_void_p), C.c_int, C.c_int]),
    "sslcr_destroy": (C.c_int, [C.c_void_p]),
    "sslcr_profile": (C.c_int, [C.c_void_p, C.c_int]),
    "sslcr_profile_read": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(C.c_double)]),
    "sslcr_profile_dump": (C.c_int, [C.c_void_p, C.c_char_p, C.c_size_t]),
    "sslcr_comm_unique_id": (C.c_int, [C.c_void_p]),
    "sslcr_comm_init": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int]),
    "sslcr_comm_info": (C.c_int, [C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "sslcr_comm_all_reduce_f32": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    "sslcr_vcomm_create": (C.c_int, [C.POINTER(C.c_void_p), C.c_int]),
    "sslcr_vcomm_destroy": (C.c_int, [C.c_void_p]),
    "sslcr_comm_init_virtual": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int]),
    "sslcr_set_bn_sync": (C.c_int, [C.c_void_p, C.c_int]),
    "sslcr_set_aux_stream": (C.c_int, [C.c_void_p, C.c_int]),
    "sslcr_set_wgrad_stream": (C.c_int, [C.c_void_p, C.c_int]),
    "sslcr_net_create": (C.c_int, [C.c_void_p, C.POINTER(SslcrNetDesc), C.POINTER(C.c_void_p)]),
    "sslcr_net_destroy": (C.c_int, [C.c_void_p]),
    "sslcr_net_set_requires_grad": (C.c_int, [C.c_void_p, C.POINTER(C.c_uint8)]),
    "sslcr_net_pack": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p]),
    "sslcr_net_forward": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int,
                                    C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]),
    "sslcr_net_backward": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p]),
    "sslcr_net_set_grad_accumulate": (C.c_int, [C.c_void_p, C.c_int]),
    "sslcr_net_set_loss_opts": (C.c_int, [C.c_void_p, C.POINTER(L.LossOpts)]),
    "sslcr_net_grad": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]),
    "sslcr_net_debug_tap": (C.c_int, [C.c_void_p, C.c_int]),
    "sslcr_net_segments_used": (C.c_int, [C.c_void_p]),
    "sslcr_net_debug_tensor": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_size_t, C.POINTER(C.c_int), C.POINTER(C.c_int),
                                         C.c_void_p]),
    "sslcr_net_optimizer_step": (C.c_int, [C.c_void_p, C.POINTER(L.OptDesc), C.POINTER(C.c_void_p), C.POINTER(C.c_void_p),
                                           C.c_void_p]),
    "sslcr_net_optimizer_step_groups": (C.c_int, [C.c_void_p, C.POINTER(L.OptDesc), C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_void_p),
                                                  C.POINTER(C.c_void_p), C.POINTER(L.ClipDesc), C.c_void_p]),
    "sslcr_net_grad_norm": (C.c_int, [C.c_void_p, C.c_float, C.c_void_p, C.c_void_p]),
    "sslcr_net_lookahead": (C.c_int, [C.c_void_p, C.POINTER(C.c_void_p), C.c_float, C.c_void_p]),
    "sslcr_net_ema_from": (C.c_int, [C.c_void_p, C.c_void_p, C.c_float, C.c_void_p]),
    "sslcr_step_ssl_cr": (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(SslCrDesc), C.c_void_p]),
    "sslcr_step_supervised": (C.c_int, [C.c_void_p, C.POINTER(SupDesc), C.c_void_p]),
}
L.SIGNATURES.update(_ENGINE_SIGS)


def _ptr_array(tensors):
    arr = (C.c_void_p * len(tensors))()
    for i, t in enumerate(tensors):
        arr[i] = None if t is None else t.data_ptr()
    return arr


def _version_sig(tensors):
    return tuple((t.data_ptr(), t._version) for t in tensors)


def plan_optimizer(inner, params, names=None):
    """Map a torch optimizer onto the engine's group table.  Pure host logic: no device, nothing is modified.

    inner: torch.optim.Adam, AdamW or SGD(nesterov=True, dampening=0) with 1..8 param groups that are pairwise disjoint and whose
    union is exactly the requires_grad entries of `params` (named_parameters() order of (model, classifier)); `names` only serves
    the error messages.  -> (rows, group_of_param): rows[g] is a dict with the fields of sslcr_opt_desc for param group g -- lr,
    wd, beta1 / beta2 / eps or momentum, and bc1 / bc2 = 1 - beta ** step for the step ABOUT to be taken (the group's recorded
    step + 1), first_step = 1 for an SGD group in which some parameter has no momentum buffer yet; group_of_param[i] is the group
    of params[i], -1 for a frozen parameter."""
    def name(i):
        return names[i] if names is not None else f"parameter {i}"
    if isinstance(inner, torch.optim.AdamW):          # (a subclass of Adam in some torch versions: test it first)
        kind = 2
    elif isinstance(inner, torch.optim.Adam):
        kind = 0
    elif isinstance(inner, torch.optim.SGD):
        kind = 1
    else:
        raise L.SslcrError(f"optimizer {type(inner).__name__}: the engine serves Adam, AdamW and SGD(nesterov=True)")
    groups = inner.param_groups
    if not 1 <= len(groups) <= L.MAX_OPT_GROUPS:
        raise L.SslcrError(f"{type(inner).__name__} has {len(groups)} param groups; the engine serves 1 to {L.MAX_OPT_GROUPS}")
    index = {id(p): i for i, p in enumerate(params)}
    group_of = [-1] * len(params)
    rows = []
    for gi, g in enumerate(groups):
        if g.get("amsgrad", False) or g.get("maximize", False):
            raise NotImplementedError(f"param group {gi}: amsgrad / maximize are not served")
        step, first = 0.0, False
        for p in g["params"]:
            i = index.get(id(p))
            if i is None:
                raise L.SslcrError(f"param group {gi} holds a tensor of shape {tuple(p.shape)} that is no parameter of (model, classifier)")
            if not params[i].requires_grad:
                raise L.SslcrError(f"{name(i)} is frozen (requires_grad=False) but listed in param group {gi}")
            if group_of[i] >= 0:
                raise L.SslcrError(f"{name(i)} is listed in param groups {group_of[i]} and {gi}: groups must be disjoint")
            group_of[i] = gi
            st = inner.state.get(p, {})
            if kind == 1:
                first = first or st.get("momentum_buffer", None) is None
            elif "step" in st:
                step = float(st["step"])
        if kind == 1:
            if not g.get("nesterov", False) or g.get("dampening", 0) != 0:
                raise NotImplementedError(f"param group {gi}: the engine serves SGD(momentum, nesterov=True, dampening=0)")
            rows.append(dict(kind=1, lr=g["lr"], beta1=0.0, beta2=0.0, eps=0.0, wd=g["weight_decay"], momentum=g["momentum"], bc1=1.0,
                             bc2=1.0, first_step=int(first)))
        else:
            b1, b2 = g["betas"]
            rows.append(dict(kind=kind, lr=g["lr"], beta1=b1, beta2=b2, eps=g["eps"], wd=g["weight_decay"], momentum=0.0,
                             bc1=1 - b1 ** (step + 1), bc2=1 - b2 ** (step + 1), first_step=0))
    for i, p in enumerate(params):
        if p.requires_grad and group_of[i] < 0:
            raise L.SslcrError(f"{name(i)} requires grad but is in no param group: the groups' union must be exactly the "
                               "requires_grad parameters of (model, classifier)")
    return rows, group_of


class BoundNet:
    """one (model, classifier) pair registered with the engine."""

    def __init__(self, engine, model, classifier):
        self.engine = engine
        self.model = model
        self.classifier = classifier
        self.triplet = isinstance(model, TripletNet)
        if not isinstance(model, (TripletNet, TripletNet_Finetune)):
            raise TypeError("model must be ssl_cr_histo_amd.net.TripletNet or TripletNet_Finetune")
        if isinstance(classifier, FinetuneResNet):
            self.head_kind, self.ncls = 0, classifier.classifier[0].out_features
        elif isinstance(classifier, Classifier):
            self.head_kind, self.ncls = 1, classifier.classifier[2].out_features
        else:
            raise TypeError("classifier must be ssl_cr_histo_amd.net.FinetuneResNet or Classifier")
        self.params = [p for _, p in model.named_parameters()] + [p for _, p in classifier.named_parameters()]
        self.param_names = ["model." + k for k, _ in model.named_parameters()] + ["classifier." + k for k, _ in classifier.named_parameters()]
        self.last_grad_norm = None
        self._loss_keep = None          # tensors the library's sticky loss options point to (set_loss_options)
        dev = engine.device
        for p in self.params:
            if p.device != dev or p.dtype != torch.float32 or not p.is_contiguous():
                raise L.SslcrError(f"parameters must be contiguous fp32 tensors on {dev} (got {p.device}, {p.dtype})")
        self.bns = model.model.bn_modules()
        self._keep = (_ptr_array(self.params), _ptr_array([b.running_mean for b in self.bns]),
                      _ptr_array([b.running_var for b in self.bns]), _ptr_array([b.num_batches_tracked for b in self.bns]))
        self._rg = self._rg_flags()
        d = SslcrNetDesc(self._keep[0], len(self.params), self._keep[1], self._keep[2], self._keep[3],
                         (C.c_uint8 * len(self.params))(*self._rg), self.head_kind, self.ncls, int(self.triplet))
        h = C.c_void_p()
        L.check(L.lib().sslcr_net_create(engine.handle, C.byref(d), C.byref(h)))
        self.handle = h
        self._sig = None
        self._finalizer = weakref.finalize(self, BoundNet._destroy, h)

    @staticmethod
    def _destroy(h):
        try:
            L.lib().sslcr_net_destroy(h)
        except Exception:
            pass

    def _rg_flags(self):
        return [int(p.requires_grad) for p in self.params]

    def _tensors(self):
        out = list(self.params)
        for b in self.bns:
            out += [b.running_mean, b.running_var]
        return out

    def still_valid(self):
        """False when a parameter/buffer was re-allocated (e.g. module.to(), load into new storage)."""
        cur = [p for _, p in self.model.named_parameters()] + [p for _, p in self.classifier.named_parameters()]
        return len(cur) == len(self.params) and all(a is b for a, b in zip(cur, self.params)) and \
            all(a.data_ptr() == k for a, k in zip(self.params, self._keep[0]))

    def sync(self):
        """propagate host-side changes (requires_grad flips, load_state_dict, in-place edits) to the engine."""
        rg = self._rg_flags()
        if rg != self._rg:
            self._rg = rg
            L.check(L.lib().sslcr_net_set_requires_grad(self.handle, (C.c_uint8 * len(rg))(*rg)))
        sig = _version_sig(self._tensors())
        if sig != self._sig:
            L.check(L.lib().sslcr_net_pack(self.handle, 3, L.stream_ptr()))
            self._sig = sig

    # ------------------------------------------------------------------ forward / backward building blocks
    def forward(self, xs, train):
        """xs: tuple of 1 (Finetune) or 3 (TripletNet) NCHW uint8|fp32 device tensors -> (feats [N,768], logits [N,C])."""
        self.sync()
        xs = [self.engine.as_input(x) for x in xs]
        N, _, H, W = xs[0].shape
        feats = torch.empty((N, 768), dtype=torch.float32, device=self.engine.device)
        logits = torch.empty((N, self.ncls), dtype=torch.float32, device=self.engine.device)
        p = [L.ptr(x) for x in xs] + [None] * (3 - len(xs))
        L.check(L.lib().sslcr_net_forward(self.handle, int(train), p[0], p[1], p[2], int(xs[0].dtype == torch.float32),
                                          N, H, W, L.ptr(feats), L.ptr(logits), L.stream_ptr()))
        self._live_inputs = xs          # the stem wgrad re-reads the inputs in backward
        if train:
            self._note_buffers_changed()
        return feats, logits

    def set_grad_accumulate(self, on):
        """Gradient accumulation, torch's ``loss.backward()`` without ``optimizer.zero_grad()``.  Sticky: every later backward of
        this net (``backward`` and the backward leg of ``Engine.step_ssl_cr`` / ``step_supervised``, which set it from their own
        ``accumulate`` argument) leaves ``prev + new`` in the gradient buffer, elementwise in fp32, where ``prev`` is what the
        buffer held on entry and ``new`` what this backward alone would have left.  ``grad()``, ``grad_norm()`` and
        ``optimizer_step()`` (clipping included) see the sum.  A net without an earlier backward has no ``prev``: on is off there.

        * Train-mode BatchNorm uses each micro-batch's own statistics: the reference's per-replica statistics under
          ``nn.DataParallel``.
        * Running statistics and ``num_batches_tracked`` are updated by every micro-step in turn, as k successive torch forwards
          would; ``DataParallel`` keeps replica 0's only.
        * Nothing clears the buffer for the caller: accumulating onto a gradient that an optimizer step has already consumed
          adds to that stale gradient, as torch does without ``zero_grad``."""
        L.check(L.lib().sslcr_net_set_grad_accumulate(self.handle, int(bool(on))))

    def set_loss_options(self, opts, denominator=None, stats=None):
        """The options of the loss leg of ``Engine.step_ssl_cr`` (this net as the student) and ``step_supervised``: a
        ``LossOptions`` or None (the defaults: the launches and the bits of a net that never had options).  Sticky in the library,
        like ``set_grad_accumulate``; the step functions set it on every call from their own ``loss_options`` argument.
        denominator: device fp32 [1+], the supervised term's divisor over the whole global batch (``kernels.ce_denominator``, all-reduced
        when sharded) when the step holds a micro-batch or a shard; stats: device fp32 [2] that receives {#confident rows, sum of
        the teacher's max-probs}.  The tensors are kept alive here until the next call."""
        if opts is None and denominator is None and stats is None:
            if self._loss_keep is not None:
                L.check(L.lib().sslcr_net_set_loss_opts(self.handle, None))
                self._loss_keep = None
            return
        o, keep = (opts if opts is not None else LossOptions()).c_opts(self.engine.device, self.ncls, denominator, stats)
        L.check(L.lib().sslcr_net_set_loss_opts(self.handle, C.byref(o)))
        self._loss_keep = keep

    def backward(self, dlogits, accumulate=False):
        """backward of the last train-mode forward from d(loss)/d(logits).  accumulate: see ``set_grad_accumulate`` (set on every
        call, so the default stays off)."""
        self.set_grad_accumulate(accumulate)
        L.check(L.lib().sslcr_net_backward(self.handle, L.ptr(dlogits.contiguous()), L.stream_ptr()))

    def grad(self, index):
        """gradient of parameter `index` (named_parameters order) in PyTorch layout -- for tests/inspection."""
        out = torch.empty_like(self.params[index])
        L.check(L.lib().sslcr_net_grad(self.handle, index, L.ptr(out), L.stream_ptr()))
        return out

    @property
    def segments_used(self):
        """True when the last train-mode forward ran the TripletNet branches as segments of one launch per layer."""
        return bool(L.lib().sslcr_net_segments_used(self.handle))

    def debug_tap(self, on):
        """keep copies of every block's transient gradient tensors in backward (layer-wise parity test; see include/sslcr.h)."""
        L.check(L.lib().sslcr_net_debug_tap(self.handle, int(bool(on))))

    def debug_tensor(self, block, kind, pass_=0):
        """-> (tensor in the engine's storage dtype, flags) of pass `pass_` (a TripletNet branch); kinds and the bits of flags as in
        include/sslcr.h:sslcr_net_debug_tensor."""
        dims, flags = (C.c_int * 4)(), C.c_int()
        code = int(kind) | int(pass_) << 8
        L.check(L.lib().sslcr_net_debug_tensor(self.handle, block, code, None, 0, dims, C.byref(flags), L.stream_ptr()))
        shape = [d for d in dims]
        vec = 11 <= kind <= 14 or 21 <= kind <= 28
        dt = torch.float32 if vec or self.engine.dtype == 0 else torch.bfloat16
        out = torch.empty(shape[:1] if vec else shape, dtype=dt, device=self.engine.device)
        L.check(L.lib().sslcr_net_debug_tensor(self.handle, block, code, L.ptr(out), out.numel() * out.element_size(), dims,
                                               C.byref(flags), L.stream_ptr()))
        return out, flags.value

    def _note_buffers_changed(self):
        # the engine updated running stats / will update params through raw pointers: keep our signature in step so
        # that only *external* edits trigger a repack (the engine invalidates its own packs itself)
        self._sig = _version_sig(self._tensors())

    # ------------------------------------------------------------------ optimizer (state lives in the torch optimizer)
    def optimizer_step(self, optimizer, max_grad_norm=None):
        """one step of `optimizer` (Adam, AdamW or SGD-Nesterov, up to 8 param groups; Lookahead wraps one) on the gradients the
        engine holds.  max_grad_norm: torch.nn.utils.clip_grad_norm_(params, max_grad_norm) in front of the step, on the device
        and without a sync; [norm, coef] of that step is then ``self.last_grad_norm``."""
        inner = getattr(optimizer, "optimizer", optimizer)           # Lookahead wraps the real optimizer
        rows, group_of = plan_optimizer(inner, self.params, self.param_names)
        s1, s2 = [None] * len(self.params), [None] * len(self.params)
        for i, p in enumerate(self.params):
            if group_of[i] < 0:
                continue
            st = inner.state[p]
            if rows[group_of[i]]["kind"] == 1:
                if st.get("momentum_buffer", None) is None:
                    st["momentum_buffer"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                s1[i] = st["momentum_buffer"]
            else:
                if len(st) == 0:
                    st["step"] = torch.tensor(0.0)
                    st["exp_avg"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                    st["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                st["step"] += 1
                s1[i], s2[i] = st["exp_avg"], st["exp_avg_sq"]
        table = (L.OptDesc * len(rows))(*[L.OptDesc(r["kind"], r["lr"], r["beta1"], r["beta2"], r["eps"], r["wd"], r["momentum"], r["bc1"],
                                                    r["bc2"], r["first_step"], 1.0) for r in rows])
        gmap = (C.c_int * len(group_of))(*[max(g, 0) for g in group_of])
        clip = None
        if max_grad_norm is not None:
            if not float(max_grad_norm) >= 0.0:
                raise L.SslcrError(f"max_grad_norm must be a non-negative number (got {max_grad_norm!r})")
            out2 = torch.empty(2, dtype=torch.float32, device=self.engine.device)
            clip = C.byref(L.ClipDesc(float(max_grad_norm), out2.data_ptr()))
        self._opt_keep = (s1, s2, _ptr_array(s1), _ptr_array(s2))
        L.check(L.lib().sslcr_net_optimizer_step_groups(self.handle, table, len(rows), gmap, self._opt_keep[2], self._opt_keep[3], clip,
                                                        L.stream_ptr()))
        if max_grad_norm is not None:
            self.last_grad_norm = out2
        self._note_buffers_changed()

    def grad_norm(self, max_norm=float("inf")):
        """-> device tensor [norm, coef]: the global 2-norm of the gradients of the last backward and
        min(1, max_norm / (norm + 1e-6)), torch.nn.utils.clip_grad_norm_'s two numbers.  No sync."""
        out2 = torch.empty(2, dtype=torch.float32, device=self.engine.device)
        L.check(L.lib().sslcr_net_grad_norm(self.handle, float(max_norm), L.ptr(out2), L.stream_ptr()))
        return out2

    def lookahead(self, cached, alpha):
        arr = _ptr_array(cached)
        L.check(L.lib().sslcr_net_lookahead(self.handle, arr, float(alpha), L.stream_ptr()))
        self._note_buffers_changed()

    def ema_from(self, student, decay):
        L.check(L.lib().sslcr_net_ema_from(self.handle, student.handle, float(decay), L.stream_ptr()))
        self._note_buffers_changed()


class Engine:
    """one per process and device (one process per GPU)."""

    def __init__(self, device=None, dtype=None):
        if not torch.cuda.is_available():
            raise L.SslcrError("no MI355X visible: the engine has no CPU path")
        self.device = torch.device(device if device is not None else f"cuda:{torch.cuda.current_device()}")
        if self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        dtype = dtype or os.environ.get("SSLCR_DTYPE", "bf16")
        if dtype not in _DTYPES:
            raise ValueError(f"dtype must be one of {sorted(_DTYPES)}")
        self.dtype = _DTYPES[dtype]
        lib = L.lib()
        for name, (res, args) in _ENGINE_SIGS.items():
            fn = getattr(lib, name)
            fn.restype, fn.argtypes = res, args
        h = C.c_void_p()
        with torch.cuda.device(self.device):
            L.check(lib.sslcr_create(C.byref(h), self.device.index, self.dtype))
        self.handle = h
        self._bound = {}
        self._dummy_cls = None
        self.rank, self.world = 0, 1

    # ------------------------------------------------------------------ distributed (one process per GPU, RCCL inside)
    def init_comm(self, rank, world, broadcast_bytes):
        """broadcast_bytes(bytes_or_None) -> bytes : host-side broadcast of the 128-byte RCCL id from rank 0.
        world == 1 needs no communicator unless SSLCR_COMM_SELFTEST is set, and whether it is set is the library's answer
        (``kernels.switches()``, rule PRESENT: set at all, so an empty value counts here as it does in sslcr_comm_init)."""
        if world == 1 and not switches()["SSLCR_COMM_SELFTEST"]["value"]:
            return
        idbuf = (C.c_char * 256)()
        if rank == 0:
            L.check(L.lib().sslcr_comm_unique_id(idbuf))
        raw = broadcast_bytes(bytes(idbuf) if rank == 0 else None)
        idbuf = (C.c_char * 256).from_buffer_copy(raw)
        L.check(L.lib().sslcr_comm_init(self.handle, idbuf, rank, world))
        self.rank, self.world = rank, world

    def init_comm_virtual(self, vcomm, rank, world):
        """join a VirtualComm (world contexts of one process on one device, see include/sslcr.h): test infrastructure that runs
        the engine's sharded code paths on a single-GPU box."""
        L.check(L.lib().sslcr_comm_init_virtual(self.handle, vcomm.handle, rank))
        self.rank, self.world = rank, world
        self._vcomm = vcomm                                        # keep it alive as long as this engine

    def comm_info(self):
        """(rank, world, transport) as the communicator itself reports them; transport: 'none' | 'rccl' | 'virtual'."""
        r, w, t = C.c_int(), C.c_int(), C.c_int()
        L.check(L.lib().sslcr_comm_info(self.handle, C.byref(r), C.byref(w), C.byref(t)))
        return r.value, w.value, ("none", "rccl", "virtual")[t.value]

    def set_bn_sync(self, on):
        """True (default): train-mode BatchNorm uses global-batch statistics across ranks; False: per-replica statistics
        like the reference's nn.DataParallel (eval_BreastPathQ_SSL_CR.py:474-477)."""
        L.check(L.lib().sslcr_set_bn_sync(self.handle, int(bool(on))))

    def set_aux_stream(self, on):
        """True: step_ssl_cr runs the teacher forward on a second stream next to the student forward (-2 % step time; per-kernel
        timings then include the sharing of the CUs).  Default off."""
        L.check(L.lib().sslcr_set_aux_stream(self.handle, int(bool(on))))

    def set_wgrad_stream(self, on):
        """True: backward's weight-gradient launches run on a second stream (bit-identical results; measured neutral on MI355X,
        off by default -- see include/sslcr.h)."""
        L.check(L.lib().sslcr_set_wgrad_stream(self.handle, int(bool(on))))

    def all_reduce_sum(self, t):
        """in-place SUM of a contiguous fp32 device tensor over the ranks of the engine's own communicator (RCCL or virtual), on
        the current stream; identity on one rank.  Logging path only (steps._Meters at print_freq / epoch end): the data-path
        collectives -- gradient buckets, BatchNorm sums -- are issued inside the step by the engine itself."""
        if self.world > 1:
            if t.dtype != torch.float32 or not t.is_contiguous() or t.device != self.device:
                raise L.SslcrError("all_reduce_sum: contiguous fp32 tensor on the engine's device expected")
            L.check(L.lib().sslcr_comm_all_reduce_f32(self.handle, L.ptr(t), t.numel(), L.stream_ptr()))
        return t

    def copy_stream(self):
        """side stream for host-to-device prefetch of the next batch (steps._ahead); torch owns streams, the engine only keeps one"""
        if getattr(self, "_copy_stream", None) is None:
            self._copy_stream = torch.cuda.Stream(self.device)
        return self._copy_stream

    # ------------------------------------------------------------------ measurement
    def profile(self, enable):
        L.check(L.lib().sslcr_profile(self.handle, int(enable)))

    def profile_read(self, which):
        """{launches, ms, flops, bytes} of the event-bracketed conv launches (0 conv_igemm fwd+dgrad, 1 wgrad)."""
        out = (C.c_double * 4)()
        L.check(L.lib().sslcr_profile_read(self.handle, which, out))
        return dict(launches=int(out[0]), ms=out[1], flops=out[2], bytes=out[3])

    def profile_table(self):
        """per kernel instance: [dict(name, launches, ms, flops, bytes)], sorted by total time."""
        buf = C.create_string_buffer(1 << 16)
        L.check(L.lib().sslcr_profile_dump(self.handle, buf, len(buf)))
        rows = []
        for line in buf.value.decode().splitlines():
            name, n, ms, fl, by = line.rsplit("|", 4)
            rows.append(dict(name=name, launches=int(float(n)), ms=float(ms), flops=float(fl), bytes=float(by)))
        return sorted(rows, key=lambda r: -r["ms"])

    # ------------------------------------------------------------------ binding
    def as_input(self, x):
        if x.dtype not in (torch.uint8, torch.float32):
            x = x.float()
        if x.device != self.device:
            x = x.to(self.device, non_blocking=True)
        return x.contiguous()

    def bind(self, model, classifier):
        model = unwrap(model)
        classifier = unwrap(classifier) if classifier is not None else self._dummy(model)
        key = (id(model), id(classifier))
        b = self._bound.get(key)
        if b is not None and (b.model is not model or b.classifier is not classifier or not b.still_valid()):
            b = None
        if b is None:
            b = BoundNet(self, model, classifier)
            self._bound[key] = b
            # drop bindings whose modules were garbage collected / replaced (teacher = deepcopy(student) every epoch)
            for k in [k for k, v in self._bound.items() if v is not b and not v.still_valid()]:
                del self._bound[k]
        return b

    def _dummy(self, model):
        if self._dummy_cls is None:
            self._dummy_cls = FinetuneResNet(1).to(self.device)
        return self._dummy_cls

    # ------------------------------------------------------------------ fused steps
    def step_ssl_cr(self, teacher, student, kind, x, y, u_w, u_s, lambda_u, backward=True, nx_global=None, nu_global=None,
                    accumulate=False, loss_options=None, denominator=None):
        """one consistency-training iteration (eval_BreastPathQ_SSL_CR.py:65-100 / eval_Camelyon_SSL_CR.py:94-121).
        x [nx,3,H,W], u_w/u_s [nu,3,H,W] uint8|fp32; y [nx] fp32 (kind 'mse') or int64 (kind 'ce').
        -> dict(losses [4] device tensor: loss, loss_x, loss_u, #correct ; feats ; logits ; logits_t).  With more than one rank the
        losses are this rank's share (scaled by 1/global-count; the SUM over ranks is the global value) -- no collective per step.
        accumulate: the student's gradients are ADDED to what its buffer holds (``BoundNet.set_grad_accumulate``, set on every call:
        the default clears first).  A micro-batch is a shard in time: pass the full batch's counts as nx_global / nu_global, then
        the sums of k micro-steps' gradients and losses are the global batch's -- with each micro-batch's own BatchNorm statistics
        (per-replica statistics under ``nn.DataParallel``), running statistics updated by every micro-step in turn (``DataParallel``
        keeps replica 0's), and no clearing of a gradient left from before an optimizer step.
        loss_options: a ``LossOptions`` for kind 'ce' (set on every call, as accumulate is: None or the defaults give the step it
        has always been); the result then also has ``stats`` = device [#confident unlabeled rows, sum of the teacher's max-probs].
        denominator: the supervised term's divisor over the whole global batch (``kernels.ce_denominator`` of the full batch's
        targets, all-reduced over ranks) -- needed whenever this call holds only a micro-batch or a shard of the batch (rows labelled -100
        are left out once an option is set, so no part knows the batch's divisor from its own rows); None: the rows of this call."""
        stats = self._set_loss_options(student, kind, loss_options, denominator)
        student.set_grad_accumulate(accumulate)
        teacher.sync()
        student.sync()
        x, u_w, u_s = self.as_input(x), self.as_input(u_w), self.as_input(u_s)
        if x.dtype != u_s.dtype or x.dtype != u_w.dtype:
            x, u_w, u_s = x.float(), u_w.float(), u_s.float()
        # torch.cat((inputs_x, inputs_u_s)) of :82 is not materialised: the stem kernel reads the two segments in place
        nx, nu = x.shape[0], u_w.shape[0]
        if u_s.shape[0] != nu or x.shape[1:] != u_s.shape[1:]:
            raise ValueError("step_ssl_cr: u_w / u_s batch sizes or image shapes differ")
        _, _, H, W = x.shape
        dev = self.device
        feats = torch.empty((nx + nu, 768), dtype=torch.float32, device=dev)
        logits = torch.empty((nx + nu, student.ncls), dtype=torch.float32, device=dev)
        logits_t = torch.empty((nu, student.ncls), dtype=torch.float32, device=dev)
        losses = torch.empty(4, dtype=torch.float32, device=dev)
        k = {"mse": 0, "ce": 1}[kind]
        y = y.to(dev).contiguous()
        tf = y.float() if k == 0 else None
        ti = y.long() if k == 1 else None
        d = SslCrDesc(k, x.data_ptr(), u_w.data_ptr(), int(x.dtype == torch.float32), nx, nu, H, W,
                      None if tf is None else tf.data_ptr(), None if ti is None else ti.data_ptr(), float(lambda_u),
                      int(nx_global or nx * self.world), int(nu_global or nu * self.world), feats.data_ptr(),
                      logits.data_ptr(), logits_t.data_ptr(), losses.data_ptr(), int(backward), u_s.data_ptr())
        L.check(L.lib().sslcr_step_ssl_cr(teacher.handle, student.handle, C.byref(d), L.stream_ptr()))
        student._live_inputs = (x, u_s, u_w, tf, ti)
        student._note_buffers_changed()
        out = dict(losses=losses, feats=feats, logits=logits, logits_t=logits_t)
        if stats is not None:
            out["stats"] = stats
        return out

    def _set_loss_options(self, net, kind, loss_options, denominator):
        """the per-call reset of the net's sticky loss options; -> the stats tensor of a call with options (None without)"""
        if loss_options is not None and not isinstance(loss_options, LossOptions):
            raise TypeError(f"loss_options must be a LossOptions or None (got {type(loss_options).__name__})")
        if loss_options is None or loss_options.is_default():
            if denominator is not None:
                raise ValueError("a denominator without loss options that need one")
            net.set_loss_options(None)
            return None
        if kind != "ce":
            raise ValueError(f"loss_options apply to the cross-entropy steps only (kind {kind!r})")
        stats = torch.empty(2, dtype=torch.float32, device=self.device)          # the loss kernel writes both entries
        net.set_loss_options(loss_options, denominator, stats)
        return stats

    def step_supervised(self, net, kind, xs, y, train=True, backward=True, n_global=None, accumulate=False, loss_options=None,
                        denominator=None):
        """student-only step: RSP pretraining (TripletNet, 3 inputs, 'ce'; pretrain_BreastPathQ.py:42-61), supervised
        fine-tuning (eval_Camelyon_SSL.py:52-98 'ce', eval_BreastPathQ_SSL.py:52-84 'mse') and every validate().
        accumulate: as in ``step_ssl_cr`` (gradients added to the buffer; n_global = the full batch's count; per-micro-batch
        BatchNorm statistics, running statistics updated every micro-step, stale gradients are not cleared).
        loss_options / denominator: as in ``step_ssl_cr`` (kind 'ce'; with train=False the weighted validation loss)."""
        stats = self._set_loss_options(net, kind, loss_options, denominator)
        net.set_grad_accumulate(accumulate)
        net.sync()
        xs = [self.as_input(x) for x in xs]
        n, _, H, W = xs[0].shape
        dev = self.device
        feats = torch.empty((n, 768), dtype=torch.float32, device=dev)
        logits = torch.empty((n, net.ncls), dtype=torch.float32, device=dev)
        losses = torch.empty(4, dtype=torch.float32, device=dev)
        k = {"ce": 2, "mse": 3}[kind]
        y = y.to(dev).contiguous()
        tf = y.float() if k == 3 else None
        ti = y.long() if k == 2 else None
        p = [x.data_ptr() for x in xs] + [None] * (3 - len(xs))
        d = SupDesc(k, p[0], p[1], p[2], int(xs[0].dtype == torch.float32), n, H, W, None if tf is None else tf.data_ptr(),
                    None if ti is None else ti.data_ptr(), int(n_global or n * self.world), feats.data_ptr(),
                    logits.data_ptr(), losses.data_ptr(), int(train), int(backward and train))
        L.check(L.lib().sslcr_step_supervised(net.handle, C.byref(d), L.stream_ptr()))
        net._live_inputs = (xs, tf, ti)
        if train:
            net._note_buffers_changed()
        out = dict(losses=losses, feats=feats, logits=logits)
        if stats is not None:
            out["stats"] = stats
        return out


class VirtualComm:
    """shared exchange object of `world` virtual ranks (see include/sslcr.h: sslcr_vcomm)."""

    def __init__(self, world):
        lib = L.lib()
        for name in ("sslcr_vcomm_create", "sslcr_vcomm_destroy", "sslcr_comm_init_virtual"):
            fn = getattr(lib, name)
            fn.restype, fn.argtypes = _ENGINE_SIGS[name]
        h = C.c_void_p()
        L.check(lib.sslcr_vcomm_create(C.byref(h), world))
        self.handle, self.world = h, world

    def close(self):
        if self.handle:
            L.lib().sslcr_vcomm_destroy(self.handle)
            self.handle = None


_engines = {}


def get_engine(device=None, dtype=None):
    """process-wide engine for `device` (created on first use; dtype from SSLCR_DTYPE, default bf16)."""
    dev = torch.device(device if device is not None else "cuda")
    idx = dev.index if dev.index is not None else torch.cuda.current_device()
    e = _engines.get(idx)
    if e is None:
        e = Engine(torch.device("cuda", idx), dtype)
        _engines[idx] = e
    elif dtype is not None and _DTYPES[dtype] != e.dtype:
        raise L.SslcrError("an engine with a different dtype already exists on this device; use set_engine()")
    return e


def set_engine(engine):
    _engines[engine.device.index] = engine
    return engine
