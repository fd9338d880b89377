"""The tail of a detector training step on the GPU: drop-ins for the two calls that follow
``loss.backward()`` in OpenPCDet's ``train_one_epoch`` --

    clip_grad_norm_(model.parameters(), optim_cfg.GRAD_NORM_CLIP)
    optimizer.step()          # OptimWrapper.step -> torch.optim.Adam.step

``clip_grad_norm_`` has torch's signature and returns ``total_norm`` as a new 0-dim float32 device tensor; two launches whatever
the number of tensors.  It hands the call to torch's own function for host tensors, ``norm_type != 2``,
``error_if_nonfinite=True``, gradients that are not dense contiguous float32, tensors on several devices and a call without any
gradient.  ``total_norm`` is (float) sqrt of a float64 sum of exact squares: it stays finite where torch's float32 sum of
per-tensor norms overflows (gradients of 1e25), and it differs from torch's value by the rounding of torch's own sums.

``step(self)`` replaces ``OptimWrapper.step`` for the ``adam_onecycle`` wrapper: the decoupled decay ``p *= 1 - wd lr`` of every
tensor that requires grad (the BN groups only with ``bn_wd``), ``weight_decay`` of the groups set to 0 as the reference does, and
Adam's update of every tensor that has a gradient, in ONE launch.  The state stays the inner ``torch.optim.Adam``'s own, in
torch's format (``step`` a 0-dim float32 host tensor, ``exp_avg``, ``exp_avg_sq``), so ``state_dict()``, checkpoints,
``load_state_dict``, ``clear()`` and a switch back to torch's ``step`` keep working.  A tensor without a gradient gets no state
and its ``step`` does not advance: the bias corrections are per tensor.  The method that was replaced runs when the wrapper's
``opt`` is not exactly ``torch.optim.Adam``, when ``true_wd`` is false, when the wrapper is a ``FastAIMixedOptim``, and for
parameters on the host.  ``amsgrad``, ``maximize``, ``capturable``, ``differentiable``, ``fused=True`` and parameters, gradients
or state that are not contiguous float32 raise ``NotImplementedError``; parameters on more than one device raise ``ValueError``
-- before anything is launched or changed.

``clip_and_step(self, max_norm)`` is the fused path for a caller's own loop: the norm kernel, then the step on ``fl(g * coef)``
-- two launches.  THE ONE VISIBLE DIFFERENCE: ``.grad`` is left unscaled.  The norm sums its chunk partials in the order of the
gradient tensors: ``clip_and_step`` takes them in the wrapper's group order (the BatchNorm tensors last), so it gives the bits
of the two calls above -- in the parameters, the state and the returned norm -- only where ``clip_grad_norm_`` was given the
tensors in that same order; after ``clip_grad_norm_(model.parameters(), ...)`` the last bit of the norm can differ.

A call that the library refuses after the checks here (nothing was launched) puts the step counts, the states it created and
the groups' ``weight_decay`` back before it raises.  ``FINISH_LAUNCH`` chooses how the consumer of the norm gets the
coefficient: False, every workgroup sums the chunk partials itself; True, one workgroup does in a launch of its own.

Every call runs on PyTorch's current stream and only enqueues; the tables of a step go up through the context's ring of pinned
slots, so the host waits for the device only when it has run a whole ring of calls ahead.  One wrapper is to be driven from one
stream at a time.
"""
import numpy as np
import torch
from torch.nn.utils import clip_grad_norm_ as torch_clip_grad_norm_

from .. import ops

METHODS = ("step", "clip_and_step")
NAME = "clip_grad_norm_"               # the name set in train_utils.train_utils
REFUSED_OPTIONS = ("amsgrad", "maximize", "capturable", "differentiable")
_ORIGINAL = {}                         # class or module -> what bind() replaced on it
_CLIP = {}                             # device -> _Tables of clip_grad_norm_
_F = np.float32
MAX_TENSORS = 1 << 20               # the library's limit, refused here before the state is touched
FINISH_LAUNCH = False                # sum the chunk partials in a launch of their own instead of in every workgroup of the consumer


def host_scalars(lr, beta1, beta2, eps, t, dec=1.0):
    """the per-tensor scalars of a step, computed in Python doubles and rounded to float32 once
    -> (dec, w, omw, b2, omb2, bc2s, eps, nss) as float32 and the flags; omw = fl(1 - w) is a float32 operation, as in lerp"""
    w = _F(1 - beta1)
    return (_F(dec), w, _F(1) - w, _F(beta2), _F(1 - beta2), _F((1 - beta2 ** t) ** 0.5), _F(eps),
            _F(-(lr / (1 - beta1 ** t)))), (ops.OPTIM_LERP_HIGH if w >= _F(0.5) else 0)


class _Tables:
    """the host tables of one parameter set, the workspace on its device and what that workspace holds"""

    def __init__(self):
        self.key = None          # what the static table was built from
        self.static = None
        self.workspace = None
        self.uploaded = False

    def build(self, dev, ptrs_p, ptrs_m, ptrs_v, sizes):
        """-> (static table, upload it?) for the tensors given by their addresses and sizes (none without elements)"""
        key = (dev, tuple(ptrs_p), tuple(ptrs_m), tuple(ptrs_v), tuple(sizes))
        if key != self.key:
            n = np.asarray(sizes, dtype=np.int64)
            chunks = -(-n // ops.optim_chunk())
            st = np.zeros(len(sizes), dtype=ops.OPTIM_STATIC)
            st["p"], st["m"], st["v"], st["n"] = ptrs_p, ptrs_m, ptrs_v, n
            st["first_chunk"] = np.cumsum(chunks) - chunks
            need = ops.optim_workspace_bytes(len(sizes), int(chunks.sum()))
            if self.workspace is None or self.workspace.device != dev or self.workspace.numel() < need:
                self.workspace = torch.empty((need,), dtype=torch.uint8, device=dev)
            self.key, self.static, self.uploaded = key, st, False
        return self.static

    def step_table(self, ptrs_g, rows=None, scalars=None, flags=None):
        """-> the step table: the gradients' addresses (0: none) and, per tensor, row `rows[i]` of `scalars` / `flags`"""
        sp = np.zeros(len(ptrs_g), dtype=ops.OPTIM_STEP)
        sp["g"] = ptrs_g
        has = sp["g"] != 0
        chunks = -(-self.static["n"] // ops.optim_chunk()) * has
        sp["norm_first"] = np.where(has, np.cumsum(chunks) - chunks, -1)
        if rows is not None:
            for k, name in enumerate(("dec", "w", "omw", "b2", "omb2", "bc2s", "eps", "nss")):
                sp[name] = scalars[rows, k]
            sp["flags"] = flags[rows]
        return sp


def _dense(t):
    return t.dtype == torch.float32 and t.layout == torch.strided and t.is_contiguous()


# ------------------------------------------------------------------------------------------------------------ clip_grad_norm_
def clip_grad_norm_(parameters, max_norm, norm_type=2.0, error_if_nonfinite=False, foreach=None):
    """torch.nn.utils.clip_grad_norm_ in two launches (module docstring) -> total_norm, a new 0-dim float32 device tensor"""
    parameters = [parameters] if torch.is_tensor(parameters) else list(parameters)   # a generator is consumed once
    grads = [p.grad for p in parameters if p.grad is not None]
    dev = grads[0].device if grads else None
    if (not grads or float(norm_type) != 2.0 or error_if_nonfinite
            or not all(g.is_cuda and g.device == dev and _dense(g) for g in grads)):
        return torch_clip_grad_norm_(parameters, max_norm, norm_type=norm_type, error_if_nonfinite=error_if_nonfinite, foreach=foreach)
    max_norm = float(max_norm)
    grads = [g for g in grads if g.numel()]
    if not grads:
        return torch.zeros((), dtype=torch.float32, device=dev)
    tab = _CLIP.setdefault(dev, _Tables())
    zeros = [0] * len(grads)
    static = tab.build(dev, zeros, zeros, zeros, [g.numel() for g in grads])
    step = tab.step_table([g.data_ptr() for g in grads])
    norm = torch.empty((), dtype=torch.float32, device=dev)
    ops.optim_clip(static, step, max_norm, tab.workspace, norm, upload_static=not tab.uploaded, finish_launch=FINISH_LAUNCH)
    tab.uploaded = True
    return norm


# ------------------------------------------------------------------------------------------------------------ OptimWrapper
def _replaced(self, name):
    for c in type(self).__mro__:
        original = _ORIGINAL.get(c, {}).get(name)
        if original is not None:
            return original
    raise NotImplementedError(f"{type(self).__name__}.{name}: modest_amd.utils.optim_step.bind() replaced no method of that name")


def _is_ours(self):
    """the wrapper build_optimizer makes for adam_onecycle: exactly torch.optim.Adam inside, true weight decay, not mixed"""
    return (type(self.__dict__.get("opt")) is torch.optim.Adam and bool(self.true_wd)
            and not any(c.__name__ == "FastAIMixedOptim" for c in type(self).__mro__))


def _rows(self):
    """-> [(parameter, group, decay factor in Python doubles)] of every tensor the reference's step touches, in the groups'
    order: a tensor that requires grad is decayed (the BN groups only with bn_wd), one with a gradient is updated"""
    groups = self.opt.param_groups
    rows = []
    for lr, wd, pg1, pg2 in zip(self._lr, self._wd, groups[::2], groups[1::2]):
        for pg, decays in ((pg1, True), (pg2, bool(self.bn_wd))):
            for p in pg["params"]:
                live = p.requires_grad is not False
                if not live and p.grad is None:
                    continue
                rows.append((p, pg, 1 - wd * lr if live and decays else 1.0))
    return rows


def _check(self, rows):
    """every refusal, before anything is launched or changed -> the device, or None for parameters on the host (which the method
    that was replaced takes, whatever their options)"""
    devs = {p.device for p, _, _ in rows}
    if len(devs) > 1:
        raise ValueError(f"the parameters are on more than one device: {sorted(str(d) for d in devs)}")
    dev = next(iter(devs)) if devs else None
    if dev is None or dev.type != "cuda":
        return None
    for pg in self.opt.param_groups:
        for name in REFUSED_OPTIONS:
            if pg.get(name):
                raise NotImplementedError(f"torch.optim.Adam({name}=True) is not provided by modest_amd.utils.optim_step")
        if pg.get("fused"):
            raise NotImplementedError("torch.optim.Adam(fused=True) is not provided by modest_amd.utils.optim_step")
    state = self.opt.state
    for p, _, _ in rows:
        tensors = [("parameters", p)] + ([("gradients", p.grad)] if p.grad is not None else [])
        tensors += [(f"state {k}", state[p][k]) for k in ("exp_avg", "exp_avg_sq") if p in state and k in state[p]]
        for what, t in tensors:
            if not _dense(t) or t.shape != p.shape or t.device != p.device:
                raise NotImplementedError(f"{what} that are not contiguous float32 ({tuple(t.shape)} {t.dtype}, strides {t.stride()}, "
                                          f"{t.device}) are not provided by modest_amd.utils.optim_step")
    if sum(1 for p, _, _ in rows if p.numel()) > MAX_TENSORS:
        raise ValueError(f"more than {MAX_TENSORS} tensors")
    return dev


def _plan(self, rows):
    """The host's part of a step, in torch's own state format: creates the state of a tensor at its first gradient, advances the
    step counts of the tensors with a gradient, sets the groups' weight_decay to 0 as the reference does
    -> (tensors of the table, their gradients or None, row index into scalars, scalars (k, 8) float32, flags (k,) uint32, undo);
    undo() puts the step counts, the states created here and the groups' weight_decay back: for a call that then fails"""
    state = self.opt.state
    steps, live, created = [], [], []
    decay_before = [pg.get("weight_decay") for pg in self.opt.param_groups]
    for p, pg, dec in rows:
        if p.grad is None:
            continue
        st = state[p]
        if len(st) == 0:
            st["step"] = torch.tensor(0.0, dtype=torch.float32)
            st["exp_avg"] = torch.zeros_like(p, memory_format=torch.preserve_format)
            st["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.preserve_format)
            created.append(p)
        elif not torch.is_tensor(st["step"]):
            st["step"] = torch.tensor(float(st["step"]), dtype=torch.float32)
        steps.append(st["step"])
        live.append(p)
    if steps:
        if all(s.device.type == "cpu" and s.dtype == torch.float32 and s.ndim == 0 for s in steps):
            torch._foreach_add_(steps, 1.0)
            counts = torch.stack(steps).tolist()
        else:
            counts = [float(s.add_(1)) for s in steps]
    count_of = dict(zip(map(id, live), counts)) if steps else {}
    uniq, index, scalars, flags = {}, [], [], []
    for p, pg, dec in rows:
        if not p.numel():
            continue
        t = count_of.get(id(p))
        beta1, beta2 = pg["betas"]
        key = (id(pg), t, dec)
        if key not in uniq:
            uniq[key] = len(scalars)
            if t is None:       # decay alone
                scalars.append((_F(dec),) + (_F(0),) * 7)
                flags.append(0)
            else:
                s, f = host_scalars(pg["lr"], beta1, beta2, pg["eps"], t, dec)
                scalars.append(s)
                flags.append(f)
        index.append(uniq[key])
    self.set_val("weight_decay", [0] * len(self._wd))
    tensors = [p for p, _, _ in rows if p.numel()]

    def undo():
        for s in steps:
            s.sub_(1)
        for p in created:
            del state[p]
        for pg, wd in zip(self.opt.param_groups, decay_before):
            pg["weight_decay"] = wd

    return (tensors, [p.grad for p in tensors], np.asarray(index, dtype=np.int64),
            np.asarray(scalars, dtype=np.float32).reshape(-1, 8), np.asarray(flags, dtype=np.uint32), undo)


def _run(self, max_norm):
    rows = _rows(self)
    dev = _check(self, rows)
    if dev is None:
        return None if not rows else NotImplemented
    tensors, grads, index, scalars, flags, undo = _plan(self, rows)
    if not tensors:
        return torch.zeros((), dtype=torch.float32, device=dev) if max_norm is not None else None
    try:
        return _launch(self, dev, tensors, grads, index, scalars, flags, max_norm)
    except BaseException:
        undo()          # nothing was launched: the optimiser is as it was before the call
        raise


def _launch(self, dev, tensors, grads, index, scalars, flags, max_norm):
    tab = self.__dict__.get("_modest_optim_tables")
    if tab is None:
        tab = self.__dict__["_modest_optim_tables"] = _Tables()
    state = self.opt.state
    has = [g is not None for g in grads]
    static = tab.build(dev, [p.data_ptr() for p in tensors],
                       [state[p]["exp_avg"].data_ptr() if h else 0 for p, h in zip(tensors, has)],
                       [state[p]["exp_avg_sq"].data_ptr() if h else 0 for p, h in zip(tensors, has)],
                       [p.numel() for p in tensors])
    step = tab.step_table([g.data_ptr() if g is not None else 0 for g in grads], index, scalars, flags)
    norm = None
    if max_norm is None:
        ops.optim_step(static, step, tab.workspace, upload_static=not tab.uploaded)
    else:
        norm = torch.empty((), dtype=torch.float32, device=dev)
        ops.optim_norm_step(static, step, max_norm, tab.workspace, norm, upload_static=not tab.uploaded, finish_launch=FINISH_LAUNCH)
    tab.uploaded = True
    return norm


def step(self) -> None:
    """OptimWrapper.step in one launch (module docstring)"""
    if not _is_ours(self) or _run(self, None) is NotImplemented:
        return _replaced(self, "step")(self)
    return None


def clip_and_step(self, max_norm):
    """clip_grad_norm_ over the wrapper's tensors and step() in two launches -> total_norm; .grad is left unscaled (module
    docstring).  A wrapper that step() hands to the method it replaced gets the two calls themselves, which scale .grad."""
    max_norm = float(max_norm)
    if _is_ours(self):
        norm = _run(self, max_norm)
        if norm is not NotImplemented:
            if norm is None:    # no tensor at all
                return torch.tensor(0.0)
            return norm
    norm = clip_grad_norm_([p for pg in self.opt.param_groups for p in pg["params"]], max_norm)
    self.step()
    return norm


KINDS = {"step": step, "clip_and_step": clip_and_step}


def bind(cls, module=None):
    """set step and clip_and_step on the wrapper class `cls` and, with `module` (train_utils.train_utils), the name
    clip_grad_norm_ in it -> cls.  What they replaced is kept in _ORIGINAL.  Idempotent."""
    if cls.__dict__.get("step") is not step:
        _ORIGINAL[cls] = {name: cls.__dict__.get(name) for name in METHODS}
        for name in METHODS:
            setattr(cls, name, KINDS[name])
    if module is not None and module.__dict__.get(NAME) is not clip_grad_norm_:
        _ORIGINAL[module] = {NAME: module.__dict__.get(NAME)}
        setattr(module, NAME, clip_grad_norm_)
    return cls


def unbind(cls, module=None):
    """put back what bind() replaced on cls and in module -> cls"""
    for target in (cls, module):
        if target is None or target not in _ORIGINAL:
            continue
        for name, original in _ORIGINAL.pop(target).items():
            if original is None:
                if name in target.__dict__:
                    delattr(target, name)
            else:
                setattr(target, name, original)
    return cls
