"""The fused optimizer step (include/lgoptim.h, csrc/lg_optim.hip): what every learner of the reference runs behind loss.backward()
(rsl_rl/algorithms/ppo.py:135-138: clip_grad_norm_ and torch.optim.Adam.step) together with the adaptive learning-rate rule in front of
it (ppo.py:193-206), as one call of two launches that reads nothing back:

    opt = FusedAdam(actor_critic.parameters(), lr=1e-3, betas=(0.9, 0.999), eps=1e-8, max_grad_norm=1.0, desired_kl=0.01)
    opt.zero_grad()
    out = loss_fn(...); out.loss.backward()
    info = opt.step(kl_mean=out.kl_mean)        # the KL stays on the device: no .item()

The learning rate and the step count live in a two-double cell on the device, so the call can be captured in a HIP graph and replayed.
`info.grad_norm`, `info.clip_coef`, `info.lr` and `info.step` are detached 0-dim views of the result vector: nothing synchronises until
the caller reads one, and the next step overwrites them.  Gradients are not scaled in place (the clipped gradient exists in registers
only).  `state_dict()` / `load_state_dict()` speak torch.optim.Adam's format, so a checkpoint written by either optimizer loads into the
other.  Weight decay, AMSGrad and maximize are out of scope.  There is no CPU path: the parameters live on a HIP device."""
from __future__ import annotations

import ctypes as C

import torch

from . import abi


def _describe(t):
    return f"{tuple(t.shape)} {t.dtype} on {t.device}, strides {tuple(t.stride())}" if isinstance(t, torch.Tensor) else type(t).__name__


def _check_array(t, what, numel, device):
    """A contiguous float32 array of `numel` elements on `device`: its address."""
    if not isinstance(t, torch.Tensor) or t.dtype != torch.float32:
        raise ValueError(f"FusedAdam: {what} must be float32; got {_describe(t)}")
    if not t.is_contiguous():
        raise ValueError(f"FusedAdam: {what} must be contiguous; got {_describe(t)}")
    if t.device != device:
        raise ValueError(f"FusedAdam: {what} must be on {device}; got {_describe(t)}")
    if t.numel() != numel:
        raise ValueError(f"FusedAdam: {what} must have {numel} elements; got {_describe(t)}")
    return t.data_ptr()


def check_parameters(params, names=None):
    """The parameter list of a FusedAdam: float32, contiguous, at least one element, all on one HIP device, at most ADAM_MAX_TENSORS of
    them.  Refusals are ValueErrors that name the parameter; the library is not touched.  Returns (tensors, names, device)."""
    params = list(params)
    if params and isinstance(params[0], (tuple, list)):                      # named_parameters()
        names, params = [str(n) for n, _ in params], [p for _, p in params]
    names = list(names) if names is not None else [f"params[{i}]" for i in range(len(params))]
    if not params:
        raise ValueError("FusedAdam: no parameters")
    if len(names) != len(params):
        raise ValueError(f"FusedAdam: {len(names)} names for {len(params)} parameters")
    device = None
    for name, p in zip(names, params):                # what is wrong with a tensor itself first, where it lives after that
        if not isinstance(p, torch.Tensor) or p.dtype != torch.float32:
            raise ValueError(f"FusedAdam: {name} must be float32; got {_describe(p)}")
        if not p.is_contiguous():
            raise ValueError(f"FusedAdam: {name} must be contiguous; got {_describe(p)}")
        if p.numel() < 1:
            raise ValueError(f"FusedAdam: {name} has no elements")
    for name, p in zip(names, params):
        if p.device.type != "cuda":
            raise ValueError(f"FusedAdam: {name} is on {p.device}, not on a HIP device; there is no CPU path")
        if device is not None and p.device != device:
            raise ValueError(f"FusedAdam: {name} is on {p.device}, the parameters before it on {device}")
        device = p.device
    if len(params) > abi.ADAM_MAX_TENSORS:
        raise ValueError(f"FusedAdam: {len(params)} parameter tensors; the kernel takes 1 .. {abi.ADAM_MAX_TENSORS} (the descriptor travels "
                         f"in the kernel-argument block)")
    return params, names, device


def adam_args(params, names, exp_avg, exp_avg_sq, state, partials, result, kl_mean, betas, eps, max_grad_norm, desired_kl, device, args=None):
    """LgAdamArgs for the parameters that have a gradient right now (a parameter whose .grad is None is left out).  Refusals are
    ValueErrors that name the parameter; the library is not touched.  Returns (descriptor, live indices); with no live parameter the
    descriptor has n_tensors = 0 and is not for launching.  `args` is a descriptor to refill instead of a fresh one."""
    if kl_mean is not None and desired_kl is None:
        raise ValueError("FusedAdam: kl_mean was given, but the optimizer has no desired_kl: the adaptive rule needs both")
    if kl_mean is not None and (not isinstance(kl_mean, torch.Tensor) or kl_mean.dtype != torch.float32 or kl_mean.numel() != 1
                                or kl_mean.device != device):
        raise ValueError(f"FusedAdam: kl_mean must be a 0-dim float32 tensor on {device}; got {_describe(kl_mean)}")
    a = args if args is not None else abi.LgAdamArgs()
    live = []
    for i, (name, p) in enumerate(zip(names, params)):
        g = p.grad
        if g is None:
            continue
        if len(live) >= abi.ADAM_MAX_TENSORS:
            raise ValueError(f"FusedAdam: more than {abi.ADAM_MAX_TENSORS} parameter tensors")
        n = p.numel()
        if not isinstance(g, torch.Tensor) or g.dtype != torch.float32 or g.layout != torch.strided:
            raise ValueError(f"FusedAdam: {name}.grad must be a dense float32 tensor; got {_describe(g)}"
                             + ("" if not isinstance(g, torch.Tensor) else f", layout {g.layout}"))
        T = a.tensor[len(live)]
        T.grad = _check_array(g, name + ".grad", n, device)
        T.param = _check_array(p, name, n, device)
        T.exp_avg = _check_array(exp_avg[i], name + "'s exp_avg", n, device)
        T.exp_avg_sq = _check_array(exp_avg_sq[i], name + "'s exp_avg_sq", n, device)
        T.numel = n
        live.append(i)
    a.n_tensors = len(live)
    a.flags = (abi.ADAM_CLIP if max_grad_norm is not None else 0) | (abi.ADAM_KL_RULE if kl_mean is not None else 0)
    a.beta1, a.beta2, a.eps = float(betas[0]), float(betas[1]), float(eps)
    a.max_grad_norm = float(max_grad_norm) if max_grad_norm is not None else 0.0
    a.desired_kl = float(desired_kl) if kl_mean is not None else 0.0
    a.kl = kl_mean.data_ptr() if kl_mean is not None else None
    for what, t, dtype, n in (("state", state, torch.float64, abi.ADAM_STATE_DOUBLES), ("partials", partials, torch.float64, 1),
                              ("result", result, torch.float32, abi.ADAM_RESULT_FLOATS)):
        if not isinstance(t, torch.Tensor) or t.dtype != dtype or not t.is_contiguous() or t.device != device or t.numel() < n:
            raise ValueError(f"FusedAdam: {what} must be a contiguous {str(dtype).replace('torch.', '')} tensor of at least {n} elements on "
                             f"{device}; got {_describe(t)}")
    a.state, a.partials, a.partials_capacity, a.result = state.data_ptr(), partials.data_ptr(), partials.numel(), result.data_ptr()
    return a, live


_WORKSPACE = {}      # numels -> doubles: the plan is a pure function of them


def workspace_doubles(numels):
    """Doubles the partials slab needs (lg_adam_workspace): the plan alone, nothing is launched."""
    key = tuple(int(n) for n in numels)
    if key in _WORKSPACE:
        return _WORKSPACE[key]
    lib = abi.load_lib()
    a = abi.LgAdamArgs()
    a.n_tensors = len(key)
    for i, n in enumerate(key[:abi.ADAM_MAX_TENSORS]):
        a.tensor[i].numel = n
    w = lib.lg_adam_workspace(C.byref(a))
    if w == 0:
        abi.check(1, lib)
    _WORKSPACE[key] = w
    return w


def launch(args, device):
    """lg_adam_step on the current stream of `device`."""
    lib = abi.load_lib()
    abi.check(lib.lg_adam_step(C.byref(args), torch.cuda.current_stream(device).cuda_stream), lib)


class AdamStepInfo:
    """Detached 0-dim views of the result vector (`result`); the next step overwrites them."""

    def __init__(self, result):
        self.result = result
        self.grad_norm, self.clip_coef = result[abi.ADAM_R_GRAD_NORM], result[abi.ADAM_R_CLIP_COEF]
        self.lr, self.step = result[abi.ADAM_R_LR], result[abi.ADAM_R_STEP]


def _validate_hyper(lr, betas, eps, max_grad_norm, desired_kl):
    if not lr >= 0.0:
        raise ValueError(f"FusedAdam: lr = {lr}; it must be at least 0")
    if len(betas) != 2 or not all(0.0 <= b < 1.0 for b in betas):
        raise ValueError(f"FusedAdam: betas = {tuple(betas)}; each must lie in [0, 1)")
    if not eps >= 0.0:
        raise ValueError(f"FusedAdam: eps = {eps}; it must be at least 0")
    if max_grad_norm is not None and not max_grad_norm > 0.0:
        raise ValueError(f"FusedAdam: max_grad_norm = {max_grad_norm}; it must be above 0 (None: no clip)")
    if desired_kl is not None and not desired_kl > 0.0:
        raise ValueError(f"FusedAdam: desired_kl = {desired_kl}; it must be above 0 (None: no adaptive rate)")


# what torch.optim.Adam keeps in a parameter group besides lr, betas, eps and params: written out so that its load_state_dict, which
# replaces the group by the saved one, finds every key its step reads
_TORCH_GROUP_DEFAULTS = dict(weight_decay=0, amsgrad=False, maximize=False, foreach=None, capturable=False, differentiable=False, fused=None,
                             decoupled_weight_decay=False)


def _moment_like(p):
    """Zeros of p's shape at p's offset from a 16-byte boundary: a parameter that is a view into a larger storage (a 12-float std behind
    the weights) and its moments then sit alike, and an aligned parameter's moments never keep it from the 16-byte path."""
    off = (p.data_ptr() % 16) // 4
    return torch.zeros(p.numel() + off, dtype=torch.float32, device=p.device)[off:].view(p.shape)


class FusedAdam:
    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, max_grad_norm=1.0, desired_kl=None):
        _validate_hyper(lr, betas, eps, max_grad_norm, desired_kl)
        self.params, self.names, self.device = check_parameters(params)
        self.betas, self.eps = (float(betas[0]), float(betas[1])), float(eps)
        self.max_grad_norm = None if max_grad_norm is None else float(max_grad_norm)
        self.desired_kl = None if desired_kl is None else float(desired_kl)
        # allocated once: the cell, both moments, the slab (sized for all parameters: a call with fewer needs no more), the result vector
        self.exp_avg = [_moment_like(p) for p in self.params]
        self.exp_avg_sq = [_moment_like(p) for p in self.params]
        self._state = torch.tensor([float(lr), 0.0], dtype=torch.float64, device=self.device)
        self._partials = torch.empty(workspace_doubles([p.numel() for p in self.params]), dtype=torch.float64, device=self.device)
        self._result = torch.zeros(abi.ADAM_RESULT_FLOATS, dtype=torch.float32, device=self.device)
        self._args = abi.LgAdamArgs()
        self._info = AdamStepInfo(self._result)

    # ---- the step ------------------------------------------------------------------------------------------------------------------
    def step(self, kl_mean=None):
        """Two launches on the current stream; nothing is read back.  Reads each p.grad where it lives now; a parameter whose .grad is None
        is left out of this call (its data and moments untouched, not in the norm).  With no gradient at all nothing is launched and the
        step count stays.  `kl_mean` (a 0-dim float32 device tensor) drives the adaptive rule and needs desired_kl; without it the rate
        stays."""
        args, live = adam_args(self.params, self.names, self.exp_avg, self.exp_avg_sq, self._state, self._partials, self._result, kl_mean,
                               self.betas, self.eps, self.max_grad_norm, self.desired_kl, self.device, self._args)
        if live:
            launch(args, self.device)
        return self._info

    def zero_grad(self, set_to_none=True):
        for p in self.params:
            if p.grad is None:
                continue
            if set_to_none:
                p.grad = None
            else:
                p.grad.detach_()
                p.grad.requires_grad_(False)
                p.grad.zero_()

    # ---- the cell ------------------------------------------------------------------------------------------------------------------
    @property
    def lr(self):
        """The learning rate in the cell.  Synchronises: for logging."""
        return float(self._state[abi.ADAM_S_LR].item())

    @property
    def step_count(self):
        """The step count in the cell.  Synchronises."""
        return int(self._state[abi.ADAM_S_STEP].item())

    def set_lr(self, lr):
        """Writes the cell on the current stream; does not synchronise."""
        self._state[abi.ADAM_S_LR:abi.ADAM_S_LR + 1].fill_(float(lr))

    # ---- checkpoints, in torch.optim.Adam's format ----------------------------------------------------------------------------------
    def state_dict(self):
        step = float(self._state[abi.ADAM_S_STEP].item())
        state = {}
        if step > 0:
            state = {i: dict(step=torch.tensor(step, dtype=torch.float32), exp_avg=self.exp_avg[i].clone(), exp_avg_sq=self.exp_avg_sq[i].clone())
                     for i in range(len(self.params))}
        group = dict(lr=self.lr, betas=self.betas, eps=self.eps, **_TORCH_GROUP_DEFAULTS, params=list(range(len(self.params))))
        return dict(state=state, param_groups=[group])

    def load_state_dict(self, sd):
        steps, moments = check_state_dict(sd, self.params, self.names)
        group = sd["param_groups"][0]
        _validate_hyper(group["lr"], group["betas"], group["eps"], self.max_grad_norm, self.desired_kl)
        self.betas, self.eps = (float(group["betas"][0]), float(group["betas"][1])), float(group["eps"])
        for i in range(len(self.params)):
            if i in moments:
                self.exp_avg[i].copy_(moments[i][0])
                self.exp_avg_sq[i].copy_(moments[i][1])
            else:                                        # torch keeps no state for a parameter that never had a gradient
                self.exp_avg[i].zero_()
                self.exp_avg_sq[i].zero_()
        self._state.copy_(torch.tensor([float(group["lr"]), steps], dtype=torch.float64))


def check_state_dict(sd, params, names):
    """A state dict in torch.optim.Adam's format against the parameter list: one parameter group over all parameters, moments of each
    parameter's shape, and one step count shared by every parameter that has state (the device keeps a single count).  Returns
    (step, {index: (exp_avg, exp_avg_sq)}).  No device is touched."""
    groups = sd.get("param_groups")
    if not isinstance(groups, (list, tuple)) or len(groups) != 1:
        raise ValueError(f"FusedAdam: the state dict has {len(groups) if isinstance(groups, (list, tuple)) else 'no'} parameter groups; "
                         "FusedAdam keeps one")
    group = groups[0]
    for key in ("lr", "betas", "eps", "params"):
        if key not in group:
            raise ValueError(f"FusedAdam: the state dict's parameter group has no '{key}'")
    for key in ("weight_decay", "amsgrad", "maximize"):
        if group.get(key):
            raise ValueError(f"FusedAdam: the state dict was written with {key} = {group[key]}; that is out of scope here")
    if len(group["params"]) != len(params):
        raise ValueError(f"FusedAdam: the state dict covers {len(group['params'])} parameters, the optimizer {len(params)}")
    steps, moments = {}, {}
    for i, pid in enumerate(group["params"]):
        st = sd["state"].get(pid)
        if st is None:
            continue
        for key in ("step", "exp_avg", "exp_avg_sq"):
            if key not in st:
                raise ValueError(f"FusedAdam: the state of {names[i]} has no '{key}'")
        for key in ("exp_avg", "exp_avg_sq"):
            if tuple(st[key].shape) != tuple(params[i].shape):
                raise ValueError(f"FusedAdam: {key} of {names[i]} has shape {tuple(st[key].shape)}, the parameter {tuple(params[i].shape)}")
        steps[i] = float(st["step"])
        moments[i] = (st["exp_avg"], st["exp_avg_sq"])
    if len(set(steps.values())) > 1:
        raise ValueError("FusedAdam: the parameters' step counts differ ("
                         + ", ".join(f"{names[i]}: {s:g}" for i, s in steps.items()) + "); the device keeps one count for all")
    return (next(iter(steps.values())) if steps else 0.0), moments
