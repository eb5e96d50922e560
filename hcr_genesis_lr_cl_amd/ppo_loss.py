"""The fused PPO loss head (include/lgppo.h, csrc/lg_ppo.hip): what PPO._compute_rl_loss (rsl_rl/algorithms/ppo.py:157-218, and the
identical blocks of PPO_EE / PPO_TS / PPO_DreamWaQ) and PPO_CTS._compute_rl_loss (ppo_cts.py:193-267) do behind the network forward, as
one call: the loss, its parts, the KL of the adaptive schedule and the gradient with respect to mu, sigma and values.

    loss_fn = FusedPPOLoss(clip_param=0.2, value_loss_coef=1.0, entropy_coef=0.01)
    out = loss_fn(mu, sigma, values, actions, old_log_prob, advantages, returns, target_values, old_mu, old_sigma)
    out.loss.backward()                                   # the stored gradients times the incoming scalar, into the networks
    lr = adjust_learning_rate(out.kl_mean, lr, desired_kl)  # the one .item() the reference also pays

`out.surrogate_loss`, `out.value_loss`, `out.entropy` and `out.kl_mean` are detached 0-dim views of the result vector: nothing synchronises
until the caller reads one.  `loss_fn.cts(teacher=dict(...), student=dict(...), values=..., returns=..., target_values=...)` is the
two-group form.  There is no CPU path: the tensors live on a HIP device."""
from __future__ import annotations

import ctypes as C

import torch

from . import abi

_GROUP_KEYS = ("mu", "sigma", "actions", "old_log_prob", "advantages", "old_mu", "old_sigma")


def adjust_learning_rate(kl_mean, learning_rate, desired_kl):
    """The host rule of ppo.py:193-206: the new learning rate for the KL this mini-batch measured."""
    kl = float(kl_mean)
    if kl > desired_kl * 2.0:
        return max(1e-5, learning_rate / 1.5)
    if kl < desired_kl / 2.0 and kl > 0.0:
        return min(1e-2, learning_rate * 1.5)
    return learning_rate


def _refuse(what, t, want):
    got = f"{tuple(t.shape)} {t.dtype} on {t.device}, strides {tuple(t.stride())}" if isinstance(t, torch.Tensor) else type(t).__name__
    raise ValueError(f"FusedPPOLoss: {what} must be {want}; got {got}")


def _matrix(t, what, rows, width, device):
    """A (rows, width) float32 view with unit inner stride on `device`: (pointer, row stride)."""
    want = f"a ({'B' if rows is None else rows}, {width}) float32 tensor with unit inner stride on {device}"
    if not isinstance(t, torch.Tensor) or t.dtype != torch.float32 or t.dim() != 2 or t.shape[1] != width or t.device != device:
        _refuse(what, t, want)
    if rows is not None and t.shape[0] != rows:
        _refuse(what, t, want)
    if t.shape[1] > 1 and t.stride(1) != 1:
        _refuse(what, t, want)
    if t.shape[0] > 1 and t.stride(0) < width:
        _refuse(what, t, want)
    return t.data_ptr(), (t.stride(0) if t.shape[0] > 1 else width)


def _column(t, what, rows, device):
    """(rows, 1) or (rows,) float32: (pointer, row stride)."""
    want = f"a ({rows}, 1) or ({rows},) float32 tensor on {device}"
    if not isinstance(t, torch.Tensor) or t.dtype != torch.float32 or t.device != device or t.dim() not in (1, 2):
        _refuse(what, t, want)
    if t.shape[0] != rows or (t.dim() == 2 and t.shape[1] != 1):
        _refuse(what, t, want)
    if rows > 1 and t.stride(0) < 1:
        _refuse(what, t, want)
    return t.data_ptr(), (t.stride(0) if rows > 1 else 1)


def _device_of(mu):
    if not isinstance(mu, torch.Tensor):
        raise ValueError(f"FusedPPOLoss: mu must be a float32 tensor on a HIP device; got {type(mu).__name__}")
    if mu.device.type != "cuda":
        raise ValueError(f"FusedPPOLoss: mu is on {mu.device}, not on a HIP device; there is no CPU path")
    return mu.device


def ppo_loss_args(groups, values, returns, target_values, grad_values, partials, result, clip_param, value_loss_coef, entropy_coef, flags,
                  device=None, outputs=True):
    """LgPpoLossArgs for one or two policy groups, each a dict of mu, sigma, actions, old_log_prob, advantages, grad_mu, grad_sigma and
    optionally old_mu, old_sigma; every tensor is addressed in place (row stride, unit inner stride).  Refusals are ValueErrors that name
    the tensor; the library is not touched.  `device` defaults to the device of the first mu.  outputs=False describes the inputs alone:
    grad_mu, grad_sigma, grad_values, partials and result are not read and stay null for `set_outputs`."""
    if len(groups) < 1 or len(groups) > abi.PPO_MAX_GROUPS:
        raise ValueError(f"FusedPPOLoss: {len(groups)} policy groups; the kernel takes 1 .. {abi.PPO_MAX_GROUPS}")
    device = device if device is not None else groups[0]["mu"].device
    a = abi.LgPpoLossArgs()
    mu0 = groups[0]["mu"]
    if not isinstance(mu0, torch.Tensor) or mu0.dim() != 2:
        _refuse("mu", mu0, "a (B, A) float32 tensor")
    A = int(mu0.shape[1])
    if A < 1 or A > abi.PPO_MAX_ACTIONS:
        raise ValueError(f"FusedPPOLoss: mu has {A} action columns; the kernel takes 1 .. {abi.PPO_MAX_ACTIONS}")
    a.n_groups, a.n_actions, a.flags = len(groups), A, int(flags)
    for gi, g in enumerate(groups):
        tag = "" if len(groups) == 1 else ("teacher." if gi == 0 else "student.")
        G = a.group[gi]
        mu = g["mu"]
        if not isinstance(mu, torch.Tensor) or mu.dim() != 2:
            _refuse(tag + "mu", mu, f"a (B, {A}) float32 tensor")
        B = int(mu.shape[0])
        if B < 1:
            raise ValueError(f"FusedPPOLoss: {tag}mu has no rows: an empty group")
        G.n_rows = B
        if (g.get("old_mu") is None) != (g.get("old_sigma") is None):
            raise ValueError(f"FusedPPOLoss: {tag}old_mu and {tag}old_sigma come together (the KL needs both); "
                             f"got {'old_mu' if g.get('old_mu') is not None else 'old_sigma'} alone")
        for key in ("mu", "sigma", "actions", "old_mu", "old_sigma") + (("grad_mu", "grad_sigma") if outputs else ()):
            if g.get(key) is None and key in ("old_mu", "old_sigma"):
                continue
            ptr, stride = _matrix(g.get(key), tag + key, B, A, device)
            setattr(G, key, ptr)
            setattr(G, key + "_stride", stride)
        for key in ("old_log_prob", "advantages"):
            ptr, stride = _column(g.get(key), tag + key, B, device)
            setattr(G, key, ptr)
            setattr(G, key + "_stride", stride)
    if not isinstance(values, torch.Tensor) or values.dim() not in (1, 2):
        _refuse("values", values, "a (B, 1) float32 tensor")
    Bv = int(values.shape[0])
    if Bv < 1:
        raise ValueError("FusedPPOLoss: values has no rows: an empty group")
    a.n_value_rows = Bv
    for key, t in (("values", values), ("returns", returns), ("target_values", target_values)) + ((("grad_values", grad_values),) if outputs else ()):
        ptr, stride = _column(t, key, Bv, device)
        setattr(a, key, ptr)
        setattr(a, key + "_stride", stride)
    a.clip_param, a.value_loss_coef, a.entropy_coef = float(clip_param), float(value_loss_coef), float(entropy_coef)
    if not outputs:
        return a
    if not isinstance(partials, torch.Tensor) or partials.dtype != torch.float64 or not partials.is_contiguous() or partials.device != device:
        _refuse("partials", partials, f"a contiguous float64 tensor on {device}")
    if not isinstance(result, torch.Tensor) or result.dtype != torch.float32 or not result.is_contiguous() or result.device != device \
            or result.numel() < abi.PPO_RESULT_FLOATS:
        _refuse("result", result, f"a contiguous float32 tensor of {abi.PPO_RESULT_FLOATS} elements on {device}")
    a.partials, a.partials_capacity, a.result = partials.data_ptr(), partials.numel(), result.data_ptr()
    return a


_WORKSPACE = {}      # (group rows, value rows, actions) -> doubles: the plan is a pure function of the shapes


def workspace_doubles(group_rows, value_rows, num_actions):
    """Doubles the partials slab needs (lg_ppo_loss_workspace): the plan alone, nothing is launched."""
    key = (tuple(int(b) for b in group_rows), int(value_rows), int(num_actions))
    if key in _WORKSPACE:
        return _WORKSPACE[key]
    lib = abi.load_lib()
    a = abi.LgPpoLossArgs()
    a.n_groups, a.n_actions, a.n_value_rows = len(group_rows), int(num_actions), int(value_rows)
    for i, b in enumerate(group_rows[:abi.PPO_MAX_GROUPS]):
        a.group[i].n_rows = int(b)
    n = lib.lg_ppo_loss_workspace(C.byref(a))
    if n == 0:
        abi.check(1, lib)
    _WORKSPACE[key] = n
    return n


def launch(args, device):
    """lg_ppo_loss on the current stream of `device`."""
    lib = abi.load_lib()
    abi.check(lib.lg_ppo_loss(C.byref(args), torch.cuda.current_stream(device).cuda_stream), lib)


class PPOLossResult:
    """`loss` carries the graph; the others are detached 0-dim views of the result vector (`result`)."""

    def __init__(self, loss, result, n_groups):
        self.loss, self.result = loss, result
        self.value_loss, self.entropy = result[abi.PPO_R_VALUE], result[abi.PPO_R_ENTROPY]
        self.surrogate_loss, self.kl_mean = result[abi.PPO_R_SURROGATE], result[abi.PPO_R_KL]
        if n_groups == 2:
            self.teacher_surrogate_loss, self.student_surrogate_loss = result[abi.PPO_R_SURROGATE], result[abi.PPO_R_SURROGATE + 1]
            self.surrogate_losses = (self.teacher_surrogate_loss, self.student_surrogate_loss)
            self.student_kl_mean = result[abi.PPO_R_KL + 1]


class _Loss(torch.autograd.Function):
    """Forward is the launch; backward hands out the gradients it stored, times the incoming scalar."""

    @staticmethod
    def forward(ctx, args, *diff):
        # diff = (mu_0, sigma_0[, mu_1, sigma_1], values): the tensors the loss is a function of; `args` describes them and the stored
        # columns (checked by _run) and gets its outputs here: fresh contiguous tensors, so there is nothing to refuse
        device = diff[0].device
        n, A = args.n_groups, args.n_actions
        grads = []
        for gi in range(n):
            G = args.group[gi]
            grads += [torch.empty((G.n_rows, A), dtype=torch.float32, device=device), torch.empty((G.n_rows, A), dtype=torch.float32, device=device)]
            G.grad_mu, G.grad_sigma, G.grad_mu_stride, G.grad_sigma_stride = grads[-2].data_ptr(), grads[-1].data_ptr(), A, A
        grads.append(torch.empty(diff[-1].shape, dtype=torch.float32, device=device))
        result = torch.empty(abi.PPO_RESULT_FLOATS, dtype=torch.float32, device=device)
        partials = torch.empty(workspace_doubles([args.group[gi].n_rows for gi in range(n)], args.n_value_rows, A), dtype=torch.float64,
                               device=device)
        args.grad_values, args.grad_values_stride = grads[-1].data_ptr(), 1
        args.partials, args.partials_capacity, args.result = partials.data_ptr(), partials.numel(), result.data_ptr()
        launch(args, device)
        ctx.grads = grads
        ctx.mark_non_differentiable(result)
        return result[abi.PPO_R_LOSS].clone(), result

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_loss, _grad_result):
        return (None,) + tuple(g * grad_loss for g in ctx.grads)


class FusedPPOLoss:
    def __init__(self, clip_param=0.2, value_loss_coef=1.0, entropy_coef=0.0, use_clipped_value_loss=True, use_spo=False):
        if not clip_param > 0.0:
            raise ValueError(f"FusedPPOLoss: clip_param = {clip_param}; it must be above 0")
        self.clip_param, self.value_loss_coef, self.entropy_coef = float(clip_param), float(value_loss_coef), float(entropy_coef)
        self.use_clipped_value_loss, self.use_spo = bool(use_clipped_value_loss), bool(use_spo)

    @property
    def flags(self):
        return (abi.PPO_CLIPPED_VALUE if self.use_clipped_value_loss else 0) | (abi.PPO_SPO if self.use_spo else 0)

    adjust_learning_rate = staticmethod(adjust_learning_rate)

    def _run(self, groups, values, returns, target_values):
        device = _device_of(groups[0]["mu"])
        # every refusal before anything is allocated or the library is loaded; the tensors stay alive in the caller's frame over the launch
        args = ppo_loss_args(groups, values, returns, target_values, None, None, None, self.clip_param, self.value_loss_coef, self.entropy_coef,
                             self.flags, device, outputs=False)
        loss, result = _Loss.apply(args, *[t for g in groups for t in (g["mu"], g["sigma"])], values)
        return PPOLossResult(loss, result, len(groups))

    def __call__(self, mu, sigma, values, actions, old_log_prob, advantages, returns, target_values, old_mu=None, old_sigma=None):
        g = dict(mu=mu, sigma=sigma, actions=actions, old_log_prob=old_log_prob, advantages=advantages, old_mu=old_mu, old_sigma=old_sigma)
        return self._run([g], values, returns, target_values)

    def cts(self, teacher, student, values, returns, target_values):
        """Two policy row groups (ppo_cts.py:193-267): `teacher` and `student` are dicts of mu, sigma, actions, old_log_prob, advantages and
        optionally old_mu, old_sigma; one value group.  The result carries teacher_surrogate_loss and student_surrogate_loss."""
        for name, g in (("teacher", teacher), ("student", student)):
            unknown = set(g) - set(_GROUP_KEYS)
            if unknown:
                raise ValueError(f"FusedPPOLoss: {name} has unknown entries {sorted(unknown)}; expected {list(_GROUP_KEYS)}")
        return self._run([dict(teacher), dict(student)], values, returns, target_values)
