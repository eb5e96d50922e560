"""The fused learner pass (include/lgtrain.h, csrc/lg_train.hip): the training forward of the plain ActorCritic of
rsl_rl/modules/actor_critic.py (two chains of Linear [+ ELU], a Hardtanh(+-clip_actions) behind the actor, sigma = mu * 0 + std) and its
backward, the block of PPO.update() between the mini-batch gather and the loss head and between the loss head and the optimizer:

    tp = FusedTrainPass(actor_critic)
    mu, sigma, values = tp(obs_batch, critic_obs_batch)          # one launch
    out = loss_fn(mu, sigma, values, ...)                        # FusedPPOLoss
    opt.zero_grad(); out.loss.backward(); opt.step(kl_mean=out.kl_mean)      # three launches of the pass, two of FusedAdam

It is one torch.autograd.Function: backward receives the gradients of mu, sigma and values, runs lg_train_backward into fresh gradient
tensors and returns them for the parameters; autograd sets or accumulates .grad as for any module.  The workspace (the stored
activations, the layer gradients, the slice partials) belongs to `tp`, grows to the largest batch seen and is reused, so a backward
whose forward has been overwritten by a later forward raises instead of using stale activations.  Weights are read where torch keeps
them on every call.  The gradient that reaches mu through sigma = mu * 0 + std is taken as exactly zero (include/lgtrain.h); there is no
gradient for the observations and no double backward.  There is no CPU path: the module lives on a HIP device."""
from __future__ import annotations

import ctypes as C

import torch
import torch.nn as nn

from . import abi

_OTHER_FAMILIES = (("estimator", "ActorCriticEE"), ("privilege_encoder", "ActorCriticTS / ActorCriticCTS"),
                   ("history_encoder", "ActorCriticTS / ActorCriticCTS"), ("vae", "ActorCriticDreamWaQ"),
                   ("memory_a", "ActorCriticRecurrent"), ("memory_c", "ActorCriticRecurrent"))


class TrainChainSpec:
    """One chain as the kernel takes it: its Linear modules in order, which of them an ELU follows, and (actor only) the clip."""

    def __init__(self, name, linears, elu, clip):
        self.name, self.linears, self.elu, self.clip = name, linears, elu, clip

    @property
    def widths(self):
        return [self.linears[0].in_features] + [l.out_features for l in self.linears]


class TrainSpec:
    def __init__(self, actor, critic, std):
        self.actor, self.critic, self.std = actor, critic, std
        self.chains = (actor, critic)
        self.num_actions, self.clip_actions = actor.widths[-1], actor.clip

    def parameters(self):
        """std, then weight and bias of every actor layer, then of every critic layer: the order of the pass's gradients."""
        return [self.std] + [p for c in self.chains for l in c.linears for p in (l.weight, l.bias)]

    def parameter_names(self):
        return ["std"] + [f"{c.name}.{i}.{n}" for c in self.chains for i in range(len(c.linears)) for n in ("weight", "bias")]


def _check_param(t, what, device):
    if not isinstance(t, torch.Tensor) or t.dtype != torch.float32:
        raise ValueError(f"FusedTrainPass: {what} is {getattr(t, 'dtype', type(t).__name__)}, the kernel reads float32")
    if not t.is_contiguous():
        raise ValueError(f"FusedTrainPass: {what} is not contiguous")
    if device is not None and t.device != device:
        raise ValueError(f"FusedTrainPass: {what} is on {t.device}, not on {device}")


def _describe_chain(name, seq, device, allow_clip):
    if not isinstance(seq, nn.Sequential):
        raise ValueError(f"FusedTrainPass: {name} is {type(seq).__name__}, expected an nn.Sequential of Linear / ELU"
                         + (" / Hardtanh" if allow_clip else ""))
    linears, elu, clip = [], [], None
    mods = list(seq)
    for i, m in enumerate(mods):
        where = f"{name}[{i}]"
        if clip is not None:
            raise ValueError(f"FusedTrainPass: {where} ({type(m).__name__}) follows the Hardtanh, which must end the actor")
        if isinstance(m, nn.Linear):
            if m.bias is None:
                raise ValueError(f"FusedTrainPass: {where} has no bias")
            if m.in_features > abi.POLICY_MAX_WIDTH or m.out_features > abi.POLICY_MAX_WIDTH:
                raise ValueError(f"FusedTrainPass: {where} is {m.in_features} -> {m.out_features}, widths are limited to {abi.POLICY_MAX_WIDTH}")
            if linears and linears[-1].out_features != m.in_features:
                raise ValueError(f"FusedTrainPass: {where} takes {m.in_features} inputs, the layer before it gives {linears[-1].out_features}")
            _check_param(m.weight, f"{where}.weight", device)
            _check_param(m.bias, f"{where}.bias", device)
            linears.append(m)
            elu.append(False)
        elif isinstance(m, nn.ELU):
            if not linears or elu[-1]:
                raise ValueError(f"FusedTrainPass: {where} (ELU) does not follow a Linear")
            if m.alpha != 1.0:
                raise ValueError(f"FusedTrainPass: {where} is ELU(alpha={m.alpha}), only alpha = 1 is built")
            elu[-1] = True
        elif isinstance(m, nn.Hardtanh) and allow_clip:
            if i != len(mods) - 1 or not linears or elu[-1] or m.min_val != -m.max_val or not m.max_val >= 0:
                raise ValueError(f"FusedTrainPass: {where} (Hardtanh({m.min_val}, {m.max_val})) must be the symmetric clip behind the actor's last Linear")
            clip = float(m.max_val)
        else:
            raise ValueError(f"FusedTrainPass: {where} is {type(m).__name__}; only Linear and ELU"
                             + (" (and a final Hardtanh)" if allow_clip else "") + " are built into the kernel")
    if not linears:
        raise ValueError(f"FusedTrainPass: {name} has no Linear layer")
    if len(linears) > abi.POLICY_MAX_LAYERS:
        raise ValueError(f"FusedTrainPass: {name} has {len(linears)} Linear layers, the kernel takes {abi.POLICY_MAX_LAYERS}")
    if elu[-1]:
        raise ValueError(f"FusedTrainPass: {name} ends in an ELU, expected a Linear output layer")
    return TrainChainSpec(name, linears, elu, clip)


def describe(actor_critic, device=None):
    """The plain ActorCritic as the kernel takes it (duck-typed: .actor, .critic, .std).  Refusals are ValueErrors that name the layer or
    the member; with `device` every parameter must live there."""
    for attr, family in _OTHER_FAMILIES:
        if getattr(actor_critic, attr, None) is not None:
            raise ValueError(f"FusedTrainPass: the module has .{attr} ({family}); only the plain ActorCritic is built, the other learners "
                             f"keep the torch path")
    if getattr(actor_critic, "is_recurrent", False):
        raise ValueError("FusedTrainPass: the module is recurrent (is_recurrent); the recurrent update keeps the torch path")
    for need in ("actor", "critic", "std"):
        if getattr(actor_critic, need, None) is None:
            raise ValueError(f"FusedTrainPass: the module has no .{need}")
    actor = _describe_chain("actor", actor_critic.actor, device, True)
    critic = _describe_chain("critic", actor_critic.critic, device, False)
    std = actor_critic.std
    _check_param(std, "std", device)
    if tuple(std.shape) != (actor.widths[-1],):
        raise ValueError(f"FusedTrainPass: std has shape {tuple(std.shape)}, the actor has {actor.widths[-1]} outputs")
    return TrainSpec(actor, critic, std)


def _rows(t, width, what, n=None, device=None):
    """(n, width) float32 with unit inner stride: (pointer, row stride)."""
    ok = isinstance(t, torch.Tensor) and t.dtype == torch.float32 and t.dim() == 2 and t.shape[1] == width and (n is None or t.shape[0] == n) \
        and (t.shape[1] == 1 or t.stride(1) == 1) and (t.shape[0] == 1 or t.stride(0) >= width) and (device is None or t.device == device)
    if not ok:
        got = f"{tuple(t.shape)} {t.dtype} on {t.device}, strides {tuple(t.stride())}" if isinstance(t, torch.Tensor) else type(t).__name__
        raise ValueError(f"FusedTrainPass: {what} must be ({'B' if n is None else n}, {width}) float32 with unit inner stride"
                         + (f" on {device}" if device is not None else "") + f"; got {got}")
    return t.data_ptr(), (t.stride(0) if t.shape[0] > 1 else width)


def train_args(spec, obs, critic_obs, mu, sigma, values, workspace, grads=None, grad_mu=None, grad_sigma=None, grad_values=None, device=None):
    """LgTrainArgs of one call; every matrix is addressed in place (row stride, unit inner stride), the weights where they live now.
    `grads` (backward): the tensors that take the gradients, in spec.parameters() order, contiguous.  Refusals are ValueErrors that name
    the tensor; the library is not touched."""
    a = abi.LgTrainArgs()
    if not isinstance(obs, torch.Tensor) or obs.dim() != 2 or obs.shape[0] < 1:
        raise ValueError(f"FusedTrainPass: obs must be a (B, {spec.actor.widths[0]}) float32 tensor with B >= 1")
    n = int(obs.shape[0])
    a.n_rows = n
    a.clip_on, a.clip_actions = (1, spec.clip_actions) if spec.clip_actions is not None else (0, 0.0)
    gi = 1
    for ci, (c, x, what) in enumerate(zip(spec.chains, (obs, critic_obs), ("obs", "critic_obs"))):
        ch = a.chain[ci]
        ch.input, ch.in_stride = _rows(x, c.widths[0], what, n, device)
        ch.n_layers = len(c.linears)
        for li, (lin, elu) in enumerate(zip(c.linears, c.elu)):
            L = ch.layer[li]
            _check_param(lin.weight, f"{c.name} layer {li} weight", device)
            _check_param(lin.bias, f"{c.name} layer {li} bias", device)
            L.weight, L.bias, L.n_in, L.n_out, L.elu = lin.weight.data_ptr(), lin.bias.data_ptr(), lin.in_features, lin.out_features, int(elu)
            if grads is not None:
                L.grad_weight, L.grad_bias = grads[gi].data_ptr(), grads[gi + 1].data_ptr()
            gi += 2
    A, V = spec.num_actions, spec.critic.widths[-1]
    _check_param(spec.std, "std", device)
    a.std = spec.std.data_ptr()
    a.mu, a.mu_stride = _rows(mu, A, "mu", n, device)
    a.sigma, a.sigma_stride = _rows(sigma, A, "sigma", n, device)
    a.values, a.values_stride = _rows(values, V, "values", n, device)
    if grads is not None:
        a.grad_std = grads[0].data_ptr()
        a.grad_mu, a.grad_mu_stride = _rows(grad_mu, A, "grad_mu", n, device)
        a.grad_sigma, a.grad_sigma_stride = _rows(grad_sigma, A, "grad_sigma", n, device)
        a.grad_values, a.grad_values_stride = _rows(grad_values, V, "grad_values", n, device)
    if workspace is not None:
        if not isinstance(workspace, torch.Tensor) or workspace.dtype != torch.float32 or not workspace.is_contiguous() \
                or (device is not None and workspace.device != device):
            raise ValueError("FusedTrainPass: the workspace must be a contiguous float32 tensor" + (f" on {device}" if device is not None else ""))
        a.workspace, a.workspace_capacity = workspace.data_ptr(), workspace.numel()
    return a


def plan_of(args):
    """LgTrainPlan of a descriptor (lg_train_plan): the shapes alone, nothing is launched."""
    lib = abi.load_lib()
    p = abi.LgTrainPlan()
    abi.check(lib.lg_train_plan(C.byref(args), C.byref(p)), lib)
    return p


_PLANS = {}      # (n_rows, actor widths, critic widths) -> LgTrainPlan: a pure function of the shapes


def plan(n_rows, actor_widths, critic_widths):
    """LgTrainPlan for n_rows rows of chains with these widths ([in, out_0, out_1, ...] each)."""
    key = (int(n_rows), tuple(int(w) for w in actor_widths), tuple(int(w) for w in critic_widths))
    if key not in _PLANS:
        a = abi.LgTrainArgs()
        a.n_rows = key[0]
        for ci, w in enumerate(key[1:]):
            a.chain[ci].n_layers = len(w) - 1
            for li in range(min(len(w) - 1, abi.POLICY_MAX_LAYERS)):
                a.chain[ci].layer[li].n_in, a.chain[ci].layer[li].n_out = w[li], w[li + 1]
        _PLANS[key] = plan_of(a)
    return _PLANS[key]


def forward(args, device):
    """lg_train_forward on the current stream of `device`."""
    lib = abi.load_lib()
    abi.check(lib.lg_train_forward(C.byref(args), torch.cuda.current_stream(device).cuda_stream), lib)


def backward(args, device):
    """lg_train_backward on the current stream of `device`."""
    lib = abi.load_lib()
    abi.check(lib.lg_train_backward(C.byref(args), torch.cuda.current_stream(device).cuda_stream), lib)


def _grad_rows(g, like):
    """An incoming gradient as the kernel reads it: zeros where autograd passed none, a copy where the strides do not fit."""
    if g is None:
        return torch.zeros_like(like)
    if g.dtype != torch.float32 or (g.shape[1] > 1 and g.stride(1) != 1) or (g.shape[0] > 1 and g.stride(0) < g.shape[1]):
        return g.to(torch.float32).contiguous()
    return g


class _Pass(torch.autograd.Function):
    @staticmethod
    def forward(ctx, tp, obs, critic_obs, *params):
        spec, device, n = tp.spec, tp.device, int(obs.shape[0])
        mu = torch.empty((n, spec.num_actions), dtype=torch.float32, device=device)
        sigma = torch.empty_like(mu)
        values = torch.empty((n, spec.critic.widths[-1]), dtype=torch.float32, device=device)
        args = train_args(spec, obs, critic_obs, mu, sigma, values, None, device=device)      # every refusal before anything grows
        ws = tp._workspace_for(n)
        args.workspace, args.workspace_capacity = ws.data_ptr(), ws.numel()
        forward(args, device)
        tp._calls += 1
        ctx.tp, ctx.call, ctx.obs, ctx.critic_obs = tp, tp._calls, obs, critic_obs
        ctx.save_for_backward(mu, sigma, values)
        return mu, sigma, values

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_mu, grad_sigma, grad_values):
        tp = ctx.tp
        if tp._calls != ctx.call:
            raise RuntimeError(f"FusedTrainPass: backward of forward call {ctx.call}, but forward call {tp._calls} has overwritten its "
                               f"activations in the workspace since; run each backward before the next forward")
        mu, sigma, values = ctx.saved_tensors
        spec, device = tp.spec, tp.device
        grads = [torch.empty_like(p) for p in spec.parameters()]
        gm, gs, gv = _grad_rows(grad_mu, mu), _grad_rows(grad_sigma, sigma), _grad_rows(grad_values, values)
        args = train_args(spec, ctx.obs, ctx.critic_obs, mu, sigma, values, tp._workspace, grads, gm, gs, gv, device=device)
        backward(args, device)
        return (None, None, None) + tuple(grads)


class FusedTrainPass:
    def __init__(self, actor_critic):
        dev = getattr(getattr(actor_critic, "std", None), "device", None)
        if isinstance(dev, torch.device) and dev.type != "cuda":
            raise ValueError(f"FusedTrainPass: the module is on {dev}, not on a HIP device (there is no CPU path)")
        self.spec = describe(actor_critic, dev)
        self.device = dev
        self._workspace = None
        self._calls = 0

    def _workspace_for(self, n):
        need = int(plan(n, self.spec.actor.widths, self.spec.critic.widths).workspace_floats)
        if self._workspace is None or self._workspace.numel() < need:
            self._workspace = torch.empty(need, dtype=torch.float32, device=self.device)
        return self._workspace

    def plan(self, n_rows):
        return plan(n_rows, self.spec.actor.widths, self.spec.critic.widths)

    def __call__(self, obs, critic_obs):
        """(mu, sigma, values) of the mini-batch: (B, A), (B, A), (B, 1).  One launch on the current stream."""
        return _Pass.apply(self, obs, critic_obs, *self.spec.parameters())
