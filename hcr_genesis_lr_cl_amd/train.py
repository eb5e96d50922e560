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
gradient for the observations and no double backward.  There is no CPU path: the module lives on a HIP device.

FusedTrainPassEE (below; include/lgtrainee.h, csrc/lg_train_ee.hip) is the same for ActorCriticEE under PPO_EE: the RL pass and the
supervised estimator pass.  FusedTrainPassTS (include/lgtraints.h, csrc/lg_train_ts.hip) is the same for ActorCriticTS under PPO_TS: the RL
pass, whose gradient reaches the privilege encoder through the latent, and the supervised history-encoder pass.  FusedTrainPassDreamWaQ
(include/lgtraindwaq.h, csrc/lg_train_dwaq.hip) is the same for ActorCriticDreamWaQ under PPO_DreamWaQ: the RL pass behind the VAE's
encoder, heads and reparameterised draw, and the VAE pass with its three losses.  FusedTrainPassCTS (include/lgtraincts.h,
csrc/lg_train_cts.hip) is the same for ActorCriticCTS under PPO_CTS: the RL pass over the teacher's, the student's and the critic's rows, and
the history-encoder pass on the teacher-student family's encoder kernels with a mask of ones.  FusedTrainPassTSTcn (include/lgtraintcn.h,
csrc/lg_train_tcn.hip) is FusedTrainPassTS for an ActorCriticTS whose history encoder is a "TCN" (Conv1d stack, Flatten, Linear tail).  FusedTrainPassRecurrent
(include/lgtrainrnn.h, csrc/lg_train_rnn.hip) is the same for ActorCriticRecurrent under PPO: the two memories over the padded trajectories
of a recurrent mini-batch, the two MLPs on the unpadded rows, and the backward through the MLPs, through time and into the memories.

The five families share what is below `_Pass`: one record per pass (workspace, call counter, entry points, descriptor builder), one
autograd.Function for an RL pass and one for a loss pass, driven by that record.  A refusal carries the name of the surface that first
raised it, which is why the helpers take an `owner`.  What a chain, a head, a parameter tensor or a row matrix must be is nets.py's, shared
with policy.py; this module keeps what must hold between a family's chains."""
from __future__ import annotations

import ctypes as C

import torch
import torch.nn as nn

from . import abi, nets, policy
from .nets import ChainSpec as TrainChainSpec      # the name callers and tests know it by here

_OTHER_FAMILIES = (("estimator", "ActorCriticEE"), ("privilege_encoder", "ActorCriticTS / ActorCriticCTS"),
                   ("history_encoder", "ActorCriticTS / ActorCriticCTS"), ("vae", "ActorCriticDreamWaQ"),
                   ("memory_a", "ActorCriticRecurrent"), ("memory_c", "ActorCriticRecurrent"))
_PLAIN, _EE, _TS, _DWAQ, _CTS = "FusedTrainPass", "FusedTrainPassEE", "FusedTrainPassTS", "FusedTrainPassDreamWaQ", "FusedTrainPassCTS"
_RNN = "FusedTrainPassRecurrent"


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


def _describe(actor_critic, device, owner, foreign, beside, chains, between=None):
    """What describe, describe_ee and describe_ts share: no member of another family (`foreign`; `beside` ends that refusal), not
    recurrent, .actor / .critic / .std there, the chains of `chains` ((name, may end in a Hardtanh) pairs) by nets.describe_chain, the
    family's own checks across them (`between`) and the shape of std.  Returns the chain specs by name, and std."""
    for attr, family in foreign:
        if getattr(actor_critic, attr, None) is not None:
            raise ValueError(f"{owner}: the module has .{attr} ({family}){beside}")
    if getattr(actor_critic, "is_recurrent", False):
        raise ValueError(f"{owner}: the module is recurrent (is_recurrent); the recurrent update keeps the torch path")
    for need in ("actor", "critic", "std"):
        if getattr(actor_critic, need, None) is None:
            raise ValueError(f"{owner}: the module has no .{need}")
    c = {name: nets.describe_chain(name, getattr(actor_critic, name), device, clip, owner) for name, clip in chains}
    if between is not None:
        between(c)
    std = actor_critic.std
    nets.check_std(std, c["actor"], device, owner)
    return c, std


def describe(actor_critic, device=None):
    """The plain ActorCritic as the kernel takes it (duck-typed: .actor, .critic, .std).  Refusals are ValueErrors that name the layer or
    the member; with `device` every parameter must live there."""
    c, std = _describe(actor_critic, device, _PLAIN, _OTHER_FAMILIES, "; only the plain ActorCritic is built, the other learners keep the torch path",
                       (("actor", True), ("critic", False)))
    return TrainSpec(c["actor"], c["critic"], std)


def _fill_chain(ch, c, device, grads=None):
    """Widths, flags and weight pointers of one LgTrainChain; `grads`: [weight, bias, weight, bias, ...] tensors of its layers."""
    ch.n_layers = len(c.linears)
    for li, (lin, elu) in enumerate(zip(c.linears, c.elu)):
        L = ch.layer[li]
        nets.check_tensor(lin.weight, f"{c.name} layer {li} weight", device, _PLAIN)        # in the plain pass's name for every family: no owner
        nets.check_tensor(lin.bias, f"{c.name} layer {li} bias", device, _PLAIN)            # reaches here, and test_train_host.py pins this text
        L.weight, L.bias, L.n_in, L.n_out, L.elu = lin.weight.data_ptr(), lin.bias.data_ptr(), lin.in_features, lin.out_features, int(elu)
        if grads is not None:
            L.grad_weight, L.grad_bias = grads[2 * li].data_ptr(), grads[2 * li + 1].data_ptr()


def _fill_heads(a, spec, mu, sigma, values, n, device, owner, grad_std=None, grad_mu=None, grad_sigma=None, grad_values=None):
    """The clip, std, the three outputs and (backward: grad_std is given) the gradient members of an RL descriptor of `owner`."""
    A, V = spec.num_actions, spec.critic.widths[-1]
    a.clip_on, a.clip_actions = (1, spec.clip_actions) if spec.clip_actions is not None else (0, 0.0)
    nets.check_tensor(spec.std, "std", device, owner)
    a.std = spec.std.data_ptr()
    a.mu, a.mu_stride = nets.rows(mu, A, "mu", n, device, owner)
    a.sigma, a.sigma_stride = nets.rows(sigma, A, "sigma", n, device, owner)
    a.values, a.values_stride = nets.rows(values, V, "values", n, device, owner)
    if grad_std is not None:
        a.grad_std = grad_std.data_ptr()
        a.grad_mu, a.grad_mu_stride = nets.rows(grad_mu, A, "grad_mu", n, device, owner)
        a.grad_sigma, a.grad_sigma_stride = nets.rows(grad_sigma, A, "grad_sigma", n, device, owner)
        a.grad_values, a.grad_values_stride = nets.rows(grad_values, V, "grad_values", n, device, owner)


def _bind_workspace(a, workspace, device, owner=_EE):
    if workspace is not None:
        if not isinstance(workspace, torch.Tensor) or workspace.dtype != torch.float32 or not workspace.is_contiguous() \
                or (device is not None and workspace.device != device):
            raise ValueError(f"{owner}: the workspace must be a contiguous float32 tensor" + (f" on {device}" if device is not None else ""))
        a.workspace, a.workspace_capacity = workspace.data_ptr(), workspace.numel()


def _scalar(t, what, device, n=1, owner=_EE):
    if not isinstance(t, torch.Tensor) or t.dtype != torch.float32 or t.numel() != n or not t.is_contiguous() or (device is not None and t.device != device):
        raise ValueError(f"{owner}: {what} must be {'one' if n == 1 else n} float32" + (f" on {device}" if device is not None else ""))
    return t.data_ptr()


def train_args(spec, obs, critic_obs, mu, sigma, values, workspace, grads=None, grad_mu=None, grad_sigma=None, grad_values=None, device=None):
    """LgTrainArgs of one call; every matrix is addressed in place (row stride, unit inner stride), the weights where they live now.
    `grads` (backward): the tensors that take the gradients, in spec.parameters() order, contiguous.  Refusals are ValueErrors that name
    the tensor; the library is not touched."""
    a = abi.LgTrainArgs()
    if not isinstance(obs, torch.Tensor) or obs.dim() != 2 or obs.shape[0] < 1:
        raise ValueError(f"FusedTrainPass: obs must be a (B, {spec.actor.widths[0]}) float32 tensor with B >= 1")
    n = int(obs.shape[0])
    a.n_rows = n
    g0 = 1
    for ch, c, x, what in zip(a.chain, spec.chains, (obs, critic_obs), ("obs", "critic_obs")):
        ch.input, ch.in_stride = nets.rows(x, c.widths[0], what, n, device, _PLAIN)
        _fill_chain(ch, c, device, None if grads is None else grads[g0:g0 + 2 * len(c.linears)])
        g0 += 2 * len(c.linears)
    _fill_heads(a, spec, mu, sigma, values, n, device, _PLAIN, *(() if grads is None else (grads[0], grad_mu, grad_sigma, grad_values)))
    _bind_workspace(a, workspace, device, _PLAIN)
    return a


def _widths_into(ch, w):
    ch.n_layers = len(w) - 1
    for li in range(min(len(w) - 1, abi.POLICY_MAX_LAYERS)):
        ch.layer[li].n_in, ch.layer[li].n_out = w[li], w[li + 1]


def plan_of(args):
    """LgTrainPlan of a descriptor (lg_train_plan): the shapes alone, nothing is launched."""
    lib = abi.load_lib()
    p = abi.LgTrainPlan()
    abi.check(lib.lg_train_plan(C.byref(args), C.byref(p)), lib)
    return p


_PLANS = {}      # (entry point, n_rows, (chain, widths) ...) -> its plan struct: a pure function of the shapes


def _plan(entry, args_cls, plan_cls, n_rows, chains, **scalars):
    """The plan `entry` gives for n_rows rows and chains of these widths ([in, out_0, out_1, ...] each).  `chains`: (index into the
    descriptor's chain array, None where it has the one chain; widths) pairs; `scalars`: further descriptor members."""
    key = (entry, int(n_rows)) + tuple((i, tuple(int(x) for x in w)) for i, w in chains)
    if key not in _PLANS:
        lib, a, p = abi.load_lib(), args_cls(), plan_cls()
        a.n_rows = key[1]
        for i, w in key[2:]:
            _widths_into(a.chain if i is None else a.chain[i], w)
        for k, v in scalars.items():
            setattr(a, k, v)
        abi.check(getattr(lib, entry)(C.byref(a), C.byref(p)), lib)
        _PLANS[key] = p
    return _PLANS[key]


def plan(n_rows, actor_widths, critic_widths):
    """LgTrainPlan for n_rows rows of chains with these widths ([in, out_0, out_1, ...] each)."""
    return _plan("lg_train_plan", abi.LgTrainArgs, abi.LgTrainPlan, n_rows, ((0, actor_widths), (1, critic_widths)))


def _call(name, args, device):
    lib = abi.load_lib()
    abi.check(getattr(lib, name)(C.byref(args), torch.cuda.current_stream(device).cuda_stream), lib)


def forward(args, device):
    """lg_train_forward on the current stream of `device`."""
    _call("lg_train_forward", args, device)


def backward(args, device):
    """lg_train_backward on the current stream of `device`."""
    _call("lg_train_backward", args, device)


def _grad_rows(g, like):
    """An incoming gradient as the kernel reads it: zeros where autograd passed none, a copy where the strides do not fit."""
    if g is None:
        return torch.zeros_like(like)
    if g.dtype != torch.float32 or (g.shape[1] > 1 and g.stride(1) != 1) or (g.shape[0] > 1 and g.stride(0) < g.shape[1]):
        return g.to(torch.float32).contiguous()
    return g


def _module_device(actor_critic, owner):
    dev = getattr(getattr(actor_critic, "std", None), "device", None)
    if isinstance(dev, torch.device) and dev.type != "cuda":
        raise ValueError(f"{owner}: the module is on {dev}, not on a HIP device (there is no CPU path)")
    return dev


class _Pass:
    """One pass of one pass object: its workspace and call counter, and what drives it: `owner` and `what` (the pass's name in messages:
    "", "RL ", "estimator ", "encoder "), the entry-point prefix, the descriptor builder, the plan and the parameters in gradient order."""

    def __init__(self, owner, what, entry, args, plan, parameters, spec, device):
        self.owner, self.what, self.entry, self.args, self.plan, self.parameters = owner, what, entry, args, plan, parameters
        self.spec, self.device, self.workspace, self.calls = spec, device, None, 0

    def run_forward(self, args, n, heads=None):
        """Plan, grow the workspace, launch, count: the number of this forward call.  `heads`: the member of `args` that holds the workspace,
        where that is not `args` itself."""
        need = int(self.plan(n).workspace_floats)
        if self.workspace is None or self.workspace.numel() < need:
            self.workspace = torch.empty(need, dtype=torch.float32, device=self.device)
        _bind_workspace(args if heads is None else heads, self.workspace, self.device)
        _call(self.entry + "_forward", args, self.device)
        self.calls += 1
        return self.calls

    def run_backward(self, call, make_args):
        if self.calls != call:
            raise RuntimeError(f"{self.owner}: backward of {self.what}forward call {call}, but {self.what}forward call {self.calls} has overwritten "
                               f"its activations in the workspace since; run each backward before the next forward"
                               + (" of the same pass" if self.what else ""))
        grads = [torch.empty_like(p) for p in self.parameters()]
        _call(self.entry + "_backward", make_args(grads), self.device)
        return grads


class _RLFunction(torch.autograd.Function):
    """(mu, sigma, values) of an RL pass `ps` from its inputs; the parameters ride along so that autograd asks for their gradients."""

    @staticmethod
    def forward(ctx, ps, n_inputs, *inputs_and_params):
        inputs, spec, device = inputs_and_params[:n_inputs], ps.spec, ps.device
        n = int(inputs[0].shape[0])
        mu = torch.empty((n, spec.num_actions), dtype=torch.float32, device=device)
        sigma = torch.empty_like(mu)
        values = torch.empty((n, spec.critic.widths[-1]), dtype=torch.float32, device=device)
        args = ps.args(spec, *inputs, mu, sigma, values, None, device=device)      # every refusal before anything grows
        ctx.ps, ctx.inputs, ctx.call = ps, inputs, ps.run_forward(args, n)
        ctx.save_for_backward(mu, sigma, values)
        return mu, sigma, values

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_mu, grad_sigma, grad_values):
        ps = ctx.ps
        mu, sigma, values = ctx.saved_tensors
        gm, gs, gv = _grad_rows(grad_mu, mu), _grad_rows(grad_sigma, sigma), _grad_rows(grad_values, values)
        grads = ps.run_backward(ctx.call, lambda g: ps.args(ps.spec, *ctx.inputs, mu, sigma, values, ps.workspace, g, gm, gs, gv, device=ps.device))
        return (None,) * (2 + len(ctx.inputs)) + tuple(grads)       # nothing for a chain that is no input of this pass


class _LossFunction(torch.autograd.Function):
    """The masked mean-squared error of a loss pass `ps` as a 0-dim tensor."""

    @staticmethod
    def forward(ctx, ps, n_inputs, *inputs_and_params):
        inputs = inputs_and_params[:n_inputs]
        loss = torch.empty((), dtype=torch.float32, device=ps.device)
        args = ps.args(ps.spec, *inputs, loss, None, device=ps.device)
        ctx.ps, ctx.inputs, ctx.call = ps, inputs, ps.run_forward(args, int(inputs[0].shape[0]))
        return loss

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_loss):
        ps = ctx.ps
        up = grad_loss.to(torch.float32).reshape(1).contiguous()        # stays on the device: the kernel reads it there
        grads = ps.run_backward(ctx.call, lambda grads: ps.args(ps.spec, *ctx.inputs, None, ps.workspace, grads, up, device=ps.device))
        return (None,) * (2 + len(ctx.inputs)) + tuple(grads)       # the target's chain carries no gradient


def _apply(fn, ps, *inputs):
    return fn.apply(ps, len(inputs), *inputs, *ps.parameters())


class FusedTrainPass:
    def __init__(self, actor_critic):
        self.device = _module_device(actor_critic, _PLAIN)
        self.spec = describe(actor_critic, self.device)
        self._pass = _Pass(_PLAIN, "", "lg_train", train_args, self.plan, self.spec.parameters, self.spec, self.device)

    def plan(self, n_rows):
        return plan(n_rows, self.spec.actor.widths, self.spec.critic.widths)

    def __call__(self, obs, critic_obs):
        """(mu, sigma, values) of the mini-batch: (B, A), (B, A), (B, 1).  One launch on the current stream."""
        return _apply(_RLFunction, self._pass, obs, critic_obs)


# ---- the explicit-estimator family (include/lgtrainee.h, csrc/lg_train_ee.hip) ----------------------------------------------------------------
class TrainSpecEE:
    """ActorCriticEE as the kernels take it: the estimator, the actor (whose input is [features | estimator output]) and the critic."""

    def __init__(self, estimator, actor, critic, std):
        self.estimator, self.actor, self.critic, self.std = estimator, actor, critic, std
        self.chains = (estimator, actor, critic)
        self.num_actions, self.clip_actions = actor.widths[-1], actor.clip
        self.num_features, self.num_labels = estimator.widths[0], estimator.widths[-1]

    def rl_parameters(self):
        """Actor, critic, then std: the order of PPO_EE.rl_parameters and of the RL pass's gradients."""
        return [p for c in (self.actor, self.critic) for l in c.linears for p in (l.weight, l.bias)] + [self.std]

    def rl_parameter_names(self):
        return [f"{c.name}.{i}.{n}" for c in (self.actor, self.critic) for i in range(len(c.linears)) for n in ("weight", "bias")] + ["std"]

    def estimator_parameters(self):
        return [p for l in self.estimator.linears for p in (l.weight, l.bias)]

    def estimator_parameter_names(self):
        return [f"estimator.{i}.{n}" for i in range(len(self.estimator.linears)) for n in ("weight", "bias")]


def describe_ee(actor_critic, device=None):
    """ActorCriticEE as the kernels take it (duck-typed: .estimator, .actor, .critic, .std), by the rules of `describe` for each chain.
    Refusals are ValueErrors that name the layer or the member."""
    if getattr(actor_critic, "estimator", None) is None:
        raise ValueError("FusedTrainPassEE: the module has no .estimator; the plain ActorCritic is FusedTrainPass's")

    def between(c):
        if c["actor"].widths[0] != c["estimator"].widths[0] + c["estimator"].widths[-1]:
            raise ValueError(f"FusedTrainPassEE: actor[0] takes {c['actor'].widths[0]} inputs, but [features | estimator output] has "
                             f"{c['estimator'].widths[0]} + {c['estimator'].widths[-1]} columns")
    c, std = _describe(actor_critic, device, _EE, [f for f in _OTHER_FAMILIES if f[0] != "estimator"], " beside .estimator; only ActorCriticEE is built",
                       (("estimator", False), ("actor", True), ("critic", False)), between)
    return TrainSpecEE(c["estimator"], c["actor"], c["critic"], std)


def _rl_grads(grads, *chains):
    """`grads` of an RL backward, [chain by chain in `chains` order ..., std], cut per chain; all None in a forward."""
    if grads is None:
        return [None] * (len(chains) + 1)
    cuts, at = [], 0
    for c in chains:
        cuts.append(grads[at:at + 2 * len(c.linears)])
        at += 2 * len(c.linears)
    return cuts + [grads[-1]]


def ee_args(spec, features, critic_obs, mu, sigma, values, workspace, grads=None, grad_mu=None, grad_sigma=None, grad_values=None, device=None):
    """LgTrainEEArgs of one call of the RL pass.  `grads` (backward): the tensors that take the gradients, in spec.rl_parameters() order."""
    a = abi.LgTrainEEArgs()
    if not isinstance(features, torch.Tensor) or features.dim() != 2 or features.shape[0] < 1:
        raise ValueError(f"FusedTrainPassEE: estimator_features must be a (B, {spec.num_features}) float32 tensor with B >= 1")
    n = int(features.shape[0])
    a.n_rows = n
    est, act, cri = a.chain[abi.TRAIN_EE_ESTIMATOR], a.chain[abi.TRAIN_EE_ACTOR], a.chain[abi.TRAIN_EE_CRITIC]
    est.input, est.in_stride = nets.rows(features, spec.num_features, "estimator_features", n, device, _EE)
    cri.input, cri.in_stride = nets.rows(critic_obs, spec.critic.widths[0], "critic_obs", n, device, _EE)
    g_act, g_cri, g_std = _rl_grads(grads, spec.actor, spec.critic)
    _fill_chain(est, spec.estimator, device)
    _fill_chain(act, spec.actor, device, g_act)
    _fill_chain(cri, spec.critic, device, g_cri)
    _fill_heads(a, spec, mu, sigma, values, n, device, _EE, g_std, grad_mu, grad_sigma, grad_values)
    _bind_workspace(a, workspace, device)
    return a


def est_args(spec, features, labels, terminated, loss, workspace, grads=None, upstream=None, device=None):
    """LgTrainEstArgs of one call of the estimator pass.  `grads` (backward): in spec.estimator_parameters() order."""
    a = abi.LgTrainEstArgs()
    if not isinstance(features, torch.Tensor) or features.dim() != 2 or features.shape[0] < 1:
        raise ValueError(f"FusedTrainPassEE: estimator_features must be a (B, {spec.num_features}) float32 tensor with B >= 1")
    n = int(features.shape[0])
    a.n_rows = n
    a.chain.input, a.chain.in_stride = nets.rows(features, spec.num_features, "estimator_features", n, device, _EE)
    _fill_chain(a.chain, spec.estimator, device, grads)
    a.labels, a.labels_stride = nets.rows(labels, spec.num_labels, "estimator_labels", n, device, _EE)
    a.mask, a.mask_stride = nets.rows(terminated, 1, "terminated", n, device, _EE)
    if loss is not None:
        a.loss = _scalar(loss, "the loss", device)
    if upstream is not None:
        a.upstream = _scalar(upstream, "the upstream gradient", device)
    _bind_workspace(a, workspace, device)
    return a


def plan_ee(n_rows, estimator_widths, actor_widths, critic_widths):
    """LgTrainEEPlan of the RL pass (lg_train_ee_plan) for chains of these widths."""
    return _plan("lg_train_ee_plan", abi.LgTrainEEArgs, abi.LgTrainEEPlan, n_rows, ((0, estimator_widths), (1, actor_widths), (2, critic_widths)))


def plan_est(n_rows, estimator_widths):
    """LgTrainEEPlan of the estimator pass (lg_train_est_plan)."""
    return _plan("lg_train_est_plan", abi.LgTrainEstArgs, abi.LgTrainEEPlan, n_rows, ((None, estimator_widths),))


class FusedTrainPassEE:
    """The two network passes of PPO_EE.update() on an ActorCriticEE (include/lgtrainee.h):

        tp = FusedTrainPassEE(actor_critic_ee)
        mu, sigma, values = tp(estimator_features, critic_obs)                        # RL step: one launch; backward three
        est_loss = tp.estimator_loss(estimator_features, estimator_labels, terminated)       # estimator step: two launches; backward three

    Optimise tp.rl_parameters() (actor, critic, std: the reference's order) and tp.estimator_parameters() apart.  The RL pass gives the
    estimator's parameters no gradient (their .grad is left as it was): the reference discards that gradient unread, and there is no
    end-to-end estimator gradient from the RL loss.  Each pass has its own workspace and call counter: a forward of one does not
    invalidate a pending backward of the other; within a pass a backward whose forward has been overwritten raises."""

    def __init__(self, actor_critic):
        self.device = _module_device(actor_critic, _EE)
        self.spec = describe_ee(actor_critic, self.device)
        self._rl = _Pass(_EE, "RL ", "lg_train_ee", ee_args, self.plan, self.rl_parameters, self.spec, self.device)
        self._est = _Pass(_EE, "estimator ", "lg_train_est", est_args, self.estimator_plan, self.estimator_parameters, self.spec, self.device)

    def rl_parameters(self):
        return self.spec.rl_parameters()

    def estimator_parameters(self):
        return self.spec.estimator_parameters()

    def plan(self, n_rows):
        s = self.spec
        return plan_ee(n_rows, s.estimator.widths, s.actor.widths, s.critic.widths)

    def estimator_plan(self, n_rows):
        return plan_est(n_rows, self.spec.estimator.widths)

    def __call__(self, estimator_features, critic_obs):
        """(mu, sigma, values) of the mini-batch: (B, A), (B, A), (B, 1).  One launch on the current stream."""
        return _apply(_RLFunction, self._rl, estimator_features, critic_obs)

    def estimator_loss(self, estimator_features, estimator_labels, terminated):
        """mse_loss(estimator(features) * terminated, labels * terminated) as a 0-dim tensor with autograd.  Two launches."""
        return _apply(_LossFunction, self._est, estimator_features, estimator_labels, terminated)


# ---- the teacher-student family (include/lgtraints.h, csrc/lg_train_ts.hip) -------------------------------------------------------------------
_TS_FOREIGN = (("estimator", "ActorCriticEE"), ("vae", "ActorCriticDreamWaQ"), ("memory_a", "ActorCriticRecurrent"), ("memory_c", "ActorCriticRecurrent"))


class TrainSpecTS:
    """ActorCriticTS as the kernels take it: the privilege encoder, the actor (whose input is [obs | latent]), the critic and the history
    encoder."""

    def __init__(self, privilege_encoder, actor, critic, history_encoder, std):
        self.privilege_encoder, self.actor, self.critic, self.history_encoder, self.std = privilege_encoder, actor, critic, history_encoder, std
        self.chains = (privilege_encoder, actor, critic, history_encoder)          # abi.TRAIN_TS_* order
        self.num_actions, self.clip_actions = actor.widths[-1], actor.clip
        self.num_latent = privilege_encoder.widths[-1]
        self.num_obs = actor.widths[0] - self.num_latent

    def rl_parameters(self):
        """Actor, critic, privilege encoder, then std: the order of PPO_TS.rl_parameters and of the RL pass's gradients."""
        return [p for c in (self.actor, self.critic, self.privilege_encoder) for l in c.linears for p in (l.weight, l.bias)] + [self.std]

    def rl_parameter_names(self):
        return [f"{c.name}.{i}.{n}" for c in (self.actor, self.critic, self.privilege_encoder) for i in range(len(c.linears))
                for n in ("weight", "bias")] + ["std"]

    def encoder_parameters(self):
        return [p for l in self.history_encoder.linears for p in (l.weight, l.bias)]

    def encoder_parameter_names(self):
        return [f"history_encoder.{i}.{n}" for i in range(len(self.history_encoder.linears)) for n in ("weight", "bias")]


def _describe_ts(actor_critic, device, owner, family):
    """describe_ts's rules under `owner`'s name; `family`: the module class the refusals speak of."""
    for need in ("privilege_encoder", "history_encoder"):
        if getattr(actor_critic, need, None) is None:
            raise ValueError(f"{owner}: the module has no .{need}; {family} has a privilege encoder and a history encoder")

    def between(c):
        hist, priv, actor = c["history_encoder"], c["privilege_encoder"], c["actor"]
        if hist.widths[-1] != priv.widths[-1]:
            raise ValueError(f"{owner}: history_encoder ends at {hist.widths[-1]} columns, privilege_encoder at {priv.widths[-1]}: the "
                             f"latent widths differ")
        if actor.widths[0] <= priv.widths[-1]:
            raise ValueError(f"{owner}: actor[0] takes {actor.widths[0]} inputs, but [obs | latent] has O + {priv.widths[-1]} columns with "
                             f"O >= 1")
    c, std = _describe(actor_critic, device, owner, _TS_FOREIGN, f" beside its encoders; only {family} is built",
                       (("privilege_encoder", False), ("history_encoder", False), ("actor", True), ("critic", False)), between)
    return TrainSpecTS(c["privilege_encoder"], c["actor"], c["critic"], c["history_encoder"], std)


def describe_ts(actor_critic, device=None):
    """ActorCriticTS as the kernels take it (duck-typed: .privilege_encoder, .history_encoder, .actor, .critic, .std), by the rules of
    `describe` for each of the four chains: a Conv1d / Flatten "TCN" history encoder is refused by its layer's name.  Refusals are
    ValueErrors that name the layer or the member."""
    return _describe_ts(actor_critic, device, _TS, "ActorCriticTS")


def ts_args(spec, obs, privileged_obs, critic_obs, mu, sigma, values, workspace, grads=None, grad_mu=None, grad_sigma=None, grad_values=None,
            device=None, owner=_TS):
    """LgTrainTSArgs of one call of the RL pass.  `grads` (backward): the tensors that take the gradients, in spec.rl_parameters() order
    (actor, critic, privilege encoder, std)."""
    a = abi.LgTrainTSArgs()
    if not isinstance(obs, torch.Tensor) or obs.dim() != 2 or obs.shape[0] < 1:
        raise ValueError(f"{owner}: obs must be a (B, O) float32 tensor with B >= 1 and O = actor[0].in_features - {spec.num_latent}")
    n = int(obs.shape[0])
    if obs.shape[1] + spec.num_latent != spec.actor.widths[0]:
        raise ValueError(f"{owner}: actor[0] takes {spec.actor.widths[0]} inputs, but [obs | latent] has {obs.shape[1]} + "
                         f"{spec.num_latent} columns")
    a.n_rows, a.n_obs = n, spec.num_obs
    pri, act, cri = a.chain[abi.TRAIN_TS_PRIVILEGE], a.chain[abi.TRAIN_TS_ACTOR], a.chain[abi.TRAIN_TS_CRITIC]
    act.input, act.in_stride = nets.rows(obs, spec.num_obs, "obs", n, device, owner)
    pri.input, pri.in_stride = nets.rows(privileged_obs, spec.privilege_encoder.widths[0], "privileged_obs", n, device, owner)
    cri.input, cri.in_stride = nets.rows(critic_obs, spec.critic.widths[0], "critic_obs", n, device, owner)
    g_act, g_cri, g_pri, g_std = _rl_grads(grads, spec.actor, spec.critic, spec.privilege_encoder)
    _fill_chain(act, spec.actor, device, g_act)
    _fill_chain(cri, spec.critic, device, g_cri)
    _fill_chain(pri, spec.privilege_encoder, device, g_pri)
    _fill_heads(a, spec, mu, sigma, values, n, device, owner, g_std, grad_mu, grad_sigma, grad_values)
    _bind_workspace(a, workspace, device, owner)
    return a


def enc_args(spec, obs_history, privileged_obs, terminated, loss, workspace, grads=None, upstream=None, device=None, owner=_TS):
    """LgTrainEncArgs of one call of the encoder pass.  `grads` (backward): in spec.encoder_parameters() order.  The privilege encoder's
    gradient pointers stay null: the pass has no use for them."""
    a = abi.LgTrainEncArgs()
    if not isinstance(obs_history, torch.Tensor) or obs_history.dim() != 2 or obs_history.shape[0] < 1:
        raise ValueError(f"{owner}: obs_history must be a (B, {spec.history_encoder.widths[0]}) float32 tensor with B >= 1")
    n = int(obs_history.shape[0])
    a.n_rows = n
    his, pri = a.chain[abi.TRAIN_ENC_HISTORY], a.chain[abi.TRAIN_ENC_PRIVILEGE]
    his.input, his.in_stride = nets.rows(obs_history, spec.history_encoder.widths[0], "obs_history", n, device, owner)
    pri.input, pri.in_stride = nets.rows(privileged_obs, spec.privilege_encoder.widths[0], "privileged_obs", n, device, owner)
    _fill_chain(his, spec.history_encoder, device, grads)
    _fill_chain(pri, spec.privilege_encoder, device)
    a.mask, a.mask_stride = nets.rows(terminated, 1, "terminated", n, device, owner)
    if loss is not None:
        a.loss = _scalar(loss, "the loss", device, 1, owner)
    if upstream is not None:
        a.upstream = _scalar(upstream, "the upstream gradient", device, 1, owner)
    _bind_workspace(a, workspace, device, owner)
    return a


def plan_ts(n_rows, privilege_widths, actor_widths, critic_widths):
    """LgTrainTSPlan of the RL pass (lg_train_ts_plan) for chains of these widths; O is actor_widths[0] less the latent width."""
    return _plan("lg_train_ts_plan", abi.LgTrainTSArgs, abi.LgTrainTSPlan, n_rows, ((0, privilege_widths), (1, actor_widths), (2, critic_widths)),
                 n_obs=int(actor_widths[0]) - int(privilege_widths[-1]))


def plan_enc(n_rows, history_widths, privilege_widths):
    """LgTrainTSPlan of the encoder pass (lg_train_enc_plan)."""
    return _plan("lg_train_enc_plan", abi.LgTrainEncArgs, abi.LgTrainTSPlan, n_rows,
                 ((abi.TRAIN_ENC_HISTORY, history_widths), (abi.TRAIN_ENC_PRIVILEGE, privilege_widths)))


class FusedTrainPassTS:
    """The two network passes of PPO_TS.update() on an ActorCriticTS (include/lgtraints.h):

        tp = FusedTrainPassTS(actor_critic_ts)
        mu, sigma, values = tp(obs, privileged_obs, critic_obs)                   # RL step: one launch; backward three
        enc_loss = tp.encoder_loss(obs_history, privileged_obs, terminated)       # encoder step: two launches; backward three

    Optimise tp.rl_parameters() (actor, critic, privilege encoder, std: the reference's order) and tp.encoder_parameters() (the history
    encoder) apart.  The RL gradient reaches the privilege encoder through the latent columns of the actor's input; the history encoder
    takes no part in the RL pass and its .grad is left as it was.  The encoder pass takes its targets from the privilege encoder with no
    gradient: that encoder's .grad is left as it was.  Each pass has its own workspace and call counter: a forward of one does not
    invalidate a pending backward of the other; within a pass a backward whose forward has been overwritten raises.  The actor may end in a
    Hardtanh or not (ActorCriticTS has none).

    This is PPO_TS's update only.  ActorCriticCTS has the same members, but PPO_CTS updates two env groups with other losses: that is
    FusedTrainPassCTS.  A "TCN" (Conv1d) history encoder is refused by layer name here: its passes are FusedTrainPassTSTcn."""

    def __init__(self, actor_critic):
        self.device = _module_device(actor_critic, _TS)
        self.spec = describe_ts(actor_critic, self.device)
        self._rl = _Pass(_TS, "RL ", "lg_train_ts", ts_args, self.plan, self.rl_parameters, self.spec, self.device)
        self._enc = _Pass(_TS, "encoder ", "lg_train_enc", enc_args, self.encoder_plan, self.encoder_parameters, self.spec, self.device)

    def rl_parameters(self):
        return self.spec.rl_parameters()

    def encoder_parameters(self):
        return self.spec.encoder_parameters()

    def plan(self, n_rows):
        s = self.spec
        return plan_ts(n_rows, s.privilege_encoder.widths, s.actor.widths, s.critic.widths)

    def encoder_plan(self, n_rows):
        return plan_enc(n_rows, self.spec.history_encoder.widths, self.spec.privilege_encoder.widths)

    def __call__(self, obs, privileged_obs, critic_obs):
        """(mu, sigma, values) of the mini-batch: (B, A), (B, A), (B, 1).  One launch on the current stream."""
        return _apply(_RLFunction, self._rl, obs, privileged_obs, critic_obs)

    def encoder_loss(self, obs_history, privileged_obs, terminated):
        """mse_loss(history_encoder(obs_history) * terminated, privilege_encoder(privileged_obs).detach() * terminated) as a 0-dim tensor
        with autograd.  Two launches."""
        return _apply(_LossFunction, self._enc, obs_history, privileged_obs, terminated)


# ---- ActorCriticTS with a "TCN" history encoder (include/lgtraintcn.h, csrc/lg_train_tcn.hip) ------------------------------------------------
_TCN = "FusedTrainPassTSTcn"


class TrainSpecTSTcn:
    """ActorCriticTS with history_encoder_type = "TCN" as the kernels take it: the privilege encoder, the actor and the critic as
    TrainSpecTS has them (the RL pass is the same), and the history encoder as a nets.TcnSpec."""

    def __init__(self, privilege_encoder, actor, critic, history_encoder, std):
        self.privilege_encoder, self.actor, self.critic, self.history_encoder, self.std = privilege_encoder, actor, critic, history_encoder, std
        self.num_actions, self.clip_actions = actor.widths[-1], actor.clip
        self.num_latent = privilege_encoder.widths[-1]
        self.num_obs = actor.widths[0] - self.num_latent

    rl_parameters, rl_parameter_names = TrainSpecTS.rl_parameters, TrainSpecTS.rl_parameter_names

    def encoder_parameters(self):
        """In history_encoder.parameters() order: every conv's weight and bias, then the tail's."""
        return self.history_encoder.parameters()

    def encoder_parameter_names(self):
        h = self.history_encoder
        at = [i for i in range(len(h.convs))] + [len(h.convs) + 1 + 2 * j for j in range(len(h.tail.linears))]      # ELU behind every tail layer but the last
        return [f"history_encoder.{i}.{n}" for i in at for n in ("weight", "bias")]


def describe_ts_tcn(actor_critic, device=None, n_history=None):
    """ActorCriticTS with a Conv1d+ / Flatten / Linear-ELU history encoder, by describe_ts's rules for the other three chains and
    nets.describe_tcn's for the history encoder; with `n_history` (H, which the module does not record) the lengths are checked too.  A
    module whose history encoder is an MLP is FusedTrainPassTS's."""
    for need in ("privilege_encoder", "history_encoder"):
        if getattr(actor_critic, need, None) is None:
            raise ValueError(f"{_TCN}: the module has no .{need}; ActorCriticTS has a privilege encoder and a history encoder")
    he = actor_critic.history_encoder
    if isinstance(he, nn.Sequential) and not any(isinstance(m, (nn.Conv1d, nn.Flatten)) for m in he):
        raise ValueError(f"{_TCN}: history_encoder has no Conv1d layer: it is an MLP, which FusedTrainPassTS builds")

    def between(c):
        if c["actor"].widths[0] <= c["privilege_encoder"].widths[-1]:
            raise ValueError(f"{_TCN}: actor[0] takes {c['actor'].widths[0]} inputs, but [obs | latent] has O + {c['privilege_encoder'].widths[-1]} "
                             f"columns with O >= 1")
    c, std = _describe(actor_critic, device, _TCN, _TS_FOREIGN, " beside its encoders; only ActorCriticTS is built",
                       (("privilege_encoder", False), ("actor", True), ("critic", False)), between)
    tcn = nets.describe_tcn("history_encoder", he, device, _TCN, n_history)
    if tcn.tail.widths[-1] != c["privilege_encoder"].widths[-1]:
        raise ValueError(f"{_TCN}: history_encoder ends at {tcn.tail.widths[-1]} columns, privilege_encoder at {c['privilege_encoder'].widths[-1]}: the "
                         f"latent widths differ")
    return TrainSpecTSTcn(c["privilege_encoder"], c["actor"], c["critic"], tcn, std)


def _history_rows(obs_history, owner):
    """obs_history as (B, H) rows: (B, H) itself, or the (B, 1, H) the reference hands its Conv1d stack (ppo_ts.py:176-178), in place."""
    if isinstance(obs_history, torch.Tensor) and obs_history.dim() == 3 and obs_history.shape[1] == 1:
        obs_history = obs_history[:, 0, :]
    if not isinstance(obs_history, torch.Tensor) or obs_history.dim() != 2 or obs_history.shape[0] < 1:
        raise ValueError(f"{owner}: obs_history must be a (B, H) or (B, 1, H) float32 tensor with B >= 1")
    return obs_history


def tcn_args(spec, obs_history, privileged_obs, terminated, loss, workspace, grads=None, upstream=None, device=None):
    """LgTrainTcnArgs of one call of the encoder pass.  `grads` (backward): in spec.encoder_parameters() order.  The privilege encoder's
    gradient pointers stay null."""
    a = abi.LgTrainTcnArgs()
    obs_history = _history_rows(obs_history, _TCN)
    n, H = int(obs_history.shape[0]), int(obs_history.shape[1])
    tcn = spec.history_encoder
    tcn.lengths(H)
    a.n_rows, a.n_history, a.n_conv = n, H, len(tcn.convs)
    a.history, a.history_stride = nets.rows(obs_history, H, "obs_history", n, device, _TCN)
    for l, (m, shape) in enumerate(zip(tcn.convs, tcn.shapes)):
        v = a.conv[l]
        nets.check_tensor(m.weight, f"history_encoder[{l}].weight", device, _TCN)
        nets.check_tensor(m.bias, f"history_encoder[{l}].bias", device, _TCN)
        v.weight, v.bias = m.weight.data_ptr(), m.bias.data_ptr()
        v.c_in, v.c_out, v.kernel, v.stride, v.padding, v.dilation = shape
        if grads is not None:
            v.grad_weight, v.grad_bias = grads[2 * l].data_ptr(), grads[2 * l + 1].data_ptr()
    a.privilege.input, a.privilege.in_stride = nets.rows(privileged_obs, spec.privilege_encoder.widths[0], "privileged_obs", n, device, _TCN)
    _fill_chain(a.tail, tcn.tail, device, None if grads is None else grads[2 * len(tcn.convs):])
    _fill_chain(a.privilege, spec.privilege_encoder, device)
    a.mask, a.mask_stride = nets.rows(terminated, 1, "terminated", n, device, _TCN)
    if loss is not None:
        a.loss = _scalar(loss, "the loss", device, 1, _TCN)
    if upstream is not None:
        a.upstream = _scalar(upstream, "the upstream gradient", device, 1, _TCN)
    _bind_workspace(a, workspace, device, _TCN)
    return a


def plan_tcn(n_rows, n_history, convs, tail_widths, privilege_widths):
    """LgTrainTcnPlan (lg_train_tcn_plan) for n_rows histories of length n_history; `convs`: (c_in, c_out, kernel, stride, padding,
    dilation) per layer; the chains' widths as [in, out_0, ...]."""
    key = ("lg_train_tcn_plan", int(n_rows), int(n_history), tuple(tuple(int(x) for x in c) for c in convs), tuple(int(x) for x in tail_widths),
           tuple(int(x) for x in privilege_widths))
    if key not in _PLANS:
        lib, a, p = abi.load_lib(), abi.LgTrainTcnArgs(), abi.LgTrainTcnPlan()
        a.n_rows, a.n_history, a.n_conv = key[1], key[2], len(key[3])
        for v, c in zip(a.conv, key[3]):
            v.c_in, v.c_out, v.kernel, v.stride, v.padding, v.dilation = c
        _widths_into(a.tail, key[4])
        _widths_into(a.privilege, key[5])
        abi.check(lib.lg_train_tcn_plan(C.byref(a), C.byref(p)), lib)
        _PLANS[key] = p
    return _PLANS[key]


class _TcnLossFunction(torch.autograd.Function):
    """_LossFunction for the TCN encoder pass, whose plan takes the history length beside the row count."""

    @staticmethod
    def forward(ctx, ps, n_inputs, *inputs_and_params):
        inputs = inputs_and_params[:n_inputs]
        loss = torch.empty((), dtype=torch.float32, device=ps.device)
        args = ps.args(ps.spec, *inputs, loss, None, device=ps.device)
        ctx.ps, ctx.inputs, ctx.call = ps, inputs, ps.run_forward(args, (int(args.n_rows), int(args.n_history)))
        return loss

    backward = _LossFunction.backward


class FusedTrainPassTSTcn:
    """The two network passes of PPO_TS.update() on an ActorCriticTS built with history_encoder_type = "TCN" (include/lgtraintcn.h):

        tp = FusedTrainPassTSTcn(actor_critic_ts)
        mu, sigma, values = tp(obs, privileged_obs, critic_obs)                   # RL step: FusedTrainPassTS's, unchanged
        enc_loss = tp.encoder_loss(obs_history, privileged_obs, terminated)       # encoder step: three launches; backward five

    The RL pass is lg_train_ts_forward / _backward as FusedTrainPassTS runs it: PPO_TS's RL step never runs the history encoder.  The
    encoder pass carries obs_history, (B, H) or the (B, 1, H) the reference unsqueezes it to, through the Conv1d stack, the Flatten and the
    Linear / ELU tail, against the privilege encoder's output as a constant.  Optimise tp.rl_parameters() and tp.encoder_parameters() (in
    history_encoder.parameters() order) apart.  Each pass has its own workspace and call counter; within a pass a backward whose forward
    has been overwritten raises.  H is fixed by the first encoder_loss call unless `n_history` is given.  The rollout of such a module is
    FusedPolicy(actor_critic, student=False): act_student through the TCN stays on torch."""

    def __init__(self, actor_critic, n_history=None):
        self.device = _module_device(actor_critic, _TCN)
        self.spec = describe_ts_tcn(actor_critic, self.device, n_history)
        self.n_history = None if n_history is None else int(n_history)
        rl_args = lambda *a, **kw: ts_args(*a, owner=_TCN, **kw)
        self._rl = _Pass(_TCN, "RL ", "lg_train_ts", rl_args, self.plan, self.rl_parameters, self.spec, self.device)
        self._enc = _Pass(_TCN, "encoder ", "lg_train_tcn", tcn_args, lambda sizes: self._plan_encoder(*sizes), self.encoder_parameters, self.spec, self.device)

    def rl_parameters(self):
        return self.spec.rl_parameters()

    def encoder_parameters(self):
        return self.spec.encoder_parameters()

    @property
    def workspace(self):
        """The float32 workspace of the last encoder forward, laid out by its plan (LgTrainTcnPlan's offsets); None before the first call.
        For reading only: the next encoder forward overwrites or replaces it."""
        return self._enc.workspace

    def plan(self, n_rows):
        s = self.spec
        return plan_ts(n_rows, s.privilege_encoder.widths, s.actor.widths, s.critic.widths)

    def _plan_encoder(self, n_rows, n_history):
        s = self.spec
        return plan_tcn(n_rows, n_history, s.history_encoder.shapes, s.history_encoder.tail.widths, s.privilege_encoder.widths)

    def plan_encoder(self, n_rows):
        if self.n_history is None:
            raise ValueError(f"{_TCN}: the history length is not known yet: pass n_history, or call encoder_loss first")
        return self._plan_encoder(n_rows, self.n_history)

    def __call__(self, obs, privileged_obs, critic_obs):
        """(mu, sigma, values) of the mini-batch: (B, A), (B, A), (B, 1).  One launch on the current stream."""
        return _apply(_RLFunction, self._rl, obs, privileged_obs, critic_obs)

    def encoder_loss(self, obs_history, privileged_obs, terminated):
        """mse_loss(history_encoder(obs_history) * terminated, privilege_encoder(privileged_obs).detach() * terminated) as a 0-dim tensor
        with autograd.  Three launches."""
        obs_history = _history_rows(obs_history, _TCN)
        H = int(obs_history.shape[1])
        if self.n_history is not None and H != self.n_history:
            raise ValueError(f"{_TCN}: obs_history has {H} columns, this pass was set up for H = {self.n_history}")
        self.spec.history_encoder.lengths(H)
        self.n_history = H
        return _apply(_TcnLossFunction, self._enc, obs_history, privileged_obs, terminated)


# ---- the concurrent teacher-student family (include/lgtraincts.h, csrc/lg_train_cts.hip) --------------------------------------------------------
def describe_cts(actor_critic, device=None):
    """ActorCriticCTS as the kernels take it: describe_ts's rules (the module has the same members) under FusedTrainPassCTS's name.  A
    Conv1d / Flatten "TCN" history encoder is refused by its layer's name."""
    return _describe_ts(actor_critic, device, _CTS, "ActorCriticCTS")


def cts_args(spec, teacher_obs, teacher_privileged_obs, student_obs, student_obs_history, critic_obs, mu_t, sigma_t, mu_s, sigma_s, values, workspace,
             grads=None, grad_mu_t=None, grad_sigma_t=None, grad_mu_s=None, grad_sigma_s=None, grad_values=None, device=None):
    """LgTrainCTSArgs of one call of the RL pass.  `grads` (backward): the tensors that take the gradients, in spec.rl_parameters() order
    (actor, critic, privilege encoder, std).  The history encoder's gradient pointers stay null: the pass has no use for them."""
    a = abi.LgTrainCTSArgs()
    for x, what in ((teacher_obs, "teacher_obs"), (student_obs, "student_obs"), (critic_obs, "critic_obs")):
        if not isinstance(x, torch.Tensor) or x.dim() != 2 or x.shape[0] < 1:
            raise ValueError(f"{_CTS}: {what} must be a (B, {spec.critic.widths[0] if what == 'critic_obs' else spec.num_obs}) float32 tensor with B >= 1")
    nt, ns, nc = int(teacher_obs.shape[0]), int(student_obs.shape[0]), int(critic_obs.shape[0])
    a.n_teacher, a.n_student, a.n_critic, a.n_obs = nt, ns, nc, spec.num_obs
    A, V = spec.num_actions, spec.critic.widths[-1]
    T, S = abi.TRAIN_CTS_TEACHER, abi.TRAIN_CTS_STUDENT
    pri, act, cri, his = (a.chain[i] for i in (abi.TRAIN_CTS_PRIVILEGE, abi.TRAIN_CTS_ACTOR, abi.TRAIN_CTS_CRITIC, abi.TRAIN_CTS_HISTORY))
    act.input, act.in_stride = nets.rows(teacher_obs, spec.num_obs, "teacher_obs", nt, device, _CTS)
    pri.input, pri.in_stride = nets.rows(teacher_privileged_obs, spec.privilege_encoder.widths[0], "teacher_privileged_obs", nt, device, _CTS)
    a.student_obs, a.student_obs_stride = nets.rows(student_obs, spec.num_obs, "student_obs", ns, device, _CTS)
    his.input, his.in_stride = nets.rows(student_obs_history, spec.history_encoder.widths[0], "student_obs_history", ns, device, _CTS)
    cri.input, cri.in_stride = nets.rows(critic_obs, spec.critic.widths[0], "critic_obs", nc, device, _CTS)
    g_act, g_cri, g_pri, g_std = _rl_grads(grads, spec.actor, spec.critic, spec.privilege_encoder)
    _fill_chain(act, spec.actor, device, g_act)
    _fill_chain(cri, spec.critic, device, g_cri)
    _fill_chain(pri, spec.privilege_encoder, device, g_pri)
    _fill_chain(his, spec.history_encoder, device)
    a.clip_on, a.clip_actions = (1, spec.clip_actions) if spec.clip_actions is not None else (0, 0.0)
    nets.check_tensor(spec.std, "std", device, _CTS)
    a.std = spec.std.data_ptr()
    for g, n, mu, sigma, tag in ((T, nt, mu_t, sigma_t, "teacher"), (S, ns, mu_s, sigma_s, "student")):
        a.mu[g], a.mu_stride[g] = nets.rows(mu, A, f"{tag} mu", n, device, _CTS)
        a.sigma[g], a.sigma_stride[g] = nets.rows(sigma, A, f"{tag} sigma", n, device, _CTS)
    a.values, a.values_stride = nets.rows(values, V, "values", nc, device, _CTS)
    if grads is not None:
        a.grad_std = g_std.data_ptr()
        for g, n, gm, gs, tag in ((T, nt, grad_mu_t, grad_sigma_t, "teacher"), (S, ns, grad_mu_s, grad_sigma_s, "student")):
            a.grad_mu[g], a.grad_mu_stride[g] = nets.rows(gm, A, f"{tag} grad_mu", n, device, _CTS)
            a.grad_sigma[g], a.grad_sigma_stride[g] = nets.rows(gs, A, f"{tag} grad_sigma", n, device, _CTS)
        a.grad_values, a.grad_values_stride = nets.rows(grad_values, V, "grad_values", nc, device, _CTS)
    _bind_workspace(a, workspace, device, _CTS)
    return a


def plan_cts(n_teacher, n_student, n_critic, privilege_widths, actor_widths, critic_widths, history_widths):
    """LgTrainCTSPlan of the RL pass (lg_train_cts_plan) for chains of these widths; O is actor_widths[0] less the latent width."""
    key = ("lg_train_cts_plan", int(n_teacher), int(n_student), int(n_critic)) + tuple(tuple(int(x) for x in w) for w in
                                                                                       (privilege_widths, actor_widths, critic_widths, history_widths))
    if key not in _PLANS:
        lib, a, p = abi.load_lib(), abi.LgTrainCTSArgs(), abi.LgTrainCTSPlan()
        a.n_teacher, a.n_student, a.n_critic = key[1:4]
        for i, w in zip((abi.TRAIN_CTS_PRIVILEGE, abi.TRAIN_CTS_ACTOR, abi.TRAIN_CTS_CRITIC, abi.TRAIN_CTS_HISTORY), key[4:]):
            _widths_into(a.chain[i], w)
        a.n_obs = int(actor_widths[0]) - int(privilege_widths[-1])
        abi.check(lib.lg_train_cts_plan(C.byref(a), C.byref(p)), lib)
        _PLANS[key] = p
    return _PLANS[key]


class _CTSFunction(torch.autograd.Function):
    """(teacher mu, teacher sigma, student mu, student sigma, values) of the RL pass `ps` from its five inputs; the parameters ride along so
    that autograd asks for their gradients."""

    @staticmethod
    def forward(ctx, ps, n_inputs, *inputs_and_params):
        inputs, spec, device = inputs_and_params[:n_inputs], ps.spec, ps.device
        n = tuple(int(x.shape[0]) if isinstance(x, torch.Tensor) and x.dim() == 2 else 0 for x in (inputs[0], inputs[2], inputs[4]))
        new = lambda rows, w: torch.empty((max(rows, 1), w), dtype=torch.float32, device=device)
        A = spec.num_actions
        outs = (new(n[0], A), new(n[0], A), new(n[1], A), new(n[1], A), new(n[2], spec.critic.widths[-1]))
        args = ps.args(spec, *inputs, *outs, None, device=device)      # every refusal before anything grows
        ctx.ps, ctx.inputs, ctx.call = ps, inputs, ps.run_forward(args, n)
        ctx.save_for_backward(*outs)
        return outs

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, *cotangents):
        ps, outs = ctx.ps, ctx.saved_tensors
        gs = [_grad_rows(g, like) for g, like in zip(cotangents, outs)]
        grads = ps.run_backward(ctx.call, lambda g: ps.args(ps.spec, *ctx.inputs, *outs, ps.workspace, g, *gs, device=ps.device))
        return (None,) * (2 + len(ctx.inputs)) + tuple(grads)


class FusedTrainPassCTS:
    """The two network passes of PPO_CTS.update() on an ActorCriticCTS (include/lgtraincts.h):

        tp = FusedTrainPassCTS(actor_critic_cts)
        mu_t, sigma_t, mu_s, sigma_s, values = tp(teacher_obs, teacher_privileged_obs, student_obs, student_obs_history, critic_obs)
        out = loss_fn.cts(teacher=dict(mu=mu_t, sigma=sigma_t, ...), student=dict(mu=mu_s, sigma=sigma_s, ...), values=values, ...)
        enc_loss = tp.encoder_loss(student_obs_history, student_privileged_obs)      # encoder step: two launches; backward three

    The RL forward is one launch over the teacher's, the student's and the critic's rows (three independent row counts), its backward
    three.  Optimise tp.rl_parameters() (actor, critic, privilege encoder, std: PPO_CTS.rl_params' order) and tp.encoder_parameters()
    (the history encoder) apart.  The RL gradient reaches the privilege encoder through the latent columns of the teacher rows; the student
    rows' latent is a constant of the RL pass and the history encoder's .grad is left as it was.  Torch does accumulate an RL gradient
    there, which the reference zeroes before the only optimizer that owns those parameters steps: the parameters after every step are the
    reference's, that .grad is not.  The encoder pass is mse_loss(history_encoder(h), privilege_encoder(p).detach()) on the teacher-student
    family's encoder kernels with a column of ones, which the pass owns, as the mask; it leaves the privilege encoder's .grad as it was.
    Each pass has its own workspace and call counter: a forward of one does not invalidate a pending backward of the other; within a pass a
    backward whose forward has been overwritten raises.  The actor may end in a Hardtanh or not.  A "TCN" (Conv1d) history encoder is
    refused by layer name: ActorCriticCTS has no such option in the reference (ActorCriticTS has: FusedTrainPassTSTcn)."""

    def __init__(self, actor_critic):
        self.device = _module_device(actor_critic, _CTS)
        self.spec = describe_cts(actor_critic, self.device)
        self._ones = None
        self._rl = _Pass(_CTS, "RL ", "lg_train_cts", cts_args, lambda n: self.plan(*n), self.rl_parameters, self.spec, self.device)
        self._enc = _Pass(_CTS, "encoder ", "lg_train_enc", self._enc_args, self.encoder_plan, self.encoder_parameters, self.spec, self.device)

    def rl_parameters(self):
        return self.spec.rl_parameters()

    def encoder_parameters(self):
        return self.spec.encoder_parameters()

    def plan(self, n_teacher, n_student, n_critic):
        s = self.spec
        return plan_cts(n_teacher, n_student, n_critic, s.privilege_encoder.widths, s.actor.widths, s.critic.widths, s.history_encoder.widths)

    def encoder_plan(self, n_rows):
        return plan_enc(n_rows, self.spec.history_encoder.widths, self.spec.privilege_encoder.widths)

    def _enc_args(self, spec, obs_history, privileged_obs, loss, workspace, grads=None, upstream=None, device=None):
        """enc_args with the pass's own ones column as the mask: grow-only, filled when it grows."""
        ones = None
        if isinstance(obs_history, torch.Tensor) and obs_history.dim() == 2 and obs_history.shape[0] >= 1:
            n = int(obs_history.shape[0])
            if self._ones is None or self._ones.shape[0] < n:
                self._ones = torch.ones((n, 1), dtype=torch.float32, device=self.device)
            ones = self._ones[:n]
        return enc_args(spec, obs_history, privileged_obs, ones, loss, workspace, grads, upstream, device=device, owner=_CTS)

    def __call__(self, teacher_obs, teacher_privileged_obs, student_obs, student_obs_history, critic_obs):
        """(mu_t, sigma_t, mu_s, sigma_s, values): (Bt, A), (Bt, A), (Bs, A), (Bs, A), (Bc, 1).  One launch on the current stream."""
        return _apply(_CTSFunction, self._rl, teacher_obs, teacher_privileged_obs, student_obs, student_obs_history, critic_obs)

    def encoder_loss(self, student_obs_history, student_privileged_obs):
        """mse_loss(history_encoder(student_obs_history), privilege_encoder(student_privileged_obs).detach()) as a 0-dim tensor with
        autograd.  Two launches."""
        return _apply(_LossFunction, self._enc, student_obs_history, student_privileged_obs)


# ---- the DreamWaQ family (include/lgtraindwaq.h, csrc/lg_train_dwaq.hip) ------------------------------------------------------------------------
_DWAQ_FOREIGN = (("estimator", "ActorCriticEE"), ("privilege_encoder", "ActorCriticTS / ActorCriticCTS"),
                 ("history_encoder", "ActorCriticTS / ActorCriticCTS"), ("memory_a", "ActorCriticRecurrent"), ("memory_c", "ActorCriticRecurrent"))


class TrainSpecDreamWaQ:
    """ActorCriticDreamWaQ as the kernels take it: the VAE's encoder (every Linear behind an ELU, the last too), its four one-layer heads,
    its decoder, the actor (whose input is [obs | z | v]) and the critic."""

    def __init__(self, encoder, heads, decoder, actor, critic, std, var_clip):
        self.encoder, self.heads, self.decoder, self.actor, self.critic, self.std, self.var_clip = encoder, heads, decoder, actor, critic, std, var_clip
        self.num_actions, self.clip_actions = actor.widths[-1], actor.clip
        self.num_latent, self.num_explicit = heads[0].widths[-1], heads[2].widths[-1]
        self.num_obs = actor.widths[0] - self.num_latent - self.num_explicit
        self.vae_chains = (encoder,) + tuple(heads) + (decoder,)

    def rl_parameters(self):
        """Actor, critic, then std: the order of PPO_DreamWaQ.rl_parameters and of the RL pass's gradients."""
        return [p for c in (self.actor, self.critic) for l in c.linears for p in (l.weight, l.bias)] + [self.std]

    def rl_parameter_names(self):
        return [f"{c.name}.{i}.{n}" for c in (self.actor, self.critic) for i in range(len(c.linears)) for n in ("weight", "bias")] + ["std"]

    def vae_parameters(self):
        """Encoder, latent_mu, latent_var, vel_mu, vel_var, decoder: the order of actor_critic.vae.parameters() and of the VAE pass's gradients."""
        return [p for c in self.vae_chains for l in c.linears for p in (l.weight, l.bias)]

    def vae_parameter_names(self):
        return [f"vae.{c.name}.{i}.{n}" for c in self.vae_chains for i in range(len(c.linears)) for n in ("weight", "bias")]


def describe_dwaq(actor_critic, device=None):
    """ActorCriticDreamWaQ as the kernels take it (duck-typed: .vae with .encoder, the four heads and .decoder; .actor, .critic, .std).  The
    encoder may end in an ELU, as the reference's does, on this path only; the actor may end in a Hardtanh or not.  Refusals are ValueErrors
    that name the layer or the member."""
    vae = getattr(actor_critic, "vae", None)
    if vae is None:
        raise ValueError(f"{_DWAQ}: the module has no .vae; the plain ActorCritic is FusedTrainPass's")
    c, std = _describe(actor_critic, device, _DWAQ, _DWAQ_FOREIGN, " beside .vae; only ActorCriticDreamWaQ is built", (("actor", True), ("critic", False)))
    for need in ("encoder", "decoder"):
        if getattr(vae, need, None) is None:
            raise ValueError(f"{_DWAQ}: the module's .vae has no .{need}")
    encoder = nets.describe_chain("encoder", vae.encoder, device, False, _DWAQ, allow_last_elu=True)
    decoder = nets.describe_chain("decoder", vae.decoder, device, False, _DWAQ)
    head = nets.describe_heads(vae, encoder.widths[-1], device, _DWAQ)
    L, E = head.L, head.E
    if decoder.widths[0] != L + E:
        raise ValueError(f"{_DWAQ}: decoder[0] takes {decoder.widths[0]} inputs, but [z | v] has {L} + {E} columns")
    if c["actor"].widths[0] <= L + E:
        raise ValueError(f"{_DWAQ}: actor[0] takes {c['actor'].widths[0]} inputs, but [obs | z | v] has O + {L} + {E} columns with O >= 1")
    spec = TrainSpecDreamWaQ(encoder, head.chains, decoder, c["actor"], c["critic"], std, head.clip)
    if isinstance(vae, nn.Module):
        theirs = list(vae.parameters())
        if len(theirs) != len(spec.vae_parameters()) or any(a is not b for a, b in zip(theirs, spec.vae_parameters())):
            raise ValueError(f"{_DWAQ}: vae.parameters() are not the encoder's, latent_mu's, latent_var's, vel_mu's, vel_var's and the decoder's, in that order")
    return spec


def _dwaq_front(a, spec, obs_history, noise, n, device, grads=None):
    """The encoder, the four heads and the noise of either descriptor; `grads`: the gradient tensors of those five chains, or None."""
    enc = a.chain[abi.TRAIN_DWAQ_ENCODER]
    enc.input, enc.in_stride = nets.rows(obs_history, spec.encoder.widths[0], "obs_history", n, device, _DWAQ)
    at = 0
    for ci, c in enumerate((spec.encoder,) + tuple(spec.heads)):
        _fill_chain(a.chain[ci], c, device, None if grads is None else grads[at:at + 2 * len(c.linears)])
        at += 2 * len(c.linears)
    a.var_clip = spec.var_clip
    a.noise, a.noise_stride = nets.rows(noise, spec.num_latent + spec.num_explicit, "latent_noise", n, device, _DWAQ)
    return at


def dwaq_args(spec, obs, obs_history, critic_obs, noise, mu, sigma, values, workspace, grads=None, grad_mu=None, grad_sigma=None, grad_values=None,
              device=None):
    """LgTrainDwaqArgs of one call of the RL pass.  `grads` (backward): the tensors that take the gradients, in spec.rl_parameters() order
    (actor, critic, std).  The encoder's and the heads' gradient pointers stay null: the pass has no use for them."""
    a = abi.LgTrainDwaqArgs()
    if not isinstance(obs, torch.Tensor) or obs.dim() != 2 or obs.shape[0] < 1:
        raise ValueError(f"{_DWAQ}: obs must be a (B, {spec.num_obs}) float32 tensor with B >= 1")
    n = int(obs.shape[0])
    a.n_rows, a.n_obs = n, spec.num_obs
    act, cri = a.chain[abi.TRAIN_DWAQ_ACTOR], a.chain[abi.TRAIN_DWAQ_CRITIC]
    act.input, act.in_stride = nets.rows(obs, spec.num_obs, "obs", n, device, _DWAQ)
    cri.input, cri.in_stride = nets.rows(critic_obs, spec.critic.widths[0], "critic_obs", n, device, _DWAQ)
    _dwaq_front(a, spec, obs_history, noise, n, device)
    g_act, g_cri, g_std = _rl_grads(grads, spec.actor, spec.critic)
    _fill_chain(act, spec.actor, device, g_act)
    _fill_chain(cri, spec.critic, device, g_cri)
    _fill_heads(a, spec, mu, sigma, values, n, device, _DWAQ, g_std, grad_mu, grad_sigma, grad_values)
    _bind_workspace(a, workspace, device, _DWAQ)
    return a


def vae_args(spec, obs_history, labels, next_states, terminated, noise, kld_weight, loss, workspace, grads=None, upstream=None, device=None):
    """LgTrainVaeArgs of one call of the VAE pass.  `loss`: the tensor of abi.TRAIN_VAE_LOSSES floats (total, estimation, reconstruction,
    kld); `grads` (backward): in spec.vae_parameters() order."""
    a = abi.LgTrainVaeArgs()
    if not isinstance(obs_history, torch.Tensor) or obs_history.dim() != 2 or obs_history.shape[0] < 1:
        raise ValueError(f"{_DWAQ}: obs_history must be a (B, {spec.encoder.widths[0]}) float32 tensor with B >= 1")
    n = int(obs_history.shape[0])
    a.n_rows, a.kld_weight = n, float(kld_weight)
    at = _dwaq_front(a, spec, obs_history, noise, n, device, grads)
    _fill_chain(a.chain[abi.TRAIN_VAE_DECODER], spec.decoder, device, None if grads is None else grads[at:])
    a.labels, a.labels_stride = nets.rows(labels, spec.num_explicit, "explicit_info_labels", n, device, _DWAQ)
    a.next_states, a.next_states_stride = nets.rows(next_states, spec.decoder.widths[-1], "next_states", n, device, _DWAQ)
    a.mask, a.mask_stride = nets.rows(terminated, 1, "terminated", n, device, _DWAQ)
    if loss is not None:
        a.loss = _scalar(loss, "the losses", device, abi.TRAIN_VAE_LOSSES, _DWAQ)
    if upstream is not None:
        a.upstream = _scalar(upstream, "the upstream gradient", device, 1, _DWAQ)
    _bind_workspace(a, workspace, device, _DWAQ)
    return a


def plan_dwaq(n_rows, encoder_widths, latent, explicit, actor_widths, critic_widths):
    """LgTrainDwaqPlan of the RL pass (lg_train_dwaq_plan): the encoder ends at H columns, the heads are H -> latent, latent, explicit, explicit."""
    H = encoder_widths[-1]
    heads = tuple((abi.TRAIN_DWAQ_LATENT_MU + h, (H, w)) for h, w in enumerate((latent, latent, explicit, explicit)))
    return _plan("lg_train_dwaq_plan", abi.LgTrainDwaqArgs, abi.LgTrainDwaqPlan, n_rows,
                 ((abi.TRAIN_DWAQ_ENCODER, encoder_widths),) + heads + ((abi.TRAIN_DWAQ_ACTOR, actor_widths), (abi.TRAIN_DWAQ_CRITIC, critic_widths)),
                 n_obs=int(actor_widths[0]) - int(latent) - int(explicit))


def plan_vae(n_rows, encoder_widths, latent, explicit, decoder_widths):
    """LgTrainDwaqPlan of the VAE pass (lg_train_vae_plan)."""
    H = encoder_widths[-1]
    heads = tuple((abi.TRAIN_DWAQ_LATENT_MU + h, (H, w)) for h, w in enumerate((latent, latent, explicit, explicit)))
    return _plan("lg_train_vae_plan", abi.LgTrainVaeArgs, abi.LgTrainDwaqPlan, n_rows,
                 ((abi.TRAIN_DWAQ_ENCODER, encoder_widths),) + heads + ((abi.TRAIN_VAE_DECODER, decoder_widths),))


class VaeLosses:
    """What FusedTrainPassDreamWaQ.vae_loss returns: .loss (0-dim, with autograd) = explicit_estimation_loss + reconstruction_loss +
    kld_weight * kld_loss, and the three terms as detached device scalars."""

    def __init__(self, losses):
        self.loss = losses[0]
        d = losses.detach()
        self.explicit_estimation_loss, self.reconstruction_loss, self.kld_loss = d[1], d[2], d[3]


class _VaeFunction(torch.autograd.Function):
    """The four losses of the VAE pass `ps` as one (4,) tensor; only element 0, the total, carries a gradient."""

    @staticmethod
    def forward(ctx, ps, kld_weight, n_inputs, *inputs_and_params):
        inputs = inputs_and_params[:n_inputs]
        losses = torch.empty(abi.TRAIN_VAE_LOSSES, dtype=torch.float32, device=ps.device)
        args = ps.args(ps.spec, *inputs, kld_weight, losses, None, device=ps.device)
        ctx.ps, ctx.inputs, ctx.kld_weight, ctx.call = ps, inputs, kld_weight, ps.run_forward(args, int(inputs[0].shape[0]))
        return losses

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_losses):
        ps = ctx.ps
        up = grad_losses.to(torch.float32)[:1].contiguous()             # stays on the device: the kernel reads it there
        grads = ps.run_backward(ctx.call, lambda grads: ps.args(ps.spec, *ctx.inputs, ctx.kld_weight, None, ps.workspace, grads, up, device=ps.device))
        return (None,) * (3 + len(ctx.inputs)) + tuple(grads)


class FusedTrainPassDreamWaQ:
    """The two network passes of PPO_DreamWaQ.update() on an ActorCriticDreamWaQ (include/lgtraindwaq.h):

        tp = FusedTrainPassDreamWaQ(actor_critic_dreamwaq, kld_weight=vae_kld_weight)
        mu, sigma, values = tp(obs, obs_history, critic_obs)                              # RL step: one launch; backward three
        out = tp.vae_loss(obs_history, explicit_info_labels, next_states, terminated)     # VAE step: two launches; backward three
        out.loss.backward()       # out.explicit_estimation_loss, out.reconstruction_loss, out.kld_loss: detached device scalars

    Optimise tp.rl_parameters() (actor, critic, std: the reference's order) and tp.vae_parameters() (the order of
    actor_critic.vae.parameters()) apart.  The RL pass gives the VAE's parameters no gradient (their .grad is left as it was): the reference
    clears that gradient before anything reads it.  The VAE pass leaves the actor, the critic and std alone.  Each pass has its own workspace
    and call counter: a forward of one does not invalidate a pending backward of the other; within a pass a backward whose forward has been
    overwritten raises.

    The KL term is the reference's arithmetic: its (B,) row sums times its (B, 1) mask broadcast to (B, B) before the mean, so that
    kld = -0.5 * (sum of the row sums) * (sum of the mask) / B^2 whatever a row's own mask.

    latent_noise is the (B, L + E) standard-normal draw of the reparameterisation, columns [z | vel] (FusedPolicy's latent_noise
    convention).  With latent_noise=None each call draws one torch.randn((B, L + E)) on the device: that is NOT the reference's stream,
    which draws two randn_like tensors (z, then vel) per call.  The draw is an allocation under torch's generator, so a captured HIP graph
    needs a caller-owned noise tensor, refilled in place between replays; the VAE backward reads the noise again, so it must not change
    between a vae_loss and its backward."""

    def __init__(self, actor_critic, kld_weight=1.0):
        self.device = _module_device(actor_critic, _DWAQ)
        self.spec = describe_dwaq(actor_critic, self.device)
        self.kld_weight = float(kld_weight)
        self._rl = _Pass(_DWAQ, "RL ", "lg_train_dwaq", dwaq_args, self.plan, self.rl_parameters, self.spec, self.device)
        self._vae = _Pass(_DWAQ, "VAE ", "lg_train_vae", vae_args, self.vae_plan, self.vae_parameters, self.spec, self.device)

    def rl_parameters(self):
        return self.spec.rl_parameters()

    def vae_parameters(self):
        return self.spec.vae_parameters()

    def plan(self, n_rows):
        s = self.spec
        return plan_dwaq(n_rows, s.encoder.widths, s.num_latent, s.num_explicit, s.actor.widths, s.critic.widths)

    def vae_plan(self, n_rows):
        s = self.spec
        return plan_vae(n_rows, s.encoder.widths, s.num_latent, s.num_explicit, s.decoder.widths)

    def _noise(self, like, latent_noise):
        if latent_noise is not None:
            return latent_noise
        return torch.randn((int(like.shape[0]), self.spec.num_latent + self.spec.num_explicit), dtype=torch.float32, device=self.device)

    def __call__(self, obs, obs_history, critic_obs, latent_noise=None):
        """(mu, sigma, values) of the mini-batch: (B, A), (B, A), (B, 1).  One launch on the current stream."""
        return _apply(_RLFunction, self._rl, obs, obs_history, critic_obs, self._noise(obs, latent_noise))

    def vae_loss(self, obs_history, explicit_info_labels, next_states, terminated, latent_noise=None):
        """The VAE loss of PPO_DreamWaQ._compute_vae_loss and its three terms, as a VaeLosses.  Two launches."""
        inputs = (obs_history, explicit_info_labels, next_states, terminated, self._noise(obs_history, latent_noise))
        return VaeLosses(_VaeFunction.apply(self._vae, self.kld_weight, len(inputs), *inputs, *self.vae_parameters()))


# ---- the recurrent family (include/lgtrainrnn.h, csrc/lg_train_rnn.hip) -------------------------------------------------------------------------
_RNN_PARAMS = ("weight_ih", "weight_hh", "bias_ih", "bias_hh")


class TrainSpecRecurrent:
    """ActorCriticRecurrent as the kernels take it: policy.py's reading of the module (the two memories, the two chains, std)."""

    def __init__(self, ps):
        self.actor, self.critic, self.std, self.memory_a, self.memory_c = ps.actor, ps.critic, ps.std, ps.memory_a, ps.memory_c
        self.chains, self.memories = (ps.actor, ps.critic), (ps.memory_a, ps.memory_c)
        self.num_actions, self.clip_actions = ps.num_actions, ps.clip_actions

    def parameters(self):
        """std, the actor's and the critic's weight and bias per layer, then per memory and layer weight_ih, weight_hh, bias_ih, bias_hh:
        the order of ActorCriticRecurrent.parameters() and of the pass's gradients."""
        return [self.std] + [p for c in self.chains for l in c.linears for p in (l.weight, l.bias)] + \
            [getattr(m.rnn, f"{n}_l{k}") for m in self.memories for k in range(m.layers) for n in _RNN_PARAMS]

    def parameter_names(self):
        return ["std"] + [f"{c.name}.{i}.{n}" for c in self.chains for i in range(len(c.linears)) for n in ("weight", "bias")] + \
            [f"{m.name}.rnn.{n}_l{k}" for m in self.memories for k in range(m.layers) for n in _RNN_PARAMS]


def describe_recurrent(actor_critic, device=None):
    """ActorCriticRecurrent through FusedPolicy's reader (policy.py), so that what can be rolled out can be trained; refusals are
    ValueErrors of FusedTrainPassRecurrent that name the member."""
    if not getattr(actor_critic, "is_recurrent", False):
        raise ValueError(f"{_RNN}: the module is not recurrent (is_recurrent); FusedTrainPass is the pass of the plain ActorCritic")
    return TrainSpecRecurrent(policy._describe_recurrent(actor_critic, device, _RNN))


def _padded(t, width, what, device):
    """A (max_len, n_traj, width) float32 tensor addressed in place: (pointer, time stride, row stride, max_len, n_traj)."""
    if not isinstance(t, torch.Tensor) or t.dtype != torch.float32 or t.dim() != 3 or t.shape[2] != width or t.shape[0] < 1 or t.shape[1] < 1 \
            or (width > 1 and t.stride(2) != 1) or (device is not None and t.device != device):
        got = f"{tuple(t.shape)} {t.dtype} with strides {t.stride()} on {t.device}" if isinstance(t, torch.Tensor) else type(t).__name__
        raise ValueError(f"{_RNN}: {what} must be (max_len, n_traj, {width}) float32 with unit inner stride" + (f" on {device}" if device is not None else "")
                         + f"; got {got}")
    return t.data_ptr(), (t.stride(0) if t.shape[0] > 1 else 0), (t.stride(1) if t.shape[1] > 1 else width), int(t.shape[0]), int(t.shape[1])


def _start_states(hid, mem, n_traj, what, device):
    """[h] (GRU) or [h, c] (LSTM) of one memory from what the generator yields: a tensor or a list, each (layers, n_traj, H)."""
    states = list(hid) if isinstance(hid, (list, tuple)) else [hid]
    want = 2 if mem.kind == "lstm" else 1
    if len(states) != want:
        raise ValueError(f"{_RNN}: {what} holds {len(states)} tensors, an {mem.kind.upper()} has {want}")
    out = []
    for t, n in zip(states, ("h", "c")):
        if not isinstance(t, torch.Tensor) or t.dtype != torch.float32 or tuple(t.shape) != (mem.layers, n_traj, mem.hidden) \
                or (mem.hidden > 1 and t.stride(2) != 1) or (device is not None and t.device != device):
            got = f"{tuple(t.shape)} {t.dtype} with strides {t.stride()} on {t.device}" if isinstance(t, torch.Tensor) else type(t).__name__
            raise ValueError(f"{_RNN}: {what} {n} must be ({mem.layers}, {n_traj}, {mem.hidden}) float32 with unit inner stride"
                             + (f" on {device}" if device is not None else "") + f"; got {got}")
        out.append((t.data_ptr(), t.stride(0) if mem.layers > 1 else 0, t.stride(1) if n_traj > 1 else mem.hidden))
    return out


def rnn_sizes(masks, obs, n_envs):
    """(n_rows, max_len, n_traj, T) of a recurrent mini-batch from the shapes and the env count."""
    if not isinstance(masks, torch.Tensor) or masks.dtype not in (torch.bool, torch.uint8) or masks.dim() != 2 or masks.shape[0] < 1 \
            or (masks.shape[1] > 1 and masks.stride(1) != 1):
        got = f"{tuple(masks.shape)} {masks.dtype} with strides {masks.stride()}" if isinstance(masks, torch.Tensor) else type(masks).__name__
        raise ValueError(f"{_RNN}: masks must be (T, n_traj) bool with unit inner stride; got {got}")
    T, n_traj = int(masks.shape[0]), int(masks.shape[1])
    if not isinstance(obs, torch.Tensor) or obs.dim() != 3 or obs.shape[1] != n_traj or not 1 <= obs.shape[0] <= T:
        got = tuple(obs.shape) if isinstance(obs, torch.Tensor) else type(obs).__name__
        raise ValueError(f"{_RNN}: obs must be (max_len, {n_traj}, width) with 1 <= max_len <= T = {T}, as the masks say; got {got}")
    if not isinstance(n_envs, int) or not 1 <= n_envs <= n_traj:
        raise ValueError(f"{_RNN}: n_envs = {n_envs!r} must be an int in [1, n_traj = {n_traj}]")
    return T * n_envs, int(obs.shape[0]), n_traj, T


def rnn_args(spec, obs, critic_obs, masks, hid, n_envs, mu, sigma, values, workspace, grads=None, grad_mu=None, grad_sigma=None, grad_values=None,
             device=None):
    """LgTrainRnnArgs of one call; the padded observations, the masks and the start states are addressed in place.  `grads` (backward):
    the tensors that take the gradients, in spec.parameters() order.  Refusals are ValueErrors; the library is not touched."""
    a = abi.LgTrainRnnArgs()
    n, max_len, n_traj, T = rnn_sizes(masks, obs, n_envs)
    if device is not None and masks.device != device:
        raise ValueError(f"{_RNN}: masks is on {masks.device}, not on {device}")
    if not isinstance(hid, (list, tuple)) or len(hid) != 2:
        raise ValueError(f"{_RNN}: hid_states must be the pair (hid_a, hid_c) of the mini-batch generator")
    a.train.n_rows = n
    g0 = 1
    for ch, c in zip(a.train.chain, spec.chains):
        _fill_chain(ch, c, device, None if grads is None else grads[g0:g0 + 2 * len(c.linears)])
        g0 += 2 * len(c.linears)
    for m, ms, x, h, what in zip(a.memory, spec.memories, (obs, critic_obs), hid, ("obs", "critic_obs")):
        m.kind, m.n_layers, m.hidden, m.n_in = (abi.TRAIN_RNN_LSTM if ms.kind == "lstm" else abi.TRAIN_RNN_GRU), ms.layers, ms.hidden, ms.input_size
        m.x, m.x_time_stride, m.x_row_stride, ml, nt = _padded(x, ms.input_size, what, device)
        if (ml, nt) != (max_len, n_traj):
            raise ValueError(f"{_RNN}: {what} is ({ml}, {nt}, .), obs ({max_len}, {n_traj}, .)")
        st = _start_states(h, ms, n_traj, f"hid_states of {ms.name}", device)
        m.h0, m.h0_layer_stride, m.h0_row_stride = st[0]
        if len(st) > 1:
            m.c0, m.c0_layer_stride, m.c0_row_stride = st[1]
        m.mask, m.mask_time_stride = masks.data_ptr(), (masks.stride(0) if T > 1 else n_traj)
        m.max_len, m.n_traj, m.T = max_len, n_traj, T
        for k in range(ms.layers):
            L = m.layer[k]
            L.weight_ih, L.weight_hh, L.bias_ih, L.bias_hh = (t.data_ptr() for t in ms.params(k))
            if grads is not None:
                L.grad_weight_ih, L.grad_weight_hh, L.grad_bias_ih, L.grad_bias_hh = (t.data_ptr() for t in grads[g0:g0 + 4])
                g0 += 4
    _fill_heads(a.train, spec, mu, sigma, values, n, device, _RNN, *(() if grads is None else (grads[0], grad_mu, grad_sigma, grad_values)))
    _bind_workspace(a.train, workspace, device, _RNN)
    return a


def plan_rnn(n_rows, max_len, n_traj, T, kind, memories, actor_widths, critic_widths):
    """LgTrainRnnPlan of a mini-batch of these sizes; `kind`: "lstm" or "gru"; `memories`: (layers, hidden, input width) of memory_a and
    memory_c; the widths [in, out_0, out_1, ...] of the two chains."""
    key = ("lg_train_rnn_plan", int(n_rows), int(max_len), int(n_traj), int(T), kind, tuple(tuple(int(v) for v in m) for m in memories),
           tuple(int(x) for x in actor_widths), tuple(int(x) for x in critic_widths))
    if key not in _PLANS:
        lib, a, p = abi.load_lib(), abi.LgTrainRnnArgs(), abi.LgTrainRnnPlan()
        a.train.n_rows = key[1]
        for m, (layers, hidden, n_in) in zip(a.memory, key[6]):
            m.kind, m.n_layers, m.hidden, m.n_in = (abi.TRAIN_RNN_LSTM if kind == "lstm" else abi.TRAIN_RNN_GRU), layers, hidden, n_in
            m.max_len, m.n_traj, m.T = key[2:5]
        _widths_into(a.train.chain[0], key[7])
        _widths_into(a.train.chain[1], key[8])
        abi.check(lib.lg_train_rnn_plan(C.byref(a), C.byref(p)), lib)
        _PLANS[key] = p
    return _PLANS[key]


class _RnnFunction(torch.autograd.Function):
    """(mu, sigma, values) of the recurrent pass `ps` from a recurrent mini-batch; the parameters ride along as in _RLFunction."""

    @staticmethod
    def forward(ctx, ps, obs, critic_obs, masks, hid, n_envs, *params):
        spec, device = ps.spec, ps.device
        sizes = rnn_sizes(masks, obs, n_envs)
        mu = torch.empty((sizes[0], spec.num_actions), dtype=torch.float32, device=device)
        sigma = torch.empty_like(mu)
        values = torch.empty((sizes[0], spec.critic.widths[-1]), dtype=torch.float32, device=device)
        args = rnn_args(spec, obs, critic_obs, masks, hid, n_envs, mu, sigma, values, None, device=device)
        ctx.ps, ctx.inputs, ctx.call = ps, (obs, critic_obs, masks, hid, n_envs), ps.run_forward(args, sizes, args.train)
        ctx.save_for_backward(mu, sigma, values)
        return mu, sigma, values

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_mu, grad_sigma, grad_values):
        ps = ctx.ps
        mu, sigma, values = ctx.saved_tensors
        gm, gs, gv = _grad_rows(grad_mu, mu), _grad_rows(grad_sigma, sigma), _grad_rows(grad_values, values)
        grads = ps.run_backward(ctx.call, lambda g: rnn_args(ps.spec, *ctx.inputs, mu, sigma, values, ps.workspace, g, gm, gs, gv, device=ps.device))
        return (None,) * 6 + tuple(grads)           # nothing for the observations, the masks or the start states


class FusedTrainPassRecurrent:
    """The network passes of PPO.update() on an ActorCriticRecurrent (include/lgtrainrnn.h), fed by what
    RolloutStorage.reccurent_mini_batch_generator yields:

        tp = FusedTrainPassRecurrent(actor_critic_recurrent)
        mu, sigma, values = tp(obs_batch, critic_obs_batch, masks_batch, hid_states_batch, n_envs=actions_batch.shape[1])
        out = loss_fn(mu, sigma, values, actions_batch.flatten(0, 1), ...)        # FusedPPOLoss, rows in unpad_trajectories' order
        opt.zero_grad(); out.loss.backward(); opt.step(kl_mean=out.kl_mean)       # FusedAdam over tp.parameters()

    obs_batch / critic_obs_batch are the (max_len, n_traj, width) views of the padded set, masks_batch the (T, n_traj) bool view and
    hid_states_batch = (hid_a, hid_c), a tensor each for a GRU and a list [h, c] each for an LSTM (hid_c may be hid_a); all are read in
    place.  mu and sigma are (T E, A), values (T E, 1), row t E + e as `unpad_trajectories(...).flatten(0, 1)` orders them.  E, the number
    of envs of the mini-batch, is mask.sum() / T and in no shape: pass it as n_envs (PPO.update has it as the second dimension of every
    stored column) and nothing synchronises with the host; without it the pass reads mask.sum() back once, which a HIP graph capture cannot
    do.  There is no gradient for the observations or the start states."""

    def __init__(self, actor_critic):
        self.device = _module_device(actor_critic, _RNN)
        self.spec = describe_recurrent(actor_critic, self.device)
        self._pass = _Pass(_RNN, "", "lg_train_rnn", rnn_args, lambda sizes: self.plan(*sizes), self.spec.parameters, self.spec, self.device)

    def parameters(self):
        return self.spec.parameters()

    @property
    def workspace(self):
        """The float32 workspace of the last forward call, laid out by its plan (LgTrainRnnPlan's offsets); None before the first call.
        For reading only: the next forward call overwrites or replaces it."""
        return self._pass.workspace

    def plan(self, n_rows, max_len, n_traj, T):
        s = self.spec
        return plan_rnn(n_rows, max_len, n_traj, T, s.memory_a.kind, [(m.layers, m.hidden, m.input_size) for m in s.memories], s.actor.widths,
                        s.critic.widths)

    def __call__(self, obs_batch, critic_obs_batch, masks_batch, hid_states_batch, n_envs=None):
        """(mu, sigma, values) of the mini-batch: (T E, A), (T E, A), (T E, 1).  2 + 2 layers launches on the current stream."""
        if n_envs is None:
            n_envs = int(masks_batch.sum().item()) // int(masks_batch.shape[0])          # the one read-back; see the class docstring
        return _RnnFunction.apply(self._pass, obs_batch, critic_obs_batch, masks_batch, hid_states_batch, int(n_envs), *self.spec.parameters())
