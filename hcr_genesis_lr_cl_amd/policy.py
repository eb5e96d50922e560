"""FusedPolicy: the rollout half of an rsl_rl actor-critic -- actor, critic, sampling and log-prob -- as ONE HIP launch (`lg_policy_act`,
include/lgpolicy.h, csrc/lg_policy.hip).

What rsl_rl/algorithms/ppo.py:93-105 asks of `ActorCritic` / `ActorCriticEE` per rollout step (act, evaluate, get_actions_log_prob,
action_mean, action_std: about 25 torch launches) is one call of `FusedPolicy.act`, which can write its five results straight into row
`storage.step` of a `RolloutStorage`.  The module is wrapped by duck typing: `.actor` and `.critic` (and optionally `.estimator`) are
`nn.Sequential`s of `Linear`, `ELU` and -- only at the actor's end -- `Hardtanh`; `.std` is the per-action standard deviation.  Weights,
biases and std are read IN PLACE on every call (no packed copy that an optimizer step could leave stale).  The class serves the rollout
only: everything runs on `.data` without autograd, and `update()` keeps using the module itself.  Recurrent policies, the TS / CTS /
DreamWaQ families and activations other than ELU are refused, with a message that names the layer.

The draw is torch's when `noise` is given, otherwise the project's Philox4x32-10: counter (env, action quad, call counter, stream tag),
key = seed, Box-Muller on the uniforms; the call counter is a device cell that a one-lane launch behind the act launch increments, so a
captured call draws fresh numbers on every replay.

Measured at 4096 envs against the same rows from torch ops replayed as one HIP graph (tools/policy_act_time.py):
go2 nets 68 us against 158 us per step, and the act -> step -> add_step loop 45.6 M against 22.8 M env-steps/s.  For the explicit-estimator
sets the fused launch does NOT beat the graph replay: go2_ee 406 us against 300 us, tron1_pf_ee 395 us against 299 us (16-row tiles
re-read 2 GB of weights from L2 per step); a rollout that only wants speed keeps the torch path for those.

There is no CPU path: the kernel lives in csrc/liblgsim.so."""
from __future__ import annotations

import ctypes as C

import torch
import torch.nn as nn

from . import abi

class ChainSpec:
    """One MLP chain as the kernel takes it: its Linear modules in order, which of them an ELU follows, and (actor only) the clip."""

    def __init__(self, name, linears, elu, clip):
        self.name, self.linears, self.elu, self.clip = name, linears, elu, clip

    @property
    def widths(self):
        return [self.linears[0].in_features] + [l.out_features for l in self.linears]


class PolicySpec:
    """`describe`'s result: the chains, whether the actor reads (features, estimator output), the clip value, the action count."""

    def __init__(self, estimator, actor, critic, std):
        self.estimator, self.actor, self.critic, self.std = estimator, actor, critic, std
        self.concat = estimator is not None
        self.clip_actions = actor.clip
        self.num_actions = actor.widths[-1]

    @property
    def chain_order(self):
        """The order a workgroup walks: the estimator precedes its actor; the critic runs in workgroups of its own."""
        return [c.name for c in (self.estimator, self.actor, self.critic) if c is not None]


def _check_tensor(t, what, device):
    if t.dtype != torch.float32:
        raise ValueError(f"FusedPolicy: {what} is {t.dtype}, the kernel reads float32")
    if not t.is_contiguous():
        raise ValueError(f"FusedPolicy: {what} is not contiguous")
    if device is not None and t.device != device:
        raise ValueError(f"FusedPolicy: {what} is on {t.device}, not on the HIP device {device}")


def _describe_chain(name, seq, device, allow_clip):
    if not isinstance(seq, nn.Sequential):
        raise ValueError(f"FusedPolicy: {name} is {type(seq).__name__}, expected an nn.Sequential of Linear / ELU"
                         + (" / Hardtanh" if allow_clip else "") + " (recurrent and encoder policies keep the torch path)")
    linears, elu, clip = [], [], None
    mods = list(seq)
    for i, m in enumerate(mods):
        where = f"{name}[{i}]"
        if clip is not None:
            raise ValueError(f"FusedPolicy: {where} ({type(m).__name__}) follows the Hardtanh, which must end the actor")
        if isinstance(m, nn.Linear):
            if m.bias is None:
                raise ValueError(f"FusedPolicy: {where} has no bias")
            if m.in_features > abi.POLICY_MAX_WIDTH or m.out_features > abi.POLICY_MAX_WIDTH:
                raise ValueError(f"FusedPolicy: {where} is {m.in_features} -> {m.out_features}, widths are limited to {abi.POLICY_MAX_WIDTH}")
            if linears and linears[-1].out_features != m.in_features:
                raise ValueError(f"FusedPolicy: {where} takes {m.in_features} inputs, the layer before it gives {linears[-1].out_features}")
            _check_tensor(m.weight.data, f"{where}.weight", device)
            _check_tensor(m.bias.data, f"{where}.bias", device)
            linears.append(m)
            elu.append(False)
        elif isinstance(m, nn.ELU):
            if not linears or elu[-1]:
                raise ValueError(f"FusedPolicy: {where} (ELU) does not follow a Linear")
            if m.alpha != 1.0:
                raise ValueError(f"FusedPolicy: {where} is ELU(alpha={m.alpha}), only alpha = 1 is built")
            elu[-1] = True
        elif isinstance(m, nn.Hardtanh) and allow_clip:
            if i != len(mods) - 1 or not linears or elu[-1] or m.min_val != -m.max_val or not m.max_val >= 0:
                raise ValueError(f"FusedPolicy: {where} (Hardtanh({m.min_val}, {m.max_val})) must be the symmetric clip behind the actor's last Linear")
            clip = float(m.max_val)
        else:
            raise ValueError(f"FusedPolicy: {where} is {type(m).__name__}; only Linear and ELU"
                             + (" (and a final Hardtanh)" if allow_clip else "") + " are built into the kernel")
    if not linears:
        raise ValueError(f"FusedPolicy: {name} has no Linear layer")
    if len(linears) > abi.POLICY_MAX_LAYERS:
        raise ValueError(f"FusedPolicy: {name} has {len(linears)} Linear layers, the kernel takes {abi.POLICY_MAX_LAYERS}")
    if elu[-1]:
        raise ValueError(f"FusedPolicy: {name} ends in an ELU, expected a Linear output layer")
    return ChainSpec(name, linears, elu, clip)


def describe(actor_critic, device=None):
    """What the kernel will be told about `actor_critic`, with every refusal; touches neither the library nor the device.  `device`:
    the HIP device every parameter must live on (None: not checked, for inspecting a module on the host)."""
    if getattr(actor_critic, "is_recurrent", False):
        raise ValueError("FusedPolicy: recurrent policies keep the torch path (actor_critic.is_recurrent)")
    for need in ("actor", "critic", "std"):
        if not hasattr(actor_critic, need):
            raise ValueError(f"FusedPolicy: the module has no .{need}")
    est = getattr(actor_critic, "estimator", None)
    estimator = _describe_chain("estimator", est, device, False) if est is not None else None
    actor = _describe_chain("actor", actor_critic.actor, device, True)
    critic = _describe_chain("critic", actor_critic.critic, device, False)
    std = actor_critic.std
    _check_tensor(std.data, "std", device)
    if tuple(std.shape) != (actor.widths[-1],):
        raise ValueError(f"FusedPolicy: std has shape {tuple(std.shape)}, the actor has {actor.widths[-1]} outputs")
    if estimator is not None and actor.widths[0] != estimator.widths[0] + estimator.widths[-1]:
        raise ValueError(f"FusedPolicy: actor[0] takes {actor.widths[0]} inputs, (features, estimator output) has "
                         f"{estimator.widths[0]} + {estimator.widths[-1]}")
    return PolicySpec(estimator, actor, critic, std)


def _rows(x, width, what, n=None, device=None):
    """(pointer, row stride) of an (N, width) float32 matrix with unit inner stride, as the kernel addresses it."""
    if (not torch.is_tensor(x) or x.dtype != torch.float32 or x.dim() != 2 or x.shape[1] != width or (n is not None and x.shape[0] != n)
            or (x.shape[1] > 1 and x.stride(1) != 1) or (x.shape[0] > 1 and x.stride(0) < width) or (device is not None and x.device != device)):
        got = f"{tuple(x.shape)} {x.dtype} strides {x.stride()} on {x.device}" if torch.is_tensor(x) else type(x).__name__
        raise ValueError(f"FusedPolicy: {what} must be ({'N' if n is None else n}, {width}) float32 with unit inner stride"
                         + (f" on {device}" if device is not None else "") + f", got {got}")
    return x.data_ptr(), (x.stride(0) if x.shape[0] > 1 else width)


def _fill_chain(dst, spec, inp, in_width, out):
    dst.n_layers = len(spec.linears)
    dst.input, dst.in_stride = inp
    dst.in_width = in_width
    dst.out, dst.out_stride = out if out is not None else (None, 0)
    for l, m, e in zip(dst.layer, spec.linears, spec.elu):
        l.weight, l.bias, l.n_in, l.n_out, l.elu = m.weight.data.data_ptr(), m.bias.data.data_ptr(), m.in_features, m.out_features, int(e)


def policy_args(spec, obs, critic_obs=None, actions=None, mu=None, sigma=None, log_prob=None, values=None, labels=None, noise=None,
                counter=None, seed=0, flags=0, dbg_uniform=None, device=None):
    """The LgPolicyArgs of one call.  Every tensor is addressed in place; nothing is copied and the library is not touched."""
    a = abi.LgPolicyArgs()
    A = spec.num_actions
    values_only, determ = bool(flags & abi.POLICY_VALUES_ONLY), bool(flags & abi.POLICY_DETERMINISTIC)
    a.flags = flags
    n = int((critic_obs if values_only else obs).shape[0])
    a.n_envs = n
    if not values_only:
        F = spec.estimator.widths[0] if spec.concat else spec.actor.widths[0]
        src = _rows(obs, F, "obs", None, device)
        if spec.concat:
            E = spec.estimator.widths[-1]
            _fill_chain(a.estimator, spec.estimator, src, F, None if labels is None else _rows(labels, E, "labels", n, device))
        _fill_chain(a.actor, spec.actor, src, F, None)
        a.mu, a.mu_stride = _rows(mu, A, "mu", n, device)
        if spec.clip_actions is not None:
            a.clip_on, a.clip_actions = 1, spec.clip_actions
        if not determ:
            a.std = spec.std.data.data_ptr()
            a.actions, a.actions_stride = _rows(actions, A, "actions", n, device)
            a.sigma, a.sigma_stride = _rows(sigma, A, "sigma", n, device)
            a.log_prob, a.log_prob_stride = _rows(log_prob, 1, "log_prob", n, device)
            if noise is not None:
                a.noise, a.noise_stride = _rows(noise, A, "noise", n, device)
            else:
                a.counter, a.seed = counter.data_ptr(), int(seed) & (2 ** 64 - 1)
                if dbg_uniform is not None:                  # the kernel writes it densely: no stride is carried
                    if not dbg_uniform.is_contiguous():
                        raise ValueError("FusedPolicy: the debug uniforms must be a contiguous (N, 4 * ceil(A / 4)) float32 tensor")
                    a.dbg_uniform = _rows(dbg_uniform, 4 * ((A + 3) // 4), "dbg_uniform", n, device)[0]
    if critic_obs is not None and not determ:
        _fill_chain(a.critic, spec.critic, _rows(critic_obs, spec.critic.widths[0], "critic_obs", n, device), spec.critic.widths[0],
                    _rows(values, 1, "values", n, device))
    return a


class FusedPolicy:
    """`FusedPolicy(actor_critic, seed=...)`; `act`, `act_inference`, `evaluate`, `fill_transition`.  See the module docstring."""

    def __init__(self, actor_critic, seed=0, device=None):
        std = getattr(actor_critic, "std", None)
        dev = torch.device(device) if device is not None else (std.device if torch.is_tensor(std) else torch.device("cpu"))
        if dev.type != "cuda":
            raise ValueError(f"FusedPolicy: the module is on {dev}, not on a HIP device (there is no CPU path)")
        if dev.index is None:
            dev = torch.device("cuda", torch.cuda.current_device())
        self.device = dev
        self.module = actor_critic
        self.spec = describe(actor_critic, dev)          # every refusal comes before the library is loaded
        self.seed = int(seed)
        self.lib = abi.load_lib()
        self.counter = torch.zeros(1, dtype=torch.int32, device=dev)        # the Philox call counter (read as uint32)
        self._own = {}
        self._args = {}
        self.last_actions = self.last_mu = self.last_sigma = self.last_log_prob = self.last_values = self.last_labels = None

    # ---- launches ------------------------------------------------------------------------------------------------------
    def _param_key(self):
        """Identity of every layer object of the LIVE module and the address of every parameter: a replaced layer
        (`module.actor[0] = nn.Linear(...)`), a moved parameter or a reassigned `.data` all miss the descriptor cache."""
        key = []
        for name in ("estimator", "actor", "critic"):
            seq = getattr(self.module, name, None)
            key.append(id(seq))
            for m in (seq if isinstance(seq, nn.Sequential) else ()):
                key.append(id(m))
                if isinstance(m, nn.Linear):
                    key += [m.weight.data.data_ptr(), 0 if m.bias is None else m.bias.data.data_ptr()]
        key.append(self.module.std.data.data_ptr())
        return tuple(key)

    def _launch(self, flags, **t):
        """Build (or reuse) the descriptor of this call and enqueue it on the current stream.  The descriptor is keyed by every address
        and stride it holds and by the module's layer objects, so a parameter that moved or a layer that was replaced is seen (the module
        is then described again, with every refusal); the parameters' CONTENTS are read by the kernel each call."""
        key = (flags, self._param_key()) + tuple((k, v.data_ptr(), v.stride(0), v.shape[0]) for k, v in sorted(t.items()) if v is not None)
        a = self._args.get(key)
        if a is None:
            self.spec = describe(self.module, self.device)
            if len(self._args) >= 256:
                self._args.clear()
            a = self._args[key] = policy_args(self.spec, t.get("obs"), t.get("critic_obs"), t.get("actions"), t.get("mu"), t.get("sigma"),
                                              t.get("log_prob"), t.get("values"), t.get("labels"), t.get("noise"), self.counter, self.seed, flags,
                                              t.get("dbg_uniform"), self.device)
        abi.check(self.lib.lg_policy_act(C.byref(a), torch.cuda.current_stream(self.device).cuda_stream), self.lib)

    def _buffers(self, n):
        b = self._own.get(n)
        if b is None:
            A, z = self.spec.num_actions, lambda w: torch.zeros(n, w, device=self.device)
            b = self._own[n] = dict(actions=z(A), mu=z(A), sigma=z(A), log_prob=z(1), values=z(1), inference=z(A), evaluate=z(1),
                                    labels=z(self.spec.estimator.widths[-1]) if self.spec.concat else None)
        return b

    def act(self, obs, critic_obs, storage=None, noise=None, labels=None, _dbg_uniform=None):
        """Sample actions for `obs` ((N, F): the actor's input, or the estimator features of an explicit-estimator module) and evaluate the
        critic on `critic_obs` (None: no critic launch, no values written).  With a `RolloutStorage` / `RolloutStorageEE` the five results
        go straight into row `storage.step` -- actions, mu, sigma, actions_log_prob, values: the rows `add_step` leaves to the caller --
        and the returned actions ARE that row; with zero-copy observation rows `obs` already is `storage.observations[storage.step]`, so
        nothing is copied at all.  Without a storage the results land in buffers this object owns (`last_mu`, `last_sigma`,
        `last_log_prob`, `last_values`; overwritten by the next call of the same N).  `noise` ((N, A), e.g. torch.randn) replaces the Philox
        draw.  `labels` ((N, E), e.g. `storage.estimator_labels[t]`-shaped) receives the estimator's output.  (`_dbg_uniform`, for the
        tests: a contiguous (N, 4 * ceil(A / 4)) tensor that receives the uniforms of the Philox draw.)"""
        n = int(obs.shape[0])
        if storage is not None:
            t = storage.step
            if t >= storage.num_transitions_per_env:
                raise AssertionError("Rollout buffer overflow")
            d = dict(actions=storage.actions[t], mu=storage.mu[t], sigma=storage.sigma[t], log_prob=storage.actions_log_prob[t],
                     values=storage.values[t])
        else:
            d = self._buffers(n)
        if labels is not None and not self.spec.concat:
            raise ValueError("FusedPolicy: a labels row was given, the module has no estimator")
        values = d["values"] if critic_obs is not None else None
        self._launch(0, obs=obs, critic_obs=critic_obs, actions=d["actions"], mu=d["mu"], sigma=d["sigma"], log_prob=d["log_prob"], values=values,
                     labels=labels, noise=noise, dbg_uniform=_dbg_uniform)
        self.last_actions, self.last_mu, self.last_sigma, self.last_log_prob = d["actions"], d["mu"], d["sigma"], d["log_prob"]
        self.last_values, self.last_labels = values, labels
        return d["actions"]

    def act_inference(self, obs):
        """The clipped mean alone (actor_critic.py act_inference): no draw, no critic."""
        mu = self._buffers(int(obs.shape[0]))["inference"]
        self._launch(abi.POLICY_DETERMINISTIC, obs=obs, mu=mu)
        return mu

    def evaluate(self, critic_obs):
        """The critic alone (`compute_returns`' last value)."""
        v = self._buffers(int(critic_obs.shape[0]))["evaluate"]
        self._launch(abi.POLICY_VALUES_ONLY, critic_obs=critic_obs, values=v)
        return v

    def fill_transition(self, transition, obs, critic_obs, noise=None):
        """What rsl_rl's PPO.act (ppo.py:97-104) does to `self.transition`, from one launch; returns the actions."""
        transition.actions = self.act(obs, critic_obs, noise=noise)
        transition.values = self.last_values
        transition.actions_log_prob = self.last_log_prob.view(-1)
        transition.action_mean = self.last_mu
        transition.action_sigma = self.last_sigma
        transition.observations = obs
        transition.critic_observations = critic_obs
        return transition.actions

    def row_tile(self, n=1):
        """Env rows one workgroup carries for this module (32, 16 or 8): the kernel's choice, for documentation and tools."""
        b = self._buffers(n)
        F = (self.spec.estimator or self.spec.actor).widths[0]
        a = policy_args(self.spec, torch.zeros(n, F, device=self.device), torch.zeros(n, self.spec.critic.widths[0], device=self.device),
                        b["actions"], b["mu"], b["sigma"], b["log_prob"], b["values"], counter=self.counter, device=self.device)
        r = self.lib.lg_policy_row_tile(C.byref(a))
        if r == 0:
            abi.check(1, self.lib)
        return r

