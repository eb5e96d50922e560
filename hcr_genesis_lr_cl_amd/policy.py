"""FusedPolicy: the rollout half of an rsl_rl actor-critic -- actor, critic, sampling and log-prob -- as ONE HIP launch (`lg_policy_act`,
include/lgpolicy.h, csrc/lg_policy.hip).

What rsl_rl/algorithms/ppo.py:93-105 asks of `ActorCritic` / `ActorCriticEE` per rollout step (act, evaluate, get_actions_log_prob,
action_mean, action_std: about 25 torch launches) is one call of `FusedPolicy.act`, which can write its five results straight into row
`storage.step` of a `RolloutStorage`.  The module is wrapped by duck typing: `.actor` and `.critic` (and optionally `.estimator`) are
`nn.Sequential`s of `Linear`, `ELU` and -- only at the actor's end -- `Hardtanh`; `.std` is the per-action standard deviation.  Weights,
biases and std are read IN PLACE on every call (no packed copy that an optimizer step could leave stale).  The class serves the rollout
only: everything runs on `.data` without autograd, and `update()` keeps using the module itself.

Three more module shapes are recognised, each still one launch per step (the keywords are in `FusedPolicy.act`'s docstring):
  TS / CTS   `.privilege_encoder` and `.history_encoder` (Linear / ELU) beside `.actor`, `.critic`, `.std` (`ActorCriticTS`, `ActorCriticCTS`):
             the actor reads (obs, latent) with the latent of whichever encoder the call wants; with `num_teacher=k` env rows [0, k) take
             the privilege encoder and the others the history encoder in the same launch (ppo_cts.py:110-135: two actor passes and four
             torch.cat otherwise).
  DreamWaQ   `.vae` with `.encoder` (Linear / ELU, may end in ELU), `.latent_mu`, `.vel_mu` (Linear), `.latent_var`, `.vel_var`
             (a Linear behind Hardtanh(-c, c), one c): the four heads, the clip, the reparameterised draw and the concatenation
             [obs | z | vel] of vae.py:65-101 / actor_critic_dreamwaq.py:145-171 run in the launch.  `.vae.decoder` is the learner's.
  recurrent  `is_recurrent` with `.memory_a.rnn` and `.memory_c.rnn`, each an `nn.LSTM` or `nn.GRU` of one or two layers, H <= 512, in
             front of `.actor` / `.critic` (`ActorCriticRecurrent`): the cell of both memories, the reset of finished envs (`reset=`) and the
             pre-step hidden-state rows the storage keeps run in the launch.  The states live in tensors this object owns, updated in
             place (`get_hidden_states`, `set_hidden_states`, `reset`, `last_hidden_states`), so a captured call keeps its addresses.
A history encoder with Conv1d / Flatten (the "TCN" option) and activations other than ELU are refused, with a message that names the
layer (`FusedPolicy(module, student=False)` does not read the history encoder at all and serves the rollout of such a module: every call but
`act_student` and `num_teacher`); so is an rnn that is bidirectional, projected, batch-first, without bias, with dropout, of more than two layers or H above 512.
What a chain, the four heads, a parameter tensor, std and a row matrix must be is nets.py's, one copy shared with train.py.

The draw is torch's when `noise` is given, otherwise the project's Philox4x32-10: counter (env, action quad, call counter, stream tag),
key = seed, Box-Muller on the uniforms; the call counter is a device cell that a one-lane launch behind the act launch increments, so a
captured call draws fresh numbers on every replay.  DreamWaQ's latent draw is the same with its own tag (`LG_POLICY_LATENT_TAG`) and the
quads of the L + E sampled columns, or `latent_noise`; both draws of a call read the same counter value and it advances once.

Measured at 4096 envs against the same rows from torch ops replayed as one HIP graph (tools/policy_act_time.py):
go2 nets 68 us against 158 us per step, and the act -> step -> add_step loop 45.6 M against 22.8 M env-steps/s.  For the explicit-estimator
sets the fused launch does NOT beat the graph replay: go2_ee 406 us against 300 us, tron1_pf_ee 395 us against 299 us (16-row tiles
re-read 2 GB of weights from L2 per step); a rollout that only wants speed keeps the torch path for those.  The families, same tool,
go2 sizes: go2_ts 294 us against 260 us and go2_dreamwaq 355 us against 323 us -- the fused launch loses there as well, for the same
reason (16-row tiles, 1.5 / 1.7 GB of weights per step) -- while go2_cts (3072 teachers of 4096) WINS, 295 us against 369 us: the torch
side runs the reference's two actor passes and four cats, the fused launch serves both row groups at the cost of the TS step.

Recurrent sets, same tool (the torch side: nn.LSTM of both memories, MLPs, sampling, five copies, the masked reset and the state copies
into the storage): go2_lstm256 (LSTM 256, 16-row tiles) WINS, 266 us against 410 us; go2_lstm512 (LSTM 512, the 8-row tile: 3.2 GB of
weights from L2 per chain and step) loses, 1133 us against 622 us.  A rollout that only wants speed takes the fused launch for hidden
sizes up to 256 and keeps the graph-replayed torch ops at 512; the data flow (no reset call, no state copies) is the same either way.

There is no CPU path: the kernel lives in csrc/liblgsim.so."""
from __future__ import annotations

import ctypes as C

import torch
import torch.nn as nn

from . import abi, nets
from .nets import ChainSpec, HeadSpec      # the names callers know them by here

_OWNER = "FusedPolicy"


class MemorySpec:
    """One memory as the kernel takes it: the `nn.LSTM` / `nn.GRU` module, its kind, layer count, hidden size H and input size."""

    def __init__(self, name, rnn):
        self.name, self.rnn = name, rnn
        self.kind = "lstm" if isinstance(rnn, nn.LSTM) else "gru"
        self.layers, self.hidden, self.input_size = rnn.num_layers, rnn.hidden_size, rnn.input_size

    def params(self, k):
        """(weight_ih, weight_hh, bias_ih, bias_hh) of layer k, as they are now"""
        return tuple(getattr(self.rnn, f"{n}_l{k}").data for n in ("weight_ih", "weight_hh", "bias_ih", "bias_hh"))


class PolicySpec:
    """`describe`'s result: the chains, whether the actor reads (features, estimator output), the clip value, the action count; for a
    recurrent module the two memories."""

    def __init__(self, estimator, actor, critic, std, privilege_encoder=None, history_encoder=None, vae_encoder=None, head=None,
                 memory_a=None, memory_c=None):
        self.estimator, self.actor, self.critic, self.std = estimator, actor, critic, std
        self.privilege_encoder, self.history_encoder, self.vae_encoder, self.head = privilege_encoder, history_encoder, vae_encoder, head
        self.memory_a, self.memory_c = memory_a, memory_c
        self.family = ("recurrent" if memory_a is not None else "ts" if privilege_encoder is not None else "dreamwaq" if head is not None
                       else "ee" if estimator is not None else "plain")
        self.concat = estimator is not None
        self.clip_actions = actor.clip
        self.num_actions = actor.widths[-1]
        # what rides behind the observations in the actor's input: the encoders' latent (TS / CTS), (z, vel) (DreamWaQ)
        if self.family == "ts":
            self.latent_width = privilege_encoder.widths[-1]
        elif self.family == "dreamwaq":
            self.latent_width = head.L + head.E
        else:
            self.latent_width = 0
        self.obs_width = (estimator.widths[0] if self.concat else actor.widths[0]) - self.latent_width
        self.critic_obs_width = critic.widths[0]
        if memory_a is not None:                         # the memories read the observations; the MLPs read the top layer's h
            self.obs_width, self.critic_obs_width = memory_a.input_size, memory_c.input_size

    @property
    def chain_order(self):
        """The order a workgroup walks: a leading chain precedes its actor; the critic runs in workgroups of its own."""
        return [c.name for c in (self.estimator, self.privilege_encoder, self.history_encoder, self.vae_encoder, self.memory_a, self.actor,
                                 self.memory_c, self.critic) if c is not None]


def _describe_memory(name, mem, device, owner=_OWNER):
    rnn = getattr(mem, "rnn", None)
    where = f"{name}.rnn"
    if not isinstance(rnn, (nn.LSTM, nn.GRU)):
        raise ValueError(f"{owner}: {where} is {type(rnn).__name__}, expected an nn.LSTM or nn.GRU")
    if rnn.bidirectional:
        raise ValueError(f"{owner}: {where} is bidirectional; a rollout step has no backward direction")
    if getattr(rnn, "proj_size", 0) != 0:
        raise ValueError(f"{owner}: {where} has proj_size={rnn.proj_size}; projections are not built into the kernel")
    if rnn.dropout != 0:
        raise ValueError(f"{owner}: {where} has dropout={rnn.dropout}; dropout between rnn layers is not built into the kernel")
    if not rnn.bias:
        raise ValueError(f"{owner}: {where} has bias=False; the kernel reads bias_ih and bias_hh")
    if rnn.batch_first:
        raise ValueError(f"{owner}: {where} has batch_first=True; the reference's Memory feeds (1, N, in)")
    if rnn.num_layers > abi.POLICY_MAX_RNN_LAYERS:
        raise ValueError(f"{owner}: {where} has num_layers={rnn.num_layers}, the kernel takes {abi.POLICY_MAX_RNN_LAYERS}")
    if rnn.hidden_size > abi.POLICY_MAX_RNN_HIDDEN:
        raise ValueError(f"{owner}: {where} has hidden_size={rnn.hidden_size}, the gates (4 H) are limited to {abi.POLICY_MAX_WIDTH}: H <= "
                         f"{abi.POLICY_MAX_RNN_HIDDEN}")
    if rnn.input_size > abi.POLICY_MAX_WIDTH:
        raise ValueError(f"{owner}: {where} has input_size={rnn.input_size}, widths are limited to {abi.POLICY_MAX_WIDTH}")
    spec = MemorySpec(name, rnn)
    for k in range(spec.layers):
        for n, t in zip(("weight_ih", "weight_hh", "bias_ih", "bias_hh"), spec.params(k)):
            nets.check_tensor(t, f"{where}.{n}_l{k}", device, owner)
    return spec


def _describe_recurrent(actor_critic, device, owner=_OWNER):
    """The recurrent module as the kernels take it; `owner` names the surface in every refusal (train.py reads the module through this too)."""
    ma, mc = getattr(actor_critic, "memory_a", None), getattr(actor_critic, "memory_c", None)
    if ma is None or mc is None:
        raise ValueError(f"{owner}: a recurrent policy (actor_critic.is_recurrent) needs .memory_a and .memory_c, each with an nn.LSTM or "
                         "nn.GRU as .rnn; other recurrent modules keep the torch path")
    for need in ("actor", "critic", "std"):
        if not hasattr(actor_critic, need):
            raise ValueError(f"{owner}: the module has no .{need}")
    for other in ("estimator", "privilege_encoder", "history_encoder", "vae"):
        if getattr(actor_critic, other, None) is not None:
            raise ValueError(f"{owner}: a memory together with .{other}; memories are built for the plain actor-critic only")
    mem_a, mem_c = _describe_memory("memory_a", ma, device, owner), _describe_memory("memory_c", mc, device, owner)
    if mem_a.kind != mem_c.kind:
        raise ValueError(f"{owner}: memory_a.rnn is an {mem_a.kind.upper()}, memory_c.rnn a {mem_c.kind.upper()}; one kind for both")
    actor = nets.describe_chain("actor", actor_critic.actor, device, True, owner)
    critic = nets.describe_chain("critic", actor_critic.critic, device, False, owner)
    for ch, mem in ((actor, mem_a), (critic, mem_c)):
        if ch.widths[0] != mem.hidden:
            raise ValueError(f"{owner}: {ch.name}[0] takes {ch.widths[0]} inputs (in_features), {mem.name}.rnn gives hidden_size = {mem.hidden}")
    std = actor_critic.std
    nets.check_std(std, actor, device, owner)
    return PolicySpec(None, actor, critic, std, memory_a=mem_a, memory_c=mem_c)


def describe(actor_critic, device=None, student=True):
    """What the kernel will be told about `actor_critic`, with every refusal; touches neither the library nor the device.  `device`:
    the HIP device every parameter must live on (None: not checked, for inspecting a module on the host).  `student=False`: the history
    encoder of a TS / CTS module is not read at all (it may be a Conv1d "TCN"); the spec then has no history_encoder, and only the calls
    that run the privilege encoder are served."""
    if getattr(actor_critic, "is_recurrent", False):
        return _describe_recurrent(actor_critic, device)
    for need in ("actor", "critic", "std"):
        if not hasattr(actor_critic, need):
            raise ValueError(f"FusedPolicy: the module has no .{need}")
    est = getattr(actor_critic, "estimator", None)
    estimator = nets.describe_chain("estimator", est, device, False, _OWNER) if est is not None else None
    actor = nets.describe_chain("actor", actor_critic.actor, device, True, _OWNER)
    critic = nets.describe_chain("critic", actor_critic.critic, device, False, _OWNER)
    std = actor_critic.std
    nets.check_std(std, actor, device, _OWNER)
    ts = hasattr(actor_critic, "privilege_encoder") or hasattr(actor_critic, "history_encoder")
    vae = getattr(actor_critic, "vae", None)
    if (ts or vae is not None) and (estimator is not None or (ts and vae is not None)):
        raise ValueError("FusedPolicy: the module mixes .estimator, .privilege_encoder / .history_encoder and .vae; one family at a time")
    if ts:
        for need in ("privilege_encoder", "history_encoder") if student else ("privilege_encoder",):
            if not hasattr(actor_critic, need):
                raise ValueError(f"FusedPolicy: the module has no .{need}")
        pe = nets.describe_chain("privilege_encoder", actor_critic.privilege_encoder, device, False, _OWNER)
        he = nets.describe_chain("history_encoder", actor_critic.history_encoder, device, False, _OWNER) if student else None
        if he is not None and pe.widths[-1] != he.widths[-1]:
            raise ValueError(f"FusedPolicy: privilege_encoder gives {pe.widths[-1]} latent dims, history_encoder {he.widths[-1]}")
        if actor.widths[0] <= pe.widths[-1]:
            raise ValueError(f"FusedPolicy: actor[0] takes {actor.widths[0]} inputs, the latent alone has {pe.widths[-1]}")
        return PolicySpec(None, actor, critic, std, privilege_encoder=pe, history_encoder=he)
    if vae is not None:
        enc = nets.describe_chain("vae.encoder", getattr(vae, "encoder", None), device, False, _OWNER, allow_last_elu=True)
        head = nets.describe_heads(vae, enc.widths[-1], device, _OWNER)
        if actor.widths[0] <= head.L + head.E:
            raise ValueError(f"FusedPolicy: actor[0] takes {actor.widths[0]} inputs, (z, vel) alone has {head.L} + {head.E}")
        return PolicySpec(None, actor, critic, std, vae_encoder=enc, head=head)
    if estimator is not None and actor.widths[0] != estimator.widths[0] + estimator.widths[-1]:
        raise ValueError(f"FusedPolicy: actor[0] takes {actor.widths[0]} inputs, (features, estimator output) has "
                         f"{estimator.widths[0]} + {estimator.widths[-1]}")
    return PolicySpec(estimator, actor, critic, std)


def _fill_chain(dst, spec, inp, in_width, out):
    dst.n_layers = len(spec.linears)
    dst.input, dst.in_stride = inp
    dst.in_width = in_width
    dst.out, dst.out_stride = out if out is not None else (None, 0)
    for l, m, e in zip(dst.layer, spec.linears, spec.elu):
        l.weight, l.bias, l.n_in, l.n_out, l.elu = m.weight.data.data_ptr(), m.bias.data.data_ptr(), m.in_features, m.out_features, int(e)


MEMORY_KEYS = ("h_a", "c_a", "h_c", "c_c", "h_prev_a", "c_prev_a", "h_prev_c", "c_prev_c", "reset")


def _fill_memory(dst, ms, which, inp, memory, n, device):
    """LgPolicyMemory of `ms` (memory_a / memory_c: `which` is "a" / "c"): parameters and states addressed in place."""
    dst.kind = abi.POLICY_LSTM if ms.kind == "lstm" else abi.POLICY_GRU
    dst.n_layers, dst.hidden, dst.in_width = ms.layers, ms.hidden, ms.input_size
    if inp is not None:
        dst.input, dst.in_stride = inp
        for k in range(ms.layers):
            l = dst.layer[k]
            l.weight_ih, l.weight_hh, l.bias_ih, l.bias_hh = (t.data_ptr() for t in ms.params(k))
    shape = (ms.layers, n, ms.hidden)
    for field, key, need in (("h", "h_" + which, True), ("c", "c_" + which, ms.kind == "lstm"), ("h_prev_out", "h_prev_" + which, False),
                             ("c_prev_out", "c_prev_" + which, False)):
        t = (memory or {}).get(key)
        if t is None:
            if need:
                raise ValueError(f"FusedPolicy: the state {key} of {ms.name} is missing")
            continue
        if field.startswith("c") and ms.kind != "lstm":
            raise ValueError(f"FusedPolicy: {key} was given, {ms.name}.rnn is a GRU and has no cell state")
        if (not torch.is_tensor(t) or t.dtype != torch.float32 or tuple(t.shape) != shape or not t.is_contiguous()
                or (device is not None and t.device != device)):
            got = f"{tuple(t.shape)} {t.dtype} on {t.device}" if torch.is_tensor(t) else type(t).__name__
            raise ValueError(f"FusedPolicy: {key} must be a contiguous {shape} float32 tensor" + (f" on {device}" if device is not None else "")
                             + f", got {got}")
        setattr(dst, field, t.data_ptr())
    mask = (memory or {}).get("reset")
    if mask is not None:
        dst.reset_mask = _mask(mask, n, device).data_ptr()


def _mask(mask, n, device):
    """A reset mask as the kernel reads it: (N,) bool or uint8, contiguous, on the device; any non-zero byte is "done"."""
    if (not torch.is_tensor(mask) or mask.dtype not in (torch.bool, torch.uint8) or mask.numel() != n or not mask.is_contiguous()
            or (device is not None and mask.device != device)):
        got = f"{tuple(mask.shape)} {mask.dtype} on {mask.device}" if torch.is_tensor(mask) else type(mask).__name__
        raise ValueError(f"FusedPolicy: reset must be a mask of {n} contiguous bool / uint8 elements" + (f" on {device}" if device is not None else "")
                         + f" (not a list of indices), got {got}")
    return mask


def _family_inputs(spec, n, privileged_obs, obs_history, num_teacher, student, latent_noise, latent, latent_params, dbg_latent_uniform):
    """Which keyword arguments the module's family takes; every refusal names the argument.  Returns (leading chain, its rows,
    second chain or None, its rows) for the TS family, None otherwise."""
    fam = spec.family
    if fam != "dreamwaq":
        for k, v in (("latent_noise", latent_noise), ("latent", latent), ("latent_params", latent_params), ("dbg_latent_uniform", dbg_latent_uniform)):
            if v is not None:
                raise ValueError(f"FusedPolicy: {k} was given, the module has no .vae")
    if fam != "ts":
        for k, v in (("privileged_obs", privileged_obs), ("num_teacher", num_teacher), ("student", student or None)):
            if v is not None:
                raise ValueError(f"FusedPolicy: {k} was given, the module has no .privilege_encoder / .history_encoder")
    if fam in ("plain", "ee") and obs_history is not None:
        raise ValueError("FusedPolicy: obs_history was given, the module has neither a .history_encoder nor a .vae")
    if fam == "dreamwaq" and obs_history is None:
        raise ValueError("FusedPolicy: obs_history is missing: the VAE's encoder reads it")
    if fam != "ts":
        return None
    if spec.history_encoder is None and (student or num_teacher is not None):
        raise ValueError("FusedPolicy: " + ("the student call" if student else "num_teacher") + " runs the history encoder, which student=False left "
                         "unread; build the FusedPolicy with student=True (a Conv1d history encoder keeps act_student on torch)")
    if num_teacher is not None:
        if student:
            raise ValueError("FusedPolicy: num_teacher and the student call exclude each other")
        if isinstance(num_teacher, bool) or int(num_teacher) != num_teacher or not 0 <= int(num_teacher) <= n:
            raise ValueError(f"FusedPolicy: num_teacher={num_teacher} is outside [0, {n}]")
        for k, v in (("privileged_obs", privileged_obs), ("obs_history", obs_history)):
            if v is None:
                raise ValueError(f"FusedPolicy: {k} is missing: with num_teacher both encoders run, each on its rows")
        return spec.privilege_encoder, privileged_obs, spec.history_encoder, obs_history
    if student:
        if obs_history is None:
            raise ValueError("FusedPolicy: obs_history is missing: the history encoder reads it")
        return spec.history_encoder, obs_history, None, None
    if privileged_obs is None:
        raise ValueError("FusedPolicy: privileged_obs is missing: the privilege encoder reads it")
    return spec.privilege_encoder, privileged_obs, None, None


def policy_args(spec, obs, critic_obs=None, actions=None, mu=None, sigma=None, log_prob=None, values=None, labels=None, noise=None,
                counter=None, seed=0, flags=0, dbg_uniform=None, device=None, privileged_obs=None, obs_history=None, num_teacher=None,
                student=False, latent_noise=None, latent=None, latent_params=None, dbg_latent_uniform=None, memory=None):
    """The LgPolicyArgs of one call.  Every tensor is addressed in place; nothing is copied and the library is not touched.  `memory`
    (recurrent modules): a dict of the MEMORY_KEYS -- the live states `h_a`, `c_a`, `h_c`, `c_c` ((layers, N, H); c for an LSTM only),
    optional snapshot destinations `h_prev_*` / `c_prev_*` and the optional `reset` mask; only the memories this call runs are filled."""
    a = abi.LgPolicyRecurrentArgs() if spec.family == "recurrent" else abi.LgPolicyArgs()     # the first with the memories behind the second
    if spec.family != "recurrent" and memory:
        raise ValueError("FusedPolicy: hidden states were given, the module has no .memory_a / .memory_c")
    A = spec.num_actions
    values_only, determ = bool(flags & abi.POLICY_VALUES_ONLY), bool(flags & abi.POLICY_DETERMINISTIC)
    a.flags = flags
    n = int((critic_obs if values_only else obs).shape[0])
    a.n_envs = n
    if not values_only:
        ts = _family_inputs(spec, n, privileged_obs, obs_history, num_teacher, student, latent_noise, latent, latent_params, dbg_latent_uniform)
        F = spec.obs_width
        if spec.family in ("ts", "dreamwaq") and torch.is_tensor(obs) and obs.dim() == 2 and obs.shape[1] != F:
            raise ValueError(f"FusedPolicy: actor[0] takes {spec.actor.widths[0]} inputs, (obs, latent) has {obs.shape[1]} + {spec.latent_width}")
        src = nets.rows(obs, F, "obs", None, device, _OWNER)
        if spec.concat:
            E = spec.estimator.widths[-1]
            _fill_chain(a.estimator, spec.estimator, src, F, None if labels is None else nets.rows(labels, E, "labels", n, device, _OWNER))
        elif labels is not None:
            raise ValueError("FusedPolicy: a labels row was given, the module has no estimator")
        if ts is not None:
            lead, rows, lead_b, rows_b = ts
            what = "privileged_obs" if lead is spec.privilege_encoder else "obs_history"
            _fill_chain(a.estimator, lead, nets.rows(rows, lead.widths[0], what, n, device, _OWNER), lead.widths[0], None)
            if lead_b is not None:
                _fill_chain(a.encoder_b, lead_b, nets.rows(rows_b, lead_b.widths[0], "obs_history", n, device, _OWNER), lead_b.widths[0], None)
                a.n_split, a.has_split = int(num_teacher), 1
        if spec.family == "dreamwaq":
            enc, h = spec.vae_encoder, spec.head
            _fill_chain(a.estimator, enc, nets.rows(obs_history, enc.widths[0], "obs_history", n, device, _OWNER), enc.widths[0], None)
            hd = a.head
            for name, m in zip(nets.HEADS, h.linears):
                setattr(hd, name + "_w", m.weight.data.data_ptr())
                setattr(hd, name + "_b", m.bias.data.data_ptr())
            hd.H, hd.L, hd.E, hd.logvar_clip = h.H, h.L, h.E, h.clip
            if latent is not None:
                hd.latent_out, hd.latent_stride = nets.rows(latent, h.L + h.E, "latent", n, device, _OWNER)
            if latent_params is not None:
                hd.params_out, hd.params_stride = nets.rows(latent_params, 2 * (h.L + h.E), "latent_params", n, device, _OWNER)
            if not determ:
                if latent_noise is not None:
                    hd.noise, hd.noise_stride = nets.rows(latent_noise, h.L + h.E, "latent_noise", n, device, _OWNER)
                elif dbg_latent_uniform is not None:
                    if not dbg_latent_uniform.is_contiguous():
                        raise ValueError("FusedPolicy: the debug uniforms must be a contiguous (N, 4 * ceil((L + E) / 4)) float32 tensor")
                    hd.dbg_latent_uniform = nets.rows(dbg_latent_uniform, 4 * ((h.L + h.E + 3) // 4), "dbg_latent_uniform", n, device, _OWNER)[0]
        _fill_chain(a.actor, spec.actor, src, F, None)
        if spec.family == "recurrent":
            _fill_memory(a.memory_a, spec.memory_a, "a", src, memory, n, device)
        a.mu, a.mu_stride = nets.rows(mu, A, "mu", n, device, _OWNER)
        if spec.clip_actions is not None:
            a.clip_on, a.clip_actions = 1, spec.clip_actions
        if not determ:
            a.std = spec.std.data.data_ptr()
            a.actions, a.actions_stride = nets.rows(actions, A, "actions", n, device, _OWNER)
            a.sigma, a.sigma_stride = nets.rows(sigma, A, "sigma", n, device, _OWNER)
            a.log_prob, a.log_prob_stride = nets.rows(log_prob, 1, "log_prob", n, device, _OWNER)
            if noise is not None:
                a.noise, a.noise_stride = nets.rows(noise, A, "noise", n, device, _OWNER)
            if noise is None or (spec.family == "dreamwaq" and latent_noise is None):
                a.counter, a.seed = counter.data_ptr(), int(seed) & (2 ** 64 - 1)
            if noise is None and dbg_uniform is not None:    # the kernel writes it densely: no stride is carried
                if not dbg_uniform.is_contiguous():
                    raise ValueError("FusedPolicy: the debug uniforms must be a contiguous (N, 4 * ceil(A / 4)) float32 tensor")
                a.dbg_uniform = nets.rows(dbg_uniform, 4 * ((A + 3) // 4), "dbg_uniform", n, device, _OWNER)[0]
    if critic_obs is not None and not determ:
        csrc = nets.rows(critic_obs, spec.critic_obs_width, "critic_obs", n, device, _OWNER)
        _fill_chain(a.critic, spec.critic, csrc, spec.critic_obs_width, nets.rows(values, 1, "values", n, device, _OWNER))
        if spec.family == "recurrent":
            _fill_memory(a.memory_c, spec.memory_c, "c", csrc, memory, n, device)
    return a


class FusedPolicy:
    """`FusedPolicy(actor_critic, seed=...)`; `act`, `act_inference`, `act_teacher`, `act_student`, `evaluate`, `fill_transition`; for a
    recurrent module also `reset`, `get_hidden_states`, `set_hidden_states` and `last_hidden_states`.  See the module docstring."""

    def __init__(self, actor_critic, seed=0, device=None, student=True):
        std = getattr(actor_critic, "std", None)
        dev = torch.device(device) if device is not None else (std.device if torch.is_tensor(std) else torch.device("cpu"))
        if dev.type != "cuda":
            raise ValueError(f"FusedPolicy: the module is on {dev}, not on a HIP device (there is no CPU path)")
        if dev.index is None:
            dev = torch.device("cuda", torch.cuda.current_device())
        self.device = dev
        self.module = actor_critic
        self.student = bool(student)                     # False: a TS module's history encoder is never read (it may be a "TCN")
        self.spec = describe(actor_critic, dev, self.student)          # every refusal comes before the library is loaded
        self.seed = int(seed)
        self.lib = abi.load_lib()
        self.counter = torch.zeros(1, dtype=torch.int32, device=dev)        # the Philox call counter (read as uint32)
        self._own = {}
        self._args = {}
        self.last_actions = self.last_mu = self.last_sigma = self.last_log_prob = self.last_values = self.last_labels = None
        self.last_latent = self.last_latent_params = None
        self.last_hidden_states = None                   # recurrent: the state the last call started from (after its reset mask)
        self._states = {}
        self._reset_args = {}
        self._n = None                                   # N of the last recurrent call: whose states the state methods mean by default

    # ---- launches ------------------------------------------------------------------------------------------------------
    def _param_key(self):
        """Identity of every layer object of the LIVE module and the address of every parameter: a replaced layer
        (`module.actor[0] = nn.Linear(...)`), a moved parameter or a reassigned `.data` all miss the descriptor cache."""
        key = []
        vae = getattr(self.module, "vae", None)
        subs = [getattr(self.module, name, None) for name in ("estimator", "actor", "critic", "privilege_encoder", "history_encoder")]
        subs += [vae] + [getattr(vae, name, None) for name in ("encoder", "latent_mu", "latent_var", "vel_mu", "vel_var")]
        for seq in subs:
            key.append(id(seq))
            for m in (seq if isinstance(seq, nn.Sequential) else (seq,) if isinstance(seq, nn.Linear) else ()):
                key.append(id(m))
                if isinstance(m, nn.Linear):
                    key += [m.weight.data.data_ptr(), 0 if m.bias is None else m.bias.data.data_ptr()]
        for mem in (getattr(self.module, name, None) for name in ("memory_a", "memory_c")):
            rnn = getattr(mem, "rnn", None)
            key += [id(mem), id(rnn)]
            if isinstance(rnn, nn.RNNBase):              # a replaced rnn or a re-flattened parameter misses the cache
                key += [p.data.data_ptr() for p in rnn.parameters()]
        key.append(self.module.std.data.data_ptr())
        return tuple(key)

    def _launch(self, flags, num_teacher=None, student=False, **t):
        """Build (or reuse) the descriptor of this call and enqueue it on the current stream.  The descriptor is keyed by every address
        and stride it holds and by the module's layer objects, so a parameter that moved or a layer that was replaced is seen (the module
        is then described again, with every refusal); the parameters' CONTENTS are read by the kernel each call."""
        key = (flags, num_teacher, student, self._param_key()) + tuple((k, v.data_ptr(), v.stride(0), v.shape[0]) for k, v in sorted(t.items())
                                                                         if torch.is_tensor(v))
        a = self._args.get(key)
        if a is None:
            self.spec = describe(self.module, self.device, self.student)
            if len(self._args) >= 256:
                self._args.clear()
            a = self._args[key] = policy_args(self.spec, t.get("obs"), t.get("critic_obs"), t.get("actions"), t.get("mu"), t.get("sigma"),
                                              t.get("log_prob"), t.get("values"), t.get("labels"), t.get("noise"), self.counter, self.seed, flags,
                                              t.get("dbg_uniform"), self.device, t.get("privileged_obs"), t.get("obs_history"), num_teacher, student,
                                              t.get("latent_noise"), t.get("latent"), t.get("latent_params"), t.get("dbg_latent_uniform"),
                                              {k: t[k] for k in MEMORY_KEYS if t.get(k) is not None})
        act = self.lib.lg_policy_act_recurrent if isinstance(a, abi.LgPolicyRecurrentArgs) else self.lib.lg_policy_act
        abi.check(act(C.byref(a), torch.cuda.current_stream(self.device).cuda_stream), self.lib)

    def _buffers(self, n):
        b = self._own.get(n)
        if b is None:
            A, z = self.spec.num_actions, lambda w: torch.zeros(n, w, device=self.device)
            b = self._own[n] = dict(actions=z(A), mu=z(A), sigma=z(A), log_prob=z(1), values=z(1), inference=z(A), student=z(A), evaluate=z(1),
                                    labels=z(self.spec.estimator.widths[-1]) if self.spec.concat else None)
        return b

    # ---- hidden states (recurrent modules) ---------------------------------------------------------------------------------
    def _state(self, n=None):
        """The states of batch size n (default: the last call's): zeros (layers, N, H) allocated once, then only ever updated in place, and
        the snapshot buffers the kernel fills when no storage row takes them."""
        sp = self.spec
        if sp.family != "recurrent":
            raise ValueError("FusedPolicy: the module has no .memory_a / .memory_c: there are no hidden states")
        n = self._n if n is None else int(n)
        if n is None:
            raise ValueError("FusedPolicy: no call has fixed the number of envs yet; pass n")
        st = self._states.get(n)
        if st is None:
            st = self._states[n] = {}
            for w, ms in (("a", sp.memory_a), ("c", sp.memory_c)):
                for name in ("h", "c") if ms.kind == "lstm" else ("h",):
                    st[f"{name}_{w}"] = torch.zeros(ms.layers, n, ms.hidden, device=self.device)
                    st[f"{name}_prev_{w}"] = torch.zeros(ms.layers, n, ms.hidden, device=self.device)
        self._n = n
        return st

    def _as_reference(self, st, prefix=""):
        lstm = self.spec.memory_a.kind == "lstm"
        one = lambda w: (st[f"h_{prefix}{w}"], st[f"c_{prefix}{w}"]) if lstm else st[f"h_{prefix}{w}"]
        return one("a"), one("c")

    def get_hidden_states(self, n=None):
        """The LIVE states in the reference's form (actor_critic_recurrent.py:88-89): ((h_a, c_a), (h_c, c_c)) for an LSTM, (h_a, h_c) for a
        GRU, each (layers, N, H); what `RolloutStorage._hidden_copies` accepts as is.  The kernel updates them in place."""
        return self._as_reference(self._state(n))

    def set_hidden_states(self, hidden_states, n=None):
        """Copy states given in the form of `get_hidden_states` into the live tensors (their addresses stay)."""
        if n is None and self._n is None:
            first = hidden_states[0]
            n = (first[0] if isinstance(first, (tuple, list)) else first).shape[1]
        for dst, src in zip(self.get_hidden_states(n), hidden_states):
            for d, x in zip(dst if isinstance(dst, tuple) else (dst,), src if isinstance(src, (tuple, list)) else (src,)):
                if tuple(x.shape) != tuple(d.shape):
                    raise ValueError(f"FusedPolicy: hidden state of shape {tuple(x.shape)} given, the live one is {tuple(d.shape)}")
                d.copy_(x)

    def reset(self, dones=None, n=None):
        """actor_critic_recurrent.py:72-74 as one launch: zero the state rows of finished envs in every state tensor of both memories.
        `dones` is an (N,) bool / uint8 MASK on the device, read in place (any non-zero byte is "done"); None zeroes every row."""
        st = self._state(n)
        n = self._n
        a = self._reset_args.get(n)
        if a is None:
            a = self._reset_args[n] = abi.LgPolicyRecurrentArgs()
            a.n_envs = n
            for dst, ms, w in ((a.memory_a, self.spec.memory_a, "a"), (a.memory_c, self.spec.memory_c, "c")):
                _fill_memory(dst, ms, w, None, {k: st[k] for k in (f"h_{w}", f"c_{w}") if k in st}, n, self.device)
        mask = None if dones is None else _mask(dones, n, self.device).data_ptr()
        abi.check(self.lib.lg_policy_reset(C.byref(a), mask, torch.cuda.current_stream(self.device).cuda_stream), self.lib)

    def _memory(self, n, which, reset=None, rows=None):
        """The memory keywords of one launch: the live states of the memories in `which` ("a", "c" or "ac"), where the pre-step snapshot
        goes (storage rows `rows`, or this object's buffers) and the reset mask; sets `last_hidden_states`."""
        st = self._state(n)
        kw, snap = {}, dict(st)
        for i, w in enumerate("ac"):
            names = [k for k in (f"h_{w}", f"c_{w}") if k in st]
            for j, k in enumerate(names):
                prev = k.replace("_", "_prev_")
                if rows is not None and w in which:
                    snap[prev] = rows[i][j]
                if w in which:
                    kw[k], kw[prev] = st[k], snap[prev]
        if reset is not None:
            kw["reset"] = reset
        self.last_hidden_states = self._as_reference(snap, "prev_")
        return kw

    def act(self, obs, critic_obs, storage=None, noise=None, labels=None, _dbg_uniform=None, privileged_obs=None, obs_history=None,
            num_teacher=None, latent_noise=None, latent=None, latent_params=None, _dbg_latent_uniform=None, reset=None):
        """Sample actions for `obs` ((N, F): the actor's input, or the estimator features of an explicit-estimator module) and evaluate the
        critic on `critic_obs` (None: no critic launch, no values written).  With a `RolloutStorage` (any of the family's) the five results
        go straight into row `storage.step` -- actions, mu, sigma, actions_log_prob, values: the rows `add_step` leaves to the caller --
        and the returned actions ARE that row; with zero-copy observation rows `obs` already is `storage.observations[storage.step]`, so
        nothing is copied at all.  Without a storage the results land in buffers this object owns (`last_mu`, `last_sigma`,
        `last_log_prob`, `last_values`; overwritten by the next call of the same N).  `noise` ((N, A), e.g. torch.randn) replaces the Philox
        draw.  `labels` ((N, E), e.g. `storage.estimator_labels[t]`-shaped) receives the estimator's output.

        By family (a keyword of another family, or a missing one, is a ValueError that names it):
          TS        act(obs, critic_obs, privileged_obs=...): latent = privilege_encoder(privileged_obs), as PPO_TS.act.
          CTS       act(obs, critic_obs, privileged_obs=..., obs_history=..., num_teacher=k): full-N tensors; env rows [0, k) take the
                    privilege encoder, the others the history encoder, in the one launch (ppo_cts.py:115-127).  With a
                    `RolloutStorageCTS`, `num_teacher` defaults to the storage's.  WITHOUT `num_teacher` (and without such a storage)
                    the call is the TS one: every row takes the privilege encoder and a given `obs_history` is IGNORED -- it is
                    accepted only because PPO_TS.act is handed one (and stores it); nothing here reads it.
          DreamWaQ  act(obs, critic_obs, obs_history=..., latent_noise=None, latent=None, latent_params=None): `latent_noise` ((N, L + E),
                    columns (z, vel)) replaces the Philox draw of the reparameterisation; `latent` ((N, L + E)) receives the samples
                    (z, vel) and `latent_params` ((N, 2L + 2E)) latent_mu, latent_logvar, vel_mu, vel_logvar (clipped).
          recurrent act(obs, critic_obs, reset=None): both memories advance one step on their live states (as `actor_critic.act` and
                    `evaluate` of PPO.act do).  `reset` ((N,) bool / uint8 mask on the device, read in place, e.g. the env's reset_buf or
                    the dones of the step before; any non-zero byte counts) folds `reset(dones)` into the launch: those rows start from
                    zero states.  It needs `critic_obs`: a call that runs one memory only would lose the other's reset.  The states the
                    call started from (after the mask) are `last_hidden_states`; with a storage they are written straight into row
                    `storage.step` of `saved_hidden_states_a` / `_c`, so `add_step` needs no `hidden_states`.
        (`_dbg_uniform` / `_dbg_latent_uniform`, for the tests: contiguous (N, 4 * ceil(A / 4)) / (N, 4 * ceil((L + E) / 4)) tensors that
        receive the uniforms of the Philox draws.)"""
        n = int(obs.shape[0])
        if storage is not None:
            t = storage.step
            if t >= storage.num_transitions_per_env:
                raise AssertionError("Rollout buffer overflow")
            d = dict(actions=storage.actions[t], mu=storage.mu[t], sigma=storage.sigma[t], log_prob=storage.actions_log_prob[t],
                     values=storage.values[t])
            if num_teacher is None and self.spec.family == "ts":
                num_teacher = getattr(storage, "num_teacher", None)
        else:
            d = self._buffers(n)
        if labels is not None and not self.spec.concat:
            raise ValueError("FusedPolicy: a labels row was given, the module has no estimator")
        if num_teacher is None and self.spec.family == "ts":
            obs_history = None                               # the teacher's call: the history is the learner's, nothing here reads it
        values = d["values"] if critic_obs is not None else None
        mem = {}
        if self.spec.family == "recurrent":
            if reset is not None and critic_obs is None:
                raise ValueError("FusedPolicy: reset= needs critic_obs: a call that runs memory_a alone would lose memory_c's reset "
                                 "(use reset(dones) instead)")
            rows = None if storage is None else storage.hidden_state_rows(self.get_hidden_states(n))
            mem = self._memory(n, "ac" if critic_obs is not None else "a", reset, rows)
        elif reset is not None:
            raise ValueError("FusedPolicy: reset was given, the module has no .memory_a / .memory_c")
        self._launch(0, num_teacher, **mem, obs=obs, critic_obs=critic_obs, actions=d["actions"], mu=d["mu"], sigma=d["sigma"], log_prob=d["log_prob"],
                     values=values, labels=labels, noise=noise, dbg_uniform=_dbg_uniform, privileged_obs=privileged_obs, obs_history=obs_history,
                     latent_noise=latent_noise, latent=latent, latent_params=latent_params, dbg_latent_uniform=_dbg_latent_uniform)
        self.last_actions, self.last_mu, self.last_sigma, self.last_log_prob = d["actions"], d["mu"], d["sigma"], d["log_prob"]
        self.last_values, self.last_labels = values, labels
        self.last_latent, self.last_latent_params = latent, latent_params
        return d["actions"]

    def act_inference(self, obs, obs_history=None, latent=None):
        """The clipped mean alone (actor_critic.py act_inference): no draw, no critic.  DreamWaQ: `act_inference(obs, obs_history)`, the
        actor on [obs | latent_mu | vel_mu] (actor_critic_dreamwaq.py:165-171); `latent` ((N, L + E)) receives those means."""
        mu = self._buffers(int(obs.shape[0]))["inference"]
        mem = self._memory(int(obs.shape[0]), "a") if self.spec.family == "recurrent" else {}     # memory_a advances, memory_c is not touched
        self._launch(abi.POLICY_DETERMINISTIC, **mem, obs=obs, mu=mu, obs_history=obs_history, latent=latent)
        return mu

    def act_teacher(self, obs, privileged_obs):
        """TS / CTS: the mean with the privilege encoder's latent (actor_critic_ts.py:178-184)."""
        mu = self._buffers(int(obs.shape[0]))["inference"]
        self._launch(abi.POLICY_DETERMINISTIC, obs=obs, mu=mu, privileged_obs=privileged_obs)
        return mu

    def act_student(self, obs, obs_history):
        """TS / CTS: the mean with the history encoder's latent (actor_critic_ts.py:186-195).  Under `student=False` this raises: the
        history encoder was not read.  For a Conv1d "TCN" history encoder act_student stays on torch (module.act_student): it is play-time
        only, PPO_TS's rollout never runs the history encoder."""
        if not self.student:
            raise ValueError("FusedPolicy: act_student runs the history encoder, which student=False left unread; build the FusedPolicy with "
                             "student=True (a Conv1d history encoder keeps act_student on torch)")
        mu = self._buffers(int(obs.shape[0]))["student"]
        self._launch(abi.POLICY_DETERMINISTIC, None, True, obs=obs, mu=mu, obs_history=obs_history)
        return mu

    def evaluate(self, critic_obs):
        """The critic alone (`compute_returns`' last value)."""
        v = self._buffers(int(critic_obs.shape[0]))["evaluate"]
        mem = self._memory(int(critic_obs.shape[0]), "c") if self.spec.family == "recurrent" else {}   # memory_c advances, as in compute_returns
        self._launch(abi.POLICY_VALUES_ONLY, **mem, critic_obs=critic_obs, values=v)
        return v

    def fill_transition(self, transition, obs, critic_obs, noise=None, privileged_obs=None, obs_history=None, num_teacher=None,
                        latent_noise=None, latent=None, latent_params=None, explicit_info_labels=None, reset=None):
        """What rsl_rl's PPO.act (ppo.py:97-104) does to `self.transition`, from one launch; returns the actions.  The TS family fills what
        PPO_TS / PPO_CTS.act fill (ppo_ts.py:81-92: also privileged_observations and observation_histories), DreamWaQ what PPO_DreamWaQ.act
        fills (ppo_dreamwaq.py:127-137: `critic_obs` is its privileged observations; explicit_info_labels is passed through).  A recurrent
        module also gets `transition.hidden_states` (ppo.py:94-95): the states the call started from, after `reset`."""
        transition.actions = self.act(obs, critic_obs, noise=noise, privileged_obs=privileged_obs, obs_history=obs_history, num_teacher=num_teacher,
                                      latent_noise=latent_noise, latent=latent, latent_params=latent_params, reset=reset)
        if self.spec.family == "recurrent":
            transition.hidden_states = self.last_hidden_states
        transition.values = self.last_values
        transition.actions_log_prob = self.last_log_prob.view(-1)
        transition.action_mean = self.last_mu
        transition.action_sigma = self.last_sigma
        transition.observations = obs
        if self.spec.family == "dreamwaq":
            transition.privileged_observations = critic_obs
            transition.observation_histories = obs_history
            transition.explicit_info_labels = explicit_info_labels
            return transition.actions
        transition.critic_observations = critic_obs
        if self.spec.family == "ts":
            transition.privileged_observations = privileged_obs
            transition.observation_histories = obs_history
        return transition.actions

    def row_tile(self, n=1, num_teacher=None):
        """Env rows one workgroup carries for this module (32, 16 or 8): the kernel's choice, for documentation and tools."""
        b = self._buffers(n)
        sp, z = self.spec, lambda w: torch.zeros(n, w, device=self.device)
        kw = {}
        if sp.family == "ts":
            kw = dict(privileged_obs=z(sp.privilege_encoder.widths[0]), num_teacher=num_teacher)
            if num_teacher is not None:
                kw["obs_history"] = z(sp.history_encoder.widths[0])
        elif sp.family == "dreamwaq":
            kw = dict(obs_history=z(sp.vae_encoder.widths[0]))
        if sp.family == "recurrent":
            n_before = self._n
            kw = dict(memory={k: v for k, v in self._state(n).items() if "_prev_" not in k})
            self._n = n_before
        a = policy_args(sp, z(sp.obs_width), z(sp.critic_obs_width), b["actions"], b["mu"], b["sigma"], b["log_prob"], b["values"],
                        counter=self.counter, device=self.device, **kw)
        r = (self.lib.lg_policy_row_tile_recurrent if isinstance(a, abi.LgPolicyRecurrentArgs) else self.lib.lg_policy_row_tile)(C.byref(a))
        if r == 0:
            abi.check(1, self.lib)
        return r
