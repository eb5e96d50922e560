"""What a network is before a kernel sees it: the one reader of the torch modules behind FusedPolicy (policy.py) and the train passes
(train.py).  A chain is an `nn.Sequential` of `Linear` (with bias, float32, contiguous, widths and depth within include/lgpolicy.h's
limits), `ELU(alpha=1)` behind a Linear and, where the caller allows it, a symmetric `Hardtanh` as its last module; the four heads of a
DreamWaQ VAE are one-layer chains, the two log-variances behind one symmetric clip.  A change to what the kernels accept -- an activation,
a width limit -- is made here once.

Every function takes the `owner` that begins its refusals ("FusedPolicy", "FusedTrainPassTS", ...): a refusal carries the name of the
surface the caller used.  Nothing here touches the library or the device; which members a module family has, and what must hold between
its chains, stays with the two callers."""
from __future__ import annotations

import torch
import torch.nn as nn

from . import abi

HEADS = ("latent_mu", "latent_var", "vel_mu", "vel_var")       # abi.TRAIN_DWAQ_LATENT_MU + h, and the order of vae.parameters()


class ChainSpec:
    """One MLP chain as the kernel takes it: its Linear modules in order, which of them an ELU follows, and (actor only) the clip."""

    def __init__(self, name, linears, elu, clip):
        self.name, self.linears, self.elu, self.clip = name, linears, elu, clip

    @property
    def widths(self):
        return [self.linears[0].in_features] + [l.out_features for l in self.linears]


class HeadSpec:
    """The four heads of a DreamWaQ VAE (rsl_rl/modules/vae.py:40-50) as one-layer chains in HEADS order, and the symmetric clip of the
    two log-variances; H -> L, L, E, E."""

    def __init__(self, chains, clip):
        self.chains, self.clip = chains, clip
        self.H, self.L, self.E = chains[0].widths[0], chains[0].widths[-1], chains[2].widths[-1]

    @property
    def linears(self):
        return tuple(c.linears[0] for c in self.chains)


def check_tensor(t, what, device, owner):
    """A parameter as the kernels read it: float32, contiguous and (unless `device` is None) on `device`."""
    if not isinstance(t, torch.Tensor) or t.dtype != torch.float32:
        raise ValueError(f"{owner}: {what} is {getattr(t, 'dtype', type(t).__name__)}, the kernel reads float32")
    if not t.is_contiguous():
        raise ValueError(f"{owner}: {what} is not contiguous")
    if device is not None and t.device != device:
        raise ValueError(f"{owner}: {what} is on {t.device}, not on {device}")


def _check_linear(m, where, device, owner):
    if m.bias is None:
        raise ValueError(f"{owner}: {where} has no bias")
    if m.in_features > abi.POLICY_MAX_WIDTH or m.out_features > abi.POLICY_MAX_WIDTH:
        raise ValueError(f"{owner}: {where} is {m.in_features} -> {m.out_features}, widths are limited to {abi.POLICY_MAX_WIDTH}")
    check_tensor(m.weight, f"{where}.weight", device, owner)
    check_tensor(m.bias, f"{where}.bias", device, owner)


def describe_chain(name, seq, device, allow_clip, owner, allow_last_elu=False, index0=0):
    """The ChainSpec of `seq`, or the refusal that names its layer.  `allow_clip`: a symmetric Hardtanh may end it (the actor);
    `allow_last_elu`: an ELU may (the DreamWaQ encoder); `index0`: the index of seq[0] in the module the refusals name (a TCN's tail)."""
    if not isinstance(seq, nn.Sequential):
        raise ValueError(f"{owner}: {name} is {type(seq).__name__}, expected an nn.Sequential of Linear / ELU"
                         + (" / Hardtanh" if allow_clip else ""))
    linears, elu, clip = [], [], None
    mods = list(seq)
    for i, m in enumerate(mods):
        where = f"{name}[{i + index0}]"
        if clip is not None:
            raise ValueError(f"{owner}: {where} ({type(m).__name__}) follows the Hardtanh, which must end the actor")
        if isinstance(m, nn.Linear):
            _check_linear(m, where, device, owner)
            if linears and linears[-1].out_features != m.in_features:
                raise ValueError(f"{owner}: {where} takes {m.in_features} inputs, the layer before it gives {linears[-1].out_features}")
            linears.append(m)
            elu.append(False)
        elif isinstance(m, nn.ELU):
            if not linears or elu[-1]:
                raise ValueError(f"{owner}: {where} (ELU) does not follow a Linear")
            if m.alpha != 1.0:
                raise ValueError(f"{owner}: {where} is ELU(alpha={m.alpha}), only alpha = 1 is built")
            elu[-1] = True
        elif isinstance(m, nn.Hardtanh) and allow_clip:
            if i != len(mods) - 1 or not linears or elu[-1] or m.min_val != -m.max_val or not m.max_val >= 0:
                raise ValueError(f"{owner}: {where} (Hardtanh({m.min_val}, {m.max_val})) must be the symmetric clip behind the actor's last Linear")
            clip = float(m.max_val)
        else:
            raise ValueError(f"{owner}: {where} is {type(m).__name__}; only Linear and ELU"
                             + (" (and a final Hardtanh)" if allow_clip else "") + " are built into the kernel")
    if not linears:
        raise ValueError(f"{owner}: {name} has no Linear layer")
    if len(linears) > abi.POLICY_MAX_LAYERS:
        raise ValueError(f"{owner}: {name} has {len(linears)} Linear layers, the kernel takes {abi.POLICY_MAX_LAYERS}")
    if elu[-1] and not allow_last_elu:
        raise ValueError(f"{owner}: {name} ends in an ELU, expected a Linear output layer")
    return ChainSpec(name, linears, elu, clip)


def describe_heads(vae, enc_width, device, owner):
    """The HeadSpec of `vae`'s four heads behind an encoder that ends at `enc_width` columns: a Linear each, the two log-variances
    behind one symmetric Hardtanh; mean and log-variance of one width."""
    chains, clips = [], {}
    for name in HEADS:
        m, where = getattr(vae, name, None), f"vae.{name}"
        if name.endswith("_var"):
            if not isinstance(m, nn.Sequential) or len(m) != 2 or not isinstance(m[0], nn.Linear) or not isinstance(m[1], nn.Hardtanh):
                raise ValueError(f"{owner}: {where} is not Sequential(Linear, Hardtanh): the log-variance head of the VAE")
            if m[1].min_val != -m[1].max_val or not m[1].max_val >= 0:
                raise ValueError(f"{owner}: {where}[1] (Hardtanh({m[1].min_val}, {m[1].max_val})) must be a symmetric clip")
            clips[name], m, where = float(m[1].max_val), m[0], where + "[0]"
        if not isinstance(m, nn.Linear):
            raise ValueError(f"{owner}: {where} is {type(m).__name__}, expected a Linear")
        _check_linear(m, where, device, owner)
        chains.append(ChainSpec(name, [m], [False], None))
    if clips["latent_var"] != clips["vel_var"]:
        raise ValueError(f"{owner}: vae.latent_var clips to {clips['latent_var']}, vae.vel_var to {clips['vel_var']}; the kernel takes one clip")
    head = HeadSpec(tuple(chains), clips["latent_var"])
    for c in chains:
        if c.widths[0] != head.H:
            raise ValueError(f"{owner}: vae.{c.name} takes {c.widths[0]} inputs, vae.latent_mu {head.H}")
    if head.H != enc_width:
        raise ValueError(f"{owner}: vae.latent_mu takes {head.H} inputs, the encoder ends at {enc_width} columns")
    for a, b in ((chains[0], chains[1]), (chains[2], chains[3])):
        if a.widths[-1] != b.widths[-1]:
            raise ValueError(f"{owner}: vae.{a.name} has {a.widths[-1]} outputs, vae.{b.name} {b.widths[-1]}")
    return head


def check_std(std, actor, device, owner):
    """The per-action standard deviation: a parameter tensor with one element per output of the chain `actor`."""
    check_tensor(std, "std", device, owner)
    if tuple(std.shape) != (actor.widths[-1],):
        raise ValueError(f"{owner}: std has shape {tuple(std.shape)}, the actor has {actor.widths[-1]} outputs")


def rows(t, width, what, n, device, owner):
    """(pointer, row stride) of an (n, width) float32 matrix with unit inner stride, as the kernels address it; n None: any row count."""
    ok = isinstance(t, torch.Tensor) and t.dtype == torch.float32 and t.dim() == 2 and t.shape[1] == width and (n is None or t.shape[0] == n) \
        and (t.shape[1] <= 1 or t.stride(1) == 1) and (t.shape[0] <= 1 or t.stride(0) >= width) and (device is None or t.device == device)
    if not ok:
        got = f"{tuple(t.shape)} {t.dtype} on {t.device}, strides {tuple(t.stride())}" if isinstance(t, torch.Tensor) else type(t).__name__
        raise ValueError(f"{owner}: {what} must be ({'B' if n is None else n}, {width}) float32 with unit inner stride"
                         + (f" on {device}" if device is not None else "") + f"; got {got}")
    return t.data_ptr(), (t.stride(0) if t.shape[0] > 1 else width)


class TcnSpec:
    """A "TCN" history encoder as the kernels take it (include/lgtraintcn.h): its Conv1d modules in order and the Linear / ELU tail
    behind the Flatten.  The history length H is no property of the module: `lengths(H)` gives [H, L_1, ..., L_n] or the refusal."""

    def __init__(self, name, convs, tail, owner):
        self.name, self.convs, self.tail, self.owner = name, convs, tail, owner

    @property
    def shapes(self):
        """(c_in, c_out, kernel, stride, padding, dilation) of every conv."""
        return [(m.in_channels, m.out_channels, m.kernel_size[0], m.stride[0], m.padding[0], m.dilation[0]) for m in self.convs]

    def lengths(self, n_history):
        out = conv_lengths(self.name, self.convs, n_history, self.owner)
        C, F = self.convs[-1].out_channels, self.convs[-1].out_channels * out[-1]
        if self.tail.widths[0] != F:
            raise ValueError(f"{self.owner}: {self.name}[{len(self.convs) + 1}].in_features = {self.tail.widths[0]}, but the flattened conv output has "
                             f"{C} * {out[-1]} = {F} columns for H = {int(n_history)}")
        return out

    def parameters(self):
        """In `seq.parameters()` order: every conv's weight and bias, then the tail's."""
        return [p for m in list(self.convs) + list(self.tail.linears) for p in (m.weight, m.bias)]


def conv_lengths(name, convs, n_history, owner):
    """[H, L_1, ..., L_n] of a stack of Conv1d modules on a history of H columns, or the refusal: H outside the kernel's widths, a window
    longer than its padded input, more columns behind the Flatten than the tail's first operand may have."""
    H = int(n_history)
    if not 1 <= H <= abi.POLICY_MAX_WIDTH:
        raise ValueError(f"{owner}: obs_history has {H} columns, the kernel takes 1 to {abi.POLICY_MAX_WIDTH}")
    out = [H]
    for i, m in enumerate(convs):
        k, s, p, d = m.kernel_size[0], m.stride[0], m.padding[0], m.dilation[0]
        span = out[-1] + 2 * p - d * (k - 1) - 1
        if span < 0:
            raise ValueError(f"{owner}: {name}[{i}] has a window of dilation * (kernel_size - 1) + 1 = {d * (k - 1) + 1} on a padded input "
                             f"of {out[-1] + 2 * p}: the output length is below 1")
        out.append(span // s + 1)
    C, F = convs[-1].out_channels, convs[-1].out_channels * out[-1]
    if F > abi.POLICY_MAX_WIDTH:
        raise ValueError(f"{owner}: {name}[{len(convs) - 1}] leaves out_channels * L = {C} * {out[-1]} = {F} columns behind the Flatten "
                         f"for H = {H}, the kernel takes {abi.POLICY_MAX_WIDTH}")
    return out


def describe_tcn(name, seq, device, owner, n_history=None):
    """The TcnSpec of `seq` = Conv1d+, Flatten, <a Linear / ELU chain by describe_chain's rules>, or the refusal that names `name[i]` and
    the attribute.  With `n_history` the lengths are checked too (TcnSpec.lengths)."""
    if not isinstance(seq, nn.Sequential):
        raise ValueError(f"{owner}: {name} is {type(seq).__name__}, expected an nn.Sequential of Conv1d, Flatten, Linear / ELU")
    mods, convs = list(seq), []
    lim = dict(kernel_size=abi.TRAIN_TCN_MAX_KERNEL, stride=abi.TRAIN_TCN_MAX_STRIDE, dilation=abi.TRAIN_TCN_MAX_DILATION)
    for i, m in enumerate(mods):
        where = f"{name}[{i}]"
        if isinstance(m, nn.Flatten):
            break
        if not isinstance(m, nn.Conv1d):
            what = "an activation between the convolutions is not built" if convs and not isinstance(m, nn.Linear) else "expected Conv1d layers, then a Flatten"
            raise ValueError(f"{owner}: {where} is {type(m).__name__}; {what}")
        if len(convs) == abi.TRAIN_TCN_MAX_CONV:
            raise ValueError(f"{owner}: {where} is Conv1d number {len(convs) + 1}, the kernel takes {abi.TRAIN_TCN_MAX_CONV}")
        if m.groups != 1:
            raise ValueError(f"{owner}: {where}.groups = {m.groups}, only groups = 1 is built")
        if m.padding_mode != "zeros":
            raise ValueError(f"{owner}: {where}.padding_mode = {m.padding_mode!r}, only 'zeros' is built")
        if isinstance(m.padding, str):
            raise ValueError(f"{owner}: {where}.padding = {m.padding!r}, only an integer padding is built")
        if m.bias is None:
            raise ValueError(f"{owner}: {where}.bias is None, the kernel adds a bias")
        want_in = convs[-1].out_channels if convs else 1
        if m.in_channels != want_in:
            raise ValueError(f"{owner}: {where}.in_channels = {m.in_channels}, " + (f"the conv before it gives {want_in}" if convs else "obs_history is one channel"))
        for attr, hi in (("in_channels", abi.TRAIN_TCN_MAX_CHANNELS), ("out_channels", abi.TRAIN_TCN_MAX_CHANNELS)):
            if not 1 <= getattr(m, attr) <= hi:
                raise ValueError(f"{owner}: {where}.{attr} = {getattr(m, attr)} is outside [1, {hi}]")
        for attr, hi in lim.items():
            if not 1 <= getattr(m, attr)[0] <= hi:
                raise ValueError(f"{owner}: {where}.{attr} = {getattr(m, attr)[0]} is outside [1, {hi}]")
        if not 0 <= m.padding[0] <= m.dilation[0] * (m.kernel_size[0] - 1):
            raise ValueError(f"{owner}: {where}.padding = {m.padding[0]} is outside [0, dilation * (kernel_size - 1) = {m.dilation[0] * (m.kernel_size[0] - 1)}]")
        check_tensor(m.weight, f"{where}.weight", device, owner)
        check_tensor(m.bias, f"{where}.bias", device, owner)
        convs.append(m)
    else:
        raise ValueError(f"{owner}: {name} has no Flatten behind its Conv1d layers")
    if not convs:
        raise ValueError(f"{owner}: {name}[0] is Flatten; expected Conv1d layers before it")
    if (m.start_dim, m.end_dim) != (1, -1):
        raise ValueError(f"{owner}: {name}[{i}] is Flatten({m.start_dim}, {m.end_dim}), only Flatten(1, -1) is built")
    if n_history is not None:
        conv_lengths(name, convs, n_history, owner)                   # before the tail: F above the limit is refused as F, with its factors
    tail = describe_chain(name, nn.Sequential(*mods[i + 1:]), device, False, owner, index0=i + 1)
    spec = TcnSpec(name, convs, tail, owner)
    if n_history is not None:
        spec.lengths(n_history)
    return spec
