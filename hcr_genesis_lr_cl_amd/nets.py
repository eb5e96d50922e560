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


def describe_chain(name, seq, device, allow_clip, owner, allow_last_elu=False):
    """The ChainSpec of `seq`, or the refusal that names its layer.  `allow_clip`: a symmetric Hardtanh may end it (the actor);
    `allow_last_elu`: an ELU may (the DreamWaQ encoder)."""
    if not isinstance(seq, nn.Sequential):
        raise ValueError(f"{owner}: {name} is {type(seq).__name__}, expected an nn.Sequential of Linear / ELU"
                         + (" / Hardtanh" if allow_clip else ""))
    linears, elu, clip = [], [], None
    mods = list(seq)
    for i, m in enumerate(mods):
        where = f"{name}[{i}]"
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
