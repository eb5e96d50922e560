"""nets.py, the one reader of the modules behind FusedPolicy and the train passes, on the host: no library, no device.

One table of malformed chains, each row one refusal of `nets.describe_chain`, driven through every slot a chain can occupy on every
surface (`policy.describe` of each family, `train.describe`, `describe_ee`, `describe_ts`, `describe_dwaq`): the surface's own prefix
and the row's text, compared whole.  A second table does the same for the four heads of the DreamWaQ VAE on its two surfaces."""
import pytest
import torch
import torch.nn as nn

from hcr_genesis_lr_cl_amd import abi, nets, policy, train

W, D = abi.POLICY_MAX_WIDTH, abi.POLICY_MAX_LAYERS
ELU, Lin, Seq = nn.ELU, nn.Linear, nn.Sequential


def _with(lin, **params):
    for k, v in params.items():
        setattr(lin, k, nn.Parameter(v))
    return lin


# (id, the malformed chain, its refusal behind "OWNER: " with {n} the chain's name; `clip`: for a slot that may end in a Hardtanh, for
# one that may not, or (None) for both; `last_elu`: likewise for a slot that may end in an ELU).  The texts of a clip slot and of a
# plain one differ where the refusal lists what is built.
def _row(id, make, text, clip=None, last_elu=None):
    return dict(id=id, make=make, text=text, clip=clip, last_elu=last_elu)


CHAIN_ROWS = [
    _row("not_sequential", lambda: Lin(4, 2), "{n} is Linear, expected an nn.Sequential of Linear / ELU", clip=False),
    _row("not_sequential_clip", lambda: nn.GRU(4, 2), "{n} is GRU, expected an nn.Sequential of Linear / ELU / Hardtanh", clip=True),
    _row("no_bias", lambda: Seq(Lin(4, 3), ELU(), Lin(3, 2, bias=False)), "{n}[2] has no bias"),
    _row("too_wide_out", lambda: Seq(Lin(4, W + 1)), f"{{n}}[0] is 4 -> {W + 1}, widths are limited to {W}"),
    _row("too_wide_in", lambda: Seq(Lin(W + 1, 2)), f"{{n}}[0] is {W + 1} -> 2, widths are limited to {W}"),
    _row("width_mismatch", lambda: Seq(Lin(4, 3), ELU(), Lin(2, 2)), "{n}[2] takes 2 inputs, the layer before it gives 3"),
    _row("elu_first", lambda: Seq(ELU(), Lin(4, 2)), "{n}[0] (ELU) does not follow a Linear"),
    _row("elu_twice", lambda: Seq(Lin(4, 3), ELU(), ELU(), Lin(3, 2)), "{n}[2] (ELU) does not follow a Linear"),
    _row("elu_alpha", lambda: Seq(Lin(4, 3), ELU(alpha=0.5), Lin(3, 2)), "{n}[1] is ELU(alpha=0.5), only alpha = 1 is built"),
    _row("foreign", lambda: Seq(Lin(4, 3), nn.Tanh(), Lin(3, 2)), "{n}[1] is Tanh; only Linear and ELU are built into the kernel", clip=False),
    _row("foreign_clip", lambda: Seq(Lin(4, 3), nn.Tanh(), Lin(3, 2)),
         "{n}[1] is Tanh; only Linear and ELU (and a final Hardtanh) are built into the kernel", clip=True),
    _row("hardtanh_not_last", lambda: Seq(Lin(4, 3), nn.Hardtanh(-1.0, 1.0), Lin(3, 2)),
         "{n}[1] (Hardtanh(-1.0, 1.0)) must be the symmetric clip behind the actor's last Linear", clip=True),
    _row("hardtanh_behind_elu", lambda: Seq(Lin(4, 2), ELU(), nn.Hardtanh(-1.0, 1.0)),
         "{n}[2] (Hardtanh(-1.0, 1.0)) must be the symmetric clip behind the actor's last Linear", clip=True),
    _row("hardtanh_asymmetric", lambda: Seq(Lin(4, 2), nn.Hardtanh(-1.0, 2.0)),
         "{n}[1] (Hardtanh(-1.0, 2.0)) must be the symmetric clip behind the actor's last Linear", clip=True),
    _row("hardtanh_not_allowed", lambda: Seq(Lin(4, 2), nn.Hardtanh(-1.0, 1.0)), "{n}[1] is Hardtanh; only Linear and ELU are built into the kernel",
         clip=False),
    _row("no_linear", lambda: Seq(), "{n} has no Linear layer"),
    _row("too_deep", lambda: Seq(*[Lin(3, 3) for _ in range(D + 1)]), f"{{n}} has {D + 1} Linear layers, the kernel takes {D}"),
    _row("last_elu", lambda: Seq(Lin(4, 2), ELU()), "{n} ends in an ELU, expected a Linear output layer", last_elu=False),
    _row("float64_weight", lambda: Seq(Lin(4, 2).double()), "{n}[0].weight is torch.float64, the kernel reads float32"),
    _row("float16_bias", lambda: Seq(_with(Lin(4, 2), bias=torch.zeros(2, dtype=torch.float16))), "{n}[0].bias is torch.float16, the kernel reads float32"),
    _row("strided_weight", lambda: Seq(_with(Lin(4, 2), weight=torch.zeros(4, 2).t())), "{n}[0].weight is not contiguous"),
]


# ---- one valid tiny module per family ---------------------------------------------------------------------------------------------------------
class Box(nn.Module):
    is_recurrent = False

    def __init__(self, **members):
        super().__init__()
        for k, v in members.items():
            setattr(self, k, v)


def _mlp(i, o, h=4):
    return Seq(Lin(i, h), ELU(), Lin(h, o))


def _base(actor_in, **more):
    return Box(actor=Seq(*_mlp(actor_in, 2), nn.Hardtanh(-1.0, 1.0)), critic=_mlp(3, 1), std=nn.Parameter(torch.ones(2)), **more)


def _vae(H=4, L=2, E=3, clip=5.0):
    """vae.py's members in its order: the encoder (ends in an ELU), the four heads H -> L, L, E, E, the decoder."""
    return Box(encoder=Seq(Lin(6, 4), ELU(), Lin(4, H), ELU()), latent_mu=Lin(H, L), latent_var=Seq(Lin(H, L), nn.Hardtanh(-clip, clip)),
               vel_mu=Lin(H, E), vel_var=Seq(Lin(H, E), nn.Hardtanh(-clip, clip)), decoder=_mlp(L + E, 3))


def _memory(hidden):
    return Box(rnn=nn.LSTM(3, hidden))


FAMILIES = {
    "plain": lambda: _base(3),
    "ee": lambda: _base(5, estimator=_mlp(3, 2)),
    "ts": lambda: _base(5, privilege_encoder=_mlp(4, 2), history_encoder=Seq(Lin(6, 2))),
    "dwaq": lambda: _base(8, vae=_vae()),
    "recurrent": lambda: _with_flag(_base(4, memory_a=_memory(4), memory_c=_memory(3))),
}


def _with_flag(m):
    m.is_recurrent = True
    return m


# (surface, describe, the prefix of its refusals, family, the member's path, the chain's name in the refusal, may end in a Hardtanh, in an ELU)
_P, _T = "FusedPolicy", "FusedTrainPass"
SLOTS = [(s, fn, owner, fam, path, name or path, path == "actor", last_elu) for s, fn, owner, fam, members in (
    ("policy", policy.describe, _P, "plain", ("actor", "critic")),
    ("policy_ee", policy.describe, _P, "ee", ("estimator", "actor", "critic")),
    ("policy_ts", policy.describe, _P, "ts", ("privilege_encoder", "history_encoder", "actor", "critic")),
    ("policy_dwaq", policy.describe, _P, "dwaq", (("vae.encoder", None, True), "actor", "critic")),
    ("policy_recurrent", policy.describe, _P, "recurrent", ("actor", "critic")),
    ("train", train.describe, _T, "plain", ("actor", "critic")),
    ("train_ee", train.describe_ee, _T + "EE", "ee", ("estimator", "actor", "critic")),
    ("train_ts", train.describe_ts, _T + "TS", "ts", ("privilege_encoder", "history_encoder", "actor", "critic")),
    ("train_dwaq", train.describe_dwaq, _T + "DreamWaQ", "dwaq", (("vae.encoder", "encoder", True), ("vae.decoder", "decoder", False), "actor", "critic")),
) for path, name, last_elu in (m if isinstance(m, tuple) else (m, None, False) for m in members)]


def _put(module, path, value):
    *parents, leaf = path.split(".")
    for p in parents:
        module = getattr(module, p)
    setattr(module, leaf, value)


def _refusal(fn, module):
    with pytest.raises(ValueError) as e:
        fn(module)
    return str(e.value)


@pytest.mark.parametrize("family", FAMILIES)
def test_the_tiny_modules_are_valid(family):
    for s, fn, owner, fam, path, name, clip, last_elu in SLOTS:
        if fam == family:
            spec = fn(FAMILIES[family]())
            assert spec.actor.widths[-1] == 2 and spec.actor.clip == 1.0 and spec.critic.widths == [3, 4, 1]


# every row in every slot it can occupy: a row about one kind of slot (with or without a clip, a last ELU) skips the other kind
CHAIN_CASES = [pytest.param(row, slot, id=f"{slot[0]}.{slot[4]}-{row['id']}") for slot in SLOTS for row in CHAIN_ROWS
               if row["clip"] in (None, slot[6]) and row["last_elu"] in (None, slot[7])]


@pytest.mark.parametrize("row, slot", CHAIN_CASES)
def test_a_malformed_chain_is_refused_in_every_slot(row, slot):
    s, fn, owner, family, path, name, clip, last_elu = slot
    m = FAMILIES[family]()
    _put(m, path, row["make"]())
    assert _refusal(fn, m) == f"{owner}: " + row["text"].format(n=name)


def test_describe_chain_itself():
    for row in CHAIN_ROWS:
        clip, last_elu = bool(row["clip"]), bool(row["last_elu"])
        with pytest.raises(ValueError) as e:
            nets.describe_chain("net", row["make"](), None, clip, "Owner", allow_last_elu=last_elu)
        assert str(e.value) == "Owner: " + row["text"].format(n="net"), row["id"]
    c = nets.describe_chain("net", Seq(Lin(4, 3), ELU(), Lin(3, 2), nn.Hardtanh(-0.5, 0.5)), None, True, "Owner")
    assert (c.name, c.widths, c.elu, c.clip, len(c.linears)) == ("net", [4, 3, 2], [True, False], 0.5, 2)
    assert policy.ChainSpec is nets.ChainSpec and train.TrainChainSpec is nets.ChainSpec


def test_a_last_elu_is_taken_where_the_slot_allows_it():
    last = Seq(Lin(4, 2), ELU())
    assert nets.describe_chain("net", last, None, False, "Owner", allow_last_elu=True).elu == [True]
    for fn, name in ((policy.describe, "vae_encoder"), (train.describe_dwaq, "encoder")):
        assert getattr(fn(FAMILIES["dwaq"]()), name).elu == [True, True]
    m = FAMILIES["dwaq"]()
    m.vae.encoder = m.vae.encoder[:3]                    # and one that ends in its Linear is taken as well
    assert policy.describe(m).vae_encoder.elu == train.describe_dwaq(m).encoder.elu == [True, False]


# ---- the four heads ---------------------------------------------------------------------------------------------------------------------------
def _clipped(i, o, lo=-5.0, hi=5.0):
    return Seq(Lin(i, o), nn.Hardtanh(lo, hi))


HEAD_ROWS = [      # (id, what replaces which member of the valid VAE (H = 4, L = 2, E = 3, clip 5), the refusal behind "OWNER: ")
    ("var_not_sequential", dict(latent_var=lambda: Lin(4, 2)), "vae.latent_var is not Sequential(Linear, Hardtanh): the log-variance head of the VAE"),
    ("var_three_modules", dict(vel_var=lambda: Seq(Lin(4, 3), ELU(), nn.Hardtanh(-5.0, 5.0))),
     "vae.vel_var is not Sequential(Linear, Hardtanh): the log-variance head of the VAE"),
    ("var_missing", dict(vel_var=lambda: None), "vae.vel_var is not Sequential(Linear, Hardtanh): the log-variance head of the VAE"),
    ("clip_asymmetric", dict(vel_var=lambda: _clipped(4, 3, -5.0, 4.0)), "vae.vel_var[1] (Hardtanh(-5.0, 4.0)) must be a symmetric clip"),
    ("clips_differ", dict(vel_var=lambda: _clipped(4, 3, -4.0, 4.0)), "vae.latent_var clips to 5.0, vae.vel_var to 4.0; the kernel takes one clip"),
    ("mu_not_linear", dict(vel_mu=lambda: Seq(Lin(4, 3))), "vae.vel_mu is Sequential, expected a Linear"),
    ("mu_missing", dict(latent_mu=lambda: None), "vae.latent_mu is NoneType, expected a Linear"),
    ("mu_no_bias", dict(vel_mu=lambda: Lin(4, 3, bias=False)), "vae.vel_mu has no bias"),
    ("var_no_bias", dict(latent_var=lambda: Seq(Lin(4, 2, bias=False), nn.Hardtanh(-5.0, 5.0))), "vae.latent_var[0] has no bias"),
    ("too_wide_out", dict(latent_mu=lambda: Lin(4, W + 1), latent_var=lambda: _clipped(4, W + 1)), f"vae.latent_mu is 4 -> {W + 1}, widths are limited to {W}"),
    ("too_wide_in", dict(vel_var=lambda: _clipped(W + 1, 3)), f"vae.vel_var[0] is {W + 1} -> 3, widths are limited to {W}"),
    ("heads_disagree", dict(vel_mu=lambda: Lin(5, 3)), "vae.vel_mu takes 5 inputs, vae.latent_mu 4"),
    ("encoder_disagrees", dict(encoder=lambda: Seq(Lin(6, 5), ELU())), "vae.latent_mu takes 4 inputs, the encoder ends at 5 columns"),
    ("latent_widths", dict(latent_var=lambda: _clipped(4, 3)), "vae.latent_mu has 2 outputs, vae.latent_var 3"),
    ("vel_widths", dict(vel_mu=lambda: Lin(4, 2)), "vae.vel_mu has 2 outputs, vae.vel_var 3"),
    ("float64_weight", dict(vel_var=lambda: _clipped(4, 3).double()), "vae.vel_var[0].weight is torch.float64, the kernel reads float32"),
    ("strided_weight", dict(latent_mu=lambda: _with(Lin(4, 2), weight=torch.zeros(4, 2).t())), "vae.latent_mu.weight is not contiguous"),
]


@pytest.mark.parametrize("fn, owner", [(policy.describe, _P), (train.describe_dwaq, _T + "DreamWaQ")], ids=["policy", "train"])
@pytest.mark.parametrize("id, members, text", HEAD_ROWS, ids=[r[0] for r in HEAD_ROWS])
def test_a_malformed_head_is_refused_on_both_surfaces(id, members, text, fn, owner):
    m = FAMILIES["dwaq"]()
    for k, make in members.items():
        setattr(m.vae, k, make())
    assert _refusal(fn, m) == f"{owner}: {text}"


def test_one_head_spec_serves_both_surfaces():
    m = FAMILIES["dwaq"]()
    h = nets.describe_heads(m.vae, 4, None, "Owner")
    assert (h.H, h.L, h.E, h.clip) == (4, 2, 3, 5.0) and tuple(c.name for c in h.chains) == nets.HEADS
    assert all(a is b for a, b in zip(h.linears, (m.vae.latent_mu, m.vae.latent_var[0], m.vae.vel_mu, m.vae.vel_var[0])))
    assert [c.widths for c in h.chains] == [[4, 2], [4, 2], [4, 3], [4, 3]] and all(c.elu == [False] and c.clip is None for c in h.chains)
    p, t = policy.describe(m), train.describe_dwaq(m)
    assert (p.head.H, p.head.L, p.head.E, p.head.clip, p.latent_width) == (4, 2, 3, 5.0, 5)
    assert [c.linears[0] for c in t.heads] == list(p.head.linears) and t.var_clip == 5.0 and (t.num_latent, t.num_explicit) == (2, 3)


# ---- tensors, std and rows --------------------------------------------------------------------------------------------------------------------
def test_tensor_std_and_rows_refusals():
    dev = torch.device("cuda:0")                         # only compared with: nothing is put there
    for t, text in ((torch.zeros(2, dtype=torch.float64), "w is torch.float64, the kernel reads float32"), (3.0, "w is float, the kernel reads float32"),
                    (torch.zeros(2, 4)[:, ::2], "w is not contiguous"), (torch.zeros(2), "w is on cpu, not on cuda:0")):
        with pytest.raises(ValueError) as e:
            nets.check_tensor(t, "w", dev, "Owner")
        assert str(e.value) == "Owner: " + text
    nets.check_tensor(torch.zeros(2), "w", None, "Owner")
    actor = nets.describe_chain("actor", _mlp(3, 2), None, True, "Owner")
    nets.check_std(torch.ones(2), actor, None, "Owner")
    for std, text in ((torch.ones(3), "std has shape (3,), the actor has 2 outputs"), (torch.ones(1, 2), "std has shape (1, 2), the actor has 2 outputs"),
                      (torch.ones(2, dtype=torch.float16), "std is torch.float16, the kernel reads float32")):
        with pytest.raises(ValueError) as e:
            nets.check_std(std, actor, None, "Owner")
        assert str(e.value) == "Owner: " + text
    wide = torch.zeros(4, 8)
    assert nets.rows(wide[:, 2:5], 3, "x", 4, None, "Owner") == (wide.data_ptr() + 8, 8)          # addressed in place
    assert nets.rows(wide[:1, :3], 3, "x", None, None, "Owner") == (wide.data_ptr(), 3)           # one row: its width is its stride
    assert nets.rows(wide[:, 7:], 1, "x", 4, None, "Owner") == (wide.data_ptr() + 28, 8)
    for t, n, d, text in ((torch.zeros(4, 2), 4, None, "x must be (4, 3) float32 with unit inner stride; got (4, 2) torch.float32 on cpu, strides (2, 1)"),
                          (torch.zeros(5, 3), 4, None, "x must be (4, 3) float32 with unit inner stride; got (5, 3) torch.float32 on cpu, strides (3, 1)"),
                          (torch.zeros(3, 4).t(), None, None, "x must be (B, 3) float32 with unit inner stride; got (4, 3) torch.float32 on cpu, strides (1, 4)"),
                          (torch.zeros(1, 3).expand(4, 3), 4, None, "x must be (4, 3) float32 with unit inner stride; got (4, 3) torch.float32 on cpu, strides (0, 1)"),
                          (torch.zeros(4, 3, dtype=torch.float64), 4, None,
                           "x must be (4, 3) float32 with unit inner stride; got (4, 3) torch.float64 on cpu, strides (3, 1)"),
                          (torch.zeros(4, 3), 4, dev, "x must be (4, 3) float32 with unit inner stride on cuda:0; got (4, 3) torch.float32 on cpu, strides (3, 1)"),
                          (None, 4, None, "x must be (4, 3) float32 with unit inner stride; got NoneType")):
        with pytest.raises(ValueError) as e:
            nets.rows(t, 3, "x", n, d, "Owner")
        assert str(e.value) == "Owner: " + text
