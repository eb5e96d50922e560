"""The cases of the concurrent teacher-student learner passes (include/lgtraincts.h; the encoder pass is include/lgtraints.h's with a mask of
ones), shared by tests/test_train_cts_host.py (CPU) and tests/test_gpu_train_cts.py (GPU): one net table, one case table of (teacher,
student, critic) row counts, the input generator, a numpy restatement of both passes built on tests/train_support.py's layers and batch
sums (float64: the reference of every comparison; float32 with the plan's per-chain slices and the teacher's std slab before the
student's: the kernel's order of sums), the same passes as torch autograd on the CPU, the plan restated and the loader of the golden
fixture (tests/golden/gen_ppo_cts_train_fixtures.py).  The plan's rules, the parity rule and the fixture readers are
tests/train_support.py's; the encoder pass and the parameter names are tests/train_ts_cases.py's.  Nothing here loads the HIP library."""
import numpy as np
import torch

from tests import train_edges as te
from tests import train_support as sup
from tests import train_ts_cases as sc
from tests.train_support import CLASSES, chain_backward          # noqa: F401
from tests.train_ts_cases import enc_names, rl_names, split_rl   # noqa: F401

TARGET_JOBS = sc.TARGET_JOBS              # LG_TRAIN_TS_TARGET_JOBS: the slice rule's job target here too
CHAIN_NAMES = sc.CHAIN_NAMES              # LG_TRAIN_CTS_* order: privilege encoder, actor, critic, history encoder
OUTPUTS = ("mu_t", "sigma_t", "mu_s", "sigma_s", "values")
COTANGENTS = ("grad_mu_t", "grad_sigma_t", "grad_mu_s", "grad_sigma_s", "grad_values")

# name -> (privilege encoder widths, actor widths, critic widths, history encoder widths); actor[0] = O + Z, both encoders end at Z
_E = lambda n: {1: [5], 2: [7, 5], 3: [7, 6, 5], 4: [7, 6, 7, 5]}[n]
NETS = {
    "fixture": sc.NETS["fixture"],
    "go2_cts": ([99, 256, 128, 99], [144, 512, 256, 128, 12], [885, 1024, 256, 128, 1], [900, 256, 128, 99]),          # config.py's go2_cts sizes
    "ts_r16":  tuple(te.ROWS["ts_r16"][k] for k in ("priv", "actor", "critic", "hist")),          # 16-row tile, O = 24, Z = 37
    "ts_r8_z": tuple(te.ROWS["ts_r8_z"][k] for k in ("priv", "actor", "critic", "hist")),         # 8-row tile, O = 5, Z = 65
}
ENC_DEPTHS = ((1, 3), (1, 2), (2, 1), (4, 2))          # (privilege, history) layers: enc_first_buffer (0, 0), (0, 1), (1, 0), (1, 1)
for _p, _h in ENC_DEPTHS:
    NETS[f"enc_{_p}_{_h}"] = ([6] + _E(_p), [9, 11, 3], [6, 5, 1], [9] + _E(_h))


# ---- the plan -------------------------------------------------------------------------------------------------------------------------------
def restated_plan_cts(bt, bs, bc, priv, actor, critic, hist):
    """include/lgtraincts.h's plan; the per-chain lists hold the privilege encoder (bt rows), the actor (bt + bs) and the critic (bc)."""
    first = [0 if (len(c) - 1) & 1 else 1 for c in (priv, hist)]
    row_tile, lds_bytes = sup.row_tile(sup.lds_widths(((priv, first[0]), (actor, 0), (critic, 0), (hist, first[1]))))
    rows, chains = (bt, bt + bs, bc), (priv, actor, critic)
    off = (bt + bs) * actor[0]
    d = dict(h_off=[], g_off=[], p_off=[], slices=[], slice_rows=[])
    for n, c in zip(rows, chains):
        h, g = [], []
        for li in range(len(c) - 1):
            if li < len(c) - 2:
                h.append(off)
                off += n * c[li + 1]
            else:
                h.append(-1)
            g.append(off)
            off += n * c[li + 1]
        d["h_off"].append(h)
        d["g_off"].append(g)
    jobs = 0
    for n, c in zip(rows, chains):
        p, s, r = [], [], []
        for li in range(len(c) - 1):
            K, M = c[li], c[li + 1]
            tiles = -(-M // sup.WG_TILE) * -(-K // sup.WG_TILE)
            S, per = sup.slice_rule(n, tiles, TARGET_JOBS)
            p.append(off)
            off += S * (M * K + M)
            jobs += S * tiles
            s.append(S)
            r.append(per)
        d["p_off"].append(p)
        d["slices"].append(s)
        d["slice_rows"].append(r)
    std = [sup.slice_rule(n, 1, TARGET_JOBS) for n in (bt, bs)]
    n_std = std[0][0] + std[1][0]
    d.update(row_tile=row_tile, lds_bytes=lds_bytes, enc_first_buffer=first, cat_off=0, std=std, std_p_off=off, workspace_floats=off + n_std * actor[-1],
             weight_jobs=jobs + n_std, tiles=[-(-n // row_tile) for n in (bt, bs, bc)] if row_tile else [0, 0, 0])
    return d


def tile_of(net):
    return restated_plan_cts(1, 1, 1, *NETS[net])["row_tile"]


def _actor_only(net):
    return lambda b: dict(slices=[restated_plan_cts(b - 1, 1, 1, *NETS[net])["slices"][1]], slice_rows=[restated_plan_cts(b - 1, 1, 1, *NETS[net])["slice_rows"][1]])


def _priv_only(net):
    return lambda b: dict(slices=[restated_plan_cts(b, 1, 1, *NETS[net])["slices"][0]], slice_rows=[restated_plan_cts(b, 1, 1, *NETS[net])["slice_rows"][0]])


def straddling_rows(net):
    """(Bt, Bs) with the smallest Bt + Bs at which an actor layer gets more than one slice and a ragged last one (b of
    train_support.smallest_ragged_b needs b >= 2: the plan is asked at (b - 1, 1)), split so that Bt is no multiple of any actor layer's
    slice rows and lies inside the first slice: that slice holds rows of both groups."""
    b = sup.smallest_ragged_b(lambda n: _actor_only(net)(max(n, 2)))
    per = min(restated_plan_cts(b - 1, 1, 1, *NETS[net])["slice_rows"][1])
    bt = per - 3
    assert 0 < bt < b and all(bt % r for r in restated_plan_cts(bt, b - bt, 1, *NETS[net])["slice_rows"][1])
    return bt, b - bt


def ragged_teacher_rows(net):
    """The smallest Bt at which a privilege-encoder layer gets more than one slice and a ragged last one."""
    return sup.smallest_ragged_b(_priv_only(net))


# ---- the cases ------------------------------------------------------------------------------------------------------------------------------
R = tile_of("fixture")
CASES = {}


def _case(name, net, bt, bs, bc, **kw):
    CASES[name] = dict(net=net, Bt=bt, Bs=bs, Bc=bc, seed=1700 + len(CASES), **kw)


_case("fixture_1_1_1", "fixture", 1, 1, 1)
_case("fixture_below_tile", "fixture", R - 1, 1, R)
_case("fixture_above_tile", "fixture", R, R + 1, 2 * R + 1, clip=None)
_case("fixture_critic_below", "fixture", R + 1, R - 1, 1)                   # Bc below both groups
_case("fixture_critic_above", "fixture", 1, 2 * R + 1, 3 * R + 3)           # Bc above the sum
_case("fixture_odd_teacher", "fixture", 7, 9, 16)                           # an odd Bt: the student regions are off 16-byte alignment
_bt, _bs = straddling_rows("fixture")
_case("fixture_straddle", "fixture", _bt, _bs, _bt + _bs)                   # an actor slice across the group boundary, ragged last slice
_case("fixture_priv_ragged", "fixture", ragged_teacher_rows("fixture"), 3, 5, clip=None)
_case("ts_r16", "ts_r16", 17, 15, 33)
_case("ts_r8_z", "ts_r8_z", 9, 7, 17, clip=None)
for _p, _h in ENC_DEPTHS:
    _case(f"enc_{_p}_{_h}", f"enc_{_p}_{_h}", 33, 17, 40)
_case("go2_cts", "go2_cts", 24, 9, 33, clip=None)


# ---- inputs ---------------------------------------------------------------------------------------------------------------------------------
def make_inputs(case):
    """float32 numpy inputs of a case (a name of CASES, or a dict of Bt, Bs, Bc, seed and either `net` or `widths`): dict(priv, actor, critic,
    hist (widths), clip, rl_params (rl_names order), enc_params, teacher_obs, teacher_privileged_obs, student_obs, student_obs_history,
    student_privileged_obs, critic_obs, the five cotangents of COTANGENTS, upstream).  The clip as tests/train_support.place_clip places it
    over both groups' means; a case with clip=None has no Hardtanh."""
    c, (priv, actor, critic, hist) = sup.case_of(case, CASES, NETS)
    rng, f = np.random.default_rng(c["seed"]), np.float32
    bt, bs, bc = c["Bt"], c["Bs"], c["Bc"]
    O, A = actor[0] - priv[-1], actor[-1]
    std = (0.5 + rng.random(A)).astype(f)
    n = lambda *s: rng.normal(size=s).astype(f)
    x = dict(priv=priv, actor=actor, critic=critic, hist=hist, clip=None,
             rl_params=sup.draw_layers(rng, actor) + sup.draw_layers(rng, critic) + sup.draw_layers(rng, priv) + [std], enc_params=sup.draw_layers(rng, hist),
             teacher_obs=n(bt, O), teacher_privileged_obs=n(bt, priv[0]), student_obs=n(bs, O), student_obs_history=n(bs, hist[0]),
             student_privileged_obs=n(bs, priv[0]), critic_obs=n(bc, critic[0]),
             grad_mu_t=n(bt, A), grad_sigma_t=n(bt, A), grad_mu_s=n(bs, A), grad_sigma_s=n(bs, A), grad_values=n(bc, critic[-1]), upstream=f(0.75))
    if "clip" in c and c["clip"] is None:
        return x
    fw = rl_forward(x)
    x["clip"] = sup.place_clip(np.concatenate([fw["mu_t"], fw["mu_s"]]))
    return x


# ---- the restatement ------------------------------------------------------------------------------------------------------------------------
WRONG = ("student_latent_from_priv", "actor_teacher_rows_only", "student_rows_at_0", "priv_all_rows", "latent_cols0", "std_one_group", "critic_bt_rows")


def rl_forward(x, dtype=np.float64, wrong=None):
    """dict(mu_t, sigma_t, mu_s, sigma_s, values, acts=(privilege encoder over the teacher rows, actor over the teacher rows then the
    student rows, critic)) of include/lgtraincts.h's RL forward.  Planted defect: wrong="student_latent_from_priv" takes the student's
    latent from the privilege encoder on the student's privileged observations."""
    actor, critic, priv, std = split_rl(x, dtype)
    a = lambda k: np.asarray(x[k]).astype(dtype)
    pa = sup.mlp(priv, a("teacher_privileged_obs"), dtype)
    if wrong == "student_latent_from_priv":
        zs = sup.mlp(priv, a("student_privileged_obs"), dtype)[-1]
    else:
        zs = sup.mlp(sup.pairs(x["enc_params"], dtype), a("student_obs_history"), dtype)[-1]
    bt = pa[-1].shape[0]
    cat = np.concatenate([np.concatenate([a("teacher_obs"), pa[-1]], axis=1), np.concatenate([a("student_obs"), zs], axis=1)], axis=0)
    aa = sup.mlp(actor, cat, dtype)
    ca = sup.mlp(critic, a("critic_obs"), dtype)
    mu = sup.hardtanh(aa[-1], x["clip"], dtype)
    sigma = mu * 0 + std
    return dict(mu_t=mu[:bt], sigma_t=sigma[:bt], mu_s=mu[bt:], sigma_s=sigma[bt:], values=ca[-1], acts=(pa, aa, ca))


def _std_sum(gs_t, gs_s, per_t, per_s, one_group=False):
    """grad_std as the combine forms it: the teacher's slice partials in slice order, then the student's, one after the other."""
    parts = [gs_t[s:s + per_t].sum(0) for s in range(0, gs_t.shape[0], per_t)]
    if not one_group:
        parts += [gs_s[s:s + per_s].sum(0) for s in range(0, gs_s.shape[0], per_s)]
    out = parts[0]
    for p in parts[1:]:
        out = out + p
    return out


def rl_backward(x, dtype=np.float64, slices=None, wrong=None):
    """The gradients of the RL pass in rl_names order (actor, critic, privilege encoder, std).  The actor's sums run over the teacher rows
    then the student rows; the latent columns [O, O + Z) of actor layer 0's input gradient over the TEACHER rows are G of the privilege
    encoder's last layer; the student's latent is a constant.  `slices`: dict(std=(teacher rows, student rows), actor=[rows per layer],
    critic=[...], priv=[...]) as the plan slices each sum, or None.  Planted defects: the names of WRONG."""
    fw = rl_forward(x, dtype, wrong if wrong == "student_latent_from_priv" else None)
    actor, critic, priv, _ = split_rl(x, dtype)
    pa, aa, ca = fw["acts"]
    a = lambda k: np.asarray(x[k]).astype(dtype)
    bt, bs, s = fw["mu_t"].shape[0], fw["mu_s"].shape[0], slices or {}
    G = np.concatenate([sup.masked_grad_mu(x["grad_mu_t"], fw["mu_t"], x["clip"], dtype), sup.masked_grad_mu(x["grad_mu_s"], fw["mu_s"], x["clip"], dtype)])
    if wrong == "student_rows_at_0":          # the student tiles store at workspace row 0: over the teacher's rows, their own rows never written
        stored = []
        for h in aa:
            m = np.zeros_like(h)
            m[:bt] = h[:bt]
            m[:bs] = h[bt:]
            stored.append(m)
        aa = stored
    if wrong == "actor_teacher_rows_only":
        ga, dcat = chain_backward(actor, [h[:bt] for h in aa], G[:bt], dtype, s.get("actor"), input_grad=True)
    else:
        ga, dcat = chain_backward(actor, aa, G, dtype, s.get("actor"), input_grad=True)
    gc_rows = bt if wrong == "critic_bt_rows" else ca[0].shape[0]
    gc, _ = chain_backward(critic, [h[:gc_rows] for h in ca], a("grad_values")[:gc_rows], dtype, s.get("critic"))
    Z = pa[-1].shape[1]
    O = dcat.shape[1] - Z
    if wrong == "priv_all_rows":              # the student rows' latent gradient sent into the privilege encoder as well
        ps = sup.mlp(priv, a("student_privileged_obs"), dtype)
        pa, gz = [np.concatenate([t, u]) for t, u in zip(pa, ps)], dcat[:, O:]
    else:
        gz = dcat[:bt, :Z] if wrong == "latent_cols0" else dcat[:bt, O:]
    gp, _ = chain_backward(priv, pa, np.ascontiguousarray(gz), dtype, s.get("priv"))
    per_t, per_s = s.get("std", (bt, bs))
    return ga + gc + gp + [_std_sum(a("grad_sigma_t"), a("grad_sigma_s"), int(per_t), int(per_s), wrong == "std_one_group")]


def enc_inputs(x):
    """The encoder pass's inputs as tests/train_ts_cases.enc_pass reads them: the student's histories and privileged observations, a mask
    of ones."""
    return dict(x, obs_history=x["student_obs_history"], privileged_obs=x["student_privileged_obs"],
                terminated=np.ones((np.asarray(x["student_obs_history"]).shape[0], 1), np.asarray(x["student_obs_history"]).dtype))


def enc_pass(x, dtype=np.float64, **kw):
    """mse_loss(history_encoder(h), privilege_encoder(p).detach()): tests/train_ts_cases.enc_pass under a mask of ones ((p - y) * 1 is exact)."""
    return sc.enc_pass(enc_inputs(x), dtype, **kw)


def kernel_order_slices(x):
    """(rl_backward's `slices`, enc_pass's `slices`, the encoder pass's row tile) as the restated plans give them."""
    bt, bs, bc = (np.asarray(x[k]).shape[0] for k in ("teacher_obs", "student_obs", "critic_obs"))
    p, q = restated_plan_cts(bt, bs, bc, x["priv"], x["actor"], x["critic"], x["hist"]), sc.restated_plan_enc(bs, x["hist"], x["priv"])
    return dict(std=(p["std"][0][1], p["std"][1][1]), priv=p["slice_rows"][0], actor=p["slice_rows"][1], critic=p["slice_rows"][2]), \
        q["slice_rows"][0], q["row_tile"]


def torch_passes(x, dtype=torch.float32):
    """Both passes as torch computes them on the CPU in `dtype`: dict(the five outputs, rl_grads, enc_rl_grads (what the RL cotangents send
    into the history encoder: torch does accumulate it, nothing ever reads it), loss, enc_grads, priv_enc_grads (None each: the target is
    formed under no_grad)), float64 numpy."""
    t = lambda v: torch.as_tensor(np.asarray(v)).to(dtype)
    rl = [t(p).requires_grad_(True) for p in x["rl_params"]]
    enc = [t(p).requires_grad_(True) for p in x["enc_params"]]
    na, nc = 2 * (len(x["actor"]) - 1), 2 * (len(x["critic"]) - 1)
    priv = rl[na + nc:-1]

    def head(obs, z):
        mu = sup.mlp_t(torch.cat((t(obs), z), dim=-1), rl[:na])
        if x["clip"] is not None:
            mu = torch.nn.functional.hardtanh(mu, -x["clip"], x["clip"])
        return mu, mu * 0.0 + rl[-1]
    mu_t, sigma_t = head(x["teacher_obs"], sup.mlp_t(t(x["teacher_privileged_obs"]), priv))
    mu_s, sigma_s = head(x["student_obs"], sup.mlp_t(t(x["student_obs_history"]), enc))
    values = sup.mlp_t(t(x["critic_obs"]), rl[na:na + nc])
    n = lambda v: None if v is None else v.detach().double().numpy().copy()
    outs = (mu_t, sigma_t, mu_s, sigma_s, values)
    out = dict(zip(OUTPUTS, (n(v) for v in outs)))
    if "grad_mu_t" in x:
        torch.autograd.backward(list(outs), [t(x[k]) for k in COTANGENTS])
        out.update(rl_grads=[n(p.grad) for p in rl], enc_rl_grads=[n(p.grad) for p in enc])
        for p in rl + enc:
            p.grad = None
    with torch.no_grad():
        target = sup.mlp_t(t(x["student_privileged_obs"]), priv)
    loss = torch.nn.functional.mse_loss(sup.mlp_t(t(x["student_obs_history"]), enc), target)
    (loss * float(x.get("upstream", 1.0))).backward()
    out.update(loss=n(loss), enc_grads=[n(p.grad) for p in enc], priv_enc_grads=[n(p.grad) for p in priv])
    return out


def named(x, outs, rl_grads, loss, enc_grads):
    """dict name -> array of both passes' outputs and gradients."""
    d = {k: outs[k] for k in OUTPUTS}
    d["loss"] = np.asarray(loss, np.float64).reshape(1)
    d.update(zip(rl_names(x["actor"], x["critic"], x["priv"]), rl_grads))
    d.update(zip(enc_names(x["hist"]), enc_grads))
    return d


def references(x):
    """(float64 restatement, torch CPU float32) of a case, as `named` dicts."""
    e, t32 = enc_pass(x), torch_passes(x)
    return named(x, rl_forward(x), rl_backward(x), e["loss"], e["grads"]), named(x, t32, t32["rl_grads"], t32["loss"], t32["enc_grads"])


def check_parity(got, ref64, ref32, label, report=None, factor=sup.PARITY_FACTOR):
    """tests/train_support.check_parity on every tensor of ref64.  Its class of a tensor goes by the names mu / sigma / values, so the two
    groups' outputs are handed to it under those names, a group at a time; the rule and the factor are its own.  Returns and reports
    {class: worst ratio} over the three calls."""
    groups = (dict(mu="mu_t", sigma="sigma_t", values="values"), dict(mu="mu_s", sigma="sigma_s"))
    rest = [k for k in ref64 if k not in OUTPUTS]
    worst, bad = {}, []
    for sel, tag in [(g, t) for g, t in zip(groups, ("teacher", "student"))] + [({k: k for k in rest}, "")]:
        pick = lambda d: {k: d[v] for k, v in sel.items()}
        try:
            w = sup.check_parity(pick(got), pick(ref64), pick(ref32), f"{label} {tag}".strip(), None, factor)
        except AssertionError as e:
            bad.append(str(e))
            continue
        for k, v in w.items():
            worst[k] = max(worst.get(k, 0.0), v)
    if report is not None:
        report.append((label, worst))
    assert not bad, "\n".join(bad)
    return worst


# ---- the module -----------------------------------------------------------------------------------------------------------------------------
class Module(sc.Module):
    """ActorCriticCTS's members as FusedTrainPassCTS reads them (tests/train_ts_cases.Module: the same four chains and std, rl_parameters()
    in PPO_CTS.rl_params' order), with the two-group forward and the unmasked encoder loss."""

    def forward(self, teacher_obs, teacher_privileged_obs, student_obs, student_obs_history, critic_obs):
        mu_t = self.actor(torch.cat((teacher_obs, self.privilege_encoder(teacher_privileged_obs)), dim=-1))
        mu_s = self.actor(torch.cat((student_obs, self.history_encoder(student_obs_history)), dim=-1))
        return mu_t, mu_t * 0.0 + self.std, mu_s, mu_s * 0.0 + self.std, self.critic(critic_obs)

    def encoder_loss(self, student_obs_history, student_privileged_obs):
        with torch.no_grad():
            target = self.privilege_encoder(student_privileged_obs)
        return torch.nn.functional.mse_loss(self.history_encoder(student_obs_history), target)


# ---- the golden fixture ---------------------------------------------------------------------------------------------------------------------
TEACHER_COLUMNS = ("teacher_obs", "teacher_privileged_obs", "teacher_actions", "teacher_old_log_prob", "teacher_advantages", "teacher_old_mu",
                   "teacher_old_sigma")
STUDENT_COLUMNS = ("student_obs", "student_obs_history", "student_actions", "student_old_log_prob", "student_advantages")
FIXTURE_COLUMNS = TEACHER_COLUMNS + STUDENT_COLUMNS + ("critic_obs", "target_values", "returns")
ENC_COLUMNS = ("enc_history", "enc_privileged")
CFG_KEYS = sc.CFG_KEYS


def load_fixture(path):
    """tests/train_support.load_two_pass_fixture's dict with priv / actor / critic / hist widths: per RL step the columns, the five outputs,
    loss, both surrogates, kl, lr, grad_norm, grads, params; per encoder step enc_history, enc_privileged, enc_loss, enc_grads,
    enc_grad_norm, enc_params."""
    chains = dict(priv="privilege_encoder", actor="actor", critic="critic", hist="history_encoder")
    return sup.load_two_pass_fixture(path, CFG_KEYS, chains, "enc", FIXTURE_COLUMNS + ENC_COLUMNS + OUTPUTS + (
        "loss", "teacher_surrogate", "student_surrogate", "kl", "lr", "grad_norm", "enc_loss", "enc_grad_norm"))


def fixture_inputs(fx, params, rl_step=None, enc_step=None):
    """The inputs of one step of the fixture around `params` (name -> array), as make_inputs shapes them, float64.  No clip: the
    reference's ActorCriticCTS has no Hardtanh."""
    x = dict(priv=fx["priv"], actor=fx["actor"], critic=fx["critic"], hist=fx["hist"], clip=None, rl_params=[params[n] for n in fx["rl_names"]],
             enc_params=[params[n] for n in fx["enc_names"]], upstream=1.0)
    if rl_step is not None:
        x.update({k: fx[k][rl_step] for k in ("teacher_obs", "teacher_privileged_obs", "student_obs", "student_obs_history", "critic_obs")})
    if enc_step is not None:
        x.update(student_obs_history=fx["enc_history"][enc_step], student_privileged_obs=fx["enc_privileged"][enc_step])
    return x


def fixture_loss_inputs(fx, s, outs):
    """tests/ppo_loss_cases.restate's input for RL step s of the fixture around the given network outputs: the teacher's group (with the
    old distribution: the KL is the teacher's), the student's, one value group."""
    t = dict(mu=outs["mu_t"], sigma=outs["sigma_t"], actions=fx["teacher_actions"][s], advantages=fx["teacher_advantages"][s],
             old_log_prob=fx["teacher_old_log_prob"][s], old_mu=fx["teacher_old_mu"][s], old_sigma=fx["teacher_old_sigma"][s])
    u = dict(mu=outs["mu_s"], sigma=outs["sigma_s"], actions=fx["student_actions"][s], advantages=fx["student_advantages"][s],
             old_log_prob=fx["student_old_log_prob"][s])
    return dict(groups=[t, u], values=outs["values"], returns=fx["returns"][s], target_values=fx["target_values"][s])
