"""Developer tool (GPU only, never read by bench.py): time of the policy half of one rollout step at N = 4096 envs for eight net sets -- go2
(actor 45-512-256-128-12, critic 45-512-256-128-1), go2_ee (estimator 900-256-128-24, actor 924-..-12, critic 870-1024-256-128-1),
tron1_pf_ee (310 / 327 / 1340, 17 labels, 6 actions) (dims: bench.py::ppo_rollout), and the go2 sizes of config.py for the other learner
families: go2_ts (privilege encoder 99-256-128-99, actor 144-512-256-128-12, critic 885-1024-256-128-1; the teacher's step, as PPO_TS.act),
go2_cts (the same plus the history encoder 900-256-128-99 on the 1024 student rows behind 3072 teachers; the torch side is the
reference's two passes and four cats, ppo_cts.py:115-127) and go2_dreamwaq (VAE encoder 900-256-128-80 with the trailing ELU, heads
16 / 16 / 24 / 24, actor 85-..-12, critic 885-..-1), and two recurrent sets (ActorCriticRecurrent, obs 45 for both memories): go2_lstm256
(LSTM 256 x 1, actor and critic 256-256-256-256-out) and go2_lstm512 (LSTM 512 x 1, actor and critic 512-512-256-128-out) -- produced three
ways into the same storage row:

  (i)   the fused launch, `FusedPolicy.act(obs, critic_obs, storage=st)` (Philox draw, so with its one-lane counter launch);
  (ii)  the torch ops of bench.py::policy_row (f32 GEMMs, ELUs, randn, log-prob arithmetic, five copy_) captured once and replayed as one
        HIP graph;
  (iii) the same ops dispatched eagerly;
  (iv)  go2 only: the loop act -> env.step -> add_step for 24 steps on zero-copy observation rows, with (i) and with (ii), in env-steps/s.

Recurrent sets: (i) is `act(obs, critic_obs, storage=st, reset=mask)` (about 2 % of the rows done): cells, MLPs, draw, reset and the
pre-step hidden-state rows in the one launch; (ii) / (iii) are the module's ops for the same rows: the masked reset of the four state
tensors, their copies into the storage's saved hidden states (two per memory), nn.LSTM of both memories, the MLPs, sampling and the five
copies; the states are kept at fixed addresses (the new ones copied back), which the graph needs.  Measured on one MI355X at 4096 envs
(DESIGN.md section 10b): go2_lstm256 fused 266 us against 410 us for the graph replay (667 us eager) -- the fused launch wins; go2_lstm512
fused 1133 us against 622 us (678 us eager) -- it loses by 1.8 x, because only the 8-row tile fits the LDS and 512 tiles per chain each
re-read 6.3 MB of weights from L2.  A rollout that only wants speed keeps H = 512 (and any size whose row tile is 8) on the torch ops.

(i)-(iii): each sample is the device-event time around a burst of launches divided by the burst length, so it is the time per step on the
device queue with launches back to back; the sides alternate in one process after a warm-up, median and p10-p90 over the repeats are
printed.  (iv): host clock around whole 24-step loops ending in a synchronise.  Before anything is timed the fused launch's mu and values are
compared with the torch ops' on the same inputs.  FLOP are counted from the shapes: 2 * in * out per layer and env.

    python tools/policy_act_time.py [--repeats 30] [--burst 50] [--envs 4096] [--sets go2,go2_ee] [--sides fused] [--no-loop]

Prints a table and one JSON line."""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import torch  # noqa: E402
import torch.nn as nn  # noqa: E402

F32_MFMA_FLOPS = 157e12          # exact-f32 MFMA rate, MI355X_MICROARCH.md
SETS = {"go2": dict(obs=45, est=None, actor=[512, 256, 128], A=12, cobs=45, critic=[512, 256, 128]),
        "go2_ee": dict(obs=900, est=([256, 128], 24), actor=[512, 256, 128], A=12, cobs=870, critic=[1024, 256, 128]),
        "tron1_pf_ee": dict(obs=310, est=([256, 128], 17), actor=[512, 256, 128], A=6, cobs=1340, critic=[1024, 256, 128])}
_GO2_FAMILY = dict(obs=45, est=None, actor=[512, 256, 128], A=12, cobs=885, critic=[1024, 256, 128], hist=900)
SETS["go2_ts"] = dict(_GO2_FAMILY, family="ts", priv=99, latent=99, enc=[256, 128])
SETS["go2_cts"] = dict(SETS["go2_ts"], teachers=3072)                 # of 4096: scaled with --envs
SETS["go2_dreamwaq"] = dict(_GO2_FAMILY, family="dreamwaq", enc=[256, 128], H=80, L=16, E=24)
SETS["go2_lstm256"] = dict(obs=45, est=None, actor=[256, 256, 256], A=12, cobs=45, critic=[256, 256, 256], family="recurrent", rnn=nn.LSTM, H=256, layers=1)
SETS["go2_lstm512"] = dict(obs=45, est=None, actor=[512, 256, 128], A=12, cobs=45, critic=[512, 256, 128], family="recurrent", rnn=nn.LSTM, H=512, layers=1)


def mlp(i, hidden, o, tail=None):
    layers, d = [], i
    for h in hidden:
        layers += [nn.Linear(d, h), nn.ELU()]
        d = h
    layers.append(nn.Linear(d, o))
    if tail is not None:
        layers.append(tail)
    return nn.Sequential(*layers)


class Nets(nn.Module):
    is_recurrent = False

    def __init__(self, d):
        super().__init__()
        E = d["est"][1] if d["est"] else 0
        if d["est"]:
            self.estimator = mlp(d["obs"], d["est"][0], E)
        if d.get("family") == "ts":
            E = d["latent"]
            self.privilege_encoder, self.history_encoder = mlp(d["priv"], d["enc"], E), mlp(d["hist"], d["enc"], E)
        if d.get("family") == "dreamwaq":
            E = d["L"] + d["E"]
            self.vae = nn.Module()
            self.vae.encoder = nn.Sequential(*mlp(d["hist"], d["enc"], d["H"]), nn.ELU())
            self.vae.latent_mu, self.vae.vel_mu = nn.Linear(d["H"], d["L"]), nn.Linear(d["H"], d["E"])
            self.vae.latent_var = nn.Sequential(nn.Linear(d["H"], d["L"]), nn.Hardtanh(-5.0, 5.0))
            self.vae.vel_var = nn.Sequential(nn.Linear(d["H"], d["E"]), nn.Hardtanh(-5.0, 5.0))
        if d.get("family") == "recurrent":           # actor_critic_recurrent.py: the MLPs read the memories' top h
            self.is_recurrent = True
            self.memory_a, self.memory_c = nn.Module(), nn.Module()
            self.memory_a.rnn, self.memory_c.rnn = d["rnn"](d["obs"], d["H"], d["layers"]), d["rnn"](d["cobs"], d["H"], d["layers"])
            self.actor, self.critic = mlp(d["H"], d["actor"], d["A"], nn.Hardtanh(-100.0, 100.0)), mlp(d["H"], d["critic"], 1)
            self.std = nn.Parameter(torch.ones(d["A"]))
            return
        self.actor = mlp(d["obs"] + E, d["actor"], d["A"], nn.Hardtanh(-100.0, 100.0))
        self.critic = mlp(d["cobs"], d["critic"], 1)
        self.std = nn.Parameter(torch.ones(d["A"]))


def _linears(*mods):
    return [l for m in mods for l in m.modules() if isinstance(l, nn.Linear)]


def work(m, d, N, k):
    """(FLOP per step, bytes of the weights one step reads): 2 * in * out per layer and env, each chain on the rows it serves."""
    fl = lambda *mods: sum(2 * l.in_features * l.out_features for l in _linears(*mods))
    by = lambda *mods: sum(4 * (l.in_features + 1) * l.out_features for l in _linears(*mods))
    fam = d.get("family")
    if fam == "recurrent":
        rnn = [p for mem in (m.memory_a, m.memory_c) for n, p in mem.rnn.named_parameters() if n.startswith("weight")]
        return N * (fl(m.actor, m.critic) + sum(2 * p.numel() for p in rnn)), by(m.actor, m.critic) + sum(4 * (p.shape[1] + 1) * p.shape[0] for p in rnn)
    if fam == "ts":
        lead = [m.privilege_encoder] + ([m.history_encoder] if k is not None else [])
        flop = N * fl(m.actor, m.critic) + (N if k is None else k) * fl(m.privilege_encoder) + (0 if k is None else (N - k) * fl(m.history_encoder))
        return flop, by(m.actor, m.critic, *lead)
    lead = [m.vae.encoder, m.vae.latent_mu, m.vae.latent_var, m.vae.vel_mu, m.vae.vel_var] if fam == "dreamwaq" else \
        [m.estimator] if hasattr(m, "estimator") else []
    return N * fl(m.actor, m.critic, *lead), by(m.actor, m.critic, *lead)


def _sample(m, mu, z=None):
    std = m.std.expand_as(mu)
    act = mu + std * (torch.randn_like(mu) if z is None else z)
    return act, (-0.5 * ((act - mu) / std) ** 2 - m.std.log() - 0.9189385332046727).sum(-1), mu, std


def _store(st, t, act, lp, mu, std, values):
    st.mu[t].copy_(mu)
    st.sigma[t].copy_(std)
    st.actions[t].copy_(act)
    st.actions_log_prob[t, :, 0].copy_(lp)
    st.values[t].copy_(values)


def torch_row(m, x, st, t, lab_row, k=None, z=None, eps=None):
    """bench.py::policy_row on the rows it is given (x: obs, cobs and the family's priv / hist); `z` / `eps` replace the two randn draws."""
    obs = x["obs"]
    if hasattr(m, "vae"):                        # vae.py:65-92, actor_critic_dreamwaq.py:145-156
        h = m.vae.encoder(x["hist"])
        lm, lv, vm, vv = m.vae.latent_mu(h), m.vae.latent_var(h), m.vae.vel_mu(h), m.vae.vel_var(h)
        sl, sv = torch.exp(0.5 * lv), torch.exp(0.5 * vv)
        L = lm.shape[1]
        lat = (torch.randn_like(sl) if eps is None else eps[:, :L]) * sl + lm
        vel = (torch.randn_like(sv) if eps is None else eps[:, L:]) * sv + vm
        out = _sample(m, m.actor(torch.cat((obs, torch.cat((lat, vel), dim=-1)), dim=-1)), z)
    elif hasattr(m, "privilege_encoder") and k is not None:     # ppo_cts.py:115-127: two passes, four cats
        te = _sample(m, m.actor(torch.cat((obs[:k], m.privilege_encoder(x["priv"][:k])), dim=-1)), None if z is None else z[:k])
        su = _sample(m, m.actor(torch.cat((obs[k:], m.history_encoder(x["hist"][k:])), dim=-1)), None if z is None else z[k:])
        out = [torch.cat((a, b), dim=0) for a, b in zip(te[:3], su[:3])] + [torch.cat((te[3], su[3]), dim=0)]
    elif hasattr(m, "privilege_encoder"):        # ppo_ts.py:81-87
        out = _sample(m, m.actor(torch.cat((obs, m.privilege_encoder(x["priv"])), dim=-1)), z)
    elif hasattr(m, "estimator"):
        lab = m.estimator(obs)
        lab_row.copy_(lab)
        out = _sample(m, m.actor(torch.cat((obs, lab), dim=-1)), z)
    else:
        out = _sample(m, m.actor(obs), z)
    _store(st, t, *out, m.critic(x["cobs"]))


def recurrent_row(m, x, st, t, state, mask, z=None):
    """What PPO.act / process_env_step ask of an ActorCriticRecurrent for one step, on states kept at fixed addresses: reset(dones) of the
    step before as a masked fill, the pre-step states into the storage (ppo.py:94-95, rollout_storage.py:104-119), both memories, the
    MLPs, the draw and the five copies."""
    keep = mask.view(1, -1, 1)
    for s in state["a"] + state["c"]:
        s.masked_fill_(keep, 0.0)
    for saved, s in zip(st.saved_hidden_states_a + st.saved_hidden_states_c, state["a"] + state["c"]):
        saved[t].copy_(s)
    top = {}
    for w, mem, inp in (("a", m.memory_a, x["obs"]), ("c", m.memory_c, x["cobs"])):
        out, new = mem.rnn(inp.unsqueeze(0), tuple(state[w]))
        top[w] = out.squeeze(0)
        for s, n in zip(state[w], new):
            s.copy_(n)
    _store(st, t, *_sample(m, m.actor(top["a"]), z), m.critic(top["c"]))


def make_storage(d, N, k, dev):
    from hcr_genesis_lr_cl_amd import rollout as r
    sh = lambda key: [d[key]]
    if d.get("family") == "ts":
        args = (sh("obs"), sh("priv"), sh("hist"), sh("cobs"), sh("A"), dev)
        return r.RolloutStorageTS(N, 2, *args) if k is None else r.RolloutStorageCTS(N, k, 2, *args)
    if d.get("family") == "dreamwaq":
        return r.RolloutStorageDreamWaQ(N, 2, sh("obs"), sh("cobs"), sh("hist"), sh("E"), sh("obs"), sh("A"), dev)
    return r.RolloutStorage(N, 2, sh("obs"), sh("cobs"), sh("A"), dev)


def capture(fn):
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        for _ in range(3):
            fn()
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        fn()
    return g


def stat(v):
    s = sorted(v)
    return dict(median=statistics.median(v), min=s[0], max=s[-1], p10=s[len(s) // 10], p90=s[(9 * len(s)) // 10])


def burst_us(fn, burst):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(burst):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / burst


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--repeats", type=int, default=30)
    ap.add_argument("--burst", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--loops", type=int, default=20, help="24-step loops per sample of (iv)")
    ap.add_argument("--sets", default=",".join(SETS), help="comma-separated net sets")
    ap.add_argument("--sides", default="fused,torch_graph,torch_eager", help="comma-separated sides to time")
    ap.add_argument("--no-loop", action="store_true", help="skip (iv)")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("policy_act_time.py: no GPU -- a time is only measured on the device")
    from hcr_genesis_lr_cl_amd import build as b
    from hcr_genesis_lr_cl_amd.policy import FusedPolicy
    from hcr_genesis_lr_cl_amd.rollout import RolloutStorage
    N, dev, T = args.envs, "cuda:0", 24
    res = dict(tool="policy_act_time", envs=N, repeats=args.repeats, burst=args.burst, f32_mfma_flops=F32_MFMA_FLOPS, source_hash=b.source_hash(),
               device=torch.cuda.get_device_name(0), sets={})
    torch.manual_seed(1)
    with torch.inference_mode():
        for name in args.sets.split(","):
            d = SETS[name]
            k = d["teachers"] * N // 4096 if "teachers" in d else None
            m = Nets(d).to(dev)
            fp = FusedPolicy(m, seed=1)
            st = make_storage(d, N, k, dev)
            x = {key: torch.randn(N, d[w], device=dev) for key, w in (("obs", "obs"), ("cobs", "cobs"), ("priv", "priv"), ("hist", "hist")) if w in d}
            lab_row = torch.zeros(N, d["est"][1], device=dev) if d["est"] else None
            fam = d.get("family")
            if fam == "recurrent":
                res["sets"][name] = time_recurrent(name, d, m, fp, st, x, N, args)
                del fp, st
                continue
            if fam == "ts":
                kw = dict(privileged_obs=x["priv"])
            elif fam == "dreamwaq":
                kw = dict(obs_history=x["hist"])
            else:
                kw = dict(labels=lab_row)
            if k is not None:
                kw.update(obs_history=x["hist"], num_teacher=k)
            z = torch.randn(N, d["A"], device=dev)                    # the agreement check: both sides on the same two draws
            eps = torch.randn(N, d["L"] + d["E"], device=dev) if fam == "dreamwaq" else None
            st.step = 0
            fp.act(x["obs"], x["cobs"], storage=st, noise=z, **kw, **(dict(latent_noise=eps) if eps is not None else {}))
            torch_row(m, x, st, 1, lab_row, k, z, eps)
            torch.cuda.synchronize()
            agree = {q: float((getattr(st, q)[0] - getattr(st, q)[1]).abs().max()) for q in ("mu", "values", "sigma")}
            if agree["mu"] > 1e-4 or agree["values"] > 1e-4 or agree["sigma"] != 0.0:
                sys.exit(f"policy_act_time.py: {name}: the fused launch and the torch ops disagree ({agree}) -- nothing timed")
            want = args.sides.split(",")
            graph = capture(lambda: torch_row(m, x, st, 1, lab_row, k)) if "torch_graph" in want else None
            sides = {"fused": lambda: fp.act(x["obs"], x["cobs"], storage=st, **kw), "torch_graph": graph and graph.replay,
                     "torch_eager": lambda: torch_row(m, x, st, 1, lab_row, k)}
            sides = {q: f for q, f in sides.items() if q in want}
            for _ in range(args.warmup):
                for f in sides.values():
                    burst_us(f, args.burst)
            times = {q: [] for q in sides}
            for _ in range(args.repeats):
                for q, f in sides.items():
                    times[q].append(burst_us(f, args.burst))
            flop, wbytes = work(m, d, N, k)
            out = dict(flop_per_step=flop, weight_bytes=wbytes, row_tile=fp.row_tile(N, **({"num_teacher": k} if k is not None else {})), step_us={k: stat(v) for k, v in times.items()},
                       max_abs_diff_vs_torch=agree)
            if "fused" in times:
                out["fused_flops"] = flop / (out["step_us"]["fused"]["median"] * 1e-6)
                out["fraction_of_f32_mfma_rate"] = out["fused_flops"] / F32_MFMA_FLOPS
            res["sets"][name] = out
            print(f"{name}: {flop / 1e9:.2f} GFLOP per step, {out['weight_bytes'] / 1e6:.2f} MB of weights, row tile {out['row_tile']}, "
                  f"|mu - torch| {agree['mu']:.1e}, |values - torch| {agree['values']:.1e}")
            for k, v in out["step_us"].items():
                print(f"  {k:12s}: median {v['median']:8.1f} us   min {v['min']:8.1f}   p10-p90 {v['p10']:8.1f} - {v['p90']:8.1f}   max {v['max']:8.1f}")
            if "fused" in times:
                print(f"  fused: {out['fused_flops'] / 1e12:.1f} TFLOP/s = {100 * out['fraction_of_f32_mfma_rate']:.1f} % of the {F32_MFMA_FLOPS / 1e12:.0f} TFLOP/s f32-MFMA rate")
            del fp, st, graph, sides
        if not args.no_loop:
            res["loop_go2"] = loop_go2(N, T, dev, args)
    for k in ("fused", "torch_graph") if not args.no_loop else ():
        v = res["loop_go2"]["env_steps_per_s"][k]
        print(f"go2 loop act -> step -> add_step, {T} steps, {k:12s}: median {v['median'] / 1e6:6.2f} M env-steps/s   p10-p90 {v['p10'] / 1e6:6.2f} - {v['p90'] / 1e6:6.2f}")
    print(json.dumps(res))


def time_sides(sides, args):
    for _ in range(args.warmup):
        for f in sides.values():
            burst_us(f, args.burst)
    times = {q: [] for q in sides}
    for _ in range(args.repeats):
        for q, f in sides.items():
            times[q].append(burst_us(f, args.burst))
    return times


def time_recurrent(name, d, m, fp, st, x, N, args):
    dev = x["obs"].device
    z = torch.randn(N, d["A"], device=dev)
    mask = torch.zeros(N, dtype=torch.bool, device=dev)
    state = {w: [torch.zeros(d["layers"], N, d["H"], device=dev) for _ in range(2)] for w in "ac"}
    st.step = 0
    for _ in range(2):                                           # two steps from zero states, so that the second reads computed ones
        fp.act(x["obs"], x["cobs"], storage=st, noise=z, reset=mask)
    for _ in range(2):
        recurrent_row(m, x, st, 1, state, mask, z)
    torch.cuda.synchronize()
    agree = {q: float((getattr(st, q)[0] - getattr(st, q)[1]).abs().max()) for q in ("mu", "values", "sigma")}
    agree["saved_h_a"] = float((st.saved_hidden_states_a[0][0] - st.saved_hidden_states_a[0][1]).abs().max())
    if agree["mu"] > 1e-4 or agree["values"] > 1e-4 or agree["saved_h_a"] > 1e-4 or agree["sigma"] != 0.0:
        sys.exit(f"policy_act_time.py: {name}: the fused launch and the torch ops disagree ({agree}) -- nothing timed")
    mask.copy_(torch.rand(N, device=dev) < 0.02)
    want = args.sides.split(",")
    graph = capture(lambda: recurrent_row(m, x, st, 1, state, mask)) if "torch_graph" in want else None
    sides = {"fused": lambda: fp.act(x["obs"], x["cobs"], storage=st, reset=mask), "torch_graph": graph and graph.replay,
             "torch_eager": lambda: recurrent_row(m, x, st, 1, state, mask)}
    times = time_sides({q: f for q, f in sides.items() if q in want}, args)
    flop, wbytes = work(m, d, N, None)
    out = dict(flop_per_step=flop, weight_bytes=wbytes, row_tile=fp.row_tile(N), step_us={k: stat(v) for k, v in times.items()},
               max_abs_diff_vs_torch=agree)
    print(f"{name}: {flop / 1e9:.2f} GFLOP per step, {wbytes / 1e6:.2f} MB of weights, row tile {out['row_tile']}, "
          f"|mu - torch| {agree['mu']:.1e}, |values - torch| {agree['values']:.1e}, |saved h_a - torch| {agree['saved_h_a']:.1e}")
    for k, v in out["step_us"].items():
        print(f"  {k:12s}: median {v['median']:8.1f} us   min {v['min']:8.1f}   p10-p90 {v['p10']:8.1f} - {v['p90']:8.1f}   max {v['max']:8.1f}")
    if "fused" in times:
        out["fused_flops"] = flop / (out["step_us"]["fused"]["median"] * 1e-6)
        out["fraction_of_f32_mfma_rate"] = out["fused_flops"] / F32_MFMA_FLOPS
        print(f"  fused: {out['fused_flops'] / 1e12:.1f} TFLOP/s = {100 * out['fraction_of_f32_mfma_rate']:.1f} % of the {F32_MFMA_FLOPS / 1e12:.0f} TFLOP/s f32-MFMA rate")
    return out


def loop_go2(N, T, dev, args):
    from hcr_genesis_lr_cl_amd.config import GO2Cfg
    from hcr_genesis_lr_cl_amd.envs import GO2, set_seed
    from hcr_genesis_lr_cl_amd.policy import FusedPolicy
    from hcr_genesis_lr_cl_amd.rollout import RolloutStorage
    cfg = GO2Cfg()
    cfg.env.num_envs = N
    cfg.hip.obs_sets = T + 1
    set_seed(int(cfg.seed))
    env = GO2(cfg, None, dev, True)
    env.reset()
    m = Nets(SETS["go2"]).to(dev)
    fp = FusedPolicy(m, seed=1)
    st = RolloutStorage(N, T, [45], [None], [12], dev, env=env)
    graphs = [capture(lambda t=t: torch_row(m, dict(obs=st.observations[t], cobs=st.observations[t]), st, t, None)) for t in range(T)]

    def loop(kind):
        for t in range(T):
            if kind == "fused":
                fp.act(st.observations[t], st.observations[t], storage=st)
            else:
                graphs[t].replay()
            out = env.step(st.actions[t])
            st.add_step(out[-3], out[-2], out[-1]["time_outs"], 0.99)
        st.clear()

    def sample(kind):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.loops):
            loop(kind)
        torch.cuda.synchronize()
        return N * T * args.loops / (time.perf_counter() - t0)

    kinds = ("fused", "torch_graph")
    for _ in range(args.warmup):
        for k in kinds:
            sample(k)
    rates = {k: [] for k in kinds}
    for _ in range(args.repeats):
        for k in kinds:
            rates[k].append(sample(k))
    return dict(steps=T, loops_per_sample=args.loops, zero_copy=bool(st.zero_copy), env_steps_per_s={k: stat(v) for k, v in rates.items()})


if __name__ == "__main__":
    main()
