"""Golden vectors for the fused PPO loss head (include/lgppo.h) from the reference's own classes: PPO._compute_rl_loss
(rsl_rl/algorithms/ppo.py:157-218) on an ActorCritic and PPO_CTS._compute_rl_loss (ppo_cts.py:193-267) on an ActorCriticCTS, tiny hidden
sizes, everything .double() on the CPU.

Build-container only:   PYTHONDONTWRITEBYTECODE=1 python tests/golden/gen_ppo_loss_fixtures.py
Output: tests/golden/ppo_loss.npz.  `cases` lists the case names; per case, under "<case>.<key>":
  cfg                    [clipped value loss, SPO, entropy_coef, clip_param, value_loss_coef, policy groups]
  g<i>.actions, .old_log_prob, .advantages, .old_mu, .old_sigma     the stored columns of policy group i, float32 (fed as .double())
  returns, target_values                                           float32
  g<i>.mu, g<i>.sigma, values    action_mean, action_std and the value batch of the double networks inside the call, float64
  loss, g<i>.surrogate, value_loss, entropy                         what the call returned (entropy: the mean the loss used), float64
  g<i>.grad_mu, g<i>.grad_sigma, grad_values                        torch.autograd.grad(loss, [mu, sigma, value]), float64
  desired_kl, lr_after          three desired_kl settings of the adaptive schedule and the learning rate after the call from 1e-3: it
                                falls, rises and stays
The old log-probs and target values are chosen (tests/ppo_loss_cases.py: gap_ratio, gap_step) so that rows fall on both sides of every
clip and none sits on one.  Written through ref_harness.save; `python tests/golden/check_fixtures.py` checks that the output still
equals the committed file."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import ref_harness as rh  # noqa: E402

rh.load_reference()
import torch  # noqa: E402

import ppo_loss_cases as pc  # noqa: E402

LR0 = 1e-3
# name -> policy rows per group, actions, clipped value loss, SPO, entropy_coef, value_loss_coef
FIXTURE_CASES = {
    "clip_cv":     dict(rows=[65], A=12, clipped=True, spo=False, ent=0.01, vlc=1.0),
    "clip_cv_e0":  dict(rows=[33], A=5, clipped=True, spo=False, ent=0.0, vlc=0.5),
    "clip_plain":  dict(rows=[64], A=3, clipped=False, spo=False, ent=0.0, vlc=1.0),
    "spo_cv":      dict(rows=[63], A=12, clipped=True, spo=True, ent=0.01, vlc=1.0),
    "spo_plain":   dict(rows=[17], A=1, clipped=False, spo=True, ent=0.0, vlc=2.0),
    "cts_17_5":    dict(rows=[17, 5], A=12, clipped=True, spo=False, ent=0.01, vlc=1.0),
}


def kl_mean(mu, sigma, old_mu, old_sigma):
    return float(np.mean(np.sum(np.log(sigma / old_sigma + 1.e-5) + (old_sigma ** 2 + (old_mu - mu) ** 2) / (2.0 * sigma ** 2) - 0.5, axis=-1)))


def one_case(name, c, seed):
    from rsl_rl.algorithms import PPO, PPO_CTS
    from rsl_rl.modules import ActorCritic, ActorCriticCTS
    torch.manual_seed(seed)
    rng = np.random.default_rng(seed)
    A, cts = c["A"], len(c["rows"]) == 2
    n_obs, n_cobs, n_priv, n_hist, n_lat = 7, 9, 6, 14, 4
    kw = dict(clip_param=pc.CLIP, value_loss_coef=c["vlc"], entropy_coef=c["ent"], use_clipped_value_loss=c["clipped"], schedule="adaptive",
              learning_rate=LR0, device="cpu")
    if cts:
        ac = ActorCriticCTS(n_obs, A, n_priv, n_hist, n_lat, n_cobs, actor_hidden_dims=[16, 8], critic_hidden_dims=[16, 8],
                            privilege_encoder_hidden_dims=[8], history_encoder_hidden_dims=[8]).double()
        alg = PPO_CTS(ac, num_teacher=c["rows"][0], **kw)
    else:
        ac = ActorCritic(n_obs, n_cobs, A, actor_hidden_dims=[16, 8], critic_hidden_dims=[16, 8]).double()
        alg = PPO(ac, use_spo=c["spo"], **kw)
    with torch.no_grad():
        ac.std.copy_(torch.from_numpy(0.5 + 0.7 * rng.random(A)))
    f32 = lambda x: np.ascontiguousarray(x, dtype=np.float32)
    d = lambda x: torch.from_numpy(np.asarray(x)).double()

    # the network outputs the call will see, to place the stored columns around them
    groups = []
    for gi, B in enumerate(c["rows"]):
        obs = f32(rng.normal(size=(B, n_obs)))
        extra = (f32(rng.normal(size=(B, n_hist))), f32(rng.normal(size=(B, n_priv)))) if cts else ()
        with torch.no_grad():
            if cts:
                ac.act(d(obs), d(extra[0]), d(extra[1]), act_type="teacher" if gi == 0 else "student")
            else:
                ac.act(d(obs))
            mu, sigma = ac.action_mean.numpy().copy(), ac.action_std.numpy().copy()
        old_mu, old_sigma = f32(mu + 0.1 * sigma * rng.normal(size=mu.shape)), f32(sigma * np.exp(0.05 * rng.normal(size=mu.shape)))
        actions = f32(old_mu + old_sigma * rng.normal(size=mu.shape))
        groups.append(dict(obs=obs, extra=extra, actions=actions, old_mu=old_mu, old_sigma=old_sigma, advantages=f32(rng.normal(size=(B, 1))),
                           old_log_prob=pc.old_log_prob_for(mu, sigma, actions, pc.gap_ratio(rng, B)).reshape(B, 1), kl=kl_mean(mu, sigma, old_mu, old_sigma)))
    Bv = sum(c["rows"])
    cobs = f32(rng.normal(size=(Bv, n_cobs)))
    with torch.no_grad():
        v0 = ac.evaluate(d(cobs)).numpy().copy()
    target_values = f32(v0 - pc.gap_step(rng, Bv).reshape(Bv, 1))
    returns = f32(target_values + 0.5 * rng.normal(size=(Bv, 1)))

    # keep what the call computes inside: the distribution of every act, the value batch of evaluate
    seen = dict(dist=[], values=[])
    act0, eval0 = ac.act, ac.evaluate

    def act(*a, **k):
        out = act0(*a, **k)
        seen["dist"].append((ac.distribution.loc, ac.distribution.scale))
        return out

    def evaluate(*a, **k):
        out = eval0(*a, **k)
        seen["values"].append(out)
        return out
    ac.act, ac.evaluate = act, evaluate

    def call(desired_kl):
        alg.learning_rate, alg.desired_kl = LR0, desired_kl
        seen["dist"].clear(); seen["values"].clear()
        hid, masks = (None, None), None
        if cts:
            t, s = groups
            return alg._compute_rl_loss(d(t["obs"]), d(t["extra"][1]), d(t["actions"]), d(t["old_log_prob"]), d(t["advantages"]), d(t["old_mu"]),
                                        d(t["old_sigma"]), d(s["obs"]), d(s["extra"][0]), d(s["actions"]), d(s["old_log_prob"]), d(s["advantages"]),
                                        d(cobs), d(target_values), d(returns), hid, masks)
        g = groups[0]
        return alg._compute_rl_loss(d(g["obs"]), d(cobs), d(g["actions"]), d(target_values), d(g["advantages"]), d(returns), d(g["old_log_prob"]),
                                    d(g["old_mu"]), d(g["old_sigma"]), hid, masks)

    kl = groups[0]["kl"]
    desired = np.array([kl / 4.0, kl * 4.0, kl])
    lr_after = []
    for dk in desired:
        out = call(float(dk))
        lr_after.append(alg.learning_rate)
    assert lr_after[0] < LR0 < lr_after[1] and lr_after[2] == LR0, (name, kl, lr_after)
    loss, surrogates, value_loss = out[0], out[1:-1], out[-1]
    leaves = [x for pair in seen["dist"] for x in pair] + [seen["values"][0]]
    assert len(seen["dist"]) == len(groups) and len(seen["values"]) == 1
    grads = torch.autograd.grad(loss, leaves)
    n = lambda x: x.detach().numpy().astype(np.float64).copy()
    ent_rows = torch.cat([(0.5 + 0.5 * np.log(2 * np.pi) + torch.log(sg)).sum(-1) for _, sg in seen["dist"]])
    entropy = ent_rows.mean()
    # the entropy mean is not returned by the call: recover it from the loss it entered and check it against the rows
    if c["ent"]:
        from_loss = (sum(surrogates) + c["vlc"] * value_loss - loss) / c["ent"]
        assert abs(float(from_loss) - float(entropy)) < 1e-9 * max(1.0, abs(float(entropy))), (name, float(from_loss), float(entropy))
    arrays = {f"{name}.cfg": np.array([c["clipped"], c["spo"], c["ent"], pc.CLIP, c["vlc"], len(groups)], np.float64)}
    for gi, g in enumerate(groups):
        for k in ("actions", "old_log_prob", "advantages", "old_mu", "old_sigma"):
            arrays[f"{name}.g{gi}.{k}"] = g[k]
        arrays[f"{name}.g{gi}.mu"], arrays[f"{name}.g{gi}.sigma"] = n(seen["dist"][gi][0]), n(seen["dist"][gi][1])
        arrays[f"{name}.g{gi}.surrogate"] = n(surrogates[gi])
        arrays[f"{name}.g{gi}.grad_mu"], arrays[f"{name}.g{gi}.grad_sigma"] = n(grads[2 * gi]), n(grads[2 * gi + 1])
    arrays.update({f"{name}.returns": returns, f"{name}.target_values": target_values, f"{name}.values": n(seen["values"][0]),
                   f"{name}.loss": n(loss), f"{name}.value_loss": n(value_loss), f"{name}.entropy": n(entropy),
                   f"{name}.grad_values": n(grads[-1]), f"{name}.desired_kl": desired, f"{name}.lr_after": np.array(lr_after, np.float64)})
    return arrays, (name, float(loss), kl)


def main(seed=41):
    arrays, info = {"cases": np.array(list(FIXTURE_CASES))}, []
    for i, (name, c) in enumerate(FIXTURE_CASES.items()):
        a, line = one_case(name, c, seed + i)
        arrays.update(a)
        info += line
    rh.save("ppo_loss", arrays, *info)


if __name__ == "__main__":
    main()
