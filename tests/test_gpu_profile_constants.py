"""The RS instantiations of quad_sim_kernel have the profile's defaults as compile-time constants: the reward set and the solver options
(two contact sweeps, W recomputed on every sub-step; lg_shared.h LG_DEFAULT_CONTACT_*).  The constant form runs the same statements in the
same order as the general one, so a rollout through either is to leave the same BITS in every engine buffer after every step; lg_host.hip's
plan() picks it only when the reward set and the engine's options are the defaults (LG_REWARD_SET_CONST=0 forces the general form).

Two envs of one seed step side by side from reset, 80 steps of a seeded bank of N(0,1) actions (standing, falling, body-sphere contact,
joint-limit stops and resets all occur), the first as plan() chooses, the second with LG_REWARD_SET_CONST=0.  The rollouts are left alone
(no state is copied across), so one differing bit anywhere in the physics would spread.  The buffers are checked in two groups: everything
the step computes but the reward sums (state, forces, observations, commands, episode clocks, draws), and the reward sums (rew_buf,
episode_sums, episode_done_sums)."""
import functools
import os

import pytest

pytestmark = pytest.mark.gpu

STEPS = 80
PROFILE = {"go2": 1, "go2_wtw": 2, "go2_ee": 3}
REWARD_SUMS = ("rew_buf", "episode_sums", "episode_done_sums")
SWITCH = "LG_REWARD_SET_CONST"


def _make(task, n, hip):
    from hcr_genesis_lr_cl_amd.envs import TASKS, set_seed
    cls, cfg_cls = TASKS[task]
    cfg = cfg_cls()
    cfg.env.num_envs = n
    for k, v in hip:
        setattr(cfg.hip, k, v)
    set_seed(int(cfg.seed))
    return cls(cfg, None, "cuda:0", True)


def _bits(t):
    import torch
    return t.view(torch.int32) if t.dtype == torch.float32 else t


@functools.lru_cache(maxsize=None)
def _rollout_pair(task, n, hip=()):
    """-> (kernel names of the default run, of the LG_REWARD_SET_CONST=0 run, {buffer: (first step it differed in bits, elements that
    differed over the run, largest absolute difference)}, resets seen).  Computed once per case and shared by the tests below."""
    import torch
    saved = os.environ.pop(SWITCH, None)
    try:
        e1, e2 = _make(task, n, hip), _make(task, n, hip)
        e1.reset(); e2.reset()
        g = torch.Generator(device="cuda"); g.manual_seed(1234)
        bank = [torch.randn(n, e1.num_actions, generator=g, device="cuda") for _ in range(16)]
        keys = sorted(e1._engine.buf.keys())
        assert keys == sorted(e2._engine.buf.keys())
        names1, names2, diffs, n_reset = set(), set(), {}, 0
        for t in range(STEPS):
            os.environ.pop(SWITCH, None)
            e1.step(bank[t % 16])
            names1.add(e1._engine.last_kernel())
            os.environ[SWITCH] = "0"
            e2.step(bank[t % 16])
            names2.add(e2._engine.last_kernel())
            ne = [_bits(e1._engine.buf.raw(k)) != _bits(e2._engine.buf.raw(k)) for k in keys]
            for k, d in zip(keys, torch.stack([d.any() for d in ne]).tolist()):
                if d:
                    a, b = e1._engine.buf.raw(k).double(), e2._engine.buf.raw(k).double()
                    first, count, worst = diffs.get(k, (t, 0, 0.0))
                    diffs[k] = (first, count + int(ne[keys.index(k)].sum()), max(worst, float((a - b).abs().nan_to_num().max())))
            n_reset += int(e1.reset_buf.sum())
        return names1, names2, diffs, n_reset
    finally:
        os.environ.pop(SWITCH, None)
        if saved is not None:
            os.environ[SWITCH] = saved


def _report(diffs, keys):
    return "\n".join(f"{k}: first at step {diffs[k][0]}, {diffs[k][1]} elements over the run, max abs diff {diffs[k][2]:.3e}" for k in keys)


CASES = [(task, n) for task in ("go2", "go2_wtw", "go2_ee") for n in (6, 64)]     # 6: the second wave is half dead lanes that shadow the last env


@pytest.mark.parametrize("task,n", CASES)
def test_the_two_runs_use_the_constant_and_the_general_instantiation(task, n):
    names1, names2, _, n_reset = _rollout_pair(task, n)
    assert names1 == {f"(lg_launch_quad_rs<4, {PROFILE[task]}, false>)"}, names1
    assert names2 == {f"(lg_launch_quad<4, true, PR, {PROFILE[task]}, 3>)"}, names2
    if n == 64:
        assert n_reset > 0


@pytest.mark.parametrize("task,n", CASES)
def test_constant_form_leaves_the_same_bits_in_every_buffer_but_the_reward_sums(task, n):
    _, _, diffs, _ = _rollout_pair(task, n)
    bad = sorted(k for k in diffs if k not in REWARD_SUMS)
    print(_report(diffs, sorted(diffs)))
    assert bad == [], "buffers differ:\n" + _report(diffs, bad)


@pytest.mark.parametrize("task,n", CASES)
def test_constant_form_leaves_the_same_bits_in_the_reward_sums(task, n):
    """The reward total adds each term's rounded product (lg_quad.h `add`: contraction off for that sum).  Left to the compiler, a term alone
    in its basic block (general form) got a multiply-add and the terms of the constant set did not: rew_buf differed in its last bit
    (at most 5.4e-8 over these runs) in one or two of a hundred env-steps."""
    _, _, diffs, _ = _rollout_pair(task, n)
    bad = sorted(k for k in diffs if k in REWARD_SUMS)
    assert bad == [], "buffers differ:\n" + _report(diffs, bad)


@pytest.mark.parametrize("hip", [(("contact_iters", 3),), (("contact_w_every", 2),)], ids=["sweeps-3", "reused-w-2"])
def test_other_solver_options_run_the_general_instantiation(hip):
    """The host check refuses the constant form: the default run reports the general kernel too, and the two runs are the same launch."""
    names1, names2, diffs, _ = _rollout_pair("go2", 64, hip)
    assert names1 == names2 == {"(lg_launch_quad<4, true, PR, 1, 3>)"}, (names1, names2)
    assert diffs == {}, _report(diffs, sorted(diffs))
