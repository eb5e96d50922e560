"""The RS instantiations of quad_sim_kernel take more of the launch-invariant configuration as given (lg_shared.h lg_rs_constants_hold,
checked by lg_host.hip's plan() next to the reward set): the configs' branch switches (heading commands, positive
rewards, the domain-randomisation switches, custom origins), the optional buffer the kernel would test for null is bound
(nonfinite_count), the per-env joint parameter arrays are not.  The null tests and flag tests are compiled out; the statements are the
same, so a rollout through the constant form leaves the same BITS in every engine buffer as one through the general form.  The byte
offsets and foot constants of lg_lane_ints.h are shared by both forms and by tron1_pf_ee's kernel, which has no constant form: its two
runs are the same launch and check that the rollout is reproducible.

Two envs of one seed step side by side from reset, 80 steps of a seeded bank of N(0,1) actions, the episode clocks seeded so that every env
times out inside the rollout: with N = 6 the first wave is full and the second ragged (dead lanes shadowing the last env), so the reset
block and every store predicate run in both kinds of wave.  Nothing is copied across, so one differing bit would spread."""
import functools
import os

import pytest

pytestmark = pytest.mark.gpu

STEPS = 80
SWITCH = "LG_REWARD_SET_CONST"
KERNELS = {   # task -> (as plan() chooses, with LG_REWARD_SET_CONST=0)
    "go2": ("(lg_launch_quad_rs<4, 1, false>)", "(lg_launch_quad<4, true, PR, 1, 3>)"),
    "go2_wtw": ("(lg_launch_quad_rs<4, 2, false>)", "(lg_launch_quad<4, true, PR, 2, 3>)"),
    "go2_ee": ("(lg_launch_quad_rs<4, 3, false>)", "(lg_launch_quad<4, true, PR, 3, 3>)"),
    "tron1_pf_ee": ("(lg_launch_quad<2, true, PR, 6, 3>)", "(lg_launch_quad<2, true, PR, 6, 3>)"),
}


def _make(task, n):
    from hcr_genesis_lr_cl_amd.envs import TASKS, set_seed
    cls, cfg_cls = TASKS[task]
    cfg = cfg_cls()
    cfg.env.num_envs = n
    set_seed(int(cfg.seed))
    return cls(cfg, None, "cuda:0", True)


def _bits(t):
    import torch
    return t.view(torch.int32) if t.dtype == torch.float32 else t


@functools.lru_cache(maxsize=None)
def _rollout_pair(task, n, unbind=None):
    """-> (kernel names of run 1, of run 2, {buffer: (first step it differed in bits, elements that differed over the run)}, resets seen by
    run 1 per env).  Run 1 is what plan() chooses; run 2 has LG_REWARD_SET_CONST=0 or, with `unbind`, that optional buffer unbound."""
    import torch
    saved = os.environ.pop(SWITCH, None)
    try:
        e1, e2 = _make(task, n), _make(task, n)
        e1.reset(); e2.reset()
        if unbind:
            e2._engine.buf.pop(unbind)
            e2._engine.bind()
        # every env times out inside the rollout, at its own step (legged_robot.py:78-92: episode_length_buf > max_episode_length)
        clocks = (int(e1.max_episode_length) - 8 - (torch.arange(n, device="cuda") * 7) % 60).to(torch.int32)
        e1.episode_length_buf[:] = clocks
        e2.episode_length_buf[:] = clocks
        g = torch.Generator(device="cuda"); g.manual_seed(4321)
        bank = [torch.randn(n, e1.num_actions, generator=g, device="cuda") for _ in range(16)]
        keys = sorted(k for k in e1._engine.buf.keys() if k != unbind)
        assert keys == sorted(e2._engine.buf.keys())
        names1, names2, diffs = set(), set(), {}
        resets = torch.zeros(n, dtype=torch.int64, device="cuda")
        for t in range(STEPS):
            os.environ.pop(SWITCH, None)
            e1.step(bank[t % 16])
            names1.add(e1._engine.last_kernel())
            if not unbind:
                os.environ[SWITCH] = "0"
            e2.step(bank[t % 16])
            names2.add(e2._engine.last_kernel())
            ne = [_bits(e1._engine.buf.raw(k)) != _bits(e2._engine.buf.raw(k)) for k in keys]
            for k, d, m in zip(keys, torch.stack([d.any() for d in ne]).tolist(), ne):
                if d:
                    first, count = diffs.get(k, (t, 0))
                    diffs[k] = (first, count + int(m.sum()))
            resets += e1.reset_buf.to(torch.int64)
        return names1, names2, diffs, resets.cpu().tolist()
    finally:
        os.environ.pop(SWITCH, None)
        if saved is not None:
            os.environ[SWITCH] = saved


def _report(diffs):
    return "\n".join(f"{k}: first at step {diffs[k][0]}, {diffs[k][1]} elements over the run" for k in sorted(diffs))


@pytest.mark.parametrize("n", [6, 64])
@pytest.mark.parametrize("task", list(KERNELS))
def test_constant_form_and_general_form_leave_the_same_bits_in_every_buffer(task, n):
    names1, names2, diffs, resets = _rollout_pair(task, n)
    assert names1 == {KERNELS[task][0]}, names1
    assert names2 == {KERNELS[task][1]}, names2
    assert min(resets) >= 1, resets          # every env reset (time-out) inside the rollout: full and ragged waves ran the reset block
    assert diffs == {}, "buffers differ:\n" + _report(diffs)


@pytest.mark.parametrize("n", [6, 64])
def test_unbound_optional_buffer_runs_the_general_form_with_the_same_results(n):
    """nonfinite_count is optional (include/lgsim.h): without it the host check refuses the constant form, and the general form leaves what
    the run with the counter bound leaves (the counter stays 0 in a healthy rollout: nothing else depends on it)."""
    names1, names2, diffs, resets = _rollout_pair("go2", n, unbind="nonfinite_count")
    assert names1 == {KERNELS["go2"][0]}, names1
    assert names2 == {KERNELS["go2"][1]}, names2
    assert min(resets) >= 1, resets
    assert diffs == {}, "buffers differ:\n" + _report(diffs)
