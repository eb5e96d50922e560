"""Pins the numpy MDP oracle (oracle/mdp_oracle.py) against golden vectors produced by running
the reference's own GO2 task class (tests/golden/gen_mdp_fixtures.py).  Tolerances: float sums of
12 squares etc. may associate differently than torch -> rtol 2e-6 / atol 2e-6 on floats;
integers, booleans and counters are exact."""
import numpy as np
import pytest

from tests import mdp_harness as h

GOLD, GOLD_WTW, GOLD_EE = h.TASKS["go2"].gold, h.TASKS["go2_wtw"].gold, h.TASKS["go2_ee"].gold
GOLD_TRON1, GOLD_PF, GOLD_SF = h.TASKS["tron1_pf_ee"].gold, h.TASKS["tron1_pf"].gold, h.TASKS["tron1_sf"].gold
ALL_HEADS = ["go2_ts", "go2_cts", "go2_dreamwaq", "go2_cat"]


def head_gold(head):
    return h.TASKS[head].gold


def replay_golden(task):
    """The oracle through the task's golden fixture, every output of tests/mdp_harness.py TASKS at ORACLE_TOL."""
    spec = h.TASKS[task]
    h.replay(spec, h.golden(spec), h.OracleStepper, h.ORACLE_TOL)


def test_fixture_exercises_the_branches():
    fx = np.load(GOLD)
    assert fx["reset"].sum() >= 8 and fx["time_out"].sum() >= 3
    assert (fx["reset"].astype(bool) & ~fx["time_out"].astype(bool)).sum() >= 2      # failure terminations
    assert (fx["counter"] % 750 == 0).any() and (fx["counter"] % 1000 == 0).any()   # push + curriculum steps
    assert fx["cmd_range_x"][-1][1] == 1.0 and fx["cmd_range_x"][0][1] == 0.5        # curriculum fired
    assert np.abs(fx["actions_in"]).max() > 100                                        # action clip exercised


def test_mdp_oracle_reproduces_reference_go2():
    replay_golden("go2")


def test_wtw_fixture_exercises_the_branches():
    fx = np.load(GOLD_WTW)
    assert fx["reset"].sum() >= 6
    th = fx["task_state"][:, :, 6:10]
    assert len({tuple(r) for r in th.reshape(-1, 4)}) >= 4            # several gaits from the table
    assert (fx["task_state"][1:, :, 0] < fx["task_state"][:-1, :, 0]).any()   # gait clock wrapped
    assert (fx["counter"] % 750 == 0).any()


def test_mdp_oracle_reproduces_reference_go2_wtw():
    replay_golden("go2_wtw")


def test_ee_fixture_exercises_the_branches():
    fx = np.load(GOLD_EE)
    assert fx["reset"].sum() >= 8
    assert (fx["terrain_levels"][-1] != fx["init_terrain_levels"]).sum() >= 4      # terrain curriculum moved envs
    assert np.ptp(fx["measured_heights"]) > 0.2 and np.abs(fx["normals"][..., 0]).max() > 0.5
    assert (fx["counter"] % 500 == 0).any()


def test_mdp_oracle_reproduces_reference_go2_ee():
    replay_golden("go2_ee")


def test_cat_fixture_exercises_the_constraints():
    fx = np.load(head_gold("go2_cat"))
    p = fx["cstr_prob"]
    assert (p == 0).any() and (p == 0.25).any() and (p == 1.0).any() and set(np.unique(p)) <= {0.0, 0.25, 1.0}
    seen = fx["cstr_sums"].max(axis=(0, 2)) > 0
    assert seen[[2, 3, 4, 5]].all()                 # action rate, base height, collision, feet stumble all occur
    assert (fx["reset"].sum(1) > 0).any() and (fx["cstr_sums"][-1] < fx["cstr_sums"].max(0)).any()    # counters zeroed at resets


@pytest.mark.parametrize("head", ALL_HEADS)
def test_head_fixture_is_what_the_reference_emits_as_configured(head):
    """17 contact-state links as configured (common_cfgs.py:100-101) although the head's size fields assume 12
    (go2_ts_config.py:8-14): privileged 99 wide / critic frames 177 wide."""
    fx = np.load(head_gold(head))
    assert fx["priv_new"].shape[-1] == 177 and fx["priv_last"].shape[-1] == 5 * 177 and fx["feat_last"].shape[-1] == 20 * 45
    assert fx["labels"].shape[-1] == (69 if head == "go2_dreamwaq" else 99)
    assert fx["reset"].sum() >= 6 and (fx["counter"] % 500 == 0).any()
    np.testing.assert_array_equal(fx["obs"], np.clip(fx["feat_new"], -100, 100))      # obs = newest history frame, clipped


@pytest.mark.parametrize("head", ALL_HEADS)
def test_mdp_oracle_reproduces_reference_head(head):
    replay_golden(head)


def test_tron1_fixture_exercises_the_branches():
    fx = np.load(GOLD_TRON1)
    r = fx["reset"].astype(bool)
    assert r.sum() >= 10
    sit = (np.abs(fx["sim_base_quat"][:, :, 1]) > 0.05) & r
    assert sit.sum() >= 2 and (r & ~sit).sum() >= 2                       # both reset branches (tron1_pf_ee.py:204-210)
    assert (fx["reset"].astype(bool) & ~fx["time_out"].astype(bool)).sum() >= 1
    assert fx["dr_joint"][-1][:, 0].max() > 0.11                           # armature randomised


def test_mdp_oracle_reproduces_reference_tron1_pf_ee():
    replay_golden("tron1_pf_ee")


def test_tron1_pf_fixture_exercises_the_branches():
    fx = np.load(GOLD_PF)
    names = [str(n) for n in fx["reward_names"]]
    assert fx["reset"].sum() >= 8 and (fx["counter"] % 500 == 0).any() and "no_fly" in names and len(names) == 19
    assert fx["obs"].shape[-1] == 5 * 27 and fx["priv"].shape[-1] == 5 * 45
    k = names.index("no_fly")
    d = np.diff(fx["episode_sums"][:, k], axis=0)
    assert (d > 0).any() and (d == 0).any()


def test_mdp_oracle_reproduces_reference_tron1_pf():
    replay_golden("tron1_pf")


def test_tron1_sf_fixture_exercises_the_branches():
    fx = np.load(GOLD_SF)
    names = [str(n) for n in fx["reward_names"]]
    assert fx["reset"].sum() >= 6 and (fx["counter"] % 500 == 0).any() and len(names) == 21
    assert {"foot_flat", "hip_pos_zero_command", "keep_ankle_pitch_zero_in_air", "no_fly"} <= set(names)
    assert fx["obs"].shape[-1] == 10 * 33 and fx["priv"].shape[-1] == 10 * 72
    r = fx["reset"].astype(bool)
    sit = r & (np.abs(fx["sim_dof_pos"][:, :, 2] - 1.35) < 1e-6)            # both reset branches (tron1_sf.py:160-166)
    assert sit.sum() >= 2 and (r & ~sit).sum() >= 2
    for n in ("foot_flat", "hip_pos_zero_command", "keep_ankle_pitch_zero_in_air"):
        d = np.diff(fx["episode_sums"][:, names.index(n)], axis=0)
        assert (np.abs(d) > 0).any(), n
    # tron1_sf.py:224-231: dof 7 is never offset by a reset, dof 0 moves by at most 0.05
    nonsit = r & ~sit
    assert np.all(fx["sim_dof_pos"][:, :, 7][nonsit] == 0) and np.abs(fx["sim_dof_pos"][:, :, 0][nonsit]).max() <= 0.05 + 1e-6


def test_mdp_oracle_reproduces_reference_tron1_sf():
    replay_golden("tron1_sf")
