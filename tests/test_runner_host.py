"""The training loop's host side (hcr_genesis_lr_cl_amd/runner.py, include/lgrunner.h), no GPU: the restatement of tests/runner_cases.py
against the reference's own run (tests/golden/runner_learn.npz), abi.py against the header, and every refusal that comes before a launch."""
import ctypes as C
import os
import re
import sys
import types

import numpy as np
import pytest
import torch

from hcr_genesis_lr_cl_amd import abi, runner
from tests import runner_cases as rc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "lgrunner.h")


@pytest.fixture(scope="module")
def fx():
    return rc.load_fixture()


# ---- the restatement is the reference's book-keeping ------------------------------------------------------------------------------------------
def test_restatement_reproduces_the_reference_deques_bit_for_bit(fx):
    c = fx["cfg"]
    r = rc.StatsRestatement(c["num_envs"], c["capacity"])
    assert int(fx["dones"].sum()) > c["capacity"], "the fixture's ring does not wrap"
    for it in range(c["iterations"]):
        for s in range(it * c["steps"], (it + 1) * c["steps"]):
            r.update(fx["rew"][s], fx["dones"][s])
        n = int(fx["buffer_len"][it])
        assert len(r.rewbuffer) == n
        assert np.array_equal(rc.bits(list(r.rewbuffer)), rc.bits(fx["rewbuffer"][it, :n])), f"rewbuffer, iteration {it}"
        assert np.array_equal(rc.bits(list(r.lenbuffer)), rc.bits(fx["lenbuffer"][it, :n])), f"lenbuffer, iteration {it}"
    assert fx["buffer_len"][-1] == c["capacity"] and fx["buffer_len"][0] < c["capacity"]


def test_restatement_reproduces_the_reference_episode_scalars(fx):
    """Episode/<key> of the reference is the mean over the iteration's steps of float32 per-step values; the restatement forms both in
    float64.  A per-step value is a float32 mean of at most N terms and one float32 division: at most (N + 2) roundings of half an ulp of
    the largest |term| / episode_length_s.  The twin's mean over T such values in float32 adds at most T + 1 more."""
    c = fx["cfg"]
    N, T = c["num_envs"], c["steps"]
    per_step = rc.fixture_episode_values(fx)
    names = [str(n) for n in fx["scalar_names"]]
    unit = float(np.abs(fx["ep_sums"]).max()) / c["episode_length_s"] * 2.0 ** -24
    for it in range(c["iterations"]):
        want = per_step[it * T:(it + 1) * T].mean(axis=0)
        for r, key in enumerate(fx["ep_keys"]):
            col = names.index("Episode/" + key)
            err64, err32 = abs(fx["scalar_values"][it, col] - want[r]), abs(fx["scalar_values32"][it, col] - want[r])
            print(f"iteration {it} {key}: |f64 run - restatement| = {err64:.3e}, twin {err32:.3e}, units {unit:.3e}")
            assert err64 <= (N + 2) * unit and err32 <= (N + 2 + T + 1) * unit


def test_ring_restatement_keeps_the_last_cap_of_an_oversized_step():
    r = rc.StatsRestatement(5, 3)
    r.update(np.arange(5, dtype=np.float32), np.ones(5, np.uint8))
    assert list(r.rewbuffer) == [2.0, 3.0, 4.0] and r.count == 5


def test_case_table_covers_its_edges():
    for cap in rc.STATS_CAP:
        for n in rc.STATS_N:
            counts = rc.done_counts(n, cap)
            assert counts[:3] == [1, min(cap, n), 0] and counts[-1] == n
        if cap > 1:
            assert rc.wraps_mid_step(rc.stats_inputs(4096, cap, 1)[1], cap)
    rew, _ = rc.stats_inputs(65, 7, 2)
    assert np.isnan(rew).sum() == 1 and np.isinf(rew).sum() == 1


# ---- abi.py against include/lgrunner.h ---------------------------------------------------------------------------------------------------------
def _prototypes():
    h = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    out = {}
    for name, params in re.findall(r"\bint\s+(lg_runner_\w+)\s*\((.*?)\)\s*;", h, flags=re.S):
        out[name] = tuple(re.sub(r"\s+", " ", re.sub(r"\s*\b\w+$", "", p.strip())) for p in params.split(","))
    return out


def test_signatures_and_constants_match_header():
    protos = _prototypes()
    assert set(protos) == set(abi.RUNNER_EXPORTS) == set(abi.RUNNER_SIGNATURES)
    for name, types_ in protos.items():
        assert types_ == abi.RUNNER_SIGNATURES[name], name
    d = dict(re.findall(r"#define\s+(LG_RUNNER_\w+)\s+(\d+)", open(HEADER).read()))
    assert {k: int(v) for k, v in d.items()} == {"LG_RUNNER_THREADS": abi.RUNNER_THREADS, "LG_RUNNER_INFO_THREADS": abi.RUNNER_INFO_THREADS,
                                                 "LG_RUNNER_MAX_ROWS": abi.RUNNER_MAX_ROWS}


def test_header_compiles_as_c():
    import subprocess
    import tempfile
    with tempfile.TemporaryDirectory() as d:
        src = os.path.join(d, "p.c")
        open(src, "w").write(f'#include "{HEADER}"\nint main(void){{return LG_RUNNER_THREADS == 1024 ? 0 : 1;}}\n')
        subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-o", os.path.join(d, "p"), src], check=True)
        subprocess.run([os.path.join(d, "p")], check=True)


def _lib():
    if not os.path.exists(abi.lib_path()):
        from hcr_genesis_lr_cl_amd import build
        build.build()
    return abi.load_lib()


def test_library_exports_every_declared_symbol_with_the_bound_types():
    lib = _lib()
    ctype = lambda t: C.c_void_p if "*" in t else {"int32_t": C.c_int32, "double": C.c_double}[t]
    for name, types_ in _prototypes().items():
        fn = getattr(lib, name)
        assert fn.restype is C.c_int and list(fn.argtypes) == [ctype(t) for t in types_], name


# ---- refusals before any launch ----------------------------------------------------------------------------------------------------------------
P = 4096        # a non-null address that no refused call reads


def _refused(rc_, lib, text):
    assert rc_ != 0
    assert text in lib.lg_last_error().decode(), lib.lg_last_error().decode()


def test_episode_stats_entry_point_refusals():
    lib = _lib()
    f = lib.lg_runner_episode_stats
    _refused(f(0, P, P, P, P, P, P, 100, P, None), lib, "n < 1")
    _refused(f(8, P, P, P, P, P, P, 0, P, None), lib, "cap < 1")
    _refused(f(8, P, P, P, P, P, P, -3, P, None), lib, "cap < 1")
    for k in range(7):
        ptrs = [P] * 7
        ptrs[k] = None
        _refused(f(8, *ptrs[:6], 100, ptrs[6], None), lib, "null argument")


def test_episode_info_entry_point_refusals():
    lib = _lib()
    f = lib.lg_runner_episode_info
    _refused(f(0, 3, P, 8, 0, None, 0, P, 0, 1.0, P, P, P, None), lib, "n < 1")
    _refused(f(8, 0, P, 8, 0, None, 0, P, 0, 1.0, P, P, P, None), lib, "rows_a < 1")
    _refused(f(8, 3, P, 8, -1, None, 0, P, 0, 1.0, P, P, P, None), lib, "rows_b < 0")
    _refused(f(8, 1000, P, 8, 25, P, 8, P, 0, 1.0, P, P, P, None), lib, "LG_RUNNER_MAX_ROWS")
    _refused(f(8, 3, P, 7, 0, None, 0, P, 0, 1.0, P, P, P, None), lib, "row stride below n")
    _refused(f(8, 3, P, 8, 2, P, 7, P, 0, 1.0, P, P, P, None), lib, "row stride below n")
    _refused(f(8, 3, P, 8, 2, None, 8, P, 0, 1.0, P, P, P, None), lib, "null argument")
    for k in (2, 7, 10, 11, 12):
        args = [8, 3, P, 8, 0, None, 0, P, 0, 1.0, P, P, P, None]
        args[k] = None
        _refused(f(*args), lib, "null argument")


def _module(**extra):
    return rc.make_actor_critic(7, 9, 3, [16, 8], [16, 8], **extra)


FAMILIES = (("memory_a", "ActorCriticRecurrent"), ("memory_c", "ActorCriticRecurrent"), ("estimator", "ActorCriticEE"),
            ("privilege_encoder", "ActorCriticTS / ActorCriticCTS"), ("history_encoder", "ActorCriticTS / ActorCriticCTS"),
            ("vae", "ActorCriticDreamWaQ"))


def _env():
    return types.SimpleNamespace(num_envs=4, num_obs=7, num_privileged_obs=9, num_actions=3, device="cpu", max_episode_length=1000)


def _cfg():
    return rc.train_cfg(rc.load_fixture())


@pytest.mark.parametrize("attr,family", FAMILIES)
def test_foreign_families_are_refused_by_name(attr, family):
    m = _module(**{attr: torch.nn.Linear(2, 2)})
    with pytest.raises(ValueError, match=re.escape(f"PPO: the module has .{attr} ({family})")):
        runner.PPO(m)
    with pytest.raises(ValueError, match=re.escape(f"OnPolicyRunner: the module has .{attr} ({family})")):
        runner.OnPolicyRunner(_env(), _cfg(), actor_critic=m)


def test_recurrent_flag_and_foreign_class_names_are_refused():
    m = _module()
    m.is_recurrent = True
    with pytest.raises(ValueError, match="PPO: the module is recurrent"):
        runner.PPO(m)
    for key, name in (("policy_class_name", "ActorCriticRecurrent"), ("algorithm_class_name", "PPO_TS")):
        cfg = _cfg()
        cfg["runner"][key] = name
        with pytest.raises(ValueError, match=f"OnPolicyRunner: {key} = '{name}'"):
            runner.OnPolicyRunner(_env(), cfg, actor_critic=_module())
    with pytest.raises(ValueError, match="PPO: schedule = 'linear'"):
        runner.PPO(_module(), schedule="linear")


def test_cpu_module_has_no_cpu_path():
    with pytest.raises(ValueError, match=re.escape("PPO: the module is on cpu, not on a HIP device (there is no CPU path)")):
        runner.PPO(_module())
    with pytest.raises(ValueError, match=re.escape("PPO: the module is on cpu, not on a HIP device (there is no CPU path)")):
        runner.PPO(_module(), device="cpu")
    with pytest.raises(ValueError, match=re.escape("OnPolicyRunner: the module is on cpu, not on a HIP device (there is no CPU path)")):
        runner.OnPolicyRunner(_env(), _cfg(), actor_critic=_module())
    with pytest.raises(ValueError, match=re.escape("EpisodeStats: the module is on cpu")):
        runner.EpisodeStats(8, 100, "cpu")


def test_missing_writer_is_refused(monkeypatch, tmp_path):
    monkeypatch.setitem(sys.modules, "torch.utils.tensorboard", None)        # as on a machine without tensorboard
    with pytest.raises(ValueError, match="pass writer="):
        runner.OnPolicyRunner(_env(), _cfg(), log_dir=str(tmp_path), actor_critic=_module())


def test_capacity_below_one_is_refused():
    for cap in (0, -1):
        with pytest.raises(ValueError, match="EpisodeStats: capacity"):
            runner.EpisodeStats(8, cap, "cuda:0")
    with pytest.raises(ValueError, match="EpisodeStats: num_envs"):
        runner.EpisodeStats(0, 100, "cuda:0")
