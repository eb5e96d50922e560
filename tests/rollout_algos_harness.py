"""Shared by tests/test_rollout_algos.py and tests/golden/gen_rollout_algos_fixtures.py: what the storages of the explicit-estimator (EE),
teacher-student (TS), concurrent teacher-student (CTS) and DreamWaQ learners look like from outside, stated once, and a float64
restatement of the CTS return computation.  numpy only; nothing here imports the package, the reference or torch.

  * WIDTHS / CTOR / ROWS: the fixture's shapes, each constructor's shape arguments in order, and which Transition attribute lands in
    which stored tensor (rsl_rl/storage/rollout_storage_{ee,ts,cts,dreamwaq}.py, `__init__` and `add_transitions`);
  * TAGGED / tag_base / tag_ids: column 0 of stored tensor k holds (k + 1) * T * N + t * N + e, so a gathered row names the tensor and the
    sample it came from; k + 1 keeps every tag above 1, so a column of zeros and ones can only be `terminated = 1 - dones`;
  * LAYOUTS: per class, (stored tensor, index set) of every mini-batch entry before the closing `(None, None), None`; "dones" stands
    for the float32 `1 - dones` entry.  test_layouts_match_the_fixture pins them to what the reference's generators yielded;
  * gae_groups_f64: rollout_storage_cts.py:81-114 in float64."""
import numpy as np

N, T, NUM_TEACHER = 12, 5, 5
GAMMA, LAM = 0.99, 0.95
CLASSES = ("EE", "TS", "CTS", "DreamWaQ")
WIDTHS = dict(observations=7, privileged_observations=9, observation_histories=14, critic_observations=11, estimator_features=6,
              estimator_labels=4, explicit_info_labels=5, next_states=8, actions=3)
_TS = ("observations", "privileged_observations", "observation_histories", "critic_observations", "actions")
CTOR = {"EE": ("privileged_observations", "estimator_features", "estimator_labels", "actions"), "TS": _TS, "CTS": _TS,
        "DreamWaQ": ("observations", "privileged_observations", "observation_histories", "explicit_info_labels", "next_states", "actions")}
_SAME = lambda *names: tuple((n, n) for n in names)
# env-side rows: (Transition attribute = add_step keyword, stored tensor)
ROWS = {"EE": (("critic_observations", "privileged_observations"),) + _SAME("estimator_features", "estimator_labels"),
        "TS": _SAME("observations", "privileged_observations", "observation_histories", "critic_observations"),
        "CTS": _SAME("observations", "privileged_observations", "observation_histories", "critic_observations"),
        "DreamWaQ": _SAME("observations", "privileged_observations", "observation_histories", "explicit_info_labels", "next_states")}
# policy-side rows: (Transition attribute, stored tensor); values and actions_log_prob are one column wide and carry data, not tags, while
# the returns are computed: they are tagged afterwards, with the computed tensors
POLICY_ROWS = (("actions", "actions"), ("values", "values"), ("actions_log_prob", "actions_log_prob"), ("action_mean", "mu"), ("action_sigma", "sigma"))
COMPUTED = ("values", "actions_log_prob", "returns", "advantages", "teacher_advantages", "student_advantages")
TAGGED = ("observations", "privileged_observations", "observation_histories", "critic_observations", "estimator_features", "estimator_labels",
          "explicit_info_labels", "next_states", "actions", "mu", "sigma") + COMPUTED

_PPO = ("actions", "values", "advantages", "returns", "actions_log_prob", "mu", "sigma")
_one_set = lambda *names: [(n, 0) for n in names + _PPO]
LAYOUTS = {
    "EE": _one_set("privileged_observations", "estimator_features", "estimator_labels", "dones"),
    "TS": _one_set("observations", "privileged_observations", "observation_histories", "critic_observations", "dones"),
    "DreamWaQ": _one_set("observations", "privileged_observations", "observation_histories", "explicit_info_labels", "next_states", "dones"),
    "CTS": [(n, 0) for n in ("observations", "privileged_observations", "actions", "actions_log_prob", "teacher_advantages", "mu", "sigma")]
           + [(n, 1) for n in ("observations", "privileged_observations", "observation_histories", "actions", "actions_log_prob", "student_advantages")]
           + [(n, 2) for n in ("critic_observations", "values", "returns")],
}
ARITY = {"EE": 13, "TS": 14, "DreamWaQ": 15, "CTS": 18}


def ctor_args(cls, n_envs, n_steps, num_teacher, widths=WIDTHS):
    """Positional constructor arguments of class `cls` in the reference's order (the device is the caller's)."""
    shapes = [[widths[k]] for k in CTOR[cls]]
    return [n_envs] + ([num_teacher] if cls == "CTS" else []) + [n_steps] + shapes


def width_of(name, widths=WIDTHS):
    return widths.get("actions" if name in ("mu", "sigma") else name, 1)


def tag_base(name, n_steps, n_envs):
    assert (len(TAGGED) + 1) * n_steps * n_envs < 1 << 24, "float32 must hold every tag"
    return (TAGGED.index(name) + 1) * n_steps * n_envs


def tag_ids(n_steps, n_envs, first=0, group=None):
    """Sample ids t * n_envs + e of envs [first, first + group) as a (T, group) float32 array."""
    group = n_envs - first if group is None else group
    return (np.arange(n_steps)[:, None] * n_envs + first + np.arange(group)[None, :]).astype(np.float32)


def decode(column, n_steps, n_envs):
    """(tensor name, sample ids) of a tagged column 0; ("dones", None) for a column of zeros and ones."""
    c = np.asarray(column, np.float64)
    if np.isin(c, (0.0, 1.0)).all():
        return "dones", None
    k = np.unique(c // (n_steps * n_envs))
    assert len(k) == 1 and 1 <= k[0] <= len(TAGGED) and (c == np.round(c)).all(), "not one tensor's tags"
    return TAGGED[int(k[0]) - 1], (c % (n_steps * n_envs)).astype(np.int64)


def gae_groups_f64(values, rewards, dones, last_values, gamma, lam, n_first):
    """rollout_storage_cts.py:81-114 in float64 from float32 inputs ((T, N, 1) arrays); gamma and lam rounded to float32 first, as the
    kernel's ABI receives them.  The recurrence is per env, so the reference's two passes are one; each group is normalised by its own
    mean and unbiased std.  Returns (returns, raw advantages, normalised advantages of [0, n_first), of [n_first, N)), all float64."""
    g = np.float64(np.float32(gamma))
    gl = g * np.float64(np.float32(lam))
    v, r = np.asarray(values, np.float64), np.asarray(rewards, np.float64)
    nt = 1.0 - np.asarray(dones).astype(np.float64)
    returns, adv = np.zeros_like(v), np.zeros_like(v[0])
    nv = np.asarray(last_values, np.float64).reshape(v[0].shape)
    for t in reversed(range(v.shape[0])):
        delta = r[t] + nt[t] * g * nv - v[t]
        adv = delta + nt[t] * gl * adv
        returns[t] = adv + v[t]
        nv = v[t]
    raw = returns - v
    return returns, raw, normalise_f64(raw[:, :n_first]), normalise_f64(raw[:, n_first:])


def normalise_f64(raw):
    a = np.asarray(raw).astype(np.float64)
    return (a - a.mean()) / (a.std(ddof=1) + 1e-8)
