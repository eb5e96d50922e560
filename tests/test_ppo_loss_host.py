"""Host side of the fused PPO loss head (hcr_genesis_lr_cl_amd/ppo_loss.py, include/lgppo.h): the ctypes mirror against the header, the
launch plan, every refusal of the entry points and of the Python surface, the float64 restatement of tests/ppo_loss_cases.py against the
golden fixture of the reference's own classes (tests/golden/ppo_loss.npz), the learning-rate rule, the coverage of the case table and
the parity rule that tests/test_gpu_ppo_loss.py holds the kernel to.  No GPU needed: nothing is launched."""
import ctypes as C
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest
import torch

from hcr_genesis_lr_cl_amd import abi, ppo_loss
from tests import ppo_loss_cases as pc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "lgppo.h")
FIXTURE = os.path.join(ROOT, "tests", "golden", "ppo_loss.npz")


# ---- the struct ---------------------------------------------------------------------------------------------------------------------------
def test_struct_layout_matches_header():
    structs = [("LgPpoGroup", abi.LgPpoGroup), ("LgPpoLossArgs", abi.LgPpoLossArgs)]
    consts = dict(LG_PPO_MAX_ACTIONS=abi.PPO_MAX_ACTIONS, LG_PPO_MAX_GROUPS=abi.PPO_MAX_GROUPS, LG_PPO_CLIPPED_VALUE=abi.PPO_CLIPPED_VALUE,
                  LG_PPO_SPO=abi.PPO_SPO, LG_PPO_THREADS=abi.PPO_THREADS, LG_PPO_MAX_BLOCKS=abi.PPO_MAX_BLOCKS,
                  LG_PPO_PARTIAL_SLOTS=abi.PPO_PARTIAL_SLOTS, LG_PPO_R_LOSS=abi.PPO_R_LOSS, LG_PPO_R_SURROGATE=abi.PPO_R_SURROGATE,
                  LG_PPO_R_VALUE=abi.PPO_R_VALUE, LG_PPO_R_ENTROPY=abi.PPO_R_ENTROPY, LG_PPO_R_KL=abi.PPO_R_KL,
                  LG_PPO_RESULT_FLOATS=abi.PPO_RESULT_FLOATS)
    lines = ["#include <stdio.h>", "#include <stddef.h>", f'#include "{HEADER}"', "int main(void){"]
    for cname, cls in structs:
        lines.append(f'printf("{cname} %zu\\n", sizeof({cname}));')
        for fname, _ in cls._fields_:
            lines.append(f'printf("{cname}.{fname} %zu\\n", offsetof({cname}, {fname}));')
    lines += [f'printf("{k} %ld\\n", (long)({k}));' for k in consts] + ["return 0;}"]
    with tempfile.TemporaryDirectory() as d:
        src, exe = os.path.join(d, "p.c"), os.path.join(d, "p")
        with open(src, "w") as f:
            f.write("\n".join(lines))
        subprocess.run(["gcc", "-o", exe, src], check=True)
        got = dict(l.split() for l in subprocess.run([exe], check=True, capture_output=True, text=True).stdout.strip().splitlines())
    for cname, cls in structs:
        assert int(got[cname]) == C.sizeof(cls), cname
        for fname, _ in cls._fields_:
            assert int(got[f"{cname}.{fname}"]) == getattr(cls, fname).offset, f"{cname}.{fname}"
    for k, v in consts.items():
        assert int(got[k]) == v, k
    assert abi.PPO_R_KL + abi.PPO_MAX_GROUPS <= abi.PPO_RESULT_FLOATS and abi.PPO_R_SURROGATE + abi.PPO_MAX_GROUPS <= abi.PPO_R_VALUE


def test_library_exports_the_ppo_entry_points():
    declared = set(re.findall(r"\b(lg_\w+)\s*\(", re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)))
    assert declared == set(abi.PPO_EXPORTS)
    lib = C.CDLL(abi.lib_path())
    for sym in declared:
        assert hasattr(lib, sym), sym
    from hcr_genesis_lr_cl_amd import build
    assert any(u[0] == "lg_ppo" and u[1] == "lg_ppo.hip" for u in build.units())
    assert f"{len(build.units())} translation units" in build.__doc__


# ---- the plan -----------------------------------------------------------------------------------------------------------------------------
def plan(rows, vrows, A):
    """(tiles, workgroups) of include/lgppo.h's launch plan, restated."""
    lanes = 1
    while lanes < (A + 3) // 4:
        lanes *= 2
    per_tile = abi.PPO_THREADS // lanes
    tiles = sum((b + per_tile - 1) // per_tile for b in rows) + (vrows + abi.PPO_THREADS - 1) // abi.PPO_THREADS
    return tiles, min(tiles, abi.PPO_MAX_BLOCKS)


@pytest.mark.parametrize("name", list(pc.CASES))
def test_workspace_of_the_table(name):
    c = pc.CASES[name]
    tiles, blocks = plan(c["rows"], c["vrows"], c["A"])
    assert ppo_loss.workspace_doubles(c["rows"], c["vrows"], c["A"]) == blocks * abi.PPO_PARTIAL_SLOTS


def test_workspace_plan_edges():
    w = ppo_loss.workspace_doubles
    assert w([1], 1, 1) == 2 * 6 and w([256], 256, 4) == 2 * 6 and w([257], 256, 4) == 3 * 6        # one lane per row at A <= 4
    assert w([64], 1, 12) == 2 * 6 and w([65], 1, 12) == 3 * 6 and w([64], 1, 16) == 2 * 6           # four lanes per row
    assert w([16], 1, 64) == 2 * 6 and w([17], 1, 64) == 3 * 6                                        # sixteen
    assert w([24576], 24576, 12) == (384 + 96) * 6                                                    # go2's mini-batch: one sweep
    assert w([10 ** 6], 10 ** 6, 12) == abi.PPO_MAX_BLOCKS * 6 and w([2 ** 31 - 1, 2 ** 31 - 1], 2 ** 31 - 1, 64) == abi.PPO_MAX_BLOCKS * 6


# ---- refusals of the entry points: nothing is enqueued (there is no device here) -----------------------------------------------------------
def _good_args(n_groups=1, kl=True, B=5, A=3):
    z = lambda *s: torch.zeros(*s)
    groups = [dict(mu=z(B, A), sigma=z(B, A), actions=z(B, A), old_log_prob=z(B, 1), advantages=z(B, 1), grad_mu=z(B, A), grad_sigma=z(B, A),
                   old_mu=z(B, A) if kl else None, old_sigma=z(B, A) if kl else None) for _ in range(n_groups)]
    keep = [groups, z(B, 1), z(B, 1), z(B, 1), z(B, 1), torch.zeros(12 * n_groups, dtype=torch.float64), z(abi.PPO_RESULT_FLOATS)]
    a = ppo_loss.ppo_loss_args(groups, *keep[1:], 0.2, 1.0, 0.01, abi.PPO_CLIPPED_VALUE)
    a._keep = keep
    return a


def _set(path, value):
    def f(a):
        obj = a
        *head, last = path
        for p in head:
            obj = obj[p] if isinstance(p, int) else getattr(obj, p)
        setattr(obj, last, value)
    return f


GROUP_MATRICES = ("mu", "sigma", "actions", "grad_mu", "grad_sigma")
ENTRY_REFUSALS = [(_set(("n_groups",), 0), b"n_groups = 0 is outside [1, 2]", True), (_set(("n_groups",), 3), b"n_groups = 3", True),
                  (_set(("n_actions",), 0), b"n_actions = 0 is outside [1, 64]", True), (_set(("n_actions",), 65), b"n_actions = 65", True),
                  (_set(("n_value_rows",), 0), b"n_value_rows < 1", True), (_set(("group", 0, "n_rows"), 0), b"group[0].n_rows < 1", True),
                  (_set(("group", 1, "n_rows"), -1), b"group[1].n_rows < 1", True),
                  (_set(("flags",), 4), b"flags has unknown bits", False), (_set(("clip_param",), 0.0), b"clip_param", False),
                  (_set(("clip_param",), float("nan")), b"clip_param", False), (_set(("value_loss_coef",), float("inf")), b"value_loss_coef", False),
                  (_set(("entropy_coef",), float("nan")), b"entropy_coef", False),
                  (_set(("group", 0, "old_mu"), None), b"group[0].old_sigma without old_mu", False),
                  (_set(("group", 1, "old_sigma"), None), b"group[1].old_mu without old_sigma", False),
                  (_set(("group", 0, "old_mu_stride"), 2), b"group[0].old_mu_stride = 2 is below the width 3", False),
                  (_set(("group", 0, "old_sigma_stride"), 0), b"group[0].old_sigma_stride = 0", False),
                  (_set(("partials",), None), b"partials is null", False), (_set(("result",), None), b"result is null", False),
                  (_set(("partials_capacity",), 17), b"partials_capacity = 17 is below the 18 doubles", False)]
ENTRY_REFUSALS += [(_set(("group", 1, k), None), f"group[1].{k} is null".encode(), False) for k in GROUP_MATRICES + ("old_log_prob", "advantages")]
ENTRY_REFUSALS += [(_set(("group", 0, k + "_stride"), 2), f"group[0].{k}_stride = 2 is below the width 3".encode(), False) for k in GROUP_MATRICES]
ENTRY_REFUSALS += [(_set(("group", 1, k + "_stride"), 0), f"group[1].{k}_stride = 0 is below the width 1".encode(), False)
                   for k in ("old_log_prob", "advantages")]
ENTRY_REFUSALS += [(_set((k,), None), f"{k} is null".encode(), False) for k in ("values", "returns", "target_values", "grad_values")]
ENTRY_REFUSALS += [(_set((k + "_stride",), 0), f"{k}_stride = 0 is below the width 1".encode(), False)
                   for k in ("values", "returns", "target_values", "grad_values")]


@pytest.mark.parametrize("i", range(len(ENTRY_REFUSALS)))
def test_entry_points_refuse_before_a_launch(i):
    change, message, in_plan = ENTRY_REFUSALS[i]
    lib = abi.load_lib()
    a = _good_args(n_groups=2)
    assert lib.lg_ppo_loss_workspace(C.byref(a)) == 3 * 6             # the descriptor is good before the change
    change(a)
    assert lib.lg_ppo_loss(C.byref(a), None) != 0
    err = lib.lg_last_error()
    assert err.startswith(b"lg_ppo_loss: ") and message in err, err
    if in_plan:
        assert lib.lg_ppo_loss_workspace(C.byref(a)) == 0 and message in lib.lg_last_error()
    else:
        assert lib.lg_ppo_loss_workspace(C.byref(a)) == 3 * 6         # the plan does not read that field


def test_entry_points_refuse_a_null_descriptor():
    lib = abi.load_lib()
    assert lib.lg_ppo_loss(None, None) != 0 and b"null descriptor" in lib.lg_last_error()
    assert lib.lg_ppo_loss_workspace(None) == 0 and b"null descriptor" in lib.lg_last_error()
    a = _good_args(n_groups=1)
    a.group[1].n_rows = 0                                             # the unused group is not read
    assert lib.lg_ppo_loss_workspace(C.byref(a)) == 2 * 6
    with pytest.raises(RuntimeError, match="n_actions = 65"):
        ppo_loss.workspace_doubles([3], 3, 65)


# ---- refusals of the Python surface: all before the library is touched ---------------------------------------------------------------------
@pytest.fixture
def no_library(monkeypatch):
    def boom():
        raise AssertionError("the library was touched")
    monkeypatch.setattr(abi, "load_lib", boom)


def test_python_refusals_name_the_tensor(no_library):
    z = lambda *s, **k: torch.zeros(*s, **k)
    B, A = 5, 3

    def build(n_groups=1, **change):
        groups = [dict(mu=z(B, A), sigma=z(B, A), actions=z(B, A), old_log_prob=z(B, 1), advantages=z(B, 1), grad_mu=z(B, A),
                       grad_sigma=z(B, A), old_mu=z(B, A), old_sigma=z(B, A)) for _ in range(n_groups)]
        rest = dict(values=z(B, 1), returns=z(B, 1), target_values=z(B, 1), grad_values=z(B, 1), partials=z(24, dtype=torch.float64),
                    result=z(8))
        for k, v in change.items():
            if k in rest:
                rest[k] = v
            else:
                groups[-1][k] = v
        return ppo_loss.ppo_loss_args(groups, rest["values"], rest["returns"], rest["target_values"], rest["grad_values"], rest["partials"],
                                      rest["result"], 0.2, 1.0, 0.0, 0)
    build()
    build(advantages=z(B), old_log_prob=z(B, 4)[:, 1:2], mu=z(B, A + 3)[:, :A], values=z(B))          # views are addressed in place
    loss_fn = ppo_loss.FusedPPOLoss()
    with pytest.raises(ValueError, match="mu is on cpu, not on a HIP device"):
        loss_fn(z(B, A), z(B, A), z(B, 1), z(B, A), z(B, 1), z(B, 1), z(B, 1), z(B, 1))
    with pytest.raises(ValueError, match="mu is on cpu"):
        loss_fn.cts(teacher=dict(mu=z(B, A)), student=dict(mu=z(B, A)), values=z(B, 1), returns=z(B, 1), target_values=z(B, 1))
    with pytest.raises(ValueError, match="student has unknown entries"):
        loss_fn.cts(teacher=dict(mu=z(B, A)), student=dict(mu=z(B, A), log_prob=z(B)), values=z(B, 1), returns=z(B, 1), target_values=z(B, 1))
    with pytest.raises(ValueError, match="clip_param"):
        ppo_loss.FusedPPOLoss(clip_param=0.0)
    for key in ("sigma", "actions", "old_mu", "old_sigma", "grad_mu", "grad_sigma"):
        with pytest.raises(ValueError, match=rf"FusedPPOLoss: {key} must be a \(5, 3\) float32.*float64"):          # dtype
            build(**{key: z(B, A, dtype=torch.float64)})
        with pytest.raises(ValueError, match=rf"FusedPPOLoss: {key} must be .*got \(4, 3\)"):                        # shape
            build(**{key: z(B - 1, A)})
        with pytest.raises(ValueError, match=rf"FusedPPOLoss: {key} must be .*unit inner stride.*strides \(6, 2\)"):  # inner stride
            build(**{key: z(B, 2 * A)[:, ::2]})
        with pytest.raises(ValueError, match=rf"FusedPPOLoss: {key} must be .* on cpu; got .* on meta"):             # device
            build(**{key: z(B, A, device="meta")})
    for key in ("old_log_prob", "advantages", "returns", "target_values", "grad_values"):
        with pytest.raises(ValueError, match=rf"FusedPPOLoss: {key} must be a \(5, 1\) or \(5,\) float32"):
            build(**{key: z(B, 1, dtype=torch.float16)})
        with pytest.raises(ValueError, match=rf"FusedPPOLoss: {key} must be"):
            build(**{key: z(B, 2)})
        with pytest.raises(ValueError, match=rf"FusedPPOLoss: {key} must be"):
            build(**{key: z(B + 1, 1)})
    with pytest.raises(ValueError, match=r"FusedPPOLoss: actions must be .*strides \(0, 1\)"):                      # rows that overlap
        build(actions=z(1, A).expand(B, A))
    with pytest.raises(ValueError, match=r"FusedPPOLoss: student.sigma must be"):
        build(n_groups=2, sigma=z(B, A + 1))
    with pytest.raises(ValueError, match="mu has 65 action columns; the kernel takes 1 .. 64"):
        build(mu=z(B, 65))
    with pytest.raises(ValueError, match="mu has no rows: an empty group"):
        build(mu=z(0, A))
    with pytest.raises(ValueError, match="student.mu has no rows: an empty group"):
        build(n_groups=2, mu=z(0, A))
    with pytest.raises(ValueError, match="values has no rows"):
        build(values=z(0, 1))
    with pytest.raises(ValueError, match="old_mu and old_sigma come together.*got old_mu alone"):
        build(old_sigma=None)
    with pytest.raises(ValueError, match="got old_sigma alone"):
        build(old_mu=None)
    with pytest.raises(ValueError, match="partials must be a contiguous float64"):
        build(partials=z(24))
    with pytest.raises(ValueError, match="result must be a contiguous float32 tensor of 8"):
        build(result=z(7))
    with pytest.raises(ValueError, match="3 policy groups"):
        ppo_loss.ppo_loss_args([{}, {}, {}], *[None] * 6, 0.2, 1.0, 0.0, 0)
    a = build(old_mu=None, old_sigma=None)
    assert a.group[0].old_mu is None and a.group[0].old_sigma is None and a.n_actions == A and a.group[0].n_rows == B


def test_descriptor_addresses_views_in_place():
    B, A = 6, 5
    slab = torch.zeros(B, 64)
    g = dict(mu=slab[:, 0:A], sigma=slab[:, 8:8 + A], actions=slab[:, 16:16 + A], old_log_prob=slab[:, 24:25], advantages=slab[:, 25],
             grad_mu=slab[:, 32:32 + A], grad_sigma=slab[:, 40:40 + A])
    v = torch.zeros(B, 4)
    a = ppo_loss.ppo_loss_args([g], v[:, 0:1], v[:, 1], v[:, 2:3], v[:, 3], torch.zeros(12, dtype=torch.float64), torch.zeros(8), 0.25, 0.5, 0.01,
                               abi.PPO_SPO)
    G = a.group[0]
    assert (G.mu, G.sigma, G.advantages, G.grad_sigma) == (slab.data_ptr(), slab.data_ptr() + 32, slab.data_ptr() + 100, slab.data_ptr() + 160)
    assert {getattr(G, k + "_stride") for k in GROUP_MATRICES + ("old_log_prob", "advantages")} == {64}
    assert (a.values_stride, a.returns_stride, a.grad_values_stride, a.returns) == (4, 4, 4, v.data_ptr() + 4)
    assert (a.n_groups, a.n_actions, a.n_value_rows, a.flags, a.clip_param, a.value_loss_coef, a.entropy_coef, a.partials_capacity) == \
        (1, A, B, abi.PPO_SPO, 0.25, 0.5, 0.01, 12)
    f = ppo_loss.FusedPPOLoss(use_clipped_value_loss=True, use_spo=True)
    assert f.flags == abi.PPO_CLIPPED_VALUE | abi.PPO_SPO and ppo_loss.FusedPPOLoss(use_clipped_value_loss=False).flags == 0


# ---- the restatement against the reference's own classes -----------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def fixture():
    return pc.load_fixture(FIXTURE)


def test_fixture_covers_what_it_should(fixture):
    cfgs = [c["cfg"] for c in fixture.values()]
    assert {(c["clipped"], c["spo"]) for c in cfgs} == {(True, False), (False, False), (True, True), (False, True)}
    assert any(c["ent"] == 0 for c in cfgs) and any(c["ent"] > 0 for c in cfgs) and len({c["value_loss_coef"] for c in cfgs}) > 1
    assert [g["mu"].shape[0] for g in fixture["cts_17_5"]["inp"]["groups"]] == [17, 5]
    for c in fixture.values():
        assert all(g["mu"].shape[0] <= 65 and g["mu"].dtype == np.float64 and g["actions"].dtype == np.float32 for g in c["inp"]["groups"])
        assert c["lr_after"][0] < 1e-3 < c["lr_after"][1] and c["lr_after"][2] == 1e-3              # falls, rises, stays


def test_restatement_reproduces_the_reference(fixture):
    """Scalars, gradients and learning rates of PPO._compute_rl_loss / PPO_CTS._compute_rl_loss in float64, to float64 round-off: this pins
    the restatement the GPU test uses, the conventions where branches meet included."""
    for name, c in fixture.items():
        got, want = pc.restate(c["inp"], dtype=torch.float64, **c["cfg"]), c["want"]
        flat = [("loss", got["loss"], want["loss"]), ("value_loss", got["value_loss"], want["value_loss"]), ("entropy", got["entropy"], want["entropy"]),
                ("grad_values", got["grad_values"], want["grad_values"])]
        for g in range(len(want["surrogate"])):
            flat += [(f"surrogate[{g}]", got["surrogate"][g], want["surrogate"][g]), (f"grad_mu[{g}]", got["grad_mu"][g], want["grad_mu"][g]),
                     (f"grad_sigma[{g}]", got["grad_sigma"][g], want["grad_sigma"][g])]
        for key, x, y in flat:
            assert x.shape == y.shape, (name, key)
            assert np.abs(x - y).max() <= 64 * np.finfo(np.float64).eps * max(1.0, np.abs(y).max()), (name, key, np.abs(x - y).max())
        assert got["kl"][0] is not None and got["kl"][0] > 0
        for desired, lr in zip(c["desired_kl"], c["lr_after"]):
            assert ppo_loss.adjust_learning_rate(got["kl"][0], 1e-3, float(desired)) == lr, (name, desired)


def test_adjust_learning_rate_rule():
    f = ppo_loss.adjust_learning_rate
    assert f(0.05, 1e-3, 0.01) == 1e-3 / 1.5 and f(0.001, 1e-3, 0.01) == 1e-3 * 1.5 and f(0.01, 1e-3, 0.01) == 1e-3
    assert f(0.02, 1e-3, 0.01) == 1e-3 and f(0.005, 1e-3, 0.01) == 1e-3                               # the bounds themselves do not move it
    assert f(0.0, 1e-3, 0.01) == 1e-3 and f(-0.1, 1e-3, 0.01) == 1e-3                                  # only a positive KL raises it
    assert f(1.0, 1.2e-5, 0.01) == 1e-5 and f(1e-9, 9e-3, 0.01) == 1e-2                                # the clamp to [1e-5, 1e-2]
    assert f(torch.tensor(0.05), 1e-3, 0.01) == 1e-3 / 1.5 and f(float("nan"), 1e-3, 0.01) == 1e-3
    assert ppo_loss.FusedPPOLoss.adjust_learning_rate is f


# ---- the table ------------------------------------------------------------------------------------------------------------------------------
def test_table_keeps_its_coverage():
    cs = pc.CASES
    single = [c for c in cs.values() if len(c["rows"]) == 1]
    assert {1, 63, 64, 65, 257, 1025} <= {c["rows"][0] for c in single}
    assert {1, 3, 4, 5, 12, 13} <= {c["A"] for c in cs.values()}
    assert {(c["clipped"], c["spo"]) for c in cs.values()} == {(True, False), (False, False), (True, True), (False, True)}
    assert any(c["ent"] == 0 for c in cs.values()) and any(c["ent"] > 0 for c in cs.values())
    assert any(all(c["kl"]) for c in cs.values()) and any(not any(c["kl"]) for c in cs.values())
    two = [c for c in cs.values() if len(c["rows"]) == 2]
    assert two and all(c["rows"][0] != c["rows"][1] for c in two) and any(1 in c["rows"] for c in two)
    assert any(c["kl"] == [True, False] for c in two)                                                 # the reference's CTS: no student KL
    big = cs[pc.LARGEST]
    tiles, blocks = plan(big["rows"], big["vrows"], big["A"])
    assert ppo_loss.workspace_doubles(big["rows"], big["vrows"], big["A"]) == blocks * abi.PPO_PARTIAL_SLOTS
    assert tiles > blocks == abi.PPO_MAX_BLOCKS                                                       # a workgroup sweeps more than once
    assert max(sum(c["rows"]) for c in cs.values()) == sum(big["rows"])


@pytest.fixture(scope="module")
def table_inputs():
    return {name: pc.make_inputs(name) for name in pc.CASES}


def test_inputs_sit_on_both_sides_of_every_branch(table_inputs):
    """In float64, for the fixed seeds: at B >= 63 between 10 % and 60 % of the rows have the ratio outside [1 - eps, 1 + eps], likewise
    |v - v_t| > eps, and no row of any case lies within 1e-4 of a boundary.  No row is excluded."""
    for name, inp in table_inputs.items():
        pc.assert_both_sides(name, inp)
    for c in pc.load_fixture(FIXTURE).values():                                                       # the fixture's rows likewise
        for g in c["inp"]["groups"]:
            r = np.exp(pc.log_prob64(g["mu"], g["sigma"], g["actions"]) - g["old_log_prob"].astype(np.float64).reshape(-1))
            assert np.minimum(np.abs(r - 0.8), np.abs(r - 1.2)).min() > 1e-4
        assert np.abs(np.abs(c["inp"]["values"] - c["inp"]["target_values"]) - 0.2).min() > 1e-4


# ---- the parity rule tells a wrong convention from a rounding ------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["b257_a12", "b257_a12_spo", "cts_17_5"])
def test_parity_rule_passes_float32_and_fails_wrong_conventions(name, table_inputs):
    """PARITY_FACTOR is derived in tests/ppo_loss_cases.py from the number formats, not from the kernel.  Here the rule is tried on what
    can be tried without one: another float32 evaluation (numpy-free torch ops in another association: the row's factors applied through
    a float64-summed log-prob, as the kernel does) passes, and two wrong conventions fail by a wide margin."""
    c, inp = pc.CASES[name], table_inputs[name]
    ref64, ref32 = pc.restate_case(name, inp), pc.restate_case(name, inp, dtype=torch.float32)
    worst = 0.0
    for (key, r64), (_, r32) in zip(pc.outputs(ref64), pc.outputs(ref32)):
        err32 = pc.max_err(r32, r64)
        assert err32 <= pc.parity_bound(err32, r64)
        worst = max(worst, err32 / max(np.abs(r64).max(), 1e-30))
    assert worst < 1e-5                                                                               # float32 against float64: rounding only
    if not c["spo"]:
        bad = pc.restate_case(name, inp, dtype=torch.float32, break_tie=True)                         # the clipped operand passes no gradient
        err = pc.max_err(bad["grad_mu"][0], ref64["grad_mu"][0])
        assert err > 100 * pc.parity_bound(pc.max_err(ref32["grad_mu"][0], ref64["grad_mu"][0]), ref64["grad_mu"][0])
    bad = pc.restate_case(name, inp, dtype=torch.float32, drop_kl_eps=True)                           # the 1e-5 inside the KL's log
    err = pc.max_err(bad["kl"][0], ref64["kl"][0])
    assert err > 10 * pc.parity_bound(pc.max_err(ref32["kl"][0], ref64["kl"][0]), ref64["kl"][0])
