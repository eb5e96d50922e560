"""Host side of the fused optimizer step (hcr_genesis_lr_cl_amd/optim.py, include/lgoptim.h): the ctypes mirror against the header, the
launch plan, every refusal of the entry points and of the Python surface, the float64 restatement of tests/optim_cases.py against the
golden fixture of the reference's own PPO.update() (tests/golden/ppo_update.npz) and against clip_grad_norm_ + torch.optim.Adam, the
learning-rate rule on ties, the checkpoint format, the coverage of the case table and the parity rule that tests/test_gpu_optim.py holds
the kernel to.  No GPU needed: nothing is launched."""
import ctypes as C
import math
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest
import torch

from hcr_genesis_lr_cl_amd import abi, optim, ppo_loss
from tests import optim_cases as oc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "lgoptim.h")
FIXTURE = os.path.join(ROOT, "tests", "golden", "ppo_update.npz")


# ---- the struct ---------------------------------------------------------------------------------------------------------------------------
def test_struct_layout_matches_header():
    structs = [("LgAdamTensor", abi.LgAdamTensor), ("LgAdamArgs", abi.LgAdamArgs)]
    consts = dict(LG_ADAM_MAX_TENSORS=abi.ADAM_MAX_TENSORS, LG_ADAM_CLIP=abi.ADAM_CLIP, LG_ADAM_KL_RULE=abi.ADAM_KL_RULE,
                  LG_ADAM_CHUNK=abi.ADAM_CHUNK, LG_ADAM_THREADS=abi.ADAM_THREADS, LG_ADAM_MAX_BLOCKS=abi.ADAM_MAX_BLOCKS,
                  LG_ADAM_STATE_DOUBLES=abi.ADAM_STATE_DOUBLES, LG_ADAM_S_LR=abi.ADAM_S_LR, LG_ADAM_S_STEP=abi.ADAM_S_STEP,
                  LG_ADAM_RESULT_FLOATS=abi.ADAM_RESULT_FLOATS, LG_ADAM_R_GRAD_NORM=abi.ADAM_R_GRAD_NORM,
                  LG_ADAM_R_CLIP_COEF=abi.ADAM_R_CLIP_COEF, LG_ADAM_R_LR=abi.ADAM_R_LR, LG_ADAM_R_STEP=abi.ADAM_R_STEP)
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
    assert C.sizeof(abi.LgAdamTensor) == 40 and abi.ADAM_CHUNK == 4 * abi.ADAM_THREADS and abi.ADAM_MAX_BLOCKS <= 2 * abi.ADAM_THREADS
    # the descriptor and the plan's prefix table (one 8-byte chunk end per tensor) travel by value in the 4 KB kernel-argument block
    assert C.sizeof(abi.LgAdamArgs) + 8 * abi.ADAM_MAX_TENSORS + 256 <= 4096
    assert "static_assert(sizeof(LgAdamArgs)" in open(HEADER).read()


def test_library_exports_the_optim_entry_points():
    declared = set(re.findall(r"\b(lg_\w+)\s*\(", re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)))
    assert declared == set(abi.OPTIM_EXPORTS) == {"lg_adam_step", "lg_adam_workspace"}
    lib = C.CDLL(abi.lib_path())
    for sym in declared:
        assert hasattr(lib, sym), sym
    from hcr_genesis_lr_cl_amd import build
    assert any(u[0] == "lg_optim" and u[1] == "lg_optim.hip" and any(d.endswith("lgoptim.h") for d in u[3]) for u in build.units())
    assert f"{len(build.units())} translation units" in build.__doc__
    ppo_header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "lgppo.h")).read(), flags=re.S)
    assert "lg_adam" not in ppo_header                                     # a header and a translation unit of its own


# ---- the plan -----------------------------------------------------------------------------------------------------------------------------
def plan(numels):
    """(chunks, workgroups) of include/lgoptim.h's launch plan, restated."""
    chunks = sum((n + abi.ADAM_CHUNK - 1) // abi.ADAM_CHUNK for n in numels)
    return chunks, min(chunks, abi.ADAM_MAX_BLOCKS)


PLAN_CASES = [[1], [1024], [1025], [1023, 1, 5], [1] * 64, [oc.TWO_SWEEPS]]


@pytest.mark.parametrize("numels", PLAN_CASES + [c["numels"] for c in oc.CASES.values()], ids=lambda n: f"{len(n)}x{max(n)}")
def test_workspace_against_the_restated_plan(numels):
    assert optim.workspace_doubles(numels) == plan(numels)[1]


def test_workspace_plan_edges():
    w = optim.workspace_doubles
    assert (w([1]), w([1024]), w([1025]), w([1023, 1, 5]), w([1] * 64)) == (1, 1, 2, 3, 64)
    assert plan([oc.TWO_SWEEPS]) == (513, 512) and w([oc.TWO_SWEEPS]) == 512               # two sweeps and a capped grid
    assert w([512 * 1024]) == 512 and w([2 ** 40, 2 ** 40]) == 512 and w([2 ** 62] * 64) == 512
    with pytest.raises(RuntimeError, match=r"n_tensors = 65 is outside \[1, 64\]"):
        w([1] * 65)
    with pytest.raises(RuntimeError, match=r"tensor\[1\].numel < 1"):
        w([4, 0])


# ---- refusals of the entry points: nothing is enqueued (there is no device here) -----------------------------------------------------------
def _good_args(n=3, kl=True):
    cpu = torch.device("cpu")
    params = [torch.zeros(5 + i) for i in range(n)]
    for p in params:
        p.grad = torch.zeros_like(p)
    keep = [params, [torch.zeros_like(p) for p in params], [torch.zeros_like(p) for p in params], torch.zeros(2, dtype=torch.float64),
            torch.zeros(n, dtype=torch.float64), torch.zeros(abi.ADAM_RESULT_FLOATS), torch.zeros(()) if kl else None]
    a, live = optim.adam_args(params, [f"p{i}" for i in range(n)], keep[1], keep[2], keep[3], keep[4], keep[5], keep[6], (0.9, 0.999), 1e-8,
                              1.0, 0.01 if kl else None, cpu)
    assert live == list(range(n))
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


def _clear(flag):
    def f(a):
        a.flags &= ~flag
    return f


ENTRY_REFUSALS = [(_set(("n_tensors",), 0), b"n_tensors = 0 is outside [1, 64]", True), (_set(("n_tensors",), 65), b"n_tensors = 65", True),
                  (_set(("n_tensors",), -1), b"n_tensors = -1", True),
                  (_set(("tensor", 0, "numel"), 0), b"tensor[0].numel < 1", True), (_set(("tensor", 2, "numel"), -4), b"tensor[2].numel < 1", True),
                  (_set(("flags",), 7), b"flags has unknown bits", False), (_set(("flags",), 1 << 31), b"flags has unknown bits", False),
                  (_set(("kl",), None), b"kl is null with LG_ADAM_KL_RULE", False), (_clear(abi.ADAM_KL_RULE), b"kl is set without LG_ADAM_KL_RULE", False),
                  (_set(("desired_kl",), 0.0), b"desired_kl must be a finite number above 0", False),
                  (_set(("desired_kl",), -0.01), b"desired_kl", False), (_set(("desired_kl",), float("nan")), b"desired_kl", False),
                  (_set(("max_grad_norm",), 0.0), b"max_grad_norm must be above 0", False),
                  (_set(("max_grad_norm",), float("nan")), b"max_grad_norm", False),
                  (_set(("beta1",), 1.0), b"beta1 = 1.000000 is outside [0, 1)", False), (_set(("beta1",), -0.1), b"beta1", False),
                  (_set(("beta1",), float("nan")), b"beta1", False),
                  (_set(("beta2",), 1.0), b"beta2 = 1.000000 is outside [0, 1)", False), (_set(("beta2",), -1e-9), b"beta2", False),
                  (_set(("eps",), -1e-12), b"eps is below 0", False), (_set(("eps",), float("nan")), b"eps is below 0", False),
                  (_set(("state",), None), b"state is null", False), (_set(("partials",), None), b"partials is null", False),
                  (_set(("result",), None), b"result is null", False),
                  (_set(("partials_capacity",), 2), b"partials_capacity = 2 is below the 3 doubles", False)]
ENTRY_REFUSALS += [(_set(("tensor", i, k), None), f"tensor[{i}].{k} is null".encode(), False)
                   for i, k in ((0, "param"), (1, "grad"), (2, "exp_avg"), (1, "exp_avg_sq"))]


@pytest.mark.parametrize("i", range(len(ENTRY_REFUSALS)))
def test_entry_points_refuse_before_a_launch(i):
    change, message, in_plan = ENTRY_REFUSALS[i]
    lib = abi.load_lib()
    a = _good_args()
    assert lib.lg_adam_workspace(C.byref(a)) == 3                     # the descriptor is good before the change
    change(a)
    assert lib.lg_adam_step(C.byref(a), None) != 0
    err = lib.lg_last_error()
    assert err.startswith(b"lg_adam_step: ") and message in err, err
    if in_plan:
        assert lib.lg_adam_workspace(C.byref(a)) == 0 and message in lib.lg_last_error()
    else:
        assert lib.lg_adam_workspace(C.byref(a)) == 3                 # the plan does not read that field


def test_entry_points_refuse_a_null_descriptor():
    lib = abi.load_lib()
    assert lib.lg_adam_step(None, None) != 0 and b"null descriptor" in lib.lg_last_error()
    assert lib.lg_adam_workspace(None) == 0 and b"null descriptor" in lib.lg_last_error()
    a = _good_args(n=2)
    a.tensor[2].numel = 0                                             # tensors behind n_tensors are not read
    assert lib.lg_adam_workspace(C.byref(a)) == 2
    a = _good_args(kl=False)                                          # without the rule desired_kl is not read, without the clip max_grad_norm
    a.desired_kl, a.flags, a.max_grad_norm = -1.0, 0, -1.0
    a.partials_capacity = 2
    assert lib.lg_adam_step(C.byref(a), None) != 0 and b"partials_capacity" in lib.lg_last_error()


# ---- refusals of the Python surface: all before the library is touched ---------------------------------------------------------------------
@pytest.fixture
def no_library(monkeypatch):
    def boom():
        raise AssertionError("the library was touched")
    monkeypatch.setattr(abi, "load_lib", boom)


def test_python_refusals_name_the_parameter(no_library):
    z = lambda *s, **k: torch.zeros(*s, **k)
    F = optim.FusedAdam
    with pytest.raises(ValueError, match=r"FusedAdam: params\[1\] must be float32; got \(3,\) torch.float64"):
        F([z(4), z(3, dtype=torch.float64)])
    with pytest.raises(ValueError, match=r"FusedAdam: actor.0.weight must be float32; got \(3, 2\) torch.float16"):
        F([("std", z(4)), ("actor.0.weight", z(3, 2, dtype=torch.float16))])                    # named_parameters() pairs name it
    with pytest.raises(ValueError, match=r"FusedAdam: params\[0\] must be contiguous; got \(3, 4\) .* strides \(1, 3\)"):
        F([z(4, 3).t()])
    with pytest.raises(ValueError, match=r"FusedAdam: params\[0\] is on cpu, not on a HIP device; there is no CPU path"):
        F([z(4)])
    with pytest.raises(ValueError, match=r"FusedAdam: params\[0\] is on meta, not on a HIP device"):
        F([z(4, device="meta"), z(4)])
    with pytest.raises(ValueError, match=r"FusedAdam: params\[0\] has no elements"):
        F([z(0)])
    with pytest.raises(ValueError, match="FusedAdam: no parameters"):
        F([])
    with pytest.raises(ValueError, match="FusedAdam: params\\[0\\] must be float32; got int"):
        F([3])
    for kw, msg in ((dict(lr=-1.0), "lr = -1.0"), (dict(betas=(0.9, 1.0)), "betas"), (dict(betas=(-0.1, 0.9)), "betas"), (dict(eps=-1.0), "eps"),
                    (dict(max_grad_norm=0.0), "max_grad_norm = 0.0"), (dict(desired_kl=0.0), "desired_kl = 0.0"), (dict(lr=float("nan")), "lr")):
        with pytest.raises(ValueError, match="FusedAdam: " + msg):
            F([z(4)], **kw)

    # the gradients, the KL and the work tensors: adam_args, which step() calls before it touches the library
    cpu = torch.device("cpu")

    class Loose(torch.Tensor):
        """torch itself refuses to assign a gradient of another dtype, device or layout; a custom backward hook or a hand-written
        optimizer state can still leave one, so .grad is a plain attribute here."""
        grad = None

    def args(params, grads, kl_mean=None, desired_kl=None, names=None, **change):
        params = [p.as_subclass(Loose) for p in params]
        for p, g in zip(params, grads):
            p.grad = g
        n = len(params)
        rest = dict(exp_avg=[z(*p.shape) for p in params], exp_avg_sq=[z(*p.shape) for p in params], state=z(2, dtype=torch.float64),
                    partials=z(max(n, 1), dtype=torch.float64), result=z(4))
        rest.update(change)
        return optim.adam_args(params, names or [f"w{i}" for i in range(n)], rest["exp_avg"], rest["exp_avg_sq"], rest["state"], rest["partials"],
                               rest["result"], kl_mean, (0.9, 0.999), 1e-8, 1.0, desired_kl, cpu)
    a, live = args([z(4), z(2, 3)], [z(4), z(2, 3)])
    assert live == [0, 1] and a.n_tensors == 2 and a.flags == abi.ADAM_CLIP and a.tensor[1].numel == 6 and a.kl is None
    a, live = args([z(4), z(2, 3), z(5)], [z(4), None, z(5)])                                    # a None gradient is left out
    assert live == [0, 2] and a.n_tensors == 2 and a.tensor[1].numel == 5
    a, live = args([z(4)], [None])
    assert live == [] and a.n_tensors == 0
    with pytest.raises(ValueError, match="more than 64 parameter tensors"):
        args([z(1) for _ in range(65)], [z(1) for _ in range(65)])
    with pytest.raises(ValueError, match=r"FusedAdam: w1.grad must be a dense float32 tensor; got \(2, 3\) torch.float64"):
        args([z(4), z(2, 3)], [z(4), z(2, 3, dtype=torch.float64)])
    with pytest.raises(ValueError, match=r"FusedAdam: w0.grad must be contiguous; got \(2, 3\) .* strides \(1, 2\)"):
        args([z(2, 3)], [z(3, 2).t()])
    with pytest.raises(ValueError, match=r"FusedAdam: w0.grad must be on cpu; got \(4,\) torch.float32 on meta"):
        args([z(4)], [z(4, device="meta")])
    with pytest.raises(ValueError, match=r"FusedAdam: w0.grad must be a dense float32 tensor; .*layout torch.sparse_coo"):
        args([z(4)], [torch.sparse_coo_tensor([[1]], [1.0], (4,))])
    with pytest.raises(ValueError, match="kl_mean was given, but the optimizer has no desired_kl"):
        args([z(4)], [z(4)], kl_mean=z(()))
    with pytest.raises(ValueError, match=r"kl_mean must be a 0-dim float32 tensor on cpu; got \(\) torch.float64"):
        args([z(4)], [z(4)], kl_mean=z((), dtype=torch.float64), desired_kl=0.01)
    with pytest.raises(ValueError, match="kl_mean must be a 0-dim float32 tensor on cpu; got float"):
        args([z(4)], [z(4)], kl_mean=0.01, desired_kl=0.01)
    with pytest.raises(ValueError, match=r"kl_mean must be .*got \(2,\)"):
        args([z(4)], [z(4)], kl_mean=z(2), desired_kl=0.01)
    with pytest.raises(ValueError, match="state must be a contiguous float64 tensor of at least 2"):
        args([z(4)], [z(4)], state=z(2))
    with pytest.raises(ValueError, match="partials must be a contiguous float64"):
        args([z(4)], [z(4)], partials=z(1))
    with pytest.raises(ValueError, match="result must be a contiguous float32 tensor of at least 4"):
        args([z(4)], [z(4)], result=z(3))
    with pytest.raises(ValueError, match=r"w0's exp_avg_sq must have 4 elements"):
        args([z(4)], [z(4)], exp_avg_sq=[z(5)])
    a, _ = args([z(4)], [z(4)], kl_mean=z(8)[5], desired_kl=0.02)                                # an element of a result vector, in place
    assert a.flags == abi.ADAM_CLIP | abi.ADAM_KL_RULE and a.desired_kl == 0.02 and a.kl == a.kl // 4 * 4


def test_more_than_64_parameters_are_refused_before_the_library(no_library, monkeypatch):
    """check_parameters asks for the device before it counts, and there is no HIP device here: the count is shown on tensors whose device
    type reads as a HIP device's."""
    class OnDevice(torch.Tensor):
        @property
        def device(self):
            return torch.device("cuda", 0)
    ps = [torch.zeros(2).as_subclass(OnDevice) for _ in range(65)]
    with pytest.raises(ValueError, match=r"FusedAdam: 65 parameter tensors; the kernel takes 1 .. 64"):
        optim.FusedAdam(ps)
    assert len(optim.check_parameters(ps[:64])[0]) == 64


def test_descriptor_addresses_views_in_place():
    slab = torch.zeros(64)
    p = slab[1:13]                                                    # a 12-float std at a 1-float offset
    p.grad = torch.zeros(16)[3:15]
    m, v = torch.zeros(13)[1:], torch.zeros(14)[2:]
    a, live = optim.adam_args([p], ["std"], [m], [v], torch.zeros(2, dtype=torch.float64), torch.zeros(1, dtype=torch.float64), torch.zeros(4), None,
                              (0.8, 0.9), 1e-5, None, None, torch.device("cpu"))
    T = a.tensor[0]
    assert (T.param, T.grad, T.numel) == (slab.data_ptr() + 4, p.grad.data_ptr(), 12) and T.exp_avg == m.data_ptr() and T.exp_avg_sq == v.data_ptr()
    assert (a.flags, a.beta1, a.beta2, a.eps, a.max_grad_norm, a.desired_kl, a.partials_capacity) == (0, 0.8, 0.9, 1e-5, 0.0, 0.0, 1)


# ---- the restatement against the reference --------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def fixture():
    return oc.load_fixture(FIXTURE)


def test_fixture_covers_what_it_should(fixture):
    cfg = fixture["cfg"]
    assert cfg["steps"] == 6 == len(fixture["grads"]) == len(fixture["params"]) == len(fixture["kl"]) == len(fixture["lr"])
    assert len(fixture["names"]) == 13 and sorted(fixture["shapes"])[-1] == (16, 7) and (3,) in fixture["shapes"]
    clipped = fixture["grad_norm"] > cfg["max_grad_norm"]
    assert clipped.any() and not clipped.all()                                                   # some steps clip and some do not
    moves = np.array(fixture["lr"]) / np.array([cfg["lr0"]] + list(fixture["lr"][:-1]))
    assert (moves > 1).any() and (moves < 1).any() and (moves == 1).any()                        # the rate rises, falls and stays
    for k in fixture["kl"]:                                                                      # float32 rounding moves no decision
        assert k > 0 and abs(k / (2 * cfg["desired_kl"]) - 1) > 0.01 and abs(k / (cfg["desired_kl"] / 2) - 1) > 0.01
    assert os.path.getsize(FIXTURE) < 100 * 1024


def test_restatement_reproduces_the_reference(fixture):
    """The parameters after each of the six steps of the reference's own PPO.update(), to 1e-12: the learning-rate sequence from the
    fixture's KLs exactly, the total norms to float64 round-off.  This pins the restatement that the GPU test holds the kernel to."""
    cfg = fixture["cfg"]
    got = oc.restate(fixture["init"], fixture["grads"], lr0=cfg["lr0"], kls=list(fixture["kl"]), betas=cfg["betas"], eps=cfg["eps"],
                     max_grad_norm=cfg["max_grad_norm"], desired_kl=cfg["desired_kl"], dtype=torch.float64)
    for s, step in enumerate(got):
        assert step["lr"] == fixture["lr"][s], s
        assert abs(step["grad_norm"] - fixture["grad_norm"][s]) <= 1e-14 * fixture["grad_norm"][s], s
        assert (step["clip_coef"] < 1.0) == (fixture["grad_norm"][s] > cfg["max_grad_norm"]), s
        for name, x, y in zip(fixture["names"], step["params"], fixture["params"][s]):
            assert np.abs(x - y).max() <= 1e-12, (s, name, np.abs(x - y).max())
    assert got[-1]["step"] == 6 and max(np.abs(x - y).max() for x, y in zip(got[-1]["params"], fixture["init"])) > 1e-3


@pytest.mark.parametrize("name", list(oc.CASES))
def test_restatement_agrees_with_torch_adam_on_the_table(name):
    """restate(float64) against clip_grad_norm_ + torch.optim.Adam in float64, at every gradient scale; and each scale does what it is
    named for: the total norm never, sometimes and always above max_grad_norm."""
    h = oc.hyper(name)
    for label, scale in oc.SCALES.items():
        params, grads = oc.make_inputs(name, scale)
        got = oc.restate(params, grads, lr0=h["lr"], betas=h["betas"], eps=h["eps"], max_grad_norm=h["max_grad_norm"])
        want = oc.torch_reference(params, grads, lr=h["lr"], betas=h["betas"], eps=h["eps"], max_grad_norm=h["max_grad_norm"])
        clipped = [s["grad_norm"] > h["max_grad_norm"] for s in got]
        assert all(abs(s["grad_norm"] / h["max_grad_norm"] - 1.0) > 0.05 for s in got)
        if label == "never":
            assert not any(clipped) and all(s["clip_coef"] == 1.0 for s in got)
        elif label == "always":
            assert all(clipped) and all(s["clip_coef"] < 0.1 for s in got)
        elif len(got) > 1:
            assert any(clipped) and not all(clipped)
        for s, (a, b) in enumerate(zip(got, want)):
            assert abs(a["grad_norm"] - b["grad_norm"]) <= 1e-14 * b["grad_norm"]
            for field in oc.FIELDS:
                for x, y in zip(a[field], b[field]):
                    assert np.abs(x - y).max() <= 1e-12 * max(1.0, np.abs(y).max()), (name, label, s, field, np.abs(x - y).max())


def test_restatement_leaves_a_tensor_without_gradient_alone():
    params, grads = oc.make_inputs("tiny_actor", 1.0)
    for g in grads:
        g[2] = None
    with_none = oc.restate(params, grads)
    without = oc.restate(params[:2] + params[3:], [g[:2] + g[3:] for g in grads])
    assert np.array_equal(with_none[-1]["params"][2], params[2].astype(np.float64)) and not with_none[-1]["exp_avg"][2].any()
    for field in oc.FIELDS:
        for x, y in zip(with_none[-1][field][:2] + with_none[-1][field][3:], without[-1][field]):
            assert np.array_equal(x, y)
    nothing = oc.restate(params, [[None] * len(params)])
    assert nothing[0]["step"] == 0


# ---- the learning-rate rule -------------------------------------------------------------------------------------------------------------------
def test_rate_rule_on_ties_is_the_host_rule_bit_for_bit():
    table = oc.tie_table()
    mine, host = oc.tie_expected(oc.adjust_rate), oc.tie_expected(ppo_loss.adjust_learning_rate)
    assert [np.float64(x).tobytes() for x in mine] == [np.float64(x).tobytes() for x in host]
    d = oc.TIE_DESIRED_KL
    kls = [float(k) for k, _ in table]
    assert kls[0] == 2 * d and kls[1] == d / 2 and mine[0] == mine[1] == 1e-3                    # the thresholds themselves: it stays
    assert kls[2] > 2 * d > kls[3] and mine[2] == 1e-3 / 1.5 and mine[3] == 1e-3                 # their float32 neighbours on either side
    assert kls[4] > d / 2 > kls[5] and mine[4] == 1e-3 and mine[5] == 1e-3 * 1.5
    assert kls[6] == 0.0 and kls[7] == -1.0 and math.isnan(kls[8]) and mine[6:9] == [1e-3] * 3   # 0, -1 and NaN stay
    assert mine[9:13] == [5e-3 * 1.5, 1e-2, 1e-2, 1e-2] and mine[13:17] == [2e-5 / 1.5, 1e-5, 1e-5, 1e-5]
    assert len(table) == 17


# ---- checkpoints ------------------------------------------------------------------------------------------------------------------------------
def test_torch_adam_state_dict_is_what_load_state_dict_accepts():
    """Format only, no device: the keys and shapes of a torch.optim.Adam after 3 CPU steps pass check_state_dict; differing step counts,
    another number of parameters, a second group, a wrong shape and weight decay are refused."""
    ps = [torch.nn.Parameter(torch.randn(3, 2)), torch.nn.Parameter(torch.randn(5)), torch.nn.Parameter(torch.randn(1))]
    adam = torch.optim.Adam(ps, lr=2e-3, betas=(0.8, 0.9), eps=1e-6)
    names = ["a", "b", "c"]
    assert optim.check_state_dict(adam.state_dict(), ps, names) == (0.0, {})                     # before the first step torch keeps no state
    for _ in range(3):
        for p in ps:
            p.grad = torch.randn_like(p)
        adam.step()
    sd = adam.state_dict()
    assert set(sd) == {"state", "param_groups"} and set(sd["state"][0]) == {"step", "exp_avg", "exp_avg_sq"}
    assert set(optim._TORCH_GROUP_DEFAULTS) | {"lr", "betas", "eps", "params"} == set(sd["param_groups"][0])
    assert {k: sd["param_groups"][0][k] for k in optim._TORCH_GROUP_DEFAULTS} == optim._TORCH_GROUP_DEFAULTS
    step, moments = optim.check_state_dict(sd, ps, names)
    assert step == 3.0 and sorted(moments) == [0, 1, 2] and moments[0][0].shape == (3, 2) and moments[1][1].shape == (5,)
    import copy
    bad = copy.deepcopy(sd)
    bad["state"][1]["step"] = torch.tensor(2.0)
    with pytest.raises(ValueError, match=r"step counts differ \(a: 3, b: 2, c: 3\)"):
        optim.check_state_dict(bad, ps, names)
    with pytest.raises(ValueError, match="covers 3 parameters, the optimizer 2"):
        optim.check_state_dict(sd, ps[:2], names[:2])
    bad = copy.deepcopy(sd)
    bad["param_groups"].append(dict(bad["param_groups"][0]))
    with pytest.raises(ValueError, match="2 parameter groups"):
        optim.check_state_dict(bad, ps, names)
    bad = copy.deepcopy(sd)
    bad["state"][2]["exp_avg"] = torch.zeros(2)
    with pytest.raises(ValueError, match=r"exp_avg of c has shape \(2,\), the parameter \(1,\)"):
        optim.check_state_dict(bad, ps, names)
    bad = copy.deepcopy(sd)
    bad["param_groups"][0]["weight_decay"] = 0.01
    with pytest.raises(ValueError, match="weight_decay = 0.01"):
        optim.check_state_dict(bad, ps, names)
    bad = copy.deepcopy(sd)
    del bad["state"][1]                                                                          # a parameter that never had a gradient
    assert sorted(optim.check_state_dict(bad, ps, names)[1]) == [0, 2]


# ---- the table and the parity rule ------------------------------------------------------------------------------------------------------------
def test_table_keeps_its_coverage():
    cs = oc.CASES
    single = {c["numels"][0] for c in cs.values() if len(c["numels"]) == 1}
    assert {1, 3, 4, 5, 1023, 1024, 1025, oc.TWO_SWEEPS} <= single
    assert cs["tiny_actor"]["numels"] == [112, 16, 128, 8, 12] and cs["view_off1"].get("view") and cs["view_off1"]["numels"][0] > abi.ADAM_CHUNK
    ragged = cs["t64_ragged"]["numels"]
    assert len(ragged) == abi.ADAM_MAX_TENSORS and len(set(ragged)) > 32 and min(ragged) >= 1 and max(ragged) > abi.ADAM_CHUNK
    assert any(n % abi.ADAM_CHUNK for n in ragged) and any(n % 4 for n in ragged)
    assert cs["two_sweeps"]["steps"] == (1,) and plan(cs["two_sweeps"]["numels"]) == (513, 512)
    assert oc.hyper("other_hyper") == dict(betas=(0.8, 0.9), eps=1e-5, max_grad_norm=0.5, lr=1e-3)
    assert all(oc.hyper(n) == oc.DEFAULTS for n in cs if n != "other_hyper")
    assert oc.SCALES == {"never": 0.01, "mixed": 1.0, "always": 30.0} and oc.STEPS == (1, 5) and oc.PARITY_FACTOR <= 8.0


@pytest.mark.parametrize("name", ["tiny_actor", "n1025", "other_hyper"])
def test_parity_rule_passes_float32_and_fails_wrong_conventions(name):
    """PARITY_FACTOR is derived in tests/optim_cases.py from the number formats, not from the kernel.  Here the rule is tried on what can be
    tried without one: the float32 restatement is rounding only, and two wrong conventions -- no bias correction, a clip per tensor instead
    of the global one -- fail by a wide margin."""
    h = oc.hyper(name)
    kw = dict(lr0=h["lr"], betas=h["betas"], eps=h["eps"], max_grad_norm=h["max_grad_norm"])
    params, grads = oc.make_inputs(name, 1.0)
    ref64, ref32 = oc.restate(params, grads, **kw)[-1], oc.restate(params, grads, dtype=torch.float32, **kw)[-1]
    assert oc.check_parity(ref32, ref64, ref32, name + " f32") <= 1.0
    for wrong in ("no_bias_correction",) + (("clip_per_tensor",) if len(params) > 1 else ()):
        bad = oc.restate(params, grads, dtype=torch.float32, wrong=wrong, **kw)[-1]
        with pytest.raises(AssertionError, match="above"):
            oc.check_parity(bad, ref64, ref32, name + " " + wrong)
        err = max(oc.max_err(x, y) for x, y in zip(bad["params"], ref64["params"]))
        assert err > 100 * max(oc.parity_bound(oc.max_err(x, y), y) for x, y in zip(ref32["params"], ref64["params"]))
