"""The product library against csrc/liblgsim_strict.so, bit for bit.  The strict build runs the DPP hazard pass in strict mode (two wait states
behind a write of ANY operand of every DPP instruction, asm blocks included: LLVM's rule, which does not depend on the forwarding the product
relies on); tests/test_dpp_hazard_pass.py checks that the two differ only in s_nop.  So every buffer after every step must be identical: a
forwarded operand read stale in some lane would show up here, however far inside the oracle tolerances it stays.

Each library runs in a freshly started child process (`python -m tests.test_gpu_dpp_strict_ab --child OUT`, LG_LIB selects the library),
one after the other, under a timeout; the parent does no GPU work."""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "hcr_genesis_lr_cl_amd", "csrc")
N_ENVS = 4096
STEPS = 200
START = 480                       # as tests/test_gpu_env.py::test_fused_launch_equals_split_launches: pushes / resamples fall in the window
CHILD_TIMEOUT = 480


def configs():
    """(name, task, split launch, environment overrides, all-terms config)."""
    from hcr_genesis_lr_cl_amd.envs import TASKS
    out = [(t, t, False, {}, False) for t in TASKS]
    out += [(t + "-split", t, True, {}, False) for t in ("go2", "go2_ee", "tron1_pf_ee", "tron1_sf")]
    out += [("go2-layout1", "go2", False, {"LG_SIM_LAYOUT": "1"}, False), ("go2-slack0", "go2", False, {"LG_OBS_SLACK": "0"}, False),
            ("go2-allterms", "go2", False, {}, True)]
    # go2's single frame has no history to shift; these two run the generic tail (lg_launch_quad<4, true, PR, 0, 3>) without slack
    out += [(t + "-slack0", t, False, {"LG_OBS_SLACK": "0"}, False) for t in ("go2_wtw", "go2_ee")]
    # the whole step in one leg-per-lane launch (lg_launch_env<LEGS, LG_PHASE_ALL, 0, JPL, false>): the instantiations that spill
    out += [(t + "-layout1", t, False, {"LG_SIM_LAYOUT": "1"}, False) for t in ("go2_ee", "tron1_pf_ee", "tron1_sf")]
    return out


def _run_config(task, split, overrides, allterms, seed):
    import torch
    from hcr_genesis_lr_cl_amd import abi
    from hcr_genesis_lr_cl_amd.envs import GO2, make_env, set_seed
    saved = {k: os.environ.get(k) for k in overrides}
    os.environ.update(overrides)
    try:
        if allterms:
            from tests.test_gpu_env import _go2_all_terms_cfg
            cfg = _go2_all_terms_cfg()
            cfg.env.num_envs = N_ENVS
            set_seed(1)
            env = GO2(cfg, None, "cuda:0", True)
        else:
            env = make_env(task, N_ENVS, "cuda:0")[0]
    finally:
        for k, v in saved.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
    env.reset()
    g = torch.Generator()              # CPU: both children draw the same clocks and actions
    g.manual_seed(seed)
    env.episode_length_buf[:] = torch.randint(0, 1000, (N_ENVS,), generator=g, dtype=torch.int32).to("cuda:0")
    env.common_step_counter = START
    eng = env._engine
    names = sorted(eng.buf.keys())
    weights = {}

    def checksum(t):
        b = t.contiguous().view(-1).view(torch.uint8).to(torch.int64)
        w = weights.get(b.numel())
        if w is None:
            w = weights[b.numel()] = torch.arange(b.numel(), device=b.device, dtype=torch.int64) % 65521 + 1
        return torch.sum(b * w)

    sums, kernels = [], set()
    for t in range(STEPS):
        act = (torch.randn(N_ENVS, env.num_actions, generator=g) * (4.0 if t % 5 == 0 else 1.0)).to("cuda:0")
        if split:
            env.common_step_counter += 1
            ca = float(env.cfg.normalization.clip_actions)
            eng.step(abi.PHASE_SIM, torch.clip(act, -ca, ca), env.common_step_counter)
            kernels.add(eng.last_kernel())
            eng.step(abi.PHASE_PRE | abi.PHASE_POST | abi.PHASE_RESET, act, env.common_step_counter)
        else:
            env.step(act)
        kernels.add(eng.last_kernel())
        sums.append(torch.stack([checksum(eng.buf.raw(k)) for k in names]))
    torch.cuda.synchronize()
    final = {k: eng.buf.raw(k).contiguous().view(-1).view(torch.uint8).cpu().numpy() for k in names}
    return {"buffers": names, "checksums": torch.stack(sums).cpu().numpy(), "final": final, "kernels": sorted(kernels)}


def save(results, path):
    flat = {}
    for cfg, r in results.items():
        flat[cfg + "|buffers"] = np.array(r["buffers"])
        flat[cfg + "|checksums"] = r["checksums"]
        flat[cfg + "|kernels"] = np.array(r["kernels"])
        for k, v in r["final"].items():
            flat[cfg + "|final|" + k] = v
    np.savez(path, **flat)


def load(path):
    out = {}
    with np.load(path) as z:
        for key in z.files:
            cfg, kind, *rest = key.split("|")
            r = out.setdefault(cfg, {"final": {}})
            if kind == "final":
                r["final"][rest[0]] = z[key]
            else:
                r[kind] = [str(x) for x in z[key]] if kind in ("buffers", "kernels") else z[key]
    return out


def compare(a, b):
    """None when the two runs are bit-identical, else the first difference: configuration, step and buffer."""
    if list(a) != list(b):
        return f"configurations differ: {list(a)} vs {list(b)}"
    for cfg in a:
        ra, rb = a[cfg], b[cfg]
        if list(ra["buffers"]) != list(rb["buffers"]):
            return f"{cfg}: buffer sets differ"
        if list(ra["kernels"]) != list(rb["kernels"]):
            return f"{cfg}: kernels differ: {ra['kernels']} vs {rb['kernels']}"
        ca, cb = np.asarray(ra["checksums"]), np.asarray(rb["checksums"])
        if ca.shape != cb.shape:
            return f"{cfg}: checksum shapes differ: {ca.shape} vs {cb.shape}"
        diff = np.argwhere(ca != cb)
        if len(diff):
            step, buf = diff[0]
            return f"{cfg}: first difference at step {step} in buffer {ra['buffers'][buf]}"
        for k in ra["buffers"]:
            fa, fb = ra["final"][k], rb["final"][k]
            if fa.shape != fb.shape or not np.array_equal(fa, fb):
                return f"{cfg}: final buffer {k} differs"
    return None


def child(path):
    results = {}
    for i, (name, task, split, overrides, allterms) in enumerate(configs()):
        results[name] = _run_config(task, split, overrides, allterms, 100 + i)
        print(f"{name}: {STEPS} steps, kernels {results[name]['kernels']}", flush=True)
    save(results, path)


def test_the_comparator_finds_a_planted_one_bit_difference():
    rng = np.random.default_rng(0)
    base = {c: {"buffers": ["a", "b"], "checksums": rng.integers(0, 1 << 40, (STEPS, 2)), "kernels": ["k<1>", "k<2>"],
                "final": {"a": rng.integers(0, 256, 64, dtype=np.uint8), "b": rng.integers(0, 256, 16, dtype=np.uint8)}} for c in ("go2", "tron1_sf")}

    def copy(r):
        return {c: {"buffers": list(v["buffers"]), "checksums": v["checksums"].copy(), "kernels": list(v["kernels"]),
                    "final": {k: x.copy() for k, x in v["final"].items()}} for c, v in r.items()}
    assert compare(base, copy(base)) is None
    other = copy(base)
    other["tron1_sf"]["checksums"][37, 1] ^= 1 << 12
    other["tron1_sf"]["checksums"][90, 0] ^= 1
    assert compare(base, other) == "tron1_sf: first difference at step 37 in buffer b"
    other = copy(base)
    other["go2"]["final"]["a"][5] ^= 0x10
    assert compare(base, other) == "go2: final buffer a differs"
    other = copy(base)
    other["go2"]["kernels"] = ["k<1>"]
    assert "kernels differ" in compare(base, other)


def test_the_checksum_sees_one_bit():
    import torch
    t = torch.arange(1000, dtype=torch.float32)
    b = t.clone()
    b.view(torch.int32)[517] ^= 1
    w = torch.arange(4000, dtype=torch.int64) % 65521 + 1
    cs = lambda x: int(torch.sum(x.view(torch.uint8).to(torch.int64) * w))
    assert cs(t) != cs(b)


@pytest.mark.gpu
def test_product_equals_strict_build_bit_for_bit(tmp_path):
    strict = os.path.join(CSRC, "liblgsim_strict.so")
    assert os.path.exists(strict), "csrc/liblgsim_strict.so missing: __graft_entry__.build() builds it"
    runs = {}
    for name, lib in (("product", None), ("strict", strict)):
        env = dict(os.environ)
        env.pop("LG_LIB", None)
        if lib:
            env["LG_LIB"] = lib
        out = str(tmp_path / f"{name}.npz")
        try:
            r = subprocess.run([sys.executable, "-m", "tests.test_gpu_dpp_strict_ab", "--child", out], cwd=ROOT, env=env,
                               capture_output=True, text=True, timeout=CHILD_TIMEOUT)
        except subprocess.TimeoutExpired:
            pytest.fail(f"{name} child timed out after {CHILD_TIMEOUT} s")
        if r.returncode != 0:
            pytest.fail(f"{name} child exited with {r.returncode}:\n{r.stdout[-2000:]}\n{r.stderr[-3000:]}")
        print(f"[{name}]\n{r.stdout}")
        runs[name] = load(out)
    msg = compare(runs["product"], runs["strict"])
    assert msg is None, msg
    kernels = sorted({k for r in runs["product"].values() for k in r["kernels"]})
    print(f"bit-identical over {len(runs['product'])} configurations x {STEPS} steps; kernels: {kernels}")


if __name__ == "__main__":
    if len(sys.argv) == 3 and sys.argv[1] == "--child":
        if ROOT not in sys.path:
            sys.path.insert(0, ROOT)
        child(sys.argv[2])
    else:
        sys.exit("usage: python -m tests.test_gpu_dpp_strict_ab --child OUT.npz")
