"""Developer tool (GPU only, never read by bench.py): time of one update's worth of feed-forward mini-batches -- 4 mini-batches x 5 epochs
at N = 4096 envs, T = 24 steps -- produced by the gather kernel (one `lg_rollout_gather` launch per mini-batch) against the same tuples
from torch index ops on the same storage (one gather launch per tensor: `x.flatten(0, 1)[idx]`, and `1.0 - dones[idx]` for the
terminated flags), which is how the mini-batches were produced before the kernel existed.  Two layouts:

  * base: RolloutStorage with go2's widths (45 observations, 61 critic observations, 12 actions), 9 tensors per mini-batch;
  * ee:   RolloutStorageEE with go2_ee's widths (900 estimator features, 24 labels, 870 critic observations, 12 actions), 11 tensors.

Each pass runs the whole generator, drops every batch as it comes and ends in a device synchronise; it is timed on the host clock.  The
two sides alternate in one process after a warm-up; medians and the spread over the repeats are printed.  Both sides draw the same
permutation (the generator's torch.randperm under one seed) and their outputs are compared before anything is timed.  Bytes are
computed from the shapes: every gathered row is read once and written once, plus 8 bytes of index per row and index set.

    python tools/mini_batch_gather_time.py [--repeats 30] [--envs 4096] [--steps 24]

Prints a table and one JSON line."""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import torch  # noqa: E402

HBM_ACHIEVABLE = 6.3e12          # bytes/s, MI355X_MICROARCH.md


def torch_pass(st, names, num_mini_batches, num_epochs):
    """The feed-forward generators' tuples from torch index ops: `names` in the tuple's order, "dones" standing for 1 - dones."""
    flat = {k: (st.privileged_observations if k == "critic" else getattr(st, k)).flatten(0, 1) for k in set(names)}
    per = st.num_envs * st.num_transitions_per_env // num_mini_batches
    blocks = torch.randperm(num_mini_batches * per, device=st.device).view(num_mini_batches, per)
    for _ in range(num_epochs):
        for b in blocks:
            yield (*((1.0 - flat[k][b]) if k == "dones" else flat[k][b] for k in names), (None, None), None)


def same(x, y):
    if isinstance(x, (list, tuple)):
        return len(x) == len(y) and all(same(p, q) for p, q in zip(x, y))
    if x is None or y is None:
        return x is y
    return x.shape == y.shape and x.dtype == y.dtype and torch.equal(x, y)


def fill(st, gen):
    for k, x in vars(st).items():
        if torch.is_tensor(x) and x.dtype == torch.float32 and x.dim() == 3:
            x.copy_(torch.randn(x.shape, generator=gen, device=x.device))
    st.dones.copy_((torch.rand(st.dones.shape, generator=gen, device=st.device) < 0.02).to(torch.uint8))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--steps", type=int, default=24)
    ap.add_argument("--mini-batches", type=int, default=4)
    ap.add_argument("--epochs", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("mini_batch_gather_time.py: no GPU -- a time is only measured on the device")
    from hcr_genesis_lr_cl_amd import build as b
    from hcr_genesis_lr_cl_amd.rollout import RolloutStorage, RolloutStorageEE
    N, T, nmb, epochs, dev = args.envs, args.steps, args.mini_batches, args.epochs, "cuda:0"
    gen = torch.Generator(device=dev)
    gen.manual_seed(1)
    ppo = ("actions", "values", "advantages", "returns", "actions_log_prob", "mu", "sigma")
    layouts = {"base": (RolloutStorage(N, T, [45], [61], [12], dev), ("observations", "critic") + ppo),
               "ee": (RolloutStorageEE(N, T, [870], [900], [24], [12], dev), ("critic", "estimator_features", "estimator_labels", "dones") + ppo)}
    res = dict(tool="mini_batch_gather_time", envs=N, steps=T, mini_batches=nmb, epochs=epochs, repeats=args.repeats, layouts={},
               hbm_achievable_bytes_per_s=HBM_ACHIEVABLE, source_hash=b.source_hash(), device=torch.cuda.get_device_name(0))
    for name, (st, names) in layouts.items():
        fill(st, gen)
        sides = {"kernel": lambda st=st: st.mini_batch_generator(nmb, epochs), "torch": lambda st=st, names=names: torch_pass(st, names, nmb, epochs)}
        got = {}
        for k, f in sides.items():
            torch.manual_seed(7)                                        # the same permutation on both sides
            got[k] = [tuple(batch) for batch in f()]
        torch.cuda.synchronize()
        if not same(got["kernel"], got["torch"]):
            sys.exit(f"mini_batch_gather_time.py: {name}: the two sides disagree -- nothing timed")
        del got

        def one_pass(f):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for batch in f():
                pass
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) * 1e6

        for _ in range(args.warmup):
            for f in sides.values():
                one_pass(f)
        times = {k: [] for k in sides}
        for _ in range(args.repeats):
            for k, f in sides.items():
                times[k].append(one_pass(f))
        per = N * T // nmb
        floats = sum(1 if k == "dones" else (st.privileged_observations if k == "critic" else getattr(st, k)).shape[2] for k in names)
        moved = nmb * epochs * per * (2 * 4 * floats - (3 if "dones" in names else 0) + 8)           # dones are read as one byte
        stat = lambda v: dict(median=statistics.median(v), min=min(v), max=max(v), p10=sorted(v)[len(v) // 10], p90=sorted(v)[(9 * len(v)) // 10])
        launches = {"kernel": nmb * epochs, "torch": nmb * epochs * (len(names) + ("dones" in names))}
        out = dict(tensors=len(names), floats_per_row=floats, rows_per_mini_batch=per, bytes_moved=moved, launches=launches,
                   pass_us={k: stat(v) for k, v in times.items()})
        out["kernel_bytes_per_s"] = moved / (out["pass_us"]["kernel"]["median"] * 1e-6)
        res["layouts"][name] = out
        print(f"{name}: {len(names)} tensors, {floats} floats per row, {per} rows per mini-batch, {nmb} x {epochs} mini-batches, {moved / 1e6:.1f} MB moved per pass")
        for k, v in out["pass_us"].items():
            print(f"  {k:6s} ({launches[k]:3d} gather launches): median {v['median']:9.1f} us   min {v['min']:9.1f}   p10-p90 {v['p10']:9.1f} - {v['p90']:9.1f}"
                  f"   max {v['max']:9.1f}")
        print(f"  kernel pass: {out['kernel_bytes_per_s'] / 1e12:.2f} TB/s over the whole pass (allocations and launch gaps included) of "
              f"{HBM_ACHIEVABLE / 1e12:.1f} TB/s achievable")
        del st
    print(json.dumps(res))


if __name__ == "__main__":
    main()
