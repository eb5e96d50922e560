"""Golden vectors for the storages of the explicit-estimator, teacher-student, concurrent teacher-student and DreamWaQ learners, from
the reference's own classes (rsl_rl/storage/rollout_storage_ee.py, _ts.py, _cts.py, _dreamwaq.py) on the CPU at N = 12 envs, T = 5
steps, 5 teacher envs, every tensor with a width of its own (tests/rollout_algos_harness.py).

Build-container only:   PYTHONDONTWRITEBYTECODE=1 python tests/golden/gen_rollout_algos_fixtures.py
Output: tests/golden/rollout_algos.npz.  Per class <C> in EE, TS, CTS, DreamWaQ:

  * <C>_in_<attribute>  (T, N, w): what each step's Transition carried, seeded; column 0 of every row wider than the one-column policy
    outputs is the tag of tensor and sample (rollout_algos_harness.tag_base + t * N + e); rewards, dones, values and log-probs are data;
  * <C>_last_values, gamma, lam: the arguments of compute_returns;
  * <C>_st_<tensor>: every stored tensor after T add_transitions and compute_returns (CTS: teacher_ / student_advantages too);
  * <C>_layout_names / _widths / _dtypes / _rows / _sets: the tuple mini_batch_generator(3, 2) yields, read off the tags after the
    one-column tensors (values, log-probs, returns, advantages) were tagged as well: for each position the stored tensor it came from,
    its width, dtype, row count and the index set it shares with others ("dones": the float32 1 - dones entry);
  * <C>_terminated, <C>_terminated_dones: that entry of every yield, and the stored dones at the sample ids of the same yield.

Data only: arrays and lists of names.  Written through ref_harness.save; `python tests/golden/check_fixtures.py` checks that the
output still equals the committed file."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import ref_harness as rh  # noqa: E402
from tests import rollout_algos_harness as ah  # noqa: E402

rh.load_reference()
import torch  # noqa: E402


def reference_classes():
    from rsl_rl.storage.rollout_storage_cts import RolloutStorageCTS
    from rsl_rl.storage.rollout_storage_dreamwaq import RolloutStorageDreamWaQ
    from rsl_rl.storage.rollout_storage_ee import RolloutStorageEE
    from rsl_rl.storage.rollout_storage_ts import RolloutStorageTS
    return {"EE": RolloutStorageEE, "TS": RolloutStorageTS, "CTS": RolloutStorageCTS, "DreamWaQ": RolloutStorageDreamWaQ}


def inputs(cls, rng):
    """Per Transition attribute a (T, N, w) array (rewards, dones, actions_log_prob: (T, N))."""
    T, N = ah.T, ah.N
    out = {}
    for attr, stored in ah.ROWS[cls] + ah.POLICY_ROWS:
        w = ah.width_of(stored)
        x = rng.normal(size=(T, N, w)).astype(np.float32)
        if stored not in ah.COMPUTED:
            x[..., 0] = ah.tag_base(stored, T, N) + ah.tag_ids(T, N)
        out[attr] = x[..., 0] if attr == "actions_log_prob" else x
    out["rewards"] = (0.02 + 0.05 * rng.normal(size=(T, N)) + 0.3 * np.sin(np.arange(N))[None, :]).astype(np.float32)
    out["dones"] = rng.random((T, N)) < 0.3
    return out


def one_class(cls, ref, seed):
    T, N, nt = ah.T, ah.N, ah.NUM_TEACHER
    rng = np.random.default_rng(seed)
    st = ref(*ah.ctor_args(cls, N, T, nt), device="cpu")
    x = inputs(cls, rng)
    for t in range(T):
        tr = ref.Transition()
        for attr, v in x.items():
            setattr(tr, attr, torch.from_numpy(v[t]))
        st.add_transitions(tr)
    last_values = rng.normal(size=(N, 1)).astype(np.float32)
    st.compute_returns(torch.from_numpy(last_values), ah.GAMMA, ah.LAM)
    arrays = {f"{cls}_in_{k}": v for k, v in x.items()}
    arrays[f"{cls}_last_values"] = last_values
    stored = [n for n in ah.TAGGED + ("rewards", "dones") if torch.is_tensor(getattr(st, n, None))]
    for n in stored:
        arrays[f"{cls}_st_{n}"] = getattr(st, n).numpy().copy()
    # the one-column tensors get their tags now; the groups' advantages are tagged with the sample ids of their own envs
    for n in ah.COMPUTED:
        if n in stored:
            first, group = {"teacher_advantages": (0, nt), "student_advantages": (nt, N - nt)}.get(n, (0, N))
            getattr(st, n)[..., 0] = torch.from_numpy(ah.tag_base(n, T, N) + ah.tag_ids(T, N, first, group))
    dones = st.dones.numpy().reshape(T * N)
    torch.manual_seed(seed)
    layout, terminated, terminated_dones = None, [], []
    for batch in st.mini_batch_generator(3, 2):
        assert batch[-2] == (None, None) and batch[-1] is None
        names, widths, dtypes, rows, sets, ids_of_set = [], [], [], [], [], []
        for item in batch[:-2]:
            a = item.numpy()
            name, ids = ah.decode(a[:, 0], T, N)
            if ids is not None:
                key = ids.tolist()
                if key not in ids_of_set:
                    ids_of_set.append(key)
                sets.append(ids_of_set.index(key))
            else:
                sets.append(-1)
            names.append(name); widths.append(a.shape[1]); dtypes.append(str(a.dtype)); rows.append(a.shape[0])
        for i, name in enumerate(names):
            if name == "dones":                                   # 1 - dones: untagged, so matched to the one set with its row count
                match = [k for k, ids in enumerate(ids_of_set) if len(ids) == rows[i]]
                assert len(match) == 1
                sets[i] = match[0]
                got, want = batch[i].numpy()[:, 0], dones[np.asarray(ids_of_set[match[0]])]
                assert np.array_equal(got, 1.0 - want.astype(np.float32))
                terminated.append(got); terminated_dones.append(want)
        this = (names, widths, dtypes, rows, sets)
        assert layout is None or layout == this, "the tuple layout changed between yields"
        layout = this
    for k, v in zip(("names", "widths", "dtypes", "rows", "sets"), layout):
        arrays[f"{cls}_layout_{k}"] = np.array(v)
    if terminated:
        arrays[f"{cls}_terminated"], arrays[f"{cls}_terminated_dones"] = np.stack(terminated), np.stack(terminated_dones)
    return arrays, layout


def main(seed=11):
    arrays = dict(gamma=np.float32(ah.GAMMA), lam=np.float32(ah.LAM), num_envs=np.int64(ah.N), num_steps=np.int64(ah.T),
                  num_teacher=np.int64(ah.NUM_TEACHER))
    info = []
    for i, (cls, ref) in enumerate(reference_classes().items()):
        a, layout = one_class(cls, ref, seed + i)
        arrays.update(a)
        info += [cls, len(layout[0]) + 2, sorted(set(layout[3]))]
    rh.save("rollout_algos", arrays, *info)


if __name__ == "__main__":
    main()
