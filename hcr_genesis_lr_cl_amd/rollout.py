"""RolloutStorage with the per-step record and the return computation as HIP kernels.

Mirrors the reference's rsl_rl/storage/rollout_storage.py: same constructor, same tensors under the same names and shapes
((T, N, width) float32; dones (T, N, 1) uint8), `add_transitions`, `clear`, `compute_returns`, `get_statistics`,
`mini_batch_generator`, `reccurent_mini_batch_generator` -- so rsl_rl's PPO takes it in place of its own, with a feed-forward ActorCritic
or with ActorCriticRecurrent (LSTM / GRU: hidden states are stored per step under the reference's names).  What changes is how the rows
are filled and how the recurrent mini-batches are cut:

  * `record(t-less API: add_step)`: reward (with the time-out bootstrap of rsl_rl/algorithms/ppo.py:106-113), done flag and any
    observation rows in ONE launch (`lg_rollout_record`) instead of nine `copy_` launches (rollout_storage.py:92-100);
  * `compute_returns`: GAE over the whole rollout plus the advantage normalisation in two launches (`lg_rollout_gae`) instead
    of a 24-iteration Python loop of elementwise ops (rollout_storage.py:124-138);
  * with `attach_env(env)` on a task with unstacked observations the storage's observation rows ARE the env's observation
    copies (LgTaskCfg.obs_sets = T + 1): step() writes each observation straight into its row and nothing is copied;
  * `reccurent_mini_batch_generator`: the trajectory split of rsl_rl/utils/utils.py:33-65 (every length to the host, one tensor per
    trajectory, pad_sequence) and the per-mini-batch sum / boolean gather of rollout_storage.py:203-228 become one index launch
    (`lg_rollout_traj_index`), one small read-back and one launch (`lg_rollout_pad`) that writes the padded observations, the masks and
    the start hidden states of every trajectory; `unpad_trajectories` is the inverse (`lg_rollout_mask_index` + `lg_rollout_unpad`);
  * `mini_batch_generator`: the nine index gathers per mini-batch of rollout_storage.py:170-186 are ONE launch (`lg_rollout_gather`) that
    writes every tensor of the mini-batch, indexed by the int64 permutation as torch.randperm gives it.

`RolloutStorageEE`, `RolloutStorageTS`, `RolloutStorageCTS` and `RolloutStorageDreamWaQ` mirror the storages that the reference's PPO_EE,
PPO_TS, PPO_CTS and PPO_DreamWaQ build (rsl_rl/storage/rollout_storage_ee.py, _ts.py, _cts.py, _dreamwaq.py): the reference's constructor
arguments in its order, its tensors and Transition attributes, and generators that yield its tuples of 13 / 14 / 18 / 15 entries -- each
from one gather launch, `terminated = 1 - dones` formed by the kernel, CTS's teacher and student halves read in place from the
(T, N, width) rows through an env window and its three index sets served together.  Their env-side rows go out with reward and done in the
one record launch, through `add_transitions` or through `add_step` with the rows as keywords; CTS computes its returns and the two
separately normalised advantage tensors with `lg_rollout_gae_groups`.

There is no CPU path: the kernels live in csrc/liblgsim.so (include/lgrollout.h)."""
from __future__ import annotations

import ctypes as C

import torch

from . import abi

_F32, _NOT = abi.GATHER_F32, abi.GATHER_NOT_U8
_PPO_BATCH = (("actions", _F32), ("values", _F32), ("advantages", _F32), ("returns", _F32), ("actions_log_prob", _F32), ("mu", _F32), ("sigma", _F32))


def _call(dev, name, *args):
    """Entry point `name` of include/lgrollout.h on the current stream of `dev` (each takes the stream last); a refusal is a RuntimeError."""
    lib = abi.load_lib()
    abi.check(getattr(lib, name)(*args, torch.cuda.current_stream(dev).cuda_stream), lib)


def _row_copies(items, refusal):
    """An LgRowCopy array from (src, dst, width, stride) items: rows of `width` floats, `stride` floats apart in src and packed in dst.
    ValueError(refusal) for anything but float32 tensors on one device, a dst that is not contiguous, or a src that is neither contiguous
    nor (where stride != width) a view with unit inner stride."""
    arr = (abi.LgRowCopy * max(len(items), 1))()
    for c, (src, dst, width, stride) in zip(arr, items):
        if (src.dtype != torch.float32 or dst.dtype != torch.float32 or src.device != dst.device or not dst.is_contiguous()
                or not (src.is_contiguous() or (stride != width and src.stride(-1) == 1))):
            raise ValueError(refusal)
        c.src, c.dst, c.width, c.src_stride = src.data_ptr(), dst.data_ptr(), width, stride
    return arr


class RolloutStorage:
    """The reference's constructor plus two keywords: `env` (zero-copy observation rows, see `attach_env`) and `lstm_critic_hidden`.

    `lstm_critic_hidden` decides what `reccurent_mini_batch_generator` hands the critic of an LSTM policy.  The reference's line
    rollout_storage.py:231 reads `hid_c_batch = hid_c_batch[0] if len(hid_c_batch)==1 else hid_a_batch`: with an LSTM (two tensors per
    network) the critic is given the ACTOR's start states.  "reference" (the default) reproduces that, so PPO.update computes what it
    computes on rsl_rl's own storage; "own" yields the critic's own (h, c).  A GRU is unaffected: its critic always gets its own.

    The storages of the other learners are this class with their own two tables and the tensors those name."""

    # (add_step keyword = Transition attribute, storage tensor), in the order of the reference's add_transitions
    STEP_ROWS = (("observations", "observations"), ("critic_observations", "privileged_observations"))
    # (storage tensor or "critic", gather kind) in the order the learner's update() unpacks, before `(None, None), None`
    BATCH = (("observations", _F32), ("critic", _F32)) + _PPO_BATCH

    class Transition:                     # rollout_storage.py:37-52
        def __init__(self):
            self.observations = None
            self.critic_observations = None
            self.actions = None
            self.rewards = None
            self.dones = None
            self.values = None
            self.actions_log_prob = None
            self.action_mean = None
            self.action_sigma = None
            self.hidden_states = None

        def clear(self):
            self.__init__()

    def __init__(self, num_envs, num_transitions_per_env, obs_shape, privileged_obs_shape, actions_shape, device="cuda:0", env=None,
                 lstm_critic_hidden="reference"):
        if lstm_critic_hidden not in ("reference", "own"):
            raise ValueError(f"lstm_critic_hidden={lstm_critic_hidden!r}: expected 'reference' or 'own'")
        self.lstm_critic_hidden = lstm_critic_hidden
        self.lib = abi.load_lib()
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise RuntimeError("hcr_genesis_lr_cl_amd.rollout.RolloutStorage needs a HIP device (no CPU fallback)")
        self.obs_shape, self.privileged_obs_shape, self.actions_shape = obs_shape, privileged_obs_shape, actions_shape
        T, N, dev = int(num_transitions_per_env), int(num_envs), self.device
        self.num_transitions_per_env, self.num_envs = T, N
        z = lambda *s, **k: torch.zeros(*s, device=dev, **k)
        self._env = None
        self.observations = None
        if env is not None:
            self.attach_env(env)
        if self.observations is None and obs_shape is not None:          # RolloutStorageEE stores no actor observations
            self.observations = z(T, N, *obs_shape)
        self.privileged_observations = z(T, N, *privileged_obs_shape) if privileged_obs_shape[0] is not None else None
        self.rewards = z(T, N, 1)
        self.actions = z(T, N, *actions_shape)
        self.dones = z(T, N, 1, dtype=torch.uint8)
        self.actions_log_prob = z(T, N, 1)
        self.values = z(T, N, 1)
        self.returns = z(T, N, 1)
        self.advantages = z(T, N, 1)
        self.mu = z(T, N, *actions_shape)
        self.sigma = z(T, N, *actions_shape)
        self._scratch = z(4, dtype=torch.float64)            # (sum, sum of squares) of the raw advantages, per group of envs
        self.saved_hidden_states_a = self.saved_hidden_states_c = None
        self._traj = self._traj_head = None                 # trajectory index buffers, allocated by the first recurrent generator call
        self.step = 0

    # ---- zero-copy observation rows -----------------------------------------------------------------------------------
    def attach_env(self, env):
        """Lay the observation rows over the env's observation copies.  Needs an env built with cfg.hip.obs_sets = T + 1 and
        unstacked observations (go2); otherwise the rows stay separate and are filled by the record kernel."""
        eng = env._engine
        raw = eng.buf.raw("obs_buf")
        T = self.num_transitions_per_env
        if int(eng.task.obs_sets) != T + 1 or int(eng.task.obs_stack) != 1 or raw.shape[1:] != (self.num_envs, *self.obs_shape):
            return False
        self._env = env
        self.observations = raw[:T]
        self._obs_all = raw
        self._sync_env_cycle()
        return True

    def _sync_env_cycle(self):
        """Start of a rollout: the env's current observation becomes row 0 and the env's next T observations land in rows 1 .. T
        (row T is the observation after the last step, i.e. row 0 of the next rollout)."""
        eng = self._env._engine
        cur = eng.obs_set()
        if cur != 0:
            self._obs_all[0].copy_(self._obs_all[cur])
        abi.check(self.lib.lg_obs_set_select(eng.handle, 0), self.lib)
        eng._refresh_obs_slot()

    @property
    def zero_copy(self):
        return self._env is not None

    # ---- filling rows -------------------------------------------------------------------------------------------------
    def add_step(self, rew, reset, time_outs, gamma, extra_copies=(), hidden_states=None, **rows):
        """One launch for everything the env contributes to row `self.step`: rewards (+ gamma * value * time_out), dones and the rows
        named in STEP_ROWS, given as keywords (each an (N, width) float32 tensor; `observations` is skipped when it is zero-copy, and so is
        a row the storage does not hold).  `values[self.step]` must already hold the critic's output for this step (the bootstrap reads
        it).  Policy-side rows (actions, values, log-prob, mean, std) are written by the caller straight into `self.actions[self.step]`
        ... as outputs of its own ops.  `hidden_states` is what a recurrent policy held BEFORE it acted on this step, as `add_transitions`
        takes it; its rows go out in the same launch."""
        self._record(gamma, *self._step_args(rew, reset, time_outs, extra_copies, hidden_states, rows))

    def _step_args(self, rew, reset, time_outs, extra_copies, hidden_states, rows):
        """What the record launch of step `self.step` takes, with every refusal of `add_step`: nothing is enqueued or written here."""
        t = self.step
        if t >= self.num_transitions_per_env:
            raise AssertionError("Rollout buffer overflow")
        known, copies = dict(self.STEP_ROWS), []
        for k, src in rows.items():
            if k not in known:
                raise TypeError(f"{type(self).__name__}.add_step: unknown row {k!r}; expected one of {', '.join(known)}")
            dst = getattr(self, known[k])
            if src is not None and dst is not None and not (k == "observations" and self.zero_copy):
                copies.append((src, dst[t]))
        copies += list(extra_copies)
        rew = self._env_row("rew", rew, (torch.float32,))
        rst = self._env_row("reset", reset, (torch.bool, torch.uint8))
        to = None if time_outs is None else self._env_row("time_outs", time_outs, (torch.bool, torch.uint8))
        copies = self._hidden_copies(t, hidden_states, len(copies)) + copies
        refusal = "row copies take (N, width) float32 views with unit inner stride"
        if any(src.dim() != 2 or src.shape != dst.shape or src.shape[0] != self.num_envs for src, dst in copies):
            raise ValueError(refusal)
        return rew, rst, to, _row_copies([(src, dst, src.shape[1], src.stride(0)) for src, dst in copies], refusal), len(copies)

    def _record(self, gamma, rew, rst, to, arr, n_copies):
        t = self.step
        _call(self.device, "lg_rollout_record", self.num_envs, rew.data_ptr(), rst.data_ptr(), 0 if to is None else to.data_ptr(),
              self.values[t].data_ptr(), float(gamma), self.rewards[t].data_ptr(), self.dones[t].data_ptr(), arr, n_copies)
        self.step += 1

    def _env_row(self, name, x, dtypes):
        """One of add_step's per-env inputs as the record kernel reads it: N elements of one of `dtypes`, consecutive in memory, on the
        storage's device.  The kernel takes a bare pointer, so anything else would be read as the wrong bytes: it is refused here, before
        any launch, and never converted (a conversion is a hidden launch; `add_transitions` is the entry point that converts).  A bool
        tensor is re-viewed as uint8, which costs nothing."""
        if (not torch.is_tensor(x) or x.dtype not in dtypes or x.numel() != self.num_envs or not x.is_contiguous()
                or x.device != self.rewards.device):
            got = f"{tuple(x.shape)} {x.dtype} strides {x.stride()} on {x.device}" if torch.is_tensor(x) else type(x).__name__
            raise ValueError(f"add_step: {name} must hold {self.num_envs} contiguous elements of {' / '.join(str(d) for d in dtypes)} on "
                             f"{self.rewards.device}, got {got}")
        return x.view(torch.uint8) if x.dtype == torch.bool else x

    def add_transitions(self, transition):
        """rollout_storage.py:89-102, the reference's entry point (rsl_rl's PPO.process_env_step has already bootstrapped
        `transition.rewards`): policy-side rows by copy_, env-side rows by the record kernel.  The reference's `copy_` converts whatever
        dtype it is given (its BaseTask.reset_buf is torch.int), so rewards and dones that are not already what the kernel reads are
        converted the same way first: dones to the uint8 of the stored row, rewards to float32."""
        rew, dones = transition.rewards.reshape(-1), transition.dones.reshape(-1)
        if rew.dtype != torch.float32 or not rew.is_contiguous():
            rew = rew.to(torch.float32).contiguous()
        if dones.dtype not in (torch.bool, torch.uint8) or not dones.is_contiguous():
            dones = dones.to(torch.uint8).contiguous()
        rows = {k: getattr(transition, k, None) for k, _ in self.STEP_ROWS}
        args = self._step_args(rew, dones, None, (), getattr(transition, "hidden_states", None), rows)      # refuses before any row is written
        t = self.step
        self.actions[t].copy_(transition.actions)
        self.values[t].copy_(transition.values)
        self.actions_log_prob[t].copy_(transition.actions_log_prob.view(-1, 1))
        self.mu[t].copy_(transition.action_mean)
        self.sigma[t].copy_(transition.action_sigma)
        self._record(0.0, *args)

    def _hidden_copies(self, t, hidden_states, n_other):
        """Row copies that store a recurrent policy's hidden states at step t (rollout_storage.py:104-119).  None or (None, None): nothing
        (the first act of a fresh policy, so row 0 of the first rollout stays zero).  A GRU gives one (L, N, H) tensor per network, an LSTM
        an (h, c) tuple; `saved_hidden_states_a` / `_c` are lists of (T, L, N, H) tensors allocated on first use -- which is why states that
        do not fit the record launch next to the step's `n_other` copies are refused here, before that allocation, and not by the launch."""
        if hidden_states is None or (hidden_states[0] is None and hidden_states[1] is None):
            return []
        hid_a, hid_c = (tuple(h) if isinstance(h, (tuple, list)) else (h,) for h in hidden_states)
        n = n_other + len(hid_a) + len(hid_c)
        if n > abi.ROLLOUT_MAX_COPIES:
            raise ValueError(f"{type(self).__name__}: {n} row copies in one step, the record launch takes {abi.ROLLOUT_MAX_COPIES}")
        self._hidden_saved(hid_a, hid_c)
        # a contiguous (L, N, H) block is copied flat; the record kernel's copies are N rows, so the block is viewed as (N, L * H)
        return [(h.contiguous().view(self.num_envs, -1), saved[t].view(self.num_envs, -1))
                for h, saved in zip(hid_a + hid_c, self.saved_hidden_states_a + self.saved_hidden_states_c)]

    def _hidden_saved(self, hid_a, hid_c):
        """`saved_hidden_states_a` / `_c` for states of these shapes: allocated on first use, checked against them afterwards."""
        T, N = self.num_transitions_per_env, self.num_envs
        if self.saved_hidden_states_a is None:
            for h in hid_a + hid_c:
                if h.dim() != 3 or h.shape[1] != N:
                    raise ValueError(f"hidden states are (layers, {N}, hidden) tensors, got {tuple(h.shape)}")
            self.saved_hidden_states_a = [torch.zeros(T, *h.shape, device=self.device) for h in hid_a]
            self.saved_hidden_states_c = [torch.zeros(T, *h.shape, device=self.device) for h in hid_c]
        if len(hid_a) != len(self.saved_hidden_states_a) or len(hid_c) != len(self.saved_hidden_states_c):
            raise ValueError("the number of hidden-state tensors changed within a storage")
        for h, saved in zip(hid_a + hid_c, self.saved_hidden_states_a + self.saved_hidden_states_c):
            if h.shape != saved.shape[1:] or h.dtype != torch.float32 or h.device != saved.device:
                raise ValueError(f"hidden state {tuple(h.shape)} {h.dtype} on {h.device} does not fit the stored {tuple(saved.shape[1:])} float32")

    def hidden_state_rows(self, hidden_states):
        """Row `self.step` of the saved hidden states, as ((L, N, H) views for the actor's memory, likewise the critic's), for a producer
        that writes the pre-step states there itself (`FusedPolicy.act(storage=...)`: the launch fills them, and `add_step` is then
        called without `hidden_states`).  `hidden_states` is the policy's `get_hidden_states()`, read for its shapes only: the saved
        lists are allocated on first use and checked exactly as `add_step(hidden_states=...)` does."""
        t = self.step
        if t >= self.num_transitions_per_env:
            raise AssertionError("Rollout buffer overflow")
        hid_a, hid_c = (tuple(h) if isinstance(h, (tuple, list)) else (h,) for h in hidden_states)
        self._hidden_saved(hid_a, hid_c)
        return [s[t] for s in self.saved_hidden_states_a], [s[t] for s in self.saved_hidden_states_c]

    def clear(self):
        self.step = 0
        if self.zero_copy:
            self._sync_env_cycle()

    def compute_returns(self, last_values, gamma, lam):
        """rollout_storage.py:124-138 in two launches."""
        self._gae("lg_rollout_gae", (), last_values, gamma, lam, self.advantages)

    def _gae(self, name, groups, last_values, gamma, lam, *advantages):
        lv = last_values.reshape(-1).contiguous().float()
        _call(self.device, name, self.num_transitions_per_env, self.num_envs, *groups, self.values.data_ptr(), self.rewards.data_ptr(),
              self.dones.data_ptr(), lv.data_ptr(), float(gamma), float(lam), self.returns.data_ptr(), *(a.data_ptr() for a in advantages),
              self._scratch.data_ptr())

    def get_statistics(self):
        """(mean trajectory length, mean reward) of the stored rollout -- what rollout_storage.py:140-146 reports: a trajectory ends at
        a done flag or at the last stored step.  Leaves `dones` untouched."""
        ends = self.dones.squeeze(-1).t().bool().clone()        # (N, T), env-major like the reference's flattening
        ends[:, -1] = True
        idx = torch.nonzero(ends.reshape(-1)).squeeze(1)
        lengths = torch.diff(idx, prepend=idx.new_full((1,), -1))
        return lengths.float().mean(), self.rewards.mean()

    def mini_batch_generator(self, num_mini_batches, num_epochs=8):
        """Mini-batches in the tuple order the learner's update() unpacks: BATCH, then hidden states (None, None) and masks None; for this
        class (rollout_storage.py:148-186) obs, critic obs, actions, target values, advantages, returns, old log-prob, old mean, old std.
        One random permutation of the T x N samples per call, cut into `num_mini_batches` equal index blocks and replayed every epoch;
        each yield is one gather launch into fresh tensors."""
        per = (self.num_envs * self.num_transitions_per_env) // num_mini_batches
        perm = torch.randperm(num_mini_batches * per, device=self.device)
        entries = [(self._batch_source(name), kind, 0, None) for name, kind in self.BATCH]
        for batch in self._gather_batches(entries, [(perm, per)], num_mini_batches, num_epochs):
            yield (*batch, (None, None), None)

    def _batch_source(self, name):
        """The tensor behind an entry of BATCH.  "critic" is what the critic reads: the privileged observations if they are stored, else the
        actor's input -- the observations, or where none are stored (the explicit estimator, rollout_storage_ee.py:116-123) the estimator
        features and labels side by side, concatenated once per generator call."""
        if name != "critic":
            return getattr(self, name)
        if self.privileged_observations is not None:
            return self.privileged_observations
        return self.observations if hasattr(self, "observations") else torch.cat((self.estimator_features, self.estimator_labels), dim=-1)

    def _gather_batches(self, entries, index_sets, num_mini_batches, num_epochs):
        """The tensors of every mini-batch, one `lg_rollout_gather` launch per mini-batch.  `entries`: (source, kind, index set, window) per
        yielded tensor; the source is a (T, n, ...) tensor with contiguous rows, `window` is None (index r is row r of source.flatten(0, 1))
        or (first env, envs): index r is row r of source[:, first:first + envs].flatten(0, 1), read in place.  `index_sets`: (permutation
        int64, rows per mini-batch); mini-batch i takes entries [i * rows, (i + 1) * rows) of each, and every epoch replays them.  Yields
        lists of freshly allocated contiguous float32 tensors (rows, ...): nothing is shared between yields."""
        if len(entries) > abi.ROLLOUT_MAX_GATHER:
            raise ValueError(f"a mini-batch of {len(entries)} tensors: one gather launch takes {abi.ROLLOUT_MAX_GATHER}")
        dev = self.device
        arr = (abi.LgGatherItem * len(entries))()
        shapes = []
        for it, (x, kind, k, window) in zip(arr, entries):
            want = torch.uint8 if kind == abi.GATHER_NOT_U8 else torch.float32
            n = x.shape[1] if x.dim() >= 2 else 0
            stride = 0 if n == 0 else (x.stride(1) if n > 1 else x.stride(0))
            width = x[0, 0].numel() if n else 0
            if (n == 0 or x.dtype != want or x.device != dev or width < 1 or not x[0, 0].is_contiguous() or stride < width
                    or (x.shape[0] > 1 and n > 1 and x.stride(0) != n * stride)):
                raise ValueError(f"mini-batch sources are (T, envs, ...) {want} tensors on {dev} with contiguous rows and one row stride, got "
                                 f"{tuple(x.shape)} {x.dtype} strides {x.stride()} on {x.device}")
            first, group = (0, n) if window is None else window
            perm, rows = index_sets[k]
            if perm.dtype != torch.int64 or not perm.is_contiguous() or perm.device != dev or perm.numel() < num_mini_batches * rows:
                raise ValueError("mini-batch index sets are contiguous int64 tensors on the storage's device")
            it.src, it.rows, it.width, it.src_stride, it.kind = x.data_ptr(), rows, width, stride, kind
            it.group, it.env_offset, it.n_envs = group, first, n
            shapes.append((rows, *x.shape[2:]))
        if all(rows == 0 for _, rows in index_sets):                  # more mini-batches than samples: empty batches, as indexing gives
            for _ in range(num_epochs * num_mini_batches):
                yield [torch.empty(sh, device=dev) for sh in shapes]
            return
        stream = torch.cuda.current_stream(dev).cuda_stream
        gather, lib, n_items = self.lib.lg_rollout_gather, self.lib, len(entries)
        bases = [index_sets[k][0].data_ptr() for _, _, k, _ in entries]
        for _ in range(num_epochs):
            for i in range(num_mini_batches):
                out = [torch.empty(sh, device=dev) for sh in shapes]
                for it, o, base in zip(arr, out, bases):
                    it.dst, it.index = o.data_ptr(), base + 8 * i * it.rows
                abi.check(gather(arr, n_items, stream), lib)
                yield out

    # ---- recurrent policies ---------------------------------------------------------------------------------------------
    def trajectory_index(self):
        """Trajectories of the stored rollout, env-major then by time (a trajectory starts at t = 0 and behind every done and ends at a
        done or at the last step): (index, n_traj, max_len, traj_offset).  `index` is a (3, T * N) int32 device tensor whose first n_traj
        columns hold env, t_start and length; `traj_offset` is a host list of N + 1 ints, the first trajectory of every env.  One launch
        and ONE device-to-host copy (header + offsets); nothing else in the recurrent generator waits for the device."""
        T, N = self.num_transitions_per_env, self.num_envs
        if self._traj is None:
            self._traj = torch.empty(3, T * N, dtype=torch.int32, device=self.device)
            self._traj_head = torch.empty(2 + N + 1, dtype=torch.int32, device=self.device)      # n_traj, max_len, traj_offset[N + 1]
        _call(self.device, "lg_rollout_traj_index", T, N, self.dones.data_ptr(), self._traj_head[2:].data_ptr(), self._traj.data_ptr(), T * N,
              self._traj_head.data_ptr())
        host = self._traj_head.cpu().tolist()
        return self._traj, host[0], host[1], host[2:]

    def pad_trajectories(self, tensors, index=None, hidden=(), masks=True):
        """split_and_pad_trajectories (rsl_rl/utils/utils.py:33-65) of up to eight contiguous (T, N, ...) float32 tensors in one launch that
        shares one trajectory index: ([padded (max_len, n_traj, ...)], [start states (L, n_traj, H) of every (T, L, N, H) tensor in
        `hidden`], masks (T, n_traj) bool or None).  The masks keep T rows where max_len < T, as the reference's do."""
        T, N = self.num_transitions_per_env, self.num_envs
        traj, n_traj, max_len, _ = index if index is not None else self.trajectory_index()
        dev = self.device

        src_items, hid_items = [], []
        for x in tensors:
            if x.dim() < 2 or x.shape[0] != T or x.shape[1] != N:
                raise ValueError(f"padded tensors are ({T}, {N}, ...), got {tuple(x.shape)}")
            width = x[0, 0].numel()
            src_items.append((x, torch.empty(max_len, n_traj, *x.shape[2:], device=dev), width, width))
        for h in hidden:
            if h.dim() != 4 or h.shape[0] != T or h.shape[2] != N:
                raise ValueError(f"saved hidden states are ({T}, layers, {N}, hidden), got {tuple(h.shape)}")
            hid_items.append((h, torch.empty(h.shape[1], n_traj, h.shape[3], device=dev), h.shape[3], h.shape[3]))
        layers = [h.shape[1] for h in hidden]
        mask = torch.empty(T, n_traj, dtype=torch.bool, device=dev) if masks else None
        _call(dev, "lg_rollout_pad", T, N, traj.data_ptr(), traj.shape[1], n_traj, max_len,
              _row_copies(src_items, f"padded tensors must be contiguous float32 tensors on {dev}"), len(src_items),
              _row_copies(hid_items, f"saved hidden states must be contiguous float32 tensors on {dev}"), (C.c_int32 * max(len(layers), 1))(*layers),
              len(hid_items), 0 if mask is None else mask.data_ptr())
        return [it[1] for it in src_items], [it[1] for it in hid_items], mask

    def reccurent_mini_batch_generator(self, num_mini_batches, num_epochs=8):
        """Mini-batches for a recurrent policy in the tuple order rsl_rl's PPO.update unpacks (rollout_storage.py:187-236; the spelling is
        the reference's): padded obs, padded critic obs (the actor's when there are no privileged observations), actions, values, advantages,
        returns, old log-prob, old mean, old std, (hid_a, hid_c), masks.  Mini-batch i is envs [i * N // num_mini_batches, (i + 1) * ...)
        in order, not shuffled; the (T, start:stop, .) tensors are views of the storage; the padded tensors and masks are views of one
        padded set built per call (index launch, one read-back, pad launch: no other host sync, whatever the number of mini-batches and
        epochs).  Start hidden states are gathered once for all trajectories as (L, n_traj, H); each mini-batch gets a contiguous copy
        of its slice (one small copy per tensor per mini-batch, made in the first epoch and yielded again in the later ones: treat them
        as read-only, as PPO.update does).  A GRU yields tensors for hid_a / hid_c, an LSTM lists of two; see the class docstring for
        `lstm_critic_hidden`."""
        if self.saved_hidden_states_a is None:
            raise RuntimeError("reccurent_mini_batch_generator: no hidden states were stored (add_transitions / add_step with hidden_states)")
        index = self.trajectory_index()
        offsets = index[3]
        tensors = [self.observations] + ([self.privileged_observations] if self.privileged_observations is not None else [])
        n_a = len(self.saved_hidden_states_a)
        # an LSTM's critic is handed the actor's start states unless asked otherwise (rollout_storage.py:231): its own are then not gathered
        own_critic = len(self.saved_hidden_states_c) == 1 or self.lstm_critic_hidden == "own"
        padded, hid, masks = self.pad_trajectories(tensors, index, self.saved_hidden_states_a + (self.saved_hidden_states_c if own_critic else []))
        padded_obs, padded_critic = padded[0], padded[-1]
        per = self.num_envs // num_mini_batches
        hid_batches = []
        for epoch in range(num_epochs):
            for i in range(num_mini_batches):
                start, stop = i * per, (i + 1) * per
                first, last = offsets[start], offsets[stop]
                if epoch == 0:
                    hid_a = [h[:, first:last].contiguous() for h in hid[:n_a]]
                    hid_c = [h[:, first:last].contiguous() for h in hid[n_a:]] if own_critic else hid_a
                    hid_batches.append((hid_a[0] if len(hid_a) == 1 else hid_a, hid_c[0] if len(hid_c) == 1 else hid_c))
                hid_a, hid_c = hid_batches[i]
                yield (padded_obs[:, first:last], padded_critic[:, first:last], self.actions[:, start:stop], self.values[:, start:stop],
                       self.advantages[:, start:stop], self.returns[:, start:stop], self.actions_log_prob[:, start:stop],
                       self.mu[:, start:stop], self.sigma[:, start:stop], (hid_a, hid_c), masks[:, first:last])


class RolloutStorageEE(RolloutStorage):
    """rsl_rl/storage/rollout_storage_ee.py (PPO_EE, the explicit estimator): no actor observations are stored; the actor's input is the
    estimator features and labels.  `add_step` keywords: critic_observations, estimator_features, estimator_labels.  Mini-batches are the
    13 entries of rollout_storage_ee.py:152-154; `terminated` is float32 1 - dones, formed by the gather."""

    class Transition(RolloutStorage.Transition):
        def __init__(self):
            super().__init__()
            self.estimator_features = None
            self.estimator_labels = None

    STEP_ROWS = (("critic_observations", "privileged_observations"), ("estimator_features", "estimator_features"), ("estimator_labels", "estimator_labels"))
    BATCH = (("critic", _F32), ("estimator_features", _F32), ("estimator_labels", _F32), ("dones", _NOT)) + _PPO_BATCH

    def __init__(self, num_envs, num_transitions_per_env, privileged_obs_shape, estimator_feature_shape, estimator_label_shape, actions_shape,
                 device="cuda:0"):
        super().__init__(num_envs, num_transitions_per_env, None, privileged_obs_shape, actions_shape, device)
        del self.observations, self.obs_shape
        self.estimator_feature_shape, self.estimator_label_shape = estimator_feature_shape, estimator_label_shape
        T, N = self.num_transitions_per_env, self.num_envs
        self.estimator_features = torch.zeros(T, N, *estimator_feature_shape, device=self.device)
        self.estimator_labels = torch.zeros(T, N, *estimator_label_shape, device=self.device)


class RolloutStorageTS(RolloutStorage):
    """rsl_rl/storage/rollout_storage_ts.py (PPO_TS, teacher-student): privileged observations feed the privilege encoder, critic
    observations the critic.  `add_step` keywords: observations, privileged_observations, observation_histories, critic_observations.
    Mini-batches are the 14 entries of rollout_storage_ts.py:115-117."""

    class Transition(RolloutStorage.Transition):
        def __init__(self):
            super().__init__()
            self.privileged_observations = None
            self.observation_histories = None

    STEP_ROWS = (("observations", "observations"), ("privileged_observations", "privileged_observations"),
                 ("observation_histories", "observation_histories"), ("critic_observations", "critic_observations"))
    BATCH = (("observations", _F32), ("privileged_observations", _F32), ("observation_histories", _F32), ("critic_observations", _F32),
             ("dones", _NOT)) + _PPO_BATCH

    def __init__(self, num_envs, num_transitions_per_env, obs_shape, privileged_obs_shape, obs_history_shape, critic_obs_shape, actions_shape,
                 device="cuda:0"):
        if privileged_obs_shape[0] is None:
            raise ValueError(f"Privileged observations are required for {type(self).__name__}")
        super().__init__(num_envs, num_transitions_per_env, obs_shape, privileged_obs_shape, actions_shape, device)
        self.obs_history_shape, self.critic_obs_shape = obs_history_shape, critic_obs_shape
        T, N = self.num_transitions_per_env, self.num_envs
        self.observation_histories = torch.zeros(T, N, *obs_history_shape, device=self.device)
        self.critic_observations = torch.zeros(T, N, *critic_obs_shape, device=self.device)


class RolloutStorageDreamWaQ(RolloutStorage):
    """rsl_rl/storage/rollout_storage_dreamwaq.py (PPO_DreamWaQ).  `add_step` keywords: observations, privileged_observations,
    observation_histories, explicit_info_labels, next_states -- five rows, so a recurrent policy's hidden states on top (an LSTM has four
    tensors) do not fit one record launch and are refused.  Mini-batches are the 15 entries of rollout_storage_dreamwaq.py:121-123."""

    class Transition(RolloutStorage.Transition):
        def __init__(self):
            super().__init__()
            self.privileged_observations = None
            self.observation_histories = None
            self.explicit_info_labels = None
            self.next_states = None

    STEP_ROWS = (("observations", "observations"), ("privileged_observations", "privileged_observations"),
                 ("observation_histories", "observation_histories"), ("explicit_info_labels", "explicit_info_labels"), ("next_states", "next_states"))
    BATCH = (("observations", _F32), ("privileged_observations", _F32), ("observation_histories", _F32), ("explicit_info_labels", _F32),
             ("next_states", _F32), ("dones", _NOT)) + _PPO_BATCH

    def __init__(self, num_envs, num_transitions_per_env, obs_shape, privileged_obs_shape, obs_history_shape, explicit_info_shape,
                 next_states_shape, actions_shape, device="cuda:0"):
        if privileged_obs_shape[0] is None:
            raise ValueError("privileged_observations is necessary for DreamWaQ RolloutStorage")
        super().__init__(num_envs, num_transitions_per_env, obs_shape, privileged_obs_shape, actions_shape, device)
        self.obs_history_shape = obs_history_shape
        T, N = self.num_transitions_per_env, self.num_envs
        self.observation_histories = torch.zeros(T, N, *obs_history_shape, device=self.device)
        self.explicit_info_labels = torch.zeros(T, N, *explicit_info_shape, device=self.device)
        self.next_states = torch.zeros(T, N, *next_states_shape, device=self.device)


class RolloutStorageCTS(RolloutStorageTS):
    """rsl_rl/storage/rollout_storage_cts.py (PPO_CTS, concurrent teacher-student): envs [0, num_teacher) are the teacher's, the rest the
    student's.  `compute_returns` is one GAE pass whose advantages are split into `teacher_advantages` (T, num_teacher, 1) and
    `student_advantages` (T, N - num_teacher, 1), each normalised by its own mean and std (`lg_rollout_gae_groups`); `advantages` is left
    alone, as in the reference.  Mini-batches are the 18 entries of rollout_storage_cts.py:179-184: seven gathered by a permutation of
    the teacher's samples, six by one of the student's, three by one of all samples, in one launch; the teacher / student tensors are
    read from the (T, N, width) rows in place (the reference flattens a copy of each on every call)."""

    def __init__(self, num_envs, num_teacher, num_transitions_per_env, obs_shape, privileged_obs_shape, obs_history_shape, critic_obs_shape,
                 actions_shape, device="cuda:0"):
        if not 1 <= int(num_teacher) <= int(num_envs) - 1:
            raise ValueError(f"num_teacher={num_teacher}: both groups need an env, expected 1 .. {int(num_envs) - 1}")
        super().__init__(num_envs, num_transitions_per_env, obs_shape, privileged_obs_shape, obs_history_shape, critic_obs_shape, actions_shape, device)
        self.num_teacher = int(num_teacher)
        T, N = self.num_transitions_per_env, self.num_envs
        self.teacher_advantages = torch.zeros(T, self.num_teacher, 1, device=self.device)
        self.student_advantages = torch.zeros(T, N - self.num_teacher, 1, device=self.device)

    def compute_returns(self, last_values, gamma, lam):
        """rollout_storage_cts.py:81-114 in four launches (memset, GAE, one normalisation per group)."""
        self._gae("lg_rollout_gae_groups", (self.num_teacher,), last_values, gamma, lam, self.teacher_advantages, self.student_advantages)

    def mini_batch_generator(self, num_mini_batches, num_epochs=8):
        """Mini-batch sizes are the reference's: num_teacher * T // n for the teacher, (N - num_teacher) * T // n for the student, their sum
        for the critic's three tensors (not N * T // n).  Three permutations per call, drawn in the reference's order."""
        T, N, nt, dev = self.num_transitions_per_env, self.num_envs, self.num_teacher, self.device
        per_t, per_s = nt * T // num_mini_batches, (N - nt) * T // num_mini_batches
        sets = [(torch.randperm(num_mini_batches * per, device=dev), per) for per in (per_t, per_s, per_t + per_s)]
        teacher, student = (0, nt), (nt, N - nt)
        entries = [(getattr(self, k), _F32, 0, teacher) for k in ("observations", "privileged_observations", "actions", "actions_log_prob")]
        entries += [(self.teacher_advantages, _F32, 0, None), (self.mu, _F32, 0, teacher), (self.sigma, _F32, 0, teacher)]
        entries += [(getattr(self, k), _F32, 1, student) for k in ("observations", "privileged_observations", "observation_histories", "actions",
                                                                   "actions_log_prob")]
        entries += [(self.student_advantages, _F32, 1, None)]
        entries += [(getattr(self, k), _F32, 2, None) for k in ("critic_observations", "values", "returns")]
        for batch in self._gather_batches(entries, sets, num_mini_batches, num_epochs):
            yield (*batch, (None, None), None)


class _Unpad(torch.autograd.Function):
    """unpad_trajectories with its gradient: forward scatters the valid rows back to (T, envs, width), backward is the pad gather."""

    @staticmethod
    def forward(ctx, trajectories, masks):
        dev = trajectories.device
        if dev.type != "cuda" or trajectories.dtype != torch.float32 or trajectories.dim() < 2:
            raise ValueError("unpad_trajectories takes a (rows, n_traj, ...) float32 tensor on a HIP device (no CPU fallback)")
        rows, n_traj = trajectories.shape[:2]
        if masks.dim() != 2 or masks.shape[1] != n_traj or masks.dtype not in (torch.bool, torch.uint8) or masks.device != dev:
            raise ValueError(f"masks are (T, {n_traj}) bool on {dev}, got {tuple(masks.shape)} {masks.dtype}")
        T = masks.shape[0]
        x, m = trajectories.contiguous(), masks.contiguous()
        width = x[0, 0].numel()
        index = torch.empty(3, n_traj, dtype=torch.int32, device=dev)
        head = torch.empty(2, dtype=torch.int32, device=dev)
        _call(dev, "lg_rollout_mask_index", T, n_traj, m.data_ptr(), index.data_ptr(), n_traj, head.data_ptr())
        steps, longest = head.cpu().tolist()                           # the one read-back: the env count sizes the output
        if steps % T or longest > rows:
            raise ValueError(f"masks cover {steps} steps with a longest trajectory of {longest}: not whole envs of {T} steps within {rows} rows")
        n = steps // T
        out = torch.empty(T, n, *x.shape[2:], device=dev)              # the trajectories tile (T, n): every element is written
        _call(dev, "lg_rollout_unpad", T, n, index.data_ptr(), n_traj, n_traj, rows, x.data_ptr(), out.data_ptr(), width)
        ctx.index, ctx.dims = index, (T, n, n_traj, rows, width, tuple(x.shape))
        return out

    @staticmethod
    def backward(ctx, grad):
        T, n, n_traj, rows, width, shape = ctx.dims
        g = grad.contiguous()
        out = torch.empty(shape, device=g.device)
        arr = _row_copies([(g, out, width, width)], "the gradient of unpad_trajectories is a float32 tensor")
        _call(g.device, "lg_rollout_pad", T, n, ctx.index.data_ptr(), n_traj, n_traj, rows, arr, 1, None, None, 0, 0)
        return out, None


def unpad_trajectories(trajectories, masks):
    """The inverse of split_and_pad_trajectories (rsl_rl/utils/utils.py:67-71, what Memory.forward applies to the RNN's output on every
    update): trajectories (rows, n_traj, ...) float32, masks (T, n_traj) bool as the recurrent generator yields them -> (T, envs, ...),
    contiguous, differentiable (the gradient is the pad gather).  The trajectory index is rebuilt from the masks on the device; the env
    count is read back from it (one small copy; the reference's boolean indexing waits for the device as well) and the masks are checked
    to cover whole envs."""
    return _Unpad.apply(trajectories, masks)
