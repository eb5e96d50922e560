"""Which Philox word the product path feeds to each uniform slot.  TEST INFRASTRUCTURE ONLY.

The INJ instantiations read their uniforms from a row `rand_in[slot]` laid out by LgRandSlots (builders.go2_slots).  Without
`rand_in` the kernels draw from Philox4x32-10 keyed on (seed, global env id, step counter, counter word).  `uniforms()`
returns the row the INJ instantiation needs to reproduce a Philox step, so an oracle fed with it computes what the product
kernels compute.  Every rule below was restated by reading the kernel; each cites the lines it restates.

Philox call (lg_kernel.h:1224-1231): key (k0, k1) = (seed lo, seed hi), counter (e_lo, e_hi, step, c3) where
(e_lo, e_hi) = global env id (env_id_offset + local id) lo / hi and step = the launch's counter.  Three spaces of c3:
  SLOT    c3 = slot >> 2, word slot & 3                 RandSrc::draw (lg_kernel.h:171-180)
  TRIPLE  c3 = 0x40000000 + first slot, words 0..2 / 3  RandSrc::draw3 / draw4 (lg_kernel.h:183-198): one call per 3 / 4 slots
  BLOCK   c3 = 0x80000000 + id, words 0..3              RandSrc::block3 / block4 (lg_kernel.h:201-214)
Block ids 0 .. 4 LEGS + 1 carry observation noise; ids 0x200 + b carry the env-level reset bundle (lg_kernel.h:1577-1641):
bundle entry i is block 0x200 + (i >> 2), word i & 3 (quadruped: lane `leg` evaluates block 0x200 + leg; biped: lane `leg`
of the env's pair evaluates blocks 0x200 + 3 leg + 0..2; the DPP broadcasts put them in eu[] in that order).
Batch-wide draws (one value for the whole batch per call) use env words 0xFFFFFFFF, 0xFFFFFFFF: the go2_wtw gait index
(task_cb + 4, task_reset + 4: lg_kernel.h:1254-1257) and the biped sit coin (task_reset: lg_kernel.h:1660-1667).
"""
from __future__ import annotations

from typing import NamedTuple

import numpy as np

from hcr_genesis_lr_cl_amd import abi
from oracle.philox import philox4x32_10, u01

TRIPLE, BLOCK, BUNDLE = 0x40000000, 0x80000000, 0x80000000 + 0x200
ALL_ONES = 0xFFFFFFFF


class Rule(NamedTuple):
    batch_wide: bool      # env words all ones instead of the global env id
    counter: int          # fourth counter word
    word: int             # which output word (0..3)


def _slot(s, batch_wide=False):
    return Rule(batch_wide, s >> 2, s & 3)


def _bundle(i):
    return Rule(False, BUNDLE + (i >> 2), i & 3)


def _block(b, w):
    return Rule(False, BLOCK + b, w)


def rules(slots, legs, jpl, obs_layout):
    """Rule per slot (a list of n_slots entries); None where no kernel reads that slot: the noise entries whose noise scale is
    zero (commands, and actions / clock / task entries outside OBS_TRON1_EE), task_cb / task_reset outside go2_wtw and the
    bipeds, and task_cb, task_reset + 3, + 4 of the bipeds."""
    S, A = slots, legs * jpl
    R = [None] * S.n_slots
    biped = legs == 2

    def triples(first, n):        # _reset_dofs / kp / kd: one TRIPLE call per lane, lane l covers dofs jpl l .. jpl l + jpl - 1
        for d in range(n):
            R[first + d] = Rule(False, TRIPLE + first + jpl * (d // jpl), d % jpl)

    # _post_physics_step_callback: command resampling, resample_commands(cb_cmd) -> draw3 (lg_kernel.h:1266-1270, 1286)
    for k in range(3):
        R[S.cb_cmd + k] = Rule(False, TRIPLE + S.cb_cmd, k)
    # push: draw(push), draw(push + 1) (lg_kernel.h:1293)
    for k in range(2):
        R[S.push + k] = _slot(S.push + k)
    # reset commands: bundle entries 0-2 (lg_kernel.h:1638-1639, 1659)
    for k in range(3):
        R[S.reset_cmd + k] = _bundle(k)
    # _reset_dofs: draw3 / draw4 at reset_dof + d0 (lg_kernel.h:1674-1675; replicated launch 1587-1607: same counter)
    triples(S.reset_dof, A)
    # root xy: draw(reset_root_xy), draw(reset_root_xy + 1) (lg_kernel.h:1687-1688; replicated 1611-1613)
    for k in range(2):
        R[S.reset_root_xy + k] = _slot(S.reset_root_xy + k)
    # root twist: bundle 8-10 and 12-14 (lg_kernel.h:1694)
    for k in range(3):
        R[S.reset_lin_vel + k] = _bundle(8 + k)
        R[S.reset_ang_vel + k] = _bundle(12 + k)
    # friction 3, mass 7, CoM 4-6 (lg_kernel.h:1756-1760)
    R[S.dr_friction] = _bundle(3)
    R[S.dr_mass] = _bundle(7)
    for k in range(3):
        R[S.dr_com + k] = _bundle(4 + k)
    # kp / kd scales: draw3 / draw4 at dr_kp + d0, dr_kd + d0 (lg_kernel.h:1732-1737)
    triples(S.dr_kp, A)
    triples(S.dr_kd, A)
    # joint armature / friction / damping: biped bundle 16-18, quadruped draw3(dr_joint) (lg_kernel.h:1765-1768)
    for k in range(3):
        R[S.dr_joint + k] = _bundle(16 + k) if biped else Rule(False, TRIPLE + S.dr_joint, k)
    # terrain level above the top: biped bundle 21, quadruped draw(terrain_level) (lg_kernel.h:1652)
    R[S.terrain_level] = _bundle(21) if biped else _slot(S.terrain_level)
    if biped:
        # sit coin, one per call: draw(task_reset) on env words all ones (lg_kernel.h:1662-1666); gait phase offset and
        # clock: bundle 19, 20 (lg_kernel.h:1706-1708).  task_cb and task_reset + 3, + 4 are not read by a biped.
        R[S.task_reset] = _slot(S.task_reset, batch_wide=True)
        R[S.task_reset + 1] = _bundle(19)
        R[S.task_reset + 2] = _bundle(20)
    elif obs_layout == abi.OBS_GO2_WTW:
        # go2_wtw behaviour resampling at the callback (task_cb) and at reset (task_reset): four per-env draws and one
        # gait index for the whole batch (lg_kernel.h:1249-1257, 1302, 1658).  The other quadrupeds read neither group.
        for base in (S.task_cb, S.task_reset):
            for k in range(4):
                R[base + k] = _slot(base + k)
            R[base + 4] = _slot(base + 4, batch_wide=True)
    # observation noise (lg_kernel.h:1860-1929): frame = commands 3, gravity 3, ang vel 3, q A, qd A, actions A, clock 2 LEGS
    ns = S.noise
    for leg in range(legs):
        for j in range(jpl):
            R[ns + 9 + jpl * leg + j] = _block(2 * leg, j)            # q: block 2 leg
            R[ns + 9 + A + jpl * leg + j] = _block(2 * leg + 1, j)    # qd: block 2 leg + 1
    for k in range(6):                                                 # gravity + ang vel: ub[0..5]
        if not biped:
            R[ns + 3 + k] = _block(k, 3)                               # fourth word of the blocks of lanes 0-2 (:1898)
        elif k >= 2:
            R[ns + 3 + k] = _block(2 * legs, k - 2)                    # block 2 LEGS (:1906)
        elif jpl == 3:
            R[ns + 3 + k] = _block(k, 3)                               # fourth word of the lead's two blocks (:1886-1887)
        else:
            R[ns + 3 + k] = _block(2 * legs + 1, k)                    # four-joint legs: block 2 LEGS + 1 (:1904)
    if obs_layout == abi.OBS_TRON1_EE:                                 # noisy actions and clock (tron1_pf_ee quirk 4, :1912-1929)
        for leg in range(legs):
            for j in range(jpl):
                R[ns + 9 + 2 * A + jpl * leg + j] = _block(2 * legs + 2 + leg, j)
            # the clock entry of foot slot f is lane f's (feet are in chain order for every model)
            R[ns + 9 + 3 * A + leg] = _block(3 * legs + 2 + leg, 0)
            R[ns + 9 + 3 * A + legs + leg] = _block(3 * legs + 2 + leg, 1)
    return R


def uniforms(slots, seed, gids, step, legs, jpl, obs_layout):
    """(N, n_slots) float32: the `rand_in` rows that make the INJ instantiation reproduce the Philox step `step` (the launch's
    counter; a scalar, or one per row) of the global env ids `gids`.  Slots without a rule get 0.5: no kernel reads them."""
    gids = np.asarray(gids, np.uint64).reshape(-1)
    N = gids.shape[0]
    step = np.broadcast_to(np.asarray(step, np.int64).astype(np.uint64) & np.uint64(ALL_ONES), (N,))
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    k0, k1 = seed & ALL_ONES, seed >> 32
    e_lo, e_hi = gids & np.uint64(ALL_ONES), gids >> np.uint64(32)
    out = np.full((N, slots.n_slots), 0.5, np.float32)
    calls = {}                                 # (batch_wide, counter) -> four words, one Philox evaluation per distinct call
    for s, r in enumerate(rules(slots, legs, jpl, obs_layout)):
        if r is None:
            continue
        key = (r.batch_wide, r.counter)
        if key not in calls:
            lo, hi = (ALL_ONES, ALL_ONES) if r.batch_wide else (e_lo, e_hi)
            w = philox4x32_10(lo, hi, step, r.counter, k0, k1)
            calls[key] = [np.broadcast_to(v, (N,)) for v in w]
        out[:, s] = u01(calls[key][r.word])
    return out


def task_uniforms(task, model, gids, step):
    """uniforms() for an LgTaskCfg (its slots, seed) and model (legs, joints per leg)."""
    return uniforms(task.slots, task.seed, gids, step, model.n_legs, model.joints_per_leg, task.obs_layout)
