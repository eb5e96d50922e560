"""What the build's DPP hazard pass (hcr_genesis_lr_cl_amd/dpp_hazard_pass.py) takes for granted about the chip, checked on the chip: a DPP
instruction needs its two wait states behind a VALU write of its DPP-ROUTED source only; a plain operand, the accumulator or the masked-off
lanes' old destination written in the slot before is forwarded.  lg_dpp_kat: the first three forms; lg_dpp_kat_run: the table of
csrc/lg_dpp_kat.h -- every form the built kernels forward (tests/test_dpp_hazard_pass.py checks that), a grid around them, and the
negative controls that show the chip does read a fresh DPP source stale, against an exact reference (hcr_genesis_lr_cl_amd/dpp_kat.py)."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def rot1(v):      # quad_perm:[1,2,0,3] inside every quad of the wave
    q = v.reshape(-1, 4)
    return q[:, [1, 2, 0, 3]].reshape(-1)


def test_only_the_dpp_routed_operand_needs_wait_states():
    from hcr_genesis_lr_cl_amd import abi
    lib = abi.load_lib()
    rng = np.random.default_rng(7)
    for rep in range(8):
        x = rng.uniform(-4, 4, 64).astype(np.float32)
        y = rng.uniform(-4, 4, 64).astype(np.float32)
        inp = np.concatenate([x, y]).astype(np.float32)
        out = np.zeros(320, np.float32)
        abi.check(lib.lg_dpp_kat(inp.ctypes.data_as(C.POINTER(C.c_float)), out.ctypes.data_as(C.POINTER(C.c_float))), lib)
        r0, r1, r2, r3, a = out.reshape(5, 64)
        xy = x * y
        np.testing.assert_array_equal(a, xy)
        np.testing.assert_array_equal(r0, rot1(x) + xy)                                   # fresh plain operand: no wait state needed
        fused = (rot1(x).astype(np.float64) * y.astype(np.float64) + xy.astype(np.float64)).astype(np.float32)
        assert np.max(np.abs(r1 - fused) / np.maximum(np.abs(fused), 1e-6)) < 2e-7            # fresh accumulator: likewise (fused multiply-add)
        np.testing.assert_array_equal(r2, rot1(xy) + x)                                   # fresh DPP source behind `s_nop 1`
    # the negative control (fresh DPP source, no wait state) is reported only: on gfx950 it reads the register's previous content
    stale = int(np.sum(~(r3 == rot1(xy) + x)))
    print(f"negative control: {stale} of 64 lanes differ from the waited result")


# ---- the table-driven KAT (csrc/lg_dpp_kat.h): every form the built kernels forward, the grid, the negative controls ----

def _kat_run(lib, inp, blocks, threads, expect=None):
    from hcr_genesis_lr_cl_amd import abi
    n = lib.lg_dpp_kat_cases()
    first = np.zeros((n, 2, 64), np.float32)
    mis = np.zeros((n, 2, 64), np.uint32)
    inp = np.ascontiguousarray(inp, np.float32)
    exp = None if expect is None else np.ascontiguousarray(expect.view(np.uint32))
    abi.check(lib.lg_dpp_kat_run(inp.ctypes.data, None if exp is None else exp.ctypes.data, blocks, threads, first.ctypes.data,
                                 None if exp is None else mis.ctypes.data), lib)
    return first, mis


def _controls(table):
    """control -> (fresh DPP source at distance 0, at 1, waited) cases of the per-control negative controls (v_add_f32_dpp, plain writer)."""
    out = {}
    for c in table:
        if c.role == "dpp_src" and c.writer == "valu" and c.mnemonic == "v_add_f32_dpp":
            out.setdefault(c.control, {})[c.dist] = c
    return out


def test_every_forwarded_dpp_form_is_exact_on_the_chip():
    from hcr_genesis_lr_cl_amd import abi
    from hcr_genesis_lr_cl_amd import dpp_kat as K
    lib = abi.load_lib()
    table = K.cases()
    assert lib.lg_dpp_kat_cases() == len(table)
    ctrls = _controls(table)
    assert len(ctrls) == 22 and all(set(v) == {0, 1, K.WAITED} for v in ctrls.values())      # the 14 controls, as the kernels spell them
    stale = {}
    for seed in range(4):
        inp = K.inputs(seed)
        ref = K.reference(table, inp)
        got, _ = _kat_run(lib, inp, 1, 64)
        bad = [c for c in table if not c.negative and not np.array_equal(got[c.index].view(np.uint32), ref[c.index].view(np.uint32))]
        assert not bad, "\n".join(f"{c}: {int(np.sum(got[c.index] != ref[c.index]))} lanes differ; {c.lines}" for c in bad[:20])
        for c in table:
            if c.negative:
                stale[c.index] = stale.get(c.index, 0) + int(np.sum(got[c.index] != ref[c.index]))
    print("fresh DPP source read without wait states, lanes (of 4 x 64) that differ from the waited result:")
    for ctrl, v in ctrls.items():
        print(f"  {ctrl:55s} distance 0: {stale[v[0].index]:3d}   distance 1: {stale[v[1].index]:3d}")
    others = [c for c in table if c.negative and (c.mnemonic != "v_add_f32_dpp" or c.writer != "valu")]
    print("  other negative cases (grid):", ", ".join(f"{c.mnemonic}<-{c.writer}@{c.dist}: {stale[c.index]}" for c in others))
    blind = [ctrl for ctrl, v in ctrls.items() if stale[v[0].index] == 0]
    assert not blind, f"no stale read at distance 0 under {blind}: the positive cases of these controls demonstrate nothing"


@pytest.mark.parametrize("blocks,threads", [(1024, 64), (1024, 512)], ids=["1024-one-wave-groups", "several-waves-per-simd"])
def test_the_answers_do_not_depend_on_occupancy(blocks, threads):
    from hcr_genesis_lr_cl_amd import abi
    from hcr_genesis_lr_cl_amd import dpp_kat as K
    lib = abi.load_lib()
    table = K.cases()
    inp = K.inputs(11)
    ref = K.reference(table, inp)
    _, mis = _kat_run(lib, inp, blocks, threads, expect=ref)
    waves = blocks * threads // 64
    bad = [c for c in table if not c.negative and mis[c.index].sum()]
    assert not bad, "\n".join(f"{c}: {int(mis[c.index].sum())} lane-waves of {waves * 128} differ" for c in bad[:20])
    ctrls = _controls(table)
    print(f"{waves} waves: fresh DPP source, lane-waves (of {waves * 64}) that differ from the waited result:")
    for ctrl, v in ctrls.items():
        print(f"  {ctrl:55s} distance 0: {int(mis[v[0].index, 0].sum()):7d}   distance 1: {int(mis[v[1].index, 0].sum()):7d}")
