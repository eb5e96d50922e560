"""The integer lane constants of the component-per-lane kernels (csrc/lg_lane_ints.h): which env, leg and component a lane works on, its
foot link and foot slot (packed per leg by the host, KParams.k.foot_pack) and the byte offsets of its element in each index pattern of the
state arrays -- formed once per launch and shared by the start-of-kernel loads and every later store to the same arrays.

The header is plain C; it is compiled here on its own (no GPU, no HIP) and every value of every lane of a launch is compared with a
derivation written out in Python from the model description: go2 (4 legs x 3 joints; its foot links do not ascend with the leg),
tron1_pf (2 x 3) and tron1_sf (2 x 4: lane 3 of a quad carries the fourth joint), at N = 1, 6, 64 and 4096 envs (1 and 6 leave dead lanes
that shadow the last env).  The lane table's columns are checked to stay inside the row's used floats."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "hcr_genesis_lr_cl_amd", "csrc")
FIELDS = ("c", "cj", "cjj", "leg", "e", "alive", "ei", "foot_link", "foot_slot", "ja", "o_ja", "o_e", "o_e3", "o_q4", "o_fs", "o_ft", "o_dj", "o_es")

SHIM = r"""
#include "lg_lane_ints.h"
unsigned shim_foot_pack(const int32_t *foot_link, int legs) { return lg_foot_pack(foot_link, legs); }
/* out: (lanes, 18) as 64-bit integers, the fields of LgLaneInts in declaration order */
void shim_lane_ints(int lanes, int n_envs, int legs, int jpl, unsigned pack, long long *out) {
    for (int t = 0; t < lanes; t++) {
        const LgLaneInts r = lg_lane_ints(t, n_envs, legs, jpl, pack);
        long long *o = out + 18 * t;
        o[0] = r.c; o[1] = r.cj; o[2] = r.cjj; o[3] = r.leg; o[4] = r.e; o[5] = r.alive; o[6] = r.ei; o[7] = r.foot_link; o[8] = r.foot_slot;
        o[9] = r.ja; o[10] = r.o_ja; o[11] = r.o_e; o[12] = r.o_e3; o[13] = r.o_q4; o[14] = r.o_fs; o[15] = r.o_ft; o[16] = r.o_dj; o[17] = r.o_es;
    }
}
"""


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    cc = shutil.which("cc") or shutil.which("gcc") or shutil.which("clang")
    if cc is None:
        pytest.fail("no C compiler (cc / gcc / clang) to compile csrc/lg_lane_ints.h with")
    d = tmp_path_factory.mktemp("lane_ints")
    src, lib = d / "shim.c", d / "libshim.so"
    src.write_text(SHIM)
    subprocess.run([cc, "-O1", "-shared", "-fPIC", "-I", CSRC, str(src), "-o", str(lib)], check=True)
    so = C.CDLL(str(lib))
    so.shim_foot_pack.restype = C.c_uint
    so.shim_foot_pack.argtypes = [C.POINTER(C.c_int32), C.c_int]
    so.shim_lane_ints.restype = None
    so.shim_lane_ints.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, C.c_uint, C.POINTER(C.c_longlong)]
    return so


def _model(task):
    from hcr_genesis_lr_cl_amd import builders
    from hcr_genesis_lr_cl_amd.envs import TASKS
    from hcr_genesis_lr_cl_amd.model_compiler import load_model
    cfg = TASKS[task][1]()
    d = builders.make_model_desc(load_model(cfg.asset.name), cfg)
    legs = int(d.n_legs)
    return legs, (int(d.n_bodies) - 1) // legs, [int(x) for x in d.foot_link][:legs]


def _expected(lanes, n, legs, jpl, foot_link):
    """The same quantities, lane by lane, from the layout rules of lg_quad.h: a quad of four lanes per leg, `legs` quads per env."""
    rank = {fl: sorted(foot_link).index(fl) for fl in foot_link}       # foot slot: order of the (N, feet, ...) arrays
    A, rows = jpl * legs, []
    for t in range(lanes):
        c, quad = t % 4, t // 4
        leg, e = quad % legs, quad // legs
        alive = int(e < n)
        e = min(e, n - 1)
        cj = min(c, 2)
        cjj = c if jpl == 4 else cj
        fl = foot_link[leg]
        slot = rank[fl]
        ja = e * A + jpl * leg + cjj
        ei = 4 * leg + c
        rows.append((c, cj, cjj, leg, e, alive, ei, fl, slot, ja, 4 * ja, 4 * e, 4 * (3 * e + cj), 4 * (4 * e + c), 4 * (e * legs + slot),
                     4 * ((e * legs + slot) * 3 + cj), 4 * (jpl * leg + cj), 4 * (ei * n + e)))
    return np.array(rows, np.int64)


@pytest.mark.parametrize("n", [1, 6, 64, 4096])
@pytest.mark.parametrize("task", ["go2", "tron1_pf", "tron1_sf"])
def test_lane_integers_equal_the_derivation_from_the_model(shim, task, n):
    legs, jpl, foot_link = _model(task)
    assert (legs, jpl) == {"go2": (4, 3), "tron1_pf": (2, 3), "tron1_sf": (2, 4)}[task]
    pack = shim.shim_foot_pack((C.c_int32 * 4)(*(foot_link + [-1] * (4 - legs))), legs)
    lanes = ((n * legs * 4 + 63) // 64) * 64                          # whole waves, as the launch: the last one may hold dead lanes
    got = np.zeros((lanes, len(FIELDS)), np.int64)
    shim.shim_lane_ints(lanes, n, legs, jpl, pack, got.ctypes.data_as(C.POINTER(C.c_longlong)))
    want = _expected(lanes, n, legs, jpl, foot_link)
    for k, name in enumerate(FIELDS):
        bad = np.nonzero(got[:, k] != want[:, k])[0]
        assert bad.size == 0, f"{task} N={n} {name}: lane {bad[0]} has {got[bad[0], k]}, derivation {want[bad[0], k]}"
    if n * legs * 4 < lanes:
        assert not got[-1, FIELDS.index("alive")] and got[-1, FIELDS.index("e")] == n - 1      # dead lanes shadow the last env
    # every offset addresses an element inside its array
    A, F = jpl * legs, legs
    for name, size in (("o_ja", n * A), ("o_e", n), ("o_e3", 3 * n), ("o_q4", 4 * n), ("o_fs", n * F), ("o_ft", 3 * n * F), ("o_dj", A), ("o_es", 4 * legs * n)):
        col = got[:, FIELDS.index(name)]
        assert (col % 4 == 0).all() and (col >= 0).all() and (col < 4 * size).all(), name


def test_go2_foot_links_do_not_ascend_with_the_leg():
    """Why the foot constants travel packed per leg instead of being taken as `foot_slot == leg`."""
    legs, _, foot_link = _model("go2")
    assert foot_link != sorted(foot_link) and len(set(foot_link)) == legs and max(foot_link) < 64


def test_lane_table_columns_stay_inside_the_used_floats():
    text = open(os.path.join(CSRC, "lg_shared.h")).read()
    row = int(re.search(r"#define LG_LT_ROW (\d+)", text).group(1))
    body = re.search(r"enum LgLaneCol \{(.*?)\};", text, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    cols = {m.group(1): int(m.group(2)) for m in re.finditer(r"(LT_\w+) = (\d+)", body)}
    used = cols.pop("LT_USED")
    assert used == 72 and row == 84                                   # the stride stays 4 x odd (bank spread), twelve floats spare
    assert len(set(cols.values())) == len(cols) and all(0 <= v < used for v in cols.values())
