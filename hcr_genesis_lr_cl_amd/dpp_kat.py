"""The DPP operand known-answer test's table (csrc/lg_dpp_kat.h) on the host side: the cases parsed from the header text, the inputs, and an
exact reference -- a small interpreter of each case's instruction sequence in which every read sees the value last written (what the chip
computes when no read is stale).  All inputs are small nonzero integers, so every intermediate is exact in f32 and comparisons are bit for
bit."""
import os
import re

import numpy as np

HEADER = os.path.join(os.path.dirname(os.path.abspath(__file__)), "csrc", "lg_dpp_kat.h")
# the asm block lg_host.hip wraps around every case's text
PROLOGUE = ["s_nop 4", "v_mov_b32_e32 %[r], %[s]", "v_mov_b32_e32 %[d], %[o]", "s_nop 4"]
EPILOGUE = ["s_nop 4"]
WAITED = 2          # distance field of the waited reference (`s_nop 1` between write and read)

_CASE = re.compile(r'X\("(\w+)",\s*"(\w+)",\s*(\d+),\s*((?:"(?:[^"\\]|\\.)*"\s*)+)\)')


class Case:
    def __init__(self, index, role, writer, dist, lines):
        self.index, self.role, self.writer, self.dist, self.lines = index, role, writer, dist, lines

    @property
    def reader(self):
        return self.lines[-1]

    @property
    def mnemonic(self):
        return self.reader.split()[0]

    @property
    def control(self):
        return " ".join(t for t in self.reader.split() if ":" in t)

    @property
    def negative(self):
        """A fresh DPP source read without its two wait states: the hardware rule says this one may be stale."""
        return self.role == "dpp_src" and self.dist < WAITED

    def key(self):
        return (self.mnemonic, self.role, self.writer, self.dist, self.control)

    def __repr__(self):
        return f"case {self.index} ({self.mnemonic} {self.role} <- {self.writer} at {self.dist}, {self.control})"


def cases(path=HEADER):
    with open(path) as f:
        text = f.read()
    out = []
    for m in _CASE.finditer(text):
        body = "".join(re.findall(r'"((?:[^"\\]|\\.)*)"', m.group(4)))
        lines = [l.strip() for l in body.replace("\\n", "\n").replace("\\t", "").split("\n") if l.strip()]
        out.append(Case(len(out), m.group(1), m.group(2), int(m.group(3)), lines))
    return out


def inputs(seed=0):
    """5 x 64 f32: x, y (odd integers in [-7, 7]), z (an odd multiple of 1/2 in [-7.5, 7.5]: a sum of it or its products with x, y and an
    integer is never an integer), the sentinel of %[r] and the old value of %[d] (lane-distinct integers, far outside the range of every
    correct result, which tests/test_gpu_dpp_operands.py checks)."""
    rng = np.random.default_rng(seed)
    sign = rng.choice([-1, 1], (3, 64))
    xyz = np.vstack([2 * rng.integers(0, 4, (2, 64)) + 1, rng.integers(0, 8, (1, 64)) + 0.5]) * sign
    lane = np.arange(64)
    sentinel = -(4096 + 64 * lane)
    old = 2048 + 16 * lane
    return np.vstack([xyz, sentinel, old]).astype(np.float32)


def _src_lane(ctrl):
    """-> (source lane of every lane or -1 when out of the row, enabled lanes, bound_ctrl) of a DPP control string."""
    lane = np.arange(64)
    row_pos = lane % 16
    m = re.search(r"quad_perm:\[(\d),(\d),(\d),(\d)\]", ctrl)
    if m:
        perm = np.array([int(g) for g in m.groups()])
        src = (lane & ~3) + perm[lane & 3]
    elif (m := re.search(r"row_shl:(\d+)", ctrl)):
        n = int(m.group(1))
        src = np.where(row_pos + n < 16, lane + n, -1)
    elif (m := re.search(r"row_shr:(\d+)", ctrl)):
        n = int(m.group(1))
        src = np.where(row_pos >= n, lane - n, -1)
    elif (m := re.search(r"row_ror:(\d+)", ctrl)):
        n = int(m.group(1))
        src = lane - row_pos + (row_pos - n) % 16
    else:
        raise ValueError(f"dpp_kat: control not modelled: {ctrl}")
    rm = re.search(r"row_mask:(0x[0-9a-f]+)", ctrl)
    bm = re.search(r"bank_mask:(0x[0-9a-f]+)", ctrl)
    rm = int(rm.group(1), 0) if rm else 0xF
    bm = int(bm.group(1), 0) if bm else 0xF
    enabled = ((rm >> (lane // 16)) & 1).astype(bool) & ((bm >> (row_pos // 4)) & 1).astype(bool)
    return src, enabled, "bound_ctrl" in ctrl


def _operand(tok, regs):
    neg = tok.startswith("-")
    v = regs[tok.lstrip("-")]
    return -v if neg else v


def run_case(case, inp, stale=False):
    """Exact result of one case: {'d': 64 f32, 'r': 64 f32} with every read fresh -- or, `stale`, with the reader seeing %[r] as it was
    before the write under test (what a missing wait state returns; the CPU tests use it to show that every case would notice)."""
    x, y, z, s, o = (a.astype(np.float32) for a in inp)
    regs = {"%[x]": x, "%[y]": y, "%[z]": z, "%[s]": s, "%[o]": o, "%[t]": np.zeros(64, np.float32), "%[d]": None, "%[r]": None}
    seq = PROLOGUE + case.lines + EPILOGUE
    reader_at, before_write = len(PROLOGUE) + len(case.lines) - 1, None
    for i, line in enumerate(seq):
        if i == len(PROLOGUE):
            before_write = regs["%[r]"]
        if stale and i == reader_at:
            regs["%[r]"] = before_write
        toks = line.split()
        mn, ops = toks[0], [t.strip() for t in " ".join(t for t in toks[1:] if ":" not in t).split(",") if t.strip()]
        if mn == "s_nop":
            continue
        dst = ops[0]
        if mn.endswith("_e32"):
            a = [_operand(t, regs) for t in ops[1:]]
            base = mn[:-4]
            res = {"v_mov_b32": lambda: a[0], "v_mul_f32": lambda: a[0] * a[1]}[base]()
            regs[dst] = np.asarray(res, np.float32)
            continue
        if not mn.endswith("_dpp"):
            raise ValueError(f"dpp_kat: instruction not modelled: {line}")
        base = mn[:-4]
        src, enabled, bound = _src_lane(line)
        a0 = _operand(ops[1], regs)
        routed = np.where(src >= 0, a0[np.clip(src, 0, 63)], np.float32(0)).astype(np.float32)
        write = enabled & ((src >= 0) | bound)
        a1 = _operand(ops[2], regs) if len(ops) > 2 else None
        old = regs[dst]
        if base == "v_mov_b32":
            res = routed
        elif base == "v_add_f32":
            res = routed + a1
        elif base == "v_sub_f32":
            res = routed - a1
        elif base == "v_subrev_f32":
            res = a1 - routed
        elif base == "v_mul_f32":
            res = routed * a1
        elif base == "v_fmac_f32":
            res = (routed.astype(np.float64) * a1.astype(np.float64) + old.astype(np.float64)).astype(np.float32)
        else:
            raise ValueError(f"dpp_kat: instruction not modelled: {line}")
        regs[dst] = np.where(write, np.asarray(res, np.float32), old).astype(np.float32)
    return {"d": regs["%[d]"], "r": regs["%[r]"]}


def reference(table, inp):
    """2 N x 64 f32 in the layout of lg_dpp_kat_run's `first` / `expect`: per case %[d] then %[r]."""
    out = np.zeros((len(table), 2, 64), np.float32)
    for c in table:
        res = run_case(c, inp)
        out[c.index, 0], out[c.index, 1] = res["d"], res["r"]
    return out
